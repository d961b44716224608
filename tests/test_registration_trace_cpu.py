"""The host C++ classes of include/fast_gicp_amd/registration.hpp against a recorded call trace, without a GPU: tests/cpp/registration_trace.cpp
replaces every fvh_* function by a fake that prints its name and arguments, drives FastVGICPCuda, FastGICP, FastVGICP and NDTCuda through
their public methods and prints the getters after each step. tests/golden/registration_trace.txt is that program's output as recorded before
the four classes were put on one device-call layer: which C calls are made, in which order, with which arguments and exception labels is
behaviour, and a line that differs is a behaviour change."""
import os
import subprocess

import pytest

from tests import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "registration_trace.cpp")
GOLDEN = os.path.join(util.ROOT, "tests", "golden", "registration_trace.txt")
CXX = ["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(util.ROOT, "include")]


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "line %d:\n  got      %r\n  expected %r" % (i + 1, a[:300], b[:300])
    return "%d lines, expected %d" % (len(g), len(w))


def test_the_classes_make_the_recorded_calls(tmp_path):
    exe = tmp_path / "registration_trace"
    r = subprocess.run(CXX + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = _run(exe), open(GOLDEN, "rb").read()
    assert got == want, _first_difference(got, want)


def test_the_same_trace_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """host code in a stand-alone binary on the CPU: out-of-bounds reads of the result structs, the neighbour rows or the cloud views would stop it"""
    exe = tmp_path / "registration_trace_san"
    r = subprocess.run(CXX + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ here")
    assert r.returncode == 0, r.stderr
    got, want = _run(exe), open(GOLDEN, "rb").read()
    assert got == want, _first_difference(got, want)
