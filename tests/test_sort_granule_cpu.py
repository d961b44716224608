"""The granule the cooperative small sort's workgroups exchange their digit counts in (fast_gicp_amd/csrc/sort_granule.hpp: four 11-bit
counts under one 20-bit launch-and-pass tag in 8 bytes) packs and unpacks exactly -- checked on the host by a stand-alone program that
compiles the very functions the kernel uses: every count 0 ... 1,024 in every slot, every tag bit, the tags around the points where they
repeat and the skipped sequence numbers."""
import os
import subprocess

from tests import util


def test_granule_pack_and_unpack_round_trip(tmp_path):
    exe = str(tmp_path / "sort_granule_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(util.ROOT, "fast_gicp_amd", "csrc"),
                           os.path.join(util.ROOT, "tests", "cpp", "sort_granule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, out.stdout
    assert out.stdout.startswith("%d granules checked, 0 mismatches" % (4 * 1025 * 5 * 6))
