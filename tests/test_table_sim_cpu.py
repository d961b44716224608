"""The voxel key and its hash (fast_gicp_amd/csrc/voxel_key.hpp) on the host: a stand-alone program compiles the very functions the
kernels use, checks the pack / unpack round trip, the 21-bit range and voxel_index_ok at its limit, for NaN and for inf, and prints key
and home slot of a fixed coordinate list at three capacities; tests/table_sim.py -- the numpy restatement the GPU tests size their crowded
tables with -- must give the same numbers. The two simulations built on the restatement are checked on cases small enough to do by hand."""
import os
import subprocess

import numpy as np
import pytest

from tests import table_sim, util


@pytest.fixture(scope="module")
def program_rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxel_key") / "voxel_key_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(util.ROOT, "fast_gicp_amd", "csrc"),
                           os.path.join(util.ROOT, "tests", "cpp", "voxel_key_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, out.stdout[-2000:]
    lines = out.stdout.splitlines()
    rows = np.array([[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("K ")], dtype=object)
    assert lines[-1] == "%d coordinates checked, 0 mismatches" % len(rows)
    return rows


def test_numpy_key_and_slot_equal_the_header(program_rows):
    rows = program_rows
    coords = rows[:, :3].astype(np.int64)
    assert len(rows) >= 4000
    big = (1 << 20) - 4097
    have = set(map(tuple, coords.tolist()))
    for c in [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (big, 0, 0), (-big, 0, 0), (0, -big, 0), (0, 0, -big), (big, big, big), (-big, -big, -big)]:
        assert c in have, c
    assert big == table_sim.COORD_LIMIT - 1
    keys = table_sim.pack_key(coords)
    assert np.array_equal(keys, rows[:, 3].astype(np.uint64))
    assert len(np.unique(keys)) == len(have)  # distinct coordinates, distinct keys
    for col, cap in ((4, 1024), (5, 8192), (6, 65536)):
        assert np.array_equal(table_sim.hash_slot(keys, cap), rows[:, col].astype(np.int64)), cap
    assert np.array_equal(table_sim.hash_slot(keys, 1), np.zeros(len(keys), np.int64))


def _coords_with_home(slots, capacity, start=0):
    """distinct voxel coordinates whose home slots at `capacity` are `slots`, in that order (searched along x)"""
    out, x = [], start
    for s in slots:
        while int(table_sim.hash_slot(table_sim.pack_key([[x, 0, 0]]), capacity)[0]) != s:
            x += 1
        out.append((x, 0, 0))
        x += 1
    return np.array(out)


def test_fill_table_counts_displacement_runs_and_the_wrap():
    cap = 16
    # three keys on slot 14: they take 14, 15 and 0 -- a run of three across the end of the table; one key alone on slot 5
    c = _coords_with_home([14, 14, 14, 5], cap)
    f = table_sim.fill_table(c, cap)
    assert f == dict(voxels=4, load=0.25, displaced=2, longest_run=3, wraps=True, across_end=1, max_displacement=2)
    # duplicates are one voxel; a run that ends AT the last slot does not cross it
    c = _coords_with_home([14, 14, 5], cap)
    f = table_sim.fill_table(np.concatenate([c, c]), cap)
    assert f == dict(voxels=3, load=3 / 16, displaced=1, longest_run=2, wraps=False, across_end=0, max_displacement=1)
    # a run that touches both ends of the table without any key pushed across: homes 15 and 0
    f = table_sim.fill_table(_coords_with_home([15, 0], cap), cap)
    assert (f["displaced"], f["longest_run"], f["wraps"], f["across_end"]) == (0, 2, True, 0)
    # a key pushed behind another key's home run: homes 3, 3, 4 -> slots 3, 4, 5
    f = table_sim.fill_table(_coords_with_home([3, 3, 4], cap), cap)
    assert (f["displaced"], f["longest_run"], f["wraps"], f["max_displacement"]) == (2, 3, False, 1)


def test_lds_spills_counts_the_points_past_eight_probes():
    # ten voxels on one LDS slot: eight find a slot within 8 probes, two spill; the same point again is staged where it already sits
    c = _coords_with_home([100] * 10, table_sim.LDS_SLOTS)
    assert table_sim.lds_spills(c) == 2
    assert table_sim.lds_spills(np.concatenate([c[:8], c[:8], c[:8]])) == 0
    assert table_sim.lds_spills(np.concatenate([c, c[8:]])) == 4  # a spilled voxel spills every time
    # the run wraps in the LDS table too: slots 510, 511, 0, ...
    assert table_sim.lds_spills(_coords_with_home([510] * 9, table_sim.LDS_SLOTS)) == 1
    # every workgroup of 256 points starts with an empty table: 250 fillers, then the ten in the NEXT block's first slots
    filler = np.stack([np.arange(250), np.full(250, 7), np.full(250, 7)], axis=1)
    pts = np.concatenate([filler, c[:6], c[6:]])  # block 0: 250 fillers + 6; block 1: the other 4
    assert table_sim.lds_spills(pts) == table_sim.lds_spills(np.concatenate([filler, c[:6]]))
