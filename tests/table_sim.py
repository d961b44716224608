"""Numpy restatement of the voxel key and its table placement (fast_gicp_amd/csrc/voxel_key.hpp: pack_key, hash_key, hash_slot -- held to
the C++ functions themselves by tests/test_table_sim_cpu.py) and two simulations built on it (test infrastructure only):

  fill_table     linear-probe insertion of a set of voxels into a table of a given capacity, as global_claim_from (kernels_voxelmap.hpp)
                 does it. The device inserts in another order, but WHICH slots end up occupied does not depend on the order (every key
                 takes the first free slot of its run), so load, the longest occupied run -- the bound on any probe -- and whether a run
                 crosses the end of the table are the device's.
  lds_spills     the 512-slot, 8-probe LDS stage of vm_accumulate_kernel, replayed per workgroup of 256 points in input order: points whose
                 key finds no slot go straight to the global table ("visitors").
"""
import numpy as np

COORD_BIAS = 1 << 20
COORD_LIMIT = COORD_BIAS - 4096      # voxel_index_ok: |index| < COORD_LIMIT
MAX_PROBE = 255                      # VM_MAX_PROBE: a key may sit at most this far from its home slot
LDS_SLOTS, LDS_PROBES, BLOCK = 512, 8, 256


def pack_key(coords):
    """(n, 3) integer voxel coordinates -> uint64 keys: 21 bits per axis, biased by 2^20"""
    c = (np.asarray(coords, np.int64).reshape(-1, 3) + COORD_BIAS).astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


def hash_key(keys):
    k = np.asarray(keys, np.uint64)
    lo, hi = k & np.uint64(0xFFFFFFFF), k >> np.uint64(32)
    return ((lo * np.uint64(0x9E3779B1) + hi * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # (uint64 arithmetic wraps at 2^64: the low 32 bits are exact)


def hash_slot(keys, capacity):
    """home slot: the top log2(capacity) bits of the 32-bit hash; capacity a power of two"""
    assert capacity >= 1 and capacity & (capacity - 1) == 0
    bits = capacity.bit_length() - 1
    h = hash_key(keys)
    return (h >> np.uint32(32 - bits)).astype(np.int64) if bits else np.zeros(len(h), np.int64)


def voxel_coords(xyz, res):
    """floor(p / res - 0.5) in fp64, as the build and the lookups compute it"""
    return np.floor(np.asarray(xyz, np.float32).astype(np.float64) / res - 0.5).astype(np.int64)


def fill_table(coords, capacity):
    """Insert the DISTINCT voxels among `coords` by linear probing. -> dict(voxels, load, displaced, longest_run, wraps, across_end, max_displacement)"""
    keys = np.unique(pack_key(coords))
    assert len(keys) < capacity
    occupied = np.zeros(capacity, bool)
    displaced = max_disp = 0
    home = hash_slot(keys, capacity)
    for s in home.tolist():
        d = 0
        while occupied[(s + d) & (capacity - 1)]:
            d += 1
        occupied[(s + d) & (capacity - 1)] = True
        displaced += d > 0
        max_disp = max(max_disp, d)
    # circular runs of occupied slots: start the walk behind a free slot
    free = np.flatnonzero(~occupied)
    rolled = np.roll(occupied, -(int(free[0]) + 1))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], rolled.astype(np.int8), [0]])))
    runs = edges[1::2] - edges[0::2]
    wraps = bool(occupied[0] and occupied[capacity - 1])
    # keys that sit PAST the end of the table whatever the insertion order: the run that crosses the end starts behind a free slot, so it holds
    # exactly the keys whose home is at or behind its start -- those that do not fit in front of the end are found by a probe that wraps
    start = capacity - 1 - int(np.argmin(occupied[::-1])) + 1 if wraps else capacity
    across = max(0, int((home >= start).sum()) - (capacity - start))
    return dict(voxels=len(keys), load=len(keys) / capacity, displaced=int(displaced), longest_run=int(runs.max()) if len(runs) else 0,
                wraps=wraps, across_end=across, max_displacement=int(max_disp))


def lds_spills(coords):
    """Points (voxel coordinate per point, input order) that leave the LDS stage of their 256-point workgroup without a slot."""
    keys = pack_key(coords)
    home = hash_slot(keys, LDS_SLOTS)
    spills = 0
    for lo in range(0, len(keys), BLOCK):
        table = {}
        for k, s in zip(keys[lo:lo + BLOCK].tolist(), home[lo:lo + BLOCK].tolist()):
            for pr in range(LDS_PROBES):
                held = table.setdefault((s + pr) & (LDS_SLOTS - 1), k)
                if held == k:
                    break
            else:
                spills += 1
    return spills
