"""tests/nn1_ref.py pinned on the CPU: the numpy definition of the exact nearest-point search against the oracle's kd-tree query (ids and
fp32 distances EQUAL), its tie rule, its fitness mean, and the premises of the GPU edge suite (tests/test_gpu_nn1_edges.py) -- each cloud
there is checked here to be the edge case it claims to be, so that a test on it cannot pass quietly."""
import math

import numpy as np
import pytest

from tests import nn1_ref as R


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _same_as_oracle(O, tgt, q):
    idx, sq = R.nearest(tgt, q)
    oi, osq = O.knn_query(tgt, q, 1)
    assert np.array_equal(idx, oi[:, 0]) and np.array_equal(sq.view(np.uint32), osq[:, 0].view(np.uint32))
    return idx, sq


def test_nearest_equals_the_oracle_query_on_a_random_cloud(O):
    tgt, src = R.gauss(12289, 1), R.gauss(4097, 2)
    _same_as_oracle(O, tgt, R.transform_f32(src, R.pose_7deg_04m()))


def test_nearest_equals_the_oracle_query_on_duplicated_points(O):
    tgt = R.gauss(4096, 3)
    tgt[2048:2048 + 500] = tgt[100:600]
    q = np.concatenate([tgt[100:600], R.gauss(1000, 4)])
    idx, sq = _same_as_oracle(O, tgt, q)
    assert np.array_equal(idx[:500], np.arange(100, 600)) and np.all(sq[:500] == 0)


def test_nearest_equals_the_oracle_query_on_the_lattice_and_ties_are_many(O):
    tgt = R.lattice()
    qs = R.lattice_queries()
    idx, sq = _same_as_oracle(O, tgt, qs["points"])
    assert np.all(sq == 0) and np.array_equal(tgt[idx], qs["points"])
    for kind, ways in R.LATTICE_WAYS.items():
        idx, sq = _same_as_oracle(O, tgt, qs[kind])
        ties = R.tie_count(tgt, qs[kind], sq)
        assert int((ties == ways).sum()) >= 1000, (kind, int((ties == ways).sum()))
        assert np.all(sq == {8: 0.75, 4: 0.5, 2: 0.25}[ways])
        # the winner is the LOWEST index among the tied points
        d = R._sqdist_block(tgt, qs[kind])
        assert np.array_equal(idx, np.argmax(d == sq[:, None], axis=1))


def test_tie_rule_lowest_original_index_wins():
    tgt = np.array([[9, 9, 9], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    idx, sq = R.nearest(tgt, np.zeros((1, 3), np.float32))
    assert idx[0] == 1 and sq[0] == 1.0
    idx, sq = R.nearest(tgt[::-1].copy(), np.zeros((1, 3), np.float32))
    assert idx[0] == 0
    assert R.nearest(tgt, np.array([[1, 0, 0]], np.float32))[0][0] == 1


def test_transform_is_the_fp32_association_of_the_kernel():
    T = R.pose_7deg_04m()
    s = R.gauss(100, 5)
    Tf = T.astype(np.float32)
    q = R.transform_f32(s, T)
    for i in (0, 57, 99):
        for r in range(3):
            a = np.float32(np.float32(s[i, 0] * Tf[r, 0]) + np.float32(s[i, 1] * Tf[r, 1]))
            b = np.float32(np.float32(s[i, 2] * Tf[r, 2]) + Tf[r, 3])
            assert q[i, r] == np.float32(a + b)
    assert q.dtype == np.float32 and np.array_equal(R.transform_f32(s, np.eye(4)), s)
    assert abs(np.linalg.norm(T[:3, 3]) - 0.4) < 1e-12 and abs(np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2)) - 7.0) < 1e-9


def test_non_finite_queries_and_the_fitness_mean():
    tgt, src = R.bad_case()
    for T in (np.eye(4), R.pose_7deg_04m()):
        corr, sq = R.search(tgt, src, T)
        for i in R.BAD_ROWS:
            assert corr[i] == -1 and not np.isfinite(sq[i])
        good = np.ones(len(src), bool); good[list(R.BAD_ROWS)] = False
        assert np.all(corr[good] >= 0) and np.all(np.isfinite(sq[good]))
        assert R.fitness(sq) == math.fsum(sq[good].astype(np.float64).tolist()) / int(good.sum())
    corr, sq = R.search(tgt, src, np.eye(4))
    assert all(corr[i] == 7 and sq[i] == 0 for i in R.NEG_ZERO_ROWS)        # -0.0 is the origin: target point 7
    assert R.fitness(np.array([1.0, 2.0, 4.0], np.float32), 2.0) == 1.5      # inclusive
    assert R.fitness(np.array([1.0, 2.0, 4.0], np.float32), float(np.nextafter(2.0, 0.0))) == 1.0
    assert R.fitness(np.array([1.0], np.float32), 0.0) == R.NO_POINT_IN_RANGE
    assert R.fitness(np.array([0.0, 1.0], np.float32), 0.0) == 0.0
    assert R.fitness(np.array([np.nan, np.inf], np.float32)) == R.NO_POINT_IN_RANGE


def test_correspondence_threshold_is_strict_and_clamped():
    tgt, src = R.threshold_case()
    at, below, above = 0, 1, 2
    assert src[below, 0] < src[at, 0] < src[above, 0]
    got = {md: R.correspondences(tgt, src, np.eye(4), md).tolist() for md in R.THRESHOLD_MAX_DISTS}
    assert got[0.5] == [-1, 0, -1]                      # 0.25 < 0.25 is false
    assert got[R.THRESHOLD_MAX_DISTS[1]] == [0, 0, -1]  # one fp64 step above 0.5 lets 0.25 in, not the next fp32 distance
    assert got[R.MAX_DIST_DEFAULT] == [0, 0, 0]         # (threshold^2 clamped: finite)


def test_premises_of_the_structured_clouds():
    for n in R.SELF_SIZES:
        p, first = R.self_cloud(n)
        assert len(p) == n and np.all(first <= np.arange(n)) and np.array_equal(p[first], p) and not np.any(np.signbit(p) & (p == 0))
        assert int((first != np.arange(n)).sum()) >= n // 16   # duplicates at every size from 16 up
        if n >= 64:
            assert int((p == np.rint(p)).all(axis=1).sum()) >= n // 8 - n // 16
    tgt, src = R.plane_case()
    assert len(tgt) == 4097 and np.all(tgt[:, 2] == np.float32(1.25))
    tgt, src = R.line_case()
    assert len(tgt) == 4097 and np.all(tgt[:, 1:] == 0)
    tgt, src = R.identical_case()
    assert len(tgt) == 1000 and np.all(tgt == tgt[0]) and np.all(R.nearest(tgt, src)[0] == 0)
    tgt, src = R.offset_case()
    assert tgt.min() == 4096.0 and np.spacing(np.float32(4096.0)) == np.float32(2.0 ** -11)
    assert np.array_equal(src * 4096, np.rint(src * 4096)) and np.abs(src - np.rint(src)).max() > 0.29   # the jitter survives only in steps of 2^-11 (2^-12 below 4,096)
    assert np.array_equal(tgt[R.nearest(tgt, src)[0]], np.rint(src))
    tgt, src = R.clusters_case()
    assert len(tgt) == 4097
    idx, sq = R.nearest(tgt, src)
    assert np.all(idx[:800] % 2 == 0) and np.all(idx[800:1600] % 2 == 1) and len(set((idx[1600:2000] % 2).tolist())) == 2
    assert np.all(sq[2000:] > 9e11)   # at 1e6: 64 / 256 truncated ulps of a bound are 4e6 / 1.7e7 -- the boxes of a cluster differ by less


def test_premises_of_the_seed_cases():
    A, B, src, P = R.twin_case()
    assert np.all(R.correspondences(A, src, np.eye(4)) == 900) and np.all(R.correspondences(B, src, np.eye(4)) == 5)
    assert np.array_equal(B[5], B[900]) and np.array_equal(A[900], P) and np.all(R.nearest(B, src)[1][:8] == 0) and np.all(R.nearest(B, src)[1][8:] > 0)
    tgt, src = R.gauss(5000, 41), R.gauss(3000, 42)
    assert np.all(R.correspondences(tgt, src, np.eye(4), 1e-6) == -1)
    assert int((R.correspondences(tgt, src, np.eye(4)) >= 80).sum()) >= 1


@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_premises_of_the_exact_sum_cases(n):
    src, k, mean = R.reduce_case(n)
    idx, sq = R.nearest(np.zeros((1, 3), np.float32), src)
    exact = (k * k).astype(np.float64) * 2.0 ** -24
    assert np.array_equal(sq.astype(np.float64), exact)                       # the fp32 squares ARE the fp64 squares
    assert np.array_equal(np.cumsum(exact), np.cumsum((k * k)) * 2.0 ** -24)  # every partial sum is an integer multiple of 2^-24 below 2^53: exact
    assert R.fitness(sq) == mean
