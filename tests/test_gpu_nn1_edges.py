"""nn1_rows_kernel (the exact nearest target point of every transformed source point: four queries per wave, one per 16-lane row, two box
levels walked nearest first, bounds as truncated float bits, seeded with the id found last time) and fitness_reduce_kernel at their edges,
against tests/nn1_ref.py -- a numpy statement of the definition that shares nothing with the engine or the oracle. Every search goes
through capi.VGICPCore (gicp_update_correspondences, gicp_align, fitness_score), covariances are 0.01 I, ids are compared with
np.array_equal over ALL queries. The premise that makes a cloud an edge case is asserted before the engine is called (and on the CPU in
tests/test_nn1_ref_cpu.py).

  a. every point finds itself (sizes that end rows, tiles and super tiles mid-way; both sort routes), a shifted search, and back
  b. structured clouds: lattice ties, zero-thickness boxes, identical points, quantised distances far from the origin, two clusters,
     queries that are not finite
  c. seeds: whatever the correspondence buffer held before a search must not change its answer (nn1_seed on == off == definition)
  d. the strict < of the correspondence threshold
  e. the fitness reduction: exact sums across its 1,024 / 4,096 strides, the inclusive max_range, 'no point in range'

Fitness tolerance on the clouds of b: the distances are bit-equal, only the fp64 summation order differs. Any order of n non-negative
terms is within (n - 1) 2^-53 (relative) of the exact sum, the reference's fsum within 2^-53, each division within 2^-53:
|fit - ref| <= n 2^-52 ref, derived, not measured."""
import numpy as np
import pytest

from tests import nn1_ref as R
from tests import util

pytestmark = pytest.mark.gpu

I4 = np.eye(4)


def _cov(n):
    return np.tile(np.eye(3) * 0.01, (n, 1, 1))


def _handle(tgt, src, seeded=True):
    from fast_gicp_amd import capi
    c = capi.VGICPCore(0)
    if not seeded:
        c.set_engine_params(nn1_seed=0)
    assert c.get_engine_params().nn1_seed == (1 if seeded else 0)
    c.set_target_cloud(tgt); c.set_target_covariances(_cov(len(tgt)))
    c.set_source_cloud(src); c.set_source_covariances(_cov(len(src)))
    return c


def _search(c, T):
    c.gicp_update_correspondences(T)
    return c.gicp_get_correspondences()


def _assert_ids(got, expect, what):
    bad = np.nonzero(got != expect)[0]
    assert len(got) == len(expect) and np.array_equal(got, expect), (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), np.asarray(expect)[bad[:8]].tolist())


def _assert_fitness(c, T, sq, what, max_range=R.NO_POINT_IN_RANGE):
    fit, ref = c.fitness_score(T, max_range), R.fitness(sq, max_range)
    if ref == R.NO_POINT_IN_RANGE or ref == 0.0:
        assert fit == ref, (what, fit, ref)
    else:
        assert abs(fit - ref) <= len(sq) * 2.0 ** -52 * ref, (what, fit, ref, abs(fit - ref) / ref)


# ---------------------------------------------------------------------------------------------------
# a. every point finds itself
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SELF_SIZES)
def test_every_point_finds_itself_then_a_shifted_search_and_back(n):
    p, first = R.self_cloud(n)
    assert np.array_equal(p[first], p) and (n < 16 or int((first != np.arange(n)).sum()) >= n // 16)
    shift = R.translation((0.37, -0.21, 0.11))
    shifted = R.search(p, p, shift) if n <= R.SELF_BRUTE_FORCE_MAX else None
    c, u = _handle(p, p), _handle(p, p, seeded=False)
    for h, who in ((c, "seeded"), (u, "unseeded")):
        _assert_ids(_search(h, I4), first, (who, "identity"))
        assert h.fitness_score(I4) == 0.0
    got, got_u = _search(c, shift), _search(u, shift)
    _assert_ids(got, got_u, "shifted: seeded against unseeded")
    if shifted is not None:
        _assert_ids(got, shifted[0], "shifted: against the definition")
        _assert_fitness(c, shift, shifted[1], "shifted")
    _assert_ids(_search(c, I4), first, "identity again (seeds: the shifted answers)")
    assert c.fitness_score(I4) == 0.0
    c.close(); u.close()


# ---------------------------------------------------------------------------------------------------
# b. structured clouds
# ---------------------------------------------------------------------------------------------------
def _premise(name, tgt, src, corr, sq):
    """what makes the cloud `name` an edge case, from the definition's answer at the identity"""
    if name == "lattice":
        assert np.all(sq[:4096] == 0) and np.array_equal(tgt[corr[:4096]], src[:4096])
        for j, (kind, ways) in enumerate(R.LATTICE_WAYS.items()):
            s = slice(4096 + j * R.LATTICE_M, 4096 + (j + 1) * R.LATTICE_M)
            assert int((R.tie_count(tgt, src[s], sq[s]) == ways).sum()) >= 1000, kind
    elif name == "plane":
        assert len(tgt) == 4097 and np.all(tgt[:, 2] == np.float32(1.25))
    elif name == "line":
        assert len(tgt) == 4097 and np.all(tgt[:, 1:] == 0)
    elif name == "identical":
        assert len(tgt) == 1000 and np.all(tgt == tgt[0]) and np.all(corr == 0)
    elif name == "offset":
        assert tgt.min() == 4096.0 and np.array_equal(src * 4096, np.rint(src * 4096)) and np.array_equal(tgt[corr], np.rint(src))
    elif name == "clusters":
        assert np.all(corr[:800] % 2 == 0) and np.all(corr[800:1600] % 2 == 1)
        assert np.all(sq[2000:] > 9e11)
    elif name == "bad":
        assert all(corr[i] == -1 and not np.isfinite(sq[i]) for i in R.BAD_ROWS) and all(corr[i] == 7 for i in R.NEG_ZERO_ROWS)
        assert int((corr >= 0).sum()) == len(src) - len(R.BAD_ROWS)


@pytest.mark.parametrize("name", list(R.STRUCTURED))
def test_structured_cloud_equals_the_definition(name):
    tgt, src = R.STRUCTURED[name]()
    poses = (("identity", I4), ("7 deg 0.4 m", R.pose_7deg_04m()))
    refs = [R.search(tgt, src, T) for _, T in poses]
    _premise(name, tgt, src, *refs[0])
    c = _handle(tgt, src)
    for (pname, T), (corr, sq) in zip(poses, refs):
        _assert_ids(_search(c, T), corr, (name, pname))
        _assert_fitness(c, T, sq, (name, pname))
    if name == "bad":
        got = _search(c, poses[1][1])
        assert all(got[i] == -1 for i in R.BAD_ROWS)
    c.close()


# ---------------------------------------------------------------------------------------------------
# c. seeds
# ---------------------------------------------------------------------------------------------------
class _Both:
    """two handles that make the same calls: [0] seeded (the default), [1] with nn1_seed=0. search() holds both to the definition."""

    def __init__(self, tgt, src):
        self.h = (_handle(tgt, src), _handle(tgt, src, seeded=False))
        self.tgt, self.src, self.max_dist = tgt, src, R.MAX_DIST_DEFAULT

    def each(self, fn):
        return [fn(h) for h in self.h]

    def set_target(self, tgt):
        self.tgt = tgt
        self.each(lambda h: (h.set_target_cloud(tgt), h.set_target_covariances(_cov(len(tgt)))))

    def set_source(self, src):
        self.src = src
        self.each(lambda h: (h.set_source_cloud(src), h.set_source_covariances(_cov(len(src)))))

    def set_max_dist(self, d):
        self.max_dist = d
        self.each(lambda h: h.gicp_set_max_correspondence_distance(d))

    def swap(self):
        self.tgt, self.src = self.src, self.tgt
        self.each(lambda h: h.gicp_swap_source_and_target())

    def search(self, T, what):
        expect = R.correspondences(self.tgt, self.src, T, self.max_dist)
        for h, who in zip(self.h, ("seeded", "unseeded")):
            _assert_ids(_search(h, T), expect, (what, who))
        return expect

    def close(self):
        self.each(lambda h: h.close())


FAR = R.rigid([0.1, 0.2, 1.0], 20.0, [2.0, -2.0, 1.0])   # 20 degrees, 3 m


def test_seeds_that_are_valid_but_wrong_then_right_again():
    b = _Both(R.gauss(5000, 41), R.gauss(3000, 42))
    first = b.search(I4, "identity")
    moved = b.search(FAR, "20 deg 3 m (seeds: the identity's)")
    assert int((moved != first).sum()) > 1500          # most seeds were wrong
    assert np.array_equal(b.search(I4, "identity again"), first)
    b.close()


def test_seeds_of_no_correspondence():
    b = _Both(R.gauss(5000, 41), R.gauss(3000, 42))
    b.search(I4, "identity")
    b.set_max_dist(1e-6)
    assert np.all(b.search(I4, "max distance 1e-6") == -1)
    b.set_max_dist(R.MAX_DIST_DEFAULT)
    assert np.all(b.search(FAR, "default distance (seeds: all -1)") >= 0)
    b.close()


def test_stale_seeds_from_a_larger_target():
    b = _Both(R.gauss(5000, 41), R.gauss(3000, 42))
    assert int((b.search(I4, "5,000-point target") >= 80).sum()) >= 1
    b.set_target(R.gauss(80, 43))
    assert b.search(I4, "80-point target (seeds: ids up to 4,999)").max() < 80
    b.search(FAR, "80-point target, moved")
    b.close()


def test_seed_that_is_the_higher_index_twin_of_the_answer():
    A, B, src, P = R.twin_case()
    b = _Both(A, src)
    assert np.all(b.search(I4, "target A") == 900)
    b.set_target(B)                                    # point 5 now lies on point 900: same distance, lower index
    assert np.all(b.search(I4, "target B (seeds: 900, the higher twin)") == 5)
    assert np.all(b.search(I4, "target B again") == 5)
    b.set_target(A)
    assert np.all(b.search(I4, "target A again (seeds: 5, now 1e3 away)") == 900)
    b.close()


def test_seeds_left_by_a_vgicp_align_are_voxel_bucket_ids():
    tgt, src, T = util.synthetic_pair(5000, 3000, seed=7, extent=20.0)
    b = _Both(tgt, src)
    rs = b.each(lambda h: (h.create_target_voxelmap(), h.align(T))[1])
    assert rs[0]["num_linearize"] >= 1 and b.h[0].get_num_correspondences() > 500
    b.search(T, "after a VGICP align")
    b.search(I4, "identity")
    b.close()


def test_seed_buffer_reallocated_for_a_larger_source():
    tgt = R.gauss(5000, 41)
    b = _Both(tgt, R.gauss(100, 44))
    b.search(I4, "100-point source")
    b.set_source(R.gauss(3000, 42))
    b.search(I4, "3,000-point source (a new buffer)")
    b.search(FAR, "3,000-point source, moved")
    b.close()


def test_seeds_across_a_swap_of_source_and_target():
    b = _Both(R.gauss(5000, 41), R.gauss(3000, 42))
    b.search(I4, "before the swap")
    b.swap()
    b.search(I4, "after the swap (seeds: ids of the other direction)")
    b.search(np.linalg.inv(FAR), "after the swap, moved")
    b.swap()
    b.search(I4, "swapped back")
    b.close()


ALIGN_FIELDS = ("T", "H", "final_error", "converged", "nr_iterations", "num_linearize", "num_error_evals")


def _align_both(seeded, unseeded, guess, what):
    r, ru = seeded.gicp_align(guess), unseeded.gicp_align(guess)
    assert r["num_linearize"] >= 2, (what, r)        # at least one LM transition searched from the ids of the one before
    for f in ALIGN_FIELDS:
        assert np.array_equal(np.asarray(r[f]), np.asarray(ru[f])), (what, f, r[f], ru[f])
    _assert_ids(seeded.gicp_get_correspondences(), unseeded.gicp_get_correspondences(), (what, "correspondences left behind"))
    return r


def test_gicp_align_is_the_same_with_and_without_seeds_on_the_bundled_pair():
    from fast_gicp_amd import capi
    tgt, src = util.bundled_pair()
    hs = []
    for seeded in (True, False):
        c = capi.VGICPCore(0)
        if not seeded:
            c.set_engine_params(nn1_seed=0)
        c.set_target_cloud(tgt); c.find_target_neighbors(20); c.calculate_target_covariances()
        c.set_source_cloud(src); c.find_source_neighbors(20); c.calculate_source_covariances()
        hs.append(c)
    assert hs[0].get_engine_params().nn1_seed == 1 and hs[1].get_engine_params().nn1_seed == 0
    guess = R.rigid([0.3, -0.2, 1.0], 5.0, [0.3, -0.3, 0.2645751311064591]) @ util.relative_pose()   # 5 degrees and 0.5 m off
    r = _align_both(hs[0], hs[1], guess, "bundled pair")
    assert r["converged"]
    _align_both(hs[0], hs[1], guess, "bundled pair, again (seeds: the last align's)")
    for h in hs:
        h.close()


def test_gicp_align_is_the_same_with_and_without_seeds_on_the_lattice():
    tgt = R.lattice()
    move = np.array([0.12, -0.12, 0.10583005244258363])   # |move| = 0.2
    src = (R.lattice(seed=98).astype(np.float64) + np.random.default_rng(51).uniform(-0.05, 0.05, size=(4096, 3)) + move).astype(np.float32)
    c, u = _handle(tgt, src), _handle(tgt, src, seeded=False)
    _align_both(c, u, I4, "lattice")
    for h in (c, u):   # and the list an align leaves behind seeds a plain search
        _assert_ids(_search(h, I4), R.correspondences(tgt, src, I4), "lattice: search after the align")
    c.close(); u.close()


# ---------------------------------------------------------------------------------------------------
# d. the threshold
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist, expect", list(zip(R.THRESHOLD_MAX_DISTS, ([-1, 0, -1], [0, 0, -1], [0, 0, 0]))))
def test_correspondence_threshold_is_strict(max_dist, expect):
    """queries at 0.5, one fp32 step below, one above (squared: 0.25, less, more) against max_dist 0.5, one fp64 step above it, float max"""
    tgt, src = R.threshold_case()
    assert R.correspondences(tgt, src, I4, max_dist).tolist() == expect
    for seeded in (True, False):
        c = _handle(tgt, src, seeded)
        c.gicp_set_max_correspondence_distance(max_dist)
        assert _search(c, I4).tolist() == expect, (max_dist, seeded)
        assert _search(c, I4).tolist() == expect, (max_dist, seeded, "again")
        c.close()


# ---------------------------------------------------------------------------------------------------
# e. fitness_reduce_kernel
# ---------------------------------------------------------------------------------------------------
ORIGIN = np.zeros((1, 3), np.float32)


@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_fitness_sum_is_exact_across_the_strides_of_the_reduction(n):
    src, k, mean = R.reduce_case(n)
    sq = R.nearest(ORIGIN, src)[1]
    assert np.array_equal(sq.astype(np.float64), (k * k).astype(np.float64) * 2.0 ** -24)   # the fp32 squares are the fp64 squares
    c = _handle(ORIGIN, src)
    fit = c.fitness_score(I4)
    assert fit == mean == R.fitness(sq), (n, fit, mean)
    c.close()


def test_fitness_max_range_is_inclusive_and_no_point_in_range():
    n = 4097
    src, k, mean = R.reduce_case(n)
    sq = R.nearest(ORIGIN, src)[1]
    assert int((k == 3).sum()) == 2
    at = 9 * 2.0 ** -24                      # the squared distance of the two sources with k = 3
    below = float(np.nextafter(at, 0.0))
    c = _handle(ORIGIN, src)
    assert c.fitness_score(I4, at) == R.fitness(sq, at) == (28 * 2.0 ** -24) / 6          # k = 1, 2, 3, twice each
    assert c.fitness_score(I4, below) == R.fitness(sq, below) == (10 * 2.0 ** -24) / 4    # the count drops by the two sources at k = 3
    assert c.fitness_score(I4, 0.0) == R.fitness(sq, 0.0) == R.NO_POINT_IN_RANGE           # no zero distance
    assert c.fitness_score(I4) == mean
    src0 = src.copy(); src0[0] = 0.0
    c.set_source_cloud(src0); c.set_source_covariances(_cov(n))
    assert c.fitness_score(I4, 0.0) == 0.0                                                 # one point in range, at distance 0
    assert c.fitness_score(I4, at) == (27 * 2.0 ** -24) / 6
    c.close()
