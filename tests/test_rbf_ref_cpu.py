"""The reference side of tests/test_gpu_rbf.py, checked without a GPU: tests/rbf_ref.py against the oracle (two independent statements of
the formula), and the bound the GPU test uses against what fp32 sums of the kernel's shape cost -- it must hold for them, and it must
still see one wrong candidate."""
import functools

import numpy as np
import pytest

from tests import rbf_ref as R

CASES = R.cases()


@functools.lru_cache(maxsize=None)
def _case(name):
    """reference (all queries, with the in-radius pairs), a Morton order, and the fp32 emulation on a sample of the queries"""
    pts, kw, md = CASES[name]
    n = len(pts)
    W, m, C, pairs = R.rbf_reference(pts, kw, md, want_pairs=True)
    order = R.morton_order(pts)
    if n <= 2048:
        queries = np.arange(n)
    else:  # both ends of the order (first tile, ragged last tile) and a random sample
        queries = np.unique(np.concatenate([order[:64], order[-64:], np.random.default_rng(5).choice(n, 400, replace=False)]))
    eW, em, eC = R.rbf_emulate_fp32(pts, kw, md, queries, order)
    counts = np.bincount(pairs[:, 0], minlength=n)
    return dict(pts=pts, kw=kw, md=md, W=W, m=m, C=C, pairs=pairs, counts=counts, order=order, queries=queries, eC=eC)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_oracle(O, name):
    c = _case(name)
    ref = O.covariances_rbf(c["pts"], c["kw"], c["md"], O.NONE)
    scale = np.abs(ref).max(axis=(1, 2))
    assert np.all(np.abs(c["C"] - ref).max(axis=(1, 2)) <= 1e-12 * scale), float((np.abs(c["C"] - ref).max(axis=(1, 2)) / np.maximum(scale, 1e-300)).max())
    assert np.array_equal(c["C"][c["counts"] == 1], np.zeros((int((c["counts"] == 1).sum()), 3, 3)))  # alone inside the radius: exactly 0 on both sides
    assert (c["counts"] >= 1).all()  # every point is its own neighbour (sq == 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_emulation_stays_within_the_bound(name):
    """|emulation - reference|max / (5e-5 (|ref|max + |m|^2) + 1e-12), maximum over the sampled queries (numpy float32, Morton order
    of rbf_ref.morton_order), measured when this test was written:
        size 1, 2: 0 (exact)   63: 0.0012   64: 0.0010   65: 0.0011   130: 0.0014   4095: 0.0015   4096: 0.0014   4097: 0.0014   8191: 0.0012
        params (0.5, 2.5): 0.0014   (0.5, 3.0): 0.0018   (5.0, 0.5): 0.0020   wide radius: 0.0011   offset: 0.0012
        lattice, kw 0.1: md 2 0.0006, below 2 0.0010, md 3 0.0012; kw 0: 0.0006 each
        ragged no limit: kw 0 0.0011, kw 0.5 0.0009      big cloud (test_big_cloud_reference_side): 0.0019
    i.e. errors of 3e-8 .. 1e-7 of (|ref|max + |m|^2): the bound is 500 x wider than the arithmetic needs and is NOT to be tightened
    from a reading of the engine -- 5e-5 is the project's figure for these sums."""
    c = _case(name)
    q = c["queries"]
    ratio = R.rbf_error(c["eC"], c["C"][q]) / R.rbf_bound(c["C"][q], c["m"][q])
    print("%s: emulation uses %.4f of the bound" % (name, ratio.max()))
    assert ratio.max() <= 1.0, float(ratio.max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_still_sees_one_candidate(name):
    """exp(-kernel_width max_dist^2) / W >= 1e-3 = 20 x the tolerance, for every query with at least two neighbours: losing or gaining
    ONE candidate at the radius moves the sums by 20 x what the bound allows. Asserted here so that nobody swaps in a denser cloud that
    blinds the comparison."""
    c = _case(name)
    s = R.sensitivity(c["pts"], c["kw"], c["md"], c["W"], c["counts"])
    print("%s: W max %.1f, neighbours max %d, sensitivity %.2e" % (name, c["W"].max(), c["counts"].max(), s))
    assert s >= 1e-3, s


@pytest.mark.parametrize("name", sorted(n for n in CASES if n not in ("size 1", "size 2")))
def test_mutant_without_one_tile_violates_the_bound(name):
    """The comparison can fail: the hardest query (largest W) loses the tile that holds its FARTHEST neighbour (smallest weight)."""
    c = _case(name)
    pts, q = c["pts"], c["queries"]
    cand = q[c["counts"][q] >= 2]
    assert len(cand)
    victim = int(cand[np.argmax(c["W"][cand])])
    nb = c["pairs"][c["pairs"][:, 0] == victim, 1]
    far = int(nb[np.argmax(((pts[nb].astype(np.float64) - pts[victim]) ** 2).sum(1))])
    tile = int(np.nonzero(c["order"] == far)[0][0]) // 64
    bound = R.rbf_bound(c["C"][[victim]], c["m"][[victim]])[0]
    with np.errstate(all="ignore"):
        _, _, mC = R.rbf_emulate_fp32(pts, c["kw"], c["md"], [victim], c["order"], drop_tile=(victim, tile))
    err = R.rbf_error(mC, c["C"][[victim]])[0]
    assert not err <= bound, (err, bound)  # (a lattice tile can hold ALL the neighbours: W = 0, NaN -- no pass either)
    row = int(np.nonzero(q == victim)[0][0])  # ... and the intact emulation of the same query passes
    assert R.rbf_error(c["eC"][[row]], c["C"][[victim]])[0] <= bound


def test_isolated_case_has_no_neighbours():
    pts, kw, md = R.isolated_case()
    W, m, C, pairs = R.rbf_reference(pts, kw, md, want_pairs=True)
    assert len(pairs) == len(pts) and np.array_equal(W, np.ones(len(pts))) and not C.any() and not m.any()
    _, _, eC = R.rbf_emulate_fp32(pts, kw, md, np.arange(0, len(pts), 8), R.morton_order(pts))
    assert not eC.any()


def test_big_cloud_reference_side():
    """The cloud of more than 64 super boxes: sensitivity and tolerance of the queries the GPU test compares (with the stand-in order)."""
    pts = R.big_cloud()
    order = R.morton_order(pts)
    q = R.big_queries(order)
    W, m, C, pairs = R.rbf_reference(pts, 5.0, 0.5, q, want_pairs=True)
    counts = np.bincount(pairs[:, 0], minlength=len(q))
    s = R.sensitivity(pts, 5.0, 0.5, W, counts)
    _, _, eC = R.rbf_emulate_fp32(pts, 5.0, 0.5, q, order)
    ratio = R.rbf_error(eC, C) / R.rbf_bound(C, m)
    print("big: neighbours mean %.1f max %d, W max %.1f, sensitivity %.2e, emulation uses %.4f of the bound" % (counts.mean(), counts.max(), W.max(), s, ratio.max()))
    assert s >= 1e-3 and ratio.max() <= 1.0
    pos = np.empty(len(pts), np.int64)
    pos[order] = np.arange(len(pts))
    assert (pos[pairs[:, 1]] >= 262144).any()  # a compared query reaches into the second pass of the super-box loop
