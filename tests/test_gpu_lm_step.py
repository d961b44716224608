"""The device LM step (kernels_cost.hpp: dev_lm_step_wave -- the 6x6 LDL^T solve, dev_se3_exp, the accept / reject / convergence machine,
the lambda / nu updates) ALONE, replayed on scripted sums through fvh_debug_lm_replay and held against an exact reference
(tests/lm_ref.py: the solve in fractions, the exponential in 80-digit decimals, the state machine of lsq_registration_impl.hpp:53-168 with
every state value rounded to fp64 once per step). The end-to-end tests hold an align to 1e-4 of the oracle's pose; LM iterates a 1e-7 error of
the step away, and the route-equality tests compare copies of the same function. Inputs: tests/lm_scripts.py (tests/test_lm_ref_cpu.py
checks there that no scripted decision sits within rounding of its threshold).

Tolerances
  (a) se3_exp: K 2^-53 max(1, |v|, |t(x0)|), + theta |v| / 2 below theta = 1e-10 (the reference's own V = R branch, which the device
      copies). K = 22 = 4 x 5.46, where 5.46 is the measured worst error, in that unit, of a plain fp64 numpy transcription of the device's
      half-angle formulas over the same 760 inputs (lm_scripts.measure_se3_K); the factor 4 is for fma contraction and the Newton reciprocal.
  (b) the solve: max |d - d_exact| <= 64 kappa_2(H + lambda I) 2^-53 max |d_exact| -- about three times the textbook constant of a 6x6
      Cholesky-type solve plus one ulp per reciprocal (numpy's solver and a no-pivot fp64 LDL^T stay within 2.1 kappa 2^-53). A DIAGONAL
      system has componentwise condition 1 whatever its kappa_2: there the bound is 64 2^-53 |d_exact| per component, and the 1e-300..1e300
      case is also held to 3 2^-53 (a ~1 ulp reciprocal and one product).
  (c), (d) integers, flags and nu exact; lambda, y0 to 64 2^-53 relative; H, b, final_H bit for bit (copies of the script); d as in (b); poses
      to the bound of (a) times the number of steps taken.
"""
import numpy as np
import pytest

from tests import lm_ref as R
from tests import lm_scripts as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _replay(script, extra_rows=0):
    from fast_gicp_amd import capi
    sums = script["sums"]
    if extra_rows:
        sums = np.vstack([sums, np.repeat(sums[-1:], extra_rows, axis=0)])
    return capi.debug_lm_replay(script["guess"], sums, **script["lm"])


# ---------------------------------------------------------------------------------------------------------------------
# (a) se3_exp over its branches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0_name", ["id", "pose"])
@pytest.mark.parametrize("v_norm", S.V_NORMS)
def test_se3_exp_against_the_exact_exponential(v_norm, x0_name):
    cases = [c for c in S.se3_cases() if c[2] == v_norm and c[0].split("-")[1] == x0_name]
    assert len(cases) == len(S.THETAS) * 5
    worst, bad = 0.0, []
    for name, a, vn, th, x0 in cases:
        rows = _replay(S.se3_script(a, x0))
        assert len(rows) == 1
        r = rows[0]
        assert np.array_equal(r["d"], a), (name, r["d"], a)  # H = I, lambda = 0: the pivots are exactly 1, d = -b bit for bit (the sign of a zero apart)
        assert r["lambda"] == 0.0 and r["phase"] in (R.PH_TRIAL, R.PH_TRIAL_FINAL) and np.array_equal(r["x0"], x0) and np.array_equal(r["x_lin"], x0)
        err = R.max_abs_diff(R.exact_mul(R.exact_exp(a), x0), r["xi"])
        unit = S.se3_unit(a, x0)
        worst = max(worst, (err - S.se3_allowance(a)) / unit)
        if not err <= S.SE3_K * unit + S.se3_allowance(a):
            bad.append((name, err / unit))
        assert np.array_equal(r["xi"][3], [0, 0, 0, 1])
    print("se3_exp |v| = %g, x0 = %s: worst error %.2f units of 2^-53 max(1, |v|, |t(x0)|) (bound %.0f)" % (v_norm, x0_name, worst, S.SE3_K))
    assert not bad, bad


def test_se3_exp_is_closer_to_the_truth_than_the_reference_formula_where_one_minus_cos_cancels():
    """so3.hpp:80-104 (restated in distributed.se3_exp) forms (1 - cos theta) / theta^2, which is 0 for theta < ~1e-8: its translation is off by
    up to theta |v| / 2. The device forms 2 sin^2(theta / 2) / theta^2 and must be better wherever that error dominates rounding."""
    from fast_gicp_amd import distributed
    n = 0
    for name, a, vn, th, x0 in S.se3_cases():
        if not (1e-10 <= th <= 1e-7 and vn >= 1e-3 and name.split("-")[1] == "id"):
            continue
        E = R.exact_exp(a)
        dev = R.max_abs_diff(E, _replay(S.se3_script(a, x0))[0]["xi"])
        ref = R.max_abs_diff(E, distributed.se3_exp(a))
        print("%s: device %.3g, restated reference formula %.3g (theta |v| / 2 = %.3g)" % (name, dev, ref, 0.5 * th * vn))
        assert dev < ref, (name, dev, ref)
        n += 1
    assert n == 2 * 3 * 5  # theta in {1.01e-10, 1e-8} x |v| in {1e-3, 3, 100} x five axes


# ---------------------------------------------------------------------------------------------------------------------
# (b) the solve
# ---------------------------------------------------------------------------------------------------------------------
def test_solve_against_the_exact_solution():
    worst, bad = 0.0, []
    for name, H, b, factor, k2 in S.solve_cases():
        r = _replay(S.solve_script(H, b, factor))[0]
        lam = factor * np.abs(np.diag(H)).max()
        assert r["lambda"] == lam, (name, r["lambda"], lam)  # one rounding
        assert r["H"].tobytes() == H.tobytes() and r["b"].tobytes() == b.tobytes() and r["y0"] == 1.0
        want = R.exact_solve(H, lam, b)
        err = max(abs(float(R.Fraction(float(x)) - w)) for x, w in zip(r["d"], want))
        ratio = err / (k2 * EPS * max(abs(float(w)) for w in want))
        worst = max(worst, ratio)
        if not ratio <= 64:
            bad.append((name, ratio))
    print("solve: worst |d - d_exact| = %.2f kappa 2^-53 max|d_exact| over %d systems (bound 64)" % (worst, len(S.solve_cases())))
    assert not bad, bad


def test_solve_special_systems():
    one = lambda H, b, **lm: _replay(dict(guess=np.eye(4), lm=dict(lm_init_lambda_factor=0.0, **lm), sums=R.pack_sums(1.0, np.asarray(b, float), np.asarray(H, float))[None, :]))[0]
    # H = 0, b = 0 (no correspondences): d = 0, not NaN
    r = one(np.zeros((6, 6)), np.zeros(6))
    assert np.array_equal(r["d"], np.zeros(6)) and np.array_equal(r["xi"], np.eye(4)) and r["lambda"] == 0.0 and r["delta_converged"] == 1 and r["phase"] == R.PH_TRIAL_FINAL
    # zero pivots (Eigen's pseudo-inverse of D): b is zero on the null space -> those components exactly 0, the others exact
    b = np.array([0.25, -0.5, 0.125, 0, 0, 0])
    for lm in (dict(), dict(optimizer=1)):
        r = one(np.diag([1.0, 1.0, 1.0, 0, 0, 0]), b, **lm)
        assert np.array_equal(r["d"], -b), r["d"]
    # a diagonal H from 1e-300 to 1e300: the reciprocal far from 1. Componentwise condition 1: 64 2^-53 per component -- and, sharper, what
    # the kernel promises of fast_rcp: d_i = -b_i * rcp(h_i) is one reciprocal good to ~1 ulp (at most 2 units of 2^-53 relative) and one
    # correctly rounded product (1 unit): 3 units per component
    h = np.array([1e-300, 1e-180, 1e-60, 1e60, 1e180, 1e300])
    c = np.array([0.3, -0.7, 0.11, 1e-3, -2e-3, 0.5e-3])
    b = h * c
    r = one(np.diag(h), b)
    want = R.exact_solve(np.diag(h), 0.0, b)
    rel = [abs(float((R.Fraction(float(x)) - w) / w)) for x, w in zip(r["d"], want)]
    print("diagonal 1e-300 .. 1e300: relative error per component / 2^-53 =", [round(x / EPS, 2) for x in rel])
    assert max(rel) <= 64 * EPS, rel
    assert max(rel) <= 3 * EPS, rel


# ---------------------------------------------------------------------------------------------------------------------
# (c), (d) the state machine
# ---------------------------------------------------------------------------------------------------------------------
def _close(got, want, rel):
    if np.isnan(want) or np.isinf(want) or want == 0.0:
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= rel * abs(want)


def _compare(script, dev, ref):
    name = script["name"]
    assert len(dev) == len(ref), (name, len(dev), len(ref))
    gn = script["lm"].get("optimizer", 0) != 0
    v_max = t_max = 0.0
    worst_pose = worst_d = 0.0
    for k, (g, w) in enumerate(zip(dev, ref)):
        where = "%s step %d" % (name, k)
        for f in R.INT_FIELDS:
            assert g[f] == w[f], (where, f, g[f], w[f])
        assert g["nu"] == w["nu"], (where, g["nu"], w["nu"])
        for f in ("lambda", "y0"):
            assert _close(g[f], w[f], 64 * EPS), (where, f, g[f], w[f])
        for f in ("H", "b", "final_H"):
            assert g[f].tobytes() == w[f].tobytes(), (where, f)
        # d: a step that proposes nothing (the loop ended in a trial) leaves d as it was; otherwise the bound of (b) against the exact
        # solution of this step's (H, lambda, b), and a singular or diagonal system must give the exact (pseudo-inverse) solution
        lam = 0.0 if gn else w["lambda"]
        M = w["H"] + lam * np.eye(6)
        wd = np.abs(np.linalg.eigvalsh(M))
        if w["phase"] == R.PH_DONE and not gn:
            assert g["d"].tobytes() == (dev[k - 1]["d"] if k else np.zeros(6)).tobytes(), (where, g["d"])
        elif np.array_equal(M, np.diag(np.diag(M))) or wd.min() == 0.0:
            assert np.array_equal(g["d"], w["d"]), (where, g["d"], w["d"])
        elif not w["d"].any():
            assert not g["d"].any(), (where, g["d"])
        else:
            want = R.exact_solve(w["H"], lam, w["b"])
            err = max(abs(float(R.Fraction(float(x)) - e)) for x, e in zip(g["d"], want))
            ratio = err / (wd.max() / wd.min() * EPS * max(abs(float(e)) for e in want))
            worst_d = max(worst_d, ratio)
            assert ratio <= 64, (where, "d", ratio)
        v_max = max(v_max, float(np.linalg.norm(w["d"][3:])))
        t_max = max(t_max, *(float(np.linalg.norm(w[f][:3, 3])) for f in ("x0", "xi", "x_lin")))
        unit = EPS * max(1.0, v_max, t_max)
        for f in ("x0", "xi", "x_lin"):
            e = np.abs(g[f] - w[f]).max() / unit
            worst_pose = max(worst_pose, e / (k + 1))
            assert e <= S.SE3_K * (k + 1), (where, f, e)
    print("%s: %d steps, worst pose error / step %.2f units (bound %.0f), worst d %.2f kappa 2^-53 (bound 64)" % (name, len(dev), worst_pose, S.SE3_K, worst_d))


@pytest.mark.parametrize("name", [s["name"] for s in S.state_machine_scripts()])
def test_state_machine_path(name):
    script = [s for s in S.state_machine_scripts() if s["name"] == name][0]
    ref, _ = R.replay(script["guess"], script["sums"], **script["lm"])
    _compare(script, _replay(script), ref)


def test_replay_stops_when_the_state_is_done():
    """rows past the step that ended the loop are never consumed: the same rows come back however many more are scripted"""
    for name in ("reject_until_lm_failed", "accept_converged", "gn_until_converged", "max_iterations_0"):
        script = [s for s in S.state_machine_scripts() if s["name"] == name][0]
        ref, _ = R.replay(script["guess"], script["sums"], **script["lm"])
        _compare(script, _replay(script, extra_rows=5), ref)


@pytest.mark.parametrize("name", S.TRAJ_NAMES + S.TRAJ_CONV_NAMES)
def test_long_trajectory(name):
    script = S.trajectory_script(name)
    ref, _ = R.replay(script["guess"], script["sums"], **script["lm"])
    _compare(script, _replay(script), ref)
