"""The reference of the LM-step tests (tests/lm_ref.py) and their inputs (tests/lm_scripts.py), checked without a GPU: the exact
exponential against scipy's expm, the state machine against the numpy restatement of LsqRegistration (distributed.ShardedLsq), the margin
condition of every script the GPU tests replay, the constant of the se3_exp tolerance, and the binding of fvh_debug_lm_replay."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import lm_ref as R
from tests import lm_scripts as S


def _twist4(a):
    w, v = a[:3], a[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


def test_exact_exponential_agrees_with_expm():
    from scipy.linalg import expm
    n = 0
    for name, a, vn, th, _ in S.se3_cases():
        if th > 3.2:
            continue
        got = R.to_fp64(R.exact_exp(a))
        err = np.abs(got - expm(_twist4(a))).max()
        assert err <= 1e-13 * max(1.0, vn), (name, err)
        n += 1
    assert n >= 300


def test_exact_exponential_is_a_rigid_motion_and_a_group_homomorphism():
    """what expm cannot say at its own 1e-13: R^T R = I to 70 digits, and exp(a) exp(-a) = I"""
    import decimal
    for a in (np.array([0.3, -2.0, 1.1, 5.0, -7.0, 100.0]), np.array([6.5, 1.0, -2.0, 0.1, 0.2, 0.3]), np.array([1e-8, 0, 0, 0, 3.0, 0])):
        with decimal.localcontext(decimal.Context(prec=80)):
            E, Em = R.exact_exp(a), R.exact_exp(-a)
            P = [[sum(E[i][k] * Em[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
            assert max(abs(P[i][j] - (1 if i == j else 0)) for i in range(4) for j in range(4)) < decimal.Decimal(10) ** -70


def test_restated_formula_is_off_by_half_theta_v_where_one_minus_cos_rounds_to_zero():
    """the observation the GPU test pins: so3.hpp:80-104 (distributed.se3_exp) at theta = 1e-8 is 1e-9-ish off for |v| ~ 0.3"""
    from fast_gicp_amd import distributed
    a = np.array([1e-8, 0, 0, 0, 0.26, 0])
    err = R.max_abs_diff(R.exact_exp(a), distributed.se3_exp(a))
    assert 0.9 * 0.5 * 1e-8 * 0.26 <= err <= 1.1 * 0.5 * 1e-8 * 0.26
    assert R.max_abs_diff(R.exact_exp(a), R.half_angle_exp_fp64(a)) < 1e-16  # 2 sin^2(theta / 2) does not cancel


def test_exact_solve():
    rng = np.random.default_rng(3)
    H = S.spd(rng, 1e6, 1.0)
    b = rng.standard_normal(6)
    d = R.exact_solve(H, 0.25, b)
    from fractions import Fraction
    for i in range(6):  # the residual is exactly zero
        assert sum((Fraction(float(H[i, j])) + (Fraction(0.25) if i == j else 0)) * d[j] for j in range(6)) == -Fraction(float(b[i]))
    # a zero pivot: that component of the solution is 0 (pseudo-inverse of D)
    d = R.solve_fp64(np.diag([1.0, 2.0, 4.0, 0, 0, 0]), 0.0, np.array([1.0, 1.0, 1.0, 0, 0, 0]))
    assert np.array_equal(d, [-1.0, -0.5, -0.25, 0, 0, 0])
    assert np.array_equal(R.solve_fp64(np.zeros((6, 6)), 0.0, np.zeros(6)), np.zeros(6))


def test_sums_layout_round_trip():
    rng = np.random.default_rng(4)
    H = S.spd(rng, 10.0, 1.0)
    b = rng.standard_normal(6)
    s = R.pack_sums(3.5, b, H, trial=2.5)
    e, b2, H2 = R.unpack_sums(s)
    assert e == 3.5 and s[28] == 2.5 and np.array_equal(b, b2) and np.array_equal(H, H2) and np.all(s[29:] == 0)
    # the layout of kernels_cost.hpp: rot-rot xx xy xz yy yz zz at 7, rot-trans row-major at 13, trans-trans at 22
    assert s[7] == H[0, 0] and s[8] == H[0, 1] and s[10] == H[1, 1] and s[12] == H[2, 2] and s[13] == H[0, 3] and s[17] == H[1, 4] and s[22] == H[3, 3] and s[27] == H[5, 5]


def _point_problem(seed):
    """point-to-point registration as a least-squares problem in the left perturbation exp(d) T: r_i = T p_i - q_i, J_i = [-skew(T p_i), I]"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-5, 5, (60, 3))
    Tt = S.random_pose(rng, 0.6)
    Q = P @ Tt[:3, :3].T + Tt[:3, 3] + 0.01 * rng.standard_normal(P.shape)

    def lin(T):
        X = P @ T[:3, :3].T + T[:3, 3]
        r = X - Q
        H, b = np.zeros((6, 6)), np.zeros(6)
        for x, ri in zip(X, r):
            J = np.zeros((3, 6))
            J[:, :3] = -np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
            J[:, 3:] = np.eye(3)
            H += J.T @ J
            b += J.T @ ri
        return float((r * r).sum()), 0.5 * (H + H.T), b

    def err(T):
        X = P @ T[:3, :3].T + T[:3, 3]
        return float(((X - Q) ** 2).sum())
    guess = np.eye(4)
    guess[:3, :3] = Tt[:3, :3] @ R.to_fp64(R.exact_exp(np.array([0.2, -0.1, 0.15, 0, 0, 0])))[:3, :3]
    return lin, err, guess


@pytest.mark.parametrize("seed,lm", [(1, {}), (2, dict(lm_init_lambda_factor=10.0)), (3, dict(max_iterations=3)), (4, dict(rotation_epsilon=1e-7, transformation_epsilon=1e-7))])
def test_state_machine_reproduces_the_numpy_restatement(seed, lm):
    from fast_gicp_amd import distributed
    lin, err, guess = _point_problem(seed)
    want = distributed.ShardedLsq(lambda T: lin(T), err, lambda v: v, **lm).align(guess)
    m = R.run_callbacks(lin, err, guess, **lm)
    assert m.phase == R.PH_DONE
    assert bool(m.converged) == bool(want["converged"]) and m.nr_iterations == want["nr_iterations"]
    assert np.abs(m.x0 - want["T"]).max() <= 1e-12
    assert np.abs(m.final_H - want["H"]).max() <= 1e-9 * np.abs(want["H"]).max()
    assert m.num_linearize >= 2 and m.num_error_evals >= m.num_linearize - 1


def test_every_script_keeps_the_margin_condition():
    """|rho| >= 1e-6 at every accept test and every convergence compare >= 1e-9 (relative) from its threshold -- apart from the decision kinds a
    script is built to sit on -- so that no device comparison of tests/test_gpu_lm_step.py can be decided by rounding"""
    scripts = S.state_machine_scripts() + S.trajectory_scripts()
    assert len(S.TRAJ_NAMES) == 40 and len(S.trajectory_scripts()) == 48 and len(set(s["name"] for s in scripts)) == len(scripts)
    decisions = 0
    for s in scripts:
        rows, margins = R.replay(s["guess"], s["sums"], **s["lm"])
        assert R.margins_ok(margins, s["exempt"]), (s["name"], margins)
        assert len(rows) == len(s["sums"]), s["name"]  # nothing is scripted past the end
        decisions += len(margins)
    assert decisions > 2000
    exempt = [s["name"] for s in scripts if s["exempt"]]
    assert all(n.startswith(("d0_", "eps_")) for n in exempt), exempt  # only the cases built to sit on NaN / a zero denominator / the division branch


def test_scripts_reach_every_path():
    rows = {s["name"]: R.replay(s["guess"], s["sums"], **s["lm"])[0] for s in S.state_machine_scripts()}
    last = {k: v[-1] for k, v in rows.items()}
    assert last["reject_until_lm_failed"]["lm_failed"] == 1 and last["reject_until_lm_failed"]["inner_iter"] == 3
    assert last["reject_converged"]["converged"] == 1 and np.array_equal(last["reject_converged"]["x0"], rows["reject_converged"][-2]["x0"])
    assert last["accept_converged"]["converged"] == 1 and np.array_equal(last["accept_converged"]["x0"], rows["accept_converged"][-2]["xi"])
    assert last["accept_exhausts_max_iterations"]["converged"] == 0 and last["accept_exhausts_max_iterations"]["outer_iter"] == 2
    assert last["final_reads_0_accept"]["outer_iter"] == 1 and last["final_reads_0_reject"]["lm_failed"] == 1
    assert [r["corr_cur"] for r in rows["accept_continue"]] == [0, 1, 0, 1, 0]
    r = rows["reject_keeps_H_b"]
    assert np.array_equal(r[1]["H"], r[0]["H"]) and np.array_equal(r[3]["b"], r[0]["b"]) and [x["nu"] for x in r[:4]] == [2.0, 4.0, 8.0, 16.0]
    assert r[1]["lambda"] == 2 * r[0]["lambda"] and r[2]["lambda"] == 8 * r[0]["lambda"] and not np.array_equal(r[4]["H"], r[0]["H"])
    assert last["max_iterations_0"]["phase"] == R.PH_DONE and last["max_iterations_0"]["num_linearize"] == 0
    assert last["lm_max_iterations_0"]["lm_failed"] == 1 and last["lm_max_iterations_0"]["num_linearize"] == 1
    assert last["d0_rho_nan_accepted"]["converged"] == 1 and last["d0_yi_above_y0_rejected"]["converged"] == 1
    f = rows["final_H_is_the_accepted_H"]
    assert np.array_equal(f[-1]["final_H"], f[-2]["H"]) and not np.array_equal(f[-1]["final_H"], f[0]["H"])
    g = rows["gn_until_converged"]
    assert [x["phase"] for x in g] == [0, 0, 0, 2] and g[-1]["converged"] == 1 and np.array_equal(g[1]["x_lin"], g[1]["x0"]) and np.array_equal(g[-1]["x_lin"], g[-2]["x0"])
    assert last["gn_exhausts_max_iterations"]["converged"] == 0 and last["gn_exhausts_max_iterations"]["outer_iter"] == 3
    for n in S.TRAJ_NAMES:  # 20 seeds x {LM, GN}: all 40 evaluations are consumed, none ends early
        sc = S.trajectory_script(n)
        assert len(sc["sums"]) == S.TRAJ_STEPS and R.replay(sc["guess"], sc["sums"], **sc["lm"])[0][-1]["phase"] != R.PH_DONE, n
    for n in S.TRAJ_CONV_NAMES:  # the extra ones end converged
        sc = S.trajectory_script(n)
        assert R.replay(sc["guess"], sc["sums"], **sc["lm"])[0][-1]["converged"] == 1 and 30 < len(sc["sums"]) < S.TRAJ_STEPS, n


def test_se3_tolerance_constant_is_four_times_the_measured_error_of_plain_fp64():
    k = S.measure_se3_K()
    assert abs(k - S.SE3_K_MEASURED) <= 0.15 * S.SE3_K_MEASURED, k  # (libm's last bits may move it a little from machine to machine)
    assert 4 * S.SE3_K_MEASURED <= S.SE3_K <= 4 * S.SE3_K_MEASURED + 1


def test_solve_cases_cover_the_grid_but_for_the_one_meaningless_bound():
    cases = S.solve_cases()
    assert len(cases) == len(S.KAPPAS) * len(S.SCALES) * len(S.FACTORS) - len(S.SCALES)
    assert all(64 * k2 * 2.0 ** -53 <= S.SOLVE_BOUND_MAX for *_, k2 in cases)


def test_replay_binding_matches_the_header_and_refuses_bad_arguments():
    from fast_gicp_amd import build, capi
    hdr = re.sub(r"/\*.*?\*/", "", open(build.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fvh_debug_lm_replay\s*\(([^)]*)\)\s*;", hdr)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(capi.LM_REPLAY_ARGTYPES) == 7
    for p, t in zip(params, capi.LM_REPLAY_ARGTYPES):
        assert t is (C.c_void_p if "*" in p else C.c_int), (p, t)
    assert int(re.search(r"#define\s+FVH_LM_REPLAY_ROW\s+(\d+)", hdr).group(1)) == capi.LM_REPLAY_ROW == 13 + 6 + 3 * 12 + 36 + 6 + 36
    assert "fvh_debug_lm_replay" in capi.declared_symbols()
    assert (capi.PH_LINEARIZE, capi.PH_TRIAL, capi.PH_DONE, capi.PH_TRIAL_FINAL) == (R.PH_LINEARIZE, R.PH_TRIAL, R.PH_DONE, R.PH_TRIAL_FINAL)
    assert capi.LM_REPLAY_INTS == R.INT_FIELDS
    # the argument checks come before the device is touched: they answer on a machine without one
    fn = capi.load().fvh_debug_lm_replay
    g = np.ascontiguousarray(np.eye(4))
    p = capi._lm_params()
    sums = np.zeros((300, 32))
    rows = np.zeros((300, capi.LM_REPLAY_ROW))
    n = C.c_int(0)
    ok = (0, capi._p(g), C.byref(p), 1, capi._p(sums), capi._p(rows), C.byref(n))
    for i in (1, 2, 4, 5, 6):
        args = list(ok)
        args[i] = None
        assert fn(*args) == 1, i
    for steps in (0, -1, 257):
        args = list(ok)
        args[3] = steps
        assert fn(*args) == 1, steps
    for bad in (np.nan, np.inf):
        gb = g.copy()
        gb[2, 1] = bad
        args = list(ok)
        args[1] = capi._p(gb)
        assert fn(*args) == 1
    with pytest.raises(capi.FvhError):
        capi.debug_lm_replay(np.eye(4), np.zeros((2, 31)))
    # a row of the result, taken apart
    row = np.arange(float(capi.LM_REPLAY_ROW))
    d = capi.lm_replay_row(row)
    assert d["phase"] == 0 and d["delta_converged"] == 9 and d["lambda"] == 10 and d["y0"] == 12 and list(d["d"]) == [13, 14, 15, 16, 17, 18]
    assert d["x0"][0, 1] == 20 and d["x0"][0, 3] == 28 and d["xi"][2, 2] == 39 and d["x_lin"][2, 3] == 54 and d["H"][0, 0] == 55 and d["b"][5] == 96 and d["final_H"][5, 5] == 132
