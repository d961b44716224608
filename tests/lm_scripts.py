"""The inputs of the LM-step tests, built once and shared: tests/test_gpu_lm_step.py replays them on the device, tests/test_lm_ref_cpu.py
checks (without a GPU) that every state-machine script keeps the margin condition, so that no device comparison is decided by rounding.

A script is a dict {name, guess, lm, sums (n x 32), exempt}: `lm` are the fvh_lm_params fields, `exempt` names the decision kinds the script
is BUILT to sit on ("rho": NaN / zero denominator, "conv": the division branch of the thresholds) -- everything else must keep
|rho| >= 1e-6 and every convergence compare >= 1e-9 (relative) away from its threshold, at every decision of the reference.
"""
import functools

import numpy as np

from tests import lm_ref as R

# ---------------------------------------------------------------------------------------------------------------------
# (a) se3_exp over its branches
# ---------------------------------------------------------------------------------------------------------------------
THETAS = (0.0, 1e-12, 9.9e-11, 1.01e-10, 1e-8, 9.99e-6, 1.001e-5, 1e-3, 0.5, 0.999, 1.0, float(np.nextafter(1.0, 2.0)), 1.5, 3.1, float(np.pi), 3.2, 6.0,
          float(2 * np.pi), 7.0)
V_NORMS = (0.0, 1e-3, 3.0, 100.0)


def _unit(rng):
    u = rng.standard_normal(3)
    return u / np.linalg.norm(u)


def random_pose(rng, t_norm=10.0):
    T = R.to_fp64(R.exact_exp(np.concatenate([_unit(rng) * rng.uniform(0.3, 3.0), _unit(rng) * t_norm])))
    T[3] = (0, 0, 0, 1)
    return T


@functools.lru_cache(maxsize=None)
def se3_cases():
    """[(name, twist a, |v|, theta, x0)]: every theta x {three coordinate axes (theta = 1.0 stays exact), two random axes} x |v| x {identity, a random pose}"""
    rng = np.random.default_rng(20241022)
    x0s = (("id", np.eye(4)), ("pose", random_pose(rng)))
    out = []
    for vn in V_NORMS:
        for xn, x0 in x0s:
            for th in THETAS:
                axes = [np.eye(3)[k] for k in range(3)] + [_unit(rng), _unit(rng)]
                for k, ax in enumerate(axes):
                    a = np.concatenate([ax * th, _unit(rng) * vn])
                    out.append(("v%g-%s-th%r-ax%d" % (vn, xn, th, k), a, vn, th, x0))
    return out


def se3_unit(a, x0):
    """the unit of the (a) tolerance: 2^-53 max(1, |v|, |t(x0)|)"""
    return 2.0 ** -53 * max(1.0, float(np.linalg.norm(a[3:])), float(np.linalg.norm(x0[:3, 3])))


def se3_allowance(a):
    """theta |v| / 2 below theta = 1e-10: the reference's own V = R branch, which the device copies"""
    th = float(np.sqrt(a[:3] @ a[:3]))
    return 0.5 * th * float(np.linalg.norm(a[3:])) if th < 1e-10 else 0.0


def se3_script(a, x0):
    """one LINEARIZE step with H = I, lambda = 0, b = -a: the pivots are exactly 1, d = a bit for bit, xi = exp(a) x0"""
    return dict(guess=x0, lm=dict(lm_init_lambda_factor=0.0), sums=R.pack_sums(1.0, -np.asarray(a), np.eye(6))[None, :])


# The plain fp64 transcription of the half-angle formulas (lm_ref.half_angle_exp_fp64, times x0 in fp64) is off from the 80-digit
# exponential by at most 5.46 units over se3_cases() (measured, tests/test_lm_ref_cpu.py measures it again); the device gets 4 x that for the
# freedom fma contraction and the Newton reciprocal have.
SE3_K_MEASURED = 5.46
SE3_K = 22.0


def measure_se3_K():
    """worst error of the plain fp64 transcription of the half-angle formulas over se3_cases(), in units of se3_unit, past the allowance"""
    worst = 0.0
    for _, a, _, _, x0 in se3_cases():
        got = R.half_angle_exp_fp64(a) @ x0
        err = R.max_abs_diff(R.exact_mul(R.exact_exp(a), x0), got)
        worst = max(worst, (err - se3_allowance(a)) / se3_unit(a, x0))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# (b) the solve
# ---------------------------------------------------------------------------------------------------------------------
KAPPAS = (1.0, 1e3, 1e6, 1e9, 1e12)
SCALES = (1e-6, 1.0, 1e6, 1e12)
FACTORS = (0.0, 1e-9, 1e3)
SOLVE_BOUND_MAX = 1e-3  # a combination whose BOUND (64 kappa 2^-53) exceeds this says nothing: lambda = 0 with kappa = 1e12 only


def spd(rng, kappa, scale):
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    s = scale * np.geomspace(1.0, 1.0 / kappa, 6)
    H = (Q * s) @ Q.T
    return 0.5 * (H + H.T)


def kappa2(M):
    w = np.abs(np.linalg.eigvalsh(M))
    return float(w.max() / w.min())


@functools.lru_cache(maxsize=None)
def solve_cases():
    """[(name, H, b, factor, kappa2(H + lambda I))] over kappa x scale x factor, random b"""
    rng = np.random.default_rng(7)
    out = []
    for kappa in KAPPAS:
        for scale in SCALES:
            for factor in FACTORS:
                H = spd(rng, kappa, scale)
                b = rng.standard_normal(6) * scale
                lam = factor * np.abs(np.diag(H)).max()
                k2 = kappa2(H + lam * np.eye(6))
                if factor == 0.0 and kappa == 1e12:
                    assert 64 * k2 * 2.0 ** -53 > SOLVE_BOUND_MAX  # the one combination the list leaves out, for the reason it states
                    continue
                assert 64 * k2 * 2.0 ** -53 <= SOLVE_BOUND_MAX
                out.append(("k%g-s%g-f%g" % (kappa, scale, factor), H, b, factor, k2))
    return out


def solve_script(H, b, factor):
    return dict(guess=np.eye(4), lm=dict(lm_init_lambda_factor=factor), sums=R.pack_sums(1.0, b, H)[None, :])


# ---------------------------------------------------------------------------------------------------------------------
# (c), (d) scripted trajectories
# ---------------------------------------------------------------------------------------------------------------------
class Builder:
    """Feeds a reference machine one evaluation at a time and keeps the rows of sums it was fed: the trial errors are chosen FROM the
    reference's own predicted decrease so that rho lands on a target."""

    def __init__(self, name, guess=None, exempt=(), **lm):
        self.name, self.guess, self.lm, self.exempt = name, (np.eye(4) if guess is None else guess), lm, tuple(exempt)
        self.m = R.Machine(self.guess, **lm)
        self.sums = []

    @property
    def phase(self):
        return self.m.phase

    def yi_for(self, rho):
        """the trial error that gives the pending trial this rho: y0 - rho * d.(lambda d - b)"""
        m = self.m
        return float(m.y0 - rho * float(m.d @ (m.lam * m.d - m.b)))

    def feed(self, s):
        self.sums.append(np.asarray(s, np.float64).copy())
        self.m.step(s)
        return self

    def linearize(self, lin):
        assert self.phase == R.PH_LINEARIZE
        return self.feed(R.pack_sums(*lin))

    def trial(self, rho, lin, yi=None):
        """a fused trial: trial error at [28], the speculative linearisation `lin` at [0..27]"""
        assert self.phase == R.PH_TRIAL
        return self.feed(R.pack_sums(*lin, trial=self.yi_for(rho) if yi is None else yi))

    def final_trial(self, rho, lin, yi=None):
        """an error-only trial: trial error at [0]; [1..27] carry `lin` (never to be used) and [28] the error that would flip the decision"""
        assert self.phase == R.PH_TRIAL_FINAL
        s = R.pack_sums(*lin, trial=self.yi_for(-rho if rho != 0 else -0.5))
        s[0] = self.yi_for(rho) if yi is None else yi
        return self.feed(s)

    def auto(self, rho, lin):
        return {R.PH_LINEARIZE: lambda: self.linearize(lin), R.PH_TRIAL: lambda: self.trial(rho, lin), R.PH_TRIAL_FINAL: lambda: self.final_trial(rho, lin)}[self.phase]()

    def script(self):
        return dict(name=self.name, guess=self.guess, lm=self.lm, sums=np.array(self.sums).reshape(-1, 32), exempt=self.exempt)


def lin(rng, b_norm=0.2, err=None):
    """a random linearisation (err, b, H): H symmetric positive definite with eigenvalues in [1, 4] (the solve adds next to nothing to the pose
    error), |b| = b_norm: steps of about b_norm / 2"""
    H = spd(rng, 4.0, 4.0)
    b = _unit6(rng) * b_norm
    return (float(rng.uniform(5.0, 50.0)) if err is None else err), b, H


def _unit6(rng):
    u = rng.standard_normal(6)
    return u / np.linalg.norm(u)


SMALL = 1e-5  # |b| of a step below the default thresholds (2e-3, 5e-4)


@functools.lru_cache(maxsize=None)
def state_machine_scripts():
    rng = np.random.default_rng(314159)
    pose = random_pose(rng, 2.0)
    out = []

    def add(b):
        out.append(b.script())

    # accept and continue: corr_cur flips, the speculative sums become H, b, y0; accepts with generic rho (lambda moves through rho). The targets
    # stay away from rho ~ 0.9, where lambda's factor 1 - (2 rho - 1)^3 is small and magnifies the last bits of rho sevenfold
    add(Builder("accept_continue", pose).linearize(lin(rng)).trial(0.6, lin(rng)).trial(0.25, lin(rng)).trial(1.7, lin(rng)).trial(0.7, lin(rng)))
    # reject: lambda nu, 2 nu, H and b unchanged -- the rejected trips carry OTHER linearisations that must not be consumed
    add(Builder("reject_keeps_H_b", pose, lm_init_lambda_factor=1e-2).linearize(lin(rng)).trial(-0.5, lin(rng, 0.4)).trial(-2.0, lin(rng, 0.1)).trial(-0.1, lin(rng))
        .trial(0.7, lin(rng)).trial(-0.3, lin(rng)).trial(0.5, lin(rng)))
    # reject until lm_max_iterations
    add(Builder("reject_until_lm_failed", pose, lm_max_iterations=3, lm_init_lambda_factor=1e-3).linearize(lin(rng)).trial(-0.5, lin(rng)).trial(-0.5, lin(rng)).trial(-0.5, lin(rng)))
    # a converged step, rejected: converged with x0 unchanged (the trial is a final one: error at [0], the flipping error at [28])
    add(Builder("reject_converged", pose).linearize(lin(rng)).trial(0.6, lin(rng, SMALL)).final_trial(-0.5, lin(rng)))
    add(Builder("accept_converged", pose).linearize(lin(rng)).trial(0.6, lin(rng, SMALL)).final_trial(0.6, lin(rng)))
    # the first proposal already converged
    add(Builder("first_step_converged", pose).linearize(lin(rng, SMALL)).final_trial(0.4, lin(rng)))
    # an accept that exhausts max_iterations: the last trial is a final one although its step is far from converged
    add(Builder("accept_exhausts_max_iterations", pose, max_iterations=2).linearize(lin(rng)).trial(0.6, lin(rng)).final_trial(0.6, lin(rng)))
    add(Builder("reject_then_accept_exhausts", pose, max_iterations=1, lm_init_lambda_factor=1e-2).linearize(lin(rng)).final_trial(-0.5, lin(rng)).final_trial(0.3, lin(rng)))
    # final trial: [0] decides, [28] would flip it (both ways; final_trial() puts the flipping error at [28])
    add(Builder("final_reads_0_accept", pose, max_iterations=1).linearize(lin(rng)).final_trial(2.0, lin(rng)))
    add(Builder("final_reads_0_reject", pose, max_iterations=1, lm_max_iterations=1).linearize(lin(rng)).final_trial(-2.0, lin(rng)))
    # plain trial: [28] decides; [0] -- the error of the speculative linearisation, the next y0 -- would flip it if it were read as the trial error
    b = Builder("trial_reads_28_accept", pose).linearize(lin(rng, err=10.0))
    b.trial(0.7, lin(rng, err=1e3))                       # y0 - 1e3 < 0: read from [0] this is a reject
    add(b.trial(0.6, lin(rng)))
    b = Builder("trial_reads_28_reject", pose, lm_init_lambda_factor=1e-2).linearize(lin(rng, err=10.0))
    b.trial(-0.8, lin(rng, err=1.0))                      # y0 - 1 > 0: read from [0] this is an accept
    add(b.trial(0.6, lin(rng)))
    # nothing to do
    b = Builder("max_iterations_0", pose, max_iterations=0)
    b.sums.append(R.pack_sums(*lin(rng)))  # (one row that must not be consumed)
    add(b)
    add(Builder("lm_max_iterations_0", pose, lm_max_iterations=0).linearize(lin(rng)))
    # d = 0 (b = 0): delta = I, the trial is a final one. yi = y0: rho = 0 / 0 = NaN, not < 0: accepted, as IEEE and the reference do
    zero = (7.0, np.zeros(6), spd(rng, 4.0, 4.0))
    add(Builder("d0_rho_nan_accepted", pose, exempt=("rho",)).linearize(zero).final_trial(0.0, lin(rng), yi=7.0))
    add(Builder("d0_yi_above_y0_rejected", pose, exempt=("rho",)).linearize(zero).final_trial(0.0, lin(rng), yi=8.0))   # rho = -1 / 0 = -inf
    add(Builder("d0_yi_below_y0_accepted", pose, exempt=("rho",)).linearize(zero).final_trial(0.0, lin(rng), yi=6.0))   # rho = +inf
    add(Builder("d0_H0_no_correspondences", pose, exempt=("rho",)).linearize((0.0, np.zeros(6), np.zeros((6, 6)))).final_trial(0.0, lin(rng), yi=0.0))
    # final_H after accept-then-done is the H of the ACCEPTED step (the final trial's [1..27] carry another one), after a plain accept too
    add(Builder("final_H_is_the_accepted_H", pose).linearize(lin(rng)).trial(0.6, lin(rng)).trial(0.5, lin(rng, SMALL)).final_trial(0.7, lin(rng)))
    # thresholds that are zero, negative or NaN: the division branch of the convergence test
    nan = float("nan")
    for rn, re_ in (("0", 0.0), ("neg", -1.0), ("nan", nan)):
        for both in (False, True):
            b = Builder("eps_rot_%s%s" % (rn, "_trans_too" if both else ""), pose, exempt=("conv",), rotation_epsilon=re_, transformation_epsilon=re_ if both else 5e-4, max_iterations=5)
            for k, (rho, bn) in enumerate(((0.6, 0.2), (0.6, 0.2), (-0.5, 0.2), (0.6, SMALL), (0.6, SMALL), (-0.5, SMALL), (0.6, 0.2), (0.6, 0.2))):
                if b.phase == R.PH_DONE:
                    break
                b.auto(rho, lin(rng, bn))
            add(b)
    for tn, te in (("0", 0.0), ("neg", -1.0), ("nan", nan)):  # ... and the translation threshold alone
        b = Builder("eps_trans_%s" % tn, pose, exempt=("conv",), transformation_epsilon=te, max_iterations=5)
        for rho, bn in ((0.6, 0.2), (0.6, SMALL), (-0.5, SMALL), (0.6, SMALL), (0.6, 0.2), (0.6, 0.2), (0.6, 0.2)):
            if b.phase == R.PH_DONE:
                break
            b.auto(rho, lin(rng, bn))
        add(b)
    # Gauss-Newton: every step taken, final_H = H, x_lin = the new x0 unless the step ends the loop, converged from the step itself
    add(Builder("gn_until_converged", pose, optimizer=1).linearize(lin(rng)).linearize(lin(rng, 0.05)).linearize(lin(rng, 0.4)).linearize(lin(rng, SMALL)))
    add(Builder("gn_exhausts_max_iterations", pose, optimizer=1, max_iterations=3).linearize(lin(rng)).linearize(lin(rng)).linearize(lin(rng)))
    add(Builder("gn_first_step_converged", pose, optimizer=1).linearize(lin(rng, SMALL)))
    add(Builder("gn_singular_H", pose, optimizer=1, max_iterations=2).linearize((1.0, np.array([0.1, -0.2, 0.05, 0, 0, 0]), np.diag([1.0, 1.0, 1.0, 0, 0, 0]))).linearize(lin(rng)))
    return out


# rho targets of the long trajectories. lambda after an accept is lambda * max(1/3, 1 - (2 rho - 1)^3) and never forgets an error: the
# targets sit where that factor does not feel the last bits of rho -- clamped at 1/3 (rho >= 0.95), stationary (rho = 0.5: the factor
# is 1 to second order) -- plus ONE generic target (0.25: d factor / d rho = 1.3) that a trajectory may take a few times.
TRAJ_ACCEPT = (0.5, 0.5, 0.97, 1.3, 3.0, 0.25)
TRAJ_REJECT = (-0.2, -1.0, -7.0)
TRAJ_STEPS = 40


TRAJ_NAMES = tuple("traj_seed%d_%s" % (seed, opt) for seed in range(20) for opt in ("lm", "gn"))         # 40 evaluations each, never done
TRAJ_CONV_NAMES = tuple("traj_seed%d_%s" % (seed, opt) for seed in range(20, 24) for opt in ("lm", "gn"))  # extra: small steps from 30 on, converge


@functools.lru_cache(maxsize=None)
def trajectory_script(name):
    """Seeds 0..19 x {LM, GN}, 40 evaluations each: random SPD H, random b, a seeded accept / reject pattern (at most three rejects in a row).
    Seeds 20..23 are extra: their steps turn small at evaluation 30 and they converge before the script runs out."""
    seed, gn = int(name.split("_")[1][4:]), int(name.endswith("_gn"))
    rng = np.random.default_rng(1000 + seed)
    b = Builder(name, random_pose(rng, 3.0), optimizer=gn, lm_init_lambda_factor=(1e-9, 1e-3, 0.05)[seed % 3])
    rejects = 0
    for k in range(TRAJ_STEPS):
        if b.phase == R.PH_DONE:
            break
        bn = SMALL if (seed >= 20 and k >= 30) else float(rng.uniform(0.05, 0.5)) * (0.2 if gn else 1.0)
        reject = rng.random() < 0.35 and rejects < 3
        rejects = rejects + 1 if reject else 0
        rho = TRAJ_REJECT[rng.integers(len(TRAJ_REJECT))] if reject else TRAJ_ACCEPT[rng.integers(len(TRAJ_ACCEPT))]
        b.auto(rho, lin(rng, bn))
    return b.script()


def trajectory_scripts():
    return [trajectory_script(n) for n in TRAJ_NAMES + TRAJ_CONV_NAMES]
