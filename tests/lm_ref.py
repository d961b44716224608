"""A plain reference of ONE Levenberg-Marquardt / Gauss-Newton transition (standard library + numpy only), for the tests of the device
LM step (kernels_cost.hpp: dev_lm_step_wave) that replay it on scripted sums (capi.debug_lm_replay).

Three parts:
  exact_solve   (H + lambda I) d = -b in fractions.Fraction built from the exact doubles; a zero pivot has Eigen's pseudo-inverse
                behaviour (that component of the solution is 0).
  exact_exp     the SE(3) exponential in `decimal` at 80 digits, from the power series in theta^2 of sin(t/2)/t, cos(t/2),
                (1 - cos t)/t^2 and (t - sin t)/t^3: no branch on theta. This is the TRUE exponential: so3.hpp:80-104 (restated in
                fast_gicp_amd/distributed.py::se3_exp) is off from it by up to theta |v| / 2 for theta in [1e-10, ~1e-7], where
                1 - cos(theta) rounds to 0.
  replay        LsqRegistration::computeTransformation + step_lm / step_gn (lsq_registration_impl.hpp:53-168) in the fused-trip form of
                the device loop: one call of Machine.step per cost evaluation, fed with the 32 doubles that evaluation reduces to --
                [0..27] = {err, b, H} of the linearisation it computed, [28] = the trial error of a fused trial (a final trial: at [0]).
                Every state value is the exact result of its step rounded to fp64 once. Decisions use IEEE arithmetic on numpy scalars
                (rho = (y0 - yi) / denom may divide by zero; comparisons with NaN are false), and every decision records its MARGIN:
                |rho| for the accept test, |x - eps| / |eps| for each of the twelve convergence compares.
"""
import decimal
from fractions import Fraction

import numpy as np

PH_LINEARIZE, PH_TRIAL, PH_DONE, PH_TRIAL_FINAL = 0, 1, 2, 6
INT_FIELDS = ("phase", "outer_iter", "inner_iter", "converged", "lm_failed", "num_linearize", "num_error_evals", "nr_iterations", "corr_cur", "delta_converged")
_CTX = decimal.Context(prec=80)
D = decimal.Decimal


# ---------------------------------------------------------------------------------------------------------------------
# sums <-> (err, b, H)
# ---------------------------------------------------------------------------------------------------------------------
_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))


def pack_sums(err, b, H, trial=0.0):
    """32 doubles of one evaluation: err, b(6), H rot-rot (6), H rot-trans (9, row-major), H trans-trans (6), trial error, 3 zeros. H must be symmetric."""
    H = np.asarray(H, np.float64)
    assert np.array_equal(H, H.T), "the sums hold one copy of every symmetric pair"
    s = np.zeros(32)
    s[0] = err
    s[1:7] = b
    for i in range(3):
        for j in range(i, 3):
            s[7 + _SYM[i][j]] = H[i, j]
            s[22 + _SYM[i][j]] = H[3 + i, 3 + j]
        for j in range(3):
            s[13 + 3 * i + j] = H[i, 3 + j]
    s[28] = trial
    return s


def unpack_sums(s):
    s = np.asarray(s, np.float64)
    H = np.zeros((6, 6))
    for i in range(3):
        for j in range(3):
            H[i, j] = s[7 + _SYM[i][j]]
            H[3 + i, 3 + j] = s[22 + _SYM[i][j]]
            H[i, 3 + j] = H[3 + j, i] = s[13 + 3 * i + j]
    return float(s[0]), s[1:7].copy(), H


# ---------------------------------------------------------------------------------------------------------------------
# exact solve
# ---------------------------------------------------------------------------------------------------------------------
def exact_solve(H, lam, b):
    """d with (H + lam I) d = -b, as a list of Fractions. LDL^T without pivoting in exact arithmetic; a pivot that is exactly zero leaves its
    column unscaled and contributes the pseudo-inverse of D: 0 (Eigen::LDLT::solve)."""
    A = [[Fraction(float(H[i][j])) + (Fraction(float(lam)) if i == j else 0) for j in range(6)] for i in range(6)]
    L = [[Fraction(0)] * 6 for _ in range(6)]
    Dg = [Fraction(0)] * 6
    for j in range(6):
        Dg[j] = A[j][j] - sum(L[j][k] * L[j][k] * Dg[k] for k in range(j))
        for i in range(j + 1, 6):
            s = A[i][j] - sum(L[i][k] * L[j][k] * Dg[k] for k in range(j))
            L[i][j] = s / Dg[j] if Dg[j] != 0 else s
    y = [Fraction(0)] * 6
    for i in range(6):
        y[i] = -Fraction(float(b[i])) - sum(L[i][k] * y[k] for k in range(i))
    y = [y[i] / Dg[i] if Dg[i] != 0 else Fraction(0) for i in range(6)]
    d = [Fraction(0)] * 6
    for i in range(5, -1, -1):
        d[i] = y[i] - sum(L[k][i] * d[k] for k in range(i + 1, 6))
    return d


def solve_fp64(H, lam, b):
    """exact_solve rounded to fp64 once per component"""
    return np.array([float(x) for x in exact_solve(H, lam, b)])


# ---------------------------------------------------------------------------------------------------------------------
# exact exponential
# ---------------------------------------------------------------------------------------------------------------------
def _series(z, first_den, step):
    """sum_k (-1)^k z^k / den_k with den_0 = first_den and den_{k+1} = den_k * step(k); z >= 0 (Decimal), every series used here converges"""
    with decimal.localcontext(_CTX):
        term = D(1) / D(first_den)
        total, k = D(0), 0
        tiny = D(10) ** -(_CTX.prec + 5)
        while True:
            total += term
            term = -term * z / D(step(k))
            k += 1
            if abs(term) < tiny:
                return total + term


def exact_exp(a):
    """exp of the twist a = (omega, v) as a 4x4 list of Decimals (rotation from the unit quaternion (cos(t/2), sin(t/2)/t omega),
    translation V v with V = I + A Omega + B Omega^2)."""
    with decimal.localcontext(_CTX):
        w = [D(float(x)) for x in a[:3]]
        v = [D(float(x)) for x in a[3:6]]
        z = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]  # theta^2, exact
        imag = _series(z, 2, lambda k: 4 * (2 * k + 2) * (2 * k + 3))   # sin(t/2)/t = sum (-1)^k t^2k / (2^(2k+1) (2k+1)!)
        real = _series(z, 1, lambda k: 4 * (2 * k + 1) * (2 * k + 2))   # cos(t/2)   = sum (-1)^k t^2k / (4^k (2k)!)
        A = _series(z, 2, lambda k: (2 * k + 3) * (2 * k + 4))          # (1 - cos t)/t^2 = sum (-1)^k t^2k / (2k+2)!
        B = _series(z, 6, lambda k: (2 * k + 4) * (2 * k + 5))          # (t - sin t)/t^3 = sum (-1)^k t^2k / (2k+3)!
        qw, qx, qy, qz = real, imag * w[0], imag * w[1], imag * w[2]
        R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
             [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
             [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
        c = [w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]]  # Omega v
        wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2]
        t = [v[i] + A * c[i] + B * (w[i] * wv - z * v[i]) for i in range(3)]                   # Omega^2 v = w (w.v) - t^2 v
        return [R[0] + [t[0]], R[1] + [t[1]], R[2] + [t[2]], [D(0), D(0), D(0), D(1)]]


def exact_mul(E, X):
    """E (Decimals) times the fp64 pose X, in Decimals"""
    with decimal.localcontext(_CTX):
        Xd = [[D(float(X[i][j])) for j in range(4)] for i in range(4)]
        return [[sum((E[i][k] * Xd[k][j] for k in range(4)), D(0)) for j in range(4)] for i in range(4)]


def to_fp64(M):
    return np.array([[float(x) for x in row] for row in M])


def max_abs_diff(M, X):
    """max |X - M| over the upper 3x4, X fp64, M Decimals; the difference is formed in Decimals"""
    with decimal.localcontext(_CTX):
        return float(max(abs(D(float(X[i][j])) - M[i][j]) for i in range(3) for j in range(4)))


def half_angle_exp_fp64(a):
    """The half-angle formulas the device uses (comments of dev_se3_exp), written out in plain fp64 numpy -- no fma, libm's sin / cos,
    IEEE divisions. Its error against exact_exp is the yardstick the GPU tolerance is taken from."""
    a = np.asarray(a, np.float64)
    ox, oy, oz = a[:3]
    v = a[3:]
    th2 = ox * ox + oy * oy + oz * oz
    th = np.sqrt(th2)
    sh, ch = (np.sin(0.5 * th), np.cos(0.5 * th)) if th >= 1e-10 else (0.0, 1.0)
    if th2 < 1e-10:
        imag = 0.5 - 1.0 / 48.0 * th2 + 1.0 / 3840.0 * (th2 * th2)
        real = 1.0 - 1.0 / 8.0 * th2 + 1.0 / 384.0 * (th2 * th2)
    else:
        imag, real = sh / th, ch
    qw, qx, qy, qz = real, imag * ox, imag * oy, imag * oz
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    if th < 1e-10:
        t = R @ v
    else:
        A = 2.0 * sh * sh / th2                       # 1 - cos t = 2 sin^2(t/2)
        B = (th - 2.0 * sh * ch) / (th2 * th)         # sin t = 2 sin(t/2) cos(t/2)
        w = a[:3]
        t = v + A * np.cross(w, v) + B * (w * (w @ v) - th2 * v)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------------------------------------------------------------
# the state machine
# ---------------------------------------------------------------------------------------------------------------------
def is_converged(rot_eps, trans_eps, delta, margins=None):
    """lsq_registration_impl.hpp:82-91 as max(r / rot_eps, t / trans_eps) < 1 on IEEE doubles; max is std::max, (a < b) ? b : a. Records the
    relative distance of each of the twelve entries from its threshold."""
    r = np.abs(delta[:3, :3] - np.eye(3)).reshape(-1)
    t = np.abs(delta[:3, 3])
    if margins is not None:
        with np.errstate(all="ignore"):
            m = [abs(x - np.float64(rot_eps)) / abs(np.float64(rot_eps)) for x in r] + [abs(x - np.float64(trans_eps)) / abs(np.float64(trans_eps)) for x in t]
        margins.append(("conv", float(min(m)) if np.all(np.isfinite(m)) else float("nan")))
    with np.errstate(all="ignore"):
        qr = np.float64(r.max()) / np.float64(rot_eps)
        qt = np.float64(t.max()) / np.float64(trans_eps)
    return bool((qt if qr < qt else qr) < 1)


class Machine:
    """The LM state and one transition per evaluation. `exp` maps a twist to the fp64 4x4 of its exponential (default: the exact one, rounded)."""

    def __init__(self, guess=None, max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, lm_max_iterations=10, lm_init_lambda_factor=1e-9,
                 optimizer=0):
        g = np.eye(4) if guess is None else np.asarray(guess, np.float64).copy()
        self.max_iterations, self.lm_max_iterations, self.gn = int(max_iterations), int(lm_max_iterations), optimizer != 0
        self.rot_eps, self.trans_eps, self.factor = rotation_epsilon, transformation_epsilon, lm_init_lambda_factor
        self.x0, self.xi, self.x_lin = g.copy(), g.copy(), g.copy()
        self.H, self.b, self.d, self.final_H = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.eye(6)
        self.y0, self.lam, self.nu = 0.0, -1.0, 2.0
        self.phase = PH_LINEARIZE if max_iterations > 0 else PH_DONE
        self.outer_iter = self.inner_iter = self.converged = self.lm_failed = self.num_linearize = self.num_error_evals = self.nr_iterations = 0
        self.corr_cur = self.delta_converged = 0
        self.margins = []  # (kind, value) per decision, in order
        self.last_rho = None

    def row(self):
        r = {k: int(getattr(self, k)) for k in INT_FIELDS}
        r.update({"lambda": float(self.lam), "nu": float(self.nu), "y0": float(self.y0), "d": self.d.copy(), "x0": self.x0.copy(), "xi": self.xi.copy(),
                  "x_lin": self.x_lin.copy(), "H": self.H.copy(), "b": self.b.copy(), "final_H": self.final_H.copy()})
        return r

    def step(self, sums):
        assert self.phase != PH_DONE
        s0, bs, Hs = unpack_sums(sums)
        phase0 = self.phase
        accepted = consume = done = False
        x0_new = self.x0
        if phase0 == PH_LINEARIZE:
            consume = True
        else:  # the trial of the step proposed last: step_lm's compute_error(xi), rho, accept / reject (lsq_registration_impl.hpp:139-164)
            yi = np.float64(s0 if phase0 == PH_TRIAL_FINAL else sums[28])
            self.num_error_evals += 1
            lam = np.float64(self.lam)
            with np.errstate(all="ignore"):
                denom = np.float64(self.d @ (lam * self.d - self.b))
                rho = (np.float64(self.y0) - yi) / denom
            self.last_rho = float(rho)
            self.margins.append(("rho", abs(float(rho))))
            conv = self.delta_converged != 0
            if rho < 0:
                if conv:  # step_lm returns true with x0 unchanged; computeTransformation: converged_ = is_converged(delta)
                    self.converged, self.phase, done = 1, PH_DONE, True
                    self.outer_iter += 1
                else:
                    self.lam = float(np.float64(self.nu) * lam)
                    self.nu = 2 * self.nu
                    self.inner_iter += 1
                    if self.inner_iter >= self.lm_max_iterations:  # "lm not converged!!"
                        self.lm_failed, self.phase, done = 1, PH_DONE, True
            else:
                accepted = True
                with np.errstate(all="ignore"):
                    u = 2 * rho - 1
                    f = 1 - u * u * u
                third = np.float64(1.0) / np.float64(3.0)
                self.lam = float(lam * (f if third < f else third))  # std::max(1.0 / 3.0, f)
                x0_new = self.xi
                self.final_H = self.H.copy()
                self.converged = 1 if conv else 0
                self.outer_iter += 1
                if self.converged or self.outer_iter >= self.max_iterations:
                    self.phase, done = PH_DONE, True
                else:  # the speculative linearisation at xi is the next step_lm's linearize()
                    self.corr_cur ^= 1
                    consume = True
        if not done and consume:
            self.y0, self.H, self.b = s0, Hs, bs
            self.num_linearize += 1
            self.nr_iterations = self.outer_iter
            if self.lam < 0.0:
                self.lam = float(np.float64(self.factor) * np.float64(np.abs(np.diag(Hs)).max()))
            self.nu, self.inner_iter = 2.0, 0
            if phase0 == PH_LINEARIZE and not self.gn:
                if self.lm_max_iterations <= 0:
                    self.lm_failed, self.phase, done = 1, PH_DONE, True
                else:
                    self.phase = PH_TRIAL
        self.x0 = x0_new.copy()
        if consume:
            self.x_lin = self.x0.copy()
        if done:
            return self.row()
        d = solve_fp64(self.H, 0.0 if self.gn else self.lam, self.b)
        E = exact_exp(d)
        delta = to_fp64(E)
        xi = to_fp64(exact_mul(E, self.x0))
        xi[3] = (0, 0, 0, 1)
        self.delta_converged = 1 if is_converged(self.rot_eps, self.trans_eps, delta, self.margins) else 0
        self.d, self.xi = d, xi
        if self.gn:  # step_gn: the step is taken at once
            self.converged = self.delta_converged
            self.outer_iter += 1
            self.phase = PH_DONE if (self.converged or self.outer_iter >= self.max_iterations) else PH_LINEARIZE
            self.final_H = self.H.copy()
            if self.phase != PH_DONE:
                self.x_lin = xi.copy()  # where the next trip linearises; a step that ends the loop leaves the stored correspondences at the old x0
            self.x0 = xi.copy()
        else:
            self.phase = PH_TRIAL_FINAL if (self.delta_converged or self.outer_iter + 1 >= self.max_iterations) else PH_TRIAL
        return self.row()


def replay(guess, sums, **lm):
    """The rows capi.debug_lm_replay must produce for the same arguments, and the decision margins: (rows, margins)"""
    m = Machine(guess, **lm)
    if m.phase == PH_DONE:
        return [m.row()], m.margins
    rows = []
    for s in np.asarray(sums, np.float64).reshape(-1, 32):
        rows.append(m.step(s))
        if m.phase == PH_DONE:
            break
    return rows, m.margins


def run_callbacks(linearize, error, guess=None, max_trips=100000, **lm):
    """Drive the machine with a real problem: linearize(T) -> (err, H, b), error(T) -> err. Returns the final Machine."""
    m = Machine(guess, **lm)
    for _ in range(max_trips):
        if m.phase == PH_DONE:
            break
        if m.phase == PH_LINEARIZE:
            e, H, b = linearize(m.x0)
            s = pack_sums(e, b, H)
        elif m.phase == PH_TRIAL:
            e, H, b = linearize(m.xi)
            s = pack_sums(e, b, H, trial=error(m.xi))
        else:
            s = np.zeros(32)
            s[0] = error(m.xi)
        m.step(s)
    return m


def margins_ok(margins, exempt=()):
    """The margin condition of a script: |rho| >= 1e-6 at every accept test, every convergence compare >= 1e-9 (relative) from its threshold.
    `exempt`: the kinds a script is BUILT to sit on ("rho": NaN / zero denominator; "conv": the division branch of the thresholds)."""
    for kind, val in margins:
        if kind in exempt:
            continue
        if not (val >= (1e-6 if kind == "rho" else 1e-9)):
            return False
    return True
