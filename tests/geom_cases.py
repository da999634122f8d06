"""Inputs, references, bounds and mutants for the camera models and the SE3 / Sim3 maps run alone through orbx_debug_geometry
(tests/test_geometry_device.py).  Nothing in this file comes from a device result.

Every function of the headers is restated ONCE as an expression tree in the header's operation order (the functions named like
the header's).  The tree is evaluated by two arithmetics:

* numpy scalars of the function's own format (float32 / float64): the *restatement*.  For the exact operations (only + - * / and
  sqrt, all correctly rounded, no contraction) it must equal the device bit for bit.  float32 libm calls are the float64 ones
  rounded once, which is what a correctly rounded float libm returns up to double rounding.
* `E`, a value of mpmath (200 bits) with a first-order forward error bound: the *reference* and its *bound*.  An arithmetic
  operation adds half an ulp of its result in the function's format (2^-24 or 2^-53, plus half the smallest denormal), nothing
  when its operands are exact and its result is representable; a libm call adds its budget in ulps.  Cancellation is handled by
  construction: the bound of a difference is the sum of the terms' bounds, whatever the size of the result.

The tree has named switch points (`m`): each is one deliberately wrong transcription (a *mutant*); the CPU test shows that every
mutant leaves the bound (or the bits) on the operation's own inputs.  kb8_unproject's reference is written apart (unproject_ref):
Newton's iteration corrects itself, and a bound carried through it operation by operation would double with every step.

Nothing here is module state: the libm budget and the record of the comparisons made belong to the pair of formats that
formats() makes for one evaluation, and every E carries its format."""
import functools

import mpmath as mp
import numpy as np

import orb_slam3_fast_amd as orbx

mp.mp.prec = 200                                   # 60 digits

# libm budgets in ulp: the accuracy table of the OpenCL full profile (OpenCL C specification, "Relative error as ULPs"), which
# the device maths library (ROCm Device Libs, OCML) documents itself against; divide and sqrt are correctly rounded in both
# formats (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt).  A ROCm installation ships the library as bitcode without
# its documentation, so the numbers are the specification's.
ULPS = {"sin": 4, "cos": 4, "acos": 4, "tan": 5, "exp": 3, "atan2": 6}
# The restatement's own libm is the host's: glibc documents the float64 functions above at 1 ulp or better, and a float32 call is
# the float64 one rounded once.  reference(family, own=True) is the bound with these budgets: what the restatement itself may be off.
ULPS_OWN = {k: 1 for k in ULPS}


class Fmt:
    """A number format within one evaluation: its constants, the libm budget in force and the list the evaluation's comparisons
    are recorded in (label, margin, exact); f32 / f64 are the two formats of the same evaluation."""

    def __init__(self, np_type, mant, emin, ulps, decisions):
        self.ulps, self.decisions, self.f32, self.f64 = ulps, decisions, None, None
        self.np, self.u, self.tiny = np_type, mp.mpf(2) ** -(mant + 1), mp.mpf(2) ** (emin - mant - 1)   # half ulp of 1, half the smallest denormal
        self.max = mp.mpf(float(np.finfo(np_type).max))

    def representable(self, v):
        with np.errstate(all="ignore"):
            return mp.mpf(float(self.np(float(v)))) == v


def formats(ulps):
    """(float32, float64) of a fresh evaluation under the given libm budget."""
    decisions = []
    f32, f64 = Fmt(np.float32, 23, -126, ulps, decisions), Fmt(np.float64, 52, -1022, ulps, decisions)
    for f in (f32, f64):
        f.f32, f.f64 = f32, f64
    return f32, f64


F32, F64 = formats(ULPS)          # for evaluations made by hand; reference() makes its own
PI2 = 2 * mp.pi
EPS64 = 2.0 ** -52
ZERO = mp.mpf(0)


class E:
    """mp value of the exact tree, bound on |device value - v|, format; nz: a zero that is -0.0; zero: the device's value is
    certainly 0 (the exact one is below half the smallest denormal)."""
    __slots__ = ("v", "e", "f", "nz", "zero", "d")

    def __init__(self, v, e, f, nz=False, zero=False, d=None):
        self.v, self.e, self.f, self.nz, self.zero, self.d = v, e, f, nz, zero, d

    def _with(self, d):
        self.d = d
        return self

    def _d(self, o, fn):
        """The device's own value while only correctly rounded operations have been made on the inputs (IEEE 754 fixes its bits);
        None behind a libm call.  Comparisons read it where it is known: such a decision is the arithmetic's, not the bound's."""
        if self.d is None or (o is not None and o.d is None):
            return None
        with np.errstate(all="ignore"):
            return fn(self.d, o.d) if o is not None else fn(self.d)

    @staticmethod
    def of(x, f):
        x = float(x)
        return E(mp.mpf(x), ZERO, f, nz=bool(x == 0 and np.signbit(x)), zero=x == 0, d=f.np(x))

    def _lift(self, o):
        return o if isinstance(o, E) else E(mp.mpf(o), ZERO, self.f, zero=o == 0, d=self.f.np(o))

    def _fin(self, v, e, exact, zero=False):
        f = self.f
        if mp.isnan(v) or mp.isinf(v):
            return E(v, ZERO, f)
        av = abs(v)
        if av > f.max:
            return E(mp.sign(v) * mp.inf, ZERO, f) if av - e > f.max * (1 + f.u) else E(v, mp.inf, f)
        if exact and f.representable(v):
            return E(v, ZERO, f, zero=v == 0)
        return E(v, e + f.u * av + f.tiny, f, zero=zero or av + e < f.tiny)

    def __add__(self, o):
        o = self._lift(o)
        assert o.f is self.f
        return self._fin(self.v + o.v, self.e + o.e, self.e == 0 and o.e == 0)._with(self._d(o, lambda a, b: a + b))
    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e, self.f, nz=self.v == 0 and not self.nz, zero=self.zero, d=self._d(None, lambda a: -a))

    def __sub__(self, o):
        return self + (-self._lift(o))

    def __rsub__(self, o):
        return self._lift(o) + (-self)

    def __mul__(self, o):
        o = self._lift(o)
        assert o.f is self.f
        v = self.v * o.v
        d = self._d(o, lambda a, b: a * b)
        if mp.isnan(v) or mp.isinf(v):
            return E(v, ZERO, self.f, d=d)
        if mp.isinf(self.e) or mp.isinf(o.e):
            return E(v, mp.inf, self.f, d=d)
        e = abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e
        return self._fin(v, e, self.e == 0 and o.e == 0, zero=(self.zero or o.zero))._with(d)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        assert o.f is self.f
        d = self._d(o, lambda a, b: a / b)
        if mp.isnan(self.v) or mp.isnan(o.v) or o.zero or (o.v == 0 and o.e == 0):
            return E(mp.nan, ZERO, self.f, d=d)           # x / 0 is inf or NaN: "not finite" is all that is claimed
        if mp.isinf(o.v):
            return E(mp.nan if mp.isinf(self.v) else ZERO, ZERO, self.f, d=d)
        v = self.v / o.v
        if mp.isinf(v):
            return E(v, ZERO, self.f, d=d)
        if o.e >= abs(o.v):
            return E(v, mp.inf, self.f, d=d)
        return self._fin(v, (self.e + abs(v) * o.e) / (abs(o.v) - o.e), self.e == 0 and o.e == 0, zero=self.zero)._with(d)

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sqrt(self):
        v, e = self.v, self.e
        d = self._d(None, np.sqrt)
        if mp.isnan(v) or v + e < 0:
            return E(mp.nan, ZERO, self.f, d=d)
        if mp.isinf(v):
            return E(v, ZERO, self.f, d=d)
        if v <= 0:
            return E(ZERO, mp.sqrt(e) + self.f.tiny, self.f, zero=e == 0, d=d)
        r = mp.sqrt(v)
        return self._fin(r, e / (r + mp.sqrt(max(v - e, 0))), e == 0)._with(d)

    def fabs(self):
        return E(abs(self.v), self.e, self.f, zero=self.zero, d=self._d(None, np.abs))

    def libm(self, name):
        v, e, f = self.v, self.e, self.f
        if mp.isnan(v) or (mp.isinf(v) and name != "exp"):
            return E(mp.nan, ZERO, f)
        if name == "sin":
            r, d = mp.sin(v), min(e * (abs(mp.cos(v)) + e / 2), 2)
        elif name == "cos":
            r, d = mp.cos(v), min(e * (abs(mp.sin(v)) + e / 2), 2)
        elif name == "tan":
            r = mp.tan(v)
            d = e * (1 + r * r) * (1 + 2 * e * abs(r))
        elif name == "exp":
            r = mp.exp(v)
            d = r * (mp.exp(e) - 1)
        else:   # acos: NaN outside [-1, 1]; monotone, so the bound is the image of [v - e, v + e]
            # the argument's side of +-1 is the device's own value's where that is known (correctly rounded operations only so far)
            if (abs(self.d) > 1) if self.d is not None else (abs(v) > 1):
                return E(mp.nan, ZERO, f)
            if abs(v) > 1:
                e, v = e + abs(v) - 1, mp.sign(v)
            r = mp.acos(v)
            d = max(mp.acos(max(v - e, -1)) - r, r - mp.acos(min(v + e, 1)))
        return E(r, d + 2 * f.ulps[name] * f.u * abs(r) + f.tiny, f)


def is_e(x):
    return isinstance(x, E)


def const(like, x):
    """x in the arithmetic of `like`."""
    return E.of(x, like.f) if is_e(like) else type(like)(x)


def narrow(x):      # (float) of a double
    if not is_e(x):
        with np.errstate(all="ignore"):
            return np.float32(x)
    r = E(x.v, x.e, x.f.f32, nz=x.nz, zero=x.zero)._fin(x.v, x.e, x.e == 0, zero=x.zero)
    r.nz = x.nz
    return r._with(x._d(None, np.float32))


def wide(x):
    """(double) of a float: exact.  A float whose bits the arithmetic fixes (correctly rounded operations on the inputs only, such
    as projectJac's float product 3 * k1) enters the double expression as that number: it is a constant of the function, and its
    float rounding is not an error of the double arithmetic that follows."""
    if not is_e(x):
        return np.float64(x)
    if x.d is not None and np.isfinite(x.d):
        return E.of(np.float64(x.d), x.f.f64)
    return E(x.v, x.e, x.f.f64, nz=x.nz, zero=x.zero, d=x._d(None, np.float64))


def sqrt(x):
    return x.sqrt() if is_e(x) else np.sqrt(x)


def fabs(x):
    return x.fabs() if is_e(x) else np.abs(x)


def _libm(name, npf):
    def call(x):
        if is_e(x):
            return x.libm(name)
        return np.float32(npf(np.float64(x))) if isinstance(x, np.float32) else npf(x)
    return call


sin, cos, tan, exp, acos = (_libm("sin", np.sin), _libm("cos", np.cos), _libm("tan", np.tan), _libm("exp", np.exp),
                            _libm("acos", np.arccos))


def atan2(y, x):
    if not is_e(y):
        return np.float32(np.arctan2(np.float64(y), np.float64(x))) if isinstance(y, np.float32) else np.arctan2(y, x)
    f = y.f
    if mp.isnan(y.v) or mp.isnan(x.v):
        return E(mp.nan, ZERO, f)
    if y.v == 0 and x.v == 0:
        r = mp.pi if x.nz else ZERO
    else:
        r = mp.atan2(y.v, x.v)
    if y.v == 0 and y.nz:
        r = -r
    den = x.v * x.v + y.v * y.v
    if mp.isinf(den) or (x.e == 0 and y.e == 0):
        d = ZERO
    elif den == 0 or 4 * (x.e + y.e) ** 2 >= den:
        d = PI2
    else:
        d = min((abs(x.v) * y.e + abs(y.v) * x.e) / den, PI2)
    return E(r, d + 2 * f.ulps["atan2"] * f.u * abs(r) + f.tiny, f)


def less(a, b, label):
    """a < b as the device decides it; an E comparison records by how much the bound leaves it decided."""
    if not (is_e(a) or is_e(b)):
        return bool(a < b)
    a = a if is_e(a) else b._lift(a)
    b = b if is_e(b) else a._lift(b)
    if a.d is not None and b.d is not None:          # every operation so far was correctly rounded: the device's own decision
        a.f.decisions.append((label, mp.inf, True))
        return bool(a.d < b.d)
    if mp.isnan(a.v) or mp.isnan(b.v):
        a.f.decisions.append((label, mp.inf, True))
        return False
    a.f.decisions.append((label, abs(a.v - b.v) - a.e - b.e, a.e == 0 and b.e == 0))
    return a.v < b.v


# ------------------------------------------------------------------------------------------------ the headers' trees
# m names the mutant in force (None: the header).  Quaternions x y z w; a pose is q [4] + t [3]; matrices row-major lists.
def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(a, b, m=None):
    s = -1 if m == "qmul sign" else 1
    r3 = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    r0 = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - s * (a[2] * b[1])
    r1 = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    r2 = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    if m == "qmul order":           # b * a
        return qmul(b, a)
    if m == "qmul swapped index":
        r1 = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[1]
    return [r0, r1, r2, r3]


def qrot(q, v, m=None):
    uv = cross3(v, q) if m == "qrot cross order" else cross3(q, v)
    uv = [x + x for x in uv] if m != "qrot uv not doubled" else uv
    c = cross3(q, uv)
    w = q[0] if m == "qrot w index" else q[3]
    return [v[i] + w * uv[i] + c[i] for i in range(3)]


def normalize_rotation(q, m=None):
    flip = less(q[3], 0, "q[3] < 0") if m != "normalize <=" else not less(0, q[3], "q[3] < 0")
    if m == "normalize no flip":
        flip = False
    if flip:
        q = [-x for x in q]
    n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if m == "normalize squared":
        n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [x / n for x in q]


def quat_from_R_diag(i, R, m=None):
    j = (i + 1) % 3
    k = (j + 1) % 3
    q = [None] * 4
    t = sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[k][j] + R[j][k]) * t if (m == "diag<2> sign" and i == 2) else (R[k][j] - R[j][k]) * t
    q[j] = (R[j][i] + R[i][j]) * t
    q[k] = (R[k][i] + R[i][k]) * t if not (m == "diag<1> index" and i == 1) else (R[k][i] + R[k][i]) * t
    return q


def quat_from_R(R, m=None):
    t = R[0][0] + R[1][1] + R[2][2]
    positive = less(0, t, "trace > 0") if m != "trace >= 0" else not less(t, 0, "trace > 0")
    if positive:
        t = sqrt(t + 1.0)
        q3 = 0.5 * t
        t = 0.5 / t
        return [(R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t, q3]
    i1 = less(R[0][0], R[1][1], "R11 > R00") if m != "argmax >=" else not less(R[1][1], R[0][0], "R11 > R00")
    if less(R[1][1] if i1 else R[0][0], R[2][2], "R22 > max"):
        return quat_from_R_diag(2, R, m)
    return quat_from_R_diag(1 if i1 else 0, R, m)


def skew_and_square(w):
    W = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    W2 = [[W[r][0] * W[0][c] + W[r][1] * W[1][c] + W[r][2] * W[2][c] for c in range(3)] for r in range(3)]
    return W, W2


def eye(r, c):
    return 1.0 if r == c else 0.0


def se3_map(P, X, m=None):
    Y = qrot(P[:4], X)
    t = P[4:]
    if m == "map t index":
        t = [t[1], t[0], t[2]]
    if m == "map minus t":
        return [Y[i] - t[i] for i in range(3)]
    if m == "map conjugate":
        Y = qrot([-P[0], -P[1], -P[2], P[3]], X)
    return [Y[i] + t[i] for i in range(3)]


def se3_compose(a, b, m=None):
    rt = qrot(a[:4], b[4:]) if m != "compose rotates a.t" else qrot(a[:4], a[4:])
    t = [a[4 + i] + rt[i] for i in range(3)]
    q = qmul(a[:4], b[:4]) if m != "compose q order" else qmul(b[:4], a[:4])
    return (normalize_rotation(q) if m != "compose not normalised" else q) + t


def oplus(x, P, m=None):
    w, u = x[:3], x[3:6]
    if m == "oplus translation first":
        w, u = x[3:6], x[:3]
    theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W, W2 = skew_and_square(w)
    thr = 0.0001 if m == "oplus threshold 1e-4" else 0.00001
    if less(theta, thr, "theta < 1e-5"):
        h = 0.5 if m == "oplus W2 / 2" else 1.0
        R = [[eye(r, c) + W[r][c] + (W2[r][c] if h == 1.0 else h * W2[r][c]) for c in range(3)] for r in range(3)]
        V = R
    else:
        s, co, th2 = sin(theta), cos(theta), theta * theta
        a, b, c3 = s / theta, (1 - co) / th2, (theta - s) / (th2 * theta)
        if m == "oplus b for c3":
            c3 = b
        R = [[eye(r, c) + a * W[r][c] + b * W2[r][c] for c in range(3)] for r in range(3)]
        V = [[eye(r, c) + b * W[r][c] + c3 * W2[r][c] for c in range(3)] for r in range(3)]
    qe = quat_from_R(R)
    if m != "oplus no normalize":
        qe = normalize_rotation(qe)
    te = [V[r][0] * u[0] + V[r][1] * u[1] + V[r][2] * u[2] for r in range(3)]
    rt = qrot(qe, P[4:])
    t = [te[r] + rt[r] for r in range(3)]
    return normalize_rotation(qmul(qe, P[:4])) + t


def sim3_exp(x, m=None):
    w, u, sigma = x[:3], x[3:6], x[6]
    theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W, W2 = skew_and_square(w)
    s = exp(sigma)
    eps = 0.0001 if m == "sim3 threshold 1e-4" else 0.00001
    small = less(theta, eps, "theta < 1e-5")
    if small:
        R = [[eye(r, c) + W[r][c] + W2[r][c] for c in range(3)] for r in range(3)]
    else:
        a, b = sin(theta) / theta, (1 - cos(theta)) / (theta * theta)
        R = [[eye(r, c) + a * W[r][c] + b * W2[r][c] for c in range(3)] for r in range(3)]
    if less(fabs(sigma), eps, "|sigma| < 1e-5"):
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1 - cos(theta)) / theta2
            B = (theta - sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        sigma2 = sigma * sigma
        if small:
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            if m == "sim3 B sign":
                B = ((0.5 * sigma2 + sigma + 1) * s) / (sigma2 * sigma)
        else:
            a, b, theta2 = s * sin(theta), s * cos(theta), theta * theta
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
            if m == "sim3 A cos for sin":
                A = (b * sigma + (1 - b) * theta) / (theta * c)
    q = quat_from_R(R)
    t = []
    for r in range(3):
        Wr = [A * W[r][c] + B * W2[r][c] + C * eye(r, c) for c in range(3)]
        t.append(Wr[0] * u[0] + Wr[1] * u[1] + Wr[2] * u[2])
    return q + t + [s]


def sim3_oplus(x, fix, P, m=None):
    x = list(x)
    if fix and m != "oplus7 ignores fixScale":
        x[6] = const(x[6], 0.0)
    Ex = sim3_exp(x)
    q = qmul(Ex[:4], P[:4]) if m != "oplus7 q order" else qmul(P[:4], Ex[:4])
    rt = qrot(Ex[:4], P[4:7])
    t = [Ex[7] * rt[i] + Ex[4 + i] for i in range(3)] if m != "oplus7 unscaled" else [rt[i] + Ex[4 + i] for i in range(3)]
    return q + t + [Ex[7] * P[7]]


def so_inverse(S, m=None):
    qc = [-S[0], -S[1], -S[2], S[3]]
    mm = -1. / S[7] if m != "inverse plus" else 1. / S[7]
    mt = [mm * S[4], mm * S[5], mm * S[6]]
    ti = qrot(qc if m != "inverse not conjugated" else S[:4], mt)
    si = 1. / S[7]
    Ri = [[None] * 3 for _ in range(3)]
    for j in range(3):
        e = [const(S[0], 1.0 if j == k else 0.0) for k in range(3)]
        c = qrot(qc, e)
        for r in range(3):
            if m == "inverse Ri transposed":
                Ri[j][r] = si * c[r]
            else:
                Ri[r][j] = si * c[r]
    return qc + ti + [si] + [Ri[r][c] for r in range(3) for c in range(3)]


K_EPS = 2.220446049250313e-16


def rodrigues2rot(w, m=None):
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    one, zero = const(w[0], 1.0), const(w[0], 0.0)
    R = [one if i % 4 == 0 else zero for i in range(9)]
    eps = 1e-3 if m == "rodrigues eps 1e-3" else K_EPS
    if less(eps, n, "n > eps"):
        a, b = sin(n) / n, (1 - cos(n)) / (n * n)
        if m == "rodrigues b / n":
            b = (1 - cos(n)) / n
        for i in range(3):
            for j in range(3):
                if m == "rodrigues transposed":
                    R[3 * i + j] = R[3 * i + j] + (a * W[3 * j + i] + b * (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j]))
                else:
                    R[3 * i + j] = R[3 * i + j] + (a * W[3 * i + j] + b * (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j]))
    return R


def rot2rodrigues(R, m=None):
    zero = const(R[0], 0.0)
    trace = R[0] + R[4] + R[8] - 1.0
    wnorm = acos(trace / 2.0) if m != "rot2 trace not halved" else acos(trace)
    if not less(K_EPS, wnorm, "wnorm > eps"):
        return [zero, zero, zero]
    sc = wnorm / (2.0 * sin(wnorm)) if m != "rot2 cos" else wnorm / (2.0 * cos(wnorm))
    if m == "rot2 index":
        return [(R[7] - R[5]) * sc, (R[2] - R[6]) * sc, (R[1] - R[3]) * sc]
    return [(R[7] - R[5]) * sc, (R[2] - R[6]) * sc, (R[3] - R[1]) * sc]


def kb8_project_f(c, X, m=None):      # orbx_kb8.h, float
    x2y2 = X[0] * X[0] + X[1] * X[1]
    theta = atan2(sqrt(x2y2), X[2]) if m != "theta atan2 swapped" else atan2(X[2], sqrt(x2y2))
    psi = atan2(X[1], X[0]) if m != "psi atan2 swapped" else atan2(X[0], X[1])
    theta2 = theta * theta
    theta3 = theta * theta2
    theta5 = theta3 * theta2
    theta7 = theta5 * theta2
    theta9 = theta7 * theta2
    r = theta + c[4] * theta3 + c[5] * theta5 + c[6] * (theta5 if m == "theta5 for theta7" else theta7) + c[7] * theta9
    return [c[0] * r * cos(psi) + c[2], c[1] * r * sin(psi) + c[3]]


def cam_project(flag, c, X, m=None):
    if flag:
        return kb8_project_f(c, X, m)
    if m == "pinhole cx for cy":
        return [c[0] * X[0] / X[2] + c[2], c[1] * X[1] / X[2] + c[2]]
    if m == "pinhole divide first":
        return [c[0] * (X[0] / X[2]) + c[2], c[1] * (X[1] / X[2]) + c[3]]
    if m == "pinhole fx for fy":
        return [c[0] * X[0] / X[2] + c[2], c[0] * X[1] / X[2] + c[3]]
    return [c[0] * X[0] / X[2] + c[2], c[1] * X[1] / X[2] + c[3]]


def kb8_project_d(k, X, m=None):      # orbx_kb8_edge.h: k float, X double
    x2y2 = X[0] * X[0] + X[1] * X[1]

    def atan2f_d(y, x):
        return wide(narrow(atan2(wide(y), wide(x))))
    theta = atan2f_d(sqrt(narrow(x2y2)), narrow(X[2]))
    psi = atan2f_d(narrow(X[1]), narrow(X[0])) if m != "psi atan2 swapped" else atan2f_d(narrow(X[0]), narrow(X[1]))
    theta2 = theta * theta
    theta3 = theta * theta2
    theta5 = theta3 * theta2
    theta7 = theta5 * theta2
    theta9 = theta7 * theta2
    kd = [wide(v) for v in k]
    r = theta + kd[4] * theta3 + kd[5] * theta5 + kd[6] * (theta5 if m == "theta5 for theta7" else theta7) + kd[7] * theta9
    sp, cp = sin(psi), cos(psi)
    if m == "sin for cos":
        sp, cp = cp, sp
    return [kd[0] * r * cp + kd[2], kd[1] * r * sp + kd[3]]


def kb8_project_jac(k, X, m=None):
    x, y, z = X
    x2, y2, z2 = x * x, y * y, z * z
    r2 = x2 + y2
    r = sqrt(r2)
    r3 = r2 * r
    theta = atan2(r, z) if m != "theta atan2 swapped" else atan2(z, r)
    theta2 = theta * theta
    theta3 = theta2 * theta
    theta4 = theta2 * theta2
    theta5 = theta4 * theta
    theta6 = theta2 * theta4
    theta7 = theta6 * theta
    theta8 = theta4 * theta4
    theta9 = theta8 * theta
    kd = [wide(v) for v in k]
    f = theta + theta3 * kd[4] + theta5 * kd[5] + theta7 * kd[6] + theta9 * kd[7]
    fd = 1 + wide(3 * k[4]) * theta2 + wide(5 * k[5]) * theta4 + wide(7 * k[6]) * theta6 + wide(9 * k[7]) * theta8
    if m == "fd 7 for 9":
        fd = 1 + wide(3 * k[4]) * theta2 + wide(5 * k[5]) * theta4 + wide(7 * k[6]) * theta6 + wide(7 * k[7]) * theta8
    den = r2 * (r2 + z2)
    k0, k1 = kd[0], kd[1]
    flip = m == "jac off-diagonal sign"
    return [k0 * (fd * z * x2 / den + f * y2 / r3),
            k0 * (fd * z * y * x / den + f * y * x / r3) if flip else k0 * (fd * z * y * x / den - f * y * x / r3),
            -k0 * fd * x / (r2 + z2),
            k1 * (fd * z * y * x / den + f * y * x / r3) if flip else k1 * (fd * z * y * x / den - f * y * x / r3),
            k1 * (fd * z * y2 / den + f * x2 / r3),
            -k1 * fd * y / (r2 + z2)]


HALF_PI_F = np.float32(3.1415926535897932384626433832795 / 2.0)


def cam_unproject(flag, c, prec, u, v, rounded, m=None):
    """The numpy restatement of cam_unproject<kRoundedTan> (float32 scalars)."""
    f32 = np.float32
    if m == "unproject cy for cx":
        pwx, pwy = (u - c[3]) / c[0], (v - c[3]) / c[1]
    else:
        pwx, pwy = (u - c[2]) / c[0], (v - c[3]) / c[1]
    if not flag:
        return [pwx, pwy, f32(1)]
    scale = f32(1)
    theta_d = np.sqrt(pwx * pwx + pwy * pwy)
    theta_d = min(max(-HALF_PI_F, theta_d), HALF_PI_F) if m != "unproject no clamp" else theta_d
    thr = 1e-8 if m != "unproject threshold 0.1" else 0.1
    if np.float64(theta_d) > thr:
        theta = theta_d
        for j in range(10 if m != "unproject one step" else 1):
            theta2 = theta * theta
            theta4 = theta2 * theta2
            theta6 = theta4 * theta2
            theta8 = theta4 * theta4
            k0, k1, k2, k3 = c[4] * theta2, c[5] * theta4, c[6] * theta6, c[7] * theta8
            fix = (theta * (1 + k0 + k1 + k2 + k3) - theta_d) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + (7 if m == "unproject 7 for 9" else 9) * k3)
            theta = theta - fix
            if np.abs(fix) < prec:
                break
        t = f32(np.tan(np.float64(theta)))        # the rounded tangent; the restatement's tanf is the same
        scale = t / theta_d
    return [pwx * scale, pwy * scale, f32(1)]


def unproject_ref(c, prec, u, v, rounded, f32):
    """kb8_unproject in E: candidates [(outputs [3] of E, stopped at)], ambiguous.  Every operation of the loop is correctly
    rounded, so |theta_fix| < precision is the arithmetic's own decision, like every comparison `less` makes on such operands: the
    float32 iteration runs beside the mpmath one and decides the break.  A break whose float32 operands were not fixed by IEEE (none
    today) would be ambiguous where |theta_fix| is within its bound of precision, and then the reference stopped at either of the two
    adjacent iterations is accepted.  Newton's step N(theta) = theta - g / g' has
    N' = g g'' / g'^2, which vanishes at the root: the bound after a step is |N'| x the bound before + what theta_d's bound moves
    the root by + the rounding of this step's own operations (evaluated with theta taken as exact)."""
    c = [E.of(x, f32) for x in c]
    u, v = E.of(u, f32), E.of(v, f32)
    pwx, pwy = (u - c[2]) / c[0], (v - c[3]) / c[1]
    one = E.of(1.0, f32)
    theta_d = sqrt(pwx * pwx + pwy * pwy)
    hp = mp.mpf(float(HALF_PI_F))
    if mp.isnan(theta_d.v):
        return [([theta_d, theta_d, one], -1)], False
    f32.decisions.append(("clamp", abs(theta_d.v - hp) - theta_d.e, theta_d.e == 0))
    if theta_d.v > hp:
        theta_d = E(hp, ZERO, f32, d=HALF_PI_F)
    if not less(1e-8, wide(theta_d), "theta_d > 1e-8"):
        return [([pwx * one, pwy * one, one], 0)], False
    kv = [x.v for x in c[4:8]]

    def finish(theta):
        t = narrow(tan(wide(theta))) if rounded else tan(theta)
        scale = t / theta_d
        return [pwx * scale, pwy * scale, one]

    def step(theta):
        th = E(theta.v, ZERO, f32)
        td = E(theta_d.v, ZERO, f32)
        theta2 = th * th
        theta4 = theta2 * theta2
        theta6 = theta4 * theta2
        theta8 = theta4 * theta4
        k0, k1, k2, k3 = c[4] * theta2, c[5] * theta4, c[6] * theta6, c[7] * theta8
        fix = (th * (1 + k0 + k1 + k2 + k3) - td) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3)
        new = th - fix

        def nprime(t):
            t2 = t * t
            g = t * (1 + kv[0] * t2 + kv[1] * t2 ** 2 + kv[2] * t2 ** 3 + kv[3] * t2 ** 4) - theta_d.v
            g1 = 1 + 3 * kv[0] * t2 + 5 * kv[1] * t2 ** 2 + 7 * kv[2] * t2 ** 3 + 9 * kv[3] * t2 ** 4
            g2 = t * (6 * kv[0] + 20 * kv[1] * t2 + 42 * kv[2] * t2 ** 2 + 72 * kv[3] * t2 ** 3)
            return abs(g * g2 / (g1 * g1)), abs(g1)
        n0, g1 = nprime(theta.v)
        n1 = max(n0, nprime(theta.v - theta.e)[0], nprime(theta.v + theta.e)[0])
        carried = n1 * theta.e + theta_d.e / g1
        # the decision reads the computed fix: its bound is this step's rounding plus what the carried bound moves it by
        return E(new.v, new.e + carried, f32), fix.v, fix.e + theta.e + theta_d.e / g1

    p = mp.mpf(float(prec))
    out, ambiguous = [], False
    theta, alt = E(theta_d.v, theta_d.e, f32), None
    known = theta_d.d is not None and all(x.d is not None for x in c)
    t_np, td_np, c_np = theta_d.d, theta_d.d, [x.d for x in c]
    for j in range(10):
        theta, fv, fe = step(theta)
        stop = abs(fv) < p
        if known:
            with np.errstate(all="ignore"):
                t2 = t_np * t_np
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t4 * t4
                k0, k1, k2, k3 = c_np[4] * t2, c_np[5] * t4, c_np[6] * t6, c_np[7] * t8
                fix_np = (t_np * (1 + k0 + k1 + k2 + k3) - td_np) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3)
                t_np = t_np - fix_np
                stop = bool(np.abs(fix_np) < np.float32(prec))
        elif alt is None and abs(abs(fv) - p) <= fe and j < 9:
            ambiguous = True
            if stop:        # the other decision: one more step
                alt = (finish(step(theta)[0]), j + 2)
            else:
                alt = (finish(theta), j + 1)
        if stop:
            break
    out.append((finish(theta), j + 1))
    if alt is not None:
        out.append(alt)
    return out, ambiguous


# ------------------------------------------------------------------------------------------------ the operations
TUM_VI = np.array([190.978477, 190.973307, 254.931706, 256.897442, 0.003482389402, 0.000715034845, -0.002053236141,
                   0.000202936736], np.float32)       # Examples/Monocular/TUM-VI.yaml of ORB-SLAM3: Camera1.fx .. k4
LARGE_K = np.array([300.5, 299.25, 320.25, 240.75, -0.05, 0.02, -0.01, 0.003], np.float32)
ORIGIN_PP = np.array([190.978477, 190.973307, 0.0, 0.0, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], np.float32)

EXACT = ("QMUL", "QROT", "NORMALIZE_ROTATION", "QUAT_FROM_R", "SE3_MAP", "SE3_COMPOSE", "SO_INVERSE", "PINHOLE_PROJECT",
         "PINHOLE_UNPROJECT")
LIBM = ("CAM_PROJECT", "CAM_UNPROJECT", "CAM_UNPROJECT_ROUNDED_TAN", "KB8_PROJECT_D", "KB8_PROJECT_JAC", "OPLUS", "SIM3_EXP",
        "SIM3_OPLUS", "RODRIGUES2ROT", "ROT2RODRIGUES")
# family -> (ORBX_GEOM op, tree over one item's scalars).  The two PINHOLE families are the flag-0 items of the camera operations.
# ROUND_TRIP is rot2rodrigues(rodrigues2rot(w)) as one tree: two calls on the device, the second on the first's output.
GEOM_OP = {"PINHOLE_PROJECT": "CAM_PROJECT", "PINHOLE_UNPROJECT": "CAM_UNPROJECT", "ROUND_TRIP": "ROT2RODRIGUES"}
TREE = {
    "QMUL": lambda a, m: qmul(a[:4], a[4:], m),
    "QROT": lambda a, m: qrot(a[:4], a[4:], m),
    "NORMALIZE_ROTATION": lambda a, m: normalize_rotation(a, m),
    "QUAT_FROM_R": lambda a, m: quat_from_R([a[0:3], a[3:6], a[6:9]], m),
    "SE3_MAP": lambda a, m: se3_map(a[:7], a[7:], m),
    "SE3_COMPOSE": lambda a, m: se3_compose(a[:7], a[7:], m),
    "SO_INVERSE": lambda a, m: so_inverse(a, m),
    "PINHOLE_PROJECT": lambda a, m: cam_project(False, a[1:9], a[9:], m),
    "CAM_PROJECT": lambda a, m: cam_project(True, a[1:9], a[9:], m),
    "KB8_PROJECT_D": lambda a, m: kb8_project_d(a[:8], a[8:], m),
    "KB8_PROJECT_JAC": lambda a, m: kb8_project_jac(a[:8], a[8:], m),
    "OPLUS": lambda a, m: oplus(a[:6], a[6:], m),
    "SIM3_EXP": lambda a, m: sim3_exp(a, m),
    "SIM3_OPLUS": lambda a, m: sim3_oplus(a[:7], float(a[7].v if is_e(a[7]) else a[7]) != 0.0, a[8:], m),
    "RODRIGUES2ROT": lambda a, m: rodrigues2rot(a, m),
    "ROT2RODRIGUES": lambda a, m: rot2rodrigues(a, m),
    "ROUND_TRIP": lambda a, m: rot2rodrigues(rodrigues2rot(a), m),
}
MUTANTS = {
    "QMUL": ("qmul sign", "qmul order", "qmul swapped index"),
    "QROT": ("qrot cross order", "qrot uv not doubled", "qrot w index"),
    "NORMALIZE_ROTATION": ("normalize <=", "normalize no flip", "normalize squared"),
    "QUAT_FROM_R": ("diag<2> sign", "diag<1> index", "trace >= 0", "argmax >="),
    "SE3_MAP": ("map t index", "map minus t", "map conjugate"),
    "SE3_COMPOSE": ("compose rotates a.t", "compose q order", "compose not normalised"),
    "SO_INVERSE": ("inverse plus", "inverse not conjugated", "inverse Ri transposed"),
    "PINHOLE_PROJECT": ("pinhole cx for cy", "pinhole divide first", "pinhole fx for fy"),
    "PINHOLE_UNPROJECT": ("unproject cy for cx", "pinhole fy for fx", "pinhole multiply"),
    "CAM_PROJECT": ("theta atan2 swapped", "psi atan2 swapped", "theta5 for theta7"),
    "CAM_UNPROJECT": ("unproject no clamp", "unproject threshold 0.1", "unproject one step", "unproject 7 for 9", "unproject cy for cx"),
    "CAM_UNPROJECT_ROUNDED_TAN": ("unproject no clamp", "unproject threshold 0.1", "unproject one step", "unproject 7 for 9"),
    "KB8_PROJECT_D": ("psi atan2 swapped", "theta5 for theta7", "sin for cos"),
    "KB8_PROJECT_JAC": ("theta atan2 swapped", "fd 7 for 9", "jac off-diagonal sign"),
    "OPLUS": ("oplus translation first", "oplus threshold 1e-4", "oplus W2 / 2", "oplus b for c3", "oplus no normalize"),
    "SIM3_EXP": ("sim3 threshold 1e-4", "sim3 B sign", "sim3 A cos for sin"),
    "SIM3_OPLUS": ("oplus7 ignores fixScale", "oplus7 q order", "oplus7 unscaled"),
    "RODRIGUES2ROT": ("rodrigues eps 1e-3", "rodrigues b / n", "rodrigues transposed"),
    "ROT2RODRIGUES": ("rot2 trace not halved", "rot2 cos", "rot2 index"),
}
UNPROJECT = ("PINHOLE_UNPROJECT", "CAM_UNPROJECT", "CAM_UNPROJECT_ROUNDED_TAN")


def geom_op(family):
    return getattr(orbx, "GEOM_" + GEOM_OP.get(family, family))


def scalars(family, item):
    """One item as the tree's scalars in numpy: the KB8 edge items carry k as float32 and X as float64."""
    if family in ("KB8_PROJECT_D", "KB8_PROJECT_JAC"):
        return [np.float32(x) for x in item[:4].view(np.float32)] + [np.float64(x) for x in item[4:]]
    t = GEOM_DTYPE(family)
    return [t(x) for x in item]


def GEOM_DTYPE(family):
    return orbx.GEOM_ITEM[geom_op(family)][0]


def restate(family, items, m=None):
    """The numpy restatement on every item: [n][out] in the operation's type."""
    n_out = orbx.GEOM_ITEM[geom_op(family)][2]
    items = np.asarray(items).reshape(len(items), -1)
    out = np.empty((len(items), n_out), GEOM_DTYPE(family))
    with np.errstate(all="ignore"):
        for i, item in enumerate(items):
            a = scalars(family, item)
            if family in UNPROJECT:
                if m == "pinhole fy for fx":
                    r = [(a[10] - a[3]) / a[1], (a[11] - a[4]) / a[2], np.float32(1)]
                    r[0] = (a[10] - a[3]) / a[2]
                elif m == "pinhole multiply":
                    r = [(a[10] - a[3]) * (np.float32(1) / a[1]), (a[11] - a[4]) * (np.float32(1) / a[2]), np.float32(1)]
                else:
                    r = cam_unproject(a[0] != 0, a[1:9], a[9], a[10], a[11], family.endswith("TAN"), m)
            else:
                r = TREE[family](a, m)
            out[i] = r
    return out


class Ref:
    """The reference of one family: candidates [c][n][out] as hi + lo doubles with the bound e (inf: nothing is claimed, NaN
    in hi: the device must be inf or NaN), the decisions made on the way, which items were ambiguous at Newton's break."""

    def __init__(self, hi, lo, e, decisions, ambiguous):
        self.hi, self.lo, self.e, self.decisions, self.ambiguous = hi, lo, e, decisions, ambiguous


def _split(x):
    if mp.isnan(x.v) or mp.isinf(x.v):
        return float("nan"), 0.0, 0.0
    hi = float(x.v)
    return hi, float(x.v - mp.mpf(hi)), float(x.e * (1 + mp.mpf(2) ** -40))


@functools.lru_cache(maxsize=None)
def reference(family, own=False):
    """The family's reference under the device's libm budget, or (own) under the host's, which bounds the restatement itself."""
    f32, f64 = formats(ULPS_OWN if own else ULPS)
    items = cases(family)[1]
    n_out = orbx.GEOM_ITEM[geom_op(family)][2]
    hi = np.full((2, len(items), n_out), np.nan)
    lo, e = np.zeros_like(hi), np.zeros_like(hi)
    ambiguous = np.zeros(len(items), bool)
    two = np.zeros(len(items), bool)
    for i, item in enumerate(items):
        a = scalars(family, item)
        if family in UNPROJECT and a[0] != 0:
            cands, amb = unproject_ref(a[1:9], a[9], a[10], a[11], family.endswith("TAN"), f32)
            ambiguous[i] = amb          # the reference stopped at either of the two adjacent iterations is accepted
            outs = [c[0] for c in cands]
        else:
            fmt = f32 if GEOM_DTYPE(family) is np.float32 else f64
            if family in ("KB8_PROJECT_D", "KB8_PROJECT_JAC"):
                ea = [E.of(x, f32) for x in a[:8]] + [E.of(x, f64) for x in a[8:]]
            else:
                ea = [E.of(x, fmt) for x in a]
            if family in UNPROJECT:
                outs = [[(ea[10] - ea[3]) / ea[1], (ea[11] - ea[4]) / ea[2], E.of(1.0, f32)]]
            else:
                outs = [TREE[family](ea, None)]
        for c, o in enumerate(outs):
            for k, x in enumerate(o):
                hi[c, i, k], lo[c, i, k], e[c, i, k] = _split(x)
        two[i] = len(outs) > 1
        if not two[i]:
            hi[1, i], lo[1, i], e[1, i] = hi[0, i], lo[0, i], e[0, i]
    return Ref(hi, lo, e, list(f32.decisions), ambiguous)


def measure(family, got, own=False):
    """(fraction [n][out] of the bound for the better candidate of each item, must_be_nonfinite [n][out], unbounded [n][out]).
    A required inf / NaN that is finite on the device counts as an infinite fraction."""
    ref = reference(family, own)
    got = np.asarray(got, np.float64)
    fr = []
    with np.errstate(all="ignore"):
        for c in range(2):
            d = np.abs((got - ref.hi[c]) - ref.lo[c])
            f = np.where(d == 0, 0.0, d / ref.e[c])
            f = np.where(np.isinf(ref.e[c]), 0.0, f)                              # nothing is claimed
            f = np.where(np.isnan(ref.hi[c]), np.where(np.isfinite(got), np.inf, 0.0), f)
            f = np.where(np.isnan(f), np.inf, f)                                  # a NaN where a number is due
            fr.append(f)
    pick = fr[1].max(1) < fr[0].max(1)
    return np.where(pick[:, None], fr[1], fr[0]), np.isnan(ref.hi[0]), np.isinf(ref.e[0])


def same_bits(a, b):
    """Bit equality, NaNs by position (the payload of a NaN is not the arithmetic's)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


# ------------------------------------------------------------------------------------------------ the inputs
def _rot(axis, angle):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _named(groups):
    names, rows = [], []
    for name, r in groups:
        r = np.atleast_2d(np.asarray(r))
        names += [name] * len(r)
        rows.append(r)
    return np.array(names), np.concatenate(rows)


SPECIAL = [0.0, -0.0, 5e-324, -2.0 ** -1040, 2.0 ** 500, -2.0 ** -500, np.inf, -np.inf, np.nan, 1.0]
THETAS = (0.0, float(np.nextafter(1e-5, 0)), float(np.nextafter(1e-5, 1)), 1e-3, 1.0, np.pi - 1e-9, np.pi + 1e-9, 2 * np.pi, 50.0)
SIGMAS = (0.0, float(np.nextafter(1e-5, 0)), float(np.nextafter(1e-5, 1)), -float(np.nextafter(1e-5, 0)), -float(np.nextafter(1e-5, 1)),
          1e-3, -1e-3, 2.0, -2.0)
AXES = np.array([[0.36, -0.48, 0.8], [-0.6, 0.64, 0.48], [1.0, 0.0, 0.0]])


def _omega(theta, axis):
    """A rotation vector of norm theta along axis.  For the two neighbours of 1e-5 the length is searched among the doubles
    around it so that the norm AS THE FUNCTIONS COMPUTE IT is the largest below 1e-5, or the smallest not below it."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    if abs(theta - 1e-5) > 1e-15:
        return theta * a
    best, t = None, 1e-5
    for _ in range(40):
        t = np.nextafter(t, 0)
    for _ in range(80):
        w = t * a
        n = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        if (theta < 1e-5 and n < 1e-5 and (best is None or n >= best[0])) or (theta >= 1e-5 and n >= 1e-5 and (best is None or n < best[0])):
            best = (n, w)
        t = np.nextafter(t, 1)
    return best[1]


def _points():
    rng = np.random.default_rng(11)
    g = []
    dirs = (np.cos(0.3), np.sin(0.3))
    for z, step in ((1.0, 1), (2.5, 8)):
        g.append(("r/z decades", [[10.0 ** -d * z * dirs[0], 10.0 ** -d * z * dirs[1], z] for d in range(0, 161, step)]))
    g.append(("on the axis", [[0, 0, 1], [0, 0, 2.5], [0.0, 0.0, -1.0]]))
    g.append(("z = 0", [[1, 2, 0], [0.3, -0.2, 0], [-1e-3, 1e-3, 0.0]]))
    g.append(("z < 0", [[1, 2, -1], [1e-3, 1e-3, -2], [-0.5, 0.25, -0.125]]))
    g.append(("-0.0", [[-0.0, 1, 1], [1, -0.0, 1], [1, 1, -0.0], [-0.0, -0.0, 1], [-0.0, -0.0, -0.0], [-1, -0.0, 1], [-1, 0.0, 1],
                       [0.0, 0.0, -0.0], [0.0, -0.0, 1], [-0.0, 0.0, 1], [-0.0, -1.0, 2.0]]))
    g.append(("x or y alone zero", [[0, 0.5, 1], [0, -0.5, 1], [0.5, 0, 1], [-0.5, 0, 1]]))
    X = rng.normal(size=(80, 3)) * [1, 1, 0.5] + [0, 0, 1.0]
    g.append(("random", X))
    g.append(("scaled by 2^100", X[:12] * 2.0 ** 100))
    g.append(("scaled by 2^-100", X[:12] * 2.0 ** -100))
    return g


def _pixels(cam):
    rng = np.random.default_rng(5)
    f32 = np.float32
    cx, cy, fx = f32(cam[2]), f32(cam[3]), float(cam[0])
    g = [("principal point", [[cx, cy], [np.nextafter(cx, f32(1e9)), cy], [np.nextafter(cx, f32(-1e9)), cy],
                              [cx, np.nextafter(cy, f32(1e9))], [cx, np.nextafter(cy, f32(-1e9))]])]
    radial = []
    for td in list(np.linspace(0.01, 1.5, 16)) + [1.55, 1.566, 1.5703, 1.5707, 1.5709, 1.58, 2.0, 5.0, 100.0]:
        for ang in (0.4, 2.3):
            radial.append([float(cx) + fx * td * np.cos(ang), float(cy) + float(cam[1]) * td * np.sin(ang)])
    g.append(("radial", radial))
    g.append(("random", rng.uniform(0, 512, size=(50, 2))))
    return g


@functools.lru_cache(maxsize=None)
def cases(family):
    """(names [n], items [n][in]) of a family, in the operation's item layout; shared and not to be written to."""
    rng = np.random.default_rng(sum(map(ord, family)))
    if family in ("KB8_PROJECT_D", "KB8_PROJECT_JAC"):
        names, rows = [], []
        for cname, cam in (("TUM-VI", TUM_VI), ("large k", LARGE_K)):
            n, X = _named(_points())
            names += [cname + ", " + x for x in n]
            rows.append(orbx.geom_kb8_items(cam, X))
        return np.array(names), np.concatenate(rows)
    if family in ("CAM_PROJECT", "PINHOLE_PROJECT"):
        names, rows = [], []
        for cname, cam in (("TUM-VI", TUM_VI), ("large k", LARGE_K)):
            # the points of the double operations narrowed to float.  Of the decades with z = 1 only r / z >= 1e-44 are kept: below
            # the smallest float denormal the narrowed x and y are zero and the point is the one on the axis.  |X| scaled by 2^+-100
            # stays: x^2 + y^2 overflows to inf (theta = pi / 2 whatever z is) or underflows to 0 (the principal point), and the
            # pinhole quotient is still normal.  2^+-40, where nothing over- or underflows, is run beside it.
            pts = []
            for n, x in _points():
                x = np.asarray(x, float)
                pts.append((n, x[:45] if n == "r/z decades" and len(x) > 45 else x))
                if "scaled by 2^" in n:
                    pts.append((n.replace("100", "40"), x * (2.0 ** -60 if n.endswith("2^100") else 2.0 ** 60)))
            n, X = _named(pts)
            names += [cname + ", " + x for x in n]
            rows.append(np.hstack([np.full((len(X), 1), float(family == "CAM_PROJECT")), np.tile(cam, (len(X), 1)), X]).astype(np.float32))
        return np.array(names), np.concatenate(rows)
    if family in UNPROJECT:
        names, rows = [], []
        flag = float(family != "PINHOLE_UNPROJECT")
        for cname, cam in (("TUM-VI", TUM_VI), ("large k", LARGE_K)):
            for prec in (1e-6, 1e-9, 1e-3):
                n, px = _named(_pixels(cam))
                names += ["%s, precision %g, %s" % (cname, prec, x) for x in n]
                rows.append(np.hstack([np.full((len(px), 1), flag), np.tile(cam, (len(px), 1)), np.full((len(px), 1), prec), px]).astype(np.float32))
        # theta_d on either side of 1e-8: only a principal point at the origin leaves pixels that fine
        fx = float(ORIGIN_PP[0])
        px = np.array([[1e-8 * fx * k, 0.0] for k in (0.5, 0.999, 1.001, 2.0)] + [[0.0, -1e-8 * float(ORIGIN_PP[1]) * k] for k in (0.999, 1.001)])
        for prec in (1e-6, 1e-9, 1e-3):
            names += ["origin, precision %g, theta_d about 1e-8" % prec] * len(px)
            rows.append(np.hstack([np.full((len(px), 1), flag), np.tile(ORIGIN_PP, (len(px), 1)), np.full((len(px), 1), prec), px]).astype(np.float32))
        return np.array(names), np.concatenate(rows)
    if family == "QUAT_FROM_R":
        near_pi = [_rot(rng.normal(size=3), np.pi - s * 10.0 ** -rng.uniform(8, 12)) for s in (1, -1) for _ in range(20)]
        small = []
        for w in ([3e-6, -4e-6, 5e-6], [1e-9, 2e-7, -3e-8], [0.0, 0.0, 9.9e-6], [-1e-6, 0.0, 0.0]):
            W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            small.append(np.eye(3) + W + W @ W)
        off = rng.normal(size=(6, 3, 3))

        def with_diag(d, k):
            M = off[k].copy()
            M[np.arange(3), np.arange(3)] = d
            return M
        g = [("identity", [np.eye(3)]),
             ("pi about an axis", [np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])]),
             ("cyclic permutations", [np.eye(3)[[1, 2, 0]], np.eye(3)[[2, 0, 1]]]),
             ("R11 == R00 > R22", [with_diag([0.125, 0.125, -0.75], 0), with_diag([-0.25, -0.25, -0.5], 1)]),
             ("R22 == R11 > R00", [with_diag([-0.75, 0.125, 0.125], 2), with_diag([-0.5, -0.25, -0.25], 3)]),
             ("R22 the largest", [with_diag([-0.5, -0.375, 0.25], 4)]),
             ("trace exactly 0, not orthogonal", [with_diag([0.5, 0.25, -0.75], 5), with_diag([-0.75, 0.5, 0.25], 0), with_diag([0.25, -0.75, 0.5], 1)]),
             ("within 1e-8 of pi", near_pi),
             ("I + W + W^2", small),
             ("random rotations", [_rot(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(60)])]
        n, r = _named([(a, np.asarray(b).reshape(len(b), 9)) for a, b in g])
        return n, r.astype(np.float64)
    if family == "NORMALIZE_ROTATION":
        q = _quat(rng, 40)
        g = [("random", q), ("w = +0", [[0.6, 0.0, 0.8, 0.0]]), ("w = -0", [[0.6, 0.0, 0.8, -0.0]]),
             ("w a denormal", [[0.6, 0.0, 0.8, 5e-324], [0.6, 0.0, 0.8, -5e-324]]),
             ("norm 2^500", q[:4] * 2.0 ** 500), ("norm 2^-500", q[:4] * 2.0 ** -500), ("zero", [[0.0, 0.0, 0.0, 0.0], [-0.0, 0.0, -0.0, -0.0]]),
             ("not finite", [[np.inf, 0, 0, 1], [np.nan, 0, 0, 1], [0, 0, 0, -np.inf]])]
        return _named(g)
    if family in ("QMUL", "QROT", "SE3_MAP", "SE3_COMPOSE", "SO_INVERSE"):
        n_in = orbx.GEOM_ITEM[geom_op(family)][1]
        r = rng.normal(size=(120, n_in))
        sp = rng.normal(size=(len(SPECIAL) * 3, n_in))
        for i in range(len(sp)):
            sp[i, (i * 5) % n_in] = SPECIAL[i % len(SPECIAL)]
            sp[i, (i * 3 + 1) % n_in] = SPECIAL[(i // 2) % len(SPECIAL)]
        big = r[:10] * 2.0 ** 400
        g = [("random", r), ("specials", sp), ("scaled by 2^400", big), ("scaled by 2^-400", r[:10] * 2.0 ** -400), ("zero", np.zeros((1, n_in)))]
        if family == "SO_INVERSE":
            g.append(("scale 0, -0, denormal", [np.r_[r[0, :7], s] for s in (0.0, -0.0, 5e-324, 2.0 ** -1030)]))
        if family == "SE3_COMPOSE":
            g.append(("product with w < 0", [np.r_[0, 0, 1, 0, 1, 2, 3, 0, 0, 1, 0, 4, 5, 6], np.r_[0.6, 0, 0, 0.8, 1, 2, 3, -0.6, 0, 0, -0.8, 4, 5, 6]]))
        return _named(g)
    if family in ("OPLUS", "SIM3_EXP", "SIM3_OPLUS"):
        poses = np.array([[0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 2.0], [0.18, -0.24, 0.4, 0.866, -1.0, 3.0, 0.5]])
        names, rows = [], []
        u = np.array([0.3, -0.2, 0.1])
        for th in THETAS:
            for ai, ax in enumerate(AXES[:2] if family != "SIM3_EXP" else AXES):
                w = _omega(th, ax)
                if family == "OPLUS":
                    for P in poses:
                        names.append("theta %r" % th)
                        rows.append(np.r_[w, u, P])
                    continue
                for sg in SIGMAS:
                    if family == "SIM3_EXP":
                        names.append("theta %r, sigma %r" % (th, sg))
                        rows.append(np.r_[w, u, sg])
                    else:
                        for fix in ((0.0, 1.0) if ai == 0 else (0.0,)):
                            names.append("theta %r, sigma %r, fixScale %d" % (th, sg, fix))
                            rows.append(np.r_[w, u, sg, fix, poses[1], 1.25])
        return np.array(names), np.array(rows)
    if family == "RODRIGUES2ROT":
        g = [("zero", [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0]]),
             ("norm about eps", [[K_EPS * k, 0.0, 0.0] for k in (0.5, 0.999, 1.001, 2.0)] + [[0.6 * K_EPS * k, 0.0, 0.8 * K_EPS * k] for k in (0.9, 1.1)]),
             ("angles", [_omega(t, ax) for t in (1e-9, 1e-7, 1e-3, 1.0, np.pi - 1e-6, np.pi, 2 * np.pi, 50.0) for ax in AXES]),
             ("random", rng.normal(size=(60, 3)))]
        return _named(g)
    if family == "ROUND_TRIP":
        return np.array(["round trip"] * len(ROUND_TRIP_W)), ROUND_TRIP_W
    if family == "ROT2RODRIGUES":
        up, down = np.eye(3), -np.eye(3)
        up[2, 2] = 1 + 2.0 ** -51              # trace / 2 = 1 + 1 ulp, every operation on the way exact
        down[0, 0] = 1.0
        down[2, 2] = -1 - 2.0 ** -51           # (1 - 1 - (1 + 2^-51) - 1) / 2 = -1 - 2^-52
        off = rng.normal(size=(3, 3)) * 1e-3
        g = [("identity", [np.eye(3)]),
             ("trace / 2 one ulp above 1", [up, up + off * (1 - np.eye(3))]),
             ("trace / 2 one ulp below -1", [down, down + off * (1 - np.eye(3))]),
             ("angles", [_rot(ax, t) for t in (1e-9, 1e-7, 1e-3, 1.0, np.pi - 1e-6, np.pi) for ax in AXES]),
             ("round trip", [restate("RODRIGUES2ROT", np.array([w]))[0].reshape(3, 3) for w in ROUND_TRIP_W]),
             ("random", [_rot(rng.normal(size=3), rng.uniform(0.01, 3.1)) for _ in range(60)])]
        return _named([(a, np.asarray(b).reshape(len(b), 9)) for a, b in g])
    raise KeyError(family)


ROUND_TRIP_W = np.array([[0.3, -0.2, 0.5], [1e-4, 2e-4, -1e-4], [1.2, 0.9, -1.7], [-2.0, 0.1, 0.3], [0.0, 0.0, 3.0], [1e-7, 0.0, 0.0]])
FAMILIES = EXACT + LIBM
