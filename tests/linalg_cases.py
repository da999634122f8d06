"""Inputs, references and checks for the functions of csrc/orbx_linalg.h run alone through orbx_debug_linalg (tests/test_linalg_device.py).

Every routine has a builder of named cases, a reference that is plain high-precision arithmetic (numpy float64 SVD, lba_cases.ldlt_dense,
numpy.longdouble or mpmath), and a check that turns (inputs, outputs) into rows of (name, measured, bound).  The same checks run on the
CPU over the references' own outputs, where they must stay within a quarter of each bound (so that no input can hide a device failure),
and on the device's outputs, where they must stay within the bound.  null_vector4 is also restated in numpy (null_vector4_restated:
the device's arithmetic in the device's order, 1 / x in place of rcp64), because its result at degenerate inputs is a property of the
iteration and not of the matrix alone.  The builders are cached: what they return is shared between the tests and must not be written to."""
import functools
import itertools

import numpy as np
import mpmath

from lba_cases import ldlt_dense          # the LDLTs' reference, used by the tests as linalg_cases.ldlt_dense

EPS = float(np.finfo(float).eps)          # 2^-52
LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63       # x87 extended: truth to 2^-64; otherwise mpmath
TINY = float(np.finfo(float).tiny)        # 2^-1022, the smallest normal
HUGE = float(np.finfo(float).max)


def fraction(rows):
    """{name: largest measured / bound} over rows of (name, measured, bound); a zero bound with a zero measurement counts as 0."""
    out = {}
    for name, m, b in rows:
        m, b = np.atleast_1d(np.asarray(m, float)), np.atleast_1d(np.asarray(b, float))
        m, b = np.broadcast_arrays(m, b)
        if not len(m):
            continue
        with np.errstate(all="ignore"):
            f = np.where((m == 0) & (b >= 0), 0.0, m / np.where(b > 0, b, np.nan))
        f = np.where(np.isnan(f), np.inf, f)      # a NaN measurement or a zero bound under a non-zero measurement fails
        out[name] = max(out.get(name, 0.0), float(f.max()))
    return out


# ------------------------------------------------------------------------------------------------ rcp64 / rsqrt64
RCP_BOUND = 2.0 ** -51
RCP_DOMAIN = (TINY, 2.0 ** 1022)          # the argument and the result both normal
RSQRT_DOMAIN = (TINY, HUGE)


@functools.lru_cache(None)
def recip_inputs(rsq):
    """About 56 K (rcp64) / 47 K (rsqrt64) arguments inside the domain: 20 log-uniform mantissas in every binade, every power of
    two, 1 +- ulp, the ends of the domain and their neighbours, negatives (rcp64), and what jacobi_cs forms: 1 + t^2 with t in
    [0, 1] and h in [1, 1e200]."""
    rng = np.random.default_rng(11 + rsq)
    lo, hi = RSQRT_DOMAIN if rsq else RCP_DOMAIN
    e_hi = 1023 if rsq else 1021
    exps = np.arange(-1022, e_hi + 1)
    body = np.ldexp(2.0 ** rng.uniform(0, 1, (len(exps), 20)), exps[:, None]).ravel()
    body = body[(body >= lo) & (body <= hi)]
    pow2 = np.ldexp(1.0, np.arange(-1022, (1023 if rsq else 1022) + 1))
    near_one = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)])
    ends = np.array([lo, np.nextafter(lo, 1.0), hi, np.nextafter(hi, 0.0)])
    t = np.concatenate([[0.0, 1.0], rng.uniform(0, 1, 2000)])
    h = 10.0 ** rng.uniform(0, 200, 2000)
    x = np.concatenate([body, pow2, near_one, ends, 1.0 + t * t, h])
    if not rsq:
        x = np.concatenate([x, -x[::5]])
    assert (np.abs(x) >= lo).all() and (np.abs(x) <= hi).all() and len(x) <= 65536
    return x


def recip_truth(x, rsq):
    """1 / x or 1 / sqrt(x) rounded once to double from 64 (or more) bits."""
    x = np.asarray(x, float)
    if EXTENDED:
        X = x.astype(LD)
        return ((1 / np.sqrt(X)) if rsq else (1 / X)).astype(float)
    mpmath.mp.prec = 120
    return np.array([float(1 / mpmath.sqrt(mpmath.mpf(v)) if rsq else 1 / mpmath.mpf(v)) for v in x])


def recip_error(x, got, rsq):
    """(relative error, error in ulp of the correctly rounded result) of got against the truth."""
    x, got = np.asarray(x, float), np.asarray(got, float)
    if EXTENDED:
        X = x.astype(LD)
        t = (1 / np.sqrt(X)) if rsq else (1 / X)
        d = np.abs(got.astype(LD) - t)
        rel = (d / np.abs(t)).astype(float)
        ulp = (d / np.spacing(np.abs(t.astype(float))).astype(LD)).astype(float)
        return np.where(np.isfinite(got), rel, np.inf), np.where(np.isfinite(got), ulp, np.inf)
    mpmath.mp.prec = 120
    rel, ulp = np.full(len(x), np.inf), np.full(len(x), np.inf)
    for i, (v, g) in enumerate(zip(x, got)):
        if np.isfinite(g):
            t = 1 / mpmath.sqrt(mpmath.mpf(v)) if rsq else 1 / mpmath.mpf(v)
            d = abs(mpmath.mpf(g) - t)
            rel[i], ulp[i] = float(d / abs(t)), float(d / mpmath.mpf(float(np.spacing(abs(float(t))))))
    return rel, ulp


def recip_check(x, got, rsq):
    rel, _ = recip_error(x, got, rsq)
    return [("rsqrt64 relative error" if rsq else "rcp64 relative error", rel, RCP_BOUND)]


# what the two functions do outside the domain (the header's sentences; test_linalg_device.py holds the device to them)
def recip_specials(rsq):
    """[(what, arguments, expected)].  expected: "nan"; "bound" (finite and within RCP_BOUND of the truth); "denormal" (within two
    denormal ulps, 2^-1073, of the truth: the Newton steps round to the denormal grid); "2.25" (2.25 times the truth: 0.5 * x
    underflows to zero, and each of the two steps multiplies the seed by 1.5)."""
    d_finite = np.array([1.5 * 2.0 ** -1024, 2.0 ** -1023, 1.5 * 2.0 ** -1023, np.nextafter(TINY, 0.0)])
    d_overflow = np.array([5e-324, 2.0 ** -1030, 2.0 ** -1025, 2.0 ** -1024])
    big = np.array([np.nextafter(2.0 ** 1022, np.inf), 1.5 * 2.0 ** 1022, 2.0 ** 1023, 1.5 * 2.0 ** 1023, HUGE])
    if rsq:
        return [("+-0", np.array([0.0, -0.0]), "nan"), ("+inf", np.array([np.inf]), "nan"), ("NaN", np.array([np.nan]), "nan"),
                ("negative", np.array([-1.0, -TINY, -5e-324, -np.inf]), "nan"),
                ("denormal powers of two above the smallest", np.array([2.0 ** -1030, 2.0 ** -1024, 2.0 ** -1072]), "bound"),
                ("the smallest denormal", np.array([5e-324]), "2.25")]
    return [("+-0", np.array([0.0, -0.0]), "nan"), ("+-inf", np.array([np.inf, -np.inf]), "nan"), ("NaN", np.array([np.nan]), "nan"),
            ("denormals whose reciprocal overflows", np.concatenate([d_overflow, -d_overflow]), "nan"),
            ("denormals whose reciprocal is finite", np.concatenate([d_finite, -d_finite]), "bound"),
            ("arguments whose reciprocal is denormal", np.concatenate([big, -big]), "denormal")]


# ------------------------------------------------------------------------------------------------ jacobi_cs
JACOBI_GATE = 1e-28


def jacobi_gate(a, b, g):
    """The gate in the device's own arithmetic (plain double operations, no contraction)."""
    with np.errstate(all="ignore"):
        return g * g > JACOBI_GATE * (a * b)


@functools.lru_cache(None)
def jacobi_cases():
    """{name: [n][3] (alpha, beta, gamma)}"""
    rng = np.random.default_rng(21)
    c = {}
    c["alpha == beta"] = np.array([[2.0, 2.0, 0.3], [2.0, 2.0, -0.3], [1e-7, 1e-7, 1e-9], [5.0, 5.0, -4.999]])
    c["signs"] = np.array([[a, b, g] for a, b in ((1.0, 3.0), (3.0, 1.0), (1.0, 1.0 + 1e-9), (1.0 + 1e-9, 1.0)) for g in (0.5, -0.5, 1e-6, -1e-6)])
    n = 2000
    a, b = 10.0 ** rng.uniform(-10, 10, n), 10.0 ** rng.uniform(-10, 10, n)
    rho = 10.0 ** rng.uniform(-13, 0, n) * rng.choice([-1.0, 1.0], n)
    c["random"] = np.stack([a, b, rho * np.sqrt(a * b)], 1)
    # gamma^2 one ulp either side of the gate (and a few more): the k-th neighbour of sqrt(1e-28 alpha beta), both signs
    rows = []
    for a, b in ((1.0, 1.0), (3.0, 7.0), (1e-7, 2e5), (0.1, 0.1), (123.456, 0.789), (2.0 ** -400, 2.0 ** -400), (2.0 ** 400, 2.0 ** 400)):
        g0 = float(np.sqrt(JACOBI_GATE * (a * b)))
        for sgn in (1.0, -1.0):
            g = g0
            for _ in range(4):
                g = np.nextafter(g, 0.0)
            for _ in range(9):
                rows.append([a, b, sgn * g])
                g = np.nextafter(g, np.inf)
    c["gate"] = np.array(rows)
    # |zeta| >= 1e100: t = 1 / (2 |zeta|); either side of the branch
    c["large zeta"] = np.array([[1e-300, 1.0, 1e-120], [1.0, 1e-300, 1e-120], [1e-300, 1.0, -1e-120], [1.0, 1e-300, -1e-120],
                                [0.0, 1.0, 0.5e-100 * (1 + 1e-3)], [0.0, 1.0, 0.5e-100 * (1 - 1e-3)], [1.0, 0.0, -0.5e-100 * (1 + 1e-3)],
                                [1.0, 0.0, 0.5e-100 * (1 - 1e-3)], [0.0, 1.0, 1e-99], [0.0, 1.0, 1e-101]])
    # the ends of the stated range: columns of norm 2^-200 and 2^200
    base = c["random"][:200]
    c["columns of norm 2^-200"] = base * 2.0 ** -400
    c["columns of norm 2^200"] = base * 2.0 ** 400
    return c


def jacobi_truth(rows):
    """(t, c, s) in mpmath: t the smaller root of t^2 + 2 zeta t - 1 (sign of zeta; +1 at zeta = 0), c = 1 / sqrt(1 + t^2), s = c t."""
    mpmath.mp.prec = 200
    out = []
    for a, b, g in rows:
        zeta = (mpmath.mpf(b) - mpmath.mpf(a)) / (2 * mpmath.mpf(g))
        t = 1 / (abs(zeta) + mpmath.sqrt(1 + zeta * zeta))
        if zeta < 0:
            t = -t
        c = 1 / mpmath.sqrt(1 + t * t)
        out.append((t, c, c * t))
    return out


def jacobi_reference(rows, prefill):
    """The truth rounded to double, the prefill where the gate says no: [n][3] (c, s, flag)."""
    rows = np.asarray(rows, float)
    out = np.full((len(rows), 3), float(prefill))
    flag = jacobi_gate(rows[:, 0], rows[:, 1], rows[:, 2])
    out[:, 2] = flag
    for i, (t, c, s) in zip(np.nonzero(flag)[0], jacobi_truth(rows[flag])):
        out[i, 0], out[i, 1] = float(c), float(s)
    return out


def jacobi_check(rows, out):
    """Rows where the routine rotated (out[:, 2] == 1): t = s / c, c and s against the truth, 8 eps relative; |c^2 + s^2 - 1| <= 4 eps."""
    rows, out = np.asarray(rows, float), np.asarray(out, float)
    on = out[:, 2] == 1
    et, ec, es, eu = [], [], [], []
    mpmath.mp.prec = 200
    for (t, c, s), (cd, sd, _) in zip(jacobi_truth(rows[on]), out[on]):
        if not (np.isfinite(cd) and np.isfinite(sd)) or cd == 0:
            et.append(np.inf); ec.append(np.inf); es.append(np.inf); eu.append(np.inf)
            continue
        cd, sd = mpmath.mpf(cd), mpmath.mpf(sd)
        et.append(float(abs(sd / cd - t) / abs(t)))
        ec.append(float(abs(cd - c) / c))
        es.append(float(abs(sd - s) / abs(s)))
        eu.append(float(abs(cd * cd + sd * sd - 1)))
    return [("jacobi_cs t", et, 8 * EPS), ("jacobi_cs c", ec, 8 * EPS), ("jacobi_cs s", es, 8 * EPS), ("jacobi_cs c^2 + s^2 - 1", eu, 4 * EPS)]


# ------------------------------------------------------------------------------------------------ svd3
ORTHO_GATE = 1e-14          # jacobi_cs: a pair is orthogonal when its cosine is below this
SVD3_SCALES = (-200, -60, 0, 60, 200)


def rotation(rng, max_deg=180.0):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = np.radians(rng.uniform(-max_deg, max_deg))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


@functools.lru_cache(None)
def svd3_cases():
    """{name: [n][3][3]}; the names 'rank 1' and 'zero' are the degenerate ones (no orthonormal U asked)."""
    rng = np.random.default_rng(31)
    c = {}
    c["random"] = rng.normal(size=(1500, 3, 3))
    R = np.stack([rotation(rng) for _ in range(100)])
    c["rotations"] = R
    c["reflections"] = R * np.array([1.0, 1.0, -1.0])[None, None, :]
    c["identity and permutations"] = np.stack([np.eye(3)[list(p)] for p in itertools.permutations(range(3))])
    c["diagonal, six orderings"] = np.stack([np.diag(p) for p in itertools.permutations((5.0, 2.0, 0.25))] +
                                            [np.diag(p) for p in itertools.permutations((-5.0, 2.0, 0.25))])
    two = []
    for _ in range(100):
        U, V = rotation(rng), rotation(rng)
        for w in ((3.0, 3.0, 1.0), (3.0, 1.0, 1.0), (2.0, 2.0, 0.0)):
            two.append(U @ np.diag(w) @ V.T)
    c["two equal singular values"] = np.stack(two)
    c["essential matrices"] = np.stack([skew(rng.normal(size=3)) @ rotation(rng, 40) for _ in range(200)])
    # what k_tv_hypotheses makes of the eight-point vector: U diag(w0, w1, 0) V^T of a float-rounded 3 x 3
    r2 = []
    for _ in range(200):
        F = rng.normal(size=(3, 3)).astype(np.float32).astype(float)
        U, w, Vt = np.linalg.svd(F)
        r2.append((U * np.array([w[0], w[1], 0.0])) @ Vt)
    c["rank 2, third value zeroed"] = np.stack(r2)
    c["rank 2, integer"] = np.stack([np.outer(a, b) + np.outer(d, e) for a, b, d, e in rng.integers(-4, 5, (60, 4, 3)).astype(float)
                                     if np.linalg.matrix_rank(np.outer(a, b) + np.outer(d, e)) == 2])
    r1 = [np.outer(a, b) for a, b in rng.integers(-4, 5, (80, 2, 3)).astype(float) if a.any() and b.any()]
    r1 += [np.outer(rng.normal(size=3), rng.normal(size=3)) for _ in range(40)]
    r1 += [np.diag(p) for p in ((3.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 3.0))]
    c["rank 1"] = np.stack(r1)
    c["zero"] = np.zeros((1, 3, 3))
    base = c["random"][:200]
    for k in SVD3_SCALES:
        if k:
            c["random, scaled by 2^%d" % k] = base * 2.0 ** k
            c["essential matrices, scaled by 2^%d" % k] = c["essential matrices"][:50] * 2.0 ** k
    return c


def svd3_reference(A):
    """A decomposition good to the last bit of a double, in the routine's output layout [n][21] (U, w, V) and with its conventions
    (w descending, zero columns of U under a zero w, U2 = U0 x U1 along A V2): a one-sided Jacobi in longdouble with its gate at
    1e-19, rounded once.  LAPACK's own U and V are orthonormal to a few ulp only, which is most of the bounds below; numpy's
    singular values stay the truth that w is held to (svd3_check)."""
    B = np.asarray(A, float).reshape(-1, 3, 3).astype(LD)
    n = len(B)
    V = np.tile(np.eye(3, dtype=LD), (n, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(60):
            rotated = False
            for p, q in ((0, 1), (0, 2), (1, 2)):
                al, be, ga = (B[:, :, p] ** 2).sum(1), (B[:, :, q] ** 2).sum(1), (B[:, :, p] * B[:, :, q]).sum(1)
                m = ga * ga > LD(1e-38) * (al * be)
                if not m.any():
                    continue
                rotated = True
                zeta = np.where(m, (be - al) / (2 * np.where(m, ga, 1)), LD(0))
                t = np.where(zeta < 0, LD(-1), LD(1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = np.where(m, 1 / np.sqrt(1 + t * t), LD(1))
                s = np.where(m, c * t, LD(0))
                for M in (B, V):
                    mp_, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = c[:, None] * mp_ - s[:, None] * mq
                    M[:, :, q] = s[:, None] * mp_ + c[:, None] * mq
            if not rotated:
                break
        nrm = (B ** 2).sum(1)
        order = np.argsort(-nrm, axis=1, kind="stable")
        B = np.take_along_axis(B, order[:, None, :], 2)
        V = np.take_along_axis(V, order[:, None, :], 2)
        w = np.sqrt(np.take_along_axis(nrm, order, 1))
        U = np.zeros_like(B)
        for j in range(2):
            U[:, :, j] = np.where(w[:, j, None] > 0, B[:, :, j] / np.where(w[:, j, None] > 0, w[:, j, None], 1), 0)
        U = U.astype(float).astype(LD)                       # the cross product is taken of the doubles that are returned
        u2 = np.cross(U[:, :, 0], U[:, :, 1])
        U[:, :, 2] = np.where(((u2 * B[:, :, 2]).sum(1) < 0)[:, None], -u2, u2)
    return np.concatenate([U.reshape(-1, 9), w, V.reshape(-1, 9)], 1).astype(float)


def _ld(a):
    return np.asarray(a, float).astype(LD)


def svd3_check(A, out, degenerate=False):
    """degenerate (rank 1, zero): the reconstruction, w, V and finiteness only."""
    A = np.asarray(A, float).reshape(-1, 3, 3)
    out = np.asarray(out, float)
    U, w, V = out[:, :9].reshape(-1, 3, 3), out[:, 9:12], out[:, 12:].reshape(-1, 3, 3)
    s = np.linalg.svd(A)[1]
    truth = svd3_reference(A)[:, 9:12]
    normA = np.sqrt((A * A).sum((1, 2)))
    I = np.eye(3)
    with np.errstate(all="ignore"):
        rows = [("svd3 not finite", (~np.isfinite(out)).sum(1), 0.5),
                ("svd3 w not descending", ((w[:, 0] < w[:, 1]) | (w[:, 1] < w[:, 2]) | (w[:, 2] < 0)).astype(float), 0.5),
                ("svd3 |w - s|, s numpy's", np.abs(w - s).max(1), 8 * EPS * s[:, 0]),
                ("svd3 |w - s|, s in longdouble", np.abs(w - truth).max(1), 8 * EPS * truth[:, 0])]
        rec = np.einsum("nij,nj,nkj->nik", _ld(U), _ld(w), _ld(V)) - _ld(A)
        # 16 eps |A| of rounding, and what the third left vector costs: U2 is U0 x U1, not the rotated third column, and the
        # sweeps stop with the cosines of (0, 2) and (1, 2) anywhere below the gate, so U2 w2 is off that column by up to
        # sqrt(2) * 1e-14 * w2 (HISTORY.md: 16 eps |A| alone leaves this out, and one matrix in 1500 exceeded it on the device)
        rows.append(("svd3 reconstruction", np.sqrt((rec * rec).sum((1, 2))).astype(float), 16 * EPS * normA + np.sqrt(2) * ORTHO_GATE * w[:, 2]))
        VtV = np.einsum("nji,njk->nik", _ld(V), _ld(V)) - I
        rows.append(("svd3 V^T V - I", np.sqrt((VtV * VtV).sum((1, 2))).astype(float), 4 * ORTHO_GATE))
        if degenerate:
            return rows
        UtU = np.einsum("nji,njk->nik", _ld(U), _ld(U)) - I
        m = w[:, 1] > 0
        rows.append(("svd3 U^T U - I", np.where(m, np.sqrt((UtU * UtU).sum((1, 2))).astype(float), 0.0),
                     np.where(m, 4 * ORTHO_GATE + 16 * EPS * w[:, 0] / np.where(m, w[:, 1], 1.0), 1.0)))
        # the third left vector: U0 x U1 up to its sign, and along A V2 wherever w2 is above the rounding of A V2 itself
        cr = np.cross(U[:, :, 0], U[:, :, 1])
        d = np.minimum(np.abs(U[:, :, 2] - cr).max(1), np.abs(U[:, :, 2] + cr).max(1))
        rows.append(("svd3 U2 = +-(U0 x U1)", d, 4 * EPS))
        av2 = np.einsum("nij,nj->ni", A, V[:, :, 2])
        along = (U[:, :, 2] * av2).sum(1)
        clear = w[:, 2] > 1e-10 * w[:, 0]
        rows.append(("svd3 U2 against A V2", (clear & ~(along > 0)).astype(float), 0.5))
    return rows


# ------------------------------------------------------------------------------------------------ null_vector4
def null_vector4_restated(A):
    """null_vector4 of csrc/orbx_linalg.h in numpy: the same operations in the same order in double, 1 / x for rcp64 and
    1 / sqrt(x) for rsqrt64.  Returns (v [n][4] float32, iterations [n])."""
    A = np.asarray(A, np.float32).reshape(-1, 4, 4).astype(float)
    n = len(A)
    with np.errstate(all="ignore"):
        B = {}
        for i in range(4):
            for j in range(i, 4):
                s = np.zeros(n)
                for k in range(4):
                    s = A[:, k, i] * A[:, k, j] + s      # (the products of two floats are exact in double: an fma adds nothing)
                B[i, j] = s
        mu = 1e-14 * (B[0, 0] + B[1, 1] + B[2, 2] + B[3, 3]) + 1e-300
        d0 = B[0, 0] + mu
        id0 = 1 / d0
        L10, L20, L30 = B[0, 1] * id0, B[0, 2] * id0, B[0, 3] * id0
        d1 = B[1, 1] + mu - L10 * B[0, 1]
        id1 = 1 / d1
        t21, t31 = B[1, 2] - L10 * B[0, 2], B[1, 3] - L10 * B[0, 3]
        L21, L31 = t21 * id1, t31 * id1
        d2 = B[2, 2] + mu - L20 * B[0, 2] - L21 * t21
        id2 = 1 / d2
        t32 = B[2, 3] - L20 * B[0, 3] - L21 * t31
        L32 = t32 * id2
        d3 = B[3, 3] + mu - L30 * B[0, 3] - L31 * t31 - L32 * t32
        id3 = 1 / d3
        x = np.full((4, n), 0.5)
        active = np.ones(n, bool)
        its = np.zeros(n, int)
        for it in range(30):
            x0, x1, x2, x3 = x
            y0 = x0
            y1 = x1 - L10 * y0
            y2 = x2 - L20 * y0 - L21 * y1
            y3 = x3 - L30 * y0 - L31 * y1 - L32 * y2
            w3 = y3 * id3
            w2 = y2 * id2 - L32 * w3
            w1 = y1 * id1 - L21 * w2 - L31 * w3
            w0 = y0 * id0 - L10 * w1 - L20 * w2 - L30 * w3
            rn = 1 / np.sqrt(w0 * w0 + w1 * w1 + w2 * w2 + w3 * w3)
            nx = np.stack([w0 * rn, w1 * rn, w2 * rn, w3 * rn])
            dx = np.abs(nx[0] - x0) + np.abs(nx[1] - x1) + np.abs(nx[2] - x2) + np.abs(nx[3] - x3)
            x = np.where(active, nx, x)
            its += active
            if it > 0:
                active = active & ~(dx < 1e-13)
            if not active.any():
                break
        return x.T.astype(np.float32), its


def _tri_rows(obs, P):
    """The two DLT rows of one camera in float: obs.x * P[2] - P[0], obs.y * P[2] - P[1]."""
    obs, P = np.asarray(obs, np.float32), np.asarray(P, np.float32)
    return np.stack([obs[0] * P[2] - P[0], obs[1] * P[2] - P[1]])


def triangulation_system(rng, parallax_deg, pixel, noise):
    """A 4 x 4 system as kb8_triangulate_matches / np_one_match (normalised coordinates, rows of [R | t]) or k_tv_check_rt (pixel
    coordinates, rows of K [R | t]) build it, for a point seen under the given parallax."""
    depth = rng.uniform(2.0, 20.0)
    X = depth * np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), 1.0])
    perp = np.cross(X, rng.normal(size=3))
    perp /= np.linalg.norm(perp)
    C = perp * 2 * np.linalg.norm(X) * np.tan(np.radians(parallax_deg) / 2)      # the second centre: the rays meet under the parallax
    C += X / np.linalg.norm(X) * np.linalg.norm(C) * rng.uniform(-0.2, 0.2)
    R = rotation(rng, 10)
    T1 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    T2 = np.concatenate([R, (-R @ C)[:, None]], 1)
    K = np.array([[rng.uniform(400, 700), 0, rng.uniform(300, 340)], [0, rng.uniform(400, 700), rng.uniform(220, 260)], [0, 0, 1.0]])
    rows = []
    for T in (T1, T2):
        xc = T[:, :3] @ X + T[:, 3]
        xn = xc[:2] / xc[2] + noise * rng.normal(size=2)
        if pixel:
            rows.append(_tri_rows(K[:2, :2] @ xn + K[:2, 2], (K @ T).astype(np.float32)))
        else:
            rows.append(_tri_rows(xn, T.astype(np.float32)))
    return np.concatenate(rows).astype(np.float32)


# cosParallaxRays > 0.9998 returns (KannalaBrandt8.cpp:356, LocalMapping.cc:604): 1.146 degrees; two-view: 0.99998, 0.362 degrees
PARALLAX_NORMALISED = (1.15, 1.7, 3.0, 5.0, 10.0, 20.0, 30.0)
PARALLAX_PIXEL = (0.37, 1.15, 3.0, 10.0, 30.0)
NULL4_SCALES = (-60, -20, 20, 60)


@functools.lru_cache(None)
def null4_cases():
    """{name: [n][4][4] float32}.  'rank 2' and 'zero' are named in the tests: only the residual and finiteness are asked of the
    first, and the second is outside the domain."""
    rng = np.random.default_rng(41)
    c = {}
    for par in PARALLAX_NORMALISED:
        c["normalised, parallax %g" % par] = np.stack([triangulation_system(rng, par, False, nz) for nz in (0.0, 1e-3) for _ in range(40)])
    for par in PARALLAX_PIXEL:
        c["pixel, parallax %g" % par] = np.stack([triangulation_system(rng, par, True, nz) for nz in (0.0, 1e-3) for _ in range(40)])
    # null vectors exactly orthogonal to the start vector (1/2, 1/2, 1/2, 1/2)
    c["null vector (1, 1, -1, -1) / 2, integer rows"] = np.array([[[1, 0, 1, 0], [0, 1, 0, 1], [1, -1, 0, 0], [2, -1, 3, -2]],
                                                                  [[1, 0, 0, 1], [0, 1, 1, 0], [3, -3, 1, -1], [1, 1, 1, 1]],
                                                                  [[5, -2, 1, 2], [1, 2, 2, 1], [0, 1, 0, 1], [-4, 1, -1, -2]]], np.float32)
    c["null vector (1, -1, 0, 0) / sqrt 2, integer rows"] = np.array([[[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 2, -3]],
                                                                      [[2, 2, 1, 0], [1, 1, 0, 3], [-1, -1, 2, 2], [3, 3, 3, 3]]], np.float32)
    for name, nv in (("(1, 1, -1, -1) / 2", np.array([0.5, 0.5, -0.5, -0.5])), ("(1, -1, 0, 0) / sqrt 2", np.array([1, -1, 0, 0]) / np.sqrt(2))):
        ms = []
        for _ in range(20):
            Q, _ = np.linalg.qr(np.concatenate([nv[:, None], rng.normal(size=(4, 3))], 1))     # Q[:, 0] = +-nv
            ms.append((rng.normal(size=(4, 3)) @ Q[:, 1:].T).astype(np.float32))
        c["null vector %s, rounded orthogonal basis" % name] = np.stack(ms)
    z = []
    for j in range(4):
        for _ in range(5):
            M = rng.normal(size=(4, 4)).astype(np.float32)
            M[:, j] = 0
            z.append(M)
    c["a zero column"] = np.stack(z)
    # exact rank 2: a pair without parallax (the same camera twice), and integer rows
    r2 = []
    for _ in range(10):
        x, y = rng.uniform(-0.5, 0.5, 2).astype(np.float32)
        r2.append(np.array([[-1, 0, x, 0], [0, -1, y, 0], [-1, 0, x, 0], [0, -1, y, 0]], np.float32))
    for _ in range(10):
        a, b = rng.integers(-3, 4, (2, 4)).astype(np.float32)
        M = np.stack([a, b, a + b, a - 2 * b])
        if np.linalg.matrix_rank(M.astype(float)) == 2:
            r2.append(M)
    c["rank 2"] = np.stack(r2)
    base = np.concatenate([c["normalised, parallax 3"][30:50], c["pixel, parallax 3"][30:50]])
    for k in NULL4_SCALES:
        c["scaled by 2^%d" % k] = (base * np.float32(2.0 ** k)).astype(np.float32)
    # the ends of the domain: one denormal entry, and entries near the largest float
    one = np.zeros((4, 4), np.float32)
    one[2, 1] = np.float32(1e-45)
    c["smallest and largest floats"] = np.stack([one, (base[0] / np.abs(base[0]).max() * np.float32(3e38)).astype(np.float32),
                                                 (base[25] / np.abs(base[25]).max() * np.float32(3e38)).astype(np.float32)])
    c["zero"] = np.zeros((1, 4, 4), np.float32)
    return c


def null4_check(A, v, residual_only=False):
    A = np.asarray(A, np.float32).reshape(-1, 4, 4).astype(float)
    v = np.asarray(v, np.float32).reshape(-1, 4).astype(float)
    _, s, Vt = np.linalg.svd(A)
    with np.errstate(all="ignore"):
        res = np.sqrt((np.einsum("nij,nj->ni", _ld(A), _ld(v)) ** 2).sum(1)).astype(float)
        nrm = np.sqrt((_ld(v) ** 2).sum(1)).astype(float)
        rows = [("null_vector4 not finite", (~np.isfinite(v)).sum(1), 0.5),
                ("null_vector4 residual - s4", np.maximum(res - s[:, 3], 0.0), 2.0 ** -23 * s[:, 0]),
                ("null_vector4 norm", np.abs(nrm - 1), 2.0 ** -22)]
        if not residual_only:
            ref = Vt[:, 3]
            perp = v / nrm[:, None] - np.sign((ref * v).sum(1))[:, None] * ref      # sine of the angle, without the cancellation of 1 - cos^2
            sine = np.sqrt((perp ** 2).sum(1))
            m = s[:, 2] >= 10 * s[:, 3]
            bound = 2.0 ** -22 + 8 * EPS * s[:, 0] ** 2 / np.where(m, s[:, 2] ** 2 - s[:, 3] ** 2, 1.0)
            rows.append(("null_vector4 angle", np.where(m, sine, 0.0), np.where(m, bound, 1.0)))
    return rows


# ------------------------------------------------------------------------------------------------ null_vector_sym
NORM_DRIFT = 2.4e-12        # 40 sweeps x 66 pairs x 4 eps of drift in y at worst
SYM_SCALES = (-60, 60)


def pad16(M):
    """A (rows <= 16) x NC matrix as the wave holds it: 16 rows, the missing ones zero."""
    M = np.asarray(M, float)
    out = np.zeros((16, M.shape[1]))
    out[:len(M)] = M
    return out


def eight_point_matrix(rng, noise_px, planar):
    """The Hartley-normalised eight-point rows of k_tv_hypotheses (model 1) in float: eight rows filled, eight zero."""
    n = 8
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), np.full(n, 6.0) if planar else rng.uniform(4, 9, n)], 1)
    R, t = rotation(rng, 8), np.array([rng.uniform(0.3, 0.6), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1]])
    p1 = (K @ X.T).T
    p2 = (K @ (R @ X.T + t[:, None])).T
    p1, p2 = p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]
    p1, p2 = (p1 + noise_px * rng.normal(size=p1.shape)).astype(np.float32), (p2 + noise_px * rng.normal(size=p2.shape)).astype(np.float32)

    def normalise(p):
        m = p.mean(0, dtype=np.float32)
        s = (np.float32(1) / np.abs(p - m).mean(0, dtype=np.float32)).astype(np.float32)
        return ((p - m) * s).astype(np.float32)
    a, b = normalise(p1), normalise(p2)
    u1, v1, u2, v2 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    one = np.ones(n, np.float32)
    rows = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], 1).astype(np.float32)
    return pad16(rows.astype(float))


def mlpnp_gram(rng, planar, noise):
    """A^T A of MLPnP's design matrix (csrc/orbx_mlpnp.hip, steps 3./4.): row 2i + k is n_k (x) (p, 1) with n_0, n_1 a basis of the
    null space of the bearing; 12 unknowns (r11 .. r33, t), or 9 in the planar case (the first column of R drops out with p_x = 0)."""
    n = 30
    R, t = rotation(rng, 60), np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 7)])
    P = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)], 1)
    if planar:
        P[:, 0] = 0.0
    rows = []
    for p in P:
        f = R @ p + t
        f = f / np.linalg.norm(f) + noise * rng.normal(size=3)
        f /= np.linalg.norm(f)
        _, _, Vt = np.linalg.svd(f[None, :])
        pe = np.append(p, 1.0)
        for nk in Vt[1:]:
            full = np.concatenate([np.outer(nk, pe[:3]).ravel(), nk * pe[3]])      # columns (a, b) = 3 a + b, then (a, the 1)
            rows.append(np.concatenate([np.outer(nk, pe[1:3]).ravel(), nk]) if planar else full)
    Ad = np.array(rows)
    G = Ad.T @ Ad
    return pad16((G + G.T) / 2)


def psd_with_gap(rng, nc, gap):
    """A symmetric positive semi-definite matrix whose two smallest eigenvalues lie `gap` (relative to the largest) apart."""
    Q, _ = np.linalg.qr(rng.normal(size=(nc, nc)))
    lam = np.sort(rng.uniform(0.1, 1.0, nc))[::-1].copy()
    lam[0] = 1.0
    lam[-1] = 1e-3
    lam[-2] = 1e-3 + gap
    G = (Q * lam) @ Q.T
    return pad16((G + G.T) / 2)


def nearly_orthogonal_columns(rng, nc, eps=1e-11):
    """U diag(sigma) (I + eps K)^T with K skew: columns whose cosines lie between the gate (1e-14) and 1e-10, so the routine has to
    rotate them although they look orthogonal, and leaving them alone costs eps in the vector: 4 x the angle bound and more."""
    U, _ = np.linalg.qr(rng.normal(size=(16, nc)))
    sigma = np.linspace(1.0, 0.3, nc - 1).tolist() + [0.2]
    K = rng.uniform(-1, 1, (nc, nc))
    K = K - K.T
    return (U * sigma) @ (np.eye(nc) + eps * K).T


@functools.lru_cache(None)
def sym_cases(nc):
    """{name: [n][16][nc]}"""
    rng = np.random.default_rng(50 + nc)
    c = {}
    if nc == 9:
        c["eight-point, exact"] = np.stack([eight_point_matrix(rng, 0.0, False) for _ in range(40)])
        c["eight-point, noisy"] = np.stack([eight_point_matrix(rng, 0.7, False) for _ in range(40)])
        c["eight-point, planar scene"] = np.stack([eight_point_matrix(rng, 0.0, True) for _ in range(20)])
        for k in SYM_SCALES:
            c["eight-point, noisy, scaled by 2^%d" % k] = c["eight-point, noisy"] * 2.0 ** k
    c["MLPnP Gram, exact bearings"] = np.stack([mlpnp_gram(rng, nc == 9, 0.0) for _ in range(20)])
    c["MLPnP Gram, noisy bearings"] = np.stack([mlpnp_gram(rng, nc == 9, 2e-3) for _ in range(20)])
    c["positive semi-definite, gap 1e-8"] = np.stack([psd_with_gap(rng, nc, 1e-8) for _ in range(10)])
    c["positive semi-definite, gap 1e-3"] = np.stack([psd_with_gap(rng, nc, 1e-3) for _ in range(10)])
    c["columns orthogonal to between 1e-14 and 1e-10"] = np.stack([nearly_orthogonal_columns(rng, nc) for _ in range(10)])
    row = rng.normal(size=nc)
    c["identical rows"] = np.stack([np.tile(row, (16, 1)), np.tile(np.arange(1.0, nc + 1), (16, 1))])
    c["zero"] = np.zeros((1, 16, nc))
    return c


def sym_reference(A):
    """numpy's right singular vector of the smallest singular value, four times over: [n][4 * NC]."""
    A = np.asarray(A, float)
    Vt = np.linalg.svd(A)[2]
    return np.tile(Vt[:, -1], (1, 4))


def sym_check(A, out):
    A = np.asarray(A, float)
    nc = A.shape[2]
    out = np.asarray(out, float).reshape(len(A), 4, nc)
    v = out[:, 0]
    _, s, Vt = np.linalg.svd(A)
    tag = "null_vector_sym<%d> " % nc
    with np.errstate(all="ignore"):
        res = np.sqrt((np.einsum("nij,nj->ni", _ld(A), _ld(v)) ** 2).sum(1)).astype(float)
        nrm = np.sqrt((_ld(v) ** 2).sum(1)).astype(float)
        ref = Vt[:, -1]
        sg = np.sign((ref * v).sum(1))
        perp = v / nrm[:, None] - sg[:, None] * ref
        sine = np.sqrt((perp ** 2).sum(1))
        gap = s[:, -2] - s[:, -1]
        m = gap > 1e-6 * s[:, 0]
        same = np.array([len({out[i, k].tobytes() for k in range(4)}) - 1 for i in range(len(A))], float)
        return [(tag + "not finite", (~np.isfinite(out)).sum((1, 2)), 0.5),
                (tag + "lanes 0, 17, 34, 63 differ", same, 0.5),
                (tag + "residual - s_min", np.maximum(res - s[:, -1], 0.0), nc * (ORTHO_GATE + 8 * EPS) * s[:, 0]),
                (tag + "norm", np.abs(nrm - 1), NORM_DRIFT),
                (tag + "angle", np.where(m, sine, 0.0), np.where(m, nc * 4 * ORTHO_GATE * s[:, 0] / np.where(m, gap, 1.0), 1.0))]


# ------------------------------------------------------------------------------------------------ ldlt6 / ldlt7
LAMBDAS = (0.0, 1e-8, 1.0, 1e6)
PREFILL = 7.0


def pack_upper(H):
    return np.asarray(H, float)[np.triu_indices(len(H))]


def unpack_upper(h, n):
    H = np.zeros((n, n))
    H[np.triu_indices(n)] = h
    return H + np.triu(H, 1).T


def spd(rng, n, spread=False):
    M = rng.normal(size=(n, n + 3))
    H = M @ M.T + 0.05 * np.eye(n)
    if spread:       # a pose Hessian: rotation rows 1e3 times the translation rows, 1e6 between the diagonal blocks
        D = np.diag([1e3] * 3 + [1.0] * (n - 3))
        H = D @ H @ D
    assert len(set(pack_upper(H).tolist())) == n * (n + 1) // 2          # every packed entry distinct: a wrong index shows
    return H


@functools.lru_cache(None)
def ldlt_systems(n):
    """[(name, H, b, lambda)]: systems that must solve."""
    rng = np.random.default_rng(60 + n)
    out = []
    for lam in LAMBDAS:
        for k in range(6):
            out.append(("random, lambda %g" % lam, spd(rng, n), rng.normal(size=n), lam))
        out.append(("1e6 scale spread, lambda %g" % lam, spd(rng, n, True), rng.normal(size=n) * np.array([1e3] * 3 + [1.0] * (n - 3)), lam))
    v = rng.normal(size=n)
    out.append(("singular positive semi-definite, lambda 1", np.outer(v, v), rng.normal(size=n), 1.0))
    out.append(("singular positive semi-definite, lambda 1e-8", np.outer(v, v), rng.normal(size=n), 1e-8))
    out.append(("zero matrix, lambda 1", np.zeros((n, n)), rng.normal(size=n), 1.0))
    return out


@functools.lru_cache(None)
def ldlt_failures(n):
    """[(name, H, b, lambda)]: systems on which the unpivoted LDLT must report a failed pivot (lambda 0 unless named)."""
    rng = np.random.default_rng(70 + n)
    out = []
    b = rng.normal(size=n)
    for j in range(n):
        for piv in (-1.0, 0.0):
            L = np.tril(rng.integers(-2, 3, (n, n)).astype(float), -1) + np.eye(n)
            d = rng.integers(1, 5, n).astype(float)
            d[j] = piv
            out.append(("pivot %g first at position %d" % (piv, j), (L * d) @ L.T, b, 0.0))       # small integers: the factors are exact
    H = spd(rng, n)
    for name, (i, k, val) in (("NaN on the diagonal", (2, 2, np.nan)), ("NaN off the diagonal", (1, n - 1, np.nan)),
                              ("inf on the diagonal", (n - 1, n - 1, np.inf)), ("inf off the diagonal", (0, 3, np.inf)),
                              ("-inf on the diagonal", (0, 0, -np.inf)), ("-0.0 first pivot", (0, 0, -0.0))):
        M = H.copy()
        M[i, k] = M[k, i] = val
        out.append((name, M, b, 0.0))
    M = np.diag(np.arange(1.0, n + 1))
    M[n - 1, n - 1] = -0.0
    out.append(("-0.0 last pivot", M, b, 0.0))
    out.append(("zero matrix, lambda 0", np.zeros((n, n)), b, 0.0))
    out.append(("negative definite, lambda 1", -spd(rng, n) - 2 * np.eye(n), b, 1.0))
    return out


def ldlt_residual(H, x, b):
    with np.errstate(all="ignore"):
        return float(np.linalg.norm(H @ x - b) / (np.linalg.norm(H, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


def ldlt_items(systems, with_lambda):
    return np.stack([np.concatenate([pack_upper(H), b, [lam] if with_lambda else []]) for _, H, b, lam in systems])


# ------------------------------------------------------------------------------------------------ sum16
@functools.lru_cache(None)
def sum16_inputs(n_waves=8):
    """64 distinct values per wave, magnitudes over 1e-8 .. 1e8 and both signs: the order of the additions shows in the last bits."""
    rng = np.random.default_rng(80)
    v = 10.0 ** rng.uniform(-8, 8, (n_waves, 64)) * rng.choice([-1.0, 1.0], (n_waves, 64))
    assert all(len(set(w.tolist())) == 64 for w in v)
    return v


def sum16_xor_tree(v):
    """v += v[lane ^ off] for off = 8, 4, 2, 1, in double: what every lane holds afterwards."""
    v = np.array(v, float)
    lane = np.arange(64)
    for off in (8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    return v


# ------------------------------------------------------------------------------------------------ huber (csrc/orbx_optim.h)
DELTA_MONO = float(np.float32(np.sqrt(5.991)))          # the project's two Huber deltas, as the reference holds them: floats
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))


@functools.lru_cache(None)
def huber_items():
    """Rows of (robust, chi2, delta): chi2 at delta^2 and its two neighbours, 0, inf, NaN, ordinary values on both sides, and a
    large chi2 without a kernel, for both deltas."""
    rows = []
    for d in (DELTA_MONO, DELTA_STEREO):
        d2 = d * d
        for chi in (d2, np.nextafter(d2, np.inf), np.nextafter(d2, -np.inf), 0.0, np.inf, np.nan, 0.37, 2.0 * d2, 1234.5678, 1e300, TINY):
            rows.append((1.0, chi, d))
        rows += [(0.0, 1e12, d), (0.0, np.nextafter(d2, np.inf), d), (0.0, np.nan, d)]
    return np.array(rows)


def huber_reference(items):
    """RobustKernelHuber::robustify in double, operation by operation: each one is correctly rounded here and on the device."""
    out = np.empty((len(items), 2))
    with np.errstate(all="ignore"):
        for i, (robust, chi, d) in enumerate(items):
            rho0, rho1 = np.float64(chi), np.float64(1.0)
            dsqr = np.float64(d) * np.float64(d)
            if robust != 0 and not chi <= dsqr:
                sq = np.sqrt(np.float64(chi))
                rho0 = np.float64(2.0) * sq * np.float64(d) - dsqr
                rho1 = np.float64(d) / sq
            out[i] = rho0, rho1
    return out


def same_bits(a, b):
    """Equal bit for bit; a NaN equals any NaN (its sign and payload are not arithmetic)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


# ------------------------------------------------------------------------------------------------ lm_step (csrc/orbx_optim.h)
LM_RETRY, LM_NEXT, LM_STOP = 0, 1, 2
STOP_ITERATIONS, STOP_QMAX, STOP_RHO_ZERO, STOP_SMALL_GAIN = 0, 1, 2, 3
LM_CLAMP_EDGES = ((1 + (1 / 3) ** (1 / 3)) / 2, (1 + (2 / 3) ** (1 / 3)) / 2)       # rho at alpha = 2/3 and at alpha = 1/3
LM_POW_BOUND = 3e-14          # 64 ulp of pow on p in [1/3, 2/3] through 1 - p: 64 * 2^-52 * p / (1 - p) <= 2.9e-14
DBL_MAX = HUGE


def lm_step_reference(item):
    """optimization_algorithm_levenberg.cpp:123-168 and the test of optimize()'s loop on one item of ORBX_LINALG_LM_STEP, in double."""
    f = np.float64
    lam, ni, cur, ini = (f(v) for v in item[:4])
    it, qmax, nbad = (int(v) for v in item[4:7])
    temp, ok, scale_sum, max_iter = f(item[7]), item[8] != 0, f(item[9]), int(item[10])
    with np.errstate(all="ignore"):
        if not ok:
            temp = f(DBL_MAX)
        rho = (cur - temp) / (scale_sum + f(1e-3))
        accepted = bool(rho > 0 and np.isfinite(temp))
        if accepted:
            alpha = f(1.0) - np.power(f(2.0) * rho - f(1.0), 3)
            alpha = min(alpha, f(2.0) / f(3.0))
            lam = lam * max(f(1.0) / f(3.0), alpha)
            ni = f(2.0)
            cur = temp
        else:
            lam = lam * ni
            ni = ni * f(2.0)
        qmax += 1
        nxt, reason = LM_STOP, -1
        if rho < 0 and qmax < 10:
            nxt = LM_RETRY
        else:
            if qmax == 10:
                reason = STOP_QMAX
            elif rho == 0:
                reason = STOP_RHO_ZERO
            if reason < 0:
                nbad = nbad + 1 if (ini - cur) * f(1e3) < ini else 0
                if nbad >= 3:
                    reason = STOP_SMALL_GAIN
            it += 1
            if reason < 0 and it < max_iter:
                ini, qmax, nxt = cur, 0, LM_NEXT
            elif reason < 0:
                reason = STOP_ITERATIONS
    return np.array([lam, ni, cur, ini, it, qmax, nbad, 1.0 if accepted else 0.0, nxt, reason], float), float(rho)


@functools.lru_cache(None)
def lm_step_cases():
    """(name, item, expected) per branch and per side of every comparison of the rule.  expected: accepted, next, reason and,
    where the clamp or the rejection decides it, the factor lambda takes (None: between the clamp edges, held to LM_POW_BOUND)."""
    cases = []

    def add(name, rho=None, temp=None, ok=1, scale_sum=0.5, lam=1e-3, ni=2.0, cur=1000.0, ini=None, it=0, qmax=0, nbad=0, max_iter=10,
            accepted=None, nxt=None, reason=-1, factor=None):
        if temp is None:
            temp = cur - rho * (scale_sum + 1e-3)
        ini = cur if ini is None else ini
        cases.append((name, np.array([lam, ni, cur, ini, it, qmax, nbad, temp, ok, scale_sum, max_iter], float),
                      dict(accepted=accepted, next=nxt, reason=reason, factor=factor)))

    big = dict(cur=1000.0, ini=1000.0)      # a trial that gains far more than 1e-3 of iniChi needs a scale to match
    for rho in (-2.0, 0.1, 0.5, 0.8, LM_CLAMP_EDGES[0] - 2e-3):
        if rho > 0:
            add("accepted, factor clamped to 2/3, rho %.4f" % rho, rho, scale_sum=500.0, accepted=1, nxt=LM_NEXT, factor=2 / 3, **big)
    for rho in (LM_CLAMP_EDGES[1] + 2e-3, 0.95, 1.0, 5.0):
        add("accepted, factor clamped to 1/3, rho %.4f" % rho, rho, scale_sum=100.0, accepted=1, nxt=LM_NEXT, factor=1 / 3, **big)
    for rho in (0.85, 0.87, 0.9, 0.93):
        add("accepted, between the clamp edges, rho %.2f" % rho, rho, scale_sum=300.0, accepted=1, nxt=LM_NEXT, **big)
    add("accepted resets ni", 0.5, scale_sum=500.0, ni=16.0, accepted=1, nxt=LM_NEXT, factor=2 / 3)
    # rho's sign: one ulp of the chi2 on either side, and zero
    add("rho just above zero", temp=float(np.nextafter(1000.0, 0)), accepted=1, nxt=LM_NEXT, factor=2 / 3)
    add("rho == 0", temp=1000.0, accepted=0, nxt=LM_STOP, reason=STOP_RHO_ZERO, factor=2.0)
    add("rho just below zero", temp=float(np.nextafter(1000.0, np.inf)), accepted=0, nxt=LM_RETRY, factor=2.0)
    add("rejected, ni 2 -> 4", -2.0, accepted=0, nxt=LM_RETRY, factor=2.0)
    add("rejected, ni 8 -> 16", -2.0, ni=8.0, qmax=3, accepted=0, nxt=LM_RETRY, factor=8.0)
    add("rejected, qmax 8 -> 9: retry", -2.0, qmax=8, accepted=0, nxt=LM_RETRY, factor=2.0)
    add("rejected, qmax 9 -> 10: stop", -2.0, qmax=9, accepted=0, nxt=LM_STOP, reason=STOP_QMAX, factor=2.0)
    add("accepted at qmax 9 -> 10: stop all the same", 0.5, scale_sum=500.0, qmax=9, accepted=1, nxt=LM_STOP, reason=STOP_QMAX, factor=2 / 3)
    add("rho == 0 at qmax 9 -> 10: QMAX comes first", temp=1000.0, qmax=9, accepted=0, nxt=LM_STOP, reason=STOP_QMAX, factor=2.0)
    # a failed solve: tempChi is DBL_MAX whatever the pass summed
    add("solve failed", temp=3.0, ok=0, accepted=0, nxt=LM_RETRY, factor=2.0)
    add("solve failed at qmax 9", temp=3.0, ok=0, qmax=9, accepted=0, nxt=LM_STOP, reason=STOP_QMAX, factor=2.0)
    add("solve failed under a negative scale: DBL_MAX is finite and rho positive", temp=3.0, ok=0, scale_sum=-1.0, accepted=1, nxt=LM_NEXT,
        factor=1 / 3)
    # a chi2 that is not finite is never accepted
    add("tempChi +inf: rho -inf", temp=np.inf, accepted=0, nxt=LM_RETRY, factor=2.0)
    add("tempChi +inf under a negative scale: rho +inf", temp=np.inf, scale_sum=-1.0, accepted=0, nxt=LM_NEXT, factor=2.0)
    add("tempChi -inf: rho +inf", temp=-np.inf, accepted=0, nxt=LM_NEXT, factor=2.0)
    add("tempChi NaN: no comparison holds", temp=np.nan, accepted=0, nxt=LM_NEXT, factor=2.0)
    add("tempChi NaN at qmax 9", temp=np.nan, qmax=9, accepted=0, nxt=LM_STOP, reason=STOP_QMAX, factor=2.0)
    # Raul's criterion: (iniChi - curChi) * 1e3 < iniChi, three times in a row
    small = dict(rho=0.5, scale_sum=1.0 - 1e-3, accepted=1, factor=2 / 3)      # gains 0.5 of 1000
    add("small gain, nbadR 0 -> 1", nbad=0, nxt=LM_NEXT, **small)
    add("small gain, nbadR 1 -> 2", nbad=1, nxt=LM_NEXT, **small)
    add("small gain, nbadR 2 -> 3: stop", nbad=2, nxt=LM_STOP, reason=STOP_SMALL_GAIN, **small)
    add("gain of exactly 1e-3 iniChi resets nbadR", temp=999.0, scale_sum=2.0 - 1e-3, nbad=2, accepted=1, nxt=LM_NEXT, factor=2 / 3)
    add("gain just under 1e-3 iniChi counts", temp=float(np.nextafter(999.0, np.inf)), scale_sum=2.0 - 1e-3, nbad=1, accepted=1, nxt=LM_NEXT,
        factor=2 / 3)
    add("large gain resets nbadR", 0.5, scale_sum=500.0, nbad=2, accepted=1, nxt=LM_NEXT, factor=2 / 3)
    add("rejected with rho NaN and a small gain counts too", temp=np.nan, nbad=2, accepted=0, nxt=LM_STOP, reason=STOP_SMALL_GAIN, factor=2.0)
    # optimize()'s loop
    add("iter reaches maxIter - 1", 0.5, scale_sum=500.0, it=3, max_iter=5, accepted=1, nxt=LM_NEXT, factor=2 / 3)
    add("iter reaches maxIter", 0.5, scale_sum=500.0, it=4, max_iter=5, accepted=1, nxt=LM_STOP, reason=STOP_ITERATIONS, factor=2 / 3)
    add("maxIter 1", 0.5, scale_sum=500.0, it=0, max_iter=1, accepted=1, nxt=LM_STOP, reason=STOP_ITERATIONS, factor=2 / 3)
    add("small gain at the last iteration: SMALL_GAIN comes first", it=9, nbad=2, nxt=LM_STOP, reason=STOP_SMALL_GAIN, **small)
    add("a retry leaves iter alone at the cap", -2.0, it=9, accepted=0, nxt=LM_RETRY, factor=2.0)
    return tuple(cases)


def lm_step_items():
    return np.stack([c[1] for c in lm_step_cases()])


def lm_step_check(out, what=""):
    """The reference and (where stated) the expectation of every case against `out` [n][10]: everything exact except lambda between
    the clamp edges, which is held to LM_POW_BOUND (relative)."""
    for (name, item, exp), o in zip(lm_step_cases(), out):
        ref, rho = lm_step_reference(item)
        assert same_bits(o[1:], ref[1:]), (what, name, o.tolist(), ref.tolist())
        assert (o[7], o[8], o[9]) == (exp["accepted"], exp["next"], exp["reason"]), (what, name, o.tolist())
        if exp["factor"] is not None:
            assert o[0].tobytes() == ref[0].tobytes() == np.float64(item[0] * exp["factor"]).tobytes(), (what, name, o[0], ref[0])
            assert min(abs(rho - e) for e in LM_CLAMP_EDGES) >= 1e-3 or not exp["accepted"], (name, rho)
        else:
            assert LM_CLAMP_EDGES[0] + 1e-3 < rho < LM_CLAMP_EDGES[1] - 1e-3 and 1 / 3 < ref[0] / item[0] < 2 / 3, (name, rho)
            assert abs(o[0] - ref[0]) <= LM_POW_BOUND * abs(ref[0]), (what, name, o[0], ref[0])
