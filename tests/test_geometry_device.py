"""The camera models and the SE3 / Sim3 maps of the solvers (csrc/orbx_kb8.h, orbx_kb8_edge.h, orbx_pose.h, and the functions
orbx_sim3opt.h and orbx_mlpnp.h hold), every function alone through orbx_debug_geometry (csrc/orbx_api_geom.hip), against the
references of tests/geom_cases.py.

The exact operations (+ - * / and sqrt only) must equal a numpy restatement in the header's order bit for bit, NaNs by position.
The operations that call libm are held to an mpmath evaluation of the header's expression tree with a first-order error bound
carried through every operation: half an ulp per arithmetic operation, the OpenCL full-profile budget per libm call.

On the CPU: the ABI, the argument checks, the headers' domain sentences, every reference held against the numpy restatement (to a
quarter of the bound, or to the bound the restatement's own arithmetic and the host's libm leave, whichever is larger), the
mutants, the branch margins, the cap on cases that need Newton's alternative break, the share of items that pass only through the
restatement's own bound and the list of outputs that have no bound.  On the device every test prints the largest
measured / bound per output.  HISTORY.md has the measured fractions."""
import os
import re
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import geom_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_fast_amd", "csrc")
NO_DEVICE = ((orbx.E_NODEVICE, "no HIP device available"), (orbx.E_BADARG, "device index out of range"))
OPS = ("CAM_PROJECT", "CAM_UNPROJECT", "CAM_UNPROJECT_ROUNDED_TAN", "KB8_PROJECT_D", "KB8_PROJECT_JAC", "SE3_MAP", "SE3_COMPOSE", "QMUL",
       "QROT", "NORMALIZE_ROTATION", "QUAT_FROM_R", "OPLUS", "SIM3_EXP", "SIM3_OPLUS", "SO_INVERSE", "RODRIGUES2ROT", "ROT2RODRIGUES")


def hold(family, got, limit=1.0, own=False):
    """Prints the largest measured / bound per output and asserts it against limit."""
    fr, must, unbounded = gc.measure(family, got, own)
    for k in range(fr.shape[1]):
        print("%s out[%d]: fraction of the bound %.3g" % (family, k, fr[:, k].max()))
    names = gc.cases(family)[0]
    bad = sorted({names[i] for i in np.nonzero(~(fr.max(1) <= limit))[0]})
    assert not bad, (family, bad, float(fr.max()))
    return fr


# ------------------------------------------------------------------------------------------------ the ABI on the CPU
def test_symbol_exported_constants_mirrored_and_header_compiles_as_c99(tmp_path):
    assert hasattr(orbx.lib(), "orbx_debug_geometry")
    h = open(os.path.join(ROOT, "include", "orbx.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define ORBX_GEOM_(\w+) (\d+)", h)}
    assert len(defs) == 19 and defs.pop("OPS") == orbx.GEOM_OPS == 17 and defs.pop("MAX_ITEMS") == orbx.GEOM_MAX_ITEMS
    assert sorted(defs.values()) == list(range(17)) and all(getattr(orbx, "GEOM_" + k) == v for k, v in defs.items())
    assert [defs[k] for k in OPS] == list(range(17))
    src = tmp_path / "abi.c"
    src.write_text('#include "orbx.h"\nint (*entry)(int, int, int, const void*, void*) = orbx_debug_geometry;\n'
                   "typedef char a0[ORBX_GEOM_ROT2RODRIGUES + 1 == ORBX_GEOM_OPS ? 1 : -1];\nint main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "abi.o")])
    # the item sizes of the Python mirror are the kernels'
    hip = open(os.path.join(CSRC, "orbx_api_geom.hip")).read()
    for name, col in (("kInElems", 1), ("kOutElems", 2)):
        expr = re.search(name + r"\[ORBX_GEOM_OPS\] = \{([^}]*)\}", hip).group(1)
        assert [int(e) for e in expr.split(",")] == [orbx.GEOM_ITEM[op][col] for op in range(orbx.GEOM_OPS)], name
    assert "op < ORBX_GEOM_KB8_PROJECT_D ? sizeof(float) : sizeof(double)" in hip
    assert [np.dtype(orbx.GEOM_ITEM[op][0]).itemsize for op in range(17)] == [4] * 3 + [8] * 14
    k = orbx.geom_kb8_items(gc.TUM_VI, [[1.0, 2.0, 3.0]])
    assert k.shape == (1, 7) and k[0, :4].view(np.float32).tobytes() == gc.TUM_VI.tobytes() and k[0, 4:].tolist() == [1.0, 2.0, 3.0]


def test_debug_kernels_call_the_headers_and_restate_nothing():
    hip = open(os.path.join(CSRC, "orbx_api_geom.hip")).read()
    for inc in ("orbx_kb8.h", "orbx_kb8_edge.h", "orbx_sim3opt.h", "orbx_mlpnp.h"):
        assert '#include "%s"' % inc in hip
    for call in ("orbx::cam_project(", "orbx::cam_unproject<false>(", "orbx::cam_unproject<true>(", "kb8_project(k, X, o[0], o[1])",
                 "kb8_project_jac(", "se3_map(", "se3_compose(", "qmul(", "qrot(", "normalize_rotation(", "quat_from_R(", "oplus(",
                 "sim3_exp(", "sim3_oplus(", "so_inverse(", "orbx::rodrigues2rot(", "orbx::rot2rodrigues("):
        assert call in hip, call
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ("sin", "cos", "atan2", "sqrt", "exp", "acos", "tan", "sinf", "cosf", "atan2f", "sqrtf", "tanf", "sincos", "fma"):
        assert not re.search(r"(?<![A-Za-z0-9_])%s\s*\(" % word, code), word
    assert "orbx_api_geom.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # the functions that moved are defined once, in the headers
    for fn, hdr, old in (("sim3_exp", "orbx_sim3opt.h", "orbx_sim3opt.hip"), ("sim3_oplus", "orbx_sim3opt.h", "orbx_sim3opt.hip"),
                         ("so_inverse", "orbx_sim3opt.h", "orbx_sim3opt.hip"), ("rodrigues2rot", "orbx_mlpnp.h", "orbx_mlpnp.hip"),
                         ("rot2rodrigues", "orbx_mlpnp.h", "orbx_mlpnp.hip")):
        define = "__device__ __forceinline__ void %s(" % fn
        assert define in open(os.path.join(CSRC, hdr)).read() and define not in open(os.path.join(CSRC, old)).read(), fn


def test_bad_arguments_are_rejected_before_any_device_is_touched():
    L = orbx.lib()
    a, out = np.ones(192), np.full(192, 7.0)

    def call(op, n, null=None, device=1 << 20):       # a device that does not exist: never reached by a rejected call
        rc = L.orbx_debug_geometry(device, op, n, None if null == "in" else orbx._p(a), None if null == "out" else orbx._p(out))
        return rc, L.orbx_last_error().decode()
    for op in range(orbx.GEOM_OPS):
        assert call(op, 1, "in") == (orbx.E_BADARG, "null argument") and call(op, 1, "out") == (orbx.E_BADARG, "null argument")
        for n in (0, -1, -2 ** 31, orbx.GEOM_MAX_ITEMS + 1, 2 ** 31 - 1):
            assert call(op, n) == (orbx.E_BADARG, "n outside [1, ORBX_GEOM_MAX_ITEMS]"), (op, n)
        assert call(op, 1) in NO_DEVICE, op
    for op in (-1, orbx.GEOM_OPS, 1 << 20, -2 ** 31):
        assert call(op, 1) == (orbx.E_BADARG, "unknown operation"), op
    assert call(-1, 0, "in") == (orbx.E_BADARG, "null argument") and call(-1, 0) == (orbx.E_BADARG, "n outside [1, ORBX_GEOM_MAX_ITEMS]")
    assert call(0, 1, device=-1) in NO_DEVICE
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ the headers' domains
JAC_DOMAIN = ("Domain: r = sqrt(x^2 + y^2) > 0 with r^3 a normal double (r above about 3e-103).  On the axis (r = 0) the first two columns "
              "are NaN (0 / 0) and the third is a signed zero; once r^3 underflows to zero (r below about 1e-108) the first two columns are "
              "inf or NaN; and as r / z -> 0 the two terms of every entry cancel, so digits are lost long before that: the off-diagonal "
              "entries keep 10 digits at r / z = 5e-4 and none at 5e-9.  This is the reference's own arithmetic (KannalaBrandt8.cpp:149-184)")
UNPROJECT_DOMAIN = ("theta_d is clamped to pi / 2, so every pixel beyond the clamp returns the scale of the clamp; where Newton ends past "
                    "pi / 2 the tangent is negative and the ray points backwards (TUM-VI: scale -49.8 at theta_d = 1.566, -34.98 for every "
                    "pixel beyond the clamp).  The break reads |theta_fix| < precision in float: a precision below float resolution (1e-9) "
                    "ends the loop only on a theta_fix of exactly 0 or after the 10 steps, and arithmetic that rounds a quotient or a root "
                    "differently may break one step earlier or later.  All of it is KannalaBrandt8::unproject's (KannalaBrandt8.cpp:116-147)")
NORMALIZE_DOMAIN = ("Domain: a quaternion whose norm is finite and not zero, and whose squared norm neither overflows nor underflows.  The "
                    "zero quaternion gives four NaNs (0 / 0)")
ROT2_DOMAIN = ("Where rounding leaves trace / 2 outside [-1, 1] (an ulp above 1 near the identity, an ulp below -1 near pi) acos is NaN, the "
               "comparison reads false and the zero vector comes back; towards pi the result is divided by sin(wnorm) -> 0 and loses "
               "digits, the error growing like 1 / (pi - angle)^2.  MLPnPsolver.cpp:684-698")
SIM3_DOMAIN = ("Just above |sigma| = 1e-5 with theta < 1e-5, A = ((sigma - 1) s + 1) / sigma^2 comes from terms of size 1 for a numerator "
               "of size 5e-11: one ulp of exp moves A = 1 / 2 by 2e-6.  sim3.h:114-116")


def test_headers_state_the_domains_the_tests_hold():
    """Each sentence is asserted on the device by the test named beside it."""
    for hdr, sentence in (("orbx_kb8_edge.h", JAC_DOMAIN),          # test_kb8_project_jac
                          ("orbx_kb8.h", UNPROJECT_DOMAIN),         # test_cam_unproject
                          ("orbx_pose.h", NORMALIZE_DOMAIN),        # test_exact_operations[NORMALIZE_ROTATION]
                          ("orbx_mlpnp.h", ROT2_DOMAIN),            # test_rodrigues_pair
                          ("orbx_sim3opt.h", SIM3_DOMAIN)):         # test_sim3_exp_and_oplus
        text = " ".join(re.sub(r"^\s*//", "", line) for line in open(os.path.join(CSRC, hdr)).read().splitlines())
        assert re.sub(r"\s+", " ", sentence) in re.sub(r"\s+", " ", text), (hdr, sentence)
        assert "se3quat.h:280-285" in text or hdr != "orbx_pose.h"


def test_domain_sentences_are_what_the_references_say():
    """The figures of the sentences, from the references alone."""
    names, items = gc.cases("KB8_PROJECT_JAC")
    ref = gc.reference("KB8_PROJECT_JAC")
    tum = np.nonzero(names == "TUM-VI, r/z decades")[0][:161]            # z = 1: decade d is item d
    with np.errstate(all="ignore"):
        rel = ref.e[0][tum, 1] / np.abs(ref.hi[0][tum, 1])
        host = np.abs((gc.restate("KB8_PROJECT_JAC", items[tum])[:, 1] - ref.hi[0][tum, 1]) - ref.lo[0][tum, 1]) / np.abs(ref.hi[0][tum, 1])
    print("PJ[0][1] by decade of r / z, bound relative to the value:", ["%.1e" % x for x in rel[:12]])
    print("PJ[0][1] by decade of r / z, the float64 restatement's relative error:", ["%.1e" % x for x in host[:12]])
    # the error grows like eps / (r / z)^2: float64 arithmetic keeps 10 digits at 5e-4 (between the decades 1e-3 and 1e-4) and the
    # bound guarantees none from 1e-8 on
    assert host[3] < 1e-9 and host[4] < 1e-7 and (rel[8:100] > 0.5).all() and 50 < rel[5] / rel[4] < 200
    assert np.isfinite(ref.hi[0][tum[:108], :2]).all() and np.isnan(ref.hi[0][tum[109:], :2]).all()    # r^3 underflows below 1e-108
    axis = np.nonzero(names == "TUM-VI, on the axis")[0]
    assert np.isnan(ref.hi[0][axis][:, [0, 1, 3, 4]]).all() and (ref.hi[0][axis][:, [2, 5]] == 0).all() and (ref.e[0][axis][:, [2, 5]] < 1e-300).all()
    # the unprojection: the scale past the polynomial's range and at the clamp (the restatement's float arithmetic)
    names, items = gc.cases("CAM_UNPROJECT")
    out = gc.restate("CAM_UNPROJECT", items)
    with np.errstate(all="ignore"):
        pw = (items[:, 10:12] - items[:, 3:5]) / items[:, 1:3]
        td, scale = np.hypot(pw[:, 0], pw[:, 1]), out[:, 0] / pw[:, 0]
    sel = np.array([n.startswith("TUM-VI") and n.endswith("radial") for n in names])
    assert np.allclose(scale[sel & (np.abs(td - 1.566) < 1e-5)], -49.8, rtol=2e-3)
    past = sel & (td > 1.5708)
    assert past.sum() >= 24 and np.allclose(scale[past], -34.98, rtol=2e-4) and len(set(scale[past].tolist())) <= 3
    # sim3_exp: A just above |sigma| = 1e-5: the bound of t is 2e-6 and more of |A W u|
    names, items = gc.cases("SIM3_EXP")
    ref = gc.reference("SIM3_EXP")
    k = [i for i, n in enumerate(names) if n == "theta 0.0, sigma %r" % gc.SIGMAS[2]][0]
    assert items[k, 6] > 1e-5 and not items[k, :3].any()
    sigma = gc.E.of(gc.SIGMAS[2], gc.F64)
    s = gc.exp(sigma)
    A = ((sigma - 1) * s + 1) / (sigma * sigma)
    print("sim3_exp just above 1e-5: A = %.9f, bound %.3g relative (exp's 3 ulp and the two roundings)" % (float(A.v), float(A.e / A.v)))
    assert abs(float(A.v) - 0.5) < 1e-5 and 3 * 2e-6 < float(A.e) < 6 * 2e-6      # exp's 3 ulp at 2e-6 each, and the roundings


# ------------------------------------------------------------------------------------------------ the references on the CPU
@pytest.mark.parametrize("family", gc.EXACT)
def test_exact_restatements_against_the_mpmath_tree(family):
    """An mpmath evaluation rounded once (60 digits, above longdouble's 19): the float restatement lies within the tracked bound of
    it, and where the tree is not finite the restatement is not either."""
    names, items = gc.cases(family)
    fr = hold(family, gc.restate(family, items), 1.0)
    assert len(items) >= 50 and fr.max() > 0          # some output is rounded somewhere


@pytest.mark.parametrize("family", gc.LIBM + ("ROUND_TRIP",))
def test_libm_restatements_within_a_quarter_of_the_bound_or_their_own(family):
    """Case by case the larger of the two holds: a quarter of the tracked bound, so that the inputs cannot hide a device failure;
    the bound the same tracker gives the restatement itself (exact inputs, half an ulp per operation, the host's libm at 1 ulp)."""
    names, items = gc.cases(family)
    out = gc.restate(family, items)
    quarter = gc.measure(family, out)[0] * 4
    own = gc.measure(family, out, own=True)[0]
    worst = np.minimum(quarter, own)
    print("%s: %d items; restatement at most %.3g of a quarter of the bound or %.3g of its own" % (family, len(items), quarter.max(), own.max()))
    bad = sorted({names[i] for i in np.nonzero(~(worst.max(1) <= 1.0))[0]})
    assert not bad, (family, bad)
    assert 1 <= len(items) <= 4000
    # The second term equals the device's bound wherever a rounding that the restatement shares with the device dominates (the float
    # narrowing of theta and psi in KB8_PROJECT_D, an output's own half ulp): an item that passes only through it does not show
    # that the inputs leave the device three quarters of the bound.  Their share is printed and held below a third per family.
    relies = (quarter.max(1) > 1.0).mean()
    print("%s: %.1f %% of the items pass only through the restatement's own bound" % (family, 100 * relies))
    assert relies <= 1.0 / 3.0, (family, relies)


# family -> the case names in which some output's tracked bound is infinite (nothing is claimed of it) and how many items they are
UNBOUNDED = {"SE3_COMPOSE": ({"scaled by 2^-400"}, 10),      # bit-compared anyway: the squared norm of the product is denormal or zero
             "ROT2RODRIGUES": ({"angles"}, 2)}                # the rotations by exactly pi whose sin(wnorm) is of the size of its own error


@pytest.mark.parametrize("family", gc.FAMILIES + ("ROUND_TRIP",))
def test_outputs_without_a_bound_are_the_listed_ones(family):
    """measure() counts an output whose bound is infinite as met; no family may become vacuous that way unnoticed."""
    names, items = gc.cases(family)
    unbounded = gc.measure(family, gc.restate(family, items))[2].any(1)
    want_names, want_items = UNBOUNDED.get(family, (set(), 0))
    print("%s: %d of %d items have an output without a bound" % (family, unbounded.sum(), len(items)))
    assert set(names[unbounded].tolist()) == want_names and unbounded.sum() == want_items, (family, sorted(set(names[unbounded].tolist())))


def test_kb8_project_jac_restatement_in_ulps_at_ordinary_points():
    names, items = gc.cases("KB8_PROJECT_JAC")
    ref = gc.reference("KB8_PROJECT_JAC")
    out = gc.restate("KB8_PROJECT_JAC", items)
    """Plain float64 evaluation is 0.05 to 6 ulp off at r / z of 1 and more.  The random points here go down to r / z = 0.26,
    where the cancellation (eps / (r / z)^2) already costs up to 29 ulp: the figure held is the error times min(1, r / z)^2."""
    sel = np.array([n.endswith("random") for n in names])
    X = items[sel, 4:]
    rz = np.hypot(X[:, 0], X[:, 1]) / np.abs(X[:, 2])
    ulp = (np.abs((out[sel] - ref.hi[0][sel]) - ref.lo[0][sel]) / np.abs(ref.hi[0][sel])).max(1) / gc.EPS64
    print("kb8_project_jac restated in float64, r / z from %.3g to %.3g: at most %.2f ulp at r / z >= 1, %.2f ulp below, %.2f ulp x min(1, r / z)^2"
          % (rz.min(), rz.max(), ulp[rz >= 1].max(), ulp[rz < 1].max(), (ulp * np.minimum(rz, 1) ** 2).max()))
    assert (rz >= 1).sum() >= 50 and (rz < 1).sum() >= 50 and (ulp * np.minimum(rz, 1) ** 2).max() <= 6.0


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_mutants_are_caught(family):
    """Every deliberately wrong restatement leaves the bound (breaks the bits, for the exact operations) on the family's inputs."""
    names, items = gc.cases(family)
    assert len(gc.MUTANTS[family]) >= 3
    good = gc.restate(family, items)
    for m in gc.MUTANTS[family]:
        out = gc.restate(family, items, m)
        if family in gc.EXACT:
            assert not gc.same_bits(out, good), (family, m)
        else:
            fr = gc.measure(family, out)[0]
            print("%s, %s: %.3g of the bound on %d items" % (family, m, fr.max(), (fr.max(1) > 1).sum()))
            assert fr.max() > 1.0, (family, m)


def test_branches_are_decided_by_more_than_the_tracked_error_and_newton_cap():
    seen = {}
    for family in gc.FAMILIES + ("ROUND_TRIP",):
        ref = gc.reference(family)
        for label, margin, exact in ref.decisions:
            assert margin > 0 or exact, (family, label, float(margin))
            seen.setdefault((family, label), 0)
            seen[(family, label)] += 1
    for key in (("OPLUS", "theta < 1e-5"), ("SIM3_EXP", "theta < 1e-5"), ("SIM3_EXP", "|sigma| < 1e-5"), ("SIM3_OPLUS", "|sigma| < 1e-5"),
                ("RODRIGUES2ROT", "n > eps"), ("ROT2RODRIGUES", "wnorm > eps"), ("CAM_UNPROJECT", "theta_d > 1e-8"), ("CAM_UNPROJECT", "clamp"),
                ("QUAT_FROM_R", "trace > 0"), ("QUAT_FROM_R", "R11 > R00"), ("QUAT_FROM_R", "R22 > max"), ("NORMALIZE_ROTATION", "q[3] < 0"),
                ("OPLUS", "q[3] < 0"), ("OPLUS", "trace > 0")):
        assert seen.get(key, 0) >= 2, key
    # both sides of every branch, from the restatement (which the references follow)
    def sides(family, pred):
        names, items = gc.cases(family)
        with np.errstate(all="ignore"):
            v = np.array([pred(x) for x in items])
        return v.any() and (~v).any()
    norm3 = lambda x: np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    assert sides("OPLUS", lambda x: norm3(x) < 1e-5) and sides("RODRIGUES2ROT", lambda x: norm3(x) > gc.K_EPS)
    names, items = gc.cases("SIM3_EXP")
    combos = {(bool(abs(x[6]) < 1e-5), bool(norm3(x) < 1e-5)) for x in items}
    assert len(combos) == 4
    for th in gc.THETAS[1:3]:       # the two neighbours: the norm as computed is the double next to 1e-5 on its side
        for ax in gc.AXES:
            n = norm3(gc._omega(th, ax))
            assert n == (np.nextafter(1e-5, 0) if th < 1e-5 else 1e-5), (th, ax, n)
    names, items = gc.cases("SIM3_OPLUS")
    assert {x[7] for x in items} == {0.0, 1.0}
    out = gc.restate("ROT2RODRIGUES", gc.cases("ROT2RODRIGUES")[1])
    names = gc.cases("ROT2RODRIGUES")[0]
    assert not out[names == "trace / 2 one ulp above 1"].any() and not out[names == "trace / 2 one ulp below -1"].any() and not out[names == "identity"].any()
    assert sides("CAM_UNPROJECT", lambda x: np.float64(np.hypot((x[10] - x[3]) / x[1], (x[11] - x[4]) / x[2])) > 1e-8)
    for family in ("CAM_UNPROJECT", "CAM_UNPROJECT_ROUNDED_TAN"):
        ref = gc.reference(family)
        share = ref.ambiguous.mean()
        print("%s: %d of %d cases need Newton's alternative break (%.2f %%): the loop's operations are all correctly rounded and "
              "the float32 iteration decides" % (family, ref.ambiguous.sum(), len(ref.ambiguous), 100 * share))
        assert share <= 0.02
    assert np.array_equal(gc.cases("CAM_UNPROJECT")[1], gc.cases("CAM_UNPROJECT_ROUNDED_TAN")[1])
    assert {float(x) for x in gc.cases("CAM_UNPROJECT")[1][:, 9]} == {float(np.float32(p)) for p in (1e-6, 1e-9, 1e-3)}


def test_newton_iterations_by_precision():
    """A precision below float resolution ends the loop one step later, on a theta_fix of exactly 0, with the same scale."""
    names, items = gc.cases("CAM_UNPROJECT")
    out = gc.restate("CAM_UNPROJECT", items)
    sel6 = np.array(["TUM-VI, precision 1e-06, random" == n for n in names])
    sel9 = np.array(["TUM-VI, precision 1e-09, random" == n for n in names])
    assert sel6.sum() == sel9.sum() >= 50
    same = (out[sel6] == out[sel9]).all(1).mean()
    print("precision 1e-9 against 1e-6: the same ray bit for bit on %.1f %% of the random pixels" % (100 * same))
    assert same > 0.9


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


_memo = {}


def device(family):
    """A family's cases in one launch, made once per module; two calls are bit-identical."""
    if family not in _memo:
        items = gc.cases(family)[1]
        out = orbx.debug_geometry(gc.geom_op(family), items, 7.0)
        assert gc.same_bits(out, orbx.debug_geometry(gc.geom_op(family), items, 7.0)), family
        _memo[family] = out
    return _memo[family]


@pytest.mark.gpu
@pytest.mark.parametrize("family", gc.EXACT)
def test_exact_operations(gpu, family):
    """+ - * / and sqrt only, no contraction: the numpy restatement's bits, NaNs by position.  NORMALIZE_ROTATION: the zero
    quaternion gives four NaNs (the header)."""
    names, items = gc.cases(family)
    out, want = device(family), gc.restate(family, items)
    diff = [names[i] for i in range(len(items)) if not gc.same_bits(out[i], want[i])]
    print("%s: %d items, %d differ from the restatement's bits" % (family, len(items), len(diff)))
    assert not diff, (family, sorted(set(diff)))
    if family == "NORMALIZE_ROTATION":
        assert np.isnan(out[names == "zero"]).all() and (names == "zero").sum() == 2
        assert (out[names == "w = -0"][:, 3] == 0).all() and not np.signbit(out[names == "w = -0"][0, 0])     # -0 is not below zero: no flip


def bounded(family):
    names, items = gc.cases(family)
    out = device(family)
    hold(family, out)
    return names, items, out


@pytest.mark.gpu
def test_cam_project(gpu):
    """|X| scaled by 2^100: x^2 + y^2 overflows to inf in float and theta is pi / 2 whatever z is, so every point lands on the
    circle of that angle; scaled by 2^-100 it underflows to 0 and the point lands on the principal point exactly."""
    names, items, out = bounded("CAM_PROJECT")
    for cname, cam in (("TUM-VI", gc.TUM_VI), ("large k", gc.LARGE_K)):
        big, tiny = out[names == cname + ", scaled by 2^100"], out[names == cname + ", scaled by 2^-100"]
        assert len(big) == len(tiny) == 12 and (tiny == cam[2:4]).all(), cname
        t = np.float64(gc.HALF_PI_F)
        r = t * (1 + cam[4] * t ** 2 + cam[5] * t ** 4 + cam[6] * t ** 6 + cam[7] * t ** 8)
        radius = np.hypot((big[:, 0] - cam[2]) / cam[0], (big[:, 1] - cam[3]) / cam[1])
        print("%s, scaled by 2^100: radius / r(pi / 2) from %.7f to %.7f" % (cname, (radius / r).min(), (radius / r).max()))
        assert np.abs(radius / r - 1).max() < 1e-5, cname


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["CAM_UNPROJECT", "CAM_UNPROJECT_ROUNDED_TAN"])
def test_cam_unproject(gpu, family):
    """The header: beyond the clamp every pixel returns the clamp's scale, past pi / 2 the scale is negative."""
    names, items, out = bounded(family)
    with np.errstate(all="ignore"):
        pw = (items[:, 10:12] - items[:, 3:5]) / items[:, 1:3]
        td, scale = np.hypot(pw[:, 0], pw[:, 1]), out[:, 0] / pw[:, 0]
    sel = np.array([n.startswith("TUM-VI") and n.endswith("radial") for n in names])
    past = sel & (td > 1.5708)
    print("%s: scale at theta_d = 1.566: %s; beyond the clamp: %s" % (family, sorted(set(scale[sel & (np.abs(td - 1.566) < 1e-5)].tolist())),
                                                                      sorted(set(scale[past].tolist()))))
    assert (scale[sel & (np.abs(td - 1.566) < 1e-5)] < -40).all() and np.allclose(scale[past], -34.98, rtol=1e-3)
    pp = np.array([n.endswith("principal point") for n in names])
    assert (out[pp][0::5] == [0.0, 0.0, 1.0]).all() and (out[:, 2] == 1.0).all()          # on the principal point: the ray of the axis


@pytest.mark.gpu
def test_kb8_project_d(gpu):
    bounded("KB8_PROJECT_D")


@pytest.mark.gpu
def test_kb8_project_jac(gpu):
    """The header: NaN on the axis, inf / NaN once r^3 underflows (measure() holds every entry the reference makes inf or NaN to
    be inf or NaN), digits lost as r / z -> 0 (the bound follows the terms, not the result)."""
    names, items, out = bounded("KB8_PROJECT_JAC")
    axis = np.array([n.endswith("on the axis") for n in names])
    assert np.isnan(out[axis][:, [0, 1, 3, 4]]).all() and (out[axis][:, [2, 5]] == 0).all()
    deep = np.nonzero(names == "TUM-VI, r/z decades")[0][110:161]
    assert not np.isfinite(out[deep][:, [0, 1, 3, 4]]).any() and np.isfinite(out[deep][:, [2, 5]]).all()


@pytest.mark.gpu
def test_oplus(gpu):
    bounded("OPLUS")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["SIM3_EXP", "SIM3_OPLUS"])
def test_sim3_exp_and_oplus(gpu, family):
    names, items, out = bounded(family)
    if family == "SIM3_OPLUS":          # a fixed scale: s comes back as the estimate's, whatever the update's sigma
        fixed = items[:, 7] == 1.0
        assert (out[fixed, 7] == items[fixed, 15]).all() and fixed.sum() >= 50


@pytest.mark.gpu
def test_rodrigues_pair(gpu):
    """The header: the zero vector where trace / 2 leaves [-1, 1]; and the round trip through both within the tracked bound."""
    bounded("RODRIGUES2ROT")
    names, items, out = bounded("ROT2RODRIGUES")
    for name in ("identity", "trace / 2 one ulp above 1", "trace / 2 one ulp below -1"):
        assert not out[names == name].any() and not np.signbit(out[names == name]).any(), name
    R = orbx.debug_geometry(orbx.GEOM_RODRIGUES2ROT, gc.ROUND_TRIP_W, 7.0)
    hold("ROUND_TRIP", orbx.debug_geometry(orbx.GEOM_ROT2RODRIGUES, R, 7.0))


@pytest.mark.gpu
def test_the_last_item_of_a_part_filled_wave_is_computed_and_nothing_past_it_is_written(gpu):
    """n = 1 and n = 65 for every operation: the kernels' bound check."""
    fam = {gc.geom_op(f): f for f in gc.FAMILIES if f not in gc.GEOM_OP}
    for op in range(orbx.GEOM_OPS):
        dt, n_in, n_out = orbx.GEOM_ITEM[op]
        items = gc.cases(fam[op])[1]
        items = np.concatenate([items] * (65 // len(items) + 1))[:66]
        full = orbx.debug_geometry(op, items[:65], 7.0)
        for n in (1, 65):
            out = np.full((66, n_out), 7.0, dt)
            assert orbx.lib().orbx_debug_geometry(0, op, n, orbx._p(np.ascontiguousarray(items)), orbx._p(out)) == 0
            assert (out[n:] == 7.0).all() and gc.same_bits(out[:n], full[:n]), (OPS[op], n)
