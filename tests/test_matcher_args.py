"""CPU pins of the matcher C ABI's argument checks: for every one-shot matcher entry a table of bad arguments (some with two
wrong at once, to pin which error is reported first) with the return code and orbx_last_error() text, plus the results of
the inputs that return before a device is touched.  The batched entries: the null-handle and bad-count checks only."""
import ctypes as C

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import E_BADARG, E_CAPACITY, E_NODEVICE, KP_DTYPE, MP_DTYPE, MPR_DTYPE, PP_DTYPE, FP_DTYPE, TRI_RIG_DTYPE

BAD = "bad argument"
LEVELS = 8


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows(n):
    # the host arrays: large counts are only passed to checks that reject them before any array is read
    return min(max(n, 1), 64)


def kps(n, octave=0):
    k = np.zeros(rows(n), KP_DTYPE)
    k["octave"] = octave
    return k


def desc(n):
    return np.zeros((rows(n), 32), np.uint8)


def u32(*v):
    return np.array(v if v else [0], np.uint32)


def i32(*v):
    return np.array(v if v else [0], np.int32)


def check(rc, code, msg):
    assert rc == code
    if code < 0 and code != E_NODEVICE:
        assert orbx.lib().orbx_last_error().decode() == msg


# ---- orbx_bf_knn2
def bf_knn2(nQ=4, nT=4, descQ=True, descT=True, idx2=True):
    lib = orbx.lib()
    return lib.orbx_bf_knn2(0, P(desc(nQ)) if descQ else None, nQ, P(desc(nT)) if descT else None, nT,
                            P(np.zeros(8, np.int32)) if idx2 else None, P(np.zeros(8, np.int32)), P(np.zeros(4, np.uint8)))


@pytest.mark.parametrize("kw", [dict(nQ=-1), dict(nT=-1), dict(descQ=False), dict(idx2=False), dict(descT=False),
                                dict(nQ=-1, descT=False)])
def test_bf_knn2_bad_arguments(kw):
    check(bf_knn2(**kw), E_BADARG, BAD)


def test_bf_knn2_no_queries_returns_before_the_device():
    assert bf_knn2(nQ=0, descQ=False, idx2=False) == 0
    assert bf_knn2(nQ=0, nT=0, descQ=False, descT=False, idx2=False) == 0


# ---- orbx_fisheye_stereo_match
def fisheye_stereo(nL=3, nR=3, monoL=0, monoR=0, rig=True, sigma=True, nlev=LEVELS, l2r=True, r2l=True, outs=None):
    lib = orbx.lib()
    o = outs or dict(l2r=np.full(max(nL, 1), 7, np.int32), r2l=np.full(max(nR, 1), 7, np.int32),
                     dep=np.full(max(nL, 1), 7, np.float32), p3=np.full(3 * max(nL, 1), 7, np.float32), nd=np.full(1, 7, np.int32))
    r = np.zeros(1, np.dtype([("v", "<f4", 29)]))
    return lib.orbx_fisheye_stereo_match(0, P(kps(nL)), P(desc(nL)), nL, monoL, P(kps(nR)), P(desc(nR)), nR, monoR,
                                         P(r) if rig else None, P(np.ones(LEVELS, np.float32)) if sigma else None, nlev,
                                         P(o["l2r"]) if l2r else None, P(o["r2l"]) if r2l else None, P(o["dep"]), P(o["p3"]),
                                         P(o["nd"]))


@pytest.mark.parametrize("kw", [dict(nL=-1), dict(nR=-1), dict(monoL=4), dict(monoR=-1), dict(rig=False), dict(sigma=False),
                                dict(nlev=0), dict(nlev=33), dict(l2r=False), dict(r2l=False), dict(monoL=5, rig=False)])
def test_fisheye_stereo_match_bad_arguments(kw):
    check(fisheye_stereo(**kw), E_BADARG, BAD)


@pytest.mark.parametrize("kw", [dict(monoL=3), dict(monoR=2), dict(nL=0, l2r=False)])
def test_fisheye_stereo_match_fills_the_outputs_before_the_device(kw):
    nL = kw.get("nL", 3)
    outs = dict(l2r=np.full(max(nL, 1), 7, np.int32), r2l=np.full(3, 7, np.int32), dep=np.full(max(nL, 1), 7, np.float32),
                p3=np.full(3 * max(nL, 1), 7, np.float32), nd=np.full(1, 7, np.int32))
    rc = fisheye_stereo(outs=outs, **kw)
    assert rc == (0 if orbx.device_count() > 0 else E_NODEVICE)
    assert (outs["l2r"][:nL] == -1).all() and (outs["dep"][:nL] == -1).all() and (outs["p3"][:3 * nL] == 0).all()
    assert (outs["r2l"] == -1).all() and outs["nd"][0] == 0


# ---- orbx_search_by_bow: two feature vectors (key frame, frame)
def search_by_bow(n_kf=4, n_f=4, kf=None, f=None, matches=True):
    """kf / f: (node_ids, node_start, feature_idx) of the key frame / the frame; default one node holding features 0..1."""
    lib = orbx.lib()
    kn, ks, ki = kf or (u32(1), i32(0, 2), u32(0, 1))
    fn, fs, fi = f or (u32(1), i32(0, 2), u32(0, 1))
    return lib.orbx_search_by_bow(0, P(kn), P(ks), P(ki), len(kn), P(kps(n_kf)), P(desc(n_kf)), P(np.ones(max(n_kf, 1), np.uint8)),
                                  n_kf, P(fn), P(fs), P(fi), len(fn), P(kps(n_f)), P(desc(n_f)), n_f, n_f, 0.6, 1,
                                  P(np.zeros(max(n_f, 1), np.int32)) if matches else None)


BOW_DESC = (u32(2, 1), i32(0, 1, 2), u32(0, 1))   # node ids descend
BOW_OFFS = (u32(1, 2), i32(0, 2, 1), u32(0, 1))   # offsets not monotone
BOW_IDX = (u32(1), i32(0, 2), u32(0, 9))          # feature index out of range
BOW_BIG = (u32(1), i32(0, 5), u32(0, 1, 2, 3, 0))  # more features than the frame


@pytest.mark.parametrize("kw,msg", [
    (dict(n_kf=-1), BAD), (dict(matches=False), BAD),
    (dict(kf=BOW_BIG), "feature vector larger than the frame"),
    (dict(f=BOW_BIG), "feature vector larger than the frame"),
    (dict(kf=BOW_DESC), "keyframe feature vector: node ids must ascend and offsets must be monotone"),
    (dict(kf=BOW_OFFS), "keyframe feature vector: node ids must ascend and offsets must be monotone"),
    (dict(f=BOW_DESC), "frame feature vector: node ids must ascend and offsets must be monotone"),
    (dict(kf=BOW_IDX), "keyframe feature index out of range"),
    (dict(f=BOW_IDX), "frame feature index out of range"),
    # two wrong at once: both sides' offsets are checked before either side's indices
    (dict(kf=BOW_IDX, f=BOW_OFFS), "frame feature vector: node ids must ascend and offsets must be monotone"),
    (dict(kf=BOW_DESC, f=BOW_DESC), "keyframe feature vector: node ids must ascend and offsets must be monotone"),
    (dict(kf=BOW_IDX, f=BOW_IDX), "keyframe feature index out of range"),
    (dict(kf=BOW_DESC, f=BOW_BIG), "feature vector larger than the frame"),
    (dict(n_f=-1, kf=BOW_DESC), BAD),
])
def test_search_by_bow_bad_arguments(kw, msg):
    check(search_by_bow(**kw), E_BADARG, msg)


# ---- orbx_search_by_bow_keyframes / orbx_search_for_triangulation(_rig): feature vectors 1 and 2
def two_vectors(fn, n1=4, n2=4, v1=None, v2=None, k1=None, k2=None, matches=True):
    a = v1 or (u32(1), i32(0, 2), u32(0, 1))
    b = v2 or (u32(1), i32(0, 2), u32(0, 1))
    k1 = kps(n1) if k1 is None else k1
    k2 = kps(n2) if k2 is None else k2
    m = P(np.zeros(max(n1, 1), np.int32)) if matches else None
    return fn(a, b, n1, n2, k1, k2, m)


def bow_keyframes(a, b, n1, n2, k1, k2, m):
    return orbx.lib().orbx_search_by_bow_keyframes(
        0, P(a[0]), P(a[1]), P(a[2]), len(a[0]), P(k1), P(desc(n1)), P(np.ones(max(n1, 1), np.uint8)), n1,
        P(b[0]), P(b[1]), P(b[2]), len(b[0]), P(k2), P(desc(n2)), P(np.ones(rows(n2), np.uint8)), n2, 0.75, 1, m)


def triangulation(a, b, n1, n2, k1, k2, m):
    ep, F12 = np.zeros(2, np.float32), np.eye(3, dtype=np.float32)
    return orbx.lib().orbx_search_for_triangulation(
        0, P(a[0]), P(a[1]), P(a[2]), len(a[0]), P(k1), P(desc(n1)), P(np.zeros(max(n1, 1), np.uint8)), None, n1,
        P(b[0]), P(b[1]), P(b[2]), len(b[0]), P(k2), P(desc(n2)), P(np.zeros(rows(n2), np.uint8)), None, n2,
        P(np.ones(LEVELS, np.float32)), P(np.ones(LEVELS, np.float32)), LEVELS, P(ep), P(F12), 0, 0, 1, m)


def triangulation_rig(a, b, n1, n2, k1, k2, m):
    rig = np.zeros(1, TRI_RIG_DTYPE)
    return orbx.lib().orbx_search_for_triangulation_rig(
        0, P(a[0]), P(a[1]), P(a[2]), len(a[0]), P(k1), P(desc(n1)), P(np.zeros(max(n1, 1), np.uint8)), n1, n1,
        P(b[0]), P(b[1]), P(b[2]), len(b[0]), P(k2), P(desc(n2)), P(np.zeros(rows(n2), np.uint8)), n2, n2,
        P(np.ones(LEVELS, np.float32)), P(np.ones(LEVELS, np.float32)), LEVELS, P(rig), 0, 0, 1, m)


VEC_CASES = [
    (dict(n1=-1), BAD), (dict(matches=False), BAD),
    (dict(v1=BOW_BIG), "feature vector larger than the key frame"),
    (dict(v2=BOW_BIG), "feature vector larger than the key frame"),
    (dict(v1=BOW_DESC), "feature vector 1: node ids must ascend and offsets must be monotone"),
    (dict(v2=BOW_OFFS), "feature vector 2: node ids must ascend and offsets must be monotone"),
    (dict(v1=BOW_IDX), "feature index 1 out of range"),
    (dict(v2=BOW_IDX), "feature index 2 out of range"),
    (dict(v1=BOW_IDX, v2=BOW_DESC), "feature vector 2: node ids must ascend and offsets must be monotone"),
    (dict(v1=BOW_OFFS, v2=BOW_OFFS), "feature vector 1: node ids must ascend and offsets must be monotone"),
    (dict(v1=BOW_IDX, v2=BOW_IDX), "feature index 1 out of range"),
    (dict(v1=BOW_DESC, v2=BOW_BIG), "feature vector larger than the key frame"),
]


@pytest.mark.parametrize("kw,msg", VEC_CASES)
def test_search_by_bow_keyframes_bad_arguments(kw, msg):
    check(two_vectors(bow_keyframes, **kw), E_BADARG, msg)


@pytest.mark.parametrize("fn", [triangulation, triangulation_rig])
@pytest.mark.parametrize("kw,msg", VEC_CASES + [
    (dict(k2=kps(4, octave=LEVELS)), None),
    (dict(k2=kps(4, octave=-1), v2=BOW_IDX), "feature index 2 out of range"),
])
def test_search_for_triangulation_bad_arguments(fn, kw, msg):
    if msg is None:
        msg = "keypoint octave outside [0, nlevels2)" if fn is triangulation else "keypoint octave outside [0, nlevels)"
    check(two_vectors(fn, **kw), E_BADARG, msg)


def test_search_for_triangulation_rig_checks_the_first_keyframe_octaves():
    check(two_vectors(triangulation_rig, k1=kps(4, octave=LEVELS)), E_BADARG, "keypoint octave outside [0, nlevels)")
    check(two_vectors(triangulation_rig, k1=kps(4, octave=-1), k2=kps(4, octave=LEVELS)), E_BADARG,
          "keypoint octave outside [0, nlevels)")


@pytest.mark.parametrize("fn", [triangulation, triangulation_rig])
def test_search_for_triangulation_feature_count_cap(fn):
    # the 2^24 cap comes before every array read: the arrays can stay small
    big = 1 << 24
    check(two_vectors(fn, n2=big, v2=(u32(1), i32(0, big), u32(0)), v1=BOW_DESC, k2=kps(1)), E_CAPACITY, "more than 2^24 features")


# ---- orbx_search_for_initialization / orbx_features_in_area
def search_init(n1=4, n2=4, k1=True, k2=True, prev=True):
    return orbx.lib().orbx_search_for_initialization(
        0, P(kps(n1)) if k1 else None, P(desc(n1)), n1, P(kps(n2)) if k2 else None, P(desc(n2)), n2, 0, 0, 640, 480,
        P(np.zeros(2 * max(n1, 1), np.float32)) if prev else None, P(np.zeros(max(n1, 1), np.int32)), 100, 0.9, 1)


@pytest.mark.parametrize("kw", [dict(n1=-1), dict(n2=-1), dict(k1=False), dict(prev=False), dict(k2=False),
                                dict(n1=0, n2=-1), dict(n1=-1, k2=False)])
def test_search_for_initialization_bad_arguments(kw):
    check(search_init(**kw), E_BADARG, BAD)


def test_search_for_initialization_without_keypoints_returns_before_the_device():
    assert search_init(n1=0, k1=False, prev=False) == 0
    assert search_init(n1=0, n2=0, k1=False, k2=False, prev=False) == 0


@pytest.mark.parametrize("kw", [dict(n=-1), dict(nq=-1), dict(kp=False), dict(q=False), dict(off=False), dict(n=-1, q=False)])
def test_features_in_area_bad_arguments(kw):
    n, nq = kw.get("n", 4), kw.get("nq", 2)
    rc = orbx.lib().orbx_features_in_area(0, P(kps(n)) if kw.get("kp", True) else None, n, 0, 0, 640, 480,
                                          P(np.zeros(5 * max(nq, 1), np.float32)) if kw.get("q", True) else None, nq,
                                          P(np.zeros(max(nq, 1) + 1, np.int32)) if kw.get("off", True) else None,
                                          None, 0, None, None)
    check(rc, E_BADARG, BAD)


# ---- the pinhole SearchByProjection family
def views(n, level=0, in_view=1):
    v = np.zeros(max(n, 1), MP_DTYPE)
    v["predicted_level"] = level
    v["in_view"] = in_view
    return v


def search_by_projection(n=4, nmp=2, nlev=LEVELS, scale=True, mps=None, occ=True):
    mps = views(nmp) if mps is None else mps
    return orbx.lib().orbx_search_by_projection(
        0, P(kps(n)) if n else None, P(desc(n)) if n else None, None, n, 0, 0, 640, 480,
        P(np.ones(LEVELS, np.float32)) if scale else None, nlev, P(mps), nmp, 1.0, 0, 0.0, 0.8,
        P(np.zeros(max(n, 1), np.uint8)) if occ else None, P(np.zeros(max(n, 1), np.int32)) if n else None)


LEVEL_MSG = "in-view map point with a predicted level outside [0, nlevels)"


@pytest.mark.parametrize("kw,msg", [
    (dict(n=-1), BAD), (dict(nmp=-1), BAD), (dict(nlev=0), BAD), (dict(scale=False), BAD), (dict(occ=False), BAD),
    (dict(mps=views(2, level=LEVELS)), LEVEL_MSG), (dict(mps=views(2, level=-1)), LEVEL_MSG),
    (dict(mps=views(2, level=LEVELS), occ=False), BAD),
    (dict(n=0, mps=views(2, level=LEVELS)), LEVEL_MSG),
])
def test_search_by_projection_bad_arguments(kw, msg):
    check(search_by_projection(**kw), E_BADARG, msg)


def test_search_by_projection_ignores_the_level_of_points_out_of_view():
    assert search_by_projection(n=0, mps=views(2, level=99, in_view=0)) == 0


def test_search_by_projection_without_keypoints_returns_before_the_device():
    assert search_by_projection(n=0) == 0
    assert search_by_projection(n=0, nmp=0) == 0


def projected(n):
    return np.zeros(max(n, 1), PP_DTYPE)


def projection_frame(n=4, npts=2, pts=True, occ=True):
    return orbx.lib().orbx_search_by_projection_frame(
        0, P(kps(n)) if n else None, P(desc(n)) if n else None, None, n, 0, 0, 640, 480, P(projected(2)) if pts else None, npts, 1,
        P(np.zeros(max(n, 1), np.uint8)) if occ else None, P(np.zeros(max(n, 1), np.int32)) if n else None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n=-1), E_BADARG, BAD), (dict(npts=-1), E_BADARG, BAD), (dict(pts=False), E_BADARG, BAD), (dict(occ=False), E_BADARG, BAD),
    (dict(npts=15001), E_CAPACITY, "more than 15000 projected points"),
    (dict(npts=15001, occ=False), E_BADARG, BAD),
])
def test_search_by_projection_frame_bad_arguments(kw, code, msg):
    check(projection_frame(**kw), code, msg)


def test_search_by_projection_frame_without_keypoints_returns_before_the_device():
    assert projection_frame(n=0) == 0
    assert projection_frame(n=0, npts=0, pts=False) == 0


def projection_keyframe(n=4, npts=2, pts=True, orb_dist=100):
    return orbx.lib().orbx_search_by_projection_keyframe(
        0, P(kps(n)) if n else None, P(desc(n)) if n else None, n, 0, 0, 640, 480, P(projected(2)) if pts else None, npts,
        orb_dist, 1, P(np.zeros(max(n, 1), np.uint8)), P(np.zeros(max(n, 1), np.int32)) if n else None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n=-1), E_BADARG, BAD), (dict(pts=False), E_BADARG, BAD),
    (dict(npts=15001), E_CAPACITY, "more than 15000 projected points"),
    (dict(orb_dist=256), E_BADARG, "ORBdist outside [0, 255]"), (dict(orb_dist=-1), E_BADARG, "ORBdist outside [0, 255]"),
    (dict(npts=15001, orb_dist=300), E_CAPACITY, "more than 15000 projected points"),
    (dict(n=0, orb_dist=300), E_BADARG, "ORBdist outside [0, 255]"),
])
def test_search_by_projection_keyframe_bad_arguments(kw, code, msg):
    check(projection_keyframe(**kw), code, msg)


def test_search_by_projection_keyframe_without_keypoints_returns_before_the_device():
    assert projection_keyframe(n=0) == 0


def fuse(n=4, npts=2, nlev=LEVELS, max_dist=50, pts=True, octave=0, k=None):
    k = kps(n, octave) if k is None else k
    return orbx.lib().orbx_fuse_search(
        0, P(k), P(desc(n)), None, n, 0, 0, 640, 480, P(np.ones(LEVELS, np.float32)), nlev,
        P(np.zeros(max(npts, 1), FP_DTYPE)) if pts else None, npts, max_dist, P(np.zeros(max(npts, 1), np.int32)), None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(max_dist=256), E_BADARG, "max_dist outside [0, 255]"), (dict(max_dist=-1), E_BADARG, "max_dist outside [0, 255]"),
    (dict(max_dist=300, n=-1), E_BADARG, "max_dist outside [0, 255]"),
    (dict(n=-1), E_BADARG, BAD), (dict(nlev=0), E_BADARG, BAD), (dict(pts=False), E_BADARG, BAD),
    (dict(n=1 << 20, k=kps(1)), E_CAPACITY, "more than 2^20 keypoints"),
    (dict(octave=LEVELS), E_BADARG, "keypoint octave outside [0, nlevels)"),
    (dict(octave=-1, pts=False), E_BADARG, BAD),
])
def test_fuse_search_bad_arguments(kw, code, msg):
    check(fuse(**kw), code, msg)


# ---- the stereo-fisheye SearchByProjection pair
def fisheye_projection(nL=3, nR=3, nmp=2, mps=None, mpr=None, l2r=None, r2l=None, nlev=LEVELS):
    mps = views(nmp) if mps is None else mps
    mpr = np.zeros(max(nmp, 1), MPR_DTYPE) if mpr is None else mpr
    l2r = np.full(max(nL, 1), -1, np.int32) if l2r is None else l2r
    r2l = np.full(max(nR, 1), -1, np.int32) if r2l is None else r2l
    n = max(nL + nR, 1)
    return orbx.lib().orbx_search_by_projection_fisheye(
        0, P(kps(n)), P(desc(n)), nL, nR, 0, 0, 640, 480, P(np.ones(LEVELS, np.float32)), nlev, P(mps), P(mpr), nmp, 1.0, 0, 0.0,
        0.8, P(l2r), P(r2l), P(np.zeros(n, np.uint8)), P(np.zeros(n, np.int32)))


def right_views(level, in_view=1):
    r = np.zeros(2, MPR_DTYPE)
    r["predicted_level_r"] = level
    r["in_view_r"] = in_view
    return r


FE_LEVEL_MSG = "map point with a predicted level outside [0, nlevels)"


@pytest.mark.parametrize("kw,msg", [
    (dict(nL=-1), BAD), (dict(nmp=-1), BAD), (dict(nlev=0), BAD),
    (dict(l2r=np.array([0, 3, -1], np.int32)), "left_to_right entry out of range"),
    (dict(l2r=np.array([-2, 0, -1], np.int32)), "left_to_right entry out of range"),
    (dict(r2l=np.array([0, 3, -1], np.int32)), "right_to_left entry out of range"),
    (dict(mps=views(2, level=LEVELS)), FE_LEVEL_MSG),
    (dict(mpr=right_views(LEVELS)), FE_LEVEL_MSG), (dict(mpr=right_views(-2)), FE_LEVEL_MSG),
    (dict(l2r=np.array([9, 0, 0], np.int32), r2l=np.array([9, 0, 0], np.int32)), "left_to_right entry out of range"),
    (dict(r2l=np.array([9, 0, 0], np.int32), mps=views(2, level=LEVELS)), "right_to_left entry out of range"),
    (dict(nlev=0, l2r=np.array([9, 0, 0], np.int32)), BAD),
])
def test_search_by_projection_fisheye_bad_arguments(kw, msg):
    check(fisheye_projection(**kw), E_BADARG, msg)


def test_search_by_projection_fisheye_without_keypoints_returns_before_the_device():
    assert fisheye_projection(nL=0, nR=0) == 0
    assert fisheye_projection(nL=0, nR=0, mps=views(2, level=3, in_view=0), mpr=right_views(-1)) == 0


def frame_fisheye(nL=3, nR=3, npts=2, uv=True):
    n = max(nL + nR, 1)
    return orbx.lib().orbx_search_by_projection_frame_fisheye(
        0, P(kps(n)), P(desc(n)), nL, nR, 0, 0, 640, 480, P(projected(2)), P(np.zeros(4, np.float32)) if uv else None, npts, 1,
        P(np.zeros(n, np.uint8)), P(np.zeros(n, np.int32)))


@pytest.mark.parametrize("kw,code,msg", [
    (dict(nL=-1), E_BADARG, BAD), (dict(npts=-1), E_BADARG, BAD), (dict(uv=False), E_BADARG, BAD),
    (dict(npts=15001), E_CAPACITY, "more than 15000 projected points"),
    (dict(npts=15001, uv=False), E_BADARG, BAD),
])
def test_search_by_projection_frame_fisheye_bad_arguments(kw, code, msg):
    check(frame_fisheye(**kw), code, msg)


def test_search_by_projection_frame_fisheye_without_keypoints_returns_before_the_device():
    assert frame_fisheye(nL=0, nR=0) == 0


# ---- the batched entries: null handle and bad frame counts
def batch_calls(ex, n_frames):
    lib = orbx.lib()
    one = np.ones(4, np.int32)
    buf = np.zeros(4096, np.uint8)
    b = P(buf)
    return {
        "bow": lib.orbx_search_by_bow_batch(ex, 0, n_frames, b, P(one), P(one), 1, b, b, b, b, P(one), 1, 0, 0.6, 1, b, b),
        "init": lib.orbx_search_for_initialization_batch(ex, 0, n_frames, b, b, P(one), 1, 0, 0, 640, 480, b, b, 100, 0.9, 1, b),
        "proj": lib.orbx_search_by_projection_batch(ex, 0, n_frames, 0, 0, 640, 480, b, P(one), 1, 1.0, 0, 0.0, 0.8, -1, None, b, b, b),
        "frame": lib.orbx_search_by_projection_frame_batch(ex, 0, n_frames, 0, 0, 640, 480, b, P(one), 1, 1, -1, None, b, b, b),
        "fisheye": lib.orbx_search_by_projection_fisheye_batch(ex, 0, 1, n_frames, 0, 0, 640, 480, b, b, P(one), 1, 1.0, 0, 0.0, 0.8,
                                                               b, b, None, b, b, b),
        "frame_fisheye": lib.orbx_search_by_projection_frame_fisheye_batch(ex, 0, 1, n_frames, 0, 0, 640, 480, b, b, P(one), 1, 1,
                                                                           None, b, b, b),
    }


@pytest.mark.parametrize("n_frames", [0, 1, -1])
def test_batched_matchers_reject_a_null_handle(n_frames):
    for name, rc in batch_calls(None, n_frames).items():
        assert rc == E_BADARG, name
        assert orbx.lib().orbx_last_error().decode() == BAD, name


def test_batched_matchers_reject_a_negative_frame_count():
    # a non-null handle that is never dereferenced: the count check comes first
    block = np.zeros(64, np.uint64)
    for name, rc in batch_calls(P(block), -1).items():
        assert rc == E_BADARG, name
        assert orbx.lib().orbx_last_error().decode() == BAD, name
