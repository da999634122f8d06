"""CPU pins of the geometric solvers' argument checks: for every one-shot entry (pose optimisation pinhole / KB8, two-view
reconstruction, the PnP and Sim3 solvers, orbx_triangulate_matches) one case per rejection it can make before it touches a
device, with the return code and the exact orbx_last_error() text, plus cases with two rejections at once that pin which one
is reported.  Every case is rejected: none may reach the device.  The two SetRansacParameters entries (host arithmetic only)
are pinned against recorded outputs."""
import ctypes as C

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import (E_BADARG, KP_DTYPE, POSE_DTYPE, POSE_KB8_DTYPE, TWO_VIEW_PARAMS_DTYPE, TWO_VIEW_RESULT_DTYPE,
                                MLPNP_PARAMS_DTYPE, MLPNP_STATE_DTYPE, MLPNP_RESULT_DTYPE, SIM3_PARAMS_DTYPE, SIM3_STATE_DTYPE,
                                SIM3_RESULT_DTYPE)

N = 8            # keypoints of a case
LEVELS = 8
NAN, INF = float("nan"), float("inf")

BAD = "bad argument"
CAM_MODEL = "camera model is neither pinhole nor KB8"
CAM_PARAMS = "camera parameters not finite, or fx / fy not positive"
CAM_PRECISION = "kb8_precision not finite and positive"
OCTAVE = "keypoint octave outside [0, nlevels)"
WORLD = "world position not finite"
SET_RANGE = "set index outside [0, n_correspondences)"
SET_REPEAT = "set index repeated within its set"
BEST = "state.best_inliers is not the number of correspondences flagged in best_mask"
COUNTER = "negative state counter"


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rejected(rc, msg):
    assert rc == E_BADARG
    assert orbx.lib().orbx_last_error().decode() == msg


def apply(arrays, edits):
    """edits: {"name": value} replaces an argument (None: a null pointer), {"name.field[i]": value} or {"name[i]": value}
    writes into a copy of the array."""
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
    for key, val in edits.items():
        if "[" not in key and "." not in key:
            a[key] = val
            continue
        name = key.split(".")[0].split("[")[0]
        rest = key[len(name):]
        field = rest[1:].split("[")[0] if rest.startswith(".") else None
        idx = int(rest[rest.index("[") + 1:rest.index("]")]) if "[" in rest else None
        tgt = a[name][field] if field else a[name]
        if idx is None:
            tgt[...] = val
        else:
            tgt.reshape(-1)[idx] = val
    return a


def keypoints(n=N):
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = np.arange(n) * 10.0, np.arange(n) * 7.0
    return k


# ---- orbx_pose_optimization
def pose_args():
    fr = np.zeros(1, POSE_DTYPE)
    fr["q"][0, 3] = 1
    fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["bf"] = 500, 500, 320, 240, 40
    return dict(kps=keypoints(), ur=None, wp=np.ones((N, 3), np.float32), hp=np.ones(N, np.uint8), n=N,
                sig=np.ones(LEVELS, np.float32), nlev=LEVELS, fr=fr, out=np.zeros(N, np.uint8))


POSE_FRAME = "pose or camera not finite (or a zero quaternion)"


@pytest.mark.parametrize("edits,msg", [
    ({"n": -1}, BAD), ({"fr": None}, BAD), ({"nlev": 0}, BAD), ({"nlev": 13}, BAD), ({"sig": None}, BAD), ({"kps": None}, BAD),
    ({"wp": None}, BAD), ({"hp": None}, BAD), ({"out": None}, BAD),
    ({"n": 15001}, "more than 15000 keypoints"),
    ({"fr.q[0]": NAN}, POSE_FRAME), ({"fr.t[2]": INF}, POSE_FRAME), ({"fr.fx": NAN}, POSE_FRAME), ({"fr.bf": INF}, POSE_FRAME),
    ({"fr.q": 0}, POSE_FRAME),
    ({"kps.octave[3]": -1}, OCTAVE), ({"kps.octave[3]": LEVELS}, OCTAVE),
    ({"wp[9]": NAN}, WORLD), ({"wp[23]": INF}, WORLD),
    # two at once: the first check in argument order, then the first offending row, then the octave within a row
    ({"n": 15001, "fr.q[0]": NAN}, "more than 15000 keypoints"),
    ({"fr.fx": NAN, "wp[0]": NAN}, POSE_FRAME),
    ({"wp[9]": NAN, "kps.octave[3]": -1}, OCTAVE),       # the same row: the octave is tested first
    ({"wp[9]": NAN, "kps.octave[5]": LEVELS}, WORLD),    # row 3 before row 5
    ({"wp[18]": NAN, "kps.octave[5]": LEVELS}, OCTAVE),  # row 5 before row 6
])
def test_pose_optimization_rejections(edits, msg):
    a = apply(pose_args(), edits)
    rejected(orbx.lib().orbx_pose_optimization(0, P(a["kps"]), P(a["ur"]), P(a["wp"]), P(a["hp"]), a["n"], P(a["sig"]), a["nlev"],
                                               P(a["fr"]), P(a["out"])), msg)


def test_pose_optimization_ignores_rows_without_a_point():
    a = apply(pose_args(), {"wp[9]": NAN, "hp[3]": 0, "kps.octave[3]": 99, "kps.octave[6]": -1})
    rejected(orbx.lib().orbx_pose_optimization(0, P(a["kps"]), None, P(a["wp"]), P(a["hp"]), N, P(a["sig"]), LEVELS, P(a["fr"]),
                                               P(a["out"])), OCTAVE)


# ---- orbx_pose_optimization_kb8
def kb8_args():
    fr = np.zeros(1, POSE_KB8_DTYPE)
    fr["q"][0, 3] = fr["trl_q"][0, 3] = 1
    fr["kb8_left"][0, :4] = fr["kb8_right"][0, :4] = (190, 190, 254, 256)
    return dict(kps=keypoints(), nl=5, nr=3, wp=np.ones((N, 3), np.float32), hp=np.ones(N, np.uint8),
                sig=np.ones(LEVELS, np.float32), nlev=LEVELS, fr=fr, out=np.zeros(N, np.uint8))


KB8_FRAME = "pose, KB8 parameters or Trl not finite (or a zero quaternion)"


@pytest.mark.parametrize("edits,msg", [
    ({"nl": -1}, BAD), ({"nr": -1}, BAD), ({"fr": None}, BAD), ({"nlev": 0}, BAD), ({"nlev": 13}, BAD), ({"sig": None}, BAD),
    ({"nl": 15000, "nr": 1}, "more than 15000 keypoints"), ({"nl": 2147483647, "nr": 2147483647}, "more than 15000 keypoints"),
    ({"kps": None}, BAD), ({"wp": None}, BAD), ({"hp": None}, BAD), ({"out": None}, BAD),
    ({"fr.q[1]": NAN}, KB8_FRAME), ({"fr.t[0]": INF}, KB8_FRAME), ({"fr.kb8_left[7]": NAN}, KB8_FRAME), ({"fr.q": 0}, KB8_FRAME),
    ({"fr.kb8_right[2]": NAN}, KB8_FRAME), ({"fr.trl_q[0]": NAN}, KB8_FRAME), ({"fr.trl_t[1]": INF}, KB8_FRAME),
    ({"fr.trl_q": 0}, KB8_FRAME),
    ({"kps.octave[6]": -1}, OCTAVE), ({"kps.octave[0]": LEVELS}, OCTAVE),
    ({"wp[2]": NAN}, WORLD), ({"wp[21]": INF}, WORLD),
    ({"nl": 15000, "nr": 1, "kps": None}, "more than 15000 keypoints"),
    ({"kps": None, "fr.q[1]": NAN}, BAD),
    ({"fr.q[1]": NAN, "kps.octave[0]": -1}, KB8_FRAME),
    ({"wp[3]": NAN, "kps.octave[1]": -1}, OCTAVE), ({"wp[3]": NAN, "kps.octave[2]": -1}, WORLD),
    # without a right camera neither Trl nor the right camera's parameters are read
    ({"nl": 8, "nr": 0, "fr.trl_q": 0, "fr.trl_t[0]": NAN, "fr.kb8_right[0]": NAN, "kps.octave[7]": -1}, OCTAVE),
])
def test_pose_optimization_kb8_rejections(edits, msg):
    a = apply(kb8_args(), edits)
    rejected(orbx.lib().orbx_pose_optimization_kb8(0, P(a["kps"]), a["nl"], a["nr"], P(a["wp"]), P(a["hp"]), P(a["sig"]), a["nlev"],
                                                   P(a["fr"]), P(a["out"])), msg)


# ---- orbx_reconstruct_two_views
TV_NULL = "null argument or negative count"
TV_PARAMS = "iterations outside [1, 4096], fx / fy / sigma not finite and positive, or cx / cy / rh_threshold not finite"
TV_TARGET = "match target outside [-1, n2)"
TV_SETS = "set index outside [0, n_matches) or repeated within its set"


def two_view_args():
    prm = np.zeros(1, TWO_VIEW_PARAMS_DTYPE)
    prm["fx"], prm["fy"], prm["cx"], prm["cy"], prm["sigma"], prm["rh_threshold"], prm["iterations"] = 500, 500, 320, 240, 1, 0.5, 2
    return dict(k1=keypoints(), n1=N, k2=keypoints(), n2=N, m=np.arange(N, dtype=np.int32),
                sets=np.array([[0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0]], np.int32), prm=prm,
                res=np.zeros(1, TWO_VIEW_RESULT_DTYPE), p3d=np.zeros((N, 3), np.float32), tri=np.zeros(N, np.uint8))


@pytest.mark.parametrize("edits,msg", [
    ({"res": None}, TV_NULL), ({"prm": None}, TV_NULL), ({"n1": -1}, TV_NULL), ({"n2": -1}, TV_NULL), ({"k1": None}, TV_NULL),
    ({"m": None}, TV_NULL), ({"p3d": None}, TV_NULL), ({"tri": None}, TV_NULL), ({"k2": None}, TV_NULL),
    ({"n1": 15001}, "more than 15000 keypoints"), ({"n2": 15001}, "more than 15000 keypoints"),
    ({"prm.iterations": 0}, TV_PARAMS), ({"prm.iterations": 4097}, TV_PARAMS), ({"prm.fx": 0}, TV_PARAMS), ({"prm.fx": NAN}, TV_PARAMS),
    ({"prm.fy": -1}, TV_PARAMS), ({"prm.fy": INF}, TV_PARAMS), ({"prm.sigma": 0}, TV_PARAMS), ({"prm.sigma": NAN}, TV_PARAMS),
    ({"prm.cx": NAN}, TV_PARAMS), ({"prm.cy": INF}, TV_PARAMS), ({"prm.rh_threshold": NAN}, TV_PARAMS),
    ({"m[2]": -2}, TV_TARGET), ({"m[7]": N}, TV_TARGET),
    ({"sets": None}, "null argument"),
    ({"sets[3]": -1}, TV_SETS), ({"sets[12]": N}, TV_SETS), ({"sets[15]": 7}, TV_SETS),
    ({"n1": 15001, "prm.fx": NAN}, "more than 15000 keypoints"),
    ({"prm.fx": NAN, "m[2]": -2}, TV_PARAMS),
    ({"m[2]": -2, "sets": None}, TV_TARGET),
    ({"sets[3]": -1, "sets[5]": 4}, TV_SETS),
])
def test_reconstruct_two_views_rejections(edits, msg):
    a = apply(two_view_args(), edits)
    rejected(orbx.lib().orbx_reconstruct_two_views(0, P(a["k1"]), a["n1"], P(a["k2"]), a["n2"], P(a["m"]), P(a["sets"]), P(a["prm"]),
                                                   P(a["res"]), P(a["p3d"]), P(a["tri"]), None), msg)


# ---- orbx_mlpnp_iterate: 8 keypoints, the first 7 for the solver (n_left), 2 sets
ML_NULL = "null argument, negative count or n_left above n"
ML_STATE = "state pose not finite"


def mlpnp_args():
    prm = orbx.mlpnp_params((500, 500, 320, 240), 6, 2, call_iterations=2)
    return dict(kps=keypoints(), n=N, nl=7, wp=np.ones((N, 3), np.float32), hp=np.ones(N, np.uint8),
                sig=np.ones(LEVELS, np.float32), nlev=LEVELS, prm=prm, sets=np.array([[0, 1, 2, 3, 4, 5], [6, 5, 4, 3, 2, 1]], np.int32),
                ns=2, st=np.zeros(1, MLPNP_STATE_DTYPE), bm=np.zeros(N, np.uint8), res=np.zeros(1, MLPNP_RESULT_DTYPE),
                inl=np.zeros(N, np.uint8))


KB8 = {"prm.model": 1, "prm.cam[4]": 0.01}


@pytest.mark.parametrize("edits,msg", [
    ({"n": -1}, ML_NULL), ({"nl": -1}, ML_NULL), ({"nl": N + 1}, ML_NULL), ({"ns": -1}, ML_NULL), ({"prm": None}, ML_NULL),
    ({"st": None}, ML_NULL), ({"res": None}, ML_NULL), ({"sig": None}, ML_NULL), ({"nlev": 0}, ML_NULL), ({"nlev": 13}, ML_NULL),
    ({"kps": None}, ML_NULL), ({"wp": None}, ML_NULL), ({"hp": None}, ML_NULL), ({"bm": None}, ML_NULL), ({"inl": None}, ML_NULL),
    ({"n": 15001}, "more than 15000 keypoints"),
    ({"prm.model": 2}, CAM_MODEL), ({"prm.model": -1}, CAM_MODEL),
    ({"prm.cam[2]": NAN}, CAM_PARAMS), ({"prm.cam[0]": 0}, CAM_PARAMS), ({"prm.cam[1]": -1}, CAM_PARAMS),
    ({**KB8, "prm.cam[7]": INF}, CAM_PARAMS),
    ({**KB8, "prm.kb8_precision": 0}, CAM_PRECISION), ({**KB8, "prm.kb8_precision": NAN}, CAM_PRECISION),
    ({"prm.th2": 0}, "th2 not finite and positive"), ({"prm.th2": INF}, "th2 not finite and positive"),
    ({"prm.min_set": 5}, "min_set other than 6"), ({"prm.min_inliers": 5}, "min_inliers below min_set"),
    ({"prm.max_iterations": 0}, "max_iterations outside [1, 4096]"), ({"prm.max_iterations": 4097}, "max_iterations outside [1, 4096]"),
    ({"prm.call_iterations": -1}, "call_iterations outside [0, 4096]"),
    ({"prm.call_iterations": 4097}, "call_iterations outside [0, 4096]"),
    ({"st.iterations": -1}, COUNTER), ({"st.best_inliers": -1}, COUNTER), ({"st.best_Tcw[11]": NAN}, ML_STATE),
    ({"sig[7]": NAN}, "level_sigma2 not finite"),
    ({"wp[4]": INF}, WORLD),
    ({"kps.octave[2]": -1}, OCTAVE), ({"kps.octave[6]": LEVELS}, OCTAVE),
    ({"kps.x[1]": NAN}, "keypoint not finite"), ({"kps.y[6]": INF}, "keypoint not finite"),
    ({"st.best_inliers": 1}, BEST), ({"bm[2]": 1}, BEST),
    ({"ns": 1}, "n_sets below max(max_iterations - state.iterations, call_iterations)"),
    ({"sets": None}, "null argument"),
    ({"sets[4]": -1}, SET_RANGE), ({"sets[6]": 7}, SET_RANGE), ({"sets[11]": 6}, SET_REPEAT),
    # two at once
    ({"n": 15001, "prm.model": 2}, "more than 15000 keypoints"),
    ({"prm.cam[2]": NAN, "prm.th2": -1}, CAM_PARAMS),                # non-finite camera and bad th2
    ({"prm.model": 2, "prm.cam[2]": NAN}, CAM_MODEL),
    ({"prm.cam[2]": NAN, "prm.kb8_precision": NAN, "prm.model": 1}, CAM_PARAMS),
    ({"prm.th2": -1, "prm.min_set": 5}, "th2 not finite and positive"),
    ({"prm.max_iterations": 0, "st.iterations": -1}, "max_iterations outside [1, 4096]"),
    ({"st.iterations": -1, "sig[0]": NAN}, COUNTER),
    ({"sig[0]": NAN, "wp[0]": NAN}, "level_sigma2 not finite"),
    ({"wp[18]": NAN, "kps.octave[0]": -1}, WORLD),                   # every world position before any octave
    ({"wp[0]": NAN, "kps.octave[0]": -1}, WORLD),
    ({"kps.octave[3]": -1, "kps.x[3]": NAN}, OCTAVE), ({"kps.octave[3]": -1, "kps.x[2]": NAN}, "keypoint not finite"),
    ({"kps.octave[3]": -1, "st.best_inliers": 1}, OCTAVE),
    ({"st.best_inliers": 1, "ns": 1}, BEST),                          # best_inliers mismatch and too few sets
    ({"ns": 1, "sets": None}, "n_sets below max(max_iterations - state.iterations, call_iterations)"),
    ({"sets[0]": 9, "sets[2]": 1}, SET_RANGE),                        # out of range and a repeat in one set: position 0 first
    ({"sets[1]": 0, "sets[2]": 9}, SET_REPEAT),                       # ... the repeat at position 1 before the range at 2
    ({"sets[5]": 4, "sets[6]": -1}, SET_REPEAT),                      # set 0 before set 1
    # rows past n_left and rows without a point are not read
    ({"wp[21]": NAN, "kps.octave[7]": 99, "wp[9]": NAN, "hp[3]": 0, "kps.octave[3]": -1, "sets[0]": 6}, SET_RANGE),
])
def test_mlpnp_iterate_rejections(edits, msg):
    a = apply(mlpnp_args(), edits)
    rejected(orbx.lib().orbx_mlpnp_iterate(0, P(a["kps"]), a["n"], a["nl"], P(a["wp"]), P(a["hp"]), P(a["sig"]), a["nlev"],
                                           P(a["prm"]), P(a["sets"]), a["ns"], P(a["st"]), P(a["bm"]), P(a["res"]), P(a["inl"]), None),
             msg)


# ---- orbx_sim3_iterate: 8 key points, 2 sets
S3_NULL = "null argument, negative count or nlevels outside [1, ORBX_MAX_LEVELS]"
S3_STATE = "state transformation not finite"
S3_SIGMA = "level_sigma2 not finite or outside [0, 1e9]"
S3_OCTAVE = "octave outside [0, nlevels)"
S3_SETS = "n_sets below min(max_iterations - state.iterations, call_iterations)"
ITER = "max_iterations outside [1, 4096]"


def sim3_args():
    prm = orbx.sim3_params((500, 500, 320, 240), (450, 450, 300, 200), 3, 2, call_iterations=2)
    T = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    return dict(n=N, T1=T, T2=T.copy(), w1=np.ones((N, 3), np.float32), w2=np.ones((N, 3), np.float32), m=np.ones(N, np.uint8),
                o1=np.zeros(N, np.int32), o2=np.zeros(N, np.int32), s1=np.ones(LEVELS, np.float32), nl1=LEVELS,
                s2=np.ones(LEVELS, np.float32), nl2=LEVELS, prm=prm, sets=np.array([[0, 1, 2], [7, 6, 5]], np.int32), ns=2,
                st=np.zeros(1, SIM3_STATE_DTYPE), bm=np.zeros(N, np.uint8), res=np.zeros(1, SIM3_RESULT_DTYPE),
                inl=np.zeros(N, np.uint8))


@pytest.mark.parametrize("edits,msg", [
    ({"n": -1}, S3_NULL), ({"ns": -1}, S3_NULL), ({"T1": None}, S3_NULL), ({"T2": None}, S3_NULL), ({"prm": None}, S3_NULL),
    ({"st": None}, S3_NULL), ({"res": None}, S3_NULL), ({"s1": None}, S3_NULL), ({"s2": None}, S3_NULL), ({"nl1": 0}, S3_NULL),
    ({"nl1": 13}, S3_NULL), ({"nl2": 0}, S3_NULL), ({"nl2": 13}, S3_NULL), ({"w1": None}, S3_NULL), ({"w2": None}, S3_NULL),
    ({"m": None}, S3_NULL), ({"o1": None}, S3_NULL), ({"o2": None}, S3_NULL), ({"bm": None}, S3_NULL), ({"inl": None}, S3_NULL),
    ({"n": 15001}, "more than 15000 key points"),
    ({"prm.model1": 2}, CAM_MODEL), ({"prm.model2": -1}, CAM_MODEL),
    ({"prm.cam1[3]": NAN}, CAM_PARAMS), ({"prm.cam1[0]": 0}, CAM_PARAMS), ({"prm.cam2[1]": -2}, CAM_PARAMS),
    ({"prm.cam2[2]": INF}, CAM_PARAMS), ({"prm.model2": 1, "prm.cam2[6]": NAN}, CAM_PARAMS),
    ({"prm.model1": 1, "prm.kb8_precision": 0}, CAM_PRECISION), ({"prm.model2": 1, "prm.kb8_precision": NAN}, CAM_PRECISION),
    ({"prm.min_inliers": 2}, "min_inliers below 3"),
    ({"prm.max_iterations": 0}, ITER), ({"prm.max_iterations": 4097}, ITER),
    ({"prm.call_iterations": -1}, "call_iterations outside [0, 4096]"),
    ({"prm.call_iterations": 4097}, "call_iterations outside [0, 4096]"),
    ({"st.iterations": -1}, COUNTER), ({"st.best_inliers": -1}, COUNTER),
    ({"st.best_R[8]": NAN}, S3_STATE), ({"st.best_t[0]": INF}, S3_STATE), ({"st.best_s": NAN}, S3_STATE),
    ({"s1[7]": NAN}, S3_SIGMA), ({"s1[0]": -1}, S3_SIGMA), ({"s2[3]": 2e9}, S3_SIGMA), ({"s2[0]": INF}, S3_SIGMA),
    ({"T1[11]": NAN}, "key-frame pose not finite"), ({"T2[0]": INF}, "key-frame pose not finite"),
    ({"w1[5]": NAN}, WORLD), ({"w2[23]": INF}, WORLD),
    ({"o1[2]": -1}, S3_OCTAVE), ({"o1[2]": LEVELS}, S3_OCTAVE), ({"o2[7]": -1}, S3_OCTAVE), ({"o2[7]": LEVELS}, S3_OCTAVE),
    ({"st.best_inliers": 2}, BEST), ({"bm[7]": 1}, BEST),
    ({"ns": 1}, S3_SETS), ({"sets": None}, "null argument"),
    ({"sets[2]": -1}, SET_RANGE), ({"sets[3]": N}, SET_RANGE), ({"sets[5]": 7}, SET_REPEAT),
    # two at once
    ({"n": 15001, "prm.model1": 2}, "more than 15000 key points"),
    ({"prm.cam1[3]": NAN, "prm.model2": 2}, CAM_PARAMS),              # camera 1 before camera 2
    ({"prm.model2": 2, "prm.min_inliers": 2}, CAM_MODEL),
    ({"prm.min_inliers": 2, "prm.max_iterations": 0}, "min_inliers below 3"),
    ({"prm.call_iterations": -1, "st.iterations": -1}, "call_iterations outside [0, 4096]"),
    ({"st.best_s": NAN, "s1[0]": -1}, S3_STATE),
    ({"s1[0]": -1, "T1[0]": NAN}, S3_SIGMA), ({"s2[0]": -1, "T1[0]": NAN}, S3_SIGMA),
    ({"T2[0]": NAN, "w1[0]": NAN}, "key-frame pose not finite"),
    ({"w1[9]": NAN, "o1[3]": -1}, WORLD),                              # the same row: the world position is tested first
    ({"w2[9]": NAN, "o2[2]": -1}, S3_OCTAVE),                          # row 2 before row 3
    ({"o1[4]": -1, "st.best_inliers": 2}, S3_OCTAVE),
    ({"st.best_inliers": 2, "ns": 1}, BEST),                           # best_inliers mismatch and too few sets
    ({"ns": 1, "sets": None}, S3_SETS),
    ({"sets[0]": 9, "sets[2]": 1}, SET_RANGE), ({"sets[1]": 0, "sets[2]": 9}, SET_REPEAT), ({"sets[2]": 1, "sets[3]": -1}, SET_REPEAT),
    # rows that are not matched are not read, and do not count as correspondences: 7 of them, index 7 is out of range
    ({"m[3]": 0, "w1[9]": NAN, "o2[3]": 99}, SET_RANGE),
])
def test_sim3_iterate_rejections(edits, msg):
    a = apply(sim3_args(), edits)
    rejected(orbx.lib().orbx_sim3_iterate(0, a["n"], P(a["T1"]), P(a["T2"]), P(a["w1"]), P(a["w2"]), P(a["m"]), P(a["o1"]), P(a["o2"]),
                                          P(a["s1"]), a["nl1"], P(a["s2"]), a["nl2"], P(a["prm"]), P(a["sets"]), a["ns"], P(a["st"]),
                                          P(a["bm"]), P(a["res"]), P(a["inl"]), None), msg)


# ---- orbx_triangulate_matches
def keyframe(**kw):
    cam = orbx.np_camera((500, 500, 320, 240), np.eye(4)[:3])
    return orbx.NpKeyFrame(kw.pop("cameras", cam), keypoints(), np.ones(LEVELS), np.ones(LEVELS), **kw)


def triangulate(kf1=None, kf2=None, edit1=None, edit2=None, prm=None, m=True, status=True, x3d=True, ps=True, match=None,
                null1=False, null2=False, null_prm=False):
    kf1, kf2 = kf1 or keyframe(), kf2 or keyframe()
    for kf, edit in ((kf1, edit1), (kf2, edit2)):
        if edit:
            edit(kf.c)
    prm = prm or orbx._np_params(40.0, False, False, 0.0, 1.8)
    mm = np.arange(N, dtype=np.int32)
    if match:
        mm[match[0]] = match[1]
    keep = [np.zeros(N, np.uint8), np.zeros((N, 3), np.float32), np.zeros(N, np.uint8)]
    return orbx.lib().orbx_triangulate_matches(0, None if null1 else C.addressof(kf1.c), None if null2 else C.addressof(kf2.c),
                                               P(mm) if m else None, None if null_prm else C.addressof(prm),
                                               P(keep[0]) if status else None, P(keep[1]) if x3d else None, P(keep[2]) if ps else None)


def setf(path, value):
    """an edit of a key-frame record: setf("cam[0].p[2]", nan)"""
    def edit(c):
        exec("c.%s = v" % path, {"c": c, "v": value})
    return edit


def both(*edits):
    def edit(c):
        for e in edits:
            e(c)
    return edit


NP_POSE = "key frame pose not finite"
NP_LEFT1 = "n_left must be -1 for a single-camera key frame"
NP_UR = "u_right and depth must both be given or both be NULL"
KEYFRAME_EDITS = [
    (setf("n", -1), BAD), (setf("nlevels", 0), BAD), (setf("scale_factors", None), BAD), (setf("level_sigma2", None), BAD),
    (setf("kps", None), BAD),
    (setf("n_cameras", 0), "n_cameras is neither 1 nor 2"), (setf("n_cameras", 3), "n_cameras is neither 1 nor 2"),
    (setf("n_left", 0), NP_LEFT1),
    (both(setf("n_cameras", 2), setf("n_left", -1)), "n_left outside [0, n]"),
    (both(setf("n_cameras", 2), setf("n_left", N + 1)), "n_left outside [0, n]"),
    (setf("u_right", 8), NP_UR), (setf("depth", 8), NP_UR),
    (setf("mb", NAN), "mb not finite"),
    (setf("cam[0].model", 2), CAM_MODEL), (setf("cam[0].p[3]", NAN), CAM_PARAMS), (setf("cam[0].p[0]", 0), CAM_PARAMS),
    (setf("cam[0].p[1]", -1), CAM_PARAMS), (both(setf("cam[0].model", 1), setf("cam[0].p[5]", INF)), CAM_PARAMS),
    (both(setf("cam[0].model", 1), setf("cam[0].kb8_precision", 0)), CAM_PRECISION),
    (setf("cam[0].Tcw[11]", NAN), NP_POSE), (setf("cam[0].Ow[1]", INF), NP_POSE),
    # two at once, in the order of the checks
    (both(setf("n", -1), setf("n_cameras", 3)), BAD),
    (both(setf("n_cameras", 3), setf("n_left", 0)), "n_cameras is neither 1 nor 2"),
    (both(setf("n_left", 0), setf("depth", 8)), NP_LEFT1),
    (both(setf("depth", 8), setf("mb", INF)), NP_UR),
    (both(setf("mb", INF), setf("cam[0].model", 2)), "mb not finite"),
    (both(setf("cam[0].model", 2), setf("cam[0].p[3]", NAN)), CAM_MODEL),
    (both(setf("cam[0].p[3]", NAN), setf("cam[0].Tcw[0]", NAN)), CAM_PARAMS),
    (both(setf("cam[0].model", 1), setf("cam[0].kb8_precision", -1), setf("cam[0].Ow[0]", NAN)), CAM_PRECISION),
]


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("case", range(len(KEYFRAME_EDITS)))
def test_triangulate_matches_keyframe_rejections(case, which):
    edit, msg = KEYFRAME_EDITS[case]
    rejected(triangulate(**{"edit%d" % which: edit}), msg)


def test_triangulate_matches_keypoint_octaves():
    for octave in (-1, LEVELS):
        kf = keyframe()
        kf.kps["octave"][5] = octave
        rejected(triangulate(kf1=kf), OCTAVE)
        rejected(triangulate(kf2=kf), OCTAVE)
    kf = keyframe()
    kf.kps["octave"][5] = -1
    rejected(triangulate(kf1=kf, edit1=setf("cam[0].Ow[0]", NAN)), NP_POSE)   # the cameras before the octaves


def two_camera_keyframe():
    cam = orbx.np_camera((190, 190, 254, 256, 0.01, 0, 0, 0), np.eye(4)[:3])
    return keyframe(cameras=(cam, cam), n_left=5)


@pytest.mark.parametrize("edit,msg", [
    (setf("cam[1].model", 2), CAM_MODEL), (setf("cam[1].p[7]", NAN), CAM_PARAMS), (setf("cam[1].kb8_precision", NAN), CAM_PRECISION),
    (setf("cam[1].Tcw[3]", INF), NP_POSE), (both(setf("cam[0].Ow[0]", NAN), setf("cam[1].model", 2)), NP_POSE),
])
def test_triangulate_matches_second_camera_rejections(edit, msg):
    rejected(triangulate(kf1=two_camera_keyframe(), kf2=two_camera_keyframe(), edit1=edit), msg)
    rejected(triangulate(kf1=two_camera_keyframe(), kf2=two_camera_keyframe(), edit2=edit), msg)


def test_triangulate_matches_call_rejections():
    rejected(triangulate(null1=True), "null key frame")
    rejected(triangulate(null2=True), "null key frame")
    rejected(triangulate(null_prm=True), "null params")
    for prm in (orbx._np_params(NAN, False, False, 0.0, 1.8), orbx._np_params(40.0, False, False, 0.0, INF),
                orbx._np_params(40.0, False, True, NAN, 1.8)):
        rejected(triangulate(prm=prm), "params not finite")
    rejected(triangulate(kf2=two_camera_keyframe()), "both key frames must be single-camera or both two-camera")
    rejected(triangulate(kf1=two_camera_keyframe()), "both key frames must be single-camera or both two-camera")
    for kw in (dict(m=False), dict(status=False), dict(x3d=False), dict(ps=False)):
        rejected(triangulate(**kw), BAD)
    rejected(triangulate(match=(2, -2)), "match index outside [-1, n2)")
    rejected(triangulate(match=(7, N)), "match index outside [-1, n2)")
    # two at once: key frame 1, key frame 2, the params, the camera counts, the arrays, the matches
    rejected(triangulate(edit1=setf("mb", NAN), edit2=setf("n_cameras", 3)), "mb not finite")
    rejected(triangulate(edit2=setf("n_cameras", 3), null_prm=True), "n_cameras is neither 1 nor 2")
    rejected(triangulate(null_prm=True, kf2=two_camera_keyframe()), "null params")
    rejected(triangulate(kf2=two_camera_keyframe(), m=False), "both key frames must be single-camera or both two-camera")
    rejected(triangulate(status=False, match=(2, -2)), BAD)
    # a single-camera key frame's second camera is not read
    rejected(triangulate(edit1=setf("cam[1].model", 7), match=(2, -2)), "match index outside [-1, n2)")


# ---- the SetRansacParameters entries: outputs recorded from the library before the checks were shared
@pytest.mark.parametrize("args,expect", [
    ((0, 0.99, 8, 300, 6, 0.4), (8, 1, 0.4)),          # N == 0
    ((10, 0.99, 10, 300, 6, 0.5), (10, 1, 1.0)),       # min_inliers == N
    ((6, 0.99, 3, 300, 6, 0.2), (6, 1, 1.0)),          # ... after min_set raised it
    ((8, 0.99, 10, 300, 6, 0.5), (10, 1, 1.25)),       # min_inliers > N: NaN -> INT_MIN -> 1
    ((100, 0.99, 10, 300, 6, 0.5), (50, 35, 0.5)),
    ((30, 0.99, 8, 300, 6, 0.4), (12, 70, 0.4)),
    ((50, 0.99, 10, 5, 6, 0.5), (25, 5, 0.5)),         # clamped by max_iterations
    ((40, 0.5, 10, 300, 6, 0.9), (36, 1, 0.9)),
])
def test_mlpnp_ransac_parameters(args, expect):
    mi, it, ep = C.c_int32(-7), C.c_int32(-7), C.c_float(-7)
    assert orbx.lib().orbx_mlpnp_ransac_parameters(*args, C.addressof(mi), C.addressof(it), C.addressof(ep)) == 0
    assert (mi.value, it.value) == expect[:2]
    assert np.float32(ep.value).tobytes() == np.float32(expect[2]).tobytes()
    assert orbx.lib().orbx_mlpnp_ransac_parameters(*args, None, None, None) == 0


@pytest.mark.parametrize("args,expect", [
    ((0, 0.99, 6, 300), 1),        # N == 0
    ((20, 0.99, 20, 300), 1),      # min_inliers == N
    ((10, 0.99, 15, 300), 1),      # min_inliers > N: NaN -> INT_MIN -> 1
    ((30, 0.99, 0, 300), 1),       # epsilon 0: -inf -> INT_MIN -> 1
    ((40, 0.99, 15, 300), 86),
    ((40, 0.99, 15, 50), 50),      # clamped by max_iterations
    ((100, 0.99, 20, 300), 300),
    ((12, 0.999, 3, 300), 300),
])
def test_sim3_ransac_parameters(args, expect):
    it = C.c_int32(-7)
    assert orbx.lib().orbx_sim3_ransac_parameters(*args, C.addressof(it)) == 0
    assert it.value == expect
    assert orbx.lib().orbx_sim3_ransac_parameters(*args, None) == 0


def _octree_grid(n, x0=3, y0=3, w=50):
    """n distinct pixels, row by row from (x0, y0) in rows of w."""
    return [(x0 + i % w, y0 + i // w, 20) for i in range(n)]


# orbx_debug_octree (k_octree alone on the caller's candidates): everything it rejects is rejected by orbx_debug_octree_check, on the
# host, before a handle or the device is touched.  Window 100 x 38 (frame 132 x 70, one level): 2 x 1 FAST cells of 50 x 38 px with
# 25 * 19 = 475 slots each, a dense list of 52 * 21 = 1092 candidates, detectable pixels 3 <= x < 97, 3 <= y < 35.
@pytest.mark.parametrize("cand,msg", [
    ([(2, 10, 20)], "candidate outside the level's detectable window"),
    ([(97, 10, 20)], "candidate outside the level's detectable window"),
    ([(10, 2, 20)], "candidate outside the level's detectable window"),
    ([(10, 35, 20)], "candidate outside the level's detectable window"),
    ([(-1, 10, 20)], "candidate outside the level's detectable window"),
    ([(10, 10, 0)], "candidate response outside 1 .. 255"),
    ([(10, 10, 256)], "candidate response outside 1 .. 255"),
    ([(10, 10, 20), (11, 10, 20), (10, 10, 21)], "candidate pixel given twice"),
    (_octree_grid(476), "more candidates in one FAST cell than it has slots (cellCap)"),
    (_octree_grid(1093, w=94), "more candidates than the level's dense list holds (candCap)"),
])
def test_debug_octree_rejections(cand, msg):
    with pytest.raises(orbx.OrbxError) as e:
        orbx.octree_check(40, 1.2, 1, 20, 7, 132, 70, [[np.zeros((0, 3), np.int32)], [cand]])   # (in the second image of two)
    assert e.value.code == E_BADARG and orbx.lib().orbx_last_error().decode() == msg


def test_debug_octree_accepts_the_limits():
    edge = [(3, 3, 1), (96, 34, 255), (96, 3, 255), (3, 34, 1)]
    orbx.octree_check(40, 1.2, 1, 20, 7, 132, 70, [[edge], [_octree_grid(475)], [_octree_grid(475) + _octree_grid(475, x0=53, w=44)]])
    orbx.octree_check(40, 1.2, 1, 20, 7, 132, 70, [[[]]])


def test_ransac_parameters_negative_count():
    rejected(orbx.lib().orbx_mlpnp_ransac_parameters(-1, 0.99, 8, 300, 6, 0.4, None, None, None), "negative count")
    rejected(orbx.lib().orbx_sim3_ransac_parameters(-1, 0.99, 6, 300, None), "negative count")
