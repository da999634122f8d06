"""The table of tests/test_scratch_reuse.py: one case per one-shot entry of the C ABI (include/orbx.h), named after the entry
(`entry` or `entry:variant`).  A case is a builder: called with the oracle module it returns (run, check).  run() calls the
entry once on fixed inputs and returns everything the entry writes -- the Python wrappers hand it fresh output arrays of one
fixed pattern on every call (zeros, -1 or the caller's flags) --, check(result) is the reference comparison the entry already
has in its own test file, with that file's bound.  The inputs come from the entries' own case modules and scene builders; no
device is touched before run().

run_protocol() is the test: the pool trimmed, one warm-up run whose blocks then sit in the cache, and three runs on cached
blocks (and a staging buffer) filled with 0x00, 0xFF and 0x55.  Nothing a call computes may depend on what an earlier call
left in the memory it is given, so the three results must agree byte for byte.
"""
import numpy as np

import orb_slam3_fast_amd as orbx

# what the recycled memory holds: zero floats and integers; NaN in every float and double, -1 in every integer; a large finite
# float (1.5e13) and a large positive integer, which a kernel that merely filters NaN would swallow
POISON = (0x00, 0xFF, 0x55)

CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return reg


def entry_of(name):
    return name.split(":")[0]


# ------------------------------------------------------------------------------------------------ the protocol
def flatten(x, path="result"):
    """Every array, record and number of a result as (path, bytes), in the result's own order."""
    if x is None:
        return [(path, b"None")]
    if isinstance(x, dict):
        return [p for k, v in x.items() for p in flatten(v, "%s[%r]" % (path, k))]
    if isinstance(x, (list, tuple)):
        return [p for i, v in enumerate(x) for p in flatten(v, "%s[%d]" % (path, i))]
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        return [(path, repr((a.dtype.str if a.dtype.names is None else a.dtype.descr, a.shape)).encode() + a.tobytes())]
    if isinstance(x, (bool, int, float, str)):
        return [(path, repr(x).encode())]
    raise TypeError("%s: a result holds a %s" % (path, type(x).__name__))


def first_difference(a, b):
    """The first output of two flattened results whose bytes differ (None: equal), with the first differing byte."""
    if [p for p, _ in a] != [p for p, _ in b]:
        return "the results are not made of the same outputs"
    for (p, x), (_, y) in zip(a, b):
        if x != y:
            n = min(len(x), len(y))
            at = next((i for i in range(n) if x[i] != y[i]), n)
            return "%s differs from byte %d on (%d bytes)" % (p, at, len(x))
    return None


def run_protocol(name, oracle, device=0):
    """The protocol of the module docstring on case `name`.  Returns the three flattened results' difference report (empty when
    they agree) after the cache condition has been asserted and result A has passed its reference check."""
    run, check = CASES[name](oracle)
    orbx.scratch_pool_trim(device)
    assert orbx.scratch_pool_stats(device)[:2] == (0, 0)
    run()                                                   # warm-up: its blocks now sit in the cache
    results = []
    for byte in POISON:
        filled = orbx.scratch_pool_fill(byte, device)
        before = orbx.scratch_pool_stats(device)
        assert filled == before[1] > 0, "%s: the warm-up run left no block in the cache" % name
        results.append(run())
        after = orbx.scratch_pool_stats(device)
        takes, hits = after[2] - before[2], after[3] - before[3]
        assert takes >= 1 and hits == takes, "%s, fill 0x%02X: %d of %d blocks came from the cache" % (name, byte, hits, takes)
    flat = [flatten(r) for r in results]
    report = []
    for k in (1, 2):
        d = first_difference(flat[0], flat[k])
        if d:
            report.append("0x00 against 0x%02X: %s" % (POISON[k], d))
    if check is not None:
        check(results[0])
    return report


def crafted_handle(frames, nfeatures=1000, w=640, h=480):
    """An extraction batch whose images are overwritten with the given (keypoints, descriptors or None) (orbx_debug_upload_results):
    the batched entries that read a handle's keypoints see crafted sets of different sizes, an empty one among them."""
    from orb_slam3_fast_amd import synth
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    F = len(frames)
    ex = orbx.ORBextractor(nfeatures, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dev = DeviceBuffer.from_numpy(np.stack([synth.mono_frame(w, h, 3, 0)] * F))
    ex.extract_batch_device(dev.ptr.value, F, w, h, w, w * h)
    ex.sync()
    for f, (k, d) in enumerate(frames):
        n = len(k)
        assert n <= ex.capacity
        d = np.zeros((n, 32), np.uint8) if d is None else d
        orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, f, orbx._p(np.ascontiguousarray(k)) if n else None,
                                                         orbx._p(np.ascontiguousarray(d)) if n else None, n, n))
    ex._keep = dev
    return ex


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------------ matchers and one-shot helpers
def _column():
    import matcher_cases as mc
    k2, d2, twins = mc.column_frame()
    return mc, k2, d2, twins


@case("orbx_bf_knn2")
def _(oracle):
    mc, k2, d2, _ = _column()
    _, d1, _ = mc.init_case(k2, d2)
    q = np.concatenate([d1, d2[:30]])     # 66 queries on 198 train rows, 30 of them at distance 0

    def check(r):
        want = oracle.bf_knn2(q, d2)
        assert all(np.array_equal(a, b) for a, b in zip(r, want))
    return (lambda: orbx.bf_knn2(q, d2)), check


@case("orbx_search_for_initialization")
def _(oracle):
    mc, k2, d2, _ = _column()
    k1, d1, prev = mc.init_case(k2, d2)   # candidate totals above the first capacity guess: the entry repeats its fill

    def check(r):
        on, om12, oprev = oracle.search_init(k1, d1, k2, d2, mc.BOUNDS, prev, 100, 0.9, True)
        assert on >= 5 and r[0] == on and np.array_equal(r[1], om12) and same(np.asarray(r[2], np.float32), np.asarray(oprev, np.float32))
    return (lambda: orbx.ORBmatcher(0.9, True).SearchForInitialization(k1, d1, k2, d2, mc.BOUNDS, prev, 100)), check


@case("orbx_features_in_area")
def _(oracle):
    mc, k2, d2, _ = _column()
    q = mc.area_queries()

    def check(r):
        res = r[0]
        for i in range(len(q)):
            assert np.array_equal(res[i], oracle.features_in_area(k2, mc.BOUNDS, *q[i, :3], int(q[i, 3]), int(q[i, 4]))), i
    return (lambda: orbx.GetFeaturesInArea(k2, mc.BOUNDS, q, return_grid=True)), check


def _projection(which):
    def build(oracle):
        mc, k2, d2, twins = _column()
        mps, pts, fp, uR = mc.projection_points(k2, d2)
        occ = (np.arange(len(k2)) % 17 == 0).astype(np.uint8)
        if which == "map":
            run = lambda: orbx.ORBmatcher(0.9, True).SearchByProjection(k2, d2, uR, mc.BOUNDS, mc.SCALE, mps, occ, 25.0, False, 50.0)
            want = lambda: oracle.search_by_projection(k2, d2, uR, mc.BOUNDS, mc.SCALE, mps, 25.0, False, 50.0, 0.9, occ)
        elif which == "frame":
            run = lambda: orbx.ORBmatcher(0.9, True).SearchByProjectionFrame(k2, d2, uR, mc.BOUNDS, pts, occ)
            want = lambda: oracle.search_by_projection_frame(k2, d2, uR, mc.BOUNDS, pts, True, occ)
        else:
            fpt = mc.fuse_twins(fp, k2, d2, twins)
            inv = (1.0 / (mc.SCALE * mc.SCALE)).astype(np.float32)
            run = lambda: orbx.ORBmatcher(0.9, True).FuseSearch(k2, d2, uR, mc.BOUNDS, inv, fpt)
            want = lambda: oracle.fuse_search(k2, d2, uR, mc.BOUNDS, inv, fpt)

        def check(r):
            w = want()
            assert w[0] >= (1 if which == "fuse" else 5) and r[0] == w[0] and np.array_equal(r[1], w[1]) and np.array_equal(r[2], w[2])
        return run, check
    return build


CASES["orbx_search_by_projection"] = _projection("map")
CASES["orbx_search_by_projection_frame"] = _projection("frame")
CASES["orbx_fuse_search"] = _projection("fuse")


def _keyframe_flavour(oracle):
    """The relocalisation flavour on the small frame pair of tests/test_reloc_triangulation.py."""
    import test_reloc_triangulation as T
    f = T._frames(oracle, 480, 360, 500, 310)
    rng = np.random.default_rng(33)
    pts = T._kf_points(orbx, rng, f, 10.0)
    occ = (rng.random(len(f["k2"])) < 0.3).astype(np.uint8)

    def check(r):
        w = oracle.search_by_projection_keyframe(f["k2"], f["d2"], f["bounds"], pts, 100, True, occ)
        assert w[0] > 20 and r[0] == w[0] and np.array_equal(r[1], w[1]) and np.array_equal(r[2], w[2])
    return (lambda: orbx.ORBmatcher(0.9, True).SearchByProjectionKeyFrame(f["k2"], f["d2"], f["bounds"], pts, occ, 100)), check


CASES["orbx_search_by_projection_keyframe"] = _keyframe_flavour
# the same call in a process of its own whose first candidate capacity is 64 (ORBX_PROJ_CAND_CAP, read once per process): pass one
# of the walk runs against a full array, then the entry repeats the attempt, with a second round of scratch
CASES["orbx_search_by_projection_keyframe:small_capacity"] = _keyframe_flavour
SMALL_CAPACITY = {"orbx_search_by_projection_keyframe:small_capacity": {"ORBX_PROJ_CAND_CAP": "64"}}


def _small_pair(oracle):
    import test_reloc_triangulation as T
    return T, T._frames(oracle, 480, 360, 500, 310)


@case("orbx_search_for_triangulation")
def _(oracle):
    T, f = _small_pair(oracle)
    fv1, mp1, ur1, fv2, mp2, ur2, ep, F = T._tri_inputs(f, np.random.default_rng(41), False)
    args = (fv1, f["k1"], f["d1"], mp1, ur1, fv2, f["k2"], f["d2"], mp2, ur2, f["sf"], f["sigma2"], ep, F, False, False)

    def check(r):
        n, pairs, m12 = r
        on, om12 = oracle.search_for_triangulation(*args, True)
        assert on > 10 and n == on and np.array_equal(m12, om12)
        assert len(pairs) == n and np.array_equal(pairs[:, 1], om12[pairs[:, 0]])
    return (lambda: orbx.ORBmatcher(0.6, True).SearchForTriangulation(*args)), check


@case("orbx_search_for_triangulation_rig")
def _(oracle):
    import test_reloc_triangulation as T
    sc, kk, dd, nL, rig, fv, mp = T._rig_inputs(orbx, 3)
    s2 = sc["level_sigma2"]

    def check(r):
        n, m = r
        on, om, bl = oracle.search_for_triangulation_rig(fv, kk, dd, mp, nL, fv, kk, dd, mp, nL, s2, s2, rig.view(oracle.TRI_RIG_DTYPE),
                                                         False, False, True)
        diff = np.nonzero(m != om)[0]     # tolerance parity, as tests/test_reloc_triangulation.py holds it
        assert on > 15 and all(bl[i] for i in diff) and len(diff) <= 3
    return (lambda: orbx.ORBmatcher(0.6, True).SearchForTriangulationRig(fv, kk, dd, mp, nL, fv, kk, dd, mp, nL, s2, s2, rig, False, False)), check


def _pairs():
    import matcher_cases as mc
    pairs = mc.bin_pairs(mc.HISTOGRAMS["second_above_third_below"])     # a rotation histogram that culls
    k1, k2, d = mc.pair_frames(pairs)
    fv1, fv2 = mc.pair_feature_vectors(len(pairs))
    return k1, k2, d, fv1, fv2, np.ones(len(pairs), np.uint8)


@case("orbx_search_by_bow")
def _(oracle):
    k1, k2, d, fv1, fv2, valid = _pairs()

    def check(r):
        w = oracle.search_by_bow(fv1, d, k1["angle"], valid, fv2, d, k2["angle"], -1, 0.7, True)
        assert 0 < w[0] < len(k1) and r[0] == w[0] and np.array_equal(r[1], w[1])
    return (lambda: orbx.SearchByBoW(fv1, k1, d, valid, fv2, k2, d, -1, 0.7, True)), check


@case("orbx_search_by_bow_keyframes")
def _(oracle):
    k1, k2, d, fv1, fv2, valid = _pairs()

    def check(r):
        w = oracle.search_by_bow_keyframes(fv1, d, k1["angle"], valid, fv2, d, k2["angle"], valid, 0.75, True)
        assert 0 < w[0] < len(k1) and r[0] == w[0] and np.array_equal(r[1], w[1])
    return (lambda: orbx.SearchByBoWKeyFrames(fv1, k1, d, valid, fv2, k2, d, valid, 0.75, True)), check


@case("orbx_fisheye_stereo_match")
def _(oracle):
    import test_fisheye as tf
    g = np.load(tf.GOLDEN)
    kL = np.ascontiguousarray(g["kL"]).view(orbx.KP_DTYPE).reshape(-1)
    kR = np.ascontiguousarray(g["kR"]).view(orbx.KP_DTYPE).reshape(-1)

    def check(r):
        gold = (int(g["n"]), int(g["nd"]), g["l2r"], g["r2l"], g["depth"], g["p3d"])
        assert tf.compare_float_results(r, gold, g["gates"], int(g["mono_left"])) <= 2
    return (lambda: orbx.ComputeStereoFishEyeMatches(kL, g["dL"], int(g["mono_left"]), kR, g["dR"], int(g["mono_right"]), g["rig"],
                                                     g["level_sigma2"])), check


def _fisheye_projection(frame):
    def build(oracle):
        import test_fisheye as tf
        g, kps, mps, mpr, pts, bounds = tf._golden_proj(orbx)
        m = orbx.ORBmatcher(0.8, True)
        if frame:
            run = lambda: m.SearchByProjectionFrameFisheye(kps, g["desc"], int(g["n_left"]), bounds, pts, g["uvr"], g["occ"])
            want = (int(g["frame_n"]), g["frame_match"], g["frame_occ"])
        else:
            run = lambda: m.SearchByProjectionFisheye(kps, g["desc"], int(g["n_left"]), bounds, g["scale"], mps, mpr, g["l2r"], g["r2l"],
                                                      g["occ"], 3.0, True, 60.0)
            want = (int(g["map_n"]), g["map_match"], g["map_occ"])

        def check(r):
            assert r[0] == want[0] > 0 and np.array_equal(r[1], want[1]) and np.array_equal(r[2], want[2])
        return run, check
    return build


CASES["orbx_search_by_projection_fisheye"] = _fisheye_projection(False)
CASES["orbx_search_by_projection_frame_fisheye"] = _fisheye_projection(True)


@case("orbx_undistort_keypoints")
def _(oracle):
    import test_undistort as tu
    k = tu._kps(orbx, 1501, 640, 480, 3)

    def check(r):
        assert r.tobytes() == oracle.undistort_keypoints(k, tu.TUM_K, tu.TUM_D).tobytes()
    return (lambda: orbx.UndistortKeyPoints(k, tu.TUM_K, tu.TUM_D)), check


@case("orbx_bow_transform")
def _(oracle):
    import test_bow as tb
    from orb_slam3_fast_amd import synth
    cols = synth.make_vocabulary(5, 3, seed=8, early_leaf_prob=0.08, stop_prob=0.04)
    voc = orbx.ORBVocabulary(5, 3, *cols)      # (the vocabulary is a handle of its own: its tables are no scratch)
    feats = synth.vocabulary_features(cols, 300, seed=300)

    def check(r):
        tb._same_transform(r, oracle.Vocabulary(5, 3, *cols).transform(feats, 1))
    return (lambda: voc.transform(feats, 1)), check


# ------------------------------------------------------------------------------------------------ pre-processing one-shots
W, H, PAD, FILL = 203, 97, 13, 0xA5     # a width that is no multiple of 16, rows 13 bytes longer than their pixels


def _pitched(h, w, cn, rng=None):
    """An h x w x cn image inside rows of w * cn + PAD bytes; the padding holds FILL."""
    buf = np.full((h, w * cn + PAD), FILL, np.uint8)
    img = buf[:, :w * cn].reshape(h, w, cn) if cn > 1 else buf[:, :w * cn]
    if rng is not None:
        img[...] = rng.integers(0, 256, img.shape, dtype=np.uint8)
    return buf, img


def _preproc(call, dst_shape, want):
    """call(dst buffer) runs the entry into a pitched destination pre-filled with FILL; the whole buffer, padding included, is
    the result."""
    def run():
        buf, _ = _pitched(*dst_shape)
        orbx._check(call(buf))
        return buf

    def check(r):
        h, w, cn = dst_shape
        got = r[:, :w * cn].reshape(h, w, cn) if cn > 1 else r[:, :w]
        assert np.array_equal(got, want()) and (r[:, w * cn:] == FILL).all()
    return run, check


@case("orbx_cvt_gray")
def _(oracle):
    src, img = _pitched(H, W, 3, np.random.default_rng(1))
    L, p = orbx.lib(), orbx._p
    return _preproc(lambda d: L.orbx_cvt_gray(0, p(src), W, H, src.strides[0], 3, 1, p(d), d.strides[0]), (H, W, 1),
                    lambda: oracle.cvt_gray(np.ascontiguousarray(img), rgb=True))


@case("orbx_resize_linear")
def _(oracle):
    src, img = _pitched(H, W, 1, np.random.default_rng(2))
    dw, dh = 171, 83
    L, p = orbx.lib(), orbx._p
    return _preproc(lambda d: L.orbx_resize_linear(0, p(src), W, H, src.strides[0], 1, p(d), dw, dh, d.strides[0]), (dh, dw, 1),
                    lambda: oracle.resize(np.ascontiguousarray(img), dw, dh))


@case("orbx_remap_linear")
def _(oracle):
    import test_rectify_clahe as trc
    rng = np.random.default_rng(3)
    src, img = _pitched(H, W, 1, rng)
    dw, dh = 187, 91
    mx, my = trc._maps(rng, dw, dh, W, H, "rectify")
    mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
    L, p = orbx.lib(), orbx._p
    return _preproc(lambda d: L.orbx_remap_linear(0, p(src), W, H, src.strides[0], 1, p(mx), p(my), dw, p(d), dw, dh, d.strides[0]),
                    (dh, dw, 1), lambda: oracle.remap(np.ascontiguousarray(img), mx, my))


@case("orbx_clahe")
def _(oracle):
    src, img = _pitched(H, W, 1, np.random.default_rng(4))
    L, p = orbx.lib(), orbx._p
    return _preproc(lambda d: L.orbx_clahe(0, p(src), W, H, src.strides[0], 3.0, 8, 8, p(d), d.strides[0]), (H, W, 1),
                    lambda: oracle.clahe(np.ascontiguousarray(img), 3.0, (8, 8)))


# ------------------------------------------------------------------------------------------------ pose optimisation
@case("orbx_pose_optimization")
def _(oracle):
    import test_pose_opt as tp
    rng = np.random.default_rng(1100)
    kps, ur, X, hp, (q, t) = tp.scene(rng, 300, stereo=0.5, gross=0.1)
    q0, t0 = (v.astype(np.float32) for v in tp.perturb(rng, q, t))

    def check(r):
        assert r[3][hp != 0].any()                                  # outliers among the edges
        tp.compare(kps, ur, X, hp, q0, t0, label="scratch", got=r)
    return (lambda: orbx.PoseOptimization(kps, ur, X, hp, tp.level_tables(), q0, t0, tp.CAM)), check


@case("orbx_pose_optimization_batch")
def _(oracle):
    import test_pose_opt as tp
    rng = np.random.default_rng(1101)
    scs = [tp.scene(rng, n, stereo=0.0, gross=0.1) for n in (150, 60)]
    starts = [tuple(v.astype(np.float32) for v in tp.perturb(rng, *s[4])) for s in scs]
    frames = [scs[0], None, scs[1]]                                 # the middle image holds no keypoint
    ex = crafted_handle([(s[0], None) if s else (np.zeros(0, orbx.KP_DTYPE), None) for s in frames], 500)
    cap = ex.capacity
    wp, hp = np.zeros((3, cap, 3), np.float32), np.zeros((3, cap), np.uint8)
    q0, t0 = np.tile(np.array([0, 0, 0, 1], np.float32), (3, 1)), np.zeros((3, 3), np.float32)
    for f, k in ((0, 0), (2, 1)):
        n = len(scs[k][0])
        wp[f, :n], hp[f, :n], q0[f], t0[f] = scs[k][2], scs[k][3], starts[k][0], starts[k][1]
    sig = ex.GetInverseScaleSigmaSquares()

    def check(r):
        ng, qb, tb, ob, tr = r
        for f, k in ((0, 0), (2, 1)):                               # each frame has the one-shot entry's bits
            n = len(scs[k][0])
            g1, q1, t1, o1 = orbx.PoseOptimization(scs[k][0], None, wp[f, :n], hp[f, :n], sig, q0[f], t0[f], tp.CAM)
            assert g1 == ng[f] > 20 and same(q1, qb[f]) and same(t1, tb[f]) and np.array_equal(o1, ob[f, :n]) and not ob[f, n:].any()
            tp.compare(scs[k][0], None, wp[f, :n], hp[f, :n], q0[f], t0[f], sig=sig, label="scratch batch", got=(g1, q1, t1, o1))
        assert ng[1] == 0 and same(qb[1], q0[1]) and same(tb[1], t0[1]) and not ob[1].any()
    return (lambda: orbx.PoseOptimizationBatch(ex, 0, 3, wp, hp, q0, t0, tp.CAM, want_trials=True)), check


@case("orbx_pose_optimization_kb8")
def _(oracle):
    import test_pose_fisheye as tf
    rng = np.random.default_rng(1102)
    kps, X, hp, (q, t), rig = tf.scene(rng, 150, 150, gross=0.1)
    q0, t0 = (v.astype(np.float32) for v in tf.perturb(rng, q, t))

    def check(r):
        assert r[3][hp != 0].any()
        tf.compare(kps, 150, X, hp, q0, t0, rig, label="scratch", got=r)
    return (lambda: tf.run_gpu(kps, 150, X, hp, q0, t0, rig)), check


@case("orbx_pose_optimization_fisheye_batch")
def _(oracle):
    import test_pose_fisheye as tf
    rng = np.random.default_rng(1103)
    sizes = ((90, 70), (0, 0), (40, 30))                            # the middle rig frame holds no keypoint in either camera
    scs = [tf.scene(rng, nl, nr, gross=0.1) if nl else None for nl, nr in sizes]
    rig = scs[0][4]
    none = np.zeros(0, orbx.KP_DTYPE)
    ex = crafted_handle([(s[0][:nl] if s else none, None) for s, (nl, _) in zip(scs, sizes)] +
                        [(s[0][nl:] if s else none, None) for s, (nl, _) in zip(scs, sizes)], 500)
    n2 = 2 * ex.capacity
    wp, hp = np.zeros((3, n2, 3), np.float32), np.zeros((3, n2), np.uint8)
    q0, t0 = np.tile(np.array([0, 0, 0, 1], np.float32), (3, 1)), np.zeros((3, 3), np.float32)
    for f, s in enumerate(scs):
        if s:
            n = len(s[0])
            wp[f, :n], hp[f, :n] = s[1], s[2]
            q0[f], t0[f] = (v.astype(np.float32) for v in tf.perturb(rng, *s[3]))
    sig = ex.GetInverseScaleSigmaSquares()

    def check(r):
        ng, qb, tb, ob = r
        for f, s in enumerate(scs):
            if not s:
                assert ng[f] == 0 and same(qb[f], q0[f]) and same(tb[f], t0[f]) and not ob[f].any()
                continue
            n, nl = len(s[0]), sizes[f][0]
            one = tf.run_gpu(s[0], nl, wp[f, :n], hp[f, :n], q0[f], t0[f], rig, sig=sig)
            assert one[0] == ng[f] > 20 and same(one[1], qb[f]) and same(one[2], tb[f]) and np.array_equal(one[3], ob[f, :n])
            assert not ob[f, n:].any()
            tf.compare(s[0], nl, wp[f, :n], hp[f, :n], q0[f], t0[f], rig, sig=sig, label="scratch batch", got=one)
    return (lambda: orbx.PoseOptimizationFisheyeBatch(ex, 0, 3, 3, wp, hp, q0, t0, rig.k[0], rig.k[1], tf.TRL_Q, tf.TRL_T)), check


# ------------------------------------------------------------------------------------------------ two views, PnP, Sim3
@case("orbx_reconstruct_two_views")
def _(oracle):
    import test_two_view as tv
    name = "general_100"
    k1, k2, m, sets, ca, _, _ = tv.scene_inputs(name)

    def check(r):
        assert r[0]                                                  # initialised: every kernel of the chain ran
        tv.compare_with_model(name, k1, k2, m, sets, ca, r, tv.SCENES[name][0].get("planar", False), [])
    return (lambda: tv.gpu_call(k1, k2, m, sets, ca)), check


@case("orbx_reconstruct_two_views_batch")
def _(oracle):
    import test_two_view as tv
    ex, pairs = tv.batch_fixture(3)
    k1, k2, m, _ = tv.make_scene(131, n=7, extra=20)                # fewer than eight matches: the pair takes no area of the block
    orbx._check(orbx.lib().orbx_debug_upload_results(ex._h, 1, orbx._p(k2), orbx._p(np.zeros((len(k2), 32), np.uint8)), len(k2), len(k2)))
    pairs[1] = (k1, k2, m, np.zeros((200, 8), np.int32))

    def check(r):
        res, p3d, tri, sc = r
        for f, (k1, k2, m, sets) in enumerate(pairs):
            one = orbx.ReconstructWithTwoViews(k1, k2, m, tv.KMAT, sets, want_scores=True)
            assert same(one[5], res[f]) and same(one[3], p3d[f]) and np.array_equal(one[4], tri[f]) and same(one[6], sc[f]), f
        assert res[1]["n_matches"] == 7 and res[1]["model"] == -1 and not p3d[1].any() and not sc[1].any()
        assert res[0]["n_matches"] >= 8 and res[2]["n_matches"] >= 8
    return (lambda: orbx.ReconstructWithTwoViewsBatch(ex, 0, [p[0] for p in pairs], [p[2] for p in pairs], tv.KMAT,
                                                      sets=[p[3] for p in pairs], want_scores=True)), check


@case("orbx_mlpnp_iterate")
def _(oracle):
    import test_mlpnp as tm
    name = "pin640_out30"

    def check(r):
        an = tm.analysis(name)
        assert an["v1"]["ok"] and an["v1"]["hypothesis"] > 0         # hypotheses were rejected before the accepted one
        tm.compare_call(name, r, an["v1"], an["stable"], an["solver"])
    return (lambda: tm.device_iterate(name)), check


@case("orbx_mlpnp_iterate_batch")
def _(oracle):
    import test_mlpnp as tm
    names = ("pin640_out30", None, "pin640_n15")                    # different n, the middle image without a keypoint
    scs = [tm.scene(n) if n else None for n in names]
    ex = crafted_handle([(s["kps"], None) if s else (np.zeros(0, orbx.KP_DTYPE), None) for s in scs], 500)
    cap, sig = ex.capacity, ex.GetScaleSigmaSquares()
    wp, hp = np.zeros((3, cap, 3), np.float32), np.zeros((3, cap), np.uint8)
    prm, sets = np.zeros(3, orbx.MLPNP_PARAMS_DTYPE), np.zeros((3, tm.N_SETS, 6), np.int32)
    for p, (n, s) in enumerate(zip(names, scs)):
        if s is None:
            prm[p] = prm[0]
            continue
        a = tm.solver(n)
        k = len(s["kps"])
        assert s["n_left"] in (None, -1, k)
        wp[p, :k], hp[p, :k], sets[p] = s["wpos"], s["has"], s["sets"]
        prm[p] = orbx.mlpnp_params(s["cam"], a.minInliers, a.maxIts, 5)[0]

    def check(r):
        res, inl, st, bm, hyp = r
        for p, s in enumerate(scs):
            k = len(s["kps"]) if s else 0
            kk = s["kps"] if s else np.zeros(0, orbx.KP_DTYPE)
            o = orbx.MLPnPIterate(kk, wp[p, :k], hp[p, :k], sig, prm[p], sets[p], want_hyp=True)
            assert same(o[0], res[p]) and np.array_equal(o[1], inl[p, :k]) and not inl[p, k:].any(), p
            assert same(o[2], st[p:p + 1]) and np.array_equal(o[3], bm[p, :k]) and np.array_equal(o[4], hyp[p]), p
        assert res[1]["no_more"] == 1 and res[1]["n_correspondences"] == 0 and res[0]["ok"] == 1
    return (lambda: orbx.MLPnPIterateBatch(ex, np.arange(3, dtype=np.int32), wp, hp, prm, sets, want_hyp=True)), check


SIM3_SCENE = 3


@case("orbx_sim3_iterate")
def _(oracle):
    import test_sim3 as ts
    num = SIM3_SCENE

    def check(r):
        res, inl, st, bm, hyp = r
        h, an = ts.hypotheses(num), ts.analysis(num)
        a = h["solver"]
        run = int(res["iterations_run"])
        assert int(res["n_correspondences"]) == a.N and (hyp[run:] == -1).all() and (hyp[:run] >= 0).all()
        for j in range(min(run, h["K"])):    # hyp_inliers against V1's count, within the set's excluded decisions
            assert abs(int(hyp[j]) - an["counts"][j]) <= int(an["excluded"][j].sum()), j
        lp = ts.serial_loop(hyp, ts.MIN_INLIERS, a.maxIts, a.maxIts) if a.N >= ts.MIN_INLIERS else an["loop"]
        for k in ("converged", "no_more", "n_inliers", "iterations_run", "hypothesis"):
            assert int(res[k]) == lp[k], k
        assert lp["best_j"] >= 0 and run > 1
        ts.assert_pose_within_bound(res["R12"], res["t12"], res["s12"], ts.ref_pose(num, lp["best_j"]), "scratch scene %d" % num)
    return (lambda: ts.device_iterate(num)), check


@case("orbx_sim3_iterate_batch")
def _(oracle):
    import test_sim3 as ts
    nums = [4, 9]                                                   # and a problem without a key point in between
    a = ts.batch_args()
    idx = [list(ts.SCENES).index(k) for k in nums]
    pick = lambda x, fill: np.stack([x[idx[0]], np.full_like(x[0], fill), x[idx[1]]])
    n = np.array([a[0][idx[0]], 0, a[0][idx[1]]], np.int32)
    prm = np.stack([a[10][idx[0]], a[10][idx[0]], a[10][idx[1]]])
    args = (n, pick(a[1], 0), pick(a[2], 0), pick(a[3], np.nan), pick(a[4], np.nan), pick(a[5], 1), pick(a[6], -5), pick(a[7], 77), a[8],
            a[9], prm, pick(a[11], 0))

    def check(r):
        res, inl, st, bm, hyp = r
        for p, k in ((0, nums[0]), (2, nums[1])):
            o, m = ts.device_iterate(k), ts.scene(k)["n"]
            assert same(o[0], res[p]) and np.array_equal(o[1], inl[p, :m]) and not inl[p, m:].any(), k
            assert same(o[2], st[p:p + 1]) and np.array_equal(o[3], bm[p, :m]) and np.array_equal(o[4], hyp[p]), k
        assert res[1]["no_more"] == 1 and res[1]["n_correspondences"] == 0 and not inl[1].any() and (hyp[1] == -1).all()
    return (lambda: orbx.Sim3IterateBatch(*args, want_hyp=True)), check


def _sim3opt_scene():
    """The smallest scene of sim3opt_cases whose model clears matches (n_bad > 0) and rejects a trial."""
    import sim3opt_cases as sc
    ok = [n for n in sc.SCENES if sc.model(n, 0)["n_bad"] > 0 and not sc.model(n, 0)["early_return"]]
    return min(ok, key=lambda n: sc.SCENES[n]["N"])


@case("orbx_optimize_sim3")
def _(oracle):
    import test_optimize_sim3 as to
    num = _sim3opt_scene()
    return (lambda: to.device(num)), (lambda r: to.check_one_shot(num, r))


@case("orbx_optimize_sim3_batch")
def _(oracle):
    import test_optimize_sim3 as to
    b = to._batch_inputs([_sim3opt_scene(), 7, 8])                  # different n, an n = 0 problem in between, an early return

    def check(r):
        res, S, m = r
        h = b["hole"]
        assert res[h]["early_return"] == 1 and same(S[h], b["S"][h]) and same(m[h], b["m"][h])
        for p, s in zip(b["rows"], b["ss"]):
            one = to.device(s["num"])
            assert same(res[p], one[4]) and same(S[p], one[1]) and same(m[p, :s["n"]], one[2]) and same(m[p, s["n"]:], b["m"][p, s["n"]:])
    return (lambda: to._run_batch(b)), check


# ------------------------------------------------------------------------------------------------ inertial pose optimisation
def _pose_inertial(cls):
    def build(oracle):
        import pose_inertial_cases as pc
        import test_pose_inertial as tpi
        sc, last = pc.scene(cls, "mixed"), pc.is_last_frame(cls)

        def check(r):
            assert r["outlier"][np.asarray(sc["has_point"]) != 0].any()
            tpi.check_against_model(r, pc.model(cls, "mixed", 1), pc.spreads(cls), "scratch %s/mixed" % cls)
        return (lambda: tpi.run_device(sc, last)), check
    return build


CASES["orbx_pose_inertial_optimization_last_keyframe"] = _pose_inertial("kf_outliers")
CASES["orbx_pose_inertial_optimization_last_frame"] = _pose_inertial("lf_outliers")


def _pose_inertial_batch(last):
    def build(oracle):
        import test_pose_inertial as tpi
        call, single, ns = tpi.batch_of_three(last)
        return call, (lambda r: tpi.check_batch_of_three(last, r[0], r[1], single, ns))
    return build


CASES["orbx_pose_inertial_optimization_last_keyframe_batch"] = _pose_inertial_batch(False)
CASES["orbx_pose_inertial_optimization_last_frame_batch"] = _pose_inertial_batch(True)


def _pose_inertial_spill(last):
    """4200 edges: above the 4096 the kernel stages in LDS, so they are staged in the call's device block.  Bitwise agreement only
    (tests/test_pose_inertial.py::test_frame_above_the_lds_staging_cap runs the float64 model of this scene)."""
    def build(oracle):
        import pose_inertial_cases as pc
        import test_pose_inertial as tpi
        seq = pc.make_sequence(9001, "mixed", n_frames=2, n_kp=4300, n_points=4200, outlier_frac=0.1)
        return (lambda: tpi.run_device(seq[1 if last else 0], last)), None
    return build


CASES["orbx_pose_inertial_optimization_last_keyframe:device_staging"] = _pose_inertial_spill(False)
CASES["orbx_pose_inertial_optimization_last_frame:device_staging"] = _pose_inertial_spill(True)


# ------------------------------------------------------------------------------------------------ bundle adjustments, pose graph
# (the wrappers return a dict of every output array and every field of the result record)
@case("orbx_local_bundle_adjustment")
def _(oracle):
    import test_local_ba as t
    name = "outliers_257"                                           # erased edges of both kinds, rejected trials, then accepted ones

    def check(r):
        assert r["erase"].any() and r["trials"] > r["iterations"]
        t.against_v1(name, d=r)
    return (lambda: t.device(name)), check


@case("orbx_local_bundle_adjustment_rig")
def _(oracle):
    import lba_rig_cases as rc
    import test_local_ba_rig as t
    name = "rig_far_start"

    def check(r):
        assert r["erase"].any() and r["trials"] > r["iterations"]
        t.against_v1(name, d=r)
    return (lambda: t.call(rc.scene(name))), check


@case("orbx_bundle_adjustment")
def _(oracle):
    import test_global_ba as t
    name = "far_start"                                              # robust, trials rejected with a margin

    def check(r):
        assert r["trials"] > r["iterations"]
        t.against_v1(name, orbx.BA_SOLVER_BLOCKED, d=r)
    return (lambda: t.device(name, solver=orbx.BA_SOLVER_BLOCKED)), check


@case("orbx_bundle_adjustment:past_128_keyframes")
def _(oracle):
    import gba_cases as gc
    import test_global_ba as t
    name = "cap_130_robust"                                         # 130 key frames to optimise: the blocked solver's path, S in the block
    assert gc.graph(gc.scene(name), True)["nOpt"] > orbx.LBA_MAX_LOCAL
    return (lambda: t.device(name, solver=orbx.BA_SOLVER_AUTO)), (lambda r: t.against_v1(name, orbx.BA_SOLVER_AUTO, d=r))


@case("orbx_bundle_adjustment_rig")
def _(oracle):
    import test_global_ba_rig as t
    name = "rig_kb8_robust"
    return (lambda: t.call(t.scene(name), solver=orbx.BA_SOLVER_AUTO)), (lambda r: t.against_v1(name, orbx.BA_SOLVER_AUTO, d=r))


def _merge(name):
    def build(oracle):
        import test_merge_ba as t

        def check(r):
            assert r["erase"].any() and r["n_level1"] > 0          # edges erased, and edges set aside after round one
            t.against_v1(name, d=r)
        return (lambda: t.device(name)), check
    return build


CASES["orbx_merge_bundle_adjustment"] = _merge("gross")
CASES["orbx_merge_bundle_adjustment_rig"] = _merge("kb8")


@case("orbx_optimize_pose_graph")
def _(oracle):
    import essential_graph_cases as eg
    import test_essential_graph as t
    name = "pair_a"
    p = eg.scenes()[name][0]
    X = np.random.default_rng(2).normal(size=(5, 3)).astype(np.float32)
    ref = np.array([1, -1, 2, 0, 1], np.int32)                      # a point without a reference key frame: not written

    def check(r):
        m = eg.model(name, 0)
        assert m["trials"] > m["iterations"]                         # a rejected trial
        t.check_against_model(name, p, r, m, "pair", [])
        t.check_counters(name, r, m)
        assert same(r["points"][1], X[1])
    return (lambda: t.run(p, points=X, ref=ref)), check


@case("orbx_optimize_pose_graph:chain")
def _(oracle):
    """A chain of nine vertices behind a fixed one: 63 rows, past the solver's 48-column block, and a block-tridiagonal system --
    most blocks of the dense S belong to no edge and hold what the clear in front of the scatter left there."""
    import essential_graph_cases as eg
    import test_essential_graph as t
    name = "chain_9"
    p = eg.scenes()[name][0]

    def check(r):
        m = eg.model(name, 0)
        t.check_against_model(name, p, r, m, "chain", [])
        t.check_counters(name, r, m)
        assert m["trials"] >= 1 and not same(r["vertices"][1], p["vertices"][1])          # the trial was accepted
    return (lambda: t.run(p, 1)), check


@case("orbx_pose_graph_evaluate")
def _(oracle):
    import essential_graph_cases as eg
    import test_essential_graph as t
    p, xs = t.branch_edges()

    def check(r):
        err, jac = r
        G = eg.graph(p)
        est = [eg.to_tuple(v) for v in p["vertices"]]
        for e in range(len(xs)):
            a = (G["C"][e], est[G["i"][e]], est[G["j"][e]])
            bound = t.evaluation_bound(*a)
            assert (np.abs(err[e] - eg.edge_error(*a)) <= bound).all(), e
            free = (p["fixed"][G["i"][e]] == 0, p["fixed"][G["j"][e]] == 0)
            J = eg.edge_jacobians(*a, free[0], free[1], False, 1e-6)
            for side in (0, 1):
                if free[side]:
                    assert (np.abs(jac[e, side] - J[side]) <= bound[:, None] / 1e-6).all(), (e, side)
                else:
                    assert not jac[e, side].any()
    return (lambda: orbx.pose_graph_evaluate(p["vertices"], p["fixed"], p["edges"], False)), check


# ------------------------------------------------------------------------------------------------ new map points
@case("orbx_triangulate_matches")
def _(oracle):
    import test_new_map_points as nmp
    name = "stereo"
    s = nmp.scene(name)

    def check(r):
        nc, st, x3d, ps = r
        r64 = nmp.reference(name)[1]
        cmp, hist = nmp.compare_decisions(st, r64, "scratch " + name)
        assert nc == int((st == 0).sum()) > 0 and (hist[1:] > 0).sum() >= 3      # created points and several kinds of rejection
        for i in np.nonzero(cmp)[0]:
            q = r64[i]
            if q["status"] not in (1, 2):
                assert bool(ps[i]) == q["ps"], i
            if q["status"] == 0 and st[i] == 0:
                Xr = np.array(q["X"], float)
                assert float(np.linalg.norm(x3d[i].astype(float) - Xr)) <= nmp.point_bound(Xr), i
    return (lambda: nmp.device_pair(s)), check


@case("orbx_create_new_map_points")
def _(oracle):
    import test_new_map_points as nmp
    ch = nmp.chain_scene(21, 300, 3, stereo=False)

    def check(r):
        assert r["n_created"][0] >= 40
        nmp.assert_chain_equals_sequence(ch, "scratch chain", out=r)
    return (lambda: nmp.device_chain(ch)), check


# ------------------------------------------------------------------------------------------------ further one-shot entries
@case("orbx_compute_image_bounds")
def _(oracle):
    import test_undistort as tu

    def check(r):
        assert same(r, np.asarray(oracle.image_bounds(640, 480, tu.TUM_K, tu.TUM_D), np.float32))
    return (lambda: orbx.ComputeImageBounds(640, 480, tu.TUM_K, tu.TUM_D)), check


def _dense_solve(entry, n):
    """The two dense LDLT solvers alone, at a size of several passes: the bound of their own tests (4 x the numpy LDLT's relative
    residual on the same matrix, plus one ulp)."""
    def build(oracle):
        import lba_cases as lc
        from test_global_ba import spd
        from test_local_ba import residual, EPS
        A, b = spd(n)

        def check(r):
            assert r["ok"] == 1 and residual(A, r["x"], b) <= 4 * residual(A, lc.ldlt_dense(A, b), b) + EPS
        return (lambda: entry(A, b)), check
    return build


CASES["orbx_lba_dense_solve"] = _dense_solve(orbx.lba_dense_solve, 210)
CASES["orbx_ba_dense_solve"] = _dense_solve(orbx.ba_dense_solve, 3 * 48 + 18)
