"""RGB-D frames: Frame::ComputeStereoFromRGBD (src/Frame.cc:1086-1104) with Tracking::GrabImageRGBD's depth conversion
(src/Tracking.cc:1490-1547) -- orbx_rgbd_depth_batch (device, batched) and orbx_extract_rgbd (one frame, host lookup).

The oracle supplies keypoints, descriptors and undistort_keypoints; the depth rule is plain IEEE single precision and is
modelled here with numpy float32.  Every comparison is on raw bits."""
import ctypes as C

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

ZED2_K = np.array([532.03125, 532.03125, 639.888671875, 356.16241455078125], np.float32)
ZED2_BF = np.float32(0.12) * np.float32(532.03125)
TUM1_K = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)
TUM1_DIST = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)   # k1 k2 p1 p2 k3
TUM1_BF = np.float32(0.07732) * np.float32(517.306408)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model(kps, x_un, depth, depth_scale, bf):
    """numpy float32 restatement of the reference: (mvuRight, mvDepth) of keypoints kps (distorted points) read from the RAW
    depth image with GrabImageRGBD's conversion; points whose truncated coordinates leave the image give -1."""
    h, w = depth.shape
    x = np.asarray(kps["x"], np.float32)
    y = np.asarray(kps["y"], np.float32)
    n = len(x)
    ur = np.full(n, -1, np.float32)
    dp = np.full(n, -1, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (x > -1) & (x < w) & (y > -1) & (y < h)
    u = np.trunc(x[ok]).astype(np.int64)
    v = np.trunc(y[ok]).astype(np.int64)
    raw = depth[v, u].astype(np.float32)
    s = np.float32(depth_scale)
    scales = float(abs(np.float32(s - np.float32(1.0)))) > 1e-5 or depth.dtype != np.float32
    with np.errstate(all="ignore"):
        d = (raw * s).astype(np.float32) if scales else raw
        pos = d > 0
        r = np.full(len(d), -1, np.float32)
        dd = np.full(len(d), -1, np.float32)
        dd[pos] = d[pos]
        r[pos] = np.asarray(x_un, np.float32)[ok][pos] - np.float32(bf) / d[pos]
    ur[ok] = r
    dp[ok] = dd
    return ur, dp


def depth_u16(w, h, seed):
    """Millimetre depth with smooth variation, holes (0) and saturated 65535 patches."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 800 + 3000 * (0.5 + 0.5 * np.sin(xx / 97.0 + seed) * np.cos(yy / 61.0)) + rng.integers(0, 40, (h, w))
    d = d.astype(np.uint16)
    for _ in range(12):
        x0, y0 = rng.integers(0, w - 80), rng.integers(0, h - 60)
        d[y0:y0 + rng.integers(10, 60), x0:x0 + rng.integers(10, 80)] = 0
    for _ in range(6):
        x0, y0 = rng.integers(0, w - 80), rng.integers(0, h - 60)
        d[y0:y0 + rng.integers(10, 60), x0:x0 + rng.integers(10, 80)] = 65535
    d[rng.random((h, w)) < 0.02] = 0
    return d


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("factor", [0.0, 1e-6, 1.0, 1000.0, 5000.0])
def test_depth_scale_from_settings(factor):
    s = orbx.depth_scale_from_settings(factor)
    assert isinstance(s, np.float32)
    f = np.float32(factor)
    want = np.float32(1.0) if abs(float(f)) < 1e-5 else np.float32(np.float32(1.0) / f)
    assert s.tobytes() == want.tobytes()
    if factor == 1000.0:
        assert s.tobytes() == (np.float32(1) / np.float32(1000)).tobytes()


def test_rgbd_entries_fail_loudly_without_a_handle_or_gpu():
    L = orbx.lib()
    K = ZED2_K.ctypes.data_as(C.c_void_p)
    rc = L.orbx_rgbd_depth_batch(None, 0, 1, None, orbx.DEPTH_U16, 2560, 2560 * 720, 0.001, 63.8, K, None, 0, None)
    assert rc == -2   # ORBX_E_BADARG: null handle
    n, mono = C.c_int(), C.c_int()
    img = np.zeros((48, 64), np.uint8)
    dep = np.zeros((48, 64), np.uint16)
    rc = L.orbx_extract_rgbd(None, img.ctypes.data, 64, 48, 64, dep.ctypes.data, orbx.DEPTH_U16, 128, 0.001, 63.8, K, None, 0,
                             None, None, 0, C.byref(n), C.byref(mono), None, None, None)
    assert rc == -2

    class _Null:
        _h = None
        capacity = 16
    with pytest.raises(orbx.OrbxError) as e:
        orbx.ComputeStereoFromRGBD(_Null(), 0, orbx.DEPTH_U16, 128, 128 * 48, 63.8, 0.001)
    assert e.value.code == -2
    with pytest.raises(orbx.OrbxError):
        orbx.rgbd_depth_async(_Null(), 0, orbx.DEPTH_F32, 256, 256 * 48, 63.8, 1.0)
    if orbx.device_count() == 0:
        with pytest.raises(orbx.OrbxError) as e:
            orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
        assert "device" in str(e.value).lower() or "hip" in str(e.value).lower()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev():
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    return DeviceBuffer


def _frames(w, h, n, stream0):
    return np.stack([synth.mono_frame(w, h, stream0 + f, 0) for f in range(n)])


@pytest.mark.gpu
def test_zed2_batched_u16(oracle):
    """ZED2 RGB-D setup: 16 frames of 1280x720, 1250 features, uint16 millimetres with holes and 65535 patches."""
    DeviceBuffer = _dev()
    w, h, nf, F = 1280, 720, 1250, 16
    imgs = _frames(w, h, F, 300)
    deps = np.stack([depth_u16(w, h, f) for f in range(F)])
    dimg, ddep = DeviceBuffer.from_numpy(imgs), DeviceBuffer.from_numpy(deps)
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    cap = ex.capacity
    dkun = DeviceBuffer(F * cap * 28)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    scale = orbx.depth_scale_from_settings(1000.0)
    u, d = orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, ZED2_BF, scale, K=ZED2_K,
                                      dist=np.zeros(5, np.float32), n_frames=F, d_kps_un_ptr=dkun.ptr.value)
    counts = np.zeros(F, np.int32)
    ua = np.zeros((F, cap), np.float32)
    da = np.zeros((F, cap), np.float32)
    ex.download_async(counts.ctypes.data, None, None, None, ua.ctypes.data, da.ctypes.data, F)
    ex.sync()
    kun = dkun.to_numpy(orbx.KP_DTYPE, (F, cap))
    valid = sat = 0
    for f in range(F):
        mono, kps, desc = ex.download(f)
        om, ok, od = oracle.OracleExtractor(nf).extract(imgs[f])
        assert mono == om and kps.tobytes() == ok.tobytes() and np.array_equal(desc, od), f
        n = len(kps)
        assert counts[f] == n
        assert kun[f, :n].tobytes() == kps.tobytes()            # no distortion: mvKeysUn = mvKeys
        mu, md = model(kps, kps["x"], deps[f], scale, ZED2_BF)
        assert np.array_equal(bits(u[f, :n]), bits(mu)) and np.array_equal(bits(d[f, :n]), bits(md)), f
        assert np.array_equal(bits(ua[f, :n]), bits(mu)) and np.array_equal(bits(da[f, :n]), bits(md)), f
        valid += int((md > 0).sum())
        sat += int((md == np.float32(65535) * scale).sum())
        assert (md == -1).sum() > 0
    assert valid > 0.8 * F * 1000 and sat > 0


@pytest.mark.gpu
def test_tum1_batched_with_distortion(oracle):
    """TUM1: 640x480, factor 5000, five coefficients.  mvKeysUn = oracle.undistort_keypoints; the depth is read at the
    DISTORTED point and uRight uses the undistorted x."""
    DeviceBuffer = _dev()
    w, h, nf, F = 640, 480, 1000, 4
    imgs = _frames(w, h, F, 410)
    deps = np.stack([(depth_u16(w, h, 40 + f).astype(np.uint32) * 5 // 2).clip(0, 65535).astype(np.uint16) for f in range(F)])
    dimg, ddep = DeviceBuffer.from_numpy(imgs), DeviceBuffer.from_numpy(deps)
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    cap = ex.capacity
    dkun = DeviceBuffer(F * cap * 28)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    scale = orbx.depth_scale_from_settings(5000.0)
    u, d = orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, TUM1_BF, scale, K=TUM1_K,
                                      dist=TUM1_DIST, n_frames=F, d_kps_un_ptr=dkun.ptr.value)
    kun = dkun.to_numpy(orbx.KP_DTYPE, (F, cap))
    for f in range(F):
        _, kps, _ = ex.download(f)
        n = len(kps)
        okun = oracle.undistort_keypoints(kps, TUM1_K, TUM1_DIST)
        assert kun[f, :n].tobytes() == okun.tobytes(), f
        assert not np.array_equal(okun["x"], kps["x"])
        mu, md = model(kps, okun["x"], deps[f], scale, TUM1_BF)
        assert np.array_equal(bits(u[f, :n]), bits(mu)) and np.array_equal(bits(d[f, :n]), bits(md)), f
        # the distorted x would give other uRight values
        wrong, _ = model(kps, kps["x"], deps[f], scale, TUM1_BF)
        assert not np.array_equal(bits(wrong), bits(mu))


def _edge_depth(w, h, kps, seed):
    rng = np.random.default_rng(seed)
    dep = rng.uniform(0.3, 9.0, (h, w)).astype(np.float32)
    edges = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-40, 1.4e-45, 1e-38, 3e38, 1.0, 2.5e-3], np.float32)
    u = np.trunc(kps["x"]).astype(np.int64)
    v = np.trunc(kps["y"]).astype(np.int64)
    dep[v, u] = edges[np.arange(len(kps)) % len(edges)]
    return dep


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.000004, 0.5, 1e-3])
def test_f32_depth_edges(scale):
    """NaN, +-inf, +-0, negatives, denormals and a tiny d whose bf / d overflows; the skip rule at 1.000004f."""
    DeviceBuffer = _dev()
    w, h, nf = 640, 480, 1000
    img = synth.mono_frame(w, h, 7, 0)
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    ex.extract_batch_device(DeviceBuffer.from_numpy(img).ptr.value, 1, w, h, w, w * h)
    _, kps, _ = ex.download(0)
    dep = _edge_depth(w, h, kps, 3)
    dd = DeviceBuffer.from_numpy(dep)
    s = np.float32(scale)
    u, d = orbx.ComputeStereoFromRGBD(ex, dd.ptr.value, orbx.DEPTH_F32, 4 * w, 4 * w * h, TUM1_BF, s)
    n = len(kps)
    mu, md = model(kps, kps["x"], dep, s, TUM1_BF)
    assert np.array_equal(bits(u[0, :n]), bits(mu)) and np.array_equal(bits(d[0, :n]), bits(md))
    if scale == 1.000004:   # |1.000004f - 1| <= 1e-5: the values are used unscaled
        i = np.flatnonzero(md > 0)
        assert np.array_equal(bits(md[i]), bits(dep[np.trunc(kps["y"][i]).astype(int), np.trunc(kps["x"][i]).astype(int)]))
    if scale == 1.0:
        assert np.isneginf(mu).any()                            # tiny positive d: bf / d overflows
        assert (mu == kps["x"]).any()                           # d = +inf: uRight = x
    # the float row pitch can be wider than the image
    pad = np.zeros((h, w + 24), np.float32)
    pad[:, :w] = dep
    u2, d2 = orbx.ComputeStereoFromRGBD(ex, DeviceBuffer.from_numpy(pad).ptr.value, orbx.DEPTH_F32, 4 * (w + 24), 0, TUM1_BF, s)
    assert np.array_equal(bits(u2[0, :n]), bits(mu)) and np.array_equal(bits(d2[0, :n]), bits(md))


def _upload(ex, image, kps):
    desc = np.zeros((len(kps), 32), np.uint8)
    k = np.ascontiguousarray(kps, orbx.KP_DTYPE)
    assert orbx.lib().orbx_debug_upload_results(ex._h, image, k.ctypes.data, desc.ctypes.data, len(k), 0) == 0


@pytest.mark.gpu
def test_crafted_keypoint_coordinates():
    """Fractional points, x in (-1, 0) (column 0, as the reference reads it), x = w - 0.001, x = w, y = h, NaN."""
    DeviceBuffer = _dev()
    w, h = 640, 480
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h)
    ex.extract_batch_device(DeviceBuffer.from_numpy(synth.mono_frame(w, h, 1, 0)).ptr.value, 1, w, h, w, w * h)
    xy = [(10.5, 20.25), (-0.5, 3.0), (-0.999, 479.9), (w - 0.001, 100.0), (w, 100.0), (100.0, h), (100.0, h - 0.001),
          (np.nan, 5.0), (5.0, np.nan), (-1.0, 5.0), (-1.0001, 5.0), (5.0, -0.25), (1e30, 5.0), (-1e30, 5.0), (np.inf, 1.0),
          (639.0, 479.0), (0.0, 0.0), (320.75, 240.5)]
    kps = np.zeros(len(xy), orbx.KP_DTYPE)
    kps["x"] = [p[0] for p in xy]
    kps["y"] = [p[1] for p in xy]
    kps["size"], kps["angle"], kps["octave"] = 31.0, 12.5, 1
    _upload(ex, 0, kps)
    rng = np.random.default_rng(5)
    for dt in (np.uint16, np.float32):
        dep = rng.integers(1, 9000, (h, w)).astype(dt)
        dd = DeviceBuffer.from_numpy(dep)
        es = dep.itemsize
        dkun = DeviceBuffer(ex.capacity * 28)
        u, d = orbx.ComputeStereoFromRGBD(ex, dd.ptr.value, orbx.DEPTH_U16 if dt == np.uint16 else orbx.DEPTH_F32, es * w,
                                          es * w * h, 40.0, 1e-3, d_kps_un_ptr=dkun.ptr.value)
        mu, md = model(kps, kps["x"], dep, np.float32(1e-3), 40.0)
        n = len(kps)
        assert np.array_equal(bits(u[0, :n]), bits(mu)) and np.array_equal(bits(d[0, :n]), bits(md))
        assert md[1] > 0 and md[2] > 0 and md[3] > 0 and (md[[4, 5, 7, 8, 9, 10, 12, 13, 14]] == -1).all()
        assert md[1] == np.float32(dep[3, 0]) * np.float32(1e-3)
        assert dkun.to_numpy(orbx.KP_DTYPE, ex.capacity)[:n].tobytes() == kps.tobytes()


@pytest.mark.gpu
def test_first_image_subrange_untouched_rows_and_invalidation():
    DeviceBuffer = _dev()
    w, h, F = 640, 480, 6
    imgs = _frames(w, h, F, 500)
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg = DeviceBuffer.from_numpy(imgs)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    deps = np.stack([depth_u16(w, h, 70 + f) for f in range(3)])
    ddep = DeviceBuffer.from_numpy(deps)
    scale = orbx.depth_scale_from_settings(1000.0)
    u, d = orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, 40.0, scale, first_image=2, n_frames=3)
    for f in range(3):
        _, kps, _ = ex.download(2 + f)
        n = len(kps)
        mu, md = model(kps, kps["x"], deps[f], scale, 40.0)
        assert np.array_equal(bits(u[f, :n]), bits(mu)) and np.array_equal(bits(d[f, :n]), bits(md)), f
    with pytest.raises(orbx.OrbxError):   # pair 3 was not produced
        orbx._check(orbx.lib().orbx_stereo_download(ex._h, 3, None, None, 0))
    # rows past a frame's keypoint count are left as they were, as the stereo association leaves them
    _, kps, desc = ex.download(2)
    n = len(kps)
    keep = n - 100
    k = np.ascontiguousarray(kps[:keep])
    assert orbx.lib().orbx_debug_upload_results(ex._h, 2, k.ctypes.data, np.ascontiguousarray(desc[:keep]).ctypes.data, keep, 0) == 0
    deps2 = deps.copy()
    deps2[0] = 1234
    u2, d2 = orbx.ComputeStereoFromRGBD(ex, DeviceBuffer.from_numpy(deps2).ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, 40.0, scale,
                                        first_image=2, n_frames=3)
    assert np.array_equal(bits(u2[0, keep:n]), bits(u[0, keep:n])) and np.array_equal(bits(d2[0, keep:n]), bits(d[0, keep:n]))
    assert (d2[0, :keep] == np.float32(1234) * scale).all()
    # the next extraction invalidates the results
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    ex.sync()
    with pytest.raises(orbx.OrbxError):
        orbx._check(orbx.lib().orbx_stereo_download(ex._h, 0, None, None, 0))
    with pytest.raises(orbx.OrbxError):
        ex.download_async(None, None, None, None, None, None, 1)
    # argument checks
    for bad in [dict(first_image=5, n_frames=2), dict(first_image=-1), dict(n_frames=0)]:
        with pytest.raises(orbx.OrbxError):
            orbx.rgbd_depth_async(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, 40.0, scale, **bad)
    with pytest.raises(orbx.OrbxError) as e:
        orbx.rgbd_depth_async(ex, ddep.ptr.value, 3, 2 * w, 2 * w * h, 40.0, scale)
    assert e.value.code == -6   # ORBX_E_UNSUPPORTED
    with pytest.raises(orbx.OrbxError):
        orbx.rgbd_depth_async(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w - 2, 2 * w * h, 40.0, scale)
    with pytest.raises(orbx.OrbxError):   # distortion without K
        orbx.rgbd_depth_async(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, 40.0, scale, dist=TUM1_DIST)


@pytest.mark.gpu
def test_rgbd_stereo_rgbd_on_one_handle():
    """RGB-D(32), stereo(16), RGB-D(32): the RGB-D growth of the result arrays must not hide the association's own buffers."""
    DeviceBuffer = _dev()
    w, h, nf = 640, 480, 1000
    pairs = [synth.stereo_pair(w, h, 600 + p, 0) for p in range(16)]
    imgs = np.stack([p[0] for p in pairs] + [p[1] for p in pairs])
    deps = np.stack([depth_u16(w, h, 90 + f) for f in range(32)])
    dimg, ddep = DeviceBuffer.from_numpy(imgs), DeviceBuffer.from_numpy(deps)
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=32)
    ref = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=32)
    scale = orbx.depth_scale_from_settings(1000.0)
    kps = []

    def rgbd_check():
        u, d = orbx.ComputeStereoFromRGBD(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, 50.0, scale, n_frames=32)
        for f in range(32):
            n = len(kps[f])
            mu, md = model(kps[f], kps[f]["x"], deps[f], scale, 50.0)
            assert np.array_equal(bits(u[f, :n]), bits(mu)) and np.array_equal(bits(d[f, :n]), bits(md)), f

    ex.extract_batch_device(dimg.ptr.value, 32, w, h, w, w * h)
    ref.extract_batch_device(dimg.ptr.value, 32, w, h, w, w * h)
    kps.extend(ex.download(f)[1] for f in range(32))
    rgbd_check()
    bf, b = np.float32(0.12) * np.float32(532.03), 0.12
    us, ds = orbx.ComputeStereoMatches(ex, ex, bf, b, first_left=0, first_right=16, n_pairs=16)
    ur, dr = orbx.ComputeStereoMatches(ref, ref, bf, b, first_left=0, first_right=16, n_pairs=16)
    for p in range(16):
        n = len(kps[p])
        assert np.array_equal(bits(us[p, :n]), bits(ur[p, :n])) and np.array_equal(bits(ds[p, :n]), bits(dr[p, :n])), p
    assert (ds[:, :100] > 0).sum() > 100
    rgbd_check()
    us, ds = orbx.ComputeStereoMatches(ex, ex, bf, b, first_left=0, first_right=16, n_pairs=16)
    for p in range(16):
        n = len(kps[p])
        assert np.array_equal(bits(us[p, :n]), bits(ur[p, :n])) and np.array_equal(bits(ds[p, :n]), bits(dr[p, :n])), p


@pytest.mark.gpu
def test_batched_matchers_on_rgbd_results(oracle):
    """SearchByProjection(Frame)Batch with stereo_pair0 = 0 read the RGB-D results like the association's."""
    DeviceBuffer = _dev()
    w, h, nf, F = 640, 480, 1000, 4
    imgs = _frames(w, h, F, 700)
    deps = np.stack([depth_u16(w, h, 110 + f) for f in range(F)])
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=F)
    dimg, ddep = DeviceBuffer.from_numpy(imgs), DeviceBuffer.from_numpy(deps)
    ex.extract_batch_device(dimg.ptr.value, F, w, h, w, w * h)
    scale = orbx.depth_scale_from_settings(1000.0)
    bf = np.float32(40.0)
    orbx.rgbd_depth_async(ex, ddep.ptr.value, orbx.DEPTH_U16, 2 * w, 2 * w * h, bf, scale, n_frames=F)
    ex.sync()
    cap, sf = ex.capacity, ex.GetScaleFactors()
    rng = np.random.default_rng(31)
    stride = nf + 40
    pts = np.zeros((F, stride), orbx.PP_DTYPE)
    mps = np.zeros((F, stride), orbx.MP_DTYPE)
    npts = np.zeros(F, np.int32)
    occ_in = (rng.random((F, cap)) < 0.05).astype(np.uint8)
    frames = []
    for f in range(F):
        _, kc, dc = ex.download(f)
        n = len(kc) - 13 * f
        npts[f] = n
        octv = kc["octave"][:n]
        p = pts[f, :n]
        p["u"] = kc["x"][:n] + rng.normal(0, 1.5, n)
        p["v"] = kc["y"][:n] + rng.normal(0, 1.5, n)
        mu, _ = model(kc, kc["x"], deps[f], scale, bf)
        p["ur"] = np.where(mu[:n] >= 0, mu[:n], p["u"] - 20) + rng.normal(0, 1.0, n).astype(np.float32)
        p["angle"] = kc["angle"][:n]
        p["valid"] = rng.random(n) < 0.9
        p["has_observations"] = rng.random(n) < 0.8
        p["radius"] = (np.float32(15.0) * sf[octv]).astype(np.float32)
        p["min_level"], p["max_level"] = octv - 1, octv + 1
        p["desc"] = dc[:n] ^ np.packbits(rng.random((n, 32, 8)) < 0.04, axis=2).reshape(n, 32)
        m = mps[f, :n]
        m["proj_x"], m["proj_y"], m["proj_xr"] = p["u"], p["v"], p["ur"]
        m["view_cos"] = rng.choice([0.9, 0.9985, 0.998], n).astype(np.float32)
        m["track_depth"] = rng.uniform(1, 80, n).astype(np.float32)
        m["predicted_level"] = np.clip(octv + rng.integers(-1, 2, n), 0, 7)
        m["in_view"] = rng.random(n) < 0.9
        m["bad"] = rng.random(n) < 0.05
        m["has_observations"] = rng.random(n) < 0.85
        m["desc"] = p["desc"]
        frames.append((kc, dc, mu))
    bounds = (0.0, 0.0, float(w), float(h))
    nm, match, occ = orbx.ORBmatcher(0.9, True).SearchByProjectionFrameBatch(ex, 0, F, bounds, pts, npts, occ_in, stereo_pair0=0)
    for f in range(F):
        kc, dc, mu = frames[f]
        onm, omatch, oocc = oracle.search_by_projection_frame(kc, dc, mu, bounds, pts[f, :npts[f]], True, occ_in[f, :len(kc)])
        assert nm[f] == onm and np.array_equal(match[f, :len(kc)], omatch) and np.array_equal(occ[f, :len(kc)], oocc), f
        one = orbx.ORBmatcher(0.9, True).SearchByProjectionFrame(kc, dc, mu, bounds, pts[f, :npts[f]], occ_in[f, :len(kc)])
        assert nm[f] == one[0] and np.array_equal(match[f, :len(kc)], one[1])
    assert nm.sum() > 100 * F
    nm, match, occ = orbx.ORBmatcher(0.8, True).SearchByProjectionBatch(ex, 0, F, bounds, mps, npts, occ_in, 3.0, True, 40.0,
                                                                        stereo_pair0=0)
    for f in range(F):
        kc, dc, mu = frames[f]
        onm, omatch, oocc = oracle.search_by_projection(kc, dc, mu, bounds, sf, mps[f, :npts[f]], 3.0, True, 40.0, 0.8,
                                                        occ_in[f, :len(kc)])
        assert nm[f] == onm and np.array_equal(match[f, :len(kc)], omatch) and np.array_equal(occ[f, :len(kc)], oocc), f
    assert nm.sum() > 100 * F


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("distorted", [False, True])
def test_extract_rgbd_single_frame(oracle, dtype, distorted):
    w, h, nf = 640, 480, 1000
    img = synth.mono_frame(w, h, 21, 0)
    ex = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    plain = orbx.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    pm, pk, pd = plain(img)
    if dtype == np.uint16:
        dep, scale = depth_u16(w, h, 9), orbx.depth_scale_from_settings(5000.0)
    else:
        dep, scale = _edge_depth(w, h, pk, 11), np.float32(1.0)
    dist = TUM1_DIST if distorted else np.zeros(5, np.float32)
    for rep in range(2):
        mono, kps, desc, kun, ur, dp = ex.extract_rgbd(img, dep, TUM1_K, dist, TUM1_BF, scale)
        assert mono == pm and kps.tobytes() == pk.tobytes() and np.array_equal(desc, pd)
        om, ok, od = oracle.OracleExtractor(nf).extract(img) if rep == 0 else (om, ok, od)
        assert mono == om and kps.tobytes() == ok.tobytes()
        okun = oracle.undistort_keypoints(kps, TUM1_K, dist) if distorted else kps
        assert kun.tobytes() == okun.tobytes()
        mu, md = model(kps, okun["x"], dep, scale, TUM1_BF)
        assert np.array_equal(bits(ur), bits(mu)) and np.array_equal(bits(dp), bits(md))
    # orbx_host_results hands out the same arrays in place
    pk_, pd_, pu_, pz_ = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_, m_ = C.c_int(), C.c_int()
    assert orbx.lib().orbx_host_results(ex._h, 0, C.byref(pk_), C.byref(pd_), C.byref(n_), C.byref(m_), C.byref(pu_), C.byref(pz_)) == 0
    n = len(kps)
    assert n_.value == n and m_.value == mono
    assert C.string_at(pk_.value, 28 * n) == kps.tobytes() and C.string_at(pd_.value, 32 * n) == desc.tobytes()
    assert C.string_at(pu_.value, 4 * n) == ur.tobytes() and C.string_at(pz_.value, 4 * n) == dp.tobytes()
    # a plain extraction afterwards hands out no uRight
    ex(img)
    assert orbx.lib().orbx_host_results(ex._h, 0, None, None, None, None, C.byref(pu_), None) == 0 and not pu_.value
