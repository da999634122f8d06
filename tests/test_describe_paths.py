"""k_describe on the device, where it decides something (tests/describe_cases.py has the scenes, tests/test_describe_census.py the
proof that they get there): its own branch-free fastAtan2 and sinf / cosf alone, every window loader at every misalignment, two
to eight keypoints per wave with every loader following every other one, tail tasks, empty levels and images, the XCD remap with
and without images past its last full group of eight, slots with and without lapping areas, what lies behind a row's end, and
the three arithmetics of the blur.  Everything is compared with the CPU oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import describe_cases as dc
import orb_slam3_fast_amd as orbx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def _kb(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


def _first_bad(got, want):
    return np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:4]


# ------------------------------------------------------------------------------------------ the two functions on their own
def test_fast_atan2_sel_equals_the_oracle_s_fast_atan2(gpu, oracle):
    """fast_atan2_sel (the form k_describe calls: |x| >= |y|, x < 0 and y < 0 as selects) against the oracle's scalar restatement
    of cv::fastAtan2: the integer moment pairs of tests/test_thirdparty_pins.py -- every pair with |m| <= 400, random pairs over
    the reachable range, the neighbourhoods of the axes and diagonals at large magnitudes -- plus both axes, |y| == |x|, each of
    those off by one, and (0, 0), in every sign combination."""
    rng = np.random.default_rng(20220131)
    g = np.arange(-400, 401, dtype=np.int64)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    M = 255 * 5000
    ry, rx = rng.integers(-M, M + 1, 300_000), rng.integers(-M, M + 1, 300_000)
    big = rng.integers(1, M + 1, 20_000)
    eps = rng.integers(-3, 4, 20_000)
    m = np.concatenate([np.arange(0, 4097), rng.integers(1, M + 1, 4000), [M]])
    edge_y, edge_x = [], []
    for sy in (1, -1):
        for sx in (1, -1):
            for d in (-1, 0, 1):
                edge_y += [np.zeros_like(m) + d, sy * m, sy * m, sy * (m + d)]          # x axis, y axis, diagonal, diagonal +- 1
                edge_x += [sx * m, np.zeros_like(m) + d, sx * (m + d), sx * m]
    ys = np.concatenate([gy.ravel(), ry, eps, big, big + eps, -big + eps, big, [0]] + edge_y).astype(np.float32)
    xs = np.concatenate([gx.ravel(), rx, big, eps, big, big, -big + eps, [0]] + edge_x).astype(np.float32)
    assert 1_000_000 < len(ys) < 1_500_000
    want = np.zeros_like(ys)
    f = oracle.lib().oro_fast_atan2_n
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    f.restype = None
    f(ys.ctypes.data, xs.ctypes.data, want.ctypes.data, len(ys))
    got = orbx.debug_fast_atan2(ys, xs)
    bad = _first_bad(got, want)
    assert got.tobytes() == want.tobytes(), "fast_atan2_sel != fastAtan2 at (y, x) = %r: %r, want %r" % (
        list(zip(ys[bad], xs[bad])), got[bad], want[bad])
    assert want[(ys == 0) & (xs == 0)].tolist() == [0.0] * int(((ys == 0) & (xs == 0)).sum())


def test_sincosf_sel_equals_host_libm(gpu, oracle):
    """glibc_sincosf_sel -- the branch-free restatement k_describe calls: n = 0 below 0x3f4, `tiny` as a select, the cosine's
    coefficients sign-flipped -- against the host libm bit for bit, on exactly the angles of
    test_gpu_parity.test_device_sincos_equals_host_libm (which keeps comparing the two forms of orbx_sincos.h): 1.2e7 angles formed
    the way the path forms them, a strided sweep of every float in [0, 2 pi], the float neighbourhoods of the quadrant boundaries
    and of 2^-12."""
    around = []
    for q in (np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, 5 * np.pi / 4, 3 * np.pi / 2, 7 * np.pi / 4, 2 * np.pi, 2.0 ** -12):
        b = np.float32(q).view(np.uint32).astype(np.int64)
        around.append((b + np.arange(-4096, 4097)).astype(np.uint32).view(np.float32))
    sweep = np.arange(0, 0x40C91000, 97, dtype=np.uint32).view(np.float32)   # 1.1e7 floats across [0, 2 pi]
    ang = np.concatenate([oracle.reachable_angles(20220131, 12_000_000), sweep] + around).astype(np.float32)
    hs, hc = oracle.libm_sincos(ang)
    ds, dc_ = orbx.debug_sincos(ang, 2)
    assert ds.tobytes() == hs.tobytes(), "glibc_sincosf_sel: sinf != host libm at %r" % ang[_first_bad(ds, hs)]
    assert dc_.tobytes() == hc.tobytes(), "glibc_sincosf_sel: cosf != host libm at %r" % ang[_first_bad(dc_, hc)]


# ------------------------------------------------------------------------------------------------------ scenes as batches
def _upload(scenes, pitch, fill=0):
    """The scenes' frames in one device buffer with `pitch` bytes per row; the bytes behind a row hold `fill`."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    h, w = scenes[0].h, scenes[0].w
    host = np.full((len(scenes), h, pitch), fill, np.uint8)
    for i, sc in enumerate(scenes):
        host[i, :, :w] = sc.img
    return DeviceBuffer.from_numpy(host)


def _extractor(scenes):
    sc = scenes[0]
    return orbx.ORBextractor(dc.NFEATURES, dc.SCALE, sc.nlevels, dc.INI_TH, dc.MIN_TH, max_width=sc.w, max_height=sc.h,
                             max_batch=len(scenes))


def _run(ex, buf, scenes, pitch, laps=None):
    sc = scenes[0]
    ex.extract_batch_device(buf.ptr.value, len(scenes), sc.w, sc.h, pitch, pitch * sc.h, lap=laps)
    ex.sync()
    return [ex.download(i) for i in range(len(scenes))]


def _compare(oracle, got, scenes, laps=None, variant=451, tag=""):
    for i, (sc, (mono, k, d)) in enumerate(zip(scenes, got)):
        lap = (0, 0) if laps is None else laps[i]
        omono, ok_, od = dc.oracle_run(oracle, sc, lap, variant)
        assert mono == omono and len(k) == len(ok_), (tag, i, sc.name, mono, omono, len(k), len(ok_))
        bad = np.flatnonzero((_kb(k) != _kb(ok_)).any(1))
        assert not len(bad), (tag, i, sc.name, "records", bad[:4], k[bad[:4]], ok_[bad[:4]])
        bad = np.flatnonzero((d != od).any(1))
        assert not len(bad), (tag, i, sc.name, "descriptors", bad[:4], ok_[bad[:4]])


@pytest.mark.parametrize("lapping", [False, True], ids=["nolap", "lap"])
@pytest.mark.parametrize("group,frames", dc.BATCHES, ids=["%s-%d" % b for b in dc.BATCHES])
def test_scene_batches_equal_the_oracle(gpu, oracle, group, frames, lapping):
    """Every scene, cycled through a device batch whose size sets k_describe's keypoints per wave (1 .. 8 over the batches,
    tests/test_describe_census.py), once with slots by position (no lapping area: slot == nullptr) and once with per-image
    lapping areas (slots from k_slots): the raw 28-byte records and the descriptors of every image against the oracle."""
    scenes = dc.batch_scenes(group, frames)
    pitch = (scenes[0].w + 3) & ~3                 # the device entry takes rows on 4-byte pitches: dense where w allows it
    laps = [dc.lap_of(sc) for sc in scenes] if lapping else None
    ex = _extractor(scenes)
    buf = _upload(scenes, pitch)
    got = _run(ex, buf, scenes, pitch, laps)
    _compare(oracle, got, scenes, laps, tag=(group, frames, lapping))
    if lapping:      # the lapping areas do split keypoints: some image has keypoints on both sides of its mono index
        assert any(0 < mono < len(k) for mono, k, _ in got)
    assert sum(len(k) for _, k, _ in got) > 0
    ex.close()
    buf.free()


@pytest.mark.parametrize("w", dc.STRIP_WIDTHS)
def test_bytes_behind_a_row_never_reach_a_result(gpu, oracle, w):
    """The `rowend` loader reads whole dwords up to the row's last pixel and clamps the columns behind it, which "only feed unused
    outputs".  Level 0 from a device buffer whose rows are 8 to 11 bytes longer than w, the padding 0x00, then 0xFF: the same
    results, the oracle's.  Then the levels above, whose rows the handle owns: its work buffers (the pyramid with its row padding
    among them) set to 0x00 and to 0xFF before the call."""
    scenes = dc.strip_group(w)
    pitch = ((w + 3) & ~3) + 8
    ex = _extractor(scenes)
    res = []
    for fill in (0x00, 0xFF):
        buf = _upload(scenes, pitch, fill)
        res.append(_run(ex, buf, scenes, pitch))
        _compare(oracle, res[-1], scenes, tag=(w, "row padding", fill))
        buf.free()
    buf = _upload(scenes, pitch, 0x5A)
    for fill in (0x00, 0xFF):
        ex.debug_fill_work_buffers(fill)
        res.append(_run(ex, buf, scenes, pitch))
        _compare(oracle, res[-1], scenes, tag=(w, "work buffers", fill))
    for r in res[1:]:
        for (m0, k0, d0), (m1, k1, d1) in zip(res[0], r):
            assert m0 == m1 and k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()
    ex.close()
    buf.free()


@pytest.mark.parametrize("variant", [440, 44016, 44032])
def test_strips_under_the_opencv_4_4_blur_variants(gpu, oracle, variant):
    """The strips under the taps of OpenCV 4.0 .. 4.5.0: the scalar model (440: no vector body, bodyEnd = 0) and the flooring 16- /
    32-lane vector bodies, whose last floored column bodyEnd = w & ~(lanes - 1) cuts through the patches of the keypoints near the
    right edge (tests/test_describe_census.py counts them per variant) -- on the `rowend` and the reflecting loader."""
    for w in dc.STRIP_WIDTHS:
        scenes = dc.strip_group(w)
        pitch = (w + 3) & ~3
        ex = _extractor(scenes)
        ex.set_opencv_compat(variant)
        buf = _upload(scenes, pitch)
        _compare(oracle, _run(ex, buf, scenes, pitch), scenes, variant=variant, tag=(w, variant))
        ex.close()
        buf.free()
