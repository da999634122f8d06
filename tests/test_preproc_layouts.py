"""The pre-processing plans (orbx_preproc_*: CLAHE, cv::remap, input resize, gray) on the memory layouts a caller really hands
over: cv::Mat ROIs and pitched camera buffers -- a row pitch larger than the row, an image pitch larger than the image, a base
pointer that is 16-byte, 4-byte or not at all aligned.  Every kernel of the plans picks a fast form or a fallback by exactly
these alignments (srcVec4 and the wide tile load of CLAHE, the 16-byte staging of k_remap_lds, k_cvt_gray16, the resize through
the pyramid's k_resize), so each plan runs on a matrix of layouts and

  * every result is compared bit for bit with the oracle applied stage by stage to the unpadded frames (no tolerance anywhere);
  * every padding byte and the bytes in front of / behind the frames are random, and a second run with other padding bytes must
    give the identical output (padding is never read into a result);
  * orbx_debug_preproc_plan tells which form ran, and the expected form is asserted per stage from the stage's real input, so
    both sides of every switch are known to have run.

The single-channel resize fast path has no alignment gate: k_resize reads the caller's rows with dword loads at byte addresses
that are only dword aligned when base and pitches are.  These tests measure it on padded and offset frames: the results equal
the oracle's on every layout, so the plan reports `plain` everywhere and no gate was added (see RESIZE_FORM below)."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_fast_amd import synth

pytestmark = pytest.mark.gpu

# What the resize fast path is expected to report: "plain" on every layout (it needs no gate: padded, offset and unaligned frames
# come out equal to the oracle).
RESIZE_FORM = {16: "plain", 4: "plain", 1: "plain"}

FRONT, TAIL = 256, 320   # random bytes in front of the first frame's allocation offset / behind the last frame


def _round_up(v, m):
    return (v + m - 1) // m * m


# (name, alignment class, base offset, row pitch(row bytes), image pitch(pitch, h))
LAYOUTS = [
    ("packed256", None, 0, lambda r: r, lambda p, h: p * h),                                  # today's layout (class follows the row)
    ("a16_rows16", 16, 0, lambda r: _round_up(r, 16), lambda p, h: p * h),
    ("a16_off16_pitch+16", 16, 16, lambda r: _round_up(r, 16) + 16, lambda p, h: p * h + 16 * 3),
    ("a16_pitch+64", 16, 0, lambda r: _round_up(r, 16) + 64, lambda p, h: p * h + 16),
    ("a4_off4_pitch+4", 4, 4, lambda r: _round_up(r, 4) + 4, lambda p, h: p * h + 4),
    ("a4_off8_rows4", 4, 8, lambda r: _round_up(r, 4), lambda p, h: p * h + 4),
    ("a1_off1_pitch+1", 1, 1, lambda r: r + 1, lambda p, h: p * h + 1),
    ("a1_off2_pitch+3", 1, 2, lambda r: r + 3, lambda p, h: p * h + 1),
    ("a1_off3_pitch+1", 1, 3, lambda r: r + 1, lambda p, h: p * h),
]
BATCHES = (1, 2, 9, 17)   # below / above one remap group of eight, odd and even per map


def _align(*values):
    v = 0
    for x in values:
        v |= int(x)
    return 16 if v % 16 == 0 else 4 if v % 4 == 0 else 1


class _Laid:
    """n frames in a device buffer at `base` bytes from a 256-byte aligned allocation, rows rp bytes apart, images ip bytes apart;
    every byte that is no pixel is random (seeded by pad_seed)."""

    def __init__(self, frames, base, rp, ip, pad_seed):
        from orb_slam3_fast_amd.hipmem import DeviceBuffer
        n, h = frames.shape[:2]
        rowb = int(np.prod(frames.shape[2:]))
        assert rp >= rowb and ip >= rp * (h - 1) + rowb
        start = FRONT + base
        host = np.random.default_rng(pad_seed).integers(0, 256, start + (n - 1) * ip + (h - 1) * rp + rowb + TAIL, dtype=np.uint8)
        view = np.lib.stride_tricks.as_strided(host[start:], shape=(n, h, rowb), strides=(ip, rp, 1))
        view[...] = frames.reshape(n, h, rowb)
        self.buf = DeviceBuffer.from_numpy(host)
        assert self.buf.ptr.value % 256 == 0
        self.ptr, self.n, self.rp, self.ip = self.buf.ptr.value + start, n, rp, ip
        self.align = _align(self.ptr, rp, ip)


def _download(ptr, n, w, h, rp, ip):
    from orb_slam3_fast_amd import hipmem
    got = np.zeros(n * ip, np.uint8)
    hipmem._ck(hipmem.hip().hipMemcpy(got.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), got.nbytes, 2))
    return np.lib.stride_tricks.as_strided(got, shape=(n, h, w), strides=(ip, rp, 1)).copy()


def _layout(name_or_index, frames):
    name, cls, base, rpf, ipf = LAYOUTS[name_or_index] if isinstance(name_or_index, int) else next(l for l in LAYOUTS if l[0] == name_or_index)
    h, rowb = frames.shape[1], int(np.prod(frames.shape[2:]))
    rp = rpf(rowb)
    return name, cls, base, rp, ipf(rp, h)


def _run(pp, frames, layout, want, expect, what):
    """One plan on one layout, twice with different padding bytes: both outputs equal the oracle's `want` (hence each other), and
    the plan reports the forms `expect(alignment class of the layout)`."""
    name, cls, base, rp, ip = _layout(layout, frames)
    n = len(frames)
    for pad_seed in (1, 2):
        laid = _Laid(frames, base, rp, ip, 1000 * pad_seed + n)
        assert cls is None or laid.align == cls, (what, name, laid.align)   # the layout is of the class the matrix lists it under
        ptr, w, h, orp, oip = pp.run_device(laid.ptr, n, rp, ip)
        got = _download(ptr, n, w, h, orp, oip)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), (what, name, n, "padding bytes %d" % pad_seed, "frame %d" % i)
        plan = pp.plan()
        assert plan["frames"] == n
        for key, val in expect(laid.align).items():
            assert plan[key] == val, (what, name, n, key, plan)
    return laid.align


def _frames(w, h, n, seed, channels=1):
    """n frames, three distinct ones repeated (the oracle runs once per distinct frame)."""
    rng = np.random.default_rng(seed)
    if channels == 1:
        base = [synth.mono_frame(w, h, seed + i) if w >= 256 else rng.integers(0, 256, (h, w), dtype=np.uint8) for i in range(3)]
    else:
        base = [rng.integers(0, 256, (h, w, channels), dtype=np.uint8) for i in range(3)]
    for b in base:
        b[::7, ::5] = rng.integers(0, 256, b[::7, ::5].shape, dtype=np.uint8)
    return base


def _batch(base, n):
    return np.ascontiguousarray(np.stack([base[i % len(base)] for i in range(n)]))


def _sweep(pp, base, want_of, expect, what, batches_on=("a16_off16_pitch+16", "a4_off4_pitch+4", "a1_off1_pitch+1")):
    """Every layout of the matrix with one batch size each (rotating through BATCHES), and every batch size on one layout of each
    alignment class.  want_of(frame index in `base`, position in the batch) -> expected image."""
    seen = set()
    for li in range(len(LAYOUTS)):
        n = BATCHES[li % len(BATCHES)]
        seen.add(_run(pp, _batch(base, n), li, [want_of(i % len(base), i) for i in range(n)], expect, what))
    for name in batches_on:
        for n in BATCHES:
            _run(pp, _batch(base, n), name, [want_of(i % len(base), i) for i in range(n)], expect, what)
    return seen


# ---- CLAHE ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,grid", [((752, 480), (8, 8)), ((512, 512), (6, 5)), ((80, 35), (3, 4)), ((1280, 720), (8, 8))])
def test_clahe_plan_on_every_layout(oracle, size, grid):
    import orb_slam3_fast_amd as orbx
    w, h = size
    base = _frames(w, h, 3, 31)
    want = [oracle.clahe(b, 3.0, grid) for b in base]
    pp = orbx.Preproc(w, h, clahe=(3.0, grid), max_batch=max(BATCHES))
    seen = _sweep(pp, base, lambda k, i: want[k], lambda al: {"clahe_vec4": al >= 4, "remap": None, "resize": None, "gray_segs": None},
                  ("clahe", size, grid), batches_on=("a1_off2_pitch+3",))
    assert seen == {16, 4, 1}


# ---- remap ------------------------------------------------------------------------------------------------------------------------
def _remap_maps(kind, sw, sh, dw, dh, nmaps):
    maps = []
    for m in range(nmaps):
        if kind == "rectify":
            maps.append(synth.rectify_maps(dw, dh, sw, sh, seed=10 + m))
        else:   # a black left border wider than one tile: whole tiles left of the source (the footprint that used to start at -16)
            u, v = np.meshgrid(np.arange(dw, dtype=np.float32), np.arange(dh, dtype=np.float32))
            maps.append(((u - 140 - 3 * m).astype(np.float32), (v + 0.5 * m).astype(np.float32)))
    return np.stack([a for a, _ in maps]), np.stack([b for _, b in maps])


@pytest.mark.parametrize("src,out,kind,nmaps", [((752, 480), (720, 460), "rectify", 2), ((640, 480), (601, 353), "rectify", 1),
                                                ((1280, 720), (1280, 720), "rectify", 2), ((512, 512), (512, 512), "shift", 1),
                                                ((512, 512), (512, 512), "shift", 2), ((80, 35), (70, 29), "rectify", 1)])
def test_remap_plan_on_every_layout(oracle, src, out, kind, nmaps):
    import orb_slam3_fast_amd as orbx
    (sw, sh), (dw, dh) = src, out
    mapsx, mapsy = _remap_maps(kind, sw, sh, dw, dh, nmaps)
    assert orbx.remap_footprints(mapsx, mapsy, sw, sh) is not None   # (tests/test_remap_footprints.py holds the table itself)
    base = _frames(sw, sh, 3, 32)
    want = [[oracle.remap(b, mapsx[m], mapsy[m]) for m in range(nmaps)] for b in base]
    pp = orbx.Preproc(sw, sh, maps=(mapsx, mapsy), max_batch=max(BATCHES))
    assert pp.plan()["lds_table"]
    # 16-byte aligned base and pitches: the LDS form; anything else: the per-thread windows of k_remap1
    seen = _sweep(pp, base, lambda k, i: want[k][i % nmaps],
                  lambda al: {"remap": orbx.REMAP_LDS if al == 16 else orbx.REMAP_WINDOWS, "clahe_vec4": None, "resize": None, "gray_segs": None},
                  ("remap", src, out, kind, nmaps))
    assert seen == {16, 4, 1}


def test_clahe_then_remap_plan_on_every_layout(oracle):
    """Behind CLAHE the remap reads the handle's own buffer (256-byte aligned, pitch = the row rounded up to 4), whatever the
    caller's layout is: 752 = 47 * 16, so the LDS form runs on EVERY layout, while CLAHE's source form follows the caller."""
    import orb_slam3_fast_amd as orbx
    sw, sh, dw, dh = 752, 480, 720, 460
    mapsx, mapsy = _remap_maps("rectify", sw, sh, dw, dh, 2)
    base = _frames(sw, sh, 3, 33)
    eq = [oracle.clahe(b, 3.0, (8, 8)) for b in base]
    want = [[oracle.remap(e, mapsx[m], mapsy[m]) for m in range(2)] for e in eq]
    pp = orbx.Preproc(sw, sh, maps=(mapsx, mapsy), clahe=(3.0, (8, 8)), max_batch=max(BATCHES))
    clahe_pitch = _round_up(sw, 4)
    remap_in = _align(clahe_pitch, clahe_pitch * sh)   # (base: the handle's allocation)
    assert remap_in == 16
    seen = _sweep(pp, base, lambda k, i: want[k][i % 2],
                  lambda al: {"clahe_vec4": al >= 4, "remap": orbx.REMAP_LDS, "resize": None, "gray_segs": None}, "clahe -> remap")
    assert seen == {16, 4, 1}


# ---- resize -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,out", [((752, 480), (600, 350)), ((1280, 720), (640, 360)), ((512, 512), (700, 650)),
                                     ((640, 480), (601, 353)), ((80, 35), (97, 41))])
def test_mono_resize_plan_on_every_layout(oracle, src, out):
    import orb_slam3_fast_amd as orbx
    (sw, sh), (dw, dh) = src, out
    base = _frames(sw, sh, 3, 34)
    want = [oracle.resize(b, dw, dh) for b in base]
    pp = orbx.Preproc(sw, sh, out_size=(dw, dh), max_batch=max(BATCHES))
    assert pp.plan()["resize_prepared"]
    seen = _sweep(pp, base, lambda k, i: want[k], lambda al: {"resize": RESIZE_FORM[al], "remap": None, "clahe_vec4": None, "gray_segs": None},
                  ("resize", src, out), batches_on=("a1_off3_pitch+1",))
    assert seen == {16, 4, 1}


# ---- gray -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,cn,rgb", [((752, 480), 3, True), ((752, 480), 4, False), ((333, 47), 3, False), ((1280, 720), 4, True),
                                         ((80, 35), 3, True)])
def test_gray_plan_on_every_layout(oracle, size, cn, rgb):
    import orb_slam3_fast_amd as orbx
    w, h = size
    base = _frames(w, h, 3, 35, channels=cn)
    want = [oracle.cvt_gray(b, rgb) for b in base]
    pp = orbx.Preproc(w, h, channels=cn, rgb=rgb, max_batch=max(BATCHES))
    gray_pitch = _round_up(w, 4)
    dst16 = _align(gray_pitch, gray_pitch * h) == 16   # the gray pass looks at its destination pitch as well

    def expect(al):
        return {"gray_segs": w // 16 if al == 16 and dst16 else 0, "remap": None, "resize": None, "clahe_vec4": None}

    seen = _sweep(pp, base, lambda k, i: want[k], expect, ("gray", size, cn, rgb), batches_on=("a16_pitch+64",))
    assert seen == {16, 4, 1}


@pytest.mark.parametrize("src,out,cn", [((640, 480), (601, 353), 3), ((752, 480), (592, 352), 4), ((752, 480), (600, 350), 3)])
def test_colour_resize_then_gray_plan_on_every_layout(oracle, src, out, cn):
    """The gray pass reads the handle's resized frames: its form depends on the OUTPUT geometry alone (16-pixel segments when both
    the colour rows, out_w * cn rounded up to 4, and the gray rows are 16-byte multiples), the colour resize is the generic kernel."""
    import orb_slam3_fast_amd as orbx
    (sw, sh), (dw, dh) = src, out
    base = _frames(sw, sh, 3, 36, channels=cn)
    want = [oracle.cvt_gray(oracle.resize_c(b, dw, dh), True) for b in base]
    pp = orbx.Preproc(sw, sh, channels=cn, rgb=True, out_size=(dw, dh), max_batch=max(BATCHES))
    assert not pp.plan()["resize_prepared"]
    geo_pitch, gray_pitch = _round_up(dw * cn, 4), _round_up(dw, 4)
    segs = dw // 16 if _align(geo_pitch, geo_pitch * dh, gray_pitch, gray_pitch * dh) == 16 else 0
    assert (segs > 0) == (out == (592, 352))
    seen = _sweep(pp, base, lambda k, i: want[k], lambda al: {"resize": "generic", "gray_segs": segs, "remap": None, "clahe_vec4": None},
                  ("resize -> gray", src, out, cn), batches_on=())
    assert seen == {16, 4, 1}


# ---- the extractor behind a plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["a16_off16_pitch+16", "a1_off1_pitch+1"])
def test_raw_extraction_from_padded_and_unaligned_frames(oracle, layout):
    """orbx_extract_batch_raw_device on a padded 16-byte aligned layout and on an unaligned one: pyramid level 0 is the plan's
    output, keypoints and descriptors are the oracle's on the oracle's pre-processed frames."""
    import orb_slam3_fast_amd as orbx
    sw, sh, dw, dh = 752, 480, 720, 460
    L, R = synth.stereo_pair(sw, sh, 21)
    mapsx, mapsy = _remap_maps("rectify", sw, sh, dw, dh, 2)
    frames = np.stack([L, R, R])
    want = [oracle.remap(oracle.clahe(f), mapsx[i % 2], mapsy[i % 2]) for i, f in enumerate(frames)]
    pp = orbx.Preproc(sw, sh, maps=(mapsx, mapsy), clahe=(3.0, (8, 8)), max_batch=3)
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=dw, max_height=dh, max_batch=3)
    oex = oracle.OracleExtractor(1000)
    name, cls, base, rp, ip = _layout(layout, frames)
    laid = _Laid(frames, base, rp, ip, 5)
    assert laid.align == cls
    ex.extract_batch_raw_device(pp, laid.ptr, 3, rp, ip)
    ex.sync()
    plan = pp.plan()
    assert plan["clahe_vec4"] == (cls >= 4) and plan["remap"] == orbx.REMAP_LDS and plan["frames"] == 3
    for i in range(3):
        assert np.array_equal(ex.image_pyramid(0, image=i), want[i]), (layout, i)
        mono, k, d = ex.download(i)
        om, ok_, od = oex.extract(want[i])
        assert mono == om and k.tobytes() == ok_.tobytes() and np.array_equal(d, od), (layout, i)


def test_a_plan_without_a_stage_passes_the_frames_through(oracle):
    """Mono frames, no maps, no resize, no CLAHE: the extractor reads the caller's frames.  Its kernels need 4-byte aligned rows,
    so an unaligned layout is refused with ORBX_E_BADARG; a padded aligned one extracts what the oracle extracts."""
    import orb_slam3_fast_amd as orbx
    w, h = 640, 480
    frames = np.stack([synth.mono_frame(w, h, 41), synth.mono_frame(w, h, 42)])
    pp = orbx.Preproc(w, h, max_batch=2)
    ex = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
    oex = oracle.OracleExtractor(1000)
    for layout in ("a1_off1_pitch+1", "a1_off2_pitch+3"):
        name, cls, base, rp, ip = _layout(layout, frames)
        laid = _Laid(frames, base, rp, ip, 6)
        with pytest.raises(orbx.OrbxError) as err:
            ex.extract_batch_raw_device(pp, laid.ptr, 2, rp, ip)
        assert err.value.code == -2   # ORBX_E_BADARG
    for layout in ("a16_off16_pitch+16", "a4_off4_pitch+4"):
        name, cls, base, rp, ip = _layout(layout, frames)
        laid = _Laid(frames, base, rp, ip, 7)
        ptr, ow, oh, orp, oip = pp.run_device(laid.ptr, 2, rp, ip)
        assert (ptr, ow, oh, orp, oip) == (laid.ptr, w, h, rp, ip)
        plan = pp.plan()
        assert (plan["remap"], plan["resize"], plan["clahe_vec4"], plan["gray_segs"], plan["frames"]) == (None, None, None, None, 2)
        ex.extract_batch_raw_device(pp, laid.ptr, 2, rp, ip)
        ex.sync()
        for i in range(2):
            assert np.array_equal(ex.image_pyramid(0, image=i), frames[i]), (layout, i)
            mono, k, d = ex.download(i)
            om, ok_, od = oex.extract(frames[i])
            assert mono == om and k.tobytes() == ok_.tobytes() and np.array_equal(d, od), (layout, i)
