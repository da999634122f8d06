"""k_resize_stream -- the batched path's pyramid kernel for the levels k_resize_tail does not fuse: one-wave workgroups without LDS,
a lane per destination quad walking the source rows of a band -- against the tiled k_resize and the oracle's cv::resize port, byte
for byte on every level, and its lane tables field by field (no GPU).

orbx_debug_resize_stream runs one of the two kernels on every level of any batch, with the strip width and band height the test
asks for.  Frames: 307 x 141 and 310 x 150 with a (1.2, 5) pyramid -- levels 1 .. 4 are 256 / 213 / 178 / 148 and 258 / 215 / 179 /
149 pixels wide: all four widths mod 4; 64 quads (a last strip exactly full, for strips of 64 and of 32 quads) and 65 quads (a last
strip of exactly one quad, for both); the fifth level is the smallest on which a handle exists (67 px).  test_cases_reach_every_path
holds those facts, and that the band boundaries of the runs fall on destination rows whose source row advances by 1 and by 2.

The bottom row: with a scale factor above 1 the last destination row's lower source row is at most the source's last row
(fy < Sh - 1), so cv::resize's clamp of sy + 1 never changes a row here; what the tables give is that the walk ends ON the source's
last row (every level of both frames: asserted), the row a kernel that ran one row too far would leave the image with."""
import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from test_front_tables import levels, resize_axis

NL = 5
PRM = (500, 1.2, NL, 20, 7)
FRAMES = [(307, 141), (310, 150)]
NIMG = 5
TABLE_SIZES = [(307, 141, NL), (310, 150, NL), (1280, 720, 8), (752, 480, 8), (640, 480, 8)]
# (frame, images, quads per strip, destination rows per band); 0 = what the batched path launches (32 quads, 16 rows).
# Batches of 1, 2, 3 and 5 with both strip widths: strips of 32 quads pair the half-waves over two images, an odd batch idles one.
DEF_QUADS, DEF_BAND = 32, 16
RUNS = [((307, 141), 3, 0, 0), ((310, 150), 5, 0, 0), ((310, 150), 1, 32, 16), ((307, 141), 2, 32, 16), ((310, 150), 3, 32, 7),
        ((307, 141), 5, 32, 5), ((307, 141), 1, 64, 16), ((310, 150), 2, 64, 16), ((307, 141), 3, 64, 7), ((310, 150), 5, 64, 16)]


def _frames(w, h):
    """NIMG frames of uniform noise: every byte of every level depends on its own taps."""
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (NIMG, h, w), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ tables (no GPU)
@pytest.mark.parametrize("quads", [64, 32])
@pytest.mark.parametrize("w,h,nl", TABLE_SIZES)
def test_lane_tables(w, h, nl, quads):
    """Every lane of every strip: its 8-byte load stays inside the source row, its selectors pick S[sx] and S[min(sx + 1, W - 1)]
    out of the loaded bytes, its coefficients are cv::resize's; lanes past the last quad repeat it and are marked."""
    tabs = orbx.resize_stream_tables(1000, 1.2, nl, 20, 7, w, h, quads)
    lv = levels(w, h, nl)
    assert tabs[0] is None
    for l in range(1, nl):
        D, S = lv[l], lv[l - 1]
        sx, a0, a1 = resize_axis(D["w"], S["w"])
        nq = -(-D["w"] // 4)
        t = tabs[l]
        assert t is not None and t.shape == (-(-nq // quads), 3, quads, 4)
        for qi in range(t.shape[0] * quads):
            sel, coef, misc = (t[qi // quads, k, qi % quads].astype(np.int64) for k in range(3))
            qv = min(qi, nq - 1)
            off = int(misc[0])
            assert 0 <= off and off + 8 <= S["w"], (l, qi, off)
            assert int(misc[1]) == (4 * qi if qi < nq else 0xFFFFFFFF) and misc[2] == 0 and misc[3] == 0
            for j in range(4):
                x = min(4 * qv + j, D["w"] - 1)      # (the columns past the level's width repeat its last column)
                s = min(max(sx[x], 0), S["w"] - 1)
                want = (2048, 0) if sx[x] < 0 or sx[x] >= S["w"] - 1 else (a0[x], a1[x])
                b0, b1 = int(sel[j]) & 0xFF, (int(sel[j]) >> 16) & 0xFF
                assert 0 <= b0 <= 7 and 0 <= b1 <= 7 and (int(sel[j]) & 0xFF00FF00) == 0x0C000C00, (l, qi, j, hex(int(sel[j])))
                assert off + b0 == s and off + b1 == min(s + 1, S["w"] - 1), (l, qi, j)
                assert (int(coef[j]) & 0xFFFF, int(coef[j]) >> 16) == want, (l, qi, j)


def test_tables_reject_bad_arguments():
    import ctypes as C
    prm = orbx._Params(1000, 1.2, 8, 20, 7)
    off = np.zeros(12, np.int32)
    L = orbx.lib()
    assert L.orbx_debug_resize_stream_tables(C.byref(prm), 640, 480, 48, None, 0, orbx._p(off)) == orbx.E_BADARG
    n = L.orbx_debug_resize_stream_tables(C.byref(prm), 640, 480, 64, None, 0, orbx._p(off))
    assert n > 0 and off[0] == -1 and off[1] == 0 and (off[8:] == -1).all()
    buf = np.full(n + 2, 0xABCD, np.uint32)
    assert L.orbx_debug_resize_stream_tables(C.byref(prm), 640, 480, 64, orbx._p(buf), n - 1, orbx._p(off)) < 0
    assert (buf == 0xABCD).all()
    assert L.orbx_debug_resize_stream_tables(C.byref(prm), 640, 480, 64, orbx._p(buf), n, orbx._p(off)) == n
    assert (buf[n:] == 0xABCD).all()


def test_cases_reach_every_path():
    seen = set()
    for (w, h), _, quads, band in RUNS:
        quads, band = quads or DEF_QUADS, band or DEF_BAND
        lv = levels(w, h, NL)
        for l in range(1, NL):
            D, S = lv[l], lv[l - 1]
            nq = -(-D["w"] // 4)
            seen.add("w%%4=%d" % (D["w"] % 4))
            if nq % quads == 1:
                seen.add("last strip of one quad / %d" % quads)
            if nq % quads == 0:
                seen.add("last strip full / %d" % quads)
            sy, _, _ = resize_axis(D["h"], S["h"])
            assert 0 <= sy[0] and sy[-1] + 1 == S["h"] - 1          # no clamp; the walk ends on the source's last row
            for y in range(band, D["h"], band):
                seen.add("band boundary, sy step %d" % (sy[y] - sy[y - 1]))
    assert seen == {"w%4=0", "w%4=1", "w%4=2", "w%4=3", "last strip of one quad / 64", "last strip full / 64",
                    "last strip of one quad / 32", "last strip full / 32", "band boundary, sy step 1", "band boundary, sy step 2"}
    assert {n for _, n, q, _ in RUNS if (q or DEF_QUADS) == 32} == {1, 2, 3, 5} == {n for _, n, q, _ in RUNS if q == 64}


# ------------------------------------------------------------------------------------------------------------------- GPU
class _Bench:
    """One handle, the frames of both sizes on the device, and -- computed once, read by every test -- the levels the oracle's
    cv::resize chain and the tiled k_resize make of them."""

    def __init__(self, oracle):
        from orb_slam3_fast_amd.hipmem import DeviceBuffer
        self.ex = orbx.ORBextractor(*PRM, max_width=320, max_height=160, max_batch=NIMG)
        self.host, self.dev, self.dev4, self.want, self.tiled = {}, {}, {}, {}, {}
        for (w, h) in FRAMES:
            f = self.host[(w, h)] = _frames(w, h)
            self.dev[(w, h)] = DeviceBuffer.from_numpy(f)
            p4 = (w + 3) & ~3                       # the same frames with 4-byte aligned rows, for the entries that need them
            f4 = np.zeros((NIMG, h, p4), np.uint8)
            f4[:, :, :w] = f
            self.dev4[(w, h)] = (DeviceBuffer.from_numpy(f4), p4)
            lv = levels(w, h, NL)
            ref = []
            for i in range(NIMG):
                chain = [f[i]]
                for l in range(1, NL):
                    chain.append(oracle.resize(chain[-1], lv[l]["w"], lv[l]["h"]))
                ref.append(chain)
            self.want[(w, h)] = ref
            self.ex.debug_resize_stream(self.dev4[(w, h)][0].ptr.value, NIMG, w, h, p4, p4 * h, kernel=0)
            self.tiled[(w, h)] = [self.ex.pyramid_download(i) for i in range(NIMG)]

    def check(self, size, n, tag):
        for i in range(n):
            got = self.ex.pyramid_download(i)
            for l in range(1, NL):
                assert got[l].shape == self.want[size][i][l].shape
                bad = np.argwhere(got[l] != self.want[size][i][l])
                assert len(bad) == 0, (tag, "oracle", i, l, bad[:4])
                assert np.array_equal(got[l], self.tiled[size][i][l]), (tag, "k_resize", i, l)


@pytest.fixture(scope="module")
def bench(oracle):
    return _Bench(oracle)


@pytest.mark.gpu
def test_tiled_kernel_matches_the_oracle(bench):
    """The second reference of the tests below is itself the oracle's (k_resize through the hook, batch of five)."""
    for size in FRAMES:
        for i in range(NIMG):
            for l in range(1, NL):
                assert np.array_equal(bench.tiled[size][i][l], bench.want[size][i][l]), (size, i, l)


@pytest.mark.gpu
@pytest.mark.parametrize("size,n,quads,band", RUNS)
def test_stream_levels(bench, size, n, quads, band):
    w, h = size
    bench.ex.debug_fill_work_buffers(0x5A)     # (nothing of an earlier run's pyramid survives into this one)
    bench.ex.debug_resize_stream(bench.dev[size].ptr.value, n, w, h, w, w * h, kernel=1, quads=quads, band=band)
    bench.check(size, n, (size, n, quads, band))


@pytest.mark.gpu
@pytest.mark.parametrize("quads", [64, 32])
def test_padded_pitch_and_odd_base(bench, quads):
    """Level 0 in a caller's buffer: rows 13 bytes apart from the width, images an odd count of bytes apart, the first pixel at an
    odd address; the bytes between the rows are 0xFF / 0x00 stripes a load that left its row would blend in."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    for size in FRAMES:
        w, h = size
        pitch, ipitch, n = w + 13, (w + 13) * h + 7, 3
        buf = np.zeros(1 + n * ipitch + 16, np.uint8)
        buf[::2] = 0xFF
        for i in range(n):
            rows = np.lib.stride_tricks.as_strided(buf[1 + i * ipitch:], (h, w), (pitch, 1))
            rows[:] = bench.host[size][i]
        d = DeviceBuffer.from_numpy(buf)
        bench.ex.debug_resize_stream(d.ptr.value + 1, n, w, h, pitch, ipitch, kernel=1, quads=quads)
        bench.check(size, n, (size, "padded", quads))
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_work_buffers(bench, byte):
    size = FRAMES[1]
    w, h = size
    bench.ex.debug_fill_work_buffers(byte)
    bench.ex.debug_resize_stream(bench.dev[size].ptr.value, NIMG, w, h, w, w * h, kernel=1)
    bench.check(size, NIMG, ("poison", byte))


@pytest.mark.gpu
def test_batched_extraction_launches_it(bench):
    """The wiring: an extraction of more than two images builds the same levels (k_resize_stream + k_resize_tail), and one of two
    images (the cascade plans) does too."""
    size = FRAMES[0]
    w, h = size
    d4, p4 = bench.dev4[size]
    for n in (NIMG, 2):
        bench.ex.debug_fill_work_buffers(0xA5)
        bench.ex.extract_batch_device(d4.ptr.value, n, w, h, p4, p4 * h)
        bench.ex.sync()
        bench.check(size, n, ("extract", n))


@pytest.mark.gpu
def test_hook_rejects_bad_arguments(bench):
    size = FRAMES[0]
    w, h = size
    p = bench.dev[size].ptr.value
    L = orbx.lib()
    hd = bench.ex._h
    assert L.orbx_debug_resize_stream(None, p, 1, w, h, w, w * h, 1, 0, 0) == orbx.E_BADARG
    assert L.orbx_debug_resize_stream(hd, p, NIMG + 1, w, h, w, w * h, 1, 0, 0) == orbx.E_CAPACITY
    assert L.orbx_debug_resize_stream(hd, p, 1, w, h, w, w * h, 2, 0, 0) == orbx.E_BADARG
    assert L.orbx_debug_resize_stream(hd, p, 1, w, h, w, w * h, 1, 48, 0) == orbx.E_BADARG
    assert L.orbx_debug_resize_stream(hd, p + 1, 1, w, h, w + 1, (w + 1) * h, 0, 0, 0) == orbx.E_BADARG   # the tiled kernel loads dwords
    assert L.orbx_debug_resize_stream(hd, p, 1, w, h, w - 1, w * h, 1, 0, 0) == orbx.E_BADARG
