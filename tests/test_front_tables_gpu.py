"""GPU parity behind the table-driven fronts of k_detect and k_resize: batches of three images on the small geometries of
tests/test_front_tables.py (one per compiled LDS tile pitch, one on the run-time pitch, and the two that hold the cell kinds
only a large level has), bit for bit against the oracle -- every pyramid level, the per-level FAST candidates, the final
keypoint records and descriptors.  Images 1 and 2 exercise the per-image base and the XCD rotation of the block order (the
grids are no multiples of 64); the level-0 frames sit in a buffer whose row pitch exceeds the width and whose image pitch
exceeds pitch x height.  Every level goes through k_resize (the fused small-level launches are switched off), and one more
pass runs with k_detect's LDS list shrunk so that the flush paths run behind the new front."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

GEOMS = [(383, 100, 2), (357, 166, 6), (340, 199, 7), (364, 239, 8), (241, 239, 8), (1118, 165, 2), (470, 897, 2)]
REJECT, WIDE = 1, 2
T_FAST, T_WHOLE = 1, 2
NF = 500


def _kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


def _level_sizes(w, h, nl):
    sc, out = np.float32(1), []
    for _ in range(nl):
        inv = np.float32(1) / sc
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
        sc = np.float32(float(sc) * float(np.float32(1.2)))
    return out


def _kinds(w, h, nl):
    """The kinds of cells and tiles this geometry holds, read from the tables the kernels use."""
    cells, tab, tile_p, _ = orbx.front_tables(NF, 1.2, nl, 20, 7, w, h)
    fl = cells[:, 2]
    ok = (fl & REJECT) == 0
    dw, dh = (cells[:, 1] & 0xFFFF).astype(int) - 6, (cells[:, 1] >> 16).astype(int) - 6
    dq = ((cells[:, 7] >> 8) & 0xFF).astype(int)
    kinds = {("pitch", tile_p if tile_p in (44, 48, 52, 56) else 0)}
    if (~ok).any():
        kinds.add("rejected cell")
    if (ok & ((fl & WIDE) == 0)).any():
        kinds.add("last-column cell on the narrow loader")
    if (ok & (dh < dq)).any():
        kinds.add("last-row cell shorter than a round")
    if (ok & (dw > 58)).any():
        kinds.add("cell wider than 58 px")
    pos = 0
    for l, (lw, lh) in enumerate(_level_sizes(w, h, nl)):
        if l == 0:
            continue
        nbx, nby = -(-lw // 256), -(-lh // 16)
        t = tab[pos:pos + 8 * nbx * nby].reshape(nby, nbx, 8)
        pos += 8 * nbx * nby + 64 * nby
        ndw, tf = t[:, :, 3] >> 16, t[:, :, 4]
        if ((tf & T_FAST) != 0).any():
            kinds.add("straight-line loader")
        if (((tf & T_FAST) == 0) & ((tf & T_WHOLE) != 0) & (ndw > 64))[-2:].any():
            kinds.add("footprint on the level's last rows")
        if nbx > 1 and (ndw[:, -1] <= 64).all():
            kinds.add("narrow last tile column")
        if l == 1 and ((tf & T_WHOLE) == 0).any():
            kinds.add("level-0 last dword read byte-wise")
    assert pos == len(tab)
    return kinds


def test_the_geometries_hold_every_kind_of_cell_and_tile():
    kinds = set()
    for g in GEOMS:
        kinds |= _kinds(*g)
    assert kinds == {("pitch", 44), ("pitch", 48), ("pitch", 52), ("pitch", 56), ("pitch", 0), "rejected cell",
                     "last-column cell on the narrow loader", "last-row cell shorter than a round", "cell wider than 58 px",
                     "straight-line loader", "footprint on the level's last rows", "narrow last tile column",
                     "level-0 last dword read byte-wise"}


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.fixture(scope="module")
def references(oracle):
    """Per geometry: three frames (textured, half noise -- dense cells for the flush paths --, low contrast zone for the
    minimum-threshold pass) and the oracle's levels, candidates and results for each.  Computed once."""
    ref = {}
    for gi, (w, h, nl) in enumerate(GEOMS):
        rng = np.random.default_rng(100 + gi)
        imgs = [synth.mono_frame(w, h, 500 + 3 * gi + i) for i in range(3)]
        imgs[1][:, w // 2:] = rng.integers(0, 256, (h, w - w // 2), dtype=np.uint8)
        imgs[2][: h // 3, : w // 2] = imgs[2][: h // 3, : w // 2] // 8 + 90
        per = []
        for im in imgs:
            oe = oracle.OracleExtractor(NF, 1.2, nl, 20, 7)
            mono, k, d = oe.extract(im, (0, 0))
            cands = []
            for l in range(nl):
                c = oe.detect_candidates(l)
                v = np.stack([c["x"], c["y"], c["response"]], 1).astype(np.int32)
                cands.append(v[np.lexsort(v.T[::-1])])
            per.append(dict(mono=mono, k=k, d=d, levels=[oe.level(l).copy() for l in range(nl)], cands=cands))
        ref[(w, h, nl)] = (imgs, per)
    return ref


def _run_and_compare(w, h, nl, imgs, per, stages):
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    pitch = (w + 3) // 4 * 4 + 8                      # row pitch > width, image pitch > pitch * height
    buf = np.full((3, h + 3, pitch), 0xA5, np.uint8)
    for i in range(3):
        buf[i, :h, :w] = imgs[i]
    dev = DeviceBuffer.from_numpy(buf)
    ex = orbx.ORBextractor(NF, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
    ex.extract_batch_device(dev.ptr.value, 3, w, h, pitch, pitch * (h + 3))
    ex.sync()
    for i in range(3):
        want = per[i]
        if stages:
            for l in range(nl):
                assert np.array_equal(ex.image_pyramid(l, image=i), want["levels"][l]), "image %d pyramid level %d" % (i, l)
            for l in range(nl):
                got = ex.debug_candidates(l, image=i)
                assert np.array_equal(got[np.lexsort(got.T[::-1])], want["cands"][l]), "image %d candidates level %d" % (i, l)
        mono, k, d = ex.download(i)
        assert mono == want["mono"] and len(k) == len(want["k"]), i
        assert np.array_equal(_kp_bytes(k), _kp_bytes(want["k"])), i
        assert np.array_equal(d, want["d"]), i
    dev.free()


@pytest.mark.parametrize("w,h,nl", GEOMS)
def test_batches_of_three_against_the_oracle(gpu, references, w, h, nl):
    imgs, per = references[(w, h, nl)]
    assert sum(len(p["k"]) for p in per) > 50
    lib = orbx.lib()
    lib.orbx_debug_set_resize_tail(0, 0, 0)           # every level through k_resize
    try:
        _run_and_compare(w, h, nl, imgs, per, True)
        lib.orbx_debug_set_detect_list_cap(320)       # mid-cell flushes, the corner limit, the tile-scan NMS
        _run_and_compare(w, h, nl, imgs, per, False)
    finally:
        lib.orbx_debug_set_detect_list_cap(1024)
        lib.orbx_debug_set_resize_tail(-1, 0, 0)


def test_default_level_fusion_keeps_its_levels(gpu, references):
    """With the library's own policy the small levels go through the fused launches and the others through k_resize."""
    w, h, nl = GEOMS[3]
    imgs, per = references[(w, h, nl)]
    _run_and_compare(w, h, nl, imgs, per, True)
