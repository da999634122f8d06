"""The scenes of tests/describe_cases.py reach every place where k_describe decides something -- CONDITIONS on the scene set, met
by the CPU oracle alone, so that the device tests of tests/test_describe_paths.py cannot pass by never getting there:

* every (level class, window loader, misalignment) cell and every reflected side and corner that exists at the scenes' level
  geometries has a keypoint (the required sets come from describe_cases.enumerate_reachable, not from the scenes);
* the blob scene holds the exact angles on the axes and diagonals and the angles under 2^-12 rad;
* every batch of the device tests lets a wave meet each loader after each other one, a tail task and a level whose count is a
  multiple of its keypoints per wave -- with nk taken from the plan tap (orbx_debug_describe_plan), not from a formula here;
* the plan's magic multiplier divides exactly for every flat workgroup index of up to 64 images.
"""
import ctypes as C

import numpy as np
import pytest

import describe_cases as dc
import orb_slam3_fast_amd as orbx


def _plan(scene, frames):
    return orbx.describe_plan(dc.NFEATURES, dc.SCALE, scene.nlevels, dc.INI_TH, dc.MIN_TH, scene.w, scene.h, frames)


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_level_geometries_are_the_oracle_s(oracle):
    for sc in dc.all_scenes():
        oe = oracle.OracleExtractor(dc.NFEATURES, dc.SCALE, sc.nlevels, dc.INI_TH, dc.MIN_TH)
        oe.compute_pyramid(sc.img)
        assert [(g[0], g[1]) for g in sc.geom] == [oe.level(l).shape[::-1] for l in range(sc.nlevels)], sc.name


def test_reachable_cells_of_the_strip_geometries():
    """Where the `rowend` loader (interior window, 48-byte rows past the row's end) exists at all: at level 0 in the band of at
    most five columns left of w - 21, with the misalignments w mod 4 allows; above level 0 only where pitch - w <= 4."""
    want0 = {192: {0, 1}, 193: {0, 1, 2}, 194: {0, 1, 2, 3}, 195: {0, 1, 2, 3}}
    for w, mis in want0.items():
        cells, sides = dc.enumerate_reachable(dc.geometry(w, dc.STRIP_H, 3)[0])
        assert {m for p, m in cells if p == "rowend"} == mis, w
        assert {m for p, m in cells if p == "dma"} == {m for p, m in cells if p == "reflect"} == {0, 1, 2, 3}
        assert sides == {dc.LEFT, dc.TOP, dc.RIGHT, dc.BOTTOM, 3, 6, 9, 12}
    for w in (230, 231):
        g = dc.geometry(w, dc.STRIP_H, 3)
        assert g[1][:3] == (192, 100, 192)                                  # level 1: as wide as its pitch
        assert {m for p, m in dc.enumerate_reachable(g[1])[0] if p == "rowend"} == {0, 1}
        assert not {m for p, m in dc.enumerate_reachable(g[2])[0] if p == "rowend"}
    for g in dc.geometry(dc.BIG_W, dc.BIG_H, 3)[1:]:                        # pitch - w = 36 / 30: no rowend above level 0
        assert g[2] - g[0] > 4 and not {m for p, m in dc.enumerate_reachable(g)[0] if p == "rowend"}
    # brute force of one geometry against the kernel's expressions written out per key
    w, h, pitch, level = g = (50, 47, 52, 1)
    for X in range(19, w - 19):
        for Y in range(19, h - 19):
            xs = (X - 21) // 4 * 4
            interior = X >= 21 and Y >= 21 and X + 21 < w and Y + 21 < h
            want = 0 if interior and xs + 48 <= pitch else 1 if interior else 2
            p, m, s = dc.classify(g, [X], [Y])
            assert (int(p[0]), int(m[0])) == (want, X - 21 - xs) and bool(s[0]) == (not interior)


# ------------------------------------------------------------------------------------------------------------ the census
def test_every_reachable_cell_side_and_corner_has_a_keypoint(oracle):
    scenes = dc.all_scenes()
    need_cells, need_sides = dc.required(scenes)
    assert {(c, p) for c, p, _ in need_cells} == {(0, "dma"), (0, "rowend"), (0, "reflect"), (1, "dma"), (1, "rowend"), (1, "reflect")}
    assert {m for c, p, m in need_cells if (c, p) == (0, "rowend")} == {0, 1, 2, 3}
    assert {m for c, p, m in need_cells if (c, p) == (1, "rowend")} == {0, 1}
    assert need_sides == {dc.LEFT, dc.TOP, dc.RIGHT, dc.BOTTOM, 3, 6, 9, 12}
    cells, sides = {}, {}
    for sc in scenes:
        c, s = dc.census(oracle, sc)
        print(sc.name, [len(x) for x, _ in dc.keys_per_level(oracle, sc)], sorted(c.items()), sorted(s.items()))
        for k, v in c.items():
            cells[k] = cells.get(k, 0) + v
        for k, v in s.items():
            sides[k] = sides.get(k, 0) + v
    assert not need_cells - set(cells), sorted(need_cells - set(cells))
    assert not set(cells) - need_cells, sorted(set(cells) - need_cells)      # (a keypoint where the enumeration sees no key)
    assert not need_sides - set(sides), sorted(need_sides - set(sides))
    assert min(cells[c] for c in need_cells) >= 5, sorted(cells.items())    # room to spare: no cell hangs on one keypoint


def test_rowend_is_hit_at_every_misalignment_its_width_allows(oracle):
    """Per strip width, not only over the union: level 0 at every mis the width's enumeration lists, level 1 of 230 / 231 at both."""
    for w in dc.STRIP_WIDTHS:
        hit = {}
        for sc in dc.strip_group(w):
            for k, v in dc.census(oracle, sc)[0].items():
                hit[k] = hit.get(k, 0) + v
        g = dc.geometry(w, dc.STRIP_H, 3)
        for lv in (0, 1):
            need = {m for p, m in dc.enumerate_reachable(g[lv])[0] if p == "rowend"}
            assert need == {m for (c, p, m) in hit if (c, p) == (lv, "rowend")}, (w, lv, sorted(hit.items()))


def test_empty_and_one_level_scenes(oracle):
    big = {s.name: s for s in dc.big_group()}
    flat = big["flat%dx%d" % (dc.BIG_W, dc.BIG_H)]
    mono, k, d = dc.oracle_run(oracle, flat)
    assert len(k) == 0
    for sc, count in [(big["dots%dx%d_%d" % (dc.BIG_W, dc.BIG_H, dc.DOTS_BIG)], dc.DOTS_BIG)] + [(dc.strip_group(w)[-1], dc.DOTS_STRIP)
                                                                                              for w in dc.STRIP_WIDTHS]:
        assert [len(x) for x, _ in dc.keys_per_level(oracle, sc)] == [count] + [0] * (sc.nlevels - 1), sc.name


def test_blob_scene_holds_the_exact_and_the_tiny_angles(oracle):
    exact, tiny = dc.blob_expectations()
    blobs = [s for s in dc.big_group() if s.name.startswith("blobs")][0]
    _, k, _ = dc.oracle_run(oracle, blobs)

    def angle_at(cx, cy):
        m = (k["octave"] == 0) & (k["x"] == cx) & (k["y"] == cy)
        assert m.sum() == 1, (cx, cy)
        return k["angle"][m][0]

    got = [angle_at(cx, cy) for cx, cy, _ in exact]
    assert [g.tobytes() for g in got] == [np.float32(a).tobytes() for _, _, a in exact], got
    assert sorted(a for _, _, a in exact) == [0.0, 0.0, 44.990456, 90.0, 135.00955, 180.0, 224.99045, 270.0, 315.00955]
    low = [a for a in (angle_at(cx, cy) for cx, cy, dy in tiny if dy > 0)]
    high = [a for a in (angle_at(cx, cy) for cx, cy, dy in tiny if dy < 0)]
    assert low and all(0 < a < dc.TINY_DEG for a in low), low               # the `tiny` select: sin = y, cos = 1
    assert high and all(360 - dc.TINY_DEG < a < 360 for a in high), high    # its mirror just under 360: the full reduction, n = 4
    assert len(set(low)) == len(low) and len(set(high)) == len(high)


def test_strip_patches_straddle_the_vector_body_s_end(oracle):
    """Per blur variant of OpenCV 4.0 .. 4.5.0 the strips hold keypoints whose 37 patch columns lie on both sides of bodyEnd, the
    column where the flooring vector body ends: k_describe floors per lane and patch column (sBody).  440 is the scalar model,
    it has no body (bodyEnd = 0) and nothing to straddle; for 44016 / 44032 a straddling keypoint's descriptor must also DIFFER
    from the scalar model's, or flooring the wrong columns would go unseen."""
    for lanes, variant in ((16, 44016), (32, 44032)):
        n_straddle = n_differ = 0
        for w in dc.STRIP_WIDTHS:
            for sc in dc.strip_group(w):
                X, _ = dc.keys_per_level(oracle, sc)[0]
                st = dc.straddles_body_end(sc.geom[0], X, lanes)
                d_body, d_scalar = dc.oracle_run(oracle, sc, (0, 0), variant)[2], dc.oracle_run(oracle, sc, (0, 0), 440)[2]
                n_straddle += int(st.sum())
                n_differ += int(((d_body[:len(X)] != d_scalar[:len(X)]).any(1) & st).sum())
        print(variant, "straddling", n_straddle, "of them with another descriptor than 440", n_differ)
        assert n_straddle >= 20 and n_differ >= 10, (variant, n_straddle, n_differ)
    assert not dc.straddles_body_end(dc.geometry(192, dc.STRIP_H, 3)[0], np.arange(19, 173), 16).any()   # w = bodyEnd: none at 192


# -------------------------------------------------------------------------------------------------- the batches, the plan
def test_batch_sizes_give_every_nk_and_the_remap_both_ways():
    nks = [_plan(dc.batch_scenes(g, n)[0], n)[0] for g, n in dc.BATCHES]
    print(list(zip(dc.BATCHES, nks)))
    assert sorted(nks) == [1, 2, 3, 4, 5, 6, 7, 8]
    big = [n for _, n in dc.BATCHES if n >= 8]
    assert any(n % 8 == 0 for n in big) and any(n % 8 for n in big)        # the XCD remap with and without images past `full`
    for g, n in dc.BATCHES:
        assert len({(s.w, s.h, s.nlevels) for s in dc.batch_scenes(g, n)}) == 1


def test_every_batch_lets_a_wave_meet_every_step(oracle):
    for g, n in dc.BATCHES:
        scenes = dc.batch_scenes(g, n)
        nk = _plan(scenes[0], n)[0]
        steps = dc.wave_steps(oracle, scenes, nk)
        print(g, n, "nk", nk, steps)
        if nk >= 2:
            assert all(v >= 1 for v in steps.values()), (g, n, nk, steps)


def test_plan_tap_layout_and_exact_division(oracle):
    """taskOff is the running sum of ceil(selCap / nk) with selCap = the level's quota + 36 (orbx_api.hip: build_geom), tasks its
    total; magic, when nonzero, is an exact divider: umulhi(j, magic) == j / tasks for EVERY j < n_images * tasks -- brute force
    over the test geometries for every batch size up to 64."""
    geoms = sorted({(s.w, s.h, s.nlevels) for s in dc.all_scenes()} | {(640, 480, 8), (1280, 720, 8)})
    remapped = 0
    for w, h, nl in geoms:
        for nf in (dc.NFEATURES,) if nl == 3 else (1000, 1500):
            quota = oracle.OracleExtractor(nf, dc.SCALE, nl, dc.INI_TH, dc.MIN_TH).tables()["nfeat"]
            sel_img = int(quota.sum()) + 36 * nl
            for n in range(1, 65):
                nk, tasks, magic, off = orbx.describe_plan(nf, dc.SCALE, nl, dc.INI_TH, dc.MIN_TH, w, h, n)
                assert 1 <= nk <= 8 and nk == min(8, max(1, n * sel_img // 12288)), (w, h, nf, n, nk)
                per = [-(-(int(q) + 36) // nk) for q in quota]
                assert off.tolist() == np.concatenate([[0], np.cumsum(per)[:-1]]).tolist() and tasks == sum(per)
                if magic:
                    j = np.arange(n * tasks, dtype=np.uint64)
                    assert np.array_equal((j * np.uint64(magic)) >> np.uint64(32), j // np.uint64(tasks)), (w, h, nf, n)
                    remapped += 1
    assert remapped > 100
    full = np.zeros(3 + 12, np.int32)
    prm = orbx._Params(dc.NFEATURES, dc.SCALE, 3, dc.INI_TH, dc.MIN_TH)
    assert orbx.lib().orbx_debug_describe_plan(C.byref(prm), 192, 120, 4, orbx._p(full)) == 0
    assert (full[3 + 3:] == 0x7fffffff).all()                              # past the last level


def test_taps_reject_bad_arguments_before_any_device():
    L = orbx.lib()
    out = np.zeros(15, np.int32)
    prm = orbx._Params(dc.NFEATURES, dc.SCALE, 3, dc.INI_TH, dc.MIN_TH)
    for args in ((None, 192, 120, 4, orbx._p(out)), (C.byref(prm), 192, 120, 4, None), (C.byref(prm), 0, 120, 4, orbx._p(out)),
                 (C.byref(prm), 192, 120, 0, orbx._p(out))):
        assert L.orbx_debug_describe_plan(*args) == orbx.E_BADARG
    with pytest.raises(orbx.OrbxError):
        orbx.describe_plan(dc.NFEATURES, dc.SCALE, 3, dc.INI_TH, dc.MIN_TH, 96, 72, 4)      # level 1 smaller than one FAST cell
    y = np.ones(4, np.float32)
    for args in ((0, None, orbx._p(y), 4, orbx._p(y)), (0, orbx._p(y), None, 4, orbx._p(y)), (0, orbx._p(y), orbx._p(y), 4, None),
                 (0, orbx._p(y), orbx._p(y), -1, orbx._p(y))):
        assert L.orbx_debug_fast_atan2(*args) == orbx.E_BADARG
    assert L.orbx_debug_fast_atan2(0, orbx._p(y), orbx._p(y), 0, orbx._p(y)) == 0            # nothing to do: no device needed
    if orbx.device_count() == 0:
        assert L.orbx_debug_fast_atan2(0, orbx._p(y), orbx._p(y), 4, orbx._p(y.copy())) == orbx.E_NODEVICE
        assert L.orbx_debug_sincos(0, orbx._p(y), 4, 2, orbx._p(y.copy()), orbx._p(y.copy())) == orbx.E_NODEVICE
