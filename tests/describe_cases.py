"""Scenes and the census for k_describe (csrc/orbx_describe.hip): which of its three window loaders a keypoint takes, at which
misalignment, over which reflected sides, and what follows what inside a wave.

The restatement below is the kernel's own classification (the `win` lambda): for a level (w, h, pitch, level) and a key (X, Y)

    xs = (X - 21) & ~3, mis = (X - 21) - xs, interior = 21 <= X < w - 21 and 21 <= Y < h - 21,
    rowValid = w at level 0 (the caller's rows), pitch above (pitch = align_up(w, 64)),
    path = dma when interior and xs + 48 <= rowValid, rowend when interior otherwise, reflect when not interior.

enumerate_reachable walks every admissible key of a geometry (19 <= X <= w - 20, 19 <= Y <= h - 20: FAST runs 16 px inside a
level and its circle has radius 3); the census tests take the cells they require from it, never from what a scene produced.

Everything here is CPU work on the oracle; every distinct (scene, lapping area, blur variant) goes through it once per process.
"""
import numpy as np

NFEATURES, SCALE, INI_TH, MIN_TH = 4000, 1.2, 20, 7
PATHS = ("dma", "rowend", "reflect")
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8
TINY_DEG = float(np.degrees(2.0 ** -12))     # glibc sinf / cosf: |y| < 2^-12 rad returns (y, 1): 0.013988 degrees


def level_dims(w, h, nlevels, sf=SCALE):
    """ComputePyramid's level sizes (src/ORBextractor.cc:1111-1113): cvRound(size * mvInvScaleFactor[l]) in float."""
    scale = [np.float32(1)]
    for _ in range(1, nlevels):
        scale.append(np.float32(scale[-1] * np.float32(sf)))
    return [(int(np.rint(np.float64(np.float32(w) * (np.float32(1) / s)))), int(np.rint(np.float64(np.float32(h) * (np.float32(1) / s)))))
            for s in scale]


def geometry(w, h, nlevels):
    """[(w, h, pitch, level)] of a frame: the pitch of the handle's pyramid is align_up(w, 64)."""
    return [(lw, lh, (lw + 63) // 64 * 64, l) for l, (lw, lh) in enumerate(level_dims(w, h, nlevels))]


def classify(geom, X, Y):
    """(path index into PATHS, mis, mask of reflected sides) of keys (X, Y) (arrays) at the level geometry (w, h, pitch, level)."""
    w, h, pitch, level = geom
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    xs = (X - 21) & ~3
    mis = (X - 21) - xs
    sides = (X < 21) * LEFT + (Y < 21) * TOP + (X + 21 >= w) * RIGHT + (Y + 21 >= h) * BOTTOM
    interior = sides == 0
    row_valid = pitch if level else w
    dma = interior & (xs + 48 <= row_valid)
    path = np.where(dma, 0, np.where(interior, 1, 2))
    return path, mis, sides


def enumerate_reachable(geom):
    """Every (path, mis) pair and every nonzero mask of reflected sides that SOME admissible key of this geometry has."""
    w, h = geom[0], geom[1]
    Y, X = np.meshgrid(np.arange(19, h - 19), np.arange(19, w - 19), indexing="ij")
    path, mis, sides = classify(geom, X.ravel(), Y.ravel())
    cells = {(PATHS[p], int(m)) for p, m in set(zip(path.tolist(), mis.tolist()))}
    return cells, {int(s) for s in set(sides.tolist()) if s}


def level_class(level):
    return 0 if level == 0 else 1     # level 0 reads the caller's rows (rowValid = w), the levels above the handle's pyramid


# ---------------------------------------------------------------------------------------------------------------- scenes
class Scene:
    def __init__(self, name, img, nlevels):
        self.name, self.img, self.nlevels = name, np.ascontiguousarray(img, np.uint8), nlevels
        self.h, self.w = self.img.shape
        self.geom = geometry(self.w, self.h, nlevels)


def _noise(rng, h, w):
    """2x2-block noise of 40 / 200: dense FAST corners on block corners."""
    b = np.where(rng.random(((h + 1) // 2, (w + 1) // 2)) < 0.5, 40, 200).astype(np.uint8)
    return np.kron(b, np.ones((2, 2), np.uint8))[:h, :w]


def strip_scene(w, h=120, seed=None):
    """Flat 128 with noise in the last 48 columns: the keypoints crowd the band left of w - 21 where a window's 48-byte rows end
    past the image row, and the reflected columns right of it."""
    seed = w if seed is None else seed
    img = np.full((h, w), 128, np.uint8)
    img[:, w - 48:] = _noise(np.random.default_rng(seed), h, 48)
    return Scene("strip%d_s%d" % (w, seed), img, 3)


def _blob(img, cx, cy, centre=240, body=200):
    img[cy - 1:cy + 2, cx - 1:cx + 2] = body
    img[cy, cx] = centre     # a flat-topped blob has no strict maximum of the FAST score: the centre stays brighter


def frame_scene(w, h, seed):
    """Noise in a 40 px band along all four borders, flat inside; a blob on a flat pad at each of the four keys nearest a
    corner that FAST can return, (19 | w - 20, 19 | h - 20), whose windows reflect over two sides."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128, np.uint8)
    n = _noise(rng, h, w)
    for ys, xs in ((slice(0, 40), slice(None)), (slice(h - 40, h), slice(None)), (slice(None), slice(0, 40)), (slice(None), slice(w - 40, w))):
        img[ys, xs] = n[ys, xs]
    for cx in (19 + seed % 2, w - 20 - seed % 2):
        for cy in (19 + (seed // 2) % 2, h - 20 - (seed // 2) % 2):
            img[max(cy - 8, 0):cy + 9, max(cx - 8, 0):cx + 9] = 100
            _blob(img, cx, cy)
    return Scene("frame%dx%d_s%d" % (w, h, seed), img, 3)


# marker offset -> IC_Angle of the blob centre (fastAtan2 of the integer moments, degrees); None: a range, see TINY_BLOBS
BLOB_ANGLES = [((0, 0), 0.0), ((10, 0), 0.0), ((-10, 0), 180.0), ((0, 10), 90.0), ((0, -10), 270.0),
               ((10, 10), 44.990456), ((-10, 10), 135.00955), ((-10, -10), 224.99045), ((10, -10), 315.00955)]
TINY_BLOBS = [+1, -1, +1, -1]     # the pixel (0, dy) of the blob raised by 1: m01 = dy against an m10 in the thousands


def blob_scene(w, h):
    """Flat 100; 3x3 blobs (200, centre 240), each with a 3x3 marker of 150 at an offset inside the radius-15 patch, so that the
    moments are exact multiples of each other: angles ON the axes and ON the diagonals, where fast_atan2_sel's selects decide.
    The tiny blobs carry a strong marker (250) on the +x axis and one pixel raised by 1 above or below the centre: m01 = +-1,
    an angle under 2^-12 rad (the `tiny` select of glibc_sincosf_sel) and its mirror just under 360.
    Returns (scene, [(cx, cy, expected angle or None)], [(cx, cy, dy)])."""
    img = np.full((h, w), 100, np.uint8)
    spots = [(40 + 56 * i + 3 * (j % 4), 40 + 56 * j) for j in range((h - 80) // 56 + 1) for i in range((w - 80) // 56 + 1)]
    exact, tiny = [], []
    for (dx, dy), ang in BLOB_ANGLES:
        cx, cy = spots.pop(0)
        img[cy + dy - 1:cy + dy + 2, cx + dx - 1:cx + dx + 2] = 150
        _blob(img, cx, cy)
        exact.append((cx, cy, ang))
    for k, dy in enumerate(TINY_BLOBS):
        cx, cy = spots.pop(0)
        off = 9 + k     # different m10 per blob
        img[cy - 1:cy + 2, cx + off - 1:cx + off + 2] = 250
        _blob(img, cx, cy)
        img[cy + dy, cx] += 1
        tiny.append((cx, cy, dy))
    return Scene("blobs%dx%d" % (w, h), img, 3), exact, tiny


def flat_scene(w, h, nlevels):
    return Scene("flat%dx%d" % (w, h), np.full((h, w), 100, np.uint8), nlevels)


def dots_scene(w, h, nlevels, count):
    """`count` single pixels of 108 on flat 100, 12 px apart: 8 over the ring passes minThFAST = 7 at level 0 only -- the first
    resize spreads a pixel with weights of at most 0.9 * 0.9 -- so every keypoint lies on level 0 and their number is `count`:
    a level whose count is a multiple of every nk that divides `count`."""
    img = np.full((h, w), 100, np.uint8)
    pos = [(x, y) for y in range(22, h - 21, 12) for x in range(22, w - 21, 12)]
    assert len(pos) >= count, (w, h, count, len(pos))
    for x, y in pos[:count]:
        img[y, x] = 108
    return Scene("dots%dx%d_%d" % (w, h, count), img, nlevels)


# ------------------------------------------------------------------------------------------------------------ the scene set
STRIP_H = 120
STRIP_WIDTHS = (192, 193, 194, 195, 230, 231)      # every w mod 4 at level 0; 230 / 231: level 1 is 192 wide = its pitch
STRIP_SEEDS = (0, 1, 2)                             # added to the width
BIG_W, BIG_H = 418, 300
DOTS_STRIP, DOTS_BIG = 60, 672                      # multiples of every nk up to 6 / of 7 and 8
_scenes = {}


def strip_group(w):
    """The scenes of one strip width, cycled through a batch: its seeded strips and a dots frame."""
    key = ("strip", w)
    if key not in _scenes:
        _scenes[key] = [strip_scene(w, STRIP_H, w + 1000 * s) for s in STRIP_SEEDS] + [dots_scene(w, STRIP_H, 3, DOTS_STRIP)]
    return _scenes[key]


def big_group():
    """The 418 x 300 scenes, three levels: frames textured to the borders and corners, the blobs, the dots, the flat frame."""
    if "big" not in _scenes:
        blobs, exact, tiny = blob_scene(BIG_W, BIG_H)
        _scenes["big"] = ([frame_scene(BIG_W, BIG_H, s) for s in range(4)] + [blobs, dots_scene(BIG_W, BIG_H, 3, DOTS_BIG),
                          flat_scene(BIG_W, BIG_H, 3)], exact, tiny)
    return _scenes["big"][0]


def blob_expectations():
    big_group()
    return _scenes["big"][1], _scenes["big"][2]


def all_scenes():
    return [s for w in STRIP_WIDTHS for s in strip_group(w)] + big_group()


# batches of the GPU tests: (group key, frames); the frames cycle through the group's scenes.  k_describe walks
# nk = min(8, max(1, frames * selImg / 12288)) keypoints per wave, selImg = nfeatures + 36 * nlevels: test_describe_census takes
# the nk of every batch from the plan tap and requires 1 .. 8 to appear.  16 is a multiple of 8, 19 / 22 / 25 are not: the XCD
# remap covers the first (frames / 8) * 8 images only.
BATCHES = [(192, 4), (193, 7), (194, 10), (195, 13), (230, 16), (231, 19), ("big", 22), ("big", 25)]


def batch_scenes(group, frames):
    sc = big_group() if group == "big" else strip_group(group)
    return [sc[i % len(sc)] for i in range(frames)]


def lap_of(scene):
    """A lapping area (vLappingArea of operator(), src/ORBextractor.cc:1086-1098) that splits the scene's keypoints."""
    return (scene.w - 40, scene.w - 26) if scene.name.startswith("strip") else (scene.w // 3, scene.w // 2)


# ------------------------------------------------------------------------------------------------------------ oracle runs
_runs = {}


def oracle_run(oracle, scene, lap=(0, 0), variant=451):
    """(mono, keypoints, descriptors) of the oracle for this scene; computed once, returned read-only."""
    key = (scene.name, tuple(lap), variant)
    if key not in _runs:
        oe = oracle.OracleExtractor(NFEATURES, SCALE, scene.nlevels, INI_TH, MIN_TH)
        if variant != 451:
            oe.set_blur_taps(variant)
        mono, k, d = oe.extract(scene.img, tuple(lap))
        k.setflags(write=False)
        d.setflags(write=False)
        _runs[key] = (mono, k, d, oe.tables()["scale"].copy())
    return _runs[key][:3]


def keys_per_level(oracle, scene):
    """Per level the keys (X, Y) in the oracle's order without a lapping area -- the order of k_describe's selected slots."""
    mono, k, _ = oracle_run(oracle, scene)
    scale = _runs[(scene.name, (0, 0), 451)][3]
    out = []
    for l in range(scene.nlevels):
        m = k["octave"] == l
        s = np.float64(scale[l])
        out.append((np.rint(k["x"][m] / s).astype(np.int64), np.rint(k["y"][m] / s).astype(np.int64)))
    assert mono < 0 or sum(len(x) for x, _ in out) == len(k)
    if len(k):
        assert (np.diff(k["octave"]) >= 0).all()      # level after level: the slot of a keypoint is (earlier levels) + its index
    return out


def census(oracle, scene):
    """{(level class, path, mis): count}, {side mask: count} of the scene's keypoints."""
    cells, sides = {}, {}
    for geom, (X, Y) in zip(scene.geom, keys_per_level(oracle, scene)):
        if len(X):
            assert X.min() >= 19 and X.max() <= geom[0] - 20 and Y.min() >= 19 and Y.max() <= geom[1] - 20, scene.name
        p, m, s = classify(geom, X, Y)
        for pi, mi, si in zip(p.tolist(), m.tolist(), s.tolist()):
            c = (level_class(geom[3]), PATHS[pi], mi)
            cells[c] = cells.get(c, 0) + 1
            if si:
                sides[si] = sides.get(si, 0) + 1
    return cells, sides


def required(scenes):
    """The cells and side masks enumerate_reachable lists over the level geometries of these scenes."""
    cells, sides, seen = set(), set(), set()
    for sc in scenes:
        for geom in sc.geom:
            if geom in seen:
                continue
            seen.add(geom)
            c, s = enumerate_reachable(geom)
            cells |= {(level_class(geom[3]), p, m) for p, m in c}
            sides |= s
    return cells, sides


def wave_steps(oracle, scenes, nk):
    """What the waves of a batch of these scenes meet when each walks nk consecutive keypoints of one (image, level):
    counts of tasks with a dma -> non-dma step, a non-dma -> dma step, reflect and rowend as neighbours, tail tasks (fewer than nk
    keypoints) and levels whose count is a positive multiple of nk."""
    out = dict(dma_to_other=0, other_to_dma=0, reflect_rowend=0, tail=0, multiple=0)
    for sc in {s.name: s for s in scenes}.values():
        for geom, (X, Y) in zip(sc.geom, keys_per_level(oracle, sc)):
            n = len(X)
            if n == 0:
                continue
            out["multiple"] += n % nk == 0
            out["tail"] += n % nk != 0
            p = classify(geom, X, Y)[0]
            for t0 in range(0, n, nk):
                a, b = p[t0:min(t0 + nk, n) - 1], p[t0 + 1:min(t0 + nk, n)]
                out["dma_to_other"] += bool(((a == 0) & (b != 0)).any())
                out["other_to_dma"] += bool(((a != 0) & (b == 0)).any())
                out["reflect_rowend"] += bool((((a == 1) & (b == 2)) | ((a == 2) & (b == 1))).any())
    return out


def straddles_body_end(geom, X, lanes):
    """Keys whose 37 blurred patch columns X - 18 .. X + 18 lie on both sides of bodyEnd = w & ~(lanes - 1), the column where
    OpenCV 4.0 .. 4.5.0's vertical pass changes from its flooring vector body to the rounding scalar tail."""
    body_end = geom[0] & ~(lanes - 1)
    return (X - 18 < body_end) & (body_end <= X + 18)
