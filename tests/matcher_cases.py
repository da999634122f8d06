"""Crafted inputs for the matchers' window walks and rotation histograms (csrc/orbx_matching.h), beside stereo_cases.py: extractor output never
puts more than a handful of keypoints into a grid column of a search window, and never lands a rotation difference on a bin edge or
two histogram bins on a tie, so the paths below need built keypoints.  Everything is 640 x 480 (64 x 48 cells of 10 x 10 px) and a
few hundred keypoints at most.  No GPU is touched here; tests/test_matcher_walks.py runs the entries on these inputs.
"""
import numpy as np

import orb_slam3_fast_amd as orbx

W, H = 640, 480
BOUNDS = (0.0, 0.0, float(W), float(H))
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
COLUMN_X, COLUMN_Y = 300.0, 240.0   # centre of the crowded column (cell column 30: PosInGrid rounds x / 10 to the nearest cell)


def _flip(desc, rng, p=0.03):
    return desc ^ np.packbits(rng.random(desc.shape + (8,)) < p, axis=-1).reshape(desc.shape)


def column_frame(seed=0):
    """F2: 150 level-0 keypoints whose x lies inside the one cell column 30 (296 .. 304) and whose y spreads over 141 .. 339, so
    the CSR range of that column inside a window of radius 100 around (300, 240) holds all 150 -- three 64-item trips of the wave
    walk, ten 16-item trips of Fuse's -- plus 48 keypoints elsewhere: 16 in the neighbouring columns on levels 0 - 3, 16 in the
    top-left corner, 16 anywhere.  Five of the column's keypoints share one position to within a pixel and one descriptor (Fuse's
    first-minimum rule then decides by the position in the walk, past the first 64 items).  Shuffled, so that the in-cell order
    is the grid's doing.  Returns (kps, desc, indices of the five twins)."""
    rng = np.random.default_rng(seed)
    n = 198
    k = np.zeros(n, orbx.KP_DTYPE)
    k["x"][:150], k["y"][:150] = rng.uniform(296.0, 304.0, 150), rng.uniform(141.0, 339.0, 150)
    k["x"][145:150], k["y"][145:150] = 300.0 + rng.uniform(-0.5, 0.5, 5), 240.0 + rng.uniform(-0.5, 0.5, 5)
    k["x"][150:166], k["y"][150:166] = rng.uniform(280.0, 320.0, 16), rng.uniform(200.0, 280.0, 16)
    k["octave"][150:166] = rng.integers(0, 4, 16)
    k["x"][166:182], k["y"][166:182] = rng.uniform(2.0, 40.0, 16), rng.uniform(2.0, 40.0, 16)
    k["octave"][166:182] = rng.integers(0, 2, 16)
    k["x"][182:], k["y"][182:] = rng.uniform(0.0, W, 16), rng.uniform(0.0, H, 16)
    k["octave"][182:] = rng.integers(0, 8, 16)
    k["angle"] = rng.uniform(0.0, 360.0, n).astype(np.float32)
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d[145:150] = d[145]
    perm = rng.permutation(n)
    k, d = k[perm], d[perm]
    twins = np.nonzero(np.isin(perm, np.arange(145, 150)))[0]
    return k, d, twins


def query_centres(n, seed=1):
    """n query centres: most on the crowded column, then one whose window of radius 100 hangs over the left and top edge, one
    wholly left of / above the bounds and one wholly right of them (no cell: GetFeaturesInArea returns at once)."""
    rng = np.random.default_rng(seed)
    c = np.stack([COLUMN_X + rng.uniform(-3.0, 3.0, n), COLUMN_Y + rng.uniform(-6.0, 6.0, n)], 1).astype(np.float32)
    c[0] = (COLUMN_X, COLUMN_Y)
    c[-3] = (20.0, 15.0)
    c[-2] = (-200.0, -200.0)
    c[-1] = (900.0, 240.0)
    return c


def area_queries():
    q = [(COLUMN_X, COLUMN_Y, 100.0, -1, -1), (COLUMN_X, COLUMN_Y, 100.0, 0, 0), (COLUMN_X, COLUMN_Y, 60.0, 1, 3),
         (303.0, 200.0, 100.0, 0, -1), (20.0, 15.0, 100.0, -1, -1), (-200.0, -200.0, 100.0, -1, -1), (900.0, 240.0, 50.0, -1, -1),
         (300.0, -50.0, 200.0, -1, -1)]
    return np.array(q, np.float32)


def init_case(k2, d2, seed=2):
    """F1 of SearchForInitialization (window 100) on column_frame: 36 keypoints, 32 of them level 0 with vbPrevMatched on the
    crowded column and the descriptor of a column keypoint with a few bits flipped (several F1 keypoints want the same F2 keypoint:
    the stealing rule runs), one level 1 (skipped), and the three edge centres of query_centres."""
    rng = np.random.default_rng(seed)
    n1 = 36
    prev = query_centres(n1, seed)
    k1 = np.zeros(n1, orbx.KP_DTYPE)
    k1["x"], k1["y"] = prev[:, 0], prev[:, 1]
    k1["angle"] = rng.uniform(0.0, 360.0, n1).astype(np.float32)
    k1["octave"][5] = 1
    k1["size"], k1["response"], k1["class_id"] = 31.0, 50.0, -1
    col = np.nonzero((k2["x"] > 295.0) & (k2["x"] < 305.0) & (k2["octave"] == 0))[0]
    src = col[rng.integers(0, 24, n1)]
    d1 = _flip(d2[src], rng)
    corner = np.nonzero((k2["x"] < 40.0) & (k2["y"] < 40.0) & (k2["octave"] == 0))[0]
    d1[-3] = d2[corner[0]]
    return k1, d1, prev


def projection_points(k2, d2, seed=3):
    """The same centres as SearchByProjection inputs: MP_DTYPE map points (radius 4 * th * scale[0] = 100 with th = 25, levels -1 .. 0)
    and PP_DTYPE last-frame points (radius 100, level windows of all three forms), FP_DTYPE Fuse points, and a uRight array for
    the frame (a third monocular, the others spread so that the stereo-consistency gate cuts some candidates)."""
    rng = np.random.default_rng(seed)
    n = 40
    c = query_centres(n, seed)
    col = np.nonzero((k2["x"] > 295.0) & (k2["x"] < 305.0) & (k2["octave"] == 0))[0]
    desc = _flip(d2[col[rng.integers(0, 24, n)]], rng)
    mps = np.zeros(n, orbx.MP_DTYPE)
    mps["proj_x"], mps["proj_y"] = c[:, 0], c[:, 1]
    mps["proj_xr"] = c[:, 0] - 40.0
    mps["view_cos"], mps["track_depth"] = 0.9, 5.0
    mps["predicted_level"] = np.where(np.arange(n) % 5 == 4, 1, 0)
    mps["in_view"], mps["has_observations"] = 1, np.arange(n) % 3 != 0
    mps["desc"] = desc
    pts = np.zeros(n, orbx.PP_DTYPE)
    pts["u"], pts["v"], pts["ur"], pts["radius"] = c[:, 0], c[:, 1], c[:, 0] - 40.0, 100.0
    pts["angle"] = rng.uniform(0.0, 360.0, n).astype(np.float32)
    pts["min_level"] = np.array([-1, 0, 0])[np.arange(n) % 3]
    pts["max_level"] = np.array([1, -1, 0])[np.arange(n) % 3]
    pts["valid"], pts["has_observations"], pts["desc"] = 1, np.arange(n) % 4 != 0, desc
    fp = np.zeros(n, orbx.FP_DTYPE)
    fp["u"], fp["v"], fp["ur"], fp["radius"] = c[:, 0], c[:, 1], c[:, 0] - 40.0, 100.0
    fp["predicted_level"] = np.where(np.arange(n) % 5 == 4, 1, 0)
    fp["valid"], fp["desc"] = 1, desc
    uR = np.where(rng.random(len(k2)) < 0.33, -1.0, k2["x"] - rng.uniform(0.0, 260.0, len(k2))).astype(np.float32)
    return mps, pts, fp, uR


def fuse_twins(fp, k2, d2, twins):
    """Fuse point 0 sits on the five twin keypoints with their descriptor: five candidates of distance 0 inside the chi-square gate."""
    fp = fp.copy()
    fp["u"][0], fp["v"][0], fp["desc"][0] = 300.0, 240.0, d2[twins[0]]
    fp["ur"][0] = -1.0
    return fp


# ---- rotation bins and histogram ties -------------------------------------------------------------------------------------------
def rot_bin(a1, a2):
    """The reference's bin of a match in float32: rot = a1 - a2 (+ 360 when negative), round(rot * (1.0f / 30)), 30 -> 0."""
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    v = np.float32(rot * (np.float32(1.0) / np.float32(30.0)))
    b = int(np.floor(np.abs(v) + np.float32(0.5)) * np.sign(v))   # roundf: halves away from zero
    return 0 if b == 30 else b


# (angle1, angle2) on the edges: rot exactly 0; -0.0; 15 = half-way between bins 0 and 1; the largest float below 360; negative
# before the + 360; 345 = half-way between bins 11 and 12, reached through the + 360
EDGE_PAIRS = [(0.0, 0.0), (-0.0, 0.0), (45.0, 30.0), (float(np.nextafter(np.float32(360.0), np.float32(0.0))), 0.0), (10.0, 350.0),
              (200.0, 215.0)]
# bin counts (the six EDGE_PAIRS add 2 each to bins 0, 1 and 12, below every cut used here except in "three_equal"): the strict '>'
# keeps the first of two equal bins as the maximum; with max1 = 40 the cut 0.1f * max1 is 4.0f, so max2 / max3 sit exactly at it
# (4: kept), just below (3: cut) and just above (5: kept)
HISTOGRAMS = {
    "tie_for_max": {5: 40, 9: 40, 3: 4, 7: 1},
    "second_and_third_at_the_cut": {5: 40, 9: 4, 3: 4, 7: 4},
    "second_below_the_cut": {5: 40, 9: 3, 3: 1},
    "second_above_third_below": {5: 40, 9: 5, 3: 3},
    "three_equal": {2: 4, 6: 4, 10: 4, 11: 4},
}
# what ComputeThreeMaxima must leave of each: (ind1, ind2, ind3) by the scan in bin order, -1 = cut
KEPT = {
    "tie_for_max": (5, 9, 3),                    # bin 9 equals bin 5 and comes later: second; bin 3 exactly at the cut stays
    "second_and_third_at_the_cut": (5, 3, 7),    # three bins of 4: the first two in bin order; bin 9 is culled
    "second_below_the_cut": (5, -1, -1),         # max2 = 3 < 4.0f: second and third both cut
    "second_above_third_below": (5, 9, -1),      # max2 = 5 stays, max3 = 3 < 4.0f is cut
    "three_equal": (2, 6, 10),                   # four bins of 4: the first three in bin order
}


def bin_pairs(hist, seed=4):
    """Matched pairs (angle1, angle2) whose bins have the counts of hist plus the six EDGE_PAIRS (bins 0, 0, 1, 12, 1, 12): a pair of
    bin b is (30 b + a2, a2) with a2 a multiple of 0.5 below 20, for which 30 b + a2 - a2 is exact.  Shuffled."""
    rng = np.random.default_rng(seed)
    pairs = list(EDGE_PAIRS)
    for b, cnt in hist.items():
        for _ in range(cnt):
            a2 = 0.5 * rng.integers(0, 40)
            pairs.append((30.0 * b + a2, a2))
    pairs = np.array(pairs, np.float32)
    return pairs[rng.permutation(len(pairs))]


def pair_frames(pairs, seed=5):
    """Two keypoint sets of len(pairs) level-0 keypoints on a 16 px lattice (nobody is in anybody else's window of 10 px), pair i at
    the same place in both with angles pairs[i] and ONE descriptor, distinct between pairs: every pair matches at distance 0."""
    rng = np.random.default_rng(seed)
    n = len(pairs)
    k1 = np.zeros(n, orbx.KP_DTYPE)
    k1["x"], k1["y"] = 24.0 + 16.0 * (np.arange(n) % 36), 24.0 + 16.0 * (np.arange(n) // 36)
    k1["size"], k1["response"], k1["class_id"] = 31.0, 50.0, -1
    k2 = k1.copy()
    k1["angle"], k2["angle"] = pairs[:, 0], pairs[:, 1]
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return k1, k2, d


def pair_feature_vectors(n, nodes=4, seed=6):
    """Feature vectors (node ids, node start, feature indices) that put pair i into node i % nodes on both sides, the second side in
    another order inside the node."""
    rng = np.random.default_rng(seed)
    ids = np.array([11, 12, 40, 77][:nodes], np.uint32)
    lists1 = [np.nonzero(np.arange(n) % nodes == j)[0] for j in range(nodes)]
    lists2 = [rng.permutation(l) for l in lists1]
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists1])]).astype(np.int32)
    return (ids, start, np.concatenate(lists1).astype(np.uint32)), (ids, start, np.concatenate(lists2).astype(np.uint32))
