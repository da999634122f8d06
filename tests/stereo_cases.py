"""Crafted keypoint sets for Frame::ComputeStereoMatches (src/Frame.cc:921-1084): a helper module, not a conftest.

compute_stereo_matches_py is the literal Python / numpy float32 restatement of the routine (checked bit for bit against the
C++ oracle in tests/test_oracle_stereo.py); with diag=True it also reports, per left keypoint, which statement decided its fate
(OUTCOMES), the SAD before the median cut, bestinc, deltaR and the right keypoint the descriptor scan chose.

The gate `deltaR < -1 || deltaR > 1` (:1050) is dead code and no case tries to reach it.  bestinc is the FIRST strict minimum
of the eleven SADs and not an end of the scan (:1041), so d1 > d2 (strictly: the scan would have stopped at d1 otherwise) and
d3 >= d2.  With a = d1 - d2 > 0 and b = d3 - d2 >= 0, deltaR = (d1 - d3) / (2 (d1 + d3 - 2 d2)) = (a - b) / (2 (a + b)): the
denominator is positive, so deltaR is never NaN, and |a - b| <= a + b puts it into [-0.5, 0.5].  (SADs are integers below
2^15 and their sums below 2^17, exact in float32; the one rounded operation is the final division, which is monotone and
cannot leave the interval.)  Should the restatement ever reach the gate it reports the code "deltaR_gate", which no case expects.

The case builders return (L, R, kL, dL, kR, dR, bf, b, expected): two uint8 images, the keypoints and descriptors of both
eyes, the camera (bf / b = 100 = maxD) and expected = {left index: (allowed outcome codes, right index the descriptor scan
must choose or None)}.  Images are uniform noise in 20 .. 235 with R[y, x] = L[y, x + d] per horizontal stripe; keypoints are
placed freely (the association never asks whether they are FAST corners); descriptors are seeded random 256-bit strings, a
partner at Hamming distance k has the first k bits flipped.  An exact SAD at level 0 is made by changing pixels of the right
window at the true shift.  Every window the reference reads stays inside its pyramid level (check_reads_in_bounds): the
reference would read outside the image otherwise, and the right keypoint at (0, 0) (maxr = -1) is left out for the same reason.
"""
import math

import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])

OUTCOMES = ("no_candidate", "hamming_ge_75", "window_guard", "bestinc_edge", "disp_negative", "disp_ge_maxD", "accepted",
            "accepted_disp0", "cut_by_median")
PASSED = ("accepted", "accepted_disp0", "cut_by_median")  # a partner below thOrbDist that every gate of the refinement let through


def c_round(v):  # C round(): halves away from zero, on a float32 value
    v = float(v)
    return f32(math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _as_ints(d):  # descriptors as Python integers: hamming(a, b) == (a ^ b).bit_count()
    return [int.from_bytes(np.ascontiguousarray(r).tobytes(), "little") for r in d]


def compute_stereo_matches_py(pyrL, pyrR, kL, dL, kR, dR, scale, inv_scale, mbf, mb, diag=False):
    N = len(kL)
    uRight, depth = np.full(N, -1.0, f32), np.full(N, -1.0, f32)
    outcome = ["no_candidate"] * N
    sadOut, incOut, iROut = np.full(N, -1, np.int64), np.full(N, 99, np.int64), np.full(N, -1, np.int64)
    deltaOut = np.full(N, np.nan, f32)
    distOut, tieOut = np.full(N, -1, np.int64), np.zeros(N, np.int64)
    iL_bits, iR_bits = _as_ints(dL), _as_ints(dR)
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyrL[0].shape[0]
    rows = [[] for _ in range(nRows)]
    for iR in range(len(kR)):
        kpY = f32(kR["y"][iR])
        if kpY == 0.0 and f32(kR["x"][iR]) == 0.0:
            continue
        r = f32(2.0) * scale[kR["octave"][iR]]
        maxr, minr = int(math.ceil(float(kpY + r))), int(math.floor(float(kpY - r)))
        for yi in range(minr, maxr + 1):
            rows[yi].append(iR)
    minZ, minD = f32(mb), f32(0)
    maxD = f32(mbf) / minZ
    vDistIdx = []
    for iL in range(N):
        levelL, vL, uL = int(kL["octave"][iL]), f32(kL["y"][iL]), f32(kL["x"][iL])
        cands = rows[int(vL)]
        if not cands:
            continue
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        for iR in cands:
            if kR["octave"][iR] < levelL - 1 or kR["octave"][iR] > levelL + 1:
                continue
            uR = f32(kR["x"][iR])
            if minU <= uR <= maxU:
                outcome[iL] = "hamming_ge_75"
                dist = (iL_bits[iL] ^ iR_bits[iR]).bit_count()
                if dist == bestDist and dist < TH_HIGH:
                    tieOut[iL] += 1
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
                    tieOut[iL] = 0
        distOut[iL] = bestDist
        if bestDist < thOrbDist:
            iROut[iL] = bestIdxR
            uR0 = f32(kR["x"][bestIdxR])
            sfac = inv_scale[levelL]
            scaleduL, scaledvL, scaleduR0 = c_round(uL * sfac), c_round(vL * sfac), c_round(uR0 * sfac)
            w, L = 5, 5
            imL, imR = pyrL[levelL], pyrR[levelL]
            IL = imL[int(scaledvL) - w:int(scaledvL) + w + 1, int(scaleduL) - w:int(scaleduL) + w + 1].astype(np.int64)
            best, bestinc = 2 ** 31 - 1, 0
            vDists = [f32(0)] * (2 * L + 1)
            iniu, endu = scaleduR0 + f32(L) - f32(w), scaleduR0 + f32(L) + f32(w) + f32(1)
            if iniu < 0 or endu >= imR.shape[1]:
                outcome[iL] = "window_guard"
                continue
            for inc in range(-L, L + 1):
                c0 = int(scaleduR0) + inc - w
                IR = imR[int(scaledvL) - w:int(scaledvL) + w + 1, c0:c0 + 2 * w + 1].astype(np.int64)
                dist = f32(np.abs(IL - IR).sum())
                if dist < f32(best):
                    best, bestinc = int(dist), inc
                vDists[L + inc] = dist
            sadOut[iL], incOut[iL] = best, bestinc
            if bestinc == -L or bestinc == L:
                outcome[iL] = "bestinc_edge"
                continue
            d1, d2, d3 = vDists[L + bestinc - 1], vDists[L + bestinc], vDists[L + bestinc + 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                deltaR = (d1 - d3) / (f32(2.0) * (d1 + d3 - f32(2.0) * d2))
            deltaOut[iL] = deltaR
            if deltaR < -1 or deltaR > 1:  # (0/0 = NaN fails both comparisons, as in C, and is rejected by the disparity test)
                outcome[iL] = "deltaR_gate"
                continue
            bestuR = scale[levelL] * (scaleduR0 + f32(bestinc) + deltaR)
            disparity = uL - bestuR
            if disparity >= minD and disparity < maxD:
                outcome[iL] = "accepted"
                if disparity <= 0:
                    outcome[iL] = "accepted_disp0"
                    disparity = f32(0.01)
                    bestuR = f32(float(uL) - 0.01)
                depth[iL] = f32(mbf) / disparity
                uRight[iL] = bestuR
                vDistIdx.append((best, iL))
            else:
                outcome[iL] = "disp_ge_maxD" if disparity >= maxD else "disp_negative"
    median, preCut = None, list(outcome)
    if vDistIdx:
        vDistIdx.sort()
        median = f32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = f32(1.5) * f32(1.4) * median
        for d, i in reversed(vDistIdx):
            if f32(d) < thDist:
                break
            uRight[i] = -1
            depth[i] = -1
            outcome[i] = "cut_by_median"
    if diag:
        return uRight, depth, dict(outcome=outcome, pre_cut=preCut, sad=sadOut, bestinc=incOut, deltaR=deltaOut, iR=iROut,
                                   dist=distOut, ties=tieOut, median=median, matches=len(vDistIdx))
    return uRight, depth


# ------------------------------------------------------------------------------------------------------- case building
W, H = 384, 288
BF, B = f32(50.0), f32(0.5)   # maxD = bf / b = 100 exactly
BALLAST_SAD = 4840            # 40 grey levels on each of the 121 window pixels: median 4840, cut threshold 10164


def tables(scale_factor, nlevels):
    """mvScaleFactor / mvInvScaleFactor as ORBextractor builds them (float32 running product, src/ORBextractor.cc:414-426)."""
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        s[i] = f32(s[i - 1] * f32(scale_factor))
    return s, (f32(1.0) / s).astype(f32)


def level_sizes(w, h, inv_scale):
    """cv::Size(cvRound(cols * inv), cvRound(rows * inv)) per level (cvRound: halves to even)."""
    rnd = lambda v: int(np.rint(f32(v)))
    return [(rnd(f32(w) * s), rnd(f32(h) * s)) for s in inv_scale]


class Scene:
    """Two noise images whose right one is the left one shifted per stripe, and the keypoint lists built on them."""

    def __init__(self, seed, w=W, h=H, pyramid=(1.2, 8), shift=12):
        self.rng = np.random.default_rng(seed)
        self.w, self.h, self.pyramid = w, h, pyramid
        self.scale, self.inv = tables(*pyramid)
        self.sizes = level_sizes(w, h, self.inv)
        self.L = self.rng.integers(20, 236, (h, w), dtype=np.uint8)
        self.R = self.rng.integers(20, 236, (h, w), dtype=np.uint8)
        self.stripe(0, h, shift)
        self.kL, self.dL, self.kR, self.dR, self.expected = [], [], [], [], {}

    # ---- images
    def stripe(self, y0, y1, d):
        """R[y, x] = L[y, x + d] on rows y0 .. y1 - 1 (fresh noise where x + d leaves the row)."""
        self.R[y0:y1] = self.rng.integers(20, 236, (y1 - y0, self.w), dtype=np.uint8)
        if d >= 0:
            self.R[y0:y1, :self.w - d] = self.L[y0:y1, d:]
        else:
            self.R[y0:y1, -d:] = self.L[y0:y1, :self.w + d]

    def set_sad(self, xc, yc, sad, left=None):
        """The 11 x 11 window of R centred at (xc, yc) becomes the left window `left` (default: what is there) with `sad` grey
        levels of absolute difference spread over its pixels."""
        win = self.R[yc - 5:yc + 6, xc - 5:xc + 6]
        base = (win if left is None else left).astype(np.int64).ravel()
        q = np.full(121, sad // 121, np.int64)
        q[:sad % 121] += 1
        win[...] = np.where(base <= 128, base + q, base - q).reshape(11, 11).astype(np.uint8)

    def speckle(self, frac):
        """+1 on a random fraction of R's pixels: windows at their true shift get small positive SADs of different sizes."""
        self.R += (self.rng.random(self.R.shape) < frac).astype(np.uint8)

    # ---- keypoints
    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    @staticmethod
    def flipped(d, k):
        bits = np.unpackbits(d)
        bits[:k] ^= 1
        return np.packbits(bits)

    def left(self, x, y, octave, d, codes=None, iR=None):
        self.kL.append((x, y, octave))
        self.dL.append(d)
        if codes is not None:
            self.expected[len(self.kL) - 1] = ((codes,) if isinstance(codes, str) else tuple(codes), iR)
        return len(self.kL) - 1

    def right(self, x, y, octave, d):
        self.kR.append((x, y, octave))
        self.dR.append(d)
        return len(self.kR) - 1

    def pair(self, uL, v, d, codes, ham=0, sad=None, uR=None, octave=0):
        """A left keypoint at (uL, v), its partner at (uR, v) (default uL - d, d = the stripe's shift) at Hamming distance ham;
        sad: exact SAD at the true shift (level 0, integer coordinates)."""
        dsc = self.desc()
        iR = self.right(uL - d if uR is None else uR, v, octave, self.flipped(dsc, ham))
        if sad is not None:
            self.set_sad(int(uL) - d, int(v), sad)
        return self.left(uL, v, octave, dsc, codes, iR if ham < 75 and codes != "no_candidate" else None), iR

    def ballast(self, n, y0, x0=120, d=12, sad=BALLAST_SAD, codes="accepted", cols=16):
        """n level-0 pairs with the same SAD on a 13-pixel grid from (x0, y0): they fix the median of the case."""
        for i in range(n):
            self.pair(x0 + 13 * (i % cols), y0 + 13 * (i // cols), d, codes, sad=sad)

    # ---- result
    def arrays(self, k):
        a = np.zeros(len(k), KP_DTYPE)
        for i, (x, y, o) in enumerate(k):
            a[i]["x"], a[i]["y"], a[i]["octave"] = x, y, o
            a[i]["size"], a[i]["angle"], a[i]["response"], a[i]["class_id"] = 31.0 * float(self.scale[o]), 0.0, 50.0, -1
        return a

    def finish(self):
        dL = np.array(self.dL, np.uint8).reshape(-1, 32)
        dR = np.array(self.dR, np.uint8).reshape(-1, 32)
        return (self.L, self.R, self.arrays(self.kL), dL, self.arrays(self.kR), dR, BF, B, self.expected)


def check_reads_in_bounds(case, pyramid):
    """Every read of the reference stays inside its image: the row table (right bands inside [0, h)), the left window and,
    for every level a left partner can have, the eleven right windows (the guard at :1023 covers the right end only)."""
    L, R, kL, dL, kR, dR, bf, b, expected = case
    h, w = L.shape
    scale, inv = tables(*pyramid)
    sizes = level_sizes(w, h, inv)
    for k in kR:
        assert not (k["x"] == 0 and k["y"] == 0)
        r = f32(2.0) * scale[k["octave"]]
        assert math.floor(float(f32(k["y"]) - r)) >= 0 and math.ceil(float(f32(k["y"]) + r)) <= h - 1, k
        for l in range(max(k["octave"] - 1, 0), min(k["octave"] + 1, len(scale) - 1) + 1):
            assert c_round(f32(k["x"]) * inv[l]) - 10 >= 0, (k, l)
    for k in kL:
        l = k["octave"]
        su, sv = int(c_round(f32(k["x"]) * inv[l])), int(c_round(f32(k["y"]) * inv[l]))
        assert 0 <= int(k["y"]) < h and su - 5 >= 0 and su + 5 < sizes[l][0] and sv - 5 >= 0 and sv + 5 < sizes[l][1], k


def permuted(case, seed, left=True, right=True):
    """The same case with the left and / or right arrays in another order (expected follows the left permutation)."""
    L, R, kL, dL, kR, dR, bf, b, expected = case
    rng = np.random.default_rng(seed)
    pL = rng.permutation(len(kL)) if left else np.arange(len(kL))
    pR = rng.permutation(len(kR)) if right else np.arange(len(kR))
    invL, invR = np.argsort(pL), np.argsort(pR)
    exp = {int(invL[i]): (c, None if r is None else int(invR[r])) for i, (c, r) in expected.items()}
    return (L, R, kL[pL], dL[pL], kR[pR], dR[pR], bf, b, exp), pL, pR


# ---------------------------------------------------------------------------------------------------------------- cases
def case_gates(pyramid=(1.2, 8), w=W, h=H):
    """Window guard, the disparity bounds, the candidate gate's two ends and the Hamming threshold."""
    s = Scene(101, w, h, pyramid)
    sc = float(s.scale[1])
    s.stripe(16, 48, 4)      # window guard, level 0
    s.stripe(48, 80, 99)     # just below maxD; uR == uL - maxD
    s.stripe(80, 112, 101)   # >= maxD
    s.stripe(112, 144, -3)   # negative disparity
    s.stripe(144, 176, 0)    # disparity 0
    s.stripe(176, 208, 2)    # uR == uL
    s.stripe(224, 260, 6)    # window guard, level 1: 6 pixels are 5 (scale 1.2) or 4 (scale 1.5) level pixels
    # (rows 208 .. 223 and 260 ..: shift 12: Hamming thresholds, equal SAD minima, ballast)
    # -- window guard at level 0: round(uR) + 11 = w - 1 passes, = w is rejected
    s.pair(w - 8, 24, 4, "accepted", sad=10)            # uR = w - 12: endu = w - 1
    s.pair(w - 7, 40, 4, "window_guard", sad=10)        # uR = w - 11: endu = w
    # -- disparity bounds: right keypoint at uL - 98, true shifts 99 and 101
    s.pair(300, 56, 99, "accepted", sad=10, uR=300 - 98)
    s.pair(300, 88, 101, "disp_ge_maxD", sad=10, uR=300 - 98)
    s.pair(200, 120, -3, "disp_negative", sad=10, uR=200)
    # -- disparity exactly 0: a patch mirror-symmetric about the keypoint column, the same in both eyes
    xc, yc = 200, 160
    for t in range(1, 17):
        s.L[yc - 5:yc + 6, xc + t] = s.L[yc - 5:yc + 6, xc - t]
    s.R[yc - 5:yc + 6, xc - 16:xc + 17] = s.L[yc - 5:yc + 6, xc - 16:xc + 17]
    s.pair(xc, yc, 0, "accepted_disp0")
    # -- the candidate gate minU <= uR <= maxU at both ends, fractional uL
    uL = f32(150.3)
    s.pair(uL, 184, 2, "accepted", sad=10, uR=uL)
    s.pair(uL, 200, 2, "no_candidate", uR=np.nextafter(uL, f32(np.inf)))
    uL = f32(250.3)
    minU = f32(uL - f32(100.0))
    s.pair(uL, 64, 99, "accepted", sad=10, uR=minU)
    s.pair(uL, 72, 99, "no_candidate", uR=np.nextafter(minU, f32(-np.inf)))
    # -- thOrbDist = 75 and TH_HIGH = 100
    for i, (ham, code) in enumerate(((74, "accepted"), (75, "hamming_ge_75"), (99, "hamming_ge_75"), (100, "hamming_ge_75"))):
        s.pair(100 + 40 * i, 215, 12, code, ham=ham, sad=10)
    # -- two equal SAD minima: rows constant from column uR - 6 on in R (and around uL in L), unrelated noise to the left.
    #    The first zero SAD is at inc = -1 and the next is zero too: deltaR = +0.5, uRight = uR - 0.5
    rows_ = slice(215 - 5, 215 + 6)
    const = s.rng.integers(20, 236, (11, 1), dtype=np.uint8)
    s.L[rows_, 290:335] = const
    s.R[rows_, 250:292] = s.rng.integers(20, 236, (11, 42), dtype=np.uint8)
    s.R[rows_, 292:335] = const
    s.pair(310, 215, 12, "accepted")
    # -- window guard at level 1 (the level's own width decides)
    w1 = s.sizes[1][0]
    for y, sr, code in ((234, w1 - 12, PASSED), (246, w1 - 11, "window_guard")):
        uR = f32((sr + 0.05) * sc)
        s.pair(f32(uR + 6), y, 6, code, uR=uR, octave=1)
    s.ballast(20, 268, x0=60, cols=20)
    return s.finish()


def case_octave_gate(pyramid=(1.2, 8), w=W, h=H):
    """Partner at levelL +- 1 (distance 40) beside a distance-0 decoy two levels away, at both clamped ends of the pyramid."""
    s = Scene(102, w, h, pyramid)
    n = len(s.scale)
    lo = int(math.ceil(17 * float(s.scale[-1])))          # 16 level pixels from every border at the coarsest level
    slots = [(x, y) for y in range(lo, h - lo - 40, 14) for x in (w - lo - 4, w - lo - 44)]
    k = 0
    for levelL in (0, 1, n - 2, n - 1):
        for sgn in (-1, 1):
            p = levelL + sgn
            if not 0 <= p < n:
                continue
            decoy = levelL + 2 * sgn if 0 <= levelL + 2 * sgn < n else levelL - 2 * sgn
            x, y = slots[k]
            k += 1
            dsc = s.desc()
            s.right(x - 12 - 60, y, decoy, dsc.copy())     # lower index, distance 0, outside the octave gate
            iR = s.right(x - 12, y, p, s.flipped(dsc, 40))
            s.left(x, y, levelL, dsc, PASSED, iR)
    s.ballast(32, h - lo - 26, x0=lo + 40, cols=16)
    return s.finish()


def case_row_band(pyramid=(1.2, 8), w=W, h=H):
    """One right keypoint per level (first, middle, last) with a fractional y; left keypoints on the first and last row of its
    band floor(yR - r) .. ceil(yR + r) and one row beyond on both sides."""
    s = Scene(103, w, h, pyramid)
    n = len(s.scale)
    lo = int(math.ceil(17 * float(s.scale[-1])))
    for j, lev in enumerate((0, n // 2 - 1 if n == 8 else n // 2, n - 1)):
        yR = f32(lo + 30 + 0.37 + 45 * j)
        r = f32(2.0) * s.scale[lev]
        minr, maxr = int(math.floor(float(yR - r))), int(math.ceil(float(yR + r)))
        dsc = s.desc()
        xR = w - lo - 60
        iR = s.right(xR, yR, lev, dsc)
        for i, (row, ok) in enumerate(((minr - 1, False), (minr, True), (maxr, True), (maxr + 1, False))):
            s.left(xR + 12, f32(row + 0.5), lev, s.flipped(dsc, i), PASSED if ok else "no_candidate", iR if ok else None)
    s.ballast(32, lo, x0=lo + 20, cols=8)
    return s.finish()


def case_workgroup_bands():
    """Left rows on both sides of the 16-row (direct form) and 24-row (row-sorted form) band edges, their partners' row bands
    straddling the edge; coarsest-level partners seven rows away."""
    s = Scene(104)
    x = 60
    for row in (15, 16, 23, 24, 47, 48):
        for dy in (-1.75, 1.75):                # partner in the other band, its +-2 px band reaching this row
            dsc = s.desc()
            iR = s.right(x - 12, f32(row + 0.75 + dy), 0, dsc)
            s.set_sad(x - 12, row + 1, 10)
            s.left(x, f32(row + 0.75), 0, dsc, PASSED, iR)
            x += 26
    for row, dy in ((47, 7.0), (48, -7.0)):     # level-7 partner (band +-7.17 rows) of a level-6 left keypoint
        dsc = s.desc()
        x = 200 + (row - 47) * 60
        iR = s.right(x - 12, f32(row + 0.5 + dy), 7, dsc)
        s.left(x, f32(row + 0.5), 6, dsc, PASSED, iR)
    s.ballast(32, 120, cols=16)
    return s.finish()


def case_ties(order):
    """Two right candidates at the same Hamming distance: the lower index wins (:985, strict '<'), wherever it lies in row
    order.  order 0: the lower index is the true partner; 1: it is the decoy, whose window holds its minimum at inc = +5."""
    s = Scene(105 + order)
    fill_d = [s.desc() for _ in range(300)]
    for j, (yA, yB) in enumerate(((100.0, 100.0), (101.5, 99.0), (None, None))):
        # (yA, yB) = rows of the true partner and of the decoy.  j = 0: the same row; 1: different rows, the true partner in the
        # later one; 2: the lower index in row 97, the higher in row 101 and 300 other right keypoints of the band in the rows
        # between them (the other side of the 256-entry right trip)
        x, y = 150 + 60 * j, 100
        dsc = s.desc()
        true_pos, decoy_pos = (x - 12, yA), (x - 60, yB)
        s.set_sad(x - 12, y, 10)
        s.set_sad(x - 60 + 5, y, 7, left=s.L[y - 5:y + 6, x - 5:x + 6])   # the decoy's SADs: smallest at inc = +5
        first, second = (true_pos, decoy_pos) if order == 0 else (decoy_pos, true_pos)
        if j == 2:
            first, second = (first[0], 97.5), (second[0], 101.5)
        iR = s.right(first[0], f32(first[1]), 0, s.flipped(dsc, 20))
        if j == 2:
            for i in range(300):
                s.right(40 + (i % 100) * 3, f32(99.0 + 0.5 * (i // 100)), 0, fill_d[i])
        s.right(second[0], f32(second[1]), 0, s.flipped(dsc, 20))
        s.left(x, f32(y + 0.25), 0, dsc, "accepted" if order == 0 else "bestinc_edge", iR)
    s.ballast(16, 200)
    return s.finish()


def case_left_trips(n_left):
    """n_left left keypoints in one 16-row band (128-entry left trips), each with its partner."""
    s = Scene(110 + n_left % 7)
    s.speckle(0.08)
    for i in range(n_left):
        x, y = 60 + 5 * (i % 60), 64 + i // 60            # rows 64 .. 68: inside one band of both forms ([64, 80) and [48, 72))
        dsc = s.desc()
        iR = s.right(x - 12, y, 0, s.flipped(dsc, i % 30))
        s.left(x, y, 0, dsc, PASSED, iR)
    return s.finish()


def case_right_trips(n_right):
    """n_right right candidates in the rows of one band (256-entry right trips); the winners come last in row order."""
    s = Scene(120 + n_right % 7)
    for i in range(n_right - 4):
        s.right(40 + 2 * (i % 150), f32(66.0 + 0.5 * (i // 150)), 0, s.desc())
    for j in range(4):                                     # partners in the band's last rows: the last trip
        x = 120 + 40 * j
        dsc = s.desc()
        iR = s.right(x - 12, 77.0, 0, s.flipped(dsc, 30))
        s.set_sad(x - 12, 76, 10 + j)
        s.left(x, 76.0, 0, dsc, PASSED, iR)
    s.ballast(16, 200)
    return s.finish()


def case_counts(n_left, n_right):
    """n_left / n_right keypoints on a 5-pixel grid (overlapping windows), partners where both exist."""
    s = Scene(130 + (n_left + 3 * n_right) % 11)
    s.speckle(0.08)
    for i in range(max(n_left, n_right)):
        x, y = 120 + 5 * (i % 44), 24 + 5 * (i // 44)
        dsc = s.desc()
        iR = None
        if i < n_right:
            iR = s.right(x - 12, y, 0, s.flipped(dsc, i % 40))
        if i < n_left:
            s.left(x, y, 0, dsc, PASSED if iR is not None else "no_candidate", iR)
    return s.finish()


def case_median(kind):
    """The median cut (:1072-1083): th = 1.5f * 1.4f * median, median = element m / 2 of the ascending SADs."""
    s = Scene(140 + len(kind))
    if kind.startswith("m"):                      # m = 1 .. 4 matches, SADs 10, 20, 30, 40
        m = int(kind[1:])
        sads = [10 * (i + 1) for i in range(m)]
    else:
        sads = {"boundary": [10] * 5 + [20, 21, 22, 40],          # median 10, th = 2.1f * 10: 20 stays, 21 is cut
                "equal": [33] * 7,
                "zeros_cut": [0] * 5 + [1, 2, 3, 4],              # median 0: th = 0 cuts everything
                "zeros_survive": [0] * 4 + [5, 6, 7, 8, 30]}[kind]  # median 5: the zeros stay
    srt = sorted(sads)
    med = f32(srt[len(srt) // 2])
    th = f32(1.5) * f32(1.4) * med
    for i, v in enumerate(sads):
        s.pair(80 + 26 * i, 100, 12, "accepted" if f32(v) < th else "cut_by_median", sad=v)
    return s.finish()


CASES = {
    "gates": case_gates,
    "octave_gate": case_octave_gate,
    "row_band": case_row_band,
    "workgroup_bands": case_workgroup_bands,
    "ties_true_first": lambda: case_ties(0),
    "ties_decoy_first": lambda: case_ties(1),
    "left_127": lambda: case_left_trips(127), "left_128": lambda: case_left_trips(128),
    "left_129": lambda: case_left_trips(129), "left_257": lambda: case_left_trips(257),
    "right_255": lambda: case_right_trips(255), "right_256": lambda: case_right_trips(256),
    "right_257": lambda: case_right_trips(257), "right_513": lambda: case_right_trips(513),
    "count_0_0": lambda: case_counts(0, 0), "count_0_1": lambda: case_counts(0, 1),
    "count_1_0": lambda: case_counts(1, 0), "count_1_1": lambda: case_counts(1, 1),
    "count_2048": lambda: case_counts(2048, 2048), "count_2049": lambda: case_counts(2049, 2049),
    "median_m1": lambda: case_median("m1"), "median_m2": lambda: case_median("m2"),
    "median_m3": lambda: case_median("m3"), "median_m4": lambda: case_median("m4"),
    "median_boundary": lambda: case_median("boundary"), "median_equal": lambda: case_median("equal"),
    "median_zeros_cut": lambda: case_median("zeros_cut"), "median_zeros_survive": lambda: case_median("zeros_survive"),
}
# The extractor needs 35 + 32 pixels at its coarsest level: 1.5^4 = 5.06 asks for 340 rows, so this pyramid runs at 480 x 352.
OTHER = dict(pyramid=(1.5, 5), w=480, h=352)
OTHER_CASES = {
    "gates_1.5x5": lambda: case_gates(**OTHER),
    "octave_gate_1.5x5": lambda: case_octave_gate(**OTHER),
    "row_band_1.5x5": lambda: case_row_band(**OTHER),
}
