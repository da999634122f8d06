"""Crafted inputs for the vocabulary-node walks (csrc/orbx_bow.hip, k_tri_match_rig in csrc/orbx_stereo.hip), beside matcher_cases.py:
SearchByBoW(KeyFrame, Frame), SearchByBoW(KeyFrame, KeyFrame), SearchForTriangulation and ComputeBoW.  A random scene puts about ten
features into a vocabulary node and almost never ties two Hamming distances where it matters, so every rule of the serial reference
that a parallel walk has to re-create gets a case of its own here, with the winner and the best / second distances it must produce.

Descriptors with full control of every distance: the walked side's feature i has its e_i HIGHEST bits set, the scored side's
feature j its d_j LOWEST bits, so dist(i, j) = e_i + d_j (as long as that is <= 256) and every walker ranks the candidates the same
way.  Feature vectors are hand-made CSR triples (node_ids, node_start, feature_idx) with permuted feature indices: the rules go by
the position in the node's list, never by the feature index.  All angles are 0: the rotation histogram keeps everything, it has
its own cases in matcher_cases.py.

The walkers below (walk_bow, walk_tri, descend, assemble) are the reference's loops with every rule behind a switch: with no switch
they are the reference, with one they are the reference with that rule replaced by its plausible wrong twin.  A case names the
switches that must change its result -- a case whose result does not depend on its rule tests nothing.

No GPU is touched here; tests/test_bow_walks.py runs the oracle and the HIP entries on these inputs.
"""
import zlib

import numpy as np

import orb_slam3_fast_amd as orbx

TH_LOW = 50
FILL = 120            # distance of the filler candidates: far above TH_LOW, never a winner, never a useful second
NODE_CAP = 4096       # kBowNodeCap


# ---- descriptors and feature vectors ----------------------------------------------------------------------------------------------
def low_bits(d):
    d = np.asarray(d, np.int64).reshape(-1, 1)
    return np.packbits((np.arange(256)[None, :] < d).astype(np.uint8), axis=1)


def high_bits(e):
    e = np.asarray(e, np.int64).reshape(-1, 1)
    return np.packbits((np.arange(256)[None, :] >= 256 - e).astype(np.uint8), axis=1)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class _LazyDist:
    def __init__(self, a, b):
        self.a, self.b = a, b

    def __getitem__(self, ij):
        return int(_POP[self.a[ij[0]] ^ self.b[ij[1]]].sum())


def dist_matrix(a, b):
    """Hamming distances [len(a), len(b)] by a byte popcount table (nothing shared with the code under test); pair by pair on
    demand where the full matrix would be large."""
    if len(a) * len(b) > (1 << 21):
        return _LazyDist(a, b)
    out = np.zeros((len(a), len(b)), np.int32)
    for s in range(0, len(a), 64):
        out[s:s + 64] = _POP[a[s:s + 64, None, :] ^ b[None, :, :]].sum(2)
    return out


def kps(n):
    k = np.zeros(n, orbx.KP_DTYPE)
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    return k


def csr(lists):
    """[(node id, [feature indices])] in ascending id order -> the CSR triple the entries take."""
    ids = np.array([n for n, _ in lists], np.uint32)
    start = np.cumsum([0] + [len(f) for _, f in lists]).astype(np.int32)
    feats = np.array([x for _, f in lists for x in f], np.uint32)
    return ids, start, feats


def lists_of(fv):
    ids, start, feats = fv
    return {int(ids[j]): [int(x) for x in feats[start[j]:start[j + 1]]] for j in range(len(ids))}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


class Case:
    def __init__(self, name, doc, **kw):
        self.name, self.doc = name, doc
        self.flips = ()          # switches that must change the result
        self.expect = {}         # what the walk must have seen: checked against the walker's trace
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


# ---- SearchByBoW, both flavours ---------------------------------------------------------------------------------------------------
def bow_case(name, flavour, nodes1, nodes2, nnratio, doc, flips=(), expect=None):
    """flavour "frame": side 1 = the key frame (walked; valid = kf_valid), side 2 = the frame (scored; right = right-eye features,
    which get the indices >= n_left).  flavour "kf": side 1 = pKF1, side 2 = pKF2, both with validity flags.
    nodes1 = [(id, e per list position, valid per list position or None)],
    nodes2 = [(id, d per list position, valid or None, right or None)]."""
    rng = _rng(name)
    e = np.array([x for _, ee, _ in nodes1 for x in ee], np.int64)
    v1 = np.array([x for _, ee, vv in nodes1 for x in (vv if vv is not None else [1] * len(ee))], np.uint8)
    d = np.array([x for _, dd, _, _ in nodes2 for x in dd], np.int64)
    v2 = np.array([x for _, dd, vv, _ in nodes2 for x in (vv if vv is not None else [1] * len(dd))], np.uint8)
    right = np.array([x for _, dd, _, rr in nodes2 for x in (rr if rr is not None else [0] * len(dd))], bool)
    n1, n2 = len(e), len(d)
    idx1 = rng.permutation(n1)                          # list position (over all nodes) -> feature index
    idx2 = np.zeros(n2, np.int64)
    n_left = -1
    if right.any():
        assert flavour == "frame"
        n_left = int((~right).sum())
        idx2[~right] = rng.permutation(n_left)
        idx2[right] = n_left + rng.permutation(n2 - n_left)
    else:
        idx2 = rng.permutation(n2)
    d1, d2 = np.zeros((n1, 32), np.uint8), np.zeros((n2, 32), np.uint8)
    d1[idx1], d2[idx2] = high_bits(e), low_bits(d)
    valid1, valid2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    valid1[idx1], valid2[idx2] = v1, v2

    def fv(nodes, idx):
        out, o = [], 0
        for nd in nodes:
            out.append((nd[0], [int(x) for x in idx[o:o + len(nd[1])]]))
            o += len(nd[1])
        return csr(out)
    c = Case(name, doc, kind="bow", flavour=flavour, fv1=fv(nodes1, idx1), d1=d1, v1=valid1, k1=kps(n1), fv2=fv(nodes2, idx2), d2=d2,
             v2=valid2, k2=kps(n2), n_left=n_left, nnratio=nnratio, flips=tuple(flips), expect=expect or {})
    c.dist = dist_matrix(d1, d2)
    return c


def walk_bow(c, flip=()):
    """src/ORBmatcher.cc:230-404 (flavour "frame") and :766-884 (flavour "kf") -> (nmatches, match, trace).  Switches:
    last_min        an equal later distance replaces the best (the reference keeps the first minimum)
    no_second       the `else if (dist < bestDist2)` update is dropped
    no_demote       a new best does not make the old best the second
    flip_th         `bestDist1 <= TH_LOW` <-> `bestDist1 < TH_LOW`
    product_double  the ratio test's product in double ((double)nnratio * b2) instead of float
    product_decimal the product with the decimal nnratio in double (as if nnratio had never been a float)
    ratio_le        `<` -> `<=` in the ratio test
    sentinel_255    bestDist1 / bestDist2 start at 255 instead of 256
    no_taken        a scored feature may be taken more than once
    no_valid2       pKF2's validity flags are ignored
    right_strict    the right eye's `bestDistR <= TH_LOW` becomes `<`
    right_ratio     the right eye gets a ratio test (the reference has `|| true`)
    right_alone     the right eye's acceptance moves out of the left eye's `bestDist1 <= TH_LOW`
    right_inside_left  the right eye is accepted only where the left eye was
    one_node        node ids are ignored: every feature is compared with every feature"""
    flip = set(flip)
    kf = c.flavour == "kf"
    m1, m2 = lists_of(c.fv1), lists_of(c.fv2)
    if "one_node" in flip:
        m1 = {0: [x for n in sorted(m1) for x in m1[n]]}
        m2 = {0: [x for n in sorted(m2) for x in m2[n]]}
    match = np.full(len(c.d1) if kf else len(c.d2), -1, np.int32)
    taken = np.zeros(len(c.d2), bool)
    r32 = np.float32(c.nnratio)
    strict = kf != ("flip_th" in flip)
    nm, trace = 0, []

    def ratio_ok(b1, b2):
        if "product_double" in flip:
            lhs, rhs = float(b1), float(r32) * float(b2)
        elif "product_decimal" in flip:
            lhs, rhs = float(b1), float(c.nnratio) * float(b2)
        else:
            lhs, rhs = np.float32(b1), r32 * np.float32(b2)
        return bool(lhs <= rhs) if "ratio_le" in flip else bool(lhs < rhs)

    for node in sorted(set(m1) & set(m2)):
        for p1, i1 in enumerate(m1[node]):
            if not c.v1[i1]:
                continue
            b2_0 = 255 if "sentinel_255" in flip else 256
            L, R = [b2_0, -1, b2_0, -1], [b2_0, -1, b2_0, -1]   # best, its feature, second, the best's list position
            for p2, i2 in enumerate(m2[node]):
                if taken[i2] and "no_taken" not in flip:
                    continue
                if kf and not c.v2[i2] and "no_valid2" not in flip:
                    continue
                dd = int(c.dist[i1, i2])
                s = R if (not kf and c.n_left != -1 and i2 >= c.n_left) else L
                if dd < s[0] or ("last_min" in flip and dd == s[0]):
                    s[2], s[0], s[1], s[3] = s[2] if "no_demote" in flip else s[0], dd, i2, p2
                elif dd < s[2] and "no_second" not in flip:
                    s[2] = dd
            th_ok = L[0] < TH_LOW if strict else L[0] <= TH_LOW
            left_ok = th_ok and ratio_ok(L[0], L[2])
            right_ok = False
            if not kf and (th_ok or "right_alone" in flip):
                right_ok = R[0] < TH_LOW if "right_strict" in flip else R[0] <= TH_LOW
                if "right_ratio" in flip:
                    right_ok = right_ok and ratio_ok(R[0], R[2])
                if "right_inside_left" in flip:
                    right_ok = right_ok and left_ok
            for ok, s in ((left_ok, L), (right_ok, R)):
                if ok:
                    if kf:
                        match[i1] = s[1]
                    else:
                        match[s[1]] = i1
                    taken[s[1]] = True
                    nm += 1
            trace.append(dict(node=node, pos1=p1, i1=i1, b1=L[0], b2=L[2], pos=L[3], b1r=R[0], b2r=R[2], posr=R[3], left=left_ok,
                              right=right_ok))
    return nm, match, trace


def _fill(n, **at):
    d = [FILL] * n
    for p, v in at.items():
        d[int(p[1:])] = v
    return d


def _chain_lists(name, n2, n1, kf, nwin=46, fill=FILL):
    """A node of n2 scored and n1 walking features in which valid walker number i takes the i-th smallest free candidate: the distinct
    distances 0, 1, ... (at most 46 of them) sit at random list positions, everything else is filler; every third walker is invalid;
    in the key-frame flavour every fourth candidate is invalid and would win (distance 0) if its flag were ignored."""
    rng = _rng(name + "/lists")
    d = np.full(n2, fill, np.int64)
    v2 = np.ones(n2, np.uint8)
    free = np.arange(n2)
    if kf and n2 >= 4:
        v2[3::4] = 0
        d[3::4] = 0
        free = np.nonzero(v2)[0]
    winners = rng.permutation(free)[:min(nwin, len(free))]
    if n2 > 64:                                          # winners on both sides of the first 64 (the register-resident ones)
        for k_, p in enumerate((62, 64)):
            if p not in winners:
                winners[k_] = p
        assert len(set(winners.tolist())) == len(winners) and v2[winners].all()
    d[winners] = (1 if kf and n2 >= 4 else 0) + np.arange(len(winners))
    e = [0] * n1
    v1 = [0 if i % 3 == 1 else 1 for i in range(n1)]
    return [int(x) for x in d], [int(x) for x in v2], e, v1, sorted(int(x) for x in winners)


def size_case(flavour, n2, n1):
    name = "%s/size_%d_%d" % (flavour, n2, n1)
    kf = flavour == "kf"
    d, v2, e, v1, winners = _chain_lists(name, n2, n1, kf)
    walkers = sum(v1)
    # with nnratio 1.0 walker i takes distance i (+1) while the next free distance is larger; the last distinct distance is taken
    # against a filler second.  Key-frame flavour: b1 < 50 always holds (distances <= 46).
    n_expect = min(walkers, len(winners))
    doc = ("a node of %d scored and %d walking features: the valid walkers take the distinct distances in ascending order, "
           "%d matches; winners at list positions %s..." % (n2, n1, n_expect, winners[:4]))
    flips = ["no_taken"] if n_expect > 1 else []
    if kf and n2 >= 4:
        flips.append("no_valid2")
    early = sum(v1[:64])                                 # valid walkers of the first batch of 64
    return bow_case(name, flavour, [(7, e, v1)], [(7, d, v2 if kf else None, None)], 1.0, doc, flips,
                    dict(nmatches=n_expect, winners=winners, both_sides=n2 > 64 and n_expect == len(winners), late_walker=n_expect > early))


def chain_case(flavour):
    """The order-dependent walk at full length: candidate distances 0 .. 50 (1 .. 51 in the key-frame flavour, whose invalid
    candidates sit at 0) at random positions of a node of 130, fillers at 200, 100 walkers with e = 0 of which every third is invalid,
    nnratio 1.0.  Valid walker i takes the i-th free distance; 43 valid walkers sit in the first batch of 64, so the later matches
    need the taken marks of the first batch."""
    kf = flavour == "kf"
    d, v2, e, v1, winners = _chain_lists(flavour + "/chain", 130, 100, kf, nwin=51, fill=200)
    n_expect = 49 if kf else 51                           # key-frame flavour: 1 .. 49 pass `bestDist1 < TH_LOW`, 50 and 51 do not
    return bow_case(flavour + "/chain", flavour, [(7, e, v1)], [(7, d, v2 if kf else None, None)], 1.0, chain_case.__doc__,
                    ["no_taken"] + (["no_valid2"] if kf else []),
                    dict(nmatches=n_expect, winners=winners, both_sides=True, late_walker=True, chain=True))


def tie_case(flavour, a, b, variant):
    """130 candidates, fillers but for list positions a < b; one walker with e = 3."""
    name = "%s/tie_%d_%d_%s" % (flavour, a, b, variant)
    at = {"p%d" % a: 10, "p%d" % b: 10 if variant in ("r1", "r1.5") else 11}
    ratio = dict(r1=1.0, **{"r1.5": 1.5}, plus1_r099=0.99, plus1_r09=0.9)[variant]
    if variant == "r1":
        doc, flips, ex = "equal minimum 13 at positions %d and %d: the second equals the best, nnratio 1.0 rejects" % (a, b), ["ratio_le"], \
            dict(nmatches=0, pos=a, b1=13, b2=13)
    elif variant == "r1.5":
        doc, flips, ex = "equal minimum at %d and %d with nnratio 1.5: the ratio passes and the EARLIER position wins" % (a, b), \
            ["last_min"], dict(nmatches=1, pos=a, b1=13, b2=13)
    elif variant == "plus1_r099":
        doc, flips, ex = "best 13 at %d, second 14 at %d: 13 < 0.99 * 14 matches" % (a, b), [], \
            dict(nmatches=1, pos=a, b1=13, b2=14)
    else:
        doc, flips, ex = "best 13 at %d, second 14 at %d: 13 < 0.9 * 14 fails; a lost second (filler) would match" % (a, b), \
            ["no_second"], dict(nmatches=0, pos=a, b1=13, b2=14)
    return bow_case(name, flavour, [(7, [3], None)], [(7, _fill(130, **at), None, None)], ratio, doc, flips, ex)


def second_before_best_case(flavour, variant):
    name = "%s/second_before_best_%s" % (flavour, variant)
    ratio = 0.99 if variant == "r099" else 0.9
    return bow_case(name, flavour, [(7, [3], None)], [(7, _fill(130, p5=11, p70=10), None, None)], ratio,
                    "second 14 at position 5 (first chunk), best 13 at 70 (second chunk): the old best becomes the second",
                    [] if variant == "r099" else ["no_demote"], dict(nmatches=1 if variant == "r099" else 0, pos=70, b1=13, b2=14))


def th_case(flavour, b1):
    name = "%s/th_%d" % (flavour, b1)
    limit = 49 if flavour == "kf" else 50
    return bow_case(name, flavour, [(7, [2], None)], [(7, [b1 - 2], None, None)], 0.7,
                    "a lone candidate at distance %d: %s (TH_LOW is %s in this flavour)" %
                    (b1, "accepted" if b1 <= limit else "rejected", "strict" if flavour == "kf" else "inclusive"),
                    ["flip_th"] if b1 == 50 else [], dict(nmatches=int(b1 <= limit), pos=0, b1=b1, b2=256))


def ratio_case(flavour, b1, b2, r, verdict, flips):
    name = "%s/ratio_%d_%d_%g" % (flavour, b1, b2, r)
    assert bool(np.float32(b1) < np.float32(r) * np.float32(b2)) == verdict      # the verdict in float arithmetic
    return bow_case(name, flavour, [(7, [5], None)], [(7, [b2 - 5, 90, b1 - 5], None, None)], r,
                    "(float)%d < %gf * (float)%d is %s" % (b1, r, b2, verdict), flips, dict(nmatches=int(verdict), pos=2, b1=b1, b2=b2))


def lone_case(flavour, r):
    name = "%s/lone_%g" % (flavour, r)
    verdict = bool(np.float32(49) < np.float32(r) * np.float32(256))
    return bow_case(name, flavour, [(7, [9], None)], [(7, [40], None, None)], r,
                    "a lone candidate at 49: the second stays 256, 49 < %gf * 256 is %s" % (r, verdict),
                    ["sentinel_255"] if r == 0.192 else [], dict(nmatches=int(verdict), pos=0, b1=49, b2=256))


def last_free_case(flavour):
    name = "%s/last_free" % flavour
    return bow_case(name, flavour, [(7, [0, 0], None)], [(7, [10, 20], None, None)], 0.6,
                    "two candidates 10 and 20, two walkers, nnratio 0.6: the first takes 10 (10 < 12), the second then sees 20 alone "
                    "against a second of 256 and takes it; without the taken mark it would take 10 again", ["no_taken"],
                    dict(nmatches=2))


def right_eye_cases():
    """The frame flavour with n_left_f inside the node: 70 candidates, right-eye ones on both sides of position 64."""
    def rc(name, left, rightd, doc, flips, ex):
        d, right = [150] * 70, [0] * 70
        for p in (2, 11, 30, 63, 64, 66, 69):
            right[p], d[p] = 1, 160
        for p, v in left.items():
            assert not right[p]
            d[p] = v
        for p, v in rightd.items():
            assert right[p]
            d[p] = v
        return bow_case("frame/right_" + name, "frame", [(7, [0], None)], [(7, d, None, right)], 0.7, doc, flips, ex)
    return [
        rc("50", {5: 20}, {64: 50}, "left 20 / 150 matches; right best 50 is accepted with no ratio test: one key-frame feature, 2 matches",
           ["right_strict"], dict(nmatches=2, b1=20, b1r=50, posr=64)),
        rc("50_50", {5: 20}, {30: 50, 66: 50}, "right best 50 and right second 50: still accepted, the earlier position wins",
           ["right_ratio", "last_min"], dict(nmatches=2, b1r=50, b2r=50, posr=30)),
        rc("10_left51", {5: 51}, {11: 10}, "right best 10 but left best 51: the right eye sits inside the left eye's TH_LOW, nothing matches",
           ["right_alone"], dict(nmatches=0, b1=51, b1r=10)),
        rc("left_fails_ratio", {5: 20, 40: 20}, {69: 30}, "left 20 / 20 passes TH_LOW and fails the ratio test; the right eye (30) is accepted",
           ["right_inside_left"], dict(nmatches=1, b1=20, b2=20, b1r=30, posr=69)),
    ]


def node_cases(flavour):
    one = lambda nid, d=3: (nid, [d], None, None)                                   # noqa: E731
    w = lambda nid: (nid, [0], None)                                               # noqa: E731
    out = [
        bow_case(flavour + "/nodes_mixed", flavour, [w(2), w(5), w(9), w(11)], [one(1, 0), one(5), one(7, 0), one(11, 4), one(12, 0)], 0.7,
                 "nodes 2, 9 only on the walked side, 1, 7, 12 only on the scored side (holding the closest candidates): 5 and 11 match",
                 ["one_node"], dict(nmatches=2)),
        bow_case(flavour + "/nodes_disjoint", flavour, [w(2), w(4), w(6)], [one(1), one(3, 10), one(5, 20), one(7, 40)], 0.7,
                 "no common node id: nothing matches", ["one_node"], dict(nmatches=0)),
        bow_case(flavour + "/partner_first", flavour, [w(5)], [one(5), one(8, 0), one(20, 0)], 0.7, "the partner node is the first of three",
                 ["one_node"], dict(nmatches=1)),
        bow_case(flavour + "/partner_last", flavour, [w(20)], [one(5, 0), one(8, 0), one(20)], 0.7, "the partner node is the last of three",
                 ["one_node"], dict(nmatches=1)),
        bow_case(flavour + "/partner_alone", flavour, [w(1), w(5), w(9)], [one(5)], 0.7, "the scored side has one node", [], dict(nmatches=1)),
    ]
    d, v2, e, v1, winners = _chain_lists(flavour + "/long_beside_short", 130, 70, flavour == "kf")
    n1 = [(3 * i, [0], None) for i in range(20)] + [(61, e, v1)] + [(100 + 3 * i, [0], None) for i in range(20)]
    n2 = [(3 * i, [5 + i], None, None) for i in range(0, 20, 2)] + [(61, d, v2 if flavour == "kf" else None, None)] + \
        [(100 + 3 * i, [7], None, None) for i in range(20)]
    out.append(bow_case(flavour + "/long_beside_short", flavour, n1, n2, 1.0,
                        "one node of 130 x 70 features between forty one-feature nodes (every second of the first twenty has no partner)",
                        ["no_taken"], dict(nmatches=10 + 20 + min(sum(v1), len(winners)))))
    return out


def cap_case(flavour, n, shared=True):
    """A node of n scored features (4096 = kBowNodeCap is served, 4097 is refused) beside an ordinary node whose match is made
    either way; shared = False: the walked side does not have the large node, which then is never looked at."""
    name = "%s/cap_%d%s" % (flavour, n, "" if shared else "_unshared")
    d = _fill(n, p0=30, p63=9, p64=8, p4000=7)
    d[n - 1] = 6
    n1 = [(4, [0], None)] + ([(9, [0, 0, 0, 0, 0], [1, 0, 1, 1, 1])] if shared else [])
    n2 = [(4, [3, 44], None, None), (9, d, None, None)]
    return bow_case(name, flavour, n1, n2, 0.9, "a node of %d scored features%s" % (n, "" if shared else ", absent from the walked side"),
                    [], dict(nmatches=5 if shared else 1, refused=shared and n > NODE_CAP))


def bow_cases(flavour):
    out = [size_case(flavour, n2, n1) for n2 in (1, 63, 64, 65, 128, 129) for n1 in (1, 64, 65, 130)]
    out += [tie_case(flavour, a, b, v) for a, b in ((3, 64), (63, 64), (0, 128), (70, 100)) for v in ("r1", "r1.5", "plus1_r099", "plus1_r09")]
    out += [second_before_best_case(flavour, v) for v in ("r099", "r09")]
    out += [th_case(flavour, b) for b in (49, 50, 51)]
    # 0.7f * 50.0f rounds to 35.0f and 0.6f * 50.0f to 30.000002f; 0.8f and 0.6f lie above 0.8 and 0.6, so their products with 50
    # and 35 are above 40 and 21 in double and round to exactly 40.0f and 21.0f in float: only the float product rejects those
    out += [ratio_case(flavour, 35, 50, 0.7, False, ["ratio_le"]), ratio_case(flavour, 30, 50, 0.6, True, ["product_decimal"]),
            ratio_case(flavour, 25, 50, 0.5, False, ["ratio_le"]), ratio_case(flavour, 45, 50, 0.9, False, ["ratio_le"]),
            ratio_case(flavour, 40, 50, 0.8, False, ["product_double"]), ratio_case(flavour, 21, 35, 0.6, False, ["product_double"])]
    out += [lone_case(flavour, r) for r in (0.2, 0.19, 0.192)]
    out.append(last_free_case(flavour))
    out.append(chain_case(flavour))
    if flavour == "frame":
        out += right_eye_cases()
    out += node_cases(flavour)
    return out


def cap_cases(flavour):
    return [cap_case(flavour, NODE_CAP), cap_case(flavour, NODE_CAP + 1), cap_case(flavour, NODE_CAP + 1, shared=False)]


# ---- SearchForTriangulation -------------------------------------------------------------------------------------------------------
# Geometry far from every float gate: F12 makes the epipolar line of (x1, y1) the row y2 = y1, so a candidate on the row has
# distance 0 and one 40 px off it 1600 against the gate 3.84 * sigma2 = 3.84; the epipole sits at (-1e4, -1e4) unless a case
# moves it onto a candidate.
F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
FAR_EPIPOLE = np.array([-1e4, -1e4], np.float32)
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)


def tri_case(name, nodes1, nodes2, doc, flips=(), expect=None, ep=FAR_EPIPOLE, only_stereo=False, coarse=False, stereo=False):
    """nodes1 = [(id, [dict(e=, mp=0, ur=-1)])], nodes2 = [(id, [dict(d=, mp=0, off=0 (rows off the epipolar line), x=None, ur=-1)])].
    Feature i of pKF1 sits at (100 + i, 200); every candidate at (x or 400 + position, 200 + off)."""
    rng = _rng(name)
    f1 = [f for _, fs in nodes1 for f in fs]
    f2 = [f for _, fs in nodes2 for f in fs]
    n1, n2 = len(f1), len(f2)
    idx1, idx2 = rng.permutation(n1), rng.permutation(n2)
    k1, k2 = kps(n1), kps(n2)
    d1, d2 = np.zeros((n1, 32), np.uint8), np.zeros((n2, 32), np.uint8)
    d1[idx1], d2[idx2] = high_bits([f["e"] for f in f1]), low_bits([f["d"] for f in f2])
    mp1, mp2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    ur1, ur2 = np.full(n1, -1, np.float32), np.full(n2, -1, np.float32)
    for p, f in enumerate(f1):
        i = idx1[p]
        k1["x"][i], k1["y"][i] = 100.0 + (p % 256), 200.0
        mp1[i], ur1[i] = f.get("mp", 0), f.get("ur", -1)
    for p, f in enumerate(f2):
        i = idx2[p]
        k2["x"][i], k2["y"][i] = f.get("x", 400.0 + (p % 200)), 200.0 + f.get("off", 0)
        mp2[i], ur2[i] = f.get("mp", 0), f.get("ur", -1)

    def fv(nodes, idx):
        out, o = [], 0
        for nid, fs in nodes:
            out.append((nid, [int(x) for x in idx[o:o + len(fs)]]))
            o += len(fs)
        return csr(out)
    c = Case(name, doc, kind="tri", fv1=fv(nodes1, idx1), k1=k1, d1=d1, mp1=mp1, ur1=ur1 if stereo else None, fv2=fv(nodes2, idx2), k2=k2,
             d2=d2, mp2=mp2, ur2=ur2 if stereo else None, ep=np.asarray(ep, np.float32), only_stereo=only_stereo, coarse=coarse,
             flips=tuple(flips), expect=expect or {})
    c.dist = dist_matrix(d1, d2)
    return c


def walk_tri(c, flip=()):
    """src/ORBmatcher.cc:886-1106 for single-camera key frames (and, with bCoarse, the rig branch: no gate takes part) ->
    (nmatches, matches12, trace).  Switches:
    first_min   an equal later distance does not replace the best (the reference's `dist > bestDist` lets it)
    strict_th   `dist > TH_LOW` -> `dist >= TH_LOW`
    shadow      bestDist is lowered before the geometric gates, so a gate-failing candidate shadows a farther gate-passer
    no_epipole / no_chi2 / no_mp2 / no_stereo2   that gate is skipped
    matched2    vbMatched2 is set for the chosen feature (the reference never sets it)"""
    flip = set(flip)
    m1, m2 = lists_of(c.fv1), lists_of(c.fv2)
    f = np.float32
    m12 = np.full(len(c.k1), -1, np.int32)
    matched2 = np.zeros(len(c.k2), bool)
    nm, trace = 0, []
    for node in sorted(set(m1) & set(m2)):
        for i1 in m1[node]:
            if c.mp1[i1]:
                continue
            st1 = c.ur1 is not None and c.ur1[i1] >= 0
            if c.only_stereo and not st1:
                continue
            best, bi, bpos = TH_LOW, -1, -1
            for p2, i2 in enumerate(m2[node]):
                if matched2[i2] or (c.mp2[i2] and "no_mp2" not in flip):
                    continue
                st2 = c.ur2 is not None and c.ur2[i2] >= 0
                if c.only_stereo and not st2 and "no_stereo2" not in flip:
                    continue
                dd = int(c.dist[i1, i2])
                if dd > TH_LOW or dd > best or ("strict_th" in flip and dd >= TH_LOW) or ("first_min" in flip and bi >= 0 and dd >= best):
                    continue
                if "shadow" in flip:
                    best = dd
                if not st1 and not st2 and "no_epipole" not in flip:
                    ex, ey = f(c.ep[0]) - f(c.k2["x"][i2]), f(c.ep[1]) - f(c.k2["y"][i2])
                    if ex * ex + ey * ey < f(100) * SCALE[c.k2["octave"][i2]]:
                        continue
                if not c.coarse and "no_chi2" not in flip:
                    x1, y1, x2, y2 = f(c.k1["x"][i1]), f(c.k1["y"][i1]), f(c.k2["x"][i2]), f(c.k2["y"][i2])
                    a, b, cc = x1 * F12[0] + y1 * F12[3] + F12[6], x1 * F12[1] + y1 * F12[4] + F12[7], x1 * F12[2] + y1 * F12[5] + F12[8]
                    num, den = a * x2 + b * y2 + cc, a * a + b * b
                    if den == 0 or not float(num * num / den) < 3.84 * float(SIGMA2[c.k2["octave"][i2]]):
                        continue
                best, bi, bpos = dd, i2, p2
            if bi >= 0:
                m12[i1] = bi
                nm += 1
                if "matched2" in flip:
                    matched2[bi] = True
            trace.append(dict(i1=i1, best=best, pos=bpos))
    return nm, m12, trace


def tri_cases():
    c2 = lambda d, **kw: dict(d=d, **kw)                                            # noqa: E731
    one = [(7, [dict(e=4)])]
    out = []
    for n in (1, 15, 16, 17, 33, 40):
        ds = [16 + (11 * p) % 29 for p in range(n)]
        ds[(5 * n) // 7] = 6                                                         # the unique minimum, somewhere in the last trip
        out.append(tri_case("tri/size_%d" % n, one, [(7, [c2(x) for x in ds])], "one feature of pKF1 against a node of %d: the unique "
                            "minimum 10 at position %d" % (n, (5 * n) // 7), [], dict(nmatches=1, pos=(5 * n) // 7, best=10)))
    for n, tie in ((40, (2, 18, 35)), (17, (0, 16)), (17, (15, 16))):
        ds = [20 + p % 9 for p in range(n)]
        for p in tie:
            ds[p] = 6
        out.append(tri_case("tri/tie_" + "_".join(map(str, tie)), one, [(7, [c2(x) for x in ds])],
                            "equal minimal distance 10 at positions %s: the LAST wins" % (tie,), ["first_min"],
                            dict(nmatches=1, pos=tie[-1], best=10)))
    out.append(tri_case("tri/th_50", one, [(7, [c2(46)])], "a lone candidate at 50 is accepted", ["strict_th"], dict(nmatches=1, pos=0, best=50)))
    out.append(tri_case("tri/th_51", one, [(7, [c2(47)])], "a lone candidate at 51 is rejected", [], dict(nmatches=0)))
    gate = [c2(36), c2(1, x=303.0), c2(26), c2(40)]                              # position 1 is the closest and fails its gate
    out.append(tri_case("tri/gate_epipole", one, [(7, gate)], "the closest candidate (5) lies 3 px from the epipole: the candidate at 30 "
                        "is chosen", ["no_epipole", "shadow"], dict(nmatches=1, pos=2, best=30), ep=(300.0, 200.0)))
    gate = [c2(36), c2(1, off=40), c2(26), c2(40, off=-40)]
    out.append(tri_case("tri/gate_chi2", one, [(7, gate)], "the closest candidate (5) lies 40 px off the epipolar line: 30 is chosen",
                        ["no_chi2", "shadow"], dict(nmatches=1, pos=2, best=30)))
    out.append(tri_case("tri/gate_chi2_coarse", one, [(7, gate)], "the same with bCoarse: no epipolar test, the closest candidate is chosen",
                        [], dict(nmatches=1, pos=1, best=5), coarse=True))
    gate = [c2(36), c2(1, mp=1), c2(26), c2(40)]
    out.append(tri_case("tri/gate_mappoint", one, [(7, gate)], "the closest candidate already has a map point: 30 is chosen", ["no_mp2"],
                        dict(nmatches=1, pos=2, best=30)))
    gate = [c2(36, ur=380.0), c2(1), c2(26, ur=390.0), c2(40, ur=395.0)]
    out.append(tri_case("tri/gate_only_stereo", [(7, [dict(e=4, ur=90.0)])], [(7, gate)], "bOnlyStereo: the closest candidate is monocular, "
                        "30 is chosen", ["no_stereo2"], dict(nmatches=1, pos=2, best=30), only_stereo=True, stereo=True))
    out.append(tri_case("tri/same_choice", [(7, [dict(e=4), dict(e=9)])], [(7, [c2(20), c2(3), c2(30)])],
                        "two features of pKF1 choose the same feature of pKF2 and both keep it (vbMatched2 is never set)", ["matched2"],
                        dict(nmatches=2, pos=1)))
    for n in (17, 4097):                                                             # the 16-per-workgroup mapping and the start1 search
        n1 = [(2 * j, [dict(e=j % 5) for _ in range(1 + j % 4)]) for j in range(n)]
        total, keep = 0, []
        for nid, fs in n1:
            if total >= n:
                break
            keep.append((nid, fs[:n - total]))
            total += len(keep[-1][1])
        n2 = [(nid, [c2(30), c2(8 + nid % 7), c2(30)]) for nid, _ in keep if nid % 6 != 2]
        out.append(tri_case("tri/list_%d" % n, keep, n2, "%d features of pKF1 over %d nodes, a third of them without a partner node"
                            % (n, len(keep)), [], dict(list1=n)))
    return out


def rig_args(c):
    """A tri case as SearchForTriangulationRig input with bCoarse: the rig record is never read, every feature is a left one."""
    rig = np.zeros((), orbx.TRI_RIG_DTYPE)
    rig["precision"] = 1e-6
    return (c.fv1, c.k1, c.d1, c.mp1, len(c.k1), c.fv2, c.k2, c.d2, c.mp2, len(c.k2), SIGMA2, SIGMA2, rig)


def rig_coarse_cases():
    return [c for c in tri_cases() if c.ur1 is None and (c.name.startswith(("tri/size", "tri/tie", "tri/th", "tri/same", "tri/list_17")) or
                                                         c.name == "tri/gate_mappoint")]


def rig_eye_case(sc, kk, dd, nL):
    """On the stereo-fisheye scene of test_reloc_triangulation._rig_inputs (both key frames = one frame, features = left | right):
    walkers of pKF1 that are left features and walkers that are right features, each against a node of three candidates: itself
    (same camera: T = identity, no parallax, far outside the gate; distance 4), a wrong feature of the other camera (outside
    wherever the two rays do not meet in front of both cameras; 12) and the true partner (inside; 20).  Descriptors are replaced by
    crafted ones, so the candidates outside the gate are closer than the partner: ll / lr are exercised by the left walkers,
    rl / rr by the right ones.  (A different feature of the walker's own camera is no candidate here: with T = identity its
    triangulation is degenerate and lands on the gates.)  Returns (fv1, fv2, descriptors1, descriptors2)."""
    tl, tr = np.asarray(sc["true_left"]), np.asarray(sc["true_right"]) + nL
    pairs = [(int(a), int(b)) for a, b in zip(tl[:48], tr[:48])]
    assert len(set(x for p in pairs for x in p)) == 96
    d1, d2 = np.zeros_like(dd), np.zeros_like(dd)
    n1, n2 = [], []
    for q in range(0, len(pairs) - 3, 4):
        (a, b), (_, b2), (a3, b3), (a4, _) = pairs[q:q + 4]
        for me, partner, wrong in ((a, b, b2), (b3, a3, a4)):
            cand = [me, wrong, partner]
            d1[me] = high_bits([2])[0]
            d2[cand] = low_bits([2, 10, 18])
            n1.append((3 + 2 * len(n1), [me]))
            n2.append((n1[-1][0], cand))
    return csr(n1), csr(n2), d1, d2


# ---- ComputeBoW -------------------------------------------------------------------------------------------------------------------
def voc_columns(children_desc, leaf_weight=None):
    """A vocabulary from nested lists: children_desc = [(descriptor, sub-list or weight)] -> (parent, is_leaf, desc, weight) in the
    file's node order (the k children of a node together, then each child expanded)."""
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def expand(pid, kids):
        first = len(parent)
        for dsc, sub in kids:
            parent.append(pid)
            leaf.append(int(not isinstance(sub, list)))
            desc.append(np.asarray(dsc, np.uint8))
            weight.append(0.0 if isinstance(sub, list) else float(sub))
        for i, (_, sub) in enumerate(kids):
            if isinstance(sub, list):
                expand(first + i, sub)
    expand(0, children_desc)
    return np.array(parent, np.int32), np.array(leaf, np.uint8), np.stack(desc).astype(np.uint8), np.array(weight, np.float64)


def block(c, width=16):
    bits = np.zeros(256, np.uint8)
    bits[c * width:(c + 1) * width] = 1
    return np.packbits(bits)


def descend(cols, feats, levelsup, L, flip=()):
    """TemplatedVocabulary::transform(feature, ...) (:1202-1250) on the columns, level by level with a popcount table ->
    (word id, weight, node id) per feature.  Switch last_min: an equal later child replaces the best."""
    parent, leaf, desc, weight = cols
    n = len(parent)
    kids = [[] for _ in range(n)]
    wid, nw = np.zeros(n, np.int64), 0
    for i in range(1, n):
        kids[parent[i]].append(i)
        if leaf[i]:
            wid[i], nw = nw, nw + 1
    out = []
    for f in feats:
        cur, level, nid, nid_level = 0, 0, None, L - levelsup
        if nid_level <= 0:
            nid = 0
        while kids[cur]:
            ch = np.array(kids[cur])
            dd = _POP[desc[ch] ^ f[None, :]].sum(1)
            j = len(dd) - 1 - int(np.argmin(dd[::-1])) if "last_min" in flip else int(np.argmin(dd))
            cur = int(ch[j])
            level += 1
            if level == nid_level:
                nid = cur
        out.append((int(wid[cur]), float(weight[cur]), cur if nid is None else nid))
    return out


def assemble(found, scoring, weighting, flip=()):
    """TemplatedVocabulary::transform(features, ...) (:1125-1188) after the descents, std::map semantics ->
    ([(word, value)], [(node, [features])]).  Switch product: a word's value is weight * count instead of weight + weight + ..."""
    bow, cnt, fv = {}, {}, {}
    must, l2, additive = scoring != 5, scoring == 1, weighting in (0, 1)
    for i, (w, wt, nid) in enumerate(found):
        if wt > 0:
            if w in bow:
                if additive:
                    bow[w] = bow[w] + wt
                    cnt[w] += 1
            else:
                bow[w], cnt[w] = wt, 1
            fv.setdefault(nid, []).append(i)
    if "product" in flip:
        for w in bow:
            bow[w] = next(wt for ww, wt, _ in found if ww == w) * cnt[w]
    keys = sorted(bow)
    if additive and bow and not must:
        for kk in keys:
            bow[kk] /= float(len(bow))
    if must:
        norm = 0.0
        for kk in keys:
            norm += abs(bow[kk]) if not l2 else bow[kk] * bow[kk]
        if l2:
            norm = float(np.sqrt(norm))
        if norm > 0.0:
            for kk in keys:
                bow[kk] /= norm
    return [(kk, bow[kk]) for kk in keys], [(kk, fv[kk]) for kk in sorted(fv)]


def voc_case(name, doc, k, L, cols, feats, levelsup, scoring=0, weighting=0, flips=(), expect=None):
    return Case(name, doc, kind="voc", k=k, L=L, cols=cols, feats=np.ascontiguousarray(feats, np.uint8), levelsup=levelsup, scoring=scoring,
                weighting=weighting, flips=tuple(flips), expect=expect or {})


def _tie_tree(k, L, twin_of, level=1):
    """Every node has k children, child c's descriptor is block c, except that child twin_of[1] is a copy of child twin_of[0]."""
    kids = []
    for c in range(k):
        dsc = block(twin_of[0] if c == twin_of[1] else c)
        kids.append((dsc, 1.0 + c if level == L else _tie_tree(k, L, twin_of, level + 1)))
    return kids


def voc_cases():
    out = []
    kids = [(block(c, 8), 1.0 + c) for c in range(17)]
    kids[16] = (block(0, 8), 17.0)
    out.append(voc_case("voc/k17_children_0_16", "k = 17, L = 1, children 0 and 16 identical (both scored by lane 0): word 0", 17, 1,
                        voc_columns(kids), [block(0, 8), block(5, 8)], 0, flips=["last_min"], expect=dict(words=[0, 5])))
    kids = [(block(c, 8), 1.0 + c) for c in range(17)]
    kids[4] = (block(3, 8), 5.0)
    out.append(voc_case("voc/k17_children_3_4", "children 3 and 4 identical (neighbouring lanes): word 3", 17, 1, voc_columns(kids),
                        [block(3, 8)], 0, flips=["last_min"], expect=dict(words=[3])))
    out.append(voc_case("voc/equidistant", "a feature at distance 8 from every one of 17 children: word 0", 17, 1,
                        voc_columns([(block(c, 8), 1.0 + c) for c in range(17)]), [np.zeros(32, np.uint8)], 0, flips=["last_min"],
                        expect=dict(words=[0])))
    cols = voc_columns(_tie_tree(10, 3, (2, 7)))
    path2 = 2 * 100 + 2 * 10 + 2
    for lu in (0, 1, 3, 4):
        out.append(voc_case("voc/k10_L3_tie_every_level_levelsup%d" % lu, "k = 10, L = 3, children 2 and 7 identical at every level: the path "
                            "is 2, 2, 2 (word %d), a feature equidistant to all children goes 0, 0, 0; levelsup %d" % (path2, lu), 10, 3,
                            cols, [block(2), block(11), block(4)], lu, flips=["last_min"], expect=dict(words=[path2, 0, 444])))
    # a leaf above level L - levelsup: child 0 of the root is a word; with levelsup 1 the node id is taken at level 2, never reached
    sub = lambda: [(block(c), [(block(d), 2.0 + d) for d in range(3)]) for c in range(3)]   # noqa: E731
    cols = voc_columns([(block(5), 9.0), (block(6), sub()), (block(7), sub())])
    out.append(voc_case("voc/early_leaf", "a word at level 1 of an L = 3 tree, levelsup 1: the node id is the word's own node", 3, 3, cols,
                        [block(5), block(6), block(5)], 1, expect=dict(words=[0, 1, 0], fv=[(1, [0, 2]), (4, [1])])))
    cols = voc_columns([(block(c, 8), 0.0) for c in range(5)] + [(block(5, 8), 0.0)])
    out.append(voc_case("voc/all_stopped", "every feature lands on a stopped word (weight 0): empty vectors", 6, 1, cols,
                        [block(c % 6, 8) for c in range(40)], 0, expect=dict(empty=True)))
    cols = voc_columns([(block(0), 0.1), (block(1), 0.3)])
    feats = np.repeat(block(0)[None, :], 8192, 0)
    feats[4000] = block(1)
    for scoring, weighting, tag in ((0, 0, "tfidf_l1"), (5, 0, "tfidf_none"), (0, 2, "idf_l1")):
        out.append(voc_case("voc/8191_on_one_word_" + tag, "8191 features on a word of weight 0.1 (one on a second word): the value is the "
                            "sequential sum, not 8191 * 0.1; scoring %d, weighting %d" % (scoring, weighting), 2, 1, cols, feats, 0,
                            scoring, weighting, flips=["product"] if weighting == 0 else [], expect=dict(count=8191)))
    feats = np.repeat(block(0)[None, :], 8192, 0)
    # all 8192 on the one word: the sequential sum is 819.2000000001177, which only the unnormalised scoring shows (L1 divides it
    # by itself: 1.0; the non-additive weighting keeps the single 0.1 and normalises it to 1.0 as well)
    for scoring, weighting, tag, value in ((0, 0, "tfidf_l1", 1.0), (5, 0, "tfidf_none", 819.2000000001177), (0, 2, "idf_l1", 1.0)):
        out.append(voc_case("voc/8192_on_one_word_" + tag, "8192 features on one word of weight 0.1: the value is %r; scoring %d, "
                            "weighting %d" % (value, scoring, weighting), 2, 1, cols, feats, 0, scoring, weighting,
                            flips=["product"] if scoring == 5 else [], expect=dict(value=value)))
    return out


def code8(v):
    """An 8-bit value in four bytes, each bit repeated four times: the codes of two different values differ by >= 4 bits."""
    bits = np.zeros(32, np.uint8)
    for i in range(8):
        bits[4 * i:4 * i + 4] = (v >> i) & 1
    return np.packbits(bits)


WIDE_K, WIDE_L = 20, 4    # the largest k TemplatedVocabulary::loadFromTextFile (and orbx_vocabulary_create) accepts
_WIDE = []


def wide_level_start(level):
    """Id of the first node of a level in wide_vocabulary's breadth-first order."""
    return sum(WIDE_K ** i for i in range(level))


def wide_vocabulary():
    """k = 20, L = 4: 160 000 words, so that word ids pass 65535, in breadth-first node order -- word w is the leaf reached by
    the children (w // 8000, w // 400 % 20, w // 20 % 20, w % 20).  The child chosen at level l carries code8(child) in bytes
    4 (l - 1) .. 4 l - 1 on top of its parent's descriptor, so the feature made for word w (= that leaf's descriptor) finds the
    right child at every level with all the others at >= 4 bits more."""
    if not _WIDE:
        k, L = WIDE_K, WIDE_L
        n = wide_level_start(L + 1)
        parent, leaf, desc, weight = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n)
        codes = np.stack([code8(v) for v in range(k)])
        for level in range(1, L + 1):
            lo, cnt = wide_level_start(level), k ** level
            par = wide_level_start(level - 1) + np.arange(cnt) // k
            parent[lo:lo + cnt] = par
            desc[lo:lo + cnt] = desc[par]
            desc[lo:lo + cnt, 4 * (level - 1):4 * level] = codes[np.arange(cnt) % k]
        lo = wide_level_start(L)
        leaf[lo:] = 1
        weight[lo:] = 0.5 + (np.arange(n - lo) % 97) / 16.0
        _WIDE.append((parent, leaf, desc, weight))
    return _WIDE[0]


def wide_features(words):
    return wide_vocabulary()[2][wide_level_start(WIDE_L) + np.asarray(words)].copy()


SORT_SIZES = (127, 128, 129, 1024, 1025, 2048, 2049, 8191, 8192)


def sort_words(n, own=False):
    """Word ids in DESCENDING feature order, so that the (word, feature) sort has work to do, on both sides of 65535 (the sort key
    packs a 16-bit feature index under the word id).  own: every feature on its own word; otherwise runs of three share one."""
    i = np.arange(n)
    return 159999 - 19 * i if own else 159999 - 50 * (i // 3)
