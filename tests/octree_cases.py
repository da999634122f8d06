"""Crafted candidate sets for every rule of ORBextractor::DistributeOctTree (src/ORBextractor.cc:490-757) and crafted inputs for the
std::sort replica it depends on, with the two instrumented restatements that say which rule a case reaches:

  distribute_octtree_py   the literal pure-Python restatement (std::list as a Python list), with an optional trace
  introsort_py            a port of csrc/orbx_introsort.h (libstdc++'s introsort), with an optional trace, and the McIlroy
                          adversary that is played against it

tests/test_octree_rules.py asserts on the CPU that every case reaches the rule it was designed for (Case.prop, from the trace) and
that the oracle agrees with the restatement, and on the GPU that k_octree, run alone on these candidates (orbx_debug_octree), gives
the oracle's selection.  tests/test_oracle_octree.py imports the restatement from here.

Geometry: a case is a single pyramid level whose FAST window (level minus the 16-px border) is W x H; candidates are integral
(x, y) relative to the window origin with 3 <= x < W - 3, 3 <= y < H - 3 (the pixels FAST can test), and a response 1 .. 255.
Node depth counts from the roots (depth 0)."""
import ctypes as C
import math

import numpy as np

f32 = np.float32


# ======================================================================================= DistributeOctTree, restated
class Node:
    __slots__ = ("UL", "UR", "BL", "BR", "keys", "no_more", "depth")

    def __init__(self, depth=0):
        self.UL = self.UR = self.BL = self.BR = (0, 0)
        self.keys = []
        self.no_more = False
        self.depth = depth

    def divide(self):
        halfX = int(math.ceil(f32(self.UR[0] - self.UL[0]) / f32(2)))
        halfY = int(math.ceil(f32(self.BR[1] - self.UL[1]) / f32(2)))
        n1, n2, n3, n4 = (Node(self.depth + 1) for _ in range(4))
        n1.UL = self.UL
        n1.UR = (self.UL[0] + halfX, self.UL[1])
        n1.BL = (self.UL[0], self.UL[1] + halfY)
        n1.BR = (self.UL[0] + halfX, self.UL[1] + halfY)
        n2.UL, n2.UR, n2.BL, n2.BR = n1.UR, self.UR, n1.BR, (self.UR[0], self.UL[1] + halfY)
        n3.UL, n3.UR, n3.BL, n3.BR = n1.BL, n1.BR, self.BL, (n1.BR[0], self.BL[1])
        n4.UL, n4.UR, n4.BL, n4.BR = n3.UR, n2.BR, n3.BR, self.BR
        for kp in self.keys:
            if kp[0] < n1.UR[0]:
                (n1 if kp[1] < n1.BR[1] else n3).keys.append(kp)
            elif kp[1] < n1.BR[1]:
                n2.keys.append(kp)
            else:
                n4.keys.append(kp)
        for n in (n1, n2, n3, n4):
            if len(n.keys) == 1:
                n.no_more = True
        return n1, n2, n3, n4


def sort_key(pair, i):
    """The 64-bit element the device sorts for a (size, node) pair: count << 28 | UL.x << 16 | index (csrc/orbx_introsort.h KeyLess)."""
    return (int(pair[0]) << 28) | (int(pair[1].UL[0]) << 16) | i


def std_sort_nodes(oracle, pairs):
    """std::sort(v.begin(), v.end(), compareNodes) on (size, node) pairs via libstdc++ (through the oracle library)."""
    v = np.array([sort_key(p, i) for i, p in enumerate(pairs)], np.uint64)
    oracle.lib().oro_std_sort_keys(v.ctypes.data_as(C.c_void_p), len(v))
    return [pairs[int(x) & 0xFFFF] for x in v]


def stable_sort_nodes(oracle, pairs):
    """What a STABLE sort would give: the foil of the tie cases (never the reference's order where keys tie)."""
    return sorted(pairs, key=lambda p: (p[0], p[1].UL[0]))


def distribute_octtree_py(oracle, keys, minX, maxX, minY, maxY, N, trace=None, sort=std_sort_nodes):
    """keys: list of (x, y, response) with float coordinates relative to the window (integral values).
    trace: a dict that receives
      nIni, dropped (roots without a candidate), single (roots with one), misassigned (candidates given to a root whose rectangle
      [int(hX i), int(hX (i + 1))) does not contain them),
      passes: per phase-1 pass (list size, expandable nodes) after the pass,
      phase2: None, or (nA, nE) of the pass whose nA + 3 nE > N entered it,
      rounds: per phase-2 round dict(keys = the sort's input as (count, UL.x), order = the sorted (count, UL.x), broke = index into
              the sorted array at which the loop broke (None: it ran to the end), size = the list size when it left the loop,
              children = non-empty children of the last node expanded),
      stop: (">=N" | "==prevSize", "phase1" | "phase2"), expandable_left: nodes with more than one candidate in the final list,
      max_split_depth, min_split_w, min_split_h, split_sizes (set of (width, height)): over every node that was divided."""
    t = trace if trace is not None else {}
    nIni = int(math.floor(float(f32(maxX - minX) / f32(maxY - minY)) + 0.5))  # C round(): halves away from zero
    hX = f32(maxX - minX) / f32(nIni)
    lNodes = []
    ini = []
    for i in range(nIni):
        ni = Node()
        ni.UL = (int(hX * f32(i)), 0)
        ni.UR = (int(hX * f32(i + 1)), 0)
        ni.BL = (ni.UL[0], maxY - minY)
        ni.BR = (ni.UR[0], maxY - minY)
        lNodes.append(ni)
        ini.append(ni)
    t.update(nIni=nIni, misassigned=0, passes=[], phase2=None, rounds=[], stop=None, max_split_depth=-1, min_split_w=1 << 30,
             min_split_h=1 << 30, split_sizes=set())
    for kp in keys:
        r = int(f32(kp[0]) / hX)
        ini[r].keys.append(kp)
        if not ini[r].UL[0] <= kp[0] < ini[r].UR[0]:
            t["misassigned"] += 1
    t["dropped"] = [i for i in range(nIni) if not ini[i].keys]
    t["single"] = [i for i in range(nIni) if len(ini[i].keys) == 1]

    def divide(node):
        t["max_split_depth"] = max(t["max_split_depth"], node.depth)
        t["min_split_w"] = min(t["min_split_w"], node.UR[0] - node.UL[0])
        t["min_split_h"] = min(t["min_split_h"], node.BL[1] - node.UL[1])
        t["split_sizes"].add((node.UR[0] - node.UL[0], node.BL[1] - node.UL[1]))
        return node.divide()

    i = 0
    while i < len(lNodes):
        if len(lNodes[i].keys) == 1:
            lNodes[i].no_more = True
            i += 1
        elif not lNodes[i].keys:
            del lNodes[i]
        else:
            i += 1
    finish = False
    size_and_node = []
    while not finish:
        prev_size = len(lNodes)
        i = 0
        n_to_expand = 0
        size_and_node = []
        while i < len(lNodes):
            lit = lNodes[i]
            if lit.no_more:
                i += 1
                continue
            for n in divide(lit):
                if len(n.keys) > 0:
                    lNodes.insert(0, n)  # push_front
                    i += 1
                    if len(n.keys) > 1:
                        n_to_expand += 1
                        size_and_node.append((len(n.keys), n))
            del lNodes[i]  # lit = lNodes.erase(lit)
        t["passes"].append((len(lNodes), n_to_expand))
        if len(lNodes) >= N or len(lNodes) == prev_size:
            finish = True
            t["stop"] = (">=N" if len(lNodes) >= N else "==prevSize", "phase1")
        elif len(lNodes) + n_to_expand * 3 > N:
            t["phase2"] = (len(lNodes), n_to_expand)
            while not finish:
                prev_size = len(lNodes)
                prev = sort(oracle, size_and_node)
                rnd = dict(keys=[(p[0], p[1].UL[0]) for p in size_and_node], order=[(p[0], p[1].UL[0]) for p in prev], broke=None,
                           children=0)
                t["rounds"].append(rnd)
                size_and_node = []
                for j in range(len(prev) - 1, -1, -1):
                    node = prev[j][1]
                    rnd["children"] = 0
                    for n in divide(node):
                        if len(n.keys) > 0:
                            lNodes.insert(0, n)
                            rnd["children"] += 1
                            if len(n.keys) > 1:
                                size_and_node.append((len(n.keys), n))
                    lNodes.remove(node)  # erase(...->lit); Node has identity semantics
                    if len(lNodes) >= N:
                        rnd["broke"] = j
                        break
                rnd["size"] = len(lNodes)
                if len(lNodes) >= N or len(lNodes) == prev_size:
                    finish = True
                    t["stop"] = (">=N" if len(lNodes) >= N else "==prevSize", "phase2")
    t["expandable_left"] = sum(1 for n in lNodes if len(n.keys) > 1)
    t["final"] = len(lNodes)
    out = []
    for node in lNodes:
        best = node.keys[0]
        for kp in node.keys[1:]:
            if kp[2] > best[2]:
                best = kp
        out.append(best)
    return out


# ======================================================================================= std::sort, ported
def introsort_py(v, trace=None, less=None):
    """Port of csrc/orbx_introsort.h: libstdc++'s std::sort on a list of elements; `less` compares two elements (default: the key
    bits 16 .. 63 of an integer).  The walk is the device's (introsort_block): a segment of more than 64 elements is partitioned
    and both halves continue; one of 17 .. 64 is carried through all of its partitions depth first with a stack of the pending
    right-hand segments of more than 16 elements (introsort_seg_reg keeps three).  Sub-ranges are disjoint, so the order of the
    walk does not change the result.  trace receives heapsorts (sizes of the segments handed to heapsort), partitions and
    max_pending (the largest number of pending right-hand segments inside a segment of 64 or fewer)."""
    if less is None:
        less = lambda a, b: (a >> 16) < (b >> 16)
    a = list(v)
    n = len(a)
    t = trace if trace is not None else {}
    t.update(heapsorts=[], partitions=0, max_pending=0)
    if n <= 0:
        return a

    def push_heap(first, hole, top, value):
        parent = (hole - 1) // 2
        while hole > top and less(a[first + parent], value):
            a[first + hole] = a[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        a[first + hole] = value

    def adjust_heap(first, hole, length, value):
        top = hole
        child = hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if (length & 1) == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        push_heap(first, hole, top, value)

    def heapsort(first, last):  # __partial_sort(first, last, last)
        t["heapsorts"].append(last - first)
        length = last - first
        if length >= 2:
            parent = (length - 2) // 2
            while True:
                adjust_heap(first, parent, length, a[first + parent])
                if parent == 0:
                    break
                parent -= 1
        l = last
        while l - first > 1:
            l -= 1
            val = a[l]
            a[l] = a[first]
            adjust_heap(first, 0, l - first, val)

    def partition(first, last):  # __unguarded_partition_pivot
        t["partitions"] += 1
        mid = first + (last - first) // 2
        ia, ib, ic = first + 1, mid, last - 1
        if less(a[ia], a[ib]):
            sel = ib if less(a[ib], a[ic]) else (ic if less(a[ia], a[ic]) else ia)
        elif less(a[ia], a[ic]):
            sel = ia
        else:
            sel = ic if less(a[ib], a[ic]) else ib
        a[first], a[sel] = a[sel], a[first]
        lo, hi = first + 1, last
        while True:
            while less(a[lo], a[first]):
                lo += 1
            hi -= 1
            while less(a[first], a[hi]):
                hi -= 1
            if not lo < hi:
                return lo
            a[lo], a[hi] = a[hi], a[lo]
            lo += 1

    def segment(first, last, depth):  # 17 .. 64 elements: introsort_seg_reg
        stk = []
        f, l, d = first, last, depth
        while True:
            while l - f > 16:
                if d == 0:
                    heapsort(f, l)
                    break
                d -= 1
                cut = partition(f, l)
                if l - cut > 16:
                    stk.append((cut, l, d))
                    t["max_pending"] = max(t["max_pending"], len(stk))
                l = cut
            if not stk:
                return
            f, l, d = stk.pop()

    def walk(first, last, depth):  # introsort_block's tree of partitions
        if last - first <= 16:
            return
        if last - first <= 64:
            segment(first, last, depth)
        elif depth == 0:
            heapsort(first, last)
        else:
            cut = partition(first, last)
            walk(first, cut, depth - 1)
            walk(cut, last, depth - 1)

    walk(0, n, 2 * (n.bit_length() - 1))

    def unguarded_linear_insert(last):
        val = a[last]
        nxt = last - 1
        while less(val, a[nxt]):
            a[last] = a[nxt]
            last = nxt
            nxt -= 1
        a[last] = val

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if less(a[i], a[first]):
                val = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = val
            else:
                unguarded_linear_insert(i)

    if n > 16:  # __final_insertion_sort
        insertion_sort(0, 16)
        for i in range(16, n):
            unguarded_linear_insert(i)
    else:
        insertion_sort(0, n)
    return a


def element(value, index):
    """Sort element of the stand-alone sort cases: key = value + 2 (bits 28 ..), payload = the element's position in the input."""
    return ((int(value) + 2) << 28) | int(index)


def mcilroy_values(n):
    """M. D. McIlroy, "A Killer Adversary for Quicksort" (1999), played against introsort_py: the values 0 .. n - 1 are decided
    while the sort compares them ("gas" items are frozen as late as possible), so that every median-of-three pivot is one of the
    smallest items of its range and the depth budget 2 floor(log2 n) runs out.  Returns value[i] of input position i."""
    gas = n - 1
    val = [gas] * n
    state = dict(nsolid=0, cand=0)

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            if x == state["cand"]:
                val[x] = state["nsolid"]
            else:
                val[y] = state["nsolid"]
            state["nsolid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    introsort_py(list(range(n)), less=less)
    return val


KILLER_SIZES = {40: 20, 64: 40, 100: 76, 128: 100, 300: 268, 1000: 964}   # n -> the segment the port hands to heapsort


def killer_inputs():
    """(name, elements, heapsorted segment): McIlroy inputs for every size of KILLER_SIZES, plain and with ties (value // 3)."""
    out = []
    for n, seg in KILLER_SIZES.items():
        val = mcilroy_values(n)
        out.append(("killer%d" % n, [element(v, i) for i, v in enumerate(val)], seg))
        out.append(("killer%d_tied" % n, [element(v // 3, i) for i, v in enumerate(val)], None))
    return out


def three_pending_inputs(want=3, seed=2024):
    """(name, elements): inputs of 52 .. 64 elements that make introsort_seg_reg hold three pending right-hand segments (17 + 17 + 17
    elements pending and one to the left of them: 52 is the smallest size at which three can exist, four never do) -- found by a
    seeded search with the port, about 3 in 1000 random inputs qualify: `want` permutations of distinct keys and `want` inputs
    with every key about twice."""
    rng = np.random.default_rng(seed)
    out = {False: [], True: []}
    while min(len(out[False]), len(out[True])) < want:
        n = int(rng.integers(52, 65))
        tied = len(out[True]) < len(out[False])
        vals = rng.integers(0, n // 2, n) if tied else rng.permutation(n)
        v = [element(x, i) for i, x in enumerate(vals)]
        tr = {}
        introsort_py(v, tr)
        if tr["max_pending"] >= 3:
            out[tied].append(("pending3_n%d_%s%d" % (n, "tied" if tied else "perm", len(out[tied])), v))
    return out[False] + out[True]


# the final rank of introsort_block deals an element's window to per = 4 / 2 / 1 lanes by 4 n <= nt and 2 n <= nt: both sides of
# both thresholds for nt = 128, 256 and 512, and of the 16 / 64 / 128 limits of the partition forms
RANK_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 500)


def rank_inputs(seed=7):
    """(name, elements): tie-heavy random inputs (n / 4 distinct keys, and two distinct keys) of every size of RANK_SIZES."""
    rng = np.random.default_rng(seed)
    out = []
    for n in RANK_SIZES:
        out.append(("ties%d" % n, [element(v, i) for i, v in enumerate(rng.integers(0, max(2, n // 4), n))]))
        out.append(("two%d" % n, [element(v, i) for i, v in enumerate(rng.integers(0, 2, n))]))
    return out


# ======================================================================================= candidate sets
def cell_grid(W, H):
    """FAST cell grid of a W x H window (src/ORBextractor.cc:901-907): nCols, nRows, wCell, hCell."""
    nCols, nRows = int(W / 35), int(H / 35)
    return nCols, nRows, int(math.ceil(W / nCols)), int(math.ceil(H / nRows))


class Case:
    """One candidate set: window W x H, quota N, pts = [(x, y, response)], and prop(trace, out, case) -> bool, the rule the case
    was designed to reach (why says it in words), evaluated on the restatement's trace and output."""

    def __init__(self, name, W, H, N, pts, why, prop):
        self.name, self.W, self.H, self.N, self.why, self.prop = name, W, H, N, why, prop
        self.stable_differs = None   # True / False: a stable sort in phase 2 must / cannot change the selection (the tie cases)
        self.pts = [(int(x), int(y), int(r)) for x, y, r in pts]
        assert len({(x, y) for x, y, _ in self.pts}) == len(self.pts), name          # FAST never yields a pixel twice
        assert all(3 <= x < W - 3 and 3 <= y < H - 3 and 1 <= r <= 255 for x, y, r in self.pts), name

    def canonical(self):
        """The candidates in the reference's order: cell row, cell column, y, x."""
        _, _, wCell, hCell = cell_grid(self.W, self.H)
        return sorted(self.pts, key=lambda p: ((p[1] - 3) // hCell, (p[0] - 3) // wCell, p[1], p[0]))

    def keys(self):
        return [(float(x), float(y), float(r)) for x, y, r in self.canonical()]

    def __repr__(self):
        return "Case(%s)" % self.name


def _rand(rng, n, x0, x1, y0, y1, taken=()):
    """n distinct random pixels of [x0, x1) x [y0, y1) that are not in `taken`, with responses 7 .. 59 (few distinct values)."""
    have = {(x, y) for x, y, *_ in taken}
    out = []
    assert (x1 - x0) * (y1 - y0) >= n + len(have)
    while len(out) < n:
        p = (int(rng.integers(x0, x1)), int(rng.integers(y0, y1)))
        if p not in have:
            have.add(p)
            out.append(p + (int(rng.integers(7, 60)),))
    return out


def _resp(rng, pts):
    return [(x, y, int(rng.integers(7, 60))) for x, y in pts]


# ---- roots (cases 1 - 2): one window per root count; 3 .. 8 (and 2) with a fractional hX
ROOT_WINDOWS = {1: (60, 50), 2: (101, 50), 3: (100, 38), 4: (150, 38), 5: (191, 38), 6: (230, 38), 7: (265, 38), 8: (300, 38)}
ROOT_N = 40


def _root_cases():
    out = []
    for n, (W, H) in ROOT_WINDOWS.items():
        rng = np.random.default_rng(100 + n)
        hX = f32(W) / f32(n)
        edge = [int(hX * f32(i)) for i in range(n + 1)]
        inside = lambda i: (max(edge[i] + 1, 3), min(edge[i + 1] - 1, W - 3))   # x range that is root i's by any reading
        ys = (3, 11, H // 2, H - 4)
        if n == 1:
            out.append(Case("roots1_random", W, H, ROOT_N, _rand(rng, 120, 3, W - 3, 3, H - 3), "one root",
                            lambda t, o, c: t["nIni"] == 1 and not t["dropped"]))
            out.append(Case("one_candidate", W, H, ROOT_N, [(31, 17, 9)], "one candidate: the root is bNoMore from the start",
                            lambda t, o, c: t["single"] == [0] and t["final"] == 1))
            out.append(Case("no_candidate", W, H, ROOT_N, [], "no candidate: every root is dropped",
                            lambda t, o, c: t["dropped"] == [0] and t["final"] == 0))
            continue
        pts = _resp(rng, [(edge[i] + d, y) for i in range(1, n) for d in (-1, 0, 1) for y in ys])
        pts += _rand(rng, 40, 3, W - 3, 3, H - 3, pts)
        out.append(Case("roots%d_bounds" % n, W, H, ROOT_N, pts,
                        "%d roots, hX = %s: candidates on and beside every inner root boundary; some belong to a root whose "
                        "rectangle excludes them" % (n, hX),
                        lambda t, o, c, n=n: t["nIni"] == n and t["misassigned"] >= 1 and not t["dropped"]))
        last = _rand(rng, 25, *inside(n - 1), 3, H - 3)
        if n == 2:
            out.append(Case("roots2_single", W, H, ROOT_N, [(20, 20, 30)] + last, "root 0 holds one candidate (bNoMore from the start)",
                            lambda t, o, c: t["single"] == [0] and not t["dropped"]))
            out.append(Case("roots2_last", W, H, ROOT_N, last, "root 0 is empty (dropped), every candidate in the last root",
                            lambda t, o, c: t["dropped"] == [0]))
        else:
            out.append(Case("roots%d_sparse" % n, W, H, ROOT_N, [(inside(1)[0] + 2, 20, 30)] + last,
                            "root 0 empty (dropped), root 1 with one candidate (bNoMore from the start), the rest in the last root",
                            lambda t, o, c, n=n: t["dropped"] == [0] + list(range(2, n - 1)) and t["single"] == [1]))
            out.append(Case("roots%d_last" % n, W, H, ROOT_N, last, "every candidate in the last root, all others dropped",
                            lambda t, o, c, n=n: t["dropped"] == list(range(n - 1))))
    W, H = ROOT_WINDOWS[8]
    hX = f32(W) / f32(8)
    out.append(Case("fewer_than_roots", W, H, ROOT_N, [(int(hX * f32(i)) + 9, 7 + i, 20 + i) for i in (1, 4, 6)],
                    "three candidates in three of eight roots",
                    lambda t, o, c: t["single"] == [1, 4, 6] and t["final"] == 3))
    # the last, partial cell column of a two-root window (2 x 51 > 101): the histogram variant decodes the winner's pixel
    W, H = ROOT_WINDOWS[2]
    rng = np.random.default_rng(110)
    pts = _resp(rng, [(W - 4, H - 4), (W - 4, 3), (W - 5, H - 5), (3, H - 4), (3, 3)])
    pts += _rand(rng, 20, W - 12, W - 3, 3, H - 3, pts)
    out.append(Case("partial_cells_two_roots", W, H, ROOT_N, pts, "candidates in the last pixels of the partial last cell column",
                    lambda t, o, c: (c.W - 4, c.H - 4) in {(int(k[0]), int(k[1])) for k in o} and cell_grid(c.W, c.H)[0] * cell_grid(c.W, c.H)[2] > c.W))
    return out


# ---- DivideNode edges and the early stop (cases 3 - 4): a 250 x 250 window (node sides 250, 125, 63 / 62, 32 / 31, 16, ...)
EDGE_W = EDGE_H = 250
EDGE_N = 120


def _sep_width(lo, hi, a):
    """Width of the node whose division separates pixel a from a + 1 along one axis of a root [lo, hi)."""
    while True:
        mid = lo + (hi - lo + 1) // 2
        if a < mid <= a + 1:
            return hi - lo
        lo, hi = (lo, mid) if a + 1 < mid else (mid, hi)


def _chain(maxd, turns=(3, 0, 1, 2, 3, 0, 1, 2)):
    """The four pixels around the split point of a node (mid - 1 and mid of x and of y), for a chain of nodes of depth 0 .. maxd
    that descends into child turns[d]."""
    x0, x1, y0, y1 = 0, EDGE_W, 0, EDGE_H
    pts = []
    for d in range(maxd + 1):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        pts += [(mx - 1, my - 1), (mx, my - 1), (mx - 1, my), (mx, my)]
        q = turns[d]
        x0, x1 = (mx, x1) if q & 1 else (x0, mx)
        y0, y1 = (my, y1) if q & 2 else (y0, my)
    return list(dict.fromkeys(pts))


def _edge_cases():
    rng = np.random.default_rng(3)
    out = []
    deep = _chain(6)
    ax = next(a for a in range(20, 60) if _sep_width(0, EDGE_W, a) == 2)
    ay = next(a for a in range(200, 240) if _sep_width(0, EDGE_H, a) == 2)
    deep += [(ax, 215), (ax + 1, 215), (30, ay), (30, ay + 1)]   # 1 px apart in x only / in y only
    parity = lambda t: {(w & 1, h & 1) for w, h in t["split_sizes"]}
    out.append(Case("divide_deep", EDGE_W, EDGE_H, EDGE_N, _resp(rng, deep),
                    "mid - 1 / mid of x and y of the nodes of depth 0 .. 6 of one chain, odd and even sides, and two pairs 1 px apart "
                    "that only a node of width / height 2 separates: the histogram variant (depth <= 5) must fall back",
                    lambda t, o, c: t["max_split_depth"] > 5 and t["min_split_w"] == 2 and t["min_split_h"] == 2 and
                    t["final"] == len(c.pts) and {(0, 0), (1, 1)} <= parity(t)))
    out.append(Case("divide_depth5", EDGE_W, EDGE_H, EDGE_N, _resp(rng, _chain(4)),
                    "a shorter chain whose deepest division is of a depth-5 node: the first depth the histogram variant cannot split",
                    lambda t, o, c: t["max_split_depth"] == 5 and t["final"] == len(c.pts)))
    out.append(Case("divide_depth4", EDGE_W, EDGE_H, EDGE_N, _resp(rng, _chain(3)),
                    "a shorter chain whose deepest division is of a depth-4 node: the histogram variant serves it",
                    lambda t, o, c: t["max_split_depth"] == 4 and t["final"] == len(c.pts)))
    out.append(Case("early_stop_phase1", EDGE_W, EDGE_H, EDGE_N, _resp(rng, [(30, 30), (31, 33), (34, 31), (36, 36), (33, 38)]),
                    "every candidate in one quadrant of the root: the pass leaves one node, size == prevSize ends the loop",
                    lambda t, o, c: t["stop"] == ("==prevSize", "phase1") and t["final"] < c.N and t["final"] < len(c.pts) and
                    t["expandable_left"] > 0))
    return out


# ---- phase 1 / phase 2 (cases 5 - 8): a 256 x 256 window, whose nodes of depth g are the equal squares of a 2^g x 2^g grid
GRID_W = GRID_H = 256


def _square_pts(rng, g, sx, sy, spec):
    """Candidates of square (sx, sy) of the depth-g grid.  spec = a count: that many random pixels of the square; or a list of
    quadrant sets [Q1, Q2, ...]: one pixel for every path q1 in Q1, q2 in Q2, ... below the square (a node of depth g + j in such
    a path has len(Qj+1) non-empty children), in the top-left corner of the path's last node."""
    S = GRID_W >> g
    ox, oy = sx * S, sy * S
    if isinstance(spec, int):
        return _rand(rng, spec, max(ox, 3), min(ox + S, GRID_W - 3), max(oy, 3), min(oy + S, GRID_H - 3))
    paths = [(ox, oy)]
    for j, Q in enumerate(spec):
        s = S >> (j + 1)
        paths = [(x + (q & 1) * s, y + (q >> 1) * s) for x, y in paths for q in sorted(Q)]
    return _resp(rng, [(max(x, 3), max(y, 3)) for x, y in paths])


def grid_case(name, N, g, squares, why, prop, seed=1):
    """squares: {(sx, sy): spec} over the depth-g grid (see _square_pts); squares not named hold ONE candidate, so that every pass
    of phase 1 down to depth g divides every node into four and the list has 4^g nodes when depth g is reached."""
    rng = np.random.default_rng(seed)
    G = 1 << g
    pts = []
    for sx in range(G):
        for sy in range(G):
            pts += _square_pts(rng, g, sx, sy, squares.get((sx, sy), 1))
    return Case(name, GRID_W, GRID_H, N, pts, why, prop)


def column_major(g, m):
    """The first m squares of the depth-g grid, column by column (squares of a column share UL.x)."""
    G = 1 << g
    return [(i // G, i % G) for i in range(m)]


A4, Q3, Q2 = {0, 1, 2, 3}, {0, 1, 2}, {0, 3}
# expandable squares of the depth-3 grid, each in a column of its own (distinct UL.x: no tied keys).  (children, candidates) per spec:
SPEC = {(4, 16): [A4, A4], (4, 12): [A4, Q3], (4, 8): [A4, Q2], (4, 4): [A4], (3, 9): [Q3, Q3], (3, 6): [Q3, Q2], (3, 3): [Q3],
        (2, 4): [Q2, Q2], (2, 2): [Q2]}
DIAGONAL = [(i, (3 * i) % 8) for i in range(8)]


def _designed(name, N, specs, why, prop):
    """A depth-3 grid (64 nodes after three passes of phase 1) whose expandable squares are `specs` = [(non-empty children,
    candidates)], largest first: phase 2 expands them in that order, the list grows by children - 1 each."""
    squares = {sq: SPEC[s] if isinstance(s, tuple) else s for sq, s in zip(DIAGONAL, specs)}
    return grid_case(name, N, 3, squares, why, prop)


def _threshold_cases():
    base = [(4, 16), (4, 12), (3, 9), (4, 8), (3, 6), (2, 4), (3, 3), (2, 2)]   # the list grows 64 -> 67 70 72 75 77 78 80 81
    r1 = lambda t: t["rounds"][0]
    entered = lambda t: t["phase2"] == (64, len(r1(t)["keys"]))
    out = [
        # ---- case 5
        _designed("threshold_equal", 88, base, "after pass 3 nA + 3 nE = 64 + 24 == N: phase 1 runs another pass",
                  lambda t, o, c: t["passes"][2] == (64, 8) and len(t["passes"]) >= 4 and t["phase2"] != (64, 8)),
        _designed("threshold_enter", 87, base, "nA + 3 nE = 88 == N + 1: phase 2 is entered after pass 3",
                  lambda t, o, c: t["passes"][2] == (64, 8) and t["phase2"] == (64, 8)),
        _designed("phase1_exact", 64, base, "nA == N exactly after pass 3 of phase 1",
                  lambda t, o, c: t["stop"] == (">=N", "phase1") and t["passes"][-1][0] == 64 == t["final"] and len(t["passes"]) == 3),
        # ---- case 6: where phase 2 breaks
        _designed("break_exact", 78, base, "the node that reaches N has 2 non-empty children: the list ends with exactly N nodes",
                  lambda t, o, c: entered(t) and r1(t)["children"] == 2 and t["final"] == c.N and r1(t)["broke"] not in (None, 0, 7)),
        _designed("break_over1", 78, base[:5] + [(3, 3), (2, 2)], "the node expanded at N - 1 nodes has 3 non-empty children: N + 1",
                  lambda t, o, c: entered(t) and r1(t)["children"] == 3 and t["final"] == c.N + 1),
        _designed("break_over2", 78, base[:5] + [(4, 4), (2, 2)], "the node expanded at N - 1 nodes has 4 non-empty children: N + 2, "
                  "the most a list can hold (the parent leaves before the size is tested)",
                  lambda t, o, c: entered(t) and r1(t)["children"] == 4 and t["final"] == c.N + 2),
        _designed("break_first", 66, base, "the first node expanded (the last of the sorted array) reaches N",
                  lambda t, o, c: entered(t) and r1(t)["broke"] == len(r1(t)["keys"]) - 1 == 7),
        _designed("break_last_of_two", 66, [(2, 4), (2, 2)], "the last node expanded (the first of the sorted array) reaches N",
                  lambda t, o, c: entered(t) and r1(t)["broke"] == 0 and len(r1(t)["keys"]) == 2 and t["final"] == c.N),
        _designed("break_single", 66, [(3, 3)], "a sorted array of one node",
                  lambda t, o, c: entered(t) and r1(t)["broke"] == 0 and len(r1(t)["keys"]) == 1 and t["final"] == c.N),
        _designed("break_last_of_eight", 84, [(4, 16), (4, 16), (4, 12), (4, 12), (4, 8), (4, 8), (2, 4), (2, 2)],
                  "the last of eight nodes reaches N", lambda t, o, c: entered(t) and r1(t)["broke"] == 0 and t["final"] == c.N),
        _designed("two_rounds", 84, base, "round 1 expands every node without reaching N; round 2 sorts their 20 children",
                  lambda t, o, c: entered(t) and len(t["rounds"]) == 2 and r1(t)["broke"] is None and
                  t["rounds"][1]["broke"] is not None and t["max_split_depth"] == 4),
        _designed("three_rounds", 80, [[Q2, Q2, Q2]] + [[{0}, {0}, A4]] * 7,
                  "seven nodes keep all their candidates in one child for two rounds (the list grows by 1, then by 2): a third round, "
                  "which divides nodes of depth 5",
                  lambda t, o, c: entered(t) and len(t["rounds"]) == 3 and [r["broke"] is None for r in t["rounds"]] == [True, True, False]
                  and t["max_split_depth"] == 5),
    ]
    # ---- case 4: the early stop inside phase 2
    rng = np.random.default_rng(4)
    clusters = [p for ox, oy in ((20, 20), (150, 20), (20, 150), (150, 150)) for p in _rand(rng, 5, ox, ox + 6, oy, oy + 6)]
    out.append(Case("early_stop_phase2", GRID_W, GRID_H, 10, clusters,
                    "four nodes, each with its candidates in one child: round 1 of phase 2 leaves the list size unchanged",
                    lambda t, o, c: t["phase2"] == (4, 4) and len(t["rounds"]) == 1 and t["stop"] == ("==prevSize", "phase2") and
                    t["final"] == 4 < c.N and t["expandable_left"] == 4))
    # ---- case 7: more quota than candidates, and the large quota
    allnodes = lambda t, o, c: t["final"] == len(c.pts) < c.N and t["stop"][0] == "==prevSize" and t["expandable_left"] == 0
    rng = np.random.default_rng(7)
    out.append(Case("all_nodes_small", GRID_W, GRID_H, 60, _rand(rng, 40, 3, 253, 3, 253), "N > candidates: each becomes a node", allnodes))
    out.append(Case("all_nodes_800", GRID_W, GRID_H, 800, _rand(rng, 300, 3, 253, 3, 253), "N = 800 > candidates: each becomes a node", allnodes))
    out.append(Case("reach_800", GRID_W, GRID_H, 800, _rand(rng, 3000, 3, 253, 3, 253), "3000 candidates, N = 800 is reached",
                    lambda t, o, c: t["final"] >= 800 and t["stop"][0] == ">=N"))
    # ---- case 10: the last, partial cell column and row (7 x 37 = 259 > 256)
    pts = _resp(rng, [(252, 252), (252, 3), (3, 252), (251, 250), (225, 225), (224, 224), (252, 224), (224, 252), (3, 3), (140, 140), (200, 140), (140, 200)])
    pts += _rand(rng, 12, 225, 253, 225, 253, pts)
    pts += _rand(rng, 12, 3, 253, 3, 253, pts)   # (spread: a pass that divides no node into two would end the loop early)
    out.append(Case("partial_cells", GRID_W, GRID_H, 60, pts, "candidates up to the last detectable pixel of the partial last cells",
                    lambda t, o, c: allnodes(t, o, c) and cell_grid(c.W, c.H)[2] * cell_grid(c.W, c.H)[0] > c.W and
                    {(252, 252), (252, 3), (3, 252)} <= {(int(k[0]), int(k[1])) for k in o}))
    return out


# ---- the sort inside the quadtree (case 8): phase-2 lists of SORT_SIZES expandable nodes with heavily tied keys.  Lists of up to 64
# nodes come from the depth-3 grid (64 nodes when phase 2 starts, N in (64, 64 + 3 m)), longer ones from the depth-4 grid (256).
SORT_SIZES = (16, 17, 32, 33, 64, 65, 128, 129, 250)
SORT_VARIANTS = ("equal", "two", "column")
# N per list size, shared by the three variants (one batch): found by a search over (nodes, nodes + 3 m) for a quota at which, in
# every variant, round 1 breaks between two nodes of equal key AND a stable sort would select other nodes
SORT_N = {16: 79, 17: 81, 32: 99, 33: 104, 64: 126, 65: 326, 128: 398, 129: 390, 250: 503}


def sort_squares(m, variant, seed):
    """Candidates per expandable square, column by column: "equal" = 3 everywhere (the keys of a column of squares tie); "two" = 2
    or 3 at random; "column" = one count per column, 2 + column % 3."""
    g = 3 if m <= 64 else 4
    rng = np.random.default_rng(seed)
    sq = column_major(g, m)
    if variant == "equal":
        return g, {s: 3 for s in sq}
    if variant == "two":
        return g, {s: int(rng.integers(2, 4)) for s in sq}
    return g, {s: 2 + s[0] % 3 for s in sq}


def _tied_break(t):
    """Round 1 broke at sorted index j with an equal key next to it on the side still to be expanded or just expanded."""
    r = t["rounds"][0]
    j, o = r["broke"], r["order"]
    return j is not None and ((j > 0 and o[j - 1] == o[j]) or (j + 1 < len(o) and o[j + 1] == o[j]))


def sort_case(m, variant, N):
    g, squares = sort_squares(m, variant, 1000 + m)
    c = grid_case("sort%d_%s" % (m, variant), N, g, squares,
                  "phase 2 sorts %d nodes with tied keys and breaks inside a run of equal keys: the tie order of std::sort "
                  "decides which nodes are divided" % m,
                  lambda t, o, c, m=m, g=g: t["phase2"] == (4 ** g, m) and _tied_break(t), seed=m)
    c.stable_differs = m > 16   # (std::sort of up to 16 elements is one insertion sort, which is stable)
    return c


def _monotone_cases():
    """One list strictly descending and one strictly ascending in creation order (33 nodes with 2 .. 34 candidates)."""
    g, m = 3, 33
    sq = column_major(g, m)
    probe = grid_case("probe", 100, g, {s: 2 + i for i, s in enumerate(sq)}, "", None)
    t = {}
    distribute_octtree_py(None, probe.keys(), 16, 16 + GRID_W, 16, 16 + GRID_H, 100, t, sort=stable_sort_nodes)
    created = [sq[k[0] - 2] for k in t["rounds"][0]["keys"]]   # the squares in the order phase 1 created their nodes
    out = []
    for name, counts in (("descending", range(34, 1, -1)), ("ascending", range(2, 35))):
        mono = (lambda k: all(a > b for a, b in zip(k, k[1:]))) if name == "descending" else (lambda k: all(a < b for a, b in zip(k, k[1:])))
        out.append(grid_case("sort33_" + name, 100, g, dict(zip(created, counts)), "the sort's input is strictly %s" % name,
                             lambda t, o, c, mono=mono: t["phase2"] == (64, 33) and mono(t["rounds"][0]["keys"])))
    return out


def _sort_cases():
    return [sort_case(m, v, SORT_N[m]) for m in SORT_SIZES for v in SORT_VARIANTS] + _monotone_cases()


# ---- winner per node (case 9): 256 x 256, cells of 37 x 37 from pixel 3 (cell column c = (x - 3) // 37); N = 4, so the four nodes of
# depth 1 are final and each holds one tie.  The reference keeps the FIRST maximum in its candidate order (cell row, cell column, y, x).
def _by_yx_winners(case, out):
    """Winners if ties went to the smallest (y, x) instead: the foil."""
    res = []
    for k in out:
        node = [p for p in case.pts if (p[0] >= 128) == (k[0] >= 128) and (p[1] >= 128) == (k[1] >= 128)]
        m = max(p[2] for p in node)
        res.append(min((p for p in node if p[2] == m), key=lambda p: (p[1], p[0]))[:2])
    return res


def _winner_cases():
    low = lambda rng, ox, oy: [(x, y, int(rng.integers(1, 40))) for x, y, _ in _rand(rng, 6, ox, ox + 20, oy + 50, oy + 70)]
    rng = np.random.default_rng(9)
    won = lambda o: {(int(k[0]), int(k[1])) for k in o}
    a = [(76, 30, 50), (77, 10, 50)]            # cell columns 1 | 2 of cell row 0: the first in order has the LARGER y
    b = [(200, 39, 60), (150, 40, 60)]          # cell rows 0 | 1: the first in order has the larger x
    c3 = [(39, 180, 70), (40, 170, 70), (41, 160, 70)]       # cell columns 0 | 1 | 1 of cell row 4, y descending
    d = [(187, 210, 255), (188, 195, 255), (170, 200, 254)]  # cell columns 4 | 5 of cell row 5: the maximum response tied with itself
    out = [Case("winner_cell_order", GRID_W, GRID_H, 4, a + b + c3 + d + low(rng, 10, 10) + low(rng, 140, 10) + low(rng, 10, 140) +
                low(rng, 140, 140), "equal maxima in one final node whose first candidate in reference order is not the one with "
                "the smallest y: across cell columns, across cell rows, three ways, and at response 255",
                lambda t, o, c: t["final"] == 4 and won(o) == {(76, 30), (200, 39), (39, 180), (187, 210)} and
                sorted(_by_yx_winners(c, o)) != sorted(won(o)))]
    e = [(113, 20, 1), (114, 5, 1), (60, 60, 1)]             # cell columns 2 | 3: every candidate of the node has response 1
    f = [(225, 100, 9), (224, 101, 9), (223, 102, 9), (226, 99, 9)]   # cell columns 5 | 6 (x = 225 is the first pixel of 6)
    out.append(Case("winner_low_responses", GRID_W, GRID_H, 4, e + f + c3 + d, "a node whose candidates all have response 1, four equal "
                    "responses over a cell boundary",
                    lambda t, o, c: t["final"] == 4 and won(o) == {(113, 20), (224, 101), (39, 180), (187, 210)} and
                    sorted(_by_yx_winners(c, o)) != sorted(won(o))))
    return out


# ---- the two forms of the histogram variant's sweep (case 11): two roots, 669 x 288, hX = 334.5
TAB_W, TAB_H = 669, 288


def _table_cases():
    rng = np.random.default_rng(11)
    pts = _resp(rng, [(333 + d, y) for d in (0, 1, 2) for y in (3, 100, 143, 144, 284)])
    pts += _rand(rng, 500, 3, TAB_W - 3, 3, TAB_H - 3, pts)
    prop = lambda t, o, c: t["nIni"] == 2 and t["misassigned"] >= 1 and t["max_split_depth"] < 5 and t["final"] >= c.N
    return [Case("path_arithmetic", TAB_W, TAB_H, 20, pts, "N = 20: the path-code tables do not fit, the sweep computes the paths", prop),
            Case("path_tables", TAB_W, TAB_H, 100, pts, "N = 100: the same candidates through the per-coordinate tables", prop)]


_CASES = None


def all_cases():
    """Every quadtree case, built once."""
    global _CASES
    if _CASES is None:
        _CASES = _root_cases() + _edge_cases() + _threshold_cases() + _sort_cases() + _winner_cases() + _table_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def groups():
    """{(W, H, N): cases}: the cases one single-level extractor (window W x H, nfeatures N) serves."""
    out = {}
    for c in all_cases():
        out.setdefault((c.W, c.H, c.N), []).append(c)
    return out


def batches(cases):
    """Batches of three images for the device: three DIFFERENT cases of the group where it has three; a smaller group's batch is
    completed with its own cases again (their candidates arrive in another order)."""
    n = max(3, len(cases))
    return [[cases[(i + j) % len(cases)] for j in range(3)] for i in range(0, n, 3)]


def device_order(case, slot, seed=5):
    """The candidates of a case as the device entry receives them in image `slot` of a batch: shuffled, in slot 1 the reference's
    order reversed (the entry takes any order; ties are broken by position, never by arrival)."""
    pts = case.canonical()
    if slot == 1:
        return pts[::-1]
    rng = np.random.default_rng(seed + slot)
    return [pts[i] for i in rng.permutation(len(pts))]
