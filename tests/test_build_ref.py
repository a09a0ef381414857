"""tests/build_ref.py, the sequential restatement of the device BVH builders, held to account before anything is held to it:
answers worked out by hand (not by running either implementation), tree_audit's strict audit over every tree it builds for the
meshes of tests/test_gpu_build_ref.py, and Karras' hierarchy against a naive top-down recursion.  No GPU.

Where a key bit lands (worked out from "x y z x y z s, most significant first", 18 bits per axis and 9 size bits in 63): the key
is nine groups of seven bits; group g = 0..8 from the top holds bits 17 - 2g and 16 - 2g of x, y, z and size bit 8 - g.  So size bit b
is key bit 7b, and bit v of axis a (x = 0) is key bit 7 * (8 - g) + 6 - (3 * ((17 - v) % 2) + a) with g = (17 - v) // 2."""
import numpy as np
import pytest

import build_ref as br
import tree_audit as ta
from gpu_support import BUILDER_ASSETS, builder_mesh

F32 = np.float32
MESHES = BUILDER_ASSETS + ("needles",) + br.SYNTHETIC
PRESPLIT = [(name, ps) for name in ("needles", "gto_sixteen", "two-scales", "needles-63", "needles-64") for ps in (50, 200)]


def bits(*positions):
    return sum(1 << p for p in positions)


def arrays(name):
    return lambda: builder_mesh(name)[1:3]


def device_kw(leaf_max):
    return dict(leaf_max=max(leaf_max, 1), cut_subtrees=True, depth_exact=leaf_max <= 1)


# --------------------------------------------------------------------------------------------------------------- the key
def test_keys_worked_out_by_hand():
    """Centre bounds (0,0,0)..(1,1,1), so the squared scene diagonal is 3 and u is the centre itself.
      box 0  a point at the lower corner: every q is 0, rel 0 -> key 0
      box 1  centre (1,1,1), extents 2: u == 1 gives 262144, clamped to 262143; rel = sqrt(12 / 3) = 2, clamped to 1 -> 512, clamped
             to 511: every bit of the key is set
      box 2  centre (.5,.5,.5), extents 1: q = 2^17 on every axis (key bits 62, 61, 60); rel = sqrt(3 / 3) = 1 exactly -> 511 again
      box 3  centre (.25,.5,.75), extents .5: x = 2^16 (key bit 59), y = 2^17 (61), z = 2^17 + 2^16 (60, 57); rel = sqrt(.75 / 3) = .5 -> 256,
             size bit 8 = key bit 56
      box 4  centre (.75,.125,0), extents (.25,.25,0): x = 2^17 + 2^16 (62, 59), y = 2^15 (group 1, first triple: 7 * 7 + 6 - 1 = 54), z = 0;
             rel = sqrt(.125 / 3) = .2041 -> 104.5 -> 104 = 64 + 32 + 8: size bits 6, 5, 3 = key bits 42, 35, 21"""
    tbox = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 2, 2, 2], [0, 0, 0, 1, 1, 1], [0, .25, .5, .5, .75, 1], [.625, 0, 0, .875, .25, 0]], F32)
    q, qs = br.quantise(tbox)
    assert q.tolist() == [[0, 0, 0], [262143] * 3, [131072] * 3, [65536, 131072, 196608], [196608, 32768, 0]]
    assert qs.tolist() == [0, 511, 511, 256, 104]
    size_all = bits(*range(0, 63, 7))
    want = [0, (1 << 63) - 1, bits(62, 61, 60) | size_all, bits(59, 61, 60, 57, 56), bits(62, 59, 54, 42, 35, 21)]
    assert [int(k) for k in br.morton_keys(tbox)] == want


def test_key_with_a_zero_extent_axis():
    """Every centre has z = .5: ext.z is 0, u.z is 0 by the rule (no division), and the squared scene diagonal is 1 + 1 + 0.  The
    point box in the middle has rel 0 and q = (2^17, 2^17, 0): key bits 62 and 61."""
    tbox = np.array([[0, 0, .5, 0, 0, .5], [1, 1, .5, 1, 1, .5], [.5, .5, .5, .5, .5, .5]], F32)
    assert [int(k) for k in br.morton_keys(tbox)] == [0, bits(*[p for g in range(9) for p in (7 * g + 6, 7 * g + 5, 7 * g + 3, 7 * g + 2)]), bits(62, 61)]


def test_plain_morton_key_at_size_bits_0():
    """21 bits per axis, bit v of axis a at key bit 3v + 2 - a; no size bits.  (.5,.5,.5) -> 2^20 each: 62, 61, 60;
    (.25,.5,.75) -> x = 2^19 (59), y = 2^20 (61), z = 2^20 + 2^19 (60, 57); the corner at (1,1,1) clamps to 2^21 - 1: all 63 bits."""
    tbox = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 2, 2, 2], [0, 0, 0, 1, 1, 1], [0, .25, .5, .5, .75, 1]], F32)
    assert [int(k) for k in br.morton_keys(tbox, size_bits=0)] == [0, (1 << 63) - 1, bits(62, 61, 60), bits(59, 61, 60, 57)]


def test_the_sort_is_stable():
    order, keys = br.sort_keys(np.array([5, 3, 5, 3, 1], np.uint64))
    assert order.tolist() == [4, 1, 3, 0, 2] and keys.tolist() == [1, 3, 3, 5, 5]


# ---------------------------------------------------------------------------------------------------------------- Karras
def test_karras_on_eight_keys_with_three_equal():
    """Keys 00001 00010 00100 00100 00100 00101 11000 11001.  Top down: bit 4 splits [0..5 | 6 7]; bit 2 splits [0 1 | 2..5]; bit 0
    splits [2 3 4 | 5]; the three equal keys go on into their positions 010 011 100: [2 3 | 4], then [2 | 3].  In Karras' numbering an
    inner child carries the number of the split position on its own side (left: gamma, right: gamma + 1)."""
    left, right, first, last = br.karras(np.array([1, 2, 4, 4, 4, 5, 24, 25], np.uint64))
    assert left.tolist() == [5, ~0, 4, ~2, 3, 1, ~6]
    assert right.tolist() == [6, ~1, ~5, ~3, ~4, 2, ~7]
    assert first.tolist() == [0, 0, 2, 2, 2, 0, 6] and last.tolist() == [7, 1, 5, 3, 4, 5, 7]
    assert br.delta([4, 4, 4], 0, 2) == 64 + 30 and br.delta([4, 4], 0, 1) == 64 + 31 and br.delta([4, 5], 0, 1) == 63 and br.delta([4], 0, 1) == -1


def naive_tree(keys, lo, hi):
    """Top-down over (key, position): split where the highest differing bit of the first and the last flips."""
    if lo == hi:
        return lo
    aug = [(int(keys[p]) << 32) | p for p in range(lo, hi + 1)]
    top = (aug[0] ^ aug[-1]).bit_length() - 1
    split = next(p for p in range(lo, hi) if (aug[p - lo + 1] >> top) & 1)
    return (naive_tree(keys, lo, split), naive_tree(keys, split + 1, hi))


def nested(left, right, c=0):
    return ~c if c < 0 else (nested(left, right, int(left[c])), nested(left, right, int(right[c])))


@pytest.mark.parametrize("name", ["soup-257", "pairs", "co-centred"])
def test_karras_equals_the_naive_recursion(name):
    verts, tris = builder_mesh(name)[1:3]
    _, keys = br.sort_keys(br.morton_keys(br.tri_boxes(verts, tris)))
    left, right, first, last = br.karras(keys)
    assert nested(left, right) == naive_tree(keys, 0, len(keys) - 1)
    assert first[0] == 0 and last[0] == len(keys) - 1


# ------------------------------------------------------------------------------------------------------------------ PLOC
def slabs(intervals):
    """Boxes with a unit cross-section over x intervals: the union's area is 4 dx + 2, so the nearest neighbour is the one with
    the shortest common interval, and equal lengths are exact ties."""
    return np.array([[a, 0, 0, b, 1, 1] for a, b in intervals], F32)


SIX = [(0, 1), (2, 3), (4, 5), (5.5, 6.5), (7, 8), (9.5, 10.5)]


def test_ploc_round_with_a_tie_and_a_non_mutual_choice():
    """0 -> 1 (3 against 5).  1: [0,3] and [2,5] are both 3 long: the tie goes to position 0.  2 -> 3 (2.5 against 3).  3: [4,6.5] and
    [5.5,8] are both 2.5 long: position 2.  4 -> 3 (2.5 against 3.5) although 3 chose 2; 5 -> 4 although 4 chose 3.  Merges: (0,1), (2,3)."""
    nn = br.ploc_neighbours(slabs(SIX))
    assert nn.tolist() == [1, 0, 3, 2, 3, 4]
    i, j = br.ploc_pairs(nn)
    assert (i.tolist(), j.tolist()) == ([0, 2], [1, 3])
    assert br.ploc_neighbours(slabs(SIX), radius=1).tolist() == [1, 0, 3, 2, 3, 4]
    assert br.ploc_neighbours(slabs([(0, 1), (50, 51), (1, 2)]), radius=1).tolist() == [1, 2, 1]      # the window, not the whole array


def test_the_window_case_tells_7_8_and_9_apart():
    """build_ref.case_soup("window"): sticks at positions 0, 8 and 17 among plates, in x order.  Window 8: sticks 0 and 8 choose each
    other (a plate costs 16 x 16 and more).  Window 7: stick 0 sees plates only and takes the nearest, 1; stick 8 takes plate 9 (1/64
    away, plate 7 is 10/64 away).  Window 9: stick 8 also sees stick 17, 9/64 away against 48/64: (8, 17) choose each other."""
    H = br.prepare(*br.soup_arrays(br.case_soup("window")), 0)
    assert H.val.tolist() == list(range(18)) and np.all(br.quantise(H.tbox)[1] == 511)
    nn = {r: br.ploc_neighbours(H.tbox, radius=r) for r in (7, 8, 9)}
    assert (nn[8][0], nn[8][8]) == (8, 0) and nn[8][17] == 16
    assert (nn[7][0], nn[7][8]) == (1, 9)
    assert (nn[9][0], nn[9][8], nn[9][17]) == (8, 17, 8)
    pairs = {r: set(zip(*(x.tolist() for x in br.ploc_pairs(nn[r])))) for r in (7, 8, 9)}
    assert [((0, 8) in pairs[r], (8, 17) in pairs[r]) for r in (7, 8, 9)] == [(False, False), (True, False), (False, True)]


def test_ploc_to_the_root():
    """Round 2 over A = [0,3], B = [4,6.5], C = [7,8], D = [9.5,10.5]: A -> B, B -> C (4 against 6.5), C -> D (3.5 against 4), D -> C: (C,D).
    Round 3 over A, B, CD = [7,10.5]: A -> B; B: [0,6.5] and [4,10.5] tie, position 0: (A,B).  Round 4: the root.  Numbers from n - 2 = 4
    down in merge order: (0,1) = 4, (2,3) = 3, (4,5) = 2, (A,B) = 1, root = 0."""
    left, right, nbox = br.ploc(slabs(SIX))
    assert left.tolist() == [1, 4, ~4, ~2, ~0] and right.tolist() == [2, 3, ~5, ~3, ~1]
    assert nbox[:, [0, 3]].tolist() == [[0, 10.5], [0, 6.5], [7, 10.5], [4, 6.5], [0, 3]]
    newpos, first, last = br.ploc_leaf_order(left, right)
    assert newpos.tolist() == [0, 1, 2, 3, 4, 5] and first.tolist() == [0, 0, 4, 2, 0] and last.tolist() == [5, 3, 5, 3, 1]


def test_ploc_leaf_order_renumbers_depth_first():
    """root = (leaf 2, node 1), node 1 = (leaf 0, leaf 1): depth-first, left first, leaf 2 comes first."""
    newpos, first, last = br.ploc_leaf_order(np.array([~2, ~0]), np.array([1, ~1]))
    assert newpos.tolist() == [1, 2, 0] and first.tolist() == [0, 1] and last.tolist() == [2, 2]


def test_ploc_gives_up():
    assert br.ploc(np.tile(slabs([(0, 1)]), (300, 1))) is None                       # one merge per round: more than 192 rounds
    chain = slabs([(0, 1.5 ** k) for k in range(70)])                                  # nested: one merge per round, a chain deeper than 64
    assert br.ploc(chain) is None
    H = br.prepare(*br.soup_arrays(np.tile(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], F32), (300, 1))), 1)
    assert not H.ploc and H.max_depth == 9                                           # the Karras tree over 300 equal keys: balanced by position


# --------------------------------------------------------------------------------------------------------- cut, collapse
def hand_tree():
    """Seven leaves with a unit cross-section over the x intervals below;
         0 = (1, 2)   1 = (3, leaf 2)   2 = (leaf 3, 4)   3 = (leaf 0, leaf 1)   4 = (5, leaf 6)   5 = (leaf 4, leaf 5)
       x extents: node 1 [0,6], node 2 [10,14], node 3 [0,4], node 4 [12,14], node 5 [12,13.5]: nodes 2 and 3 have the SAME area."""
    H = br.Hierarchy()
    H.tbox = slabs([(0, 1), (3, 4), (5, 6), (10, 11), (12, 12.5), (13, 13.5), (13.5, 14)])
    H.n, H.val, H.ref_tri = 7, np.arange(7), None
    H.left, H.right = np.array([1, 3, ~3, ~0, 5, ~4]), np.array([2, ~2, 4, ~1, ~6, ~5])
    H.parent_i, H.parent_l, H.depth, H.leaf_depth = br.parents_and_depths(H.left, H.right)
    H.nbox = br.fit(H.left, H.right, H.depth, H.tbox)
    newpos, H.first, H.last = br.ploc_leaf_order(H.left, H.right)
    assert newpos.tolist() == list(range(7))
    H.max_depth = int(H.leaf_depth.max())
    return H


def test_collapse_of_a_hand_drawn_tree():
    """leaf_max 1.  Root: [1, 2]; node 1 is larger: the last entry takes its place, its children are appended: [2, 3, leaf 2].
    Nodes 2 and 3 tie: strict >, the first wins, node 2 is opened: [leaf 2, 3, leaf 3, 4].  Node 4: [5, leaf 6] -> [leaf 6, leaf 4, leaf 5].
    Slots in level order: node 3 = 1, node 4 = 2; two wide levels."""
    H = hand_tree()
    assert H.nbox[:, [0, 3]].tolist() == [[0, 14], [0, 6], [10, 14], [0, 4], [12, 14], [12, 13.5]]
    assert br.collapse_children(H, 0, 1) == [~2, 3, ~3, 4]
    assert br.collapse_children(H, 3, 1) == [~0, ~1] and br.collapse_children(H, 4, 1) == [~6, ~4, ~5]
    W, depth = br.wide_nodes(H, 1)
    rec, wide = 4 * 6, 4 * 6 + 4 * 7
    assert depth == 2 and W.view(np.int32)[:, 10:14].tolist() == [
        [~(rec + 8), wide + 4, ~(rec + 12), wide + 8], [~rec, ~(rec + 4), ~rec, ~rec], [~(rec + 24), ~(rec + 16), ~(rec + 20), ~(rec + 24)]]
    assert br.last_flags(H, 1).tolist() == [1] * 7


def test_cut_rule_and_count_bits():
    """leaf_max 2: nodes 3 and 5 (two records each) are leaves; node 4 (three) is not; the root never is, whatever leaf_max says.
    Root: [1, 2] -> [2, 3, leaf 2] -> only node 2 is no leaf: [leaf 2, 3, leaf 3, 4]; node 4: [5, leaf 6] and nothing to open.  A leaf
    link carries min(records, 4) - 1 in its low bits.  leaf_max 3: node 4 is a leaf too, and node 1 (three records)."""
    H = hand_tree()
    assert [br.is_cut(H, c, 2) for c in range(6)] == [False, False, False, True, False, True]
    assert [br.is_cut(H, c, 3) for c in range(6)] == [False, True, False, True, True, True]
    assert not br.is_cut(H, 0, 7)
    assert br.last_flags(H, 2).tolist() == [0, 1, 1, 1, 0, 1, 1] and br.last_flags(H, 3).tolist() == [0, 0, 1, 1, 0, 0, 1]
    W, depth = br.wide_nodes(H, 2)
    rec, wide = 24, 52
    assert depth == 2 and W.view(np.int32)[:, 10:14].tolist() == [
        [~(rec + 8), ~(rec | 1), ~(rec + 12), wide + 4], [~((rec + 16) | 1), ~(rec + 24), ~((rec + 16) | 1), ~((rec + 16) | 1)]]
    B = br.binary_nodes(H, 2).view(np.int32)
    assert B[:, 12:14].tolist() == [[4, 8], [~(rec + 0), ~(rec + 8)], [~(rec + 12), 16], [~rec, ~(rec + 4)], [~(rec + 16), ~(rec + 24)], [~(rec + 16), ~(rec + 20)]]
    W7, depth7 = br.wide_nodes(H, 7)                    # everything below the root's children is one leaf each
    assert depth7 == 1 and W7.view(np.int32)[0, 10:14].tolist() == [~(rec | 2), ~((rec + 12) | 3), ~(rec | 2), ~(rec | 2)]


def test_records_lone_triangle_and_minus_zero():
    """A lone triangle is doubled and both records report id 0; -0.0f becomes +0.0f in v0.x and nowhere else."""
    tri = np.array([[-0.0, -0.0, -0.0], [1.0, -0.0, 0.0], [-0.0, 1.0, -0.0]], F32)
    B, R, W, info, wd = br.build(tri, np.array([[0, 1, 2]]), 1, 2)
    assert info == dict(n_inner=1, n_tri_refs=2, n_leaves=2, max_depth=1) and wd == 1 and len(W) == 1
    Ri = R.view(np.int32)
    assert Ri[:, 3].tolist() == [0, 0] and Ri[:, 7].tolist() == [1, 1]
    neg = np.int32(-2 ** 31)
    assert Ri[0, 0:3].tolist() == [0, neg, neg]          # v0: x cleared, y and z keep their sign
    assert W.view(np.int32)[0, 10:14].tolist() == [~4, ~8, ~4, ~4]


# -------------------------------------------------------------------------------------------------------------- pre-split
def test_split_count_at_its_branch_points():
    """target 1: an extent of exactly 1 is not above it (1); 1.5 -> ceil = 2; 6.5 -> 7; 8.5 -> 9, capped at 8; exactly 32 = 4 * 8 targets is
    not above the wall limit (8); 33 is (1: the wall stays whole); a target of 0 cuts nothing.  The axis is the longest, x before y
    before z on ties."""
    def tri(ex, ey=0.25, ez=0.125):
        return [0, 0, 0, ex, ey, 0, 0, 0, ez]
    k, axis = br.split_count(np.array([tri(1.0), tri(1.5), tri(6.5), tri(8.5), tri(32.0), tri(33.0), tri(0.25, 3.5, 0.5), tri(2, 2, 2), tri(1, 2, 2)], F32), 1.0)
    assert k.tolist() == [1, 2, 7, 8, 8, 1, 4, 2, 2] and axis.tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 1]
    assert br.split_count(np.array([tri(5.0)], F32), 0.0)[0].tolist() == [1]
    assert br.split_count(np.array([tri(1.0 + 2.0 ** -23)], F32), 1.0)[0].tolist() == [2]


def test_split_slabs_of_one_triangle():
    """(0,0,0) (4,0,0) (0,2,0) cut in two along x.  Slab [0,2]: the two vertices at x = 0 and the crossings (2,0,0), (2,1,0) of the plane
    x = 2 (a plane through a vertex is no crossing): x 0 .. 2 + pad, y 0 .. 2, z 0.  Slab [2,4]: vertex (4,0,0) and the same crossings:
    x 2 - pad .. 4, y 0 .. 1 + pad_y.  pad = 1e-5f * 4 (+ 1e-30f, absorbed), pad_y = 1e-5f * 2; never beyond the triangle's own box."""
    s = br.split_slabs(np.array([0, 0, 0, 4, 0, 0, 0, 2, 0], F32), 2, 0)
    pad, pad_y = F32(1e-5) * F32(4), F32(1e-5) * F32(2)
    want = np.array([[0, 0, 0, F32(2) + pad, 2, 0], [F32(2) - pad, 0, 0, 4, F32(1) + pad_y, 0]], F32)
    assert np.array_equal(s.view(np.int32), want.view(np.int32)), s.tolist()


def test_split_target_in_binary32():
    v = np.array([[0, 0, 0], [3, 4, 12], [1, 1, 1]], F32)           # diagonal 13
    assert br.split_target(v, 64, 50) == F32(F32(0.01) * F32(50) * F32(13)) / F32(8)


@pytest.mark.parametrize("name,presplit", PRESPLIT)
def test_presplit_reference_counts(name, presplit):
    """More references than triangles where test_gpu_tree_audit expects it of the device (needles, gto_sixteen); nothing at all is
    cut below 64 triangles."""
    n = len(builder_mesh(name)[3])
    info = br.cached_build(name, arrays(name), 0, 2, presplit)[3]
    if name == "needles-63":
        assert info["n_tri_refs"] == 63
    elif name != "two-scales":
        assert info["n_tri_refs"] > n
    assert br._prepared[(name, 0, presplit)].ref_tri is not None or info["n_tri_refs"] == n


# ------------------------------------------------------------------------------------------------------------ the cases
def test_what_the_synthetic_cases_are_for():
    tb = {name: ta.tri_boxes(br.case_soup(name)) for name in ("co-centred", "co-centred-far", "flat", "at-the-max", "two-scales", "pairs", "soup-257")}
    assert len(br.case_soup("co-centred")) == 40 and np.all(br.centres(tb["co-centred"]) == F32(0.5))
    keys = br.morton_keys(tb["co-centred"])
    assert np.all(keys == 0)                                         # no centre extent: rel is 0 by the rule, every key equal
    assert br.prepare(*br.soup_arrays(br.case_soup("co-centred")), 1).ploc, "PLOC finishes on co-centred (else the expected tree is the Karras one)"
    q, qs = br.quantise(tb["co-centred-far"])
    assert np.all(q[:40] == 0) and len(set(qs[:40].tolist())) > 8     # only the size bits differ among the forty
    assert np.all(br.quantise(tb["flat"])[0][:, 1] == 0)
    q, _ = br.quantise(tb["at-the-max"])
    assert [(q[:, a] == 262143).sum() for a in range(3)] == [1, 1, 1]
    _, qs = br.quantise(tb["two-scales"])
    assert (qs == 511).sum() >= 2 and qs.min() == 0 and all(np.any((qs >> np.uint64(b)) & np.uint64(1)) for b in range(9))
    k = br.morton_keys(tb["pairs"])
    assert np.array_equal(k[400:], k[:400:5])
    c = br.centres(tb["soup-257"])
    assert c[:, 0].argmax() == 256 and c[:, 1].argmax() == 256 and c[:, 2].argmin() == 256 and c[:, 0].argmin() == 255


def test_inputs_outside_the_normal_range_are_refused():
    s = br.case_soup("soup-16")
    for scale in (1.0e-20, 1.0e25):            # products of extents near 1e-42 (subnormal) and 1e48 (infinite)
        with pytest.raises(br.OutOfRange):
            br.prepare(*br.soup_arrays(s * F32(scale)), 1)


# ---------------------------------------------------------------------------------------------------------------- audit
@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name", MESHES)
def test_reference_trees_pass_the_strict_audit(name, algo):
    """Every mesh of the device comparison stays inside the normal-range condition (the build would raise), and every tree is what
    tree_audit demands of a device-built one."""
    soup = builder_mesh(name)[3]
    for leaf_max in (1, 2, 4, 8):
        B, R, W, info, wd = br.cached_build(name, arrays(name), algo, leaf_max)
        v = ta.audit(B, R, W, info, soup, wide_depth=wd, strict=True, **device_kw(leaf_max))
        assert v == [], f"{name} algo {algo} leaf_max {leaf_max}\n" + "\n".join(f"{x.kind} | {x.item} | {x.what}" for x in v[:12])


@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name,presplit", PRESPLIT)
def test_presplit_reference_trees_pass_the_audit(name, presplit, algo):
    soup = builder_mesh(name)[3]
    B, R, W, info, wd = br.cached_build(name, arrays(name), algo, 2, presplit)
    v = ta.audit(B, R, W, info, soup, wide_depth=wd, split_refs=True, coverage=True, **device_kw(2))
    assert v == [], f"{name} algo {algo} presplit {presplit}\n" + "\n".join(f"{x.kind} | {x.item} | {x.what}" for x in v[:12])


# ------------------------------------------------------------------------------------------------------------ tree cost
def test_tree_cost_by_hand():
    """Two wide nodes, steps (.5, .25, 1).  Root: slot 0 bytes 0..(4,8,2) -> extents (2,2,2), area 24, a leaf of two records; slot 1
    bytes (4,0,0)..(8,8,2) -> area 24, an inner link.  Child: one leaf, bytes 0..(2,4,1) -> (1,1,1), area 6, one record.  The root's box:
    (8 * .5, 8 * .25, 2 * 1) = (4,2,2), area 40.  node_visits = (40 + 24) / 40, tri_tests = (2 * 24 + 6) / 40."""
    def node(lo, hi, links):
        d = np.zeros(16, F32)
        di = d.view(np.uint32)
        d[3], d[14], d[15] = 0.5, 0.25, 1.0
        for a in range(3):
            di[4 + a] = sum((lo[k][a] if k < len(lo) else 255) << (8 * k) for k in range(4))
            di[7 + a] = sum((hi[k][a] if k < len(hi) else 0) << (8 * k) for k in range(4))
        d.view(np.int32)[10:14] = [links[k] if k < len(links) else links[0] for k in range(4)]
        return d
    n_bin, n_rec = 2, 3
    rec, wide = 4 * n_bin, 4 * (n_bin + n_rec)
    W = np.array([node([(0, 0, 0), (4, 0, 0)], [(4, 8, 2), (8, 8, 2)], [~(rec | 1), wide + 4]), node([(0, 0, 0)], [(2, 4, 1)], [~(rec + 8)])])
    R = np.zeros((3, 16), F32)
    R.view(np.int32)[:, 7] = [0, 1, 1]
    assert br.tree_cost(W, n_bin, n_rec) == (1.6, 1.35) == br.tree_cost(W, n_bin, n_rec, records=R)
    assert br.cost_terms(W) == (2, 2)
