"""The auditor of tests/tree_audit.py can fail: a valid tree built entirely in numpy passes it in strict mode, and every single
mutation of that tree — the defects a grazing-ray cap would hide — is reported, as the right kind.  No GPU, no project library."""
from fractions import Fraction

import numpy as np
import pytest

import tree_audit as ta


# ------------------------------------------------------------------------------------------------------ a tree in numpy
def make_soup(n, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-4.0, 4.0, (n, 1, 3))
    return (c + rng.uniform(-0.6, 0.6, (n, 3, 3))).astype(np.float32).reshape(n, 9)


def numpy_tree(soup, seed=2):
    """Median-split binary tree (leaves of 1..3 triangles), collapsed 4-wide the way emit / k_collapse do it (the inner child
    with the largest box is opened first), in the [binary][records][wide] layout with the restated encoders."""
    rng = np.random.default_rng(seed)
    tb = ta.tri_boxes(soup)
    nodes, leaf_runs, rec_ids = [], [], []          # nodes[i] = [(is_leaf, ref, box), (is_leaf, ref, box)]

    def box_of(ids):
        b = tb[ids[0]].copy()
        for t in ids[1:]:
            b = ta._union(b, tb[t])
        return b

    def split(ids):
        """-> (is_leaf, ref, box)"""
        if len(ids) <= int(rng.integers(1, 4)):
            leaf_runs.append((len(rec_ids), len(ids)))
            rec_ids.extend(ids)
            return True, len(leaf_runs) - 1, box_of(ids)
        b = box_of(ids)
        ax = int(np.argmax(b[3:] - b[:3]))
        ids = sorted(ids, key=lambda t: (float(tb[t][ax]) + float(tb[t][3 + ax]), t))
        me = len(nodes)
        nodes.append(None)
        m = len(ids) // 2 if len(ids) != 3 else 1
        left = split(ids[:m])
        right = split(ids[m:])
        nodes[me] = [left, right]
        return False, me, b

    split(list(range(len(soup))))
    nb, nr = len(nodes), len(rec_ids)
    rec_base, wide_base = 4 * nb, 4 * (nb + nr)
    last = np.zeros(nr, np.int32)
    for first, cnt in leaf_runs:
        last[first + cnt - 1] = 1
    R = ta.encode_records(soup[rec_ids], np.array(rec_ids, np.int32), last)
    B = np.zeros((nb, 16), np.float32)
    depth_bin = 0
    depth = {0: 0}
    for i, kids in enumerate(nodes):
        for k, (is_leaf, ref, box) in enumerate(kids):
            B[i, 4 * k], B[i, 4 * k + 1], B[i, 4 * k + 2], B[i, 4 * k + 3] = box[0], box[3], box[1], box[4]
            B[i, 8 + 2 * k], B[i, 9 + 2 * k] = box[2], box[5]
            B.view(np.int32)[i, 12 + k] = ~(rec_base + 4 * leaf_runs[ref][0]) if is_leaf else 4 * ref
            if is_leaf:
                depth_bin = max(depth_bin, depth[i] + 1)
            else:
                depth[ref] = depth[i] + 1

    def area(b):
        d = b[3:] - b[:3]
        return 2.0 * float(d[0] * d[1] + d[1] * d[2] + d[2] * d[0])

    wide, todo, depth_wide = [None], [(0, 0, 0)], 0           # (binary node, wide slot, depth)
    while todo:
        u, slot, d = todo.pop(0)
        kids = list(nodes[u])
        while len(kids) < 4:
            inner = [k for k in range(len(kids)) if not kids[k][0]]
            if not inner:
                break
            best = max(inner, key=lambda k: (area(kids[k][2]), -k))
            v = kids[best][1]
            kids[best] = kids[-1]
            kids.pop()
            kids += list(nodes[v])
        links = []
        for is_leaf, ref, _ in kids:
            if is_leaf:
                first, cnt = leaf_runs[ref]
                links.append(~((rec_base + 4 * first) | (min(cnt, 4) - 1)))
                depth_wide = max(depth_wide, d + 1)
            else:
                wide.append(None)
                links.append(wide_base + 4 * (len(wide) - 1))
                todo.append((ref, len(wide) - 1, d + 1))
        wide[slot] = ta.encode_wide_node([b for _, _, b in kids], links)
    W = np.array(wide, np.float32)
    info = dict(n_inner=nb, n_tri_refs=nr, n_leaves=len(leaf_runs), max_depth=depth_bin)
    return B, R, W, info, depth_wide


@pytest.fixture(scope="module")
def tree():
    soup = make_soup(40)
    B, R, W, info, wd = numpy_tree(soup)
    for a in (B, R, W):
        a.setflags(write=False)
    return soup, B, R, W, info, wd


def run(tree, B=None, R=None, W=None, info=None, **kw):
    soup, B0, R0, W0, info0, wd = tree
    kw.setdefault("strict", True)
    kw.setdefault("coverage", True)
    return ta.audit(B0 if B is None else B, R0 if R is None else R, W0 if W is None else W, info0 if info is None else info, soup,
                    wide_depth=wd, leaf_max=3, **kw)


def kinds(v):
    return {x.kind for x in v}


def child_counts(W):
    out = []
    for w in W.view(np.int32):
        n = 1
        while n < 4 and w[10 + n] != w[10]:
            n += 1
        out.append(n)
    return np.array(out)


def leaf_slot(tree, want_records=None):
    """(wide node, slot, first record) of a leaf slot (holding `want_records` records when given)."""
    _, _, R, W, _, _ = tree
    nb = len(tree[1])
    Wi, n = W.view(np.int32), child_counts(W)
    for w in range(len(W)):
        for k in range(n[w]):
            if Wi[w, 10 + k] < 0:
                j = ((~Wi[w, 10 + k] & ~3) - 4 * nb) // 4
                if (want_records is None or (~Wi[w, 10 + k] & 3) + 1 == want_records) and j + 4 < len(R):
                    return w, k, j
    raise AssertionError("no such leaf")


# -------------------------------------------------------------------------------------------------------- the valid tree
def test_the_numpy_tree_has_the_shapes_the_mutations_need(tree):
    soup, B, R, W, info, wd = tree
    n = child_counts(W)
    assert 2 in n and 3 in n and 4 in n, np.bincount(n)
    runs = np.diff(np.concatenate([[-1], np.nonzero(R.view(np.int32)[:, 7])[0]]))
    assert set(runs.tolist()) == {1, 2, 3}
    assert info["max_depth"] > 3 and wd >= 2


def test_the_valid_tree_passes_strict(tree):
    assert run(tree) == []


def test_a_larger_valid_tree_passes_strict():
    soup = make_soup(300, seed=7)
    B, R, W, info, wd = numpy_tree(soup, seed=8)
    assert ta.audit(B, R, W, info, soup, wide_depth=wd, leaf_max=3, strict=True, coverage=True) == []


# ------------------------------------------------------------------------------------------------------------- mutations
def touching_plane(tree, hi):
    """A used slot and axis whose decoded plane cannot move inward by one grid step without cutting the exact box."""
    soup, B, R, W, info, wd = tree
    Wi, n = W.view(np.int32), child_counts(W)
    for w in range(len(W)):
        for k in range(n[w]):
            for a in range(3):
                word = 7 + a if hi else 4 + a
                q = (int(Wi[w, word]) >> (8 * k)) & 255
                if (q > 0) if hi else (q < 255):
                    return w, k, a, word, q
    raise AssertionError


def test_lo_byte_plus_one_is_a_containment_violation(tree):
    w, k, a, word, q = touching_plane(tree, hi=False)
    W = tree[3].copy()
    W.view(np.uint32)[w, word] += np.uint32(1 << (8 * k))
    v = run(tree, W=W)
    assert "containment" in kinds(v) and any(x.item == f"wide node {w} slot {k}" for x in v), v
    assert "containment" in kinds(run(tree, W=W, strict=False))


def test_hi_byte_minus_one_is_a_containment_violation(tree):
    w, k, a, word, q = touching_plane(tree, hi=True)
    W = tree[3].copy()
    W.view(np.uint32)[w, word] -= np.uint32(1 << (8 * k))
    v = run(tree, W=W, strict=False)
    assert {"containment"} <= kinds(v) <= {"containment", "coverage"} and v[0].item == f"wide node {w} slot {k}", v


def test_a_grid_step_one_ulp_smaller_lets_plane_255_fall_short(tree):
    """The encoder keeps a margin of 2^-18 on its step, so the step is taken down ulp by ulp to the smallest one whose plane 255
    still reaches the upper bound (no `step` violation); ONE ulp below that is reported, and strict sees every one of them."""
    W0 = tree[3]
    assert "strict-wide" in kinds(run(tree, W=_step_down(W0, 1), coverage=False))
    for k in range(1, 200):
        v = run(tree, W=_step_down(W0, k), strict=False, coverage=False)
        if "step" in kinds(v):
            assert any(x.item == "wide node 0" and "plane 255" in x.what for x in v), v
            break
        assert kinds(v) <= {"containment"}, v          # (the stale hi bytes may fall short before plane 255 does)
    else:
        raise AssertionError("plane 255 never fell short")
    assert k > 1 and "step" not in kinds(run(tree, W=_step_down(W0, k - 1), strict=False, coverage=False))


def _step_down(W0, ulps):
    W = W0.copy()
    W.view(np.int32)[0, 3] -= ulps
    return W


def test_an_unused_slot_that_is_not_inverted(tree):
    n = child_counts(tree[3])
    w = int(np.nonzero(n == 3)[0][0])
    W = tree[3].copy()
    Wu = W.view(np.uint32)
    for a in range(3):
        Wu[w, 4 + a] &= np.uint32(0x00ffffff)
        Wu[w, 7 + a] |= np.uint32(0xff000000)
    v = run(tree, W=W, strict=False)
    assert kinds(v) == {"unused-slot"} and v[0].item == f"wide node {w} slot 3", v


def test_a_last_flag_cleared(tree):
    R = tree[2].copy()
    j = int(np.nonzero(R.view(np.int32)[:, 7])[0][2])
    R.view(np.int32)[j, 7] = 0
    v = run(tree, R=R, strict=False)
    assert "partition" in kinds(v), v


def test_a_last_flag_one_record_early(tree):
    w, k, j = leaf_slot(tree, 3)
    R = tree[2].copy()
    Ri = R.view(np.int32)
    assert Ri[j + 2, 7] == 1 and Ri[j + 1, 7] == 0
    Ri[j + 2, 7], Ri[j + 1, 7] = 0, 1
    v = run(tree, R=R, strict=False)
    assert "partition" in kinds(v) and "hint" in kinds(v), v
    assert any("orphan" in x.what for x in v), v


def test_a_duplicated_link_reaches_a_node_twice(tree):
    soup, B, R, W0, info, wd = tree
    Wi0, n = W0.view(np.int32), child_counts(W0)
    for w in range(len(W0)):
        inner = [k for k in range(1, n[w]) if Wi0[w, 10 + k] >= 0]
        if len(inner) >= 2:
            W = W0.copy()
            W.view(np.int32)[w, 10 + inner[1]] = Wi0[w, 10 + inner[0]]
            v = run(tree, W=W, strict=False)
            assert any(x.kind == "shape" and "reached twice" in x.what for x in v), v
            break
    else:
        raise AssertionError("no wide node with two inner children behind slot 0")
    Bm = B.copy()
    i = next(i for i in range(len(B)) if B.view(np.int32)[i, 12] >= 0 and B.view(np.int32)[i, 13] >= 0)
    Bm.view(np.int32)[i, 13] = Bm.view(np.int32)[i, 12]
    v = run(tree, B=Bm, strict=False)
    assert any(x.kind == "shape" and "reached twice" in x.what for x in v), v


def test_an_orphaned_record(tree):
    """A leaf of two loses its first record: both trees now link the second one."""
    w, k, j = leaf_slot(tree, 2)
    soup, B0, R, W0, info, wd = tree
    B, W = B0.copy(), W0.copy()
    Bi, Wi = B.view(np.int32), W.view(np.int32)
    old = ~(4 * len(B) + 4 * j)
    assert (Bi[:, 12:14] == old).sum() == 1
    Bi[:, 12:14][Bi[:, 12:14] == old] = ~(4 * len(B) + 4 * (j + 1))
    Wi[w, 10 + k] = ~((4 * len(B) + 4 * (j + 1)) | 0)
    v = run(tree, B=B, W=W, strict=False)
    assert "partition" in kinds(v), v


def test_an_id_swapped(tree):
    R = tree[2].copy()
    Ri = R.view(np.int32)
    Ri[3, 3], Ri[11, 3] = Ri[11, 3], Ri[3, 3]
    v = run(tree, R=R, strict=False, coverage=False)
    assert {"record"} <= kinds(v) <= {"record", "containment"}, v      # (the leaves' boxes no longer hold the swapped triangles either)
    assert {x.item for x in v if x.kind == "record"} == {"record 3", "record 11"}, v


def test_a_binary_child_box_one_ulp_short(tree):
    B = tree[1].copy()
    i = len(B) // 2
    assert B[i, 1] != 0
    B.view(np.int32)[i, 1] += -1 if B[i, 1] > 0 else 1          # child 0's hi.x one ulp down
    v = run(tree, B=B, strict=False)
    assert {"containment"} <= kinds(v) <= {"containment", "coverage"} and v[0].item == f"binary node {i}", v
    assert "strict-box" in kinds(run(tree, B=B))


def test_one_ulp_on_an_edge_component(tree):
    R = tree[2].copy()
    R.view(np.int32)[5, 5] += 1
    v = run(tree, R=R, strict=False, coverage=False)
    assert kinds(v) == {"record"} and v[0].item == "record 5" and "[5]" in v[0].what, v


def test_a_wrong_count_hint(tree):
    w, k, j = leaf_slot(tree, 2)
    W = tree[3].copy()
    W.view(np.int32)[w, 10 + k] = ~((~W.view(np.int32)[w, 10 + k]) ^ 3)     # 2 records -> the link says 3
    v = run(tree, W=W, strict=False)
    assert kinds(v) == {"hint"} and v[0].item == f"wide node {w} slot {k}", v


def test_max_depth_one_too_small(tree):
    info = dict(tree[4])
    info["max_depth"] -= 1
    v = run(tree, info=info, strict=False)
    assert kinds(v) == {"depth"}, v
    assert "depth" in kinds(run(tree, info=info, strict=False, depth_exact=False))
    for key in ("n_inner", "n_tri_refs", "n_leaves"):
        info = dict(tree[4])
        info[key] += 1
        assert kinds(run(tree, info=info, strict=False)) == {"counts"}


def test_a_wrong_wide_depth_and_a_big_leaf(tree):
    soup, B, R, W, info, wd = tree
    assert "depth" in kinds(ta.audit(B, R, W, info, soup, wide_depth=wd + 1))
    assert "leaf-size" in kinds(ta.audit(B, R, W, info, soup, wide_depth=wd, leaf_max=2))


def test_coverage_sees_a_leaf_box_that_misses_a_part_of_its_triangle(tree):
    """What only coverage can see: with split references a leaf box may be smaller than its triangle, so containment is silent."""
    soup, B0, R, W, info, wd = tree
    B = B0.copy()
    Bi = B.view(np.int32)
    i, k = next((i, k) for i in range(len(B)) for k in range(2) if Bi[i, 12 + k] < 0 and B[i, 4 * k + 1] - B[i, 4 * k] > 0.1)
    B[i, 4 * k + 1] = B[i, 4 * k] + np.float32(0.5) * (B[i, 4 * k + 1] - B[i, 4 * k])
    v = ta.audit(B, R, W, info, soup, wide_depth=wd, split_refs=True, coverage=True)
    assert kinds(v) == {"coverage"}, v
    assert ta.audit(B, R, W, info, soup, wide_depth=wd, split_refs=True, coverage=False) == []


# -------------------------------------------------------------------------------------------------------- canonical form
def permuted(A, link_words, base, seed):
    """A's rows under a random renumbering that keeps row 0, every inner link following its target."""
    perm = np.concatenate([[0], 1 + np.random.default_rng(seed).permutation(len(A) - 1)])     # old row -> new row
    out = np.empty_like(A)
    out[perm] = A
    Oi = out.view(np.int32)
    for w in link_words:
        inner = Oi[:, w] >= 0
        Oi[inner, w] = base + 4 * perm[(Oi[inner, w] - base) // 4]
    return out


def test_the_canonical_form_does_not_depend_on_the_numbering(tree):
    soup, B, R, W, info, wd = tree
    form = ta.canonical_form(B, R, W)
    wide_base = 4 * (len(B) + len(R))
    assert form[:R.nbytes + B.nbytes] == R.tobytes() + B.tobytes()       # numpy_tree numbers its binary nodes depth-first already
    for seed in (1, 2, 3):
        Bp, Wp = permuted(B, (12, 13), 0, seed), permuted(W, (10, 11, 12, 13), wide_base, 10 + seed)
        assert not np.array_equal(Bp, B) and not np.array_equal(Wp, W)
        assert ta.audit(Bp, R, Wp, info, soup, wide_depth=wd, leaf_max=3, strict=True, coverage=True) == []     # still the same valid tree
        assert ta.canonical_form(Bp, R, Wp) == form
        assert ta.canonical_form(Bp, R, W) == form and ta.canonical_form(B, R, Wp) == form


def test_the_canonical_form_sees_what_is_not_numbering(tree):
    soup, B, R, W, info, wd = tree
    form = ta.canonical_form(B, R, W)
    Bs = B.copy()                                  # the root's children change places: another child order
    Bs[0, 0:4], Bs[0, 4:8] = B[0, 4:8], B[0, 0:4]
    Bs[0, 8:10], Bs[0, 10:12] = B[0, 10:12], B[0, 8:10]
    Bs[0, 12], Bs[0, 13] = B[0, 13], B[0, 12]
    assert ta.canonical_form(Bs, R, W) != form
    Ws = W.copy()                                  # a wide node's first two links change places
    Ws.view(np.int32)[0, 10], Ws.view(np.int32)[0, 11] = W.view(np.int32)[0, 11], W.view(np.int32)[0, 10]
    assert ta.canonical_form(B, R, Ws) != form
    Rs = R.copy()
    Rs.view(np.int32)[5, 5] += 1                   # one ulp in a record
    assert ta.canonical_form(B, Rs, W) != form


# ----------------------------------------------------------------------------------------------------------------- fma32
def f32(x):
    return np.float32(x)


def test_fma32_rounds_once_where_binary64_rounds_twice():
    """A q * step + origin that lands on a binary32 tie only AFTER the binary64 rounding.  130 * 16519105 = 2^31 + 2 exactly, so with
    origin 2^55 (binary32 spacing 2^32, binary64 spacing 8) the exact sum 2^55 + 2^31 + 2 lies above the tie 2^55 + 2^31 and rounds
    UP; binary64 drops the 2, stands on the tie and the second rounding goes to the even neighbour, DOWN."""
    q, step, origin = f32(130.0), f32(16519105.0), f32(2.0 ** 55)
    assert Fraction(float(q)) * Fraction(float(step)) == 2 ** 31 + 2
    via64 = np.float64(q) * np.float64(step) + np.float64(origin)
    assert via64 == 2.0 ** 55 + 2.0 ** 31 and np.float32(via64) == f32(2.0 ** 55)          # two roundings: down
    up = f32(2.0 ** 55 + 2.0 ** 32)
    assert ta.fma32(q, step, origin) == up                                                 # one rounding: up
    assert ta.fma32_fast(q, step, origin) == up
    for scale in (2.0 ** -24, 2.0 ** -60, 2.0 ** 40):                                      # the same bits at other exponents
        assert ta.fma32(q, f32(step * f32(scale)), f32(origin * f32(scale))) == f32(up * f32(scale))
        assert ta.fma32_fast(q, f32(step * f32(scale)), f32(origin * f32(scale))) == f32(up * f32(scale))
    assert ta.fma32(q, step, -origin) == f32(-(2.0 ** 55) + 2.0 ** 31)                     # below 2^55 the spacing is 2^31: exact + 2 rounds to it


def test_fma32_basic_cases():
    assert ta.fma32(2.0, 3.0, 4.0) == 10.0
    assert ta.fma32(f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23), -1.0) == f32(2.0 ** -22 + 2.0 ** -46)      # the product is not rounded
    assert ta.fma32(2.0 ** -100, 2.0 ** -49, 0.0) == f32(2.0 ** -149)                                    # the smallest subnormal
    assert ta.fma32(2.0 ** -100, 2.0 ** -50, 0.0) == 0.0                                                 # a tie to even: zero
    assert ta.fma32(3.0 * 2.0 ** -100, 2.0 ** -50, 0.0) == f32(2.0 ** -148)                              # 1.5 ulp: tie to even, up
    assert np.isinf(ta.fma32(3.0e38, 2.0, 0.0))
    assert ta.fma32(1.0, f32(2.0 ** 24), 1.0) == f32(2.0 ** 24)                                          # tie, even
    assert ta.fma32(1.0, f32(2.0 ** 24 + 2), 1.0) == f32(2.0 ** 24 + 4)                                  # tie, the even one is up
    assert np.signbit(ta.fma32(0.0, 1.0, -0.0)) == False and np.signbit(ta.fma32(-0.0, 1.0, -0.0))      # noqa: E712
    assert ta.round_f32(Fraction(1, 3)) == f32(1.0 / 3.0)


def test_fma32_fast_equals_fma32_on_random_and_tie_inputs():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, 4000).astype(np.float32)
    b = (rng.uniform(0.5, 2.0, 4000) * 2.0 ** rng.integers(-130, 20, 4000)).astype(np.float32)
    c = (rng.normal(size=4000) * 2.0 ** rng.integers(-130, 30, 4000)).astype(np.float32)
    c[::7] = (b[::7] * np.float32(128)).astype(np.float32)
    got = ta.fma32_fast(a, b, c)
    want = np.array([ta.fma32(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_the_restated_encoder_contains_and_is_tight():
    rng = np.random.default_rng(9)
    for trial in range(40):
        n = int(rng.integers(1, 5))
        scale = 10.0 ** rng.integers(-20, 20)
        lo = (rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
        hi = (lo + rng.uniform(0, 1, (n, 3)).astype(np.float32) * np.float32(scale) * (trial % 3 != 0)).astype(np.float32)
        d = ta.encode_wide_node(np.concatenate([lo, hi], 1), list(range(-8, -8 - 4 * n, -4)))
        di = d.view(np.uint32)
        step, origin = np.array([d[3], d[14], d[15]]), d[0:3]
        assert np.all(step >= ta.F32_MIN_NORMAL)
        for k in range(4):
            qlo = np.array([(int(di[4 + a]) >> (8 * k)) & 255 for a in range(3)])
            qhi = np.array([(int(di[7 + a]) >> (8 * k)) & 255 for a in range(3)])
            if k >= n:
                assert np.all(qlo == 255) and np.all(qhi == 0) and d.view(np.int32)[10 + k] == -8
                continue
            assert np.all(ta.fma32_fast(qlo, step, origin) <= lo[k]) and np.all(ta.fma32_fast(qhi, step, origin) >= hi[k])


# ----------------------------------------------------------------------------------------------------------- Woop records
def woop_tree(tree):
    """the tree with its records restated as Woop records (PT_OPT_TRI_TEST 1): same ids, same runs"""
    soup, B, R, W, info, wd = tree
    Ri = R.view(np.int32)
    return ta.encode_woop_records(soup[Ri[:, 3]], Ri[:, 3], Ri[:, 7])


def test_the_valid_tree_passes_with_woop_records(tree):
    stats = {}
    assert run(tree, R=woop_tree(tree), woop=True, stats=stats) == []
    assert stats == dict(woop_floats=12 * len(tree[2]), woop_floats_differ=0)


def test_woop_rows_send_the_vertices_to_the_unit_points(tree):
    """what the audit's identity check rests on, seen from outside it: in binary64 the rows are M^-1 to a few ulp of binary32"""
    soup, R = tree[0], woop_tree(tree)
    ids = R.view(np.int32)[:, 15] >> 1
    v = soup[ids].astype(np.float64).reshape(-1, 3, 3)
    r = R.astype(np.float64)
    u = np.einsum("ni,nki->nk", r[:, 4:7], v) + r[:, 7:8]
    w = np.einsum("ni,nki->nk", r[:, 8:11], v) + r[:, 11:12]
    z = np.einsum("ni,nki->nk", r[:, 0:3], v) - r[:, 3:4]
    assert np.allclose(u, [[1, 0, 0]], atol=1e-4) and np.allclose(w, [[0, 1, 0]], atol=1e-4) and np.allclose(z, 0, atol=1e-4)


@pytest.mark.parametrize("what", ["rows-swapped", "translation-sign", "two-ulp", "normal-one-ulp", "id-word", "last-bit-into-id"])
def test_a_wrong_woop_record_is_reported(tree, what):
    R = woop_tree(tree).copy()
    Ri = R.view(np.int32)
    j = 5
    if what == "rows-swapped":
        R[j, 4:12] = R[j, [8, 9, 10, 11, 4, 5, 6, 7]]
    elif what == "translation-sign":
        R[j, 7] = -R[j, 7]
    elif what == "two-ulp":
        Ri[j, 9] += 2
    elif what == "normal-one-ulp":
        Ri[j, 13] += 1
    elif what == "id-word":
        other = next(k for k in range(len(R)) if (Ri[k, 15] & 1) == (Ri[j, 15] & 1) and k != j)
        Ri[j, 15], Ri[other, 15] = Ri[other, 15], Ri[j, 15]
    else:
        Ri[j, 15] = Ri[j, 15] >> 1     # the bare id where id << 1 | last belongs
    v = run(tree, R=R, woop=True)
    assert kinds(v) & {"woop-rows", "woop-record", "ids", "partition", "containment", "leaf-size"}, v
    if what in ("rows-swapped", "translation-sign"):
        assert "woop-rows" in kinds(v)
    if what in ("two-ulp", "normal-one-ulp"):
        assert kinds(v) == {"woop-record"}
