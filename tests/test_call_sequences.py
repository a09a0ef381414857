"""tests/call_sequences.py without a GPU: the sequences are deterministic, never hold an invalid operation, the shadow state's
canonical form tells apart what the alphabet can tell apart and nothing else, and the committed seeds and DIRECTED together meet
the coverage condition that tests/test_gpu_call_sequences.py relies on."""
import itertools

import numpy as np
import pytest

import call_sequences as cs
import gpu_pathtracer_amd as g
from call_sequences import DIRECTED, LENGTH, SEEDS, Op, Runner, State, StubTracer, random_sequence

SEQUENCES = cs.all_sequences()


def test_a_seed_gives_one_sequence():
    for seed in SEEDS:
        a, b = random_sequence(seed, LENGTH), random_sequence(seed, LENGTH)
        assert a == b and [repr(o) for o in a] == [repr(o) for o in b] and len(a) == LENGTH
        assert eval(repr(a), {"Op": Op, "inf": np.inf}) == a, "a sequence's repr must paste back"
    assert len({tuple(random_sequence(s, LENGTH)) for s in SEEDS}) == len(SEEDS)
    n_obs = sum(o.observes for s in SEEDS for o in random_sequence(s, LENGTH))
    assert 0.2 < n_obs / (LENGTH * len(SEEDS)) < 0.45, "about one operation in three is an observation"


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_no_invalid_operation_reaches_the_context(name):
    """Every sequence replayed on the stub, fresh contexts included: the stub's own model of the host's checks accepts every
    state change (a refusal there raises PtError out of apply), answers every refused call with its documented code (apply asserts
    it), never sees a call that would reach a kernel with bad data (StubViolation), and ends up holding what the shadow state says."""
    ops = SEQUENCES[name]
    seen = []
    t = StubTracer(0)
    runner = Runner(t, lambda step, ops_, state, args, got, want: seen.append((step, cs.first_difference(got, want))), make=StubTracer)
    runner.run(ops)
    assert len(seen) == sum(o.observes for o in ops) and all(d is None for _, d in seen), seen
    s = runner.state
    assert t.n_tree == (cs.n_tris(s.tree.mesh) if s.tree else 0) and t.n_table == (s.table[1] if s.table else 0)
    assert t.n_spheres == (len(cs.sphere_set(s.spheres)) if s.spheres else 0)
    assert (t.env is not None) == (s.env is not None) and (t.env is None or t.env[1] == s.env[1])
    assert (t.stream is None) == (s.stream == "own")
    for k, v in s.options:
        assert t.opts[cs.OPTIONS[k][0]] == v
    refused = [c for c in t.calls if c[0] == "refused"]
    assert len(refused) >= sum(o.kind == "refused" for o in ops)


def test_the_shadow_state_blocks_what_the_library_would_refuse():
    """valid() is False wherever the stub's model of the library refuses a state change (a tree the table does not cover, a refit
    without a tree), and where the alphabet's own rules say so (cornell_box's table stands beside that mesh only)."""
    t = StubTracer(0)
    big = Op("upload_bvh", "bunny_low").apply(t, State())
    small = Op("table", "dark").apply(StubTracer(0), Op("upload_bvh", "cube").apply(StubTracer(0), State()))
    box = Op("table", "cornell_box").apply(StubTracer(0), Op("upload_bvh", "cornell_box").apply(StubTracer(0), State()))
    every = list(itertools.chain.from_iterable(cs.change_ops(State(tree=cs.Tree("upload", "cornell_box", 1, 2))).values()))
    n_blocked = n_refused = 0
    for state in (State(), big, small, box):
        for op in every:
            stub = StubTracer(0)
            cs.install(stub, state)
            if op.valid(state):
                assert op.apply(stub, state) is not None
                continue
            n_blocked += 1
            with pytest.raises(AssertionError):
                op.apply(stub, state)
            if op.kind in ("upload_bvh", "build_bvh") and cs.n_tris(op.args[0]) > state.table[1]:
                n_refused += 1
                with pytest.raises(g.PtError) as e:
                    _unchecked(op, stub, state)
                assert e.value.code == cs.PT_ERR_INVALID
    assert n_blocked > 20 and n_refused > 5
    with pytest.raises(g.PtError) as e:
        StubTracer(0).refit_bvh(StubTracer(0).malloc(36))
    assert e.value.code == cs.PT_ERR_NO_SCENE and not Op("refit", "twist").valid(State())


def _unchecked(op, stub, state):
    """apply without the shadow state's own check."""
    valid, Op.valid = Op.valid, lambda self, s: True
    try:
        op.apply(stub, state)
    finally:
        Op.valid = valid


def test_the_canonical_form():
    def after(*ops):
        s, t = State(), StubTracer(0)
        for op in ops:
            s = op.apply(t, s)
        return s.canon()

    a, b = Op("upload_bvh", "cornell"), Op("upload_bvh", "cube")
    assert after(a, b, a) == after(a)
    assert after(Op("spheres", "forty"), Op("spheres", None)) == after() == State().canon()
    assert after(Op("opt", "WALK", 0), Op("opt", "WALK", 2)) == after()
    assert after(Op("env", "5x3", True), Op("env", None)) == after()
    assert after(Op("stream", "torch"), Op("stream", "own")) == after()
    assert after(a, Op("refit", "twist"), Op("refit", "drop"), Op("refit", "twist")) == after(a, Op("refit", "twist"))
    assert after(a, Op("refused", "refit_count"), Op("refused", "tri_id")) == after(a)
    assert after(a, Op("table", "dark"), Op("table", None)) == after(a)
    hash(after(a, Op("table", "dark"), Op("env", "16x8", False)))
    # every single change is told apart from every other and from no change, on a state where all of them are valid
    base = [Op("upload_bvh", "cornell_box")]
    start = base[0].apply(StubTracer(0), State())
    reached = {}
    for op in itertools.chain.from_iterable(cs.change_ops(start).values()):
        t = StubTracer(0)
        cs.install(t, start)
        c = op.apply(t, start).canon()
        same_as_start = (op == base[0] or op == Op("stream", "own") or op == Op("spheres", None) or op == Op("table", None) or op == Op("env", None)
                         or (op.kind == "opt" and op.args[1] == cs.OPTIONS[op.args[0]][1]))
        assert (c == start.canon()) == same_as_start, op
        if not same_as_start:
            assert c not in reached, f"{op!r} and {reached[c]!r} reach the same canonical state"
            reached[c] = op
    assert len(reached) > 50


def test_the_coverage_condition():
    """Over the committed seeds and DIRECTED together: every (state-changing kind, observation kind) pair occurs with no other
    change of that kind in between, and every observation kind follows a refused call.  A condition on the committed sequences:
    a change to the alphabet or to a sequence that loses a pair fails here."""
    pairs, after_refused = cs.coverage(SEQUENCES.values())
    missing = sorted({(c, o) for c in cs.CHANGE_KINDS for o in cs.OBS_KINDS} - pairs)
    assert not missing, f"no sequence makes {missing}"
    assert after_refused == set(cs.OBS_KINDS), f"never behind a refused call: {set(cs.OBS_KINDS) - after_refused}"
    assert any(cs.relights(random_sequence(s, LENGTH)) for s in SEEDS) and cs.relights(DIRECTED["lights"])
    refused = {o.args[0] for ops in SEQUENCES.values() for o in ops if o.kind == "refused"}
    assert refused == set(cs.REFUSED)
    used = {o for ops in SEQUENCES.values() for o in ops}
    for name, (_, _, values) in cs.OPTIONS.items():
        assert {Op("opt", name, v) for v in values} <= used, f"a value of {name} is never set"
    for m in cs.MESHES:
        assert Op("upload_bvh", m) in used and any(o.kind == "build_bvh" and o.args[0] == m for o in used), m
    assert {o.args[1:3] for o in used if o.kind == "build_bvh"} == {(0, 1), (0, 2), (1, 1), (1, 2)}
    assert {o.args for o in used if o.kind == "env"} == {("16x8", False), ("16x8", True), ("5x3", False), ("5x3", True), (None,)}
    assert {o.args[0] for o in used if o.kind == "refit"} == set(cs.REFITS)
    renders = [o.args for o in used if o.observes and o.args[0] == "render"]
    assert {a[1:3] for a in renders} == set(cs.FRAMES) and {a[3] for a in renders} == set(cs.SPPS)
    assert {a[4] for a in renders} == set(cs.DEPTHS) and {a[5] for a in renders} == set(cs.FLAGS)
    assert {a[6] for a in renders} == {1, 2} and {a[7] for a in renders} == {1, 2, 3}


def test_the_directed_sequences_hold_what_they_are_for():
    d = DIRECTED
    big, small = cs.obs_render(257, 131, 16, 4, cs.NEE), cs.obs_render(8, 8, 1, 1, 0)
    assert d["grow-only"].index(big) < d["grow-only"].index(small) < d["grow-only"].index(cs.obs_render(96, 64, 3, 4, cs.NEE))
    assert len({o for o in d["auto-table"] if o.observes}) == 10 and len(cs.AUTO_RESTARTS) == 4 and len(cs.AUTO_UNCHANGED) == 1
    assert all(d["auto-table"][i].observes and not d["auto-table"][i - 1].observes or i == cs.AUTO_RESTARTS[0] for i in cs.AUTO_RESTARTS)
    ss = d["side-slots"]
    assert [o.kind for o in ss].count("later") == 34 and ss[-1] == Op("collect") and ss[4] == Op("refit", "orig")
    changes = [i for i, o in enumerate(ss) if i > 4 and o.kind in cs.CHANGE_KINDS]
    assert {ss[i].kind for i in changes} == {"refit", "spheres", "table", "env", "opt"}
    assert all([o.kind for o in ss[i - 4:i]] == ["later"] * 4 for i in changes), "four calls back to back in front of every change"
    assert [o.args[0] for o in d["streams"] if o.kind == "stream"] == ["own", "torch", "own"] * 2
    assert sum(o.kind == "refit" for o in d["refit-owner"]) == 4 and cs.n_tris("cornell_perm") == cs.n_tris("cornell")
    rb = d["refused-between"]
    between = {o.args[0] for i, o in enumerate(rb) if o.kind == "refused" and rb[i - 1].observes and rb[i - 1] == rb[i + 1]}
    assert between == set(cs.REFUSED), "every refused call sits between two identical observations"
    assert all(o.observes or o.kind == "opt" for o in d["every-option"][2:])
