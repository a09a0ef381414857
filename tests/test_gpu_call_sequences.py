"""A context's call history never changes what it renders: every sequence of tests/call_sequences.py — the committed seeds and the
directed ones, one per piece of state that outlives a call — applied to ONE long-lived context, and at every
observation the outputs compared with those of a fresh context that was given only the current shadow state.

THE REFERENCE CHAIN
  1. The long-lived context equals the fresh one bit for bit (call_sequences.first_difference over the words of every output:
     accumulator, display words, moments and the frame error, guides, denoised and temporal outputs, t / id / normal, any-hit bytes,
     environment outputs, every return code, pt_scene_info, the sign of pt_last_build_ms and the last refit's count of dropped triangles
     (which on the fresh side must be the number the vertex set was given); the work counters where PT_OPT_KERNEL is
     not AUTO, so that both sides ran the same kernel).  Under PT_KERNEL_AUTO the two sides may run different kernels: include/ptmi.h
     promises the same images, so a difference there is a finding as well.
  2. For every distinct (state, pt_render observation) without an environment map, the fresh context's frame goes once through
     gpu_support.judge against orc.render: bit for bit where the context walks the very tree the oracle walks with a binary walk
     (an uploaded host tree, never refit, PT_OPT_LEAF_MAX 2, PT_OPT_WALK 0 or 1) or has no tree; per-pixel L2 < 1e-3 with at most
     gpu_support.MAX_DIFF differing pixels, each holding the brute-force renderer's colour, everywhere else (the wide walks; a
     device-built or refit tree, whose boxes are not the oracle's: the grazing cases of PT_OPT_REBUILD).  One oracle render per
     configuration, shared through gpu_support.oracle.
  3. pt_trace_rays' hits of the fresh context equal orc.trace_brute over the state's (moved) mesh, t and id, bit for bit;
     pt_closest_hits' may differ from brute force under the bound at MAX_DIFF rays (a grazing ray between the wide tree's boxes),
     and pt_any_hits says what pt_closest_hits found.
  So the fresh side is never the only witness.

NOT COMPARED: timings — pt_auto_choice's milliseconds, pt_get_stage_ms, pt_last_kernel_ms, the value of pt_last_build_ms.

A failure names the sequence, the step, the operations up to it as text that pastes back into call_sequences.DIRECTED, and the
first differing word.  Nothing is retried."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import call_sequences as cs
import gpu_pathtracer_amd as g
import orc
from call_sequences import DIRECTED, LENGTH, SEEDS, Runner, random_sequence
from gpu_support import MAX_DIFF, judge, oracle

pytestmark = pytest.mark.gpu
_judged = set()


def judge_fresh(state, args, want):
    """Links 2 and 3 of the chain, once per (canonical state, observation)."""
    key = (state.canon(), args)
    if key in _judged or want["rc"].any() or (args[0] == "render" and "rgba" not in want):   # (a "later" render continues a running mean)
        return
    _judged.add(key)
    tree = state.tree
    if args[0] == "render" and state.env is None:
        W, H, spp, depth, flags, calls, _ = args[1:]
        mesh = cs.oracle_mesh(tree.mesh, tree.refit) if tree else None
        same_tree = tree is not None and tree.how == "upload" and tree.refit is None and tree.leaf_max == 2
        bvh = None if tree is None else cs.host_tree(tree.mesh) if same_tree else cs._once(("obvh", tree.mesh, tree.refit), lambda: g.Bvh(mesh))
        rows = ids = None
        if state.table is not None:
            rows, ids = cs.table_of(state.table, tree.mesh)
            ids = np.ascontiguousarray(ids[:mesh.n_tris])
        sph, cam, p = cs.sphere_set(state.spheres), cs.camera_of(state, W, H), cs.params_of(W, H, depth, flags, 7, 1)
        lights = None if rows is None or not any(any(m.emi) for m in rows) else orc.tri_lights(mesh, rows, ids)
        ref = oracle(("call-sequences", tree and (tree.mesh, tree.refit, same_tree), state.spheres, state.table, args),
                     lambda: orc.render(bvh, sph, cam, p, spp * calls, materials=rows, tri_material=ids, lights=lights)[:2])
        variant = SimpleNamespace(name="call-sequences-fresh", exact=tree is None or (same_tree and state.opt("WALK") in (0, 1)))
        judge(variant, f"{state.canon()} {args}", (want["acc"], want["rgba"]), ref, mesh, sph, cam, p, spp * calls, materials=rows, tri_material=ids)
    if args[0] == "hits":
        mesh = cs.oracle_mesh(tree.mesh, tree.refit)
        lo, hi = cs.bounds_of(state)
        rays = orc.random_rays(cs.N_HITS, lo, hi, seed=78)   # (observe's rays; its bounds only shape word 7)
        tb, ib, _ = orc.trace_brute(mesh, rays, args[1])
        bad = np.flatnonzero((want["trace_id"] != ib) | (want["trace_t"].view(np.int32) != tb.view(np.int32)))
        assert len(bad) == 0, f"pt_trace_rays on the fresh context: {len(bad)} rays differ from brute force, first {bad[:5]}"
        t_max = np.full(cs.N_HITS, np.inf, np.float32)
        t_max[cs.N_HITS // 2:] = np.random.default_rng(79).uniform(0.05, 1.5, cs.N_HITS - cs.N_HITS // 2).astype(np.float32) * float(np.max(hi - lo))
        inside = (ib >= 0) & (tb < t_max)
        ib, tb = np.where(inside, ib, -1), np.where(inside, tb, np.float32(3.4028234663852886e38))
        bad = np.flatnonzero((want["closest_id"] != ib) | (want["closest_t"].view(np.int32) != tb.view(np.int32)))
        print(f"pt_closest_hits on the fresh context: {len(bad)} of {cs.N_HITS} rays differ from brute force; {int(inside.sum())} hit")
        assert len(bad) <= MAX_DIFF, f"pt_closest_hits on the fresh context: {len(bad)} rays differ from brute force, first {bad[:5]}"
        assert np.array_equal(want["any"] != 0, want["closest_id"] >= 0), "pt_any_hits and pt_closest_hits disagree on the fresh context"


def run_sequence(name, ops):
    t = g.PathTracer(0)
    n_fresh, t0, asked = cs.fresh_contexts[0], time.perf_counter(), {}

    def compare(step, ops_, state, args, got, want):
        if name == "auto-table" and step in cs.AUTO_RESTARTS:
            assert t.auto_choice()[0] == g.KERNEL_AUTO, f"{name} step {step}: the trials of a configuration the table cannot hold did not start over"
        if name == "auto-table" and step in [s_ for pair in cs.AUTO_UNCHANGED for s_ in pair]:
            asked[step] = t.auto_choice()[0]
            before = [b for b, a in cs.AUTO_UNCHANGED if a == step]
            assert not before or asked[before[0]] == asked[step], f"{name} step {step}: with a map up no entry is consulted, yet pt_auto_choice answers {asked[step]} after {asked[before[0]]}"
        if "dropped" in want:
            n = cs.n_dropped(state.tree.mesh, state.tree.refit)
            assert int(want["dropped"][0]) == n, f"{name} step {step}: the fresh context's refit dropped {int(want['dropped'][0])} triangles, not {n}"
        d = cs.first_difference(got, want)
        if d is not None:
            pytest.fail(f"{name} step {step}: {args} differs from a fresh context in output {d[0]!r} at word {d[1]}: {d[2]!r} on the "
                        f"long-lived context, {d[3]!r} on the fresh one.  State {state}.  The sequence up to here:\n[" +
                        ",\n ".join(repr(o) for o in ops_[:step + 1]) + "]", pytrace=False)
        judge_fresh(state, args, want)

    try:
        Runner(t, compare).run(ops)
        t.sync()
    finally:
        t.close()
    print(f"{name}: {len(ops)} operations, {sum(o.observes for o in ops)} observations, {cs.fresh_contexts[0] - n_fresh} fresh contexts, "
          f"{time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequence(seed):
    run_sequence(f"seed-{seed}", random_sequence(seed, LENGTH))


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_sequence(name):
    run_sequence(name, DIRECTED[name])
