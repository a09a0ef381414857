"""The schedule knobs of pt_render at the ends of their ranges.  include/ptmi.h says of PT_OPT_BATCH, PT_OPT_REFILL, PT_OPT_VOTE_NODE /
PT_OPT_VOTE_REC, PT_OPT_SPHERE_LDS, PT_OPT_TOP_NODES, PT_OPT_OCCUPANCY, PT_OPT_LDS_STACK, PT_OPT_WAVE_BATCH, PT_OPT_WAVE_BLOCKS and
PT_OPT_OVERLAP "speed, never results"; here every one of them is rendered at both ends of what pt_set_option accepts and the frame
is compared.  (tests/test_gpu_render_rays.py does the same for k_render_rays' copy of the refill loop, tests/test_gpu_query.py for
k_query_rays'.)

THE REFERENCE CHAIN
  1. The exact binary walks (PT_OPT_WALK 0 and 1, persistent kernel and megakernel) equal orc.render bit for bit, accumulator and
     display words, at every setting.
  2. The wide walks (2, 4, and the stage-split pipeline) equal THEIR OWN frame at the default knobs bit for bit.
  3. That default frame goes through gpu_support.judge against the oracle: per-pixel L2 < 1e-3, at most gpu_support.MAX_DIFF
     differing pixels, each of which must hold the brute-force renderer's colour.
  One oracle render per (scene, size, samples), shared through gpu_support.oracle.  For every case below the oracle's own walk was
  compared with the brute-force loop (orc.sample_pixels(..., mesh=...)) on the CPU before the inputs were fixed, over all pixels
  (every fourth one of the big case); the counts stand beside the cases.

WHAT MAKES A LOST OR DOUBLED SLOT VISIBLE.  A slot traced twice writes the same value twice; a slot never traced leaves whatever
the sample buffer held.  So every setting (`run`):
  (a) first renders the same context and buffers with another `frame` (the poison), then the call under test with
      sample_index = 1;
  (b) renders it once more with PT_OPT_COUNTERS 1: paths == W * H * samples exactly; rays and hits equal the oracle's (exact
      walks) or the default-knob run's (wide walks); inner, tris and leaves equal the default-knob run's as well where a lane's
      own walk does not depend on the schedule (see counter_keys: walks 1 and 2, not 0 and 4);
  (c) the frame is not empty and differs from the poison frame.

WHY NO SETTING CAN SPIN (read off the loops before the first run; b = batch, r = refill as the kernel gets them)
  - k_trace_persist_bvh2 / k_render_rays.  queue_knobs (pt_plan.h) clamps r <= b.  A walk (every trav_run_*) only returns early when
    64 - live - dead >= b lanes wait: they are finished walkers, lanes to shade, or idle lanes of a queue that is not empty (idle
    lanes of an empty queue are `dead` and never count).  Finished walkers and lanes to shade are shaded in the same round:
    progress.  If none of the b waiting lanes is one of those, all b are idle with work left, and b >= r triggers the refill at the
    top of the next round, which draws min(idle, avail) > 0 slots or finds the queue empty (then they are dead): progress.  At
    b = 64 a walk returns only with live == 0; at b = r = 1 a wave leaves the walk for every single lane.  Without the clamp
    (b = 1, r = 64) one idle lane would end every walk at once and never be refilled: that is the spin the clamp's comment names.
    The chunk fetch tries each of the PT_SHARDS shards once and then declares the queue empty; a slot pt_slot_pixel refuses (a
    ragged image) is consumed and its lane stays idle.  The loop ends when the queue is empty and every lane idle.
  - trav_run / trav_run_unified / trav_run_wide.  Entered by walking lanes only; the early exit is tested after (while-while) or
    before a step, and on entry live + dead + waiting = 64 with waiting < b or the round has something to shade, so a step runs.
    In trav_run_wide the phase with more lanes runs; the lanes of the other phase `continue`, which is safe because the chosen
    phase has at least one lane (n_live > 0 and the vote picks the larger side) and that lane advances.
  - trav_run_wide_pend.  node_phase = n_node * vote_node >= n_rec * vote_rec with both weights >= 1.  Not node_phase implies
    n_rec * vote_rec > 0, so a lane tests a record; node_phase with n_node == 0 implies n_rec == 0, hence n_live == 0, and that
    case has left the loop one line earlier.  So every iteration advances at least one lane whatever the weights are; a weight of
    64 against 1 only makes one phase wait until the other has no lane left.
  - k_wf_extend / k_query_rays.  The refill runs when n_idle >= b or n_idle == 64.  The walk returns when b lanes have finished
    (then n_idle >= b: refill) or all have (n_idle == 64: refill).  The refill's `round < 8` loop hands out min(idle - served,
    end - next) records per round; a region with walk_in[r] == 0 gives next == end and take == 0, costs one of the eight rounds
    and one queue ticket, and the next round draws the next region: every region is drawn once, so after at most n_regions
    tickets the queue is empty.  A wave that leaves the refill without a live lane and with the queue not empty `continue`s into
    the next refill (n_idle == 64); with the queue empty it breaks.  Lanes that can get no work are `dead` and do not count
    towards b, so the walk's first test cannot be true on entry (busy - live == 0 < 1 <= b).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import COUNTERS, MAX_DIFF, bvh_of, golden_camera, judge, oracle
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 1000   # the poison calls render frames `frame + POISON ..`


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """One scene, camera, size and sample count.  samples = spp x calls; `frame` is the first frame number."""

    def __init__(self, name, scene, spheres, W, H, spp, tri_mat=g.MAT_DIFF, cam=None, frame=0):
        self.name, self.scene, self.spheres, self.W, self.H, self.spp, self.tri_mat, self.frame = name, scene, spheres, W, H, spp, tri_mat, frame
        self.cam = golden_camera(W, H) if cam is None else cam

    def with_spp(self, spp):
        return Case(self.name, self.scene, self.spheres, self.W, self.H, spp, self.tri_mat, self.cam, self.frame)

    def sph(self):
        return g.reference_spheres() if self.spheres else None

    def params(self, frame=None, sample_index=1):
        p = g.default_params(self.W, self.H, depth=4, tri_mat=self.tri_mat)
        p.flags = g.FLAG_WRITE_RGBA
        p.frame, p.sample_index = self.frame if frame is None else frame, sample_index
        return p


# open: the dragon alone, seen from close by (40 % of the first segments hit it); ragged in both directions, so pt_slot_pixel refuses
# slots; paths end on a miss at different bounces, so lanes go idle at different times; 153 tiles x 3 samples = 29 376 slots, so
# queue_chunk gives 16 and a wave with 64 idle lanes crosses several chunk ends in a row.
# CPU: oracle walk against brute force over all 9 159 pixels, 3 samples (frame 7, and the poison's frame 1007) and 8 samples: 0 differ.
OPEN = Case("open", "dragon", False, 129, 71, 3, cam=make_camera(129, 71, pos=(1.0, -9.0, -27.0), front=(-3.2, -2.2, -9.0)), frame=7)
# room: every path is long (REFR triangles in a closed room), the sphere table is used; the committed oracle image refr_4.
# CPU: oracle walk against brute force over all 4 096 pixels, 4 and 8 samples: 0 differ.
ROOM = Case("room", "cornell", True, 64, 64, 4, tri_mat=g.MAT_REFR, frame=0)
# big: 42 x 32 tiles; the samples per call come from big_spp so that queue_chunk gives 32 and 64.
# CPU: oracle walk against brute force over every fourth pixel, (x + y) % 4 == 0: 20 896 of 83 583 (all of them take 25 minutes on
# eight cores), at 8 and at 16 samples (frames 7 ..): 0 differ.  On the MI355X the wide walk's default frame, which walks other
# boxes than the oracle, differs from the oracle at 0 pixels for both sample counts.
BIG = Case("big", "cornell_dragon", True, 333, 251, 8, frame=7)

PERSIST, MEGA, PIPE = g.KERNEL_PERSISTENT, g.KERNEL_MEGA_BVH2, g.KERNEL_WAVEFRONT
KNAME = {PERSIST: "persistent", MEGA: "mega", PIPE: "pipeline"}
CORNERS = ((1, 1), (1, 64), (64, 1), (64, 64), (36, 8), (2, 64))   # (PT_OPT_BATCH, PT_OPT_REFILL); (1, 64) and (2, 64): the clamp works


def corner(batch, refill):
    return ((g.OPT_BATCH, batch), (g.OPT_REFILL, refill))


def counter_keys(kernel, walk):
    """The counters that must not depend on the schedule.  rays, hits, paths: always.  inner, tris, leaves: where a lane's own
    walk is a function of its ray alone — the unified walk 1 and the wide walk 2 (the pipeline's per-lane and packet walks are
    walk 2 over slots whose wave is fixed by the slot order, not by the knobs).  Not walk 0: its lanes keep descending while
    they wait for their wave to reach a leaf (trav_run's ballot), so which nodes a lane fetches depends on its wave mates.  Not
    walk 4: the vote decides WHEN a parked leaf tightens h.t, hence how many boxes the lane still opens before it does."""
    return COUNTERS if walk in (1, 2) else ("rays", "hits", "paths")


# ------------------------------------------------------------------------------------------------ one setting
def run(case, kernel, walk, options=(), calls=1):
    """(accumulator, display words, counters) of `calls` consecutive pt_render calls of case.spp samples each, without a sync
    between them, on a fresh context with `options` set before the scene goes up — after (a) the poison, with (b) the counter
    run and (c) the emptiness checks of the module docstring."""
    W, H, spp = case.W, case.H, case.spp
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, kernel)
        t.set_option(g.OPT_WALK, walk)
        for o, v in options:
            t.set_option(o, v)
        t.upload_bvh(bvh_of(case.scene)[1])
        t.upload_spheres(case.sph())
        acc, rgba = t.alloc_frame(W, H)

        def render(first_frame, n_calls, counters=False):
            total = {}
            for k in range(n_calls):
                t.launch_kernel(acc.ptr, rgba.ptr, case.cam, case.params(first_frame + k * spp, 1 + k * spp), spp)
                if counters:   # (the counters are those of the last launch; reading them waits for it)
                    for key, v in {**t.counters(), **t.wave_stats()}.items():   # (their keys do not collide)
                        total[key] = total.get(key, 0) + v
            t.sync()
            return acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W)), total

        # (a) one call more than under test: with PT_OPT_OVERLAP the calls behind the first alternate between two side buffers
        poison = render(case.frame + POISON, calls + 1 if calls > 1 else 1)
        got = render(case.frame, calls)
        what = f"{case.name} {KNAME[kernel]} walk {walk} {dict(options)}"
        assert got[0].any(), f"{what}: the frame is empty"                                                       # (c)
        assert not np.array_equal(got[0], poison[0]), f"{what}: the frame is the poison frame"
        t.set_option(g.OPT_COUNTERS, 1)                                                                          # (b)
        again = render(case.frame, calls, counters=True)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), f"{what}: the instrumented launch renders another frame"
        assert again[2]["paths"] == W * H * spp * calls, f"{what}: {again[2]['paths']} paths, not {W * H * spp * calls}"
        acc.free()
        rgba.free()
        return got[0], got[1], again[2]
    finally:
        t.close()


def oracle_of(case, calls=1):
    """(accumulator, display words, counters) of orc.render over all samples of `calls` calls, once per run."""
    n = case.spp * calls
    return oracle(("schedule-knobs", case.name, case.W, case.H, n),
                  lambda: orc.render(bvh_of(case.scene)[1], case.sph(), case.cam, case.params(), n))


_default = {}


def default_frame(case, kernel, walk, calls=1, keep=()):
    """A walk's own run at the default knobs (`keep`: options that are part of the variant, not knobs), judged against the
    oracle once: bit for bit for an exact walk, links 2 and 3 of the chain for a wide one.  Its counters are the reference of
    counter_keys for every walk: the oracle's inner, tris and leaves belong to the oracle's own walk and tree."""
    key = (case.name, case.spp, calls, kernel, walk, tuple(keep))
    if key not in _default:
        got = run(case, kernel, walk, keep, calls)
        ref = oracle_of(case, calls)
        variant = SimpleNamespace(name=f"knobs-{KNAME[kernel]}-walk{walk}", exact=walk in (0, 1))
        judge(variant, f"{case.name} x{calls} {dict(keep)}", got[:2], ref[:2], bvh_of(case.scene)[0], case.sph(), case.cam, case.params(), case.spp * calls)
        _default[key] = got
    return _default[key]


def check(case, kernel, walk, options, calls=1, keep=()):
    """One setting through the chain.  The frame: an exact walk against the oracle, a wide one against its default frame.  The
    counters: counter_keys against the walk's own default-knob run, and for an exact walk rays, hits and paths against the
    oracle's as well."""
    exact = walk in (0, 1)
    base = default_frame(case, kernel, walk, calls, keep)
    ref = oracle_of(case, calls) if exact else base
    got = run(case, kernel, walk, tuple(keep) + tuple(options), calls)
    what = f"{case.name} x{calls} {KNAME[kernel]} walk {walk} {dict(tuple(keep) + tuple(options))}"
    print(f"{what}: " + ", ".join(f"{k} {got[2][k]}" for k in COUNTERS + ("stack_overflows",)))
    n_diff = int(np.any(got[0] != ref[0], axis=-1).sum())
    assert n_diff == 0, f"{what}: {n_diff} pixels differ from {'the oracle' if exact else 'the default-knob frame'}"
    assert np.array_equal(got[1], ref[1]), f"{what}: display words differ"
    for k in counter_keys(kernel, walk):
        assert got[2][k] == base[2][k], f"{what}: counter {k} {got[2][k]}, default knobs {base[2][k]}"
    if exact:
        for k in ("rays", "hits", "paths"):
            assert got[2][k] == ref[2][k], f"{what}: counter {k} {got[2][k]}, oracle {ref[2][k]}"


def test_the_room_is_the_committed_oracle_image():
    """The reference of the room case is tests/golden/oracle_images.npz refr_4; needs no GPU work of its own."""
    z = np.load(os.path.join(GOLD, "oracle_images.npz"))
    acc, rgba, _ = oracle_of(ROOM)
    assert np.array_equal(acc, z["refr_4"]) and np.array_equal(rgba, z["refr_4_rgba"])


# ------------------------------------------------------------------------------------------------ batch / refill
@pytest.mark.parametrize("walk", [1, 2, 4])
@pytest.mark.parametrize("case", [OPEN, ROOM], ids=lambda c: c.name)
def test_batch_and_refill_corners(case, walk):
    """Phases A and B of k_trace_persist_bvh2: the ballot / mbcnt lane -> slot map with 1 .. 64 idle lanes, the chunk tail, the
    `64 - live - dead >= batch` exit of the three resumable walks, the refill <= batch clamp."""
    for batch, refill in CORNERS:
        check(case, PERSIST, walk, corner(batch, refill))


# ------------------------------------------------------------------------------------------------ the phase vote of walk 4
@pytest.mark.parametrize("batch", [1, 36, 64])
@pytest.mark.parametrize("case", [OPEN, ROOM], ids=lambda c: c.name)
def test_vote_weights(case, batch):
    """trav_run_wide_pend with one phase starved as long as the other has a lane (1 : 64, 64 : 1), level (64 : 64) and odd (3 : 2)."""
    for node, rec in ((1, 64), (64, 1), (64, 64), (3, 2)):
        check(case, PERSIST, 4, ((g.OPT_VOTE_NODE, node), (g.OPT_VOTE_REC, rec), (g.OPT_BATCH, batch)))


# ------------------------------------------------------------------------------------------------ sphere table in LDS or not
@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("case", [ROOM, BIG], ids=lambda c: c.name)
def test_sphere_table_in_lds_or_not(case, walk):
    """path_shade reads the spheres from the block's LDS copy (1) or through scalar / global loads (0): the same words."""
    for v in (0, 1):
        check(case, PERSIST, walk, ((g.OPT_SPHERE_LDS, v),))


# ------------------------------------------------------------------------------------------------ occupancy x LDS stack
@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("kernel", [PERSIST, MEGA], ids=lambda k: KNAME[k])
@pytest.mark.parametrize("case", [OPEN, ROOM], ids=lambda c: c.name)
def test_every_occupancy_and_stack_pair(case, kernel, walk):
    """All twelve pairs pt_set_option accepts, so every "nearest instantiation" of launch_persist and launch_mega is taken: the
    LDS layout is sized for the REQUESTED window and the kernel runs the instantiated one.  (No ray of these scenes leaves the
    16-entry window: `check` prints stack_overflows, measured 0 at every pair on both scenes.  The overflow to private memory
    is pinned on both sides of the window by tests/test_gpu_deep_stack.py, on hand-built trees.)"""
    for occ in (4, 5, 6, 8):
        for lstk in (0, 16, 24):
            check(case, kernel, walk, ((g.OPT_OCCUPANCY, occ), (g.OPT_LDS_STACK, lstk)))


# ------------------------------------------------------------------------------------------------ top of the tree in LDS
@pytest.mark.parametrize("kernel", [PERSIST, MEGA], ids=lambda k: KNAME[k])
@pytest.mark.parametrize("case", [ROOM, OPEN], ids=lambda c: c.name)
def test_top_nodes_mirror(case, kernel):
    """The while-while walk (the only reader of the mirror) over the producer's own leaves, as in test_gpu_parity: no mirror, one
    node, the default, the most.  cornell's tree is smaller than the mirror; of the dragon's the mirror is a strict prefix."""
    n_inner = bvh_of(case.scene)[1].nodes.size // 16   # four vec4 per inner node; PT_OPT_LEAF_MAX 0 keeps them as they come
    assert (1 < n_inner < 64) if case is ROOM else n_inner > 1024, n_inner
    for top in (0, 1, 64, 1024):
        check(case, kernel, 0, ((g.OPT_LEAF_MAX, 0), (g.OPT_TOP_NODES, top)))


# ------------------------------------------------------------------------------------------------ the stage-split pipeline
@pytest.mark.parametrize("first_walk", [1, 0])
@pytest.mark.parametrize("case", [OPEN, ROOM], ids=lambda c: c.name)
def test_pipeline_wave_batch_and_blocks(case, first_walk):
    """k_wf_extend's refill rounds and walk exit.  first_walk 0 sends bounce 0 through the refilling kernel as well (FIRST: slots,
    not records).  At depth 4 the open scene's late bounces have regions with few or no walkers: `round < 8` meets
    walk_in[r] == 0.  Both variants hold the same frame."""
    keep = ((g.OPT_FIRST_WALK, first_walk),)
    for batch in (1, 5, 16, 64):
        for blocks in (1, 8):
            check(case, PIPE, 2, ((g.OPT_WAVE_BATCH, batch), (g.OPT_WAVE_BLOCKS, blocks)), keep=keep)
    a, b = default_frame(case, PIPE, 2, keep=keep), default_frame(case, PIPE, 2, keep=((g.OPT_FIRST_WALK, 1),))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "PT_OPT_FIRST_WALK changes the frame"


# ------------------------------------------------------------------------------------------------ two calls, overlapped or not
@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("case", [OPEN, ROOM], ids=lambda c: c.name)
def test_two_calls_overlapped_or_in_line(case, walk):
    """Two consecutive calls of 4 samples without a sync between them: with PT_OPT_OVERLAP 1 the second one's path kernel runs
    on a side stream into a sample buffer and queue counters of its own while the first drains; the fold order makes the result
    the 8-sample running mean.  NOT CONFIRMED: that the second call did take the side stream.  plan_call takes it only when
    hipStreamQuery finds the caller's stream busy at the second launch — likely with the first call just issued, not certain on
    frames this small — and the call plan can only be read back under PT_OPT_TIMING, which itself puts the call in line.  What
    the test does guarantee: whichever way each of the four settings ran, the frame is the oracle's (or the default-knob one)."""
    four = case.with_spp(4)
    for overlap in (0, 1):
        for batch in (1, 64):
            check(four, PERSIST, walk, ((g.OPT_OVERLAP, overlap),) + corner(batch, batch), calls=2)


# ------------------------------------------------------------------------------------------------ the three chunk sizes
def queue_chunk(n_cu, slots):
    """pt_plan.h::queue_chunk"""
    waves = n_cu * 20
    return 64 if slots // 64 >= 4 * waves else 32 if slots // 32 >= 4 * waves else 16


def big_spp(n_cu, chunk):
    """The fewest samples per call at which the big case's launch gets `chunk`-slot chunks on a device of n_cu CUs: 8 and 16 on
    the MI355X's 256.  On another device the samples scale with its CUs, so that all three chunk sizes still occur."""
    tiles = ((BIG.W + 7) // 8) * ((BIG.H + 7) // 8)
    return -(-(4 * 20 * n_cu * chunk) // (tiles * 64))


@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("chunk", [32, 64])
def test_three_chunk_sizes(chunk, walk):
    """The `min(first + chunk, total)` tail and the lane -> slot map at chunks of 32 and 64 slots (the open scene has 16), at the
    batch / refill corners.  The CPU check of the reference stands beside BIG."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    spp = big_spp(n_cu, chunk)
    tiles = ((BIG.W + 7) // 8) * ((BIG.H + 7) // 8)
    print(f"{n_cu} CUs: {spp} samples per call for chunks of {chunk} slots")
    assert queue_chunk(n_cu, tiles * 64 * spp) == chunk and (spp == 1 or queue_chunk(n_cu, tiles * 64 * (spp - 1)) < chunk)
    assert queue_chunk(n_cu, 153 * 64 * OPEN.spp) == 16, "the open scene does not get 16-slot chunks on this device"
    case = BIG.with_spp(spp)
    for batch, refill in CORNERS:
        check(case, PERSIST, walk, corner(batch, refill))
