"""Call histories of one long-lived context, for tests/test_call_sequences.py (CPU) and tests/test_gpu_call_sequences.py (GPU).

THE PROPERTY.  Whatever valid calls a context has seen, the next observation is bit for bit what a fresh context returns when it
is given only the current state.  The library keeps state that outlives a call (csrc/pt_ctx.h: the grow-only DevBuf members d_wave,
d_samples, side[x].samples, d_denoise, d_frame_err and d_occ, each grown by one reserve() behind the wait its call site states; the
scene's values tree / d_spheres / mat / env, each adopted behind quiesce(); the generations scene_gen / geom_gen / mat_gen / env_gen
and what is keyed by them; the emissive-triangle light list in `mat`; PT_KERNEL_AUTO's table of picks; the two side-stream slots;
the caller's stream), so a wrong key, a missed wait or a stale carve shows only after a particular history.

WHAT IS HERE
  State        the shadow state: what the context should hold now, as a hashable value (`canon()` is its canonical form).
  Op           one operation of the alphabet; `Op.apply(t, state)` calls the context `t` and returns the new shadow state;
               `repr(op)` can be pasted back into DIRECTED.  Kinds: the state changes (CHANGE_KINDS), "refused" (REFUSED: calls
               the host refuses before any launch; the shadow state stays) and "obs" / "later" / "collect" (observations).
  observe      makes one observation on a context and returns its outputs as a dict of arrays.
  expected     the same observation on a FRESH context that was given the shadow state with the fewest calls, memoised.
  Runner       applies a sequence to one long-lived context and hands every observation to a `compare` callback.
  random_sequence, SEEDS, LENGTH, DIRECTED     the sequences; coverage() is the condition test_call_sequences.py asserts on them.
  StubTracer   a context without a GPU that records calls and checks their preconditions with a model of its own.

Importing this module needs the built host library and no GPU."""
import hashlib
import itertools
from dataclasses import dataclass, replace

import numpy as np

import gpu_pathtracer_amd as g
import orc
from gpu_support import bvh_of, dark_table, golden_camera, set_options, soup_mesh, turn_rows, twist
from scene_matrix import SPHERE_SETS, make_camera

_abi = g._abi
PT_ERR_INVALID, PT_ERR_NO_SCENE, PT_ERR_UNSUPPORTED = -1, -3, -5

# ---------------------------------------------------------------------------------------------------- the alphabet's values
OPTIONS = {   # name: (option, default, the values the alphabet sets)
    "KERNEL": (g.OPT_KERNEL, g.KERNEL_AUTO, (g.KERNEL_AUTO, g.KERNEL_MEGA_BVH2, g.KERNEL_PERSISTENT, g.KERNEL_WAVEFRONT)),
    "OVERLAP": (g.OPT_OVERLAP, 1, (0, 1)),
    "COUNTERS": (g.OPT_COUNTERS, 0, (0, 1)),
    "TIMING": (g.OPT_TIMING, 0, (0, 1)),
    "WALK": (g.OPT_WALK, 2, (0, 1, 2, 4)),
    "FUSE_STAGES": (g.OPT_FUSE_STAGES, 1, (0, 1)),
    "LAST_ANYHIT": (g.OPT_LAST_ANYHIT, 1, (0, 1, 2)),
    "ROOT_CULL": (g.OPT_ROOT_CULL, 1, (0, 1, 2)),
    "ROOT_ENTRY": (_abi.OPT_ROOT_ENTRY, 1, (0, 1, 2)),
    "PATH_HISTORY": (_abi.OPT_PATH_HISTORY, 1, (0, 1, 2)),
    "FIRST_WALK": (g.OPT_FIRST_WALK, 1, (0, 1)),
    "WAVE_SAMPLES": (g.OPT_WAVE_SAMPLES, 16, (1, 4, 16, 64)),
}
MESHES = ("cube", "cornell", "bunny_low", "cornell_box", "cornell_perm")   # cornell_perm: cornell's soup, rows permuted (same count)
REFITS = ("twist", "orig", "drop", "light")                                 # light: cornell_box's emissive quad moved
SPHERES = ("reference", "one-emitter", "forty", None)
TABLES = ("cornell_box", "dark", None)
ENVS = ("16x8", "5x3")
FRAMES = ((8, 8), (37, 23), (96, 64), (257, 131))
SPPS, DEPTHS = (1, 3, 4, 16), (1, 2, 4)
FLAGS = (0, g.FLAGS_SMALLPT, g.FLAGS_SMALLPT | g.FLAG_NEE, g.FLAG_MISS_KEEPS_PATH)
NEE = g.FLAGS_SMALLPT | g.FLAG_NEE
REFUSED = ("tri_id", "nan_vertex", "option_range", "spp_2_20", "refit_count", "null_accum")
CHANGE_KINDS = ("upload_bvh", "build_bvh", "refit", "spheres", "table", "env", "opt", "stream")
OBS_KINDS = ("render", "moments", "rays", "denoise", "temporal", "hits", "envq")
N_RAYS, N_HITS, N_ENVQ = 1000, 2000, 512


# ---------------------------------------------------------------------------------------------------- inputs, made once
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def mesh_of(name):
    def make():
        if name == "cornell_perm":
            soup = g.scene_mesh("cornell").triangle_soup()
            return soup_mesh(soup[np.random.default_rng(5).permutation(len(soup))])
        return g.scene_mesh(name)
    return _once(("mesh", name), make)


def n_tris(name):
    return _once(("n", name), lambda: int(mesh_of(name).n_tris))


def host_tree(name):
    return _once(("bvh", name), lambda: g.Bvh(mesh_of(name)) if name == "cornell_perm" else bvh_of(name)[1])


def emissive_rows(name):
    m = mesh_of(name)
    emi = np.array([[*r.emi] for r in m.materials], np.float32)
    return np.nonzero(np.any(emi[m.tri_material] != 0, axis=1))[0]


def drop_rows(name):
    """A few triangles that a "drop" refit makes non-finite: never an emissive one (the light list keeps its members)."""
    n = n_tris(name)
    rows = np.unique(np.random.default_rng(11).integers(0, n, max(2, n // 16)))
    return np.setdiff1d(rows, emissive_rows(name)) if name == "cornell_box" else rows


def soup_of(name, refit):
    """The vertex set of a refit variant, float32 [n][9]; None / "orig": the mesh's own."""
    def make():
        soup = mesh_of(name).triangle_soup()
        if refit in (None, "orig"):
            return soup
        if refit == "light":
            return turn_rows(soup, emissive_rows(name), 20.0, (0.0, -0.1, 0.02))
        moved = twist(soup, 0.6, np.array([0.05, -0.02, 0.03]))
        if refit == "drop":
            bad = (np.nan, np.inf, -np.inf, np.float32(3.2e38))
            for i, r in enumerate(drop_rows(name)):
                moved[r, (3 * i) % 9] = bad[i % 4]
        return moved
    return _once(("soup", name, refit), make)


def oracle_mesh(name, refit):
    """The mesh the oracle and brute force see: a dropped triangle keeps its id as a zero-area one (never hit)."""
    def make():
        soup = soup_of(name, refit).copy()
        if refit == "drop":
            rows = drop_rows(name)
            soup[rows] = np.tile(soup_of(name, "twist")[rows, :3], 3)
        return soup_mesh(soup)
    return _once(("omesh", name, refit), make)


def sphere_set(name):
    if name is None:
        return None
    return _once(("sph", name), lambda: g.reference_spheres() if name == "reference" else SPHERE_SETS[name]())


def table_of(table, mesh_name):
    """(rows, ids) of a shadow state's material table."""
    kind, n = table
    if kind == "cornell_box":
        m = mesh_of("cornell_box")
        return m.materials, m.tri_material
    rows, ids = dark_table(mesh_of(mesh_name))
    return rows, np.zeros(n, np.int32) if len(ids) != n else ids


def env_texels(size):
    """A 16 x 8 and a 5 x 3 map: positive, uneven, one texel a hundred times brighter than the rest (a sun)."""
    w, h = (int(v) for v in size.split("x"))
    tex = np.random.default_rng(w * 100 + h).uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)
    tex[h // 3, (2 * w) // 3] = (90.0, 80.0, 60.0)
    return tex


def env_filter(size):
    return g.ENV_BILINEAR if size == "16x8" else g.ENV_NEAREST


def bounds_of(state):
    if state.tree is None:
        return np.array([-16.0, -16.0, -60.0], np.float32), np.array([16.0, 16.0, -28.0], np.float32)
    v = oracle_mesh(state.tree.mesh, state.tree.refit).verts
    return v.min(0), v.max(0)


def camera_of(state, W, H, moved=False):
    """The golden camera for the Cornell meshes (modelled in its frame) and for spheres alone; else one that sees the mesh."""
    if state.tree is None or state.tree.mesh.startswith("cornell"):
        cam = golden_camera(W, H)
        if moved:
            cam.pos[:] = (0.4, 0.2, 0.1)
        return cam
    lo, hi = bounds_of(state)
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    off = np.array([0.35, 0.25, 1.4]) + (np.array([0.04, 0.02, 0.0]) if moved else 0.0)
    return make_camera(W, H, pos=tuple(c + off * ext), front=tuple(-off))


# ---------------------------------------------------------------------------------------------------- the shadow state
@dataclass(frozen=True)
class Tree:
    how: str            # "upload" (a host tree) or "build" (pt_build_bvh)
    mesh: str
    algo: int           # PT_OPT_BUILD_ALGO at the install (build only; 1 for an upload)
    leaf_max: int       # PT_OPT_LEAF_MAX at the install
    refit: str = None   # the vertex set of the LAST refit (every refit rewrites every box and record): None = never refit


@dataclass(frozen=True)
class State:
    tree: Tree = None
    spheres: str = None
    table: tuple = None        # (kind, rows of tri_material)
    env: tuple = None          # (size, light)
    stream: str = "own"
    leaf_max: int = 2          # PT_OPT_LEAF_MAX as the last build_bvh left it: the next upload_bvh reads it
    options: tuple = ()        # ((name, value), ...) sorted, every option that was set

    def opt(self, name):
        return dict(self.options).get(name, OPTIONS[name][1])

    def with_opt(self, name, value):
        return replace(self, options=tuple(sorted({**dict(self.options), name: value}.items())))

    def canon(self):
        """Hashable and route-free: an option set to its default equals one never set."""
        return (self.tree, self.spheres, self.table, self.env, self.stream, self.leaf_max,
                tuple((k, v) for k, v in self.options if v != OPTIONS[k][1]))


def covers(table, mesh):
    """Whether a tree over `mesh` may stand beside `table`: the table's ids cover the mesh, and cornell_box's own table (whose
    emissive rows name its quad) goes with that mesh only."""
    return table is None or (n_tris(mesh) <= table[1] and (table[0] == "dark" or mesh == "cornell_box"))


# ---------------------------------------------------------------------------------------------------- operations
class Op:
    """One operation: Op(kind, *args).  apply(t, state) -> the new shadow state (the same one for "refused" and observations)."""

    def __init__(self, kind, *args):
        self.kind, self.args = kind, tuple(args)

    def __repr__(self):
        return "Op(" + ", ".join(repr(a) for a in (self.kind,) + self.args) + ")"

    def __eq__(self, o):
        return isinstance(o, Op) and (self.kind, self.args) == (o.kind, o.args)

    def __hash__(self):
        return hash((self.kind, self.args))

    @property
    def observes(self):
        return self.kind in ("obs", "later")

    def valid(self, s):
        k, a = self.kind, self.args
        if k in ("upload_bvh", "build_bvh"):
            return covers(s.table, a[0])
        if k == "refit":
            return s.tree is not None and (a[0] != "light" or s.tree.mesh == "cornell_box")
        if k == "table":
            if a[0] is None:
                return True
            return s.tree is not None and (a[0] == "dark" or s.tree.mesh == "cornell_box")
        if k == "refused":
            if a[0] == "spp_2_20":   # the pipeline must be what the call would run (plan_walk's wave_ok), or it is no refusal
                return s.tree is not None and s.env is None and s.opt("KERNEL") == g.KERNEL_WAVEFRONT and s.opt("WALK") == 2
            if a[0] == "refit_count":
                return s.tree is not None
        if k in ("obs", "later") and a[0] == "envq":
            return s.env is not None
        return True

    # ------------------------------------------------------------------ state changes
    def apply(self, t, s):
        k, a = self.kind, self.args
        assert self.valid(s), f"{self!r} is not valid in {s}"
        if k == "upload_bvh":
            t.upload_bvh(host_tree(a[0]))
            hold_soups(t, a[0])
            return replace(s, tree=Tree("upload", a[0], 1, s.leaf_max))
        if k == "build_bvh":
            mesh, algo, leaf_max = a
            t.set_option(g.OPT_BUILD_ALGO, algo)
            t.set_option(g.OPT_LEAF_MAX, leaf_max)
            t.build_bvh(mesh_of(mesh))
            hold_soups(t, mesh)
            return replace(s, leaf_max=leaf_max, tree=Tree("build", mesh, algo, leaf_max))
        if k == "refit":
            refit_to(t, s.tree.mesh, a[0])
            return replace(s, tree=replace(s.tree, refit=a[0]))
        if k == "spheres":
            t.upload_spheres(sphere_set(a[0]))
            return replace(s, spheres=a[0])
        if k == "table":
            if a[0] is None:
                t.upload_tri_materials(None, None)
                return replace(s, table=None)
            table = (a[0], n_tris(s.tree.mesh))
            t.upload_tri_materials(*table_of(table, s.tree.mesh))
            return replace(s, table=table)
        if k == "env":
            if a[0] is None:
                t.clear_environment()
                return replace(s, env=None)
            t.upload_environment(env_texels(a[0]), filter=env_filter(a[0]), light=a[1])
            return replace(s, env=(a[0], bool(a[1])))
        if k == "opt":
            t.set_option(OPTIONS[a[0]][0], a[1])
            return s.with_opt(a[0], a[1])
        if k == "stream":
            t.set_stream(stream_handle(t, a[0]))
            return replace(s, stream=a[0])
        if k == "refused":
            code = refused_call(t, s, a[0])
            want = PT_ERR_UNSUPPORTED if a[0] == "spp_2_20" else PT_ERR_INVALID
            assert code == want, f"{self!r}: returned {code}, documented {want}"
            return s
        raise ValueError(f"{self!r}: the Runner makes observations")


def stream_handle(t, which):
    """NULL for the context's own stream; one torch stream per process for "torch" (the stub takes any non-zero handle)."""
    if which == "own":
        return None
    if isinstance(t, StubTracer):
        return 0x5ca1ab1e
    def make():
        import torch
        return torch.cuda.Stream(device=torch.device("cuda", 0))
    return _once("torch-stream", make).cuda_stream


def hold_soups(t, mesh):
    """Device copies of the vertex sets a tree over `mesh` can be refit to, kept by the context and uploaded where its tree goes up
    (a call that synchronises anyway), so that a refit in the middle of a sequence does not upload.  (A tree's FIRST refit still
    synchronises once, in the library: the sequences that need an asynchronous refit make a warm-up refit to "orig" after the install.)"""
    held = t.__dict__.setdefault("_sequence_soups", {})
    for refit in REFITS:
        if (mesh, refit) not in held and (refit != "light" or mesh == "cornell_box"):
            soup = soup_of(mesh, refit)
            held[(mesh, refit)] = t.malloc(soup.nbytes)
            held[(mesh, refit)].upload(soup)
    return held


def refit_to(t, mesh, refit):
    """pt_refit_bvh to a held vertex set; every refit leaves its count of dropped triangles in a word the context keeps."""
    held = hold_soups(t, mesh)
    if "dropped" not in held:
        held["dropped"] = t.malloc(4)
    t.refit_bvh(held[(mesh, refit)], n_dropped=held["dropped"])


def n_dropped(mesh, refit):
    return len(drop_rows(mesh)) if refit == "drop" else 0


def code_of(fn):
    try:
        fn()
        return 0
    except g.PtError as e:
        return e.code


def refused_call(t, s, which):
    """One call the host refuses before any launch; returns its code."""
    if which == "tri_id":
        bvh = host_tree("cube")
        bad = type("B", (), {})()
        bad.nodes, bad.tris, bad.index = bvh.nodes, bvh.tris, bvh.index.copy()
        bad.index[int(np.flatnonzero(bad.index >= 0)[0])] = 1 << 30
        return code_of(lambda: t.upload_bvh(bad))
    if which == "nan_vertex":
        soup = mesh_of("cube").triangle_soup()
        soup[3, 4] = np.nan
        return code_of(lambda: t.build_bvh(soup_mesh(soup)))
    if which == "option_range":
        return code_of(lambda: t.set_option(g.OPT_WALK, 3))
    if which == "refit_count":
        buf = t.malloc(36)
        try:
            return code_of(lambda: t.refit_bvh(buf, n_tris=1))   # every mesh of the alphabet has more
        finally:
            buf.free()
    W = H = 2 if which == "spp_2_20" else 8
    acc, rgba = t.alloc_frame(W, H)
    try:
        p = g.default_params(W, H, depth=1)
        spp = 1 << 20 if which == "spp_2_20" else 1
        return code_of(lambda: t.launch_kernel(None if which == "null_accum" else acc.ptr, rgba.ptr, golden_camera(W, H), p, spp))
    finally:
        acc.free()
        rgba.free()


# ---------------------------------------------------------------------------------------------------- observations
def obs_render(W, H, spp, depth, flags, calls=1, parts=1):
    return Op("obs", "render", W, H, spp, depth, flags, calls, parts)


def params_of(W, H, depth, flags, frame, sample_index):
    p = g.default_params(W, H, depth=depth)
    p.flags = flags | g.FLAG_WRITE_RGBA
    p.frame, p.sample_index = frame, sample_index
    return p


def counter_keys(state):
    """gpu_support.COUNTERS where a lane's walk is a function of its ray alone (walks 1 and 2: test_gpu_schedule_knobs.counter_keys)."""
    return ("rays", "inner", "tris", "leaves", "hits", "paths") if state.opt("WALK") in (1, 2) else ("rays", "hits", "paths")


class _Bufs:
    def __init__(self, t):
        self.t, self.all = t, []

    def get(self, nbytes, zero=False):
        b = self.t.malloc(max(int(nbytes), 4))
        self.all.append(b)
        if zero:
            b.zero()
        return b

    def up(self, arr):
        b = self.get(arr.nbytes)
        b.upload(arr)
        return b

    def free(self):
        for b in self.all:
            b.free()


def render_calls(t, state, args, acc, rgba, first, moments=None):
    """The pt_render calls of a render observation, back to back; returns the first refusal's code or 0."""
    W, H, spp, depth, flags, calls, parts = args
    cam = camera_of(state, W, H)
    for call in range(calls):
        for part in range(parts):
            p = params_of(W, H, depth, flags, 7 + (first - 1) + call * spp, first + call * spp)
            if parts > 1:
                p.part_index, p.part_count, p.part_rows = part, parts, 8
            rc = code_of(lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp, None if moments is None else moments.ptr))
            if rc:
                return rc
    return 0


def scene_words(t):
    """pt_scene_info (or its refusal) and the documented sign of pt_last_build_ms."""
    try:
        info = t.scene_info()
        return np.array([info[k] for k in ("n_inner", "n_tri_refs", "n_leaves", "max_depth", "device_bytes")] + [int(t.last_build_ms() >= 0)], np.int64)
    except g.PtError as e:
        return np.array([e.code], np.int64)


def observe(t, state, args, init=None, first=1):
    """One observation on context `t`, which holds `state`: launches without a host sync in front, then the downloads.  Returns
    {name: array}.  init / first: the accumulator a render starts from and its first sample_index (a running mean under way)."""
    kind, a = args[0], args[1:]
    B = _Bufs(t)
    out = {}
    try:
        if kind in ("render", "moments", "denoise", "temporal"):
            W, H, spp, depth, flags = a[:5]
            acc, rgba = B.get(W * H * 12, True), B.get(W * H * 4, True)
            if init is not None:
                acc.upload(init)
        if kind == "render":
            out["rc"] = np.array([render_calls(t, state, a, acc, rgba, first)])
            if state.opt("COUNTERS") and state.opt("KERNEL") != g.KERNEL_AUTO and not out["rc"][0]:
                cnt = t.counters()
                out["counters"] = np.array([cnt[k] for k in counter_keys(state)], np.int64)
            out["acc"], out["rgba"] = acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W))
        elif kind == "moments":
            mom = B.get(W * H * 8, True)
            out["rc"] = np.array([render_calls(t, state, (W, H, spp, depth, flags, 2, 1), acc, rgba, 1, mom)])
            try:
                mean, above = t.frame_error(mom.ptr, W, H, 2 * spp, 0.05)
                out["error"] = np.array([mean], np.float64).view(np.int64)
                out["above"] = np.array([above], np.int64)
            except g.PtError as e:
                out["rc_error"] = np.array([e.code])
            out["acc"], out["moments"] = acc.download(np.float32, (H, W, 3)), mom.download(np.float32, (H, W, 2))
        elif kind == "rays":
            hdr, spp, depth, flags = a
            lo, hi = bounds_of(state)
            rays = B.up(orc.random_rays(N_RAYS, lo, hi, seed=77))
            res = B.get(N_RAYS * 12, True)
            rcs = []
            for call in range(2):   # folded: two calls that continue the running mean
                p = params_of(64, 64, depth, flags, 3 + call * spp, 1 + call * spp)
                rcs.append(code_of(lambda: t.render_rays(rays.ptr, N_RAYS, res.ptr, p, spp, first_index=5, hdr=hdr)))
            out["rc"], out["radiance"] = np.array(rcs), res.download(np.float32, (N_RAYS, 3))
        elif kind == "denoise":
            cam, p = camera_of(state, W, H), params_of(W, H, depth, flags, 7, 1)
            gd = [B.get(W * H * 16, True) for _ in range(3)] + [B.get(W * H * 4, True)]
            den, word = B.get(W * H * 12, True), B.get(W * H * 4, True)
            out["rc"] = np.array([render_calls(t, state, (W, H, spp, depth, flags, 1, 1), acc, rgba, 1),
                                  code_of(lambda: t.render_aux(cam, p, gd[0].ptr, gd[1].ptr, gd[2].ptr, gd[3].ptr)),
                                  code_of(lambda: t.denoise(acc.ptr, gd[0].ptr, gd[1].ptr, gd[2].ptr, W, H, den.ptr, word.ptr))])
            out["acc"] = acc.download(np.float32, (H, W, 3))
            for name, b in zip(("albedo", "normal", "position"), gd):
                out[name] = b.download(np.float32, (H, W, 4))
            out["ids"], out["denoised"], out["words"] = gd[3].download(np.int32, (H, W)), den.download(np.float32, (H, W, 3)), word.download(np.uint32, (H, W))
        elif kind == "temporal":
            th = g.TemporalHistory(t, W, H)
            try:
                rcs, last = [], None
                for k in range(2):
                    cam, p = camera_of(state, W, H, moved=k == 1), params_of(W, H, depth, flags, 7 + k * spp, 1)
                    rcs.append(code_of(lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)))
                    try:
                        last = th.push(cam, p, acc.ptr, rgba.ptr)
                        rcs.append(0)
                    except g.PtError as e:
                        rcs.append(e.code)
                out["rc"] = np.array(rcs)
                if last is not None:
                    k = 1 - th.cur
                    out["history"], out["length"] = th.color[k].download(np.float32, (H, W, 3)), th.length[k].download(np.float32, (H, W))
                    out["words"] = rgba.download(np.uint32, (H, W))
            finally:
                th.free()
        elif kind == "hits":
            cull, = a
            lo, hi = bounds_of(state)
            rays = orc.random_rays(N_HITS, lo, hi, seed=78)
            rays[: N_HITS // 2, 7] = np.inf
            rays[N_HITS // 2:, 7] = np.random.default_rng(79).uniform(0.05, 1.5, N_HITS - N_HITS // 2).astype(np.float32) * float(np.max(hi - lo))
            d_r = B.up(rays)
            tb, ib, nb = B.get(N_HITS * 4, True), B.get(N_HITS * 4, True), B.get(N_HITS * 12, True)
            tc, ic, nc, ha = B.get(N_HITS * 4, True), B.get(N_HITS * 4, True), B.get(N_HITS * 12, True), B.get(N_HITS, True)
            out["rc"] = np.array([code_of(lambda: t.trace_rays(d_r.ptr, N_HITS, cull, tb.ptr, ib.ptr, nb.ptr)),
                                  code_of(lambda: t.closest_hits(d_r.ptr, N_HITS, cull, tc.ptr, ic.ptr, nc.ptr)),
                                  code_of(lambda: t.any_hits(d_r.ptr, N_HITS, cull, ha.ptr))])
            for name, b, dt, shape in (("trace_t", tb, np.float32, (N_HITS,)), ("trace_id", ib, np.int32, (N_HITS,)), ("trace_n", nb, np.float32, (N_HITS, 3)),
                                       ("closest_t", tc, np.float32, (N_HITS,)), ("closest_id", ic, np.int32, (N_HITS,)), ("closest_n", nc, np.float32, (N_HITS, 3)),
                                       ("any", ha, np.uint8, (N_HITS,))):
                out[name] = b.download(dt, shape)
        elif kind == "envq":
            rays = B.up(orc.random_rays(N_ENVQ, (-1, -1, -1), (1, 1, 1), seed=80))
            u = B.up(np.random.default_rng(81).random((N_ENVQ, 2), dtype=np.float32))
            ev, dp, rad, pdf = B.get(N_ENVQ * 12, True), B.get(N_ENVQ * 16, True), B.get(N_ENVQ * 12, True), B.get(N_ENVQ * 4, True)
            out["rc"] = np.array([code_of(lambda: t.eval_environment(rays.ptr, N_ENVQ, ev.ptr)),
                                  code_of(lambda: t.sample_environment(u.ptr, N_ENVQ, dp.ptr, rad.ptr)),
                                  code_of(lambda: t.environment_pdf(rays.ptr, N_ENVQ, pdf.ptr))])
            out["eval"], out["dir_pdf"] = ev.download(np.float32, (N_ENVQ, 3)), dp.download(np.float32, (N_ENVQ, 4))
            out["radiance"], out["pdf"] = rad.download(np.float32, (N_ENVQ, 3)), pdf.download(np.float32, (N_ENVQ,))
            out["is_light"] = np.array([int(t.environment_is_light())])
        else:
            raise ValueError(kind)
        out["scene"] = scene_words(t)
        if state.tree is not None and state.tree.refit is not None:   # what the last refit dropped
            out["dropped"] = t.__dict__["_sequence_soups"]["dropped"].download(np.uint32, (1,))
        return out
    finally:
        B.free()


# ---------------------------------------------------------------------------------------------------- the fresh context
def install(t, s):
    """The shadow state on a fresh context with the fewest calls: every option (gpu_support.set_options: all of them before the
    uploads they govern), the stream, the tree — a refit state is the install then ONE refit — spheres, table, map."""
    opts = [(OPTIONS[k][0], v) for k, v in s.options]
    if s.tree is not None:
        opts += [(g.OPT_BUILD_ALGO, s.tree.algo), (g.OPT_LEAF_MAX, s.tree.leaf_max)]
    set_options(t, opts)
    if s.stream != "own":
        t.set_stream(stream_handle(t, s.stream))
    if s.tree is not None:
        if s.tree.how == "upload":
            t.upload_bvh(host_tree(s.tree.mesh))
        else:
            t.build_bvh(mesh_of(s.tree.mesh))
        hold_soups(t, s.tree.mesh)
        if s.tree.refit is not None:
            refit_to(t, s.tree.mesh, s.tree.refit)
    t.set_option(g.OPT_LEAF_MAX, s.leaf_max)
    if s.spheres is not None:
        t.upload_spheres(sphere_set(s.spheres))
    if s.table is not None:
        t.upload_tri_materials(*table_of(s.table, s.tree.mesh))
    if s.env is not None:
        t.upload_environment(env_texels(s.env[0]), filter=env_filter(s.env[0]), light=s.env[1])


_expected = {}
fresh_contexts = [0]   # opened so far, for the record in profiles/


def expected(state, args, init=None, first=1, make=None):
    """The observation on a fresh context that holds `state`; memoised on (canonical state, observation, first, the bytes of init)
    for the whole run, so that sequences which pass through the same state share the fresh context's answer."""
    key = (make, state.canon(), args, first, None if init is None else hashlib.sha1(np.ascontiguousarray(init).tobytes()).hexdigest())
    if key not in _expected:
        t = (make or g.PathTracer)(0)
        fresh_contexts[0] += 1
        try:
            install(t, state)
            _expected[key] = observe(t, state, args, init, first)
        finally:
            free_held(t)
            t.close()
    return _expected[key]


def free_held(t):
    for b in t.__dict__.pop("_sequence_soups", {}).values():
        b.free()


class Runner:
    """Applies a sequence to ONE long-lived context.  compare(step, ops, state, args, got, want) is called at every observation.
    Op("later", ...) is a render whose accumulator — a running mean carried from the previous "later" — is copied on the caller's
    stream into a buffer of its own (pt_temporal without a history: out = cur bit for bit, no scratch, no synchronisation); nothing
    is downloaded until Op("collect"), which compares every copy after one final sync."""

    def __init__(self, t, compare, make=None):
        self.t, self.compare, self.make = t, compare, make
        self.state = State()
        self.pending, self.carry, self.n_carried = [], None, 0

    def run(self, ops):
        try:
            for step, op in enumerate(ops):
                if op.kind == "obs":
                    assert op.valid(self.state), f"step {step}: {op!r} is not valid in {self.state}"
                    got = observe(self.t, self.state, op.args)
                    self.compare(step, ops, self.state, op.args, got, expected(self.state, op.args, make=self.make))
                elif op.kind == "later":
                    self._later(step, op, ops)
                elif op.kind == "collect":
                    self._collect(ops)
                else:
                    self.state = op.apply(self.t, self.state)
            self._collect(ops)
        finally:
            for b in [p[3] for p in self.pending] + getattr(self, "snaps", []):
                b.free()
            if self.carry is not None:
                for b in self.carry:
                    b.free()
            free_held(self.t)

    def _later(self, step, op, ops):
        kind, W, H, spp, depth, flags = op.args[:6]
        assert kind == "render" and op.args[6:] == (1, 1)
        t = self.t
        if self.carry is None:   # every buffer of the group now: no allocation between its calls
            group = list(itertools.takewhile(lambda o: o.kind != "collect", ops[step:]))
            self.size = (W, H)
            self.carry = [t.malloc(W * H * 12), t.malloc(W * H * 4), t.malloc(W * H * 16), t.malloc(W * H * 4)]   # accumulator, display words, zeros, lengths
            self.snaps = [t.malloc(W * H * 12) for o in group if o.kind == "later"]
            for b in self.carry:
                b.zero()
            self.n_carried = 0
        assert (W, H) == self.size, f"step {step}: the \"later\" renders of one group share their buffers, so their size: {(W, H)} after {self.size}"
        acc, rgba, zeros, length = self.carry
        first = 1 + self.n_carried
        rc = render_calls(t, self.state, op.args[1:], acc, rgba, first)
        snap = self.snaps.pop()
        t.temporal(W, H, None, None, None, None, None, None, acc.ptr, zeros.ptr, zeros.ptr, None, snap.ptr, length.ptr)
        self.pending.append((step, self.state, op.args, snap, rc, first))   # (the fresh contexts wait for "collect": nothing here blocks the host)
        self.n_carried += spp

    def _collect(self, ops):
        if self.pending:
            self.t.sync()
        pending, self.pending = self.pending, []
        gots = [{"rc": np.array([rc]), "acc": snap.download(np.float32, (args[2], args[1], 3))} for _, _, args, snap, rc, _ in pending]
        carried = None   # the fresh side's running mean: every call starts from what the fresh context before it left
        for (step, state, args, snap, rc, first), got in zip(pending, gots):
            snap.free()
            want = expected(state, args, carried, first, make=self.make)
            carried = want["acc"]
            self.compare(step, ops, state, args, got, {k: want[k] for k in got})
        if self.carry is not None:
            for b in self.carry:
                b.free()
            self.carry = None


def first_difference(got, want):
    """None when two observations agree bit for bit, else (output, flat index, got word, wanted word) of the first difference."""
    for name in want:
        if name not in got:
            return name, -1, None, None
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            return name, -1, a.shape, b.shape
        wa, wb = a.view(np.uint8).ravel(), b.view(np.uint8).ravel()
        if not np.array_equal(wa, wb):
            i = int(np.flatnonzero(wa != wb)[0]) // a.dtype.itemsize
            return name, i, a.ravel()[i], b.ravel()[i]
    extra = [k for k in got if k not in want]
    return (extra[0], -1, None, None) if extra else None


# ---------------------------------------------------------------------------------------------------- random sequences
def change_ops(s):
    """Every state change of the alphabet that is valid in s, by kind."""
    ops = {k: [] for k in CHANGE_KINDS}
    for m in MESHES:
        ops["upload_bvh"].append(Op("upload_bvh", m))
        ops["build_bvh"] += [Op("build_bvh", m, algo, leaf) for algo in (0, 1) for leaf in (1, 2)]
    ops["refit"] = [Op("refit", r) for r in REFITS]
    ops["spheres"] = [Op("spheres", n) for n in SPHERES]
    ops["table"] = [Op("table", n) for n in TABLES]
    ops["env"] = [Op("env", size, light) for size in ENVS for light in (False, True)] + [Op("env", None)]
    ops["opt"] = [Op("opt", name, v) for name, (_, _, values) in OPTIONS.items() for v in values]
    ops["stream"] = [Op("stream", "torch"), Op("stream", "own")]
    return {k: [o for o in v if o.valid(s)] for k, v in ops.items()}


def draw_observation(rng, s, kind=None):
    kinds = [k for k in OBS_KINDS if k != "envq" or s.env is not None]
    kind = kind or ("render" if rng.random() < 0.4 else kinds[rng.integers(len(kinds))])   # pt_render is the call this is about
    W, H = FRAMES[rng.integers(len(FRAMES))]
    spp, depth, flags = (int(x[rng.integers(len(x))]) for x in (SPPS, DEPTHS, FLAGS))
    if s.table is not None and s.table[0] == "cornell_box" and rng.random() < 0.5:
        flags = NEE   # (emissive triangles are on the context: the call that samples the light list)
    if kind == "render":
        calls = int(rng.integers(1, 3))
        parts = int(rng.integers(1, 4)) if H > 16 else 1
        return obs_render(W, H, spp, depth, flags, calls, parts)
    if kind in ("moments", "denoise", "temporal"):
        if (W, H) == (257, 131):
            W, H = 96, 64   # these make several calls per observation; the big frame is the plain render's
        return Op("obs", kind, W, H, spp, depth, flags)
    if kind == "rays":
        return Op("obs", "rays", bool(rng.integers(2)), spp, depth, flags)
    if kind == "hits":
        return Op("obs", "hits", bool(rng.integers(2)))
    return Op("obs", "envq")


def random_sequence(seed, length):
    """`length` operations, deterministic in the seed: about one in three an observation, one in ten a refused call, the rest state
    changes with the kinds equally likely; never an operation that is invalid in the shadow state it meets.  The first two
    operations put a tree and spheres up, so that most observations render something."""
    rng = np.random.default_rng(seed)
    s, ops = State(), []
    stub = StubTracer(0)
    while len(ops) < length:
        u = rng.random()
        if len(ops) == 0:
            op = (Op("upload_bvh", MESHES[rng.integers(4)]), Op("build_bvh", MESHES[rng.integers(4)], int(rng.integers(2)), int(rng.integers(1, 3))))[rng.integers(2)]
        elif len(ops) == 1:
            op = Op("spheres", SPHERES[rng.integers(3)])
        elif u < 1 / 3:
            op = draw_observation(rng, s)
        elif u < 1 / 3 + 0.1:
            valid = [Op("refused", r) for r in REFUSED if Op("refused", r).valid(s)]
            op = valid[rng.integers(len(valid))]
        else:
            by_kind = {k: v for k, v in change_ops(s).items() if v}
            kinds = sorted(by_kind)
            pick = by_kind[kinds[rng.integers(len(kinds))]]
            op = pick[rng.integers(len(pick))]
            if op.kind == "table" and Op("table", "cornell_box").valid(s) and rng.random() < 0.5:
                op = Op("table", "cornell_box")   # (the one table with lights in it)
            if op.kind == "env" and s.env is not None and rng.random() < 0.5:
                op = Op("env", None)   # (a map keeps the stage-split pipeline out: as many clears as uploads)
        ops.append(op)
        if not op.observes:
            s = op.apply(stub, s)
    return ops


# 8 seeds x 40 operations meet the coverage condition (tests/test_call_sequences.py).  Seven are 0 .. 6; the eighth is the first seed
# whose sequence samples the emissive triangles' light list, refits, and samples it again (relights below), so that a seed, not only
# DIRECTED["lights"], fails when the list goes stale.
SEEDS = (0, 1, 2, 3, 4, 5, 6, 12)
LENGTH = 40


def relights(ops):
    """Whether a sequence holds: a PT_FLAG_NEE call over cornell_box's emissive table, later a refit, later such a call again."""
    s, stub, stage = State(), StubTracer(0), 0
    for op in ops:
        if op.observes:
            a = op.args
            lit = s.table is not None and s.table[0] == "cornell_box" and ((a[0] == "render" and a[5] == NEE) or (a[0] == "rays" and a[4] == NEE))
            stage += lit and stage in (0, 2)
        elif op.kind != "collect":
            s = op.apply(stub, s)
            stage += stage == 1 and op.kind == "refit"
    return stage == 3


# ---------------------------------------------------------------------------------------------------- directed sequences
WAVE, PERSIST, MEGA, AUTO = g.KERNEL_WAVEFRONT, g.KERNEL_PERSISTENT, g.KERNEL_MEGA_BVH2, g.KERNEL_AUTO


def _grow_only():
    sizes = ((257, 131, 16, 4, NEE), (8, 8, 1, 1, 0), (96, 64, 3, 4, NEE), (37, 23, 4, 4, 0))
    ops = [Op("upload_bvh", "cornell"), Op("spheres", "reference"), Op("opt", "KERNEL", WAVE)]
    ops += [obs_render(*z) for z in sizes]
    ops += [Op("opt", "KERNEL", PERSIST), Op("opt", "OVERLAP", 1)]
    ops += [obs_render(*z, 2, 1) for z in sizes]
    for W, H in ((96, 64), (8, 8), (96, 64)):
        ops += [Op("obs", "denoise", W, H, 4, 2, 0), Op("obs", "moments", W, H, 3, 2, 0)]
    return ops


def _auto_table():
    """Ten configurations x five calls under PT_KERNEL_AUTO (the table holds eight), the first again (evicted: its trials start
    over, which test_gpu_call_sequences.py reads from auto_choice), then a tree, a material and a map change under one configuration."""
    cfgs = [(8, 8, 1, 2), (37, 23, 1, 2), (96, 64, 1, 2), (8, 8, 4, 2), (37, 23, 4, 2), (96, 64, 4, 4), (8, 8, 16, 4), (37, 23, 3, 4),
            (96, 64, 3, 1), (37, 23, 16, 2)]
    ops = [Op("upload_bvh", "cornell"), Op("spheres", "reference"), Op("opt", "KERNEL", AUTO)]
    for W, H, spp, depth in cfgs:
        ops += [obs_render(W, H, spp, depth, 0)] * 5
    ops += [obs_render(*cfgs[0], 0)] * 5
    AUTO_RESTARTS.append(len(ops) - 5)
    for change in (Op("build_bvh", "cornell", 1, 2), Op("table", "dark"), Op("env", "16x8", False), Op("env", None)):
        ops += [change] + [obs_render(*cfgs[0], 0)] * 5
        if change.kind == "env" and change.args[0] is not None:
            AUTO_UNCHANGED.append((len(ops) - 7, len(ops) - 5))
        else:
            AUTO_RESTARTS.append(len(ops) - 5)
    return ops


# steps of "auto-table" whose call is the first of a configuration the table does not hold (evicted; a new tree; a material table; the
# map cleared): the trials start over, so pt_auto_choice reports PT_KERNEL_AUTO.  With a map up a call consults no entry at all
# (plan_call: the pipeline is not eligible), so pt_auto_choice keeps answering for the entry looked up last: AUTO_UNCHANGED holds
# (the last step before the map, the first behind it), whose answers must be equal.
AUTO_UNCHANGED = []
AUTO_RESTARTS = []


def _lights():
    def body(between):
        # (the refit to "orig" is the tree's first, which synchronises: the one to "light" behind it does not.  The second upload of
        # cornell_box with the table still up changes scene_gen alone: the list collected from the MOVED quad must not survive it.)
        seq = [Op("upload_bvh", "cornell_box"), Op("table", "cornell_box"), "nee", Op("table", None), Op("upload_bvh", "cube"), "nee",
               Op("upload_bvh", "cornell_box"), Op("table", "cornell_box"), Op("refit", "orig"), "nee", Op("refit", "light"), "nee",
               Op("upload_bvh", "cornell_box"), "nee", Op("table", None), "nee", Op("table", "dark"), "nee"]
        # between: three calls back to back for one — in line on the idle stream, then the two side slots, the change behind them while
        # they run, so that the next call's side kernel has a light list (lights_ev) and a tree (geom_ev) to wait for
        look = [Op("later", "render", 257, 131, 4, 4, NEE, 1, 1)] * 3 if between else [obs_render(37, 23, 4, 4, NEE)]
        return [x for o in seq for x in (look if o == "nee" else [o])] + ([Op("collect")] if between else [])
    return ([Op("opt", "KERNEL", PERSIST)] + body(False) + [Op("table", None), Op("opt", "KERNEL", MEGA), Op("opt", "OVERLAP", 1)] + body(True))


def _side_slots():
    """plan_call puts a call on a side stream only while the caller's stream is busy, and every upload synchronises that stream.  So
    behind each change comes a burst of four calls back to back: a 16-sample one in line on the idle stream, a 4-sample one on slot 0
    while it runs, a 16-sample one on slot 1, a 4-sample one on slot 0 again behind the fold that reads it (fold_pending).  The two
    refits and the two set_option calls synchronise nothing (the refit to "orig" up front is the tree's first, which does): they sit
    between calls in flight, where the next side kernel must wait for geom_ev."""
    r, w = Op("later", "render", 257, 131, 4, 4, 0, 1, 1), Op("later", "render", 257, 131, 16, 4, 0, 1, 1)
    burst = [w, r, w, r]
    ops = [Op("upload_bvh", "cornell_box"), Op("spheres", "reference"), Op("opt", "KERNEL", PERSIST), Op("opt", "OVERLAP", 1), Op("refit", "orig")]
    for change in (Op("refit", "twist"), Op("spheres", "one-emitter"), Op("table", "cornell_box"), Op("env", "16x8", True), Op("env", None),
                   Op("refit", "light"), Op("opt", "WAVE_SAMPLES", 4), Op("opt", "OVERLAP", 0)):
        ops += burst + [change]
    return ops + [w, r, Op("collect")]


def _streams():
    r = Op("later", "render", 257, 131, 4, 4, 0, 1, 1)
    w = Op("later", "render", 257, 131, 16, 4, 0, 1, 1)
    ops = []
    for kernel in (PERSIST, WAVE):
        ops += [Op("stream", "own"), Op("build_bvh", "cornell", 1, 2), Op("refit", "orig"), Op("spheres", "reference"), Op("opt", "KERNEL", kernel),
                w, Op("stream", "torch"), r, Op("refit", "twist"), w, Op("stream", "own"), r, Op("collect")]
    return ops


def _records_across_a_stream_switch():
    """What pt_set_stream left unordered before it made the new stream wait for the old one: a 16-sample pipeline call on the context's
    own stream, the switch, a 4-sample call on the new stream.  The second call carves the shared path records (d_wave) for its own,
    smaller layout while the first still reads them by the larger one.  (DIRECTED["streams"] met an illegal memory access on the
    library without that wait; this is the shortest history that, read from the code, cannot go right without it.)"""
    return [Op("build_bvh", "cornell", 1, 2), Op("spheres", "reference"), Op("opt", "KERNEL", WAVE), Op("later", "render", 257, 131, 16, 4, 0, 1, 1),
            Op("stream", "torch"), Op("later", "render", 257, 131, 4, 4, 0, 1, 1), Op("collect")]


def _refit_owner():
    look = [Op("obs", "hits", True), obs_render(37, 23, 1, 2, 0)]
    return ([Op("spheres", "reference"), Op("build_bvh", "cornell", 1, 2), Op("refit", "twist")] + look + [Op("upload_bvh", "bunny_low"), Op("refit", "twist")] + look +
            [Op("build_bvh", "cornell", 1, 2), Op("refit", "drop")] + look + [Op("build_bvh", "cornell_perm", 1, 2), Op("refit", "twist")] + look)


def _refused_between():
    """Every refused call between two identical observations, every observation kind behind one."""
    ops = [Op("upload_bvh", "cornell_box"), Op("spheres", "reference"), Op("env", "5x3", True), Op("opt", "KERNEL", WAVE)]
    looks = [obs_render(37, 23, 4, 2, g.FLAG_MISS_KEEPS_PATH), Op("obs", "moments", 37, 23, 3, 2, 0), Op("obs", "rays", True, 3, 2, 0),
             Op("obs", "denoise", 37, 23, 4, 2, 0), Op("obs", "temporal", 37, 23, 1, 2, 0), Op("obs", "hits", False), Op("obs", "envq")]
    for i, r in enumerate(REFUSED):
        if r == "spp_2_20":
            ops.append(Op("env", None))
        look = looks[i % len(looks)] if r != "spp_2_20" else looks[0]
        ops += [look, Op("refused", r), look]
    ops += [Op("env", "5x3", True)]
    for look in looks:
        ops += [Op("refused", "null_accum"), look]
    return ops


def _every_option():
    """Every value the alphabet sets of every option, one at a time over the defaults, each with a frame behind it: the stage-split
    switches under PT_KERNEL_WAVEFRONT (PT_OPT_COUNTERS 1 with them, so that the values 2 differ from 1), the walks under each kernel."""
    ops = [Op("upload_bvh", "cornell"), Op("spheres", "reference")]
    look = obs_render(37, 23, 4, 4, 0)
    for kernel in OPTIONS["KERNEL"][2]:
        ops.append(Op("opt", "KERNEL", kernel))
        for walk in (0, 1, 4, 2):
            ops += [Op("opt", "WALK", walk), look]
    for name in ("OVERLAP", "TIMING", "FUSE_STAGES", "FIRST_WALK", "WAVE_SAMPLES", "LAST_ANYHIT", "ROOT_CULL", "ROOT_ENTRY", "PATH_HISTORY"):
        _, default, values = OPTIONS[name]
        for v in values:
            if v != default:
                ops += [Op("opt", name, v), look] + ([Op("opt", "COUNTERS", 1), look, Op("opt", "COUNTERS", 0)] if v == 2 else [])
        ops.append(Op("opt", name, default))
    return ops


DIRECTED = {
    "grow-only": _grow_only(),
    "auto-table": _auto_table(),
    "lights": _lights(),
    "side-slots": _side_slots(),
    "streams": _streams(),
    "refit-owner": _refit_owner(),
    "refused-between": _refused_between(),
    "every-option": _every_option(),
    "records-across-a-stream-switch": _records_across_a_stream_switch(),
}


def all_sequences():
    return {**{f"seed-{s}": random_sequence(s, LENGTH) for s in SEEDS}, **DIRECTED}


# ---------------------------------------------------------------------------------------------------- the coverage condition
def coverage(sequences):
    """(pairs, after_refused): the ordered pairs (state-changing kind, observation kind) that occur with no other state change of
    the SAME kind in between, and the observation kinds that directly follow a refused call."""
    pairs, after_refused = set(), set()
    for ops in sequences:
        live, prev = set(), None
        for op in ops:
            if op.observes:
                pairs |= {(k, op.args[0]) for k in live}
                if prev is not None and prev.kind == "refused":
                    after_refused.add(op.args[0])
            elif op.kind in CHANGE_KINDS:
                live.add(op.kind)   # (a second change of the same kind replaces the first: the later one is what the pair means)
            prev = op
    return pairs, after_refused


# ---------------------------------------------------------------------------------------------------- a context without a GPU
class StubViolation(AssertionError):
    pass


class _StubBuffer:
    def __init__(self, owner, nbytes):
        self.owner, self.nbytes, self.ptr = owner, nbytes, owner._next_ptr()

    def zero(self):
        pass

    def upload(self, arr):
        assert np.ascontiguousarray(arr).nbytes <= self.nbytes

    def download(self, dtype, shape):
        out = np.zeros(shape, dtype)
        assert out.nbytes <= self.nbytes, "a download past the end of its buffer"
        return out

    def free(self):
        self.ptr = None


class StubTracer:
    """PathTracer's surface with a model of the host's checks and no device: records (name, arguments) in `calls`, raises PtError
    with the documented code where the library refuses, and StubViolation where a call would reach a kernel with bad data."""

    def __init__(self, device=0):
        self.calls, self._ptr = [], 0x1000
        self.n_tree = self.n_table = self.n_spheres = 0   # triangles of the tree (0: none), rows of the table, spheres
        self.env, self.opts, self.stream = None, {}, None

    def _next_ptr(self):
        self._ptr += 0x1000
        return self._ptr

    def _rec(self, name, *a):
        self.calls.append((name,) + a)

    def _refuse(self, code, why):
        self._rec("refused", code, why)
        raise g.PtError(code, why)

    def _opt(self, name):
        return self.opts.get(OPTIONS[name][0], OPTIONS[name][1])

    def close(self):
        self._rec("close")

    def sync(self):
        self._rec("sync")

    def malloc(self, nbytes):
        if nbytes <= 0:
            raise StubViolation("pt_malloc of nothing")
        return _StubBuffer(self, nbytes)

    def alloc_frame(self, W, H):
        return self.malloc(W * H * 12), self.malloc(W * H * 4)

    def set_stream(self, h):
        self._rec("set_stream", h)
        self.stream = h

    def set_option(self, opt, value):
        ranges = {g.OPT_KERNEL: (0, 1, 3, 5), g.OPT_WALK: (0, 1, 2, 4), g.OPT_BUILD_ALGO: (0, 1), g.OPT_LEAF_MAX: range(0, 1025), _abi.OPT_ENV_LIGHT: (0, 1),
                  g.OPT_FUSE_STAGES: (0, 1), g.OPT_FIRST_WALK: (0, 1), g.OPT_WAVE_SAMPLES: range(1, 65), g.OPT_LAST_ANYHIT: (0, 1, 2),
                  g.OPT_ROOT_CULL: (0, 1, 2), _abi.OPT_ROOT_ENTRY: (0, 1, 2), _abi.OPT_PATH_HISTORY: (0, 1, 2)}
        if opt in ranges and value not in ranges[opt]:
            self._refuse(PT_ERR_UNSUPPORTED if opt == g.OPT_KERNEL else PT_ERR_INVALID, "option value out of range")
        if opt not in ranges and opt not in (g.OPT_OVERLAP, g.OPT_COUNTERS, g.OPT_TIMING):
            raise StubViolation(f"option {opt} is not in the alphabet")
        self._rec("set_option", opt, value)
        self.opts[opt] = value

    def _tree(self, n, what):
        if self.n_table and n > self.n_table:
            self._refuse(PT_ERR_INVALID, f"{what}: the material table does not cover the tree")
        self._rec(what, n)
        self.n_tree = n

    def upload_bvh(self, bvh):
        real = bvh.index[np.ascontiguousarray(bvh.tris, np.float32).view(np.uint32)[:, 0] != 0x80000000]   # not a leaf's terminator
        if np.any(real < 0) or np.any(real >= (1 << 30)):
            self._refuse(PT_ERR_INVALID, "triangle id out of range")
        self._tree(int(real.max()) + 1, "upload_bvh")

    def build_bvh(self, mesh):
        if not np.all(np.abs(mesh.verts) <= 3.0e38):
            self._refuse(PT_ERR_INVALID, "non-finite vertex")
        self._tree(int(mesh.n_tris), "build_bvh")
        return 0.0

    def refit_bvh(self, verts, n_tris=None, n_dropped=None):
        n = verts.nbytes // 36 if n_tris is None else n_tris
        if not self.n_tree:
            self._refuse(PT_ERR_NO_SCENE, "refit without a tree")
        if n < self.n_tree:
            self._refuse(PT_ERR_INVALID, "refit: n_tris does not cover the tree")
        if n * 36 > verts.nbytes:
            raise StubViolation("refit would read past its vertex buffer")
        self._rec("refit_bvh", n)

    def upload_spheres(self, spheres):
        self.n_spheres = len(spheres) if spheres is not None else 0
        self._rec("upload_spheres", self.n_spheres)

    def upload_tri_materials(self, table, ids):
        n = 0 if table is None or len(table) == 0 else len(ids)
        if n and self.n_tree > n:
            self._refuse(PT_ERR_INVALID, "table does not cover the tree")
        if n and (np.min(ids) < 0 or np.max(ids) >= len(table)):
            self._refuse(PT_ERR_INVALID, "material index out of range")
        self.n_table = n
        self._rec("upload_tri_materials", n)

    def upload_environment(self, texels, filter=1, light=False, **kw):
        if not (np.all(np.isfinite(texels)) and np.all(texels >= 0)):
            self._refuse(PT_ERR_INVALID, "texel")
        self.env = (texels.shape, bool(light))
        self._rec("upload_environment", texels.shape, filter, bool(light))

    def clear_environment(self):
        self.env = None
        self._rec("clear_environment")

    def environment_is_light(self):
        return bool(self.env and self.env[1])

    def scene_info(self):
        if not self.n_tree:
            self._refuse(PT_ERR_NO_SCENE, "scene_info")
        return dict(n_inner=0, n_tri_refs=self.n_tree, n_leaves=0, max_depth=0, device_bytes=0)

    def last_build_ms(self):
        return -1.0

    def counters(self):
        return dict.fromkeys(("rays", "inner", "tris", "leaves", "hits", "paths"), 0)

    def _need(self, ok, code, why):
        if not ok:
            self._refuse(code, why)

    def launch_kernel(self, acc, rgba, cam, p, spp=1, moments_ptr=None):
        self._need(acc and p.width >= 2 and p.height >= 2 and spp >= 1 and p.sample_index >= 1, PT_ERR_INVALID, "pt_render: argument")
        self._need(not (p.flags & g.FLAG_NEE) or p.flags & g.FLAG_COSINE_DIFF, PT_ERR_INVALID, "NEE without COSINE_DIFF")
        self._need(self.n_tree or self.n_spheres, PT_ERR_NO_SCENE, "pt_render: no scene")
        if p.part_count > 1:
            self._need(0 <= p.part_index < p.part_count and p.part_rows > 0 and p.part_rows % 8 == 0, PT_ERR_INVALID, "partition")
        wave = self.n_tree and p.depth > 0 and self._opt("WALK") == 2 and self.env is None and self._opt("KERNEL") == g.KERNEL_WAVEFRONT
        self._need(not (wave and spp >= 1 << 20), PT_ERR_UNSUPPORTED, "the pipeline packs < 2^20 samples per call")
        if spp >= 1 << 20:
            raise StubViolation("a call of 2^20 samples would run")
        self._rec("render", p.width, p.height, spp, p.depth, p.flags)

    def frame_error(self, mom, W, H, n, thr=0.0):
        self._need(mom and W >= 1 and H >= 1 and n >= 2, PT_ERR_INVALID, "frame_error")
        self._rec("frame_error", W, H, n)
        return 0.0, 0

    def _rays(self, name, need_tree, *ptrs):
        self._need(self.n_tree if need_tree else (self.n_tree or self.n_spheres), PT_ERR_NO_SCENE, name)
        self._need(all(ptrs), PT_ERR_INVALID, name + ": null")
        self._rec(name)

    def trace_rays(self, rays, n, cull, t, tri, nrm=None):
        self._rays("trace_rays", True, rays, t, tri)

    def closest_hits(self, rays, n, cull, t, tri, nrm=None):
        self._rays("closest_hits", True, rays, t, tri)

    def any_hits(self, rays, n, cull, hit):
        self._rays("any_hits", True, rays, hit)

    def render_rays(self, rays, n, out, p, spp=1, first_index=0, hdr=False):
        self._rays("render_rays", False, rays, out)

    def render_aux(self, cam, p, alb, nrm, pos, ids=None):
        self._rays("render_aux", True, alb, nrm, pos)

    def denoise(self, color, alb, nrm, pos, W, H, out, rgba=None, **kw):
        self._need(color and alb and nrm and pos and out and W >= 1 and H >= 1, PT_ERR_INVALID, "denoise")
        self._rec("denoise", W, H)

    def temporal(self, W, H, prev_cam, pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, rgba=None, **kw):
        self._need(cc and cn and cp and oc and ol and W >= 2 and H >= 2, PT_ERR_INVALID, "temporal")
        self._need(pc is None or (prev_cam is not None and pl and pn and pp and oc != pc and ol != pl), PT_ERR_INVALID, "temporal history")
        self._rec("temporal", W, H)

    def eval_environment(self, rays, n, out):
        self._need(self.env, PT_ERR_NO_SCENE, "no map")
        self._rec("eval_environment")

    def sample_environment(self, u, n, dp, rad=None):
        self._need(self.env, PT_ERR_NO_SCENE, "no map")
        self._need(self.env[1], PT_ERR_UNSUPPORTED, "the map is no light")
        self._rec("sample_environment")

    def environment_pdf(self, rays, n, pdf):
        self._need(self.env, PT_ERR_NO_SCENE, "no map")
        self._need(self.env[1], PT_ERR_UNSUPPORTED, "the map is no light")
        self._rec("environment_pdf")
