"""The inputs of tests/test_gpu_scene_matrix.py: camera poses, sphere sets, meshes with coincident triangles and the grids whose
shared edges make exact ties.  tests/test_scene_matrix_oracle.py checks the oracle on them (CPU only)."""
import numpy as np

import gpu_pathtracer_amd as g

# the dragon of cornell_dragon: ids >= N_ROOM (the room's 32 triangles come first)
N_ROOM = g.Mesh.asset("cornell").n_tris


def _dragon_box():
    m = g.scene_mesh("cornell_dragon")
    v = np.asarray(m.verts, np.float64)[np.asarray(m.tris)[N_ROOM:]].reshape(-1, 3)
    return v.min(0), v.max(0)


DRAGON_LO, DRAGON_HI = _dragon_box()
DRAGON_C = 0.5 * (DRAGON_LO + DRAGON_HI)


# ---------------------------------------------------------------------------------------------------- cameras
def make_camera(W, H, pos, front, up=(0.0, 1.0, 0.0), roll=0.0, fov=1.0, dist=None):
    """A camera basis built in float64 (right = front x up, up = right x front, then turned by `roll` about front), stored as
    float32.  dist defaults to golden_camera's 18 H / 1080."""
    f = np.asarray(front, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    r, u = np.cos(roll) * r + np.sin(roll) * u, np.cos(roll) * u - np.sin(roll) * r
    cam = g.default_camera(W, H)
    cam.pos[:] = [np.float32(x) for x in pos]
    cam.front[:] = [np.float32(x) for x in f]
    cam.right[:] = [np.float32(x) for x in r]
    cam.up[:] = [np.float32(x) for x in u]
    cam.fov = np.float32(fov)
    cam.dist = np.float32(18.0 * H / 1080.0 if dist is None else dist)
    return cam


def yaw_pitch(yaw, pitch):
    return (np.sin(yaw) * np.cos(pitch), np.sin(pitch), -np.cos(yaw) * np.cos(pitch))


FAR_DIR = np.array([0.2, 0.1, 1.0]) / np.linalg.norm([0.2, 0.1, 1.0])
# name: (camera arguments, with the sphere room).  Away looks out of the open front of the box into empty space.
POSES = {
    "control": (dict(pos=(0, 0, 0), front=(0, 0, -1)), True),
    "reversed": (dict(pos=(1.0, -6.0, -57.0), front=(0.05, 0.1, 1.0)), True),
    "top-down": (dict(pos=(-2.0, 10.0, -36.0), front=(0, -1, 0), up=(0, 0, -1)), True),
    "along-x": (dict(pos=(-14.5, -8.0, -36.0), front=(1, 0, 0)), True),
    "oblique": (dict(pos=(9.0, 4.0, -18.0), front=yaw_pitch(-0.55, -0.45), roll=0.35), True),
    "inside": (dict(pos=tuple(DRAGON_C), front=(0.5, 0.3, -1.0)), True),
    "wide": (dict(pos=(0.0, -2.0, -18.0), front=(0, 0, -1), fov=6.0), True),
    "narrow": (dict(pos=(0, 0, 0), front=(13.0, -1.985, -35.0), fov=1e-3), True),    # the mirror sphere's rim on the back wall
    "far": (dict(pos=tuple(DRAGON_C + 5000.0 * FAR_DIR), front=tuple(-FAR_DIR), fov=2.4e-3), False),
    "away": (dict(pos=(0.0, 0.0, 10.0), front=(0.1, 0.05, 1.0)), False),
}


def pose_camera(name, W, H):
    kw, _ = POSES[name]
    return make_camera(W, H, **kw)


def pose_spheres(name):
    return g.reference_spheres() if POSES[name][1] else None


# ---------------------------------------------------------------------------------------------------- sphere sets
def spheres(rows):
    """rows of (x, y, z, r, emission, colour, material) as a pt_sphere array"""
    arr = (g.Sphere * len(rows))()
    for s, (x, y, z, r, emi, col, mat) in zip(arr, rows):
        s.pos_rad[:] = [np.float32(v) for v in (x, y, z, r)]
        s.emi[:] = [np.float32(v) for v in emi]
        s.col[:] = [np.float32(v) for v in col]
        s.mat = mat
    return arr


def rows_of(arr):
    return [(*s.pos_rad, tuple(s.emi), tuple(s.col), s.mat) for s in arr]


GLASS = (8.0, 4.0, -20.0, 4.0, (0, 0, 0), (1, 1, 1), g.MAT_REFR)          # in front of the box's opening
METAL = (-9.0, 6.0, -40.0, 3.0, (0, 0, 0), (0.9, 0.7, 0.3), g.MAT_METAL)
LAMP = (-4.0, 3.0, -36.0, 2.5, (6.0, 5.0, 3.0), (0.5, 0.5, 0.5), g.MAT_DIFF)
WALLS = rows_of(g.reference_spheres())[:6]


def many_spheres():
    """the reference set and 32 small spheres inside the box: all four materials, emitters below and above index 8"""
    rows = rows_of(g.reference_spheres())
    mats = (g.MAT_DIFF, g.MAT_METAL, g.MAT_SPEC, g.MAT_REFR)
    for i in range(32):
        x, y, z = -12.0 + 8.0 * (i % 4), -3.0 + 5.5 * ((i // 4) % 3), -54.0 + 7.0 * (i // 12)
        emi = (3.0, 2.0 + 0.1 * i, 1.0) if i % 5 == 0 else (0, 0, 0)
        rows.append((x, y, z, 1.2 + 0.1 * (i % 3), emi, (0.3 + 0.02 * i, 0.6, 0.9 - 0.02 * i), mats[i % 4]))
    return spheres(rows)


def unreachable_spheres():
    """the reference set and 24 spheres that lie wholly inside the solid wall spheres: a ray that starts in the room meets
    the wall first, so none of them can ever be the closest hit"""
    rows = rows_of(g.reference_spheres())
    for i in range(24):
        cx, cy, cz, _ = rows[i % 6][0:4]
        off = np.array([np.sin(1.7 * i), np.cos(2.3 * i), np.sin(0.9 * i + 1.0)])
        c = np.array([cx, cy, cz]) + 300.0 * off / np.linalg.norm(off)
        rows.append((*c, 20.0 + i, (1.0, 0.5, 0.25), (0.8, 0.8, 0.8), (g.MAT_DIFF, g.MAT_METAL, g.MAT_SPEC, g.MAT_REFR)[i % 4]))
    return spheres(rows)


SPHERE_SETS = {
    "one-emitter": lambda: spheres([LAMP]),
    "seven-metal-glass": lambda: spheres(WALLS[:5] + [METAL, GLASS]),
    "nine-global": lambda: spheres(rows_of(g.reference_spheres()) + [GLASS]),
    "forty": many_spheres,
    "inside-glass": lambda: spheres(rows_of(g.reference_spheres()) + [(0.0, 0.0, -3.0, 6.0, (0, 0, 0), (1, 1, 1), g.MAT_REFR)]),
}
STALE_THREE = lambda: spheres([WALLS[0], WALLS[4], GLASS])   # noqa: E731
SPHERES_ONLY = lambda: spheres(rows_of(g.reference_spheres()) + [GLASS, METAL, LAMP])   # noqa: E731


# ---------------------------------------------------------------------------------------------------- coincident triangles
def copy_rows(mesh):
    """the triangles that get an identical copy: the 32 room triangles and every 7th dragon triangle"""
    return np.concatenate([np.arange(N_ROOM), np.arange(N_ROOM, mesh.n_tris, 7)])


def duplicated(mesh, reverse=False):
    """mesh + copies of copy_rows(mesh) at higher ids (same vertex indices, so bit-identical vertices; reverse: the copies'
    winding reversed).  Returns (mesh, number of original triangles)."""
    f = np.asarray(mesh.tris, np.int32)
    c = f[copy_rows(mesh)]
    if reverse:
        c = c[:, ::-1]
    return g.Mesh.from_arrays(np.asarray(mesh.verts, np.float32), np.ascontiguousarray(np.concatenate([f, c]), np.int32)), len(f)


def red_copies_table(n_orig, n_all, p):
    """row 0 = the global material of p, row 1 = a red emitter for the copies: a copy that wins a tie shows up red"""
    m0, m1 = g.Material(), g.Material()
    m0.col[:], m0.emi[:], m0.mat, m0.phong_expo = list(p.tri_col), list(p.tri_emi), p.tri_mat, p.phong_expo
    m1.col[:], m1.emi[:], m1.mat, m1.phong_expo = (1, 0, 0), (40, 0, 0), g.MAT_DIFF, 0.0
    ids = np.zeros(n_all, np.int32)
    ids[n_orig:] = 1
    return [m0, m1], ids


def grid_mesh(n=8):
    """three integer grids of n x n unit squares (two triangles each, alternating diagonals), one per axis plane"""
    verts, tris = [], []
    for axis, off in ((2, -3.0), (0, 5.0), (1, -6.0)):
        base = len(verts)
        for j in range(n + 1):
            for i in range(n + 1):
                p = [0.0, 0.0, 0.0]
                a, b = [k for k in range(3) if k != axis]
                p[a], p[b], p[axis] = float(i), float(j), off
                verts.append(p)
        for j in range(n):
            for i in range(n):
                v00, v10 = base + j * (n + 1) + i, base + j * (n + 1) + i + 1
                v01, v11 = v00 + n + 1, v10 + n + 1
                if (i + j) % 2:
                    tris += [[v00, v10, v11], [v00, v11, v01]]
                else:
                    tris += [[v00, v10, v01], [v10, v11, v01]]
    return g.Mesh.from_arrays(np.array(verts, np.float32), np.array(tris, np.int32))


def grid_rays(n=8):
    """rays through every shared edge midpoint and vertex of the grids (and through the cell centres), from both sides of
    each grid.  The directions are small binary fractions, (1/4, -1/8) across the grid and 1 along its normal, unnormalised,
    so every ray meets its target at t = 4 exactly, the triangles that share the edge or vertex report the same t, and the
    tie goes to the smaller id.  No direction component is zero: a ray that lies IN a bounding plane (an axis-aligned ray
    along a shared edge) is kept or culled by the slab test according to which side of it the box lies, so even the oracle's
    own walk leaves brute force there."""
    rays = []
    for axis, off in ((2, -3.0), (0, 5.0), (1, -6.0)):
        a, b = [k for k in range(3) if k != axis]
        for j2 in range(0, 2 * n + 1):
            for i2 in range(0, 2 * n + 1):
                for sgn in (1.0, -1.0):
                    tgt, d = [0.0] * 3, [0.0] * 3
                    tgt[a], tgt[b], tgt[axis] = i2 / 2.0, j2 / 2.0, off
                    d[a], d[b], d[axis] = 0.25, -0.125, -sgn
                    rays.append([tgt[k] - 4.0 * d[k] for k in range(3)] + [0.0] + d + [0.0])
    return np.array(rays, np.float32)


def axis_rays(n=8):
    """axis-aligned rays exactly along the grids' shared edges and through their vertices: each lies IN bounding planes of
    the tree (a zero direction component, the slab test's 0 x 2^80 case), so whether a box keeps it depends on the box; the
    binary walk over the same boxes must still give the oracle's walk bit for bit"""
    rays = []
    for axis, off in ((2, -3.0), (0, 5.0), (1, -6.0)):
        a, b = [k for k in range(3) if k != axis]
        for j2 in range(0, 2 * n + 1):
            for i2 in range(0, 2 * n + 1):
                for sgn in (1.0, -1.0):
                    o, d = [0.0] * 3, [0.0] * 3
                    o[a], o[b], o[axis] = i2 / 2.0, j2 / 2.0, off + 4.0 * sgn
                    d[axis] = -sgn
                    rays.append(o + [0.0] + d + [0.0])
    return np.array(rays, np.float32)


# ---------------------------------------------------------------------------------------------------- ties inside a frame
def tilted_grid(n=8):
    """n x n unit squares on the plane z = -3 + x / 2 + y / 4 (every vertex exact in binary32), each split along its
    (i, j)-(i + 1, j + 1) diagonal, both triangles wound counter-clockwise seen from +z.  Returns the mesh and the midpoints
    (x, y) of the diagonals, in the order of the squares: square k holds triangles 2k and 2k + 1.

    A ray along -z through a midpoint meets both triangles of its square at the same t, exactly: the edges are small dyadic
    vectors and the determinant is 1, so Moller-Trumbore's t, u, v are exact.  The tie goes to 2k.  The midpoint has
    half-integer x and y, and every bounding plane of the tree lies at an integer x or y (the vertices'), so the ray never
    lies in a bounding plane: its hits do not depend on the walk."""
    verts = [(float(i), float(j), -3.0 + i / 2.0 + j / 4.0) for j in range(n + 1) for i in range(n + 1)]
    tris, mids = [], []
    for j in range(n):
        for i in range(n):
            v00, v10 = j * (n + 1) + i, j * (n + 1) + i + 1
            v01, v11 = v00 + n + 1, v10 + n + 1
            tris += [[v00, v10, v11], [v00, v11, v01]]
            mids.append((i + 0.5, j + 0.5))
    return g.Mesh.from_arrays(np.array(verts, np.float32), np.array(tris, np.int32)), mids


def tilted_grid_table(n_tris):
    """one emissive DIFF row per triangle, emission ((id + 1) / 256, 0.5, 0.25): at depth 1 a pixel's colour names the
    triangle its primary ray hit (below the accumulator's clamp at 1)"""
    rows = []
    for k in range(n_tris):
        m = g.Material()
        m.col[:], m.emi[:], m.mat, m.phong_expo = (0.5, 0.5, 0.5), ((k + 1) / 256.0, 0.5, 0.25), g.MAT_DIFF, 0.0
        rows.append(m)
    return rows, np.arange(n_tris, dtype=np.int32)


def pinhole_camera(x, y, from_below=False):
    """fov 0: every pixel's primary ray, jitter or not, is the same ray along -z (from above) or +z (from below) through
    (x, y); the camera's ray origin pos + front * dist is exact"""
    if from_below:
        return make_camera(2, 2, pos=(x, y, -30.0), front=(0, 0, 1), fov=0.0, dist=1.0)
    return make_camera(2, 2, pos=(x, y, 10.0), front=(0, 0, -1), fov=0.0, dist=1.0)


PINHOLE_SIDES = {"above-cull": (False, 1), "below-nocull": (True, 0)}   # side: (from below, cull_backfaces)


def pinhole_params(cull):
    p = g.default_params(2, 2, depth=1)
    p.cull_backfaces = cull
    p.bk_color[:] = (0, 0, 0)
    p.flags = g.FLAG_WRITE_RGBA
    return p

