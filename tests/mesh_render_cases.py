"""Meshes, views and mirror results shared by test_cpu_mesh_render.py and test_gpu_mesh_render.py.

A view is (T_w2c [4,4], fx, fy, cx, cy, H, W); pixel (x, y) is centred at u = x, v = y.

Sizes.  The render works in blocks of 256 faces and 256 pixels; a face whose clamped box holds more than 1024 pixels takes
the large-face launch, whose 256 workgroups stride the list of such faces; the cull scans in blocks of 256.
  70 x 45                 H W = 3150 is no multiple of 256 (empty_faces, empty_all, odd, large_boxes, large33)
  odd                     1003 faces: four blocks, the last partial
  large_boxes             boxes of exactly 1024 (lane), 1025 (workgroup) and the whole image (workgroup)
  large33                 33 large faces; with large_grid = 8 the launch strides its list five times
  snap_limit              vertices snapped at exactly +-2^24 (kept) and one step beyond (skipped)
  pillar_room (visibility and cull)   V = 636 and F = 960, past 256 and no multiple of it"""
import functools

import numpy as np

import mesh_clean_cases as MC
import mesh_eval_cases as K


def look(H, W, f, T=None, cx=None, cy=None):
    T = np.eye(4, dtype=np.float32) if T is None else np.asarray(T, np.float32)
    return (T, float(f), float(f), 0.5 * (W - 1) if cx is None else float(cx), 0.5 * (H - 1) if cy is None else float(cy),
            H, W)


def pose(yaw=0.0, pitch=0.0, centre=(0.0, 0.0, 0.0)):
    """World-to-camera of a camera at `centre` that looks along +z turned by `yaw` about y, then `pitch` about x."""
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    R = (Ry @ Rx).T                                           # camera-to-world is Ry Rx
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ np.asarray(centre, np.float64)
    return T.astype(np.float32)


def look_at(centre, target=(0.0, 0.0, 0.0)):
    """World-to-camera of a camera at `centre` whose +z axis points at `target`."""
    c, t = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, y, z])
    T[:3, 3] = -T[:3, :3] @ c
    return T.astype(np.float32)


def from_pixels(tris, view):
    """Triangles given as three (u, v, z) corners each, in pixels and depth, under an identity pose: (verts, faces)."""
    _, fx, fy, cx, cy, _, _ = view
    t = np.asarray(tris, np.float64).reshape(-1, 3)
    v = np.stack([(t[:, 0] - cx) / fx * t[:, 2], (t[:, 1] - cy) / fy * t[:, 2], t[:, 2]], 1).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def grid_wall(origin, du, dv, n):
    """(n + 1)^2 vertices origin + i du / n + j dv / n and 2 n^2 triangles."""
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    i, j = (t.reshape(-1) for t in np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"))
    v = o + i[:, None] * du / n + j[:, None] * dv / n
    i, j = (t.reshape(-1) for t in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    return v.astype(np.float32), np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def box(lo, hi, n):
    """The six walls of the box [lo, hi], each n x n quads; the walls share positions along their edges, not indices."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = np.diag(hi - lo)
    walls = []
    for ax in range(3):
        a, b = e[(ax + 1) % 3], e[(ax + 2) % 3]
        walls.append(grid_wall(lo, a, b, n))
        walls.append(grid_wall(lo + e[ax], a, b, n))
    return merge(walls)


def merge(meshes):
    vs, fs, first = [], [], 0
    for v, f in meshes:
        vs.append(v), fs.append(f + first)
        first += v.shape[0]
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def uv_sphere(radius=1.0, centre=(0.0, 0.0, 0.0), n_lat=16, n_lon=32):
    """A closed sphere: two poles, n_lat - 1 rings of n_lon vertices; no degenerate face."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.cos(th)[:, None] * np.ones_like(ph)[None, :]], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    f = []
    idx = lambda r, k: 1 + r * n_lon + k % n_lon
    for k in range(n_lon):
        f.append((0, idx(0, k), idx(0, k + 1)))
        f.append((len(v) - 1, idx(n_lat - 2, k + 1), idx(n_lat - 2, k)))
        for r in range(n_lat - 2):
            f.append((idx(r, k), idx(r + 1, k), idx(r + 1, k + 1)))
            f.append((idx(r, k), idx(r + 1, k + 1), idx(r, k + 1)))
    return v.astype(np.float32), np.asarray(f, np.int32)


# ---- the render cases ------------------------------------------------------------------------------------------------
SQUARE_VIEW = look(16, 16, 16.0, cx=8.0, cy=8.0)
SQUARE_CORNERS = (3, 4, 11, 12)                              # x0, y0, x1, y1: vertices ON pixel centres


def case_square():
    """A fronto-parallel square at depth 2.0, two triangles that share the diagonal (3,4)-(11,12)."""
    x0, y0, x1, y1 = SQUARE_CORNERS
    c = [(x0, y0, 2.0), (x1, y0, 2.0), (x1, y1, 2.0), (x0, y1, 2.0)]
    v = from_pixels(c + c[:2], SQUARE_VIEW)[0][:4]
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), SQUARE_VIEW


SLANT = (2.0, 0.3, 0.2)                                      # the plane z = c + a x + b y in the camera's frame
SLANT_VIEW = look(45, 70, 60.0)


def case_slanted():
    """The slanted plane over the rectangle [-2,2] x [-1.5,1.5], which contains the whole view."""
    c, a, b = SLANT
    xy = np.array([[-2, -1.5], [2, -1.5], [2, 1.5], [-2, 1.5]], np.float64)
    v = np.concatenate([xy, (c + a * xy[:, :1] + b * xy[:, 1:])], 1).astype(np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), SLANT_VIEW


ROOM = ((-2.0, -1.5, -2.0), (2.0, 1.5, 2.0))
WIDE_VIEW = look(32, 48, 40.0, pose(0.07, -0.04, (0.1, -0.05, -1.5)))       # sees the far wall and the ends of four others
NARROW_VIEW = look(32, 48, 48.0, pose(0.02, 0.0, (0.0, 0.0, -1.5)))         # sees the far wall (and the pillar) only
PILLAR = ((-0.3, -1.5, 0.2), (0.3, 1.5, 0.8))


def case_box_inside():
    """The closed room seen from inside: every pixel is covered."""
    return box(*ROOM, 8) + (WIDE_VIEW,)


def case_pillar_room():
    """The room with a floor-to-ceiling pillar between the camera and the far wall."""
    return merge([box(*ROOM, 8), box(*PILLAR, 4)]) + (NARROW_VIEW,)


VIEW_70 = look(45, 70, 16.0, cx=35.0, cy=22.0)


def case_empty_faces():
    return np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32), VIEW_70


def case_empty_all():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), VIEW_70


def case_odd():
    """The 1003-face mesh of mesh_eval_cases from 14 units away."""
    v, f = K.mesh_odd()
    return v, f, look(45, 70, 40.0, pose(0.0, 0.0, (0.0, 0.0, -14.0)))


def _floater_view(yaw):
    c = np.array([11.5, 11.5, 11.5])
    back = np.array([-np.sin(yaw), 0.0, -np.cos(yaw)]) * 26.0
    return look(48, 64, 64.0, pose(yaw, 0.0, c + back))


def case_floaters_a():
    v, f, _ = MC.floater_mesh()
    return v, f, _floater_view(0.0)


def case_floaters_b():
    v, f, _ = MC.floater_mesh()
    return v, f, _floater_view(0.6)


def case_behind_and_nan():
    """Face 0 is drawn, face 1 has a vertex behind z_near, face 2 a NaN vertex, face 3 an infinite one."""
    v, f = from_pixels([(2, 2, 2.0), (12, 3, 2.0), (4, 13, 2.5), (3, 3, 1.0), (10, 3, 1.0), (5, 9, 0.15),
                        (1, 1, 1.5), (9, 2, 1.5), (2, 9, 1.5), (6, 6, 1.2), (14, 7, 1.2), (7, 14, 1.2)], SQUARE_VIEW)
    v[6, 1] = np.nan
    v[11, 0] = np.inf
    return v, f, SQUARE_VIEW


def case_bad_index():
    v, f = from_pixels([(2, 2, 2.0), (12, 3, 2.0), (4, 13, 2.5), (3, 3, 1.0), (10, 3, 1.0), (5, 9, 1.0),
                        (1, 1, 1.5), (9, 2, 1.5), (2, 9, 1.5)], SQUARE_VIEW)
    f = f.copy()
    f[1, 2] = v.shape[0]
    f[2, 0] = -1
    return v, f, SQUARE_VIEW


def case_zero_area():
    """Face 0 names a vertex twice, face 1 has three collinear snapped vertices, face 2 is drawn."""
    v, f = from_pixels([(2, 2, 2.0), (12, 3, 2.0), (4, 13, 2.5), (3, 3, 1.0), (6, 6, 1.0), (9, 9, 1.0),
                        (1, 1, 4.0), (14, 2, 4.0), (2, 14, 4.0)], SQUARE_VIEW)
    f = f.copy()
    f[0, 2] = f[0, 1]
    return v, f, SQUARE_VIEW


def case_coplanar_duplicates():
    """The same slanted triangle three times over separate vertices and once more by the indices of face 0: four equal
    depths at every covered pixel, the smallest face id wins."""
    tri = [(2.25, 2.5, 2.0), (13.5, 3.75, 3.0), (4.5, 13.25, 2.5)]
    v, f = from_pixels(tri * 3, SQUARE_VIEW)
    return v, np.concatenate([f, f[:1]]), SQUARE_VIEW


SNAP_VIEW = (np.eye(4, dtype=np.float32), 256.0, 16.0, 0.0, 8.0, 16, 16)


def case_snap_limit():
    """Vertices with u = +-65536 (snapped to exactly +-2^24: kept) and one fp32 step beyond (skipped); z = 1."""
    far, step = 256.0, 2.0 ** -15                             # u = 256 x: 65536, and 65536 + 2^-7
    tris = []
    for x in (far, -far, far + step, -(far + step)):
        tris += [(x, 0.0, 1.0), (2.0 / 256, -0.4, 1.0), (3.0 / 256, 0.45, 1.0)]
    v = np.asarray(tris, np.float32)
    return v, np.arange(12, dtype=np.int32).reshape(4, 3), SNAP_VIEW


def case_large_boxes():
    """Face 0: a box of 32 x 32 = 1024 pixels; face 1: 41 x 25 = 1025; face 2 covers the whole 70 x 45 image."""
    v, f = from_pixels([(2, 2, 2.0), (33, 2, 2.0), (2, 33, 2.0), (20, 10, 1.0), (60, 10, 1.0), (20, 34, 1.0),
                        (-40, -30, 4.0), (200, -30, 4.0), (-40, 180, 4.0)], VIEW_70)
    return v, f, VIEW_70


def case_large33():
    """33 triangles of 40 x 30 pixel boxes at shifting places and depths."""
    tris = []
    for k in range(33):
        x, y, z = k % 11 * 2.5, k % 7 * 2.0, 1.0 + 0.125 * (k * 7 % 33)
        tris += [(x, y, z), (x + 39, y + 1, z + 0.5), (x + 2, y + 29, z + 0.25)]
    v, f = from_pixels(tris, VIEW_70)
    return v, f, VIEW_70


RENDER_CASES = {f.__name__[5:]: f for f in (
    case_square, case_slanted, case_box_inside, case_pillar_room, case_empty_faces, case_empty_all, case_odd,
    case_floaters_a, case_floaters_b, case_behind_and_nan, case_bad_index, case_zero_area, case_coplanar_duplicates,
    case_snap_limit, case_large_boxes, case_large33)}
# record = {bad, skipped, large at the default threshold, 0} where the case pins it
RECORDS = {"square": (0, 0, 0, 0), "slanted": (0, 0, 2, 0), "empty_faces": (0, 0, 0, 0), "empty_all": (0, 0, 0, 0),
           "behind_and_nan": (0, 3, 0, 0), "bad_index": (2, 0, 0, 0), "zero_area": (0, 0, 0, 0),
           "coplanar_duplicates": (0, 0, 0, 0), "snap_limit": (0, 2, 0, 0), "large_boxes": (0, 0, 2, 0),
           "large33": (0, 0, 33, 0)}


@functools.lru_cache(maxsize=None)
def render_case(name):
    """(verts, faces, view) of a case (computed once; callers must not write into it)."""
    return RENDER_CASES[name]()


@functools.lru_cache(maxsize=None)
def mirror_render(name, large_threshold=1024):
    """render_mesh_depth_numpy of a case (computed once and shared)."""
    from monogs_amd.mesh_render import render_mesh_depth_numpy
    v, f, (T, fx, fy, cx, cy, H, W) = render_case(name)
    return render_mesh_depth_numpy(v, f, T, fx, fy, cx, cy, H, W, large_threshold=large_threshold)


# ---- visibility and cull ---------------------------------------------------------------------------------------------
def pillar_vertex_sets():
    """Indices of the far wall's vertices (z = 2) behind the pillar and clear of it, inside the narrow view."""
    v, _, _ = render_case("pillar_room")
    far = (v[:, 2] == 2.0) & (np.abs(v[:, 1]) <= 0.75)
    hidden = np.flatnonzero(far & (np.abs(v[:, 0]) <= 0.5))
    clear = np.flatnonzero(far & (np.abs(v[:, 0]) >= 1.0) & (np.abs(v[:, 0]) <= 1.5))
    return hidden, clear


def seen_vectors(V, seed=0):
    """Random seen_count vectors for the cull: sparse, dense, all zero, all seen."""
    rng = np.random.default_rng(seed)
    return {"sparse": (rng.random(V) < 0.3).astype(np.int32) * rng.integers(1, 4, V).astype(np.int32),
            "dense": rng.integers(0, 3, V).astype(np.int32), "none": np.zeros(V, np.int32),
            "every": np.full(V, 2, np.int32)}


CULL_PARAMS = [(s, m, r) for s in ("sparse", "dense") for m in (1, 2) for r in ("all", "any")] + [
    ("none", 1, "any"), ("every", 2, "all")]


# ---- the two protocol scenes -----------------------------------------------------------------------------------------
SPHERE_THRESHOLD, SPHERE_SAMPLES = 0.2, 4000


def sphere_views(three=False):
    """Six cameras at distance 3 on the axes (or the three on the positive ones), looking at the origin; 64 x 64."""
    axes = [(3, 0, 0), (0, 3, 0), (0, 0, 3), (-3, 0, 0), (0, -3, 0), (0, 0, -3)]
    return [look(64, 64, 80.0, look_at(a)) for a in (axes[:3] if three else axes)]


@functools.lru_cache(maxsize=None)
def hidden_sphere():
    """(pred, gt, views): gt is the unit sphere, pred the same sphere plus a sphere of radius 0.5 hidden inside it."""
    gt = uv_sphere(1.0)
    return merge([gt, uv_sphere(0.5, n_lat=8, n_lon=16)]), gt, sphere_views()


@functools.lru_cache(maxsize=None)
def far_hemisphere():
    """(pred, gt, views): gt is the unit sphere, the views are the three cameras on one side, pred is what they see of
    it (the mirror's cull of gt itself)."""
    from monogs_amd.mesh_render import cull_by_visibility_numpy
    gt, views = uv_sphere(1.0), sphere_views(three=True)
    v, f, _, _ = cull_by_visibility_numpy(gt, views, occluder="self")
    return (v, f), gt, views
