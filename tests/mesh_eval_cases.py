"""Meshes and point sets shared by test_cpu_mesh_eval.py and test_gpu_mesh_eval.py.

Sizes.  The sampler works in blocks of 256 faces / samples and its one-workgroup scan takes 1024 block totals per trip
(262 144 faces); the nearest-distance grid has at most 2^21 cells, at most 1024 per axis, scanned in blocks of 256 cells
with 1024 block totals per trip (262 144 cells).
  sampler  odd (F = 1003, n = 1001), two_trips (F = 262 200: 1025 block totals, the faces past the trip boundary carry
           about a third of the area), ratio (areas 2^32 : 2^16 : 1 - the unit faces get weight 0), degenerate (zero-area,
           NaN and infinite faces in the middle), bad_index, zero_area (T = 0), no_faces (F = 0), and n = 0
  nearest  one case per line of NEAREST_CASES' docstrings"""
import functools

import numpy as np

# ---- sampler ---------------------------------------------------------------------------------------------------------


def _soup(F, seed, scale=1.0):
    """F separate random triangles: (verts [3F,3], faces [F,3])."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4.0, 4.0, (F, 1, 3))
    v = (centre + scale * rng.standard_normal((F, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def mesh_odd():
    v, f = _soup(1003, 1)
    f = f.copy()
    f[5:900:7, 1] = f[4:899:7, 2]            # shared vertices: an indexed mesh, not only a soup
    return v, f


def mesh_two_trips():
    F = 262200
    v, f = _soup(F, 2, 0.1)
    v = v.reshape(F, 3, 3)
    c = v[262144:].mean(axis=1, keepdims=True)
    v[262144:] = c + (v[262144:] - c) * np.float32(48.0)       # 56 faces of 2304 times the area
    return v.reshape(-1, 3), f


def _right_triangle(first, leg, at):
    v = np.array([[0, 0, 0], [leg, 0, 0], [0, leg, 0]], np.float32) + np.asarray(at, np.float32)
    return v, np.array([[first, first + 1, first + 2]], np.int32)


def mesh_ratio():
    """One face with |n| = 2^32, 40 with 2^16, 300 with 1: the last get q = trunc(2^-2) = 0."""
    legs = [65536.0] + [256.0] * 40 + [1.0] * 300
    order = np.random.default_rng(3).permutation(len(legs))
    vs, fs = [], []
    for k, i in enumerate(order):
        v, f = _right_triangle(3 * k, legs[i], (7.0 * k, 3.0, -2.0))
        vs.append(v), fs.append(f)
    return np.concatenate(vs), np.concatenate(fs), np.asarray(legs)[order]


def mesh_degenerate():
    v, f = _soup(700, 4)
    f = f.copy()
    f[100:140, 2] = f[100:140, 1]            # (a, b, b): no area
    v[3 * 200:3 * 200 + 3] = v[3 * 200]      # three equal points
    v[3 * 300 + 1] = np.nan                  # a NaN area
    v[3 * 301 + 2, 0] = np.inf               # a non-finite area
    v[3 * 302] = 3e30                        # the area overflows to infinity
    return v, f


def mesh_bad_index():
    v, f = _soup(300, 5)
    f = f.copy()
    f[17, 1] = v.shape[0]
    f[250, 0] = -1
    return v, f


def mesh_zero_area():
    v, f = _soup(50, 6)
    f = f.copy()
    f[:, 2] = f[:, 0]
    return v, f


def mesh_no_faces():
    return np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32)


def two_triangles_3_to_1():
    """Areas 3 : 1 exactly (|n| = 6 and 2)."""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [10, 0, 0], [11, 0, 0], [10, 2, 0]], np.float32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)


SAMPLER_MESHES = {"odd": mesh_odd, "two_trips": mesh_two_trips, "ratio": lambda: mesh_ratio()[:2],
                  "degenerate": mesh_degenerate, "bad_index": mesh_bad_index, "zero_area": mesh_zero_area,
                  "no_faces": mesh_no_faces}
# (mesh, n, seed)
SAMPLER_PARAMS = (("odd", 1001, 0), ("odd", 256, 2 ** 40 + 17), ("two_trips", 4099, 1), ("ratio", 3000, 2),
                  ("degenerate", 2049, 3), ("bad_index", 777, 4), ("zero_area", 300, 5), ("no_faces", 65, 6),
                  ("odd", 0, 7), ("no_faces", 0, 8))


@functools.lru_cache(maxsize=None)
def sampler_mesh(name):
    return SAMPLER_MESHES[name]()


def replay_words(n, seed):
    """[n,4] int64 holding u32 words, a few of them at the extremes of the fold and of the modulus."""
    w = np.random.default_rng(1000 + seed).integers(0, 2 ** 32, (n, 4), dtype=np.int64)
    if n >= 6:
        w[0] = (0, 0, 0, 0)
        w[1] = (2 ** 32 - 1,) * 4
        w[2, 2:] = (2 ** 31, 2 ** 31)              # k1 + k2 = 2^24 exactly: not folded
        w[3, 2:] = (2 ** 31 + 256, 2 ** 31)        # one past: folded
        w[4, 2:] = (2 ** 32 - 1, 0)
        w[5, 2:] = (0, 2 ** 32 - 1)
    return w


# ---- nearest distance ------------------------------------------------------------------------------------------------
def _cube(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def nn_odd_sizes():
    """P, Q no multiples of 256."""
    return _cube(1001, 10), _cube(777, 11), None


def nn_single_ref():
    """Q = 1."""
    return _cube(300, 12), _cube(1, 13), None


def nn_no_ref():
    """Q = 0."""
    return _cube(70, 14), np.zeros((0, 3), np.float32), None


def nn_no_query():
    """P = 0."""
    return np.zeros((0, 3), np.float32), _cube(500, 15), None


def nn_coincident():
    """All reference points coincident: a box of zero extent."""
    return _cube(257, 16), np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (300, 1)), None


def nn_plane():
    """Points on a plane: a box thin (zero) in one axis."""
    r = _cube(1500, 17)
    r[:, 2] = 0.375
    return _cube(700, 18), r, None


def nn_line():
    """Points on a line: a 1-D grid."""
    r = np.zeros((900, 3), np.float32)
    r[:, 1] = np.random.default_rng(19).uniform(-3, 3, 900).astype(np.float32)
    return _cube(400, 20, -3, 3), r, None


def nn_outlier():
    """One far outlier stretches the box: nearly all points share a cell."""
    r = _cube(2000, 21)
    r[1234] = (1.0e4, -2.0e4, 3.0e4)
    q = _cube(600, 22)
    q[::50] = r[1234] + _cube(12, 23)
    return q, r, None


def nn_lattice_ties():
    """An integer lattice, queries at the cell centres: eight-way ties, the smallest index wins."""
    g = np.arange(8, dtype=np.float32)
    r = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    r = r[np.random.default_rng(24).permutation(len(r))]
    c = np.arange(7, dtype=np.float32) + np.float32(0.5)
    q = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return q, r, None


def nn_duplicates():
    """Every reference point three times."""
    r = np.repeat(_cube(400, 25), 3, axis=0)
    r = r[np.random.default_rng(26).permutation(len(r))]
    return np.concatenate([_cube(500, 27), r[::7]]), r, None


def nn_outside():
    """Queries ten box extents outside on each side, and at the corners."""
    r = _cube(3000, 28)
    offs = np.array([[sx, sy, sz] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)], np.float32)
    q = np.concatenate([_cube(20, 29 + k) + 20.0 * o for k, o in enumerate(offs)]).astype(np.float32)
    return q, r, None


def nn_empty_region():
    """Two clusters in opposite corners of the box, queries in the empty middle."""
    r = np.concatenate([_cube(1500, 60, -1.0, -0.8), _cube(1500, 61, 0.8, 1.0)])
    return _cube(500, 62, -0.5, 0.5), r, None


def nn_cell_cap():
    """cell_size so small that the cell cap engages."""
    return _cube(800, 63), _cube(2500, 64), 1e-6


def nn_one_cell():
    """cell_size so large that there is one cell."""
    return _cube(300, 65), _cube(900, 66), 1.0e6


def nn_scan_trips():
    """81^3 = 531 441 cells for 4000 points: three trips of the scan of cell blocks."""
    return _cube(1000, 67), _cube(4000, 68), 2.0 / 80.0


def nn_non_finite():
    """NaN / inf rows on both sides."""
    q, r = _cube(600, 69), _cube(900, 70)
    r[3] = np.nan
    r[100, 1] = np.inf
    r[101, 2] = -np.inf
    r[899] = np.nan
    q[0, 0] = np.nan
    q[77] = np.inf
    q[599, 2] = -np.inf
    return q, r, None


def nn_all_non_finite():
    """No finite reference point at all."""
    return _cube(100, 71), np.full((40, 3), np.nan, np.float32), None


def nn_surface():
    """Samples of two spheres against each other: what evaluate_mesh asks."""
    rng = np.random.default_rng(72)
    a = rng.standard_normal((5000, 3))
    b = rng.standard_normal((4099, 3))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    b = (1.02 * b / np.linalg.norm(b, axis=1, keepdims=True) + 0.01).astype(np.float32)
    return a, b, None


NEAREST_CASES = {f.__name__[3:]: f for f in (
    nn_odd_sizes, nn_single_ref, nn_no_ref, nn_no_query, nn_coincident, nn_plane, nn_line, nn_outlier, nn_lattice_ties,
    nn_duplicates, nn_outside, nn_empty_region, nn_cell_cap, nn_one_cell, nn_scan_trips, nn_non_finite,
    nn_all_non_finite, nn_surface)}


@functools.lru_cache(maxsize=None)
def nearest_case(name):
    return NEAREST_CASES[name]()


# ---- analytic scenes -------------------------------------------------------------------------------------------------
def square(z, n=1):
    """The unit square at height z as 2 n^2 triangles."""
    g = np.linspace(0.0, 1.0, n + 1, dtype=np.float32)
    v = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((n + 1, n + 1), z, np.float32)], -1).reshape(-1, 3)
    i, j = (t.reshape(-1) for t in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    return v.astype(np.float32), np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def square_lattice(z, pitch):
    """The lattice of pitch `pitch` on the unit square at height z, borders included."""
    g = np.arange(0.0, 1.0 + 0.5 * pitch, pitch)
    x, y = (t.reshape(-1) for t in np.meshgrid(g, g, indexing="ij"))
    return np.stack([x, y, np.full_like(x, z)], 1).astype(np.float32)


def two_layer_truth(cam):
    """The two true layers of surface_cases.two_layer_scene as a mesh: the front layer where its splats are (u < W / 2,
    one splat radius more), the back layer everywhere; both wider than the fused volume."""
    import surface_cases as SC
    xe = (0.5 * cam.W + 2.0 - cam.cx) / cam.fx * SC.Z_FRONT
    quads = [((-0.6, xe), SC.Z_FRONT), ((-1.2, 1.2), SC.Z_BACK)]
    vs, fs = [], []
    for k, ((x0, x1), z) in enumerate(quads):
        vs.append(np.array([[x0, -0.6, z], [x1, -0.6, z], [x1, 0.6, z], [x0, 0.6, z]], np.float32))
        fs.append(np.array([[0, 1, 2], [0, 2, 3]], np.int32) + 4 * k)
    return np.concatenate(vs), np.concatenate(fs)
