"""Meshes shared by test_cpu_mesh_normals.py and test_gpu_mesh_normals.py.

Sizes.  Every kernel of the mesh normals works in blocks of 256 faces, vertices, samples or pixels; nothing scans, so
there is no trip boundary of their own.  mesh_eval_cases' two_trips (262 200 faces) is run for its size alone.
  soup(F)          F = 1, 63, 64, 65, 257: below, at and past a wave, and one past a block
  special          cancellation, an unreferenced vertex and a face at 2^-32 of the largest cross product, in one mesh
  star / strip     mesh_clean_cases': one accumulator in every face; 4099 vertices, one past 16 blocks"""
import functools

import numpy as np

import mesh_clean_cases as MC
import mesh_eval_cases as K
import mesh_render_cases as R

SOUP_SIZES = (1, 63, 64, 65, 257)
FACE_CASES = ("odd", "two_trips", "ratio", "degenerate", "bad_index", "zero_area", "no_faces")


@functools.lru_cache(maxsize=None)
def soup(F):
    return K._soup(F, 40 + F)


def axis_triangles():
    """Four right triangles in the coordinate planes, legs 1, 2 and 4 (powers of two: every step is exact):
    normals +z, -z, +x, +y."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [0, 2, 3], [0, 3, 1]], np.int32)
    n = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0]], np.float32)
    return v, f, n


def special():
    """(verts, faces, expected): vertices 0-2 carry two coincident faces of opposite winding (the sums cancel), vertex 3
    is named by no face, 4-6 a unit right triangle in z = 1 (cross product 1), 7-9 the same triangle scaled by 2^-16
    (cross product 2^-32 of the largest: its q is 0).  expected[v] is the normal, None where it is (0,0,0)."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    v = np.concatenate([tri + np.float32(5.0), [[9, 9, 9]], tri + np.array([0, 0, 1], np.float32),
                        tri * np.float32(2.0 ** -16)]).astype(np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [4, 5, 6], [7, 8, 9]], np.int32)
    expected = [None] * 4 + [(0.0, 0.0, 1.0)] * 3 + [None] * 3
    return v, f, expected


@functools.lru_cache(maxsize=None)
def sphere(n_lat=16, n_lon=32):
    return R.uv_sphere(1.0, n_lat=n_lat, n_lon=n_lon)


def vertex_cases():
    """name -> (verts, faces) of the vertex-normal comparisons that need no device to build."""
    sv, _, sf = MC.star(3000)
    tv, _, tf = MC.strip(4099)
    bv, bf = K.sampler_mesh("bad_index")
    nv, nf = K.sampler_mesh("no_faces")
    return {"star": (sv, sf), "strip": (tv, tf), "sphere": sphere(), "special": special()[:2], "bad_index": (bv, bf),
            "no_faces": (nv, nf), "degenerate": K.sampler_mesh("degenerate")}


def area_normals_float64(v, f):
    """The area-weighted vertex normals as a plain float64 sum: what the fixed point approximates."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    s = np.zeros_like(v)
    for k in range(3):
        np.add.at(s, f[:, k], c)
    return s / np.linalg.norm(s, axis=1, keepdims=True)


# ---- the three evaluation scenes -------------------------------------------------------------------------------------
EVAL_SAMPLES, EVAL_SEED = 4099, 3


def rotated_box():
    """The box [-1,1]^3 and itself turned by 45 degrees about z."""
    v, f = R.box((-1, -1, -1), (1, 1, 1), 4)
    c = s = np.sqrt(0.5)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return (v, f), ((v.astype(np.float64) @ rot.T).astype(np.float32), f)


def eval_scenes():
    """name -> (pred, gt): the sphere pair, the same with pred wound the other way, the box against itself rotated."""
    a, b = sphere(16, 32), sphere(32, 64)
    return {"spheres": (a, b), "flipped": ((a[0], np.ascontiguousarray(a[1][:, ::-1])), b), "box": rotated_box()}


@functools.lru_cache(maxsize=None)
def mirror_scores(name):
    """evaluate_mesh_numpy(normals=True, with_record=True) of a scene (computed once and shared)."""
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    pred, gt = eval_scenes()[name]
    return evaluate_mesh_numpy(pred, gt, n_samples=EVAL_SAMPLES, threshold=0.05, seed=EVAL_SEED, with_record=True,
                               normals=True)


# ---- frames ----------------------------------------------------------------------------------------------------------
FRAME_CASES = ("square", "slanted", "pillar_room", "odd", "bad_index", "zero_area", "empty_all", "large33")
BACKGROUND = (0.2, 0.4, 1.0)                # quantised: (51, 102, 255)


def frame_colors(V, u8=False):
    rng = np.random.default_rng(90 + V)
    return rng.integers(0, 256, (V, 3)).astype(np.uint8) if u8 else rng.random((V, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mirror_frame(name, mode, u8=False):
    """render_mesh_frame_numpy of a render case (computed once and shared)."""
    from monogs_amd.mesh_render import render_mesh_frame_numpy
    v, f, view = R.render_case(name)
    colors = frame_colors(v.shape[0], u8) if mode == "color" else None
    return render_mesh_frame_numpy(v, f, view, mode, colors=colors, background=BACKGROUND)
