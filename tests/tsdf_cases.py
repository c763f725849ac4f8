"""Analytic volumes and mesh checks shared by test_cpu_tsdf.py and test_gpu_tsdf.py."""
import numpy as np

SPHERE_C, SPHERE_R = (9.37, 9.61, 9.13), 6.3          # lattice units
ORIGIN, VOXEL = (-0.31, 0.17, 0.9), 0.05


def lattice_index(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i, j, k


def sphere_volume(dims, c=SPHERE_C, r=SPHERE_R, half=False, seed=0):
    """(tsdf, weight, color) [nz,ny,nx]: clip((|p - c| - r) / 3, -1, 1) in lattice units, weights 1 (0 on the half
    i < 10 with `half`), a smooth random colour."""
    i, j, k = lattice_index(dims)
    d = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2)
    tsdf = np.clip((d - r) / 3.0, -1.0, 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    if half:
        weight[:, :, :10] = 0.0
    rng = np.random.default_rng(seed)
    color = rng.random((3,) + tsdf.shape).astype(np.float32)
    return tsdf, weight, color


def zero_plane_volume(dims):
    """tsdf exactly 0 on the lattice plane i = 5."""
    i, _, _ = lattice_index(dims)
    tsdf = ((i - 5).astype(np.float32) / np.float32(3.0)).astype(np.float32)
    rng = np.random.default_rng(1)
    return tsdf, np.ones_like(tsdf), rng.random((3,) + tsdf.shape).astype(np.float32)


def edge_counts(faces, num_verts):
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = np.unique(de[:, 0] * num_verts + de[:, 1], return_counts=True)[1]
    ue = np.sort(de, axis=1)
    undirected = np.unique(ue[:, 0] * num_verts + ue[:, 1], return_counts=True)[1]
    return directed, undirected


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def assert_closed_sphere(verts, faces, origin=ORIGIN, voxel=VOXEL, c=SPHERE_C, r=SPHERE_R):
    """The sphere's mesh is a closed, consistently wound 2-manifold of genus 0 that hugs the sphere."""
    V, F = len(verts), len(faces)
    assert V > 0 and F > 0
    directed, undirected = edge_counts(faces, V)
    assert set(undirected.tolist()) == {2}          # every undirected edge in exactly two faces
    assert set(directed.tolist()) == {1}            # every directed edge in exactly one face
    assert V - len(undirected) + F == 2
    assert len(np.unique(np.asarray(faces))) == V   # no unreferenced vertex
    assert face_areas(verts, faces).min() > 0.0
    assert signed_volume(verts, faces) > 0.0
    lat = (np.asarray(verts, np.float64) - np.asarray(origin, np.float64)) / voxel
    dist = np.abs(np.linalg.norm(lat - np.asarray(c), axis=1) - r)
    # linear interpolation along an edge of length L <= sqrt(3): at most L^2 / (8 r) = 0.06 voxel off the sphere
    assert dist.max() <= 0.1, dist.max()


def assert_open_half(verts, faces):
    V = len(verts)
    directed, undirected = edge_counts(faces, V)
    assert set(undirected.tolist()) == {1, 2}
    assert set(directed.tolist()) == {1}
    assert len(np.unique(np.asarray(faces))) == V


def canonical_faces(faces):
    """Each triple rotated to start at its smallest index, rows sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    s = np.argmin(f, axis=1)
    rows = np.arange(f.shape[0])
    g = np.stack([f[rows, s], f[rows, (s + 1) % 3], f[rows, (s + 2) % 3]], 1)
    return g[np.lexsort((g[:, 2], g[:, 1], g[:, 0]))]
