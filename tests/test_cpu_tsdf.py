"""Mesh export without a GPU: the mirrors that define the contract (monogs_amd/tsdf.py), the mesh PLY, and the C-ABI
boundary of the new entry points.

Plane tolerance: with an identity pose and a constant depth the projective sdf is linear in z, so the interpolated
vertex is exact up to fewer than 20 fp32 roundings of values of size O(1): 20 * 2^-24 * 2 = 2.4e-6; the bound is
1e-5."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tsdf_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tet_table_is_the_one_in_the_kernel_source():
    from monogs_amd import tsdf as T
    src = open(os.path.join(ROOT, "monogs_amd", "csrc", "tsdf.hip")).read()
    block = src[src.index("TET_TABLE_BEGIN"):src.index("TET_TABLE_END")]
    ntri = [int(v) for v in re.search(r"c_tet_ntri\[16\] = \{([^}]*)\}", block).group(1).split(",")]
    body = block[block.index("c_tet_tri[16][6]"):]
    rows = [[int(v) for v in m.split(",")] for m in re.findall(r"\{([0-9, ]+)\}", body)]
    assert len(rows) == 16 and ntri == [len(t) for t in T.TET_TABLE]
    for case, tris in enumerate(T.TET_TABLE):
        flat = [e for tri in tris for e in tri]
        assert rows[case][:len(flat)] == flat, case
    # the kernel's corner codes, orientation flags and slot order
    assert T.TET_CORNERS == ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
    assert T.TET_FLIP == (False, True, True, False, False, True)
    assert T.SLOT_CODES == (1, 2, 4, 3, 5, 6, 7)


def test_sphere_mesh_is_a_closed_manifold():
    from monogs_amd.tsdf import extract_mesh_numpy
    tsdf, weight, color = K.sphere_volume((20, 20, 20))
    verts, faces, colors = extract_mesh_numpy(tsdf, weight, color, K.ORIGIN, K.VOXEL, 1.0)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and colors.shape == verts.shape
    K.assert_closed_sphere(verts, faces)
    assert colors.min() >= 0.0 and colors.max() <= 1.0
    # lattice units, zero origin: the same topology
    v1, f1, _ = extract_mesh_numpy(tsdf, weight, None, (0, 0, 0), 1.0, 1.0)
    K.assert_closed_sphere(v1, f1, origin=(0, 0, 0), voxel=1.0)
    assert np.array_equal(f1, faces)


def test_half_weight_sphere_is_open_and_has_no_stray_vertex():
    from monogs_amd.tsdf import extract_mesh_numpy
    tsdf, weight, color = K.sphere_volume((20, 20, 20), half=True)
    verts, faces, _ = extract_mesh_numpy(tsdf, weight, color, K.ORIGIN, K.VOXEL, 1.0)
    K.assert_open_half(verts, faces)
    lat_x = (verts[:, 0] - K.ORIGIN[0]) / K.VOXEL
    assert lat_x.min() >= 10.0 - 1e-4       # nothing in the half without weight


def test_fronto_parallel_plane():
    from monogs_amd.tsdf import extract_mesh_numpy, integrate_torch
    nx, ny, nz = 21, 16, 21
    origin, vs = (-0.2, -0.15, 1.3), 0.02
    tsdf, weight = torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx)
    color = torch.zeros(3, nz, ny, nx)
    depth = torch.full((45, 70), 1.5)
    image = torch.rand(3, 45, 70, generator=torch.Generator().manual_seed(0))
    integrate_torch(tsdf, weight, color, origin, vs, 4 * vs, depth, torch.eye(4), 60.0, 60.0, 34.5, 22.0, image=image)
    assert float(weight.max()) == 1.0 and float(weight.min()) == 0.0      # behind the truncation band: untouched
    assert bool((tsdf[weight == 0] == 1.0).all())
    verts, faces, colors = extract_mesh_numpy(tsdf.numpy(), weight.numpy(), color.numpy(), origin, vs, 1.0)
    assert len(verts) > 100 and len(faces) > 100
    assert np.abs(verts[:, 2].astype(np.float64) - 1.5).max() <= 1e-5
    assert len(np.unique(faces)) == len(verts)
    assert colors.min() >= 0.0 and colors.max() <= 1.0


def test_integrate_torch_skips_what_the_contract_skips():
    from monogs_amd.tsdf import integrate_torch
    nx, ny, nz = 9, 8, 7
    mk = lambda: (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    depth = torch.full((45, 70), 1.5)
    args = ((-0.1, -0.1, 1.4), 0.02, 0.08, depth)
    away = torch.eye(4)
    away[0, 0] = away[2, 2] = -1.0                     # looking down -z: every zc is negative
    t, w, c = mk()
    integrate_torch(t, w, c, *args, away, 60.0, 60.0, 34.5, 22.0)
    assert bool((w == 0).all()) and bool((t == 1).all())
    bad = depth.clone()
    bad[:, :] = float("nan")
    integrate_torch(t, w, c, *args[:3], bad, torch.eye(4), 60.0, 60.0, 34.5, 22.0)
    assert bool((w == 0).all())
    integrate_torch(t, w, c, *args, torch.eye(4), 60.0, 60.0, 34.5, 22.0, depth_max=1.4)
    assert bool((w == 0).all())
    integrate_torch(t, w, c, *args, torch.eye(4), 60.0, 60.0, 34.5, 22.0, opacity=torch.full((45, 70), 0.5))
    assert bool((w == 0).all())
    for _ in range(3):                                 # the clamp of the stored weight
        integrate_torch(t, w, c, *args, torch.eye(4), 60.0, 60.0, 34.5, 22.0, max_weight=2.0)
    assert float(w.max()) == 2.0


def test_exact_zero_plane_extracts_without_nan():
    from monogs_amd.tsdf import extract_mesh_numpy
    tsdf, weight, color = K.zero_plane_volume((11, 9, 8))
    assert (tsdf[:, :, 5] == 0).all()
    verts, faces, colors = extract_mesh_numpy(tsdf, weight, color, K.ORIGIN, K.VOXEL, 1.0)
    assert len(verts) > 0 and len(faces) > 0
    assert np.isfinite(verts).all() and np.isfinite(colors).all()
    assert faces.min() >= 0 and faces.max() < len(verts)
    # zero counts as outside: every vertex sits on the plane i = 5 itself
    assert np.abs((verts[:, 0] - K.ORIGIN[0]) / K.VOXEL - 5.0).max() < 1e-4


def test_all_positive_volume_gives_an_empty_mesh():
    from monogs_amd.tsdf import extract_mesh_numpy
    verts, faces, colors = extract_mesh_numpy(np.ones((5, 6, 7), np.float32), np.ones((5, 6, 7), np.float32), None,
                                              (0, 0, 0), 1.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)


def test_mesh_ply_round_trip_and_header(tmp_path):
    from monogs_amd.ply_io import mesh_ply_header, quantise_colors, read_mesh_ply, write_mesh_ply
    from monogs_amd.tsdf import extract_mesh_numpy
    tsdf, weight, color = K.sphere_volume((20, 20, 20))
    verts, faces, colors = extract_mesh_numpy(tsdf, weight, color, K.ORIGIN, K.VOXEL, 1.0)
    path = str(tmp_path / "sub" / "mesh.ply")
    write_mesh_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(colors))
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(verts)}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(faces)}\n"
              "property list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header.encode("ascii")) and header == mesh_ply_header(len(verts), len(faces))
    assert len(raw) == len(header) + 15 * len(verts) + 13 * len(faces)
    v, f, c = read_mesh_ply(path)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and c.dtype == torch.uint8
    assert np.array_equal(v.numpy().view(np.uint32), verts.view(np.uint32)) and np.array_equal(f.numpy(), faces)
    assert np.array_equal(c.numpy(), quantise_colors(colors))
    assert np.abs(c.numpy().astype(np.float64) / 255.0 - colors).max() <= 0.5 / 255.0 + 1e-7
    # empty mesh, default colour, rejected input
    write_mesh_ply(path, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    v0, f0, c0 = read_mesh_ply(path)
    assert v0.shape == (0, 3) and f0.shape == (0, 3) and c0.shape == (0, 3)
    with pytest.raises(ValueError):
        write_mesh_ply(path, torch.zeros(2, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    with pytest.raises(ValueError):
        read_mesh_ply(os.path.join(ROOT, "README.md"))


def test_exports_struct_sizes_and_abi_version(built):
    from monogs_amd import _cabi
    names = ("mgs_tsdf_integrate_args_size", "mgs_tsdf_integrate", "mgs_tsdf_mesh_args_size",
             "mgs_tsdf_mesh_scratch_bytes", "mgs_tsdf_mesh_count", "mgs_tsdf_mesh_emit")
    for n in names:
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_tsdf_integrate_args_size() == C.sizeof(_cabi.TsdfIntegrateArgs) == 22 * 4 + 7 * 8
    assert L.mgs_tsdf_mesh_args_size() == C.sizeof(_cabi.TsdfMeshArgs) == 10 * 4 + 8 * 8 + 2 * 4
    assert _cabi.ABI_VERSION == 10 and L.mgs_abi_version() == 10
    assert L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1          # the list ends where it ended


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_tsdf_integrate(None, None) == -1
    assert L.mgs_tsdf_mesh_count(None, None) == -1 and L.mgs_tsdf_mesh_emit(None, None) == -1
    a = _cabi.TsdfIntegrateArgs()
    a.nx, a.ny, a.nz, a.width, a.height = 8, 8, 8, 16, 16
    a.voxel_size, a.trunc, a.fx, a.fy, a.weight, a.max_weight = 0.1, 0.4, 10.0, 10.0, 1.0, 64.0
    assert L.mgs_tsdf_integrate(C.byref(a), None) == -1                   # null planes
    a.T = a.depth = a.tsdf = a.wsum = 4096
    a.image = 4096                                                        # an image without colour planes
    assert L.mgs_tsdf_integrate(C.byref(a), None) == -1
    a.image = None
    a.voxel_size = 0.0
    assert L.mgs_tsdf_integrate(C.byref(a), None) == -1
    a.voxel_size = 0.1
    a.nx, a.ny, a.nz = 675, 675, 675                                      # 7 * 675^3 >= 2^31
    assert L.mgs_tsdf_integrate(C.byref(a), None) == -3
    m = _cabi.TsdfMeshArgs()
    m.nx, m.ny, m.nz, m.voxel_size = 8, 8, 8, 0.1
    assert L.mgs_tsdf_mesh_count(C.byref(m), None) == -1
    m.tsdf = m.weight = m.scratch = 4096
    assert L.mgs_tsdf_mesh_count(C.byref(m), None) == -1                  # no counts
    m.num_verts = -1
    assert L.mgs_tsdf_mesh_emit(C.byref(m), None) == -1
    m.num_verts, m.num_faces = 3, 1
    assert L.mgs_tsdf_mesh_emit(C.byref(m), None) == -1                   # counts without outputs
    m.num_verts, m.num_faces = 0, 0
    assert L.mgs_tsdf_mesh_emit(C.byref(m), None) == 0                    # nothing to write: no launch
    m.nx, m.ny, m.nz = 675, 675, 675
    m.counts = 4096
    assert L.mgs_tsdf_mesh_count(C.byref(m), None) == -3 and L.mgs_tsdf_mesh_emit(C.byref(m), None) == -3
    assert L.mgs_tsdf_mesh_scratch_bytes(675, 675, 675) == 0 and L.mgs_tsdf_mesh_scratch_bytes(0, 4, 4) == 0
    assert 7 * 674 ** 3 < 2 ** 31 <= 7 * 675 ** 3
    assert L.mgs_tsdf_mesh_scratch_bytes(674, 674, 674) > 6 * 674 ** 3
    n, blocks = 21 * 18 * 13, (21 * 18 * 13 + 255) // 256
    pad = lambda b: (b + 255) // 256 * 256
    assert L.mgs_tsdf_mesh_scratch_bytes(21, 18, 13) == 3 * pad(2 * n) + pad(8 * blocks)


def test_over_large_dims_raise_value_error():
    from monogs_amd.tsdf import TSDFVolume, check_dims
    assert check_dims((674, 674, 674)) == (674, 674, 674)
    with pytest.raises(ValueError):
        check_dims((675, 675, 675))
    with pytest.raises(ValueError):
        TSDFVolume((0, 0, 0), 0.01, (675, 675, 675), device="cpu")
    with pytest.raises(ValueError):
        TSDFVolume((0, 0, 0), 0.01, (0, 4, 4), device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        TSDFVolume((0, 0, 0), 0.01, (4, 4, 4), device="cpu")
