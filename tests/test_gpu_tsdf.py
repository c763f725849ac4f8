"""Mesh export on the device against its mirrors (monogs_amd/tsdf.py): k_tsdf_integrate bit for bit against
integrate_torch, the extraction bit for bit (vertices, colours; faces as a set) against extract_mesh_numpy, and the path
from a map to a PLY file.

Sizes.  The integration works in bricks of 32 x 8 x 4 points, four x-consecutive points per thread, with 16-byte accesses
when nx is a multiple of 4 and the planes are 16-byte aligned: (21,18,13) is one brick wide, off every brick edge and on
the scalar path; (72,19,10) is three bricks along every axis and on the vector path, and - one float off alignment - on
the scalar path again.  The extraction classifies in the same 32 x 8 x 4 tiles and scans blocks of 256 points, 1024 block
totals per trip of the one-workgroup scan: (22,19,17) has 28 blocks, (70,45,40) has 493 (more than one per thread of the
scan), (70,45,90) has 1108 with the sphere across the boundary between the two trips."""
import math

import numpy as np
import pytest
import torch

import tsdf_cases as K

pytestmark = pytest.mark.gpu

H, W = 45, 70
FX, FY, CX, CY = 60.0, 60.0, 34.5, 22.0
GUARD = 4          # floats on either side of a plane; keeps a plane at offset 0 of the guard 16-byte aligned
SENTINEL = 12345.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def make_views(origin, vs, dims):
    """(T_w2c, weight) of the four views: rotated outside, inside, facing away, the first again (clamp live)."""
    from monogs_amd.pose import SE3_exp
    ext = [vs * (n - 1) for n in dims]
    centre = torch.tensor([origin[a] + 0.5 * ext[a] for a in range(3)])
    T0 = SE3_exp(torch.tensor([0.04, -0.03, 0.0, 0.08, -0.12, 0.05]))
    T0[:3, 3] = -T0[:3, :3] @ (centre - torch.tensor([0.1, -0.05, ext[2] * 0.5 + 1.2]))    # 1.2 in front of the volume
    T1 = SE3_exp(torch.tensor([0.0, 0.0, 0.0, -0.05, 0.07, 0.02]))
    T1[:3, 3] = -T1[:3, :3] @ centre                                                         # at the volume's centre
    T2 = torch.eye(4)
    T2[0, 0] = T2[2, 2] = -1.0
    T2[:3, 3] = -T2[:3, :3] @ (centre - torch.tensor([0.0, 0.0, 2.0]))                       # looks away from it
    return [(T0, 1.0), (T1, 1.0), (T2, 1.0), (T0, 1.5)]


def make_planes(ext_z):
    g = torch.Generator().manual_seed(3)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.2 + 0.5 * ext_z + 0.12 * torch.sin(u / 9.0) * torch.cos(v / 7.0)
    depth[3:6, 10:20] = 0.0
    depth[20:23, 30:40] = float("nan")
    depth[30:34, 5:15] = float("inf")
    depth[10:14, 50:60] = 3.0                       # over depth_max
    opacity = 0.93 + 0.07 * torch.rand(H, W, generator=g)
    opacity[40:43, 20:30] = 0.0
    opacity[25:27, 60:66] = float("nan")
    image = torch.rand(3, H, W, generator=g)
    return depth, opacity, image


@pytest.mark.parametrize("with_image", [False, True])
@pytest.mark.parametrize("with_opacity", [False, True])
@pytest.mark.parametrize("dims,vs,offset", [((21, 18, 13), 0.05, 0), ((72, 19, 10), 0.02, 0), ((72, 19, 10), 0.02, 1)])
def test_integration_equals_the_torch_mirror_bit_for_bit(built, dims, vs, offset, with_opacity, with_image):
    from monogs_amd.tsdf import TSDFVolume, integrate_torch
    dev = _dev()
    nx, ny, nz = dims
    n = nx * ny * nz
    origin = (-0.5 * vs * (nx - 1) + 0.013, -0.4 * vs * (ny - 1), 1.0)
    vol = TSDFVolume(origin, vs, dims, device=dev, max_weight=2.0)
    # the planes inside guarded buffers; `offset` floats take the 16-byte alignment away
    lead = GUARD + offset
    bufs = {}
    for name, planes, init in (("tsdf", 1, 1.0), ("weight", 1, 0.0), ("color", 3, 0.0)):
        buf = torch.full((lead + planes * n + GUARD,), SENTINEL, device=dev)
        buf[lead:lead + planes * n] = init
        bufs[name] = buf
        shape = (nz, ny, nx) if planes == 1 else (3, nz, ny, nx)
        setattr(vol, name, buf[lead:lead + planes * n].view(shape))
    assert (vol.tsdf.data_ptr() % 16 == 0) == (offset == 0)
    depth, opacity, image = make_planes(vs * (nz - 1))
    ref = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    kw = dict(depth_max=2.5, z_near=0.05)          # the camera inside the volume sees the points 5 cm in front of it
    if with_opacity:
        kw.update(opacity=opacity, normalize=True, min_opacity=0.95)
    if with_image:
        kw.update(image=image)
    d_in = depth * opacity if with_opacity else depth          # the forward's depth is the unnormalised blend
    updated = []
    for step, (T, w) in enumerate(make_views(origin, vs, dims)):
        before = [bits(t) for t in (vol.tsdf, vol.weight, vol.color)]
        vol.integrate(d_in.to(dev), T.to(dev), FX, FY, CX, CY, weight=w, **kw)
        integrate_torch(*ref, origin, vs, vol.trunc, d_in, T, FX, FY, CX, CY, view_weight=w, max_weight=2.0, **kw)
        torch.cuda.synchronize()
        after = [bits(t) for t in (vol.tsdf, vol.weight, vol.color)]
        for got, want, name in zip(after, ref, ("tsdf", "weight", "color")):
            assert torch.equal(got, bits(want)), (name, step, int((got != bits(want)).sum()))
        updated.append(int((after[1] != before[1]).sum() + (after[0] != before[0]).sum()))
        if step == 2:                                          # facing away: unchanged bit for bit
            assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert updated[0] > n // 20 and 0 < updated[1] < updated[0] and updated[2] == 0, updated
    assert float(ref[1].max()) == 2.0                          # 1 + 1.5 and 1 + 1 + 1.5 were clamped
    assert bool(torch.isfinite(vol.tsdf).all()) and float(vol.tsdf.min()) < 0.0 < float(vol.tsdf.max())
    if with_image:
        assert float(vol.color.max()) > 0.0
    else:
        assert float(vol.color.abs().max()) == 0.0
    for buf, planes in ((bufs["tsdf"], 1), (bufs["weight"], 1), (bufs["color"], 3)):
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + planes * n:] == SENTINEL).all())


# ---- extraction ------------------------------------------------------------------------------------------------------
BIG_C, BIG_R = (40.37, 25.61, 28.13), 9.3
TRIP_C, TRIP_R = (35.37, 22.61, 80.13), 8.3


def extraction_case(name):
    if name == "sphere":
        return (22, 19, 17), K.sphere_volume((22, 19, 17))
    if name == "half":
        return (22, 19, 17), K.sphere_volume((22, 19, 17), half=True)
    if name == "zero_plane":
        return (37, 9, 8), K.zero_plane_volume((37, 9, 8))
    if name == "all_positive":
        t, w, c = K.sphere_volume((22, 19, 17))
        return (22, 19, 17), (np.abs(t) + np.float32(0.25), w, c)
    if name == "blocks_493":
        return (70, 45, 40), K.sphere_volume((70, 45, 40), c=BIG_C, r=BIG_R)
    if name == "two_scan_trips":
        return (70, 45, 90), K.sphere_volume((70, 45, 90), c=TRIP_C, r=TRIP_R)
    raise KeyError(name)


def device_mesh(dims, planes, min_weight=1.0):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(K.ORIGIN, K.VOXEL, dims, device=_dev())
    for dst, src in zip((vol.tsdf, vol.weight, vol.color), planes):
        dst.copy_(torch.from_numpy(src))
    return vol, vol.extract_mesh(min_weight)


@pytest.mark.parametrize("name", ["sphere", "half", "zero_plane", "all_positive", "blocks_493", "two_scan_trips"])
def test_extraction_equals_the_numpy_mirror(built, name):
    from monogs_amd.tsdf import extract_mesh_numpy
    dims, planes = extraction_case(name)
    vol, (verts, faces, colors) = device_mesh(dims, planes)
    torch.cuda.synchronize()
    rv, rf, rc = extract_mesh_numpy(*planes, K.ORIGIN, K.VOXEL, 1.0)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert tuple(verts.shape) == rv.shape and tuple(faces.shape) == rf.shape and tuple(colors.shape) == rc.shape
    assert np.array_equal(bits(verts).numpy(), rv.view(np.int32))                # key order, bit for bit
    assert np.array_equal(bits(colors).numpy(), rc.view(np.int32))
    assert np.array_equal(K.canonical_faces(faces.cpu().numpy()), K.canonical_faces(rf))
    if name == "all_positive":
        assert verts.shape[0] == 0 and faces.shape[0] == 0
        return
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    if name == "sphere":
        K.assert_closed_sphere(v, f)
    elif name == "blocks_493":
        K.assert_closed_sphere(v, f, c=BIG_C, r=BIG_R)
        inside = np.flatnonzero(planes[0].reshape(-1) < 0)
        assert inside[0] // 256 < 256 < inside[-1] // 256                        # past one total per scan thread
    elif name == "two_scan_trips":
        K.assert_closed_sphere(v, f, c=TRIP_C, r=TRIP_R)
        inside = np.flatnonzero(planes[0].reshape(-1) < 0)
        assert inside[0] // 256 < 1024 < inside[-1] // 256                       # the surface spans both trips
    elif name == "half":
        K.assert_open_half(v, f)
    else:
        assert np.isfinite(v).all() and f.min() >= 0 and f.max() < len(v)
    # a second extraction gives the same bytes (the faces in the same order, too)
    v2, f2, c2 = vol.extract_mesh(1.0)
    assert torch.equal(bits(v2), bits(verts)) and torch.equal(f2, faces) and torch.equal(bits(c2), bits(colors))
    assert np.array_equal(f, rf)                                                 # cell, tetrahedron, triangle order


# ---- from a map to a file --------------------------------------------------------------------------------------------
def test_fuse_map_reconstruct_and_save(built, tmp_path):
    from scenes import wide_scene
    from monogs_amd import tsdf as T
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.ply_io import quantise_colors, read_mesh_ply
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera
    from monogs_amd.slam_surrogate import reconstruct_mesh
    dev = _dev()
    sc = wide_scene()
    cam = sc.cam
    gm = GaussianParams(*(t.to(dev) for t in (sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit, sc.features_dc)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    tau = torch.tensor([0.1, -0.05, 0.08, 0.03, -0.02, 0.01])
    cams = [ViewCamera(k, torch.zeros(3, cam.H, cam.W), SE3_exp(k * tau), cam.projmatrix_raw, fovx, fovy, cam.H, cam.W, dev)
            for k in range(3)]
    bg = torch.zeros(3, device=dev)
    vs = 0.125
    vol = T.fuse_map(gm, cams, bg, vs)
    # the mirror, fed the same rendered planes
    nx, ny, nz = vol.dims
    ref = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    for v in cams:
        with torch.no_grad():
            pkg = render(v, gm, Pipe, bg)
        T.integrate_torch(*ref, vol.origin, vs, vol.trunc, pkg["depth"].cpu(), v.T.cpu(), v.fx, v.fy, v.cx, v.cy,
                          image=pkg["render"].cpu(), opacity=pkg["opacity"].cpu(), min_opacity=0.95, normalize=True,
                          max_weight=vol.max_weight)
    for got, want, name in zip((vol.tsdf, vol.weight, vol.color), ref, ("tsdf", "weight", "color")):
        assert torch.equal(bits(got), bits(want)), name
    assert float(vol.weight.max()) >= 2.0
    verts, faces, colors = vol.extract_mesh()
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    rv, rf, rc = T.extract_mesh_numpy(*(t.numpy() for t in ref), vol.origin, vs, 1.0)
    assert np.array_equal(bits(verts).numpy(), rv.view(np.int32)) and np.array_equal(faces.cpu().numpy(), rf)
    # a run's result
    result = {"cameras": {k: v for k, v in enumerate(cams)}, "kf_ids": [0, 1, 2], "gaussians": gm}
    v2, f2, c2 = reconstruct_mesh(result, vs)
    assert torch.equal(bits(v2), bits(verts)) and torch.equal(f2, faces) and torch.equal(bits(c2), bits(colors))
    v3, f3, _ = reconstruct_mesh(result, vs, every_keyframe=2)
    assert v3.shape[0] > 0 and not (v3.shape == verts.shape and torch.equal(v3, verts))
    # measured depth instead of the rendered one: the same normalised depth as a "sensor" plane, holes as 0, gives
    # the same geometry (the colour is then the keyframe's image: zeros here)
    sensor = {}
    for k, v in enumerate(cams):
        with torch.no_grad():
            pkg = render(v, gm, Pipe, bg)
        sensor[k] = torch.where(pkg["opacity"] >= 0.95, pkg["depth"] / pkg["opacity"], torch.zeros_like(pkg["depth"]))[0]
    v4, f4, c4 = reconstruct_mesh(result, vs, sensor_depth=sensor)
    assert torch.equal(bits(v4), bits(verts)) and torch.equal(f4, faces) and float(c4.abs().max()) == 0.0
    # the file, next to the point cloud
    path = save_mesh(vol, str(tmp_path))
    assert path == str(tmp_path / "point_cloud" / "final" / "mesh.ply")
    pv, pf, pc = read_mesh_ply(path)
    assert torch.equal(bits(pv), bits(verts)) and torch.equal(pf, faces.cpu())
    assert np.array_equal(pc.numpy(), quantise_colors(colors))
    path2 = save_mesh(gm, str(tmp_path / "b"), cameras=cams, voxel_size=vs)
    assert open(path2, "rb").read() == open(path, "rb").read()
