"""CPU tests of the ray cast of the TSDF volumes: the mirror tsdf_raycast.raycast_torch against arithmetic written here,
the march's rules on hand-built planes, the refusals of the entry points (no GPU is touched), the brick and the dense
mirror paths against each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sparse_tsdf_cases as SC
import tsdf_raycast_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: a fronto-parallel plane: the mirror against arithmetic written here ------------------------------------------
def march64(t, w, origin, vs, pixels, z_near, dz, N):
    """The contract in fp64 NumPy for T = I: trilinear samples along z_n = z_near + n dz where all eight weights are >= 1,
    the first + -> - crossing between two valid samples, one linear interpolation.  Returns the depth per pixel (nan
    without a hit)."""
    t = np.asarray(t, np.float64)
    out = np.full(len(pixels), np.nan)
    for m, (x, y) in enumerate(pixels):
        xn, yn = (x - RC.CX) / RC.FX, (y - RC.CY) / RC.FY
        prev = None
        for n in range(N):
            z = z_near + n * dz
            l = (np.array([xn * z, yn * z, z]) - np.asarray(origin, np.float64)) / vs
            b = np.floor(l).astype(int)
            f = l - b
            if (b < 0).any() or (b[::-1] + 1 >= np.array(t.shape)).any() or \
                    not (w[b[2]:b[2] + 2, b[1]:b[1] + 2, b[0]:b[0] + 2] >= 1).all():
                prev = None
                continue
            c = t[b[2]:b[2] + 2, b[1]:b[1] + 2, b[0]:b[0] + 2]
            cx = c[:, :, 0] + f[0] * (c[:, :, 1] - c[:, :, 0])
            cy = cx[:, 0] + f[1] * (cx[:, 1] - cx[:, 0])
            v = cy[0] + f[2] * (cy[1] - cy[0])
            if prev is not None and prev > 0 and v <= 0:
                out[m] = (z - dz) + prev / (prev - v) * dz
                break
            prev = v
    return out


def test_plane_depth_and_normal_against_arithmetic():
    from monogs_amd.surface import depth_normal_torch
    from monogs_amd.tsdf_raycast import march_steps, raycast_torch
    t, w, c = RC.plane_volume()
    r = raycast_torch(t, w, c, RC.PLANE_ORIGIN, RC.PLANE_VS, (0, 0, 0), torch.eye(4), *RC.INTR, RC.H, RC.W, **RC.PLANE_KW)
    inner = (slice(8, RC.H - 8), slice(8, RC.W - 8))
    depth, normal = r["depth"][inner], r["normal"][inner]
    assert bool((r["hit_step"][inner] >= 0).all())
    err = float((depth - RC.PLANE_D0).abs().max())
    print(f"plane: max |depth - d0| over the central pixels = {err:.3e}")
    # the bound 1e-5 (about twenty fp32 roundings on quantities <= 1.2 give 1.5e-6) is confirmed in fp64 first: the band is
    # linear in z and trilinear interpolation of it is exact
    dz, N = march_steps(RC.PLANE_VS, RC.PLANE_KW["z_near"], RC.PLANE_KW["z_far"])
    pixels = [(x, y) for y in (8, 22, RC.H - 9) for x in (8, 35, RC.W - 9)]
    d64 = march64(t.numpy(), w.numpy(), RC.PLANE_ORIGIN, RC.PLANE_VS, pixels, RC.PLANE_KW["z_near"], dz, N)
    err64 = np.abs(d64 - RC.PLANE_D0).max()
    print(f"plane: fp64 evaluation, max |depth - d0| = {err64:.3e}")
    assert err64 <= 1e-5
    d32 = np.array([float(r["depth"][y, x]) for x, y in pixels])
    assert np.abs(d32 - d64).max() <= 1e-5
    assert err <= 1e-5
    # the normal is (0, 0, -1): towards the positive-TSDF side, which is the camera's
    sign = torch.sign(normal[..., 2])
    assert bool((sign == sign[0, 0]).all()) and float(sign[0, 0]) == -1.0
    want = torch.tensor([0.0, 0.0, float(sign[0, 0])])
    assert float((normal - want).abs().max()) <= 1e-4
    # ... and surface.depth_normal_torch of the ray cast's own depth plane has the same sign
    dn = depth_normal_torch(r["depth"], *RC.INTR, pixel_center=0.0).permute(1, 2, 0)[inner]
    assert float((dn[..., 2] * normal[..., 2]).min()) > 0.99
    # world frame at T = I is the same normal; the colour plane is zero (no image was fused) and finite
    rw = raycast_torch(t, w, c, RC.PLANE_ORIGIN, RC.PLANE_VS, (0, 0, 0), torch.eye(4), *RC.INTR, RC.H, RC.W, frame="world",
                       **RC.PLANE_KW)
    assert RC.same_planes(r, rw)


# ---- 2: refusals -----------------------------------------------------------------------------------------------------
def test_march_steps_and_its_refusals():
    from monogs_amd.tsdf_raycast import march_steps, raycast_torch
    dz, N = march_steps(0.05, 0.2, 2.0)
    assert dz == float(np.float32(0.5) * np.float32(0.05)) and N == int((float(np.float32(2.0)) - float(np.float32(0.2))) // dz) + 1
    assert march_steps(0.25, 0.25, 2.5, step=1.0) == (0.25, 10)
    assert march_steps(0.25, 0.25, 0.5, step=1.0) == (0.25, 2)
    for kw in (dict(z_far=None), dict(z_far=0.2), dict(z_far=0.1), dict(z_far=0.21),          # none, <= z_near, N < 2
               dict(z_far=2.0, step=0.0), dict(z_far=2.0, step=-1.0), dict(z_far=2.0, step=float("nan")),
               dict(z_far=1.0e6, step=1.0e-3),                                                 # N > 2^20
               dict(z_far=2.0, frame="object")):
        with pytest.raises(ValueError):
            march_steps(0.05, 0.2, **kw)
    assert march_steps(1.0, 0.0, float(2 ** 20 - 1), step=1.0)[1] == 2 ** 20
    with pytest.raises(ValueError):
        march_steps(1.0, 0.0, float(2 ** 20), step=1.0)
    with pytest.raises(ValueError):
        raycast_torch(None, None, None, (0, 0, 0), 0.05, (0, 0, 0), torch.eye(4), *RC.INTR, 4, 4, z_far=1.0)


NAMES = ("mgs_tsdf_raycast_args_size", "mgs_sparse_tsdf_raycast_args_size", "mgs_raycast_shade_args_size",
         "mgs_sparse_tsdf_raycast_scratch_bytes", "mgs_tsdf_raycast", "mgs_sparse_tsdf_raycast", "mgs_raycast_shade")


def _view(v, ptr):
    v.width, v.height, v.num_steps, v.frame, v.skip = 70, 45, 50, 0, 1
    v.fx, v.fy, v.cx, v.cy, v.z_near, v.dz, v.min_weight = 60.0, 60.0, 34.5, 22.0, 0.2, 0.025, 1.0
    v.T = v.depth = v.normal = v.color = v.hit_step = ptr


def test_entry_points_refuse_before_any_launch(built):
    """Pointers that are not null but point at host memory: a call that is refused never reads them, and a call that is
    not refused is not made here."""
    from monogs_amd import _cabi
    L = _cabi.lib()
    header = open(os.path.join(ROOT, "include", "monogs_raster.h"), encoding="utf-8").read()
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n) and re.search(r"\b%s\(" % n, header), n
    assert L.mgs_abi_version() == _cabi.ABI_VERSION
    assert L.mgs_tsdf_raycast_args_size() == C.sizeof(_cabi.TsdfRaycastArgs)
    assert L.mgs_sparse_tsdf_raycast_args_size() == C.sizeof(_cabi.SparseTsdfRaycastArgs)
    assert L.mgs_raycast_shade_args_size() == C.sizeof(_cabi.RaycastShadeArgs)
    cap = _cabi.SPARSE_TSDF_MAX_BRICKS
    assert [L.mgs_sparse_tsdf_raycast_scratch_bytes(n) for n in (0, 1, 400, cap, cap + 1)] == [0, 108, 43200, 108 * cap, 0]
    host = (C.c_float * 64)()
    ptr = C.addressof(host)
    BAD, UNSUPPORTED = -1, -3

    def dense(**kw):
        a = _cabi.TsdfRaycastArgs()
        a.nx = a.ny = a.nz = 8
        a.voxel_size = 0.05
        a.tsdf = a.weight = a.color = ptr
        _view(a.view, ptr)
        for k, v in kw.items():
            setattr(a.view if hasattr(a.view, k) and not hasattr(a, k) else a, k, v)
        return L.mgs_tsdf_raycast(C.byref(a), None)

    def sparse(**kw):
        a = _cabi.SparseTsdfRaycastArgs()
        a.vol.max_bricks, a.vol.voxel_size = 16, 0.05
        for n in ("tsdf", "weight", "color", "brick_coords", "map_keys", "map_vals", "state"):
            setattr(a.vol, n, ptr)
        a.scratch = ptr
        _view(a.view, ptr)
        for k, v in kw.items():
            where = a.vol if hasattr(a.vol, k) and k != "reserved0" else a.view if hasattr(a.view, k) else a
            setattr(where, k, v)
        return L.mgs_sparse_tsdf_raycast(C.byref(a), None)

    assert L.mgs_tsdf_raycast(None, None) == BAD and L.mgs_sparse_tsdf_raycast(None, None) == BAD
    assert L.mgs_raycast_shade(None, None) == BAD
    for call in (dense, sparse):
        for kw in (dict(tsdf=None), dict(weight=None), dict(T=None), dict(depth=None), dict(normal=None), dict(hit_step=None),
                   dict(num_steps=1), dict(num_steps=0), dict(dz=0.0), dict(dz=-0.025), dict(dz=float("nan")),
                   dict(fx=0.0), dict(fy=-1.0), dict(frame=2), dict(frame=-1), dict(skip=2), dict(width=0), dict(height=0),
                   dict(voxel_size=0.0)):
            assert call(**kw) == BAD, (call.__name__, kw)
        assert call(num_steps=2 ** 20 + 1) == UNSUPPORTED
        assert call(width=40000, height=40000) == UNSUPPORTED
    assert dense(nx=0) == BAD and dense(nx=2048, ny=2048, nz=2048) == UNSUPPORTED
    assert sparse(scratch=None) == BAD and sparse(state=None) == BAD and sparse(build_table=2) == BAD
    assert sparse(max_bricks=cap + 1) == UNSUPPORTED
    s = _cabi.RaycastShadeArgs()
    s.width, s.height, s.mode, s.fx, s.fy = 70, 45, 0, 60.0, 60.0
    s.hit_step = s.out = ptr
    assert L.mgs_raycast_shade(C.byref(s), None) == BAD                      # SHADED without a normal plane
    s.normal, s.mode = ptr, 4
    assert L.mgs_raycast_shade(C.byref(s), None) == BAD
    s.mode = 3
    assert L.mgs_raycast_shade(C.byref(s), None) == BAD                      # DEPTH without depth and lut
    s.mode, s.fx = 1, 0.0
    assert L.mgs_raycast_shade(C.byref(s), None) == BAD
    s.mode, s.out = 0, None
    assert L.mgs_raycast_shade(C.byref(s), None) == BAD


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fall_back():
    from monogs_amd.tsdf import TSDFVolume
    with pytest.raises(RuntimeError, match="GPU only"):
        TSDFVolume((0, 0, 0), 0.05, (8, 8, 8), device="cpu")


# ---- 3: the march's rules on hand-built planes -----------------------------------------------------------------------
# T = I, voxel 0.25, step 1, z_near 0.25: sample n lies exactly on layer k = n + 1 of a field that depends on k alone, so
# its value is the layer's (f_z = 0, and lerp(a, a, f) = a) and it needs the weights of the layers k and k + 1.
VS, ORIGIN, DIMS = 0.25, (-4.0, -3.0, 0.0), (32, 24, 12)
KW = dict(z_near=0.25, z_far=2.5, step=1.0)


def layered(values, weights=None):
    nx, ny, nz = DIMS
    t = torch.ones(nz, ny, nx) * torch.tensor(values, dtype=torch.float32)[:, None, None]
    w = torch.ones(nz, ny, nx) if weights is None else torch.ones(nz, ny, nx) * torch.tensor(weights, dtype=torch.float32)[:, None, None]
    g = torch.Generator().manual_seed(5)
    return t, w, torch.rand(3, nz, ny, nx, generator=g)


def cast(t, w, c, **kw):
    from monogs_amd.tsdf_raycast import raycast_torch
    return raycast_torch(t, w, c, ORIGIN, VS, (0, 0, 0), torch.eye(4), *RC.INTR, RC.H, RC.W, **{**KW, **kw})


def test_hit_back_face_and_running_out():
    P = 0.5
    r = cast(*layered([P] * 5 + [-P] * 7))                       # + up to layer 4, - from layer 5: hit at n = 4
    assert bool((r["hit_step"] == 4).all())
    assert torch.equal(r["depth"], torch.full((RC.H, RC.W), 1.125))            # z_3 + 0.5 dz
    assert float((r["normal"] - torch.tensor([0.0, 0.0, -1.0])).abs().max()) == 0.0
    assert float(r["color"].min()) > 0.0 and float(r["color"].max()) < 1.0
    r = cast(*layered([-P] * 5 + [P] * 7))                       # - then +: the ray starts inside and ends on a back face
    assert bool((r["hit_step"] == -2).all()) and not r["depth"].any() and not r["normal"].any() and not r["color"].any()
    r = cast(*layered([P] * 12))                                 # nothing crosses: the ray runs out
    assert bool((r["hit_step"] == -1).all()) and not r["depth"].any()
    r = cast(*layered([-P] * 3 + [P] * 3 + [-P] * 6))            # the back face comes first and ends the ray
    assert bool((r["hit_step"] == -2).all())


def test_zero_after_an_invalid_sample_and_nan():
    P = 0.5
    values = [P] * 5 + [0.0] + [-P] * 6                          # layer 5 is exactly 0
    r = cast(*layered(values))
    assert bool((r["hit_step"] == 4).all()) and torch.equal(r["depth"], torch.full((RC.H, RC.W), 1.25))      # t = 1
    weights = [1.0] * 4 + [0.0] + [1.0] * 7                      # layer 4 has no weight: samples k = 3 and k = 4 are invalid
    r = cast(*layered(values, weights))
    # k = 5 is valid with value 0 but has no valid predecessor; after it prev = 0 is not > 0: no hit, the ray runs out
    assert bool((r["hit_step"] == -1).all()) and not r["depth"].any()
    values = [P] * 5 + [float("nan")] + [-P] * 6                 # + , NaN, -: no comparison with a NaN holds
    r = cast(*layered(values))
    assert bool((r["hit_step"] == -1).all()) and not r["depth"].any()
    weights = [1.0] * 8 + [float("nan")] + [1.0] * 3             # a NaN weight is no weight: like 0 it only hides samples
    r = cast(*layered([P] * 5 + [-P] * 7, weights))
    assert bool((r["hit_step"] == 4).all())
    # the normal's samples reach one lattice unit each way, layers 3 .. 6; the march needed 4 .. 6 only: a NaN weight on
    # layer 3 leaves the hit and zeroes normal and colour
    weights = [1.0] * 3 + [float("nan")] + [1.0] * 8
    r = cast(*layered([P] * 5 + [-P] * 7, weights))
    assert bool((r["hit_step"] == 4).all()) and bool((r["depth"] > 0).all()) and not r["normal"].any() and not r["color"].any()


def _base_cells(z):
    """floor(l_x), floor(l_y) of every pixel at camera depth z, formed as the contract forms them (fp32, T = I)."""
    x, y = np.meshgrid(np.arange(RC.W, dtype=np.float32), np.arange(RC.H, dtype=np.float32))
    xn, yn = (x - np.float32(RC.CX)) / np.float32(RC.FX), (y - np.float32(RC.CY)) / np.float32(RC.FY)
    lx = (xn * np.float32(z) - np.float32(ORIGIN[0])) / np.float32(VS)
    ly = (yn * np.float32(z) - np.float32(ORIGIN[1])) / np.float32(VS)
    return np.floor(lx).astype(int), np.floor(ly).astype(int)


def test_one_light_corner_hides_the_cells_around_it():
    P = 0.5
    t, w, c = layered([P] * 5 + [-P] * 7)
    i, j = 17, 12
    w[5, j, i] = 0.5                                             # below min_weight 1: the samples k = 4 and k = 5 near it
    r = cast(t, w, c)
    touched = lambda z: (lambda bx, by: ((bx == i) | (bx == i - 1)) & ((by == j) | (by == j - 1)))(*_base_cells(z))
    t4, t5 = touched(1.0), touched(1.25)                         # n = 3 (k = 4) and n = 4 (k = 5)
    assert t4.sum() > 20 and t5.sum() > 20
    hs = r["hit_step"].numpy()
    assert (hs[~t4 & ~t5] == 4).all()
    assert (hs[t4 | t5] == -1).all()                             # n = 4 or its predecessor is invalid; nothing crosses later
    assert not r["depth"].numpy()[t4 | t5].any()
    r2 = cast(t, w, c, min_weight=0.5)                           # 0.5 >= 0.5: the corner counts again
    assert bool((r2["hit_step"] == 4).all())


def test_absent_neighbour_brick_and_the_brick_path():
    """Brick (0,0,0) .. of a 4 x 3 x 2 box with ONE brick missing: a base point in a present brick whose cell reaches
    into the absent one is invalid.  The brick mirror equals the dense mirror on the same planes, bit for bit."""
    from monogs_amd.tsdf_raycast import raycast_bricks_torch, raycast_torch
    P = 0.5
    t, w, c = layered([P] * 5 + [-P] * 7)
    nx, ny, nz = DIMS
    pad = lambda a, v: torch.nn.functional.pad(a, (0, 0, 0, 0, 0, 16 - nz), value=v)       # two bricks deep
    t, w, c = pad(t, 1.0), pad(w, 0.0), pad(c, 0.0)
    lo = (-16, -8, 0)                                            # the box's first point: bricks (-2..1, -1..1, 0..1)
    origin = tuple(ORIGIN[a] - lo[a] * VS for a in range(3))     # exact in fp32: the same lattice as ORIGIN at lo = 0
    gone = (0, 0, 0)                                             # lattice i in [0, 8), j in [0, 8), k in [0, 8)
    bricks = np.array([b for b in SC.box_bricks(lo, (nx, ny, 16)) if tuple(b) != gone])
    rows = SC.brick_rows((t.numpy(), w.numpy(), c.numpy()), lo, bricks)
    kw = dict(KW)
    rb = raycast_bricks_torch(bricks, *rows, origin, VS, torch.eye(4), *RC.INTR, RC.H, RC.W, **kw)
    wd = w.clone()
    wd[0:8, 8:16, 16:24] = 0.0                                   # the same volume as dense planes, in a LARGER box
    big = lambda a, v: torch.nn.functional.pad(a, (3, 5, 2, 1, 4, 0), value=v)
    rd = raycast_torch(big(t, 1.0), big(wd, 0.0), torch.stack([big(c[ch], 0.0) for ch in range(3)]), origin, VS,
                       (lo[0] - 3, lo[1] - 2, lo[2] - 4), torch.eye(4), *RC.INTR, RC.H, RC.W, **kw)
    assert RC.same_planes(rb, rd)
    # box index = lattice index - lo; the crossing samples are k = 4, 5 (inside the missing brick's k range)
    hs = rb["hit_step"].numpy()
    bx, by = _base_cells(1.0)
    bx5, by5 = _base_cells(1.25)
    inside = lambda bx, by: (bx - 16 >= -1) & (bx - 16 < 8) & (by - 8 >= -1) & (by - 8 < 8)      # the cell touches the brick
    hidden = inside(bx, by) | inside(bx5, by5)
    under = (bx - 16 == -1) & (by - 8 >= 0) & (by - 8 < 7) & (bx5 - 16 == -1)       # base brick (-1,0,0) present, +x neighbour absent
    assert under.sum() > 10 and hidden.sum() > under.sum()
    assert (hs[hidden] == -1).all() and (hs[~hidden] == 4).all()


def test_views_volume_mirror_is_a_surface():
    """The four-view volume from its first pose: most rays of the view hit, at the fused depth."""
    r = RC.views_mirror(0)
    depth, _, _ = SC.view_planes()
    hit = r["hit_step"] >= 0
    assert int(hit.sum()) > 0.6 * RC.H * RC.W
    err = (r["depth"] - depth)[hit & torch.isfinite(depth) & (depth > 0) & (depth < 2.5)].abs()
    assert float(err.median()) < 0.5 * SC.VS
    n = r["normal"][hit]
    length = n.norm(dim=-1)
    assert bool(((length - 1).abs() < 1e-5)[length > 0].all()) and bool((length > 0).any())
