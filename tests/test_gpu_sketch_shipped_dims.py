"""The sketched second-order path at the shipped sketch dimensions, stack_dim 16 x sketch_dim 64 = 1024 buckets, COMPARED
with a reference (not merely run), each case on the smallest image that crosses one of the path's multi-trip thresholds:

  k_sketch_bucket        zero / flush loops of the LDS bucket table: 16 * 64 * 6 = 6144 floats, 6 trips of 1024 threads
                         (all cases); the per-stack index branch with 16 stacks (cases 1, 2 and the Python side of 3);
                         the tile loop's second trip: more than 256 workgroups * 4 = 1024 tiles (case 2: 1056 tiles)
  sketch_residual_block  the pixel loop's second trip: more than 256 * 256 = 65 536 pixels (case 3: 71 680); the flush
                         of 1024 bucket sums by 256 threads, 4 trips (case 3, colour and RGB-D)
  mgs_lm_solve_step      the fused solve and the trust-region update over 1024 sketched rows (case 3)

640x480 itself stays run-only (tests/test_gpu_rgbd_tracking.py::test_replica_shape_rgbd_iterations, bench.py).
Bucket sums are float atomics: nothing here is compared bit for bit."""
import pytest
import torch

from conftest import gpu_settings, oracle_settings, rel_err
import sketch_oracle as SO
from test_raster_gpu import _dev, _inputs, _loop_fixture

pytestmark = pytest.mark.gpu

STACK, SKETCH = 16, 64
D = STACK * SKETCH


def _sketched_render(sc, inputs, idx, dev, sketch_mode):
    """One render through the autograd binding; sketch_mode 1: per-stack index table `idx` [1, 16, H, W]."""
    from monogs_amd.rasterizer import GaussianRasterizer
    N = inputs[0].shape[0]
    L = [t.to(dev).requires_grad_() for t in inputs]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    kw = {}
    sk = None
    if sketch_mode:
        sk = torch.empty(STACK, SKETCH, 6, device=dev, requires_grad=True)
        kw = dict(sketch_mode=1, sketch_dim=SKETCH, stack_dim=STACK, sketch_dtau=sk, sketch_indices=idx.to(dev))
    img, radii, dep, opa, nt = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))(
        means3D=L[0], means2D=torch.zeros(N, 3, device=dev, requires_grad=True), shs=L[4],
        opacities=L[3], scales=L[1], rotations=L[2], theta=theta, rho=rho, **kw)
    return img, dep, theta, rho, sk


def test_sketched_pose_jacobian_16x64_matches_the_fp64_oracle(built):
    """All 1024 rows of the sketched Jacobian (autograd binding, per-stack index table) against the fp64 oracle:
    the construction of test_sketched_pose_jacobian_matches_oracle[500-70-45-...] (70x45 = 3150 pixels, not a whole
    number of tiles; moved camera; scales * 1.5; random A_img / B_dep) with 16 x 64 buckets, so the 6144-float bucket
    table of k_sketch_bucket is zeroed and flushed in 6 trips and its per-stack branch walks 16 stacks.  The reference
    rows are bucket sums of the forward-mode per-pixel Jacobian (tests/sketch_oracle.py, held to reverse mode by
    tests/test_cpu_sketch_oracle.py).  Bound as in that test: max |got - want| <= 2e-3 max |SJ|.
    Reference-side conditions (measured on the CPU oracle): every bucket holds exactly 3 pixels; 78 pixels lie in no
    bucket; 1024 of 1024 buckets (100 %) have a non-zero oracle row, asserted >= 95 %.
    The figures are printed before they are asserted (run with -s)."""
    from monogs_amd import synthetic as S
    from monogs_amd.slam_loops import gen_forward_sketch_args
    from oracle import torch_raster as O
    dev = _dev()
    N, W, H = 500, 70, 45
    sc = S.make_scene(N, W, H, seed=12)
    sc = sc._replace(cam=S.make_camera(W, H, O.se3_exp(torch.tensor([0.04, -0.03, 0.08, 0.02, -0.03, 0.02]))))
    m, s, r, o, sh = _inputs(sc)
    s = s * 1.5
    g = torch.Generator().manual_seed(3)
    Aimg = torch.randn(3, H, W, generator=g)
    Bdep = torch.randn(1, H, W, generator=g)
    fsa = gen_forward_sketch_args(H, W, 1, STACK, SKETCH, "cpu", generator=g)
    idx, wts = fsa["sketch_indices"], fsa["rand_weights"][0]        # [1, 16, H, W], [H, W]

    # reference side
    counts = torch.stack([torch.bincount(idx[0, st][idx[0, st] >= 0].long(), minlength=SKETCH) for st in range(STACK)])
    assert fsa["chunk_size"] == 3 and bool((counts == 3).all())
    assert int((idx[0] < 0).all(0).sum()) == 78
    J = SO.per_pixel_pose_jacobian(m, s, r, o, sh, oracle_settings(sc.cam, sc.bg, dtype=torch.float64), Aimg, Bdep)
    want = SO.bucket_rows(J, idx[0], wts, SKETCH)
    nonzero = float((want.abs().amax(-1) > 0).double().mean())
    print(f"16x64 @ {W}x{H}: share of non-zero oracle rows {nonzero:.4f}")
    assert nonzero >= 0.95

    # HIP
    img, dep, theta, rho, sk = _sketched_render(sc, (m, s, r, o, sh), idx, dev, 1)
    res = (img * Aimg.to(dev)).sum(0) + (dep * Bdep.to(dev))[0]
    weighted = res * wts.to(dev)
    weighted.backward(gradient=torch.ones_like(weighted))
    torch.cuda.synchronize()
    SJ = sk.grad.double().cpu()
    assert SJ.shape == (STACK, SKETCH, 6)
    scale = SJ.abs().max().item()
    err = (SJ - want).abs().amax(-1)
    worst = err.max().item()
    print(f"16x64 @ {W}x{H}: worst |got - want| {worst:.3e}, max |SJ| {scale:.3e}, worst row (stack, bucket) "
          f"{divmod(int(err.argmax()), SKETCH)}")
    assert worst <= 2e-3 * scale, (worst, scale)


def test_bucket_kernel_second_tile_trip_matches_the_dense_backward(built):
    """520x512: 33 x 32 = 1056 tiles (a partial tile column), so the 256 workgroups x 4 tiles of k_sketch_bucket make a
    second trip for the tiles 1024 ... 1055; 520 * 512 = 260 * 1024 pixels, every pixel in a bucket.  The last tile row
    (image rows >= 496) is the tiles 1023 ... 1055: all of it but its first tile belongs to the second trip.  The index
    table is built on the host so that the 8320 pixels of the rows >= 496 fill 32 whole buckets of their own
    (tests/sketch_oracle.py::partition_with_tail_buckets), the 256 pixels of tile 1023 all in the first of them: the
    other 31 lie entirely in tiles >= 1024, and a bucket kernel that skips the second trip leaves exactly those rows
    empty.  Reference: the DENSE fp32 backward of the same render (sketch_mode 0: k_blend_bwd<false>
    and the per-Gaussian pose reduction - no slab, mask-word or bucket code) of the bucket's masked, weighted residual
    sum, for the 32 tail buckets and 32 others drawn at random.  Each side is held to 2e-3 of the oracle by other
    tests, hence max |SJ_bucket - dense| <= 4e-3 max |SJ|; over all 1024 buckets the rows add up to the full dense pose
    gradient (rel_err < 2e-3).  Condition: every dense reference row of a tail bucket is non-zero.
    The figures are printed before they are asserted (run with -s)."""
    from monogs_amd import synthetic as S
    dev = _dev()
    N, W, H, row0 = 4000, 520, 512, 496
    grid_x = (W + 15) // 16
    assert grid_x * ((H + 15) // 16) == 1056 and grid_x * (row0 // 16) == 1023
    sc = S.make_scene(N, W, H, seed=12)
    inputs = _inputs(sc)
    g = torch.Generator().manual_seed(7)
    Aimg = torch.randn(3, H, W, generator=g).to(dev)
    Bdep = torch.randn(1, H, W, generator=g).to(dev)
    tile_of = (torch.arange(H).view(-1, 1) // 16) * grid_x + torch.arange(W).view(1, -1) // 16      # [H, W]
    idx, tail = SO.partition_with_tail_buckets(H, W, STACK, SKETCH, row0, g, lead=tile_of == 1023)
    wts = (torch.randint(0, 2, (H, W), generator=g).float() * 2 - 1).to(dev)
    assert tail.numel() == 32
    others = torch.tensor([b for b in torch.randperm(D, generator=g).tolist() if b not in set(tail.tolist())][:32])
    idx_d = idx.to(dev)

    # sketched backward: all 1024 rows in one launch sequence
    img, dep, theta, rho, sk = _sketched_render(sc, inputs, idx, dev, 1)
    res = (img * Aimg).sum(0) + (dep * Bdep)[0]
    (res * wts).backward(gradient=torch.ones_like(res))
    torch.cuda.synchronize()
    SJ = sk.grad.clone()
    full_own = torch.cat([rho.grad, theta.grad])
    scale = SJ.abs().max().item()

    # dense backward of the same render, one call per compared bucket
    img, dep, theta, rho, _ = _sketched_render(sc, inputs, None, dev, 0)
    res = (img * Aimg).sum(0) + (dep * Bdep)[0]
    weighted = res * wts

    def dense(mask):
        gr, gt = torch.autograd.grad((weighted * mask).sum(), (rho, theta), retain_graph=True)
        return torch.cat([gr, gt])

    full = dense(torch.ones_like(weighted))
    worst = {"tail": 0.0, "random": 0.0}
    smallest_tail_row = float("inf")
    for tag, ids in (("tail", tail), ("random", others)):
        for b in ids.tolist():
            st, k = divmod(b, SKETCH)
            mask = idx_d[0, st] == k
            if tag == "tail":
                assert int(mask.sum()) == 260 and int(tile_of[mask.cpu()].min()) >= (1023 if b == int(tail[0]) else 1024)
            want = dense(mask)
            if tag == "tail":
                smallest_tail_row = min(smallest_tail_row, want.abs().max().item())
            worst[tag] = max(worst[tag], (SJ[st, k] - want).abs().max().item())
    e_sum, e_own = rel_err(SJ.sum((0, 1)), full), rel_err(SJ.sum((0, 1)), full_own)
    print(f"16x64 @ {W}x{H}: worst bucket difference tail {worst['tail']:.3e} / random {worst['random']:.3e}, "
          f"max |SJ| {scale:.3e}; sum of rows vs dense {e_sum:.3e}, vs the sketched launch's dL/dtau {e_own:.3e}; "
          f"smallest tail reference row {smallest_tail_row:.3e}")
    assert smallest_tail_row > 0.0
    assert worst["tail"] <= 4e-3 * scale, (worst, scale)
    assert worst["random"] <= 4e-3 * scale, (worst, scale)
    assert e_sum < 2e-3 and e_own < 2e-3


def _cam(view, uid, T0, target, gain=0.97):
    v = view(uid, T0)
    v.original_image = target
    v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    with torch.no_grad():
        v.exposure_a.fill_(gain)
        v.exposure_b.fill_(0.01)
    return v


def _assert_partition(bucket, HW):
    """so_bucket of the native iteration: values in [-1, 1024), every bucket exactly chunk pixels, the rest left over
    (a wrong cycle walk of the keyed permutation - 17 index bits above 65 536 pixels - breaks one of the three)."""
    b = bucket.reshape(-1).cpu().long()
    chunk = HW // D
    assert b.numel() == HW and int(b.min()) >= -1 and int(b.max()) < D
    assert bool((torch.bincount(b[b >= 0], minlength=D) == chunk).all())
    assert int((b < 0).sum()) == HW - D * chunk
    return chunk, HW - D * chunk


@pytest.mark.parametrize("W,H", [(320, 224), (150, 101)])
def test_native_second_order_iteration_16x64_matches_python_formulation(built, W, H):
    """test_native_second_order_iteration_matches_python_formulation at stack 16 / sketch 64 (1024 sketched rows through
    the residual pass, the sketch-mode backward, the fused LM solve and the trust-region update), same assertions and
    bounds.  320x224: 71 680 = 70 * 1024 pixels - above the 256 * 256 = 65 536 pixels of one trip of the residual
    pass's pixel loop, 280 tiles, chunk 70, no pixel left over, 17 index bits in the keyed permutation.  150x101:
    15 150 pixels, not a whole number of tiles, chunk 14, 814 pixels left over.
    The figures are printed before they are asserted (run with -s)."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, sketch_args_from_buckets, tracking_step_second_order
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture(N=4000, W=W, H=H)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    va, vb, vc = _cam(view, 2, T0, target), _cam(view, 3, T0, target), _cam(view, 4, T0, target)
    lam = 1e-3
    trk = NativeTracker(vb, gauss, bg)
    trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, initial_lambda=lam, seed=5, keep_sketch=True)
    state = trk.step_second_order()
    torch.cuda.synchronize()
    Sf_n, SJ_n = trk.sketch
    assert Sf_n.shape == (D,) and SJ_n.shape == (D, 8)
    chunk, left = _assert_partition(trk.so_bucket, H * W)
    assert (chunk, left) == {(320, 224): (70, 0), (150, 101): (14, 814)}[(W, H)]
    assert bool((trk.so_weights.abs() == 1).all())
    fsa = sketch_args_from_buckets(trk.so_bucket, trk.so_weights, H, W, STACK, SKETCH)
    l1, x, SJ, Sf = tracking_step_second_order(va, gauss, bg, lambda_=lam, repeat_dim=1, stack_dim=STACK,
                                               sketch_dim=SKETCH, fused_solve=True, fsa=fsa)
    errs = (rel_err(Sf_n, Sf), rel_err(SJ_n[:, 6:], SJ[:, 6:]), rel_err(SJ_n[:, :6], SJ[:, :6]), rel_err(trk.so_x, x))
    print(f"16x64 @ {W}x{H}: rel_err Sf {errs[0]:.3e}, exposure columns {errs[1]:.3e}, pose columns {errs[2]:.3e}, "
          f"LM step {errs[3]:.3e}; chunk {chunk}, left over {left}; worst Sf row "
          f"{int((Sf_n - Sf).abs().argmax())}, |x| {float(x.norm()):.3e}")
    assert float(Sf.abs().max()) > 0 and float(SJ[:, :6].abs().max()) > 0 and float(x.abs().max()) > 0
    assert errs[0] < 1e-4
    assert errs[1] < 1e-4                                     # exposure columns
    assert errs[2] < 2e-3                                     # pose columns (through the rasteriser)
    assert errs[3] < 5e-3
    assert torch.allclose(va.T, vb.T, atol=1e-4)
    assert torch.allclose(va.exposure_a, vb.exposure_a, atol=1e-4)
    assert torch.allclose(va.exposure_b, vb.exposure_b, atol=1e-4)
    st = state.cpu()
    assert abs(st[0].item() - lam) < 1e-9 and st[2].item() == 1.0
    assert abs(st[1].item() - float(l1)) < 1e-4 * float(l1)          # the L1 criterion, summed over all pixel trips
    # the memset-free form (accumulators cleared by their consumers) takes the same step and leaves them zero
    fast = NativeTracker(vc, gauss, bg)
    fast.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, initial_lambda=lam, seed=5)
    fast.step_second_order()
    torch.cuda.synchronize()
    assert torch.allclose(vc.T, vb.T, atol=1e-5) and torch.allclose(vc.exposure_a, vb.exposure_a, atol=1e-5)
    assert float(fast.so_accum.abs().max()) == 0.0
    assert trk.check_capacity() and fast.check_capacity()


def test_sketched_jacobian_16x64_sums_to_the_pose_gradient_with_depth_rows(built):
    """test_sketched_jacobian_sums_to_the_pose_gradient_with_depth_rows at 320x224 / 16 x 64 / alpha 0.9: the RGB-D
    residual pass (k_sketch_prep_residual_rgbd) past 65 536 pixels with 1024 bucket sums to flush.  Every pixel lies in
    exactly one bucket (71 680 = 1024 * 70), so the tau columns add up to the gradient of the weighted, Hubered,
    stacked residual; the alpha = 1 tracker (no depth row) must give a different vector.
    The figures are printed before they are asserted (run with -s)."""
    from monogs_amd import losses as Ls
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe
    from monogs_amd.tracking_native import NativeTracker
    from test_gpu_rgbd_tracking import _cfg, _frame, _target
    W, H, alpha = 320, 224, 0.9
    sc, gauss, view, dev = _loop_fixture(N=4000, W=W, H=H)
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.03, 0.004, -0.006, 0.003]))
    vb = _frame(view, 3, T0, target, depth)
    trk = NativeTracker(vb, gauss, bg, gt_depth=depth, alpha=alpha)
    trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, seed=5, keep_sketch=True)
    trk.step_second_order()
    torch.cuda.synchronize()
    Sf_n, SJ_n = trk.sketch
    assert Sf_n.shape == (D,) and SJ_n.shape == (D, 8)
    assert bool((trk.so_bucket >= 0).all())
    _assert_partition(trk.so_bucket, H * W)
    va = _frame(view, 2, T0, target, depth)
    pkg = render(va, gauss, Pipe, bg)
    res = Ls.get_loss_tracking_stacked(_cfg(alpha), pkg["render"], pkg["depth"], pkg["opacity"], va)
    res = Ls.HuberLoss.apply(res, 0.01).sum(dim=0) / (H * W / D)
    weighted = res * trk.so_weights.view(H, W)
    weighted.sum().backward()
    full = torch.cat([va.cam_trans_delta.grad, va.cam_rot_delta.grad])
    # Sf: the bucket sums of the same weighted residual (every bucket, colour and depth rows)
    Sf = torch.zeros(D, device=dev).index_add_(0, trk.so_bucket.reshape(-1).long(), weighted.detach().reshape(-1))
    e_sum, e_sf = rel_err(SJ_n[:, :6].sum(0), full), rel_err(Sf_n, Sf)
    vc = _frame(view, 4, T0, target, depth)
    trk1 = NativeTracker(vc, gauss, bg)
    trk1.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, seed=5, keep_sketch=True)
    trk1.step_second_order()
    e_mono = rel_err(trk1.sketch[1][:, :6].sum(0), full)
    print(f"16x64 RGB-D @ {W}x{H}: rel_err of the summed tau columns {e_sum:.3e}, Sf {e_sf:.3e}; alpha = 1 differs by {e_mono:.3e}")
    assert e_sum < 2e-3
    assert e_sf < 1e-4
    assert e_mono > 1e-2
