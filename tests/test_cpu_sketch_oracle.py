"""The forward-mode per-pixel pose Jacobian of tests/sketch_oracle.py (the reference side of
tests/test_gpu_sketch_shipped_dims.py) against reverse mode through the same fp64 oracle."""
import torch

from conftest import oracle_settings
import sketch_oracle as SO


def test_forward_mode_pixel_jacobian_reproduces_reverse_mode():
    """70x45 / 500 Gaussians, moved camera (the scene of the 16 x 64 GPU comparison): for random pixel masks,
    J[mask].sum(0) must equal autograd.grad(res[mask].sum(), tau).  Both sides are fp64 runs of one oracle, so the
    bound is 1e-10 of the largest gradient entry; bucket_rows() must be the same sums for a 2 x 5 index table."""
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    N, W, H = 500, 70, 45
    sc = S.make_scene(N, W, H, seed=12)
    sc = sc._replace(cam=S.make_camera(W, H, O.se3_exp(torch.tensor([0.04, -0.03, 0.08, 0.02, -0.03, 0.02]))))
    m, s, r, o, sh = S.activated(sc)
    s = s * 1.5
    g = torch.Generator().manual_seed(3)
    A = torch.randn(3, H, W, generator=g)
    B = torch.randn(1, H, W, generator=g)
    st = oracle_settings(sc.cam, sc.bg, dtype=torch.float64)
    J = SO.per_pixel_pose_jacobian(m, s, r, o, sh, st, A, B)
    assert J.shape == (H, W, 6) and J.dtype == torch.float64 and bool(torch.isfinite(J).all())
    assert float((J.abs().amax(-1) > 0).double().mean()) > 0.5          # not a Jacobian of background pixels

    rho = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    theta = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    res = SO.residual(*[SO.f64(t) for t in (m, s, r, o, sh)], st, A.double(), B.double(), rho, theta)
    masks = [torch.rand(H, W, generator=g) < p for p in (0.5, 0.1, 0.01)]
    masks += [torch.ones(H, W, dtype=torch.bool), torch.zeros(H, W, dtype=torch.bool)]
    masks[-1][H - 1, W - 1] = True                                      # one pixel, in the partial tile column
    for mask in masks:
        gr, gt = torch.autograd.grad(res[mask].sum(), (rho, theta), retain_graph=True)
        want = torch.cat([gr, gt])
        got = J[mask].sum(0)
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max()), (int(mask.sum()), got, want)

    # bucket_rows: a signed 2 x 5 table with left-over pixels, against the masked sums
    idx = torch.randint(-1, 5, (2, H, W), generator=g, dtype=torch.int32)
    w = torch.randint(0, 2, (H, W), generator=g).double() * 2 - 1
    rows = SO.bucket_rows(J, idx, w, 5)
    assert rows.shape == (2, 5, 6)
    for s_ in range(2):
        for k in range(5):
            want = (J * w[..., None])[idx[s_] == k].sum(0)
            assert float((rows[s_, k] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_partition_with_tail_buckets_is_an_equal_partition_with_whole_buckets_in_the_last_rows():
    """64 x 48 into 4 x 8 buckets of 96 pixels, the last 6 rows = 4 buckets: every pixel in exactly one (stack,
    bucket), every bucket `chunk` pixels, the tail buckets entirely in the rows >= 42 and no other bucket there."""
    H, W, stack, sketch, row0 = 48, 64, 4, 8, 42
    g = torch.Generator().manual_seed(1)
    idx, tail = SO.partition_with_tail_buckets(H, W, stack, sketch, row0, g)
    assert idx.shape == (1, stack, H, W) and idx.dtype == torch.int32 and tail.numel() == 4
    assert bool(((idx[0] >= 0).sum(0) == 1).all()) and int(idx.max()) == sketch - 1 and int(idx.min()) == -1
    s_of = (idx[0] >= 0).long().argmax(0)
    flat = s_of * sketch + idx[0].long().gather(0, s_of[None])[0]
    assert bool((torch.bincount(flat.reshape(-1), minlength=stack * sketch) == H * W // (stack * sketch)).all())
    in_tail = torch.isin(flat, tail)
    assert bool(in_tail[row0:].all()) and not bool(in_tail[:row0].any())
    # lead: the 6 x 16 pixels of the last rows' first tile column all land in tail[0]; no other bucket holds one
    lead = torch.zeros(H, W, dtype=torch.bool)
    lead[row0:, :16] = True
    idx, tail = SO.partition_with_tail_buckets(H, W, stack, sketch, row0, g, lead=lead)
    s_of = (idx[0] >= 0).long().argmax(0)
    flat = s_of * sketch + idx[0].long().gather(0, s_of[None])[0]
    assert bool((torch.bincount(flat.reshape(-1), minlength=stack * sketch) == H * W // (stack * sketch)).all())
    assert bool(torch.isin(flat, tail)[row0:].all()) and not bool(torch.isin(flat, tail)[:row0].any())
    assert bool((flat[lead] == tail[0]).all()) and int((flat == tail[0]).sum()) == 96
