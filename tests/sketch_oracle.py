"""fp64 reference rows for the sketched pose Jacobian, for any number of buckets.

The per-bucket reference of tests/test_raster_gpu.py::test_sketched_pose_jacobian_matches_oracle costs one reverse
pass of the CPU oracle per bucket.  The pose has six degrees of freedom, so SIX forward-mode passes give the whole
per-pixel Jacobian J[H, W, 6], and the row of a bucket is a plain sum of weights_p * J_p over its pixels."""
import torch
import torch.autograd.forward_ad as fwAD


def f64(t):
    return None if t is None else t.detach().double()


def residual(means, scales, rots, opac, shs, settings, A_img, B_dep, rho, theta):
    """res[H, W] = sum_c img_c * A_c + depth * B of the CPU oracle's render (the construction of the reference's hot-
    path self check, slam_frontend.py:1031-1127); `settings` = conftest.oracle_settings(..., dtype=torch.float64)."""
    from oracle import torch_raster as O
    img, _, dep, _, _, _ = O.rasterize(means, None, shs, None, opac, scales, rots, None, settings, theta, rho)
    return (img * A_img).sum(0) + (dep * B_dep)[0]


def per_pixel_pose_jacobian(means, scales, rots, opac, shs, settings, A_img, B_dep):
    """J[H, W, 6] (fp64): the derivative of residual() at every pixel w.r.t. tau = [rho; theta], by six forward-mode
    passes through oracle.torch_raster.rasterize as it stands (its detached masks and the straight-through clamp
    drop the tangent exactly where reverse mode drops the cotangent)."""
    ins = [f64(t) for t in (means, scales, rots, opac, shs)]
    A, B = f64(A_img), f64(B_dep)
    cols = []
    for i in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[i] = 1.0
        with fwAD.dual_level():
            tau = fwAD.make_dual(torch.zeros(6, dtype=torch.float64), e)
            res = residual(*ins, settings, A, B, tau[:3], tau[3:])
            tangent = fwAD.unpack_dual(res).tangent
            cols.append(torch.zeros_like(res.detach()) if tangent is None else tangent.clone())
    return torch.stack(cols, dim=-1)


def partition_with_tail_buckets(H, W, stack, sketch, row0, generator, lead=None):
    """An index table [1, stack, H, W] (int32, the layout of gen_forward_sketch_args) in which the pixels of the image
    rows >= row0 fill WHOLE buckets of their own: (H - row0) * W must be a multiple of chunk = H * W // (stack *
    sketch).  Which buckets those are, and which pixels go to which bucket, is drawn at random - except that the pixels
    of `lead` (a boolean [H, W] mask inside the rows >= row0), if given, are put first: they fill tail[0], tail[1] ...
    as far as they go, so the remaining tail buckets hold no pixel of `lead`.  Returns (idx, tail): tail = the flat ids
    (s * sketch + k) of the buckets that lie in the rows >= row0."""
    m, d = H * W, stack * sketch
    chunk = m // d
    n_tail_px = (H - row0) * W
    assert n_tail_px % chunk == 0 and chunk * d == m, (H, W, row0, chunk)
    n_tail = n_tail_px // chunk
    order = torch.randperm(d, generator=generator)
    tail, head = order[:n_tail], order[n_tail:]
    px_tail = row0 * W + torch.randperm(n_tail_px, generator=generator)
    if lead is not None:
        assert not bool(lead[:row0].any())
        first = lead.reshape(-1)[px_tail]
        px_tail = torch.cat([px_tail[first], px_tail[~first]])
    px_head = torch.randperm(row0 * W, generator=generator)
    flat = torch.empty(m, dtype=torch.long)                    # pixel -> flat bucket
    flat[px_tail] = tail.repeat_interleave(chunk)
    flat[px_head] = head.repeat_interleave(chunk)
    idx = torch.full((stack, m), -1, dtype=torch.int32)
    idx[flat // sketch, torch.arange(m)] = (flat % sketch).to(torch.int32)
    return idx.view(1, stack, H, W), tail


def bucket_rows(J, sketch_idx, weights, sketch_dim):
    """Rows [stack, sketch_dim, 6] of the sketched Jacobian: for every stack s, bucket k collects weights_p * J_p of
    the pixels with sketch_idx[s, p] == k (sketch_idx [stack, H, W], -1 = in no bucket; weights [H, W])."""
    stack = sketch_idx.shape[0]
    wj = (J * weights.double()[..., None]).reshape(-1, 6)
    out = torch.zeros(stack, sketch_dim, 6, dtype=torch.float64)
    for s in range(stack):
        k = sketch_idx[s].reshape(-1).long()
        on = k >= 0
        out[s].index_add_(0, k[on], wj[on])
    return out
