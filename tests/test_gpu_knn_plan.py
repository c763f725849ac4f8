"""distCUDA2 (csrc/knn.hip) at the sizes where its plan changes, compared directly with the oracle's formula.

The plan rule (knn_plan): a lane owns Q queries,
    Q = 4 for P >= 20 000,   Q = 2 for 11 000 <= P < 20 000,   Q = 1 below,
a workgroup 256 Q consecutive queries, and the candidates are cut into slices of whole batches of 8; the batches
that overlap the workgroup's own 256 Q queries carry the self-exclusion test, the others do not, and the fewer than
8 candidates left at the end of the last slice go one by one.  So the sizes that matter are the two switches of Q
from either side, and a P that is a multiple of neither 8 (a tail of single candidates) nor 256 Q (a last workgroup
with idle queries) for every Q.

Reference: oracle.torch_raster.dist2_knn3 - squared distances in fp64, the three smallest but the point itself,
their mean rounded to fp32 - evaluated with the same chunked formula in fp64 on the device (the CPU takes 1.9 s at
P = 11 000 and 6.1 s at 20 000), and held to the CPU oracle itself at a small P.  Bound: that of test_knn_dist2,
rtol 1e-4 / atol 1e-7.  The seed tests reach these kernels only through log(sqrt(max(d2, 1e-7) s)), whose clamp
hides small distances; here coincident points must give exactly 0.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOX = (4.0, 3.0, 6.0)
SIZES = (9600, 10999, 11000, 11003, 19999, 20000, 20003)      # 9 600: the TUM keyframe size
RTOL, ATOL = 1e-4, 1e-7


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _q_of(P):
    """knn_plan's choice of queries per lane, restated."""
    return 4 if P >= 20000 else (2 if P >= 11000 else 1)


def _points(P, seed=0):
    g = torch.Generator().manual_seed(seed + P)
    return torch.rand(P, 3, generator=g) * torch.tensor(BOX)


def _knn3_fp64(points, chunk=1024):
    """dist2_knn3's formula (P >= 4) on the points' own device: (mean of the three smallest squared distances to
    OTHER points, rounded to fp32; their indices)."""
    P = points.shape[0]
    assert P >= 4
    p64 = points.double()
    out = torch.empty(P, dtype=torch.float32, device=points.device)
    idx = torch.empty(P, 3, dtype=torch.long, device=points.device)
    for s in range(0, P, chunk):
        q = p64[s:s + chunk]
        d2 = ((q[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
        r = torch.arange(q.shape[0], device=points.device)
        d2[r, r + s] = float("inf")
        best = torch.topk(d2, 3, dim=1, largest=False)
        out[s:s + chunk] = (best.values.sum(1) / 3.0).float()
        idx[s:s + chunk] = best.indices
    return out, idx


def _check(pts_cpu, dev):
    from monogs_amd.knn import distCUDA2
    pts = pts_cpu.to(dev)
    got = distCUDA2(pts)
    want, idx = _knn3_fp64(pts)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = ((got.double() - want.double()).abs() / (ATOL + RTOL * want.double().abs())).max().item()
    print(f"P = {pts.shape[0]}: worst error {err:.3g} of the bound")
    assert torch.allclose(got, want, rtol=RTOL, atol=ATOL), err
    return got.cpu(), want.cpu(), idx.cpu()


def test_the_sizes_cover_the_plan_rule():
    """Each Q in {1, 2, 4} is hit from both sides of its switch, and has a P that is a multiple of neither 8 nor
    256 Q."""
    assert {_q_of(P) for P in SIZES} == {1, 2, 4}
    assert (_q_of(10999), _q_of(11000), _q_of(19999), _q_of(20000)) == (1, 2, 2, 4)
    for Q in (1, 2, 4):
        assert any(_q_of(P) == Q and P % 8 != 0 and P % (256 * Q) != 0 for P in SIZES), Q


def test_the_device_formula_is_the_oracle(built):
    from oracle import torch_raster as O
    pts = _points(1500)
    want = O.dist2_knn3(pts)
    got, _ = _knn3_fp64(pts.to(_dev()), chunk=256)
    assert torch.allclose(got.cpu(), want, rtol=2e-7, atol=0)      # one fp32 ulp: the order of the three-term sums


@pytest.mark.parametrize("P", SIZES)
def test_dist2_across_the_plan_switches(built, P):
    _check(_points(P), _dev())


@pytest.mark.parametrize("P", [11003, 20003])
def test_dist2_of_points_sorted_along_x(built, P):
    """The same points sorted along x: a point's neighbours lie within about one neighbour distance in x, which is
    a few hundred places in the sorted order (P r / 4 with r ~ (72 / P)^(1/3): ~500 at 11 003, ~780 at 20 003)
    against workgroup ranges of 512 and 1024 queries.  So for a large share of the points all three neighbours
    are candidates of the workgroup's own query range, the batches compiled with the self-exclusion test - in
    random order that takes (256 Q / P)^3 of the points, fewer than ten.  Asserted from the reference's neighbour
    indices: at least a twentieth of the points, and at least a hundred times the random order's share."""
    dev = _dev()
    pts = _points(P)
    srt = pts[torch.argsort(pts[:, 0])]
    span = 256 * _q_of(P)

    def own_range(idx):
        first = torch.arange(P) // span * span
        return int(((idx >= first[:, None]) & (idx < first[:, None] + span)).all(1).sum())

    _, _, idx_sorted = _check(srt, dev)
    _, idx_random = _knn3_fp64(pts.to(dev))
    n_sorted, n_random = own_range(idx_sorted), own_range(idx_random.cpu())
    print(f"P = {P}: all three neighbours in the own range for {n_sorted} sorted / {n_random} unsorted points")
    assert n_sorted >= P // 20 and n_sorted >= 100 * max(n_random, 1)


@pytest.mark.parametrize("P", [11003, 20003])
def test_dist2_with_coincident_points(built, P):
    """64 rows overwritten with exact copies of other rows (their nearest neighbour is at distance exactly 0: half
    of the copies sit next to their original, inside the same workgroup's self-exclusion batches, half far from
    it), and one group of four coincident points, which must give exactly 0 - a point is excluded by its index,
    never by its distance.  Exact copies only: nearly coincident points cancel in fp32 and would need a wider
    bound than the project has."""
    dev = _dev()
    pts = _points(P)
    g = torch.Generator().manual_seed(P)
    # 128 distinct rows: even places for the originals and the far copies, the odd place after an original for a
    # near copy; clear of the group of four below
    h = P // 2
    cand = 8 + 2 * torch.randperm((P - 16) // 2, generator=g)
    cand = cand[(cand != h) & (cand != h - 1)][:96]
    src = cand[:64]
    dst = torch.cat([src[:32] + 1, cand[64:]])                # next to the original / anywhere
    assert len(dst) == 64 and len(torch.unique(torch.cat([src, dst]))) == 128      # pairs only, no chains
    pts[dst] = pts[src]
    four = torch.tensor([5, 6, h, P - 1])                # same wave, another workgroup, the single-candidate tail
    pts[four] = pts[5].clone()
    got, want, idx = _check(pts, dev)
    assert bool((want[four] == 0).all()) and bool((got[four] == 0).all()), got[four]
    # a copy and its original see each other at 0 and two true neighbours beyond
    assert bool((got[dst] > 0).all()) and bool((idx[dst, 0] == src).all()) and bool((idx[src, 0] == dst).all())
