"""Map maintenance past the sizes at which every loop in its kernels makes one trip
(csrc/map_update.hip), and at the edges of the rebuild plan.

Every case compares the HIP path with oracle/map_update_ref.py on the CPU or with plain torch, and first
asserts the precondition that puts it on the path it names.  Bounds are those of
test_raster_gpu.py::test_densify_and_prune_matches_the_reference_restatement: row copies, Adam moments, ids and
counts bit-exact; the xyz and scaling of split children rtol 1e-5 / atol 1e-6 (expf / logf / the rotation on the
device against torch on the CPU).

Thresholds crossed here ("Size thresholds of the map kernels"):
  k_plan_scan      1024 plan blocks per trip          n = 1 049 601 -> 1026 blocks, a second trip with a carry
  k_gather_rows    4096 x 256 threads per trip        rows x 45 > 1 048 576 (SH degree 3)
  k_map_append     4096 x 256 threads per trip        (old + new) x 45 > 1 048 576
  k_pack_grads     8192 x 256 threads per trip        16 N + ... > 2 097 152
  k_adam_multi     vec = 0 (a pointer off 16 bytes), 8 groups, numel < 4, numel = 0
"""
import ctypes as C

import pytest
import torch

from map_models import ATTR, _make_model, _state_of

pytestmark = pytest.mark.gpu

PLAN_BLOCK = 1024              # kPlanBlock: Gaussians per plan workgroup
SCAN_TRIP = 1024               # k_plan_scan: plan blocks per trip
GATHER_CAP = 4096 * 256        # k_gather_rows / k_map_append: elements per trip of the widest tensor
PACK_CAP = 8192 * 256          # k_pack_grads
EXTENT, MAX_GRAD, MIN_OPACITY = 6.0, 2e-4, 0.1


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _plan_columns(state, percent_dense, max_screen_size):
    """The four plan columns (kept original, clone, split children, selected) per Gaussian, from the
    restatement's own masks (oracle/map_update_ref.py:densify_and_prune)."""
    grads = state["grad_accum"] / state["denom"]
    grads[grads.isnan()] = 0.0
    hot = grads.squeeze(-1) >= MAX_GRAD
    smax = torch.exp(state["scaling"]).max(dim=1).values
    clone = hot & (smax <= percent_dense * EXTENT)
    split = hot & (smax > percent_dense * EXTENT)
    low = (torch.sigmoid(state["opacity"]) < MIN_OPACITY).squeeze(-1)
    big = (smax > 0.1 * EXTENT) if max_screen_size else torch.zeros_like(low)
    big_child = (torch.exp(torch.log(torch.exp(state["scaling"]) / 1.6)).max(dim=1).values > 0.1 * EXTENT) \
        if max_screen_size else torch.zeros_like(low)
    return torch.stack([~split & ~low & ~big, clone & ~low & ~big, split & ~low & ~big_child, split], 1)


def _step_twice(m, attr, dev, g):
    """Two optimiser steps so that the Adam moments are populated."""
    for a in attr.values():
        getattr(m, a).grad = torch.randn(getattr(m, a).shape, generator=g).to(dev) * 1e-2
    m.optimizer.step()
    m.optimizer.step()


def _clear_of_thresholds(m, attr, state, percent_dense, max_screen_size, dev):
    """densify_and_prune decides by comparing exp(scaling) and sigmoid(opacity) with thresholds; expf on the
    device and torch.exp on the CPU may differ in the last place, so a Gaussian within an ulp of a threshold can
    fall on either side and every later row would shift.  At 10^6 random rows a few do.  Rows within 1e-4
    (relative) of a scale threshold get their log-scales lowered by 0.01, rows within 1e-5 of the opacity
    threshold their logit raised by 0.01 - in the model and in `state` alike; the thresholds are a factor 1.6 or
    more apart, so a moved row lands near no other."""
    sc, op = state["scaling"], state["opacity"]
    smax = torch.exp(sc).max(dim=1).values
    near = torch.zeros_like(smax, dtype=torch.bool)
    for thr in [percent_dense * EXTENT] + ([0.1 * EXTENT, 0.16 * EXTENT] if max_screen_size else []):
        near |= (smax / thr - 1.0).abs() < 1e-4
    sc[near] -= 0.01
    near_o = ((torch.sigmoid(op) - MIN_OPACITY).abs() < 1e-5).squeeze(-1)
    op[near_o] += 0.01
    getattr(m, attr["scaling"]).data.copy_(sc.to(dev))
    getattr(m, attr["opacity"]).data.copy_(op.to(dev))


def _assert_state(got, want, n_child_rows=0, exact=False):
    """`n_child_rows`: the trailing rows that are split children; everything before them is a row copy."""
    for k, w in want.items():
        gk = got[k]
        assert gk.shape == w.shape, (k, gk.shape, w.shape)
        if not w.dtype.is_floating_point:
            assert gk.dtype == torch.int32 and torch.equal(gk, w.to(gk.dtype)), k
        elif exact or k not in ("xyz", "scaling"):
            assert torch.equal(gk, w), k
        else:
            assert torch.allclose(gk, w, rtol=1e-5, atol=1e-6), k
            copies = w.shape[0] - n_child_rows
            assert torch.equal(gk[:copies], w[:copies]), k


def _assert_registered(m, attr):
    """The rebuilt parameters are leaves registered in the optimiser, with moments of their own shape."""
    for grp in m.optimizer.param_groups:
        p = grp["params"][0]
        assert p is getattr(m, attr[grp["name"]]) and p.requires_grad and p.is_leaf
        st = m.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape


def _densify_against_ref(m, attr, cpu, before, max_screen_size, noise, dev, pass_noise=True):
    from monogs_amd import map_update as MU
    from oracle import map_update_ref as REF
    cols = _plan_columns({k: v.clone() for k, v in before.items()}, m.percent_dense, max_screen_size)
    want = REF.densify_and_prune({k: v.clone() for k, v in before.items()}, MAX_GRAD, MIN_OPACITY, EXTENT,
                                 max_screen_size, m.percent_dense, noise)
    MU.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size,
                         noise=noise.to(dev) if pass_noise else None)
    got = _state_of(m, attr, cpu)
    n_child = int(cols[:, 2].sum())
    assert want["xyz"].shape[0] == int(cols[:, 0].sum()) + int(cols[:, 1].sum()) + 2 * n_child
    _assert_state(got, want, n_child_rows=2 * n_child)
    _assert_registered(m, attr)
    return got, want, cols


# ---------------------------------------------------------------------------------------
# k_plan_scan: second trip
# ---------------------------------------------------------------------------------------
def test_plan_scan_second_trip_carries_the_running_total(built):
    """n = 1024 * 1025 + 1 = 1 049 601 Gaussians are 1026 plan blocks: k_plan_scan scans 1024 block counts per
    trip, so blocks 1024 and 1025 (rows >= 1 048 576) are placed by a second trip whose positions start at the
    first trip's total.  densify_and_prune with a supplied noise, then prune_points with a random mask on its
    result (about 1.36 million rows: two trips again), each against the restatement.  Every plan column is
    non-zero both below and from row 1 048 576 on, so the carry is non-zero in every column and rows depend on it.
    The restatement takes 0.4 - 0.8 s for the densify and 0.1 s for the prune at this n on 8 CPU threads (the
    seeded normals of the model itself take 2.8 s), so the two halves stay in one case."""
    from monogs_amd import _cabi, map_update as MU
    from oracle import map_update_ref as REF
    dev = _dev()
    n = PLAN_BLOCK * (SCAN_TRIP + 1) + 1
    assert n == 1049601 and _cabi.lib().mgs_map_plan_blocks(n) == 1026 > SCAN_TRIP
    m, cpu, attr = _make_model(n, dev, 11, fused=True, rest=0)
    g = torch.Generator().manual_seed(2)
    _step_twice(m, attr, dev, g)
    before = _state_of(m, attr, cpu)
    _clear_of_thresholds(m, attr, before, m.percent_dense, 20, dev)
    cols = _plan_columns({k: v.clone() for k, v in before.items()}, m.percent_dense, 20)
    first = PLAN_BLOCK * SCAN_TRIP
    assert bool((cols[:first].sum(0) > 0).all()), cols[:first].sum(0)      # a non-zero carry in every column ...
    assert bool((cols[first:].sum(0) > 0).all()), cols[first:].sum(0)      # ... that rows of the second trip need
    noise = torch.randn(2 * int(cols[:, 3].sum()), 3, generator=g)
    got, want, _ = _densify_against_ref(m, attr, cpu, before, 20, noise, dev)

    rows = got["xyz"].shape[0]
    assert _cabi.lib().mgs_map_plan_blocks(rows) > SCAN_TRIP
    mask = torch.rand(rows, generator=g) < 0.3
    assert int((~mask[:first]).sum()) > 0 and int((~mask[first:]).sum()) > 0
    # statistics are gathered by prune_points: give them values to carry
    m.xyz_gradient_accum = torch.rand(rows, 1, generator=g).to(dev)
    m.denom = torch.rand(rows, 1, generator=g).to(dev)
    m.max_radii2D = torch.rand(rows, generator=g).to(dev)
    got = _state_of(m, attr, cpu)
    want2 = REF.prune_points(got, mask)
    MU.prune_points(m, mask.to(dev))
    _assert_state(_state_of(m, attr, cpu), want2, exact=True)
    _assert_registered(m, attr)


# ---------------------------------------------------------------------------------------
# grid caps of the row movers
# ---------------------------------------------------------------------------------------
def test_gather_strides_past_its_grid_cap(built):
    """k_gather_rows' grid is capped at 4096 blocks of 256 threads, sized for the widest tensor, and loops beyond:
    with SH degree 3 (rest = 15, width 45) the rebuilt f_rest and its two moments make a second and third trip,
    the narrow tensors of the same launch one.  Parameters, both moments, kf and n_obs against the restatement."""
    dev = _dev()
    n = 40000
    m, cpu, attr = _make_model(n, dev, 13, fused=True, rest=15)
    g = torch.Generator().manual_seed(3)
    _step_twice(m, attr, dev, g)
    before = _state_of(m, attr, cpu)
    assert before["f_rest"][0].numel() == 45
    _clear_of_thresholds(m, attr, before, m.percent_dense, None, dev)
    cols = _plan_columns({k: v.clone() for k, v in before.items()}, m.percent_dense, None)
    noise = torch.randn(2 * int(cols[:, 3].sum()), 3, generator=g)
    got, want, _ = _densify_against_ref(m, attr, cpu, before, None, noise, dev)
    rows = got["xyz"].shape[0]
    assert rows * 45 > GATHER_CAP and rows * 4 < GATHER_CAP, rows      # only the width-45 tensors stride
    assert bool((cols.sum(0) > 0).all())


def test_append_strides_past_its_grid_cap(built):
    """GaussianModel.extend_from_pcd (one mgs_map_append launch, grid capped like the gather's) on 20 000 old +
    4 800 new rows of an SH-degree-3 model against REF.extend_from_pcd: old rows, new rows, the zero-filled
    moments of the new rows (the kernel's `new_rows == NULL` branch), kf, n_obs and the restarted statistics."""
    from monogs_amd.gaussian_model import GaussianModel
    from oracle import map_update_ref as REF
    dev = _dev()
    g = torch.Generator().manual_seed(5)

    def cloud(P):
        return (torch.randn(P, 3, generator=g), torch.randn(P, 3, 16, generator=g), torch.randn(P, 3, generator=g),
                torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g))

    n_old, n_new = 20000, 4800
    assert (n_old + n_new) * 45 > GATHER_CAP and n_old * 45 < GATHER_CAP      # the second trip copies new rows only
    gm = GaussianModel(sh_degree=3, device=dev)
    gm.init_lr(1.0)
    gm.extend_from_pcd(*(t.to(dev) for t in cloud(n_old)), kf_id=0)
    gm.training_setup()
    gm.unique_kfIDs = torch.randint(0, 9, (n_old,), generator=g).int().to(dev)
    gm.n_obs = torch.randint(0, 5, (n_old,), generator=g).int().to(dev)
    _step_twice(gm, ATTR, dev, g)
    gm.xyz_gradient_accum += 1.0
    before = _state_of(gm, ATTR, None)
    assert before["f_rest"].shape == (n_old, 15, 3) and float(before["exp_avg_f_rest"].abs().min()) > 0
    new = cloud(n_new)
    want = REF.extend_from_pcd(before, *new, 7)
    gm.extend_from_pcd(*(t.to(dev) for t in new), kf_id=7)
    _assert_state(_state_of(gm, ATTR, None), want, exact=True)
    _assert_registered(gm, ATTR)
    assert all(gm.optimizer.state[grp["params"][0]]["step"] == 2 for grp in gm.optimizer.param_groups)


def test_pack_strides_past_its_grid_cap(built):
    """k_pack_grads' grid is capped at 8192 blocks of 256 threads: N = 150 001 with the five gradient shapes of
    test_gradient_bucket_pack_kernel_matches_torch is 14 N of gradients + 2 N of statistics = 2 400 016 elements,
    so the statistics and the end of the last gradient come from the second trip.  Bound as in that test."""
    from monogs_amd.parallel import FlatGradBucket
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    N = 150001
    shapes = [(N, 3), (N, 1, 3), (N, 1), (N, 3), (N, 4)]
    params = [torch.zeros(s, device=dev) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    n_grad = sum(p.numel() for p in params)
    assert n_grad + 2 * N == 16 * N == 2400016 > PACK_CAP and n_grad > PACK_CAP > n_grad - params[4].numel()
    m2d = torch.randn(N, 3, generator=g).to(dev)
    radii = torch.randint(-1, 4, (N,), generator=g).int().to(dev)
    b = FlatGradBucket(params)
    want = torch.cat([p.grad.reshape(-1) for p in params]
                     + [torch.where(radii > 0, torch.linalg.norm(m2d[:, :2], dim=-1), torch.zeros(N, device=dev)),
                        (radii > 0).float()])
    b.flat.fill_(float("nan"))
    b.radii.fill_(-7)
    stat, denom, rad = b.all_reduce(m2d, radii)          # single process: pack + unpack
    assert b.flat.shape == want.shape and torch.allclose(b.flat, want, rtol=1e-6, atol=0)
    assert torch.equal(b.flat[:n_grad], want[:n_grad])   # the gradients are copies
    assert torch.equal(rad, radii) and torch.equal(b.radii, radii) and torch.equal(denom, (radii > 0).float())
    assert params[4].grad.data_ptr() == b.flat[sum(p.numel() for p in params[:4]):].data_ptr()


# ---------------------------------------------------------------------------------------
# plan edges: prune_points is exact
# ---------------------------------------------------------------------------------------
def _keep_mask(kind, n, g):
    i = torch.arange(n)
    if kind == "all":
        return torch.ones(n, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(n, dtype=torch.bool)
    if kind == "lane63":                    # every wave's only survivor is its last lane
        return i % 64 == 63
    if kind == "block_last_row":            # every block's only survivor is its last thread
        return i % PLAN_BLOCK == PLAN_BLOCK - 1
    if kind == "block_last_wave":           # every block's survivors all sit in its last wave
        return i % PLAN_BLOCK >= PLAN_BLOCK - 64
    assert kind == "random"
    return torch.rand(n, generator=g) < 0.5


@pytest.mark.parametrize("kind", ["all", "none", "lane63", "block_last_row", "block_last_wave", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_prune_points_at_wave_and_block_edges(built, n, kind):
    """prune_points at n around one wave (64) and one plan block (1024), with survivor patterns that put a wave's
    whole count in lane 63, a block's in its last thread or last wave, all rows or none: torch.equal against the
    reference's boolean indexing.  A pattern that has no row at this n is the "none" case: zero rows, every
    tensor and moment of shape (0, ...), parameters still registered, and the optimiser still steps."""
    from monogs_amd import map_update as MU
    from oracle import map_update_ref as REF
    dev = _dev()
    m, cpu, attr = _make_model(n, dev, 100 + n, fused=True, rest=2)
    g = torch.Generator().manual_seed(n)
    _step_twice(m, attr, dev, g)
    keep = _keep_mask(kind, n, g)
    expect = {"all": n, "none": 0, "lane63": n // 64, "block_last_row": n // PLAN_BLOCK,
              "block_last_wave": 64 * (n // PLAN_BLOCK) + max(0, n % PLAN_BLOCK - (PLAN_BLOCK - 64))}
    if kind in expect:
        assert int(keep.sum()) == expect[kind]
    before = _state_of(m, attr, cpu)
    want = REF.prune_points(before, ~keep)
    MU.prune_points(m, (~keep).to(dev))
    got = _state_of(m, attr, cpu)
    assert got["xyz"].shape[0] == int(keep.sum())
    _assert_state(got, want, exact=True)
    _assert_registered(m, attr)
    # the rebuilt model, empty or not, still steps
    for a in attr.values():
        getattr(m, a).grad = torch.ones_like(getattr(m, a))
    m.optimizer.step()
    torch.cuda.synchronize()
    assert getattr(m, attr["xyz"]).shape == want["xyz"].shape
    if want["xyz"].shape[0]:
        assert float((getattr(m, attr["xyz"]).detach().cpu() - want["xyz"]).abs().min()) > 0


# ---------------------------------------------------------------------------------------
# densify edges: crafted statistics at n = 1025 (one full plan block and one row)
# ---------------------------------------------------------------------------------------
def _crafted(n, dev, seed, hot, large, low):
    """A model whose rows are hot (gradient 1 >= 2e-4) / large (scale ~0.37 against a dense extent of 0.06,
    otherwise ~0.0025) / low (opacity logit -10, otherwise ~ +2) exactly where the masks say: far from every
    threshold."""
    m, cpu, attr = _make_model(n, dev, seed, fused=True, rest=1)
    g = torch.Generator().manual_seed(seed + 1)
    _step_twice(m, attr, dev, g)
    sc = torch.where(large[:, None], torch.tensor(-1.0), torch.tensor(-6.0)) + 0.1 * torch.randn(n, 3, generator=g)
    op = torch.where(low[:, None], torch.tensor(-10.0), torch.tensor(2.0)) + 0.3 * torch.randn(n, 1, generator=g)
    getattr(m, attr["scaling"]).data.copy_(sc.to(dev))
    getattr(m, attr["opacity"]).data.copy_(op.to(dev))
    m.xyz_gradient_accum = hot[:, None].float().to(dev)
    m.denom = torch.ones(n, 1).to(dev)
    return m, cpu, attr, g


@pytest.mark.parametrize("case", ["nothing_selected", "everything_split", "everything_pruned",
                                  "alternate_children_pruned"])
def test_densify_and_prune_edge_selections(built, case):
    """densify_and_prune at n = 1025 against the restatement, with statistics crafted so that
      nothing_selected           no Gaussian splits (clones only): n_par = 0, no noise is drawn or read;
      everything_split           every Gaussian splits and every child survives: no original, no clone, 2 n rows;
      everything_pruned          every Gaussian is selected and every row is pruned by opacity: zero rows;
      alternate_children_pruned  about half the rows are selected and every other selected parent's children are
                                 pruned by opacity: a surviving child's noise row is its parent's ordinal among
                                 the SELECTED (the reference draws noise before the final prune), not its ordinal
                                 among the surviving children - asserted to differ."""
    dev = _dev()
    n = PLAN_BLOCK + 1
    g0 = torch.Generator().manual_seed(77)
    every = torch.ones(n, dtype=torch.bool)
    if case == "nothing_selected":
        hot, large, low = torch.rand(n, generator=g0) < 0.5, ~every, torch.rand(n, generator=g0) < 0.2
    elif case == "everything_split":
        hot, large, low = every, every, ~every
    elif case == "everything_pruned":
        hot, large, low = every, every, every
    else:
        hot, large = torch.rand(n, generator=g0) < 0.7, torch.rand(n, generator=g0) < 0.7
        sel = hot & large
        low = torch.rand(n, generator=g0) < 0.1
        low[sel] = (torch.cumsum(sel, 0)[sel] - 1) % 2 == 1      # every other selected parent
        hot[-1] = large[-1] = True                               # the row of the second plan block is a parent
        low[-1] = False
    m, cpu, attr, g = _crafted(n, dev, 31, hot, large, low)
    before = _state_of(m, attr, cpu)
    cols = _plan_columns({k: v.clone() for k, v in before.items()}, m.percent_dense, None)
    n_sel, n_child = int(cols[:, 3].sum()), int(cols[:, 2].sum())
    assert bool((cols[:, 3] == (hot & large)).all())
    if case == "nothing_selected":
        assert n_sel == 0 and n_child == 0 and int(cols[:, 1].sum()) > 0
    elif case == "everything_split":
        assert n_sel == n == n_child and int(cols[:, 0].sum()) == 0 and int(cols[:, 1].sum()) == 0
    elif case == "everything_pruned":
        assert n_sel == n and int(cols[:, :3].sum()) == 0
    else:
        kept = cols[:, 2]
        sel_ord = (torch.cumsum(cols[:, 3], 0) - 1)[kept]
        child_ord = (torch.cumsum(kept, 0) - 1)[kept]
        assert 0 < n_child < n_sel and int((sel_ord != child_ord).sum()) > 0 and bool(kept[-1])
    noise = torch.randn(2 * n_sel, 3, generator=g)
    got, want, _ = _densify_against_ref(m, attr, cpu, before, None, noise, dev, pass_noise=n_sel > 0)
    expect_rows = {"everything_split": 2 * n, "everything_pruned": 0}
    if case in expect_rows:
        assert got["xyz"].shape[0] == expect_rows[case]
    for a in attr.values():      # the rebuilt model, empty or not, still steps
        getattr(m, a).grad = torch.ones_like(getattr(m, a))
    m.optimizer.step()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# k_adam_multi: scalar path, all 8 groups, tiny and empty groups
# ---------------------------------------------------------------------------------------
ADAM_NUMELS = (1, 2, 3, 5, 4099, 0, 7, 1024)
ADAM_LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 1e-3, 7e-3, 3.3e-5, 1e-2)
ADAM_STEP0 = (1, 2, 5, 40, 3, 9, 1000, 1)      # the first step of each group
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-15
ADAM_STEPS = 3


def _adam_layout(lead):
    """Element offsets of the 8 groups in a flat buffer: the first group starts `lead` floats in, every group at a
    multiple of 4 floats after that, with at least 4 guard floats between groups and at either end."""
    offs, o = [], lead
    for k in ADAM_NUMELS:
        offs.append(o)
        o += (k + 3) // 4 * 4 + 4
    return offs, o + 4


def _adam_inputs():
    g = torch.Generator().manual_seed(17)
    return {"p": [torch.randn(k, generator=g) for k in ADAM_NUMELS],
            "m": [0.1 * torch.randn(k, generator=g) for k in ADAM_NUMELS],
            "v": [0.01 * (0.5 + torch.rand(k, generator=g)) for k in ADAM_NUMELS],
            "g": [[torch.randn(k, generator=g) * (10.0 ** -(t % 3)) for k in ADAM_NUMELS] for t in range(ADAM_STEPS)]}


def _adam_fp64(inp):
    """torch/optim/adam.py:_single_tensor_adam (no weight decay, no amsgrad), evaluated in fp64."""
    b1, b2 = ADAM_BETAS
    out = []
    for i, k in enumerate(ADAM_NUMELS):
        p, m, v = inp["p"][i].double(), inp["m"][i].double(), inp["v"][i].double()
        for t in range(ADAM_STEPS):
            grad, step = inp["g"][t][i].double(), ADAM_STEP0[i] + t
            m = m + (grad - m) * (1 - b1)                                   # exp_avg.lerp_(grad, 1 - beta1)
            v = v * b2 + (1 - b2) * grad * grad                             # mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + ADAM_EPS
            p = p - (float(ADAM_LRS[i]) / (1 - b1 ** step)) * (m / denom)   # addcdiv_(exp_avg, denom, -step_size)
        out.append((p, m, v))
    return out


def _adam_hip(inp, lead, dev):
    """Three mgs_adam_step_multi calls over the 8 groups carved out of four flat buffers (parameters, gradients
    and both moments) `lead` floats in.  Returns the groups' (p, m, v) on the CPU."""
    from monogs_amd import _cabi
    offs, total = _adam_layout(lead)
    guard = torch.arange(total, dtype=torch.float32) * 0.5 - 1000.0        # a distinct value in every guard slot
    flat = {}
    for name in ("p", "m", "v"):
        host = guard.clone()
        for o, t in zip(offs, inp[name]):
            host[o:o + t.numel()] = t
        flat[name] = host.to(dev)
    flat["g"] = guard.clone().to(dev)
    in_group = torch.zeros(total, dtype=torch.bool)
    for o, k in zip(offs, ADAM_NUMELS):
        in_group[o:o + k] = True
    assert all(flat[name].data_ptr() % 16 == 0 for name in flat)
    for t in range(ADAM_STEPS):
        host = guard.clone()
        for o, gr in zip(offs, inp["g"][t]):
            host[o:o + gr.numel()] = gr
        flat["g"].copy_(host)
        arr = (_cabi.AdamGroup * len(ADAM_NUMELS))()
        for i, (o, k) in enumerate(zip(offs, ADAM_NUMELS)):
            arr[i].param, arr[i].grad = flat["p"][o:].data_ptr(), flat["g"][o:].data_ptr()
            arr[i].exp_avg, arr[i].exp_avg_sq = flat["m"][o:].data_ptr(), flat["v"][o:].data_ptr()
            arr[i].numel, arr[i].lr, arr[i].step = k, ADAM_LRS[i], ADAM_STEP0[i] + t
            for ptr in (arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq):
                assert ptr % 16 == (4 * lead) % 16      # lead = 1: no pointer is 16-byte aligned -> vec = 0
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(_cabi.lib().mgs_adam_step_multi(arr, len(ADAM_NUMELS), ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS,
                                                    stream), "mgs_adam_step_multi")
    torch.cuda.synchronize()
    res = {name: flat[name].cpu() for name in ("p", "m", "v")}
    for name in ("p", "m", "v"):      # guard elements before and after every group are untouched
        assert torch.equal(res[name][~in_group], guard[~in_group]), name
    return [tuple(res[name][o:o + k] for name in ("p", "m", "v")) for o, k in zip(offs, ADAM_NUMELS)]


def _assert_adam_close(a, b):
    for i, ((pa, ma, va), (pb, mb, vb)) in enumerate(zip(a, b)):
        assert pa.shape == pb.shape == (ADAM_NUMELS[i],)
        assert torch.allclose(pa.double(), pb.double(), rtol=2e-6, atol=1e-7), ("param", i)
        assert torch.allclose(ma.double(), mb.double(), rtol=1e-5, atol=1e-7), ("exp_avg", i)
        assert torch.allclose(va.double(), vb.double(), rtol=1e-5, atol=1e-10), ("exp_avg_sq", i)


def test_adam_scalar_path_and_group_limits(built):
    """mgs_adam_step_multi called directly with all 8 groups, numels {1, 2, 3, 5, 4099, 0, 7, 1024}, a step count
    and learning rate of its own per group, three steps:
      * carved one float into the flat buffers, so that no pointer is 16-byte aligned: the scalar path (vec = 0),
        which FusedGaussianAdam never takes because torch allocations are aligned;
      * the same groups 16-byte aligned: the float4 path with its scalar tails (numel % 4 != 0) and groups
        smaller than one float4.
    The empty group is skipped without shifting its neighbours.  Reference: the _single_tensor_adam formula in
    fp64 on the CPU, held to the bounds of test_fused_gaussian_adam_matches_torch_adam (parameters rtol 2e-6 /
    atol 1e-7, moments rtol 1e-5 with atol 1e-7 / 1e-10).  Measured on the CPU on these inputs: torch.optim.Adam
    itself in fp32 is at most 0.077 (parameters), 0.049 (exp_avg) and 0.025 (exp_avg_sq) of those bounds away
    from the fp64 values, so the fp64 reference needs no more room.  The two paths agree with each other
    to the same bounds, and every guard float between the groups is unchanged.
    Not reached: the kernel's own grid cap of 65 535 x 16 blocks of 256 threads x 4 elements, which needs more
    than 10^9 parameters."""
    dev = _dev()
    inp = _adam_inputs()
    assert len(ADAM_NUMELS) == 8 and 0 in ADAM_NUMELS and min(k for k in ADAM_NUMELS if k) < 4
    ref = _adam_fp64(inp)
    scalar = _adam_hip(inp, 1, dev)
    vector = _adam_hip(inp, 4, dev)
    _assert_adam_close(scalar, ref)
    _assert_adam_close(vector, ref)
    _assert_adam_close(scalar, vector)
