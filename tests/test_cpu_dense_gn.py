"""Dense Gauss-Newton tracking, the parts that need no GPU: the C ABI of the new entry points, the config key, and the
algebra the mode rests on - a CountSketch whose buckets hold one pixel each IS the dense system."""
import ctypes as C

import torch

NEW_SYMBOLS = ("mgs_tracking_gn_args_size", "mgs_gauss_newton_scratch_bytes", "mgs_tracking_iteration_gauss_newton",
               "mgs_tracking_iteration_gauss_newton_rgbd", "mgs_normal_equations")


def test_library_exports_the_gauss_newton_entry_points(built):
    from monogs_amd import _cabi
    raw = C.CDLL(_cabi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _cabi.EXPORTS
    L = _cabi.lib()
    assert L.mgs_tracking_gn_args_size() == C.sizeof(_cabi.TrackingGNArgs)
    # appended: the indexed list of struct sizes is the parent's (the ABI version has moved on since: an export was removed)
    assert len(_cabi.struct_mirrors()) == 26 and L.mgs_struct_size(26) == -1
    assert _cabi.ABI_VERSION == 10 and L.mgs_abi_version() == 10
    assert L.mgs_struct_size(10) == C.sizeof(_cabi.TrackingSOArgs)
    assert L.mgs_struct_size(6) == C.sizeof(_cabi.LMStepArgs)


def test_scratch_query_and_null_arguments(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    sh = _cabi.RasterShape(1000, 640, 480, 0, 1, 10000, 0.6, 0.45, 1.0)
    n = L.mgs_gauss_newton_scratch_bytes(C.byref(sh))
    # three planes, 256 workgroups x 44 sums, 256 L1 partials
    assert n >= 3 * 640 * 480 * 4 + 256 * 44 * 4 + 256 * 4
    small = _cabi.RasterShape(10, 70, 45, 0, 1, 100, 0.6, 0.45, 1.0)
    assert 3 * 70 * 45 * 4 <= L.mgs_gauss_newton_scratch_bytes(C.byref(small)) < n
    bad = _cabi.RasterShape(0, 640, 480, 0, 1, 0, 0.6, 0.45, 1.0)
    assert L.mgs_gauss_newton_scratch_bytes(C.byref(bad)) == 0
    assert L.mgs_gauss_newton_scratch_bytes(None) == 0
    a = _cabi.TrackingGNArgs()
    assert L.mgs_tracking_iteration_gauss_newton(None, None) == -1
    assert L.mgs_tracking_iteration_gauss_newton(C.byref(a), None) == -1
    assert L.mgs_tracking_iteration_gauss_newton_rgbd(C.byref(a), None, None) == -1
    assert L.mgs_normal_equations(C.byref(a), None, None) == -1


def test_exact_is_read_from_the_config():
    from monogs_amd.slam_loops import DEFAULT_CONFIG, second_order_exact
    assert second_order_exact(DEFAULT_CONFIG) is False
    assert second_order_exact({}) is False
    rgn = {"use_huber": True, "huber_delta": 0.01, "pnorm": 1}
    assert second_order_exact({"Training": {"RGN": dict(rgn, second_order={"exact": True})}}) is True
    assert second_order_exact({"Training": {"RGN": dict(rgn, second_order={"exact": False})}}) is False
    assert second_order_exact({"Training": {"RGN": dict(rgn, second_order={"repeat_dim": 1})}}) is False
    assert second_order_exact({"Training": {"RGN": dict(rgn, second_order=None)}}) is False


def test_chunk_one_partition_gives_the_exact_normal_matrix():
    """stack * sketch = H * W buckets of exactly one pixel: SJ is a signed row permutation of J, so SJ^T SJ = J^T J and
    SJ^T Sf = J^T f whatever the signs (fp64: equal to rounding of a reordered sum, 1e-13 relative).  With chunk 2 the
    cross terms of a bucket survive and the two differ - the sketch noise the dense mode removes."""
    from monogs_amd.slam_loops import gen_forward_sketch_args, normal_equations_from_rows, sketch_rows
    g = torch.Generator().manual_seed(11)
    Hh, Ww = 12, 10
    m = Hh * Ww
    J = torch.randn(m, 8, generator=g, dtype=torch.float64)
    f = torch.randn(m, generator=g, dtype=torch.float64)
    Hx, gx = normal_equations_from_rows(J, f)
    assert Hx.dtype == torch.float64 and Hx.shape == (8, 8) and gx.shape == (8,)
    assert torch.equal(Hx, Hx.T)

    def sketched(stack, sketch):
        fsa = gen_forward_sketch_args(Hh, Ww, 1, stack, sketch, "cpu", generator=g)
        idx = fsa["sketch_indices"][0].reshape(stack, m).long()                       # [stack, m], -1 = not in this stack
        flat = torch.where(idx >= 0, idx + sketch * torch.arange(stack).view(-1, 1), idx).amax(0)
        SJ, Sf = sketch_rows(J, f, flat, fsa["rand_weights"][0].reshape(-1), stack * sketch)
        return fsa["chunk_size"], SJ, Sf

    chunk, SJ, Sf = sketched(8, 15)
    assert chunk == 1 and bool((SJ.abs().amax(1) > 0).all())
    assert float((SJ.T @ SJ - Hx).abs().max()) <= 1e-13 * float(Hx.abs().max())
    assert float((SJ.T @ Sf - gx).abs().max()) <= 1e-13 * float(gx.abs().max())
    chunk, SJ, Sf = sketched(4, 15)
    assert chunk == 2
    assert float((SJ.T @ SJ - Hx).abs().max()) > 1e-3 * float(Hx.abs().max())


def test_identity_sketch_args_cover_every_pixel_once():
    """The row harvester's passes: pass k owns the pixels [2048 k, 2048 (k + 1)), ids 0 .. 2047, -1 elsewhere; the
    exposure table's rows / cols name the same pixels; the ragged last pass has no pixel past H * W."""
    from monogs_amd.slam_loops import IDENTITY_PASS_PIXELS, identity_sketch_args
    Hh, Ww = 45, 70                                          # 3150 pixels: two passes, the second ragged
    m = Hh * Ww
    fsa = identity_sketch_args(Hh, Ww, "cpu")
    P = fsa["repeat_dim"]
    assert IDENTITY_PASS_PIXELS == 2048 and P == 2 and fsa["stack_dim"] == 1 and fsa["sketch_dim"] == 2048
    assert IDENTITY_PASS_PIXELS * 6 * 4 <= 64 * 1024         # the bucket table of one pass fits in LDS
    idx = fsa["sketch_indices"].reshape(P, m).long()
    assert int((idx >= 0).sum()) == m and bool(((idx >= 0).sum(0) == 1).all())
    for k in range(P):
        own = torch.nonzero(idx[k] >= 0).squeeze(1)
        assert int(own.min()) == 2048 * k and int(own.max()) == min(2048 * (k + 1), m) - 1
        assert torch.equal(idx[k, own], own - 2048 * k)
        rows, cols = fsa["rand_indices_row"][k, 0, :, 0].long(), fsa["rand_indices_col"][k, 0, :, 0].long()
        assert torch.equal((rows * Ww + cols)[: own.numel()], own)
    assert bool((fsa["rand_weights"] == 1).all())
    assert fsa["sketch_dtau"].shape == (1, 2048, 6) and fsa["sketch_dexposure"].shape == (1, 2048, 2)
