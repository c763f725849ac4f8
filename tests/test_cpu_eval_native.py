"""Host side of the native evaluation tail: the C ABI additions and their ctypes mirrors, the PLY map export against
the PLY specification written out here (plyfile is not available: agreement with a file it would write is unpinned,
DESIGN.md §2) plus the round trip, and eval_rendering_native's selection of views against eval_metrics.eval_rendering's."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn as nn

from monogs_amd import _cabi, eval_metrics, eval_native, ply_io
from monogs_amd.gaussian_model import GaussianModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_mirror_agree(built):
    with open(os.path.join(ROOT, "include", "monogs_raster.h"), encoding="utf-8") as fh:
        header = fh.read()
    declared = set(re.findall(r"^\w[\w ]*\b(mgs_eval_\w+)\(", header, flags=re.M))
    assert declared == {"mgs_eval_score", "mgs_eval_score_partial_count", "mgs_eval_score_args_size",
                        "mgs_eval_view_args_size", "mgs_eval_view"}
    assert declared <= set(_cabi.EXPORTS)
    L = _cabi.lib()
    assert L.mgs_eval_score_args_size() == C.sizeof(_cabi.EvalScoreArgs) == 8 * 4 + 9 * 8
    assert L.mgs_eval_view_args_size() == C.sizeof(_cabi.EvalViewArgs) == (
        C.sizeof(_cabi.ForwardArgs) + 8 + C.sizeof(_cabi.EvalScoreArgs) + 8)
    assert L.mgs_abi_version() == _cabi.ABI_VERSION
    for name, value in re.findall(r"#define MGS_(EVAL_\w+) (\d+)", header):
        assert getattr(_cabi, name) == int(value), name
    # 7 partial sums per workgroup - one per 32x16 tile and channel up to 512 of them - and the ticket
    assert L.mgs_eval_score_partial_count(480, 640) == 7 * 512 + 1
    assert L.mgs_eval_score_partial_count(33, 65) == 7 * 3 * 3 * 3 + 1
    assert L.mgs_eval_score_partial_count(0, 640) == -1 and L.mgs_eval_score_partial_count(480, -1) == -1
    assert L.mgs_eval_score_partial_count(1 << 20, 1 << 20) == -1          # more tiles than an int indexes
    assert L.mgs_eval_score_partial_count(2 ** 31 - 1, 2 ** 31 - 1) == -1  # and no overflow on the way there
    a = _cabi.EvalScoreArgs()                                              # refused before anything is dereferenced
    a.height = a.width = 1 << 20
    a.num_rows = 1
    a.image = a.gt = a.partial = a.table = 64
    assert L.mgs_eval_score(C.byref(a), None) == -3


def _model(n, sh_degree, isotropic=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    gm = GaussianModel(sh_degree, device="cpu", isotropic=isotropic)
    K = (sh_degree + 1) ** 2
    r = lambda *s: nn.Parameter(torch.randn(*s, generator=g))
    gm._xyz, gm._features_dc, gm._features_rest = r(n, 3), r(n, 1, 3), r(n, K - 1, 3)
    gm._opacity, gm._scaling, gm._rotation = r(n, 1), r(n, 1 if isotropic else 3), r(n, 4)
    return gm


def test_ply_bytes_follow_the_specification(tmp_path):
    gm = _model(2, 1)
    path = str(tmp_path / "a" / "point_cloud.ply")
    gm.save_ply(path)
    names = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(9)]
             + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    header = "ply\n" + "format binary_little_endian 1.0\n" + "element vertex 2\n"
    for nm in names:
        header += f"property float {nm}\n"
    header += "end_header\n"
    body = b""
    xyz, dc, rest, opa, sca, rot = (getattr(gm, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity",
                                                                      "_scaling", "_rotation"))
    for i in range(2):
        row = [float(v) for v in xyz[i]] + [0.0, 0.0, 0.0]
        row += [float(dc[i, 0, c]) for c in range(3)]
        # channel-major: the three coefficients of red, then of green, then of blue
        row += [float(rest[i, k, c]) for c in range(3) for k in range(3)]
        row += [float(opa[i, 0])] + [float(v) for v in sca[i]] + [float(v) for v in rot[i]]
        assert len(row) == len(names) == 26
        body += struct.pack("<" + "f" * len(row), *row)
    with open(path, "rb") as fh:
        assert fh.read() == header.encode("ascii") + body


@pytest.mark.parametrize("n,sh_degree,isotropic", ((5, 0, False), (7, 3, False), (4, 0, True), (0, 1, False)))
def test_ply_round_trip_is_exact(tmp_path, n, sh_degree, isotropic):
    gm = _model(n, sh_degree, isotropic, seed=n)
    path = eval_native.save_gaussians(gm, str(tmp_path / "run"), 7, final=(n == 5))
    want = os.path.join(str(tmp_path / "run"), "point_cloud", "final" if n == 5 else "iteration_7", "point_cloud.ply")
    assert path == want and os.path.isfile(want)
    back = GaussianModel(sh_degree, device="cpu")
    back.load_ply(path)
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        a, b = getattr(gm, attr).detach(), getattr(back, attr)
        assert isinstance(b, nn.Parameter) and b.requires_grad and b.is_contiguous()
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.detach().view(torch.int32)), attr
    assert back.isotropic == isotropic and back.active_sh_degree == sh_degree and len(back) == n
    assert back.max_radii2D.shape == (n,) and back.unique_kfIDs.shape == (n,) and back.n_obs.dtype == torch.int32
    back.init_lr(6.0)
    back.training_setup()
    assert [g["name"] for g in back.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert eval_native.save_gaussians(gm, None, 0) is None


def test_load_ply_checks_the_f_rest_count(tmp_path):
    path = str(tmp_path / "m.ply")
    _model(3, 1).save_ply(path)
    with pytest.raises(ValueError, match="f_rest"):
        GaussianModel(2, device="cpu").load_ply(path)
    got = ply_io.read_gaussian_ply(path)
    assert got["features_rest"].shape == (3, 3, 3)


class _Recorder:
    def __init__(self):
        self.rows, self.depths, self.began, self.done = [], [], 0, 0

    def begin(self):
        self.began += 1

    def score(self, view, gt_image, gt_depth=None, apply_exposure=False):
        assert not apply_exposure and float(gt_image) == view     # dataset[idx][0] of the scored frame
        self.rows.append(view)
        self.depths.append(gt_depth)
        return len(self.rows) - 1

    def finish(self):
        """Per-view arrays of the views scored since begin(): psnr 20 + the frame's index, ssim 0.5, depth_l1 0.25."""
        new = slice(self.done, len(self.rows))
        self.done = len(self.rows)
        psnr = np.array([20.0 + v for v in self.rows[new]])
        return {"psnr": psnr, "ssim": np.full(psnr.shape, 0.5),
                "depth_l1": np.array([np.nan if d is None else 0.25 for d in self.depths[new]])}


@pytest.mark.parametrize("n_frames", (1, 2, 6, 11))
@pytest.mark.parametrize("with_depth", (False, True))
@pytest.mark.parametrize("interval", (5, 2))         # 5: the reference's; with keyframes 0 and 5 it leaves nothing below 11 frames
def test_selection_rule_is_eval_renderings(tmp_path, n_frames, with_depth, interval):
    frames = list(range(n_frames))                           # a "frame" is its index
    dataset = [(torch.tensor(float(i)), torch.ones(2, 2) if with_depth else None, None) for i in range(n_frames)]
    kf = [0, 5]
    seen = []

    def render_fn(frame, gaussians, pipe, background):
        seen.append(frame)
        return {"render": torch.full((3, 4, 4), 0.5)}

    class _DS:
        def __getitem__(self, i):
            return torch.full((3, 4, 4), 0.25), None, None

    want = eval_metrics.eval_rendering(frames, None, _DS(), render_fn, None, None, kf, save_dir=str(tmp_path / "a"),
                                       interval=interval)
    rec = _Recorder()
    got = eval_native.eval_rendering_native(frames, None, dataset, None, None, kf, save_dir=str(tmp_path / "b"),
                                            interval=interval, evaluator=rec)
    assert rec.rows == seen == [i for i in range(0, n_frames - 1, interval) if i not in kf]
    assert bool(seen) == (interval == 2 and n_frames >= 6)
    assert got["mean_lpips"] is None and set(want) <= set(got)
    assert ("mean_depth_l1" in got) == (with_depth and bool(seen))
    if seen:
        assert rec.began == 1 and got["mean_psnr"] == 20.0 + np.mean(seen) and got["mean_ssim"] == 0.5
        # in batches of two views: as many begin / finish pairs as batches, the same means
        rec2 = _Recorder()
        got2 = eval_native.eval_rendering_native(frames, None, dataset, None, None, kf, interval=interval, evaluator=rec2,
                                                 chunk=2)
        assert rec2.rows == seen and rec2.began == (len(seen) + 1) // 2 and got2 == got
    else:
        assert rec.began == 0 and np.isnan(got["mean_psnr"]) and np.isnan(got["mean_ssim"])
    for sub in ("a", "b"):
        assert os.path.isfile(os.path.join(str(tmp_path / sub), "psnr", "final", "final_result.json"))
    with open(os.path.join(str(tmp_path / "b"), "psnr", "final", "final_result.json"), encoding="utf-8") as fh:
        stored = json.load(fh)
    assert stored.keys() == got.keys() and stored["mean_lpips"] is None


def test_scores_from_records_edge_values():
    t = np.zeros((3, _cabi.EVAL_RECORD_DOUBLES))
    t[0, [_cabi.EVAL_SSE, _cabi.EVAL_N_MASK]] = 0.5, 50.0      # 10 log10(100) = 20 dB
    t[1, _cabi.EVAL_N_MASK] = 10.0                              # x == y on the mask: inf
    s = eval_native.scores_from_records(t, 100)                 # row 2: an empty mask: nan
    assert s["psnr"][0] == pytest.approx(20.0, abs=1e-12) and np.isposinf(s["psnr"][1]) and np.isnan(s["psnr"][2])
    assert np.isnan(s["depth_l1"]).all()


def test_the_evaluator_refuses_the_cpu():
    with pytest.raises(RuntimeError, match="GPU only"):
        eval_native.NativeEvaluator(None, torch.zeros(3), 4, 4, "cpu")
