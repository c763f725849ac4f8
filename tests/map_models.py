"""GaussianModel-shaped fixtures shared by the map-maintenance tests (test_raster_gpu.py,
test_gpu_map_update_sizes.py): a seeded model with its optimiser on the device, and its whole
per-Gaussian state as CPU tensors under the names oracle/map_update_ref.py uses."""
import torch
import torch.nn as nn


class _Model:
    """GaussianModel-shaped holder (gaussian_model.py:30-52, :247-285)."""
    percent_dense = 0.01


ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "scaling": "_scaling", "rotation": "_rotation"}


def _make_model(n, dev, seed, fused, rest=0):
    from monogs_amd.map_update import FusedGaussianAdam
    g = torch.Generator().manual_seed(seed)
    cpu = {
        "xyz": torch.randn(n, 3, generator=g),
        "f_dc": torch.randn(n, 1, 3, generator=g),
        "f_rest": torch.randn(n, rest, 3, generator=g),
        "opacity": torch.randn(n, 1, generator=g) * 2.0,
        "scaling": torch.randn(n, 3, generator=g) * 0.7 - 3.0,
        "rotation": torch.randn(n, 4, generator=g),
    }
    m = _Model()
    attr = dict(ATTR)
    groups = []
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 1e-3, "rotation": 1e-3}
    for name, t in cpu.items():
        p = nn.Parameter(t.clone().to(dev))
        setattr(m, attr[name], p)
        groups.append({"params": [p], "lr": lrs[name], "name": name})
    m.optimizer = FusedGaussianAdam(groups, lr=0.0, eps=1e-15) if fused else torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    m.xyz_gradient_accum = (torch.rand(n, 1, generator=g) * 4e-4).to(dev)
    m.denom = torch.randint(0, 3, (n, 1), generator=g).float().to(dev)      # zeros -> NaN grads
    m.max_radii2D = torch.rand(n, generator=g).to(dev) * 30
    m.unique_kfIDs = torch.randint(0, 9, (n,), generator=g).int().to(dev)
    m.n_obs = torch.randint(0, 5, (n,), generator=g).int().to(dev)
    return m, cpu, attr


def _state_of(m, attr, cpu_names):
    st = {}
    for name, a in attr.items():
        p = getattr(m, a)
        st[name] = p.detach().cpu().clone()
        s = m.optimizer.state.get(p)
        st["exp_avg_" + name] = s["exp_avg"].cpu().clone()
        st["exp_avg_sq_" + name] = s["exp_avg_sq"].cpu().clone()
    st["kf"], st["n_obs"] = m.unique_kfIDs.cpu().clone(), m.n_obs.cpu().clone()
    st["grad_accum"], st["denom"] = m.xyz_gradient_accum.cpu().clone(), m.denom.cpu().clone()
    st["max_radii"] = m.max_radii2D.cpu().clone()
    return st
