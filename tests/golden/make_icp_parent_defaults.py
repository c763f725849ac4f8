"""Writes icp_parent_defaults.npz: what the mirrors of the frame-to-model ICP returned on the commit BEFORE the RGB-D rows
were added - record, history, D and T_w2c of two schedules, the sums and counts of one rows call, and the keys of the result
dicts.  test_cpu_icp_rgbd.py::test_defaults_are_the_old_path holds the present mirrors to these bytes.  Run it with the root
of a checkout of that commit and the output path:  python make_icp_parent_defaults.py <root> icp_parent_defaults.npz"""
import sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, root + '/tests')
import numpy as np, torch
import icp_cases as IC
from monogs_amd import icp
out = {}
r = icp.align_numpy(IC.model_planes(), IC.frame_depth(), IC.INTR, np.eye(4, dtype=np.float32), levels=((2, 2), (1, 3)), sensor_normal=IC.sensor_normal())
keys = sorted(r)
out["keys"] = np.array(",".join(keys)); out["info_keys"] = np.array(",".join(sorted(r["info"])))
for k in ("record", "history", "D", "T_w2c"):
    out["recovery_" + k] = r[k]
model, depth, kw, status = IC.status_cases()["degenerate"]
r = icp.align_numpy(model, depth, IC.INTR, np.eye(4, dtype=np.float32), levels=((2, 2), (1, 3)), **kw)
for k in ("record", "history", "D", "T_w2c"):
    out["degenerate_" + k] = r[k]
s, c = icp.icp_rows_numpy(IC.model_planes(), IC.patched_depth(), IC.sensor_normal(), np.eye(4)[:3], IC.INTR, stride=3)
out["rows_sums"], out["rows_counts"] = s, c
np.savez_compressed(sys.argv[2], **out)
print(keys, out["info_keys"])
