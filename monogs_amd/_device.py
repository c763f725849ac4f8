"""What the device drivers of the mesh pipeline share (mesh_clean, mesh_eval, mesh_render and the extraction of tsdf):
the scratch buffers kept between calls, the stream and pointer arguments of the C ABI, the validators of their tensor
arguments, and the tail of a compaction - allocate the outputs from the counts read on the host, emit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _cabi

_SCRATCH_SLOTS = 4
_scratch = {}          # kind -> {(device, sizes): (scratch bytes, counts | None)}; the last _SCRATCH_SLOTS of each kind


def workspace(kind, dev, sizes, nbytes_fn, too_large, counts=0):
    """(scratch bytes, counts): the uint8 scratch of nbytes_fn(*sizes) bytes and, with `counts`, a zeroed int32 record of
    that length, kept for the next call of this kind on this device with these sizes.  nbytes_fn returns 0 for sizes
    the library refuses: ValueError(too_large)."""
    slots = _scratch.setdefault(kind, {})
    key = (str(dev),) + tuple(sizes)
    ws = slots.pop(key, None)
    if ws is None:
        nbytes = int(nbytes_fn(*sizes))
        if nbytes == 0:
            raise ValueError(too_large)
        ws = (torch.empty(nbytes, dtype=torch.uint8, device=dev),
              torch.zeros(counts, dtype=torch.int32, device=dev) if counts else None)
        while len(slots) >= _SCRATCH_SLOTS:
            slots.pop(next(iter(slots)))
    slots[key] = ws          # most recently used last
    return ws


def stream_ptr(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ptr(t):
    return t.data_ptr() if t.numel() else None


def device_rows(t, what, name, mirrors, dtype=None, dev=None):
    """The [n,3] tensor `t` on the GPU (on `dev` if given), detached, contiguous and of `dtype` if given; `mirrors` names
    what runs off the GPU instead."""
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (HIP kernels, gfx950); the mirrors {mirrors} run anywhere")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: {name} must be on {dev}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: {name} must be [n,3], got {tuple(t.shape)}")
    if t.shape[0] > _cabi.MESH_EVAL_MAX_ITEMS:
        raise ValueError(f"{what}: {name} has {t.shape[0]} rows: 3 n must stay below 2^31")
    return t if dtype is None else t.detach().to(dtype).contiguous()


def device_colors(colors, what, V, dev):
    """colors [V,3] on `dev` as contiguous fp32, or None."""
    if colors is None:
        return None
    if not torch.is_tensor(colors) or colors.device != dev or tuple(colors.shape) != (V, 3):
        raise ValueError(f"{what}: colors must be [{V},3] on the device of faces")
    return colors.detach().to(torch.float32).contiguous()


def emit_compacted(args, emit_fn, what, verts, colors, V2, F2):
    """(verts [V2,3] f32, faces [F2,3] i32, colors [V2,3] f32 | None): the outputs of a compaction whose counts V2, F2
    were read on the host, written by `emit_fn` (mgs_mesh_clean_emit, mgs_mesh_cull_emit) from its `args`."""
    dev = verts.device
    out_v = torch.empty(V2, 3, device=dev)
    out_f = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    out_c = None if colors is None else torch.empty(V2, 3, device=dev)
    args.out_num_verts, args.out_num_faces = V2, F2
    if V2:
        args.verts, args.out_verts = verts.data_ptr(), out_v.data_ptr()
        if colors is not None:
            args.colors, args.out_colors = colors.data_ptr(), out_c.data_ptr()
    if F2:
        args.out_faces = out_f.data_ptr()
    _cabi.check(emit_fn(C.byref(args), stream_ptr(dev)), what)
    return out_v, out_f, out_c


def compact_numpy(v, f, col, vkeep, fkeep):
    """(verts, faces i32, colors | None) of the mirrors: the kept vertices and faces in their order, the faces
    re-indexed by the running count of kept vertices."""
    new_index = np.cumsum(vkeep) - 1
    out_f = new_index[f[fkeep]].astype(np.int32).reshape(-1, 3)
    return v[vkeep], out_f, (None if col is None else col[vkeep])
