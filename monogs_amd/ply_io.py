"""The Gaussian map as a PLY file, in the layout of GaussianModel.save_ply / load_ply of the reference
(gaussian_splatting/scene/gaussian_model.py:314-362, 379-470), which is what 3DGS viewers read:

    ply / format binary_little_endian 1.0 / element vertex N / property float <name> ... / end_header
    N rows of little-endian fp32 in the order of construct_list_of_attributes:
    x y z  nx ny nz (zero)  f_dc_*  f_rest_*  opacity  scale_*  rot_*

f_dc and f_rest are stored channel-major: the [N,K,3] parameter is written as transpose(1, 2).flatten(1), so f_rest_j
is coefficient j % (K - 1) of channel j // (K - 1).  Every value is the RAW parameter (log scale, opacity logit,
un-normalised quaternion).  An isotropic model has the single column scale_0.

write_mesh_ply / read_mesh_ply hold the triangle mesh of monogs_amd.tsdf (DESIGN.md "Mesh export"): vertices
x y z (fp32), optionally nx ny nz (fp32), red green blue (uchar), faces `property list uchar int vertex_indices`, binary
little-endian.

Free functions on plain tensors, no GPU needed.  `plyfile` is not used: the writer emits the bytes above itself, so the
agreement with a file plyfile would write is by the PLY specification, not by comparison."""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np
import torch


def ply_attribute_names(n_dc: int, n_rest: int, n_scale: int, n_rot: int = 4) -> List[str]:
    """construct_list_of_attributes (:314-326)."""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names.append("opacity")
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def write_gaussian_ply(path: str, xyz, features_dc, features_rest, opacity, scaling, rotation) -> None:
    """xyz [N,3], features_dc [N,1,3], features_rest [N,K-1,3], opacity [N,1], scaling [N,3] or [N,1], rotation [N,4].
    The rows are concatenated on the tensors' device and copied to the host once."""
    t = lambda a: a.detach().to(torch.float32)
    xyz = t(xyz)
    n = int(xyz.shape[0])
    f_dc = t(features_dc).transpose(1, 2).flatten(1)
    f_rest = t(features_rest).transpose(1, 2).flatten(1)
    cols = (xyz, torch.zeros_like(xyz), f_dc, f_rest, t(opacity).reshape(n, 1), t(scaling).flatten(1),
            t(rotation).flatten(1))
    rows = torch.cat(cols, dim=1).contiguous().cpu().numpy().astype("<f4", copy=False)
    names = ply_attribute_names(f_dc.shape[1], f_rest.shape[1], cols[5].shape[1], cols[6].shape[1])
    assert rows.shape == (n, len(names))
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    header += [f"property float {name}" for name in names]
    header.append("end_header")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rows.tobytes())


MESH_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
MESH_FACE_DTYPE = np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])


MESH_VERTEX_NORMAL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                     ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def mesh_ply_header(num_verts: int, num_faces: int, normals: bool = False) -> str:
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {num_verts}\n"
            "property float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "") +
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {num_faces}\n"
            "property list uchar int vertex_indices\n"
            "end_header\n")


def quantise_colors(colors) -> np.ndarray:
    """fp32 colours in [0, 1] -> uint8, rounded to nearest (NaN gives 0)."""
    c = torch.as_tensor(colors).detach().to(torch.float32)
    c = torch.nan_to_num(c, nan=0.0).clamp(0.0, 1.0)
    return torch.floor(c * 255.0 + 0.5).to(torch.uint8).cpu().numpy()


def write_mesh_ply(path: str, verts, faces, colors=None, normals=None) -> None:
    """A triangle mesh as binary little-endian PLY: per vertex x y z (fp32) and red green blue (uint8; fp32 colours are
    quantised by quantise_colors, None is white), per face a uchar count of 3 and three int32 vertex indices.  With
    `normals` [V,3] the vertex element is x y z nx ny nz red green blue, the order MeshLab and Open3D write; without,
    the file is what it was before there were normals.  The tensors are copied to the host once each."""
    v = torch.as_tensor(verts).detach().to(torch.float32).cpu().numpy().reshape(-1, 3)
    f = torch.as_tensor(faces).detach().to(torch.int32).cpu().numpy().reshape(-1, 3)
    if colors is None:
        c = np.full((v.shape[0], 3), 255, np.uint8)
    else:
        c = torch.as_tensor(colors)
        c = c.detach().cpu().numpy() if c.dtype == torch.uint8 else quantise_colors(c)
        c = c.reshape(-1, 3)
    if c.shape[0] != v.shape[0]:
        raise ValueError(f"{c.shape[0]} colours for {v.shape[0]} vertices")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("face index out of range")
    vr = np.empty(v.shape[0], MESH_VERTEX_DTYPE if normals is None else MESH_VERTEX_NORMAL_DTYPE)
    if normals is not None:
        n = torch.as_tensor(normals).detach().to(torch.float32).cpu().numpy().reshape(-1, 3)
        if n.shape[0] != v.shape[0]:
            raise ValueError(f"{n.shape[0]} normals for {v.shape[0]} vertices")
        vr["nx"], vr["ny"], vr["nz"] = n[:, 0], n[:, 1], n[:, 2]
    vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
    vr["red"], vr["green"], vr["blue"] = c[:, 0], c[:, 1], c[:, 2]
    fr = np.empty(f.shape[0], MESH_FACE_DTYPE)
    fr["count"] = 3
    fr["vertex_indices"] = f
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(mesh_ply_header(v.shape[0], f.shape[0], normals is not None).encode("ascii"))
        fh.write(vr.tobytes())
        fh.write(fr.tobytes())


def read_mesh_ply(path: str, with_normals: bool = False):
    """The inverse of write_mesh_ply: (verts [V,3] f32, faces [F,3] i32, colors [V,3] uint8) as CPU tensors, of a file
    with or without normals; `with_normals` adds a fourth element, normals [V,3] f32 or None when the file has none.
    Only the two layouts write_mesh_ply emits are read."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = blob[:end].decode("ascii").split("\n")
    body = end + len(b"end_header\n")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    if "vertex" not in counts or "face" not in counts:
        raise ValueError(f"{path}: a vertex and a face element are expected")
    nv, nf = counts["vertex"], counts["face"]
    header = blob[:body].decode("ascii")
    has_normals = header == mesh_ply_header(nv, nf, True)
    if not has_normals and header != mesh_ply_header(nv, nf):
        raise ValueError(f"{path}: not the layout write_mesh_ply emits")
    vertex_dtype = MESH_VERTEX_NORMAL_DTYPE if has_normals else MESH_VERTEX_DTYPE
    need = nv * vertex_dtype.itemsize + nf * MESH_FACE_DTYPE.itemsize
    if len(blob) - body < need:
        raise ValueError(f"{path}: {need} bytes of data expected, file too short")
    vr = np.frombuffer(blob, vertex_dtype, count=nv, offset=body)
    fr = np.frombuffer(blob, MESH_FACE_DTYPE, count=nf, offset=body + nv * vertex_dtype.itemsize)
    if nf and (fr["count"] != 3).any():
        raise ValueError(f"{path}: only triangles are read")
    verts = np.stack([vr["x"], vr["y"], vr["z"]], 1).astype(np.float32)
    cols = np.stack([vr["red"], vr["green"], vr["blue"]], 1).astype(np.uint8)
    out = (torch.from_numpy(verts.reshape(nv, 3)), torch.from_numpy(fr["vertex_indices"].astype(np.int32).reshape(nf, 3)),
           torch.from_numpy(cols.reshape(nv, 3)))
    if not with_normals:
        return out
    if not has_normals:
        return out + (None,)
    return out + (torch.from_numpy(np.stack([vr["nx"], vr["ny"], vr["nz"]], 1).astype(np.float32).reshape(nv, 3)),)


def read_gaussian_ply(path: str) -> Dict[str, torch.Tensor]:
    """The inverse of write_gaussian_ply: CPU float tensors xyz, features_dc [N,1,3], features_rest [N,K-1,3],
    opacity [N,1], scaling, rotation.  Properties are found by name (f_rest_*, scale_*, rot_* in index order), as
    load_ply (:379-470) finds them."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = blob[:end].decode("ascii").split("\n")
    body = end + len(b"end_header\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian 1.0 is read")
    n, names, in_vertex, seen_vertex = 0, [], False, False
    for ln in lines:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "element":
            if tok[1] != "vertex" and not seen_vertex:
                raise ValueError(f"{path}: element {tok[1]} before the vertex element")
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                n, seen_vertex = int(tok[2]), True
        elif tok[0] == "property" and in_vertex:
            if tok[1] not in ("float", "float32"):
                raise ValueError(f"{path}: property {tok[-1]} is {tok[1]}, not float")
            names.append(tok[-1])
    if not seen_vertex:
        raise ValueError(f"{path}: no vertex element")
    width = len(names)
    if len(blob) - body < 4 * n * width:
        raise ValueError(f"{path}: {n} x {width} floats expected, file too short")
    rows = np.frombuffer(blob, dtype="<f4", count=n * width, offset=body).reshape(n, width).astype(np.float32)
    col = {name: i for i, name in enumerate(names)}

    def numbered(prefix):
        found = [nm for nm in names if nm.startswith(prefix)]
        return [col[nm] for nm in sorted(found, key=lambda s: int(s.split("_")[-1]))]

    def take(idx):
        return torch.from_numpy(np.ascontiguousarray(rows[:, idx]))

    for need in ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"):
        if need not in col:
            raise ValueError(f"{path}: property {need} is missing")
    rest = numbered("f_rest_")
    if len(rest) % 3:
        raise ValueError(f"{path}: {len(rest)} f_rest properties are no multiple of 3")
    return {
        "xyz": take([col["x"], col["y"], col["z"]]),
        "features_dc": take([col["f_dc_0"], col["f_dc_1"], col["f_dc_2"]]).reshape(n, 3, 1).transpose(1, 2).contiguous(),
        "features_rest": take(rest).reshape(n, 3, len(rest) // 3).transpose(1, 2).contiguous(),
        "opacity": take([col["opacity"]]),
        "scaling": take(numbered("scale_")),
        "rotation": take(numbered("rot_")),
    }
