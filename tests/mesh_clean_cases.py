"""Meshes shared by test_cpu_mesh_clean.py and test_gpu_mesh_clean.py, and two independent statements of the
components (SciPy's, a plain union-find).

Sizes.  Every kernel of the clean-up works in blocks of 256 vertices / faces; the one-workgroup scan takes 1024 block
totals per trip (262 144 items); the select's three histogram levels split a face count at bits 10 and 21.
  strip(4099)      one past 16 blocks; long parent chains, hooks in both directions (identity, reversed, random order)
  floaters         counts 4580 / 308 / 144 / 144 / 48: the level-2 bucket separates 4580, level 3 the rest, with a tie
  ties             40 + 6 + 3 clusters of 1 / 5 / 9 faces: cuts inside and at the ends of both tie groups
  two_scan_trips   262 250 vertices and more than 262 144 faces: 1025 block totals, i.e. a second trip of the scan for
                   the ties, the vertices and the faces; single triangles on both sides of the trip boundary tie
  level1           a cluster of 2^21 + 1 faces: the select's first level (bits 31..21) separates it from the rest"""
import numpy as np

FLOATER_SPHERES = (((11.3, 11.6, 12.2), 6.4), ((2.4, 2.6, 2.5), 1.3), ((20.5, 3.4, 19.6), 1.7),
                   ((3.5, 20.4, 4.4), 1.3), ((20.3, 20.6, 3.5), 0.8))
FLOATER_DIMS = (24, 24, 24)
FLOATER_ORIGIN, FLOATER_VOXEL = (0.0, 0.0, 0.0), 1.0
FLOATER_CLUSTERS = (4580, 308, 144, 144, 48)          # faces, as extract_mesh_numpy and SciPy give them
FLOATER_VF, BIG_ONLY_VF = (2622, 5224), (2292, 4580)


def floater_planes(big_only=False):
    """(tsdf, weight, color) [24,24,24]: clip(min over the spheres of (|p - c| - r) / 3, -1, 1), weight 1, the colour a
    function of the position."""
    nx, ny, nz = FLOATER_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    sdf = np.full(i.shape, np.inf)
    for c, r in FLOATER_SPHERES[:1] if big_only else FLOATER_SPHERES:
        sdf = np.minimum(sdf, np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r)
    tsdf = np.clip(sdf / 3.0, -1.0, 1.0).astype(np.float32)
    color = np.stack([i / 23.0, j / 23.0, 0.5 + 0.5 * np.sin(0.3 * k)]).astype(np.float32)
    return tsdf, np.ones_like(tsdf), color


_floater_cache = {}


def floater_mesh(big_only=False):
    """extract_mesh_numpy of the floater volume (computed once; callers must not write into it)."""
    if big_only not in _floater_cache:
        from monogs_amd.tsdf import extract_mesh_numpy
        _floater_cache[big_only] = extract_mesh_numpy(*floater_planes(big_only), FLOATER_ORIGIN, FLOATER_VOXEL, 1.0)
    return _floater_cache[big_only]


def _attributes(V, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.random((V, 3)).astype(np.float32)


def _strip_faces(p):
    p = np.asarray(p, np.int64)
    return np.stack([p[:-2], p[1:-1], p[2:]], 1).astype(np.int32)


def strip(n=4099, perm="identity", seed=5):
    if perm == "identity":
        p = np.arange(n)
    elif perm == "reversed":
        p = np.arange(n)[::-1]
    else:
        p = np.random.default_rng(seed).permutation(n)
    return _attributes(n, 1) + (_strip_faces(p),)


def star(n=3000):
    """One vertex (index 7, so not the label) in every face."""
    V = 2 * n + 8
    others = np.delete(np.arange(V), 7)[:2 * n].reshape(n, 2)
    faces = np.concatenate([others[:, :1], np.full((n, 1), 7), others[:, 1:]], 1).astype(np.int32)
    return _attributes(V, 2) + (faces,)


def interleaved():
    """Two strips, on the even (1001 faces) and on the odd (1000 faces) vertex indices."""
    even, odd = 2 * np.arange(1003), 2 * np.arange(1002) + 1
    faces = np.concatenate([_strip_faces(even), _strip_faces(odd)])
    faces = faces[np.random.default_rng(3).permutation(len(faces))]
    return _attributes(2006, 3) + (faces,)


def _fan(first, faces):
    """`faces` triangles over faces + 2 consecutive vertices from `first` on."""
    return _strip_faces(np.arange(first, first + faces + 2))


def ties():
    """40 single triangles, six clusters of 5 faces and three of 9, interleaved in label order."""
    sizes = [1] * 40 + [5] * 6 + [9] * 3
    order = np.random.default_rng(11).permutation(len(sizes))
    blocks, first = [], 0
    for s in np.asarray(sizes)[order]:
        blocks.append(_fan(first, int(s)))
        first += int(s) + 2
    faces = np.concatenate(blocks)
    faces = faces[np.random.default_rng(12).permutation(len(faces))]
    return _attributes(first, 4) + (faces.astype(np.int32),)


TIES_KEEP = (1, 3, 4, 6, 9, 10, 49, 50)
TIES_MIN = (0, 2, 5, 6)


def odd():
    """Degenerate and duplicate faces, unreferenced vertices in the middle and at the end."""
    faces = np.array([[0, 0, 1], [1, 2, 2], [4, 5, 6], [4, 5, 6], [6, 5, 4], [9, 9, 9], [10, 12, 10], [12, 13, 14],
                      [16, 15, 15], [15, 16, 16], [2, 1, 0]], np.int32)
    return _attributes(20, 6) + (faces,)           # 3, 7, 8, 11, 17, 18, 19 are named by no face


def empty(V):
    return _attributes(V, 7) + (np.zeros((0, 3), np.int32),)


def disjoint_triangles(n, first=0):
    return (first + np.arange(3 * n, dtype=np.int64).reshape(n, 3)).astype(np.int32)


def two_scan_trips():
    """5 single triangles, a strip over 262 160 vertices, 25 single triangles: V = 262 250 (1025 blocks), F = 262 188
    (1025 blocks).  The strip ends past vertex 262 144, the second group of triangles lies in the scan's second trip."""
    n = 262160
    faces = np.concatenate([disjoint_triangles(5), _strip_faces(np.arange(15, 15 + n)), disjoint_triangles(25, 15 + n)])
    V = 15 + n + 75
    v = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    return v, (v * np.float32(0.5)), faces


def level1():
    """A fan of 2^21 + 1 faces around vertex 0 and a strip of 2^10 + 1 faces after it."""
    n = 2 ** 21 + 1
    rim = np.arange(1, n + 2, dtype=np.int64)
    fan = np.stack([np.zeros(n, np.int64), rim[:-1], rim[1:]], 1).astype(np.int32)
    small = _fan(n + 2, 2 ** 10 + 1)
    V = n + 2 + 2 ** 10 + 3
    v = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    return v, None, np.concatenate([small, fan])


def case(name):
    if name == "floaters":
        v, f, c = floater_mesh()
        return v, c, f
    if name.startswith("strip_"):
        return strip(perm=name[6:])
    return {"star": star, "interleaved": interleaved, "ties": ties, "odd": odd, "two_scan_trips": two_scan_trips,
            "level1": level1, "empty_v0": lambda: empty(0), "empty_f0": lambda: empty(7)}[name]()


SMALL_CASES = ("floaters", "strip_identity", "strip_reversed", "strip_random", "star", "interleaved", "ties", "odd",
               "empty_v0", "empty_f0")
LARGE_CASES = ("two_scan_trips", "level1")

# (case, keep_largest, min_faces): what the clean-up is run with
PARAMS = ([("floaters", k, m) for k, m in ((None, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (7, 0), (0, 0),
                                            (None, 145), (None, 144), (None, 309), (3, 200), (None, 5000))]
          + [(n, k, 0) for n in ("strip_identity", "strip_reversed", "strip_random", "star") for k in (None, 1)]
          + [("interleaved", k, m) for k, m in ((None, 0), (1, 0), (2, 0), (None, 1001))]
          + [("ties", k, m) for k in (None,) + TIES_KEEP for m in TIES_MIN]
          + [("odd", k, m) for k, m in ((None, 0), (1, 0), (2, 0), (3, 2), (None, 2), (None, 3))]
          + [(n, k, 0) for n in ("empty_v0", "empty_f0") for k in (None, 1)]
          + [("two_scan_trips", k, m) for k, m in ((None, 0), (1, 0), (11, 0), (28, 0), (None, 2))]
          + [("level1", k, 0) for k in (1, 2)])


def param_id(p):
    return f"{p[0]}-k{p[1]}-m{p[2]}"


# ---- independent statements of the components ------------------------------------------------------------------------
def scipy_components(V, faces):
    """(number of components, partition id per vertex) from scipy.sparse.csgraph."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = np.concatenate([f[:, 0], f[:, 1]])
    cols = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(V, V))
    return connected_components(g, directed=False)


def assert_labels_are(labels, V, partition):
    """`labels` induces the partition `partition`, and every label is the smallest index of its part."""
    labels = np.asarray(labels, np.int64)
    assert labels.shape == (V,)
    smallest = np.full(int(partition.max()) + 1 if V else 0, V, np.int64)
    np.minimum.at(smallest, partition, np.arange(V))
    assert np.array_equal(labels, smallest[partition])


def union_find_labels(V, faces):
    """A plain sequential union-find, then the smallest index per set."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[rw] = ru              # no ordering: the minimum is taken below
    roots = [find(x) for x in range(V)]
    smallest = {}
    for x, r in enumerate(roots):
        smallest.setdefault(r, x)            # x ascends: the first is the smallest
    return np.array([smallest[r] for r in roots], np.int32).reshape(V)
