"""Meshes shared by test_cpu_mesh_simplify.py and test_gpu_mesh_simplify.py, and an independent plain-Python statement
of the contract of monogs_amd/mesh_simplify.py (a dict over cell tuples, a set of frozensets).

Every case is (verts, colors | None, faces, keywords).  Sizes: every kernel works in blocks of 256 vertices / faces; the
one-workgroup scan takes 1024 block totals per trip (262 144 items); the hash tables hold the smallest power of two
>= 2 n entries.
  hand             repeated / rewound / rotated faces, duplicates that only clustering makes, faces with equal indices,
                   unreferenced vertices in the middle and at the end, negative cells, a vertex on a cell boundary, a
                   tiny negative coordinate whose fraction rounds to 1
  one_cell         every vertex in one cell: nothing is emitted
  crowd            10 000 vertices in one cell and one triangle that survives: contention on one slot and one row
  vertex_home      40 cells that share one home slot of the vertex table (and a second vertex in every fourth)
  vertex_wrap      the same with the table's LAST slot as the home: the probe wraps
  face_home/_wrap  the two for 40 label triples in the face table (and other windings of every fifth)
  two_scan_trips   263 144 vertices and 263 136 faces, kept ones on both sides of item 262 144: 1028 block totals"""
import itertools
from fractions import Fraction

import numpy as np

from monogs_amd import mesh_simplify as MS


def _colors(V, seed):
    return np.random.default_rng(seed).random((V, 3)).astype(np.float32)


def hand():
    v = np.array([[0.2, 0.2, 0.2], [0.7, 0.1, 0.3], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [9.5, 9.5, 9.5], [-0.5, 0.5, 0.5],
                  [-1.5, -0.25, 0.5], [2.0, 0.5, 0.5], [1.25, 0.75, 0.5], [0.5, 0.5, 1.5], [-1e-10, 0.5, 0.5],
                  [7.5, 7.5, 7.5], [7.25, 7.5, 7.75]], np.float32)
    f = np.array([[0, 2, 3], [0, 2, 3], [3, 2, 0], [2, 3, 0],      # a face, repeated, rewound, rotated
                  [1, 8, 3],                                       # the same three cells through other vertices
                  [0, 1, 2], [5, 5, 6], [4, 4, 4],                 # two vertices of one cell; equal indices
                  [5, 6, 7], [10, 6, 7],                           # negative cells; 10 lies in the cell of 5
                  [9, 3, 2], [7, 9, 0]], np.int32)
    c = _colors(len(v), 1)
    c[1] = (np.nan, -0.5, 1.5)                                     # NaN -> 0, clamped below and above
    return v, c, f, dict(cell=1.0, origin=(0.0, 0.0, 0.0))


HAND_INFO = dict(verts_in=13, faces_in=12, verts_out=7, faces_out=4, num_clusters=9, collapsed_faces=3, duplicate_faces=5)


def one_cell(n=300):
    rng = np.random.default_rng(2)
    v = (0.25 + 0.5 * rng.random((n, 3))).astype(np.float32)
    f = rng.integers(0, n, (2 * n, 3)).astype(np.int32)
    return v, _colors(n, 3), f, dict(cell=1.0, origin=(0.0, 0.0, 0.0))


def crowd(n=10000):
    """n vertices in the cell (0,0,0), two more in cells of their own; faces inside the crowd collapse, [5, n, n+1] stays
    and its rewound twin through another vertex of the crowd is a duplicate."""
    rng = np.random.default_rng(4)
    v = np.concatenate([rng.random((n, 3)), [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]]).astype(np.float32)
    f = np.concatenate([rng.integers(0, n, (500, 3)), [[5, n, n + 1], [n + 1, n, n - 1]]]).astype(np.int32)
    return v, _colors(n + 2, 5), f, dict(cell=1.0, origin=(0.0, 0.0, 0.0))


def _cells_with_home(count, size, home):
    """`count` distinct cells (cx, cy, 0) whose keys have the home slot `home` in a table of `size` entries."""
    out = []
    for cx, cy in itertools.product(range(-40, 40), repeat=2):
        if MS._home_slot(MS.cell_key(cx, cy, 0), size) == home:
            out.append((cx, cy, 0))
            if len(out) == count:
                return out
    raise AssertionError("not enough cells")


def vertex_collisions(wrap):
    """(case, cells, table size, home): 40 cells with one home slot, a second vertex in every fourth of them (so the
    minimum is taken in a slot reached by probing), a closed fan of faces over the cells."""
    n, extra = 40, 10
    V = n + extra
    size = MS.table_size(V)
    home = size - 1 if wrap else 5
    cells = _cells_with_home(n, size, home)
    rng = np.random.default_rng(6)
    order = rng.permutation(n)
    first = [cells[k] for k in order]
    second = [cells[k] for k in order[::4]]
    v = (np.array(second + first, np.float64) + 0.125 + 0.75 * rng.random((V, 3))).astype(np.float32)    # the second vertices come first
    ring = np.arange(extra, V)
    f = np.stack([ring, np.roll(ring, -1), np.roll(ring, -2)], 1).astype(np.int32)
    return (v, _colors(V, 7), f, dict(cell=1.0, origin=(0.0, 0.0, 0.0))), cells, size, home


def face_collisions(wrap):
    """(case, triples, table size, home): 64 vertices in cells of their own (label = index), 40 faces whose label triples
    share one home slot, then other windings of every fifth (duplicates found by probing)."""
    V, n = 64, 40
    F = n + n // 5
    size = MS.table_size(F)
    home = size - 1 if wrap else 9
    triples = []
    for t in itertools.combinations(range(V), 3):
        if MS._home_slot_faces(t, size) == home:
            triples.append(t)
            if len(triples) == n:
                break
    assert len(triples) == n
    rng = np.random.default_rng(8)
    f = [tuple(rng.permutation(t)) for t in triples] + [tuple(rng.permutation(t)) for t in triples[::5]]
    f = np.array(f, np.int32)[rng.permutation(F)]
    v = np.stack([np.arange(V) % 8, np.arange(V) // 8, np.zeros(V)], 1) * 2.0 + 0.5
    return (v.astype(np.float32), None, f, dict(cell=2.0, origin=(0.0, 0.0, 0.0))), triples, size, home


TRIPS_V = 262144 + 1000


def two_scan_trips():
    """Vertices 2k and 2k+1 share the cell (k,0,0).  Face [2k, 2k+2, 2k+4] is kept, [2k+5, 2k+3, 2k+1] after it is its
    duplicate: every second face and every even vertex stay, up to the last block."""
    V = TRIPS_V
    i = np.arange(V)
    v = np.stack([i // 2 + 0.25 + 0.5 * (i % 2), 0.25 + 0.125 * (i % 5), 0.5 + 0.0 * i], 1).astype(np.float32)
    k = 2 * np.arange(V // 2 - 2)
    f = np.stack([np.stack([k, k + 2, k + 4], 1), np.stack([k + 5, k + 3, k + 1], 1)], 1).reshape(-1, 3).astype(np.int32)
    c = np.stack([(i % 7) / 7.0, (i % 11) / 11.0, (i % 13) / 13.0], 1).astype(np.float32)
    return v, c, f, dict(cell=1.0, origin=(0.0, 0.0, 0.0))


def empty(V, F=0):
    rng = np.random.default_rng(9)
    return rng.random((V, 3)).astype(np.float32), _colors(V, 10), np.zeros((F, 3), np.int32), dict(cell=0.25, origin=None)


def one_face():
    v = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5]], np.float32)
    return v, _colors(3, 11), np.array([[2, 0, 1]], np.int32), dict(cell=1.0, origin=None)


SMALL_CASES = dict(hand=hand, one_cell=one_cell, crowd=crowd, one_face=one_face, empty_v0=lambda: empty(0),
                   empty_f0=lambda: empty(7), vertex_home=lambda: vertex_collisions(False)[0],
                   vertex_wrap=lambda: vertex_collisions(True)[0], face_home=lambda: face_collisions(False)[0],
                   face_wrap=lambda: face_collisions(True)[0])


# ---- an independent statement of the contract ------------------------------------------------------------------------
def plain_simplify(v, c, f, cell, origin):
    """The contract with a dict over cell tuples and a set of frozensets; exact rational means, rounded once where the
    contract rounds.  Returns (verts, faces, colors | None, info) like the mirror."""
    v = np.asarray(v, np.float32)
    cell = np.float32(cell)
    o = np.asarray(origin, np.float32)
    clusters = {}                                   # cell tuple -> vertex indices, ascending
    cells = []
    for i in range(len(v)):
        t = [np.float32(np.float32(v[i, ax] - o[ax]) / cell) for ax in range(3)]
        cells.append(tuple(int(np.floor(x)) for x in t))
        clusters.setdefault(cells[-1], []).append(i)
    label = [clusters[cells[i]][0] for i in range(len(v))]
    seen, kept, collapsed = set(), [], 0
    for face in np.asarray(f).tolist():
        l = [label[x] for x in face]
        if len(set(l)) < 3:
            collapsed += 1
        elif frozenset(l) not in seen:
            seen.add(frozenset(l))
            kept.append(l)
    names = sorted({x for l in kept for x in l})
    index = {x: k for k, x in enumerate(names)}
    out_v, out_c = [], []
    for x in names:
        members, cc = clusters[cells[x]], cells[x]
        row, crow = [], []
        for ax in range(3):
            S = 0
            for i in members:
                t = np.float32(np.float32(v[i, ax] - o[ax]) / cell)
                S += int(np.float32(t - np.floor(t)) * np.float32(2 ** 24))
            m = float(Fraction(S, len(members) * 2 ** 24))          # one rounding of the exact quotient
            row.append(np.float32(float(o[ax]) + (float(cc[ax]) + m) * float(cell)))
            if c is not None:
                S = 0
                for i in members:
                    x32 = np.float32(c[i, ax])
                    x32 = np.float32(0) if np.isnan(x32) else min(max(x32, np.float32(0)), np.float32(1))
                    S += int(x32 * np.float32(2 ** 24))
                crow.append(np.float32(float(Fraction(S, len(members) * 2 ** 24))))
        out_v.append(row)
        out_c.append(crow)
    F = len(np.asarray(f))
    info = dict(verts_in=len(v), faces_in=F, verts_out=len(names), faces_out=len(kept), num_clusters=len(clusters),
                collapsed_faces=collapsed, duplicate_faces=F - collapsed - len(kept))
    return (np.array(out_v, np.float32).reshape(-1, 3), np.array([[index[x] for x in l] for l in kept], np.int32).reshape(-1, 3),
            None if c is None else np.array(out_c, np.float32).reshape(-1, 3), info)


def edge_counts(faces):
    """{undirected edge: number of faces on it}"""
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    uniq, n = np.unique(e, axis=0, return_counts=True)
    return uniq, n
