"""Meshes shared by test_cpu_mesh_edges.py and test_gpu_mesh_edges.py, and an independent plain-Python statement of the
contracts of monogs_amd/mesh_topology.py and monogs_amd/mesh_smooth.py (a dict over frozensets, Fraction means rounded
once).

Every case is (verts [V,3] f32, faces [F,3] i32).  Sizes: every kernel works in blocks of 256 half-edges / vertices; the
one-workgroup scan takes 1024 block totals per trip (262 144 items); the hash table of F faces holds the smallest power
of two >= 6 F entries.
  hand             degenerate, repeated, rewound and rotated faces, an edge on three faces, unreferenced vertices in the
                   middle and at the end
  random(V)        V = 3, 7, 50, 300 vertices under 2 V + 1 random faces: no multiple of 64 or 256 anywhere
  star             MC.star(): one vertex on 6 000 edges - one degree counter, one cursor, one row
  long_rows        hubs of 255, 256 and 257 neighbours in one block of vertices (a lane walks a row of up to 256, the
                   workgroup a longer one), a hub of 1 001 in another block, and a closed fan of 600 whose hub moves while
                   its rim is pinned
  edge_home/_wrap  40 edges that share one home slot of the table (the LAST slot: the probe wraps), every fifth on a
                   second, rewound face
  two_scan_trips   K.two_scan_trips(): 789 420 half-edges and 263 144 vertices - a second trip of the scan for both, CSR
                   offsets past block 1 024"""
import itertools
import math
from fractions import Fraction

import numpy as np

import mesh_clean_cases as MC
import mesh_simplify_cases as K
from monogs_amd import mesh_smooth as SM
from monogs_amd import mesh_topology as MT
from monogs_amd.mesh_simplify import table_size

SPHERE_CENTRE = np.array(MC.FLOATER_SPHERES[0][0], np.float64)
NOISE_SIGMA = 0.15                                    # voxels


def _verts(V, seed):
    return (8.0 * np.random.default_rng(seed).standard_normal((V, 3))).astype(np.float32)


def hand():
    f = np.array([[0, 1, 2], [2, 1, 3], [0, 1, 2], [2, 1, 0], [1, 2, 0],      # a face, a neighbour, repeated, rewound, rotated
                  [4, 4, 5], [6, 7, 6], [8, 8, 8],                            # degenerate: no edge, not even 4-5
                  [1, 3, 9], [3, 1, 10],                                      # 1-3 on three faces
                  [12, 13, 14], [14, 13, 15], [12, 13, 16]],                  # 13-14 consistent, 12-13 twice in one direction
                 np.int32)
    return _verts(19, 1), f                           # 4..8, 11, 17, 18 lie on no edge


HAND_INFO = dict(verts_in=19, faces_in=13, edges=16, boundary_edges=10, manifold_edges=2, nonmanifold_edges=4,
                 inconsistent_edges=1, degenerate_faces=3, referenced_verts=11, boundary_verts=11, euler=5, closed=False,
                 oriented=False)


def random_mesh(V):
    rng = np.random.default_rng(100 + V)
    return _verts(V, V), rng.integers(0, V, (2 * V + 1, 3)).astype(np.int32)


def sphere():
    v, f, _ = MC.floater_mesh(big_only=True)
    return v, f


def floaters():
    v, f, _ = MC.floater_mesh()
    return v, f


def reversed_face():
    v, f = sphere()
    f = f.copy()
    f[17] = f[17][::-1]
    return v, f


def upper_half():
    """The faces of the sphere whose centroid lies above the centre: an open cap, its rim pinned, the rest unreferenced."""
    v, f = sphere()
    return v, f[v[f].mean(axis=1)[:, 2] > SPHERE_CENTRE[2]]


def three_on_an_edge():
    return _verts(5, 2), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def star():
    v, _, f = MC.star()
    return v, f


_noisy_cache = []


def noisy_sphere():
    """The sphere plus Gaussian noise of NOISE_SIGMA voxel (computed once; callers must not write into it)."""
    if not _noisy_cache:
        v, f = sphere()
        _noisy_cache.append((v + np.random.default_rng(0).normal(0.0, NOISE_SIGMA, v.shape)).astype(np.float32))
    return _noisy_cache[0], sphere()[1]


def radii(v):
    """(mean, std) of the distances to the analytic centre, in voxels."""
    r = np.linalg.norm(np.asarray(v, np.float64) - SPHERE_CENTRE, axis=1)
    return float(r.mean()), float(r.std())


def edge_collisions(wrap):
    """((verts, faces), edges, table size, home): 40 edges (a, b) with one home slot, face i = (a, b, 230 + i), and for
    every fifth a second face (b, a, 270 + i) on the other side."""
    n, V0 = 40, 230
    F = n + n // 5
    size = table_size(3 * F)
    home = size - 1 if wrap else 11
    edges = []
    for a, b in itertools.combinations(range(V0), 2):
        if MT._home_slot_edges(a, b, size) == home:
            edges.append((a, b))
            if len(edges) == n:
                break
    assert len(edges) == n
    f = [(a, b, V0 + i) for i, (a, b) in enumerate(edges)] + [(b, a, V0 + n + i) for i, (a, b) in enumerate(edges[::5])]
    f = np.array(f, np.int32)[np.random.default_rng(13).permutation(F)]
    return (_verts(V0 + n + n // 5, 3), f), edges, size, home


LONG_ROW_HUBS = {0: 255, 1: 256, 2: 257, 300: 1001, 301: 600}        # hub vertex -> neighbours


def long_rows():
    """Open fans of 254, 255, 256 and 1 000 faces on the hubs 0, 1, 2 and 300 (an open fan of n faces gives its hub n + 1
    neighbours), a closed fan of 600 faces on hub 301; the rims lie behind vertex 301."""
    faces, first = [], 302
    for hub, n, closed in ((0, 254, False), (1, 255, False), (2, 256, False), (300, 1000, False), (301, 600, True)):
        rim = np.arange(first, first + (n if closed else n + 1))
        first = int(rim[-1]) + 1
        nxt = np.roll(rim, -1) if closed else rim[1:]
        faces.append(np.stack([np.full(n, hub), rim[:n], nxt[:n]], 1))
    return _verts(first, 6), np.concatenate(faces).astype(np.int32)


def two_scan_trips():
    v, _, f, _ = K.two_scan_trips()
    return v, f


def empty(V, F=0):
    return _verts(V, 4), np.zeros((F, 3), np.int32)


def one_face():
    return _verts(3, 5), np.array([[2, 0, 1]], np.int32)


SMALL_CASES = dict(hand=hand, one_face=one_face, empty_v0=lambda: empty(0), empty_f0=lambda: empty(7),
                   random_3=lambda: random_mesh(3), random_7=lambda: random_mesh(7), random_50=lambda: random_mesh(50),
                   random_300=lambda: random_mesh(300), star=star, long_rows=long_rows, three_on_an_edge=three_on_an_edge,
                   reversed_face=reversed_face, upper_half=upper_half, floaters=floaters,
                   edge_home=lambda: edge_collisions(False)[0], edge_wrap=lambda: edge_collisions(True)[0])


# ---- an independent statement of the contracts -------------------------------------------------------------------------
def plain_edges(faces, V):
    """(edges, edge_faces, degree, flags, info) with a dict over frozensets, in plain Python."""
    faces = np.asarray(faces).tolist()
    first, count, forward, degenerate = {}, {}, {}, 0
    for f, face in enumerate(faces):
        if len(set(face)) < 3:
            degenerate += 1
            continue
        for k in range(3):
            a, b = face[k], face[(k + 1) % 3]
            e = frozenset((a, b))
            first.setdefault(e, 3 * f + k)
            count[e] = count.get(e, 0) + 1
            forward[e] = forward.get(e, 0) + (1 if a < b else 0)
    order = sorted(first, key=first.get)
    degree, flags = [0] * V, [0] * V
    for e in order:
        for x in e:
            degree[x] += 1
            flags[x] |= 1 | (2 if count[e] != 2 else 0)
    n = [count[e] for e in order]
    boundary, manifold = sum(c == 1 for c in n), sum(c == 2 for c in n)
    inconsistent = sum(count[e] == 2 and forward[e] != 1 for e in order)
    referenced = sum(d > 0 for d in degree)
    info = dict(verts_in=V, faces_in=len(faces), edges=len(order), boundary_edges=boundary, manifold_edges=manifold,
                nonmanifold_edges=len(order) - boundary - manifold, inconsistent_edges=inconsistent,
                degenerate_faces=degenerate, referenced_verts=referenced, boundary_verts=sum(x & 2 != 0 for x in flags),
                euler=referenced - len(order) + len(faces) - degenerate, closed=boundary == 0 and len(order) == manifold,
                oriented=boundary == 0 and len(order) == manifold and inconsistent == 0)
    return (np.array([sorted(e) for e in order], np.int32).reshape(-1, 2), np.array(n, np.int32),
            np.array(degree, np.int32), np.array(flags, np.int32), info)


def plain_smooth(verts, faces, iterations, lam, mu, boundary):
    """The positions after smoothing: sets of neighbours, exact integer sums, Fraction means rounded once, Python floats
    (one fp64 rounding per operation)."""
    v = np.asarray(verts, np.float32)
    V = len(v)
    nbr = [set() for _ in range(V)]
    count = {}
    for face in np.asarray(faces).tolist():
        if len(set(face)) == 3:
            for k in range(3):
                e = frozenset((face[k], face[(k + 1) % 3]))
                count[e] = count.get(e, 0) + 1
    pinned = set()
    for e, c in count.items():
        a, b = tuple(e)
        nbr[a].add(b)
        nbr[b].add(a)
        if c != 2 and boundary == "pin":
            pinned |= e
    E = max([math.frexp(abs(float(x)))[1] - 1 for x in v.reshape(-1) if x != 0] or [-127])
    K28 = SM.FIXED_BITS
    p = [[float(x) for x in row] for row in v]
    weights = [float(np.float32(lam))] + ([] if mu is None else [float(np.float32(mu))])
    for _ in range(iterations):
        for w in weights:
            new = [list(row) for row in p]
            for i in range(V):
                if not nbr[i] or i in pinned:
                    continue
                for ax in range(3):
                    S = sum(int(math.ldexp(p[u][ax], K28 - E)) for u in nbr[i])          # int() truncates
                    m = float(Fraction(S, len(nbr[i])) * Fraction(2) ** (E - K28))       # one rounding of the exact mean
                    new[i][ax] = float(np.float32(p[i][ax] + w * (m - p[i][ax])))
            p = new
    return np.array(p, np.float64).astype(np.float32).reshape(-1, 3)
