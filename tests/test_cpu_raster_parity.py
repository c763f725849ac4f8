"""The per-pixel / per-Gaussian parity construction of tests/raster_parity.py, held on the CPU: the fp32 oracle and
the C++ host emulation (which shares raster_math.h with the kernels) stay inside every bound and cap on every scene,
and deliberately wrong variants of the oracle are rejected - two of them while they still pass the aggregate
thresholds of tests/test_raster_gpu.py::_compare, which is the gap this comparison closes."""
import types

import pytest
import torch

import raster_parity as P


ALL_NAMES = P.CASE_NAMES + [P.LONG] + P.DECISION_NAMES
DECISIONS = "decisions_70x45"


def _modes(name):
    """The decision scene is held under both treatments of the clamp in the backward, every other scene under the
    product default."""
    return ("upstream", "exact") if name == DECISIONS else ("upstream",)


def _caps(ref):
    """The caps are asserted on every scene but the long oblique needles, whose own band (1 %) makes a third of their
    rows fragile by construction: there the shares are reported (4.5 % of the pixels, 30 ... 37 % of the rows)."""
    return P.cap_shares(ref) if ref.case.name == P.LONG else P.check_caps(ref)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_reference_alone_stays_within_bounds(name):
    """scene_margins (inside reference()) and the caps hold, and the fp32 oracle passes against the fp64 one."""
    for mode in _modes(name):
        ref = P.reference(name, mode)
        shares = _caps(ref)
        stats = P.assert_parity(P.run_oracle(ref.case, torch.float32, clamp_grad=mode), ref, f"fp32 oracle, {mode}")
        print(name, mode, "caps:", f"pixels {100 * shares['pixels']:.2f} %, radii {100 * shares['radii']:.2f} %, rows",
              ", ".join(f"{k} {100 * v:.1f} %" for k, v in shares["rows"].items()), "| fp32 oracle,", P.ratios(stats))


def _emulate(c, exact_cull, clamp_grad="upstream"):
    from oracle.host_emul import HostEmul
    em = HostEmul()
    em.set_clamp_gradient_mode(clamp_grad)
    img, radii, dep, opa, nt = em.forward(P.settings_of(c, torch.float32), c.m, c.sh, c.col, c.o, c.s, c.r, c.cov,
                                          exact_cull=exact_cull)
    HW = c.cam.H * c.cam.W
    out = em.backward(c.gi / HW, c.gd / HW)
    grads = P.pack_grads(c.m.shape[0], out["means3D"], out["means2D"], out["opacities"], out["colors"],
                         None if c.s is None else out["scales"], None if c.r is None else out["rotations"],
                         None if c.cov is None else out["cov3D"])
    return dict(image=img, depth=dep, opacity=opa, radii=radii, n_touched=nt, grads=grads, tau=out["tau"]), em.pairs


@pytest.mark.parametrize("name", ALL_NAMES)
def test_host_emulation_stays_within_bounds(built, name):
    """Forward with the reference's bounding-square binning and with the exact cull (box_reachable: "never rejects a
    contributing pair" - checked pixel by pixel, on the grazing scenes in particular), and the backward of each."""
    for mode in _modes(name):
        ref = P.reference(name, mode)
        for exact in (False, True):
            got, pairs = _emulate(ref.case, exact, mode)
            stats = P.assert_parity(got, ref, f"host emulation, exact_cull={exact}, {mode}")
            print(name, mode, "exact_cull", exact, P.ratios(stats))
            if name in P.TIE_NAMES:          # the cull drops nothing either: the tile's list is the whole scene
                assert pairs == ref.case.m.shape[0], pairs


@pytest.mark.parametrize("name", ["grazing_41x23", "grazing_49x33", "grazing_long"])
def test_exact_cull_drops_no_contributing_pair_of_a_needle(built, name):
    """Culled and unculled host emulation use the same fp32 conic, so this comparison is free of the conditioning
    that loosens the fp64 comparison of long oblique needles (raster_parity._grazing): the cull removes pairs and
    changes no output bit and no gradient."""
    c = P.case(name)
    a, pairs_a = _emulate(c, False)
    b, pairs_b = _emulate(c, True)
    assert pairs_b < pairs_a
    for k in ("image", "depth", "opacity", "radii", "n_touched"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert torch.equal(a["tau"], b["tau"])


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
MUTANT_SCENE = "generic_moved_nopose"


def _opaque_overlapping_pair(ref):
    """(tile x, tile y, i, j): the two closest centres among the opaque (opacity > 0.8) visible splats that share a tile
    and lie inside it."""
    c, proj = ref.case, ref.out["info"]["proj"]
    xy, op = proj.xy.detach(), c.o.reshape(-1)
    ids = ((ref.out["radii"] > 0) & (op > 0.8)).nonzero().flatten()
    best = None
    for a in range(ids.numel()):
        for b in range(a + 1, ids.numel()):
            i, j = int(ids[a]), int(ids[b])
            ti, tj = (xy[i] // 16).tolist(), (xy[j] // 16).tolist()
            inside = 0 <= xy[i, 0] < c.cam.W and 0 <= xy[i, 1] < c.cam.H
            d = (xy[i] - xy[j]).norm().item()
            if ti == tj and inside and (best is None or d < best[0]):
                best = (d, int(ti[0]), int(ti[1]), i, j)
    assert best is not None and best[0] < 3.0, best
    return best[1:]


def _mutants(ref):
    """name -> (outputs, must the aggregate thresholds accept it).  (i) ... (iv) are the four planned mutants; applied to the whole image
    they are gross enough for the aggregate thresholds to notice, so (i) and (iii) come a second time confined to what a
    kernel bug typically hits - one tile, fewer rows - and those pass them.  (The count-based n_touched threshold, 1 % of
    the touched entries, notices even one dropped pixel row of a quadrant: 17 entries > 11.)"""
    c = ref.case
    out = {}
    with P.thresholds(alpha_min=1.05):
        whole = P.run_oracle(c)
    out["(i) alpha_min x 1.05"] = (whole, False)
    tile = {k: (v.clone() if k in ("image", "depth", "opacity") else v) for k, v in ref.out.items()}
    y0, x0 = c.cam.H // 2 // 16 * 16, c.cam.W // 2 // 16 * 16
    for k in ("image", "depth", "opacity"):
        tile[k][:, y0:y0 + 16, x0:x0 + 16] = whole[k][:, y0:y0 + 16, x0:x0 + 16]
    out["(i') alpha_min x 1.05 in the forward outputs of one tile"] = (tile, True)
    tx0, ty0, i, j = _opaque_overlapping_pair(ref)

    def swap(tx, ty, ids):
        if (tx, ty) != (tx0, ty0):
            return ids
        ids = ids.clone()
        pi, pj = int((ids == i).nonzero()), int((ids == j).nonzero())
        ids[pi], ids[pj] = j, i
        return ids

    with P.hooks(order=swap):
        out["(ii) two opaque splats swapped in one tile"] = (P.run_oracle(c), False)
    g = ref.out["grads"]["means3D"]
    n = g.norm(dim=1)
    rows = (n > 0).nonzero().flatten()
    for label, share, accepted in (("(iii) 5 %", 0.05, False), ("(iii') 2 %", 0.02, True)):
        m = {k: (dict(v) if k == "grads" else v) for k, v in ref.out.items()}
        z = g.clone()
        z[rows[n[rows].argsort()[: max(1, int(share * rows.numel()))]]] = 0.0
        m["grads"]["means3D"] = z
        out[label + " smallest means3D rows zeroed"] = (m, accepted)
    qx, qy = c.cam.W // 2 // 8, c.cam.H // 2 // 8
    for label, accepted in (("(iv) one quadrant's n_touched dropped", False),):
        with P.hooks(touch=lambda tx, ty, PX, PY: ~((PX // 8 == qx) & (PY // 8 == qy))):
            dropped = P.run_oracle(c, backward=False)
        out[label] = ({**ref.out, "n_touched": dropped["n_touched"]}, accepted)
    return out


def test_constants_are_what_the_reference_measures():
    """Re-measures every constant (fp32 oracle against fp64 oracle, the observer hook of the oracle included) and
    holds the committed value to factor x measured, rounded up by at most 5 %: the table cannot drift from the scenes."""
    worst = max(P.alpha_rel_diff(P.case(n)) for n in P.CASE_NAMES)
    measured = dict(band=P.BAND_FACTOR * worst, base=0.0, base_depth=0.0, base_g=0.0, base_tau=0.0)
    for n in P.CASE_NAMES:
        r = P.measure_bases(n)
        for k, v in (("base", max(r["image"], r["opacity"])), ("base_depth", r["depth"]), ("base_g", r["row_max"]), ("base_tau", r["tau"])):
            measured[k] = max(measured[k], P.BASE_FACTOR * v)
    r = P.measure_bases(P.LONG)
    long = dict(band=P.BAND_FACTOR * P.alpha_rel_diff(P.case(P.LONG)), base=P.BASE_FACTOR * max(r["image"], r["opacity"]),
                base_depth=P.BASE_FACTOR * r["depth"], base_g=P.BASE_FACTOR * r["row_max"], base_tau=P.BASE_FACTOR * r["tau"])
    for what, const, meas in (("CONST", P.CONST, measured), ("CONST_LONG", P.CONST_LONG, long)):
        print(what, {k: f"{const[k]:.3g} (measured {meas[k]:.4g})" for k in const})
        for k in const:
            assert meas[k] <= const[k] <= P.ROUND_UP * meas[k], (what, k, const[k], meas[k])


def test_a_candidate_without_gradients_fails():
    ref = P.reference("faint_two")
    fwd = {**ref.out, "grads": None, "tau": None}
    assert P.assert_parity(fwd, ref, forward_only=True)["ok"]
    with pytest.raises(AssertionError, match="no gradients"):
        P.assert_parity(fwd, ref)
    with pytest.raises(AssertionError, match="no pose gradient"):
        P.assert_parity({**ref.out, "tau": None}, ref)


def test_a_pair_dropped_from_a_long_oblique_needle_is_rejected():
    """What the long-needle scene is for: alpha_min x 1.05 - pairs up to 5 % above 1/255 dropped, as a cull with too
    little slack would - in the forward outputs of ONE tile of it is rejected at that scene's own constants, for
    each of the six whole tiles of the 49x33 image (the one-pixel tiles of its last row and column may hold no pair
    in that window)."""
    ref = P.reference(P.LONG)
    c = ref.case
    with P.thresholds(alpha_min=1.05):
        whole = P.run_oracle(c, backward=False)
    rejected = tiles = 0
    for y0 in range(0, c.cam.H - 15, 16):
        for x0 in range(0, c.cam.W - 15, 16):
            tiles += 1
            mut = {k: (v.clone() if k in ("image", "depth", "opacity") else v) for k, v in ref.out.items()}
            for k in ("image", "depth", "opacity"):
                mut[k][:, y0:y0 + 16, x0:x0 + 16] = whole[k][:, y0:y0 + 16, x0:x0 + 16]
            rejected += not P.assert_parity(mut, ref, raise_on_fail=False)["ok"]
    print(f"rejected in {rejected} of {tiles} tiles")
    assert tiles == 6 and rejected == tiles


def _old_compare(got, ref):
    """The real aggregate comparison of tests/test_raster_gpu.py on this module's layout; True when it passes."""
    from test_raster_gpu import _compare
    ns = lambda t: None if t is None else types.SimpleNamespace(grad=t)
    c = ref.case

    def side(o):
        g = o["grads"]
        N = c.m.shape[0]
        L = dict(m=ns(g["means3D"]), o=ns(g["opacities"]), sh=ns(g["colors"]) if c.sh is not None else None,
                 col=ns(g["colors"]) if c.col is not None else None, s=ns(g.get("scales")), r=ns(g.get("rotations")),
                 cov=ns(g.get("cov3D")))
        tau = o["tau"] if o["tau"] is not None else torch.ones(6, dtype=torch.float64)
        return ((o["image"], o["radii"], o["depth"], o["opacity"], o["n_touched"]), L, ns(tau[3:]), ns(tau[:3]),
                ns(g["means2D"].reshape(N, 3)))

    try:
        _compare(side(got), side(ref.out))
    except AssertionError:
        return False
    return True


def test_mutants_are_rejected_here_and_accepted_by_the_aggregate_thresholds():
    """Every mutant must be rejected by assert_parity.  What each measures against both comparisons is printed (run with
    -s).  Measured on the 1468-splat scene at 150x101: the four planned mutants, applied to the whole image, do NOT pass the
    aggregate thresholds of _compare - (i) n_touched differs for 499 Gaussians and the gradient norms by 0.2 ... 1.5 %,
    (ii) two wrong rows of opaque splats move the gradient norms by 0.2 ... 2 %, (iii) means3D norm 1.65e-3 > 1e-3,
    (iv) 22 n_touched entries > 11 - and are kept.  The confined forms (i') and (iii') pass every aggregate threshold
    and are rejected here: that pair of outcomes is the gap this comparison closes."""
    ref = P.reference(MUTANT_SCENE)
    assert _old_compare(ref.out, ref) and P.assert_parity(ref.out, ref)["ok"]
    for name, (mut, accepted) in _mutants(ref).items():
        stats = P.assert_parity(mut, ref, raise_on_fail=False)
        agg = P.aggregate_metrics(mut, ref)
        old = _old_compare(mut, ref)
        assert old == P.aggregate_passes(agg), (name, agg)
        print(f"\nMUTANT {name}: aggregate thresholds {'PASS' if old else 'FAIL'}: "
              + ", ".join(f"{k} {v:.3g} (<= {lim:.3g})" for k, (v, lim) in agg.items()))
        print(f"  per-pixel / per-row comparison {'PASS' if stats['ok'] else 'REJECTS'}:")
        for line in stats["fails"]:
            print("    " + line)
        assert not stats["ok"], f"mutant '{name}' passes the per-pixel / per-row comparison"
        assert old == accepted, f"mutant '{name}': aggregate thresholds {'accept' if old else 'reject'} it"


# ---------------------------------------------------------------------------------------------------------------------
# decision scenes: what they are, from the reference alone, and the mutants they must reject
# ---------------------------------------------------------------------------------------------------------------------
# rows of decisions_70x45 (raster_parity._decisions): per group the order is +2 band, -2 band, +16 band, -16 band
NEAR = dict(visible=[0, 2, 6], culled=[1, 3, 4, 5, 7])              # 0.2 (1 +- 2 band), 0.2 (1 +- 16 band), 0.1, 0.19, 0.21, behind
CLAMP_FIRST, RECT_FIRST = 8, 24
CLAMPED = [CLAMP_FIRST + 4 * side + j for side in range(4) for j in (0, 2)]       # beyond the limit: + 2 band, + 16 band
CLAMP_PLUS2 = [CLAMP_FIRST + 4 * side for side in range(4)]
CLAMP_MINUS2 = [CLAMP_FIRST + 4 * side + 1 for side in range(4)]


def test_decision_scene_sits_where_it_claims():
    """Nothing is taken out of it, every Gaussian of a group lies 2 or 16 bands from its decision and on the side it
    is meant to, the rectangle splats end 0.5 px before / after their tile boundary with the oracle's own radius, the
    visible ones come out with radii > 0 and full gradient rows, the others with radii 0 and zero rows."""
    built = P._BUILDERS[DECISIONS]()
    ref = P.reference(DECISIONS)
    c, out, K, band = ref.case, ref.out, P.O.CONSTANTS, P.CONST["band"]
    assert c.m.shape[0] == built.m.shape[0] == 32 and torch.equal(c.m, built.m)
    trips, _ = P.margin_trips(c, out, ref.radius_fragile)
    assert not any(m.any() for m in trips.values()) and not ref.radius_fragile.any()
    m = c.m.double()
    z = m[:, 2]
    steps = torch.tensor([2.0, -2.0, 16.0, -16.0], dtype=torch.float64) * band
    assert torch.allclose(z[:4] / K["near_z"] - 1.0, steps, rtol=1e-3, atol=0)
    assert z[4:8].tolist() == pytest.approx([0.1, 0.19, 0.21, -1.0])
    for side, (axis, sign, tanfov) in enumerate(((0, 1, c.cam.tanfovx), (0, -1, c.cam.tanfovx), (1, 1, c.cam.tanfovy), (1, -1, c.cam.tanfovy))):
        i = CLAMP_FIRST + 4 * side
        ratio = sign * m[i:i + 4, axis] / z[i:i + 4] / (K["fov_clamp"] * tanfov)
        assert torch.allclose(ratio - 1.0, steps, rtol=1e-3, atol=0), (side, ratio)
        assert ((2.0 <= z[i:i + 4]) & (z[i:i + 4] <= 3.0)).all()
    # depths are distinct and well separated: the closest two are the near-plane pair at 0.2 (1 +- 2 band), 4 bands
    # = 2.7e-3 apart, against the 1e-6 below which the order inside a tile would be in question
    zs = torch.sort(z[z > 0]).values
    assert ((zs[1:] - zs[:-1]) / zs[1:]).min() > 3.9 * band > 1000 * P.DEPTH_GAP
    # the rectangle splats, with the radius the oracle would give them were they visible
    pr = out["info"]["proj"]
    rad = torch.ceil(K["radius_sigma"] * torch.sqrt(P._lambda_max(pr.cov2d.detach())))
    xy = pr.xy.detach()
    gx, gy = (c.cam.W + 15) // 16, (c.cam.H + 15) // 16
    ends = []
    for j, (axis, side, edge) in enumerate(((0, 1, 1.0), (0, -1, 16.0 * gx), (1, 1, 1.0), (1, -1, 16.0 * gy))):
        for k in (0, 1):
            i = RECT_FIRST + 2 * j + k
            ends.append(side * (xy[i, axis] + side * rad[i] - edge))
    assert torch.allclose(torch.stack(ends), torch.tensor([-0.5, 0.5] * 4, dtype=torch.float64), atol=1e-4), ends
    visible = NEAR["visible"] + list(range(CLAMP_FIRST, RECT_FIRST)) + [RECT_FIRST + 2 * j + 1 for j in range(4)]
    assert (out["radii"] > 0).nonzero().flatten().tolist() == sorted(visible)
    # a visible splat that reaches a pixel has a full row in every tensor, a culled one a zero row
    reaches = out["n_touched"] > 0
    assert reaches[NEAR["visible"]].all() and reaches[CLAMP_FIRST:RECT_FIRST].all()
    for mode in ("upstream", "exact"):
        g = P.reference(DECISIONS, mode).out["grads"]
        for name, rows in g.items():
            n = rows.norm(dim=1)
            assert (n[reaches] > 0).all(), (mode, name)
            assert (n[out["radii"] == 0] == 0).all(), (mode, name)
            used = rows[:, :2] if name == "means2D" else rows        # the third column of means2D is never written
            assert (used[reaches] != 0).all(), (mode, name)


@pytest.mark.parametrize("name", P.TIE_NAMES)
def test_tie_scenes_are_what_they_claim(name):
    """Most sorted neighbours are exact ties; every pair of the tile is well above 1/255 (raw alpha >= 1.15/255), so the
    list holds all N splats, past the sort class the scene is for; ties_40 and ties_1100 end at T >= 10 t_stop, ties_4200
    stops everywhere and no pixel's allowance exceeds its base."""
    ref = P.reference(name)
    c, out, K = ref.case, ref.out, P.O.CONSTANTS
    N = c.m.shape[0]
    assert N == P._BUILDERS[name]().m.shape[0] and N > P.TIE_LIST_CLASS[name]
    assert torch.equal(c.cam.viewmatrix, torch.eye(4)) and (c.cam.W, c.cam.H) == (16, 16)
    depth = out["info"]["proj"].depth.detach()
    assert torch.equal(depth, c.m[:, 2].double()) and torch.equal(depth * 8, torch.round(depth * 8))
    d = torch.sort(depth).values
    assert (d[1:] == d[:-1]).sum() > 0.6 * (N - 1)
    assert out["info"]["pairs"] == N
    seen = {}
    with P.hooks(pairs=lambda tx, ty, ids, raw, inc: seen.update(raw=raw, ids=ids)):
        P.run_oracle(c, backward=False)
    assert seen["ids"].numel() == N and seen["raw"].min() >= 1.15 / 255 and seen["raw"].max() <= 2.5 / 255
    final_T = 1.0 - out["opacity"]
    if name == P.STOPS:
        assert final_T.max() < 1.02 * K["t_stop"]
        a, k = ref.allow, P.CONST
        assert not ((a["image"] > k["base"]) | (a["depth"] > k["base_depth"]) | (a["opacity"] > k["base"])).any()
    else:
        assert final_T.min() >= P.MIN_FINAL_T * K["t_stop"], final_T.min()
    P.check_caps(ref)


def _over(stats):
    return stats["over"]


def test_a_moved_near_plane_is_rejected():
    """near_z x (1 +- 4 band): the splat at 0.2 (1 + 2 band) resp. 0.2 (1 - 2 band) changes sides - its radius differs, its
    rows are over and so are more than 100 of the pixels it owns."""
    ref = P.reference(DECISIONS)
    band = P.CONST["band"]
    for factor, row in ((1 + 4 * band, 0), (1 - 4 * band, 1)):
        with P.thresholds(near_z=factor):
            mut = P.run_oracle(ref.case)
        stats = P.assert_parity(mut, ref, raise_on_fail=False)
        o = _over(stats)
        print(f"near_z x {factor:.5f}:", o)
        assert not stats["ok"] and o["radii"] == [row]
        assert o["pixels"]["image"] > 100 and o["pixels"]["opacity"] > 100
        assert all(row in rows for rows in o["rows"].values())


def test_a_moved_clamp_limit_is_rejected():
    """fov_clamp x (1 +- 4 band), under both backward treatments: the four splats at 1.3 tanfov (1 + 2 band) resp.
    (1 - 2 band) change their clamp flag, and the means3D row of each of them is over.  (The limit enters the forward
    of every clamped splat too, so pixels and a row or two of the other splats are over as well.)"""
    band = P.CONST["band"]
    for mode in ("upstream", "exact"):
        ref = P.reference(DECISIONS, mode)
        for factor, flipped in ((1 + 4 * band, CLAMP_PLUS2), (1 - 4 * band, CLAMP_MINUS2)):
            with P.thresholds(fov_clamp=factor):
                mut = P.run_oracle(ref.case, clamp_grad=mode)
            stats = P.assert_parity(mut, ref, raise_on_fail=False)
            print(f"fov_clamp x {factor:.5f}, {mode}:", _over(stats))
            assert not stats["ok"] and not _over(stats)["radii"]
            assert set(flipped) <= set(_over(stats)["rows"]["means3D"])


def test_the_other_clamp_gradient_treatment_is_rejected():
    """"exact" against the "upstream" reference and the reverse: the forward is the same, so no pixel and no radius
    moves; the means3D rows of all eight clamped splats are over and no other row of any tensor.  (dtau, which sums
    the same camera-space gradients, is over too.)"""
    up, ex = P.reference(DECISIONS, "upstream"), P.reference(DECISIONS, "exact")
    for got, ref in ((ex.out, up), (up.out, ex)):
        stats = P.assert_parity(got, ref, raise_on_fail=False)
        o = _over(stats)
        print(o, P.ratios(stats))
        assert not stats["ok"] and not o["radii"] and not any(o["pixels"].values())
        assert o["rows"].pop("means3D") == CLAMPED
        assert not any(o["rows"].values())


def _by_descending_index(depth):
    def order(tx, ty, ids):
        d, i = depth[ids].tolist(), ids.tolist()
        return ids[torch.tensor(sorted(range(len(i)), key=lambda k: (d[k], -i[k])))]
    return order


@pytest.mark.parametrize("name", P.TIE_NAMES)
def test_ties_broken_by_descending_index_are_rejected(name):
    ref = P.reference(name)
    with P.hooks(order=_by_descending_index(ref.out["info"]["proj"].depth.detach())):
        mut = P.run_oracle(ref.case)
    stats = P.assert_parity(mut, ref, raise_on_fail=False)
    print(name, {k: (v if k != "rows" else {t: len(r) for t, r in v.items()}) for k, v in _over(stats).items()})
    assert not stats["ok"] and _over(stats)["pixels"]["image"] == 256


def test_one_exchanged_pair_of_tied_neighbours_is_rejected_by_its_rows():
    """ties_1100, the first tied neighbours from the middle of the list on: the image moves by less than `base` (no
    pixel is over), the two splats' gradient rows catch it."""
    ref = P.reference("ties_1100")
    depth = ref.out["info"]["proj"].depth.detach()
    order = torch.sort(depth, stable=True).indices
    d = depth[order]
    tied = (d[1:] == d[:-1]).nonzero().flatten()
    pos = int(tied[tied >= d.numel() // 2][0])
    pair = sorted((int(order[pos]), int(order[pos + 1])))

    def swap(tx, ty, ids):
        ids = ids.clone()
        ids[pos], ids[pos + 1] = int(ids[pos + 1]), int(ids[pos])
        return ids

    with P.hooks(order=swap):
        mut = P.run_oracle(ref.case)
    assert not torch.equal(mut["image"], ref.out["image"])
    stats = P.assert_parity(mut, ref, raise_on_fail=False)
    o = _over(stats)
    print("exchanged", pair, "at list position", pos, o, P.ratios(stats))
    assert not stats["ok"] and not any(o["pixels"].values())
    assert o["rows"]["colors"] == pair and o["rows"]["means3D"] == pair
