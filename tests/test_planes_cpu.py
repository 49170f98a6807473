"""CPU checks of the plane-set queries' restatement (planes_ref.py) and of what the kernel relies on: the restatement against a float64 brute
force within the proof's bound (R1 of query_core.h), the two relations to the box queries (superset; bit equality where at most one axis has
an excess), plane and margin validity, the tiles of a camera holding every sphere their pixels' rays hit (the oracle's objs_hit), the helpers'
premises, the node test's counterexample search (build/plane_query_bound_check: clean with the slack, violations without it and on the partial
boxes), and the loader's symbols and the header's declarations."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import boxes_ref as B
import oracle_lib as O
import planes_ref as PL
import ray_query_ref as RQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


@pytest.fixture(scope="module", params=[("rgbbox", {}), ("irreg", {}), ("floor", {"n": 37, "k": 222.0})], ids=["rgbbox", "irreg", "floor"])
def scene(request):
    name, kw = request.param
    return O.OracleScene(name, **kw).arrays()["L"]


# ---- accuracy: the float32 restatement against float64 on the exactly normalised planes
@pytest.mark.parametrize("K", [1, 4, 6, 8])
def test_against_float64(scene, K):
    L = scene
    m = 256
    planes = PL.random_planes(L, m, K, 30 + K)
    assert PL.plane_ok(planes).all()
    margin = np.random.default_rng(21).uniform(0.0, 3.0, m).astype(F)
    g32, g64, bound = PL.gaps(L, planes), PL.gaps64(L, planes), PL.gap_error_bound(L, planes)
    err = np.abs(g32.astype(np.float64) - g64)
    print(f"pairs {err.size}, worst |G - g| / bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    sel32, sel64 = g32 <= margin[:, None], g64 <= margin[:, None].astype(np.float64)
    clear = np.abs(g64 - margin[:, None].astype(np.float64)) > bound
    left_out = 1.0 - clear.mean()
    print(f"left out {left_out:.3g}, selected {int(sel32.sum())}, disagreeing {int((sel32 != sel64)[clear].sum())}")
    assert not (sel32 != sel64)[clear].any()
    assert left_out <= 1e-4
    assert sel32.sum() >= 3000                                               # not vacuous
    # ... and the CSR assembly is that selection
    off, idx, gap = PL.in_planes(L, planes, margin)
    r, c = np.nonzero(sel32)
    assert np.array_equal(np.diff(off), sel32.sum(axis=1)) and np.array_equal(idx, c) and np.array_equal(_bits(gap), _bits(g32[r, c]))
    # a centre inside every half-space: gap -r exactly
    inside = PL.depths64(L, planes).min(axis=1) > 1e-3
    assert inside.sum() > 100 and np.array_equal(_bits(g32[inside]), _bits(np.broadcast_to(-L[None, :, 6], g32.shape)[inside]))
    # the contradictory queries (two planes are needed) hold no centre
    assert K == 1 or not inside[7::8].any()


# ---- the two relations to the box queries
def test_box_relations(scene):
    L = scene
    m = 384
    boxes = B.random_boxes(L, m, 3)
    planes = PL.box_planes(boxes)
    q, ln = PL.normalise(planes)
    assert (ln == 1.0).all() and np.array_equal(_bits(q + F(0)), _bits(planes + F(0)))      # len exactly 1 (-0.0 aside)
    gp, gb = PL.gaps(L, planes), B.gaps(L, boxes)
    assert (gp <= gb).all()                                                   # the plane gap never exceeds the box gap ...
    for margin in (0.0, 0.5, np.random.default_rng(4).uniform(0.0, 3.0, m).astype(F)):
        po, pi, _ = PL.in_planes(L, planes, margin)
        bo, bi, _ = B.in_boxes(L, boxes, margin)
        assert bo[-1] > 0 and po[-1] >= bo[-1]
        for i in range(m):                                                    # ... so the plane row holds the box row
            assert np.isin(bi[bo[i]:bo[i + 1]], pi[po[i]:po[i + 1]]).all(), i
    # where at most one axis has a positive excess the two gaps are the same bits
    with np.errstate(all="ignore"):
        pos = sum((np.fmax(boxes[:, None, k] - L[None, :, k], L[None, :, k] - boxes[:, None, 3 + k]) > 0).astype(int) for k in range(3))
    one = pos <= 1
    print(f"pairs {one.size}, at most one axis: {int(one.sum())}, exactly one: {int((pos == 1).sum())}")
    assert (pos == 1).sum() > 1000 and (pos >= 2).sum() > 1000
    assert np.array_equal(_bits(gp[one]), _bits(gb[one]))
    assert (gp[pos >= 2] < gb[pos >= 2]).any()                                # and beyond an edge or a corner the plane gap is smaller


# ---- validity
def test_plane_and_margin_validity(scene):
    L = scene
    c = L[L.shape[0] // 2, :3].astype(np.float64)
    good = np.array([[1, 0, 0, -(c[0] - 2.0)], [-1, 0, 0, c[0] + 2.0]], F)
    nan, inf = np.nan, np.inf
    lo, hi = F(2.0 ** -40), F(2.0 ** 40)
    cases = [
        (good[1], True),
        ([0, 0, 0, 1], False),                                                # a zero normal
        ([nan, 0, 0, 1], False), ([1, nan, 0, 1], False), ([1, 0, nan, 1], False), ([1, 0, 0, nan], False),
        ([inf, 0, 0, 1], False), ([1, -inf, 0, 1], False), ([1, 0, inf, 1], False), ([1, 0, 0, -inf], False),
        ([lo, 0, 0, -lo * F(c[0] - 2.0)], True),                              # len == 2^-40 ...
        ([np.nextafter(lo, F(0)), 0, 0, 0], False),                           # ... and one ulp below
        ([0, -hi, 0, hi * F(c[1] + 2.0)], True),                              # len == 2^40 ...
        ([0, np.nextafter(hi, F(inf)), 0, 0], False),                         # ... and one ulp above
        ([0, 0, lo, 1e38], False),                                            # d / len overflows
        ([1e30, 0, 0, 0], False),                                             # a * a overflows: len = inf
        ([-0.0, 1, -0.0, 3.0 - c[1]], True),
    ]
    m = len(cases)
    planes = np.tile(good[0], (m, 2, 1)).astype(F)
    for i, (p, _) in enumerate(cases):
        planes[i, 1] = np.asarray(p, F)
    want_ok = np.array([ok for _, ok in cases])
    with np.errstate(all="ignore"):
        ok = PL.plane_ok(planes)
    assert ok[:, 0].all() and ok[:, 1].tolist() == want_ok.tolist()
    off, idx, gap = PL.in_planes(L, planes, 1.0)
    ln = np.diff(off)
    assert (ln[want_ok] > 0).all() and not ln[~want_ok].any()
    # an invalid plane in either slot empties the row
    swapped = np.ascontiguousarray(planes[:, ::-1])
    assert np.array_equal(np.diff(PL.in_planes(L, swapped, 1.0)[0]) > 0, want_ok)
    # margins
    pm = np.tile(good, (6, 1, 1)).astype(F)
    margin = np.array([1.0, -0.0, nan, -1.0, 1.0000001e9, inf], F)
    off, idx, gap = PL.in_planes(L, pm, margin)
    ln = np.diff(off)
    assert ln[0] > 0 and ln[1] > 0 and not ln[2:].any()
    z = PL.in_planes(L, pm[:1], 0.0)
    assert ln[1] == z[0][1] and np.array_equal(idx[off[1]:off[2]], z[1]) and np.array_equal(_bits(gap[off[1]:off[2]]), _bits(z[2]))
    s = PL.in_planes(L, pm[:2], 1.0)                                          # a scalar margin reaches the same row
    assert np.array_equal(s[1][: s[0][1]], idx[: off[1]])


# ---- the tiles of a camera hold every sphere their pixels' rays hit
@pytest.mark.parametrize("name,h,w,th,tw", [("rgbbox", 120, 120, 8, 8), ("irreg", 96, 128, 8, 8), ("irreg", 50, 70, 5, 7)])
def test_tile_frusta_hold_what_their_rays_hit(name, h, w, th, tw):
    import raytracers_amd as R
    sc = O.OracleScene(name)
    L = sc.arrays()["L"]
    cam = sc.camera_floats(h, w)
    idx, _ = sc.objs_hit_rays(RQ.camera_rays(cam, h, w), 0.0, 1e9)
    planes = R.tile_frusta(cam, h, w, th, tw)
    ty, tx = -(-h // th), -(-w // tw)
    assert planes.shape == (ty * tx, 4, 4) and planes.dtype == F
    rows, cols = np.divmod(np.arange(h * w), w)
    tile = (rows // th) * tx + cols // tw
    hit = idx >= 0
    assert hit.sum() > h * w // 4
    off, pi, _ = PL.in_planes(L, planes, 0.0)
    member = np.zeros((ty * tx, L.shape[0]), bool)
    member[np.repeat(np.arange(ty * tx), np.diff(off)), pi] = True
    g = PL.gaps(L, planes)
    print(f"{name} {w}x{h}: {int(hit.sum())} hits, worst gap of a hit sphere {float(g[tile[hit], idx[hit]].max()):.3f}, "
          f"spheres per tile {off[-1] / (ty * tx):.1f} of {L.shape[0]}")
    missed = int((~member[tile[hit], idx[hit]]).sum())
    assert missed == 0, missed
    assert off[-1] / (ty * tx) < 0.05 * L.shape[0]                             # and the rows are short: the query culls


def test_helper_premises():
    import raytracers_amd as R
    for name, h, w in (("rgbbox", 120, 120), ("irreg", 96, 128)):
        cam = O.OracleScene(name).camera_floats(h, w).astype(np.float64)
        o, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
        for args in ((), (0.25, 0.5, 0.125, 0.75)):
            p4 = R.frustum_planes(cam, *args)
            p6 = R.frustum_planes(cam, *args, near=1.0, far=500.0)
            p5 = R.frustum_planes(cam, *args, far=500.0)
            assert p4.shape == (4, 4) and p5.shape == (5, 4) and p6.shape == (6, 4) and p6.dtype == F
            assert np.array_equal(p4, p6[:4]) and np.array_equal(p5[4], p6[5])
            n = p6[:, :3].astype(np.float64)
            assert (np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0) <= 2.0 ** -23).all()      # unit normals, to float32 rounding
            u0, u1, v0, v1 = args or (0.0, 1.0, 0.0, 1.0)
            mid = llc + 0.5 * (u0 + u1) * hor + 0.5 * (v0 + v1) * ver - o
            x = o + mid
            depth = n @ x + p6[:, 3]
            assert (depth[:4] > 0).all()                                      # the central ray is inside all four side planes ...
            assert (np.abs(n[:4] @ o + p6[:4, 3]) <= 1e-4 * (1.0 + np.abs(o).max())).all()   # ... which pass through the origin
            f = np.cross(hor, ver)
            f = f / np.sqrt(f @ f) * np.sign(np.cross(hor, ver) @ (llc - o))
            assert np.allclose(n[4], f, atol=1e-6) and np.allclose(n[5], -f, atol=1e-6)
            for dist, inside in ((0.5, [False, True]), (10.0, [True, True]), (600.0, [True, False])):
                y = o + dist * f
                assert ((n[4:] @ y + p6[4:, 3]) >= 0).tolist() == inside
        t = R.tile_frusta(cam, h, w, 8, 8)
        assert np.array_equal(t[0], R.frustum_planes(cam, 0.0, 8 / w, (h - 8) / h, 1.0))            # tile 0: the top-left corner
        assert np.array_equal(t[-1], R.frustum_planes(cam, (w - 8) / w, 1.0, 0.0, 8 / h))
    with pytest.raises(ValueError):
        R.tile_frusta(cam, 0, 8, 8, 8)


# ---- the node test's counterexample search
def _bound_check(*args):
    exe = os.path.join(ROOT, "build", "plane_query_bound_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/plane_query_bound_check"], check=True, capture_output=True)
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bound_check_finds_no_counterexample(seed):
    r = _bound_check(300, seed)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "R1 violations 0" in r.stdout and "safety violations 0" in r.stdout, r.stdout
    assert " 0 tall scenes" not in r.stdout and " 0 scaled normals" not in r.stdout and " 0 axis normals" not in r.stdout, r.stdout


def test_bound_check_sees_missing_slack():
    # the same search without the slack must find node boxes that would drop a selected sphere -- the check can fail
    r = _bound_check(100, 2, 0.0)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout and "R1 violations 0" in r.stdout, r.stdout


def test_bound_check_sees_partial_boxes():
    # ... and so must testing the partial boxes near the root of trees taller than the AABB propagation's sweeps
    r = _bound_check(100, 3, 1.0, 1)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout and "R1 violations 0" in r.stdout, r.stdout


# ---- presence
def test_library_exports_planes():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym, nargs in {"rt_spheres_in_planes_count": 9, "rt_spheres_in_planes_fill": 13}.items():
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
        assert len(getattr(_lib.lib, sym).argtypes) == nargs, sym
    for name in ("spheres_in_planes", "spheres_in_planes_count_into", "spheres_in_planes_fill_into", "frustum_planes", "tile_frusta"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.spheres_in_planes).parameters) == ["prepared", "planes", "margin", "first", "gaps", "rows"]
    assert inspect.signature(R.spheres_in_planes).parameters["margin"].default == 0.0
    assert list(inspect.signature(R.frustum_planes).parameters) == ["cam12", "u0", "u1", "v0", "v1", "near", "far"]
    assert list(inspect.signature(R.tile_frusta).parameters) == ["cam12", "h", "w", "tile_h", "tile_w"]


def test_header_declares_planes():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_spheres_in_planes_count(", "rt_spheres_in_planes_fill("):
        assert sym in h, sym
    assert "family=planes count|fill k=K" in h and "CONSERVATIVE" in h and "superset of the box row" in h and "2^-40 <= len <= 2^40" in h
