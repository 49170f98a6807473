"""Proximity queries on the GPU: rt_nearest_spheres and rt_nearest_spheres_ranged against the numpy restatement (proximity_ref.py), bit for
bit (count, index, gap bits), in count mode and in k-nearest (pruned) mode, on the reference's scenes, random scenes of every GPU-builder size
class, point clouds and adversarial inputs; self-contacts mapped through rt_prepared_get_sphere_ids; refusals and launch strings; and the
sphere ids themselves (both builders, update_spheres, prepare_scene_from_spheres)."""
import numpy as np
import pytest

import oracle_lib as O
import proximity_ref as P

pytestmark = pytest.mark.gpu

F = np.float32
KS = (1, 3, 8, 32)


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import raytracers_amd
    return raytracers_amd


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _assert_same(got, want, what, count=True):
    names = ("count", "index", "gap")
    for name, g, w in zip(names, got, want):
        if name == "count" and not count:
            assert g is None, what
            continue
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} points, first {bad[:5]}: got {g[bad[:2]]} want {w[bad[:2]]}"


def _random_spheres(n, seed, r_lo=0.3, r_hi=2.0):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), F)
    ext = 10.0 * max(1.0, float(n) ** (1.0 / 3.0))
    s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(r_lo, r_hi, n)
    return s


VIEW = ((0.0, 5.0, 40.0), (0.0, 0.0, 0.0), 50.0)


def _points(L, m, seed):
    """points in and around the scene's box; a quarter at centres, a quarter on surfaces (rounded to float32)"""
    rng = np.random.default_rng(seed)
    lo, hi = L[:, :3].min(axis=0).astype(np.float64), L[:, :3].max(axis=0).astype(np.float64)
    pad = 0.1 * (hi - lo) + 1.0
    p = rng.uniform(lo - pad, hi + pad, (m, 3)).astype(F)
    j = rng.integers(0, L.shape[0], m // 4)
    p[: j.size] = L[j, :3]
    d = rng.normal(size=(m // 4, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    j2 = rng.integers(0, L.shape[0], m // 4)
    p[j.size: j.size + j2.size] = (L[j2, :3] + d * L[j2, 6:7]).astype(F)
    return p


def _restate(L, p, md, k):
    # the dense brute force, or for the 10^6-sphere floor the restricted one (the CPU suite holds the two equal)
    if L.shape[0] > 200000:
        return P.nearest_near(L, p, md, k)
    return P.nearest(L, p, md, k, chunk=max(8, min(256, (1 << 22) // L.shape[0])))


def _check_all_modes(R, ctx, ps, L, p, md, what, ks=KS):
    want = _restate(L, p, md, max(ks))
    ranged = np.ndim(md) > 0
    for k in ks:
        w = (want[0], want[1][:, :k], want[2][:, :k])
        got = R.nearest_spheres(ps, p, k, md)
        assert ctx.last_launch == f"family=nearest k={k}" + (" (per-point)" if ranged else ""), ctx.last_launch
        _assert_same(got, w, f"{what} k={k}")
        got = R.nearest_spheres(ps, p, k, md, count=False)
        assert ctx.last_launch == f"family=nearest k={k} pruned" + (" (per-point)" if ranged else ""), ctx.last_launch
        _assert_same(got, w, f"{what} k={k} pruned", count=False)
    return want


@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "big"])
def test_reference_scenes(R, ctx, spec):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(100, 100, scene)
    A = ps.bvh_arrays()
    L = A["L"]
    if spec != "big":
        assert L.tobytes() == O.OracleScene(spec).arrays()["L"].tobytes()
    else:
        assert ps.height > 15
    m = 1024 if spec != "big" else 768
    p = _points(L, m, 3)
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    bounds = [0.0, 0.01 * ext, 1e9] if spec != "big" else [0.0, 0.002 * ext, 30.0]
    for md in bounds:
        want = _check_all_modes(R, ctx, ps, L, p, md, f"{spec} max_dist={md}")
        if md == bounds[1]:
            assert (want[0] > 1).any() and (want[0] == 0).any(), spec
    rng = np.random.default_rng(8)
    md = rng.uniform(0.0, bounds[1] * 2, m).astype(F)
    _check_all_modes(R, ctx, ps, L, p, md, f"{spec} per-point", ks=(3, 32))
    ps.free()
    scene.free()


# the GPU builder's size classes: one workgroup (<= 768), ranked (<= 24576), chained (<= 131072), one sweep per launch beyond
@pytest.mark.parametrize("n", [2, 3, 767, 768, 769, 24576, 24577, 131073])
def test_random_scenes(R, ctx, n):
    s = _random_spheres(n, n)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, n)
    for md in (0.0, 3.0, 1e9):
        _check_all_modes(R, ctx, ps, L, p, md, f"random:{n} max_dist={md}", ks=(1, 8, 32) if n > 30000 else KS)
    ps.free()


def _geometric(n, seed):
    # geometric spacing along a diagonal: a tree far taller than the floor(log2 n) + 2 sweeps of the AABB propagation, whose top boxes
    # therefore do not contain their subtrees (the walk must not prune there)
    rng = np.random.default_rng(seed)
    t = np.exp2(-0.7 * np.arange(n))
    s = np.zeros((n, 7), F)
    s[:, 0], s[:, 1], s[:, 2] = 100.0 * t, 50.0 * t, -100.0 * t
    s[:, 3:6] = 0.5
    s[:, 6] = 10.0 * t * rng.uniform(0.0, 1.0, n)
    return s


def test_tall_trees(R, ctx):
    import edge_rays as E
    for what, s, view in (("tall1100", E.SCENES["tall1100"][0], E.SCENES["tall1100"][1:]), ("geometric", _geometric(120, 3), VIEW)):
        ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *view)
        n = s.shape[0]
        assert ps.height > int(np.log2(np.float32(n))) + 2, (what, ps.height)
        L = ps.bvh_arrays()["L"]
        p = _points(L, 1024, 41)
        rng = np.random.default_rng(43)
        p[:256] = (L[rng.integers(0, n, 256), :3] * rng.uniform(0.5, 1.5, (256, 1))).astype(F)   # near the small spheres
        for md in (0.0, 0.5, 1e9):
            _check_all_modes(R, ctx, ps, L, p, md, f"{what} max_dist={md}")
        ps.free()


def test_point_cloud(R, ctx):
    # radius 0: k-nearest-neighbour search of the centres
    rng = np.random.default_rng(5)
    s = np.zeros((5000, 7), F)
    s[:, :3] = rng.normal(0.0, 20.0, (5000, 3))
    s[::7, :3] = s[1::7, :3][: s[::7].shape[0]]     # duplicate centres: ties broken by j
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    q = rng.normal(0.0, 25.0, (2048, 3)).astype(F)
    q[:256] = L[rng.integers(0, 5000, 256), :3]
    for md in (1e9, 2.0, 0.0):
        _check_all_modes(R, ctx, ps, L, q, md, f"cloud max_dist={md}")
    ps.free()


def test_adversarial_inputs(R, ctx):
    rng = np.random.default_rng(17)
    s = _random_spheres(600, 17)
    s[300:400] = s[200:300]                         # duplicate spheres: equal gaps, ties by j
    s[400:420, 6] = 0.0                             # radius 0
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, 21)
    # points exactly on surfaces along the axes (c + r e_x is exact for moderate values), at centres, far away
    j = rng.integers(0, 600, 64)
    p[:64] = L[j, :3]
    p[:64, 0] += L[j, 6]
    p[64:96] = L[rng.integers(0, 600, 32), :3]
    p[96:112] = np.float32(1e8) * rng.normal(size=(16, 3)).astype(F)
    for md in (0.0, 1e9, 2.5):
        _check_all_modes(R, ctx, ps, L, p, md, f"adversarial max_dist={md}")
    # a sphere at exactly max_dist: the bound equal to a computed gap, and the float just below it
    g = P.gaps(L, p[200:201])[0]
    for t in (g[g > 0].min(), np.sort(g[g > 0])[5]):
        for md in (float(t), float(np.nextafter(F(t), F(0)))):
            _check_all_modes(R, ctx, ps, L, p, md, f"gap-equal max_dist={md!r}", ks=(1, 8))
    # non-finite points and invalid per-point bounds
    q = p.copy()
    q[[1, 2, 3, 4], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    md = np.full(512, 4.0, F)
    bad = [10, 11, 12, 13, 14, 15]
    md[bad] = [np.nan, np.inf, -np.inf, -1.0, 2e9, 1.0000001e9]
    md[20:30] = -0.0
    for k in (1, 32):
        got = R.nearest_spheres(ps, q, k, md)
        _assert_same(got, P.nearest(L, q, md, k), f"invalid inputs k={k}")
        cnt, idx, gap = got
        assert not cnt[[1, 2, 3, 4] + bad].any() and (idx[[1, 2, 3, 4] + bad] == -1).all() and not gap[[1, 2, 3, 4] + bad].any()
        zero = R.nearest_spheres(ps, q[20:30], k, 0.0)
        _assert_same(tuple(a[20:30] for a in got), zero, "-0.0 bound")
    ps.free()


def test_huge_coordinates(R, ctx):
    s = _random_spheres(800, 23)
    s[:, :3] *= F(1e16)
    s[:, :3] += F(1e18)
    s[:, 6] *= F(1e16)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, (1e18, 1e18, 2e18), (1e18, 1e18, 1e18), 50.0)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, 29)
    for md in (0.0, 1e9):
        _check_all_modes(R, ctx, ps, L, p, md, f"1e18 max_dist={md}", ks=(1, 8))
    ps.free()


def test_self_contacts(R, ctx):
    s = _random_spheres(3000, 31, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    ids = ps.sphere_ids()
    L = ps.bvh_arrays()["L"]
    cnt, idx, gap = R.nearest_spheres(ps, L[:, :3].copy(), 32, L[:, 6].copy())
    assert cnt.max() <= 32
    pairs = set()
    for i in range(L.shape[0]):
        m = int(cnt[i])
        row = idx[i, :m]
        assert i in row.tolist(), i                                    # every sphere touches itself at gap -r
        assert gap[i, 0] <= 0 and _bits(gap[i, list(row).index(i)]) == _bits(-L[i, 6])
        pairs.update((int(ids[i]), int(ids[j])) for j in row)
    assert all((b, a) in pairs for a, b in pairs)                      # symmetric
    # brute force in the caller's order
    g = P.gaps(s, s[:, :3])
    want = set(zip(*np.nonzero(g <= s[:, 6][:, None])))
    assert pairs == {(int(a), int(b)) for a, b in want}
    assert len(pairs) > 3000
    ps.free()


def test_refusals_and_launch(R, ctx):
    import ctypes as C
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    pts = R.api.DeviceBuffer(ctx, 12 * 64)
    out = R.api.DeviceBuffer(ctx, 4 * 64 * 32)
    md = R.api.DeviceBuffer(ctx, 4 * 64)
    try:
        for v in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(v)
            h, p, o, vp = ctx._h, ps._h, out.ptr, C.c_void_p
            bad = [
                lib.rt_nearest_spheres(h, p, -1, vp(pts.ptr), 1.0, 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 1 << 31, vp(pts.ptr), 1.0, 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, None, 1.0, 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), 1.0, 4, None, None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), 1.0, 0, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), 1.0, 33, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), -1.0, 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), float("nan"), 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), float("inf"), 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, p, 64, vp(pts.ptr), 2e9, 4, vp(o), None, None),
                lib.rt_nearest_spheres(h, None, 64, vp(pts.ptr), 1.0, 4, vp(o), None, None),
                lib.rt_nearest_spheres_ranged(h, p, 64, vp(pts.ptr), None, 4, vp(o), None, None),
                lib.rt_nearest_spheres_ranged(h, p, 64, vp(pts.ptr), vp(md.ptr), 4, None, None, None),
                lib.rt_nearest_spheres_ranged(h, p, 64, vp(pts.ptr), vp(md.ptr), 40, vp(o), None, None),
            ]
            for i, rc in enumerate(bad):
                assert rc != 0, (v, i)
                assert lib.rt_last_error(h).decode(), (v, i)
            with pytest.raises(R.RtError):
                R.nearest_spheres(ps, np.zeros((4, 3), F), 4, -0.5)
            assert lib.rt_nearest_spheres(h, p, 0, vp(pts.ptr), 1.0, 4, vp(o), None, None) == 0
            assert ctx.last_launch == "family=none (no points)"
            assert lib.rt_nearest_spheres_ranged(h, p, 0, vp(pts.ptr), vp(md.ptr), 4, None, vp(o), None) == 0
            assert ctx.last_launch == "family=none (no points)"
            q = np.zeros((5, 3), F)
            R.nearest_spheres(ps, q, 5, 1.0)
            assert ctx.last_launch == "family=nearest k=5"
            R.nearest_spheres(ps, q, 5, 1.0, count=False)
            assert ctx.last_launch == "family=nearest k=5 pruned"
            R.nearest_spheres(ps, q, 32, np.ones(5, F))
            assert ctx.last_launch == "family=nearest k=32 (per-point)"
            R.nearest_spheres(ps, q, 2, np.ones(5, F), count=False)
            assert ctx.last_launch == "family=nearest k=2 pruned (per-point)"
            # only one output: the others stay NULL
            assert lib.rt_nearest_spheres(h, p, 5, vp(pts.ptr), 1.0, 4, None, None, vp(o)) == 0
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        for b in (pts, out, md):
            b.free()
        ps.free()
        scene.free()


def _check_ids(ps, s, what):
    ids = ps.sphere_ids()
    n = s.shape[0]
    assert ids.dtype == np.int32 and ids.shape == (n,)
    assert np.array_equal(np.sort(ids), np.arange(n)), f"{what}: not a permutation"
    L = ps.bvh_arrays()["L"]
    assert L.tobytes() == np.ascontiguousarray(s[ids]).tobytes(), f"{what}: L7[i] != spheres[ids[i]]"
    return ids


@pytest.mark.parametrize("n", [2, 600, 768, 769, 5000, 24577, 131073])
def test_sphere_ids(R, n):
    s = _random_spheres(n, 100 + n)
    if n >= 600:
        s[n // 2: n // 2 + 200] = s[10:210]                        # equal Morton keys in runs
    got = {}
    for gpu_build in (1, 0):
        c = R.Context(0)
        c.set_option("gpu_build", gpu_build)
        try:
            sc = c.scene_from_spheres(s, *VIEW)
            ps = R.prepare_scene(64, 64, sc)
            got[gpu_build] = _check_ids(ps, s, f"n={n} gpu_build={gpu_build}")
            ps.free()
            sc.free()
            ps = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            assert np.array_equal(_check_ids(ps, s, f"n={n} device gpu_build={gpu_build}"), got[gpu_build])
            # refreshed by update_spheres: a permutation of the same spheres, and new spheres
            perm = np.random.default_rng(n).permutation(n)
            ps.update_spheres(s[perm])
            _check_ids(ps, s[perm], f"n={n} updated gpu_build={gpu_build}")
            s2 = _random_spheres(n, 7 + n)
            ps.update_spheres(s2)
            _check_ids(ps, s2, f"n={n} updated to new spheres gpu_build={gpu_build}")
            ps.free()
        finally:
            c.close()
    assert np.array_equal(got[0], got[1]), f"n={n}: the builders' ids differ"
    # ascending within a run of equal Morton keys (the oracle's sort keys, for the same L)
    if n <= 24577:
        orc = O.OracleScene("custom", spheres7=s, look_from=VIEW[0], look_at=VIEW[1], fov=VIEW[2]).arrays()
        assert orc["L"].tobytes() == np.ascontiguousarray(s[got[1]]).tobytes()
        key = orc["morton"]
        same = key[1:] == key[:-1]
        if n >= 600:
            assert same.any()
        assert (got[1][1:][same] > got[1][:-1][same]).all()


def test_generator_scene_ids(R, ctx):
    import ctypes as C
    for spec in ("rgbbox", "irreg"):
        orc = O.OracleScene(spec)
        s = np.ctypeslib.as_array(C.cast(orc.scene.spheres, C.POINTER(C.c_float)), shape=(orc.n * 7,)).reshape(orc.n, 7).copy()
        scene = ctx.scene(spec)
        ps = R.prepare_scene(64, 64, scene)
        _check_ids(ps, s, spec)
        ps.free()
        scene.free()
