"""Sphere casts on the GPU: rt_sweep_spheres and rt_sweep_spheres_ranged against the numpy restatement (sweep_ref.py), bit for bit, against
rt_multi_hit_rays at radius 0 on the same rays, and the ranged entry's invalid queries, exclusions, variants, refusals and edges."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as V
import occlusion_ref as X
import ray_query_ref as Q
import sweep_ref as S
from test_ray_intervals_gpu import INTERVALS

pytestmark = pytest.mark.gpu

F = np.float32
KS = (1, 3, 8, 32)          # the list capacities 4, 8 and 32, and k = 3, which is not one of them
SCENES = ("rgbbox", "irreg", "big")   # big: the 10^6-sphere floor, a tree taller than 15 levels
RADII = (0.0, 3.0, 40.0)    # none, the scenes' typical sphere radius, and one that spans many spheres


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


def _prefix(res, k):
    count, index, start, hit = res
    return count, index[:, :k], start[:, :k], hit[:, :k]


def _assert_same(got, want, what):
    for name, g, w in zip(("count", "index", "start", "hit7"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} queries, first {bad[:5]}"


def _scene(R, ctx, spec, size=100):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(size, size, scene)
    return scene, ps, ps.bvh_arrays()


def _restate(arr, rays, radius, t_min, t_max, k, exclude=None):
    # the restatement on the prepared scene's own BVH: the dense form, or for the 10^6-sphere floor the breadth-first one (the CPU suite
    # holds the two equal)
    o, d = rays[:, :3], rays[:, 3:]
    if arr["L"].shape[0] > 4096:
        return S.sweep_walk(arr, o, d, radius, t_min, t_max, k, exclude)
    return S.sweep(Q.RefScene(arr), o, d, radius, t_min, t_max, k, exclude)


def _free(scene, ps):
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec", SCENES)
def test_against_restatement(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec)
    sets = {"seeded": X.seeded_rays(arr, 2048, seed=17), "camera": R.camera_rays(ps, 40, 40)}
    starts = entries = 0
    for name, rays in sets.items():
        for t0, t1 in INTERVALS:
            for radius in RADII:
                want = _restate(arr, rays, radius, t0, t1, max(KS))
                starts += int(want[2].sum())
                entries += int(((want[1] >= 0) & (want[2] == 0)).sum())
                if (t0, t1) == (0.0, 1e9) and name == "seeded":
                    assert want[0].max() > 8 and 0 < (want[0] > 0).mean() <= 1, (spec, radius)
                for k in KS:
                    got = R.sweep_spheres(ps, rays, radius, k, t0, t1)
                    assert ctx.last_launch == f"family=sweep k={k}", ctx.last_launch
                    _assert_same(got, _prefix(want, k), f"{spec} {name} radius {radius} ({t0}, {t1}) k={k}")
    assert starts > 100 and entries > 100, (starts, entries)
    _free(scene, ps)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_radius_zero_against_multi_hit_on_the_device(R, ctx, spec):
    # radius 0 walks multi-hit's leaves: the entry contacts are its root-1 crossings, in its order, with its t and its hit record (the
    # normal's 1 / R is then 1 / radius); every other contact is an overlap at the start, at tau = t_min
    scene, ps, arr = _scene(R, ctx, spec, 128)
    rays = np.concatenate([R.camera_rays(ps, 64, 64), X.seeded_rays(arr, 4096, seed=5)])
    checked = 0
    for t0, t1 in INTERVALS + ((0.5, 30.0),):
        mc, mi, mr, mh = R.multi_hit_rays(ps, rays, 32, t0, t1)
        for radius in (0.0, -0.0):
            sc, si, ss, sh = R.sweep_spheres(ps, rays, radius, 32, t0, t1)
            n_entry = ((mr == 1) & (mi >= 0)).sum(axis=1)
            fits = (mc <= 32) & (sc <= 32)
            assert np.array_equal(((ss == 0) & (si >= 0)).sum(axis=1)[fits], n_entry[fits]), f"{spec} ({t0}, {t1}): entry contact counts"
            for i in np.nonzero(fits & (n_entry > 0))[0][:1500]:
                a, b = (mr[i] == 1) & (mi[i] >= 0), (ss[i] == 0) & (si[i] >= 0)
                assert np.array_equal(mi[i][a], si[i][b]) and np.array_equal(_bits(mh[i][a]), _bits(sh[i][b])), (spec, t0, t1, i)
                checked += 1
            over = (ss == 1)
            assert (sh[over][:, 0] == F(t0)).all()
    assert checked > 1000
    _free(scene, ps)


@pytest.mark.parametrize("spec", SCENES)
def test_ranged_mixed_and_invalid_queries(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec)
    rays = X.seeded_rays(arr, 2048, seed=31)
    n = rays.shape[0]
    lo, hi, b1 = V.mixed_intervals(n, seed=11)
    radii = np.asarray(RADII, F)
    b2 = np.random.default_rng(12).integers(0, len(RADII), n)
    rq = radii[b2].copy()
    bad = [(np.nan, 1e9, 3.0), (0.1, np.nan, 3.0), (0.1, np.inf, 3.0), (-np.inf, 1e9, 3.0), (-1.0, 1e9, 3.0), (5.0, 4.0, 3.0), (0.1, 2e9, 3.0),
           (0.0, 1e9, np.nan), (0.0, 1e9, np.inf), (0.0, 1e9, -np.inf), (0.0, 1e9, -1.0), (0.0, 1e9, 2e9)]
    full = R.sweep_spheres(ps, rays, 3.0, 1, 0.0, 1e9)[0]
    where = np.nonzero(full > 0)[0][3::41][:len(bad)]
    assert where.size == len(bad)
    for i, (a, b, c) in zip(where, bad):
        lo[i], hi[i], rq[i] = a, b, c
    neg0 = np.setdiff1d(np.nonzero(lo == 0.0)[0][::7], where)
    lo[neg0] = -0.0
    negr = np.setdiff1d(np.nonzero(rq == 0.0)[0][::5], where)
    rq[negr] = -0.0
    ok = S.query_ok(lo, hi, rq)
    assert ok.sum() == n - len(bad)
    for k in (3, 32):
        got = R.sweep_spheres(ps, rays, rq, k, lo, hi)
        assert ctx.last_launch == f"family=sweep k={k} (per-query)", ctx.last_launch
        _assert_same(got, _restate(arr, rays, rq, lo, hi, k), f"{spec} k={k} mixed")
        count, index, start, hit = got
        assert not count[where].any() and (index[where] == -1).all() and not start[where].any() and not hit[where].any()
        # bucket by bucket the scalar entry on the same rays
        for a in np.unique(b1):
            for b in range(len(RADII)):
                m = (b1 == a) & (b2 == b) & ok
                t0, t1 = abs(float(lo[m][0])), float(hi[m][0])   # (-0.0 in the (0, 1e9) bucket)
                want = R.sweep_spheres(ps, rays[m], float(radii[b]), k, t0, t1)
                assert ctx.last_launch == f"family=sweep k={k}"
                _assert_same(tuple(g[m] for g in got), want, f"{spec} k={k} bucket ({t0}, {t1}) radius {radii[b]}")
    # a scalar next to an array is broadcast
    _assert_same(R.sweep_spheres(ps, rays, 3.0, 4, lo, 1e9), _restate(arr, rays, 3.0, lo, 1e9, 4), f"{spec} scalar radius, array t_min")
    _free(scene, ps)


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), F)
    s[:, 0:3] = rng.uniform(-30, 30, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 0.9, (n, 3))
    s[:, 6] = rng.uniform(0.2, 1.5, n)
    return s, ((0.0, 0.0, 90.0), (0.0, 0.0, 0.0), 60.0)


def test_exclude_self_sweep_and_update(R, ctx):
    # a scene sweeps its own spheres: query i is the centre and radius of L[i], d its displacement, exclude = i
    spheres, view = _cloud(3000, 7)
    ps = R.prepare_scene_from_spheres(ctx, spheres, 64, 64, *view)
    k = 5
    for step in range(2):
        arr = ps.bvh_arrays()
        L = arr["L"]
        n = L.shape[0]
        d = np.random.default_rng(21 + step).normal(size=(n, 3)).astype(F) * F(2.0)
        rays = np.concatenate([L[:, :3], d], axis=1).astype(F)
        me = np.arange(n)
        got = R.sweep_spheres(ps, rays, L[:, 6].copy(), k, exclude=me)
        assert ctx.last_launch == f"family=sweep k={k} (per-query) exclude", ctx.last_launch
        _assert_same(got, _restate(arr, rays, L[:, 6], 0.0, 1.0, k, me), f"self-sweep step {step}")
        assert not (got[1] == me[:, None]).any(), "a query reports itself"
        assert (got[0] > 0).mean() > 0.2
        # without the exclusion a query whose own leaf is consulted finds itself, as an overlap at the start (R = 2 r: t1 < 0 < t2);
        # removing i from that answer with k + 1 slots gives the excluded answer
        cnt, idx, start, hit = R.sweep_spheres(ps, rays, L[:, 6].copy(), k + 1, 0.0, 1.0)
        assert ctx.last_launch == f"family=sweep k={k + 1} (per-query)", ctx.last_launch
        own = S.contact_kinds(Q.RefScene(arr), rays[:, :3], rays[:, 3:], L[:, 6], 0.0, 1.0)[me, me]
        assert set(np.unique(own)) <= {0, 2} and (own == 2).mean() > 0.5
        assert np.array_equal(got[0], cnt - (own == 2))
        mine = idx == me[:, None]
        assert (start[mine] == 1).all() and mine.sum(axis=1).max() == 1
        for i in range(n):
            keep = ~mine[i]
            for name, g, w in (("index", got[1], idx), ("start", got[2], start), ("hit7", got[3], hit)):
                assert np.array_equal(_bits(g[i]), _bits(w[i][keep][:k])), f"step {step} query {i}: {name} differs from the un-excluded answer without i"
        # excludes outside [0, n) change nothing
        out = np.where(me % 2 == 0, -1 - me, n + me)
        _assert_same(R.sweep_spheres(ps, rays, L[:, 6].copy(), k + 1, exclude=out), (cnt, idx, start, hit), f"step {step}: out-of-range excludes")
        # the next step: the spheres move and change size; the answers follow the new scene
        if step == 0:
            moved = spheres.copy()
            moved[:, 0:3] += np.random.default_rng(9).uniform(-4, 4, (n, 3)).astype(F)
            moved[:, 6] *= np.random.default_rng(10).uniform(0.6, 1.4, n).astype(F)
            before = got
            ps.update_spheres(moved)
            after = R.sweep_spheres(ps, rays, L[:, 6].copy(), k, exclude=me)
            assert not np.array_equal(after[1], before[1]), "the answers did not follow the update"
            fresh = R.prepare_scene_from_spheres(ctx, moved, 64, 64, *view)
            _assert_same(after, R.sweep_spheres(fresh, rays, L[:, 6].copy(), k, exclude=me), "updated scene against a fresh one")
            fresh.free()
    ps.free()


def test_optional_outputs(R, ctx):
    import torch
    scene, ps, arr = _scene(R, ctx, "irreg")
    rays_np = X.seeded_rays(arr, 1000, seed=3)
    rays = torch.from_numpy(rays_np).cuda()
    n, k = rays.shape[0], 5
    lo, hi, _ = V.mixed_intervals(n, seed=9)
    rq = np.random.default_rng(4).uniform(0, 5, n).astype(F)
    ex = np.random.default_rng(5).integers(0, arr["L"].shape[0], n).astype(np.int32)
    lo_t, hi_t, rq_t, ex_t = (torch.from_numpy(a).cuda() for a in (lo, hi, rq, ex))
    for ranged in (False, True):
        want = R.sweep_spheres(ps, rays_np, rq, k, lo, hi, exclude=ex) if ranged else R.sweep_spheres(ps, rays_np, 2.0, k, 0.1, 1e9)
        for missing in range(4):
            outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), -7, dtype=torch.int32, device="cuda"),
                    torch.full((n, k), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n, k, 7), -7.0, dtype=torch.float32, device="cuda")]
            ptrs = [None if i == missing else t.data_ptr() for i, t in enumerate(outs)]
            torch.cuda.synchronize()
            if ranged:
                R.sweep_spheres_ranged_into(rays.data_ptr(), n, ps, rq_t.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), k, *ptrs,
                                            exclude_ptr=ex_t.data_ptr())
            else:
                R.sweep_spheres_into(rays.data_ptr(), n, ps, 2.0, k, *ptrs, t_min=0.1, t_max=1e9)
            ctx.sync()
            for i, (t, w) in enumerate(zip(outs, want)):
                g = t.cpu().numpy()
                if i == missing:
                    sentinel = 0xAB if i == 2 else -7
                    assert (g == sentinel).all(), f"ranged={ranged}: output {i} was written though its pointer is NULL"
                else:
                    assert np.array_equal(_bits(g), _bits(w)), f"ranged={ranged}, output {missing} NULL: output {i} differs"
    # torch tensors for the rays, the per-query values and the excludes are used in place
    _assert_same(R.sweep_spheres(ps, rays, rq_t, k, lo_t, hi, exclude=ex_t), R.sweep_spheres(ps, rays_np, rq, k, lo, hi, exclude=ex), "torch inputs")
    _free(scene, ps)


def test_every_variant_same_outputs(R, ctx):
    scene, ps, arr = _scene(R, ctx, "rgbbox")
    rays = X.seeded_rays(arr, 2048, seed=23)
    lo, hi, _ = V.mixed_intervals(rays.shape[0], seed=4)
    rq = np.random.default_rng(6).uniform(0, 6, rays.shape[0]).astype(F)
    ex = np.random.default_rng(7).integers(0, arr["L"].shape[0], rays.shape[0])
    ctx.set_variant(R.VARIANT_AUTO)
    want = R.sweep_spheres(ps, rays, 3.0, 8, 0.0, 1e9)
    want_r = R.sweep_spheres(ps, rays, rq, 8, lo, hi, exclude=ex)
    try:
        for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_AUTO):
            ctx.set_variant(variant)
            _assert_same(R.sweep_spheres(ps, rays, 3.0, 8, 0.0, 1e9), want, f"variant {variant}")
            assert ctx.last_launch == "family=sweep k=8"
            _assert_same(R.sweep_spheres(ps, rays, rq, 8, lo, hi, exclude=ex), want_r, f"variant {variant} per-query")
            assert ctx.last_launch == "family=sweep k=8 (per-query) exclude"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


def test_query_count_edges(R, ctx):
    import torch
    scene, ps, _ = _scene(R, ctx, "irreg", 64)
    n_max, k = 4097, 3
    rays = torch.empty((n_max, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), 17, 241, ps)            # 4097 rays
    lo_np, hi_np, _ = V.mixed_intervals(n_max, seed=19)
    rq_np = np.random.default_rng(2).uniform(0, 4, n_max).astype(F)
    lo, hi, rq = torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda(), torch.from_numpy(rq_np).cuda()
    rays_np = rays.cpu().numpy()
    want = {False: R.sweep_spheres(ps, rays_np, 1.5, k, 0.1, 1e9), True: R.sweep_spheres(ps, rays_np, rq_np, k, lo_np, hi_np)}
    for ranged in (False, True):
        for n in (0, 1, 63, 64, 65, 130, 4097):
            cnt = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
            idx = torch.full((n + 1, k), -7, dtype=torch.int32, device="cuda")
            start = torch.full((n + 1, k), 0xAB, dtype=torch.uint8, device="cuda")
            hit = torch.full((n + 1, k, 7), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ptrs = (cnt.data_ptr(), idx.data_ptr(), start.data_ptr(), hit.data_ptr())
            if ranged:
                R.sweep_spheres_ranged_into(rays.data_ptr(), n, ps, rq.data_ptr(), lo.data_ptr(), hi.data_ptr(), k, *ptrs)
            else:
                R.sweep_spheres_into(rays.data_ptr(), n, ps, 1.5, k, *ptrs, t_min=0.1, t_max=1e9)
            ctx.sync()
            got = [t.cpu().numpy() for t in (cnt, idx, start, hit)]
            assert got[0][n] == -7 and (got[1][n] == -7).all() and (got[2][n] == 0xAB).all() and (got[3][n] == -7.0).all(), \
                f"n={n} ranged={ranged}: the record past the output was written"
            if n == 0:
                assert ctx.last_launch == "family=none (no rays)"
                continue
            assert ctx.last_launch == f"family=sweep k={k}" + (" (per-query)" if ranged else "")
            _assert_same([g[:n] for g in got], [w[:n] for w in want[ranged]], f"n={n} ranged={ranged}")
    _free(scene, ps)


def test_refusals(R, ctx):
    import torch
    from raytracers_amd._lib import lib
    scene, ps, _ = _scene(R, ctx, "rgbbox", 8)
    rays = torch.from_numpy(R.camera_rays(ps, 8, 8)).cuda()
    lo = torch.zeros(64, dtype=torch.float32, device="cuda")
    hi = torch.full((64,), 1e9, dtype=torch.float32, device="cuda")
    rq = torch.full((64,), 1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((64 * 32,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rp, lp, hp, qp = (C.c_void_p(t.data_ptr()) for t in (rays, lo, hi, rq))
    cp, ip = C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr())
    ctx.sync()
    R.sweep_spheres(ps, rays, 1.0)
    launched = ctx.last_launch

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        assert ctx.last_launch == launched, f"{what}: something was launched"
        ctx.sync()
        assert (cnt.cpu().numpy() == -7).all(), f"{what}: the count output was written"
        assert (idx.cpu().numpy() == -7).all(), f"{what}: the index output was written"

    nan, inf = float("nan"), float("inf")
    for name, n, r, k, outs in (("n < 0", -1, rp, 4, (cp, ip)), ("n = 2^31", 1 << 31, rp, 4, (cp, ip)), ("NULL rays", 64, None, 4, (cp, ip)),
                                ("all outputs NULL", 64, rp, 4, (None, None)), ("k = 0", 64, rp, 0, (cp, ip)), ("k = -1", 64, rp, -1, (cp, ip)),
                                ("k = 33", 64, rp, 33, (cp, ip))):
        refused(lib.rt_sweep_spheres(ctx._h, ps._h, n, r, 1.0, 0.0, 1e9, k, *outs, None, None), f"scalar: {name}")
        refused(lib.rt_sweep_spheres_ranged(ctx._h, ps._h, n, r, qp, lp, hp, None, k, *outs, None, None), f"ranged: {name}")
    for t0, t1 in ((nan, 1e9), (0.0, nan), (-1.0, 1e9), (0.0, inf), (2.0, 1.0), (0.0, 2e9)):
        refused(lib.rt_sweep_spheres(ctx._h, ps._h, 64, rp, 1.0, t0, t1, 4, cp, ip, None, None), f"scalar interval ({t0}, {t1})")
    for radius in (nan, inf, -inf, -1.0, 2e9):
        refused(lib.rt_sweep_spheres(ctx._h, ps._h, 64, rp, radius, 0.0, 1.0, 4, cp, ip, None, None), f"scalar radius {radius}")
    refused(lib.rt_sweep_spheres_ranged(ctx._h, ps._h, 64, rp, None, lp, hp, None, 4, cp, ip, None, None), "ranged: NULL radius")
    refused(lib.rt_sweep_spheres_ranged(ctx._h, ps._h, 64, rp, qp, None, hp, None, 4, cp, ip, None, None), "ranged: NULL t_min")
    refused(lib.rt_sweep_spheres_ranged(ctx._h, ps._h, 64, rp, qp, lp, None, None, 4, cp, ip, None, None), "ranged: NULL t_max")
    refused(lib.rt_sweep_spheres(ctx._h, None, 64, rp, 1.0, 0.0, 1e9, 4, cp, ip, None, None), "NULL prepared scene")
    # radius 1e9 and -0.0 are accepted
    assert lib.rt_sweep_spheres(ctx._h, ps._h, 64, rp, 1e9, 0.0, 1.0, 1, None, None, None, C.c_void_p(idx.data_ptr())) == 0
    assert lib.rt_sweep_spheres(ctx._h, ps._h, 64, rp, -0.0, -0.0, 1.0, 1, None, None, None, C.c_void_p(idx.data_ptr())) == 0
    ctx.sync()
    # n == 0 launches nothing, even with k = 32
    assert lib.rt_sweep_spheres(ctx._h, ps._h, 0, rp, 1.0, 0.0, 1e9, 32, cp, ip, None, None) == 0
    assert ctx.last_launch == "family=none (no rays)"
    R.sweep_spheres(ps, rays, 1.0)
    assert lib.rt_sweep_spheres_ranged(ctx._h, ps._h, 0, rp, qp, lp, hp, None, 32, cp, ip, None, None) == 0
    assert ctx.last_launch == "family=none (no rays)"
    got = R.sweep_spheres(ps, np.zeros((0, 6), F), 1.0, 4)
    assert [g.shape for g in got] == [(0,), (0, 4), (0, 4), (0, 4, 7)]
    # Python: k out of range and bad scalars are RtError; a wrong shape is a ValueError
    for k in (0, 33):
        with pytest.raises(R.RtError):
            R.sweep_spheres(ps, rays, 1.0, k)
    for radius, t0, t1 in ((nan, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, -1.0, np.ones(64, F)), (np.ones(64, F), 0.0, 2e9), (2e9, np.zeros(64, F), 1.0)):
        with pytest.raises(R.RtError):
            R.sweep_spheres(ps, rays, radius, 4, t0, t1)
    # a scalar interval is held to the scalar rule as a pair on the ranged path too (reached through exclude or an array radius)
    for kw in ({"exclude": np.zeros(64, np.int32)}, {}):
        with pytest.raises(R.RtError):
            R.sweep_spheres(ps, rays, 1.0 if kw else np.ones(64, F), 4, 2.0, 1.0, **kw)
    with pytest.raises(R.RtError):
        R.sweep_spheres(ps, rays, 1.0, 4, 2.0, 1.0)
    with pytest.raises(ValueError):
        R.sweep_spheres(ps, rays, np.zeros(63, F), 4)
    with pytest.raises(ValueError):
        R.sweep_spheres(ps, rays, 1.0, 4, exclude=np.zeros(63, np.int32))
    with pytest.raises(ValueError):
        R.sweep_spheres(ps, rays, 1.0, 4, exclude=np.zeros(64, F))
    _free(scene, ps)
    # a multi-device context (a device listed twice) is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    bp = C.c_void_p(mb.ptr)
    assert lib.rt_sweep_spheres(mc._h, mps._h, 4, bp, 1.0, 0.0, 1e9, 4, bp, None, None, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    assert lib.rt_sweep_spheres_ranged(mc._h, mps._h, 4, bp, bp, bp, bp, None, 4, bp, None, None, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()


def test_existing_launch_strings_unchanged(R, ctx):
    scene, ps, _ = _scene(R, ctx, "rgbbox")
    rays = R.camera_rays(ps, 32, 32)
    try:
        ctx.set_variant(R.VARIANT_PIXEL)
        R.multi_hit_rays(ps, rays, 8, 0.1, 1e9)
        before = ctx.last_launch
        assert before == "family=multi-hit k=8"
        R.sweep_spheres(ps, rays, 2.0, 32, 0.1, 1e9)
        assert ctx.last_launch == "family=sweep k=32"
        R.multi_hit_rays(ps, rays, 8, 0.1, 1e9)
        assert ctx.last_launch == before
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)
