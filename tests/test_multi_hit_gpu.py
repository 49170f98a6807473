"""Multi-hit queries on the GPU: rt_multi_hit_rays and rt_multi_hit_rays_ranged against the numpy restatement (multi_hit_ref.py), bit for bit,
and against rt_occluded_rays (count > 0) and rt_intersect_rays (crossing 0) run on the same rays."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import ray_query_ref as Q
from test_ray_intervals_gpu import INTERVALS

pytestmark = pytest.mark.gpu

F = np.float32
KS = (1, 3, 8, 32)          # the list capacities 4, 8 and 32, and k = 3, which is not one of them
SCENES = ("rgbbox", "irreg", "big")   # big: the 1000-sphere floor, a tree taller than 15 levels


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
    count, index, root, hit = res
    return count, index[:, :k], root[:, :k], hit[:, :k]


def _assert_same(got, want, what):
    for name, g, w in zip(("count", "index", "root", "hit7"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape {g.shape} != {w.shape}"
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} rays, first {bad[:5]}"


def _scene(R, ctx, spec, size=100):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(size, size, scene)
    return scene, ps, ps.bvh_arrays()


def _restate(arr, rays, t_min, t_max, k):
    # the restatement on the prepared scene's own BVH: the dense form, or for the 10^6-sphere floor the breadth-first one (the CPU suite
    # holds the two equal)
    o, d = rays[:, :3], rays[:, 3:]
    if arr["L"].shape[0] > 4096:
        return M.multi_hit_walk(arr, o, d, t_min, t_max, k)
    return M.multi_hit(Q.RefScene(arr), o, d, t_min, t_max, k)


def _free(scene, ps):
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec", SCENES)
def test_against_restatement(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec)
    sets = {"seeded": X.seeded_rays(arr, 2048, seed=17), "camera": R.camera_rays(ps, 40, 40)}
    for name, rays in sets.items():
        for t0, t1 in INTERVALS:
            want = _restate(arr, rays, t0, t1, max(KS))
            if (t0, t1) == (0.0, 1e9) and name == "seeded":
                assert want[0].max() > 8 and 0 < (want[0] > 0).mean() < 1, spec
            for k in KS:
                got = R.multi_hit_rays(ps, rays, k, t0, t1)
                assert ctx.last_launch == f"family=multi-hit k={k}", ctx.last_launch
                _assert_same(got, _prefix(want, k), f"{spec} {name} ({t0}, {t1}) k={k}")
    _free(scene, ps)


@pytest.mark.parametrize("spec", SCENES)
def test_ranged_mixed_and_invalid_intervals(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec)
    rays = X.seeded_rays(arr, 2048, seed=31)
    n = rays.shape[0]
    lo, hi, bucket = V.mixed_intervals(n, seed=11)
    bad = [(np.nan, 1e9), (0.1, np.nan), (0.1, np.inf), (-np.inf, 1e9), (-1.0, 1e9), (5.0, 4.0), (0.1, 2e9)]
    full = R.multi_hit_rays(ps, rays, 1, 0.0, 1e9)[0]
    where = np.nonzero(full > 0)[0][3::41][:len(bad)]
    assert where.size == len(bad)
    for i, (a, b) in zip(where, bad):
        lo[i], hi[i] = a, b
    neg0 = np.setdiff1d(np.nonzero(lo == 0.0)[0][::7], where)
    lo[neg0] = -0.0
    ok = V.interval_ok(lo, hi)
    assert ok.sum() == n - len(bad)
    for k in (3, 32):
        got = R.multi_hit_rays(ps, rays, k, lo, hi)
        assert ctx.last_launch == f"family=multi-hit k={k} (per-ray)", ctx.last_launch
        _assert_same(got, _restate(arr, rays, lo, hi, k), f"{spec} k={k} mixed")
        count, index, root, hit = got
        assert not count[where].any() and (index[where] == -1).all() and not root[where].any() and not hit[where].any()
        # bucket by bucket the scalar entry on the same rays
        for b in np.unique(bucket):
            m = (bucket == b) & ok
            t0, t1 = abs(float(lo[m][0])), float(hi[m][0])   # (-0.0 in the (0, 1e9) bucket)
            want = R.multi_hit_rays(ps, rays[m], k, t0, t1)
            _assert_same(tuple(g[m] for g in got), want, f"{spec} k={k} bucket ({t0}, {t1})")
    _free(scene, ps)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_device_cross_checks(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec, 128)
    rays = np.concatenate([R.camera_rays(ps, 64, 64), X.seeded_rays(arr, 4096, seed=5)])
    ctx.set_variant(R.VARIANT_PIXEL)
    try:
        for t0, t1 in INTERVALS + ((0.5, 30.0),):
            count = R.multi_hit_rays(ps, rays, 1, t0, t1)[0]
            occ = R.occluded_rays(ps, rays, t0, t1)
            assert np.array_equal(count > 0, occ), f"{spec} ({t0}, {t1}): {int(((count > 0) != occ).sum())} rays differ from occluded_rays"
        for t1 in (1e9, 30.0):
            idx, hit = R.intersect_rays(ps, rays, 0.1, t1)
            count, index, root, mh = R.multi_hit_rays(ps, rays, 3, 0.1, t1)
            small = (idx >= 0) & (hit[:, 0] < 2.0 ** 23)
            assert small.sum() > 100
            assert (count[small] > 0).all()
            assert np.array_equal(index[small, 0], idx[small]), f"{spec} t_max={t1}: crossing 0 is not intersect_rays's hit"
            assert np.array_equal(_bits(mh[small, 0]), _bits(hit[small])), f"{spec} t_max={t1}: hit records differ"
        # the ranged entries agree with each other in the same way
        lo, hi, _ = V.mixed_intervals(rays.shape[0], seed=2)
        count = R.multi_hit_rays(ps, rays, 1, lo, hi)[0]
        assert np.array_equal(count > 0, R.occluded_rays(ps, rays, lo, hi))
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


def test_optional_outputs(R, ctx):
    import torch
    scene, ps, arr = _scene(R, ctx, "irreg")
    rays_np = X.seeded_rays(arr, 1000, seed=3)
    rays = torch.from_numpy(rays_np).cuda()
    n, k = rays.shape[0], 5
    lo, hi, _ = V.mixed_intervals(n, seed=9)
    lo_t, hi_t = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    for ranged in (False, True):
        want = R.multi_hit_rays(ps, rays_np, k, lo, hi) if ranged else R.multi_hit_rays(ps, rays_np, k, 0.1, 1e9)
        for missing in range(4):
            outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), -7, dtype=torch.int32, device="cuda"),
                    torch.full((n, k), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n, k, 7), -7.0, dtype=torch.float32, device="cuda")]
            ptrs = [None if i == missing else t.data_ptr() for i, t in enumerate(outs)]
            torch.cuda.synchronize()
            if ranged:
                R.multi_hit_rays_ranged_into(rays.data_ptr(), n, ps, lo_t.data_ptr(), hi_t.data_ptr(), k, *ptrs)
            else:
                R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, *ptrs, t_min=0.1, t_max=1e9)
            ctx.sync()
            for i, (t, w) in enumerate(zip(outs, want)):
                g = t.cpu().numpy()
                if i == missing:
                    sentinel = 0xAB if i == 2 else -7
                    assert (g == sentinel).all(), f"ranged={ranged}: output {i} was written though its pointer is NULL"
                else:
                    assert np.array_equal(_bits(g), _bits(w)), f"ranged={ranged}, output {missing} NULL: output {i} differs"
    _free(scene, ps)


def test_every_variant_same_outputs(R, ctx):
    scene, ps, arr = _scene(R, ctx, "rgbbox")
    rays = X.seeded_rays(arr, 2048, seed=23)
    lo, hi, _ = V.mixed_intervals(rays.shape[0], seed=4)
    ctx.set_variant(R.VARIANT_AUTO)
    want = R.multi_hit_rays(ps, rays, 8, 0.0, 1e9)
    want_r = R.multi_hit_rays(ps, rays, 8, lo, hi)
    try:
        for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_AUTO):
            ctx.set_variant(variant)
            _assert_same(R.multi_hit_rays(ps, rays, 8, 0.0, 1e9), want, f"variant {variant}")
            assert ctx.last_launch == "family=multi-hit k=8"
            _assert_same(R.multi_hit_rays(ps, rays, 8, lo, hi), want_r, f"variant {variant} per-ray")
            assert ctx.last_launch == "family=multi-hit k=8 (per-ray)"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


def test_ray_count_edges(R, ctx):
    import torch
    scene, ps, _ = _scene(R, ctx, "irreg", 64)
    n_max, k = 4097, 3
    rays = torch.empty((n_max, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), 17, 241, ps)            # 4097 rays
    lo_np, hi_np, _ = V.mixed_intervals(n_max, seed=19)
    lo, hi = torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    rays_np = rays.cpu().numpy()
    want = {False: R.multi_hit_rays(ps, rays_np, k, 0.1, 1e9), True: R.multi_hit_rays(ps, rays_np, k, lo_np, hi_np)}
    for ranged in (False, True):
        for n in (0, 1, 63, 64, 65, 130, 4097):
            cnt = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
            idx = torch.full((n + 1, k), -7, dtype=torch.int32, device="cuda")
            root = torch.full((n + 1, k), 0xAB, dtype=torch.uint8, device="cuda")
            hit = torch.full((n + 1, k, 7), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ptrs = (cnt.data_ptr(), idx.data_ptr(), root.data_ptr(), hit.data_ptr())
            if ranged:
                R.multi_hit_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), k, *ptrs)
            else:
                R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, *ptrs, t_min=0.1, t_max=1e9)
            ctx.sync()
            got = [t.cpu().numpy() for t in (cnt, idx, root, hit)]
            assert got[0][n] == -7 and (got[1][n] == -7).all() and (got[2][n] == 0xAB).all() and (got[3][n] == -7.0).all(), \
                f"n={n} ranged={ranged}: the record past the output was written"
            if n == 0:
                assert ctx.last_launch == "family=none (no rays)"
                continue
            assert ctx.last_launch == f"family=multi-hit k={k}" + (" (per-ray)" if ranged else "")
            _assert_same([g[:n] for g in got], [w[:n] for w in want[ranged]], f"n={n} ranged={ranged}")
    _free(scene, ps)


def test_torch_in_place(R, ctx):
    import torch
    scene, ps, arr = _scene(R, ctx, "irreg")
    rays_np = X.seeded_rays(arr, 2048, seed=13)
    lo_np, hi_np, _ = V.mixed_intervals(2048, seed=17)
    rays, lo, hi = torch.from_numpy(rays_np).cuda(), torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    want = _restate(arr, rays_np, lo_np, hi_np, 4)
    _assert_same(R.multi_hit_rays(ps, rays, 4, lo, hi), want, "torch rays and bounds")
    _assert_same(R.multi_hit_rays(ps, rays, 4, lo, hi_np), want, "torch t_min, numpy t_max")
    _assert_same(R.multi_hit_rays(ps, rays, 4, 0.0, 1e9), _restate(arr, rays_np, 0.0, 1e9, 4), "torch rays")
    _free(scene, ps)


def test_wide_outputs_use_64_bit_offsets(R, ctx):
    # n * k * 7 above 2^31: the last rays' records land at their own place (a 32-bit offset would wrap)
    import torch
    scene, ps, _ = _scene(R, ctx, "rgbbox", 64)
    k = 32
    n = (1 << 31) // (7 * k) + 1000
    assert n * k * 7 > (1 << 31)
    tail = torch.from_numpy(R.camera_rays(ps, 32, 32)).cuda()   # 1024 rays at the end, after copies of the first one
    rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    rays[: n - tail.shape[0]] = tail[0]
    rays[n - tail.shape[0]:] = tail
    hit = torch.zeros((n, k, 7), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, cnt.data_ptr(), None, None, hit.data_ptr())
    ctx.sync()
    want = R.multi_hit_rays(ps, tail, k)
    got_tail = hit[n - tail.shape[0]:].cpu().numpy()
    assert np.array_equal(cnt[n - tail.shape[0]:].cpu().numpy(), want[0])
    assert np.array_equal(_bits(got_tail), _bits(want[3]))
    assert (want[0] > 0).any()
    del hit, rays
    torch.cuda.empty_cache()
    _free(scene, ps)


def test_existing_launch_strings_unchanged(R, ctx):
    scene, ps, _ = _scene(R, ctx, "rgbbox")
    rays = R.camera_rays(ps, 32, 32)
    lo, hi = np.zeros(rays.shape[0], F), np.full(rays.shape[0], 1e9, F)
    try:
        ctx.set_variant(R.VARIANT_PIXEL)
        before = []
        for call in (lambda: R.intersect_rays(ps, rays, 0.1, 1e9), lambda: R.intersect_rays(ps, rays, lo, hi),
                     lambda: R.occluded_rays(ps, rays, 0.1, 1e9), lambda: R.occluded_rays(ps, rays, lo, hi), lambda: R.trace_rays(ps, rays)):
            call()
            before.append(ctx.last_launch)
        assert before == ["family=intersect", "family=intersect (per-ray)", "family=occluded", "family=occluded (per-ray)", "family=pixel (rays)"]
        R.multi_hit_rays(ps, rays, 32, 0.1, 1e9)
        assert ctx.last_launch == "family=multi-hit k=32"
        R.multi_hit_rays(ps, rays, 1, lo, hi)
        assert ctx.last_launch == "family=multi-hit k=1 (per-ray)"
        R.intersect_rays(ps, rays, 0.1, 1e9)
        assert ctx.last_launch == before[0]
        R.intersect_rays(ps, rays, lo, hi)
        assert ctx.last_launch == before[1]
        R.occluded_rays(ps, rays, 0.1, 1e9)
        assert ctx.last_launch == before[2]
        R.occluded_rays(ps, rays, lo, hi)
        assert ctx.last_launch == before[3]
        R.trace_rays(ps, rays)
        assert ctx.last_launch == before[4]
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


def test_refusals(R, ctx):
    import torch
    from raytracers_amd._lib import lib
    scene, ps, _ = _scene(R, ctx, "rgbbox", 8)
    rays = torch.from_numpy(R.camera_rays(ps, 8, 8)).cuda()
    lo = torch.zeros(64, dtype=torch.float32, device="cuda")
    hi = torch.full((64,), 1e9, dtype=torch.float32, device="cuda")
    cnt = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((64 * 32,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rp, lp, hp = C.c_void_p(rays.data_ptr()), C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr())
    cp, ip = C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr())

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        ctx.sync()
        assert (cnt.cpu().numpy() == -7).all(), f"{what}: the count output was written"
        assert (idx.cpu().numpy() == -7).all(), f"{what}: the index output was written"

    nan, inf = float("nan"), float("inf")
    for name, n, r, k, outs in (("n < 0", -1, rp, 4, (cp, ip)), ("n = 2^31", 1 << 31, rp, 4, (cp, ip)), ("NULL rays", 64, None, 4, (cp, ip)),
                                ("all outputs NULL", 64, rp, 4, (None, None)), ("k = 0", 64, rp, 0, (cp, ip)), ("k = -1", 64, rp, -1, (cp, ip)),
                                ("k = 33", 64, rp, 33, (cp, ip))):
        refused(lib.rt_multi_hit_rays(ctx._h, ps._h, n, r, 0.0, 1e9, k, *outs, None, None), f"scalar: {name}")
        refused(lib.rt_multi_hit_rays_ranged(ctx._h, ps._h, n, r, lp, hp, k, *outs, None, None), f"ranged: {name}")
    for t0, t1 in ((nan, 1e9), (0.0, nan), (-1.0, 1e9), (0.0, inf), (2.0, 1.0), (0.0, 2e9)):
        refused(lib.rt_multi_hit_rays(ctx._h, ps._h, 64, rp, t0, t1, 4, cp, ip, None, None), f"scalar interval ({t0}, {t1})")
    refused(lib.rt_multi_hit_rays_ranged(ctx._h, ps._h, 64, rp, None, hp, 4, cp, ip, None, None), "ranged: NULL t_min")
    refused(lib.rt_multi_hit_rays_ranged(ctx._h, ps._h, 64, rp, lp, None, 4, cp, ip, None, None), "ranged: NULL t_max")
    refused(lib.rt_multi_hit_rays(ctx._h, None, 64, rp, 0.0, 1e9, 4, cp, ip, None, None), "NULL prepared scene")
    # n == 0 launches nothing, even with k = 32
    assert lib.rt_multi_hit_rays(ctx._h, ps._h, 0, rp, 0.0, 1e9, 32, cp, ip, None, None) == 0
    assert ctx.last_launch == "family=none (no rays)"
    assert lib.rt_multi_hit_rays_ranged(ctx._h, ps._h, 0, rp, lp, hp, 32, cp, ip, None, None) == 0
    assert ctx.last_launch == "family=none (no rays)"
    # Python: k out of range and bad scalar bounds are RtError; a wrong bound shape is a ValueError
    for k in (0, 33):
        with pytest.raises(R.RtError):
            R.multi_hit_rays(ps, rays, k)
    for t0, t1 in ((nan, 1e9), (-1.0, np.zeros(64, F)), (np.zeros(64, F), 2e9)):
        with pytest.raises(R.RtError):
            R.multi_hit_rays(ps, rays, 4, t0, t1)
    with pytest.raises(ValueError):
        R.multi_hit_rays(ps, rays, 4, np.zeros(63, F), 1.0)
    _free(scene, ps)
    # a multi-device context (a device listed twice) is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    bp = C.c_void_p(mb.ptr)
    assert lib.rt_multi_hit_rays(mc._h, mps._h, 4, bp, 0.0, 1e9, 4, bp, None, None, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    assert lib.rt_multi_hit_rays_ranged(mc._h, mps._h, 4, bp, bp, bp, 4, bp, None, None, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()
