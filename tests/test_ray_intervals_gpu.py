"""Per-ray intervals on the GPU: rt_occluded_rays_ranged under the pooled any-hit loop and the lane kernel, and rt_intersect_rays_ranged,
against the scalar entries run on the same rays (byte for byte) and against the numpy restatement (interval_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import interval_ref as V
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
PER_RAY = " intervals=per-ray"
POOLED_ANY = "family=pooled tickets=rays instantiation=any"
LANE_OCC = "family=occluded (per-ray)"
LANE_INT = "family=intersect (per-ray)"
INTERVALS = ((0.0, 1e9), (0.1, 1e9), (0.1, 30.0), (1e-3, 1.0), (3.0, 3.0))


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


def _families(R):
    # (variant, check of last_launch) for the ranged occlusion entry: the pooled loop in its per-ray mode, the lane kernel, and AUTO -- which
    # takes the lane kernel (api_queries.cpp)
    pooled = lambda s: s.startswith(POOLED_ANY) and s.endswith(PER_RAY)   # noqa: E731
    lane = lambda s: s == LANE_OCC                                        # noqa: E731
    return ((R.VARIANT_POOLED, pooled), (R.VARIANT_PIXEL, lane), (R.VARIANT_AUTO, lane))


def _scene(R, ctx, spec, size=100):
    scene = ctx.scene(spec)
    return scene, R.prepare_scene(size, size, scene)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_constant_arrays_equal_scalar_entry(R, ctx, spec):
    arr = O.OracleScene(spec).arrays()
    scene, ps = _scene(R, ctx, spec)
    sets = {"seeded": X.seeded_rays(arr, 4096, seed=17 if spec == "rgbbox" else 29), "camera": R.camera_rays(ps, 64, 64)}
    try:
        for name, rays in sets.items():
            n = rays.shape[0]
            for t0, t1 in INTERVALS:
                lo, hi = np.full(n, t0, F), np.full(n, t1, F)
                for variant, fam in _families(R):
                    ctx.set_variant(variant)
                    want = R.occluded_rays(ps, rays, t0, t1)
                    scalar_ll = ctx.last_launch
                    got = R.occluded_rays(ps, rays, lo, hi)
                    assert fam(ctx.last_launch), ctx.last_launch
                    if variant == R.VARIANT_POOLED:
                        assert ctx.last_launch == scalar_ll + PER_RAY
                    bad = np.nonzero(got != want)[0]
                    assert bad.size == 0, f"{spec} {name} ({t0}, {t1}) variant {variant}: {bad.size} rays differ, first {bad[:5]}"
                want_i, want_h = R.intersect_rays(ps, rays, t0, t1)
                assert ctx.last_launch == "family=intersect"
                got_i, got_h = R.intersect_rays(ps, rays, lo, hi)
                assert ctx.last_launch == LANE_INT
                assert np.array_equal(got_i, want_i), f"{spec} {name} ({t0}, {t1}): {int((got_i != want_i).sum())} indices differ"
                assert np.array_equal(_bits(got_h), _bits(want_h)), f"{spec} {name} ({t0}, {t1}): hit records differ"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_mixed_intervals_equal_buckets(R, ctx, spec):
    arr = O.OracleScene(spec).arrays()
    ref = Q.RefScene(arr)
    scene, ps = _scene(R, ctx, spec)
    rays = X.seeded_rays(arr, 4096, seed=31)
    lo, hi, k = V.mixed_intervals(rays.shape[0], seed=11)
    want_ref = V.occluded(ref, rays[:, :3], rays[:, 3:], lo, hi)
    want_i_ref, want_h_ref = V.objs_hit(ref, rays[:, :3], rays[:, 3:], lo, hi)
    assert want_ref.any() and not want_ref.all()
    try:
        for variant, fam in _families(R):
            ctx.set_variant(variant)
            got = R.occluded_rays(ps, rays, lo, hi)
            assert fam(ctx.last_launch), ctx.last_launch
            for b in np.unique(k):
                m = k == b
                want = R.occluded_rays(ps, rays[m], float(lo[m][0]), float(hi[m][0]))
                assert np.array_equal(got[m], want), f"{spec} variant {variant} bucket {b}: {int((got[m] != want).sum())} rays differ"
            assert np.array_equal(got, want_ref), f"{spec} variant {variant}: {int((got != want_ref).sum())} rays differ from the restatement"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    got_i, got_h = R.intersect_rays(ps, rays, lo, hi)
    for b in np.unique(k):
        m = k == b
        want_i, want_h = R.intersect_rays(ps, rays[m], float(lo[m][0]), float(hi[m][0]))
        assert np.array_equal(got_i[m], want_i) and np.array_equal(_bits(got_h[m]), _bits(want_h)), f"{spec} bucket {b}"
    assert np.array_equal(got_i, want_i_ref)
    assert np.array_equal(_bits(got_h), _bits(want_h_ref))
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec,size", [("rgbbox", 256), ("irreg", 96)])
def test_normalised_shadow_rays(R, ctx, spec, size):
    arr = O.OracleScene(spec).arrays()
    ref = Q.RefScene(arr)
    scene, ps = _scene(R, ctx, spec, size)
    idx, hit = R.intersect_rays(ps, R.camera_rays(ps, size, size), 0.0, 1e9)
    sh, t_max = V.normalised_shadow_rays(idx, hit, X.LIGHTS[spec])
    want = V.occluded(ref, sh[:, :3], sh[:, 3:], 1e-3, t_max)
    assert 0.1 < want.mean() < 0.9, want.mean()
    try:
        for variant, fam in _families(R):
            ctx.set_variant(variant)
            got = R.occluded_rays(ps, sh, 1e-3, t_max)       # a scalar t_min next to per-ray t_max
            assert fam(ctx.last_launch), ctx.last_launch
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{spec} variant {variant}: {bad.size} shadow rays differ, first {bad[:5]}"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_pooled_shapes_per_ray(R, ctx):
    # every shape of the any-hit loop in its per-ray mode: 16 waves with the whole scene in LDS (rgbbox) and without (irreg), four-wave
    # workgroups, and the spilling box stack at the test capacity (192) on irreg
    cases = (("rgbbox", {}, "waves=16"), ("irreg", {}, "waves=16"), ("irreg", {"wide_waves": 2}, "waves=4"),
             ("irreg", {"wide_waves": 2, "stack_cap": 192}, "+SPILL"))
    ctx.set_variant(R.VARIANT_POOLED)
    try:
        for spec, opts, mark in cases:
            arr = O.OracleScene(spec).arrays()
            ref = Q.RefScene(arr)
            rays = X.seeded_rays(arr, 4096, seed=5)
            lo, hi, _ = V.mixed_intervals(rays.shape[0], seed=23)
            want = V.occluded(ref, rays[:, :3], rays[:, 3:], lo, hi)
            scene, ps = _scene(R, ctx, spec)
            for key, v in opts.items():
                ctx.set_option(key, v)
            try:
                got = R.occluded_rays(ps, rays, lo, hi)
                ll = ctx.last_launch
                scalar = R.occluded_rays(ps, rays, 0.1, 30.0)
                sll = ctx.last_launch
            finally:
                ctx.set_option("wide_waves", 1)
                ctx.set_option("stack_cap", 0)
            assert ll.startswith(POOLED_ANY) and mark in ll and ll.endswith(PER_RAY), (spec, opts, ll)
            assert ("+SPILL" in ll) == ("stack_cap" in opts), (spec, opts, ll)
            assert sll + PER_RAY == ll, (sll, ll)
            assert np.array_equal(got, want), f"{spec} {opts}: {int((got != want).sum())} rays differ ({ll})"
            assert np.array_equal(scalar, X.occluded(ref, rays[:, :3], rays[:, 3:], 0.1, 30.0)), (spec, opts, sll)
            ps.free()
            scene.free()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)


def test_tall_tree_pooled_and_spill_per_ray(R, ctx):
    # a 1000-sphere floor (a tree taller than 15 levels): the sixteen-wave shape and, with the wide shape forced, the spilling box stack at
    # the production capacity, each against the lane kernel and the scalar entry bucket by bucket
    scene = ctx.floor(1000, 6000.0)
    ps = R.prepare_scene(256, 256, scene)
    rays = R.camera_rays(ps, 256, 256)
    lo, hi, k = V.mixed_intervals(rays.shape[0], seed=3)
    try:
        ctx.set_variant(R.VARIANT_PIXEL)
        lane = R.occluded_rays(ps, rays, lo, hi)
        assert ctx.last_launch == LANE_OCC
        assert lane.any() and not lane.all()
        for b in np.unique(k):
            m = k == b
            assert np.array_equal(lane[m], R.occluded_rays(ps, rays[m], float(lo[m][0]), float(hi[m][0]))), b
        ctx.set_variant(R.VARIANT_POOLED)
        for wide in (None, 2):
            if wide is not None:
                ctx.set_option("wide_waves", wide)
            got = R.occluded_rays(ps, rays, lo, hi)
            ll = ctx.last_launch
            assert ll.startswith(POOLED_ANY) and ll.endswith(PER_RAY), ll
            assert ("+SPILL" in ll) == (wide is not None), ll
            assert np.array_equal(got, lane), f"wide={wide}: {int((got != lane).sum())} rays differ from the lane kernel ({ll})"
    finally:
        ctx.set_option("wide_waves", 1)
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_invalid_intervals_are_misses(R, ctx):
    arr = O.OracleScene("rgbbox").arrays()
    scene, ps = _scene(R, ctx, "rgbbox")
    rays = R.camera_rays(ps, 64, 64)
    n = rays.shape[0]
    want_occ = R.occluded_rays(ps, rays, 0.1, 1e9)
    want_occ0 = R.occluded_rays(ps, rays, 0.0, 1e9)
    want_i, want_h = R.intersect_rays(ps, rays, 0.1, 1e9)
    want_i0, want_h0 = R.intersect_rays(ps, rays, 0.0, 1e9)
    lo, hi = np.full(n, 0.1, F), np.full(n, 1e9, F)
    bad = [(np.nan, 1e9), (0.1, np.nan), (np.nan, np.nan), (0.1, np.inf), (-np.inf, 1e9), (np.inf, np.inf), (-1.0, 1e9), (-1e-30, 5.0),
           (5.0, 4.0), (0.1, 2e9), (0.1, 1.0000001e9)]
    # rays that hit over (0.1, 1e9) -- a miss is then the rule's doing -- scattered through a few 64-ray tickets among valid rays
    hits = np.nonzero(want_occ & (want_i >= 0))[0]
    where = hits[hits >= n // 2][::5][:len(bad)]
    assert where.size == len(bad) and where[-1] - where[0] < 4 * 64
    for i, (a, b) in zip(where, bad):
        lo[i], hi[i] = a, b
    ok = V.interval_ok(lo, hi)
    assert ok.sum() == n - len(bad)
    # -0.0 is valid and behaves as 0.0
    neg0 = np.setdiff1d(np.arange(7, n, 97), where)
    lo[neg0] = -0.0
    ref_lo = lo.copy()
    ref_lo[neg0] = 0.0
    exp_occ = np.where(ok, np.where(lo == 0, want_occ0, want_occ), False)
    exp_i = np.where(ok, np.where(lo == 0, want_i0, want_i), -1)
    exp_h = np.where(ok[:, None], np.where((lo == 0)[:, None], want_h0, want_h), F(0))
    try:
        for variant, fam in _families(R):
            ctx.set_variant(variant)
            got = R.occluded_rays(ps, rays, lo, hi)
            assert fam(ctx.last_launch), ctx.last_launch
            assert not got[where].any(), f"variant {variant}: an invalid interval was answered as occluded"
            assert np.array_equal(got, exp_occ), f"variant {variant}: {int((got != exp_occ).sum())} rays differ"
            assert np.array_equal(R.occluded_rays(ps, rays, ref_lo, hi), got), f"variant {variant}: -0.0 differs from 0.0"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    got_i, got_h = R.intersect_rays(ps, rays, lo, hi)
    assert (got_i[where] == -1).all() and not got_h[where].any()
    assert np.array_equal(got_i, exp_i)
    assert np.array_equal(_bits(got_h), _bits(exp_h))
    ref = Q.RefScene(arr)
    assert np.array_equal(got_i, V.objs_hit(ref, rays[:, :3], rays[:, 3:], lo, hi)[0])
    ps.free()
    scene.free()


def test_ray_count_edges(R, ctx):
    import torch
    scene = ctx.irreg()
    ps = R.prepare_scene(64, 64, scene)
    n_max = 4097
    rays = torch.empty((n_max, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), 17, 241, ps)            # 4097 rays
    lo_np, hi_np, _ = V.mixed_intervals(n_max, seed=19)
    lo, hi = torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    rays_np = rays.cpu().numpy()
    ctx.set_variant(R.VARIANT_PIXEL)
    want_all = R.occluded_rays(ps, rays_np, lo_np, hi_np).astype(np.uint8)
    want_i_all, want_h_all = R.intersect_rays(ps, rays_np, lo_np, hi_np)
    try:
        for variant, fam in _families(R):
            ctx.set_variant(variant)
            for n in (0, 1, 63, 64, 65, 4097):
                out = torch.full((n + 1,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                R.occluded_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), out.data_ptr())
                ctx.sync()
                o = out.cpu().numpy()
                assert o[n] == 0xAB, f"n={n}: the byte past the output was written"
                if n == 0:
                    assert ctx.last_launch == "family=none (no rays)"
                    continue
                assert fam(ctx.last_launch), ctx.last_launch
                assert np.array_equal(o[:n], want_all[:n]), f"variant {variant} n={n}: {int((o[:n] != want_all[:n]).sum())} rays differ"
        for n in (0, 1, 63, 64, 65, 4097):
            idx = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
            hit = torch.full((n + 1, 7), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            R.intersect_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), idx.data_ptr(), hit.data_ptr())
            ctx.sync()
            ih, hh = idx.cpu().numpy(), hit.cpu().numpy()
            assert ih[n] == -7 and (hh[n] == -7.0).all(), f"n={n}: the record past the output was written"
            assert ctx.last_launch == ("family=none (no rays)" if n == 0 else LANE_INT)
            assert np.array_equal(ih[:n], want_i_all[:n]) and np.array_equal(_bits(hh[:n]), _bits(want_h_all[:n])), f"n={n}"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_refusals(R, ctx):
    import torch
    from raytracers_amd._lib import lib
    scene = ctx.rgbbox()
    ps = R.prepare_scene(8, 8, scene)
    rays = torch.from_numpy(R.camera_rays(ps, 8, 8)).cuda()
    lo = torch.zeros(64, dtype=torch.float32, device="cuda")
    hi = torch.full((64,), 1e9, dtype=torch.float32, device="cuda")
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    idx = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rp, lp, hp = C.c_void_p(rays.data_ptr()), C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr())
    op, ip = C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr())

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        ctx.sync()
        assert (out.cpu().numpy() == 0xAB).all(), f"{what}: the output was written"
        assert (idx.cpu().numpy() == -7).all(), f"{what}: the index output was written"

    for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_AUTO):
        ctx.set_variant(variant)
        try:
            for name, occ_args, int_args in (
                    ("n < 0", (-1, rp, lp, hp, op), (-1, rp, lp, hp, ip, None)),
                    ("n = 2^31", (1 << 31, rp, lp, hp, op), (1 << 31, rp, lp, hp, ip, None)),
                    ("NULL rays", (64, None, lp, hp, op), (64, None, lp, hp, ip, None)),
                    ("NULL t_min", (64, rp, None, hp, op), (64, rp, None, hp, ip, None)),
                    ("NULL t_max", (64, rp, lp, None, op), (64, rp, lp, None, ip, None)),
                    ("NULL output", (64, rp, lp, hp, None), (64, rp, lp, hp, None, None))):
                refused(lib.rt_occluded_rays_ranged(ctx._h, ps._h, *occ_args), f"occluded: {name}")
                refused(lib.rt_intersect_rays_ranged(ctx._h, ps._h, *int_args), f"intersect: {name}")
            assert lib.rt_occluded_rays_ranged(ctx._h, ps._h, 0, rp, lp, hp, op) == 0
            assert ctx.last_launch == "family=none (no rays)"
            assert lib.rt_intersect_rays_ranged(ctx._h, ps._h, 0, rp, lp, hp, ip, None) == 0
            assert ctx.last_launch == "family=none (no rays)"
        finally:
            ctx.set_variant(R.VARIANT_AUTO)
    # Python: a bad scalar next to an array is refused as the scalar entries refuse it; a wrong length or dtype is a ValueError
    arr = np.zeros(64, F)
    for t0, t1 in ((float("nan"), arr), (-1.0, arr), (arr, float("inf")), (arr, 2e9), (arr, -0.5)):
        with pytest.raises(R.RtError):
            R.occluded_rays(ps, rays, t0, t1)
        with pytest.raises(R.RtError):
            R.intersect_rays(ps, rays, t0, t1)
    for t0, t1 in ((np.zeros(63, F), 1.0), (0.0, np.ones(65, F)), (np.zeros(64, np.int32), 1.0), (0.0, np.ones((64, 1), F)),
                   (torch.zeros(64, dtype=torch.float64, device="cuda"), 1.0), (0.0, torch.ones(64)), (0.0, torch.ones(65, device="cuda"))):
        with pytest.raises(ValueError):
            R.occluded_rays(ps, rays, t0, t1)
        with pytest.raises(ValueError):
            R.intersect_rays(ps, rays, t0, t1)
    ps.free()
    scene.free()
    # a multi-device context is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    bp = C.c_void_p(mb.ptr)
    assert lib.rt_occluded_rays_ranged(mc._h, mps._h, 4, bp, bp, bp, bp) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    assert lib.rt_intersect_rays_ranged(mc._h, mps._h, 4, bp, bp, bp, bp, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()


def test_torch_in_place(R, ctx):
    import torch
    arr = O.OracleScene("irreg").arrays()
    scene, ps = _scene(R, ctx, "irreg")
    rays_np = X.seeded_rays(arr, 2048, seed=13)
    lo_np, hi_np, _ = V.mixed_intervals(2048, seed=17)
    rays, lo, hi = torch.from_numpy(rays_np).cuda(), torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    try:
        for variant, fam in _families(R):
            ctx.set_variant(variant)
            want = R.occluded_rays(ps, rays_np, lo_np, hi_np)
            got = R.occluded_rays(ps, rays, lo, hi)
            assert fam(ctx.last_launch), ctx.last_launch
            assert np.array_equal(got, want), variant
            assert np.array_equal(R.occluded_rays(ps, rays, lo, hi_np), want), variant      # one of each
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    wi, wh = R.intersect_rays(ps, rays_np, lo_np, hi_np)
    gi, gh = R.intersect_rays(ps, rays, lo, hi)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gh), _bits(wh))
    ps.free()
    scene.free()


def test_scalar_launch_strings_unchanged_after_ranged(R, ctx):
    scene, ps = _scene(R, ctx, "rgbbox")
    rays = R.camera_rays(ps, 32, 32)
    lo, hi = np.zeros(rays.shape[0], F), np.full(rays.shape[0], 1e9, F)
    try:
        ctx.set_variant(R.VARIANT_POOLED)
        R.occluded_rays(ps, rays, 0.1, 1e9)
        pooled_scalar = ctx.last_launch
        assert pooled_scalar.startswith(POOLED_ANY) and "intervals" not in pooled_scalar
        R.occluded_rays(ps, rays, lo, hi)
        assert ctx.last_launch == pooled_scalar + PER_RAY
        R.occluded_rays(ps, rays, 0.1, 1e9)
        assert ctx.last_launch == pooled_scalar
        ctx.set_variant(R.VARIANT_PIXEL)
        R.occluded_rays(ps, rays, lo, hi)
        assert ctx.last_launch == LANE_OCC
        R.occluded_rays(ps, rays, 0.1, 1e9)
        assert ctx.last_launch == "family=occluded"
        R.intersect_rays(ps, rays, lo, hi)
        assert ctx.last_launch == LANE_INT
        R.intersect_rays(ps, rays, 0.1, 1e9)
        assert ctx.last_launch == "family=intersect"
        R.trace_rays(ps, rays)
        assert ctx.last_launch == "family=pixel (rays)"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()
