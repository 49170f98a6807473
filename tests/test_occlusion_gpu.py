"""Occlusion (any-hit) queries on the GPU: rt_occluded_rays under the pooled any-hit loop and the lane kernel, against the numpy
restatement (occlusion_ref.py) and against rt_intersect_rays at t_min = 0.1."""
import numpy as np
import pytest

import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

POOLED_ANY = "family=pooled tickets=rays instantiation=any"


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


def _families(R, spec=None, t_max=None):
    # (variant, what last_launch must start with): the pooled family, the lane kernel, and AUTO -- the pooled loop only for a scene that is
    # staged in LDS whole (rgbbox) and t_max > 1, the lane kernel otherwise (api_queries.cpp)
    auto = "family=" if spec is None else POOLED_ANY if spec == "rgbbox" and t_max > 1.0 else "family=occluded"
    return ((R.VARIANT_POOLED, POOLED_ANY), (R.VARIANT_PIXEL, "family=occluded"), (R.VARIANT_AUTO, auto))


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_seeded_rays_against_restatement(R, ctx, spec):
    arr = O.OracleScene(spec).arrays()
    ref = Q.RefScene(arr)
    rays = X.seeded_rays(arr, 4096, seed=17 if spec == "rgbbox" else 29)
    scene = ctx.scene(spec)
    ps = R.prepare_scene(100, 100, scene)
    assert np.array_equal(ps.bvh_arrays()["L"], arr["L"])
    try:
        for t0, t1 in ((0.0, 1e9), (0.1, 1e9), (0.5, 30.0), (0.0, 0.05), (7.0, 7.0)):
            want = X.occluded(ref, rays[:, :3], rays[:, 3:], t0, t1)
            if t1 >= 30.0:
                assert want.any() and not want.all()
            for variant, family in _families(R, spec, t1):
                ctx.set_variant(variant)
                got = R.occluded_rays(ps, rays, t0, t1)
                assert ctx.last_launch.startswith(family), ctx.last_launch
                assert got.dtype == bool and got.shape == (4096,)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, f"{spec} ({t0}, {t1}) variant {variant}: {bad.size} rays differ, first {bad[:5]}"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_camera_rays_agree_with_intersect(R, ctx, spec):
    import torch
    arr = O.OracleScene(spec).arrays()
    ref = Q.RefScene(arr)
    scene = ctx.scene(spec)
    h = w = 1000
    ps = R.prepare_scene(h, w, scene)
    rays = torch.empty((h * w, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), h, w, ps)
    ctx.sync()
    idx, _ = R.intersect_rays(ps, rays, 0.1, 1e9)
    want = idx >= 0
    sub = np.random.default_rng(3).choice(h * w, 2048, replace=False)
    rays_np = rays.cpu().numpy()
    want_sub = X.occluded(ref, rays_np[sub, :3], rays_np[sub, 3:], 0.1, 1e9)
    try:
        for variant, family in _families(R, spec, 1e9):
            ctx.set_variant(variant)
            got = R.occluded_rays(ps, rays, 0.1, 1e9)
            assert ctx.last_launch.startswith(family), ctx.last_launch
            assert np.array_equal(got, want), f"{spec} variant {variant}: {int((got != want).sum())} rays differ from intersect_rays"
            assert np.array_equal(got[sub], want_sub)
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


@pytest.mark.parametrize("spec,size", [("rgbbox", 256), ("irreg", 96)])
def test_shadow_rays_against_restatement(R, ctx, spec, size):
    arr = O.OracleScene(spec).arrays()
    ref = Q.RefScene(arr)
    scene = ctx.scene(spec)
    ps = R.prepare_scene(size, size, scene)
    idx, hit = R.intersect_rays(ps, R.camera_rays(ps, size, size), 0.0, 1e9)
    sh = X.shadow_rays(idx, hit, X.LIGHTS[spec])
    want = X.occluded(ref, sh[:, :3], sh[:, 3:], 1e-3, 1.0)
    assert 0.1 < want.mean() < 0.9, want.mean()
    try:
        for variant, family in _families(R, spec, 1.0):
            ctx.set_variant(variant)
            got = R.occluded_rays(ps, sh, 1e-3, 1.0)
            assert ctx.last_launch.startswith(family), ctx.last_launch
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{spec} variant {variant}: {bad.size} shadow rays differ, first {bad[:5]}"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_pooled_shapes(R, ctx):
    # every shape of the any-hit loop: 16 waves with the whole scene in LDS (rgbbox) and without (irreg), four-wave workgroups, and the
    # spilling box stack at the test capacity (192) on irreg's 15 levels
    cases = (("rgbbox", {}, "waves=16"), ("irreg", {}, "waves=16"), ("irreg", {"wide_waves": 2}, "waves=4"),
             ("irreg", {"wide_waves": 2, "stack_cap": 192}, "+SPILL"))
    ctx.set_variant(R.VARIANT_POOLED)
    try:
        for spec, opts, mark in cases:
            arr = O.OracleScene(spec).arrays()
            ref = Q.RefScene(arr)
            rays = X.seeded_rays(arr, 4096, seed=5)
            want = X.occluded(ref, rays[:, :3], rays[:, 3:], 0.0, 1e9)
            scene = ctx.scene(spec)
            ps = R.prepare_scene(100, 100, scene)
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                got = R.occluded_rays(ps, rays)
                ll = ctx.last_launch
            finally:
                ctx.set_option("wide_waves", 1)
                ctx.set_option("stack_cap", 0)
            assert ll.startswith(POOLED_ANY) and mark in ll, (spec, opts, ll)
            assert ("+SPILL" in ll) == ("stack_cap" in opts), (spec, opts, ll)
            assert np.array_equal(got, want), f"{spec} {opts}: {int((got != want).sum())} rays differ ({ll})"
            ps.free()
            scene.free()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)


def test_tall_tree_pooled_and_spill(R, ctx):
    # a 1000-sphere floor (a tree taller than 15 levels): the pooled loop in its sixteen-wave shape and, with the wide shape forced, its
    # spilling box stack at the production capacity; AUTO takes the lane kernel here (the scene is not staged in LDS whole)
    scene = ctx.floor(1000, 6000.0)
    ps = R.prepare_scene(256, 256, scene)
    rays = R.camera_rays(ps, 256, 256)
    idx, hit = R.intersect_rays(ps, rays, 0.1, 1e9)
    sh = X.shadow_rays(idx, hit, (0.0, 50.0, 0.0))
    try:
        ctx.set_variant(R.VARIANT_PIXEL)
        lane = R.occluded_rays(ps, rays, 0.1, 1e9)
        lane_sh = R.occluded_rays(ps, sh, 1e-3, 1.0)
        assert ctx.last_launch == "family=occluded"
        assert np.array_equal(lane, idx >= 0)
        ctx.set_variant(R.VARIANT_AUTO)
        assert np.array_equal(R.occluded_rays(ps, rays, 0.1, 1e9), lane)
        ctx.set_variant(R.VARIANT_POOLED)
        for wide in (None, 2):
            if wide is not None:
                ctx.set_option("wide_waves", wide)
            got = R.occluded_rays(ps, rays, 0.1, 1e9)
            ll = ctx.last_launch
            assert ll.startswith(POOLED_ANY), ll
            if wide is not None:
                assert "+SPILL" in ll, ll
            assert np.array_equal(got, lane), f"wide={wide}: {int((got != lane).sum())} rays differ from the lane kernel ({ll})"
            assert np.array_equal(got, idx >= 0)
            got_sh = R.occluded_rays(ps, sh, 1e-3, 1.0)
            assert np.array_equal(got_sh, lane_sh), f"wide={wide}: {int((got_sh != lane_sh).sum())} shadow rays differ"
    finally:
        ctx.set_option("wide_waves", 1)
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_ray_count_edges(R, ctx):
    import torch
    scene = ctx.irreg()
    ps = R.prepare_scene(64, 64, scene)
    big = torch.empty(((1 << 20) + 1024, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(big.data_ptr(), 1025, 1024, ps)             # 2^20 + 1024 rays
    idx, _ = R.intersect_rays(ps, big, 0.1, 1e9)
    want_all = (idx >= 0).astype(np.uint8)
    try:
        for variant, family in _families(R):
            ctx.set_variant(variant)
            for n in (0, 1, 63, 64, 65, (1 << 20) + 1024):
                out = torch.full((n + 1,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                R.occluded_rays_into(big.data_ptr(), n, ps, out.data_ptr(), 0.1, 1e9)
                ctx.sync()
                o = out.cpu().numpy()
                assert o[n] == 0xAB, f"n={n}: the byte past the output was written"
                if n == 0:
                    assert ctx.last_launch == "family=none (no rays)"
                    continue
                assert ctx.last_launch.startswith(family), ctx.last_launch
                assert np.array_equal(o[:n], want_all[:n]), f"variant {variant} n={n}: {int((o[:n] != want_all[:n]).sum())} rays differ"
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    ps.free()
    scene.free()


def test_refusals(R, ctx):
    import ctypes as C
    import torch
    from raytracers_amd._lib import lib
    scene = ctx.rgbbox()
    ps = R.prepare_scene(8, 8, scene)
    rays = torch.from_numpy(R.camera_rays(ps, 8, 8)).cuda()
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rp, op = C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr())

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        ctx.sync()
        assert (out.cpu().numpy() == 0xAB).all(), f"{what}: the output was written"

    refused(lib.rt_occluded_rays(ctx._h, ps._h, -1, rp, 0.0, 1.0, op), "n < 0")
    refused(lib.rt_occluded_rays(ctx._h, ps._h, 1 << 31, rp, 0.0, 1.0, op), "n = 2^31")
    refused(lib.rt_occluded_rays(ctx._h, ps._h, 64, None, 0.0, 1.0, op), "NULL rays")
    refused(lib.rt_occluded_rays(ctx._h, ps._h, 64, rp, 0.0, 1.0, None), "NULL output")
    for t0, t1 in ((float("nan"), 1.0), (0.0, float("inf")), (0.0, float("nan")), (-1.0, 1.0), (2.0, 1.0), (0.0, 2e9), (-0.5, -0.1),
                   (float("-inf"), 1.0)):
        refused(lib.rt_occluded_rays(ctx._h, ps._h, 64, rp, t0, t1, op), f"interval ({t0}, {t1})")
    with pytest.raises(R.RtError):
        R.occluded_rays(ps, np.zeros((4, 6), np.float32), 1.0, 0.5)
    # n == 0 succeeds without a launch; t_min == t_max is legal and occludes nothing
    assert lib.rt_occluded_rays(ctx._h, ps._h, 0, rp, 0.0, 1.0, op) == 0
    assert ctx.last_launch == "family=none (no rays)"
    assert not R.occluded_rays(ps, rays, 3.0, 3.0).any()
    ps.free()
    scene.free()
    # a multi-device context is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    assert lib.rt_occluded_rays(mc._h, mps._h, 4, C.c_void_p(mb.ptr), 0.0, 1.0, C.c_void_p(mb.ptr)) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()
