"""Caller-supplied rays on the GPU: rt_camera_rays / rt_trace_rays / rt_intersect_rays against rt_render and the numpy restatement."""
import numpy as np
import pytest

import oracle_lib as O
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

FAMILIES = ("pooled", "pixel")


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


def _variant(R, fam):
    return {"pooled": R.VARIANT_POOLED, "pixel": R.VARIANT_PIXEL}[fam]


def _scene(ctx, spec):
    if spec.startswith("floor:"):
        _, n, k = spec.split(":")
        return ctx.floor(int(n), float(k))
    return ctx.scene(spec)


def _oracle(spec):
    if spec.startswith("floor:"):
        _, n, k = spec.split(":")
        return O.OracleScene("floor", n=int(n), k=float(k))
    return O.OracleScene(spec)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "floor:300:1800"])
def test_camera_rays_trace_equals_render(R, ctx, spec):
    scene = _scene(ctx, spec)
    for h, w in ((1, 1), (37, 53), (200, 200), (1000, 1000)):
        ps = R.prepare_scene(h, w, scene)
        rays = R.camera_rays(ps, h, w)
        if h * w <= 40000:
            want_rays = Q.camera_rays(ps.camera(), h, w)
            assert rays.tobytes() == want_rays.tobytes(), f"{spec} {h}x{w}: camera rays differ from the restatement"
        for fam in FAMILIES:
            ctx.set_variant(_variant(R, fam))
            for depth in (0, 1, 2, 50):
                want = R.render_image(ps, w, h, ps.camera(), max_depth=depth).reshape(-1)
                colour, pixel = R.trace_rays(ps, rays, max_depth=depth)
                assert np.array_equal(pixel, want), f"{spec} {h}x{w} {fam} depth {depth}: {int((pixel != want).sum())} pixels differ"
                assert np.array_equal(Q.colour_to_pixel(colour), pixel)
                if depth > 0:
                    assert ("family=pooled tickets=rays" if fam == "pooled" else "family=pixel (rays)") in ctx.last_launch, ctx.last_launch
        ctx.set_variant(R.VARIANT_AUTO)
        R.trace_rays(ps, rays)
        assert ctx.last_launch.startswith("family=pooled tickets=rays"), ctx.last_launch
        ps.free()
    scene.free()


def test_camera_rays_custom_camera(R, ctx):
    scene = ctx.rgbbox()
    ps = R.prepare_scene(64, 64, scene)
    cam = ps.camera().copy()
    cam[0:3] += np.float32([1.5, -0.5, 4.0])
    rays = R.camera_rays(ps, 37, 53, cam)
    assert rays.tobytes() == Q.camera_rays(cam, 37, 53).tobytes()
    ctx.set_variant(R.VARIANT_AUTO)
    _, pixel = R.trace_rays(ps, rays)
    assert np.array_equal(pixel, R.render_image(ps, 53, 37, cam).reshape(-1))


def test_big_floor_pooled_and_spill(R, ctx):
    scene = ctx.floor(1000, 6000.0)
    ps = R.prepare_scene(256, 256, scene)
    rays = R.camera_rays(ps, 256, 256)
    want = R.render(256, 256, ps).reshape(-1)
    ctx.set_variant(R.VARIANT_AUTO)
    try:
        for wide in (None, 2):
            if wide is not None:
                ctx.set_option("wide_waves", wide)
            _, pixel = R.trace_rays(ps, rays)
            ll = ctx.last_launch
            assert ll.startswith("family=pooled tickets=rays"), ll
            if wide is not None:
                assert "+SPILL" in ll, ll
            assert np.array_equal(pixel, want), f"wide={wide}: {int((pixel != want).sum())} pixels differ ({ll})"
    finally:
        ctx.set_option("wide_waves", 1)
    ps.free()
    scene.free()


def _seeded_rays(sc_arrays, n, seed):
    rng = np.random.default_rng(seed)
    L = sc_arrays["L"]
    lo, hi = L[:, :3].min(0) - L[:, 6:7].max(), L[:, :3].max(0) + L[:, 6:7].max()
    ext = hi - lo
    k = n // 4
    o_in = lo + rng.random((k, 3)) * ext
    o_out = lo - ext + rng.random((k, 3)) * 3 * ext
    pick = rng.integers(0, L.shape[0], k)
    o_sph = L[pick, :3] + (rng.random((k, 3)) - 0.5) * L[pick, 6:7]        # inside spheres
    o_mix = lo + rng.random((n - 3 * k, 3)) * ext
    o = np.concatenate([o_in, o_out, o_sph, o_mix]).astype(np.float32)
    d = rng.normal(size=(n, 3))
    axis = rng.integers(0, 3, n // 8)
    d[: n // 8] = 0
    d[np.arange(n // 8), axis] = rng.choice([-1.0, 1.0], n // 8)           # axis-aligned
    d[n // 8: n // 4, rng.integers(0, 3)] = 0.0                            # one zero component
    d *= 10.0 ** rng.uniform(-3, 3, (n, 1))                                # magnitudes 1e-3 .. 1e3
    return np.concatenate([o, d.astype(np.float32)], axis=1).astype(np.float32)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_seeded_rays_against_restatement(R, ctx, spec):
    orc = _oracle(spec)
    arr = orc.arrays()
    ref = Q.RefScene(arr)
    rays = _seeded_rays(arr, 4096, seed=17 if spec == "rgbbox" else 29)
    scene = _scene(ctx, spec)
    ps = R.prepare_scene(100, 100, scene)
    assert np.array_equal(ps.bvh_arrays()["L"], arr["L"])
    for depth in (1, 50):
        want_c = ref.ray_colour(rays[:, :3], rays[:, 3:], depth)
        for fam in FAMILIES:
            ctx.set_variant(_variant(R, fam))
            colour, pixel = R.trace_rays(ps, rays, max_depth=depth)
            bad = np.nonzero(np.any(colour.view(np.int32) != want_c.view(np.int32), axis=1))[0]
            assert bad.size == 0, f"{spec} {fam} depth {depth}: {bad.size} colours differ, first ray {bad[:3]}"
            assert np.array_equal(pixel, Q.colour_to_pixel(want_c))
    ctx.set_variant(R.VARIANT_AUTO)
    for t0, t1 in ((0.0, 1e9), (0.5, 30.0), (0.0, 0.05), (7.0, 7.0)):
        want_i, want_h = ref.objs_hit(rays[:, :3], rays[:, 3:], np.float32(t0), np.float32(t1))
        idx, hit = R.intersect_rays(ps, rays, t0, t1)
        assert ctx.last_launch == "family=intersect"
        assert np.array_equal(idx, want_i), f"{spec} ({t0}, {t1}): {int((idx != want_i).sum())} indices differ"
        assert hit.tobytes() == want_h.tobytes(), f"{spec} ({t0}, {t1}): hit records differ"
    ps.free()
    scene.free()


def test_ray_count_edges_and_outputs(R, ctx):
    import torch
    scene = ctx.irreg()
    ps = R.prepare_scene(64, 64, scene)
    big = R.camera_rays(ps, 1025, 1024)            # 2^20 + 1024 rays
    dev = torch.cuda.current_device()
    for fam in FAMILIES:
        ctx.set_variant(_variant(R, fam))
        for n in (0, 1, 63, 64, 65, (1 << 20) + 3):
            rays_t = torch.from_numpy(big[:max(n, 1)].copy()).to(f"cuda:{dev}")   # (n == 0: still a real pointer -- NULL is refused)
            col_t = torch.full((max(n, 1), 3), -7.0, dtype=torch.float32, device=f"cuda:{dev}")
            px_t = torch.full((max(n, 1),), -7, dtype=torch.int32, device=f"cuda:{dev}")
            col2 = torch.full_like(col_t, -7.0)
            px2 = torch.full_like(px_t, -7)
            torch.cuda.synchronize()
            R.trace_rays_into(rays_t.data_ptr(), n, ps, colour_ptr=col_t.data_ptr(), pixel_ptr=px_t.data_ptr())
            R.trace_rays_into(rays_t.data_ptr(), n, ps, colour_ptr=col2.data_ptr())
            R.trace_rays_into(rays_t.data_ptr(), n, ps, pixel_ptr=px2.data_ptr())
            ctx.sync()
            c, p = col_t.cpu().numpy(), px_t.cpu().numpy()
            if n == 0:
                assert (p == -7).all() and (c == -7).all()
                continue
            assert np.array_equal(Q.colour_to_pixel(c[:n]), p[:n])
            assert c[:n].tobytes() == col2.cpu().numpy()[:n].tobytes()
            assert np.array_equal(px2.cpu().numpy()[:n], p[:n])
            assert (px2.cpu().numpy()[n:] == -7).all()
            # the torch tensor is used in place by the convenience form as well
            if n <= 65:
                c3, p3 = R.trace_rays(ps, rays_t[:n])
                assert np.array_equal(p3, p[:n])
    ps.free()
    scene.free()


def test_refusals(R, ctx):
    import ctypes as C
    from raytracers_amd._lib import lib
    scene = ctx.rgbbox()
    ps = R.prepare_scene(8, 8, scene)
    buf = ctx.alloc_i32(64 * 7)
    p = C.c_void_p(buf.ptr)

    def refused(rc):
        assert rc != 0
        assert lib.rt_last_error(ctx._h).decode() != ""

    refused(lib.rt_trace_rays(ctx._h, ps._h, -1, p, 50, p, p))
    refused(lib.rt_trace_rays(ctx._h, ps._h, 1 << 31, p, 50, p, p))
    refused(lib.rt_trace_rays(ctx._h, ps._h, 4, None, 50, p, p))
    refused(lib.rt_trace_rays(ctx._h, ps._h, 4, p, 50, None, None))
    refused(lib.rt_trace_rays(ctx._h, ps._h, 4, p, -1, p, p))
    refused(lib.rt_intersect_rays(ctx._h, ps._h, -1, p, 0.0, 1.0, p, p))
    refused(lib.rt_intersect_rays(ctx._h, ps._h, 1 << 31, p, 0.0, 1.0, p, p))
    refused(lib.rt_intersect_rays(ctx._h, ps._h, 4, None, 0.0, 1.0, p, p))
    refused(lib.rt_intersect_rays(ctx._h, ps._h, 4, p, 0.0, 1.0, None, None))
    for t0, t1 in ((float("nan"), 1.0), (0.0, float("inf")), (0.0, float("nan")), (-1.0, 1.0), (2.0, 1.0), (0.0, 2e9), (-0.5, -0.1)):
        refused(lib.rt_intersect_rays(ctx._h, ps._h, 4, p, t0, t1, p, p))
    refused(lib.rt_camera_rays(ctx._h, ps._h, 0, 4, None, p))
    refused(lib.rt_camera_rays(ctx._h, ps._h, 4, 4, None, None))
    with pytest.raises(R.RtError):
        R.intersect_rays(ps, np.zeros((4, 6), np.float32), 1.0, 0.5)
    # n == 0 succeeds without a launch
    assert lib.rt_trace_rays(ctx._h, ps._h, 0, p, 50, p, None) == 0
    assert ctx.last_launch == "family=none (no rays)"
    assert lib.rt_intersect_rays(ctx._h, ps._h, 0, p, 0.0, 1.0, p, None) == 0
    buf.free()
    ps.free()
    scene.free()
    # a multi-device context is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    for rc in (lib.rt_trace_rays(mc._h, mps._h, 4, C.c_void_p(mb.ptr), 50, C.c_void_p(mb.ptr), None),
               lib.rt_intersect_rays(mc._h, mps._h, 4, C.c_void_p(mb.ptr), 0.0, 1.0, C.c_void_p(mb.ptr), None),
               lib.rt_camera_rays(mc._h, mps._h, 2, 2, None, C.c_void_p(mb.ptr))):
        assert rc != 0
        assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()
