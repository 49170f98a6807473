"""Ray paths on the GPU: rt_trace_paths and rt_trace_paths_shaped against the numpy restatement (path_ref.py), bit for bit, against
rt_intersect_rays and rt_trace_rays run on the same rays, and over launch shapes, ray counts, optional outputs, bad rays and refusals."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as E
import occlusion_ref as X
import oracle_lib as O
import path_ref as P

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ("rgbbox", "irreg", "big")   # big: the 1000 x 1000-sphere floor, a tree taller than 15 levels
DEPTHS = (0, 1, 3, 50)
KS = (1, 3, 8, 64)                    # 64 exceeds max_depth: the padding
SHAPES = (0, 64, 128, 512)


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


def _scene(R, ctx, spec, size=100):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(size, size, scene)
    return scene, ps, ps.bvh_arrays()


def _free(scene, ps):
    ps.free()
    scene.free()


def _launch(n, k, max_depth, R_):
    return f"family=paths k={k} depth={max_depth} rays/wave={R_}"


def _auto(R, ctx, n):
    return P.auto_rays_per_wave(n, ctx.device_info()["num_cu"])


def _outputs(torch, n, k, pad=0):
    """the seven outputs as poisoned device tensors of n + pad rays"""
    m = n + pad
    return [torch.full((m,), -7, dtype=torch.int32, device="cuda"), torch.full((m,), 0xAB, dtype=torch.uint8, device="cuda"),
            torch.full((m, k), -7, dtype=torch.int32, device="cuda"), torch.full((m, k, 7), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((m, 3), -7.0, dtype=torch.float32, device="cuda"), torch.full((m, 6), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((m, 3), -7.0, dtype=torch.float32, device="cuda")]


SENTINEL = (-7, 0xAB, -7, -7.0, -7.0, -7.0, -7.0)


def _device_paths(R, ctx, ps, rays_t, n, k, max_depth=50, rays_per_wave=0):
    """trace_paths_into on the first n rays of a device tensor -> numpy outputs"""
    import torch
    outs = _outputs(torch, n, k)
    torch.cuda.synchronize()
    R.trace_paths_into(rays_t.data_ptr(), n, ps, k, *[t.data_ptr() for t in outs], max_depth=max_depth, rays_per_wave=rays_per_wave)
    ctx.sync()
    return tuple(t.cpu().numpy() for t in outs)


@pytest.mark.parametrize("spec", SCENES)
def test_against_restatement(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec)
    orc = O.OracleScene(spec)
    ref = orc.arrays()
    for key in ("L", "bmin", "bmax", "left", "right"):
        assert np.array_equal(arr[key], ref[key]), f"{spec}: the prepared scene's {key} is not the oracle's"
    sets = {"seeded": X.seeded_rays(arr, 2048, seed=17), "camera": R.camera_rays(ps, 40, 40)}
    for name, rays in sets.items():
        n = rays.shape[0]
        for max_depth in DEPTHS:
            want = P.trace_paths(P.oracle_hit(orc), arr["L"][:, 3:6], rays, max_depth, max(KS))
            codes = np.bincount(want[1], minlength=3)
            if name == "seeded" and max_depth == 3:
                assert (codes > 0).all(), f"{spec}: the seeded rays miss an end code at max_depth 3: {codes}"
            if name == "seeded" and max_depth == 50:
                assert codes[P.ESCAPED] > 0 and codes[P.ABSORBED] > 0 and want[0].max() > 8, (spec, codes)
            for k in KS:
                for shape in SHAPES:
                    got = R.trace_paths(ps, rays, k, max_depth, shape)
                    assert ctx.last_launch == _launch(n, k, max_depth, shape or _auto(R, ctx, n)), ctx.last_launch
                    P.assert_same(got, P.prefix(want, k), f"{spec} {name} max_depth={max_depth} k={k} rays_per_wave={shape}")
    _free(scene, ps)


def _reflected(rays, hit):
    """{hit.p, reflect (normalise d) normal}: the next ray of the chain, rebuilt in numpy (ray.fut:116-121)"""
    with np.errstate(all="ignore"):
        refl, _ = P._scatter(rays[:, 3:], hit[:, 4:7])
    return np.concatenate([hit[:, 1:4], refl], axis=1).astype(F)


@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_device_cross_checks(R, ctx, spec):
    scene, ps, arr = _scene(R, ctx, spec, 128)
    rays = np.concatenate([R.camera_rays(ps, 64, 64), X.seeded_rays(arr, 4096, seed=5)])
    count, end, index, hit, light, last, colour = want = R.trace_paths(ps, rays, 4)
    # vertex s is intersect_rays(0, 1e9) of the chain's s-th ray, rebuilt in numpy from vertex s - 1: the first four vertices, three segments
    cur, alive = rays, np.arange(rays.shape[0])     # the rays that make an s-th objs_hit call, and whose chains they belong to
    for s in range(4):
        idx, h7 = R.intersect_rays(ps, cur, 0.0, 1e9)
        have = idx >= 0
        assert np.array_equal(have, count[alive] > s), f"{spec}: call {s}: count disagrees with intersect_rays"
        assert np.array_equal(end[alive[~have]] == P.ESCAPED, count[alive[~have]] == s), f"{spec}: call {s}: ESCAPED is not a miss"
        assert np.array_equal(index[alive, s], idx), f"{spec}: vertex {s} is not intersect_rays's sphere"
        assert np.array_equal(P.bits(hit[alive, s]), P.bits(h7)), f"{spec}: vertex {s}'s record is not intersect_rays's"
        on = have & ((count[alive] > s + 1) | (end[alive] == P.ESCAPED))     # the chains that scatter at vertex s (max_depth 50 > s + 1)
        assert np.array_equal(end[alive[have & ~on]] == P.ABSORBED, np.ones((have & ~on).sum(), bool)), f"{spec}: vertex {s}"
        assert on.sum() > 50, (spec, s, int(on.sum()))
        cur, alive = _reflected(cur[on], h7[on]), alive[on]
    try:
        for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_AUTO):
            ctx.set_variant(variant)
            if variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL):
                col, _ = R.trace_rays(ps, rays)
                assert np.array_equal(P.bits(col), P.bits(colour)), f"{spec}: colour is not trace_rays's under variant {variant}"
            P.assert_same(R.trace_paths(ps, rays, 4), want, f"{spec} variant {variant}")
            assert ctx.last_launch == _launch(rays.shape[0], 4, 50, _auto(R, ctx, rays.shape[0]))
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


def test_block_edges_and_unaligned_pointers(R, ctx):
    import torch
    scene, ps, arr = _scene(R, ctx, "rgbbox", 64)
    n_max, k = 128 * 3 + 1, 3
    # one float of slack in front: every buffer below starts one ELEMENT past its allocation's start
    flat = torch.empty(6 * n_max + 1, dtype=torch.float32, device="cuda")
    rays = flat[1:].view(n_max, 6)
    rays.copy_(torch.from_numpy(np.concatenate([R.camera_rays(ps, 16, 16), X.seeded_rays(arr, n_max - 256, seed=7)])))
    assert rays.data_ptr() % 8 == 4
    rays_np = rays.cpu().numpy()
    want = R.trace_paths(ps, rays_np, k, 50, 64)
    assert want[0].max() > k and (want[1] == P.ABSORBED).any()
    for n in (0, 1, 63, 64, 65, 127, 128, 129, n_max):
        for shape in (128, 64):
            outs = _outputs(torch, n, k, pad=2)           # a guard row either side
            torch.cuda.synchronize()
            R.trace_paths_into(rays.data_ptr(), n, ps, k, *[t[1:].data_ptr() for t in outs], rays_per_wave=shape)
            ctx.sync()
            assert ctx.last_launch == ("family=none (no rays)" if n == 0 else _launch(n, k, 50, shape))
            got = [t.cpu().numpy() for t in outs]
            for name, g, sent in zip(P.NAMES, got, SENTINEL):
                assert (g[0] == sent).all() and (g[n + 1] == sent).all(), f"n={n} rays_per_wave={shape}: {name} was written outside its n rows"
            P.assert_same([g[1:n + 1] for g in got], [w[:n] for w in want], f"n={n} rays_per_wave={shape}")
    # ... and every output ONE ELEMENT past its allocation's start (k = 3: int32 rows of 12 bytes, hit rows of 84)
    outs = _outputs(torch, n_max, k, pad=1)
    torch.cuda.synchronize()
    R.trace_paths_into(rays.data_ptr(), n_max, ps, k, *[t.reshape(-1)[1:].data_ptr() for t in outs], rays_per_wave=128)
    ctx.sync()
    for name, t, w, sent in zip(P.NAMES, outs, want, SENTINEL):
        g = t.reshape(-1).cpu().numpy()
        assert g[0] == sent, f"unaligned {name}: written in front of its start"
        assert np.array_equal(P.bits(g[1:1 + w.size].reshape(w.shape)), P.bits(w)), f"unaligned {name}"
        assert (g[1 + w.size:] == sent).all(), f"unaligned {name}: written past its end"
    _free(scene, ps)


def test_optional_outputs_and_guard_bands(R, ctx):
    import torch
    from raytracers_amd._lib import lib
    scene, ps, arr = _scene(R, ctx, "irreg")
    rays_np = np.concatenate([X.seeded_rays(arr, 1000, seed=3), R.camera_rays(ps, 10, 10)])
    rays = torch.from_numpy(rays_np).cuda()
    n, k, band = rays.shape[0], 5, 3
    want = R.trace_paths(ps, rays_np, k, 3)
    assert (np.bincount(want[1], minlength=3) > 0).all()
    wanted_sets = [[i] for i in range(7)] + [[0, 1], list(range(7))]
    for shape in (0, 128):
        for keep in wanted_sets:
            outs = _outputs(torch, n + 2 * band, k)           # guard bands of `band` rows either side
            ptrs = [t[band:].data_ptr() if i in keep else None for i, t in enumerate(outs)]
            torch.cuda.synchronize()
            R.trace_paths_into(rays.data_ptr(), n, ps, k, *ptrs, max_depth=3, rays_per_wave=shape)
            ctx.sync()
            for i, (name, t, w, s) in enumerate(zip(P.NAMES, outs, want, SENTINEL)):
                g = t.cpu().numpy()
                if i not in keep:
                    assert (g == s).all(), f"keep={keep}: {name} was written though its pointer is NULL"
                    continue
                assert (g[:band] == s).all() and (g[band + n:] == s).all(), f"keep={keep}: {name} was written outside its rows"
                assert np.array_equal(P.bits(g[band:band + n]), P.bits(w)), f"keep={keep} rays_per_wave={shape}: {name} differs"
    assert lib.rt_trace_paths(ctx._h, ps._h, n, C.c_void_p(rays.data_ptr()), 3, k, *([None] * 7)) != 0
    assert "NULL" in lib.rt_last_error(ctx._h).decode()
    _free(scene, ps)


def test_shape_independence_at_size(R, ctx):
    import torch
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(512, 512, scene)
    n, k, piece = 1 << 18, 4, 4096
    rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), 512, 512, ps)
    whole = _device_paths(R, ctx, ps, rays, n, k)
    want_shape = _auto(R, ctx, n)
    assert want_shape > 64 and ctx.last_launch == _launch(n, k, 50, want_shape), (ctx.last_launch, want_shape)
    assert whole[0].max() > 8 and whole[0].min() < 4      # chains of very different lengths share the waves
    for s in range(0, n, piece):
        part = _device_paths(R, ctx, ps, rays[s:s + piece], piece, k)
        assert ctx.last_launch == _launch(piece, k, 50, 64), ctx.last_launch
        P.assert_same(part, [w[s:s + piece] for w in whole], f"rays {s} .. {s + piece}")
    del rays
    _free(scene, ps)


def test_wide_outputs_use_64_bit_offsets(R, ctx):
    # n * k * 7 = 2^32 * 7 / 8 floats past 2^31: the last rays' rows land at their own place (a 32-bit offset would wrap)
    import torch
    scene, ps, _ = _scene(R, ctx, "rgbbox", 64)
    n, k, tail_n = 1 << 19, 1024, 4096
    try:
        hit = torch.empty((n, k, 7), dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError as e:
        _free(scene, ps)
        pytest.skip(f"the device cannot allocate the {n * k * 28 / 2 ** 30:.1f} GiB hit7 buffer: {str(e)[:80]}")
    tail = torch.from_numpy(R.camera_rays(ps, 64, 64)).cuda()
    rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    rays[: n - tail_n] = tail[0]
    rays[n - tail_n:] = tail
    hit[n - tail_n:] = -7.0
    # ... and so do the rows on either side of the places where a 32-bit offset would wrap or change sign: float index 2^31 (byte offset
    # 2^33) and byte offsets 2^31 and 2^32 (all of them copies of ray tail[0])
    windows = sorted({(1 << e) // (k * 7 * unit) for e in (31, 32, 33) for unit in (1, 4) if (1 << e) // (k * 7 * unit) < n - tail_n})
    assert windows == [74898, 149796, 299593]
    for w in windows:
        hit[w - 8:w + 8] = -7.0
    torch.cuda.synchronize()
    R.trace_paths_into(rays.data_ptr(), n, ps, k, hit_ptr=hit.data_ptr(), max_depth=2)
    ctx.sync()
    want = R.trace_paths(ps, tail, k, 2)
    assert want[0].max() == 2
    got = hit[n - tail_n:].cpu().numpy()
    assert np.array_equal(P.bits(got), P.bits(want[3]))
    assert np.array_equal(P.bits(hit[0].cpu().numpy()), P.bits(want[3][0]))
    for w in windows:
        rows = hit[w - 8:w + 8].cpu().numpy()
        assert np.array_equal(P.bits(rows), P.bits(np.broadcast_to(want[3][0], rows.shape))), f"rows {w - 8} .. {w + 8}"
    del hit, rays
    torch.cuda.empty_cache()
    _free(scene, ps)


def test_bad_rays_leave_the_good_ones_alone(R, ctx):
    scene, ps, arr = _scene(R, ctx, "irreg")
    fam = E.ray_families(arr, seed=4)
    bad = np.concatenate([fam["non_finite"], fam["zero_dir"], fam["denormal"]])
    good = np.concatenate([X.seeded_rays(arr, 2 * bad.shape[0], seed=9), R.camera_rays(ps, 12, 12)])[: 2 * bad.shape[0]]
    mixed = np.empty((3 * bad.shape[0], 6), F)
    mixed[0::3], mixed[1::3], mixed[2::3] = good[0::2], bad, good[1::2]
    is_good = np.ones(mixed.shape[0], bool)
    is_good[1::3] = False
    n_sph = arr["L"].shape[0]
    for max_depth, k, shape in ((50, 8, 0), (3, 2, 64), (3, 8, 128), (1, 1, 128)):
        count, end, index, hit, light, last, colour = got = R.trace_paths(ps, mixed, k, max_depth, shape)   # (the call returns)
        assert (count >= 0).all() and (count <= max_depth).all()
        assert np.isin(end, (P.ESCAPED, P.ABSORBED, P.TRUNCATED)).all()
        assert (index >= -1).all() and (index < n_sph).all()
        alone = R.trace_paths(ps, good, k, max_depth, 64)
        order = np.empty(good.shape[0], np.int64)
        order[0::2], order[1::2] = np.arange(0, mixed.shape[0], 3), np.arange(2, mixed.shape[0], 3)
        P.assert_same([g[order] for g in got], alone, f"max_depth={max_depth} k={k} rays_per_wave={shape}: the good rays")
    _free(scene, ps)


def test_refusals(R, ctx):
    import torch
    from raytracers_amd._lib import lib
    scene, ps, _ = _scene(R, ctx, "rgbbox", 8)
    rays = torch.from_numpy(R.camera_rays(ps, 8, 8)).cuda()
    outs = _outputs(torch, 64, 4)
    torch.cuda.synchronize()
    rp = C.c_void_p(rays.data_ptr())
    op = [C.c_void_p(t.data_ptr()) for t in outs]

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        ctx.sync()
        for name, t, s in zip(P.NAMES, outs, SENTINEL):
            assert (t.cpu().numpy() == s).all(), f"{what}: {name} was written"

    R.intersect_rays(ps, rays, 0.0, 1e9)
    before = ctx.last_launch
    for name, n, r, depth, k in (("k = 0", 64, rp, 50, 0), ("k = 1025", 64, rp, 50, 1025), ("negative max_depth", 64, rp, -1, 4),
                                 ("NULL rays", 64, None, 50, 4), ("n < 0", -1, rp, 50, 4), ("n = 2^31", 1 << 31, rp, 50, 4)):
        refused(lib.rt_trace_paths(ctx._h, ps._h, n, r, depth, k, *op), name)
        refused(lib.rt_trace_paths_shaped(ctx._h, ps._h, n, r, depth, k, *op, 128), f"shaped: {name}")
    for shape in (32, 65, 8192, -64, 4160):
        refused(lib.rt_trace_paths_shaped(ctx._h, ps._h, 64, rp, 50, 4, *op, shape), f"rays_per_wave = {shape}")
    refused(lib.rt_trace_paths(ctx._h, None, 64, rp, 50, 4, *op), "NULL prepared scene")
    refused(lib.rt_trace_paths(ctx._h, ps._h, 64, rp, 50, 4, *([None] * 7)), "all outputs NULL")
    assert ctx.last_launch == before, "a refused call changed last_launch"
    # the largest shape and k are accepted; n == 0 launches nothing
    assert lib.rt_trace_paths_shaped(ctx._h, ps._h, 64, rp, 50, 4, *op, 4096) == 0
    assert ctx.last_launch == _launch(64, 4, 50, 4096)
    assert lib.rt_trace_paths(ctx._h, ps._h, 0, rp, 50, 1024, *op) == 0
    assert ctx.last_launch == "family=none (no rays)"
    ctx.sync()
    for k in (0, 1025):
        with pytest.raises(R.RtError):
            R.trace_paths(ps, rays, k)
    with pytest.raises(R.RtError):
        R.trace_paths(ps, rays, 4, -1)
    with pytest.raises(R.RtError):
        R.trace_paths(ps, rays, 4, 50, 65)
    # the other entries' launch strings are what they were
    try:
        ctx.set_variant(R.VARIANT_PIXEL)
        lo, hi = np.zeros(64, F), np.full(64, 1e9, F)
        seen = []
        for call in (lambda: R.intersect_rays(ps, rays, 0.1, 1e9), lambda: R.intersect_rays(ps, rays, lo, hi),
                     lambda: R.occluded_rays(ps, rays, 0.1, 1e9), lambda: R.trace_rays(ps, rays), lambda: R.multi_hit_rays(ps, rays, 8)):
            R.trace_paths(ps, rays, 2)
            call()
            seen.append(ctx.last_launch)
        assert seen == ["family=intersect", "family=intersect (per-ray)", "family=occluded", "family=pixel (rays)", "family=multi-hit k=8"]
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)
    # a multi-device context (a device listed twice) is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64)
    bp = C.c_void_p(mb.ptr)
    assert lib.rt_trace_paths(mc._h, mps._h, 4, bp, 50, 1, bp, None, None, None, None, None, None) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    assert lib.rt_trace_paths_shaped(mc._h, mps._h, 4, bp, 50, 1, bp, None, None, None, None, None, None, 64) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mb.free()
    mps.free()
    ms.free()
    mc.close()


def test_torch_in_place(R, ctx):
    import torch
    scene, ps, arr = _scene(R, ctx, "irreg")
    orc = O.OracleScene("irreg")
    rays_np = X.seeded_rays(arr, 2048, seed=13)
    rays = torch.from_numpy(rays_np).cuda()
    want = P.trace_paths(P.oracle_hit(orc), arr["L"][:, 3:6], rays_np, 50, 4)
    P.assert_same(R.trace_paths(ps, rays, 4), want, "torch rays")
    P.assert_same(_device_paths(R, ctx, ps, rays, 2048, 4, rays_per_wave=256), want, "torch rays and outputs")
    assert ctx.last_launch == _launch(2048, 4, 50, 256)
    _free(scene, ps)
