"""Scenes prepared from spheres in device memory (rt_prepare_scene_device) and rebuilt in place (rt_prepared_update_spheres): the same
prepared scene as rt_scene_from_spheres + rt_prepare_scene on the same bytes -- BVH arrays, height, camera, the launch every variant picks
(culling included), every pixel and every caller-ray output -- and the update's reset of the views' state, stream order and refusals."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

SIDES = (200, 1000)


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import raytracers_amd
    return raytracers_amd


def _ctx(R, **opts):
    c = R.Context(0)
    c.set_option("sync_policy", 1)   # (which instantiation renders frame k is then the same in every run: launches can be compared)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _oracle_scene(name):
    """(spheres7, (look_from, look_at, fov)) of one of the reference's scenes, from the C oracle's generator"""
    if name.startswith("floor:"):
        _, n, k = name.split(":")
        orc = O.OracleScene("floor", n=int(n), k=float(k))
    else:
        orc = O.OracleScene(name)
    sc = orc.scene
    s = np.ctypeslib.as_array(C.cast(sc.spheres, C.POINTER(C.c_float)), shape=(orc.n * 7,)).reshape(orc.n, 7).copy()
    v = lambda a: (a.x, a.y, a.z)   # noqa: E731
    return s, (v(sc.look_from), v(sc.look_at), float(sc.fov))


def _random_scene(n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), np.float32)
    ext = 10.0 * max(1.0, float(n) ** (1.0 / 3.0))
    s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.3, 2.0, n)
    return s, ((0.0, 0.5 * ext, 3.0 * ext), (0.0, 0.0, 0.0), 50.0)


def _degenerate(kind):
    s, view = _random_scene(500, 99)
    if kind == "nan":
        s[7, 1] = np.nan
        s[300, 6] = np.nan
    elif kind == "inf":
        s[11, 0] = np.inf
        s[12, 2] = -np.inf
    elif kind == "zero_radius":
        s[5, 6] = 0.0
        s[6, 6] = np.nextafter(np.float32(2.0 ** -20), np.float32(0))
    return s, view


def _host(R, ctx, s, view, h, w):
    sc = ctx.scene_from_spheres(s, *view)
    ps = R.prepare_scene(h, w, sc)
    sc.free()
    return ps


def _same_prepared(a, b, what):
    A, B = a.bvh_arrays(), b.bvh_arrays()
    for k in ("L", "bmin", "bmax", "left", "right", "parent"):
        assert A[k].tobytes() == B[k].tobytes(), f"{what}: {k} differs"
    assert a.height == b.height, f"{what}: height {a.height} != {b.height}"
    assert a.camera().tobytes() == b.camera().tobytes(), f"{what}: camera differs"


def _frames(R, ctx, ps, sides=SIDES, variants=None, pixels=True):
    """every (variant, side) frame of ps with the launch that rendered it"""
    out = []
    for v in variants or (R.VARIANT_AUTO, R.VARIANT_POOLED, R.VARIANT_PIXEL):
        ctx.set_variant(v)
        for side in sides:
            img = R.render(side, side, ps)
            out.append((v, side, img if pixels else None, ctx.last_launch))
    ctx.set_variant(R.VARIANT_AUTO)
    return out


def _same_frames(got, want, what):
    assert len(got) == len(want)
    for (v, side, gi, gl), (_, _, wi, wl) in zip(got, want):
        assert gl == wl, f"{what} variant {v} {side}x{side}: launch {gl!r} != {wl!r}"
        if wi is not None:
            assert int((gi != wi).sum()) == 0, f"{what} variant {v} {side}x{side}: {int((gi != wi).sum())} pixels differ"


CASES = (["rgbbox", "irreg", "floor:300:1800"] + [f"random:{n}" for n in (2, 3, 767, 768, 769, 24576, 24577, 131072, 131073)]
         + ["random:1000000", "tall", "nan", "inf", "zero_radius"])


def _case(name):
    if name.startswith("random:"):
        n = int(name.split(":")[1])
        return _random_scene(n, n)
    if name == "tall":
        s, lf, la, fov = E.SCENES["tall1100"]
        return s, (lf, la, fov)
    if name in ("nan", "inf", "zero_radius"):
        return _degenerate(name)
    return _oracle_scene(name)


# (gpu_build = 0 for every case but the 10^6 spheres: the host builder's seconds there add nothing the smaller cases do not check)
@pytest.mark.parametrize("name, gpu_build", [(c, g) for g in (1, 0) for c in CASES if not (g == 0 and c == "random:1000000")])
def test_device_prepare_equals_host_prepare(R, name, gpu_build):
    import torch
    s, view = _case(name)
    degenerate = name in ("nan", "inf", "zero_radius")
    sides = (200,) if (degenerate or name == "random:1000000") else SIDES
    ctx = _ctx(R, gpu_build=gpu_build)
    try:
        host = _host(R, ctx, s, view, 200, 200)
        t = torch.from_numpy(s).cuda()
        torch.cuda.synchronize()
        dev = R.prepare_scene_from_spheres(ctx, t, 200, 200, *view)          # torch tensor, in place
        dev_np = R.prepare_scene_from_spheres(ctx, s, 200, 200, *view)       # numpy, through a temporary device buffer
        _same_prepared(dev, host, name)
        _same_prepared(dev_np, host, f"{name} (numpy)")
        if name == "tall":
            assert host.height > 15, host.height
        want = _frames(R, ctx, host, sides, pixels=not degenerate)
        _same_frames(_frames(R, ctx, dev, sides, pixels=not degenerate), want, name)
        if not degenerate:
            # culling forced wherever the guards pass: the guards themselves are what is compared
            ctx.set_option("cull", 1)
            ctx.set_variant(R.VARIANT_POOLED)
            ll = []
            for ps in (host, dev_np):
                R.render_image(ps, 200, 200, ps.camera() + np.float32(0.25), max_depth=5)   # (a new view: its first frame)
                ll.append(ctx.last_launch)
            assert ll[0] == ll[1], (name, ll)
            ctx.set_option("cull", -1)
            ctx.set_variant(R.VARIANT_AUTO)
        if name in ("rgbbox", "irreg"):
            gold = O.load_golden(name)
            ps5 = R.prepare_scene_from_spheres(ctx, t, 500, 500, *view)
            for v in (R.VARIANT_AUTO, R.VARIANT_POOLED, R.VARIANT_PIXEL):
                ctx.set_variant(v)
                assert int((R.render(500, 500, ps5) != gold).sum()) == 0, (name, v)
            ctx.set_variant(R.VARIANT_AUTO)
            ps5.free()
        for ps in (host, dev, dev_np):
            ps.free()
    finally:
        ctx.close()


def _view_sequence(R, ctx, ps, rays):
    """the same view three times, a batch, a second view, and the three ray queries on the camera's rays"""
    import torch
    h = w = 300
    out = [R.render(h, w, ps) for _ in range(3)]
    buf = torch.full((3, h, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=h * w)
    ctx.sync()
    out += list(buf.cpu().numpy())
    cam2 = ps.camera().copy()
    cam2[0:3] += np.float32(3.0)
    cam2[3:6] += np.float32(3.0)
    out += [R.render_image(ps, w, h, cam2) for _ in range(2)]
    idx, hit = R.intersect_rays(ps, rays)
    occ = R.occluded_rays(ps, rays)
    cnt, midx, root, mhit = R.multi_hit_rays(ps, rays, 4)
    return out, (idx, hit, occ, cnt, midx, root, mhit)


def _fresh_want(R, ctx, s, view, rays):
    ps = _host(R, ctx, s, view, 300, 300)
    img = R.render(300, 300, ps)
    first_launch = ctx.last_launch
    cam2 = ps.camera().copy()
    cam2[0:3] += np.float32(3.0)
    cam2[3:6] += np.float32(3.0)
    img2 = R.render_image(ps, 300, 300, cam2)
    idx, hit = R.intersect_rays(ps, rays)
    occ = R.occluded_rays(ps, rays)
    mh = R.multi_hit_rays(ps, rays, 4)
    ps.free()
    return [img] * 6 + [img2] * 2, (idx, hit, occ) + tuple(mh), first_launch   # (three frames and a batch of three; the second view twice)


def _check_sequence(got, want, what):
    (gi, gr), (wi, wr, _) = got, want
    assert len(gi) == len(wi) and len(gr) == len(wr), what
    for k, (a, b) in enumerate(zip(gi, wi)):
        assert int((a != b).sum()) == 0, f"{what}: frame {k}: {int((a != b).sum())} pixels differ"
    for k, (a, b) in enumerate(zip(gr, wr)):
        E.same_bits(a, b, f"{what}: ray output {k}")


def test_update_resets_view_state(R):
    import torch
    a, view = _oracle_scene("irreg")
    rng = np.random.default_rng(5)
    b = a.copy()
    b[:, 0:3] += rng.uniform(-3, 3, (len(b), 3)).astype(np.float32)
    b[:, 6] *= rng.uniform(0.7, 1.3, len(b)).astype(np.float32)
    ctx = _ctx(R)
    try:
        probe = _host(R, ctx, a, view, 300, 300)
        rays = R.camera_rays(probe, 64, 64)
        probe.free()
        want_a, want_b = _fresh_want(R, ctx, a, view, rays), _fresh_want(R, ctx, b, view, rays)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        ps = R.prepare_scene_from_spheres(ctx, ta, 300, 300, *view)
        _check_sequence(_view_sequence(R, ctx, ps, rays), want_a, "A")
        for t, want, what in ((tb, want_b, "A -> B"), (ta, want_a, "B -> A")):
            ps.update_spheres(t)
            img = R.render(300, 300, ps)
            assert ctx.last_launch == want[2], f"{what}: first frame after the update {ctx.last_launch!r}, a fresh scene's {want[2]!r}"
            assert int((img != want[0][0]).sum()) == 0, what
            _check_sequence(_view_sequence(R, ctx, ps, rays), want, what)
        ps.free()
    finally:
        ctx.close()


def test_animation_on_torch_stream(R):
    """Spheres moved by torch ops on the stream the context shares, an update and a frame per step, no explicit synchronisation between
    them: every frame equals a fresh prepare of the same bytes.  One step makes the tree taller than 15 levels (the SPILL shape), one
    shrinks a radius below the reach guard (culling off) and the next restores it (on again)."""
    import torch
    s0, view = _oracle_scene("irreg")
    stream = torch.cuda.current_stream()
    ctx = R.Context(0, stream=stream.cuda_stream)
    ctx.set_option("sync_policy", 1)
    ctx.set_option("cull", 1)
    ctx.set_variant(R.VARIANT_POOLED)
    try:
        h = w = 500
        t = torch.from_numpy(s0).cuda()
        ps = R.prepare_scene_from_spheres(ctx, t, h, w, *view)
        out = torch.empty((h, w), dtype=torch.int32, device="cuda")
        tall = torch.from_numpy(E._tall(len(s0) - 31)).cuda()
        step_v = torch.linspace(-0.5, 0.5, t.shape[0], device="cuda")
        heights, culled = [], []
        for step in range(10):
            if step == 4:
                t.copy_(tall)                                  # a 30-level Morton chain over coincident centres: far past 15 levels
            elif step == 5:
                t.copy_(torch.from_numpy(s0).cuda())
            elif step == 6:
                t[17, 6] = 1e-3                                # below the reach guard (2 (R + r_max) > 2^15 r_min): no culling
            elif step == 7:
                t[17, 6] = float(s0[17, 6])
            else:
                t[:, 1] += step_v                              # a torch op on the shared stream
            ps.update_spheres(t)
            R.render_into(out.data_ptr(), h, w, ps)
            got, launch = out.cpu().numpy(), ctx.last_launch
            heights.append(ps.height)
            culled.append("+CULL" in launch)
            fresh = _host(R, ctx, t.cpu().numpy(), view, h, w)
            want = R.render(h, w, fresh)
            assert launch == ctx.last_launch, f"step {step}: {launch!r} != {ctx.last_launch!r}"
            _same_prepared(ps, fresh, f"step {step}")
            fresh.free()
            assert int((got != want).sum()) == 0, f"step {step}: {int((got != want).sum())} pixels differ"
        assert heights[4] > 15 and heights[5] <= 15, heights
        assert culled[5] and not culled[4] and not culled[6] and culled[7], (culled, heights)
        ps.free()
    finally:
        ctx.close()


def test_source_buffer_reusable_after_update(R):
    import torch
    a, view = _oracle_scene("irreg")
    b = a.copy()
    b[:, 0] += 1.5
    ctx = _ctx(R)
    try:
        fresh = _host(R, ctx, b, view, 200, 200)
        want = R.render(200, 200, fresh)
        fresh.free()
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        ps = R.prepare_scene_from_spheres(ctx, t, 200, 200, *view)
        t.copy_(torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
        ps.update_spheres(t)
        t.fill_(float("nan"))                                  # right after the update returns
        t2 = torch.from_numpy(a).cuda()
        ps_other = R.prepare_scene_from_spheres(ctx, t2, 200, 200, *view)
        del t2                                                 # (freed: its memory may be reused by torch at once)
        torch.cuda.synchronize()
        for _ in range(3):
            assert int((R.render(200, 200, ps) != want).sum()) == 0
        ps.free()
        ps_other.free()
    finally:
        ctx.close()


def test_refusals(R):
    import torch
    from raytracers_amd._lib import lib
    s, view = _oracle_scene("rgbbox")
    n = len(s)
    ctx = _ctx(R)
    other = _ctx(R)
    multi = R.Context(devices=[0, 0])
    try:
        t = torch.from_numpy(s).cuda()
        torch.cuda.synchronize()
        ps = R.prepare_scene_from_spheres(ctx, t, 100, 100, *view)
        want = R.render(100, 100, ps)
        lf, la = (C.c_float * 3)(*view[0]), (C.c_float * 3)(*view[1])
        p = C.c_void_p()
        ptr = C.c_void_p(t.data_ptr())

        def refused(c, rc, what):
            assert rc != 0, what
            assert lib.rt_last_error(c._h).decode(), what

        for args, what in (((None, 100, 100, ptr, n, lf, la, 50.0), "null out"),
                           ((C.byref(p), 100, 100, None, n, lf, la, 50.0), "null spheres"),
                           ((C.byref(p), 100, 100, ptr, n, None, la, 50.0), "null look_from"),
                           ((C.byref(p), 100, 100, ptr, n, lf, None, 50.0), "null look_at"),
                           ((C.byref(p), 0, 100, ptr, n, lf, la, 50.0), "h = 0"),
                           ((C.byref(p), 100, -1, ptr, n, lf, la, 50.0), "w < 0"),
                           ((C.byref(p), 100, 100, ptr, 1, lf, la, 50.0), "n = 1"),
                           ((C.byref(p), 100, 100, ptr, (1 << 26) + 1, lf, la, 50.0), "n > 2^26")):
            refused(ctx, lib.rt_prepare_scene_device(ctx._h, *args), what)
        refused(multi, lib.rt_prepare_scene_device(multi._h, C.byref(p), 100, 100, ptr, n, lf, la, 50.0), "multi-device prepare")
        assert lib.rt_prepare_scene_device(None, C.byref(p), 100, 100, ptr, n, lf, la, 50.0) != 0
        for c, ps_h, sp, nn, what in ((ctx, None, ptr, n, "null ps"), (ctx, ps._h, None, n, "null spheres"),
                                      (ctx, ps._h, ptr, n - 1, "different n"), (ctx, ps._h, ptr, 1, "n = 1"),
                                      (ctx, ps._h, ptr, (1 << 26) + 1, "n > 2^26"), (multi, ps._h, ptr, n, "multi-device update"),
                                      (other, ps._h, ptr, n, "not the home context")):
            refused(c, lib.rt_prepared_update_spheres(c._h, ps_h, sp, nn), what)
        assert lib.rt_prepared_update_spheres(None, ps._h, ptr, n) != 0
        with pytest.raises(ValueError):
            ps.update_spheres(t[:, :6].contiguous())
        with pytest.raises(ValueError):
            ps.update_spheres(t.double())
        with pytest.raises(ValueError):
            ps.update_spheres(t.t().contiguous().t())            # (n, 7), not contiguous
        with pytest.raises(ValueError):
            ps.update_spheres(t.cpu())
        with pytest.raises(ValueError):
            ps.update_spheres(s[:, :6])
        with pytest.raises(ValueError):
            R.prepare_scene_from_spheres(ctx, s.reshape(-1), 100, 100, *view)
        with pytest.raises(R.RtError):
            ps.update_spheres(s[:-1])
        # a refused update leaves the scene as it was
        assert ps.num_spheres == n
        assert int((R.render(100, 100, ps) != want).sum()) == 0
        ps.free()
    finally:
        multi.close()
        other.close()
        ctx.close()
