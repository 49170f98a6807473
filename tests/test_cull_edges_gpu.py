"""The CULL instantiations of the pooled kernel at the limits of the guards that admit them (cases: edge_cull.py): scenes and
cameras just inside and just outside the scene guard, the camera guard, c_max, r_min and the height guard, images that straddle the d.d gate,
ties, and bounce chains between tiny and huge spheres.  Every image is compared bit for bit with the oracle's render through the same cam12,
and rt_context_last_launch must say +CULL exactly where edge_cull's float64 restatement of the guards says so (launches of 16 or 4 waves).
test_cull_edges_cpu.py holds the same cases against the host code and the per-ray arithmetic on the CPU."""
import functools

import numpy as np
import pytest

import edge_cull as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = tuple(E.cases())
PAIRS = tuple(n for n in CASES if "pair" in E.cases()[n].tags)
POISON = 0x5a5a5a5a
# the launch shapes of the culled loop: the scene read from L2 by 16 waves (as the plan picks the shape, and configured), staged in LDS, the
# wide_waves switch with and without the test capacity of the box stack, and twenty waves per CU (five workgroups of four) whose box stacks
# spill at that capacity
SHAPES = (dict(lds_scene_bytes=0), dict(), dict(wide_waves=2), dict(wide_waves=2, stack_cap=192),
          dict(waves_per_wg=16, wgs_per_cu=1, lds_scene_bytes=0), dict(waves_per_wg=4, wgs_per_cu=5, stack_cap=192))
L2_16 = dict(waves_per_wg=16, wgs_per_cu=1, lds_scene_bytes=0)
DEFAULTS = dict(lds_scene_bytes=-1, wide_waves=1, stack_cap=0, waves_per_wg=0, wgs_per_cu=1, cull=-1, gpu_build=1)
LOOK = ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 40.0)          # the prepared camera is never used: every render takes a cam12


@pytest.fixture(scope="module")
def R():
    import raytracers_amd
    return raytracers_amd


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _want(name):
    c = E.cases()[name]
    orc = O.OracleScene("custom", spheres7=c.spheres7, look_from=LOOK[0], look_at=LOOK[1], fov=LOOK[2])
    return tuple(orc.render(c.h, c.w, cam=cam)[0] for cam in c.cams)


def _restore(R, ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.set_variant(R.VARIANT_AUTO)


def _decision(ll, expect, what):
    """+CULL in the launch's name iff expected, for the shapes the CULL instantiations exist for; never otherwise."""
    if "waves=16" in ll or "waves=4" in ll:
        assert ("+CULL" in ll) == bool(expect), (what, expect, ll)
    else:
        assert "+CULL" not in ll, (what, ll)


def _same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape and int((got != want).sum()) == 0, (what, int((got != want).sum()))


@pytest.mark.parametrize("name", CASES)
def test_culled_edge_case(R, ctx, name):
    import torch
    case = E.cases()[name]
    want = _want(name)
    h, w, k = case.h, case.w, len(case.cams)
    per_cam = [case.scene_ok and ok for ok in case.origin_ok]
    scene = ctx.scene_from_spheres(case.spheres7, *LOOK)
    ps = R.prepare_scene(h, w, scene)
    out = torch.empty((h, w), dtype=torch.int32, device="cuda")
    buf = torch.empty((k, h, w), dtype=torch.int32, device="cuda")
    seen = set()
    try:
        ctx.set_variant(R.VARIANT_POOLED)
        for shape in SHAPES:
            for key, v in shape.items():
                ctx.set_option(key, v)
            try:
                ctx.set_option("cull", 1)
                # frames 1 .. 3 of a view (the first records it, the second orders the record, then the policy), into a poisoned image
                for frame in range(3):
                    out.fill_(POISON)
                    torch.cuda.synchronize()
                    R.render_into(out.data_ptr(), h, w, ps, cam=case.cams[0])
                    ctx.sync()
                    ll = ctx.last_launch
                    _same(out.cpu().numpy(), want[0], (name, shape, "frame", frame, ll))
                    _decision(ll, per_cam[0], (name, shape, "frame", frame))
                    seen.add(("waves=16" in ll, "waves=4" in ll, "+SPILL" in ll, "+CULL" in ll))
                if "waves_per_wg" in shape:
                    assert f"waves={shape['waves_per_wg']}" in ll, (name, shape, ll)
                if shape.get("waves_per_wg") == 4:
                    assert "+SPILL" in ll, (name, shape, ll)
                # render_image through each cam12
                for i, cam in enumerate(case.cams):
                    got = R.render_image(ps, w, h, cam)
                    ll = ctx.last_launch
                    _same(got, want[i], (name, shape, "render_image", i, ll))
                    _decision(ll, per_cam[i], (name, shape, "render_image", i))
                # one batch with the case's cameras: culled only if every origin passes
                buf.fill_(POISON)
                torch.cuda.synchronize()
                R.render_batch_into(buf.data_ptr(), h, w, ps, k, frame_stride=h * w, cams=np.stack(case.cams))
                ctx.sync()
                ll = ctx.last_launch
                frames = buf.cpu().numpy()
                for i in range(k):
                    _same(frames[i], want[i], (name, shape, "batch", i, ll))
                _decision(ll, case.expect_culled, (name, shape, "batch"))
                # the same frame with culling switched off
                ctx.set_option("cull", 0)
                out.fill_(POISON)
                torch.cuda.synchronize()
                R.render_into(out.data_ptr(), h, w, ps, cam=case.cams[0])
                ctx.sync()
                assert "+CULL" not in ctx.last_launch, (name, shape, ctx.last_launch)
                _same(out.cpu().numpy(), want[0], (name, shape, "cull=0", ctx.last_launch))
            finally:
                for key in shape:
                    ctx.set_option(key, DEFAULTS[key])
                ctx.set_option("cull", DEFAULTS["cull"])
        # every shape ran, and where the guards pass each of them ran culled
        assert any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen), (name, seen)
        if per_cam[0]:
            assert any(s[0] and s[3] for s in seen) and any(s[1] and s[2] and s[3] for s in seen), (name, seen)
        # ... and the pixel kernel, which never culls
        ctx.set_variant(R.VARIANT_PIXEL)
        for i, cam in enumerate(case.cams):
            _same(R.render_image(ps, w, h, cam), want[i], (name, "pixel kernel", i, ctx.last_launch))
            assert "+CULL" not in ctx.last_launch
    finally:
        _restore(R, ctx)
        ps.free()
        scene.free()


@pytest.mark.parametrize("gpu_build", [1, 0])
@pytest.mark.parametrize("name", PAIRS)
def test_guard_pairs_from_device_spheres(R, ctx, name, gpu_build):
    """The guard pairs prepared from spheres in device memory (rt_prepare_scene_device: the statistics reduced on the device) and rebuilt in
    place from them (rt_prepared_update_spheres, over a scene that decided the other way or had other constants): the decision and the
    pixels of the host path."""
    case = E.cases()[name]
    want = _want(name)[0]
    h, w, n = case.h, case.w, len(case.spheres7)
    expect = case.scene_ok and case.origin_ok[0]
    before = E.cases()["scene_out" if case.scene_ok else "control"].spheres7[:n]
    try:
        ctx.set_variant(R.VARIANT_POOLED)
        ctx.set_option("gpu_build", gpu_build)
        for key, v in L2_16.items():
            ctx.set_option(key, v)
        ctx.set_option("cull", 1)
        scene = ctx.scene_from_spheres(case.spheres7, *LOOK)
        host = R.prepare_scene(h, w, scene)
        fresh = R.prepare_scene_from_spheres(ctx, case.spheres7, h, w, *LOOK)
        updated = R.prepare_scene_from_spheres(ctx, before, h, w, *LOOK)
        R.render_image(updated, w, h, case.cams[0])              # (a view of the scene it is about to lose)
        updated.update_spheres(case.spheres7)
        for what, ps in (("host", host), ("device", fresh), ("updated", updated)):
            for frame in range(2):
                got = R.render_image(ps, w, h, case.cams[0])
                ll = ctx.last_launch
                assert "waves=16" in ll and ("+CULL" in ll) == bool(expect), (name, what, frame, expect, ll)
                _same(got, want, (name, what, frame, ll))
            ps.free()
        scene.free()
    finally:
        _restore(R, ctx)
