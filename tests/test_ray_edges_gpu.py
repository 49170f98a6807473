"""The caller-ray entries on the GPU against the numpy restatements, on the edge scenes, ray families and intervals of edge_rays.py: NaN and
+-inf components, zero / denormal / tiny / huge directions, -0.0 slab swaps, origins on box faces, tangent rays, roots on kEps and on the
interval's ends, and ties in t.  test_ray_edges_cpu.py holds each restatement equal to the C oracle's literal walk on the same inputs.
Every comparison is bit for bit (edge_rays.same_bits: any NaN matches any NaN)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_rays as E
import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = tuple(E.SCENES)
POOLED_ANY = "family=pooled tickets=rays instantiation=any"
PER_RAY = " intervals=per-ray"
KS = (1, 4, 5, 8, 9, 16, 17, 32)      # each list capacity of the multi-hit lane kernel and one past it
same_bits = E.same_bits


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


@functools.lru_cache(maxsize=None)
def _inputs(name):
    s, lf, la, fov = E.SCENES[name]
    arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    rays = np.concatenate(list(E.ray_families(arr, seed=1).values()))
    lo, hi, _ = E.edge_intervals(arr, rays, seed=2)
    return arr, Q.RefScene(arr), rays, lo, hi


@functools.lru_cache(maxsize=None)
def _want_colour(name, depth):
    _, ref, rays, _, _ = _inputs(name)
    return ref.ray_colour(rays[:, :3], rays[:, 3:], depth)


@functools.lru_cache(maxsize=None)
def _want_multi(name, ranged):
    _, ref, rays, lo, hi = _inputs(name)
    b = (lo, hi) if ranged else (F(0.0), F(1e9))
    return M.multi_hit(ref, rays[:, :3], rays[:, 3:], *b, max(KS))


def _prepared(R, ctx, name):
    s, lf, la, fov = E.SCENES[name]
    arr = _inputs(name)[0]
    scene = ctx.scene_from_spheres(s, lf, la, fov)
    ps = R.prepare_scene(64, 64, scene)
    got = ps.bvh_arrays()
    for k in ("left", "right", "parent"):
        assert (got[k] == arr[k]).all(), (name, k)
    for k in ("L", "bmin", "bmax"):
        assert got[k].tobytes() == arr[k].tobytes(), (name, k)
    return scene, ps


def _free(scene, ps):
    ps.free()
    scene.free()


def _same_pixels(pixel, colour, what):
    # colour_to_pixel of a NaN colour is the conversion's own business (x86 and the GPU differ); every finite colour's pixel must match
    fin = np.isfinite(colour).all(axis=1)
    assert fin.any(), what
    same_bits(pixel[fin], Q.colour_to_pixel(colour[fin]), what + " pixel")


@pytest.mark.parametrize("name", SCENES)
def test_trace_rays(R, ctx, name):
    _, _, rays, _, _ = _inputs(name)
    scene, ps = _prepared(R, ctx, name)
    try:
        for variant, family in ((R.VARIANT_POOLED, "family=pooled tickets=rays"), (R.VARIANT_PIXEL, "family=pixel (rays)")):
            ctx.set_variant(variant)
            for depth in (1, 2, 50):
                want = _want_colour(name, depth)
                colour, pixel = R.trace_rays(ps, rays, max_depth=depth)
                assert ctx.last_launch.startswith(family), (name, ctx.last_launch)
                same_bits(colour, want, f"{name} {family} depth {depth} colour")
                _same_pixels(pixel, want, f"{name} {family} depth {depth}")
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
    _free(scene, ps)


@pytest.mark.parametrize("name", SCENES)
def test_intersect_rays(R, ctx, name):
    _, ref, rays, lo, hi = _inputs(name)
    o, d = rays[:, :3], rays[:, 3:]
    scene, ps = _prepared(R, ctx, name)
    for t0, t1 in ((0.0, 1e9), (0.1, 40.0), (0.1, 0.1)):
        idx, hit = R.intersect_rays(ps, rays, t0, t1)
        assert ctx.last_launch == "family=intersect", ctx.last_launch
        wi, wh = ref.objs_hit(o, d, F(t0), F(t1))
        same_bits(idx, wi, f"{name} ({t0}, {t1}) index")
        same_bits(hit, wh, f"{name} ({t0}, {t1}) hit7")
    idx, hit = R.intersect_rays(ps, rays, lo, hi)
    assert ctx.last_launch == "family=intersect (per-ray)", ctx.last_launch
    wi, wh = V.objs_hit(ref, o, d, lo, hi)
    same_bits(idx, wi, f"{name} per-ray index")
    same_bits(hit, wh, f"{name} per-ray hit7")
    _free(scene, ps)


def test_occluded_rays_every_shape(R, ctx):
    # the pooled any-hit loop in every shape -- 16 waves with the scene in LDS and without (lds_scene_bytes=0), 4 waves, +SPILL at the test
    # capacity -- the lane kernel and AUTO, scalar and per-ray, on every edge scene and on a tree too large for LDS (height 43, 5031 spheres:
    # the only one here on which wide_waves=2 gives the four-wave, twenty-per-CU shape)
    shapes = ({}, {"lds_scene_bytes": 0}, {"wide_waves": 2}, {"wide_waves": 2, "stack_cap": 192})
    seen = set()
    for name in SCENES + ("tall5000",):
        if name == "tall5000":
            s, lf, la, fov = E._tall(5000), (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0
            arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
            ref = Q.RefScene(arr)
            rays = np.concatenate([v[:24] for v in E.ray_families(arr, seed=3).values()])
            lo, hi, _ = E.edge_intervals(arr, rays, seed=4)
            scene = ctx.scene_from_spheres(s, lf, la, fov)
            ps = R.prepare_scene(64, 64, scene)
            assert ps.bvh_arrays()["bmin"].tobytes() == arr["bmin"].tobytes()
        else:
            _, ref, rays, lo, hi = _inputs(name)
            scene, ps = _prepared(R, ctx, name)
        o, d = rays[:, :3], rays[:, 3:]
        want = {"scalar": X.occluded(ref, o, d, 0.0, 1e9), "scalar eps": X.occluded(ref, o, d, 0.1, 30.0),
                "per-ray": V.occluded(ref, o, d, lo, hi)}
        bounds = {"scalar": (0.0, 1e9), "scalar eps": (0.1, 30.0), "per-ray": (lo, hi)}
        try:
            ctx.set_variant(R.VARIANT_POOLED)
            for opts in shapes:
                for key, v in opts.items():
                    ctx.set_option(key, v)
                try:
                    for what, b in bounds.items():
                        got = R.occluded_rays(ps, rays, *b)
                        ll = ctx.last_launch
                        assert ll.startswith(POOLED_ANY) and ("waves=16" in ll or "waves=4" in ll), (name, opts, ll)
                        assert ll.endswith(PER_RAY) == (what == "per-ray"), (name, opts, ll)
                        same_bits(got, want[what], f"{name} pooled {opts} {what}")
                    ctx.set_variant(R.VARIANT_AUTO)
                    R.occluded_rays(ps, rays, 0.0, 1e9)
                    in_lds = ctx.last_launch.startswith(POOLED_ANY)     # AUTO takes the pooled loop iff the scene is staged in LDS whole
                    ctx.set_variant(R.VARIANT_POOLED)
                    assert not (in_lds and "lds_scene_bytes" in opts), (name, ctx.last_launch)
                    seen.add(("waves=16" in ll and in_lds, "waves=16" in ll and not in_lds, "waves=4" in ll, "+SPILL" in ll))
                finally:
                    ctx.set_option("wide_waves", 1)
                    ctx.set_option("stack_cap", 0)
                    ctx.set_option("lds_scene_bytes", -1)
            for variant in (R.VARIANT_PIXEL, R.VARIANT_AUTO):
                ctx.set_variant(variant)
                for what, b in bounds.items():
                    got = R.occluded_rays(ps, rays, *b)
                    ll = ctx.last_launch
                    if what == "per-ray":
                        assert ll == "family=occluded (per-ray)", (name, variant, ll)
                    elif variant == R.VARIANT_PIXEL:
                        assert ll == "family=occluded", (name, variant, ll)
                    else:
                        assert ll == "family=occluded" or ll.startswith(POOLED_ANY), (name, variant, ll)
                    same_bits(got, want[what], f"{name} variant {variant} {what}")
        finally:
            ctx.set_variant(R.VARIANT_AUTO)
        _free(scene, ps)
    # every shape ran: 16 waves in LDS, 16 waves without, 4 waves, +SPILL
    for i, shape in enumerate(("16 waves in LDS", "16 waves without", "4 waves", "+SPILL")):
        assert any(k[i] for k in seen), (shape, seen)


@pytest.mark.parametrize("name", SCENES)
def test_multi_hit_rays(R, ctx, name):
    _, ref, rays, lo, hi = _inputs(name)
    scene, ps = _prepared(R, ctx, name)
    for ranged in (False, True):
        want = _want_multi(name, ranged)
        b = (lo, hi) if ranged else (0.0, 1e9)
        for k in KS:
            got = R.multi_hit_rays(ps, rays, k, *b)
            assert ctx.last_launch == f"family=multi-hit k={k}" + (" (per-ray)" if ranged else ""), ctx.last_launch
            for part, g, w in zip(("count", "index", "root", "hit7"), got, want):
                same_bits(g, w[:, :k] if part != "count" else w, f"{name} ranged={ranged} k={k} {part}")
    if name == "overlap":
        assert (_want_multi(name, False)[0] > 32).any()
    _free(scene, ps)


def test_multi_hit_null_outputs(R, ctx):
    import torch
    name = "overlap"
    _, ref, rays_np, lo_np, hi_np = _inputs(name)
    scene, ps = _prepared(R, ctx, name)
    n = rays_np.shape[0]
    rays = torch.from_numpy(rays_np).cuda()
    lo, hi = torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    for ranged in (False, True):
        want = _want_multi(name, ranged)
        for k in (5, 17, 32):
            for keep in ((0,), (1,), (2,), (3,), (0, 3), (1, 2)):
                outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), -7, dtype=torch.int32, device="cuda"),
                        torch.full((n, k), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n, k, 7), -7.0, dtype=torch.float32, device="cuda")]
                ptrs = [t.data_ptr() if i in keep else None for i, t in enumerate(outs)]
                torch.cuda.synchronize()
                if ranged:
                    R.multi_hit_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), k, *ptrs)
                else:
                    R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, *ptrs, t_min=0.0, t_max=1e9)
                ctx.sync()
                for i, t in enumerate(outs):
                    if i in keep:
                        w = want[i] if i == 0 else want[i][:, :k]
                        same_bits(t.cpu().numpy(), w, f"ranged={ranged} k={k} keep={keep} output {i}")
    _free(scene, ps)


def test_unaligned_pointers(R, ctx):
    # rays, bounds and every output as slices of larger tensors: rays 24 bytes in, the rest 4 bytes (or 1, or k) in -- no device pointer is
    # 16-byte aligned
    import torch
    for name in ("random600", "overlap"):
        _, ref, rays_np, lo_np, hi_np = _inputs(name)
        o, d = rays_np[:, :3], rays_np[:, 3:]
        n = rays_np.shape[0]
        scene, ps = _prepared(R, ctx, name)

        def big(shape, dtype, fill):
            t = torch.full((n + 1,) + shape, fill, dtype=dtype, device="cuda")
            return t, t[1:]

        _, rays = big((6,), torch.float32, 0.0)
        rays.copy_(torch.from_numpy(rays_np))
        _, lo = big((), torch.float32, 0.0)
        _, hi = big((), torch.float32, 0.0)
        lo.copy_(torch.from_numpy(lo_np))
        hi.copy_(torch.from_numpy(hi_np))
        for t in (rays, lo, hi):
            assert t.data_ptr() % 16 != 0 and t.is_contiguous()
        torch.cuda.synchronize()
        try:
            for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL):
                ctx.set_variant(variant)
                _, col = big((3,), torch.float32, -7.0)
                _, px = big((), torch.int32, -7)
                torch.cuda.synchronize()
                R.trace_rays_into(rays.data_ptr(), n, ps, col.data_ptr(), px.data_ptr(), max_depth=50)
                ctx.sync()
                want = _want_colour(name, 50)
                same_bits(col.cpu().numpy(), want, f"{name} variant {variant} trace colour")
                _same_pixels(px.cpu().numpy(), want, f"{name} variant {variant} trace")
                _, occ = big((), torch.uint8, 0xAB)
                torch.cuda.synchronize()
                R.occluded_rays_into(rays.data_ptr(), n, ps, occ.data_ptr(), 0.0, 1e9)
                ctx.sync()
                same_bits(occ.cpu().numpy().astype(bool), X.occluded(ref, o, d, 0.0, 1e9), f"{name} variant {variant} occluded")
                occ.fill_(0xAB)
                torch.cuda.synchronize()
                R.occluded_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), occ.data_ptr())
                ctx.sync()
                same_bits(occ.cpu().numpy().astype(bool), V.occluded(ref, o, d, lo_np, hi_np), f"{name} variant {variant} occluded per-ray")
        finally:
            ctx.set_variant(R.VARIANT_AUTO)
        _, idx = big((), torch.int32, -7)
        _, hit = big((7,), torch.float32, -7.0)
        torch.cuda.synchronize()
        R.intersect_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), idx.data_ptr(), hit.data_ptr())
        ctx.sync()
        wi, wh = V.objs_hit(ref, o, d, lo_np, hi_np)
        same_bits(idx.cpu().numpy(), wi, f"{name} intersect per-ray index")
        same_bits(hit.cpu().numpy(), wh, f"{name} intersect per-ray hit7")
        R.intersect_rays_into(rays.data_ptr(), n, ps, idx.data_ptr(), hit.data_ptr(), 0.0, 1e9)
        ctx.sync()
        wi, wh = ref.objs_hit(o, d, F(0.0), F(1e9))
        same_bits(idx.cpu().numpy(), wi, f"{name} intersect index")
        same_bits(hit.cpu().numpy(), wh, f"{name} intersect hit7")
        for k in (5, 32):
            want = _want_multi(name, True)
            outs = [big((), torch.int32, -7)[1], big((k,), torch.int32, -7)[1], big((k,), torch.uint8, 0xAB)[1], big((k, 7), torch.float32, -7.0)[1]]
            torch.cuda.synchronize()
            R.multi_hit_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), k, *[t.data_ptr() for t in outs])
            ctx.sync()
            for i, t in enumerate(outs):
                same_bits(t.cpu().numpy(), want[i] if i == 0 else want[i][:, :k], f"{name} multi-hit per-ray k={k} output {i}")
        _free(scene, ps)


def test_random_ray_campaign():
    """tools/ray_fuzz.py for a bounded time: random scenes, edge and random rays, random per-ray intervals, every caller-ray entry and family
    against the restatements."""
    out = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "tools", "ray_fuzz.py"), "25", "5100"],
                         capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert " 0 mismatches" in out.stdout, out.stdout[-2000:]
