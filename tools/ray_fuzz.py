#!/usr/bin/env python3
"""Randomised campaign for the caller-ray entries: random scenes (the kinds of fuzz_parity.py), rays drawn from the edge families of
tests/edge_rays.py and at random, random per-ray intervals; rt_trace_rays (pooled and pixel families), rt_intersect_rays[_ranged],
rt_occluded_rays[_ranged] (pooled shapes, lane kernel, AUTO) and rt_multi_hit_rays[_ranged] against the numpy restatements, bit for bit
(any NaN matches any NaN).
usage: ray_fuzz.py [seconds] [seed] [max spheres = 1500]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import edge_rays as E
from fuzz_scenes import random_scene
import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import ray_query_ref as Q
import raytracers_amd as R

F = np.float32
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
max_n = int(sys.argv[3]) if len(sys.argv) > 3 else 1500
ctx = R.Context()
t_end = time.time() + budget
cases = fails = 0


def check(what, got, want):
    global ok
    try:
        E.same_bits(got, want, what)
    except AssertionError as e:
        ok = False
        print(f"  {e}", flush=True)


while time.time() < t_end:
    seed = seed0 + cases
    rng = np.random.default_rng(seed)
    s, kind = random_scene(rng, max_n)
    scene = ctx.scene_from_spheres(s, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 60.0)
    ps = R.prepare_scene(16, 16, scene)
    arr = ps.bvh_arrays()
    ref = Q.RefScene(arr)
    fam = E.ray_families(arr, seed=seed, per=8)
    picks = [v[rng.permutation(v.shape[0])[: int(rng.integers(1, 24))]] for v in fam.values()]
    rays = np.concatenate(picks + [X.seeded_rays(arr, int(rng.integers(16, 512)), seed)])
    rays = rays[rng.permutation(rays.shape[0])]
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    lo_e, hi_e, _ = E.edge_intervals(arr, rays, seed=seed)
    lo_m, hi_m, _ = V.mixed_intervals(n, seed=seed)
    pick = rng.random(n) < 0.5
    lo, hi = np.where(pick, lo_e, lo_m).astype(F), np.where(pick, hi_e, hi_m).astype(F)
    t0, t1 = [(0.0, 1e9), (0.1, 1e9), (0.5, 30.0), (1e-3, 1.0)][int(rng.integers(0, 4))]
    ok = True
    try:
        depth = int(rng.choice([1, 2, 3, 50]))
        want_c = ref.ray_colour(o, d, depth)
        for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL):
            ctx.set_variant(variant)
            col, px = R.trace_rays(ps, rays, max_depth=depth)
            check(f"trace variant {variant} depth {depth}", col, want_c)
        ctx.set_variant(R.VARIANT_AUTO)
        idx, hit = R.intersect_rays(ps, rays, t0, t1)
        wi, wh = ref.objs_hit(o, d, F(t0), F(t1))
        check("intersect index", idx, wi); check("intersect hit7", hit, wh)
        idx, hit = R.intersect_rays(ps, rays, lo, hi)
        wi, wh = V.objs_hit(ref, o, d, lo, hi)
        check("intersect per-ray index", idx, wi); check("intersect per-ray hit7", hit, wh)
        w_s, w_r = X.occluded(ref, o, d, t0, t1), V.occluded(ref, o, d, lo, hi)
        shape = [{}, {"lds_scene_bytes": 0}, {"wide_waves": 2}, {"wide_waves": 2, "stack_cap": 192}][int(rng.integers(0, 4))]
        for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_AUTO):
            ctx.set_variant(variant)
            for k_, v_ in shape.items():
                ctx.set_option(k_, v_)
            try:
                check(f"occluded variant {variant} {shape}", R.occluded_rays(ps, rays, t0, t1), w_s)
                check(f"occluded per-ray variant {variant} {shape}", R.occluded_rays(ps, rays, lo, hi), w_r)
            finally:
                ctx.set_option("wide_waves", 1); ctx.set_option("stack_cap", 0); ctx.set_option("lds_scene_bytes", -1)
        ctx.set_variant(R.VARIANT_AUTO)
        k = int(rng.integers(1, 33))
        for b, what in (((t0, t1), "scalar"), ((lo, hi), "per-ray")):
            got = R.multi_hit_rays(ps, rays, k, *b)
            want = M.multi_hit(ref, o, d, *(b if what == "per-ray" else (F(t0), F(t1))), k)
            for part, g, w in zip(("count", "index", "root", "hit7"), got, want):
                check(f"multi-hit {what} k={k} {part}", g, w)
    except Exception as e:                      # an entry that raises is a mismatch too
        ok = False
        print(f"  {type(e).__name__}: {e}", flush=True)
    ps.free(); scene.free()
    cases += 1
    if not ok:
        fails += 1
        print(f"MISMATCH seed {seed}: n={s.shape[0]} kind={kind} rays={n} interval=({t0}, {t1})", flush=True)
ctx.set_variant(R.VARIANT_AUTO)
print(f"ray_fuzz: {cases} cases, {fails} mismatches (seeds {seed0}..{seed0 + cases - 1})", flush=True)
sys.exit(1 if fails else 0)
