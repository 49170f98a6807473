#!/usr/bin/env python3
"""Randomised campaign for the sphere-cast, proximity and range-query entries: random scenes (fuzz_scenes.py: ray_fuzz.py's, seed for seed),
sweep queries drawn from the edge families of tests/edge_sweeps.py and from seeded_rays with random radii and intervals, points at sphere
centres, on surfaces and far away.  rt_sweep_spheres (scalar), rt_sweep_spheres_ranged (with and without excludes), rt_nearest_spheres[_ranged]
(counted and pruned), rt_spheres_within_* (with `first`) and rt_contact_pairs_* against the numpy restatements, bit for bit (any NaN matches
any NaN).  An entry that raises is a mismatch.
usage: query_fuzz.py [seconds] [seed] [max spheres = 1500]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import edge_rays as E
import edge_sweeps as ES
from fuzz_scenes import random_scene
import interval_ref as V
import occlusion_ref as X
import proximity_ref as P
import ray_query_ref as Q
import sweep_ref as S
import within_ref as W
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


def sweep_queries(arr, rng, seed):
    """(rays, radius, t_min, t_max): a few of every edge family, and seeded rays under random radii and mixed intervals"""
    fam = ES.sweep_families(arr, seed=seed, per=8)
    picks = []
    for v in fam.values():
        take = rng.permutation(v[0].shape[0])[: int(rng.integers(1, 24))]
        picks.append(tuple(a[take] for a in v))
    rays = X.seeded_rays(arr, int(rng.integers(16, 384)), seed)
    m = rays.shape[0]
    r0 = float(ES.median_radius(arr))
    rq = (rng.choice([0.0, 0.5 * r0, r0, 4.0 * r0, 40.0 * r0], m) * rng.uniform(0.5, 1.5, m)).astype(F)
    rq[rng.random(m) < 0.03] = F(np.nan)
    rq[rng.random(m) < 0.03] = F(-1.0)
    lo, hi, _ = V.mixed_intervals(m, seed=seed)
    picks.append((rays, rq, lo, hi))
    out = tuple(np.concatenate([p[i] for p in picks]) for i in range(4))
    perm = rng.permutation(out[0].shape[0])
    return tuple(a[perm] for a in out)


def query_points(L, rng, origins):
    n = L.shape[0]
    j = rng.integers(0, n, 96)
    u = rng.normal(size=(96, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    axis = np.eye(3, dtype=F)[rng.integers(0, 3, 32)] * rng.choice([-1.0, 1.0], (32, 1)).astype(F)
    pts = [L[j[:32], :3], L[j[32:64], :3] + axis * L[j[32:64], 6:7], L[j[64:], :3] + u[64:] * L[j[64:], 6:7],
           L[j[:16], :3] + u[:16] * 1e6, origins[: int(rng.integers(1, 64))]]
    return np.ascontiguousarray(np.concatenate(pts), dtype=F)


while time.time() < t_end:
    seed = seed0 + cases
    rng = np.random.default_rng(seed)
    s, kind = random_scene(rng, max_n)
    scene = ctx.scene_from_spheres(s, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 60.0)
    ps = R.prepare_scene(16, 16, scene)
    arr = ps.bvh_arrays()
    L = np.asarray(arr["L"], dtype=F)
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    rays, rq, lo, hi = sweep_queries(arr, rng, seed)
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    r0 = float(ES.median_radius(arr))
    t0, t1 = [(0.0, 1e9), (0.0, 1.0), (0.1, 1e9), (0.5, 30.0)][int(rng.integers(0, 4))]
    rs = float(F(rng.choice([0.0, -0.0, r0, 8.0 * r0, 1e8])))
    ok = True
    try:
        names = ("count", "index", "start", "hit7")
        k = int(rng.integers(1, 33))
        for part, g, w in zip(names, R.sweep_spheres(ps, rays, rs, k, t0, t1), S.sweep(ref, o, d, rs, t0, t1, k)):
            check(f"sweep scalar radius {rs} k={k} {part}", g, w)
        k = int(rng.integers(1, 33))
        for part, g, w in zip(names, R.sweep_spheres(ps, rays, rq, k, lo, hi), S.sweep(ref, o, d, rq, lo, hi, k)):
            check(f"sweep per-query k={k} {part}", g, w)
        k = int(rng.integers(1, 33))
        first_hit = S.sweep(ref, o, d, rq, lo, hi, 1)[1][:, 0]
        ex = np.where(rng.random(n) < 0.5, first_hit, rng.integers(-2, L.shape[0] + 2, n)).astype(np.int64)
        for part, g, w in zip(names, R.sweep_spheres(ps, rays, rq, k, lo, hi, exclude=ex), S.sweep(ref, o, d, rq, lo, hi, k, ex)):
            check(f"sweep exclude k={k} {part}", g, w)
        pts = query_points(L, rng, o)
        m = pts.shape[0]
        md_s = float(F(rng.choice([0.0, r0, 6.0 * r0, 1e9])))
        md = (rng.choice([0.0, r0, 6.0 * r0], m) * rng.uniform(0.0, 2.0, m)).astype(F)
        md[rng.random(m) < 0.05] = F(np.nan)
        md[rng.random(m) < 0.05] = F(-0.0)
        k = int(rng.integers(1, 33))
        for bound, what in ((md_s, "scalar"), (md, "per-point")):
            want = P.nearest(L, pts, bound, k)
            for counted in (True, False):
                got = R.nearest_spheres(ps, pts, k, bound, count=counted)
                if counted:
                    check(f"nearest {what} k={k} count", got[0], want[0])
                check(f"nearest {what} k={k} counted={counted} index", got[1], want[1])
                check(f"nearest {what} k={k} counted={counted} gap", got[2], want[2])
        first = rng.integers(-1, L.shape[0] + 1, m)
        for bound, fi, what in ((min(md_s, 6.0 * r0), None, "scalar"), (md, first, "per-point first")):
            off, idx, gap, row = R.spheres_within(ps, pts, bound, first=fi, rows=True)
            w_off, w_idx, w_gap = W.within(L, pts, bound, fi)
            check(f"within {what} offsets", off, w_off)
            if w_idx.size and off.shape == w_off.shape and (off == w_off).all():
                check(f"within {what} index", idx, w_idx)
                check(f"within {what} gap", gap, w_gap)
                check(f"within {what} point", row, np.repeat(np.arange(m, dtype=np.int32), np.diff(w_off)))
        margin = float(F(rng.choice([0.0, 0.25 * r0, r0])))
        pairs, gap = R.contact_pairs(ps, margin)
        w_pairs, w_gap = W.contact_pairs(L, margin)
        if w_pairs.shape[0] == 0:
            ok = ok and pairs.shape[0] == 0
        else:
            check(f"contact pairs margin {margin}", pairs, w_pairs)
            if pairs.shape == w_pairs.shape:
                check(f"contact pairs margin {margin} gap", gap, w_gap)
    except Exception as e:                      # an entry that raises is a mismatch too
        ok = False
        print(f"  {type(e).__name__}: {e}", flush=True)
    ps.free(); scene.free()
    cases += 1
    if not ok:
        fails += 1
        print(f"MISMATCH seed {seed}: n={s.shape[0]} kind={kind} queries={n} interval=({t0}, {t1}) radius={rs}", flush=True)
print(f"query_fuzz: {cases} cases, {fails} mismatches (seeds {seed0}..{seed0 + cases - 1})", flush=True)
sys.exit(1 if fails else 0)
