"""Throughput of the sphere casts on one GPU; prints one JSON line per case (ms per call and Mquery/s = queries answered / us).

    python tools/sweep_probe.py [--iters N] [--floor N]

Self-sweeps: every sphere of a scene swept along a random small displacement (query i = centre and radius of L[i], |d| about its radius,
exclude = i, over (0, 1)) through rt_sweep_spheres_ranged -- irreg and the floor of N x N spheres (default 1000: 10^6), with the queries in L
order (Morton order: neighbouring lanes walk neighbouring leaves) and shuffled, at k = 1 and 8.
Casts: N * N random casts on the floor (origins over it, displacements of 20 units) through rt_sweep_spheres at radius 0, 1 and 30, k = 1 and 8.
The yardstick of every case is rt_multi_hit_rays[_ranged] on the same rays with the same k and interval in the same run: at radius 0 it does the
same walk.  With every output and with count / index only.  A sample of each case's queries goes through tests/sweep_ref.py's walk for the mean
number of box tests and consulted leaves per query (the yardstick's: the same walk at radius 0).  Times are HIP events on a torch stream
the context enqueues on."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raytracers_amd as R  # noqa: E402
import sweep_ref as S  # noqa: E402

KS = (1, 8)
SAMPLE = 2048


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def probe(ctx, ps, arr, case, rays_np, radius, exclude_np, iters):
    """radius: a scalar (the scalar entry) or an [n] array (the ranged entry, over (0, 1) for every query)"""
    n = rays_np.shape[0]
    ranged = np.ndim(radius) > 0
    rays = torch.from_numpy(rays_np).cuda()
    kmax = max(KS)
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    idx = torch.empty(n * kmax, dtype=torch.int32, device="cuda")
    flag = torch.empty(n * kmax, dtype=torch.uint8, device="cuda")
    hit = torch.empty(n * kmax * 7, dtype=torch.float32, device="cuda")
    if ranged:
        rq = torch.from_numpy(np.ascontiguousarray(radius, np.float32)).cuda()
        lo = torch.zeros(n, dtype=torch.float32, device="cuda")
        hi = torch.ones(n, dtype=torch.float32, device="cuda")
        ex = torch.from_numpy(np.ascontiguousarray(exclude_np, np.int32)).cuda() if exclude_np is not None else None
    torch.cuda.synchronize()
    rp, cp, ip, fp, hp = rays.data_ptr(), cnt.data_ptr(), idx.data_ptr(), flag.data_ptr(), hit.data_ptr()

    def sweep(k, full):
        outs = (cp, ip, fp, hp) if full else (cp, ip, None, None)
        if ranged:
            R.sweep_spheres_ranged_into(rp, n, ps, rq.data_ptr(), lo.data_ptr(), hi.data_ptr(), k, *outs,
                                        exclude_ptr=None if ex is None else ex.data_ptr())
        else:
            R.sweep_spheres_into(rp, n, ps, radius, k, *outs, t_min=0.0, t_max=1.0)

    def yardstick(k, full):
        outs = (cp, ip, fp, hp) if full else (cp, ip, None, None)
        if ranged:
            R.multi_hit_rays_ranged_into(rp, n, ps, lo.data_ptr(), hi.data_ptr(), k, *outs)
        else:
            R.multi_hit_rays_into(rp, n, ps, k, *outs, t_min=0.0, t_max=1.0)

    pick = np.random.default_rng(1).choice(n, min(n, SAMPLE), replace=False)
    o, d = rays_np[pick, :3], rays_np[pick, 3:]
    boxes, leaves = S.walk_counts(arr, o, d, radius[pick] if ranged else radius, 0.0, 1.0)
    boxes0, leaves0 = S.walk_counts(arr, o, d, 0.0, 0.0, 1.0)
    for k in KS:
        r = {"case": case, "queries": n, "k": k, "radius": "per-query" if ranged else radius, "iters": iters}
        for full in (True, False):
            key = "all" if full else "index"
            ms = timed(lambda: sweep(k, full), iters)
            r[f"sweep_{key}_ms"] = round(ms, 4)
            r[f"sweep_{key}_mq"] = round(n / (ms * 1e3), 1)
            if full:
                r["launch"] = ctx.last_launch
                torch.cuda.synchronize()
                r["contacts_mean"] = round(float(cnt.float().mean()), 3)
                r["contacts_max"] = int(cnt.max())
                r["queries_with_contact"] = round(float((cnt > 0).float().mean()), 4)
            ms_y = timed(lambda: yardstick(k, full), iters)
            r[f"multi_hit_{key}_ms"] = round(ms_y, 4)
            r[f"ratio_{key}"] = round(ms / ms_y, 3)       # sweep time / multi-hit time on the same rays
        r["boxes_mean"], r["leaves_mean"] = round(float(boxes.mean()), 2), round(float(leaves.mean()), 2)
        r["multi_hit_boxes_mean"], r["multi_hit_leaves_mean"] = round(float(boxes0.mean()), 2), round(float(leaves0.mean()), 2)
        print(json.dumps(r), flush=True)


def self_sweeps(ctx, ps, name, iters):
    arr = ps.bvh_arrays()
    L = arr["L"]
    n = L.shape[0]
    rng = np.random.default_rng(3)
    v = rng.normal(size=(n, 3))
    v *= (L[:, 6] / np.linalg.norm(v, axis=1))[:, None]          # a displacement of one radius per step
    rays = np.concatenate([L[:, :3], v], axis=1).astype(np.float32)
    me = np.arange(n, dtype=np.int32)
    probe(ctx, ps, arr, f"{name} self-sweep, L order", rays, L[:, 6].copy(), me, iters)
    sh = rng.permutation(n)
    probe(ctx, ps, arr, f"{name} self-sweep, shuffled", rays[sh], L[sh, 6].copy(), me[sh], iters)
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--floor", type=int, default=1000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = R.Context(0, stream=stream.cuda_stream)
    ps = R.prepare_scene(100, 100, ctx.scene("irreg"))
    self_sweeps(ctx, ps, "irreg", a.iters)
    ps.free()
    ps = R.prepare_scene(100, 100, ctx.floor(a.floor, 6.0 * a.floor))
    arr = self_sweeps(ctx, ps, f"floor {a.floor}x{a.floor}", a.iters)
    L = arr["L"]
    n = L.shape[0]
    rng = np.random.default_rng(4)
    lo, hi = L[:, :3].min(0), L[:, :3].max(0)
    o = lo + rng.random((n, 3)) * (hi - lo)
    o[:, 1] = rng.uniform(0.0, 30.0, n)
    d = rng.normal(size=(n, 3))
    d *= (20.0 / np.linalg.norm(d, axis=1))[:, None]
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    for radius in (0.0, 1.0, 30.0):
        probe(ctx, ps, arr, f"floor {a.floor}x{a.floor} random casts", rays, radius, None, a.iters)
    ps.free()
    ctx.close()


if __name__ == "__main__":
    main()
