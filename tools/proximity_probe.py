"""Throughput of the proximity query (rt_nearest_spheres) on one GPU; prints one JSON line per case: ms per call and Mq/s = queries
answered / us, HIP events on a torch stream the context enqueues on, after one untimed warm-up call.

    python tools/proximity_probe.py [--iters N]

Cases:
  * self-contacts (points = the spheres' centres, per-point max_dist = their radii, k = 8, count mode) of irreg and of the 10^6-sphere floor,
    with the points in L order (Morton order, neighbouring lanes walk neighbouring subtrees) and shuffled (lane divergence);
  * k-nearest, k = 1 and k = 8, of 10^6 random points in the floor's box: the pruned mode at max_dist = 1e9 and at 30, and the count mode
    at 30, with the points in random order and sorted by the L index (Morton order) of their nearest sphere;
  * count mode against pruned mode at max_dist = 1e9 on 4096 of those points (count mode then counts every sphere for every point: the walk
    can prune nothing)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracers_amd as R  # noqa: E402


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


def case(ctx, ps, pts, k, max_dist, count, iters, **info):
    n = pts.shape[0]
    cnt = torch.empty(n, dtype=torch.int32, device="cuda") if count else None
    idx = torch.empty(n * k, dtype=torch.int32, device="cuda")
    gap = torch.empty(n * k, dtype=torch.float32, device="cuda")
    cp = cnt.data_ptr() if count else None
    if torch.is_tensor(max_dist):
        fn = lambda: R.nearest_spheres_ranged_into(pts.data_ptr(), n, ps, max_dist.data_ptr(), k, cp, idx.data_ptr(), gap.data_ptr())  # noqa: E731
    else:
        fn = lambda: R.nearest_spheres_into(pts.data_ptr(), n, ps, k, cp, idx.data_ptr(), gap.data_ptr(), max_dist)  # noqa: E731
    ms = timed(fn, iters)
    r = dict(info, queries=n, k=k, max_dist="per-point" if torch.is_tensor(max_dist) else max_dist, ms=round(ms, 4),
             mq_per_s=round(n / (ms * 1e3), 2), launch=ctx.last_launch)
    if count:
        r["count_mean"] = round(float(cnt.float().mean()), 3)
    filled = idx.view(n, k)[:, k - 1] >= 0
    r["kth_filled"] = int(filled.sum())
    r["gap_k_mean"] = round(float(gap.view(n, k)[:, k - 1][filled].mean()), 4) if bool(filled.any()) else None
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for name in ("irreg", "big"):
        ps = R.prepare_scene(64, 64, ctx.scene(name))
        L = torch.from_numpy(ps.bvh_arrays()["L"]).cuda()
        c, r = L[:, :3].contiguous(), L[:, 6].contiguous()
        perm = torch.from_numpy(rng.permutation(L.shape[0])).cuda()
        for order, cc, rr in (("morton", c, r), ("shuffled", c[perm].contiguous(), r[perm].contiguous())):
            case(ctx, ps, cc, 8, rr, True, a.iters, case="self-contacts", scene=name, spheres=int(L.shape[0]), height=ps.height, order=order)
        if name == "big":
            lo, hi = c.min(0).values, c.max(0).values
            pts = (lo + torch.rand((1000000, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(7)) * (hi - lo)).contiguous()
            pts[:, 1] = torch.rand(1000000, device="cuda") * 20.0 - 10.0
            # Morton-sorted queries: the points ordered by the L index of their nearest sphere (k = 1 of the pruned query)
            i1 = torch.empty(1000000, dtype=torch.int32, device="cuda")
            R.nearest_spheres_into(pts.data_ptr(), 1000000, ps, 1, None, i1.data_ptr(), None, 1e9)
            torch.cuda.synchronize()
            srt = pts[torch.argsort(i1)].contiguous()
            for k in (1, 8):
                for order, q in (("random", pts), ("sorted", srt)):
                    case(ctx, ps, q, k, 1e9, False, a.iters, case="k-nearest", scene=name, order=order, mode="pruned")
                    case(ctx, ps, q, k, 30.0, False, a.iters, case="k-nearest", scene=name, order=order, mode="pruned")
                    case(ctx, ps, q, k, 30.0, True, a.iters, case="k-nearest", scene=name, order=order, mode="count")
            # count mode at max_dist = 1e9 counts every sphere for every point: a smaller batch
            q = pts[:4096].contiguous()
            case(ctx, ps, q, 8, 1e9, True, 2, case="k-nearest", scene=name, order="random", mode="count")
            case(ctx, ps, q, 8, 1e9, False, 2, case="k-nearest", scene=name, order="random", mode="pruned")
        ps.free()
    ctx.close()


if __name__ == "__main__":
    main()
