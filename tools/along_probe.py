"""Cost of the along-ray queries on one GPU; prints one JSON line per case.

    python tools/along_probe.py [--iters N] [--brackets B] [--floor N]

tools/sweep_probe.py's inputs: N * N random casts on the floor of N x N spheres (default 1000: 10^6; origins over it, displacements of 20
units) over (0, 1) at radius 0, 1 and 30 through the scalar form; the self-sweep of the floor and of irreg (query i = centre and radius of
L[i], a displacement of one radius, exclude = i) through the per-query form, in L order.
Per case, in the same run on the same queries:
  yardstick : rt_sweep_spheres[_ranged] with k = 1, count and index only -- the same boxes, the same rule, plus the list insertion
  count     : rt_spheres_along_rays_count -- the count kernel and the scan's three launches
  fill      : rt_spheres_along_rays_fill into arrays of offsets[n] entries, all four outputs; and with the index alone
Each is warmed up once, then timed in B brackets of N calls between HIP events on the torch stream the context enqueues on, the three
alternating bracket by bracket; reported: the median bracket's ms per call and the spread (min, max).  Also entries per row (mean, max,
share of rows above 32) and the bytes the fill writes."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracers_amd as R  # noqa: E402


def bracket(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def spread(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def probe(ctx, ps, case, rays_np, radius, exclude_np, iters, brackets):
    """radius: a scalar (the scalar forms) or an [n] array (the per-query forms, over (0, 1) for every query)"""
    n = rays_np.shape[0]
    ranged = np.ndim(radius) > 0
    rays = torch.from_numpy(rays_np).cuda()
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    one = torch.empty(n, dtype=torch.int32, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    kw = dict(t_min=0.0, t_max=1.0)
    if ranged:
        rq = torch.from_numpy(np.ascontiguousarray(radius, np.float32)).cuda()
        lo = torch.zeros(n, dtype=torch.float32, device="cuda")
        hi = torch.ones(n, dtype=torch.float32, device="cuda")
        ex = torch.from_numpy(np.ascontiguousarray(exclude_np, np.int32)).cuda()
        kw = dict(radius_ptr=rq.data_ptr(), t_min_ptr=lo.data_ptr(), t_max_ptr=hi.data_ptr(), exclude_ptr=ex.data_ptr())
    else:
        kw["radius"] = radius
    torch.cuda.synchronize()
    rp = rays.data_ptr()

    def yardstick():
        if ranged:
            R.sweep_spheres_ranged_into(rp, n, ps, rq.data_ptr(), lo.data_ptr(), hi.data_ptr(), 1, cnt.data_ptr(), one.data_ptr(),
                                        exclude_ptr=ex.data_ptr())
        else:
            R.sweep_spheres_into(rp, n, ps, radius, 1, cnt.data_ptr(), one.data_ptr(), t_min=0.0, t_max=1.0)

    def count():
        R.spheres_along_rays_count_into(rp, n, ps, off.data_ptr(), **kw)

    count()
    launch = ctx.last_launch
    torch.cuda.synchronize()
    rows = (off[1:] - off[:-1]).cpu().numpy()
    total = int(off[n].item())
    idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    roots = torch.empty(2 * max(total, 1), dtype=torch.float32, device="cuda")
    start = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    qry = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")

    def fill():
        R.spheres_along_rays_fill_into(rp, n, ps, off.data_ptr(), total, idx.data_ptr(), roots.data_ptr(), start.data_ptr(), qry.data_ptr(), **kw)

    def fill_index():
        R.spheres_along_rays_fill_into(rp, n, ps, off.data_ptr(), total, idx.data_ptr(), None, None, None, **kw)

    fns = {"yardstick": yardstick, "count": count, "fill": fill, "fill_index": fill_index}
    for fn in fns.values():                      # warm-up: every kernel once
        fn()
    torch.cuda.synchronize()
    yardstick()
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), rows), "the yardstick's count is not the row length"
    ms = {k: [] for k in fns}
    for _ in range(brackets):                    # alternating, so that a drift of the machine meets all of them
        for k, fn in fns.items():
            ms[k].append(bracket(fn, iters))
    r = {"case": case, "queries": n, "radius": "per-query" if ranged else radius, "iters": iters, "brackets": brackets, "launch": launch,
         "entries": total, "entries_per_row_mean": round(float(rows.mean()), 3), "entries_per_row_max": int(rows.max()),
         "rows_above_32": round(float((rows > 32).mean()), 4), "fill_bytes_written": 17 * total}
    for k in fns:
        r[k] = spread(ms[k])
    r["count_over_yardstick"] = round(r["count"]["ms"] / r["yardstick"]["ms"], 3)
    r["count_minus_yardstick_us"] = round(1e3 * (r["count"]["ms"] - r["yardstick"]["ms"]), 1)
    r["fill_over_count"] = round(r["fill"]["ms"] / r["count"]["ms"], 3)
    r["fill_write_GBps"] = round(17 * total / (r["fill"]["ms"] * 1e6), 1)
    print(json.dumps(r), flush=True)


def self_sweep(ctx, ps, name, iters, brackets):
    arr = ps.bvh_arrays()
    L = arr["L"]
    n = L.shape[0]
    rng = np.random.default_rng(3)
    v = rng.normal(size=(n, 3))
    v *= (L[:, 6] / np.linalg.norm(v, axis=1))[:, None]          # a displacement of one radius per step
    rays = np.concatenate([L[:, :3], v], axis=1).astype(np.float32)
    probe(ctx, ps, f"{name} self-sweep, L order", rays, L[:, 6].copy(), np.arange(n, dtype=np.int32), iters, brackets)
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--floor", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("along_probe: no GPU; nothing is measured without one")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = R.Context(0, stream=stream.cuda_stream)
    ps = R.prepare_scene(100, 100, ctx.scene("irreg"))
    self_sweep(ctx, ps, "irreg", 20 * a.iters, a.brackets)          # (a small scene: more calls per bracket)
    ps.free()
    ps = R.prepare_scene(100, 100, ctx.floor(a.floor, 6.0 * a.floor))
    arr = self_sweep(ctx, ps, f"floor {a.floor}x{a.floor}", a.iters, a.brackets)
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
        probe(ctx, ps, f"floor {a.floor}x{a.floor} random casts", rays, radius, None, a.iters, a.brackets)
    ps.free()
    ctx.close()


if __name__ == "__main__":
    main()
