"""Throughput of the caller-ray entries on one GPU; prints one JSON line (Gray/s = rays traced incl. bounces / ns).

    python tools/ray_query_probe.py [--iters N]

For rgbbox and irreg at 1000 x 1000: rt_render of the frame, rt_trace_rays on its camera rays through the pooled family
(AUTO) and the pixel family, and rt_trace_rays on a seeded random-ray set of the same size.  Times are HIP events on a torch
stream the context enqueues on; ray counts come from the instrumented frame (rt_render_stats)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=1000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = R.Context(0, stream=stream.cuda_stream)
    h = w = a.size
    n = h * w
    out = {"size": f"{w}x{h}", "iters": a.iters}
    rng = np.random.default_rng(5)
    for name in ("rgbbox", "irreg"):
        ps = R.prepare_scene(h, w, ctx.scene(name))
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        R.camera_rays_into(rays.data_ptr(), h, w, ps)
        col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        px = torch.empty(n, dtype=torch.int32, device="cuda")
        img = torch.empty(n, dtype=torch.int32, device="cuda")
        nrays = ps.stats()["rays"]
        r = {"rays_per_frame": nrays}
        ctx.set_variant(R.VARIANT_AUTO)
        r["render_ms"] = timed(lambda: R.render_into(img.data_ptr(), h, w, ps), a.iters)
        r["render_launch"] = ctx.last_launch
        r["trace_pooled_ms"] = timed(lambda: R.trace_rays_into(rays.data_ptr(), n, ps, pixel_ptr=px.data_ptr()), a.iters)
        r["trace_pooled_launch"] = ctx.last_launch
        torch.cuda.synchronize()
        r["trace_equals_render"] = bool(torch.equal(px, img))
        r["trace_pooled_colour_ms"] = timed(lambda: R.trace_rays_into(rays.data_ptr(), n, ps, col.data_ptr(), px.data_ptr()), a.iters)
        ctx.set_variant(R.VARIANT_PIXEL)
        r["trace_pixel_ms"] = timed(lambda: R.trace_rays_into(rays.data_ptr(), n, ps, pixel_ptr=px.data_ptr()), a.iters)
        ctx.set_variant(R.VARIANT_AUTO)
        # seeded random rays: origins in the scene's box, directions uniform on the sphere (bounce counts differ from the frame's)
        L = ps.bvh_arrays()["L"]
        lo, hi = L[:, :3].min(0), L[:, :3].max(0)
        o = lo + rng.random((n, 3)) * (hi - lo)
        d = rng.normal(size=(n, 3))
        rnd = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).cuda()
        r["random_pooled_ms"] = timed(lambda: R.trace_rays_into(rnd.data_ptr(), n, ps, pixel_ptr=px.data_ptr()), a.iters)
        ctx.set_variant(R.VARIANT_PIXEL)
        r["random_pixel_ms"] = timed(lambda: R.trace_rays_into(rnd.data_ptr(), n, ps, pixel_ptr=px.data_ptr()), a.iters)
        ctx.set_variant(R.VARIANT_AUTO)
        for k in ("render", "trace_pooled", "trace_pixel"):
            r[k + "_grays"] = round(nrays / (r[k + "_ms"] * 1e6), 3)
        r["random_primary_grays_pooled"] = round(n / (r["random_pooled_ms"] * 1e6), 3)
        r["random_primary_grays_pixel"] = round(n / (r["random_pixel_ms"] * 1e6), 3)
        out[name] = r
        ps.free()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
