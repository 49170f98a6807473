"""Throughput of the occlusion query on one GPU; prints one JSON line (Mray/s = rays answered / us).

    python tools/occlusion_probe.py [--iters N] [--size S]

For rgbbox and irreg at S x S (default 1000 x 1000), two ray sets: the shadow rays of the frame's camera rays -- from every hit of
intersect_rays(0, 1e9) toward a fixed point light per scene (tests/occlusion_ref.py: LIGHTS), d = light - p over (1e-3, 1) -- and a
seeded random-ray set of S * S rays over (0.1, 1e9).  Each set through rt_occluded_rays in the pooled family (VARIANT_POOLED), through
the lane kernel (VARIANT_PIXEL), under AUTO, and through rt_intersect_rays on the same rays and interval (the only way to the answer
before).  Times are HIP events on a torch stream the context enqueues on."""
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
from occlusion_ref import LIGHTS  # noqa: E402


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


def probe_set(ctx, ps, rays, t0, t1, iters):
    n = rays.shape[0]
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    r = {"rays": n, "interval": [t0, t1]}
    results = {}
    for key, variant in (("pooled", R.VARIANT_POOLED), ("lane", R.VARIANT_PIXEL), ("auto", R.VARIANT_AUTO)):
        ctx.set_variant(variant)
        r[key + "_ms"] = timed(lambda: R.occluded_rays_into(rays.data_ptr(), n, ps, occ.data_ptr(), t0, t1), iters)
        r[key + "_launch"] = ctx.last_launch.split(" frames=")[0]
        results[key] = occ.clone()
    ctx.set_variant(R.VARIANT_AUTO)
    r["intersect_ms"] = timed(lambda: R.intersect_rays_into(rays.data_ptr(), n, ps, idx.data_ptr(), None, t0, t1), iters)
    torch.cuda.synchronize()
    r["occluded_share"] = round(float(results["pooled"].float().mean()), 4)
    r["pooled_equals_lane"] = bool(torch.equal(results["pooled"], results["lane"]))
    for key in ("pooled", "lane", "auto", "intersect"):
        r[key + "_mrays"] = round(n / (r[key + "_ms"] * 1e3), 1)
    return r


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
        cam = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        R.camera_rays_into(cam.data_ptr(), h, w, ps)
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        hit = torch.empty((n, 7), dtype=torch.float32, device="cuda")
        R.intersect_rays_into(cam.data_ptr(), n, ps, idx.data_ptr(), hit.data_ptr(), 0.0, 1e9)
        torch.cuda.synchronize()
        p = hit[idx >= 0, 1:4]
        light = torch.tensor(LIGHTS[name], dtype=torch.float32, device="cuda")
        shadow = torch.cat([p, light[None, :] - p], dim=1).contiguous()
        r = {"light": list(LIGHTS[name]), "shadow": probe_set(ctx, ps, shadow, 1e-3, 1.0, a.iters)}
        # seeded random rays: origins in the scene's box, directions uniform on the sphere
        L = ps.bvh_arrays()["L"]
        lo, hi = L[:, :3].min(0), L[:, :3].max(0)
        o = lo + rng.random((n, 3)) * (hi - lo)
        d = rng.normal(size=(n, 3))
        rnd = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).cuda()
        r["random"] = probe_set(ctx, ps, rnd, 0.1, 1e9, a.iters)
        out[name] = r
        ps.free()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
