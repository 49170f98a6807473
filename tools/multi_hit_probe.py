"""Throughput of the multi-hit query on one GPU; prints one JSON line (ms per call and Mray/s = rays answered / us).

    python tools/multi_hit_probe.py [--iters N] [--size S]

For rgbbox and irreg at S x S (default 1000 x 1000), occlusion_probe's two ray sets: the shadow rays of the frame's camera rays -- from
every hit of intersect_rays(0, 1e9) toward a fixed point light per scene (tests/occlusion_ref.py: LIGHTS), d = light - p over (1e-3, 1)
-- and S * S seeded random rays over (0.1, 1e9).  Each set through rt_multi_hit_rays at k in {1, 4, 16, 32}, once with every output
(count, index, root, hit7) and once with count and index only, next to rt_intersect_rays (index only) and rt_occluded_rays (the lane
kernel) on the same rays and interval; with the mean and largest crossing count.  Times are HIP events on a torch stream the context
enqueues on."""
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

KS = (1, 4, 16, 32)


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
    kmax = max(KS)
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    idx = torch.empty(n * kmax, dtype=torch.int32, device="cuda")
    root = torch.empty(n * kmax, dtype=torch.uint8, device="cuda")
    hit = torch.empty(n * kmax * 7, dtype=torch.float32, device="cuda")
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    r = {"rays": n, "interval": [t0, t1]}

    def put(key, ms):
        r[key + "_ms"] = round(ms, 4)
        r[key + "_mrays"] = round(n / (ms * 1e3), 1)

    ctx.set_variant(R.VARIANT_PIXEL)
    put("intersect", timed(lambda: R.intersect_rays_into(rays.data_ptr(), n, ps, idx.data_ptr(), None, t0, t1), iters))
    put("occluded", timed(lambda: R.occluded_rays_into(rays.data_ptr(), n, ps, occ.data_ptr(), t0, t1), iters))
    ctx.set_variant(R.VARIANT_AUTO)
    for k in KS:
        put(f"k{k}_all", timed(lambda: R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, cnt.data_ptr(), idx.data_ptr(), root.data_ptr(),
                                                             hit.data_ptr(), t0, t1), iters))
        put(f"k{k}_index", timed(lambda: R.multi_hit_rays_into(rays.data_ptr(), n, ps, k, cnt.data_ptr(), idx.data_ptr(), None, None, t0, t1),
                                 iters))
        r[f"k{k}_launch"] = ctx.last_launch
    torch.cuda.synchronize()
    c = cnt.float()
    r["crossings_mean"] = round(float(c.mean()), 3)
    r["crossings_max"] = int(cnt.max())
    r["count_matches_occluded"] = bool(torch.equal((cnt > 0).to(torch.uint8), occ))
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
        # seeded random rays: origins in the scene's box, directions uniform on the sphere (occlusion_probe's set)
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
