"""Cost and use of per-ray intervals on one GPU; prints one JSON line (ms per call and Mray/s = rays answered / us).

    python tools/interval_probe.py [--iters N] [--size S]

For rgbbox and irreg at S x S (default 1000 x 1000):
  overhead   occlusion_probe's two sets -- the shadow rays d = light - p over (1e-3, 1) from every camera-ray hit, and S * S seeded random rays
             over (0.1, 1e9) -- through rt_occluded_rays and through rt_occluded_rays_ranged with constant arrays of the same interval, each
             under the pooled loop (VARIANT_POOLED), the lane kernel (VARIANT_PIXEL) and AUTO; and rt_intersect_rays against
             rt_intersect_rays_ranged on the same rays and interval
  use        the shadow rays normalised, t_max_i = |light - p_i| - 1e-3, through the ranged entry (next to the unnormalised set through the
             scalar entry, above), and the random set with per-ray t_max drawn log-uniformly in [1, 1e3] over t_min = 0.1
Times are HIP events on a torch stream the context enqueues on."""
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

FAMILIES = (("pooled", R.VARIANT_POOLED), ("lane", R.VARIANT_PIXEL), ("auto", R.VARIANT_AUTO))


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


def occ_ranged(ctx, ps, rays, lo, hi, iters):
    """the ranged occlusion entry under each family: {family_ms, family_mrays, family_launch}, and the answers"""
    n = rays.shape[0]
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    r, res = {}, {}
    for key, variant in FAMILIES:
        ctx.set_variant(variant)
        r[key + "_ms"] = round(timed(lambda: R.occluded_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), occ.data_ptr()), iters), 4)
        r[key + "_mrays"] = round(n / (r[key + "_ms"] * 1e3), 1)
        r[key + "_launch"] = ctx.last_launch.split(" frames=")[0]
        res[key] = occ.clone()
    ctx.set_variant(R.VARIANT_AUTO)
    r["pooled_equals_lane"] = bool(torch.equal(res["pooled"], res["lane"]))
    r["occluded_share"] = round(float(res["lane"].float().mean()), 4)
    return r, res["lane"]


def occ_scalar(ctx, ps, rays, t0, t1, iters):
    n = rays.shape[0]
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    r, res = {}, {}
    for key, variant in FAMILIES:
        ctx.set_variant(variant)
        r[key + "_ms"] = round(timed(lambda: R.occluded_rays_into(rays.data_ptr(), n, ps, occ.data_ptr(), t0, t1), iters), 4)
        r[key + "_mrays"] = round(n / (r[key + "_ms"] * 1e3), 1)
        r[key + "_launch"] = ctx.last_launch.split(" frames=")[0]
        res[key] = occ.clone()
    ctx.set_variant(R.VARIANT_AUTO)
    return r, res["lane"]


def overhead_set(ctx, ps, rays, t0, t1, iters):
    n = rays.shape[0]
    lo = torch.full((n,), t0, dtype=torch.float32, device="cuda")
    hi = torch.full((n,), t1, dtype=torch.float32, device="cuda")
    scalar, a = occ_scalar(ctx, ps, rays, t0, t1, iters)
    ranged, b = occ_ranged(ctx, ps, rays, lo, hi, iters)
    out = {"rays": n, "interval": [t0, t1], "scalar": scalar, "ranged": ranged, "same_answers": bool(torch.equal(a, b))}
    for key, _ in FAMILIES:
        out[key + "_ranged_over_scalar"] = round(ranged[key + "_ms"] / scalar[key + "_ms"], 3)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    hit = torch.empty((n, 7), dtype=torch.float32, device="cuda")
    i_s = timed(lambda: R.intersect_rays_into(rays.data_ptr(), n, ps, idx.data_ptr(), hit.data_ptr(), t0, t1), iters)
    want = idx.clone(), hit.clone()
    i_r = timed(lambda: R.intersect_rays_ranged_into(rays.data_ptr(), n, ps, lo.data_ptr(), hi.data_ptr(), idx.data_ptr(), hit.data_ptr()), iters)
    torch.cuda.synchronize()
    out["intersect"] = {"scalar_ms": round(i_s, 4), "ranged_ms": round(i_r, 4), "ranged_over_scalar": round(i_r / i_s, 3),
                        "same_answers": bool(torch.equal(idx, want[0]) and torch.equal(hit.view(torch.int32), want[1].view(torch.int32)))}
    return out


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
        v = light[None, :] - p
        shadow = torch.cat([p, v], dim=1).contiguous()
        L = ps.bvh_arrays()["L"]
        lo, hi = L[:, :3].min(0), L[:, :3].max(0)
        o = lo + rng.random((n, 3)) * (hi - lo)
        d = rng.normal(size=(n, 3))
        rnd = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).cuda()
        r = {"light": list(LIGHTS[name]),
             "overhead_shadow": overhead_set(ctx, ps, shadow, 1e-3, 1.0, a.iters),
             "overhead_random": overhead_set(ctx, ps, rnd, 0.1, 1e9, a.iters)}
        # normalised shadow rays, each over (1e-3, |light - p| - 1e-3)
        dist = torch.sqrt((v * v).sum(dim=1))
        nshadow = torch.cat([p, v / dist[:, None]], dim=1).contiguous()
        t_lo = torch.full((nshadow.shape[0],), 1e-3, dtype=torch.float32, device="cuda")
        t_hi = (dist - 1e-3).contiguous()
        rn, a_n = occ_ranged(ctx, ps, nshadow, t_lo, t_hi, a.iters)
        _, a_u = occ_scalar(ctx, ps, shadow, 1e-3, 1.0, 1)
        rn["agrees_with_unnormalised"] = round(float((a_n == a_u).float().mean()), 5)
        r["normalised_shadow_ranged"] = rn
        # the random set with t_max log-uniform in [1, 1e3]
        t_lo = torch.full((n,), 0.1, dtype=torch.float32, device="cuda")
        t_hi = torch.from_numpy((10.0 ** rng.uniform(0.0, 3.0, n)).astype(np.float32)).cuda()
        r["random_logt_ranged"], _ = occ_ranged(ctx, ps, rnd, t_lo, t_hi, a.iters)
        out[name] = r
        ps.free()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
