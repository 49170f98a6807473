"""Throughput of the ray-path query on one GPU and the sweep behind its launch rule; prints one JSON line (ms per call).

    python tools/paths_probe.py [--iters N] [--size S] [--repeats M] [--ks 1,8,50] [--shapes 64,128,256,512,1024,0]

For rgbbox and irreg at S x S (default 1000 x 1000), two ray sets -- the frame's camera rays and S * S seeded random rays (origins in the
scene's box, directions uniform on the sphere) -- through rt_trace_paths at max_depth 50 and k in {1, 8, 50}, once with every output and
once with count and end only, at rays_per_wave 64, 128, 256, 512, 1024 and auto, ALTERNATED in one process; the whole sweep is repeated
(default three times) so that the spread of a figure is known: each entry is [median, min, max] ms over the repeats.  Next to them, on the
same rays in the same process, rt_trace_rays under RT_VARIANT_PIXEL -- the same walk, one ray per lane, no path stores: what paths add --
and under AUTO (the pooled family) for context; and the mean and largest vertex count.  Times are HIP events on a torch stream the context
enqueues on."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracers_amd as R  # noqa: E402

KS = (1, 8, 50)
SHAPES = (64, 128, 256, 512, 1024, 0)
MAX_DEPTH = 50


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


def summary(ms):
    return [round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)]


def probe_set(ctx, ps, rays, iters, repeats, ks=KS, shapes=SHAPES):
    n = rays.shape[0]
    kmax = max(ks)
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    end = torch.empty(n, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n * kmax, dtype=torch.int32, device="cuda")
    hit = torch.empty(n * kmax * 7, dtype=torch.float32, device="cuda")
    light = torch.empty(n * 3, dtype=torch.float32, device="cuda")
    last = torch.empty(n * 6, dtype=torch.float32, device="cuda")
    col = torch.empty(n * 3, dtype=torch.float32, device="cuda")
    times = {}

    def put(key, ms):
        times.setdefault(key, []).append(ms)

    def paths(k, every, shape):
        if every:
            R.trace_paths_into(rays.data_ptr(), n, ps, k, cnt.data_ptr(), end.data_ptr(), idx.data_ptr(), hit.data_ptr(), light.data_ptr(),
                               last.data_ptr(), col.data_ptr(), max_depth=MAX_DEPTH, rays_per_wave=shape)
        else:
            R.trace_paths_into(rays.data_ptr(), n, ps, k, cnt.data_ptr(), end.data_ptr(), max_depth=MAX_DEPTH, rays_per_wave=shape)

    launches = {}
    for _ in range(repeats):
        ctx.set_variant(R.VARIANT_PIXEL)
        put("trace_rays_pixel", timed(lambda: R.trace_rays_into(rays.data_ptr(), n, ps, col.data_ptr(), None, MAX_DEPTH), iters))
        ctx.set_variant(R.VARIANT_AUTO)
        put("trace_rays_auto", timed(lambda: R.trace_rays_into(rays.data_ptr(), n, ps, col.data_ptr(), None, MAX_DEPTH), iters))
        launches["trace_rays_auto"] = ctx.last_launch
        for k in ks:
            for every in (True, False):
                for shape in shapes:
                    key = f"k{k}_{'all' if every else 'count_end'}_r{shape or 'auto'}"
                    put(key, timed(lambda: paths(k, every, shape), iters))
                    launches[key] = ctx.last_launch
    torch.cuda.synchronize()
    r = {"rays": n, "ms_median_min_max": {key: summary(ms) for key, ms in times.items()}}
    r["auto_launch"] = launches.get(f"k{ks[0]}_all_rauto")
    r["trace_rays_auto_launch"] = launches["trace_rays_auto"]
    r["count_mean"] = round(float(cnt.float().mean()), 3)
    r["count_max"] = int(cnt.max())
    r["ends"] = [int(x) for x in torch.bincount(end.long(), minlength=3)]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ks", default=",".join(map(str, KS)), help="the k values of the sweep")
    ap.add_argument("--shapes", default=",".join(map(str, SHAPES)), help="the rays_per_wave values of the sweep (0: auto)")
    a = ap.parse_args()
    ks, shapes = tuple(int(x) for x in a.ks.split(",")), tuple(int(x) for x in a.shapes.split(","))
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = R.Context(0, stream=stream.cuda_stream)
    h = w = a.size
    n = h * w
    out = {"size": f"{w}x{h}", "iters": a.iters, "repeats": a.repeats, "max_depth": MAX_DEPTH, "num_cu": ctx.device_info()["num_cu"]}
    rng = np.random.default_rng(5)
    for name in ("rgbbox", "irreg"):
        ps = R.prepare_scene(h, w, ctx.scene(name))
        cam = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        R.camera_rays_into(cam.data_ptr(), h, w, ps)
        torch.cuda.synchronize()
        r = {"camera": probe_set(ctx, ps, cam, a.iters, a.repeats, ks, shapes)}
        L = ps.bvh_arrays()["L"]
        lo, hi = L[:, :3].min(0), L[:, :3].max(0)
        o = lo + rng.random((n, 3)) * (hi - lo)
        d = rng.normal(size=(n, 3))
        rnd = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).cuda()
        r["random"] = probe_set(ctx, ps, rnd, a.iters, a.repeats, ks, shapes)
        out[name] = r
        ps.free()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
