"""Cost of the visibility matrix on one GPU against the route a caller had before it; prints one JSON line per case.

    python tools/pairs_probe.py [--iters N] [--brackets B] [--size S] [--out FILE]

For rgbbox and irreg at S x S (default 1000 x 1000): the points are the hit points of the frame's camera rays (intersect_rays over (0, 1e9),
as tests/occlusion_ref.shadow_rays takes them).  Cases: 16 and 64 lights -- tests/occlusion_ref.LIGHTS[scene] first, the rest seeded around
it -- as TARGETS over (1e-3, 1), and a fan of 64 seeded directions as DIRECTIONS over (1e-3, 1e9).

Two routes to the per-point count of visible targets, timed in the same process, alternating bracket by bracket:
  old : a torch expression builds the n * m x 6 rays, rt_occluded_rays answers a byte per pair, torch sums the bytes per point.  Timed whole,
        and in parts: the ray construction alone, the walk alone (under AUTO and with the lane kernel forced), the reduction alone.
  new : rt_visible_pairs -- mask and count, and count alone; and rt_visible_pairs_shaped with one point and one word per wave, which for 16
        targets is the shape the library's rule avoids (it packs four points into a wave there).
Each time is the median over the brackets of (HIP events around `iters` calls) / iters, after one untimed call of everything; min and max
are kept.  The two routes' counts are compared (they must be equal), and the peak of torch's device allocations over each route is
recorded next to the bytes of the inputs both share.

A last group sweeps rt_visible_pairs_shaped's words_per_wave on long rows (few points x many targets, and many points x 1024 targets):
the measurement behind pairs_auto_words_per_wave (query_device.hpp)."""
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


def bracket(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def measure(fns, iters, brackets):
    """{name: [median, min, max] ms per call}: one untimed call of each, then `brackets` rounds that take the functions in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(brackets):
        for k, fn in fns.items():
            times[k].append(bracket(fn, iters))
    return {k: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)] for k, v in times.items()}


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def case(ctx, ps, points, tg, mode, t0, t1, iters, brackets):
    n, m = points.shape[0], tg.shape[0]
    words = (m + 63) // 64
    vis = torch.empty((n, words), dtype=torch.int64, device="cuda")
    cnt_new = torch.empty(n, dtype=torch.int32, device="cuda")
    occ = torch.empty(n * m, dtype=torch.uint8, device="cuda")
    keep = {}

    def build():
        o = points[:, None, :].expand(n, m, 3)
        d = tg[None, :, :] - points[:, None, :] if mode == R.PAIRS_TARGETS else tg[None, :, :].expand(n, m, 3)
        return torch.cat([o, d], dim=2).reshape(n * m, 6)

    def walk(rays):
        R.occluded_rays_into(rays.data_ptr(), n * m, ps, occ.data_ptr(), t0, t1)

    def reduce():
        return (occ.view(n, m) == 0).sum(dim=1, dtype=torch.int32)

    def old():
        rays = build()
        walk(rays)
        keep["old"] = reduce()

    rays_kept = build()

    def walk_lane():
        ctx.set_variant(R.VARIANT_PIXEL)
        walk(rays_kept)
        ctx.set_variant(R.VARIANT_AUTO)

    def new_both():
        R.visible_pairs_into(points.data_ptr(), n, tg.data_ptr(), m, ps, mode, vis.data_ptr(), cnt_new.data_ptr(), t0, t1)

    def new_count():
        R.visible_pairs_into(points.data_ptr(), n, tg.data_ptr(), m, ps, mode, None, cnt_new.data_ptr(), t0, t1)

    def new_general():
        R.visible_pairs_into(points.data_ptr(), n, tg.data_ptr(), m, ps, mode, vis.data_ptr(), cnt_new.data_ptr(), t0, t1, words_per_wave=1)

    fns = {"old_route": old, "old_build": build, "old_walk_auto": lambda: walk(rays_kept), "old_walk_lane": walk_lane, "old_reduce": reduce,
           "new_mask_count": new_both, "new_count": new_count, "new_point_per_wave": new_general}
    r = {"points": n, "targets": m, "pairs": n * m, "mode": "targets" if mode == R.PAIRS_TARGETS else "directions", "interval": [t0, t1]}
    r["ms"] = measure(fns, iters, brackets)
    walk(rays_kept)
    r["old_walk_auto_launch"] = ctx.last_launch.split(" frames=")[0]
    new_both()
    r["new_launch"] = ctx.last_launch
    old()
    torch.cuda.synchronize()
    r["counts_equal"] = bool(torch.equal(keep["old"], cnt_new))
    r["mask_popcount_equal"] = bool(np.array_equal(
        np.unpackbits(vis.cpu().numpy().view(np.uint8).reshape(n, -1), axis=1).sum(axis=1), cnt_new.cpu().numpy()))
    r["visible_share"] = round(float(cnt_new.double().sum()) / (n * m), 4)
    keep.clear()
    del rays_kept
    r["shared_input_bytes"] = 12 * (n + m)
    r["old_peak_bytes"] = peak_of(old) + occ.numel()
    keep.clear()
    r["new_peak_bytes"] = peak_of(new_both) + vis.numel() * 8 + cnt_new.numel() * 4
    med = r["ms"]
    r["gpairs_per_s"] = {k: round(n * m / (med[k][0] * 1e6), 2) for k in ("old_route", "old_walk_auto", "old_walk_lane", "new_mask_count", "new_count", "new_point_per_wave")}
    return r


def sweep(ctx, ps, points, tg, t0, t1, shapes, iters, brackets):
    n, m = points.shape[0], tg.shape[0]
    words = (m + 63) // 64
    vis = torch.empty((n, words), dtype=torch.int64, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")

    def shaped(w):
        return lambda: R.visible_pairs_into(points.data_ptr(), n, tg.data_ptr(), m, ps, R.PAIRS_TARGETS, vis.data_ptr(), cnt.data_ptr(), t0, t1,
                                            words_per_wave=w)

    fns = {("auto" if w == 0 else str(w)): shaped(w) for w in shapes if w <= words}
    ref = None
    same = True
    for fn in fns.values():
        fn()
        torch.cuda.synchronize()
        got = (vis.clone(), cnt.clone())
        same = same and (ref is None or (torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])))
        ref = ref or got
    return {"points": n, "targets": m, "words": words, "interval": [t0, t1], "all_shapes_equal": same, "ms_by_words_per_wave": measure(fns, iters, brackets)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    sink = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit({"device": ctx.device_info(), "size": a.size, "iters": a.iters, "brackets": a.brackets})
    h = w = a.size
    n = h * w
    for name in ("rgbbox", "irreg"):
        rng = np.random.default_rng(11)
        scene = ctx.scene(name)
        ps = R.prepare_scene(h, w, scene)
        cam = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        R.camera_rays_into(cam.data_ptr(), h, w, ps)
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        hit = torch.empty((n, 7), dtype=torch.float32, device="cuda")
        R.intersect_rays_into(cam.data_ptr(), n, ps, idx.data_ptr(), hit.data_ptr(), 0.0, 1e9)
        torch.cuda.synchronize()
        points = hit[idx >= 0, 1:4].contiguous()
        del cam, hit, idx
        light = np.asarray(LIGHTS[name], dtype=np.float64)
        spread = 0.25 * float(np.abs(light).max())
        lights = np.concatenate([light[None, :], light[None, :] + rng.normal(size=(63, 3)) * spread]).astype(np.float32)
        fan = rng.normal(size=(64, 3)).astype(np.float32)
        for label, tg, mode, t1 in (("lights16", lights[:16], R.PAIRS_TARGETS, 1.0), ("lights64", lights, R.PAIRS_TARGETS, 1.0),
                                    ("fan64", fan, R.PAIRS_DIRECTIONS, 1e9)):
            rec = case(ctx, ps, points, torch.from_numpy(tg).cuda(), mode, 1e-3, t1, a.iters, a.brackets)
            emit({"scene": name, "case": label, **rec})
        # launch shapes on long rows: 256 points x 16384 targets (the points alone do not fill the machine), 10^5 points x 1024 targets
        far = (light[None, :] + rng.normal(size=(16384, 3)) * spread).astype(np.float32)
        pick = torch.from_numpy(rng.choice(points.shape[0], 100000, replace=False)).cuda()
        some = points[pick].contiguous()
        emit({"scene": name, "case": "sweep few points", **sweep(ctx, ps, some[:256].contiguous(), torch.from_numpy(far).cuda(), 1e-3, 1.0,
                                                                   (0, 1, 2, 4, 8, 16, 64, 256), a.iters, a.brackets)})
        emit({"scene": name, "case": "sweep long rows", **sweep(ctx, ps, some, torch.from_numpy(far[:1024]).cuda(), 1e-3, 1.0,
                                                                 (0, 1, 2, 4, 8, 16), a.iters, a.brackets)})
        ps.free()
        scene.free()
    if sink:
        sink.close()
    ctx.close()


if __name__ == "__main__":
    main()
