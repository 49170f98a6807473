"""Cost of the plane-set queries (rt_spheres_in_planes_count / _fill) on one GPU against the box queries (rt_spheres_in_boxes_count / _fill),
re-measured in the same run.  Prints one JSON line per measurement: ms per call from HIP events on a torch stream the context enqueues on,
after one untimed warm-up call (tools/boxes_probe.py's protocol).

    python tools/planes_probe.py [--iters N] [--rounds R] [--scenes irreg,big]

Cases, for irreg and for the 10^6-sphere floor:
  * random cubes sized for about 100 spheres per row (boxes_probe's), margin 0, asked as boxes and as their six planes: the same regions, so
    the difference is the price of six plane tests per node and leaf against one box test -- the plane rows are supersets (asserted) and
    slightly longer (spheres off an edge or a corner);
  * the tile frusta of the scene's camera at 1000 x 1000 with 16 x 16 tiles (tile_frusta: four planes per tile), margin 0, against what a
    caller without plane queries has: spheres_in_boxes on each frustum's bounding box truncated at the scene's extent, to be filtered on the
    host afterwards.  Rows per query of both are printed: the figure that says what the feature buys.
Per case the bracket [boxes count + scan, planes count + scan, boxes fill, planes fill] is measured `rounds` times in turn; the spread of a
measurement over the rounds is what a difference between two of them has to exceed.  Both fill passes write index and gap."""
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


def bracket(ctx, ps, boxes, planes, iters, rounds, **info):
    """boxes (n, 6) and planes (n, K, 4), float32 device tensors, margin 0"""
    n, k = int(planes.shape[0]), int(planes.shape[1])
    off_b = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    off_p = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    bcount = lambda: R.spheres_in_boxes_count_into(boxes.data_ptr(), n, ps, off_b.data_ptr(), 0.0)  # noqa: E731
    pcount = lambda: R.spheres_in_planes_count_into(planes.data_ptr(), n, k, ps, off_p.data_ptr(), 0.0)  # noqa: E731
    bcount()
    pcount()
    tb, tp = int(off_b[n].item()), int(off_p[n].item())
    cap = max(tb, tp, 1)
    idx_b, idx_p = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    gap_b, gap_p = (torch.empty(cap, dtype=torch.float32, device="cuda") for _ in range(2))
    bfill = lambda: R.spheres_in_boxes_fill_into(boxes.data_ptr(), n, ps, off_b.data_ptr(), tb, idx_b.data_ptr(), gap_b.data_ptr(), None, 0.0)  # noqa: E731
    pfill = lambda: R.spheres_in_planes_fill_into(planes.data_ptr(), n, k, ps, off_p.data_ptr(), tp, idx_p.data_ptr(), gap_p.data_ptr(), None, 0.0)  # noqa: E731
    bfill()
    pfill()
    torch.cuda.synchronize()
    if info.get("superset") == "planes":
        assert bool((torch.diff(off_p) >= torch.diff(off_b)).all()), "a box selected more than its six planes"
    steps = [("boxes count + scan (yardstick)", bcount, tb), ("planes count + scan", pcount, tp), ("boxes fill (yardstick)", bfill, tb),
             ("planes fill (index, gap)", pfill, tp)]
    for rnd in range(rounds):
        for what, fn, entries in steps:
            ms = timed(fn, iters)
            print(json.dumps(dict(info, what=what, round=rnd, queries=n, nplanes=k, entries=entries, per_row=round(entries / n, 3),
                                  ms=round(ms, 4), mq_per_s=round(n / (ms * 1e3), 2), launch=ctx.last_launch)), flush=True)


def box_planes(boxes):
    """(n, 6) boxes as (n, 6, 4) planes: (1,0,0,-lo.x), (0,1,0,-lo.y), (0,0,1,-lo.z), (-1,0,0,hi.x), (0,-1,0,hi.y), (0,0,-1,hi.z)"""
    p = torch.zeros((boxes.shape[0], 6, 4), dtype=torch.float32, device=boxes.device)
    for k in range(3):
        p[:, k, k], p[:, k, 3] = 1.0, -boxes[:, k]
        p[:, 3 + k, k], p[:, 3 + k, 3] = -1.0, boxes[:, 3 + k]
    return p.contiguous()


def frustum_boxes(cam12, h, w, th, tw, lo, hi):
    """the bounding box of every tile's frustum, from the camera's origin to the far side of the scene's extent [lo, hi], truncated at that
    extent: (tiles, 6) float32, tiles in tile_frusta's order"""
    c = np.asarray(cam12, dtype=np.float64)
    o, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    f = np.cross(hor, ver)
    f = f / np.sqrt(f @ f)
    if f @ (llc - o) < 0:
        f = -f
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    far = max(float(((corners - o) @ f).max()), 0.0)
    out = []
    for y0 in range(0, h, th):
        y1 = min(h, y0 + th)
        for x0 in range(0, w, tw):
            x1 = min(w, x0 + tw)
            d = [llc + u * hor + v * ver - o for u in (x0 / w, x1 / w) for v in ((h - y1) / h, (h - y0) / h)]
            pts = np.array([o] + [o + di * (far / (f @ di)) for di in d])
            blo, bhi = np.maximum(pts.min(axis=0), lo), np.minimum(pts.max(axis=0), hi)
            out.append(np.concatenate([blo, np.maximum(blo, bhi)]))
    return np.ascontiguousarray(np.array(out), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scenes", default="irreg,big")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator("cuda").manual_seed(7)
    for name in a.scenes.split(","):
        scene = ctx.scene(name)
        ps = R.prepare_scene(1000, 1000, scene)
        L = torch.from_numpy(ps.bvh_arrays()["L"]).cuda()
        c, r = L[:, :3].contiguous(), L[:, 6].contiguous()
        n = int(L.shape[0])
        info = dict(scene=name, spheres=n, height=ps.height)
        lo, hi = (c - r[:, None]).min(0).values, (c + r[:, None]).max(0).values
        # random cubes at about 100 spheres per row (boxes_probe's), as boxes and as their six planes
        m = min(n, 250000)
        half = 0.5 * float(np.sqrt(100.0 * float((hi[0] - lo[0]) * (hi[2] - lo[2])) / n))
        ctr = lo + torch.rand((m, 3), device="cuda", generator=gen) * (hi - lo)
        ctr[:, 1] = c[torch.randint(0, n, (m,), device="cuda", generator=gen), 1]
        boxes = torch.cat([ctr - half, ctr + half], dim=1).contiguous()
        bracket(ctx, ps, boxes, box_planes(boxes), a.iters, a.rounds, case=f"random cubes, half side {half:.3g}", superset="planes", **info)
        # the camera's tiles: four planes per tile against the frustum's bounding box
        cam = ps.camera()
        planes = torch.from_numpy(R.tile_frusta(cam, 1000, 1000, 16, 16)).cuda()
        fb = torch.from_numpy(frustum_boxes(cam, 1000, 1000, 16, 16, lo.cpu().numpy().astype(np.float64), hi.cpu().numpy().astype(np.float64))).cuda()
        bracket(ctx, ps, fb, planes, a.iters, a.rounds, case="tile frusta 1000 x 1000 / 16 x 16 against their bounding boxes", **info)
        ps.free()
        scene.free()
    ctx.close()


if __name__ == "__main__":
    main()
