"""Cost of the box queries (rt_spheres_in_boxes_count / _fill) on one GPU against the point queries (rt_spheres_within_count / _fill) on the
same positions, re-measured in the same run.  Prints one JSON line per measurement: ms per call from HIP events on a torch stream the
context enqueues on, after one untimed warm-up call.

    python tools/boxes_probe.py [--iters N] [--rounds R]

Cases, for irreg and for the 10^6-sphere floor:
  * degenerate boxes at the spheres' centres, per-box margins = their radii, in L order (Morton order): the two walks are identical (the same
    nodes, the same leaves, the same rows -- asserted), so the difference is the price of the six-coordinate tests;
  * a grid of cells of about three sphere diameters over the scene's x / z extent, the whole y extent, margin 0;
  * random cubes sized for about 100 spheres per row, margin 0.
For real boxes the yardstick is the point query at the box's centre with the half diagonal as its bound -- the circumscribed ball a caller
without box queries would have to ask for, and then filter: its rows are longer, and both row counts are printed.
Per case the bracket [within count + scan, boxes count + scan, within fill, boxes fill] is measured `rounds` times in turn; the spread of a
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


def bracket(ctx, ps, boxes, margin, pts, bound, iters, rounds, identical, **info):
    """boxes (n, 6) with margin (a float or an (n,) float32 device tensor); the yardstick's points (n, 3) with bound (likewise)"""
    n = boxes.shape[0]
    mg, mgp = (0.0, margin.data_ptr()) if torch.is_tensor(margin) else (margin, None)
    md, mdp = (0.0, bound.data_ptr()) if torch.is_tensor(bound) else (bound, None)
    off_b = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    off_w = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    bcount = lambda: R.spheres_in_boxes_count_into(boxes.data_ptr(), n, ps, off_b.data_ptr(), mg, mgp)  # noqa: E731
    wcount = lambda: R.spheres_within_count_into(pts.data_ptr(), n, ps, off_w.data_ptr(), md, mdp)  # noqa: E731
    bcount()
    wcount()
    tb, tw = int(off_b[n].item()), int(off_w[n].item())
    cap = max(tb, tw, 1)
    idx_b, idx_w = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    gap_b, gap_w = (torch.empty(cap, dtype=torch.float32, device="cuda") for _ in range(2))
    bfill = lambda: R.spheres_in_boxes_fill_into(boxes.data_ptr(), n, ps, off_b.data_ptr(), tb, idx_b.data_ptr(), gap_b.data_ptr(), None, mg, mgp)  # noqa: E731
    wfill = lambda: R.spheres_within_fill_into(pts.data_ptr(), n, ps, off_w.data_ptr(), tw, idx_w.data_ptr(), gap_w.data_ptr(), None, md, mdp)  # noqa: E731
    bfill()
    wfill()
    torch.cuda.synchronize()
    if identical:
        assert torch.equal(off_b, off_w) and torch.equal(idx_b[:tb], idx_w[:tw]), "degenerate boxes: rows differ from the point query's"
        assert torch.equal(gap_b[:tb].view(torch.int32), gap_w[:tw].view(torch.int32)), "degenerate boxes: gap bits differ from the point query's"
    else:
        assert bool((torch.diff(off_b) <= torch.diff(off_w)).all()), "a box selected more than its circumscribed ball"
    steps = [("within count + scan (yardstick)", wcount, tw), ("boxes count + scan", bcount, tb), ("within fill (yardstick)", wfill, tw),
             ("boxes fill (index, gap)", bfill, tb)]
    for rnd in range(rounds):
        for what, fn, entries in steps:
            ms = timed(fn, iters)
            print(json.dumps(dict(info, what=what, round=rnd, queries=n, entries=entries, per_row=round(entries / n, 3), ms=round(ms, 4),
                                  mq_per_s=round(n / (ms * 1e3), 2), launch=ctx.last_launch)), flush=True)


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
        ps = R.prepare_scene(64, 64, scene)
        L = torch.from_numpy(ps.bvh_arrays()["L"]).cuda()
        c, r = L[:, :3].contiguous(), L[:, 6].contiguous()
        n = int(L.shape[0])
        info = dict(scene=name, spheres=n, height=ps.height)
        # degenerate boxes at the centres
        bracket(ctx, ps, torch.cat([c, c], dim=1).contiguous(), r, c, r, a.iters, a.rounds, True, case="degenerate boxes at the centres", **info)
        lo, hi = (c - r[:, None]).min(0).values, (c + r[:, None]).max(0).values
        # a grid of cells of about three diameters over x / z (at most 1024 x 1024 cells)
        cell = max(6.0 * float(r.median()), float(max(hi[0] - lo[0], hi[2] - lo[2])) / 1024.0)
        gx, gz = (max(1, int(np.ceil(float(hi[k] - lo[k]) / cell))) for k in (0, 2))
        ix, iz = torch.meshgrid(torch.arange(gx, device="cuda"), torch.arange(gz, device="cuda"), indexing="ij")
        ix, iz = ix.reshape(-1).float(), iz.reshape(-1).float()
        blo = torch.stack([lo[0] + ix * cell, lo[1].expand_as(ix), lo[2] + iz * cell], dim=1)
        bhi = torch.stack([lo[0] + (ix + 1) * cell, hi[1].expand_as(ix), lo[2] + (iz + 1) * cell], dim=1)
        boxes = torch.cat([blo, bhi], dim=1).contiguous()
        mid = (0.5 * (blo + bhi)).contiguous()
        half_diag = torch.linalg.norm(0.5 * (bhi - blo), dim=1).contiguous() * 1.001   # (rounded up: the ball holds the box, float32 centres included)
        bracket(ctx, ps, boxes, 0.0, mid, half_diag, a.iters, a.rounds, False, case=f"grid {gx} x 1 x {gz}, cell {cell:.3g}", **info)
        # random cubes at about 100 spheres per row (by the density over x / z: both scenes are layers)
        m = min(n, 250000)
        half = 0.5 * float(np.sqrt(100.0 * float((hi[0] - lo[0]) * (hi[2] - lo[2])) / n))
        ctr = lo + torch.rand((m, 3), device="cuda", generator=gen) * (hi - lo)
        ctr[:, 1] = c[torch.randint(0, n, (m,), device="cuda", generator=gen), 1]
        boxes = torch.cat([ctr - half, ctr + half], dim=1).contiguous()
        bound = float(np.sqrt(3.0) * half * 1.001)
        bracket(ctx, ps, boxes, 0.0, ctr.contiguous(), bound, a.iters, a.rounds, False, case=f"random cubes, half side {half:.3g}", **info)
        ps.free()
        scene.free()
    ctx.close()


if __name__ == "__main__":
    main()
