"""Cost of the range queries (rt_spheres_within_count / _fill, rt_contact_pairs_count / _fill) on one GPU against the yardstick that does the
identical walk: rt_nearest_spheres in count mode (k = 1, only count_dev), re-measured in the same run on the same inputs.  Prints one JSON
line per measurement: ms per call from HIP events on a torch stream the context enqueues on, after one untimed warm-up call.

    python tools/within_probe.py [--iters N] [--rounds R]

Cases:
  * self-contacts of irreg and of the 10^6-sphere floor: points = the spheres' centres, per-point bounds = their radii, in L order (Morton
    order) and shuffled; in L order also the contact-pair entries (the self mode: no points array, each pair once);
  * 10^6 random points in the floor's box at bound 30 (about 92 spheres per row).
Per case the bracket [yardstick, count pass with its scan, fill pass] is measured `rounds` times in turn; the spread of a measurement over the
rounds is what a difference between two of them has to exceed.  The fill pass writes index and gap (pairs and gap in the self mode):
`bytes` is what one call writes."""
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


def bracket(ctx, ps, pts, bound, iters, rounds, self_mode=False, **info):
    """bound: a float (scalar max_dist) or a float32 device tensor (per-point); self_mode: also the contact-pair entries at margin 0"""
    n = pts.shape[0]
    ranged = torch.is_tensor(bound)
    md, mdp = (0.0, bound.data_ptr()) if ranged else (bound, None)
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    if ranged:
        yard = lambda: R.nearest_spheres_ranged_into(pts.data_ptr(), n, ps, mdp, 1, cnt.data_ptr(), None, None)  # noqa: E731
    else:
        yard = lambda: R.nearest_spheres_into(pts.data_ptr(), n, ps, 1, cnt.data_ptr(), None, None, md)  # noqa: E731
    count = lambda: R.spheres_within_count_into(pts.data_ptr(), n, ps, off.data_ptr(), md, mdp)  # noqa: E731
    count()
    total = int(off[n].item())
    yard()
    torch.cuda.synchronize()
    assert torch.equal(torch.diff(off).to(torch.int32), cnt), "row lengths != the yardstick's counts"
    idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    gap = torch.empty(max(total, 1), dtype=torch.float32, device="cuda")
    fill = lambda: R.spheres_within_fill_into(pts.data_ptr(), n, ps, off.data_ptr(), total, idx.data_ptr(), gap.data_ptr(), None, md, mdp)  # noqa: E731
    steps = [("nearest count k=1 (yardstick)", yard, 4 * n, total), ("within count + scan", count, 8 * (n + 1), total),
             ("within fill (index, gap)", fill, 8 * total, total)]
    if self_mode:
        off2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        pcount = lambda: R.contact_pairs_count_into(ps, off2.data_ptr(), 0.0)  # noqa: E731
        pcount()
        ptotal = int(off2[n].item())
        pair = torch.empty((max(ptotal, 1), 2), dtype=torch.int32, device="cuda")
        pgap = torch.empty(max(ptotal, 1), dtype=torch.float32, device="cuda")
        pfill = lambda: R.contact_pairs_fill_into(ps, off2.data_ptr(), ptotal, pair.data_ptr(), pgap.data_ptr(), 0.0)  # noqa: E731
        steps += [("contact pairs count + scan", pcount, 8 * (n + 1), ptotal), ("contact pairs fill (pairs, gap)", pfill, 12 * ptotal, ptotal)]
    for rnd in range(rounds):
        for what, fn, nbytes, entries in steps:
            ms = timed(fn, iters)
            print(json.dumps(dict(info, what=what, round=rnd, queries=n, entries=entries, per_row=round(entries / n, 3), bytes=nbytes,
                                  ms=round(ms, 4), mq_per_s=round(n / (ms * 1e3), 2), launch=ctx.last_launch)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for name in ("irreg", "big"):
        scene = ctx.scene(name)
        ps = R.prepare_scene(64, 64, scene)
        L = torch.from_numpy(ps.bvh_arrays()["L"]).cuda()
        c, r = L[:, :3].contiguous(), L[:, 6].contiguous()
        info = dict(scene=name, spheres=int(L.shape[0]), height=ps.height)
        bracket(ctx, ps, c, r, a.iters, a.rounds, self_mode=True, case="self-contacts", order="morton", **info)
        if name == "big":
            perm = torch.from_numpy(rng.permutation(L.shape[0])).cuda()
            bracket(ctx, ps, c[perm].contiguous(), r[perm].contiguous(), a.iters, a.rounds, case="self-contacts", order="shuffled", **info)
            lo, hi = c.min(0).values, c.max(0).values
            pts = (lo + torch.rand((1000000, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(7)) * (hi - lo)).contiguous()
            pts[:, 1] = torch.rand(1000000, device="cuda") * 20.0 - 10.0
            bracket(ctx, ps, pts, 30.0, a.iters, a.rounds, case="random points, bound 30", order="random", **info)
        ps.free()
        scene.free()
    ctx.close()


if __name__ == "__main__":
    main()
