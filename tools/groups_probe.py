"""Cost of the sphere groups (rt_prepared_set_groups, rt_*_masked) on one GPU, each figure next to a yardstick measured in the same run on the
same inputs.  Prints one JSON line per measurement: ms per call from HIP events on a torch stream the context enqueues on, after one untimed
warm-up call, `rounds` times in turn (the spread over the rounds is what a difference has to exceed).

    python tools/groups_probe.py [--iters N] [--rounds R] [--queries Q]

Scenes: irreg and the 10^6-sphere floor.  Queries: Q = 2^20 primary rays of the prepared camera (a 1024 x 1024 frame) and Q uniform points in the
scene's box at a modest bound.
  (a) mask 0xFFFFFFFF on groups of all ones against the unmasked entry: the price of the feature when it filters nothing (outputs held equal).
  (b) a mask that sees 1/8 of the spheres, once with spatially coherent groups (eight cells: x quartile by z half, equal counts) and once with
      scattered ones (c % 8 in the caller's order): the masked entry on the whole scene against the unmasked entry on a scene prepared from the
      seen spheres alone; for the range query also against the unmasked query on the whole scene plus a filter of its rows on the host.
  (c) set_groups with its derive, from words already on the device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracers_amd as R  # noqa: E402

VIEW = ((0.0, 5.0, 40.0), (0.0, 0.0, 0.0), 50.0)


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


class Queries:
    """the entries on fixed device inputs and outputs; mask None: the unmasked entry"""

    def __init__(self, ps, rays, pts, bound, k=8):
        self.ps, self.rays, self.pts, self.bound, self.k = ps, rays, pts, bound, k
        n = self.n = rays.shape[0]
        self.idx = torch.empty(n, dtype=torch.int32, device="cuda")
        self.hit = torch.empty((n, 7), dtype=torch.float32, device="cuda")
        self.occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        self.nidx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        self.ngap = torch.empty((n, k), dtype=torch.float32, device="cuda")
        self.off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        self.widx = self.wgap = None

    def intersect(self, mask):
        if mask is None:
            R.intersect_rays_into(self.rays.data_ptr(), self.n, self.ps, self.idx.data_ptr(), self.hit.data_ptr())
        else:
            R.intersect_rays_masked_into(self.rays.data_ptr(), self.n, self.ps, self.idx.data_ptr(), self.hit.data_ptr(), mask=mask)

    def occluded(self, mask):
        if mask is None:
            R.occluded_rays_into(self.rays.data_ptr(), self.n, self.ps, self.occ.data_ptr(), 0.1, 1e9)
        else:
            R.occluded_rays_masked_into(self.rays.data_ptr(), self.n, self.ps, self.occ.data_ptr(), 0.1, 1e9, mask=mask)

    def nearest(self, mask, count=True):
        c = self.cnt.data_ptr() if count else None
        if mask is None:
            R.nearest_spheres_into(self.pts.data_ptr(), self.n, self.ps, self.k, c, self.nidx.data_ptr(), self.ngap.data_ptr(), self.bound)
        else:
            R.nearest_spheres_masked_into(self.pts.data_ptr(), self.n, self.ps, self.k, c, self.nidx.data_ptr(), self.ngap.data_ptr(), self.bound, mask=mask)

    def within_count(self, mask):
        if mask is None:
            R.spheres_within_count_into(self.pts.data_ptr(), self.n, self.ps, self.off.data_ptr(), self.bound)
        else:
            R.spheres_within_masked_count_into(self.pts.data_ptr(), self.n, self.ps, self.off.data_ptr(), self.bound, mask=mask)

    def within_alloc(self, mask):
        self.within_count(mask)
        self.total = int(self.off[self.n].item())
        self.widx = torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda")
        self.wgap = torch.empty(max(self.total, 1), dtype=torch.float32, device="cuda")

    def within_fill(self, mask):
        if mask is None:
            R.spheres_within_fill_into(self.pts.data_ptr(), self.n, self.ps, self.off.data_ptr(), self.total, self.widx.data_ptr(), self.wgap.data_ptr(),
                                       None, self.bound)
        else:
            R.spheres_within_masked_fill_into(self.pts.data_ptr(), self.n, self.ps, self.off.data_ptr(), self.total, self.widx.data_ptr(),
                                              self.wgap.data_ptr(), None, self.bound, mask=mask)

    def steps(self, mask):
        self.within_alloc(mask)
        return [("intersect", lambda: self.intersect(mask)), ("occluded (0.1, 1e9)", lambda: self.occluded(mask)),
                (f"nearest k={self.k} count", lambda: self.nearest(mask)), (f"nearest k={self.k} pruned", lambda: self.nearest(mask, False)),
                ("within count + scan", lambda: self.within_count(mask)), ("within fill (index, gap)", lambda: self.within_fill(mask))]

    def outputs(self, mask):
        for _, fn in self.steps(mask):
            fn()
        torch.cuda.synchronize()
        return [t.clone() for t in (self.idx, self.hit, self.occ, self.cnt, self.nidx, self.ngap, self.off, self.widx[: self.total], self.wgap[: self.total])]


def emit(ctx, info, what, side, rnd, n, ms, **more):
    print(json.dumps(dict(info, what=what, side=side, round=rnd, queries=n, ms=round(ms, 4), mq_per_s=round(n / (ms * 1e3), 2), launch=ctx.last_launch,
                          **more)), flush=True)


def compare(ctx, info, a, b, iters, rounds):
    """a, b: (side name, Queries, mask): every step measured on a then on b, `rounds` times in turn"""
    sa, sb = a[1].steps(a[2]), b[1].steps(b[2])
    for rnd in range(rounds):
        for (what, fa), (_, fb) in zip(sa, sb):
            emit(ctx, info, what, a[0], rnd, a[1].n, timed(fa, iters), entries=a[1].total if "within" in what else None)
            emit(ctx, info, what, b[0], rnd, b[1].n, timed(fb, iters), entries=b[1].total if "within" in what else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--scenes", default="irreg,big")
    a = ap.parse_args()
    side = int(round(a.queries ** 0.5))
    n = side * side
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    for name in a.scenes.split(","):
        scene = ctx.scene(name)
        ps = R.prepare_scene(side, side, scene)
        L = ps.bvh_arrays()["L"]
        ids = ps.sphere_ids().astype(np.int64)
        ns = L.shape[0]
        caller = np.empty_like(L)
        caller[ids] = L
        info = dict(scene=name, spheres=ns, height=ps.height)
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        R.camera_rays_into(rays.data_ptr(), side, side, ps)
        lo, hi = L[:, :3].min(axis=0), L[:, :3].max(axis=0)
        g = torch.Generator("cuda").manual_seed(7)
        pts = (torch.from_numpy(lo).cuda() + torch.rand((n, 3), device="cuda", generator=g) * torch.from_numpy(hi - lo).cuda()).contiguous()
        bound = 30.0 if name == "big" else 10.0
        full = Queries(ps, rays, pts, bound)

        # (c) set_groups + derive, words already on the device
        ones = torch.full((ns,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for rnd in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                ps.set_groups(ones)          # (returns after a synchronise: a host clock around it)
            emit(ctx, info, "set_groups + derive", "masked", rnd, ns, (time.perf_counter() - t0) * 1e3 / a.iters)

        # (a) all ones against the unmasked entries; the outputs are the same
        want = full.outputs(None)
        got = full.outputs(0xFFFFFFFF)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), "mask all ones differs from the unmasked entry"
        compare(ctx, dict(info, case="(a) mask all ones"), ("unmasked", full, None), ("masked", full, 0xFFFFFFFF), a.iters, a.rounds)

        # (b) a mask that sees 1/8 of the spheres
        qx = np.searchsorted(np.quantile(caller[:, 0], [0.25, 0.5, 0.75]), caller[:, 0])
        cell = np.zeros(ns, np.int64)
        for q in range(4):
            sel = qx == q
            cell[sel] = 2 * q + (caller[sel, 2] > np.median(caller[sel, 2]))
        for kind, words in (("coherent", cell), ("scattered", np.arange(ns) % 8)):
            mask = 1 << 3
            ps.set_groups((1 << words).astype(np.uint32))
            seen = np.nonzero(words == 3)[0]
            sub = R.prepare_scene_from_spheres(ctx, caller[seen], side, side, *VIEW)
            subq = Queries(sub, rays, pts, bound)
            case = dict(info, case=f"(b) 1/8 seen, {kind}", seen=int(seen.size), subset_height=sub.height)
            compare(ctx, case, ("subset scene, unmasked", subq, None), ("masked", full, mask), a.iters, a.rounds)
            # the range query against unmasked + a filter of its rows on the host
            gL = torch.from_numpy(((1 << words).astype(np.uint32))[ids].astype(np.int64))
            for rnd in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                full.within_alloc(None)
                full.within_fill(None)
                torch.cuda.synchronize()
                off, idx, gap = full.off.cpu(), full.widx[: full.total].cpu(), full.wgap[: full.total].cpu()
                keep = (gL[idx.long()] & mask) != 0
                row = torch.repeat_interleave(torch.arange(n), torch.diff(off))
                rows = torch.bincount(row[keep], minlength=n)
                fidx, fgap = idx[keep], gap[keep]
                emit(ctx, case, "within: unmasked count + fill + copy + host filter", "unmasked + host filter", rnd, n, (time.perf_counter() - t0) * 1e3,
                     entries=int(full.total), kept=int(fidx.numel()))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                full.within_alloc(mask)
                full.within_fill(mask)
                torch.cuda.synchronize()
                off2, idx2, gap2 = full.off.cpu(), full.widx[: full.total].cpu(), full.wgap[: full.total].cpu()
                emit(ctx, case, "within: masked count + fill + copy", "masked", rnd, n, (time.perf_counter() - t0) * 1e3, entries=int(full.total))
                assert torch.equal(idx2, fidx) and torch.equal(gap2, fgap) and torch.equal(torch.diff(off2), rows), "masked rows != filtered rows"
            del subq
            sub.free()
        ps.free()
        scene.free()
    ctx.close()


if __name__ == "__main__":
    main()
