"""The sphere casts on the GPU against the numpy restatement (sweep_ref.py) on the edge scenes and query families of edge_sweeps.py: roots
equal to t_min / t_max bit for bit, zero discriminants, stationary queries, lists full of equal tau, origins on widened box faces, radii
that absorb the coordinates, inflated radii of zero, and the NaN / inf / denormal rays of edge_rays.py under edge radii and intervals.
test_sweep_edges_cpu.py holds the restatement equal to its walk form, to query_core.h's rule on the host and to a float64 brute force on
these inputs.  Also here: device pointers that are not 16-byte aligned for the sweep, proximity and range-query entries, and a bounded run
of tools/query_fuzz.py.  Every comparison is bit for bit (edge_rays.same_bits: any NaN matches any NaN)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_rays as E
import edge_sweeps as ES
import oracle_lib as O
import proximity_ref as P
import ray_query_ref as Q
import sweep_ref as S
import within_ref as W

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = tuple(ES.SCENES) + ("tall5000",)
KS = (1, 4, 5, 8, 9, 16, 17, 32)      # each list capacity of the sweep lane kernel and one past it
PARTS = ("count", "index", "start", "hit7")
same_bits = E.same_bits


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import raytracers_amd
    return raytracers_amd


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def _spec(name):
    if name == "tall5000":       # height 43, too large for LDS: the tallest tree of the suite's edge scenes
        return E._tall(5000), (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0
    return ES.SCENES[name]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    s, lf, la, fov = _spec(name)
    arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    fam = ES.sweep_families(arr, seed=3, per=24, cap=24) if name == "tall5000" else ES.sweep_families(arr, seed=1)
    rays, rq, lo, hi, label = ES.joined(fam)
    assert rays.shape[0] < 2500
    return arr, ref, fam, rays, rq, lo, hi, label


@functools.lru_cache(maxsize=None)
def _want(name):
    arr, ref, fam, rays, rq, lo, hi, label = _inputs(name)
    return S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, max(KS))


def _prefix(res, k):
    return (res[0],) + tuple(a[:, :k] for a in res[1:])


def _prepared(R, ctx, name):
    s, lf, la, fov = _spec(name)
    arr = _inputs(name)[0]
    scene = ctx.scene_from_spheres(s, lf, la, fov)
    ps = R.prepare_scene(64, 64, scene)
    got = ps.bvh_arrays()
    for k in ("left", "right", "parent"):
        assert (got[k] == arr[k]).all(), (name, k)
    for k in ("L", "bmin", "bmax"):
        assert got[k].tobytes() == arr[k].tobytes(), (name, k)
    return scene, ps


def _free(scene, ps):
    ps.free()
    scene.free()


def _same(got, want, what, label=None, fam=None):
    for part, g, w in zip(PARTS, got, want):
        try:
            same_bits(g, w, f"{what} {part}")
        except AssertionError:
            if label is not None:                 # again family by family, so that the failure names the family
                for i, f in enumerate(fam):
                    if (label == i).any():
                        same_bits(g[label == i], w[label == i], f"{what} {part} [{f}]")
            raise


def _outputs(torch, n, k):
    return [torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), -7, dtype=torch.int32, device="cuda"),
            torch.full((n, k), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n, k, 7), -7.0, dtype=torch.float32, device="cuda")]


@pytest.mark.parametrize("name", SCENES)
def test_edge_scene(R, ctx, name):
    import torch
    arr, ref, fam, rays, rq, lo, hi, label = _inputs(name)
    want = _want(name)
    n = rays.shape[0]
    scene, ps = _prepared(R, ctx, name)
    # the ranged entry: every query with its own radius and interval
    for k in KS:
        got = R.sweep_spheres(ps, rays, rq, k, lo, hi)
        assert ctx.last_launch == f"family=sweep k={k} (per-query)", ctx.last_launch
        _same(got, _prefix(want, k), f"{name} per-query k={k}", label, fam)
    # the scalar entry: the queries sorted into their (radius, t_min, t_max) buckets, one launch per bucket into its rows of the outputs
    order = np.lexsort((hi.view(np.uint32), lo.view(np.uint32), rq.view(np.uint32)))
    key = np.stack([rq.view(np.uint32), lo.view(np.uint32), hi.view(np.uint32)], axis=1)[order]
    first = np.nonzero(np.concatenate([[True], (key[1:] != key[:-1]).any(axis=1)]))[0]
    last = np.concatenate([first[1:], [n]])
    valid = S.query_ok(lo, hi, rq)[order]
    rays_d = torch.from_numpy(rays[order]).cuda()
    torch.cuda.synchronize()
    refused = 0
    for k in KS:
        outs = _outputs(torch, n, k)
        torch.cuda.synchronize()
        for a, b in zip(first.tolist(), last.tolist()):
            q = order[a]
            ptrs = [outs[0].data_ptr() + 4 * a, outs[1].data_ptr() + 4 * k * a, outs[2].data_ptr() + k * a, outs[3].data_ptr() + 28 * k * a]
            args = (rays_d.data_ptr() + 24 * a, b - a, ps, float(rq[q]), k, *ptrs)
            if valid[a]:
                R.sweep_spheres_into(*args, t_min=float(lo[q]), t_max=float(hi[q]))
                assert ctx.last_launch == f"family=sweep k={k}", ctx.last_launch
            else:                                  # the scalar entry refuses what the ranged one turns into a miss; nothing is written
                with pytest.raises(R.RtError):
                    R.sweep_spheres_into(*args, t_min=float(lo[q]), t_max=float(hi[q]))
                refused += 1
        ctx.sync()
        got = [t.cpu().numpy() for t in outs]
        assert (got[0][~valid] == -7).all() and (got[1][~valid] == -7).all() and (got[2][~valid] == 0xAB).all() and (got[3][~valid] == -7).all()
        _same([g[valid] for g in got], [w[order][valid] for w in _prefix(want, k)], f"{name} scalar buckets k={k}", label[order][valid], fam)
    assert refused > 0 and valid.sum() > n // 2 and first.size > 50, (refused, int(valid.sum()), first.size)
    _free(scene, ps)


def test_inputs_reach_long_lists_and_ties():
    # (of the restatement's answers the tests above compare with: lists longer than 32, equal tau in neighbouring slots of a full list)
    for name in ("same64", "tall1100", "overlap", "tall5000"):
        count, index, start, hit = _want(name)
        tau = hit[:, :, 0]
        tie = ((tau[:, 1:] == tau[:, :-1]) & (index[:, 1:] >= 0)).sum(axis=1)
        assert count.max() > 32 and tie.max() == 31, (name, int(count.max()), int(tie.max()))
        assert ((tau[:, 1:] == tau[:, :-1]) & (index[:, 1:] >= 0) & (start[:, 1:] == 0)).any(), name


@pytest.mark.parametrize("name", ["same64", "nan_grid", "overlap"])
def test_exclusion_under_ties(R, ctx, name):
    # excluding the lowest index of a tie group moves the rest of the list up one slot: against the restatement, and against the
    # un-excluded answer with one more slot minus that sphere
    arr, ref, fam, rays, rq, lo, hi, label = _inputs(name)
    scene, ps = _prepared(R, ctx, name)
    full = _want(name)
    tau, idx = full[3][:, :, 0], full[1]
    tie = (tau[:, 1:] == tau[:, :-1]) & (idx[:, 1:] >= 0)
    has = tie.any(axis=1)
    slot = np.argmax(tie, axis=1)
    ex = np.where(has, idx[np.arange(idx.shape[0]), slot], np.where(full[0] > 0, idx[:, 0], -1)).astype(np.int64)
    assert has.sum() > 100, (name, int(has.sum()))
    for k in (1, 8, 31):
        got = R.sweep_spheres(ps, rays, rq, k, lo, hi, exclude=ex)
        assert ctx.last_launch == f"family=sweep k={k} (per-query) exclude", ctx.last_launch
        _same(got, S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, k, ex), f"{name} exclude k={k}", label, fam)
        cnt, index, start, hit = R.sweep_spheres(ps, rays, rq, k + 1, lo, hi)
        listed = (index == ex[:, None]) & (index >= 0)
        assert listed.sum(axis=1).max() == 1 and listed.any(axis=1).sum() > 100, name
        assert np.array_equal(got[0], cnt - (ex >= 0))                 # (the excluded sphere is one of the query's contacts)
        keep = np.argsort(listed, axis=1, kind="stable")[:, :k]        # the slots without the excluded one, in order
        rows = np.arange(index.shape[0])[:, None]
        _same(got, (got[0], index[rows, keep], start[rows, keep], hit[rows, keep]), f"{name} un-excluded minus the sphere k={k}", label, fam)
    _free(scene, ps)


def test_null_outputs(R, ctx):
    import torch
    name = "overlap"
    arr, ref, fam, rays_np, rq_np, lo_np, hi_np, label = _inputs(name)
    scene, ps = _prepared(R, ctx, name)
    n = rays_np.shape[0]
    rays, rq, lo, hi = (torch.from_numpy(a).cuda() for a in (rays_np, rq_np, lo_np, hi_np))
    r0 = float(ES.median_radius(arr))
    want_s = S.sweep(ref, rays_np[:, :3], rays_np[:, 3:], r0, 0.0, 1e9, 32)
    assert want_s[0].max() > 32
    for ranged, want in ((True, _want(name)), (False, want_s)):
        for k in (5, 17, 32):
            for keep in range(4):
                outs = _outputs(torch, n, k)
                ptrs = [t.data_ptr() if i == keep else None for i, t in enumerate(outs)]
                torch.cuda.synchronize()
                if ranged:
                    R.sweep_spheres_ranged_into(rays.data_ptr(), n, ps, rq.data_ptr(), lo.data_ptr(), hi.data_ptr(), k, *ptrs)
                else:
                    R.sweep_spheres_into(rays.data_ptr(), n, ps, r0, k, *ptrs, t_min=0.0, t_max=1e9)
                ctx.sync()
                for i, t in enumerate(outs):
                    g = t.cpu().numpy()
                    if i == keep:
                        same_bits(g, want[i] if i == 0 else want[i][:, :k], f"ranged={ranged} k={k} only output {i}")
                    else:
                        assert (g == (0xAB if i == 2 else -7)).all(), f"ranged={ranged} k={k}: output {i} was written though its pointer is NULL"
    _free(scene, ps)


def test_unaligned_pointers(R, ctx):
    # rays 24 bytes into a larger tensor, points 12 bytes, per-query values, excludes and every 4-byte output 4 bytes (the start flags 1
    # byte) in: no such pointer is 16-byte aligned.  The int64 offsets of the range queries are 8 bytes in: aligned for their type only.
    import torch
    for name in ("random600", "overlap"):
        arr, ref, fam, rays_np, rq_np, lo_np, hi_np, label = _inputs(name)
        L = np.asarray(arr["L"], dtype=F)
        o, d = rays_np[:, :3], rays_np[:, 3:]
        n = rays_np.shape[0]
        scene, ps = _prepared(R, ctx, name)

        def big(shape, dtype, fill, rows=n, skip=1):
            # [rows, *shape], `skip` elements into a larger allocation
            t = torch.full((rows * int(np.prod(shape, dtype=np.int64)) + skip,), fill, dtype=dtype, device="cuda")[skip:].view((rows,) + shape)
            assert t.data_ptr() % 16 != 0 and t.is_contiguous()
            return t

        def dev(a, dtype):
            t = big(a.shape[1:], dtype, 0, a.shape[0], skip=int(np.prod(a.shape[1:], dtype=np.int64)))
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
            return t

        rays, rq, lo, hi = dev(rays_np, torch.float32), dev(rq_np, torch.float32), dev(lo_np, torch.float32), dev(hi_np, torch.float32)
        ex_np = np.random.default_rng(6).integers(-1, L.shape[0], n).astype(np.int32)
        ex = dev(ex_np, torch.int32)
        r0 = float(ES.median_radius(arr))
        for k in (5, 32):
            def outs():
                return [big((), torch.int32, -7), big((k,), torch.int32, -7), big((k,), torch.uint8, 0xAB), big((k, 7), torch.float32, -7.0)]
            for what in ("scalar", "per-query", "exclude"):
                ts = outs()
                torch.cuda.synchronize()
                if what == "scalar":
                    R.sweep_spheres_into(rays.data_ptr(), n, ps, r0, k, *[t.data_ptr() for t in ts], t_min=0.0, t_max=1e9)
                    want = S.sweep(ref, o, d, r0, 0.0, 1e9, k)
                else:
                    R.sweep_spheres_ranged_into(rays.data_ptr(), n, ps, rq.data_ptr(), lo.data_ptr(), hi.data_ptr(), k, *[t.data_ptr() for t in ts],
                                                exclude_ptr=ex.data_ptr() if what == "exclude" else None)
                    want = S.sweep(ref, o, d, rq_np, lo_np, hi_np, k, ex_np) if what == "exclude" else _prefix(_want(name), k)
                ctx.sync()
                _same([t.cpu().numpy() for t in ts], want, f"{name} sweep {what} k={k}", label, fam)
        # the proximity and range-query entries: points 12 bytes in
        pts_np = np.ascontiguousarray(o)
        pts = dev(pts_np, torch.float32)
        md_np = np.where(np.arange(n) % 5 == 0, F(np.nan), np.abs(rq_np) % F(50.0)).astype(F)
        md_np[1::7] = F(-1.0)
        md = dev(md_np, torch.float32)
        for k in (5, 32):
            for ranged in (False, True):
                for counted in (True, False):
                    cnt, idx, gap = big((), torch.int32, -7), big((k,), torch.int32, -7), big((k,), torch.float32, -7.0)
                    torch.cuda.synchronize()
                    cp = cnt.data_ptr() if counted else None
                    if ranged:
                        R.nearest_spheres_ranged_into(pts.data_ptr(), n, ps, md.data_ptr(), k, cp, idx.data_ptr(), gap.data_ptr())
                        want = P.nearest(L, pts_np, md_np, k)
                    else:
                        R.nearest_spheres_into(pts.data_ptr(), n, ps, k, cp, idx.data_ptr(), gap.data_ptr(), max_dist=12.5)
                        want = P.nearest(L, pts_np, 12.5, k)
                    ctx.sync()
                    what = f"{name} nearest k={k} ranged={ranged} counted={counted}"
                    if counted:
                        same_bits(cnt.cpu().numpy(), want[0], what + " count")
                    same_bits(idx.cpu().numpy(), want[1], what + " index")
                    same_bits(gap.cpu().numpy(), want[2], what + " gap")
        first_np = np.random.default_rng(8).integers(0, L.shape[0], n).astype(np.int32)
        first = dev(first_np, torch.int32)
        for ranged, with_first in ((False, False), (True, False), (True, True)):
            off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")[1:]
            assert off.data_ptr() % 16 == 8
            kw = dict(max_dist=0.0, max_dist_ptr=md.data_ptr()) if ranged else dict(max_dist=12.5)
            if with_first:
                kw["first_ptr"] = first.data_ptr()
            torch.cuda.synchronize()
            R.spheres_within_count_into(pts.data_ptr(), n, ps, off.data_ptr(), **kw)
            ctx.sync()
            want = W.within(L, pts_np, md_np if ranged else 12.5, first_np if with_first else None)
            what = f"{name} within ranged={ranged} first={with_first}"
            same_bits(off.cpu().numpy(), want[0], what + " offsets")
            total = int(want[0][-1])
            assert total > n // 4, (what, total)
            idx, gap, row = big((), torch.int32, -7, total), big((), torch.float32, -7.0, total), big((), torch.int32, -7, total)
            torch.cuda.synchronize()
            R.spheres_within_fill_into(pts.data_ptr(), n, ps, off.data_ptr(), total, idx.data_ptr(), gap.data_ptr(), row.data_ptr(), **kw)
            ctx.sync()
            same_bits(idx.cpu().numpy(), want[1], what + " index")
            same_bits(gap.cpu().numpy(), want[2], what + " gap")
            same_bits(row.cpu().numpy(), np.repeat(np.arange(n, dtype=np.int32), np.diff(want[0])), what + " point")
        for margin in (0.0, 1.5):
            ns = L.shape[0]
            off = torch.full((ns + 2,), -7, dtype=torch.int64, device="cuda")[1:]
            torch.cuda.synchronize()
            R.contact_pairs_count_into(ps, off.data_ptr(), margin)
            ctx.sync()
            pairs, gaps = W.contact_pairs(L, margin)
            total = pairs.shape[0]
            assert total > 0 and int(off.cpu().numpy()[-1]) == total, (name, margin, total)
            pair, gap = big((2,), torch.int32, -7, total), big((), torch.float32, -7.0, total)
            assert pair.data_ptr() % 8 == 4
            torch.cuda.synchronize()
            R.contact_pairs_fill_into(ps, off.data_ptr(), total, pair.data_ptr(), gap.data_ptr(), margin)
            ctx.sync()
            same_bits(pair.cpu().numpy(), pairs, f"{name} contact pairs margin {margin}")
            same_bits(gap.cpu().numpy(), gaps, f"{name} contact pairs margin {margin} gap")
        _free(scene, ps)


def test_random_query_campaign():
    """tools/query_fuzz.py for a bounded time: random scenes; sweep queries from the edge families and at random, scalar, per-query and
    with excludes; points at centres, on surfaces and far away through the proximity and range-query entries; contact pairs -- all
    against the restatements, bit for bit."""
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "query_fuzz.py"), "15", "7100"],
                         capture_output=True, text=True, timeout=170)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert " 0 mismatches" in out.stdout, out.stdout[-2000:]
