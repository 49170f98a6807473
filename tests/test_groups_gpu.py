"""Sphere groups on the GPU: rt_prepared_set_groups / rt_prepared_get_groups and the five masked entries against the numpy restatement
(groups_ref.py), every compare == on bits: scenes of 2, 3 and 65 random spheres, rgbbox (through prepare_scene), irreg and a tall chain (through
prepare_scene_from_spheres); 1, 63, 64, 65 and 1024 queries; six group patterns; scalar and per-query masks (mask arrays also at device
pointers that are only 4-byte aligned), scalar and per-query bounds, `first`, both k-nearest modes; poisoned outputs; the masked entries
against the unmasked ones and against one another; update_spheres; refusals, launch strings, n == 0 and repeatability."""

import numpy as np
import pytest

import groups_ref as G
import interval_ref as I
import occlusion_ref as X
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
COUNTS = (1, 63, 64, 65, 1024)
SCENES = ("rand2", "rand3", "rand65", "rgbbox", "irreg", "tall")
VIEW = ((0.0, 5.0, 40.0), (0.0, 0.0, 0.0), 50.0)
POISON = 0x7F


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: output {k} shape {g.shape} != {w.shape}"
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))[0] if g.size else np.zeros(0, int)
        assert bad.size == 0, f"{what}: output {k} differs on {bad.size} rows, first {bad[:5]}: got {g[bad[:2]]} want {w[bad[:2]]}"


def _random_spheres(n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), F)
    ext = 6.0 * max(1.0, float(n) ** (1.0 / 3.0))
    s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.5, 3.0, n)
    return s


class Prep:
    """one prepared scene with what the restatement needs: its arrays, ids, the spheres in the caller's order, and the queries of the tests"""

    def __init__(self, R, ctx, name):
        self.name = name
        if name in ("rgbbox", "irreg"):
            self.scene = ctx.scene(name)
            self.ps = R.prepare_scene(64, 64, self.scene)
        else:
            s = G.tall_chain() if name == "tall" else _random_spheres(int(name[4:]), int(name[4:]))
            self.scene = None
            self.ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
        self.refresh()
        arr, L = self.arr, self.arr["L"]
        n = L.shape[0]
        rng = np.random.default_rng(31)
        j = rng.integers(0, n, 256)
        off = rng.normal(size=(256, 3))
        off *= (3.0 * L[j, 6:7] + 1e-3) / np.linalg.norm(off, axis=1)[:, None]
        aimed = np.concatenate([L[j, :3] + off, -off * rng.uniform(0.5, 2.0, (256, 1))], axis=1)
        cam = self.ps.camera()
        self.rays = np.concatenate([Q.camera_rays(cam, 16, 16), aimed, X.seeded_rays(arr, 512, 7)]).astype(F)
        self.rays = self.rays[rng.permutation(1024)]
        lo, hi = (L[:, :3] - L[:, 6:7]).min(axis=0).astype(np.float64), (L[:, :3] + L[:, 6:7]).max(axis=0).astype(np.float64)
        self.extent = float(np.max(hi - lo))
        p = rng.uniform(lo, hi, (1024, 3)).astype(F)
        p[:256] = L[rng.integers(0, n, 256), :3]
        self.points = p[rng.permutation(1024)]
        self.masks = G.mixed_masks(1024, 13)
        self.masks[:5] = G.SCALAR_MASKS   # (every kind among the first 63 queries too)

    def refresh(self):
        self.arr = self.ps.bvh_arrays()
        self.ids = self.ps.sphere_ids().astype(np.int64)
        with np.errstate(divide="ignore"):
            self.ref = G.MaskedScene(self.arr)
        self.caller = np.empty_like(self.arr["L"])
        self.caller[self.ids] = self.arr["L"]

    def set(self, words):
        self.ps.set_groups(words)
        return G.gather(words, self.ids)


@pytest.fixture(scope="module")
def prep(R, ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Prep(R, ctx, name)
        return made[name]
    yield get
    for p in made.values():
        p.ps.free()
        if p.scene is not None:
            p.scene.free()


# ---- the entries through their pointer forms, on torch tensors: inputs on the device, outputs poisoned ------------------------------------
def _dev(t, a, dtype=None):
    a = np.array(a, copy=True, order="C")   # (a writable copy: torch does not take read-only arrays quietly)
    return t.as_tensor(a if dtype is None else a.view(dtype), device="cuda:0")


def _out(t, rows, cols, dtype):
    """a poisoned output of rows x cols elements of a 4-byte dtype (or uint8)"""
    size = 1 if dtype == t.uint8 else 4
    raw = t.full((max(rows * cols, 1) * size,), POISON, dtype=t.uint8, device="cuda:0")
    return raw.view(dtype)[: rows * cols].reshape(rows, cols) if cols > 1 else raw.view(dtype)[:rows]


def _mask_kw(t, masks, n, keep, misalign=True):
    """mask / mask_ptr for the pointer forms: a scalar, or an [n] array put at a device pointer that is 4-byte but not 8-byte aligned"""
    if np.ndim(masks) == 0:
        return {"mask": int(masks)}
    buf = t.zeros(n + 2, dtype=t.int32, device="cuda:0")
    at = 1 if (buf.data_ptr() % 8 == 0) == misalign else 2
    buf[at:at + n] = _dev(t, np.asarray(masks[:n], dtype=U), np.int32)
    keep.append(buf)
    assert (buf.data_ptr() + 4 * at) % 4 == 0 and ((buf.data_ptr() + 4 * at) % 8 != 0) == misalign
    return {"mask_ptr": buf.data_ptr() + 4 * at}


def _bound_kw(t, lo, hi, n, keep):
    if np.ndim(lo) == 0 and np.ndim(hi) == 0:
        return {"t_min": float(lo), "t_max": float(hi)}
    a, b = I._bounds(n, lo if np.ndim(lo) == 0 else lo[:n], hi if np.ndim(hi) == 0 else hi[:n])
    ta, tb = _dev(t, a), _dev(t, b)
    keep += [ta, tb]
    return {"t_min_ptr": ta.data_ptr(), "t_max_ptr": tb.data_ptr()}


def _gpu_intersect(R, ctx, pr, n, lo, hi, masks, hits=True):
    import torch as t
    keep = []
    rays = _dev(t, pr.rays[:n])
    idx, hit = _out(t, n, 1, t.int32), _out(t, n, 7, t.float32)
    kw = {**_bound_kw(t, lo, hi, n, keep), **_mask_kw(t, masks, n, keep)}
    t.cuda.synchronize()
    R.intersect_rays_masked_into(rays.data_ptr(), n, pr.ps, idx.data_ptr(), hit.data_ptr() if hits else None, **kw)
    ctx.sync()
    return idx.cpu().numpy(), hit.cpu().numpy().reshape(n, 7)


def _gpu_occluded(R, ctx, pr, n, lo, hi, masks):
    import torch as t
    keep = []
    rays = _dev(t, pr.rays[:n])
    out = _out(t, n, 1, t.uint8)
    kw = {**_bound_kw(t, lo, hi, n, keep), **_mask_kw(t, masks, n, keep)}
    t.cuda.synchronize()
    R.occluded_rays_masked_into(rays.data_ptr(), n, pr.ps, out.data_ptr(), **kw)
    ctx.sync()
    return out.cpu().numpy()


def _gpu_nearest(R, ctx, pr, n, k, md, masks, count=True):
    import torch as t
    keep = []
    pts = _dev(t, pr.points[:n])
    cnt, idx, gap = _out(t, n, 1, t.int32), _out(t, n * k, 1, t.int32), _out(t, n * k, 1, t.float32)
    kw = _mask_kw(t, masks, n, keep)
    if np.ndim(md) > 0:
        m = _dev(t, np.asarray(md[:n], dtype=F))
        keep.append(m)
        kw["max_dist_ptr"] = m.data_ptr()
    else:
        kw["max_dist"] = float(md)
    t.cuda.synchronize()
    R.nearest_spheres_masked_into(pts.data_ptr(), n, pr.ps, k, cnt.data_ptr() if count else None, idx.data_ptr(), gap.data_ptr(), **kw)
    ctx.sync()
    c = cnt.cpu().numpy()
    if not count:
        assert (c.view(np.uint8) == POISON).all()   # (untouched)
    return c, idx.cpu().numpy().reshape(n, k), gap.cpu().numpy().reshape(n, k)


# ---- groups() -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_groups_follow_ids_and_node_groups_are_exact(R, ctx, prep, name):
    pr = prep(name)
    A = pr.arr
    assert (pr.ids != np.arange(pr.ids.size)).any() or pr.ids.size <= 3
    for pname, words in G.patterns(pr.caller, 5).items():
        want = pr.set(words)
        g, ng = pr.ps.groups()
        assert g.dtype == U and np.array_equal(g, want), (name, pname)
        assert np.array_equal(ng, G.node_groups(A["left"], A["right"], want)), (name, pname)
    if name == "tall":
        assert pr.ps.height > int(np.log2(F(pr.ids.size))) + 6, pr.ps.height
    # a device tensor of int32 bits is taken in place; None clears; new words answer
    import torch as t
    words = G.patterns(pr.caller, 9)["random"]
    pr.ps.set_groups(_dev(t, words, np.int32))
    assert np.array_equal(pr.ps.groups()[0], words[pr.ids])
    pr.ps.set_groups(None)
    for call in (lambda: pr.ps.groups(), lambda: R.intersect_rays(pr.ps, pr.rays[:4], mask=1), lambda: R.occluded_rays(pr.ps, pr.rays[:4], mask=1),
                 lambda: R.nearest_spheres_masked(pr.ps, pr.points[:4], 1, mask=1), lambda: R.spheres_within_masked(pr.ps, pr.points[:4], 1.0, mask=1)):
        with pytest.raises(R.RtError, match="rt_prepared_set_groups"):
            call()
    assert R.intersect_rays(pr.ps, pr.rays[:4])[0].shape == (4,)   # (the unmasked entries do not care)
    g1 = pr.set(np.full(pr.ids.size, 2, U))
    assert (R.intersect_rays(pr.ps, pr.rays[:64], mask=1)[0] == -1).all()
    _same(R.intersect_rays(pr.ps, pr.rays[:64], mask=2), R.intersect_rays(pr.ps, pr.rays[:64]), "one group, its mask")
    assert np.array_equal(pr.ps.groups()[0], g1)


# ---- the ray entries against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["random", "octant", "bit_c_mod_32", "bit31_on_one", "all_zero", "all_ones"])
@pytest.mark.parametrize("name", SCENES)
def test_ray_entries(R, ctx, prep, name, pname):
    pr = prep(name)
    g = pr.set(G.patterns(pr.caller, 5)[pname])
    masks = pr.masks.copy()
    if pname == "bit31_on_one":
        masks[::3] = 0x80000000
    heavy = name == "irreg" and pname not in ("random", "octant")      # (the dense restatement of 1024 rays on 10^4 spheres takes a second)
    m = 65 if heavy else 1024
    iv_lo, iv_hi, _ = I.mixed_intervals(1024, 5)
    iv_hi[7], iv_lo[9], iv_hi[11] = np.nan, -1.0, 2e9                   # invalid per-ray intervals: misses
    short = F(0.3 * pr.extent)
    want = {("scalar", "idx"): G.objs_hit(pr.ref, pr.rays[:m], 0.0, 1e9, g, masks[:m]),
            ("scalar", "occ"): G.occluded(pr.ref, pr.rays[:m], F(0.1), short, g, masks[:m]),
            ("ranged", "idx"): G.objs_hit(pr.ref, pr.rays[:m], iv_lo[:m], iv_hi[:m], g, masks[:m]),
            ("ranged", "occ"): G.occluded(pr.ref, pr.rays[:m], iv_lo[:m], iv_hi[:m], g, masks[:m])}
    for n in [c for c in COUNTS if c <= m]:
        what = f"{name}/{pname} n={n}"
        _same(_gpu_intersect(R, ctx, pr, n, 0.0, 1e9, masks), [w[:n] for w in want["scalar", "idx"]], what)
        assert ctx.last_launch == "family=intersect masked mask=per-query", ctx.last_launch
        assert np.array_equal(_gpu_occluded(R, ctx, pr, n, 0.1, short, masks), want["scalar", "occ"][:n].astype(np.uint8)), what
        assert ctx.last_launch == "family=occluded masked mask=per-query", ctx.last_launch
        _same(_gpu_intersect(R, ctx, pr, n, iv_lo, iv_hi, masks), [w[:n] for w in want["ranged", "idx"]], what + " per-ray")
        assert ctx.last_launch == "family=intersect (per-ray) masked mask=per-query", ctx.last_launch
        assert np.array_equal(_gpu_occluded(R, ctx, pr, n, iv_lo, iv_hi, masks), want["ranged", "occ"][:n].astype(np.uint8)), what + " per-ray"
        assert ctx.last_launch == "family=occluded (per-ray) masked mask=per-query", ctx.last_launch
    # misses hold the unmasked entries' fill values (the outputs were poisoned)
    idx, hit = _gpu_intersect(R, ctx, pr, m, 0.0, 1e9, masks)
    assert (hit[idx < 0] == 0).all() and (idx[masks[:m] == 0] == -1).all()
    # scalar masks, each against the restatement; the index-only call
    for v in G.SCALAR_MASKS:
        w = G.objs_hit(pr.ref, pr.rays[:65], 0.0, 1e9, g, v)
        _same(_gpu_intersect(R, ctx, pr, 65, 0.0, 1e9, v), w, f"{name}/{pname} mask={v:#x}")
        assert ctx.last_launch == "family=intersect masked", ctx.last_launch
        assert np.array_equal(_gpu_intersect(R, ctx, pr, 65, 0.0, 1e9, v, hits=False)[0], w[0])
        assert np.array_equal(_gpu_occluded(R, ctx, pr, 65, iv_lo, iv_hi, v), G.occluded(pr.ref, pr.rays[:65], iv_lo[:65], iv_hi[:65], g, v))
        assert ctx.last_launch == "family=occluded (per-ray) masked", ctx.last_launch
    # the package's keyword: a Python int and an array, scalar and per-ray bounds
    _same(R.intersect_rays(pr.ps, pr.rays[:65], mask=masks[:65]), [w[:65] for w in want["scalar", "idx"]], "mask= array")
    _same(R.intersect_rays(pr.ps, pr.rays[:65], iv_lo[:65], iv_hi[:65], mask=masks[:65]), [w[:65] for w in want["ranged", "idx"]], "mask= array, ranged")
    assert np.array_equal(R.occluded_rays(pr.ps, pr.rays[:65], 0.1, float(short), mask=masks[:65]), want["scalar", "occ"][:65])


# ---- the proximity entries against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["random", "octant", "bit_c_mod_32", "bit31_on_one", "all_zero", "all_ones"])
@pytest.mark.parametrize("name", SCENES)
def test_proximity_entries(R, ctx, prep, name, pname):
    pr = prep(name)
    L = pr.arr["L"]
    g = pr.set(G.patterns(pr.caller, 5)[pname])
    masks = pr.masks.copy()
    if pname == "bit31_on_one":
        masks[::3] = 0x80000000
    heavy = name == "irreg" and pname not in ("random", "octant")
    m = 65 if heavy else 1024
    md = 0.05 * pr.extent
    rng = np.random.default_rng(3)
    mds = rng.uniform(0.0, 2 * md, 1024).astype(F)
    mds[5], mds[6], mds[8] = np.nan, -1.0, 2e9                          # invalid per-point bounds: misses
    first = rng.integers(-3, L.shape[0] + 3, 1024)
    want = {"scalar": G.nearest(L, pr.points[:m], md, 32, g, masks[:m]), "ranged": G.nearest(L, pr.points[:m], mds[:m], 32, g, masks[:m])}
    for n in [c for c in COUNTS if c <= m]:
        for k in (1, 8, 32) if n in (65, 1024) else (3,):
            for kind, bound in (("scalar", md), ("ranged", mds)):
                w = [want[kind][0][:n], want[kind][1][:n, :k], want[kind][2][:n, :k]]
                what = f"{name}/{pname} n={n} k={k} {kind}"
                _same(_gpu_nearest(R, ctx, pr, n, k, bound, masks), w, what)
                tail = (" (per-point)" if kind == "ranged" else "") + " masked mask=per-query"
                assert ctx.last_launch == f"family=nearest k={k}" + tail, ctx.last_launch
                _same(_gpu_nearest(R, ctx, pr, n, k, bound, masks, count=False)[1:], w[1:], what + " pruned")
                assert ctx.last_launch == f"family=nearest k={k} pruned" + tail, ctx.last_launch
    for v in G.SCALAR_MASKS:
        w = G.nearest(L, pr.points[:65], md, 8, g, v)
        _same(_gpu_nearest(R, ctx, pr, 65, 8, md, v), w, f"{name}/{pname} mask={v:#x}")
        assert ctx.last_launch == "family=nearest k=8 masked", ctx.last_launch
    _same(R.nearest_spheres_masked(pr.ps, pr.points[:65], 8, md, mask=masks[:65]), [want["scalar"][0][:65], want["scalar"][1][:65, :8], want["scalar"][2][:65, :8]],
          "mask= array")
    # the range query: scalar and per-point bounds, first, gaps=False / rows=True, per-query and scalar masks
    for bound in (md, mds):
        for fi in (None, first):
            ranged = np.ndim(bound) > 0
            w = G.within(L, pr.points[:m], bound[:m] if ranged else bound, g, masks[:m], None if fi is None else fi[:m])
            tail = (" (per-point)" if ranged else "") + (" first" if fi is not None else "") + " masked mask=per-query"
            for n in [c for c in COUNTS if c <= m]:
                got = R.spheres_within_masked(pr.ps, pr.points[:n], bound[:n] if ranged else bound, first=None if fi is None else fi[:n], mask=masks[:n])
                end = int(w[0][n])   # (a row depends on its own query alone: the first n rows of the restatement)
                _same(got, (w[0][: n + 1], w[1][:end], w[2][:end]), f"{name}/{pname} within n={n}{tail}")
                assert ctx.last_launch in ("family=within fill" + tail, "family=within count" + tail), ctx.last_launch
    w = G.within(L, pr.points[:65], md, g, masks[:65])
    off, idx, gap, row = R.spheres_within_masked(pr.ps, pr.points[:65], md, gaps=False, rows=True, mask=masks[:65])
    assert gap is None and np.array_equal(off, w[0]) and np.array_equal(idx, w[1])
    assert np.array_equal(row, np.repeat(np.arange(65), np.diff(off)))
    for v in G.SCALAR_MASKS:
        _same(R.spheres_within_masked(pr.ps, pr.points[:65], md, mask=v), G.within(L, pr.points[:65], md, g, v), f"{name}/{pname} within mask={v:#x}")
    # masked nearest == masked within, re-sorted by (gap, index) and cut at k (GPU against GPU)
    off, idx, gap = R.spheres_within_masked(pr.ps, pr.points[:m], mds[:m], mask=masks[:m])
    _same(_gpu_nearest(R, ctx, pr, m, 8, mds, masks), G.nearest_from_rows(m, 8, off, idx, gap), f"{name}/{pname} nearest from rows")


def test_within_fill_into_poisoned_arrays_with_room_to_spare(R, ctx, prep):
    import torch as t
    pr = prep("rgbbox")
    L = pr.arr["L"]
    g = pr.set(G.patterns(pr.caller, 5)["random"])
    n, md = 65, 0.05 * pr.extent
    w = G.within(L, pr.points[:n], md, g, pr.masks[:n])
    total = int(w[0][-1])
    assert total > 0
    keep = []
    pts = _dev(t, pr.points[:n])
    off = _out(t, (n + 1) * 2, 1, t.int32)
    idx, gap, row = _out(t, total + 7, 1, t.int32), _out(t, total + 7, 1, t.float32), _out(t, total + 7, 1, t.int32)
    kw = _mask_kw(t, pr.masks, n, keep)
    t.cuda.synchronize()
    R.spheres_within_masked_count_into(pts.data_ptr(), n, pr.ps, off.data_ptr(), md, **kw)
    assert ctx.last_launch == "family=within count masked mask=per-query"
    R.spheres_within_masked_fill_into(pts.data_ptr(), n, pr.ps, off.data_ptr(), total + 7, idx.data_ptr(), gap.data_ptr(), row.data_ptr(), md, **kw)
    assert ctx.last_launch == "family=within fill masked mask=per-query"
    ctx.sync()
    assert np.array_equal(off.cpu().numpy().view(np.int64), w[0])
    _same((idx.cpu().numpy()[:total], gap.cpu().numpy()[:total]), w[1:], "fill")
    for a in (idx, gap, row):
        assert (a.cpu().numpy()[total:].view(np.uint8) == POISON).all()
    # a capacity below the total: nothing at or past it
    idx2 = _out(t, total + 7, 1, t.int32)
    t.cuda.synchronize()
    R.spheres_within_masked_fill_into(pts.data_ptr(), n, pr.ps, off.data_ptr(), total // 2, idx2.data_ptr(), None, None, md, **kw)
    ctx.sync()
    h = idx2.cpu().numpy()
    assert np.array_equal(h[: total // 2], w[1][: total // 2]) and (h[total // 2:].view(np.uint8) == POISON).all()


# ---- GPU against GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_masked_entries_against_the_unmasked_ones(R, ctx, prep, name):
    pr = prep(name)
    ps, rays, pts = pr.ps, pr.rays, pr.points
    md = 0.05 * pr.extent
    short = float(F(0.3 * pr.extent))
    # mask all ones on groups without a zero word == the unmasked entry, on all outputs
    pr.set(G.patterns(pr.caller, 5)["bit_c_mod_32"])
    for mask in (0xFFFFFFFF, np.full(1024, 0xFFFFFFFF, U)):
        _same(R.intersect_rays(ps, rays, mask=mask), R.intersect_rays(ps, rays), "intersect, all ones")
        assert np.array_equal(R.occluded_rays(ps, rays, 0.1, short, mask=mask), R.occluded_rays(ps, rays, 0.1, short))
        for count in (True, False):
            got, want = R.nearest_spheres_masked(ps, pts, 8, md, count=count, mask=mask), R.nearest_spheres(ps, pts, 8, md, count=count)
            _same(got[1:], want[1:], "nearest, all ones")
            assert (got[0] is None and want[0] is None) or np.array_equal(got[0], want[0])
        _same(R.spheres_within_masked(ps, pts, md, mask=mask), R.spheres_within(ps, pts, md), "within, all ones")
    # within: the masked rows == the unmasked rows filtered by groups[index] & mask
    g = pr.set(G.patterns(pr.caller, 5)["random"])
    off, idx, gap, row = R.spheres_within(ps, pts, md, rows=True)
    keep = (g[idx] & pr.masks[row]) != 0
    got = R.spheres_within_masked(ps, pts, md, rows=True, mask=pr.masks)
    assert np.array_equal(got[1], idx[keep]) and np.array_equal(_bits(got[2]), _bits(gap[keep])) and np.array_equal(got[3], row[keep])
    assert np.array_equal(np.diff(got[0]), np.bincount(row[keep], minlength=1024))
    if name not in ("rand2", "rand3"):
        assert 0 < keep.sum() < keep.size
    # masked occluded == (masked intersect over the same interval hits), wherever the unmasked pair agrees the same way
    agree = R.occluded_rays(ps, rays, 0.1, short) == (R.intersect_rays(ps, rays, 0.1, short)[0] >= 0)
    occ, hit = R.occluded_rays(ps, rays, 0.1, short, mask=pr.masks), R.intersect_rays(ps, rays, 0.1, short, mask=pr.masks)[0] >= 0
    assert agree.mean() > 0.5 and np.array_equal(occ[agree], hit[agree]), name
    # repeatability
    _same(R.intersect_rays(ps, rays, mask=pr.masks), R.intersect_rays(ps, rays, mask=pr.masks), "two runs")
    _same(R.spheres_within_masked(ps, pts, md, mask=pr.masks), got[:3], "two runs")


# ---- update_spheres ----------------------------------------------------------------------------------------------------------------------------
def test_groups_follow_update_spheres(R, ctx):
    s = _random_spheres(300, 77)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    words = G.patterns(s, 5)["random"]
    ps.set_groups(words)
    ids0 = ps.sphere_ids().astype(np.int64)
    assert np.array_equal(ps.groups()[0], words[ids0])
    rng = np.random.default_rng(78)
    moved = s.copy()
    moved[:, :3] = moved[rng.permutation(300), :3] + rng.normal(0.0, 1.0, (300, 3)).astype(F)   # (sphere c keeps its radius, colour and word)
    ps.update_spheres(moved)
    ids1 = ps.sphere_ids().astype(np.int64)
    assert (ids0 != ids1).any()
    A = ps.bvh_arrays()
    g, ng = ps.groups()                                                   # no new set_groups
    assert np.array_equal(g, words[ids1]) and np.array_equal(ng, G.node_groups(A["left"], A["right"], g))
    ref = G.MaskedScene(A)
    rays = X.seeded_rays(A, 256, 3)
    masks = G.mixed_masks(256, 4)
    _same(R.intersect_rays(ps, rays, mask=masks), G.objs_hit(ref, rays, 0.0, 1e9, g, masks), "after update")
    pts = A["L"][rng.integers(0, 300, 128), :3]
    _same(R.spheres_within_masked(ps, pts, 3.0, mask=masks[:128]), G.within(A["L"], pts, 3.0, g, masks[:128]), "after update")
    # an update straight behind a masked query, then a masked query first: the derive runs ahead of it
    ps.update_spheres(s)
    ids2 = ps.sphere_ids().astype(np.int64)
    A = ps.bvh_arrays()
    _same(R.nearest_spheres_masked(ps, pts, 4, 3.0, mask=masks[:128]), G.nearest(A["L"], pts, 3.0, 4, words[ids2], masks[:128]), "derive ahead of the launch")
    ps.free()


# ---- refusals, n == 0 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_queries(R, ctx, prep):
    import torch as t
    pr = prep("rand65")
    ps = pr.ps
    n = pr.ids.size
    pr.set(np.ones(n, U))
    with pytest.raises(R.RtError, match="rt_prepared_num_spheres"):
        ps.set_groups(np.ones(n + 1, U))
    with pytest.raises(R.RtError, match="rt_prepared_num_spheres"):
        ps.set_groups(np.ones(n - 1, U))
    with pytest.raises(ValueError):
        ps.set_groups(np.full(n, -1, np.int64))
    with pytest.raises(ValueError):
        ps.set_groups(np.full(n, 2 ** 32, np.int64))
    with pytest.raises(ValueError):
        R.intersect_rays(ps, pr.rays[:4], mask=2 ** 32)
    with pytest.raises(ValueError):
        R.intersect_rays(ps, pr.rays[:4], mask=np.ones(5, U))
    assert np.array_equal(ps.groups()[0], np.ones(n, U))                 # (a refusal changes nothing)
    rays, pts = _dev(t, pr.rays[:8]), _dev(t, pr.points[:8])
    out = t.zeros(64, dtype=t.int32, device="cuda:0")
    t.cuda.synchronize()
    o = out.data_ptr()
    bad = [
        (lambda: R.intersect_rays_masked_into(rays.data_ptr(), 8, ps, None), "null index"),
        (lambda: R.intersect_rays_masked_into(None, 8, ps, o), "null rays"),
        (lambda: R.intersect_rays_masked_into(rays.data_ptr(), 8, ps, o, t_min=2.0, t_max=1.0), "t_min <= t_max"),
        (lambda: R.intersect_rays_masked_into(rays.data_ptr(), 8, ps, o, t_max=float("nan")), "t_min <= t_max"),
        (lambda: R.intersect_rays_masked_into(rays.data_ptr(), 8, ps, o, t_min_ptr=o), "both"),
        (lambda: R.intersect_rays_masked_into(rays.data_ptr(), -1, ps, o), "out of range"),
        (lambda: R.occluded_rays_masked_into(rays.data_ptr(), 8, ps, None), "null output"),
        (lambda: R.occluded_rays_masked_into(rays.data_ptr(), 8, ps, o, t_max=2e9), "t_min <= t_max"),
        (lambda: R.nearest_spheres_masked_into(pts.data_ptr(), 8, ps, 4, None, None, None), "outputs are NULL"),
        (lambda: R.nearest_spheres_masked_into(pts.data_ptr(), 8, ps, 33, o, o, None), "k <= 32"),
        (lambda: R.nearest_spheres_masked_into(pts.data_ptr(), 8, ps, 0, o, o, None), "k <= 32"),
        (lambda: R.nearest_spheres_masked_into(None, 8, ps, 4, o, o, None), "null points"),
        (lambda: R.nearest_spheres_masked_into(pts.data_ptr(), 8, ps, 4, o, o, None, max_dist=-1.0), "max_dist"),
        (lambda: R.spheres_within_masked_count_into(pts.data_ptr(), 8, ps, None), "null offsets"),
        (lambda: R.spheres_within_masked_count_into(pts.data_ptr(), 8, ps, o, max_dist=float("inf")), "max_dist"),
        (lambda: R.spheres_within_masked_fill_into(pts.data_ptr(), 8, ps, o, 8, None), "every output is NULL"),
        (lambda: R.spheres_within_masked_fill_into(pts.data_ptr(), 8, ps, o, -1, o), "negative capacity"),
        (lambda: ps.groups_into(None, None), "both outputs are NULL"),
    ]
    for call, text in bad:
        with pytest.raises(R.RtError, match=text):
            call()
    ctx.sync()
    assert (out == 0).all()                                               # nothing launched or written
    # a foreign context
    other = R.Context(0)
    foreign = R.Prepared(other, ps._h, 64, 64)
    try:
        for call in (lambda: foreign.set_groups(np.ones(n, U)), lambda: foreign.groups(), lambda: R.intersect_rays(foreign, pr.rays[:4], mask=1),
                     lambda: R.spheres_within_masked(foreign, pr.points[:4], 1.0, mask=1)):
            with pytest.raises(R.RtError, match="context that prepared"):
                call()
    finally:
        foreign._h = None
        other.close()
    # n == 0
    empty_r, empty_p = np.zeros((0, 6), F), np.zeros((0, 3), F)
    assert R.intersect_rays(ps, empty_r, mask=1)[0].shape == (0,) and ctx.last_launch == "family=none (no rays)"
    assert R.occluded_rays(ps, empty_r, mask=np.zeros(0, U)).shape == (0,) and ctx.last_launch == "family=none (no rays)"
    assert R.nearest_spheres_masked(ps, empty_p, 3, mask=1)[1].shape == (0, 3) and ctx.last_launch == "family=none (no points)"
    off, idx, gap = R.spheres_within_masked(ps, empty_p, 1.0, mask=1)
    assert np.array_equal(off, [0]) and idx.size == 0 and ctx.last_launch == "family=within count masked"


def test_multi_device_context_is_refused(R):
    try:
        multi = R.Context(devices=[0, 0])
    except R.RtError:
        pytest.skip("no multi-device context on this box")
    try:
        scene = multi.scene("rgbbox")
        ps = R.prepare_scene(32, 32, scene)
        with pytest.raises(R.RtError, match="multi-device"):
            ps.set_groups(np.ones(ps.num_spheres, U))
        with pytest.raises(R.RtError, match="multi-device"):
            ps.groups()
        ps.free()
        scene.free()
    finally:
        multi.close()
