"""Range queries on the GPU: rt_spheres_within_count / _fill and rt_contact_pairs_count / _fill against the numpy restatement (within_ref.py),
bit for bit (offsets, index, gap bits), on the reference's scenes, random scenes of every GPU-builder size class, tall trees, point clouds
and adversarial inputs; a dense case the capped query cannot answer; consistency with rt_nearest_spheres; the `first` filter; contact pairs
(one-sided rule, sphere ids, update_spheres); 64-bit offsets and the capacity guard; refusals, launch strings, n == 0, repeatability and
outputs allocated by torch.

Measured note on test 7: the issue's 4 096 points x 10^6 spheres give a total of 4.096e9, which is past 2^31 (int32) but below 2^32 =
4.295e9; the test keeps that case as stated (offsets[i] == i * 10^6) and adds 4 352 points (4.352e9 > 2^32) so that a sum really passes
32 bits."""
import ctypes as C

import numpy as np
import pytest

import proximity_ref as P
import within_ref as W
from test_proximity_gpu import VIEW, _geometric, _points, _random_spheres

pytestmark = pytest.mark.gpu

F = np.float32


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


@pytest.fixture(scope="module")
def floor(R, ctx):
    """the 10^6-sphere floor, prepared once: (prepared scene, L)"""
    scene = ctx.scene("big")
    ps = R.prepare_scene(100, 100, scene)
    L = ps.bvh_arrays()["L"]
    assert L.shape[0] == 1000000 and ps.height > 15
    yield ps, L
    ps.free()
    scene.free()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(got, want, what):
    for name, g, w in zip(("offsets", "index", "gap"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        bad = np.nonzero(_bits(g) != _bits(w))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


def _restate(L, p, md, first=None):
    # the dense brute force; the restricted one where that would be large and every bound is modest (the CPU suite holds the two equal)
    big = L.shape[0] * p.shape[0] > (1 << 27)
    if big:
        assert float(np.nanmax(np.where(P.max_dist_ok(np.asarray(md, F)), md, 0))) <= 100.0
        return W.within_near(L, p, md, first)
    return W.within(L, p, md, first)


def _check(R, ctx, ps, L, p, md, what, nearest=True):
    """spheres_within against the restatement (with and without gaps / rows), and against the shipped capped query on the same inputs"""
    want = _restate(L, p, md)
    ranged = np.ndim(md) > 0
    got = R.spheres_within(ps, p, md)
    assert ctx.last_launch == "family=within fill" + (" (per-point)" if ranged else "") or want[0][-1] == 0, ctx.last_launch
    _same(got, want, what)
    off, idx, gap = got
    m = p.shape[0]
    o2, i2, g2, r2 = R.spheres_within(ps, p, md, gaps=False, rows=True)
    assert g2 is None and np.array_equal(o2, off) and np.array_equal(i2, idx)
    assert r2.dtype == np.int32 and np.array_equal(r2, np.repeat(np.arange(m, dtype=np.int32), np.diff(off))), what
    if nearest:
        # 4. the shipped query: row lengths == its counts; rows no longer than 32, re-sorted by (gap, j), == its slots
        cnt, nidx, ngap = R.nearest_spheres(ps, p, 32, md)
        assert np.array_equal(np.diff(off), cnt), what
        sidx, sgap = W.sort_rows_by_gap(off, idx, gap)
        ln = np.diff(off)
        short = np.nonzero(ln <= 32)[0]
        slot = np.arange(32)[None, :] < ln[short, None]
        assert np.array_equal(nidx[short][slot], np.concatenate([sidx[off[i]:off[i + 1]] for i in short] + [np.zeros(0, np.int32)])), what
        assert np.array_equal(_bits(ngap[short][slot]), _bits(np.concatenate([sgap[off[i]:off[i + 1]] for i in short] + [np.zeros(0, F)]))), what
        assert (nidx[short][~slot] == -1).all(), what
    return want


def _check_pairs(R, ctx, ps, L, margin, what, near=None):
    near = L.shape[0] > 4000 if near is None else near
    want = W.contact_pairs(L, margin, near=near)
    pairs, gap = R.contact_pairs(ps, margin)
    assert ctx.last_launch in ("family=within fill self", "family=within count self"), ctx.last_launch
    assert pairs.dtype == np.int32 and pairs.shape == want[0].shape, f"{what}: {pairs.shape} pairs, want {want[0].shape}"
    assert np.array_equal(pairs, want[0]), what
    assert np.array_equal(_bits(gap), _bits(want[1])), what
    p2, g2 = R.contact_pairs(ps, margin, gaps=False)
    assert g2 is None and np.array_equal(p2, pairs)
    return pairs, gap


# ---- 1. the reference's scenes
@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_reference_scenes(R, ctx, spec):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(100, 100, scene)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 1024, 3)
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    for md in (0.0, 0.01 * ext, 1e9):
        want = _check(R, ctx, ps, L, p, md, f"{spec} max_dist={md}")
        if md == 1e9:
            assert (np.diff(want[0]) == L.shape[0]).all()
    md = np.random.default_rng(8).uniform(0.0, 0.02 * ext, 1024).astype(F)
    _check(R, ctx, ps, L, p, md, f"{spec} per-point")
    for margin in (0.0, 1.0, 60.0):
        _check_pairs(R, ctx, ps, L, margin, f"{spec} pairs margin={margin}")
    ps.free()
    scene.free()


def test_floor(R, ctx, floor):
    ps, L = floor
    p = _points(L, 768, 3)
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    for md in (0.0, 0.002 * ext, 30.0):
        want = _check(R, ctx, ps, L, p, md, f"floor max_dist={md}")
    assert np.diff(want[0]).max() > 32                         # (bound 30: rows the capped query cannot return)
    md = np.random.default_rng(8).uniform(0.0, 0.004 * ext, 768).astype(F)
    _check(R, ctx, ps, L, p, md, "floor per-point")
    for margin in (0.0, 1.0):
        pairs, _ = _check_pairs(R, ctx, ps, L, margin, f"floor pairs margin={margin}")
        assert pairs.shape[0] > 1000000


# ---- 2. random scenes of every GPU-builder size class, tall trees, a point cloud, adversarial and huge inputs
@pytest.mark.parametrize("n", [2, 3, 767, 768, 769, 24576, 24577, 131073])
def test_random_scenes(R, ctx, n):
    s = _random_spheres(n, n)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, n)
    for md in (0.0, 3.0) + ((1e9,) if n <= 769 else ()):
        want = _check(R, ctx, ps, L, p, md, f"random:{n} max_dist={md}")
        if md == 1e9:
            assert (np.diff(want[0]) == n).all()
    for margin in (0.0, 1.0) + ((60.0,) if n < 131073 else ()):
        _check_pairs(R, ctx, ps, L, margin, f"random:{n} pairs margin={margin}")
    ps.free()


def test_tall_trees(R, ctx):
    import edge_rays as E
    for what, s, view in (("tall1100", E.SCENES["tall1100"][0], E.SCENES["tall1100"][1:]), ("geometric", _geometric(120, 3), VIEW)):
        ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *view)
        n = s.shape[0]
        assert ps.height > int(np.log2(np.float32(n))) + 2, (what, ps.height)      # partial boxes near the root
        L = ps.bvh_arrays()["L"]
        p = _points(L, 1024, 41)
        rng = np.random.default_rng(43)
        p[:256] = (L[rng.integers(0, n, 256), :3] * rng.uniform(0.5, 1.5, (256, 1))).astype(F)
        for md in (0.0, 0.5, 1e9):
            _check(R, ctx, ps, L, p, md, f"{what} max_dist={md}")
        for margin in (0.0, 1.0, 60.0):
            _check_pairs(R, ctx, ps, L, margin, f"{what} pairs margin={margin}")
        ps.free()


def test_point_cloud(R, ctx):
    rng = np.random.default_rng(5)
    s = np.zeros((5000, 7), F)
    s[:, :3] = rng.normal(0.0, 20.0, (5000, 3))
    s[::7, :3] = s[1::7, :3][: s[::7].shape[0]]     # duplicate centres
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    q = rng.normal(0.0, 25.0, (2048, 3)).astype(F)
    q[:256] = L[rng.integers(0, 5000, 256), :3]
    for md in (1e9, 2.0, 0.0):
        _check(R, ctx, ps, L, q, md, f"cloud max_dist={md}")
    for margin in (0.0, 1.0, 60.0):
        pairs, gap = _check_pairs(R, ctx, ps, L, margin, f"cloud pairs margin={margin}")
        if margin == 0.0:
            assert pairs.shape[0] >= 700 and not gap.any()        # radius 0, margin 0: exactly the coincident centres
    ps.free()


def test_adversarial_inputs(R, ctx):
    rng = np.random.default_rng(17)
    s = _random_spheres(600, 17)
    s[300:400] = s[200:300]                         # duplicate spheres
    s[400:420, 6] = 0.0                             # radius 0
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, 21)
    j = rng.integers(0, 600, 64)
    p[:64] = L[j, :3]
    p[:64, 0] += L[j, 6]                            # exactly on surfaces along x
    p[64:96] = L[rng.integers(0, 600, 32), :3]
    p[96:112] = np.float32(1e8) * rng.normal(size=(16, 3)).astype(F)
    for md in (0.0, 1e9, 2.5):
        _check(R, ctx, ps, L, p, md, f"adversarial max_dist={md}")
    g = P.gaps(L, p[200:201])[0]
    for t in (g[g > 0].min(), np.sort(g[g > 0])[5]):                     # a bound equal to a computed gap, and the float just below it
        for md in (float(t), float(np.nextafter(F(t), F(0)))):
            _check(R, ctx, ps, L, p, md, f"gap-equal max_dist={md!r}")
    q = p.copy()
    q[[1, 2, 3, 4], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    md = np.full(512, 4.0, F)
    bad = [10, 11, 12, 13, 14, 15]
    md[bad] = [np.nan, np.inf, -np.inf, -1.0, 2e9, 1.0000001e9]
    md[20:30] = -0.0
    want = _check(R, ctx, ps, L, q, md, "invalid inputs")
    ln = np.diff(want[0])
    assert not ln[[1, 2, 3, 4] + bad].any() and ln.sum() > 0
    zero = R.spheres_within(ps, q[20:30], 0.0)
    got = R.spheres_within(ps, q, md)
    assert np.array_equal(np.diff(got[0])[20:30], np.diff(zero[0])) and np.array_equal(got[1][got[0][20]:got[0][30]], zero[1])
    for margin in (0.0, 1.0, 60.0):
        _check_pairs(R, ctx, ps, L, margin, f"adversarial pairs margin={margin}")
    ps.free()


def test_huge_coordinates(R, ctx):
    s = _random_spheres(800, 23)
    s[:, :3] *= F(1e16)
    s[:, :3] += F(1e18)
    s[:, 6] *= F(1e16)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, (1e18, 1e18, 2e18), (1e18, 1e18, 1e18), 50.0)
    L = ps.bvh_arrays()["L"]
    p = _points(L, 512, 29)
    for md in (0.0, 1e9):
        _check(R, ctx, ps, L, p, md, f"1e18 max_dist={md}")
    for margin in (0.0, 1.0, 60.0):
        _check_pairs(R, ctx, ps, L, margin, f"1e18 pairs margin={margin}", near=False)
    ps.free()


# ---- 3. a dense case the capped query cannot answer; 6. contact pairs on it, on test_self_contacts's scene, through sphere ids and updates
def test_dense_rows_and_contact_pairs(R, ctx):
    s = _random_spheres(3000, 31, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    ids = ps.sphere_ids()
    L = ps.bvh_arrays()["L"]
    centres, radii = L[:, :3].copy(), L[:, 6].copy()
    bound = radii + F(60)
    want = _check(R, ctx, ps, L, centres, bound, "dense", nearest=False)
    ln = np.diff(want[0])
    assert (ln > 32).sum() >= 1500, (ln > 32).sum()              # at least half the rows are longer than the capped query's k
    cnt = R.nearest_spheres(ps, centres, 32, bound)[0]
    assert np.array_equal(cnt, ln) and cnt.max() > 32
    longest = {}
    for margin in (0.0, 1.0, 20.0, 60.0):
        pairs, gap = _check_pairs(R, ctx, ps, L, margin, f"dense pairs margin={margin}", near=False)
        # the one-sided rule, straight from the definition (no symmetry assumed)
        G = P.gaps(L, centres)
        sel = np.triu(G <= W.contact_bounds(L, margin)[:, None], 1)
        assert np.array_equal(pairs, np.argwhere(sel).astype(np.int32)) and np.array_equal(_bits(gap), _bits(G[sel]))
        longest[margin] = int(np.bincount(pairs[:, 0], minlength=3000).max())
    assert longest[60.0] > 32
    # test_self_contacts's query at margin 0: the pairs are the j > i entries of nearest_spheres's rows, exactly
    cnt, idx, ngap = R.nearest_spheres(ps, centres, 32, radii)
    assert cnt.max() <= 32
    pairs, gap = R.contact_pairs(ps, 0.0)
    rows = [(i, int(j), ngap[i, s]) for i in range(3000) for s, j in enumerate(idx[i, : cnt[i]]) if j > i]
    rows.sort(key=lambda t: (t[0], t[1]))
    assert pairs.tolist() == [[i, j] for i, j, _ in rows]
    assert np.array_equal(_bits(gap), _bits(np.array([g for _, _, g in rows], F)))
    # mapped through the sphere ids: the brute force in the caller's order (with the lower L index as the one whose bound is used)
    Gs = P.gaps(s, s[:, :3])
    got = {(int(ids[i]), int(ids[j])) for i, j in pairs}
    assert all(Gs[a, b] <= s[a, 6] for a, b in got) and len(got) == pairs.shape[0]
    pos = np.empty(3000, np.int64)
    pos[ids] = np.arange(3000)
    want_set = {(a, b) for a, b in zip(*np.nonzero(Gs <= s[:, 6][:, None])) if pos[a] < pos[b]}
    # (few: test_self_contacts's scene is sparse at margin 0 -- its own `> 3000` counts the 3000 self pairs and both directions)
    assert got == want_set and len(got) > 0
    # after update_spheres with moved spheres: the pairs of a freshly prepared scene
    s2 = s.copy()
    s2[:, :3] += np.random.default_rng(77).normal(0.0, 1.5, (3000, 3)).astype(F)
    ps.update_spheres(s2)
    fresh = R.prepare_scene_from_spheres(ctx, s2, 64, 64, *VIEW)
    L2 = fresh.bvh_arrays()["L"]
    assert ps.bvh_arrays()["L"].tobytes() == L2.tobytes()
    for margin in (0.0, 1.0):
        a, b = R.contact_pairs(ps, margin), R.contact_pairs(fresh, margin)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        w = W.contact_pairs(L2, margin)
        assert np.array_equal(a[0], w[0]) and np.array_equal(_bits(a[1]), _bits(w[1]))
        assert not np.array_equal(a[0], W.contact_pairs(L, margin)[0])
    fresh.free()
    ps.free()


# ---- 5. the lower index bound
def test_first(R, ctx):
    s = _random_spheres(5000, 55, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    n, m = 5000, 1024
    p = _points(L, m, 7)
    rng = np.random.default_rng(3)
    first = rng.integers(-10, n + 10, m)
    first[:6] = [0, -1, -(2 ** 31), n, n + 1, 2 ** 31 - 1]
    for md in (8.0, rng.uniform(0.0, 12.0, m).astype(F)):
        off, idx, gap = R.spheres_within(ps, p, md)
        got = R.spheres_within(ps, p, md, first=first)
        assert ctx.last_launch == "family=within fill" + (" (per-point)" if np.ndim(md) else "") + " first"
        _same(got, W.within(L, p, md, first), "first")
        foff, fidx, fgap = got
        for i in range(m):                                       # a row with first = f: the unfiltered row's entries with j >= f
            row, g = idx[off[i]:off[i + 1]], gap[off[i]:off[i + 1]]
            keep = row >= first[i]
            assert np.array_equal(fidx[foff[i]:foff[i + 1]], row[keep]) and np.array_equal(_bits(fgap[foff[i]:foff[i + 1]]), _bits(g[keep])), i
        assert np.array_equal(np.diff(foff)[:3], np.diff(off)[:3]) and not np.diff(foff)[3:6].any()
    import torch
    ft = torch.as_tensor(first.astype(np.int32), device="cuda")
    pt = torch.as_tensor(p, device="cuda")
    _same(R.spheres_within(ps, pt, 8.0, first=ft), W.within(L, p, 8.0, first), "first as a device tensor")
    ps.free()


# ---- 7. 64-bit offsets and the capacity guard
def test_offsets_past_32_bits_and_capacity(R, ctx, floor):
    from raytracers_amd._lib import lib
    ps, L = floor
    n = 1000000
    m2 = 4352
    p = _points(L, m2, 13)
    pts = R.api.DeviceBuffer(ctx, 12 * m2)
    off = R.api.DeviceBuffer(ctx, 8 * (m2 + 1))
    cap, guard = 2 * n, 4096
    idx = R.api.DeviceBuffer(ctx, 4 * (cap + guard))
    gap = R.api.DeviceBuffer(ctx, 4 * (cap + guard))
    row = R.api.DeviceBuffer(ctx, 4 * (cap + guard))
    try:
        ctx._check(lib.rt_copy_to_device(ctx._h, C.c_void_p(pts.ptr), p.ctypes.data, p.nbytes))
        for m in (4096, m2):
            R.spheres_within_count_into(pts.ptr, m, ps, off.ptr, 1e9)
            assert ctx.last_launch == "family=within count"
            o = off.to_host((m + 1,), np.int64)
            assert np.array_equal(o, np.arange(m + 1, dtype=np.int64) * n), m    # every row is the whole scene
            assert o[m] == m * n and o[m] > 1 << 31
        assert o[m2] > 1 << 32
        # the same 4 096-point query filled into 2 * 10^6 entries: the first two rows, nothing beyond
        m = 4096
        R.spheres_within_count_into(pts.ptr, m, ps, off.ptr, 1e9)
        sentinel = np.full(cap + guard, 0x5A5A5A5A, np.int32)
        for b in (idx, gap, row):
            ctx._check(lib.rt_copy_to_device(ctx._h, C.c_void_p(b.ptr), sentinel.ctypes.data, sentinel.nbytes))
        R.spheres_within_fill_into(pts.ptr, m, ps, off.ptr, cap, idx.ptr, gap.ptr, row.ptr, 1e9)
        assert ctx.last_launch == "family=within fill"
        gi, gg, gr = idx.to_host((cap + guard,)), gap.to_host((cap + guard,), F), row.to_host((cap + guard,))
        assert np.array_equal(gi[:cap], np.tile(np.arange(n, dtype=np.int32), 2))
        assert np.array_equal(gr[:cap], np.repeat(np.arange(2, dtype=np.int32), n))
        assert np.array_equal(_bits(gg[:cap]), _bits(P.gaps(L, p[:2]).reshape(-1)))
        for g in (gi, gg.view(np.int32), gr):
            assert (g[cap:] == 0x5A5A5A5A).all()                                  # the sentinels are untouched
    finally:
        for b in (pts, off, idx, gap, row):
            b.free()


# ---- 8. refusals, launch strings, n == 0, repeatability, torch outputs
def test_refusals_and_launch(R, ctx):
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    n = ps.num_spheres
    vp = C.c_void_p
    pts = R.api.DeviceBuffer(ctx, 12 * 64)
    md = R.api.DeviceBuffer(ctx, 4 * 64)
    fi = R.api.DeviceBuffer(ctx, 4 * 64)
    off = R.api.DeviceBuffer(ctx, 8 * (max(n, 64) + 1))
    out = R.api.DeviceBuffer(ctx, 8 * 4096)
    try:
        mark_off = np.full(max(n, 64) + 1, -7, np.int64)
        mark_out = np.full(2 * 4096, 0x5A5A5A5A, np.int32)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(off.ptr), mark_off.ctypes.data, mark_off.nbytes))
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(out.ptr), mark_out.ctypes.data, mark_out.nbytes))
        zeros = np.zeros(64 * 3, F)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(pts.ptr), zeros.ctypes.data, zeros.nbytes))
        R.nearest_spheres(ps, np.zeros((5, 3), F), 5, 1.0)
        before = ctx.last_launch
        assert before == "family=nearest k=5"
        h, p, o, f = ctx._h, ps._h, vp(off.ptr), vp(out.ptr)
        nan, inf = float("nan"), float("inf")
        bad = [
            lib.rt_spheres_within_count(h, None, 64, vp(pts.ptr), 1.0, None, None, o),
            lib.rt_spheres_within_count(h, p, -1, vp(pts.ptr), 1.0, None, None, o),
            lib.rt_spheres_within_count(h, p, 1 << 31, vp(pts.ptr), 1.0, None, None, o),
            lib.rt_spheres_within_count(h, p, 64, None, 1.0, None, None, o),
            lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), 1.0, None, None, None),
            lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), -1.0, None, None, o),
            lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), nan, None, None, o),
            lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), inf, None, None, o),
            lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), 2e9, None, vp(fi.ptr), o),
            lib.rt_spheres_within_fill(h, None, 64, vp(pts.ptr), 1.0, None, None, o, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, -1, vp(pts.ptr), 1.0, None, None, o, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, 1 << 31, vp(pts.ptr), 1.0, None, None, o, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, 64, None, 1.0, None, None, o, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, 64, vp(pts.ptr), 1.0, None, None, None, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, 64, vp(pts.ptr), 1.0, None, None, o, -1, f, None, None),
            lib.rt_spheres_within_fill(h, p, 64, vp(pts.ptr), 1.0, None, None, o, 4096, None, None, None),
            lib.rt_spheres_within_fill(h, p, 64, vp(pts.ptr), nan, None, None, o, 4096, f, None, None),
            lib.rt_spheres_within_fill(h, p, 64, vp(pts.ptr), -0.5, None, None, o, 4096, None, f, None),
            lib.rt_contact_pairs_count(h, None, 0.0, o),
            lib.rt_contact_pairs_count(h, p, 0.0, None),
            lib.rt_contact_pairs_count(h, p, -1.0, o),
            lib.rt_contact_pairs_count(h, p, nan, o),
            lib.rt_contact_pairs_count(h, p, inf, o),
            lib.rt_contact_pairs_count(h, p, 2e9, o),
            lib.rt_contact_pairs_fill(h, None, 0.0, o, 4096, f, None),
            lib.rt_contact_pairs_fill(h, p, 0.0, None, 4096, f, None),
            lib.rt_contact_pairs_fill(h, p, 0.0, o, -1, f, None),
            lib.rt_contact_pairs_fill(h, p, 0.0, o, 4096, None, None),
            lib.rt_contact_pairs_fill(h, p, nan, o, 4096, f, None),
        ]
        for i, rc in enumerate(bad):
            assert rc != 0, i
            assert lib.rt_last_error(h).decode(), i
        assert ctx.last_launch == before                                      # every refusal leaves the launch string ...
        assert np.array_equal(off.to_host(mark_off.shape, np.int64), mark_off)   # ... and the outputs untouched
        assert np.array_equal(out.to_host(mark_out.shape), mark_out)
        with pytest.raises(R.RtError):
            R.spheres_within(ps, np.zeros((4, 3), F), -0.5)
        with pytest.raises(R.RtError):
            R.contact_pairs(ps, float("nan"))
        # a scalar max_dist is ignored when per-point bounds are given
        ones = np.ones(64, F)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(md.ptr), ones.ctypes.data, ones.nbytes))
        assert lib.rt_spheres_within_count(h, p, 64, vp(pts.ptr), nan, vp(md.ptr), None, o) == 0
        assert ctx.last_launch == "family=within count (per-point)"
        # n == 0: offsets[0] = 0 is still written
        assert lib.rt_spheres_within_count(h, p, 0, vp(pts.ptr), 1.0, None, None, o) == 0
        assert off.to_host((1,), np.int64)[0] == 0
        assert lib.rt_spheres_within_fill(h, p, 0, vp(pts.ptr), 1.0, None, None, o, 0, f, None, None) == 0
        e = R.spheres_within(ps, np.zeros((0, 3), F), 1.0, rows=True)
        assert e[0].tolist() == [0] and e[1].shape == (0,) and e[2].shape == (0,) and e[3].shape == (0,)
        # the launch strings under every variant
        for v in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(v)
            zi = np.zeros(64, np.int32)
            ctx._check(lib.rt_copy_to_device(ctx._h, vp(fi.ptr), zi.ctypes.data, zi.nbytes))
            for mdp, fip, tail in ((None, None, ""), (md.ptr, None, " (per-point)"), (None, fi.ptr, " first"), (md.ptr, fi.ptr, " (per-point) first")):
                R.spheres_within_count_into(pts.ptr, 64, ps, off.ptr, 1.0, mdp, fip)
                assert ctx.last_launch == "family=within count" + tail
                R.spheres_within_fill_into(pts.ptr, 64, ps, off.ptr, 4096, out.ptr, None, None, 1.0, mdp, fip)
                assert ctx.last_launch == "family=within fill" + tail
            R.contact_pairs_count_into(ps, off.ptr, 0.5)
            assert ctx.last_launch == "family=within count self"
            R.contact_pairs_fill_into(ps, off.ptr, 4096, out.ptr, None, 0.5)
            assert ctx.last_launch == "family=within fill self"
            R.contact_pairs_fill_into(ps, off.ptr, 4096, None, out.ptr, 0.5)   # only the gaps
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        for b in (pts, md, fi, off, out):
            b.free()
        ps.free()
        scene.free()


def test_repeatable_and_torch_outputs(R):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = R.Context(0, stream=stream.cuda_stream)
        try:
            s = _random_spheres(20000, 91, 0.5, 3.0)
            ps = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            L = ps.bvh_arrays()["L"]
            p = _points(L, 4096, 5)
            a, b = R.spheres_within(ps, p, 6.0, rows=True), R.spheres_within(ps, p, 6.0, rows=True)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            a, b = R.contact_pairs(ps, 2.0), R.contact_pairs(ps, 2.0)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            # outputs allocated by torch on the context's stream, in place
            want = W.within_near(L, p, 6.0)
            pt = torch.as_tensor(p, device="cuda")
            off = torch.empty(4097, dtype=torch.int64, device="cuda")
            R.spheres_within_count_into(pt.data_ptr(), 4096, ps, off.data_ptr(), 6.0)
            total = int(off[4096].item())
            assert total == want[0][-1]
            idx = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            gap = torch.full((total + 64,), -3.0, dtype=torch.float32, device="cuda")
            row = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            R.spheres_within_fill_into(pt.data_ptr(), 4096, ps, off.data_ptr(), total, idx.data_ptr(), gap.data_ptr(), row.data_ptr(), 6.0)
            stream.synchronize()
            _same((off.cpu().numpy(), idx[:total].cpu().numpy(), gap[:total].cpu().numpy()), want, "torch outputs")
            assert np.array_equal(row[:total].cpu().numpy(), np.repeat(np.arange(4096, dtype=np.int32), np.diff(want[0])))
            assert (idx[total:] == -3).all() and (gap[total:] == -3.0).all() and (row[total:] == -3).all()
            wp = W.contact_pairs(L, 2.0, near=True)
            off2 = torch.empty(20001, dtype=torch.int64, device="cuda")
            R.contact_pairs_count_into(ps, off2.data_ptr(), 2.0)
            tot2 = int(off2[20000].item())
            assert tot2 == wp[0].shape[0]
            pair = torch.full((tot2 + 8, 2), -3, dtype=torch.int32, device="cuda")
            R.contact_pairs_fill_into(ps, off2.data_ptr(), tot2, pair.data_ptr(), None, 2.0)
            stream.synchronize()
            assert np.array_equal(pair[:tot2].cpu().numpy(), wp[0]) and (pair[tot2:] == -3).all()
            ps.free()
        finally:
            c.close()
