"""Along-ray queries on the GPU: rt_spheres_along_rays_count / _fill against the numpy restatement (along_ref.py) -- offsets, index, start bits
and root bits with == (NaN roots match as "both NaN"; -0.0 and +0.0 are told apart) -- on the reference's scenes with scalar and per-query
values mixed, through the library's own capped queries on both sides (sweep_spheres and multi_hit_rays at k = 32 via row_contacts and
row_crossings), on a scene's self-sweep, the edge families of edge_sweeps.py, a tall tree whose answer is the tree's and not the brute
force's, a 30 000-sphere scene through every way to prepare it, the capacity guard, unaligned pointers, every refusal with its message (a multi-device context among them), n == 0, repeatability,
outputs allocated by torch and device-tensor inputs."""
import ctypes as C
import functools

import numpy as np
import pytest

import along_ref as A
import edge_sweeps as ES
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q
from test_along_cpu import INTERVALS, KMAX, invalid_values
from test_proximity_gpu import VIEW, _random_spheres

pytestmark = pytest.mark.gpu

F = np.float32
NRAYS = 512
POISON = 0x5A5A5A5A


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
    """offsets, index, roots, start of `got` against `want`: ==, on the bits of the roots, except that a NaN matches a NaN"""
    for name, g, w in zip(("offsets", "index", "roots", "start"), got, want):
        if g is None and name == "roots":
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        differ = _bits(g) != _bits(w)
        if name == "roots":
            differ &= ~(np.isnan(g) & np.isnan(w))
        bad = np.nonzero(differ.reshape(differ.shape[0], int(np.prod(differ.shape[1:]))).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


def _radii(arr):
    r0 = float(np.median(arr["L"][:, 6]))
    return {"zero": 0.0, "neg_zero": -0.0, "median": r0, "four_medians": 4.0 * r0}


def _reference(R, ctx, spec):
    scene = ctx.floor(37, 222.0) if spec == "floor" else ctx.scene(spec)
    ps = R.prepare_scene(64, 64, scene)
    arr = ps.bvh_arrays()
    seed = {"rgbbox": 17, "irreg": 29, "floor": 41}[spec]
    return scene, ps, arr, Q.RefScene(arr), X.seeded_rays(arr, NRAYS, seed)


def _tail(per_query=False, exclude=False, first=False):
    return (" (per-query)" if per_query else "") + (" exclude" if exclude else "") + (" first" if first else "")


# ---- 1. the reference's scenes: every radius and interval, scalar and per-query values mixed, the optional outputs, the launch strings
@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "floor"])
def test_reference_scenes(R, ctx, spec):
    scene, ps, arr, ref, rays = _reference(R, ctx, spec)
    o, d = rays[:, :3], rays[:, 3:]
    radii = _radii(arr)
    for rname, radius in radii.items():
        for t_min, t_max in INTERVALS:
            want = A.along(ref, o, d, radius, t_min, t_max)
            got = R.spheres_along_rays(ps, rays, radius, t_min, t_max)
            assert ctx.last_launch == ("family=along fill" if want[0][-1] else "family=along count"), ctx.last_launch
            _same(got, want, f"{spec} {rname} ({t_min}, {t_max})")
    # per-query values with -0.0, NaN, negative, reversed and 2e9 entries; a scalar next to an array is broadcast
    lo, hi, rq, bad = invalid_values(NRAYS, radii["median"])
    rq[~bad] = np.random.default_rng(4).choice(np.array([0.0, radii["median"], radii["four_medians"]], F), int((~bad).sum()))
    rq[2::37] = -0.0
    want = A.along(ref, o, d, rq, lo, hi)
    assert want[0][-1] > NRAYS and not np.diff(want[0])[bad].any()
    got = R.spheres_along_rays(ps, rays, rq, lo, hi)
    assert ctx.last_launch == "family=along fill (per-query)"
    _same(got, want, f"{spec} per-query")
    for args in ((rq, 0.1, 30.0), (radii["median"], lo, hi), (radii["median"], lo, 30.0), (rq, 0.0, hi)):
        _same(R.spheres_along_rays(ps, rays, *args), A.along(ref, o, d, *args), f"{spec} mixed scalars and arrays")
        assert ctx.last_launch == "family=along fill (per-query)"
    # without roots, with rows
    o2, i2, r2, s2, q2 = R.spheres_along_rays(ps, rays, rq, lo, hi, roots=False, rows=True)
    assert r2 is None
    _same((o2, i2, None, s2), want, f"{spec} roots=False")
    assert q2.dtype == np.int32 and np.array_equal(q2, np.repeat(np.arange(NRAYS, dtype=np.int32), np.diff(want[0])))
    res = R.spheres_along_rays(ps, rays, rq, lo, hi, rows=True)
    _same(res[:4], want, f"{spec} rows=True")
    assert np.array_equal(res[4], q2)
    ps.free()
    scene.free()


# ---- 2. the identities through the library on both sides
@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "floor"])
def test_identities_through_the_library(R, ctx, spec):
    scene, ps, arr, ref, rays = _reference(R, ctx, spec)
    radii = _radii(arr)
    for rname, radius in radii.items():
        for t_min, t_max in INTERVALS:
            off, idx, roots, start = R.spheres_along_rays(ps, rays, radius, t_min, t_max)
            cnt, sidx, sstart, shit = R.sweep_spheres(ps, rays, radius, KMAX, t_min, t_max)
            what = f"{spec} {rname} ({t_min}, {t_max})"
            n = np.diff(off)
            assert np.array_equal(n, cnt), what                                                    # identity 1
            got = R.row_contacts(off, idx, roots, start, t_min, KMAX)                               # identity 2 (and the first 32 of longer rows)
            for g, w, part in zip(got[1:], (sidx, sstart, shit[:, :, 0]), ("index", "start", "tau")):
                assert np.array_equal(_bits(g), _bits(np.ascontiguousarray(w))), f"{what}: {part}"
            if rname == "four_medians" and t_max == 1e9:
                short, long_ = (n > 0) & (n <= KMAX), n > KMAX
                print(f"{spec}: {short.mean():.1%} rows of 1..32 entries, {long_.mean():.1%} above 32, longest {n.max()}")
                assert short.mean() >= 0.25 and long_.mean() >= 0.25, (short.mean(), long_.mean())
            if rname in ("zero", "neg_zero"):                                                      # identity 3
                mc, mi, mr, mh = R.multi_hit_rays(ps, rays, KMAX, t_min, t_max)
                c3, i3, r3, t3 = R.row_crossings(off, idx, roots, t_min, t_max, KMAX)
                assert np.array_equal(c3, mc) and np.array_equal(i3, mi) and np.array_equal(r3, mr), what
                assert np.array_equal(_bits(t3), _bits(np.ascontiguousarray(mh[:, :, 0]))), what
    # per-query values on both sides
    lo, hi, rq, bad = invalid_values(NRAYS, radii["four_medians"])
    off, idx, roots, start = R.spheres_along_rays(ps, rays, rq, lo, hi)
    cnt, sidx, sstart, shit = R.sweep_spheres(ps, rays, rq, KMAX, lo, hi)
    assert np.array_equal(np.diff(off), cnt) and not cnt[bad].any()
    got = R.row_contacts(off, idx, roots, start, lo, KMAX)
    for g, w in zip(got[1:], (sidx, sstart, shit[:, :, 0])):
        assert np.array_equal(_bits(g), _bits(np.ascontiguousarray(w)))
    ps.free()
    scene.free()


# ---- 3. a scene sweeps its own spheres
def test_self_sweep(R, ctx):
    rng = np.random.default_rng(7)
    s = np.zeros((3000, 7), F)
    s[:, 0:3] = rng.uniform(-30, 30, (3000, 3))
    s[:, 3:6] = rng.uniform(0.1, 0.9, (3000, 3))
    s[:, 6] = rng.uniform(0.2, 1.5, 3000)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, (0.0, 0.0, 90.0), (0.0, 0.0, 0.0), 60.0)
    arr = ps.bvh_arrays()
    L = arr["L"]
    n = L.shape[0]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rays = np.concatenate([L[:, :3], u * L[:, 6:7]], axis=1).astype(F)          # a displacement of one radius over (0, 1)
    me = np.arange(n)
    ref = Q.RefScene(arr)
    want = A.along(ref, rays[:, :3], rays[:, 3:], L[:, 6], 0.0, 1.0, exclude=me)
    got = R.spheres_along_rays(ps, rays, L[:, 6].copy(), 0.0, 1.0, exclude=me, rows=True)
    assert ctx.last_launch == "family=along fill (per-query) exclude"
    _same(got[:4], want, "self-sweep")
    assert want[0][-1] > n // 4 and not (got[1] == got[4]).any(), "a query reports itself"
    # every pair once: first = i + 1 keeps the j > i of every row
    want2 = A.along(ref, rays[:, :3], rays[:, 3:], L[:, 6], 0.0, 1.0, exclude=me, first=me + 1)
    got2 = R.spheres_along_rays(ps, rays, L[:, 6].copy(), 0.0, 1.0, exclude=me, first=me + 1, rows=True)
    assert ctx.last_launch == "family=along fill (per-query) exclude first"
    _same(got2[:4], want2, "self-sweep first = i + 1")
    keep = got[1] > got[4]
    assert 0 < keep.sum() < keep.size and np.array_equal(got2[1], got[1][keep]) and np.array_equal(got2[4], got[4][keep])
    assert np.array_equal(_bits(got2[2]), _bits(got[2][keep])) and np.array_equal(got2[3], got[3][keep])
    ps.free()


# ---- 4. the edge families on their degenerate scenes, the non-finite rays of edge_rays.py among them; 5. the tall tree
@functools.lru_cache(maxsize=None)
def _edge_inputs(name):
    s, lf, la, fov = ES.SCENES[name]
    arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    fam = ES.sweep_families(arr, seed=1)
    return (arr, ref, fam) + ES.joined(fam)


def _edge_prepared(R, ctx, name):
    s, lf, la, fov = ES.SCENES[name]
    arr = _edge_inputs(name)[0]
    scene = ctx.scene_from_spheres(s, lf, la, fov)
    ps = R.prepare_scene(64, 64, scene)
    got = ps.bvh_arrays()
    for k in ("left", "right", "parent"):
        assert (got[k] == arr[k]).all(), (name, k)
    for k in ("L", "bmin", "bmax"):
        assert got[k].tobytes() == arr[k].tobytes(), (name, k)
    return scene, ps


@pytest.mark.parametrize("name", list(ES.SCENES))
def test_edge_families(R, ctx, name):
    arr, ref, fam, rays, rq, lo, hi, label = _edge_inputs(name)
    o, d = rays[:, :3], rays[:, 3:]
    scene, ps = _edge_prepared(R, ctx, name)
    want = A.along(ref, o, d, rq, lo, hi)
    got = R.spheres_along_rays(ps, rays, rq, lo, hi)
    n = np.diff(want[0])
    try:
        _same(got, want, name)
    except AssertionError:
        for i, f in enumerate(fam):                       # again family by family, so that the failure names the family
            m = label == i
            _same(R.spheres_along_rays(ps, rays[m], rq[m], lo[m], hi[m]), A.along(ref, o[m], d[m], rq[m], lo[m], hi[m]), f"{name} [{f}]")
        raise
    names = list(fam)
    absorbed = label == names.index("absorbed")
    assert n[absorbed].max() == ref.n, "no query of `absorbed` selects every sphere"
    assert not n[label == names.index("stationary")].any()
    assert np.isnan(rays).any() and np.isinf(rays).any()
    if name == "tall1100":
        # the top boxes of this tree are partial: the answer is the tree's (the restatement's), and the brute force has more on some query
        brute = A.along_brute(ref, o, d, rq, lo, hi)
        differ = np.diff(brute[0]) != n
        print(f"tall1100: the brute force differs on {int(differ.sum())} queries, {int(brute[0][-1] - want[0][-1])} entries")
        assert differ.sum() >= 1 and ps.height > int(np.log2(np.float32(ref.n))) + 2
        assert not np.array_equal(np.diff(got[0]), np.diff(brute[0]))
    # with excludes and first bounds under the same edges
    rng = np.random.default_rng(12)
    ex = np.where(n > 0, want[1][np.minimum(want[0][:-1] + (rng.random(n.size) * n).astype(np.int64), want[1].size - 1)], -1)
    fi = rng.integers(-3, ref.n + 3, n.size)
    _same(R.spheres_along_rays(ps, rays, rq, lo, hi, exclude=ex, first=fi), A.along(ref, o, d, rq, lo, hi, exclude=ex, first=fi),
          f"{name} exclude and first")
    assert ctx.last_launch == "family=along fill (per-query) exclude first"
    ps.free()
    scene.free()


# ---- 6. a 30 000-sphere scene through both builders, prepare_scene_from_spheres and update_spheres; one row that holds the whole scene
def test_large_scene_every_builder(R):
    n, m = 30000, 256
    s = _random_spheres(n, 71)
    s[29000:29100, :3] = s[0, :3]                                             # equal Morton keys
    other = _random_spheres(n, 72)
    wants = {}
    checked = 0
    for gpu_build in (1, 0):
        c = R.Context(0)
        c.set_option("gpu_build", gpu_build)
        try:
            sc = c.scene_from_spheres(s, *VIEW)
            a = R.prepare_scene(64, 64, sc)
            b = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            u = R.prepare_scene_from_spheres(c, other, 64, 64, *VIEW)
            u.update_spheres(s)
            for ps in (a, b, u):
                arr = ps.bvh_arrays()
                key = b"".join(np.ascontiguousarray(arr[k]).tobytes() for k in ("L", "bmin", "bmax", "left", "right"))
                if key not in wants:
                    rays = X.seeded_rays(arr, m, 9)
                    rays[:8, :3] = arr["L"][29000, :3]                        # from the coincident run
                    rq = np.random.default_rng(5).uniform(0.0, 40.0, m).astype(F)
                    rq[0] = 1e9                                               # every widened box and every R holds the origin
                    wants[key] = (rays, rq, A.along_walk(arr, rays[:, :3], rays[:, 3:], rq, 0.0, 1e9))
                rays, rq, want = wants[key]
                assert want[0][1] == n and np.array_equal(want[1][:n], np.arange(n, dtype=np.int32)) and want[3][:n].all()
                assert np.diff(want[0])[1:].max() > KMAX
                _same(R.spheres_along_rays(ps, rays, rq, 0.0, 1e9), want, f"30000 spheres gpu_build={gpu_build}")
                checked += 1
                ps.free()
            sc.free()
        finally:
            c.close()
    assert checked == 6


# ---- 7. the capacity guard, foreign and negative offsets: nothing is written outside [0, capacity)
def test_capacity_guard_and_foreign_offsets(R, ctx):
    import torch
    scene, ps, arr, ref, rays = _reference(R, ctx, "irreg")
    radius = _radii(arr)["four_medians"]
    want = A.along(ref, rays[:, :3], rays[:, 3:], radius, 0.0, 1e9)
    total, guard = int(want[0][-1]), 4096
    rd = torch.from_numpy(rays).cuda()
    off = torch.from_numpy(want[0]).cuda()
    row = np.repeat(np.arange(NRAYS, dtype=np.int32), np.diff(want[0]))

    def fill(offsets, capacity):
        bufs = [torch.full((total + guard,), POISON, dtype=torch.int32, device="cuda"),
                torch.full((total + guard, 2), POISON, dtype=torch.int32, device="cuda"),
                torch.full((total + guard,), 0xAB, dtype=torch.uint8, device="cuda"),
                torch.full((total + guard,), POISON, dtype=torch.int32, device="cuda")]
        torch.cuda.synchronize()
        R.spheres_along_rays_fill_into(rd.data_ptr(), NRAYS, ps, offsets.data_ptr(), capacity, *[t.data_ptr() for t in bufs], radius=radius,
                                       t_min=0.0, t_max=1e9)
        ctx.sync()
        return [t.cpu().numpy() for t in bufs]

    for cap in (total, total // 2 + 3, 1, 0):
        gi, gr, gs, gq = fill(off, cap)
        assert np.array_equal(gi[:cap], want[1][:cap]) and np.array_equal(gr[:cap].view(np.uint32), _bits(want[2][:cap])), cap
        assert np.array_equal(gs[:cap], want[3][:cap]) and np.array_equal(gq[:cap], row[:cap]), cap
        assert (gi[cap:] == POISON).all() and (gr[cap:] == POISON).all() and (gs[cap:] == 0xAB).all() and (gq[cap:] == POISON).all(), cap
    # foreign offsets: another query's, shifted, reversed, negative, huge -- entries may be misplaced, never outside [0, capacity)
    rng = np.random.default_rng(2)
    foreign = [np.concatenate([[0], np.cumsum(rng.integers(0, 9, NRAYS))]), want[0] + 1000, want[0][::-1].copy(), want[0] - total // 2,
               np.full(NRAYS + 1, -1), np.where(np.arange(NRAYS + 1) % 2 == 0, -(2 ** 62), 2 ** 62),
               np.where(np.arange(NRAYS + 1) % 3 == 0, 0, total + guard // 2)]
    cap = total // 2
    for k, f in enumerate(foreign):
        gi, gr, gs, gq = fill(torch.from_numpy(np.ascontiguousarray(f, dtype=np.int64)).cuda(), cap)
        assert (gi[cap:] == POISON).all() and (gr[cap:] == POISON).all() and (gs[cap:] == 0xAB).all() and (gq[cap:] == POISON).all(), k
        written = gi[:cap] != POISON
        assert ((gi[:cap][written] >= 0) & (gi[:cap][written] < ref.n)).all(), k
        if k == 4:
            assert not written.any(), "a negative offsets[i] wrote something"
    ps.free()
    scene.free()


# ---- 8. unaligned pointers: every 4-byte array 4 bytes into its allocation, the start flags 1 byte; offsets 8 bytes (aligned for their type)
def test_unaligned_pointers(R, ctx):
    import torch
    scene, ps, arr, ref, rays_np = _reference(R, ctx, "rgbbox")
    radii = _radii(arr)
    lo_np, hi_np, rq_np, _ = invalid_values(NRAYS, radii["four_medians"])
    rng = np.random.default_rng(6)
    ex_np, fi_np = rng.integers(-1, ref.n, NRAYS).astype(np.int32), rng.integers(-1, ref.n // 2, NRAYS).astype(np.int32)
    want = A.along(ref, rays_np[:, :3], rays_np[:, 3:], rq_np, lo_np, hi_np, exclude=ex_np, first=fi_np)
    total = int(want[0][-1])
    assert total > NRAYS

    def shifted(a, fill=0):
        flat = np.ascontiguousarray(a).reshape(-1)
        t = torch.full((flat.size + 1,), fill, dtype=torch.from_numpy(flat[:1].copy()).dtype, device="cuda")[1:]
        t.copy_(torch.from_numpy(flat))
        return t

    rays, rq, lo, hi, ex, fi = (shifted(a) for a in (rays_np, rq_np, lo_np, hi_np, ex_np, fi_np))
    for t in (rays, rq, lo, hi, ex, fi):
        assert t.data_ptr() % 8 == 4
    off = torch.full((NRAYS + 2,), -7, dtype=torch.int64, device="cuda")[1:]
    assert off.data_ptr() % 16 == 8
    kw = dict(radius_ptr=rq.data_ptr(), t_min_ptr=lo.data_ptr(), t_max_ptr=hi.data_ptr(), exclude_ptr=ex.data_ptr(), first_ptr=fi.data_ptr())
    torch.cuda.synchronize()
    R.spheres_along_rays_count_into(rays.data_ptr(), NRAYS, ps, off.data_ptr(), **kw)
    ctx.sync()
    assert np.array_equal(off.cpu().numpy(), want[0])
    idx, qry = shifted(np.full(total, -7, np.int32)), shifted(np.full(total, -7, np.int32))
    roots = shifted(np.full((total, 2), -7.0, F))
    start = shifted(np.full(total, 0xAB, np.uint8))
    assert idx.data_ptr() % 8 == 4 and roots.data_ptr() % 8 == 4 and start.data_ptr() % 2 == 1
    torch.cuda.synchronize()
    R.spheres_along_rays_fill_into(rays.data_ptr(), NRAYS, ps, off.data_ptr(), total, idx.data_ptr(), roots.data_ptr(), start.data_ptr(),
                                   qry.data_ptr(), **kw)
    ctx.sync()
    _same((off.cpu().numpy(), idx.cpu().numpy(), roots.cpu().numpy().reshape(-1, 2), start.cpu().numpy()), want, "unaligned")
    assert np.array_equal(qry.cpu().numpy(), np.repeat(np.arange(NRAYS, dtype=np.int32), np.diff(want[0])))
    ps.free()
    scene.free()


# ---- 9. refusals, n == 0, repeatability, torch outputs, device-tensor inputs
def test_refusals_and_launch_strings(R, ctx):
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    vp = C.c_void_p
    rays = R.api.DeviceBuffer(ctx, 24 * 64)
    val = R.api.DeviceBuffer(ctx, 4 * 64)
    ind = R.api.DeviceBuffer(ctx, 4 * 64)
    off = R.api.DeviceBuffer(ctx, 8 * 65)
    out = R.api.DeviceBuffer(ctx, 8 * 4096)
    try:
        mark_off = np.full(65, -7, np.int64)
        mark_out = np.full(2 * 4096, POISON, np.int32)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(off.ptr), mark_off.ctypes.data, mark_off.nbytes))
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(out.ptr), mark_out.ctypes.data, mark_out.nbytes))
        some = X.seeded_rays(ps.bvh_arrays(), 64, 3)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(rays.ptr), some.ctypes.data, some.nbytes))
        ones, zi = np.ones(64, F), np.zeros(64, np.int32)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(val.ptr), ones.ctypes.data, ones.nbytes))
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(ind.ptr), zi.ctypes.data, zi.nbytes))
        R.sweep_spheres(ps, some[:5], 1.0, 5)
        before = ctx.last_launch
        assert before == "family=sweep k=5"
        h, p, r, o, f, v = ctx._h, ps._h, vp(rays.ptr), vp(off.ptr), vp(out.ptr), vp(val.ptr)
        nan, inf = float("nan"), float("inf")
        cnt, fil = lib.rt_spheres_along_rays_count, lib.rt_spheres_along_rays_fill
        q = (1.0, None, 0.0, 1.0, None, None, None, None)             # radius, radius_dev, t_min, t_max, t_min_dev, t_max_dev, exclude, first
        cn, fn = "rt_spheres_along_rays_count", "rt_spheres_along_rays_fill"
        count_text, rays_text, off_text = ": query count out of range: 0 <= n < 2^31", ": null rays pointer", ": null offsets pointer"
        radius_text, interval_text = ": need 0 <= radius <= 1e9, finite", ": need 0 <= t_min <= t_max <= 1e9, both finite"
        pair_text = ": t_min_dev and t_max_dev must both be NULL or both be given"
        ft = (o, 4096, f, None, None, None)                           # offsets, capacity, index, roots, start, query
        bad = [
            (lambda: cnt(h, None, 64, r, *q, o), "null prepared scene"),
            (lambda: cnt(h, p, -1, r, *q, o), cn + count_text),
            (lambda: cnt(h, p, 1 << 31, r, *q, o), cn + count_text),
            (lambda: cnt(h, p, 64, None, *q, o), cn + rays_text),
            (lambda: cnt(h, p, 64, r, *q, None), cn + off_text),
            (lambda: cnt(h, p, 64, r, -1.0, None, 0.0, 1.0, None, None, None, None, o), cn + radius_text),
            (lambda: cnt(h, p, 64, r, nan, None, 0.0, 1.0, None, None, None, None, o), cn + radius_text),
            (lambda: cnt(h, p, 64, r, inf, None, 0.0, 1.0, None, None, None, None, o), cn + radius_text),
            (lambda: cnt(h, p, 64, r, 2e9, None, 0.0, 1.0, None, None, vp(ind.ptr), vp(ind.ptr), o), cn + radius_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, 2.0, 1.0, None, None, None, None, o), cn + interval_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, -1.0, 1.0, None, None, None, None, o), cn + interval_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, 0.0, inf, None, None, None, None, o), cn + interval_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, 0.0, 2e9, None, None, None, None, o), cn + interval_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, nan, 1.0, None, None, None, None, o), cn + interval_text),
            (lambda: cnt(h, p, 64, r, 1.0, v, 0.0, nan, None, None, None, None, o), cn + interval_text),      # (a per-query radius: the pair is still used)
            (lambda: cnt(h, p, 64, r, nan, None, 0.0, 1.0, v, v, None, None, o), cn + radius_text),           # (per-query intervals: the radius is still used)
            (lambda: cnt(h, p, 64, r, 1.0, None, 0.0, 1.0, v, None, None, None, o), cn + pair_text),
            (lambda: cnt(h, p, 64, r, 1.0, None, 0.0, 1.0, None, v, None, None, o), cn + pair_text),
            (lambda: fil(h, None, 64, r, *q, *ft), "null prepared scene"),
            (lambda: fil(h, p, -1, r, *q, *ft), fn + count_text),
            (lambda: fil(h, p, 1 << 31, r, *q, *ft), fn + count_text),
            (lambda: fil(h, p, 64, None, *q, *ft), fn + rays_text),
            (lambda: fil(h, p, 64, r, *q, None, 4096, f, None, None, None), fn + off_text),
            (lambda: fil(h, p, 64, r, *q, o, -1, f, None, None, None), fn + ": negative capacity"),
            (lambda: fil(h, p, 64, r, *q, o, 4096, None, None, None, None), fn + ": every output is NULL"),
            (lambda: fil(h, p, 64, r, -1.0, None, 0.0, 1.0, None, None, None, None, *ft), fn + radius_text),
            (lambda: fil(h, p, 64, r, nan, None, 0.0, 1.0, None, None, None, None, *ft), fn + radius_text),
            (lambda: fil(h, p, 64, r, inf, None, 0.0, 1.0, None, None, None, None, o, 4096, None, f, None, None), fn + radius_text),
            (lambda: fil(h, p, 64, r, 1.0, None, 2.0, 1.0, None, None, None, None, *ft), fn + interval_text),
            (lambda: fil(h, p, 64, r, 1.0, None, 0.0, 2e9, None, None, None, None, o, 4096, None, None, f, None), fn + interval_text),
            (lambda: fil(h, p, 64, r, 1.0, None, nan, 1.0, None, None, None, None, o, 4096, None, None, None, f), fn + interval_text),
            (lambda: fil(h, p, 64, r, 1.0, None, 0.0, 1.0, v, None, None, None, *ft), fn + pair_text),
            (lambda: fil(h, p, 64, r, 1.0, None, 0.0, 1.0, None, v, None, None, *ft), fn + pair_text),
        ]
        for i, (call, text) in enumerate(bad):
            assert call() != 0, i
            assert lib.rt_last_error(h).decode() == text, (i, lib.rt_last_error(h).decode())
        ctx.sync()
        assert ctx.last_launch == before                                      # every refusal leaves the launch string ...
        assert np.array_equal(off.to_host(mark_off.shape, np.int64), mark_off)   # ... and the outputs untouched
        assert np.array_equal(out.to_host(mark_out.shape), mark_out)
        for args in ((-0.5, 0.0, 1.0), (1.0, 2.0, 1.0), (1.0, 0.0, float("nan")), (float("inf"), 0.0, 1.0)):
            with pytest.raises(R.RtError):
                R.spheres_along_rays(ps, some, *args)
        with pytest.raises(R.RtError):
            R.spheres_along_rays(ps, some, np.ones(64, F), 2.0, 1.0)          # a scalar pair with t_min > t_max next to an array
        with pytest.raises(R.RtError):
            R.spheres_along_rays(ps, some, 1.0, np.zeros(64, F), -1.0)        # an invalid scalar next to an array
        # a scalar is ignored where per-query values are given
        assert cnt(h, p, 64, r, nan, v, nan, nan, v, v, None, None, o) == 0
        assert ctx.last_launch == "family=along count (per-query)"
        # n == 0: offsets[0] = 0 is still written
        assert cnt(h, p, 0, r, *q, o) == 0
        assert off.to_host((1,), np.int64)[0] == 0
        assert fil(h, p, 0, r, *q, o, 0, f, None, None, None) == 0
        e = R.spheres_along_rays(ps, np.zeros((0, 6), F), 1.0, rows=True)
        assert e[0].tolist() == [0] and e[1].shape == (0,) and e[2].shape == (0, 2) and e[3].shape == (0,) and e[4].shape == (0,)
        # the launch strings under every variant
        for variant in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(variant)
            for rp, tp, ep, fp, tail in ((None, None, None, None, ""), (val.ptr, None, None, None, _tail(True)), (None, val.ptr, None, None, _tail(True)),
                                         (None, None, ind.ptr, None, _tail(exclude=True)), (None, None, None, ind.ptr, _tail(first=True)),
                                         (val.ptr, val.ptr, ind.ptr, ind.ptr, _tail(True, True, True))):
                kw = dict(radius=1.0, t_min=0.0, t_max=1.0, radius_ptr=rp, t_min_ptr=tp, t_max_ptr=tp, exclude_ptr=ep, first_ptr=fp)
                R.spheres_along_rays_count_into(rays.ptr, 64, ps, off.ptr, **kw)
                assert ctx.last_launch == "family=along count" + tail
                R.spheres_along_rays_fill_into(rays.ptr, 64, ps, off.ptr, 4096, out.ptr, None, None, None, **kw)
                assert ctx.last_launch == "family=along fill" + tail
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        for b in (rays, val, ind, off, out):
            b.free()
        ps.free()
        scene.free()


def test_multi_device_context_is_refused(R):
    from raytracers_amd._lib import lib
    vp = C.c_void_p
    cnt, fil = lib.rt_spheres_along_rays_count, lib.rt_spheres_along_rays_fill
    mc = R.Context(devices=[0, 0])                      # a multi-device context (a device listed twice)
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64 * 6)
    mark = np.full(64 * 6, POISON, np.int32)
    mc._check(lib.rt_copy_to_device(mc._h, vp(mb.ptr), mark.ctypes.data, mark.nbytes))
    bp = vp(mb.ptr)
    q = (1.0, None, 0.0, 1.0, None, None, None, None)
    tail = ": a multi-device context is not supported (use a context on one device)"
    assert cnt(mc._h, mps._h, 4, bp, *q, bp) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_along_rays_count" + tail
    assert fil(mc._h, mps._h, 4, bp, *q, bp, 8, bp, None, None, None) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_along_rays_fill" + tail
    assert np.array_equal(mb.to_host((64 * 6,)), mark), "a refused call wrote something"
    mb.free()
    mps.free()
    ms.free()
    mc.close()


def test_repeatable_torch_outputs_and_device_inputs(R):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = R.Context(0, stream=stream.cuda_stream)
        try:
            s = _random_spheres(20000, 91, 0.5, 3.0)
            ps = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            arr = ps.bvh_arrays()
            m = 1024
            rays = X.seeded_rays(arr, m, 5)
            rng = np.random.default_rng(1)
            rq, lo, hi = rng.uniform(0.0, 8.0, m).astype(F), rng.uniform(0.0, 1.0, m).astype(F), rng.uniform(1.0, 200.0, m).astype(F)
            ex, fi = rng.integers(0, 20000, m).astype(np.int32), rng.integers(-5, 10000, m).astype(np.int32)
            a = R.spheres_along_rays(ps, rays, rq, lo, hi, ex, fi, rows=True)
            b = R.spheres_along_rays(ps, rays, rq, lo, hi, ex, fi, rows=True)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            want = A.along_walk(arr, rays[:, :3], rays[:, 3:], rq, lo, hi, ex, fi)
            _same(a[:4], want, "20000 spheres")
            total = int(want[0][-1])
            assert total > m
            # device tensors used in place
            dt = [torch.as_tensor(v, device="cuda") for v in (rays, rq, lo, hi, ex, fi)]
            stream.synchronize()
            _same(R.spheres_along_rays(ps, dt[0], dt[1], dt[2], dt[3], exclude=dt[4], first=dt[5]), want, "device tensors")
            for v, w in zip(dt, (rays, rq, lo, hi, ex, fi)):
                assert np.array_equal(_bits(v.cpu().numpy()), _bits(w))
            with pytest.raises(ValueError):
                R.spheres_along_rays(ps, dt[0], dt[1].double(), dt[2], dt[3])
            # outputs allocated by torch on the context's stream
            off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            kw = dict(radius_ptr=dt[1].data_ptr(), t_min_ptr=dt[2].data_ptr(), t_max_ptr=dt[3].data_ptr(), exclude_ptr=dt[4].data_ptr(),
                      first_ptr=dt[5].data_ptr())
            R.spheres_along_rays_count_into(dt[0].data_ptr(), m, ps, off.data_ptr(), **kw)
            assert int(off[m].item()) == total
            idx = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            roots = torch.full((total + 64, 2), -3.0, dtype=torch.float32, device="cuda")
            start = torch.full((total + 64,), 7, dtype=torch.uint8, device="cuda")
            qry = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            R.spheres_along_rays_fill_into(dt[0].data_ptr(), m, ps, off.data_ptr(), total, idx.data_ptr(), roots.data_ptr(), start.data_ptr(),
                                           qry.data_ptr(), **kw)
            stream.synchronize()
            _same((off.cpu().numpy(), idx[:total].cpu().numpy(), roots[:total].cpu().numpy(), start[:total].cpu().numpy()), want, "torch outputs")
            assert np.array_equal(qry[:total].cpu().numpy(), np.repeat(np.arange(m, dtype=np.int32), np.diff(want[0])))
            assert (idx[total:] == -3).all() and (roots[total:] == -3.0).all() and (start[total:] == 7).all() and (qry[total:] == -3).all()
            ps.free()
        finally:
            c.close()
