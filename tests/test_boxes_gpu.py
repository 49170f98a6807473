"""Box queries on the GPU: rt_spheres_in_boxes_count / _fill against the numpy restatement (boxes_ref.py), bit for bit (offsets, index, gap
bits): the reference's scenes with boxes of mixed sizes, degenerate boxes against rt_spheres_within_* through the library on both sides, tall
trees whose top boxes are partial, hand-made edge boxes (tangent faces, one ulp off, the whole scene, slabs, inside a sphere, invalid ones),
a grid of cells in one call, the `first` filter, a 30 000-sphere scene through both builders and every way to prepare it, the capacity guard,
pointers offset by 4 bytes, refusals, launch strings, n == 0, repeatability and outputs allocated by torch.

The offsets array is int64 and keeps its natural 8-byte alignment in the misalignment test: only the 4-byte arrays (boxes, margins, first,
index, gap, point) are moved off the 16-byte boundary."""
import ctypes as C

import numpy as np
import pytest

import boxes_ref as B
from test_proximity_gpu import VIEW, _geometric, _points, _random_spheres

pytestmark = pytest.mark.gpu

F = np.float32
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
    for name, g, w in zip(("offsets", "index", "gap"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        bad = np.nonzero(_bits(g) != _bits(w))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


def _check(R, ctx, ps, L, boxes, margin, what, first=None):
    """spheres_in_boxes against the restatement, with and without gaps / rows, and the launch strings"""
    want = B.in_boxes(L, boxes, margin, first)
    tail = (" (per-box)" if np.ndim(margin) else "") + (" first" if first is not None else "")
    got = R.spheres_in_boxes(ps, boxes, margin, first=first)
    assert ctx.last_launch == ("family=boxes fill" if want[0][-1] else "family=boxes count") + tail, ctx.last_launch
    _same(got, want, what)
    o2, i2, g2, r2 = R.spheres_in_boxes(ps, boxes, margin, first=first, gaps=False, rows=True)
    assert g2 is None and np.array_equal(o2, got[0]) and np.array_equal(i2, got[1]), what
    assert r2.dtype == np.int32 and np.array_equal(r2, np.repeat(np.arange(boxes.shape[0], dtype=np.int32), np.diff(got[0]))), what
    return want


def _upload(ctx, ptr, a):
    from raytracers_amd._lib import lib
    a = np.ascontiguousarray(a)
    ctx._check(lib.rt_copy_to_device(ctx._h, C.c_void_p(ptr), a.ctypes.data, a.nbytes))


def _download(ctx, ptr, count, dtype):
    from raytracers_amd._lib import lib
    out = np.empty(count, dtype)
    ctx._check(lib.rt_copy_to_host(ctx._h, out.ctypes.data, C.c_void_p(ptr), out.nbytes))
    return out


# ---- 1. the reference's scenes, boxes of mixed sizes; 2. degenerate boxes against spheres_within
@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "floor"])
def test_reference_scenes(R, ctx, spec):
    scene = ctx.floor(37, 222.0) if spec == "floor" else ctx.scene(spec)
    ps = R.prepare_scene(100, 100, scene)
    L = ps.bvh_arrays()["L"]
    m = 256
    boxes = B.random_boxes(L, m, 3)
    assert (boxes[::8, :3] == boxes[::8, 3:]).all() and (boxes[:, :3] < boxes[:, 3:]).all(axis=1).sum() > m // 2   # from zero extent up
    per_box = np.random.default_rng(8).uniform(0.0, 3.0, m).astype(F)
    per_box[5] = -0.0
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    for margin in (0.0, 0.01 * ext, 1e9, per_box):
        want = _check(R, ctx, ps, L, boxes, margin, f"{spec} margin={margin if np.ndim(margin) == 0 else 'per-box'}")
        if np.ndim(margin) == 0 and margin == 1e9:
            assert (np.diff(want[0]) == L.shape[0]).all()
    assert np.diff(want[0]).max() > 8 and want[0][-1] > 1000
    # degenerate boxes: the point query on the same points and bounds, through the library on both sides
    p = _points(L, m, 5)
    p[7, 1] = np.nan
    bounds = np.random.default_rng(9).uniform(0.0, 0.02 * ext, m).astype(F)
    bounds[[11, 12, 13]] = [np.nan, -1.0, 2e9]
    first = np.random.default_rng(10).integers(-3, L.shape[0] + 3, m)
    for md in (0.0, 0.01 * ext, 1e9, bounds):
        for f in (None, first):
            got = R.spheres_in_boxes(ps, B.degenerate(p), md, first=f)
            ref = R.spheres_within(ps, p, md, first=f)
            _same(got, ref, f"{spec} degenerate")
            assert got[0][8] == got[0][7] and got[0][-1] > 0
    ps.free()
    scene.free()


# ---- 3. tall trees: the walk descends untested through the partial top boxes
def _boxes_off_the_root_box(A, m, seed):
    """small boxes around spheres that lie outside the root's STORED box (partial in a tree taller than the AABB propagation's sweeps), and
    their float64 distance to that box"""
    L, rlo, rhi = A["L"], A["bmin"][0].astype(np.float64), A["bmax"][0].astype(np.float64)
    c, r = L[:, :3].astype(np.float64), L[:, 6].astype(np.float64)
    out = np.maximum(np.maximum(rlo - (c + r[:, None]), (c - r[:, None]) - rhi), 0.0)
    far = np.nonzero(np.sqrt((out * out).sum(axis=1)) > 0)[0]
    assert far.size > 0
    rng = np.random.default_rng(seed)
    j = far[rng.integers(0, far.size, m)]
    half = r[j, None] * rng.uniform(0.0, 0.5, (m, 3))
    boxes = np.concatenate([(c[j] - half).astype(F), (c[j] + half).astype(F)], axis=1)
    boxes = np.concatenate([np.minimum(boxes[:, :3], boxes[:, 3:]), np.maximum(boxes[:, :3], boxes[:, 3:])], axis=1)
    e = np.maximum(np.maximum(rlo - boxes[:, 3:].astype(np.float64), boxes[:, :3].astype(np.float64) - rhi), 0.0)
    return np.ascontiguousarray(boxes, dtype=F), np.sqrt((e * e).sum(axis=1))


def test_tall_trees(R, ctx):
    """tall1100 and _geometric(120, 3) put their deep spheres at the origin, which the zero boxes the AABB propagation starts from hold: their
    partial top boxes happen to contain every subtree (computed from the oracle's arrays), so no query box can tell a tested root from an
    untested one there.  The third scene is _geometric moved off the origin: its root's stored box misses the deep spheres by 0.23 to 0.68,
    and the boxes around them are the ones a tested root would drop."""
    import edge_rays as E
    moved = _geometric(120, 3)
    moved[:, :3] += np.array([-300.0, -200.0, 300.0], F)
    for what, s, view in (("tall1100", E.SCENES["tall1100"][0], E.SCENES["tall1100"][1:]), ("geometric", _geometric(120, 3), VIEW),
                          ("geometric moved", moved, VIEW)):
        ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *view)
        n = s.shape[0]
        sweeps = int(np.log2(np.float32(n))) + 2
        assert ps.height > sweeps, (what, ps.height)                          # partial boxes near the root
        if what == "tall1100":
            assert ps.height - sweeps == 29                                   # the top 29 levels are untested
        A = ps.bvh_arrays()
        L = A["L"]
        deep = B.random_boxes(L, 256, 41, max_half=0.05)                      # boxes deep in the scene
        for margin in (0.0, 0.5, 1e9):
            _check(R, ctx, ps, L, deep, margin, f"{what} deep margin={margin}")
        if what == "geometric moved":
            off_root, dist = _boxes_off_the_root_box(A, 256, 43)
            margin = float(F(0.25 * dist.min()))
            want = _check(R, ctx, ps, L, off_root, margin, f"{what} off the root box")
            # the root's stored box is farther than margin + slack (about 1e-3 here) from these boxes -- its test would drop them -- yet their
            # rows are not empty
            assert (dist > margin + 0.01).all() and (np.diff(want[0]) > 0).all(), what
        ps.free()


# ---- 4. edge boxes on a hand-made scene with exactly representable coordinates
def test_edge_boxes(R, ctx):
    s = np.zeros((5, 7), F)
    s[:, :3] = [[0, 0, 0], [4, 0, 0], [0, 8, 0], [-4, -4, 2], [16, 16, 16]]
    s[:, 3:6] = 0.5
    s[:, 6] = [1.0, 0.5, 2.0, 0.25, 1.0]
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    at = {tuple(c): j for j, c in enumerate(L[:, :3].tolist())}
    j0, j2 = at[(0.0, 0.0, 0.0)], at[(0.0, 8.0, 0.0)]
    up = np.nextafter(F(1), F(2))
    boxes = np.array([
        [1, -0.5, -0.5, 2, 0.5, 0.5],                 # 0: the face x = 1 exactly tangent to sphere 0
        [up, -0.5, -0.5, 2, 0.5, 0.5],                # 1: one ulp further out
        [-100, -100, -100, 100, 100, 100],            # 2: holds the whole scene
        [0.5, -10, -10, 0.5, 10, 10],                 # 3: a zero-volume slab
        [0.25, 7.75, -0.25, 0.75, 8.25, 0.25],        # 4: wholly inside sphere (0, 8, 0) r 2, its centre outside the box
        [2, 0, 0, 1, 1, 1],                           # 5: lo.x > hi.x
        [-100, -100, -100, 100, 100, 100],            # 6
        [0, 0, np.nan, 1, 1, 1],                      # 7
        [0, 0, 0, 1, np.inf, 1],                      # 8
        [-100, -100, -100, 100, 100, 100],            # 9: invalid margins below, between valid neighbours
        [-100, -100, -100, 100, 100, 100],            # 10
        [-100, -100, -100, 100, 100, 100],            # 11
        [-100, -100, -100, 100, 100, 100],            # 12
        [0, 0, 0, 0, 0, 0],                           # 13: a degenerate box at a centre
    ], F)
    want = _check(R, ctx, ps, L, boxes, 0.0, "edge boxes, margin 0")
    off, idx, gap = R.spheres_in_boxes(ps, boxes, 0.0)
    row = lambda i: (idx[off[i]:off[i + 1]].tolist(), gap[off[i]:off[i + 1]].tolist())   # noqa: E731
    assert row(0) == ([j0], [0.0])                                            # tangency: gap == 0, selected at margin 0
    assert row(1) == ([], [])                                                 # one ulp out: gap 2^-23 > 0
    assert B.gaps(L, boxes[1:2])[0, j0] == F(2.0 ** -23)
    assert row(2)[0] == list(range(5)) and np.array_equal(_bits(gap[off[2]:off[3]]), _bits(-L[:, 6]))
    assert row(3) == (sorted([j0, j2]), [-0.5, -1.5] if j0 < j2 else [-1.5, -0.5])
    assert row(4) == ([j2], [-1.75])
    assert not np.diff(off)[[5, 7, 8]].any() and off[7] - off[6] == 5
    assert row(13) == ([j0], [-1.0])
    margins = np.zeros(14, F)
    margins[9:13] = [np.nan, -1.0, 1.0000001e9, -0.0]
    margins[1] = F(2.0 ** -23)                                                # the off-by-one-ulp box at exactly its gap
    want = _check(R, ctx, ps, L, boxes, margins, "edge boxes, per-box margins")
    ln = np.diff(want[0])
    assert ln[1] == 1 and not ln[[5, 7, 8, 9, 10, 11]].any() and ln[6] == 5 and ln[12] == 5 and ln[13] == 1
    ps.free()


# ---- 5. a grid of cells in one call: the CSR answer is the cell list
def test_grid_of_cells(R, ctx):
    scene = ctx.scene("irreg")
    ps = R.prepare_scene(100, 100, scene)
    L = ps.bvh_arrays()["L"]
    n = L.shape[0]
    lo, hi = L[:, :3].min(axis=0).astype(np.float64), L[:, :3].max(axis=0).astype(np.float64)
    gx, gz = 16, 16
    ex = np.linspace(lo[0], hi[0], gx + 1).astype(F)
    ez = np.linspace(lo[2], hi[2], gz + 1).astype(F)
    ex[0], ex[-1], ez[0], ez[-1] = F(lo[0]), F(hi[0]), F(lo[2]), F(hi[2])
    ix, iz = np.meshgrid(np.arange(gx), np.arange(gz), indexing="ij")
    ix, iz = ix.ravel(), iz.ravel()
    boxes = np.stack([ex[ix], np.full(ix.size, F(lo[1])), ez[iz], ex[ix + 1], np.full(ix.size, F(hi[1])), ez[iz + 1]], axis=1).astype(F)
    want = _check(R, ctx, ps, L, boxes, 0.0, "grid 16 x 1 x 16")
    off, idx, gap = R.spheres_in_boxes(ps, boxes, 0.0)
    # every sphere appears in the row of the cell that holds its centre (closed cells: any one of them), with gap -r
    cx = np.clip(np.searchsorted(ex, L[:, 0], side="right") - 1, 0, gx - 1)
    cz = np.clip(np.searchsorted(ez, L[:, 2], side="right") - 1, 0, gz - 1)
    cell = cx * gz + cz
    for j in range(n):
        a, b = off[cell[j]], off[cell[j] + 1]
        k = np.searchsorted(idx[a:b], j)
        assert k < b - a and idx[a + k] == j and _bits(gap[a + k:a + k + 1])[0] == _bits(np.array([-L[j, 6]], F))[0], j
    assert off[-1] >= n
    ps.free()
    scene.free()


# ---- 6. the lower index bound
def test_first(R, ctx):
    s = _random_spheres(5000, 55, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    n, m = 5000, 512
    boxes = B.random_boxes(L, m, 7, max_half=0.1)
    rng = np.random.default_rng(3)
    first = rng.integers(-10, n + 10, m)
    first[:7] = [0, -1, -(2 ** 31), n // 2, n, n + 1, 2 ** 31 - 1]
    boxes[:7] = [-1e3, -1e3, -1e3, 1e3, 1e3, 1e3]                              # whole-scene boxes for the stated values
    for margin in (1.0, rng.uniform(0.0, 4.0, m).astype(F)):
        off, idx, gap = R.spheres_in_boxes(ps, boxes, margin)
        want = _check(R, ctx, ps, L, boxes, margin, "first", first=first)
        foff, fidx, fgap = want
        for i in range(m):                                       # a row with first = f: the unfiltered row's entries with j >= f
            row, g = idx[off[i]:off[i + 1]], gap[off[i]:off[i + 1]]
            keep = row >= first[i]
            assert np.array_equal(fidx[foff[i]:foff[i + 1]], row[keep]) and np.array_equal(_bits(fgap[foff[i]:foff[i + 1]]), _bits(g[keep])), i
        assert np.diff(foff)[:7].tolist() == [n, n, n, n - n // 2, 0, 0, 0]
    import torch
    ft = torch.as_tensor(first.astype(np.int32), device="cuda")
    bt = torch.as_tensor(boxes, device="cuda")
    mt = torch.full((m,), 1.0, dtype=torch.float32, device="cuda")
    _same(R.spheres_in_boxes(ps, bt, mt, first=ft), B.in_boxes(L, boxes, 1.0, first), "device tensors")
    assert ctx.last_launch == "family=boxes fill (per-box) first"
    ps.free()


# ---- 7. the builder's large class with a run of coincident centres, through every way to prepare the scene
def test_large_scene_every_builder(R):
    n, m = 30000, 512
    s = _random_spheres(n, 71)
    s[29000:29100, :3] = s[0, :3]                                             # equal Morton keys
    other = _random_spheres(n, 72)
    answers = []
    L0 = None
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
                L = ps.bvh_arrays()["L"]
                if L0 is None:
                    L0 = L
                    boxes = B.random_boxes(L0, m, 13, max_half=0.05)
                    boxes[:16, :3] = s[0, :3] - F(0.5)                        # boxes on the coincident run
                    boxes[:16, 3:] = s[0, :3] + F(0.5)
                    margin = np.random.default_rng(5).uniform(0.0, 2.0, m).astype(F)
                assert L.tobytes() == L0.tobytes()
                answers.append(R.spheres_in_boxes(ps, boxes, margin, rows=True))
                ps.free()
            sc.free()
        finally:
            c.close()
    want = B.in_boxes(L0, boxes, margin)
    _same(answers[0][:3], want, "30000 spheres")
    assert np.diff(want[0])[:16].min() >= 100
    for k, got in enumerate(answers[1:]):
        for x, y in zip(got, answers[0]):
            assert x.tobytes() == y.tobytes(), k + 1


# ---- 8. the capacity guard; 9. pointers 4 bytes off a 16-byte boundary
def test_capacity_guard_and_misaligned_pointers(R, ctx):
    s = _random_spheres(3000, 31, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    m = 300
    boxes = B.random_boxes(L, m, 17, max_half=0.1)
    margin = np.random.default_rng(6).uniform(0.0, 40.0, m).astype(F)
    first = np.random.default_rng(7).integers(-5, 1500, m).astype(np.int32)
    want = B.in_boxes(L, boxes, margin, first)
    total = int(want[0][-1])
    assert total > 2000
    guard = 257                                                               # entries in front of and behind each output; odd, and ...
    pad = 1                                                                   # ... every 4-byte array starts 4 bytes past a 16-byte boundary
    DB = R.api.DeviceBuffer
    bbuf, mbuf, fbuf = DB(ctx, 24 * m + 16), DB(ctx, 4 * m + 16), DB(ctx, 4 * m + 16)
    off = DB(ctx, 8 * (m + 1))
    outs = [DB(ctx, 4 * (total + 2 * guard)) for _ in range(3)]
    try:
        bp, mp, fp = bbuf.ptr + 4 * pad, mbuf.ptr + 4 * pad, fbuf.ptr + 4 * pad
        assert bp % 16 == 4 and mp % 16 == 4 and fp % 16 == 4
        _upload(ctx, bp, boxes)
        _upload(ctx, mp, margin)
        _upload(ctx, fp, first)
        op = [o.ptr + 4 * guard for o in outs]
        assert all(p % 16 == 4 for p in op)

        def poison():
            for o in outs:
                _upload(ctx, o.ptr, np.full(total + 2 * guard, POISON, np.int32))

        def read():
            ctx.sync()
            return [_download(ctx, o.ptr, total + 2 * guard, np.int32) for o in outs]

        R.spheres_in_boxes_count_into(bp, m, ps, off.ptr, 0.0, mp, fp)
        assert ctx.last_launch == "family=boxes count (per-box) first"
        offsets = off.to_host((m + 1,), np.int64)
        assert np.array_equal(offsets, want[0])
        # the whole answer through the misaligned pointers
        poison()
        R.spheres_in_boxes_fill_into(bp, m, ps, off.ptr, total, op[0], op[1], op[2], 0.0, mp, fp)
        gi, gg, gr = read()
        assert np.array_equal(gi[guard:guard + total], want[1]) and np.array_equal(gg[guard:guard + total].view(np.uint32), _bits(want[2]))
        assert np.array_equal(gr[guard:guard + total], np.repeat(np.arange(m, dtype=np.int32), np.diff(want[0])))
        for g in (gi, gg, gr):
            assert (g[:guard] == POISON).all() and (g[guard + total:] == POISON).all()
        # capacity below the total: the entries below it, nothing at or past it
        cap = total // 2 + 1
        poison()
        R.spheres_in_boxes_fill_into(bp, m, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
        gi, gg, gr = read()
        assert np.array_equal(gi[guard:guard + cap], want[1][:cap]) and np.array_equal(gg[guard:guard + cap].view(np.uint32), _bits(want[2][:cap]))
        for g in (gi, gg, gr):
            assert (g[:guard] == POISON).all() and (g[guard + cap:] == POISON).all()
        # offsets of another query (longer rows: a scalar margin of 80, no first), then shifted far up and far down: no write outside [0, cap)
        foreign = B.in_boxes(L, boxes, 80.0)[0]
        assert foreign[-1] > 2 * total
        for o in (foreign, foreign + (1 << 40), foreign - (foreign[-1] // 2), want[0][::-1].copy()):
            _upload(ctx, off.ptr, o.astype(np.int64))
            poison()
            R.spheres_in_boxes_fill_into(bp, m, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
            for g in read():
                assert (g[:guard] == POISON).all() and (g[guard + cap:] == POISON).all()
        # negative offsets everywhere: nothing is written at all
        _upload(ctx, off.ptr, np.arange(-(m + 1) * 10, 0, 10, dtype=np.int64))
        poison()
        R.spheres_in_boxes_fill_into(bp, m, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
        for g in read():
            assert (g == POISON).all()
    finally:
        for b in [bbuf, mbuf, fbuf, off] + outs:
            b.free()
        ps.free()


# ---- 10. refusals, n == 0, launch strings under every variant, repeatability, torch outputs
def test_refusals_and_launch(R, ctx):
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    vp = C.c_void_p
    DB = R.api.DeviceBuffer
    bx, mg, fi, off, out = DB(ctx, 24 * 64), DB(ctx, 4 * 64), DB(ctx, 4 * 64), DB(ctx, 8 * 65), DB(ctx, 8 * 4096)
    try:
        mark_off = np.full(65, -7, np.int64)
        mark_out = np.full(2 * 4096, POISON, np.int32)
        _upload(ctx, off.ptr, mark_off)
        _upload(ctx, out.ptr, mark_out)
        _upload(ctx, bx.ptr, np.tile(np.array([-1, -1, -1, 1, 1, 1], F), (64, 1)))
        R.nearest_spheres(ps, np.zeros((5, 3), F), 5, 1.0)
        before = ctx.last_launch
        assert before == "family=nearest k=5"
        h, p, b, o, f = ctx._h, ps._h, vp(bx.ptr), vp(off.ptr), vp(out.ptr)
        nan, inf = float("nan"), float("inf")
        cnt, fill = lib.rt_spheres_in_boxes_count, lib.rt_spheres_in_boxes_fill
        bad = [
            (lambda: cnt(h, None, 64, b, 1.0, None, None, o), "null prepared scene"),
            (lambda: cnt(h, p, -1, b, 1.0, None, None, o), "rt_spheres_in_boxes_count: box count out of range: 0 <= n < 2^31"),
            (lambda: cnt(h, p, 1 << 31, b, 1.0, None, None, o), "rt_spheres_in_boxes_count: box count out of range: 0 <= n < 2^31"),
            (lambda: cnt(h, p, 64, None, 1.0, None, None, o), "rt_spheres_in_boxes_count: null boxes pointer"),
            (lambda: cnt(h, p, 64, b, 1.0, None, None, None), "rt_spheres_in_boxes_count: null offsets pointer"),
            (lambda: cnt(h, p, 64, b, -1.0, None, None, o), "rt_spheres_in_boxes_count: need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, nan, None, None, o), "rt_spheres_in_boxes_count: need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, inf, None, None, o), "rt_spheres_in_boxes_count: need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, 2e9, None, vp(fi.ptr), o), "rt_spheres_in_boxes_count: need 0 <= margin <= 1e9, finite"),
            (lambda: fill(h, None, 64, b, 1.0, None, None, o, 4096, f, None, None), "null prepared scene"),
            (lambda: fill(h, p, -1, b, 1.0, None, None, o, 4096, f, None, None), "rt_spheres_in_boxes_fill: box count out of range: 0 <= n < 2^31"),
            (lambda: fill(h, p, 1 << 31, b, 1.0, None, None, o, 4096, f, None, None), "rt_spheres_in_boxes_fill: box count out of range: 0 <= n < 2^31"),
            (lambda: fill(h, p, 64, None, 1.0, None, None, o, 4096, f, None, None), "rt_spheres_in_boxes_fill: null boxes pointer"),
            (lambda: fill(h, p, 64, b, 1.0, None, None, None, 4096, f, None, None), "rt_spheres_in_boxes_fill: null offsets pointer"),
            (lambda: fill(h, p, 64, b, 1.0, None, None, o, -1, f, None, None), "rt_spheres_in_boxes_fill: negative capacity"),
            (lambda: fill(h, p, 64, b, 1.0, None, None, o, 4096, None, None, None), "rt_spheres_in_boxes_fill: every output is NULL"),
            (lambda: fill(h, p, 64, b, nan, None, None, o, 4096, f, None, None), "rt_spheres_in_boxes_fill: need 0 <= margin <= 1e9, finite"),
            (lambda: fill(h, p, 64, b, -0.5, None, None, o, 4096, None, f, None), "rt_spheres_in_boxes_fill: need 0 <= margin <= 1e9, finite"),
        ]
        for i, (call, text) in enumerate(bad):
            assert call() != 0, i
            assert lib.rt_last_error(h).decode() == text, (i, lib.rt_last_error(h).decode())
        assert ctx.last_launch == before                                      # every refusal leaves the launch string ...
        ctx.sync()
        assert np.array_equal(off.to_host(mark_off.shape, np.int64), mark_off)   # ... and the outputs untouched
        assert np.array_equal(out.to_host(mark_out.shape), mark_out)
        with pytest.raises(R.RtError):
            R.spheres_in_boxes(ps, np.zeros((4, 6), F), -0.5)
        with pytest.raises(ValueError):
            R.spheres_in_boxes(ps, np.zeros((4, 3), F), 0.0)
        # a scalar margin is ignored when per-box margins are given
        _upload(ctx, mg.ptr, np.ones(64, F))
        assert cnt(h, p, 64, b, nan, vp(mg.ptr), None, o) == 0
        assert ctx.last_launch == "family=boxes count (per-box)"
        # n == 0: offsets[0] = 0 is still written
        _upload(ctx, off.ptr, mark_off)
        assert cnt(h, p, 0, b, 1.0, None, None, o) == 0
        assert off.to_host((2,), np.int64).tolist() == [0, -7]
        assert fill(h, p, 0, b, 1.0, None, None, o, 0, f, None, None) == 0
        e = R.spheres_in_boxes(ps, np.zeros((0, 6), F), 1.0, rows=True)
        assert e[0].tolist() == [0] and e[1].shape == (0,) and e[2].shape == (0,) and e[3].shape == (0,)
        # the launch strings under every variant
        _upload(ctx, fi.ptr, np.zeros(64, np.int32))
        for v in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(v)
            for mgp, fip, tail in ((None, None, ""), (mg.ptr, None, " (per-box)"), (None, fi.ptr, " first"), (mg.ptr, fi.ptr, " (per-box) first")):
                R.spheres_in_boxes_count_into(bx.ptr, 64, ps, off.ptr, 1.0, mgp, fip)
                assert ctx.last_launch == "family=boxes count" + tail
                R.spheres_in_boxes_fill_into(bx.ptr, 64, ps, off.ptr, 4096, out.ptr, None, None, 1.0, mgp, fip)
                assert ctx.last_launch == "family=boxes fill" + tail
            R.spheres_in_boxes_fill_into(bx.ptr, 64, ps, off.ptr, 4096, None, out.ptr, None, 1.0)   # only the gaps
            R.spheres_in_boxes_fill_into(bx.ptr, 64, ps, off.ptr, 4096, None, None, out.ptr, 1.0)   # only the rows
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        for x in (bx, mg, fi, off, out):
            x.free()
        ps.free()
        scene.free()


def test_multi_device_context_is_refused(R):
    from raytracers_amd._lib import lib
    vp = C.c_void_p
    cnt, fill = lib.rt_spheres_in_boxes_count, lib.rt_spheres_in_boxes_fill
    # a multi-device context (a device listed twice)
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64 * 6)
    bp = vp(mb.ptr)
    assert cnt(mc._h, mps._h, 4, bp, 1.0, None, None, bp) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_in_boxes_count: a multi-device context is not supported (use a context on one device)"
    assert fill(mc._h, mps._h, 4, bp, 1.0, None, None, bp, 8, bp, None, None) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_in_boxes_fill: a multi-device context is not supported (use a context on one device)"
    mb.free()
    mps.free()
    ms.free()
    mc.close()


def test_repeatable_and_torch_outputs(R):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = R.Context(0, stream=stream.cuda_stream)
        try:
            s = _random_spheres(20000, 91, 0.5, 3.0)
            ps = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            L = ps.bvh_arrays()["L"]
            m = 1024
            boxes = B.random_boxes(L, m, 5, max_half=0.05)
            a, b = R.spheres_in_boxes(ps, boxes, 1.5, rows=True), R.spheres_in_boxes(ps, boxes, 1.5, rows=True)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            # outputs allocated by torch on the context's stream, in place
            want = B.in_boxes(L, boxes, 1.5)
            _same(a[:3], want, "20000 spheres")
            bt = torch.as_tensor(boxes, device="cuda")
            off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            R.spheres_in_boxes_count_into(bt.data_ptr(), m, ps, off.data_ptr(), 1.5)
            total = int(off[m].item())
            assert total == want[0][-1]
            idx = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            gap = torch.full((total + 64,), -3.0, dtype=torch.float32, device="cuda")
            row = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            R.spheres_in_boxes_fill_into(bt.data_ptr(), m, ps, off.data_ptr(), total, idx.data_ptr(), gap.data_ptr(), row.data_ptr(), 1.5)
            stream.synchronize()
            _same((off.cpu().numpy(), idx[:total].cpu().numpy(), gap[:total].cpu().numpy()), want, "torch outputs")
            assert np.array_equal(row[:total].cpu().numpy(), np.repeat(np.arange(m, dtype=np.int32), np.diff(want[0])))
            assert (idx[total:] == -3).all() and (gap[total:] == -3.0).all() and (row[total:] == -3).all()
            ps.free()
        finally:
            c.close()
