"""Plane-set queries on the GPU: rt_spheres_in_planes_count / _fill against the numpy restatement (planes_ref.py), bit for bit (offsets, index,
gap bits, point): the reference's scenes with half-spaces, slabs, oriented boxes, frusta and empty regions at every plane count the walk is
instantiated for and at partial waves, tall trees whose top boxes are partial, hand-made edge planes (tangent, one ulp either side, through
centres, -0.0 components, the whole scene, duplicated, contradictory, scaled to the ends of the valid range, invalid ones), the box entry on the
same boxes written as planes, the tiles of a camera against the ray entries, the `first` filter, the capacity guard, pointers offset by 4
bytes, refusals, launch strings, n == 0, rebuilt scenes, a 30 000-sphere scene through both builders, repeatability and torch tensors.

The offsets array is int64 and keeps its natural 8-byte alignment in the misalignment test: only the 4-byte arrays (planes, margins, first,
index, gap, point) are moved off the 16-byte boundary."""
import ctypes as C

import numpy as np
import pytest

import boxes_ref as B
import planes_ref as PL
from test_boxes_gpu import _boxes_off_the_root_box
from test_proximity_gpu import VIEW, _geometric, _random_spheres

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


def _check(R, ctx, ps, L, planes, margin, what, first=None):
    """spheres_in_planes against the restatement, with and without gaps / rows, and the launch strings"""
    want = PL.in_planes(L, planes, margin, first)
    tail = f" k={planes.shape[1]}" + (" (per-query)" if np.ndim(margin) else "") + (" first" if first is not None else "")
    got = R.spheres_in_planes(ps, planes, margin, first=first)
    assert ctx.last_launch == ("family=planes fill" if want[0][-1] else "family=planes count") + tail, ctx.last_launch
    _same(got, want, what)
    o2, i2, g2, r2 = R.spheres_in_planes(ps, planes, margin, first=first, gaps=False, rows=True)
    assert g2 is None and np.array_equal(o2, got[0]) and np.array_equal(i2, got[1]), what
    assert r2.dtype == np.int32 and np.array_equal(r2, np.repeat(np.arange(planes.shape[0], dtype=np.int32), np.diff(got[0]))), what
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


# ---- 1. the reference's scenes: every kind of region, plane counts 1 .. 8, partial waves and the block boundary
@pytest.fixture(scope="module", params=["rgbbox", "irreg", "floor"])
def ref_scene(request, R, ctx):
    scene = ctx.floor(37, 222.0) if request.param == "floor" else ctx.scene(request.param)
    ps = R.prepare_scene(100, 100, scene)
    yield request.param, ps, ps.bvh_arrays()["L"]
    ps.free()
    scene.free()


@pytest.mark.parametrize("K", [1, 2, 4, 5, 6, 8])
def test_reference_scenes(R, ctx, ref_scene, K):
    spec, ps, L = ref_scene
    m = 320
    planes = PL.random_planes(L, m, K, 100 + K)
    per_query = np.random.default_rng(8).uniform(0.0, 3.0, m).astype(F)
    per_query[5] = -0.0
    per_query[[11, 12, 13]] = [np.nan, -1.0, 2e9]
    total = 0
    for margin in (0.0, 0.5, per_query):
        want = _check(R, ctx, ps, L, planes, margin, f"{spec} K={K} margin={margin if np.ndim(margin) == 0 else 'per-query'}")
        total += int(want[0][-1])
        if np.ndim(margin):
            assert want[0][6] > want[0][5] and not np.diff(want[0])[[11, 12, 13]].any()
    assert total > 3000
    for n in (1, 63, 64, 65):                                                 # a partial wave, a full one, the block boundary
        _check(R, ctx, ps, L, np.ascontiguousarray(planes[:n]), 0.5, f"{spec} K={K} n={n}")
    want = _check(R, ctx, ps, L, np.ascontiguousarray(planes[:65]), 1e9, f"{spec} K={K} margin=1e9")
    assert (np.diff(want[0]) == L.shape[0]).all()                             # every sphere of the scene in every row


# ---- 2. tall trees: the walk descends untested through the partial top boxes
def test_tall_trees(R, ctx):
    """As test_boxes_gpu.test_tall_trees: tall1100 and _geometric(120, 3) happen to keep every subtree inside their partial top boxes; the
    third scene is _geometric moved off the origin, whose root's stored box misses the deep spheres.  The planes aimed at those are the faces
    of small boxes around them (six planes), and one face alone (a half-space): a tested root would fail a plane by more than the margin."""
    import edge_rays as E
    moved = _geometric(120, 3)
    moved[:, :3] += np.array([-300.0, -200.0, 300.0], F)
    for what, s, view in (("tall1100", E.SCENES["tall1100"][0], E.SCENES["tall1100"][1:]), ("geometric", _geometric(120, 3), VIEW),
                          ("geometric moved", moved, VIEW)):
        ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *view)
        n = s.shape[0]
        sweeps = int(np.log2(np.float32(n))) + 2
        assert ps.height > sweeps, (what, ps.height)                          # partial boxes near the root
        A = ps.bvh_arrays()
        L = A["L"]
        for K in (3, 6):
            deep = PL.random_planes(L, 256, K, 41 + K)
            for margin in (0.0, 0.5, 1e9):
                _check(R, ctx, ps, L, deep, margin, f"{what} deep K={K} margin={margin}")
        if what == "geometric moved":
            off_root, dist = _boxes_off_the_root_box(A, 256, 43)
            planes = PL.box_planes(off_root)
            margin = float(F(0.25 * dist.min()))
            want = _check(R, ctx, ps, L, planes, margin, f"{what} off the root box")
            assert (np.diff(want[0]) > 0).all(), what
            # the root's stored box lies beyond one face of every query by more than margin + slack (about 1e-3 here): its test would drop them
            rlo, rhi = A["bmin"][0].astype(np.float64), A["bmax"][0].astype(np.float64)
            p = planes.astype(np.float64)
            v = np.where(p[..., :3] >= 0, rhi, rlo)
            D = (p[..., :3] * v).sum(axis=2) + p[..., 3]
            worst = (-D).argmax(axis=1)
            assert ((-D).max(axis=1) > margin + 0.01).all(), what
            # ... and so would the test of that one face as a half-space
            half = np.ascontiguousarray(planes[np.arange(256), worst][:, None, :])
            want = _check(R, ctx, ps, L, half, margin, f"{what} one face off the root box")
            assert (np.diff(want[0]) > 0).all(), what
        ps.free()


# ---- 3. edge planes on a hand-made scene with exactly representable coordinates
def test_edge_planes(R, ctx):
    s = np.zeros((5, 7), F)
    s[:, :3] = [[0, 0, 0], [4, 0, 0], [0, 8, 0], [-4, -4, 2], [16, 16, 16]]
    s[:, 3:6] = 0.5
    s[:, 6] = [1.0, 0.5, 2.0, 0.25, 1.0]
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    at = {tuple(c): j for j, c in enumerate(L[:, :3].tolist())}
    j0, j2 = at[(0.0, 0.0, 0.0)], at[(0.0, 8.0, 0.0)]
    up, down = np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0))
    nan, inf = np.nan, np.inf
    left, low = [-1, 0, 0, 2], [0, -1, 0, 4]                                  # x <= 2 and y <= 4: with x >= 1 a region only sphere 0 meets
    far = [1, 0, 0, 100]                                                      # a half-space that holds the whole scene
    one = np.array([
        [[1, 0, 0, -1], left, low],                                # 0: x >= 1 exactly tangent to sphere 0: gap == 0
        [[1, 0, 0, -up], left, low],                               # 1: one ulp further out: gap 2^-23
        [[1, 0, 0, -down], left, low],                             # 2: one ulp nearer: gap -2^-24
        [[0, 1, 0, -8], [0, -1, 0, 8], [0, 1, 0, -8]],             # 3: the plane y == 8, through the centre of sphere (0, 8, 0) r 2
        [[-0.0, 1, -0.0, -8], [0.0, -1, -0.0, 8], [-0.0, 1, 0.0, -8]],   # 4: the same with -0.0 components
        [far, far, far],                                           # 5: the whole scene, the plane twice duplicated
        [[1, 0, 0, -10], [-1, 0, 0, -10], [1, 0, 0, -10]],         # 6: contradictory: x >= 10 and x <= -10
        [[2.0 ** -39, 0, 0, -2.0 ** -39], left, low],              # 7: query 0's plane scaled by 2^-39 ...
        [[2.0 ** 39, 0, 0, -2.0 ** 39], left, low],                # 8: ... and by 2^39
        [[0, 0, 0, 1], left, low],                                 # 9: a zero normal
        [far, far, far],                                           # 10
        [[1, 0, nan, 100], far, far],                              # 11
        [far, far, [1, 0, 0, inf]],                                # 12
        [far, far, far],                                           # 13: invalid margins below, between valid neighbours
        [far, far, far],                                           # 14
        [far, far, far],                                           # 15
        [far, far, far],                                           # 16
        [[2.0 ** -41, 0, 0, 0], left, low],                        # 17: len below 2^-40
        [left, [0, 2.0 ** 41, 0, 0], low],                         # 18: len above 2^40
    ], F)
    want = _check(R, ctx, ps, L, one, 0.0, "edge planes, margin 0")
    off, idx, gap = R.spheres_in_planes(ps, one, 0.0)
    row = lambda i: (idx[off[i]:off[i + 1]].tolist(), gap[off[i]:off[i + 1]].tolist())   # noqa: E731
    assert row(0) == ([j0], [0.0])                                            # tangency: gap == 0, selected at margin 0
    assert row(1) == ([], [])                                                 # one ulp out: gap 2^-23 > 0
    assert PL.gaps(L, one[1:2])[0, j0] == F(2.0 ** -23)
    assert row(2) == ([j0], [-(2.0 ** -24)])
    assert row(3) == ([j2], [-2.0]) and row(4) == ([j2], [-2.0])
    assert row(5)[0] == list(range(5)) and np.array_equal(_bits(gap[off[5]:off[6]]), _bits(-L[:, 6]))
    assert row(6) == ([], [])
    assert row(7) == row(0) and row(8) == row(0)
    assert not np.diff(off)[[9, 11, 12, 17, 18]].any() and off[11] - off[10] == 5
    margins = np.zeros(19, F)
    margins[13:17] = [np.nan, -1.0, 1.0000001e9, -0.0]
    margins[1] = F(2.0 ** -23)                                                # the off-by-one-ulp plane at exactly its gap
    margins[6] = F(9.0)                                                       # the contradictory pair at exactly sphere 0's gap, 10 - 1
    want = _check(R, ctx, ps, L, one, margins, "edge planes, per-query margins")
    ln = np.diff(want[0])
    assert ln[1] == 1 and not ln[[9, 11, 12, 13, 14, 15, 17, 18]].any() and ln[10] == 5 and ln[16] == 5
    a, b = want[0][6], want[0][7]
    assert j0 in want[1][a:b].tolist() and want[2][a:b][want[1][a:b].tolist().index(j0)] == F(9.0)
    ps.free()
    # one half-space that holds a whole scene of more spheres than any stack is deep: all of them, ascending, with gap -r
    s = _random_spheres(5000, 57, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    whole = np.array([[[0, 0, 1, 1e4]], [[0, 0, -3, 1e5]]], F)
    want = _check(R, ctx, ps, L, whole, 0.0, "whole scene")
    assert np.array_equal(want[1], np.tile(np.arange(5000, dtype=np.int32), 2)) and np.array_equal(_bits(want[2]), _bits(np.tile(-L[:, 6], 2)))
    ps.free()


# ---- 4. against the box entry, on the same device boxes written as planes
def test_against_the_box_entry(R, ctx):
    scene = ctx.scene("irreg")
    ps = R.prepare_scene(100, 100, scene)
    L = ps.bvh_arrays()["L"]
    m = 384
    boxes = B.random_boxes(L, m, 3)
    planes = PL.box_planes(boxes)
    with np.errstate(all="ignore"):
        pos = sum((np.fmax(boxes[:, None, k] - L[None, :, k], L[None, :, k] - boxes[:, None, 3 + k]) > 0).astype(int) for k in range(3))
    shared = equal = 0
    for margin in (0.0, 0.5, np.random.default_rng(4).uniform(0.0, 3.0, m).astype(F)):
        _check(R, ctx, ps, L, planes, margin, "box planes")
        po, pi, pg = R.spheres_in_planes(ps, planes, margin)
        bo, bi, bg = R.spheres_in_boxes(ps, boxes, margin)
        assert bo[-1] > 0 and po[-1] >= bo[-1]
        for i in range(m):
            prow, brow = pi[po[i]:po[i + 1]], bi[bo[i]:bo[i + 1]]
            where = np.searchsorted(prow, brow)
            assert (where < prow.size).all() and np.array_equal(prow[where], brow), i    # the plane row holds the box row
            one = pos[i, brow] <= 1
            assert np.array_equal(_bits(pg[po[i]:po[i + 1]][where][one]), _bits(bg[bo[i]:bo[i + 1]][one])), i
            assert (pg[po[i]:po[i + 1]][where] <= bg[bo[i]:bo[i + 1]]).all(), i
            shared += brow.size
            equal += int(one.sum())
    assert equal > 1000 and shared > equal
    ps.free()
    scene.free()


# ---- 5. against the ray entries: a camera's tiles hold every sphere their pixels' rays hit
def test_tiles_hold_what_their_rays_hit(R, ctx):
    h, w, th, tw = 96, 128, 8, 8
    scene = ctx.scene("irreg")
    ps = R.prepare_scene(h, w, scene)
    L = ps.bvh_arrays()["L"]
    idx, _ = R.intersect_rays(ps, R.camera_rays(ps, h, w))
    planes = R.tile_frusta(ps.camera(), h, w, th, tw)
    assert planes.shape == (12 * 16, 4, 4)
    want = _check(R, ctx, ps, L, planes, 0.0, "tile frusta")
    off, pi, _ = R.spheres_in_planes(ps, planes, 0.0)
    member = np.zeros((planes.shape[0], L.shape[0]), bool)
    member[np.repeat(np.arange(planes.shape[0]), np.diff(off)), pi] = True
    rows, cols = np.divmod(np.arange(h * w), w)
    tile = (rows // th) * (w // tw) + cols // tw
    hit = idx >= 0
    assert hit.sum() > h * w // 4
    assert member[tile[hit], idx[hit]].all()                                  # zero missed spheres
    assert want[0][-1] / planes.shape[0] < 0.05 * L.shape[0]
    ps.free()
    scene.free()


# ---- 6. the lower index bound
def test_first(R, ctx):
    s = _random_spheres(5000, 55, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    n, m = 5000, 512
    planes = PL.random_planes(L, m, 6, 7)
    rng = np.random.default_rng(3)
    first = rng.integers(-10, n + 10, m)
    first[:7] = [0, -1, -(2 ** 31), n // 2, n, n + 1, 2 ** 31 - 1]
    planes[:7] = [0, 1, 0, 1e4]                                               # whole-scene half-spaces for the stated values
    for margin in (1.0, rng.uniform(0.0, 4.0, m).astype(F)):
        off, idx, gap = R.spheres_in_planes(ps, planes, margin)
        foff, fidx, fgap = _check(R, ctx, ps, L, planes, margin, "first", first=first)
        for i in range(m):                                       # a row with first = f: the unfiltered row's entries with j >= f
            row, g = idx[off[i]:off[i + 1]], gap[off[i]:off[i + 1]]
            keep = row >= first[i]
            assert np.array_equal(fidx[foff[i]:foff[i + 1]], row[keep]) and np.array_equal(_bits(fgap[foff[i]:foff[i + 1]]), _bits(g[keep])), i
        assert np.diff(foff)[:7].tolist() == [n, n, n, n - n // 2, 0, 0, 0]
    import torch
    ft = torch.as_tensor(first.astype(np.int32), device="cuda")
    pt = torch.as_tensor(planes, device="cuda")
    mt = torch.full((m,), 1.0, dtype=torch.float32, device="cuda")
    _same(R.spheres_in_planes(ps, pt, mt, first=ft), PL.in_planes(L, planes, 1.0, first), "device tensors")
    assert ctx.last_launch == "family=planes fill k=6 (per-query) first"
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
                    planes = PL.random_planes(L0, m, 6, 13)
                    box = np.concatenate([s[0, :3] - F(0.5), s[0, :3] + F(0.5)])[None, :]
                    planes[:16] = PL.box_planes(box)                          # queries on the coincident run
                    margin = np.random.default_rng(5).uniform(0.0, 2.0, m).astype(F)
                assert L.tobytes() == L0.tobytes()
                answers.append(R.spheres_in_planes(ps, planes, margin, rows=True))
                ps.free()
            sc.free()
        finally:
            c.close()
    want = PL.in_planes(L0, planes, margin)
    _same(answers[0][:3], want, "30000 spheres")
    assert np.diff(want[0])[:16].min() >= 100
    for k, got in enumerate(answers[1:]):
        for x, y in zip(got, answers[0]):
            assert x.tobytes() == y.tobytes(), k + 1


# ---- 8. rebuilt scenes: the rows follow the new spheres
def test_rebuilt_scenes(R, ctx):
    a, b = _random_spheres(3000, 81, 0.5, 3.0), _random_spheres(3000, 82, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, a, 64, 64, *VIEW)
    La = ps.bvh_arrays()["L"]
    planes = PL.random_planes(La, 256, 7, 19)                                 # (seven planes: with the other tests every instantiation's rows are compared)
    wa = _check(R, ctx, ps, La, planes, 0.5, "prepared from spheres")
    ps.update_spheres(b)
    Lb = ps.bvh_arrays()["L"]
    wb = _check(R, ctx, ps, Lb, planes, 0.5, "after update_spheres")
    assert wa[0][-1] > 1000 and wb[0][-1] > 1000 and not np.array_equal(wa[0], wb[0])
    ps.update_spheres(a)
    _same(R.spheres_in_planes(ps, planes, 0.5), wa, "updated back")
    ps.free()


# ---- 9. the capacity guard; 10. pointers 4 bytes off a 16-byte boundary
def test_capacity_guard_and_misaligned_pointers(R, ctx):
    s = _random_spheres(3000, 31, 0.5, 3.0)
    ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)
    L = ps.bvh_arrays()["L"]
    m, K = 300, 5
    planes = PL.random_planes(L, m, K, 17)
    margin = np.random.default_rng(6).uniform(0.0, 40.0, m).astype(F)
    first = np.random.default_rng(7).integers(-5, 1500, m).astype(np.int32)
    want = PL.in_planes(L, planes, margin, first)
    total = int(want[0][-1])
    assert total > 2000
    guard = 257                                                               # entries in front of and behind each output; odd, and ...
    pad = 1                                                                   # ... every 4-byte array starts 4 bytes past a 16-byte boundary
    DB = R.api.DeviceBuffer
    pbuf, mbuf, fbuf = DB(ctx, 16 * K * m + 16), DB(ctx, 4 * m + 16), DB(ctx, 4 * m + 16)
    off = DB(ctx, 8 * (m + 1))
    outs = [DB(ctx, 4 * (total + 2 * guard)) for _ in range(3)]
    try:
        pp, mp, fp = pbuf.ptr + 4 * pad, mbuf.ptr + 4 * pad, fbuf.ptr + 4 * pad
        assert pp % 16 == 4 and mp % 16 == 4 and fp % 16 == 4
        _upload(ctx, pp, planes)
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

        R.spheres_in_planes_count_into(pp, m, K, ps, off.ptr, 0.0, mp, fp)
        assert ctx.last_launch == "family=planes count k=5 (per-query) first"
        offsets = off.to_host((m + 1,), np.int64)
        assert np.array_equal(offsets, want[0])
        # the whole answer through the misaligned pointers; capacity at the total, then above it
        for cap in (total, total + 100):
            poison()
            R.spheres_in_planes_fill_into(pp, m, K, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
            gi, gg, gr = read()
            assert np.array_equal(gi[guard:guard + total], want[1]) and np.array_equal(gg[guard:guard + total].view(np.uint32), _bits(want[2]))
            assert np.array_equal(gr[guard:guard + total], np.repeat(np.arange(m, dtype=np.int32), np.diff(want[0])))
            for g in (gi, gg, gr):
                assert (g[:guard] == POISON).all() and (g[guard + total:] == POISON).all()
        # capacity below the total: the entries below it, nothing at or past it
        cap = total // 2 + 1
        poison()
        R.spheres_in_planes_fill_into(pp, m, K, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
        gi, gg, gr = read()
        assert np.array_equal(gi[guard:guard + cap], want[1][:cap]) and np.array_equal(gg[guard:guard + cap].view(np.uint32), _bits(want[2][:cap]))
        for g in (gi, gg, gr):
            assert (g[:guard] == POISON).all() and (g[guard + cap:] == POISON).all()
        # offsets of another query (longer rows: a scalar margin of 80, no first), then shifted far up and far down: no write outside [0, cap)
        foreign = PL.in_planes(L, planes, 80.0)[0]
        assert foreign[-1] > 2 * total
        for o in (foreign, foreign + (1 << 40), foreign - (foreign[-1] // 2), want[0][::-1].copy()):
            _upload(ctx, off.ptr, o.astype(np.int64))
            poison()
            R.spheres_in_planes_fill_into(pp, m, K, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
            for g in read():
                assert (g[:guard] == POISON).all() and (g[guard + cap:] == POISON).all()
        # negative offsets everywhere: nothing is written at all
        _upload(ctx, off.ptr, np.arange(-(m + 1) * 10, 0, 10, dtype=np.int64))
        poison()
        R.spheres_in_planes_fill_into(pp, m, K, ps, off.ptr, cap, op[0], op[1], op[2], 0.0, mp, fp)
        for g in read():
            assert (g == POISON).all()
    finally:
        for b in [pbuf, mbuf, fbuf, off] + outs:
            b.free()
        ps.free()


# ---- 11. refusals, n == 0, launch strings under every variant
def test_refusals_and_launch(R, ctx):
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    vp = C.c_void_p
    DB = R.api.DeviceBuffer
    px, mg, fi, off, out = DB(ctx, 16 * 8 * 64), DB(ctx, 4 * 64), DB(ctx, 4 * 64), DB(ctx, 8 * 65), DB(ctx, 8 * 4096)
    try:
        mark_off = np.full(65, -7, np.int64)
        mark_out = np.full(2 * 4096, POISON, np.int32)
        _upload(ctx, off.ptr, mark_off)
        _upload(ctx, out.ptr, mark_out)
        _upload(ctx, px.ptr, np.tile(np.array([0, 1, 0, 1], F), (64 * 8, 1)))
        R.nearest_spheres(ps, np.zeros((5, 3), F), 5, 1.0)
        before = ctx.last_launch
        assert before == "family=nearest k=5"
        h, p, b, o, f = ctx._h, ps._h, vp(px.ptr), vp(off.ptr), vp(out.ptr)
        nan, inf = float("nan"), float("inf")
        cnt, fill = lib.rt_spheres_in_planes_count, lib.rt_spheres_in_planes_fill
        cn, fn = "rt_spheres_in_planes_count", "rt_spheres_in_planes_fill"
        bad = [
            (lambda: cnt(h, None, 64, b, 4, 1.0, None, None, o), "null prepared scene"),
            (lambda: cnt(h, p, -1, b, 4, 1.0, None, None, o), cn + ": query count out of range: 0 <= n < 2^31"),
            (lambda: cnt(h, p, 1 << 31, b, 4, 1.0, None, None, o), cn + ": query count out of range: 0 <= n < 2^31"),
            (lambda: cnt(h, p, 64, b, 0, 1.0, None, None, o), cn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: cnt(h, p, 64, b, 9, 1.0, None, None, o), cn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: cnt(h, p, 64, b, -1, 1.0, None, None, o), cn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: cnt(h, p, 0, b, 9, 1.0, None, None, o), cn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: cnt(h, p, 64, None, 4, 1.0, None, None, o), cn + ": null planes pointer"),
            (lambda: cnt(h, p, 64, b, 4, 1.0, None, None, None), cn + ": null offsets pointer"),
            (lambda: cnt(h, p, 64, b, 4, -1.0, None, None, o), cn + ": need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, 4, nan, None, None, o), cn + ": need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, 4, inf, None, None, o), cn + ": need 0 <= margin <= 1e9, finite"),
            (lambda: cnt(h, p, 64, b, 4, 2e9, None, vp(fi.ptr), o), cn + ": need 0 <= margin <= 1e9, finite"),
            (lambda: fill(h, None, 64, b, 4, 1.0, None, None, o, 4096, f, None, None), "null prepared scene"),
            (lambda: fill(h, p, -1, b, 4, 1.0, None, None, o, 4096, f, None, None), fn + ": query count out of range: 0 <= n < 2^31"),
            (lambda: fill(h, p, 1 << 31, b, 4, 1.0, None, None, o, 4096, f, None, None), fn + ": query count out of range: 0 <= n < 2^31"),
            (lambda: fill(h, p, 64, b, 0, 1.0, None, None, o, 4096, f, None, None), fn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: fill(h, p, 64, b, 9, 1.0, None, None, o, 4096, f, None, None), fn + ": plane count out of range: 1 <= nplanes <= 8"),
            (lambda: fill(h, p, 64, None, 4, 1.0, None, None, o, 4096, f, None, None), fn + ": null planes pointer"),
            (lambda: fill(h, p, 64, b, 4, 1.0, None, None, None, 4096, f, None, None), fn + ": null offsets pointer"),
            (lambda: fill(h, p, 64, b, 4, 1.0, None, None, o, -1, f, None, None), fn + ": negative capacity"),
            (lambda: fill(h, p, 64, b, 4, 1.0, None, None, o, 4096, None, None, None), fn + ": every output is NULL"),
            (lambda: fill(h, p, 64, b, 4, nan, None, None, o, 4096, f, None, None), fn + ": need 0 <= margin <= 1e9, finite"),
            (lambda: fill(h, p, 64, b, 4, -0.5, None, None, o, 4096, None, f, None), fn + ": need 0 <= margin <= 1e9, finite"),
        ]
        for i, (call, text) in enumerate(bad):
            assert call() != 0, i
            assert lib.rt_last_error(h).decode() == text, (i, lib.rt_last_error(h).decode())
        assert ctx.last_launch == before                                      # every refusal leaves the launch string ...
        ctx.sync()
        assert np.array_equal(off.to_host(mark_off.shape, np.int64), mark_off)   # ... and the outputs untouched
        assert np.array_equal(out.to_host(mark_out.shape), mark_out)
        with pytest.raises(R.RtError):
            R.spheres_in_planes(ps, np.ones((4, 2, 4), F), -0.5)
        for shape in ((4, 4), (4, 2, 3), (4, 9, 4), (4, 0, 4)):
            with pytest.raises(ValueError):
                R.spheres_in_planes(ps, np.ones(shape, F), 0.0)
        # a scalar margin is ignored when per-query margins are given
        _upload(ctx, mg.ptr, np.ones(64, F))
        assert cnt(h, p, 64, b, 4, nan, vp(mg.ptr), None, o) == 0
        assert ctx.last_launch == "family=planes count k=4 (per-query)"
        # n == 0: offsets[0] = 0 is still written
        _upload(ctx, off.ptr, mark_off)
        assert cnt(h, p, 0, b, 4, 1.0, None, None, o) == 0
        assert off.to_host((2,), np.int64).tolist() == [0, -7]
        assert fill(h, p, 0, b, 4, 1.0, None, None, o, 0, f, None, None) == 0
        e = R.spheres_in_planes(ps, np.zeros((0, 6, 4), F), 1.0, rows=True)
        assert e[0].tolist() == [0] and e[1].shape == (0,) and e[2].shape == (0,) and e[3].shape == (0,)
        # the launch strings under every variant and at every plane count
        _upload(ctx, fi.ptr, np.zeros(64, np.int32))
        for v in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(v)
            for k in range(1, 9):
                for mgp, fip, tail in ((None, None, ""), (mg.ptr, None, " (per-query)"), (None, fi.ptr, " first"), (mg.ptr, fi.ptr, " (per-query) first")):
                    R.spheres_in_planes_count_into(px.ptr, 64, k, ps, off.ptr, 1.0, mgp, fip)
                    assert ctx.last_launch == f"family=planes count k={k}" + tail
                    R.spheres_in_planes_fill_into(px.ptr, 64, k, ps, off.ptr, 4096, out.ptr, None, None, 1.0, mgp, fip)
                    assert ctx.last_launch == f"family=planes fill k={k}" + tail
            R.spheres_in_planes_fill_into(px.ptr, 64, 4, ps, off.ptr, 4096, None, out.ptr, None, 1.0)   # only the gaps
            R.spheres_in_planes_fill_into(px.ptr, 64, 4, ps, off.ptr, 4096, None, None, out.ptr, 1.0)   # only the rows
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        for x in (px, mg, fi, off, out):
            x.free()
        ps.free()
        scene.free()


def test_multi_device_context_is_refused(R):
    from raytracers_amd._lib import lib
    vp = C.c_void_p
    cnt, fill = lib.rt_spheres_in_planes_count, lib.rt_spheres_in_planes_fill
    # a multi-device context (a device listed twice)
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(64 * 6)
    bp = vp(mb.ptr)
    assert cnt(mc._h, mps._h, 4, bp, 4, 1.0, None, None, bp) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_in_planes_count: a multi-device context is not supported (use a context on one device)"
    assert fill(mc._h, mps._h, 4, bp, 4, 1.0, None, None, bp, 8, bp, None, None) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_spheres_in_planes_fill: a multi-device context is not supported (use a context on one device)"
    mb.free()
    mps.free()
    ms.free()
    mc.close()


# ---- 12. repeatability; planes and outputs as torch tensors, in place
def test_repeatable_and_torch_tensors(R):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = R.Context(0, stream=stream.cuda_stream)
        try:
            s = _random_spheres(20000, 91, 0.5, 3.0)
            ps = R.prepare_scene_from_spheres(c, s, 64, 64, *VIEW)
            L = ps.bvh_arrays()["L"]
            m, K = 1024, 6
            planes = PL.random_planes(L, m, K, 5)
            a, b = R.spheres_in_planes(ps, planes, 1.5, rows=True), R.spheres_in_planes(ps, planes, 1.5, rows=True)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            want = PL.in_planes(L, planes, 1.5)
            _same(a[:3], want, "20000 spheres")
            pt = torch.as_tensor(planes, device="cuda")
            _same(R.spheres_in_planes(ps, pt, 1.5), want, "planes as a device tensor")
            with pytest.raises(ValueError):
                R.spheres_in_planes(ps, pt.double(), 1.5)
            with pytest.raises(ValueError):
                R.spheres_in_planes(ps, pt[:, :, :3], 1.5)
            # outputs allocated by torch on the context's stream, in place
            off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            R.spheres_in_planes_count_into(pt.data_ptr(), m, K, ps, off.data_ptr(), 1.5)
            total = int(off[m].item())
            assert total == want[0][-1]
            idx = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            gap = torch.full((total + 64,), -3.0, dtype=torch.float32, device="cuda")
            row = torch.full((total + 64,), -3, dtype=torch.int32, device="cuda")
            R.spheres_in_planes_fill_into(pt.data_ptr(), m, K, ps, off.data_ptr(), total, idx.data_ptr(), gap.data_ptr(), row.data_ptr(), 1.5)
            stream.synchronize()
            _same((off.cpu().numpy(), idx[:total].cpu().numpy(), gap[:total].cpu().numpy()), want, "torch outputs")
            assert np.array_equal(row[:total].cpu().numpy(), np.repeat(np.arange(m, dtype=np.int32), np.diff(want[0])))
            assert (idx[total:] == -3).all() and (gap[total:] == -3.0).all() and (row[total:] == -3).all()
            ps.free()
        finally:
            c.close()
