"""Contact clusters on the GPU: rt_contact_clusters against the restatement (clusters_ref.py: a union-find over within_ref's pair rows) AND
against a union-find over the GPU's own rt_contact_pairs_fill rows, with == throughout, on the shapes at which each mechanism can break: the
reference's scenes, the last block's tail, chains (the deepest trees) in and out of L order, interleaved chains, a coincident clique (every
lane on one word), isolated spheres, a point cloud near percolation, non-finite and out-of-range spheres, tall BVHs; every combination of
the optional outputs; poisoned, 4-byte-misaligned torch outputs; repeatability on one and two contexts; update_spheres; cluster_members;
refusals and the launch string."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clusters_ref as K
from test_proximity_gpu import VIEW, _geometric, _random_spheres

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


def _spheres(centres, radius):
    s = np.zeros((len(centres), 7), F)
    s[:, :3] = centres
    s[:, 3:6] = 0.5
    s[:, 6] = radius
    return s


def _prepare(R, ctx, s):
    return R.prepare_scene_from_spheres(ctx, s, 64, 64, *VIEW)


def _same(got, want, what):
    for name, g, w in zip(("root", "cluster", "size"), got[:3], want[:3]):
        assert g.dtype == np.int32 and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape}"
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first {bad[:5]}: got {g[bad[:5]]} want {w[bad[:5]]}"
    assert got[3] == want[3], f"{what}: num {got[3]} != {want[3]}"


def _check(R, ctx, ps, margin, what, near=None):
    """contact_clusters == the restatement over L == a union-find over the GPU's own contact pairs"""
    L = ps.bvh_arrays()["L"]
    n = L.shape[0]
    near = n > 4000 if near is None else near
    want = K.clusters(L, margin, near=near)
    got = R.contact_clusters(ps, margin)
    assert ctx.last_launch == "family=clusters", ctx.last_launch
    _same(got, want, what)
    pairs = R.contact_pairs(ps, margin, gaps=False)[0]
    _same(got, K.from_roots(K.roots_union_find(n, pairs)), what + " (the GPU's own pairs)")
    return got


# ---- the reference's scenes
@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_reference_scenes(R, ctx, spec):
    scene = ctx.scene(spec)
    ps = R.prepare_scene(100, 100, scene)
    nums = [_check(R, ctx, ps, margin, f"{spec} margin={margin}")[3] for margin in (0.0, 0.5, 2.0)]
    assert nums[0] >= nums[1] >= nums[2] >= 1
    ps.free()
    scene.free()


# ---- the last block's tail
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_small_scenes(R, ctx, n):
    s = _random_spheres(max(n, 2), 100 + n)[:n]
    if n == 1:
        # a prepared scene has at least two spheres: the one-sphere answer of the launcher (root = {0}, num = 1, no walk) cannot be reached
        # through the public surface.  Should that limit ever go, this case checks the answer.
        try:
            ps = _prepare(R, ctx, s)
        except R.RtError as e:
            assert "2 .. 2^26" in str(e) or "at least 2" in str(e), str(e)
            return
        root, cluster, size, num = R.contact_clusters(ps, 0.0)
        assert root.tolist() == [0] and cluster.tolist() == [0] and size.tolist() == [1] and num == 1
        ps.free()
        return
    ps = _prepare(R, ctx, s)
    seen = set()
    for margin in (0.0, 3.0, 12.0, 1e9):
        seen.add(_check(R, ctx, ps, margin, f"random:{n} margin={margin}")[3])
    assert 1 in seen and (n < 63 or len(seen) > 2)          # margin 1e9: one cluster; the partitions differ with the margin
    ps.free()


# ---- chains: the deepest trees
def _line(n):
    c = np.zeros((n, 3))
    c[:, 0] = 2.0 * np.arange(n) - n                       # unit spheres 2 apart: gap 1 <= 1 + 0, exactly, to the neighbours only
    return c


def _zigzag(n, seed):
    """the same chain with every other step along +-y in seeded runs: neighbours 2 apart, the Morton order is not the chain's"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 3))
    up, left = 1.0, 0
    for k in range(1, n):
        c[k] = c[k - 1]
        if k % 2:
            c[k, 0] += 2.0
        else:
            if left == 0:
                up, left = -up, int(rng.integers(3, 40))
            c[k, 1] += 2.0 * up
            left -= 1
    c[:, 0] -= 2.0 * round(c[:, 0].mean() / 2.0)            # (integers: every distance stays exact in float32)
    return c


def test_chains(R, ctx):
    n = 4097
    ps = _prepare(R, ctx, _spheres(_line(n), 1.0))
    root, cluster, size, num = _check(R, ctx, ps, 0.0, "line chain", near=True)
    assert num == 1 and not root.any() and (size == n).all()
    pairs = R.contact_pairs(ps, 0.0, gaps=False)[0]
    assert pairs.shape[0] == n - 1                          # each sphere touches only its neighbours
    ps.free()
    ps = _prepare(R, ctx, _spheres(_zigzag(n, 5), 1.0))
    ids = ps.sphere_ids()
    assert np.count_nonzero(np.abs(np.diff(ids.astype(np.int64))) > 1) > n // 8      # L order is not chain order
    root, cluster, size, num = _check(R, ctx, ps, 0.0, "zigzag chain", near=True)
    assert num == 1 and not root.any() and (size == n).all()
    ps.free()
    # two chains that never touch, side by side along x (3 apart in y, shifted by 1 in x); the first goes on along -y for as long again, so
    # that the scene is as deep as it is wide and the chains differ only in the low bits of their Morton keys: alternating members along L
    a, b = _line(2048), _line(2048)
    b[:, 0] += 1.0
    b[:, 1] += 3.0
    arm = np.zeros((2048, 3))
    arm[:, 0] = a[-1, 0] + 2.0
    arm[:, 1] = -2.0 * np.arange(2048)
    ps = _prepare(R, ctx, _spheres(np.concatenate([a, arm, b]), 1.0))
    root, cluster, size, num = _check(R, ctx, ps, 0.0, "two chains", near=True)
    assert num == 2 and sorted(np.unique(size).tolist()) == [2048, 4096] and sorted(set(root.tolist())) == [0, int(root.max())]
    assert np.count_nonzero(np.diff(cluster)) > 512, np.count_nonzero(np.diff(cluster))
    ps.free()


# ---- every lane of every wave contending on one word; no edge at all
def test_clique_and_isolated(R, ctx):
    n = 1000
    ps = _prepare(R, ctx, _spheres(np.tile([[1.5, -2.0, 3.25]], (n, 1)), 1.0))
    root, cluster, size, num = _check(R, ctx, ps, 0.0, "coincident clique")
    assert num == 1 and not root.any() and not cluster.any() and (size == n).all()
    assert R.contact_pairs(ps, 0.0, gaps=False)[0].shape[0] == n * (n - 1) // 2
    ps.free()
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3) * 10.0 - 45.0
    ps = _prepare(R, ctx, _spheres(g, 1.0))
    root, cluster, size, num = _check(R, ctx, ps, 0.0, "isolated")
    ar = np.arange(n, dtype=np.int32)
    assert num == n and np.array_equal(root, ar) and np.array_equal(cluster, ar) and (size == 1).all()
    assert _check(R, ctx, ps, 8.0, "isolated, margin 8")[3] == 1        # 10 apart: gap 9 <= 1 + 8
    ps.free()


# ---- friends of friends: radius 0, the margin is the linking length, near the percolation threshold
def test_point_cloud(R, ctx):
    rng = np.random.default_rng(20)
    ps = _prepare(R, ctx, _spheres(rng.uniform(0.0, 100.0, (20000, 3)), 0.0))
    root, cluster, size, num = _check(R, ctx, ps, 3.2, "cloud", near=True)
    assert size.min() == 1 and size.max() > 1000 and 1000 < num < 10000
    assert np.unique(size).size > 30                        # sizes from singletons to thousands
    ps.free()


def test_million_point_cloud(R, ctx):
    """the same density at 10^6 points: long finds under full occupancy, and the in-place flatten racing with itself (a flatten that still
    halved paths left non-roots in `root` here).  Held to the invariants and to a union-find over the GPU's own pair rows."""
    n = 1000000
    rng = np.random.default_rng(3)
    ps = _prepare(R, ctx, _spheres(rng.uniform(0.0, 100.0 * 50.0 ** (1.0 / 3.0), (n, 3)), 0.0))
    root, cluster, size, num = R.contact_clusters(ps, 3.2)
    again = R.contact_clusters(ps, 3.2)
    assert all(np.array_equal(a, b) for a, b in zip((root, cluster, size), again[:3])) and num == again[3]
    ar = np.arange(n, dtype=np.int32)
    assert np.array_equal(root[root], root) and (root <= ar).all()
    roots = np.nonzero(root == ar)[0]
    assert num == roots.size and np.array_equal(cluster, np.searchsorted(roots, root).astype(np.int32))
    assert np.array_equal(size, np.bincount(root, minlength=n)[root]) and size.max() > 10000 and size.min() == 1
    pairs = R.contact_pairs(ps, 3.2, gaps=False)[0]
    assert pairs.shape[0] > n and np.array_equal(root[pairs[:, 0]], root[pairs[:, 1]])
    assert np.array_equal(root, K.roots_union_find(n, pairs))
    ps.free()


# ---- spheres that offer no edge from their own side
def test_non_finite_and_out_of_range_spheres(R, ctx):
    import proximity_ref as P
    s = _random_spheres(600, 17)
    s[5, 0] = np.nan
    s[40, 1] = np.inf
    s[41, 2] = -np.inf
    s[90, 6] = np.nan
    s[130, 6] = 2e9                                         # radius + margin past 1e9: edgeless as i, inside reach of every lower i as j
    s[131, 6] = 9.9999994e8                                 # a valid bound at margin 0, not at margin 100
    s[200:210, 6] = 0.0
    ps = _prepare(R, ctx, s)
    L = ps.bvh_arrays()["L"]
    bad_centre = ~P.point_ok(L[:, :3])
    assert bad_centre.sum() == 3
    for margin in (0.0, 1.0, 100.0):
        root, cluster, size, num = _check(R, ctx, ps, margin, f"non-finite margin={margin}", near=False)
        # a non-finite centre gives a NaN or +inf gap from every side: a singleton
        assert (size[bad_centre] == 1).all() and np.array_equal(root[bad_centre], np.nonzero(bad_centre)[0])
    ps.free()


def test_tall_trees(R, ctx):
    import edge_rays as E
    for what, s, view in (("tall1100", E.SCENES["tall1100"][0], E.SCENES["tall1100"][1:]), ("geometric", _geometric(120, 3), VIEW)):
        ps = R.prepare_scene_from_spheres(ctx, s, 64, 64, *view)
        assert ps.height > int(np.log2(np.float32(s.shape[0]))) + 2, (what, ps.height)      # partial boxes near the root
        for margin in (0.0, 1.0, 60.0):
            _check(R, ctx, ps, margin, f"{what} margin={margin}", near=False)
        ps.free()


# ---- the optional outputs; poisoned torch tensors, misaligned by 4 bytes
def test_optional_outputs_into_poisoned_tensors(R, ctx):
    import torch
    n = 5000
    ps = _prepare(R, ctx, _random_spheres(n, 55, 0.5, 3.0))
    want = K.clusters(ps.bvh_arrays()["L"], 1.0, near=True)
    assert 1 < want[3] < n
    for with_cluster, with_size, with_num in itertools.product((False, True), repeat=3):
        t = [torch.full((n + 3,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
        num = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        root, cluster, size = (x[1:n + 1] for x in t)
        assert root.data_ptr() % 8 == 4 and (num.data_ptr() + 4) % 8 == 4
        torch.cuda.synchronize()
        R.contact_clusters_into(ps, root.data_ptr(), cluster.data_ptr() if with_cluster else None, size.data_ptr() if with_size else None,
                                num.data_ptr() + 4 if with_num else None, 1.0)
        assert ctx.last_launch == "family=clusters"
        ctx.sync()
        what = f"outputs cluster={with_cluster} size={with_size} num={with_num}"
        assert np.array_equal(root.cpu().numpy(), want[0]), what
        assert np.array_equal(cluster.cpu().numpy(), want[1] if with_cluster else np.full(n, -7, np.int32)), what
        assert np.array_equal(size.cpu().numpy(), want[2] if with_size else np.full(n, -7, np.int32)), what
        assert num.cpu().numpy().tolist() == ([-7, want[3], 0, -7] if with_num else [-7] * 4), what
        for x in t:                                         # the guards on both sides
            assert x[0].item() == -7 and (x[n + 1:] == -7).all().item(), what
    ps.free()


# ---- the same answer from run to run, and on another context
def test_repeatable_on_two_contexts(R, ctx):
    s = _random_spheres(20000, 91, 0.5, 3.0)
    ps = _prepare(R, ctx, s)
    a, b = R.contact_clusters(ps, 2.0), R.contact_clusters(ps, 2.0)
    other = R.Context(0)
    try:
        ps2 = _prepare(R, other, s)
        c = R.contact_clusters(ps2, 2.0)
        assert other.last_launch == "family=clusters"
        ps2.free()
    finally:
        other.close()
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[3] == b[3] == c[3]
    _same(a, K.clusters(ps.bvh_arrays()["L"], 2.0, near=True), "20000 random spheres")
    ps.free()


# ---- clusters follow update_spheres; the member lists; the caller's order
def test_update_spheres_and_members(R, ctx):
    s = _random_spheres(3000, 31, 0.5, 3.0)
    ps = _prepare(R, ctx, s)
    before = _check(R, ctx, ps, 1.0, "before the update")
    s2 = s.copy()
    s2[:, :3] += np.random.default_rng(77).normal(0.0, 1.5, (3000, 3)).astype(F)
    ps.update_spheres(s2)
    fresh = _prepare(R, ctx, s2)
    assert ps.bvh_arrays()["L"].tobytes() == fresh.bvh_arrays()["L"].tobytes()
    after = _check(R, ctx, ps, 1.0, "after the update")
    _same(after, R.contact_clusters(fresh, 1.0), "updated == freshly prepared")
    assert not np.array_equal(after[0], before[0])
    root, cluster, size, num = after
    off, mem = R.cluster_members(cluster, num)
    assert off.shape == (num + 1,) and off[-1] == 3000 and np.array_equal(np.diff(off), size[root == np.arange(3000)])
    for c in (0, num // 2, num - 1, int(cluster[np.argmax(size)])):
        m = mem[off[c]:off[c + 1]]
        assert (np.diff(m) > 0).all() and (cluster[m] == c).all() and (root[m] == m[0]).all()
    back = np.empty(3000, np.int32)
    back[mem] = np.repeat(np.arange(num, dtype=np.int32), np.diff(off))
    assert np.array_equal(back, cluster)
    # in the caller's order: spheres of one cluster are connected through touching spheres of s2 (checked on the largest cluster's edges)
    ids = ps.sphere_ids()
    pairs = R.contact_pairs(ps, 1.0, gaps=False)[0]
    label = np.empty(3000, np.int32)
    label[ids] = cluster
    assert (label[ids[pairs[:, 0]]] == label[ids[pairs[:, 1]]]).all()
    fresh.free()
    ps.free()


# ---- the refusals one by one, their text, the launch string
def test_refusals_and_launch(R, ctx):
    from raytracers_amd._lib import lib
    scene = ctx.scene("rgbbox")
    ps = R.prepare_scene(64, 64, scene)
    n = ps.num_spheres
    vp = C.c_void_p
    out = R.api.DeviceBuffer(ctx, 4 * 3 * n + 8)
    try:
        mark = np.full(3 * n + 2, 0x5A5A5A5A, np.int32)
        ctx._check(lib.rt_copy_to_device(ctx._h, vp(out.ptr), mark.ctypes.data, mark.nbytes))
        R.nearest_spheres(ps, np.zeros((5, 3), F), 5, 1.0)
        before = ctx.last_launch
        assert before == "family=nearest k=5"
        h, p = ctx._h, ps._h
        r, c, s, m = vp(out.ptr), vp(out.ptr + 4 * n), vp(out.ptr + 8 * n), vp(out.ptr + 12 * n)
        nan, inf = float("nan"), float("inf")
        fn = lib.rt_contact_clusters
        margin_text = "rt_contact_clusters: need 0 <= margin <= 1e9, finite"
        for args, text in (((h, None, 0.0, r, c, s, m), "null prepared scene"),
                           ((h, p, 0.0, None, c, s, m), "rt_contact_clusters: null root pointer"),
                           ((h, p, -1.0, r, c, s, m), margin_text),
                           ((h, p, nan, r, c, s, m), margin_text),
                           ((h, p, inf, r, c, s, m), margin_text),
                           ((h, p, -inf, r, c, s, m), margin_text),
                           ((h, p, 2e9, r, c, s, m), margin_text),
                           ((h, p, 1.0000001e9, r, c, s, m), margin_text)):
            assert fn(*args) != 0, text
            assert lib.rt_last_error(h).decode() == text
        assert fn(None, p, 0.0, r, c, s, m) != 0
        assert ctx.last_launch == before                                        # every refusal leaves the launch string ...
        assert np.array_equal(out.to_host(mark.shape), mark)                    # ... and the outputs untouched
        with pytest.raises(R.RtError):
            R.contact_clusters(ps, float("nan"))
        with pytest.raises(R.RtError):
            R.contact_clusters_into(ps, None)
        # -0.0 counts as 0, and 1e9 is inside the range: one cluster
        a, b = R.contact_clusters(ps, -0.0), R.contact_clusters(ps, 0.0)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        assert R.contact_clusters(ps, 1e9)[3] == 1
        for v in (R.VARIANT_AUTO, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(v)
            R.nearest_spheres(ps, np.zeros((5, 3), F), 5, 1.0)
            R.contact_clusters_into(ps, out.ptr, None, None, out.ptr + 12 * n, 0.5)
            assert ctx.last_launch == "family=clusters"
            ctx.sync()
    finally:
        ctx.set_variant(R.VARIANT_AUTO)
        out.free()
        ps.free()
        scene.free()


def test_multi_device_context_is_refused(R):
    from raytracers_amd._lib import lib
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    mb = mc.alloc_i32(4 * mps.num_spheres + 2)
    bp = C.c_void_p(mb.ptr)
    assert lib.rt_contact_clusters(mc._h, mps._h, 0.0, bp, None, None, None) != 0
    assert lib.rt_last_error(mc._h).decode() == "rt_contact_clusters: a multi-device context is not supported (use a context on one device)"
    mb.free()
    mps.free()
    ms.free()
    mc.close()
