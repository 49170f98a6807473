"""CPU checks of the sphere groups: the restatement (groups_ref.py) against itself -- the dense definitions against the stack walk that prunes by
node words, on rgbbox, irreg and a tall chain --, the gather through ids, node_groups by recursion against the derive kernel's climb in several
orders, the rule, combine and climb of query_core.h through build/groups_check (and once more under the address and undefined-behaviour
sanitizers), wrong variants (mutants) each caught by a named input, the selectivity premise of the GPU tests' inputs, and the library's
symbols, header and Python surface.  No GPU needed."""
import ctypes as C
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import groups_ref as G
import occlusion_ref as X
import oracle_lib as O
import proximity_ref as P
import ray_query_ref as Q
import within_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
SCENES = ("rgbbox", "irreg", "tall")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _input_spheres(osc):
    return np.ctypeslib.as_array(C.cast(osc.scene.spheres, C.POINTER(C.c_float)), shape=(osc.n, 7)).copy()


def _ids(spheres, L):
    """ids[i] = the input's index of L[i]: the stable Morton sort keeps equal spheres in input order"""
    where = {}
    for c in range(spheres.shape[0] - 1, -1, -1):
        where.setdefault(spheres[c].tobytes(), []).append(c)
    return np.array([where[L[i].tobytes()].pop() for i in range(L.shape[0])], np.int64)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(MaskedScene, arrays, the input spheres in the caller's order, ids)"""
    if name == "tall":
        osc = O.OracleScene("custom", spheres7=G.tall_chain(), look_from=G.TALL_VIEW[0], look_at=G.TALL_VIEW[1], fov=G.TALL_VIEW[2])
    else:
        osc = O.OracleScene(name)
    arr = osc.arrays()
    s = _input_spheres(osc)
    with np.errstate(divide="ignore"):
        ref = G.MaskedScene(arr)
    ref.keep = osc
    return ref, arr, s, _ids(s, arr["L"])


def _rays(name, n_seeded=192, side=8):
    ref, arr, s, ids = _scene(name)
    cam = ref.keep.camera_floats(side, side)
    # (and rays aimed at spheres, so that the tall chain's small spheres are hit too)
    rng = np.random.default_rng(29)
    L = arr["L"]
    j = rng.integers(0, L.shape[0], 64)
    off = rng.normal(size=(64, 3))
    off *= (3.0 * L[j, 6:7] + 1e-3) / np.linalg.norm(off, axis=1)[:, None]
    aimed = np.concatenate([L[j, :3] + off, -off * rng.uniform(0.5, 2.0, (64, 1))], axis=1)
    return np.concatenate([Q.camera_rays(cam, side, side), X.seeded_rays(arr, n_seeded, 7), aimed]).astype(F)


def _points(arr, m, seed):
    rng = np.random.default_rng(seed)
    L = arr["L"]
    lo, hi = L[:, :3].min(axis=0).astype(np.float64), L[:, :3].max(axis=0).astype(np.float64)
    p = rng.uniform(lo, hi, (m, 3)).astype(F)
    j = rng.integers(0, L.shape[0], m // 2)
    p[: j.size] = L[j, :3]
    return p


def _box(arr):
    """the scene's box, spheres included (occlusion_ref.seeded_rays' box without its padding)"""
    L = arr["L"]
    return (L[:, :3] - L[:, 6:7]).min(axis=0).astype(np.float64), (L[:, :3] + L[:, 6:7]).max(axis=0).astype(np.float64)


def _extent(arr):
    """the longest side of that box"""
    lo, hi = _box(arr)
    return float(np.max(hi - lo))


# ------------------------------------------------------------------------------------------------------------- the inputs
def test_the_tall_chain_is_tall():
    ref, arr, s, ids = _scene("tall")
    n = s.shape[0]
    sweeps = int(np.log2(F(n))) + 2
    # (taller than the AABB propagation's sweeps: the boxes nearest the root are left partial, and the proximity walks do not test them)
    assert G.levels(arr["left"], arr["right"]) > sweeps + 4, G.levels(arr["left"], arr["right"])


@pytest.mark.parametrize("name", SCENES)
def test_ids_are_a_permutation_that_is_not_the_identity(name):
    ref, arr, s, ids = _scene(name)
    assert np.array_equal(np.sort(ids), np.arange(s.shape[0])) and (ids != np.arange(s.shape[0])).any()
    assert np.array_equal(s[ids], arr["L"])


# ------------------------------------------------------------------------------------------------------------- gather and node words
@pytest.mark.parametrize("name", SCENES)
def test_gather_and_node_groups(name):
    ref, arr, s, ids = _scene(name)
    n = s.shape[0]
    left, right, parent = arr["left"], arr["right"], arr["parent"]
    for pname, words in G.patterns(s, 5).items():
        g = G.gather(words, ids)
        assert all(g[i] == words[ids[i]] for i in range(0, n, max(1, n // 97)))
        ng = G.node_groups(left, right, g)
        assert ng[0] == np.bitwise_or.reduce(g), pname
        # every node's word is the OR of its children's: the definition, node by node
        wl = np.where(left < 0, g[np.clip(-2 - left, 0, n - 1)], ng[np.clip(left, 0, n - 2)])
        wr = np.where(right < 0, g[np.clip(-2 - right, 0, n - 1)], ng[np.clip(right, 0, n - 2)])
        assert np.array_equal(ng, wl | wr), pname
        # the derive kernel's climb, in three orders of the nodes
        rng = np.random.default_rng(11)
        for order in (None, range(n - 2, -1, -1), rng.permutation(n - 1)):
            assert np.array_equal(G.node_groups_climb(left, right, parent, g, order), ng), pname
        lv = G.levels(left, right)
        assert np.array_equal(G.node_groups_sweeps(left, right, g, lv), ng), pname


# ------------------------------------------------------------------------------------------------------------- pruning changes nothing
@pytest.mark.parametrize("pname", ["random", "octant", "bit31_on_one", "all_zero"])
@pytest.mark.parametrize("name", SCENES)
def test_pruning_changes_no_ray_answer(name, pname):
    ref, arr, s, ids = _scene(name)
    rays = _rays(name)
    g = G.gather(G.patterns(s, 5)[pname], ids)
    masks = G.mixed_masks(rays.shape[0], 13)
    if pname == "bit31_on_one":
        masks[::2] = 0x80000000
    lo, hi = (0.0, 1e9) if pname != "octant" else (F(0.1), F(0.3 * _extent(arr)))
    dense = G.objs_hit(ref, rays, lo, hi, g, masks)
    dense_occ = G.occluded(ref, rays, lo, hi, g, masks)
    for prune in (True, False):
        assert _same(G.objs_hit(ref, rays, lo, hi, g, masks, walk=True, prune=prune), dense), (name, pname, prune)
        assert np.array_equal(G.occluded(ref, rays, lo, hi, g, masks, walk=True, prune=prune), dense_occ), (name, pname, prune)
    # ... and the masks matter on these inputs (all_zero: nothing is seen at all)
    plain = ref.objs_hit(rays[:, :3], rays[:, 3:], lo, hi)
    if pname == "all_zero":
        assert (dense[0] == -1).all() and not dense_occ.any()
    elif pname == "random":
        assert (dense[0] != plain[0]).any() and (dense[0] >= 0).any()
    # a scalar mask of all ones on words without a zero: the unmasked answer
    if pname == "octant":
        assert _same(G.objs_hit(ref, rays, lo, hi, g, 0xFFFFFFFF), plain)


@pytest.mark.parametrize("pname", ["random", "octant", "bit31_on_one"])
@pytest.mark.parametrize("name", SCENES)
def test_pruning_changes_no_proximity_answer(name, pname):
    ref, arr, s, ids = _scene(name)
    L = arr["L"]
    p = _points(arr, 96, 3)
    g = G.gather(G.patterns(s, 5)[pname], ids)
    masks = G.mixed_masks(p.shape[0], 17)
    md = 0.05 * _extent(arr)
    first = np.random.default_rng(2).integers(-3, L.shape[0] + 3, p.shape[0])
    for fi in (None, first):
        dense = G.within(L, p, md, g, masks, fi)
        for prune in (True, False):
            assert _same(G.within_walk(ref, p, md, g, masks, fi, prune=prune), dense), (name, pname, prune)
    # nearest is within, re-sorted by (gap, index) and cut at k
    off, idx, gap = G.within(L, p, md, g, masks)
    for k in (1, 5, 32):
        assert _same(G.nearest(L, p, md, k, g, masks), G.nearest_from_rows(p.shape[0], k, off, idx, gap)), (name, pname, k)
    # all ones on every word: the unmasked restatements
    ones = np.full(L.shape[0], 0xFFFFFFFF, U)
    assert _same(G.within(L, p, md, ones, 0x80000000), W.within(L, p, md))
    assert _same(G.nearest(L, p, md, 8, ones, 1), P.nearest(L, p, md, 8))


# ------------------------------------------------------------------------------------------------------------- C++ rule, combine and climb
def _check_file(name, tmp_path):
    ref, arr, s, ids = _scene(name)
    n = s.shape[0]
    rng = np.random.default_rng(19)
    g = G.gather(G.patterns(s, 5)["random"], ids)
    g[:: 7] = U(1) << rng.integers(0, 32, g[::7].size).astype(U)
    pairs = rng.integers(0, 2 ** 32, (4000, 2), dtype=np.uint64).astype(U)
    pairs[:500, 0] = U(1) << rng.integers(0, 32, 500).astype(U)
    pairs[250:1000, 1] = U(1) << rng.integers(0, 32, 750).astype(U)
    pairs[1000:1010] = [[0x80000000, 0x80000000], [0x80000000, 0x7FFFFFFF], [0, 0], [0, 0xFFFFFFFF], [0xFFFFFFFF, 0], [3, 1], [1, 3],
                        [0xFFFFFFFF, 0xFFFFFFFF], [0x80000001, 0x80000000], [0x40000000, 0x80000000]]
    order = rng.permutation(n - 1)
    words = np.concatenate([[pairs.shape[0]], pairs.reshape(-1), [n], arr["left"].view(U), arr["right"].view(U), arr["parent"].view(U), g,
                            order.astype(U)]).astype(U)
    src = tmp_path / "groups_cases.bin"
    words.tofile(src)
    return src, pairs, g, arr


def _run_check(exe, src, dst):
    if not os.path.exists(os.path.join(ROOT, exe)):
        subprocess.run(["make", "-C", ROOT, exe], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, exe), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(dst, dtype=U)


@pytest.mark.parametrize("name", SCENES)
def test_groups_check_agrees_with_the_restatement(name, tmp_path):
    src, pairs, g, arr = _check_file(name, tmp_path)
    out = _run_check("build/groups_check", src, tmp_path / "out.bin")
    P_ = pairs.shape[0]
    got = out[: 2 * P_].reshape(-1, 2)
    want_seen = np.array([G.seen(pairs[i:i + 1, 0], pairs[i, 1])[0, 0] for i in range(P_)])
    assert np.array_equal(got[:, 0].astype(bool), want_seen)
    assert np.array_equal(got[:, 1], pairs[:, 0] | pairs[:, 1])
    assert want_seen.sum() > 100 and (~want_seen).sum() > 100
    assert np.array_equal(out[2 * P_:], G.node_groups(arr["left"], arr["right"], g))


def test_groups_check_under_the_sanitizers(tmp_path):
    src, pairs, g, arr = _check_file("tall", tmp_path)
    out = _run_check("build/asan/groups_check", src, tmp_path / "out_asan.bin")
    assert np.array_equal(out[2 * pairs.shape[0]:], G.node_groups(arr["left"], arr["right"], g))


# ------------------------------------------------------------------------------------------------------------- mutants
def _mutant_case(mutant):
    """(scene, caller-order words, masks, rays) of the named input that catches `mutant`"""
    if mutant == "rule_all_bits":          # a mask of two bits against single-bit words
        ref, arr, s, ids = _scene("rgbbox")
        return "rgbbox", G.patterns(s, 5)["bit_c_mod_32"], 0x3, None
    if mutant == "rule_signed":            # bit 31
        ref, arr, s, ids = _scene("rgbbox")
        return "rgbbox", np.full(s.shape[0], 0x80000000, U), 0x80000000, None
    if mutant == "node_groups_short":      # the tall chain, its deepest leaves alone in their group
        ref, arr, s, ids = _scene("tall")
        words = np.ones(s.shape[0], U)
        depth = _leaf_depths(arr)
        words[ids[depth >= depth.max() - 1]] = 0x80000000
        return "tall", words, 0x80000000, None
    if mutant == "no_gather":              # ids is not the identity
        ref, arr, s, ids = _scene("irreg")
        return "irreg", G.patterns(s, 5)["bit_c_mod_32"], 0x5, None
    if mutant == "sibling_word":           # sibling leaves in different groups
        ref, arr, s, ids = _scene("rgbbox")
        return "rgbbox", G.patterns(s, 5)["random"], 0x1, None
    raise ValueError(mutant)


def _leaf_depths(arr):
    left, right = arr["left"], arr["right"]
    depth = np.zeros(left.size + 1, np.int64)
    frontier, d = [0], 0
    while frontier:
        d += 1
        nxt = []
        for v in frontier:
            for c in (int(left[v]), int(right[v])):
                if c < 0:
                    depth[-2 - c] = d
                else:
                    nxt.append(c)
        frontier = nxt
    return depth


def _walk_answers(name, words, masks, mutant):
    """the walk's answers under `mutant` next to the dense definition's, for the scene's seeded rays and points"""
    ref, arr, s, ids = _scene(name)
    g_true = G.gather(words, ids)
    g = G.gather(words, ids, mutant)
    ng = G.node_groups(arr["left"], arr["right"], g)
    if mutant == "node_groups_short":
        ng = G.node_groups_sweeps(arr["left"], arr["right"], g, G.levels(arr["left"], arr["right"]) - 1)
    rays = _rays(name, 128, 8)
    p = _points(arr, 64, 3)
    md = 0.2 * _extent(arr)
    dense = (G.objs_hit(ref, rays, 0.0, 1e9, g_true, masks), G.within(arr["L"], p, md, g_true, masks))
    walk = (G.objs_hit(ref, rays, 0.0, 1e9, g, masks, walk=True, ngroups=ng, mutant=mutant),
            G.within_walk(ref, p, md, g, masks, ngroups=ng, mutant=mutant))
    return dense, walk


def test_the_walk_passes_on_the_mutants_inputs():
    for mutant in G.MUTANTS:
        name, words, masks, _ = _mutant_case(mutant)
        dense, walk = _walk_answers(name, words, masks, None)
        assert _same(walk[0], dense[0]) and _same(walk[1], dense[1]), mutant
        assert (dense[0][0] >= 0).any() or dense[1][1].size > 0, mutant


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_mutants_are_caught(mutant):
    name, words, masks, _ = _mutant_case(mutant)
    dense, walk = _walk_answers(name, words, masks, mutant)
    rays_differ = not _same(walk[0], dense[0])
    rows_differ = not _same(walk[1], dense[1])
    print(f"{mutant}: {name}: rays differ {rays_differ}, rows differ {rows_differ}")
    assert rows_differ, mutant   # (every named input is caught by the range query: it sees every sphere within its bound)


def test_the_rule_mutants_differ_from_the_rule_where_named():
    assert G.seen([0x80000000], 0x80000000)[0, 0] and not G.seen([0x80000000], 0x80000000, "rule_signed")[0, 0]
    assert G.seen([1], 3)[0, 0] and not G.seen([1], 3, "rule_all_bits")[0, 0]
    assert not G.seen([0xFFFFFFFF], 0)[0, 0] and not G.seen([0], 0xFFFFFFFF)[0, 0]


# ------------------------------------------------------------------------------------------------------------- the selectivity premise
@pytest.mark.parametrize("name", ["rgbbox", "irreg"])
def test_selectivity_premise(name):
    """Group words 1 << (j % 4) in L order, mask 1: at least 20 % of the rays get another index than unmasked, at least 10 % still hit; and the
    masked nearest counts differ from the unmasked ones on more than a third of 256 uniform points at max_dist = 0.05 x extent."""
    ref, arr, s, ids = _scene(name)
    n = s.shape[0]
    g = (U(1) << (np.arange(n) % 4).astype(U)).astype(U)
    cam = ref.keep.camera_floats(32, 32)
    rays = np.concatenate([Q.camera_rays(cam, 32, 32), X.seeded_rays(arr, 1024, 7)]).astype(F)
    plain = ref.objs_hit(rays[:, :3], rays[:, 3:], 0.0, 1e9)[0]
    masked = G.objs_hit(ref, rays, 0.0, 1e9, g, 1)[0]
    changed, hit = float((masked != plain).mean()), float((masked >= 0).mean())
    print(f"{name}: changed {changed:.3f}, masked hits {hit:.3f}")
    assert changed >= 0.20 and hit >= 0.10
    L = arr["L"]
    rng = np.random.default_rng(7)
    lo, hi = _box(arr)
    p = rng.uniform(lo, hi, (256, 3)).astype(F)
    md = 0.05 * _extent(arr)
    differ = float((G.nearest(L, p, md, 1, g, 1)[0] != P.nearest(L, p, md, 1)[0]).mean())
    print(f"{name}: nearest counts differ on {differ:.3f}")
    assert differ > 1.0 / 3.0


# ------------------------------------------------------------------------------------------------------------- the interface
NEW_SYMBOLS = ("rt_prepared_set_groups", "rt_prepared_get_groups", "rt_intersect_rays_masked", "rt_occluded_rays_masked",
               "rt_nearest_spheres_masked", "rt_spheres_within_masked_count", "rt_spheres_within_masked_fill")


def test_library_exports_groups():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in NEW_SYMBOLS:
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert [len(getattr(_lib.lib, s).argtypes) for s in NEW_SYMBOLS] == [4, 4, 12, 11, 12, 10, 14]
    for name in ("intersect_rays_masked_into", "occluded_rays_masked_into", "nearest_spheres_masked_into", "spheres_within_masked_count_into",
                 "spheres_within_masked_fill_into"):
        assert callable(getattr(R, name)), name
    for name in ("set_groups", "groups", "groups_into"):
        assert callable(getattr(R.Prepared, name)), name
    for fn in (R.intersect_rays, R.occluded_rays):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[-1] == "mask" and sig.parameters["mask"].default is None, fn.__name__
    # nearest_spheres and spheres_within keep their parameter lists (the proximity and range suites pin them): their masked forms are twins
    # that take the same arguments and mask= as a required keyword
    for plain, twin in ((R.nearest_spheres, R.nearest_spheres_masked), (R.spheres_within, R.spheres_within_masked)):
        a, b = inspect.signature(plain).parameters, inspect.signature(twin).parameters
        assert list(b) == list(a) + ["mask"] and "mask" not in a, twin.__name__
        assert b["mask"].kind is inspect.Parameter.KEYWORD_ONLY and b["mask"].default is inspect.Parameter.empty
        assert [b[k].default for k in a] == [a[k].default for k in a]
    assert list(inspect.signature(R.intersect_rays_masked_into).parameters) == [
        "rays_ptr", "n", "prepared", "index_ptr", "hit_ptr", "t_min", "t_max", "t_min_ptr", "t_max_ptr", "mask", "mask_ptr"]
    assert list(inspect.signature(R.spheres_within_masked_fill_into).parameters) == [
        "points_ptr", "n", "prepared", "offsets_ptr", "capacity", "index_ptr", "gap_ptr", "point_ptr", "max_dist", "max_dist_ptr", "first_ptr",
        "mask", "mask_ptr"]


def test_header_declares_groups():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym + "(" in h, sym
    for text in ("masked[ mask=per-query]", "family=within fill (per-point) first masked mask=per-query", "(groups[j] & mask_i) != 0"):
        assert text in h, text
    core = open(os.path.join(ROOT, "raytracers_amd", "csrc", "query_core.h")).read()
    assert "RT_HD bool group_seen(" in core and "RT_HD uint32_t group_combine(" in core and "RT_HD void group_climb(" in core
