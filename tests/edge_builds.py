"""Edge scenes for the GPU BVH builder's two large size classes (plain numpy): the CHAINED class (24 577 .. 131 072 spheres: 4-bit radix passes
without count launches, three Jacobi sweeps per launch) and the class BEYOND it (a count / scan / scatter per pass, one sweep per launch with
final nodes dropping out) -- on ties, skewed digits, trees far taller than the sweep count and non-finite spheres, which the uniform scenes
these classes are otherwise built from cannot produce.

A family is a function of n returning spheres7 {pos.xyz, colour.rgb, radius}.  Every sphere carries its own index in its colour and a radius
out of 3 072 values, so the rows of L are pairwise distinct: any order other than the stable sort by key changes L's bytes, and `ids_of(L)`
reads the order back from L alone.  Radii are multiples of 2^-13 below 1/2 and the lattice families' coordinates integers in [0, 1023], so
sphere_aabb and its centre are exact; the lattice scenes contain (0, 0, 0) and (1023, 1023, 1023), so floor(c / 1023 * 1024) = c: a centre's
Morton key is the interleave of its coordinates (as in edge_rays._tall).

The restatements below are built on the oracle's left / right / morton arrays (oracle_lib.OracleScene(...).arrays()): the Jacobi
propagation of bvh.fut:44-58 for ANY number of sweeps, the builder's "final nodes drop out" rule over two ping-pong buffers, the stable
order by key, and the depth of every inner node.  test_build_edges_cpu.py holds them against the oracle and shows that each family can
catch what it is there for; test_build_edges_gpu.py builds the scenes on the device.
"""
import functools

import numpy as np

F = np.float32

CHAINED = (24577, 32768, 65536, 131072)      # smallest (25 sort tiles, the last with 1 element; 16 sweeps = 5 x 3 + 1), a power of two (17 =
#                                              5 x 3 + 2), 18 = 6 x 3 sweeps (no remainder launch), largest (128 full tiles, 19 sweeps)
BEYOND = (131073,)                           # smallest: 129 tiles, one sweep per launch with `fin`
HUGE = 524289                                # 513 tiles: 16 x 513 counters, the one-block scan's second round and its carry
SIZES = CHAINED + BEYOND
FINITE = ("same", "few", "line", "line_z", "tall", "forest")
NON_FINITE = ("nan", "nan_y", "inf", "zero_radius")
TALL = ("tall", "forest")
HUGE_FAMILIES = ("same", "few", "tall")
NON_FINITE_SIZES = (24577, 131073)


def sweeps_of(n):
    """floor(log2 n) + 2 with float32 log2, as bvh.fut:47"""
    return int(np.log2(F(n), dtype=F)) + 2


# ---------------------------------------------------------------------------------------- the families
def _dress(pos):
    """spheres7 at `pos` [n, 3]: colour = (i mod 1024, i div 1024, 512) / 2048 + 0.3 -- exact, and distinct for i < 2^20 --
    radius = (1024 + 1571 i mod 3072) 2^-13 in [1/8, 1/2): neighbours in the input, and the copies of a point, differ widely."""
    n = pos.shape[0]
    assert n <= 1 << 20
    i = np.arange(n)
    s = np.zeros((n, 7), F)
    s[:, 0:3] = pos
    s[:, 3] = 0.3 + (i % 1024) / 2048.0
    s[:, 4] = 0.3 + (i // 1024) / 2048.0
    s[:, 5] = 0.55
    s[:, 6] = (1024 + (1571 * i) % 3072) / 8192.0
    return s


def ids_of(L):
    """the caller's index of every row of L, read from its colour"""
    L = np.asarray(L, dtype=F)
    lo = np.rint((L[:, 3].astype(np.float64) - F(0.3)) * 2048.0).astype(np.int64)
    hi = np.rint((L[:, 4].astype(np.float64) - F(0.3)) * 2048.0).astype(np.int64)
    return hi * 1024 + lo


def same(n):
    """every centre equal: every digit of every pass takes one value, the tree is pure index tie-break (height ceil(log2 n))"""
    return _dress(np.full((n, 3), 5.0, F))


# (one centre in each of seven octants: the keys part in their top three bits, so the tree is 3 levels over 7 tie-break trees)
FEW_CENTRES = np.array([(0, 0, 0), (1023, 1023, 1023), (3, 700, 64), (700, 3, 64), (100, 200, 900), (900, 800, 5), (600, 100, 1000)], F)


def few(n):
    """7 distinct centres dealt out as i mod 7: groups of n / 7 (far above two sort tiles), interleaved in the input"""
    return _dress(FEW_CENTRES[np.arange(n) % 7])


def _line(n, axis):
    pos = np.full((n, 3), 7.0, F)
    pos[:, axis] = (np.arange(n, dtype=np.float64) * (1023.0 / (n - 1))).astype(F)
    return _dress(pos)


def line(n):
    """n spheres evenly spaced along x (not on the lattice: the keys go through the division), y and z flat (0 / 0): about n / 1024 ties per
    key, the occupied bits the highest of each triple"""
    return _line(n, 0)


def line_z(n):
    """... along z: the occupied bits are the lowest of each triple"""
    return _line(n, 2)


def tall_points():
    """edge_rays._tall's chain: single-bit Morton codes (a 30-level chain) and the far corner"""
    pts = [(1023.0, 1023.0, 1023.0)]
    for a in range(3):
        for m in range(10):
            p = [0.0, 0.0, 0.0]
            p[a] = float(2 ** m)
            pts.append(tuple(p))
    return np.array(pts, F)


def tall(n):
    """edge_rays._tall(n - 31) with per-sphere radii: the 30-level chain with all n - 31 duplicates at its far end, the origin -- the greatest
    height n spheres can have here (30 + ceil(log2 (n - 31)) levels or so)"""
    return _dress(np.concatenate([tall_points(), np.zeros((n - 31, 3), F)]))


FOREST_PERIOD = 512 * 24


def forest_points():
    """8 x 8 x 8 cells of 128 lattice units, each its origin (three times: the chain's deep end, as in `tall`) plus origin + 2^m along each
    axis (m = 0 .. 6): 512 x 24 points"""
    cell = [(0.0, 0.0, 0.0)] * 3
    for a in range(3):
        for m in range(7):
            p = [0.0, 0.0, 0.0]
            p[a] = float(2 ** m)
            cell.append(tuple(p))
    cell = np.array(cell, F)
    g = np.arange(8, dtype=F) * 128.0
    org = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return (org[:, None, :] + cell[None, :, :]).reshape(-1, 3)


def forest(n):
    """forest_points() dealt out as i mod 12 288, the last sphere at the far corner: 512 chains of 21 levels under a balanced top of 9,
    every point a small tie group (n / 12 288 spheres, three times that at the cells' origins).  With one copy of each origin the deepest
    node of the 24 577-sphere forest is at depth 31, one short of the depth sort's second digit taking the value 2."""
    pos = forest_points()[np.arange(n) % FOREST_PERIOD]
    pos[n - 1] = 1023.0
    return _dress(pos)


def random_scene(n, seed):
    """test_device_scene_gpu._random_scene's spheres"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), F)
    ext = 10.0 * max(1.0, float(n) ** (1.0 / 3.0))
    s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.3, 2.0, n)
    return s


def non_finite(kind, n):
    """test_device_scene_gpu._degenerate's edits on a uniform random scene of n spheres: one in the first sort tile, one in the last, one in
    the middle (for the bounds: the first reduction block, the last, one between)"""
    s = random_scene(n, n)
    mid = n // 2 + 1
    if kind == "nan":
        s[7, 1] = np.nan
        s[n - 3, 6] = np.nan
        s[mid, 0] = np.nan
    elif kind == "nan_y":
        s[:, 1] = np.nan
    elif kind == "inf":
        s[11, 0] = np.inf
        s[n - 2, 2] = -np.inf
        s[mid, 1] = np.inf
    elif kind == "zero_radius":
        s[5, 6] = 0.0
        s[n - 6, 6] = np.nextafter(F(2.0 ** -20), F(0))
        s[mid, 6] = 0.0
    else:
        raise ValueError(kind)
    return s


_FAMILIES = dict(same=same, few=few, line=line, line_z=line_z, tall=tall, forest=forest)


@functools.lru_cache(maxsize=8)
def scene(family, n):
    """spheres7 of `family` at n (read-only: shared between tests)"""
    s = non_finite(family, n) if family in NON_FINITE else _FAMILIES[family](n)
    s = np.ascontiguousarray(s, dtype=F)
    s.setflags(write=False)
    return s


def finite_cases(huge=True):
    """(family, n) of the finite families at every size of the GPU leg"""
    out = [(f, n) for f in FINITE for n in SIZES]
    return out + ([(f, HUGE) for f in HUGE_FAMILIES] if huge else [])


# (look_from, look_at, fov): at least 5 % of a small frame's primary rays hit (test_build_edges_cpu checks it on the oracle).  The lattice
# scenes are sparse -- radii below 1/2 in a box of 1023 -- so the cameras stand close to where the spheres are.
VIEWS = {
    "same": ((5.0, 5.3, 7.6), (5.0, 5.0, 5.0), 30.0),
    "few": ((0.3, 0.4, 2.6), (0.0, 0.0, 0.0), 30.0),
    "line": ((500.0, 7.4, 9.2), (500.0, 7.0, 7.0), 50.0),
    "line_z": ((9.2, 7.4, 500.0), (7.0, 7.0, 500.0), 50.0),
    "tall": ((1.9, 0.9, 4.4), (1.6, 0.0, 0.0), 50.0),
    "forest": ((1.9, 0.9, 4.4), (1.6, 0.4, 0.0), 50.0),
}
FRAME = {"same": (24, 32)}          # (h, w); (48, 64) otherwise.  `same`: every ray that hits tests every sphere


def frame_of(family):
    return FRAME.get(family, (48, 64))


def rays_of(family, n):
    """(h, w) of the rays a scene is looked at with: its frame, or -- at 524 289 spheres, through intersect_rays -- 64 x 64 primary rays"""
    return (64, 64) if n == HUGE and family != "same" else frame_of(family)


def primary_rays(cam12, h, w):
    """[h * w, 6] float32 {origin, direction} of a frame's primary rays, row-major from the top row, in the kernels' float32 arithmetic
    (lane_core.h: primary_ray; edge_cull.primary_dd)"""
    c = np.asarray(cam12, dtype=F)
    u = (np.arange(w, dtype=F) / F(w))[None, :]
    v = ((F(h) - np.arange(h, dtype=F)) / F(h))[:, None]
    d = [np.broadcast_to(((c[3 + a] + u * c[6 + a]) + v * c[9 + a]) - c[a], (h, w)) for a in range(3)]
    o = [np.full((h, w), c[a], F) for a in range(3)]
    return np.stack(o + d, axis=-1).reshape(-1, 6).astype(F)


# ---------------------------------------------------------------------------------------- restatements
def leaf_boxes(L):
    """sphere_aabb (ray.fut:28-30) of every row of L, float32"""
    L = np.asarray(L, dtype=F)
    with np.errstate(invalid="ignore"):
        return L[:, 0:3] - L[:, 6:7], L[:, 0:3] + L[:, 6:7]


def _sources(left, right, L):
    """(lo, hi, kl, kr): boxes [n + (n - 1), 3] whose first n rows are the leaves' sphere boxes and the rest the inner nodes' (zero: the
    boxes before the first sweep), and each inner node's children as rows of them"""
    lmin, lmax = leaf_boxes(L)
    n, ni = len(lmin), len(left)
    kids = []
    for kid in (np.asarray(left, np.int64), np.asarray(right, np.int64)):
        kids.append(np.where(kid <= -2, -2 - kid, n + kid))
    return np.concatenate([lmin, np.zeros((ni, 3), F)]), np.concatenate([lmax, np.zeros((ni, 3), F)]), kids[0], kids[1]


def propagate_states(left, right, L, wanted):
    """{s: (bmin, bmax)} for every sweep count s in `wanted`: the inner boxes [n - 1, 3] float32 after s Jacobi sweeps from all-zero boxes,
    each sweep reading the previous sweep's array only (bvh.fut:44-58); enclosing is componentwise fmin / fmax (prim.fut:38-45), which drop
    a NaN"""
    lo, hi, kl, kr = _sources(left, right, L)
    n = len(lo) - len(left)
    out = {}
    for s in range(max(wanted) + 1):
        if s in wanted:
            out[s] = (lo[n:].copy(), hi[n:].copy())
        lo[n:], hi[n:] = np.fmin(lo[kl], lo[kr]), np.fmax(hi[kl], hi[kr])      # (the right-hand sides are complete before either store)
    return out


def propagate(left, right, L, sweeps):
    return propagate_states(left, right, L, (sweeps,))[sweeps]


def propagate_dropout(left, right, L, sweeps, early=0):
    """The builder's one-sweep-per-launch form: two ping-pong buffers, both zero at first; fin[i] = the sweep in which node i first computed
    its final box (both children leaves, or final in an earlier sweep); a node is skipped from sweep fin + 2 on, when its final box sits in
    both buffers.  Returns the buffer the last sweep wrote.  early = 1 is the mutant that skips from sweep fin + 1 on."""
    lo, hi, kl, kr = _sources(left, right, L)
    ni = len(left)
    n = len(lo) - ni
    leaf_l, leaf_r = kl < n, kr < n
    never = np.iinfo(np.int64).max
    fin = np.full(ni, never, np.int64)
    prev, cur = (lo, hi), (lo.copy(), hi.copy())
    for s in range(sweeps):
        live = np.nonzero(fin > s - 2 + early)[0]
        a, b = kl[live], kr[live]
        cur[0][n + live], cur[1][n + live] = np.fmin(prev[0][a], prev[0][b]), np.fmax(prev[1][a], prev[1][b])
        open_ = live[fin[live] > s]
        # (fin as it was before this sweep: a child that finishes in this very sweep stores s, which is not < s)
        done = (leaf_l[open_] | (fin[np.where(leaf_l[open_], 0, kl[open_] - n)] < s)) & \
               (leaf_r[open_] | (fin[np.where(leaf_r[open_], 0, kr[open_] - n)] < s))
        fin[open_[done]] = s
        prev, cur = cur, prev
    return prev[0][n:], prev[1][n:]


def boxes_differ(a, b):
    """[n - 1] bool: the node's box differs in some bit"""
    return ((a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1].view(np.uint32) != b[1].view(np.uint32))).any(axis=1)


def unsorted_keys(morton, L):
    """the Morton key of every sphere in the caller's order, from the oracle's sorted keys and L"""
    keys = np.empty(len(morton), np.uint32)
    keys[ids_of(L)] = morton
    return keys


def ids_by_rows(L, spheres7):
    """the caller's index of every row of L by matching bytes (for scenes that do not carry it in their colours; rows pairwise distinct)"""
    a, b = np.ascontiguousarray(L, dtype=F).view(np.uint32), np.ascontiguousarray(spheres7, dtype=F).view(np.uint32)
    oa, ob = np.lexsort(a.T[::-1]), np.lexsort(b.T[::-1])
    assert (a[oa] == b[ob]).all()
    ids = np.empty(len(a), np.int64)
    ids[oa] = ob
    return ids


def stable_order(keys):
    """the stable sort by key (bvh.fut:43): ascending (key, index)"""
    return np.argsort(keys, kind="stable")


def unstable_order(keys):
    """the mutant: equal keys by DESCENDING index"""
    return np.lexsort((-np.arange(len(keys)), keys))


def tie_groups(morton):
    """sizes of the groups of equal keys (sorted keys)"""
    return np.unique(morton, return_counts=True)[1]


def node_depths(left, right):
    """[n - 1] depth of every inner node (the root, node 0, at depth 0)"""
    ni = len(left)
    depth = np.full(ni, -1, np.int64)
    level = np.zeros(1, np.int64)
    d = 0
    while level.size:
        depth[level] = d
        kids = np.concatenate([np.asarray(left, np.int64)[level], np.asarray(right, np.int64)[level]])
        level = kids[kids >= 0]
        d += 1
    assert (depth >= 0).all()
    return depth


def height_of(left, right):
    """levels of inner nodes on the longest root-to-leaf path (Prepared.height)"""
    return int(node_depths(left, right).max()) + 1
