"""numpy restatement of the sphere groups (rt_prepared_set_groups, rt_*_masked) over a prepared scene's arrays (oracle_lib.OracleScene(...).arrays()
or Prepared.bvh_arrays()), on top of the unmasked restatements (ray_query_ref, interval_ref, proximity_ref, within_ref).

THE rule: query i sees sphere j iff groups[j] & mask_i != 0 on unsigned 32-bit words; mask 0 sees nothing.
  * groups in L order are the caller's words gathered through ids: groups_L[i] = words[ids[i]]                     (gather)
  * node_groups[v] = the OR of groups_L over every leaf below inner node v, by plain recursion over left / right    (node_groups)
  * masked objs_hit / occluded: the dense folds of RefScene with `visited` AND-ed with the seen set                 (objs_hit, occluded)
  * masked nearest / within: proximity_ref.nearest / within_ref.within over L[seen], indices mapped back to L       (nearest, within)
Each answer exists twice: DENSE, as above (the definition), and as a WALK -- a stack-based traversal of the tree, one query at a time, that
skips an inner node whose word shares no bit with the mask and asks a leaf's word before it looks at the sphere, the way the kernels do.  The
two must be equal: pruning is an optimisation, never a definition.  The walk takes a `mutant`, a wrong variant of the rule or of its inputs
(MUTANTS); the CPU suite shows each caught by a named input.
"""
import numpy as np

import interval_ref as I
import proximity_ref as P
import ray_query_ref as Q
import within_ref as W

F = np.float32
U = np.uint32
MUTANTS = ("rule_all_bits", "rule_signed", "node_groups_short", "no_gather", "sibling_word")


def seen(groups, masks, mutant=None):
    """[m, n] bool: does query i (masks: a scalar or [m]) see the sphere / node whose word is groups[j]"""
    g = np.asarray(groups, dtype=np.uint64).astype(U)[None, :]
    m = np.atleast_1d(np.asarray(masks, dtype=np.uint64).astype(U))[:, None]
    a = np.ascontiguousarray(g & m)
    if mutant == "rule_all_bits":
        return a == m
    if mutant == "rule_signed":
        return a.view(np.int32) > 0
    return a != 0


def _seen1(g, m, rule):
    """seen() of one word against one mask, on Python ints"""
    a = g & m
    if rule == "rule_all_bits":
        return a == m
    if rule == "rule_signed":
        return 0 < a < 2 ** 31   # (a signed 32-bit compare: bit 31 makes the word negative)
    return a != 0


def gather(words, ids, mutant=None):
    """the caller-order words in L order"""
    w = np.asarray(words, dtype=np.uint64).astype(U)
    return w.copy() if mutant == "no_gather" else w[np.asarray(ids, dtype=np.int64)]


def _leaf(c):
    return -2 - c   # (the ptr encoding of rt_prepared_get_bvh: a leaf j is -2 - j)


def node_groups(left, right, groups):
    """[n - 1] uint32: the exact subtree ORs, by plain recursion from the root"""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    g = np.asarray(groups, dtype=U)
    out = np.zeros(left.size, U)

    def below(c):
        if c < 0:
            return U(g[_leaf(c)])
        out[c] = below(left[c]) | below(right[c])
        return out[c]

    below(0)
    return out


def node_groups_sweeps(left, right, groups, sweeps):
    """`sweeps` Jacobi sweeps from zero words, each reading the previous sweep's array (how the boxes are propagated): exact iff sweeps >= the
    number of inner-node levels"""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    g = np.asarray(groups, dtype=U)
    cur = np.zeros(left.size, U)
    for _ in range(sweeps):
        wl = np.where(left < 0, g[np.clip(_leaf(left), 0, g.size - 1)], cur[np.clip(left, 0, left.size - 1)])
        wr = np.where(right < 0, g[np.clip(_leaf(right), 0, g.size - 1)], cur[np.clip(right, 0, left.size - 1)])
        cur = (wl | wr).astype(U)
    return cur


def levels(left, right):
    """the number of inner-node levels (the root alone: 1)"""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    depth, frontier = 0, [0]
    while frontier:
        depth += 1
        frontier = [int(c) for v in frontier for c in (left[v], right[v]) if c >= 0]
    return depth


def node_groups_climb(left, right, parent, groups, order=None):
    """the derive kernel's mechanism on the host, one node at a time in `order` (any order gives the same words): every inner node seeds the OR
    of its LEAF children's words and climbs `parent`, OR-ing in what it carries and carrying on only with the bits it newly set"""
    left, right, parent = (np.asarray(a, dtype=np.int64) for a in (left, right, parent))
    g = np.asarray(groups, dtype=U)
    out = np.zeros(left.size, U)
    for v in (range(left.size) if order is None else order):
        carry = U(0)
        for c in (left[v], right[v]):
            if c < 0:
                carry |= g[_leaf(c)]
        u = int(v)
        while carry != 0 and u >= 0:
            old = out[u]
            out[u] = old | carry
            carry = U(carry & ~old)
            u = int(parent[u])
    return out


class MaskedScene(Q.RefScene):
    """RefScene whose `visited` is filtered by what the queries see: DENSE (visited & seen) or through the WALK."""

    def __init__(self, arrays):
        super().__init__(arrays)
        self.left = np.asarray(arrays["left"], dtype=np.int64)
        self.right = np.asarray(arrays["right"], dtype=np.int64)
        self._filter = None

    def visited(self, o, d, tmin0, tmax0):
        if self._filter is None:
            return super().visited(o, d, tmin0, tmax0)
        return self._filter(o, d, tmin0, tmax0)

    def sibling_words(self, groups):
        """the mutant's leaf words: a leaf whose sibling is a leaf gets the sibling's word"""
        g = np.asarray(groups, dtype=U)
        out = g.copy()
        both = np.nonzero((self.left < 0) & (self.right < 0))[0]
        out[_leaf(self.left[both])] = g[_leaf(self.right[both])]
        out[_leaf(self.right[both])] = g[_leaf(self.left[both])]
        return out

    def walk_leaves(self, node_ok, groups, ngroups, mask, prune=True, mutant=None):
        """the leaves one query's walk offers, in the order it meets them: node_ok[v] -- does inner node v's own test pass (None: every node
        does) --, a child pushed only if its word shares a bit with the mask (prune), a leaf offered only if its word does.  groups / ngroups:
        sequences of Python ints (the walk is scalar code)"""
        rule = mutant if mutant in ("rule_all_bits", "rule_signed") else None
        mask = int(mask)
        left, right = self._kids()
        out = []
        if mask == 0 or (prune and not _seen1(ngroups[0], mask, rule)):
            return out
        def offer(c):
            if _seen1(groups[_leaf(c)], mask, rule):
                out.append(_leaf(c))

        def wanted(c):
            return not prune or _seen1(ngroups[c], mask, rule)

        stack = [0]   # (an inner node, or a leaf in its ptr encoding: a right leaf waits behind an inner left sibling)
        while stack:
            v = stack.pop()
            if v < 0:
                offer(v)
                continue
            if node_ok is not None and not node_ok[v]:
                continue
            lc, rc = left[v], right[v]
            if lc < 0:
                offer(lc)
                if rc < 0:
                    offer(rc)
                elif wanted(rc):
                    stack.append(rc)
            else:
                if rc < 0 or wanted(rc):
                    stack.append(rc)
                if wanted(lc):
                    stack.append(lc)
        return out

    def _kids(self):
        if not hasattr(self, "_kid_lists"):
            self._kid_lists = (self.left.tolist(), self.right.tolist())
        return self._kid_lists


def _chunks(n, chunk=256):
    return [(s, min(n, s + chunk)) for s in range(0, n, chunk)]


def _masks(n, masks):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(masks, dtype=np.uint64).astype(U), (n,)))


def _ray_filter(ref, groups, ngroups, masks, walk, prune, mutant):
    """RefScene.visited's replacement for one chunk of rays with the masks `masks`"""
    if not walk:
        return lambda o, d, lo, hi: Q.RefScene.visited(ref, o, d, lo, hi) & seen(groups, masks)

    def through_the_walk(o, d, lo, hi):
        g = (ref.sibling_words(groups) if mutant == "sibling_word" else np.asarray(groups)).tolist()
        ng = np.asarray(ngroups).tolist()
        ok = ref._boxes(o, d, lo, hi, np.arange(ref.n - 1))
        out = np.zeros((o.shape[0], ref.n), bool)
        for i in range(o.shape[0]):
            out[i, ref.walk_leaves(ok[i], g, ng, masks[i], prune, mutant)] = True
        return out
    return through_the_walk


def _ray_query(fn, ref, rays, t_min, t_max, groups, masks, walk, prune, ngroups, mutant):
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    n = rays.shape[0]
    lo, hi = I._bounds(n, t_min, t_max)
    m = _masks(n, masks)
    if walk and ngroups is None:
        ngroups = node_groups(ref.left, ref.right, groups)
    parts = []
    try:
        for s, e in _chunks(n):
            ref._filter = _ray_filter(ref, groups, ngroups, m[s:e], walk, prune, mutant)
            parts.append(fn(ref, rays[s:e, :3], rays[s:e, 3:], lo[s:e], hi[s:e], chunk=256))
    finally:
        ref._filter = None
    return parts


def objs_hit(ref, rays, t_min, t_max, groups, masks, walk=False, prune=True, ngroups=None, mutant=None):
    """(index [n] int32, hit [n, 7] float32): rt_intersect_rays_masked.  ref: a MaskedScene; groups: [spheres] uint32 in L order; masks: a
    scalar or [n]; t_min / t_max: scalars or [n] (an invalid interval: a miss).  walk: through the stack walk (ngroups: the node words it
    prunes by, default the exact ones)"""
    parts = _ray_query(I.objs_hit, ref, rays, t_min, t_max, groups, masks, walk, prune, ngroups, mutant)
    if not parts:
        return np.zeros(0, np.int32), np.zeros((0, 7), F)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def occluded(ref, rays, t_min, t_max, groups, masks, walk=False, prune=True, ngroups=None, mutant=None):
    """[n] bool: rt_occluded_rays_masked (arguments as objs_hit)"""
    parts = _ray_query(I.occluded, ref, rays, t_min, t_max, groups, masks, walk, prune, ngroups, mutant)
    return np.concatenate(parts) if parts else np.zeros(0, bool)


def _by_mask(n, masks):
    m = _masks(n, masks)
    return m, [(v, np.nonzero(m == v)[0]) for v in np.unique(m)]


def nearest(L, points, max_dist, k, groups, masks):
    """(count [m] int32, index [m, k] int32, gap [m, k] float32): rt_nearest_spheres_masked -- proximity_ref.nearest over L[seen] with the
    indices mapped back to L, mask value by mask value"""
    L = np.asarray(L, dtype=F)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m = p.shape[0]
    md = P._bounds(m, max_dist)
    count, index, gap = np.zeros(m, np.int32), np.full((m, k), -1, np.int32), np.zeros((m, k), F)
    for v, who in _by_mask(m, masks)[1]:
        sel = np.nonzero(seen(groups, v)[0])[0]
        if sel.size == 0:
            continue
        c, ix, g = P.nearest(L[sel], p[who], md[who], k)
        count[who], gap[who] = c, g
        index[who] = np.where(ix >= 0, sel[np.maximum(ix, 0)], -1)
    return count, index, gap


def within(L, points, max_dist, groups, masks, first=None):
    """(offsets [m + 1] int64, index [total] int32, gap [total] float32): rt_spheres_within_masked_* -- within_ref.within over L[seen], indices
    mapped back to L, then the `first` rule on those indices"""
    L = np.asarray(L, dtype=F)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m = p.shape[0]
    md = P._bounds(m, max_dist)
    fi = np.zeros(m, np.int64) if first is None else np.asarray(first).astype(np.int64)
    rows, cols, gs = [], [], []
    for v, who in _by_mask(m, masks)[1]:
        sel = np.nonzero(seen(groups, v)[0])[0]
        if sel.size == 0:
            continue
        off, idx, g = W.within(L[sel], p[who], md[who])
        r = who[np.repeat(np.arange(who.size), np.diff(off))]
        j = sel[idx]
        keep = j >= fi[r]
        rows.append(r[keep]), cols.append(j[keep]), gs.append(g[keep])
    if not rows:
        return np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    r, j, g = np.concatenate(rows), np.concatenate(cols), np.concatenate(gs)
    o = np.lexsort((j, r))
    return W._csr(m, r[o], j[o], g[o])


def within_walk(ref, points, max_dist, groups, masks, first=None, prune=True, ngroups=None, mutant=None):
    """within() through the stack walk: no box test (the walk's box test is the unmasked query's own, proven elsewhere), every node pruned by
    its word, every offered leaf's gap held against the bound"""
    L = np.concatenate([ref.pos, ref.col, ref.rad[:, None]], axis=1)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m = p.shape[0]
    md = P._bounds(m, max_dist)
    ok = P.point_ok(p) & P.max_dist_ok(md)
    fi = np.zeros(m, np.int64) if first is None else np.asarray(first).astype(np.int64)
    mk = _masks(m, masks)
    if ngroups is None:
        ngroups = node_groups(ref.left, ref.right, groups)
    g_leaf = (ref.sibling_words(groups) if mutant == "sibling_word" else np.asarray(groups)).tolist()
    ng = np.asarray(ngroups).tolist()
    rows, cols, gs = [], [], []
    for i in np.nonzero(ok)[0]:
        js = np.asarray(ref.walk_leaves(None, g_leaf, ng, mk[i], prune, mutant), dtype=np.int64)
        if js.size == 0:
            continue
        assert (np.diff(js) > 0).all(), "the ordered walk meets the leaves in ascending j"
        g = P.gaps(L[js], p[i:i + 1])[0]
        with np.errstate(invalid="ignore"):
            keep = (g <= md[i]) & (js >= fi[i])
        rows.append(np.full(int(keep.sum()), i)), cols.append(js[keep]), gs.append(g[keep])
    if not rows:
        return np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    return W._csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(gs))


def nearest_from_rows(m, k, offsets, index, gap):
    """(count, index [m, k], gap [m, k]): CSR rows re-sorted by (gap, index) and cut at k -- what masked nearest must equal"""
    count = np.diff(offsets).astype(np.int32)
    ix, g = W.sort_rows_by_gap(offsets, index, gap)
    oi, og = np.full((m, k), -1, np.int32), np.zeros((m, k), F)
    rows = np.repeat(np.arange(m), count)
    rank = np.arange(rows.size) - offsets[:-1][rows]
    keep = rank < k
    oi[rows[keep], rank[keep]] = ix[keep]
    og[rows[keep], rank[keep]] = g[keep]
    return count, oi, og


# ---- group patterns and masks of the tests ---------------------------------------------------------------------------------------------
def patterns(spheres7, seed):
    """name -> [n] uint32 words in the CALLER's order for the scene `spheres7` (n x 7)"""
    s = np.asarray(spheres7, dtype=F)
    n = s.shape[0]
    rng = np.random.default_rng(seed)
    c = np.arange(n)
    mid = 0.5 * (s[:, :3].min(axis=0) + s[:, :3].max(axis=0))
    octant = ((s[:, 0] > mid[0]).astype(U) | ((s[:, 1] > mid[1]).astype(U) << U(1)) | ((s[:, 2] > mid[2]).astype(U) << U(2)))
    one31 = np.zeros(n, U)
    one31[n - 1 - (seed % n)] = U(0x80000000)
    return {
        "all_ones": np.full(n, 0xFFFFFFFF, U),
        "all_zero": np.zeros(n, U),
        "bit_c_mod_32": (U(1) << (c % 32).astype(U)).astype(U),
        "octant": (U(1) << octant).astype(U),
        "bit31_on_one": one31,
        "random": rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U),
    }


SCALAR_MASKS = (0, 0xFFFFFFFF, 1, 0x10, 0x80000000)


def mixed_masks(n, seed):
    """[n] uint32: zeros, all ones, single bits (bit 31 among them) and random words, at random"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 5, n)
    bits = (U(1) << rng.integers(0, 32, n).astype(U)).astype(U)
    rnd = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U)
    out = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [U(0), U(0xFFFFFFFF), bits, U(0x80000000)], rnd).astype(U)
    return out


def tall_chain(n=200, seed=3):
    """n x 7 spheres with geometric spacing along a diagonal: a tree far taller than floor(log2 n) + 2, whose top boxes the AABB propagation
    leaves partial (test_proximity_gpu's _geometric, with radii that never vanish)"""
    rng = np.random.default_rng(seed)
    t = np.exp2(-0.25 * np.arange(n))
    s = np.zeros((n, 7), F)
    s[:, 0], s[:, 1], s[:, 2] = 100.0 * t, 50.0 * t, -100.0 * t
    s[:, 3:6] = 0.5
    s[:, 6] = 10.0 * t * rng.uniform(0.05, 1.0, n)
    return s


TALL_VIEW = ((0.0, 5.0, 40.0), (0.0, 0.0, 0.0), 50.0)
