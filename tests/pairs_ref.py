"""numpy float32 restatement of rt_visible_pairs on top of occlusion_ref.occluded.

Pair (i, j) has the ray o = P_i and d = fl(T_j - P_i) per component (TARGETS) or d = T_j (DIRECTIONS).  It is valid iff the six components of
o and d are finite and d is not (+-0, +-0, +-0); it is visible iff it is valid and occlusion_ref.occluded says False for that ray over
(t_min, t_max).  The rays are materialised here -- n * m of them -- which is what the library's entry avoids.  Words are little-endian
uint64: bit j & 63 of word [i, j >> 6].
"""
import numpy as np

import occlusion_ref as X

F = np.float32
TARGETS, DIRECTIONS = 0, 1


def pair_rays(points, targets, mode):
    """(o, d), each (n * m, 3) float32, pair (i, j) at row i * m + j."""
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(targets, dtype=F).reshape(-1, 3)
    n, m = p.shape[0], t.shape[0]
    o = np.broadcast_to(p[:, None, :], (n, m, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (t[None, :, :] - p[:, None, :]).astype(F) if mode == TARGETS else np.broadcast_to(t[None, :, :], (n, m, 3))
    return np.ascontiguousarray(o).reshape(-1, 3), np.ascontiguousarray(d, dtype=F).reshape(-1, 3)


def valid_pairs(points, targets, mode):
    """(n, m) bool: the validity rule."""
    n, m = np.asarray(points).reshape(-1, 3).shape[0], np.asarray(targets).reshape(-1, 3).shape[0]
    o, d = pair_rays(points, targets, mode)
    return (np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)).reshape(n, m)


def visible(ref, points, targets, mode, t_min, t_max):
    """(n, m) bool: the contract of rt_visible_pairs, one entry per pair."""
    n, m = np.asarray(points).reshape(-1, 3).shape[0], np.asarray(targets).reshape(-1, 3).shape[0]
    o, d = pair_rays(points, targets, mode)
    ok = valid_pairs(points, targets, mode).reshape(-1)
    vis = np.zeros(n * m, bool)
    if ok.any():
        vis[ok] = ~X.occluded(ref, o[ok], d[ok], t_min, t_max)
    return vis.reshape(n, m)


def pack(vis):
    """(n, m) bool -> (n, W) uint64, W = (m + 63) // 64; the bits past m are 0."""
    vis = np.asarray(vis, dtype=bool)
    n, m = vis.shape
    words = (m + 63) // 64
    padded = np.zeros((n, 64 * words), np.uint8)
    padded[:, :m] = vis
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(n, words)


def popcount(words):
    """(n, W) uint64 -> (n,) int32: the set bits of every row."""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1).sum(axis=1).astype(np.int32)


def reference(ref, points, targets, mode, t_min, t_max):
    """(words (n, W) uint64, count (n,) int32) as rt_visible_pairs writes them."""
    words = pack(visible(ref, points, targets, mode, t_min, t_max))
    return words, popcount(words)


def seeded(sc_arrays, n, m, seed):
    """(points (n, 3), targets (m, 3), directions (m, 3)) float32 around a scene: the origins of occlusion_ref.seeded_rays(n) at `seed` (a
    quarter each inside the scene's box, far outside it, inside spheres, mixed), and the first m origins at seed + 1 and directions at
    seed + 2 of draws of 2 m rays -- so the targets are half inside the scene's box and half far outside it."""
    points = X.seeded_rays(sc_arrays, n, seed)[:, :3]
    targets = X.seeded_rays(sc_arrays, 2 * m, seed + 1)[:m, :3]
    directions = X.seeded_rays(sc_arrays, 2 * m, seed + 2)[:m, 3:]
    return np.ascontiguousarray(points), np.ascontiguousarray(targets), np.ascontiguousarray(directions)


SEEDS = {"rgbbox": 17, "irreg": 29}
