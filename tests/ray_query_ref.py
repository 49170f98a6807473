"""numpy float32 restatement of objs_hit and ray_colour (futhark/ray.fut:76-86, :126-148) over the oracle's {L, I}.

The checker for the caller-ray entries (rt_trace_rays, rt_intersect_rays, rt_camera_rays).  Elementwise float32 only, in
the reference's association order: IEEE binary32 with no contraction, as the kernels are built.

The fold (bvh_fold, bvh.fut:61-84) is restated by what it computes, not by its walk:
  * a leaf is visited iff every inner ancestor's box passes `aabb_hit box r t_min t_max`;
  * `sphere_hit s r scene_epsilon t_max'` with the running t_max' accepts root1 if 0.1 < root1 < t_max', else root2 on the
    same terms; since root2 >= root1, the sphere's candidate (root1 if > 0.1, else root2 if > 0.1) does not depend on
    t_max', and the fold's result is the smallest candidate below the caller's t_max, ties to the lowest leaf index;
  * the winner is re-intersected with `sphere_hit s r t_min (t + 1)`; #none if that fails.
"""
import numpy as np

F = np.float32
EPS = F(0.1)          # scene_epsilon, ray.fut:3
TMAX = F(1e9)         # ray.fut:130


def dot(ax, ay, az, bx, by, bz):                      # prim.fut:22-24
    return (ax * bx + ay * by) + az * bz


class RefScene:
    """{L, I} of OracleScene(...).arrays(), arranged for vectorised folds over many rays."""

    def __init__(self, arrays):
        L = np.ascontiguousarray(arrays["L"], dtype=F)
        self.pos, self.col, self.rad = L[:, 0:3], L[:, 3:6], L[:, 6]
        self.n = L.shape[0]
        self.bmin = np.asarray(arrays["bmin"], dtype=F)
        self.bmax = np.asarray(arrays["bmax"], dtype=F)
        left, right, parent = (np.asarray(arrays[k], dtype=np.int64) for k in ("left", "right", "parent"))
        ni = self.n - 1
        # inner nodes by level (root 0 first) and each leaf's parent
        self.leaf_parent = np.full(self.n, -1, np.int64)
        depth = np.full(ni, -1, np.int64)
        depth[0] = 0
        frontier = [0]
        while frontier:
            nxt = []
            for i in frontier:
                for c in (left[i], right[i]):
                    if c >= 0:
                        depth[c] = depth[i] + 1
                        nxt.append(int(c))
                    else:
                        self.leaf_parent[-2 - c] = i
            frontier = nxt
        assert (depth >= 0).all() and (self.leaf_parent >= 0).all()
        self.levels = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]
        self.parent = parent
        self.inv_rad = (F(1.0) / self.rad).astype(F)

    # -- aabb_hit (ray.fut:53-70) of every (ray, inner node)
    def _boxes(self, o, d, tmin0, tmax0, nodes):
        tmin = np.broadcast_to(tmin0, (o.shape[0], 1)).astype(F)
        tmax = np.broadcast_to(tmax0, (o.shape[0], 1)).astype(F)
        ok = np.ones((o.shape[0], nodes.size), bool)
        with np.errstate(all="ignore"):
            for a in range(3):
                inv = (F(1.0) / d[:, a:a + 1]).astype(F)
                t0 = (self.bmin[nodes, a][None, :] - o[:, a:a + 1]) * inv
                t1 = (self.bmax[nodes, a][None, :] - o[:, a:a + 1]) * inv
                neg = inv < 0
                t0s, t1s = np.where(neg, t1, t0), np.where(neg, t0, t1)
                tmin = np.fmax(t0s, tmin)   # f32.max: the non-NaN operand
                tmax = np.fmin(t1s, tmax)
                ok &= ~(tmax <= tmin)
        return ok

    def visited(self, o, d, tmin0, tmax0):
        """[rays, leaves] bool: every inner ancestor's box passes with (tmin0, tmax0)."""
        ni = self.n - 1
        path = np.zeros((o.shape[0], ni), bool)
        for lvl, nodes in enumerate(self.levels):
            ok = self._boxes(o, d, tmin0, tmax0, nodes)
            if lvl > 0:
                ok &= path[:, self.parent[nodes]]
            path[:, nodes] = ok
        return path[:, self.leaf_parent]

    def roots(self, o, d):
        """sphere_hit's two roots (ray.fut:32-51) of every (ray, sphere) and whether the discriminant is positive."""
        ocx = o[:, 0:1] - self.pos[None, :, 0]
        ocy = o[:, 1:2] - self.pos[None, :, 1]
        ocz = o[:, 2:3] - self.pos[None, :, 2]
        dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        with np.errstate(all="ignore"):
            a = dot(dx, dy, dz, dx, dy, dz)
            b = dot(ocx, ocy, ocz, dx, dy, dz)
            c = dot(ocx, ocy, ocz, ocx, ocy, ocz) - self.rad[None, :] * self.rad[None, :]
            disc = b * b - a * c
            sq = np.sqrt(disc)
            r1 = (-b - sq) / a
            r2 = (-b + sq) / a
        return r1, r2, ~(disc <= 0)

    def objs_hit(self, o, d, t_min, t_max, chunk=256):
        """objs_hit bvh r t_min t_max -> (index [n] int32 (-1: #none), hit [n, 7] float32 {t, p, normal}, zeros for #none).
        t_min / t_max: scalars or per-ray arrays."""
        o = np.ascontiguousarray(o, dtype=F)
        d = np.ascontiguousarray(d, dtype=F)
        nr = o.shape[0]
        t_min = np.broadcast_to(np.asarray(t_min, dtype=F), (nr,))
        t_max = np.broadcast_to(np.asarray(t_max, dtype=F), (nr,))
        idx = np.full(nr, -1, np.int32)
        hit = np.zeros((nr, 7), F)
        for s in range(0, nr, chunk):
            e = min(nr, s + chunk)
            oo, dd, lo, hi = o[s:e], d[s:e], t_min[s:e], t_max[s:e]
            vis = self.visited(oo, dd, lo[:, None], hi[:, None])
            r1, r2, pos = self.roots(oo, dd)
            with np.errstate(invalid="ignore"):
                g = np.where(r1 > EPS, r1, np.where(r2 > EPS, r2, F(np.inf)))
                acc = vis & pos & (g < hi[:, None])
            gm = np.where(acc, g, F(np.inf))
            j = np.argmin(gm, axis=1)                                # first minimum: the lowest leaf index
            found = acc[np.arange(e - s), j]
            best = gm[np.arange(e - s), j]
            # re-hit: sphere_hit s r t_min (best + 1)
            rr1, rr2 = r1[np.arange(e - s), j], r2[np.arange(e - s), j]
            ok = pos[np.arange(e - s), j]
            with np.errstate(invalid="ignore"):
                lim = best + F(1.0)
                a1 = ok & (rr1 < lim) & (rr1 > lo)
                a2 = ok & ~a1 & (rr2 < lim) & (rr2 > lo)
            have = found & (a1 | a2)
            t = np.where(a1, rr1, rr2).astype(F)
            with np.errstate(all="ignore"):
                p = oo + t[:, None] * dd                             # point_at_param
                nrm = self.inv_rad[j][:, None] * (p - self.pos[j])   # scale (1.0/s.radius) (p - s.pos)
            idx[s:e] = np.where(have, j, -1)
            hit[s:e, 0] = np.where(have, t, F(0))
            hit[s:e, 1:4] = np.where(have[:, None], p, F(0))
            hit[s:e, 4:7] = np.where(have[:, None], nrm, F(0))
        return idx, hit

    def ray_colour(self, o, d, max_depth=50):
        """ray_colour objs r max_depth (ray.fut:126-148) -> colour [n, 3] float32 (before colour_to_pixel)."""
        o = np.array(o, dtype=F)
        d = np.array(d, dtype=F)
        nr = o.shape[0]
        light = np.ones((nr, 3), F)
        colour = np.zeros((nr, 3), F)
        live = np.arange(nr) if max_depth > 0 else np.arange(0)
        depth = 0
        while live.size:
            idx, hit = self.objs_hit(o[live], d[live], F(0), TMAX)
            with np.errstate(all="ignore"):
                dl = d[live]
                inv_norm = F(1.0) / np.sqrt(dot(dl[:, 0], dl[:, 1], dl[:, 2], dl[:, 0], dl[:, 1], dl[:, 2]))   # normalise
                u = inv_norm[:, None] * dl
                h = idx >= 0
                n = hit[:, 4:7]
                k = F(2.0) * dot(u[:, 0], u[:, 1], u[:, 2], n[:, 0], n[:, 1], n[:, 2])    # reflect
                refl = u - k[:, None] * n
                sc = h & (dot(refl[:, 0], refl[:, 1], refl[:, 2], n[:, 0], n[:, 1], n[:, 2]) > 0)   # scatter
                # miss: the sky
                tt = F(0.5) * (u[:, 1] + F(1.0))
                w = F(1.0) - tt
                sky = np.stack([w * F(1.0) + tt * F(0.5), w * F(1.0) + tt * F(0.7), w * F(1.0) + tt * F(1.0)], axis=1)
            L = light[live]
            C0 = colour[live]
            with np.errstate(all="ignore"):
                newc = np.where(h[:, None], L * C0, L * sky)         # scatter / absorb: light * colour; miss: light * sky
                att = self.col[np.where(h, idx, 0)]
                newl = np.where(sc[:, None], L * att, L)
            colour[live] = newc
            light[live] = newl
            o[live[sc]] = hit[sc, 1:4]
            d[live[sc]] = refl[sc]
            depth += 1
            live = live[sc] if depth < max_depth else np.arange(0)
        return colour


def colour_to_pixel(c):                                  # ray.fut:156-162
    c = np.asarray(c, dtype=F)
    with np.errstate(invalid="ignore"):
        q = (F(255.99) * c).astype(np.int32)
    return (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]


def camera_rays(cam12, h, w):
    """get_ray at pixel_u / pixel_v (ray.fut:109-114, :150-154, :166-169) for every pixel, row-major from the top row: [h*w, 6]."""
    c = np.asarray(cam12, dtype=F)
    ori, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    cols = np.arange(w)
    rows = np.arange(h)
    u = (cols.astype(F) / F(w)).astype(F)
    v = ((h - rows).astype(F) / F(h)).astype(F)
    U = np.broadcast_to(u[None, :], (h, w)).reshape(-1)
    V = np.broadcast_to(v[:, None], (h, w)).reshape(-1)
    d = ((llc[None, :] + U[:, None] * hor[None, :]) + V[:, None] * ver[None, :]) - ori[None, :]
    o = np.broadcast_to(ori[None, :], d.shape)
    return np.concatenate([o, d], axis=1).astype(F)
