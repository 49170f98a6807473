"""numpy float32 restatement of rt_trace_paths: ray_colour's loop (futhark/ray.fut:126-148) with its vertices and its loop variables kept.

The loop is restated around an `objs_hit` callable, rays [m, 6] -> (index [m] int32, hit [m, 7] float32), the reference's
objs_hit objs r 0.0 1e9 (ray.fut:76-86):
  * ref_hit(RefScene): ray_query_ref's dense numpy restatement, for small scenes;
  * oracle_hit(OracleScene): the C oracle's literal walk, for any size.
Everything behind the callable is elementwise float32 in the reference's association order (normalise, reflect, scatter, the light's
product, the sky), as ray_query_ref.RefScene.ray_colour has it.

`fault` names one deliberate mistake of the restatement (FAULTS): the CPU suite shows that comparing against the true restatement reports
each of them under the output it corrupts.  bounce_cases restates one bounce on one sphere for tools/path_check.cpp."""
import numpy as np

from ray_query_ref import EPS, TMAX, F, dot

ESCAPED, ABSORBED, TRUNCATED = 0, 1, 2
CONTINUE = 3                      # path_check's fourth outcome: the chain goes on
NAMES = ("count", "end", "index", "hit", "light", "last_ray", "colour")

# fault -> the outputs it must corrupt (at least these are reported by differing())
FAULTS = {
    "absorbing_not_counted": ("count",),          # an absorbing last vertex left out of count
    "light_at_absorbing": ("light",),             # light multiplied by the colour of an absorbing vertex
    "no_light_at_truncating": ("light",),         # light not multiplied at the vertex that spends the budget
    "absorbed_for_truncated": ("end",),           # ABSORBED reported where depth + 1 == max_depth truncates
    "last_ray_not_advanced": ("last_ray",),       # the last ray left at the truncating vertex's incoming ray
    "root_from_fold": ("hit",),                   # a vertex's t taken from the fold's root instead of the re-intersection's
}


def ref_hit(ref):
    return lambda rays: ref.objs_hit(rays[:, :3], rays[:, 3:], F(0), TMAX)


def oracle_hit(orc):
    return lambda rays: orc.objs_hit_rays(rays, 0.0, 1e9)


def fold_hit(ref, chunk=256):
    """objs_hit WITHOUT its re-intersection (the root_from_fold fault): the fold's winner with the fold's own root as t."""
    def hit_fn(rays):
        o = np.ascontiguousarray(rays[:, :3], dtype=F)
        d = np.ascontiguousarray(rays[:, 3:], dtype=F)
        idx = np.full(o.shape[0], -1, np.int32)
        hit = np.zeros((o.shape[0], 7), F)
        for s in range(0, o.shape[0], chunk):
            oo, dd = o[s:s + chunk], d[s:s + chunk]
            rows = np.arange(oo.shape[0])
            vis = ref.visited(oo, dd, F(0), TMAX)
            r1, r2, pos = ref.roots(oo, dd)
            with np.errstate(all="ignore"):
                g = np.where(r1 > EPS, r1, np.where(r2 > EPS, r2, F(np.inf)))
                acc = vis & pos & (g < TMAX)
                gm = np.where(acc, g, F(np.inf))
                j = np.argmin(gm, axis=1)
                have = acc[rows, j]
                t = gm[rows, j].astype(F)
                p = oo + t[:, None] * dd
                nrm = ref.inv_rad[j][:, None] * (p - ref.pos[j])
            idx[s:s + chunk] = np.where(have, j, -1)
            hit[s:s + chunk, 0] = np.where(have, t, F(0))
            hit[s:s + chunk, 1:4] = np.where(have[:, None], p, F(0))
            hit[s:s + chunk, 4:7] = np.where(have[:, None], nrm, F(0))
        return idx, hit
    return hit_fn


def _scatter(d, nrm):
    """(refl [m, 3], u [m, 3]): normalise, reflect (ray.fut:116-121)"""
    inv_norm = F(1.0) / np.sqrt(dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    u = inv_norm[:, None] * d
    k = F(2.0) * dot(u[:, 0], u[:, 1], u[:, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2])
    return u - k[:, None] * nrm, u


def _sky(u):
    tt = F(0.5) * (u[:, 1] + F(1.0))
    w = F(1.0) - tt
    return np.stack([w * F(1.0) + tt * F(0.5), w * F(1.0) + tt * F(0.7), w * F(1.0) + tt * F(1.0)], axis=1)


def trace_paths(hit_fn, colours, rays, max_depth, k, fault=None):
    """(count (n,) int32, end (n,) uint8, index (n, k) int32, hit (n, k, 7), light (n, 3), last_ray (n, 6), colour (n, 3) float32): the
    contract of rt_trace_paths.  colours: [spheres, 3], the colours of L."""
    assert fault is None or fault in FAULTS, fault
    colours = np.asarray(colours, dtype=F)
    r = np.array(rays, dtype=F).reshape(-1, 6)
    n = r.shape[0]
    light = np.ones((n, 3), F)
    colour = np.zeros((n, 3), F)
    count = np.zeros(n, np.int32)
    end = np.full(n, TRUNCATED, np.uint8)          # what a ray keeps if it still scatters at its max_depth-th vertex (or max_depth == 0)
    index = np.full((n, k), -1, np.int32)
    hit = np.zeros((n, k, 7), F)
    live = np.arange(n) if max_depth > 0 else np.arange(0)
    depth = 0
    while live.size:
        idx, h7 = hit_fn(r[live])
        have = idx >= 0
        with np.errstate(all="ignore"):
            refl, u = _scatter(r[live, 3:], h7[:, 4:7])
            nrm = h7[:, 4:7]
            sc = have & (dot(refl[:, 0], refl[:, 1], refl[:, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2]) > 0)
            L = light[live]
            colour[live] = np.where(have[:, None], L * F(0), L * _sky(u))
            lit = L * colours[np.where(have, idx, 0)]
        last = depth + 1 == max_depth
        if depth < k:
            index[live[have], depth] = idx[have]
            hit[live[have], depth] = h7[have]
        count[live] += sc if fault == "absorbing_not_counted" else have
        end[live[~have]] = ESCAPED
        end[live[have & ~sc]] = ABSORBED
        if last and fault == "absorbed_for_truncated":
            end[live[sc]] = ABSORBED
        upd = have if fault == "light_at_absorbing" else sc
        if not (last and fault == "no_light_at_truncating"):
            light[live[upd]] = lit[upd]
        if not (last and fault == "last_ray_not_advanced"):
            r[live[sc], :3] = h7[sc, 1:4]
            r[live[sc], 3:] = refl[sc]
        depth += 1
        live = live[sc] if depth < max_depth else np.arange(0)
    return count, end, index, hit, light, r, colour


def objs_hit_calls(count, end):
    """the objs_hit calls ray_colour makes per ray: what OracleScene.chain_lengths counts per pixel"""
    return count + (end == ESCAPED)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def differing(got, want):
    """{output name: rays on which it differs, bit for bit} for two results of trace_paths / rt_trace_paths"""
    out = {}
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{name}: {g.shape} {g.dtype} != {w.shape} {w.dtype}"
        if g.shape[0] == 0:
            continue
        bad = np.nonzero((bits(g) != bits(w)).reshape(g.shape[0], -1).any(axis=1))[0]
        if bad.size:
            out[name] = bad
    return out


def assert_same(got, want, what):
    diff = differing(got, want)
    assert not diff, f"{what}: " + "; ".join(f"{name} differs on {bad.size} rays, first {bad[:5]}" for name, bad in diff.items())


def prefix(res, k):
    count, end, index, hit, light, last, colour = res
    return count, end, index[:, :k], hit[:, :k], light, last, colour


def auto_rays_per_wave(n, num_cu):
    """the documented launch rule of rt_trace_paths, restated for the tests that read rt_context_last_launch: 64 rays per
    wave while n <= 64 * 8 * num_cu, above that the smallest multiple of 64 that keeps the grid at 8 * num_cu waves, at most 256"""
    waves = 8 * max(int(num_cu), 1)
    if n <= 64 * waves:
        return 64
    return min((-(-int(n) // waves) + 63) // 64 * 64, 256)


def bounce_cases(cases, depth=0, max_depth=50):
    """tools/path_check.cpp restated: cases [m, 16] float32 {ray 6, sphere pos 3, colour 3, radius, light 3} -> [m, 20] uint32: the outcome
    (ESCAPED, ABSORBED, TRUNCATED, CONTINUE), hit7, the new ray, the new light, the colour.  The fold of the one sphere (sphere_root from
    best = 1e9), its re-intersection over (0, best + 1), then the bounce at `depth` of `max_depth`."""
    c = np.ascontiguousarray(cases, dtype=F).reshape(-1, 16)
    o, d, pos, col, rad, light = c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9:12], c[:, 12], c[:, 13:16]
    m = c.shape[0]
    with np.errstate(all="ignore"):
        oc = o - pos
        a = dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
        b = dot(oc[:, 0], oc[:, 1], oc[:, 2], d[:, 0], d[:, 1], d[:, 2])
        cc = dot(oc[:, 0], oc[:, 1], oc[:, 2], oc[:, 0], oc[:, 1], oc[:, 2]) - rad * rad
        disc = b * b - a * cc
        ok = ~(disc <= 0)
        sq = np.sqrt(disc)
        t1, t2 = (-b - sq) / a, (-b + sq) / a
        g = np.where(t1 > EPS, t1, np.where(t2 > EPS, t2, F(np.inf)))        # sphere_root
        found = ok & (g < TMAX)                                              # closest_update from (1e9, none)
        lim = g + F(1.0)                                                     # rehit_full
        a1 = ok & (t1 < lim) & (t1 > F(0))
        a2 = ok & ~a1 & (t2 < lim) & (t2 > F(0))
        have = found & (a1 | a2)
        t = np.where(a1, t1, t2).astype(F)
        inv_rad = F(1.0) / rad
        p = o + t[:, None] * d
        nrm = inv_rad[:, None] * (p - pos)
        refl, u = _scatter(d, nrm)
        dt = dot(refl[:, 0], refl[:, 1], refl[:, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2])
        sc = have & (dt > 0)
        colour = np.where(have[:, None], light * F(0), light * _sky(u))
        lit = light * col
    kind = np.where(~have, ESCAPED, np.where(~sc, ABSORBED, CONTINUE if depth + 1 < max_depth else TRUNCATED)).astype(np.uint32)
    out = np.zeros((m, 20), np.uint32)
    out[:, 0] = kind
    vals = np.zeros((m, 19), F)
    vals[:, 0] = np.where(have, t, F(0))
    vals[:, 1:4] = np.where(have[:, None], p, F(0))
    vals[:, 4:7] = np.where(have[:, None], nrm, F(0))
    vals[:, 7:10] = np.where(sc[:, None], p, o)
    vals[:, 10:13] = np.where(sc[:, None], refl, d)
    vals[:, 13:16] = np.where(sc[:, None], lit, light)
    vals[:, 16:19] = colour
    out[:, 1:] = vals.view(np.uint32)
    return out, {"have": have, "scatter": sc, "dot": dt, "disc": disc, "t": t}
