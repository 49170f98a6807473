"""Edge scenes and cameras for the CULL instantiations of the pooled kernel (plain numpy): renders placed at the limits of the guards that decide
whether a launch is culled at all -- the scene guard 2 reach <= 2^15 r_min, the camera guard, the per-ray gate
d.d in [2^-6, 2^20], c_max <= 2^40, r_min >= 2^-20, tree height <= floor(log2 n) + 2 -- in inside / outside pairs that differ by as little as
a guard can resolve, plus ties and bounce chains between tiny and huge spheres.

`cases()` maps a name to a Case: (spheres7, cams, h, w, expect_culled, ...).  spheres7 is {pos.xyz, colour.rgb, radius} for
`Context.scene_from_spheres` and `OracleScene("custom", ...)`, cams a list of cam12 {origin, llc, horizontal, vertical}.  `expect_culled` is
whether a launch with ALL of the case's cameras must be culled; `scene_ok` and `origin_ok[i]` are its parts.  They come from `guards` /
`origin_ok` below, a float64 restatement of rt::cull_stats / cull_finish / cull_origin_ok written from DESIGN.md 3.4 -- not from the
library -- and from the height of the reference's tree (OracleScene.arrays()).

The guards compute in double with (1 + 2^-20) factors, so a pair sits at 1 - 2^-12 and 1 + 2^-12 of a limit: far more than the factor and far
more than a float32 ulp, so which side the float32 inputs land on is decided here in float64 and asserted against the intention.
"""
import collections
import functools

import numpy as np

F = np.float32
D = np.float64
EPS = 2.0 ** -12            # a pair's distance from its limit, relative

Case = collections.namedtuple("Case", "spheres7 cams h w expect_culled scene_ok origin_ok tags")
# tags: "control" (far inside every guard), "bounce" (chains of 3 rays and more are the point), "gate_all" / "gate_some" (every / some primary
# ray of some camera fails the d.d gate), "rmin_hits" (rays must land on a sphere of the smallest radius), "pair" (half of a guard pair)


# ---------------------------------------------------------------------------------------- the guards, restated in float64
def tree_height(left, right):
    """Inner nodes on the longest root-to-leaf path of the canonical tree (inner i -> i >= 0, leaf i -> -2 - i; node 0 is the root)."""
    depth = np.zeros(len(left), np.int64)
    todo, height = [0], 1
    depth[0] = 1
    while todo:
        i = todo.pop()
        height = max(height, int(depth[i]))
        for c in (int(left[i]), int(right[i])):
            if c >= 0:
                depth[c] = depth[i] + 1
                todo.append(c)
    return height


def guards(spheres7, height):
    """The scene's side: dict(ok, c2, kappa (float32 or None), centre, reach, r_min) from float32 spheres and the tree's height."""
    s = np.asarray(spheres7, dtype=F).astype(D)
    n = s.shape[0]
    out = dict(ok=False, c2=None, kappa=None, centre=None, reach=None, r_min=None)
    if n < 2 or height > int(np.floor(np.log2(n))) + 2:
        return out
    p, r = s[:, 0:3], s[:, 6]
    if not np.isfinite(s[:, [0, 1, 2, 6]]).all() or not (r >= 2.0 ** -20).all():
        return out
    r_min, r_max = r.min(), r.max()
    c_max = (np.abs(p) + r[:, None]).max()
    if c_max > 2.0 ** 40:
        return out
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = hi - lo
    diag2 = (ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]
    out.update(centre=0.5 * (lo + hi), reach=0.5 * np.sqrt(diag2) * (1.0 + 2.0 ** -20) + r_max, r_min=r_min)
    if 2.0 * out["reach"] > 2.0 ** 15 * r_min:
        return out
    c2 = 1.01 * (2.0 ** -16 / r_min + 2.0 ** -21)
    c0 = 1.01 * (2.0 ** -16 * r_max * r_max / r_min + 2.0 ** -18 * r_max + 2.0 ** -24 * c_max + 2.0 ** -21)
    out["c2"] = np.nextafter(F(c2), F(np.inf))
    out["kappa"] = np.nextafter(F(c0 / (c2 * 0.015625)), F(np.inf))
    out["ok"] = bool(np.isfinite(out["c2"]) and np.isfinite(out["kappa"]))
    return out


def origin_ok(g, origin):
    """The camera's side: |origin - centre| (1 + 2^-20) + reach <= 2^15 r_min, for a scene that passed."""
    if not g["ok"]:
        return False
    o = np.asarray(origin, dtype=F).astype(D)
    if not np.isfinite(o).all():
        return False
    d = o - g["centre"]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return bool(np.sqrt(d2) * (1.0 + 2.0 ** -20) + g["reach"] <= 2.0 ** 15 * g["r_min"])


def scene_guard_use(spheres7):
    """2 reach / (2^15 r_min): the scene guard holds iff this is <= 1."""
    g = guards(spheres7, 0)
    return 2.0 * g["reach"] / (2.0 ** 15 * g["r_min"])


# ---------------------------------------------------------------------------------------- cameras
def camera(look_from, look_at, fov, aspect=1.0, focal=1.0):
    """cam12 in the manner of the reference's camera (ray.fut:93-107), computed in float64 and rounded once: the image plane `focal` from the
    origin, so the centre ray has d.d = focal^2 and the corner rays more."""
    lf, la = np.asarray(look_from, D), np.asarray(look_at, D)
    half_h = np.tan(np.radians(fov) / 2.0) * focal
    half_w = aspect * half_h
    wv = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(np.array([0.0, 1.0, 0.0]), wv)
    u /= np.linalg.norm(u)
    v = np.cross(wv, u)
    llc = lf - half_w * u - half_h * v - focal * wv
    return np.concatenate([lf, llc, 2 * half_w * u, 2 * half_h * v]).astype(F)


def scale_dirs(cam, s):
    """`llc - origin`, `horizontal` and `vertical` times s (a power of two): every primary direction times s, the origin where it was."""
    c = np.asarray(cam, dtype=F).copy()
    c[3:6] = (c[0:3].astype(D) + s * (c[3:6].astype(D) - c[0:3].astype(D))).astype(F)
    c[6:12] = (c[6:12].astype(D) * s).astype(F)
    return c


def primary_dd(cam, h, w):
    """d.d of every primary ray in the kernel's float32 arithmetic (lane_core.h: primary_ray), [h, w]."""
    c = np.asarray(cam, dtype=F)
    u = (np.arange(w, dtype=F) / F(w))[None, :]
    v = ((F(h) - np.arange(h, dtype=F)) / F(h))[:, None]
    d = [((c[3 + a] + u * c[6 + a]) + v * c[9 + a]) - c[a] for a in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def primary_gated(cam, h, w):
    """[h, w] bool: the primary ray is never culled -- d.d outside [2^-6, 2^20], or a zero direction component (max |1 / d_k| = inf)."""
    c = np.asarray(cam, dtype=F)
    u = (np.arange(w, dtype=F) / F(w))[None, :]
    v = ((F(h) - np.arange(h, dtype=F)) / F(h))[:, None]
    d = [np.broadcast_to(((c[3 + a] + u * c[6 + a]) + v * c[9 + a]) - c[a], (h, w)) for a in range(3)]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return ~((dd >= F(2.0 ** -6)) & (dd <= F(2.0 ** 20))) | (d[0] == 0) | (d[1] == 0) | (d[2] == 0)


# ---------------------------------------------------------------------------------------- scenes
def _colours(n, seed):
    return np.random.default_rng(seed).uniform(0.35, 0.95, (n, 3)).astype(F)


def grid(r_lo, r_hi, m=32, spacing=16.0, seed=5):
    """m x m spheres on the plane y = 0, `spacing` apart, centred on the origin, radii log-uniform in [r_lo, r_hi] with both ends present."""
    rng = np.random.default_rng(seed)
    n = m * m
    x = (np.arange(m, dtype=D) - (m - 1) / 2.0) * spacing
    xs, zs = np.meshgrid(x, x, indexing="ij")
    s = np.zeros((n, 7), F)
    s[:, 0], s[:, 2] = xs.ravel(), zs.ravel()
    s[:, 3:6] = _colours(n, seed + 1)
    r = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), n))
    r[n // 2 + 3], r[n // 3] = r_lo, r_hi
    s[:, 6] = r
    return s


R_MIN_AT, R_MAX_AT = 32 * 32 // 2 + 3, 32 * 32 // 3      # grid(): the spheres that carry r_lo and r_hi


def with_r_min(s, j, use):
    """s with sphere j's radius set so that the scene guard's 2 reach / (2^15 r_min) becomes `use` (sphere j then IS r_min)."""
    s = s.copy()
    s[j, 6] = s[:, 6].max()                               # (out of the way: reach depends on r_max and the centres only)
    reach = guards(s, 0)["reach"]
    s[j, 6] = F(2.0 * reach / (2.0 ** 15 * use))
    assert s[j, 6] == s[:, 6].min()
    return s


def cloud(seed=11):
    """8 x 8 x 16 spheres on a lattice 64, 64 and 32 apart, radii 4 .. 8 and one of 1/16: depth in every direction, for rays with three
    comparable direction components (a small one blows the limit's max |1 / d_k| up, and nothing is culled along such a ray)."""
    rng = np.random.default_rng(seed)
    xs, ys, zs = np.meshgrid((np.arange(8, dtype=D) - 3.5) * 64.0, (np.arange(8, dtype=D) - 3.5) * 64.0, (np.arange(16, dtype=D) - 7.5) * 32.0,
                             indexing="ij")
    n = xs.size
    s = np.zeros((n, 7), F)
    s[:, 0], s[:, 1], s[:, 2] = xs.ravel(), ys.ravel(), zs.ravel()
    s[:, 6] = rng.uniform(4.0, 8.0, n)
    s[R_MIN_AT, 6], s[R_MAX_AT, 6] = 1.0 / 16.0, 8.0
    s[:, 3:6] = _colours(n, seed + 1)
    return s


def packed(seed=21):
    """Close-packed: 16 spheres of radius 32 touching on a 4 x 4 grid, and 1008 spheres of radius 1/4 on a lattice 8 apart, each resting on the
    large sphere below it (touching it) or, in the gaps between four of them, on the plane of their centres.  A ray that lands on a small
    one leaves from beside a sphere 128 times its size."""
    big = np.array([[(i - 1.5) * 64.0, 0.0, (k - 1.5) * 64.0, 32.0] for i in range(4) for k in range(4)], D)
    rows = [b for b in big]
    for i in range(32):
        for k in range(32):
            if i % 8 == 0 and k % 8 == 0:
                continue
            x, z = (i - 15.5) * 8.0, (k - 15.5) * 8.0
            d2 = ((big[:, 0] - x) ** 2 + (big[:, 2] - z) ** 2).min()
            rows.append([x, np.sqrt(max(32.25 ** 2 - d2, 0.0)), z, 0.25])
    a = np.array(rows, D)
    s = np.zeros((a.shape[0], 7), F)
    s[:, 0:3], s[:, 6] = a[:, 0:3], a[:, 3]
    s[:, 3:6] = _colours(a.shape[0], seed + 1)
    return s


def coincident(s, k):
    """s with spheres 1 .. k - 1 moved onto sphere 0 (same centre, same radius: k equal Morton keys, ceil(log2 k) more levels there)."""
    s = s.copy()
    s[1:k, [0, 1, 2, 6]] = s[0, [0, 1, 2, 6]]
    return s


def scaled(s, k, shift=(0.0, 0.0, 0.0)):
    """Positions and radii times 2^k (exact), then the positions moved by `shift`."""
    s = s.copy()
    s[:, [0, 1, 2, 6]] = np.ldexp(s[:, [0, 1, 2, 6]], k)
    s[:, 0:3] = (s[:, 0:3].astype(D) + np.asarray(shift, D)).astype(F)
    return s


def scaled_cam(cam, k, shift=(0.0, 0.0, 0.0)):
    """The camera moved with `scaled`: every vector times 2^k, origin and lower-left corner moved by `shift`."""
    c = np.ldexp(np.asarray(cam, F), k).astype(D)
    c[0:3] += np.asarray(shift, D)
    c[3:6] += np.asarray(shift, D)
    return c.astype(F)


def c_max(s):
    s = np.asarray(s, F).astype(D)
    return (np.abs(s[:, 0:3]) + s[:, 6:7]).max()


# ---------------------------------------------------------------------------------------- the cases
def _height(s):
    import oracle_lib as O
    a = O.OracleScene("custom", spheres7=s, look_from=(0.0, 0.0, 1.0), look_at=(0.0, 0.0, 0.0), fov=40.0).arrays()
    return tree_height(a["left"], a["right"])


def _case(s, cams, h, w, intend, tags=()):
    """The Case with its expectation from the restatement; `intend` = (scene_ok, (origin_ok ...)) is what the construction aimed at."""
    s = np.ascontiguousarray(s, dtype=F)
    cams = [np.ascontiguousarray(c, dtype=F) for c in cams]
    g = guards(s, _height(s))
    oks = tuple(origin_ok(g, c[0:3]) for c in cams)
    assert (g["ok"], oks) == (intend[0], tuple(intend[1])), (g["ok"], oks, intend)
    return Case(s, cams, h, w, bool(g["ok"] and all(oks)), g["ok"], oks, frozenset(tags))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    IN, OUT = 1.0 - EPS, 1.0 + EPS
    near = camera((330.0, 60.0, 330.0), (0.0, 0.0, 0.0), 45.0)              # low over a corner of the grid, looking along its diagonal
    mid = camera((450.0, 120.0, 450.0), (0.0, 0.0, 0.0), 38.0, focal=0.93)  # every sphere at least 100 away; d.d in [0.86, 1.07]

    # far inside every guard, and the radius ratio 128 at 0.35 of the scene guard
    control, r128 = grid(2.0, 8.0), grid(1.0 / 16.0, 8.0)
    out["control"] = _case(control, [near], 96, 96, (True, [True]), ["control"])
    out["ratio128"] = _case(r128, [near], 96, 96, (True, [True]))

    # ---- scene guard: one sphere's radius sets r_min, just inside and just outside 2 reach = 2^15 r_min (radius ratio 365 on the grid,
    # 2^12 in the lattice with one sphere of radius 128.  The guard ties the ratio to the scene's extent, r_max / r_min = 2^14 / (1 + R / r_max),
    # and the limit's constant term is at least 2^-16 r_max^2 / r_min: nearer 2^14 the small spheres are squeezed into R << r_max while that
    # term stays near r_max / 4, a launch is still culled but no box can ever fail, and a wrong limit could not show)
    # (at the limit 2^15 r_min = 2 reach, so the camera guard leaves the origin `reach` = 359 around the centre: over the grid, not beside it)
    over = camera((215.0, 45.0, 215.0), (0.0, 0.0, 0.0), 50.0)
    out["scene_in"] = _case(with_r_min(r128, R_MIN_AT, IN), [over], 96, 96, (True, [True]), ["pair"])
    out["scene_out"] = _case(with_r_min(r128, R_MIN_AT, OUT), [over], 96, 96, (False, [False]), ["pair"])
    lat = cloud()
    lump = lat.copy()                                       # the lattice's far corner sphere grown to radius 128
    lump[0, 6] = 128.0
    # (kappa is c0 / (c2 2^-6), so that W2 kappa covers c0 for every admitted d.d: at d.d = 1 the constant term is 64 times what the proof needs
    # and swamps this scene; directions of length 1.05 / 8 keep it at its proper size)
    across = scale_dirs(camera((280.0, 230.0, 340.0), (0.0, 0.0, 0.0), 60.0, focal=1.05), 0.125)
    out["ratio_in"] = _case(with_r_min(lump, R_MIN_AT, IN), [across], 96, 96, (True, [True]), ["pair"])
    out["ratio_out"] = _case(with_r_min(lump, R_MIN_AT, OUT), [across], 96, 96, (False, [False]), ["pair"])
    assert out["ratio_in"].spheres7[:, 6].max() / out["ratio_in"].spheres7[:, 6].min() > 0.24 * 2.0 ** 14

    # ---- camera guard: the scene at 0.8 of its own guard, origins at |origin - centre| (1 + 2^-20) + reach = 2^15 r_min (1 -+ 2^-12)
    far_scene = with_r_min(r128, R_MIN_AT, 0.8)
    g = guards(far_scene, 0)

    def at_guard(direction, use):
        d = np.asarray(direction, D) / np.linalg.norm(direction)
        dist = (2.0 ** 15 * g["r_min"] * use - g["reach"]) / (1.0 + 2.0 ** -20)
        return camera(g["centre"] + dist * d, (0.0, 0.0, 0.0), 52.0)
    cam_in, cam_out, cam_in2 = at_guard((1.0, 0.12, 1.0), IN), at_guard((1.0, 0.12, 1.0), OUT), at_guard((-1.0, 0.2, 0.4), IN)
    out["camera_in"] = _case(far_scene, [cam_in], 96, 96, (True, [True]), ["pair"])
    out["camera_out"] = _case(far_scene, [cam_out], 96, 96, (True, [False]), ["pair"])
    out["camera_batch"] = _case(far_scene, [cam_in, cam_out, cam_in2], 64, 64, (True, [True, False, True]))

    # ---- the d.d gate: every primary direction times 1/8 and 1024 (one image straddles 2^-6, one 2^20), 1/16 and 2048 (wholly outside),
    # and a camera on the z axis whose centre column has d_x = 0 and centre row d_y = 0 exactly
    out["gate_low"] = _case(r128, [scale_dirs(mid, 0.125)], 96, 96, (True, [True]), ["gate_some"])
    out["gate_high"] = _case(r128, [scale_dirs(mid, 1024.0)], 96, 96, (True, [True]), ["gate_some"])
    out["gate_below"] = _case(r128, [scale_dirs(mid, 0.0625)], 96, 96, (True, [True]), ["gate_all"])
    out["gate_above"] = _case(r128, [scale_dirs(mid, 2048.0)], 96, 96, (True, [True]), ["gate_all"])
    axis = np.array([0.0, 0.0, 300.0, -0.5, -0.5, 299.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], F)
    tilted = r128.copy()                                   # the grid stood up to face the z axis: y <- z
    tilted[:, 1], tilted[:, 2] = r128[:, 2], 0.0
    out["gate_zero"] = _case(tilted, [axis], 96, 96, (True, [True]))
    dd = primary_dd(axis, 96, 96)
    assert dd.min() == 1.0 and (np.asarray(axis)[3] + F(0.5) * axis[6]) - axis[0] == 0.0

    # ---- magnitude, the camera scaled with the scene: the same image as at scale 1, but every primary ray is outside the gate.  At 2^40 a
    # coordinate's ulp is 2^16, so directions short enough for the gate vanish in the origin's rounding: only bounce rays are ever culled
    # there.  The small scenes get a second camera whose directions are brought back inside the gate.
    big_k = 24
    span = c_max(scaled(r128, big_k))
    for name, use, ok in (("cmax_in", IN, True), ("cmax_out", OUT, False)):
        shift = (2.0 ** 40 * use - span, 0.0, 0.0)
        s = scaled(r128, big_k, shift)
        assert abs(c_max(s) / 2.0 ** 40 - use) < EPS / 4
        out[name] = _case(s, [scaled_cam(mid, big_k, shift)], 96, 96, (ok, [ok]), ["pair", "gate_all"])
    # (a root needs t > 0.1 and the gate |d| >= 1/8, so a hit lies at least 2^-16 * 820 away; the camera guard allows 2^-16 * 1640; the
    # lattice has depth along a ray with three comparable components, which is what lets the limit fail boxes at r_min = 2^-20)
    tiny_cams = [scaled_cam(camera((300.0, 240.0, 360.0), (0.0, 0.0, 0.0), 60.0), -16),
                 scale_dirs(scaled_cam(camera((700.0, 560.0, 840.0), (0.0, 0.0, 0.0), 30.0, focal=1.05), -16), 2.0 ** 13)]
    at = scaled(lat, -16)
    assert at[:, 6].min() == F(2.0 ** -20)
    below = at.copy()
    below[R_MIN_AT, 6] = np.nextafter(F(2.0 ** -20), F(0.0))
    out["rmin_at"] = _case(at, tiny_cams, 96, 96, (True, [True, True]), ["pair", "gate_all"])
    out["rmin_below"] = _case(below, tiny_cams, 96, 96, (False, [False, False]), ["pair", "gate_all"])
    out["tiny_scene"] = _case(scaled(control, -16), [scaled_cam(near, -16), scale_dirs(scaled_cam(
        camera((950.0, 260.0, 950.0), (0.0, 0.0, 0.0), 24.0, focal=1.05), -16), 2.0 ** 13)], 96, 96, (True, [True, True]), ["gate_all"])

    # ---- tree height: 8 coincident spheres in the 32 x 32 grid make exactly floor(log2 1024) + 2 = 12 levels, 9 make 13; the 12-level tree
    # less one sphere has 1023 leaves and only 11 sweeps
    tall = coincident(r128, 8)
    out["height_at"] = _case(tall, [near], 96, 96, (True, [True]), ["pair"])
    out["height_over"] = _case(coincident(r128, 9), [near], 96, 96, (False, [False]), ["pair"])
    out["height_1023"] = _case(np.delete(tall, 700, axis=0), [near], 96, 96, (False, [False]), ["pair"])
    assert _height(tall) == 12 and _height(out["height_over"].spheres7) == 13 and _height(out["height_1023"].spheres7) == 12

    # ---- ties: coincident centres and exact duplicates (the tie goes to the lowest leaf) inside the scene at its guard
    ties = out["scene_in"].spheres7.copy()
    ties[100:140, 0:3] = ties[0:40, 0:3]
    ties[140:150] = ties[40:50]
    out["ties"] = _case(ties, [over], 96, 96, (True, [True]))

    # ---- bounces that start on tiny spheres beside huge ones
    down = camera((70.0, 95.0, 60.0), (32.0, 30.0, 32.0), 40.0)
    out["bounce"] = _case(packed(), [down], 128, 128, (True, [True]), ["bounce", "rmin_hits"])
    return out
