"""CPU checks of the ray paths: the restatement (path_ref.py) over its two objs_hit callables, against RefScene.ray_colour and the oracle's
chain lengths, its prefix and max_depth rules, its named faults, one bounce against the C++ arithmetic (build/path_check runs
query_core.h's path_bounce behind sphere_root and rehit_full), and the loader's symbols and Python signatures."""
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

import occlusion_ref as X
import oracle_lib as O
import path_ref as P
import ray_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# the end codes of seeded_rays(arr, 512, 17) at max_depth 3: (escaped, absorbed, truncated)
PREMISE = {"rgbbox": (335, 131, 46), "irreg": (312, 189, 11)}


@pytest.fixture(scope="module", params=["rgbbox", "irreg"])
def scene(request):
    orc = O.OracleScene(request.param)
    arr = orc.arrays()
    cam = Q.camera_rays(orc.camera_floats(40, 40), 40, 40)
    return request.param, orc, arr, Q.RefScene(arr), X.seeded_rays(arr, 512, 17), cam


def _colours(arr):
    return arr["L"][:, 3:6]


def test_the_two_objs_hit_callables_give_equal_paths(scene):
    name, orc, arr, ref, seeded, cam = scene
    for rays, what in ((seeded, "seeded"), (cam[::5], "camera")):
        for max_depth in (3, 50):
            a = P.trace_paths(P.oracle_hit(orc), _colours(arr), rays, max_depth, 8)
            b = P.trace_paths(P.ref_hit(ref), _colours(arr), rays, max_depth, 8)
            P.assert_same(b, a, f"{name} {what} max_depth={max_depth}")


def test_premise_every_end_code(scene):
    name, orc, arr, ref, seeded, cam = scene
    end = P.trace_paths(P.oracle_hit(orc), _colours(arr), seeded, 3, 1)[1]
    assert tuple(np.bincount(end, minlength=3)) == PREMISE[name]
    count, end = P.trace_paths(P.oracle_hit(orc), _colours(arr), seeded, 50, 1)[:2]
    got = np.bincount(end, minlength=3)
    assert got[P.ESCAPED] > 0 and got[P.ABSORBED] > 0 and got[P.TRUNCATED] == 0, got
    assert count.max() > 8


def test_colour_is_ray_colour(scene):
    name, orc, arr, ref, seeded, cam = scene
    for max_depth in (1, 3, 50):
        got = P.trace_paths(P.oracle_hit(orc), _colours(arr), seeded, max_depth, 1)[6]
        want = ref.ray_colour(seeded[:, :3], seeded[:, 3:], max_depth)
        assert np.array_equal(P.bits(got), P.bits(want)), max_depth
        assert np.array_equal(P.bits(got), P.bits(orc.ray_colour_rays(seeded, max_depth))), max_depth


@pytest.mark.parametrize("max_depth", [1, 3, 50])
def test_objs_hit_calls_are_the_chain_lengths(scene, max_depth):
    name, orc, arr, ref, seeded, cam = scene
    count, end = P.trace_paths(P.oracle_hit(orc), _colours(arr), cam, max_depth, 1)[:2]
    want = orc.chain_lengths(40, 40, max_depth=max_depth)
    assert np.array_equal(P.objs_hit_calls(count, end).reshape(40, 40), want)
    assert (count <= max_depth).all() and ((end == P.TRUNCATED) <= (count == max_depth)).all()
    if max_depth == 50:
        assert count.max() == {"rgbbox": 28, "irreg": 9}[name]


def test_prefix_over_k_and_padding(scene):
    name, orc, arr, ref, seeded, cam = scene
    rays = np.concatenate([seeded, cam[::7]])
    full = P.trace_paths(P.oracle_hit(orc), _colours(arr), rays, 50, 64)
    count, end, index, hit = full[:4]
    assert count.max() > 3
    filled = np.arange(64)[None, :] < count[:, None]
    assert np.array_equal(index >= 0, filled) and not hit[~filled].any()
    for k in (1, 3, 8):
        P.assert_same(P.trace_paths(P.oracle_hit(orc), _colours(arr), rays, 50, k), P.prefix(full, k), f"{name} k={k}")


def test_max_depth_zero(scene):
    name, orc, arr, ref, seeded, cam = scene
    count, end, index, hit, light, last, colour = P.trace_paths(P.oracle_hit(orc), _colours(arr), seeded, 0, 4)
    assert not count.any() and (end == P.TRUNCATED).all() and (index == -1).all() and not hit.any()
    assert (light == 1).all() and np.array_equal(P.bits(last), P.bits(seeded)) and not P.bits(colour).any()


def _near_root_rays(arr, m=64):
    """rays that start 0.05 in front of a sphere, towards its centre: the fold takes root 2 (root 1 <= 0.1), the re-intersection root 1"""
    rng = np.random.default_rng(5)
    L = arr["L"]
    j = rng.integers(0, L.shape[0], m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = L[j, :3] - u * (L[j, 6:7] + 0.05)
    return np.concatenate([o, u], axis=1).astype(F)


@pytest.mark.parametrize("fault", sorted(P.FAULTS))
def test_every_named_fault_is_caught(scene, fault):
    name, orc, arr, ref, seeded, cam = scene
    rays = np.concatenate([seeded, _near_root_rays(arr)])
    hit_fn = P.fold_hit(ref) if fault == "root_from_fold" else P.ref_hit(ref)
    # (irreg's spheres are white, which hides a wrong light: the faults are shown with colours that differ from 1 and from one another)
    colours = np.linspace(0.3, 0.95, 3 * ref.n, dtype=F).reshape(-1, 3)
    want = P.trace_paths(P.ref_hit(ref), colours, rays, 3, 4)
    got = P.trace_paths(hit_fn, colours, rays, 3, 4, None if fault == "root_from_fold" else fault)
    diff = P.differing(got, want)
    for output in P.FAULTS[fault]:
        assert output in diff, f"{fault}: not reported under {output} (reported: {sorted(diff)})"
    with pytest.raises(AssertionError, match=P.FAULTS[fault][0] + " differs"):
        P.assert_same(got, want, fault)


def _ulp_steps(x, lo, hi):
    """the float32 values lo .. hi ulps from x"""
    return (np.array([x], F).view(np.int32)[0] + np.arange(lo, hi + 1)).astype(np.int32).view(F)


def _axis_case(perm, along, across, centre_along, x, r, speed, zeros=(1.0, 1.0, 1.0, 1.0)):
    """a ray along axis perm[0] (sign `along`) whose LINE touches the sphere of radius |r| at its pole on axis perm[1] (sign `across`); the
    origin lies x in front of the touching point.  zeros: the signs of the four zeros (direction on perm[1], perm[2]; origin, centre on perm[2])"""
    o, d, c = np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
    c[perm[0]], c[perm[2]] = F(centre_along), F(0.0) * F(zeros[3])
    o[perm[0]], o[perm[1]], o[perm[2]] = F(centre_along) - F(along) * F(x), F(across) * F(abs(r)), F(0.0) * F(zeros[2])
    d[perm[0]], d[perm[1]], d[perm[2]] = F(along) * F(speed), F(0.0) * F(zeros[0]), F(0.0) * F(zeros[1])
    return np.concatenate([o, d, c, [0.5, 0.25, 0.75], [r], [0.9, 0.8, 0.7]]).astype(F)


def knife_edge_cases():
    """Cases on scatter's knife edge, dot(reflected, normal) at and within rounding of 0 on both sides.  A true grazing hit cannot get there:
    with a chord of half-length h the dot is -+h / radius, and float32 inputs keep h / radius above sqrt(2^-23) ~ 3e-4.  The edge is
    reached where the ROOT's rounding makes the hit, so every case here is axis-aligned with short mantissas (oc and its squares exact):
      * chord: x^2 a few ulps above a multiple of ulp(radius^2): c = |oc|^2 - radius^2 rounds to that multiple, the discriminant is the
        few ulps left, the near root is taken in front of the sphere: dot = +h / radius, h / radius from 2^-23.5 up;
      * touch: the origin so close to the touching point that c rounds to 0: the near root is 0 and refused, the far root 2x is taken from
        behind: dot ~ -x / radius, x / radius from 2^-12 down to 2^-40;
      * zero: the touch family with the centre so far along the ray that p = o + t d rounds ONTO the touching point: normal . direction
        is exactly 0, over every sign of the zero components and of the radius (a negative radius turns the normal: -0)."""
    rows = []
    for perm, along, across in itertools.product(((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)), (1.0, -1.0), (1.0, -1.0)):
        for r in (F(1) - F(2.0 ** -12), F(1.0), F(0.5) - F(2.0 ** -13), F(4) - F(2.0 ** -10)):
            grid = np.spacing(F(r * r) * F(1 - 2.0 ** -20))
            for m in (1, 2, 3, 5):
                for x in _ulp_steps(np.sqrt(np.float64(m) * np.float64(grid)), -6, 6):
                    rows.append(_axis_case(perm, along, across, 0.0, x, r, F(2.0 ** -14) * r))
            for e in range(-40, -11):
                x = F(2.0 ** e) * F(1.25) * r
                rows.append(_axis_case(perm, along, across, 0.0, x, r, x * F(4)))
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)):
        for far, r, x in ((2.0 ** 20, 256.0, 2.0 ** -4), (2.0 ** 16, 16.0, 2.0 ** -8), (2.0 ** 22, 1024.0, 0.25)):
            for along, across, turn, *zeros in itertools.product((1.0, -1.0), repeat=7):
                rows.append(_axis_case(perm, along, across, far, x, F(turn) * F(r), 4 * x, zeros))
    return np.array(rows, F)


def bounce_case_set(seed=20261019, m=6000):
    """(m', 16) float32 cases for build/path_check: random rays at a sphere, grazing rays (offsets a few ulps to 1e-4 inside the rim),
    origins inside and on the sphere, origins a little in front of it (the re-intersection's other root), zero, tiny and huge directions,
    non-finite components, and knife_edge_cases()"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, (m, 3))
    r = rng.uniform(0.2, 5.0, m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(m, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    speed = 10.0 ** rng.uniform(-2, 2, m)
    dist = rng.uniform(1.0, 30.0, m) + r
    kind = rng.integers(0, 8, m)
    off = rng.uniform(0, 1.3, m) * r
    graze = kind == 1
    off[graze] = (r * (1 - 2.0 ** -rng.integers(8, 24, m)))[graze]
    o = c - u * dist[:, None] + w * off[:, None]
    inside = kind == 2
    o[inside] = (c + u * (rng.uniform(0, 0.99, m) * r)[:, None])[inside]
    graze_in = kind == 3                                  # grazing from the inside: just below the surface, moving along it ...
    eps_in = 2.0 ** -rng.integers(8, 24, m)
    o[graze_in] = (c + w * (r * (1 - eps_in))[:, None])[graze_in]
    speed[graze_in] = (r * np.sqrt(2 * eps_in) / rng.uniform(0.2, 2.0, m))[graze_in]   # ... slowly: the exit lies past scene_epsilon
    surf = kind == 4
    o[surf] = (c - u * r[:, None])[surf]
    front = kind == 5
    o[front] = (c - u * (r + rng.uniform(0.0, 0.1, m))[:, None])[front]
    d = u * speed[:, None]
    d[front] = u[front]
    cases = np.concatenate([o, d, c, rng.uniform(0.0, 1.0, (m, 3)), r[:, None], rng.uniform(0.0, 1.0, (m, 3))], axis=1).astype(F)
    special = cases[: 16 * 12].copy()
    for i in range(16 * 12):
        special[i, i % 16] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 1e-30, 3e38, np.nan, 0.0, np.inf][i // 16]
    zero = cases[300:360].copy()
    zero[:, 3:6] = np.where(rng.random((60, 3)) < 0.5, F(0.0), F(-0.0))
    huge = cases[400:460].copy()
    huge[:, 3:6] *= F(1e20)
    tiny = cases[500:560].copy()
    tiny[:, 3:6] *= F(1e-22)
    return np.concatenate([cases, special, zero, huge, tiny, knife_edge_cases()]).astype(F)


def _same_words(got, want):
    """rows whose words differ; in the float words any NaN matches any NaN (a NaN's payload depends on the operand order the compiler and
    numpy choose)"""
    gf, wf = got[:, 1:].view(F), want[:, 1:].view(F)
    bad = (got[:, 1:] != want[:, 1:]) & ~(np.isnan(gf) & np.isnan(wf))
    return np.nonzero((got[:, 0] != want[:, 0]) | bad.any(axis=1))[0]


def test_path_check_agrees_with_the_restatement(tmp_path):
    exe = os.path.join(ROOT, "build", "path_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/path_check"], check=True, capture_output=True)
    cases = bounce_case_set()
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.tofile(src)
    kinds = {}
    for depth, max_depth in ((0, 50), (2, 3), (49, 50), (0, 1)):
        r = subprocess.run([exe, str(src), str(dst), str(depth), str(max_depth)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(dst, dtype=np.uint32).reshape(-1, 20)
        assert got.shape[0] == cases.shape[0]
        want, info = P.bounce_cases(cases, depth, max_depth)
        bad = _same_words(got, want)
        assert bad.size == 0, f"depth {depth} of {max_depth}: {bad.size} cases differ, first {bad[:5]}: {cases[bad[:3]]}"
        assert np.isfinite(want[:, 1:].view(F)).mean() > 0.9
        kinds[(depth, max_depth)] = np.bincount(want[:, 0], minlength=4)
    # the case set reaches the three end codes and "continue"; depth + 1 == max_depth turns every continue into a truncation
    first = kinds[(0, 50)]
    assert first[P.ESCAPED] > 500 and first[P.ABSORBED] > 500 and first[P.CONTINUE] > 1500 and first[P.TRUNCATED] == 0, first
    for key in ((2, 3), (49, 50), (0, 1)):
        k = kinds[key]
        assert k[P.TRUNCATED] == first[P.CONTINUE] and k[P.CONTINUE] == 0 and k[P.ESCAPED] == first[P.ESCAPED] and k[P.ABSORBED] == first[P.ABSORBED], (key, k)
    # grazing hits on both sides of scatter's test, the re-intersection's other root, and degenerate directions are all in the set
    want, info = P.bounce_cases(cases, 0, 50)
    with np.errstate(invalid="ignore"):
        small = info["have"] & (np.abs(info["dot"]) < 2.0 ** -8)
        assert (small & (info["dot"] > 0)).sum() > 50 and (small & ~(info["dot"] > 0)).sum() > 50
        # ... and scatter's knife edge: dot(reflected, normal) within rounding of 0 (1e-7 < 2^-23, an ulp of the unit vectors) on both sides,
        # where the chain goes on and where it ends, and exactly +0 and -0, where it ends
        edge = info["have"] & (np.abs(info["dot"]) <= 1e-7)
        above, below, zero = edge & (info["dot"] > 0), edge & (info["dot"] < 0), edge & (info["dot"] == 0)
        assert above.sum() >= 100 and (want[above, 0] == P.CONTINUE).all(), above.sum()
        assert below.sum() >= 500 and (want[below, 0] == P.ABSORBED).all(), below.sum()
        assert (info["have"] & (info["dot"] > 0) & (info["dot"] <= 1e-10)).sum() >= 50 and (below & (info["dot"] >= -1e-10)).sum() >= 100
        assert (zero & ~np.signbit(info["dot"])).sum() >= 200 and (zero & np.signbit(info["dot"])).sum() >= 200, zero.sum()
        assert (want[zero, 0] == P.ABSORBED).all()
        assert (info["have"] & (info["t"] > 0) & (info["t"] <= F(0.1))).sum() > 100      # root 1 <= 0.1: only the re-intersection returns it
    assert (~np.isfinite(want[:, 1:].view(F))).any()


def test_library_exports_paths():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_trace_paths", "rt_trace_paths_shaped"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_trace_paths.argtypes) == 13
    assert len(_lib.lib.rt_trace_paths_shaped.argtypes) == 14
    assert (R.PATH_ESCAPED, R.PATH_ABSORBED, R.PATH_TRUNCATED) == (0, 1, 2) == (P.ESCAPED, P.ABSORBED, P.TRUNCATED)
    assert list(inspect.signature(R.trace_paths).parameters) == ["prepared", "rays", "k", "max_depth", "rays_per_wave"]
    sig = inspect.signature(R.trace_paths)
    assert (sig.parameters["max_depth"].default, sig.parameters["rays_per_wave"].default) == (R.MAX_DEPTH, 0)
    assert list(inspect.signature(R.trace_paths_into).parameters) == [
        "rays_ptr", "n", "prepared", "k", "count_ptr", "end_ptr", "index_ptr", "hit_ptr", "light_ptr", "last_ray_ptr", "colour_ptr", "max_depth",
        "rays_per_wave"]
    assert not hasattr(R, "paths_auto_rays_per_wave")      # the launch rule is the library's; the tests restate it (path_ref.py)


def test_the_restated_launch_rule():
    # the documented rule: 64 up to 64 * 8 * CUs rays, then the multiple of 64 that keeps 8 * CUs waves, at most 256
    assert P.auto_rays_per_wave(1, 256) == 64 and P.auto_rays_per_wave(64 * 8 * 256, 256) == 64
    assert P.auto_rays_per_wave(64 * 8 * 256 + 1, 256) == 128 and P.auto_rays_per_wave(1 << 18, 256) == 128
    assert P.auto_rays_per_wave(3 * 64 * 8 * 256, 256) == 192 and P.auto_rays_per_wave(10 ** 6, 256) == 256
    assert P.auto_rays_per_wave((1 << 31) - 1, 256) == 256 and P.auto_rays_per_wave(10 ** 6, 0) == 256


def test_header_declares_paths():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_trace_paths(", "rt_trace_paths_shaped(", "RT_PATH_ESCAPED = 0, RT_PATH_ABSORBED = 1, RT_PATH_TRUNCATED = 2", "family=paths k="):
        assert sym in h, sym
