"""Visibility matrices on the GPU: rt_visible_pairs against the numpy restatement (pairs_ref.py), against the library's own rt_occluded_rays
on the materialised pairs, across word boundaries and launch shapes between guard words, from unaligned inputs, with invalid pairs, on
degenerate scenes, its refusals, and two calls in flight.  Every comparison is ==.

The references are computed once (lru_cache) and shared; pairs are independent of one another, so the answer for the first n points and m
targets of a set is the top-left block of the set's matrix."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_rays as E
import oracle_lib as O
import pairs_ref as P
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
N, M = 67, 130
INTERVALS = ((1e-3, 1.0), (0.1, 1e9), (0.5, 30.0), (7.0, 7.0))
MODES = (P.TARGETS, P.DIRECTIONS)
GUARD = 4          # guard words (mask) and guard ints (count) on either side of an output
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


@pytest.fixture(scope="module")
def prepared(R, ctx):
    made = {}
    for spec in ("rgbbox", "irreg"):
        scene = ctx.scene(spec)
        made[spec] = (scene, R.prepare_scene(64, 64, scene))
    yield {k: v[1] for k, v in made.items()}
    for scene, ps in made.values():
        ps.free()
        scene.free()


@functools.lru_cache(maxsize=None)
def _scene(spec):
    if spec in E.SCENES:
        s, lf, la, fov = E.SCENES[spec]
        arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    else:
        arr = O.OracleScene(spec).arrays()
    return arr, Q.RefScene(arr)


@functools.lru_cache(maxsize=None)
def _inputs(spec):
    return P.seeded(_scene(spec)[0], N, M, P.SEEDS.get(spec, 41))


def _targets(spec, mode):
    _, targets, directions = _inputs(spec)
    return targets if mode == P.TARGETS else directions


@functools.lru_cache(maxsize=None)
def _want(spec, mode, interval):
    """(N, M) bool: the restatement's matrix of the seeded set"""
    vis = P.visible(_scene(spec)[1], _inputs(spec)[0], _targets(spec, mode), mode, *interval)
    vis.setflags(write=False)
    return vis


def _kw(mode, tg):
    return {"targets": tg} if mode == P.TARGETS else {"directions": tg}


def _string(mode, mask=True, count=True):
    return "family=pairs " + ("targets" if mode == P.TARGETS else "directions") + (" mask" if mask else "") + (" count" if count else "")


class _Guarded:
    """A mask and a count buffer for n points and m targets, poisoned, with guards on either side."""

    def __init__(self, n, m):
        import torch
        self.n, self.words = n, (m + 63) // 64
        self.mask = torch.full((2 * GUARD + n * self.words,), -1, dtype=torch.int64, device="cuda")          # every byte 0xFF
        self.count = torch.full((2 * GUARD + n,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.mask_ptr = self.mask.data_ptr() + 8 * GUARD
        self.count_ptr = self.count.data_ptr() + 4 * GUARD

    def read(self, what, mask=True, count=True):
        mk, ct = self.mask.cpu().numpy(), self.count.cpu().numpy()
        assert (mk[:GUARD] == -1).all() and (mk[GUARD + self.n * self.words:] == -1).all(), f"{what}: a guard word of the mask was written"
        assert (ct[:GUARD] == POISON).all() and (ct[GUARD + self.n:] == POISON).all(), f"{what}: a guard of the count was written"
        mk, ct = mk[GUARD:GUARD + self.n * self.words], ct[GUARD:GUARD + self.n]
        if not mask:
            assert (mk == -1).all(), f"{what}: the mask was written by a count-only call"
        if not count:
            assert (ct == POISON).all(), f"{what}: the count was written by a mask-only call"
        return mk.view(np.uint64).reshape(self.n, self.words), ct

    def untouched(self, what):
        self.read(what, mask=False, count=False)


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


# --------------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_against_restatement(R, ctx, prepared, spec, mode, interval):
    ps = prepared[spec]
    assert np.array_equal(ps.bvh_arrays()["L"], _scene(spec)[0]["L"])
    points, tg = _inputs(spec)[0], _targets(spec, mode)
    want = _want(spec, mode, interval)
    ok = P.valid_pairs(points, tg, mode)
    if interval == (7.0, 7.0):
        assert np.array_equal(want, ok)                       # the empty interval: every valid pair is visible
    elif interval in ((1e-3, 1.0), (0.1, 1e9)):
        assert want.any() and (ok & ~want).any()
    want_words, want_count = P.pack(want), want.sum(axis=1).astype(np.int32)
    try:
        for variant in (R.VARIANT_AUTO, R.VARIANT_POOLED, R.VARIANT_PIXEL, R.VARIANT_PERSISTENT):
            ctx.set_variant(variant)
            words, count = R.visible_pairs(ps, points, t_min=interval[0], t_max=interval[1], **_kw(mode, tg))
            assert ctx.last_launch == _string(mode), ctx.last_launch
            assert words.dtype == np.uint64 and words.shape == (N, 3) and count.dtype == np.int32 and count.shape == (N,)
            bad = np.argwhere(R.unpack_visible(words, M) != want)
            assert bad.size == 0, f"{spec} mode {mode} {interval} variant {variant}: {len(bad)} pairs differ, first {bad[:5].tolist()}"
            assert np.array_equal(words, want_words)          # (the tail bits too)
            assert np.array_equal(count, want_count)
            assert np.array_equal(count, P.popcount(words))
    finally:
        ctx.set_variant(R.VARIANT_AUTO)


# ----------------------------------------------------------------------------------------------- 2. against the library's occluded_rays
def _by_occluded_rays(R, ps, points_t, tg_t, mode, t0, t1):
    """(visible (n, m) bool, valid (n, m) bool) by the route a caller has without rt_visible_pairs: the n * m rays materialised with torch in
    float32, rt_occluded_rays, and the validity rule."""
    import torch
    n, m = points_t.shape[0], tg_t.shape[0]
    o = points_t[:, None, :].expand(n, m, 3)
    d = tg_t[None, :, :] - points_t[:, None, :] if mode == P.TARGETS else tg_t[None, :, :].expand(n, m, 3)
    rays = torch.cat([o, d], dim=2).reshape(n * m, 6).contiguous()
    valid = (torch.isfinite(rays).all(dim=1) & (rays[:, 3:] != 0).any(dim=1)).cpu().numpy().reshape(n, m)
    occ = R.occluded_rays(ps, rays, t0, t1).reshape(n, m)
    return valid & ~occ, valid


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("spec", ["rgbbox", "irreg"])
def test_against_occluded_rays(R, ctx, prepared, spec, mode):
    arr = _scene(spec)[0]
    points, targets, directions = P.seeded(arr, 515, 193, P.SEEDS[spec] + 100)
    pt, tt = _device(points), _device(targets if mode == P.TARGETS else directions)
    for ps_name in ("host", "device"):
        if ps_name == "host":
            ps = prepared[spec]
        else:
            sph = _device(arr["L"][np.random.default_rng(9).permutation(arr["L"].shape[0])])
            ps = R.prepare_scene_from_spheres(ctx, sph, 64, 64, (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0)
        try:
            for t0, t1 in ((1e-3, 1.0), (0.1, 1e9)):
                want, valid = _by_occluded_rays(R, ps, pt, tt, mode, t0, t1)
                assert valid.all()
                assert want.any() and not want.all()
                words, count = R.visible_pairs(ps, pt, t_min=t0, t_max=t1, **_kw(mode, tt))
                got = R.unpack_visible(words, 193)
                bad = np.argwhere(got[valid] != want[valid])
                assert bad.size == 0, f"{spec} {ps_name} mode {mode} ({t0}, {t1}): {len(bad)} pairs differ from occluded_rays"
                assert np.array_equal(count, want.sum(axis=1))
        finally:
            if ps_name == "device":
                ps.free()


# ------------------------------------------------------------------------------------------- 3. word boundaries and launch shapes
SMALL_M = (1, 2, 3, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129)   # (up to 32: the packed shape, 64 / G points per wave, G = 1 .. 32)


@pytest.mark.parametrize("n", [1, 2, 65])
@pytest.mark.parametrize("mode", MODES)
def test_word_boundaries(R, ctx, prepared, mode, n):
    ps = prepared["rgbbox"]
    interval = (1e-3, 1.0) if mode == P.TARGETS else (0.1, 1e9)
    full = _want("rgbbox", mode, interval)
    pt, tt = _device(_inputs("rgbbox")[0]), _device(_targets("rgbbox", mode))
    for m in SMALL_M:
        want = full[:n, :m]
        want_words, want_count = P.pack(want), want.sum(axis=1).astype(np.int32)
        words_n = (m + 63) // 64
        # words_per_wave 0: the library's rule (m <= 32: the packed shape); then the general shape with one word per wave, two, and the
        # whole row (5 is above every row here)
        for wpw in (0, 1, 2, 5):
            for mask, count in ((True, True), (True, False), (False, True)):
                what = f"mode {mode} n={n} m={m} words/wave={wpw} mask={mask} count={count}"
                g = _Guarded(n, m)
                R.visible_pairs_into(pt.data_ptr(), n, tt.data_ptr(), m, ps, mode, g.mask_ptr if mask else None, g.count_ptr if count else None,
                                     interval[0], interval[1], words_per_wave=wpw)
                ctx.sync()
                assert ctx.last_launch == _string(mode, mask, count) + (f" words/wave={min(wpw, words_n)}" if wpw else ""), ctx.last_launch
                words, cnt = g.read(what, mask, count)
                if mask:
                    assert np.array_equal(words, want_words), what
                    assert not R.unpack_visible(words, 64 * words_n)[:, m:].any(), f"{what}: a tail bit is set"
                if count:
                    assert np.array_equal(cnt, want_count), what


@pytest.mark.parametrize("mode", MODES)
def test_rule_steps_and_shapes_on_long_rows(R, ctx, prepared, mode):
    # The library's rule cuts a row into runs of at most 8 words once the points alone fill the machine (64 waves per CU: 16384 points on
    # 256 CUs): with 16400 points a row of 8 words (m = 512) is one run, 9 words (m = 513 .. 576) two, 17 words (m = 1025) three.  Against
    # rt_occluded_rays on the materialised pairs; every caller's shape gives the same words and counts.
    ps = prepared["irreg"]
    arr = _scene("irreg")[0]
    n = 16400
    points, targets, directions = P.seeded(arr, n, 1025, 77)
    interval = (1e-3, 1.0) if mode == P.TARGETS else (0.1, 1e9)
    pt, tt = _device(points), _device(targets if mode == P.TARGETS else directions)
    full, valid = _by_occluded_rays(R, ps, pt, tt, mode, *interval)
    assert valid.all() and full.any() and not full.all()
    for m in (511, 512, 513, 576, 577, 1025):
        want = full[:, :m]
        want_words, want_count = P.pack(want), want.sum(axis=1).astype(np.int32)
        for wpw in (0, 1, 3, 8, 9, 17) if m in (513, 1025) else (0,):
            g = _Guarded(n, m)
            R.visible_pairs_into(pt.data_ptr(), n, tt.data_ptr(), m, ps, mode, g.mask_ptr, g.count_ptr, *interval, words_per_wave=wpw)
            ctx.sync()
            words, cnt = g.read(f"m={m} words/wave={wpw}")
            assert np.array_equal(words, want_words), (m, wpw)
            assert np.array_equal(cnt, want_count), (m, wpw)


# --------------------------------------------------------------------------------------------------------------- 4. unaligned inputs
def _at_4_mod_16(a):
    """A device copy of the float32 array `a` whose first element is at an address that is 4 mod 16 -> (holder, pointer)"""
    import torch
    flat = np.ascontiguousarray(a, dtype=F).reshape(-1)
    buf = torch.zeros(flat.size + 8, dtype=torch.float32, device="cuda")
    off = ((4 - buf.data_ptr() % 16) % 16) // 4
    buf[off:off + flat.size] = torch.from_numpy(flat).cuda()
    ptr = buf.data_ptr() + 4 * off
    assert ptr % 16 == 4
    return buf, ptr


@pytest.mark.parametrize("mode", MODES)
def test_unaligned_inputs(R, ctx, prepared, mode):
    ps = prepared["rgbbox"]
    interval = (1e-3, 1.0) if mode == P.TARGETS else (0.1, 1e9)
    want = _want("rgbbox", mode, interval)
    hold_p, pp = _at_4_mod_16(_inputs("rgbbox")[0])
    hold_t, tp = _at_4_mod_16(_targets("rgbbox", mode))
    g = _Guarded(N, M)
    R.visible_pairs_into(pp, N, tp, M, ps, mode, g.mask_ptr, g.count_ptr, *interval)
    ctx.sync()
    words, cnt = g.read("unaligned")
    assert np.array_equal(words, P.pack(want))
    assert np.array_equal(cnt, want.sum(axis=1))


# ------------------------------------------------------------------------------------------------------------------ 5. invalid pairs
@pytest.mark.parametrize("mode", MODES)
def test_invalid_pairs(R, ctx, prepared, mode):
    ps = prepared["rgbbox"]
    interval = (1e-3, 1.0) if mode == P.TARGETS else (0.1, 1e9)
    base = _want("rgbbox", mode, interval)
    points, tg = _inputs("rgbbox")[0].copy(), _targets("rgbbox", mode).copy()
    assert base[3].any() and base[:, 6].any() and base[:, 70].any() and base[9].any()
    points[3, 1] = np.nan                   # a NaN point: row 3
    tg[6, 0] = np.inf                       # an infinite target / direction: column 6
    tg[70] = (0.0, -0.0, 0.0)               # DIRECTIONS: a zero direction, column 70 (TARGETS: a target at the origin, an ordinary one)
    points[9] = tg[100]                     # TARGETS: a point equal to its target, pair (9, 100) (row 9 is a new point in both modes)
    ok = P.valid_pairs(points, tg, mode)
    assert not ok[3].any() and not ok[:, 6].any() and (mode == P.DIRECTIONS or not ok[9, 100]) and (mode == P.TARGETS or not ok[:, 70].any())
    # what the restatement says about the rows and columns whose inputs changed; every other pair keeps its inputs and so its answer
    want = base.copy()
    ref = _scene("rgbbox")[1]
    want[3] = False
    want[:, 6] = False
    want[9] = P.visible(ref, points[9:10], tg, mode, *interval)[0]
    want[:, 70] = P.visible(ref, points, tg[70:71], mode, *interval)[:, 0]
    want[3, 70] = False
    assert not (want & ~ok).any()
    words, count = R.visible_pairs(ps, points, t_min=interval[0], t_max=interval[1], **_kw(mode, tg))
    got = R.unpack_visible(words, M)
    assert not (got & ~ok).any(), "an invalid pair is visible"
    changed = np.zeros_like(ok)
    changed[[3, 9]] = True
    changed[:, [6, 70]] = True
    assert np.array_equal(got[~changed], base[~changed]), "a pair with unchanged inputs changed"
    assert np.array_equal(got, want)
    assert np.array_equal(count, want.sum(axis=1))
    assert count[3] == 0


# --------------------------------------------------------------------------------------------------------------- 6. degenerate scenes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["two_apart", "same64"])
def test_degenerate_scenes(R, ctx, name, mode):
    s, lf, la, fov = E.SCENES[name]
    arr = _scene(name)[0]
    scene = ctx.scene_from_spheres(s, lf, la, fov)
    ps = R.prepare_scene(64, 64, scene)
    try:
        got_bvh = ps.bvh_arrays()
        for k in ("L", "bmin", "bmax", "left", "right"):
            assert got_bvh[k].tobytes() == arr[k].tobytes(), (name, k)
        points, tg = _inputs(name)[0], _targets(name, mode)
        for interval in ((1e-3, 1.0), (0.0, 1e9)):
            want = _want(name, mode, interval)
            words, count = R.visible_pairs(ps, points, t_min=interval[0], t_max=interval[1], **_kw(mode, tg))
            assert np.array_equal(words, P.pack(want)), (name, mode, interval)
            assert np.array_equal(count, want.sum(axis=1)), (name, mode, interval)
        assert _want(name, mode, (0.0, 1e9)).any() and not _want(name, mode, (0.0, 1e9)).all()
    finally:
        ps.free()
        scene.free()


# ------------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(R, ctx, prepared):
    from raytracers_amd._lib import lib
    ps = prepared["rgbbox"]
    pt, tt = _device(_inputs("rgbbox")[0]), _device(_targets("rgbbox", P.TARGETS))
    g = _Guarded(N, M)
    pp, tp, mp, cp = C.c_void_p(pt.data_ptr()), C.c_void_p(tt.data_ptr()), C.c_void_p(g.mask_ptr), C.c_void_p(g.count_ptr)
    before = ctx.last_launch

    def refused(rc, what):
        assert rc != 0, what
        assert lib.rt_last_error(ctx._h).decode() != "", what
        ctx.sync()
        g.untouched(what)
        assert ctx.last_launch == before, what

    call = lib.rt_visible_pairs
    refused(call(ctx._h, None, N, pp, M, tp, 0, 0.0, 1.0, mp, cp), "null scene")
    refused(call(ctx._h, ps._h, -1, pp, M, tp, 0, 0.0, 1.0, mp, cp), "n < 0")
    refused(call(ctx._h, ps._h, 1 << 31, pp, 1, tp, 0, 0.0, 1.0, mp, cp), "n = 2^31")
    refused(call(ctx._h, ps._h, N, pp, 0, tp, 0, 0.0, 1.0, mp, cp), "m = 0")
    refused(call(ctx._h, ps._h, N, pp, -5, tp, 0, 0.0, 1.0, mp, cp), "m < 0")
    refused(call(ctx._h, ps._h, N, pp, (1 << 24) + 1, tp, 0, 0.0, 1.0, mp, cp), "m > 2^24")
    refused(call(ctx._h, ps._h, 1 << 25, pp, 4096, tp, 0, 0.0, 1.0, mp, cp), "n * W = 2^31")
    refused(call(ctx._h, ps._h, N, None, M, tp, 0, 0.0, 1.0, mp, cp), "NULL points")
    refused(call(ctx._h, ps._h, N, pp, M, None, 0, 0.0, 1.0, mp, cp), "NULL targets")
    refused(call(ctx._h, ps._h, N, pp, M, tp, 0, 0.0, 1.0, None, None), "both outputs NULL")
    refused(call(ctx._h, ps._h, N, pp, M, tp, 2, 0.0, 1.0, mp, cp), "mode 2")
    refused(call(ctx._h, ps._h, N, pp, M, tp, -1, 0.0, 1.0, mp, cp), "mode -1")
    for t0, t1 in ((float("nan"), 1.0), (0.0, float("inf")), (0.0, float("nan")), (-1.0, 1.0), (2.0, 1.0), (0.0, 2e9), (-0.5, -0.1),
                   (float("-inf"), 1.0)):
        refused(call(ctx._h, ps._h, N, pp, M, tp, 0, t0, t1, mp, cp), f"interval ({t0}, {t1})")
    refused(lib.rt_visible_pairs_shaped(ctx._h, ps._h, N, pp, M, tp, 0, 0.0, 1.0, mp, cp, -1), "words_per_wave < 0")
    with pytest.raises(R.RtError):
        R.visible_pairs(ps, pt, targets=tt, t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError):
        R.visible_pairs(ps, pt)
    with pytest.raises(ValueError):
        R.visible_pairs(ps, pt, targets=tt, directions=tt)
    with pytest.raises(ValueError):
        R.visible_pairs(ps, pt, targets=tt, mask=False, count=False)
    # n == 0 succeeds without a launch and writes nothing; (n * W = 2^31 - 64 passes the size checks: refused nowhere, but not run here)
    assert call(ctx._h, ps._h, 0, pp, M, tp, 0, 0.0, 1.0, mp, cp) == 0
    assert ctx.last_launch == "family=none (no points)"
    ctx.sync()
    g.untouched("n == 0")
    words, count = R.visible_pairs(ps, np.zeros((0, 3), F), targets=tt)
    assert words.shape == (0, 3) and count.shape == (0,)
    # a multi-device context is refused
    mc = R.Context(devices=[0, 0])
    ms = mc.rgbbox()
    mps = R.prepare_scene(8, 8, ms)
    assert call(mc._h, mps._h, N, pp, M, tp, 0, 0.0, 1.0, mp, cp) != 0
    assert "multi-device" in lib.rt_last_error(mc._h).decode()
    mc.sync()
    g.untouched("multi-device context")
    mps.free()
    ms.free()
    mc.close()


# ------------------------------------------------------------------------------------------------------------------------ 8. ordering
@pytest.mark.parametrize("mode", MODES)
def test_two_calls_in_flight(R, ctx, prepared, mode):
    # back to back on the context's stream, different targets into different buffers, one sync: rows of three words from 67 points are cut
    # into one-word runs, so each call zeroes its count and its waves add to it
    ps = prepared["rgbbox"]
    interval = (1e-3, 1.0) if mode == P.TARGETS else (0.1, 1e9)
    base = _want("rgbbox", mode, interval)
    tg = _targets("rgbbox", mode)
    pt, ta, tb = _device(_inputs("rgbbox")[0]), _device(tg), _device(tg[::-1])
    ga, gb = _Guarded(N, M), _Guarded(N, M)
    R.visible_pairs_into(pt.data_ptr(), N, ta.data_ptr(), M, ps, mode, ga.mask_ptr, ga.count_ptr, *interval)
    R.visible_pairs_into(pt.data_ptr(), N, tb.data_ptr(), M, ps, mode, gb.mask_ptr, gb.count_ptr, *interval)
    ctx.sync()
    for g, want, what in ((ga, base, "first call"), (gb, base[:, ::-1], "second call")):
        words, cnt = g.read(what)
        assert np.array_equal(words, P.pack(want)), what
        assert np.array_equal(cnt, want.sum(axis=1)), what
    # ... and the same buffer reused by a second call: the count is the second call's alone
    R.visible_pairs_into(pt.data_ptr(), N, tb.data_ptr(), M, ps, mode, ga.mask_ptr, ga.count_ptr, *interval)
    ctx.sync()
    words, cnt = ga.read("reused buffers")
    assert np.array_equal(words, P.pack(base[:, ::-1])) and np.array_equal(cnt, base.sum(axis=1))
