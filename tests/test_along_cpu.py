"""CPU checks of the along-ray queries: the restatement (along_ref.py) against the capped restatements it must agree with (sweep_ref.sweep:
identities 1 and 2; multi_hit_ref.multi_hit: identity 3) with rows above and below 32 entries both present, against its own brute force,
its per-sphere rule against the C++ arithmetic (build/along_check runs query_core.h's sweep_contact_roots), exclude and first, invalid
per-query values, the package's two row helpers against their per-row twins, wrong variants of the restatement (mutants) each caught by a
named input, and the loader's symbols and Python signatures.  No GPU needed."""
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import along_ref as A
import edge_sweeps as ES
import multi_hit_ref as M
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q
import sweep_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"rgbbox": ({}, 17), "irreg": ({}, 29), "floor": ({"n": 37, "k": 222.0}, 41)}
NRAYS = 512
F = np.float32
INTERVALS = ((0.0, 1e9), (0.1, 30.0), (7.0, 7.0))
KMAX = 32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _scene(name):
    kw, seed = SCENES[name]
    arr = O.OracleScene(name, **kw).arrays()
    return Q.RefScene(arr), X.seeded_rays(arr, NRAYS, seed), arr


def _radii(arr):
    r0 = float(np.median(arr["L"][:, 6]))
    return {"zero": 0.0, "neg_zero": -0.0, "median": r0, "four_medians": 4.0 * r0}


@functools.lru_cache(maxsize=None)
def _along(name, rname, interval):
    ref, rays, arr = _scene(name)
    return A.along(ref, rays[:, :3], rays[:, 3:], _radii(arr)[rname], interval[0], interval[1])


@functools.lru_cache(maxsize=None)
def _sweep(name, rname, interval):
    ref, rays, arr = _scene(name)
    return S.sweep(ref, rays[:, :3], rays[:, 3:], _radii(arr)[rname], interval[0], interval[1], KMAX)


def _rows_equal_sweep(rows, sweep, t_min, who):
    """identities 1 and 2 of a result against sweep_ref.sweep's (count, index, start, hit): every row's length, and the rows of at most 32
    entries in (tau, j) order; -> the number of non-empty rows compared"""
    off, idx, roots, start = rows
    cnt, sidx, sstart, shit = sweep
    assert np.array_equal(np.diff(off), cnt), f"{who}: row lengths differ from the sweep's count on {np.nonzero(np.diff(off) != cnt)[0][:5]}"
    got = A.row_contacts(off, idx, roots, start, t_min, KMAX)
    short = cnt <= KMAX
    for g, w, what in zip(got[1:], (sidx, sstart, shit[:, :, 0]), ("index", "start", "tau")):
        assert _same_bits(g[short], np.ascontiguousarray(w[short])), f"{who}: {what} differs from the sweep's on a row of at most 32 entries"
    # (the first 32 of a longer row are the sweep's too)
    for g, w in zip(got[1:], (sidx, sstart, shit[:, :, 0])):
        assert _same_bits(g, np.ascontiguousarray(w)), who
    return int((short & (cnt > 0)).sum())


@pytest.mark.parametrize("interval", INTERVALS, ids=str)
@pytest.mark.parametrize("rname", ["zero", "neg_zero", "median", "four_medians"])
@pytest.mark.parametrize("name", list(SCENES))
def test_identities_1_and_2_against_the_sweep(name, rname, interval):
    rows = _along(name, rname, interval)
    compared = _rows_equal_sweep(rows, _sweep(name, rname, interval), interval[0], (name, rname, interval))
    off, idx, roots, start = rows
    if interval[0] == interval[1]:
        assert off[-1] == 0
    else:
        assert compared > 0
    # rows ascend in j, strictly: a sphere is listed once
    row = np.repeat(np.arange(NRAYS), np.diff(off))
    inner = row[1:] == row[:-1]
    assert (np.diff(idx)[inner] > 0).all()
    # an entry contact lies inside the interval at t1; an overlap at the start has t1 <= t_min < t2
    lo, hi = F(interval[0]), F(interval[1])
    e, s = start == 0, start == 1
    assert (e | s).all()
    with np.errstate(invalid="ignore"):
        assert ((roots[e, 0] > lo) & (roots[e, 0] < hi)).all()
        assert (~(roots[s, 0] > lo) & (roots[s, 1] > lo)).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_coverage_short_and_long_rows(name):
    # a comparison restricted to rows of at most 32 entries could hide the long rows: at four medians over (0, 1e9) both kinds are common,
    # the short ones are compared with the sweep (above), the long ones with the brute force where the brute force has nothing extra
    ref, rays, arr = _scene(name)
    interval = INTERVALS[0]
    off, idx, roots, start = rows = _along(name, "four_medians", interval)
    n = np.diff(off)
    short, long_ = (n > 0) & (n <= KMAX), n > KMAX
    print(f"{name}: {short.mean():.1%} rows of 1..32 entries, {long_.mean():.1%} above 32, longest {n.max()}")
    assert short.mean() >= 0.25, short.mean()
    assert long_.mean() >= 0.25, long_.mean()
    brute = A.along_brute(ref, rays[:, :3], rays[:, 3:], _radii(arr)["four_medians"], *interval)
    nb = np.diff(brute[0])
    assert (nb >= n).all()
    no_extra = nb == n
    held = long_ & no_extra
    assert held.sum() >= 0.9 * long_.sum(), (held.sum(), long_.sum())
    for i in np.nonzero(held)[0]:
        a, b = slice(off[i], off[i + 1]), slice(brute[0][i], brute[0][i + 1])
        assert np.array_equal(idx[a], brute[1][b]) and _same_bits(roots[a], brute[2][b]) and np.array_equal(start[a], brute[3][b]), i


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_answer_equals_brute_force(name):
    # 3.5g: on these three scenes the tree drops no contact the brute force has
    ref, rays, arr = _scene(name)
    for rname, interval in (("zero", INTERVALS[0]), ("median", INTERVALS[1]), ("four_medians", INTERVALS[1])):
        tree = _along(name, rname, interval)
        brute = A.along_brute(ref, rays[:, :3], rays[:, 3:], _radii(arr)[rname], *interval)
        extra = int(brute[0][-1] - tree[0][-1])
        print(f"{name} {rname} {interval}: {tree[0][-1]} entries, the brute force has {extra} more")
        assert extra == 0, (name, rname, interval, extra)
        for g, w, part in zip(tree, brute, ("offsets", "index", "roots", "start")):
            assert g.dtype == w.dtype and _same_bits(g, w), (name, rname, interval, part)


@pytest.mark.parametrize("interval", INTERVALS, ids=str)
@pytest.mark.parametrize("name", list(SCENES))
def test_identity_3_against_multi_hit(name, interval):
    ref, rays, arr = _scene(name)
    o, d = rays[:, :3], rays[:, 3:]
    mc, mi, mr, mh = M.multi_hit(ref, o, d, interval[0], interval[1], KMAX)
    for rname in ("zero", "neg_zero"):
        off, idx, roots, start = _along(name, rname, interval)
        cnt, gi, gr, gt = A.row_crossings(off, idx, roots, interval[0], interval[1], KMAX)
        assert np.array_equal(cnt, mc)
        assert np.array_equal(gi, mi) and np.array_equal(gr, mr) and _same_bits(gt, np.ascontiguousarray(mh[:, :, 0]))
        if interval[0] < interval[1]:
            if name == "irreg" and interval == INTERVALS[0]:
                assert (mc > KMAX).any() and (np.diff(off) > KMAX).any()         # rays with more than 32 crossings, and contacts
            # the selected set is a superset of the crossed spheres: every crossed sphere is in the row ...
            for i in np.nonzero((mc > 0) & (mc <= KMAX))[0][:100]:
                assert set(mi[i, :mc[i]].tolist()) <= set(idx[off[i]:off[i + 1]].tolist()), i
    # ... and some selected sphere has no root inside the interval (a segment wholly inside it)
    if interval == (0.1, 30.0):
        off, idx, roots, start = _along(name, "zero", interval)
        with np.errstate(invalid="ignore"):
            none_inside = ~((roots > F(0.1)) & (roots < F(30.0))).any(axis=1)
        print(f"{name}: {int(none_inside.sum())} selected spheres hold the whole segment")
        assert (start[none_inside] == 1).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_helpers_equal_their_twins(name):
    import raytracers_amd as R
    rng = np.random.default_rng(5)
    lo = rng.choice(np.array([0.0, 0.1, 2.0], F), NRAYS)
    hi = rng.choice(np.array([30.0, 1e9], F), NRAYS)
    ref, rays, arr = _scene(name)
    for radius in (0.0, _radii(arr)["four_medians"]):
        off, idx, roots, start = A.along(ref, rays[:, :3], rays[:, 3:], radius, lo, hi)
        for k in (1, 5, KMAX):
            for g, w in zip(R.row_contacts(off, idx, roots, start, lo, k), A.row_contacts(off, idx, roots, start, lo, k)):
                assert g.dtype == w.dtype and _same_bits(g, w), k
            for g, w in zip(R.row_crossings(off, idx, roots, lo, hi, k), A.row_crossings(off, idx, roots, lo, hi, k)):
                assert g.dtype == w.dtype and _same_bits(g, w), k
    # scalar bounds, and an empty answer
    off, idx, roots, start = _along(name, "median", INTERVALS[1])
    for g, w in zip(R.row_contacts(off, idx, roots, start, 0.1, 4), A.row_contacts(off, idx, roots, start, 0.1, 4)):
        assert _same_bits(g, w)
    empty = (np.zeros(NRAYS + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), F), np.zeros(0, np.uint8))
    c, i, s, t = R.row_contacts(*empty, 0.0, 3)
    assert not c.any() and (i == -1).all() and not s.any() and not t.any() and i.shape == (NRAYS, 3)
    c, i, r, t = R.row_crossings(empty[0], empty[1], empty[2], 0.0, 1e9, 3)
    assert not c.any() and (i == -1).all() and not r.any() and not t.any()


@pytest.mark.parametrize("name", list(SCENES))
def test_exclude_and_first(name):
    ref, rays, arr = _scene(name)
    o, d = rays[:, :3], rays[:, 3:]
    r0 = _radii(arr)["median"]
    off, idx, roots, start = _along(name, "median", INTERVALS[0])
    n = np.diff(off)
    rng = np.random.default_rng(11)
    pick = off[:-1] + (rng.random(NRAYS) * np.maximum(n, 1)).astype(np.int64)
    member = np.where(n > 0, idx[np.minimum(pick, max(idx.size - 1, 0))], 3).astype(np.int64)
    row = np.repeat(np.arange(NRAYS), n)
    # exclude: exactly that sphere's entry is gone; out-of-range values on both sides exclude nothing
    ex = member.copy()
    ex[::7] = -1
    ex[1::7] = ref.n
    ex[2::7] = -2 ** 31
    ex[3::7] = 2 ** 31 - 1
    got = A.along(ref, o, d, r0, *INTERVALS[0], exclude=ex)
    keep = idx != ex[row]
    assert (~keep).sum() > NRAYS // 4
    assert np.array_equal(np.diff(got[0]), np.bincount(row[keep], minlength=NRAYS))
    assert np.array_equal(got[1], idx[keep]) and _same_bits(got[2], roots[keep]) and np.array_equal(got[3], start[keep])
    _rows_equal_sweep(got, S.sweep(ref, o, d, r0, *INTERVALS[0], KMAX, exclude=ex), 0.0, "exclude")
    # first: the entries with j >= first; <= 0 selects everything, >= the sphere count nothing
    fi = member.copy()
    fi[::7] = -5
    fi[1::7] = ref.n
    fi[2::7] = 0
    fi[3::7] = ref.n + 9
    fi[4::7] = member[4::7] + 1
    got = A.along(ref, o, d, r0, *INTERVALS[0], first=fi)
    keep = idx >= fi[row]
    assert 0 < keep.sum() < keep.size
    assert np.array_equal(np.diff(got[0]), np.bincount(row[keep], minlength=NRAYS))
    assert np.array_equal(got[1], idx[keep]) and _same_bits(got[2], roots[keep]) and np.array_equal(got[3], start[keep])
    assert not np.diff(got[0])[1::7].any() and not np.diff(got[0])[3::7].any()
    assert np.array_equal(np.diff(got[0])[::7], n[::7]) and np.array_equal(np.diff(got[0])[2::7], n[2::7])
    # both at once
    got = A.along(ref, o, d, r0, *INTERVALS[0], exclude=ex, first=fi)
    keep = (idx >= fi[row]) & (idx != ex[row])
    assert np.array_equal(got[1], idx[keep]) and np.array_equal(np.diff(got[0]), np.bincount(row[keep], minlength=NRAYS))


@pytest.mark.parametrize("name", list(SCENES))
def test_walk_equals_dense(name):
    ref, rays, arr = _scene(name)
    o, d = rays[:, :3], rays[:, 3:]
    rng = np.random.default_rng(3)
    ex, fi = rng.integers(-2, ref.n + 2, NRAYS), rng.integers(-2, ref.n + 2, NRAYS)
    lo, hi, rq, _ = invalid_values(NRAYS, _radii(arr)["four_medians"])
    for args in ((0.0, 0.0, 1e9), (_radii(arr)["median"], 0.1, 30.0), (rq, lo, hi)):
        for kw in ({}, {"exclude": ex}, {"first": fi}, {"exclude": ex, "first": fi}):
            for g, w in zip(A.along_walk(arr, o, d, *args, **kw), A.along(ref, o, d, *args, **kw)):
                assert g.dtype == w.dtype and _same_bits(g, w), kw


def invalid_values(n, r0):
    """(t_min, t_max, radius [n] float32, bad [n] bool): valid values with NaN, inf, negative, reversed and 2e9 entries planted, and -0.0"""
    lo, hi, rq = np.full(n, 0.0, F), np.full(n, 1e9, F), np.full(n, r0, F)
    bad = [(np.nan, 1.0, r0), (0.0, np.nan, r0), (0.0, np.inf, r0), (-1.0, 1.0, r0), (2.0, 1.0, r0), (0.0, 2e9, r0),
           (0.0, 1e9, np.nan), (0.0, 1e9, np.inf), (0.0, 1e9, -1.0), (0.0, 1e9, 2e9), (0.0, 1e9, -np.inf)]
    where = np.arange(len(bad)) * 37 + 3
    for i, (a, b, c) in zip(where, bad):
        lo[i], hi[i], rq[i] = a, b, c
    lo[1::37] = -0.0
    rq[2::37] = -0.0
    mask = np.zeros(n, bool)
    mask[where] = True
    return lo, hi, rq, mask


@pytest.mark.parametrize("name", list(SCENES))
def test_invalid_per_query_values_give_empty_rows(name):
    ref, rays, arr = _scene(name)
    o, d = rays[:, :3], rays[:, 3:]
    r0 = _radii(arr)["median"]
    lo, hi, rq, bad = invalid_values(NRAYS, r0)
    assert np.array_equal(S.query_ok(lo, hi, rq), ~bad)
    got = A.along(ref, o, d, rq, lo, hi)
    n = np.diff(got[0])
    full = np.diff(_along(name, "median", INTERVALS[0])[0])
    assert full[bad].any() and not n[bad].any()
    # every other row is the scalar form's, -0.0 behaving as +0.0: bucket by bucket
    zero_r = _bits(rq) == 0x80000000
    for m, radius in ((~bad & ~zero_r, r0), (~bad & zero_r, 0.0)):
        want = A.along(ref, o[m], d[m], radius, 0.0, 1e9)
        assert np.array_equal(n[m], np.diff(want[0]))
        row = np.repeat(np.arange(NRAYS), n)
        sel = m[row]
        assert np.array_equal(got[1][sel], want[1]) and _same_bits(got[2][sel], want[2]) and np.array_equal(got[3][sel], want[3])
    _rows_equal_sweep(got, S.sweep(ref, o, d, rq, lo, hi, KMAX), lo, "per-query")


# ------------------------------------------------------------------------------------------------------------- C++ arithmetic
def _run_check(exe_name, cases, tmp_path, words):
    exe = os.path.join(ROOT, "build", exe_name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/" + exe_name], check=True, capture_output=True)
    src, dst = tmp_path / (exe_name + "_cases.bin"), tmp_path / (exe_name + "_out.bin")
    cases.tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(dst, dtype=np.uint32).reshape(-1, words)
    assert out.shape[0] == cases.shape[0]
    return out


def _scene_cases(name, m=3000):
    """(m, 13) cases from a scene: its seeded rays paired with random spheres of it, radii and intervals of the tests above"""
    ref, rays, arr = _scene(name)
    rng = np.random.default_rng(23)
    i, j = rng.integers(0, NRAYS, m), rng.integers(0, ref.n, m)
    r0 = _radii(arr)["median"]
    rq = rng.choice(np.array([0.0, -0.0, r0, 4 * r0], F), m)
    iv = np.asarray(INTERVALS, F)[rng.integers(0, 3, m)]
    return np.concatenate([rays[i], ref.pos[j], ref.rad[j, None], rq[:, None], iv], axis=1).astype(F)


def test_along_check_agrees_with_the_restatement(tmp_path):
    from test_sweep_cpu import rule_case_set
    cases = np.concatenate([rule_case_set()] + [_scene_cases(name) for name in SCENES]).astype(F)
    got = _run_check("along_check", cases, tmp_path, 5)
    args = (cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9], cases[:, 10], cases[:, 11], cases[:, 12])
    kind, tau, good, t1, t2 = A.rule_cases(*args)
    nan1, nan2 = np.isnan(t1), np.isnan(t2)
    g1, g2 = got[:, 3].view(F), got[:, 4].view(F)
    bad = np.nonzero((got[:, 0] != kind) | (got[:, 1] != _bits(tau)) | (got[:, 2] != good)
                     | np.where(nan1, ~np.isnan(g1), got[:, 3] != _bits(t1)) | np.where(nan2, ~np.isnan(g2), got[:, 4] != _bits(t2)))[0]
    assert bad.size == 0, f"{bad.size} cases differ, first {bad[:5]}: {cases[bad[:3]]}"
    assert all((kind == v).sum() > 100 for v in (0, 1, 2)), np.bincount(kind)
    assert (nan1 & good).sum() > 0 and (good & (kind == 0)).sum() > 100          # NaN roots, and roots written for no contact
    # kind and tau are sweep_contact's: against sweep_ref's rule and against build/sweep_check on the same file
    skind, stau = S.rule_cases(*args)
    assert np.array_equal(got[:, 0], skind) and np.array_equal(got[:, 1], _bits(stau))
    old = _run_check("sweep_check", cases, tmp_path, 2)
    assert np.array_equal(old, got[:, :2])


# ------------------------------------------------------------------------------------------------------------- mutants
@functools.lru_cache(maxsize=None)
def _edge_scene(name):
    s, lf, la, fov = ES.SCENES[name]
    arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    return arr, ref, ES.sweep_families(arr, seed=1)


def _edge_filters(ref, q):
    """(exclude, first) for a family's queries: the lowest selected sphere of every other row excluded; first = the median of the row"""
    rays, rq, lo, hi = q
    off, idx, _, _ = A.along(ref, rays[:, :3], rays[:, 3:], rq, lo, hi)
    m = rays.shape[0]
    n = np.diff(off)
    ex = np.where(n > 0, idx[np.minimum(off[:-1], max(idx.size - 1, 0))], -1).astype(np.int64)
    ex[1::2] = -1
    fi = np.where(n > 0, idx[np.minimum(off[:-1] + n // 2, max(idx.size - 1, 0))], 0).astype(np.int64)
    assert m == n.size
    return ex, fi


def _failed_checks(ref, q, mutant):
    """the names of the checks a (possibly wrong) restatement fails on the queries q: the checks of the tests above, against sweep_ref.sweep,
    sweep_ref.swept_roots and the restatement's own unfiltered rows"""
    rays, rq, lo, hi = q
    o, d = rays[:, :3], rays[:, 3:]
    ex, fi = _edge_filters(ref, q)
    tau_mutant = mutant if mutant == "tau_t1_at_start" else None
    row_mutant = None if mutant == "tau_t1_at_start" else mutant
    failed = set()
    for exclude in (None, ex):
        off, idx, roots, start = A.along(ref, o, d, rq, lo, hi, exclude=exclude, mutant=row_mutant)
        cnt, sidx, sstart, shit = S.sweep(ref, o, d, rq, lo, hi, KMAX, exclude=exclude)
        if not np.array_equal(np.diff(off), cnt):
            failed.add("identity 1")
        else:
            got = A.row_contacts(off, idx, roots, start, lo, KMAX, mutant=tau_mutant)
            if not all(_same_bits(g, np.ascontiguousarray(w)) for g, w in zip(got[1:], (sidx, sstart, shit[:, :, 0]))):
                failed.add("identity 2")
        row = np.repeat(np.arange(rays.shape[0]), np.diff(off))
        if not (np.diff(idx)[row[1:] == row[:-1]] > 0).all():
            failed.add("ascending j")
        t1, t2, _, _ = S.swept_roots(o[row, 0], o[row, 1], o[row, 2], d[row, 0], d[row, 1], d[row, 2], ref.pos[idx, 0], ref.pos[idx, 1],
                                     ref.pos[idx, 2], ref.rad[idx], S._radii(rq.size, rq)[row])
        both_nan = np.isnan(roots) & np.isnan(np.stack([t1, t2], axis=1))
        if not ((_bits(roots) == _bits(np.stack([t1, t2], axis=1).astype(F))) | both_nan).all():
            failed.add("roots")
    off, idx, roots, start = A.along(ref, o, d, rq, lo, hi, mutant=row_mutant)
    row = np.repeat(np.arange(rays.shape[0]), np.diff(off))
    got = A.along(ref, o, d, rq, lo, hi, first=fi, mutant=row_mutant)
    keep = idx >= fi[row]
    if not (np.array_equal(got[1], idx[keep]) and np.array_equal(np.diff(got[0]), np.bincount(row[keep], minlength=rays.shape[0]))):
        failed.add("first")
    return failed


MUTANT_INPUTS = {
    "multi_hit_set": ("random600", "absorbed", "identity 1"),
    "boxes_not_widened": ("random600", "ties", "identity 1"),
    "exclude_ignored": ("overlap", "ties", "identity 1"),
    "first_off_by_one": ("random600", "ties", "first"),
    "tau_order": ("random600", "ties", "ascending j"),
    "roots_of_r": ("overlap", "ties", "roots"),
    "tau_t1_at_start": ("random600", "ties", "identity 2"),
}


def test_the_restatement_passes_on_the_mutants_inputs():
    for scene, family in sorted({(s, f) for s, f, _ in MUTANT_INPUTS.values()}):
        arr, ref, fam = _edge_scene(scene)
        assert _failed_checks(ref, fam[family], None) == set(), (scene, family)


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutants_are_caught(mutant):
    assert set(MUTANT_INPUTS) == set(A.MUTANTS)
    scene, family, check = MUTANT_INPUTS[mutant]
    arr, ref, fam = _edge_scene(scene)
    failed = _failed_checks(ref, fam[family], mutant)
    print(f"{mutant}: {scene}/{family} fails {sorted(failed)}")
    assert check in failed, (mutant, failed)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_library_exports_along():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_spheres_along_rays_count", "rt_spheres_along_rays_fill"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_spheres_along_rays_count.argtypes) == 13
    assert len(_lib.lib.rt_spheres_along_rays_fill.argtypes) == 18
    for name in ("spheres_along_rays", "spheres_along_rays_count_into", "spheres_along_rays_fill_into", "row_contacts", "row_crossings"):
        assert callable(getattr(R, name)), name
    sig = inspect.signature(R.spheres_along_rays)
    assert list(sig.parameters) == ["prepared", "rays", "radius", "t_min", "t_max", "exclude", "first", "roots", "rows"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:]] == [0.0, 0.0, 1e9, None, None, True, False]
    assert list(inspect.signature(R.spheres_along_rays_count_into).parameters) == [
        "rays_ptr", "n", "prepared", "offsets_ptr", "radius", "t_min", "t_max", "radius_ptr", "t_min_ptr", "t_max_ptr", "exclude_ptr", "first_ptr"]
    assert list(inspect.signature(R.spheres_along_rays_fill_into).parameters) == [
        "rays_ptr", "n", "prepared", "offsets_ptr", "capacity", "index_ptr", "roots_ptr", "start_ptr", "query_ptr", "radius", "t_min", "t_max",
        "radius_ptr", "t_min_ptr", "t_max_ptr", "exclude_ptr", "first_ptr"]
    assert list(inspect.signature(R.row_contacts).parameters) == ["offsets", "index", "roots", "start", "t_min", "k"]
    assert list(inspect.signature(R.row_crossings).parameters) == ["offsets", "index", "roots", "t_min", "t_max", "k"]


def test_header_declares_along():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_spheres_along_rays_count(", "rt_spheres_along_rays_fill(", "family=along count", "IDENTITIES"):
        assert sym in h, sym
    core = open(os.path.join(ROOT, "raytracers_amd", "csrc", "query_core.h")).read()
    assert "RT_HD int sweep_contact_roots(" in core and "RT_HD int sweep_contact(" in core
