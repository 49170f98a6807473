"""CPU checks of the sphere casts on the edge inputs of edge_sweeps.py: every family provably sits on its edge, the restatement's dense form
equals its walk form there, query_core.h's sweep_contact (build/sweep_check) equals the restatement's per-sphere rule on every query paired
with its target sphere, the tree-defined answer differs from the brute force only on unconsulted leaves, wrong variants of the restatement
(mutants) are told apart by the inputs, and the defined answer is the geometric one: a float64 brute force of the contact rule agrees with
it outside a thin band around the rule's boundaries.  No GPU needed."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_rays as E
import edge_sweeps as ES
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q
import sweep_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
SCENES = tuple(ES.SCENES)
same_bits = E.same_bits


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


@functools.lru_cache(maxsize=None)
def _scene(name):
    s, lf, la, fov = ES.SCENES[name]
    arr = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).arrays()
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    fam = ES.sweep_families(arr, seed=1)
    tgt = ES.sweep_targets(arr, seed=1)
    return arr, ref, fam, tgt


@functools.lru_cache(maxsize=None)
def _answer(name, k=S.KMAX):
    arr, ref, fam, _ = _scene(name)
    rays, rq, lo, hi, label = ES.joined(fam)
    return S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, k)


def _target_roots(arr, q, j):
    """(t1, t2, disc > 0, kind, tau) of every query of the family against its own target sphere"""
    L = np.asarray(arr["L"], dtype=F)
    rays, rq, lo, hi = q
    o, d, c, r = rays[:, :3], rays[:, 3:], L[j, :3], L[j, 6]
    t1, t2, good, _ = S.swept_roots(o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], c[:, 0], c[:, 1], c[:, 2], r, S._radii(rq.size, rq))
    kind, tau = S.rule_cases(o, d, c, r, S._radii(rq.size, rq), lo, hi)
    return t1, t2, good, kind, tau


def _eq(a, b):
    return _bits(np.asarray(a, F)) == _bits(np.asarray(b, F))


@pytest.mark.parametrize("name", SCENES)
def test_families_hit_their_edge(name):
    arr, ref, fam, tgt = _scene(name)
    L = np.asarray(arr["L"], dtype=F)
    n = L.shape[0]
    assert all(v[0].shape[0] > 0 and all(a.dtype == F for a in v) for v in fam.values()), name
    want = {"ray_edges", "entry_at_t_min", "entry_just_past_t_min", "exit_at_t_min", "entry_at_t_max", "stationary", "ties", "widened_face",
            "absorbed"}
    if name in ES.INTEGER_SCENES:
        want.add("grazing")
    if name == "random600_r0":
        want.add("zero_radius")
    assert set(fam) == want, (name, sorted(fam))
    assert sum(v[0].shape[0] for v in fam.values()) < 2500, name
    rays_all, rq_all, lo_all, hi_all, label = ES.joined(fam)
    count, index, start, hit = _answer(name)
    names = list(fam)

    def of(f):
        return label == names.index(f)

    # ray_edges: the seven radii exactly, each next to edge intervals
    rq = fam["ray_edges"][1]
    r0 = ES.median_radius(arr)
    for v in (F(0.0), E.NEG0, F(1e-40), r0, F(40.0), F(1e8), F(1e9)):
        assert _eq(rq, v).sum() > 100, (name, v)
    # a root equal to a bound, bit for bit, and what the rule makes of it
    t1, t2, good, kind, tau = _target_roots(arr, fam["entry_at_t_min"], tgt["entry_at_t_min"])
    at = good & _eq(t1, fam["entry_at_t_min"][2])
    assert at.sum() >= 20 and (kind[at] == 2).all() and _eq(tau[at], fam["entry_at_t_min"][2][at]).all(), (name, at.sum())
    assert sum((at & _eq(fam["entry_at_t_min"][2], t)).sum() for t in ES.T_MINS) > 0, name        # found by search too, not only own roots
    t1, t2, good, kind, tau = _target_roots(arr, fam["entry_just_past_t_min"], tgt["entry_just_past_t_min"])
    lo = fam["entry_just_past_t_min"][2]
    at = good & _eq(t1, np.nextafter(lo, INF, dtype=F))
    assert at.sum() >= 20 and (kind[at] == 1).all() and _eq(tau[at], t1[at]).all(), (name, at.sum())
    t1, t2, good, kind, tau = _target_roots(arr, fam["exit_at_t_min"], tgt["exit_at_t_min"])
    at = good & _eq(t2, fam["exit_at_t_min"][2])
    assert at.sum() >= 20 and (kind[at] == 0).all(), (name, at.sum())
    t1, t2, good, kind, tau = _target_roots(arr, fam["entry_at_t_max"], tgt["entry_at_t_max"])
    hi = fam["entry_at_t_max"][3]
    at, below = good & _eq(t1, hi), good & _eq(np.nextafter(t1, INF, dtype=F), hi)
    assert at.sum() >= 20 and (kind[at] == 0).all(), (name, at.sum())
    assert below.sum() >= 20 and (kind[below] == 1).all(), (name, below.sum())
    # grazing: the discriminant of the inflated sphere is exactly zero on the tangent third, and that is no contact
    if "grazing" in fam:
        rays, rq, lo, hi = fam["grazing"]
        j = tgt["grazing"]
        R = (L[j, 6] + rq).astype(F)
        oc = rays[:, :3] - L[j, :3]
        a = Q.dot(rays[:, 3], rays[:, 4], rays[:, 5], rays[:, 3], rays[:, 4], rays[:, 5])
        b = Q.dot(oc[:, 0], oc[:, 1], oc[:, 2], rays[:, 3], rays[:, 4], rays[:, 5])
        c = Q.dot(oc[:, 0], oc[:, 1], oc[:, 2], oc[:, 0], oc[:, 1], oc[:, 2]) - R * R
        disc = b * b - a * c
        third = rays.shape[0] // 3
        assert (disc[:third] == 0).all() and not (rays[:third] == rays[third:2 * third]).all(), name
        kind = _target_roots(arr, fam["grazing"], j)[3]
        assert (kind[:third] == 0).all(), name
    # stationary queries have no contact at all, wherever they rest
    rays = fam["stationary"][0]
    assert (rays[:, 3:] == 0).all() and np.signbit(rays[:, 3:]).any() and not np.signbit(rays[:, 3:]).all(), name
    assert not count[of("stationary")].any(), name
    inside = S.contact_kinds(ref, rays[:, :3], rays[:, 3:] + F(1), fam["stationary"][1], fam["stationary"][2], fam["stationary"][3], boxes=False)
    assert (inside == 2).any(), name          # (the same origins DO overlap spheres at the start once they move)
    # ties: equal tau in neighbouring slots, lists that overflow, an entry one ulp behind a block of overlaps
    m = of("ties")
    tau_t, idx_t, st_t, cnt_t = hit[m][:, :, 0], index[m], start[m], count[m]
    tie = (tau_t[:, 1:] == tau_t[:, :-1]) & (idx_t[:, 1:] >= 0)
    assert (tie & (st_t[:, 1:] == 0)).any(), f"{name}: no two entry contacts at one tau"
    assert (tie & (st_t[:, 1:] == 1)).any(), f"{name}: no two overlaps at the start"
    if n > S.KMAX:
        assert (cnt_t > S.KMAX).any(), name
    if name not in ("two_same", "same64"):      # (every sphere of these coincides with every other: no entry behind an overlap)
        lo_t = fam["ties"][2]
        behind = (st_t[:, :-1] == 1) & (st_t[:, 1:] == 0) & (idx_t[:, 1:] >= 0) & _eq(tau_t[:, 1:], np.nextafter(lo_t, INF, dtype=F)[:, None])
        assert behind.any(), f"{name}: no entry at nextafter(t_min) behind the overlaps at t_min"
    # widened_face: the origin is on a widened face of some inner node, with a zero direction component on that axis
    rays, rq, lo, hi = fam["widened_face"]
    bmin, bmax = np.asarray(arr["bmin"], dtype=F), np.asarray(arr["bmax"], dtype=F)
    wlo = (bmin[None, :, :] - rq[:, None, None]).astype(F)
    whi = (bmax[None, :, :] + rq[:, None, None]).astype(F)
    on = ((rays[:, None, :3] == wlo) | (rays[:, None, :3] == whi)) & (rays[:, None, 3:] == 0)
    assert on.any(axis=(1, 2)).all(), name
    assert np.signbit(rays[:, 3:][rays[:, 3:] == 0]).any(), name
    # absorbed: every leaf is consulted, and the count reaches the scene's sphere count
    rays, rq, lo, hi = fam["absorbed"]
    assert S.consulted(ref, rays[:, :3], rays[:, 3:], rq, lo, hi).all(), name
    assert count[of("absorbed")].max() == n, name
    # zero_radius: contacts with R == 0, whose normals are not finite
    if "zero_radius" in fam:
        m = of("zero_radius")
        j = tgt["zero_radius"]
        R0 = (L[j, 6] + S._radii(j.size, fam["zero_radius"][1])) == 0
        mine = (index[m] == j[:, None]) & R0[:, None]
        assert mine.sum() > 10 and not np.isfinite(hit[m][mine][:, 4:]).all(axis=1).any(), (name, mine.sum())
        assert (~R0).any() and ((index[m] == j[:, None]) & ~R0[:, None]).any(), name       # and with a denormal R


def test_inputs_reach_long_lists_and_ties():
    # what the issue measured: 31 equal-tau neighbours in a 32-slot list, and counts past the scenes' sphere counts' reach
    for name, floor in (("same64", 64), ("tall1100", 1114), ("overlap", 48)):
        count, index, start, hit = _answer(name)
        tau = hit[:, :, 0]
        tie = ((tau[:, 1:] == tau[:, :-1]) & (index[:, 1:] >= 0)).sum(axis=1)
        assert tie.max() == S.KMAX - 1 and count.max() >= floor, (name, tie.max(), count.max())


@pytest.mark.parametrize("name", SCENES)
def test_dense_equals_walk(name):
    arr, ref, fam, _ = _scene(name)
    rays, rq, lo, hi, label = ES.joined(fam)
    o, d = rays[:, :3], rays[:, 3:]
    ex = np.random.default_rng(3).integers(-2, ref.n + 2, rays.shape[0])
    for k, exclude in ((S.KMAX, None), (5, None), (8, ex)):
        want = _answer(name, k) if exclude is None else S.sweep(ref, o, d, rq, lo, hi, k, exclude)
        got = S.sweep_walk(arr, o, d, rq, lo, hi, k, exclude)
        for part, g, w in zip(("count", "index", "start", "hit7"), got, want):
            try:
                same_bits(g, w, f"{name} k={k} {part}")
            except AssertionError:
                for i, f in enumerate(fam):
                    same_bits(g[label == i], w[label == i], f"{name}/{f} k={k} {part}")
                raise


def edge_rule_cases():
    """[m, 13] float32 cases for build/sweep_check: every edge query of every scene paired with its target sphere (a random one where it has
    none) and with three random spheres; and `family` [m], the query's family"""
    rows, fams = [], []
    rng = np.random.default_rng(20261018)
    for name in SCENES:
        arr, ref, fam, tgt = _scene(name)
        L = np.asarray(arr["L"], dtype=F)
        for f, (rays, rq, lo, hi) in fam.items():
            m = rays.shape[0]
            j = np.where(tgt[f] >= 0, tgt[f], rng.integers(0, L.shape[0], m))
            for jj in (j, rng.integers(0, L.shape[0], m), rng.integers(0, L.shape[0], m), rng.integers(0, L.shape[0], m)):
                rows.append(np.concatenate([rays, L[jj, :3], L[jj, 6:7], rq[:, None], lo[:, None], hi[:, None]], axis=1).astype(F))
                fams += [f] * m
    return np.concatenate(rows), np.array(fams)


def test_sweep_check_agrees_on_the_edge_cases(tmp_path):
    exe = os.path.join(ROOT, "build", "sweep_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/sweep_check"], check=True, capture_output=True)
    cases, fams = edge_rule_cases()
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, dtype=np.uint32).reshape(-1, 2)
    assert got.shape[0] == cases.shape[0]
    kind, tau = S.rule_cases(cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9], cases[:, 10], cases[:, 11], cases[:, 12])
    bad = np.nonzero((got[:, 0] != kind) | (got[:, 1] != _bits(tau)))[0]
    assert bad.size == 0, f"{bad.size} cases differ, families {sorted(set(fams[bad]))}, first {bad[:5]}: {cases[bad[:3]]}"
    # the boundary cases are in the set: t1 == t_min exactly is an overlap at the start, and there are hundreds of them
    o, d, c = cases[:, 0:3], cases[:, 3:6], cases[:, 6:9]
    t1, t2, good, _ = S.swept_roots(o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], c[:, 0], c[:, 1], c[:, 2], cases[:, 9], cases[:, 10])
    at = good & _eq(t1, cases[:, 11]) & (fams == "entry_at_t_min")
    assert at.sum() >= 20 * len(SCENES) and (got[at, 0] == 2).all(), at.sum()
    print(f"{cases.shape[0]} cases, {int(at.sum())} with t1 == t_min bit for bit: {r.stdout.strip()}")


@pytest.mark.parametrize("name", SCENES)
def test_tree_answer_against_brute_force_on_the_edge_scenes(name):
    arr, ref, fam, _ = _scene(name)
    rays, rq, lo, hi, label = ES.joined(fam)
    o, d = rays[:, :3], rays[:, 3:]
    tree = S.contact_kinds(ref, o, d, rq, lo, hi)
    brute = S.contact_kinds(ref, o, d, rq, lo, hi, boxes=False)
    seen = S.consulted(ref, o, d, rq, lo, hi)
    diff = tree != brute
    print(f"{name}: {int(diff.sum())} of {int((brute > 0).sum())} brute-force contacts are not in the tree's answer "
          f"({diff.any(axis=1).mean():.3%} of the queries; by family "
          f"{ {f: int(diff[label == i].sum()) for i, f in enumerate(fam) if diff[label == i].any()} })")
    assert not (tree[diff] != 0).any(), "the tree's answer has a contact the brute force has not"
    assert not seen[diff].any(), "a differing contact is on a consulted leaf"
    assert np.array_equal(tree[seen], brute[seen])
    same = ~diff.any(axis=1)
    a = S.sweep(ref, o[same], d[same], rq[same], lo[same], hi[same], 8)
    b = S.sweep_brute(ref, o[same], d[same], rq[same], lo[same], hi[same], 8)
    for part, g, w in zip(("count", "index", "start", "hit7"), a, b):
        same_bits(g, w, f"{name} {part}")


# ------------------------------------------------------------------------------------------------------------------ mutants
def _m_contact_rule(t1_ge_lo=False, t1_le_hi=False, t2_ge_lo=False, no_plus_zero=False):
    def rule(t1, t2, good, lo, hi):
        with np.errstate(invalid="ignore"):
            past = (t1 >= lo) if t1_ge_lo else (t1 > lo)
            entry = good & past & ((t1 <= hi) if t1_le_hi else (t1 < hi))
            start = good & ~past & ((t2 >= lo) if t2_ge_lo else (t2 > lo)) & (lo < hi)
            at = (lo + F(0)) if not no_plus_zero else lo * np.ones_like(t1)
            tau = np.where(entry, t1, np.where(start, at, F(0))).astype(F)
        return np.where(entry, 1, np.where(start, 2, 0)).astype(np.uint8), tau
    return rule


def _m_swept_roots(ox, oy, oz, dx, dy, dz, px, py, pz, rad, rq):
    t1, t2, good, R = _TRUE["swept_roots"](ox, oy, oz, dx, dy, dz, px, py, pz, rad, rq)
    with np.errstate(all="ignore"):
        ocx, ocy, ocz = ox - px, oy - py, oz - pz
        disc = Q.dot(ocx, ocy, ocz, dx, dy, dz) ** 2 - Q.dot(dx, dy, dz, dx, dy, dz) * (Q.dot(ocx, ocy, ocz, ocx, ocy, ocz) - R * R)
    return t1, t2, ~(disc < 0), R                                        # disc < 0 in place of disc <= 0


def _m_radii(n, radius):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=F), (n,))).astype(F)      # without + 0.0


def _m_box(mode):
    def box(ox, oy, oz, dx, dy, dz, bmin, bmax, rq, lo, hi):
        if mode == "bmin_only":
            return _TRUE["box_pass"](ox, oy, oz, dx, dy, dz, [b - rq for b in bmin], bmax, F(0), lo, hi)
        return _TRUE["box_pass"](ox, oy, oz, dx, dy, dz, bmin, bmax, np.roll(rq, 1, axis=0), lo, hi)    # the neighbouring query's rq
    return box


_TRUE = {k: getattr(S, k) for k in ("swept_roots", "contact_rule", "_radii", "box_pass")}


def _reordered(full, k, key):
    """the answer with every query's contacts re-sorted by `key(tau, j, start)` (a lexsort tuple, last key first) and cut to k slots"""
    count, index, start, hit = full
    have = index >= 0
    keys = key(np.where(have, hit[:, :, 0], INF), np.where(have, index, 1 << 30), start)
    order = np.lexsort(keys, axis=1)[:, :k]
    rows = np.arange(index.shape[0])[:, None]
    return count, index[rows, order], start[rows, order], hit[rows, order]


# (mutant, the family that must tell it from the true restatement, how to install it)
MUTANTS = (
    ("t1 >= lo", "entry_at_t_min", {"contact_rule": _m_contact_rule(t1_ge_lo=True)}),
    ("t1 <= hi", "entry_at_t_max", {"contact_rule": _m_contact_rule(t1_le_hi=True)}),
    ("t2 >= lo", "exit_at_t_min", {"contact_rule": _m_contact_rule(t2_ge_lo=True)}),
    ("disc < 0", "grazing", {"swept_roots": _m_swept_roots}),
    ("tau without + 0.0", "ties", {"contact_rule": _m_contact_rule(no_plus_zero=True)}),
    ("rq without + 0.0", "zero_radius", {"_radii": _m_radii}),
    ("box widened on bmin only", "absorbed", {"box_pass": _m_box("bmin_only")}),
    ("box widened with the neighbouring query's rq", "ray_edges", {"box_pass": _m_box("neighbour")}),
)
MUTANT_SCENES = ("same64", "nan_grid", "overlap", "random600_r0")


def _differs(got, want, label, fam):
    """the families on which the two answers differ (NaN == NaN)"""
    out = []
    for i, f in enumerate(fam):
        m = label == i
        for g, w in zip(got, want):
            g, w = g[m], w[m]
            if g.dtype == F:
                bad = (np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & (_bits(g) != _bits(w)))
            else:
                bad = g != w
            if bad.any():
                out.append(f)
                break
    return out


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_caught(mutant, monkeypatch):
    what, family, patch = mutant
    caught = {}
    for name in MUTANT_SCENES:
        arr, ref, fam, _ = _scene(name)
        rays, rq, lo, hi, label = ES.joined(fam)
        want = _answer(name)
        with monkeypatch.context() as mp:
            for k, v in patch.items():
                mp.setattr(S, k, v)
            got = S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, S.KMAX)
        caught[name] = _differs(got, want, label, fam)
    print(f"mutant '{what}': caught by {caught}")
    assert any(family in v for v in caught.values()), f"mutant '{what}' is not told apart by {family}: {caught}"
    # and the true restatement, re-installed, is itself again
    arr, ref, fam, _ = _scene("overlap")
    rays, rq, lo, hi, label = ES.joined(fam)
    assert not _differs(S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, S.KMAX), _answer("overlap"), label, fam)


def test_order_mutants_are_caught():
    # the list order: (tau, j) against (tau, -j), and the start flag in the key.  With the flag between tau and j -- (tau, start, j) -- the
    # order CANNOT change: an overlap's tau is t_min (+0.0 for -0.0) and an entry's is t1 > t_min, so two contacts of one query with equal
    # tau have equal flags.  That variant is held equal here, as a proof by enumeration on the tie inputs; the flag above tau -- (start,
    # tau, j), entries before overlaps -- is the one that can be, and must be, told apart.
    caught = {"(tau, -j)": set(), "(start, tau, j)": set()}
    for name in ("same64", "nan_grid", "overlap"):
        arr, ref, fam, _ = _scene(name)
        rays, rq, lo, hi, label = ES.joined(fam)
        full = S.sweep(ref, rays[:, :3], rays[:, 3:], rq, lo, hi, ref.n)
        assert full[0].max() <= ref.n
        for k in (1, 5, S.KMAX):
            want = tuple(a if i == 0 else a[:, :k] for i, a in enumerate(_answer(name)))
            assert not _differs(_reordered(full, k, lambda t, j, s: (j, t)), want, label, fam), name           # the true order, re-derived
            assert not _differs(_reordered(full, k, lambda t, j, s: (j, s, t)), want, label, fam), name        # (tau, start, j): identical
            caught["(tau, -j)"].update(_differs(_reordered(full, k, lambda t, j, s: (-j, t)), want, label, fam))
            caught["(start, tau, j)"].update(_differs(_reordered(full, k, lambda t, j, s: (j, t, s)), want, label, fam))
    print(f"order mutants caught by {caught}")
    assert "ties" in caught["(tau, -j)"] and "ties" in caught["(start, tau, j)"], caught


# ------------------------------------------------------------------------------------------------------------------ float64 truth
TRUTH_SCENES = (("rgbbox", 17), ("irreg", 29), ("random600", 41))
BAND = 1e-3
TAU_BOUND = 4 * 3.92e-3


def _truth_arrays(name):
    if name in ES.SCENES:
        return _scene(name)[0]
    return O.OracleScene(name).arrays()


def _float64_rule(L, rays, rq, lo, hi):
    """(kind [m, n], t1 [m, n], near [m, n]) of the contact rule in float64 from the float32 inputs; near: a deciding quantity lies within
    a relative BAND of its boundary"""
    o, d = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    c = L[None, :, :3].astype(np.float64)
    R = L[None, :, 6].astype(np.float64) + float(F(rq) + F(0))
    lo, hi = float(F(lo)), float(F(hi))
    oc = o - c
    a = (d * d).sum(axis=2)
    b = (oc * d).sum(axis=2)
    cc = (oc * oc).sum(axis=2) - R * R
    disc = b * b - a * cc
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.maximum(disc, 0))
        t1, t2 = (-b - sq) / a, (-b + sq) / a
        good = disc > 0
        past = t1 > lo
        entry = good & past & (t1 < hi)
        start = good & ~past & (t2 > lo) & (lo < hi)
        near = np.abs(disc) <= BAND * np.maximum(b * b, np.abs(a * cc))
        for t, bound in ((t1, lo), (t1, hi), (t2, lo)):
            near |= good & (np.abs(t - bound) <= BAND * np.maximum(1.0, np.abs(t)))
    return np.where(entry, 1, np.where(start, 2, 0)).astype(np.uint8), t1, near


@pytest.mark.parametrize("name,seed", TRUTH_SCENES, ids=[s[0] for s in TRUTH_SCENES])
def test_float64_truth(name, seed):
    """The defined answer is the geometric one: outside a band of relative 1e-3 around the rule's boundaries (disc over max(b^2, |a c|);
    t1 - t_min, t1 - t_max and t2 - t_min over max(1, |t|)) the restatement's kind of every (query, sphere) pair equals the kind a float64
    brute force of the same rule gives from the same float32 inputs, without exception; the band removes at most 1 % of the pairs of any
    case.  An entry contact's tau lies within TAU_BOUND of the float64 t1, relative to max(1, |t1|): measured on these inputs with the
    restatement the largest such error is 3.92e-3 (rgbbox, radius 40 over (0.1, 30): c = |o - c|^2 - R^2 cancels against the scene's
    largest spheres; 8.4e-4 on irreg and 8.6e-4 on random600 in the same case, at most 1.8e-5 in the other three), and the bound is four
    times that, 1.57e-2 -- the cancellation varies with the seed, and a wrong root is off by O(1)."""
    arr = _truth_arrays(name)
    with np.errstate(divide="ignore"):
        ref = Q.RefScene(arr)
    L = np.asarray(arr["L"], dtype=F)
    rays = X.seeded_rays(arr, 1024, seed)
    o, d = rays[:, :3], rays[:, 3:]
    worst = 0.0
    for rq, lo, hi in ((0.0, 0.0, 1e9), (3.0, 0.0, 1.0), (40.0, 0.1, 30.0), (float(ES.median_radius(arr)), 0.0, 1e9)):
        kinds = S.contact_kinds(ref, o, d, rq, lo, hi)
        brute = S.contact_kinds(ref, o, d, rq, lo, hi, boxes=False)
        tau = np.zeros(kinds.shape, F)
        for s in range(0, rays.shape[0], 256):
            e = min(rays.shape[0], s + 256)
            tau[s:e] = S._dense_contacts(ref, o[s:e], d[s:e], np.full(e - s, F(lo)), np.full(e - s, F(hi)), np.full(e - s, F(rq)),
                                         np.ones(e - s, bool), np.full(e - s, -1), False)[1]
        k64 = np.zeros(kinds.shape, np.uint8)
        t64 = np.zeros(kinds.shape)
        near = np.zeros(kinds.shape, bool)
        for s in range(0, rays.shape[0], 128):
            k64[s:s + 128], t64[s:s + 128], near[s:s + 128] = _float64_rule(L, rays[s:s + 128], rq, lo, hi)
        share = near.mean()
        bad = (kinds != k64) & ~near
        entries = (kinds == 1) & (k64 == 1) & ~near
        err = np.abs(tau[entries].astype(np.float64) - t64[entries]) / np.maximum(1.0, np.abs(t64[entries]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
        print(f"{name} radius {rq} ({lo}, {hi}): band removes {share:.3%} of {near.size} pairs, {int(bad.sum())} disagreements outside it, "
              f"{int((kinds != brute).sum())} tree-versus-brute differences, {int(entries.sum())} entry contacts, "
              f"max |tau - t1| / max(1, |t1|) = {float(err.max()) if err.size else 0.0:.3e}")
        assert share <= 0.01, (name, rq, share)
        assert not bad.any(), f"{name} radius {rq} ({lo}, {hi}): {int(bad.sum())} pairs differ outside the band, first {np.argwhere(bad)[:5].tolist()}"
        assert entries.sum() > 100, (name, rq, int(entries.sum()))
        assert (err <= TAU_BOUND).all(), (name, rq, float(err.max()))
    print(f"{name}: worst tau error {worst:.3e} (bound {TAU_BOUND:.1e})")


def test_fuzz_scenes_are_the_ray_campaign_s():
    # tools/fuzz_scenes.py is ray_fuzz.py's random_scene moved into a module of its own: the same scene for the same seed as before the move
    # (the digest was taken from the function while it still lived in ray_fuzz.py)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from fuzz_scenes import random_scene
    finally:
        sys.path.pop(0)
    h = hashlib.sha256()
    for seed in (1, 2, 3, 5100, 5101, 7100, 7101, 7102):
        s, kind = random_scene(np.random.default_rng(seed), 1500)
        h.update(s.tobytes())
        h.update(str(kind).encode())
    assert h.hexdigest() == "26ad91872b1599165822f475cf134d65b89179722ac2e87c146943314da1e2e6"
