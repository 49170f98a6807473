"""CPU checks of the box queries' restatement (boxes_ref.py) and of what the kernel relies on: degenerate boxes against within_ref.within bit
for bit, the restatement against a float64 brute force, box and margin validity, the node test's counterexample search
(build/box_query_bound_check: clean with the slack, violations without it and on the partial boxes), and the loader's symbols and the
header's declarations."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import boxes_ref as B
import oracle_lib as O
import proximity_ref as P
import within_ref as W
from test_proximity_cpu import _points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


@pytest.fixture(scope="module", params=[("rgbbox", {}), ("irreg", {}), ("floor", {"n": 37, "k": 222.0})], ids=["rgbbox", "irreg", "floor"])
def scene(request):
    name, kw = request.param
    return O.OracleScene(name, **kw).arrays()["L"]


@pytest.mark.parametrize("margin", [0.0, 0.5, 3.0, 1e9, "per-box"])
def test_degenerate_boxes_equal_within(scene, margin):
    L = scene
    m = 384
    p = _points(L, m, 5)
    p[7, 1] = np.nan
    p[9, 2] = np.inf
    if margin == "per-box":
        margin = np.random.default_rng(3).uniform(0.0, 6.0, m).astype(F)
        margin[[11, 12, 13, 14]] = [np.nan, -1.0, np.inf, 2e9]
        margin[15] = -0.0
    assert np.array_equal(_bits(B.gaps(L, B.degenerate(p[16:80]))), _bits(P.gaps(L, p[16:80])))       # the expression itself, every pair
    rng = np.random.default_rng(2)
    first = rng.integers(-5, L.shape[0] + 5, m)
    for f in (None, first):
        got, want = B.in_boxes(L, B.degenerate(p), margin, f), W.within(L, p, margin, f)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w))
        assert got[0][-1] > 0 and got[0][8] == got[0][7] and got[0][10] == got[0][9]


def test_against_float64(scene):
    L = scene
    m = 512
    rng = np.random.default_rng(21)
    boxes = B.random_boxes(L, m, 20, zero_every=0)
    margin = rng.uniform(0.0, 3.0, m).astype(F)
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    g32, g64 = B.gaps(L, boxes), B.gaps64(L, boxes)
    clear = np.abs(g64 - margin[:, None].astype(np.float64)) > 2.0 ** -18 * (1.0 + ext)
    sel32, sel64 = g32 <= margin[:, None], g64 <= margin[:, None].astype(np.float64)
    left_out = 1.0 - clear.mean()
    print(f"pairs {clear.size}, left out {left_out:.3g}, selected {int(sel32.sum())}, disagreeing {int((sel32 != sel64)[clear].sum())}")
    assert not (sel32 != sel64)[clear].any()
    assert left_out <= 1e-4
    assert sel32.sum() >= 3000                                               # not vacuous
    # ... and the CSR assembly is that selection
    off, idx, gap = B.in_boxes(L, boxes, margin)
    r, c = np.nonzero(sel32)
    assert np.array_equal(np.diff(off), sel32.sum(axis=1)) and np.array_equal(idx, c) and np.array_equal(_bits(gap), _bits(g32[r, c]))
    # a box that holds a centre: gap -r exactly
    inside = ((boxes[:, None, :3] <= L[None, :, :3]) & (L[None, :, :3] <= boxes[:, None, 3:])).all(axis=2)
    assert inside.sum() > 100 and np.array_equal(_bits(g32[inside]), _bits(np.broadcast_to(-L[None, :, 6], g32.shape)[inside]))


def test_box_and_margin_validity(scene):
    L = scene
    c = L[L.shape[0] // 2, :3].astype(np.float64)
    good = np.concatenate([c - 2.0, c + 2.0]).astype(F)
    boxes = np.tile(good, (12, 1))
    boxes[1, 0], boxes[1, 3] = good[3], good[0]                              # lo.x > hi.x
    boxes[2, 4] = np.nan
    boxes[3, 2] = -np.inf
    boxes[4, 5] = np.inf
    boxes[5, 1] = boxes[5, 4] = good[1]                                      # zero extent in y: valid
    boxes[6, :3] = boxes[6, 3:] = c.astype(F)                                # zero extent in all: valid
    boxes[7, 2], boxes[7, 5] = np.nextafter(good[5], F(np.inf)), good[5]     # lo.z one ulp above hi.z
    ok = B.box_ok(boxes)
    assert ok.tolist() == [True, False, False, False, False, True, True, False, True, True, True, True]
    margin = np.full(12, 1.0, F)
    margin[8:12] = [-0.0, np.nan, -1.0, 1.0000001e9]
    off, idx, gap = B.in_boxes(L, boxes, margin)
    ln = np.diff(off)
    assert ln[0] > 0 and not ln[[1, 2, 3, 4, 7, 9, 10, 11]].any() and ln[6] > 0 and ln[5] > 0
    z = B.in_boxes(L, boxes[8:9], 0.0)
    assert ln[8] == z[0][1] > 0 and np.array_equal(idx[off[8]:off[9]], z[1]) and np.array_equal(_bits(gap[off[8]:off[9]]), _bits(z[2]))
    # a scalar margin reaches the same rows
    s = B.in_boxes(L, boxes[:8], 1.0)
    assert np.array_equal(s[0], off[:9]) and np.array_equal(s[1], idx[: off[8]])


def _bound_check(*args):
    exe = os.path.join(ROOT, "build", "box_query_bound_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/box_query_bound_check"], check=True, capture_output=True)
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bound_check_finds_no_counterexample(seed):
    r = _bound_check(300, seed)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Q1 violations 0" in r.stdout and "safety violations 0" in r.stdout, r.stdout
    assert " 0 tall scenes" not in r.stdout and " 0 degenerate boxes" not in r.stdout and " 0 flat" not in r.stdout, r.stdout


def test_bound_check_sees_missing_slack():
    # the same search without the slack must find node boxes that would drop a selected sphere -- the check can fail
    r = _bound_check(100, 2, 0.0)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout, r.stdout


def test_bound_check_sees_partial_boxes():
    # ... and so must testing the partial boxes near the root of trees taller than the AABB propagation's sweeps
    r = _bound_check(100, 3, 1.0, 1)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout, r.stdout


def test_library_exports_boxes():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym, nargs in {"rt_spheres_in_boxes_count": 8, "rt_spheres_in_boxes_fill": 12}.items():
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
        assert len(getattr(_lib.lib, sym).argtypes) == nargs, sym
    for name in ("spheres_in_boxes", "spheres_in_boxes_count_into", "spheres_in_boxes_fill_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.spheres_in_boxes).parameters) == ["prepared", "boxes", "margin", "first", "gaps", "rows"]
    assert inspect.signature(R.spheres_in_boxes).parameters["margin"].default == 0.0


def test_header_declares_boxes():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_spheres_in_boxes_count(", "rt_spheres_in_boxes_fill("):
        assert sym in h, sym
    assert "family=boxes count" in h and "lo == hi == p" in h and "bit for bit" in h
