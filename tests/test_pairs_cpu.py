"""Visibility matrices (rt_visible_pairs) without a GPU: the restatement's packing and counts against a plain double loop, unpack_visible
against the packing, the premise of the GPU cases -- the seeded pairs give both outcomes on both scenes -- and the interface."""
import functools
import inspect
import os

import numpy as np
import pytest

import oracle_lib as O
import pairs_ref as P
import ray_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _scene(spec):
    arr = O.OracleScene(spec).arrays()
    return arr, Q.RefScene(arr)


def test_packing_and_counts_against_a_double_loop():
    rng = np.random.default_rng(5)
    vis = rng.random((3, 130)) < 0.4
    vis[1, 128:] = True                     # the last word's two live bits
    vis[2] = False
    words = P.pack(vis)
    assert words.dtype == np.uint64 and words.shape == (3, 3)
    want = [[0, 0, 0] for _ in range(3)]
    count = [0, 0, 0]
    for i in range(3):
        for j in range(130):
            if vis[i, j]:
                want[i][j >> 6] |= 1 << (j & 63)
                count[i] += 1
    assert [[int(x) for x in row] for row in words] == want
    assert P.popcount(words).tolist() == count
    assert P.popcount(words).dtype == np.int32
    # the little-endian layout the header documents: byte b of a row holds pairs 8 b .. 8 b + 7, lowest bit first
    raw = words.astype("<u8").view(np.uint8).reshape(3, 24)
    assert np.array_equal(np.unpackbits(raw, axis=1, bitorder="little")[:, :130].astype(bool), vis)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 130])
def test_unpack_visible_inverts_the_packing(m):
    import raytracers_amd as R
    rng = np.random.default_rng(m)
    vis = rng.random((5, m)) < 0.5
    vis[0] = True
    vis[1] = False
    words = P.pack(vis)
    assert words.shape == (5, (m + 63) // 64)
    back = R.unpack_visible(words, m)
    assert back.dtype == bool and back.shape == (5, m)
    assert np.array_equal(back, vis)
    # the tail bits are zero: a row of all-visible pairs fills exactly m bits
    tail = R.unpack_visible(words, 64 * words.shape[1])[:, m:]
    assert not tail.any()
    assert int(P.popcount(words)[0]) == m


def test_validity_rule():
    nan, inf = np.float32("nan"), np.float32("inf")
    pts = np.array([[0, 0, 0], [nan, 0, 0], [1, 2, 3], [0, -inf, 0], [3e38, 0, 0]], np.float32)
    tg = np.array([[1, 2, 3], [0, 0, 0], [inf, 0, 0], [0, nan, 0], [-0.0, 0.0, -0.0], [-3e38, 0, 0]], np.float32)
    t = P.valid_pairs(pts, tg, P.TARGETS)
    assert t.tolist() == [[True, False, False, False, False, True],     # (0,0,0): equal to target 1 and to target 4 (-0.0)
                          [False] * 6,                                   # a NaN point
                          [False, True, False, False, True, True],      # equal to target 0
                          [False] * 6,                                   # an infinite point
                          [True, True, False, False, True, False]]      # 3e38 - (-3e38) overflows: d is not finite
    d = P.valid_pairs(pts, tg, P.DIRECTIONS)
    assert d.tolist() == [[True, False, False, False, False, True], [False] * 6, [True, False, False, False, False, True], [False] * 6,
                          [True, False, False, False, False, True]]


PREMISE = [("rgbbox", P.TARGETS, (1e-3, 1.0), 69), ("rgbbox", P.DIRECTIONS, (0.1, 1e9), 49),
           ("irreg", P.TARGETS, (1e-3, 1.0), 91), ("irreg", P.DIRECTIONS, (0.1, 1e9), 59)]


@pytest.mark.parametrize("spec,mode,interval,blocked_pct", PREMISE)
def test_seeded_pairs_give_both_outcomes(spec, mode, interval, blocked_pct):
    arr, ref = _scene(spec)
    points, targets, directions = P.seeded(arr, 64, 130, P.SEEDS[spec])
    tg = targets if mode == P.TARGETS else directions
    vis = P.visible(ref, points, tg, mode, *interval)
    ok = P.valid_pairs(points, tg, mode)
    assert ok.sum() > 0 and not (vis & ~ok).any()
    blocked = (ok & ~vis).sum() / ok.sum()
    seen = (ok & vis).sum() / ok.sum()
    print(f"{spec} mode {mode}: {ok.sum()} valid pairs, {100 * blocked:.1f} % blocked")
    assert blocked >= 0.05 and seen >= 0.05, (blocked, seen)
    assert round(100 * blocked) == blocked_pct, blocked
    words, count = P.reference(ref, points, tg, mode, *interval)
    assert np.array_equal(count, vis.sum(axis=1))


def test_library_exports_pairs():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_visible_pairs", "rt_visible_pairs_shaped"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_visible_pairs.argtypes) == 11
    assert len(_lib.lib.rt_visible_pairs_shaped.argtypes) == 12
    for name in ("visible_pairs", "visible_pairs_into", "unpack_visible"):
        assert callable(getattr(R, name)), name
    assert (R.PAIRS_TARGETS, R.PAIRS_DIRECTIONS) == (0, 1)
    sig = inspect.signature(R.visible_pairs)
    assert list(sig.parameters)[:8] == ["prepared", "points", "targets", "directions", "t_min", "t_max", "mask", "count"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:8]] == [None, None, 0.0, 1e9, True, True]
    assert list(inspect.signature(R.visible_pairs_into).parameters)[:10] == [
        "points_ptr", "n", "targets_ptr", "m", "prepared", "mode", "visible_ptr", "count_ptr", "t_min", "t_max"]
    assert list(inspect.signature(R.unpack_visible).parameters) == ["words", "m"]


def test_header_declares_pairs():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_visible_pairs(", "rt_visible_pairs_shaped(", "RT_PAIRS_TARGETS = 0, RT_PAIRS_DIRECTIONS = 1", "family=pairs targets",
                "family=pairs directions", "little-endian", 'bitorder="little"'):
        assert sym in h, sym
    dev = open(os.path.join(ROOT, "raytracers_amd", "csrc", "query_device.hpp")).read()
    assert "pairs_auto_words_per_wave" in dev and "launch_visible_pairs" in dev
