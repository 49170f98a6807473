"""CPU checks of the range queries' restatement (within_ref.py) and of what the kernels rely on: the restatement against proximity_ref.nearest
(row lengths equal its counts; a row no longer than 32, sorted by (gap, j), equals its slots), its restricted form against the dense one,
contact pairs against the i < j half of a dense self-query, the left-first depth-first leaf order of the oracle's trees (ascending: why rows
need no sort), the scan's arithmetic in three passes with 64-bit sums, and the loader's symbols and the header's declarations."""
import inspect
import os

import numpy as np
import pytest

import oracle_lib as O
import proximity_ref as P
import within_ref as W
from test_proximity_cpu import _points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _random_scene(n, seed, dup=0):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), F)
    s[:, :3] = rng.uniform(-40, 40, (n, 3))
    s[:, 3:6] = 0.5
    s[:, 6] = rng.uniform(0.3, 2.5, n)
    if dup:
        s[n - dup:, :3] = s[0, :3]        # coincident centres: equal Morton keys
    return s


@pytest.fixture(scope="module", params=[("rgbbox", {}), ("irreg", {}), ("floor", {"n": 37, "k": 222.0})], ids=["rgbbox", "irreg", "floor"])
def scene(request):
    name, kw = request.param
    return O.OracleScene(name, **kw).arrays()["L"]


@pytest.mark.parametrize("max_dist", [0.0, 0.5, 3.0, 1e9, "per-point"])
def test_rows_against_nearest(scene, max_dist):
    L = scene
    m = 384
    p = _points(L, m, 5)
    p[7, 1] = np.nan
    if max_dist == "per-point":
        max_dist = np.random.default_rng(3).uniform(0.0, 6.0, m).astype(F)
        max_dist[[11, 12, 13, 14]] = [np.nan, -1.0, np.inf, 2e9]
        max_dist[15] = -0.0
    off, idx, gap = W.within(L, p, max_dist)
    cnt, nidx, ngap = P.nearest(L, p, max_dist, P.KMAX)
    assert off.dtype == np.int64 and off[0] == 0 and off.shape == (m + 1,)
    assert np.array_equal(np.diff(off), cnt)                                  # row lengths == the capped query's counts
    assert idx.shape == (off[-1],) and gap.shape == (off[-1],)
    sidx, sgap = W.sort_rows_by_gap(off, idx, gap)
    short = 0
    for i in range(m):
        a, b = off[i], off[i + 1]
        row = idx[a:b]
        assert (np.diff(row) > 0).all()                                       # ascending j
        if b - a <= P.KMAX:
            short += 1
            assert np.array_equal(sidx[a:b], nidx[i, : b - a]) and np.array_equal(_bits(sgap[a:b]), _bits(ngap[i, : b - a])), i
            assert (nidx[i, b - a:] == -1).all()
    assert short > 0
    if np.ndim(max_dist) == 0 and max_dist == 1e9:
        assert (np.diff(off)[np.isfinite(p).all(axis=1)] == L.shape[0]).all()
    assert off[8] == off[7]                                                   # the NaN point's row is empty


def test_first_filters_rows(scene):
    L = scene
    n = L.shape[0]
    m = 200
    p = _points(L, m, 6)
    rng = np.random.default_rng(2)
    first = rng.integers(-5, n + 5, m)
    first[:4] = [0, -7, n, n + 3]
    off, idx, gap = W.within(L, p, 4.0)
    foff, fidx, fgap = W.within(L, p, 4.0, first)
    for i in range(m):
        row, g = idx[off[i]:off[i + 1]], gap[off[i]:off[i + 1]]
        keep = row >= first[i]
        assert np.array_equal(fidx[foff[i]:foff[i + 1]], row[keep]) and np.array_equal(_bits(fgap[foff[i]:foff[i + 1]]), _bits(g[keep])), i
    assert foff[1] - foff[0] == off[1] - off[0] and foff[2] - foff[1] == off[2] - off[1]
    assert foff[3] == foff[2] and foff[4] == foff[3]


@pytest.mark.parametrize("kind", ["irreg", "dups", "cloud", "floor"])
def test_near_equals_dense(kind):
    rng = np.random.default_rng(4)
    if kind == "irreg":
        L = O.OracleScene("irreg").arrays()["L"]
    elif kind == "floor":
        L = O.OracleScene("floor", n=37, k=222.0).arrays()["L"]
    else:
        L = _random_scene(900, 9)
        if kind == "cloud":
            L[:, 6] = 0.0
        else:
            L[450:] = L[:450]
    m = 400
    p = _points(L, m, 11)
    p[:8] *= F(1e6)                                                           # far outside the grid
    p[9, 2] = np.inf
    md = rng.uniform(0.0, 8.0, m).astype(F)
    md[::17] = np.nan
    first = rng.integers(-3, L.shape[0] + 3, m)
    for bound in (md, 4.0, 0.0):
        for f in (None, first):
            got, want = W.within_near(L, p, bound, f), W.within(L, p, bound, f)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), (kind, f is None)
    for margin in (0.0, 1.0, 6.0):
        got, want = W.contact_pairs(L, margin, near=True), W.contact_pairs(L, margin)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), (kind, margin)


@pytest.mark.parametrize("margin", [0.0, 0.75, 20.0])
def test_contact_pairs_are_half_of_the_self_query(scene, margin):
    L = scene
    n = L.shape[0]
    pairs, gap = W.contact_pairs(L, margin)
    assert pairs.dtype == np.int32 and pairs.shape == (gap.size, 2)
    assert (pairs[:, 0] < pairs[:, 1]).all()
    assert (np.lexsort((pairs[:, 1], pairs[:, 0])) == np.arange(gap.size)).all()          # ascending (i, j)
    # the dense self-query with the same one-sided bound: all j, then the i < j half; every sphere selects itself at gap -r
    off, idx, g = W.within(L, L[:, :3], W.contact_bounds(L, margin))
    rows = np.repeat(np.arange(n), np.diff(off))
    assert ((rows == idx) & (_bits(g) == _bits(-L[rows, 6]))).sum() == n
    half = idx > rows
    assert np.array_equal(pairs[:, 0], rows[half]) and np.array_equal(pairs[:, 1], idx[half]) and np.array_equal(_bits(gap), _bits(g[half]))
    # ... and directly, pair by pair, from the definition
    G = P.gaps(L, L[:, :3])
    want = {(i, j) for i, j in zip(*np.nonzero(G <= W.contact_bounds(L, margin)[:, None])) if i < j}
    assert want == set(map(tuple, pairs.tolist()))
    assert len(want) > 0


def _dfs_leaf_order(left, right):
    """the leaves in the order a depth-first walk from the root meets them when it pushes the right child, then the left (leaf j is -2 - j)"""
    out, stack = [], [0]
    while stack:
        c = stack.pop()
        if c < 0:
            out.append(-2 - c)
            continue
        stack.append(int(right[c]))
        stack.append(int(left[c]))
    return np.array(out)


def _custom(s):
    return O.OracleScene("custom", spheres7=s, look_from=(0.0, 5.0, 90.0), look_at=(0.0, 0.0, 0.0), fov=50.0).arrays()


@pytest.mark.parametrize("spec", ["rgbbox", "irreg", "random", "tall1100"])
def test_left_first_walk_meets_leaves_in_ascending_order(spec):
    import edge_rays as E
    if spec in ("rgbbox", "irreg"):
        A = O.OracleScene(spec).arrays()
    elif spec == "random":
        A = _custom(_random_scene(5000, 12, dup=40))
    else:
        A = _custom(E.SCENES["tall1100"][0])
    n = A["L"].shape[0]
    assert A["left"].min() < -1 and A["right"].min() < -1                      # leaves are coded -2 - j
    order = _dfs_leaf_order(A["left"], A["right"])
    assert np.array_equal(order, np.arange(n)), spec


def _scan3(counts, items=1024, threads=256):
    """the device scan's three passes: block sums; one pass over the block sums, `threads` at a time with a carry; block re-scan plus base"""
    c = np.asarray(counts, dtype=np.int32)
    n = c.size
    nb = (n + items - 1) // items
    padded = np.zeros(nb * items, np.int64)
    padded[:n] = c
    sums = padded.reshape(nb, items).sum(axis=1)
    base = np.zeros(nb, np.int64)
    carry = 0
    for s in range(0, nb, threads):
        part = sums[s:s + threads]
        incl = np.cumsum(part)
        base[s:s + threads] = carry + incl - part
        carry += int(part.sum())
    offsets = np.zeros(n + 1, np.int64)
    inner = np.cumsum(padded.reshape(nb, items), axis=1) + base[:, None]
    offsets[1:] = inner.reshape(-1)[:n]
    return offsets


@pytest.mark.parametrize("n", [0, 1, 63, 1023, 1024, 1025, 300000])
def test_scan_arithmetic(n):
    rng = np.random.default_rng(n)
    c = rng.integers(0, 1 << 26, n).astype(np.int32)
    want = np.concatenate([[0], np.cumsum(c.astype(np.int64))])
    got = _scan3(c)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if n == 300000:
        assert want[-1] > 1 << 32                                              # past 32 bits
        assert not np.array_equal(np.cumsum(c, dtype=np.int32).astype(np.int64), want[1:])   # (a 32-bit scan would be wrong)


def test_scan_arithmetic_whole_scene_rows():
    # 4 096 rows of 10^6 entries: offsets[i] = i * 10^6 exactly, total 4.096e9: past int32 (2^31 = 2.147e9) though still below 2^32 = 4.295e9;
    # 4 352 such rows pass 2^32 too
    for rows in (4096, 4352):
        got = _scan3(np.full(rows, 1000000, np.int32))
        assert np.array_equal(got, np.arange(rows + 1, dtype=np.int64) * 1000000) and got[-1] > 1 << 31
    assert got[-1] > 1 << 32


def test_library_exports_within():
    from raytracers_amd import _lib
    import raytracers_amd as R
    want = {"rt_spheres_within_count": 8, "rt_spheres_within_fill": 12, "rt_contact_pairs_count": 4, "rt_contact_pairs_fill": 7}
    for sym, nargs in want.items():
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
        assert len(getattr(_lib.lib, sym).argtypes) == nargs, sym
    for name in ("spheres_within", "contact_pairs", "spheres_within_count_into", "spheres_within_fill_into", "contact_pairs_count_into",
                 "contact_pairs_fill_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.spheres_within).parameters) == ["prepared", "points", "max_dist", "first", "gaps", "rows"]
    assert list(inspect.signature(R.contact_pairs).parameters) == ["prepared", "margin", "gaps"]


def test_header_declares_within():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_spheres_within_count(", "rt_spheres_within_fill(", "rt_contact_pairs_count(", "rt_contact_pairs_fill("):
        assert sym in h, sym
    assert "family=within count" in h and "ASCENDING j" in h
