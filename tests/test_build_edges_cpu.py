"""The scenes of edge_builds.py can catch what they are there for (oracle and numpy only; the device leg is test_build_edges_gpu.py).

For every family at every size of the device leg: the premises each family is built on (distinct rows of L, one key, groups above two sort
tiles, flat axes, many small tie groups); edge_builds' Jacobi propagation at floor(log2 n) + 2 sweeps equals the oracle's boxes bit for
bit, and with one sweep more or fewer at least 256 inner nodes of `forest` change (at least one of `tall`); the builder's drop-out rule
restated over two ping-pong buffers equals the plain propagation on the tall families, and the mutant that drops a node one sweep early
does not; an order that is not stable changes L's bytes; the tall families reach depth 32 (48 at 524 289 spheres), the second depth
digit's values 2 and 3; their height exceeds the sweep count and that of `same` / `few` does not; and every frame's camera sees spheres.

`python tests/test_build_edges_cpu.py` prints the figures DESIGN.md 7 quotes."""
import functools

import numpy as np
import pytest

import edge_builds as B
import oracle_lib as O

CASES = B.finite_cases()
NON_FINITE_CASES = [(f, n) for f in B.NON_FINITE for n in B.NON_FINITE_SIZES]
SORT_TILE = 1024
_id = lambda c: f"{c[0]}:{c[1]}"   # noqa: E731


def _oracle(family, n):
    lf, la, fov = B.VIEWS.get(family, ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 40.0))
    return O.OracleScene("custom", spheres7=B.scene(family, n), look_from=lf, look_at=la, fov=fov)


@functools.lru_cache(maxsize=None)
def facts(family, n):
    """everything the tests below assert, as small values (the arrays of a 524 289-sphere scene are not kept)"""
    s = B.scene(family, n)
    orc = _oracle(family, n)
    a = orc.arrays()
    left, right, L, morton = a["left"], a["right"], a["L"], a["morton"]
    f = dict(n=n, sweeps=B.sweeps_of(n))
    sw = f["sweeps"]
    # the order
    ids = B.ids_of(L)
    # (the index read from a row's colour is a permutation: no two rows are equal)
    f["rows_distinct"] = bool((np.sort(ids) == np.arange(n)).all() and s[ids].tobytes() == L.tobytes())
    keys = B.unsorted_keys(morton, L)
    f["stable_is_oracle"] = bool((B.stable_order(keys) == ids).all())
    f["unstable_changes_L"] = s[B.unstable_order(keys)].tobytes() != L.tobytes()
    groups = B.tie_groups(morton)
    f["keys"], f["max_group"], f["groups_ge2"] = int(groups.size), int(groups.max()), int((groups >= 2).sum())
    f["flat_axes"] = int(sum(np.ptp(s[:, k]) == 0 for k in range(3)))
    # the boxes
    st = B.propagate_states(left, right, L, (sw - 1, sw, sw + 1))
    f["propagation_is_oracle"] = not B.boxes_differ(st[sw], (a["bmin"], a["bmax"])).any()
    f["plus_one"], f["minus_one"] = int(B.boxes_differ(st[sw], st[sw + 1]).sum()), int(B.boxes_differ(st[sw], st[sw - 1]).sum())
    if family in B.TALL:
        f["dropout_is_plain"] = not B.boxes_differ(B.propagate_dropout(left, right, L, sw), st[sw]).any()
        f["early_dropout_differs"] = int(B.boxes_differ(B.propagate_dropout(left, right, L, sw, early=1), st[sw]).sum())
    depth = B.node_depths(left, right)
    f["max_depth"], f["height"] = int(depth.max()), int(depth.max()) + 1
    # the view
    h, w = B.rays_of(family, n)
    idx, _ = orc.objs_hit_rays(B.primary_rays(orc.camera_floats(h, w), h, w), 0.0, 1e9)
    f["hit_fraction"] = float(np.mean(idx >= 0))
    orc.close()
    return f


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_premises(case):
    family, n = case
    f = facts(family, n)
    assert f["rows_distinct"], "every sphere has its own row, and edge_builds.ids_of reads the order back from L"
    assert f["stable_is_oracle"], "the oracle's order is the stable sort by key"
    if family == "same":
        assert f["keys"] == 1 and f["max_group"] == n
    elif family == "few":
        assert f["keys"] == 7 and f["max_group"] > 2 * SORT_TILE
    elif family in ("line", "line_z"):
        assert f["flat_axes"] == 2 and f["keys"] == 1024 and n // 1024 <= f["max_group"] <= n // 1024 + 2
    elif family == "forest":
        assert f["groups_ge2"] >= 1000 and f["max_group"] < 64
    elif family == "tall":
        assert f["keys"] == 32 and f["max_group"] == n - 31
    assert f["hit_fraction"] >= 0.05, f["hit_fraction"]


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "tall"], ids=_id)
def test_an_unstable_order_changes_L(case):
    """(equal keys by descending index; `tall` is one tie group at the end of a chain: `same` is the family for that)"""
    family, n = case
    assert facts(family, n)["unstable_changes_L"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_sweep_count_shows_in_the_boxes(case):
    family, n = case
    f = facts(family, n)
    assert f["sweeps"] == int(np.floor(np.log2(n))) + 2            # (no size here is near 2^23, where float32 log2 rounds up)
    assert f["propagation_is_oracle"], "edge_builds.propagate at floor(log2 n) + 2 sweeps == the oracle's boxes, bit for bit"
    if family == "forest":
        assert f["plus_one"] >= 256 and f["minus_one"] >= 256, (f["plus_one"], f["minus_one"])
    elif family == "tall":
        assert f["plus_one"] >= 1 and f["minus_one"] >= 1, (f["plus_one"], f["minus_one"])
    if family in B.TALL:
        assert f["dropout_is_plain"], "the drop-out rule gives the plain propagation's boxes"
        assert f["early_dropout_differs"] >= 256, f["early_dropout_differs"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_heights_and_depths(case):
    family, n = case
    f = facts(family, n)
    if family in B.TALL:
        assert f["max_depth"] >= 32, f["max_depth"]                # the depth sort's second digit takes the value 2
        assert f["height"] > f["sweeps"]                           # no culling, exact_depth > 0
        if (family, n) == ("tall", B.HUGE):
            assert f["max_depth"] >= 48, f["max_depth"]            # ... and 3
    elif family in ("same", "few"):
        assert f["height"] <= f["sweeps"], (f["height"], f["sweeps"])


@pytest.mark.parametrize("case", NON_FINITE_CASES, ids=_id)
def test_oracle_build_is_defined_on_non_finite_spheres(case):
    """The oracle's build of the non-finite families: fminf / fmaxf drop a NaN in the bounds and in `enclosing`, a non-finite quotient
    quantises to 0 or 1023 -- nothing undefined -- so the device leg expects the oracle's arrays for them too.  The numpy propagation
    agrees wherever the oracle's box is not NaN, and is NaN where it is."""
    family, n = case
    orc = _oracle(family, n)
    a = orc.arrays()
    s = B.scene(family, n)
    ids = B.ids_by_rows(a["L"], s)
    keys = np.empty(n, np.uint32)
    keys[ids] = a["morton"]
    assert (B.stable_order(keys) == ids).all()
    lo, hi = B.propagate(a["left"], a["right"], a["L"], B.sweeps_of(n))
    for got, want in ((lo, a["bmin"]), (hi, a["bmax"])):
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()
    assert np.isnan(a["bmin"]).any() == (family == "nan_y")       # (one NaN is dropped by its sibling: only a whole axis of them stays)
    orc.close()


if __name__ == "__main__":
    print("| family:n | height | sweeps | nodes changed by +1 / -1 sweep | largest tie group | keys | max depth |")
    print("|---|---|---|---|---|---|---|")
    for fam, n in CASES:
        f = facts(fam, n)
        print(f"| {fam}:{n} | {f['height']} | {f['sweeps']} | {f['plus_one']} / {f['minus_one']} | {f['max_group']} | {f['keys']} | {f['max_depth']} |")
