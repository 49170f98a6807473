"""The view-order tests' CPU side: the premises of every case of tests/view_order_cases.py (which sizes sit on which side of the sorts'
workgroup, chunk and cap arithmetic), the restatements of tests/view_order_ref.py against their own invariants, the mutants -- each
deliberate fault of the restatement must change the expected arrays of the cases named for it, so that a kernel with that fault
cannot pass tests/test_view_order_gpu.py -- and the oracle's per-pixel chain lengths against its `rays` counter."""
import functools

import numpy as np
import pytest

import edge_rays as E
import oracle_lib as O
import view_order_cases as C
import view_order_ref as V


# ---------------------------------------------------------------------------------------------------------------- premises
def test_tile_order_premises():
    wg = C.tile_order_workgroups
    assert (64 * 32, wg(64 * 32, 1)) == (2048, 1), "64x32: the last size with one workgroup"
    assert (683 * 3, wg(683 * 3, 1)) == (2049, 2), "683x3: the first size with two workgroups"
    assert 500 * 500 == 250000 and (250000 + 2047) // 2048 > 64 and wg(250000, 1) == 64, "500x500: the workgroups are capped at 64"
    geoms = set(C.TILE_GEOMS)
    for g in [(1, 1, 1), (7, 3, 1), (64, 32, 1), (683, 3, 1), (500, 500, 1)] + [(tx, ty, 8) for tx in (3, 8, 13, 125) for ty in (5, 125)]:
        assert g in geoms
        assert g[2] == 1 or wg(g[0] * g[1], 8) == 1, "the issue's eight-strip grids: one workgroup per strip"
    widths = lambda tx: [s[1] for s in V.strips(tx, 5, 8)]
    assert 0 in widths(3) and sum(widths(3)) == 3, "tiles_x = 3 under eight strips: strips of zero width"
    assert ((24 + 7) // 8, (40 + 7) // 8) == (3, 5), "... the grid of a 24 x 40 frame (that the host cuts it into eight strips under xcd_queues = 1: test_view_order_gpu)"
    assert (400, 100, 8) in geoms and wg(400 * 100, 8) == 3, "400x100 under eight strips: 5 000 tiles and three workgroups per strip"
    assert set(widths(8)) == {1}
    assert sorted(set(widths(13))) == [1, 2], "tiles_x = 13: unequal strips"
    assert sorted(set(widths(125))) == [15, 16], "tiles_x = 125: unequal strips of 15 and 16 columns"
    for tx in (3, 8, 13, 125):
        for ty in (5, 125):
            st = V.strips(tx, ty, 8)
            assert st[0][2] == 0 and all(a[2] + a[3] == b[2] for a, b in zip(st, st[1:])) and st[-1][2] + st[-1][3] == tx * ty, "the segments tile the table"
    # the records are what their names say
    for (tx, ty, ns) in C.TILE_GEOMS:
        n = tx * ty
        assert (C.tile_record(tx, ty, ns, "zeros") == 0).all() and (C.tile_record(tx, ty, ns, "all63") == 63).all()
        assert np.count_nonzero(C.tile_record(tx, ty, ns, "one")) == 1
        if n > 1:
            assert (np.diff(C.tile_record(tx, ty, ns, "rising")) > 0).all() and (np.diff(C.tile_record(tx, ty, ns, "falling")) < 0).all()
        if n >= 2048:
            w = C.tile_record(tx, ty, ns, "wild")
            assert w.min() < 0 and w.max() > 63 and {62, 63, 64, -1, 0, 1} <= set(w.tolist())
            assert len(set(V.tile_bin(C.tile_record(tx, ty, ns, "mix")).tolist())) == 64, "the mix occupies every bin"


def test_pixel_list_premises():
    g = C.px_geoms()
    wg = lambda name: V.px_workgroups(g[name].ntiles)
    assert wg("512x512") == (16, 256), "512x512: 256 workgroups, one round of the scan"
    assert wg("520x512") == (16, 260), "520x512: 260 workgroups, the scan's second round"
    assert g["1456x1448"].ntiles > 32768 and wg("1456x1448")[0] == 32, "1456x1448: more than 2048 x 16 tiles, 32 tiles per workgroup"
    assert g["1600x1600"].ntiles == 40000 and wg("1600x1600") == (32, 1250), "1600x1600: exactly the 40 000-tile gate"
    assert wg("250x333")[0] == 16 and wg("53x37") == (16, 3)
    for name in ("1x1", "8x8", "77x1", "1x77", "53x37", "250x333"):
        assert name in g
    from raytracers_amd import dist
    for (h, rpt, part, nparts) in ((100, 8, 0, 3), (300, 16, 2, 8), (53, 8, 1, 3), (256, 16, 1, 3), (7, 8, 0, 1), (40, 8, 2, 3)):
        assert np.array_equal(C.part_rows(h, rpt, part, nparts), dist.tile_rows(h, part, nparts, rpt)), "part_rows restates dist.tile_rows"
    a, b = g["in place 53x100 rpt 8 part 0 of 3"], g["in place 40x300 rpt 16 part 2 of 8"]
    assert (a.rpt_log2, a.out_skip, a.rows_local) == (3, 2 * 8 * 53, 36) and (b.rpt_log2, b.out_skip, b.rows_local) == (4, 7 * 16 * 40, 44)
    assert a.rows_local % 8 and b.rows_local % 8, "both parts end in a ragged row of tiles"
    for name, geo in g.items():
        lrow, col = V.px_in_tile_order(geo)
        assert lrow.size == geo.npix and np.unique(geo.record_index(lrow, col)).size == geo.npix, name
        assert geo.w < 65536 and geo.rows_local < 65536
    big = g["250x333"]
    assert len(np.flatnonzero(V.px_histogram(C.px_record("250x333", big, "gradient"), big))) == 64, "the gradient occupies every bin"
    assert len(np.flatnonzero(V.px_histogram(C.px_record("8x8", g["8x8"], "lanes"), g["8x8"]))) == 64, "lanes: 64 bins in one tile"
    assert len(np.flatnonzero(V.px_histogram(C.px_record("53x37", g["53x37"], "chequer"), g["53x37"]))) == 2
    assert V.px_histogram(C.px_record("53x37", g["53x37"], "some0"), g["53x37"])[0] > 0
    assert V.px_histogram(C.px_record("53x37", g["53x37"], "all255"), g["53x37"])[63] == 53 * 37
    pols = C.px_policies()
    assert len(pols) == 3 * 2 * (3 + 2 * 2)
    assert {tuple(p.thr) for p in pols.values()} == {(4, 3, 2, 2), (1, 1, 1, 1), (255, 255, 255, 255), (0, 24, 14, 9)}
    assert {p.solo_cap for p in pols.values()} == {0, 5, 2**30} and {p.nwaves for p in pols.values()} == {1, 256 * 16}


def test_first_order_premises():
    # the gates of the host: more than one tile row, at most 4096 rows and 32768 columns; the rank kernel's table holds rows + blocks <= 1024
    assert C.FIRST_GEOMS == [(1, 2), (3, 5), (8, 8), (125, 125), (9, 4096), (32768, 2)]
    for tx, ty in C.FIRST_GEOMS:
        assert 1 < ty <= 4096 and tx <= 32768
        o = V.first_order(tx, ty)
        assert np.array_equal(np.sort(o[:tx * ty]), np.arange(tx * ty)), "a permutation of the tiles"
        assert (o[tx * ty:] == 0).all() and o.size == tx * ty + 128
    assert 125 + 16 <= 1024 < 4096 + 2 and 2 + 4096 > 1024, "125x125 within the table, 9x4096 and 32768x2 beyond it"
    assert V.first_order(8, 8)[:16].tolist() == list(range(8)) + list(range(32, 40)), "rows 0, 4, 2, 6, ..."
    assert V.first_order(20, 2)[:20].tolist() == list(range(0, 8)) + list(range(16, 20)) + list(range(8, 16)), "blocks 0, 2, 1; the narrow block keeps its width"


# ---------------------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("geom", [g for g in C.TILE_GEOMS if g[0] * g[1] <= 20000], ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}")
def test_tile_order_restatement_invariants(geom):
    tx, ty, ns = geom
    n = tx * ty
    for rec in C.TILE_RECORDS:
        cost = C.tile_record(tx, ty, ns, rec)
        order, after = V.tile_order(cost, tx, ty, ns, C.FILL_I32)
        assert np.array_equal(np.sort(order[:n]), np.arange(n)) and not after.any()
        sat = np.clip(cost, 0, 63)
        for s, (x0, sw, seg, cnt) in enumerate(V.strips(tx, ty, ns)):
            mine = order[seg:seg + cnt]
            assert ((mine % tx >= x0) & (mine % tx < x0 + sw)).all()
            assert (np.diff(sat[mine]) <= 0).all(), "descending"
            same = np.diff(sat[mine]) == 0
            key = (mine // tx) * tx + mine % tx
            assert (np.diff(key)[same] > 0).all(), "stable"
            tab = order[n + 16 * s:n + 16 * s + 16]
            assert tab[8] == cnt and (tab[9:] == C.FILL_I32).all() and (tab[:3] == 0).all()
            for c in range(3, 8):
                assert tab[c] == 0 or sat[mine[tab[c] - 1]] >= 2 ** (8 - c)
                assert tab[c] == cnt or sat[mine[tab[c]]] < 2 ** (8 - c)
        for s in range(ns, 8):
            assert (order[n + 16 * s:n + 16 * s + 16] == C.FILL_I32).all()


def test_pixel_list_restatement_invariants():
    geoms = C.px_geoms()
    for gname in ("1x1", "8x8", "77x1", "1x77", "53x37", "in place 53x100 rpt 8 part 0 of 3", "in place 40x300 rpt 16 part 2 of 8"):
        g = geoms[gname]
        want = np.sort((np.arange(g.rows_local)[:, None] << 16 | np.arange(g.w)[None, :]).ravel())
        for rec in C.PX_RECORDS:
            r = C.px_record(gname, g, rec)
            lst = V.px_list(r, g)
            assert np.array_equal(np.sort(lst), want), "a permutation of the part's pixels"
            rays = np.minimum(r[g.record_index(lst >> 16, lst & 0xffff)].astype(int), 63)
            assert (np.diff(rays) <= 0).all()
            # the same list from the sort key spelt out: (-min(rays, 63), tile, lane)
            lrow, col = (lst >> 16).astype(np.int64), (lst & 0xffff).astype(np.int64)
            key = ((63 - rays) << 40) | (((lrow >> 3) * g.tiles_x + (col >> 3)) << 6) | ((lrow & 7) * 8 + (col & 7))
            assert (np.diff(key) > 0).all()
            hist = V.px_histogram(r, g)
            hdr = V.px_header(hist, C.DEFAULT_POLICY, C.FILL_I32)
            assert hdr[0] == 0 and (np.diff(hdr[:6]) >= 0).all() and hdr[5] == g.npix and (np.diff(hdr[8:14]) >= 0).all() and hdr[14] == hdr[15] == 0


def test_header_restatement_by_hand():
    hist = [0] * 64
    hist[1], hist[2], hist[3], hist[4], hist[10], hist[63] = 1000, 100, 50, 20, 3, 2
    h = V.px_header(hist, V.PxPolicy((4, 3, 2, 2), C.G_LDS, 250, 4096, 5, 1), -7)
    # at most 5 pixels in the one-pixel class: chains of >= 5, the first length from 4 on that so few reach (the 5 pixels of 10 and 63 rays); then >= 3 (8 per ticket), >= 2 (16), nothing for 32, the rest 64
    assert h[:6].tolist() == [0, 5, 75, 175, 175, 1175] and h[6] == 5 | 3 << 8 | 2 << 16 | 2 << 24 and h[7] == 1
    assert h[8:14].tolist() == [0, 5, 5 + 9, 14 + 7, 21, 21 + 16] and h[14] == 0 and h[15] == 0
    h = V.px_header(hist, V.PxPolicy((4, 3, 2, 2), C.G_LDS, 250, 4096, 0, 0), -7)
    assert h[:6].tolist() == [0, 0, 75, 175, 175, 1175] and h[6] == 64 | 3 << 8 | 2 << 16 | 2 << 24 and h[7] == 0
    # the model on one bin: T = 63 * g[0] = 1260 -> cuts min(64, 1260 // g + 1) = 29, 20, 13, 8; the waves' time does not raise it
    one = [0] * 64
    one[63] = 10
    assert V.model_cuts(one, V.PxPolicy((0, 0, 0, 0), C.G_LDS, 250, 4096, 5, 1)) == [29, 20, 13, 8]
    # one wave for everything, no solo loop: T = 1 * g[1] = 45 puts the one-ray chains into the 8-pixel class (cuts 64, 1, 1, 1), whose 1000 rays
    # take the one wave 1000 * 45 // 8 = 5625; at T = 5625 the cuts are 64, 64, 57, 32, the rays are bulk (2500 <= T) and T stands
    lots = [0] * 64
    lots[1] = 1000
    assert V.model_cuts(lots, V.PxPolicy((0, 0, 0, 0), C.G_LDS, 250, 1, 0, 1)) == [64, 64, 57, 32]


    # where the roundings matter (each bin's share is floored on its own): one pixel of 1 ray and 13 of 3, g = 10 .. 50, one wave, no solo loop.  T = 3 * 20
    # = 60 -> cuts 64, 3, 2, 2: the 1-ray pixel is bulk, 250 // 100 = 2 (2.5), the 39 rays of the 3-ray pixels ride 8 to a wave, 39 * 20 // 8 = 97 (97.5):
    # T = 99, not 100 -> cuts 64, 4, 3, 2 (at 100 the 32-pixel cut would be 100 // 50 + 1 = 3); then 2 + 39 * 30 // 16 = 75 <= 99 and T stands
    two = [0] * 64
    two[1], two[3] = 1, 13
    assert V.model_cuts(two, V.PxPolicy((0, 0, 0, 0), (10, 20, 30, 40, 50), 250, 1, 0, 1)) == [64, 4, 3, 2]


# ---------------------------------------------------------------------------------------------------------------- mutants
@functools.lru_cache(maxsize=None)
def _geoms():
    return C.px_geoms()


def _expected(case, mutant):
    if case[0] == "tile":
        _, tx, ty, ns, rec = case
        assert (tx, ty, ns) in C.TILE_GEOMS and rec in C.TILE_RECORDS
        return V.tile_order(C.tile_record(tx, ty, ns, rec), tx, ty, ns, C.FILL_I32, mutant)[0]
    g = _geoms()[case[1]]
    assert case[2] in C.PX_RECORDS
    rec = C.px_record(case[1], g, case[2])
    if case[0] == "px":
        return V.px_list(rec, g, C.FILL_U32, mutant)
    assert case[1] == C.POLICY_GEOM and case[2] in C.POLICY_RECORDS
    return V.px_header(V.px_histogram(rec, g, mutant), C.px_policies()[case[3]], C.FILL_I32, mutant)


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_every_mutant_changes_a_named_case(mutant):
    assert set(C.KILLERS) == set(V.MUTANTS)
    assert len(C.KILLERS[mutant]) >= 1
    for case in C.KILLERS[mutant]:
        good, bad = _expected(case, None), _expected(case, mutant)
        assert good.shape == bad.shape and not np.array_equal(good, bad), f"mutant {mutant} is not caught by case {case}"


def test_mutants_leave_the_other_families_alone():
    """a mutant is ONE fault: the pixel-list faults do not touch the tile order and the other way round"""
    g = _geoms()["53x37"]
    rec = C.px_record("53x37", g, "mix")
    for m in ("segments_reversed", "no_clamp0", "solo_uncapped", "cut_gt"):
        assert np.array_equal(V.px_list(rec, g, mutant=m), V.px_list(rec, g))
    cost = C.tile_record(13, 5, 8, "mix")
    for m in ("carry256", "lane_colmajor", "no_out_skip", "solo_uncapped"):
        assert np.array_equal(V.tile_order(cost, 13, 5, 8, 0, m)[0], V.tile_order(cost, 13, 5, 8, 0)[0])


# ---------------------------------------------------------------------------------------------------------------- chain lengths
def _custom():
    s7, lf, la, fov = E.SCENES["random600"]
    return O.OracleScene("custom", spheres7=s7, look_from=lf, look_at=la, fov=fov)


@pytest.mark.parametrize("scene,h,w,depth,rows", [("rgbbox", 77, 53, 50, None), ("rgbbox", 40, 40, 3, None), ("irreg", 64, 96, 50, (8, 40)),
                                                  ("custom", 72, 96, 50, None)])
def test_chain_lengths_add_up_to_the_rays_counter(scene, h, w, depth, rows):
    orc = _custom() if scene == "custom" else O.OracleScene(scene)
    _, cnt = orc.render(h, w, max_depth=depth, rows=rows)
    n = orc.chain_lengths(h, w, max_depth=depth, rows=rows)
    assert n.shape == ((h if rows is None else rows[1] - rows[0]), w)
    assert int(n.sum()) == cnt["rays"]
    assert n.min() >= 1 and n.max() <= depth
    if depth == 3:
        assert n.max() == 3, "some chains are cut off by max_depth"
    cost_px, cost = V.view_records(n, w)
    assert cost_px.shape == n.shape and cost.size == ((w + 7) // 8) * ((n.shape[0] + 7) // 8) and set(np.unique(cost)) <= {0} | set(range(3, depth + 1))
