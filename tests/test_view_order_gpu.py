"""The view-order sorts on the GPU, as integers, against the restatements of tests/view_order_ref.py: a view's tile order
with its class tables (tile_count / tile_scan / tile_place), its pixel list and 16-int header (px_count / px_scan / px_header / px_place),
the bit-reversed first order, and the same arrays of real views after rendered frames, whose records are compared with the oracle's
per-pixel chain lengths.  tools/view_order_check runs the launches (one process per test function) with every buffer between guards;
every array is compared with ==, guards included.  tests/test_view_order_cpu.py holds the premises of the cases and shows that each
fault the sorts could have (unstable, ascending, a bin or a carry or a cut off by one, ...) changes what is expected here."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import edge_rays as E
import oracle_lib as O
import view_order_cases as C
import view_order_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_failed = []      # a run of the tool that ended badly: nothing further is started on the device by this file


def _run(cases, tmp_path):
    """the tool over the cases, one process; a non-zero exit fails the test (the tool stops at its first HIP error) and every later one"""
    assert not _failed, f"not started: an earlier run of view_order_check failed ({_failed[0]})"
    exe = os.path.join(ROOT, "build", "view_order_check")
    subprocess.run(["make", "-s", "build/view_order_check"], cwd=ROOT, check=True)
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    cases.write(src)
    try:
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _failed.append("timeout")
        raise
    if out.returncode != 0:
        _failed.append(f"exit {out.returncode}")
    assert out.returncode == 0, f"view_order_check exited with {out.returncode}: {out.stdout}{out.stderr}"
    return C.Results(dst)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} elements, expected {want.shape}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:6].tolist()}: got {got[bad[:6]].tolist()}, expected {want[bad[:6]].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- tile orders
@pytest.mark.parametrize("geom", C.TILE_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}")
def test_tile_order(geom, tmp_path):
    tx, ty, ns = geom
    n = tx * ty
    cf = C.CaseFile()
    costs = {rec: C.tile_record(tx, ty, ns, rec) for rec in C.TILE_RECORDS}
    for rec in C.TILE_RECORDS:
        cf.tile_order(costs[rec], tx, ns)
    res = _run(cf, tmp_path)
    used = ns * 64 * C.tile_order_workgroups(n, ns)
    for rec in C.TILE_RECORDS:
        name = C.tile_name(tx, ty, ns, rec)
        want_order, want_cost = V.tile_order(costs[rec], tx, ty, ns, C.FILL_I32)
        cost = res.guarded(np.int32, name + ": cost")
        order = res.guarded(np.int32, name + ": order")
        scratch = res.guarded(np.int32, name + ": scratch")
        _same(cost, want_cost, name + ": cost is cleared")
        _same(np.sort(order[:n]), np.arange(n), name + ": the order is a permutation of the tiles")
        _same(order[:n], want_order[:n], name + ": order")
        _same(order[n:], want_order[n:], name + ": class tables (untouched dwords keep the fill)")
        _same(scratch[used:], np.full(scratch.size - used, C.FILL_I32), name + ": scratch beyond the workgroups' counts")
    assert res.done()


# ---------------------------------------------------------------------------------------------------------------- pixel lists
def _check_px(res, name, g, rec, pol):
    got_rec = res.guarded(np.uint8, name + ": record")
    lst = res.guarded(np.uint32, name + ": list")
    hdr = res.guarded(np.int32, name + ": header")
    scratch = res.guarded(np.int32, name + ": scratch")
    _same(got_rec, rec, name + ": the record is only read")
    _same(np.sort(lst), np.sort((np.arange(g.rows_local, dtype=np.uint32)[:, None] << 16 | np.arange(g.w, dtype=np.uint32)[None, :]).ravel()),
          name + ": the list is a permutation of the part's pixels")
    _same(lst, V.px_list(rec, g), name + ": list")
    _same(hdr, V.px_header(V.px_histogram(rec, g), pol, C.FILL_I32), name + f": header ({pol})")
    counts = 64 * V.px_workgroups(g.ntiles)[1]
    _same(scratch[counts:64 * 2048], np.full(64 * 2048 - counts, C.FILL_I32), name + ": scratch between the counts and the totals")
    _same(scratch[64 * 2048 + 128:], np.full(128, C.FILL_I32), name + ": scratch behind the bins' totals and first positions")


@pytest.mark.parametrize("gname", C.PX_GEOM_NAMES)
def test_pixel_list(gname, tmp_path):
    g = C.px_geoms()[gname]
    cf = C.CaseFile()
    recs = {rec: C.px_record(gname, g, rec) for rec in C.PX_RECORDS}
    for rec in C.PX_RECORDS:
        cf.px_order(recs[rec], g, C.DEFAULT_POLICY)
    res = _run(cf, tmp_path)
    for rec in C.PX_RECORDS:
        _check_px(res, C.px_name(gname, rec), g, recs[rec], C.DEFAULT_POLICY)
    assert res.done()


def test_pixel_list_header_policies(tmp_path):
    g = C.px_geoms()[C.POLICY_GEOM]
    cf = C.CaseFile()
    recs = {rec: C.px_record(C.POLICY_GEOM, g, rec) for rec in C.POLICY_RECORDS}
    pols = C.px_policies()
    for rec in C.POLICY_RECORDS:
        for pol in pols.values():
            cf.px_order(recs[rec], g, pol)
    res = _run(cf, tmp_path)
    for rec in C.POLICY_RECORDS:
        for pname, pol in pols.items():
            _check_px(res, C.px_name(C.POLICY_GEOM, rec, pname), g, recs[rec], pol)
    assert res.done()


# ---------------------------------------------------------------------------------------------------------------- first orders
def test_first_order(tmp_path):
    cf = C.CaseFile()
    for tx, ty in C.FIRST_GEOMS:
        cf.first_order(tx, ty)
    res = _run(cf, tmp_path)
    for tx, ty in C.FIRST_GEOMS:
        name = f"first order {tx}x{ty}"
        order = res.guarded(np.int32, name + ": order")
        res.guarded(np.int32, name + ": rank scratch")
        _same(np.sort(order[:tx * ty]), np.arange(tx * ty), name + ": a permutation of the tiles")
        _same(order, V.first_order(tx, ty), name)
    assert res.done()


# ---------------------------------------------------------------------------------------------------------------- views
SCENES = {"rgbbox": "rgbbox", "irreg": "irreg", "random600": E.SCENES["random600"]}
# the model's cadences set by name, so that the expected header does not depend on where the plan puts the scene: both of sort_view's tables
G_OF = {"rgbbox": C.G_LDS, "irreg": C.G_L2, "random600": C.G_LDS}
# name -> (scene, h, w, max_depth, entry, rows_per_tile, part, nparts, extra options)
VIEWS = {
    "rgbbox 8x8": ("rgbbox", 8, 8, 50, 0, 8, 0, 1, ()),
    "rgbbox 77x53": ("rgbbox", 53, 77, 50, 0, 8, 0, 1, ()),
    "rgbbox 200x200": ("rgbbox", 200, 200, 50, 0, 8, 0, 1, ()),
    "irreg 256x256": ("irreg", 256, 256, 50, 0, 8, 0, 1, ()),
    "random600 96x72": ("random600", 72, 96, 50, 0, 8, 0, 1, ()),
    "rgbbox 77x53 max_depth 3": ("rgbbox", 53, 77, 3, 0, 8, 0, 1, ()),
    "rgbbox 77x53 part 1 of 3": ("rgbbox", 53, 77, 50, 1, 8, 1, 3, ()),
    "rgbbox 77x53 part 1 of 3 in place": ("rgbbox", 53, 77, 50, 2, 8, 1, 3, ()),
    "irreg 256x256 part 1 of 3 in place": ("irreg", 256, 256, 50, 2, 16, 1, 3, ()),
    "rgbbox 200x200 waves_per_wg 8": ("rgbbox", 200, 200, 50, 0, 8, 0, 1, (("waves_per_wg", 8),)),
}


@functools.lru_cache(maxsize=None)
def _chains(scene, h, w, depth):
    if scene == "random600":
        s7, lf, la, fov = E.SCENES["random600"]
        orc = O.OracleScene("custom", spheres7=s7, look_from=lf, look_at=la, fov=fov)
    else:
        orc = O.OracleScene(scene)
    n = orc.chain_lengths(h, w, max_depth=depth)
    n.setflags(write=False)
    return n


def _frame(res):
    meta = res.block(np.int32)
    keys = ("ntiles", "nshards", "px_elems", "rec_out_skip", "cost_px_bytes", "num_cu", "valid", "px_valid", "tiles_x", "tiles_y", "rows_local", "px_solo")
    f = dict(zip(keys, (int(x) for x in meta)))
    f["launch"] = bytes(res.block()).decode()
    f["cost"], f["order"], f["cost_px"], f["list"] = res.block(np.int32), res.block(np.int32), res.block(np.uint8), res.block(np.uint32)
    return f


def _view_expectation(name):
    scene, h, w, depth, entry, rpt, part, nparts, _ = VIEWS[name]
    rows = np.arange(h) if entry == 0 else C.part_rows(h, rpt, part, nparts)
    chains = _chains(scene, h, w, depth)[rows]
    g = V.PxGeom(w, len(rows), rpt.bit_length() - 1, (nparts - 1) * rpt * w if entry == 2 else 0)
    cost_px, cost = V.view_records(chains, w)
    return g, cost_px, cost


def _check_records(name, f, g, cost_px, cost):
    assert (f["ntiles"], f["tiles_x"], f["tiles_y"], f["rows_local"]) == (g.ntiles, g.tiles_x, g.tiles_y, g.rows_local), name
    assert "recording=2" in f["launch"], f"{name}: {f['launch']}"
    lrow, col = np.divmod(np.arange(g.npix, dtype=np.int64), g.w)
    _same(f["cost_px"][g.record_index(lrow, col)], cost_px.ravel(), name + ": cost_px == min(chain length, 255)")
    return lrow, col


def _check_sorted(name, f, g, cost_px, cost, view=None):
    """order, class table, list and header == the restatement applied to the record"""
    n = g.ntiles
    assert f["valid"] == 1 and f["px_valid"] == 1 and f["px_elems"] == g.npix and f["rec_out_skip"] == g.out_skip, f"{name}: {f}"
    _same(f["cost"], np.zeros(n, np.int32), name + ": cost is cleared by the sort")
    ns = f["nshards"]
    want = V.tile_order(cost, g.tiles_x, g.tiles_y, ns, C.FILL_I32)[0]
    _same(f["order"][:n], want[:n], name + ": order")
    for s in range(ns):
        _same(f["order"][n + 16 * s:n + 16 * s + 9], want[n + 16 * s:n + 16 * s + 9], name + f": class table of shard {s}")
    rec = np.full(g.record_bytes(), C.POISON, np.uint8)
    lrow, col = np.divmod(np.arange(g.npix, dtype=np.int64), g.w)
    rec[g.record_index(lrow, col)] = cost_px.ravel()
    lst = f["list"][:g.npix]
    _same(np.sort(lst), np.sort(((lrow << 16) | col).astype(np.uint32)), name + ": the list is a permutation of the part's pixels")
    _same(lst, V.px_list(rec, g), name + ": list")
    # the policy sort_view hands to the sort: the default cuts by the model, the cadences the case set by name, every persistent workgroup's waves (one
    # workgroup per CU, a multiple of 8 of them), the one-pixel class capped at a quarter of the waves where the list was cut with one
    waves = int(re.search(r"waves=(\d+)", f["launch"]).group(1))
    nwaves = (f["num_cu"] - f["num_cu"] % 8) * waves
    pol = V.PxPolicy((0, 24, 14, 9), G_OF[VIEWS[view or name][0]], 250, nwaves, nwaves // 4 if f["px_solo"] else 0, 1)
    _same(f["list"][g.npix:].view(np.int32), V.px_header(V.px_histogram(rec, g), pol, 0), name + f": header ({pol})")


def _view_options(name, eager):
    scene = VIEWS[name][0]
    opts = [("pixel_order", 2), ("eager_sort", eager), ("px_solo_div", 4)]
    opts += [(k, v) for k, v in zip(("px_g1", "px_g8", "px_g16", "px_g32", "px_g64"), G_OF[scene])]
    return opts + list(VIEWS[name][8])


@pytest.mark.parametrize("name", list(VIEWS))
def test_view_records_then_sorts(name, tmp_path):
    """eager_sort = 0: frame 1 leaves the record, frame 2's sorts turn exactly that record into the view's tables.
    (Chains cut off by max_depth are recorded with the rays traced, max_depth of them: the oracle's count.)"""
    scene, h, w, depth, entry, rpt, part, nparts, _ = VIEWS[name]
    cf = C.CaseFile()
    cf.view(SCENES[scene], h, w, depth, entry, rpt, part, nparts, 2, _view_options(name, 0))
    res = _run(cf, tmp_path)
    g, cost_px, cost = _view_expectation(name)
    f1, f2 = _frame(res), _frame(res)
    assert res.done()
    _check_records(name + ", frame 1", f1, g, cost_px, cost)
    _same(f1["cost"], cost, name + ", frame 1: cost == the tile's longest chain if >= 3, else 0")
    assert f1["valid"] == 0 and "recording=0" in f2["launch"], f"{name}: {f2['launch']}"
    if "waves_per_wg" in name:
        assert "DONATE" not in f1["launch"] and "waves=8" in f1["launch"], f1["launch"]
    # frame 2's tables from what was READ after frame 1
    lrow, col = np.divmod(np.arange(g.npix, dtype=np.int64), g.w)
    _check_sorted(name + ", frame 2", f2, g, f1["cost_px"][g.record_index(lrow, col)].reshape(g.rows_local, g.w), f1["cost"], view=name)


@pytest.mark.parametrize("name", list(VIEWS))
def test_view_eager_sort_after_one_frame(name, tmp_path):
    """eager_sort = 1 on a fresh prepared scene: the same tables behind frame 1 alone"""
    scene, h, w, depth, entry, rpt, part, nparts, _ = VIEWS[name]
    cf = C.CaseFile()
    cf.view(SCENES[scene], h, w, depth, entry, rpt, part, nparts, 1, _view_options(name, 1))
    res = _run(cf, tmp_path)
    g, cost_px, cost = _view_expectation(name)
    f1 = _frame(res)
    assert res.done()
    _check_records(name, f1, g, cost_px, cost)
    _check_sorted(name, f1, g, cost_px, cost)


def test_view_with_strips_of_zero_width(tmp_path):
    """xcd_queues = 1 on a frame 24 pixels wide: the host lays the view's order table out for eight strips of the three tile columns, five of them
    empty (the premise of the 3 x 5 and 3 x 125 grids above).  Such a view has no pixel list: frame 1 records the tiles' chains only, frame 2's
    sort leaves eight segments and eight class tables."""
    h, w = 40, 24
    cf = C.CaseFile()
    cf.view("irreg", h, w, 50, 0, 8, 0, 1, 2, [("xcd_queues", 1), ("eager_sort", 0)])
    res = _run(cf, tmp_path)
    f1, f2 = _frame(res), _frame(res)
    assert res.done()
    _, cost = V.view_records(_chains("irreg", h, w, 50), w)
    assert (f1["nshards"], f1["tiles_x"], f1["tiles_y"], f1["ntiles"]) == (8, 3, 5, 15), f1
    assert sorted(s[1] for s in V.strips(3, 5, 8)) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert "recording=1" in f1["launch"] and "counters=8" in f1["launch"] and "(turns)" not in f1["launch"], f1["launch"]
    _same(f1["cost"], cost, "frame 1: cost == the tile's longest chain if >= 3, else 0")
    assert cost.any(), "some tile has a chain of >= 3 rays"
    assert f2["valid"] == 1 and f2["nshards"] == 8 and "recording=0" in f2["launch"], f2["launch"]
    want = V.tile_order(f1["cost"], 3, 5, 8, C.FILL_I32)[0]
    _same(f2["order"][:15], want[:15], "frame 2: order")
    for s in range(8):
        _same(f2["order"][15 + 16 * s:15 + 16 * s + 9], want[15 + 16 * s:15 + 16 * s + 9], f"frame 2: class table of strip {s}")
    _same(f2["cost"], np.zeros(15, np.int32), "frame 2: cost is cleared by the sort")
