"""The trimmed ENTRY kernels of the pooled family on the GPU: the kernel that starts primary rays at their tile's entry list has the
leaf filter and the dark stop compiled in, reads the winner's colour from LDS where the colour table fits next to 16 waves, and a view keeps its
table of entry lists between its launches.  Every image is the oracle's, bit for bit.  What the launch line has no field for -- the colour's
source, whether the flags were compile-time constants, how many tables were built and how many found in place -- comes from
Context.entry_info().  (sync_policy = 1 throughout: which launch renders a frame is then the same in every run.)"""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_entry_lists_gpu as E
import test_leaf_box_gpu as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


@functools.lru_cache(maxsize=None)
def _exe():
    subprocess.run(["make", "-s", "build/batch_trim_check"], cwd=ROOT, check=True)
    return os.path.join(ROOT, "build", "batch_trim_check")


@functools.lru_cache(maxsize=None)
def _tool(*args):
    _exe()
    out =subprocess.run([os.path.join(ROOT, "build", "batch_trim_check"), *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout)}


def _batch(R, c, ps, h, w, wants, what, settled=False, **kw):
    """a batch of len(wants) frames against the oracle's images; returns the launch line.  `settled`: the batch is launched twice and the second launch
    counts -- a view's first batch records its chains (recording=1: no dark stop, so the twin that reads the flags), its later ones do not"""
    import torch
    if settled:
        _batch(R, c, ps, h, w, wants, what + " (the view's first batch)", **kw)
    rows = wants[0].shape[0]
    buf = torch.full((len(wants), rows, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(buf.data_ptr(), h, w, ps, len(wants), frame_stride=rows * w, **kw)
    c.sync()
    ll = c.last_launch
    bad = [int((f != x).sum()) for f, x in zip(buf.cpu().numpy(), wants)]
    print(f"{what}: differing pixels {bad}; {ll}; {c.entry_info()}")
    assert all(b == 0 for b in bad), (what, bad, ll)
    assert not settled or "recording=0" in ll, ll
    return ll


def _frame(R, c, ps, h, w, want, what, **kw):
    import torch
    out = torch.full(want.shape, -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_into(out.data_ptr(), h, w, ps, **kw)
    c.sync()
    ll = c.last_launch
    bad = int((out.cpu().numpy() != want).sum())
    print(f"{what}: differing pixels {bad}; {ll}; {c.entry_info()}")
    assert bad == 0, (what, bad, ll)
    return ll


# ------------------------------------------------------------------------------------------------ lists exactly when all three are on
@pytest.mark.parametrize("h,w", [(64, 64), (192, 192), (136, 200), (61, 83)])
def test_lists_exactly_when_the_filter_the_dark_stop_and_the_lists_are_on(R, h, w):
    """batches of 2 and 3 frames of rgbbox under dark_stop x leaf_box x entry_lists in {-1, 0}: the launch says entry=lists exactly when all three
    are on -- the kernel with lists has the two flags compiled in -- and then, unless it records, reads its colours from LDS (rgbbox's 400 fit);
    (61, 83) cuts tiles at both edges.  One context: the options are read per launch, and the view's kept table is rebuilt whenever the filter it was built under changes"""
    want = E._want("rgbbox", h, w)
    c = L._ctx(R)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    for nframes, (dark, leaf, lists) in itertools.product((2, 3), itertools.product((-1, 0), repeat=3)):
        for k, v in (("dark_stop", dark), ("leaf_box", leaf), ("entry_lists", lists)):
            c.set_option(k, v)
        ll = _batch(R, c, ps, h, w, [want] * nframes, f"rgbbox {w}x{h} x{nframes} dark_stop={dark} leaf_box={leaf} entry_lists={lists}")
        on = (dark, leaf, lists) == (-1, -1, -1)
        assert E._entry(ll) == on, (dark, leaf, lists, ll)
        assert (dark != 0 or ",dark=0," in ll) and L._leaf(ll) == (leaf != 0), ll
        # (the view's first batch records its chains, so it runs without the dark stop: lists through the twin that reads the flags, colours from memory)
        const = on and ll.endswith(",dark=1,leaf_box=1")
        assert const == (on and "recording=0" in ll), ll
        info = c.entry_info()
        assert (info["flags_const"], info["colour_lds"]) == (const, const), (info, ll)
    c.close()


@pytest.mark.parametrize("leaf_box,lists", [(-1, -1), (0, 1)])
def test_the_counting_twins_still_add_up(R, tmp_path, leaf_box, lists):
    """rgbbox 64 x 64, two frames, option entry_count: lists + fallbacks = 64 x (tiles the CPU gives a list) x frames, through the twin with the flags
    compiled in (everything at its default) and, with entry_lists = 1 and the filter off, through the twin that reads them: 3 968 + 0"""
    h = w = 64
    c = L._ctx(R, entry_count=1, leaf_box=leaf_box, entry_lists=lists)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    ll = _batch(R, c, ps, h, w, [E._want("rgbbox", h, w)] * 2, f"rgbbox counted, leaf_box={leaf_box} entry_lists={lists}", settled=True)
    assert E._entry(ll) and L._leaf(ll) == (leaf_box != 0), ll
    info, n = c.entry_info(), c.entry_counts()
    assert info["flags_const"] == (leaf_box != 0), (info, ll)
    tiles, _ = E._cpu_lists(tmp_path, "rgbbox", h, w, L._leaf(ll))
    print(f"tiles with a list {tiles}; device {n['lists']} + {n['fallbacks']} over {n['waves']} waves")
    assert n["waves"] > 0 and n["lists"] + n["fallbacks"] == 64 * tiles * 2 and n["fallbacks"] == 0, (n["lists"], n["fallbacks"], tiles)
    if leaf_box == 0:
        assert (n["lists"], n["fallbacks"]) == (3968, 0), n
    c.close()


# ------------------------------------------------------------------------------------------------ the colour table: shorter than a wave, and too long
def _grid(n, spacing=1.1, radius=0.5):
    """n spheres on a square grid in the plane z = 0, every one visible from the z axis, every one its own colour"""
    m = int(np.ceil(np.sqrt(n)))
    i, j = np.divmod(np.arange(n), m)
    s = np.zeros((n, 7), F)
    s[:, 0] = (i - (m - 1) / 2) * spacing
    s[:, 1] = (j - (m - 1) / 2) * spacing
    s[:, 3:6] = np.linspace(0.2, 1.0, 3 * n, dtype=F).reshape(-1, 3)
    s[:, 6] = radius
    return s


def _plan16(n, height):
    """api.cpp's make_plan restated for a scene that may live in LDS whole under 16 waves: the ray table keeps its {d} plane (3 planes) if the scene
    then still fits, else 2 planes; None: no 16-wave shape holds the scene.  A wave's bytes and the colour layout's come from the library's own
    formulas (tools/batch_trim_check.cpp)."""
    capb, capl = 64 * (height + 3), 192
    for planes in (3, 2):
        t = _tool("colbytes", n - 1, n, capb, capl, planes)
        if 64 * (n - 1) + 16 * n <= LDS_LIMIT - 16 * t["wave"] - 512:
            return planes, t["bytes"]
    return None


def _too_many(R, c, h, w, look_from, fov):
    """the largest grid whose scene lives in LDS under 16 waves while its colour table does NOT fit beside them"""
    for n in range(640, 200, -6):
        s = _grid(n)
        ps = R.prepare_scene_from_spheres(c, s, h, w, look_from, (0.0, 0.0, 0.0), fov)
        plan = _plan16(n, ps.height)
        if plan is not None and plan[1] > LDS_LIMIT:
            return n, s, ps, plan
        ps.free()
    raise AssertionError("no grid of 200 .. 640 spheres lives in LDS under 16 waves with a colour table that does not fit")


def test_the_colour_table_from_two_spheres_to_too_many(R):
    """two spheres and 33 (a table shorter than a wave; the last index wins somewhere: every sphere of the grid is seen), rgbbox's 400, and a grid
    so large that col[n] does not fit beside 16 waves: the launch keeps all 16 waves and loads its colours from memory.  The oracle's image either way"""
    h, w = 64, 72
    c = L._ctx(R)
    # (the two spheres of the entry-list tests through THEIR camera, which the leaf filter's camera guard refuses: the launch runs unfiltered, so its lists go
    # through the twin that reads the flags, and that one loads its colours from memory)
    ps = R.prepare_scene(40, 56, E._scene(c, "two"))
    ll = _batch(R, c, ps, 40, 56, [E._want("two", 40, 56)] * 2, "two spheres, the far camera", settled=True)
    assert not L.camera_ok(L.guards(E.SCENES["two"][0]), E._orc("two").camera_floats(40, 56))
    info = c.entry_info()
    assert E._entry(ll) and not L._leaf(ll) and (info["flags_const"], info["colour_lds"]) == (False, False), (ll, info)
    ps.free()
    seen = []
    for what, n in (("two spheres", 2), ("33 spheres", 33), ("too many", None)):
        # (cameras inside the filter's camera guard)
        lf, fov = ((0.0, 0.5, 3.0), 80.0) if n == 2 else ((0.0, 0.0, 4.5), 90.0) if n == 33 else ((0.0, 0.0, 16.0), 75.0)
        if n is None:
            n, s, ps, plan = _too_many(R, c, h, w, lf, fov)
            print(f"too many: n = {n}, tree height {ps.height}, {plan[0]} ray planes, the colour layout would take {plan[1]} of {LDS_LIMIT} bytes")
        else:
            s = E.SCENES["two"][0] if n == 2 else _grid(n)
            ps = R.prepare_scene_from_spheres(c, s, h, w, lf, (0.0, 0.0, 0.0), fov)
            plan = _plan16(n, ps.height)
            assert plan is not None and plan[1] <= LDS_LIMIT, plan
        orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=(0.0, 0.0, 0.0), fov=fov)
        assert L.camera_ok(L.guards(s), orc.camera_floats(h, w)), what       # (the leaf filter is on: the launch may start at lists)
        want, _ = orc.render(h, w)
        ll = _batch(R, c, ps, h, w, [want] * 3, what, settled=True)
        info = c.entry_info()
        assert E._entry(ll) and "waves=16" in ll and "nodes=sign-ordered" in ll and info["flags_const"], (what, ll, info)
        assert info["colour_lds"] == (plan[1] <= LDS_LIMIT), (what, plan, info)
        c.set_option("col_lds", 0)
        ll = _batch(R, c, ps, h, w, [want] * 3, what + ", col_lds = 0")
        assert E._entry(ll) and not c.entry_info()["colour_lds"], (ll, c.entry_info())
        c.set_option("col_lds", -1)
        seen.append(info["colour_lds"])
        ps.free()
    assert seen == [True, True, False], seen
    c.close()


def test_the_last_sphere_wins_somewhere(R):
    """33 spheres, one colour each: the first hits of the frame's primary rays (rt_intersect_rays over rt_camera_rays) name every index 0 .. 32 -- so
    the last entry of the 33-entry table in LDS is read by some fold's winner -- and the image is the oracle's"""
    h, w = 64, 72
    s = _grid(33)
    lf, fov = (0.0, 0.0, 4.5), 90.0
    orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=(0.0, 0.0, 0.0), fov=fov)
    assert L.camera_ok(L.guards(s), orc.camera_floats(h, w))
    want, _ = orc.render(h, w)
    c = L._ctx(R)
    ps = R.prepare_scene_from_spheres(c, s, h, w, lf, (0.0, 0.0, 0.0), fov)
    idx, _ = R.intersect_rays(ps, R.camera_rays(ps, h, w))
    winners = set(int(i) for i in np.unique(idx) if i >= 0)
    assert winners == set(range(33)), sorted(winners)
    ll = _batch(R, c, ps, h, w, [want] * 2, "33 spheres", settled=True)
    assert E._entry(ll) and c.entry_info()["colour_lds"], (ll, c.entry_info())
    c.close()


# ------------------------------------------------------------------------------------------------ a view keeps its table
def _cams(orc, h, w, k, step):
    cams = np.tile(orc.camera_floats(h, w), (k, 1))
    cams[:, 0] += F(step) * np.arange(1, k + 1, dtype=F)
    cams[:, 1] -= F(0.5 * step) * np.arange(1, k + 1, dtype=F)
    return cams


def test_a_view_keeps_its_table(R):
    """the same view three times: one table built, then found in place twice.  A scene update (a sphere moved across a tile boundary) resets the views:
    the next render builds again and is the oracle's image of the NEW scene.  Other cameras are other views (single frames here: a batch through another
    camera has no view; handover / pixel_order / solo at 0 make a view's later frames launches of the plain kernel, which has lists): each builds its own
    table once, and a ninth view evicts the least recently used one, whose table is built again when it comes back"""
    import torch
    h = w = 64
    s = L._wall()
    lf, la, fov = (0.0, 0.0, 12.0), (0.0, 0.0, 0.0), 75.0             # (inside the leaf filter's camera guard: the default policy wants the filter)
    orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)
    assert L.camera_ok(L.guards(s), orc.camera_floats(h, w))
    want, _ = orc.render(h, w)
    c = L._ctx(R, handover=0, pixel_order=0, solo=0)
    ps = R.prepare_scene_from_spheres(c, torch.from_numpy(s).cuda(), h, w, lf, la, fov)
    base = c.entry_info()
    assert (base["tables_built"], base["tables_kept"]) == (0, 0), base

    def counts():
        i = c.entry_info()
        return i["tables_built"], i["tables_kept"]

    for k in range(3):
        ll = _batch(R, c, ps, h, w, [want] * 2, f"the view, launch {k + 1}")
        assert E._entry(ll) and L._leaf(ll), ll
        assert counts() == (1, k), (k, counts())
    # entry_keep = 0: the launch builds its table in the context's buffer; the view's stays as it is for the launch after
    c.set_option("entry_keep", 0)
    _batch(R, c, ps, h, w, [want] * 2, "entry_keep = 0")
    assert counts() == (2, 2), counts()
    c.set_option("entry_keep", -1)
    _batch(R, c, ps, h, w, [want] * 2, "entry_keep back on")
    assert counts() == (2, 3), counts()
    # the filter changes: the table is built again under the new one (entry_lists = 1: a launch without the filter keeps its lists)
    c.set_option("entry_lists", 1)
    c.set_option("leaf_box", 0)
    ll = _batch(R, c, ps, h, w, [want] * 2, "leaf_box = 0, entry_lists = 1")
    assert E._entry(ll) and not L._leaf(ll) and counts() == (3, 3), (ll, counts())
    c.set_option("leaf_box", -1)
    c.set_option("entry_lists", -1)
    _batch(R, c, ps, h, w, [want] * 2, "the filter back on")
    assert counts() == (4, 3), counts()
    _batch(R, c, ps, h, w, [want] * 2, "... and kept")
    assert counts() == (4, 4), counts()

    # two spheres move by more than a tile (8 pixels are 2.3 units here)
    s2 = s.copy()
    s2[0, 0] += F(3.1)
    s2[17, 1] -= F(3.4)
    orc2 = O.OracleScene("custom", spheres7=s2, look_from=lf, look_at=la, fov=fov)
    want2, _ = orc2.render(h, w)
    assert int((want2 != want).sum()) > 0
    ps.update_spheres(torch.from_numpy(s2).cuda())
    ll = _batch(R, c, ps, h, w, [want2] * 2, "after the update")
    assert E._entry(ll) and counts() == (5, 4), (ll, counts())
    _batch(R, c, ps, h, w, [want2] * 2, "after the update, again")
    assert counts() == (5, 5), counts()

    # other cameras: single frames, three per view.  The model: a view that says entry=lists builds iff it has no table yet
    have, lru = {"prepared"}, ["prepared"]
    cams = _cams(orc2, h, w, 9, 0.06)
    assert all(L.camera_ok(L.guards(s2), cam) for cam in cams)
    lists_seen = 0

    def touch(key):
        if key in lru:
            lru.remove(key)
        elif len(lru) == 8:
            have.discard(lru.pop(0))
        lru.append(key)

    for v, cam in enumerate(cams[:1].tolist() + [None] + cams.tolist()):
        key = "prepared" if cam is None else tuple(cam)
        w_v = want2 if cam is None else orc2.render(h, w, cam=np.array(cam, F))[0]
        for k in range(3):
            built, kept = counts()
            if cam is None:
                ll = _batch(R, c, ps, h, w, [w_v] * 2, f"view {v} (the prepared camera), launch {k + 1}")
            else:
                ll = _frame(R, c, ps, h, w, w_v, f"view {v}, frame {k + 1}", cam=np.array(cam, F))
            touch(key)
            if E._entry(ll):
                lists_seen += cam is not None
                assert counts() == ((built, kept + 1) if key in have else (built + 1, kept)), (v, k, key in have, built, kept, counts(), ll)
                have.add(key)
            else:
                assert counts() == (built, kept), (v, k, counts(), ll)
    assert lists_seen >= 9, lists_seen                       # (every view's later frames did start at lists)
    # nine other views have been rendered since: the prepared camera's view was evicted, and its table with it
    assert "prepared" not in have
    built, kept = counts()
    ll = _batch(R, c, ps, h, w, [want2] * 2, "the evicted view comes back")
    assert E._entry(ll) and counts() == (built + 1, kept), (ll, counts())
    c.close()


# ------------------------------------------------------------------------------------------------ no view: parts, a camera per frame
def test_a_part_launch_and_a_camera_per_frame(R):
    """part 1 of 2 with row tiles of 8 (a view of its own, table kept), and batches with a camera per frame (no view: a list per frame and tile, built
    by every launch; the tiles of different frames hold different lists)"""
    h, w = 136, 200
    c = L._ctx(R)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    want = E._want("rgbbox", h, w)
    rows = L.VC.part_rows(h, 8, 1, 2)
    for k in range(2):
        ll = _batch(R, c, ps, h, w, [want[rows]] * 3, f"part 1 of 2, launch {k + 1}", part=1, nparts=2, rows_per_tile=8)
        assert E._entry(ll), ll
        i = c.entry_info()
        assert (i["tables_built"], i["tables_kept"], i["colour_lds"]) == (1, k, k == 1), i      # (the first batch records: colours from memory)
    orc = E._orc("rgbbox")
    cams = _cams(orc, h, w, 3, 0.35)
    wants = [E._want("rgbbox", h, w, tuple(float(x) for x in cam)) for cam in cams]
    for k in range(2):
        ll = _batch(R, c, ps, h, w, wants, f"a camera per frame, launch {k + 1}", cams=cams)
        i = c.entry_info()
        assert E._entry(ll) == (E._allowed(ll, -1, cams=True) and ll.endswith("dark=1,leaf_box=1")), ll
        assert (i["tables_built"], i["tables_kept"]) == (2 + k if E._entry(ll) else 1, 1), (i, ll)
    c.close()
