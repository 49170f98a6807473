"""Per-tile entry lists on the GPU (lane_core.h: tile_entry): a new primary ray of the ENTRY instantiations starts at its tile's
list -- at most one inner node and six leaves that every ray of the tile provably reaches -- instead of at the root.  Every image is the
oracle's, bit for bit, with option entry_lists at 0, 1 and its default: batches of rgbbox (16 waves, the scene in LDS, sign-ordered records),
of irreg and of a 6 400-sphere floor (read from L2 in the twenty-wave shape, CULL and not: no ENTRY kernel, always the root), at frame sizes that cut tiles at both edges, a
camera per frame, parts of a cyclic partition, cameras on an axis (tiles whose direction components change sign get no list) and inside the
scene.  rt_context_last_launch says "entry=lists" exactly where the policy allows it, and that policy is restated here from the launch's
other tokens, not asked of the library.  Images are the same with and without lists by design, so the counting twin of the kernel (option
entry_count) says what the device did: how many primary rays started from a list and how many were sent back to the root because their
wave's leaf list had no room -- against the tiles tools/entry_check.cpp gives a list on the CPU.  (sync_policy = 1 throughout: which launch renders a frame is then the same in every run.)"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_leaf_box_gpu as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIZES = [(64, 64), (200, 200), (29, 37), (1, 1), (8, 8)]


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


def _two():
    """two spheres: the root's children are both leaves"""
    s = np.zeros((2, 7), F)
    s[0] = (-1.2, 0.0, 0.0, 0.9, 0.3, 0.3, 1.0)
    s[1] = (1.2, 0.0, 0.0, 0.3, 0.3, 0.9, 1.0)
    return s, (0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 50.0


SCENES = dict(L.SCENES, two=_two(), wall=(L._wall(), (0.0, 0.0, 30.0), (0.0, 0.0, 0.0), 40.0))


@functools.lru_cache(maxsize=None)
def _orc(name):
    if name in L.NAMED:
        return O.OracleScene(name)
    s, lf, la, fov = SCENES[name]
    return O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)


@functools.lru_cache(maxsize=None)
def _want(name, h, w, cam=None):
    img, _ = _orc(name).render(h, w, cam=None if cam is None else np.array(cam, F))
    img.setflags(write=False)
    return img


def _scene(c, name):
    if name in L.NAMED:
        return c.scene(name)
    s, lf, la, fov = SCENES[name]
    return c.scene_from_spheres(s, lf, la, fov)


def _entry(ll):
    m = re.search(r" nodes=[a-z-]+,entry=(lists|root),dark=[01],leaf_box=[01]$", ll)
    assert m, ll
    return m.group(1) == "lists"


def _allowed(ll, option, rows_per_tile=8, nparts=1, cams=False):
    """api.cpp's policy (set_entry) from the launch's other tokens: the instantiation exists with ENTRY -- plain tile tickets on 16 waves with the
    scene in LDS (sign-ordered records); the kernels that read the scene from L2 were slower with lists and have none.  A launch with a camera
    per frame finds its lists at the ticket positions, so only without an order table and with one queue over all tiles; the default
    additionally wants tiles of 8 consecutive image rows"""
    tok = dict(t.split("=", 1) for t in ll.split(" ")[1:] if "=" in t)
    if option == 0:
        return False
    if option < 0 and nparts > 1 and rows_per_tile < 8:
        return False
    waves, inst, nodes = int(tok["waves"]), tok["instantiation"], tok["nodes"].split(",")[0]
    one_queue = tok["counters"] == "1" or tok["counters"].endswith("(turns)")
    if cams and not (tok["tickets"] == "tiles-raster" and one_queue):
        return False
    return waves == 16 and inst == "plain" and nodes == "sign-ordered"


def _batch(R, c, ps, h, w, wants, what, option, **kw):
    import torch
    rows = wants[0].shape[0]
    buf = torch.full((len(wants), rows, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(buf.data_ptr(), h, w, ps, len(wants), frame_stride=rows * w, **kw)
    c.sync()
    ll = c.last_launch
    bad = [int((f != x).sum()) for f, x in zip(buf.cpu().numpy(), wants)]
    print(f"{what}: differing pixels {bad}; {ll}")
    assert all(b == 0 for b in bad), (what, bad, ll)
    assert _entry(ll) == _allowed(ll, option, kw.get("rows_per_tile", 8), kw.get("nparts", 1), "cams" in kw), (what, option, ll)
    return ll


def _frame(R, c, ps, h, w, want, what, option, **kw):
    import torch
    out = torch.full(want.shape, -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_into(out.data_ptr(), h, w, ps, **kw)
    c.sync()
    ll = c.last_launch
    bad = int((out.cpu().numpy() != want).sum())
    print(f"{what}: differing pixels {bad}; {ll}")
    assert bad == 0, (what, bad, ll)
    if ll.startswith("family=pooled tickets"):
        assert _entry(ll) == _allowed(ll, option, kw.get("rows_per_tile", 8), kw.get("nparts", 1)), (what, option, ll)
    return ll


# ------------------------------------------------------------------------------------------------ the frames, every setting of the option
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("name,opts", [("rgbbox", {}), ("irreg", dict(wide_waves=2)), ("floor", dict(wide_waves=2, cull=1))])
def test_batches_with_the_option_off_on_and_default(R, name, opts, h, w):
    """a batch of three frames of one view (its first batch records nothing: a batch has no view order without adaptive frames before it) and a
    batch with a camera per frame, under entry_lists = 0, 1 and -1; the launches that may start at lists say so"""
    orc = _orc(name)
    want = _want(name, h, w)
    cams = np.tile(orc.camera_floats(h, w), (3, 1))
    cams[:, 0] += F(0.4) * np.arange(3, dtype=F)
    cams[:, 1] -= F(0.2) * np.arange(3, dtype=F)
    wants = [_want(name, h, w, tuple(float(x) for x in cam)) for cam in cams]
    said = []
    for option in (0, 1, -1):
        c = L._ctx(R, entry_lists=option, **opts)
        ps = R.prepare_scene(h, w, _scene(c, name))
        said.append(_entry(_batch(R, c, ps, h, w, wants, f"{name} {w}x{h} entry_lists={option}, a camera each", option, cams=cams)))
        _batch(R, c, ps, h, w, [want] * 3, f"{name} {w}x{h} entry_lists={option}, one camera", option)
        c.close()
    # (rgbbox's launches ARE the ENTRY instantiation's: the option decides alone; the scenes read from L2 always start at the root)
    assert said == ([False, True, True] if name == "rgbbox" else [False] * 3), (name, h, w, said)


def test_three_cameras_against_their_single_renders(R):
    """each frame of a batch with three different cameras is what a single render through that camera gives (and both are the oracle's)"""
    import torch
    h, w = 93, 131
    for name, opts in (("rgbbox", {}), ("irreg", dict(wide_waves=2))):
        orc = _orc(name)
        cams = np.tile(orc.camera_floats(h, w), (3, 1))
        cams[1, 0:3] += np.array([0.7, 0.3, -0.5], F)
        cams[2, 3:6] += np.array([-0.2, 0.1, 0.0], F)
        c = L._ctx(R, entry_lists=1, **opts)
        ps = R.prepare_scene(h, w, _scene(c, name))
        buf = torch.full((3, h, w), -7, dtype=torch.int32, device="cuda")
        R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=h * w, cams=cams)
        c.sync()
        assert _entry(c.last_launch) == (name == "rgbbox"), c.last_launch
        got = buf.cpu().numpy()
        for f, cam in enumerate(cams):
            one = torch.full((h, w), -3, dtype=torch.int32, device="cuda")
            R.render_into(one.data_ptr(), h, w, ps, cam=cam)
            c.sync()
            single = one.cpu().numpy()
            assert int((got[f] != single).sum()) == 0, (name, f)
            assert int((single != _want(name, h, w, tuple(float(x) for x in cam))).sum()) == 0, (name, f)
        c.close()


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("leaf_box", [0, 1])
def test_with_culling_and_the_leaf_filter(R, cull, leaf_box):
    """rgbbox filters its leaves (the list is built under the launch's filter), the floor is culled by the best hit: every combination"""
    for name, h, w, opts in (("rgbbox", 53, 77, {}), ("floor", 120, 160, dict(wide_waves=2)), ("dupes_near", 97, 131, {}), ("tall_fat", 97, 131, {})):
        c = L._ctx(R, entry_lists=1, cull=cull, leaf_box=leaf_box, **opts)
        ps = R.prepare_scene(h, w, _scene(c, name))
        ll = _batch(R, c, ps, h, w, [_want(name, h, w)] * 2, f"{name} cull={cull} leaf_box={leaf_box}", 1)
        if name == "floor":
            assert ("+CULL" in ll) == (cull == 1), ll
        assert L._leaf(ll) == (leaf_box == 1 and name != "floor"), ll
        c.close()


def test_single_frames_and_parts(R):
    """frames of a view (the first is a plain kernel's on rgbbox at this size only if the policy picks it: the assertion follows the launch),
    parts of a cyclic partition with row tiles of 8 and of 2 rows: the default leaves the latter at the root, entry_lists = 1 does not"""
    h, w = 61, 83
    for name, opts in (("rgbbox", {}), ("irreg", dict(wide_waves=2))):
        want = _want(name, h, w)
        for option in (-1, 1):
            c = L._ctx(R, entry_lists=option, **opts)
            ps = R.prepare_scene(h, w, _scene(c, name))
            for k in (1, 2, 3):
                _frame(R, c, ps, h, w, want, f"{name} frame {k} entry_lists={option}", option)
            for rpt in (8, 2):
                rows = L.VC.part_rows(h, rpt, 1, 3)
                ll = _batch(R, c, ps, h, w, [want[rows]] * 2, f"{name} part 1 of 3, row tiles of {rpt}, entry_lists={option}", option, part=1, nparts=3,
                            rows_per_tile=rpt)
                if rpt == 2 and option < 0:
                    assert not _entry(ll), ll
            c.close()


def test_tiles_without_a_list(R):
    """a camera looking exactly down the z axis at a wall of spheres: the centre column's d_x and the centre row's d_y are 0, the tiles around
    them hold both signs (no list: their rays start at the root), every other tile has one; a camera inside the scene's box; two spheres"""
    for name, h, w, cam in (("wall", 64, 64, L._axis_cam(30.0)), ("wall", 37, 29, L._axis_cam(3.0)), ("wall", 64, 64, L._axis_cam(0.5)), ("two", 40, 56, None),
                            ("dupes", 97, 131, None)):
        for option in (0, 1):
            c = L._ctx(R, entry_lists=option)
            ps = R.prepare_scene(h, w, _scene(c, name))
            if cam is None:
                _batch(R, c, ps, h, w, [_want(name, h, w)] * 2, f"{name} {w}x{h} entry_lists={option}", option)
            else:
                cams = np.tile(cam, (2, 1))
                _batch(R, c, ps, h, w, [_want(name, h, w, tuple(float(x) for x in cam))] * 2, f"{name} {w}x{h} axis camera z={cam[2]} entry_lists={option}",
                       option, cams=cams)
            c.close()


# ------------------------------------------------------------------------------------------------ what the device did: the counting twin
def _cpu_lists(tmp_path, name, h, w, filt):
    """tiles that tile_entry gives a list, and the most leaves such a list holds, from the CPU tool over the same records and camera"""
    exe = os.path.join(ROOT, "build", "entry_check")
    subprocess.run(["make", "-s", "build/entry_check"], cwd=ROOT, check=True)
    if name in L.NAMED:
        scene, cam = name, "-"
    else:
        scene, cam = str(tmp_path / f"{name}.f32"), str(tmp_path / f"{name}_cam.f32")
        np.ascontiguousarray(SCENES[name][0], F).tofile(scene)
        _orc(name).camera_floats(h, w).astype(F).tofile(cam)
    out = subprocess.run([exe, "frame", scene, cam, str(h), str(w), str(int(filt))], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    assert (int(f["bound_violations"]), int(f["set_violations"])) == (0, 0), f
    return int(f["packed_lists"]), int(f["packed_leaf_max"])


@pytest.mark.parametrize("name,h,w,leaf_box,falls", [("two", 40, 56, 0, False), ("rgbbox", 64, 64, 0, False), ("rgbbox", 192, 192, 0, True),
                                                     ("rgbbox", 192, 192, 1, False)])
def test_the_device_starts_from_lists_and_falls_back(R, tmp_path, name, h, w, leaf_box, falls):
    """frames of whole tiles only (h, w multiples of 8): every pixel of a tile with a list passes the root test (the root is ALLHIT), so over a
    launch lists + fallbacks = 64 x (tiles with a list) x frames, exactly.  These launches have more waves than positions, so every position is
    some wave's FIRST ticket: an empty wave starts the tile's 64 rays in one SHADE, and their 64 equal lists fit its leaf list of 192 iff they
    hold 3 leaves or fewer -- the launch falls back iff the CPU finds a list of 4 or more (two spheres: 2 leaves; rgbbox 192 x 192 unfiltered:
    5; filtered: 1).  Per-wave words add up."""
    nframes = 2
    c = L._ctx(R, entry_lists=1, entry_count=1, leaf_box=leaf_box)
    ps = R.prepare_scene(h, w, _scene(c, name))
    ll = _batch(R, c, ps, h, w, [_want(name, h, w)] * nframes, f"{name} {w}x{h} leaf_box={leaf_box} counted", 1)
    assert _entry(ll), ll
    n = c.entry_counts()
    tiles, leaf_max = _cpu_lists(tmp_path, name, h, w, L._leaf(ll))
    tok = dict(t.split("=", 1) for t in ll.split(" ")[1:] if "=" in t)
    assert int(tok["grid"]) * int(tok["waves"]) > int(tok["tiles"]) * nframes and n["waves"] == int(tok["grid"]) * int(tok["waves"]), (ll, n["waves"])
    print(f"{name}: longest list {leaf_max} leaves; tiles with a list {tiles} of {(h // 8) * (w // 8)}; device: {n['lists']} from lists, {n['fallbacks']} back to the root, {n['waves']} waves")
    assert n["waves"] > 0 and tiles > 0, n
    assert int(n["per_wave"][:, 0].sum()) == n["lists"] and int(n["per_wave"][:, 1].sum()) == n["fallbacks"], n
    assert n["lists"] + n["fallbacks"] == 64 * tiles * nframes, (n["lists"], n["fallbacks"], tiles)
    assert n["lists"] > 0, n
    assert (64 * leaf_max > 192) == falls, (leaf_max, falls)          # (the case is what it was chosen to be)
    assert (n["fallbacks"] > 0) == falls, n
    c.close()


def test_no_counts_without_a_table(R):
    h, w = 64, 64
    for opts in (dict(entry_lists=0, entry_count=1), dict(entry_lists=1, entry_count=0)):
        c = L._ctx(R, **opts)
        ps = R.prepare_scene(h, w, _scene(c, "rgbbox"))
        _batch(R, c, ps, h, w, [_want("rgbbox", h, w)] * 2, f"rgbbox {opts}", opts["entry_lists"])
        n = c.entry_counts()
        assert (n["waves"], n["lists"], n["fallbacks"]) == (0, 0, 0), n
        c.close()
