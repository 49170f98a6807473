"""The leaf's own box in the pooled BOX / BOX2 operations on the GPU (lane_core.h: leaf_box_eps): a leaf child is appended
to the leaf list only if the box in its slot of the node record -- the sphere's own, widened by the proven margin -- passes.  Every image is
the oracle's, bit for bit: frames 1, 2, 3 of a view, batches with one camera and a camera each, a part of a partition, both node layouts, the
twenty-wave CULL and SPILL kernels (scenes read from L2: never filtered, the parent's kernels), a 30-level tree that passes the guards, scenes
prepared and updated from device spheres.  rt_context_last_launch says whether a launch filtered
("leaf_box=0|1" in its last token) and the expected decision is restated here in float64, not asked of the library: scenes and cameras just
inside and outside the guards, grazing rays, zero direction components.  The instrumented launch counts the filtered sphere tests under
leaf_box = 1 only.  (sync_policy = 1 throughout: which launch renders frame k is then the same in every run.)"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import dark_stop_cases as D
import oracle_lib as O
import test_presorted_gpu as P
import view_order_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


# ------------------------------------------------------------------------------------------------ the guards, restated (rt_host.hpp: LeafBoxConst)
def guards(s):
    """float64 restatement of rt::leaf_box_finish: ok, the centre, D_eps and the largest admitted |origin - centre|"""
    p, r = s[:, 0:3].astype(np.float64), s[:, 6].astype(np.float64)
    out = dict(ok=False)
    if not (np.isfinite(p).all() and np.isfinite(r).all() and (r >= 2.0 ** -20).all()):
        return out
    c_max = (np.abs(p) + r[:, None]).max()
    lo, hi = p.min(axis=0), p.max(axis=0)
    big_r = 0.5 * np.sqrt(((hi - lo) ** 2).sum()) * (1.0 + 2.0 ** -20)
    d_eps = 2.0 * (big_r + r.max())
    out.update(centre=0.5 * (lo + hi), d_eps=d_eps, cam_max=d_eps - big_r)
    out["ok"] = bool(c_max <= 2.0 ** 40 and c_max + d_eps <= 2.0 ** 15 * r.min() and
                     2.0 ** -18 * (d_eps * d_eps / (r.min() * r.min()) + 1.0) <= 0.4375 * (1.0 - 2.0 ** -10))
    return out


def camera_ok(g, cam):
    cam = np.asarray(cam, np.float64)
    if not g["ok"] or not np.isfinite(cam).all() or np.abs(cam).max() > 2.0 ** 15:
        return False
    if np.linalg.norm(cam[0:3] - g["centre"]) * (1.0 + 2.0 ** -20) > g["cam_max"]:
        return False
    n = np.cross(cam[6:9], cam[9:12])
    nn = np.linalg.norm(n)
    return bool(nn > 0 and abs(np.dot(cam[3:6] - cam[0:3], n)) / nn * (1.0 - 2.0 ** -20) - 2.0 ** -19 * np.abs(cam).max() >= 2.0 ** -12)


# ------------------------------------------------------------------------------------------------ scenes
def _wall(m=12, spacing=1.5, radius=0.25):
    """m x m small spheres in the plane z = 0, centred on the origin: seen from the z axis every ray grazes many of them (D^2 / r in the
    thousands), and the centre column / row of an axis camera have d_x = 0 / d_y = 0"""
    i, j = np.divmod(np.arange(m * m), m)
    s = np.zeros((m * m, 7), F)
    s[:, 0] = (i - (m - 1) / 2) * spacing
    s[:, 1] = (j - (m - 1) / 2) * spacing
    s[:, 3:6] = np.linspace(0.3, 1.0, 3 * m * m, dtype=F).reshape(-1, 3)
    s[:, 6] = radius
    s[::7, 2] = 0.75                                       # some stand forward: bounces between neighbours
    s[::7, 6] = 0.5
    return s


def _axis_cam(z):
    return np.array([0.0, 0.0, z, -0.5, -0.5, z - 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], F)


def _dust():
    """spheres of radius 0.02 in a box of 40: D_eps / r_min = 3 500 -- the scene guard refuses (a root's error may exceed the radius)"""
    rng = np.random.default_rng(3)
    s = np.zeros((300, 7), F)
    s[:, 0:3] = rng.uniform(-20, 20, (300, 3))
    s[:, 3:6] = rng.uniform(0.3, 1.0, (300, 3))
    s[:, 6] = 0.02
    s[:40, 6] = 4.0
    return s, (0.0, 10.0, 45.0), (0.0, 0.0, 0.0), 50.0


def _tall_fat():
    """the 30-level chain of test_presorted_gpu with radii large enough for the scene guard (D_eps / r_min = 300) and a camera inside the
    camera guard: the filter runs on a tree five times taller than its sweeps (unconverged upper boxes)"""
    s = P._tall_scene()[0].copy()
    s[:, 6] = 6.0
    return s, (700.0, 640.0, 820.0), (300.0, 300.0, 300.0), 60.0


SCENES = {"tall_fat": _tall_fat(), "tall": P._tall_scene(), "dupes": P._dupes_scene(), "floor": D.coloured_floor(), "dust": _dust(),
          "dupes_near": P._dupes_scene()[:1] + ((3.0, 10.0, 35.0), (0.0, 0.0, 0.0), 70.0)}
NAMED = ("rgbbox", "irreg")
# the decision each scene's own camera gets (checked against the restatement in test_the_expected_decisions)
EXPECT = {"rgbbox": True, "irreg": True, "tall_fat": True, "tall": False, "dupes": False, "dupes_near": True, "floor": True, "dust": False}


@functools.lru_cache(maxsize=None)
def _orc(name):
    if name in NAMED:
        return O.OracleScene(name)
    s, lf, la, fov = SCENES[name]
    return O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)


@functools.lru_cache(maxsize=None)
def _want(name, h, w):
    img, cnt = _orc(name).render(h, w)
    img.setflags(write=False)
    return img, cnt


def _ctx(R, **opts):
    c = R.Context()
    c.set_variant(R.VARIANT_POOLED)
    c.set_option("sync_policy", 1)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _scene(c, name):
    if name in NAMED:
        return c.scene(name)
    s, lf, la, fov = SCENES[name]
    return c.scene_from_spheres(s, lf, la, fov)


L2_SCENES = ("irreg", "floor")     # read from L2, not wholly LDS resident: never filtered (api.cpp: set_leaf_box), whatever their guards say


def _leaf(ll):
    m = re.search(r"nodes=\S+,leaf_box=([01])$", ll)
    assert m, ll
    return m.group(1) == "1"


def _filters(name, ll, expect):
    """the decision for a scene whose guards say `expect`: a scene read from L2 never filters (rt_device.hpp: pooled_leaf_box)"""
    return expect and name not in L2_SCENES


def _frame(R, c, ps, h, w, want, what, expect, **kw):
    import torch
    rows = R.part_rows(h, kw.get("part", 0), kw.get("nparts", 1)) if "part" in kw else h
    out = torch.full((rows, w), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_into(out.data_ptr(), h, w, ps, **kw)
    c.sync()
    ll = c.last_launch
    bad = int((out.cpu().numpy() != want).sum())
    print(f"{what}: differing pixels {bad}; {ll}")
    assert bad == 0, (what, bad, ll)
    assert expect is None or _leaf(ll) == expect, (what, ll)
    return ll


def _batch(R, c, ps, h, w, wants, what, expect, **kw):
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
    assert _leaf(ll) == expect and f"frames={len(wants)}" in ll, (what, ll)
    return ll


def test_the_expected_decisions():
    """EXPECT is what the float64 restatement of the guards says about each scene's own camera (at a square image)"""
    for name, expect in EXPECT.items():
        if name in NAMED:
            continue
        s, lf, la, fov = SCENES[name]
        g = guards(s)
        assert camera_ok(g, _orc(name).camera_floats(64, 64)) == expect, (name, g)
    assert not guards(SCENES["tall"][0])["ok"] and not guards(SCENES["dust"][0])["ok"] and guards(SCENES["dupes"][0])["ok"]


# ------------------------------------------------------------------------------------------------ frames of a view, both layouts
@pytest.mark.parametrize("name,h,w", [("rgbbox", 64, 64), ("rgbbox", 53, 77), ("irreg", 200, 200), ("tall_fat", 97, 131), ("tall", 97, 131), ("dupes", 97, 131),
                                      ("dupes_near", 97, 131), ("dust", 64, 64)])
def test_frames_of_a_view(R, name, h, w):
    """frame 1 records the view (and filters: the record is the chains' lengths), frames 2 and 3 draw from its order / pixel list; then the
    option off: the parent's launches"""
    c = _ctx(R)
    want, _ = _want(name, h, w)
    ps = R.prepare_scene(h, w, _scene(c, name))
    lls = [_frame(R, c, ps, h, w, want, f"{name} {w}x{h} frame {k}", None) for k in (1, 2, 3)]
    assert [_leaf(ll) for ll in lls] == [_filters(name, ll, EXPECT[name]) for ll in lls], lls
    c.set_option("leaf_box", 0)
    _frame(R, c, ps, h, w, want, f"{name} {w}x{h} leaf_box=0", False)
    c.close()


@pytest.mark.parametrize("name,filtered", [("rgbbox", True), ("irreg", False)])
def test_frames_through_the_pixel_list(R, name, filtered):
    """pixel_order = 2: a view's third frame draws from its pixel list whatever its size -- the ORD kernels, which filter on a scene that lives
    in LDS; a scene read from L2 is never filtered"""
    h = w = 200
    c = _ctx(R, pixel_order=2)
    want, _ = _want(name, h, w)
    ps = R.prepare_scene(h, w, _scene(c, name))
    lls = [_frame(R, c, ps, h, w, want, f"{name} {w}x{h} pixel_order 2 frame {k}", None) for k in (1, 2, 3)]
    assert _leaf(lls[0]) == filtered and "instantiation=ORD" not in lls[0], lls[0]
    assert "instantiation=ORD" in lls[2] and "tickets=pixel-list" in lls[2] and _leaf(lls[2]) == filtered, lls[2]
    c.close()


@pytest.mark.parametrize("name,h,w,nodes", [("rgbbox", 53, 77, "sign-ordered"), ("irreg", 200, 200, "planes"), ("dupes_near", 97, 131, "sign-ordered"),
                                            ("tall_fat", 97, 131, "sign-ordered")])
def test_batches(R, name, h, w, nodes):
    c = _ctx(R)
    orc = _orc(name)
    want, _ = _want(name, h, w)
    ps = R.prepare_scene(h, w, _scene(c, name))
    on = _filters(name, "", True)
    for k in (1, 2):     # one camera: the view's first batch records its tiles
        ll = _batch(R, c, ps, h, w, [want] * 3, f"{name} one camera, batch {k}", on)
    assert f"nodes={nodes}," in ll and "instantiation=plain" in ll, ll
    cams = np.tile(orc.camera_floats(h, w), (3, 1))
    cams[:, 0] += F(0.3) * np.arange(3, dtype=F)
    _batch(R, c, ps, h, w, [orc.render(h, w, cam=cam)[0] for cam in cams], f"{name} a camera each", on, cams=cams)
    rows = VC.part_rows(h, 8, 1, 3)
    for k in (1, 2):
        _batch(R, c, ps, h, w, [want[rows]] * 3, f"{name} part 1 of 3, batch {k}", on, part=1, nparts=3)
        ll = _frame(R, c, ps, h, w, want[rows], f"{name} part 1 of 3, frame {k}", None, part=1, nparts=3)
        assert _leaf(ll) == on, ll
    c.set_option("leaf_box", 0)
    _batch(R, c, ps, h, w, [want] * 3, f"{name} leaf_box=0", False)
    c.close()


# ------------------------------------------------------------------------------------------------ the four-wave kernels
def test_twenty_wave_cull(R):
    """6 400 spheres read from L2, a batch of 3 in five workgroups of four waves per CU, culled by the best hit: the scene passes the guards
    and its slots are filled, but a scene read from L2 is never filtered -- the parent's kernel over the new records"""
    assert guards(SCENES["floor"][0])["ok"]
    h, w = 120, 160
    c = _ctx(R, wide_waves=2, cull=1)
    want, _ = _want("floor", h, w)
    ps = R.prepare_scene(h, w, _scene(c, "floor"))
    for k in (1, 2):
        ll = _batch(R, c, ps, h, w, [want] * 3, f"floor twenty-wave batch {k}", False)
    assert "waves=4" in ll and "instantiation=plain+CULL " in ll and "nodes=planes," in ll, ll
    c.close()


def test_spill(R):
    """stack_cap = 192: the SPILL kernels (scenes read from L2 only) over the new records, unfiltered"""
    h, w = 120, 160
    c = _ctx(R, wide_waves=2, stack_cap=192)
    want, _ = _want("floor", h, w)
    ps = R.prepare_scene(h, w, _scene(c, "floor"))
    for k in (1, 2):
        ll = _batch(R, c, ps, h, w, [want] * 3, f"floor stack_cap 192 batch {k}", False)
    assert "+SPILL" in ll, ll
    c.close()


# ------------------------------------------------------------------------------------------------ device spheres
@pytest.mark.parametrize("gpu_build", [1, 0])
def test_device_spheres_prepared_then_updated(R, gpu_build):
    """the slots are written by the host builder (gpu_build = 0) or behind the device's build (1): the same images; after an update in place
    the slots are the new spheres' -- and a set that fails the guards switches the filter off"""
    import torch
    h, w = 97, 131
    s, lf, la, fov = SCENES["dupes_near"]
    c = _ctx(R, gpu_build=gpu_build)
    ps = R.prepare_scene_from_spheres(c, torch.from_numpy(s).cuda(), h, w, lf, la, fov)
    want, _ = _want("dupes_near", h, w)
    for k in (1, 2):
        _frame(R, c, ps, h, w, want, f"device spheres, gpu_build {gpu_build}, frame {k}", True)
    _batch(R, c, ps, h, w, [want] * 3, "device spheres, batch", True)
    rng = np.random.default_rng(9)
    s2 = s.copy()
    s2[:, 0:3] += rng.uniform(-2, 2, (len(s), 3)).astype(F)
    s2[:, 6] *= F(1.25)
    want2, _ = O.OracleScene("custom", spheres7=s2, look_from=lf, look_at=la, fov=fov).render(h, w)
    ps.update_spheres(torch.from_numpy(s2).cuda())
    assert camera_ok(guards(s2), _orc("dupes_near").camera_floats(h, w))
    for k in (1, 2):
        _frame(R, c, ps, h, w, want2, f"updated spheres, frame {k}", True)
    _batch(R, c, ps, h, w, [want2] * 3, "updated spheres, batch", True)
    s3 = s2.copy()
    s3[5, 6] = 0.01                                        # one tiny sphere: D_eps / r_min beyond the guard
    assert not guards(s3)["ok"]
    want3, _ = O.OracleScene("custom", spheres7=s3, look_from=lf, look_at=la, fov=fov).render(h, w)
    ps.update_spheres(torch.from_numpy(s3).cuda())
    _frame(R, c, ps, h, w, want3, "updated spheres, guard failed", False)
    _batch(R, c, ps, h, w, [want3] * 3, "updated spheres, guard failed, batch", False)
    c.close()


# ------------------------------------------------------------------------------------------------ grazing rays, the camera guard
def test_grazing_and_the_camera_guard(R):
    h = w = 96
    s = _wall()
    g = guards(s)
    assert g["ok"] and (g["d_eps"] ** 2 / 0.25) > 2000
    orc = O.OracleScene("custom", spheres7=s, look_from=(0.0, 0.0, 11.0), look_at=(0.0, 0.0, 0.0), fov=50.0)
    axis = _axis_cam(11.0)
    assert (axis[3] + F(0.5) * axis[6]) - axis[0] == 0.0 and (axis[4] + F(0.5) * axis[10]) - axis[1] == 0.0   # d_x = 0 down column w/2, d_y = 0 along row h/2
    assert g["centre"][0] == 0.0 and g["centre"][1] == 0.0
    inside, outside = (_axis_cam(F(g["centre"][2] + g["cam_max"] * (1 + k * 2.0 ** -12))) for k in (-1, 1))
    skim = np.array([-8.0, 0.0, 0.3, -7.0, -0.5, 0.05, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0], F)     # along the wall, just above it: every sphere of a row is grazed
    cams = [axis, inside, outside, skim]
    expect = [camera_ok(g, cam) for cam in cams]
    assert expect == [True, True, False, True], expect
    c = _ctx(R)
    ps = R.prepare_scene(h, w, c.scene_from_spheres(s, (0.0, 0.0, 11.0), (0.0, 0.0, 0.0), 50.0))
    wants = [orc.render(h, w, cam=cam)[0] for cam in cams]
    assert all(int((x != wants[0]).sum()) > 0 for x in wants[2:])
    for cam, want, e, what in zip(cams, wants, expect, ("axis", "inside the guard", "outside the guard", "skimming")):
        for k in (1, 2):
            _frame(R, c, ps, h, w, want, f"wall, camera {what}, frame {k}", e, cam=cam)
    # batches: filtered only if every camera passes
    _batch(R, c, ps, h, w, [wants[0], wants[1], wants[3]], "wall, three cameras inside", True, cams=np.stack([cams[0], cams[1], cams[3]]))
    _batch(R, c, ps, h, w, wants[:3], "wall, the third camera outside", False, cams=np.stack(cams[:3]))
    c.close()


# ------------------------------------------------------------------------------------------------ counts
def test_the_instrumented_launch_counts_what_was_asked_for(R):
    """rt_render_trace's leaf items for rgbbox 200 x 200, cull = 0: tools/leaf_box_check's filtered count under leaf_box = 1, the reference's
    1 013 272 under 0 and under the default; with the dark stop on as well, the filtered count of the stopped chains"""
    from raytracers_amd._lib import lib
    h = w = 200
    subprocess.run(["make", "-s", "build/leaf_box_check"], cwd=ROOT, check=True)
    out = subprocess.run([os.path.join(ROOT, "build", "leaf_box_check"), "frame", "rgbbox", "-", str(h), str(w)], capture_output=True, text=True, check=True)
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)(?=\s)", out.stdout)}
    print(out.stdout.strip())
    assert f["spheres"] == 1013272 and f["lost"] == 0 and f["differ"] == 0
    c = _ctx(R, cull=0)
    want, cnt = _want("rgbbox", h, w)
    assert cnt["leaf_tests"] == f["spheres"]
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    for _ in range(2):
        assert int((R.render(h, w, ps) != want).sum()) == 0
    for leaf_box, dark_stop, expect in ((1, 0, f["filtered"]), (0, 0, f["spheres"]), (-1, 0, f["spheres"]), (1, 1, f["filtered_stop"]), (-1, 1, f["spheres_stop"])):
        c.set_option("leaf_box", leaf_box)
        c.set_option("dark_stop", dark_stop)
        rec = np.zeros((8192, 16), dtype=np.uint64)
        n = C.c_int32()
        c._check(lib.rt_render_trace(c._h, ps._h, h, w, 50, rec.ctypes.data, 8192, C.byref(n)))
        leaf_items = int((rec[: n.value].astype(np.int64)[:, 6] & 0xFFFFFFFF).sum())
        print(f"leaf_box {leaf_box} dark_stop {dark_stop}: leaf items {leaf_items}, expected {expect}")
        assert leaf_items == expect, (leaf_box, dark_stop, leaf_items, expect)
        assert int((R.render(h, w, ps) != want).sum()) == 0
    c.close()


# ------------------------------------------------------------------------------------------------ non-finite spheres
def test_nonfinite_spheres_equal_the_pixel_family(R):
    """a sphere at x = inf, one with a NaN radius, one of radius 0: no filter for the scene (its slots stay zero), and the pooled image is the
    pixel family's"""
    h = w = 64
    s, lf, la, fov = SCENES["dupes_near"]
    s = s.copy()
    s[3, 0] = np.inf
    s[17, 6] = np.nan
    s[29, 6] = 0.0
    assert not guards(s)["ok"]
    c = _ctx(R)
    ps = R.prepare_scene(h, w, c.scene_from_spheres(s, lf, la, fov))
    c.set_variant(R.VARIANT_PIXEL)
    want = R.render(h, w, ps)
    assert c.last_launch == "family=pixel"
    c.set_variant(R.VARIANT_POOLED)
    for k in (1, 2, 3):
        _frame(R, c, ps, h, w, want, f"non-finite spheres frame {k}", False)
    _batch(R, c, ps, h, w, [want] * 3, "non-finite spheres batch", False)
    c.close()
