"""The render path's dark stop on the GPU (lane_core.h: light_is_dead): the pooled family finishes a bounce chain whose
light is exactly (0, 0, 0) as pixel 0.  Every image is the oracle's, bit for bit -- single frames of a view (the first records and does not
stop, the later ones stop), batches, a part of a partition, and every instantiation the rule was compiled into, each named by
rt_context_last_launch; the instrumented launch counts the stopped chains' sphere tests under dark_stop = 1 and the reference's otherwise;
a view's record keeps the FULL chain lengths; scenes with inf and NaN colours equal the pixel family's image; caller rays are untouched.
(sync_policy = 1 throughout: which launch renders frame k is then the same in every run.)"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dark_stop_cases as D
import oracle_lib as O
import view_order_cases as VC
import view_order_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = {"rgbbox": "rgbbox", "two_walls": D.two_walls(), "underflow": D.underflow(), "negative_zero": D.negative_zero(), "floor": D.coloured_floor()}


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


@functools.lru_cache(maxsize=None)
def _orc(name):
    if name == "rgbbox":
        return O.OracleScene("rgbbox")
    s, lf, la, fov = SCENES[name]
    return O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)


@functools.lru_cache(maxsize=None)
def _want(name, h, w, max_depth=50):
    img, cnt = _orc(name).render(h, w, max_depth=max_depth)
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
    if name == "rgbbox":
        return c.scene("rgbbox")
    s, lf, la, fov = SCENES[name]
    return c.scene_from_spheres(s, lf, la, fov)


def _dark(ll):
    assert ("dark=1" in ll) != ("dark=0" in ll), ll
    return "dark=1" in ll


def _frame(R, c, ps, h, w, want, what, **kw):
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
    # a launch stops exactly when it does not record
    assert _dark(ll) == ("recording=0" in ll), ll
    return ll


# ---------------------------------------------------------------------------------------------------------------- single frames
@pytest.mark.parametrize("name,h,w", [("rgbbox", 53, 77), ("rgbbox", 24, 40), ("rgbbox", 8, 8), ("two_walls", 64, 64), ("underflow", 64, 64),
                                      ("negative_zero", 64, 64)])
def test_frames_of_a_view(R, name, h, w):
    """frame 1 records the view and does not stop; frames 2 and 3 stop"""
    c = _ctx(R)
    want, _ = _want(name, h, w)
    ps = R.prepare_scene(h, w, _scene(c, name))
    lls = [_frame(R, c, ps, h, w, want, f"{name} {w}x{h} frame {k}") for k in (1, 2, 3)]
    assert [_dark(ll) for ll in lls] == [False, True, True], lls
    c.set_option("dark_stop", 0)
    assert not _dark(_frame_plain(R, c, ps, h, w, want, f"{name} {w}x{h} dark_stop=0"))
    c.close()


def _frame_plain(R, c, ps, h, w, want, what):
    got = R.render(h, w, ps)
    ll = c.last_launch
    assert int((got != want).sum()) == 0, (what, ll)
    return ll


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_light_dies_where_the_budget_ends(R, max_depth):
    h = w = 64
    c = _ctx(R)
    want, _ = _want("two_walls", h, w, max_depth)
    ps = R.prepare_scene(h, w, _scene(c, "two_walls"))
    for k in (1, 2, 3):
        _frame(R, c, ps, h, w, want, f"two walls max_depth {max_depth} frame {k}", max_depth=max_depth)
    c.close()


@pytest.mark.parametrize("name,h,w", [("rgbbox", 24, 40), ("two_walls", 64, 64)])
def test_the_record_keeps_the_full_chains(name, h, w, tmp_path):
    """tools/view_order_check reads a view's arrays behind its frames: after the recording frame cost_px is min(chain length, 255) of the
    oracle's FULL chains (two walls: 50 everywhere, where the stopped chains have 2 rays), and the frame behind it stops."""
    exe = os.path.join(ROOT, "build", "view_order_check")
    subprocess.run(["make", "-s", "build/view_order_check"], cwd=ROOT, check=True)
    cf = VC.CaseFile()
    cf.view(SCENES[name], h, w, 50, 0, 8, 0, 1, 2, [("pixel_order", 2), ("eager_sort", 0), ("sync_policy", 1)])
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    cf.write(src)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    res = VC.Results(dst)
    frames = []
    for _ in range(2):
        meta = res.block(np.int32)
        launch = bytes(res.block()).decode()
        cost, order, cost_px, lst = res.block(np.int32), res.block(np.int32), res.block(np.uint8), res.block(np.uint32)
        frames.append((launch, cost, cost_px))
    assert res.done()
    chains = _orc(name).chain_lengths(h, w)
    g = V.PxGeom(w, h, 3, 0)
    want_px, want_cost = V.view_records(chains, w)
    lrow, col = np.divmod(np.arange(g.npix, dtype=np.int64), g.w)
    (l1, cost1, px1), (l2, _, _) = frames
    print(l1, l2, sep="\n")
    assert "recording=2" in l1 and not _dark(l1), l1
    assert "recording=0" in l2 and _dark(l2), l2
    assert (px1[g.record_index(lrow, col)] == want_px.ravel()).all(), "cost_px == min(full chain length, 255)"
    assert (cost1 == want_cost).all(), "cost == the tile's longest full chain"
    if name == "two_walls":
        assert (want_px == 50).all()


# ---------------------------------------------------------------------------------------------------------------- batches
def test_batches(R):
    import torch
    h, w = 53, 77
    c = _ctx(R)
    orc = _orc("rgbbox")
    want, _ = _want("rgbbox", h, w)
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))

    def batch(what, wants, **kw):
        rows = wants[0].shape[0]
        buf = torch.full((3, rows, w), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=rows * w, **kw)
        c.sync()
        ll = c.last_launch
        bad = [int((f != x).sum()) for f, x in zip(buf.cpu().numpy(), wants)]
        print(f"{what}: differing pixels {bad}; {ll}")
        assert all(b == 0 for b in bad), (what, bad, ll)
        assert _dark(ll) == ("recording=0" in ll) and "frames=3" in ll, ll
        return ll

    # one camera: the view's first batch records its tiles, the second stops -- on the plain kernel over the sign-ordered records
    lls = [batch(f"one camera, batch {k}", [want] * 3) for k in (1, 2)]
    assert _dark(lls[1]) and "instantiation=plain " in lls[1] and "nodes=sign-ordered" in lls[1], lls
    # a camera each: no view, nothing records
    cams = np.tile(orc.camera_floats(h, w), (3, 1))
    cams[:, 0] += np.float32(0.3) * np.arange(3, dtype=np.float32)
    ll = batch("a camera each", [orc.render(h, w, cam=cam)[0] for cam in cams], cams=cams)
    assert _dark(ll), ll
    # part 1 of 3
    rows = VC.part_rows(h, 8, 1, 3)
    for k in (1, 2):
        ll = batch(f"part 1 of 3, batch {k}", [want[rows]] * 3, part=1, nparts=3)
    assert _dark(ll), ll
    for k in (1, 2):
        ll = _frame(R, c, ps, h, w, want[rows], f"part 1 of 3, frame {k}", part=1, nparts=3)
    assert _dark(ll), ll
    c.close()


# ---------------------------------------------------------------------------------------------------------------- instantiations
def test_ord_solo(R):
    h = w = 200
    c = _ctx(R)
    want, _ = _want("rgbbox", h, w)
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    lls = [_frame(R, c, ps, h, w, want, f"rgbbox 200x200 frame {k}") for k in (1, 2, 3)]
    assert "DONATE" in lls[0] and not _dark(lls[0]), lls[0]          # a new view: recorded by the DONATE kernel, not stopped
    for ll in lls[1:]:
        assert "instantiation=ORD+SOLO " in ll and "tickets=pixel-list" in ll and _dark(ll), ll
    c.close()


def test_donate(R):
    """unordered single frames that record nothing (adaptive_order = 0): the DONATE kernel, stopping -- stopped rays are not given away"""
    h = w = 200
    c = _ctx(R, adaptive_order=0)
    want, _ = _want("rgbbox", h, w)
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    for k in (1, 2):
        ll = _frame(R, c, ps, h, w, want, f"rgbbox 200x200 unordered frame {k}")
        assert "DONATE" in ll and _dark(ll), ll
    c.close()


def test_cold(R):
    """rgbbox 400 x 400: 2 500 tiles, inside the COLD kernel's gate (2 048 .. 10 000 tiles, ordered frames drawing tile tickets)"""
    h = w = 400
    c = _ctx(R, pixel_order=0)
    want, _ = _want("rgbbox", h, w)
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    lls = [_frame(R, c, ps, h, w, want, f"rgbbox 400x400 frame {k}") for k in (1, 2, 3)]
    for ll in lls[1:]:
        assert "instantiation=COLD" in ll and "tiles=2500" in ll and _dark(ll), ll
    c.close()


def test_scene_read_from_l2_in_the_twenty_wave_shape(R):
    """6 400 spheres in three saturated colours, 20 frames of 600 x 600 (112 500 tiles): five workgroups of four waves per CU"""
    import torch
    h = w = 600
    c = _ctx(R)
    want, _ = _want("floor", h, w)
    ps = R.prepare_scene(h, w, _scene(c, "floor"))
    want_t = torch.from_numpy(np.array(want)).cuda()
    buf = torch.empty((20, h, w), dtype=torch.int32, device="cuda")
    for k in (1, 2):
        buf.fill_(-7)
        torch.cuda.synchronize()
        R.render_batch_into(buf.data_ptr(), h, w, ps, 20, frame_stride=h * w)
        c.sync()
        ll = c.last_launch
        bad = int((buf != want_t).sum().item())
        print(f"floor 600x600 x 20, batch {k}: differing pixels {bad}; {ll}")
        assert bad == 0, ll
        assert "waves=4" in ll and "nodes=planes" in ll and _dark(ll) == ("recording=0" in ll), ll
    assert _dark(ll), ll
    c.close()


def test_spill(R):
    """the SPILL kernels (stack_cap = 192: the box stack overflows into device memory all the time)"""
    import torch
    h, w = 120, 160
    c = _ctx(R, wide_waves=2, stack_cap=192)
    want, _ = _want("floor", h, w)
    ps = R.prepare_scene(h, w, _scene(c, "floor"))
    buf = torch.empty((3, h, w), dtype=torch.int32, device="cuda")
    for k in (1, 2):
        buf.fill_(-7)
        torch.cuda.synchronize()
        R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=h * w)
        c.sync()
        ll = c.last_launch
        bad = [int((f != want).sum()) for f in buf.cpu().numpy()]
        print(f"floor 160x120 x 3, stack_cap 192, batch {k}: differing pixels {bad}; {ll}")
        assert all(b == 0 for b in bad), ll
        assert "+SPILL" in ll and _dark(ll) == ("recording=0" in ll), ll
    assert _dark(ll), ll
    c.close()


# ---------------------------------------------------------------------------------------------------------------- stopped counts
def test_the_instrumented_launch_counts_what_was_asked_for(R):
    """rt_render_trace's leaf items (sphere tests) for rgbbox 200 x 200, cull = 0: the stopped chains' under dark_stop = 1, the reference's
    under 0 and under the default"""
    from raytracers_amd._lib import lib
    h = w = 200
    (_, _, spheres), (_, _, spheres_stop), _, _ = D.RGBBOX[(h, w)]
    c = _ctx(R, cull=0)
    want, cnt = _want("rgbbox", h, w)
    assert cnt["leaf_tests"] == spheres
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    for _ in range(2):
        assert int((R.render(h, w, ps) != want).sum()) == 0
    for dark_stop, expect in ((1, spheres_stop), (0, spheres), (-1, spheres)):
        c.set_option("dark_stop", dark_stop)
        rec = np.zeros((8192, 16), dtype=np.uint64)
        n = C.c_int32()
        c._check(lib.rt_render_trace(c._h, ps._h, h, w, 50, rec.ctypes.data, 8192, C.byref(n)))
        leaf_items = int((rec[: n.value].astype(np.int64)[:, 6] & 0xFFFFFFFF).sum())
        print(f"dark_stop {dark_stop}: leaf items {leaf_items}, expected {expect}")
        assert leaf_items == expect, (dark_stop, leaf_items, expect)
        assert int((R.render(h, w, ps) != want).sum()) == 0
    c.close()


# ---------------------------------------------------------------------------------------------------------------- non-finite colours
def test_nonfinite_colours_equal_the_pixel_family(R):
    """a black wall, a wall of colour (inf, NaN, 1), a sphere of colour (inf, 0, 1): stopped chains whose continuation meets inf and NaN, and
    chains kept alive by NaN.  Both images are the device's (the oracle's conversion of NaN is undefined in C)."""
    import torch
    h = w = 64
    s, lf, la, fov = D.nonfinite()
    c = _ctx(R)
    ps = R.prepare_scene(h, w, c.scene_from_spheres(s, lf, la, fov))
    c.set_variant(R.VARIANT_PIXEL)
    want = R.render(h, w, ps)
    assert c.last_launch == "family=pixel"
    assert 0 < int((want == 0).sum()) and 0 < int((want != 0).sum()), "some pixels dark, some not"
    c.set_variant(R.VARIANT_POOLED)
    lls = [_frame(R, c, ps, h, w, want, f"non-finite colours frame {k}") for k in (1, 2, 3)]
    assert _dark(lls[2]), lls
    buf = torch.full((3, h, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=h * w)
    c.sync()
    assert _dark(c.last_launch) and all(int((f != want).sum()) == 0 for f in buf.cpu().numpy()), c.last_launch
    c.close()


# ---------------------------------------------------------------------------------------------------------------- caller rays
def test_caller_rays_do_not_stop(R):
    """rt_trace_rays on rgbbox 64 x 64's primary rays: float colours show -0 and NaN payloads, so these chains are traced in full --
    the colours are bit-equal under dark_stop -1 and 0, and they are the oracle's"""
    import torch
    h = w = 64
    n = h * w
    c = _ctx(R)
    ps = R.prepare_scene(h, w, c.scene("rgbbox"))
    rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    R.camera_rays_into(rays.data_ptr(), h, w, ps)
    c.sync()
    got = {}
    for dark_stop in (-1, 0):
        c.set_option("dark_stop", dark_stop)
        col = torch.full((n, 3), -1.0, dtype=torch.float32, device="cuda")
        pix = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        R.trace_rays_into(rays.data_ptr(), n, ps, colour_ptr=col.data_ptr(), pixel_ptr=pix.data_ptr())
        c.sync()
        assert "tickets=rays" in c.last_launch and "dark" not in c.last_launch, c.last_launch
        got[dark_stop] = (col.cpu().numpy().view(np.uint32), pix.cpu().numpy())
    assert (got[-1][0] == got[0][0]).all() and (got[-1][1] == got[0][1]).all()
    want = _orc("rgbbox").ray_colour_rays(rays.cpu().numpy(), 50).view(np.uint32)
    assert (got[-1][0] == want).all()
    assert (got[-1][1].reshape(h, w) == _want("rgbbox", h, w)[0]).all()
    c.close()
