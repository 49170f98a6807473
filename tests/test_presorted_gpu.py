"""The sign-ordered node layout of the pooled kernel's plain LDS-resident instantiation: node records staged with their
lo / hi entries at addresses the ray's signs pick, box_hit_presorted in BOX and BOX2.  Bit-exact against the oracle on rgbbox and two more
scenes that live in LDS whole -- a tree far taller than its sweeps (unconverged upper boxes) and a scene with coincident and exactly
duplicated spheres (equal roots: the lowest leaf wins) -- at ragged sizes, as batches (the launches that take the new layout) and one frame
at a time (a view's first, second and later frames: the DONATE / ORD kernels, which keep the four planes).  rt_context_last_launch names
the layout of every launch; scenes read from L2 (irreg) must stay on the planes."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


def _tall_scene():
    """test_tall_trees' chain: single-bit Morton codes, 30 levels against floor(log2 31) + 2 = 6 sweeps"""
    pts = [(1023.0, 1023.0, 1023.0)]
    for a in range(3):
        for m in range(10):
            p = [0.0, 0.0, 0.0]
            p[a] = float(2 ** m)
            pts.append(tuple(p))
    s = np.zeros((len(pts), 7), np.float32)
    s[:, 0:3] = np.array(pts, np.float32)
    s[:, 3:6] = np.linspace(0.3, 1.0, 3 * len(pts), dtype=np.float32).reshape(-1, 3)
    s[:, 6] = 0.4
    s[1:, 6] = np.maximum(0.4, 0.3 * np.abs(s[1:, 0:3]).max(axis=1))   # (spheres a camera 70 units away can see)
    return s, (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0


def _dupes_scene():
    rng = np.random.default_rng(77)
    n = 240
    s = np.zeros((n, 7), np.float32)
    s[:, 0:3] = rng.uniform(-30, 30, (n, 3))
    s[:, 3:6] = rng.uniform(0.2, 1.0, (n, 3))
    s[:, 6] = rng.uniform(1.0, 5.0, n)
    s[100:140, 0:3] = s[0:40, 0:3]          # coincident centres, other colours and radii
    s[140:170] = s[40:70]                   # exact duplicates
    return s, (5.0, 25.0, 70.0), (0.0, 0.0, 0.0), 60.0


def _cases(ctx):
    yield "rgbbox", ctx.scene("rgbbox"), O.OracleScene("rgbbox")
    for name, (s, lf, la, fov) in (("tall", _tall_scene()), ("dupes", _dupes_scene())):
        yield name, ctx.scene_from_spheres(s, lf, la, fov), O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)


@pytest.mark.parametrize("h,w", [(203, 317), (97, 131), (64, 8)])
def test_lds_resident_scenes_bit_exact(R, h, w):
    import torch
    c = R.Context()
    c.set_variant(3)
    for name, scene, orc in _cases(c):
        want, _ = orc.render(h, w)
        ps = R.prepare_scene(h, w, scene)
        # batches: the plain kernel on the sign-ordered records
        for nb in (3, 1):
            buf = torch.full((nb, h, w), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            R.render_batch_into(buf.data_ptr(), h, w, ps, nb, frame_stride=h * w)
            c.sync()
            ll = c.last_launch
            bad = [int((f != want).sum()) for f in buf.cpu().numpy()]
            print(f"{name} {w}x{h} batch of {nb}: differing pixels {bad}; {ll}")
            assert all(b == 0 for b in bad), (name, "batch", nb, bad, ll)
            if nb > 1:
                assert "instantiation=plain " in ll and "nodes=sign-ordered" in ll, (name, ll)
                if name != "tall":      # (a 30-level tree's box stacks leave room for 12 waves)
                    assert "waves=16" in ll, (name, ll)
        # one frame at a time: the first frame records the view, the second sorts the record, later ones draw from the pixel list
        out = torch.empty((h, w), dtype=torch.int32, device="cuda")
        for frame in range(4):
            out.fill_(-3)
            torch.cuda.synchronize()
            R.render_into(out.data_ptr(), h, w, ps)
            c.sync()
            ll = c.last_launch
            bad = int((out.cpu().numpy() != want).sum())
            print(f"{name} {w}x{h} frame {frame}: differing pixels {bad}; {ll}")
            assert bad == 0, (name, frame, ll)
            # the layout follows the instantiation: sign-ordered exactly for the plain kernel
            assert ("nodes=sign-ordered" in ll) == ("instantiation=plain " in ll), (name, frame, ll)
        ps.free()
    c.close()


def test_smaller_workgroups_take_the_layout_too(R):
    """The plain LDS-resident kernels of 4, 8 and 12 waves are the same template: rgbbox through each."""
    c = R.Context()
    c.set_variant(3)
    c.set_option("pixel_order", 0)
    c.set_option("adaptive_order", 0)
    want, _ = O.OracleScene("rgbbox").render(120, 152)
    for waves in (4, 8, 12, 16):
        c.set_option("waves_per_wg", waves)
        got = R.render(120, 152, R.prepare_scene(120, 152, c.scene("rgbbox")))
        ll = c.last_launch
        bad = int((got != want).sum())
        print(f"rgbbox 152x120, {waves} waves: differing pixels {bad}; {ll}")
        assert bad == 0, (waves, ll)
        assert f"waves={waves}" in ll, ll
        if waves != 16:         # (16 waves: an unordered single frame is a DONATE launch)
            assert "instantiation=plain " in ll, ll
        assert ("nodes=sign-ordered" in ll) == ("instantiation=plain " in ll), ll
    c.close()


def test_scenes_read_from_l2_keep_the_planes(R):
    import torch
    c = R.Context()
    c.set_variant(3)
    h, w = 120, 160
    want, _ = O.OracleScene("irreg").render(h, w)
    ps = R.prepare_scene(h, w, c.scene("irreg"))
    buf = torch.full((3, h, w), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(buf.data_ptr(), h, w, ps, 3, frame_stride=h * w)
    c.sync()
    ll = c.last_launch
    assert all(int((f != want).sum()) == 0 for f in buf.cpu().numpy()), ll
    assert "nodes=planes" in ll and "nodes=sign-ordered" not in ll, ll
    for frame in range(3):
        got = R.render(h, w, ps)
        assert int((got != want).sum()) == 0, (frame, c.last_launch)
        assert "nodes=planes" in c.last_launch, c.last_launch
    c.close()
