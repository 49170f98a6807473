"""Rendered frames at the frame-size guards (tests/edge_frames.py): thin frames whose columns, rows or local rows reach 2^16, the limits of the
bit-reversed first order, the largest sides, batches at the bound of the ticket arithmetic, and the refusals.  Every pixel is compared with `==`
against the oracle's frame through the same explicit camera; `Context.last_launch` is compared, frame by frame, with the restated decision --
so an inside case provably runs the guarded path and an outside case provably does not.  Output buffers are poisoned before every frame.
sync_policy = 1: the same launches in every run."""
import functools
import time

import numpy as np
import pytest

import edge_frames as E
import oracle_lib as O
import ray_query_ref as Q

pytestmark = pytest.mark.gpu

POISON = -7777777           # (a pixel is 0xRRGGBB: never negative)
LDS = {"rgbbox": True, "irreg": False}      # does the whole scene live in LDS (edge_frames.expected)?


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import raytracers_amd
    return raytracers_amd


def _context(R, variant=None, **options):
    c = R.Context(0)
    c.set_option("sync_policy", 1)
    if variant:
        c.set_variant(variant)
    for k, v in options.items():
        c.set_option(k, v)
    return c


@pytest.fixture(scope="module")
def ctx(R):
    c = _context(R)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _oracle(scene):
    return O.OracleScene(scene)


@functools.lru_cache(maxsize=None)
def _cam(scene):
    return _oracle(scene).camera_floats(*E.SQUARE)


@functools.lru_cache(maxsize=None)
def _want(scene, h, w):
    """the oracle's h x w frame through the square camera, on the device -- built once per module"""
    import torch
    px, _ = _oracle(scene).render(h, w, cam=_cam(scene))
    return torch.from_numpy(px).cuda()


def _want_rows(scene, f):
    import torch
    from raytracers_amd.dist import tile_rows
    full = _want(scene, f.h, f.w)
    if f.nparts == 1:
        return full
    return full[torch.from_numpy(tile_rows(f.h, f.part, f.nparts, f.rpt)).cuda()]


def _prepared(R, ctx, scene):
    return R.prepare_scene(E.SQUARE[0], E.SQUARE[1], ctx.scene(scene))


def _check_launch(ctx, dec, what):
    s = ctx.last_launch
    got = E.parse_launch(s)
    assert got.family == dec.family, (what, s)
    if dec.family != "pooled":
        return got
    assert got.tickets == dec.tickets and not got.borrowed, (what, dec, s)
    assert got.recording == dec.recording, (what, dec, s)
    wide = E.wide_launch(ctx.device_info()["num_cu"])
    assert ((got.grid, got.waves) == wide) == dec.wide, (what, dec, s)
    if dec.tickets == "pixel-list":
        assert got.instantiation.startswith("ORD") and got.waves == 16, (what, s)
    return got


def _frames(R, ctx, ps, scene, f, frames, **options):
    """frames `frames` (1-based numbers of the view) of Frame f, packed: each equal to the oracle's rows, each launch the restated decision"""
    import torch
    want = _want_rows(scene, f)
    out = torch.empty((E.rows_local(f), f.w), dtype=torch.int32, device="cuda")
    seen = []
    for k in frames:
        out.fill_(POISON)
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the render on the context's own: order them)
        R.render_into(out.data_ptr(), f.h, f.w, ps, part=f.part, nparts=f.nparts, rows_per_tile=f.rpt, cam=_cam(scene))
        ctx.sync()
        what = f"{scene} {tuple(f)} frame {k} {options}"
        bad = int((out != want).sum())
        assert bad == 0, f"{what}: {bad} pixels differ from the oracle ({int((out == POISON).sum())} never written); {ctx.last_launch}"
        seen.append(_check_launch(ctx, E.expected(f, k, LDS[scene], **options), what))
    return seen


# ---------------------------------------------------------------------------------------------------------------- guard pairs
@pytest.mark.parametrize("name", list(E.PAIRS))
@pytest.mark.parametrize("scene", E.SCENES)
def test_guard_pair(R, ctx, scene, name):
    """Frames 1 to 4 of the view on either side of a guard.  The inside frames of the list's guards render frames 2 .. 4 through the pixel list
    (ORD); their outside twins -- one column, one row, one tile of local rows more -- never do."""
    inside, outside = E.PAIRS[name]
    ps = _prepared(R, ctx, scene)
    got_in = _frames(R, ctx, ps, scene, inside, (1, 2, 3, 4))
    got_out = _frames(R, ctx, ps, scene, outside, (1, 2, 3, 4))
    if name.startswith("list_"):
        assert [g.tickets for g in got_in[1:]] == ["pixel-list"] * 3 and all(g.instantiation.startswith("ORD") for g in got_in[1:])
        assert all(g.tickets != "pixel-list" for g in got_out)
    else:
        assert got_in[0].tickets == "tiles-bit-reversed" and got_out[0].tickets == "tiles-raster"
    assert all(g.tiles == E.tile_grid(f)[0] * E.tile_grid(f)[1] for f, gs in ((inside, got_in), (outside, got_out)) for g in gs)
    ps.free()


def test_one_tile_row_is_a_raster(R, ctx):
    """tiles_y == 1 is outside the first order by its guard: (8, 65 535) as a first frame is drawn in raster order, 8192 tiles long."""
    ps = _prepared(R, ctx, "irreg")
    got = _frames(R, ctx, ps, "irreg", E.Frame(8, 65535), (1,))
    assert got[0].tickets == "tiles-raster" and got[0].tiles == 8192
    ps.free()


@pytest.mark.parametrize("h", E.PART_PAIR)
@pytest.mark.parametrize("scene", E.SCENES)
def test_parts_with_local_rows_at_the_guard(R, ctx, scene, h):
    """Both parts of two of an h x 8 image (local rows 65 528: the list; 65 536: no list; global rows beyond 2^16 either way): three frames packed,
    then three frames in place into ONE image -- the list the packed frames recorded serves the in-place ones.  Every row is the oracle's, and a
    part's in-place frames write nothing into the other part's rows."""
    import torch
    from raytracers_amd.dist import tile_rows
    ps = _prepared(R, ctx, scene)
    want = _want(scene, h, 8)
    image = torch.full((h, 8), POISON, dtype=torch.int32, device="cuda")
    for part in (0, 1):
        f = E.Frame(h, 8, part, 2)
        _frames(R, ctx, ps, scene, f, (1, 2, 3))
        mine = torch.from_numpy(tile_rows(h, part, 2)).cuda()
        for k in (4, 5, 6):
            image[mine] = POISON
            before = image.clone()
            torch.cuda.synchronize()
            R.render_inplace_into(image.data_ptr(), h, 8, ps, cams=_cam(scene), part=part, nparts=2)
            ctx.sync()
            what = f"{scene} {h} x 8 part {part} in place, frame {k}"
            assert torch.equal(image[mine], want[mine]), what
            others = torch.ones(h, dtype=torch.bool, device="cuda")
            others[mine] = False
            assert torch.equal(image[others], before[others]), what + ": rows of the other part were written"
            _check_launch(ctx, E.expected(f, k, LDS[scene]), what)
    assert torch.equal(image, want)
    ps.free()


# ---------------------------------------------------------------------------------------------------------------- other schemes and families
@pytest.mark.parametrize("options", [dict(xcd_queues=0), dict(xcd_queues=1), dict(pixel_order=0), dict(pixel_order=2), dict(first_order=0),
                                     dict(variant=1), dict(variant=2)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_sixteen_bit_frames_under_other_schemes(R, options):
    """(8, 65 535), (8, 65 536), (65 535, 8), (65 536, 8) with one counter, with eight strips (no list; tiles_x == 1 leaves seven strips empty),
    without the list, with the list forced, without the first order, and through the pixel and persistent families (blockIdx.x % tiles_x)."""
    opts = dict(options)
    variant = opts.pop("variant", None)
    c = _context(R, variant, **opts)
    for scene in E.SCENES:
        for f in E.SIXTEEN_BIT:
            ps = _prepared(R, c, scene)
            got = _frames(R, c, ps, scene, f, (1, 2) if variant else (1, 2, 3, 4), **options)
            if options.get("xcd_queues") == 1:
                assert all(g.counters == 8 and not g.turns and g.tickets != "pixel-list" for g in got)
            if options.get("xcd_queues") == 0:
                assert all(g.counters == 1 for g in got)
            ps.free()
    c.close()


@pytest.mark.parametrize("f", E.LARGEST, ids=lambda f: f"{f.h}x{f.w}")
def test_largest_sides(R, ctx, f):
    """(8, 2^20) and (2^20, 8), irreg: 131 072 tiles in one row or one column, in the shape of twenty waves per CU (grid and waves from the device's
    CU count), a raster first and through the tile order then."""
    ps = _prepared(R, ctx, "irreg")
    got = _frames(R, ctx, ps, "irreg", f, (1, 2))
    assert [g.tickets for g in got] == ["tiles-raster", "tiles-ordered"] and all(g.tiles == 131072 for g in got)
    assert all((g.grid, g.waves) == E.wide_launch(ctx.device_info()["num_cu"]) for g in got)
    ps.free()


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("scene", E.SCENES)
def test_batches_of_thin_frames(R, ctx, scene):
    """Three frames of (8, 65 535) and of (65 535, 8) in one launch with a padded stride (the padding stays poisoned); then with a camera per
    frame, each frame equal to render_image through that camera."""
    import torch
    n, pad = 3, 40
    for f in (E.Frame(8, 65535), E.Frame(65535, 8)):
        ps = _prepared(R, ctx, scene)
        want = _want(scene, f.h, f.w).reshape(-1)
        stride = f.h * f.w + pad
        for rep in (1, 2):
            out = torch.full((n, stride), POISON, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            R.render_batch_into(out.data_ptr(), f.h, f.w, ps, n, frame_stride=stride, cams=np.tile(_cam(scene), n))
            ctx.sync()
            for k in range(n):
                assert torch.equal(out[k, :f.h * f.w], want), (scene, tuple(f), rep, k, ctx.last_launch)
            assert bool((out[:, f.h * f.w:] == POISON).all())
            got = _check_launch(ctx, E.expected(f, rep, LDS[scene], nframes=n, cams=True), (scene, tuple(f), rep))
            assert got.frames == n
        base = _cam(scene)
        cams = np.stack([base + np.float32(0.37 * k) * np.array([1, 0, 0] + [0] * 9, np.float32) for k in range(n)])
        out = torch.full((n, stride), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        R.render_batch_into(out.data_ptr(), f.h, f.w, ps, n, frame_stride=stride, cams=cams)
        ctx.sync()
        launch = ctx.last_launch
        got = out.cpu().numpy()
        for k in range(n):
            one = R.render_image(ps, f.w, f.h, cams[k])
            assert int((got[k, :f.h * f.w].reshape(f.h, f.w) != one).sum()) == 0, (scene, tuple(f), k, launch)
        assert (got[:, f.h * f.w:] == POISON).all()
        ps.free()
        # the same view again and again (no camera array: the prepared camera, which is the square one), on a scene that has rendered nothing yet:
        # the first batch records, the second is drawn through the tile order
        ps = _prepared(R, ctx, scene)
        assert ps.camera().tobytes() == base.tobytes()
        for rep in (1, 2):
            out.fill_(POISON)
            torch.cuda.synchronize()
            R.render_batch_into(out.data_ptr(), f.h, f.w, ps, n, frame_stride=stride)
            ctx.sync()
            for k in range(n):
                assert torch.equal(out[k, :f.h * f.w], want), (scene, tuple(f), "one view", rep, k, ctx.last_launch)
            _check_launch(ctx, E.expected(f, rep, LDS[scene], nframes=n), (scene, tuple(f), "one view", rep))
        ps.free()


def test_position_bound_is_refused(R, ctx):
    """512 frames of 1 x 2^20 are 2^26 positions: refused with the bound in the message, before anything is launched or written (a single-device and
    a multi-device context).  Frames of 1 x 1 cannot get there: a batch has at most 4096 frames, and that older limit answers first."""
    import torch
    h, w = E.BOUND_FRAME
    out = torch.full((4096,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ps = _prepared(R, ctx, "rgbbox")
    mc = R.Context(devices=[0, 0])
    mps = R.prepare_scene(E.SQUARE[0], E.SQUARE[1], mc.scene("rgbbox"))
    for c, p in ((ctx, ps), (mc, mps)):
        with pytest.raises(R.RtError, match=r"tiles per frame x frames < 2\^26"):
            R.render_batch_into(out.data_ptr(), h, w, p, E.BOUND_OUTSIDE, frame_stride=h * w)
        with pytest.raises(R.RtError, match=r"tiles per frame x frames < 2\^26"):
            R.render_batch_into(out.data_ptr(), h, w, p, E.BOUND_OUTSIDE + 1, frame_stride=h * w)
    with pytest.raises(R.RtError, match=r"tiles per frame x frames < 2\^26"):
        R.render_inplace_into(out.data_ptr(), h, w, ps, nframes=E.BOUND_OUTSIDE, frame_stride=h * w)
    with pytest.raises(R.RtError, match="4096 frames"):
        R.render_batch_into(out.data_ptr(), 1, 1, ps, 4097, frame_stride=1)
    ctx.sync()
    mc.sync()
    assert bool((out == POISON).all())
    # both contexts still render
    px, _ = _oracle("rgbbox").render(64, 80, cam=_cam("rgbbox"))
    for c, p in ((ctx, ps), (mc, mps)):
        small = torch.full((64, 80), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        R.render_batch_into(small.data_ptr(), 64, 80, p, 1, cams=_cam("rgbbox"))
        c.sync()
        assert int((small.cpu().numpy() != px).sum()) == 0
    mps.free()
    mc.close()
    ps.free()


def test_largest_batch_of_1x1_frames(R, ctx):
    """4096 frames of 1 x 1 with frame_stride = 1, the largest batch of such frames there is: every frame is the oracle's single pixel."""
    import torch
    ps = _prepared(R, ctx, "rgbbox")
    out = torch.full((4096 + 8,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    R.render_batch_into(out.data_ptr(), 1, 1, ps, 4096, frame_stride=1, cams=np.tile(_cam("rgbbox"), 4096))
    ctx.sync()
    want = _want("rgbbox", 1, 1).reshape(())
    assert bool((out[:4096] == want).all()) and bool((out[4096:] == POISON).all()), ctx.last_launch
    ps.free()


def test_batch_just_inside_the_position_bound(R, ctx):
    """511 frames of 1 x 2^20, rgbbox: 2^26 - 2^17 positions, the largest batch of this frame the bound admits (2 GB of pixels), every frame equal
    to the oracle's, compared on the device.  The accept side AT the bound (2^26 - 1 positions) rests on the CPU check of the arithmetic alone
    (test_frame_edges_cpu.py): no frame shape within the other limits gives that product."""
    import torch
    h, w = E.BOUND_FRAME
    n = E.BOUND_INSIDE
    ps = _prepared(R, ctx, "rgbbox")
    want = _want("rgbbox", h, w).reshape(-1)
    out = torch.full((n, w), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R.render_batch_into(out.data_ptr(), h, w, ps, n, frame_stride=h * w, cams=np.tile(_cam("rgbbox"), n))
    ctx.sync()
    print(f"511 frames of 1 x 2^20: {time.perf_counter() - t0:.2f} s; {ctx.last_launch}")
    bad = 0
    for k0 in range(0, n, 64):      # (in slices: the comparison's temporaries stay small)
        bad += int((out[k0:k0 + 64] != want).sum())
    assert bad == 0, (bad, ctx.last_launch)
    got = E.parse_launch(ctx.last_launch)
    assert got.frames == n and got.tiles == 131072 and got.frames * got.tiles < E.MAX_POSITIONS
    ps.free()


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("h,w", E.REFUSED, ids=lambda v: str(v))
def test_sizes_out_of_range_are_refused(R, ctx, h, w):
    """A side beyond 2^20, or more than 2^30 pixels: "image size out of range" from every entry that takes a size, nothing written, and the next
    valid render on the same context is correct.  (The buffers of the side cases have the refused frame's size -- 32 MB -- so that a library
    without the check would render into memory it owns; the area case, 4 GB, gets a small one: the call fails before using it.)"""
    import torch
    n = h * w if h * w < 1 << 24 else 4096
    out = torch.full((2 * n,), POISON, dtype=torch.int32, device="cuda")
    rays = torch.full((6 * n,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ps = R.prepare_scene(64, 80, ctx.scene("rgbbox"))
    mc = R.Context(devices=[0, 0])
    mps = R.prepare_scene(64, 80, mc.scene("rgbbox"))
    cam = _cam("rgbbox")
    calls = {
        "render_into": lambda: R.render_into(out.data_ptr(), h, w, ps, cam=cam),
        "render_into, prepared camera": lambda: R.render_into(out.data_ptr(), h, w, ps),
        "render_batch_into": lambda: R.render_batch_into(out.data_ptr(), h, w, ps, 2, frame_stride=h * w),
        "render_inplace_into": lambda: R.render_inplace_into(out.data_ptr(), h, w, ps, cams=cam),
        "camera_rays_into": lambda: R.camera_rays_into(rays.data_ptr(), h, w, ps, cam),
        "multi-device render_into": lambda: R.render_into(out.data_ptr(), h, w, mps),
        "multi-device render_batch_into": lambda: R.render_batch_into(out.data_ptr(), h, w, mps, 2, frame_stride=h * w),
    }
    for name, call in calls.items():
        with pytest.raises(R.RtError, match="image size out of range"):
            call()
            pytest.fail(f"{name} accepted a {h} x {w} frame")
    ctx.sync()
    mc.sync()
    assert bool((out == POISON).all()) and bool((rays == -1.0).all())
    want, _ = _oracle("rgbbox").render(64, 80)
    for p in (ps, mps):
        assert int((R.render(64, 80, p) != want).sum()) == 0
    mps.free()
    mc.close()
    ps.free()


# ---------------------------------------------------------------------------------------------------------------- table caches
def test_a_view_survives_the_eviction_of_the_contexts_tables(R):
    """A context keeps 16 u / v tables and 16 first orders and evicts the oldest.  A view (32 768 x 16: a first order, then its pixel list) is
    rendered, 29 other sizes -- 20 of them with first orders of their own -- pass through the same context from another prepared scene, and the
    view's next frames still equal the oracle and still draw from its list."""
    c = _context(R)
    scene = "irreg"
    first = E.PAIRS["first_order_tiles_y"][0]
    ps = _prepared(R, c, scene)
    other = _prepared(R, c, scene)
    _frames(R, c, ps, scene, first, (1, 2, 3))
    sizes = [s for s in E.oracle_sizes() if s != (first.h, first.w)] + [(f.h, f.w) for f in E.LARGEST] + [(16 + 8 * i, 24) for i in range(18)]
    assert len(sizes) > 16 and sum(1 for h, w in sizes if 1 < -(-h // 8) <= 4096 and -(-w // 8) <= 32768) > 16
    for h, w in sizes:
        _frames(R, c, other, scene, E.Frame(h, w), (1,))
    got = _frames(R, c, ps, scene, first, (4, 5))
    assert all(g.tickets == "pixel-list" for g in got)
    # ... and a new view of the first size gets a first order again (its table was evicted and is rebuilt)
    got = _frames(R, c, other, scene, first, (1, 2))
    assert got[0].tickets == "tiles-bit-reversed"
    other.free()
    ps.free()
    c.close()


# ---------------------------------------------------------------------------------------------------------------- camera rays
def test_camera_rays_at_the_side_limit(R, ctx):
    """rt_camera_rays at (8, 2^20) through the explicit camera: 2^23 rays, bit for bit the restatement's (tests/ray_query_ref.py)."""
    import torch
    h, w = 8, 1 << 20
    ps = _prepared(R, ctx, "irreg")
    cam = _cam("irreg")
    rays = torch.full((h * w, 6), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    R.camera_rays_into(rays.data_ptr(), h, w, ps, cam)
    ctx.sync()
    want = torch.from_numpy(np.ascontiguousarray(Q.camera_rays(cam, h, w), dtype=np.float32).reshape(h * w, 6)).cuda()
    assert torch.equal(rays.view(torch.int32), want.view(torch.int32))
    ps.free()
