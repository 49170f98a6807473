"""The twenty-wave shape's constants compiled into its kernels (rt_device.hpp: pooled_wide_plan): launches in the shape of five workgroups
of four waves per CU stage no scene prefix and keep two ray planes, and run twins of the plain / CULL / SPILL four-wave kernels that have
lds_nodes = lds_sph = 0 and ray_planes = 2 as literals.  Every image is the oracle's, bit for bit; the launch line is the generic kernel's, character
for character; whether a twin ran comes from Context.wide_info().  Option wide_const = 0 is the A/B switch: the generic kernels on the same launches.
A four-wave workgroup that DOES stage a prefix must keep the generic kernel -- the one way this change could read wrong data.
(wide_waves = 2 gives the shape at small frames; sync_policy = 1 throughout: which launch renders a frame is then the same in every run.)"""
import itertools
import re

import numpy as np
import pytest

import oracle_lib as O
import test_batch_trim_gpu as B
import test_entry_lists_gpu as E
import test_leaf_box_gpu as L

pytestmark = pytest.mark.gpu

F = np.float32
TWINS = ("plain", "plain+CULL", "plain+SPILL", "plain+CULL+SPILL")     # the instantiations that have a twin (rt_device.hpp: pooled_wide_ok)


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


def _inst(ll):
    m = re.search(r"instantiation=(\S+) .* waves=(\d+) ", ll)
    assert m, ll
    return m.group(1), int(m.group(2))


def _expect(ll):
    """under wide_waves = 2 and nothing else configured a four-wave launch IS the twenty-wave shape (api.cpp: make_plan picks it only there); the twin runs
    iff the chosen instantiation has one -- every batch does; a single frame of an ordered view may take the four-wave SOLO kernel, which has none"""
    name, waves = _inst(ll)
    return waves == 4 and name in TWINS


def _pair(R, **opts):
    """two contexts that differ in wide_const alone: the twins (the default) and the generic kernels"""
    return L._ctx(R, wide_waves=2, **opts), L._ctx(R, wide_waves=2, wide_const=0, **opts)


def _both(R, pair, prepared, fn, what, must=None):
    """the same launch on both contexts: fn(context, prepared scene, label) -> launch line.  Equal lines; the info bit as _expect says on the first,
    clear on the second.  `must`: what the bit has to be on the first (None: whatever the instantiation says)"""
    lines = []
    for c, ps, tag in zip(pair, prepared, ("wide_const=-1", "wide_const=0")):
        ll = fn(c, ps, f"{what}, {tag}")
        bit = c.wide_info()["shape_const"]
        print(f"{what}, {tag}: shape_const {bit}")
        lines.append(ll)
        assert bit == (_expect(ll) if tag == "wide_const=-1" else False), (what, tag, ll, bit)
        if must is not None and tag == "wide_const=-1":
            assert bit == must, (what, ll, bit)
    assert lines[0] == lines[1], lines
    return lines[0]


# ------------------------------------------------------------------------------------------------ the basic cases, twins against generic kernels
@pytest.mark.parametrize("h,w", [(64, 64), (61, 83), (136, 200)])
@pytest.mark.parametrize("name", ["irreg", "floor"])
def test_batches_and_frames_under_cull_and_dark_stop(R, name, h, w):
    """irreg (10 000 spheres) and the floor of 6 400, read from L2: batches of 2 and 3 frames and single frames under cull x dark_stop in {-1, 0}"""
    want = E._want(name, h, w)
    pair = _pair(R)
    prepared = [R.prepare_scene(h, w, E._scene(c, name)) for c in pair]
    seen = set()
    for cull, dark in itertools.product((-1, 0), repeat=2):
        for c in pair:
            c.set_option("cull", cull)
            c.set_option("dark_stop", dark)
        tag = f"{name} {w}x{h} cull={cull} dark_stop={dark}"
        for n in (2, 3):
            ll = _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want] * n, what, settled=n == 2), f"{tag} x{n}", must=True)
            assert f"frames={n} " in ll and "nodes=planes," in ll and "entry=root" in ll and "leaf_box=0" in ll, ll
            seen.add(_inst(ll)[0])
        for k in (1, 2):
            ll = _both(R, pair, prepared, lambda c, ps, what: B._frame(R, c, ps, h, w, want, what), f"{tag} frame {k}")
            assert _inst(ll)[1] == 4, ll
    assert "plain" in seen and seen <= set(TWINS), seen
    for c in pair:
        c.close()


# ------------------------------------------------------------------------------------------------ SPILL
@pytest.mark.parametrize("name", ["irreg", "floor"])
def test_spill_small_capacity(R, name):
    """stack_cap = 192: the box stack spills thousands of times per frame, through the twins of the test capacity"""
    h, w = 61, 83
    want = E._want(name, h, w)
    pair = _pair(R, stack_cap=192)
    prepared = [R.prepare_scene(h, w, E._scene(c, name)) for c in pair]
    for cull in (-1, 0):
        for c in pair:
            c.set_option("cull", cull)
        ll = _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want] * 3, what, settled=True), f"{name} stack_cap 192 cull={cull} x3", must=True)
        assert "+SPILL " in ll and _inst(ll)[1] == 4, ll
        ll = _both(R, pair, prepared, lambda c, ps, what: B._frame(R, c, ps, h, w, want, what), f"{name} stack_cap 192 cull={cull} frame", must=True)
        assert "+SPILL " in ll, ll
    for c in pair:
        c.close()


def test_spill_real_capacity(R):
    """90 000 spheres, a tree taller than 15 levels (the scene tests/test_gpu_parity.py spills with): the twins of the production capacity"""
    h, w = 64, 72
    want, _ = O.OracleScene("floor", n=300, k=1800.0).render(h, w)
    pair = _pair(R)
    prepared = [R.prepare_scene(h, w, c.floor(300, 1800.0)) for c in pair]
    assert prepared[0].height > 15, prepared[0].height
    for cull in (-1, 0):
        for c in pair:
            c.set_option("cull", cull)
        ll = _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want] * 2, what, settled=True), f"90 000 spheres cull={cull} x2", must=True)
        assert "+SPILL " in ll and _inst(ll)[1] == 4, ll
    ll = _both(R, pair, prepared, lambda c, ps, what: B._frame(R, c, ps, h, w, want, what), "90 000 spheres, a frame", must=True)
    assert "+SPILL " in ll, ll
    for c in pair:
        c.close()


# ------------------------------------------------------------------------------------------------ launch forms
def test_bounce_limits_cameras_and_parts(R):
    """max_depth 1 and 2, a camera per frame, part 1 of 2 of the cyclic row-tile partition"""
    h, w = 61, 83
    orc = E._orc("irreg")
    pair = _pair(R)
    prepared = [R.prepare_scene(h, w, E._scene(c, "irreg")) for c in pair]
    for md in (1, 2):
        want, _ = orc.render(h, w, max_depth=md)
        _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want] * 2, what, settled=True, max_depth=md), f"irreg max_depth={md}", must=True)
    cams = np.tile(orc.camera_floats(h, w), (3, 1))
    cams[1, 0:3] += np.array([0.7, 0.3, -0.5], F)
    cams[2, 3:6] += np.array([-0.2, 0.1, 0.0], F)
    wants = [E._want("irreg", h, w, tuple(float(x) for x in cam)) for cam in cams]
    _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, wants, what, cams=cams), "irreg, a camera per frame", must=True)
    rows = L.VC.part_rows(h, 8, 1, 2)
    part = E._want("irreg", h, w)[rows]
    _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [part] * 2, what, settled=True, part=1, nparts=2, rows_per_tile=8), "irreg part 1 of 2", must=True)
    _both(R, pair, prepared, lambda c, ps, what: B._frame(R, c, ps, h, w, part, what, part=1, nparts=2, rows_per_tile=8), "irreg part 1 of 2, a frame")
    for c in pair:
        c.close()


def test_device_spheres_prepared_then_updated(R):
    """the floor's spheres from device memory, then updated in place: the new scene's oracle image through the same kernels"""
    import torch
    h, w = 61, 83
    s, lf, la, fov = L.SCENES["floor"]
    pair = _pair(R)
    prepared = [R.prepare_scene_from_spheres(c, torch.from_numpy(s).cuda(), h, w, lf, la, fov) for c in pair]
    want = E._want("floor", h, w)
    _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want] * 2, what, settled=True), "device spheres", must=True)
    rng = np.random.default_rng(11)
    s2 = s.copy()
    s2[:, 0:3] += rng.uniform(-1.5, 1.5, (len(s), 3)).astype(F)
    s2[:, 6] *= F(1.2)
    want2, _ = O.OracleScene("custom", spheres7=s2, look_from=lf, look_at=la, fov=fov).render(h, w)
    for ps in prepared:
        ps.update_spheres(torch.from_numpy(s2).cuda())
    _both(R, pair, prepared, lambda c, ps, what: B._batch(R, c, ps, h, w, [want2] * 2, what, settled=True), "updated spheres", must=True)
    _both(R, pair, prepared, lambda c, ps, what: B._frame(R, c, ps, h, w, want2, what), "updated spheres, a frame")
    for c in pair:
        c.close()


# ------------------------------------------------------------------------------------------------ four waves WITH a prefix: the generic kernel
@pytest.mark.parametrize("name,opts,all_lds", [("rgbbox", dict(waves_per_wg=4), True), ("irreg", dict(waves_per_wg=4), False),
                                               ("irreg", dict(waves_per_wg=4, wgs_per_cu=2), False), ("irreg", dict(waves_per_wg=4, ray_planes=3), False)])
def test_a_four_wave_plan_with_a_prefix_keeps_the_generic_kernel(R, name, opts, all_lds):
    """a configured four-wave workgroup, one or two per CU (make_plan's add(wgs, 4) shapes): rgbbox then lives in LDS whole, irreg gets a prefix of
    its nodes and spheres staged -- its instantiation is one that HAS a twin, and only the plan says that it must not run: the bit is clear, the
    image the oracle's.  (nodes=sign-ordered says that rgbbox's records are all in LDS; irreg's launch stages whatever fits beside four waves.)"""
    h, w = 61, 83
    want = E._want(name, h, w)
    c = L._ctx(R, wide_waves=2, **opts)
    ps = R.prepare_scene(h, w, E._scene(c, name))
    for cull in (-1, 0):
        c.set_option("cull", cull)
        for k in (1, 2):
            ll = B._batch(R, c, ps, h, w, [want] * 2, f"{name} {opts} cull={cull} batch {k}")
            assert _inst(ll)[1] == 4 and not c.wide_info()["shape_const"], (ll, c.wide_info())
            assert ("nodes=sign-ordered," in ll) == all_lds, ll
        ll = B._frame(R, c, ps, h, w, want, f"{name} {opts} cull={cull} frame")
        assert _inst(ll)[1] == 4 and not c.wide_info()["shape_const"], (ll, c.wide_info())
    if not all_lds:
        assert _inst(ll)[0] in TWINS or "SOLO" in ll, ll
    c.close()


def test_the_configured_twenty_wave_shape_takes_the_twin(R):
    """waves_per_wg = 4 with wgs_per_cu = 5 IS the shape: no prefix, and two ray planes, asked for or not (irreg's stack of 1 088 dwords leaves a wave no
    room for the third beside four others per SIMD); wide_const = 0 switches the twin off there too"""
    h, w = 61, 83
    want = E._want("irreg", h, w)
    for planes in (0, 2):
        c = L._ctx(R, waves_per_wg=4, wgs_per_cu=5, ray_planes=planes)
        ps = R.prepare_scene(h, w, E._scene(c, "irreg"))
        ll = B._batch(R, c, ps, h, w, [want] * 2, f"irreg configured 5 x 4, ray_planes={planes}", settled=True)
        assert _inst(ll)[1] == 4 and c.wide_info()["shape_const"], (planes, ll, c.wide_info())
        c.set_option("wide_const", 0)
        assert B._batch(R, c, ps, h, w, [want] * 2, f"irreg configured 5 x 4, ray_planes={planes}, wide_const=0") == ll and not c.wide_info()["shape_const"]
        c.close()


# ------------------------------------------------------------------------------------------------ tiny scenes
def test_two_spheres_and_33_spheres(R):
    """whichever kernel the plan picks for them under wide_waves = 2: the pixels only"""
    h, w = 64, 72
    c = L._ctx(R, wide_waves=2)
    for what, s, lf, la, fov in (("two spheres", E.SCENES["two"][0], (0.0, 0.5, 3.0), (0.0, 0.0, 0.0), 80.0),
                                 ("33 spheres", B._grid(33), (0.0, 0.0, 4.5), (0.0, 0.0, 0.0), 90.0)):
        ps = R.prepare_scene_from_spheres(c, s, h, w, lf, la, fov)
        want, _ = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov).render(h, w)
        B._batch(R, c, ps, h, w, [want] * 3, what, settled=True)
        B._frame(R, c, ps, h, w, want, what + ", a frame")
        print(f"{what}: shape_const {c.wide_info()['shape_const']}")
        ps.free()
    c.close()
