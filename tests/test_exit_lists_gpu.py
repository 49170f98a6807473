"""Exit lists on the GPU: in the pooled kernel that has the leaf filter and the dark stop compiled in and reads its colours from
LDS, a ray that has just scattered starts at the exit list of the sphere it leaves -- a node of even depth <= 4 on that sphere's chain and the
siblings above it, two to a pair record -- when it passes that node's box, else at the root.  Every image is the oracle's, bit for bit, under
exit_lists x entry_lists x dark_stop; the counting twin's figures are the CPU tool's (tools/exit_check.cpp) for the same frames; the tables
are built once per tree and again after rt_prepared_update_spheres.  (sync_policy = 1 throughout, as in test_batch_trim_gpu.py.)"""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_batch_trim_gpu as B
import test_entry_lists_gpu as E
import test_leaf_box_gpu as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DMAX = 4


@pytest.fixture(scope="module")
def R():
    import raytracers_amd as R
    return R


@functools.lru_cache(maxsize=None)
def _cpu(scene, cam, h, w, max_depth=50):
    """tools/exit_check.cpp over the same records: the bounce rays of one frame that start from a list, and that have one and fail its box"""
    subprocess.run(["make", "-s", "build/exit_check"], cwd=ROOT, check=True)
    out = subprocess.run([os.path.join(ROOT, "build", "exit_check"), "frame", scene, cam, str(h), str(w), str(max_depth)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout.strip())
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout)}


def _active(c, option):
    """the policy (api.cpp: set_exit) from what the launch says about itself: exit lists exactly in the kernel with both flags compiled in and the
    colours in LDS, unless the option is 0 (every scene of this file fits its pair records next to 16 waves)"""
    info, x = c.entry_info(), c.exit_info()
    assert x["dmax"] == DMAX, x
    assert x["active"] == (option != 0 and info["flags_const"] and info["colour_lds"]), (option, info, x)
    return x["active"]


# ------------------------------------------------------------------------------------------------ every setting of the three options
@pytest.mark.parametrize("h,w", [(64, 64), (61, 83), (136, 200)])
def test_batches_under_every_setting(R, h, w):
    """batches of 2 and 3 frames of rgbbox under exit_lists x entry_lists x dark_stop in {-1, 0}: the oracle's pixels every time, and exit lists
    exactly when all three are on (the second batch of a view: its first one records its chains and runs without the dark stop)"""
    want = E._want("rgbbox", h, w)
    c = L._ctx(R)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    seen = set()
    for nframes, (xl, el, dark) in itertools.product((2, 3), itertools.product((-1, 0), repeat=3)):
        for k, v in (("exit_lists", xl), ("entry_lists", el), ("dark_stop", dark)):
            c.set_option(k, v)
        ll = B._batch(R, c, ps, h, w, [want] * nframes, f"rgbbox {w}x{h} x{nframes} exit_lists={xl} entry_lists={el} dark_stop={dark}", settled=True)
        on = _active(c, xl)
        assert on == ((xl, el, dark) == (-1, -1, -1)), (xl, el, dark, ll, c.exit_info())
        seen.add(on)
    assert seen == {True, False}
    c.close()


def test_bounce_limits_cameras_and_parts(R):
    """max_depth 1 (no ray ever scatters into a new ray) and 2, a camera per frame, a part of a cyclic partition: the oracle's pixels, with exit
    lists wherever the launch runs the kernel that has them"""
    import torch
    h, w = 61, 83
    orc = E._orc("rgbbox")
    c = L._ctx(R)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    for md in (1, 2):
        want, _ = orc.render(h, w, max_depth=md)
        B._batch(R, c, ps, h, w, [want] * 2, f"rgbbox max_depth={md}", settled=True, max_depth=md)
        assert _active(c, -1), (md, c.last_launch)
    cams = np.tile(orc.camera_floats(h, w), (3, 1))
    cams[1, 0:3] += np.array([0.7, 0.3, -0.5], F)
    cams[2, 3:6] += np.array([-0.2, 0.1, 0.0], F)
    wants = [E._want("rgbbox", h, w, tuple(float(x) for x in cam)) for cam in cams]
    B._batch(R, c, ps, h, w, wants, "rgbbox, a camera per frame", cams=cams)
    _active(c, -1)
    rows = L.VC.part_rows(h, 8, 1, 3)
    B._batch(R, c, ps, h, w, [E._want("rgbbox", h, w)[rows]] * 2, "rgbbox part 1 of 3", settled=True, part=1, nparts=3, rows_per_tile=8)
    assert _active(c, -1), c.last_launch
    c.close()


# ------------------------------------------------------------------------------------------------ other trees
def test_two_spheres_33_spheres_and_the_tall_tree(R):
    """two spheres (the root's children are leaves: no sphere has a list, the kernel runs with empty tables), a grid of 33, and trees taller than
    their sweeps (tall_fat, which the leaf filter admits: 30 levels -- its box stacks leave room for 12 waves only, so it renders through another
    kernel, from the root -- and its first 13 spheres, 12 levels, which 16 waves hold: that one runs the kernel with exit lists).  No chain that is
    NOT nested can reach the device: the product's builders yield nested boxes in the first four levels even of these trees
    (tests/test_exit_lists_cpu.py: 28 of 31 spheres with a list, with or without the check), so what the device shows here is that trees taller
    than their sweeps render the oracle's pixels through the new code; the un-nested chain is the CPU tool's, on records it shrinks itself"""
    h, w = 64, 72
    c = L._ctx(R)
    for what, s, lf, la, fov in (("two spheres", E.SCENES["two"][0], (0.0, 0.5, 3.0), (0.0, 0.0, 0.0), 80.0),
                                 ("33 spheres", B._grid(33), (0.0, 0.0, 4.5), (0.0, 0.0, 0.0), 90.0),
                                 ("the tall tree",) + L.SCENES["tall_fat"],
                                 ("the tall tree's first 13 spheres", L.SCENES["tall_fat"][0][:13]) + L.SCENES["tall_fat"][1:]):
        ps = R.prepare_scene_from_spheres(c, s, h, w, lf, la, fov)
        orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)
        want, _ = orc.render(h, w)
        for xl in (-1, 0):
            c.set_option("exit_lists", xl)
            ll = B._batch(R, c, ps, h, w, [want] * 3, f"{what}, exit_lists={xl}", settled=True)
            on = _active(c, xl)
            print(f"{what}: exit lists {on}")
            if what == "the tall tree":
                assert not on and "waves=12" in ll, (what, xl, ll, c.exit_info())
            else:
                assert on == (xl != 0) and "waves=16" in ll, (what, xl, ll, c.entry_info(), c.exit_info())
        ps.free()
    c.close()


# ------------------------------------------------------------------------------------------------ the counting twin against the CPU tool
@pytest.mark.parametrize("h,w,falls", [(64, 64, 1), (136, 200, 0), (128, 128, 1)])
def test_the_counting_twin_counts_what_the_cpu_tool_counts(R, h, w, falls):
    """option entry_count: over a batch of two frames the scattered rays that started from a list and the ones that had a list and took the root
    are twice the CPU tool's figures for one frame (rgbbox: every sphere has a list, so their sum is every bounce ray; the stack never lacks room).
    At 64 x 64 and 128 x 128 one ray of the frame fails its resume node's box: the path that tests the root again and pushes the root item"""
    cpu = _cpu("rgbbox", "-", h, w)
    assert cpu["fallbacks"] == falls, cpu
    c = L._ctx(R, entry_count=1)
    ps = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    B._batch(R, c, ps, h, w, [E._want("rgbbox", h, w)] * 2, "rgbbox counted", settled=True)
    assert _active(c, -1)
    x = c.exit_info()
    print(f"device {x['lists']} + {x['fallbacks']}; CPU, one frame: {cpu['lists']} + {cpu['fallbacks']} of {cpu['bounce']} bounce rays")
    assert (x["lists"], x["fallbacks"]) == (2 * cpu["lists"], 2 * cpu["fallbacks"]), (x, cpu)
    assert cpu["spheres_with_list"] == 400 and cpu["lists"] + cpu["fallbacks"] == cpu["bounce"], cpu
    c.set_option("exit_lists", 0)
    B._batch(R, c, ps, h, w, [E._want("rgbbox", h, w)] * 2, "rgbbox counted, exit_lists = 0")
    x = c.exit_info()
    assert not x["active"] and (x["lists"], x["fallbacks"]) == (0, 0), x
    c.close()


# ------------------------------------------------------------------------------------------------ the tables follow the tree
def test_tables_are_built_once_per_tree_and_again_after_an_update(R):
    import torch
    h, w = 97, 131
    s, lf, la, fov = L.SCENES["dupes_near"]
    c = L._ctx(R)
    ps = R.prepare_scene_from_spheres(c, torch.from_numpy(s).cuda(), h, w, lf, la, fov)
    want, _ = L._want("dupes_near", h, w)
    for k in range(3):
        B._batch(R, c, ps, h, w, [want] * 2, f"device spheres, batch {k}")
    x = c.exit_info()
    assert x["active"] and x["tables_built"] == 1 and x["tables_kept"] >= 1, x
    rng = np.random.default_rng(9)
    s2 = s.copy()
    s2[:, 0:3] += rng.uniform(-2, 2, (len(s), 3)).astype(F)
    s2[:, 6] *= F(1.25)
    want2, _ = O.OracleScene("custom", spheres7=s2, look_from=lf, look_at=la, fov=fov).render(h, w)
    ps.update_spheres(torch.from_numpy(s2).cuda())
    for k in range(3):
        B._batch(R, c, ps, h, w, [want2] * 2, f"updated spheres, batch {k}")
    x = c.exit_info()
    assert x["active"] and x["tables_built"] == 2, x
    # another prepared scene in between: the context keeps one tree's tables
    ps2 = R.prepare_scene(h, w, E._scene(c, "rgbbox"))
    B._batch(R, c, ps2, h, w, [E._want("rgbbox", h, w)] * 2, "rgbbox in between", settled=True)
    B._batch(R, c, ps, h, w, [want2] * 2, "updated spheres again")
    x = c.exit_info()
    assert x["active"] and x["tables_built"] == 4, x
    c.close()
