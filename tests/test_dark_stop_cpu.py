"""The render path's dark stop on the CPU (lane_core.h: light_is_dead): tools/dark_stop_check.cpp walks every pixel's bounce
chain in full with the product's own arithmetic and marks where the pooled kernel's SHADE would stop it.  No pixel may differ; the full
chains' counts and image are the oracle's, the stopped chains' counts are the ones the change was proposed with (dark_stop_cases.RGBBOX);
and the rule stated wrongly -- any ONE channel zero -- must be found."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import dark_stop_cases as D
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "dark_stop_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/dark_stop_check"], cwd=ROOT, check=True)
    return EXE


def run_tool(exe, scene, cam, h, w, max_depth=50, rule=0):
    out = subprocess.run([exe, scene, cam, str(h), str(w), str(max_depth), str(rule)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    print(out.stdout.strip())
    return {k: (int(v, 16) if k.startswith("checksum") else v if k == "scene" else int(v)) for k, v in f.items()}


def run_custom(exe, tmp, case, h, w, max_depth=50, rule=0):
    s, lf, la, fov = case
    sp, cp = os.path.join(tmp, "spheres.f32"), os.path.join(tmp, "cam.f32")
    np.ascontiguousarray(s, np.float32).tofile(sp)
    orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)
    orc.camera_floats(h, w).tofile(cp)
    return run_tool(exe, sp, cp, h, w, max_depth, rule), orc


@functools.lru_cache(maxsize=None)
def _rgbbox_oracle(h, w):
    return O.OracleScene("rgbbox").render(h, w)


@pytest.mark.parametrize("h,w", [hw for hw in D.RGBBOX if hw != (1000, 1000)])
def test_rgbbox_stopped_chains(exe, h, w):
    (rays, boxes, spheres), (rays_s, boxes_s, spheres_s), checksum, cut = D.RGBBOX[(h, w)]
    f = run_tool(exe, "rgbbox", "-", h, w)
    want, cnt = _rgbbox_oracle(h, w)
    # the full walk is the oracle's: image and all three counters
    assert f["checksum"] == O.checksum(want) == checksum
    assert (f["rays"], f["boxes"], f["spheres"]) == (cnt["rays"], cnt["box_tests"], cnt["leaf_tests"]) == (rays, boxes, spheres)
    # the stopped walk: no pixel differs, and the work left is the table's
    assert f["differ"] == 0 and f["checksum_stop"] == checksum
    assert (f["rays_stop"], f["boxes_stop"], f["spheres_stop"], f["cut"]) == (rays_s, boxes_s, spheres_s, cut)


def test_rgbbox_at_the_bench_size(exe):
    """1000 x 1000, the frame bench.py times: -16.9 % rays, -17.5 % box tests, -18.8 % sphere tests, 212 583 pixels cut, 92 237 of them after their
    second ray; 17 of the 22 chains that run all 50 bounces remain (the longest chain is still 50)."""
    (rays, boxes, spheres), (rays_s, boxes_s, spheres_s), checksum, cut = D.RGBBOX[(1000, 1000)]
    f = run_tool(exe, "rgbbox", "-", 1000, 1000)
    assert (f["rays"], f["boxes"], f["spheres"], f["checksum"]) == (rays, boxes, spheres, checksum)
    assert (f["rays_stop"], f["boxes_stop"], f["spheres_stop"], f["checksum_stop"]) == (rays_s, boxes_s, spheres_s, checksum)
    assert (f["differ"], f["cut"], f["cut_at2"], f["longest"], f["longest_stop"]) == (0, cut, 92237, 50, 50)


def test_irreg_never_stops(exe):
    """all spheres white: light stays (1, 1, 1), no chain dies"""
    f = run_tool(exe, "irreg", "-", 200, 200)
    want, cnt = O.OracleScene("irreg").render(200, 200)
    assert f["checksum"] == f["checksum_stop"] == O.checksum(want)
    assert (f["cut"], f["differ"]) == (0, 0) and f["rays_stop"] == f["rays"] == cnt["rays"]


def test_the_wrong_rule_is_found(exe):
    """'any one channel zero' stops a chain that has touched one red wall: a red pixel under the sky becomes 0"""
    f = run_tool(exe, "rgbbox", "-", 53, 77, rule=1)
    assert f["differ"] > 0 and f["checksum_stop"] != f["checksum"], f
    assert f["cut"] > D.RGBBOX[(53, 77)][3]


def test_two_walls_die_at_the_second_bounce(exe, tmp_path):
    h = w = 64
    f, orc = run_custom(exe, str(tmp_path), D.two_walls(), h, w)
    want, cnt = orc.render(h, w)
    assert f["checksum"] == O.checksum(want) and int((want != 0).sum()) == 0
    # every chain runs to the bounce budget, and every one is stopped behind its second ray
    assert f["rays"] == cnt["rays"] == 50 * h * w and f["longest"] == 50
    assert (f["rays_stop"], f["longest_stop"], f["cut"], f["cut_at2"], f["differ"]) == (2 * h * w, 2, h * w, h * w, 0)


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_light_dies_where_the_budget_ends(exe, tmp_path, max_depth):
    """two walls: light is dead behind the second scatter.  max_depth 1 and 2: the budget ends first (no second scatter: nothing is cut);
    max_depth 3: the stop takes exactly the one ray the budget had left"""
    h = w = 64
    f, orc = run_custom(exe, str(tmp_path), D.two_walls(), h, w, max_depth=max_depth)
    want, cnt = orc.render(h, w, max_depth=max_depth)
    assert f["checksum"] == f["checksum_stop"] == O.checksum(want) and f["differ"] == 0
    assert f["rays"] == cnt["rays"] == max_depth * h * w
    assert f["rays_stop"] == min(max_depth, 2) * h * w and f["cut"] == (h * w if max_depth == 3 else 0)


def test_negative_zero_channels(exe, tmp_path):
    """-0 == 0: light (-0, -0, -0) is dead; the full chain's pixel is 0 too (255.99 * -0 converts to 0)"""
    h = w = 64
    f, orc = run_custom(exe, str(tmp_path), D.negative_zero(), h, w)
    want, _ = orc.render(h, w)
    assert f["checksum"] == f["checksum_stop"] == O.checksum(want)
    assert (f["differ"], f["cut"], f["longest_stop"], f["longest"]) == (0, h * w, 2, 50)


def test_underflow_to_zero(exe, tmp_path):
    """colours of 1e-20: 1e-40 is a denormal and alive, the third product is 0"""
    h = w = 64
    f, orc = run_custom(exe, str(tmp_path), D.underflow(), h, w)
    want, _ = orc.render(h, w)
    assert f["checksum"] == f["checksum_stop"] == O.checksum(want)
    assert (f["differ"], f["cut"], f["longest_stop"], f["longest"]) == (0, h * w, 3, 50)


def test_nonfinite_colours(exe, tmp_path):
    """0 * inf and NaN are not == 0: a chain that carries them is not stopped; a chain stopped at (0, 0, 0) whose continuation meets inf and NaN
    colours stores what the full chain stores under the device's conversion (NaN -> 0).  (No oracle image here: C leaves its conversion of
    NaN undefined.)"""
    h = w = 64
    f, _ = run_custom(exe, str(tmp_path), D.nonfinite(), h, w)
    assert f["differ"] == 0 and f["checksum"] == f["checksum_stop"]
    assert 0 < f["cut"] < h * w and f["longest"] == 50 and f["longest_stop"] == 50, f


def test_coloured_floor_has_chains_to_cut(exe, tmp_path):
    """the L2-resident scene of the GPU leg is not vacuous: some of its chains go dark"""
    f, _ = run_custom(exe, str(tmp_path), D.coloured_floor(), 150, 150)
    assert f["differ"] == 0 and f["cut"] > 0 and f["rays_stop"] < f["rays"], f
