"""Per-tile entry lists on the CPU (lane_core.h: tile_rays, tile_verdict, tile_frontier, tile_entry): tools/entry_check.cpp
builds every tile's bounds and list with the product's functions over the product's records and walks every primary ray from the root and
from its list -- the same leaves must be tested either way, every ray's 1 / d_k must lie inside its tile's bounds -- for the uncapped frontier
and for the packed list the kernel reads.  Tile verdicts are checked against rays sampled inside the bounds.  Three mutants (ALLMISS decided
with <, bounds from two corners, the sign check dropped) must each be found by some case."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "entry_check")
F = np.float32


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/entry_check"], cwd=ROOT, check=True)
    return EXE


def _run(args):
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout.strip())
    f = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    return {k: (v if k == "scene" else float(v) if "." in v else int(v)) for k, v in f.items()}


def frame(exe, scene, cam, h, w, filt=1, mutant=0, step=1):
    return _run([exe, "frame", scene, cam, str(h), str(w), str(filt), str(mutant), str(step)])


# ------------------------------------------------------------------------------------------------ scenes and cameras written for the tool
def _wall(m=12, spacing=1.5, radius=0.25):
    """m x m small spheres in the plane z = 0, some standing forward (tests/test_leaf_box_gpu.py: the same wall)"""
    i, j = np.divmod(np.arange(m * m), m)
    s = np.zeros((m * m, 7), F)
    s[:, 0] = (i - (m - 1) / 2) * spacing
    s[:, 1] = (j - (m - 1) / 2) * spacing
    s[:, 3:6] = np.linspace(0.3, 1.0, 3 * m * m, dtype=F).reshape(-1, 3)
    s[:, 6] = radius
    s[::7, 2] = 0.75
    s[::7, 6] = 0.5
    return s


def _axis_cam(z):
    """looking exactly down the z axis: the centre column's d_x and the centre row's d_y are 0, the tiles around them hold both signs"""
    return np.array([0.0, 0.0, z, -0.5, -0.5, z - 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], F)


def _rolled_cam():
    """the image plane rolled by 45 degrees: d_y = l_y + 0.7 u + 0.7 v takes its extremes at the corners (last column, first row) and
    (first column, last row) -- not the two the two-corner mutant looks at"""
    return np.array([0, 0, 30, 0, -0.7, 29, 0.7, 0.7, 0, -0.7, 0.7, 0], F)


def _two():
    s = np.zeros((2, 7), F)
    s[0] = (-1.2, 0.0, 0.0, 0.9, 0.3, 0.3, 1.0)
    s[1] = (1.2, 0.0, 0.0, 0.3, 0.3, 0.9, 1.0)
    return s


def _dupes():
    """every sphere three times: equal Morton keys, leaves that tie"""
    rng = np.random.default_rng(5)
    s = np.zeros((40, 7), F)
    s[:, 0:3] = rng.uniform(-6, 6, (40, 3))
    s[:, 3:6] = rng.uniform(0.3, 1.0, (40, 3))
    s[:, 6] = rng.uniform(0.5, 1.5, 40)
    return np.repeat(s, 3, axis=0)


def _look(spheres, look_from, look_at, fov, h, w):
    return O.OracleScene("custom", spheres7=spheres, look_from=look_from, look_at=look_at, fov=fov).camera_floats(h, w)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("entry")
    out = {}
    for name, arr in (("wall", _wall()), ("two", _two()), ("dupes", _dupes()), ("axis30", _axis_cam(30.0)), ("axis3", _axis_cam(3.0)),
                      ("axis_inside", _axis_cam(0.5)), ("rolled", _rolled_cam()),
                      ("two_cam", _look(_two(), (0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 50.0, 40, 56)),
                      ("dupes_cam", _look(_dupes(), (3.0, 10.0, 35.0), (0.0, 0.0, 0.0), 40.0, 97, 131)),
                      # inside the box of the sphere at the wall's corner cell (centre (0.75, 0.75, 0), radius 0.25), outside the sphere itself
                      ("in_box_cam", _look(_wall(), (0.95, 0.95, 0.2), (-8.0, -8.0, 0.0), 70.0, 64, 64))):
        p = d / f"{name}.f32"
        np.ascontiguousarray(arr, F).tofile(p)
        out[name] = str(p)
    return out


def _sound(f):
    assert (f["bound_violations"], f["set_violations"]) == (0, 0), f
    assert f["items_list"] <= f["items_root"] and f["items_packed"] <= f["items_root"] and f["items_list"] <= f["items_packed"], f


# ------------------------------------------------------------------------------------------------ the frames
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("h,w", [(64, 64), (200, 200), (29, 37), (1, 1), (8, 8)])
@pytest.mark.parametrize("scene", ["rgbbox", "irreg"])
def test_same_leaves_from_the_list_as_from_the_root(exe, scene, h, w, filt):
    f = frame(exe, scene, "-", h, w, filt)
    _sound(f)
    assert f["rays"] == h * w and f["tiles"] == ((h + 7) // 8) * ((w + 7) // 8), f


def test_edge_scenes_and_cameras(exe, files):
    f = frame(exe, files["two"], files["two_cam"], 40, 56, 0)
    _sound(f)
    assert f["packed_lists"] > 0 and f["inner_mean"] == 0 and f["leaf_mean"] == 2, f      # the root's two leaf children, no inner item
    _sound(frame(exe, files["two"], files["two_cam"], 40, 56, 1))
    for filt in (0, 1):
        _sound(frame(exe, files["dupes"], files["dupes_cam"], 97, 131, filt))
        _sound(frame(exe, files["wall"], files["in_box_cam"], 64, 64, filt))
        _sound(frame(exe, files["wall"], files["rolled"], 64, 64, filt))
    # down the axis: 64 x 64 has its centre column and row ON tile borders (u = 0.5 at column 32: a corner with d_x = 0); 37 x 29 inside tiles
    for cam, h, w in (("axis30", 64, 64), ("axis3", 29, 37), ("axis_inside", 64, 64), ("axis30", 29, 37)):
        f = frame(exe, files["wall"], files[cam], h, w, 1)
        _sound(f)
        assert f["no_list"] >= (h + 7) // 8 + (w + 7) // 8 - 1, f     # at least the centre column's and the centre row's tiles


# ------------------------------------------------------------------------------------------------ verdicts and mutants
def test_verdicts_against_sampled_rays(exe):
    f = _run([exe, "verdicts", "0"])
    assert f["verdict_errors"] == 0 and min(f["mixed"], f["allhit"], f["allmiss"]) > 1000, f


def test_the_mutants_are_found(exe, files):
    """1: `<` where ALLMISS needs `<=` calls a tile whose origin lies ON a far face MIXED (sound, but not the rule: the stated verdicts fail);
    2: two corners miss the extremes of a rolled image plane; 3: without the sign check a tile that holds both signs of d_x gets bounds its
    rays lie outside of"""
    assert _run([exe, "verdicts", "1"])["verdict_errors"] > 0
    base, two = frame(exe, files["wall"], files["rolled"], 64, 64, 1, 0), frame(exe, files["wall"], files["rolled"], 64, 64, 1, 2)
    assert base["bound_violations"] == 0 and two["bound_violations"] > 0, two
    for cam, h, w in (("axis30", 64, 64), ("axis3", 29, 37), ("axis_inside", 64, 64)):
        f = frame(exe, files["wall"], files[cam], h, w, 1, 3)
        assert f["bound_violations"] + f["set_violations"] > 0, f


# ------------------------------------------------------------------------------------------------ the counts at the bench size
def test_rgbbox_at_the_bench_size(exe):
    """1000 x 1000, unfiltered: the frontier saves 81.1 % of the primary rays' box items, a list holds 3.4 entries on average (0.5 inner items,
    2.8 leaves; p95 8, longest 13); under the product's caps (one inner item, six leaves) 65.9 %, and 69.8 % with the leaf filter the launch runs"""
    f = frame(exe, "rgbbox", "-", 1000, 1000, 0)
    _sound(f)
    assert (f["items_root"], f["items_list"], f["len_p95"], f["len_max"]) == (14206065, 2682225, 8, 13), f
    assert abs(f["saved_pct"] - 81.12) < 0.01 and abs(f["saved_pct_L6"] - 65.88) < 0.01 and f["saved_pct_packed"] == f["saved_pct_L6"], f
    g = frame(exe, "rgbbox", "-", 1000, 1000, 1)
    _sound(g)
    assert abs(g["saved_pct_packed"] - 69.77) < 0.01, g


def test_irreg_at_the_bench_size(exe):
    """1000 x 1000, unfiltered, every tile: 64.7 % uncapped, 35.2 % under the caps; lists of 5.15 entries on average (p95 10, longest 23).  (Figures
    quoted from a sample of every 25th / 36th tile -- 66 - 68 %, 38.4 %, lists of 3.3 / 9 / 17 -- differ from these: DESIGN.md 3.4b)"""
    f = frame(exe, "irreg", "-", 1000, 1000, 0)
    _sound(f)
    assert (f["items_root"], f["items_list"], f["len_p95"], f["len_max"], f["no_list"]) == (13919079, 4911143, 10, 23, 7693), f
    assert abs(f["saved_pct"] - 64.72) < 0.01 and abs(f["saved_pct_L6"] - 35.18) < 0.01 and abs(f["len_mean"] - 5.15) < 0.01, f
