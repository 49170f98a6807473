"""Exit lists on the CPU (lane_core.h: exit_tables_path): tools/exit_check.cpp builds the pair records and the per-sphere table
with the product's function over the product's records and walks every bounce ray of a frame from the root and -- as SHADE does -- from the list
of the sphere it leaves: the same leaves must be tested either way.  The lemma the design rests on (nested boxes, a pass on the inner one => a
pass on the outer one) is run against sampled adversarial rays.  Two mutants (tables without the nesting check; lists pushed without the test
of the resume node's box) must each be found by a case.  The counts at the bench size are pinned.  The box stack's bound with lists is played
against a greedy adversary."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "exit_check")
F = np.float32
DMAX = 4


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/exit_check"], cwd=ROOT, check=True)
    return EXE


def _run(args):
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout.strip())
    f = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    return {k: (v if k in ("scene", "inner_per_depth") else int(v)) for k, v in f.items()}


def frame(exe, scene, cam, h, w, max_depth=50, mutant=0, dark=1, shrink=0):
    return _run([exe, "frame", scene, cam, str(h), str(w), str(max_depth), str(mutant), str(dark), str(shrink)])


# ------------------------------------------------------------------------------------------------ scenes and cameras written for the tool
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


def _tall(radius=None):
    """single-bit Morton codes: a chain of 30 levels against floor(log2 31) + 2 = 6 sweeps (tests/test_presorted_gpu.py: the same spheres;
    radius 6: tests/test_leaf_box_gpu.py's tall_fat, which the leaf filter admits)"""
    pts = [(1023.0, 1023.0, 1023.0)]
    for a in range(3):
        for m in range(10):
            p = [0.0, 0.0, 0.0]
            p[a] = float(2 ** m)
            pts.append(tuple(p))
    s = np.zeros((len(pts), 7), F)
    s[:, 0:3] = np.array(pts, F)
    s[:, 3:6] = np.linspace(0.3, 1.0, 3 * len(pts), dtype=F).reshape(-1, 3)
    s[:, 6] = 0.4
    s[1:, 6] = np.maximum(0.4, 0.3 * np.abs(s[1:, 0:3]).max(axis=1))
    if radius is not None:
        s[:, 6] = radius
    return s


def _grid(n, spacing=1.1, radius=0.5):
    m = int(np.ceil(np.sqrt(n)))
    i, j = np.divmod(np.arange(n), m)
    s = np.zeros((n, 7), F)
    s[:, 0] = (i - (m - 1) / 2) * spacing
    s[:, 1] = (j - (m - 1) / 2) * spacing
    s[:, 3:6] = np.linspace(0.2, 1.0, 3 * n, dtype=F).reshape(-1, 3)
    s[:, 6] = radius
    return s


def _look(spheres, look_from, look_at, fov, h, w):
    return O.OracleScene("custom", spheres7=spheres, look_from=look_from, look_at=look_at, fov=fov).camera_floats(h, w)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("exit")
    out = {}
    for name, arr in (("two", _two()), ("dupes", _dupes()), ("tall", _tall()), ("tall_fat", _tall(6.0)), ("grid33", _grid(33)),
                      ("two_cam", _look(_two(), (0.0, 0.5, 3.0), (0.0, 0.0, 0.0), 80.0, 64, 72)),
                      ("dupes_cam", _look(_dupes(), (3.0, 10.0, 35.0), (0.0, 0.0, 0.0), 40.0, 97, 131)),
                      ("tall_cam", _look(_tall(), (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0, 97, 131)),
                      ("tall_fat_cam", _look(_tall(6.0), (700.0, 640.0, 820.0), (300.0, 300.0, 300.0), 60.0, 97, 131)),
                      ("grid33_cam", _look(_grid(33), (0.0, 0.0, 4.5), (0.0, 0.0, 0.0), 90.0, 64, 72)),
                      # the grid from far outside the leaf filter's camera guard: the walk is unfiltered (a leaf child is tested whatever its slot says)
                      ("grid33_far", _look(_grid(33), (2.0, 1.0, 400.0), (0.0, 0.0, 0.0), 2.0, 64, 72))):
        p = d / f"{name}.f32"
        np.ascontiguousarray(arr, F).tofile(p)
        out[name] = str(p)
    return out


def _sound(f):
    assert f["set_violations"] == 0, f
    assert f["items_list"] <= f["items_root"] and f["lists"] + f["fallbacks"] <= f["bounce"], f


# ------------------------------------------------------------------------------------------------ the frames
@pytest.mark.parametrize("h,w", [(64, 64), (200, 136), (61, 83), (1, 1), (8, 8)])
@pytest.mark.parametrize("scene", ["rgbbox", "irreg"])
def test_same_leaves_from_the_list_as_from_the_root(exe, scene, h, w):
    for max_depth, dark in ((50, 1), (2, 1), (50, 0)):
        f = frame(exe, scene, "-", h, w, max_depth, 0, dark)
        _sound(f)
        assert f["primary"] == h * w and f["dmax"] == DMAX, f


def test_edge_scenes(exe, files):
    f = frame(exe, files["two"], files["two_cam"], 64, 72)
    _sound(f)
    assert f["spheres_with_list"] == 0 and f["lists"] == 0 and f["bounce"] > 0, f          # the root's children are leaves: no list
    f = frame(exe, files["dupes"], files["dupes_cam"], 97, 131)
    _sound(f)
    assert f["lists"] > 0, f
    f = frame(exe, files["grid33"], files["grid33_cam"], 64, 72)
    _sound(f)
    assert f["lists"] > 0 and f["filter"] == 1, f
    f = frame(exe, files["grid33"], files["grid33_far"], 64, 72)
    _sound(f)
    assert f["filter"] == 0, f


def test_a_chain_that_is_not_nested_gets_no_list(exe, files):
    """the tall tree (30 levels against 6 sweeps): its first four levels ARE nested on the floats as stored, so every sphere below them has a list;
    with the boxes of the root's inner children shrunk by 30 % (upper boxes that do not hold what lies below them) the chains through them are not
    nested, those spheres get no list, and the leaves tested stay the root walk's"""
    for name in ("tall", "tall_fat"):
        f = frame(exe, files[name], files[name + "_cam"], 97, 131)
        _sound(f)
        assert f["n"] == 31 and f["spheres_with_list"] == 28 and f["bounce"] > 0, f
        g = frame(exe, files[name], files[name + "_cam"], 97, 131, shrink=30)
        _sound(g)
        assert g["spheres_with_list"] < 28, g
    g = frame(exe, "rgbbox", "-", 200, 136, shrink=30)
    _sound(g)
    assert g["spheres_with_list"] < 400 and g["bounce"] > 0, g


# ------------------------------------------------------------------------------------------------ the lemma and the mutants
def test_the_lemma_against_sampled_rays(exe):
    f = _run([exe, "lemma", "0"])
    assert f["lemma_errors"] == 0 and f["pass_inner"] > 100000, f
    assert _run([exe, "lemma", "1"])["lemma_errors"] > 0            # (the sample does tell boxes that are not nested)


def test_the_mutants_are_found(exe, files):
    """1: without the nesting check the tall tree's chains all get a list, and rays that pass a resume node's box fail an ancestor's;
    (the shrunk upper boxes);
    2: without the test of the resume node's box its leaf children are tested by rays the root walk never brings there (the unfiltered walk)"""
    hits = {1: 0, 2: 0}
    for name, cam in (("tall", "tall_cam"), ("grid33", "grid33_far")):
        _sound(frame(exe, files[name], files[cam], 97, 131))
        hits[2] += frame(exe, files[name], files[cam], 97, 131, 50, 2)["set_violations"]
    # (chains that are not nested: the shrunk upper boxes of test_a_chain_that_is_not_nested_gets_no_list)
    for scene, cam in ((files["tall"], files["tall_cam"]), ("rgbbox", "-")):
        _sound(frame(exe, scene, cam, 97, 131, shrink=30))
        hits[1] += frame(exe, scene, cam, 97, 131, 50, 1, 1, 30)["set_violations"]
    assert hits[1] > 0 and hits[2] > 0, hits


# ------------------------------------------------------------------------------------------------ the counts at the bench size
def test_rgbbox_at_the_bench_size(exe):
    """1000 x 1000, dark stop on: 2 342 084 bounce rays expand 42 977 069 items from the root, 21 403 186 of them ancestors of the sphere the ray
    leaves; resuming at depth 4 replaces four of those by two pair items: 4 684 156 items fewer (9.9 % of the frame's 47.3 M); six rays fail their
    resume node's box and take the root; 14 rays fail an ancestor's box in the root walk (one box each: nothing below it is tested; tested each on
    its own they would fail 37); the primary rays' 14 206 065 items from the root are 4 295 025 behind the entry lists as packed
    (tools/entry_check.cpp, the launch's filter on): the frame's 47.3 M; the inner nodes per depth"""
    f = frame(exe, "rgbbox", "-", 1000, 1000)
    _sound(f)
    assert (f["anc_failed"], f["anc_failing_boxes"]) == (14, 37), f
    assert f["inner_per_depth"] == "1,2,4,8,16,32,64,86,57,41,43,33,11,1", f
    subprocess.run(["make", "-s", "build/entry_check"], cwd=ROOT, check=True)
    out = subprocess.run([os.path.join(ROOT, "build", "entry_check"), "frame", "rgbbox", "-", "1000", "1000", "1"], capture_output=True, text=True, check=True)
    e = {k: int(v) for k, v in re.findall(r"(items_\w+)=(\d+)", out.stdout)}
    assert (e["items_root"], e["items_packed"]) == (14206065, 4295025) and f["items_root"] + e["items_packed"] == 47272094, e
    assert (f["bounce"], f["items_root"], f["items_anc"], f["items_primary"]) == (2342084, 42977069, 21403186, 14206065), f
    assert (f["items_root"] - f["items_list"], f["lists"], f["fallbacks"], f["spheres_with_list"]) == (4684156, 2342078, 6, 400), f


def test_irreg_at_the_bench_size(exe):
    """the un-culled walk (irreg's kernels carry no lists: counts only): 728 608 bounce rays, 15 419 864 items, 9 779 902 of them ancestors; one
    ray fails an ancestor's box; the inner nodes per depth"""
    f = frame(exe, "irreg", "-", 1000, 1000)
    _sound(f)
    assert f["anc_failed"] == 1 and f["inner_per_depth"] == "1,2,4,8,16,32,64,128,256,512,1024,2048,3312,2592", f
    assert (f["bounce"], f["items_root"], f["items_anc"], f["items_primary"]) == (728608, 15419864, 9779902, 13919079), f
    assert (f["items_root"] - f["items_list"], f["fallbacks"]) == (1457214, 1), f


# ------------------------------------------------------------------------------------------------ the box stack's bound with lists
def _play(H, capb, choose, rounds, rng):
    """the pooled loop's stack discipline with exit lists: a SHADE runs on fewer than 64 items, finds F and may add up to 64 lists
    of 1 + DMAX / 2 items -- all of them when F + added fits KParams::exit_room = capb - 64 (H - 3) - 128, else 64 roots --; an item of depth d
    (a pair item of virtual depth 2i - 2) pushes up to two children of depth > d, inner items have depth <= H - 2.  Returns the high-water mark."""
    room = capb - 64 * max(0, H - 3) - 128
    stack, high = [], 0
    for _ in range(rounds):
        if len(stack) < 64:
            per = 1 + DMAX // 2
            if len(stack) + 64 * per <= room:
                for _ in range(64):
                    stack.extend([2 * i for i in range(DMAX // 2)] + [DMAX])   # pair items (virtual depths 0, 2, ...) and the resume node
            else:
                stack.extend([0] * 64)
        else:
            batch, stack = stack[-64:], stack[:-64]
            for d in batch:
                stack.extend(choose(d, H, rng))
        high = max(high, len(stack))
    return high


def test_box_stack_bound_with_lists():
    """greedy (every item pushes two children one level down: the deepest stack) and random adversaries stay within capb = 64 (H + 3) for every
    height the 16-wave shapes allocate; with DMAX = 4 the lists of a SHADE always fit the room (63 + 192 <= 256)"""
    rng = np.random.default_rng(3)

    def greedy(d, H, rng):
        return [d + 1, d + 1] if d + 1 <= H - 2 else []

    def random(d, H, rng):
        return [d + 1 + int(rng.integers(0, 3))] * int(rng.integers(0, 3)) if d + 1 <= H - 2 else []

    for H in range(3, 22):
        capb = 64 * (H + 3)
        assert capb - 64 * max(0, H - 3) - 128 >= 63 + 64 * (1 + DMAX // 2), H
        for choose in (greedy, random):
            high = _play(H, capb, lambda d, H, rng: [c for c in choose(d, H, rng) if c <= H - 2], 40 * H, rng)
            assert high <= capb, (H, high, capb)
