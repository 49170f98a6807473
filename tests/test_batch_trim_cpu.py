"""The host-side predicates behind the trimmed ENTRY kernels (rt_device.hpp), through tools/batch_trim_check.cpp: which compiled instantiation exists
with entry lists (pooled_entry_ok), when a launch may take the kernel that has the leaf filter and the dark stop compiled in
(pooled_entry_flags_const), how much LDS the layout with the colour table takes (pooled_col_lds_bytes) and whether it fits (pooled_col_fits), and the
ENTRY template value that follows (pooled_entry_bits)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "batch_trim_check")
LDS = 160 * 1024
LISTS, COUNT, COL, RT = 1, 2, 4, 8


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/batch_trim_check"], cwd=ROOT, check=True)
    return EXE


def run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def fields(text):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", text)}


def test_one_instantiation_has_entry_lists(exe):
    """the plain tile-ticket kernel of 16 waves on a scene in LDS, and no other: it stages sign-ordered records and honours the leaf filter"""
    keys = [(line.split(" ")[0], fields(line)) for line in run(exe, "keys").splitlines()]
    assert len(keys) > 50
    ok = [(name, f) for name, f in keys if f["entry_ok"]]
    assert len(ok) == 1, ok
    name, f = ok[0]
    assert name == "plain" and (f["threads"], f["all_lds"], f["stats"], f["solo"], f["tail"], f["ord"], f["cull"], f["spill"], f["rays"]) == (1024, 1, 0, 0, 0, 0, 0, 0, 0), f
    assert f["presort"] == 1 and f["leaf_box"] == 1, f


@pytest.mark.parametrize("leaf_box", [0, 1, 2, -1])
@pytest.mark.parametrize("dark", [0, 1, 2, -1])
def test_the_flags_are_constants_only_when_both_are_set(exe, leaf_box, dark):
    assert fields(run(exe, "flags", leaf_box, dark))["const"] == int(leaf_box != 0 and dark != 0)


def test_the_colour_layout_of_rgbbox(exe):
    """399 nodes, 400 spheres, a tree of 14 levels (box stack 64 x 17, leaf list 192), two ray planes: 7 952 bytes per wave; the records packed at
    56 bytes (22 344, rounded up to 22 352), 6 400 bytes of spheres, 6 400 of colours, 16 waves: 162 384 bytes -- 127 of the 128 blocks of 1 280"""
    t = fields(run(exe, "colbytes", 399, 400, 64 * 17, 192, 2))
    assert t == {"bytes": 22352 + 6400 + 6400 + 16 * 7952, "wave": 7952}, t
    assert t["bytes"] == 162384 and -(-t["bytes"] // 1280) == 127
    assert fields(run(exe, "fits", t["bytes"], LDS))["fits"] == 1
    # with the {d} plane (1 KB per wave more) it would not
    t3 = fields(run(exe, "colbytes", 399, 400, 64 * 17, 192, 3))
    assert t3["wave"] == 7952 + 1024 and fields(run(exe, "fits", t3["bytes"], LDS))["fits"] == 0


@pytest.mark.parametrize("nodes,sph", [(1, 2), (32, 33), (2, 3), (7, 8)])
def test_the_layout_keeps_sixteen_byte_offsets(exe, nodes, sph):
    """the spheres, the colours and the waves' regions start at multiples of 16 bytes whatever the number of 56-byte records"""
    t = fields(run(exe, "colbytes", nodes, sph, 64 * 5, 192, 3))
    rec = -(-nodes * 56 // 16) * 16
    assert t["bytes"] == rec + 32 * sph + 16 * t["wave"] and t["bytes"] % 16 == 0 and t["wave"] % 16 == 0, t


def test_fits_at_the_limit(exe):
    for b, want in ((LDS - 16, 1), (LDS, 1), (LDS + 16, 0), (0, 1)):
        assert fields(run(exe, "fits", b, LDS))["fits"] == want, b


@pytest.mark.parametrize("mode", [LISTS, COUNT])
def test_the_template_value(exe, mode):
    """both flags set: constants, and the colours in LDS where they fit and the option allows; a flag clear: the twin that reads them, which keeps
    the load from memory whatever fits"""
    def bits(leaf, dark, nbytes, col):
        return fields(run(exe, "bits", mode, leaf, dark, nbytes, LDS, col))
    assert bits(1, 1, 162384, 1) == {"entry": mode | COL, "mode": mode, "col_lds": 1, "rt_flags": 0}
    assert bits(1, 1, LDS + 16, 1)["entry"] == mode
    assert bits(1, 1, 162384, 0)["entry"] == mode
    for leaf, dark in ((0, 1), (1, 0), (0, 0)):
        for nbytes in (162384, LDS + 16):
            assert bits(leaf, dark, nbytes, 1) == {"entry": mode | RT, "mode": mode, "col_lds": 0, "rt_flags": 1}, (leaf, dark, nbytes)
