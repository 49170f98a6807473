"""The host-side predicates behind the kernels that have the twenty-wave shape's constants compiled in (rt_device.hpp), through
tools/wide_const_check.cpp: which launch shapes may take such a kernel (pooled_wide_plan: four waves, five workgroups per CU, no scene prefix in
LDS, two ray planes -- and nothing else: a kernel compiled for lds_nodes = 0 that met a staged prefix would read the wrong records), and which
compiled instantiations have the twin (pooled_wide_ok)."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "wide_const_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/wide_const_check"], cwd=ROOT, check=True)
    return EXE


def run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def fields(text):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", text)}


def test_exactly_one_plan_takes_the_flag(exe):
    """waves x workgroups per CU x prefix (none, nodes only, spheres only, both) x ray planes: the flag for one combination of the 64"""
    chosen = []
    for waves, wgs, (nodes, sph), planes in itertools.product((4, 8, 12, 16), (1, 5), ((0, 0), (40, 0), (0, 100), (40, 100)), (2, 3)):
        if fields(run(exe, "plan", waves, wgs, nodes, sph, planes))["wide"]:
            chosen.append((waves, wgs, nodes, sph, planes))
    assert chosen == [(4, 5, 0, 0, 2)], chosen


@pytest.mark.parametrize("plan", [(4, 2, 0, 0, 2), (4, 4, 0, 0, 2), (4, 6, 0, 0, 2), (5, 4, 0, 0, 2), (4, 5, 1, 0, 2), (4, 5, 0, 1, 2), (4, 5, 0, 0, 0), (4, 5, 0, 0, 1),
                                  (20, 1, 0, 0, 2), (0, 0, 0, 0, 0), (4, 5, -1, 0, 2)])
def test_neighbours_of_the_shape_keep_the_generic_kernel(exe, plan):
    assert fields(run(exe, "plan", *plan))["wide"] == 0, plan


def test_the_instantiations_that_have_a_twin(exe):
    """the four-wave render kernels that read the scene from memory: plain and CULL, each without SPILL and with both capacities -- not the kernels of a
    scene in LDS, the solo prologue's, the instrumented ones or the caller-ray loops"""
    keys = [(line.split(" ")[0], fields(line)) for line in run(exe, "keys").splitlines()]
    assert len(keys) > 50
    ok = sorted((name, f["cull"], f["spill"]) for name, f in keys if f["wide_ok"])
    assert ok == sorted([("plain", 0, 0), ("plain+CULL", 1, 0), ("plain+SPILL", 0, 1024), ("plain+CULL+SPILL", 1, 1024), ("plain+SPILL", 0, 128),
                         ("plain+CULL+SPILL", 1, 128)]), ok
    for name, f in keys:
        if f["wide_ok"]:
            assert (f["threads"], f["all_lds"], f["stats"], f["solo"], f["tail"], f["ord"], f["rays"]) == (256, 0, 0, 0, 0, 0, 0), (name, f)
