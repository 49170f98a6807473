"""The culling guards in two stages (rt_host.hpp: cull_stats + cull_finish): the composition equals the one-pass function it replaced,
and the statistics merged over any partition and order -- the host's model of the device reduction behind rt_prepare_scene_device and
rt_prepared_update_spheres (bvh_build.hip: launch_cull_stats) -- equal the sequential pass (tools/cull_stats_check.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cull_stats_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/cull_stats_check"], cwd=ROOT, check=True)
    return EXE


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cull_stats_two_stage(exe, seed):
    out = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 composition, 0 partition, 0 device-model mismatches" in out.stdout, out.stdout


def test_cull_stats_check_sees_fp32_cmax(exe):
    """The device model with |p_a| + r summed in fp32 instead of fp64: the check must fail (it is sensitive to the arithmetic)."""
    out = subprocess.run([exe, "1000", "1", "1"], capture_output=True, text=True)
    assert out.returncode != 0, out.stdout
    assert "MISMATCH device model" in out.stdout
