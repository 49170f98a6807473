"""Culled renders at the limits of the culling proof's guards, on the CPU (cases: edge_cull.py).  tools/cull_guard_check.cpp takes
each case through the product's own host code -- rt::cull_scene_constants on the canonical tree, rt::cull_origin_ok per camera -- and follows
every pixel's whole ray chain with lane_core.h, every ray walked un-culled and again under the strongest limit any traversal order could apply.
Per case: the host's decision and constants equal edge_cull's float64 restatement, no ray changes its winner, the image is the oracle's, a
limit of 0.5 * best IS caught, and the case is not empty (hits, chains, boxes actually culled)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import edge_cull as E
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "cull_guard_check")
CASES = tuple(E.cases())


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/cull_guard_check"], cwd=ROOT, check=True)
    return EXE


def _fields(line):
    return dict(re.findall(r"(\w+)=(\S+)", line))


def run_tool(exe, case, tmp, halve=0):
    """(scene fields, [camera fields ...]) as printed: strings, numbers left to the caller."""
    sp, cp = os.path.join(tmp, "spheres.f32"), os.path.join(tmp, "cams.f32")
    case.spheres7.tofile(sp)
    np.stack(case.cams).astype(np.float32).tofile(cp)
    out = subprocess.run([exe, sp, cp, str(case.h), str(case.w), "50", str(halve)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("scene ") and len(lines) == 1 + len(case.cams), out.stdout
    return _fields(lines[0]), [_fields(ln) for ln in lines[1:]]


@functools.lru_cache(maxsize=None)
def oracle_images(name):
    """The oracle's image through each camera of the case (shared with the GPU leg's module when both run in one process)."""
    c = E.cases()[name]
    orc = O.OracleScene("custom", spheres7=c.spheres7, look_from=(0.0, 0.0, 1.0), look_at=(0.0, 0.0, 0.0), fov=40.0)
    return tuple(orc.render(c.h, c.w, cam=cam)[0] for cam in c.cams)


@pytest.mark.parametrize("name", CASES)
def test_guard_edge_case(exe, tmp_path, name):
    case = E.cases()[name]
    scene, cams = run_tool(exe, case, str(tmp_path))
    pixels = case.h * case.w

    # the host's decision and constants against the float64 restatement
    g = E.guards(case.spheres7, int(scene["height"]))
    assert g["ok"] == case.scene_ok
    assert int(scene["ok"]) == int(case.scene_ok), (name, scene)
    if case.scene_ok:
        assert np.float32(float.fromhex(scene["c2"])) == g["c2"] and np.float32(float.fromhex(scene["kappa"])) == g["kappa"], (name, scene, g)
    assert tuple(int(c["origin_ok"]) for c in cams) == tuple(int(o) for o in case.origin_ok), (name, cams)

    # the pixels are the oracle's, and no ray's winner changes under the strongest limit
    want = oracle_images(name)
    for i, c in enumerate(cams):
        print(name, "cam", i, {k: c[k] for k in ("rays", "hits", "primary_hits", "primary_gated", "longest_chain", "finite_w2", "boxes",
                                                  "boxes_limit", "violations")})
        assert int(c["checksum"], 16) == O.checksum(want[i]), (name, i)
        assert int(c["violations"]) == 0, (name, i, c)
        assert int(c["culled_walk"]) == int(case.scene_ok and case.origin_ok[i]), (name, i)

    # the case is not empty: >= 5 % of every camera's primary rays hit; bounce cases have a chain of 3 rays; a case expected culled has
    # boxes that fail against the limit only; the control has 5 % of them
    for i, c in enumerate(cams):
        assert 20 * int(c["primary_hits"]) >= pixels, (name, i, c["primary_hits"], pixels)
    if "bounce" in case.tags:
        assert max(int(c["longest_chain"]) for c in cams) >= 3, name
    if "rmin_hits" in case.tags:
        assert sum(int(c["rmin_hits"]) for c in cams) > 0, name
    boxes, boxes_limit = (sum(int(c[k]) for c in cams) for k in ("boxes", "boxes_limit"))
    if case.expect_culled:
        assert boxes_limit < boxes, (name, boxes, boxes_limit)
    if "control" in case.tags:
        assert boxes_limit <= 0.95 * boxes, (name, boxes, boxes_limit)

    # the gate cases gate what they say: every primary ray of some camera, or a share of them with a share on the other side (at least
    # 5 % of the image each way), and the tool's count is the float32 restatement's
    for i, c in enumerate(cams):
        assert int(c["primary_gated"]) == int(E.primary_gated(case.cams[i], case.h, case.w).sum()), (name, i)
    gated = [int(c["primary_gated"]) for c in cams]
    if "gate_all" in case.tags:
        assert max(gated) == pixels, (name, gated)
    if "gate_some" in case.tags:
        assert all(20 * k >= pixels and 20 * (pixels - k) >= pixels for k in gated), (name, gated)
    if name == "gate_zero":
        assert gated == [case.h + case.w - 1], (name, gated)      # the centre column and the centre row: W2 = inf through 1 / 0

    # non-vacuity: with the limit replaced by 0.5 * best the comparison must fail wherever a launch would be culled
    if case.expect_culled:
        _, halved = run_tool(exe, case, str(tmp_path), halve=1)
        assert sum(int(c["violations"]) for c in halved) > 0, (name, halved)


def test_pairs_differ_by_the_guard_alone():
    """Each inside / outside pair renders the same image or nearly so -- what differs is the decision."""
    cs = E.cases()
    for a, b in (("scene_in", "scene_out"), ("ratio_in", "ratio_out"), ("camera_in", "camera_out"), ("cmax_in", "cmax_out"),
                 ("rmin_at", "rmin_below"), ("height_at", "height_over"), ("height_at", "height_1023")):
        assert cs[a].expect_culled and not cs[b].expect_culled, (a, b)
        assert abs(len(cs[a].spheres7) - len(cs[b].spheres7)) <= 1
    assert cs["camera_batch"].origin_ok == (True, False, True) and not cs["camera_batch"].expect_culled
    assert len(cs["height_1023"].spheres7) == 1023 and len(cs["height_at"].spheres7) == 1024
    for c in cs.values():
        assert len(c.spheres7) <= 1100 and c.h <= 128 and c.w <= 128
