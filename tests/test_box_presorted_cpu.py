"""box_hit_presorted on sign-ordered operands (lane_core.h) against box_hit_interval: the predicate of the pooled kernel's LDS-resident
instantiation, whose node records are read at addresses picked by the ray's sign offsets (tools/box_presorted_check.cpp).  Every case
checks the predicate for both children of a packed record over two intervals, the dwords read as near / far bit for bit, and that an
axis's offset bit is set exactly when `1/d < 0.0f` (-inf: yes; +inf, +-0, NaN: no).  The cases: the cross product of special values per
axis (+-0 and +-inf directions, origins on a slab, +-inf / NaN / denormal bounds) and >= 10^6 seeded random ones."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "box_presorted_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "build/box_presorted_check"], cwd=ROOT, check=True)
    return EXE


@pytest.mark.parametrize("seed", [1, 2])
def test_presorted_equals_interval(exe, seed):
    out = subprocess.run([exe, "1000000", str(seed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"(\d+) cases \((\d+) special, (\d+) random, seed \d+\): 0 predicate, 0 operand, 0 offset mismatches", out.stdout)
    assert m, out.stdout
    assert int(m.group(2)) >= 100000 and int(m.group(3)) >= 1000000, out.stdout


def test_check_sees_sign_bit_offsets(exe):
    """Offsets taken from the sign BIT of 1/d (wrong for -0 = 1/-inf and for NaN with the sign set): the check must fail."""
    out = subprocess.run([exe, "1000", "1", "1"], capture_output=True, text=True)
    assert out.returncode != 0, out.stdout
    assert not re.search(r" 0 offset mismatches", out.stdout), out.stdout
