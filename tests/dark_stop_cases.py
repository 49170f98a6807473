"""Scenes and expected counts of the dark-stop tests (lane_core.h: light_is_dead), shared by test_dark_stop_cpu.py and
test_dark_stop_gpu.py.  A scene is (spheres7 float32 [n, 7] {pos.xyz, colour.rgb, radius}, look_from, look_at, fov)."""
import numpy as np

# rgbbox (h, w) -> the oracle's (rays, box tests, sphere tests), the same with every chain stopped at light == (0, 0, 0), the image's checksum
# (of both), pixels cut.  Counted on the CPU with the oracle's walk; the stopped chains with that walk left where light is zero.
RGBBOX = {
    (1000, 1000): ((4022099, 117685724, 25443619), (3342084, 97038689, 20669663), 0xfc0f53a6, 212583),
    (200, 200): ((160461, 4697273, 1013272), (133549, 3878966, 824055), 0x9082f119, 8547),
    (53, 77): ((16737, 468796, 104377), (13927, 385510, 85063), 0x5065c363, 870),
    (64, 64): ((16577, 484045, 104850), (13787, 398970, 84985), 0x7ac867c6, 864),
    (24, 40): ((3802, 105787, 23457), (3189, 86884, 19001), 0x50b7187d, 211),
    (8, 8): ((234, 6824, 1406), (211, 6011, 1184), 0xce87f83b, 7),
}

VIEW = ((0.0, 0.0, 0.25), (0.0, 0.0, -1.0), 20.0)     # between the two walls, looking at the first


def _walls(c0, c1):
    """Two facing walls -- spheres of radius 1000 whose surfaces stand at z = -0.5 and z = +0.5 -- seen from between them: a ray bounces from
    one to the other until the bounce budget is spent (convex mirrors spread the rays by e^(sqrt(2 gap / radius)) per bounce: 9 x over 50
    bounces of a 20 degree view, far from leaving the walls), taking the colours c0, c1, c0, ... in turn."""
    s = np.zeros((2, 7), np.float32)
    s[0] = (0.0, 0.0, -1000.5, *c0, 1000.0)
    s[1] = (0.0, 0.0, 1000.5, *c1, 1000.0)
    return (s,) + VIEW


def two_walls():
    """(1,0,0) then (0,1,1): light is (0,0,0) after the second bounce; the full chain runs on to max_depth"""
    return _walls((1.0, 0.0, 0.0), (0.0, 1.0, 1.0))


def negative_zero():
    """channels that are -0: light (-0, 1, 1) after one bounce, (-0, -0, -0) after two -- dead, and the full chain's pixel is 0 as well"""
    return _walls((-0.0, 1.0, 1.0), (1.0, -0.0, -0.0))


def underflow():
    """colours of 1e-20: light 1e-20, then 1e-40 (a denormal, not zero), then 0 at the third bounce"""
    return _walls((1e-20, 1e-20, 1e-20), (1e-20, 1e-20, 1e-20))


def nonfinite():
    """A black wall facing a wall of colour (inf, NaN, 1), and a small sphere of colour (inf, 0, 1) in front of the black wall.  A chain that
    meets the black wall first is dead at once and STOPPED; carried on, it meets the other wall and its light becomes 0 * inf = NaN, NaN, 0 --
    a pixel of 0 under the device's conversion all the same.  A chain that meets the small sphere first carries inf into the black wall:
    inf * 0 = NaN is not == 0, so it is NOT stopped."""
    s, lf, la, fov = _walls((0.0, 0.0, 0.0), (np.inf, np.nan, 1.0))
    s = np.concatenate([s, np.array([[0.02, 0.0, -0.35, np.inf, 0.0, 1.0, 0.05]], np.float32)])
    return s, lf, la, fov


def coloured_floor(n=80, k=480.0):
    """An n x n floor of spheres in the manner of irreg (10 000 spheres there; 6 400 here: read from L2, not LDS resident), its colours red,
    yellow and blue dealt by index: chains that touch blue and one of the others go dark."""
    cols = np.array([(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 1.0)], np.float32)
    s = np.zeros((n * n, 7), np.float32)
    i, j = np.divmod(np.arange(n * n), n)
    cell = k / n
    s[:, 0] = (-k / 2 + cell * i).astype(np.float32)
    s[:, 1] = np.float32(2.0) * ((i + j) % 2)            # every other sphere raised: neighbours reflect into each other
    s[:, 2] = (-k / 2 + cell * j).astype(np.float32)
    s[:, 3:6] = cols[np.arange(n * n) % 3]
    s[:, 6] = np.float32(cell / 2) * (1.0 + 0.3 * ((i * 7 + j * 3) % 5) / 4).astype(np.float32)   # uneven radii: neighbours overlap and shadow each other
    return s, (0.0, 12.0, 30.0), (0.0, 0.0, 0.0), 75.0
