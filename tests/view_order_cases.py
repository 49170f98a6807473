"""The cases of the view-order tests: geometries, records and policies for the tile order, the pixel list and its header, and the first
order -- shared by tests/test_view_order_cpu.py (premises, mutants) and tests/test_view_order_gpu.py (the kernels), together with the
writer of tools/view_order_check's case file and the reader of its results.  Every record is a pure function of the case's name."""
import struct
import zlib

import numpy as np

import view_order_ref as V

FILL_BYTE = 0xA5
FILL_I32 = int(np.frombuffer(bytes([FILL_BYTE] * 4), dtype=np.int32)[0])
FILL_U32 = int(np.frombuffer(bytes([FILL_BYTE] * 4), dtype=np.uint32)[0])
GUARD = 256


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------------------------- tile orders
# (tiles_x, tiles_y, shards)
TILE_GEOMS = [(1, 1, 1), (7, 3, 1), (64, 32, 1), (683, 3, 1), (500, 500, 1)] + [(tx, ty, 8) for tx in (3, 8, 13, 125) for ty in (5, 125)]
TILE_GEOMS.append((400, 100, 8))      # (beyond the issue's list: 5 000 tiles per strip, three workgroups per shard -- the counts' [shard][bin][workgroup] indexing with shard > 0)
TILE_RECORDS = ("zeros", "all63", "wild", "one", "rising", "falling", "mix")


def tile_name(tx, ty, ns, rec):
    return f"tiles {tx}x{ty} x{ns} / {rec}"


def tile_record(tx, ty, ns, rec):
    n = tx * ty
    rng = _rng(tile_name(tx, ty, ns, rec))
    i = np.arange(n, dtype=np.int64)
    if rec == "zeros":
        c = np.zeros(n)
    elif rec == "all63":
        c = np.full(n, 63)
    elif rec == "wild":        # above 63 and below 0, with 62 / 63 / 64 and -1 / 0 / 1 among them
        c = rng.integers(-70, 200, n)
        edge = rng.random(n) < 0.4
        c = np.where(edge, rng.choice(np.array([-1, 0, 1, 61, 62, 63, 64, 65]), n), c)
    elif rec == "one":
        c = np.zeros(n)
        c[(2 * n) // 3] = 17
    elif rec == "rising":      # strictly: the first three below 0, everything from 66 on saturated
        c = i - 3
    elif rec == "falling":
        c = 70 - i
    elif rec == "mix":         # chain lengths as frames have them, mostly short, among lengths from every bin and past the last
        c = np.where(rng.random(n) < 0.5, np.minimum(rng.geometric(0.08, n) - 1, 90), rng.integers(0, 91, n))
    else:
        raise ValueError(rec)
    return np.clip(c, -2**31, 2**31 - 1).astype(np.int32)


def tile_cases():
    return [(tx, ty, ns, rec) for (tx, ty, ns) in TILE_GEOMS for rec in TILE_RECORDS]


def tile_order_workgroups(ntiles, nshards):
    """workgroups per shard of the tile-order sort (a PREMISE of the cases): one per 2048 tiles of a shard's share, at most 64"""
    per_shard = (ntiles + nshards - 1) // nshards
    return max(1, min(64, (per_shard + 2047) // 2048))


# ---------------------------------------------------------------------------------------------------------------- pixel lists
def part_rows(h, rpt, part, nparts):
    """the image rows of part `part` of `nparts`, in packed order: the row tiles (rpt rows each, the last one ragged) part, part + nparts, ...
    (raytracers_amd.dist.tile_rows gives the same: tests/test_view_order_cpu.py)"""
    return np.array([r for t in range(part, (h + rpt - 1) // rpt, nparts) for r in range(t * rpt, min(h, (t + 1) * rpt))], dtype=np.int64)


def _inplace(w, h, rpt, part, nparts):
    """part `part` of `nparts` of an h x w image rendered in place: out_skip as api.cpp"""
    rows = part_rows(h, rpt, part, nparts)
    assert len(rows) > rpt          # more than one row tile: out_skip matters
    return V.PxGeom(w, len(rows), rpt.bit_length() - 1, (nparts - 1) * rpt * w)


PX_GEOM_NAMES = ("1x1", "8x8", "77x1", "1x77", "53x37", "250x333", "512x512", "520x512", "1456x1448", "1600x1600",
                 "in place 53x100 rpt 8 part 0 of 3", "in place 40x300 rpt 16 part 2 of 8")


def px_geoms():
    g = {f"{w}x{r}": V.PxGeom(w, r) for (w, r) in ((1, 1), (8, 8), (77, 1), (1, 77), (53, 37), (250, 333), (512, 512), (520, 512), (1456, 1448), (1600, 1600))}
    g["in place 53x100 rpt 8 part 0 of 3"] = _inplace(53, 100, 8, 0, 3)
    g["in place 40x300 rpt 16 part 2 of 8"] = _inplace(40, 300, 16, 2, 8)
    assert tuple(g) == PX_GEOM_NAMES
    return g


PX_RECORDS = ("ones", "all255", "some0", "lanes", "chequer", "gradient", "mix")
POISON = 201      # record bytes no pixel of the part owns (a part in place: the other parts' rows)


def px_name(gname, rec, pname="default"):
    return f"px {gname} / {rec} / {pname}"


def px_record(gname, g, rec):
    rng = _rng(px_name(gname, rec))
    lrow, col = np.divmod(np.arange(g.npix, dtype=np.int64), g.w)
    if rec == "ones":
        v = np.ones(g.npix)
    elif rec == "all255":
        v = np.full(g.npix, 255)
    elif rec == "some0":
        v = np.where(rng.random(g.npix) < 0.3, 0, rng.integers(1, 6, g.npix))
    elif rec == "lanes":       # lane l of every tile holds l: 64 bins in one tile
        v = (lrow & 7) * 8 + (col & 7)
    elif rec == "chequer":     # two bins chequered inside the tiles
        v = np.where((lrow + col) & 1, 7, 2)
    elif rec == "gradient":    # every bin occupied (a part of >= 64 pixels), and the lengths past the last bin
        v = np.arange(g.npix) * 70 // max(g.npix, 1)
    elif rec == "mix":
        v = np.minimum(rng.geometric(0.2, g.npix), 255)
    else:
        raise ValueError(rec)
    out = np.full(g.record_bytes(), POISON, dtype=np.uint8)
    out[g.record_index(lrow, col)] = v.astype(np.uint8)
    return out


G_LDS = (20, 45, 65, 100, 180)       # sort_view's cadence tables: a scene that lives in LDS, one that is read from L2
G_L2 = (38, 120, 170, 230, 330)
PLAN_WAVES = 256 * 16                # what a real plan gives: 256 CUs, one workgroup of 16 waves each
DEFAULT_POLICY = V.PxPolicy((4, 3, 2, 2), G_LDS, 250, PLAN_WAVES, 5, 1)


def px_policies():
    out = {}
    for cap in (0, 5, 2**30):
        for z in (0, 1):
            for thr in ((4, 3, 2, 2), (1, 1, 1, 1), (255, 255, 255, 255)):
                out[f"hand {thr[0]},{thr[1]},{thr[2]},{thr[3]} cap {cap} zip {z}"] = V.PxPolicy(thr, G_LDS, 250, PLAN_WAVES, cap, z)
            for gname, gt in (("lds", G_LDS), ("l2", G_L2)):
                for nw in (1, PLAN_WAVES):
                    out[f"model {gname} waves {nw} cap {cap} zip {z}"] = V.PxPolicy((0, 24, 14, 9), gt, 250, nw, cap, z)
    return out


POLICY_GEOM = "250x333"
POLICY_RECORDS = ("mix", "gradient")

# ---------------------------------------------------------------------------------------------------------------- first orders
FIRST_GEOMS = [(1, 2), (3, 5), (8, 8), (125, 125), (9, 4096), (32768, 2)]

# ---------------------------------------------------------------------------------------------------------------- mutants
# mutant -> the cases that kill it: ("tile", tx, ty, ns, record) | ("px", geometry, record) | ("hdr", geometry, record, policy)
KILLERS = {
    "unstable": [("tile", 7, 3, 1, "mix"), ("tile", 13, 5, 8, "zeros"), ("px", "53x37", "chequer")],
    "ascending": [("tile", 7, 3, 1, "mix"), ("tile", 125, 125, 8, "rising"), ("px", "53x37", "mix")],
    "saturate62": [("tile", 64, 32, 1, "wild"), ("px", "8x8", "lanes")],
    "carry256": [("px", "520x512", "mix"), ("px", "1600x1600", "ones")],
    "lane_colmajor": [("px", "8x8", "ones"), ("px", "53x37", "mix")],
    "no_out_skip": [("px", "in place 53x100 rpt 8 part 0 of 3", "gradient"), ("px", "in place 40x300 rpt 16 part 2 of 8", "mix")],
    "cut_gt": [("tile", 64, 32, 1, "mix"), ("hdr", "250x333", "mix", "hand 4,3,2,2 cap 0 zip 0")],
    "solo_uncapped": [("hdr", "250x333", "mix", "hand 4,3,2,2 cap 5 zip 1"), ("hdr", "250x333", "mix", "model lds waves 4096 cap 5 zip 0")],
    "segments_reversed": [("tile", 13, 5, 8, "mix"), ("tile", 3, 5, 8, "rising")],
    "no_clamp0": [("tile", 7, 3, 1, "wild"), ("tile", 683, 3, 1, "rising")],
}


# ---------------------------------------------------------------------------------------------------------------- the tool's files
class CaseFile:
    def __init__(self):
        self.parts, self.n = [], 0

    def _ints(self, *v):
        self.parts.append(np.asarray(v, dtype=np.int32).tobytes())

    def tile_order(self, cost, tiles_x, nshards):
        self.n += 1
        self._ints(1, len(cost), tiles_x, nshards)
        self.parts.append(np.asarray(cost, dtype=np.int32).tobytes())

    def px_order(self, rec, g, pol):
        self.n += 1
        self._ints(2, *g.ints(), *pol.ints(), len(rec))
        raw = np.asarray(rec, dtype=np.uint8).tobytes()
        self.parts.append(raw + b"\0" * (-len(raw) % 4))

    def first_order(self, tiles_x, tiles_y):
        self.n += 1
        self._ints(3, tiles_x, tiles_y)

    def view(self, scene, h, w, max_depth, entry, rpt, part, nparts, frames, options):
        """scene: "rgbbox" | "irreg" | (spheres7, look_from, look_at, fov)"""
        self.n += 1
        if scene == "rgbbox":
            self._ints(4, 0)
        elif scene == "irreg":
            self._ints(4, 1)
        else:
            s7, lf, la, fov = scene
            s7 = np.ascontiguousarray(s7, dtype=np.float32)
            self._ints(4, 2, s7.shape[0])
            self.parts.append(s7.tobytes())
            self.parts.append(np.asarray(list(lf) + list(la) + [fov], dtype=np.float32).tobytes())
        self._ints(h, w, max_depth, entry, rpt, part, nparts, frames, len(options))
        for name, value in options:
            self.parts.append(name.encode().ljust(64, b"\0"))
            self._ints(value)

    def write(self, path):
        with open(path, "wb") as f:
            f.write(b"VORD" + struct.pack("<i", self.n))
            for p in self.parts:
                f.write(p)


class Results:
    """the tool's blocks, in order"""

    def __init__(self, path):
        self.raw = np.fromfile(path, dtype=np.uint8)
        self.at = 0

    def block(self, dtype=np.uint8):
        n = int(self.raw[self.at:self.at + 8].view(np.int64)[0])
        self.at += 8
        out = self.raw[self.at:self.at + n]
        self.at += n
        assert out.size == n, "the results file ends inside a block"
        return out.view(dtype)

    def guarded(self, dtype, what):
        """a synthetic case's buffer: both guards must still hold the fill; -> the data between them"""
        b = self.block()
        lo, mid, hi = b[:GUARD], b[GUARD:b.size - GUARD], b[b.size - GUARD:]
        assert (lo == FILL_BYTE).all(), f"{what}: written in front of the buffer, at guard bytes {np.flatnonzero(lo != FILL_BYTE)[:8]}"
        assert (hi == FILL_BYTE).all(), f"{what}: written behind the buffer, at guard bytes {np.flatnonzero(hi != FILL_BYTE)[:8]}"
        return mid.view(dtype)

    def done(self):
        return self.at == self.raw.size
