"""Frames at the render path's size guards (plain Python): thin frames whose columns or rows reach 2^16 and 2^20, and batches at the bound of the
ticket arithmetic -- in inside / outside pairs that differ by the least a guard can resolve (one pixel, or one tile of 8).

What a frame sits on:
  * the pixel list packs a pixel as (local row << 16) | column, so a view gets one only while w < 65536 and rows_local < 65536 (api.cpp: find_view,
    choose_tickets) -- the LOCAL row: a part of a taller image has global rows beyond 2^16 and still qualifies;
  * the bit-reversed first order is built for 1 < tiles_y <= 4096 and tiles_x <= 32768 only;
  * the launch shape of twenty waves per CU from 100 000 tiles, px_max_tiles = 40 000, the sparse first frame up to 32 768 tiles;
  * sides <= 2^20 and h * w <= 2^30, else "image size out of range";
  * tiles per frame x frames < 2^26 for a batch (rt_device.hpp: ticket_span counts 64 slots per position in 32 bits).

Every frame is traced through the scene's SQUARE camera (the one prepare_scene derives for 500 x 500), passed explicitly: the camera derived for
an 8 x 65 535 frame looks almost entirely at the background.  Stretched over the strip, the square camera gives 1.7 (irreg) to 3.9 (rgbbox) rays
per pixel and chains up to the bounce limit.

`expected(...)` restates, from DESIGN.md 3.3 and the guards above and never by calling the library, what frame k of a view must get: the ticket
kind, whether the frame records, and whether the launch takes the wide shape.  The GPU tests compare it with `Context.last_launch`.
"""
import collections
import re

SCENES = ("rgbbox", "irreg")
SQUARE = (500, 500)        # the camera: OracleScene(scene).camera_floats(*SQUARE)

# part `part` of `nparts` (cyclic row tiles of `rpt` rows) of an h x w image
Frame = collections.namedtuple("Frame", "h w part nparts rpt", defaults=(0, 1, 8))


def part_rows(h, part=0, nparts=1, rpt=8):
    """rows of a part: its row tiles part, part + nparts, ... of ceil(h / rpt), the last one possibly short"""
    ntiles = -(-h // rpt)
    return sum(min(rpt, h - t * rpt) for t in range(part, ntiles, nparts))


def rows_local(f):
    return part_rows(f.h, f.part, f.nparts, f.rpt)


def tile_grid(f):
    """(tiles_x, tiles_y) of the part: tiles of 8 x 8 pixels over its packed rows"""
    return -(-f.w // 8), -(-rows_local(f) // 8)


# ---------------------------------------------------------------------------------------- the guard pairs
# name -> (inside, outside); None: no such frame can be rendered by a test
PAIRS = {
    "list_column": (Frame(8, 65535), Frame(8, 65536)),
    "list_row": (Frame(65535, 8), Frame(65536, 8)),
    # a part's LOCAL rows: 65 528 (global rows to 131 055) and 65 536
    "list_part_row": (Frame(131056, 8, 0, 2), Frame(131072, 8, 0, 2)),
    "first_order_tiles_y": (Frame(32768, 16), Frame(32776, 16)),
    "first_order_tiles_x": (Frame(16, 262144), Frame(16, 262152)),
}
PART_PAIR = (131056, 131072)          # h of the part pair; w = 8, nparts = 2, rows_per_tile = 8
# one tile row: outside the first order by its guard (tiles_y > 1) -- (8, 65 535) as a first frame is the case; no inside
LARGEST = (Frame(8, 1 << 20), Frame(1 << 20, 8))          # the side limit's inside: 131 072 tiles, irreg only (the twenty-wave shape)
REFUSED = ((8, (1 << 20) + 1), ((1 << 20) + 1, 8), (32768, 32769))   # side limit twice, area limit (its inside, 2^30 pixels, is out of a test's reach)
SIXTEEN_BIT = (Frame(8, 65535), Frame(8, 65536), Frame(65535, 8), Frame(65536, 8))

# the batch bound: tiles per frame x frames < 2^26, at frames one pixel high (a tile per 8 pixels, so the pixel limit nframes * frame_stride < 2^31 does not imply it)
MAX_POSITIONS = 1 << 26
BOUND_FRAME = (1, 1 << 20)            # 131 072 tiles
BOUND_INSIDE, BOUND_OUTSIDE = 511, 512


def oracle_sizes():
    """every (h, w) whose oracle frame the tests need, each once (a part's frame is the whole image)"""
    out = []
    for pair in PAIRS.values():
        for f in pair:
            if (f.h, f.w) not in out:
                out.append((f.h, f.w))
    return out


# ---------------------------------------------------------------------------------------- the expected decision
DEFAULTS = dict(pixel_order=1, first_order=1, xcd_queues=-1, px_max_tiles=40000, max_depth=50, variant=0, nframes=1, cams=False)
Decision = collections.namedtuple("Decision", "family tickets recording wide")


def expected(f, frame, scene_in_lds, **options):
    """What frame number `frame` (1-based) of a view of Frame f gets on a context with `options` (the library's defaults otherwise;
    variant: 0 / 3 the pooled family, 1 pixel, 2 persistent).  scene_in_lds: the whole scene is staged in LDS (rgbbox; not irreg)."""
    o = dict(DEFAULTS, **options)
    if o["variant"] == 1:
        return Decision("pixel", None, None, None)
    if o["variant"] == 2:
        return Decision("persistent", None, None, None)
    rows = rows_local(f)
    tiles_x, tiles_y = tile_grid(f)
    ntiles = tiles_x * tiles_y
    batch = o["nframes"] > 1
    # the wide shape (five workgroups of four waves per CU): launches of 100 000 tiles or more that are batches or beyond the list's range -- for a
    # scene that is read from L2 (one that fits in LDS keeps the 16-wave kernels)
    wide = ntiles * o["nframes"] >= 100000 and (batch or ntiles > o["px_max_tiles"]) and not scene_in_lds
    # counters: one (xcd_queues = 0), eight strips (1; single frames only), eight taking turns (the default).  The list and the first order
    # are defined over ONE queue: not over strips
    one_queue = o["xcd_queues"] != 1 or batch
    # the view may have a pixel list: the static gates, then the 16-bit packing of (local row, column)
    px_static = o["pixel_order"] == 2 or (o["pixel_order"] == 1 and o["max_depth"] > 4 and not wide and ntiles <= o["px_max_tiles"] and
                                          (ntiles >= 1024 or scene_in_lds))
    px_can = px_static and not batch and f.w < 65536 and rows < 65536 and one_queue
    if batch and o.get("cams"):       # a batch with a camera per frame has no single view to order tiles by, and records nothing
        return Decision("pooled", "tiles-raster", 0, wide)
    if batch:
        return Decision("pooled", "tiles-raster" if frame == 1 else "tiles-ordered", 1 if frame == 1 else 0, wide)
    if frame == 1:
        bitrev = o["first_order"] == 1 and one_queue and 1 < tiles_y <= 4096 and tiles_x <= 32768
        return Decision("pooled", "tiles-bit-reversed" if bitrev else "tiles-raster", 2 if px_can else 1, wide)
    return Decision("pooled", "pixel-list" if px_can and not wide else "tiles-ordered", 0, wide)


def wide_launch(num_cu):
    """(grid, waves per workgroup) of the wide shape: five workgroups of four waves per CU, the grid a multiple of 8"""
    grid = 5 * num_cu
    return grid - grid % 8 if grid >= 8 else grid, 4


_LAUNCH = re.compile(r"family=pooled tickets=([a-z-]+)(\(borrowed\))? instantiation=(\S+) frames=(\d+) tiles=(\d+) grid=(\d+) waves=(\d+) counters=(\d+)(\(turns\))? "
                     r"deep_class=(-?\d+) deep_split=(-?\d+) recording=(\d) nodes=(\S+)$")
Launch = collections.namedtuple("Launch", "family tickets borrowed instantiation frames tiles grid waves counters turns recording")


def parse_launch(s):
    """Context.last_launch -> Launch (the pooled family's fields None for the other families)"""
    m = _LAUNCH.match(s)
    if not m:
        fam = re.match(r"family=(\w+)", s)
        return Launch(fam.group(1) if fam else None, *([None] * 10))
    return Launch("pooled", m.group(1), m.group(2) is not None, m.group(3), int(m.group(4)), int(m.group(5)), int(m.group(6)), int(m.group(7)), int(m.group(8)),
                  m.group(9) is not None, int(m.group(12)))
