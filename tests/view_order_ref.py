"""Plain restatements of what the view-order sorts produce: a view's tile order with its class tables, its pixel
list, the list's 16-int header and the bit-reversed order of a view nothing is known about.  numpy and Python ints, written from
the rules in rt_device.hpp / DESIGN.md, not from the kernels: no chunks, no workgroups, no ballots, no scans -- a stable sort by one
key and a handful of counts.  TEST INFRASTRUCTURE (tests/test_view_order_cpu.py, tests/test_view_order_gpu.py).

Every function takes `mutant`: the name of ONE deliberate fault (MUTANTS); the CPU test shows that each fault changes the expected
arrays of a named case, i.e. that a kernel with that fault cannot pass the GPU test."""
import numpy as np

ORDER_CLASSES = 8        # kOrderClasses
ORDER_TABLE_DW = 16      # kOrderTableDw: ints per shard behind order[ntiles]
MAX_SHARDS = 8           # kMaxShards
PX_CLASSES = 5           # kPxClasses
PX_HDR_INTS = 16         # kPxHdrInts
BINS = 64

MUTANTS = (
    "unstable",          # equal bins in descending tile order
    "ascending",         # shortest chains first
    "saturate62",        # a bin that saturates one too early
    "carry256",          # the bins' block prefixes restart after 256 workgroups (pixel list)
    "lane_colmajor",     # a tile's pixels column by column
    "no_out_skip",       # the record of a part rendered in place read as if it were packed
    "cut_gt",            # a class holds the chains of > its cut instead of >=
    "solo_uncapped",     # the one-pixel class not capped at solo_cap pixels
    "segments_reversed", # the strips' segments of the tile order in the wrong order
    "no_clamp0",         # cost values below 0 not clamped to 0
)


def order_table_ints(ntiles):
    return ntiles + ORDER_TABLE_DW * MAX_SHARDS


# ---------------------------------------------------------------------------------------------------------------- tile order
def strips(tiles_x, tiles_y, nshards):
    """shard_of(s, 3, ...): strip s owns the tile columns [s * tiles_x // 8, (s + 1) * tiles_x // 8); its segment of the order table
    starts where the strips before it end.  One shard: the whole grid.  -> [(x0, width, segment start, tiles)]"""
    out = []
    for s in range(nshards):
        x0, x1 = s * tiles_x // nshards, (s + 1) * tiles_x // nshards
        out.append((x0, x1 - x0, x0 * tiles_y, (x1 - x0) * tiles_y))
    return out


def tile_bin(cost, mutant=None):
    top = 62 if mutant == "saturate62" else 63
    c = np.asarray(cost, dtype=np.int64)
    if mutant != "no_clamp0":
        c = np.maximum(c, 0)
    return 63 - np.minimum(c, top)


def tile_order(cost, tiles_x, tiles_y, nshards, fill, mutant=None):
    """-> (order[order_table_ints(ntiles)] int32, cost afterwards).  Strip by strip: the strip's tiles, row-major within the strip, stably
    sorted by bin into the strip's segment; behind order[ntiles] one 16-int table per strip: [c] for c < 8 the first position (relative
    to the segment) of the chains shorter than 2^(8 - c), i.e. the number of the strip's tiles with a (saturated) chain of >= 2^(8 - c) --
    class c = chains of 2^(7 - c) .. 2^(8 - c) - 1 --, [8] the strip's tile count.  Everything else keeps `fill`."""
    ntiles = tiles_x * tiles_y
    cost = np.asarray(cost, dtype=np.int32)
    assert cost.shape == (ntiles,) and nshards in (1, 8)
    out = np.full(order_table_ints(ntiles), fill, dtype=np.int32)
    st = strips(tiles_x, tiles_y, nshards)
    segs = [s[2] for s in st]
    if mutant == "segments_reversed":      # the last strip's segment first
        acc, segs = 0, [0] * nshards
        for s in reversed(range(nshards)):
            segs[s] = acc
            acc += st[s][3]
    for s, (x0, sw, _, n) in enumerate(st):
        rows, cols = np.divmod(np.arange(n, dtype=np.int64), max(sw, 1))
        tiles = rows * tiles_x + x0 + cols
        b = tile_bin(cost[tiles], mutant)
        if mutant == "ascending":
            b = -b
        if mutant == "unstable":
            perm = np.lexsort((-np.arange(n), b))
        else:
            perm = np.argsort(b, kind="stable")
        out[segs[s]:segs[s] + n] = tiles[perm]
        sat = np.minimum(np.maximum(cost[tiles].astype(np.int64), 0), 63)
        table = ntiles + ORDER_TABLE_DW * s
        for c in range(ORDER_CLASSES):
            cut = 1 << (ORDER_CLASSES - c)
            out[table + c] = int((sat > cut).sum() if mutant == "cut_gt" else (sat >= cut).sum())
        out[table + ORDER_CLASSES] = n
    return out, np.zeros(ntiles, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- pixel list
class PxGeom:
    """A part's geometry as the pixel list sees it: w columns, rows_local rows (packed numbering), the record read at
    lrow * w + col + (lrow >> rpt_log2) * out_skip."""

    def __init__(self, w, rows_local, rpt_log2=3, out_skip=0):
        self.w, self.rows_local, self.rpt_log2, self.out_skip = w, rows_local, rpt_log2, out_skip
        self.tiles_x, self.tiles_y = (w + 7) // 8, (rows_local + 7) // 8

    @property
    def ntiles(self):
        return self.tiles_x * self.tiles_y

    @property
    def npix(self):
        return self.w * self.rows_local

    def record_index(self, lrow, col, mutant=None):
        skip = 0 if mutant == "no_out_skip" else self.out_skip
        return lrow * self.w + col + (lrow >> self.rpt_log2) * skip

    def record_bytes(self):
        """bytes of record the part's pixels reach"""
        return int(self.record_index(self.rows_local - 1, self.w - 1)) + 1

    def ints(self):
        return [self.w, self.rows_local, self.rpt_log2, self.out_skip, self.tiles_x, self.tiles_y]


def px_in_tile_order(g, mutant=None):
    """The part's in-range pixels, tile by tile (row-major tiles), inside a tile by lane = (lrow & 7) * 8 + (col & 7) -> (lrow, col)"""
    tile, lane = np.divmod(np.arange(g.ntiles * 64, dtype=np.int64), 64)
    ty, tx = np.divmod(tile, g.tiles_x)
    hi, lo = lane >> 3, lane & 7
    if mutant == "lane_colmajor":
        hi, lo = lo, hi
    lrow, col = ty * 8 + hi, tx * 8 + lo
    keep = (lrow < g.rows_local) & (col < g.w)
    return lrow[keep], col[keep]


def px_bin(rays, mutant=None):
    return np.minimum(np.asarray(rays).astype(np.int64), 62 if mutant == "saturate62" else 63)


def px_histogram(rec, g, mutant=None):
    lrow, col = px_in_tile_order(g)
    return np.bincount(px_bin(rec[g.record_index(lrow, col, mutant)], mutant), minlength=BINS).astype(np.int64)


def px_workgroups(ntiles):
    """(tiles per workgroup, workgroups) of the pixel-list launches: 16 tiles each, doubled until at most 2048 workgroups (a PREMISE of
    the cases and the shape of the carry256 mutant; the list itself does not depend on it)."""
    tpb = 16
    while (ntiles + tpb - 1) // tpb > 2048:
        tpb *= 2
    return tpb, (ntiles + tpb - 1) // tpb


def px_list(rec, g, fill=0, mutant=None):
    """The part's pixels as lrow << 16 | col, sorted by (-min(rays, 63), tile index, lane): the pixels in tile order, stably sorted by
    descending saturated chain length.  Nothing here knows how many tiles a workgroup takes: the order is independent of
    tiles_per_block by construction (the 16- and 32-tile geometries of the cases prove that the kernels' is too)."""
    rec = np.asarray(rec, dtype=np.uint8)
    lrow, col = px_in_tile_order(g, mutant)
    b = px_bin(rec[g.record_index(lrow, col, mutant)], mutant)
    key = (b if mutant == "ascending" else 63 - b).astype(np.uint8)
    packed = ((lrow << 16) | col).astype(np.uint32)
    if mutant == "carry256":
        # position = the bin's start + the pixels of the bin in earlier workgroups + the rank inside the workgroup, the middle term
        # restarting at every 256th workgroup
        tpb, nblocks = px_workgroups(g.ntiles)
        block = ((lrow >> 3) * g.tiles_x + (col >> 3)) // tpb
        counts = np.zeros((BINS, nblocks), dtype=np.int64)
        np.add.at(counts, (key, block), 1)
        bin_start = np.concatenate(([0], np.cumsum(counts.sum(axis=1))))[:BINS]
        prefix = np.zeros_like(counts)
        for r0 in range(0, nblocks, 256):
            seg = counts[:, r0:r0 + 256]
            prefix[:, r0:r0 + 256] = np.cumsum(seg, axis=1) - seg
        order = np.lexsort((np.arange(key.size), block, key))
        rank = np.empty(key.size, dtype=np.int64)
        ks, bs = key[order].astype(np.int64), block[order]
        grp = ks * nblocks + bs
        first = np.concatenate(([True], grp[1:] != grp[:-1]))
        start_of = np.maximum.accumulate(np.where(first, np.arange(key.size), 0))
        rank[order] = np.arange(key.size) - start_of
        pos = bin_start[key] + prefix[key, block] + rank
        out = np.full(g.npix, fill, dtype=np.uint32)
        out[pos] = packed
        return out
    if mutant == "unstable":
        return packed[np.lexsort((-np.arange(key.size), key))]
    return packed[np.argsort(key, kind="stable")]


# ---------------------------------------------------------------------------------------------------------------- header
class PxPolicy:
    def __init__(self, thr, g, ray_ns, nwaves, solo_cap, zip_):
        self.thr, self.g, self.ray_ns, self.nwaves, self.solo_cap, self.zip = list(thr), list(g), ray_ns, nwaves, solo_cap, zip_
        assert len(self.thr) == PX_CLASSES - 1 and len(self.g) == PX_CLASSES

    def ints(self):
        return self.thr + self.g + [self.ray_ns, self.nwaves, self.solo_cap, self.zip]

    def __repr__(self):
        return f"thr={self.thr} g={self.g} ray_ns={self.ray_ns} nwaves={self.nwaves} solo_cap={self.solo_cap} zip={self.zip}"


def px_width_log2(k):
    return 0 if k == 0 else k + 2          # 1, 8, 16, 32, 64 pixels per ticket


def model_cuts(hist, pol):
    """thr[0] == 0 (rt_device.hpp, above struct PxPolicy): a wave that carries the rays of class k advances them one bounce per g[k], so
    class k + 1 may hold chains of up to T // g[k + 1] rays if the frame is to end by T -- class k takes the chains too long for it --
    and T is the larger of what the longest chain takes in the narrowest class there is and of what the waves' time adds up to: a ray
    of class k costs g[k] / width of a wave's time, one of the 64-pixel class ray_ns (in 0.1 us: / 100); at most four rounds, stopping
    when T no longer grows.  Unbounded ints.
    The comment fixes the rule, not its roundings; these are taken from px_header_kernel as part of the rule, because the cuts depend on them
    (test_view_order_cpu.test_header_restatement_by_hand has a histogram where they move a cut): every division floors; a class holds the chains of
    >= T // g + 1 rays, at most 64; each BIN's share of the waves' time is floored on its own (rays * g[k] // width, rays * ray_ns // 100) before the
    bins are added and the sum is divided by the waves; the cuts in force are those of the last T tried, also when the fourth round still raised it."""
    hist = [int(x) for x in hist]
    lengths = [l for l in range(1, BINS) if hist[l] > 0]
    maxlen = max(lengths) if lengths else 1
    solo = pol.solo_cap > 0
    T = maxlen * pol.g[0 if solo else 1]
    thr = [0] * (PX_CLASSES - 1)
    for _ in range(4):
        thr = [min(BINS, T // pol.g[k + 1] + 1) for k in range(PX_CLASSES - 1)]
        if not solo:
            thr[0] = BINS
        total = 0
        for l in range(1, BINS):
            k = PX_CLASSES - 1
            while k > 0 and l >= thr[k - 1]:
                k -= 1
            rays = hist[l] * l
            total += rays * pol.ray_ns // 100 if k == PX_CLASSES - 1 else rays * pol.g[k] // (1 << px_width_log2(k))
        Tn = max(T, total // max(1, pol.nwaves))
        if Tn <= T:
            break
        T = Tn
    return thr


def px_header(hist, pol, fill, mutant=None):
    """-> hdr[16] int32.  Cuts by hand (thr[0] > 0) or from the model; the one-pixel class starts at the first length >= max(thr[0], 1)
    that at most solo_cap pixels reach (none: no such class); every later cut is at most the one before it; class k begins at the number of
    pixels with chains of >= its cut.  px_make_header's layout: [0..5] first position of class k / the pixel count, [8..13] first ticket of
    class k / all tickets (class k: 2^width_log2(k) pixels per ticket, rounded up per class), [6] the cuts packed a byte each, [7] zip,
    [14] = [15] = 0."""
    hist = [int(x) for x in hist]
    assert len(hist) == BINS
    suf = [sum(hist[l:]) for l in range(BINS)]
    total = suf[0]

    def at_least(t):
        if mutant == "cut_gt":
            t += 1
        return total if t <= 0 else (0 if t > BINS - 1 else suf[t])

    thr = list(pol.thr) if pol.thr[0] > 0 else model_cuts(hist, pol)
    t0 = BINS
    if pol.solo_cap > 0:
        for l in range(max(thr[0], 1), BINS):
            if suf[l] <= pol.solo_cap or mutant == "solo_uncapped":
                t0 = l
                break
    t1 = min(thr[1], t0)
    t2 = min(thr[2], t1)
    t3 = min(thr[3], t2)
    pos = [0, at_least(t0), at_least(t1), at_least(t2), at_least(t3), total]
    hdr = np.full(PX_HDR_INTS, fill, dtype=np.int32)
    tick = 0
    for k in range(PX_CLASSES):
        hdr[k] = pos[k]
        hdr[8 + k] = tick
        width = 1 << px_width_log2(k)
        tick += (pos[k + 1] - pos[k] + width - 1) // width
    hdr[PX_CLASSES] = total
    hdr[8 + PX_CLASSES] = tick
    hdr[6] = t0 | (t1 << 8) | (t2 << 16) | (t3 << 24)
    hdr[7] = pol.zip
    hdr[14] = hdr[15] = 0
    return hdr


# ---------------------------------------------------------------------------------------------------------------- first order
def bit_reversed_sequence(n):
    """0 .. n-1 in the order of their bit-reversed indices (ceil(log2 n) bits)"""
    bits = (n - 1).bit_length()
    rev = [int(format(i, f"0{bits}b")[::-1], 2) if bits else 0 for i in range(n)]
    return np.argsort(np.asarray(rev), kind="stable")


def first_order(tiles_x, tiles_y):
    """The visiting order of a view nothing is known about: the tile rows in bit-reversed order and, inside a row, the blocks of 8 tiles
    in bit-reversed order of the blocks (the last block may be narrower); behind it zeroed class tables."""
    rows = bit_reversed_sequence(tiles_y)
    nb = (tiles_x + 7) // 8
    cols = np.concatenate([np.arange(8 * b, min(8 * b + 8, tiles_x)) for b in bit_reversed_sequence(nb)])
    out = np.zeros(order_table_ints(tiles_x * tiles_y), dtype=np.int32)
    out[:tiles_x * tiles_y] = (rows[:, None] * tiles_x + cols[None, :]).ravel()
    return out


# ---------------------------------------------------------------------------------------------------------------- views
def view_records(chains, w):
    """What a view's first frame records from the per-pixel chain lengths N (int [rows_local, w], the oracle's): cost_px = min(N, 255)
    and per 8x8 tile the largest N if that is >= 3, else 0."""
    rows = chains.shape[0]
    tx, ty = (w + 7) // 8, (rows + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), dtype=np.int64)
    pad[:rows, :w] = chains
    mx = pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).reshape(-1)
    return np.minimum(chains, 255).astype(np.uint8), np.where(mx >= 3, mx, 0).astype(np.int32)
