// rt_device.hpp -- kernel parameter block and launcher declarations (host <-> .hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "lane_core.h"
#include "treelet.h"

namespace rtk {

constexpr int kTraceWords = 16;   // u64 per wave of the instrumented pooled launch's timeline (rt_render_trace)
constexpr int kStackPixel = 64;   // pixel_kernel: LDS stack entries per lane (>= any LBVH height)
// pooled_kernel: a wave's LDS region in dwords: hit keys 64 x u64, counters 64, dump 4, then the ray
// table (ray_planes x 64 float4), the box stack and the leaf list
constexpr int kPooledWaveFixedDw = 128 + 64 + 4;
constexpr int pooled_wave_dw(int ray_planes, int capb, int capl) { return kPooledWaveFixedDw + 256 * ray_planes + capb + capl; }
// the shape of twenty waves per CU: the LDS box stack a wave can have there (2 000 - 196 - 512 - 192 dwords, whole batches), and the tiny one that
// option stack_cap selects to make the SPILL kernels spill all the time (testing)
constexpr int kSpillCapb = 1088, kSpillCapbTest = 192;

// ---- the tile queue of the persistent families --------------------------------------------------
// Tickets are drawn with returning device-scope atomics; one word saturates at ~88 draws per microsecond
// (MI355X_MICROARCH.md, "dequeue"), which a 4000x4000 frame's 250 000 tiles reach, and 4096 waves drawing their first
// ticket keep it busy for ~46 us of a 0.4 ms frame.  So (a) a wave's FIRST ticket is its own number -- no atomic --
// and (b) the queue has nshards in {1, 8} counters, each on its own 128-byte line; counter s is the home of the
// workgroups with blockIdx % 8 == s (the workgroups one XCD runs).  Two layouts:
//   * the counters TAKE TURNS over one queue (interleave, the default): counter s hands out tickets s, s + 8, ... of
//     the one adaptive order over all tiles -- the deepest tiles stay first, spread over all XCDs;
//   * STRIPS: counter s owns the s-th vertical strip of tile columns with its own segment of the order table, so an
//     XCD's L2 (4 MiB, not shared with the others) serves one strip's part of the scene.
// A wave whose home counter has run dry takes tickets from the next ones (every wave fails at most once on every
// counter before it leaves); the last wave to leave zeroes the counters for the next launch on the stream.
constexpr int kQueueStride = 32;                                // dwords between the shards' counters
constexpr int kMaxShards = 8;
constexpr int kQueueExit = kQueueStride * kMaxShards;           // dword index of the counter of waves that have left
constexpr int kQueueDwords = kQueueStride * (kMaxShards + 1);
// Behind the ticket -> tile table of a view (order[0 .. ntiles)) sits one table per shard: the first position
// (relative to the shard's segment) of each of the 8 cost classes, then the shard's tile count.
constexpr int kOrderTableDw = 16;
constexpr int order_table_ints(int ntiles) { return ntiles + kOrderTableDw * kMaxShards; }

struct Shard {
  int x0, sw;      // tile columns [x0, x0 + sw)
  int seg;         // first position of the shard's segment in the order table
  int ntiles;
};
// (the number of shards is 1 << ns_log2: 1 or 8)
__host__ __device__ inline Shard shard_of(int s, int ns_log2, int tiles_x, int tiles_y) {
  const int x0 = (s * tiles_x) >> ns_log2, x1 = ((s + 1) * tiles_x) >> ns_log2;
  return Shard{x0, x1 - x0, x0 * tiles_y, (x1 - x0) * tiles_y};
}
// k-th tile of a strip, row-major within the strip -> index in the image's tile grid (one shard: the identity)
__host__ __device__ inline int shard_tile(const Shard &sh, int k, int tiles_x) {
  const int r = k / sh.sw;
  return r * tiles_x + sh.x0 + (k - r * sh.sw);
}
// Tickets of a shard with `npos` positions (tiles x frames), whose first n_deep positions are deep tiles (waves that
// draw one do not refill until it is finished): the first n_split <= n_deep of them (the deepest tiles of the order) are
// handed out in 2^ds pieces each, the other deep tiles one per ticket (several to one wave would be traced one after
// the other), the rest 2^tpt positions per ticket.
__host__ __device__ inline unsigned shard_tickets(unsigned npos, unsigned n_split, unsigned n_deep, int ds, int tpt) {
  return (n_split << ds) + (n_deep - n_split) + ((npos - n_deep + (1u << tpt) - 1u) >> tpt);
}
// ticket t < shard_tickets(...) -> the pixels it covers, as [q_next, q_end) in units of (position * 64 + pixel in tile)
struct TicketSpan { unsigned q_next, q_end; unsigned cls; };   // cls: pixel tickets only (kPxClasses - 1 for tile tickets)

// ---- pixel tickets (round 5): an ORDERED single frame's queue runs over a list of the view's PIXELS sorted by the length of
// their bounce chains (recorded by the view's first frame, px_order kernels in render_kernels.hip), longest first, cut into
// kPxClasses segments by chain length.  A ticket of class k covers 1 << kPxLog2[k] consecutive pixels of the list: the longest
// chains go out one pixel per ticket (traced by the solo loop), the next ones 8 / 16 / 32 per ticket to waves that do not refill
// while they trace them (a wave's bounce cadence grows with the rays it carries: ~8 us per bounce with 16 rays, ~17 with 40), the
// bulk 64 per ticket.  The table's header (kPxHdrInts ints, device memory, written by px_header_kernel):
//   [0 .. 5] first list position of class k (k = 5: the number of pixels)   [8 .. 13] first ticket of class k (k = 5: all tickets)
//   [6] the cuts that were used (diagnostics)   [7] != 0: the bulk's tickets are zipped
constexpr int kPxClasses = 5;
constexpr int kPxHdrInts = 16;
__host__ __device__ inline int px_log2(int cls) { return cls == 0 ? 0 : cls + 2; }   // 1, 8, 16, 32, 64 pixels
__host__ __device__ inline TicketSpan px_ticket_span(unsigned t, const int *hdr) {
  int k = 0;
  while (k + 1 < kPxClasses && t >= (unsigned)hdr[8 + k + 1]) ++k;
  TicketSpan sp;
  sp.cls = (unsigned)k;
  unsigned j = t - (unsigned)hdr[8 + k];
  if (k == kPxClasses - 1 && hdr[7] != 0) {
    // the bulk ZIPPED (hdr[7], the default): its tickets alternately from the long end and from the short end of the segment.  Sorted
    // straight through, the list ends in one- and two-ray pixels -- nothing but SHADE operations, 60 of whose 250 instructions are
    // division and square-root expansions, on every wave of the chip at once; zipped, that work runs next to the box tests of the
    // longer bulk chains all the way, and the queue ends in the middle of the bulk (chains of ~3 rays: a short drain).  irreg 1000 x 1000
    // 0.274 -> 0.249 ms, 700 x 700 -7.5 %, rgbbox 500 x 500 -7 %, 1000 x 1000 +-0 (profiles/r05/exp/e13)
    const unsigned n = (unsigned)hdr[8 + k + 1] - (unsigned)hdr[8 + k];
    j = (j & 1u) ? n - 1u - (j >> 1) : (j >> 1);
  }
  sp.q_next = (unsigned)hdr[k] + (j << px_log2(k));
  const unsigned end = sp.q_next + (1u << px_log2(k)), seg_end = (unsigned)hdr[k + 1];
  sp.q_end = end < seg_end ? end : seg_end;
  return sp;
}
// the header for a list whose classes start at the positions pos[0 .. kPxClasses] (pos[0] = 0, non-decreasing)
__host__ __device__ inline void px_make_header(const int *pos, int *hdr) {
  int tick = 0;
  for (int k = 0; k < kPxClasses; ++k) {
    hdr[k] = pos[k];
    hdr[8 + k] = tick;
    tick += (pos[k + 1] - pos[k] + (1 << px_log2(k)) - 1) >> px_log2(k);
  }
  hdr[kPxClasses] = pos[kPxClasses];
  hdr[8 + kPxClasses] = tick;
  hdr[6] = hdr[7] = hdr[14] = hdr[15] = 0;
}
__host__ __device__ inline TicketSpan ticket_span(unsigned t, unsigned seg, unsigned npos, unsigned n_split, unsigned n_deep, int ds, int tpt) {
  TicketSpan sp;
  sp.cls = kPxClasses - 1;
  if (t < (n_split << ds)) {
    const unsigned piece = 64u >> ds;
    sp.q_next = (seg + (t >> ds)) * 64u + (t & ((1u << ds) - 1u)) * piece;
    sp.q_end = sp.q_next + piece;
    sp.cls = kPxClasses - 1;
    return sp;
  }
  t -= n_split << ds;
  if (t < n_deep - n_split) {
    sp.q_next = (seg + n_split + t) * 64u;
    sp.q_end = sp.q_next + 64u;
    return sp;
  }
  const unsigned k0 = n_deep + ((t - (n_deep - n_split)) << tpt);
  const unsigned k1 = k0 + (1u << tpt) < npos ? k0 + (1u << tpt) : npos;
  sp.q_next = (seg + k0) * 64u;
  sp.q_end = (seg + k1) * 64u;
  return sp;
}

// Drawing a ticket (wave-uniform; shared by the kernel and tools/queue_check.cpp, which plays the protocol on the
// CPU).  `fetch_add(shard)` returns the shard's counter before its increment.
struct QueueConst {
  int ns_log2, tiles_x, tiles_y, nframes;
  int interleave;            // 1: the shards are not strips but every (1 << ns_log2)-th ticket of ONE queue over all tiles (geometry and tables of a single shard)
  int ds, tpt;               // deep_split, tpt_log2
  int cap_log2;              // the pieces of split tiles may occupy one in 2^cap_log2 of the waves
  int ntiles;                // all shards' tiles: the class tables sit at order[ntiles + kOrderTableDw * shard]
  const int *order;          // nullptr: no tables
  int deep_class;            // 0: no deep tiles
  const int *px;             // pixel tickets: the list's header (px_ticket_span); nullptr: tile tickets.  (One queue: interleave, or a single counter.)
  unsigned home_waves;       // waves whose home is one shard (total waves >> ns_log2)
  unsigned q_static;         // tickets [0, q_static) of every shard are the home waves' first tickets: never drawn from the counter
};
// A wave's queue state is one word (it lives in an SGPR across the whole render loop):
// bits 0-2 the shard being drawn from, bit 7 "the first draw is still to come", bits 8-15 the shards seen dry.
constexpr unsigned kQueueFirst = 0x80u;
__host__ __device__ inline unsigned queue_state_init(int home_shard, bool static_first) {
  return (unsigned)home_shard | (static_first ? kQueueFirst : 0u);
}
__host__ __device__ inline int queue_shard(unsigned state) { return (int)(state & 7u); }
// the shard whose geometry (strip, segment, class table) the ticket in hand belongs to
__host__ __device__ inline int queue_geo_shard(const QueueConst &c, unsigned state) { return c.interleave ? 0 : queue_shard(state); }
__host__ __device__ inline int queue_geo_log2(const QueueConst &c) { return c.interleave ? 0 : c.ns_log2; }
// deep tiles at the head of a shard's segment (0: none / feature off)
__host__ __device__ inline int queue_ndeep(const QueueConst &c, int shard) {
  return (c.order != nullptr && c.deep_class > 0) ? c.order[c.ntiles + kOrderTableDw * shard + c.deep_class] : 0;
}
// deep tiles handed out in pieces: the deepest ones, as many as one in 2^cap_log2 of the waves the queue (strips: the
// shard) serves can take
__host__ __device__ inline unsigned queue_nsplit(const QueueConst &c, int ndeep) {
  const int cap = (int)((c.interleave ? c.home_waves << c.ns_log2 : c.home_waves) >> (c.cap_log2 + c.ds));
  return c.ds > 0 ? (unsigned)(ndeep < cap ? ndeep : cap) : 0u;
}
template <class FetchAdd>
__host__ __device__ inline bool queue_draw(unsigned &state, const QueueConst &c, unsigned wave_rank, FetchAdd &&fetch_add, TicketSpan *sp) {
  const unsigned all = ((1u << (1 << c.ns_log2)) - 1u) << 8;
  for (;;) {   // until a shard yields a ticket or all have run dry
    const int sh = queue_shard(state);
    const int geo = c.interleave ? 0 : sh;
    const Shard s = shard_of(geo, queue_geo_log2(c), c.tiles_x, c.tiles_y);
    const unsigned npos = (unsigned)s.ntiles * (unsigned)c.nframes;
    const int ndeep = queue_ndeep(c, geo);               // (<= the shard's tiles: a position of its class table)
    const unsigned n_split = queue_nsplit(c, ndeep);
    unsigned tickets = c.px != nullptr ? (unsigned)c.px[8 + kPxClasses] : shard_tickets(npos, n_split, (unsigned)ndeep, c.ds, c.tpt);
    // interleaved: this counter's tickets are the queue's tickets sh, sh + n, sh + 2 n, ... (n counters)
    if (c.interleave) tickets = (tickets + (1u << c.ns_log2) - 1u - (unsigned)sh) >> c.ns_log2;
    unsigned t = 0;
    bool got = false;
    if (state & kQueueFirst) {
      state &= ~kQueueFirst;
      t = wave_rank;
      got = t < tickets;           // (not: the shard has no tickets beyond the static ones either)
    } else if (tickets > c.q_static) {
      t = fetch_add(sh) + c.q_static;
      got = t < tickets;
    }
    if (got) {
      if (c.interleave) t = (t << c.ns_log2) + (unsigned)sh;
      *sp = c.px != nullptr ? px_ticket_span(t, c.px) : ticket_span(t, (unsigned)s.seg, npos, n_split, (unsigned)ndeep, c.ds, c.tpt);
      return true;
    }
    state |= 0x100u << sh;
    if ((state & all) == all) return false;
    unsigned nx = (unsigned)sh;
    do nx = (nx + 1u) & ((1u << c.ns_log2) - 1u); while ((state >> (8 + nx)) & 1u);
    state = (state & ~7u) | nx;
  }
}

struct KParams {
  // scene (traversal copy; see rt::TravLayout)
  const float4 *nodes;   // [2*(n-1)]  {lo.xyz, left}, {hi.xyz, right}; child >= 0 inner, < 0 ~leaf
  const float4 *nodes64; // [4*(n-1)]  pooled family: {L.lo,left<<8} {L.hi,right<<8} {R.lo,mask_l} {R.hi,mask_r} (children's boxes; treelet masks)
  const float4 *sph;     // [n] {pos.xyz, radius}
  const float4 *col;     // [n] {colour.rgb, 1/radius}
  float root_lo[3], root_hi[3];   // the root's own box
  int n_nodes, n_sph;    // n-1, n
  Cam cam;
  // image + partition
  int w, h;              // full image
  int rows_local;        // rows of this part (packed)
  int rows_per_tile, part, nparts;
  int rpt_log2;          // log2(rows_per_tile) when it is a power of two, else -1
  int tiles_x;           // ceil(w / 8)
  int tiles_y;           // ceil(rows_local / 8) (nchunks = tiles_x * tiles_y; on the host: no integer division in the kernel)
  int max_depth;
  int32_t *out;          // [rows_local * w]  (batch launch: frame f at out + f * frame_stride)
  int out_skip;          // 0: the part's rows are PACKED at out.  In place (rt_render_part_inplace): out = the full image's row
                         // part * rows_per_tile, and the part's row tile k lies k * out_skip = k * (nparts - 1) * rows_per_tile * w
                         // elements further than in the packed layout -- every pixel is stored where the assembled image has it
                         // (that image may be another device's memory: the stores then are the framebuffer exchange)
  int nframes;           // pooled family: frames rendered by this one launch (>= 1)
  int tpt_log2;          // pooled family: a ticket of the tile queue covers 1 << tpt_log2 consecutive tiles
  int frame_stride;      // int32 elements between consecutive frames' buffers
  const Cam *cams;       // [nframes] per-frame cameras (nullptr: `cam` for every frame)
  unsigned long long *stats;   // [3] rays, box tests, sphere tests (instrumented launches only)
  unsigned long long *trace;   // [waves][kTraceWords] per-wave timeline (instrumented pooled launch only)
  // persistent family
  unsigned *queue;       // [kQueueDwords] ticket counter of shard s at [kQueueStride * s], waves that have left at [kQueueExit]; all zero between launches
  int nshards;           // 1, or 8 (pooled family, one frame per launch): one ticket counter per XCD ...
  int interleave;        // ... 0: and one strip of tile columns per counter; 1: the counters take turns over ONE queue (order table of a single shard)
  int static_first;      // pooled family: a wave's first ticket is its own number among its home counter's waves (no atomic: no ramp at launch)
  int nchunks;           // 8x8 tiles in this part
  int lds_nodes;         // breadth-first node prefix staged in LDS
  int lds_sph;           // sphere prefix staged in LDS
  int smax, lmax;        // per-lane LDS stack / deferred-leaf capacities
  int thr_shade, thr_leaf;   // phase-vote thresholds (lanes)
  // pooled family
  int capb, capl;        // per-wave box-stack / leaf-list capacities (dwords)
  int ray_planes;        // ray table: 3 = {o, a} {1/d} {d} per slot; 2 = without {d} (LEAF then pulls d with ds_bpermute: 1 KB per wave less)
  int prio_depth;        // bounce depth at which a wave raises its issue priority (0: never)
  const int *order;      // [order_table_ints(nchunks)] position -> tile (nullptr: the strips in row-major order), then the shards' class tables
  int donate;            // pooled family: > 0 = the DONATE instantiation: a wave that cannot refill and holds at most `donate` rays gives them to waiting sibling waves of its workgroup
  int cold;              // pooled family: > 0 = the COLD instantiation: a wave that cannot refill hands its last `cold` rays to the solo loop from inside the pooled loop
  int look_max;          // pooled family: a wave with this many box items or more does not look at finished folds / vacant slots (64: it looks whenever it has less than a full batch)
  int box2;              // pooled family: a wave with <= 32 box items runs the two-level BOX2 operation (0: off)
  int solo;              // pooled family: single-pixel tickets (deep_split == 6) are traced by solo_trace in a PROLOGUE ahead of the pooled loop (the SOLO instantiation; 0: off).  The hand-over of a wave's last rays from INSIDE the loop is `cold`, below
  int tl_log2;           // levels per treelet of the traversal copy (treelet.h; the masks in nodes64)
  int deep_class;        // a shard's positions below its class table's entry [deep_class] are "deep" tiles (0: feature off)
  int deep_split;        // log2 of the pieces a deep tile is handed out in (2: four tickets of two rows each; 0: whole)
  int deep_cap_log2;     // ... to at most one in 2^this of the launch's waves (5)
  int *cost;             // [nchunks] longest bounce chain seen per tile (nullptr: not recorded)
  unsigned char *cost_px;   // [h * w] with `cost`, single frames: rays traced per PIXEL (depth + 1, saturating), indexed like `out` (nullptr: not recorded)
  const int *px_hdr;     // pixel tickets (the ORD instantiation; nullptr: tile tickets): header of the view's pixel list (kPxHdrInts) ...
  const unsigned *px_list;   // ... and the list itself: (local row << 16) | column, longest bounce chains first
  int px_hold;           // bit k: a wave that draws a ticket of class k does not refill until it is finished
  int px_prio;           // ... and runs at this issue priority meanwhile (0 .. 3)
  int cull;              // pooled family, workgroups of 16 waves: != 0 = the CULL instantiations (boxes are tested against the slot's best root so far: lane_core.h, cull_limit) ...
  float cull_c2;         // ... the scene's constant in a ray's weight W2 = max|1 / d_k| * (d.d) * c2 ...
  float cull_kappa;      // ... and in the limit best + W2 (best^2 + kappa)   (api.cpp: the prepared scene's CullConst)
  int dark;              // pooled family, render launches (RAYS == 0): != 0 = a chain whose light has become exactly zero is finished as pixel 0 instead of being traced on (lane_core.h:
                         // light_is_dead).  The host's decision (api.cpp: set_dark): never with a recording launch -- the record is the FULL chain's length.  Read in SHADE and in
                         // solo_trace only.  (in the four bytes of padding ahead of u_tab: no field's offset in the argument block moves, and the block keeps its size)
  const float *u_tab;    // [w]  pixel_u(col, w)
  const float *v_tab;    // [h]  pixel_v(row, h), indexed by the FULL image row
  // pooled family, workgroups of four waves (the shape of twenty waves per CU): a box stack whose LDS capacity `capb` is BELOW its bound (64 H + 63: trees taller
  // than 15 levels) keeps its oldest items in device memory when it would overflow -- [waves][spill_stride] dwords, a wave's own region (nullptr: capb holds the bound)
  unsigned *spill;
  int spill_stride;
  int leaf_box;          // pooled family, render launches (RAYS == 0): != 0 = BOX / BOX2 append a leaf child only if the box in its slot -- the sphere's own, widened (lane_core.h:
                         // leaf_box_eps) -- passes.  The host's decision (api.cpp: set_leaf_box): the scene's slots filled and every camera of the launch inside the guard.  (in the
                         // four bytes of padding behind spill_stride: no field's offset in the argument block moves, and the block keeps its size)
  // caller-supplied rays (rt_trace_rays: the RAYS instantiations of the pixel and pooled kernels): ray i is rays[6 i .. 6 i + 6) = {o.xyz, d.xyz};
  // its colour goes to colour3[3 i ..] and / or its packed pixel to out[i] (either pointer may be nullptr, not both)
  const float *rays;
  // (... in one slot with `entry`: a launch has caller rays or tiles, never both, and the argument block keeps its size and every field its offset)
  // pooled family, render launches, the ENTRY instantiations: the launch's table of per-tile entry lists (lane_core.h: tile_entry), kEntryDw dwords
  // per tile -- with a camera per frame (`cams`) per position frame * nchunks + tile --, filled by tile_entry_kernel on the launch's stream ahead of it (nullptr: every ray starts at the root)
  union {
    float *colour3;
    const unsigned *entry;
  };
  // (... in one slot with `exit_room`, and `occluded` below with `exit_tab`: a launch has caller rays or exit lists, never both; the block keeps its size and every field its offset)
  // pooled family, render launches, the ENTRY instantiations with kEntryExit: a ray that has just scattered off sphere j starts at the exit list of j
  // instead of the root.  exit_tab: kExitPairs pair records in the 64-byte format of nodes64 -- staged in LDS behind the n_nodes real records --, then two uint4 per
  // sphere (exit_tables_kernel).  exit_room: the box-stack items one SHADE may find plus add (what capb leaves under the bound of DESIGN.md 3.1).
  union {
    int nrays;
    int exit_room;
  };
  // rt_occluded_rays (the any-hit instantiations of the pooled kernel): occluded[i] = 1 iff some leaf is reached with every box tested over
  // (ray_tlo, ray_thi) and its sphere has a root strictly inside that interval, else 0
  union {
    unsigned char *occluded;
    const float4 *exit_tab;
  };
  float ray_tlo, ray_thi;
  // rt_intersect_rays_ranged / rt_occluded_rays_ranged: ray i's own interval (ray_tlo_dev[i], ray_thi_dev[i]) in place of (ray_tlo, ray_thi); a ray
  // whose interval fails 0 <= t_min <= t_max <= 1e9 (NaN included) is a miss.  nullptr: the scalar interval (both set, or neither)
  const float *ray_tlo_dev, *ray_thi_dev;
};

// ---- device helpers shared by the kernel sources (render_kernels.hip, query_kernels.hip) --------
#if defined(__HIPCC__)
__device__ __forceinline__ int f2i(float f) { return __float_as_int(f); }

// 16-byte global load through a buffer resource (buffer_load_dwordx4, base in SGPRs, 32-bit
// byte offset per lane).  Used for the part of the scene that is NOT staged in LDS: an
// ordinary pointer load next to an LDS load gets if-converted by hipcc into one flat_load
// with a selected address, which is far slower than ds_read / buffer_load.
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, int byte_off) {
  const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, 0, 0);
  return make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
}
// caller ray i of `rays`: rays[6 i .. 6 i + 6) = {o.xyz, d.xyz}, with its derived fields
__device__ __forceinline__ Ray load_ray(const float *rays, int i) {
  const float *const q = rays + (size_t)i * 6;
  Ray r;
  r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
  r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
  ray_derive(r);
  return r;
}
#endif

// ---- the pooled kernel's instantiations ----------------------------------------------------------
// pooled_kernel's RAYS mode: 0 the render path's pixels, kRaysColour rt_trace_rays, kRaysAny rt_occluded_rays
constexpr int kRaysColour = 1, kRaysAny = 2;
// The template arguments of one pooled_kernel instantiation: pooled_kernel<threads, all_lds, stats, solo, tail, ord, cull, spill, rays>
struct PooledKey {
  int threads;
  bool all_lds, stats, solo;
  int tail;      // 1: COLD, 2: DONATE
  bool ord, cull;
  int spill;     // the LDS box stack's capacity minus 64 (kSpillCapb, kSpillCapbTest), or 0
  int rays;
  constexpr bool operator==(const PooledKey &o) const {
    return threads == o.threads && all_lds == o.all_lds && stats == o.stats && solo == o.solo && tail == o.tail && ord == o.ord && cull == o.cull &&
           spill == o.spill && rays == o.rays;
  }
};
// Every compiled instantiation (render_kernels.hip launches these and no others).  Abbreviations: T / F for true / false.
namespace pooled_keys {
constexpr bool T = true, F = false;
constexpr int SP = kSpillCapb - 64, ST = kSpillCapbTest - 64, RC = kRaysColour, RA = kRaysAny;
constexpr PooledKey kPooledKeys[] = {
    // workgroups of 16 waves: each flavour on the scene wholly in LDS, in general, and with CULL (the general scene path only)
    {1024, T, F, F, 0, F, F, 0, 0}, {1024, F, F, F, 0, F, F, 0, 0}, {1024, F, F, F, 0, F, T, 0, 0},   // plain
    {1024, T, F, T, 0, F, F, 0, 0}, {1024, F, F, T, 0, F, F, 0, 0}, {1024, F, F, T, 0, F, T, 0, 0},   // SOLO
    {1024, T, F, F, 1, F, F, 0, 0}, {1024, F, F, F, 1, F, F, 0, 0}, {1024, F, F, F, 1, F, T, 0, 0},   // COLD
    {1024, T, F, T, 1, F, F, 0, 0}, {1024, F, F, T, 1, F, F, 0, 0}, {1024, F, F, T, 1, F, T, 0, 0},   // COLD+SOLO
    {1024, T, F, F, 2, F, F, 0, 0}, {1024, F, F, F, 2, F, F, 0, 0}, {1024, F, F, F, 2, F, T, 0, 0},   // DONATE
    {1024, T, F, T, 2, F, F, 0, 0}, {1024, F, F, T, 2, F, F, 0, 0}, {1024, F, F, T, 2, F, T, 0, 0},   // DONATE+SOLO
    {1024, T, F, F, 0, T, F, 0, 0}, {1024, F, F, F, 0, T, F, 0, 0}, {1024, F, F, F, 0, T, T, 0, 0},   // ORD
    {1024, T, F, T, 0, T, F, 0, 0}, {1024, F, F, T, 0, T, F, 0, 0}, {1024, F, F, T, 0, T, T, 0, 0},   // ORD+SOLO
    {1024, T, F, F, 2, T, F, 0, 0}, {1024, F, F, F, 2, T, F, 0, 0}, {1024, F, F, F, 2, T, T, 0, 0},   // ORD+DONATE
    {1024, T, F, T, 2, T, F, 0, 0}, {1024, F, F, T, 2, T, F, 0, 0}, {1024, F, F, T, 2, T, T, 0, 0},   // ORD+SOLO+DONATE
    // ... instrumented (rt_render_trace)
    {1024, F, T, F, 0, F, F, 0, 0}, {1024, F, T, F, 0, F, T, 0, 0}, {1024, F, T, F, 0, T, F, 0, 0}, {1024, F, T, F, 0, T, T, 0, 0},
    {1024, F, T, T, 0, T, F, 0, 0}, {1024, F, T, T, 0, T, T, 0, 0}, {512, F, T, F, 0, F, F, 0, 0},
    // workgroups of 4, 8 and 12 waves
    {256, T, F, F, 0, F, F, 0, 0}, {256, F, F, F, 0, F, F, 0, 0}, {256, T, F, T, 0, F, F, 0, 0}, {256, F, F, T, 0, F, F, 0, 0},
    {512, T, F, F, 0, F, F, 0, 0}, {512, F, F, F, 0, F, F, 0, 0}, {512, T, F, T, 0, F, F, 0, 0}, {512, F, F, T, 0, F, F, 0, 0},
    {768, T, F, F, 0, F, F, 0, 0}, {768, F, F, F, 0, F, F, 0, 0}, {768, T, F, T, 0, F, F, 0, 0}, {768, F, F, T, 0, F, F, 0, 0},
    // four waves: CULL, and the SPILL kernels for trees taller than 15 levels (production and stack_cap capacity)
    {256, F, F, F, 0, F, T, 0, 0}, {256, F, F, F, 0, F, F, SP, 0}, {256, F, F, F, 0, F, T, SP, 0}, {256, F, F, F, 0, F, F, ST, 0}, {256, F, F, F, 0, F, T, ST, 0},
    // caller rays: 16 waves (scene in LDS or not), 4 waves, SPILL
    {1024, T, F, F, 0, F, F, 0, RC}, {1024, F, F, F, 0, F, F, 0, RC}, {256, F, F, F, 0, F, F, 0, RC}, {256, F, F, F, 0, F, F, SP, RC}, {256, F, F, F, 0, F, F, ST, RC},
    {1024, T, F, F, 0, F, F, 0, RA}, {1024, F, F, F, 0, F, F, 0, RA}, {256, F, F, F, 0, F, F, 0, RA}, {256, F, F, F, 0, F, F, SP, RA}, {256, F, F, F, 0, F, F, ST, RA},
};
}  // namespace pooled_keys
using pooled_keys::kPooledKeys;
constexpr int kNumPooledKeys = sizeof(kPooledKeys) / sizeof(kPooledKeys[0]);
// What warm_render_kernels resolves at context creation: the instantiations a single-GPU render may switch to between a view's frames --
// workgroups of 16 waves, and the four-wave plain / CULL / SPILL kernels of the twenty-wave shape
constexpr bool pooled_warmed(const PooledKey &k) {
  return !k.stats && k.rays == 0 && (k.threads == 1024 || (k.threads == 256 && !k.all_lds && !k.solo && k.spill != kSpillCapbTest - 64));
}

// The instantiation that exists a second time with ENTRY -- new primary rays start at their tile's entry list (KParams::entry) -- and so the
// launches that may carry a table: plain tile tickets, no solo loop, no tail, 16 waves with the scene wholly in LDS (rgbbox's batches).  Not the four-wave
// kernels that read the scene from L2: with lists irreg's batch ran 4 - 5 % SLOWER (0.100 -> 0.105 ms per frame; -0.5 % VALU instructions, +6 % scalar ones:
// profiles/entry_lists), as with the leaf filter.  launch_pooled takes the ENTRY twin of choose_pooled's key whenever p.entry is set, and refuses a table on
// any other key
constexpr bool pooled_entry_ok(const PooledKey &k) {
  return k.threads == 1024 && k.all_lds && !k.stats && !k.solo && k.tail == 0 && !k.ord && !k.cull && k.spill == 0 && k.rays == 0;
}

// WIDE: the four-wave plain and CULL render kernels (no SPILL, and both SPILL capacities) exist a second time with the constants of the twenty-wave shape
// compiled in -- no scene prefix in LDS, two ray planes (render_kernels.hip).  The flag travels in the SPILL template argument, above any capacity.
// pooled_wide_ok: the keys that have the twin.  pooled_wide_plan: the launch shapes that may take it -- workgroups of four waves, five of them per CU, nothing of
// the scene staged, two ray planes; a four-wave workgroup that does stage a prefix keeps the generic kernel, which is the one way the twin could read wrong data.
// launch_pooled takes the twin of choose_pooled's key when its caller says `wide`, and refuses where either predicate fails.  The key, and so the launch's name
// in rt_context_last_launch, is the generic kernel's.
constexpr int kSpillWide = 1 << 20;
constexpr bool pooled_wide_ok(const PooledKey &k) {
  return k.threads == 256 && !k.all_lds && !k.stats && !k.solo && k.tail == 0 && !k.ord && k.rays == 0 && (k.spill == 0 || k.spill == kSpillCapb - 64 || k.spill == kSpillCapbTest - 64);
}
constexpr bool pooled_wide_plan(int waves_per_wg, int wgs_per_cu, int lds_nodes, int lds_sph, int ray_planes) {
  return waves_per_wg == 4 && wgs_per_cu == 5 && lds_nodes == 0 && lds_sph == 0 && ray_planes == 2;
}

// Which instantiation renders a launch with these parameters (false: none -- hipErrorInvalidValue).  `rays`: 0, kRaysColour, kRaysAny.
// No HIP runtime calls: the CPU check tools/pooled_choice_check.cpp runs it over its inputs.
inline bool choose_pooled(const KParams &p, bool stats, int waves_per_wg, int rays, PooledKey *out) {
  const bool all_lds = p.lds_nodes == p.n_nodes && p.lds_sph == p.n_sph;
  PooledKey k{64 * waves_per_wg, false, stats, false, 0, false, p.cull != 0, 0, rays};
  if (rays && (stats || p.cull || p.px_hdr != nullptr || p.order != nullptr || p.nframes != 1)) return false;
  if (p.cull && waves_per_wg != 16 && waves_per_wg != 4) return false;
  if (p.spill != nullptr) {
    // (workgroups of four waves, for a tree taller than 15 levels: the kernels whose box stack may overflow into device memory)
    if (waves_per_wg != 4 || stats || p.px_hdr != nullptr || (p.capb != kSpillCapb && p.capb != kSpillCapbTest)) return false;
    k.spill = p.capb - 64;
  } else if (p.cull && waves_per_wg == 4) {
    // (workgroups of four waves, CULL: the plain kernel -- batches and large frames in the shape of five workgroups per CU, api.cpp: make_plan)
    if (stats || p.px_hdr != nullptr) return false;
  } else if (rays) {
    if (waves_per_wg != 16 && waves_per_wg != 4) return false;
    k.all_lds = waves_per_wg == 16 && all_lds;
  } else if (stats) {
    // (the instrumented launch: no ALL_LDS; ORD for a view that renders through its pixel list; other shapes than 16 waves take 8)
    if (waves_per_wg != 16) k.threads = 512;
    else if (p.px_hdr != nullptr) { k.ord = true; k.solo = p.solo != 0; }
  } else if (p.px_hdr != nullptr) {
    // (ORD: pixel tickets, workgroups of 16 waves only; p.solo clear: a list without a one-pixel class; p.donate: with the DONATE tail --
    // a list borrowed from another view)
    if (waves_per_wg != 16 || p.nframes != 1) return false;
    k.ord = true; k.solo = p.solo != 0; k.tail = p.donate ? 2 : 0;
    k.all_lds = all_lds && !k.cull;
  } else {
    // (SOLO: the instantiation with the solo prologue, for launches whose first tickets are single pixels.  COLD: small ordered single frames;
    // DONATE: the first frame of a view; workgroups of 16 waves only -- other shapes render them with the ordinary kernels)
    k.solo = p.solo && p.nframes == 1 && p.order != nullptr && p.deep_class > 0 && p.deep_split == 6 && p.tl_log2 == kTreeletDepth;
    if (waves_per_wg == 16) k.tail = p.cold ? 1 : p.donate ? 2 : 0;
    else if (waves_per_wg != 4 && waves_per_wg != 8 && waves_per_wg != 12) return false;
    k.all_lds = all_lds && !k.cull;
  }
  *out = k;
  return true;
}

// PRESORT: the instantiations that stage the node records sign-ordered (lane_core.h: presort_pack) and read near / far bounds at addresses the
// ray's signs pick -- the plain render kernels on a scene wholly in LDS.  The kernels that call solo_trace (SOLO, COLD, DONATE, ORD: its treelet
// reads want the four planes of quarters), the caller-ray loops and everything that reads nodes from L2 keep the 64-byte records.
constexpr bool pooled_presort(bool all_lds, bool solo, int tail, bool ord, int rays) { return all_lds && !solo && tail == 0 && !ord && rays == 0; }
constexpr bool pooled_presort(const PooledKey &k) { return pooled_presort(k.all_lds, k.solo, k.tail, k.ord, k.rays); }

// The instantiations whose BOX / BOX2 can filter leaf children by their own box (KParams::leaf_box): the render kernels of a scene that lives in LDS whole
// (ALL_LDS), and the instrumented ones without CULL (rt_render_trace counts what the filter leaves of such a scene's frame).  Left out, and so the parent's
// instructions:
//  * every kernel that reads the scene from L2, CULL or not: those launches already skip most of the sphere tests the filter would (irreg's batch: -3.5 % VALU
//    instructions for -32 % sphere tests, its launch 0.1069 -> 0.1065 ms, inside the noise) and pay for the flag's scalar load in every BOX operation -- its
//    ordered single frames, bound by their chains, were 0.5 - 1 % slower with it.  The host admits LDS-resident scenes only (api.cpp: set_leaf_box);
//  * four waves, scene in LDS, SOLO: three more VGPRs put it at 96 with a larger private segment;
//  * the caller-ray loops (no guard covers a caller's origins).
constexpr bool pooled_leaf_box(int threads, bool all_lds, bool stats, bool solo, bool cull, int rays) {
  return rays == 0 && !cull && (stats || (all_lds && !(threads == 256 && solo)));
}
constexpr bool pooled_leaf_box(const PooledKey &k) { return pooled_leaf_box(k.threads, k.all_lds, k.stats, k.solo, k.cull, k.rays); }

// The instantiation's name in rt_context_last_launch: plain, SOLO, COLD, COLD+SOLO, DONATE, DONATE+SOLO, ORD, ORD+SOLO, ORD+DONATE, ORD+SOLO+DONATE,
// any (the occlusion loop); then +CULL, +SPILL
inline std::string pooled_name(const PooledKey &k) {
  std::string s = k.rays == kRaysAny ? "any" : k.ord ? "ORD" : k.tail == 1 ? "COLD" : k.tail == 2 ? "DONATE" : "";
  if (k.solo) s += s.empty() ? "SOLO" : "+SOLO";
  if (k.ord && k.tail == 2) s += "+DONATE";
  if (s.empty()) s = "plain";
  if (k.cull) s += "+CULL";
  if (k.spill) s += "+SPILL";
  return s;
}

hipError_t launch_pixel(const KParams &p, bool stats, hipStream_t stream);
// caller rays (render_kernels.hip): ray_colour of p.nrays rays, one lane per ray (the pixel family); the other queries' launchers: query_device.hpp
hipError_t launch_pixel_rays(const KParams &p, hipStream_t stream);
// block = 64 * waves_per_wg threads (4, 8 or 16 waves); grid = persistent workgroups
hipError_t launch_persistent(const KParams &p, bool stats, int grid, int waves_per_wg, hipStream_t stream);
size_t persistent_lds_bytes(int lds_nodes, int lds_sph, int smax, int lmax, int waves_per_wg);
// the pooled family: the instantiation choose_pooled picks (grid workgroups of 64 * waves_per_wg threads).  `rays`: 64 consecutive caller rays
// per ticket (the plain loop; kRaysAny: occlusion of p.nrays rays over (p.ray_tlo, p.ray_thi), or each over its own with p.ray_tlo_dev, into p.occluded)
// `entry`: 0 = every ray starts at the root (p.entry is not looked at: it shares its slot with colour3); kEntryLists = p.entry is the launch's table of entry lists
// (launch_tile_entry has filled it) and the ENTRY twin of the chosen instantiation renders -- an error where there is none (pooled_entry_ok) or with caller rays;
// kEntryCount = the same through the counting twin, p.trace holding two zeroed words per wave
constexpr int kEntryLists = 1, kEntryCount = 2;
// ... and what else the ENTRY template value says, in bits above that mode (the caller of launch_pooled ORs them in; pooled_entry_bits is the policy):
// kEntryColLds: the colour table is staged in LDS behind the sphere prefix and SHADE reads the winner's colour there -- in the layout of pooled_col_lds_bytes;
// kEntryRtFlags: KParams::leaf_box and KParams::dark are read at run time, as in every other instantiation -- without it both are ON by construction and
// BOX / BOX2 / SHADE carry neither the scalar load nor the mask term (a launch with either flag clear must not take such a kernel)
constexpr int kEntryModeMask = 3, kEntryColLds = 4, kEntryRtFlags = 8;
// kEntryExit (only with kEntryColLds and without kEntryRtFlags): scattered rays start at their origin sphere's exit list (KParams::exit_tab).
// kExitDmax (lane_core.h): the deepest (even) depth of a node a list resumes at -- a compile-time constant of the kernel and of the tables; a list holds that
// node's item and one pair item per two levels above it.  The counting twin then writes two more words per wave behind the 2 * waves words of the entry counts.
constexpr int kEntryExit = 16;
constexpr int kExitItems = 1 + kExitDmax / 2;          // items of a full list
// The exit tables of a scene fit the item format (record offsets / 8 in 16 bits) and the LDS next to 16 waves
constexpr bool pooled_exit_fits(int n_nodes, int n_sph, int capb, int capl, int ray_planes, size_t lds_limit) {
  return n_nodes >= 1 && (size_t)(n_nodes + kExitPairs) * (kPsNodeBytes / 8) < 65536u &&
         (((size_t)(n_nodes + kExitPairs) * kPsNodeBytes + 15) & ~(size_t)15) + (size_t)n_sph * 32 + (size_t)16 * pooled_wave_dw(ray_planes, capb, capl) * sizeof(unsigned) <= lds_limit;
}
// (bytes of KParams::exit_tab)
constexpr size_t exit_tab_bytes(int n_sph) { return (size_t)kExitPairs * 64 + (size_t)n_sph * 32; }
// The two launch flags the ENTRY kernels without kEntryRtFlags were compiled for
constexpr bool pooled_entry_flags_const(int leaf_box, int dark) { return leaf_box != 0 && dark != 0; }
// The LDS of a 16-wave workgroup of a kEntryColLds kernel on a scene of n_nodes inner nodes and n_sph spheres, all of it staged: the sign-ordered records PACKED
// (kPsNodeBytes each, rounded up to 16 bytes in all: the other kernels keep the 64-byte pitch of the planes and leave 8 bytes per node unused), the spheres, the
// colours, the waves' regions.  rgbbox: 22 352 + 6 400 + 6 400 + 16 x 7 952 = 162 384 of 163 840 bytes.
constexpr size_t pooled_col_lds_bytes(int n_nodes, int n_sph, int capb, int capl, int ray_planes) {
  return (((size_t)n_nodes * kPsNodeBytes + 15) & ~(size_t)15) + (size_t)n_sph * 32 + (size_t)16 * pooled_wave_dw(ray_planes, capb, capl) * sizeof(unsigned);
}
// Does that fit a CU (never at the price of a wave: a scene whose table does not fit keeps the load from memory)?
constexpr bool pooled_col_fits(size_t col_lds_bytes, size_t lds_limit) { return col_lds_bytes <= lds_limit; }
// The ENTRY template value of a launch whose mode is `mode` (kEntryLists / kEntryCount): flags constant where both are set, colours in LDS where they fit and
// the flags are constant (the run-time twin is the kernel as it was: it keeps the global load).  `col_lds`: the context's option (0: never)
constexpr int pooled_entry_bits(int mode, int leaf_box, int dark, size_t col_lds_bytes, size_t lds_limit, bool col_lds = true) {
  return !pooled_entry_flags_const(leaf_box, dark) ? mode | kEntryRtFlags : mode | (col_lds && pooled_col_fits(col_lds_bytes, lds_limit) ? kEntryColLds : 0);
}
// `wide`: the WIDE twin of the chosen instantiation renders (above: pooled_wide_ok, pooled_wide_plan) -- an error where there is none, or with `entry`
hipError_t launch_pooled(const KParams &p, bool stats, int grid, int waves_per_wg, hipStream_t stream, int rays = 0, int entry = 0, bool wide = false);
// fills p.entry for the launch launch_pooled(p, stats, grid, waves_per_wg, stream) is about to make (hipErrorInvalidValue: that launch has no ENTRY instantiation)
hipError_t launch_tile_entry(const KParams &p, bool stats, int waves_per_wg, hipStream_t stream);
// fills `tab` (exit_tab_bytes(p.n_sph) bytes) from p's scene: the pair records and the per-sphere exit lists of the kEntryExit kernels
hipError_t launch_exit_tables(const KParams &p, float4 *tab, hipStream_t stream);
size_t pooled_lds_bytes(int lds_nodes, int lds_sph, int capb, int capl, int ray_planes, int waves_per_wg);
// prepare_scene on the GPU (bvh_build.hip).  Canonical {L, I} arrays + the traversal copy.
struct GpuBvhOut {
  float *L7;                 // [n][7]
  float *bmin, *bmax;        // [n-1][3]
  int *left, *right, *parent;   // [n-1]  ptr: inner i -> i, leaf i -> -2 - i
  float4 *nodes32;           // [2*(n-1)]
  float4 *nodes64;           // [4*(n-1)]
  float4 *sph, *col;         // [n]
  int *ids;                  // [n]  the input's index of L[i] (rt_prepared_get_sphere_ids)
};
void warm_render_kernels();
hipError_t warm_scratch(hipStream_t stream, int *sink_dev);   // the queue's scratch allocated now, not inside the first frame
void warm_build_kernels();
size_t gpu_build_scratch_bytes(int n);   // device scratch one build of n spheres needs
hipError_t gpu_copy_from_pinned(void *dst_dev, const void *src_pinned, size_t bytes, hipStream_t stream);
size_t gpu_build_pinned_bytes();         // host-pinned block the build kernels report through
// `sph7_dev`: the n spheres in device memory; `scratch`, `pinned`: blocks of the sizes above.
// Synchronises the stream; returns the tree height and the root's box.
hipError_t gpu_build_bvh(const float *sph7_dev, int n, const GpuBvhOut &out, char *scratch, char *pinned, hipStream_t stream,
                         int *height_out, float root_lo[3], float root_hi[3]);
// The spheres' statistics behind the culling guards (rt_host.hpp: CullStats, the host's cull_stats), reduced on the device from spheres
// in device memory: min / max of the positions, r_min, r_max in fp32 (exact), c_max = max |p_a| + r in fp64 (the host's arithmetic), and
// `bad`: a non-finite component or a radius failing r >= 2^-20.  Two launches (per-block partials, one block over them) on `stream`;
// the second writes the record into `out` -- the slot of the build's pinned block at kCullStatsPinnedOffset, read by the host after
// gpu_build_bvh's synchronisation.  `partial`: cull_stats_scratch_bytes() of device memory.
struct CullStatsDev {
  double c_max;
  float lo[3], hi[3];
  float r_min, r_max;
  int bad;
  int pad;
};
static_assert(sizeof(CullStatsDev) == 48, "CullStatsDev: 48 bytes");
constexpr size_t kCullStatsPinnedOffset = 256;   // bytes into the pinned block (gpu_build_pinned_bytes)
constexpr int kCullStatsBlocks = 1024;           // partials: at most this many
constexpr size_t cull_stats_scratch_bytes() { return sizeof(CullStatsDev) * kCullStatsBlocks; }
hipError_t launch_cull_stats(const float *sph7_dev, int n, CullStatsDev *partial, CullStatsDev *out, hipStream_t stream);

// The leaf-child slots of nodes64 from sph (the device's copy of rt::fill_leaf_boxes: the same leaf_box_bounds, the same bits), behind a build
// on the device -- whose records come out with zeroed slots -- once the host has the scene's constants
hipError_t launch_leaf_boxes(float4 *nodes64, const float4 *sph, int n_nodes, float q, float lin, float abs, hipStream_t stream);

constexpr int kOrderBlocksMax = 64;                                  // workgroups per shard of the tile-order sort
constexpr int kOrderScratchInts = kMaxShards * 64 * kOrderBlocksMax;   // its scratch: [shard][bin][workgroup] counts
hipError_t launch_tile_order(int *cost, int *order, int ntiles, int tiles_x, int nshards, int *scratch, hipStream_t stream);
// The view's pixel list from the per-pixel record of its first frame (px_count / px_scan / px_place kernels): pixels by
// descending chain length, header per px_make_header with the classes cut at chains of >= thr[k] rays (thr[0] >= thr[1] >= ...;
// the one-pixel class also capped at `solo_cap` pixels).  `scratch`: px_scratch_ints(ntiles) ints.
struct PxGeom {
  int w, rows_local, rpt_log2, out_skip, tiles_x, tiles_y;
};
// How the classes are cut.  thr[0] > 0: by hand -- class k (1, 8, 16, 32 pixels per ticket) holds the chains of >= thr[k] rays that no
// earlier class holds.  thr[0] == 0: from a model of the launch, evaluated on the device from the list's histogram: a wave that carries
// n rays of equal chain length advances them one bounce per g[k] (units of 0.1 us; k = 0 the solo loop, then 8, 16, 32, 64 rays; they
// differ by where the scene lives: LDS or L2), so a class may hold chains of up to T / g[k] rays if the frame is to end by T, and T is
// the larger of what the longest chain takes in the solo loop and what the waves' time adds up to -- rays of class k cost g[k] / width
// of a wave's time each, those of the 64-pixel class ray_ns -- iterated to a fixed point.
struct PxPolicy {
  int thr[kPxClasses - 1];
  int g[kPxClasses];
  int ray_ns;        // a wave's time per ray in the 64-pixel class (rays of mixed phases share the wave: cheaper than g[4] / 64, the lockstep figure)
  int nwaves;
  int solo_cap;      // the one-pixel class: at most this many pixels (0: no solo loop on this launch)
  int zip;           // the bulk's tickets alternately from both ends of its segment (px_ticket_span)
};
constexpr int kPxBlocksMax = 2048;
constexpr size_t px_scratch_ints() { return (size_t)64 * kPxBlocksMax + 256; }
hipError_t launch_px_order(const unsigned char *cost_px, const PxGeom &g, const PxPolicy &pol, unsigned *list, int *hdr, int *scratch, hipStream_t stream);
hipError_t launch_place_part(const int32_t *part, int32_t *image, int w, int rows_local, int rows_per_tile, int part_id,
                             int nparts, hipStream_t stream);

// (a batch: nframes frames, frame f's parts frame_stride_in elements behind frame f - 1's, its image frame_stride_out behind)
hipError_t launch_place_all(const int32_t *stacked, int32_t *image, int w, int h, int rows_per_tile, int nparts,
                            size_t part_stride, hipStream_t stream, int nframes = 1, size_t frame_stride_in = 0,
                            size_t frame_stride_out = 0);

}  // namespace rtk
