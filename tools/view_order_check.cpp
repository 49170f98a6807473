// view_order_check.cpp -- runs the view-order sorts on cases read from a file and writes what they left in device memory,
// for tests/test_view_order_gpu.py to compare with tests/view_order_ref.py.  Not a product path; no timing.
//   view_order_check <cases> <results>
// Cases file (little-endian int32): 'VORD', number of cases, then per case its kind and arguments:
//   1 tile order:   ntiles, tiles_x, nshards, cost[ntiles]
//   2 pixel list:   PxGeom (6 ints), PxPolicy (13 ints), record bytes n, the record (n bytes, padded to a multiple of 4)
//   3 first order:  tiles_x, tiles_y
//   4 view:         scene (0 rgbbox, 1 irreg, 2 spheres: n, 7 n floats, look_from, look_at, fov), h, w, max_depth, entry (0 rt_render /
//                   rt_render_part, 1 rt_render_part, 2 rt_render_part_inplace), rows_per_tile, part, nparts, frames, number of options,
//                   per option 16 ints of name (zero padded) and the value
// Results file: a sequence of blocks, each an int64 byte count and the bytes.  Synthetic cases (1-3) call rtk::launch_tile_order /
// launch_px_order / launch_first_order of the library on buffers of their own: every device buffer has 256 guard bytes on either side,
// all of it filled with 0xA5 before the inputs are uploaded, and is written out guards included -- cost, order, scratch | record, list,
// header, scratch | order, rank.  A view case (white box: rt_internal.hpp only to find the view's arrays) renders through the public C ABI
// and writes after every synchronised frame: 16 ints {ntiles, nshards, px_elems, rec_out_skip, cost_px_bytes, num_cu, valid, px_valid,
// tiles_x, tiles_y, rows_local, px_solo, ...0}, rt_context_last_launch, cost, order + tables, cost_px, list + header.
// Every launch sequence is followed by hipStreamSynchronize and hipGetLastError: on any HIP error the program exits at once with that
// status and runs no further case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_internal.hpp"

namespace {

constexpr size_t kGuard = 256;
constexpr int kFill = 0xA5;
FILE *g_out = nullptr;

[[noreturn]] void die(int status, const char *what, const char *detail) {
  std::fprintf(stderr, "view_order_check: %s: %s\n", what, detail);
  std::fflush(nullptr);
  std::exit(status ? status : 1);
}
void hip_ok(hipError_t e, const char *what) {
  if (e != hipSuccess) die(static_cast<int>(e), what, hipGetErrorString(e));
}
void block(const void *p, size_t bytes) {
  const int64_t n = static_cast<int64_t>(bytes);
  if (std::fwrite(&n, sizeof n, 1, g_out) != 1 || (bytes && std::fwrite(p, 1, bytes, g_out) != bytes)) die(1, "results", "short write");
}

// a device buffer of `bytes` between two guards, everything 0xA5
struct Guarded {
  char *base = nullptr;
  size_t bytes = 0;
  explicit Guarded(size_t n) : bytes(n) {
    hip_ok(hipMalloc(reinterpret_cast<void **>(&base), n + 2 * kGuard), "hipMalloc");
    hip_ok(hipMemset(base, kFill, n + 2 * kGuard), "hipMemset");
  }
  Guarded(const Guarded &) = delete;
  ~Guarded() { (void)hipFree(base); }
  template <class T> T *as() const { return reinterpret_cast<T *>(base + kGuard); }
  void upload(const void *src, size_t n) const { hip_ok(hipMemcpy(base + kGuard, src, n, hipMemcpyHostToDevice), "upload"); }
  void dump() const {      // guards included
    std::vector<char> h(bytes + 2 * kGuard);
    hip_ok(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost), "download");
    block(h.data(), h.size());
  }
};
void dump_dev(const void *dev, size_t bytes) {
  std::vector<char> h(bytes);
  if (bytes) hip_ok(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost), "download");
  block(h.data(), bytes);
}

struct Reader {
  std::vector<int32_t> v;
  size_t at = 0;
  int32_t i() {
    if (at >= v.size()) die(1, "cases", "truncated file");
    return v[at++];
  }
  const int32_t *take(size_t n) {
    if (at + n > v.size()) die(1, "cases", "truncated file");
    const int32_t *p = v.data() + at;
    at += n;
    return p;
  }
};

void finish(hipError_t launched, hipStream_t st, const char *what) {
  hip_ok(launched, what);
  hip_ok(hipStreamSynchronize(st), what);
  hip_ok(hipGetLastError(), what);
}

void tile_order_case(Reader &in, hipStream_t st) {
  const int ntiles = in.i(), tiles_x = in.i(), nshards = in.i();
  if (ntiles < 1 || tiles_x < 1 || ntiles % tiles_x || (nshards != 1 && nshards != 8)) die(1, "cases", "bad tile-order case");
  const int32_t *cost = in.take(static_cast<size_t>(ntiles));
  Guarded d_cost(sizeof(int) * static_cast<size_t>(ntiles)), d_order(sizeof(int) * static_cast<size_t>(rtk::order_table_ints(ntiles))),
      d_scratch(sizeof(int) * static_cast<size_t>(rtk::kOrderScratchInts));
  d_cost.upload(cost, d_cost.bytes);
  finish(rtk::launch_tile_order(d_cost.as<int>(), d_order.as<int>(), ntiles, tiles_x, nshards, d_scratch.as<int>(), st), st, "tile order");
  d_cost.dump();
  d_order.dump();
  d_scratch.dump();
}

void px_order_case(Reader &in, hipStream_t st) {
  rtk::PxGeom g{};
  g.w = in.i(); g.rows_local = in.i(); g.rpt_log2 = in.i(); g.out_skip = in.i(); g.tiles_x = in.i(); g.tiles_y = in.i();
  rtk::PxPolicy pol{};
  for (int k = 0; k < 4; ++k) pol.thr[k] = in.i();
  for (int k = 0; k < 5; ++k) pol.g[k] = in.i();
  pol.ray_ns = in.i(); pol.nwaves = in.i(); pol.solo_cap = in.i(); pol.zip = in.i();
  const int nrec = in.i();
  // the bounds the kernels rely on, checked before anything is launched: the grid covers the part, the record covers every pixel read
  if (g.w < 1 || g.rows_local < 1 || g.w >= 65536 || g.rows_local >= 65536 || g.rpt_log2 < 0 || g.rpt_log2 > 16 || g.out_skip < 0 ||
      g.tiles_x != (g.w + 7) / 8 || g.tiles_y != (g.rows_local + 7) / 8)
    die(1, "cases", "bad pixel-list geometry");
  const size_t last = static_cast<size_t>(g.rows_local - 1) * g.w + (g.w - 1) + static_cast<size_t>((g.rows_local - 1) >> g.rpt_log2) * g.out_skip;
  if (nrec < 1 || static_cast<size_t>(nrec) != last + 1) die(1, "cases", "the record does not end at the part's last pixel");
  for (int k = 0; k < 5; ++k)
    if (pol.g[k] < 1) die(1, "cases", "bad policy");
  const int32_t *rec = in.take((static_cast<size_t>(nrec) + 3) / 4);
  const size_t npix = static_cast<size_t>(g.w) * g.rows_local;
  Guarded d_rec(static_cast<size_t>(nrec)), d_list(sizeof(unsigned) * npix), d_hdr(sizeof(int) * rtk::kPxHdrInts),
      d_scratch(sizeof(int) * rtk::px_scratch_ints());
  d_rec.upload(rec, d_rec.bytes);
  finish(rtk::launch_px_order(d_rec.as<unsigned char>(), g, pol, d_list.as<unsigned>(), d_hdr.as<int>(), d_scratch.as<int>(), st), st, "pixel list");
  d_rec.dump();
  d_list.dump();
  d_hdr.dump();
  d_scratch.dump();
}

void first_order_case(Reader &in, hipStream_t st) {
  const int tiles_x = in.i(), tiles_y = in.i();
  if (tiles_x < 1 || tiles_y < 1 || tiles_y > 4096 || tiles_x > 32768) die(1, "cases", "bad first-order case");   // (the sizes api.cpp admits)
  const int ntiles = tiles_x * tiles_y, nb = (tiles_x + 7) / 8;
  Guarded d_order(sizeof(int) * static_cast<size_t>(rtk::order_table_ints(ntiles))), d_rank(sizeof(int) * static_cast<size_t>(tiles_y + nb));
  finish(rtk::launch_first_order(d_order.as<int>(), d_rank.as<int>(), tiles_x, tiles_y, st), st, "first order");
  d_order.dump();
  d_rank.dump();
}

void rt_ok(rt_context *ctx, int rc, const char *what) {
  if (rc) die(rc, what, ctx ? rt_last_error(ctx) : "no context");
}

void view_case(Reader &in) {
  rt_context *ctx = nullptr;
  rt_ok(nullptr, rt_context_create(&ctx, -1, nullptr, 0), "rt_context_create");
  rt_ok(ctx, rt_context_set_variant(ctx, RT_VARIANT_POOLED), "rt_context_set_variant");
  rt_scene *sc = nullptr;
  const int scene = in.i();
  if (scene == 0) rt_ok(ctx, rt_scene_rgbbox(ctx, &sc), "scene");
  else if (scene == 1) rt_ok(ctx, rt_scene_irreg(ctx, &sc), "scene");
  else {
    const int n = in.i();
    if (n < 2) die(1, "cases", "bad scene");
    const float *sph = reinterpret_cast<const float *>(in.take(static_cast<size_t>(n) * 7));
    const float *look = reinterpret_cast<const float *>(in.take(7));
    rt_ok(ctx, rt_scene_from_spheres(ctx, &sc, sph, n, look, look + 3, look[6]), "scene");
  }
  const int h = in.i(), w = in.i(), max_depth = in.i(), entry = in.i(), rpt = in.i(), part = in.i(), nparts = in.i(), frames = in.i(), nopts = in.i();
  for (int o = 0; o < nopts; ++o) {
    char name[68] = {0};
    std::memcpy(name, in.take(16), 64);
    rt_ok(ctx, rt_context_set_option(ctx, name, in.i()), name);
  }
  rt_prepared *ps = nullptr;
  rt_ok(ctx, rt_prepare_scene(ctx, &ps, h, w, sc), "rt_prepare_scene");
  const int64_t rows = entry == 0 ? h : rt_part_rows(h, rpt, part, nparts);
  void *out = nullptr;
  rt_ok(ctx, rt_device_alloc(ctx, &out, static_cast<int64_t>(entry == 2 ? h : rows) * w * 4), "rt_device_alloc");
  rt_ok(ctx, rt_context_sync(ctx), "rt_context_sync");
  for (int f = 0; f < frames; ++f) {
    int rc;
    if (entry == 0) rc = max_depth == 50 ? rt_render(ctx, ps, h, w, static_cast<int32_t *>(out)) : rt_render_part(ctx, ps, h, w, max_depth, 8, 0, 1, static_cast<int32_t *>(out));
    else if (entry == 1) rc = rt_render_part(ctx, ps, h, w, max_depth, rpt, part, nparts, static_cast<int32_t *>(out));
    else rc = rt_render_part_inplace(ctx, ps, h, w, max_depth, rpt, part, nparts, 1, nullptr, 0, static_cast<int32_t *>(out));
    rt_ok(ctx, rc, "render");
    rt_ok(ctx, rt_context_sync(ctx), "rt_context_sync");
    hip_ok(hipDeviceSynchronize(), "the sort streams");     // (eager_sort: the sorts run on streams of their own, which rt_context_sync does not wait for)
    hip_ok(hipGetLastError(), "render");
    if (ps->orders.size() != 1) die(1, "view", "the prepared scene does not hold exactly one view");
    const TileOrder &v = ps->orders.back();
    const int32_t meta[16] = {v.ntiles, v.nshards, static_cast<int32_t>(v.px_elems), v.rec_out_skip, static_cast<int32_t>(v.cost_px_bytes), ctx->num_cu,
                              v.valid ? 1 : 0, v.px_valid ? 1 : 0, (w + 7) / 8, static_cast<int32_t>((rows + 7) / 8), static_cast<int32_t>(rows), v.px_solo ? 1 : 0, 0, 0, 0, 0};
    block(meta, sizeof meta);
    const std::string ll = rt_context_last_launch(ctx);
    block(ll.data(), ll.size());
    dump_dev(v.cost, sizeof(int) * static_cast<size_t>(v.ntiles));
    dump_dev(v.order, sizeof(int) * static_cast<size_t>(rtk::order_table_ints(v.ntiles)));
    dump_dev(v.cost_px, v.cost_px ? v.cost_px_bytes : 0);
    dump_dev(v.px_list, v.px_list ? sizeof(unsigned) * (v.px_elems + rtk::kPxHdrInts) : 0);
  }
  rt_device_free(ctx, out);
  rt_prepared_free(ctx, ps);
  rt_scene_free(ctx, sc);
  rt_context_destroy(ctx);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) die(2, "usage", "view_order_check <cases> <results>");
  Reader in;
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) die(2, "cases", "cannot open");
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in.v.resize(static_cast<size_t>(bytes) / 4);
    if (bytes < 8 || bytes % 4 || std::fread(in.v.data(), 4, in.v.size(), f) != in.v.size()) die(2, "cases", "cannot read");
    std::fclose(f);
  }
  if (in.i() != 0x44524f56) die(2, "cases", "not a cases file");   // 'VORD'
  const int ncases = in.i();
  g_out = std::fopen(argv[2], "wb");
  if (!g_out) die(2, "results", "cannot open");
  hipStream_t st = nullptr;
  hip_ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
  for (int c = 0; c < ncases; ++c) {
    const int kind = in.i();
    if (kind == 1) tile_order_case(in, st);
    else if (kind == 2) px_order_case(in, st);
    else if (kind == 3) first_order_case(in, st);
    else if (kind == 4) view_case(in);
    else die(2, "cases", "unknown kind");
  }
  hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
  if (std::fclose(g_out) != 0) die(1, "results", "close failed");
  std::printf("view_order_check: %d cases\n", ncases);
  return 0;
}
