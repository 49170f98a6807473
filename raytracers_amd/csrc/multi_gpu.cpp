// multi_gpu.cpp -- one process, several MI355X: the row-tile partition of SURVEY.md 8(e) behind the
// C ABI (rt_context_create_multi / futhark_context_config_set_device("0-7")), so that the reference's
// own harness (futhark/main.c:59-64 context, :107-124 render + sync loop, :126-135 values) drives N GPUs
// without a line changed.
//
// A multi-device context is a PARENT context on the first device plus one child context (own
// stream) per device entry.  prepare_scene replicates the scene: every device builds its own BVH from
// the same spheres (bit-identical by construction; <= 66 MB even for the 10^6-sphere scene).  render
// fans out rt_render_part over the children -- part i of N = the tiles t of 8 rows with t % N == i,
// cyclic because contiguous bands would give irreg's devices 0.1 % .. 25 % of the work each -- and
// gathers the packed parts on the first device, where one kernel (place_all_kernel) scatters them
// into the [h][w]i32 image:
//   * RCCL (default when the devices are distinct and librccl loads): one ncclCommInitAll communicator
//     per device, grouped ncclSend (child stream, right behind the render) / ncclRecv (parent stream)
//     straight into the part's slice of the stacked buffer -- point-to-point over xGMI, 7 links into
//     device 0 in parallel; nothing is reduced, so no ring collective is involved;
//   * peer copies (hipMemcpyPeerAsync on the child's stream; also the fallback for a failing RCCL);
//   * DIRECT STORES (gather = 3; what "auto" picks when every device can reach the first one): no part buffers, no
//     gather, no assembly launch -- every device's kernel stores its finished pixels at their places in the caller's image
//     on the first device (rt_render_part_inplace's layout; peer access over xGMI).  The 4-byte pixel stores leave a device
//     while it is still tracing, so the exchange is off the frame's critical path: behind the slowest device's kernel there
//     is only an event.  (Modelled, tools/scale_prediction.py: irreg 4000x4000 on 8 devices 516 -> ~420 us per frame.)
// librccl is loaded on demand (dlopen): the single-device library has no RCCL dependency.
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl itself is dlopen'ed at the first multi-device frame

#include <algorithm>
#include <cstring>
#include <future>
#include <memory>

#include "rt_internal.hpp"

struct rt_group {
  std::vector<rt_context *> kids;   // one per device entry, own stream each
  std::vector<int> devices;
  bool distinct = true;
  int gather = 0;                   // 0 auto, 1 peer copies, 2 RCCL (then part 0 goes through RCCL too), 3 direct stores into the image on the first device
  bool peer_ok = true;              // every device can store into the first device's memory (peer access enabled, or the same device)
  hipEvent_t ev_begin = nullptr;    // direct stores: the parent stream's position when the frame was asked for (the image's previous readers)
  bool last_direct = false;         // what carried the last frame (rt_context_gather_mode)
  bool rendered = false;            // a frame has been rendered (before that the getter reports what auto WOULD pick)
  // gather buffers, grown on demand
  int64_t buf_elems = 0;            // capacity of one part in int32
  std::vector<int32_t *> part;      // part[i] on device i (kid 0 renders into the stacked buffer unless gather == 2)
  int32_t *stacked = nullptr;       // first device: kids x buf_elems
  std::vector<hipEvent_t> ev_part;  // kid i's render (+ peer copy) of the current frame
  hipEvent_t ev_placed = nullptr;   // the parent's assembly of the current frame
  bool placed_valid = false;
  // RCCL, loaded on demand
  void *rccl = nullptr;
  bool rccl_tried = false;
  std::vector<ncclComm_t> comms;
  decltype(&ncclCommInitAll) p_init = nullptr;
  decltype(&ncclCommDestroy) p_destroy = nullptr;
  decltype(&ncclGroupStart) p_gstart = nullptr;
  decltype(&ncclGroupEnd) p_gend = nullptr;
  decltype(&ncclSend) p_send = nullptr;
  decltype(&ncclRecv) p_recv = nullptr;
  decltype(&ncclGetErrorString) p_errstr = nullptr;
  std::string rccl_note;            // why RCCL is not in use (rt_context_report)
  bool rccl_failed = false;         // a gather through RCCL failed at run time: peer copies from then on
};

namespace {

using rti::fail;

bool load_rccl(rt_group *g) {
  if (g->rccl_tried) return !g->comms.empty();
  g->rccl_tried = true;
  if (!g->distinct) { g->rccl_note = "device list has repeats (test mode): peer copies"; return false; }
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
    g->rccl = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (g->rccl) break;
  }
  if (!g->rccl) { g->rccl_note = std::string("librccl not loadable: ") + dlerror(); return false; }
#define RT_SYM(field, sym)                                                         \
  g->field = reinterpret_cast<decltype(g->field)>(dlsym(g->rccl, #sym));          \
  if (!g->field) { g->rccl_note = "librccl lacks " #sym; return false; }
  RT_SYM(p_init, ncclCommInitAll) RT_SYM(p_destroy, ncclCommDestroy) RT_SYM(p_gstart, ncclGroupStart)
  RT_SYM(p_gend, ncclGroupEnd) RT_SYM(p_send, ncclSend) RT_SYM(p_recv, ncclRecv) RT_SYM(p_errstr, ncclGetErrorString)
#undef RT_SYM
  g->comms.assign(g->devices.size(), nullptr);
  const ncclResult_t r = g->p_init(g->comms.data(), static_cast<int>(g->devices.size()), g->devices.data());
  if (r != ncclSuccess) {
    g->rccl_note = std::string("ncclCommInitAll failed: ") + g->p_errstr(r);
    g->comms.clear();
    return false;
  }
  return true;
}

int ensure_buffers(rt_context *ctx, int64_t elems) {
  rt_group *g = ctx->group;
  if (elems <= g->buf_elems) return 0;
  if (int rc = rti::group_sync(ctx)) return rc;
  const size_t n = g->kids.size();
  for (size_t i = 0; i < n; ++i)
    if (g->part[i]) {
      (void)hipSetDevice(g->devices[i]);
      (void)hipFree(g->part[i]);
      g->part[i] = nullptr;
    }
  RT_HIP(ctx, hipSetDevice(ctx->device));
  if (g->stacked) (void)hipFree(g->stacked);
  g->stacked = nullptr;
  g->buf_elems = 0;
  RT_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&g->stacked), sizeof(int32_t) * static_cast<size_t>(elems) * n));
  for (size_t i = 0; i < n; ++i) {
    RT_HIP(ctx, hipSetDevice(g->devices[i]));
    RT_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&g->part[i]), sizeof(int32_t) * static_cast<size_t>(elems)));
  }
  RT_HIP(ctx, hipSetDevice(ctx->device));
  g->buf_elems = elems;
  g->placed_valid = false;
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
extern "C" int rt_context_create_multi(rt_context **out, const int *devices, int ndev) {
  if (!out || !devices || ndev < 1 || ndev > 64) return 1;
  *out = nullptr;
  rt_context *parent = nullptr;
  if (int rc = rt_context_create(&parent, devices[0], nullptr, 0)) return rc;
  rt_group *g = new rt_group;
  parent->group = g;   // owned by the parent from here on: rt_context_destroy releases whatever exists so far
  g->devices.assign(devices, devices + ndev);
  for (int i = 0; i < ndev; ++i)
    for (int j = 0; j < i; ++j)
      if (devices[i] == devices[j]) g->distinct = false;
  auto bail = [&](int code, const std::string &why) {
    std::fprintf(stderr, "libray_mi355x: rt_context_create_multi: %s\n", why.c_str());
    rt_context_destroy(parent);
    return code;
  };
  g->part.assign(static_cast<size_t>(ndev), nullptr);
  g->ev_part.assign(static_cast<size_t>(ndev), nullptr);
  for (int i = 0; i < ndev; ++i) {
    rt_context *kid = nullptr;
    if (int rc = rt_context_create(&kid, devices[i], nullptr, 0)) return bail(rc, "cannot create a context on device " + std::to_string(devices[i]));
    g->kids.push_back(kid);
    // (system-scope release: what a device stored into the first device's memory must be visible there once the event has passed)
    if (hipSetDevice(devices[i]) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_part[static_cast<size_t>(i)], hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess)
      return bail(8, "hipEventCreate failed");
    if (devices[i] != devices[0]) {
      // direct xGMI access both ways (an already enabled pair reports an error that is not one)
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) != hipSuccess || !can) g->peer_ok = false;
      const hipError_t pe = hipDeviceEnablePeerAccess(devices[0], 0);
      if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) g->peer_ok = false;
      (void)hipSetDevice(devices[0]);
      (void)hipDeviceEnablePeerAccess(devices[i], 0);
      (void)hipGetLastError();
    }
  }
  if (hipSetDevice(devices[0]) != hipSuccess || hipEventCreateWithFlags(&g->ev_placed, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev_begin, hipEventDisableTiming) != hipSuccess)
    return bail(8, "hipEventCreate failed");
  *out = parent;
  return 0;
}

extern "C" int rt_context_num_devices(const rt_context *ctx) {
  if (!ctx) return 0;
  return ctx->group ? static_cast<int>(ctx->group->kids.size()) : 1;
}

extern "C" const char *rt_context_gather_mode(rt_context *ctx) {
  RT_LOCK(ctx);
  if (!ctx || !ctx->group || ctx->group->kids.size() < 2) return ctx && ctx->group && ctx->group->gather == 2 ? "rccl" : "none";
  rt_group *g = ctx->group;
  // (auto: what the last frame was carried by -- an image the other devices cannot be shown to reach goes through the gather)
  if (g->gather == 3 || (g->gather == 0 && g->peer_ok && (g->last_direct || !g->rendered))) return "direct-store";
  if (g->gather == 1 || g->rccl_failed || !g->distinct) return "peer-copy";
  if (!g->rccl_tried) return "rccl (loaded at the first frame; peer copies if that fails)";   // (a getter creates no communicators)
  return g->comms.empty() ? "peer-copy" : "rccl";
}

// ranks of the RCCL communicator that carries the gather (0: none -- one device, direct stores or peer copies, or RCCL not loaded yet)
extern "C" int rt_context_rccl_ranks(rt_context *ctx) {
  RT_LOCK(ctx);
  if (!ctx || !ctx->group || ctx->group->rccl_failed) return 0;
  return static_cast<int>(ctx->group->comms.size());
}

void rti::group_destroy(rt_context *ctx) {
  rt_group *g = ctx ? ctx->group : nullptr;
  if (!g) return;
  (void)rti::group_sync(ctx);
  for (ncclComm_t c : g->comms)
    if (c && g->p_destroy) (void)g->p_destroy(c);
  for (size_t i = 0; i < g->devices.size(); ++i) {
    (void)hipSetDevice(g->devices[i]);
    if (i < g->part.size() && g->part[i]) (void)hipFree(g->part[i]);
    if (i < g->ev_part.size() && g->ev_part[i]) (void)hipEventDestroy(g->ev_part[i]);
    if (i < g->kids.size()) rt_context_destroy(g->kids[i]);
  }
  (void)hipSetDevice(ctx->device);
  if (g->stacked) (void)hipFree(g->stacked);
  if (g->ev_placed) (void)hipEventDestroy(g->ev_placed);
  if (g->ev_begin) (void)hipEventDestroy(g->ev_begin);
  // librccl stays loaded: unloading a library that owns device state at exit time is asking for trouble
  delete g;
  ctx->group = nullptr;
}

int rti::group_sync(rt_context *ctx) {
  rt_group *g = ctx->group;
  // Every stream is drained even when one reports an error, and a device whose launch died gets its ticket counters
  // re-zeroed (the launch's last wave never did: later frames would draw out-of-range tickets and silently leave that
  // device's rows stale -- the single-device rt_context_sync does the same).
  hipError_t first = hipSuccess;
  std::string where;
  for (rt_context *kid : g->kids) {
    hipError_t e = hipSetDevice(kid->device);
    if (e == hipSuccess) e = hipStreamSynchronize(kid->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      (void)hipMemset(kid->queue_dev, 0, sizeof(unsigned) * rtk::kQueueDwords);
      if (first == hipSuccess) { first = e; where = "device " + std::to_string(kid->device); }
    }
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipMemset(ctx->queue_dev, 0, sizeof(unsigned) * rtk::kQueueDwords);
    if (first == hipSuccess) { first = e; where = "first device"; }
  }
  if (first != hipSuccess) return rti::hip_fail(ctx, first, ("stream synchronisation on " + where + " (ticket counters reset)").c_str());
  return 0;
}

void rti::group_mark_synced(rt_context *ctx) {
  for (rt_context *kid : ctx->group->kids) kid->synced_since_render = true;
}

int rti::group_set_variant(rt_context *ctx, int variant) {
  for (rt_context *kid : ctx->group->kids)
    if (rt_context_set_variant(kid, variant)) return fail(ctx, rt_last_error(kid));
  return 0;
}

int rti::group_set_option(rt_context *ctx, const char *name, int64_t value) {
  if (std::strcmp(name, "gather") == 0) {
    if (value < 0 || value > 3) return fail(ctx, "gather must be 0 (auto), 1 (peer copies), 2 (RCCL) or 3 (direct stores into the first device's image)");
    if (value == 3 && !ctx->group->peer_ok) return fail(ctx, "gather=3 (direct stores): a device of this context cannot access the first device's memory");
    if (int rc = rti::group_sync(ctx)) return rc;
    ctx->group->gather = static_cast<int>(value);
    return 0;
  }
  for (rt_context *kid : ctx->group->kids)
    if (rt_context_set_option(kid, name, value)) return fail(ctx, rt_last_error(kid));
  return -1;   // not a group-only option: the caller applies it to the parent as well
}

// prepare_scene on every device: the parent's own prepared scene (first device) serves child 0, children 1.. build
// replicas concurrently -- one host thread per device, started BEFORE the parent builds its own (the build ends in a
// stream synchronise, and the reference's harness times this call).
void rti::group_prepare_begin(rt_context *ctx, rt_prepared *ps, int64_t h, int64_t w, const rt_scene *scene) {
  rt_group *g = ctx->group;
  const size_t n = g->kids.size();
  ps->replicas.assign(n, nullptr);
  ps->replica_jobs.clear();
  for (size_t i = 1; i < n; ++i)
    ps->replica_jobs.push_back(std::async(std::launch::async, [=] { return rt_prepare_scene(g->kids[i], &ps->replicas[i], h, w, scene); }));
}
int rti::group_prepare_end(rt_context *ctx, rt_prepared *ps) {
  rt_group *g = ctx->group;
  int rc = 0;
  for (size_t i = 0; i < ps->replica_jobs.size(); ++i)
    if (ps->replica_jobs[i].get() != 0 && !rc)
      rc = fail(ctx, std::string("device ") + std::to_string(g->devices[i + 1]) + ": " + rt_last_error(g->kids[i + 1]));
  ps->replica_jobs.clear();
  (void)hipSetDevice(ctx->device);
  return rc;
}

void rti::group_prepared_free(rt_context *ctx, rt_prepared *ps) {
  rt_group *g = ctx ? ctx->group : nullptr;
  if (g) (void)rti::group_sync(ctx);
  for (size_t i = 0; i < ps->replicas.size(); ++i)
    if (ps->replicas[i]) rt_prepared_free(g && i < g->kids.size() ? g->kids[i] : nullptr, ps->replicas[i]);
  ps->replicas.clear();
  if (ctx) (void)hipSetDevice(ctx->device);
}

int rti::group_render(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, int32_t max_depth, int32_t *out_dev,
                      const float *cam12, int32_t nframes, int64_t frame_stride, const float *cams12) {
  rt_group *g = ctx->group;
  const int n = static_cast<int>(g->kids.size());
  if (ps->replicas.size() != static_cast<size_t>(n)) return fail(ctx, "prepared scene does not belong to this multi-device context");
  if (!out_dev) return fail(ctx, "null output pointer");
  if (h <= 0 || w <= 0 || h > (1 << 20) || w > (1 << 20) || h * w > (int64_t(1) << 30)) return fail(ctx, "image size out of range");
  if (nframes < 1 || (nframes > 1 && (frame_stride < h * w || frame_stride * nframes >= (int64_t(1) << 31))))
    return fail(ctx, "bad batch: nframes >= 1, frame_stride >= h * w, nframes * frame_stride < 2^31");
  // (enqueue_render's limit, on the whole frame -- no device's rows have more tiles -- so that no device has launched when another one refuses)
  if (rti::tiles_of(h, w) * nframes >= rti::kMaxPositions)
    return fail(ctx, "bad batch: tiles per frame x frames < 2^26 (a frame has ceil(rows / 8) x ceil(w / 8) tiles of 8 x 8 pixels)");
  constexpr int32_t kRows = 8;
  // Auto mode takes the direct path only for an image the other devices can certainly reach: a device allocation on the first
  // device, which hipDeviceEnablePeerAccess covers (memory from a virtual-memory mapping or another device's pool is not, and
  // an unreadable pointer says nothing) -- any other image goes through the gather, which only the first device touches.
  bool direct = g->gather == 3;
  if (g->gather == 0 && g->peer_ok) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, out_dev) == hipSuccess) direct = at.type == hipMemoryTypeDevice && at.device == g->devices[0];
    else (void)hipGetLastError();
  }
  g->last_direct = direct;
  g->rendered = true;
  if (direct) {
    // ---- direct stores: every device writes its rows where the image has them; nothing is gathered or assembled ----
    // (the image's previous readers sit on the parent's stream: the devices start behind them)
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipEventRecord(g->ev_begin, ctx->stream));
    const int64_t fs = nframes > 1 ? frame_stride : h * w;
    for (int i = 0; i < n; ++i) {
      rt_context *kid = g->kids[static_cast<size_t>(i)];
      RT_HIP(ctx, hipSetDevice(kid->device));
      RT_HIP(ctx, hipStreamWaitEvent(kid->stream, g->ev_begin, 0));
      const rt_prepared *kps = i == 0 ? ps : ps->replicas[static_cast<size_t>(i)];
      const float *cams_dev = nullptr;
      if (nframes > 1 && rti::stage_cams(kid, cams12, nframes, &cams_dev)) return fail(ctx, rt_last_error(kid));
      if (rti::enqueue_render(kid, kps, h, w, max_depth, kRows, i, n, out_dev, false, cam12, nframes, fs, cams_dev, true))
        return fail(ctx, rt_last_error(kid));
      RT_HIP(ctx, hipEventRecord(g->ev_part[static_cast<size_t>(i)], kid->stream));
    }
    RT_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n; ++i) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, g->ev_part[static_cast<size_t>(i)], 0));
    return 0;
  }
  const bool want_rccl = !g->rccl_failed && (g->gather == 2 || (g->gather == 0 && n > 1));
  bool rccl = want_rccl && load_rccl(g);
  if (g->gather == 2 && !rccl) return fail(ctx, "gather=2 (RCCL) requested but unavailable: " + (g->rccl_failed ? std::string("it failed at run time") : g->rccl_note));
  if (n == 1 && !rccl) {
    const float *cams_dev = nullptr;
    if (nframes > 1 && rti::stage_cams(g->kids[0], cams12, nframes, &cams_dev)) return fail(ctx, rt_last_error(g->kids[0]));
    if (rti::enqueue_render(g->kids[0], ps, h, w, max_depth, kRows, 0, 1, out_dev, false, cam12, nframes, frame_stride, cams_dev))
      return fail(ctx, rt_last_error(g->kids[0]));
    // the frame lives on child 0's stream: order the parent's stream (values, frees) behind it
    RT_HIP(ctx, hipEventRecord(g->ev_part[0], g->kids[0]->stream));
    RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, g->ev_part[0], 0));
    return 0;
  }
  // A device's part buffer: its rows of frame 0, then of frame 1, ... (pad_rows * w elements apart).
  int64_t pad_rows = 0;
  for (int p = 0; p < n; ++p) pad_rows = std::max<int64_t>(pad_rows, rt::part_rows(h, kRows, p, n));
  const int64_t fstride = pad_rows * w, stride = fstride * nframes;
  if (stride >= (int64_t(1) << 31)) return fail(ctx, "batch too large for one gather");
  if (int rc = ensure_buffers(ctx, stride)) return rc;
  const bool all_rccl = rccl && g->gather == 2;   // forced: part 0 travels through RCCL as well (self send/recv)
  auto part_elems = [&](int i) {                  // what device i has to deliver (0: nothing)
    const int64_t rows = rt::part_rows(h, kRows, i, n);
    return rows > 0 ? static_cast<size_t>((nframes - 1) * fstride + rows * w) : size_t(0);
  };
  for (int i = 0; i < n; ++i) {
    rt_context *kid = g->kids[static_cast<size_t>(i)];
    RT_HIP(ctx, hipSetDevice(kid->device));
    // the previous frame's assembly must have read the stacked buffer before this frame overwrites it
    if (g->placed_valid) RT_HIP(ctx, hipStreamWaitEvent(kid->stream, g->ev_placed, 0));
    const bool direct = i == 0 && !all_rccl;
    int32_t *dst = direct ? g->stacked : g->part[static_cast<size_t>(i)];
    const rt_prepared *kps = i == 0 ? ps : ps->replicas[static_cast<size_t>(i)];
    const float *cams_dev = nullptr;
    if (nframes > 1 && rti::stage_cams(kid, cams12, nframes, &cams_dev)) return fail(ctx, rt_last_error(kid));
    if (rti::enqueue_render(kid, kps, h, w, max_depth, kRows, i, n, dst, false, cam12, nframes, fstride, cams_dev)) return fail(ctx, rt_last_error(kid));
    if (!direct && !rccl && part_elems(i) > 0)
      RT_HIP(ctx, hipMemcpyPeerAsync(g->stacked + static_cast<int64_t>(i) * stride, g->devices[0], dst, kid->device,
                                     sizeof(int32_t) * part_elems(i), kid->stream));
    RT_HIP(ctx, hipEventRecord(g->ev_part[static_cast<size_t>(i)], kid->stream));
  }
  RT_HIP(ctx, hipSetDevice(ctx->device));
  if (rccl) {
    // part 0 (or, forced, its send) must be complete on the parent's stream's view
    RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, g->ev_part[0], 0));
    ncclResult_t r = g->p_gstart();
    for (int i = all_rccl ? 0 : 1; i < n && r == ncclSuccess; ++i) {
      const size_t count = part_elems(i);
      if (count == 0) continue;
      // comm[0]'s operations all sit on the parent's stream; a child's send follows its render on its own stream
      hipStream_t sstream = i == 0 ? ctx->stream : g->kids[static_cast<size_t>(i)]->stream;
      r = g->p_send(g->part[static_cast<size_t>(i)], count, ncclInt32, 0, g->comms[static_cast<size_t>(i)], sstream);
      if (r == ncclSuccess) r = g->p_recv(g->stacked + static_cast<int64_t>(i) * stride, count, ncclInt32, i, g->comms[0], ctx->stream);
    }
    const ncclResult_t e = g->p_gend();
    if (r == ncclSuccess) r = e;
    if (r != ncclSuccess) {
      // The RCCL path has only ever been exercised on one device (the round-end 8-GPU node is the first real run): a
      // failure must not take the harness down.  This frame's parts still sit in the devices' part buffers: move them
      // with peer copies, and stay with peer copies.
      if (g->gather == 2) return fail(ctx, std::string("RCCL gather failed: ") + g->p_errstr(r));
      g->rccl_failed = true;
      g->rccl_note = std::string("RCCL gather failed at run time (") + g->p_errstr(r) + "): peer copies since";
      std::fprintf(stderr, "libray_mi355x: %s\n", g->rccl_note.c_str());
      rccl = false;
      for (int i = 1; i < n; ++i) {
        rt_context *kid = g->kids[static_cast<size_t>(i)];
        if (part_elems(i) == 0) continue;
        RT_HIP(ctx, hipSetDevice(kid->device));
        RT_HIP(ctx, hipMemcpyPeerAsync(g->stacked + static_cast<int64_t>(i) * stride, g->devices[0], g->part[static_cast<size_t>(i)],
                                       kid->device, sizeof(int32_t) * part_elems(i), kid->stream));
        RT_HIP(ctx, hipEventRecord(g->ev_part[static_cast<size_t>(i)], kid->stream));
      }
      RT_HIP(ctx, hipSetDevice(ctx->device));
    }
  }
  if (!rccl)
    for (int i = 0; i < n; ++i) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, g->ev_part[static_cast<size_t>(i)], 0));
  // one assembly launch for all frames of the batch
  RT_HIP(ctx, rtk::launch_place_all(g->stacked, out_dev, static_cast<int>(w), static_cast<int>(h), kRows, n, static_cast<size_t>(stride),
                                    ctx->stream, nframes, static_cast<size_t>(fstride), static_cast<size_t>(nframes > 1 ? frame_stride : h * w)));
  RT_HIP(ctx, hipEventRecord(g->ev_placed, ctx->stream));
  g->placed_valid = true;
  return 0;
}
