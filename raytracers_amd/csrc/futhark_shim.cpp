// futhark_shim.cpp -- the Futhark-shaped drop-in boundary of libray_mi355x.so (include/ray.h) that the reference's futhark/main.c is
// written against: thin wrappers over the rt_* surface (api.cpp), plus the pool of result images.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ray.h"
#include "../../include/rt_mi355x.h"
#include "rt_internal.hpp"

using rti::pool_alloc;
using rti::pool_free;

// ====================================================================================
// The Futhark-shaped boundary (include/ray.h) -- thin wrappers over the rt_* surface.
// ====================================================================================
struct futhark_context_config {
  int device = -1;
  std::vector<int> devices;   // more than one entry: a multi-device context (set_device("0-7") / "0,2,4"; env RT_DEVICES)
  int debugging = 0, logging = 0, profiling = 0;
};
struct futhark_context {
  std::recursive_mutex mu;   // Futhark's context lock: every futhark_* entry holds it (the image pool, the pending error, the counters)
  rt_context *rt = nullptr;
  // freed images are kept for reuse: main.c frees and re-renders every run, and a
  // hipFree/hipMalloc pair per frame costs more than the frame itself
  struct PooledImage { int64_t elems; int32_t *dev; size_t block_bytes; };
  std::vector<PooledImage> image_pool;
  std::string pending;   // error not yet collected by futhark_context_get_error
  int logging = 0;
  uint64_t renders = 0, prepares = 0;
};
struct futhark_opaque_scene {
  rt_scene *s = nullptr;
};
struct futhark_opaque_prepared_scene {
  rt_prepared *p = nullptr;
};
struct futhark_i32_2d {
  int32_t *dev = nullptr;
  int64_t shape[2] = {0, 0};
  size_t block_bytes = 0;   // != 0: a block of the context's arena / block pool (image_alloc); 0: rt_device_alloc's
};
namespace {
// An entry point's result array from the context's arena (pool_alloc): a hipMalloc of 4 MB inside the harness's first render call was ~0.1 ms
// of its first frame.  Freed (image_release) behind a drained stream, like rt_device_free.
int image_alloc(rt_context *ctx, void **dev, size_t *block_bytes, int64_t bytes) {
  RT_LOCK(ctx);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  char *blk = nullptr;
  *block_bytes = static_cast<size_t>(std::max<int64_t>(bytes, 16));
  RT_HIP(ctx, pool_alloc(ctx, &blk, block_bytes));
  *dev = blk;
  return 0;
}
int image_release(rt_context *ctx, void *dev, size_t block_bytes) {
  if (!block_bytes) return rt_device_free(ctx, dev);
  RT_LOCK(ctx);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pool_free(ctx, static_cast<char *>(dev), block_bytes);
  return 0;
}
}  // namespace

#ifndef RT_NO_CONTEXT_LOCK
#define FUT_LOCK(ctx) std::unique_lock<std::recursive_mutex> fut_lock_ = (ctx) ? std::unique_lock<std::recursive_mutex>((ctx)->mu) : std::unique_lock<std::recursive_mutex>()
#else
#define FUT_LOCK(ctx) (void)(ctx)
#endif

namespace {
int fut_fail(futhark_context *ctx, int rc) {
  if (rc && ctx) ctx->pending = rt_last_error(ctx->rt);
  return rc;
}
}  // namespace

extern "C" struct futhark_context_config *futhark_context_config_new(void) { return new futhark_context_config(); }
extern "C" void futhark_context_config_free(struct futhark_context_config *cfg) { delete cfg; }
extern "C" void futhark_context_config_set_debugging(struct futhark_context_config *cfg, int flag) { if (cfg) cfg->debugging = flag; }
extern "C" void futhark_context_config_set_logging(struct futhark_context_config *cfg, int flag) { if (cfg) cfg->logging = flag; }
extern "C" void futhark_context_config_set_profiling(struct futhark_context_config *cfg, int flag) { if (cfg) cfg->profiling = flag; }
// "k" / "#k": HIP device k (the Futhark convention); "a-b" or "a,b,c": several devices = one multi-device
// context (the frame is partitioned over them, include/rt_mi355x.h: rt_context_create_multi)
static std::vector<int> parse_device_list(const char *s) {
  std::vector<int> out;
  while (*s) {
    while (*s == ' ' || *s == ',' || *s == '#') ++s;
    if (!*s) break;
    char *end = nullptr;
    const long a = std::strtol(s, &end, 10);
    if (end == s || a < 0) return {};
    s = end;
    long b = a;
    if (*s == '-') {
      b = std::strtol(s + 1, &end, 10);
      if (end == s + 1 || b < a) return {};
      s = end;
    }
    for (long d = a; d <= b && out.size() < 64; ++d) out.push_back(static_cast<int>(d));
  }
  return out;
}
extern "C" void futhark_context_config_set_device(struct futhark_context_config *cfg, const char *s) {
  if (!cfg || !s) return;
  cfg->devices = parse_device_list(s);
  cfg->device = cfg->devices.empty() ? std::atoi(*s == '#' ? s + 1 : s) : cfg->devices[0];
}

extern "C" void futhark_context_config_set_num_threads(struct futhark_context_config *, int) {}
extern "C" void futhark_context_config_set_cache_file(struct futhark_context_config *, const char *) {}

extern "C" struct futhark_context *futhark_context_new(struct futhark_context_config *cfg) {
  auto ctx = std::make_unique<futhark_context>();
  ctx->logging = cfg ? (cfg->logging | cfg->debugging) : 0;
  // RT_DEVICES lets a harness that never calls set_device (futhark/main.c does not) use several GPUs
  // (an explicit futhark_context_config_set_device wins over the environment)
  std::vector<int> devs = cfg ? cfg->devices : std::vector<int>();
  if (const char *env = std::getenv("RT_DEVICES"); env && devs.empty() && !(cfg && cfg->device >= 0)) devs = parse_device_list(env);
  const int rc = devs.size() > 1 ? rt_context_create_multi(&ctx->rt, devs.data(), static_cast<int>(devs.size()))
                                 : rt_context_create(&ctx->rt, !devs.empty() ? devs[0] : (cfg ? cfg->device : -1), nullptr, 0);
  if (rc) {
    // Futhark returns a context whose error is set; main.c asserts it is NULL.
    ctx->pending = "libray_mi355x: cannot create a HIP context (code " + std::to_string(rc) + "); no CPU path exists";
  }
  return ctx.release();
}
extern "C" void futhark_context_free(struct futhark_context *ctx) {
  if (!ctx) return;
  for (auto &e : ctx->image_pool) (void)image_release(ctx->rt, e.dev, e.block_bytes);
  rt_context_destroy(ctx->rt);
  delete ctx;
}
extern "C" char *futhark_context_get_error(struct futhark_context *ctx) {
  FUT_LOCK(ctx);
  if (!ctx || ctx->pending.empty()) return nullptr;
  char *s = static_cast<char *>(std::malloc(ctx->pending.size() + 1));
  if (s) std::memcpy(s, ctx->pending.c_str(), ctx->pending.size() + 1);
  ctx->pending.clear();
  return s;
}
extern "C" int futhark_context_sync(struct futhark_context *ctx) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt) return 1;
  return fut_fail(ctx, rt_context_sync(ctx->rt));
}
extern "C" char *futhark_context_report(struct futhark_context *ctx) {
  FUT_LOCK(ctx);
  char buf[512];
  int dev = -1, cus = 0, lds = 0;
  char name[64] = "";
  if (ctx && ctx->rt) rt_context_device_info(ctx->rt, &dev, &cus, &lds, name, sizeof name);
  std::snprintf(buf, sizeof buf, "libray_mi355x: device %d (%s), %d CUs, %d B LDS/CU; %d device(s), framebuffer gather: %s; %llu prepare_scene, %llu render calls\n",
                dev, name, cus, lds, ctx && ctx->rt ? rt_context_num_devices(ctx->rt) : 0,
                ctx && ctx->rt ? rt_context_gather_mode(ctx->rt) : "none", ctx ? (unsigned long long)ctx->prepares : 0ull,
                ctx ? (unsigned long long)ctx->renders : 0ull);
  char *s = static_cast<char *>(std::malloc(std::strlen(buf) + 1));
  if (s) std::strcpy(s, buf);
  return s;
}

extern "C" int futhark_entry_rgbbox(struct futhark_context *ctx, struct futhark_opaque_scene **out0) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !out0) return 1;
  auto o = std::make_unique<futhark_opaque_scene>();
  if (int rc = rt_scene_rgbbox(ctx->rt, &o->s)) return fut_fail(ctx, rc);
  *out0 = o.release();
  return 0;
}
extern "C" int futhark_entry_irreg(struct futhark_context *ctx, struct futhark_opaque_scene **out0) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !out0) return 1;
  auto o = std::make_unique<futhark_opaque_scene>();
  if (int rc = rt_scene_irreg(ctx->rt, &o->s)) return fut_fail(ctx, rc);
  *out0 = o.release();
  return 0;
}
extern "C" int futhark_entry_prepare_scene(struct futhark_context *ctx, struct futhark_opaque_prepared_scene **out0,
                                           const int64_t in0, const int64_t in1, const struct futhark_opaque_scene *in2) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !out0 || !in2) return 1;
  auto o = std::make_unique<futhark_opaque_prepared_scene>();
  if (int rc = rt_prepare_scene(ctx->rt, &o->p, in0, in1, in2->s)) return fut_fail(ctx, rc);
  ctx->prepares++;
  *out0 = o.release();
  return 0;
}
extern "C" int futhark_entry_render(struct futhark_context *ctx, struct futhark_i32_2d **out0, const int64_t in0,
                                    const int64_t in1, const struct futhark_opaque_prepared_scene *in2) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !out0 || !in2) return 1;
  auto img = std::make_unique<futhark_i32_2d>();
  void *dev = nullptr;
  for (size_t i = 0; i < ctx->image_pool.size(); ++i)
    if (ctx->image_pool[i].elems == in0 * in1) {
      dev = ctx->image_pool[i].dev;   // same stream => the new frame orders after any pending use
      img->block_bytes = ctx->image_pool[i].block_bytes;
      ctx->image_pool.erase(ctx->image_pool.begin() + static_cast<long>(i));
      break;
    }
  if (!dev)
    if (int rc = image_alloc(ctx->rt, &dev, &img->block_bytes, static_cast<int64_t>(sizeof(int32_t)) * in0 * in1)) return fut_fail(ctx, rc);
  img->dev = static_cast<int32_t *>(dev);
  img->shape[0] = in0;
  img->shape[1] = in1;
  if (int rc = rt_render(ctx->rt, in2->p, in0, in1, img->dev)) {
    (void)image_release(ctx->rt, dev, img->block_bytes);
    return fut_fail(ctx, rc);
  }
  ctx->renders++;
  *out0 = img.release();
  return 0;
}
extern "C" int futhark_values_i32_2d(struct futhark_context *ctx, struct futhark_i32_2d *arr, int32_t *data) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !arr || !data) return 1;
  return fut_fail(ctx, rt_copy_to_host(ctx->rt, data, arr->dev, static_cast<int64_t>(sizeof(int32_t)) * arr->shape[0] * arr->shape[1]));
}
extern "C" int futhark_free_i32_2d(struct futhark_context *ctx, struct futhark_i32_2d *arr) {
  FUT_LOCK(ctx);
  if (!arr) return 0;
  int rc = 0;
  if (ctx && ctx->rt && arr->dev) {
    if (ctx->image_pool.size() < 4) ctx->image_pool.push_back({arr->shape[0] * arr->shape[1], arr->dev, arr->block_bytes});
    else rc = image_release(ctx->rt, arr->dev, arr->block_bytes);
  }
  delete arr;
  return fut_fail(ctx, rc);
}
extern "C" struct futhark_i32_2d *futhark_new_i32_2d(struct futhark_context *ctx, const int32_t *data, int64_t dim0, int64_t dim1) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt || !data || dim0 < 0 || dim1 < 0) return nullptr;
  auto arr = std::make_unique<futhark_i32_2d>();
  arr->shape[0] = dim0; arr->shape[1] = dim1;
  const int64_t bytes = static_cast<int64_t>(sizeof(int32_t)) * dim0 * dim1;
  if (rt_device_alloc(ctx->rt, reinterpret_cast<void **>(&arr->dev), std::max<int64_t>(bytes, 4)) != 0) { fut_fail(ctx, 1); return nullptr; }
  if (bytes > 0 && hipMemcpy(arr->dev, data, static_cast<size_t>(bytes), hipMemcpyHostToDevice) != hipSuccess) {
    (void)rt_device_free(ctx->rt, arr->dev);
    ctx->pending = "futhark_new_i32_2d: host to device copy failed";
    return nullptr;
  }
  return arr.release();
}
extern "C" int32_t *futhark_values_raw_i32_2d(struct futhark_context *, struct futhark_i32_2d *arr) { return arr ? arr->dev : nullptr; }
extern "C" int futhark_context_clear_caches(struct futhark_context *ctx) {
  FUT_LOCK(ctx);
  if (!ctx || !ctx->rt) return 1;
  if (rt_context_sync(ctx->rt)) return fut_fail(ctx, 1);
  for (auto &im : ctx->image_pool) (void)image_release(ctx->rt, im.dev, im.block_bytes);
  ctx->image_pool.clear();
  for (auto &b : ctx->rt->pool) (void)hipFree(b.p);
  ctx->rt->pool.clear();
  return 0;
}
extern "C" void futhark_context_pause_profiling(struct futhark_context *) {}
extern "C" void futhark_context_unpause_profiling(struct futhark_context *) {}

extern "C" const int64_t *futhark_shape_i32_2d(struct futhark_context *, struct futhark_i32_2d *arr) {
  return arr ? arr->shape : nullptr;
}
extern "C" int futhark_free_opaque_prepared_scene(struct futhark_context *ctx, struct futhark_opaque_prepared_scene *obj) {
  FUT_LOCK(ctx);
  if (!obj) return 0;
  if (ctx && ctx->rt) rt_prepared_free(ctx->rt, obj->p);
  delete obj;
  return 0;
}
extern "C" int futhark_free_opaque_scene(struct futhark_context *ctx, struct futhark_opaque_scene *obj) {
  FUT_LOCK(ctx);
  if (!obj) return 0;
  rt_scene_free(ctx ? ctx->rt : nullptr, obj->s);
  delete obj;
  return 0;
}
