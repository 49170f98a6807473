// api_queries.cpp -- the caller queries of the rt_* surface (include/rt_mi355x.h): rays traced, intersected, tested for occlusion, multi-hit,
// sphere casts, ray paths, the proximity, range, box, plane-set and along-ray queries, contact pairs and clusters, visibility matrices, a frame's primary rays.  Checks and launches only: the lane kernels are
// query_kernels.hip, and where an entry runs the pooled family (rt_trace_rays, rt_occluded_rays[_ranged]) its plan, parameters and launch
// are the render policy's (api.cpp, through rt_internal.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/rt_mi355x.h"
#include "query_device.hpp"
#include "rt_internal.hpp"

using rti::fail;
using rti::Plan;

// ------------------------------------------------------------------------------------ caller rays
namespace {
// The checks every caller-ray entry shares; on success p holds the prepared scene's traversal copy and the ray count.
int ray_entry_params(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, rtk::KParams *p) {
  if (!ps) return fail(ctx, "null prepared scene");
  if (ctx->group) return fail(ctx, "caller rays: a multi-device context is not supported (use a context on one device)");
  if (n < 0 || n >= (int64_t(1) << 31)) return fail(ctx, "ray count out of range: 0 <= n < 2^31");
  if (!rays_dev) return fail(ctx, "null rays pointer");
  *p = rtk::KParams{};
  rti::scene_params(ps, p);
  p->rays = rays_dev;
  p->nrays = static_cast<int>(n);
  return 0;
}

// The interval rule of the entries that take one (aabb_hit's NaN argument in lane_core.h -- the last slab test decides -- needs a
// finite interval; its one-test form needs a finite start).
bool ray_interval_ok(float t_min, float t_max) {
  return std::isfinite(t_min) && std::isfinite(t_max) && t_min >= 0.0f && t_min <= t_max && t_max <= rtk::kTMax;
}
// ... and the rule of a scalar distance (a cast's radius, a proximity bound, a margin)
bool distance_ok(float d) { return std::isfinite(d) && d >= 0.0f && d <= rtk::kTMax; }

// What a query entry does between its argument checks and its launch: the prepared scene's lock, the context's device, the thread's last
// error cleared (the launchers read it right behind their launches), and n == 0 answered with `empty` in rt_context_last_launch.
// launch() enqueues, names the launch and returns the entry's code.  The caller holds the context lock.
const char *const kNoRays = "family=none (no rays)", *const kNoPoints = "family=none (no points)";
template <class Launch>
int locked_launch(rt_context *ctx, const rt_prepared *ps, int64_t n, const char *empty, Launch &&launch) {
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  ctx->synced_since_render = false;
  if (n == 0) {
    ctx->last_launch = empty;
    return 0;
  }
  return launch();
}
}  // namespace

extern "C" int rt_trace_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth,
                             float *colour3_dev, int32_t *pixel_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!colour3_dev && !pixel_dev) return fail(ctx, "rt_trace_rays: both outputs are NULL");
  if (max_depth < 0) return fail(ctx, "negative max_depth");
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    if (max_depth == 0) {
      // `while depth < 0`: every ray's colour is the initial (0,0,0)
      if (colour3_dev) RT_HIP(ctx, hipMemsetAsync(colour3_dev, 0, sizeof(float) * 3 * static_cast<size_t>(n), ctx->stream));
      if (pixel_dev) RT_HIP(ctx, hipMemsetAsync(pixel_dev, 0, sizeof(int32_t) * static_cast<size_t>(n), ctx->stream));
      ctx->last_launch = "family=none (memset)";
      return 0;
    }
    p.max_depth = max_depth;
    p.out = pixel_dev;
    p.colour3 = colour3_dev;
    p.nframes = 1;
    // the pooled family's plan; the pixel family beyond its limits (AUTO), or under RT_VARIANT_PIXEL / RT_VARIANT_PERSISTENT
    Plan pl;
    if (int rc = rti::pooled_rays_plan(ctx, ps, n, &pl)) return rc;
    if (pl.variant != RT_VARIANT_POOLED) {
      RT_HIP(ctx, rtk::launch_pixel_rays(p, ctx->stream));
      ctx->last_launch = "family=pixel (rays)";
      return 0;
    }
    if (int rc = rti::pooled_rays_params(ctx, ps, pl, &p)) return rc;
    return rti::launch_pooled_rays(ctx, p, pl, rtk::kRaysColour);
  });
}

// The closest-hit entries past their checks: the lane kernel under every variant, with the scalar interval or (p.ray_tlo_dev set) each
// ray's own.  The caller holds the context lock.
static int intersect_launch(rt_context *ctx, const rt_prepared *ps, int64_t n, const rtk::KParams &p, float t_min, float t_max,
                            int32_t *index_dev, float *hit7_dev) {
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    const bool ranged = p.ray_tlo_dev != nullptr;
    RT_HIP(ctx, ranged ? rtk::launch_intersect_rays_ranged(p, index_dev, hit7_dev, ctx->stream)
                       : rtk::launch_intersect_rays(p, t_min, t_max, index_dev, hit7_dev, ctx->stream));
    ctx->last_launch = ranged ? "family=intersect (per-ray)" : "family=intersect";
    return 0;
  });
}

extern "C" int rt_intersect_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                                 int32_t *index_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!index_dev) return fail(ctx, "rt_intersect_rays: null index pointer");
  if (!ray_interval_ok(t_min, t_max)) return fail(ctx, "rt_intersect_rays: need 0 <= t_min <= t_max <= 1e9, both finite");
  return intersect_launch(ctx, ps, n, p, t_min, t_max, index_dev, hit7_dev);
}

// The per-ray form: the intervals are device data, so they are not checked here -- the kernel answers a ray whose interval fails the rule
// above (NaN included) as a miss (lane_core.h: interval_ok).
extern "C" int rt_intersect_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *t_min_dev,
                                        const float *t_max_dev, int32_t *index_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!index_dev) return fail(ctx, "rt_intersect_rays_ranged: null index pointer");
  if (!t_min_dev || !t_max_dev) return fail(ctx, "rt_intersect_rays_ranged: null t_min or t_max pointer");
  p.ray_tlo_dev = t_min_dev;
  p.ray_thi_dev = t_max_dev;
  return intersect_launch(ctx, ps, n, p, 0.0f, 0.0f, index_dev, hit7_dev);
}

// The occlusion entries past their checks (p.occluded and the interval -- scalar, or per-ray with p.ray_tlo_dev -- are set): the pooled family's
// any-hit loop under RT_VARIANT_POOLED; the lane kernel under RT_VARIANT_PIXEL / RT_VARIANT_PERSISTENT, and beyond the pooled family's limits.
// AUTO, scalar interval: the pooled loop only where it was measured faster: the whole scene staged in LDS, and rays rather
// than segments (t_max > 1; a shadow ray's (eps, 1) is a segment) -- elsewhere the lane kernel.
// AUTO, per-ray intervals: the host cannot see the rays' t_max, so the scalar rule's t_max > 1 clause cannot be asked.  Measured (DESIGN.md
// 3.5c), the pooled loop won only long random rays on a scene staged in LDS (1.3x) and lost normalised shadow rays on the same scene (1.8x):
// AUTO takes the lane kernel.
static int occluded_launch(rt_context *ctx, const rt_prepared *ps, int64_t n, rtk::KParams &p) {
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    const bool ranged = p.ray_tlo_dev != nullptr;
    Plan pl;
    if (int rc = rti::pooled_rays_plan(ctx, ps, n, &pl)) return rc;
    if (ctx->variant == RT_VARIANT_AUTO &&
        (ranged || (pl.variant == RT_VARIANT_POOLED &&
                    !(pl.lds_nodes == static_cast<int>(ps->n - 1) && pl.lds_sph == static_cast<int>(ps->n) && p.ray_thi > 1.0f))))
      pl.variant = RT_VARIANT_PIXEL;
    if (pl.variant != RT_VARIANT_POOLED) {
      RT_HIP(ctx, ranged ? rtk::launch_occluded_rays_ranged(p, ctx->stream) : rtk::launch_occluded_rays(p, ctx->stream));
      ctx->last_launch = ranged ? "family=occluded (per-ray)" : "family=occluded";
      return 0;
    }
    if (int rc = rti::pooled_rays_params(ctx, ps, pl, &p)) return rc;
    return rti::launch_pooled_rays(ctx, p, pl, rtk::kRaysAny);
  });
}

extern "C" int rt_occluded_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                                uint8_t *occluded_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!occluded_dev) return fail(ctx, "rt_occluded_rays: null output pointer");
  if (!ray_interval_ok(t_min, t_max)) return fail(ctx, "rt_occluded_rays: need 0 <= t_min <= t_max <= 1e9, both finite");
  p.occluded = occluded_dev;
  p.ray_tlo = t_min;
  p.ray_thi = t_max;
  return occluded_launch(ctx, ps, n, p);
}

extern "C" int rt_occluded_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *t_min_dev,
                                       const float *t_max_dev, uint8_t *occluded_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!occluded_dev) return fail(ctx, "rt_occluded_rays_ranged: null output pointer");
  if (!t_min_dev || !t_max_dev) return fail(ctx, "rt_occluded_rays_ranged: null t_min or t_max pointer");
  p.occluded = occluded_dev;
  p.ray_tlo_dev = t_min_dev;
  p.ray_thi_dev = t_max_dev;
  return occluded_launch(ctx, ps, n, p);
}

// The multi-hit entries' checks past ray_entry_params and their launch: the lane kernel under every variant, k crossings per ray.  The caller
// holds the context lock and has set p's interval (scalar, or per-ray).
static int multi_hit_launch(rt_context *ctx, const rt_prepared *ps, int64_t n, rtk::KParams &p, int32_t k, int32_t *count_dev,
                            int32_t *index_dev, uint8_t *root_dev, float *hit7_dev, bool ranged) {
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    RT_HIP(ctx, rtk::launch_multi_hit_rays(p, k, count_dev, index_dev, root_dev, hit7_dev, ctx->stream));
    ctx->last_launch = "family=multi-hit k=" + std::to_string(k) + (ranged ? " (per-ray)" : "");
    return 0;
  });
}

extern "C" int rt_multi_hit_rays(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max, int32_t k,
                                 int32_t *count_dev, int32_t *index_dev, uint8_t *root_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!count_dev && !index_dev && !root_dev && !hit7_dev) return fail(ctx, "rt_multi_hit_rays: all four outputs are NULL");
  if (k < 1 || k > rtk::kMultiHitMaxK) return fail(ctx, "rt_multi_hit_rays: need 1 <= k <= 32");
  if (!ray_interval_ok(t_min, t_max)) return fail(ctx, "rt_multi_hit_rays: need 0 <= t_min <= t_max <= 1e9, both finite");
  p.ray_tlo = t_min;
  p.ray_thi = t_max;
  return multi_hit_launch(ctx, ps, n, p, k, count_dev, index_dev, root_dev, hit7_dev, false);
}

// The per-ray form: as rt_intersect_rays_ranged, a ray whose interval fails the rule is a miss in the kernel (count 0, every slot padded).
extern "C" int rt_multi_hit_rays_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *t_min_dev,
                                        const float *t_max_dev, int32_t k, int32_t *count_dev, int32_t *index_dev, uint8_t *root_dev,
                                        float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!count_dev && !index_dev && !root_dev && !hit7_dev) return fail(ctx, "rt_multi_hit_rays_ranged: all four outputs are NULL");
  if (k < 1 || k > rtk::kMultiHitMaxK) return fail(ctx, "rt_multi_hit_rays_ranged: need 1 <= k <= 32");
  if (!t_min_dev || !t_max_dev) return fail(ctx, "rt_multi_hit_rays_ranged: null t_min or t_max pointer");
  p.ray_tlo_dev = t_min_dev;
  p.ray_thi_dev = t_max_dev;
  return multi_hit_launch(ctx, ps, n, p, k, count_dev, index_dev, root_dev, hit7_dev, true);
}

// The sweep entries' checks past ray_entry_params and their launch: the lane kernel under every variant, k contacts per query.  The caller holds
// the context lock and has set p's interval (scalar, or per-query next to radius_dev).
static int sweep_launch(rt_context *ctx, const rt_prepared *ps, int64_t n, rtk::KParams &p, const float *radius_dev, float radius,
                        const int32_t *exclude_dev, int32_t k, int32_t *count_dev, int32_t *index_dev, uint8_t *start_dev, float *hit7_dev) {
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    RT_HIP(ctx, rtk::launch_sweep_spheres(p, radius_dev, radius, exclude_dev, k, count_dev, index_dev, start_dev, hit7_dev, ctx->stream));
    ctx->last_launch = "family=sweep k=" + std::to_string(k) + (radius_dev ? " (per-query)" : "") + (exclude_dev ? " exclude" : "");
    return 0;
  });
}

extern "C" int rt_sweep_spheres(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius, float t_min, float t_max,
                                int32_t k, int32_t *count_dev, int32_t *index_dev, uint8_t *start_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!count_dev && !index_dev && !start_dev && !hit7_dev) return fail(ctx, "rt_sweep_spheres: all four outputs are NULL");
  if (k < 1 || k > rtk::kSweepMaxK) return fail(ctx, "rt_sweep_spheres: need 1 <= k <= 32");
  if (!ray_interval_ok(t_min, t_max)) return fail(ctx, "rt_sweep_spheres: need 0 <= t_min <= t_max <= 1e9, both finite");
  if (!distance_ok(radius)) return fail(ctx, "rt_sweep_spheres: need 0 <= radius <= 1e9, finite");
  p.ray_tlo = t_min;
  p.ray_thi = t_max;
  return sweep_launch(ctx, ps, n, p, nullptr, radius, nullptr, k, count_dev, index_dev, start_dev, hit7_dev);
}

// The per-query form: a query whose interval or radius fails its rule is a miss in the kernel (count 0, every slot padded).
extern "C" int rt_sweep_spheres_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, const float *radius_dev,
                                       const float *t_min_dev, const float *t_max_dev, const int32_t *exclude_dev, int32_t k,
                                       int32_t *count_dev, int32_t *index_dev, uint8_t *start_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!count_dev && !index_dev && !start_dev && !hit7_dev) return fail(ctx, "rt_sweep_spheres_ranged: all four outputs are NULL");
  if (k < 1 || k > rtk::kSweepMaxK) return fail(ctx, "rt_sweep_spheres_ranged: need 1 <= k <= 32");
  if (!radius_dev || !t_min_dev || !t_max_dev) return fail(ctx, "rt_sweep_spheres_ranged: null radius, t_min or t_max pointer");
  p.ray_tlo_dev = t_min_dev;
  p.ray_thi_dev = t_max_dev;
  return sweep_launch(ctx, ps, n, p, radius_dev, 0.0f, exclude_dev, k, count_dev, index_dev, start_dev, hit7_dev);
}

// a refusal's message behind the entry's name
static int fail_in(rt_context *ctx, const char *what, const char *msg) { return fail(ctx, std::string(what) + msg); }

// The path entries: checks, then the lane kernel under every variant.  rays_per_wave == 0: the auto rule (query_device.hpp:
// paths_auto_per_wave, from the context's CU count).  The caller holds the context lock.
static int paths_entry(rt_context *ctx, const rt_prepared *ps, const char *what, int64_t n, const float *rays_dev, int32_t max_depth, int32_t k,
                       int32_t *count_dev, uint8_t *end_dev, int32_t *index_dev, float *hit7_dev, float *light3_dev, float *last_ray6_dev,
                       float *colour3_dev, int32_t rays_per_wave) {
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!count_dev && !end_dev && !index_dev && !hit7_dev && !light3_dev && !last_ray6_dev && !colour3_dev)
    return fail_in(ctx, what, ": all seven outputs are NULL");
  if (k < 1 || k > rtk::kPathsMaxK) return fail_in(ctx, what, ": need 1 <= k <= 1024");
  if (max_depth < 0) return fail_in(ctx, what, ": negative max_depth");
  if (rays_per_wave != 0 && (rays_per_wave < 64 || rays_per_wave > rtk::kPathsMaxPerWave || rays_per_wave % 64 != 0))
    return fail_in(ctx, what, ": rays_per_wave must be 0 or a multiple of 64 in [64, 4096]");
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    const int per_wave = rays_per_wave != 0 ? rays_per_wave : rtk::paths_auto_per_wave(n, ctx->num_cu);
    RT_HIP(ctx, rtk::launch_trace_paths(p, max_depth, k, per_wave, count_dev, end_dev, index_dev, hit7_dev, light3_dev, last_ray6_dev, colour3_dev,
                                        ctx->stream));
    ctx->last_launch = "family=paths k=" + std::to_string(k) + " depth=" + std::to_string(max_depth) + " rays/wave=" + std::to_string(per_wave);
    return 0;
  });
}

extern "C" int rt_trace_paths(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth, int32_t k,
                              int32_t *count_dev, uint8_t *end_dev, int32_t *index_dev, float *hit7_dev, float *light3_dev,
                              float *last_ray6_dev, float *colour3_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return paths_entry(ctx, ps, "rt_trace_paths", n, rays_dev, max_depth, k, count_dev, end_dev, index_dev, hit7_dev, light3_dev, last_ray6_dev,
                     colour3_dev, 0);
}

extern "C" int rt_trace_paths_shaped(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, int32_t max_depth, int32_t k,
                                     int32_t *count_dev, uint8_t *end_dev, int32_t *index_dev, float *hit7_dev, float *light3_dev,
                                     float *last_ray6_dev, float *colour3_dev, int32_t rays_per_wave) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return paths_entry(ctx, ps, "rt_trace_paths_shaped", n, rays_dev, max_depth, k, count_dev, end_dev, index_dev, hit7_dev, light3_dev,
                     last_ray6_dev, colour3_dev, rays_per_wave);
}

// The refusals every entry of n points, boxes or queries (`noun`) opens with, `what` being the entry's name in their messages; the checks the
// point entries share on top of them (self: the points are the scene's own centres, *n their number); and past the checks the parameter
// block of n points with exact_depth, the depth from which the walk tests boxes: the boxes
// that contain their subtrees are those of the nodes whose subtree is at most `sweeps` levels tall (the AABB propagation's
// floor(log2 n) + 2 Jacobi sweeps from zero boxes, bvh.fut:44-58), which every node at depth >= height - sweeps is.
static int query_entry_checks(rt_context *ctx, const rt_prepared *ps, const char *what, const char *noun, int64_t n) {
  if (!ps) return fail(ctx, "null prepared scene");
  if (ctx->group) return fail_in(ctx, what, ": a multi-device context is not supported (use a context on one device)");
  if (n < 0 || n >= (int64_t(1) << 31)) return fail(ctx, std::string(what) + ": " + noun + " count out of range: 0 <= n < 2^31");
  return 0;
}
static int point_entry_checks(rt_context *ctx, const rt_prepared *ps, const char *what, bool self, int64_t *n, const float *points3_dev) {
  if (self && ps) *n = ps->n;
  if (int rc = query_entry_checks(ctx, ps, what, "point", *n)) return rc;
  if (!self && !points3_dev) return fail_in(ctx, what, ": null points pointer");
  return 0;
}
static rtk::KParams point_params(const rt_prepared *ps, int64_t n, int *exact_depth) {
  rtk::KParams p{};
  rti::scene_params(ps, &p);
  p.nrays = static_cast<int>(n);
  const int sweeps = static_cast<int>(log2f(static_cast<float>(ps->n))) + 2;
  *exact_depth = std::max(0, ps->height - sweeps);
  return p;
}

// The proximity entries: checks, then the lane kernel under every variant (count_dev NULL: its pruned walk).  max_dist_dev != nullptr: the
// per-point form, whose bounds are device data -- an invalid one makes its point a miss in the kernel (query_core.h: max_dist_ok).
static int nearest_entry(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist, const float *max_dist_dev,
                         bool ranged, int32_t k, int32_t *count_dev, int32_t *index_dev, float *gap_dev) {
  const char *const what = ranged ? "rt_nearest_spheres_ranged" : "rt_nearest_spheres";
  if (int rc = point_entry_checks(ctx, ps, what, false, &n, points3_dev)) return rc;
  if (!count_dev && !index_dev && !gap_dev) return fail_in(ctx, what, ": all three outputs are NULL");
  if (k < 1 || k > rtk::kNearestMaxK) return fail_in(ctx, what, ": need 1 <= k <= 32");
  if (ranged && !max_dist_dev) return fail_in(ctx, what, ": null max_dist pointer");
  if (!ranged && !distance_ok(max_dist)) return fail_in(ctx, what, ": need 0 <= max_dist <= 1e9, finite");
  return locked_launch(ctx, ps, n, kNoPoints, [&] {
    int exact_depth;
    const rtk::KParams p = point_params(ps, n, &exact_depth);
    RT_HIP(ctx, rtk::launch_nearest_spheres(p, points3_dev, ranged ? max_dist_dev : nullptr, max_dist, k, exact_depth, count_dev, index_dev, gap_dev,
                                            ctx->stream));
    ctx->last_launch = "family=nearest k=" + std::to_string(k) + (count_dev ? "" : " pruned") + (ranged ? " (per-point)" : "");
    return 0;
  });
}

extern "C" int rt_nearest_spheres(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist, int32_t k,
                                  int32_t *count_dev, int32_t *index_dev, float *gap_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return nearest_entry(ctx, ps, n, points3_dev, max_dist, nullptr, false, k, count_dev, index_dev, gap_dev);
}

extern "C" int rt_nearest_spheres_ranged(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, const float *max_dist_dev,
                                         int32_t k, int32_t *count_dev, int32_t *index_dev, float *gap_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return nearest_entry(ctx, ps, n, points3_dev, 0.0f, max_dist_dev, true, k, count_dev, index_dev, gap_dev);
}

// The range entries (rt_spheres_within_*, rt_contact_pairs_*): checks, then within_lane under every variant.  self: the contact pairs (the
// points are the scene's own centres, `max_dist` is the margin).  The count pass keeps its int32 counts and the scan's block sums in a buffer
// cached on the context, grown when a call needs more (the steady path allocates nothing).
static int query_scratch(rt_context *ctx, size_t want, char **out) {
  if (want > ctx->within_bytes) {
    if (ctx->within_scratch) {
      RT_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (an earlier count pass may still be reading it)
      RT_HIP(ctx, hipFree(ctx->within_scratch));
      ctx->within_scratch = nullptr;
      ctx->within_bytes = 0;
    }
    const size_t bytes = std::max(want + want / 2, size_t(1) << 20);
    RT_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->within_scratch), bytes));
    ctx->within_bytes = bytes;
  }
  *out = ctx->within_scratch;
  return 0;
}
// The CSR entries (count and fill pass of the range, box, plane-set and along-ray queries) share the refusals of a pass ...
static int csr_pass_checks(rt_context *ctx, const char *what, bool fill, const int64_t *offsets_dev, int64_t capacity, bool outputs) {
  if (!offsets_dev) return fail_in(ctx, what, ": null offsets pointer");
  if (fill && capacity < 0) return fail_in(ctx, what, ": negative capacity");
  if (fill && !outputs) return fail_in(ctx, what, ": every output is NULL");
  return 0;
}
// ... and what lies between an entry's argument checks and its name in rt_context_last_launch: the prepared scene's lock, the
// context's device, the thread's last error cleared, the parameter block of n queries with exact_depth (point_params), and for a count pass
// of n > 0 queries the cached scratch.  count(p, exact_depth, scratch) / fill(p, exact_depth) enqueue and return the entry's code;
// rt_context_last_launch is `family`, the pass and `detail`.  The caller holds the context lock.
template <class Count, class Fill>
static int csr_entry(rt_context *ctx, const rt_prepared *ps, bool is_fill, int64_t n, const char *family, const std::string &detail, Count &&count,
                     Fill &&fill) {
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  int exact_depth;
  rtk::KParams p = point_params(ps, n, &exact_depth);
  char *scratch = nullptr;
  if (!is_fill && n > 0 && query_scratch(ctx, rtk::within_scratch_bytes(n), &scratch) != 0) return 1;
  ctx->synced_since_render = false;
  if (int rc = is_fill ? fill(p, exact_depth) : count(p, exact_depth, scratch)) return rc;
  ctx->last_launch = std::string("family=") + family + (is_fill ? " fill" : " count") + detail;
  return 0;
}
static int within_entry(rt_context *ctx, const rt_prepared *ps, const char *what, bool fill, bool self, int64_t n, const float *points3_dev,
                        float max_dist, const float *max_dist_dev, const int32_t *first_dev, int64_t *offsets_dev, int64_t capacity,
                        int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (int rc = point_entry_checks(ctx, ps, what, self, &n, points3_dev)) return rc;
  if (int rc = csr_pass_checks(ctx, what, fill, offsets_dev, capacity, index_dev || gap_dev || point_dev)) return rc;
  if ((self || !max_dist_dev) && !distance_ok(max_dist))
    return fail_in(ctx, what, self ? ": need 0 <= margin <= 1e9, finite" : ": need 0 <= max_dist <= 1e9, finite");
  const std::string detail = std::string(!self && max_dist_dev ? " (per-point)" : "") + (!self && first_dev ? " first" : "") + (self ? " self" : "");
  return csr_entry(
      ctx, ps, fill, n, "within", detail,
      [&](const rtk::KParams &p, int exact_depth, char *scratch) {
        RT_HIP(ctx, rtk::launch_within_count(p, points3_dev, max_dist_dev, max_dist, first_dev, self, exact_depth, scratch, offsets_dev, ctx->stream));
        return 0;
      },
      [&](const rtk::KParams &p, int exact_depth) {
        RT_HIP(ctx, rtk::launch_within_fill(p, points3_dev, max_dist_dev, max_dist, first_dev, self, exact_depth, offsets_dev, capacity, index_dev,
                                            gap_dev, point_dev, ctx->stream));
        return 0;
      });
}

extern "C" int rt_spheres_within_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                       const float *max_dist_dev, const int32_t *first_dev, int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_entry(ctx, ps, "rt_spheres_within_count", false, false, n, points3_dev, max_dist, max_dist_dev, first_dev, offsets_dev, 0, nullptr,
                      nullptr, nullptr);
}

extern "C" int rt_spheres_within_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                      const float *max_dist_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                                      int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_entry(ctx, ps, "rt_spheres_within_fill", true, false, n, points3_dev, max_dist, max_dist_dev, first_dev,
                      const_cast<int64_t *>(offsets_dev), capacity, index_dev, gap_dev, point_dev);
}

extern "C" int rt_contact_pairs_count(rt_context *ctx, const rt_prepared *ps, float margin, int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_entry(ctx, ps, "rt_contact_pairs_count", false, true, 0, nullptr, margin, nullptr, nullptr, offsets_dev, 0, nullptr, nullptr, nullptr);
}

extern "C" int rt_contact_pairs_fill(rt_context *ctx, const rt_prepared *ps, float margin, const int64_t *offsets_dev, int64_t capacity,
                                     int32_t *pair_dev, float *gap_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_entry(ctx, ps, "rt_contact_pairs_fill", true, true, 0, nullptr, margin, nullptr, nullptr, const_cast<int64_t *>(offsets_dev), capacity,
                      nullptr, gap_dev, pair_dev);
}

// The contact clusters (rt_contact_clusters): the checks of the contact pairs' entries, then the union-find over the same walk
// (query_kernels.hip: launch_contact_clusters).  The dense ids and the count go through the range queries' scan, in the same cached buffer.
// A scene of one sphere has no node: point_params / launch_within_count refuse it, this entry answers it (one cluster) without a walk.
extern "C" int rt_contact_clusters(rt_context *ctx, const rt_prepared *ps, float margin, int32_t *root_dev, int32_t *cluster_dev, int32_t *size_dev,
                                   int64_t *num_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_contact_clusters";
  int64_t n = 0;
  if (int rc = point_entry_checks(ctx, ps, what, true, &n, nullptr)) return rc;
  if (!root_dev) return fail_in(ctx, what, ": null root pointer");
  if (!distance_ok(margin)) return fail_in(ctx, what, ": need 0 <= margin <= 1e9, finite");
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  int exact_depth;
  const rtk::KParams p = point_params(ps, n, &exact_depth);
  char *scratch = nullptr;
  if ((cluster_dev || num_dev) && query_scratch(ctx, rtk::clusters_scratch_bytes(n), &scratch) != 0) return 1;
  ctx->synced_since_render = false;
  RT_HIP(ctx, rtk::launch_contact_clusters(p, margin, exact_depth, scratch, root_dev, cluster_dev, size_dev, num_dev, ctx->stream));
  ctx->last_launch = "family=clusters";
  return 0;
}

// The box entries (rt_spheres_in_boxes_*): the range entries' checks in the boxes' words, then boxes_lane under every variant; the count pass
// shares the range queries' cached scratch.
static int boxes_entry(rt_context *ctx, const rt_prepared *ps, const char *what, bool fill, int64_t n, const float *boxes6_dev, float margin,
                       const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev, int64_t capacity, int32_t *index_dev,
                       float *gap_dev, int32_t *point_dev) {
  if (int rc = query_entry_checks(ctx, ps, what, "box", n)) return rc;
  if (!boxes6_dev) return fail_in(ctx, what, ": null boxes pointer");
  if (int rc = csr_pass_checks(ctx, what, fill, offsets_dev, capacity, index_dev || gap_dev || point_dev)) return rc;
  if (!margin_dev && !distance_ok(margin)) return fail_in(ctx, what, ": need 0 <= margin <= 1e9, finite");
  return csr_entry(
      ctx, ps, fill, n, "boxes", std::string(margin_dev ? " (per-box)" : "") + (first_dev ? " first" : ""),
      [&](const rtk::KParams &p, int exact_depth, char *scratch) {
        RT_HIP(ctx, rtk::launch_boxes_count(p, boxes6_dev, margin_dev, margin, first_dev, exact_depth, scratch, offsets_dev, ctx->stream));
        return 0;
      },
      [&](const rtk::KParams &p, int exact_depth) {
        RT_HIP(ctx, rtk::launch_boxes_fill(p, boxes6_dev, margin_dev, margin, first_dev, exact_depth, offsets_dev, capacity, index_dev, gap_dev,
                                           point_dev, ctx->stream));
        return 0;
      });
}

extern "C" int rt_spheres_in_boxes_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *boxes6_dev, float margin,
                                         const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return boxes_entry(ctx, ps, "rt_spheres_in_boxes_count", false, n, boxes6_dev, margin, margin_dev, first_dev, offsets_dev, 0, nullptr, nullptr,
                     nullptr);
}

extern "C" int rt_spheres_in_boxes_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *boxes6_dev, float margin,
                                        const float *margin_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                                        int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return boxes_entry(ctx, ps, "rt_spheres_in_boxes_fill", true, n, boxes6_dev, margin, margin_dev, first_dev, const_cast<int64_t *>(offsets_dev),
                     capacity, index_dev, gap_dev, point_dev);
}

// The plane-set entries (rt_spheres_in_planes_*): the box entries' checks in the planes' words and the plane count's, then planes_lane under
// every variant; the count pass shares the range queries' cached scratch.
static int planes_entry(rt_context *ctx, const rt_prepared *ps, const char *what, bool fill, int64_t n, const float *planes4_dev, int32_t nplanes,
                        float margin, const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev, int64_t capacity,
                        int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (int rc = query_entry_checks(ctx, ps, what, "query", n)) return rc;
  if (nplanes < 1 || nplanes > rtk::kMaxPlanes) return fail_in(ctx, what, ": plane count out of range: 1 <= nplanes <= 8");
  if (!planes4_dev) return fail_in(ctx, what, ": null planes pointer");
  if (int rc = csr_pass_checks(ctx, what, fill, offsets_dev, capacity, index_dev || gap_dev || point_dev)) return rc;
  if (!margin_dev && !distance_ok(margin)) return fail_in(ctx, what, ": need 0 <= margin <= 1e9, finite");
  return csr_entry(
      ctx, ps, fill, n, "planes", " k=" + std::to_string(nplanes) + (margin_dev ? " (per-query)" : "") + (first_dev ? " first" : ""),
      [&](const rtk::KParams &p, int exact_depth, char *scratch) {
        RT_HIP(ctx, rtk::launch_planes_count(p, planes4_dev, nplanes, margin_dev, margin, first_dev, exact_depth, scratch, offsets_dev, ctx->stream));
        return 0;
      },
      [&](const rtk::KParams &p, int exact_depth) {
        RT_HIP(ctx, rtk::launch_planes_fill(p, planes4_dev, nplanes, margin_dev, margin, first_dev, exact_depth, offsets_dev, capacity, index_dev,
                                            gap_dev, point_dev, ctx->stream));
        return 0;
      });
}

extern "C" int rt_spheres_in_planes_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *planes4_dev, int32_t nplanes, float margin,
                                          const float *margin_dev, const int32_t *first_dev, int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return planes_entry(ctx, ps, "rt_spheres_in_planes_count", false, n, planes4_dev, nplanes, margin, margin_dev, first_dev, offsets_dev, 0, nullptr,
                      nullptr, nullptr);
}

extern "C" int rt_spheres_in_planes_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *planes4_dev, int32_t nplanes, float margin,
                                         const float *margin_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                                         int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return planes_entry(ctx, ps, "rt_spheres_in_planes_fill", true, n, planes4_dev, nplanes, margin, margin_dev, first_dev,
                      const_cast<int64_t *>(offsets_dev), capacity, index_dev, gap_dev, point_dev);
}

// The along-ray entries (rt_spheres_along_rays_*): the range entries' checks in a ray query's words, the scalar interval and radius checked
// where they are used, then along_lane under every variant; the count pass shares the range queries' cached scratch.
static int along_entry(rt_context *ctx, const rt_prepared *ps, const char *what, bool fill, int64_t n, const float *rays_dev, float radius,
                       const float *radius_dev, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev,
                       const int32_t *exclude_dev, const int32_t *first_dev, int64_t *offsets_dev, int64_t capacity, int32_t *index_dev,
                       float *roots_dev, uint8_t *start_dev, int32_t *query_dev) {
  if (int rc = query_entry_checks(ctx, ps, what, "query", n)) return rc;
  if (!rays_dev) return fail_in(ctx, what, ": null rays pointer");
  if (int rc = csr_pass_checks(ctx, what, fill, offsets_dev, capacity, index_dev || roots_dev || start_dev || query_dev)) return rc;
  if ((t_min_dev == nullptr) != (t_max_dev == nullptr)) return fail_in(ctx, what, ": t_min_dev and t_max_dev must both be NULL or both be given");
  if (!t_min_dev && !ray_interval_ok(t_min, t_max)) return fail_in(ctx, what, ": need 0 <= t_min <= t_max <= 1e9, both finite");
  if (!radius_dev && !distance_ok(radius)) return fail_in(ctx, what, ": need 0 <= radius <= 1e9, finite");
  const std::string detail = std::string(radius_dev || t_min_dev ? " (per-query)" : "") + (exclude_dev ? " exclude" : "") + (first_dev ? " first" : "");
  // (the walk of the along-ray queries tests every node: exact_depth is not used)
  return csr_entry(
      ctx, ps, fill, n, "along", detail,
      [&](rtk::KParams &p, int, char *scratch) {
        p.rays = rays_dev;
        RT_HIP(ctx, rtk::launch_along_count(p, radius_dev, radius, t_min_dev, t_max_dev, t_min, t_max, exclude_dev, first_dev, scratch, offsets_dev,
                                            ctx->stream));
        return 0;
      },
      [&](rtk::KParams &p, int) {
        p.rays = rays_dev;
        RT_HIP(ctx, rtk::launch_along_fill(p, radius_dev, radius, t_min_dev, t_max_dev, t_min, t_max, exclude_dev, first_dev, offsets_dev, capacity,
                                           index_dev, roots_dev, start_dev, query_dev, ctx->stream));
        return 0;
      });
}

extern "C" int rt_spheres_along_rays_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius,
                                           const float *radius_dev, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev,
                                           const int32_t *exclude_dev, const int32_t *first_dev, int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return along_entry(ctx, ps, "rt_spheres_along_rays_count", false, n, rays_dev, radius, radius_dev, t_min, t_max, t_min_dev, t_max_dev, exclude_dev,
                     first_dev, offsets_dev, 0, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int rt_spheres_along_rays_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float radius,
                                          const float *radius_dev, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev,
                                          const int32_t *exclude_dev, const int32_t *first_dev, const int64_t *offsets_dev, int64_t capacity,
                                          int32_t *index_dev, float *roots_dev, uint8_t *start_dev, int32_t *query_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return along_entry(ctx, ps, "rt_spheres_along_rays_fill", true, n, rays_dev, radius, radius_dev, t_min, t_max, t_min_dev, t_max_dev, exclude_dev,
                     first_dev, const_cast<int64_t *>(offsets_dev), capacity, index_dev, roots_dev, start_dev, query_dev);
}

// The visibility-matrix entries (rt_visible_pairs[_shaped]): checks, then the pairs kernels under every variant.  words_per_wave == 0: the
// auto rule (query_device.hpp: pairs_auto_words_per_wave, from the context's CU count -- the packed shape for short rows, else a run length);
// a caller's positive value is a run length of the general shape.  The caller holds the context lock.
static int pairs_entry(rt_context *ctx, const rt_prepared *ps, const char *what, int64_t n, const float *points3_dev, int64_t m,
                       const float *targets3_dev, int32_t mode, float t_min, float t_max, uint64_t *visible_dev, int32_t *count_dev,
                       int32_t words_per_wave) {
  if (int rc = query_entry_checks(ctx, ps, what, "point", n)) return rc;
  if (m < 1 || m > rtk::kPairsMaxTargets) return fail_in(ctx, what, ": target count out of range: 1 <= m <= 2^24");
  const int64_t words = (m + 63) / 64;
  if (n * words >= (int64_t(1) << 31)) return fail_in(ctx, what, ": too many words: need n * ((m + 63) / 64) < 2^31");
  if (!points3_dev) return fail_in(ctx, what, ": null points pointer");
  if (!targets3_dev) return fail_in(ctx, what, ": null targets pointer");
  if (!visible_dev && !count_dev) return fail_in(ctx, what, ": both outputs are NULL");
  if (mode != RT_PAIRS_TARGETS && mode != RT_PAIRS_DIRECTIONS) return fail_in(ctx, what, ": mode must be RT_PAIRS_TARGETS or RT_PAIRS_DIRECTIONS");
  if (!ray_interval_ok(t_min, t_max)) return fail_in(ctx, what, ": need 0 <= t_min <= t_max <= 1e9, both finite");
  if (words_per_wave < 0) return fail_in(ctx, what, ": words_per_wave must be 0 (the library's rule) or positive");
  return locked_launch(ctx, ps, n, kNoPoints, [&] {
    rtk::KParams p{};
    rti::scene_params(ps, &p);
    p.nrays = static_cast<int>(n);
    const int per_wave = words_per_wave != 0 ? static_cast<int>(std::min<int64_t>(words_per_wave, words))
                                             : rtk::pairs_auto_words_per_wave(n, m, ctx->num_cu);
    RT_HIP(ctx, rtk::launch_visible_pairs(p, points3_dev, targets3_dev, static_cast<int>(m), mode == RT_PAIRS_DIRECTIONS, per_wave, t_min, t_max,
                                          reinterpret_cast<unsigned long long *>(visible_dev), count_dev, ctx->stream));
    ctx->last_launch = std::string(mode == RT_PAIRS_DIRECTIONS ? "family=pairs directions" : "family=pairs targets") +
                       (visible_dev ? " mask" : "") + (count_dev ? " count" : "") +
                       (words_per_wave != 0 ? " words/wave=" + std::to_string(per_wave) : std::string());
    return 0;
  });
}

extern "C" int rt_visible_pairs(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, int64_t m, const float *targets3_dev,
                                int32_t mode, float t_min, float t_max, uint64_t *visible_dev, int32_t *count_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return pairs_entry(ctx, ps, "rt_visible_pairs", n, points3_dev, m, targets3_dev, mode, t_min, t_max, visible_dev, count_dev, 0);
}

extern "C" int rt_visible_pairs_shaped(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, int64_t m,
                                       const float *targets3_dev, int32_t mode, float t_min, float t_max, uint64_t *visible_dev,
                                       int32_t *count_dev, int32_t words_per_wave) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return pairs_entry(ctx, ps, "rt_visible_pairs_shaped", n, points3_dev, m, targets3_dev, mode, t_min, t_max, visible_dev, count_dev,
                     words_per_wave);
}

// ------------------------------------------------------------------------------------ sphere groups
// The groups hang off the prepared scene (rt_internal.hpp: PreparedGroups) and are brought up to date lazily: rt_prepared_update_spheres
// (api.cpp) knows nothing of them, it only gives the scene a new tree_gen.  Every entry below goes through the scene's home context alone, so
// the derive and every launch that reads its words are ordered by that context's one stream.
namespace {
// the refusals the groups' entries share past their own argument checks
int groups_entry_checks(rt_context *ctx, const rt_prepared *ps, const char *what) {
  if (!ps) return fail(ctx, "null prepared scene");
  if (ctx->group) return fail_in(ctx, what, ": a multi-device context is not supported (use a context on one device)");
  if (ps->home != ctx) return fail_in(ctx, what, ": only through the context that prepared the scene");
  return 0;
}
// ... and of those that need groups: a scene that has none (looked at under its lock)
int groups_present(rt_context *ctx, const rt_prepared *ps, const char *what) {
  if (int rc = groups_entry_checks(ctx, ps, what)) return rc;
  RT_LOCK_PS(ps);
  if (!ps->groups.block) return fail_in(ctx, what, ": the scene has no groups (rt_prepared_set_groups gives it some)");
  return 0;
}
// ps's block with the derived words valid for its current tree: derived on the context's stream if they are another tree's.  The caller holds
// both locks and has set the device.
int groups_ready(rt_context *ctx, const rt_prepared *ps, const char *what, rtk::GroupBlock *b) {
  if (!ps->groups.block) return fail_in(ctx, what, ": the scene has no groups (rt_prepared_set_groups gives it some)");
  *b = rtk::groups_carve(ps->groups.block, ps->n);
  if (ps->groups.derived_gen != ps->tree_gen) {
    RT_HIP(ctx, rtk::launch_groups_derive(*b, ps->ids, ps->nodes, ps->left, ps->right, ps->parent, static_cast<int>(ps->n), ctx->stream));
    ps->groups.derived_gen = ps->tree_gen;
  }
  return 0;
}
int group_args(rt_context *ctx, const rt_prepared *ps, const char *what, uint32_t mask, const uint32_t *mask_dev, rtk::GroupArgs *ga) {
  rtk::GroupBlock b;
  if (int rc = groups_ready(ctx, ps, what, &b)) return rc;
  *ga = rtk::GroupArgs{b.groups, b.trav_groups, mask_dev, mask};
  return 0;
}
std::string masked_suffix(const uint32_t *mask_dev) { return mask_dev ? " masked mask=per-query" : " masked"; }
// the optional per-ray interval of the masked ray entries (the rt_spheres_along_rays_* convention): both pointers or neither; the scalar pair
// is checked only where it is used
int masked_interval(rt_context *ctx, const char *what, float t_min, float t_max, const float *t_min_dev, const float *t_max_dev, rtk::KParams *p) {
  if ((t_min_dev == nullptr) != (t_max_dev == nullptr)) return fail_in(ctx, what, ": t_min_dev and t_max_dev must both be NULL or both be given");
  if (!t_min_dev && !ray_interval_ok(t_min, t_max)) return fail_in(ctx, what, ": need 0 <= t_min <= t_max <= 1e9, both finite");
  p->ray_tlo = t_min;
  p->ray_thi = t_max;
  p->ray_tlo_dev = t_min_dev;
  p->ray_thi_dev = t_max_dev;
  return 0;
}
}  // namespace

extern "C" int rt_prepared_set_groups(rt_context *ctx, rt_prepared *ps, const uint32_t *groups_dev, int64_t n) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_prepared_set_groups";
  if (int rc = groups_entry_checks(ctx, ps, what)) return rc;
  if (groups_dev && n != ps->n) return fail(ctx, std::string(what) + ": n must equal rt_prepared_num_spheres (" + std::to_string(ps->n) + ")");
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  ctx->synced_since_render = false;
  PreparedGroups &g = ps->groups;
  if (!groups_dev) {
    if (g.block) {
      RT_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (an earlier masked launch may still be reading it)
      RT_HIP(ctx, hipFree(g.block));
      g.block = nullptr;
    }
    g.derived_gen = 0;
    return 0;
  }
  if (!g.block) RT_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&g.block), rtk::groups_bytes(ps->n)));
  g.derived_gen = 0;
  rtk::GroupBlock b = rtk::groups_carve(g.block, ps->n);
  RT_HIP(ctx, hipMemcpyAsync(b.caller, groups_dev, static_cast<size_t>(ps->n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  return groups_ready(ctx, ps, what, &b);
}

extern "C" int rt_prepared_get_groups(rt_context *ctx, const rt_prepared *ps, uint32_t *groups_dev, uint32_t *node_groups_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_prepared_get_groups";
  if (int rc = groups_entry_checks(ctx, ps, what)) return rc;
  if (!groups_dev && !node_groups_dev) return fail_in(ctx, what, ": both outputs are NULL");
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  ctx->synced_since_render = false;
  rtk::GroupBlock b;
  if (int rc = groups_ready(ctx, ps, what, &b)) return rc;
  const size_t n = static_cast<size_t>(ps->n);
  if (groups_dev) RT_HIP(ctx, hipMemcpyAsync(groups_dev, b.groups, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  if (node_groups_dev)
    RT_HIP(ctx, hipMemcpyAsync(node_groups_dev, b.node_groups, (n - 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

extern "C" int rt_intersect_rays_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                                        const float *t_min_dev, const float *t_max_dev, uint32_t mask, const uint32_t *mask_dev,
                                        int32_t *index_dev, float *hit7_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_intersect_rays_masked";
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!index_dev) return fail_in(ctx, what, ": null index pointer");
  if (int rc = masked_interval(ctx, what, t_min, t_max, t_min_dev, t_max_dev, &p)) return rc;
  if (int rc = groups_present(ctx, ps, what)) return rc;
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    rtk::GroupArgs ga;
    if (int rc = group_args(ctx, ps, what, mask, mask_dev, &ga)) return rc;
    RT_HIP(ctx, rtk::launch_intersect_rays_masked(p, ga, t_min, t_max, index_dev, hit7_dev, ctx->stream));
    ctx->last_launch = std::string(t_min_dev ? "family=intersect (per-ray)" : "family=intersect") + masked_suffix(mask_dev);
    return 0;
  });
}

// (the lane kernel under every variant: the pooled any-hit loop has no masked instantiation)
extern "C" int rt_occluded_rays_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *rays_dev, float t_min, float t_max,
                                       const float *t_min_dev, const float *t_max_dev, uint32_t mask, const uint32_t *mask_dev,
                                       uint8_t *occluded_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_occluded_rays_masked";
  rtk::KParams p;
  if (int rc = ray_entry_params(ctx, ps, n, rays_dev, &p)) return rc;
  if (!occluded_dev) return fail_in(ctx, what, ": null output pointer");
  if (int rc = masked_interval(ctx, what, t_min, t_max, t_min_dev, t_max_dev, &p)) return rc;
  if (int rc = groups_present(ctx, ps, what)) return rc;
  p.occluded = occluded_dev;
  return locked_launch(ctx, ps, n, kNoRays, [&] {
    rtk::GroupArgs ga;
    if (int rc = group_args(ctx, ps, what, mask, mask_dev, &ga)) return rc;
    RT_HIP(ctx, rtk::launch_occluded_rays_masked(p, ga, ctx->stream));
    ctx->last_launch = std::string(t_min_dev ? "family=occluded (per-ray)" : "family=occluded") + masked_suffix(mask_dev);
    return 0;
  });
}

extern "C" int rt_nearest_spheres_masked(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                         const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, int32_t k, int32_t *count_dev,
                                         int32_t *index_dev, float *gap_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  const char *const what = "rt_nearest_spheres_masked";
  if (int rc = point_entry_checks(ctx, ps, what, false, &n, points3_dev)) return rc;
  if (!count_dev && !index_dev && !gap_dev) return fail_in(ctx, what, ": all three outputs are NULL");
  if (k < 1 || k > rtk::kNearestMaxK) return fail_in(ctx, what, ": need 1 <= k <= 32");
  if (!max_dist_dev && !distance_ok(max_dist)) return fail_in(ctx, what, ": need 0 <= max_dist <= 1e9, finite");
  if (int rc = groups_present(ctx, ps, what)) return rc;
  return locked_launch(ctx, ps, n, kNoPoints, [&] {
    rtk::GroupArgs ga;
    if (int rc = group_args(ctx, ps, what, mask, mask_dev, &ga)) return rc;
    int exact_depth;
    const rtk::KParams p = point_params(ps, n, &exact_depth);
    RT_HIP(ctx, rtk::launch_nearest_spheres_masked(p, ga, points3_dev, max_dist_dev, max_dist, k, exact_depth, count_dev, index_dev, gap_dev,
                                                   ctx->stream));
    ctx->last_launch = "family=nearest k=" + std::to_string(k) + (count_dev ? "" : " pruned") + (max_dist_dev ? " (per-point)" : "") + masked_suffix(mask_dev);
    return 0;
  });
}

static int within_masked_entry(rt_context *ctx, const rt_prepared *ps, const char *what, bool fill, int64_t n, const float *points3_dev,
                               float max_dist, const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, const int32_t *first_dev,
                               int64_t *offsets_dev, int64_t capacity, int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (int rc = point_entry_checks(ctx, ps, what, false, &n, points3_dev)) return rc;
  if (int rc = csr_pass_checks(ctx, what, fill, offsets_dev, capacity, index_dev || gap_dev || point_dev)) return rc;
  if (!max_dist_dev && !distance_ok(max_dist)) return fail_in(ctx, what, ": need 0 <= max_dist <= 1e9, finite");
  if (int rc = groups_present(ctx, ps, what)) return rc;
  const std::string detail = std::string(max_dist_dev ? " (per-point)" : "") + (first_dev ? " first" : "") + masked_suffix(mask_dev);
  rtk::GroupArgs ga{};
  return csr_entry(
      ctx, ps, fill, n, "within", detail,
      [&](const rtk::KParams &p, int exact_depth, char *scratch) {
        if (int rc = group_args(ctx, ps, what, mask, mask_dev, &ga)) return rc;
        RT_HIP(ctx, rtk::launch_within_count_masked(p, ga, points3_dev, max_dist_dev, max_dist, first_dev, exact_depth, scratch, offsets_dev, ctx->stream));
        return 0;
      },
      [&](const rtk::KParams &p, int exact_depth) {
        if (int rc = group_args(ctx, ps, what, mask, mask_dev, &ga)) return rc;
        RT_HIP(ctx, rtk::launch_within_fill_masked(p, ga, points3_dev, max_dist_dev, max_dist, first_dev, exact_depth, offsets_dev, capacity, index_dev,
                                                   gap_dev, point_dev, ctx->stream));
        return 0;
      });
}

extern "C" int rt_spheres_within_masked_count(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                              const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, const int32_t *first_dev,
                                              int64_t *offsets_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_masked_entry(ctx, ps, "rt_spheres_within_masked_count", false, n, points3_dev, max_dist, max_dist_dev, mask, mask_dev, first_dev,
                             offsets_dev, 0, nullptr, nullptr, nullptr);
}

extern "C" int rt_spheres_within_masked_fill(rt_context *ctx, const rt_prepared *ps, int64_t n, const float *points3_dev, float max_dist,
                                             const float *max_dist_dev, uint32_t mask, const uint32_t *mask_dev, const int32_t *first_dev,
                                             const int64_t *offsets_dev, int64_t capacity, int32_t *index_dev, float *gap_dev, int32_t *point_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  return within_masked_entry(ctx, ps, "rt_spheres_within_masked_fill", true, n, points3_dev, max_dist, max_dist_dev, mask, mask_dev, first_dev,
                             const_cast<int64_t *>(offsets_dev), capacity, index_dev, gap_dev, point_dev);
}

extern "C" int rt_prepared_get_sphere_ids(rt_context *ctx, const rt_prepared *ps, int32_t *ids_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  if (!ps || !ids_dev) return fail(ctx, "null argument");
  RT_LOCK_PS(ps);
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  ctx->synced_since_render = false;
  RT_HIP(ctx, hipMemcpyAsync(ids_dev, ps->ids, static_cast<size_t>(ps->n) * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

extern "C" int rt_camera_rays(rt_context *ctx, const rt_prepared *ps, int64_t h, int64_t w, const float cam12[12], float *rays_dev) {
  if (!ctx) return 1;
  RT_LOCK(ctx);
  if (!ps) return fail(ctx, "null prepared scene");
  if (ctx->group) return fail(ctx, "caller rays: a multi-device context is not supported (use a context on one device)");
  if (!rays_dev) return fail(ctx, "null rays pointer");
  if (h <= 0 || w <= 0 || h > (1 << 20) || w > (1 << 20) || h * w > (int64_t(1) << 30)) return fail(ctx, "image size out of range");
  rtk::Cam cam;
  std::memcpy(&cam, cam12 ? static_cast<const void *>(cam12) : static_cast<const void *>(&ps->cam), sizeof(cam));
  RT_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipGetLastError();
  ctx->synced_since_render = false;
  RT_HIP(ctx, rtk::launch_camera_rays(cam, static_cast<int>(h), static_cast<int>(w), rays_dev, ctx->stream));
  ctx->last_launch = "family=camera-rays";
  return 0;
}
