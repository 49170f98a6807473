// query_kernels.hip -- the lane kernels of the caller queries, one lane per ray or point: closest hit (rt_intersect_rays), occlusion
// (rt_occluded_rays), multi-hit, sphere casts, ray paths, the nearest spheres, the range queries / contact pairs with their scan, the contact clusters, the box, plane-set and along-ray queries, the visibility matrices, and the primary
// rays of a frame (rt_camera_rays).  The render path -- pixel_kernel, persistent_kernel, pooled_kernel and their RAYS modes -- is
// render_kernels.hip; nothing here is launched by a render entry.  Build: as render_kernels.hip (-ffp-contract=off, bit-exact fp32).
#include <hip/hip_runtime.h>

#include "query_core.h"
#include "query_device.hpp"

namespace rtk {

// Sphere groups: a lane's view of GroupArgs (query_device.hpp), what a masked lane kernel takes on top of its unmasked twin's
// arguments.  MASKED false: every test is the constant true and the lanes compile to what they were.  MASKED: both arrays are read
// through buffer resources of the scene's sizes, 4 bytes per test (an index outside the scene reads 0: unseen).
template <bool MASKED>
struct GroupView {
  __device__ __forceinline__ GroupView(const KParams &, const GroupArgs &, int) {}
  __device__ __forceinline__ bool start() const { return true; }
  __device__ __forceinline__ bool node(int) const { return true; }
  __device__ __forceinline__ bool leaf(int) const { return true; }
};
template <>
struct GroupView<true> {
  const __amdgpu_buffer_rsrc_t rs_g, rs_ng;
  const uint32_t m;
  __device__ __forceinline__ GroupView(const KParams &p, const GroupArgs &ga, int i)
      : rs_g(make_rsrc(ga.groups, (unsigned)p.n_sph * 4u)), rs_ng(make_rsrc(ga.node_groups, (unsigned)p.n_nodes * 4u)),
        m(ga.mask_dev != nullptr ? ga.mask_dev[i] : ga.mask) {}
  // may a seen sphere lie below inner node v: asked where v would be pushed, so an unseen subtree costs neither its record nor a stack slot
  __device__ __forceinline__ bool node(int v) const { return group_seen((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_ng, v * 4, 0, 0), m); }
  // is sphere j seen: asked ahead of its 16-byte load
  __device__ __forceinline__ bool leaf(int j) const { return group_seen((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_g, j * 4, 0, 0), m); }
  // does the walk start at all: mask 0 sees nothing, and the root is a node like the others
  __device__ __forceinline__ bool start() const { return m != 0u && node(0); }
};

// A lane's interval in the lane kernels: the caller's (t_min, t_max), or with RANGED ray i's own -- two coalesced 4-byte loads next to its ray.
// A ray whose own interval fails interval_ok does not start its walk: it is a miss.
template <bool RANGED>
__device__ __forceinline__ bool lane_interval(const KParams &p, int i, float &t_min, float &t_max) {
  if constexpr (!RANGED) return true;
  t_min = p.ray_tlo_dev[i];
  t_max = p.ray_thi_dev[i];
  return interval_ok(t_min, t_max);
}

// objs_hit bvh r t_min t_max (ray.fut:76-86), one lane per ray: the pixel family's stack fold with the caller's interval on every box,
// the spheres folded over (scene_epsilon, best) from best = t_max, then one re-intersection of the winner over (t_min, best + 1).
template <bool RANGED, bool MASKED = false>
__device__ __forceinline__ void intersect_lane(const KParams &p, float t_min, float t_max, int32_t *index, float *hit7,
                                               const GroupArgs &ga = GroupArgs{}) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= p.nrays) return;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const Ray r = load_ray(p.rays, i);
  const bool valid = lane_interval<RANGED>(p, i, t_min, t_max);
  const GroupView<MASKED> gv(p, ga, i);
  float best = t_max;
  int bestj = -1;
  int sp = 0;
  if (valid && gv.start()) stack[sp++][lane] = 0;
  while (sp > 0) {
    const int ni = stack[--sp][lane];
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (!box_hit_interval(r, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, t_min, t_max)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = kids[k];
      if (c < 0) {
        const int j = ~c;
        if (gv.leaf(j)) {
          const float4 s = buf_load16(rs_sph, j * 16);
          closest_update(sphere_root(r, s.x, s.y, s.z, s.w), j, best, bestj);
        }
      } else if (gv.node(c)) {
        stack[sp++][lane] = c;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
      }
    }
  }
  float t = 0.0f, h[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool have = false;
  if (bestj >= 0) {
    const float4 s = p.sph[bestj];
    have = rehit_range(r, t_min, best, s.x, s.y, s.z, s.w, &t);
    if (have) {
      const float inv_rad = p.col[bestj].w;   // 1.0f / radius, the bits of scale (1.0/s.radius) (ray.fut:43)
      h[0] = r.ox + t * r.dx; h[1] = r.oy + t * r.dy; h[2] = r.oz + t * r.dz;   // point_at_param
      h[3] = inv_rad * (h[0] - s.x); h[4] = inv_rad * (h[1] - s.y); h[5] = inv_rad * (h[2] - s.z);
    }
  }
  index[i] = have ? bestj : -1;
  if (hit7 != nullptr) {
    float *const o = hit7 + (size_t)i * 7;
    o[0] = have ? t : 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[1 + k] = h[k];
  }
}
__global__ __launch_bounds__(64) void intersect_kernel(KParams p, float t_min, float t_max, int32_t *index, float *hit7) {
  intersect_lane<false>(p, t_min, t_max, index, hit7);
}
__global__ __launch_bounds__(64) void intersect_ranged_kernel(KParams p, int32_t *index, float *hit7) {
  intersect_lane<true>(p, 0.0f, 0.0f, index, hit7);
}

hipError_t launch_intersect_rays(const KParams &p, float t_min, float t_max, int32_t *index, float *hit7, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  hipLaunchKernelGGL(intersect_kernel, dim3((unsigned)((p.nrays + 63) / 64)), dim3(64), 0, stream, p, t_min, t_max, index, hit7);
  return hipGetLastError();
}
hipError_t launch_intersect_rays_ranged(const KParams &p, int32_t *index, float *hit7, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (p.ray_tlo_dev == nullptr || p.ray_thi_dev == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(intersect_ranged_kernel, dim3((unsigned)((p.nrays + 63) / 64)), dim3(64), 0, stream, p, index, hit7);
  return hipGetLastError();
}

// rt_occluded_rays, one lane per ray: intersect_kernel's stack fold with the caller's interval on every box and on every sphere
// (sphere_hit_any); the lane leaves the walk at its first accepted sphere -- the fold is an OR, so no order can change the answer.
template <bool RANGED, bool MASKED = false>
__device__ __forceinline__ void occluded_lane(const KParams &p, const GroupArgs &ga = GroupArgs{}) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= p.nrays) return;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const Ray r = load_ray(p.rays, i);
  float t_min = p.ray_tlo, t_max = p.ray_thi;
  const bool valid = lane_interval<RANGED>(p, i, t_min, t_max);
  const GroupView<MASKED> gv(p, ga, i);
  bool hit = false;
  int sp = 0;
  if (valid && gv.start()) stack[sp++][lane] = 0;
  while (sp > 0 && !hit) {
    const int ni = stack[--sp][lane];
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (!box_hit_interval(r, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, t_min, t_max)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = kids[k];
      if (c < 0) {
        if (gv.leaf(~c)) {
          const float4 s = buf_load16(rs_sph, ~c * 16);
          hit = hit || sphere_hit_any(r, t_min, t_max, s.x, s.y, s.z, s.w);
        }
      } else if (gv.node(c)) {
        stack[sp++][lane] = c;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
      }
    }
  }
  p.occluded[i] = hit ? 1 : 0;
}
__global__ __launch_bounds__(64) void occluded_kernel(KParams p) { occluded_lane<false>(p); }
__global__ __launch_bounds__(64) void occluded_ranged_kernel(KParams p) { occluded_lane<true>(p); }

hipError_t launch_occluded_rays(const KParams &p, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (p.occluded == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(occluded_kernel, dim3((unsigned)((p.nrays + 63) / 64)), dim3(64), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_occluded_rays_ranged(const KParams &p, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (p.occluded == nullptr || p.ray_tlo_dev == nullptr || p.ray_thi_dev == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(occluded_ranged_kernel, dim3((unsigned)((p.nrays + 63) / 64)), dim3(64), 0, stream, p);
  return hipGetLastError();
}

// rt_multi_hit_rays: a lane's crossings -- (t, j, root) for every root of every visited sphere strictly inside (t_min, t_max) -- kept as
// one 64-bit key each, bits(t) << 32 | j << 1 | (root - 1).  t > t_min >= 0 (-0.0 included) and t < t_max <= 1e9, so t is positive and
// finite and its bits order as t does; j < 2^26 (rt_scene's sphere limit; any j < 2^31 would do) fills the low word below bit 27 next to
// the root bit.  The key carries no ray index, so the order is (t, j, root) for every ray count.  An empty slot is ~0: no crossing has a
// high word of 0xffffffff.
__device__ __forceinline__ unsigned long long crossing_key(float t, int j, int root2) {
  return ((unsigned long long)__float_as_uint(t) << 32) | ((unsigned)j << 1) | (unsigned)root2;
}
// Insert x into the sorted list of the CAP smallest keys: x is carried down the list, each slot keeping the smaller of the two.  Every index
// is a compile-time constant after unrolling, so the list stays in VGPRs (a runtime index would put it in scratch).  Skipped when x is
// not below the last slot.
template <int CAP>
__device__ __forceinline__ void crossing_insert(unsigned long long (&list)[CAP], unsigned long long x) {
  if (!(x < list[CAP - 1])) return;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    const unsigned long long y = list[s];
    list[s] = x < y ? x : y;
    x = x < y ? y : x;
  }
}

// One lane per ray: occluded_lane's walk (box_hit_interval over the lane's interval on every box) without its early exit and without
// culling.  At each leaf both roots are computed once (sphere_roots); each one inside the interval is counted and inserted into the
// lane's list of the CAP smallest crossings (k <= CAP of them are written).  At write-out slot s < min(count, k) gets j, its root and
// {t, p.xyz, normal.xyz} with intersect_lane's arithmetic; slots up to k are padded with -1, 0 and seven zeros.  Outputs are at
// 64-bit offsets (n * k * 7 passes 2^31); any of them may be nullptr.
template <bool RANGED, int CAP>
__device__ __forceinline__ void multi_hit_lane(const KParams &p, int k, int32_t *count, int32_t *index, uint8_t *root, float *hit7) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= p.nrays) return;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const Ray r = load_ray(p.rays, i);
  float t_min = p.ray_tlo, t_max = p.ray_thi;
  const bool valid = lane_interval<RANGED>(p, i, t_min, t_max);
  unsigned long long list[CAP];
#pragma unroll
  for (int s = 0; s < CAP; ++s) list[s] = ~0ull;
  int cnt = 0;
  int sp = 0;
  if (valid) stack[sp++][lane] = 0;
  while (sp > 0) {
    const int ni = stack[--sp][lane];
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (!box_hit_interval(r, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, t_min, t_max)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int c = kids[c2];
      if (c < 0) {
        const int j = ~c;
        const float4 s = buf_load16(rs_sph, j * 16);
        float t1, t2;
        if (sphere_roots(r, s.x, s.y, s.z, s.w, &t1, &t2)) {
          const bool in1 = (t1 < t_max) && (t1 > t_min), in2 = (t2 < t_max) && (t2 > t_min);   // (sphere_hit_any's tests)
          cnt += (in1 ? 1 : 0) + (in2 ? 1 : 0);
          if (in1) crossing_insert<CAP>(list, crossing_key(t1, j, 0));
          if (in2) crossing_insert<CAP>(list, crossing_key(t2, j, 1));
        }
      } else {
        stack[sp++][lane] = c;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
      }
    }
  }
  if (count != nullptr) count[i] = cnt;
  const size_t base = (size_t)i * (size_t)k;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    if (s < k) {
      const bool have = s < cnt;
      const int j = have ? (int)((unsigned)list[s] >> 1) : -1;
      if (index != nullptr) index[base + s] = j;
      if (root != nullptr) root[base + s] = have ? (uint8_t)(((unsigned)list[s] & 1u) + 1u) : (uint8_t)0;
      if (hit7 != nullptr) {
        float h[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
          const float t = __uint_as_float((unsigned)(list[s] >> 32));
          const float4 ce = p.sph[j];
          const float inv_rad = p.col[j].w;   // 1.0f / radius, as intersect_lane
          h[0] = t;
          h[1] = r.ox + t * r.dx; h[2] = r.oy + t * r.dy; h[3] = r.oz + t * r.dz;   // point_at_param
          h[4] = inv_rad * (h[1] - ce.x); h[5] = inv_rad * (h[2] - ce.y); h[6] = inv_rad * (h[3] - ce.z);
        }
        float *const o = hit7 + (base + s) * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) o[q] = h[q];
      }
    }
  }
}
template <bool RANGED, int CAP>
__global__ __launch_bounds__(64) void multi_hit_kernel(KParams p, int k, int32_t *count, int32_t *index, uint8_t *root, float *hit7) {
  multi_hit_lane<RANGED, CAP>(p, k, count, index, root, hit7);
}

template <bool RANGED>
static hipError_t launch_multi_hit_cap(const KParams &p, int k, int32_t *count, int32_t *index, uint8_t *root, float *hit7, hipStream_t stream) {
  const dim3 grid((unsigned)((p.nrays + 63) / 64)), block(64);
  if (k <= 4) hipLaunchKernelGGL((multi_hit_kernel<RANGED, 4>), grid, block, 0, stream, p, k, count, index, root, hit7);
  else if (k <= 8) hipLaunchKernelGGL((multi_hit_kernel<RANGED, 8>), grid, block, 0, stream, p, k, count, index, root, hit7);
  else if (k <= 16) hipLaunchKernelGGL((multi_hit_kernel<RANGED, 16>), grid, block, 0, stream, p, k, count, index, root, hit7);
  else hipLaunchKernelGGL((multi_hit_kernel<RANGED, 32>), grid, block, 0, stream, p, k, count, index, root, hit7);
  return hipGetLastError();
}

hipError_t launch_multi_hit_rays(const KParams &p, int k, int32_t *count, int32_t *index, uint8_t *root, float *hit7, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (k < 1 || k > kMultiHitMaxK) return hipErrorInvalidValue;
  if (count == nullptr && index == nullptr && root == nullptr && hit7 == nullptr) return hipErrorInvalidValue;
  if ((p.ray_tlo_dev == nullptr) != (p.ray_thi_dev == nullptr)) return hipErrorInvalidValue;
  return p.ray_tlo_dev != nullptr ? launch_multi_hit_cap<true>(p, k, count, index, root, hit7, stream)
                                  : launch_multi_hit_cap<false>(p, k, count, index, root, hit7, stream);
}

// rt_sweep_spheres: one lane per query -- a sphere of radius rq whose centre moves along the lane's ray.  multi_hit_lane's walk with every
// node's box widened by rq per component (fl(lo - rq), fl(hi + rq): six additions per box test, rq being the query's own) and, at a
// leaf, sweep_contact (query_core.h) in place of the two roots: a sphere gives at most one contact, counted and inserted into the same
// sorted list as the key bits(tau) << 32 | j << 1 | start.  tau is t1 inside (t_min, t_max), or t_min + 0.0f for an overlap at the start:
// never negative, finite, so its bits order as it does, and the key order is (tau, j).  The interval is never narrowed by the contacts
// found: the visited leaves are part of the contract.  RANGED: the query's own radius and interval (a failing interval_ok or max_dist_ok
// is a miss, its walk does not start).  exclude != nullptr: sphere exclude[i] is skipped at the leaf, one compare (a value no leaf has
// excludes nothing).  At write-out slot s < min(count, k) gets j, start and {tau, p, (1.0f / R) * (p - centre)} with R = radius_j + rq;
// slots up to k are padded with -1, 0 and seven zeros.  64-bit output offsets; any output may be nullptr.
template <bool RANGED, int CAP>
__device__ __forceinline__ void sweep_lane(const KParams &p, const float *radius_dev, float rq, const int32_t *exclude, int k, int32_t *count,
                                           int32_t *index, uint8_t *start, float *hit7) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= p.nrays) return;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const Ray r = load_ray(p.rays, i);
  float t_min = p.ray_tlo, t_max = p.ray_thi;
  bool valid = lane_interval<RANGED>(p, i, t_min, t_max);
  if constexpr (RANGED) {
    rq = radius_dev[i] + 0.0f;   // (-0.0 -> +0.0)
    valid = valid && max_dist_ok(rq);
  }
  const int skip = exclude != nullptr ? exclude[i] : -1;
  unsigned long long list[CAP];
#pragma unroll
  for (int s = 0; s < CAP; ++s) list[s] = ~0ull;
  int cnt = 0;
  int sp = 0;
  if (valid) stack[sp++][lane] = 0;
  while (sp > 0) {
    const int ni = stack[--sp][lane];
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (!box_hit_interval(r, lo.x - rq, lo.y - rq, lo.z - rq, hi.x + rq, hi.y + rq, hi.z + rq, t_min, t_max)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int c = kids[c2];
      if (c < 0) {
        const int j = ~c;
        if (j != skip) {
          const float4 s = buf_load16(rs_sph, j * 16);
          float tau;
          const int what = sweep_contact(r, s.x, s.y, s.z, s.w, rq, t_min, t_max, &tau);
          if (what != kSweepNone) {
            cnt += 1;
            crossing_insert<CAP>(list, crossing_key(tau, j, what == kSweepStart ? 1 : 0));
          }
        }
      } else {
        stack[sp++][lane] = c;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
      }
    }
  }
  if (count != nullptr) count[i] = cnt;
  const size_t base = (size_t)i * (size_t)k;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    if (s < k) {
      const bool have = s < cnt;
      const int j = have ? (int)((unsigned)list[s] >> 1) : -1;
      if (index != nullptr) index[base + s] = j;
      if (start != nullptr) start[base + s] = have ? (uint8_t)((unsigned)list[s] & 1u) : (uint8_t)0;
      if (hit7 != nullptr) {
        float h[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
          const float tau = __uint_as_float((unsigned)(list[s] >> 32));
          const float4 ce = p.sph[j];
          const float inv_rad = 1.0f / (ce.w + rq);   // 1 / R: the one division of the slot
          h[0] = tau;
          h[1] = r.ox + tau * r.dx; h[2] = r.oy + tau * r.dy; h[3] = r.oz + tau * r.dz;   // point_at_param: the moving centre at contact
          h[4] = inv_rad * (h[1] - ce.x); h[5] = inv_rad * (h[2] - ce.y); h[6] = inv_rad * (h[3] - ce.z);
        }
        float *const o = hit7 + (base + s) * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) o[q] = h[q];
      }
    }
  }
}
template <bool RANGED, int CAP>
__global__ __launch_bounds__(64) void sweep_kernel(KParams p, const float *radius_dev, float rq, const int32_t *exclude, int k, int32_t *count,
                                                   int32_t *index, uint8_t *start, float *hit7) {
  sweep_lane<RANGED, CAP>(p, radius_dev, rq, exclude, k, count, index, start, hit7);
}

template <bool RANGED>
static hipError_t launch_sweep_cap(const KParams &p, const float *radius_dev, float rq, const int32_t *exclude, int k, int32_t *count,
                                   int32_t *index, uint8_t *start, float *hit7, hipStream_t stream) {
  const dim3 grid((unsigned)((p.nrays + 63) / 64)), block(64);
  if (k <= 4) hipLaunchKernelGGL((sweep_kernel<RANGED, 4>), grid, block, 0, stream, p, radius_dev, rq, exclude, k, count, index, start, hit7);
  else if (k <= 8) hipLaunchKernelGGL((sweep_kernel<RANGED, 8>), grid, block, 0, stream, p, radius_dev, rq, exclude, k, count, index, start, hit7);
  else if (k <= 16) hipLaunchKernelGGL((sweep_kernel<RANGED, 16>), grid, block, 0, stream, p, radius_dev, rq, exclude, k, count, index, start, hit7);
  else hipLaunchKernelGGL((sweep_kernel<RANGED, 32>), grid, block, 0, stream, p, radius_dev, rq, exclude, k, count, index, start, hit7);
  return hipGetLastError();
}

hipError_t launch_sweep_spheres(const KParams &p, const float *radius_dev, float radius, const int32_t *exclude, int k, int32_t *count,
                                int32_t *index, uint8_t *start, float *hit7, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (k < 1 || k > kSweepMaxK) return hipErrorInvalidValue;
  if (count == nullptr && index == nullptr && start == nullptr && hit7 == nullptr) return hipErrorInvalidValue;
  const bool ranged = radius_dev != nullptr;
  if (ranged != (p.ray_tlo_dev != nullptr) || ranged != (p.ray_thi_dev != nullptr)) return hipErrorInvalidValue;
  if (!ranged && !max_dist_ok(radius)) return hipErrorInvalidValue;
  radius += 0.0f;   // (-0.0 -> +0.0)
  return ranged ? launch_sweep_cap<true>(p, radius_dev, 0.0f, exclude, k, count, index, start, hit7, stream)
                : launch_sweep_cap<false>(p, nullptr, radius, exclude, k, count, index, start, hit7, stream);
}

// rt_nearest_spheres: one lane per point.  The walk of multi_hit_lane with the box test replaced by box_may_hold (query_core.h: the
// point-to-box distance against the threshold plus a proven slack) and the crossing list by the same sorted list of CAP 64-bit keys,
// gap_key(gap, j): every sphere with gap <= max_dist is counted and inserted.  A box is tested only at depth >= exact_depth: the reference's
// AABB propagation runs floor(log2 n) + 2 sweeps from zero boxes (bvh.fut:44-58), so in a taller tree the boxes of the nodes nearer the root
// than height - sweeps levels need not contain their subtrees -- the walk descends through them untested.  A stack entry is the node and its
// depth (capped at 63) in bits 26..31 (node < 2^26).
// PRUNED (no count output): once the list holds k keys the threshold is min(max_dist, the k-th gap) -- read with an unrolled select, a
// runtime index would put the list in scratch -- and the children of a node are pushed farther first, so the nearer one is walked first (one
// extra 32-byte read per inner child).  Neither changes the first k keys: a skipped box holds only spheres whose gap exceeds the threshold.
// Outputs at 64-bit offsets; any may be nullptr.
template <int CAP>
__device__ __forceinline__ float kth_gap(const unsigned long long (&list)[CAP], int k) {
  unsigned long long x = ~0ull;
#pragma unroll
  for (int s = 0; s < CAP; ++s) x = s == k - 1 ? list[s] : x;
  return x == ~0ull ? kNoHit : gap_of_key(x);
}
__device__ __forceinline__ int nearest_stack_entry(int node, int depth) { return (int)((unsigned)node | ((unsigned)(depth < 63 ? depth : 63) << 26)); }

template <bool RANGED, bool PRUNED, int CAP, bool MASKED = false>
__device__ __forceinline__ void nearest_lane(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, int k, int exact_depth,
                                             int32_t *count, int32_t *index, float *gap, const GroupArgs &ga = GroupArgs{}) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= p.nrays) return;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const float px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
  if constexpr (RANGED) max_dist = max_dist_dev[i] + 0.0f;   // (-0.0 -> +0.0)
  const bool valid = point_ok(px, py, pz) && (!RANGED || max_dist_ok(max_dist));
  const float pmag = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
  const GroupView<MASKED> gv(p, ga, i);
  unsigned long long list[CAP];
#pragma unroll
  for (int s = 0; s < CAP; ++s) list[s] = ~0ull;
  int cnt = 0;
  float T = max_dist;
  int sp = 0;
  if (valid && gv.start()) stack[sp++][lane] = nearest_stack_entry(0, 0);
  while (sp > 0) {
    const unsigned e = (unsigned)stack[--sp][lane];
    const int ni = (int)(e & 0x3ffffffu), depth = (int)(e >> 26);
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (depth >= exact_depth && !box_may_hold(px, py, pz, pmag, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, T)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int c = kids[c2];
      if (c < 0 && gv.leaf(~c)) {
        const int j = ~c;
        const float4 s = buf_load16(rs_sph, j * 16);
        const float g = point_gap(px, py, pz, s.x, s.y, s.z, s.w);
        if (g <= max_dist) {
          ++cnt;
          crossing_insert<CAP>(list, gap_key(g, j));
          if constexpr (PRUNED) T = fminf(max_dist, kth_gap<CAP>(list, k));
        }
      }
    }
    if constexpr (PRUNED) {
      // the inner children, farther first; one that already fails the test is not pushed
      float b[2] = {0.0f, 0.0f};
      bool push[2] = {false, false};
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const int c = kids[c2];
        if (c >= 0 && gv.node(c)) {
          const float4 clo = buf_load16(rs_nodes, c * 32), chi = buf_load16(rs_nodes, c * 32 + 16);
          push[c2] = depth + 1 < exact_depth || box_may_hold(px, py, pz, pmag, clo.x, clo.y, clo.z, chi.x, chi.y, chi.z, T);
          b[c2] = box_gap_bound(px, py, pz, clo.x, clo.y, clo.z, chi.x, chi.y, chi.z);
        }
      }
      const int first = b[0] >= b[1] ? 0 : 1;   // (the farther one goes below the nearer one)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c2 = q == 0 ? first : 1 - first;
        if (push[c2]) stack[sp++][lane] = nearest_stack_entry(kids[c2], depth + 1);   // (one pending sibling per level: sp <= height + 1 <= kStackPixel)
      }
    } else {
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
        if (kids[c2] >= 0 && gv.node(kids[c2])) stack[sp++][lane] = nearest_stack_entry(kids[c2], depth + 1);
    }
  }
  if (count != nullptr) count[i] = cnt;
  const size_t base = (size_t)i * (size_t)k;
#pragma unroll
  for (int s = 0; s < CAP; ++s) {
    if (s < k) {
      const bool have = list[s] != ~0ull;
      if (index != nullptr) index[base + s] = have ? (int)(unsigned)list[s] : -1;
      if (gap != nullptr) gap[base + s] = have ? gap_of_key(list[s]) : 0.0f;
    }
  }
}
template <bool RANGED, bool PRUNED, int CAP>
__global__ __launch_bounds__(64) void nearest_kernel(KParams p, const float *pts, const float *max_dist_dev, float max_dist, int k, int exact_depth,
                                                     int32_t *count, int32_t *index, float *gap) {
  nearest_lane<RANGED, PRUNED, CAP>(p, pts, max_dist_dev, max_dist, k, exact_depth, count, index, gap);
}

template <bool RANGED, bool PRUNED>
static hipError_t launch_nearest_cap(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, int k, int exact_depth,
                                     int32_t *count, int32_t *index, float *gap, hipStream_t stream) {
  const dim3 grid((unsigned)((p.nrays + 63) / 64)), block(64);
#define RT_NEAREST(CAP) \
  hipLaunchKernelGGL((nearest_kernel<RANGED, PRUNED, CAP>), grid, block, 0, stream, p, pts, max_dist_dev, max_dist, k, exact_depth, count, index, gap)
  if (k <= 4) RT_NEAREST(4);
  else if (k <= 8) RT_NEAREST(8);
  else if (k <= 16) RT_NEAREST(16);
  else RT_NEAREST(32);
#undef RT_NEAREST
  return hipGetLastError();
}

hipError_t launch_nearest_spheres(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, int k, int exact_depth,
                                  int32_t *count, int32_t *index, float *gap, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (pts == nullptr || k < 1 || k > kNearestMaxK || p.n_nodes < 1) return hipErrorInvalidValue;
  if (count == nullptr && index == nullptr && gap == nullptr) return hipErrorInvalidValue;
  const bool ranged = max_dist_dev != nullptr, pruned = count == nullptr;
  if (!ranged && !max_dist_ok(max_dist)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  if (ranged) return pruned ? launch_nearest_cap<true, true>(p, pts, max_dist_dev, 0.0f, k, exact_depth, count, index, gap, stream)
                            : launch_nearest_cap<true, false>(p, pts, max_dist_dev, 0.0f, k, exact_depth, count, index, gap, stream);
  return pruned ? launch_nearest_cap<false, true>(p, pts, nullptr, max_dist, k, exact_depth, count, index, gap, stream)
                : launch_nearest_cap<false, false>(p, pts, nullptr, max_dist, k, exact_depth, count, index, gap, stream);
}

// The CSR queries -- rt_spheres_within_* / rt_contact_pairs_*, rt_spheres_in_boxes_*, rt_spheres_in_planes_*, rt_spheres_along_rays_* -- and the
// contact clusters' hook share ONE walk and ONE row protocol; this is their contract (i, j, k, m).
// The walk (OrderedWalk), one lane per query, EVERY selected sphere, no key list: a row has no length limit.
//  * Order.  Rows come out in ASCENDING j with no sort: the leaves below a node are a contiguous run of L and the left child holds the lower
//    part, so a depth-first walk that takes the left child first meets the leaves in ascending j.  The children are therefore pushed right
//    then left, and a right child that is a leaf waits on the stack behind an inner left sibling.
//  * Stack entries.  The node (< 2^26) and its depth in bits 26..31.  Depth field 63 is the leaf tag: the entry is a sphere index; a node's
//    depth is capped at 62, above any exact_depth (height <= 63 and at least 3 sweeps).
//  * Depth.  With DEPTH a node's box is tested only at depth >= exact_depth: above it the reference's AABB propagation leaves boxes that need
//    not contain their subtrees (nearest_lane), and the walk descends through them untested.  Without DEPTH (the along-ray queries: the
//    answer is the tree's, as the sweep's) every popped node is tested, the root included, and every node entry carries depth 0.
//  * Stack bound.  One pending sibling per level: sp <= height + 1 <= kStackPixel.
//  * Leaves.  Sphere j is offered to the leaf action only if j >= first (first >= 0, so the empty leaf slot, -1, never passes); no subtree is
//    pruned by `first`.  The action loads the sphere itself, through the walk's descriptor, behind whatever test of j is its own.
// The row (CsrRow<FILL>).  The count pass (FILL false) and the fill pass evaluate ONE predicate in one order, so they select the same set.
// The count pass counts; the fill pass writes entry offsets[i] + rank, only below offsets[i + 1] and below `capacity`, and nothing for a
// negative offsets[i]: offsets from another query can misplace entries, never put one outside the caller's arrays.
constexpr int kWithinLeaf = 63, kWithinMaxDepth = 62;
__device__ __forceinline__ int within_node_entry(int node, int depth) {
  return (int)((unsigned)node | ((unsigned)(depth < kWithinMaxDepth ? depth : kWithinMaxDepth) << 26));
}
__device__ __forceinline__ int within_leaf_entry(int j) { return (int)((unsigned)j | ((unsigned)kWithinLeaf << 26)); }

struct OrderedWalk {
  const __amdgpu_buffer_rsrc_t rs_nodes, rs_sph;
  __device__ __forceinline__ explicit OrderedWalk(const KParams &p)
      : rs_nodes(make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u)), rs_sph(make_rsrc(p.sph, (unsigned)p.n_sph * 16u)) {}
  __device__ __forceinline__ float4 sphere(int j) const { return buf_load16(rs_sph, j * 16); }
  // node_test(lo, hi): may the node's box hold a selected sphere; leaf(j): the action on sphere j >= first
  template <bool DEPTH, class NodeTest, class Leaf>
  __device__ __forceinline__ void run(bool valid, int first, int exact_depth, NodeTest &&node_test, Leaf &&leaf) const {
    run<DEPTH>(valid, first, exact_depth, node_test, leaf, GroupView<false>(KParams{}, GroupArgs{}, 0));
  }
  // ... with a second node predicate, the sphere groups' (GroupView: may the subtree hold a seen sphere).  It is asked of an inner child where
  // the child would be pushed and of a sphere where it would be offered, so the order of the remaining leaves and the stack bound are the walk's.
  template <bool DEPTH, class NodeTest, class Leaf, class Groups>
  __device__ __forceinline__ void run(bool valid, int first, int exact_depth, NodeTest &&node_test, Leaf &&leaf, const Groups &gv) const {
    __shared__ int stack[kStackPixel][64];
    const int lane = threadIdx.x;
    int sp = 0;
    if (valid && gv.start()) stack[sp++][lane] = within_node_entry(0, 0);
    while (sp > 0) {
      const unsigned e = (unsigned)stack[--sp][lane];
      const int ni = (int)(e & 0x3ffffffu), depth = (int)(e >> 26);
      int slot[2] = {-1, -1};
      if (depth == kWithinLeaf) {
        slot[0] = ni;
      } else {
        const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
        if ((!DEPTH || depth >= exact_depth) && !node_test(lo, hi)) continue;
        const int l = f2i(lo.w), r = f2i(hi.w);
        if (l < 0) {
          slot[0] = ~l;
          if (r < 0) slot[1] = ~r;
          else if (gv.node(r)) stack[sp++][lane] = within_node_entry(r, DEPTH ? depth + 1 : 0);
        } else {
          if (r < 0 || gv.node(r)) stack[sp++][lane] = r < 0 ? within_leaf_entry(~r) : within_node_entry(r, DEPTH ? depth + 1 : 0);
          if (gv.node(l)) stack[sp++][lane] = within_node_entry(l, DEPTH ? depth + 1 : 0);
        }
      }
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
        if (slot[c2] >= first && gv.leaf(slot[c2])) leaf(slot[c2]);
    }
  }
};

// Row i of a CSR query: its length in the count pass, its write cursor in the fill pass (the contract above).
template <bool FILL>
struct CsrRow {
  int cnt = 0;
  int64_t at = 0, end = 0;
  __device__ __forceinline__ CsrRow(int i, const int64_t *offsets, int64_t capacity) {
    if constexpr (FILL) {
      at = offsets[i];
      end = offsets[i + 1] < capacity ? offsets[i + 1] : capacity;
      if (at < 0) at = end;   // (offsets that are not a scan of counts: nothing is written)
    }
  }
  // one offered sphere, selected or not: emit(at) writes a selected one's entry
  template <class Emit>
  __device__ __forceinline__ void take(bool selected, Emit &&emit) {
    if constexpr (FILL) {
      if (selected) {
        if (at < end) emit(at);
        ++at;
      }
    } else {
      cnt += selected ? 1 : 0;
    }
  }
  __device__ __forceinline__ void finish(int i, int32_t *count) const {
    if constexpr (!FILL) count[i] = cnt;
  }
};

// rt_spheres_within_* / rt_contact_pairs_* (DESIGN.md 3.5f): the node test is nearest_lane's box_may_hold with T = the point's bound, the leaf
// rule gap <= that bound.  SELF (contact pairs): point i is the centre of L[i], its bound fl(radius_i + max_dist), first = i + 1; `point` then
// is the pair array, rows {i, j}.
template <bool FILL, bool SELF, bool MASKED = false>
__device__ __forceinline__ void within_lane(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev,
                                            int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                            int32_t *point, const GroupArgs &ga = GroupArgs{}) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.nrays) return;
  const OrderedWalk walk(p);
  float px, py, pz;
  int first = 0;
  bool valid;
  if constexpr (SELF) {
    const float4 me = p.sph[i];
    px = me.x, py = me.y, pz = me.z;
    max_dist = (me.w + max_dist) + 0.0f;
    first = i + 1;
    valid = point_ok(px, py, pz) && max_dist_ok(max_dist);
  } else {
    px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
    if (max_dist_dev != nullptr) max_dist = max_dist_dev[i] + 0.0f;   // (-0.0 -> +0.0)
    if (first_dev != nullptr) first = first_dev[i] > 0 ? first_dev[i] : 0;
    valid = point_ok(px, py, pz) && max_dist_ok(max_dist);
  }
  const float pmag = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
  CsrRow<FILL> row(i, offsets, capacity);
  const auto node_test = [&](const float4 &lo, const float4 &hi) { return box_may_hold(px, py, pz, pmag, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, max_dist); };
  const auto leaf = [&](int j) {
    const float4 s = walk.sphere(j);
    const float g = point_gap(px, py, pz, s.x, s.y, s.z, s.w);
    row.take(g <= max_dist, [&](int64_t at) {
      if constexpr (SELF) {
        if (point != nullptr) *reinterpret_cast<int2 *>(point + 2 * at) = make_int2(i, j);
      } else {
        if (index != nullptr) index[at] = j;
        if (point != nullptr) point[at] = i;
      }
      if (gap != nullptr) gap[at] = g;
    });
  };
  walk.run<true>(valid, first, exact_depth, node_test, leaf, GroupView<MASKED>(p, ga, i));
  row.finish(i, count);
}
template <bool FILL, bool SELF>
__global__ __launch_bounds__(64) void within_kernel(KParams p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev,
                                                    int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index,
                                                    float *gap, int32_t *point) {
  within_lane<FILL, SELF>(p, pts, max_dist_dev, max_dist, first_dev, exact_depth, count, offsets, capacity, index, gap, point);
}

// The scan between the two passes: n int32 counts -> n + 1 int64 offsets (offsets[0] = 0, offsets[i + 1] = counts[0] + .. + counts[i]), in
// three plain launches.  No workgroup waits on another: 1. every workgroup sums its kWithinScanItems counts; 2. ONE workgroup turns the block
// sums into their exclusive prefix, kWithinScanThreads at a time with a running carry; 3. every workgroup scans its own counts again on top
// of its prefix.  All sums are 64-bit: a row may hold 2^26 entries, the total of 2^31 rows does not fit 32 bits.
constexpr int kWithinScanThreads = 256, kWithinScanPer = 4, kWithinScanItems = kWithinScanThreads * kWithinScanPer;
__device__ __forceinline__ long long wave_scan_incl(long long v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}
// inclusive scan of v over the workgroup's kWithinScanThreads threads; *total = the workgroup's sum (wsum: one slot per wave, reusable after return)
__device__ __forceinline__ long long block_scan_incl(long long v, long long *wsum, long long *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long incl = wave_scan_incl(v, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kWithinScanThreads / 64; ++k) {
    const long long w = wsum[k];
    if (k < wave) before += w;
    all += w;
  }
  __syncthreads();
  *total = all;
  return before + incl;
}
__device__ __forceinline__ void within_load_counts(const int32_t *counts, int n, int (&c)[kWithinScanPer]) {
  const long long at = ((long long)blockIdx.x * kWithinScanThreads + threadIdx.x) * kWithinScanPer;
#pragma unroll
  for (int q = 0; q < kWithinScanPer; ++q) c[q] = at + q < n ? counts[at + q] : 0;
}
__global__ __launch_bounds__(kWithinScanThreads) void within_scan_sums_kernel(const int32_t *counts, int n, long long *sums) {
  __shared__ long long wsum[kWithinScanThreads / 64];
  int c[kWithinScanPer];
  within_load_counts(counts, n, c);
  long long v = 0, total;
#pragma unroll
  for (int q = 0; q < kWithinScanPer; ++q) v += c[q];
  (void)block_scan_incl(v, wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kWithinScanThreads) void within_scan_carry_kernel(long long *sums, int nblocks) {
  __shared__ long long wsum[kWithinScanThreads / 64];
  long long carry = 0;   // (the same value in every thread)
  for (int base = 0; base < nblocks; base += kWithinScanThreads) {
    const int b = base + (int)threadIdx.x;
    const long long v = b < nblocks ? sums[b] : 0;
    long long total;
    const long long incl = block_scan_incl(v, wsum, &total);
    if (b < nblocks) sums[b] = carry + incl - v;
    carry += total;
  }
}
__global__ __launch_bounds__(kWithinScanThreads) void within_scan_apply_kernel(const int32_t *counts, int n, const long long *sums, int64_t *offsets) {
  __shared__ long long wsum[kWithinScanThreads / 64];
  int c[kWithinScanPer];
  within_load_counts(counts, n, c);
  long long v = 0, total;
#pragma unroll
  for (int q = 0; q < kWithinScanPer; ++q) v += c[q];
  long long run = sums[blockIdx.x] + block_scan_incl(v, wsum, &total) - v;
  const long long at = ((long long)blockIdx.x * kWithinScanThreads + threadIdx.x) * kWithinScanPer;
  if (at == 0) offsets[0] = 0;
#pragma unroll
  for (int q = 0; q < kWithinScanPer; ++q) {
    run += c[q];
    if (at + q < n) offsets[at + q + 1] = run;
  }
}

// A count pass's scratch: the n int32 counts, padded to 256 bytes, then the scan's block sums.
static int scan_blocks(int64_t n) { return (int)((n + kWithinScanItems - 1) / kWithinScanItems); }
static size_t scan_sums_at(int64_t n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }
size_t within_scratch_bytes(int64_t n) { return scan_sums_at(n) + (size_t)scan_blocks(n) * 8; }
// ... and the scan over it: the n counts at the start of `scratch` -> offsets[0 .. n]
static hipError_t launch_count_scan(char *scratch, int n, int64_t *offsets, hipStream_t stream) {
  const int32_t *const counts = reinterpret_cast<const int32_t *>(scratch);
  long long *const sums = reinterpret_cast<long long *>(scratch + scan_sums_at(n));
  const int nblocks = scan_blocks(n);
  hipLaunchKernelGGL(within_scan_sums_kernel, dim3(nblocks), dim3(kWithinScanThreads), 0, stream, counts, n, sums);
  hipLaunchKernelGGL(within_scan_carry_kernel, dim3(1), dim3(kWithinScanThreads), 0, stream, sums, nblocks);
  hipLaunchKernelGGL(within_scan_apply_kernel, dim3(nblocks), dim3(kWithinScanThreads), 0, stream, counts, n, sums, offsets);
  return hipGetLastError();
}

// What every CSR launcher answers before its family's own argument rules; true: *rc is the launcher's answer.  The count pass (fill false)
// refuses null offsets, answers no queries with offsets[0] = 0, and needs its scratch; the fill pass answers no queries with success and
// refuses null offsets, a negative capacity and `outputs` false (every output null).  Both need a tree.
static bool csr_answered(const KParams &p, bool fill, const int64_t *offsets, const char *scratch, int64_t capacity, bool outputs,
                         hipStream_t stream, hipError_t *rc) {
  *rc = hipErrorInvalidValue;
  if (!fill && offsets == nullptr) return true;
  if (p.nrays <= 0) {
    *rc = fill ? hipSuccess : hipMemsetAsync(const_cast<int64_t *>(offsets), 0, sizeof(int64_t), stream);   // (the count pass's own output)
    return true;
  }
  if (fill ? (offsets == nullptr || capacity < 0 || !outputs) : scratch == nullptr) return true;
  return p.n_nodes < 1;
}
static dim3 lane_grid(int n) { return dim3(((unsigned)n + 63u) / 64u); }

static bool within_args_ok(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, bool self) {
  if (self ? p.nrays != p.n_sph : pts == nullptr) return false;
  return (!self && max_dist_dev != nullptr) || max_dist_ok(max_dist);
}

hipError_t launch_within_count(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev, bool self,
                               int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, false, offsets, scratch, 0, true, stream, &rc)) return rc;
  if (!within_args_ok(p, pts, max_dist_dev, max_dist, self)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  int32_t *const counts = reinterpret_cast<int32_t *>(scratch);
  if (self)
    hipLaunchKernelGGL((within_kernel<false, true>), lane_grid(p.nrays), dim3(64), 0, stream, p, nullptr, nullptr, max_dist, nullptr, exact_depth,
                       counts, nullptr, (int64_t)0, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL((within_kernel<false, false>), lane_grid(p.nrays), dim3(64), 0, stream, p, pts, max_dist_dev, max_dist, first_dev,
                       exact_depth, counts, nullptr, (int64_t)0, nullptr, nullptr, nullptr);
  return launch_count_scan(scratch, p.nrays, offsets, stream);
}

hipError_t launch_within_fill(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev, bool self,
                              int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point,
                              hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, true, offsets, nullptr, capacity, index != nullptr || gap != nullptr || point != nullptr, stream, &rc)) return rc;
  if (!within_args_ok(p, pts, max_dist_dev, max_dist, self) || (self && index != nullptr)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  if (self)
    hipLaunchKernelGGL((within_kernel<true, true>), lane_grid(p.nrays), dim3(64), 0, stream, p, nullptr, nullptr, max_dist, nullptr, exact_depth,
                       nullptr, offsets, capacity, nullptr, gap, point);
  else
    hipLaunchKernelGGL((within_kernel<true, false>), lane_grid(p.nrays), dim3(64), 0, stream, p, pts, max_dist_dev, max_dist, first_dev,
                       exact_depth, nullptr, offsets, capacity, index, gap, point);
  return hipGetLastError();
}

// rt_contact_clusters: the connected components of the contact pairs' graph, with no pair list.  `root` is the union-find's
// parent array in place: clusters_init_kernel (root[i] = i), clusters_hook_kernel (the unions), clusters_flatten_kernel (root[i] = its root),
// then, as asked for, the dense ids through the range queries' scan and the sizes through integer atomics.
// Inside the hook and the flatten kernels EVERY access to the parent array goes through ParentOps: relaxed agent-scope atomics, which are
// served past the CU's L1.  No plain load, no fence: a stale parent is still a vertex of the same tree below its child, and root-ness is decided
// by the compare-exchange alone (query_core.h: uf_find / uf_unite); the kernel boundaries carry the array from one launch to the next.
struct ParentOps {
  int32_t *parent;
  __device__ __forceinline__ int32_t load(int32_t x) const { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(int32_t x, int32_t v) const {
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ int32_t cas(int32_t x, int32_t expect, int32_t v) const {
    (void)__hip_atomic_compare_exchange_strong(parent + x, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
  }
};
constexpr int kClustersThreads = 256;
__global__ __launch_bounds__(kClustersThreads) void clusters_init_kernel(int32_t *root, int n) {
  const long long i = (long long)blockIdx.x * kClustersThreads + threadIdx.x;
  if (i < n) root[i] = (int32_t)i;
}
// The hook: within_lane<false, true>'s query, node test and leaf rule over the same walk, with no row -- where the count pass counts, the union
// of i and j.  `mine` is the lane's own root so far, kept across its row: when j's root equals it (on a dense scene nearly every edge) there
// is no atomic.  It may have been hooked by another lane since; uf_unite then walks on from it.
__global__ __launch_bounds__(64) void clusters_hook_kernel(KParams p, float margin, int exact_depth, int32_t *root) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.n_sph) return;
  const OrderedWalk walk(p);
  const ParentOps ops{root};
  const float4 me = p.sph[i];
  const float px = me.x, py = me.y, pz = me.z;
  const float max_dist = (me.w + margin) + 0.0f;
  const bool valid = point_ok(px, py, pz) && max_dist_ok(max_dist);
  const float pmag = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
  int32_t mine = i;
  walk.run<true>(
      valid, i + 1, exact_depth,
      [&](const float4 &lo, const float4 &hi) { return box_may_hold(px, py, pz, pmag, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, max_dist); },
      [&](int j) {
        if (j >= p.n_sph) return;   // (j indexes root[], which no descriptor guards)
        const float4 s = walk.sphere(j);
        const float g = point_gap(px, py, pz, s.x, s.y, s.z, s.w);
        if (g <= max_dist) {
          const int32_t theirs = uf_find(ops, j);
          if (theirs != mine) mine = uf_unite(ops, mine, theirs);
        }
      });
}
// In place, and safe: no union runs any more, so every tree has its final root; the only store to word i is its owner's, of that root, and
// the walk stores nothing else (uf_root, not uf_find: a halving store landing behind the owner's would leave a non-root in the answer).  A
// lane that passes through a word reads its old parent or the root -- both lead to the root.
__global__ __launch_bounds__(kClustersThreads) void clusters_flatten_kernel(int32_t *root, int n) {
  const long long i = (long long)blockIdx.x * kClustersThreads + threadIdx.x;
  if (i >= n) return;
  const ParentOps ops{root};
  const int32_t r = uf_root(ops, (int32_t)i);
  if (r != (int32_t)i) ops.store((int32_t)i, r);
}
// root is final from here on: plain loads.  flag[i] = 1 at a cluster's root (the scan's input); size[] zeroed by the launcher.  The sizes are
// counted a wave at a time: the lanes that share the first active lane's root are counted by ballot and added once, then the rest go round
// again -- neighbours in L mostly share a root, and one cluster of 10^6 spheres is 15 625 atomics on its word instead of 10^6.
__global__ __launch_bounds__(kClustersThreads) void clusters_count_kernel(const int32_t *root, int n, int32_t *flag, int32_t *size) {
  const long long i = (long long)blockIdx.x * kClustersThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t r = root[i];
  if (flag != nullptr) flag[i] = r == (int32_t)i ? 1 : 0;
  if (size == nullptr) return;
  for (;;) {
    const int32_t lead = __builtin_amdgcn_readfirstlane(r);
    const unsigned long long same = __ballot(r == lead);
    if (r == lead) {
      if ((int)(threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(size + lead, __builtin_popcountll(same));
      return;
    }
  }
}
// cluster[i] = the number of roots below root[i]; size[i] = its root's count (a root's own entry already holds it and is only read here)
__global__ __launch_bounds__(kClustersThreads) void clusters_label_kernel(const int32_t *root, int n, const int64_t *offsets, int32_t *cluster,
                                                                          int32_t *size) {
  const long long i = (long long)blockIdx.x * kClustersThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t r = root[i];
  if (cluster != nullptr) cluster[i] = (int32_t)offsets[r];
  if (size != nullptr && r != (int32_t)i) size[i] = size[r];
}

// the scan's scratch over the root flags, then its n + 1 offsets
static size_t clusters_offsets_at(int64_t n) { return (within_scratch_bytes(n) + 255) & ~(size_t)255; }
size_t clusters_scratch_bytes(int64_t n) { return clusters_offsets_at(n) + ((size_t)n + 1) * 8; }

hipError_t launch_contact_clusters(const KParams &p, float margin, int exact_depth, char *scratch, int32_t *root, int32_t *cluster, int32_t *size,
                                   int64_t *num, hipStream_t stream) {
  const int n = p.n_sph;
  if (n < 1 || root == nullptr || !max_dist_ok(margin)) return hipErrorInvalidValue;
  if (n > 1 && p.n_nodes < 1) return hipErrorInvalidValue;
  const bool ids = cluster != nullptr || num != nullptr;
  if (ids && scratch == nullptr) return hipErrorInvalidValue;
  margin += 0.0f;   // (-0.0 -> +0.0)
  const dim3 flat((unsigned)(((int64_t)n + kClustersThreads - 1) / kClustersThreads)), threads(kClustersThreads);
  hipLaunchKernelGGL(clusters_init_kernel, flat, threads, 0, stream, root, n);
  if (n > 1) {   // (one sphere: no tree, no edge)
    hipLaunchKernelGGL(clusters_hook_kernel, lane_grid(n), dim3(64), 0, stream, p, margin, exact_depth, root);
    hipLaunchKernelGGL(clusters_flatten_kernel, flat, threads, 0, stream, root, n);
  }
  if (!ids && size == nullptr) return hipGetLastError();
  int32_t *const flag = ids ? reinterpret_cast<int32_t *>(scratch) : nullptr;
  int64_t *const offsets = ids ? reinterpret_cast<int64_t *>(scratch + clusters_offsets_at(n)) : nullptr;
  if (size != nullptr) {
    const hipError_t rc = hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)n, stream);
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL(clusters_count_kernel, flat, threads, 0, stream, root, n, flag, size);
  if (ids) {   // (the flags are the scan's counts)
    const hipError_t rc = launch_count_scan(scratch, n, offsets, stream);
    if (rc != hipSuccess) return rc;
  }
  if (cluster != nullptr || size != nullptr) hipLaunchKernelGGL(clusters_label_kernel, flat, threads, 0, stream, root, n, offsets, cluster, size);
  const hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  // (a copy, not a store from a kernel: num_dev needs only 4-byte alignment)
  if (num != nullptr) return hipMemcpyAsync(num, offsets + n, sizeof(int64_t), hipMemcpyDeviceToDevice, stream);
  return hipSuccess;
}

// rt_spheres_in_boxes_*: EVERY sphere whose gap to the lane's box is <= the box's margin, in CSR form.  One lane per box over
// the shared walk and row, with box_may_meet at the nodes and box_gap at the leaves (query_core.h).  A row of `boxes` is {lo.xyz, hi.xyz}, 24
// bytes: six 4-byte loads, only 4-byte alignment is assumed.  A box failing qbox_ok or a margin failing max_dist_ok does not start its walk.
template <bool FILL>
__device__ __forceinline__ void boxes_lane(const KParams &p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev,
                                           int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                           int32_t *point) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.nrays) return;
  const OrderedWalk walk(p);
  const float *const row6 = boxes + (size_t)i * 6;
  const QBox q = {row6[0], row6[1], row6[2], row6[3], row6[4], row6[5]};
  if (margin_dev != nullptr) margin = margin_dev[i] + 0.0f;   // (-0.0 -> +0.0)
  int first = 0;
  if (first_dev != nullptr) first = first_dev[i] > 0 ? first_dev[i] : 0;
  const bool valid = qbox_ok(q) && max_dist_ok(margin);
  const float qmag = box_mag(q.lox, q.loy, q.loz, q.hix, q.hiy, q.hiz);
  CsrRow<FILL> row(i, offsets, capacity);
  walk.run<true>(
      valid, first, exact_depth,
      [&](const float4 &lo, const float4 &hi) { return box_may_meet(q, qmag, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, margin); },
      [&](int j) {
        const float4 s = walk.sphere(j);
        const float g = box_gap(q, s.x, s.y, s.z, s.w);
        row.take(g <= margin, [&](int64_t at) {
            if (index != nullptr) index[at] = j;
            if (point != nullptr) point[at] = i;
            if (gap != nullptr) gap[at] = g;
          });
      });
  row.finish(i, count);
}
template <bool FILL>
__global__ __launch_bounds__(64) void boxes_kernel(KParams p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev,
                                                   int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index,
                                                   float *gap, int32_t *point) {
  boxes_lane<FILL>(p, boxes, margin_dev, margin, first_dev, exact_depth, count, offsets, capacity, index, gap, point);
}

hipError_t launch_boxes_count(const KParams &p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev, int exact_depth,
                              char *scratch, int64_t *offsets, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, false, offsets, scratch, 0, true, stream, &rc)) return rc;
  if (boxes == nullptr || (margin_dev == nullptr && !max_dist_ok(margin))) return hipErrorInvalidValue;
  margin += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((boxes_kernel<false>), lane_grid(p.nrays), dim3(64), 0, stream, p, boxes, margin_dev, margin, first_dev, exact_depth,
                     reinterpret_cast<int32_t *>(scratch), nullptr, (int64_t)0, nullptr, nullptr, nullptr);
  return launch_count_scan(scratch, p.nrays, offsets, stream);
}

hipError_t launch_boxes_fill(const KParams &p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev, int exact_depth,
                             const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, true, offsets, nullptr, capacity, index != nullptr || gap != nullptr || point != nullptr, stream, &rc)) return rc;
  if (boxes == nullptr || (margin_dev == nullptr && !max_dist_ok(margin))) return hipErrorInvalidValue;
  margin += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((boxes_kernel<true>), lane_grid(p.nrays), dim3(64), 0, stream, p, boxes, margin_dev, margin, first_dev, exact_depth, nullptr,
                     offsets, capacity, index, gap, point);
  return hipGetLastError();
}

// rt_spheres_in_planes_*: EVERY sphere whose gap to the lane's K planes is <= the query's margin, in CSR form.  One lane per
// query over the shared walk and row, with planes_may_meet at the nodes and plane_gap at the leaves (query_core.h).  A query's planes are K
// rows {a, b, c, d} of 16 bytes: 4 K 4-byte loads, only 4-byte alignment is assumed, and one normalisation per plane before the walk.  K is a
// template parameter, so the planes stay in 4 K registers through the fully unrolled loops.  A query with a plane failing plane_normalise or a
// margin failing max_dist_ok does not start its walk.
template <int K, bool FILL>
__device__ __forceinline__ void planes_lane(const KParams &p, const float *planes, const float *margin_dev, float margin, const int32_t *first_dev,
                                            int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                            int32_t *point) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.nrays) return;
  const OrderedWalk walk(p);
  const float *const row4 = planes + (size_t)i * (4 * K);
  QPlane pl[K];
  bool valid = true;
#pragma unroll
  for (int k = 0; k < K; ++k) valid &= plane_normalise(row4[4 * k], row4[4 * k + 1], row4[4 * k + 2], row4[4 * k + 3], &pl[k]);
  if (margin_dev != nullptr) margin = margin_dev[i] + 0.0f;   // (-0.0 -> +0.0)
  int first = 0;
  if (first_dev != nullptr) first = first_dev[i] > 0 ? first_dev[i] : 0;
  valid = valid && max_dist_ok(margin);
  const float wmag = planes_wmag(pl);
  CsrRow<FILL> row(i, offsets, capacity);
  walk.run<true>(
      valid, first, exact_depth,
      [&](const float4 &lo, const float4 &hi) { return planes_may_meet(pl, wmag, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, margin); },
      [&](int j) {
        const float4 s = walk.sphere(j);
        const float g = plane_gap(pl, s.x, s.y, s.z, s.w);
        row.take(g <= margin, [&](int64_t at) {
            if (index != nullptr) index[at] = j;
            if (point != nullptr) point[at] = i;
            if (gap != nullptr) gap[at] = g;
          });
      });
  row.finish(i, count);
}
template <int K, bool FILL>
__global__ __launch_bounds__(64) void planes_kernel(KParams p, const float *planes, const float *margin_dev, float margin, const int32_t *first_dev,
                                                    int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index,
                                                    float *gap, int32_t *point) {
  planes_lane<K, FILL>(p, planes, margin_dev, margin, first_dev, exact_depth, count, offsets, capacity, index, gap, point);
}
// one instantiation per plane count, 1 .. kMaxPlanes
template <bool FILL>
static void launch_planes_kernel(int nplanes, const KParams &p, const float *planes, const float *margin_dev, float margin, const int32_t *first_dev,
                                 int exact_depth, int32_t *count, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                 int32_t *point, hipStream_t stream) {
  const dim3 grid = lane_grid(p.nrays), block(64);
#define RT_PLANES_CASE(KK)                                                                                                                       \
  case KK:                                                                                                                                        \
    hipLaunchKernelGGL((planes_kernel<KK, FILL>), grid, block, 0, stream, p, planes, margin_dev, margin, first_dev, exact_depth, count, offsets, \
                       capacity, index, gap, point);                                                                                              \
    break;
  switch (nplanes) {
    RT_PLANES_CASE(1) RT_PLANES_CASE(2) RT_PLANES_CASE(3) RT_PLANES_CASE(4) RT_PLANES_CASE(5) RT_PLANES_CASE(6) RT_PLANES_CASE(7) RT_PLANES_CASE(8)
  }
#undef RT_PLANES_CASE
}

hipError_t launch_planes_count(const KParams &p, const float *planes, int nplanes, const float *margin_dev, float margin, const int32_t *first_dev,
                               int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream) {
  hipError_t rc;
  if (nplanes < 1 || nplanes > kMaxPlanes) return hipErrorInvalidValue;
  if (csr_answered(p, false, offsets, scratch, 0, true, stream, &rc)) return rc;
  if (planes == nullptr || (margin_dev == nullptr && !max_dist_ok(margin))) return hipErrorInvalidValue;
  margin += 0.0f;   // (-0.0 -> +0.0)
  launch_planes_kernel<false>(nplanes, p, planes, margin_dev, margin, first_dev, exact_depth, reinterpret_cast<int32_t *>(scratch), nullptr,
                              (int64_t)0, nullptr, nullptr, nullptr, stream);
  return launch_count_scan(scratch, p.nrays, offsets, stream);
}

hipError_t launch_planes_fill(const KParams &p, const float *planes, int nplanes, const float *margin_dev, float margin, const int32_t *first_dev,
                              int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point,
                              hipStream_t stream) {
  hipError_t rc;
  if (nplanes < 1 || nplanes > kMaxPlanes) return hipErrorInvalidValue;
  if (csr_answered(p, true, offsets, nullptr, capacity, index != nullptr || gap != nullptr || point != nullptr, stream, &rc)) return rc;
  if (planes == nullptr || (margin_dev == nullptr && !max_dist_ok(margin))) return hipErrorInvalidValue;
  margin += 0.0f;   // (-0.0 -> +0.0)
  launch_planes_kernel<true>(nplanes, p, planes, margin_dev, margin, first_dev, exact_depth, nullptr, offsets, capacity, index, gap, point, stream);
  return hipGetLastError();
}

// rt_spheres_along_rays_*: EVERY sphere a ray crosses or a moving sphere touches over its interval, in CSR form.  One lane
// per query.  From sweep_lane's RANGED form the SELECTION: every popped node's box widened by the query's rq (six additions) through
// box_hit_interval over (t_min, t_max) -- the walk without DEPTH -- the leaf's j != skip, and the contact rule (sweep_contact_roots:
// sweep_contact's kind, plus the two roots it compared).  From the shared walk and row the ORDER and the protocol.  No sorted list: one
// counter, or one cursor.  The per-query radius and interval are kernel arguments, each scalar or per query: radius_dev / tlo_dev / thi_dev
// nullptr means the scalar next to it (tlo_dev and thi_dev: both or neither).  A per-query interval failing interval_ok or radius failing
// max_dist_ok does not start its walk.  A row of `roots` is {t1, t2}, one 8-byte store; only 4-byte alignment of the array is assumed (as the
// pair rows of within_lane<.., SELF>).
template <bool FILL>
__device__ __forceinline__ void along_lane(const KParams &p, const float *radius_dev, float rq, const float *tlo_dev, const float *thi_dev,
                                           float t_min, float t_max, const int32_t *exclude, const int32_t *first_dev, int32_t *count,
                                           const int64_t *offsets, int64_t capacity, int32_t *index, float *roots, uint8_t *start,
                                           int32_t *query) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.nrays) return;
  const OrderedWalk walk(p);
  const Ray r = load_ray(p.rays, i);
  bool valid = true;
  if (tlo_dev != nullptr) {
    t_min = tlo_dev[i];
    t_max = thi_dev[i];
    valid = interval_ok(t_min, t_max);
  }
  if (radius_dev != nullptr) {
    rq = radius_dev[i] + 0.0f;   // (-0.0 -> +0.0)
    valid = valid && max_dist_ok(rq);
  }
  const int skip = exclude != nullptr ? exclude[i] : -1;
  int first = 0;
  if (first_dev != nullptr) first = first_dev[i] > 0 ? first_dev[i] : 0;
  CsrRow<FILL> row(i, offsets, capacity);
  walk.run<false>(
      valid, first, 0,
      [&](const float4 &lo, const float4 &hi) {
        return box_hit_interval(r, lo.x - rq, lo.y - rq, lo.z - rq, hi.x + rq, hi.y + rq, hi.z + rq, t_min, t_max);
      },
      [&](int j) {
        if (j == skip) return;
        const float4 s = walk.sphere(j);
        float tau, t1, t2;
        const int what = sweep_contact_roots(r, s.x, s.y, s.z, s.w, rq, t_min, t_max, &tau, &t1, &t2);
        row.take(what != kSweepNone, [&](int64_t at) {
            if (index != nullptr) index[at] = j;
            if (roots != nullptr) *reinterpret_cast<float2 *>(roots + 2 * at) = make_float2(t1, t2);
            if (start != nullptr) start[at] = what == kSweepStart ? (uint8_t)1 : (uint8_t)0;
            if (query != nullptr) query[at] = i;
          });
      });
  row.finish(i, count);
}
template <bool FILL>
__global__ __launch_bounds__(64) void along_kernel(KParams p, const float *radius_dev, float rq, const float *tlo_dev, const float *thi_dev,
                                                   float t_min, float t_max, const int32_t *exclude, const int32_t *first_dev, int32_t *count,
                                                   const int64_t *offsets, int64_t capacity, int32_t *index, float *roots, uint8_t *start,
                                                   int32_t *query) {
  along_lane<FILL>(p, radius_dev, rq, tlo_dev, thi_dev, t_min, t_max, exclude, first_dev, count, offsets, capacity, index, roots, start, query);
}

// the launchers' shared argument rule: a scalar interval or radius is checked only where it is used
static bool along_args_ok(const float *radius_dev, float radius, const float *tlo_dev, const float *thi_dev, float t_min, float t_max) {
  if ((tlo_dev == nullptr) != (thi_dev == nullptr)) return false;
  if (tlo_dev == nullptr && !interval_ok(t_min, t_max)) return false;
  return radius_dev != nullptr || max_dist_ok(radius);
}

hipError_t launch_along_count(const KParams &p, const float *radius_dev, float radius, const float *tlo_dev, const float *thi_dev, float t_min,
                              float t_max, const int32_t *exclude, const int32_t *first_dev, char *scratch, int64_t *offsets, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, false, offsets, scratch, 0, true, stream, &rc)) return rc;
  if (p.rays == nullptr || !along_args_ok(radius_dev, radius, tlo_dev, thi_dev, t_min, t_max)) return hipErrorInvalidValue;
  radius += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((along_kernel<false>), lane_grid(p.nrays), dim3(64), 0, stream, p, radius_dev, radius, tlo_dev, thi_dev, t_min, t_max, exclude,
                     first_dev, reinterpret_cast<int32_t *>(scratch), nullptr, (int64_t)0, nullptr, nullptr, nullptr, nullptr);
  return launch_count_scan(scratch, p.nrays, offsets, stream);
}

hipError_t launch_along_fill(const KParams &p, const float *radius_dev, float radius, const float *tlo_dev, const float *thi_dev, float t_min,
                             float t_max, const int32_t *exclude, const int32_t *first_dev, const int64_t *offsets, int64_t capacity,
                             int32_t *index, float *roots, uint8_t *start, int32_t *query, hipStream_t stream) {
  hipError_t rc;
  const bool outputs = index != nullptr || roots != nullptr || start != nullptr || query != nullptr;
  if (csr_answered(p, true, offsets, nullptr, capacity, outputs, stream, &rc)) return rc;
  if (p.rays == nullptr || !along_args_ok(radius_dev, radius, tlo_dev, thi_dev, t_min, t_max)) return hipErrorInvalidValue;
  radius += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((along_kernel<true>), lane_grid(p.nrays), dim3(64), 0, stream, p, radius_dev, radius, tlo_dev, thi_dev, t_min, t_max, exclude,
                     first_dev, nullptr, offsets, capacity, index, roots, start, query);
  return hipGetLastError();
}

// rt_trace_paths: the mirror-bounce chain of each ray -- ray_colour's loop (ray.fut:126-148) with every vertex kept.  One wave per
// workgroup; the wave owns the block of `per_wave` consecutive rays [blockIdx.x * per_wave, ...) and its lanes start on the block's first 64.
// A lane holds one ray's loop state (the ray, light, depth) and the fold of the current objs_hit: intersect_lane's stack walk over (0, 1e9)
// (box_hit_interval, sphere_root / closest_update), then rehit_range(r, 0.0f, best, ..) and path_bounce (query_core.h).  Vertex s is stored
// when it is found, at slot s < k of the ray's row, so k costs no registers; the padding behind min(count, k) and the per-ray outputs are
// written when the ray ends.
// Phases: lanes whose stack is not empty walk one node per step; a lane whose fold is finished waits until kPathsVote lanes wait or nobody
// walks, then those lanes bounce together (the bounce is ~10 node steps long: two divisions and two square roots).
// Refill: behind a bounce phase the idle lanes (ray ended, or none yet) claim the block's next unclaimed rays in lane order -- a ballot of
// the idle lanes, each one's rank among them by mbcnt, the cursor advanced by their number: wave-uniform, no atomics, no barriers.  The
// wave leaves when no lane holds a ray and the block is used up.  Every loop is bounded: the walk by the tree (sp <= height + 1), the bounces
// of a ray by max_depth, the refills by per_wave, the padding by k.  Ray i's outputs are a function of ray i alone: per_wave cannot
// change a bit.  A non-finite or zero-direction ray takes the same bounded loops (its compares fail or pass, nothing else).
constexpr int kPathsVote = 24;   // (measured against 1, 8, 40 and 64: DESIGN.md 3.5h)
__global__ __launch_bounds__(64) void paths_kernel(KParams p, int max_depth, int k, int per_wave, int32_t *count, uint8_t *end, int32_t *index,
                                                   float *hit7, float *light3, float *last_ray6, float *colour3) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const long long block_lo = (long long)blockIdx.x * per_wave;
  const long long block_hi = block_lo + per_wave < (long long)p.nrays ? block_lo + per_wave : (long long)p.nrays;
  long long cursor = block_lo;   // the block's next unclaimed ray (wave-uniform)
  bool active = false;
  int i = 0, sp = 0, depth = 0, bestj = -1;
  float best = kTMax, lr = 1.0f, lg = 1.0f, lb = 1.0f;
  Ray r = {};

  // the ray has ended: its padding and per-ray outputs (cnt vertices, the first min(cnt, k) already stored)
  auto finish = [&](int code, int cnt, const Ray &last, const float *lt, const float *col) {
    if (count != nullptr) count[i] = cnt;
    if (end != nullptr) end[i] = (uint8_t)code;
    const size_t row = (size_t)i * (size_t)k;
    for (int s = cnt < k ? cnt : k; s < k; ++s) {
      if (index != nullptr) index[row + s] = -1;
      if (hit7 != nullptr) {
        float *const o = hit7 + (row + s) * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) o[q] = 0.0f;
      }
    }
    if (light3 != nullptr) {
      float *const o = light3 + (size_t)i * 3;
      o[0] = lt[0]; o[1] = lt[1]; o[2] = lt[2];
    }
    if (last_ray6 != nullptr) {
      float *const o = last_ray6 + (size_t)i * 6;
      o[0] = last.ox; o[1] = last.oy; o[2] = last.oz;
      o[3] = last.dx; o[4] = last.dy; o[5] = last.dz;
    }
    if (colour3 != nullptr) {
      float *const o = colour3 + (size_t)i * 3;
      o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
    }
  };

  for (;;) {
    // refill: the idle lanes claim the next rays of the block
    const unsigned long long idle = __ballot(!active);
    if (idle != 0ull && cursor < block_hi) {
      const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
      const long long mine = cursor + rank;
      if (!active && mine < block_hi) {
        i = (int)mine;
        r = load_ray(p.rays, i);
        lr = lg = lb = 1.0f;
        depth = 0;
        if (max_depth > 0) {
          active = true;
          best = kTMax;
          bestj = -1;
          stack[0][lane] = 0;
          sp = 1;
        } else {
          // `while depth < 0`: no objs_hit at all -- the initial loop variables, colour (0, 0, 0)
          const float lt[3] = {1.0f, 1.0f, 1.0f}, col[3] = {0.0f, 0.0f, 0.0f};
          finish(kPathTruncated, 0, r, lt, col);
        }
      }
      cursor += __popcll(idle);
    }
    const unsigned long long act = __ballot(active);
    if (act == 0ull) {
      if (cursor >= block_hi) break;
      continue;
    }
    // walk: one node per step, until enough lanes wait with a finished fold
    for (;;) {
      const bool walking = active && sp > 0;
      const unsigned long long wk = __ballot(walking);
      if (wk == 0ull || __popcll(act) - __popcll(wk) >= kPathsVote) break;
      if (walking) {
        const int ni = stack[--sp][lane];
        const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
        if (box_hit_interval(r, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, 0.0f, kTMax)) {
          const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2) {
            const int c = kids[c2];
            if (c < 0) {
              const int j = ~c;
              const float4 s = buf_load16(rs_sph, j * 16);
              closest_update(sphere_root(r, s.x, s.y, s.z, s.w), j, best, bestj);
            } else {
              stack[sp++][lane] = c;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
            }
          }
        }
      }
    }
    // bounce: the lanes whose fold is finished
    if (active && sp == 0) {
      float t = 0.0f;
      bool have = false;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f), c = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bestj >= 0) {
        s = p.sph[bestj];
        c = p.col[bestj];   // {colour, 1.0f / radius}
        have = rehit_range(r, 0.0f, best, s.x, s.y, s.z, s.w, &t);
      }
      float h[7], nl[3], col[3];
      Ray nr;
      const int code = path_bounce(r, have, t, s.x, s.y, s.z, c.x, c.y, c.z, c.w, lr, lg, lb, depth, max_depth, h, &nr, nl, col);
      if (have && depth < k) {
        const size_t slot = (size_t)i * (size_t)k + (size_t)depth;
        if (index != nullptr) index[slot] = bestj;
        if (hit7 != nullptr) {
          float *const o = hit7 + slot * 7;
#pragma unroll
          for (int q = 0; q < 7; ++q) o[q] = h[q];
        }
      }
      if (code == kPathContinue) {
        r = nr;
        lr = nl[0]; lg = nl[1]; lb = nl[2];
        depth += 1;
        best = kTMax;
        bestj = -1;
        stack[0][lane] = 0;
        sp = 1;
      } else {
        finish(code, have ? depth + 1 : depth, nr, nl, col);
        active = false;
      }
    }
  }
}

hipError_t launch_trace_paths(const KParams &p, int max_depth, int k, int per_wave, int32_t *count, uint8_t *end, int32_t *index, float *hit7,
                              float *light3, float *last_ray6, float *colour3, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (max_depth < 0 || k < 1 || k > kPathsMaxK || p.n_nodes < 1) return hipErrorInvalidValue;
  if (per_wave < 64 || per_wave > kPathsMaxPerWave || per_wave % 64 != 0) return hipErrorInvalidValue;
  if (count == nullptr && end == nullptr && index == nullptr && hit7 == nullptr && light3 == nullptr && last_ray6 == nullptr && colour3 == nullptr)
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(((long long)p.nrays + per_wave - 1) / per_wave);
  hipLaunchKernelGGL(paths_kernel, dim3(grid), dim3(64), 0, stream, p, max_depth, k, per_wave, count, end, index, hit7, light3, last_ray6, colour3);
  return hipGetLastError();
}

// rt_visible_pairs: every point against every target (DIRS false: d = fl(T_j - P_i) per component) or direction (DIRS true: d = T_j), one bit
// per pair and a count per point.  pair_visible is one lane's pair: the ray is built in registers from the point and the
// target row `tg` (three 4-byte loads: 12-byte rows, 4-byte aligned) and walked as occluded_lane walks it -- the same stack,
// box_hit_interval, sphere_hit_any and early exit -- so the answer is what rt_occluded_rays gives for that ray, negated.  A pair whose o or d
// has a non-finite component, or whose d is (+-0, +-0, +-0), is not visible and does not start its walk; neither does a lane that holds no pair
// (`have` false: nothing is loaded).
template <bool DIRS>
__device__ __forceinline__ bool pair_visible(const __amdgpu_buffer_rsrc_t rs_nodes, const __amdgpu_buffer_rsrc_t rs_sph, int (*stack)[64], int lane,
                                             bool have, float px, float py, float pz, const float *tg, float t_min, float t_max) {
  bool valid = have && point_ok(px, py, pz);
  Ray r;
  r.ox = px; r.oy = py; r.oz = pz;
  r.dx = r.dy = r.dz = 1.0f;
  if (valid) {
    const float tx = tg[0], ty = tg[1], tz = tg[2];
    r.dx = DIRS ? tx : tx - px;
    r.dy = DIRS ? ty : ty - py;
    r.dz = DIRS ? tz : tz - pz;
    valid = point_ok(r.dx, r.dy, r.dz) && !(r.dx == 0.0f && r.dy == 0.0f && r.dz == 0.0f);
  }
  ray_derive(r);
  bool hit = false;
  int sp = 0;
  if (valid) stack[sp++][lane] = 0;
  while (sp > 0 && !hit) {
    const int ni = stack[--sp][lane];
    const float4 lo = buf_load16(rs_nodes, ni * 32), hi = buf_load16(rs_nodes, ni * 32 + 16);
    if (!box_hit_interval(r, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, t_min, t_max)) continue;
    const int kids[2] = {f2i(lo.w), f2i(hi.w)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ch = kids[k];
      if (ch < 0) {
        const float4 s = buf_load16(rs_sph, ~ch * 16);
        hit = hit || sphere_hit_any(r, t_min, t_max, s.x, s.y, s.z, s.w);
      } else {
        stack[sp++][lane] = ch;   // (at most one pending sibling per level: sp <= tree height + 1 <= kStackPixel)
      }
    }
  }
  return valid && !hit;
}

// The general shape, one wave per workgroup.  A wave owns ONE point i and the run of `words_per_wave` consecutive 64-target words
// [c * words_per_wave, ...) of its row, blockIdx.x = i * chunks + c with chunks = ceil(words / words_per_wave); lane l of word w is pair
// (i, 64 w + l).  i is wave-uniform, so the point's three floats are uniform loads.  A lane with j >= m holds no pair, so the tail bits of a
// row's last word are 0 by construction.  The word is the wave's ballot, stored by lane 0 with one 8-byte vector store.  The count is the sum
// of the words' popcounts: stored once where the wave owns the whole row (chunks == 1), else added with atomicAdd to count[i], which the
// launcher zeroed on the same stream -- integer sums, so exact whatever the order.  words_per_wave changes no bit of either output.
template <bool DIRS>
__global__ __launch_bounds__(64) void pairs_kernel(KParams p, const float *points, const float *targets, int m, int words, int words_per_wave,
                                                   float t_min, float t_max, unsigned long long *visible, int32_t *count) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const unsigned chunks = ((unsigned)words + (unsigned)words_per_wave - 1u) / (unsigned)words_per_wave;
  const unsigned i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;   // (the grid is n * chunks: i < n)
  const float *const pt = points + (size_t)i * 3;
  const float px = pt[0], py = pt[1], pz = pt[2];
  const int w_lo = (int)c * words_per_wave, w_hi = w_lo + words_per_wave < words ? w_lo + words_per_wave : words;
  int total = 0;
  for (int w = w_lo; w < w_hi; ++w) {
    const int j = w * 64 + lane;
    const bool vis = pair_visible<DIRS>(rs_nodes, rs_sph, stack, lane, j < m, px, py, pz, targets + (size_t)j * 3, t_min, t_max);
    const unsigned long long word = __ballot(vis);
    if (visible != nullptr && lane == 0) visible[(size_t)i * (size_t)words + (size_t)w] = word;
    total += __popcll(word);
  }
  if (count != nullptr && lane == 0) {
    if (chunks == 1u) count[i] = total;
    else if (total != 0) atomicAdd(&count[i], total);
  }
}

// The shape for short rows, m <= kPairsPackedMax = 32 (a row is one word): with one point per wave 64 - m lanes would hold no pair, so a
// wave owns the 64 >> shift consecutive points [blockIdx.x * (64 >> shift), ...), G = 1 << shift being the least power of two >= m: lane l is
// pair (that base + l / G, l % G).  The point is then a per-lane load.  A point's word is its G lanes' slice of the wave's ballot, stored
// by the slice's first lane with its popcount -- whole rows, so no atomics.  The same pair_visible: the shape changes no bit.
template <bool DIRS>
__global__ __launch_bounds__(64) void pairs_packed_kernel(KParams p, const float *points, const float *targets, int m, int shift, float t_min,
                                                          float t_max, unsigned long long *visible, int32_t *count) {
  __shared__ int stack[kStackPixel][64];
  const int lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rs_nodes = make_rsrc(p.nodes, (unsigned)p.n_nodes * 32u);
  const __amdgpu_buffer_rsrc_t rs_sph = make_rsrc(p.sph, (unsigned)p.n_sph * 16u);
  const long long i = (long long)blockIdx.x * (64 >> shift) + (lane >> shift);
  const int j = lane & ((1 << shift) - 1);
  const bool have = i < (long long)p.nrays && j < m;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (have) {
    const float *const pt = points + (size_t)i * 3;
    px = pt[0], py = pt[1], pz = pt[2];
  }
  const bool vis = pair_visible<DIRS>(rs_nodes, rs_sph, stack, lane, have, px, py, pz, targets + (size_t)j * 3, t_min, t_max);
  const unsigned long long all = __ballot(vis);
  const unsigned long long word = (all >> (lane - j)) & ((1ull << (1 << shift)) - 1ull);   // (1 << shift <= 32)
  if (j == 0 && i < (long long)p.nrays) {
    if (visible != nullptr) visible[i] = word;
    if (count != nullptr) count[i] = __popcll(word);
  }
}

// words_per_wave: kPairsPacked (m <= kPairsPackedMax: the packed shape), or the general shape's run length >= 1 (above `words`: the whole row)
hipError_t launch_visible_pairs(const KParams &p, const float *points, const float *targets, int m, bool directions, int words_per_wave,
                                float t_min, float t_max, unsigned long long *visible, int32_t *count, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (points == nullptr || targets == nullptr || m < 1 || m > kPairsMaxTargets || p.n_nodes < 1) return hipErrorInvalidValue;
  if (visible == nullptr && count == nullptr) return hipErrorInvalidValue;
  if (!interval_ok(t_min, t_max)) return hipErrorInvalidValue;
  const int words = (m + 63) / 64;
  if ((long long)p.nrays * words >= (1ll << 31)) return hipErrorInvalidValue;
  if (words_per_wave == kPairsPacked) {
    if (m > kPairsPackedMax) return hipErrorInvalidValue;
    int shift = 0;
    while ((1 << shift) < m) ++shift;
    const int per_wave = 64 >> shift;
    const dim3 grid((unsigned)(((long long)p.nrays + per_wave - 1) / per_wave)), block(64);
    if (directions) hipLaunchKernelGGL((pairs_packed_kernel<true>), grid, block, 0, stream, p, points, targets, m, shift, t_min, t_max, visible, count);
    else hipLaunchKernelGGL((pairs_packed_kernel<false>), grid, block, 0, stream, p, points, targets, m, shift, t_min, t_max, visible, count);
    return hipGetLastError();
  }
  if (words_per_wave < 1) return hipErrorInvalidValue;
  if (words_per_wave > words) words_per_wave = words;
  const int chunks = (words + words_per_wave - 1) / words_per_wave;
  if (count != nullptr && chunks > 1) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)p.nrays, stream);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)((long long)p.nrays * chunks)), block(64);   // (n * chunks <= n * words < 2^31)
  if (directions) hipLaunchKernelGGL((pairs_kernel<true>), grid, block, 0, stream, p, points, targets, m, words, words_per_wave, t_min, t_max, visible, count);
  else hipLaunchKernelGGL((pairs_kernel<false>), grid, block, 0, stream, p, points, targets, m, words, words_per_wave, t_min, t_max, visible, count);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void camera_rays_kernel(Cam cam, int h, int w, float *rays) {
  const int64_t n = (int64_t)h * w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / w), col = (int)(i - (int64_t)row * w);
    const Ray r = primary_ray(cam, col, row, w, h);
    float *const o = rays + i * 6;
    o[0] = r.ox; o[1] = r.oy; o[2] = r.oz;
    o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
  }
}

hipError_t launch_camera_rays(const Cam &cam, int h, int w, float *rays, hipStream_t stream) {
  const int64_t n = (int64_t)h * w;
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  hipLaunchKernelGGL(camera_rays_kernel, dim3(grid), dim3(256), 0, stream, cam, h, w, rays);
  return hipGetLastError();
}

// ---- sphere groups ------------------------------------------------------------------------------------------------------
// The masked lane kernels: the MASKED instantiations of the lanes above -- the same walks, LDS stacks and 64-thread workgroups, with GroupView's
// two tests -- behind kernel entries of their own.  A masked query sees sphere j iff group_seen(groups[j], mask); the answer is the unmasked
// entry's with every unseen sphere absent at the leaf, and skipping a subtree whose node word shares no bit with the mask removes only unseen
// spheres.
template <bool RANGED>
__global__ __launch_bounds__(64) void intersect_masked_kernel(KParams p, GroupArgs ga, float t_min, float t_max, int32_t *index, float *hit7) {
  intersect_lane<RANGED, true>(p, t_min, t_max, index, hit7, ga);
}
template <bool RANGED>
__global__ __launch_bounds__(64) void occluded_masked_kernel(KParams p, GroupArgs ga) {
  occluded_lane<RANGED, true>(p, ga);
}
template <bool RANGED, bool PRUNED, int CAP>
__global__ __launch_bounds__(64) void nearest_masked_kernel(KParams p, GroupArgs ga, const float *pts, const float *max_dist_dev, float max_dist, int k,
                                                            int exact_depth, int32_t *count, int32_t *index, float *gap) {
  nearest_lane<RANGED, PRUNED, CAP, true>(p, pts, max_dist_dev, max_dist, k, exact_depth, count, index, gap, ga);
}
template <bool FILL>
__global__ __launch_bounds__(64) void within_masked_kernel(KParams p, GroupArgs ga, const float *pts, const float *max_dist_dev, float max_dist,
                                                           const int32_t *first_dev, int exact_depth, int32_t *count, const int64_t *offsets,
                                                           int64_t capacity, int32_t *index, float *gap, int32_t *point) {
  within_lane<FILL, false, true>(p, pts, max_dist_dev, max_dist, first_dev, exact_depth, count, offsets, capacity, index, gap, point, ga);
}

static bool group_args_ok(const KParams &p, const GroupArgs &ga) { return ga.groups != nullptr && ga.node_groups != nullptr && p.n_nodes >= 1; }

hipError_t launch_intersect_rays_masked(const KParams &p, const GroupArgs &ga, float t_min, float t_max, int32_t *index, float *hit7,
                                        hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (!group_args_ok(p, ga) || index == nullptr || (p.ray_tlo_dev == nullptr) != (p.ray_thi_dev == nullptr)) return hipErrorInvalidValue;
  if (p.ray_tlo_dev != nullptr)
    hipLaunchKernelGGL((intersect_masked_kernel<true>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga, 0.0f, 0.0f, index, hit7);
  else
    hipLaunchKernelGGL((intersect_masked_kernel<false>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga, t_min, t_max, index, hit7);
  return hipGetLastError();
}

hipError_t launch_occluded_rays_masked(const KParams &p, const GroupArgs &ga, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (!group_args_ok(p, ga) || p.occluded == nullptr || (p.ray_tlo_dev == nullptr) != (p.ray_thi_dev == nullptr)) return hipErrorInvalidValue;
  if (p.ray_tlo_dev != nullptr) hipLaunchKernelGGL((occluded_masked_kernel<true>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga);
  else hipLaunchKernelGGL((occluded_masked_kernel<false>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga);
  return hipGetLastError();
}

template <bool RANGED, bool PRUNED>
static hipError_t launch_nearest_masked_cap(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist, int k,
                                            int exact_depth, int32_t *count, int32_t *index, float *gap, hipStream_t stream) {
#define RT_NEAREST_MASKED(CAP)                                                                                                                     \
  hipLaunchKernelGGL((nearest_masked_kernel<RANGED, PRUNED, CAP>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga, pts, max_dist_dev, max_dist, k, \
                     exact_depth, count, index, gap)
  if (k <= 4) RT_NEAREST_MASKED(4);
  else if (k <= 8) RT_NEAREST_MASKED(8);
  else if (k <= 16) RT_NEAREST_MASKED(16);
  else RT_NEAREST_MASKED(32);
#undef RT_NEAREST_MASKED
  return hipGetLastError();
}

hipError_t launch_nearest_spheres_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist, int k,
                                         int exact_depth, int32_t *count, int32_t *index, float *gap, hipStream_t stream) {
  if (p.nrays <= 0) return hipSuccess;
  if (!group_args_ok(p, ga) || pts == nullptr || k < 1 || k > kNearestMaxK) return hipErrorInvalidValue;
  if (count == nullptr && index == nullptr && gap == nullptr) return hipErrorInvalidValue;
  const bool ranged = max_dist_dev != nullptr, pruned = count == nullptr;
  if (!ranged && !max_dist_ok(max_dist)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  if (ranged) return pruned ? launch_nearest_masked_cap<true, true>(p, ga, pts, max_dist_dev, 0.0f, k, exact_depth, count, index, gap, stream)
                            : launch_nearest_masked_cap<true, false>(p, ga, pts, max_dist_dev, 0.0f, k, exact_depth, count, index, gap, stream);
  return pruned ? launch_nearest_masked_cap<false, true>(p, ga, pts, nullptr, max_dist, k, exact_depth, count, index, gap, stream)
                : launch_nearest_masked_cap<false, false>(p, ga, pts, nullptr, max_dist, k, exact_depth, count, index, gap, stream);
}

hipError_t launch_within_count_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist,
                                      const int32_t *first_dev, int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, false, offsets, scratch, 0, true, stream, &rc)) return rc;
  if (!group_args_ok(p, ga) || !within_args_ok(p, pts, max_dist_dev, max_dist, false)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((within_masked_kernel<false>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga, pts, max_dist_dev, max_dist, first_dev, exact_depth,
                     reinterpret_cast<int32_t *>(scratch), nullptr, (int64_t)0, nullptr, nullptr, nullptr);
  return launch_count_scan(scratch, p.nrays, offsets, stream);
}

hipError_t launch_within_fill_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist,
                                     const int32_t *first_dev, int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                     int32_t *point, hipStream_t stream) {
  hipError_t rc;
  if (csr_answered(p, true, offsets, nullptr, capacity, index != nullptr || gap != nullptr || point != nullptr, stream, &rc)) return rc;
  if (!group_args_ok(p, ga) || !within_args_ok(p, pts, max_dist_dev, max_dist, false)) return hipErrorInvalidValue;
  max_dist += 0.0f;   // (-0.0 -> +0.0)
  hipLaunchKernelGGL((within_masked_kernel<true>), lane_grid(p.nrays), dim3(64), 0, stream, p, ga, pts, max_dist_dev, max_dist, first_dev, exact_depth,
                     nullptr, offsets, capacity, index, gap, point);
  return hipGetLastError();
}

// The derive: the caller-order words gathered into L order, then the exact subtree OR of every inner node, twice -- in the canonical numbering
// (left / right / parent: what rt_prepared_get_groups hands out) and in the traversal numbering (p.nodes: what the walks index).  Each is ONE
// launch of group_climb (query_core.h) over words zeroed on the stream ahead of it: inner node v seeds the combine of its leaf children's
// words and climbs the parents with relaxed agent-scope atomic ORs, carrying on only with the bits it newly set.  Vector atomics only, no
// workgroup waits on another, and the result does not depend on the tree's height (63 levels are as exact as 3).  The traversal records hold
// no parent: groups_parents_kernel writes one from the child references first (every inner node but the root is the child of exactly one).
// Every index read from memory is checked against the scene's sizes before it is used as one.
struct GroupOps {
  uint32_t *words;
  const int32_t *up;
  int n_nodes;
  __device__ __forceinline__ uint32_t fetch_or(int32_t v, uint32_t bits) const {
    return __hip_atomic_fetch_or(&words[v], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ int32_t parent(int32_t v) const {
    const int32_t u = up[v];
    return u < n_nodes ? u : -1;
  }
};
__global__ __launch_bounds__(256) void groups_gather_kernel(const int32_t *ids, const uint32_t *caller_words, int n, uint32_t *groups) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = ids[i];
  groups[i] = c >= 0 && c < n ? caller_words[c] : 0u;
}
__global__ __launch_bounds__(256) void groups_parents_kernel(const float4 *nodes, int n_nodes, int32_t *trav_parent) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_nodes) return;
  const int kids[2] = {f2i(nodes[2 * (size_t)v].w), f2i(nodes[2 * (size_t)v + 1].w)};
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (kids[k] > 0 && kids[k] < n_nodes) trav_parent[kids[k]] = v;   // (the root, 0, is nobody's child: its word stays -1)
}
// TRAV: children from the traversal records (a leaf is ~j); else from the canonical left / right (a leaf is -2 - j)
template <bool TRAV>
__global__ __launch_bounds__(256) void groups_climb_kernel(const float4 *nodes, const int32_t *left, const int32_t *right, const int32_t *up, int n_nodes,
                                                           const uint32_t *groups, uint32_t *words) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_nodes) return;
  int kids[2];
  if constexpr (TRAV) {
    kids[0] = f2i(nodes[2 * (size_t)v].w);
    kids[1] = f2i(nodes[2 * (size_t)v + 1].w);
  } else {
    kids[0] = left[v] <= -2 ? ~(-2 - left[v]) : 0;   // (an inner child contributes through its own climb)
    kids[1] = right[v] <= -2 ? ~(-2 - right[v]) : 0;
  }
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = ~kids[k];
    if (kids[k] < 0 && j <= n_nodes) w[k] = groups[j];   // (n = n_nodes + 1 spheres)
  }
  group_climb(GroupOps{words, up, n_nodes}, v, group_combine(w[0], w[1]));
}

size_t groups_bytes(int64_t n) {
  const size_t words = ((size_t)n * 4 + 255) & ~(size_t)255;
  return 5 * words;
}
GroupBlock groups_carve(char *block, int64_t n) {
  const size_t words = ((size_t)n * 4 + 255) & ~(size_t)255;
  GroupBlock b;
  b.caller = reinterpret_cast<uint32_t *>(block);
  b.groups = reinterpret_cast<uint32_t *>(block + words);
  b.node_groups = reinterpret_cast<uint32_t *>(block + 2 * words);
  b.trav_groups = reinterpret_cast<uint32_t *>(block + 3 * words);
  b.trav_parent = reinterpret_cast<int32_t *>(block + 4 * words);
  return b;
}
hipError_t launch_groups_derive(const GroupBlock &b, const int32_t *ids, const float4 *nodes, const int32_t *left, const int32_t *right,
                                const int32_t *parent, int n, hipStream_t stream) {
  if (n < 2 || b.caller == nullptr || ids == nullptr || nodes == nullptr || left == nullptr || right == nullptr || parent == nullptr)
    return hipErrorInvalidValue;
  const int ni = n - 1;
  const size_t words = ((size_t)n * 4 + 255) & ~(size_t)255;
  hipError_t e = hipMemsetAsync(b.node_groups, 0, 2 * words, stream);   // (both numberings' words: adjacent)
  if (e == hipSuccess) e = hipMemsetAsync(b.trav_parent, 0xff, words, stream);
  if (e != hipSuccess) return e;
  const dim3 block(256), gn(((unsigned)n + 255u) / 256u), gi(((unsigned)ni + 255u) / 256u);
  hipLaunchKernelGGL(groups_gather_kernel, gn, block, 0, stream, ids, b.caller, n, b.groups);
  hipLaunchKernelGGL(groups_parents_kernel, gi, block, 0, stream, nodes, ni, b.trav_parent);
  hipLaunchKernelGGL((groups_climb_kernel<false>), gi, block, 0, stream, nodes, left, right, parent, ni, b.groups, b.node_groups);
  hipLaunchKernelGGL((groups_climb_kernel<true>), gi, block, 0, stream, nodes, left, right, b.trav_parent, ni, b.groups, b.trav_groups);
  return hipGetLastError();
}

}  // namespace rtk
