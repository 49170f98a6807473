// query_device.hpp -- launcher declarations and constants of the caller queries (host <-> query_kernels.hip).  The parameter block
// (KParams) and everything the render path launches stay in rt_device.hpp.
#pragma once
#include "rt_device.hpp"

namespace rtk {

// rt_occluded_rays's lane kernel (query_kernels.hip), each lane leaving its traversal at its first accepted sphere
hipError_t launch_occluded_rays(const KParams &p, hipStream_t stream);
// objs_hit bvh r t_min t_max of n rays (ray.fut:76-86): index[i] = the winning leaf or -1, hit7 (may be nullptr) = {t, p.xyz, normal.xyz}
hipError_t launch_intersect_rays(const KParams &p, float t_min, float t_max, int32_t *index, float *hit7, hipStream_t stream);
// ... the two lane kernels with ray i's interval from (p.ray_tlo_dev[i], p.ray_thi_dev[i]) (both non-null)
hipError_t launch_intersect_rays_ranged(const KParams &p, int32_t *index, float *hit7, hipStream_t stream);
hipError_t launch_occluded_rays_ranged(const KParams &p, hipStream_t stream);
// rt_multi_hit_rays[_ranged]: the first k (1 <= k <= kMultiHitMaxK) crossings of each ray in (t, j, root) order and their count, one lane per
// ray: count[i], index / root [i * k + s], hit7 [(i * k + s) * 7 ..] (any may be nullptr, not all).  The interval: (p.ray_tlo, p.ray_thi), or
// ray i's own with p.ray_tlo_dev / p.ray_thi_dev (both set, or neither)
constexpr int kMultiHitMaxK = 32;
hipError_t launch_multi_hit_rays(const KParams &p, int k, int32_t *count, int32_t *index, uint8_t *root, float *hit7, hipStream_t stream);
// rt_nearest_spheres[_ranged]: for p.nrays points (pts: n x 3 float32) the first k (1 <= k <= kNearestMaxK) spheres of L by (gap, j) with
// gap <= max_dist -- or point i's own max_dist_dev[i] when max_dist_dev is set -- and their count: count[i], index / gap [i * k + s] (any may
// be nullptr, not all).  count == nullptr: the pruned walk (the k-th gap so far narrows the threshold).  Boxes are tested at depth >=
// exact_depth only: the nodes whose boxes provably contain their subtrees (api_queries.cpp: nearest_entry)
constexpr int kNearestMaxK = 32;
hipError_t launch_nearest_spheres(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, int k, int exact_depth,
                                  int32_t *count, int32_t *index, float *gap, hipStream_t stream);
// rt_spheres_within_* / rt_contact_pairs_*: for p.nrays points EVERY sphere of L with gap <= the point's bound and j >= first_dev[i] (nullptr: no
// lower index bound), as n + 1 int64 offsets and rows in ascending j.  launch_within_count: the count kernel (n int32 counts at `scratch`,
// within_scratch_bytes(n) bytes of device memory) and the three launches of the scan, offsets[0 .. n]; p.nrays == 0 writes offsets[0] = 0.
// launch_within_fill: entry offsets[i] + rank -> index / gap / point (any may be nullptr, not all), only below offsets[i + 1] and `capacity`.
// self: the contact pairs -- point i is the centre of L[i] (p.nrays == p.n_sph), its bound fl(radius_i + max_dist), first = i + 1, and `point` is
// the pair array, rows {i, j} (index must be nullptr).  Boxes are tested at depth >= exact_depth only, as launch_nearest_spheres.
size_t within_scratch_bytes(int64_t n);
hipError_t launch_within_count(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev, bool self,
                               int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream);
hipError_t launch_within_fill(const KParams &p, const float *pts, const float *max_dist_dev, float max_dist, const int32_t *first_dev, bool self,
                              int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point,
                              hipStream_t stream);
// rt_contact_clusters: the connected components of the graph whose edges are launch_within_fill's self rows at the same margin, for the
// p.n_sph >= 1 spheres of the scene: root[i] = the smallest index of i's component (the union-find's parent array, in place), cluster[i] = the
// rank of root[i] among the roots, size[i] = the component's sphere count, *num = the number of components (each but root may be nullptr;
// num needs only 4-byte alignment).  scratch: clusters_scratch_bytes(n) bytes, needed when cluster or num is asked for (the root flags, the
// scan's block sums and its n + 1 offsets).  p.n_sph == 1 launches no walk (such a scene has no node).
size_t clusters_scratch_bytes(int64_t n);
hipError_t launch_contact_clusters(const KParams &p, float margin, int exact_depth, char *scratch, int32_t *root, int32_t *cluster, int32_t *size,
                                   int64_t *num, hipStream_t stream);
// rt_spheres_in_boxes_*: for p.nrays boxes (boxes: n x 6 float32, {lo.xyz, hi.xyz}, 4-byte aligned) EVERY sphere of L with box_gap <= the box's
// margin -- `margin`, or box i's own margin_dev[i] -- and j >= first_dev[i], in the range queries' CSR form and two passes: the same scratch
// (within_scratch_bytes(n)), scan, capacity guard and exact_depth rule as launch_within_count / launch_within_fill.
hipError_t launch_boxes_count(const KParams &p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev, int exact_depth,
                              char *scratch, int64_t *offsets, hipStream_t stream);
hipError_t launch_boxes_fill(const KParams &p, const float *boxes, const float *margin_dev, float margin, const int32_t *first_dev, int exact_depth,
                             const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point, hipStream_t stream);
// rt_spheres_in_planes_*: for p.nrays queries of `nplanes` planes each (planes: n x nplanes x 4 float32, rows {a, b, c, d}, 4-byte aligned;
// 1 <= nplanes <= kMaxPlanes, else hipErrorInvalidValue) EVERY sphere of L with plane_gap <= the query's margin and j >= first_dev[i]: the box
// queries' CSR form, two passes, scratch, scan, capacity guard and exact_depth rule (launch_boxes_count / launch_boxes_fill).
constexpr int kMaxPlanes = 8;
hipError_t launch_planes_count(const KParams &p, const float *planes, int nplanes, const float *margin_dev, float margin, const int32_t *first_dev,
                               int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream);
hipError_t launch_planes_fill(const KParams &p, const float *planes, int nplanes, const float *margin_dev, float margin, const int32_t *first_dev,
                              int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap, int32_t *point,
                              hipStream_t stream);
// rt_sweep_spheres[_ranged]: the first k (1 <= k <= kSweepMaxK) contacts of a sphere moving along each ray, in (tau, j) order, and their count,
// one lane per query: count[i], index / start [i * k + s], hit7 [(i * k + s) * 7 ..] (any may be nullptr, not all).  radius_dev == nullptr:
// the radius `radius` (0 <= radius <= 1e9) and the interval (p.ray_tlo, p.ray_thi) for every query; otherwise query i's own radius_dev[i]
// and (p.ray_tlo_dev[i], p.ray_thi_dev[i]) (all three set, or none).  exclude: nullptr, or n sphere indices skipped at the leaf
constexpr int kSweepMaxK = 32;
hipError_t launch_sweep_spheres(const KParams &p, const float *radius_dev, float radius, const int32_t *exclude, int k, int32_t *count,
                                int32_t *index, uint8_t *start, float *hit7, hipStream_t stream);
// rt_spheres_along_rays_*: for p.nrays queries (p.rays: n x 6 float32) EVERY sphere rt_sweep_spheres_ranged would count -- the widened box test
// on every node, sweep_contact at the leaf, j != exclude[i] -- and j >= first_dev[i], in the range queries' CSR form and two passes: the same
// scratch (within_scratch_bytes(n)), scan and capacity guard as launch_within_count / launch_within_fill, rows in ascending j.  radius_dev
// nullptr: `radius` for every query; tlo_dev / thi_dev both nullptr: (t_min, t_max) for every query, else both set (a scalar that is used and
// fails its rule: hipErrorInvalidValue).  exclude / first_dev: nullptr, or n int32.  The entry arrays: index, roots (rows {t1, t2} of the
// sphere (c, r + rq), unclamped), start (0 entry contact, 1 overlap at the start), query (the row number) -- any may be nullptr, not all.
hipError_t launch_along_count(const KParams &p, const float *radius_dev, float radius, const float *tlo_dev, const float *thi_dev, float t_min,
                              float t_max, const int32_t *exclude, const int32_t *first_dev, char *scratch, int64_t *offsets, hipStream_t stream);
hipError_t launch_along_fill(const KParams &p, const float *radius_dev, float radius, const float *tlo_dev, const float *thi_dev, float t_min,
                             float t_max, const int32_t *exclude, const int32_t *first_dev, const int64_t *offsets, int64_t capacity,
                             int32_t *index, float *roots, uint8_t *start, int32_t *query, hipStream_t stream);
// rt_trace_paths[_shaped]: the bounce chain of each ray (ray_colour with objs_hit r 0 1e9, up to max_depth >= 0 vertices): count[i], end[i]
// (kPathEscaped / kPathAbsorbed / kPathTruncated, query_core.h), the first min(count, k) vertices at index [i * k + s] and hit7
// [(i * k + s) * 7 ..] (1 <= k <= kPathsMaxK; padded with -1 and seven zeros), light3 / last_ray6 / colour3 [i]: the loop variables at exit
// (any may be nullptr, not all).  One wave per `per_wave` consecutive rays (a multiple of 64 in [64, kPathsMaxPerWave]): its lanes refill
// from the block in-wave.  paths_auto_per_wave: the launch shape of rt_trace_paths (fitted to the measured sweep)
constexpr int kPathsMaxK = 1024, kPathsMaxPerWave = 4096;
constexpr int kPathsWavesPerCu = 8, kPathsAutoCap = 256;
inline int paths_auto_per_wave(int64_t n, int num_cu) {
  const int64_t waves = (int64_t)kPathsWavesPerCu * (num_cu > 0 ? num_cu : 1);
  if (n <= 64 * waves) return 64;
  const int64_t per = ((n + waves - 1) / waves + 63) / 64 * 64;
  return (int)(per < kPathsAutoCap ? per : kPathsAutoCap);
}
hipError_t launch_trace_paths(const KParams &p, int max_depth, int k, int per_wave, int32_t *count, uint8_t *end, int32_t *index, float *hit7,
                              float *light3, float *last_ray6, float *colour3, hipStream_t stream);
// rt_visible_pairs[_shaped]: p.nrays points (points: n x 3 float32) against m targets or directions (targets: m x 3 float32; both 4-byte
// aligned), 1 <= m <= kPairsMaxTargets, n * words < 2^31 with words = (m + 63) / 64: visible[i * words + (j >> 6)] bit j & 63 = pair (i, j)
// is valid and rt_occluded_rays's predicate over (t_min, t_max) is false for its ray; count[i] = the set bits of row i (either may be nullptr,
// not both).  words_per_wave >= 1: one wave per point and run of that many words (above `words`: the whole row); where a row is cut into
// several runs, count is zeroed on the stream ahead of the kernel and the waves add to it.  words_per_wave == kPairsPacked (m <=
// kPairsPackedMax only): one wave per 64 / G consecutive points, G the least power of two >= m.  The shape changes no bit.
// pairs_auto_words_per_wave: the launch shape of rt_visible_pairs, fitted to the measured sweeps.  Short rows are packed: with
// a point per wave, 16 targets leave 48 lanes without a pair (measured 2.5 x the time of the packed shape's).  Otherwise a row is cut into
// runs of at most kPairsAutoCap words (runs of 8 or 16 were the fastest where the points alone fill the machine; the whole row of 256 words
// as one run was 12 x slower on 256 points), and into more and shorter runs, down to one word, until the grid has kPairsWavesPerCu waves per
// CU -- about six rounds of the 10 waves a CU holds (16 KB of LDS stack each): runs of 2 or 4 words were the fastest on 256 points x 256 words.
constexpr int kPairsMaxTargets = 1 << 24;
constexpr int kPairsPacked = 0, kPairsPackedMax = 32;
constexpr int kPairsWavesPerCu = 64, kPairsAutoCap = 8;
inline int pairs_auto_words_per_wave(int64_t n, int64_t m, int num_cu) {
  if (m <= kPairsPackedMax) return kPairsPacked;
  const int64_t words = (m + 63) / 64;
  const int64_t waves = (int64_t)kPairsWavesPerCu * (num_cu > 0 ? num_cu : 1);
  int64_t chunks = (words + kPairsAutoCap - 1) / kPairsAutoCap;
  const int64_t fill = (waves + n - 1) / (n > 0 ? n : 1);
  if (chunks < fill) chunks = fill < words ? fill : words;
  return (int)((words + chunks - 1) / chunks);
}
hipError_t launch_visible_pairs(const KParams &p, const float *points, const float *targets, int m, bool directions, int words_per_wave,
                                float t_min, float t_max, unsigned long long *visible, int32_t *count, hipStream_t stream);
// Sphere groups (rt_prepared_set_groups, rt_*_masked).  GroupArgs: what a masked launch takes on top of its unmasked twin's
// arguments -- the scene's group words in L order (n), the exact subtree ORs of the inner nodes in the TRAVERSAL numbering (n - 1: the
// numbering of p.nodes' child references), and the mask: mask_dev[i] of query i when given (n 4-byte-aligned words), else `mask`.  They are
// kernel arguments of their own: KParams belongs to the render path.  Query i sees sphere j iff groups[j] & mask_i != 0; a mask of 0 starts no
// walk.  Each launcher otherwise is its unmasked twin (the ranged forms are selected as there: p.ray_tlo_dev / max_dist_dev set).
struct GroupArgs {
  const uint32_t *groups, *node_groups, *mask_dev;
  uint32_t mask;
};
hipError_t launch_intersect_rays_masked(const KParams &p, const GroupArgs &ga, float t_min, float t_max, int32_t *index, float *hit7,
                                        hipStream_t stream);
hipError_t launch_occluded_rays_masked(const KParams &p, const GroupArgs &ga, hipStream_t stream);
hipError_t launch_nearest_spheres_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist, int k,
                                         int exact_depth, int32_t *count, int32_t *index, float *gap, hipStream_t stream);
hipError_t launch_within_count_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist,
                                      const int32_t *first_dev, int exact_depth, char *scratch, int64_t *offsets, hipStream_t stream);
hipError_t launch_within_fill_masked(const KParams &p, const GroupArgs &ga, const float *pts, const float *max_dist_dev, float max_dist,
                                     const int32_t *first_dev, int exact_depth, const int64_t *offsets, int64_t capacity, int32_t *index, float *gap,
                                     int32_t *point, hipStream_t stream);
// The groups' device block of a scene of n spheres (groups_bytes(n) bytes, 256-byte aligned pieces): the caller-order words, then what
// launch_groups_derive makes of them for one tree -- the words in L order (groups[i] = caller[ids[i]]), the subtree ORs in the canonical
// numbering (left / right / parent) and in the traversal numbering (nodes), and the traversal numbering's parent array it climbs.
struct GroupBlock {
  uint32_t *caller = nullptr, *groups = nullptr, *node_groups = nullptr, *trav_groups = nullptr;
  int32_t *trav_parent = nullptr;
};
size_t groups_bytes(int64_t n);
GroupBlock groups_carve(char *block, int64_t n);
hipError_t launch_groups_derive(const GroupBlock &b, const int32_t *ids, const float4 *nodes, const int32_t *left, const int32_t *right,
                                const int32_t *parent, int n, hipStream_t stream);
// the primary rays of an h x w frame through p.cam (get_ray at pixel_u / pixel_v), row-major from the top row: rays[6 (row w + col) ..]
hipError_t launch_camera_rays(const Cam &cam, int h, int w, float *rays, hipStream_t stream);

}  // namespace rtk
