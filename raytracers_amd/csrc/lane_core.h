// lane_core.h -- per-lane arithmetic of the render hot path, shared by every kernel
// family (render_kernels.hip) and by the host-side wave simulator (tools/wavesim.cpp,
// a design tool that executes the same per-lane code with 64 emulated lanes).
//
// Parity contract: IEEE binary32, no FMA contraction (build with
// -ffp-contract=off), correctly rounded / and sqrt, fmaxf/fminf NaN semantics, and the
// reference's operation order.  Each function cites the Futhark lines it follows.
//
// What is NOT taken from the reference is the traversal ORDER.  bvh_fold
// (futhark/bvh.fut:61-84) walks parent pointers and meets leaves in increasing index
// order; here a leaf is tested iff every ancestor box passes aabb_hit with the FIXED
// interval (0, 1e9) (ray.fut:77 closes over the outer t_max), and the winner is the
// smallest accepted root, ties to the lowest leaf index -- the same (j, t) the fold
// returns, for any visiting order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace rtk {

constexpr float kTMax = 1000000000.0f;   // ray.fut:130
constexpr float kEps = 0.1f;             // scene_epsilon, ray.fut:3
constexpr float kNoHit = __builtin_inff();

struct Cam {   // camera (ray.fut:88-91) as 12 floats
  float ox, oy, oz, lx, ly, lz, hx, hy, hz, vx, vy, vz;
};

struct Ray {
  float ox, oy, oz;
  float dx, dy, dz;
  float ix, iy, iz;   // 1/d per axis: aabb_hit's invD (ray.fut:55) depends on the ray only
  float a;            // dot d d: sphere_hit's `a` (ray.fut:34) and norm's argument (prim.fut:26)
};

RT_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) {   // prim.fut:22-24
  float px = ax * bx, py = ay * by, pz = az * bz;
  return (px + py) + pz;
}

RT_HD void ray_derive(Ray &r) {
  r.ix = 1.0f / r.dx;
  r.iy = 1.0f / r.dy;
  r.iz = 1.0f / r.dz;
  r.a = dot3(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz);
}

// trace_ray + get_ray (ray.fut:150-154, :109-114).  `col` = i, `row` = image row from
// the top; the reference evaluates pixel (j = row) at v = (height - j) / height.
RT_HD float pixel_u(int col, int width) { return (float)col / (float)width; }
RT_HD float pixel_v(int row, int height) { return (float)(height - row) / (float)height; }

// get_ray for precomputed (u, v): the pooled kernel reads u and v from per-column / per-row
// tables the host fills with pixel_u / pixel_v (two correctly rounded divisions per pixel
// become two loads; the values are the same bits).
RT_HD void primary_dir_uv(const Cam &c, float u, float v, Ray &r) {   // origin + direction only
  r.ox = c.ox; r.oy = c.oy; r.oz = c.oz;
  r.dx = ((c.lx + u * c.hx) + v * c.vx) - c.ox;
  r.dy = ((c.ly + u * c.hy) + v * c.vy) - c.oy;
  r.dz = ((c.lz + u * c.hz) + v * c.vz) - c.oz;
}

RT_HD Ray primary_ray(const Cam &c, int col, int row, int width, int height) {
  const float u = pixel_u(col, width);
  const float v = pixel_v(row, height);
  Ray r;
  r.ox = c.ox; r.oy = c.oy; r.oz = c.oz;
  r.dx = ((c.lx + u * c.hx) + v * c.vx) - c.ox;
  r.dy = ((c.ly + u * c.hy) + v * c.vy) - c.oy;
  r.dz = ((c.lz + u * c.hz) + v * c.vz) - c.oz;
  ray_derive(r);
  return r;
}

// aabb_hit (ray.fut:53-70) with tmin0 = 0, tmax0 = 1e9.
//
// The reference tests `tmax_k <= tmin_k -> false` after each of the x, y, z slabs.  Only
// the last test is evaluated here, which is the same predicate: fmax/fmin return the
// non-NaN operand, so starting from the finite (0, 1e9) no tmin_k/tmax_k is ever NaN,
// tmin_1 <= tmin_2 <= tmin_3 and tmax_1 >= tmax_2 >= tmax_3; hence tmax_3 > tmin_3 implies
// tmax_k > tmin_k for k = 1, 2, and a failed earlier test implies tmax_3 <= tmin_3.
// (The per-axis swap on `invD < 0` must stay a select: with a zero direction component,
// 0 * inf = NaN bounds arise that min/max-based swapping would treat differently.)
typedef float rt_f2 __attribute__((vector_size(8)));
// box_hit_clamped's `tclamp`: the interval's upper end (lower end 0).  kTMax gives aabb_hit itself (box_hit below); the CULL instantiations of the pooled kernel pass
// min(kTMax, a proven lower bound on every sphere root the box's subtree could still contribute) -- see cull_limit.
// box_hit_interval: aabb_hit box r tlo thi with the caller's interval (rt_intersect_rays); tlo, thi finite, tlo <= thi.
RT_HD bool box_hit_interval(const Ray &r, float lox, float loy, float loz, float hix, float hiy, float hiz, float tlo, float thi) {
  // x and y as a pair: two packed subtracts + two packed multiplies (v_pk_add/mul_f32 round
  // each lane exactly like the scalar instructions)
  const rt_f2 o2 = {r.ox, r.oy}, i2 = {r.ix, r.iy};
  const rt_f2 lo2 = {lox, loy}, hi2 = {hix, hiy};
  const rt_f2 t0 = (lo2 - o2) * i2, t1 = (hi2 - o2) * i2;
  const float t0z = (loz - r.oz) * r.iz, t1z = (hiz - r.oz) * r.iz;
  const bool nx = r.ix < 0.0f, ny = r.iy < 0.0f, nz = r.iz < 0.0f;
  float tmin = fmaxf(nx ? t1[0] : t0[0], tlo);
  float tmax = fminf(nx ? t0[0] : t1[0], thi);
  tmin = fmaxf(ny ? t1[1] : t0[1], tmin);
  tmax = fminf(ny ? t0[1] : t1[1], tmax);
  tmin = fmaxf(nz ? t1z : t0z, tmin);
  tmax = fminf(nz ? t0z : t1z, tmax);
  return !(tmax <= tmin);
}
// box_hit_interval for a caller that holds the bounds already ORDERED by the ray's signs: near_k = (r.i_k < 0 ? hi_k : lo_k), far_k the
// other one.  Bit-equal to box_hit_interval on the same box in every case: `nx ? t1 : t0` picks between two products, each of which is a
// function of its own operands alone -- (lo - o) * i or (hi - o) * i, one IEEE subtraction and one IEEE multiplication (no contraction) --
// so computing only the picked product from the picked operand, ((nx ? hi : lo) - o) * i, gives the same bits, NaN products (0 * inf:
// the origin on a slab of a zero direction component) and their payloads included.  The select still happens on `i_k < 0` (sign_offsets
// below), never through min / max, and the fmaxf / fminf chain is box_hit_interval's in its order.  What moves is WHERE the select is
// made: once per ray, as a choice of addresses, instead of six v_cndmask per box (the pooled kernel's LDS-resident instantiation).
RT_HD bool box_hit_presorted(const Ray &r, float nx, float fx, float ny, float fy, float nz, float fz, float tlo, float thi) {
  float tmin = fmaxf((nx - r.ox) * r.ix, tlo);
  float tmax = fminf((fx - r.ox) * r.ix, thi);
  tmin = fmaxf((ny - r.oy) * r.iy, tmin);
  tmax = fminf((fy - r.oy) * r.iy, tmax);
  tmin = fmaxf((nz - r.oz) * r.iz, tmin);
  tmax = fminf((fz - r.oz) * r.iz, tmax);
  return !(tmax <= tmin);
}
// The ray's three selects as one word: bit 3 / 4 / 5 set iff i_x / i_y / i_z < 0.0f (true for -inf and every negative finite value; false
// for +-0, +inf and NaN -- box_hit_interval's own condition).  The bits are the BYTE distances between a record's lo and hi entries of
// that axis in the sign-ordered node layout (render_kernels.hip, PRESORT): near_k is read at `entry_k + (w & d_k)`, far_k at
// `entry_k + d_k - (w & d_k)` (= `entry_k + ((w ^ kSignAll) & d_k)`).
constexpr uint32_t kSignX = 8u, kSignY = 16u, kSignZ = 32u, kSignAll = kSignX | kSignY | kSignZ;
RT_HD uint32_t sign_offsets(const Ray &r) {
  return (r.ix < 0.0f ? kSignX : 0u) | (r.iy < 0.0f ? kSignY : 0u) | (r.iz < 0.0f ? kSignZ : 0u);
}
// The sign-ordered node record: 14 dwords in seven 8-byte entries {left child's value, right child's value}; the lo and hi entries of an
// axis lie d_k = 8 / 16 / 32 bytes apart (x / y / z), the child references take the entry that is left over:
//   byte  0 z lo | 8 y lo | 16 refs | 24 y hi | 32 z hi | 40 x lo | 48 x hi
// Seven entries make the record's stride an ODD number of 8-byte bank pairs: the ds_read_b64 of 32 lanes on 32 different records are
// conflict-free whichever records they are consecutive in, and random records spread over all 32 pairs (a 64-byte stride: over four).
constexpr int kPsNodeBytes = 56, kPsX = 40, kPsY = 8, kPsZ = 0, kPsRefs = 16;
// (the work items of the instantiations that use it: the record's byte offset -- a multiple of 8 -- from bit 11, the ray's sign_offsets << 5 in
// bits 8 .. 10, the slot * 4 below)
constexpr int kPsItemShift = 11;
constexpr uint32_t kPsItemLow = 0x7fcu;
RT_HD void presort_pack(uint32_t *cell, const float *lo_l, const float *hi_l, const float *lo_r, const float *hi_r, uint32_t ref_l, uint32_t ref_r) {
  auto put = [&](int byte, float l, float r) {
    __builtin_memcpy(cell + byte / 4, &l, 4);
    __builtin_memcpy(cell + byte / 4 + 1, &r, 4);
  };
  put(kPsX, lo_l[0], lo_r[0]); put(kPsX + (int)kSignX, hi_l[0], hi_r[0]);
  put(kPsY, lo_l[1], lo_r[1]); put(kPsY + (int)kSignY, hi_l[1], hi_r[1]);
  put(kPsZ, lo_l[2], lo_r[2]); put(kPsZ + (int)kSignZ, hi_l[2], hi_r[2]);
  cell[kPsRefs / 4] = ref_l; cell[kPsRefs / 4 + 1] = ref_r;
}
RT_HD bool box_hit_clamped(const Ray &r, float lox, float loy, float loz, float hix, float hiy, float hiz, float tclamp) {
  return box_hit_interval(r, lox, loy, loz, hix, hiy, hiz, 0.0f, tclamp);
}
RT_HD bool box_hit(const Ray &r, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  return box_hit_clamped(r, lox, loy, loz, hix, hiy, hiz, kTMax);
}

// ---- culling by the best hit so far (the CULL instantiations of the pooled kernel) -------------------------
// The reference's fold tests every leaf whose ancestors' boxes pass with the FIXED interval (0, 1e9) (ray.fut:77) -- it never
// narrows the interval.  Only its RESULT is the contract: the smallest accepted root, ties to the lowest leaf.  A subtree may
// therefore be skipped when every root any of its spheres could produce is proven LARGER than a root already found.
//
// The bound (proof and constants: DESIGN.md 3.4; tools/cull_bound_check.cpp hammers the two inequalities it rests on).  For a
// ray (o, d) and a sphere (p, r) let g be ANY root sphere_root computes in binary32, P = o + g d the exact point at that
// parameter, D = |o - p|, a = d.d.  Then
//     | |P - p|^2 - r^2 |  <=  2^-18 (D^2 + r^2)                                                     (E1)
// i.e. P lies within rho = 2^-18 (D^2 / r + r) of the sphere, hence inside any box that contains the sphere's binary32 box
// (pos -+ r, rounded: off by at most 2^-24 max|coordinate|) widened by rho' = rho + 2^-24 C_max on every side, hence
//     g  >=  tmin(box) (1 - 3.01 * 2^-24)  -  rho' max_k |1 / d_k|                                   (E2)
// with tmin the entry parameter box_hit computes.  With g <= best (only such a root could matter), D <= 2 (a best^2 + r^2)^(1/2)
// under the scene guard of cull_scene_constants, and the right-hand side exceeds `best` whenever
//     tmin  >=  best + W2 (best^2 + kappa),    W2 = max_k |1 / d_k| * a * c2
// c2 and kappa being per-scene constants.  A box is tested against min(kTMax, that limit) instead of kTMax: one instruction
// stream, and a box that fails only against the limit is a subtree whose every root is > best -- it cannot win or tie.
// Requires every box to contain the boxes of the spheres below it (tree height <= the reference's number of sweeps).
constexpr float kCullALo = 1.0f / 64.0f, kCullAHi = 1048576.0f;   // a = d.d outside [2^-6, 2^20]: the ray is not culled
RT_HD float cull_weight(const Ray &r, float c2) {                 // W2 of a ray (inf: never cull)
  const float m = fmaxf(fmaxf(fabsf(r.ix), fabsf(r.iy)), fabsf(r.iz));
  return (r.a >= kCullALo && r.a <= kCullAHi) ? m * r.a * c2 : kNoHit;
}
RT_HD float cull_limit(float best, float w2, float kappa) {       // the interval's upper end for a slot whose best root is `best`
  return fminf(__builtin_fmaf(w2, __builtin_fmaf(best, best, kappa), best), kTMax);
}

// ---- the leaf's own box (the pooled kernel's BOX / BOX2 append a leaf child only if it passes) ------------
// The record of an inner node has a box slot for either child; the slot of a LEAF child holds the sphere's own box widened by
// eps(r) on every side, [p - (r + eps), p + (r + eps)] in binary32, and BOX's test of that slot -- the arithmetic it always ran
// there -- decides whether the sphere is tested at all.  Claim: whenever sphere_root accepts a root g (0.1 < g < 1e9) for a ray
// (o, d) and a sphere (p, r), box_hit / box_hit_presorted pass on that box over (0, 1e9) -- the CULL instantiations never filter.
// With D = |o - p| <= D_eps:
//   (E1)  | |P - p|^2 - r^2 | <= 2^-18 (D^2 + r^2) for P = o + g d, so P lies at most r (sqrt(1 + phi) - 1) <= rho / 2 OUTSIDE
//         the sphere, rho = 2^-18 (D^2 / r + r), phi = rho / r;
//   slab: each of the six products is exact within (1 -+ 2^-24)^3, so the interval computed for a box that holds P with
//         m >= 4 * 2^-24 |P - o| to spare on every side contains g (a NaN slab is skipped, an infinite one has the right sign);
//   corner: fl(p -+ fl(r + eps)) gives away at most 4 * 2^-24 C_max.
// eps(r) = q / r + lin r + abs covers the three with 1 % to spare for its own roundings (rt_host.hpp: leaf_box_finish sets q,
// lin, abs from the scene's statistics and D_eps = 2 (R + r_max); leaf_box_camera_ok admits a launch's cameras).
RT_HD float leaf_box_eps(float rad, float q, float lin, float abs) { return (q / rad + lin * rad) + abs; }
RT_HD void leaf_box_bounds(float px, float py, float pz, float rad, float q, float lin, float abs, float lo[3], float hi[3]) {
  const float rw = rad + leaf_box_eps(rad, q, lin, abs);
  lo[0] = px - rw; lo[1] = py - rw; lo[2] = pz - rw;
  hi[0] = px + rw; hi[1] = py + rw; hi[2] = pz + rw;
}

// The root closest_hit would accept for this sphere if its running t_max were large
// (ray.fut:32-51 called with t_min = 0.1, :79): root1 if root1 > 0.1, else root2 if
// root2 > 0.1, else none.  (root2 >= root1, so "root1 >= t_max, try root2" can never
// succeed; the caller's `g < best` test is then exactly the reference's `temp < t_max`.)
RT_HD float sphere_root(const Ray &r, float px, float py, float pz, float rad) {
  const float ocx = r.ox - px, ocy = r.oy - py, ocz = r.oz - pz;
  const float b = dot3(ocx, ocy, ocz, r.dx, r.dy, r.dz);
  const float c = dot3(ocx, ocy, ocz, ocx, ocy, ocz) - rad * rad;
  const float disc = b * b - r.a * c;
  if (disc <= 0.0f) return kNoHit;
  const float sq = sqrtf(disc);
  float t = (-b - sq) / r.a;
  if (!(t > kEps)) {
    t = (-b + sq) / r.a;
    if (!(t > kEps)) return kNoHit;
  }
  return t;
}

// closest_hit's accumulator update (ray.fut:78-81) made order-independent.
RT_HD void closest_update(float g, int idx, float &best, int &bestj) {
  if (g < best || (g == best && idx < bestj)) {
    best = g;
    bestj = idx;
  }
}

RT_HD int32_t pack_pixel(float r, float g, float b) {   // colour_to_pixel, ray.fut:158-162
  const int32_t ir = (int32_t)(255.99f * r);
  const int32_t ig = (int32_t)(255.99f * g);
  const int32_t ib = (int32_t)(255.99f * b);
  return (ir << 16) | (ig << 8) | ib;
}

// sphere_root plus what the later re-intersection needs to know: *near_root is set when the
// fold took root2 (root1 <= 0.1) although root1 > 0 -- exactly the case in which
// `sphere_hit s r 0.0 (t+1)` (ray.fut:83-85) returns root1 instead of the fold's t.
RT_HD float sphere_root_flag(const Ray &r, float px, float py, float pz, float rad, bool *near_root) {
  const float ocx = r.ox - px, ocy = r.oy - py, ocz = r.oz - pz;
  const float b = dot3(ocx, ocy, ocz, r.dx, r.dy, r.dz);
  const float c = dot3(ocx, ocy, ocz, ocx, ocy, ocz) - rad * rad;
  const float disc = b * b - r.a * c;
  *near_root = false;
  if (disc <= 0.0f) return kNoHit;
  const float sq = sqrtf(disc);
  float t = (-b - sq) / r.a;
  if (!(t > kEps)) {
    *near_root = t > 0.0f;
    t = (-b + sq) / r.a;
    if (!(t > kEps)) return kNoHit;
  }
  return t;
}

// The literal re-intersection of the winning sphere, `sphere_hit s r t_min (best+1)`
// (ray.fut:83-85, :32-51): may pick the OTHER root than the fold did, or none.  ray_colour's
// objs_hit has t_min = 0.0 (rehit_full); rt_intersect_rays passes the caller's.
RT_HD bool rehit_range(const Ray &r, float tlo, float best, float spx, float spy, float spz, float srad, float *t_out) {
  const float ocx = r.ox - spx, ocy = r.oy - spy, ocz = r.oz - spz;
  const float b = dot3(ocx, ocy, ocz, r.dx, r.dy, r.dz);
  const float c = dot3(ocx, ocy, ocz, ocx, ocy, ocz) - srad * srad;
  const float disc = b * b - r.a * c;
  bool have = false;
  float t = 0.0f;
  if (!(disc <= 0.0f)) {
    const float sq = sqrtf(disc);
    const float lim = best + 1.0f;
    t = (-b - sq) / r.a;
    have = (t < lim) && (t > tlo);
    if (!have) {
      t = (-b + sq) / r.a;
      have = (t < lim) && (t > tlo);
    }
  }
  *t_out = t;
  return have;
}
RT_HD bool rehit_full(const Ray &r, float best, float spx, float spy, float spz, float srad, float *t_out) {
  return rehit_range(r, 0.0f, best, spx, spy, spz, srad, t_out);
}

// `sphere_hit s r tlo thi is #some` (ray.fut:32-51): root1 or root2 strictly inside (tlo, thi).  The any-hit
// predicate of rt_occluded_rays -- rehit_range's arithmetic with the caller's upper end, and no t kept.
RT_HD bool sphere_hit_any(const Ray &r, float tlo, float thi, float spx, float spy, float spz, float srad) {
  const float ocx = r.ox - spx, ocy = r.oy - spy, ocz = r.oz - spz;
  const float b = dot3(ocx, ocy, ocz, r.dx, r.dy, r.dz);
  const float c = dot3(ocx, ocy, ocz, ocx, ocy, ocz) - srad * srad;
  const float disc = b * b - r.a * c;
  if (disc <= 0.0f) return false;
  const float sq = sqrtf(disc);
  const float t1 = (-b - sq) / r.a, t2 = (-b + sq) / r.a;
  return ((t1 < thi) && (t1 > tlo)) || ((t2 < thi) && (t2 > tlo));
}

// The interval rule of the queries that take one: 0 <= tlo <= thi <= 1e9.  Three compares, each false on a NaN operand, so NaN and +-inf fail
// too (+inf exceeds 1e9, -inf is below 0).  A per-ray interval is checked with it once, where the ray is loaded: box_hit_interval's
// fmaxf / fminf drop a NaN bound rather than empty the box interval.
RT_HD bool interval_ok(float tlo, float thi) { return (tlo >= 0.0f) & (tlo <= thi) & (thi <= kTMax); }

// Shortcut for the same call when the fold's accepted root `best` is known not to be
// displaced: with near_root clear, root1 (if it was the fold's root) or root2 passes
// `0 < t < best + 1` iff best + 1 > best, and the re-intersection returns t = best.
// Returns false when the caller must run rehit_full instead.
RT_HD bool rehit_is_best(float best, bool near_root) { return !near_root && (best + 1.0f > best); }

// The rest of one ray_colour iteration (ray.fut:126-148, :119-124): scatter or terminate.
// `have`/`t`: result of the re-intersection.  Returns true when the pixel continues with the
// scattered ray: r.o/r.d, light and depth are updated (and, if DERIVE, r's derived fields;
// otherwise the caller runs ray_derive); false when the pixel is finished, after emit(r, g, b)
// was called with ray_colour's result -- the operand of colour_to_pixel.  sph = {pos.xyz},
// col = colour, inv_rad = 1.0f / radius as an IEEE division (tabulated by the host).
// (The absorbed colour is written light * 0: ray_colour's running colour stays (0,0,0) until the
// sky is reached -- the same value for scenes whose colours are not negative.)
// (emit is called in each of the two finishing branches, not once behind them: merging them costs
// the pooled kernels a VGPR.)
template <bool DERIVE, class Emit>
RT_HD bool shade_ray_emit(Ray &r, bool have, float t, float spx, float spy, float spz, float scr, float scg, float scb,
                          float inv_rad, float &lr, float &lg, float &lb, int &depth, int max_depth, Emit &&emit) {
  const float inv_norm = 1.0f / sqrtf(r.a);   // normalise r.dir = scale (1/norm d) d
  if (have) {
    // hit record (ray.fut:40-46)
    const float hpx = r.ox + t * r.dx, hpy = r.oy + t * r.dy, hpz = r.oz + t * r.dz;
    const float nx = inv_rad * (hpx - spx), ny = inv_rad * (hpy - spy), nz = inv_rad * (hpz - spz);
    // scatter (ray.fut:119-124), reflect (ray.fut:116-117)
    const float ux = inv_norm * r.dx, uy = inv_norm * r.dy, uz = inv_norm * r.dz;
    const float k = 2.0f * dot3(ux, uy, uz, nx, ny, nz);
    const float rx = ux - k * nx, ry = uy - k * ny, rz = uz - k * nz;
    if (dot3(rx, ry, rz, nx, ny, nz) > 0.0f && depth + 1 < max_depth) {
      r.ox = hpx; r.oy = hpy; r.oz = hpz;
      r.dx = rx; r.dy = ry; r.dz = rz;
      if (DERIVE) ray_derive(r);
      lr = lr * scr; lg = lg * scg; lb = lb * scb;
      depth = depth + 1;
      return true;
    }
    // absorbed, or the bounce budget is spent: colour = light * (0,0,0)
    emit(lr * 0.0f, lg * 0.0f, lb * 0.0f);
    return false;
  }
  // miss: sky gradient (ray.fut:140-148)
  const float uy = inv_norm * r.dy;
  const float tt = 0.5f * (uy + 1.0f);
  const float w = 1.0f - tt;
  const float sr = w * 1.0f + tt * 0.5f, sg = w * 1.0f + tt * 0.7f, sb = w * 1.0f + tt * 1.0f;
  emit(lr * sr, lg * sg, lb * sb);
  return false;
}

// The render path's form: *pixel = colour_to_pixel of the finished colour.
template <bool DERIVE>
RT_HD bool shade_ray(Ray &r, bool have, float t, float spx, float spy, float spz, float scr, float scg, float scb,
                     float inv_rad, float &lr, float &lg, float &lb, int &depth, int max_depth, int32_t *pixel) {
  return shade_ray_emit<DERIVE>(r, have, t, spx, spy, spz, scr, scg, scb, inv_rad, lr, lg, lb, depth, max_depth,
                                [&](float cr, float cg, float cb) { *pixel = pack_pixel(cr, cg, cb); });
}

// A chain whose light is exactly zero cannot change its pixel any more (the render path's dark stop; DESIGN.md 3.1, SHADE).  Asked where a fold
// has just scattered: shade_ray returned true and lr, lg, lb hold the NEW light.
//  - ray_colour (ray.fut:126-148) keeps colour = (0,0,0) until the chain ends and then returns light * sky (a miss, :140-148) or light * 0
//    (absorbed, or the bounce budget spent); light is the running product of the colours of the spheres hit so far (:136-138).
//  - `== 0.0f` holds for +0 and -0 and fails for NaN.  From a channel that is +-0 every later value of that channel is 0 * colour: +-0 for a
//    finite colour, NaN for an infinite or NaN one, never anything else -- and NaN stays NaN.
//  - colour_to_pixel's operand (:158-162) is that value times the sky term or times 0.0f: +-0 or NaN again, whatever the sky term is (finite,
//    inf or NaN from a degenerate direction).  255.99f * (+-0 | NaN) is +-0 or NaN, the device's float -> int conversion gives 0 for both, and
//    (0 << 16) | (0 << 8) | 0 == 0.
// So a pixel stored as 0 here is what the full chain would have stored: no guard on the scene, the camera or max_depth.  Only for PACKED
// pixels: the entries that return float colours (rt_trace_rays, rt_trace_paths) show -0 and NaN payloads and never stop.
RT_HD bool light_is_dead(float lr, float lg, float lb) { return (lr == 0.0f) & (lg == 0.0f) & (lb == 0.0f); }

// One whole iteration of ray_colour's loop body AFTER the fold: re-intersect the winning
// sphere with (0.0, best+1), then scatter or terminate.
RT_HD bool finish_ray(Ray &r, float best, int bestj, float spx, float spy, float spz, float srad,
                      float scr, float scg, float scb, float inv_rad, float &lr, float &lg, float &lb,
                      int &depth, int max_depth, int32_t *pixel) {
  float t = 0.0f;
  const bool have = bestj >= 0 && rehit_full(r, best, spx, spy, spz, srad, &t);
  return shade_ray<true>(r, have, t, spx, spy, spz, scr, scg, scb, inv_rad, lr, lg, lb, depth, max_depth, pixel);
}
template <class Emit>
RT_HD bool finish_ray_emit(Ray &r, float best, int bestj, float spx, float spy, float spz, float srad,
                           float scr, float scg, float scb, float inv_rad, float &lr, float &lg, float &lb,
                           int &depth, int max_depth, Emit &&emit) {
  float t = 0.0f;
  const bool have = bestj >= 0 && rehit_full(r, best, spx, spy, spz, srad, &t);
  return shade_ray_emit<true>(r, have, t, spx, spy, spz, scr, scg, scb, inv_rad, lr, lg, lb, depth, max_depth, emit);
}

// ---- per-tile entry lists (the ENTRY instantiations of the pooled kernel) ---------------------------------
// The primary rays of one tile share their origin and nearly their direction: for most upper nodes box_hit gives all of them the
// same verdict, and that is proven once per tile.  tile_rays bounds every ray's 1 / d_k from the tile's corner pixels;
// tile_verdict folds those bounds through box_hit_presorted's own chain; tile_frontier walks the tree while both children of a
// node have one verdict for the whole tile, and what it stops at -- at most one inner node and kEntryLeaves leaves -- is what a
// new primary ray of the tile starts from instead of the root.  A tile with no list starts at the root: same pixels either way.
// `MUT`: the faults tools/entry_check.cpp must find (1: ALLMISS decided with < instead of <=; 2: bounds from two corners; 3: the
// sign check dropped); 0 everywhere else.
constexpr int kEntryLeaves = 6;              // leaves a kept list holds at most (with one inner item and the header: kEntryDw dwords)
constexpr int kEntryDw = 8;                  // dwords per position of the table: header, inner item or 0, kEntryLeaves leaf references
constexpr int kEntryStack = 24;              // tile_frontier's private stack (overflow: no list)
constexpr uint32_t kEntryValid = 1u, kEntryInner = 2u;   // header: bit 0 the position has a list, bit 1 it holds an inner item, ...
constexpr int kEntryCountShift = 4;                      // ... bits 4 .. 7 its number of leaves
enum { kTileMixed = 0, kTileAllHit = 1, kTileAllMiss = 2 };
struct TileRays {
  float o[3];
  float imin[3], imax[3];   // every ray's 1 / d_k lies in [imin_k, imax_k]; both finite, non-zero, of one sign
};

// (u0, u1) x (v0, v1): u and v of the tile's first / last column and row THAT EXIST.  Each d_k = ((l_k + u h_k) + v v_k) - o_k is a chain
// of rounded binary32 operations, monotone in u for fixed v and in v for fixed u, and the tables are monotone in column and row: over the
// tile's pixel rectangle d_k takes its extremes at the four corners.  Four corners finite, non-zero and of one sign: so is every ray's
// d_k, and 1 / d_k (monotone on either side of zero) lies between the corners' extremes.  A quotient that is not finite (a subnormal d_k)
// gives no bounds either: tile_verdict's products must never meet 0 * inf.
template <int MUT = 0>
RT_HD bool tile_rays(const Cam &c, float u0, float u1, float v0, float v1, TileRays *t) {
  Ray q[4];
  primary_dir_uv(c, u0, v0, q[0]);
  primary_dir_uv(c, u1, v1, q[3]);
  if (MUT == 2) { q[1] = q[0]; q[2] = q[3]; }
  else { primary_dir_uv(c, u1, v0, q[1]); primary_dir_uv(c, u0, v1, q[2]); }
  t->o[0] = c.ox; t->o[1] = c.oy; t->o[2] = c.oz;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    float lo = 0.0f, hi = 0.0f;
    bool pos = true, neg = true;
    for (int j = 0; j < 4; ++j) {
      const float d = k == 0 ? q[j].dx : k == 1 ? q[j].dy : q[j].dz;
      const float i = 1.0f / d;
      pos = pos & (d > 0.0f) & (i > 0.0f) & (i < kNoHit);
      neg = neg & (d < 0.0f) & (i < 0.0f) & (i > -kNoHit);
      lo = j == 0 || i < lo ? i : lo;
      hi = j == 0 || i > hi ? i : hi;
    }
    if (MUT != 3) ok = ok & (pos | neg);
    t->imin[k] = lo; t->imax[k] = hi;
  }
  return ok;
}

// box_hit_presorted over (0, 1e9) for every ray of the tile at once.  near_k - o_k and far_k - o_k are one float each for the whole tile
// (one origin, one sign per axis); a product c * i is monotone in i, so it lies between c * imin and c * imax, both attained; fmaxf / fminf
// over non-NaN values are monotone, so the folds of the lower ends bound every ray's tmin / tmax from below and those of the upper ends
// from above.  ALLHIT: every ray has tmax > tmin; ALLMISS: every ray has tmax <= tmin.
template <int MUT = 0>
RT_HD int tile_verdict(const TileRays &t, const float lo[3], const float hi[3]) {
  float tmin_lo = 0.0f, tmin_hi = 0.0f, tmax_lo = kTMax, tmax_hi = kTMax;
  for (int k = 0; k < 3; ++k) {
    const bool neg = t.imax[k] < 0.0f;
    const float cn = (neg ? hi[k] : lo[k]) - t.o[k], cf = (neg ? lo[k] : hi[k]) - t.o[k];
    const float na = cn * t.imin[k], nb = cn * t.imax[k], fa = cf * t.imin[k], fb = cf * t.imax[k];
    tmin_lo = fmaxf(na < nb ? na : nb, tmin_lo);
    tmin_hi = fmaxf(na < nb ? nb : na, tmin_hi);
    tmax_lo = fminf(fa < fb ? fa : fb, tmax_lo);
    tmax_hi = fminf(fa < fb ? fb : fa, tmax_hi);
  }
  if (tmax_lo > tmin_hi) return kTileAllHit;
  if (MUT == 1 ? tmax_hi < tmin_lo : tmax_hi <= tmin_lo) return kTileAllMiss;
  return kTileMixed;
}

// The frontier of a tile over the pooled records (nodes64: 16 floats per inner node -- {L.lo, left << 8} {L.hi, right << 8} {R.lo, .} {R.hi, .},
// a leaf child's slot holding the sphere's own widened box where the scene's slots are filled).  A child is UNIFORM when the whole tile
// agrees on what a BOX operation does with it: an inner child that is ALLHIT or ALLMISS; a leaf child of an unfiltered launch (always
// tested); a leaf child of a filtering launch (`filter`, 3.4a) whose slot is ALLHIT (tested) or ALLMISS (dropped).  An ALLHIT node with two
// uniform children is expanded here; every other reached node is emitted as an inner item.  false: no list (the root is not ALLHIT, the
// stack or a cap overflowed, or the list is the root alone).
template <int MUT, int MAXI, int MAXL>
RT_HD bool tile_frontier(const TileRays &t, const float root_lo[3], const float root_hi[3], const float *nodes64, int n_nodes, bool filter,
                         int *inner, int *n_inner, int *leaf, int *n_leaf) {
  *n_inner = 0; *n_leaf = 0;
  if (n_nodes < 1 || tile_verdict<MUT>(t, root_lo, root_hi) != kTileAllHit) return false;
  int stack[kEntryStack], sp = 0, ni = 0, nl = 0;
  stack[sp++] = 0;
  while (sp > 0) {
    const int node = stack[--sp];
    const float *const rec = nodes64 + 16 * (size_t)node;
    int child[2], verdict[2];
    bool uniform = true;
    for (int s = 0; s < 2; ++s) {
      int32_t w;
      __builtin_memcpy(&w, rec + 4 * s + 3, 4);
      child[s] = w >> 8;
      verdict[s] = tile_verdict<MUT>(t, rec + 8 * s, rec + 8 * s + 4);
      if (child[s] < 0 && !filter) verdict[s] = kTileAllHit;
      uniform = uniform & (verdict[s] != kTileMixed);
    }
    if (!uniform) {
      if (node == 0 || ni >= MAXI) return false;
      inner[ni++] = node;
      continue;
    }
    for (int s = 0; s < 2; ++s) {
      if (verdict[s] != kTileAllHit) continue;
      if (child[s] < 0) {
        if (nl >= MAXL) return false;
        leaf[nl++] = ~child[s];
      } else {
        if (sp >= kEntryStack) return false;
        stack[sp++] = child[s];
      }
    }
  }
  *n_inner = ni; *n_leaf = nl;
  return true;
}

// One position of the table: the header, the inner item and the leaf references in the form the consuming kernel's work items carry them
// (render_kernels.hip: an inner node as (node * node_mul) << ref_shift, a leaf as ~leaf << ref_shift; the slot and the ray's signs are
// ORed in by the ray that pushes them).  All zero: no list.
template <int MUT = 0>
RT_HD void tile_entry(const TileRays &t, bool rays_ok, const float root_lo[3], const float root_hi[3], const float *nodes64, int n_nodes, bool filter,
                      int ref_shift, int node_mul, uint32_t out[kEntryDw]) {
  int inner[1], leaf[kEntryLeaves], ni = 0, nl = 0;
  const bool ok = rays_ok && tile_frontier<MUT, 1, kEntryLeaves>(t, root_lo, root_hi, nodes64, n_nodes, filter, inner, &ni, leaf, &nl);
  for (int i = 0; i < kEntryDw; ++i) out[i] = 0u;
  if (!ok) return;
  out[0] = kEntryValid | (ni ? kEntryInner : 0u) | (uint32_t)nl << kEntryCountShift;
  if (ni) out[1] = (uint32_t)(inner[0] * node_mul) << ref_shift;
  for (int i = 0; i < kEntryLeaves; ++i)
    if (i < nl) out[2 + i] = (uint32_t)~leaf[i] << ref_shift;
}

// ---- exit lists: a ray that has just scattered starts below the root -------------------------------------
// For a leaf j take its chain of ancestors c_0 = root, c_1, ... and the siblings s_k (the child of c_{k-1} that is not on the chain).
// A walk from the root whose ray passes the box of every c_k, k <= e, tests exactly the leaves that the walks from c_e and from
// s_1 ... s_e test, each sibling under the verdict of its own box.  Two siblings make one PAIR RECORD -- a node record whose two child
// slots are copied bit for bit from the siblings' slots in their real parents' records -- so that an ordinary BOX item naming it gives
// both verdicts.  The list of j: the node E = c_e, e even and <= kExitDmax, its box, and the e / 2 pair records above it.
// Legality: (host side of it, here) every c_k, k < e, CONTAINS E's box component-wise on the floats as stored, all of them finite;
// (per ray, in SHADE) the ray passes box_hit on E's box.  The lemma of DESIGN.md 3.4c then gives a pass on every c_k.
// The table: kExitPairs pair records of 16 floats in the nodes64 format, then 8 dwords per sphere:
//   {E.lo.xyz, E's ref | pair 1's ref << 16} {E.hi.xyz, pair 2's ref | pair 3's ref << 16},
// a ref being the record's index (pair record p: n_nodes + p) times `ref_mul` -- the kernel's: kPsNodeBytes / 8, the byte offset of the staged record / 8 --
// in 16 bits (the caller checks that the scene fits: rt_device.hpp, pooled_exit_fits); E's ref 0: no list.
// `MUT`: the faults tools/exit_check.cpp must find (1: no nesting check); 0 everywhere else.
constexpr int kExitDmax = 4;
constexpr int kExitPairs = (4 << kExitDmax) / 3 - 1;   // 4 + 16 + ... + 2^Dmax: one pair record per node of depth 2, 4, ... Dmax (4: 20; 6: 84)
constexpr int kExitStack = 48;                         // exit_tables_path's private stack (overflow: the leaves not reached get no list)
// pair record i (1-based: the siblings of depth 2i - 1 and 2i) of the paths whose first 2i turns are `prefix` (left = 0, the first turn in the highest bit)
constexpr int exit_pair_id(int i, int prefix) { return ((4 << (2 * (i - 1))) / 3 - 1) + prefix; }

// Path t of kExitDmax turns from the root (bit kExitDmax - k of t is turn k): writes the pair records the path is the first to reach and
// the entries of the leaves whose list resumes on it.  The table must be zeroed beforehand; paths write disjoint words.
template <int MUT = 0>
RT_HD void exit_tables_path(int t, const float root_lo[3], const float root_hi[3], const float *nodes64, int n_nodes, int n_sph, float *tab, int ref_mul = kPsNodeBytes / 8) {
  constexpr int D = kExitDmax;
  if (n_nodes < 1) return;
  float clo[D + 1][3], chi[D + 1][3];    // the chain's boxes, [0] the root's
  int cidx[D + 1];                       // ... and node indices
  float srec[D + 1][8];                  // sibling k's slot: lo.xyz, w of the lo quarter, hi.xyz, its reference word
  for (int a = 0; a < 3; ++a) { clo[0][a] = root_lo[a]; chi[0][a] = root_hi[a]; }
  cidx[0] = 0;
  int depth = 0, leaf = -1, cur = 0;
  for (int k = 1; k <= D; ++k) {
    if (leaf >= 0) continue;
    const int bit = (t >> (D - k)) & 1;
    const float *const rec = nodes64 + 16 * (size_t)cur;
    for (int s = 0; s < 2; ++s) {
      if (s == bit) {
        for (int a = 0; a < 3; ++a) { clo[k][a] = rec[8 * s + a]; chi[k][a] = rec[8 * s + 4 + a]; }
      } else {
        for (int a = 0; a < 3; ++a) { srec[k][a] = rec[8 * s + a]; srec[k][4 + a] = rec[8 * s + 4 + a]; }
        srec[k][3] = 0.0f;
        srec[k][7] = rec[4 * s + 3];
      }
    }
    int32_t w;
    __builtin_memcpy(&w, rec + 4 * bit + 3, 4);
    depth = k;
    if ((w >> 8) < 0) leaf = ~(w >> 8);
    else { cur = w >> 8; cidx[k] = cur; }
  }
  // (a path that ends at a leaf of depth < D is shared by the paths that differ in the turns behind it: the one whose are all left does the work)
  if (leaf >= 0 && (t & ((1 << (D - depth)) - 1)) != 0) return;
  for (int i = 1; 2 * i <= depth; ++i) {
    if ((t & ((1 << (D - 2 * i)) - 1)) != 0) continue;
    float *const out = tab + 16 * (size_t)exit_pair_id(i, t >> (D - 2 * i));
    const float *const a = srec[2 * i - 1], *const b = srec[2 * i];
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[7];      // {L.lo, left ref}
    out[4] = a[4]; out[5] = a[5]; out[6] = a[6]; out[7] = b[7];      // {L.hi, right ref}
    out[8] = b[0]; out[9] = b[1]; out[10] = b[2]; out[11] = 0.0f;    // {R.lo, .}
    out[12] = b[4]; out[13] = b[5]; out[14] = b[6]; out[15] = 0.0f;  // {R.hi, .}
  }
  // the node the lists of this path resume at: the deepest INNER node of even depth on it
  const int e = leaf >= 0 ? (depth - 1) & ~1 : D;
  if (e < 2) return;
  bool nested = true;
  for (int a = 0; a < 3; ++a) nested = nested & (clo[e][a] > -kNoHit) & (chi[e][a] < kNoHit);
  for (int k = 0; k < e; ++k)
    for (int a = 0; a < 3; ++a) nested = nested & (clo[k][a] <= clo[e][a]) & (chi[k][a] >= chi[e][a]) & (clo[k][a] > -kNoHit) & (chi[k][a] < kNoHit);
  if (MUT != 1 && !nested) return;
  uint32_t ref[4] = {(uint32_t)cidx[e] * (uint32_t)ref_mul, 0u, 0u, 0u};
  for (int i = 1; 2 * i <= e; ++i) ref[i] = (uint32_t)(n_nodes + exit_pair_id(i, t >> (D - 2 * i))) * (uint32_t)ref_mul;
  const uint32_t w0 = ref[0] | ref[1] << 16, w1 = ref[2] | ref[3] << 16;
  auto put = [&](int j) {
    if (j < 0 || j >= n_sph) return;
    float *const out = tab + 16 * (size_t)kExitPairs + 8 * (size_t)j;
    for (int a = 0; a < 3; ++a) { out[a] = clo[e][a]; out[4 + a] = chi[e][a]; }
    __builtin_memcpy(out + 3, &w0, 4);
    __builtin_memcpy(out + 7, &w1, 4);
  };
  if (leaf >= 0) { put(leaf); return; }
  int stack[kExitStack], sp = 0;
  stack[sp++] = cur;
  while (sp > 0) {
    const float *const rec = nodes64 + 16 * (size_t)stack[--sp];
    for (int s = 0; s < 2; ++s) {
      int32_t w;
      __builtin_memcpy(&w, rec + 4 * s + 3, 4);
      if ((w >> 8) < 0) put(~(w >> 8));
      else if (sp < kExitStack) stack[sp++] = w >> 8;
    }
  }
}

}  // namespace rtk
