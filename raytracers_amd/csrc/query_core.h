// query_core.h -- per-lane arithmetic of the caller queries that no render-path kernel calls: both roots of a sphere and the sphere
// casts' contact rule, the proximity queries' gap, box bound, slack and selection key, the box queries' gap and node test, the plane-set
// queries' normalisation, gap and node test, a ray path's bounce, the contact clusters' union-find.  Shared by query_kernels.hip and the host-side checks (tools/sweep_check.cpp, tools/along_check.cpp, tools/path_check.cpp, tools/clusters_check.cpp, tools/proximity_bound_check.cpp,
// tools/box_query_bound_check.cpp, tools/plane_query_bound_check.cpp).  Same parity contract as lane_core.h, which holds what the render
// path shares with the queries (box_hit_interval, sphere_hit_any, interval_ok, rehit_range).
#pragma once
#include "lane_core.h"

namespace rtk {

// `sphere_hit`'s two roots (ray.fut:32-51) with sphere_hit_any's arithmetic, both kept: the crossings of rt_multi_hit_rays.  False (roots
// not written) when the discriminant is not positive; a NaN discriminant gives two NaN roots, which lie inside no interval.
RT_HD bool sphere_roots(const Ray &r, float spx, float spy, float spz, float srad, float *t1, float *t2) {
  const float ocx = r.ox - spx, ocy = r.oy - spy, ocz = r.oz - spz;
  const float b = dot3(ocx, ocy, ocz, r.dx, r.dy, r.dz);
  const float c = dot3(ocx, ocy, ocz, ocx, ocy, ocz) - srad * srad;
  const float disc = b * b - r.a * c;
  if (disc <= 0.0f) return false;
  const float sq = sqrtf(disc);
  *t1 = (-b - sq) / r.a;
  *t2 = (-b + sq) / r.a;
  return true;
}

// The contact of a sphere of radius rq moving along r with scene sphere (sp, srad) over (tlo, thi) (rt_sweep_spheres): the
// ray of its centre against the sphere (sp, R = srad + rq), sphere_roots' arithmetic with R for the radius.  kSweepEntry: root 1 lies past
// tlo and the contact is there, accepted iff it is below thi.  kSweepStart: root 1 is at or before tlo and root 2 past it -- the two
// spheres already overlap where the interval begins -- and the contact is at tlo itself (-0.0 reported as +0.0), provided the interval is
// not empty.  kSweepNone otherwise: touching only at the exit (t2 == tlo) is none, and NaN roots pass no compare.  *tau is written for a
// contact only.
constexpr int kSweepNone = 0, kSweepEntry = 1, kSweepStart = 2;
RT_HD int sweep_contact(const Ray &r, float spx, float spy, float spz, float srad, float rq, float tlo, float thi, float *tau) {
  const float R = srad + rq;
  float t1, t2;
  if (!sphere_roots(r, spx, spy, spz, R, &t1, &t2)) return kSweepNone;
  if (t1 > tlo) {
    if (!(t1 < thi)) return kSweepNone;
    *tau = t1;
    return kSweepEntry;
  }
  if ((t2 > tlo) && (tlo < thi)) {
    *tau = tlo + 0.0f;
    return kSweepStart;
  }
  return kSweepNone;
}
// sweep_contact with the two roots handed back (rt_spheres_along_rays_*): the same operations in the same order, so kind and
// *tau are sweep_contact's bit for bit; *t1 and *t2 are the roots it compared -- of (sp, R = srad + rq), unclamped -- and are written
// whenever the discriminant is positive (a NaN discriminant: two NaN roots, kSweepNone), also for kSweepNone.
RT_HD int sweep_contact_roots(const Ray &r, float spx, float spy, float spz, float srad, float rq, float tlo, float thi, float *tau, float *t1,
                              float *t2) {
  const float R = srad + rq;
  if (!sphere_roots(r, spx, spy, spz, R, t1, t2)) return kSweepNone;
  if (*t1 > tlo) {
    if (!(*t1 < thi)) return kSweepNone;
    *tau = *t1;
    return kSweepEntry;
  }
  if ((*t2 > tlo) && (tlo < thi)) {
    *tau = tlo + 0.0f;
    return kSweepStart;
  }
  return kSweepNone;
}

// ---- proximity: the spheres nearest to a point (rt_nearest_spheres) ------------------------------------------------
// The gap of point p to sphere (c, r): the signed distance to its surface, negative inside.  This exact binary32 arithmetic IS the
// definition (with -ffp-contract=off and a correctly rounded sqrtf); it is never -0.0 (sqrtf gives +0 or more, and x - x = +0).
RT_HD float point_gap(float px, float py, float pz, float cx, float cy, float cz, float r) {
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  return sqrtf(dot3(dx, dy, dz, dx, dy, dz)) - r;
}
// The point-to-box distance, computed in binary32: for every sphere whose binary32 box fl(c -+ r) lies inside [lo, hi] it is, up to the slack
// below, a LOWER bound on max(gap, 0).  Those are the spheres below a node only where the node's box contains its subtree: the boxes are
// unions of the spheres' boxes after floor(log2 n) + 2 sweeps from zero boxes, so in a taller tree the nodes nearer the root than
// height - sweeps levels are never tested (query_kernels.hip: nearest_lane).
RT_HD float box_gap_bound(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float ex = fmaxf(fmaxf(lox - px, px - hix), 0.0f);
  const float ey = fmaxf(fmaxf(loy - py, py - hiy), 0.0f);
  const float ez = fmaxf(fmaxf(loz - pz, pz - hiz), 0.0f);
  return sqrtf(dot3(ex, ey, ez, ex, ey, ez));
}
// The slack of the box test.  Let u = 2^-24, g the exact gap of p to a sphere (c, r) below the node, G = point_gap (computed), B =
// box_gap_bound (computed), P = max_k |p_k|, M = max_k max(|lo_k|, |hi_k|) of the node's box, t >= 0 the threshold.  Then
//   (P1)  |G - g| <= 4.6 u D + u r + 2^-62,   D = |p - c| <= sqrt(3) (P + M) (1 + 3u),  r <= M (1 + 2u)
//         (dx = (p - c)(1 + e): the sum of squares is within (1 + u)^5 of exact, sqrtf adds u, the subtraction of r adds u |G|;
//         2^-62 covers squares that underflow, flushed or not)
//   (P2)  the stored box misses at most u M (1 + 2u) of the exact sphere on each side (round to nearest of c -+ r, whose magnitude is
//         at most M / (1 - u)), so the exact point-to-box distance is at most max(g, 0) + sqrt(3) u M (1 + 2u)
//   (P3)  B <= (1 + 3.5 u) (exact point-to-box distance) + 2^-62 (the same chain as P1 on the box's per-axis excesses)
// Hence G <= T implies, with t = max(T, 0):  B <= t + u (3.6 t + 9.8 P + 12.6 M) + 2^-61  (second-order terms folded into the decimals).
// proximity_slack is 2^-19 = 32 u times t + P + M, plus 2^-56: at least twice every coefficient, which also absorbs the rounding of the
// slack's own two additions and of t + slack.  A box with B > t + slack therefore holds no sphere with G <= T; t clamps T at 0 because B
// bounds max(gap, 0), not the gap (a point inside a sphere is at distance 0 from its box).  tools/proximity_bound_check.cpp searches for
// counterexamples with boxes from the host builder; with the slack set to 0 it finds them.  An overflowing sum (|coordinates| near 2^64
// and beyond) gives B = +inf (the node is skipped) only where every G below it is +inf too, and a slack of +inf skips nothing.
RT_HD float proximity_slack(float t, float pmag, float bmag) { return 0x1p-19f * ((t + pmag) + bmag) + 0x1p-56f; }
RT_HD float box_mag(float lox, float loy, float loz, float hix, float hiy, float hiz) {
  return fmaxf(fmaxf(fmaxf(fabsf(lox), fabsf(hix)), fmaxf(fabsf(loy), fabsf(hiy))), fmaxf(fabsf(loz), fabsf(hiz)));
}
// May the node with box [lo, hi] hold a sphere whose gap to p is <= T?  (pmag = max_k |p_k|; T finite.)  `slack_scale` is 1 in the
// product; the bound check's sensitivity run passes 0.
RT_HD bool box_may_hold(float px, float py, float pz, float pmag, float lox, float loy, float loz, float hix, float hiy, float hiz, float T,
                        float slack_scale = 1.0f) {
  const float t = fmaxf(T, 0.0f);
  const float b = box_gap_bound(px, py, pz, lox, loy, loz, hix, hiy, hiz);
  return !(b > t + slack_scale * proximity_slack(t, pmag, box_mag(lox, loy, loz, hix, hiy, hiz)));
}
// The selection key of sphere j at gap g: g's bits mapped to an order-preserving unsigned word (negative: all bits flipped; otherwise the
// sign bit set) above j.  A selected gap is <= 1e9, so its high word is below 0xffffffff and the empty slot ~0 never collides with it.
RT_HD uint64_t gap_key(float g, int j) {
  uint32_t b;
  __builtin_memcpy(&b, &g, 4);
  const uint32_t hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)hi << 32) | (uint32_t)j;
}
RT_HD float gap_of_key(uint64_t key) {
  const uint32_t hi = (uint32_t)(key >> 32);
  const uint32_t b = (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
  float g;
  __builtin_memcpy(&g, &b, 4);
  return g;
}
// A point with a non-finite component gets no walk (count 0); so does, in rt_nearest_spheres_ranged, a bound failing 0 <= max_dist <= 1e9.
RT_HD bool point_ok(float px, float py, float pz) {
  return fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) <= 3.40282347e38f && px == px && py == py && pz == pz;
}
RT_HD bool max_dist_ok(float m) { return (m >= 0.0f) & (m <= kTMax); }

// ---- box queries: the spheres that meet an axis-aligned box (rt_spheres_in_boxes_*) ---------------------------------
// A caller's box {lo, hi}.  Valid iff its six components are finite and lo_k <= hi_k for every k (zero extent is valid); an invalid box
// gets no walk, as a point failing point_ok.
struct QBox {
  float lox, loy, loz, hix, hiy, hiz;
};
RT_HD bool qbox_ok(const QBox &q) {
  return box_mag(q.lox, q.loy, q.loz, q.hix, q.hiy, q.hiz) <= 3.40282347e38f && q.lox <= q.hix && q.loy <= q.hiy && q.loz <= q.hiz;   // (a NaN fails a <=)
}
// The gap of box q to sphere (c, r): the signed distance from the box to the sphere's surface, -r where the centre is inside the box.  This
// exact binary32 arithmetic IS the definition (as point_gap: no contraction, a correctly rounded sqrtf).  With lo == hi == p the excess of an
// axis is fmaxf(fmaxf(p - c, c - p), 0) = |fl(p - c)| (fl(c - p) = -fl(p - c)), whose square is point_gap's dx * dx: box_gap of a degenerate
// box IS point_gap(p, ...), bit for bit.
RT_HD float box_gap(const QBox &q, float cx, float cy, float cz, float r) {
  const float ex = fmaxf(fmaxf(q.lox - cx, cx - q.hix), 0.0f);
  const float ey = fmaxf(fmaxf(q.loy - cy, cy - q.hiy), 0.0f);
  const float ez = fmaxf(fmaxf(q.loz - cz, cz - q.hiz), 0.0f);
  return sqrtf(dot3(ex, ey, ez, ex, ey, ez)) - r;
}
// The box-to-box distance of q and the node's box [lo, hi], computed in binary32.  With q.lo == q.hi == p it is box_gap_bound(p, lo, hi),
// operation for operation (lo - p, p - hi), so the walk of a degenerate box is the point walk.
RT_HD float box_box_bound(const QBox &q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float ex = fmaxf(fmaxf(lox - q.hix, q.lox - hix), 0.0f);
  const float ey = fmaxf(fmaxf(loy - q.hiy, q.loy - hiy), 0.0f);
  const float ez = fmaxf(fmaxf(loz - q.hiz, q.loz - hiz), 0.0f);
  return sqrtf(dot3(ex, ey, ez, ex, ey, ez));
}
// The slack of the box-to-box test.  u, M and t as for proximity_slack; now g is the exact gap of the box q to a sphere (c, r) below the node
// (the exact distance from q to c, minus r), G = box_gap (computed), B = box_box_bound (computed), and P = the largest magnitude among
// q's SIX coordinates.  Every excess, at the leaf and at the node, is still ONE rounded subtraction of a query coordinate and a scene
// coordinate, then clamped: fl is monotone and odd, so fmaxf(fmaxf(fl(a), fl(b)), 0) = fl(max(a, b, 0)) = (exact excess)(1 + e), |e| <= u --
// the clamps add no error, and an excess is at most P + M in magnitude.  So the three steps keep their coefficients:
//   (Q1)  |G - g| <= 4.6 u D + u r + 2^-62,   D = the exact distance from q to c <= sqrt(3) (P + M) (1 + 3u),  r <= M (1 + 2u)
//         (P1's chain on the three excesses in place of p - c)
//   (Q2)  the stored box misses at most d = u M (1 + 2u) of the sphere's exact box on each side (P2), so per axis the exact excess of q
//         against the node's box is at most a_k + d, a_k = max(c_k - r - qhi_k, qlo_k - c_k - r, 0) being the excess against the sphere's exact
//         box; the ball lies inside that box, so |a| <= max(g, 0), and the exact box-to-box distance is at most max(g, 0) + sqrt(3) d
//   (Q3)  B <= (1 + 3.5 u) (exact box-to-box distance) + 2^-62 (P3's chain)
// Hence G <= T implies B <= t + u (3.6 t + 9.8 P + 12.6 M) + 2^-61 exactly as for points, and proximity_slack(t, P, M) with this P covers it
// with the same factor of two to spare.  P must be the maximum over all six coordinates: an excess subtracts q.hi on one side and q.lo on the
// other.  tools/box_query_bound_check.cpp searches for counterexamples; with the slack set to 0 it finds them (the degenerate boxes alone
// guarantee that: they are the point checker's cases).
RT_HD bool box_may_meet(const QBox &q, float qmag, float lox, float loy, float loz, float hix, float hiy, float hiz, float T,
                        float slack_scale = 1.0f) {
  const float t = fmaxf(T, 0.0f);
  const float b = box_box_bound(q, lox, loy, loz, hix, hiy, hiz);
  return !(b > t + slack_scale * proximity_slack(t, qmag, box_mag(lox, loy, loz, hix, hiy, hiz)));
}

// ---- plane-set queries: the spheres inside a frustum or convex polytope (rt_spheres_in_planes_*) ---------------------
// A caller's plane {a, b, c, d} (inside: a x + b y + c z + d >= 0) normalised once per query: n = (a, b, c) / len, w = d / len.  This exact
// binary32 arithmetic IS the definition (no contraction, correctly rounded sqrtf and /).  Valid iff the four inputs are finite,
// 2^-40 <= len <= 2^40 and the four quotients are finite (a NaN fails every compare); a query with an invalid plane gets no walk.
struct QPlane {
  float nx, ny, nz, w;
};
#if defined(__clang__)
#define RT_UNROLL _Pragma("unroll")   // (the loops over a query's K planes: K is a template parameter, the planes stay in registers)
#else
#define RT_UNROLL
#endif
RT_HD bool plane_normalise(float a, float b, float c, float d, QPlane *p) {
  const float len = sqrtf((a * a + b * b) + c * c);
  p->nx = a / len;
  p->ny = b / len;
  p->nz = c / len;
  p->w = d / len;
  // Three compares say all of it: a NaN or infinite a, b or c, or one of 2^64 and more, makes len NaN or +inf; with len in range each of
  // |a|, |b|, |c| is at most len (1 + 3u), so three quotients are finite; and w is finite iff d is finite and d / len does not overflow.
  return len >= 0x1p-40f && len <= 0x1p40f && fabsf(p->w) <= 3.40282347e38f;
}
// The signed depth of the point x inside the plane, positive inside.
RT_HD float plane_depth(const QPlane &p, float x, float y, float z) { return dot3(p.nx, p.ny, p.nz, x, y, z) + p.w; }
// The gap of the plane set pl[0 .. K) to sphere (c, r): how far the sphere's surface is outside the half-space it is furthest outside of,
// -r where the centre is inside every half-space (as box_gap's).  The planes enter in the caller's order; a repeated plane changes nothing.
template <int K>
RT_HD float plane_gap(const QPlane (&pl)[K], float cx, float cy, float cz, float r) {
  float e = 0.0f;
RT_UNROLL
  for (int k = 0; k < K; ++k) e = fmaxf(e, -plane_depth(pl[k], cx, cy, cz));
  return e - r;
}
// The node test.  For plane k the largest depth over the node's box [lo, hi] is taken at its most-inside vertex v (v_j = hi_j where
// n_j >= 0, else lo_j); D_k = plane_depth(k, v) computed in binary32.  The node is skipped iff some plane has -D_k > t + slack.  No radius
// enters: the sphere's own box lies inside the node's box.  Let u = 2^-24, n^ = (a, b, c) / |(a, b, c)| and w^ = d / |(a, b, c)| the exact
// unit plane, g = max(0, max_k -(n^_k . c + w^_k)) - r the exact gap, G = plane_gap (computed), W = max_k |w_k|, M = box_mag of the node's
// box, t = max(T, 0).  |x| is the Euclidean norm.
//   (R0)  len = |(a, b, c)| (1 + e), |e| <= 2.5 u (three roundings on a sum of squares, halved by the root, and the root's own); each
//         quotient adds u: n_j = n^_j (1 + e_j), w = w^ (1 + e_w), |e_j|, |e_w| <= 3.6 u, so |n|_2 = 1 + e_n, |e_n| <= 3.6 u.  (With
//         len >= 2^-40 a square that underflows is below 2^-46 of the sum.)
//   (R1)  |G - g| <= u (8.8 |c| + 5.8 W + r) + 2^-62.  A computed depth is within u (4 |n . c|* + |w|), |n . c|* = sum_j |n_j c_j| <= |n| |c|,
//         of n . c + w in exact arithmetic (the first product meets four roundings, w one), and that is within 3.6 u (|c| + |w^|) of the
//         exact plane's depth (R0): 7.7 u |c| + 4.7 u W together.  max and the clamp at 0 add nothing; the subtraction of r adds
//         u |G| <= u (|c| + W + r) (1 + 9u).  2^-62 covers products that underflow, flushed or not.
//   (R2)  the stored box misses at most d = u M (1 + 2u) of the sphere's exact box on each side (P2), and a centre lies INSIDE its stored
//         box (fl(c - r) <= c <= fl(c + r)).  Over the sphere's exact box the largest depth is n . c + w + r |n|_1, and |n|_1 >= |n|_2 >=
//         1 - 3.6 u, |n|_1 <= sqrt(3) (1 + 3.6 u); so in exact arithmetic on the computed plane
//         -(n . v + w) <= -(n . c + w) - r (1 - 3.6 u) + sqrt(3) (1 + 4u) d.
//   (R3)  D_k is within u (4 sqrt(3) M + W) (1 + 4u) of n . v + w (|v_j| <= M), and the leaf's depth_k within the same of n . c + w
//         (|c_j| <= M).
// G <= T means fl(E - r) <= t for E = max(0, max_k -depth_k), hence -depth_k <= E <= r + t + u (r + t) (1 + 2u).  Chaining R3, R2, R3:
//   -D_k <= t + u (t + 4.6 r + (8 sqrt(3) + sqrt(3)) M + 2 W) <= t + u (t + 20.2 M + 2 W) + 2^-61     (r <= M (1 + 2u))
// with second-order terms folded into the decimals.  plane_slack is 2^-18 = 64 u times t + W + M, plus 2^-56: more than twice every
// coefficient (the factor proximity_slack keeps), which also absorbs the rounding of the slack's own additions and of t + slack.  A NaN D_k
// (inf - inf at |coordinates| near 2^127) skips nothing, and -D_k = +inf skips only where every leaf depth below is -inf as well: every
// product and partial sum at v is >= the one at a centre inside the box, rounding being monotone.  tools/plane_query_bound_check.cpp
// searches for counterexamples; with the slack scaled to 0 it finds them.
RT_HD float plane_slack(float t, float wmag, float bmag) { return 0x1p-18f * ((t + wmag) + bmag) + 0x1p-56f; }
template <int K>
RT_HD float planes_wmag(const QPlane (&pl)[K]) {
  float m = 0.0f;
RT_UNROLL
  for (int k = 0; k < K; ++k) m = fmaxf(m, fabsf(pl[k].w));
  return m;
}
template <int K>
RT_HD bool planes_may_meet(const QPlane (&pl)[K], float wmag, float lox, float loy, float loz, float hix, float hiy, float hiz, float T,
                           float slack_scale = 1.0f) {
  const float t = fmaxf(T, 0.0f);
  const float lim = t + slack_scale * plane_slack(t, wmag, box_mag(lox, loy, loz, hix, hiy, hiz));
  // fl(n_j v_j) is taken as fmaxf(fl(n_j lo_j), fl(n_j hi_j)): rounding is monotone, so the larger rounded product IS the rounded product at the
  // most-inside vertex (the sign of a zero aside, which the compare below cannot see) -- and the walk keeps no sign masks per plane and axis.
RT_UNROLL
  for (int k = 0; k < K; ++k) {
    const float px = fmaxf(pl[k].nx * lox, pl[k].nx * hix), py = fmaxf(pl[k].ny * loy, pl[k].ny * hiy), pz = fmaxf(pl[k].nz * loz, pl[k].nz * hiz);
    const float D = ((px + py) + pz) + pl[k].w;
    if (-D > lim) return false;
  }
  return true;
}

// ---- ray paths: one iteration of ray_colour's loop behind objs_hit (rt_trace_paths) ---------------------------------
// `have` / `t`: the re-intersection's result for the ray r (rehit_full), sphere {sp, colour sc, inv_rad = 1.0f / radius}; `light` the loop's
// light, `depth` the number of vertices before this one.  Writes the vertex record hit7 = {t, p.xyz, normal.xyz} (seven zeros without a hit)
// and the loop variables behind the iteration: the ray *nr, the light nl[3] and ray_colour's result col[3]; returns how the loop goes on.
//   kPathContinue : the vertex scattered and depth + 1 < max_depth: nr = {p, reflected} with its derived fields, nl = light * colour
//   kPathEscaped  : no hit.  nr = r, nl = light, col = light * sky(r) -- shade_ray_emit's sky arithmetic (lane_core.h)
//   kPathAbsorbed : scatter gave #none (dot(reflected, normal) > 0 is false, NaN included).  nr = r, nl = light, col = light * 0
//   kPathTruncated: the vertex scattered and was the max_depth-th: nr and nl as for kPathContinue (the ray ray_colour never traces, the light
//                   with this vertex's colour), col = light * 0 with the light BEFORE the vertex, as ray_colour's tuple evaluates it
// The arithmetic of a hit is shade_ray_emit's, operation for operation (normalise, the hit record, reflect, scatter's test); what differs
// is what is kept: shade_ray_emit folds absorbed and truncated into one branch and updates neither the ray nor the light there.
constexpr int kPathContinue = -1, kPathEscaped = 0, kPathAbsorbed = 1, kPathTruncated = 2;
RT_HD int path_bounce(const Ray &r, bool have, float t, float spx, float spy, float spz, float scr, float scg, float scb, float inv_rad,
                      float lr, float lg, float lb, int depth, int max_depth, float *hit7, Ray *nr, float *nl, float *col) {
  const float inv_norm = 1.0f / sqrtf(r.a);   // normalise r.dir = scale (1/norm d) d
  *nr = r;
  nl[0] = lr; nl[1] = lg; nl[2] = lb;
  if (!have) {
    for (int q = 0; q < 7; ++q) hit7[q] = 0.0f;
    const float uy = inv_norm * r.dy;
    const float tt = 0.5f * (uy + 1.0f);
    const float w = 1.0f - tt;
    col[0] = lr * (w * 1.0f + tt * 0.5f); col[1] = lg * (w * 1.0f + tt * 0.7f); col[2] = lb * (w * 1.0f + tt * 1.0f);
    return kPathEscaped;
  }
  const float hpx = r.ox + t * r.dx, hpy = r.oy + t * r.dy, hpz = r.oz + t * r.dz;
  const float nx = inv_rad * (hpx - spx), ny = inv_rad * (hpy - spy), nz = inv_rad * (hpz - spz);
  hit7[0] = t;
  hit7[1] = hpx; hit7[2] = hpy; hit7[3] = hpz;
  hit7[4] = nx; hit7[5] = ny; hit7[6] = nz;
  const float ux = inv_norm * r.dx, uy = inv_norm * r.dy, uz = inv_norm * r.dz;
  const float k = 2.0f * dot3(ux, uy, uz, nx, ny, nz);
  const float rx = ux - k * nx, ry = uy - k * ny, rz = uz - k * nz;
  col[0] = lr * 0.0f; col[1] = lg * 0.0f; col[2] = lb * 0.0f;
  if (!(dot3(rx, ry, rz, nx, ny, nz) > 0.0f)) return kPathAbsorbed;
  nr->ox = hpx; nr->oy = hpy; nr->oz = hpz;
  nr->dx = rx; nr->dy = ry; nr->dz = rz;
  ray_derive(*nr);
  nl[0] = lr * scr; nl[1] = lg * scg; nl[2] = lb * scb;
  return depth + 1 < max_depth ? kPathContinue : kPathTruncated;
}

// The contact clusters' union-find (rt_contact_clusters) over a parent array reached through an atomic-ops policy A:
//   int32_t A::load(int32_t x)                          parent[x], relaxed
//   void    A::store(int32_t x, int32_t v)              parent[x] = v, relaxed
//   int32_t A::cas(int32_t x, int32_t expect, int32_t v)   strong compare-exchange of parent[x], relaxed; returns the value it found
// (the device's policy is query_kernels.hip's ParentOps, agent-scope __hip_atomic_*; a host's is std::atomic<int32_t>, tools/clusters_check.cpp).
// Invariants, under any interleaving of any number of callers: parent[x] <= x; parent[x] is a vertex of x's tree; a vertex with
// parent[x] == x (a root) loses that only to a successful cas of uf_unite, which hangs it under a SMALLER vertex of the tree it joins.  So
// every chain x, parent[x], .. strictly descends and ends at a root, trees only ever merge, and a tree's only root is its smallest vertex.
// A load may return any EARLIER value of its word (a stale cache line): every earlier value was a vertex of the same tree that is <= x.
//
// uf_find: a root of x's tree at some moment during the call (it may have been hooked since), with path halving: a vertex passed on the way
// is re-pointed at its grandparent -- a vertex of its tree below it, never at a root's own word (the store's target had a parent != itself,
// and a vertex that was once not a root never is one again), so it cannot undo a hook.
template <class A>
RT_HD int32_t uf_find(const A &a, int32_t x) {
  for (;;) {
    const int32_t p = a.load(x);
    if (p == x) return x;
    const int32_t g = a.load(p);
    if (g == p) return p;
    a.store(x, g);
    x = g;
  }
}
// uf_root: the same walk without a store -- for the flatten pass, where a halving store that lands behind the owner's final store would
// leave a word pointing at a vertex that is not the root.
template <class A>
RT_HD int32_t uf_root(const A &a, int32_t x) {
  for (;;) {
    const int32_t p = a.load(x);
    if (p == x) return x;
    x = p;
  }
}
// uf_unite: afterwards x and y are in one tree; returns a vertex of it that was its root when the call ended its work (the lane's next
// starting point).  The LARGER root's word is swung from itself to the smaller root by one cas: it succeeds only if that vertex is still a
// root, so no link is ever overwritten; where it fails, another caller hooked that vertex first, and the walk goes on from the value the cas
// found -- a retry is always another caller's progress, nothing waits.
template <class A>
RT_HD int32_t uf_unite(const A &a, int32_t x, int32_t y) {
  for (;;) {
    x = uf_find(a, x);
    y = uf_find(a, y);
    if (x == y) return x;
    if (x > y) {
      const int32_t t = x;
      x = y;
      y = t;
    }
    const int32_t seen = a.cas(y, y, x);
    if (seen == y) return x;
    y = seen;
  }
}

// ---- sphere groups: 32-bit masks that filter the masked queries (rt_prepared_set_groups, rt_*_masked) --------------------
// THE rule: a query with mask m sees a sphere -- or may find a seen sphere below an inner node -- whose word is g iff g and m share a bit.
// An unsigned test: bit 31 is a bit like the others, and mask 0 sees nothing.
RT_HD bool group_seen(uint32_t g, uint32_t m) { return (g & m) != 0u; }
// A node's word is the OR of its two children's: for an inner child its own word, for a leaf child the sphere's group word.
RT_HD uint32_t group_combine(uint32_t left, uint32_t right) { return left | right; }
// One step of the derive kernel's climb (query_kernels.hip: groups_climb_kernel): `carry` arrives at a node whose word was `old` before the
// atomic OR.  What goes on to the parent are the bits this step newly set; bits that were there already have been, or are being, carried up
// by the lane that set them.  Zero: the climb ends.
RT_HD uint32_t group_climb_carry(uint32_t old, uint32_t carry) { return carry & ~old; }
// A node's subtree words through a memory policy A, for hosts and the device alike (the device's: query_kernels.hip's GroupOps, relaxed
// agent-scope atomics; a host's: plain words, tools/groups_check.cpp):
//   uint32_t A::fetch_or(int32_t v, uint32_t bits)   node_groups[v] |= bits, returns the value before
//   int32_t  A::parent(int32_t v)                    the parent of inner node v, negative for the root
// Every word starts at 0.  Seeded from every inner node with the combine of its LEAF children's words, the result is the exact OR of the leaves
// below each node: a bit of leaf j reaches every ancestor, because a climb that drops it at node v does so only where another climb set it at
// v and carries it on from there -- by induction along the (finite) root path it is set at every ancestor when the last climb ends.  No bit
// that is not some leaf's is ever set.  Nothing waits: a step is one atomic OR.
template <class A>
RT_HD void group_climb(const A &a, int32_t v, uint32_t carry) {
  while (carry != 0u && v >= 0) {
    carry = group_climb_carry(a.fetch_or(v, carry), carry);
    v = a.parent(v);
  }
}

}  // namespace rtk
