// box_hit_presorted on sign-ordered operands against box_hit_interval (lane_core.h), the way the pooled kernel's PRESORT instantiations use
// it: the ray's sign_offsets word picks the near / far dwords out of a record packed by presort_pack, at `entry + (w & d)` and
// `entry + ((w ^ kSignAll) & d)`.  Checked on every case:
//   * the predicate equals box_hit_interval's, for both children of the record, over (0, 1e9) and over a second, case-dependent interval;
//   * the dword read as near_k is bit for bit (r.i_k < 0.0f ? hi_k : lo_k), far_k the other one;
//   * the offset word has the axis's bit exactly when r.i_k < 0.0f (so -inf selects hi; +inf, +-0 and NaN select lo).
// Cases: the cross product of a list of special values (+-0, denormals, +-inf, NaN of both signs, slab-aligned origins, huge and tiny
// magnitudes) per axis, and seeded random cases drawn from raw bit patterns and from scene-like ranges.
// usage: box_presorted_check <random cases> <seed> [1: derive the offsets from the SIGN BIT of 1/d instead of the compare -- must fail]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "lane_core.h"

using namespace rtk;

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static long n_cases = 0, bad_pred = 0, bad_operand = 0, bad_offset = 0;
static bool use_sign_bit = false;

static float rec_read(const uint32_t *cell, int byte, int child) { return from_bits(cell[byte / 4 + child]); }

static void check(const float o[3], const float d[3], const float lo[3], const float hi[3], float tlo2, float thi2) {
  Ray r;
  r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
  r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
  ray_derive(r);
  uint32_t w = sign_offsets(r);
  if (use_sign_bit) w = ((bits(r.ix) >> 31) ? kSignX : 0u) | ((bits(r.iy) >> 31) ? kSignY : 0u) | ((bits(r.iz) >> 31) ? kSignZ : 0u);
  const float inv[3] = {r.ix, r.iy, r.iz};
  const uint32_t dist[3] = {kSignX, kSignY, kSignZ};
  const int entry[3] = {kPsX, kPsY, kPsZ};
  // the record: this box as the left child, the box with lo and hi exchanged as the right one
  uint32_t cell[kPsNodeBytes / 4];
  presort_pack(cell, lo, hi, hi, lo, 0x1234500u, 0xfffffe00u);
  n_cases++;
  if (cell[kPsRefs / 4] != 0x1234500u || cell[kPsRefs / 4 + 1] != 0xfffffe00u) bad_operand++;
  for (int child = 0; child < 2; ++child) {
    const float *blo = child ? hi : lo, *bhi = child ? lo : hi;
    float nr[3], fr[3];
    for (int k = 0; k < 3; ++k) {
      const bool neg = inv[k] < 0.0f;
      if (((w & dist[k]) != 0u) != neg) bad_offset++;
      nr[k] = rec_read(cell, entry[k] + (int)(w & dist[k]), child);
      fr[k] = rec_read(cell, entry[k] + (int)((w ^ kSignAll) & dist[k]), child);
      if (bits(nr[k]) != bits(neg ? bhi[k] : blo[k]) || bits(fr[k]) != bits(neg ? blo[k] : bhi[k])) bad_operand++;
    }
    const bool want1 = box_hit_interval(r, blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], 0.0f, kTMax);
    const bool got1 = box_hit_presorted(r, nr[0], fr[0], nr[1], fr[1], nr[2], fr[2], 0.0f, kTMax);
    const bool want2 = box_hit_interval(r, blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], tlo2, thi2);
    const bool got2 = box_hit_presorted(r, nr[0], fr[0], nr[1], fr[1], nr[2], fr[2], tlo2, thi2);
    if (want1 != got1 || want2 != got2) {
      if (bad_pred < 5)
        printf("MISMATCH predicate: o %a %a %a d %a %a %a lo %a %a %a hi %a %a %a child %d\n", o[0], o[1], o[2], d[0], d[1], d[2], lo[0], lo[1],
               lo[2], hi[0], hi[1], hi[2], child);
      bad_pred++;
    }
  }
}

int main(int argc, char **argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 1000000;
  const unsigned seed = argc > 2 ? (unsigned)atol(argv[2]) : 1u;
  use_sign_bit = argc > 3 && atoi(argv[3]) == 1;
  const float inf = __builtin_inff(), qnan = from_bits(0x7fc00000u), nnan = from_bits(0xffc00001u);
  const float den = from_bits(1u), den2 = from_bits(0x00400000u), fmin_n = from_bits(0x00800000u), fmax_n = from_bits(0x7f7fffffu);
  // direction components (1 / d: +-inf from +-0, +-0 from +-inf, overflow to inf from denormals, NaN), origins, bounds
  const std::vector<float> dirs = {0.0f, -0.0f, 1.0f, -1.0f, 0.3f, -0.7f, den, -den, den2, -den2, fmin_n, -fmin_n, fmax_n, -fmax_n, inf, -inf, qnan, nnan};
  const std::vector<float> orgs = {0.0f, -0.0f, 1.0f, -1.0f, 2.5f, den, -den, fmax_n, -fmax_n, inf, -inf, qnan};
  const std::vector<float> bnds = {0.0f, -0.0f, 1.0f, -1.0f, 2.5f, -3.0f, den, -den, den2, fmax_n, -fmax_n, inf, -inf, qnan, nnan};
  std::mt19937 rng(seed);
  auto pick = [&](const std::vector<float> &v) { return v[rng() % v.size()]; };
  // (1) one axis runs through the whole cross product (origins equal to a bound included: lo - o = 0 against 1 / d = +-inf gives NaN
  // products); the other two axes draw from the same lists
  for (int axis = 0; axis < 3; ++axis)
    for (float dk : dirs)
      for (float ok : orgs)
        for (float lk : bnds)
          for (float hk : bnds) {
            float o[3], d[3], lo[3], hi[3];
            for (int k = 0; k < 3; ++k) {
              const bool benign = (rng() & 1u) != 0u;
              d[k] = benign ? (k == 1 ? -0.5f : 0.25f) : pick(dirs);
              o[k] = benign ? 0.5f : pick(orgs);
              lo[k] = benign ? -4.0f : pick(bnds);
              hi[k] = benign ? 4.0f : pick(bnds);
            }
            d[axis] = dk; o[axis] = ok; lo[axis] = lk; hi[axis] = hk;
            check(o, d, lo, hi, 0.25f, 8.0f);
          }
  const long n_special = n_cases;
  // (2) slab-aligned origins with zero direction components, all sign combinations, every axis subset
  for (int m = 0; m < 64; ++m)
    for (int sub = 0; sub < 27; ++sub) {
      float o[3], d[3], lo[3] = {-1.0f, -2.0f, -3.0f}, hi[3] = {1.0f, 2.0f, 3.0f};
      int s = sub;
      for (int k = 0; k < 3; ++k, s /= 3) {
        const int zero = (m >> (2 * k)) & 3;   // 0: +0, 1: -0, 2: positive, 3: negative
        d[k] = zero == 0 ? 0.0f : zero == 1 ? -0.0f : zero == 2 ? 0.5f : -0.5f;
        o[k] = s % 3 == 0 ? lo[k] : s % 3 == 1 ? hi[k] : 0.0f;
      }
      check(o, d, lo, hi, 0.0f, 4.0f);
    }
  // (3) seeded random cases: raw bit patterns (every class of value), and scene-like rays against scene-like boxes
  std::uniform_real_distribution<float> pos(-20.0f, 20.0f), ext(0.0f, 6.0f), dir(-1.0f, 1.0f);
  for (long i = 0; i < n_random; ++i) {
    float o[3], d[3], lo[3], hi[3];
    const int kind = (int)(rng() % 4u);
    for (int k = 0; k < 3; ++k) {
      if (kind == 0) {
        o[k] = from_bits(rng()); d[k] = from_bits(rng()); lo[k] = from_bits(rng()); hi[k] = from_bits(rng());
      } else {
        o[k] = pos(rng); d[k] = dir(rng); lo[k] = pos(rng); hi[k] = lo[k] + ext(rng);
        if (kind == 2 && (rng() % 3u) == 0u) d[k] = (rng() & 1u) ? 0.0f : -0.0f;
        if (kind == 3 && (rng() % 3u) == 0u) o[k] = (rng() & 1u) ? lo[k] : hi[k];
        if (kind == 3 && (rng() % 5u) == 0u) d[k] = (rng() & 1u) ? 0.0f : -0.0f;
      }
    }
    const float tlo2 = kind == 1 ? 0.0f : 0.5f, thi2 = kind == 1 ? 30.0f : 1000.0f;
    check(o, d, lo, hi, tlo2, thi2);
  }
  printf("%ld cases (%ld special, %ld random, seed %u): %ld predicate, %ld operand, %ld offset mismatches\n", n_cases, n_special, n_cases - n_special - 64 * 27,
         seed, bad_pred, bad_operand, bad_offset);
  return (bad_pred || bad_operand || bad_offset) ? 1 : 0;
}
