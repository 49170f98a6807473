// The per-sphere rule of the along-ray queries (query_core.h: sweep_contact_roots, what along_lane runs at a leaf) on the host, over cases read
// from a file: the CPU suite holds the numpy restatement (tests/along_ref.py: rule_cases) equal to this arithmetic bit for bit, without a GPU,
// and this program holds sweep_contact_roots' kind and tau equal to sweep_contact's on every case (exit status 1 where they differ).
// A case is 13 float32, as tools/sweep_check.cpp's: ray origin xyz, direction xyz, sphere centre xyz, sphere radius, query radius, t_min, t_max.
// For each case five uint32 are written: the kind (0 none, 1 entry contact, 2 overlap at the start), tau's bits (0 for none), whether the roots
// were written (the discriminant is not <= 0), and the bits of t1 and t2 (0 where they were not written).
// usage: along_check <cases.bin> <out.bin>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "query_core.h"

using namespace rtk;

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: along_check <cases.bin> <out.bin>\n");
    return 2;
  }
  FILE *in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "along_check: cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<float> cases;
  float row[13];
  while (fread(row, sizeof(float), 13, in) == 13) cases.insert(cases.end(), row, row + 13);
  fclose(in);
  const size_t n = cases.size() / 13;
  std::vector<uint32_t> out(5 * n);
  size_t kinds[3] = {0, 0, 0}, differ = 0;
  for (size_t i = 0; i < n; ++i) {
    const float *c = &cases[13 * i];
    Ray r;
    r.ox = c[0]; r.oy = c[1]; r.oz = c[2];
    r.dx = c[3]; r.dy = c[4]; r.dz = c[5];
    ray_derive(r);
    float tau = 0.0f, t1 = 0.0f, t2 = 0.0f, tau0 = 0.0f, u1, u2;
    const int kind = sweep_contact_roots(r, c[6], c[7], c[8], c[9], c[10], c[11], c[12], &tau, &t1, &t2);
    const int kind0 = sweep_contact(r, c[6], c[7], c[8], c[9], c[10], c[11], c[12], &tau0);
    const bool good = sphere_roots(r, c[6], c[7], c[8], c[9] + c[10], &u1, &u2);
    if (kind == kSweepNone) tau = 0.0f;
    if (kind0 == kSweepNone) tau0 = 0.0f;
    if (!good) t1 = t2 = 0.0f;
    if (kind != kind0 || memcmp(&tau, &tau0, 4) != 0) differ += 1;
    out[5 * i] = static_cast<uint32_t>(kind);
    memcpy(&out[5 * i + 1], &tau, 4);
    out[5 * i + 2] = good ? 1u : 0u;
    memcpy(&out[5 * i + 3], &t1, 4);
    memcpy(&out[5 * i + 4], &t2, 4);
    kinds[kind] += 1;
  }
  FILE *o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), sizeof(uint32_t), out.size(), o) != out.size()) {
    fprintf(stderr, "along_check: cannot write %s\n", argv[2]);
    return 2;
  }
  fclose(o);
  printf("%zu cases: %zu none, %zu entry contacts, %zu overlaps at the start; %zu differ from sweep_contact\n", n, kinds[0], kinds[1], kinds[2],
         differ);
  return differ ? 1 : 0;
}
