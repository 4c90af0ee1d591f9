// hm_emu_slots_main.cpp — the slot transform of hm_emu_slots.cpp as a program of its own (TEST INFRASTRUCTURE: tests/test_emu_slots.py compiles it
// with -fsanitize=address,undefined and runs it as a process; nothing of it is loaded into Python).  Every buffer is a std::vector of exactly the
// size the transform may touch, so an index beyond a tile, a vector or a limb-poly is reported.
//   usage: hm_emu_slots_main <logN> <log2 scale> <modulus>
// Per fill (uniform in the unit disc, one slot at 0 / 1 / n - 1, all ones, all zero) and for n_vec = 2: encode, no overflow, decode, and every slot
// back within N / 2 / scale plus 1e-9 for the two double transforms; then a fill beyond half the modulus must raise the flag and store zeros.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {
int emu_slots_encode(uint32_t logN, const double *z, uint32_t n_vec, double scale, uint64_t q, uint64_t *coef, uint32_t *overflow);
int emu_slots_decode(uint32_t logN, const uint64_t *coef, uint32_t n_vec, double scale, uint64_t q, double *z);
}

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s <logN> <log2 scale> <modulus>\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]);
  const double scale = ldexp(1.0, atoi(argv[2]));
  const uint64_t q = strtoull(argv[3], nullptr, 10);
  const size_t N = (size_t)1 << logN, n = N / 2;
  const uint32_t n_vec = 2;
  int bad = 0;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto uni = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  const char *fills[] = {"uniform", "slot0", "slot1", "slot_last", "ones", "zero"};
  for (int f = 0; f < 6; ++f) {
    std::vector<double> z(2 * n * n_vec, 0.0), back(2 * n * n_vec, -7.0);
    for (uint32_t v = 0; v < n_vec; ++v) {
      double *zv = z.data() + 2 * n * v;
      if (f == 0) for (size_t j = 0; j < n; ++j) { zv[2 * j] = uni() * 0.7; zv[2 * j + 1] = uni() * 0.7; }
      if (f == 1) { zv[0] = 1.0; zv[1] = -0.5; }
      if (f == 2) { zv[2] = -1.0; zv[3] = 0.25; }
      if (f == 3) { zv[2 * (n - 1)] = 0.5; zv[2 * (n - 1) + 1] = 1.0; }
      if (f == 4) for (size_t j = 0; j < n; ++j) zv[2 * j] = 1.0;
    }
    std::vector<uint64_t> coef(N * n_vec, ~0ull);
    uint32_t ovf = 7;
    if (emu_slots_encode(logN, z.data(), n_vec, scale, q, coef.data(), &ovf) || ovf) { printf("%s: encode failed or overflowed (%u)\n", fills[f], ovf); ++bad; continue; }
    for (uint64_t c : coef) if (c >= q) { printf("%s: a coefficient is not reduced\n", fills[f]); ++bad; break; }
    if (emu_slots_decode(logN, coef.data(), n_vec, scale, q, back.data())) { printf("%s: decode failed\n", fills[f]); ++bad; continue; }
    double worst = 0;
    for (size_t i = 0; i < z.size(); i += 2) worst = std::fmax(worst, std::hypot(back[i] - z[i], back[i + 1] - z[i + 1]));
    if (!(worst <= (double)N / 2 / scale + 1e-9)) { printf("%s: round trip off by %g\n", fills[f], worst); ++bad; }
  }
  {   // every coefficient of the constant slot vector's encoding but the first is 0; the first is scale * v: beyond half the modulus
    std::vector<double> z(2 * n, 0.0);
    for (size_t j = 0; j < n; ++j) z[2 * j] = (double)q / scale;
    std::vector<uint64_t> coef(N, ~0ull);
    uint32_t ovf = 0;
    if (emu_slots_encode(logN, z.data(), 1, scale, q, coef.data(), &ovf) || ovf != 1 || coef[0] != 0) { printf("overflow: flag %u, word %llu\n", ovf, (unsigned long long)coef[0]); ++bad; }
  }
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
