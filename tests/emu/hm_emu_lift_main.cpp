// hm_emu_lift_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_lift.cpp: the lifted forward first pass (MODE 10) in both
// geometries, for every ordered pair of moduli of the chain given on the command line (logN, then L + K = 4 moduli) and the fills uniform, 0, q_s - 1,
// (q_s - 1) / 2 and (q_s + 1) / 2.  The load routine's arithmetic is compared word by word with 128-bit integers, the lifted transform with the plain
// one (source modulus = target modulus: the identity lift) fed the separately centred and reduced input.  tests/test_emu_lift.py builds it with
// -fsanitize=address,undefined and runs it: every buffer is sized exactly, so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" {
void *emu_lift_create(uint32_t, uint32_t, uint32_t, const uint64_t *, const uint64_t *);
void emu_lift_destroy(void *);
uint64_t emu_lift_modulus(void *, uint32_t);
int emu_ntt_lift(void *, int, uint32_t, uint32_t, const uint64_t *, uint64_t *);
uint64_t emu_lift_word(void *, uint32_t, uint32_t, uint64_t);
}
static uint64_t centred_mod(uint64_t c, uint64_t qs, uint64_t q) {
  const __int128 v = c <= (qs - 1) / 2 ? (__int128)c : (__int128)c - (__int128)qs;
  const __int128 r = v % (__int128)q;
  return (uint64_t)(r < 0 ? r + (__int128)q : r);
}
int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 p0\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN;
  uint64_t m[4];
  for (int i = 0; i < 4; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  void *h = emu_lift_create(logN, 3, 1, m, m + 3);
  if (!h) { printf("no context\n"); return 2; }
  int bad = 0;
  for (uint32_t s = 0; s < 4; ++s)
    for (uint32_t d = 0; d < 4; ++d) {
      const uint64_t qs = emu_lift_modulus(h, s), q = emu_lift_modulus(h, d);
      for (int fill = 0; fill < 5; ++fill) {
        std::vector<uint64_t> in(N), red(N), o1(N), o2(N);
        uint64_t x = 88172645463325252ull + s * 7 + d;
        auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % qs; };
        const uint64_t fixed[5] = {0, 0, qs - 1, (qs - 1) / 2, (qs + 1) / 2};
        for (uint32_t i = 0; i < N; ++i) in[i] = fill ? fixed[fill] : next();
        for (uint32_t i = 0; i < N; ++i) {
          red[i] = centred_mod(in[i], qs, q);
          if (i < 64 && emu_lift_word(h, s, d, in[i]) != red[i]) { ++bad; printf("word s=%u d=%u fill=%d i=%u\n", s, d, fill, i); }
        }
        for (int ept : {16, 8}) {
          if (ept == 8 && logN < 15) continue;
          const int rc = emu_ntt_lift(h, ept, s, d, in.data(), o1.data()) | emu_ntt_lift(h, ept, d, d, red.data(), o2.data());
          if (rc || o1 != o2) { ++bad; printf("transform ept=%d s=%u d=%u fill=%d rc=%d\n", ept, s, d, fill, rc); }
        }
      }
    }
  // any word below 2^60, not only residues of the source modulus: the reduction's stated range
  for (uint32_t d = 0; d < 4; ++d) {
    const uint64_t q = emu_lift_modulus(h, d), top = (1ull << 60) - 1;
    for (uint64_t c : {top, top - 1, q, q - 1, 2 * q - 1 < top ? 2 * q - 1 : top, (top / q) * q, (top / q) * q - 1}) {
      // source = target: c is "positive" when c <= (q - 1) / 2, otherwise the routine computes c - q mod q = c mod q as well
      if (emu_lift_word(h, d, d, c) != c % q) { ++bad; printf("range d=%u c=%llu\n", d, (unsigned long long)c); }
    }
  }
  emu_lift_destroy(h);
  printf("bad=%d\n", bad);
  return bad != 0;
}
