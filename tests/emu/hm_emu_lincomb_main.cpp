// hm_emu_lincomb_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_lincomb.cpp: the per-thread core of hm_lincomb for
// every modulus of the chain given on the command line (logN, then 4 moduli), T in {1, 2, 3, 16}, the fills uniform, 0 and q - 1, the scalars 0, 1,
// q - 1 and random ones, the constants none, 0, q - 1 and random ones, with permuted input limbs and every chunk of every entry, compared with
// 128-bit integers.  T = 16 with fill, scalars and constant all q - 1 fills the accumulator as far as it can be filled.
// tests/test_emu_lincomb.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_lincomb(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *,
                           uint32_t, uint32_t, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t);
typedef unsigned __int128 u128;

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 q3\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, M = 4;
  uint64_t m[M];
  for (uint32_t i = 0; i < M; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  std::vector<uint32_t> chunks(N / 512);
  for (uint32_t i = 0; i < chunks.size(); ++i) chunks[i] = i;
  uint64_t x = 88172645463325252ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  int bad = 0, cases = 0;
  const uint32_t lo[M] = {3, 2, 0, 1}, ids[M] = {0, 1, 2, 3};
  for (uint32_t T : {1u, 2u, 3u, 16u})
    for (int fill = 0; fill < 3; ++fill)
      for (int sc = 0; sc < 4; ++sc)
        for (int kc = 0; kc < 4; ++kc) {    // 0: no addend list
          // entry i works under modulus i; term t of entry i sits at a permuted limb of a buffer of exactly M T limbs (7 is coprime to M T)
          std::vector<uint64_t> in((size_t)M * T * N), out((size_t)M * N), s((size_t)M * T), k(M);
          std::vector<uint32_t> li((size_t)M * T);
          for (uint32_t i = 0; i < M; ++i) {
            const uint64_t q = m[i];
            k[i] = kc == 2 ? q - 1 : kc == 3 ? next() % q : 0;
            for (uint32_t t = 0; t < T; ++t) {
              const uint32_t e = i * T + t;
              li[e] = (e * 7 + 3) % (M * T);
              s[e] = sc == 0 ? 0 : sc == 1 ? 1 : sc == 2 ? q - 1 : next() % q;
              for (uint32_t j = 0; j < N; ++j) in[(size_t)li[e] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
            }
          }
          if (emu_lincomb(m, M, logN, in.data(), li.data(), out.data(), lo, ids, M, T, s.data(), kc == 0 ? nullptr : k.data(), chunks.data(),
                          (uint32_t)chunks.size())) { printf("no context\n"); return 2; }
          ++cases;
          for (uint32_t i = 0; i < M; ++i) {
            const uint64_t q = m[i];
            for (uint32_t j = 0; j < N; ++j) {
              u128 e = k[i];
              for (uint32_t t = 0; t < T; ++t) e += (u128)s[i * T + t] * in[(size_t)li[i * T + t] * N + j] % q;
              if (out[(size_t)lo[i] * N + j] != (uint64_t)(e % q)) {
                if (bad < 10) printf("T=%u fill=%d scale=%d const=%d entry=%u j=%u\n", T, fill, sc, kc, i, j);
                ++bad;
              }
            }
          }
        }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
