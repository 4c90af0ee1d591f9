// hm_emu_plincomb_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_plincomb.cpp: the per-thread core of hm_plincomb for
// every modulus of the chain given on the command line (logN, then 4 moduli), T in {1, 2, 3, 16}, the fills uniform, 0 and q - 1 for the plaintexts
// and for the ciphertexts independently (all 9 pairs), the addend none, 0, q - 1 and random, with permuted ciphertext limbs, a plaintext limb per
// (entry, term) and every chunk of every entry, compared with 128-bit integers.  T = 16 with everything q - 1 fills both accumulators as far as
// they can be filled.
// tests/test_emu_plincomb.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_plincomb(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *,
                            const uint64_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t,
                            const uint32_t *, uint32_t);
typedef unsigned __int128 u128;

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 q3\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, M = 4;
  uint64_t m[M];
  for (uint32_t i = 0; i < M; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  std::vector<uint32_t> chunks(N / 512);
  for (uint32_t i = 0; i < chunks.size(); ++i) chunks[i] = i;
  uint64_t s = 88172645463325252ull;
  auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  auto fill = [&](int kind, uint64_t q) { return kind == 0 ? next() % q : kind == 1 ? 0 : q - 1; };
  int bad = 0, cases = 0;
  // entry i works under modulus i; its outputs are limbs l0[i], l1[i] of a buffer of exactly 2 M limbs, its addend limb la[i] of one of M
  const uint32_t l0[M] = {3, 6, 0, 5}, l1[M] = {7, 2, 4, 1}, la[M] = {2, 0, 3, 1}, ids[M] = {0, 1, 2, 3};
  for (uint32_t T : {1u, 2u, 3u, 16u})
    for (int fp = 0; fp < 3; ++fp)
      for (int fx = 0; fx < 3; ++fx)
        for (int ka = 0; ka < 4; ++ka) {    // 0: no addend
          // term t of entry i: plaintext limb i T + t reversed, ciphertext limbs at a permutation of 2 M T (7 is coprime to it)
          std::vector<uint64_t> p((size_t)M * T * N), x((size_t)2 * M * T * N), add((size_t)M * N), out((size_t)2 * M * N);
          std::vector<uint32_t> lp((size_t)M * T), lx0((size_t)M * T), lx1((size_t)M * T);
          for (uint32_t i = 0; i < M; ++i) {
            const uint64_t q = m[i];
            for (uint32_t j = 0; j < N; ++j) add[(size_t)la[i] * N + j] = ka == 0 ? 0 : ka == 1 ? 0 : ka == 2 ? q - 1 : next() % q;
            for (uint32_t t = 0; t < T; ++t) {
              const uint32_t e = i * T + t;
              lp[e] = M * T - 1 - e;
              lx0[e] = (2 * e * 7 + 3) % (2 * M * T);
              lx1[e] = ((2 * e + 1) * 7 + 3) % (2 * M * T);
              for (uint32_t j = 0; j < N; ++j) {
                p[(size_t)lp[e] * N + j] = fill(fp, q);
                x[(size_t)lx0[e] * N + j] = fill(fx, q);
                x[(size_t)lx1[e] * N + j] = fill(fx, q);
              }
            }
          }
          if (emu_plincomb(m, M, logN, p.data(), lp.data(), x.data(), lx0.data(), lx1.data(), ka ? add.data() : nullptr, ka ? la : nullptr, out.data(), l0,
                           l1, ids, M, T, chunks.data(), (uint32_t)chunks.size())) {
            printf("no context\n");
            return 2;
          }
          ++cases;
          for (uint32_t i = 0; i < M; ++i) {
            const uint64_t q = m[i];
            for (uint32_t j = 0; j < N; ++j) {
              u128 e0 = ka ? add[(size_t)la[i] * N + j] : 0, e1 = 0;
              for (uint32_t t = 0; t < T; ++t) {
                const uint32_t e = i * T + t;
                const uint64_t pv = p[(size_t)lp[e] * N + j];
                e0 += (u128)pv * x[(size_t)lx0[e] * N + j] % q;
                e1 += (u128)pv * x[(size_t)lx1[e] * N + j] % q;
              }
              if (out[(size_t)l0[i] * N + j] != (uint64_t)(e0 % q) || out[(size_t)l1[i] * N + j] != (uint64_t)(e1 % q)) {
                if (bad < 10) printf("T=%u plain=%d ct=%d addend=%d entry=%u j=%u\n", T, fp, fx, ka, i, j);
                ++bad;
              }
            }
          }
        }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
