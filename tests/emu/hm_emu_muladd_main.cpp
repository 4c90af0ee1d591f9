// hm_emu_muladd_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_muladd.cpp: the per-thread core of hm_tensor_muladd
// for every modulus of the chain given on the command line (logN, then 4 moduli), A in {0, 1, 2, 3, 8}, the fills uniform, 0 and q - 1, the
// scalars 1 (no scale list), 2, q - 1 and random ones, the addend scalars 0, 1, q - 1 and random ones, the constants none, 0, q - 1 and random
// ones, with permuted input limbs and every chunk of every entry, compared with 128-bit integers.  A = 8 with fill, scalars and constant all
// q - 1 fills the accumulators as far as they can be filled.
// tests/test_emu_muladd.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_muladd(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                          const uint32_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t,
                          uint32_t, const uint64_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t);
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
  // entry i works under modulus i and writes d0, d1, d2 to the limbs l0[i], l1[i], l2[i] of a buffer of exactly 3 M limbs
  const uint32_t l0[M] = {3, 2, 0, 1}, l1[M] = {7, 4, 5, 6}, l2[M] = {8, 11, 10, 9}, ids[M] = {0, 1, 2, 3};
  for (uint32_t A : {0u, 1u, 2u, 3u, 8u})
    for (int fill = 0; fill < 3; ++fill)
      for (int sc = 0; sc < 4; ++sc)        // 0: no scale list
        for (int uc = 0; uc < 4; ++uc)
          for (int kc = 0; kc < 4; ++kc) {  // 0: no addend list
            if (A == 0 && uc) continue;     // no addend scalars to vary
            // operand r of entry i sits at a permuted limb of a buffer of exactly M W limbs, W = 4 + 2A (7 is coprime to M W)
            const uint32_t W = 4 + 2 * A;
            std::vector<uint64_t> in((size_t)M * W * N), out((size_t)3 * M * N), s(M), u((size_t)M * A), k(M);
            std::vector<uint32_t> li((size_t)M * W), la(M), lb(M), lc(M), ld(M), lx0((size_t)M * A), lx1((size_t)M * A);
            for (uint32_t i = 0; i < M; ++i) {
              const uint64_t q = m[i];
              s[i] = sc == 1 ? 2 : sc == 2 ? q - 1 : sc == 3 ? 1 + next() % (q - 1) : 1;
              k[i] = kc == 2 ? q - 1 : kc == 3 ? next() % q : 0;
              for (uint32_t r = 0; r < W; ++r) {
                const uint32_t e = i * W + r;
                li[e] = (e * 7 + 3) % (M * W);
                for (uint32_t j = 0; j < N; ++j) in[(size_t)li[e] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
              }
              la[i] = li[i * W]; lb[i] = li[i * W + 1]; lc[i] = li[i * W + 2]; ld[i] = li[i * W + 3];
              for (uint32_t t = 0; t < A; ++t) {
                lx0[i * A + t] = li[i * W + 4 + 2 * t]; lx1[i * A + t] = li[i * W + 5 + 2 * t];
                u[i * A + t] = uc == 0 ? 0 : uc == 1 ? 1 : uc == 2 ? q - 1 : next() % q;
              }
            }
            if (emu_muladd(m, M, logN, in.data(), la.data(), lb.data(), lc.data(), ld.data(), A ? lx0.data() : nullptr, A ? lx1.data() : nullptr,
                           out.data(), l0, l1, l2, ids, M, A, sc == 0 ? nullptr : s.data(), A ? u.data() : nullptr, kc == 0 ? nullptr : k.data(),
                           chunks.data(), (uint32_t)chunks.size())) { printf("no context\n"); return 2; }
            ++cases;
            for (uint32_t i = 0; i < M; ++i) {
              const uint64_t q = m[i];
              for (uint32_t j = 0; j < N; ++j) {
                const u128 a = in[(size_t)la[i] * N + j], b = in[(size_t)lb[i] * N + j], c = in[(size_t)lc[i] * N + j], d = in[(size_t)ld[i] * N + j];
                u128 e0 = a * b % q * s[i] % q + k[i], e1 = (a * d % q + c * b % q) % q * s[i] % q, e2 = c * d % q * s[i] % q;
                for (uint32_t t = 0; t < A; ++t) {
                  e0 += (u128)u[i * A + t] * in[(size_t)lx0[i * A + t] * N + j] % q;
                  e1 += (u128)u[i * A + t] * in[(size_t)lx1[i * A + t] * N + j] % q;
                }
                if (out[(size_t)l0[i] * N + j] != (uint64_t)(e0 % q) || out[(size_t)l1[i] * N + j] != (uint64_t)(e1 % q) ||
                    out[(size_t)l2[i] * N + j] != (uint64_t)(e2 % q)) {
                  if (bad < 10) printf("A=%u fill=%d scale=%d addscale=%d const=%d entry=%u j=%u\n", A, fill, sc, uc, kc, i, j);
                  ++bad;
                }
              }
            }
          }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
