// hm_emu_dotadd_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_dotadd.cpp: the per-thread core of hm_tensor_dotadd
// for every modulus of the chain given on the command line (logN, then 4 moduli, then "all" or "few"), (T, A) in {(1,0), (1,1), (2,1), (2,2),
// (3,3), (16,8)}, the fills uniform, 0 and q - 1 independently for the operands of the pairs and for the addends, the pair scalars 1 (no scale
// list), 2, q - 1, random ones and a mix within one record (1, 2, q - 1, random by pair), the addend scalars 0, 1, q - 1 and random ones, the
// constants none, 0, q - 1 and random ones, with permuted input limbs, on the first, a middle and the last chunk of every entry, compared with
// 128-bit integers; the output limbs outside those chunks keep their guard value.  (16, 8) with both fills, every scalar and the constant q - 1
// fills the accumulators as far as they can be filled.  "few": the shapes (2,1) and (3,3) with uniform fills only (the large ring).
// tests/test_emu_dotadd.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern "C" int emu_dotadd(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                          const uint32_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t,
                          uint32_t, uint32_t, const uint64_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t);
typedef unsigned __int128 u128;
static const uint64_t GUARD = 0xDEADBEEFDEADBEEFull;

int main(int argc, char **argv) {
  if (argc != 7) { printf("usage: %s logN q0 q1 q2 q3 all|few\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, M = 4;
  const bool few = !strcmp(argv[6], "few");
  uint64_t m[M];
  for (uint32_t i = 0; i < M; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  const std::vector<uint32_t> chunks = {0, N / 1024, N / 512 - 1};
  uint64_t x = 88172645463325252ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  int bad = 0, cases = 0;
  // entry i works under modulus i and writes d0, d1, d2 to the limbs l0[i], l1[i], l2[i] of a buffer of exactly 3 M limbs
  const uint32_t l0[M] = {3, 2, 0, 1}, l1[M] = {7, 4, 5, 6}, l2[M] = {8, 11, 10, 9}, ids[M] = {0, 1, 2, 3};
  const uint32_t shapes[6][2] = {{1, 0}, {1, 1}, {2, 1}, {2, 2}, {3, 3}, {16, 8}};
  for (const auto &shape : shapes) {
    const uint32_t T = shape[0], A = shape[1], W = 4 * T + 2 * A;
    if (few && !((T == 2 && A == 1) || (T == 3 && A == 3))) continue;
    // sized exactly, once per shape: only the chunks that run are ever written or read, the rest stays zero
    std::vector<uint64_t> in((size_t)M * W * N), out((size_t)3 * M * N);
    for (int fillP = 0; fillP < (few ? 1 : 3); ++fillP)
      for (int fillA = 0; fillA < (few ? 1 : 3); ++fillA)
        for (int sc = 0; sc < 5; ++sc)        // 0: no scale list, 4: mixed within the record
          for (int uc = 0; uc < 4; ++uc)
            for (int kc = 0; kc < 4; ++kc) {  // 0: no addend list
              if (A == 0 && (uc || fillA)) continue;     // no addends to vary
              // operand r of entry i sits at a permuted limb of a buffer of exactly M W limbs (7 is coprime to M W for every shape of the list: W = 4, 6, 10, 12, 18, 80)
              std::fill(out.begin(), out.end(), GUARD);
              std::vector<uint64_t> s((size_t)M * T), u((size_t)M * A), k(M);
              std::vector<uint32_t> li((size_t)M * W), la((size_t)M * T), lb((size_t)M * T), lc((size_t)M * T), ld((size_t)M * T), lx0((size_t)M * A),
                  lx1((size_t)M * A);
              for (uint32_t i = 0; i < M; ++i) {
                const uint64_t q = m[i];
                k[i] = kc == 2 ? q - 1 : kc == 3 ? next() % q : 0;
                for (uint32_t r = 0; r < W; ++r) {
                  const uint32_t e = i * W + r;
                  const int fill = r < 4 * T ? fillP : fillA;
                  li[e] = (e * 7 + 3) % (M * W);
                  for (uint32_t ch : chunks)
                    for (uint32_t j = ch * 512; j < ch * 512 + 512; ++j) in[(size_t)li[e] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
                }
                for (uint32_t t = 0; t < T; ++t) {
                  const int kind = sc == 4 ? (int)(t % 4) : sc;
                  s[i * T + t] = kind == 1 ? 2 : kind == 2 ? q - 1 : kind == 3 ? 1 + next() % (q - 1) : 1;
                  la[i * T + t] = li[i * W + 4 * t]; lb[i * T + t] = li[i * W + 4 * t + 1]; lc[i * T + t] = li[i * W + 4 * t + 2]; ld[i * T + t] = li[i * W + 4 * t + 3];
                }
                for (uint32_t t = 0; t < A; ++t) {
                  lx0[i * A + t] = li[i * W + 4 * T + 2 * t]; lx1[i * A + t] = li[i * W + 4 * T + 2 * t + 1];
                  u[i * A + t] = uc == 0 ? 0 : uc == 1 ? 1 : uc == 2 ? q - 1 : next() % q;
                }
              }
              if (emu_dotadd(m, M, logN, in.data(), la.data(), lb.data(), lc.data(), ld.data(), A ? lx0.data() : nullptr, A ? lx1.data() : nullptr,
                             out.data(), l0, l1, l2, ids, M, T, A, sc == 0 ? nullptr : s.data(), A ? u.data() : nullptr, kc == 0 ? nullptr : k.data(),
                             chunks.data(), (uint32_t)chunks.size())) { printf("no context\n"); return 2; }
              ++cases;
              for (uint32_t i = 0; i < M; ++i) {
                const uint64_t q = m[i];
                for (uint32_t j = 0; j < N; ++j) {
                  const bool ran = j / 512 == chunks[0] || j / 512 == chunks[1] || j / 512 == chunks[2];
                  const uint64_t g0 = out[(size_t)l0[i] * N + j], g1 = out[(size_t)l1[i] * N + j], g2 = out[(size_t)l2[i] * N + j];
                  bool ok;
                  if (!ran) {
                    ok = g0 == GUARD && g1 == GUARD && g2 == GUARD;
                  } else {
                    u128 e0 = k[i], e1 = 0, e2 = 0;
                    for (uint32_t t = 0; t < T; ++t) {
                      const u128 a = in[(size_t)la[i * T + t] * N + j], b = in[(size_t)lb[i * T + t] * N + j], c = in[(size_t)lc[i * T + t] * N + j],
                                 d = in[(size_t)ld[i * T + t] * N + j], st = s[i * T + t];
                      e0 += a * b % q * st % q; e1 += (a * d % q + c * b % q) % q * st % q; e2 += c * d % q * st % q;
                    }
                    for (uint32_t t = 0; t < A; ++t) {
                      e0 += (u128)u[i * A + t] * in[(size_t)lx0[i * A + t] * N + j] % q;
                      e1 += (u128)u[i * A + t] * in[(size_t)lx1[i * A + t] * N + j] % q;
                    }
                    ok = g0 == (uint64_t)(e0 % q) && g1 == (uint64_t)(e1 % q) && g2 == (uint64_t)(e2 % q);
                  }
                  if (!ok) {
                    if (bad < 10) printf("T=%u A=%u fills=%d,%d scale=%d addscale=%d const=%d entry=%u j=%u\n", T, A, fillP, fillA, sc, uc, kc, i, j);
                    ++bad;
                  }
                }
              }
            }
  }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
