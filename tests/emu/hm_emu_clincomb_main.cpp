// hm_emu_clincomb_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_clincomb.cpp: the per-thread core of hm_clincomb for
// every modulus of the chain given on the command line (logN, then 4 moduli), T in {1, 2, 3, 16}, the fills uniform, 0 and q - 1, the scalars 0, 1,
// q - 1 and random ones in both parts (all 16 pairs), the constants none, 0, q - 1 and random ones in both parts, with permuted input limbs and every
// chunk of every entry, compared with 128-bit integers: entry e of a limb-poly meets v = psi^(N/2) for e < N/2 and q - v behind.  T = 16 with fill,
// real scalars and constant all q - 1 fills the accumulator as far as it can be filled.
// tests/test_emu_clincomb.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_clincomb(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *,
                            uint32_t, uint32_t, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t,
                            uint64_t *);
typedef unsigned __int128 u128;

static uint64_t powmod(uint64_t b, uint64_t e, uint64_t q) {
  uint64_t r = 1;
  for (; e; e >>= 1, b = (uint64_t)((u128)b * b % q))
    if (e & 1) r = (uint64_t)((u128)r * b % q);
  return r;
}

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 q3\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, M = 4;
  uint64_t m[M], psi[M], v[M];
  for (uint32_t i = 0; i < M; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  std::vector<uint32_t> chunks(N / 512);
  for (uint32_t i = 0; i < chunks.size(); ++i) chunks[i] = i;
  uint64_t x = 88172645463325252ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  auto pick = [&](int kind, uint64_t q) { return kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? q - 1 : next() % q; };
  int bad = 0, cases = 0;
  const uint32_t lo[M] = {3, 2, 0, 1}, ids[M] = {0, 1, 2, 3};
  for (uint32_t T : {1u, 2u, 3u, 16u})
    for (int fill = 0; fill < 3; ++fill)
      for (int sa = 0; sa < 4; ++sa)
        for (int sb = 0; sb < 4; ++sb)
          for (int kc = 0; kc < 4; ++kc) {    // 0: no addend lists
            // entry i works under modulus i; term t of entry i sits at a permuted limb of a buffer of exactly M T limbs (7 is coprime to M T)
            std::vector<uint64_t> in((size_t)M * T * N), out((size_t)M * N), a((size_t)M * T), b((size_t)M * T), kr(M), ki(M);
            std::vector<uint32_t> li((size_t)M * T);
            for (uint32_t i = 0; i < M; ++i) {
              const uint64_t q = m[i];
              kr[i] = kc ? pick(kc, q) : 0;
              ki[i] = kc ? pick(kc, q) : 0;
              for (uint32_t t = 0; t < T; ++t) {
                const uint32_t e = i * T + t;
                li[e] = (e * 7 + 3) % (M * T);
                a[e] = pick(sa, q);
                b[e] = pick(sb, q);
                for (uint32_t j = 0; j < N; ++j) in[(size_t)li[e] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
              }
            }
            if (emu_clincomb(m, M, logN, in.data(), li.data(), out.data(), lo, ids, M, T, a.data(), sb == 0 && (sa & 1) ? nullptr : b.data(),
                             kc == 0 ? nullptr : kr.data(), kc == 0 ? nullptr : ki.data(), chunks.data(), (uint32_t)chunks.size(), psi)) {
              printf("no context\n");
              return 2;
            }
            if (!cases)
              for (uint32_t i = 0; i < M; ++i) {
                v[i] = powmod(psi[i], N / 2, m[i]);
                if (powmod(psi[i], N, m[i]) != m[i] - 1 || (u128)v[i] * v[i] % m[i] != m[i] - 1) { printf("psi[%u] is no 2N-th root\n", i); return 2; }
              }
            ++cases;
            for (uint32_t i = 0; i < M; ++i) {
              const uint64_t q = m[i];
              for (uint32_t j = 0; j < N; ++j) {
                const uint64_t vv = j < N / 2 ? v[i] : q - v[i];
                u128 e = kr[i] + (u128)ki[i] * vv % q;
                for (uint32_t t = 0; t < T; ++t) {
                  const uint64_t s = (uint64_t)((a[i * T + t] + (u128)b[i * T + t] * vv) % q);
                  e += (u128)s * in[(size_t)li[i * T + t] * N + j] % q;
                }
                if (out[(size_t)lo[i] * N + j] != (uint64_t)(e % q)) {
                  if (bad < 10) printf("T=%u fill=%d re=%d im=%d const=%d entry=%u j=%u\n", T, fill, sa, sb, kc, i, j);
                  ++bad;
                }
              }
            }
          }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
