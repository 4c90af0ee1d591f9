// hm_emu_mlincomb_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_mlincomb.cpp: the per-thread core of
// hm_lincomb_multi for every modulus of the chain given on the command line (logN, then 4 moduli), both built tiles, T in {1, 2, 3, 16}, M in
// {1, tile - 1, tile, tile + 1, 16}, the fills uniform, 0 and q - 1, the scalars 0, 1, q - 1 and random ones, the constants none, 0, q - 1 and
// random ones, with permuted input limbs, the first and the last chunk of every record, compared with 128-bit integers; the chunks that did not run
// keep their guard value.  T = 16 with fill, scalars and constants all q - 1 fills every accumulator as far as it can be filled.
// tests/test_emu_mlincomb.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is sized exactly,
// so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_mlincomb(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *,
                            uint32_t, uint32_t, uint32_t, uint32_t, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t);
typedef unsigned __int128 u128;

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 q3\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, E = 4;
  const uint64_t GUARD = 0xDEADBEEFDEADBEEFull;
  uint64_t m[E];
  for (uint32_t i = 0; i < E; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  const uint32_t chunks[2] = {0, N / 512 - 1}, ids[E] = {0, 1, 2, 3};
  uint64_t x = 88172645463325252ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  int bad = 0, cases = 0;
  for (uint32_t tile : {4u, 8u})
    for (uint32_t T : {1u, 2u, 3u, 16u})
      for (uint32_t M : {1u, tile - 1, tile, tile + 1, 16u})
        for (int fill = 0; fill < 3; ++fill)
          for (int sc = 0; sc < 4; ++sc)
            for (int kc = 0; kc < 4; ++kc) {    // 0: no addend list
              // entry i works under modulus i; term t of entry i sits at a permuted limb of a buffer of exactly E T limbs (7 is coprime to E T), output
              // m of entry i at a permuted limb of a buffer of exactly E M limbs (11 is coprime to E M)
              std::vector<uint64_t> in((size_t)E * T * N), out((size_t)E * M * N, GUARD), s((size_t)E * M * T), k((size_t)E * M);
              std::vector<uint32_t> li((size_t)E * T), lo((size_t)E * M);
              for (uint32_t i = 0; i < E; ++i) {
                const uint64_t q = m[i];
                for (uint32_t t = 0; t < T; ++t) {
                  const uint32_t e = i * T + t;
                  li[e] = (e * 7 + 3) % (E * T);
                  for (uint32_t j = 0; j < N; ++j) in[(size_t)li[e] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
                }
                for (uint32_t o = 0; o < M; ++o) {
                  const uint32_t e = i * M + o;
                  lo[e] = (e * 11 + 1) % (E * M);
                  k[e] = kc == 2 ? q - 1 : kc == 3 ? next() % q : 0;
                  for (uint32_t t = 0; t < T; ++t) s[(size_t)e * T + t] = sc == 0 ? 0 : sc == 1 ? 1 : sc == 2 ? q - 1 : next() % q;
                }
              }
              if (emu_mlincomb(m, E, logN, in.data(), li.data(), out.data(), lo.data(), ids, E, T, M, tile, s.data(), kc == 0 ? nullptr : k.data(),
                               chunks, 2)) { printf("no context\n"); return 2; }
              ++cases;
              for (uint32_t i = 0; i < E; ++i) {
                const uint64_t q = m[i];
                for (uint32_t o = 0; o < M; ++o) {
                  const uint32_t e = i * M + o;
                  for (uint32_t j = 0; j < N; ++j) {
                    u128 want = GUARD;
                    if (j < 512 || j >= N - 512) {
                      want = k[e];
                      for (uint32_t t = 0; t < T; ++t) want += (u128)s[(size_t)e * T + t] * in[(size_t)li[i * T + t] * N + j] % q;
                      want %= q;
                    }
                    if (out[(size_t)lo[e] * N + j] != (uint64_t)want) {
                      if (bad < 10) printf("tile=%u T=%u M=%u fill=%d scale=%d const=%d entry=%u out=%u j=%u\n", tile, T, M, fill, sc, kc, i, o, j);
                      ++bad;
                    }
                  }
                }
              }
            }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
