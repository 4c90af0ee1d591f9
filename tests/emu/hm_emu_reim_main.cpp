// hm_emu_reim_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_reim.cpp: the per-thread core of hm_reim_split for
// every modulus of the chain given on the command line (logN, then 4 moduli), the fills uniform, 0, q - 1 and x = y, with permuted input limbs
// and every chunk of every entry, compared with 128-bit integers against w on entries [0, N/2) and q - w on [N/2, N); w itself is checked to
// square to -1.  tests/test_emu_reim.py builds it with -fsanitize=address,undefined and runs it: every buffer, the record table included, is
// sized exactly, so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" int emu_reim(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, uint64_t *,
                        const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *, uint32_t, const uint32_t *, uint32_t, uint64_t *);
typedef unsigned __int128 u128;

int main(int argc, char **argv) {
  if (argc != 6) { printf("usage: %s logN q0 q1 q2 q3\n", argv[0]); return 2; }
  const uint32_t logN = (uint32_t)atoi(argv[1]), N = 1u << logN, M = 4;
  uint64_t m[M], w[M];
  for (uint32_t i = 0; i < M; ++i) m[i] = strtoull(argv[2 + i], nullptr, 10);
  std::vector<uint32_t> chunks(N / 512);
  for (uint32_t i = 0; i < chunks.size(); ++i) chunks[i] = i;
  uint64_t s = 88172645463325252ull;
  auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  int bad = 0, cases = 0;
  // entry i works under modulus i; x, y and the two outputs at permuted limbs of buffers of exactly M limbs
  const uint32_t lx[M] = {2, 0, 3, 1}, ly[M] = {1, 3, 0, 2}, lre[M] = {3, 2, 0, 1}, lim[M] = {0, 1, 2, 3}, ids[M] = {0, 1, 2, 3};
  for (int fill = 0; fill < 4; ++fill) {
    std::vector<uint64_t> x((size_t)M * N), y((size_t)M * N), re((size_t)M * N), im((size_t)M * N);
    for (uint32_t i = 0; i < M; ++i)
      for (uint32_t j = 0; j < N; ++j) {
        const uint64_t q = m[i];
        uint64_t &xv = x[(size_t)lx[i] * N + j], &yv = y[(size_t)ly[i] * N + j];
        xv = fill == 0 || fill == 3 ? next() % q : fill == 1 ? 0 : q - 1;
        yv = fill == 0 ? next() % q : fill == 1 ? 0 : fill == 2 ? q - 1 : xv;
      }
    if (emu_reim(m, M, logN, x.data(), lx, y.data(), ly, re.data(), lre, im.data(), lim, ids, M, chunks.data(), (uint32_t)chunks.size(), w)) {
      printf("no context\n");
      return 2;
    }
    ++cases;
    for (uint32_t i = 0; i < M; ++i) {
      const uint64_t q = m[i];
      if ((u128)w[i] * w[i] % q != q - 1) { printf("w^2 != -1 at modulus %u\n", i); ++bad; }
      for (uint32_t j = 0; j < N; ++j) {
        const uint64_t xv = x[(size_t)lx[i] * N + j], yv = y[(size_t)ly[i] * N + j], u = j < N / 2 ? w[i] : q - w[i];
        const uint64_t e_re = (uint64_t)(((u128)xv + yv) % q), e_im = (uint64_t)((u128)u * ((xv + q - yv) % q) % q);
        if (re[(size_t)lre[i] * N + j] != e_re || im[(size_t)lim[i] * N + j] != e_im) {
          if (bad < 10) printf("fill=%d entry=%u j=%u\n", fill, i, j);
          ++bad;
        }
      }
    }
  }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
