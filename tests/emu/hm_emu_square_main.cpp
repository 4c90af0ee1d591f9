// hm_emu_square_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_square.cpp: the per-thread core of hm_tensor_square
// for every modulus of the chain given on the command line (logN, then 4 moduli), the fills uniform, 0 and q - 1, the scalars 1, 2, q - 1 and a
// random one, the constants 0, q - 1 and a random one, with permuted limb lists and every chunk of every entry, compared with 128-bit integers.
// tests/test_emu_square.py builds it with -fsanitize=address,undefined and runs it: every buffer is sized exactly, so a read or write past one
// ends the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" {
int emu_tensor_square(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, uint64_t *,
                      const uint32_t *, uint64_t *, const uint32_t *, uint64_t *, const uint32_t *, const uint32_t *, uint32_t, const uint64_t *,
                      const uint64_t *, const uint32_t *, uint32_t);
int emu_add_const_words(const uint64_t *, uint32_t, uint32_t, uint32_t, uint64_t, const uint64_t *, uint32_t, uint64_t *);
}
typedef unsigned __int128 u128;
static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }

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
  // entry i works under modulus i; its inputs and outputs sit at permuted limbs of buffers of exactly M limbs
  const uint32_t la[M] = {2, 0, 3, 1}, lc[M] = {1, 3, 0, 2}, l0[M] = {3, 2, 1, 0}, l1[M] = {0, 1, 2, 3}, l2[M] = {1, 0, 3, 2}, ids[M] = {0, 1, 2, 3};
  for (int fill = 0; fill < 3; ++fill)
    for (int sc = 0; sc < 5; ++sc)        // 4: no scale list
      for (int kc = 0; kc < 4; ++kc) {    // 3: no addend list
        std::vector<uint64_t> a((size_t)M * N), c((size_t)M * N), o0((size_t)M * N), o1((size_t)M * N), o2((size_t)M * N);
        uint64_t s[M], k[M];
        for (uint32_t i = 0; i < M; ++i) {
          const uint64_t q = m[i];
          s[i] = sc == 0 ? 1 : sc == 1 ? 2 : sc == 2 ? q - 1 : sc == 3 ? 1 + next() % (q - 1) : 1;
          k[i] = kc == 0 ? 0 : kc == 1 ? q - 1 : kc == 2 ? next() % q : 0;
          for (uint32_t j = 0; j < N; ++j) {
            a[(size_t)la[i] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
            c[(size_t)lc[i] * N + j] = fill == 0 ? next() % q : fill == 1 ? 0 : q - 1;
          }
        }
        if (emu_tensor_square(m, M, logN, a.data(), la, c.data(), lc, o0.data(), l0, o1.data(), l1, o2.data(), l2, ids, M, sc == 4 ? nullptr : s,
                              kc == 3 ? nullptr : k, chunks.data(), (uint32_t)chunks.size())) { printf("no context\n"); return 2; }
        ++cases;
        for (uint32_t i = 0; i < M; ++i) {
          const uint64_t q = m[i];
          for (uint32_t j = 0; j < N; ++j) {
            const uint64_t av = a[(size_t)la[i] * N + j], cv = c[(size_t)lc[i] * N + j];
            const uint64_t e0 = (uint64_t)(((u128)mulmod(mulmod(av, av, q), s[i], q) + k[i]) % q);
            const uint64_t e1 = (uint64_t)((u128)2 * mulmod(mulmod(av, cv, q), s[i], q) % q), e2 = mulmod(mulmod(cv, cv, q), s[i], q);
            if (o0[(size_t)l0[i] * N + j] != e0 || o1[(size_t)l1[i] * N + j] != e1 || o2[(size_t)l2[i] * N + j] != e2) {
              if (bad < 10) printf("fill=%d scale=%d const=%d entry=%u j=%u\n", fill, sc, kc, i, j);
              ++bad;
            }
          }
        }
      }
  // the element-wise opcode out = a + k
  for (uint32_t i = 0; i < M; ++i) {
    const uint64_t q = m[i];
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, q - 1, next() % q}) {
      std::vector<uint64_t> in = {0, 1, q - 1, q - 2, next() % q, next() % q}, out(in.size());
      if (emu_add_const_words(m, M, logN, i, k, in.data(), (uint32_t)in.size(), out.data())) { printf("no context\n"); return 2; }
      for (size_t j = 0; j < in.size(); ++j)
        if (out[j] != (uint64_t)(((u128)in[j] + k) % q)) { ++bad; printf("add_const mod=%u k=%llu j=%zu\n", i, (unsigned long long)k, j); }
    }
  }
  printf("cases=%d bad=%d\n", cases, bad);
  return bad != 0;
}
