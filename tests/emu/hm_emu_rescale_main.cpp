// hm_emu_rescale_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_rescale.cpp: the product epilogue (MODE 8, with and
// without the mix prologue and the addend) and the product input of the inverse first pass (MODE 9) at N = 2^13 in the 16-coefficient geometry and at
// N = 2^15 in the 8-coefficient one, each compared with the existing pass fed a separately computed product.  tests/test_emu_rescale.py builds it
// with -fsanitize=address,undefined and runs it: every buffer is sized exactly, so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <vector>
extern "C" {
void *emu_rescale_create(uint32_t, uint32_t, uint32_t, const uint64_t *, const uint64_t *);
void emu_rescale_destroy(void *);
uint64_t emu_rescale_modulus(void *, uint32_t);
int emu_ntt_sub_scale_mul(void *, int, uint32_t, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, uint64_t *, uint64_t, const uint64_t *,
                          uint64_t, uint64_t);
int emu_intt_mul(void *, int, uint32_t, const uint64_t *, const uint64_t *, uint64_t *, uint64_t, int);
uint64_t emu_epi_mul(void *, uint32_t, uint64_t, uint64_t);
}
int main() {
  int bad = 0;
  for (int ept : {16, 8}) {
    const uint32_t logN = ept == 16 ? 13 : 15, N = 1u << logN;
    void *h = emu_rescale_create(logN, 2, 1, nullptr, nullptr);
    if (!h) { printf("no context\n"); return 2; }
    for (uint32_t mod = 0; mod < 3; ++mod) {
      const uint64_t q = emu_rescale_modulus(h, mod);
      std::vector<uint64_t> in(N), a(N), b(N), ab(N), d(N), mix(N), o1(N), o2(N);
      uint64_t s = 88172645463325252ull + mod;
      auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s % q; };
      for (uint32_t i = 0; i < N; ++i) { in[i] = next(); a[i] = i % 3 ? next() : q - 1; b[i] = i % 5 ? next() : q - 1; d[i] = next(); mix[i] = next(); }
      for (uint32_t i = 0; i < N; ++i) ab[i] = emu_epi_mul(h, mod, a[i], b[i]);
      for (int form = 0; form < 4; ++form) {   // bit 0: addend (with a constant), bit 1: mix prologue
        const uint64_t *ad = form & 1 ? d.data() : nullptr, *mx = form & 2 ? mix.data() : nullptr;
        int rc = emu_ntt_sub_scale_mul(h, ept, mod, in.data(), a.data(), b.data(), ad, o1.data(), 12345 % q, mx, mx ? q - 2 : 0, ad ? 777 : 0);
        rc |= emu_ntt_sub_scale_mul(h, ept, mod, in.data(), ab.data(), nullptr, ad, o2.data(), 12345 % q, mx, mx ? q - 2 : 0, ad ? 777 : 0);
        if (rc || o1 != o2) { ++bad; printf("forward ept=%d mod=%u form=%d rc=%d\n", ept, mod, form, rc); }
      }
      int rc = emu_intt_mul(h, ept, mod, a.data(), b.data(), o1.data(), 999, 1) | emu_intt_mul(h, ept, mod, ab.data(), nullptr, o2.data(), 999, 1);
      if (rc || o1 != o2) { ++bad; printf("inverse ept=%d mod=%u rc=%d\n", ept, mod, rc); }
    }
    emu_rescale_destroy(h);
  }
  printf("bad=%d\n", bad);
  return bad != 0;
}
