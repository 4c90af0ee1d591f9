// hm_emu_identity_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_identity.cpp: the host-side table builder of
// hm_inner_product_lintrans_id (hm_ip_fill_recs + hm_ip_fill_lin + hm_ip_fill_multi + hm_ip_fill_id) and the identity form of the per-thread core
// at TERMS 1 / 4, n_rot 1 / 15, n_out 1 / 2 / 3 / 4 / 5 / 16, both tile sizes (and the single-sum core at n_out = 1), one entry with and one without an addend, each compared with the
// core without the identity step plus the element-wise ops.  tests/test_emu_identity.py builds it with -fsanitize=address,undefined and runs it:
// every table and buffer is sized exactly, so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <vector>
extern "C" int emu_ip_lintrans_id(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *,
    const uint32_t *, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, uint64_t *, uint64_t *, const uint32_t *, uint64_t *, uint64_t *, const uint32_t *,
    uint64_t *, uint64_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t *, const uint32_t *, uint32_t);
int main() {
  const uint32_t logN = 13, N = 1u << logN;
  const uint64_t moduli[2] = {1152921504606584833ull, 1152921504598720513ull};
  int bad = 0;
  for (uint32_t T : {1u, 4u}) for (uint32_t R : {1u, 15u}) for (uint32_t G : {1u, 2u, 3u, 4u, 5u, 16u}) for (uint32_t tile : {1u, 2u, 4u}) {
    if (tile == 1 && G != 1) continue;   // tile 1: the single-sum core, one output
    const uint32_t n = 2;
    // the identity plaintexts are limbs G * R * n .. of the plaintext buffer; entry 1 has no addend: its identity records are never read
    std::vector<uint64_t> X((size_t)n * T * N, 5), Y((size_t)R * n * 2 * T * N, 7), P((size_t)(G * R * n + G) * N, 3), A((size_t)1 * N, 9), A1((size_t)1 * N, 11);
    std::vector<uint64_t> out((size_t)G * n * 2 * N), out1(out.size()), ao((size_t)G * N), ao1(ao.size()), wo((size_t)G * N), wo1(wo.size());
    std::vector<uint32_t> xl(n * T), yl(R * n * 2 * T), pl(G * R * n), idl(G * n, 0xFFFFFFFFu), al = {0, 0xFFFFFFFFu}, a1l = {0, 0xFFFFFFFFu}, ol(G * n * 2),
        aol(G * n, 0xFFFFFFFFu), a1ol(G * n, 0xFFFFFFFFu), mods = {0, 1}, gal(R), chunks = {0, N / 512 - 1};
    for (size_t i = 0; i < xl.size(); ++i) xl[i] = i;
    for (size_t i = 0; i < yl.size(); ++i) yl[i] = i;
    for (size_t i = 0; i < pl.size(); ++i) pl[i] = i;
    for (size_t i = 0; i < ol.size(); ++i) ol[i] = i;
    for (uint32_t m = 0; m < G; ++m) { idl[m * n] = G * R * n + m; aol[m * n] = m; a1ol[m * n] = G - 1 - m; }
    uint64_t g = 1; for (uint32_t r = 0; r < R; ++r) { g = g * 5 % (2 * N); gal[r] = (uint32_t)g; }
    int rc = emu_ip_lintrans_id(moduli, 2, logN, X.data(), xl.data(), Y.data(), yl.data(), P.data(), pl.data(), idl.data(), A.data(), al.data(), A1.data(), a1l.data(),
        out.data(), out1.data(), ol.data(), ao.data(), ao1.data(), aol.data(), wo.data(), wo1.data(), a1ol.data(), mods.data(), n, T, R, G, tile, gal.data(), chunks.data(), 2);
    if (rc != 0 || out != out1 || ao != ao1 || wo != wo1 || wo[0] != 33) { ++bad; printf("T=%u R=%u G=%u tile=%u rc=%d\n", T, R, G, tile, rc); }
  }
  printf("bad=%d\n", bad);
  return bad != 0;
}
