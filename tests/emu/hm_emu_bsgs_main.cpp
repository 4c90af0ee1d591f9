// hm_emu_bsgs_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over tests/emu/hm_emu_bsgs.cpp: the host-side table builder of
// hm_inner_product_lintrans_multi (hm_ip_fill_recs + hm_ip_fill_lin + hm_ip_fill_multi) and its per-thread core at TERMS 1 / 4, n_rot 1 / 3 / 16,
// n_out 1 / 4 / 5 / 16, both tile sizes, with and without addend, each compared with the single-sum core.  tests/test_emu_bsgs.py builds it
// with -fsanitize=address,undefined and runs it: every table and buffer is sized exactly, so a read or write past one ends the program.
#include <cstdint>
#include <cstdio>
#include <vector>
#include <random>
extern "C" int emu_ip_lintrans_multi(const uint64_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *,
    const uint64_t *, const uint32_t *, uint64_t *, uint64_t *, const uint32_t *, uint64_t *, uint64_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
    const uint32_t *, const uint32_t *, uint32_t);
int main() {
  const uint32_t logN = 13, N = 1u << logN;
  const uint64_t moduli[2] = {1152921504606584833ull, 1152921504598720513ull};
  int bad = 0;
  for (uint32_t T : {1u, 4u}) for (uint32_t R : {1u, 3u, 16u}) for (uint32_t G : {1u, 4u, 5u, 16u}) for (uint32_t tile : {2u, 4u}) for (int add = 0; add < 2; ++add) {
    const uint32_t n = 2;
    std::vector<uint64_t> X((size_t)n * T * N, 5), Y((size_t)R * n * 2 * T * N, 7), P((size_t)G * R * n * N, 3), A((size_t)n * N, 9);
    std::vector<uint64_t> out((size_t)G * n * 2 * N), out1(out.size()), ao((size_t)G * n * N), ao1(ao.size());
    std::vector<uint32_t> xl(n * T), yl(R * n * 2 * T), pl(G * R * n), al(n), ol(G * n * 2), aol(G * n), mods = {0, 1}, gal(R), chunks = {0, N / 512 - 1};
    for (size_t i = 0; i < xl.size(); ++i) xl[i] = i;
    for (size_t i = 0; i < yl.size(); ++i) yl[i] = i;
    for (size_t i = 0; i < pl.size(); ++i) pl[i] = i;
    for (size_t i = 0; i < ol.size(); ++i) ol[i] = i;
    for (size_t i = 0; i < aol.size(); ++i) aol[i] = i;
    al[0] = 0; al[1] = 0xFFFFFFFFu;
    uint64_t g = 1; for (uint32_t r = 0; r < R; ++r) { g = g * 5 % (2 * N); gal[r] = (uint32_t)g; }
    int rc = emu_ip_lintrans_multi(moduli, 2, logN, X.data(), xl.data(), Y.data(), yl.data(), P.data(), pl.data(), add ? A.data() : nullptr, add ? al.data() : nullptr,
        out.data(), out1.data(), ol.data(), add ? ao.data() : nullptr, add ? ao1.data() : nullptr, add ? aol.data() : nullptr, mods.data(), n, T, R, G, tile, gal.data(), chunks.data(), 2);
    if (rc != 0 || out != out1 || ao != ao1) { ++bad; printf("T=%u R=%u G=%u tile=%u add=%d rc=%d\n", T, R, G, tile, add, rc); }
  }
  printf("bad=%d\n", bad);
  return bad != 0;
}
