// hm_emu_mlincomb.cpp — the per-thread core of hm_lincomb_multi (hm_rec_core.h: hm_lincomb_multi_thread and its helpers) on the CPU (TEST
// INFRASTRUCTURE, compiled by tests/test_emu_mlincomb.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same
// records the entry point builds (hm_lincomb_multi_fill_recs), the same per-modulus constants (hm_params.cpp), every thread of the chosen
// workgroups one after the other, for either built tile.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_mlincomb_generic() { return HM_GENERIC; }
extern "C" uint32_t emu_mlincomb_default_tile() { return HM_LINCOMB_MULTI_TILE; }
extern "C" uint32_t emu_mlincomb_rec_words(uint32_t T, uint32_t tile) { return HM_MLINCOMB_REC_WORDS(T, tile); }
extern "C" uint32_t emu_mlincomb_records(uint32_t M, uint32_t tile) { return hm_lincomb_multi_tiles(M, tile); }

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  Limb lists and constants as hm_lincomb_multi's;
// tile: 4 or 8; chunks[n_chunks]: the 512-coefficient chunks of every record to run (the outputs elsewhere are left as they are).  Returns 0, 1 if
// the moduli are refused, 2 for a tile that is not built.
extern "C" int emu_mlincomb(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *in, const uint32_t *li, uint64_t *out,
                            const uint32_t *lo, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t M, uint32_t tile, const uint64_t *scale,
                            const uint64_t *addend, const uint32_t *chunks, uint32_t n_chunks) {
  if (tile != 4 && tile != 8) return 2;
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return 1;
  }
  const uint32_t n_rec = n * hm_lincomb_multi_tiles(M, tile);
  std::vector<uint32_t> recs((size_t)n_rec * HM_MLINCOMB_REC_WORDS(T, tile));   // sized exactly: a record word read past the last slot ends a sanitizer build
  hm_lincomb_multi_fill_recs(recs.data(), li, lo, mod_ids, n, T, M, tile, scale, addend);
  HmLincombMultiArgs g;
  g.in = in; g.out = out;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n_rec; g.n_terms = T;
  for (uint32_t entry = 0; entry < n_rec; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) {
        if (tile == 8) hm_lincomb_multi_thread<8>(g, entry, chunks[k], tid);
        else hm_lincomb_multi_thread<4>(g, entry, chunks[k], tid);
      }
  return 0;
}
