// hm_emu_plincomb.cpp — the per-thread core of hm_plincomb (hm_rec_core.h: hm_plincomb_thread and its helpers) on the CPU (TEST INFRASTRUCTURE,
// compiled by tests/test_emu_plincomb.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same records the entry
// point builds (hm_plincomb_fill_recs), the same per-modulus constants (hm_params.cpp), every thread of the chosen workgroups one after the
// other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_plincomb_generic() { return HM_GENERIC; }
extern "C" uint32_t emu_plincomb_rec_words(uint32_t T) { return HM_PLINCOMB_REC_WORDS(T); }

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  Buffers and limb lists as hm_plincomb's (addend
// may be null: no addend, la is then not read); chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left
// as they are).  Returns 0, or 1 if the moduli are refused.
extern "C" int emu_plincomb(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *p, const uint32_t *lp, const uint64_t *x,
                            const uint32_t *lx0, const uint32_t *lx1, const uint64_t *addend, const uint32_t *la, uint64_t *out, const uint32_t *l0,
                            const uint32_t *l1, const uint32_t *mod_ids, uint32_t n, uint32_t T, const uint32_t *chunks, uint32_t n_chunks) {
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint32_t> recs((size_t)n * HM_PLINCOMB_REC_WORDS(T));   // sized exactly: a record word read past the last term ends a sanitizer build
  hm_plincomb_fill_recs(recs.data(), lp, lx0, lx1, addend != nullptr, la, l0, l1, mod_ids, n, T);
  HmPlincombArgs g;
  g.p = p; g.x = x; g.addend = addend ? addend : p; g.out = out;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n; g.n_terms = T;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_plincomb_thread(g, entry, chunks[k], tid);
  return 0;
}
