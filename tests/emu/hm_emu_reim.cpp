// hm_emu_reim.cpp — the per-thread core of hm_reim_split (hm_rec_core.h: hm_reim_thread) on the CPU (TEST INFRASTRUCTURE, compiled by
// tests/test_emu_reim.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same records the entry point builds
// (hm_reim_fill_recs) with the constant derived as the entry point derives it (w = q - psi^(N/2) from hm::Params::psi), the same per-modulus
// constants (hm_params.cpp), every thread of the chosen workgroups one after the other.  It is not a CPU backend: the product library never links
// or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_reim_generic() { return HM_GENERIC; }
extern "C" uint32_t emu_reim_rec_words() { return HM_REIM_REC_WORDS; }

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  Limb lists as hm_reim_split's;
// chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are); w_out[n_mods] (may be null):
// the constant of every modulus.  Returns 0, or 1 if the moduli are refused.
extern "C" int emu_reim(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *x, const uint32_t *lx, const uint64_t *y,
                        const uint32_t *ly, uint64_t *o_re, const uint32_t *lre, uint64_t *o_im, const uint32_t *lim, const uint32_t *mod_ids,
                        uint32_t n, const uint32_t *chunks, uint32_t n_chunks, uint64_t *w_out) {
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint64_t> qs(n), ws(n);
  for (uint32_t i = 0; i < n; ++i) {
    qs[i] = P.mod[mod_ids[i]];
    ws[i] = qs[i] - hm::powmod(P.psi[mod_ids[i]], P.N / 2, qs[i]);
  }
  if (w_out)
    for (uint32_t m = 0; m < n_mods; ++m) w_out[m] = P.mod[m] - hm::powmod(P.psi[m], P.N / 2, P.mod[m]);
  std::vector<uint32_t> recs((size_t)n * HM_REIM_REC_WORDS);   // sized exactly: a record word read past the end ends a sanitizer build
  hm_reim_fill_recs(recs.data(), lx, ly, lre, lim, mod_ids, ws.data(), qs.data(), n);
  HmReimArgs g;
  g.x = x; g.y = y; g.o_re = o_re; g.o_im = o_im;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_reim_thread(g, entry, chunks[k], tid);
  return 0;
}
