// hm_emu_clincomb.cpp — the per-thread core of hm_clincomb (hm_rec_core.h: hm_clincomb_thread and its helpers) on the CPU (TEST INFRASTRUCTURE,
// compiled by tests/test_emu_clincomb.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same records the entry
// point builds (hm_clincomb_fill_recs, from psi^(N/2) of the same root table), the same per-modulus constants (hm_params.cpp), every thread of the
// chosen workgroups one after the other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_clincomb_generic() { return HM_GENERIC; }
extern "C" uint32_t emu_clincomb_rec_words(uint32_t T) { return HM_CLINCOMB_REC_WORDS(T); }

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  Limb lists and constants as hm_clincomb's (im,
// add_re, add_im may be null); chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are);
// psi_out[n_mods] (may be null) receives the 2N-th roots the records were built from.  Returns 0, or 1 if the moduli are refused.
extern "C" int emu_clincomb(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *in, const uint32_t *li, uint64_t *out,
                            const uint32_t *lo, const uint32_t *mod_ids, uint32_t n, uint32_t T, const uint64_t *re, const uint64_t *im,
                            const uint64_t *add_re, const uint64_t *add_im, const uint32_t *chunks, uint32_t n_chunks, uint64_t *psi_out) {
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint64_t> qs(n), vs(n);
  for (uint32_t i = 0; i < n; ++i) {
    qs[i] = P.mod[mod_ids[i]];
    vs[i] = hm::powmod(P.psi[mod_ids[i]], P.N / 2, qs[i]);
  }
  for (uint32_t i = 0; psi_out && i < n_mods; ++i) psi_out[i] = P.psi[i];
  std::vector<uint32_t> recs((size_t)n * HM_CLINCOMB_REC_WORDS(T));   // sized exactly: a record word read past the last term ends a sanitizer build
  hm_clincomb_fill_recs(recs.data(), li, lo, mod_ids, vs.data(), qs.data(), n, T, re, im, add_re, add_im);
  HmClincombArgs g;
  g.in = in; g.out = out;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n; g.n_terms = T;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_clincomb_thread(g, entry, chunks[k], tid);
  return 0;
}
