// hm_emu_dot.cpp — the per-thread core of hm_tensor_dot (hm_rec_core.h: hm_tensor_dot_thread) on the CPU (TEST INFRASTRUCTURE, compiled by
// tests/test_emu_dot.py with g++, once per arithmetic back-end as tests/emu/Makefile defines them: HM_GENERIC = 0 and -DHM_GENERIC=1).
// The same records the entry point builds (hm_tensor_dot_fill_recs), the same per-modulus constants (hm_params.cpp), every thread of the chosen
// workgroups one after the other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_dot_generic() { return HM_GENERIC; }

// moduli[n_mods]: distinct primes = 1 mod 2N below 2^60 (mod id = index).  Limb lists as hm_tensor_dot's; chunks[n_chunks]: the 512-coefficient
// chunks of every entry to run (the outputs elsewhere are left as they are).  Returns 0, or 1 if the moduli are refused.
extern "C" int emu_tensor_dot(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *a, const uint32_t *la, const uint64_t *b,
                              const uint32_t *lb, const uint64_t *c, const uint32_t *lc, const uint64_t *d, const uint32_t *ld, uint64_t *o0,
                              const uint32_t *l0, uint64_t *o1, const uint32_t *l1, uint64_t *o2, const uint32_t *l2, const uint32_t *mod_ids,
                              uint32_t n, uint32_t n_terms, const uint32_t *chunks, uint32_t n_chunks) {
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, /*forGeneric: the core reads q, mu, r64, r64s, sh only*/ true);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint32_t> recs((size_t)n * HM_DOT_REC_WORDS(n_terms));
  hm_tensor_dot_fill_recs(recs.data(), la, lb, lc, ld, l0, l1, l2, mod_ids, n, n_terms);
  HmTensorDotArgs g;
  g.a = a; g.b = b; g.c = c; g.d = d; g.o0 = o0; g.o1 = o1; g.o2 = o2;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n; g.n_terms = n_terms;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_tensor_dot_thread(g, entry, chunks[k], tid);
  return 0;
}
