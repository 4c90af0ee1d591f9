// hm_emu_dotadd.cpp — the per-thread core of hm_tensor_dotadd (hm_rec_core.h: hm_tensor_dotadd_thread and its helpers) on the CPU (TEST
// INFRASTRUCTURE, compiled by tests/test_emu_dotadd.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same records
// the entry point builds (hm_tensor_dotadd_fill_recs), the same per-modulus constants (hm_params.cpp), every thread of the chosen workgroups one
// after the other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_dotadd_generic() { return HM_GENERIC; }
extern "C" uint32_t emu_dotadd_rec_words(uint32_t T, uint32_t A) { return HM_DOTADD_REC_WORDS(T, A); }
extern "C" uint32_t emu_dotadd_max_terms() { return HM_DOTADD_MAX_TERMS; }
extern "C" uint32_t emu_dotadd_max_addends() { return HM_DOTADD_MAX_ADDENDS; }

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  One buffer `in` holds the operands of the pairs
// (limb lists la .. ld, [n][T]) and the addends (lx0, lx1: [n][A]); limb lists and constants as hm_tensor_dotadd's (scale / addend null: 1 / 0);
// chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are).  Returns 0, or 1 if the
// moduli are refused.
extern "C" int emu_dotadd(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *in, const uint32_t *la, const uint32_t *lb,
                          const uint32_t *lc, const uint32_t *ld, const uint32_t *lx0, const uint32_t *lx1, uint64_t *out, const uint32_t *l0,
                          const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t A, const uint64_t *scale,
                          const uint64_t *add_scale, const uint64_t *addend, const uint32_t *chunks, uint32_t n_chunks) {
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint32_t> recs((size_t)n * HM_DOTADD_REC_WORDS(T, A));   // sized exactly: a record word read past the last addend ends a sanitizer build
  std::vector<uint64_t> qs(n);
  for (uint32_t i = 0; i < n; ++i) qs[i] = moduli[mod_ids[i]];
  hm_tensor_dotadd_fill_recs(recs.data(), la, lb, lc, ld, lx0, lx1, l0, l1, l2, mod_ids, qs.data(), n, T, A, scale, add_scale, addend);
  HmTensorDotAddArgs g;
  g.a = g.b = g.c = g.d = g.x = in;
  g.o0 = g.o1 = g.o2 = out;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n; g.n_terms = T; g.n_addends = A;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_tensor_dotadd_thread(g, entry, chunks[k], tid);
  return 0;
}
