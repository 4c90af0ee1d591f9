// hm_emu_square.cpp — the per-thread core of hm_tensor_square (hm_rec_core.h: hm_tensor_square_one, hm_tensor_square_thread) on the CPU (TEST
// INFRASTRUCTURE, compiled by tests/test_emu_square.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same
// records the entry point builds (hm_tensor_square_fill_recs), the same per-modulus constants (hm_params.cpp), every thread of the chosen
// workgroups one after the other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_rec_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_square_generic() { return HM_GENERIC; }

static bool params(hm::Params &P, const uint64_t *moduli, uint32_t n_mods, uint32_t logN) {
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    return false;
  }
  return true;
}

// moduli[n_mods]: distinct primes = 1 mod 2N this build's arithmetic accepts (mod id = index).  Limb lists and constants as hm_tensor_square's;
// chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are).  Returns 0, or 1 if the moduli
// are refused.
extern "C" int emu_tensor_square(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *a, const uint32_t *la, const uint64_t *c,
                                 const uint32_t *lc, uint64_t *o0, const uint32_t *l0, uint64_t *o1, const uint32_t *l1, uint64_t *o2, const uint32_t *l2,
                                 const uint32_t *mod_ids, uint32_t n, const uint64_t *scale, const uint64_t *addend, const uint32_t *chunks,
                                 uint32_t n_chunks) {
  hm::Params P;
  if (!params(P, moduli, n_mods, logN)) return 1;
  std::vector<HmTensorSqRec> recs(n);
  std::vector<uint64_t> q(n);
  for (uint32_t i = 0; i < n; ++i) q[i] = P.mod[mod_ids[i]];
  hm_tensor_square_fill_recs(recs.data(), la, lc, l0, l1, l2, mod_ids, q.data(), n, scale, addend);
  HmTensorSqArgs g;
  g.a = a; g.c = c; g.o0 = o0; g.o1 = o1; g.o2 = o2;
  g.mods = P.modc.data(); g.rec = recs.data(); g.logN = logN; g.n_limbs = n;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_tensor_square_thread(g, entry, chunks[k], tid);
  return 0;
}

// the arithmetic on single words: out[3 i .. 3 i + 2] = (d0, d1, d2) of (a[i], c[i]) under modulus id `mod` with the scalar s and the constant k
extern "C" int emu_square_words(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, uint32_t mod, uint64_t s, uint64_t k, const uint64_t *a,
                                const uint64_t *c, uint32_t n, uint64_t *out) {
  hm::Params P;
  if (!params(P, moduli, n_mods, logN)) return 1;
  const uint64_t q = P.mod[mod];
  HmTensorSqRec r;
  hm_tensor_square_fill_recs(&r, nullptr, nullptr, nullptr, nullptr, nullptr, &mod, &q, 1, &s, &k);
  for (uint32_t i = 0; i < n; ++i) hm_tensor_square_one(a[i], c[i], r.scale, r.scale_s, r.scaled, r.addend, P.modc[mod], out[3 * i], out[3 * i + 1], out[3 * i + 2]);
  return 0;
}

// the new element-wise opcode on single words: out[i] = a[i] + k mod q (hm_ewe_one<HM_EWE_ADD_CONST>, the constant where the launch puts it)
extern "C" int emu_add_const_words(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, uint32_t mod, uint64_t k, const uint64_t *a, uint32_t n,
                                   uint64_t *out) {
  hm::Params P;
  if (!params(P, moduli, n_mods, logN)) return 1;
  const HmTw kk = {k, hm::shoup(k, P.mod[mod])};
  for (uint32_t i = 0; i < n; ++i) out[i] = hm_ewe_one<HM_EWE_ADD_CONST>(a[i], 0, 0, 0, kk, P.modc[mod]);
  return 0;
}
