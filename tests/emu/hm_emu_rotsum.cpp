// hm_emu_rotsum.cpp — the per-thread core of hm_inner_product_rotsum (hm_ip_core.h: hm_ip_rotsum_thread) on the CPU (TEST INFRASTRUCTURE, compiled
// by tests/test_emu_rotsum.py with g++, once per arithmetic back-end as tests/emu/Makefile defines them: HM_GENERIC = 0 and -DHM_GENERIC=1).
// The same records the entry point builds (hm_ip_fill_recs + hm_ip_fill_sum), the same per-modulus constants (hm_params.cpp), every thread of
// the chosen workgroups one after the other.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_ip_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_rotsum_generic() { return HM_GENERIC; }

// moduli[n_mods]: distinct primes = 1 mod 2N below 2^60 (mod id = index).  Limb lists as hm_ip_rotsum_desc's (al == NULL: no entry has an
// addend); chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are).  Returns 0, 1 if the
// moduli are refused, 2 for counts outside the kernel's range.
extern "C" int emu_ip_rotsum(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *x, const uint32_t *xl, const uint64_t *y,
                             const uint32_t *yl, const uint64_t *addend, const uint32_t *al, uint64_t *out, const uint32_t *ol, uint64_t *addend_out,
                             const uint32_t *aol, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t G, const uint32_t *galois,
                             const uint32_t *chunks, uint32_t n_chunks) {
  if (T < 1 || T > HM_IP_MAX_TERMS || G < 1 || G > HM_IP_ROTSUM_MAX_CT) return 2;
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, /*forGeneric: the core reads q, mu, r64, r64s, sh only*/ true);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<HmIpSumRec> recs((size_t)G * n);
  hm_ip_fill_recs(recs.data(), xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, G);
  hm_ip_fill_sum(recs.data(), xl, al, aol, n, T, G);
  HmIpSumArgs a;
  a.x = x; a.y = y; a.addend = addend; a.out = out; a.addend_out = addend_out;
  a.mods = P.modc.data(); a.rec = recs.data(); a.logN = logN; a.n_limbs = n; a.n_ct = G;
  for (uint32_t g = 0; g < HM_IP_ROTSUM_MAX_CT; ++g) a.galois[g] = g < G ? galois[g] : 1u;
  for (uint32_t entry = 0; entry < n; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) switch (T) {
        case 1: hm_ip_rotsum_thread<1>(a, entry, chunks[k], tid); break;
        case 2: hm_ip_rotsum_thread<2>(a, entry, chunks[k], tid); break;
        case 3: hm_ip_rotsum_thread<3>(a, entry, chunks[k], tid); break;
        case 4: hm_ip_rotsum_thread<4>(a, entry, chunks[k], tid); break;
      }
  return 0;
}
