// hm_emu_slots.cpp — the slot transform (homulator_amd/csrc/hm_slot_core.h: the per-thread code of k_slot_fft, hm_encode / hm_decode) on the CPU
// (TEST INFRASTRUCTURE, compiled by tests/test_emu_slots.py with g++ -ffp-contract=off).  The passes run phase by phase, thread by thread, tile by
// tile, exactly as the workgroups of the two launches do.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <map>
#include <vector>
#include "../../homulator_amd/csrc/hm_slot_core.h"

namespace {
struct Tables {
  std::vector<HmC> roots;
  std::vector<uint32_t> rot;
};
const Tables &tables(uint32_t logN) {
  static std::map<uint32_t, Tables> made;
  auto it = made.find(logN);
  if (it == made.end()) {
    it = made.emplace(logN, Tables()).first;
    hm_slot_tables(logN, it->second.roots, it->second.rot);
  }
  return it->second;
}
// one launch of k_slot_fft<INVERSE>: every workgroup, phase by phase (a barrier on the GPU = the end of a thread loop here)
template <bool INVERSE, bool HIGH>
void run_pass(const HmSlotArgs &a, uint32_t n_vec) {
  std::vector<HmC> lds(HM_SLOT_LDS);
  const bool coefSide = !HIGH;   // LOW: the inverse direction stores coefficients, the forward direction loads them
  for (uint32_t v = 0; v < n_vec; ++v)
    for (uint32_t tile = 0; tile < a.tiles; ++tile) {
      for (uint32_t t = 0; t < HM_SLOT_THREADS; ++t) {
        if (coefSide && !INVERSE) hm_slot_load_coef(a, v, tile, t, lds.data());
        else hm_slot_load<HIGH>(a, v, tile, t, lds.data());
      }
      for (uint32_t s = 0; s < (HIGH ? a.log1 : a.log2); ++s)
        for (uint32_t t = 0; t < HM_SLOT_THREADS; ++t) hm_slot_stage<INVERSE, HIGH>(a, tile, t, lds.data(), s);
      for (uint32_t t = 0; t < HM_SLOT_THREADS; ++t) {
        if (coefSide && INVERSE) hm_slot_store_coef(a, v, tile, t, lds.data());
        else hm_slot_store<HIGH>(a, v, tile, t, lds.data());
      }
    }
}
bool base_args(uint32_t logN, uint64_t q, HmSlotArgs &a) {
  if (logN < HM_SLOT_MIN_LOGN + 1 || logN > HM_SLOT_MAX_LOGN + 1 || q < 3) return false;
  const Tables &t = tables(logN);
  a = HmSlotArgs{};
  a.roots = t.roots.data(); a.rot = t.rot.data();
  a.logn = logN - 1; a.log1 = hm_slot_log1(a.logn); a.log2 = hm_slot_log2(a.logn); a.tiles = (1u << a.logn) >> HM_SLOT_TL;
  a.q = q; a.half = (q - 1) / 2;
  return true;
}
}   // namespace

extern "C" {
// coef[v][N] = the coefficient-form limb-poly of slots z[v][n] (re, im) at scale `scale` modulo q; *overflow = the device flag.  1: bad arguments
int emu_slots_encode(uint32_t logN, const double *z, uint32_t n_vec, double scale, uint64_t q, uint64_t *coef, uint32_t *overflow) {
  HmSlotArgs a;
  if (!base_args(logN, q, a)) return 1;
  const size_t n = (size_t)1 << a.logn;
  std::vector<HmC> tmp(n * n_vec);
  std::vector<uint32_t> limbs(n_vec);
  for (uint32_t v = 0; v < n_vec; ++v) limbs[v] = v;
  uint32_t flag = 0;
  a.limbs = limbs.data(); a.flag = &flag; a.coef = coef;
  a.mul = scale * (2.0 / (double)(2 * n));
  a.zin = reinterpret_cast<const HmC *>(z); a.zout = tmp.data();
  run_pass<true, true>(a, n_vec);
  a.zin = tmp.data(); a.zout = nullptr;
  run_pass<true, false>(a, n_vec);
  *overflow = flag;
  return 0;
}
// z[v][n] = the slots of the coefficient-form limb-poly coef[v][N] modulo q at scale `scale`
int emu_slots_decode(uint32_t logN, const uint64_t *coef, uint32_t n_vec, double scale, uint64_t q, double *z) {
  HmSlotArgs a;
  if (!base_args(logN, q, a)) return 1;
  std::vector<uint32_t> limbs(n_vec);
  for (uint32_t v = 0; v < n_vec; ++v) limbs[v] = v;
  a.limbs = limbs.data(); a.coef = const_cast<uint64_t *>(coef);
  a.mul = 1.0 / scale;
  a.zout = reinterpret_cast<HmC *>(z);
  run_pass<false, false>(a, n_vec);
  a.zin = a.zout;
  run_pass<false, true>(a, n_vec);
  return 0;
}
}
