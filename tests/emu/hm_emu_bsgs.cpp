// hm_emu_bsgs.cpp — the per-thread core of hm_inner_product_lintrans_multi (hm_ip_core.h: hm_ip_lintrans_multi_thread) on the CPU (TEST
// INFRASTRUCTURE, compiled by tests/test_emu_bsgs.py with g++, once per arithmetic back-end as tests/emu/Makefile defines them: HM_GENERIC = 0 and
// -DHM_GENERIC=1).  The same table the entry point builds (hm_ip_fill_recs + hm_ip_fill_lin + hm_ip_fill_multi), the same per-modulus constants
// (hm_params.cpp), every thread of the chosen workgroups and of every tile one after the other; and, into a second pair of output buffers, the
// single-sum core hm_ip_lintrans_thread once per output.  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_ip_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_bsgs_generic() { return HM_GENERIC; }
extern "C" int emu_bsgs_default_tile() { return HM_IP_LINTRANS_MULTI_TILE; }

template <int TERMS, int TILE>
static void run_multi(const HmIpLinMultiArgs &a, const uint32_t *chunks, uint32_t n_chunks) {
  for (uint32_t tile = 0; tile * TILE < a.n_out; ++tile)
    for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
      for (uint32_t k = 0; k < n_chunks; ++k)
        for (uint32_t tid = 0; tid < 256; ++tid) hm_ip_lintrans_multi_thread<TERMS, TILE>(a, entry, chunks[k], tid, tile);
}
template <int TERMS>
static void run_single(const HmIpLinArgs &a, const uint32_t *chunks, uint32_t n_chunks) {
  for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_ip_lintrans_thread<TERMS>(a, entry, chunks[k], tid);
}

// moduli[n_mods]: distinct primes = 1 mod 2N below 2^60 (mod id = index).  Limb lists as hm_ip_lintrans_multi_desc's (al == NULL: no entry has an
// addend); chunks[n_chunks]: the 512-coefficient chunks of every entry to run (the outputs elsewhere are left as they are).  out / addend_out: by
// the multi core in tiles of `tile` (2 or 4); out1 / addend_out1: by G runs of the single-sum core.  Returns 0, 1 if the moduli are refused, 2 for
// counts outside the kernel's range.
extern "C" int emu_ip_lintrans_multi(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *x, const uint32_t *xl, const uint64_t *y,
                                     const uint32_t *yl, const uint64_t *pt, const uint32_t *pl, const uint64_t *addend, const uint32_t *al,
                                     uint64_t *out, uint64_t *out1, const uint32_t *ol, uint64_t *addend_out, uint64_t *addend_out1,
                                     const uint32_t *aol, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t R, uint32_t G, uint32_t tile,
                                     const uint32_t *galois, const uint32_t *chunks, uint32_t n_chunks) {
  if (T < 1 || T > HM_IP_MAX_TERMS || R < 1 || R > HM_IP_LINTRANS_MAX_ROT || G < 1 || G > HM_IP_LINTRANS_MULTI_MAX_OUT || (tile != 2 && tile != 4)) return 2;
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, /*forGeneric: the core reads q, mu, r64, r64s, sh only*/ true);
  } catch (const std::exception &) {
    return 1;
  }
  std::vector<uint64_t> table((hm_ip_multi_table_bytes(n, R, G) + 7) / 8);   // 8-byte aligned, as the device allocation is
  unsigned char *tb = reinterpret_cast<unsigned char *>(table.data());
  HmIpLinRec *recs = reinterpret_cast<HmIpLinRec *>(tb);
  hm_ip_fill_recs(recs, xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, R);
  hm_ip_fill_lin(recs, pl, al, aol, n, R);
  hm_ip_fill_multi(tb, pl, ol, al, aol, n, R, G);
  HmIpLinMultiArgs a;
  a.x = x; a.y = y; a.pt = pt; a.addend = addend; a.out = out; a.addend_out = addend_out;
  a.mods = P.modc.data(); a.rec = recs; a.outs = reinterpret_cast<const HmIpMultiOut *>(recs + (size_t)R * n);
  a.pts = reinterpret_cast<const uint16_t *>(a.outs + (size_t)G * n);
  a.logN = logN; a.n_limbs = n; a.n_rot = R; a.n_out = G;
  for (uint32_t r = 0; r < HM_IP_LINTRANS_MAX_ROT; ++r) a.galois[r] = r < R ? galois[r] : 1u;
  switch (T * 10 + tile) {
    case 12: run_multi<1, 2>(a, chunks, n_chunks); break;
    case 14: run_multi<1, 4>(a, chunks, n_chunks); break;
    case 22: run_multi<2, 2>(a, chunks, n_chunks); break;
    case 24: run_multi<2, 4>(a, chunks, n_chunks); break;
    case 32: run_multi<3, 2>(a, chunks, n_chunks); break;
    case 34: run_multi<3, 4>(a, chunks, n_chunks); break;
    case 42: run_multi<4, 2>(a, chunks, n_chunks); break;
    case 44: run_multi<4, 4>(a, chunks, n_chunks); break;
  }
  for (uint32_t m = 0; m < G; ++m) {   // the single-sum form, as the entry point of hm_inner_product_lintrans builds it, once per output
    std::vector<HmIpLinRec> one((size_t)R * n);
    hm_ip_fill_recs(one.data(), xl, yl, ol + (size_t)m * n * 2, (size_t)n * 2, mod_ids, n, T, 2, R);
    hm_ip_fill_lin(one.data(), pl + (size_t)m * R * n, al, al ? aol + (size_t)m * n : nullptr, n, R);
    HmIpLinArgs s;
    s.x = x; s.y = y; s.pt = pt; s.addend = addend; s.out = out1; s.addend_out = addend_out1;
    s.mods = P.modc.data(); s.rec = one.data(); s.logN = logN; s.n_limbs = n; s.n_rot = R;
    for (uint32_t r = 0; r < HM_IP_LINTRANS_MAX_ROT; ++r) s.galois[r] = a.galois[r];
    switch (T) {
      case 1: run_single<1>(s, chunks, n_chunks); break;
      case 2: run_single<2>(s, chunks, n_chunks); break;
      case 3: run_single<3>(s, chunks, n_chunks); break;
      case 4: run_single<4>(s, chunks, n_chunks); break;
    }
  }
  return 0;
}
