// hm_emu_identity.cpp — the identity forms of the per-thread cores of the weighted sums (hm_ip_core.h: hm_ip_lintrans_multi_thread<TERMS, TILE, true>
// and, for one sum, hm_ip_lintrans_thread<TERMS, true>: the kernels of hm_inner_product_lintrans_id) on the CPU (TEST INFRASTRUCTURE, compiled by tests/test_emu_identity.py with g++, once per arithmetic
// back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The same table the entry point builds (hm_ip_fill_recs + hm_ip_fill_lin + hm_ip_fill_multi +
// hm_ip_fill_id), the same per-modulus constants (hm_params.cpp), every thread of the chosen workgroups and of every tile one after the other;
// and, into a second set of output buffers, what the entry point promises to equal bit for bit: the core without the identity step, then the
// element-wise HM_EWE_MAC_ADD (addend output) and HM_EWE_MUL (second addend output) of hm_elem_core.h.  It is not a CPU backend: the product
// library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_elem_core.h"
#include "../../homulator_amd/csrc/hm_ip_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

extern "C" int emu_identity_generic() { return HM_GENERIC; }

template <int TERMS, int TILE, bool ID, class Args>
static void run_multi(const Args &a, const uint32_t *chunks, uint32_t n_chunks) {
  for (uint32_t tile = 0; tile * TILE < a.n_out; ++tile)
    for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
      for (uint32_t k = 0; k < n_chunks; ++k)
        for (uint32_t tid = 0; tid < 256; ++tid) hm_ip_lintrans_multi_thread<TERMS, TILE, ID>(a, entry, chunks[k], tid, tile);
}
template <int TERMS>
static void run_one(const HmIpLinIdOneArgs &a, const uint32_t *chunks, uint32_t n_chunks) {
  for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_ip_lintrans_thread<TERMS, true>(a, entry, chunks[k], tid);
}
template <bool ID, class Args>
static void run_any(const Args &a, uint32_t T, uint32_t tile, const uint32_t *chunks, uint32_t n_chunks) {
  switch (T * 10 + tile) {
    case 12: run_multi<1, 2, ID>(a, chunks, n_chunks); break;
    case 14: run_multi<1, 4, ID>(a, chunks, n_chunks); break;
    case 22: run_multi<2, 2, ID>(a, chunks, n_chunks); break;
    case 24: run_multi<2, 4, ID>(a, chunks, n_chunks); break;
    case 32: run_multi<3, 2, ID>(a, chunks, n_chunks); break;
    case 34: run_multi<3, 4, ID>(a, chunks, n_chunks); break;
    case 42: run_multi<4, 2, ID>(a, chunks, n_chunks); break;
    case 44: run_multi<4, 4, ID>(a, chunks, n_chunks); break;
  }
}

// moduli[n_mods]: distinct primes = 1 mod 2N below 2^60 (mod id = index).  Limb lists as hm_ip_lintrans_id_desc's (al[i] == HM_NO_LIMB: entry i has
// no addend; a1l[i] then too); chunks[n_chunks]: the 512-coefficient chunks of every entry to run.  out / addend_out / addend1_out: by the identity
// core in tiles of `tile` (2 or 4), or with tile = 1 (one sum only) by the single-sum identity core on its own table; out1 / addend_out1 / addend1_out1: by the core without it, then the element-wise ops.  Returns 0, 1 if the
// moduli are refused, 2 for counts outside the kernel's range.
extern "C" int emu_ip_lintrans_id(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *x, const uint32_t *xl, const uint64_t *y,
                                  const uint32_t *yl, const uint64_t *pt, const uint32_t *pl, const uint32_t *idl, const uint64_t *addend,
                                  const uint32_t *al, const uint64_t *addend1, const uint32_t *a1l, uint64_t *out, uint64_t *out1, const uint32_t *ol,
                                  uint64_t *addend_out, uint64_t *addend_out1, const uint32_t *aol, uint64_t *addend1_out, uint64_t *addend1_out1,
                                  const uint32_t *a1ol, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t R, uint32_t G, uint32_t tile,
                                  const uint32_t *galois, const uint32_t *chunks, uint32_t n_chunks) {
  if (T < 1 || T > HM_IP_MAX_TERMS || R < 1 || R > HM_IP_LINTRANS_ID_MAX_ROT || G < 1 || G > HM_IP_LINTRANS_MULTI_MAX_OUT || (tile != 2 && tile != 4 && !(tile == 1 && G == 1))) return 2;
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, /*forGeneric: the cores read q, mu, r64, r64s, sh only*/ true);
  } catch (const std::exception &) {
    return 1;
  }
  const size_t N = (size_t)1 << logN;
  std::vector<uint64_t> table((hm_ip_id_table_bytes(n, R, G) + 7) / 8);   // 8-byte aligned, as the device allocation is; sized exactly otherwise
  unsigned char *tb = reinterpret_cast<unsigned char *>(table.data());
  HmIpLinRec *recs = reinterpret_cast<HmIpLinRec *>(tb);
  hm_ip_fill_recs(recs, xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, R);
  hm_ip_fill_lin(recs, pl, al, aol, n, R);
  hm_ip_fill_multi(tb, pl, ol, al, aol, n, R, G);
  hm_ip_fill_id(tb, idl, al, a1l, a1ol, n, R, G);
  HmIpLinIdArgs a;
  a.x = x; a.y = y; a.pt = pt; a.addend = addend; a.out = out; a.addend_out = addend_out;
  a.mods = P.modc.data(); a.rec = recs; a.outs = reinterpret_cast<const HmIpMultiOut *>(recs + (size_t)R * n);
  a.pts = reinterpret_cast<const uint16_t *>(a.outs + (size_t)G * n);
  a.ids = reinterpret_cast<const HmIpIdRec *>(a.pts + (size_t)G * R * n);
  a.add1_src = reinterpret_cast<const uint16_t *>(a.ids + (size_t)G * n);
  a.addend1 = addend1; a.addend1_out = addend1_out;
  a.logN = logN; a.n_limbs = n; a.n_rot = R; a.n_out = G;
  for (uint32_t r = 0; r < HM_IP_LINTRANS_MAX_ROT; ++r) a.galois[r] = r < R ? galois[r] : 1u;
  if (tile == 1) {   // one sum: the entry point's other table, HmIpLinRec [R][n] with the identity records behind them
    const size_t recBytes = (size_t)R * n * sizeof(HmIpLinRec);
    std::vector<uint64_t> one((recBytes + hm_ip_id_bytes(n, 1) + 7) / 8);
    unsigned char *ob = reinterpret_cast<unsigned char *>(one.data());
    HmIpLinRec *r1 = reinterpret_cast<HmIpLinRec *>(ob);
    hm_ip_fill_recs(r1, xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, R);
    hm_ip_fill_lin(r1, pl, al, aol, n, R);
    hm_ip_fill_id(ob, idl, al, a1l, a1ol, n, R, 1, recBytes);
    HmIpLinIdOneArgs s;
    s.x = x; s.y = y; s.pt = pt; s.addend = addend; s.out = out; s.addend_out = addend_out; s.addend1 = addend1; s.addend1_out = addend1_out;
    s.mods = P.modc.data(); s.rec = r1; s.ids = reinterpret_cast<const HmIpIdRec *>(r1 + (size_t)R * n);
    s.add1_src = reinterpret_cast<const uint16_t *>(s.ids + n);
    s.logN = logN; s.n_limbs = n; s.n_rot = R;
    for (uint32_t r = 0; r < HM_IP_LINTRANS_MAX_ROT; ++r) s.galois[r] = a.galois[r];
    switch (T) {
      case 1: run_one<1>(s, chunks, n_chunks); break;
      case 2: run_one<2>(s, chunks, n_chunks); break;
      case 3: run_one<3>(s, chunks, n_chunks); break;
      case 4: run_one<4>(s, chunks, n_chunks); break;
    }
    tile = 2;   // (the composition below: any tile serves one sum)
  } else {
    run_any<true>(a, T, tile, chunks, n_chunks);
  }
  // the composition: the same table's first part through the core without the identity step ...
  HmIpLinMultiArgs b = a;
  b.out = out1; b.addend_out = addend_out1;
  run_any<false>(b, T, tile, chunks, n_chunks);
  // ... then, on the entries with an addend, addend_out1 = pt_0 * c0 + addend_out1 (MAC_ADD) and addend1_out1 = pt_0 * c1 (MUL)
  const HmTw none{0, 0};
  for (uint32_t m = 0; m < G; ++m)
    for (uint32_t i = 0; i < n; ++i) {
      if (al[i] == HM_NO_LIMB) continue;
      const HmMod &md = P.modc[mod_ids[i]];
      const uint64_t *p0 = pt + (size_t)idl[m * n + i] * N, *c0 = addend + (size_t)al[i] * N, *c1 = addend1 + (size_t)a1l[i] * N;
      uint64_t *u = addend_out1 + (size_t)aol[m * n + i] * N, *w = addend1_out1 + (size_t)a1ol[m * n + i] * N;
      for (uint32_t k = 0; k < n_chunks; ++k)
        for (size_t e = (size_t)chunks[k] * HM_IP_CHUNK; e < ((size_t)chunks[k] + 1) * HM_IP_CHUNK; ++e) {
          u[e] = hm_ewe_one<HM_EWE_MAC_ADD>(p0[e], c0[e], u[e], 0, none, md);
          w[e] = hm_ewe_one<HM_EWE_MUL>(p0[e], c1[e], 0, 0, none, md);
        }
    }
  return 0;
}

// The sum over ciphertexts with initial sums (hm_ip_rotsum_thread<TERMS, true>, the kernel of hm_inner_product_rotsum_init).  Limb lists as
// hm_ip_rotsum_init_desc's (al[c * n + i] == HM_NO_LIMB: entry i has no addend; ail[i] then too).  out / addend_out: by the core with initial sums
// on the entry point's table (records, then one HmIpSumInit per entry); out1 / addend_out1: by the core without them, then HM_EWE_ADD of the
// initial sums.  Returns 0, 1 if the moduli are refused, 2 for counts outside the kernel's range.
template <int TERMS, bool INIT, class Args>
static void run_sum(const Args &a, const uint32_t *chunks, uint32_t n_chunks) {
  for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (uint32_t tid = 0; tid < 256; ++tid) hm_ip_rotsum_thread<TERMS, INIT>(a, entry, chunks[k], tid);
}
template <bool INIT, class Args>
static void run_sum_any(const Args &a, uint32_t T, const uint32_t *chunks, uint32_t n_chunks) {
  switch (T) {
    case 1: run_sum<1, INIT>(a, chunks, n_chunks); break;
    case 2: run_sum<2, INIT>(a, chunks, n_chunks); break;
    case 3: run_sum<3, INIT>(a, chunks, n_chunks); break;
    case 4: run_sum<4, INIT>(a, chunks, n_chunks); break;
  }
}
extern "C" int emu_ip_rotsum_init(const uint64_t *moduli, uint32_t n_mods, uint32_t logN, const uint64_t *x, const uint32_t *xl, const uint64_t *y,
                                  const uint32_t *yl, const uint64_t *addend, const uint32_t *al, const uint64_t *init, const uint32_t *il,
                                  const uint32_t *ail, uint64_t *out, uint64_t *out1, const uint32_t *ol, uint64_t *addend_out, uint64_t *addend_out1,
                                  const uint32_t *aol, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t G, const uint32_t *galois,
                                  const uint32_t *chunks, uint32_t n_chunks) {
  if (T < 1 || T > HM_IP_MAX_TERMS || G < 1 || G > HM_IP_ROTSUM_INIT_MAX_CT) return 2;
  hm::Params P;
  try {
    P.init(logN, n_mods, 0, moduli, nullptr, nullptr, true);
  } catch (const std::exception &) {
    return 1;
  }
  const size_t N = (size_t)1 << logN, recBytes = (size_t)G * n * sizeof(HmIpSumRec);
  std::vector<uint32_t> table((recBytes + (size_t)n * sizeof(HmIpSumInit) + 3) / 4);   // as the entry point sizes it
  HmIpSumRec *recs = reinterpret_cast<HmIpSumRec *>(table.data());
  hm_ip_fill_recs(recs, xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, G);
  hm_ip_fill_sum(recs, xl, al, aol, n, T, G);
  hm_ip_fill_sum_init(reinterpret_cast<HmIpSumInit *>(recs + (size_t)G * n), il, ail, n);
  HmIpSumInitArgs a;
  a.x = x; a.y = y; a.addend = addend; a.out = out; a.addend_out = addend_out; a.init = init;
  a.mods = P.modc.data(); a.rec = recs; a.inits = reinterpret_cast<const HmIpSumInit *>(recs + (size_t)G * n);
  a.logN = logN; a.n_limbs = n; a.n_ct = G;
  for (uint32_t g = 0; g < HM_IP_ROTSUM_MAX_CT; ++g) a.galois[g] = g < G ? galois[g] : 1u;
  run_sum_any<true>(a, T, chunks, n_chunks);
  HmIpSumArgs b = a;
  b.out = out1; b.addend_out = addend_out1;
  run_sum_any<false>(b, T, chunks, n_chunks);
  const HmTw none{0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const HmMod &md = P.modc[mod_ids[i]];
    for (uint32_t k = 0; k < n_chunks; ++k)
      for (size_t e = (size_t)chunks[k] * HM_IP_CHUNK; e < ((size_t)chunks[k] + 1) * HM_IP_CHUNK; ++e) {
        for (int c = 0; c < 2; ++c) {
          uint64_t *o = out1 + (size_t)ol[i * 2 + c] * N;
          o[e] = hm_ewe_one<HM_EWE_ADD>(o[e], 0, init[(size_t)il[i * 2 + c] * N + e], 0, none, md);
        }
        if (al && al[i] != HM_NO_LIMB) {
          uint64_t *u = addend_out1 + (size_t)aol[i] * N;
          u[e] = hm_ewe_one<HM_EWE_ADD>(u[e], 0, addend[(size_t)ail[i] * N + e], 0, none, md);
        }
      }
  }
  return 0;
}
