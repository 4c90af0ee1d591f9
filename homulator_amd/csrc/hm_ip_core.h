// hm_ip_core.h — K5, the inner product with the evaluation key, in its five forms: plain (hm_inner_product_ex), hoisted
// (hm_inner_product_hoisted), the weighted sum of rotations (hm_inner_product_lintrans), the sum of rotations of different ciphertexts
// (hm_inner_product_rotsum) and several weighted sums of the same rotations (hm_inner_product_lintrans_multi).
// The weighted sums also come with an identity step (hm_inner_product_lintrans_id), the sum over ciphertexts with initial sums
// (hm_inner_product_rotsum_init): template flags of the same cores, off for the forms above.
// Per-thread bodies (no cross-thread state) and the records they read, shared by the HIP kernels, the entry points and the host emulator.
// A workgroup of 256 threads covers 512 coefficients of one entry: thread tid of chunk c owns the aligned pair at c * 512 + 2 * tid.
//
// Reference shape: the HPIP unit (InsGen::GenHPIP src/InsGen.cpp:356-406, HPIP src/Components.cpp:571-595; in the shipped configs it runs on
// the EWE as beta-1 MAC groups per key, KeySwitch::InnerProduceOperation src/Operation.cpp:294-414).  One pass: acc_k = sum_j x_j * y_{j,k}.
#pragma once
#include "../../include/homulator_hip.h"   // HM_IP_HOISTED_MAX_ROT, HM_IP_LINTRANS_MAX_ROT, HM_IP_ROTSUM_MAX_CT
#include "hm_modarith.h"
#include "hm_ntt_core.h"

#define HM_IP_MAX_TERMS 4
#define HM_IP_MAX_OUT 2
#define HM_IP_MAX_LIMBS 64
#define HM_IP_CHUNK 512   // coefficients per workgroup

// ---- records: the limbs of one entry's digits, keys and outputs, then what the form adds.  HmIpKeys is the prefix of all three.
struct HmIpKeys {
  uint16_t x[HM_IP_MAX_TERMS];
  uint16_t y[HM_IP_MAX_OUT][HM_IP_MAX_TERMS];
  uint16_t out[HM_IP_MAX_OUT];
};
struct HmIpLimb : HmIpKeys {
  uint16_t mod, pad;
};
typedef HmIpLimb HmIpHoistRec;   // one per (rotation, entry), in a device table (16 rotations of 64 entries do not fit the kernel arguments)
struct HmIpLinRec : HmIpKeys {   // one per (rotation, entry); the digits, the addend, the outputs and the modulus are read from rotation 0's
  uint16_t pt, add_src, add_out;
  uint16_t mod, has_add, pad;
};
struct HmIpSumRec : HmIpKeys {   // one per (ciphertext, entry): its own digits, keys and addend source; the outputs and the modulus are ciphertext 0's
  uint16_t mod, add_src, add_out, has_add;
};
struct HmIpMultiOut {   // several weighted sums: one per (output, entry), behind the HmIpLinRec records [n_rot][n] the outputs share (whose pt, out and add_out are output 0's)
  uint16_t out[2], add_out, pad;
};
struct HmIpIdRec {   // the identity step of several weighted sums: one per (output, entry), behind the table of HmIpMultiOut and plaintext limbs
  uint16_t pt, add1_out;   // the identity plaintext's limb (in pt) and the limb of W = pt_0 * c1 (in addend1_out); read on entries with an addend only
};
static_assert(sizeof(HmIpKeys) == 28 && sizeof(HmIpHoistRec) == 32 && sizeof(HmIpLinRec) == 40 && sizeof(HmIpSumRec) == 36 && sizeof(HmIpMultiOut) == 8 &&
                  sizeof(HmIpIdRec) == 4,
              "the device tables' record sizes");

struct HmIpArgs {
  const uint64_t *x, *y;
  uint64_t *out;
  const HmMod *mods;
  uint32_t logN, n_limbs, n_terms, n_out;
  uint32_t x_galois;   // > 1: the x operands are read through the automorphism X -> X^x_galois (round 6, hm_inner_product_ex)
  HmIpLimb limb[HM_IP_MAX_LIMBS];
};
struct HmIpHoistArgs {
  const uint64_t *x, *y;
  uint64_t *out;
  const HmMod *mods;
  const HmIpHoistRec *rec;   // [n_rot][n_limbs]
  uint32_t logN, n_limbs, n_rot;
  uint32_t dst_galois[HM_IP_HOISTED_MAX_ROT];   // g_r^-1 mod 2N: coefficient i of a digit lands at hm_auto_src(i, g_r^-1) of rotation r
};
struct HmIpLinArgs {
  const uint64_t *x, *y, *pt, *addend;
  uint64_t *out, *addend_out;
  const HmMod *mods;
  const HmIpLinRec *rec;   // [n_rot][n_limbs]
  uint32_t logN, n_limbs, n_rot;
  uint32_t galois[HM_IP_LINTRANS_MAX_ROT];
};
struct HmIpLinMultiArgs {
  const uint64_t *x, *y, *pt, *addend;
  uint64_t *out, *addend_out;
  const HmMod *mods;
  const HmIpLinRec *rec;      // [n_rot][n_limbs]: digits, keys, modulus, addend source
  const HmIpMultiOut *outs;   // [n_out][n_limbs]
  const uint16_t *pts;        // [n_out][n_rot][n_limbs]
  uint32_t logN, n_limbs, n_rot, n_out;
  uint32_t galois[HM_IP_LINTRANS_MAX_ROT];
};
struct HmIpIdStep {   // what the identity step (hm_inner_product_lintrans_id) adds to the arguments of a weighted sum: the unrotated term
  const uint64_t *addend1;      // the second addend source (c1), read unrotated as `addend` (c0) is
  uint64_t *addend1_out;
  const HmIpIdRec *ids;         // [n_out][n_limbs] (one sum: [n_limbs]), behind the records in their table
  const uint16_t *add1_src;     // [n_limbs]
};
struct HmIpLinIdOneArgs : HmIpLinArgs, HmIpIdStep {};     // ONE sum (n_out = 1): the single-sum kernel form
struct HmIpLinIdArgs : HmIpLinMultiArgs, HmIpIdStep {};   // several sums
struct HmIpSumInit {   // the sum over ciphertexts with initial sums (hm_inner_product_rotsum_init): one per entry, behind the HmIpSumRec records
  uint16_t init[2], add_init, pad;   // limbs of the initial S_0, S_1 (in `init`) and of the initial addend sum (in `addend`; read with has_add)
};
struct HmIpSumArgs {
  const uint64_t *x, *y, *addend;
  uint64_t *out, *addend_out;
  const HmMod *mods;
  const HmIpSumRec *rec;   // [n_ct][n_limbs]
  uint32_t logN, n_limbs, n_ct;
  uint32_t galois[HM_IP_ROTSUM_MAX_CT];
};
struct HmIpSumInitArgs : HmIpSumArgs {
  const uint64_t *init;
  const HmIpSumInit *inits;     // [n_limbs]
};

// The records of n entries x n_rot rotations, rec[r * n + i], from the entry points' limb lists: digits x [n][T], keys y [n_rot][n][K][T],
// outputs out [n_outs / K][K] — every rotation its own (n_outs = n_rot * n * K) or all of them rotation 0's (n_outs = n * K).  Host side.
template <class Rec>
inline void hm_ip_fill_recs(Rec *rec, const uint32_t *x, const uint32_t *y, const uint32_t *out, size_t n_outs, const uint32_t *mod_ids, uint32_t n,
                            uint32_t T, uint32_t K, uint32_t n_rot) {
  for (size_t e = 0; e < (size_t)n_rot * n; ++e) {
    const size_t i = e % n;
    Rec l{};
    l.mod = (uint16_t)mod_ids[i];
    for (uint32_t j = 0; j < T; ++j) l.x[j] = (uint16_t)x[i * T + j];
    for (uint32_t k = 0; k < K; ++k) {
      l.out[k] = (uint16_t)out[(e * K + k) % n_outs];
      for (uint32_t j = 0; j < T; ++j) l.y[k][j] = (uint16_t)y[(e * K + k) * T + j];
    }
    rec[e] = l;
  }
}
// ... and what the weighted sum adds: plaintexts pt [n_rot][n]; addend sources / outputs [n], or nullptr (none), HM_NO_LIMB: not this entry
inline void hm_ip_fill_lin(HmIpLinRec *rec, const uint32_t *pt, const uint32_t *addend, const uint32_t *addend_out, uint32_t n, uint32_t n_rot) {
  for (size_t e = 0; e < (size_t)n_rot * n; ++e) {
    const size_t i = e % n;
    rec[e].pt = (uint16_t)pt[e];
    if (addend && addend[i] != HM_NO_LIMB) { rec[e].has_add = 1; rec[e].add_src = (uint16_t)addend[i]; rec[e].add_out = (uint16_t)addend_out[i]; }
  }
}
// ... and what several weighted sums add behind those records, in ONE table (one content-cached allocation): the outputs' limbs out [n_out][n][2]
// and addend_out [n_out][n] as HmIpMultiOut [n_out][n], then the plaintext limbs pt [n_out][n_rot][n] as 16-bit words.  `recs`: the table's first
// n_rot * n * sizeof(HmIpLinRec) bytes, filled by hm_ip_fill_recs + hm_ip_fill_lin with output 0's lists
inline size_t hm_ip_multi_table_bytes(uint32_t n, uint32_t n_rot, uint32_t n_out) {
  return (size_t)n_rot * n * sizeof(HmIpLinRec) + (size_t)n_out * n * sizeof(HmIpMultiOut) + (size_t)n_out * n_rot * n * sizeof(uint16_t);
}
inline void hm_ip_fill_multi(unsigned char *table, const uint32_t *pt, const uint32_t *out, const uint32_t *addend, const uint32_t *addend_out, uint32_t n,
                             uint32_t n_rot, uint32_t n_out) {
  HmIpMultiOut *o = reinterpret_cast<HmIpMultiOut *>(table + (size_t)n_rot * n * sizeof(HmIpLinRec));
  uint16_t *p = reinterpret_cast<uint16_t *>(o + (size_t)n_out * n);
  for (size_t e = 0; e < (size_t)n_out * n; ++e) {
    const bool add = addend && addend[e % n] != HM_NO_LIMB;
    o[e] = HmIpMultiOut{{(uint16_t)out[e * 2], (uint16_t)out[e * 2 + 1]}, (uint16_t)(add ? addend_out[e] : 0), 0};
  }
  for (size_t e = 0; e < (size_t)n_out * n_rot * n; ++e) p[e] = (uint16_t)pt[e];
}
// ... and what the identity step adds behind that table (the same allocation): HmIpIdRec [n_out][n] from id_pt [n_out][n] and addend1_out [n_out][n],
// then the second addend's source limbs addend1 [n] as 16-bit words.  Entries without an addend (addend[i] == HM_NO_LIMB) get zeros, never read
inline size_t hm_ip_id_table_bytes(uint32_t n, uint32_t n_rot, uint32_t n_out) {
  return hm_ip_multi_table_bytes(n, n_rot, n_out) + (size_t)n_out * n * sizeof(HmIpIdRec) + (size_t)n * sizeof(uint16_t);
}
// (one sum: the same records behind the HmIpLinRec [n_rot][n] of hm_inner_product_lintrans: `at` = the table's size without them)
inline size_t hm_ip_id_bytes(uint32_t n, uint32_t n_out) { return (size_t)n_out * n * sizeof(HmIpIdRec) + (size_t)n * sizeof(uint16_t); }
inline void hm_ip_fill_id(unsigned char *table, const uint32_t *id_pt, const uint32_t *addend, const uint32_t *addend1, const uint32_t *addend1_out, uint32_t n,
                          uint32_t n_rot, uint32_t n_out, size_t at = 0) {
  HmIpIdRec *d = reinterpret_cast<HmIpIdRec *>(table + (at ? at : hm_ip_multi_table_bytes(n, n_rot, n_out)));
  uint16_t *s = reinterpret_cast<uint16_t *>(d + (size_t)n_out * n);
  for (size_t e = 0; e < (size_t)n_out * n; ++e) {
    const bool add = addend[e % n] != HM_NO_LIMB;
    d[e] = HmIpIdRec{(uint16_t)(add ? id_pt[e] : 0), (uint16_t)(add ? addend1_out[e] : 0)};
  }
  for (uint32_t i = 0; i < n; ++i) s[i] = (uint16_t)(addend[i] != HM_NO_LIMB ? addend1[i] : 0);
}
// ... and what the sum over ciphertexts changes: every ciphertext has its own digits x [n_ct][n][T] and addend source [n_ct][n] (or nullptr)
inline void hm_ip_fill_sum(HmIpSumRec *rec, const uint32_t *x, const uint32_t *addend, const uint32_t *addend_out, uint32_t n, uint32_t T, uint32_t n_ct) {
  for (size_t e = 0; e < (size_t)n_ct * n; ++e) {
    const size_t i = e % n;
    for (uint32_t j = 0; j < T; ++j) rec[e].x[j] = (uint16_t)x[e * T + j];
    if (addend && addend[e] != HM_NO_LIMB) { rec[e].has_add = 1; rec[e].add_src = (uint16_t)addend[e]; rec[e].add_out = (uint16_t)addend_out[i]; }
  }
}

static_assert(sizeof(HmIpSumInit) == 8, "the device tables' record sizes");
// ... and the initial sums behind the sum over ciphertexts' records: init [n][2], addend_init [n] (HM_NO_LIMB: none)
inline void hm_ip_fill_sum_init(HmIpSumInit *t, const uint32_t *init, const uint32_t *addend_init, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    t[i] = HmIpSumInit{{(uint16_t)init[i * 2], (uint16_t)init[i * 2 + 1]}, (uint16_t)(addend_init && addend_init[i] != HM_NO_LIMB ? addend_init[i] : 0), 0};
}

// ---- per-thread pieces
struct HmIpPair { uint64_t x, y; };   // an aligned pair of coefficients: one 16-byte access
HM_HD HmIpPair hm_ip_ld(const uint64_t *base, uint32_t limb, uint32_t N, uint32_t off) {
  HmIpPair v;
  hm_ld2(base + (size_t)limb * N + off, v.x, v.y);
  return v;
}
HM_HD void hm_ip_st(uint64_t *base, uint32_t limb, uint32_t N, uint32_t off, const HmIpPair &v) { hm_st2(base + (size_t)limb * N + off, v.x, v.y); }

// sum_j x_j * y_j mod q for both words of a pair, the digit words taken in the other order when `swap` (hm_auto_pair): the ONE place the three
// forms multiply and reduce.  TERMS <= 4 products below 2^120: within hm_barrett's 2^(k+63)
template <int TERMS>
HM_HD HmIpPair hm_ip_dot(const HmIpPair *vx, const HmIpPair *vy, bool swap, const HmMod &m) {
  hm_u128 s0 = 0, s1 = 0;
#pragma unroll
  for (int j = 0; j < TERMS; ++j) {
    const uint64_t x0 = swap ? vx[j].y : vx[j].x, x1 = swap ? vx[j].x : vx[j].y;
    s0 += (hm_u128)x0 * vy[j].x;
    s1 += (hm_u128)x1 * vy[j].y;
  }
  return HmIpPair{hm_barrett(s0, m), hm_barrett(s1, m)};
}

// plain: out_k = sum_j x_j y_kj at the thread's pair; x through an automorphism when x_galois > 1 (wave-uniform choice)
template <int TERMS, int OUTS>
HM_HD void hm_ip_thread(const HmIpArgs &a, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const uint32_t N = 1u << a.logN;
  const HmIpLimb &lb = a.limb[entry];
  const HmMod m = a.mods[lb.mod];
  const uint32_t off = chunk * HM_IP_CHUNK + 2 * tid;
  uint32_t offx = off;
  bool swap = false;
  if (a.x_galois > 1) offx = hm_auto_pair(off, a.x_galois, a.logN, swap);
  HmIpPair vx[TERMS], vy[OUTS][TERMS];
#pragma unroll
  for (int j = 0; j < TERMS; ++j) {
    vx[j] = hm_ip_ld(a.x, lb.x[j], N, offx);
#pragma unroll
    for (int k = 0; k < OUTS; ++k) vy[k][j] = hm_ip_ld(a.y, lb.y[k][j], N, off);
  }
#pragma unroll
  for (int k = 0; k < OUTS; ++k) {
    const HmIpPair o = hm_ip_dot<TERMS>(vx, vy[k], swap, m);
    hm_ip_st(a.out, lb.out[k], N, off, o);
  }
}

// hoisted, the SCATTER form: the key products of n_rot rotations of ONE ciphertext from its unrotated digits.  sigma_g takes the aligned pair
// (off, off + 1) of a digit to the aligned pair at hm_auto_src(off, g^-1 mod 2N), in order or swapped: a thread loads its pair of every digit
// ONCE and, rotation by rotation, gathers the two keys and stores the two sums at that destination.
template <int TERMS>
HM_HD void hm_ip_hoisted_thread(const HmIpHoistArgs &a, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const uint32_t N = 1u << a.logN;
  const HmIpHoistRec &l0 = a.rec[entry];
  const HmMod m = a.mods[l0.mod];
  const uint32_t off = chunk * HM_IP_CHUNK + 2 * tid;
  HmIpPair vx[TERMS];
#pragma unroll
  for (int j = 0; j < TERMS; ++j) vx[j] = hm_ip_ld(a.x, l0.x[j], N, off);
#pragma unroll 1
  for (uint32_t r = 0; r < a.n_rot; ++r) {
    const HmIpHoistRec &lb = a.rec[(size_t)r * a.n_limbs + entry];
    bool swap;
    const uint32_t p = hm_auto_pair(off, a.dst_galois[r], a.logN, swap);
    HmIpPair vy[2][TERMS];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < TERMS; ++j) vy[k][j] = hm_ip_ld(a.y, lb.y[k][j], N, p);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const HmIpPair o = hm_ip_dot<TERMS>(vx, vy[k], swap, m);   // before lb.out[k] is read: two VGPRs fewer at TERMS = 3
      hm_ip_st(a.out, lb.out[k], N, p, o);
    }
  }
}

// weighted sum of rotations, sum_r pt_r * (the hoisted key product of rotation r), formed before anything is stored.  The sum over the
// rotations needs a fixed destination, so this is the GATHER form: a thread owns the aligned pair p of the outputs; rotation by rotation it
// loads every digit's pair at the automorphism's source of p, both keys and the plaintext at p, and adds pt * (the hoisted form's output) to a
// 128-bit accumulator per key and word.  Entries with an addend source (the Q limbs: c0) gather it at the same source and accumulate pt * c0
// as a third output.
// ID (Args = HmIpLinIdOneArgs): the identity step, as in hm_ip_lintrans_multi_thread below.  ID = false is the code as it was.
template <int TERMS, bool ID = false, class Args = HmIpLinArgs>
HM_HD void hm_ip_lintrans_thread(const Args &a, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const uint32_t N = 1u << a.logN;
  const HmIpLinRec &l0 = a.rec[entry];
  const HmMod m = a.mods[l0.mod];
  const bool add = l0.has_add != 0;   // workgroup-uniform
  const uint32_t p = chunk * HM_IP_CHUNK + 2 * tid;
  hm_u128 S[2][2] = {{0, 0}, {0, 0}}, U[2] = {0, 0};
  if constexpr (ID) {
    if (add) {   // the unrotated pairs of c0, c1 and the identity plaintext at p: U starts from pt_0 * c0, W = pt_0 * c1 is stored at once
      const HmIpIdRec &li = a.ids[entry];
      const HmIpPair c0 = hm_ip_ld(a.addend, l0.add_src, N, p), c1 = hm_ip_ld(a.addend1, a.add1_src[entry], N, p), vp = hm_ip_ld(a.pt, li.pt, N, p);
      U[0] = (hm_u128)vp.x * c0.x;
      U[1] = (hm_u128)vp.y * c0.y;
      hm_ip_st(a.addend1_out, li.add1_out, N, p, HmIpPair{hm_barrett((hm_u128)vp.x * c1.x, m), hm_barrett((hm_u128)vp.y * c1.y, m)});
    }
  }
#pragma unroll 1
  for (uint32_t r = 0; r < a.n_rot; ++r) {
    const HmIpLinRec &lb = a.rec[(size_t)r * a.n_limbs + entry];
    bool swap;
    const uint32_t sp = hm_auto_pair(p, a.galois[r], a.logN, swap);
    HmIpPair vx[TERMS], vy[2][TERMS];
#pragma unroll
    for (int j = 0; j < TERMS; ++j) vx[j] = hm_ip_ld(a.x, l0.x[j], N, sp);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < TERMS; ++j) vy[k][j] = hm_ip_ld(a.y, lb.y[k][j], N, p);
    const HmIpPair vp = hm_ip_ld(a.pt, lb.pt, N, p);
    if (add) {
      const HmIpPair vc = hm_ip_ld(a.addend, l0.add_src, N, sp);
      U[0] += (hm_u128)vp.x * (swap ? vc.y : vc.x);
      U[1] += (hm_u128)vp.y * (swap ? vc.x : vc.y);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const HmIpPair t = hm_ip_dot<TERMS>(vx, vy[k], swap, m);
      S[k][0] += (hm_u128)vp.x * t.x;
      S[k][1] += (hm_u128)vp.y * t.y;
    }
  }
  // n_rot <= 16 products of two residues below q < 2^60: every accumulator stays below 2^124, inside 128 bits but beyond hm_barrett's
  // z < 2^(k+63) (sums of up to 8 products), so the top word is folded first (hm_barrett_wide: f < 2^64 + 2q < 2^(k+63) for k > 20)
#pragma unroll
  for (int k = 0; k < 2; ++k) hm_ip_st(a.out, l0.out[k], N, p, HmIpPair{hm_barrett_wide(S[k][0], m), hm_barrett_wide(S[k][1], m)});
  if (add) hm_ip_st(a.addend_out, l0.add_out, N, p, HmIpPair{hm_barrett_wide(U[0], m), hm_barrett_wide(U[1], m)});
}

// n_out weighted sums of the SAME rotations, out_m = sum_r pt_{m,r} * (the hoisted key product of rotation r): the gather form of
// hm_ip_lintrans_thread, whose per-rotation work — the digits' pairs at the automorphism's source of p, both keys at p, t_k = hm_ip_dot — is done
// ONCE for the TILE outputs [tile * TILE, min(n_out, (tile + 1) * TILE)) the thread serves; per output only the plaintext pair is loaded and
// pt * t_k added to that output's own 128-bit accumulators (and pt * c0 to its addend accumulator).  Every output sees exactly the operations of
// hm_ip_lintrans_thread in its order: bit-identical to n_out runs of it.  The accumulators are indexed by unrolled loops only (registers).
//
// ID (hm_inner_product_lintrans_id, Args = HmIpLinIdArgs): the identity step.  On entries with an addend the thread also loads the UNROTATED pairs
// of both addend sources (c0, c1) at p, once per tile: no automorphism, no swap.  Per output it loads that output's identity plaintext pair,
// starts the addend accumulator from pt_0 * c0 instead of zero and stores W = hm_barrett(pt_0 * c1), a single product, as the second addend
// output; the pairs are dead before the rotations start.  n_rot <= 15 keeps the accumulator at 16 products.  ID = false is the code above, untouched.
template <int TERMS, int TILE, bool ID = false, class Args = HmIpLinMultiArgs>
HM_HD void hm_ip_lintrans_multi_thread(const Args &a, uint32_t entry, uint32_t chunk, uint32_t tid, uint32_t tile) {
  const uint32_t N = 1u << a.logN;
  const HmIpLinRec &l0 = a.rec[entry];
  const HmMod m = a.mods[l0.mod];
  const bool add = l0.has_add != 0;   // workgroup-uniform
  const uint32_t p = chunk * HM_IP_CHUNK + 2 * tid, m0 = tile * TILE;
  const uint32_t cnt = a.n_out - m0 < (uint32_t)TILE ? a.n_out - m0 : (uint32_t)TILE;   // (workgroup-uniform) outputs of this tile
  hm_u128 S[TILE][2][2], U[TILE][2];
#pragma unroll
  for (int o = 0; o < TILE; ++o) { S[o][0][0] = S[o][0][1] = S[o][1][0] = S[o][1][1] = 0; U[o][0] = U[o][1] = 0; }
  if constexpr (ID) {
    if (add) {
      const HmIpPair c0 = hm_ip_ld(a.addend, l0.add_src, N, p), c1 = hm_ip_ld(a.addend1, a.add1_src[entry], N, p);
#pragma unroll
      for (int o = 0; o < TILE; ++o) {
        if ((uint32_t)o < cnt) {
          const HmIpIdRec &li = a.ids[(size_t)(m0 + o) * a.n_limbs + entry];
          const HmIpPair vp = hm_ip_ld(a.pt, li.pt, N, p);
          U[o][0] = (hm_u128)vp.x * c0.x;
          U[o][1] = (hm_u128)vp.y * c0.y;
          hm_ip_st(a.addend1_out, li.add1_out, N, p, HmIpPair{hm_barrett((hm_u128)vp.x * c1.x, m), hm_barrett((hm_u128)vp.y * c1.y, m)});
        }
      }
    }
  }
#pragma unroll 1
  for (uint32_t r = 0; r < a.n_rot; ++r) {
    const HmIpLinRec &lb = a.rec[(size_t)r * a.n_limbs + entry];
    bool swap;
    const uint32_t sp = hm_auto_pair(p, a.galois[r], a.logN, swap);
    HmIpPair vx[TERMS], vy[2][TERMS];
#pragma unroll
    for (int j = 0; j < TERMS; ++j) vx[j] = hm_ip_ld(a.x, l0.x[j], N, sp);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < TERMS; ++j) vy[k][j] = hm_ip_ld(a.y, lb.y[k][j], N, p);
    HmIpPair vc{0, 0};
    if (add) {
      const HmIpPair c = hm_ip_ld(a.addend, l0.add_src, N, sp);
      vc = swap ? HmIpPair{c.y, c.x} : c;
    }
    const HmIpPair t0 = hm_ip_dot<TERMS>(vx, vy[0], swap, m), t1 = hm_ip_dot<TERMS>(vx, vy[1], swap, m);
#pragma unroll
    for (int o = 0; o < TILE; ++o) {
      if ((uint32_t)o < cnt) {
        const HmIpPair vp = hm_ip_ld(a.pt, a.pts[((size_t)(m0 + o) * a.n_rot + r) * a.n_limbs + entry], N, p);
        if (add) {
          U[o][0] += (hm_u128)vp.x * vc.x;
          U[o][1] += (hm_u128)vp.y * vc.y;
        }
        S[o][0][0] += (hm_u128)vp.x * t0.x;
        S[o][0][1] += (hm_u128)vp.y * t0.y;
        S[o][1][0] += (hm_u128)vp.x * t1.x;
        S[o][1][1] += (hm_u128)vp.y * t1.y;
      }
    }
  }
  // n_rot <= 16 products below 2^120 per accumulator: below 2^124, reduced once by hm_barrett_wide as in hm_ip_lintrans_thread
#pragma unroll
  for (int o = 0; o < TILE; ++o) {
    if ((uint32_t)o < cnt) {
      const HmIpMultiOut &lo = a.outs[(size_t)(m0 + o) * a.n_limbs + entry];
#pragma unroll
      for (int k = 0; k < 2; ++k) hm_ip_st(a.out, lo.out[k], N, p, HmIpPair{hm_barrett_wide(S[o][k][0], m), hm_barrett_wide(S[o][k][1], m)});
      if (add) hm_ip_st(a.addend_out, lo.add_out, N, p, HmIpPair{hm_barrett_wide(U[o][0], m), hm_barrett_wide(U[o][1], m)});
    }
  }
}

// sum of rotations of n_ct DIFFERENT ciphertexts, sum_c (the key product of ciphertext c through sigma_c), formed before anything is stored: the
// gather form again.  A thread owns the aligned pair p of the outputs; ciphertext by ciphertext it loads every digit's pair at the
// automorphism's source of p, both keys at p, and adds the RAW 64 x 64 products to one 128-bit accumulator per key and word: n_ct * TERMS <=
// 64 products below 2^120 stay below 2^126, and each accumulator is reduced ONCE (hm_barrett_wide takes any 128-bit value).  Entries with
// addend sources (the Q limbs: every ciphertext's c0) gather them at the same source; at most 16 residues below 2^60 sum to below 2^64.
template <int TERMS>
struct HmIpSumOps {   // what one ciphertext brings to the thread's pair
  HmIpPair x[TERMS], y[2][TERMS], c;
  bool swap;
};
template <int TERMS>
HM_HD void hm_ip_rotsum_ld(HmIpSumOps<TERMS> &v, const HmIpSumArgs &a, uint32_t c, uint32_t entry, uint32_t p, bool add) {
  const uint32_t N = 1u << a.logN;
  const HmIpSumRec &lb = a.rec[(size_t)c * a.n_limbs + entry];
  const uint32_t sp = hm_auto_pair(p, a.galois[c], a.logN, v.swap);
#pragma unroll
  for (int j = 0; j < TERMS; ++j) v.x[j] = hm_ip_ld(a.x, lb.x[j], N, sp);
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < TERMS; ++j) v.y[k][j] = hm_ip_ld(a.y, lb.y[k][j], N, p);
  v.c = add ? hm_ip_ld(a.addend, lb.add_src, N, sp) : HmIpPair{0, 0};
}
template <int TERMS>
HM_HD void hm_ip_rotsum_acc(hm_u128 (&S)[2][2], uint64_t (&U)[2], const HmIpSumOps<TERMS> &v) {
#pragma unroll
  for (int j = 0; j < TERMS; ++j) {
    const uint64_t x0 = v.swap ? v.x[j].y : v.x[j].x, x1 = v.swap ? v.x[j].x : v.x[j].y;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      S[k][0] += (hm_u128)x0 * v.y[k][j].x;
      S[k][1] += (hm_u128)x1 * v.y[k][j].y;
    }
  }
  U[0] += v.swap ? v.c.y : v.c.x;
  U[1] += v.swap ? v.c.x : v.c.y;
}
// HM_IP_ROTSUM_AHEAD = 1: the loads of ciphertext c + 1 are issued before the products of ciphertext c are formed, in two named register sets
// (no copy between them), kept above the arithmetic as hm_tensor_dot_thread keeps its own; 0: one ciphertext at a time, the loads where hipcc
// puts them.  The faster form on the MI355X is the default (DESIGN.md section 14 records both).
#ifndef HM_IP_ROTSUM_AHEAD
#define HM_IP_ROTSUM_AHEAD 0
#endif
#if defined(__HIP_DEVICE_COMPILE__) && HM_IP_ROTSUM_AHEAD
#define HM_IP_ROTSUM_ISSUED() __builtin_amdgcn_sched_barrier(0)
#else
#define HM_IP_ROTSUM_ISSUED() ((void)0)
#endif
// INIT (hm_inner_product_rotsum_init, Args = HmIpSumInitArgs): the accumulators start from the loaded pairs init[k] (and the addend accumulator
// from the entry's initial addend sum) at p instead of zero; n_ct <= 15 keeps the addend accumulator at 16 residues.  INIT = false is the code as it was.
template <int TERMS, bool INIT = false, class Args = HmIpSumArgs>
HM_HD void hm_ip_rotsum_thread(const Args &a, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const uint32_t N = 1u << a.logN;
  const HmIpSumRec &l0 = a.rec[entry];
  const HmMod m = a.mods[l0.mod];
  const bool add = l0.has_add != 0;   // workgroup-uniform, the same for every ciphertext of the entry
  const uint32_t p = chunk * HM_IP_CHUNK + 2 * tid, G = a.n_ct;
  hm_u128 S[2][2] = {{0, 0}, {0, 0}};
  uint64_t U[2] = {0, 0};
  if constexpr (INIT) {
    const HmIpSumInit &li = a.inits[entry];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const HmIpPair s = hm_ip_ld(a.init, li.init[k], N, p);
      S[k][0] = s.x;
      S[k][1] = s.y;
    }
    if (add) {
      const HmIpPair u = hm_ip_ld(a.addend, li.add_init, N, p);
      U[0] = u.x;
      U[1] = u.y;
    }
  }
  HmIpSumOps<TERMS> v0;
#if HM_IP_ROTSUM_AHEAD
  HmIpSumOps<TERMS> v1;
  hm_ip_rotsum_ld(v0, a, 0, entry, p, add);
  uint32_t c = 1;
#pragma unroll 1
  for (; c + 1 < G; c += 2) {
    hm_ip_rotsum_ld(v1, a, c, entry, p, add);
    HM_IP_ROTSUM_ISSUED();
    hm_ip_rotsum_acc(S, U, v0);
    hm_ip_rotsum_ld(v0, a, c + 1, entry, p, add);
    HM_IP_ROTSUM_ISSUED();
    hm_ip_rotsum_acc(S, U, v1);
  }
  if (c < G) {   // (wave-uniform) an even number of ciphertexts: one more behind the rounds
    hm_ip_rotsum_ld(v1, a, c, entry, p, add);
    HM_IP_ROTSUM_ISSUED();
    hm_ip_rotsum_acc(S, U, v0);
    hm_ip_rotsum_acc(S, U, v1);
  } else {
    hm_ip_rotsum_acc(S, U, v0);
  }
#else
#pragma unroll 1
  for (uint32_t c = 0; c < G; ++c) {
    hm_ip_rotsum_ld(v0, a, c, entry, p, add);
    hm_ip_rotsum_acc(S, U, v0);
  }
#endif
#pragma unroll
  for (int k = 0; k < 2; ++k) hm_ip_st(a.out, l0.out[k], N, p, HmIpPair{hm_barrett_wide(S[k][0], m), hm_barrett_wide(S[k][1], m)});
  if (add) hm_ip_st(a.addend_out, l0.add_out, N, p, HmIpPair{hm_barrett(U[0], m), hm_barrett(U[1], m)});
}
