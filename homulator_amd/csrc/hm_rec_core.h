// hm_rec_core.h — the record-table element-wise kernels: hm_tensor_dot, hm_tensor_square, hm_lincomb, hm_tensor_muladd, hm_reim_split,
// hm_clincomb, hm_plincomb, hm_tensor_dotadd, hm_lincomb_multi.  Per-thread bodies (no cross-thread state) shared by the HIP kernels (hm_backend.hip: k_tensor_dot, k_tensor_square, k_lincomb,
// k_tensor_muladd, k_reim_split, k_clincomb, k_plincomb, k_tensor_dotadd, k_lincomb_multi) and the host emulator.
//
// A record-table kernel: one record per limb-poly of the call in a device table cached by content, read through the scalar cache (the index is
// wave-uniform); k_tensor's geometry — a workgroup owns 512 coefficients of one record, a thread an aligned pair (16-byte accesses) — and ONE
// launch for any number of records.  A record is a multiple of 16 bytes with its 64-bit values at 8-byte offsets; the host builds it with the
// kernel's own *_fill_recs.
#pragma once
#include <cstddef>
#include "../../include/homulator_hip.h"   // HM_TENSOR_DOT_MAX_TERMS, HM_LINCOMB_MAX_TERMS, HM_TENSOR_MULADD_MAX_ADDENDS, HM_CLINCOMB_MAX_TERMS, HM_PLINCOMB_MAX_TERMS, HM_TENSOR_DOTADD_MAX_TERMS, HM_TENSOR_DOTADD_MAX_ADDENDS, HM_LINCOMB_MULTI_TILE
#include "hm_elem_core.h"                  // HM_CONST_PROB_T, HM_CONST_MODS
#include "hm_modarith.h"
#include "hm_ntt_core.h"

// ---- what every record is written and read with
// host: entry i of a limb list; a null list is the identity
inline uint32_t hm_rec_limb(const uint32_t *l, uint32_t i) { return l ? l[i] : i; }
// host: a 64-bit value into two words of a record
inline void hm_rec_put64(uint32_t *r, uint64_t v) { r[0] = (uint32_t)v; r[1] = (uint32_t)(v >> 32); }
// the 64-bit value in words w, w + 1 of a record
template <class REC>
HM_HD uint64_t hm_rec64(REC rec, uint32_t w) { return (uint64_t)rec[w] | ((uint64_t)rec[w + 1] << 32); }
// the byte offset, inside every limb-poly, of the pair that thread tid of the workgroup of chunk `chunk` owns: coefficients chunk * 512 + 2 tid, + 1
HM_HD uint32_t hm_rec_lane_bytes(uint32_t chunk, uint32_t tid) { return (chunk * 512u + 2u * tid) << 3; }

// hipcc sinks loads to their first use; this keeps what was issued above it above the arithmetic below it (no instruction is emitted)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HM_ABL_DOT_NOPIN)   // (timing-only ablation: the loads where hipcc puts them)
#define HM_DOT_ISSUED() __builtin_amdgcn_sched_barrier(0)
#else
#define HM_DOT_ISSUED() ((void)0)
#endif

// ---- the term loop of the kernels that sum a run-time number of terms (pairs of hm_tensor_dot, terms of hm_lincomb, hm_clincomb and hm_plincomb, addends of hm_tensor_muladd)
// term_at(t): the record words of term t; ld(l): the loads of the term with words l, issued; acc(p): its products into the sums.  Software-
// pipelined by hand: two terms per round in two named register sets p0, p1 (no copy between them), the loads of term t + 1 issued before the
// products of term t are formed, and the record words of a term requested a step before its loads.  The index of that request is clamped to the
// last term, so no word beyond the record is ever read (term_at is never called with t >= T, nor at all for T = 0).
// On entry terms [0, t) are issued: p0 holds the loads of term t - 1, its products still to be formed (have_p0; false only for t = T = 0, a sum
// of no terms), and l = the words of term min(t, T - 1).  An odd number of terms left runs one more behind the rounds; none left (t = T) runs no
// round at all.  Every branch is wave-uniform.
template <class L, class P, class TermAt, class Ld, class Acc>
HM_HD void hm_term_rounds(uint32_t t, uint32_t T, bool have_p0, L l, P p0, TermAt term_at, Ld ld, Acc acc) {
  P p1;
#pragma unroll 1
  for (; t + 1 < T; t += 2) {
    p1 = ld(l);                                   // term t
    l = term_at(t + 1);
    HM_DOT_ISSUED();
    acc(p0);
    p0 = ld(l);                                   // term t + 1
    l = term_at(t + 2 < T ? t + 2 : T - 1);
    HM_DOT_ISSUED();
    acc(p1);
  }
  if (t < T) {
    p1 = ld(l);
    HM_DOT_ISSUED();
    acc(p0);
    acc(p1);
  } else if (have_p0) {
    acc(p0);
  }
}

// ---- Sum of T tensor products in one pass over the 4T inputs (hm_tensor_dot; HDOT):
//   d0 = sum_t a_t b_t,  d1 = sum_t (a_t d_t + c_t b_t),  d2 = sum_t c_t d_t      with a_t = c00, b_t = c10, c_t = c01, d_t = c11 of pair t.
// The raw 64 x 64 products are summed in three 128-bit accumulators per coefficient and each accumulator is reduced ONCE: T <= HM_DOT_MAX_TERMS = 16
// pairs put 2T <= 32 products below 2^120 into d1's, a sum below 2^125, and hm_barrett_wide takes any 128-bit value.  One form on both arithmetic
// back-ends: the launch streams 4T + 3 limb-polys per record and does about ten multiplies per loaded word.
#define HM_DOT_MAX_TERMS HM_TENSOR_DOT_MAX_TERMS
static_assert(HM_DOT_MAX_TERMS <= 16, "d1's accumulator: 2T products below 2^120 must stay below 2^128");
// a record = HM_DOT_REC_WORDS(T) 32-bit words: modulus id, the limbs of d0, d1, d2, then (a, b, c, d) of every pair; a multiple of 16 bytes
#define HM_DOT_REC_WORDS(T) (4u + 4u * (T))
struct HmTensorDotArgs {
  const uint64_t *a, *b, *c, *d;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_DOT_REC_WORDS(n_terms)]
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's limb lists (a .. d: [n][T], o0 .. o2: [n]).  Host side.
inline void hm_tensor_dot_fill_recs(uint32_t *rec, const uint32_t *la, const uint32_t *lb, const uint32_t *lc, const uint32_t *ld, const uint32_t *l0,
                                    const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids, uint32_t n, uint32_t T) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_DOT_REC_WORDS(T);
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(l0, i); r[2] = hm_rec_limb(l1, i); r[3] = hm_rec_limb(l2, i);
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      r[4 + 4 * t] = hm_rec_limb(la, e); r[5 + 4 * t] = hm_rec_limb(lb, e); r[6 + 4 * t] = hm_rec_limb(lc, e); r[7 + 4 * t] = hm_rec_limb(ld, e);
    }
  }
}
struct HmDotAcc {   // one coefficient's three sums
  hm_u128 d0, d1, d2;
};
HM_HD void hm_tensor_dot_acc(HmDotAcc &s, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  s.d0 += (hm_u128)a * b;
  s.d1 += (hm_u128)a * d;
  s.d1 += (hm_u128)c * b;
  s.d2 += (hm_u128)c * d;
}
struct HmDotPair {   // the aligned pair of coefficients a thread owns, of the four operands of one pair of ciphertexts
  uint64_t a[2], b[2], c[2], d[2];
};
struct HmDotLimbs {   // the (a, b, c, d) limbs of one pair: four words of the record
  uint32_t a, b, c, d;
};
template <class REC>
HM_HD HmDotLimbs hm_tensor_dot_limbs(REC rec, uint32_t t) {
  return HmDotLimbs{rec[4 + 4 * t], rec[5 + 4 * t], rec[6 + 4 * t], rec[7 + 4 * t]};
}
// four 16-byte loads from wave-uniform bases at one lane offset
HM_HD HmDotPair hm_tensor_dot_ld(const HmTensorDotArgs &g, const HmDotLimbs &l, size_t N, uint32_t lane_bytes) {
  HmDotPair v;
  hm_bld2(g.a + l.a * N, lane_bytes, v.a[0], v.a[1]);
  hm_bld2(g.b + l.b * N, lane_bytes, v.b[0], v.b[1]);
  hm_bld2(g.c + l.c * N, lane_bytes, v.c[0], v.c[1]);
  hm_bld2(g.d + l.d * N, lane_bytes, v.d[0], v.d[1]);
  return v;
}
HM_HD void hm_tensor_dot_acc2(HmDotAcc (&s)[2], const HmDotPair &v) {
  hm_tensor_dot_acc(s[0], v.a[0], v.b[0], v.c[0], v.d[0]);
  hm_tensor_dot_acc(s[1], v.a[1], v.b[1], v.c[1], v.d[1]);
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: 4T 16-byte loads (hm_term_rounds behind the loads of pair 0), three stores
HM_HD void hm_tensor_dot_thread(const HmTensorDotArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_DOT_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  HmDotAcc s[2] = {{0, 0, 0}, {0, 0, 0}};
  const auto term_at = [&](uint32_t t) { return hm_tensor_dot_limbs(rec, t); };
  const auto ld = [&](const HmDotLimbs &l) { return hm_tensor_dot_ld(g, l, N, lane_bytes); };
  const HmDotPair p0 = ld(term_at(0));
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmDotPair &v) { hm_tensor_dot_acc2(s, v); });
  hm_bst2(g.o0 + rec[1] * N, lane_bytes, hm_barrett_wide(s[0].d0, m), hm_barrett_wide(s[1].d0, m));
  hm_bst2(g.o1 + rec[2] * N, lane_bytes, hm_barrett_wide(s[0].d1, m), hm_barrett_wide(s[1].d1, m));
  hm_bst2(g.o2 + rec[3] * N, lane_bytes, hm_barrett_wide(s[0].d2, m), hm_barrett_wide(s[1].d2, m));
}

// ---- Scaled square of ONE ciphertext plus a constant, in one pass over its two polynomials (hm_tensor_square; HSQUARE):
//   d0 = s a a + k,  d1 = 2 s a c,  d2 = s c c      with a = c0, c = c1, s in [1, q) and k in [0, q) per entry, every residue canonical.
// The tensor product of a ciphertext with itself needs two loads and five products where hm_tensor_one, fed the same operands twice, takes
// four and six; the scalar and the constant are linear and act in front of the key switch, so they are applied here, in registers.
// A record = 64 bytes.  The per-entry constants are stored in the form the arithmetic takes (hm_tensor_square_fill_recs).  mont32: scale =
// s 2^128 mod q, which takes the place of m.r128 in the step to Montgomery form, so that the scalar costs no product at all.  generic: scale = s
// with its Shoup companion scale_s = floor(s 2^64 / q): a and c are multiplied by s once, by two Shoup products, in front of the three Barrett
// products.  addend = k on both.
struct HmTensorSqRec {
  uint32_t mod, a, c, o0, o1, o2;
  uint32_t scaled, pad;   // generic: s != 1 (a limb-uniform branch skips the two products by s)
  uint64_t scale, scale_s, addend, pad1;
};
static_assert(sizeof(HmTensorSqRec) == 64 && offsetof(HmTensorSqRec, scale) == 32, "HmTensorSqRec: layout");
struct HmTensorSqArgs {
  const uint64_t *a, *c;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  const HmTensorSqRec *rec;   // device, [n_limbs]
  uint32_t logN, n_limbs;
};
// host: the record form of the scalar s in [1, q)
inline uint64_t hm_tensor_square_scale(uint64_t s, uint64_t q) { return HM_GENERIC ? s : hm_to_mont(hm_to_mont(s, q), q); }
// The records of n entries from the entry point's limb lists and constants (scale null: 1, addend null: 0; both already checked: reduced,
// scale != 0); q[i] = the modulus of entry i.  Host side.
inline void hm_tensor_square_fill_recs(HmTensorSqRec *rec, const uint32_t *la, const uint32_t *lc, const uint32_t *l0, const uint32_t *l1, const uint32_t *l2,
                                       const uint32_t *mod_ids, const uint64_t *q, uint32_t n, const uint64_t *scale, const uint64_t *addend) {
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t s = scale ? scale[i] : 1;
    rec[i] = HmTensorSqRec{mod_ids[i], hm_rec_limb(la, i), hm_rec_limb(lc, i), hm_rec_limb(l0, i), hm_rec_limb(l1, i), hm_rec_limb(l2, i),
                           s != 1 ? 1u : 0u, 0u, hm_tensor_square_scale(s, q[i]), HM_GENERIC ? hm_shoup_companion(s, q[i]) : 0, addend ? addend[i] : 0, 0};
  }
}
// mont32, with the bound of hm_mont_acc (v <= floor(x wt / 2^64) + q + h + 1, h = q >> 32 < 2^28, for x < 2^63 and no sum above 2^64) and the
// largest modulus the back-end accepts, q < 2^60:
//   at, ct   = a, c (x) st with a, c, st < q: floor(q q / 2^64) < q / 16, so at, ct < 1.0625 q + 2^28 + 1 < 2^61  (a s 2^64 mod q + {0, q})
//   a (x) at, c (x) at, c (x) ct with the left operand below q: floor(q (1.0625 q + 2^28 + 1) / 2^64) < 0.07 q, so each is below 1.07 q + 2^28 + 1
//            < 2 q: ONE conditional subtraction leaves the canonical residue (s a a, s a c, s c c: x wt 2^-64 with wt = y s 2^64)
//   2 x with x < q is below 2 q, and d0 + k with d0, k < q is below 2 q: one conditional subtraction each
//   inside hm_mont_acc, wt < 2^61: b0 w1 < 2^61, b1 w0 < 2^60, (~P0) h < 2^60, cc < 2^60 + 2^33, a sum below 2^63.
// generic: as = s a and cs = s c by the exact Shoup product (canonical, for any 64-bit operand), then three Barrett products of canonical operands.
HM_HD void hm_tensor_square_one(uint64_t a, uint64_t c, uint64_t scale, uint64_t scale_s, uint32_t scaled, uint64_t addend, const HmMod &m, uint64_t &d0,
                                uint64_t &d1, uint64_t &d2) {
#if HM_GENERIC
  uint64_t as = a, cs = c;
  if (scaled) {   // (limb-uniform)
    as = hm_shoup(a, scale, scale_s, m.q);
    cs = hm_shoup(c, scale, scale_s, m.q);
  }
  d0 = hm_mulmod(as, a, m);
  const uint64_t x = hm_mulmod(as, c, m);
  d2 = hm_mulmod(cs, c, m);
  d1 = hm_csub(x + x, m.q);
  d0 = hm_csub(d0 + addend, m.q);
#else
  (void)scaled; (void)scale_s;
  const HmBflyMod bm = hm_bfly_mod(m.q);
  const uint64_t at = hm_mont_acc(0, a, scale, bm), ct = hm_mont_acc(0, c, scale, bm);   // below 1.0625 q + 2^28 + 1
  d0 = hm_csub_neg(hm_mont_acc(0, a, at, bm), bm.nq);                                    // lazy: below 1.07 q + 2^28 + 1
  const uint64_t x = hm_csub_neg(hm_mont_acc(0, c, at, bm), bm.nq);
  d2 = hm_csub_neg(hm_mont_acc(0, c, ct, bm), bm.nq);
  d1 = hm_csub_neg(x + x, bm.nq);          // below 2 q
  d0 = hm_csub_neg(d0 + addend, bm.nq);    // below 2 q
#endif
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: two 16-byte loads, three 16-byte stores
HM_HD void hm_tensor_square_thread(const HmTensorSqArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto r = HM_CONST_PROB_T(HmTensorSqRec, g.rec) + entry;
  const HmMod m = HM_CONST_MODS(g.mods)[r->mod];
  const uint64_t scale = r->scale, scale_s = r->scale_s, addend = r->addend;
  const uint32_t scaled = r->scaled;
  uint64_t a[2], c[2], d0[2], d1[2], d2[2];
  hm_bld2(g.a + r->a * N, lane_bytes, a[0], a[1]);
  hm_bld2(g.c + r->c * N, lane_bytes, c[0], c[1]);
  hm_tensor_square_one(a[0], c[0], scale, scale_s, scaled, addend, m, d0[0], d1[0], d2[0]);
  hm_tensor_square_one(a[1], c[1], scale, scale_s, scaled, addend, m, d0[1], d1[1], d2[1]);
  hm_bst2(g.o0 + r->o0 * N, lane_bytes, d0[0], d0[1]);
  hm_bst2(g.o1 + r->o1 * N, lane_bytes, d1[0], d1[1]);
  hm_bst2(g.o2 + r->o2 * N, lane_bytes, d2[0], d2[1]);
}

// ---- Sum of T scaled polynomials plus a constant in one pass over the T inputs (hm_lincomb; HLINCOMB):
//   out = sum_t s_t x_t + k      with s_t, k in [0, q) per record and every x_t canonical.
// The raw 64 x 64 products are summed in ONE 128-bit accumulator per coefficient, k is added, and the accumulator is reduced once, as
// hm_tensor_dot_acc does: T <= HM_LINCOMB_MAX_TERMS = 16 products below 2^120 are below 2^124, plus k < 2^60 below 2^125, and hm_barrett_wide
// takes any 128-bit value.  The result is the canonical residue of the exact integer sum, hence bit-identical to the chain of MUL_CONST, ADD
// and ADD_CONST.  One form on both arithmetic back-ends: T + 1 limb-polys per record and one wide multiply per loaded word.
static_assert(HM_LINCOMB_MAX_TERMS == 16, "the accumulator: 16 products below 2^120 plus k below 2^60 stay below 2^125");
// a record = HM_LINCOMB_REC_WORDS(T) 32-bit words: (modulus id, output limb, T, 0), (k: 2 words, 0, 0), then per term (input limb, 0, s_t: 2 words)
#define HM_LINCOMB_REC_WORDS(T) (8u + 4u * (T))
struct HmLincombArgs {
  const uint64_t *in;
  uint64_t *out;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_LINCOMB_REC_WORDS(n_terms)]
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's lists (in: [n][T], out: [n]) and constants (scale: [n][T]; addend: [n] or null = 0; both
// already checked: reduced).  Host side.
inline void hm_lincomb_fill_recs(uint32_t *rec, const uint32_t *li, const uint32_t *lo, const uint32_t *mod_ids, uint32_t n, uint32_t T,
                                 const uint64_t *scale, const uint64_t *addend) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_LINCOMB_REC_WORDS(T);
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(lo, i); r[2] = T; r[3] = 0;
    hm_rec_put64(r + 4, addend ? addend[i] : 0); r[6] = 0; r[7] = 0;
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      r[8 + 4 * t] = hm_rec_limb(li, e); r[9 + 4 * t] = 0; hm_rec_put64(r + 10 + 4 * t, scale[e]);
    }
  }
}
struct HmLincombTerm {   // the (input limb, scalar) of one term: four words of the record
  uint32_t limb;
  uint64_t s;
};
template <class REC>
HM_HD HmLincombTerm hm_lincomb_term(REC rec, uint32_t t) {
  return HmLincombTerm{rec[8 + 4 * t], hm_rec64(rec, 10 + 4 * t)};
}
struct HmLincombPair {   // the aligned pair of coefficients a thread owns of one term, with the term's scalar
  uint64_t x[2], s;
};
// one 16-byte load from a wave-uniform base at the lane's offset
HM_HD HmLincombPair hm_lincomb_ld(const HmLincombArgs &g, const HmLincombTerm &l, size_t N, uint32_t lane_bytes) {
  HmLincombPair v;
  hm_bld2(g.in + l.limb * N, lane_bytes, v.x[0], v.x[1]);
  v.s = l.s;
  return v;
}
HM_HD void hm_lincomb_acc2(hm_u128 (&s)[2], const HmLincombPair &v) {
  s[0] += (hm_u128)v.x[0] * v.s;
  s[1] += (hm_u128)v.x[1] * v.s;
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: T 16-byte loads (hm_term_rounds behind the load of term 0), one store
HM_HD void hm_lincomb_thread(const HmLincombArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_LINCOMB_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint64_t k = hm_rec64(rec, 4);
  hm_u128 s[2] = {0, 0};
  const auto term_at = [&](uint32_t t) { return hm_lincomb_term(rec, t); };
  const auto ld = [&](const HmLincombTerm &l) { return hm_lincomb_ld(g, l, N, lane_bytes); };
  const HmLincombPair p0 = ld(term_at(0));
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmLincombPair &v) { hm_lincomb_acc2(s, v); });
  hm_bst2(g.out + rec[1] * N, lane_bytes, hm_barrett_wide(s[0] + k, m), hm_barrett_wide(s[1] + k, m));
}

// ---- M scaled sums of the SAME T polynomials, each plus a constant, the inputs read once per tile of outputs (hm_lincomb_multi; HMLINCOMB,
// DESIGN.md section 26):
//   out_m = sum_t s_{m,t} x_t + k_m      with s_{m,t}, k_m in [0, q) per record and every x_t canonical.
// hm_lincomb's arithmetic per output: the raw 64 x 64 products in ONE 128-bit accumulator per coefficient and output, k_m added, one
// hm_barrett_wide; the bound is hm_lincomb's.  Every output is the canonical residue of the exact integer sum, hence bit-identical to hm_lincomb
// per output.  A record is one limb-poly position with a TILE of up to TILE outputs: the pair of x_t a thread loads goes into 2 TILE
// accumulators, so an entry of M outputs moves ceil(M / TILE) T + M limb-polys where M hm_lincomb records move M (T + 1).  One form on both
// arithmetic back-ends.
static_assert(HM_LINCOMB_MAX_TERMS == 16, "every accumulator: 16 products below 2^120 plus k below 2^60 stay below 2^125");
static_assert(HM_LINCOMB_MULTI_TILE == 4 || HM_LINCOMB_MULTI_TILE == 8, "the two built tiles");
#define HM_LINCOMB_MULTI_TILE_ALT (HM_LINCOMB_MULTI_TILE == 8 ? 4u : 8u)   // the other built tile (hm_set_option "lincomb_multi_tile")
// a record = HM_MLINCOMB_REC_WORDS(T, TILE) 32-bit words, a multiple of 16 bytes:
//   (modulus id, T, outputs in this tile: 1..TILE, 0), the T input limbs (padded with 0 to a multiple of four words), then per output slot of the
//   tile (output limb, 0, k: 2 words, s_{m,0} .. s_{m,T-1}: 2 words each).  The slots behind a short last tile hold zeros and are never used
//   but for their scalars, which the term loop requests with the others (inside the record) and multiplies with nothing.
#define HM_MLINCOMB_REC_HEAD 4u
#define HM_MLINCOMB_SLOT_WORDS(T) (4u + 2u * (T))
#define HM_MLINCOMB_SLOT0(T) (HM_MLINCOMB_REC_HEAD + (((T) + 3u) & ~3u))
#define HM_MLINCOMB_REC_WORDS(T, TILE) (HM_MLINCOMB_SLOT0(T) + (TILE) * HM_MLINCOMB_SLOT_WORDS(T))
// records per entry: the tiles of its M outputs
inline uint32_t hm_lincomb_multi_tiles(uint32_t M, uint32_t tile) { return (M + tile - 1) / tile; }
struct HmLincombMultiArgs {
  const uint64_t *in;
  uint64_t *out;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_MLINCOMB_REC_WORDS(n_terms, TILE)]; n_limbs = records = entries x tiles per entry
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's lists (in: [n][T], out: [n][M]) and constants (scale: [n][M][T]; addend: [n][M] or null = 0;
// both already checked: reduced): hm_lincomb_multi_tiles(M, tile) records per entry, tile after tile.  Host side.
inline void hm_lincomb_multi_fill_recs(uint32_t *rec, const uint32_t *li, const uint32_t *lo, const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t M,
                                       uint32_t tile, const uint64_t *scale, const uint64_t *addend) {
  const uint32_t tiles = hm_lincomb_multi_tiles(M, tile), words = HM_MLINCOMB_REC_WORDS(T, tile);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < tiles; ++r) {
      uint32_t *w = rec + ((size_t)i * tiles + r) * words;
      const uint32_t cnt = M - r * tile < tile ? M - r * tile : tile;
      for (uint32_t x = 0; x < words; ++x) w[x] = 0;
      w[0] = mod_ids[i]; w[1] = T; w[2] = cnt;
      for (uint32_t t = 0; t < T; ++t) w[HM_MLINCOMB_REC_HEAD + t] = hm_rec_limb(li, i * T + t);
      for (uint32_t o = 0; o < cnt; ++o) {
        const size_t e = (size_t)i * M + r * tile + o;
        uint32_t *s = w + HM_MLINCOMB_SLOT0(T) + o * HM_MLINCOMB_SLOT_WORDS(T);
        s[0] = hm_rec_limb(lo, (uint32_t)e);
        hm_rec_put64(s + 2, addend ? addend[e] : 0);
        for (uint32_t t = 0; t < T; ++t) hm_rec_put64(s + 4 + 2 * t, scale[e * T + t]);
      }
    }
}
struct HmLincombMultiTerm {   // the input limb of one term, with the term's index: its scalars are requested with its load
  uint32_t limb, t;
};
template <class REC>
HM_HD HmLincombMultiTerm hm_lincomb_multi_term(REC rec, uint32_t t) {
  return HmLincombMultiTerm{rec[HM_MLINCOMB_REC_HEAD + t], t};
}
template <uint32_t TILE>
struct HmLincombMultiPair {   // the aligned pair of coefficients a thread owns of one term, with the term's scalars
  uint64_t x[2], s[TILE];
};
// the products of one term into the accumulators of the cnt outputs of the tile: the slot index is a compile-time index of an unrolled loop
// (a run-time one would put the accumulators into scratch), a short tile leaves it behind a wave-uniform branch
template <uint32_t TILE>
HM_HD void hm_lincomb_multi_acc(hm_u128 (&s)[TILE][2], const HmLincombMultiPair<TILE> &v, uint32_t cnt) {
#pragma unroll
  for (uint32_t o = 0; o < TILE; ++o) {
    if (o < cnt) {   // (wave-uniform; a branch of its own per slot: an early exit would hand every accumulator on through every exit)
      s[o][0] += (hm_u128)v.x[0] * v.s[o];
      s[o][1] += (hm_u128)v.x[1] * v.s[o];
    }
  }
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: T 16-byte loads (hm_term_rounds behind the load of term 0), then one
// 16-byte store per output of the tile, after all loads.  chunk < N / 512 (the launch has n_limbs N / 512 workgroups), so the last byte touched
// is N * 8 - 1 of each limb-poly.
template <uint32_t TILE>
HM_HD void hm_lincomb_multi_thread(const HmLincombMultiArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_MLINCOMB_REC_WORDS(T, TILE);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint32_t cnt = rec[2];
  hm_u128 s[TILE][2];
#pragma unroll
  for (uint32_t o = 0; o < TILE; ++o) s[o][0] = s[o][1] = 0;
  const auto term_at = [&](uint32_t t) { return hm_lincomb_multi_term(rec, t); };
  // one 16-byte load from a wave-uniform base at the lane's offset; the term's scalar of every slot of the tile is requested beside it (the limb
  // a step ahead, as every term loop's words; the TILE scalars with the load, so that two sets of them are live, not three)
  const auto ld = [&](const HmLincombMultiTerm &l) {
    HmLincombMultiPair<TILE> v;
    hm_bld2(g.in + l.limb * N, lane_bytes, v.x[0], v.x[1]);
#pragma unroll
    for (uint32_t o = 0; o < TILE; ++o) v.s[o] = hm_rec64(rec, HM_MLINCOMB_SLOT0(T) + o * HM_MLINCOMB_SLOT_WORDS(T) + 4 + 2 * l.t);
    return v;
  };
  const HmLincombMultiPair<TILE> p0 = ld(term_at(0));
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmLincombMultiPair<TILE> &v) { hm_lincomb_multi_acc<TILE>(s, v, cnt); });
#pragma unroll
  for (uint32_t o = 0; o < TILE; ++o) {
    if (o < cnt) {   // (wave-uniform)
      const uint32_t w = HM_MLINCOMB_SLOT0(T) + o * HM_MLINCOMB_SLOT_WORDS(T);
      const uint64_t k = hm_rec64(rec, w + 2);
      hm_bst2(g.out + rec[w] * N, lane_bytes, hm_barrett_wide(s[o][0] + k, m), hm_barrett_wide(s[o][1] + k, m));
    }
  }
}

// ---- Scaled tensor product of TWO ciphertexts plus a linear combination of A further ciphertexts plus a constant, in one pass over the 4 + 2A
// inputs (hm_tensor_muladd; HMULADD):
//   d0 = s a b + sum_t u_t x_t + k,  d1 = s (a d + c b) + sum_t u_t y_t,  d2 = s c d
// with hm_tensor_one's roles (a = c00, b = c10, c = c01, d = c11), x_t / y_t = c0 / c1 of addend t, s in [1, q), u_t and k in [0, q) per record and
// every input canonical.  One form on both arithmetic back-ends: a and c are brought to as = s a mod q and cs = s c mod q, canonical, by the
// exact Shoup product (hm_shoup: any 64-bit operand, w < q) behind a limb-uniform branch that s = 1 skips; then the raw 64 x 64 products as b,
// as d + cs b, cs d and u_t x_t, u_t y_t are summed in three 128-bit accumulators per coefficient, k is added to d0's, and each accumulator is
// reduced ONCE by hm_barrett_wide, which takes any 128-bit value.  Every factor is below q < 2^60, so a product is below 2^120: d1's accumulator
// holds 2 + A <= 10 of them, below 10 * 2^120 < 2^124; d0's 1 + A <= 9 and k < 2^60, below 2^124 as well; d2's one.  The result is the canonical
// residue of the exact integer sum, and s a b = (s a mod q) b mod q, hence bit-identical to hm_tensor followed by MUL_CONST, MUL_CONST + ADD per
// addend and ADD_CONST.
#define HM_MULADD_MAX_ADDENDS HM_TENSOR_MULADD_MAX_ADDENDS
static_assert(HM_MULADD_MAX_ADDENDS == 8, "d1's accumulator: 2 + A <= 10 products below 2^120 stay below 2^124; d0's: 1 + A products plus k < 2^60 as well");
// a record = HM_MULADD_REC_WORDS(A) 32-bit words:
//   0: modulus id   1..4: the limbs of a, b, c, d   5..7: the limbs of d0, d1, d2   8: A   9: s != 1
//   10, 11: s   12, 13: its Shoup companion floor(s 2^64 / q)   14, 15: k
// then per addend (limb of x_t, limb of y_t, u_t: 2 words)
#define HM_MULADD_REC_HEAD 16u
#define HM_MULADD_REC_WORDS(A) (HM_MULADD_REC_HEAD + 4u * (A))
struct HmTensorMulAddArgs {
  const uint64_t *a, *b, *c, *d, *x;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_MULADD_REC_WORDS(n_addends)]
  uint32_t logN, n_limbs, n_addends;
};
// The records of n entries from the entry point's limb lists (a .. d, o0 .. o2: [n]; lx0, lx1: [n][A], never null) and constants (scale: [n] or
// null = 1; add_scale: [n][A]; addend: [n] or null = 0; all already checked: reduced, scale != 0); q[i] = the modulus of entry i.  Host side.
inline void hm_tensor_muladd_fill_recs(uint32_t *rec, const uint32_t *la, const uint32_t *lb, const uint32_t *lc, const uint32_t *ld, const uint32_t *lx0,
                                       const uint32_t *lx1, const uint32_t *l0, const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids,
                                       const uint64_t *q, uint32_t n, uint32_t A, const uint64_t *scale, const uint64_t *add_scale, const uint64_t *addend) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_MULADD_REC_WORDS(A);
    const uint64_t s = scale ? scale[i] : 1;
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(la, i); r[2] = hm_rec_limb(lb, i); r[3] = hm_rec_limb(lc, i); r[4] = hm_rec_limb(ld, i);
    r[5] = hm_rec_limb(l0, i); r[6] = hm_rec_limb(l1, i); r[7] = hm_rec_limb(l2, i); r[8] = A; r[9] = s != 1 ? 1u : 0u;
    hm_rec_put64(r + 10, s); hm_rec_put64(r + 12, hm_shoup_companion(s, q[i])); hm_rec_put64(r + 14, addend ? addend[i] : 0);
    for (uint32_t t = 0; t < A; ++t) {
      const uint32_t e = i * A + t;
      uint32_t *w = r + HM_MULADD_REC_HEAD + 4 * t;
      w[0] = lx0[e]; w[1] = lx1[e]; hm_rec_put64(w + 2, add_scale[e]);
    }
  }
}
struct HmMulAddTerm {   // the (limb of x_t, limb of y_t, scalar) of one addend: four words of the record
  uint32_t x, y;
  uint64_t u;
};
// the words of addend t; the caller clamps t to the last addend, and a record without addends hands out words of its header instead (never used):
// always inside the record
template <class REC>
HM_HD HmMulAddTerm hm_muladd_term(REC rec, uint32_t A, uint32_t t) {
  const uint32_t w = A ? HM_MULADD_REC_HEAD + 4 * t : HM_MULADD_REC_HEAD - 4;
  return HmMulAddTerm{rec[w], rec[w + 1], hm_rec64(rec, w + 2)};
}
struct HmMulAddPair {   // the aligned pair of coefficients a thread owns of both components of one addend, with the addend's scalar
  uint64_t x[2], y[2], u;
};
// two 16-byte loads from wave-uniform bases at the lane's offset
HM_HD HmMulAddPair hm_muladd_ld(const HmTensorMulAddArgs &g, const HmMulAddTerm &l, size_t N, uint32_t lane_bytes) {
  HmMulAddPair v;
  hm_bld2(g.x + l.x * N, lane_bytes, v.x[0], v.x[1]);
  hm_bld2(g.x + l.y * N, lane_bytes, v.y[0], v.y[1]);
  v.u = l.u;
  return v;
}
HM_HD void hm_muladd_acc2(HmDotAcc (&s)[2], const HmMulAddPair &v) {
  s[0].d0 += (hm_u128)v.x[0] * v.u;
  s[0].d1 += (hm_u128)v.y[0] * v.u;
  s[1].d0 += (hm_u128)v.x[1] * v.u;
  s[1].d1 += (hm_u128)v.y[1] * v.u;
}
// the scaled product of one coefficient into fresh accumulators
HM_HD void hm_muladd_product(HmDotAcc &s, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t scale, uint64_t scale_s, uint32_t scaled, uint64_t k,
                             const HmMod &m) {
  uint64_t as = a, cs = c;
  if (scaled) {   // (limb-uniform)
    as = hm_shoup(a, scale, scale_s, m.q);
    cs = hm_shoup(c, scale, scale_s, m.q);
  }
  s.d0 = (hm_u128)as * b + k;
  s.d1 = (hm_u128)as * d + (hm_u128)cs * b;
  s.d2 = (hm_u128)cs * d;
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: four 16-byte loads for the product, two per addend, three 16-byte stores.
// The product stands in the place of hm_term_rounds' first term: the loads of addend 0 are issued under it, before its products are formed
// (hm_muladd_term: always inside the record), and the rounds go on from addend 1.  A = 0 and A = 1 run no round.
HM_HD void hm_tensor_muladd_thread(const HmTensorMulAddArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t A = g.n_addends, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_MULADD_REC_WORDS(A);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint32_t scaled = rec[9];
  const uint64_t scale = hm_rec64(rec, 10), scale_s = hm_rec64(rec, 12), k = hm_rec64(rec, 14);
  const auto term_at = [&](uint32_t t) { return hm_muladd_term(rec, A, t); };
  const auto ld = [&](const HmMulAddTerm &l) { return hm_muladd_ld(g, l, N, lane_bytes); };
  HmDotPair v;
  hm_bld2(g.a + rec[1] * N, lane_bytes, v.a[0], v.a[1]);
  hm_bld2(g.b + rec[2] * N, lane_bytes, v.b[0], v.b[1]);
  hm_bld2(g.c + rec[3] * N, lane_bytes, v.c[0], v.c[1]);
  hm_bld2(g.d + rec[4] * N, lane_bytes, v.d[0], v.d[1]);
  HmMulAddTerm l = term_at(0);
  HmMulAddPair p0;   // (A = 0 leaves it unwritten: hm_term_rounds, handed it by value, then reads none of it; zeroing it costs nine instructions)
  if (A > 0) {   // (wave-uniform) addend 0 under the product
    p0 = ld(l);
    l = term_at(A > 1 ? 1u : 0u);
  }
  HM_DOT_ISSUED();
  HmDotAcc s[2];
  hm_muladd_product(s[0], v.a[0], v.b[0], v.c[0], v.d[0], scale, scale_s, scaled, k, m);
  hm_muladd_product(s[1], v.a[1], v.b[1], v.c[1], v.d[1], scale, scale_s, scaled, k, m);
  hm_term_rounds(A ? 1u : 0u, A, A > 0, l, p0, term_at, ld, [&](const HmMulAddPair &p) { hm_muladd_acc2(s, p); });
  hm_bst2(g.o0 + rec[5] * N, lane_bytes, hm_barrett_wide(s[0].d0, m), hm_barrett_wide(s[1].d0, m));
  hm_bst2(g.o1 + rec[6] * N, lane_bytes, hm_barrett_wide(s[0].d1, m), hm_barrett_wide(s[1].d1, m));
  hm_bst2(g.o2 + rec[7] * N, lane_bytes, hm_barrett_wide(s[0].d2, m), hm_barrett_wide(s[1].d2, m));
}

// ---- Real and imaginary parts of the slots from a polynomial x and its conjugate y in one pass over both (hm_reim_split; HREIM):
//   re = x + y,   im = U (.) (x - y)
// with U the evaluation form of -X^(N/2).  Entry e of a limb-poly holds the value at psi^(2 brev(e) + 1); for e < N/2 the exponent is 1 mod 4, for
// e >= N/2 it is 3 mod 4, and psi^(N/2) has order 4: U is the constant w = -psi^(N/2) mod q on entries [0, N/2) and q - w on [N/2, N), w^2 = -1.
// A workgroup's 512 coefficients lie in one half (N >= 1024), so the choice is uniform per workgroup: chunk < N/1024 takes w.
// One form on both arithmetic back-ends, every input canonical (< q < 2^60):
//   re = hm_addmod(x, y): x + y < 2q < 2^61, one conditional subtraction, canonical;
//   d  = hm_submod(x, y): in [0, q), canonical;
//   im = hm_shoup(d, u, us, q): exact for any 64-bit d and u < q with us = floor(u 2^64 / q), canonical (hm_modarith.h).
// The record carries w and ws = floor(w 2^64 / q) only.  For u = q - w: (q - w) 2^64 / q = 2^64 - w 2^64 / q, and w 2^64 / q is no integer (q is
// an odd prime, 0 < w < q), so floor((q - w) 2^64 / q) = 2^64 - 1 - ws = ~ws, exactly.
// Bit-identical to HM_OP_ADD, HM_OP_SUB and HM_OP_MUL by the stored U: each of those yields the canonical residue of the same exact value.
// a record = HM_REIM_REC_WORDS 32-bit words (48 bytes):
//   0: modulus id   1, 2: the limbs of x, y   3, 4: the limbs of re, im   5..7: 0   8, 9: w   10, 11: ws
#define HM_REIM_REC_WORDS 12u
struct HmReimArgs {
  const uint64_t *x, *y;
  uint64_t *o_re, *o_im;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_REIM_REC_WORDS]
  uint32_t logN, n_limbs;
};
// The records of n entries from the entry point's limb lists; w[i] = -psi^(N/2) mod q[i], q[i] = the modulus of entry i.  Host side.
inline void hm_reim_fill_recs(uint32_t *rec, const uint32_t *lx, const uint32_t *ly, const uint32_t *lre, const uint32_t *lim, const uint32_t *mod_ids,
                              const uint64_t *w, const uint64_t *q, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_REIM_REC_WORDS;
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(lx, i); r[2] = hm_rec_limb(ly, i); r[3] = hm_rec_limb(lre, i); r[4] = hm_rec_limb(lim, i);
    r[5] = r[6] = r[7] = 0;
    hm_rec_put64(r + 8, w[i]); hm_rec_put64(r + 10, hm_shoup_companion(w[i], q[i]));
  }
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: two 16-byte loads and two 16-byte stores.  chunk < N / 512 (the launch
// has n N / 512 workgroups), so the last byte touched is N * 8 - 1 of each limb-poly.
HM_HD void hm_reim_thread(const HmReimArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_REIM_REC_WORDS;
  const uint64_t q = HM_CONST_MODS(g.mods)[rec[0]].q;
  const uint64_t w = hm_rec64(rec, 8), ws = hm_rec64(rec, 10);
  const bool first = chunk < (uint32_t)(N >> 10);   // (workgroup-uniform) entries [0, N/2)
  const uint64_t u = first ? w : q - w, us = first ? ws : ~ws;
  uint64_t x[2], y[2];
  hm_bld2(g.x + rec[1] * N, lane_bytes, x[0], x[1]);
  hm_bld2(g.y + rec[2] * N, lane_bytes, y[0], y[1]);
  hm_bst2(g.o_re + rec[3] * N, lane_bytes, hm_addmod(x[0], y[0], q), hm_addmod(x[1], y[1], q));
  hm_bst2(g.o_im + rec[4] * N, lane_bytes, hm_shoup(hm_submod(x[0], y[0], q), u, us, q), hm_shoup(hm_submod(x[1], y[1], q), u, us, q));
}

// ---- Sum of T polynomials, each times a + b X^(N/2), plus a constant, in one pass over the T inputs (hm_clincomb; HCLINCOMB):
//   out = sum_t (a_t + b_t X^(N/2)) x_t + (k_re + k_im X^(N/2))      with a_t, b_t, k_re, k_im in [0, q) per record and every x_t canonical.
// In evaluation form X^(N/2) is the constant v = psi^(N/2) on entries [0, N/2) of a limb-poly and q - v on [N/2, N) (hm_reim_split above: its w is
// q - v), v^2 = -1.  So the factor of term t is ONE scalar per half,
//   s_lo = a_t + b_t v mod q   on [0, N/2),      s_hi = a_t - b_t v mod q   on [N/2, N),
// and the constant k_lo = k_re + k_im v, k_hi = k_re - k_im v likewise: the host forms the halves when it fills the records (hm_clincomb_halves)
// and the kernel picks one set per workgroup, whose 512 coefficients lie in one half (N >= 1024): chunk < N/1024 takes the _lo words.  From there
// it is hm_lincomb's arithmetic on both back-ends: raw 64 x 64 products in ONE 128-bit accumulator per coefficient, the constant added, one
// hm_barrett_wide.  s_lo, s_hi, k_lo, k_hi < q < 2^60, so the bound is hm_lincomb's: T <= HM_CLINCOMB_MAX_TERMS = 16 products below 2^120 are below
// 2^124, plus a constant below 2^60 below 2^125.  The result is the canonical residue of the exact sum, hence bit-identical to the chain of
// MUL_CONST, MUL by the stored monomial, ADD and ADD_CONST.  T + 1 limb-polys per record and one wide multiply per loaded word.
static_assert(HM_CLINCOMB_MAX_TERMS == 16, "the accumulator: 16 products below 2^120 plus a constant below 2^60 stay below 2^125");
// a record = HM_CLINCOMB_REC_WORDS(T) 32-bit words (32 + 32 T bytes):
//   (modulus id, output limb, T, 0), (k_lo: 2 words, k_hi: 2 words), then per term (input limb, 0, s_lo: 2 words, s_hi: 2 words, 0, 0)
#define HM_CLINCOMB_REC_HEAD 8u
#define HM_CLINCOMB_REC_WORDS(T) (HM_CLINCOMB_REC_HEAD + 8u * (T))
struct HmClincombArgs {
  const uint64_t *in;
  uint64_t *out;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_CLINCOMB_REC_WORDS(n_terms)]
  uint32_t logN, n_limbs, n_terms;
};
// host: the two halves of a + b X^(N/2) in evaluation form, v = psi^(N/2) mod q; a, b, v < q
inline void hm_clincomb_halves(uint64_t a, uint64_t b, uint64_t v, uint64_t q, uint64_t &lo, uint64_t &hi) {
  const uint64_t bv = (uint64_t)(((unsigned __int128)b * v) % q);
  lo = a + bv >= q ? a + bv - q : a + bv;
  hi = a >= bv ? a - bv : a + q - bv;
}
// The records of n entries from the entry point's lists (in: [n][T], out: [n]) and constants (re: [n][T]; im: [n][T] or null = 0; add_re, add_im:
// [n] or null = 0; all already checked: reduced); v[i] = psi^(N/2) mod q[i], q[i] = the modulus of entry i.  Host side.
inline void hm_clincomb_fill_recs(uint32_t *rec, const uint32_t *li, const uint32_t *lo, const uint32_t *mod_ids, const uint64_t *v, const uint64_t *q,
                                  uint32_t n, uint32_t T, const uint64_t *re, const uint64_t *im, const uint64_t *add_re, const uint64_t *add_im) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_CLINCOMB_REC_WORDS(T);
    uint64_t s_lo, s_hi;
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(lo, i); r[2] = T; r[3] = 0;
    hm_clincomb_halves(add_re ? add_re[i] : 0, add_im ? add_im[i] : 0, v[i], q[i], s_lo, s_hi);
    hm_rec_put64(r + 4, s_lo); hm_rec_put64(r + 6, s_hi);
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      uint32_t *w = r + HM_CLINCOMB_REC_HEAD + 8 * t;
      hm_clincomb_halves(re[e], im ? im[e] : 0, v[i], q[i], s_lo, s_hi);
      w[0] = hm_rec_limb(li, e); w[1] = 0; hm_rec_put64(w + 2, s_lo); hm_rec_put64(w + 4, s_hi); w[6] = 0; w[7] = 0;
    }
  }
}
// the (input limb, scalar of the workgroup's half) of term t: hi = 0 takes s_lo, hi = 2 takes s_hi (the word offset of the half)
template <class REC>
HM_HD HmLincombTerm hm_clincomb_term(REC rec, uint32_t t, uint32_t hi) {
  const uint32_t w = HM_CLINCOMB_REC_HEAD + 8 * t;
  return HmLincombTerm{rec[w], hm_rec64(rec, w + 2 + hi)};
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: T 16-byte loads (hm_term_rounds behind the load of term 0), one store.
// chunk < N / 512 (the launch has n N / 512 workgroups), so the last byte touched is N * 8 - 1 of each limb-poly.
HM_HD void hm_clincomb_thread(const HmClincombArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_CLINCOMB_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint32_t hi = chunk < (uint32_t)(N >> 10) ? 0u : 2u;   // (workgroup-uniform) entries [0, N/2) take the _lo words
  const uint64_t k = hm_rec64(rec, 4 + hi);
  hm_u128 s[2] = {0, 0};
  const auto term_at = [&](uint32_t t) { return hm_clincomb_term(rec, t, hi); };
  const auto ld = [&](const HmLincombTerm &l) {
    HmLincombPair v;
    hm_bld2(g.in + l.limb * N, lane_bytes, v.x[0], v.x[1]);
    v.s = l.s;
    return v;
  };
  const HmLincombPair p0 = ld(term_at(0));
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmLincombPair &v) { hm_lincomb_acc2(s, v); });
  hm_bst2(g.out + rec[1] * N, lane_bytes, hm_barrett_wide(s[0] + k, m), hm_barrett_wide(s[1] + k, m));
}

// ---- Sum of T ciphertexts, each times a plaintext, plus a plaintext on c0, in one pass over the 3T inputs (hm_plincomb; HPLINCOMB):
//   o0 = sum_t p_t (.) x_t + p_0,   o1 = sum_t p_t (.) y_t      with p_t a limb-poly of plaintext t, x_t / y_t = c0 / c1 of ciphertext t, every
// residue canonical.  A record is one output limb with BOTH components: the pair of p_t a thread loads serves the product with x_t and the one with
// y_t, so a term costs three 16-byte loads where two separate sums would take four.  The raw 64 x 64 products are summed in TWO 128-bit
// accumulators per coefficient (c0's and c1's), the addend goes into c0's, and each accumulator is reduced once: T <= HM_PLINCOMB_MAX_TERMS = 16
// products below 2^120 are below 2^124, plus an addend below 2^60 below 2^125, and hm_barrett_wide takes any 128-bit value.  The result is the
// canonical residue of the exact integer sum, hence bit-identical to the chain of MUL, MAC_ADD and ADD.  One form on both arithmetic back-ends:
// 3T + 2 (+ 1) limb-polys per record and two wide multiplies per three loaded words.
static_assert(HM_PLINCOMB_MAX_TERMS == 16, "either accumulator: 16 products below 2^120 plus an addend below 2^60 stay below 2^125");
// a record = HM_PLINCOMB_REC_WORDS(T) 32-bit words (32 + 16 T bytes):
//   (modulus id, limb of o0, limb of o1, T), (addend flag, addend limb, 0, 0), then per term (limb of p_t, limb of x_t, limb of y_t, 0)
#define HM_PLINCOMB_REC_HEAD 8u
#define HM_PLINCOMB_REC_WORDS(T) (HM_PLINCOMB_REC_HEAD + 4u * (T))
struct HmPlincombArgs {
  const uint64_t *p, *x, *addend;   // addend: any readable buffer when no record has one (never loaded from)
  uint64_t *out;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_PLINCOMB_REC_WORDS(n_terms)]
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's limb lists (lp, lx0, lx1: [n][T]; l0, l1: [n]; la: [n], read with has_addend only).  Host side.
inline void hm_plincomb_fill_recs(uint32_t *rec, const uint32_t *lp, const uint32_t *lx0, const uint32_t *lx1, bool has_addend, const uint32_t *la,
                                  const uint32_t *l0, const uint32_t *l1, const uint32_t *mod_ids, uint32_t n, uint32_t T) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_PLINCOMB_REC_WORDS(T);
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(l0, i); r[2] = hm_rec_limb(l1, i); r[3] = T;
    r[4] = has_addend ? 1u : 0u; r[5] = has_addend ? hm_rec_limb(la, i) : 0u; r[6] = 0; r[7] = 0;
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      uint32_t *w = r + HM_PLINCOMB_REC_HEAD + 4 * t;
      w[0] = hm_rec_limb(lp, e); w[1] = hm_rec_limb(lx0, e); w[2] = hm_rec_limb(lx1, e); w[3] = 0;
    }
  }
}
struct HmPlincombLimbs {   // the limbs of (p_t, x_t, y_t) of one term: three words of the record
  uint32_t p, x, y;
};
template <class REC>
HM_HD HmPlincombLimbs hm_plincomb_limbs(REC rec, uint32_t t) {
  const uint32_t w = HM_PLINCOMB_REC_HEAD + 4 * t;
  return HmPlincombLimbs{rec[w], rec[w + 1], rec[w + 2]};
}
struct HmPlincombPair {   // the aligned pair of coefficients a thread owns of the plaintext and of both components of one term
  uint64_t p[2], x[2], y[2];
};
struct HmPlincombAcc {   // one coefficient's two sums
  hm_u128 c0, c1;
};
// three 16-byte loads from wave-uniform bases at the lane's offset
HM_HD HmPlincombPair hm_plincomb_ld(const HmPlincombArgs &g, const HmPlincombLimbs &l, size_t N, uint32_t lane_bytes) {
  HmPlincombPair v;
  hm_bld2(g.p + l.p * N, lane_bytes, v.p[0], v.p[1]);
  hm_bld2(g.x + l.x * N, lane_bytes, v.x[0], v.x[1]);
  hm_bld2(g.x + l.y * N, lane_bytes, v.y[0], v.y[1]);
  return v;
}
HM_HD void hm_plincomb_acc2(HmPlincombAcc (&s)[2], const HmPlincombPair &v) {
  s[0].c0 += (hm_u128)v.p[0] * v.x[0];
  s[0].c1 += (hm_u128)v.p[0] * v.y[0];
  s[1].c0 += (hm_u128)v.p[1] * v.x[1];
  s[1].c1 += (hm_u128)v.p[1] * v.y[1];
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: 3T 16-byte loads (hm_term_rounds behind the loads of term 0), one more for
// the addend behind a record-uniform flag, two 16-byte stores.  chunk < N / 512 (the launch has n N / 512 workgroups), so the last byte touched is
// N * 8 - 1 of each limb-poly.
HM_HD void hm_plincomb_thread(const HmPlincombArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_PLINCOMB_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  uint64_t k[2] = {0, 0};
  if (rec[4]) hm_bld2(g.addend + rec[5] * N, lane_bytes, k[0], k[1]);   // (record-uniform)
  const auto term_at = [&](uint32_t t) { return hm_plincomb_limbs(rec, t); };
  const auto ld = [&](const HmPlincombLimbs &l) { return hm_plincomb_ld(g, l, N, lane_bytes); };
  const HmPlincombPair p0 = ld(term_at(0));
  HmPlincombAcc s[2] = {{k[0], 0}, {k[1], 0}};
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmPlincombPair &v) { hm_plincomb_acc2(s, v); });
  hm_bst2(g.out + rec[1] * N, lane_bytes, hm_barrett_wide(s[0].c0, m), hm_barrett_wide(s[1].c0, m));
  hm_bst2(g.out + rec[2] * N, lane_bytes, hm_barrett_wide(s[0].c1, m), hm_barrett_wide(s[1].c1, m));
}

// ---- Scaled sum of T tensor products plus a linear combination of A further ciphertexts plus a constant, in one pass over the 4T + 2A inputs
// (hm_tensor_dotadd; HDOTADD):
//   d0 = sum_t s_t a_t b_t + sum_r u_r x_r + k,  d1 = sum_t s_t (a_t d_t + c_t b_t) + sum_r u_r y_r,  d2 = sum_t s_t c_t d_t
// with hm_tensor_dot's roles per pair (a_t = c00, b_t = c10, c_t = c01, d_t = c11), x_r / y_r = c0 / c1 of addend r, s_t in [1, q), u_r and k in
// [0, q) per record and every input canonical.  One form on both arithmetic back-ends: a pair with s_t != 1 first brings a_t and c_t to
// s_t a_t mod q and s_t c_t mod q, canonical, by the exact Shoup product (hm_shoup: any 64-bit operand, w < q) behind a wave-uniform branch that
// s_t = 1 skips; then the raw 64 x 64 products of every pair and every addend are summed in three 128-bit accumulators per coefficient
// (HmDotAcc), k is added to d0's, and each accumulator is reduced ONCE by hm_barrett_wide, which takes any 128-bit value.  Every factor is below
// q < 2^60, so a product is below 2^120: d1's accumulator holds 2T + A <= 40 of them, below 40 * 2^120 < 2^126; d0's T + A <= 24 and k < 2^60;
// d2's T <= 16.  The result is the canonical residue of the exact integer sum, and s a b = (s a mod q) b mod q, hence bit-identical to hm_tensor
// per pair followed by MUL_CONST, ADD, MUL_CONST + ADD per addend and ADD_CONST.
#define HM_DOTADD_MAX_TERMS HM_TENSOR_DOTADD_MAX_TERMS
#define HM_DOTADD_MAX_ADDENDS HM_TENSOR_DOTADD_MAX_ADDENDS
static_assert(HM_DOTADD_MAX_TERMS == 16 && HM_DOTADD_MAX_ADDENDS == 8,
              "d1's accumulator: 2T + A <= 40 products below 2^120 stay below 2^126; d0's: T + A <= 24 products plus k < 2^60 as well");
// a record = HM_DOTADD_REC_WORDS(T, A) 32-bit words (32 + 32 T + 16 A bytes):
//   0: modulus id   1..3: the limbs of d0, d1, d2   4: T   5: A   6, 7: k
// then per pair (limbs of a, b, c, d; s_t: 2 words; its Shoup companion floor(s_t 2^64 / q): 2 words)
// then per addend (limb of x_r, limb of y_r, u_r: 2 words) — hm_tensor_muladd's addend words
#define HM_DOTADD_REC_HEAD 8u
#define HM_DOTADD_REC_ADDENDS(T) (HM_DOTADD_REC_HEAD + 8u * (T))
#define HM_DOTADD_REC_WORDS(T, A) (HM_DOTADD_REC_ADDENDS(T) + 4u * (A))
struct HmTensorDotAddArgs {
  const uint64_t *a, *b, *c, *d, *x;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_DOTADD_REC_WORDS(n_terms, n_addends)]
  uint32_t logN, n_limbs, n_terms, n_addends;
};
// The records of n entries from the entry point's limb lists (a .. d: [n][T], o0 .. o2: [n], a null list is the identity; lx0, lx1: [n][A], never
// null at A > 0) and constants (scale: [n][T] or null = 1; add_scale: [n][A]; addend: [n] or null = 0; all already checked: reduced, scale != 0);
// q[i] = the modulus of entry i.  Host side.
inline void hm_tensor_dotadd_fill_recs(uint32_t *rec, const uint32_t *la, const uint32_t *lb, const uint32_t *lc, const uint32_t *ld, const uint32_t *lx0,
                                       const uint32_t *lx1, const uint32_t *l0, const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids,
                                       const uint64_t *q, uint32_t n, uint32_t T, uint32_t A, const uint64_t *scale, const uint64_t *add_scale,
                                       const uint64_t *addend) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_DOTADD_REC_WORDS(T, A);
    r[0] = mod_ids[i]; r[1] = hm_rec_limb(l0, i); r[2] = hm_rec_limb(l1, i); r[3] = hm_rec_limb(l2, i); r[4] = T; r[5] = A;
    hm_rec_put64(r + 6, addend ? addend[i] : 0);
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      const uint64_t s = scale ? scale[e] : 1;
      uint32_t *w = r + HM_DOTADD_REC_HEAD + 8 * t;
      w[0] = hm_rec_limb(la, e); w[1] = hm_rec_limb(lb, e); w[2] = hm_rec_limb(lc, e); w[3] = hm_rec_limb(ld, e);
      hm_rec_put64(w + 4, s); hm_rec_put64(w + 6, hm_shoup_companion(s, q[i]));
    }
    for (uint32_t t = 0; t < A; ++t) {
      const uint32_t e = i * A + t;
      uint32_t *w = r + HM_DOTADD_REC_ADDENDS(T) + 4 * t;
      w[0] = lx0[e]; w[1] = lx1[e]; hm_rec_put64(w + 2, add_scale[e]);
    }
  }
}
struct HmDotAddTerm {   // the limbs of one pair with its scalar and the scalar's Shoup companion: eight words of the record
  HmDotLimbs l;
  uint64_t s, ss;
};
template <class REC>
HM_HD HmDotAddTerm hm_dotadd_term(REC rec, uint32_t t) {
  const uint32_t w = HM_DOTADD_REC_HEAD + 8 * t;
  return HmDotAddTerm{HmDotLimbs{rec[w], rec[w + 1], rec[w + 2], rec[w + 3]}, hm_rec64(rec, w + 4), hm_rec64(rec, w + 6)};
}
// the words of addend r; the caller clamps r to the last addend, and a record without addends hands out words of its header instead (never used):
// always inside the record
template <class REC>
HM_HD HmMulAddTerm hm_dotadd_addend(REC rec, uint32_t T, uint32_t A, uint32_t r) {
  const uint32_t w = A ? HM_DOTADD_REC_ADDENDS(T) + 4 * r : HM_DOTADD_REC_HEAD - 4;
  return HmMulAddTerm{rec[w], rec[w + 1], hm_rec64(rec, w + 2)};
}
struct HmDotAddPair {   // the aligned pair of coefficients a thread owns of the four operands of one pair, with the pair's scalar
  HmDotPair v;
  uint64_t s, ss;
};
// one coefficient of one pair into the sums: s = 1 leaves a and c as they are
HM_HD void hm_tensor_dotadd_acc(HmDotAcc &acc, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t s, uint64_t ss, uint64_t q) {
  uint64_t as = a, cs = c;
  if (s != 1) {   // (wave-uniform)
    as = hm_shoup(a, s, ss, q);
    cs = hm_shoup(c, s, ss, q);
  }
  hm_tensor_dot_acc(acc, as, b, cs, d);
}
HM_HD void hm_tensor_dotadd_acc2(HmDotAcc (&acc)[2], const HmDotAddPair &p, uint64_t q) {
  hm_tensor_dotadd_acc(acc[0], p.v.a[0], p.v.b[0], p.v.c[0], p.v.d[0], p.s, p.ss, q);
  hm_tensor_dotadd_acc(acc[1], p.v.a[1], p.v.b[1], p.v.c[1], p.v.d[1], p.s, p.ss, q);
}
// thread tid of the workgroup that owns chunk `chunk` of record `entry`: four 16-byte loads per pair, two per addend, three 16-byte stores.
// hm_term_rounds twice: over the pairs behind the loads of pair 0, as hm_tensor_dot_thread, then over the addends, as hm_tensor_muladd_thread.  The
// loads of addend 0 are issued together with pair 0's and held through the pair loop (8 VGPRs and the scalar), so the addend loop starts with its
// first term in flight.  chunk < N / 512 (the launch has n N / 512 workgroups), so the last byte touched is N * 8 - 1 of each limb-poly.
HM_HD void hm_tensor_dotadd_thread(const HmTensorDotAddArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, A = g.n_addends, lane_bytes = hm_rec_lane_bytes(chunk, tid);
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_DOTADD_REC_WORDS(T, A);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint64_t k = hm_rec64(rec, 6);
  const auto term_at = [&](uint32_t t) { return hm_dotadd_term(rec, t); };
  const auto ld = [&](const HmDotAddTerm &l) {
    HmDotAddPair p;
    hm_bld2(g.a + l.l.a * N, lane_bytes, p.v.a[0], p.v.a[1]);
    hm_bld2(g.b + l.l.b * N, lane_bytes, p.v.b[0], p.v.b[1]);
    hm_bld2(g.c + l.l.c * N, lane_bytes, p.v.c[0], p.v.c[1]);
    hm_bld2(g.d + l.l.d * N, lane_bytes, p.v.d[0], p.v.d[1]);
    p.s = l.s; p.ss = l.ss;
    return p;
  };
  const auto addend_at = [&](uint32_t r) { return hm_dotadd_addend(rec, T, A, r); };
  const auto ld_addend = [&](const HmMulAddTerm &l) {
    HmMulAddPair p;
    hm_bld2(g.x + l.x * N, lane_bytes, p.x[0], p.x[1]);
    hm_bld2(g.x + l.y * N, lane_bytes, p.y[0], p.y[1]);
    p.u = l.u;
    return p;
  };
  const HmDotAddPair p0 = ld(term_at(0));
  HmMulAddTerm la = addend_at(0);
  HmMulAddPair x0;   // (A = 0 leaves it unwritten: hm_term_rounds, handed it by value, then reads none of it)
  if (A > 0) {   // (wave-uniform) addend 0 under the pairs
    x0 = ld_addend(la);
    la = addend_at(A > 1 ? 1u : 0u);
  }
  HM_DOT_ISSUED();
  HmDotAcc s[2] = {{k, 0, 0}, {k, 0, 0}};
  hm_term_rounds(1, T, true, term_at(T > 1 ? 1u : 0u), p0, term_at, ld, [&](const HmDotAddPair &p) { hm_tensor_dotadd_acc2(s, p, m.q); });
  hm_term_rounds(A ? 1u : 0u, A, A > 0, la, x0, addend_at, ld_addend, [&](const HmMulAddPair &p) { hm_muladd_acc2(s, p); });
  hm_bst2(g.o0 + rec[1] * N, lane_bytes, hm_barrett_wide(s[0].d0, m), hm_barrett_wide(s[1].d0, m));
  hm_bst2(g.o1 + rec[2] * N, lane_bytes, hm_barrett_wide(s[0].d1, m), hm_barrett_wide(s[1].d1, m));
  hm_bst2(g.o2 + rec[3] * N, lane_bytes, hm_barrett_wide(s[0].d2, m), hm_barrett_wide(s[1].d2, m));
}
