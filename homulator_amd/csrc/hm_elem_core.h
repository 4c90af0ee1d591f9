// hm_elem_core.h — K2 automorphism, K3 element-wise engine, K4 base conversion, synthetic fill.
// Per-thread bodies (no cross-thread state) shared by the HIP kernels and the host emulator.
//
// Reference shapes (the reference carries address tokens only; the arithmetic is the build's):
//   K3 EWE   InsGen::GenEWE src/InsGen.cpp:77-125, "(op1 x op2) + (op3 x op4)" :90-95,
//            adder tree src/Components.cpp:8-57.  Upstream has no opcode (always tagged MULT);
//            the opcodes below are what the stages of src/Operation.cpp actually need.
//   K4 BCONV InsGen::GenBCONV src/InsGen.cpp:263-313 (an InLevel-deep MAC chain per output limb),
//            BCONVU 2x6 MAC array src/Components.cpp:268-295.
//   K2 AUTO  InsGen::GenAUTO src/InsGen.cpp:46-71, AUTOU src/Components.cpp:173-194.
#pragma once
#include <cstddef>
#include "../../include/homulator_hip.h"   // HM_TENSOR_DOT_MAX_TERMS
#include "hm_modarith.h"
#include "hm_ntt_core.h"

enum HmEweOp {
  HM_EWE_MUL = 0,        // out = a*b
  HM_EWE_MAC2 = 1,       // out = a*b + c*d
  HM_EWE_MAC_ADD = 2,    // out = a*b + c
  HM_EWE_ADD = 3,        // out = a + c
  HM_EWE_SUB = 4,        // out = a - c
  HM_EWE_MUL_CONST = 5,  // out = a*k
  HM_EWE_SUB_SCALE = 6,  // out = (a - c)*k
  HM_EWE_COPY = 7,       // out = a
  HM_EWE_SUB_SCALE_ADD = 8,  // out = (a - c)*k + d   (ModDown finish fused with the final add)
  HM_EWE_ADD_CONST = 9,  // out = a + k         (a constant polynomial added to evaluation-form entries; k.w holds the residue on both back-ends)
  HM_EWE_NOPS
};

struct HmEweLimb {
  uint16_t a, b, c, d, out, mod;
};
struct HmEweArgs {
  const uint64_t *a, *b, *c, *d;
  uint64_t *out;
  const HmMod *mods;
  uint32_t logN, n_limbs, op;
  HmEweLimb limb[HM_MAX_LIMBS];
  HmTw k[HM_MAX_LIMBS];  // per-limb constant (Shoup form) for *_CONST / *_SCALE
};

template <int OP>
HM_HD uint64_t hm_ewe_one(uint64_t a, uint64_t b, uint64_t c, uint64_t d, const HmTw &k, const HmMod &m) {
  switch (OP) {
  case HM_EWE_MUL: return hm_mulmod(a, b, m);
  case HM_EWE_MAC2: return hm_barrett((hm_u128)a * b + (hm_u128)c * d, m);
  case HM_EWE_MAC_ADD: return hm_addmod(hm_mulmod(a, b, m), c, m.q);
  case HM_EWE_ADD: return hm_addmod(a, c, m.q);
  case HM_EWE_SUB: return hm_submod(a, c, m.q);
  case HM_EWE_MUL_CONST: return hm_shoup(a, k.w, k.ws, m.q);
  case HM_EWE_SUB_SCALE: return hm_shoup(a - c + m.q, k.w, k.ws, m.q);
  case HM_EWE_SUB_SCALE_ADD: return hm_addmod(hm_shoup(a - c + m.q, k.w, k.ws, m.q), d, m.q);
  case HM_EWE_ADD_CONST: return hm_addmod(a, k.w, m.q);
  default: return a;
  }
}

// operand usage per opcode (bit 0 = a, 1 = b, 2 = c, 3 = d)
HM_HD constexpr int hm_ewe_uses(int op) {
  return op == HM_EWE_MUL ? 3 : op == HM_EWE_MAC2 ? 15 : op == HM_EWE_MAC_ADD ? 7 :
         op == HM_EWE_ADD ? 5 : op == HM_EWE_SUB ? 5 : op == HM_EWE_MUL_CONST ? 1 :
         op == HM_EWE_SUB_SCALE ? 5 : op == HM_EWE_SUB_SCALE_ADD ? 13 : 1;   // (COPY, ADD_CONST: a)
}

// tensor product of two ciphertexts in one pass over the four inputs (TensorCompute::computeD0/D1/D2,
// src/Operation.cpp:624-739): d0 = a*b, d1 = a*d + c*b, d2 = c*d with a = c00, b = c10, c = c01, d = c11
struct HmTensorLimb {
  uint16_t a, b, c, d, o0, o1, o2, mod;
};
struct HmTensorArgs {
  const uint64_t *a, *b, *c, *d;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  uint32_t logN, n_limbs;
  HmTensorLimb limb[HM_MAX_LIMBS];
};
// Round 4: on the word-wise Montgomery product (hm_mont_acc, q = h 2^32 + 1).  b and d are taken to Montgomery form once (a product
// with 2^128 mod q: b 2^64 mod q + {0, q}, below 1.5q + 2^28), then the four products are exact: x wt 2^-64 with wt = b 2^64 is x b.  Six
// products of 11 instructions + four subtractions where three Barrett reductions of full 128-bit products took about twice as many.
// A product with an operand below q and a constant below 1.5q + 2^28 comes out below 1.1q + 1.
HM_HD void hm_tensor_one(uint64_t a, uint64_t b, uint64_t c, uint64_t d, const HmMod &m, uint64_t &d0, uint64_t &d1, uint64_t &d2) {
#if HM_GENERIC
  d0 = hm_mulmod(a, b, m);   // generic: three Barrett reductions of full 128-bit products
  d1 = hm_barrett((hm_u128)a * d + (hm_u128)c * b, m);
  d2 = hm_mulmod(c, d, m);
#else
  const HmBflyMod bm = hm_bfly_mod(m.q);
  const uint64_t bt = hm_mont_acc(0, b, m.r128, bm), dt = hm_mont_acc(0, d, m.r128, bm);
  d0 = hm_csub_neg(hm_mont_acc(0, a, bt, bm), bm.nq);
  d2 = hm_csub_neg(hm_mont_acc(0, c, dt, bm), bm.nq);
  d1 = hm_mont_acc(hm_mont_acc(0, a, dt, bm), c, bt, bm);   // below 2.2q + 2
  d1 = hm_csub_neg(hm_csub_neg(d1, bm.nq2), bm.nq);
#endif
}

// (K5, the inner product with the evaluation key: hm_ip_core.h)

// ---- K4 base conversion: out[t][x] = sum_i in[i][x] * table[i][t] mod q_t (device table: hm_bconv_entry form)
// One launch carries up to HM_BCONV_MAX_PROB independent conversions (the beta digits of a ModUp, the two
// keys of a ModDown): grid = (N / (HM_BCONV_THREADS * HM_BCONV_CPT), output chunks, problems); two adjacent
// coefficients per thread (16-byte accesses; every scalar operand feeds two multiply-adds).
#define HM_BCONV_MAX_IN 32   // parameter set A converts from a 28-limb basis (alpha = 28)
#define HM_BCONV_MAX_OUT 64
#define HM_BCONV_MAX_PROB 256  // problems per launch (blockIdx.z); the records live in a device table cached by content
#ifndef HM_BCONV_CHUNK
#define HM_BCONV_CHUNK 8    // output limbs per block when the launch is small (hm_bconv_batch raises it for big ones)
#endif
#define HM_BCONV_THREADS 256
#ifndef HM_BCONV_CPT
#define HM_BCONV_CPT 2       // coefficients per thread
#endif
struct HmBconvProb {
  const uint64_t *in;
  uint64_t *out;
  const uint64_t *table;  // device, [n_out][HM_BCONV_ROW(n_in)], entries in hm_bconv_entry form, rows zero-padded
  const uint64_t *qn;     // device, [n_out] x {q, -q^-1 mod 2^64} of the output moduli (HmQn)
  uint32_t n_in, n_out;
  // 32-bit entries: indexed by the (wave-uniform) output counter, they must be scalar loads from the kernarg
  // segment; 16-bit entries made hipcc emit a VECTOR load per output, and the modulus record load that depends on it
  // was a second serialised global-memory round trip per output (the kernel was latency-bound on these two loads)
  uint32_t in_limb[HM_BCONV_MAX_IN];
  uint32_t out_limb[HM_BCONV_MAX_OUT];
  // optional epilogue (ep_a != nullptr): out_t = (ep_a[ep_a_limb[t]] - conv_t) * ep_k[t] [+ ep_b[ep_b_limb[t]]]
  const uint64_t *ep_a, *ep_b;
  const HmTw *ep_k;                      // device, [n_out]
  uint32_t ep_a_limb[HM_BCONV_MAX_OUT], ep_b_limb[HM_BCONV_MAX_OUT];
  uint32_t in_packed;                    // the inputs are stored in the split-30 packed form (hm_pack30)
};
struct HmBconvArgs {
  const HmBconvProb *prob;  // device, [n_prob]: read with scalar loads (wave-uniform index)
  uint32_t logN, n_prob;
  uint32_t chunk;           // output limbs per block (the host trades input re-reads against blocks in flight)
};
// ---- the records of the base conversion fused into the first pass of the transform that consumes it (kernels: hm_bcol.h)
#define HM_BCOL_ONE_GROUP 15    // up to here every input of an access unit is held at once (16: hipcc leaves the arrays in scratch, 1 KB per lane)
struct HmBcolProb {
  const uint64_t *in;
  const uint64_t *table, *qn;
  uint32_t n_in, n_out;
  uint32_t in_limb[HM_BCONV_MAX_IN];
  uint32_t out_limb[HM_BCONV_MAX_OUT];   // where the hand-off of output o goes (limb of `out`)
  uint32_t out_mod[HM_BCONV_MAX_OUT];    // its modulus id (shared twiddles)
  uint32_t mix_limb[HM_BCONV_MAX_OUT];   // MIX: the operand added to output o before the transform (limb of HmBcolArgs::mix), constant in mixk
  const HmTw *mixk;                      // MIX: device, [n_out]
  uint32_t in_packed;                    // the inputs are stored in the split-30 packed form (hm_pack30): no shift / mask per input and workgroup
  // round 6 (scalar-register diet): ONE buffer descriptor for all inputs of a conversion — base = the lowest input limb-poly, input i at
  // byte offset in_off[i] from it (a scalar operand of the load).  A descriptor per input (four scalar registers each: 60 for a 15-limb
  // digit, 112 for 28) was hoisted out of the unit loop together with the table rows and spilled into vector-register lanes: 390
  // v_readlane / v_writelane in 5 531 vector instructions of k_bconv_col2<15>, 1 444 in 9 045 of k_bconv_col2<28>.  The host checks that
  // the inputs of a conversion lie within 4 GiB of each other (the digits of a plan are neighbours in the pool); a conversion whose inputs
  // are further apart runs as conversion + first pass (bconv_col_launch).
  const uint64_t *in_base;
  uint32_t in_off[HM_BCONV_MAX_IN];
};
struct HmBcolArgs {
  const HmBcolProb *prob;   // device
  uint64_t *out;
  const HmW *tw;
  uint32_t logN, n_prob, max_out;   // max_out: output GROUPS (of NOUT limbs) per (conversion, tile)
  const uint64_t *mix;
  uint32_t tile0, logTiles;         // the column tiles this launch works on: [tile0, tile0 + 2^logTiles) (all of them, or a rank's column slice)
};
// The block-to-work map of the fused launch, one half of a contract with the host's grid (hm_bcol_plan, hm_bconv_plan.h: grid = max_out *
// 8 * ceil(n_prob * tiles / 8)): blocks b, b + 8 share an XCD; inside an XCD: (conversion, tile) pairs, each with its max_out output groups
// in consecutive slots.  pi >= n_prob (the padding of the pairs to a multiple of 8) and og * NOUT >= n_out (a conversion with fewer
// outputs than the launch's widest) are the kernel's two early returns.
struct HmBcolBlock {
  uint32_t pi, tile, og;   // conversion, column tile, output group
};
HM_HD HmBcolBlock hm_bcol_block(uint32_t b, uint32_t max_out, uint32_t tile0, uint32_t logTiles) {
  const uint32_t xcd = b & 7u, slot = b >> 3;
  // (the division runs on the vector unit: its results are made scalar again by hand, or every buffer access of the kernel becomes a waterfall loop)
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t sdiv = __builtin_amdgcn_readfirstlane(slot / max_out);
#else
  const uint32_t sdiv = slot / max_out;
#endif
  const uint32_t pair = sdiv * 8u + xcd;
  return HmBcolBlock{pair >> logTiles, tile0 + (pair & ((1u << logTiles) - 1u)), slot - sdiv * max_out};
}
// (the records are read by compiled kernels through scalar loads at fixed offsets: the layouts are pinned)
static_assert(sizeof(HmBconvProb) == 968 && offsetof(HmBconvProb, table) == 16 && offsetof(HmBconvProb, in_limb) == 40 && offsetof(HmBconvProb, out_limb) == 168,
              "HmBconvProb: layout");
static_assert(sizeof(HmBcolProb) == 1080 && offsetof(HmBcolProb, table) == 8 && offsetof(HmBcolProb, in_limb) == 32 && offsetof(HmBcolProb, out_limb) == 160 &&
              offsetof(HmBcolProb, in_base) == 944 && offsetof(HmBcolProb, in_off) == 952, "HmBcolProb: layout");
#if defined(__HIP_DEVICE_COMPILE__)
typedef const HmBconvProb __attribute__((address_space(4))) *HmConstProb;
#define HM_CONST_PROB(p) ((HmConstProb)(uintptr_t)(p))
#define HM_CONST_PROB_T(T, p) ((const T __attribute__((address_space(4))) *)(uintptr_t)(p))
#else
#define HM_CONST_PROB_T(T, p) ((const T *)(p))
typedef const HmBconvProb *HmConstProb;
#define HM_CONST_PROB(p) (p)
#endif

// Split-30 MAC: operands are below 2^60, so y = y1 2^30 + y0 and w = w1 2^30 + w0 with 30-bit halves; each
// of the four partial-product columns y_a w_b stays below 2^64 over 16 terms, so a MAC is four
// v_mad_u64_u32 into plain 64-bit accumulators with no carry chain; the columns are recombined once per
// output.  Device table entries are pre-split: low word = w0, high word = w1 (hm_bconv_pack).
HM_HD uint64_t hm_bconv_pack(uint64_t w) { return (w & 0x3FFFFFFFull) | ((w >> 30) << 32); }
// device form of a conversion factor w for output modulus m: Montgomery form (the accumulator is reduced by
// hm_redc_wide, which divides by 2^64), split-30 packed
HM_HD uint64_t hm_bconv_entry(uint64_t w, const HmMod &m) { return hm_bconv_pack(hm_mulmod(w, m.r64, m)); }

#if defined(__HIP_DEVICE_COMPILE__)
typedef const HmMod __attribute__((address_space(4))) *HmConstMod;
#define HM_CONST_MODS(p) ((HmConstMod)(uintptr_t)(p))
#else
typedef const HmMod *HmConstMod;
#define HM_CONST_MODS(p) (p)
#endif

// Sum of T tensor products in one pass over the 4T inputs (hm_tensor_dot; HDOT):
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
  const uint32_t *rec;   // device, [n_limbs][HM_DOT_REC_WORDS(n_terms)]: read through the scalar cache (wave-uniform index)
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's limb lists (a .. d: [n][T], o0 .. o2: [n]; a null list is the identity).  Host side.
inline void hm_tensor_dot_fill_recs(uint32_t *rec, const uint32_t *la, const uint32_t *lb, const uint32_t *lc, const uint32_t *ld, const uint32_t *l0,
                                    const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids, uint32_t n, uint32_t T) {
  auto at = [](const uint32_t *l, uint32_t i) { return l ? l[i] : i; };
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_DOT_REC_WORDS(T);
    r[0] = mod_ids[i]; r[1] = at(l0, i); r[2] = at(l1, i); r[3] = at(l2, i);
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      r[4 + 4 * t] = at(la, e); r[5 + 4 * t] = at(lb, e); r[6 + 4 * t] = at(lc, e); r[7 + 4 * t] = at(ld, e);
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
// hipcc sinks loads to their first use; this keeps what was issued above it above the arithmetic below it (no instruction is emitted)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HM_ABL_DOT_NOPIN)   // (timing-only ablation: the loads where hipcc puts them)
#define HM_DOT_ISSUED() __builtin_amdgcn_sched_barrier(0)
#else
#define HM_DOT_ISSUED() ((void)0)
#endif
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
// thread tid of the workgroup that owns chunk `chunk` (512 coefficients) of record `entry`: the pair at chunk * 512 + 2 tid.  T is a run-time
// loop, two pairs per round in two named register sets (no copy between them): the four loads of pair t + 1 are issued before the products of
// pair t are formed, and the record words of a pair are requested a step before its loads (index clamped to the last pair: always inside the record).
HM_HD void hm_tensor_dot_thread(const HmTensorDotArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = (chunk * 512u + 2u * tid) << 3;
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_DOT_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  HmDotAcc s[2] = {{0, 0, 0}, {0, 0, 0}};
  HmDotPair p0 = hm_tensor_dot_ld(g, hm_tensor_dot_limbs(rec, 0), N, lane_bytes), p1;
  HmDotLimbs l = hm_tensor_dot_limbs(rec, T > 1 ? 1u : 0u);
  uint32_t t = 1;
#pragma unroll 1
  for (; t + 1 < T; t += 2) {
    p1 = hm_tensor_dot_ld(g, l, N, lane_bytes);                  // pair t
    l = hm_tensor_dot_limbs(rec, t + 1);
    HM_DOT_ISSUED();
    hm_tensor_dot_acc2(s, p0);
    p0 = hm_tensor_dot_ld(g, l, N, lane_bytes);                  // pair t + 1
    l = hm_tensor_dot_limbs(rec, t + 2 < T ? t + 2 : T - 1);
    HM_DOT_ISSUED();
    hm_tensor_dot_acc2(s, p1);
  }
  if (t < T) {   // (wave-uniform) an even number of pairs: one more behind the rounds
    p1 = hm_tensor_dot_ld(g, l, N, lane_bytes);
    HM_DOT_ISSUED();
    hm_tensor_dot_acc2(s, p0);
    hm_tensor_dot_acc2(s, p1);
  } else {
    hm_tensor_dot_acc2(s, p0);
  }
  hm_bst2(g.o0 + rec[1] * N, lane_bytes, hm_barrett_wide(s[0].d0, m), hm_barrett_wide(s[1].d0, m));
  hm_bst2(g.o1 + rec[2] * N, lane_bytes, hm_barrett_wide(s[0].d1, m), hm_barrett_wide(s[1].d1, m));
  hm_bst2(g.o2 + rec[3] * N, lane_bytes, hm_barrett_wide(s[0].d2, m), hm_barrett_wide(s[1].d2, m));
}

// Scaled square of ONE ciphertext plus a constant, in one pass over its two polynomials (hm_tensor_square; HSQUARE):
//   d0 = s a a + k,  d1 = 2 s a c,  d2 = s c c      with a = c0, c = c1, s in [1, q) and k in [0, q) per entry, every residue canonical.
// The tensor product of a ciphertext with itself needs two loads and five products where hm_tensor_one, fed the same operands twice, takes
// four and six; the scalar and the constant are linear and act in front of the key switch, so they are applied here, in registers.
// A record = 64 bytes (a multiple of 16), read through the scalar cache (wave-uniform index).  The per-entry constants are stored in the form
// the arithmetic takes (hm_tensor_square_fill_recs).  mont32: scale = s 2^128 mod q, which takes the place of m.r128 in the step to Montgomery
// form, so that the scalar costs no product at all.  generic: scale = s with its Shoup companion scale_s = floor(s 2^64 / q): a and c are
// multiplied by s once, by two Shoup products, in front of the three Barrett products.  addend = k on both.
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
// The records of n entries from the entry point's limb lists (a null list is the identity) and constants (scale null: 1, addend null: 0; both
// already checked: reduced, scale != 0); q[i] = the modulus of entry i.  Host side.
inline void hm_tensor_square_fill_recs(HmTensorSqRec *rec, const uint32_t *la, const uint32_t *lc, const uint32_t *l0, const uint32_t *l1, const uint32_t *l2,
                                       const uint32_t *mod_ids, const uint64_t *q, uint32_t n, const uint64_t *scale, const uint64_t *addend) {
  auto at = [](const uint32_t *l, uint32_t i) { return l ? l[i] : i; };
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t s = scale ? scale[i] : 1;
    rec[i] = HmTensorSqRec{mod_ids[i], at(la, i), at(lc, i), at(l0, i), at(l1, i), at(l2, i), s != 1 ? 1u : 0u, 0u, hm_tensor_square_scale(s, q[i]),
                           HM_GENERIC ? hm_shoup_companion(s, q[i]) : 0, addend ? addend[i] : 0, 0};
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
// thread tid of the workgroup that owns chunk `chunk` (512 coefficients) of record `entry`: two 16-byte loads, three 16-byte stores
HM_HD void hm_tensor_square_thread(const HmTensorSqArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t lane_bytes = (chunk * 512u + 2u * tid) << 3;
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

// Sum of T scaled polynomials plus a constant in one pass over the T inputs (hm_lincomb; HLINCOMB):
//   out = sum_t s_t x_t + k      with s_t, k in [0, q) per record and every x_t canonical.
// The raw 64 x 64 products are summed in ONE 128-bit accumulator per coefficient, k is added, and the accumulator is reduced once, as
// hm_tensor_dot_acc does: T <= HM_LINCOMB_MAX_TERMS = 16 products below 2^120 are below 2^124, plus k < 2^60 below 2^125, and hm_barrett_wide
// takes any 128-bit value.  The result is the canonical residue of the exact integer sum, hence bit-identical to the chain of MUL_CONST, ADD
// and ADD_CONST.  One form on both arithmetic back-ends: T + 1 limb-polys per record and one wide multiply per loaded word.
static_assert(HM_LINCOMB_MAX_TERMS == 16, "the accumulator: 16 products below 2^120 plus k below 2^60 stay below 2^125");
// a record = HM_LINCOMB_REC_WORDS(T) 32-bit words, a multiple of 16 bytes: (modulus id, output limb, T, 0), (k: 2 words, 0, 0), then per term
// (input limb, 0, s_t: 2 words).  The 64-bit values sit at 8-byte offsets.
#define HM_LINCOMB_REC_WORDS(T) (8u + 4u * (T))
struct HmLincombArgs {
  const uint64_t *in;
  uint64_t *out;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_LINCOMB_REC_WORDS(n_terms)]: read through the scalar cache (wave-uniform index)
  uint32_t logN, n_limbs, n_terms;
};
// The records of n entries from the entry point's lists (in: [n][T], out: [n]; a null list is the identity) and constants (scale: [n][T];
// addend: [n] or null = 0; both already checked: reduced).  Host side.
inline void hm_lincomb_fill_recs(uint32_t *rec, const uint32_t *li, const uint32_t *lo, const uint32_t *mod_ids, uint32_t n, uint32_t T,
                                 const uint64_t *scale, const uint64_t *addend) {
  auto at = [](const uint32_t *l, uint32_t i) { return l ? l[i] : i; };
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_LINCOMB_REC_WORDS(T);
    const uint64_t k = addend ? addend[i] : 0;
    r[0] = mod_ids[i]; r[1] = at(lo, i); r[2] = T; r[3] = 0;
    r[4] = (uint32_t)k; r[5] = (uint32_t)(k >> 32); r[6] = 0; r[7] = 0;
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t e = i * T + t;
      r[8 + 4 * t] = at(li, e); r[9 + 4 * t] = 0; r[10 + 4 * t] = (uint32_t)scale[e]; r[11 + 4 * t] = (uint32_t)(scale[e] >> 32);
    }
  }
}
struct HmLincombTerm {   // the (input limb, scalar) of one term: four words of the record
  uint32_t limb;
  uint64_t s;
};
template <class REC>
HM_HD HmLincombTerm hm_lincomb_term(REC rec, uint32_t t) {
  return HmLincombTerm{rec[8 + 4 * t], (uint64_t)rec[10 + 4 * t] | ((uint64_t)rec[11 + 4 * t] << 32)};
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
// thread tid of the workgroup that owns chunk `chunk` (512 coefficients) of record `entry`: the pair at chunk * 512 + 2 tid, T 16-byte loads and
// one 16-byte store.  T is a run-time loop in hm_tensor_dot_thread's shape: two terms per round in two named register sets, the load of term
// t + 1 issued before the products of term t, the record words of a term requested a step before its load (index clamped to the last term:
// always inside the record).  An even T leaves one term behind the rounds, T = 1 runs no round at all.
HM_HD void hm_lincomb_thread(const HmLincombArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t T = g.n_terms, lane_bytes = (chunk * 512u + 2u * tid) << 3;
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_LINCOMB_REC_WORDS(T);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint64_t k = (uint64_t)rec[4] | ((uint64_t)rec[5] << 32);
  hm_u128 s[2] = {0, 0};
  HmLincombPair p0 = hm_lincomb_ld(g, hm_lincomb_term(rec, 0), N, lane_bytes), p1;
  HmLincombTerm l = hm_lincomb_term(rec, T > 1 ? 1u : 0u);
  uint32_t t = 1;
#pragma unroll 1
  for (; t + 1 < T; t += 2) {
    p1 = hm_lincomb_ld(g, l, N, lane_bytes);                     // term t
    l = hm_lincomb_term(rec, t + 1);
    HM_DOT_ISSUED();
    hm_lincomb_acc2(s, p0);
    p0 = hm_lincomb_ld(g, l, N, lane_bytes);                     // term t + 1
    l = hm_lincomb_term(rec, t + 2 < T ? t + 2 : T - 1);
    HM_DOT_ISSUED();
    hm_lincomb_acc2(s, p1);
  }
  if (t < T) {   // (wave-uniform) an even number of terms: one more behind the rounds
    p1 = hm_lincomb_ld(g, l, N, lane_bytes);
    HM_DOT_ISSUED();
    hm_lincomb_acc2(s, p0);
    hm_lincomb_acc2(s, p1);
  } else {
    hm_lincomb_acc2(s, p0);
  }
  hm_bst2(g.out + rec[1] * N, lane_bytes, hm_barrett_wide(s[0] + k, m), hm_barrett_wide(s[1] + k, m));
}

// Scaled tensor product of TWO ciphertexts plus a linear combination of A further ciphertexts plus a constant, in one pass over the 4 + 2A
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
// a record = HM_MULADD_REC_WORDS(A) 32-bit words, a multiple of 16 bytes, the 64-bit values at 8-byte offsets:
//   0: modulus id   1..4: the limbs of a, b, c, d   5..7: the limbs of d0, d1, d2   8: A   9: s != 1
//   10, 11: s   12, 13: its Shoup companion floor(s 2^64 / q)   14, 15: k
// then per addend (limb of x_t, limb of y_t, u_t: 2 words)
#define HM_MULADD_REC_HEAD 16u
#define HM_MULADD_REC_WORDS(A) (HM_MULADD_REC_HEAD + 4u * (A))
struct HmTensorMulAddArgs {
  const uint64_t *a, *b, *c, *d, *x;
  uint64_t *o0, *o1, *o2;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_MULADD_REC_WORDS(n_addends)]: read through the scalar cache (wave-uniform index)
  uint32_t logN, n_limbs, n_addends;
};
// The records of n entries from the entry point's limb lists (a .. d, o0 .. o2: [n], a null list is the identity; lx0, lx1: [n][A]) and
// constants (scale: [n] or null = 1; add_scale: [n][A]; addend: [n] or null = 0; all already checked: reduced, scale != 0); q[i] = the modulus
// of entry i.  Host side.
inline void hm_tensor_muladd_fill_recs(uint32_t *rec, const uint32_t *la, const uint32_t *lb, const uint32_t *lc, const uint32_t *ld, const uint32_t *lx0,
                                       const uint32_t *lx1, const uint32_t *l0, const uint32_t *l1, const uint32_t *l2, const uint32_t *mod_ids,
                                       const uint64_t *q, uint32_t n, uint32_t A, const uint64_t *scale, const uint64_t *add_scale, const uint64_t *addend) {
  auto at = [](const uint32_t *l, uint32_t i) { return l ? l[i] : i; };
  auto put64 = [](uint32_t *r, uint64_t v) { r[0] = (uint32_t)v; r[1] = (uint32_t)(v >> 32); };
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_MULADD_REC_WORDS(A);
    const uint64_t s = scale ? scale[i] : 1;
    r[0] = mod_ids[i]; r[1] = at(la, i); r[2] = at(lb, i); r[3] = at(lc, i); r[4] = at(ld, i);
    r[5] = at(l0, i); r[6] = at(l1, i); r[7] = at(l2, i); r[8] = A; r[9] = s != 1 ? 1u : 0u;
    put64(r + 10, s); put64(r + 12, hm_shoup_companion(s, q[i])); put64(r + 14, addend ? addend[i] : 0);
    for (uint32_t t = 0; t < A; ++t) {
      const uint32_t e = i * A + t;
      uint32_t *w = r + HM_MULADD_REC_HEAD + 4 * t;
      w[0] = lx0[e]; w[1] = lx1[e]; put64(w + 2, add_scale[e]);
    }
  }
}
template <class REC>
HM_HD uint64_t hm_muladd_rec64(REC rec, uint32_t w) { return (uint64_t)rec[w] | ((uint64_t)rec[w + 1] << 32); }
struct HmMulAddTerm {   // the (limb of x_t, limb of y_t, scalar) of one addend: four words of the record
  uint32_t x, y;
  uint64_t u;
};
// the words of addend t; the caller clamps t to the last addend, and a record without addends hands out words of its header instead (never used):
// always inside the record
template <class REC>
HM_HD HmMulAddTerm hm_muladd_term(REC rec, uint32_t A, uint32_t t) {
  const uint32_t w = A ? HM_MULADD_REC_HEAD + 4 * t : HM_MULADD_REC_HEAD - 4;
  return HmMulAddTerm{rec[w], rec[w + 1], hm_muladd_rec64(rec, w + 2)};
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
// thread tid of the workgroup that owns chunk `chunk` (512 coefficients) of record `entry`: the pair at chunk * 512 + 2 tid, four 16-byte loads
// for the product, two per addend, three 16-byte stores.  A is a run-time loop in hm_lincomb_thread's shape with the product in the place of
// its first term: the loads of addend 1 are issued before the products of the tensor product are formed, then two addends per round in two
// named register sets, the loads of addend t + 1 issued before the products of addend t, the record words of an addend requested a step
// before its loads (hm_muladd_term: always inside the record).  A = 0 and A = 1 run no round; one addend is left behind the rounds.
HM_HD void hm_tensor_muladd_thread(const HmTensorMulAddArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t A = g.n_addends, lane_bytes = (chunk * 512u + 2u * tid) << 3;
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_MULADD_REC_WORDS(A);
  const HmMod m = HM_CONST_MODS(g.mods)[rec[0]];
  const uint32_t scaled = rec[9];
  const uint64_t scale = hm_muladd_rec64(rec, 10), scale_s = hm_muladd_rec64(rec, 12), k = hm_muladd_rec64(rec, 14);
  HmDotPair v;
  hm_bld2(g.a + rec[1] * N, lane_bytes, v.a[0], v.a[1]);
  hm_bld2(g.b + rec[2] * N, lane_bytes, v.b[0], v.b[1]);
  hm_bld2(g.c + rec[3] * N, lane_bytes, v.c[0], v.c[1]);
  hm_bld2(g.d + rec[4] * N, lane_bytes, v.d[0], v.d[1]);
  HmMulAddTerm l = hm_muladd_term(rec, A, 0);
  HmMulAddPair p0, p1;
  uint32_t t = 0;
  if (A > 0) {   // (wave-uniform) addend 1 under the product
    p0 = hm_muladd_ld(g, l, N, lane_bytes);
    l = hm_muladd_term(rec, A, A > 1 ? 1u : 0u);
    t = 1;
  }
  HM_DOT_ISSUED();
  HmDotAcc s[2];
  hm_muladd_product(s[0], v.a[0], v.b[0], v.c[0], v.d[0], scale, scale_s, scaled, k, m);
  hm_muladd_product(s[1], v.a[1], v.b[1], v.c[1], v.d[1], scale, scale_s, scaled, k, m);
#pragma unroll 1
  for (; t + 1 < A; t += 2) {
    p1 = hm_muladd_ld(g, l, N, lane_bytes);                      // addend t + 1
    l = hm_muladd_term(rec, A, t + 1);
    HM_DOT_ISSUED();
    hm_muladd_acc2(s, p0);
    p0 = hm_muladd_ld(g, l, N, lane_bytes);                      // addend t + 2
    l = hm_muladd_term(rec, A, t + 2 < A ? t + 2 : A - 1);
    HM_DOT_ISSUED();
    hm_muladd_acc2(s, p1);
  }
  if (t < A) {   // (wave-uniform) an even number of addends: one more behind the rounds
    p1 = hm_muladd_ld(g, l, N, lane_bytes);
    HM_DOT_ISSUED();
    hm_muladd_acc2(s, p0);
    hm_muladd_acc2(s, p1);
  } else if (A > 0) {
    hm_muladd_acc2(s, p0);
  }
  hm_bst2(g.o0 + rec[5] * N, lane_bytes, hm_barrett_wide(s[0].d0, m), hm_barrett_wide(s[1].d0, m));
  hm_bst2(g.o1 + rec[6] * N, lane_bytes, hm_barrett_wide(s[0].d1, m), hm_barrett_wide(s[1].d1, m));
  hm_bst2(g.o2 + rec[7] * N, lane_bytes, hm_barrett_wide(s[0].d2, m), hm_barrett_wide(s[1].d2, m));
}

// Real and imaginary parts of the slots from a polynomial x and its conjugate y in one pass over both (hm_reim_split; HREIM):
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
// a record = HM_REIM_REC_WORDS 32-bit words (48 bytes, a multiple of 16), the 64-bit values at 8-byte offsets:
//   0: modulus id   1, 2: the limbs of x, y   3, 4: the limbs of re, im   5..7: 0   8, 9: w   10, 11: ws
#define HM_REIM_REC_WORDS 12u
struct HmReimArgs {
  const uint64_t *x, *y;
  uint64_t *o_re, *o_im;
  const HmMod *mods;
  const uint32_t *rec;   // device, [n_limbs][HM_REIM_REC_WORDS]: read through the scalar cache (wave-uniform index)
  uint32_t logN, n_limbs;
};
// The records of n entries from the entry point's limb lists (a null list is the identity); w[i] = -psi^(N/2) mod q[i], q[i] = the modulus of
// entry i.  Host side.
inline void hm_reim_fill_recs(uint32_t *rec, const uint32_t *lx, const uint32_t *ly, const uint32_t *lre, const uint32_t *lim, const uint32_t *mod_ids,
                              const uint64_t *w, const uint64_t *q, uint32_t n) {
  auto at = [](const uint32_t *l, uint32_t i) { return l ? l[i] : i; };
  auto put64 = [](uint32_t *r, uint64_t v) { r[0] = (uint32_t)v; r[1] = (uint32_t)(v >> 32); };
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *r = rec + (size_t)i * HM_REIM_REC_WORDS;
    r[0] = mod_ids[i]; r[1] = at(lx, i); r[2] = at(ly, i); r[3] = at(lre, i); r[4] = at(lim, i); r[5] = r[6] = r[7] = 0;
    put64(r + 8, w[i]); put64(r + 10, hm_shoup_companion(w[i], q[i]));
  }
}
// thread tid of the workgroup that owns chunk `chunk` (512 coefficients) of record `entry`: the pair at chunk * 512 + 2 tid, two 16-byte loads and
// two 16-byte stores.  chunk < N / 512 (the launch has n N / 512 workgroups), so the last byte touched is N * 8 - 1 of each limb-poly.
HM_HD void hm_reim_thread(const HmReimArgs &g, uint32_t entry, uint32_t chunk, uint32_t tid) {
  const size_t N = (size_t)1 << g.logN;
  const uint32_t lane_bytes = (chunk * 512u + 2u * tid) << 3;
  const auto rec = HM_CONST_PROB_T(uint32_t, g.rec) + (size_t)entry * HM_REIM_REC_WORDS;
  const uint64_t q = HM_CONST_MODS(g.mods)[rec[0]].q;
  const uint64_t w = hm_muladd_rec64(rec, 8), ws = hm_muladd_rec64(rec, 10);
  const bool first = chunk < (uint32_t)(N >> 10);   // (workgroup-uniform) entries [0, N/2)
  const uint64_t u = first ? w : q - w, us = first ? ws : ~ws;
  uint64_t x[2], y[2];
  hm_bld2(g.x + rec[1] * N, lane_bytes, x[0], x[1]);
  hm_bld2(g.y + rec[2] * N, lane_bytes, y[0], y[1]);
  hm_bst2(g.o_re + rec[3] * N, lane_bytes, hm_addmod(x[0], y[0], q), hm_addmod(x[1], y[1], q));
  hm_bst2(g.o_im + rec[4] * N, lane_bytes, hm_shoup(hm_submod(x[0], y[0], q), u, us, q), hm_shoup(hm_submod(x[1], y[1], q), u, us, q));
}

// The conversion table is read through the SCALAR cache: every lane of a wave needs the same entries, so they are
// s_load'ed into SGPRs (asynchronously, no VGPRs, no LDS, no barrier) and feed v_mad_u64_u32 as scalar operands.
// hipcc only emits scalar loads for memory it knows to be constant, hence the constant-address-space view of the
// table pointer.  Device layout: [n_out][HM_BCONV_ROW(n_in)] entries (hm_bconv_entry form), a row = the factors of
// one output limb padded with zeros to a multiple of 8 entries, so that a row is fetched by 64-byte scalar loads
// (s_load_dwordx16) instead of one 8-byte load plus three address instructions per entry.
struct HmRow8 {
  uint64_t w[8];
};
#define HM_BCONV_ROW(n_in) ((((n_in) + 7u) / 8u) * 8u)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const HmRow8 __attribute__((address_space(4))) *HmConstRow8;
#define HM_CONST_ROWS(p) ((HmConstRow8)(uintptr_t)(p))
#else
typedef const HmRow8 *HmConstRow8;
#define HM_CONST_ROWS(p) ((const HmRow8 *)(p))
#endif

// one output limb of one coefficient: sum_i y_i w_i with the split-30 columns, Montgomery-reduced
template <int N_IN>
HM_HD uint64_t hm_bconv_dot(const uint32_t (&yl)[N_IN], const uint32_t (&yh)[N_IN], const HmRow8 (&row)[(N_IN + 7) / 8], uint64_t q, uint64_t nqinv) {
  hm_u128 acc = 0;
  constexpr int GROUPS = (N_IN + 15) / 16;  // 16 terms per carry-free column group (each column stays below 2^64)
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    uint64_t s00 = 0, s01 = 0, s10 = 0, s11 = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = g * 16 + j;
      if (i < N_IN) {
        const uint64_t w = row[i >> 3].w[i & 7];
        const uint32_t wl = (uint32_t)w, wh = (uint32_t)(w >> 32);
        s00 += (uint64_t)yl[i] * wl;
#if !defined(HM_ABL_BCONV_HALF)   // (timing-only ablation: half of the multiply-adds of a conversion)
        s01 += (uint64_t)yl[i] * wh;
        s10 += (uint64_t)yh[i] * wl;
#endif
        s11 += (uint64_t)yh[i] * wh;
      }
    }
    acc += (hm_u128)s00 + (((hm_u128)s01 + s10) << 30) + ((hm_u128)s11 << 60);   // 32 products of < 2^120: below 2^125
  }
  HmMod m;
  m.q = q;
  m.nqinv = nqinv;
  return hm_redc_wide<N_IN>(acc, m);
}

// the same sum for up to 16 consecutive inputs, NOT reduced: the carry-free split-30 columns of one group, recombined into a 128-bit value
// (round 6: the fused conversion + first pass takes digits of 16 .. 32 limbs in two such groups, each loaded, multiplied and dropped before
// the next one, so that at most 16 inputs x 2 coefficients x 2 halves = 64 VGPRs of inputs are live; hm_redc_wide<N_IN> reduces the sum of
// the groups).  row = the table entries of these inputs (a whole number of 8-entry groups: the chunk starts at a multiple of 8).
template <int CN>
HM_HD hm_u128 hm_bconv_cols(const uint32_t (&yl)[CN], const uint32_t (&yh)[CN], const HmRow8 (&row)[(CN + 7) / 8]) {
  static_assert(CN >= 1 && CN <= 16, "one carry-free column group");
  uint64_t s00 = 0, s01 = 0, s10 = 0, s11 = 0;
#pragma unroll
  for (int i = 0; i < CN; ++i) {
    const uint64_t w = row[i >> 3].w[i & 7];
    const uint32_t wl = (uint32_t)w, wh = (uint32_t)(w >> 32);
    s00 += (uint64_t)yl[i] * wl;
    s01 += (uint64_t)yl[i] * wh;
    s10 += (uint64_t)yh[i] * wl;
    s11 += (uint64_t)yh[i] * wh;
  }
  return (hm_u128)s00 + (((hm_u128)s01 + s10) << 30) + ((hm_u128)s11 << 60);
}

// per-output modulus constants, stored behind the table rows (HmBconvProb::qn): no load depends on another load
struct HmQn {
  uint64_t q, nqinv;
};
#if defined(__HIP_DEVICE_COMPILE__)
typedef const HmQn __attribute__((address_space(4))) *HmConstQn;
#define HM_CONST_QN(p) ((HmConstQn)(uintptr_t)(p))
#else
typedef const HmQn *HmConstQn;
#define HM_CONST_QN(p) ((const HmQn *)(p))
#endif

// CPT coefficients x, x+1, .. (CPT = 2: one 16-byte access per input / output limb) for outputs [t0, t1).  The inputs
// stay in registers for all outputs of the chunk; a row feeds 4 * N_IN * CPT multiply-adds as scalar operands.
// (Requesting the NEXT output's row ahead of the products changed nothing: hipcc sinks the loads to the end of the
// iteration, and the kernel is bound by VALU issue — per output and coefficient 4 * N_IN multiply-adds plus ~30
// instructions of column recombination and Montgomery reduction — not by the scalar-cache latency.)
// PACKED: the inputs are stored in the split-30 packed form (hm_pack30): the halves are taken as they are (a template parameter: chosen per
// value at run time the select costs what the packed form saves)
template <int N_IN, int CPT, bool PACKED = false, class PROB>
HM_HD void hm_bconv_thread(const PROB &p, uint32_t logN, uint32_t x, uint32_t t0, uint32_t t1) {
  const size_t N = (size_t)1 << logN;
  constexpr int NG = (N_IN + 7) / 8;  // 8-entry groups per row
  HmConstRow8 tab = HM_CONST_ROWS(p.table);
  HmConstQn qn = HM_CONST_QN(p.qn);
  uint32_t yl[CPT][N_IN], yh[CPT][N_IN];
#pragma unroll
  for (int i = 0; i < N_IN; ++i) {
    uint64_t v[2] = {0, 0};
    // uniform limb base + one lane offset: all N_IN loads issue back to back (with a 64-bit address per load hipcc
    // recycled the registers of loaded data for the next addresses and serialised the loads pairwise)
    if (CPT == 2) hm_bld2(p.in + (size_t)p.in_limb[i] * N, x << 3, v[0], v[1]);
    else v[0] = p.in[(size_t)p.in_limb[i] * N + x];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      if (PACKED) { yl[c][i] = (uint32_t)v[c]; yh[c][i] = (uint32_t)(v[c] >> 32); }
      else { yl[c][i] = (uint32_t)v[c] & 0x3FFFFFFFu; yh[c][i] = (uint32_t)(v[c] >> 30); }
    }
  }
  for (uint32_t t = t0; t < t1; ++t) {
    HmRow8 row[NG];
#if defined(HM_ABL_BCONV_NOTAB)   // timing-only ablation: one table row for every output (no per-output scalar loads)
    const HmQn m = qn[t0];
#pragma unroll
    for (int g = 0; g < NG; ++g) row[g] = tab[t0 * NG + g];
#else
    const HmQn m = qn[t];
#pragma unroll
    for (int g = 0; g < NG; ++g) row[g] = tab[t * NG + g];
#endif
    uint64_t r[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < CPT; ++c) r[c] = hm_bconv_dot<N_IN>(yl[c], yh[c], row, m.q, m.nqinv);
    if (p.ep_a) {   // (wave-uniform) out = (a - conv) * k [+ b]
#if defined(__HIP_DEVICE_COMPILE__)
      typedef const HmTw __attribute__((address_space(4))) *ConstTw;
      const HmTw k = {((ConstTw)(uintptr_t)p.ep_k)[t].w, ((ConstTw)(uintptr_t)p.ep_k)[t].ws};
#else
      const HmTw k = p.ep_k[t];
#endif
      uint64_t av[2] = {0, 0}, bv[2] = {0, 0};
      if (CPT == 2) hm_bld2(p.ep_a + (size_t)p.ep_a_limb[t] * N, x << 3, av[0], av[1]);
      else av[0] = p.ep_a[(size_t)p.ep_a_limb[t] * N + x];
      if (p.ep_b) {
        if (CPT == 2) hm_bld2(p.ep_b + (size_t)p.ep_b_limb[t] * N, x << 3, bv[0], bv[1]);
        else bv[0] = p.ep_b[(size_t)p.ep_b_limb[t] * N + x];
      }
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        r[c] = hm_shoup(av[c] + m.q - r[c], k.w, k.ws, m.q);
        if (p.ep_b) r[c] = hm_addmod(r[c], bv[c], m.q);
      }
    }
    if (CPT == 2) hm_bst2(p.out + (size_t)p.out_limb[t] * N, x << 3, r[0], r[1]);
    else p.out[(size_t)p.out_limb[t] * N + x] = r[0];
  }
}

// (K2, the automorphism's index map hm_auto_src: hm_ntt_core.h — the transforms gather through it as well)

// ---- deterministic synthetic data (same definition as oracle/homoracle.c ho_fill_uniform)
HM_HD uint64_t hm_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
HM_HD uint64_t hm_synth(uint64_t stream, uint32_t x, uint64_t q) {
  uint64_t z = hm_mix64(stream * 0xD1342543DE82EF95ull + (uint64_t)x * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull);
  return hm_mulhi(z, q);
}
