// hm_slot_core.h — the canonical embedding of CKKS: slot vectors <-> coefficient vectors (hm_encode / hm_decode).
// Per-thread bodies (no cross-thread state) shared by the HIP kernel k_slot_fft and the host emulator (tests/emu/hm_emu_slots.cpp).
//
// N = ring degree, n = N / 2 slots, zeta = exp(i pi / N), e_j = 5^j mod 2N.  With u_k = m_k + i m_{k+n} (k < n):
//     decode (forward)   z_j = sum_{k<n} u_k zeta^{e_j k}
//     encode (inverse)   u_k = (1/n) sum_j z_j zeta^{-e_j k}
// zeta^{e_j} are the n roots of X^n = i, and (zeta^{e_j})^2 depends on j mod n/2 only, so the radix-2 network of a plain FFT serves with the
// twiddle of stage LEN at position J < LEN/2 read from the root table at (e_J mod 4 LEN) * (n / LEN): the slot order costs index arithmetic
// on the table and no permutation of the data.  Forward: bit-reversed input, stages LEN = 2 .. n; inverse: stages LEN = n .. 2 with the
// conjugate twiddles, bit-reversed output.
//
// Two passes over n = n1 * n2 (n2 = 2^log2 the contiguous, low stages; n1 = 2^log1 the strided, high stages), each workgroup transforming a
// tile of HM_SLOT_T elements in LDS:
//     HIGH  tile = all n1 rows r of W = T / n1 adjacent columns c: element c + n2 r; stages LEN = n2 l, l = 2 .. n1
//     LOW   tile = W2 = T / n2 blocks B of n2 contiguous elements; stages LEN = 2 .. n2.  The blocks of a tile are the ones whose
//           bit-reversed numbers are adjacent, so the coefficient side of the pass (k = bitrev(t) n1 + bitrev(B)) is contiguous in runs of W2.
// Every floating-point operation that fuses is an explicit __builtin_fma; all others are compiled with contraction off, so the host compiler
// gives the bits the GPU gives.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cmath>
#include <vector>
#include "hm_modarith.h"

#define HM_SLOT_TL 11
#define HM_SLOT_T (1u << HM_SLOT_TL)           // elements of a tile
#define HM_SLOT_THREADS 256u
#define HM_SLOT_LDS (HM_SLOT_T + (HM_SLOT_T >> 6))   // LOW tiles pad one element per block (the narrowest block is 64 elements)
#define HM_SLOT_MIN_LOGN 12u                   // N = 2^13
#define HM_SLOT_MAX_LOGN 16u                   // N = 2^17
#define HM_SLOT_FP_STRICT _Pragma("clang fp contract(off)")

struct alignas(16) HmC {
  double re, im;
};
struct alignas(16) HmU2 {
  uint64_t x, y;
};

// n = 2^logn = 2^log1 * 2^log2; both at most 8, so both fit a tile
HM_HD uint32_t hm_slot_log2(uint32_t logn) { return (logn + 1) / 2; }
HM_HD uint32_t hm_slot_log1(uint32_t logn) { return logn - hm_slot_log2(logn); }

struct HmSlotArgs {
  const HmC *roots;        // [4n]: (cos, sin)(pi k / N)
  const uint32_t *rot;     // [n]: 5^j mod 2N
  const HmC *zin;          // [n_vec][n]: the side of a pass that is read in tile order
  HmC *zout;               // [n_vec][n]: ... written in tile order
  uint64_t *coef;          // the coefficient side of the LOW pass: limb-poly limbs[v] of this buffer
  const uint32_t *limbs;   // [n_vec]
  uint32_t *flag;          // encode: set to 1 by any coefficient beyond (q - 1) / 2
  double mul;              // encode: Delta * 2 / N; decode: 1 / Delta
  uint64_t q, half;        // encode: the source modulus; decode: the limb's modulus; half = (q - 1) / 2
  uint32_t logn, log1, log2, tiles;   // tiles = n / T per vector
};

HM_HD uint32_t hm_slot_bitrev(uint32_t x, uint32_t bits) {
  x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
  x = ((x & 0x33333333u) << 2) | ((x >> 2) & 0x33333333u);
  x = ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu);
  x = ((x & 0x00FF00FFu) << 8) | ((x >> 8) & 0x00FF00FFu);
  x = (x << 16) | (x >> 16);
  return bits ? x >> (32u - bits) : 0u;
}

HM_HD HmC hm_slot_mul(HmC a, HmC w) {
  HM_SLOT_FP_STRICT
  HmC r;
  r.re = __builtin_fma(a.re, w.re, -(a.im * w.im));
  r.im = __builtin_fma(a.re, w.im, a.im * w.re);
  return r;
}
// forward: (a, b) -> (a + w b, a - w b); inverse: (a, b) -> (a + b, (a - b) conj(w))
template <bool INVERSE>
HM_HD void hm_slot_bfly(HmC &a, HmC &b, HmC w) {
  HM_SLOT_FP_STRICT
  if (INVERSE) {
    const HmC s = {a.re + b.re, a.im + b.im}, d = {a.re - b.re, a.im - b.im};
    w.im = -w.im;
    a = s;
    b = hm_slot_mul(d, w);
  } else {
    const HmC v = hm_slot_mul(b, w);
    const HmC s = {a.re + v.re, a.im + v.im}, d = {a.re - v.re, a.im - v.im};
    a = s;
    b = d;
  }
}
// encode's epilogue on one coefficient: c = rint(v * mul), ties to even; |c| <= half: c mod q, otherwise 0 and the overflow is reported
HM_HD uint64_t hm_slot_round(double v, double mul, uint64_t q, uint64_t half, bool &ovf) {
  HM_SLOT_FP_STRICT
  const double r = __builtin_rint(v * mul);
  const bool fits = __builtin_fabs(r) < 9223372036854775808.0;   // false for a NaN too
  const int64_t c = fits ? (int64_t)r : 0;
  const uint64_t mag = c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c;
  if (!fits || mag > half) { ovf = true; return 0; }
  return c < 0 ? q - mag : mag;
}
// decode's prologue: the centred representative as a double, times 1 / Delta
HM_HD double hm_slot_centre(uint64_t x, double mul, uint64_t q, uint64_t half) {
  HM_SLOT_FP_STRICT
  const int64_t c = x <= half ? (int64_t)x : (int64_t)(x - q);
  return (double)c * mul;
}

template <bool HIGH>
HM_HD uint32_t hm_slot_phys(const HmSlotArgs &a, uint32_t x) { return HIGH ? x : x + (x >> a.log2); }
// the element of the vector (stage order: after the bit reversal of the coefficient index) a tile keeps at x
template <bool HIGH>
HM_HD uint32_t hm_slot_elem(const HmSlotArgs &a, uint32_t tile, uint32_t x) {
  if (HIGH) {
    const uint32_t logW = HM_SLOT_TL - a.log1;
    return (tile << logW) + (x & ((1u << logW) - 1u)) + ((x >> logW) << a.log2);
  }
  const uint32_t block = hm_slot_bitrev((tile << (HM_SLOT_TL - a.log2)) + (x >> a.log2), a.log1);
  return (block << a.log2) + (x & ((1u << a.log2) - 1u));
}
// LOW pass, coefficient side: pair y < T / 2 is the elements x0 and x0 + n2 of the tile, coefficients k0 and k0 + 1 (k0 even)
HM_HD void hm_slot_pair(const HmSlotArgs &a, uint32_t tile, uint32_t y, uint32_t &x0, uint32_t &k0) {
  const uint32_t logW2 = HM_SLOT_TL - a.log2;
  const uint32_t wb = (y & ((1u << (logW2 - 1)) - 1u)) << 1, tr = y >> (logW2 - 1);
  x0 = (wb << a.log2) + hm_slot_bitrev(tr, a.log2);
  k0 = (tr << a.log1) + (tile << logW2) + wb;
}

// ---- the phases of a pass; a barrier separates them.  v = vector, tile < a.tiles, tid < HM_SLOT_THREADS ----
// tile-ordered load (HIGH either direction; LOW of the inverse direction, whose other side is the coefficients)
template <bool HIGH>
HM_HD void hm_slot_load(const HmSlotArgs &a, uint32_t v, uint32_t tile, uint32_t tid, HmC *lds) {
  const HmC *src = a.zin + ((size_t)v << a.logn);
  for (uint32_t x = tid; x < HM_SLOT_T; x += HM_SLOT_THREADS) lds[hm_slot_phys<HIGH>(a, x)] = src[hm_slot_elem<HIGH>(a, tile, x)];
}
template <bool HIGH>
HM_HD void hm_slot_store(const HmSlotArgs &a, uint32_t v, uint32_t tile, uint32_t tid, const HmC *lds) {
  HmC *dst = a.zout + ((size_t)v << a.logn);
  for (uint32_t x = tid; x < HM_SLOT_T; x += HM_SLOT_THREADS) dst[hm_slot_elem<HIGH>(a, tile, x)] = lds[hm_slot_phys<HIGH>(a, x)];
}
// decode's LOW pass: coefficients k and k + n of limb-poly limbs[v] -> (re, im), centred and scaled
HM_HD void hm_slot_load_coef(const HmSlotArgs &a, uint32_t v, uint32_t tile, uint32_t tid, HmC *lds) {
  const uint64_t *src = a.coef + ((size_t)a.limbs[v] << (a.logn + 1));
  for (uint32_t y = tid; y < HM_SLOT_T / 2; y += HM_SLOT_THREADS) {
    uint32_t x0, k0;
    hm_slot_pair(a, tile, y, x0, k0);
    const HmU2 re = *reinterpret_cast<const HmU2 *>(src + k0), im = *reinterpret_cast<const HmU2 *>(src + ((size_t)1 << a.logn) + k0);
    const HmC e0 = {hm_slot_centre(re.x, a.mul, a.q, a.half), hm_slot_centre(im.x, a.mul, a.q, a.half)};
    const HmC e1 = {hm_slot_centre(re.y, a.mul, a.q, a.half), hm_slot_centre(im.y, a.mul, a.q, a.half)};
    lds[hm_slot_phys<false>(a, x0)] = e0;
    lds[hm_slot_phys<false>(a, x0 + (1u << a.log2))] = e1;
  }
}
// encode's LOW pass: (re, im) -> coefficients k and k + n, scaled, rounded, reduced by the source modulus
HM_HD void hm_slot_store_coef(const HmSlotArgs &a, uint32_t v, uint32_t tile, uint32_t tid, const HmC *lds) {
  uint64_t *dst = a.coef + ((size_t)a.limbs[v] << (a.logn + 1));
  bool ovf = false;
  for (uint32_t y = tid; y < HM_SLOT_T / 2; y += HM_SLOT_THREADS) {
    uint32_t x0, k0;
    hm_slot_pair(a, tile, y, x0, k0);
    const HmC e0 = lds[hm_slot_phys<false>(a, x0)], e1 = lds[hm_slot_phys<false>(a, x0 + (1u << a.log2))];
    const HmU2 re = {hm_slot_round(e0.re, a.mul, a.q, a.half, ovf), hm_slot_round(e1.re, a.mul, a.q, a.half, ovf)};
    const HmU2 im = {hm_slot_round(e0.im, a.mul, a.q, a.half, ovf), hm_slot_round(e1.im, a.mul, a.q, a.half, ovf)};
    *reinterpret_cast<HmU2 *>(dst + k0) = re;
    *reinterpret_cast<HmU2 *>(dst + ((size_t)1 << a.logn) + k0) = im;
  }
  if (ovf) *a.flag = 1u;
}
// stage s of a pass (s < log1 for HIGH, < log2 for LOW): the thread's T / 2 / THREADS butterflies
template <bool INVERSE, bool HIGH>
HM_HD void hm_slot_stage(const HmSlotArgs &a, uint32_t tile, uint32_t tid, HmC *lds, uint32_t s) {
  const uint32_t logsub = HIGH ? a.log1 : a.log2, logW = HIGH ? HM_SLOT_TL - a.log1 : 0u;
  const uint32_t logl = INVERSE ? logsub - s : s + 1u;          // the stage joins sub-transforms of length l / 2 into length l
  const uint32_t loghs = logl - 1u + logW, hs = 1u << loghs;    // distance of a butterfly's two elements in the tile
  const uint32_t logLEN = HIGH ? a.log2 + logl : logl;          // the stage's length in the whole transform
  const uint32_t mask = (4u << logLEN) - 1u, shift = a.logn - logLEN;
  for (uint32_t bf = tid; bf < HM_SLOT_T / 2; bf += HM_SLOT_THREADS) {
    const uint32_t rem = bf & (hs - 1u), xa = ((bf >> loghs) << (loghs + 1u)) + rem, xb = xa + hs;
    // J = (element index) mod LEN / 2
    const uint32_t J = HIGH ? (tile << logW) + (rem & ((1u << logW) - 1u)) + ((rem >> logW) << a.log2) : rem;
    const HmC w = a.roots[(a.rot[J] & mask) << shift];
    const uint32_t pa = hm_slot_phys<HIGH>(a, xa), pb = hm_slot_phys<HIGH>(a, xb);
    HmC ea = lds[pa], eb = lds[pb];
    hm_slot_bfly<INVERSE>(ea, eb, w);
    lds[pa] = ea;
    lds[pb] = eb;
  }
}

// the two tables of a ring, built once per context on the host: roots in long double, rounded to double
static inline void hm_slot_tables(uint32_t logN, std::vector<HmC> &roots, std::vector<uint32_t> &rot) {
  const uint32_t N = 1u << logN;
  const long double pi = 3.141592653589793238462643383279502884L;
  roots.resize((size_t)2 * N);
  for (uint32_t k = 0; k < 2 * N; ++k) {
    const long double t = pi * (long double)k / (long double)N;
    roots[k].re = (double)cosl(t);
    roots[k].im = (double)sinl(t);
  }
  rot.resize(N / 2);
  uint32_t e = 1;
  for (uint32_t j = 0; j < N / 2; ++j) { rot[j] = e; e = (uint32_t)(((uint64_t)e * 5u) & (2u * N - 1u)); }
}
