// hm_emu_rescale.cpp — the product operands of the transforms (hm_ntt_passes.inl: MODE 8, the fused forward epilogue whose minuend is a (.) b, and
// MODE 9, the inverse first pass whose input is src (.) b: the kernels of hm_ntt_mix_sub_scale_mul and hm_ntt_mul) on the CPU (TEST INFRASTRUCTURE,
// compiled by tests/test_emu_rescale.py with g++, once per arithmetic back-end: HM_GENERIC = 0 and -DHM_GENERIC=1).  The passes run phase by phase,
// thread by thread, in both geometries (16 and 8 coefficients per thread); the same entry points run the existing MODE 3 / plain inverse passes when
// no second factor is given, so that a test can feed them a separately computed product.  It is not a CPU backend: the product library never links
// or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_modarith.h"
#include "../../homulator_amd/csrc/hm_ntt_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

namespace {
struct Emu {
  hm::Params P;
  std::vector<std::vector<HmW>> fwd, inv, twf, twi;
};
struct G16 {
  typedef hm16::HmNttState State;
  static constexpr int EPT = 16;
  template <int LOGR> static constexpr int rounds() { return hm16::HmRounds<LOGR>::n; }
  template <int TL, int LOGR, bool STRIDED> static constexpr int ldsWords() { return hm16::HmLds<TL, LOGR, STRIDED>::WORDS; }
  template <int TL, int LOGR, bool STRIDED, bool INV, int MODE, int P, class... A> static void phase(A &&...a) { hm16::hm_ntt_phase<TL, LOGR, STRIDED, INV, MODE, P>(a...); }
};
struct G8 {
  typedef hm8::HmNttState State;
  static constexpr int EPT = 8;
  template <int LOGR> static constexpr int rounds() { return hm8::HmRounds<LOGR>::n; }
  template <int TL, int LOGR, bool STRIDED> static constexpr int ldsWords() { return hm8::HmLds<TL, LOGR, STRIDED>::WORDS; }
  template <int TL, int LOGR, bool STRIDED, bool INV, int MODE, int P, class... A> static void phase(A &&...a) { hm8::hm_ntt_phase<TL, LOGR, STRIDED, INV, MODE, P>(a...); }
};
// phase P of every thread of the workgroup, then phase P + 1, ... (a barrier on the GPU = the end of a phase loop here)
template <class G, int TL, int LOGR, bool STRIDED, bool INV, int MODE, int P>
void run_phases(std::vector<typename G::State> &st, uint64_t *lds, const uint64_t *src, uint64_t *dst, uint32_t tile, const HmW *twl, const HmW *twt,
                uint32_t s0, uint32_t prefix0, uint64_t q, HmTw sc, HmEpi ep) {
  for (int t = 0; t < (int)st.size(); ++t) G::template phase<TL, LOGR, STRIDED, INV, MODE, P>(st[t], t, lds, src, dst, tile, twl, twt, s0, prefix0, q, sc, ep);
  if constexpr (P < G::template rounds<LOGR>()) run_phases<G, TL, LOGR, STRIDED, INV, MODE, P + 1>(st, lds, src, dst, tile, twl, twt, s0, prefix0, q, sc, ep);
}
template <class G, int LOGR, bool STRIDED, bool INV, int MODE>
void run_pass(const Emu &e, uint32_t mod, const uint64_t *src, uint64_t *dst, HmTw sc, HmEpi ep) {
  constexpr int TL = HM_TL(STRIDED), THREADS = (1 << TL) / G::EPT;
  const uint64_t q = e.P.mod[mod];
  const HmW *twl = (INV ? e.inv : e.fwd)[mod].data(), *twist = (INV ? e.twi : e.twf)[mod].data();
  const uint32_t s0 = STRIDED ? 0u : (e.P.logN - HM_ROW_LOG);
  std::vector<uint64_t> lds(G::template ldsWords<TL, LOGR, STRIDED>());
  std::vector<typename G::State> st(THREADS);
  for (uint32_t tile = 0; tile < (e.P.N >> TL); ++tile) {
    const uint32_t prefix0 = STRIDED ? 0u : (tile << (TL - LOGR));
    run_phases<G, TL, LOGR, STRIDED, INV, MODE, 0>(st, lds.data(), src, dst, tile, twl, twist + (size_t)prefix0 * 3, s0, prefix0, q, sc, ep);
  }
}
// forward: COL pass (MODE 0, or 4 with the mix prologue `first`), then the ROW pass with the fused epilogue `last`: MODE 8 if `mul`, MODE 3 if not
template <class G, int LOG1>
void forward(const Emu &e, uint32_t mod, const uint64_t *in, uint64_t *out, HmTw sc, const HmEpi &first, const HmEpi &last, bool mul) {
  if (first.b) run_pass<G, LOG1, true, false, 4>(e, mod, in, out, sc, first); else run_pass<G, LOG1, true, false, 0>(e, mod, in, out, sc, first);
  if (mul) run_pass<G, HM_ROW_LOG, false, false, 8>(e, mod, out, out, sc, last); else run_pass<G, HM_ROW_LOG, false, false, 3>(e, mod, out, out, sc, last);
}
// inverse: ROW pass (MODE 9 if `mul`: the second factor in first.b, MODE 0 if not), then the COL pass with the scale
template <class G, int LOG1>
void inverse(const Emu &e, uint32_t mod, const uint64_t *in, uint64_t *out, HmTw sc, const HmEpi &first, const HmEpi &, bool mul) {
  if (mul) run_pass<G, HM_ROW_LOG, false, true, 9>(e, mod, in, out, sc, first); else run_pass<G, HM_ROW_LOG, false, true, 0>(e, mod, in, out, sc, first);
  run_pass<G, LOG1, true, true, 2>(e, mod, out, out, sc, hm_epi_none());
}
template <bool INV>
int run(const Emu &e, int ept, uint32_t mod, const uint64_t *in, uint64_t *out, HmTw sc, const HmEpi &first, const HmEpi &last, bool mul) {
  const uint32_t log1 = e.P.logN - HM_ROW_LOG;
#define HM_CASE(G, n) { if (INV) inverse<G, n>(e, mod, in, out, sc, first, last, mul); else forward<G, n>(e, mod, in, out, sc, first, last, mul); return 0; }
  if (ept == 8) {
    if (log1 == 8) HM_CASE(G8, 8)
    if (log1 == 7) HM_CASE(G8, 7)
    return 1;
  }
  switch (log1) {
  case 5: HM_CASE(G16, 5)
  case 6: HM_CASE(G16, 6)
  case 7: HM_CASE(G16, 7)
  case 8: HM_CASE(G16, 8)
  case 9: HM_CASE(G16, 9)
  }
#undef HM_CASE
  return 1;
}
// the second factor and the modulus's Barrett constants, where MODE 8 / 9 take them (hm_ntt_core.h)
void product_operand(const Emu &e, uint32_t mod, HmEpi &ep, const uint64_t *b) { ep.b = b; ep.bk.w = e.P.modc[mod].mu; ep.bk.ws = e.P.modc[mod].sh; }
}   // namespace

extern "C" {
int emu_rescale_generic(void) { return HM_GENERIC; }
// q: L moduli, p: K special moduli (primes = 1 mod 2N below 2^60); nullptr if the chain does not fit this build's arithmetic
void *emu_rescale_create(uint32_t logN, uint32_t L, uint32_t K, const uint64_t *q, const uint64_t *p) {
  Emu *e = new Emu;
  try {
    e->P.init(logN, L, K, q, p, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    delete e;
    return nullptr;
  }
  e->fwd.resize(L + K); e->inv.resize(L + K); e->twf.resize(L + K); e->twi.resize(L + K);
  for (uint32_t m = 0; m < L + K; ++m) {
    e->fwd[m].resize(e->P.N); e->inv[m].resize(e->P.N);
    e->twf[m].resize((e->P.N >> 8) * 3); e->twi[m].resize((e->P.N >> 8) * 3);
    e->P.make_twist(m, false, e->twf[m].data());
    e->P.make_twist(m, true, e->twi[m].data());
    e->P.make_table(m, false, e->fwd[m].data());
    e->P.make_table(m, true, e->inv[m].data());
  }
  return e;
}
void emu_rescale_destroy(void *h) { delete (Emu *)h; }
uint64_t emu_rescale_modulus(void *h, uint32_t m) { return ((Emu *)h)->P.mod[m]; }

// out = (minuend [(.) minuend_b] - NTT(in [+ mix_k * mix])) * k [+ addend [* addend_k]]; minuend_b == nullptr: the existing MODE 3 epilogue
// (mix_k / addend_k = 0: none).  ept: 16 or 8 coefficients per thread
int emu_ntt_sub_scale_mul(void *h, int ept, uint32_t mod, const uint64_t *in, const uint64_t *minuend, const uint64_t *minuend_b, const uint64_t *addend,
                          uint64_t *out, uint64_t k, const uint64_t *mix, uint64_t mix_k, uint64_t addend_k) {
  Emu &e = *(Emu *)h;
  const uint64_t q = e.P.mod[mod];
  HmEpi first = hm_epi_none(), last = hm_epi_none();
  last.a = minuend; last.d = addend;
  if (addend_k) last.dk = hm_kconst(addend_k, q);
  if (mix) { first.b = mix; first.bk = hm_kconst(mix_k, q); }
  if (minuend_b) product_operand(e, mod, last, minuend_b);
  return run<false>(e, ept, mod, in, out, hm_kconst(k, q), first, last, minuend_b != nullptr);
}
// out = INTT(in [(.) in_b]) * N^-1 [* scale]; in_b == nullptr: the existing plain inverse transform (has_scale = 0: no extra scale)
int emu_intt_mul(void *h, int ept, uint32_t mod, const uint64_t *in, const uint64_t *in_b, uint64_t *out, uint64_t scale, int has_scale) {
  Emu &e = *(Emu *)h;
  const uint64_t q = e.P.mod[mod];
  uint64_t k = e.P.modc[mod].ninv;
  if (has_scale) k = hm::mulmod(k, scale, q);
  HmEpi first = hm_epi_none();
  if (in_b) product_operand(e, mod, first, in_b);
  return run<true>(e, ept, mod, in, out, hm_kconst(k, q), first, hm_epi_none(), in_b != nullptr);
}
// the product step alone: x (.) y as MODE 8 / 9 form it
uint64_t emu_epi_mul(void *h, uint32_t mod, uint64_t x, uint64_t y) {
  Emu &e = *(Emu *)h;
  HmEpi ep = hm_epi_none();
  product_operand(e, mod, ep, nullptr);
  return hm_epi_mul(x, y, e.P.mod[mod], ep);
}
// the MODE 8 epilogue of ONE coefficient: x = the transform's lazy value (any value below 2 HM_LAZY_Q q), va = the product minuend, vd = the addend
// (has_addend = 0: none; addend_k = 0: as is)
uint64_t emu_epilogue8(void *h, uint32_t mod, uint64_t x, uint64_t va, uint64_t vd, int has_addend, uint64_t k, uint64_t addend_k) {
  Emu &e = *(Emu *)h;
  const uint64_t q = e.P.mod[mod];
  HmEpi ep = hm_epi_none();
  ep.d = has_addend ? &vd : nullptr;
  if (addend_k) ep.dk = hm_kconst(addend_k, q);
  return hm16::hm_epilogue<8>(x, va, vd, q, hm_kconst(k, q), ep);
}
int emu_lazy_q(void) { return HM_LAZY_Q; }
}
