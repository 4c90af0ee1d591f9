// hm_emu_lift.cpp — the lifted forward first pass (hm_ntt_passes.inl: MODE 10, hm_ph_load_global_lift over hm_lift of hm_ntt_core.h: the kernel of
// hm_ntt_lift, ModRaise) on the CPU (TEST INFRASTRUCTURE, compiled by tests/test_emu_lift.py with g++, once per arithmetic back-end: HM_GENERIC = 0
// and -DHM_GENERIC=1).  The passes run phase by phase, thread by thread, in both geometries (16 and 8 coefficients per thread): the COL pass in MODE 10,
// then the plain ROW pass (MODE 1).  It is not a CPU backend: the product library never links or calls this.
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_modarith.h"
#include "../../homulator_amd/csrc/hm_ntt_core.h"
#include "../../homulator_amd/csrc/hm_params.h"

namespace {
struct Emu {
  hm::Params P;
  std::vector<std::vector<HmW>> fwd, twf;
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
  static_assert(!INV, "forward passes only");
  const HmW *twl = e.fwd[mod].data(), *twist = e.twf[mod].data();
  const uint32_t s0 = STRIDED ? 0u : (e.P.logN - HM_ROW_LOG);
  std::vector<uint64_t> lds(G::template ldsWords<TL, LOGR, STRIDED>());
  std::vector<typename G::State> st(THREADS);
  for (uint32_t tile = 0; tile < (e.P.N >> TL); ++tile) {
    const uint32_t prefix0 = STRIDED ? 0u : (tile << (TL - LOGR));
    run_phases<G, TL, LOGR, STRIDED, INV, MODE, 0>(st, lds.data(), src, dst, tile, twl, twist + (size_t)prefix0 * 3, s0, prefix0, q, sc, ep);
  }
}
// the lift's constants where MODE 10 takes them (hm_ntt_core.h), made as the launch code makes them: q_s, q_s mod q, floor(2^64 / q)
HmEpi lift_operand(const Emu &e, uint32_t src_mod, uint32_t mod) {
  const uint64_t qs = e.P.mod[src_mod], q = e.P.mod[mod];
  HmEpi ep = hm_epi_none();
  ep.dk.w = qs; ep.bk.ws = qs % q; ep.bk.w = (uint64_t)(((hm_u128)1 << 64) / q);
  return ep;
}
template <class G, int LOG1>
void forward(const Emu &e, uint32_t src_mod, uint32_t mod, const uint64_t *in, uint64_t *out) {
  const HmTw none = {0, 0};
  run_pass<G, LOG1, true, false, 10>(e, mod, in, out, none, lift_operand(e, src_mod, mod));
  run_pass<G, HM_ROW_LOG, false, false, 1>(e, mod, out, out, none, hm_epi_none());
}
}   // namespace

extern "C" {
int emu_lift_generic(void) { return HM_GENERIC; }
// q: L moduli, p: K special moduli (primes = 1 mod 2N between 2^20 and 2^60); nullptr if the chain does not fit this build's arithmetic
void *emu_lift_create(uint32_t logN, uint32_t L, uint32_t K, const uint64_t *q, const uint64_t *p) {
  Emu *e = new Emu;
  try {
    e->P.init(logN, L, K, q, p, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    delete e;
    return nullptr;
  }
  e->fwd.resize(L + K); e->twf.resize(L + K);
  for (uint32_t m = 0; m < L + K; ++m) {
    e->fwd[m].resize(e->P.N);
    e->twf[m].resize((e->P.N >> 8) * 3);
    e->P.make_twist(m, false, e->twf[m].data());
    e->P.make_table(m, false, e->fwd[m].data());
  }
  return e;
}
void emu_lift_destroy(void *h) { delete (Emu *)h; }
uint64_t emu_lift_modulus(void *h, uint32_t m) { return ((Emu *)h)->P.mod[m]; }
// out = NTT_{mod}(centre_{src_mod}(in) mod q_mod); in and out must not overlap (the first pass of a tile reads `in` while earlier tiles have
// written `out`).  ept: 16 or 8 coefficients per thread.  1: the geometry does not exist at this ring size
int emu_ntt_lift(void *h, int ept, uint32_t src_mod, uint32_t mod, const uint64_t *in, uint64_t *out) {
  const Emu &e = *(Emu *)h;
  const uint32_t log1 = e.P.logN - HM_ROW_LOG;
#define HM_CASE(G, n) { forward<G, n>(e, src_mod, mod, in, out); return 0; }
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
// the load routine's arithmetic on ONE word: c is any word below 2^60, not only a residue of q_src
uint64_t emu_lift_word(void *h, uint32_t src_mod, uint32_t mod, uint64_t c) {
  const Emu &e = *(Emu *)h;
  return hm_lift(c, e.P.mod[mod], lift_operand(e, src_mod, mod));
}
}
