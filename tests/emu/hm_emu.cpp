// hm_emu.cpp — host emulator of the HIP kernels' per-thread phase functions (TEST INFRASTRUCTURE).
// Compiles homulator_amd/csrc/hm_*_core.h with g++ and runs each workgroup phase by phase, thread by
// thread, so that index maths, twiddle indexing, lazy-reduction ranges and the host-side parameter
// tables (hm_params.cpp) are checked against the oracle on the CPU before a GPU is involved.
// It is not a CPU backend: the product library never links or calls this.
// Built twice, like the kernels: libhm_emu.so (HM_GENERIC = 0: word-wise Montgomery on primes h 2^32 + 1) and libhm_emu_gen.so
// (-DHM_GENERIC=1: Shoup / Barrett arithmetic on any NTT-friendly chain).
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../../homulator_amd/csrc/hm_elem_core.h"
#include "../../homulator_amd/csrc/hm_ip_core.h"
#include "../../homulator_amd/csrc/hm_modarith.h"
#include "../../homulator_amd/csrc/hm_ntt_core.h"
#include "../../homulator_amd/csrc/hm_params.h"
#include "../../homulator_amd/csrc/hm_launch.h"
#include "../../homulator_amd/csrc/hm_bconv_plan.h"

struct Emu {
  hm::Params P;
  std::vector<std::vector<HmW>> fwd, inv, twf, twi;
};

// the two geometries of the passes (hm_ntt_core.h): 16 coefficients per thread (hm16) and 8 (hm8, N = 2^16 only)
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
static void run_phases(std::vector<typename G::State> &st, uint64_t *lds, const uint64_t *src, uint64_t *dst, uint32_t tile, const HmW *twl,
                       const HmW *twt, uint32_t s0, uint32_t prefix0, uint64_t q, HmTw sc, HmEpi ep) {
  for (int t = 0; t < (int)st.size(); ++t) G::template phase<TL, LOGR, STRIDED, INV, MODE, P>(st[t], t, lds, src, dst, tile, twl, twt, s0, prefix0, q, sc, ep);
  if constexpr (P < G::template rounds<LOGR>()) run_phases<G, TL, LOGR, STRIDED, INV, MODE, P + 1>(st, lds, src, dst, tile, twl, twt, s0, prefix0, q, sc, ep);
}

template <class G, int LOGR, bool STRIDED, bool INV, int MODE>
static void run_pass(const Emu &e, uint32_t mod, const uint64_t *src, uint64_t *dst, HmTw sc, HmEpi ep = hm_epi_none()) {
  constexpr int TL = HM_TL(STRIDED), THREADS = (1 << TL) / G::EPT;
  const uint32_t tiles = e.P.N >> TL;
  const uint64_t q = e.P.mod[mod];
  const HmW *twl = (INV ? e.inv : e.fwd)[mod].data();
  const uint32_t s0 = STRIDED ? 0u : (e.P.logN - HM_ROW_LOG);
  std::vector<uint64_t> lds(G::template ldsWords<TL, LOGR, STRIDED>());
  std::vector<typename G::State> st(THREADS);
  const HmW *twist = (INV ? e.twi : e.twf)[mod].data();
  // a pass may run in place (src == dst): every thread reads its elements before any thread writes its own
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    const uint32_t prefix0 = STRIDED ? 0u : (tile << (TL - LOGR));
    const HmW *twt = twist + (size_t)prefix0 * 3;
    run_phases<G, TL, LOGR, STRIDED, INV, MODE, 0>(st, lds.data(), src, dst, tile, twl, twt, s0, prefix0, q, sc, ep);
  }
}

template <class G, int LOG1>
static void run_ntt(const Emu &e, uint32_t mod, const uint64_t *in, uint64_t *out, int inverse, HmTw sc) {
  if (!inverse) {
    run_pass<G, LOG1, true, false, 0>(e, mod, in, out, sc);
    run_pass<G, HM_ROW_LOG, false, false, 1>(e, mod, out, out, sc);
  } else {
    run_pass<G, HM_ROW_LOG, false, true, 0>(e, mod, in, out, sc);
    run_pass<G, LOG1, true, true, 2>(e, mod, out, out, sc);
  }
}

// the conversion through the kernel of width KN >= p.n_in (p.table: the conversion's device table for that width, hm_bconv_table_words; the inputs
// a narrow digit does not have: p.in_limb[n_in .. KN), hm_bcol_window)
template <int KN>
static void emu_bconv_n(const HmBconvProb &p, uint32_t logN) {
  for (uint32_t t0 = 0; t0 < p.n_out; t0 += HM_BCONV_CHUNK) {
    uint32_t t1 = t0 + HM_BCONV_CHUNK < p.n_out ? t0 + HM_BCONV_CHUNK : p.n_out;
    for (uint32_t x = 0; x < (1u << logN); x += HM_BCONV_CPT) {
      if (p.in_packed) hm_bconv_thread<KN, HM_BCONV_CPT, true>(p, logN, x, t0, t1);
      else hm_bconv_thread<KN, HM_BCONV_CPT, false>(p, logN, x, t0, t1);
    }
  }
}

// round 6: the arithmetic of the two-group conversion of k_bconv_col (digits of 16 .. 32 limbs, hm_bcol_units_wide): per output and coefficient the
// 128-bit sums of the group [0, 16) and of the group [16, n_in) (hm_bconv_cols: carry-free split-30 columns, recombined per group), added, ONE
// Montgomery reduction for all n_in terms (hm_redc_wide<N_IN>).  Same table as the kernel (hm_bconv_table_words); packed != 0: the inputs arrive in the split-30 packed form.
template <int N_IN>
static void emu_bconv_wide_n(Emu &e, const uint32_t *out_ids, uint32_t n_out, const std::vector<uint64_t> &table, const uint64_t *in, uint64_t *out, int packed) {
  constexpr int ROWS = (N_IN + 7) / 8, C1 = N_IN - 16;
  const uint32_t N = e.P.N;
  HmConstRow8 rows = HM_CONST_ROWS(table.data());
  for (uint32_t t = 0; t < n_out; ++t) {
    const HmMod &m = e.P.modc[out_ids[t]];
    HmRow8 r0[2], r1[(C1 > 0 ? C1 + 7 : 8) / 8];
    r0[0] = rows[(size_t)t * ROWS]; r0[1] = rows[(size_t)t * ROWS + 1];
    for (int g = 0; g < (C1 + 7) / 8; ++g) r1[g] = rows[(size_t)t * ROWS + 2 + g];
    for (uint32_t x = 0; x < N; ++x) {
      uint32_t yl[16], yh[16], zl[C1 > 0 ? C1 : 1] = {0}, zh[C1 > 0 ? C1 : 1] = {0};
      for (int i = 0; i < N_IN; ++i) {
        const uint64_t v = in[(size_t)i * N + x];
        const uint32_t lo = packed ? (uint32_t)v : (uint32_t)v & 0x3FFFFFFFu, hi = packed ? (uint32_t)(v >> 32) : (uint32_t)(v >> 30);
        if (i < 16) { yl[i] = lo; yh[i] = hi; } else { zl[i - 16] = lo; zh[i - 16] = hi; }
      }
      hm_u128 acc = hm_bconv_cols<16>(yl, yh, r0);
      if constexpr (C1 > 0) acc += hm_bconv_cols<C1>(zl, zh, r1);
      out[(size_t)t * N + x] = hm_redc_wide<N_IN>(acc, m);
    }
  }
}

// the 256-point ROW pass's LDS image as the kernels index it, for tools/lds_banks.py's bank model (tests/test_emu_kernels.py pins the
// model to these): the LDS word of access unit a of thread tid in round R (ept = 16 / 8: geometry; inverse: the pass's direction)
template <int R> static int row_unit16(int tid, int a, bool inv) {
  int i0, i1, xb, d, c;
  hm16::HmRound<12, 8, false, R>::unit_split(tid, a, i0, i1, xb, d, c);
  return inv ? hm16::hm_lds_at<12, 8, false, true>(xb, d, c) : hm16::hm_lds_at<12, 8, false, false>(xb, d, c);
}
template <int R> static int row_unit8(int tid, int a, bool inv) {
  int i0, i1, xb, d, c;
  hm8::HmRound<12, 8, false, R>::unit_split(tid, a, i0, i1, xb, d, c);
  return inv ? hm8::hm_lds_at<12, 8, false, true>(xb, d, c) : hm8::hm_lds_at<12, 8, false, false>(xb, d, c);
}
// round 6: the transforms that read an operand through an automorphism (MODE 6: the inverse transform's input; MODE 7: the fused epilogue's addend),
// both geometries (ept = 16 / 8)
template <class G, int LOG1>
static void run_intt_auto(const Emu &e, uint32_t mod, const uint64_t *in, uint64_t *out, HmTw sc, uint32_t g) {
  HmEpi ep = hm_epi_none();
  ep.g = g; ep.logN = e.P.logN;
  run_pass<G, HM_ROW_LOG, false, true, 6>(e, mod, in, out, sc, ep);
  run_pass<G, LOG1, true, true, 2>(e, mod, out, out, sc);
}
// K5 (hm_ip_core.h): a form's per-thread function over every (entry, chunk, thread) of its launch, in that order.  No thread reads what another
// writes (the entry points refuse such calls), so the order is free
template <class Args, class Thread>
static void run_ip(const Args &a, Thread thread) {
  for (uint32_t entry = 0; entry < a.n_limbs; ++entry)
    for (uint32_t chunk = 0; chunk < (1u << a.logN) / HM_IP_CHUNK; ++chunk)
      for (uint32_t tid = 0; tid < HM_IP_CHUNK / 2; ++tid) thread(a, entry, chunk, tid);
}
static bool ip_counts_ok(uint32_t T, uint32_t v, uint32_t vmax) { return T >= 1 && T <= HM_IP_MAX_TERMS && v >= 1 && v <= vmax; }

extern "C" {
// q == nullptr: the default chain; otherwise a caller-chosen one (q: L moduli, p: K special moduli; primes = 1 mod 2N below 2^60).
// Returns nullptr if the chain does not fit this build's arithmetic.
static void *emu_make(uint32_t logN, uint32_t L, uint32_t K, const uint64_t *q, const uint64_t *p, bool tables) {
  Emu *e = new Emu;
  try {
    e->P.init(logN, L, K, q, p, nullptr, HM_GENERIC != 0);
  } catch (const std::exception &) {
    delete e;
    return nullptr;
  }
  if (!tables) return e;
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
void *emu_create(uint32_t logN, uint32_t L, uint32_t K) { return emu_make(logN, L, K, nullptr, nullptr, true); }
void *emu_create_chain(uint32_t logN, uint32_t L, uint32_t K, const uint64_t *q, const uint64_t *p) { return emu_make(logN, L, K, q, p, true); }
// only the modulus constants (the element-wise checks that need no twiddle tables)
void *emu_create_mods(uint32_t logN, uint32_t L, uint32_t K, const uint64_t *q, const uint64_t *p) { return emu_make(logN, L, K, q, p, false); }
int emu_generic(void) { return HM_GENERIC; }
void emu_destroy(void *h) { delete (Emu *)h; }
uint64_t emu_modulus(void *h, uint32_t m) { return ((Emu *)h)->P.mod[m]; }
uint64_t emu_psi(void *h, uint32_t m) { return ((Emu *)h)->P.psi[m]; }

int emu_ntt(void *h, uint32_t mod, const uint64_t *in, uint64_t *out, int inverse, uint64_t scale, int has_scale) {
  Emu &e = *(Emu *)h;
  uint64_t q = e.P.mod[mod], k = e.P.modc[mod].ninv;
  if (has_scale) k = hm::mulmod(k, scale, q);
  HmTw sc = hm_kconst(k, q);
  switch (e.P.logN - HM_ROW_LOG) {
  case 5: run_ntt<G16, 5>(e, mod, in, out, inverse, sc); break;
  case 6: run_ntt<G16, 6>(e, mod, in, out, inverse, sc); break;
  case 7: run_ntt<G16, 7>(e, mod, in, out, inverse, sc); break;
  case 8: run_ntt<G16, 8>(e, mod, in, out, inverse, sc); break;
  case 9: run_ntt<G16, 9>(e, mod, in, out, inverse, sc); break;
  default: return 1;
  }
  return 0;
}

// fused forward transform: out = (minuend - NTT(in [+ mix_k * mix])) * k [+ addend [* addend_k]]   (mix_k / addend_k = 0: none)
int emu_ntt_sub_scale(void *h, uint32_t mod, const uint64_t *in, const uint64_t *minuend, const uint64_t *addend, uint64_t *out,
                      uint64_t k, const uint64_t *mix, uint64_t mix_k, uint64_t addend_k) {
  Emu &e = *(Emu *)h;
  const uint64_t q = e.P.mod[mod];
  HmTw sc = hm_kconst(k, q);
  HmEpi ep = hm_epi_none();
  ep.a = minuend; ep.d = addend;
  if (addend_k) ep.dk = hm_kconst(addend_k, q);
  if (mix) { ep.b = mix; ep.bk = hm_kconst(mix_k, q); }
  switch (e.P.logN - HM_ROW_LOG) {
#define HM_CASE(n) case n: if (mix) run_pass<G16, n, true, false, 4>(e, mod, in, out, sc, ep); else run_pass<G16, n, true, false, 0>(e, mod, in, out, sc); break;
    HM_CASE(5) HM_CASE(6) HM_CASE(7) HM_CASE(8) HM_CASE(9)
#undef HM_CASE
  default: return 1;
  }
  run_pass<G16, HM_ROW_LOG, false, false, 3>(e, mod, out, out, sc, ep);
  return 0;
}
// the 8-coefficient geometry (hm8: 512-thread workgroups, radix-4 rounds), N = 2^16 and (round 6) N = 2^15
int emu_ntt8(void *h, uint32_t mod, const uint64_t *in, uint64_t *out, int inverse, uint64_t scale, int has_scale) {
  Emu &e = *(Emu *)h;
  if (e.P.logN != 16 && e.P.logN != 15) return 1;
  uint64_t q = e.P.mod[mod], k = e.P.modc[mod].ninv;
  if (has_scale) k = hm::mulmod(k, scale, q);
  if (e.P.logN == 16) run_ntt<G8, 8>(e, mod, in, out, inverse, hm_kconst(k, q));
  else run_ntt<G8, 7>(e, mod, in, out, inverse, hm_kconst(k, q));
  return 0;
}
int emu_ntt_sub_scale8(void *h, uint32_t mod, const uint64_t *in, const uint64_t *minuend, const uint64_t *addend, uint64_t *out,
                       uint64_t k, const uint64_t *mix, uint64_t mix_k, uint64_t addend_k) {
  Emu &e = *(Emu *)h;
  if (e.P.logN != 16 && e.P.logN != 15) return 1;
  const uint64_t q = e.P.mod[mod];
  HmTw sc = hm_kconst(k, q);
  HmEpi ep = hm_epi_none();
  ep.a = minuend; ep.d = addend;
  if (addend_k) ep.dk = hm_kconst(addend_k, q);
  if (mix) { ep.b = mix; ep.bk = hm_kconst(mix_k, q); }
  if (e.P.logN == 16) { if (mix) run_pass<G8, 8, true, false, 4>(e, mod, in, out, sc, ep); else run_pass<G8, 8, true, false, 0>(e, mod, in, out, sc); }
  else { if (mix) run_pass<G8, 7, true, false, 4>(e, mod, in, out, sc, ep); else run_pass<G8, 7, true, false, 0>(e, mod, in, out, sc); }
  run_pass<G8, HM_ROW_LOG, false, false, 3>(e, mod, out, out, sc, ep);
  return 0;
}
int emu_intt_auto(void *h, uint32_t mod, const uint64_t *in, uint64_t *out, uint32_t galois, int ept) {
  Emu &e = *(Emu *)h;
  if (in == out || (ept == 8 && e.P.logN != 16 && e.P.logN != 15)) return 1;
  const uint64_t q = e.P.mod[mod];
  const HmTw sc = hm_kconst(e.P.modc[mod].ninv, q);
  if (ept == 8) { if (e.P.logN == 16) run_intt_auto<G8, 8>(e, mod, in, out, sc, galois); else run_intt_auto<G8, 7>(e, mod, in, out, sc, galois); return 0; }
  switch (e.P.logN - HM_ROW_LOG) {
  case 5: run_intt_auto<G16, 5>(e, mod, in, out, sc, galois); break;
  case 6: run_intt_auto<G16, 6>(e, mod, in, out, sc, galois); break;
  case 7: run_intt_auto<G16, 7>(e, mod, in, out, sc, galois); break;
  case 8: run_intt_auto<G16, 8>(e, mod, in, out, sc, galois); break;
  case 9: run_intt_auto<G16, 9>(e, mod, in, out, sc, galois); break;
  default: return 1;
  }
  return 0;
}
int emu_ntt_sub_scale_auto(void *h, uint32_t mod, const uint64_t *in, const uint64_t *minuend, const uint64_t *addend, uint64_t *out, uint64_t k,
                           uint64_t addend_k, uint32_t galois, int ept) {
  Emu &e = *(Emu *)h;
  if (ept == 8 && e.P.logN != 16 && e.P.logN != 15) return 1;
  const uint64_t q = e.P.mod[mod];
  const HmTw sc = hm_kconst(k, q);
  HmEpi ep = hm_epi_none();
  ep.a = minuend; ep.d = addend; ep.g = galois; ep.logN = e.P.logN;
  if (addend_k) ep.dk = hm_kconst(addend_k, q);
  if (ept == 8) {
    if (e.P.logN == 16) run_pass<G8, 8, true, false, 0>(e, mod, in, out, sc); else run_pass<G8, 7, true, false, 0>(e, mod, in, out, sc);
    run_pass<G8, HM_ROW_LOG, false, false, 7>(e, mod, out, out, sc, ep);
    return 0;
  }
  switch (e.P.logN - HM_ROW_LOG) {
#define HM_CASE(n) case n: run_pass<G16, n, true, false, 0>(e, mod, in, out, sc); break;
    HM_CASE(5) HM_CASE(6) HM_CASE(7) HM_CASE(8) HM_CASE(9)
#undef HM_CASE
  default: return 1;
  }
  run_pass<G16, HM_ROW_LOG, false, false, 7>(e, mod, out, out, sc, ep);
  return 0;
}
void emu_tensor(void *h, uint32_t mod, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d, uint64_t *o0,
                uint64_t *o1, uint64_t *o2) {
  Emu &e = *(Emu *)h;
  for (uint32_t x = 0; x < e.P.N; ++x) hm_tensor_one(a[x], b[x], c[x], d[x], e.P.modc[mod], o0[x], o1[x], o2[x]);
}

void emu_ewe(void *h, int op, uint32_t mod, const uint64_t *a, const uint64_t *b, const uint64_t *c,
             const uint64_t *d, uint64_t kk, uint64_t *out) {
  Emu &e = *(Emu *)h;
  const HmMod m = e.P.modc[mod];
  HmTw k = {kk, hm::shoup(kk, m.q)};
  for (uint32_t x = 0; x < e.P.N; ++x) {
    uint64_t va = a ? a[x] : 0, vb = b ? b[x] : 0, vc = c ? c[x] : 0, vd = d ? d[x] : 0, r = 0;
    switch (op) {
    case 0: r = hm_ewe_one<0>(va, vb, vc, vd, k, m); break;
    case 1: r = hm_ewe_one<1>(va, vb, vc, vd, k, m); break;
    case 2: r = hm_ewe_one<2>(va, vb, vc, vd, k, m); break;
    case 3: r = hm_ewe_one<3>(va, vb, vc, vd, k, m); break;
    case 4: r = hm_ewe_one<4>(va, vb, vc, vd, k, m); break;
    case 5: r = hm_ewe_one<5>(va, vb, vc, vd, k, m); break;
    case 6: r = hm_ewe_one<6>(va, vb, vc, vd, k, m); break;
    case 7: r = hm_ewe_one<7>(va, vb, vc, vd, k, m); break;
    case 8: r = hm_ewe_one<8>(va, vb, vc, vd, k, m); break;
    }
    out[x] = r;
  }
}

// packed != 0: the inputs are first brought into the split-30 packed form (hm_pack30) and the conversion is told so (in_packed).
// kn >= n_in: the width of the kernel the conversion runs (kn > n_in: a narrow digit in a wider digit's kernel, as bconv_col_launch merges them);
// log_len: limb-polys of 2^log_len coefficients (hm_bconv_desc::log_len; 0 = the ring's)
int emu_bconv_kn(void *h, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out, uint32_t kn,
                 const uint64_t *in, uint64_t *out, int packed, uint32_t log_len) {
  Emu &e = *(Emu *)h;
  const uint32_t logN = log_len ? log_len : e.P.logN;
  if (kn < n_in || kn > HM_BCONV_MAX_IN || logN < 8 || logN > e.P.logN) return 1;
  const std::vector<uint64_t> table = hm_bconv_table_words(e.P, in_ids, n_in, out_ids, n_out, kn);
  std::vector<uint64_t> pk;
  if (packed) {
    pk.assign(in, in + ((size_t)n_in << logN));
    for (uint64_t &v : pk) v = hm_pack30(v);
    in = pk.data();
  }
  HmBconvProb p;
  hm_bconv_fill(p, in, table.data(), kn, nullptr, n_in, nullptr, n_out, packed != 0);
  p.out = out;
  const HmBcolWindow w = hm_bcol_window(nullptr, n_in, kn, logN);
  memcpy(p.in_limb, w.limb, sizeof p.in_limb);
  switch (kn) {
#define HM_CASE(n) case n: emu_bconv_n<n>(p, logN); break;
    HM_CASE(1) HM_CASE(2) HM_CASE(3) HM_CASE(4) HM_CASE(5) HM_CASE(6) HM_CASE(7) HM_CASE(8)
    HM_CASE(9) HM_CASE(10) HM_CASE(11) HM_CASE(12) HM_CASE(13) HM_CASE(14) HM_CASE(15) HM_CASE(16)
    HM_CASE(17) HM_CASE(18) HM_CASE(19) HM_CASE(20) HM_CASE(21) HM_CASE(22) HM_CASE(23) HM_CASE(24)
    HM_CASE(25) HM_CASE(26) HM_CASE(27) HM_CASE(28) HM_CASE(29) HM_CASE(30) HM_CASE(31) HM_CASE(32)
#undef HM_CASE
  }
  return 0;
}
void emu_bconv_form(void *h, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out,
                    const uint64_t *in, uint64_t *out, int packed) { emu_bconv_kn(h, in_ids, n_in, out_ids, n_out, n_in, in, out, packed, 0); }
void emu_bconv(void *h, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out,
               const uint64_t *in, uint64_t *out) { emu_bconv_kn(h, in_ids, n_in, out_ids, n_out, n_in, in, out, 0, 0); }
int emu_bconv_two_groups(void *h, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out, const uint64_t *in, uint64_t *out, int packed) {
  Emu &e = *(Emu *)h;
  const std::vector<uint64_t> table = hm_bconv_table_words(e.P, in_ids, n_in, out_ids, n_out, n_in);
  switch (n_in) {
#define HM_CASE(n) case n: emu_bconv_wide_n<n>(e, out_ids, n_out, table, in, out, packed); break;
    HM_CASE(16) HM_CASE(17) HM_CASE(18) HM_CASE(19) HM_CASE(20) HM_CASE(21) HM_CASE(22) HM_CASE(23) HM_CASE(24)
    HM_CASE(25) HM_CASE(26) HM_CASE(27) HM_CASE(28) HM_CASE(29) HM_CASE(30) HM_CASE(31) HM_CASE(32)
#undef HM_CASE
  default: return 1;
  }
  return 0;
}
void emu_bconv_consts(void *h, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out,
                      uint64_t *qh, uint64_t *tb) {
  ((Emu *)h)->P.bconv_consts(in_ids, n_in, out_ids, n_out, qh, tb);
}
void emu_automorph(void *h, const uint64_t *in, uint64_t *out, uint32_t g) {
  Emu &e = *(Emu *)h;
  for (uint32_t i = 0; i < e.P.N; ++i) out[i] = in[hm_auto_src(i, g, e.P.logN)];
}
void emu_fill(void *h, uint32_t mod, uint64_t stream, uint64_t *out) {
  Emu &e = *(Emu *)h;
  for (uint32_t x = 0; x < e.P.N; ++x) out[x] = hm_synth(stream, x, e.P.mod[mod]);
}

// the fused kernel's key multiply-accumulate (hm_mac_add, lazy form) element by element: acc[i] (+)= x[i] * y[i], `fold` as for the third
// and later terms; returns the raw lazy accumulators (the test checks range and congruence), and the final reduction separately
int emu_mac(void *h, uint32_t mod, uint64_t *acc, const uint64_t *x, const uint64_t *y, uint32_t n, int fold) {
  Emu &e = *(Emu *)h;
  const HmMod &m = e.P.modc[mod];
  const hm16::HmMacMod mm = hm16::hm_mac_mod(m);
  for (uint32_t i = 0; i < n; ++i) hm16::hm_mac_add(acc[i], x[i], y[i], m, mm, fold != 0);
  return 0;
}
uint64_t emu_mac_final(void *h, uint32_t mod, uint64_t acc) { return hm16::hm_mac_final(acc, ((Emu *)h)->P.modc[mod]); }
// the word-wise Montgomery product itself (hm_mont_acc): out[i] = c[i] + x[i] * wt[i] * 2^-64 mod q + {0, q}; and the per-launch constant
// product (hm_mont_const_mul), the wide reduction (hm_redc_wide) and one forward / inverse butterfly of each kind
#if !HM_GENERIC
void emu_mont_acc(void *h, uint32_t mod, const uint64_t *c, const uint64_t *x, const uint64_t *wt, uint64_t *out, uint32_t n) {
  const HmBflyMod m = hm_bfly_mod(((Emu *)h)->P.mod[mod]);
  for (uint32_t i = 0; i < n; ++i) out[i] = hm_mont_acc(c[i], x[i], wt[i], m);
}
uint64_t emu_mont_const_mul(void *h, uint32_t mod, uint64_t x, uint64_t k) {
  const uint64_t q = ((Emu *)h)->P.mod[mod];
  return hm_mont_const_mul(x, hm_to_mont(k, q), q);
}
#endif
uint64_t emu_redc_wide(void *h, uint32_t mod, uint64_t lo, uint64_t hi, int terms) {
  const HmMod &m = ((Emu *)h)->P.modc[mod];
  const hm_u128 z = ((hm_u128)hi << 64) | lo;
  return terms <= 16 ? hm_redc_wide<16>(z, m) : hm_redc_wide<32>(z, m);
}
void emu_bfly(void *h, uint32_t mod, int kind, uint64_t *X, uint64_t *Y, uint64_t w) {   // kind 0..2: forward; 3: inverse
  const uint64_t q = ((Emu *)h)->P.mod[mod];
  const HmBflyMod m = hm_bfly_mod(q);
  const HmW wt = hm_tw_entry(w, q);
  if (kind == 0) hm_bfly_fwd_k<0>(*X, *Y, wt, m);
  else if (kind == 1) hm_bfly_fwd_k<1>(*X, *Y, wt, m);
  else if (kind == 2) hm_bfly_fwd_k<2>(*X, *Y, wt, m);
  else hm_bfly_inv(*X, *Y, wt, m);
}
// ---- K5 in its three forms on host arrays of limb-polys, arguments as the entry points' (include/homulator_hip.h); the records come from the
// back-end's own builder (hm_ip_fill_recs).  Returns 1 for counts outside the kernels' range
int emu_ip(void *h, const uint64_t *x, const uint32_t *xl, const uint64_t *y, const uint32_t *yl, uint64_t *out, const uint32_t *ol, const uint32_t *mod_ids,
           uint32_t n, uint32_t T, uint32_t K, uint32_t x_galois) {
  Emu &e = *(Emu *)h;
  if (!ip_counts_ok(T, K, HM_IP_MAX_OUT) || n > HM_IP_MAX_LIMBS) return 1;
  HmIpArgs a;
  a.x = x; a.y = y; a.out = out; a.mods = e.P.modc.data(); a.logN = e.P.logN; a.n_limbs = n; a.n_terms = T; a.n_out = K; a.x_galois = x_galois;
  hm_ip_fill_recs(a.limb, xl, yl, ol, (size_t)n * K, mod_ids, n, T, K, 1);
  switch (T * 10 + K) {
#define HM_CASE(t) case t * 10 + 1: run_ip(a, hm_ip_thread<t, 1>); break; case t * 10 + 2: run_ip(a, hm_ip_thread<t, 2>); break;
    HM_CASE(1) HM_CASE(2) HM_CASE(3) HM_CASE(4)
#undef HM_CASE
  }
  return 0;
}
int emu_ip_hoisted(void *h, const uint64_t *x, const uint32_t *xl, const uint64_t *y, const uint32_t *yl, uint64_t *out, const uint32_t *ol,
                   const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t R, const uint32_t *galois) {
  Emu &e = *(Emu *)h;
  if (!ip_counts_ok(T, R, HM_IP_HOISTED_MAX_ROT)) return 1;
  std::vector<HmIpHoistRec> recs((size_t)R * n);
  hm_ip_fill_recs(recs.data(), xl, yl, ol, (size_t)R * n * 2, mod_ids, n, T, 2, R);
  HmIpHoistArgs a;
  a.x = x; a.y = y; a.out = out; a.mods = e.P.modc.data(); a.rec = recs.data(); a.logN = e.P.logN; a.n_limbs = n; a.n_rot = R;
  for (uint32_t r = 0; r < HM_IP_HOISTED_MAX_ROT; ++r) a.dst_galois[r] = hm_auto_inv(r < R ? galois[r] : 1u, a.logN);
  switch (T) {
#define HM_CASE(t) case t: run_ip(a, hm_ip_hoisted_thread<t>); break;
    HM_CASE(1) HM_CASE(2) HM_CASE(3) HM_CASE(4)
#undef HM_CASE
  }
  return 0;
}
// al == NULL: no entry has an addend
int emu_ip_lintrans(void *h, const uint64_t *x, const uint32_t *xl, const uint64_t *y, const uint32_t *yl, const uint64_t *pt, const uint32_t *pl,
                    const uint64_t *addend, const uint32_t *al, uint64_t *out, const uint32_t *ol, uint64_t *addend_out, const uint32_t *aol,
                    const uint32_t *mod_ids, uint32_t n, uint32_t T, uint32_t R, const uint32_t *galois) {
  Emu &e = *(Emu *)h;
  if (!ip_counts_ok(T, R, HM_IP_LINTRANS_MAX_ROT)) return 1;
  std::vector<HmIpLinRec> recs((size_t)R * n);
  hm_ip_fill_recs(recs.data(), xl, yl, ol, (size_t)n * 2, mod_ids, n, T, 2, R);
  hm_ip_fill_lin(recs.data(), pl, al, aol, n, R);
  HmIpLinArgs a;
  a.x = x; a.y = y; a.pt = pt; a.addend = addend; a.out = out; a.addend_out = addend_out;
  a.mods = e.P.modc.data(); a.rec = recs.data(); a.logN = e.P.logN; a.n_limbs = n; a.n_rot = R;
  for (uint32_t r = 0; r < HM_IP_LINTRANS_MAX_ROT; ++r) a.galois[r] = r < R ? galois[r] : 1u;
  switch (T) {
#define HM_CASE(t) case t: run_ip(a, hm_ip_lintrans_thread<t>); break;
    HM_CASE(1) HM_CASE(2) HM_CASE(3) HM_CASE(4)
#undef HM_CASE
  }
  return 0;
}
uint32_t emu_auto_inv(uint32_t g, uint32_t logN) { return hm_auto_inv(g, logN); }
// ---- the back-end's launch layouts (hm_launch.h) as its entry points compute them.  policy 0: a transform (ntt_common; one_launch = the call runs
// as ONE launch), 1: the last pass x key product (hm_ntt_inner_product; weight = per limb-poly cost for its heaviest-first order, or NULL).
// Writes logG, per limb-poly its launch and slot, per launch its entry count (up to max_launch); returns the number of launches
uint32_t emu_launch_layout(int policy, int one_launch, uint32_t entry_cap, const uint32_t *mod_ids, uint32_t n, const uint32_t *weight, uint32_t *logG,
                           uint32_t *launch_of, uint32_t *slot_of, uint32_t *entries_of, uint32_t max_launch) {
  std::vector<uint32_t> all(n);
  for (uint32_t i = 0; i < n; ++i) all[i] = i;
  HmGrouping g = hm_group_by_modulus(mod_ids, all, policy == 0 ? hm_ntt_group_policy(one_launch != 0) : hm_nip_group_policy());
  if (weight) hm_sort_groups_heaviest_first(g.groups, [&](uint32_t i) { return weight[i]; });
  const uint32_t G = 1u << g.logG, nGroups = (uint32_t)g.groups.size();
  const HmLaunchSplit parts = hm_launch_split(nGroups, entry_cap, G);
  uint32_t launch = 0;
  for (uint32_t base = 0; base < nGroups; base += parts.perLaunch, ++launch) {
    const uint32_t ng = hm_launch_groups(parts, nGroups, base);
    if (launch < max_launch) entries_of[launch] = hm_launch_entries(ng, G);
    for (uint32_t kk = 0; kk < ng; ++kk)
      for (uint32_t which = 0; which < G; ++which)
        if (g.groups[base + kk][which] >= 0) {
          launch_of[g.groups[base + kk][which]] = launch;
          slot_of[g.groups[base + kk][which]] = hm_entry_slot(kk, which, G);
        }
  }
  *logG = g.logG;
  return launch;
}
// ---- the conversion's launch plans (hm_bconv_plan.h) as its entry points compute them.  Per descriptor: its launch and its place among the launch's
// members; per launch (up to max_launch): a row of `info`; returns the number of launches.
// stand-alone (hm_bconv_batch): info row = {n_in, chunk, grid x, grid y, grid z}
uint32_t emu_bconv_plan(const uint32_t *n_in, const uint32_t *n_out, uint32_t n_desc, uint32_t log_len, uint32_t bconv_blocks, uint32_t *launch_of,
                        uint32_t *place_of, uint32_t *info, uint32_t max_launch) {
  std::vector<HmBconvShape> d(n_desc);
  for (uint32_t i = 0; i < n_desc; ++i) d[i] = HmBconvShape{n_in[i], n_out[i], false};
  const std::vector<HmBconvLaunch> ls = hm_bconv_plan(d.data(), n_desc, log_len, bconv_blocks);
  for (uint32_t k = 0; k < ls.size(); ++k) {
    for (uint32_t j = 0; j < ls[k].members.size(); ++j) { launch_of[ls[k].members[j]] = k; place_of[ls[k].members[j]] = j; }
    const uint32_t row[5] = {ls[k].n_in, ls[k].chunk, ls[k].grid[0], ls[k].grid[1], ls[k].grid[2]};
    if (k < max_launch) memcpy(info + 5 * k, row, sizeof row);
  }
  return (uint32_t)ls.size();
}
// fused conversion + first pass (bconv_col_launch): outs / merge = the options bconv_col_outs / bconv_col_merge; writes NOUT and per descriptor its
// kernel width; info row = {kernel key (width, + 256 packed), output groups, grid, logTiles}
uint32_t emu_bcol_plan(const uint32_t *n_in, const uint32_t *n_out, const uint8_t *packed, uint32_t n_desc, uint32_t n_tiles, uint32_t outs, int merge, int mix,
                       uint32_t *nout, uint32_t *kn, uint32_t *launch_of, uint32_t *place_of, uint32_t *info, uint32_t max_launch) {
  std::vector<HmBconvShape> d(n_desc);
  for (uint32_t i = 0; i < n_desc; ++i) d[i] = HmBconvShape{n_in[i], n_out[i], packed[i] != 0};
  const HmBcolPlan plan = hm_bcol_plan(d.data(), n_desc, n_tiles, outs, merge != 0, mix != 0);
  *nout = plan.NOUT;
  for (uint32_t i = 0; i < n_desc; ++i) kn[i] = plan.kn[i];
  for (uint32_t k = 0; k < plan.launches.size(); ++k) {
    const HmBcolLaunch &l = plan.launches[k];
    for (uint32_t j = 0; j < l.members.size(); ++j) { launch_of[l.members[j]] = k; place_of[l.members[j]] = j; }
    const uint32_t row[4] = {l.key, l.groups, l.grid, l.logTiles};
    if (k < max_launch) memcpy(info + 4 * k, row, sizeof row);
  }
  return (uint32_t)plan.launches.size();
}
// the kernel's block map (hm_bcol_block) over a whole grid: out[3 b ..] = {conversion, tile, output group} of block b
void emu_bcol_blocks(uint32_t grid, uint32_t groups, uint32_t tile0, uint32_t log_tiles, uint32_t *out) {
  for (uint32_t b = 0; b < grid; ++b) {
    const HmBcolBlock k = hm_bcol_block(b, groups, tile0, log_tiles);
    out[3 * b] = k.pi; out[3 * b + 1] = k.tile; out[3 * b + 2] = k.og;
  }
}
// the input window of a fused conversion (hm_bcol_window): returns fits; base limb, and per kernel input its limb and byte offset
int emu_bcol_window(const uint32_t *in_limbs, uint32_t n_in, uint32_t kn, uint32_t logN, uint32_t *base, uint32_t *limb, uint32_t *off) {
  const HmBcolWindow w = hm_bcol_window(in_limbs, n_in, kn, logN);
  *base = w.base;
  memcpy(limb, w.limb, 4 * kn);
  memcpy(off, w.off, 4 * kn);
  return w.fits;
}
int emu_tile_range_ok(uint32_t tile0, uint32_t n_tiles, uint32_t all_tiles) { return hm_tile_range_ok(tile0, n_tiles, all_tiles); }
// the alias test of the entry points: the first entry of (ib, il) among those with pick[i] != 0 (NULL: all) that shares an address with (ob, ol); -1: none
int64_t emu_first_overlap(uint64_t ob, const uint32_t *ol, uint32_t no, uint64_t ib, const uint32_t *il, uint32_t ni, uint32_t N, const uint8_t *pick) {
  return hm_first_overlap(reinterpret_cast<const void *>(ob), ol, no, reinterpret_cast<const void *>(ib), il, ni, N, [&](uint32_t i) { return !pick || pick[i]; });
}
int emu_row_lds_word(int ept, int R, int tid, int a, int inverse) {
  if (ept == 16) return R == 0 ? row_unit16<0>(tid, a, inverse) : R == 1 ? row_unit16<1>(tid, a, inverse) : row_unit16<2>(tid, a, inverse);
  return R == 0 ? row_unit8<0>(tid, a, inverse) : R == 1 ? row_unit8<1>(tid, a, inverse) : R == 2 ? row_unit8<2>(tid, a, inverse) : row_unit8<3>(tid, a, inverse);
}
}
