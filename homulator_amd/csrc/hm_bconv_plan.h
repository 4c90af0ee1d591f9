// Launch plans, device tables and problem records of the base conversion's entry points (hm_bconv.inl): how the conversions of a call are
// grouped into launches and with what grids, which kernel width a conversion runs, whether its inputs fit one buffer descriptor, the words of
// its device table and the fields its two record types share.  Host-only, plain C++17 (no HIP include), like hm_launch.h: the back-end and the
// CPU emulator (tests/emu) compile the same text, and a plan is a value one can print and compare (tests/test_emu_bconv_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>
#include "hm_elem_core.h"
#include "hm_launch.h"
#include "hm_params.h"

struct HmBconvShape {   // what the plans read of a conversion (hm_bconv_desc)
  uint32_t n_in, n_out;
  bool packed;
};

// ---- the stand-alone conversion (hm_bconv_batch, k_bconv<N_IN>) ------------------------------------------------------------------------------
struct HmBconvLaunch {
  uint32_t n_in;                   // the kernel's input-basis size
  std::vector<uint32_t> members;   // indices into the call's descriptors, in order
  uint32_t chunk;                  // output limbs per block
  uint32_t grid[3];                // (coefficient blocks, output chunks, problems)
};
// output limbs per block: a block re-reads its N_IN input limbs for every chunk, so the chunk should be as large as the launch allows while
// leaving >= ~4 rounds of blocks for the chip (3 blocks of 256 threads per CU); `want` = the option bconv_blocks
static inline void hm_bconv_grid(HmBconvLaunch &l, uint32_t logN, uint32_t max_out, uint32_t want) {
  const uint32_t n_prob = (uint32_t)l.members.size();
  const uint32_t xb = std::max(1u, (1u << logN) / (HM_BCONV_THREADS * HM_BCONV_CPT));
  uint32_t nchunk = std::max<uint32_t>(1, (want + xb * n_prob - 1) / (xb * n_prob));
  nchunk = std::min(nchunk, (max_out + HM_BCONV_CHUNK / 2 - 1) / std::max(1, HM_BCONV_CHUNK / 2));  // chunks of >= 4 outputs
  nchunk = std::max<uint32_t>(1, nchunk);
  l.chunk = (max_out + nchunk - 1) / nchunk;
  l.grid[0] = xb; l.grid[1] = (max_out + l.chunk - 1) / l.chunk; l.grid[2] = n_prob;
}
// one launch per distinct input-basis size, in first-appearance order (the digits of a ModUp differ only in the last, shorter digit), up to
// HM_BCONV_MAX_PROB problems each
static inline std::vector<HmBconvLaunch> hm_bconv_plan(const HmBconvShape *d, uint32_t n_desc, uint32_t logN, uint32_t want) {
  std::vector<HmBconvLaunch> ls;
  std::vector<char> done(n_desc, 0);
  for (uint32_t first = 0; first < n_desc; ++first) {
    if (done[first]) continue;
    HmBconvLaunch l;
    l.n_in = d[first].n_in;
    uint32_t max_out = 0;
    for (uint32_t pi = first; pi < n_desc; ++pi) {
      if (done[pi] || d[pi].n_in != l.n_in) continue;
      done[pi] = 1;
      l.members.push_back(pi);
      max_out = std::max(max_out, d[pi].n_out);
      if (l.members.size() == HM_BCONV_MAX_PROB) { hm_bconv_grid(l, logN, max_out, want); ls.push_back(l); l.members.clear(); max_out = 0; }
    }
    if (!l.members.empty()) { hm_bconv_grid(l, logN, max_out, want); ls.push_back(l); }
  }
  return ls;
}

// ---- conversion + first transform pass (bconv_col_launch, k_bconv_col / k_bconv_col2 / k_bconv_col2w) -------------------------------------------
// the column tiles a call works on: a power of two of them, aligned, inside the limb-poly
static inline bool hm_tile_range_ok(uint32_t tile0, uint32_t n_tiles, uint32_t allTiles) {
  return n_tiles && !(n_tiles & (n_tiles - 1)) && tile0 % n_tiles == 0 && tile0 + n_tiles <= allTiles;
}
struct HmBcolLaunch {
  uint32_t key;                    // the kernel: its input-basis size, + 256 for conversions whose inputs are stored packed (kernels of their own)
  std::vector<uint32_t> members;   // indices into the call's descriptors, in order
  uint32_t groups;                 // output groups (of NOUT limbs) per (conversion, tile): HmBcolArgs::max_out
  uint32_t grid, logTiles;         // workgroups (hm_bcol_block maps them back to (conversion, tile, output group))
};
struct HmBcolPlan {
  uint32_t NOUT;              // output limbs per workgroup
  std::vector<uint32_t> kn;   // per descriptor: the input-basis size of the kernel it runs (>= its n_in)
  std::vector<HmBcolLaunch> launches;   // in the order they run
};
// outs / merge: the options bconv_col_outs (1 | 2; 0 = by launch size) and bconv_col_merge; mix: the call has the mix prologue.
//
// Output limbs per workgroup: two share the loaded and split inputs (+2 % hmult/s at batch 10), but halve the workgroups of a launch that
// fills the chip only once or twice (one op at a time: -2 %): by launch size unless the option says otherwise.
//
// Small launches (one op at a time, a rank's share of a sharded op): digits of different width are launches of different kernels (N_IN is a
// template parameter), one behind the other, and each leaves the chip part empty — hmult 45/35/15: 1 120 workgroups of <15> on 1 024 slots (a
// second, nearly empty round: 40.7 us) and then 720 of <5> (19.5 us).  When the whole call is small, the narrower digits run the WIDEST digit's
// kernel with zero table columns for the inputs they do not have (the padded inputs re-read the digit's first limb: exact zeros are added):
// ONE launch of 1 840 workgroups — and then with two outputs per workgroup: 920 workgroups on the chip's 1 024 slots (one round), one op at a
// time +1.3 % on top of the merge.  More multiply-adds for the narrow digit, fewer rounds for the launch.  A small call of ONE width keeps one
// output per workgroup (level since the four-wave kernels).  (Running the launches side by side on a second stream between a fork and a join
// event was measured slower: +21 us per op, profiles/README.md "side launches".)
static inline HmBcolPlan hm_bcol_plan(const HmBconvShape *d, uint32_t n_desc, uint32_t n_tiles, uint32_t outs, bool merge, bool mix) {
  HmBcolPlan r;
  size_t wgsAll = 0;
  bool widths[2][HM_BCONV_MAX_IN + 1] = {};
  uint32_t nWidths = 0, widest[2] = {0, 0};
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    wgsAll += (size_t)d[pi].n_out * n_tiles;
    const uint32_t n_in = std::min<uint32_t>(d[pi].n_in, HM_BCONV_MAX_IN);   // (a wider one is refused by the caller's checks)
    bool &w = widths[d[pi].packed ? 1 : 0][n_in];
    nWidths += !w;
    w = true;
    widest[d[pi].packed ? 1 : 0] = std::max(widest[d[pi].packed ? 1 : 0], n_in);
  }
  const bool mayMerge = merge && !mix && wgsAll <= 4096 && nWidths > 1;
  r.NOUT = outs ? outs : wgsAll > 4096 || mayMerge ? 2 : 1;
  std::map<uint32_t, HmBcolLaunch> byIn;
  r.kn.resize(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const uint32_t w = widest[d[pi].packed ? 1 : 0];
    // (a digit runs the widest digit's kernel only inside one family: up to 15 limbs, or two input groups; and not for more than four times its own work)
    r.kn[pi] = mayMerge && (w <= HM_BCOL_ONE_GROUP || d[pi].n_in > HM_BCOL_ONE_GROUP) && w <= 4 * d[pi].n_in ? w : d[pi].n_in;
    byIn[r.kn[pi] + (d[pi].packed ? 256u : 0u)].members.push_back(pi);
  }
  uint32_t logTiles = 0;
  while ((1u << logTiles) < n_tiles) ++logTiles;
  for (auto &kv : byIn) {
    HmBcolLaunch &l = kv.second;
    uint32_t max_out = 0;
    for (uint32_t pi : l.members) max_out = std::max(max_out, d[pi].n_out);
    l.key = kv.first;
    l.groups = (max_out + r.NOUT - 1) / r.NOUT;
    const uint32_t pairs = ((uint32_t)l.members.size() * n_tiles + 7) / 8 * 8;
    l.grid = pairs * l.groups;
    l.logTiles = logTiles;
    r.launches.push_back(l);
  }
  return r;
}

// The input window of a fused conversion: ONE buffer descriptor per conversion — the lowest input limb-poly is the base, the others are byte
// offsets from it (HmBcolProb::in_off); the inputs a narrow digit does not have in a kernel of width kn > n_in repeat input 0 (a valid limb-poly,
// zero table columns).  fits = false: the inputs are more than 4 GiB apart and cannot be addressed with 32-bit offsets.
struct HmBcolWindow {
  bool fits;
  uint32_t base;   // limb-poly of the descriptor's base
  uint32_t limb[HM_BCONV_MAX_IN], off[HM_BCONV_MAX_IN];   // [kn]
};
static inline HmBcolWindow hm_bcol_window(const uint32_t *in_limbs, uint32_t n_in, uint32_t kn, uint32_t logN) {
  HmBcolWindow w;
  memset(&w, 0, sizeof w);
  uint32_t hi = limb_at(in_limbs, 0);
  w.base = hi;
  for (uint32_t i = 0; i < n_in; ++i) { w.limb[i] = limb_at(in_limbs, i); w.base = std::min(w.base, w.limb[i]); hi = std::max(hi, w.limb[i]); }
  w.fits = ((uint64_t)(hi - w.base) + 1) << (logN + 3) <= (1ull << 32);
  if (!w.fits) return w;
  for (uint32_t i = 0; i < n_in; ++i) w.off[i] = (w.limb[i] - w.base) << (logN + 3);
  for (uint32_t i = n_in; i < kn; ++i) { w.limb[i] = w.limb[0]; w.off[i] = w.off[0]; }
  return w;
}

// ---- device table and records ------------------------------------------------------------------------------------------------------------------
// The words of a conversion's device table.  Format: [n_out][row], row = HM_BCONV_ROW(kn): one output's factors contiguous and padded (wide scalar
// loads), Montgomery form, split-30 packed; kn = the input-basis size of the kernel that reads it (> n_in: a narrow digit in the widest digit's
// kernel, zero columns for the inputs it does not have).  Behind the rows: {q, -q^-1} per output (HmQn)
static inline std::vector<uint64_t> hm_bconv_table_words(const hm::Params &P, const uint32_t *in_ids, uint32_t n_in, const uint32_t *out_ids, uint32_t n_out,
                                                         uint32_t kn) {
  const uint32_t row = HM_BCONV_ROW(kn);
  std::vector<uint64_t> qh(n_in), tb((size_t)n_in * n_out);
  P.bconv_consts(in_ids, n_in, out_ids, n_out, qh.data(), tb.data());
  std::vector<uint64_t> tt((size_t)row * n_out, 0);
  for (uint32_t i = 0; i < n_in; ++i)
    for (uint32_t t = 0; t < n_out; ++t) tt[(size_t)t * row + i] = hm_bconv_entry(tb[(size_t)i * n_out + t], P.modc[out_ids[t]]);
  for (uint32_t t = 0; t < n_out; ++t) { tt.push_back(P.modc[out_ids[t]].q); tt.push_back(P.modc[out_ids[t]].nqinv); }
  return tt;
}
// what HmBconvProb and HmBcolProb share (everything else zero).  table: the conversion's table for the kernel width kn, where the kernel reads it
template <class PROB>
static inline void hm_bconv_fill(PROB &p, const uint64_t *in, const uint64_t *table, uint32_t kn, const uint32_t *in_limbs, uint32_t n_in,
                                 const uint32_t *out_limbs, uint32_t n_out, bool packed) {
  memset(&p, 0, sizeof p);
  p.in = in; p.table = table; p.qn = table + (size_t)HM_BCONV_ROW(kn) * n_out;
  p.n_in = n_in; p.n_out = n_out;
  p.in_packed = packed ? 1u : 0u;
  for (uint32_t i = 0; i < n_in; ++i) p.in_limb[i] = limb_at(in_limbs, i);
  for (uint32_t t = 0; t < n_out; ++t) p.out_limb[t] = limb_at(out_limbs, t);
}
