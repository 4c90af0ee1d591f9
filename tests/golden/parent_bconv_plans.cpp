// The base conversion's launch plans of commit e00f8c34375caf07d0846f6b5e49940735c6a3a9 (the parent of the change that moved this arithmetic into
// homulator_amd/csrc/hm_bconv_plan.h): the planning loops of hm_bconv_batch and of bconv_col_launch in that commit's homulator_amd/csrc/hm_backend.hip
// (lines 2004-2040, 2061-2091, 2135 and 2160-2177), VERBATIM between the "parent text" marks, with the lines that fill device records, check arguments
// and launch replaced by RECORD_* / stand-in records.  The stand-ins above the marks give the text the names it reads (c, descs, probs, mix, n_tiles).
// Compiled and run by make_bconv_launch_plans.py to record tests/golden/bconv_launch_plans.json; no test and no library builds this file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#define HM_BCONV_MAX_IN 32      // hm_elem_core.h of that commit
#define HM_BCONV_MAX_PROB 256
#define HM_BCONV_CHUNK 8
#define HM_BCONV_THREADS 256
#define HM_BCONV_CPT 2
#define HM_BCOL_ONE_GROUP 15    // hm_bcol.h of that commit
typedef int hm_status;
#define HM_OK 0
struct Ctx { uint32_t bcol_outs, bcol_merge, bconv_blocks; };
struct hm_bconv_desc { uint32_t n_in, n_out, in_packed; };
struct Prob { uint32_t n_in, n_out, index; };   // what the plans read of HmBconvProb / HmBcolProb, and the descriptor it was made from
typedef Prob HmBconvProb;
typedef Prob HmBcolProb;
struct dim3 { uint32_t x, y, z; dim3(uint32_t x_, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {} };
struct HmBconvArgs { uint32_t logN, n_prob, chunk; };

extern "C" uint32_t parent_bconv_plan(const uint32_t *n_in_of, const uint32_t *n_out_of, uint32_t n_desc, uint32_t logN, uint32_t bconv_blocks,
                                      uint32_t *launch_of, uint32_t *place_of, uint32_t *info, uint32_t max_launch) {
  Ctx cc = {0, 0, bconv_blocks}, *c = &cc;
  std::vector<HmBconvProb> probs(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) probs[pi] = Prob{n_in_of[pi], n_out_of[pi], pi};
  uint32_t n_launch = 0;
#define RECORD_BCONV_LAUNCH() do { \
    for (uint32_t j = 0; j < grp.size(); ++j) { launch_of[grp[j].index] = n_launch; place_of[grp[j].index] = j; } \
    const uint32_t row[5] = {n_in, a.chunk, grid.x, grid.y, grid.z}; \
    if (n_launch < max_launch) memcpy(info + 5 * n_launch, row, sizeof row); \
    ++n_launch; } while (0)
  // ---- parent text: hm_bconv_batch
  // one launch per distinct input-basis size (the digits of a ModUp differ only in the last, shorter digit), up to
  // HM_BCONV_MAX_PROB problems each; the problem records go into a device table cached by content (plans repeat)
  std::vector<char> done(n_desc, 0);
  for (uint32_t first = 0; first < n_desc; ++first) {
    if (done[first]) continue;
    const uint32_t n_in = probs[first].n_in;
    std::vector<HmBconvProb> grp;
    uint32_t max_out = 0;
    auto launch = [&]() -> hm_status {
      HmBconvArgs a;
      a.logN = logN; a.n_prob = (uint32_t)grp.size();
      // output limbs per block: a block re-reads its N_IN input limbs for every chunk, so the chunk should be as large
      // as the launch allows while leaving >= ~4 rounds of blocks for the chip (3 blocks of 256 threads per CU)
      const uint32_t xb = std::max(1u, (1u << logN) / (HM_BCONV_THREADS * HM_BCONV_CPT));
      const uint32_t want = c->bconv_blocks;
      uint32_t nchunk = std::max<uint32_t>(1, (want + xb * a.n_prob - 1) / (xb * a.n_prob));
      nchunk = std::min(nchunk, (max_out + HM_BCONV_CHUNK / 2 - 1) / std::max(1, HM_BCONV_CHUNK / 2));  // chunks of >= 4 outputs
      nchunk = std::max<uint32_t>(1, nchunk);
      a.chunk = (max_out + nchunk - 1) / nchunk;
      dim3 grid(xb, (max_out + a.chunk - 1) / a.chunk, a.n_prob);
      RECORD_BCONV_LAUNCH();   // (the parent uploads the records and launches k_bconv_by_n_in[n_in] here)
      grp.clear(); max_out = 0;
      return HM_OK;
    };
    for (uint32_t pi = first; pi < n_desc; ++pi) {
      if (done[pi] || probs[pi].n_in != n_in) continue;
      done[pi] = 1;
      grp.push_back(probs[pi]);
      max_out = std::max(max_out, probs[pi].n_out);
      if (grp.size() == HM_BCONV_MAX_PROB) { hm_status st = launch(); if (st) return st; }
    }
    if (!grp.empty()) { hm_status st = launch(); if (st) return st; }
  }
  // ---- end of parent text
  return n_launch;
}

extern "C" uint32_t parent_bcol_plan(const uint32_t *n_in_of, const uint32_t *n_out_of, const uint8_t *packed_of, uint32_t n_desc, uint32_t n_tiles, uint32_t outs,
                                     int merge_opt, int with_mix, uint32_t *nout, uint32_t *kn_of, uint32_t *launch_of, uint32_t *place_of, uint32_t *info,
                                     uint32_t max_launch) {
  Ctx cc = {outs, (uint32_t)(merge_opt != 0), 0}, *c = &cc;
  std::vector<hm_bconv_desc> dv(n_desc);
  for (uint32_t pi = 0; pi < n_desc; ++pi) dv[pi] = hm_bconv_desc{n_in_of[pi], n_out_of[pi], packed_of[pi]};
  const hm_bconv_desc *descs = dv.data();
  const int mixStandIn = 0, *mix = with_mix ? &mixStandIn : nullptr;
  // ---- parent text: bconv_col_launch, the plan
  uint32_t NOUT = c->bcol_outs;
  size_t wgsAll = 0;
  bool widths[2][HM_BCONV_MAX_IN + 1] = {};
  uint32_t nWidths = 0;
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    wgsAll += (size_t)descs[pi].n_out * n_tiles;
    bool &w = widths[descs[pi].in_packed ? 1 : 0][std::min<uint32_t>(descs[pi].n_in, HM_BCONV_MAX_IN)];
    nWidths += !w;
    w = true;
  }
  const bool mayMerge = c->bcol_merge && !mix && wgsAll <= 4096 && nWidths > 1;
  if (!NOUT) NOUT = wgsAll > 4096 || mayMerge ? 2 : 1;
  std::map<uint32_t, std::vector<HmBcolProb>> byIn;   // key: n_in, + 256 for conversions whose inputs are stored packed (kernels of their own)
  std::vector<uint32_t> kernelNin(n_desc);
  {
    uint32_t widest[2] = {0, 0};
    for (uint32_t pi = 0; pi < n_desc; ++pi) widest[descs[pi].in_packed ? 1 : 0] = std::max(widest[descs[pi].in_packed ? 1 : 0], descs[pi].n_in);
    const bool merge = mayMerge;
    for (uint32_t pi = 0; pi < n_desc; ++pi) {
      const uint32_t w = widest[descs[pi].in_packed ? 1 : 0];
      // (a digit runs the widest digit's kernel only inside one family: up to 15 limbs, or two input groups; and not for more than four times its own work)
      kernelNin[pi] = merge && (w <= HM_BCOL_ONE_GROUP || descs[pi].n_in > HM_BCOL_ONE_GROUP) && w <= 4 * descs[pi].n_in ? w : descs[pi].n_in;
    }
  }
  for (uint32_t pi = 0; pi < n_desc; ++pi) {
    const hm_bconv_desc &d = descs[pi];
    const uint32_t kn = kernelNin[pi];   // the input-basis size of the kernel this conversion runs (>= d.n_in)
    HmBcolProb p = Prob{d.n_in, d.n_out, pi};   // (the parent checks the descriptor and fills its record here)
    byIn[kn + (d.in_packed ? 256u : 0u)].push_back(p);
  }
  struct Lnch { uint32_t n_in; dim3 grid; uint32_t groups, logTiles; };   // (the parent: the launch's HmBcolArgs in place of the last two)
  std::vector<Lnch> ls;
  for (auto &kv : byIn) {
    auto &grp = kv.second;
    uint32_t max_out = 0;
    for (auto &p : grp) max_out = std::max(max_out, p.n_out);
    const uint32_t groups = (max_out + NOUT - 1) / NOUT;   // output groups per (conversion, tile)
    uint32_t logTiles = 0;
    while ((1u << logTiles) < n_tiles) ++logTiles;
    const uint32_t pairs = ((uint32_t)grp.size() * n_tiles + 7) / 8 * 8;
    ls.push_back(Lnch{kv.first, dim3(pairs * groups), groups, logTiles});
    for (uint32_t j = 0; j < grp.size(); ++j) { launch_of[grp[j].index] = (uint32_t)ls.size() - 1; place_of[grp[j].index] = j; }   // (RECORD)
  }
  // ---- end of parent text
  *nout = NOUT;
  for (uint32_t pi = 0; pi < n_desc; ++pi) kn_of[pi] = kernelNin[pi];
  for (uint32_t k = 0; k < ls.size() && k < max_launch; ++k) {
    const uint32_t row[4] = {ls[k].n_in, ls[k].groups, ls[k].grid.x, ls[k].logTiles};
    memcpy(info + 4 * k, row, sizeof row);
  }
  return (uint32_t)ls.size();
}
