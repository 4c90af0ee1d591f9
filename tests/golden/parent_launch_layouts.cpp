// The launch layouts of commit 9ac0d5eb11dc9ca3493f7cd963a7eb1a923b80a5 (the parent of the change that moved this arithmetic into
// homulator_amd/csrc/hm_launch.h): the grouping / split / slot loops of ntt_common and of hm_ntt_inner_product in that commit's
// homulator_amd/csrc/hm_backend.hip (lines 1356-1403 and 1930-1987), VERBATIM between the "parent text" marks, with the lines that fill device records
// replaced by RECORD_LAUNCH / RECORD_SLOT.  The stand-ins above the marks give the text the names it reads (c, f, d, n, mod_ids, T, K, st).
// Compiled and run by make_launch_layouts.py to record tests/golden/launch_layouts.json; no test and no library builds this file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#define HM_NTT_MAX_ENTRIES 448   // hm_ntt_core.h of that commit
#define HM_NIP_MAX_LIMBS 4096    // hm_backend.hip of that commit
struct Ctx { uint32_t fused_small, ntt_launch_entries; };
static uint32_t fused_small_entries(const Ctx *c) { return c->fused_small; }   // (the parent scales the option by the ring size first)
struct Flags { bool firstPassOnly, secondPassOnly; };
struct Desc { const uint32_t *mod_ids; const uint8_t *x_is_coeff, *out_inverse; };
#define RECORD_LAUNCH(cnt) do { if (launch < max_launch) entries_of[launch] = (cnt); } while (0)
#define RECORD_SLOT(i, e) do { launch_of[i] = launch; slot_of[i] = (e); } while (0)

extern "C" uint32_t parent_ntt_layout(uint32_t fused_small, uint32_t ntt_launch_entries, const uint32_t *mod_ids, uint32_t n, uint32_t *logG_out,
                                      uint32_t *launch_of, uint32_t *slot_of, uint32_t *entries_of, uint32_t max_launch) {
  Ctx cc = {fused_small, ntt_launch_entries}, *c = &cc;
  const Flags f = {false, false};
  uint32_t launch = 0;
  // ---- parent text: ntt_common
  std::map<uint32_t, std::vector<int>> byMod;
  for (uint32_t i = 0; i < n; ++i) byMod[mod_ids[i]].push_back((int)i);
  uint32_t logG = 1;
  // a call that will run as ONE launch (k_ntt_fused8) takes single limb-polys as groups: a kernel then has at most 15 workgroups per XCD
  // waiting for siblings that have no slot yet (launch_ntt), and the 50-limb sweep 56 entries instead of 64
  if (fused_small_entries(c) && !f.firstPassOnly && !f.secondPassOnly && (n + 7) / 8 * 8 <= fused_small_entries(c)) logG = 0;
#ifndef HM_NTT_MAX_LOGG
#define HM_NTT_MAX_LOGG 3
#endif
  for (uint32_t lg = HM_NTT_MAX_LOGG; lg >= 2; --lg) {
    size_t full = 0;
    for (auto &kv : byMod) full += kv.second.size() >> lg << lg;
    if (full * 8 >= (size_t)n * 7 && n >= (64u << lg)) { logG = lg; break; }
  }
  const uint32_t G = 1u << logG;
  std::vector<std::vector<int>> groups;  // indices into the caller's lists, -1 = empty
  {
    std::vector<int> rest;
    for (auto &kv : byMod) {
      auto &v = kv.second;
      size_t i = 0;
      for (; i + G <= v.size(); i += G) groups.emplace_back(v.begin() + i, v.begin() + i + G);
      rest.insert(rest.end(), v.begin() + i, v.end());   // leftovers of one modulus stay adjacent: they still share among themselves
    }
    for (size_t i = 0; i < rest.size(); i += G) {
      std::vector<int> g(rest.begin() + i, rest.begin() + std::min(rest.size(), i + G));
      g.resize(G, -1);
      groups.push_back(g);
    }
  }
  // As few launches as the kernel-argument segment allows (HM_NTT_MAX_ENTRIES records), of equal size; the constants
  // of a launch live in a device table cached by content (plans repeat their launches)
  // whole blocks of 8 groups (one per XCD)
  const uint32_t maxGroups = std::max(8u, std::min<uint32_t>(HM_NTT_MAX_ENTRIES, c->ntt_launch_entries) / G / 8 * 8);
  const uint32_t nLaunch = ((uint32_t)groups.size() + maxGroups - 1) / maxGroups;
  const uint32_t perLaunch = nLaunch ? (((uint32_t)groups.size() + nLaunch - 1) / nLaunch + 7) / 8 * 8 : 0;
  for (uint32_t base = 0; base < groups.size(); base += perLaunch) {
    const uint32_t ng = std::min<uint32_t>(perLaunch, (uint32_t)groups.size() - base);
    const uint32_t cnt = ((ng + 7) / 8) * 8 * G;  // entries: blocks of 8 groups = 8G entries
    RECORD_LAUNCH(cnt);   // (the parent fills the launch's records here)
    for (uint32_t kk = 0; kk < ng; ++kk) {
      for (uint32_t which = 0; which < G; ++which) {
        const int gi = groups[base + kk][which];
        if (gi < 0) continue;
        const uint32_t g = (uint32_t)gi, e = (kk / 8) * 8 * G + which * 8 + (kk % 8), m = mod_ids[g];
        RECORD_SLOT(g, e); (void)m;
      }
    }
    ++launch;
  }
  // ---- end of parent text
  *logG_out = logG;
  return launch;
}

extern "C" uint32_t parent_nip_layout(const uint32_t *mod_ids, uint32_t n, const uint8_t *x_is_coeff, const uint8_t *out_inverse, uint32_t *logG_out,
                                      uint32_t *launch_of, uint32_t *slot_of, uint32_t *entries_of, uint32_t max_launch) {
  const Desc dd = {mod_ids, x_is_coeff, out_inverse}, *d = &dd;
  const uint32_t T = 1, K = 1;   // one digit, one key: a limb-poly weighs 1 or 3 (its digit goes through the transform), + 2 with out_inverse
  auto inSet = [](uint32_t) { return true; };
  uint32_t launch = 0;
  // ---- parent text: hm_ntt_inner_product
  std::map<uint32_t, std::vector<uint32_t>> byMod;
  uint32_t nSet = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (inSet(i)) { byMod[d->mod_ids[i]].push_back(i); ++nSet; }
  if (!nSet) { *logG_out = 0; return 0; }   // (the parent: `continue` with the next set)
  uint32_t logG = 0;
  for (uint32_t lg = 3; lg >= 1; --lg) {
    size_t full = 0;
    for (auto &kv : byMod) full += kv.second.size() >> lg << lg;
    if (full * 8 >= (size_t)nSet * 7 && nSet >= (8u << lg)) { logG = lg; break; }
  }
  const uint32_t G = 1u << logG;
  std::vector<std::vector<int>> groups;
  {
    std::vector<int> rest;
    for (auto &kv : byMod) {
      auto &v = kv.second;
      size_t i = 0;
      for (; i + G <= v.size(); i += G) groups.emplace_back(v.begin() + i, v.begin() + i + G);
      rest.insert(rest.end(), v.begin() + i, v.end());
    }
    for (size_t i = 0; i < rest.size(); i += G) {
      std::vector<int> g(rest.begin() + i, rest.begin() + std::min(rest.size(), i + G));
      g.resize(G, -1);
      groups.push_back(g);
    }
  }
  // longest first: a limb whose digits all go through the transform (the special limbs of a ModUp: beta transforms) costs more than one
  // with a digit of its own; workgroups are dispatched in entry order, so the heavy ones start first and the partly filled last round of a
  // small launch holds light ones
  {
    auto weight = [&](const std::vector<int> &g) {
      uint32_t w = 0;
      for (int gi : g)
        if (gi >= 0)
          {
            for (uint32_t j = 0; j < T; ++j) w += d->x_is_coeff[(uint32_t)gi * T + j] ? 3 : 1;
            if (d->out_inverse && d->out_inverse[gi]) w += 2 * K;   // ... and an inverse first pass per output on top
          }
      return w;
    };
    std::stable_sort(groups.begin(), groups.end(), [&](const std::vector<int> &a, const std::vector<int> &b) { return weight(a) > weight(b); });
  }
  const uint32_t maxGroups = HM_NIP_MAX_LIMBS / G / 8 * 8;
  const uint32_t nLaunch = ((uint32_t)groups.size() + maxGroups - 1) / maxGroups;
  const uint32_t perLaunch = nLaunch ? (((uint32_t)groups.size() + nLaunch - 1) / nLaunch + 7) / 8 * 8 : 0;
  for (uint32_t base = 0; base < groups.size(); base += perLaunch) {
    const uint32_t ng = std::min<uint32_t>(perLaunch, (uint32_t)groups.size() - base);
    const uint32_t cnt = ((ng + 7) / 8) * 8 * G;
    RECORD_LAUNCH(cnt);   // (the parent fills the launch's records here)
    for (uint32_t kk = 0; kk < ng; ++kk)
      for (uint32_t which = 0; which < G; ++which) {
        const int gi = groups[base + kk][which];
        if (gi < 0) continue;
        const uint32_t i = (uint32_t)gi, e = (kk / 8) * 8 * G + which * 8 + (kk % 8);
        RECORD_SLOT(i, e);
      }
    ++launch;
  }
  // ---- end of parent text
  *logG_out = logG;
  return launch;
}
