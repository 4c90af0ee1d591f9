// Launch-layout arithmetic of the back-end's entry points: which slot of a launch a limb-poly takes, how limb-polys that share a modulus
// are grouped, how groups are split over launches, and whether two limb lists name the same memory.  Host-only, plain C++17 (no HIP
// include): the back-end (hm_backend.hip) and the CPU emulator (tests/emu) compile the same text.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

static inline uint32_t limb_at(const uint32_t *l, uint32_t i) { return l ? l[i] : i; }   // a NULL limb list is the identity

// The slot (entry of the launch's records) of member `which` of the launch's kk-th group of G = 2^logG limb-polys, as hm_block_map expects it:
// a launch is a sequence of blocks of 8 groups (8 G slots), one group per XCD; group kk is column kk % 8 of block kk / 8 and its members sit
// 8 slots apart, so they run on ONE XCD and share its L2 for the twiddles / keys of their modulus.
static inline uint32_t hm_entry_slot(uint32_t kk, uint32_t which, uint32_t G) { return (kk / 8) * 8 * G + which * 8 + (kk % 8); }

// Same-modulus grouping.  logG = the largest lg in [minLogG, maxLogG] for which at least 7 of 8 limb-polys fall into full same-modulus groups
// of 2^lg and the call has at least sizeUnit << lg limb-polys; defaultLogG when none qualifies (a transform that runs as ONE launch passes 0).
struct HmGroupPolicy {
  uint32_t defaultLogG, minLogG, maxLogG, sizeUnit;
};
#ifndef HM_NTT_MAX_LOGG
#define HM_NTT_MAX_LOGG 3   // a transform's groups hold up to 2^3 limb-polys
#endif
// The two policies in use.  A transform (ntt_common): pairs (single limb-polys if the call runs as ONE launch) unless a call of 64 G or more
// limb-polys fills groups of G = 4 or 8.  The last pass x key product (hm_ntt_inner_product): single limb-polys unless 8 G or more fill G = 2, 4, 8.
static inline HmGroupPolicy hm_ntt_group_policy(bool oneLaunch) { return HmGroupPolicy{oneLaunch ? 0u : 1u, 2, HM_NTT_MAX_LOGG, 64}; }
static inline HmGroupPolicy hm_nip_group_policy() { return HmGroupPolicy{0, 1, 3, 8}; }
struct HmGrouping {
  uint32_t logG = 0;
  std::vector<std::vector<int>> groups;   // 2^logG indices into the caller's lists each, -1 = empty
};
// `members`: indices into mod_ids.  Full groups first, by ascending modulus; leftovers of a modulus stay adjacent and fill the last groups
static inline HmGrouping hm_group_by_modulus(const uint32_t *mod_ids, const std::vector<uint32_t> &members, const HmGroupPolicy &p) {
  std::map<uint32_t, std::vector<int>> byMod;
  for (uint32_t i : members) byMod[mod_ids[i]].push_back((int)i);
  const size_t n = members.size();
  HmGrouping r;
  r.logG = p.defaultLogG;
  for (uint32_t lg = p.maxLogG; lg >= p.minLogG && lg > 0; --lg) {
    size_t full = 0;
    for (auto &kv : byMod) full += kv.second.size() >> lg << lg;
    if (full * 8 >= n * 7 && n >= ((size_t)p.sizeUnit << lg)) { r.logG = lg; break; }
  }
  const size_t G = (size_t)1 << r.logG;
  std::vector<int> rest;
  for (auto &kv : byMod) {
    auto &v = kv.second;
    size_t i = 0;
    for (; i + G <= v.size(); i += G) r.groups.emplace_back(v.begin() + i, v.begin() + i + G);
    rest.insert(rest.end(), v.begin() + i, v.end());
  }
  for (size_t i = 0; i < rest.size(); i += G) {
    std::vector<int> g(rest.begin() + i, rest.begin() + std::min(rest.size(), i + G));
    g.resize(G, -1);
    r.groups.push_back(g);
  }
  return r;
}
// heaviest group first (stable; workgroups are dispatched in slot order).  weight(i) = the cost of limb-poly i
template <class Weight>
static inline void hm_sort_groups_heaviest_first(std::vector<std::vector<int>> &groups, Weight weight) {
  auto of = [&](const std::vector<int> &g) {
    uint32_t w = 0;
    for (int gi : g)
      if (gi >= 0) w += weight((uint32_t)gi);
    return w;
  };
  std::stable_sort(groups.begin(), groups.end(), [&](const std::vector<int> &a, const std::vector<int> &b) { return of(a) > of(b); });
}

// As few launches as the cap on a launch's entries allows, of equal size, in whole blocks of 8 groups (launch k starts at group k * perLaunch)
struct HmLaunchSplit {
  uint32_t maxGroups, nLaunch, perLaunch;
};
static inline HmLaunchSplit hm_launch_split(uint32_t nGroups, uint32_t entryCap, uint32_t G) {
  HmLaunchSplit s;
  s.maxGroups = std::max(8u, entryCap / G / 8 * 8);
  s.nLaunch = (nGroups + s.maxGroups - 1) / s.maxGroups;
  s.perLaunch = s.nLaunch ? ((nGroups + s.nLaunch - 1) / s.nLaunch + 7) / 8 * 8 : 0;
  return s;
}
static inline uint32_t hm_launch_groups(const HmLaunchSplit &s, uint32_t nGroups, uint32_t base) { return std::min(s.perLaunch, nGroups - base); }
static inline uint32_t hm_launch_entries(uint32_t ng, uint32_t G) { return (ng + 7) / 8 * 8 * G; }

// The alias test of every entry point that reads an operand at OTHER positions than the ones its workgroups write (through an automorphism, or
// scattered): the index of the first entry i of (ib, il[0..ni)) that pick(i) admits and whose limb-poly shares an address with a limb-poly of
// (ob, ol[0..no)), or -1.  Limb-polys are compared as address RANGES (base + limb * N words of 8 bytes), not by base pointer and limb number:
// different pointers into one allocation are caught, whole limb-polys apart or a fraction of one (which then touches two).
template <class Pick>
static inline int64_t hm_first_overlap(const void *ob, const uint32_t *ol, uint32_t no, const void *ib, const uint32_t *il, uint32_t ni, uint32_t N,
                                       Pick pick) {
  std::vector<int64_t> written(no);
  for (uint32_t i = 0; i < no; ++i) written[i] = limb_at(ol, i);
  std::sort(written.begin(), written.end());
  const int64_t lb = (int64_t)N * 8, base = (int64_t)(reinterpret_cast<intptr_t>(ib) - reinterpret_cast<intptr_t>(ob));
  for (uint32_t i = 0; i < ni; ++i) {
    if (!pick(i)) continue;
    const int64_t s = base + (int64_t)limb_at(il, i) * lb;          // bytes [s, s + lb) from the output base
    const int64_t o0 = s >= 0 ? s / lb : -((-s + lb - 1) / lb);     // output limb-polys touched: o0, and o0 + 1 unless s is aligned to one
    const int64_t o1 = o0 + (s != o0 * lb ? 1 : 0);
    auto it = std::lower_bound(written.begin(), written.end(), o0);
    if (it != written.end() && *it <= o1) return i;
  }
  return -1;
}
static inline bool hm_limbs_overlap(const void *ob, const uint32_t *ol, uint32_t no, const void *ib, const uint32_t *il, uint32_t ni, uint32_t N) {
  return hm_first_overlap(ob, ol, no, ib, il, ni, N, [](uint32_t) { return true; }) >= 0;
}
