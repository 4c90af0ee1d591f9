// hm_table_cache_main.cpp — a stand-alone program (TEST INFRASTRUCTURE) over homulator_amd/csrc/hm_table_cache.h, the launch-table cache of a
// context, instantiated with malloc / memcpy / free instead of the HIP calls.  It replays request sequences shaped like the back-end's calls: a
// call makes t = 1 .. 8 requests and every later table embeds the "device" pointers of the earlier ones (hm_bconv_batch: ep_k inside the problem
// records; the fused conversion: mixk).  After its last request the call reads every table THROUGH the embedded pointers, as the kernel it then
// launches would.  Limits 1 .. 9, the cache filled so that the limit is reached at every position within the call; then the same under a live graph,
// while capturing, and after both are gone.  tests/test_emu_table_cache.py builds it with -fsanitize=address,undefined and runs it as a process of
// its own: a table freed before its call has returned is a heap-use-after-free at the read.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../homulator_amd/csrc/hm_table_cache.h"

struct HostBackend {
  bool capture = false, fail_wait = false, waited = true;
  long live = 0, waits = 0, freed_unwaited = 0;
  int upload(const void *data, size_t bytes, void **dev) {
    void *p = malloc(bytes);
    if (!p) return 1;
    memcpy(p, data, bytes);
    *dev = p;
    ++live;
    return 0;
  }
  void release(void *dev) { if (!waited) ++freed_unwaited; free(dev); --live; }
  int wait() { ++waits; if (fail_wait) return 7; waited = true; return 0; }
  bool stream_capturing() { return capture; }
  void launch() { waited = false; }   // a kernel that reads the call's tables is now in flight
};
typedef HmTableCache<HostBackend> Cache;

#define MAX_T 8
struct Rec {   // a launch table: its own words and the device pointers of the call's earlier tables
  uint64_t tag, n_earlier;
  const Rec *earlier[MAX_T];
  uint64_t words[5];
};
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t word(uint64_t tag, int k) { return (tag + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)k * 0xD1B54A32D192ED03ull; }

// One ABI call: t requests, then the read a kernel would do.  `serial` decides the bytes (the same serial asks for the same tables again, provided
// the earlier pointers are the same).  dev[]: the pointers handed out.  Returns the status of the first refused step.
static HmTableStatus call(Cache &c, HostBackend &b, uint64_t serial, int t, const Rec **dev) {
  HmTableCall<HostBackend> span(c, b);
  if (span.st) return span.st;
  Rec host[MAX_T];
  for (int i = 0; i < t; ++i) {
    Rec &r = host[i];
    memset(&r, 0, sizeof r);
    r.tag = serial * 16 + (uint64_t)i;
    r.n_earlier = (uint64_t)i;
    for (int j = 0; j < i; ++j) r.earlier[j] = dev[j];
    for (int k = 0; k < 5; ++k) r.words[k] = word(r.tag, k);
    const void *p = nullptr;
    const HmTableStatus st = c.get(b, &r, sizeof r, &p);
    if (st) return st;
    dev[i] = static_cast<const Rec *>(p);
    const void *again = nullptr;   // a hit returns the same pointer
    CHECK(c.get(b, &r, sizeof r, &again) == HM_TABLE_OK && again == p, "serial %llu request %d: a hit moved", (unsigned long long)serial, i);
  }
  for (int i = 0; i < t; ++i) {   // what the kernel reads: the last tables, and through them the earlier ones
    CHECK(!memcmp(dev[i], &host[i], sizeof(Rec)), "serial %llu table %d: contents", (unsigned long long)serial, i);
    for (int j = 0; j < i; ++j) {
      const Rec *e = dev[i]->earlier[j];
      CHECK(e == dev[j] && e->tag == host[j].tag && e->words[4] == word(host[j].tag, 4), "serial %llu table %d -> %d: contents through the pointer",
            (unsigned long long)serial, i, j);
    }
  }
  b.launch();
  return HM_TABLE_OK;
}

int main() {
  uint64_t serial = 1, calls = 0, evictions_unpinned = 0;
  const Rec *dev[MAX_T], *dev2[MAX_T];
  // ---- unpinned: the limit reached at every position within a call
  for (size_t limit = 1; limit <= 9; ++limit) {
    uint64_t ev_limit = 0;
    for (int t = 1; t <= MAX_T; ++t)
      for (int j = 0; j <= t; ++j) {
        if ((size_t)j > limit) continue;
        Cache c;
        HostBackend b;
        c.limit = limit;
        while (c.tables.size() < limit - (size_t)j) {   // fillers: calls of one table
          CHECK(call(c, b, serial++, 1, dev) == HM_TABLE_OK, "filler refused");
          CHECK(c.tables.size() <= limit, "fillers: %zu tables at limit %zu", c.tables.size(), limit);
        }
        CHECK(c.tables.size() == limit - (size_t)j && c.evictions == 0, "fill: %zu tables, %llu evictions", c.tables.size(), (unsigned long long)c.evictions);
        for (int rep = 0; rep < 3; ++rep) {   // the call under test, then two more of its size: each meets what the one before left
          const size_t before = c.tables.size();
          const uint64_t ev = c.evictions;
          CHECK(call(c, b, serial++, t, dev) == HM_TABLE_OK, "call refused");
          ++calls;
          // at most limit - 1 tables survive an entry, plus this call's
          CHECK(c.tables.size() <= limit - 1 + (size_t)t, "limit %zu t %d j %d: %zu tables", limit, t, j, c.tables.size());
          CHECK((c.evictions > ev) == (before >= limit), "limit %zu t %d j %d: %zu tables at the entry, evictions %llu -> %llu", limit, t, j, before,
                (unsigned long long)ev, (unsigned long long)c.evictions);
          if (c.tables.size() < limit) {   // the same call again: all hits, the same pointers, nothing freed
            const uint64_t ev2 = c.evictions;
            const size_t n = c.tables.size();
            CHECK(call(c, b, serial - 1, t, dev2) == HM_TABLE_OK, "repeat refused");
            CHECK(!memcmp(dev, dev2, sizeof(dev[0]) * (size_t)t) && c.tables.size() == n && c.evictions == ev2, "limit %zu t %d j %d: the repeat missed", limit, t, j);
          }
        }
        CHECK(b.freed_unwaited == 0, "limit %zu t %d j %d: %ld tables freed with a kernel in flight", limit, t, j, b.freed_unwaited);
        CHECK((long)c.tables.size() == b.live, "limit %zu t %d j %d: %zu tables, %ld allocations", limit, t, j, c.tables.size(), b.live);
        ev_limit += c.evictions;
        c.clear(b);
        CHECK(b.live == 0, "leak");
      }
    CHECK(ev_limit > 0, "limit %zu: no eviction in the unpinned runs", limit);
    evictions_unpinned += ev_limit;
  }
  // ---- pinned: a live graph, a capture in progress, then neither
  for (size_t limit = 1; limit <= 9; ++limit)
    for (int t = 1; t <= MAX_T; ++t) {
      Cache c;
      HostBackend b;
      c.limit = limit;
      const Rec *graph[MAX_T];
      const uint64_t warm = serial++;
      CHECK(call(c, b, warm, t, graph) == HM_TABLE_OK, "warm run refused");   // the plan, run once ...
      c.capturing = true; b.capture = true;                                    // ... and captured
      size_t n = c.tables.size();
      CHECK(call(c, b, warm, t, dev) == HM_TABLE_OK && !memcmp(dev, graph, sizeof(dev[0]) * (size_t)t), "limit %zu t %d: the warm plan missed under capture", limit, t);
      CHECK(call(c, b, serial++, t, dev) == HM_TABLE_CAPTURE_MISS, "limit %zu t %d: a miss under capture was served", limit, t);
      CHECK(c.tables.size() == n && c.evictions == 0 && c.depth == 0, "limit %zu t %d: the refused miss changed the cache", limit, t);
      c.capturing = false; b.capture = false;
      c.live_graphs = 1;
      while (c.tables.size() < limit + 3) {
        const int tt = 1 + (int)(serial % MAX_T);
        CHECK(call(c, b, serial++, tt, dev) == HM_TABLE_OK, "call under a live graph refused");
      }
      CHECK(c.evictions == 0 && b.waits == 0 && c.tables.size() > limit, "limit %zu t %d: %llu evictions under a live graph", limit, t, (unsigned long long)c.evictions);
      // someone else's capture of the stream (not hm_capture_begin): nothing is freed either
      c.live_graphs = 0; b.capture = true;
      n = c.tables.size();
      CHECK(call(c, b, warm, t, dev) == HM_TABLE_OK && c.evictions == 0 && c.tables.size() == n, "limit %zu t %d: evicted under a foreign capture", limit, t);
      b.capture = false; c.live_graphs = 1;
      // the replay: the graph's tables, through the pointers its nodes hold
      for (int i = 0; i < t; ++i) {
        CHECK(graph[i]->tag == warm * 16 + (uint64_t)i && graph[i]->words[0] == word(graph[i]->tag, 0), "limit %zu t %d: the graph's table %d", limit, t, i);
        for (int k = 0; k < i; ++k) CHECK(graph[i]->earlier[k] == graph[k], "limit %zu t %d: the graph's table %d -> %d", limit, t, i, k);
      }
      // a wait that fails frees nothing
      c.live_graphs = 0; b.fail_wait = true;
      n = c.tables.size();
      CHECK(call(c, b, serial++, t, dev) == HM_TABLE_BACKEND && c.backend_status == 7 && c.tables.size() == n && c.evictions == 0 && c.depth == 0,
            "limit %zu t %d: a failed wait", limit, t);
      b.fail_wait = false;
      // the graph is gone: the next call starts over, and is served
      CHECK(call(c, b, serial++, t, dev) == HM_TABLE_OK && c.evictions == 1 && c.tables.size() == (size_t)t, "limit %zu t %d: after the pin, %zu tables, %llu evictions", limit, t,
            c.tables.size(), (unsigned long long)c.evictions);
      CHECK(b.freed_unwaited == 0 && (long)c.tables.size() == b.live, "limit %zu t %d: frees", limit, t);
      c.clear(b);
      CHECK(b.live == 0, "leak");
      calls += 4;
    }
  // a call inside a call (hm_bconv -> hm_bconv_batch) is one call: the inner entry frees nothing
  {
    Cache c;
    HostBackend b;
    c.limit = 2;
    HmTableCall<HostBackend> outer(c, b);
    const void *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;
    uint64_t w[3] = {1, 2, 3};
    CHECK(c.get(b, &w[0], 8, &p0) == HM_TABLE_OK && c.get(b, &w[1], 8, &p1) == HM_TABLE_OK, "outer requests");
    {
      HmTableCall<HostBackend> inner(c, b);
      CHECK(inner.st == HM_TABLE_OK && c.evictions == 0 && c.tables.size() == 2, "the inner entry evicted");
      CHECK(c.get(b, &w[2], 8, &p2) == HM_TABLE_OK, "inner request");
    }
    CHECK(*static_cast<const uint64_t *>(p0) == 1 && *static_cast<const uint64_t *>(p1) == 2 && *static_cast<const uint64_t *>(p2) == 3 && c.depth == 1, "nested contents");
    c.clear(b);
  }
  CHECK(HM_LAUNCH_TABLE_LIMIT == 1024 && Cache().limit == 1024, "the default limit");
  printf("calls=%llu evictions_unpinned=%llu bad=%d\n", (unsigned long long)calls, (unsigned long long)evictions_unpinned, bad);
  return bad != 0;
}
