// The per-context cache of launch tables (NTT entry constants, base-conversion problem records, key-product records): device copies keyed by
// their bytes, the limit, what pins the cache, and when it starts over.  Host-only, plain C++17 (no HIP include), like hm_bconv_plan.h: the
// back-end instantiates it with the HIP calls (hm_backend.hip: device_table), tests/emu/hm_table_cache_main.cpp with malloc / memcpy / free.
//
// Contract: no table handed out since the entry of the current ABI call is freed before that call returns.  A call obtains several tables before
// it launches and stores earlier device pointers inside later tables (hm_bconv_batch: ep_k in the problem records; the fused conversion: mixk), so
// the cache never starts over inside a request: it does so at the ENTRY of an outermost call (begin_call), when it holds `limit` tables or more
// and nothing pins it.  Between two evictions it therefore holds at most limit - 1 tables plus those of one call.
//
// `Backend` supplies:
//   int upload(const void *data, size_t bytes, void **dev)   a new device copy (synchronous); 0 = done
//   void release(void *dev)                                  free one
//   int wait()                                               everything enqueued on the stream has finished; 0 = done
//   bool stream_capturing()                                  the stream records into a graph (asked on a miss and before an eviction only)
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>

#define HM_LAUNCH_TABLE_LIMIT 1024   // tables a context keeps before it starts over (option "launch_table_limit": tests)

enum HmTableStatus {
  HM_TABLE_OK = 0,
  HM_TABLE_CAPTURE_MISS,   // a table is missing while the stream is capturing: the upload would be a hidden synchronisation
  HM_TABLE_BACKEND         // the backend refused (its own status is in `backend_status`)
};

template <class Backend>
struct HmTableCache {
  std::map<std::string, void *> tables;   // key: the table's bytes
  size_t limit = HM_LAUNCH_TABLE_LIMIT;
  int live_graphs = 0;      // captured graphs whose kernel nodes keep table addresses: no eviction while > 0
  bool capturing = false;   // between hm_capture_begin and hm_capture_end: the graph being recorded keeps them too
  uint64_t evictions = 0;   // times the cache started over
  int depth = 0;            // ABI calls in progress (one calls another: hm_bconv -> hm_bconv_batch)
  int backend_status = 0;

  bool pinned() const { return live_graphs > 0 || capturing; }

  // entry of an ABI call that may request tables: the only place where tables are freed (besides clear)
  HmTableStatus begin_call(Backend &b) {
    if (depth++ > 0 || tables.size() < limit || pinned() || b.stream_capturing()) return HM_TABLE_OK;
    if ((backend_status = b.wait())) return HM_TABLE_BACKEND;   // kernels already enqueued read their tables
    clear(b);
    ++evictions;
    return HM_TABLE_OK;
  }
  void end_call() { --depth; }

  // the device copy of `data`: the cached one, or a new one (uploaded synchronously)
  HmTableStatus get(Backend &b, const void *data, size_t bytes, const void **out) {
    const std::string key(static_cast<const char *>(data), bytes);
    auto it = tables.find(key);
    if (it == tables.end()) {
      if (b.stream_capturing()) return HM_TABLE_CAPTURE_MISS;
      void *dev = nullptr;
      if ((backend_status = b.upload(data, bytes, &dev))) return HM_TABLE_BACKEND;
      it = tables.emplace(key, dev).first;
    }
    *out = it->second;
    return HM_TABLE_OK;
  }

  void clear(Backend &b) {
    for (auto &kv : tables) b.release(kv.second);
    tables.clear();
  }
};

// one ABI call's span of the cache (the status of its entry is in `st`)
template <class Backend>
struct HmTableCall {
  HmTableCache<Backend> &cache;
  HmTableStatus st;
  HmTableCall(HmTableCache<Backend> &c, Backend &b) : cache(c), st(c.begin_call(b)) {}
  ~HmTableCall() { cache.end_call(); }
  HmTableCall(const HmTableCall &) = delete;
  HmTableCall &operator=(const HmTableCall &) = delete;
};
