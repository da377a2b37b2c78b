// rl_set_shim.cpp — test access to HipRateLimitCache::Set / Peek (api-ratelimit_amd/csrc/
// rl_cache.hpp), C++ entry points that ctypes cannot reach, to the batcher's trace hook and to its
// auto-grow counters. Test infrastructure only: tests/test_gpu_set_cache.py drives it with
// one-descriptor requests.
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rl_cache.hpp"

using namespace ratelimit;

namespace {
class FixedTime : public TimeSource {
 public:
  std::atomic<int64_t> t{0};
  int64_t UnixNow() override { return t.load(); }
};
struct Shim {
  std::shared_ptr<FixedTime> ts = std::make_shared<FixedTime>();
  StatsStore store;
  std::vector<std::shared_ptr<RateLimit>> rules;
  std::unique_ptr<HipRateLimitCache> cache;
  std::mutex mu;  // err, trace
  std::string err;
  std::map<const RateLimitRequest*, std::pair<uint64_t, uint32_t>> trace;  // request -> (seq, pos)
};
RateLimitRequest one(const char* domain, const char* key, const char* value, uint32_t hits) {
  RateLimitRequest req;
  req.Domain = domain;
  req.Descriptors.resize(1);
  req.Descriptors[0].Entries.push_back({key, value});
  req.HitsAddend = hits;
  return req;
}
// The traced place of a request as (seq, pos); seq = ~0 when it was not traced.
void place_of(Shim* s, const RateLimitRequest* req, uint64_t* seq, uint32_t* pos) {
  std::lock_guard<std::mutex> g(s->mu);
  auto it = s->trace.find(req);
  *seq = it == s->trace.end() ? ~0ull : it->second.first;
  *pos = it == s->trace.end() ? 0u : it->second.second;
  if (it != s->trace.end()) s->trace.erase(it);
}
int failed(Shim* s, const std::exception& e) {
  std::lock_guard<std::mutex> g(s->mu);
  s->err = e.what();
  return -1;
}
void put(const HipRateLimitCache::PeekStatus& r, uint32_t* out) {
  out[0] = r.Found;
  out[1] = r.LocalCached;
  out[2] = r.Count;
  out[3] = r.TtlSeconds;
  out[4] = r.CachedSeconds;
}
}  // namespace

extern "C" {

// log2_slots, max_log2_slots: four words each (SECOND, MINUTE, HOUR, DAY homes)
void* rls_create(int local_cache, uint32_t window_us, const uint32_t* log2_slots, uint32_t autogrow_permille,
                 const uint32_t* max_log2_slots) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = log2_slots[u];
  hs.autogrow_permille = autogrow_permille;
  for (int u = 0; u < 4; ++u) hs.max_log2_slots[u] = max_log2_slots[u];
  hs.batch_limit = 1u << 12;
  hs.batch_window_us = window_us;
  try {
    s->cache = std::make_unique<HipRateLimitCache>(hs, s->ts);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  s->cache->set_trace([s](const RateLimitRequest* req, uint64_t seq, uint32_t pos) {
    std::lock_guard<std::mutex> g(s->mu);
    s->trace[req] = {seq, pos};
  });
  return s;
}
void rls_destroy(void* p) { delete static_cast<Shim*>(p); }
void rls_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rls_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of one descriptor (domain, [(key, value)]) under rule `rule`: out = code,
// LimitRemaining, ThrottleMillis; the call's traced (seq, pos). -1 on RedisError (rls_error).
int rls_do_limit(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t hits,
                 uint32_t* out, uint64_t* seq, uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  const RateLimitRequest req = one(domain, key, value, hits);
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  try {
    const DoLimitResponse r = s->cache->DoLimit(req, limits);
    out[0] = (uint32_t)r.DescriptorStatuses[0].code;
    out[1] = r.DescriptorStatuses[0].LimitRemaining;
    out[2] = r.ThrottleMillis;
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// Peek of the same kind of request: out = Found, LocalCached, Count, TtlSeconds, CachedSeconds.
int rls_peek(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t* out, uint64_t* seq,
             uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  const RateLimitRequest req = one(domain, key, value, 1);
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  try {
    put(s->cache->Peek(req, limits)[0], out);
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// Set: value = Found, LocalCached, Count, TtlSeconds, CachedSeconds; out = the status before.
int rls_set(void* p, const char* domain, const char* key, const char* value, int rule, const uint32_t* val,
            int keep_counter, int keep_cache, uint32_t* out, uint64_t* seq, uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  const RateLimitRequest req = one(domain, key, value, 1);
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  HipRateLimitCache::PeekStatus v;
  v.Found = val[0] != 0;
  v.LocalCached = val[1] != 0;
  v.Count = val[2];
  v.TtlSeconds = val[3];
  v.CachedSeconds = val[4];
  try {
    put(s->cache->Set(req, limits, {v}, keep_counter != 0, keep_cache != 0)[0], out);
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// out: live[8], slots[8]
int rls_occupancy(void* p, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  try {
    const rl_occupancy o = s->cache->Occupancy();
    for (int r = 0; r < 8; ++r) {
      out[r] = o.live[r];
      out[8 + r] = o.slots[r];
    }
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
uint64_t rls_resizes(void* p) { return static_cast<Shim*>(p)->cache->batcher_stats().resizes; }
uint64_t rls_total_hits(void* p, int rule) { return static_cast<Shim*>(p)->rules[(size_t)rule]->Stats->TotalHits.Value(); }
uint32_t rls_trace_control(void) { return HipRateLimitCache::kTraceControl; }
const char* rls_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
