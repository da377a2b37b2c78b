// rl_merge_shim.cpp — test access to HipRateLimitCache::Merge / Peek / Resize (api-ratelimit_amd/
// csrc/rl_cache.hpp), C++ entry points that ctypes cannot reach, to the batcher's trace hook and
// to its auto-grow counters. Test infrastructure only: tests/test_gpu_merge_cache.py drives it
// with one-descriptor requests.
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
  std::mutex mu;  // err, trace, control
  std::string err;
  std::map<const RateLimitRequest*, std::pair<uint64_t, uint32_t>> trace;  // request -> (seq, pos)
  std::vector<uint64_t> control;  // seq of every control call traced without a request (a Merge chunk)
};
RateLimitRequest one(const char* domain, const char* key, const char* value, uint32_t hits) {
  RateLimitRequest req;
  req.Domain = domain;
  req.Descriptors.resize(1);
  req.Descriptors[0].Entries.push_back({key, value});
  req.HitsAddend = hits;
  return req;
}
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
}  // namespace

extern "C" {

// log2_slots, max_log2_slots: four words each (SECOND, MINUTE, HOUR, DAY homes)
void* rlm_create(int local_cache, uint32_t window_us, const uint32_t* log2_slots, uint32_t autogrow_permille,
                 const uint32_t* max_log2_slots, uint32_t batch_limit) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = log2_slots[u];
  hs.autogrow_permille = autogrow_permille;
  for (int u = 0; u < 4; ++u) hs.max_log2_slots[u] = max_log2_slots[u];
  hs.batch_limit = batch_limit;
  hs.batch_window_us = window_us;
  try {
    s->cache = std::make_unique<HipRateLimitCache>(hs, s->ts);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  s->cache->set_trace([s](const RateLimitRequest* req, uint64_t seq, uint32_t pos) {
    std::lock_guard<std::mutex> g(s->mu);
    if (req) s->trace[req] = {seq, pos};
    else if (pos == HipRateLimitCache::kTraceControl) s->control.push_back(seq);
  });
  return s;
}
void rlm_destroy(void* p) { delete static_cast<Shim*>(p); }
void rlm_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rlm_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of one descriptor: out = code, LimitRemaining, ThrottleMillis; its traced (seq, pos).
int rlm_do_limit(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t hits,
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
// out = Found, LocalCached, Count, TtlSeconds, CachedSeconds
int rlm_peek(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  const RateLimitRequest req = one(domain, key, value, 1);
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  try {
    const HipRateLimitCache::PeekStatus r = s->cache->Peek(req, limits)[0];
    out[0] = r.Found;
    out[1] = r.LocalCached;
    out[2] = r.Count;
    out[3] = r.TtlSeconds;
    out[4] = r.CachedSeconds;
    uint64_t seq;
    uint32_t pos;
    place_of(s, &req, &seq, &pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// report = Records, Folded, Claimed, DroppedOver, DroppedEmpty. -1 on RedisError (rlm_error);
// *merged = the records merged before a refusal (~0 when the error carries no count).
int rlm_merge(void* p, const char* path, uint64_t first_record, uint64_t* report, uint64_t* merged) {
  auto* s = static_cast<Shim*>(p);
  *merged = ~0ull;
  try {
    const HipRateLimitCache::MergeReport r = s->cache->Merge(path, first_record);
    report[0] = r.Records;
    report[1] = r.Folded;
    report[2] = r.Claimed;
    report[3] = r.DroppedOver;
    report[4] = r.DroppedEmpty;
    return 0;
  } catch (const HipRateLimitCache::MergeError& e) {
    *merged = e.Merged;
    return failed(s, e);
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// The batch sequence numbers the Merge chunks were traced at, in order; returns how many there are.
uint32_t rlm_control_seqs(void* p, uint64_t* out, uint32_t cap) {
  auto* s = static_cast<Shim*>(p);
  std::lock_guard<std::mutex> g(s->mu);
  for (uint32_t i = 0; i < cap && i < s->control.size(); ++i) out[i] = s->control[i];
  return (uint32_t)s->control.size();
}
int rlm_resize(void* p, const uint32_t* log2_slots) {
  auto* s = static_cast<Shim*>(p);
  try {
    s->cache->Resize(log2_slots);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// out: live[8], slots[8]
int rlm_occupancy(void* p, uint32_t* out) {
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
uint64_t rlm_resizes(void* p) { return static_cast<Shim*>(p)->cache->batcher_stats().resizes; }
const char* rlm_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
