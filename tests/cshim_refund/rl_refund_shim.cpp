// rl_refund_shim.cpp — test access to HipRateLimitCache with HipSettings::refund_rejected
// (api-ratelimit_amd/csrc/rl_cache.hpp): DoLimit of two-descriptor requests, Peek, the refund
// counters and the trace hook. Test infrastructure only: tests/test_gpu_refund_cache.py drives it.
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
int failed(Shim* s, const std::exception& e) {
  std::lock_guard<std::mutex> g(s->mu);
  s->err = e.what();
  return -1;
}
}  // namespace

extern "C" {

// log2_slots: four words (SECOND, MINUTE, HOUR, DAY homes)
void* rlf_create(int local_cache, int refund, uint32_t window_us, const uint32_t* log2_slots, uint32_t batch_limit) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  hs.refund_rejected = refund != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = log2_slots[u];
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
    s->trace[req] = {seq, pos};
  });
  return s;
}
void rlf_destroy(void* p) { delete static_cast<Shim*>(p); }
void rlf_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rlf_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of two descriptors, (domain, [("k", v0)]) under rule r0 and (domain, [("k", v1)])
// under rule r1: out = code, LimitRemaining of each, then ThrottleMillis; the call's traced
// (seq, pos). -1 on RedisError (rlf_error).
int rlf_do_limit(void* p, const char* domain, const char* v0, int r0, const char* v1, int r1, uint32_t hits,
                 uint32_t* out, uint64_t* seq, uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = domain;
  req.Descriptors.resize(2);
  req.Descriptors[0].Entries.push_back({"k", v0});
  req.Descriptors[1].Entries.push_back({"k", v1});
  req.HitsAddend = hits;
  std::vector<std::shared_ptr<RateLimit>> limits{s->rules[(size_t)r0], s->rules[(size_t)r1]};
  try {
    const DoLimitResponse r = s->cache->DoLimit(req, limits);
    for (int k = 0; k < 2; ++k) {
      out[2 * k] = (uint32_t)r.DescriptorStatuses[k].code;
      out[2 * k + 1] = r.DescriptorStatuses[k].LimitRemaining;
    }
    out[4] = r.ThrottleMillis;
    std::lock_guard<std::mutex> g(s->mu);
    auto it = s->trace.find(&req);
    *seq = it == s->trace.end() ? ~0ull : it->second.first;
    *pos = it == s->trace.end() ? 0u : it->second.second;
    if (it != s->trace.end()) s->trace.erase(it);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// Peek of one descriptor: out = Found, LocalCached, Count.
int rlf_peek(void* p, const char* domain, const char* v, int rule, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = domain;
  req.Descriptors.resize(1);
  req.Descriptors[0].Entries.push_back({"k", v});
  req.HitsAddend = 1;
  std::vector<std::shared_ptr<RateLimit>> limits{s->rules[(size_t)rule]};
  try {
    const HipRateLimitCache::PeekStatus r = s->cache->Peek(req, limits)[0];
    out[0] = r.Found;
    out[1] = r.LocalCached;
    out[2] = r.Count;
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
uint64_t rlf_refunds(void* p) { return static_cast<Shim*>(p)->cache->refund_flights(); }
uint64_t rlf_refund_failures(void* p) { return static_cast<Shim*>(p)->cache->refund_failures(); }
uint64_t rlf_batches(void* p) { return static_cast<Shim*>(p)->cache->batcher_stats().batches; }
uint64_t rlf_compact_batches(void* p) { return static_cast<Shim*>(p)->cache->batcher_stats().compact_batches; }
const char* rlf_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
