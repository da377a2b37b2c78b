// rl_routed_refund_shim.cpp — test access to HipRoutedRateLimitCache (api-ratelimit_amd/csrc/
// rl_cache.hpp) with HipSettings::refund_rejected, for one rank of an emulated world: DoLimit of a
// request of one or two descriptors, Peek, the refund counters and the batcher's trace hook, which
// reports the batcher's own refunds with a null request. Test infrastructure only:
// tests/test_gpu_routed_refund_cache.py drives it.
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
  std::unique_ptr<HipRoutedRateLimitCache> cache;
  std::mutex mu;  // err, trace, refunds
  std::string err;
  std::map<const RateLimitRequest*, std::pair<uint64_t, uint32_t>> trace;  // request -> (seq, pos)
  std::vector<uint64_t> refunds;  // seq of every control call traced with a null request
};
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

// One rank of an emulated world (id from rl_router_emu_world). Collective: every rank's create runs
// at the same time, one thread per rank; so does rlr_destroy.
void* rlr_create(uint32_t n_shards, uint32_t rank, const uint8_t* id, int local_cache, int refund_rejected,
                 uint32_t step_us, uint32_t rule_sync_every) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  hs.refund_rejected = refund_rejected != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = 12;
  hs.batch_limit = 1u << 12;
  HipRoutedSettings rs;
  rs.n_shards = n_shards;
  rs.rank = rank;
  rs.id.assign(id, id + RL_ROUTER_ID_BYTES);
  rs.emulated = true;
  rs.step_us = step_us;
  rs.rule_sync_every = rule_sync_every;
  try {
    s->cache = std::make_unique<HipRoutedRateLimitCache>(hs, rs, s->ts);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  s->cache->set_trace([s](const RateLimitRequest* req, uint64_t seq, uint32_t pos) {
    std::lock_guard<std::mutex> g(s->mu);
    if (req)
      s->trace[req] = {seq, pos};
    else if (pos == HipRoutedRateLimitCache::kTraceControl)
      s->refunds.push_back(seq);
  });
  return s;
}
void rlr_destroy(void* p) { delete static_cast<Shim*>(p); }
void rlr_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rlr_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of n (1 or 2) descriptors (key, values[i]) under rules[i] (-1: no limit): out = per
// descriptor its code and LimitRemaining; the call's traced (seq, pos). -1 on RedisError (rlr_error).
int rlr_do_limit(void* p, const char* domain, const char* key, uint32_t n, const char* const* values, const int* rules,
                 uint32_t hits, uint32_t* out, uint64_t* seq, uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = domain;
  req.HitsAddend = hits;
  req.Descriptors.resize(n);
  std::vector<std::shared_ptr<RateLimit>> limits;
  for (uint32_t i = 0; i < n; ++i) {
    req.Descriptors[i].Entries.push_back({key, values[i]});
    limits.push_back(rules[i] < 0 ? nullptr : s->rules[(size_t)rules[i]]);
  }
  try {
    const DoLimitResponse r = s->cache->DoLimit(req, limits);
    for (uint32_t i = 0; i < n; ++i) {
      out[2 * i] = (uint32_t)r.DescriptorStatuses[i].code;
      out[2 * i + 1] = r.DescriptorStatuses[i].LimitRemaining;
    }
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
// Peek of a request of one descriptor: out = Found, LocalCached, Count, TtlSeconds, CachedSeconds.
int rlr_peek(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t* out, uint64_t* seq,
             uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = domain;
  req.HitsAddend = 1;
  req.Descriptors.resize(1);
  req.Descriptors[0].Entries.push_back({key, value});
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  try {
    const PeekStatus r = s->cache->Peek(req, limits)[0];
    out[0] = r.Found;
    out[1] = r.LocalCached;
    out[2] = r.Count;
    out[3] = r.TtlSeconds;
    out[4] = r.CachedSeconds;
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
uint64_t rlr_refund_flights(void* p) { return static_cast<Shim*>(p)->cache->refund_flights(); }
uint64_t rlr_refund_failures(void* p) { return static_cast<Shim*>(p)->cache->refund_failures(); }
// The step numbers the trace hook reported for the batcher's own refunds so far: up to cap of them
// into out; returns how many there are.
uint32_t rlr_refund_seqs(void* p, uint64_t* out, uint32_t cap) {
  auto* s = static_cast<Shim*>(p);
  std::lock_guard<std::mutex> g(s->mu);
  for (uint32_t i = 0; i < cap && i < s->refunds.size(); ++i) out[i] = s->refunds[i];
  return (uint32_t)s->refunds.size();
}
uint32_t rlr_trace_control(void) { return HipRoutedRateLimitCache::kTraceControl; }
const char* rlr_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
