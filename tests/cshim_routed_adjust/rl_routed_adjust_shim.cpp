// rl_routed_adjust_shim.cpp — test access to HipRoutedRateLimitCache::Adjust (api-ratelimit_amd/
// csrc/rl_cache.hpp) beside DoLimit and Peek, for one rank of an emulated world, and to the
// batcher's trace hook. Test infrastructure only: tests/test_gpu_routed_adjust_cache.py drives it
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
  std::unique_ptr<HipRoutedRateLimitCache> cache;
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
void put(const PeekStatus& r, uint32_t* out) {
  out[0] = r.Found;
  out[1] = r.LocalCached;
  out[2] = r.Count;
  out[3] = r.TtlSeconds;
  out[4] = r.CachedSeconds;
}
}  // namespace

extern "C" {

// One rank of an emulated world (id from rl_router_emu_world). Collective: every rank's create runs
// at the same time, one thread per rank; so does rla_destroy.
void* rla_create(uint32_t n_shards, uint32_t rank, const uint8_t* id, int local_cache, uint32_t step_us,
                 uint32_t rule_sync_every) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
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
    s->trace[req] = {seq, pos};
  });
  return s;
}
void rla_destroy(void* p) { delete static_cast<Shim*>(p); }
void rla_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rla_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of one descriptor under rule `rule`: out = code, LimitRemaining, ThrottleMillis; the
// call's traced (seq, pos). -1 on RedisError (rla_error).
int rla_do_limit(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t hits,
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
int rla_peek(void* p, const char* domain, const char* key, const char* value, int rule, uint32_t* out, uint64_t* seq,
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
// Adjust of the same kind of request by delta; out = the state before the call, in Peek's words.
int rla_adjust(void* p, const char* domain, const char* key, const char* value, int rule, int32_t delta,
               int keep_cache, uint32_t* out, uint64_t* seq, uint32_t* pos) {
  auto* s = static_cast<Shim*>(p);
  const RateLimitRequest req = one(domain, key, value, 1);
  std::vector<std::shared_ptr<RateLimit>> limits{rule < 0 ? nullptr : s->rules[(size_t)rule]};
  try {
    put(s->cache->Adjust(req, limits, {delta}, keep_cache != 0)[0], out);
    place_of(s, &req, seq, pos);
    return 0;
  } catch (const std::exception& e) {
    return failed(s, e);
  }
}
uint32_t rla_trace_control(void) { return HipRoutedRateLimitCache::kTraceControl; }
const char* rla_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
