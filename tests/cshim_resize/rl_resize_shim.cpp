// rl_resize_shim.cpp — test access to HipRateLimitCache::Resize / Occupancy and the auto-grow
// settings (api-ratelimit_amd/csrc/rl_cache.hpp), C++ entry points that ctypes cannot reach. Test
// infrastructure only: tests/test_gpu_resize_cache.py drives it with one-descriptor requests.
#include <atomic>
#include <memory>
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
  std::string err;
};
}  // namespace

extern "C" {

// log2_slots, max_log2_slots: four words each (SECOND, MINUTE, HOUR, DAY homes)
void* rlz_create(int local_cache, const uint32_t* log2_slots, uint32_t autogrow_permille,
                 const uint32_t* max_log2_slots) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = log2_slots[u];
  hs.batch_limit = 1u << 12;
  hs.autogrow_permille = autogrow_permille;
  for (int u = 0; u < 4; ++u) hs.max_log2_slots[u] = max_log2_slots[u];
  try {
    s->cache = std::make_unique<HipRateLimitCache>(hs, s->ts);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  return s;
}
void rlz_destroy(void* p) { delete static_cast<Shim*>(p); }
void rlz_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rlz_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of one descriptor ("grow", [("k", value)]) under rule `rule`:
// out = code, LimitRemaining, ThrottleMillis. -1 on RedisError (rlz_error).
int rlz_do_limit(void* p, const char* value, int rule, uint32_t hits, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = "grow";
  req.Descriptors.resize(1);
  req.Descriptors[0].Entries.push_back({"k", value});
  req.HitsAddend = hits;
  std::vector<std::shared_ptr<RateLimit>> limits{s->rules[(size_t)rule]};
  try {
    const DoLimitResponse r = s->cache->DoLimit(req, limits);
    out[0] = (uint32_t)r.DescriptorStatuses[0].code;
    out[1] = r.DescriptorStatuses[0].LimitRemaining;
    out[2] = r.ThrottleMillis;
    return 0;
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}
int rlz_resize(void* p, const uint32_t* log2_slots) {
  auto* s = static_cast<Shim*>(p);
  try {
    s->cache->Resize(log2_slots);
    return 0;
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}
// out: 32 words, rl_occupancy's gen, live, limit, slots
int rlz_occupancy(void* p, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  try {
    const rl_occupancy o = s->cache->Occupancy();
    for (int r = 0; r < 8; ++r) {
      out[r] = o.gen[r];
      out[8 + r] = o.live[r];
      out[16 + r] = o.limit[r];
      out[24 + r] = o.slots[r];
    }
    return 0;
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}
// out: batches, drains, resizes, resize_failures
void rlz_batcher_stats(void* p, uint64_t* out) {
  const auto b = static_cast<Shim*>(p)->cache->batcher_stats();
  out[0] = b.batches;
  out[1] = b.drains;
  out[2] = b.resizes;
  out[3] = b.resize_failures;
}
const char* rlz_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
