// rl_snapshot_shim.cpp — test access to HipRateLimitCache::Save / Load (api-ratelimit_amd/csrc/
// rl_cache.hpp), C++ entry points that ctypes cannot reach. Test infrastructure only:
// tests/test_gpu_snapshot.py drives it with one-descriptor requests.
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

// log2_slots: four words (SECOND, MINUTE, HOUR, DAY homes)
void* rls_create(int local_cache, const uint32_t* log2_slots) {
  auto* s = new Shim();
  HipSettings hs;
  hs.local_cache = local_cache != 0;
  for (int u = 0; u < 4; ++u) hs.log2_slots[u] = log2_slots[u];
  hs.batch_limit = 1u << 12;
  try {
    s->cache = std::make_unique<HipRateLimitCache>(hs, s->ts);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  return s;
}
void rls_destroy(void* p) { delete static_cast<Shim*>(p); }
void rls_set_time(void* p, int64_t now) { static_cast<Shim*>(p)->ts->t.store(now); }
int rls_add_rule(void* p, uint32_t rpu, uint32_t unit) {
  auto* s = static_cast<Shim*>(p);
  s->rules.push_back(NewRateLimit(rpu, (Unit)unit, "rule" + std::to_string(s->rules.size()), s->store, false, false));
  return (int)s->rules.size() - 1;
}
// One request of one descriptor ("snap", [("k", value)]) under rule `rule`:
// out = code, LimitRemaining, ThrottleMillis. -1 on RedisError (rls_error).
int rls_do_limit(void* p, const char* value, int rule, uint32_t hits, uint32_t* out) {
  auto* s = static_cast<Shim*>(p);
  RateLimitRequest req;
  req.Domain = "snap";
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
int rls_save(void* p, const char* path) {
  auto* s = static_cast<Shim*>(p);
  try {
    s->cache->Save(path);
    return 0;
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}
int rls_load(void* p, const char* path) {
  auto* s = static_cast<Shim*>(p);
  try {
    s->cache->Load(path);
    return 0;
  } catch (const std::exception& e) {
    s->err = e.what();
    return -1;
  }
}
const char* rls_error(void* p) { return static_cast<Shim*>(p)->err.c_str(); }

}  // extern "C"
