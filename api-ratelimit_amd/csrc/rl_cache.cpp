// rl_cache.cpp — HipRateLimitCache: the reference's RateLimitCache contract on the HIP engine.
#include "rl_cache.hpp"

#include "rl_common.h"  // decide_status (a local-cache hit's status, as the device makes it)

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

namespace ratelimit {

std::shared_ptr<RateLimitStats> StatsStore::Get(const std::string& key) {
  std::lock_guard<std::mutex> g(mu_);
  auto& p = m_[key];
  if (!p) p = std::make_shared<RateLimitStats>();
  return p;
}

std::shared_ptr<RateLimit> NewRateLimit(uint32_t requests_per_unit, Unit unit, const std::string& key,
                                        StatsStore& scope, bool sleep_on_throttle, bool report_details) {
  auto r = std::make_shared<RateLimit>();
  r->FullKey = key;
  r->Stats = scope.Get(key);
  r->Limit.RequestsPerUnit = requests_per_unit;
  r->Limit.unit = unit;
  r->SleepOnThrottle = sleep_on_throttle;
  r->ReportDetails = report_details;
  return r;
}

bool DescriptorStatus::operator==(const DescriptorStatus& o) const {
  if (code != o.code || LimitRemaining != o.LimitRemaining) return false;
  if ((CurrentLimit == nullptr) != (o.CurrentLimit == nullptr)) return false;
  if (CurrentLimit && (CurrentLimit->RequestsPerUnit != o.CurrentLimit->RequestsPerUnit ||
                       CurrentLimit->unit != o.CurrentLimit->unit))
    return false;
  if (HasDurationUntilReset != o.HasDurationUntilReset) return false;
  return !HasDurationUntilReset || DurationUntilResetSeconds == o.DurationUntilResetSeconds;
}

int64_t SystemTimeSource::UnixNow() {
  return std::chrono::duration_cast<std::chrono::seconds>(std::chrono::system_clock::now().time_since_epoch())
      .count();
}

struct PendingCall {
  const RateLimitRequest* req = nullptr;
  const std::vector<std::shared_ptr<RateLimit>>* limits = nullptr;
  int64_t now = 0;
  uint32_t hits = 1;
  std::vector<std::string> prefix;  // per descriptor ("" = nil limit)
  // HIP_LOCAL_CACHE=freecache: per descriptor, a hit of the lookup made at enqueue (no INCRBY)
  // and the full cache key (GenerateCacheKey, cache_key.go:57-68) it was looked up / is Set by
  std::vector<uint8_t> lhit;
  std::vector<std::string> fkey;
  size_t blob_bytes = 0;
  DoLimitResponse resp;
  std::promise<void> done;
  // A control call (Save / Load) instead of a request: it keeps its place in the queue, and the
  // submitter runs it with nothing in flight. Returns an error message, empty on success.
  std::function<std::string()> ctl;
  // HipRoutedRateLimitCache: a Peek (1), Forget (2), Set (3) or Adjust (4; 5 with keep_cache)
  // instead of a request, answered at a rule / stop agreement into `peek`; a Set's values (with its
  // KEEP bits or-ed in) in `set_vals`, an Adjust's deltas in `deltas`
  // or, queued by the batcher itself with nobody waiting (HIP_REFUND_REJECTED), the refund of a
  // rejected request (6; 7 with RL_REFUND_KEEP_CACHE): req and limits are null (the caller has been
  // answered), the request's time and raw HitsAddend in `now` and `hits`, its agreed rule ids in
  // `rule_ids` and its statuses in `statuses`
  int kind = 0;
  std::vector<PeekStatus> peek;
  std::vector<rl_peek_reply> set_vals;
  std::vector<int32_t> deltas;
  std::vector<uint32_t> rule_ids;
  std::vector<rl_status> statuses;
  // HipRateLimitCache::AdjustQueued: an adjust that waits in the queue like a DoLimit (prefix,
  // limits and deltas as above, answered into `peek`); keep: RL_ADJUST_KEEP_CACHE
  bool adj_queued = false, keep = false;
};

namespace {

// The caller's side of DoLimit, shared by both batchers: GenerateCacheKeys' prefix bytes per
// descriptor with a limit (cache_key.go:57-65), one time per request (base_limiter.go:43), the
// hits (fixed_cache_impl.go:39), Stats.TotalHits (base_limiter.go:49-51).
std::shared_ptr<PendingCall> make_call(const RateLimitRequest& request,
                                       const std::vector<std::shared_ptr<RateLimit>>& limits, TimeSource& ts) {
  // assert.Assert(len(request.Descriptors) == len(limits))  base_limiter.go:41
  if (request.Descriptors.size() != limits.size())
    throw std::logic_error("assert: len(request.Descriptors) == len(limits)");
  auto call = std::make_shared<PendingCall>();
  call->req = &request;
  call->limits = &limits;
  call->now = ts.UnixNow();                                     // base_limiter.go:43
  call->hits = request.HitsAddend > 1 ? request.HitsAddend : 1;  // fixed_cache_impl.go:39
  call->prefix.resize(limits.size());
  for (size_t i = 0; i < limits.size(); ++i) {
    if (!limits[i]) continue;
    // GenerateCacheKey prefix: domain '_' (key '_' value '_')*   cache_key.go:57-65
    std::string& p = call->prefix[i];
    p = request.Domain;
    p += '_';
    for (const auto& e : request.Descriptors[i].Entries) {
      p += e.Key;
      p += '_';
      p += e.Value;
      p += '_';
    }
    call->blob_bytes += p.size();
    // Stats.TotalHits.Add(hitsAddend) for every non-nil limit  base_limiter.go:49-51
    limits[i]->Stats->TotalHits.Add(call->hits);
  }
  return call;
}

// A call's DescriptorStatuses and stat adds from its statuses (GetResponseDescriptorStatus's
// outputs, base_limiter.go:70-115,129-177), then the caller is released.
uint32_t unit_divider(Unit u) {  // utils.UnitToDivider
  return u == Unit::SECOND ? 1u : u == Unit::MINUTE ? 60u : u == Unit::HOUR ? 3600u : u == Unit::DAY ? 86400u : 0u;
}

void answer(PendingCall& c, const rl_status* out, uint32_t thr) {
  c.resp.DescriptorStatuses.resize(c.prefix.size());
  c.resp.ThrottleMillis = thr;
  for (size_t i = 0; i < c.prefix.size(); ++i) {
    const auto& lim = (*c.limits)[i];
    rl_status hit_st;
    if (!c.lhit.empty() && c.lhit[i]) {
      // IsOverLimitWithLocalCache: OVER_LIMIT, nothing remaining, OverLimit and
      // OverLimitWithLocalCache += hits (base_limiter.go:76-81); no ThrottleMillis
      rlhip::DevRule R{};
      R.L = lim->Limit.RequestsPerUnit;
      R.div = unit_divider(lim->Limit.unit);
      R.unit = (uint32_t)lim->Limit.unit;
      R.shadow = lim->ShadowMode ? 1u : 0u;
      rlhip::decide_status(0, true, c.hits, (uint32_t)(c.now % R.div), R, hit_st);
    }
    const rl_status& s = (!c.lhit.empty() && c.lhit[i]) ? hit_st : out[i];
    DescriptorStatus& o = c.resp.DescriptorStatuses[i];
    o.code = (Code)(s.code_flags & 0xFF);
    o.LimitRemaining = s.limit_remaining;
    const uint32_t fl = s.code_flags >> 8;
    if (lim && (fl & RL_FLAG_HAS_LIMIT)) {
      o.CurrentLimit = &lim->Limit;
      o.HasDurationUntilReset = true;
      o.DurationUntilResetSeconds = s.reset_s;
      // Stats adds of GetResponseDescriptorStatus (base_limiter.go:77-78,129-177)
      if (s.over_limit_delta) lim->Stats->OverLimit.Add(s.over_limit_delta);
      if (fl & RL_FLAG_LOCAL_CACHE_HIT) lim->Stats->OverLimitWithLocalCache.Add(s.over_limit_delta);
      if (s.near_limit_delta) lim->Stats->NearLimit.Add(s.near_limit_delta);
      if (fl & RL_FLAG_SHADOW) lim->Stats->ShadowMode.Add(1);
    }
  }
  c.done.set_value();
}

// EXPIRATION_JITTER_MAX_SECONDS: the settings' jitter source, or a seeded Int63n one (the
// reference seeds its lockedSource with the start time, runner.go / utils.NewLockedSource).
bool setup_jitter(HipSettings& s) {
  if (s.expiration_jitter_max_seconds <= 0) return false;
  if (s.expiration_jitter_max_seconds > 65536)
    throw RedisError("EXPIRATION_JITTER_MAX_SECONDS above 65536 (rl_batch.ttl_jitter is 16-bit)");
  if (!s.jitter_rand) {
    auto state = std::make_shared<std::pair<std::mutex, uint64_t>>();
    state->second = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    s.jitter_rand = [state](int64_t n) {
      std::lock_guard<std::mutex> g(state->first);
      uint64_t z = (state->second += 0x9E3779B97F4A7C15ull);  // splitmix64
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      return (int64_t)(z % (uint64_t)n);
    };
  }
  return true;
}
// One draw: expirationSeconds += JitterRand.Int63n(max)  fixed_cache_impl.go:69-72
uint16_t draw_jitter(const HipSettings& s) { return (uint16_t)s.jitter_rand(s.expiration_jitter_max_seconds); }

}  // namespace

// The batch being built in one of the engine's pinned staging slots (rl_host_acquire_c, or
// rl_host_acquire for the full format): calls are written straight into C memory, the way the Go
// batcher does. The compact wire format (rl_batch_c) is the default; a batch
// whose first call does not fit it goes as rl_batch.
struct HipRateLimitCache::Staged {
  std::vector<std::shared_ptr<PendingCall>> calls;
  bool compact = true;
  rl_host_batch hb{};      // full format
  rl_host_batch_c hc{};    // compact format
  uint32_t nd = 0, nr = 0, nb = 0;
  uint32_t max_desc = 0, max_req = 0, max_blob = 0;
  int64_t tmin = 0, tmax = 0;
  bool one_per_req = true;  // compact: every request so far holds one descriptor (req_of implicit)
  bool failed = false;      // refused at submit: its callers already have the error
  uint64_t seq = 0;         // gathered (and submitted) in this order
  bool adjust = false;      // an rl_adjust_submit flight of queued adjusts (calls, nd and failed only)
  bool refund = false;      // the rl_refund_behind flight of the decision batch in front of it (adjust is
                            // set too: it claims nothing and is no decision; no calls wait on it)
};

// The queued adjusts of one gather with one keep flag: one rl_batch in plain memory, one request
// per call (rl_adjust_submit copies it).
struct HipRateLimitCache::AdjGather {
  std::vector<std::shared_ptr<PendingCall>> calls;
  std::vector<uint8_t> blob;
  std::vector<uint32_t> off{0u}, rule, req_of;
  std::vector<int64_t> now;
  std::vector<int32_t> delta;
};

HipRateLimitCache::HipRateLimitCache(const HipSettings& s, std::shared_ptr<TimeSource> ts)
    : s_(s), ts_(std::move(ts)) {
  jitter_ = setup_jitter(s_);
  rl_config c;
  memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.device = s.device;
  for (int u = 0; u < 4; ++u) c.log2_slots[u] = s.log2_slots[u];
  c.near_limit_ratio = s.near_limit_ratio;
  // HIP_LOCAL_CACHE=freecache: the host's bounded model is the local cache, the device keeps none
  if (s.local_cache && s.local_cache_freecache) fc_ = std::make_unique<FreeCacheModel>(s.local_cache_bytes);
  c.local_cache = s.local_cache && !fc_ ? 1 : 0;
  c.per_second_split = s.per_second_split ? 1 : 0;
  c.max_batch_desc = s.batch_limit + 4096;
  c.max_batch_req = s.batch_limit + 4096;
  c.max_blob_bytes = (s.batch_limit + 4096) * 128u;
  c.hash_seed = s.hash_seed;
  c.max_load_permille = s.max_load_permille;
  int rc = rl_create(&c, &eng_);
  if (rc) throw RedisError("rl_create failed: " + std::to_string(rc));
  thr_ = std::thread([this] { submitter(); });
}

HipRateLimitCache::~HipRateLimitCache() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  thr_.join();
  rl_destroy(eng_);
}

void HipRateLimitCache::Flush() {
  std::unique_lock<std::mutex> g(mu_);
  idle_cv_.wait(g, [&] { return inflight_ == 0; });
}

// Save / Load: a control call through the batcher's queue, so that every engine call stays on the
// submitter thread and the snapshot sits at one point of the serial order.
void HipRateLimitCache::control(std::function<std::string()> f) {
  auto call = std::make_shared<PendingCall>();
  call->ctl = std::move(f);
  std::future<void> fut = call->done.get_future();
  {
    std::lock_guard<std::mutex> g(mu_);
    q_.push_back(call);
    ++inflight_;
  }
  cv_.notify_one();
  fut.get();  // rethrows RedisError
}

namespace {
constexpr uint32_t kSnapChunk = 1u << 16;  // records per rl_snapshot_next / rl_restore_put
struct File {
  FILE* f;
  ~File() {
    if (f) fclose(f);
  }
};
}  // namespace

void HipRateLimitCache::Save(const std::string& path) {
  control([this, path]() -> std::string {
    File fp{fopen(path.c_str(), "wb")};
    if (!fp.f) return "Save: cannot open " + path;
    rl_snapshot_header h;
    if (rl_snapshot_begin(eng_, &h)) return rl_last_error(eng_);
    std::string msg;
    if (fwrite(&h, sizeof h, 1, fp.f) != 1) msg = "Save: write failed: " + path;
    std::vector<uint8_t> buf((size_t)kSnapChunk * RL_SNAP_RECORD_BYTES);
    for (uint32_t n = 1; msg.empty() && n;) {
      if (rl_snapshot_next(eng_, buf.data(), kSnapChunk, &n)) msg = rl_last_error(eng_);
      else if (n && fwrite(buf.data(), RL_SNAP_RECORD_BYTES, n, fp.f) != n) msg = "Save: write failed: " + path;
    }
    rl_snapshot_end(eng_);
    if (msg.empty() && fflush(fp.f)) msg = "Save: write failed: " + path;
    return msg;
  });
}

void HipRateLimitCache::Load(const std::string& path) {
  control([this, path]() -> std::string {
    File fp{fopen(path.c_str(), "rb")};
    if (!fp.f) return "Load: cannot open " + path;
    rl_snapshot_header h;
    if (fread(&h, sizeof h, 1, fp.f) != 1) return "Load: " + path + " is shorter than a snapshot header";
    if (fseek(fp.f, 0, SEEK_END)) return "Load: cannot seek " + path;
    const long size = ftell(fp.f);
    const uint64_t body = size < (long)sizeof h ? ~0ull : (uint64_t)size - sizeof h;
    if (body % RL_SNAP_RECORD_BYTES || body / RL_SNAP_RECORD_BYTES != h.n_records ||
        fseek(fp.f, (long)sizeof h, SEEK_SET))
      return "Load: " + path + " does not hold the header and its n_records records";
    if (rl_restore_begin(eng_, &h)) return rl_last_error(eng_);
    std::string msg;
    std::vector<uint8_t> buf((size_t)kSnapChunk * RL_SNAP_RECORD_BYTES);
    for (uint64_t left = h.n_records; msg.empty() && left;) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(left, kSnapChunk);
      if (fread(buf.data(), RL_SNAP_RECORD_BYTES, n, fp.f) != n) msg = "Load: read failed: " + path;
      else if (rl_restore_put(eng_, buf.data(), n)) msg = rl_last_error(eng_);
      left -= n;
    }
    if (!msg.empty()) {
      rl_reset(eng_);  // closes the restore: the table is empty
      return msg;
    }
    if (rl_restore_end(eng_)) return rl_last_error(eng_);
    return "";
  });
}

void HipRateLimitCache::Resize(const uint32_t log2_slots[4]) {
  uint32_t lg[4];
  for (int u = 0; u < 4; ++u) lg[u] = log2_slots[u];
  control([this, lg]() -> std::string { return rl_resize(eng_, lg) ? rl_last_error(eng_) : ""; });
}

// Merge: the file is read here, on the caller's thread; every chunk is a control call of its own,
// so what was enqueued while a chunk ran is decided before the next one.
HipRateLimitCache::MergeReport HipRateLimitCache::Merge(const std::string& path, uint64_t first_record) {
  File fp{fopen(path.c_str(), "rb")};
  if (!fp.f) throw RedisError("hip backend: Merge: cannot open " + path);
  rl_snapshot_header h;
  if (fread(&h, sizeof h, 1, fp.f) != 1)
    throw RedisError("hip backend: Merge: " + path + " is shorter than a snapshot header");
  if (fseek(fp.f, 0, SEEK_END)) throw RedisError("hip backend: Merge: cannot seek " + path);
  const long size = ftell(fp.f);
  const uint64_t body = size < (long)sizeof h ? ~0ull : (uint64_t)size - sizeof h;
  if (h.record_bytes != RL_SNAP_RECORD_BYTES || body % RL_SNAP_RECORD_BYTES ||
      body / RL_SNAP_RECORD_BYTES != h.n_records)
    throw RedisError("hip backend: Merge: " + path + " does not hold the header and its n_records records");
  if (first_record > h.n_records)
    throw RedisError("hip backend: Merge: first_record is past the file's n_records");
  if (fseek(fp.f, (long)(sizeof h + first_record * RL_SNAP_RECORD_BYTES), SEEK_SET))
    throw RedisError("hip backend: Merge: cannot seek " + path);
  const uint32_t chunk = std::max(1u, std::min(kSnapChunk, s_.batch_limit));
  std::vector<uint8_t> buf((size_t)chunk * RL_SNAP_RECORD_BYTES);
  MergeReport total;
  uint64_t done = first_record;
  // (a file without records left still has its header checked by the engine: one empty call)
  for (bool first = true; first || done < h.n_records; first = false) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(h.n_records - done, chunk);
    if (n && fread(buf.data(), RL_SNAP_RECORD_BYTES, n, fp.f) != n)
      throw MergeError("hip backend: Merge: read failed: " + path + " (" + std::to_string(done) + " records merged)", done);
    rl_merge_report rep;
    memset(&rep, 0, sizeof rep);
    try {
      control([this, &h, &buf, n, &rep]() -> std::string {
        if (trace_) trace_(nullptr, staged_seq_, kTraceControl);
        if (rl_merge(eng_, &h, buf.data(), n, ts_->UnixNow(), &rep)) return rl_last_error(eng_);
        grow_after_ctl_ = true;  // the chunk may have claimed slots: the watermark check of a completed batch
        return "";
      });
    } catch (const RedisError& e) {
      throw MergeError(std::string(e.what()) + " (Merge: " + std::to_string(done) + " records of " + path +
                           " are merged; after a Resize resume with first_record = " + std::to_string(done) + ")",
                       done);
    }
    total.Records += rep.records;
    total.Folded += rep.folded;
    total.Claimed += rep.claimed;
    total.DroppedOver += rep.dropped_over;
    total.DroppedEmpty += rep.dropped_empty;
    done += n;
  }
  return total;
}

rl_occupancy HipRateLimitCache::Occupancy() {
  rl_occupancy o;
  memset(&o, 0, sizeof o);
  control([this, &o]() -> std::string { return rl_get_occupancy(eng_, &o) ? rl_last_error(eng_) : ""; });
  return o;
}

// Auto-grow (rl_cache.hpp Resize), after a completed batch: while a home unit is over the
// watermark and below its maximum, complete what is in flight and double it. The occupancy is
// the host mirror's (no device call). This engine is a lone one (no lag window), so a region
// keeps no previous generation: live is all it holds.
void HipRateLimitCache::autogrow(std::deque<Staged>& inflight) {
  if (!s_.autogrow_permille) return;
  for (;;) {
    rl_occupancy o;
    if (rl_get_occupancy(eng_, &o)) return;
    uint32_t lg[4] = {0, 0, 0, 0}, used[4];
    bool any = false;
    for (int u = 0; u < 4; ++u) {
      used[u] = std::max(o.live[2 * u], o.live[2 * u + 1]);
      uint32_t log2 = 0;
      while ((1u << log2) < o.slots[2 * u]) ++log2;
      if ((uint64_t)used[u] * 1000u <= (uint64_t)o.slots[2 * u] * s_.autogrow_permille) continue;
      if (log2 >= s_.max_log2_slots[u] || log2 >= 31u) continue;
      if (grow_failed_at_[u] && used[u] <= grow_failed_at_[u]) continue;  // not before occupancy rises again
      lg[u] = log2 + 1;
      any = true;
    }
    if (!any) return;
    if (!inflight.empty()) {
      while (!inflight.empty()) {
        finish(inflight.front());
        inflight.pop_front();
      }
      n_drains_ += 1;
      continue;  // the drained batches moved the occupancy: decide on what it is now
    }
    if (rl_resize(eng_, lg)) {
      n_resize_fail_ += 1;
      for (int u = 0; u < 4; ++u)
        if (lg[u]) grow_failed_at_[u] = used[u];
      return;
    }
    n_resizes_ += 1;
    for (int u = 0; u < 4; ++u)
      if (lg[u]) grow_failed_at_[u] = 0;
  }
}

void HipRateLimitCache::finish_oldest(std::deque<Staged>& inflight) {
  const bool adjust = inflight.front().adjust;
  finish(inflight.front());
  inflight.pop_front();
  if (!adjust) autogrow(inflight);  // an adjust claims nothing
}

// Peek / Forget / Set: the request's descriptors as one rl_batch of one request, built and handed
// to rl_peek / rl_forget / rl_set by the submitter thread (a control call), at the time it reads
// there. values != nullptr: a Set, with `keep` (RL_SET_KEEP_*) or-ed into every value's flags.
// deltas != nullptr: an Adjust, with `keep` as rl_adjust's flags.
std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::peek_call(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits, bool forget,
    const std::vector<PeekStatus>* values, uint32_t keep, const std::vector<int32_t>* deltas) {
  if (request.Descriptors.size() != limits.size())
    throw std::logic_error("assert: len(request.Descriptors) == len(limits)");
  if (values && values->size() != limits.size()) throw std::logic_error("assert: len(values) == len(limits)");
  if (deltas && deltas->size() != limits.size()) throw std::logic_error("assert: len(deltas) == len(limits)");
  const size_t n = limits.size();
  // GenerateCacheKey prefixes (cache_key.go:57-65), on the caller's thread
  std::vector<uint8_t> blob;
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if (limits[i]) {
      std::string p = request.Domain;
      p += '_';
      for (const auto& e : request.Descriptors[i].Entries) {
        p += e.Key;
        p += '_';
        p += e.Value;
        p += '_';
      }
      blob.insert(blob.end(), p.begin(), p.end());
    }
    off[i + 1] = (uint32_t)blob.size();
  }
  std::vector<PeekStatus> result(n);
  control([&]() -> std::string {
    if (trace_) trace_(&request, staged_seq_, kTraceControl);
    if (!n) return "";
    std::vector<uint32_t> rule(n), req_of(n, 0u);
    for (size_t i = 0; i < n; ++i)
      rule[i] = limits[i] ? rule_id(limits[i]->Limit, limits[i]->ShadowMode) : RL_NIL_RULE;
    if (rules_dirty_) {  // nothing is in flight: any table may be loaded
      if (rl_load_rules(eng_, rules_.data(), (uint32_t)rules_.size())) return rl_last_error(eng_);
      rules_dirty_ = false;
      n_loads_ += 1;
    }
    const int64_t now = ts_->UnixNow();
    rl_batch b;
    memset(&b, 0, sizeof b);
    b.n_desc = (uint32_t)n;
    b.n_req = 1;
    b.blob_bytes = (uint32_t)blob.size();
    b.prefix_blob = blob.data();
    b.prefix_off = off.data();
    b.rule_id = rule.data();
    b.req_of = req_of.data();
    b.now = &now;
    std::vector<rl_peek_reply> rep(n);
    if (deltas) {
      // nothing is claimed: the auto-grow check does not run behind it
      if (rl_adjust(eng_, &b, deltas->data(), keep, rep.data(), nullptr)) return rl_last_error(eng_);
    } else if (values) {
      std::vector<rl_peek_reply> val(n);
      for (size_t i = 0; i < n; ++i) {
        const PeekStatus& v = (*values)[i];
        val[i].count = v.Count;
        val[i].ttl_s = v.TtlSeconds;
        val[i].cached_s = v.CachedSeconds;
        val[i].flags = (v.Found ? RL_PEEK_FOUND : 0u) | (v.LocalCached ? RL_PEEK_LOCAL_CACHED : 0u) | keep;
      }
      if (rl_set(eng_, &b, val.data(), rep.data())) return rl_last_error(eng_);
      grow_after_ctl_ = true;  // the call may have claimed slots: the watermark check of a completed batch
    } else if (forget ? rl_forget(eng_, &b, rep.data()) : rl_peek(eng_, &b, rep.data())) {
      return rl_last_error(eng_);
    }
    for (size_t i = 0; i < n; ++i) {
      PeekStatus& s = result[i];
      s.Found = (rep[i].flags & RL_PEEK_FOUND) != 0;
      s.LocalCached = (rep[i].flags & RL_PEEK_LOCAL_CACHED) != 0;
      s.Count = rep[i].count;
      s.TtlSeconds = rep[i].ttl_s;
      s.CachedSeconds = rep[i].cached_s;
    }
    return "";
  });
  return result;
}

std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::Peek(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits) {
  return peek_call(request, limits, false);
}

std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::Forget(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits) {
  return peek_call(request, limits, true);
}

std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::Set(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
    const std::vector<PeekStatus>& values, bool keep_counter, bool keep_cache) {
  // HIP_LOCAL_CACHE=freecache: the device cache is unused, the cache part is ignored
  const uint32_t keep = (keep_counter ? (uint32_t)RL_SET_KEEP_COUNTER : 0u) |
                        (keep_cache || fc_ ? (uint32_t)RL_SET_KEEP_CACHE : 0u);
  return peek_call(request, limits, false, &values, keep);
}

std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::Adjust(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
    const std::vector<int32_t>& deltas, bool keep_cache) {
  // HIP_LOCAL_CACHE=freecache: the device cache is unused, the cache part is ignored
  return peek_call(request, limits, false, nullptr, keep_cache || fc_ ? (uint32_t)RL_ADJUST_KEEP_CACHE : 0u, &deltas);
}

// AdjustQueued: the call waits in the queue like a DoLimit; the submitter gathers it (add_adjust)
// and answers it when its flight completes (finish).
std::vector<HipRateLimitCache::PeekStatus> HipRateLimitCache::AdjustQueued(
    const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
    const std::vector<int32_t>& deltas, bool keep_cache) {
  if (request.Descriptors.size() != limits.size())
    throw std::logic_error("assert: len(request.Descriptors) == len(limits)");
  if (deltas.size() != limits.size()) throw std::logic_error("assert: len(deltas) == len(limits)");
  auto call = std::make_shared<PendingCall>();
  call->req = &request;
  call->limits = &limits;
  call->adj_queued = true;
  call->keep = keep_cache || fc_;  // HIP_LOCAL_CACHE=freecache: the device cache is unused
  call->deltas = deltas;
  call->prefix.resize(limits.size());
  for (size_t i = 0; i < limits.size(); ++i) {
    if (!limits[i]) continue;
    std::string& p = call->prefix[i];  // GenerateCacheKey prefix  cache_key.go:57-65
    p = request.Domain;
    p += '_';
    for (const auto& e : request.Descriptors[i].Entries) {
      p += e.Key;
      p += '_';
      p += e.Value;
      p += '_';
    }
  }
  std::future<void> f = call->done.get_future();
  {
    std::lock_guard<std::mutex> g(mu_);
    q_.push_back(call);
    ++inflight_;
  }
  cv_.notify_one();
  f.get();  // rethrows RedisError
  return std::move(call->peek);
}

// A group is cut in front of a call that would take it past HIP_BATCH_LIMIT descriptors; a call
// larger than that goes alone, and the engine refuses it.
bool HipRateLimitCache::fits_adjust(const AdjGather& g, const PendingCall& c) const {
  return g.calls.empty() || g.rule.size() + c.prefix.size() <= s_.batch_limit;
}

// One queued adjust into its gather's group: one request, at the time read here.
void HipRateLimitCache::add_adjust(AdjGather& g, const std::shared_ptr<PendingCall>& cp, uint64_t seq) {
  PendingCall& c = *cp;
  const uint32_t r = (uint32_t)g.calls.size();
  if (trace_) trace_(c.req, seq, kTraceAdjust | (c.keep ? kTraceAdjustKeep : 0u) | r);
  g.now.push_back(ts_->UnixNow());
  for (size_t i = 0; i < c.prefix.size(); ++i) {
    const auto& lim = (*c.limits)[i];
    g.blob.insert(g.blob.end(), c.prefix[i].begin(), c.prefix[i].end());
    g.off.push_back((uint32_t)g.blob.size());
    g.rule.push_back(lim ? rule_id(lim->Limit, lim->ShadowMode) : RL_NIL_RULE);
    g.req_of.push_back(r);
    g.delta.push_back(c.deltas[i]);
  }
  g.calls.push_back(cp);
}

// Hand a gather's group to the engine as one flight (rl_adjust_submit), as submit() hands a batch:
// new rules first, one drain-and-retry on RL_ESTATE, any other refusal fails the group's calls.
HipRateLimitCache::Staged HipRateLimitCache::submit_adjust(AdjGather& g, bool keep, uint64_t seq,
                                                           std::deque<Staged>& inflight) {
  Staged st;
  st.adjust = true;
  st.seq = seq;
  st.nd = (uint32_t)g.rule.size();
  st.calls = std::move(g.calls);
  g.blob.resize(g.blob.size() + RL_BLOB_SLACK, 0);  // (never read past blob_bytes on the host; keeps data() non-null)
  rl_batch b;
  memset(&b, 0, sizeof b);
  b.n_desc = st.nd;
  b.n_req = (uint32_t)st.calls.size();
  b.blob_bytes = g.off.back();
  b.prefix_blob = g.blob.data();
  b.prefix_off = g.off.data();
  b.rule_id = g.rule.data();
  b.req_of = g.req_of.data();
  b.now = g.now.data();
  for (int attempt = 0;; ++attempt) {
    int rc = 0;
    if (rules_dirty_) {
      rc = rl_load_rules(eng_, rules_.data(), (uint32_t)rules_.size());
      if (!rc) {
        rules_dirty_ = false;
        n_loads_ += 1;
        if (!inflight.empty()) n_loads_inflight_ += 1;
      }
    }
    if (!rc) rc = rl_adjust_submit(eng_, &b, g.delta.data(), keep ? (uint32_t)RL_ADJUST_KEEP_CACHE : 0u, 1);
    if (rc == RL_ESTATE && attempt == 0 && !inflight.empty()) {
      while (!inflight.empty()) {
        finish(inflight.front());
        inflight.pop_front();
      }
      n_drains_ += 1;
      continue;
    }
    if (rc) {
      fail(st.calls);
      st.failed = true;
    }
    return st;
  }
}

DoLimitResponse HipRateLimitCache::DoLimit(const RateLimitRequest& request,
                                           const std::vector<std::shared_ptr<RateLimit>>& limits) {
  auto call = make_call(request, limits, *ts_);
  if (fc_) {
    // every lookup of the request before any of its INCRBYs (fixed_cache_impl.go:55-66)
    PendingCall& c = *call;
    c.lhit.assign(c.prefix.size(), 0);
    c.fkey.resize(c.prefix.size());
    std::lock_guard<std::mutex> g(fc_mu_);
    for (size_t i = 0; i < c.prefix.size(); ++i) {
      if (!limits[i]) continue;  // "" keys are skipped
      const int64_t div = unit_divider(limits[i]->Limit.unit);
      if (!div) continue;
      c.fkey[i] = c.prefix[i] + std::to_string(c.now / div * div);
      c.lhit[i] = fc_->Get(c.fkey[i], (uint32_t)c.now) ? 1 : 0;
    }
  }
  std::future<void> f = call->done.get_future();
  {
    std::lock_guard<std::mutex> g(mu_);
    q_.push_back(call);
    ++inflight_;  // until its batch is decided (Flush waits for 0)
  }
  cv_.notify_one();
  f.get();  // rethrows RedisError
  return std::move(call->resp);
}

uint32_t HipRateLimitCache::rule_id(const RateLimitLimit& l, bool shadow) {
  auto k = std::make_pair(l.RequestsPerUnit, (uint32_t)l.unit | (shadow ? RL_RULE_SHADOW : 0u));
  auto it = rule_ids_.find(k);
  if (it != rule_ids_.end()) return it->second;
  const uint32_t id = (uint32_t)rules_.size();
  rules_.push_back(rl_rule{l.RequestsPerUnit, k.second});
  rule_ids_.emplace(k, id);
  rules_dirty_ = true;
  return id;
}

static int64_t compact_base(int64_t first_now) { return first_now > 0 ? first_now - 1 : 0; }

// A call the compact form can carry: prefixes of at most 65535 bytes, hits_addend below 2^24 and
// rule ids (those it has and those it would be given) below 0xFFFF.
bool HipRateLimitCache::compactable(const PendingCall& c) const {
  if (s_.refund_rejected) return false;  // a refund reads statuses on the device: a compact batch leaves none there
  if (c.req->HitsAddend > 0xFFFFFFu) return false;
  size_t fresh = 0;
  for (size_t i = 0; i < c.prefix.size(); ++i) {
    if (c.prefix[i].size() > 0xFFFFu) return false;
    const auto& lim = (*c.limits)[i];
    if (!lim) continue;
    auto it = rule_ids_.find({lim->Limit.RequestsPerUnit, (uint32_t)lim->Limit.unit | (lim->ShadowMode ? RL_RULE_SHADOW : 0u)});
    if (it == rule_ids_.end()) ++fresh;
    else if (it->second >= RL_NIL_RULE16) return false;
  }
  return rules_.size() + fresh < RL_NIL_RULE16;
}

bool HipRateLimitCache::fits(const Staged& st, const PendingCall& c) const {
  if (st.calls.empty()) return true;
  if (st.compact && !compactable(c)) return false;  // starts a full-format batch
  const int64_t lo = c.now < st.tmin ? c.now : st.tmin, hi = c.now > st.tmax ? c.now : st.tmax;
  // A batch may straddle at most one window boundary of a unit (rl_submit refuses a SECOND key
  // spanning three windows), so it is cut before a request 2 s or more from the others; and
  // before one the slot cannot hold, or past HIP_BATCH_LIMIT descriptors.
  return hi - lo < 2 && st.nd + c.prefix.size() <= s_.batch_limit && st.nd + c.prefix.size() <= st.max_desc &&
         st.nr + 1 <= st.max_req && st.nb + c.blob_bytes <= st.max_blob;
}

// One request into the slot: GenerateCacheKey's bytes before the timestamp per descriptor with
// a limit (cache_key.go:57-65), the rule id, the request index; now and the raw HitsAddend.
void HipRateLimitCache::add(Staged& st, const std::shared_ptr<PendingCall>& cp) {
  PendingCall& c = *cp;
  if (st.calls.empty()) st.tmin = st.tmax = c.now;
  st.tmin = c.now < st.tmin ? c.now : st.tmin;
  st.tmax = c.now > st.tmax ? c.now : st.tmax;
  const uint32_t r = st.nr++;
  if (trace_) trace_(c.req, st.seq, r);
  if (st.compact) {
    // one word per request: hits_addend | (now - now_base) << 24, now_base = the batch's first
    // time minus one (the batch spans < 2 s, so the delta is 0..2)
    const int64_t base = compact_base(st.calls.empty() ? c.now : st.calls[0]->now);
    st.hc.req_word[r] = c.req->HitsAddend | (uint32_t)(c.now - base) << 24;
    if (c.prefix.size() != 1) st.one_per_req = false;
    for (size_t i = 0; i < c.prefix.size(); ++i) {
      const auto& lim = (*c.limits)[i];
      memcpy(st.hc.prefix_blob + st.nb, c.prefix[i].data(), c.prefix[i].size());
      st.nb += (uint32_t)c.prefix[i].size();
      // a local-cache hit goes as a nil descriptor: no INCRBY, and no jitter draw (:61-65)
      const bool inc = lim && (c.lhit.empty() || !c.lhit[i]);
      const uint32_t rid = inc ? rule_id(lim->Limit, lim->ShadowMode) : RL_NIL_RULE16;
      st.hc.desc_word[st.nd] = (uint32_t)c.prefix[i].size() | rid << 16;
      st.hc.req_of[st.nd] = r;  // (sent only when some request holds several descriptors)
      if (jitter_) st.hc.ttl_jitter[st.nd] = inc ? draw_jitter(s_) : 0;
      ++st.nd;
    }
    st.calls.push_back(cp);
    return;
  }
  st.hb.now[r] = c.now;
  st.hb.hits_addend[r] = c.req->HitsAddend;
  st.hb.prefix_off[0] = 0;
  for (size_t i = 0; i < c.prefix.size(); ++i) {
    const auto& lim = (*c.limits)[i];
    memcpy(st.hb.prefix_blob + st.nb, c.prefix[i].data(), c.prefix[i].size());
    st.nb += (uint32_t)c.prefix[i].size();
    const bool inc = lim && (c.lhit.empty() || !c.lhit[i]);
    st.hb.rule_id[st.nd] = inc ? rule_id(lim->Limit, lim->ShadowMode) : RL_NIL_RULE;
    st.hb.req_of[st.nd] = r;
    if (jitter_) st.hb.ttl_jitter[st.nd] = inc ? draw_jitter(s_) : 0;
    ++st.nd;
    st.hb.prefix_off[st.nd] = st.nb;
  }
  st.calls.push_back(cp);
}

void HipRateLimitCache::fail(std::vector<std::shared_ptr<PendingCall>>& calls) {
  // checkError -> panic(RedisError(...))  src/redis/driver_impl.go:50-54
  const std::string msg = std::string("hip backend: ") + rl_last_error(eng_);
  for (auto& c : calls) c->done.set_exception(std::make_exception_ptr(RedisError(msg)));
  done_calls(calls.size());
  calls.clear();
}

void HipRateLimitCache::done_calls(size_t n) {
  {
    std::lock_guard<std::mutex> g(mu_);
    inflight_ -= n;
  }
  idle_cv_.notify_all();
}

// Hand the slot's batch to the engine. New (L, unit) rules are appended to the device table
// first: that is allowed while the previous batch is in flight (rule ids keep their meaning,
// rl_hip.h rl_load_rules). Two things need nothing in flight (RL_ESTATE otherwise): a rule
// table that crosses V4_MAX_RULES or outgrows its allocation, and a second batch in flight once
// the engine runs the LSD pipeline (more than 32768 rules). Then the batches in flight are
// completed first (their callers answered) and the load / submit is made again; any other
// refusal fails this batch's calls, keeping the table dirty.
void HipRateLimitCache::submit(Staged& st, std::deque<Staged>& inflight) {
  for (int attempt = 0;; ++attempt) {
    int rc = 0;
    if (rules_dirty_) {
      rc = rl_load_rules(eng_, rules_.data(), (uint32_t)rules_.size());
      if (!rc) {
        rules_dirty_ = false;
        n_loads_ += 1;
        if (!inflight.empty()) n_loads_inflight_ += 1;
      }
    }
    if (!rc && st.compact) {
      rl_batch_c b;
      memset(&b, 0, sizeof b);
      b.n_desc = st.nd;
      b.n_req = st.nr;
      b.blob_bytes = st.nb;
      b.flags = st.one_per_req ? RL_BC_ONE_PER_REQ : 0u;
      b.now_base = compact_base(st.calls[0]->now);
      b.prefix_blob = st.hc.prefix_blob;  // the slot's own arrays: rl_submit_c does not copy them
      b.desc_word = st.hc.desc_word;
      b.req_word = st.hc.req_word;
      b.req_of = st.one_per_req ? nullptr : st.hc.req_of;
      b.ttl_jitter = jitter_ ? st.hc.ttl_jitter : nullptr;
      rc = rl_submit_c(eng_, &b);  // raw replies stay in the slot until rl_wait_raw_view
      if (!rc) n_batches_ += 1, n_compact_ += 1;
    } else if (!rc) {
      rl_batch b;
      memset(&b, 0, sizeof b);
      b.n_desc = st.nd;
      b.n_req = st.nr;
      b.blob_bytes = st.nb;
      b.prefix_blob = st.hb.prefix_blob;  // the slot's own arrays: rl_submit does not copy them
      b.prefix_off = st.hb.prefix_off;
      b.rule_id = st.hb.rule_id;
      b.req_of = st.hb.req_of;
      b.now = st.hb.now;
      b.hits_addend = st.hb.hits_addend;
      b.ttl_jitter = jitter_ ? st.hb.ttl_jitter : nullptr;
      rc = rl_submit(eng_, &b, nullptr, nullptr);  // results stay in the slot until rl_wait_view
      if (!rc) n_batches_ += 1;
    }
    if (rc == RL_ESTATE && attempt == 0 && !inflight.empty()) {
      // the slot acquired for this batch stays this batch's: completing the others submits nothing
      while (!inflight.empty()) {
        finish(inflight.front());
        inflight.pop_front();
      }
      n_drains_ += 1;
      continue;
    }
    if (rc) {
      fail(st.calls);
      st.failed = true;
    }
    return;
  }
}

// Collect the oldest batch in flight: rl_wait_view hands out its results in the slot's pinned
// memory (no copy), read here before the next submit reuses the slot.
void HipRateLimitCache::finish(Staged& st) {
  if (st.failed) return;
  if (st.refund) {
    // (nobody waits for it; a failed refund wrote nothing, and its batch's answers stand)
    if (rl_wait_refund(eng_, nullptr)) n_refund_fail_ += 1;
    return;
  }
  if (st.adjust) {
    // nothing was applied when the flight fails: every call of it gets the error
    adj_rep_.resize(st.nd ? st.nd : 1u);
    if (rl_wait_adjust(eng_, adj_rep_.data(), nullptr)) {
      fail(st.calls);
      return;
    }
    size_t d = 0;
    for (auto& cp : st.calls) {
      PendingCall& c = *cp;
      c.peek.resize(c.prefix.size());
      for (size_t i = 0; i < c.prefix.size(); ++i, ++d) {
        const rl_peek_reply& r = adj_rep_[d];
        PeekStatus& s = c.peek[i];
        s.Found = (r.flags & RL_PEEK_FOUND) != 0;
        s.LocalCached = (r.flags & RL_PEEK_LOCAL_CACHED) != 0;
        s.Count = r.count;
        s.TtlSeconds = r.ttl_s;
        s.CachedSeconds = r.cached_s;
      }
      c.done.set_value();
    }
    done_calls(st.calls.size());
    return;
  }
  const rl_status* out = nullptr;
  const uint32_t* thr = nullptr;
  if (st.compact) {
    // raw replies (the INCRBY post-values, fixed_cache_impl.go:91-102) -> statuses on the host:
    // GetResponseDescriptorStatus (base_limiter.go:70-195) by rl_decide_raw
    const rl_raw_reply* raw = nullptr;
    rl_batch_c b;
    memset(&b, 0, sizeof b);
    b.n_desc = st.nd;
    b.n_req = st.nr;
    b.blob_bytes = st.nb;
    b.flags = st.one_per_req ? RL_BC_ONE_PER_REQ : 0u;
    b.now_base = compact_base(st.calls[0]->now);
    b.prefix_blob = st.hc.prefix_blob;
    b.desc_word = st.hc.desc_word;  // the slot's inputs stay until it is acquired again
    b.req_word = st.hc.req_word;
    b.req_of = st.one_per_req ? nullptr : st.hc.req_of;
    if (dec_out_.size() < st.nd) dec_out_.resize(st.nd);
    if (dec_thr_.size() < st.nr) dec_thr_.resize(st.nr);
    if (rl_wait_raw_view(eng_, &raw) || rl_decide_raw(eng_, &b, raw, 0, st.nd, dec_out_.data(), dec_thr_.data())) {
      fail(st.calls);
      return;
    }
    out = dec_out_.data();
    thr = dec_thr_.data();
  } else if (rl_wait_view(eng_, &out, &thr)) {
    fail(st.calls);
    return;
  }
  size_t d = 0;
  for (size_t r = 0; r < st.calls.size(); ++r) {
    PendingCall& c = *st.calls[r];
    if (fc_) {
      // a reply past the limit Sets the key with TTL = the unit's divider (base_limiter.go:94-106),
      // shadow rules included (the limiter does not know them), before the caller is released
      std::lock_guard<std::mutex> g(fc_mu_);
      for (size_t i = 0; i < c.prefix.size(); ++i) {
        const auto& lim = (*c.limits)[i];
        if (!lim || c.lhit[i]) continue;
        const uint32_t cf = out[d + i].code_flags;
        if ((cf & 0xFFu) == RL_CODE_OVER_LIMIT || ((cf >> 8) & RL_FLAG_SHADOW))
          fc_->Set(c.fkey[i], unit_divider(lim->Limit.unit), (uint32_t)c.now);
      }
    }
    if (!fc_ && s_.local_cache) {
      // the device cache's lookup counters: one Get per descriptor with a limit
      // (fixed_cache_impl.go:55-66), a hit where the status says so, before the caller is released
      uint64_t looks = 0, hits = 0;
      for (size_t i = 0; i < c.prefix.size(); ++i) {
        if (!(*c.limits)[i]) continue;
        ++looks;
        hits += ((out[d + i].code_flags >> 8) & RL_FLAG_LOCAL_CACHE_HIT) ? 1u : 0u;
      }
      lc_lookups_.fetch_add(looks, std::memory_order_relaxed);
      lc_hits_.fetch_add(hits, std::memory_order_relaxed);
    }
    answer(c, out + d, thr[r]);
    d += c.prefix.size();
  }
  done_calls(st.calls.size());
}

// hits, misses, lookups, entries, evicted, expired. HIP_LOCAL_CACHE=freecache: the host model's.
// The device cache: hits / lookups as finish() counted them; entries / expired from an rl_census
// at the time source's now, a control call on the submitter thread (as Peek), so every DoLimit
// enqueued before it is decided first; evicted is 0, the device cache never evicts.
void HipRateLimitCache::local_cache_stats(uint64_t* out) {
  for (int k = 0; k < 6; ++k) out[k] = 0;
  {
    std::lock_guard<std::mutex> g(fc_mu_);
    if (fc_) {
      fc_->stats(out);
      return;
    }
  }
  if (!s_.local_cache) return;
  rl_census_report rep;
  memset(&rep, 0, sizeof rep);
  rep.struct_size = sizeof rep;
  control([this, &rep]() -> std::string { return rl_census(eng_, ts_->UnixNow(), &rep) ? rl_last_error(eng_) : ""; });
  const uint64_t hits = lc_hits_.load(std::memory_order_relaxed), looks = lc_lookups_.load(std::memory_order_relaxed);
  out[0] = hits;
  out[1] = looks - hits;
  out[2] = looks;
  for (int r = 0; r < 8; ++r) {
    out[3] += rep.cached[r];
    out[5] += rep.cache_expired[r];
  }
}

// The submitter thread owns the engine (rl_hip.h: one thread per engine) and keeps two batches
// in flight, as the Go batcher does: batch k+1 is gathered, built in its
// pinned slot and submitted (its H2D copy and fingerprint overlap batch k's kernels) before
// batch k's results are collected; with nothing queued it finishes what is in flight instead
// of waiting. Gathering lasts up to batch_window_us (implicit pipelining analogue,
// src/redis/driver_impl.go:84-89).
void HipRateLimitCache::submitter() {
  std::deque<Staged> inflight;
  std::shared_ptr<PendingCall> carry;
  for (;;) {
    std::shared_ptr<PendingCall> first = std::move(carry);
    carry.reset();
    if (!first) {
      std::unique_lock<std::mutex> g(mu_);
      if (!inflight.empty() && q_.empty()) {
        g.unlock();
        finish_oldest(inflight);
        continue;
      }
      cv_.wait(g, [&] { return stop_ || !q_.empty(); });
      if (q_.empty()) break;  // stopping
      first = q_.front();
      q_.pop_front();
    }
    if (first->ctl) {
      // every call enqueued before it is decided and answered; the engine is idle
      for (auto& st : inflight) finish(st);
      inflight.clear();
      autogrow(inflight);
      const std::string msg = first->ctl();
      if (grow_after_ctl_) {  // a Set: the auto-grow check, as after a completed batch
        grow_after_ctl_ = false;
        autogrow(inflight);
      }
      if (msg.empty()) first->done.set_value();
      else first->done.set_exception(std::make_exception_ptr(RedisError("hip backend: " + msg)));
      done_calls(1);
      continue;
    }
    // a flight of either kind takes a slot: the one acquired here is free once at most two are in flight
    while (inflight.size() >= RL_MAX_IN_FLIGHT) finish_oldest(inflight);
    Staged st;
    st.seq = staged_seq_++;
    AdjGather ag[2];  // the gather's queued adjusts without / with keep_cache
    // The slot in both layouts (the same memory): the first decision call picks one. A gather of
    // adjusts alone leaves it unused.
    if (rl_host_acquire_c(eng_, &st.hc) || rl_host_acquire(eng_, &st.hb)) {
      std::vector<std::shared_ptr<PendingCall>> one{first};
      fail(one);
      continue;
    }
    // the first decision call of the gather: the batch's format and the slot's room (false: a request no slot holds)
    auto begin_decision = [&](const PendingCall& c) {
      st.compact = compactable(c);
      st.max_desc = st.compact ? st.hc.max_desc : st.hb.max_desc;
      st.max_req = st.compact ? st.hc.max_req : st.hb.max_req;
      st.max_blob = st.compact ? st.hc.max_blob : st.hb.max_blob;
      return c.prefix.size() <= st.max_desc && c.blob_bytes <= st.max_blob;
    };
    if (first->adj_queued) {
      add_adjust(ag[first->keep], first, st.seq);
    } else {
      if (!begin_decision(*first)) {
        first->done.set_exception(std::make_exception_ptr(RedisError("hip backend: request larger than a batch")));
        done_calls(1);
        continue;
      }
      add(st, first);
    }
    {
      std::unique_lock<std::mutex> g(mu_);
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(s_.batch_window_us);
      for (;;) {
        while (!q_.empty()) {
          std::shared_ptr<PendingCall> c = q_.front();
          q_.pop_front();
          // (a decision call the slot cannot hold as the batch's first is refused as the next gather's first)
          const bool ok = c->ctl          ? false
                          : c->adj_queued ? fits_adjust(ag[c->keep], *c)
                          : st.calls.empty() ? begin_decision(*c)
                                             : fits(st, *c);
          if (!ok) {
            carry = std::move(c);  // starts the next batch (a control call: runs after this one)
            goto full;
          }
          if (c->adj_queued) add_adjust(ag[c->keep], c, st.seq);
          else add(st, c);
        }
        if (stop_ || st.nd >= s_.batch_limit) break;
        if (!inflight.empty() && s_.answer_early) {
          // while gathering, answer the batch in flight as soon as the device is done with it
          // (rl_query), not when this window closes: under light load a caller's latency is then
          // its batch's own, not that plus the next batch's window
          g.unlock();
          const int qr = rl_query(eng_);
          if (qr == 1) finish_oldest(inflight);
          g.lock();
          if (qr == 1) continue;
          const auto slice = std::min(deadline, std::chrono::steady_clock::now() + std::chrono::microseconds(10));
          cv_.wait_until(g, slice);
        } else if (cv_.wait_until(g, deadline) == std::cv_status::timeout && q_.empty()) {
          break;
        }
        if (std::chrono::steady_clock::now() >= deadline) break;
      }
    full:;
    }
    // The decision batch first: it was built in the slot of the next flight. The adjust flights go
    // behind it; all calls of one gather are concurrent, so that is a legal serial order, and the
    // trace hook's positions say so (kTraceAdjust sorts behind every request position).
    const uint64_t seq = st.seq;
    if (!st.calls.empty()) {
      submit(st, inflight);
      const bool decided = !st.failed;
      inflight.push_back(std::move(st));
      // HIP_REFUND_REJECTED: the batch's rejected requests get their hits back, right behind it and
      // in front of the gather's adjusts. Completing older flights for room never reaches the batch
      // itself: it is the newest of at most RL_MAX_IN_FLIGHT.
      if (s_.refund_rejected && decided) {
        while (inflight.size() >= RL_MAX_IN_FLIGHT) finish_oldest(inflight);
        Staged rf;
        rf.adjust = rf.refund = true;
        rf.seq = seq;
        // HIP_LOCAL_CACHE=freecache: the device cache is unused, as in Adjust
        if (rl_refund_behind(eng_, fc_ ? (uint32_t)RL_REFUND_KEEP_CACHE : 0u)) {
          n_refund_fail_ += 1;  // (the engine refused it: the batch stays charged as the reference charges it)
        } else {
          n_refunds_ += 1;
          inflight.push_back(std::move(rf));
        }
      }
    }
    for (int k = 0; k < 2; ++k) {
      if (ag[k].calls.empty()) continue;
      while (inflight.size() >= RL_MAX_IN_FLIGHT) finish_oldest(inflight);
      inflight.push_back(submit_adjust(ag[k], k == 1, seq, inflight));
    }
    // one decision batch stays in flight while the next is gathered, as before; with it at most one other flight
    auto decisions = [&] {
      size_t n = 0;
      for (auto& f : inflight) n += f.adjust ? 0u : 1u;
      return n;
    };
    while (decisions() >= 2 || inflight.size() >= RL_MAX_IN_FLIGHT) finish_oldest(inflight);
  }
  for (auto& st : inflight) finish(st);
}

// ---- HipRoutedRateLimitCache ------------------------------------------------------------
struct HipRoutedRateLimitCache::Step {
  std::vector<std::shared_ptr<PendingCall>> calls;
  uint32_t nd = 0, nr = 0, nb = 0;
  int64_t tmin = 0, tmax = 0;
};

namespace {
// One rank's words in a rule / stop agreement (rl_router_allgather_host, RL_ROUTER_AG_MAX bytes).
constexpr uint32_t SYNC_RULES = (RL_ROUTER_AG_MAX - 40) / sizeof(rl_rule);
struct SyncWords {
  uint32_t stop, n;
  uint32_t n_peek, n_forget, n_set;  // pending Peek / Forget / Set calls of this rank
  uint32_t n_adj, n_adj_keep;        // pending Adjust calls without / with keep_cache
  uint32_t n_ref, n_ref_keep, pad;   // pending refunds of rejected requests without / with keep_cache
  rl_rule rules[SYNC_RULES];
};
static_assert(sizeof(SyncWords) <= RL_ROUTER_AG_MAX, "sync words");
std::pair<uint32_t, uint32_t> limit_key(const RateLimit& r) {
  return {r.Limit.RequestsPerUnit, (uint32_t)r.Limit.unit | (r.ShadowMode ? RL_RULE_SHADOW : 0u)};
}
}  // namespace

HipRoutedRateLimitCache::HipRoutedRateLimitCache(const HipSettings& s, const HipRoutedSettings& r,
                                                 std::shared_ptr<TimeSource> ts)
    : s_(s), r_(r), ts_(std::move(ts)) {
  jitter_ = setup_jitter(s_);
  if (r.id.size() != RL_ROUTER_ID_BYTES) throw RedisError("routed cache: id must hold RL_ROUTER_ID_BYTES bytes");
  if (s.local_cache && s.local_cache_freecache)
    throw RedisError("routed cache: HIP_LOCAL_CACHE=freecache is single-engine only (the device cache is the routed one)");
  rl_config c;
  memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.device = s.device;
  for (int u = 0; u < 4; ++u) c.log2_slots[u] = s.log2_slots[u];
  c.near_limit_ratio = s.near_limit_ratio;
  c.local_cache = s.local_cache ? 1 : 0;
  c.per_second_split = s.per_second_split ? 1 : 0;
  // an owner may receive every origin's whole batch (a key hot everywhere)
  c.max_batch_desc = s.batch_limit * r.n_shards;
  c.max_batch_req = s.batch_limit * r.n_shards;
  c.max_blob_bytes = s.batch_limit * 128u;
  c.hash_seed = s.hash_seed;
  c.max_load_permille = s.max_load_permille;
  int rc = rl_create(&c, &eng_);
  if (rc) throw RedisError("rl_create failed: " + std::to_string(rc) + ": " + rl_last_error(nullptr));
  rl_router_config rc2;
  memset(&rc2, 0, sizeof rc2);
  rc2.struct_size = sizeof rc2;
  rc2.n_shards = r.n_shards;
  rc2.rank = r.rank;
  rc2.max_desc = s.batch_limit;
  rc2.rccl_id = r.id.data();
  rc2.flags = RL_ROUTER_HOST | (r.emulated ? RL_ROUTER_EMULATED : 0u);
  rc2.max_blob_bytes = s.batch_limit * 128u;
  rl_engine* es[1] = {eng_};
  rc = rl_router_create(&rc2, es, &rt_);
  if (rc) {
    rl_destroy(eng_);
    throw RedisError("rl_router_create failed: " + std::to_string(rc));
  }
  thr_ = std::thread([this] { submitter(); });
}

HipRoutedRateLimitCache::~HipRoutedRateLimitCache() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  thr_.join();
  rl_router_destroy(rt_);
  rl_destroy(eng_);
}

void HipRoutedRateLimitCache::Flush() {
  std::unique_lock<std::mutex> g(mu_);
  idle_cv_.wait(g, [&] { return inflight_ == 0; });
}

DoLimitResponse HipRoutedRateLimitCache::DoLimit(const RateLimitRequest& request,
                                                 const std::vector<std::shared_ptr<RateLimit>>& limits) {
  auto call = make_call(request, limits, *ts_);
  std::future<void> f = call->done.get_future();
  {
    std::lock_guard<std::mutex> g(mu_);
    if (broken_) throw RedisError("hip backend: " + broken_msg_);
    q_.push_back(call);
    ++inflight_;
  }
  cv_.notify_one();
  f.get();  // rethrows RedisError
  return std::move(call->resp);
}

void HipRoutedRateLimitCache::done_calls(size_t n) {
  {
    std::lock_guard<std::mutex> g(mu_);
    inflight_ -= n;
  }
  idle_cv_.notify_all();
}

void HipRoutedRateLimitCache::fail(std::vector<std::shared_ptr<PendingCall>>& calls, const std::string& msg) {
  for (auto& c : calls) c->done.set_exception(std::make_exception_ptr(RedisError("hip backend: " + msg)));
  done_calls(calls.size());
  calls.clear();
}

// Every limit of the call has an agreed id; otherwise its new limits are queued for the next sync.
bool HipRoutedRateLimitCache::known(const PendingCall& c) {
  bool ok = true;
  for (const auto& lim : *c.limits) {
    if (!lim) continue;
    const auto k = limit_key(*lim);
    if (ids_.count(k)) continue;
    ok = false;
    if (pending_set_.insert(k).second) pending_.push_back(rl_rule{k.first, k.second});
  }
  return ok;
}

// The rule / stop agreement (nothing in flight on any rank): every rank's new limits appended to
// every rank's table in rank order (the first occurrence keeps its id), loaded into the engine.
// Returns true when every rank asked to stop.
// Then the control calls: first the refunds of the requests the steps before rejected
// (HIP_REFUND_REJECTED; rl_router_refund, without the keep bit and with it: its flags word is per
// origin), so that every caller's control call of this agreement sees them; then, if any rank has
// pending Peeks every rank makes one rl_router_peek, then the same for Forgets, then for Sets
// (rl_router_set), then for Adjusts without keep_cache and for Adjusts with it (rl_router_adjust:
// its flags word is per origin too, hence the two calls).
bool HipRoutedRateLimitCache::sync(bool want_stop, std::deque<std::shared_ptr<PendingCall>>& ctl, uint64_t seq) {
  SyncWords mine;
  memset(&mine, 0, sizeof mine);
  mine.stop = want_stop ? 1u : 0u;
  for (const auto& c : ctl)
    (c->kind == 1   ? mine.n_peek
     : c->kind == 2 ? mine.n_forget
     : c->kind == 3 ? mine.n_set
     : c->kind == 4 ? mine.n_adj
     : c->kind == 5 ? mine.n_adj_keep
     : c->kind == 6 ? mine.n_ref
                    : mine.n_ref_keep) += 1;
  mine.n = (uint32_t)std::min<size_t>(pending_.size(), SYNC_RULES);
  std::copy(pending_.begin(), pending_.begin() + mine.n, mine.rules);
  std::vector<SyncWords> all(r_.n_shards);
  int rc = rl_router_allgather_host(rt_, &mine, sizeof mine, all.data());
  if (rc) throw RedisError(std::string("rule agreement: ") + rl_router_last_error(rt_));
  n_syncs_ += 1;
  bool all_stop = true, any_peek = false, any_forget = false, any_set = false, any_adj = false, any_adj_keep = false;
  bool any_ref = false, any_ref_keep = false;
  const size_t before = rules_.size();
  for (const SyncWords& w : all) {
    all_stop &= w.stop != 0;
    any_peek |= w.n_peek != 0;
    any_forget |= w.n_forget != 0;
    any_set |= w.n_set != 0;
    any_adj |= w.n_adj != 0;
    any_adj_keep |= w.n_adj_keep != 0;
    any_ref |= w.n_ref != 0;
    any_ref_keep |= w.n_ref_keep != 0;
    for (uint32_t i = 0; i < w.n; ++i) {
      const auto k = std::make_pair(w.rules[i].requests_per_unit, w.rules[i].unit);
      if (ids_.emplace(k, (uint32_t)rules_.size()).second) rules_.push_back(w.rules[i]);
    }
  }
  for (uint32_t i = 0; i < mine.n; ++i)
    pending_set_.erase(std::make_pair(pending_[i].requests_per_unit, pending_[i].unit));
  pending_.erase(pending_.begin(), pending_.begin() + mine.n);
  if (rules_.size() != before) {
    rc = rl_load_rules(eng_, rules_.data(), (uint32_t)rules_.size());
    if (rc) throw RedisError(std::string("rl_load_rules: ") + rl_last_error(eng_));
    n_rules_ = rules_.size();
  }
  if (any_ref) run_control(6, ctl, seq);
  if (any_ref_keep) run_control(7, ctl, seq);
  if (any_peek) run_control(1, ctl, seq);
  if (any_forget) run_control(2, ctl, seq);
  if (any_set) run_control(3, ctl, seq);
  if (any_adj) run_control(4, ctl, seq);
  if (any_adj_keep) run_control(5, ctl, seq);
  return all_stop;
}

// One collective rl_router_peek (kind 1) / rl_router_forget (kind 2) / rl_router_set (kind 3) /
// rl_router_adjust (kind 4; kind 5 with RL_ADJUST_KEEP_CACHE) / rl_router_refund (kind 6; kind 7
// with RL_REFUND_KEEP_CACHE) at an agreement: this rank's pending calls of the kind whose limits are
// agreed, in enqueue order, as one request each, as far as one router batch holds them (the others
// wait for the following agreement); an empty batch when there are none. A refund is a rejected
// request as it was decided: its own time, rule ids, HitsAddend and statuses.
void HipRoutedRateLimitCache::run_control(int kind, std::deque<std::shared_ptr<PendingCall>>& ctl, uint64_t seq) {
  std::vector<std::shared_ptr<PendingCall>> calls;
  std::vector<uint8_t> blob;
  std::vector<uint32_t> off(1, 0u), rule, req_of;
  std::vector<int64_t> now;
  std::vector<rl_peek_reply> val;  // (a Set's)
  std::vector<int32_t> dl;         // (an Adjust's)
  std::vector<uint32_t> hits;      // (a refund's)
  std::vector<rl_status> sts;      // (a refund's)
  const bool refund = kind == 6 || kind == 7;
  const size_t max_blob = (size_t)s_.batch_limit * 128u;
  for (auto it = ctl.begin(); it != ctl.end();) {
    PendingCall& c = **it;
    if (c.kind != kind || (!refund && !known(c))) {  // (a refund's rule ids were agreed when it was decided)
      ++it;
      continue;
    }
    if (rule.size() + c.prefix.size() > s_.batch_limit || now.size() + 1 > s_.batch_limit ||
        blob.size() + c.blob_bytes > max_blob)
      break;  // (enqueue order: the rest of the kind waits too)
    if (trace_) trace_(c.req, seq, kTraceControl);
    const uint32_t rq = (uint32_t)now.size();
    now.push_back(refund ? c.now : ts_->UnixNow());
    for (size_t i = 0; i < c.prefix.size(); ++i) {
      blob.insert(blob.end(), c.prefix[i].begin(), c.prefix[i].end());
      off.push_back((uint32_t)blob.size());
      if (refund) {
        rule.push_back(c.rule_ids[i]);
      } else {
        const auto& lim = (*c.limits)[i];
        rule.push_back(lim ? ids_.at(limit_key(*lim)) : RL_NIL_RULE);
      }
      req_of.push_back(rq);
    }
    if (refund) {
      hits.push_back(c.hits);
      sts.insert(sts.end(), c.statuses.begin(), c.statuses.end());
    }
    val.insert(val.end(), c.set_vals.begin(), c.set_vals.end());
    dl.insert(dl.end(), c.deltas.begin(), c.deltas.end());
    calls.push_back(*it);
    it = ctl.erase(it);
  }
  rl_batch b;
  memset(&b, 0, sizeof b);
  b.n_desc = (uint32_t)rule.size();
  b.n_req = (uint32_t)now.size();
  b.blob_bytes = (uint32_t)blob.size();
  b.prefix_blob = blob.data();
  b.prefix_off = off.data();
  b.rule_id = rule.data();
  b.req_of = req_of.data();
  b.now = now.data();
  std::vector<rl_peek_reply> rep(std::max<size_t>(1, rule.size()));
  rl_peek_reply* outs[1] = {rep.data()};
  val.resize(std::max<size_t>(1, val.size()));
  const rl_peek_reply* vals[1] = {val.data()};
  dl.resize(std::max<size_t>(1, dl.size()));
  const int32_t* dls[1] = {dl.data()};
  const uint32_t flags[1] = {kind == 5 || kind == 7 ? (uint32_t)RL_ADJUST_KEEP_CACHE : 0u};
  static_assert((uint32_t)RL_REFUND_KEEP_CACHE == (uint32_t)RL_ADJUST_KEEP_CACHE, "one keep bit");
  hits.resize(std::max<size_t>(1, hits.size()));
  sts.resize(std::max<size_t>(1, sts.size()));
  b.hits_addend = refund ? hits.data() : nullptr;
  const rl_status* stp[1] = {sts.data()};
  const int rc = kind == 1   ? rl_router_peek(rt_, &b, outs)
                 : kind == 2 ? rl_router_forget(rt_, &b, outs)
                 : kind == 3 ? rl_router_set(rt_, &b, vals, outs)
                 : refund    ? rl_router_refund(rt_, &b, stp, flags, nullptr, nullptr, nullptr)
                             : rl_router_adjust(rt_, &b, dls, flags, outs, nullptr);
  if (refund && !calls.empty()) (rc ? n_refund_fail_ : n_refunds_) += 1;
  if (rc) {
    const std::string msg = rl_router_last_error(rt_);
    fail(calls, msg);
    if (rc == RL_ECOMM) throw RedisError(msg);  // the communicator is gone: the cache is broken
    return;
  }
  if (refund) {  // nobody waits for these
    done_calls(calls.size());
    return;
  }
  size_t d = 0;
  for (auto& cp : calls) {
    PendingCall& c = *cp;
    c.peek.resize(c.prefix.size());
    for (size_t i = 0; i < c.prefix.size(); ++i, ++d) {
      PeekStatus& s = c.peek[i];
      s.Found = (rep[d].flags & RL_PEEK_FOUND) != 0;
      s.LocalCached = (rep[d].flags & RL_PEEK_LOCAL_CACHED) != 0;
      s.Count = rep[d].count;
      s.TtlSeconds = rep[d].ttl_s;
      s.CachedSeconds = rep[d].cached_s;
    }
    c.done.set_value();
  }
  done_calls(calls.size());
}

// Peek / Forget / Set: the caller's side. GenerateCacheKey prefixes as DoLimit builds them (no hit, no
// stat), queued behind the calls enqueued before; the submitter keeps it for the next agreement.
std::vector<PeekStatus> HipRoutedRateLimitCache::peek_call(const RateLimitRequest& request,
                                                           const std::vector<std::shared_ptr<RateLimit>>& limits,
                                                           int kind, const std::vector<PeekStatus>* values,
                                                           uint32_t keep, const std::vector<int32_t>* deltas) {
  if (request.Descriptors.size() != limits.size())
    throw std::logic_error("assert: len(request.Descriptors) == len(limits)");
  if (values && values->size() != limits.size()) throw std::logic_error("assert: len(values) == len(limits)");
  if (deltas && deltas->size() != limits.size()) throw std::logic_error("assert: len(deltas) == len(limits)");
  auto call = std::make_shared<PendingCall>();
  if (deltas) call->deltas = *deltas;
  if (values) {
    call->set_vals.resize(values->size());
    for (size_t i = 0; i < values->size(); ++i) {
      const PeekStatus& v = (*values)[i];
      call->set_vals[i] = rl_peek_reply{v.Count, v.TtlSeconds, v.CachedSeconds,
                                        (v.Found ? (uint32_t)RL_PEEK_FOUND : 0u) |
                                            (v.LocalCached ? (uint32_t)RL_PEEK_LOCAL_CACHED : 0u) | keep};
    }
  }
  call->req = &request;
  call->limits = &limits;
  call->kind = kind;
  call->prefix.resize(limits.size());
  for (size_t i = 0; i < limits.size(); ++i) {
    if (!limits[i]) continue;
    std::string& p = call->prefix[i];
    p = request.Domain;
    p += '_';
    for (const auto& e : request.Descriptors[i].Entries) {
      p += e.Key;
      p += '_';
      p += e.Value;
      p += '_';
    }
    call->blob_bytes += p.size();
  }
  if (limits.size() > s_.batch_limit || call->blob_bytes > (size_t)s_.batch_limit * 128u)
    throw RedisError("hip backend: the request exceeds one router batch (HIP_BATCH_LIMIT)");
  std::future<void> f = call->done.get_future();
  {
    std::lock_guard<std::mutex> g(mu_);
    if (broken_) throw RedisError("hip backend: " + broken_msg_);
    q_.push_back(call);
    ++inflight_;
  }
  cv_.notify_one();
  f.get();  // rethrows RedisError
  return std::move(call->peek);
}

std::vector<PeekStatus> HipRoutedRateLimitCache::Peek(const RateLimitRequest& request,
                                                      const std::vector<std::shared_ptr<RateLimit>>& limits) {
  return peek_call(request, limits, 1);
}

std::vector<PeekStatus> HipRoutedRateLimitCache::Forget(const RateLimitRequest& request,
                                                        const std::vector<std::shared_ptr<RateLimit>>& limits) {
  return peek_call(request, limits, 2);
}

std::vector<PeekStatus> HipRoutedRateLimitCache::Set(const RateLimitRequest& request,
                                                     const std::vector<std::shared_ptr<RateLimit>>& limits,
                                                     const std::vector<PeekStatus>& values, bool keep_counter,
                                                     bool keep_cache) {
  const uint32_t keep = (keep_counter ? (uint32_t)RL_SET_KEEP_COUNTER : 0u) |
                        (keep_cache ? (uint32_t)RL_SET_KEEP_CACHE : 0u);
  return peek_call(request, limits, 3, &values, keep);
}

std::vector<PeekStatus> HipRoutedRateLimitCache::Adjust(const RateLimitRequest& request,
                                                        const std::vector<std::shared_ptr<RateLimit>>& limits,
                                                        const std::vector<int32_t>& deltas, bool keep_cache) {
  return peek_call(request, limits, keep_cache ? 5 : 4, nullptr, 0, &deltas);
}

// The rank's step loop: rule / stop agreement every rule_sync_every steps (nothing in flight),
// otherwise gather for one step period, submit (an empty batch when idle), two steps in flight.
void HipRoutedRateLimitCache::submitter() {
  std::deque<Step> fl;
  std::deque<std::shared_ptr<PendingCall>> held;  // calls waiting for a rule agreement
  std::deque<std::shared_ptr<PendingCall>> ctl;   // Peek / Forget calls waiting for the next agreement
  std::vector<rl_status> out;
  std::vector<uint32_t> thr;
  uint64_t seq = 0;
  // HIP_REFUND_REJECTED: a request one of whose descriptors came back over its limit is queued as
  // a control call of the batcher's own, for the next agreement (rl_router_refund there decides
  // which of its descriptors are owed)
  auto queue_refund = [&](const PendingCall& c, const rl_status* out) {
    bool rejected = false;
    for (size_t i = 0; i < c.prefix.size(); ++i) rejected |= (out[i].code_flags & 0xFFu) == (uint32_t)RL_CODE_OVER_LIMIT;
    if (!rejected) return;
    auto rf = std::make_shared<PendingCall>();
    rf->kind = s_.local_cache && s_.local_cache_freecache ? 7 : 6;
    rf->now = c.now;
    rf->hits = c.req->HitsAddend;
    rf->prefix = c.prefix;
    rf->blob_bytes = c.blob_bytes;
    rf->statuses.assign(out, out + c.prefix.size());
    for (const auto& lim : *c.limits) rf->rule_ids.push_back(lim ? ids_.at(limit_key(*lim)) : RL_NIL_RULE);
    {
      std::lock_guard<std::mutex> g(mu_);
      ++inflight_;
    }
    ctl.push_back(std::move(rf));
  };
  auto finish_one = [&] {
    Step st = std::move(fl.front());
    fl.pop_front();
    out.resize(std::max<size_t>(1, st.nd));
    thr.resize(std::max<size_t>(1, st.nr));
    rl_status* o[1] = {out.data()};
    uint32_t* t[1] = {thr.data()};
    const int rc = rl_router_wait_into(rt_, o, t);
    if (rc) {
      if (rc == RL_ECOMM) {
        std::lock_guard<std::mutex> g(mu_);
        broken_ = true;
        broken_msg_ = rl_router_last_error(rt_);
      }
      fail(st.calls, rl_router_last_error(rt_));
      return;
    }
    size_t d = 0;
    for (size_t r = 0; r < st.calls.size(); ++r) {
      PendingCall& c = *st.calls[r];
      if (s_.refund_rejected) queue_refund(c, out.data() + d);  // (before the caller is released)
      answer(c, out.data() + d, thr[r]);
      d += c.prefix.size();
    }
    done_calls(st.calls.size());
  };
  auto fail_all = [&](const std::string& msg) {
    while (!fl.empty()) {
      fail(fl.front().calls, msg);
      fl.pop_front();
    }
    std::vector<std::shared_ptr<PendingCall>> rest(held.begin(), held.end());
    held.clear();
    rest.insert(rest.end(), ctl.begin(), ctl.end());
    ctl.clear();
    {
      std::lock_guard<std::mutex> g(mu_);
      broken_ = true;
      broken_msg_ = msg;
      rest.insert(rest.end(), q_.begin(), q_.end());
      q_.clear();
    }
    fail(rest, msg);
  };
  try {
    for (;;) {
      if (broken_) break;
      if (seq % r_.rule_sync_every == 0) {
        while (!fl.empty()) finish_one();
        bool want_stop;
        {
          std::lock_guard<std::mutex> g(mu_);
          want_stop = stop_ && q_.empty() && held.empty() && ctl.empty();
        }
        if (sync(want_stop, ctl, seq)) break;  // every rank stops here
        if (!held.empty()) {  // calls whose limits are agreed now go back to the front, in order
          std::lock_guard<std::mutex> g(mu_);
          for (auto it = held.rbegin(); it != held.rend(); ++it) q_.push_front(*it);
          held.clear();
        }
      }
      Step st;
      rl_host_batch hb;
      if (rl_router_host_acquire(rt_, 0, &hb)) throw RedisError(rl_router_last_error(rt_));
      {
        std::unique_lock<std::mutex> g(mu_);
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(r_.step_us);
        for (;;) {
          while (!q_.empty()) {
            std::shared_ptr<PendingCall> cp = q_.front();
            PendingCall& c = *cp;
            if (c.kind) {  // a Peek / Forget: runs at the next agreement (its new limits are queued for it)
              (void)known(c);
              ctl.push_back(cp);
              q_.pop_front();
              continue;
            }
            if (!known(c)) {  // waits for the next agreement
              held.push_back(cp);
              q_.pop_front();
              n_held_ += 1;
              continue;
            }
            const int64_t lo = st.calls.empty() ? c.now : std::min(st.tmin, c.now);
            const int64_t hi = st.calls.empty() ? c.now : std::max(st.tmax, c.now);
            // one batch straddles at most one window boundary (hi - lo < 2), and fits the slot
            if (hi - lo >= 2 || st.nd + c.prefix.size() > s_.batch_limit || st.nd + c.prefix.size() > hb.max_desc ||
                st.nr + 1 > hb.max_req || st.nb + c.blob_bytes > hb.max_blob)
              goto full;
            q_.pop_front();
            st.tmin = lo;
            st.tmax = hi;
            const uint32_t rq = st.nr++;
            if (trace_) trace_(c.req, seq, rq);
            hb.now[rq] = c.now;
            hb.hits_addend[rq] = c.req->HitsAddend;
            hb.prefix_off[0] = 0;
            for (size_t i = 0; i < c.prefix.size(); ++i) {
              const auto& lim = (*c.limits)[i];
              memcpy(hb.prefix_blob + st.nb, c.prefix[i].data(), c.prefix[i].size());
              st.nb += (uint32_t)c.prefix[i].size();
              hb.rule_id[st.nd] = lim ? ids_.at(limit_key(*lim)) : RL_NIL_RULE;
              hb.req_of[st.nd] = rq;
              if (jitter_) hb.ttl_jitter[st.nd] = lim ? draw_jitter(s_) : 0;
              ++st.nd;
              hb.prefix_off[st.nd] = st.nb;
            }
            st.calls.push_back(cp);
          }
          if (st.nd >= s_.batch_limit) break;
          if (cv_.wait_until(g, deadline) == std::cv_status::timeout) break;
          if (std::chrono::steady_clock::now() >= deadline) break;
        }
      full:;
      }
      rl_batch b;
      memset(&b, 0, sizeof b);
      b.n_desc = st.nd;
      b.n_req = st.nr;
      b.blob_bytes = st.nb;
      if (st.nd || st.nr) {
        b.prefix_blob = hb.prefix_blob;  // the router's pinned slot: staged without a copy
        b.prefix_off = hb.prefix_off;
        b.rule_id = hb.rule_id;
        b.req_of = hb.req_of;
        b.now = hb.now;
        b.hits_addend = hb.hits_addend;
        b.ttl_jitter = jitter_ ? hb.ttl_jitter : nullptr;
      } else {
        n_empty_ += 1;  // an idle rank still takes part in the step's collectives
      }
      const int rc = rl_router_submit_host(rt_, &b);
      ++seq;
      n_steps_ += 1;
      if (rc) {  // refused before its collectives (a broken communicator): this rank cannot step on
        const std::string msg = rl_router_last_error(rt_);
        fail(st.calls, msg);
        throw RedisError(msg);
      }
      fl.push_back(std::move(st));
      if (fl.size() == 2) finish_one();
    }
  } catch (const RedisError& e) {
    fail_all(e.what());
  }
  while (!fl.empty()) finish_one();
}

}  // namespace ratelimit
