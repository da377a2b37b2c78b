// rl_cache.hpp — C++ mirror of the reference's backend plugin interface, implemented on
// the HIP engine (include/rl_hip.h).
//
// The reference host code is Go; its toolchain is absent here, so this is the host side
// above the C ABI, with the same names, argument meaning and error behaviour:
//   limiter.RateLimitCache{DoLimit, Flush}            src/limiter/cache.go:15-33
//   limiter.DoLimitResponse                            src/limiter/cache.go:9-12
//   config.RateLimit / config.RateLimitStats           src/config/config.go:18-32
//   redis.RedisError (thrown, Go panics)               src/redis/driver.go:6-10
//   utils.TimeSource                                   src/utils/utilities.go:10-14
//   redis.NewFixedRateLimitCacheImpl (constructor)     src/redis/fixed_cache_impl.go:128-135
// DoLimit may be called concurrently from many threads (as grpc-go does); calls are
// micro-batched by one submitter thread (REDIS_PIPELINE_WINDOW / _LIMIT analogue,
// src/settings/settings.go:32-33), and the batch order is the serial order.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "rl_freecache.hpp"
#include "rl_hip.h"

namespace ratelimit {

// pb.RateLimitResponse_RateLimit_Unit / _Code
enum class Unit : uint32_t { UNKNOWN = 0, SECOND = 1, MINUTE = 2, HOUR = 3, DAY = 4 };
enum class Code : uint32_t { UNKNOWN = 0, OK = 1, OVER_LIMIT = 2 };

// gostats counter (additive only)
class Counter {
 public:
  void Add(uint64_t d) { v_.fetch_add(d, std::memory_order_relaxed); }
  uint64_t Value() const { return v_.load(std::memory_order_relaxed); }

 private:
  std::atomic<uint64_t> v_{0};
};

// config.RateLimitStats  src/config/config.go:18-23
struct RateLimitStats {
  Counter TotalHits, OverLimit, NearLimit, OverLimitWithLocalCache;
  Counter ShadowMode;  // extension (rl_hip.h RL_RULE_SHADOW): over-limit decisions reported as OK
};

// Stats scope: counters are shared by name (`<FullKey>.total_hits` ...), like
// statsScope.NewCounter returning the existing counter (config_impl.go:64-71,281-289).
class StatsStore {
 public:
  std::shared_ptr<RateLimitStats> Get(const std::string& key);

 private:
  std::mutex mu_;
  std::unordered_map<std::string, std::shared_ptr<RateLimitStats>> m_;
};

// pb.RateLimitResponse_RateLimit
struct RateLimitLimit {
  uint32_t RequestsPerUnit = 0;
  Unit unit = Unit::UNKNOWN;
};

// config.RateLimit  src/config/config.go:26-32
struct RateLimit {
  std::string FullKey;
  std::shared_ptr<RateLimitStats> Stats;
  RateLimitLimit Limit;
  bool SleepOnThrottle = false;
  bool ReportDetails = false;
  bool ShadowMode = false;  // extension (rl_hip.h RL_RULE_SHADOW); the fork's config has no shadow_mode key
};
// config.NewRateLimit  src/config/config_impl.go:79-89
std::shared_ptr<RateLimit> NewRateLimit(uint32_t requests_per_unit, Unit unit, const std::string& key,
                                        StatsStore& scope, bool sleep_on_throttle, bool report_details);

struct DescriptorEntry {
  std::string Key, Value;
};
struct RateLimitDescriptor {
  std::vector<DescriptorEntry> Entries;
};
// pb.RateLimitRequest
struct RateLimitRequest {
  std::string Domain;
  std::vector<RateLimitDescriptor> Descriptors;
  uint32_t HitsAddend = 0;
};

// pb.RateLimitResponse_DescriptorStatus
struct DescriptorStatus {
  Code code = Code::UNKNOWN;
  const RateLimitLimit* CurrentLimit = nullptr;  // nil when no limit applies
  uint32_t LimitRemaining = 0;
  bool HasDurationUntilReset = false;
  int64_t DurationUntilResetSeconds = 0;
  bool operator==(const DescriptorStatus& o) const;
};

// limiter.DoLimitResponse  src/limiter/cache.go:9-12
struct DoLimitResponse {
  std::vector<DescriptorStatus> DescriptorStatuses;
  uint32_t ThrottleMillis = 0;
};

// redis.RedisError — the only backend failure the service recovers
// (src/service/ratelimit.go:276-281).
class RedisError : public std::runtime_error {
 public:
  explicit RedisError(const std::string& m) : std::runtime_error(m) {}
};

// utils.TimeSource
class TimeSource {
 public:
  virtual ~TimeSource() = default;
  virtual int64_t UnixNow() = 0;
};
class SystemTimeSource : public TimeSource {
 public:
  int64_t UnixNow() override;
};

// limiter.RateLimitCache  src/limiter/cache.go:15-33
class RateLimitCache {
 public:
  virtual ~RateLimitCache() = default;
  virtual DoLimitResponse DoLimit(const RateLimitRequest& request,
                                  const std::vector<std::shared_ptr<RateLimit>>& limits) = 0;
  virtual void Flush() = 0;
};

// One DoLimit call waiting in a micro-batcher (rl_cache.cpp).
struct PendingCall;

// What Peek / Forget of either cache report per descriptor (rl_hip.h rl_peek_reply).
struct PeekStatus {
  bool Found = false, LocalCached = false;
  uint32_t Count = 0, TtlSeconds = 0, CachedSeconds = 0;
};
// The trace hook's position of a control call (Peek / Forget).
constexpr uint32_t kTraceControl = 0xFFFFFFFFu;

// Test hook of both batchers: every call's place in the serial order as it is put in a batch —
// (the batch's / step's sequence number, the call's request position in it). The serial order
// of one engine is (batch, position); of a routed deployment (step, rank, position). A Peek /
// Forget of HipRateLimitCache is reported as (the next batch to be gathered, kTraceControl): it
// comes after every call of the batches before that one and before every call of it. A Peek /
// Forget of HipRoutedRateLimitCache runs at a rule / stop agreement and is reported as (the next
// step, kTraceControl): after every call of the steps before that agreement on every rank, before
// every call of the steps after it; within one agreement every rank's Peeks (rank order, enqueue
// order) come before every rank's Forgets.
using TraceFn = std::function<void(const RateLimitRequest* request, uint64_t seq, uint32_t pos)>;

// HIP_* settings (BACKEND_TYPE=hip)
struct HipSettings {
  int device = 0;                         // HIP_DEVICES
  uint32_t log2_slots[4] = {20, 20, 20, 18};  // HIP_TABLE_SLOTS per unit
  float near_limit_ratio = 0.8f;          // NEAR_LIMIT_RATIO
  bool local_cache = false;               // LOCAL_CACHE_SIZE_IN_BYTES > 0
  // HIP_LOCAL_CACHE=freecache (single-engine batcher): the local cache is a host-side model of
  // freecache holding LOCAL_CACHE_SIZE_IN_BYTES bytes (rl_freecache.hpp: it evicts, as the
  // reference's does under a small size; parity-unpinned), looked up when a call is enqueued and
  // Set when its batch is decided, instead of the device's cache (which never evicts)
  bool local_cache_freecache = false;
  int64_t local_cache_bytes = 0;
  bool per_second_split = false;          // REDIS_PERSECOND
  uint32_t batch_window_us = 75;          // HIP_BATCH_WINDOW
  uint32_t batch_limit = 1u << 16;        // HIP_BATCH_LIMIT (descriptors)
  uint64_t hash_seed = 0x5ee7ab1e5eedull;  // HIP_HASH_SEED: the same in every process of a deployment
  uint32_t max_load_permille = 750;        // HIP_TABLE_MAX_LOAD: refuse a batch past this region load
  // HIP_TABLE_AUTOGROW (0 = off, the default): once a completed batch leaves either parity region
  // of a home unit with more than slots * autogrow_permille / 1000 live slots, the single-engine
  // batcher doubles that unit's regions (rl_resize), up to 2^max_log2_slots[unit]
  // (HIP_TABLE_MAX_SLOTS). HipRateLimitCache::Resize below.
  uint32_t autogrow_permille = 0;
  uint32_t max_log2_slots[4] = {31, 31, 31, 31};
  // HIP_REFUND_REJECTED (off by default; an extension, rl_hip.h "Refund"): every decision batch is
  // followed by one rl_refund_behind flight, so a request the limiter rejects gives back what its
  // descriptors were charged. The statuses must stay on the device for it, so the batcher then
  // sends every batch in the full format, never the compact one.
  bool refund_rejected = false;
  bool answer_early = true;                // HIP_BATCH_ANSWER_EARLY: while gathering, answer the batch in
                                           // flight as soon as the device is done with it (rl_query)
  // EXPIRATION_JITTER_MAX_SECONDS (settings.go:43, default 300; at most 65536 here): every INCRBY's
  // EXPIRE gets JitterRand.Int63n(max) more seconds (fixed_cache_impl.go:69-72). The batcher draws
  // one value per descriptor with a limit, in enqueue order, from jitter_rand (a seeded Int63n
  // source by default; the reference's NewFixedRateLimitCacheImpl takes its jitterRand too).
  int64_t expiration_jitter_max_seconds = 0;
  std::function<int64_t(int64_t)> jitter_rand;  // Int63n(n): uniform in [0, n)
};

// The HIP backend. Equivalent of redis.NewFixedRateLimitCacheImpl + fixedRateLimitCacheImpl.
class HipRateLimitCache : public RateLimitCache {
 public:
  HipRateLimitCache(const HipSettings& s, std::shared_ptr<TimeSource> time_source);
  ~HipRateLimitCache() override;
  DoLimitResponse DoLimit(const RateLimitRequest& request,
                          const std::vector<std::shared_ptr<RateLimit>>& limits) override;
  // Flush() is a no-op for the Redis backend (fixed_cache_impl.go:125-126); here it
  // waits until every enqueued call has been decided.
  void Flush() override;

  // Snapshot / restore of the counter table (rl_hip.h "Snapshot / restore") to a file: the 256-B
  // rl_snapshot_header, then n_records 32-B records, nothing else. Both go through the batcher's
  // queue as a control call: every DoLimit enqueued before it is decided first, the engine calls
  // run on the submitter thread with nothing in flight (all engine calls stay on one thread), and
  // the batcher resumes with the calls enqueued behind it; DoLimit callers are held meanwhile
  // (Save: for the export pass and the drain to the file). Load may be given a snapshot of a
  // table of another size (HIP_TABLE_SLOTS); it needs the same HIP_HASH_SEED and REDIS_PERSECOND.
  // The rule registry is not part of a snapshot: a record carries no rule, limits come with each
  // request. HIP_LOCAL_CACHE=freecache: that cache lives on the host and is neither saved nor
  // touched by Load (a restarted process starts it empty, as the reference's freecache starts).
  // Both throw RedisError (the engine's message, or the file's); a failed Load leaves the table
  // untouched when the header is refused, else empty.
  void Save(const std::string& path);
  void Load(const std::string& path);

  // Peek / Forget (rl_hip.h "Peek / forget"): what an operator asks Redis with GET / TTL and DEL,
  // per descriptor of a request as DoLimit would key it (limits[i] == nullptr: no lookup, a zero
  // status). Peek spends nothing (no hit, no stat, no jitter draw); Forget clears the descriptor's
  // counter on its store and the string's device local-cache entry, so the next DoLimit counts
  // from 0, and returns what Peek would have returned just before. Both are control calls like
  // Save / Load: every DoLimit enqueued before them is decided first, the engine call runs on
  // the submitter thread with nothing in flight, and the time is ts_->UnixNow() taken there, so
  // their place in the serial order is well defined (the trace hook reports it: the sequence
  // number of the first batch gathered after the call, position kTraceControl). A new
  // (RequestsPerUnit, unit) is registered as DoLimit registers it. Errors throw RedisError.
  // HIP_LOCAL_CACHE=freecache: that cache lives on the host and is neither reported (LocalCached
  // is false) nor cleared; its entries expire after at most one divider.
  // HipRoutedRateLimitCache has its own Peek / Forget (below), which ask each key's owner. Out of
  // scope: a compact wire form.
  using PeekStatus = ratelimit::PeekStatus;
  static constexpr uint32_t kTraceControl = ratelimit::kTraceControl;
  std::vector<PeekStatus> Peek(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits);
  std::vector<PeekStatus> Forget(const RateLimitRequest& request,
                                 const std::vector<std::shared_ptr<RateLimit>>& limits);

  // Set (rl_hip.h "Set"): Redis SET key n EX ttl per descriptor, and the string's device
  // local-cache entry: values[i] is what descriptor i's key string holds afterwards (Found: Count
  // with TtlSeconds, else DEL; LocalCached: CachedSeconds, else no entry), keep_counter /
  // keep_cache leave that part of every descriptor as it is. Returns what Peek would have
  // returned just before. A control call exactly like Forget: its place in the serial order, the
  // time taken on the submitter thread, the trace hook's kTraceControl, registration of new
  // (RequestsPerUnit, unit) pairs. After it the auto-grow check runs as after a completed batch
  // (a Set can claim slots). HIP_LOCAL_CACHE=freecache: the cache part is ignored, as the device
  // cache is unused there. HipRoutedRateLimitCache has no Set yet (rl_hip.h "Set", out of scope).
  std::vector<PeekStatus> Set(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
                              const std::vector<PeekStatus>& values, bool keep_counter = false,
                              bool keep_cache = false);

  // Adjust (rl_hip.h "Adjust"): Redis INCRBY / DECRBY by key outside a decision, per descriptor of
  // a request as DoLimit would key it: deltas[i] (signed: a refund is negative, a true-up either)
  // is added to descriptor i's counter where it exists at the call's time, clamped to
  // [0, 2^32 - 1]; a counter that is absent (its window is over) is left alone and nothing is
  // claimed. A refund that brings the key back to its limit releases it from the device local cache
  // unless keep_cache. Returns what Peek would have returned just before. No hit, no stat, no
  // decision. A control call exactly like Forget: every DoLimit enqueued before it is decided
  // first, the time is taken on the submitter thread, the trace hook reports kTraceControl, new
  // (RequestsPerUnit, unit) pairs are registered as DoLimit registers them. The auto-grow check
  // does not run behind it (nothing is claimed). HIP_LOCAL_CACHE=freecache: the cache part is
  // ignored, as the device cache is unused there (a host entry expires after at most one divider).
  // Errors throw RedisError. HipRoutedRateLimitCache has its own Adjust (below), applied at each
  // key's owner.
  std::vector<PeekStatus> Adjust(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
                                 const std::vector<int32_t>& deltas, bool keep_cache = false);

  // AdjustQueued (rl_hip.h "Adjust in flight"): Adjust without emptying the pipeline. The call goes
  // into the queue like a DoLimit. The submitter's gather takes the queued calls of both kinds:
  // DoLimits form the decision batch, queued adjusts one adjust batch per keep flag, one request per
  // call at the time read on the submitter thread, and each adjust batch goes to the engine as one
  // rl_adjust_submit flight BEHIND the gather's decision batch (the decision batch is built in the
  // staging slot of the next flight, so it has to go first; all calls in the queue at one gather
  // are concurrent, so this is a legal serial order). Nothing is drained. The trace hook reports
  // (the gather's sequence number, kTraceAdjust | kTraceAdjustKeep for keep_cache | the call's
  // index in its group): behind every DoLimit position of that gather, the group without
  // keep_cache first. Different from Adjust: the corrections gathered into one engine call ARE one
  // call: summed per (string, store), clamped once, and every reply is the state before that engine
  // call. A failed flight fails every call in it with RedisError; nothing was applied and the cache
  // keeps serving. HIP_LOCAL_CACHE=freecache forces keep_cache, as in Adjust. No auto-grow check
  // runs behind it. Out of scope: HipRoutedRateLimitCache, the Python mirror, a compact wire form.
  static constexpr uint32_t kTraceAdjust = 0x80000000u, kTraceAdjustKeep = 0x40000000u;
  std::vector<PeekStatus> AdjustQueued(const RateLimitRequest& request,
                                       const std::vector<std::shared_ptr<RateLimit>>& limits,
                                       const std::vector<int32_t>& deltas, bool keep_cache = false);

  // Resize (rl_hip.h "Resize"): the counter table moved into one of log2_slots[u] slots per window
  // generation for home unit u (0 keeps that unit's size), on the device, every counter kept. A
  // control call like Save / Load: every DoLimit enqueued before it is decided first, rl_resize
  // runs on the submitter thread with nothing in flight, DoLimit callers are held for the pass.
  // A refusal throws RedisError and changes nothing (a shrink is checked against the occupancy
  // mirror, which may over-count: a tight one can be refused although it would fit). Peak device
  // memory is the old table plus the new one. Occupancy is rl_get_occupancy at the same point of
  // the serial order.
  // Auto-grow (HipSettings::autogrow_permille > 0): after every completed batch the submitter
  // reads rl_get_occupancy; if either parity region of a home unit holds more than
  // slots * autogrow_permille / 1000 live slots and the unit is below 2^max_log2_slots[unit], it
  // completes the batches in flight (counted in drains) and calls rl_resize with that unit's
  // log2 + 1. With the watermark below HIP_TABLE_MAX_LOAD the table therefore grows before a
  // batch is refused; no batch is retried or reordered. A single batch that takes a region from
  // under the watermark to over its load limit is still refused as without auto-grow (its callers
  // get RedisError), and the growth follows it. A grow that fails (no device memory for the two
  // tables) is counted in resize_failures and not tried again until that unit's occupancy has
  // risen; the old table keeps serving and DoLimit never throws because of it.
  // Out of scope: HipRoutedRateLimitCache (every rank would have to resize between the same two
  // steps; rl_resize itself is legal on a router's engine between steps) and a resize while
  // batches are in flight.
  void Resize(const uint32_t log2_slots[4]);
  rl_occupancy Occupancy();

  // Merge (rl_hip.h "Merge"): a snapshot file's records, from record first_record on, folded into
  // the live counters while the cache serves: counters add, expiries and local-cache deadlines
  // take the later one, absent strings are claimed. The file is read on the caller's thread and
  // every chunk (at most min(2^16, batch_limit) records) is ONE control call of its own, so the
  // DoLimit calls enqueued meanwhile are decided between two chunks, not behind the whole file:
  // callers are held for one chunk's rl_merge at a time. Each chunk's time is ts_->UnixNow()
  // taken on the submitter thread, each is reported to the trace hook as (the next batch to be
  // gathered, kTraceControl) with a null request, and after each the auto-grow check runs as after
  // a Set (a chunk can claim slots). A chunk the engine refuses throws RedisError naming how many
  // records of the file are merged (those stay merged; the refused chunk changed nothing), so
  // after a Resize the caller resumes with first_record = that number; MergeError carries it.
  // A malformed file throws before anything is merged. The same chunk merged twice adds twice.
  // HIP_LOCAL_CACHE=freecache: the host cache is neither read nor written. Needs the writer's
  // HIP_HASH_SEED and REDIS_PERSECOND; the table sizes may differ. HipRoutedRateLimitCache has no
  // Merge (records carry no owner): consolidate into one engine, or let a rank take back its own.
  struct MergeReport {
    uint64_t Records = 0, Folded = 0, Claimed = 0, DroppedOver = 0, DroppedEmpty = 0;
  };
  struct MergeError : RedisError {
    MergeError(const std::string& msg, uint64_t merged) : RedisError(msg), Merged(merged) {}
    uint64_t Merged;  // records of the file merged before the refusal (first_record included)
  };
  MergeReport Merge(const std::string& path, uint64_t first_record = 0);

  // Batcher counters (tests): batches submitted, rule-table loads, and loads made while an
  // earlier batch was still in flight (append-only rule table, rl_hip.h rl_load_rules).
  // drains: times the batches in flight were completed early so that a rule-table load or a
  // submit the engine refused with them in flight (RL_ESTATE) could be made.
  // compact_batches: batches sent in the compact wire format (rl_submit_c); the others went as
  // rl_batch (a rule id past 0xFFFE, a prefix past 65535 bytes or hits_addend past 2^24 - 1).
  // resizes / resize_failures: auto-grow's rl_resize calls that succeeded / failed.
  struct BatcherStats {
    uint64_t batches, rule_loads, rule_loads_in_flight, drains, compact_batches, resizes, resize_failures;
  };
  BatcherStats batcher_stats() const {
    return {n_batches_.load(), n_loads_.load(),   n_loads_inflight_.load(), n_drains_.load(),
            n_compact_.load(), n_resizes_.load(), n_resize_fail_.load()};
  }
  // HIP_REFUND_REJECTED: refund flights made, and those the engine refused or that failed (such a
  // batch stays charged as the reference charges it).
  uint64_t refund_flights() const { return n_refunds_.load(); }
  uint64_t refund_failures() const { return n_refund_fail_.load(); }
  // (tests) set before the first DoLimit
  void set_trace(TraceFn f) { trace_ = std::move(f); }
  // The ratelimit.localcache.* gauges: hits, misses, lookups, entries, evicted,
  // expired. HIP_LOCAL_CACHE=freecache: the host model's. The device cache: hits / lookups counted
  // from every answered batch's statuses, entries / expired from an rl_census at the time source's
  // now (a control call: every DoLimit enqueued before it is decided first), evicted 0. Zeros with
  // the local cache off.
  void local_cache_stats(uint64_t* out);

 private:
  struct Staged;
  struct AdjGather;
  bool fits_adjust(const AdjGather& g, const PendingCall& c) const;
  void add_adjust(AdjGather& g, const std::shared_ptr<PendingCall>& c, uint64_t seq);
  Staged submit_adjust(AdjGather& g, bool keep, uint64_t seq, std::deque<Staged>& inflight);
  std::vector<rl_peek_reply> adj_rep_;  // a completed adjust flight's replies (submitter thread)
  void submitter();
  void control(std::function<std::string()> f);
  std::vector<PeekStatus> peek_call(const RateLimitRequest& request,
                                    const std::vector<std::shared_ptr<RateLimit>>& limits, bool forget,
                                    const std::vector<PeekStatus>* values = nullptr, uint32_t keep = 0,
                                    const std::vector<int32_t>* deltas = nullptr);
  bool grow_after_ctl_ = false;  // set by a Set's control call, read by the submitter behind it
  uint32_t rule_id(const RateLimitLimit& l, bool shadow);
  bool fits(const Staged& st, const PendingCall& c) const;
  bool compactable(const PendingCall& c) const;
  void add(Staged& st, const std::shared_ptr<PendingCall>& c);
  void submit(Staged& st, std::deque<Staged>& inflight);
  void finish(Staged& st);
  void finish_oldest(std::deque<Staged>& inflight);
  void autogrow(std::deque<Staged>& inflight);
  void fail(std::vector<std::shared_ptr<PendingCall>>& calls);
  void done_calls(size_t n);

  HipSettings s_;
  std::shared_ptr<TimeSource> ts_;
  rl_engine* eng_ = nullptr;
  std::mutex mu_;
  std::condition_variable cv_, idle_cv_;
  std::deque<std::shared_ptr<PendingCall>> q_;
  size_t inflight_ = 0;  // calls enqueued and not yet answered
  bool stop_ = false;
  std::thread thr_;
  // rule registry (submitter thread only): append-only, so ids keep their meaning while
  // batches that use them are in flight
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> rule_ids_;
  std::vector<rl_rule> rules_;
  bool rules_dirty_ = false;
  std::atomic<uint64_t> n_batches_{0}, n_loads_{0}, n_loads_inflight_{0}, n_drains_{0}, n_compact_{0};
  std::atomic<uint64_t> n_refunds_{0}, n_refund_fail_{0};  // HIP_REFUND_REJECTED: flights made; refused or failed
  std::atomic<uint64_t> n_resizes_{0}, n_resize_fail_{0};
  std::atomic<uint64_t> lc_lookups_{0}, lc_hits_{0};  // the device cache's Gets and hits (finish())
  uint32_t grow_failed_at_[4] = {0, 0, 0, 0};  // live slots of the unit when its last grow failed (0 = none)
  // statuses of a compact batch made on the host from its raw replies (rl_decide_raw)
  std::vector<rl_status> dec_out_;
  std::vector<uint32_t> dec_thr_;
  TraceFn trace_;
  bool jitter_ = false;
  uint64_t staged_seq_ = 0;  // batches gathered (= submitted, in order)
  std::unique_ptr<FreeCacheModel> fc_;  // HIP_LOCAL_CACHE=freecache
  std::mutex fc_mu_;                    // (freecache's segment locks)
};

// ---- Multi-GPU deployment ------------------------------------------------
// One HipRoutedRateLimitCache per GPU: one process per GPU over RCCL (rl_router_unique_id made by
// rank 0 and handed to the others out of band), or one thread per rank of this process over the
// emulated collectives (rl_router_emu_world; tests). Each rank's DoLimit callers enqueue on its
// own batcher; every rank steps on a fixed cadence (step_us) — gathering what its callers queued
// during the step into the router's pinned slot, or an EMPTY batch when its queue is idle — so the
// ranks' collectives always pair up (rl_hip.h: every rank makes the same sequence of router
// calls). Two steps are in flight. Rule ids must mean one limit on every owner: a new (L, unit)
// is agreed at the next rule-sync step (every rule_sync_every steps, with nothing in flight, by
// rl_router_allgather_host: every rank appends every rank's new rules in rank order), and a call
// that needs it waits for that step. A stop is agreed the same way: a rank leaves only when every
// rank asked to stop with nothing queued. Serial order: each step, rank 0's batch, rank 1's, ...
// The reference's equivalent is the radix cluster client sending each key's commands to the node
// that owns it, pipelined (src/redis/driver_impl.go:84-110); DoLimit stays synchronous for its
// caller (src/limiter/cache.go:15-33).
struct HipRoutedSettings {
  uint32_t n_shards = 1;
  uint32_t rank = 0;
  std::vector<uint8_t> id;        // RL_ROUTER_ID_BYTES: rl_router_unique_id, or rl_router_emu_world
  bool emulated = false;          // id is an emulated world (one thread per rank in this process)
  uint32_t step_us = 200;         // step cadence (HIP_STEP_US)
  uint32_t rule_sync_every = 16;  // steps between rule / stop agreements
};

class HipRoutedRateLimitCache : public RateLimitCache {
 public:
  // Collective: every rank constructs at the same time (rl_router_create agrees configurations).
  HipRoutedRateLimitCache(const HipSettings& s, const HipRoutedSettings& r, std::shared_ptr<TimeSource> time_source);
  // Collective too: returns once every rank has asked to stop and nothing is queued anywhere.
  ~HipRoutedRateLimitCache() override;
  DoLimitResponse DoLimit(const RateLimitRequest& request,
                          const std::vector<std::shared_ptr<RateLimit>>& limits) override;
  void Flush() override;

  // Peek / Forget (rl_hip.h "Routed peek / forget"): HipRateLimitCache's calls, same signatures
  // and PeekStatus, answered by the owner of each key through rl_router_peek / rl_router_forget.
  // They are control calls agreed at the rule / stop agreement: every rank's agreement words carry
  // its numbers of pending Peeks and Forgets; with nothing in flight on any rank, if any rank has
  // pending Peeks every rank calls rl_router_peek once — its own pending calls as one request
  // each, in enqueue order, at the time ts_->UnixNow() gives the submitter thread there; a rank
  // with none passes an empty batch — and then, if any rank has pending Forgets, every rank calls
  // rl_router_forget once the same way. Place in the serial order: after every call of the steps
  // before that agreement and before every call of the steps after it; within one agreement all
  // Peeks come before all Forgets (the trace hook reports (the next step's sequence number,
  // kTraceControl)). A call whose limit has no agreed id yet queues the limit as DoLimit does and
  // waits for the following agreement, as do calls beyond one router batch (batch_limit
  // descriptors). Worst-case latency is therefore rule_sync_every x step_us (twice that for a new
  // limit). Errors throw RedisError; a communicator failure marks the cache broken, as a step's.
  using PeekStatus = ratelimit::PeekStatus;
  static constexpr uint32_t kTraceControl = ratelimit::kTraceControl;
  std::vector<PeekStatus> Peek(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits);
  std::vector<PeekStatus> Forget(const RateLimitRequest& request,
                                 const std::vector<std::shared_ptr<RateLimit>>& limits);
  // Set (rl_hip.h "Routed set"): HipRateLimitCache::Set's signature and PeekStatus, written at the
  // owner of each key through rl_router_set, all owners or none. A third control kind beside Peek
  // and Forget: agreed at the rule / stop agreement (every rank's words carry its number of pending
  // Sets), run after the agreement's Peeks and Forgets, every rank's pending Sets as one
  // rl_router_set (a rank with none passes an empty batch), reported to the trace hook as (the next
  // step's sequence number, kTraceControl). Returns what Peek would have returned just before.
  std::vector<PeekStatus> Set(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
                              const std::vector<PeekStatus>& values, bool keep_counter = false,
                              bool keep_cache = false);

  // Adjust (rl_hip.h "Routed adjust"): HipRateLimitCache::Adjust's signature and PeekStatus, each
  // correction applied at the owner of its key through rl_router_adjust, all owners or none; the
  // corrections of one key from every rank of one agreement are summed and applied once. A further
  // control kind beside Peek, Forget and Set: agreed at the rule / stop agreement and run after the
  // agreement's Sets. rl_router_adjust's flags word is per origin, so every rank's agreement words
  // carry two counts, its pending Adjusts without keep_cache and those with it, and they run as at
  // most two router calls in that order: every rank's pending calls of the kind as one
  // rl_router_adjust, one request each in enqueue order (a rank with none passes an empty batch).
  // Reported to the trace hook as (the next step's sequence number, kTraceControl). Returns what
  // Peek would have returned just before. A new limit waits one agreement, as for Set.
  std::vector<PeekStatus> Adjust(const RateLimitRequest& request, const std::vector<std::shared_ptr<RateLimit>>& limits,
                                 const std::vector<int32_t>& deltas, bool keep_cache = false);

  // HIP_REFUND_REJECTED (off by default; rl_hip.h "Routed refund"): when a step completes, every
  // request of it that the limiter rejected is queued as a control call of the batcher's own, with
  // nobody waiting on it: the request's prefixes, rule ids, time, HitsAddend and statuses. Two
  // further control kinds carry them, without and with the keep bit (set when the host freecache
  // model is on, as in the single-engine batcher), counted in every rank's agreement words like the
  // other kinds. At the agreement they run first, before the callers' Peeks, Forgets, Sets and
  // Adjusts: every rank's pending ones as one rl_router_refund, as far as one router batch holds
  // them (the rest waits for the following agreement; a rank with none passes an empty batch). So a
  // refund is applied at the agreement after its step, not behind the step itself as on the
  // single-engine batcher: until then the counters hold the rejected request's charge, at most
  // rule_sync_every x step_us. The trace hook reports each as (the next step's sequence number,
  // kTraceControl) with a null request. A stop is agreed only when none is pending. With the
  // option off nothing changes.
  // refund_flights(): rl_router_refund calls that carried refunds of this rank; refund_failures():
  // those that were refused or failed (their refunds are dropped: the counters stay charged).
  uint64_t refund_flights() const { return n_refunds_.load(); }
  uint64_t refund_failures() const { return n_refund_fail_.load(); }

  struct RoutedStats {
    uint64_t steps, empty_steps, rule_syncs, rules, held_calls;
  };
  RoutedStats routed_stats() const {
    return {n_steps_.load(), n_empty_.load(), n_syncs_.load(), n_rules_.load(), n_held_.load()};
  }
  // (tests) set before the first DoLimit
  void set_trace(TraceFn f) { trace_ = std::move(f); }

 private:
  struct Step;
  void submitter();
  bool known(const PendingCall& c);
  bool sync(bool want_stop, std::deque<std::shared_ptr<PendingCall>>& ctl, uint64_t seq);
  void run_control(int kind, std::deque<std::shared_ptr<PendingCall>>& ctl, uint64_t seq);
  std::vector<PeekStatus> peek_call(const RateLimitRequest& request,
                                    const std::vector<std::shared_ptr<RateLimit>>& limits, int kind,
                                    const std::vector<PeekStatus>* values = nullptr, uint32_t keep = 0,
                                    const std::vector<int32_t>* deltas = nullptr);
  void fail(std::vector<std::shared_ptr<PendingCall>>& calls, const std::string& msg);
  void done_calls(size_t n);

  HipSettings s_;
  HipRoutedSettings r_;
  std::shared_ptr<TimeSource> ts_;
  rl_engine* eng_ = nullptr;
  rl_router* rt_ = nullptr;
  std::mutex mu_;
  std::condition_variable cv_, idle_cv_;
  std::deque<std::shared_ptr<PendingCall>> q_;
  size_t inflight_ = 0;
  bool stop_ = false;
  bool broken_ = false;  // the router's communicator is gone: every call fails
  std::string broken_msg_;
  std::thread thr_;
  // agreed rule registry (submitter thread): identical on every rank after each sync
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> ids_;
  std::vector<rl_rule> rules_;
  std::vector<rl_rule> pending_;  // new limits seen here, not agreed yet
  std::set<std::pair<uint32_t, uint32_t>> pending_set_;
  std::atomic<uint64_t> n_steps_{0}, n_empty_{0}, n_syncs_{0}, n_rules_{0}, n_held_{0};
  std::atomic<uint64_t> n_refunds_{0}, n_refund_fail_{0};  // HIP_REFUND_REJECTED: router calls made; refused or failed
  TraceFn trace_;
  bool jitter_ = false;
};

}  // namespace ratelimit
