/*
 * rl_hip.h — C ABI of the MI355X-native fixed-window rate-limit backend.
 *
 * This is the drop-in boundary for the reference's hot path. It replaces
 *   limiter.RateLimitCache.DoLimit / Flush         src/limiter/cache.go:15-33
 * as implemented by the Redis backend
 *   fixedRateLimitCacheImpl.DoLimit                src/redis/fixed_cache_impl.go:31-123
 *   redis.Client.PipeAppend / PipeDo (INCRBY+EXPIRE pipeline)
 *                                                  src/redis/driver.go:13-47, fixed_cache_impl.go:26-29
 * A Go `src/hip` package binds these entry points over cgo; the C++
 * mirror of the Go interface lives in api-ratelimit_amd/csrc/rl_cache.hpp.
 *
 * Plain C types only; no exceptions cross the ABI. Every call returns 0 on success or a
 * negative RL_E* code; rl_last_error() then holds a message (the Go side turns a
 * non-zero return into panic(redis.RedisError(msg)), src/redis/driver.go:6-10, so the
 * service maps it to the redis_error stat exactly as for Redis, service/ratelimit.go:276-281).
 * All calls on one engine must come from one thread (the batch submitter).
 */
#ifndef RL_HIP_H
#define RL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RL_ABI_VERSION 7u

/* rule id of a descriptor whose limit is nil ("don't check", src/limiter/cache.go:19-22) */
#define RL_NIL_RULE 0xFFFFFFFFu

/* pb.RateLimitResponse_RateLimit_Unit (go-control-plane v0.9.7) */
enum { RL_UNIT_UNKNOWN = 0, RL_UNIT_SECOND = 1, RL_UNIT_MINUTE = 2, RL_UNIT_HOUR = 3, RL_UNIT_DAY = 4 };
/* pb.RateLimitResponse_Code */
enum { RL_CODE_UNKNOWN = 0, RL_CODE_OK = 1, RL_CODE_OVER_LIMIT = 2 };
/* rl_status.code_flags bits 8.. */
enum {
  RL_FLAG_HAS_LIMIT = 1u,       /* DescriptorStatus.CurrentLimit != nil and DurationUntilReset set */
  RL_FLAG_LOCAL_CACHE_HIT = 2u, /* over limit via the local cache: add over_limit_delta to
                                   OverLimitWithLocalCache too (base_limiter.go:76-81) */
  RL_FLAG_SHADOW = 4u           /* extension (rule with RL_RULE_SHADOW): the descriptor was over its limit
                                   and is reported OK; add 1 to Stats.ShadowMode. Counters, local cache,
                                   limit_remaining and the over/near deltas are those of the OVER_LIMIT decision */
};

/* error codes */
enum {
  RL_OK = 0,
  RL_EINVAL = -1,    /* bad argument / malformed batch */
  RL_EHIP = -2,      /* HIP runtime error */
  RL_ENOSPC = -3,    /* a counter-table region would pass its load limit: the batch was refused before
                        any counter changed (raise log2_slots / max_load_permille) */
  RL_ECAPACITY = -4, /* batch larger than the engine was created for */
  RL_ESTATE = -5,    /* call out of order (e.g. rl_wait without rl_submit) */
  RL_EDEVICE = -6,   /* device-side fault detected (bounded spin expired) */
  RL_EPEER = -7,     /* rl_router_step: another shard failed this step (its code in rl_router_stats) */
  RL_ECOMM = -8,     /* rl_router: RCCL error */
  RL_ELATE = -9      /* rl_router: this shard's origin batch starts more than 3 s behind the step clock; none of
                        its descriptors was applied (the other shards' steps went ahead: a clock-skew signal,
                        counted in rl_router_stats.late_steps) */
};

typedef struct rl_engine rl_engine;

/* Engine configuration (REDIS_* settings analogues, src/settings/settings.go:10-48). */
typedef struct rl_config {
  uint32_t struct_size;        /* = sizeof(rl_config) */
  int32_t device;              /* HIP device ordinal (HIP_DEVICES) */
  uint32_t log2_slots[4];      /* table slots per window generation of the key strings whose home unit is
                                  SECOND/MINUTE/HOUR/DAY (HIP_TABLE_SLOTS) */
  float near_limit_ratio;      /* NEAR_LIMIT_RATIO, default 0.8 (settings.go:44) */
  uint32_t local_cache;        /* 1 = local over-limit cache on (LOCAL_CACHE_SIZE_IN_BYTES > 0, settings.go:45) */
  uint32_t per_second_split;   /* REDIS_PERSECOND (settings.go:35): SECOND keys count in their own store; else
                                  one store holds every unit and same-string keys share a counter */
  uint32_t max_batch_desc;     /* capacity: descriptors per batch (HIP_BATCH_LIMIT) */
  uint32_t max_batch_req;      /* capacity: requests per batch */
  uint32_t max_blob_bytes;     /* capacity: key-prefix bytes per batch */
  uint32_t sort_bits;          /* LSD pipeline: fingerprint bits radix-sorted per batch (8..64, multiple of 8; 0 = 48) */
  uint32_t flags;              /* RL_CFG_* */
  uint64_t hash_seed;          /* fingerprint seed: one value for every engine of a deployment (multi-GPU
                                  owners must agree), secret against hash flooding */
  uint32_t max_load_permille;  /* load limit per table region, 100..950 (0 = 750): a batch that could push a
                                  region past it is refused with RL_ENOSPC before anything changes */
  uint32_t reserved;           /* 0 */
} rl_config;

/* rl_config.flags */
enum {
  RL_CFG_LSD_ONLY = 1u,  /* always use the LSD radix-sort pipeline (default: v4 pipeline, LSD as fallback) */
  RL_CFG_LAG_WINDOW = 2u,/* keep a SECOND key string findable for requests up to 3 s behind the newest time the
                            table has seen, at up to twice the SECOND regions' live slots against the same load
                            limit. rl_router_create turns it on for its engines (origins' clocks differ); a lone
                            engine fed in enqueue order does not need it */
  RL_CFG_RULE_STATS = 4u,/* add every completed batch's stat increments to the per-rule counters on the device
                            ("Rule stats" below) */
  RL_CFG_CACHE_STATS = 8u /* add every completed batch's local-cache lookups and hits to the lookup counters on
                            the device ("Local-cache gauges" below); nothing is counted or launched with
                            local_cache == 0 */
};

/* One rate-limit rule: config.RateLimit.Limit (src/config/config.go:26-32). */
typedef struct rl_rule {
  uint32_t requests_per_unit;
  uint32_t unit; /* RL_UNIT_SECOND..RL_UNIT_DAY, optionally | RL_RULE_SHADOW; anything else is RL_EINVAL
                    (utilities.go:31 panics) */
} rl_rule;
/* Shadow mode (BASELINE config 4; an extension: this fork has none, config_impl.go:49-59 rejects a
 * shadow_mode key). A rule whose unit carries this bit never answers OVER_LIMIT: such a decision
 * is reported as RL_CODE_OK with RL_FLAG_SHADOW, everything else unchanged (envoyproxy/ratelimit's
 * later `shadow_mode`: counters still increment, the local cache still freezes the key, over/near
 * stats still count). Parity unpinned by a reference fixture. */
#define RL_RULE_SHADOW 0x100u

/* A batch of requests in serial (enqueue) order. Descriptor i belongs to request req_of[i]
 * (non-decreasing). Its cache-key prefix is the exact byte string
 *   domain '_' key1 '_' value1 '_' ... keyN '_' valueN '_'
 * of GenerateCacheKey (src/limiter/cache_key.go:57-65) without the window timestamp, which
 * the device appends (cache_key.go:66-68): bytes prefix_blob[prefix_off[i] .. prefix_off[i+1]).
 * The same struct carries host pointers (rl_submit) or device pointers (rl_submit_device).
 * A device prefix_blob must be readable (not meaningful) for RL_BLOB_SLACK bytes past
 * blob_bytes, non-null even when every prefix is empty: the device reads prefixes in 16-B
 * words. Host batches need no slack (rl_submit stages them with it). A batch with
 * descriptors has at least one request. */
#define RL_BLOB_SLACK 32
typedef struct rl_batch {
  uint32_t n_desc;
  uint32_t n_req;
  uint32_t blob_bytes;
  uint32_t reserved;
  const uint8_t* prefix_blob;
  const uint32_t* prefix_off;  /* n_desc + 1 entries */
  const uint32_t* rule_id;     /* n_desc, RL_NIL_RULE for a nil limit */
  const uint32_t* req_of;      /* n_desc */
  const int64_t* now;          /* n_req: unix seconds, one per request (TimeSource.UnixNow) */
  const uint32_t* hits_addend; /* n_req: RateLimitRequest.HitsAddend (0 means 1, fixed_cache_impl.go:39) */
  const uint16_t* ttl_jitter;  /* n_desc or NULL (= all 0): seconds added to the EXPIRE of the descriptor's
                                  INCRBY, JitterRand.Int63n(EXPIRATION_JITTER_MAX_SECONDS) drawn by the host in
                                  serial order (fixed_cache_impl.go:69-72); the key lives until its last INCRBY's
                                  now + divider + jitter. Ignored for nil limits and local-cache hits.
                                  Draw order: the reference draws no jitter for a local-cache hit
                                  (fixed_cache_impl.go:60-72); the device cache's hits are known only
                                  after the batch, so a host drawing one per descriptor with a limit
                                  matches the reference's sequence of draws only with the local cache
                                  off or with HIP_LOCAL_CACHE=freecache (its hits are found on the
                                  host, before the draws). Each INCRBY's jitter is still one
                                  independent draw (tests/test_jitter.py pins the current behaviour) */
} rl_batch;

/* One DescriptorStatus plus its stat increments (20 B). */
typedef struct rl_status {
  uint32_t code_flags;       /* RL_CODE_* | RL_FLAG_* << 8 */
  uint32_t limit_remaining;  /* DescriptorStatus.LimitRemaining */
  uint32_t reset_s;          /* DescriptorStatus.DurationUntilReset.Seconds (0 if no limit) */
  uint32_t over_limit_delta; /* add to Stats.OverLimit (and OverLimitWithLocalCache if LOCAL_CACHE_HIT) */
  uint32_t near_limit_delta; /* add to Stats.NearLimit */
} rl_status;
/* Stats.TotalHits is incremented by max(1, HitsAddend) for every non-nil limit on the host
 * (base_limiter.go:49-51); it needs no device round trip. */

typedef struct rl_engine_stats {
  uint64_t batches;           /* batches completed */
  uint64_t descriptors;       /* descriptors decided */
  uint64_t resorts;           /* batches re-sorted on the full fingerprint after a sort-prefix collision */
  uint64_t inserted_keys;     /* table slots claimed since creation (one per key string and window) */
  uint64_t lsd_fallbacks;     /* batches the bucketed pipeline handed to the LSD pipeline */
  uint64_t hot_keys;          /* size of the hot-key set used by the last batch */
  uint64_t live_keys;         /* slots of the current window generations, all regions (after the last batch) */
  uint64_t host_batches;      /* batches submitted from host memory (rl_submit) */
} rl_engine_stats;

/* Occupancy of the 8 table regions (home unit x window parity) after the last completed batch. */
typedef struct rl_occupancy {
  uint32_t gen[8];    /* window generation the count belongs to (home window index + 1; 0 = unused) */
  uint32_t live[8];   /* slots claimed for that generation */
  uint32_t limit[8];  /* load limit (slots) */
  uint32_t slots[8];  /* region size */
} rl_occupancy;

int rl_create(const rl_config* cfg, rl_engine** out);
void rl_destroy(rl_engine* e);
/* The engine's last error message; with e == NULL, the calling thread's last rl_create
 * failure (which HIP call failed and why). */
const char* rl_last_error(const rl_engine* e);
uint32_t rl_abi_version(void);

/* Load the rule table; rule ids index it. While batches are in flight the new table must keep
 * every loaded rule at its id and may only append (RL_ESTATE otherwise): in-flight batches read
 * rules by id, and the appended entries are written to slots none of them reads. A micro-batcher
 * whose rule registry only grows (new (L, unit) pairs from a config reload or a descriptor.Limit
 * override, src/config/config_impl.go:281-289) can therefore load at any time. Replacing or
 * dropping rules needs nothing in flight. */
int rl_load_rules(rl_engine* e, const rl_rule* rules, uint32_t n);

/* Batches that may be in flight at once (rl_submit, rl_submit_pipelined). */
#define RL_MAX_IN_FLIGHT 3

/* ---- Host-memory batches (the Go micro-batcher's path) ---------------------------------
 * Up to RL_MAX_IN_FLIGHT host batches are in flight: each has its own pinned staging slot,
 * its H2D copies run on a copy stream while the previous batch's kernels run, and its D2H
 * copies on another while the next batch's run.
 *
 * rl_host_acquire returns the next free staging slot: pinned host arrays (C memory, so a cgo
 * caller fills them through unsafe slices without passing Go pointers) with their
 * capacities. rl_submit takes a batch whose arrays are that slot's (no copy) or any host
 * memory (copied into the slot before rl_submit returns: the caller's arrays are free again).
 * out[n_desc] / req_throttle_ms[n_req] (DoLimitResponse.ThrottleMillis, base_limiter.go:163-165)
 * may be NULL: the results then stay in the engine until rl_wait_into copies them out
 * (the cgo-safe form: Go memory is only touched during that call); non-NULL C memory is
 * filled by rl_wait and must stay valid until then. Completion is in submission order. */
typedef struct rl_host_batch {
  uint8_t* prefix_blob;
  uint32_t* prefix_off;
  uint32_t* rule_id;
  uint32_t* req_of;
  int64_t* now;
  uint32_t* hits_addend;
  uint16_t* ttl_jitter;  /* the slot's jitter array: pass it as rl_batch.ttl_jitter to use it */
  uint32_t max_desc, max_req, max_blob, reserved;
} rl_host_batch;
int rl_host_acquire(rl_engine* e, rl_host_batch* out);
int rl_submit(rl_engine* e, const rl_batch* batch, rl_status* out, uint32_t* req_throttle_ms);
/* Complete the oldest batch in flight (any submit form). */
int rl_wait(rl_engine* e);
/* Non-blocking: 1 if the oldest batch in flight is done on the device (rl_wait would not block on
 * it, barring a rerun the device asked for), 0 if not yet, RL_ESTATE with nothing in flight. A
 * batcher gathering its next batch polls it to answer the callers of the batch in flight as soon
 * as they can be answered (no counterpart in the reference: radix's pipelining answers each
 * command as its reply arrives, src/redis/driver_impl.go:84-89). */
int rl_query(rl_engine* e);
/* Complete the oldest batch in flight, copying its results into out[n_desc] and
 * req_throttle_ms[n_req] (a host batch's, or NULL to discard). */
int rl_wait_into(rl_engine* e, rl_status* out, uint32_t* req_throttle_ms);
/* Complete the oldest batch in flight, a host batch (rl_submit) whose outputs were NULL, and
 * hand out its results where they landed: its staging slot's pinned arrays (C memory; a cgo
 * caller reads them through unsafe slices, no copy). *out holds n_desc statuses and
 * *req_throttle_ms n_req words. They stay valid until the slot is reused: until the batch
 * submitted RL_MAX_IN_FLIGHT places after this one is submitted (a caller that keeps two
 * batches in flight and collects one after each submit may read them until its next submit
 * after this call returns). A device batch, or a host batch submitted with output pointers,
 * gives RL_ESTATE (nothing completed).
 * Replaces the copy of rl_wait_into for a batcher that answers its callers straight from the
 * slot (DoLimit's []*DescriptorStatus, src/redis/fixed_cache_impl.go:108-123). */
int rl_wait_view(rl_engine* e, const rl_status** out, const uint32_t** req_throttle_ms);

/* ---- Compact host batches (the PCIe wire format of a Go batcher) ------------------------
 * The same batch as rl_batch in fewer bytes: per descriptor the prefix bytes plus ONE word
 *   desc_word[i] = prefix_len (bits 0-15) | rule_id (bits 16-31; RL_NIL_RULE16 = nil limit)
 * (prefixes lie back to back in prefix_blob, so their offsets are implicit), per request ONE word
 *   req_word[r]  = hits_addend (bits 0-23; 0 means 1) | (now - now_base) (bits 24-31)
 * and the request index of each descriptor only when requests hold several descriptors
 * (req_of; NULL with RL_BC_ONE_PER_REQ: descriptor i belongs to request i). At one descriptor
 * per request that is len(prefix) + 8 bytes per descriptor against len(prefix) + 24 for
 * rl_batch. A batch whose rule ids reach 0xFFFF, whose prefixes pass 65535 bytes, whose
 * hits_addend pass 2^24 - 1 or whose request times span more than 255 s goes through rl_submit.
 * The device expands the words into the rl_batch arrays (a kernel on the copy stream) and runs
 * the pipeline unchanged.
 * Results come back as raw replies, 8 B per descriptor: the INCRBY post-value each descriptor
 * saw, or its local-cache hit, or nil — what Redis answers the reference's DoLimit
 * (fixed_cache_impl.go:91-102) plus the local-cache verdict (base_limiter.go:57-66). The status
 * is then made on the host by the unchanged BaseRateLimiter logic (GetResponseDescriptorStatus,
 * base_limiter.go:70-195): rl_decide_raw in C, or the Go service's own BaseRateLimiter. */
#define RL_NIL_RULE16 0xFFFFu
#define RL_RAW_NIL 2u /* rl_raw_reply.flags: a nil-limit descriptor (no INCRBY) */
enum { RL_BC_ONE_PER_REQ = 1u /* req_of is implicit: descriptor i belongs to request i (n_desc == n_req) */ };
typedef struct rl_batch_c {
  uint32_t n_desc;
  uint32_t n_req;
  uint32_t blob_bytes;          /* = sum of the prefix lengths */
  uint32_t flags;               /* RL_BC_* */
  int64_t now_base;             /* request r's time = now_base + (req_word[r] >> 24) */
  const uint8_t* prefix_blob;
  const uint32_t* desc_word;    /* n_desc */
  const uint32_t* req_word;     /* n_req */
  const uint32_t* req_of;       /* n_desc, or NULL with RL_BC_ONE_PER_REQ */
  const uint16_t* ttl_jitter;   /* n_desc or NULL: rl_batch.ttl_jitter */
} rl_batch_c;
typedef struct rl_host_batch_c {
  uint8_t* prefix_blob;
  uint32_t* desc_word;
  uint32_t* req_word;
  uint32_t* req_of;
  uint16_t* ttl_jitter;
  uint32_t max_desc, max_req, max_blob, reserved;
} rl_host_batch_c;
/* The next free staging slot, compact layout (the rl_host_acquire contract). */
int rl_host_acquire_c(rl_engine* e, rl_host_batch_c* out);
/* Submit a compact host batch (arrays in the acquired slot, or any host memory: copied before
 * the call returns). Complete it with rl_wait_raw_view / rl_wait_raw_into. */
int rl_submit_c(rl_engine* e, const rl_batch_c* batch);
typedef struct rl_raw_reply rl_raw_reply;
/* Complete the oldest batch in flight, a compact host batch, and hand out its n_desc raw replies
 * in the slot's pinned memory (valid as rl_wait_view's results are). */
int rl_wait_raw_view(rl_engine* e, const rl_raw_reply** out);
/* The same, copying the replies into out[n_desc] (NULL discards). */
int rl_wait_raw_into(rl_engine* e, rl_raw_reply* out);
/* Host side of the compact form: GetResponseDescriptorStatus + the near/over checks + the
 * ThrottleMillis max (base_limiter.go:70-195) for descriptors [d0, d1) of a compact batch from
 * its raw replies (indexed like the batch), with the engine's loaded rules. out / req_throttle_ms
 * are indexed by descriptor / request; a request's ThrottleMillis is written once every one of
 * its descriptors is in [d0, d1) (so a caller may split the range over threads at request
 * boundaries). Bit-exact with the statuses rl_submit returns. Thread-safe against itself; not
 * against rl_load_rules. */
int rl_decide_raw(rl_engine* e, const rl_batch_c* batch, const rl_raw_reply* raw, uint32_t d0, uint32_t d1,
                  rl_status* out, uint32_t* req_throttle_ms);

/* Device-memory batch (inputs already resident in HBM; outputs stay in HBM), with nothing
 * else in flight. Ordered on the engine's stream; rl_wait() completes it. Used by the
 * multi-GPU router and by the benchmark. */
int rl_submit_device(rl_engine* e, const rl_batch* device_batch, rl_status* d_out, uint32_t* d_req_throttle_ms);

/* Device-memory batch whose inputs are complete when the call is made, submitted behind at
 * most RL_MAX_IN_FLIGHT - 1 batches still in flight (the micro-batcher's multi-buffering:
 * batch k+1, k+2 are handed over before rl_wait returns batch k). The engine fingerprints and
 * tile-sorts batch k+2 on a second stream as soon as batch k is done on the GPU, while batch
 * k+1 is decided, and decides batches strictly in submission order, so the results equal
 * serial rl_submit_device/rl_wait rounds. rl_wait completes the oldest batch. Batches in
 * flight together need distinct d_out / d_req_throttle_ms buffers. More than one batch in
 * flight needs the default (v4) pipeline; otherwise RL_ESTATE. Replaces nothing in the
 * reference: it is how the batcher overlaps the radix-style implicit pipelining of
 * src/redis/driver_impl.go:84-89 across batches. */
int rl_submit_pipelined(rl_engine* e, const rl_batch* device_batch, rl_status* d_out, uint32_t* d_req_throttle_ms);

/* The engine's HIP stream (hipStream_t), for ordering external work against it. */
void* rl_stream(rl_engine* e);

/* Run the engine's work on an external stream (e.g. the stream RCCL collectives run on), so
 * that device-side ordering needs no host synchronisation; NULL restores the engine's own
 * stream. The stream must outlive its use. Not while a batch is in flight. */
int rl_set_stream(rl_engine* e, void* hip_stream);

/* ---- Multi-GPU router -------------------------------------------------
 * One engine per GPU; GPU s owns the keys whose prefix fingerprint maps to s (every window
 * of a key lands on the same GPU, like a Redis cluster slot for the reference's INCRBY
 * pipeline, src/redis/fixed_cache_impl.go:66-80, driver_impl.go:56-90). All shards must use
 * the same hash_seed and rule table. One routed step:
 *   origin: rl_route_pack       batch -> records grouped by owner, per-owner counts
 *   RCCL:   all-to-all of counts, then of records (send_counts / received counts)
 *   owner:  rl_submit_routed    records received from every origin (origin-major) -> replies
 *   RCCL:   all-to-all of replies (reverse splits)
 *   origin: rl_route_unpack     replies -> rl_status[n_desc], ThrottleMillis[n_req]
 * An owner decides records in origin-major order, i.e. as if the origins' batches had been
 * submitted to one engine one after another. */
#define RL_ROUTE_RECORD_BYTES 32u
#define RL_ROUTE_REPLY_BYTES 24u
#define RL_ROUTE_MAX_SHARDS 16u
#define RL_ROUTE_MAX_REQ (1u << 27) /* requests per origin batch */
#define RL_ROUTE_LOCAL 0xFFFFFFFFu  /* perm[] value of a nil-limit descriptor (decided at the origin) */

/* Device batch -> d_send[n_desc routed records, grouped by owner 0..n_shards-1, serial order
 * inside each group], d_perm[n_desc] (record position, or RL_ROUTE_LOCAL), per-owner record
 * counts in d_send_counts[n_shards] and h_send_counts[n_shards]. Validates the batch
 * (unknown rule / request index, time outside [0, 2^32)) and synchronises the stream. */
int rl_route_pack(rl_engine* e, const rl_batch* device_batch, uint32_t origin, uint32_t n_shards, void* d_send,
                  uint32_t* d_send_counts, uint32_t* d_perm, uint32_t* h_send_counts);

/* rl_route_pack without the host round trip: the same records and d_perm, and for the count
 * exchange d_x[2 j] = records for owner j, d_x[2 j + 1] = 0 or RL_EINVAL when the device found
 * the batch malformed (an unknown rule / request index, a time outside the range) — the pair
 * each origin sends to owner j in the all-to-all of counts (router.py). Ordered on the engine
 * stream, nothing synchronised; argument errors are returned at once. */
int rl_route_pack_async(rl_engine* e, const rl_batch* device_batch, uint32_t origin, uint32_t n_shards, void* d_send,
                        uint32_t* d_x, uint32_t* d_perm);

/* rl_route_pack_async into a strided send buffer, in one kernel: owner j's records at
 * d_send[j * stride ...] (d_send holds n_shards * stride records), d_perm[i] = j * stride +
 * position, pairs in d_x as above (status RL_EDEVICE if the device's look-back spin expired).
 * For transports that take per-peer displacements (ncclAllToAllv; rl_router_step uses it):
 * no temporary records, no separate scan. n_desc must be <= stride <= 2^27. */
int rl_route_pack_strided(rl_engine* e, const rl_batch* device_batch, uint32_t origin, uint32_t n_shards,
                          uint32_t stride, void* d_send, uint32_t* d_x, uint32_t* d_perm);

/* Owner side: decide n routed records (device memory, RL_ROUTE_RECORD_BYTES each) and write
 * one reply per record (RL_ROUTE_REPLY_BYTES each: rl_status + ThrottleMillis) into d_reply.
 * Asynchronous like rl_submit_device; rl_wait() completes it. */
int rl_submit_routed(rl_engine* e, const void* d_records, uint32_t n, void* d_reply);

/* Owner side, asynchronous and pipelined: like rl_submit_routed, but with RL_ROUTED_RAW the
 * owner writes one raw reply per record (rl_raw_reply, 8 B: the INCRBY post-value the record
 * saw, or a local-cache hit) and the origin makes the decisions (rl_route_unpack_raw); the call
 * may be made while up to RL_MAX_IN_FLIGHT - 1 batches are in flight (distinct reply buffers),
 * and the pipeline waits on the device for ready_event (a hipEvent_t recorded after the records
 * arrived, e.g. on the stream of the exchange; NULL: ordered on the engine stream). flags = 0 is
 * rl_submit_routed (ready_event must be NULL). rl_wait completes the oldest batch. */
#define RL_ROUTED_RAW 1u
struct rl_raw_reply {
  uint32_t after; /* INCRBY post-value (uint32, as fixed_cache_impl.go:51 decodes it); 0 for a hit */
  uint32_t flags; /* RL_RAW_LOCAL_HIT: the key was in the local over-limit cache, no INCRBY;
                     RL_RAW_NIL: nil limit */
};
#define RL_RAW_LOCAL_HIT 1u
int rl_submit_routed_async(rl_engine* e, const void* d_records, uint32_t n, void* d_reply, uint32_t flags,
                           void* ready_event);

/* Origin side: replies (in d_send order) -> d_out[n_desc] and d_req_throttle_ms[n_req].
 * Ordered on the engine stream; no host synchronisation. */
int rl_route_unpack(rl_engine* e, const rl_batch* device_batch, const uint32_t* d_perm, const void* d_reply,
                    rl_status* d_out, uint32_t* d_req_throttle_ms);

/* ---- Router object: the routed step above behind one call ------------------------------
 * Owns the exchange buffers and the transport, so a non-Python host (the Go service over cgo)
 * can route without torch.distributed:
 *   RCCL transport  (rccl_id != NULL): one process per GPU, engines[0] = this rank's engine;
 *                   counts, records and replies move by ncclAllToAll / ncclAllToAllv over the
 *                   communicator the router owns (xGMI between GPUs of a node). rank 0 makes the
 *                   id with rl_router_unique_id and hands it to the others out of band.
 *   local transport (rccl_id == NULL): n_shards engines in this process (logical shards, one
 *                   device or several); the exchanges are device-to-device copies.
 * One step: each origin packs its batch by owner into a strided send buffer —
 * one record per descriptor, except that descriptors of a hot prefix (the router's route hot
 * set) are combined into one record carrying their sum of hits_addend (exact: one request time,
 * one rule, local cache off; otherwise the batch is packed without combining); counts, then
 * records move by all-to-all; each owner decides its records in origin order and answers each
 * with its raw INCRBY post-value (rl_raw_reply); the replies return by the reverse all-to-all
 * and the origin makes every descriptor's decision.
 * Every shard finishes every exchange of a step even when one fails, then all of them return
 * the failure: the failing shard its own code, the others RL_EPEER. The counts exchange
 * carries each origin's pack status, the reply exchange each owner's decide status (and any
 * local HIP failure after the counts), so a bad batch or a fault on one GPU cannot leave its
 * peers blocked in a collective. An RCCL failure aborts the communicator (ncclCommAbort) and
 * every later call returns RL_ECOMM. A refused owner batch (RL_ENOSPC, RL_ECAPACITY) leaves that
 * owner's table unchanged; other owners of the step have applied theirs (per-shard atomicity,
 * as a Redis cluster pipeline gives per-node): rl_router_stats.status says which, and after a
 * failure at an owner (decide or later) the outputs still hold every decision the healthy
 * owners made, the descriptors of a failed owner coming out with code RL_CODE_UNKNOWN (not
 * known to be applied) — the caller can answer those requests and fail only the others. After
 * a pack failure (any origin) nothing was applied anywhere and the statuses are untouched; the
 * ThrottleMillis words of origins whose pack ran may have been zeroed (the pack starts them at 0).
 * Request times: every origin's batch-time range travels with its counts. An owner decides its
 * records origin by origin in engine batches whose times span at most one second, so origins
 * whose clocks or batch cuts differ by seconds are exact. An origin whose batch starts more than
 * 3 s behind the newest request time before it (the step clock: earlier steps and the origins
 * before it in rank order) is left out of the step alone: its shard returns RL_ELATE with none of
 * its descriptors applied, every other shard's step goes ahead (the late shard still decides the
 * records it owns), and the clock does not move for it. */
#define RL_ROUTER_ID_BYTES 128u
typedef struct rl_router rl_router;

typedef struct rl_router_config {
  uint32_t struct_size;   /* sizeof(rl_router_config) */
  uint32_t n_shards;      /* 1..RL_ROUTE_MAX_SHARDS */
  uint32_t rank;          /* RCCL transport: this process's shard; local transport: 0 */
  uint32_t max_desc;      /* descriptors per origin batch (an owner can receive n_shards x this) */
  const uint8_t* rccl_id; /* RL_ROUTER_ID_BYTES from rl_router_unique_id, or NULL: local transport */
  uint32_t flags;         /* RL_ROUTER_* */
  uint32_t max_blob_bytes; /* host staging (RL_ROUTER_HOST): key-prefix bytes per origin batch (0 = 64 x max_desc) */
} rl_router_config;
enum {
  RL_ROUTER_NO_COMBINE = 1u, /* one record per descriptor (no hot-prefix combining) */
  RL_ROUTER_HOST = 2u,       /* allocate pinned host staging: rl_router_host_acquire / _submit_host / _wait_into */
  RL_ROUTER_EMULATED = 4u,   /* rccl_id is an rl_router_emu_world id: the collective transport's code path with
                                the collectives emulated in process (one thread per rank; tests) */
  RL_ROUTER_HOST_XCHG = 8u   /* the collectives through the host exchange registered by rl_router_use_host_xchg
                                (one process per rank where RCCL cannot run them; tests). rccl_id unused */
};

typedef struct rl_router_stats {
  uint64_t steps;
  uint32_t n_shards;
  int32_t status[RL_ROUTE_MAX_SHARDS]; /* last step: each shard's status (0 = ok, RL_EPEER = a peer failed) */
  uint32_t recv[RL_ROUTE_MAX_SHARDS];  /* last step: records each owner decided (RCCL: this rank's only) */
  uint32_t sent[RL_ROUTE_MAX_SHARDS];  /* last step: records origin 0 (RCCL: this rank) sent each owner */
  double pack_us, exchange_us, decide_us, decide_max_us, reply_us, unpack_us, step_us; /* last step, host clock */
  uint32_t hot_groups;     /* last step: route hot set size of origin 0 (RCCL: this rank) */
  uint32_t combined;       /* last step: combined records origin 0 (RCCL: this rank) sent (one per hot group) */
  uint64_t repacks;        /* steps packed again without combining (a hot group not one key string) */
  uint64_t combined_steps; /* steps whose origin 0 combined */
  uint32_t owner_batches;  /* last step: engine batches owner 0 (collective: this rank) decided its records in
                              (origins whose request times differ by 2 s or more go to separate batches) */
  uint32_t step_clock;     /* the newest request time of every step applied so far (unix seconds) */
  uint64_t late_steps;     /* steps in which this rank's origin batch (local transport: any shard's) was refused
                              with RL_ELATE */
} rl_router_stats;

/* A fresh RCCL unique id (ncclGetUniqueId), RL_ROUTER_ID_BYTES bytes. */
int rl_router_unique_id(uint8_t* id_out);
/* An in-process world of n_ranks emulated ranks (RL_ROUTER_EMULATED): the id to pass as
 * rccl_id to each rank's rl_router_create, every rank driven by its own thread. The collective
 * transport runs unchanged; ncclAllToAll / ncclAllToAllv / ncclAllGather become device copies
 * driven by the same count and displacement vectors, each rank's receive counts checked against
 * its peers' send counts. The world is freed when the last of its n_ranks routers is destroyed. */
int rl_router_emu_world(uint32_t n_ranks, uint8_t* id_out);
/* A host exchange (RL_ROUTER_HOST_XCHG; tests): an all-to-all-v of host bytes among the ranks of
 * a process group the caller runs (e.g. torch.distributed over gloo). Rank j's bytes for this
 * rank arrive at recv + recv_displs[j]; n_ranks counts and displacements each way. 0 = success.
 * The collective transport then runs its code path unchanged with one process per rank on any
 * number of GPUs — RCCL refuses two ranks on one device, so a one-GPU box cannot run it across
 * processes otherwise. Every collective stages through host memory: not for performance. The
 * registration holds for this thread's next rl_router_create with the flag. */
typedef int (*rl_host_xchg_fn)(void* ctx, const void* send, const size_t* send_counts, const size_t* send_displs,
                               void* recv, const size_t* recv_counts, const size_t* recv_displs);
int rl_router_use_host_xchg(rl_host_xchg_fn fn, void* ctx);
/* engines: n_shards engines (local transport) or 1 (RCCL transport). The router does not own
 * them; they must outlive it and be used by nothing else while a step runs. All engines share
 * hash_seed and the rule table. */
int rl_router_create(const rl_router_config* cfg, rl_engine* const* engines, rl_router** out);
/* One routed step, synchronous: rl_router_submit + rl_router_wait. batches / d_out /
 * d_req_throttle_ms: one per engine passed at create (device pointers; the same layouts as
 * rl_submit_device). Decisions equal one engine deciding the origins' batches one after
 * another in shard order. */
int rl_router_step(rl_router* r, const rl_batch* batches, rl_status* const* d_out, uint32_t* const* d_req_throttle_ms);
/* Pipelined steps: up to three in flight. rl_router_submit packs, exchanges counts, exchanges
 * the replies of the older steps in flight, exchanges records and hands the owner its records
 * (returns once they are queued); rl_router_wait completes the oldest step (its origin's
 * decisions) and returns its status. With two in flight, step k+1's pack overlaps step k's
 * decide on the device. Every
 * shard must make the same sequence of submit / wait calls (the collectives follow it). Inputs
 * and outputs of a step stay untouched by the caller until its wait returns. */
int rl_router_submit(rl_router* r, const rl_batch* batches, rl_status* const* d_out, uint32_t* const* d_req_throttle_ms);
int rl_router_wait(rl_router* r);
/* Host-memory steps (RL_ROUTER_HOST): a Go service on a multi-GPU node stages its batch in the
 * router's pinned memory — rl_router_host_acquire hands out the next step's slot of a shard
 * (RCCL: shard 0), C memory a cgo caller fills through unsafe slices — or passes any host
 * arrays (copied before rl_router_submit_host returns). rl_router_wait_into completes the oldest
 * step and copies each shard's statuses / ThrottleMillis into host memory during the call
 * (NULL entries discard). No caller memory is retained. */
int rl_router_host_acquire(rl_router* r, uint32_t shard, rl_host_batch* out);
int rl_router_submit_host(rl_router* r, const rl_batch* host_batches);
int rl_router_wait_into(rl_router* r, rl_status* const* out, uint32_t* const* req_throttle_ms);
/* A small collective over the router's transport (collective transports only): every rank
 * contributes n_bytes (<= RL_ROUTER_AG_MAX, the same on every rank) of host memory `in`, and out
 * receives n_shards * n_bytes in rank order. Synchronous. Every rank must make the same sequence
 * of router calls (steps and these), e.g. with no step in flight at the same step number: a
 * multi-GPU batcher uses it to agree new rules and a stop at the same step on every rank (rule
 * ids must mean the same limit on every owner). */
#define RL_ROUTER_AG_MAX 8192u
int rl_router_allgather_host(rl_router* r, const void* in, uint32_t n_bytes, void* out);
int rl_router_get_stats(const rl_router* r, rl_router_stats* out);
const char* rl_router_last_error(const rl_router* r);
void rl_router_destroy(rl_router* r);

/* Clear the counter table and local-cache state (FLUSHALL analogue; tests and restarts). */
int rl_reset(rl_engine* e);

int rl_get_stats(rl_engine* e, rl_engine_stats* s);
/* Table occupancy, from the engine's host mirror: no device call and no synchronisation. The
 * mirror is advanced by rl_wait / rl_wait_into as each batch completes, so the figures are those
 * after the last completed batch; batches still in flight are not in them yet. Legal at any point
 * on the engine's thread (a batcher reads it between rl_waits). */
int rl_get_occupancy(rl_engine* e, rl_occupancy* o);

/* Per-kernel timing with HIP events on the engine stream (off by default). When on, each
 * pipeline kernel is bracketed by an event pair; rl_kernel_times() returns the accumulated
 * milliseconds and launch counts for up to `cap` kernels, their names in names[] (static strings). */
int rl_set_timing(rl_engine* e, int on);
int rl_kernel_times(rl_engine* e, const char** names, double* total_ms, uint64_t* launches, uint32_t cap,
                    uint32_t* n_out);

/* Algorithmic-byte accounting for the last completed batch: unique keys U
 * (segments), descriptors, requests and prefix bytes, read back from the device. */
int rl_last_batch_info(rl_engine* e, uint64_t* unique_keys, uint64_t* n_desc, uint64_t* n_req,
                       uint64_t* blob_bytes);

/* ---- Snapshot / restore -------------------------------------------------
 * The counter table is the whole state of the backend (the hot set is a cache and is learned
 * again). A snapshot is a fixed header and one 32-B record per live table slot, verbatim: the
 * claim word (window generation | tag << 32), the sort key (region | 58 fingerprint bits), both
 * counters, the main store's expiry second and the local-cache deadline. A slot's place is the
 * top bits of its key, so the records restore into a table of any size: log2_slots may differ in
 * every region between the engine that saved and the one that loads. No counterpart in the
 * reference, whose counters live in Redis and survive a restart of the service there.
 *
 * What is live: a slot of region r whose generation g is not 0 and equals the region's newest
 * generation (rl_occupancy.gen[r]) or, in a lag region (RL_CFG_LAG_WINDOW, the two SECOND-home
 * regions), g + 2 == that generation — exactly the slots a request at the table's newest time
 * can still find. Record order is unspecified; the set is exact.
 *
 * Saving: rl_snapshot_begin (nothing in flight, else RL_ESTATE) compacts the live slots into a
 * device buffer sized from the occupancy mirror (one streaming pass over the table, then a
 * stream synchronise: that pass is the whole pause) and fills *out; live[] / prev[] are the
 * counts the pass exported. If the buffer cannot be allocated: RL_EHIP, nothing changed. From
 * then on the engine takes batches again: rl_snapshot_next copies the next at most cap_records
 * records of that device copy to host_buf (*n = 0: drained) and never reads the table, so the
 * records are the state at begin whatever was submitted since. rl_snapshot_end frees the copy
 * (legal at any point, also with none open). One snapshot at a time per engine.
 *
 * Loading: rl_restore_begin validates before anything changes — magic, header_bytes,
 * record_bytes, reserved words, seed_check against this engine's hash_seed, RL_SNAP_SPLIT and
 * RL_SNAP_LAG against its settings (RL_SNAP_LOCAL_CACHE may differ: the local-cache deadline of
 * a record is simply unused with the cache off), n_records against the per-region counts: RL_EINVAL
 * otherwise; live[r] + prev[r] over the region's load limit: RL_ENOSPC; either way the engine is
 * untouched. Needs nothing in flight (RL_ESTATE). Then the table, hot set and candidate stash
 * are cleared as rl_reset clears them, and every submit returns RL_ESTATE until rl_restore_end.
 * rl_restore_put imports n records from host memory (any chunking; staged through bounded pinned
 * memory); a call that would pass the header's n_records imports nothing and returns RL_EINVAL
 * (the restore stays open: rl_restore_end or rl_reset closes it). rl_restore_end checks what arrived against the header: on success the occupancy
 * becomes the header's {gen, live, prev} (the load limits stay this engine's) and
 * rl_engine_stats.live_keys follows; inserted_keys is cumulative and is not restored. A record
 * whose identity occurs twice, a generation that is neither gen[r] nor a lag region's gen[r] - 2,
 * or counts that differ from the header: RL_EINVAL, and the engine is left reset (empty).
 * rl_reset and rl_destroy close an open snapshot or restore.
 *
 * A routed deployment saves and loads per rank: a record does not carry what the owner hash
 * needs, so a restore needs the same n_shards and hash_seed; and such an engine must have
 * RL_CFG_LAG_WINDOW from rl_create, or its router created first, before it is restored. */
#define RL_SNAP_RECORD_BYTES 32u
#define RL_SNAP_HEADER_BYTES 256u
enum {
  RL_SNAP_SPLIT = 1u,       /* rl_config.per_second_split */
  RL_SNAP_LAG = 2u,         /* RL_CFG_LAG_WINDOW */
  RL_SNAP_LOCAL_CACHE = 4u  /* rl_config.local_cache (informational) */
};
typedef struct rl_snapshot_header { /* 256 B, little-endian, reserved words 0 */
  uint8_t magic[8];        /* "RLSNAP01" */
  uint32_t header_bytes;   /* RL_SNAP_HEADER_BYTES */
  uint32_t record_bytes;   /* RL_SNAP_RECORD_BYTES */
  uint32_t flags;          /* RL_SNAP_* */
  uint32_t reserved0;
  uint64_t seed_check;     /* a mix of hash_seed, never the seed itself (it is a secret) */
  uint64_t n_records;      /* = sum of live[] and prev[] */
  uint32_t gen[8];         /* per region: newest window generation (0 = unused) */
  uint32_t live[8];        /* records of that generation */
  uint32_t prev[8];        /* records of generation gen - 2 (lag regions; else 0) */
  uint32_t src_log2[8];    /* log2 of the region sizes of the engine that saved (informational) */
  uint32_t reserved[22];
} rl_snapshot_header;

int rl_snapshot_begin(rl_engine* e, rl_snapshot_header* out);
int rl_snapshot_next(rl_engine* e, void* host_buf, uint32_t cap_records, uint32_t* n);
int rl_snapshot_end(rl_engine* e);

int rl_restore_begin(rl_engine* e, const rl_snapshot_header* hdr);
int rl_restore_put(rl_engine* e, const void* host_recs, uint32_t n);
int rl_restore_end(rl_engine* e);

/* ---- Merge ------------------------------------------------------------------
 * Fold records of a snapshot into a table that is already serving: counters add, expiries and
 * local-cache deadlines take the later of the two, absent identities are claimed. Three uses:
 * a restarted process that answers at once and takes its last snapshot afterwards; the per-rank
 * snapshots of a routed deployment consolidated into one engine (records carry no key string and
 * need none); a blue/green handover, the new process taking the old one's counters while it
 * already serves. No counterpart in the reference, whose counters live in Redis.
 *
 * The call is stateless and synchronous and runs between batches: one call takes one chunk of a
 * snapshot's records from host memory (staged through the restore's bounded pinned memory), in
 * any order and in chunks of any size; there is no begin / end, so nothing stays open. The same
 * record in two calls adds twice: a caller must not repeat a chunk that was applied.
 *
 * Header: validated on every call as rl_restore_begin validates it (magic, header_bytes,
 * record_bytes, reserved words, seed_check against this engine's hash_seed, RL_SNAP_SPLIT against
 * per_second_split; RL_EINVAL otherwise). RL_SNAP_LAG and RL_SNAP_LOCAL_CACHE may differ: the
 * records are judged by this engine's rules. n_records and the per-region counts are not used (a
 * chunk is a subset).
 *
 * Records, checked on the host before anything is staged: RL_EINVAL for a generation of 0, for a
 * (region, generation) no engine writes (the window start of the generation in that region must
 * have exactly that region and generation as its place, and must not be above 0xFFFD0000), and
 * for now outside [0, 0xFFFD0000].
 *
 * Target generation per region: T[r] = max(rl_occupancy.gen[r], the largest generation among
 * this call's records of region r that leave something). A record of generation g applies as
 * newest when g == T[r], as previous when r is a lag region of this engine and g + 2 == T[r], and
 * is over otherwise (dropped_over). A snapshot newer than the table so advances the region
 * exactly as a batch does (the older slots turn stale); one older than the table is dropped.
 *
 * A record leaves something when now < exp, or pcount != 0, or this engine's local cache is on
 * and now < frz. Any other record is dropped_empty and claims nothing, even when its identity is
 * present.
 *
 * Fold, slot state S (zeros for a fresh claim) and record R, aR = now < R.exp, aS = found &&
 * now < S.exp:  aR && aS: count = S.count + R.count (mod 2^32, the counter's own width), exp =
 * max(S.exp, R.exp);  aR && !aS: count = R.count, exp = R.exp;  !aR: both words stay.
 * pcount = S.pcount + R.pcount (mod 2^32);  frz = max(S.frz, R.frz). For a caller: rl_peek at
 * `now` after the merge answers, for every key string, the sum of the counts, the larger TTL and
 * the larger cached seconds of what rl_peek at `now` answered on the two sides. That equals one
 * server that saw both histories when every string is counted under one unit, there is no EXPIRE
 * jitter, and the snapshot's touches are not later than the table's. With jitter the expiry is the
 * maximum rather than the last one; a string shared by rules of different units can differ where
 * an expiry falls between the two histories, which neither side can tell. The local cache is only
 * a cache, as the reference's freecache: a string over its limit only in the sum is not frozen
 * until its next INCRBY.
 *
 * Atomic per call, refused before anything changes (table, occupancy, stats and *report are then
 * untouched; after rl_resize the same chunk can be passed again):
 *   RL_ESTATE     a batch in flight, a restore open, or a routed-set plan open (an open snapshot
 *                 does not block)
 *   RL_ECAPACITY  n above max_batch_desc, or max_batch_desc above 2^29
 *   RL_EINVAL     the header and record checks above; one identity (claim word, key) twice in
 *                 the call (found by the planning pass on the device)
 *   RL_EDEVICE    two identities of the call share one 64-bit sort key: split the call (as rl_set)
 *   RL_ENOSPC     per region, the slots a key of generation T[r] cannot take plus the call's exact
 *                 number of absent identities that apply and leave something pass the load limit
 *   RL_EHIP       any HIP failure before the applying pass
 * A failure of the applying pass itself (RL_EHIP, or RL_EDEVICE for a region without a free slot,
 * which the RL_ENOSPC check rules out) may leave part of the call in the table.
 *
 * Occupancy: claims are counted per (region, class) on the device and enter the occupancy as a
 * batch's do, the newest class at T[r] and the previous class at T[r] - 2; inserted_keys grows by
 * the claims and live_keys follows. A region where the call claims nothing keeps its occupancy.
 * The hot set and the candidate stash are untouched. n == 0 validates the header and returns 0.
 *
 * Not provided: a router-level call (records carry no owner: merging is for consolidating into
 * one engine, or for a rank taking back its own snapshot, which this call on a router's engine
 * between steps already does), a device-memory form, and undoing a merge. */
typedef struct rl_merge_report {   /* 64 B */
  uint64_t records;        /* n of the call */
  uint64_t folded;         /* identity found in the table: the record's state folded into its slot */
  uint64_t claimed;        /* identity absent: a slot claimed, the record's state written */
  uint64_t dropped_over;   /* its window generation is over in this table */
  uint64_t dropped_empty;  /* it leaves nothing at `now` (looked at after dropped_over) */
  uint64_t reserved[3];    /* 0 */
} rl_merge_report;         /* records == folded + claimed + dropped_over + dropped_empty */

int rl_merge(rl_engine* e, const rl_snapshot_header* hdr, const void* host_recs, uint32_t n,
             int64_t now, rl_merge_report* report_or_null);

/* ---- Resize ---------------------------------------------------------------
 * Resize the counter table in place: log2_slots[u] slots per window generation for home unit u
 * (0 = keep that unit's size). Every live slot ("What is live" above) keeps its claim word, key,
 * counters, expiry and local-cache deadline; only its place changes. One device pass reads the
 * old table and claims each live slot's place in the new one (no host copy, no record buffer);
 * the call returns after a stream synchronise, and that pass plus the new table's clearing is
 * the whole pause. The hot set and the candidate stash hold key prefixes, not slots, and are
 * kept: the next batch runs as if nothing had happened. An open snapshot is a separate device
 * copy and does not block the call; rl_snapshot_next keeps draining the records of its begin.
 *
 * Refused before anything changes, the engine exactly as it was:
 *   RL_ESTATE  a batch is in flight (call rl_wait until none is: a resize while batches are in
 *              flight is out of scope), or a restore is open;
 *   RL_EINVAL  a non-zero log2 outside 4..31;
 *   RL_ENOSPC  a region's mirrored live + prev exceeds its new load limit,
 *              2^log2 * max_load_permille / 1000. The mirror never under-counts but may
 *              over-count, so a shrink to within a few slots of the true live count can be
 *              refused although it would fit: the check is conservative, never unsafe;
 *   RL_EHIP    the new table cannot be allocated. Old and new table coexist during the call:
 *              peak device memory is 32 B * (sum of old slots + sum of new slots), i.e. three
 *              times the old table for a doubling of every unit.
 * After the checks a failure of the pass itself — a device error word, a count above the
 * mirror's (RL_EDEVICE), a HIP error (RL_EHIP) — frees the new table; the old one was only read
 * and stays in service. Only on success the tables are swapped, the old one is freed, the load
 * limits follow the new sizes, the occupancy's live / prev become the exact counts of the pass
 * (gen is unchanged) and rl_engine_stats.live_keys follows; inserted_keys is cumulative and does
 * not change. Legal on a router's engine between steps.
 *
 * Auto-grow is the batcher's, not the engine's (rl_cache.hpp HipSettings::autogrow_permille,
 * HIP_TABLE_AUTOGROW): after each completed batch it reads rl_get_occupancy,
 * and when either parity region of a home unit holds more than slots * autogrow_permille / 1000
 * live slots and the unit is below its maximum (HIP_TABLE_MAX_SLOTS) it completes the batches in
 * flight and calls rl_resize with that unit's log2 + 1 — before a batch is refused with
 * RL_ENOSPC whenever the watermark is below max_load_permille. A single batch that jumps from
 * under the watermark to over the limit is still refused, and the growth follows it.
 * Out of scope: the routed batcher (every rank would have to resize between the same two
 * steps), and resizing while batches are in flight. */
int rl_resize(rl_engine* e, const uint32_t log2_slots[4]);

/* ---- Peek / forget: read and clear counters by key -----------------------
 * What an operator does to the Redis backend with GET / TTL domain_key_value_<window> and DEL,
 * and what freecache's Get answers for the local over-limit cache, by key and on the device. The
 * batch is an ordinary rl_batch, the one a caller would submit: hits_addend and ttl_jitter are
 * ignored and may be NULL; req_of and now give each descriptor its time.
 *
 * rl_peek: descriptor i reads exactly the state an rl_submit of the same batch would read for it
 * before its INCRBY, and writes nothing. The key string is prefix || decimal((now/div)*div) under
 * the rule's unit; its table region and window generation follow from that window start, its
 * store (main or per-second) from the rule's unit and rl_config.per_second_split.
 *   RL_PEEK_FOUND         main store: the string's slot exists for that generation and now < its
 *                         expiry; per-second store: the slot exists and its counter is not 0
 *   RL_PEEK_LOCAL_CACHED  rl_config.local_cache is on and now < the string's local-cache deadline
 *   RL_PEEK_NIL           the rule is RL_NIL_RULE: nothing is looked up
 *   RL_PEEK_PER_SECOND    the descriptor's store is the per-second one
 *   RL_PEEK_BAD           rl_peek_device only: a malformed descriptor (below); every other word 0
 * rl_forget: Redis DEL on the descriptor's store (main: counter and expiry; per-second: counter)
 * plus dropping the string's local-cache entry. The table slot stays claimed for its window
 * generation (open addressing without tombstones), so occupancy, live_keys and inserted_keys do
 * not change and the next INCRBY of the string starts from 0, exactly as after DEL. A string
 * that is absent is left alone: nothing is claimed. out (may be NULL) receives each descriptor's
 * reply as rl_peek would have given it before the call, duplicates within the call included. The
 * hot set and the candidate stash hold prefixes, not counters, and are not touched.
 *
 * rl_peek / rl_forget take host memory and are synchronous (staged through a free host staging
 * slot, never the one rl_host_acquire handed out; results rl_wait_view handed out stay valid).
 * Before anything is staged they refuse: an unknown rule id, a time outside [0, 0xFFFD0000], a
 * decreasing req_of or a request index >= n_req, prefix offsets out of order or past blob_bytes
 * (RL_EINVAL); n_desc, n_req or blob_bytes over the engine's capacities (RL_ECAPACITY).
 * rl_peek_device takes device memory (the blob readable for RL_BLOB_SLACK bytes past blob_bytes,
 * as for rl_submit_device), runs on the engine stream and returns at once; it cannot see such an
 * error, so a malformed descriptor gets flags = RL_PEEK_BAD and zeros, and the others are answered.
 * All three return RL_ESTATE while a batch is in flight (the rl_get_occupancy rule: a batcher
 * calls them between batches) and between rl_restore_begin and rl_restore_end. An open snapshot
 * does not block them: the snapshot is the state at its begin.
 *
 * A routed deployment: each rank's engine answers only for the keys it owns (the others read as
 * absent there), so a router is asked through rl_router_peek / rl_router_forget ("Routed peek /
 * forget" below), which send every key to its owner. Out of scope: a compact wire form. */
enum {
  RL_PEEK_FOUND = 1u,
  RL_PEEK_LOCAL_CACHED = 2u,
  RL_PEEK_NIL = 4u,
  RL_PEEK_PER_SECOND = 8u,
  RL_PEEK_BAD = 16u
};
typedef struct rl_peek_reply { /* 16 B */
  uint32_t count;    /* GET: the counter INCRBY would add to (0 when not found) */
  uint32_t ttl_s;    /* main store: expiry second - now (> 0 when found); per-second store: 0 (the table keeps
                        no TTL for it) */
  uint32_t cached_s; /* local over-limit cache: deadline - now when LOCAL_CACHED, else 0 */
  uint32_t flags;    /* RL_PEEK_* */
} rl_peek_reply;
int rl_peek(rl_engine* e, const rl_batch* host_batch, rl_peek_reply* out);
int rl_peek_device(rl_engine* e, const rl_batch* device_batch, rl_peek_reply* d_out);
int rl_forget(rl_engine* e, const rl_batch* host_batch, rl_peek_reply* out_or_null);

/* ---- Set: write counters by key -------------------------------------------
 * Redis SET key n EX ttl, per store, plus freecache's Set / Del on the string's local over-limit
 * cache entry: the write that completes rl_peek (read) and rl_forget (clear). It is what a cutover
 * from a live Redis deployment (resp.py import_batch), a correction of one key and a move of keys
 * between engines ("peek there, set here") are made of. host_batch is an ordinary batch, read as
 * rl_peek reads it (hits_addend and ttl_jitter ignored, may be NULL); values[i] says what
 * descriptor i's key string holds afterwards, in the rl_peek_reply that peek and forget speak;
 * out (may be NULL) receives what rl_peek would have answered just before the call, duplicates
 * within the call included (rl_forget's rule). Host memory, synchronous.
 *
 * Descriptor i, with t = now[req_of[i]] and its rule's unit giving the store and the window
 * (RL_NIL_RULE: nothing):
 *   counter part, unless RL_SET_KEEP_COUNTER:
 *     RL_PEEK_FOUND      main store: count = values[i].count, expiry = t + ttl_s;
 *                        per-second store: counter = count (ttl_s ignored: the table keeps no TTL
 *                        there; count == 0 is the store's "absent", so it reads back as not found
 *                        and, like a DEL, claims nothing)
 *     otherwise          DEL on that store, exactly what rl_forget writes
 *   cache part, unless RL_SET_KEEP_CACHE, and only when rl_config.local_cache is on (else ignored):
 *     RL_PEEK_LOCAL_CACHED  deadline = t + cached_s;  otherwise  no entry (deadline 0)
 * RL_PEEK_NIL, RL_PEEK_PER_SECOND and RL_PEEK_BAD in values are ignored, so a peek reply can be fed
 * back verbatim, and after rl_set(b, v) without KEEP bits rl_peek(b) returns v wherever v's
 * (count, ttl_s, cached_s) are 0 under a clear flag (PER_SECOND / NIL recomputed; the per-second
 * count == 0 case above excepted). Each part is written as its own 32-bit stores: two descriptors
 * that write the two stores of one shared string lose nothing. A descriptor with both KEEP bits
 * (or KEEP_COUNTER with the local cache off) is a peek.
 *
 * Claims: an absent string gets a table slot (zero state first; the pipelines' own claim) only if
 * the call leaves something in it, a FOUND counter or a cache deadline. A pure DEL or a peek of an
 * absent string claims nothing.
 * Duplicates: the same (string, store) may occur several times. The last in descriptor order wins
 * its counter part, and the last descriptor of the string that writes the cache part wins that
 * part — a pipeline of Redis SETs. The result does not depend on scheduling.
 * Occupancy: per region the call claims in, the claims (distinct absent strings that get
 * something, counted on the device) and the call's window generation there go through the batch's
 * occupancy update, on the device and in the host mirror: rl_engine_stats.inserted_keys grows by
 * the claims, live_keys follows, and a region whose generation the call advances leaves its
 * older slots stale, exactly as a batch does. A region where the call claims nothing keeps its
 * occupancy word for word. The hot set and the candidate stash hold prefixes and are untouched.
 *
 * Refused before anything changes (table, occupancy, mirror, stats and out exactly as before):
 *   RL_ESTATE     a batch in flight, or between rl_restore_begin and rl_restore_end (an open
 *                 snapshot does not block the call)
 *   RL_ECAPACITY  rl_peek's capacity limits (and max_batch_desc above 2^29)
 *   RL_EINVAL     anything rl_peek refuses; values == NULL with n_desc > 0; of the parts a
 *                 descriptor writes: a FOUND main-store value with ttl_s == 0, a LOCAL_CACHED value
 *                 with cached_s == 0, t + ttl_s or t + cached_s not below 2^32; among the
 *                 descriptors that write something: two window generations of one region in one
 *                 call (split the call: the batch rule behind a window span error), or a window
 *                 generation that is neither the region's newest, nor newer, nor a lag region's
 *                 newest - 2 (that window is over)
 *   RL_ENOSPC     a region's live slots plus the call's claims there would pass its load limit
 *   RL_EDEVICE    two identities of the call share one 64-bit sort key (split the call), found by
 *                 the planning pass: nothing written
 * Every check above runs before the applying pass, and so does every HIP failure of the staging,
 * indexing and planning passes (RL_EHIP): nothing written. A failure of the applying pass itself
 * (RL_EHIP, or RL_EDEVICE for a region without a free slot, which the RL_ENOSPC check rules
 * out) leaves the table with some of the call's writes and the occupancy not advanced: the engine
 * is to be reset or restored, as after any failed stream.
 * The index (32 B x the power of two >= 2 x max_batch_desc) and two per-descriptor scratch arrays
 * (40 B x max_batch_desc) are allocated at the first call and kept.
 * Behind a router the call is rl_router_set ("Routed set" below).
 * Out of scope: a device-memory public form, a compact wire form. */
enum { RL_SET_KEEP_COUNTER = 32u, RL_SET_KEEP_CACHE = 64u }; /* rl_peek_reply.flags, input only */
int rl_set(rl_engine* e, const rl_batch* host_batch, const rl_peek_reply* values, rl_peek_reply* out_or_null);

/* ---- Adjust: signed counter corrections by key -------------------------------
 * Redis INCRBY / DECRBY by key, outside a decision: what a cost limiter (hits_addend as tokens,
 * bytes, credits) needs to give a charge back (a refund: the request failed downstream, was
 * rejected by a later stage or was cancelled) and to replace an estimate by the real cost (a
 * true-up, positive or negative). A submit can only add, and rl_peek + rl_set(KEEP_CACHE) is a
 * read-modify-write through the host that loses every increment in between and cannot sum two
 * corrections of one key in one call. host_batch is an ordinary batch, read exactly as rl_peek
 * reads it (hits_addend and ttl_jitter ignored, may be NULL; req_of and now give descriptor i its
 * time t); delta[i] is descriptor i's signed correction. Host memory, synchronous, between batches.
 * No decision, no stat increment and no local-cache hit comes of it.
 *
 * Store and identity: rl_peek's. The key string is prefix || decimal window start under the rule's
 * unit; the store is the main or the per-second one by rl_config.per_second_split.
 * Found: rl_peek's RL_PEEK_FOUND at t, word for word. Main store: the string's slot exists for that
 * window generation and t < its expiry; per-second store: the slot exists and its counter is not 0.
 * Not found: the descriptor is `absent`: nothing is written and nothing is ever claimed. A
 * correction belongs to the window that was charged; if that window is over, it is dropped. So
 * occupancy, the host mirror, inserted_keys, live_keys, the hot set and the candidate stash never
 * change, and RL_ENOSPC cannot occur.
 *
 * Sum per (string, store) pair: net = the 64-bit sum of delta[i] over the call's found descriptors
 * of the pair, and new = clamp(count + net, 0, 0xFFFFFFFF), applied once per pair. The result
 * depends on neither the descriptor order nor scheduling: a counter of 5 with deltas (-10, +3)
 * ends at 0, not 3. The call is one atomic INCRBY net, not a pipeline of INCRBYs.
 * Saturation at both ends is deliberate. Redis would go negative, and the reference decodes the
 * reply as uint32, which would leave the key over its limit for its whole window; at the top a
 * wrapped counter would forgive everything. The reference has no such command, so parity is
 * unpinned here by construction.
 * What is written, as separate 32-bit stores (two pairs may share one slot). Main store: count =
 * new; the expiry is never touched, so a counter that reaches 0 keeps its TTL and reads back FOUND
 * with count 0, as after DECRBY. Per-second store: counter = new; 0 is that store's "absent", so it
 * reads back as not found.
 *
 * Cache part, only with rl_config.local_cache on and without RL_ADJUST_KEEP_CACHE: a pair qualifies
 * when net < 0 and new <= the smallest requests_per_unit among the call's found descriptors of that
 * pair; a string with at least one qualifying pair loses its local-cache deadline (set to 0), and
 * `unfrozen` counts the strings whose deadline word was non-zero, each once. Without it a refunded
 * key would stay OVER_LIMIT until its window ends. A positive net never freezes anything: the
 * cache is only a cache, the next INCRBY freezes the key (rl_merge's rule).
 *
 * out (may be NULL) receives rl_peek's reply for every descriptor as of just before the call,
 * duplicates included (rl_forget's rule); with every delta 0 the call is a peek. Untouched: rule
 * stats, the cache-stats counters, the step clock and every field of rl_engine_stats.
 *
 * Report: descriptors == nil + absent + applied. floored / capped count the pairs whose count + net
 * fell below 0 / rose above 0xFFFFFFFF and stopped there (a sum of exactly 0 is not floored).
 *
 * Refused before anything changes (table, out and *report untouched):
 *   RL_ESTATE     a batch in flight, a restore open, or a routed set or adjust plan open (an open
 *                 snapshot does not block the call)
 *   RL_ECAPACITY  rl_peek's capacity limits, or max_batch_desc above 2^29
 *   RL_EINVAL     everything rl_peek refuses; delta == NULL with n_desc > 0; any flag bit other than
 *                 RL_ADJUST_KEEP_CACHE
 *   RL_EDEVICE    the scratch index had no entry left (unreachable: it has 2^k >= 2 n_desc entries);
 *                 the applying pass then writes nothing
 *   RL_EHIP       any HIP failure before the applying pass
 * n_desc == 0 returns 0 and zeroes the report.
 * Scratch: the call runs in rl_set's scratch (its index, 32 B x the power of two >= 2 x
 * max_batch_desc, its control block, and its staged-value array for the 4 B x n_desc deltas), which
 * is allocated at the first rl_set or rl_adjust and kept: both calls are synchronous and exclude each
 * other, and an open routed-set plan, which lives there, refuses this one. The batch goes through
 * rl_peek's free host staging slot; the replies pass through 16 B x max_batch_desc of pinned memory,
 * allocated at the first call that asks for them.
 * The routed forms (rl_router_adjust; rl_adjust_routed_plan / _commit over routed records) are
 * "Routed adjust" below; the device-memory form and adjusting while batches are in flight are
 * "Adjust in flight" below. Out of scope: a compact wire form. */
enum { RL_ADJUST_KEEP_CACHE = 1u };
typedef struct rl_adjust_report {   /* 64 B */
  uint64_t descriptors;  /* n_desc of the call */
  uint64_t nil;          /* RL_NIL_RULE descriptors: nothing looked up */
  uint64_t absent;       /* descriptors with a limit whose counter was not found: nothing written */
  uint64_t applied;      /* descriptors whose counter was found: delta entered its pair's sum (delta 0 too) */
  uint64_t floored;      /* (string, store) pairs whose result stopped at 0 */
  uint64_t capped;       /* pairs whose result stopped at 0xFFFFFFFF */
  uint64_t unfrozen;     /* strings whose non-zero local-cache deadline the call cleared */
  uint64_t reserved;     /* 0 */
} rl_adjust_report;      /* descriptors == nil + absent + applied */
int rl_adjust(rl_engine* e, const rl_batch* host_batch, const int32_t* delta, uint32_t flags,
              rl_peek_reply* out_or_null, rl_adjust_report* report_or_null);

/* ---- Adjust in flight ---------------------------------------------------------
 * rl_adjust without stopping the engine: the adjust is queued between the batches in flight and
 * completes in its turn. A cost limiter makes about one adjust per decision (the true-up or refund
 * when a request ends); with rl_adjust each of them waits out the pipeline first.
 *
 * Semantics are rl_adjust's, word for word, taken at the call's place in submission order among the
 * flights: identity, the found rule, the per-pair 64-bit sum, the clamp, the cache part and the
 * report. Nothing is claimed; rl_engine_stats, rule stats and cache stats are not touched.
 *
 * rl_adjust_pipelined: the batch's arrays and d_delta (n_desc words) are device memory, as for
 * rl_submit_pipelined; hits_addend and ttl_jitter are not read. d_reply_or_null receives the n_desc
 * replies in device memory. Returns at once. The kernels run on the engine stream, behind everything
 * queued there. The caller leaves the arrays alone until the flight's wait has returned (a flight
 * behind a refused batch reads them again).
 * rl_adjust_submit: host memory. The batch's arrays are the rl_host_acquire slot's (no copy) or any
 * host memory (copied before the call returns); delta is always copied, through 4 B x max_batch_desc
 * of pinned and of device staging per slot, allocated at the first call and kept. want_replies != 0
 * keeps the replies for rl_wait_adjust. The call stages through the slot rl_host_acquire hands out
 * and consumes it, as rl_submit does: a batch that is being built in an acquired slot and is not
 * this call's is overwritten, so a caller that builds a decision batch in place submits that batch
 * first and the adjust behind it (the batcher's order, rl_cache.hpp AdjustQueued).
 * rl_wait_adjust: completes the oldest flight, which must be an adjust. out (host form with
 * want_replies only; may be NULL) receives the replies, *report (may be NULL) the report.
 *
 * Flights: a flight of either kind counts towards RL_MAX_IN_FLIGHT, and one more returns RL_ESTATE.
 * rl_wait completes an adjust flight and discards its report; rl_query works on it. rl_wait_into,
 * rl_wait_view and rl_wait_raw_* on an adjust flight, and rl_wait_adjust on a batch, return RL_ESTATE
 * and complete nothing. Everything that needs the engine quiet keeps returning RL_ESTATE while an
 * adjust is in flight (the synchronous by-key calls, snapshot begin, restore, merge, resize, census,
 * the stats reads, rl_set_stream, the routed plans). Both submit calls return RL_ESTATE with a
 * restore or a routed plan open (the adjust runs in rl_set's scratch), and, behind another flight,
 * without the v4 pipeline (RL_CFG_LSD_ONLY, or too many rules: rl_submit_pipelined's rule). With
 * nothing in flight they are legal in every mode.
 *
 * Refused at once, no flight added: rl_adjust's list (RL_ECAPACITY: the capacities, max_batch_desc
 * above 2^29; RL_EINVAL: reserved, null arrays, unknown flag bits), and for the host form everything
 * rl_adjust refuses of a batch's contents. The device form cannot see the contents: a malformed
 * descriptor (rule id at or above the loaded count and not RL_NIL_RULE, request index at or above
 * n_req, req_of decreasing, offsets out of order or past blob_bytes, time outside [0, 0xFFFD0000])
 * gets RL_PEEK_BAD, the applying pass writes nothing at all, and the wait returns RL_EINVAL;
 * d_reply still holds the state before the call for the well-formed descriptors. So the call is all
 * or nothing, as rl_adjust is. A refused or failed host-form flight leaves out untouched.
 * n_desc == 0 is a legal empty flight with a zero report.
 * RL_EHIP from either submit call (a launch or copy the runtime refused) adds no flight, but what
 * was queued before the failure still runs, as after such a failure in rl_adjust's applying pass:
 * the table may hold the call.
 *
 * Order against a refused batch: a batch the bucketed pipeline refuses is rerun by the host at its
 * wait, after everything queued behind it has run on the device. An adjust queued behind such a batch
 * finds the batch's poison word set, writes nothing (neither table nor replies) and is run again by
 * the wait, behind the batch's rerun and before the flight behind it, so the serial order holds.
 * Such an adjust does not count in rl_engine_stats.lsd_fallbacks. */
int rl_adjust_pipelined(rl_engine* e, const rl_batch* device_batch, const int32_t* d_delta, uint32_t flags,
                        rl_peek_reply* d_reply_or_null);
int rl_adjust_submit(rl_engine* e, const rl_batch* host_batch, const int32_t* delta, uint32_t flags,
                     int want_replies);
int rl_wait_adjust(rl_engine* e, rl_peek_reply* out_or_null, rl_adjust_report* report_or_null);

/* ---- Refund -------------------------------------------------------------------
 * Gives a rejected request's hits back, on the device. An extension, opt-in per call: the reference
 * issues INCRBY for every descriptor that is not a local-cache hit, whatever the verdict
 * (fixed_cache_impl.go:60-80), and only ORs the codes afterwards (ratelimit.go:208-215), so a request
 * it rejects is still charged on every one of its descriptors. For a cost limiter (hits_addend as
 * tokens, bytes, credits) that is the largest source of wrong charges: a request of cost 1500 that
 * meets a counter at 9000 / 10000 leaves it at 10500, and a request of cost 100 behind it is refused
 * although 1000 units remain; a request rejected by its global descriptor has still spent its
 * per-user descriptor's quota. Everything the correction needs is in device memory when the batch
 * ends (the statuses, req_of, hits_addend, the key prefixes), so no status is read back.
 *
 * Which descriptors are owed: a request is rejected when any of its descriptors has code
 * RL_CODE_OVER_LIMIT in d_status (a shadowed descriptor is RL_CODE_OK with RL_FLAG_SHADOW and rejects
 * nothing). A descriptor of a rejected request is owed max(1, hits_addend[req_of[i]]), the over-limit
 * descriptor itself included (it was counted), unless its rule is RL_NIL_RULE or its status carries
 * RL_FLAG_LOCAL_CACHE_HIT: no INCRBY happened for those. Every other descriptor is skipped: no
 * lookup is made for it. The amount is the full uint32 and is summed in 64 bits: it never passes
 * through an int32 delta, so hits_addend of 2^31 and 2^32 - 1 refund exactly. d_amount_or_null
 * (n_desc words of device memory) receives the amount per descriptor, 0 for a skipped one.
 *
 * What is written: rl_adjust's rules ("Adjust" above), word for word, with net = -(the sum of the
 * amounts over the call's found descriptors of a (string, store) pair): identity, store and "found"
 * at the descriptor's own request time; nothing is ever claimed; the result is clamped at 0; the
 * expiry is untouched; each pair is written once. The cache part is rl_adjust's, RL_REFUND_KEEP_CACHE
 * is RL_ADJUST_KEEP_CACHE: a pair with new <= its smallest limit gets its string's local-cache
 * deadline cleared, so a key a rejected request froze and the refund brought back under its limit
 * counts again. Untouched, as for an adjust: rule stats, cache stats, rl_engine_stats, occupancy,
 * the hot set and the candidate stash. The statuses of the refunded batch are not rewritten: the
 * answer stays the reference's. The refund is after the fact, not an atomic multi-descriptor
 * decision: later descriptors of the same batch were decided on the counters before it.
 *
 * rl_refund_pipelined: the batch's arrays (hits_addend included; ttl_jitter is not read), d_status
 * (n_desc statuses) and d_amount are device memory; the caller leaves them alone until the flight's
 * wait has returned. rl_refund_behind: refunds the most recently submitted flight, which must be a
 * decision batch with statuses on the device (rl_submit, rl_submit_device, rl_submit_pipelined) and
 * still be in flight; it reads that flight's own device arrays and statuses, so a host batcher
 * passes no pointer. RL_ESTATE when nothing is in flight or the newest flight is an adjust, a
 * refund, a compact (rl_submit_c) or a routed batch. A host batch's staging slot is held for the
 * refund: the slot's next copy-in is ordered behind the refund's kernels on the device.
 *
 * Flights: a refund is a flight exactly as an adjust is ("Adjust in flight" above): it counts
 * towards RL_MAX_IN_FLIGHT, completes in submission order, runs on the engine stream, and the same
 * RL_ESTATE gates apply (a restore or a routed plan open; behind another flight only with the v4
 * pipeline). rl_wait completes it and drops the report; rl_query works on it. rl_wait_refund on
 * anything else, and rl_wait_adjust, rl_wait_into, rl_wait_view and rl_wait_raw_* on a refund,
 * return RL_ESTATE and complete nothing. Behind a batch the bucketed pipeline refused, every refund
 * kernel finds the poison word, writes nothing, and the wait runs the whole refund again behind the
 * batch's rerun, marking pass included: the statuses are final only then.
 * A batch that fails on the device (RL_ENOSPC, a window span, RL_EDEVICE, bad input: its wait returns
 * the error) wrote no statuses, and its status array still holds whatever an earlier batch left
 * there. rl_refund_behind, and rl_refund_pipelined when d_status is the status array of the most
 * recently submitted flight, read that batch's device error word first: behind a failed batch every
 * refund kernel writes nothing and the refund's wait returns RL_ESTATE. rl_refund_pipelined with any
 * other d_status cannot be tied to a batch: the caller passes only statuses of a batch whose wait
 * has returned 0.
 * Refused at once, no flight added: rl_adjust_pipelined's list, a null d_status or hits_addend, a
 * flag bit other than RL_REFUND_KEEP_CACHE. A descriptor rl_peek_device would answer RL_PEEK_BAD
 * makes the wait return RL_EINVAL with nothing written. n_desc == 0 is an empty flight with a zero
 * report. Scratch: rl_set's, and 4 B x max_batch_req. */
enum { RL_REFUND_KEEP_CACHE = 1u };
typedef struct rl_refund_report {  /* 64 B */
  uint64_t descriptors;   /* n_desc of the refunded batch */
  uint64_t rejected_req;  /* requests with at least one descriptor of code RL_CODE_OVER_LIMIT */
  uint64_t skipped;       /* descriptors that refund nothing: no lookup made */
  uint64_t absent;        /* owed a refund, counter not found: nothing written */
  uint64_t refunded;      /* owed a refund, counter found: amount entered its pair's sum */
  uint64_t floored;       /* (string, store) pairs whose result stopped at 0 */
  uint64_t unfrozen;      /* strings whose non-zero local-cache deadline was cleared */
  uint64_t reserved;      /* 0 */
} rl_refund_report;       /* descriptors == skipped + absent + refunded */
int rl_refund_pipelined(rl_engine* e, const rl_batch* device_batch, const rl_status* d_status, uint32_t flags,
                        uint32_t* d_amount_or_null);
int rl_refund_behind(rl_engine* e, uint32_t flags);
int rl_wait_refund(rl_engine* e, rl_refund_report* report_or_null);

/* ---- Routed peek / forget --------------------------------------------------
 * The same lookups where the keys are spread over the shards of a router.
 *
 * Engine level (the pieces a router call is made of; device memory, ordered on the engine
 * stream, returning at once):
 * rl_peek_routed: the owner's lookup of n routed records (RL_ROUTE_RECORD_BYTES each, as
 * rl_route_pack_strided writes them: prefix lanes, request time, rule id), one rl_peek_reply per
 * record into d_reply. The key string's identity is rebuilt from the record as the owner's decision
 * path rebuilds it, and from there the lookup is rl_peek_device's own code. A record whose rule id
 * is at or above the loaded rule count, or whose time is above 0xFFFD0000, gets RL_PEEK_BAD and
 * zeros. With RL_PEEK_ROUTED_FORGET the lookup pass over all n records is followed by the clearing
 * pass over the same records (rl_forget's order: every duplicate reports the state before the
 * call); d_reply may then be NULL. RL_ESTATE while a batch is in flight or a restore is open;
 * n == 0 launches nothing.
 * rl_route_unpack_peek: the origin's side. d_out[i] = {0, 0, 0, RL_PEEK_NIL} when d_perm[i] is
 * RL_ROUTE_LOCAL, else d_back[d_perm[i]]: d_perm as rl_route_pack_strided wrote it, d_back the
 * owners' replies strided like the send buffer. Reads only n_desc of the batch.
 *
 * rl_router_peek / rl_router_forget: host memory in and out, synchronous; one batch and one output
 * per engine passed at create (local transport: n_shards, collective transports: one).
 * hits_addend and ttl_jitter are ignored and may be NULL. Collective: every rank makes the call at
 * the same place in its sequence of router calls; a rank with nothing to ask passes n_desc == 0.
 * With a step in flight the call returns RL_ESTATE before any collective (by the router's contract
 * every rank is then in the same state). Each origin packs its batch by owner (one record per
 * descriptor, no combining), counts and records move as in a step, each owner runs rl_peek_routed
 * over everything it received (origin-major), the 16-B replies return by the reverse exchange and
 * the origin unpacks them. A forget's owners run the lookup pass over all received records before
 * the clearing pass, so every duplicate of a string, across descriptors and across origins of
 * the call, reports the state before the call.
 * Refused before anything is staged: rl_peek's list (RL_EINVAL), a rule id at or above 0xFFFF (the
 * record's rule word shares its upper half; RL_EINVAL), n_desc / n_req over the router's max_desc
 * or blob_bytes over its max_blob_bytes (RL_ECAPACITY). Such a refusal, a staging or allocation
 * failure and a pack status travel as this origin's status in the counts exchange, as a step's
 * pack status does: if any origin's is non-zero no owner looks up or clears anything, every rank
 * still finishes the counts exchange, the failing rank returns its code (local transport: the
 * first failing shard's code) and the others RL_EPEER, and out is untouched — a forget is
 * all-or-nothing across ranks for every failure the call can see before records move. A HIP or
 * communicator failure after that returns RL_EHIP / RL_EPEER / RL_ECOMM as a step's does, and a
 * forget may then have been applied at some owners: the per-node atomicity of a Redis cluster DEL
 * pipeline. The call does not move the step clock, cannot return RL_ELATE, does not touch the hot
 * sets and leaves rl_router_stats alone. Its two reply buffers (and, without RL_ROUTER_HOST, its
 * input staging) are allocated at the first call; everything else is a free step slot's. */
enum { RL_PEEK_ROUTED_FORGET = 1u };
int rl_peek_routed(rl_engine* e, const void* d_records, uint32_t n, rl_peek_reply* d_reply, uint32_t flags);
int rl_route_unpack_peek(rl_engine* e, const rl_batch* device_batch, const uint32_t* d_perm,
                         const rl_peek_reply* d_back, rl_peek_reply* d_out);
int rl_router_peek(rl_router* r, const rl_batch* host_batches, rl_peek_reply* const* out);
int rl_router_forget(rl_router* r, const rl_batch* host_batches, rl_peek_reply* const* out_or_null);

/* ---- Routed set --------------------------------------------------------------
 * rl_set where the keys are spread over the shards of a router: the cutover of a multi-GPU
 * deployment from Redis (every rank imports whatever share of the SCAN it likes) and the move of
 * counters to a router of another size ("peek there, set here"; a snapshot needs the same
 * n_shards). A routed set can claim table slots and can be refused at an owner after the records
 * have moved (RL_ENOSPC, a window generation that is over, two identities on one sort key), so it is
 * two-phase: every owner plans, the plan statuses are exchanged, and only if all are zero does any
 * owner write.
 *
 * Engine level (device memory, between batches):
 * rl_set_routed_plan: phase 1 over n routed records (RL_ROUTE_RECORD_BYTES each, as
 * rl_route_pack_strided writes them) with one value each beside them (d_values[i] for record i,
 * rl_set's value semantics). Replies (the state before the call, rl_peek_routed's) go to d_reply
 * when it is not NULL; then the records are indexed and planned exactly as rl_set's descriptors are.
 * Record order is the serial order: the last record of a string that writes a part wins it. The
 * call synchronises the engine stream. 0: a plan is open and nothing has been written. Any other
 * return: nothing written and no plan open:
 *   RL_ESTATE     a batch in flight, a restore open, or a plan already open
 *   RL_ECAPACITY  n above max_batch_desc, or max_batch_desc above 2^29
 *   RL_EINVAL     null arrays with n > 0; a record whose rule id is not below the loaded rule
 *                 count or whose time is above 0xFFFD0000; of the parts a record writes: a FOUND
 *                 main-store value with ttl_s == 0, a LOCAL_CACHED value with cached_s == 0, a sum
 *                 with the time not below 2^32; two window generations of one region among the
 *                 records that write something; a generation that is over (rl_set's rule). All of
 *                 these are found on the device: the owner's host never sees records or values
 *   RL_EDEVICE    two identities share one 64-bit sort key, or the index overflowed
 *   RL_ENOSPC     rl_set's check: a region's live slots plus the plan's claims pass its load limit
 *   RL_EHIP
 * n == 0 opens an empty plan whose commit does nothing (a rank that receives nothing keeps the
 * collective sequence). While a plan is open every entry point that an open restore refuses
 * returns RL_ESTATE (rl_adjust_routed_plan and rl_adjust_routed_commit too); rl_reset and rl_destroy
 * close the plan.
 * rl_set_routed_commit: phase 2. apply != 0 runs rl_set's applying pass and publishes the occupancy
 * exactly as rl_set does (and fails as it does); apply == 0 drops the plan. RL_ESTATE with no plan
 * open. Either way the plan is closed.
 *
 * rl_router_set: rl_router_forget's contract. Collective; one batch, one value array and one output
 * (or NULL) per engine passed at create; host memory, synchronous; a rank with nothing to set passes
 * n_desc == 0; RL_ESTATE before any collective while a step is in flight.
 *   1. Origin: rl_router_peek's refusals plus rl_set's per-value checks; the batch and the values are
 *      staged, packed by owner (one record per descriptor) and the values laid out like the records.
 *      A refusal here travels as this origin's status in the counts exchange: nothing is planned
 *      anywhere, the failing rank returns its code (local transport: the first failing shard's) and
 *      the others RL_EPEER.
 *   2. Counts, then records and values in one collective group.
 *   3. Every owner runs rl_set_routed_plan over everything it received, origin-major: "the last SET
 *      wins" is taken with the origins' batches one after another in shard order, descriptor order
 *      inside each, per part.
 *   4. Each owner's plan code goes to every rank. If any is non-zero every owner drops its plan:
 *      the failing rank returns its code and the others RL_EPEER (local transport: the first failing
 *      shard's code). No owner has written anything and out is untouched.
 *   5. Every owner commits; the replies (the state before the call, for every duplicate across
 *      descriptors and origins) and the commit status return by the reverse exchange and the origin
 *      unpacks them into out. A HIP or communicator failure in this phase leaves per-owner
 *      atomicity, as rl_set's applying pass and a routed forget document.
 * The call does not move the step clock, cannot return RL_ELATE, does not touch the hot sets and
 * leaves rl_router_stats alone. Its value staging and two value buffers are allocated at the first
 * call, beside the routed peek's buffers. An engine's max_batch_desc bounds what one owner can
 * receive in one call (RL_ECAPACITY from its plan).
 * Out of scope: a set while steps are in flight, a device-memory form of the router call. */
int rl_set_routed_plan(rl_engine* e, const void* d_records, const rl_peek_reply* d_values, uint32_t n,
                       rl_peek_reply* d_reply_or_null);
int rl_set_routed_commit(rl_engine* e, int apply);
int rl_router_set(rl_router* r, const rl_batch* host_batches, const rl_peek_reply* const* values,
                  rl_peek_reply* const* out_or_null);

/* ---- Routed adjust -----------------------------------------------------------
 * rl_adjust where the keys are spread over the shards of a router. In a routed deployment an engine
 * holds only the keys it owns, and the rank that learns that a request failed downstream is in
 * general not the owner of that request's keys: this is the call that gives a charge back there.
 * A routed forget or set is idempotent; an adjust is not (a refund applied twice is a double
 * refund), and an owner can refuse after the records have moved (its max_batch_desc below what it
 * received, a restore or plan open, a batch in flight). So the call is all owners or none, two-phase
 * like rl_router_set. The plan is k_adjust_index's record form, which writes nothing to the table;
 * the commit is k_adjust_apply, which does all the writing.
 *
 * Engine level (device memory):
 * rl_route_pack_adjust: the origin's second pack step, behind rl_route_pack_strided of the same
 * batch (d_perm and d_send as that call wrote them, no combining). For every descriptor i with
 * d_perm[i] != RL_ROUTE_LOCAL the record d_send[d_perm[i]] gets h = (uint32_t)d_delta[i] and
 * rule = rule_id[i] | (flags & RL_ADJUST_KEEP_CACHE) << 16 (rule ids are below 0xFFFF, the routed
 * record's rule). Both are whole 32-bit stores computed from the batch; the record is not read and
 * nothing else of the send buffer is touched. Ordered on the engine stream, returns at once. Reads
 * n_desc and rule_id of the batch. RL_EINVAL for a null array with n_desc > 0 or a flag bit other
 * than RL_ADJUST_KEEP_CACHE. With this the records alone carry the call: there is no second value
 * exchange as a set has. A routed refund ("Routed refund" below) passes its uint32 amounts as the
 * delta words and RL_REFUND_KEEP_CACHE (the same bit) as the flag: the word's 32 bits are stored
 * whole, so the refund needs no pack kernel of its own.
 * rl_adjust_routed_plan: phase 1 over n such records. Identity and lookup are rl_peek_routed's (the
 * record's prefix lanes, time and rule), then rl_adjust's own index step: a found record adds
 * (int32_t)h, its rule's limit and one to its (string, store) pair's entry of the call's scratch
 * index, and the entry collects "some found record of this pair came without KEEP_CACHE". Replies
 * (rl_peek's, the state before the call, for every duplicate) go to d_reply when it is not NULL.
 * A record is malformed when its rule id is not below the loaded rule count, its time is above
 * 0xFFFD0000 or bits 17..31 of its rule word are not 0: it gets RL_PEEK_BAD and is never indexed.
 * The call synchronises the engine stream. 0: a plan is open and nothing has been written. Any
 * other return: nothing written and no plan open:
 *   RL_ESTATE     a batch in flight, a restore open, or a set or adjust plan open
 *   RL_ECAPACITY  n above max_batch_desc, or max_batch_desc above 2^29
 *   RL_EINVAL     null records with n > 0; a malformed record (found on the device: the owner's
 *                 host never sees the records)
 *   RL_EDEVICE    the scratch index had no entry left (unreachable, as in rl_adjust)
 *   RL_EHIP
 * n == 0 opens an empty plan. The plan lives in rl_set's scratch, as rl_adjust's index does. While
 * an adjust plan is open everything an open routed-set plan refuses returns RL_ESTATE, and so does
 * the commit of the other kind (rl_set_routed_commit on an adjust plan, rl_adjust_routed_commit on a
 * set plan: the plan stays open); rl_reset and rl_destroy close the plan.
 * rl_adjust_routed_commit: phase 2. apply == 0 drops the plan. Otherwise rl_adjust's applying pass
 * runs over the index: new = clamp(count + net, 0, 0xFFFFFFFF) once per pair; a pair's cache part
 * runs when the local cache is on, net < 0, new <= the pair's smallest limit and at least one of the
 * pair's found records came without KEEP_CACHE — with one flag on every record, rl_adjust's rule
 * word for word. *report is filled as rl_adjust fills it, with descriptors = n, nil = 0 and
 * descriptors == absent + applied (apply == 0 leaves it alone). RL_ESTATE with no adjust plan
 * open. Either way the plan is closed. RL_EHIP from the applying pass: the table may hold part of
 * the call, as rl_adjust documents.
 *
 * rl_router_adjust: rl_router_set's contract. Collective; one batch, one delta array, one flags
 * word, one output (or NULL) and one report (or NULL) per engine passed at create; the two pointer
 * arrays themselves may be NULL; host memory, synchronous; a rank with nothing to adjust passes
 * n_desc == 0; RL_ESTATE before any collective while a step is in flight.
 *   1. Origin: rl_router_peek's refusals, plus RL_EINVAL for a null delta array with n_desc > 0 or
 *      a flag bit other than RL_ADJUST_KEEP_CACHE. The deltas are staged (4 B x max_desc of pinned
 *      plus device memory, allocated at the first call), the batch is packed by owner (one record
 *      per descriptor) and the deltas and the keep bit are written into the records behind it. A
 *      refusal travels as this origin's status in the counts exchange: nothing is planned anywhere,
 *      the failing rank returns its code (local transport: the first failing shard's) and the
 *      others RL_EPEER.
 *   2. Counts, then records: one all-to-all-v. No values travel.
 *   3. Every owner runs rl_adjust_routed_plan over everything it received.
 *   4. Each owner's plan code goes to every rank. If any is non-zero every owner drops its plan:
 *      the failing rank returns its code and the others RL_EPEER (local transport: the first failing
 *      shard's code). No owner has written anything; out and the reports are untouched.
 *   5. Every owner commits; the replies and the commit status return by the reverse exchange and
 *      the origin unpacks them into out. A HIP or communicator failure in this phase leaves
 *      per-owner atomicity, as a routed set documents.
 * Semantics: the deltas of one (string, store) pair are summed over all descriptors of all origins
 * and applied once, clamped, so the result does not depend on the order of the origins: a counter
 * of 5 given -10 by origin 0 and +3 by origin 1 ends at 0. out[s][i] is the state before the call,
 * for every duplicate across descriptors and origins. *report[s] is what engine s did as an owner:
 * its commit's report over the records it received; summed over the ranks these are the call's
 * totals. Nil descriptors never leave their origin: an origin counts them from its replies
 * (RL_PEEK_NIL), and it learns whether its own corrections were applied from RL_PEEK_FOUND in out.
 * The call does not move the step clock, cannot return RL_ELATE, does not touch the hot sets and
 * leaves rl_router_stats alone. An engine's max_batch_desc bounds what one owner can receive in one
 * call (RL_ECAPACITY from its plan, so nobody applies).
 * Out of scope: an adjust while steps are in flight, a device-memory form of the router call, a
 * compact wire form, corrections to rule stats. */
int rl_route_pack_adjust(rl_engine* e, const rl_batch* device_batch, const uint32_t* d_perm, const int32_t* d_delta,
                         uint32_t flags, void* d_send);
int rl_adjust_routed_plan(rl_engine* e, const void* d_records, uint32_t n, rl_peek_reply* d_reply_or_null);
int rl_adjust_routed_commit(rl_engine* e, int apply, rl_adjust_report* report_or_null);
int rl_router_adjust(rl_router* r, const rl_batch* host_batches, const int32_t* const* delta,
                     const uint32_t* flags /* one per engine passed at create */,
                     rl_peek_reply* const* out_or_null, rl_adjust_report* const* report_or_null);

/* ---- Routed refund -----------------------------------------------------------
 * "Refund" above where the keys are spread over the shards of a router. The rank that sees a
 * request's verdict is in general not the owner of its keys, and rl_refund_behind refuses a routed
 * flight (its statuses are made at the origin, its counters live elsewhere). rl_router_adjust cannot
 * stand in: its deltas are int32, it looks up every descriptor, and the host would have to rebuild
 * the rule for which descriptors are owed from statuses it read back. Here that rule runs on the
 * origin's device, only the owed descriptors travel, and the amount is a full uint32 end to end.
 *
 * Engine level (device memory):
 * rl_refund_route_owed: the origin's pass over a device batch and its n_desc statuses. Ordered on
 * the engine stream, returns at once. Two kernels with the kernel boundary between them: the
 * refund's marking pass (an over-limit descriptor marks its request in the refund's own scratch,
 * 4 B x max_batch_req), then one lane per descriptor, streaming (no rule entry, no prefix byte and no
 * table slot is read): d_amount[i] = max(1, hits_addend[req_of[i]]) when descriptor i is owed, else
 * 0, where owed is rl_refund_pipelined's rule exactly (its request has a descriptor of code
 * RL_CODE_OVER_LIMIT, its rule is not RL_NIL_RULE, its status carries no RL_FLAG_LOCAL_CACHE_HIT);
 * d_rule_out[i] = rule_id[i] when owed, else RL_NIL_RULE (a descriptor whose request index is not
 * below n_req keeps its rule id, so that the pack behind refuses the batch). d_rule_out may be the
 * batch's own rule_id array: every lane reads its word before it writes it. d_counts[0] receives
 * the number of rejected requests and d_counts[1] the number of owed descriptors; both words are
 * zeroed on the stream by the call. rl_route_pack_strided of the batch with d_rule_out as its rule
 * array then leaves every unowed descriptor at home (perm[i] == RL_ROUTE_LOCAL): no record, no
 * lookup and no byte on the wire is spent on it. Behind that pack, rl_route_pack_adjust is passed
 * d_amount as its delta words (and the batch with d_rule_out as its rule array): it stores the
 * word's 32 bits whole into h and rule | keep << 16 beside it, so no pack kernel of the refund's own
 * exists. RL_EINVAL for a null array with n_desc > 0 (hits_addend is read) or null d_counts;
 * RL_ECAPACITY for n_desc / n_req over the engine's maxima; RL_ESTATE while a batch or flight is in
 * flight, a restore is open or a plan is open (the scratch is shared); all with nothing launched.
 * n_desc == 0 launches nothing and writes zeros to d_counts.
 * rl_refund_routed_plan: phase 1 over n such records; rl_adjust_routed_plan's lifecycle, return
 * codes and gates, word for word. Identity and lookup are rl_peek_routed's at the record's own time;
 * replies (the state before the call, for every duplicate; RL_PEEK_BAD and zeros for a malformed
 * record) go to d_reply when it is not NULL. Where the counter is found the amount is the record's h
 * as a full uint32: it never passes through an int32. The lanes of a wave that hold one (string,
 * store) pair combine before the atomics, as the refund flight's do: the 64-bit sum of the amounts,
 * the smallest limit, and the number of the pair's records that came without the keep bit. A record
 * is malformed as an adjust's is (rule id, time above 0xFFFD0000, a bit 17..31 of the rule word):
 * RL_EINVAL, nothing indexed. Nothing is written to the table. A refund plan is a third kind of
 * plan: rl_set_routed_commit or rl_adjust_routed_commit on it returns RL_ESTATE and leaves it open,
 * and rl_refund_routed_commit on a set or adjust plan likewise. n == 0 opens an empty plan. The call
 * synchronises the engine stream; the plan lives in rl_set's scratch.
 * rl_refund_routed_commit: phase 2. apply == 0 drops the plan. Otherwise rl_adjust's applying pass
 * runs in its per-key form: new = max(0, count - sum) once per pair, the expiry untouched; a pair
 * with new <= its smallest limit and a found record without the keep bit gets its local-cache
 * deadline cleared (when the local cache is on). *report holds the owner's fields: descriptors = n,
 * rejected_req = skipped = 0, absent, refunded, floored, unfrozen, with descriptors == absent +
 * refunded.
 *
 * rl_router_refund: rl_router_adjust's contract. Collective; one batch (hits_addend is read), one
 * status array (n_desc statuses, as the step returned them), one flags word, and one amount array,
 * output and report (each or NULL, and the three pointer arrays themselves may be NULL) per engine
 * passed at create; host memory, synchronous; a rank with nothing to refund passes n_desc == 0;
 * RL_ESTATE before any collective while a step is in flight; all owners or none.
 *   1. Origin: rl_router_peek's refusals, plus RL_EINVAL for a null status array or null hits_addend
 *      with n_desc > 0 or a flag bit other than RL_REFUND_KEEP_CACHE; each travels as this origin's
 *      status in the counts exchange. The batch (hits_addend really staged this time) and the
 *      statuses are staged (20 B x max_desc of pinned plus device memory, and the origin pass's
 *      scratch and amounts, allocated at the first call); the origin runs the two kernels of
 *      rl_refund_route_owed, the plain pack with the rewritten rules, and the amount and keep pack.
 *   2. Counts, then records: one all-to-all-v. No values travel.
 *   3. Every owner runs rl_refund_routed_plan over everything it received. The plan codes go to
 *      every rank; any non-zero code makes every owner drop its plan: the failing rank returns its
 *      code and the others RL_EPEER (local transport: the first failing shard's code). Nothing is
 *      written anywhere and every output is untouched.
 *   4. Every owner commits; the replies and the commit status return by the reverse exchange and
 *      the origin unpacks them (rl_route_unpack_peek).
 * Semantics: the amounts of one (string, store) pair are summed over all owed descriptors of all
 * origins in 64 bits and applied once, floored at 0: a counter of 9 owed 6 by origin 0 and 6 by
 * origin 1 ends at 0, floored once, in any order. amount[s][i] is what descriptor i was owed, 0
 * when skipped. out[s][i] is the state before the call for an owed descriptor and {0, 0, 0,
 * RL_PEEK_NIL} for any other: it was not asked. *report[s] holds engine s's origin fields
 * (descriptors, rejected_req, skipped: of the batch it passed) and its owner fields (absent,
 * refunded, floored, unfrozen: of the records it received). The lone engine's identity
 * descriptors == skipped + absent + refunded therefore does not hold per report; over the world,
 * the sum of descriptors - skipped equals the sum of absent + refunded.
 * The step clock, RL_ELATE, the hot sets and rl_router_stats do not move; rule stats, cache stats
 * and occupancy are untouched as for an adjust; the refunded step's statuses are not rewritten.
 * Out of scope: a refund while steps are in flight, a device-memory form of the router call, a
 * compact wire form. */
int rl_refund_route_owed(rl_engine* e, const rl_batch* device_batch, const rl_status* d_status, uint32_t* d_rule_out,
                         uint32_t* d_amount, uint32_t* d_counts /* [2] */);
int rl_refund_routed_plan(rl_engine* e, const void* d_records, uint32_t n, rl_peek_reply* d_reply_or_null);
int rl_refund_routed_commit(rl_engine* e, int apply, rl_refund_report* report_or_null);
int rl_router_refund(rl_router* r, const rl_batch* host_batches, const rl_status* const* status,
                     const uint32_t* flags /* one per engine passed at create */, uint32_t* const* amount_or_null,
                     rl_peek_reply* const* out_or_null, rl_refund_report* const* report_or_null);

/* ---- Rule stats: per-rule stat counters summed on the device ---------------
 * The reference keeps four counters per limit, <FullKey>.total_hits / .over_limit / .near_limit /
 * .over_limit_with_local_cache (src/config/config_impl.go:64-70), and BaseRateLimiter adds to
 * them for every descriptor (base_limiter.go:49-51, 77-78, 129-177). An rl_status carries the
 * increments and a host that reads the statuses adds them up itself; on the device path
 * (rl_resolve_device -> rl_submit_pipelined) the host reads no status, so the engine keeps one
 * rl_rule_stat row per rule id in device memory and a kernel adds a batch's increments to it.
 *
 * Contribution of descriptor i, with r = rule_id[i]: nothing for RL_NIL_RULE; otherwise
 * total_hits[r] += max(1, hits_addend[req_of[i]]), and when its status has RL_FLAG_HAS_LIMIT the
 * other four words as annotated below. Sums are 64-bit and wrap. A rule id at or above the loaded
 * rule count, or a request index at or above n_req, adds nothing and indexes nothing (only the
 * explicit call can meet either: a submit refuses such a batch).
 *
 * rl_rule_stats_add_device folds the statuses d_out[n_desc] of one device batch into the rows.
 * It reads rule_id, req_of, hits_addend, n_desc and n_req of the rl_batch (the other arrays may
 * be NULL; n_desc <= 2^30), is ordered on the engine stream, returns at once and is legal at any
 * time, batches in flight included. The caller leaves the arrays alone until work it orders
 * behind it on rl_stream(e) has run, or until the next rl_rule_stats_read. A routed origin calls
 * it on the statuses rl_route_unpack left in device memory.
 *
 * RL_CFG_RULE_STATS makes it automatic: every batch completed through rl_submit,
 * rl_submit_device or rl_submit_pipelined is folded in exactly once, from its final statuses —
 * also a batch the device handed to the LSD pipeline, re-sorted, or refused behind a refused one
 * and ran again. A batch whose rl_wait returns an error counts nothing. (The reference differs
 * there: it adds TotalHits before the Redis call, base_limiter.go:49-51, so it counts the hits of
 * a request whose Redis call then fails.) The raw forms (rl_submit_c, RL_ROUTED_RAW) and
 * rl_submit_routed are not counted at the owner: their decisions are made, or reported, elsewhere.
 * With the flag set a device batch completes on an event behind the counting kernel, so its
 * arrays are the caller's again when rl_wait returns, as without the flag.
 *
 * rl_rule_stats_read synchronises the engine stream and copies rows [first_rule, first_rule + n)
 * to host memory; with RL_RULE_STATS_CLEAR it zeroes those rows afterwards. RL_ESTATE while a
 * batch is in flight or a restore is open (the rl_peek rule); RL_EINVAL when the range passes the
 * loaded rule count.
 *
 * The rows are allocated at first use beside the rule table, one per rule id the table has room
 * for, and keep their contents when rl_load_rules grows it; rules appended while batches are in
 * flight need nothing new and start at 0. The counters are the service's, not the backend's
 * state: rl_reset, restore and rl_resize leave them alone, only RL_RULE_STATS_CLEAR zeroes them.
 * Rows are per rule id, so a caller that replaces rules (an id changes its meaning) reads and
 * clears first. Out of scope: HipRateLimitCache (its ids name (limit, unit, shadow), not a stats
 * key, and it walks every status on the host anyway) and counting inside rl_router_step.
 * (freecache's gauges have their own section, "Local-cache gauges" below.) */
typedef struct rl_rule_stat {     /* 64 B, one per rule id */
  uint64_t total_hits;                  /* += max(1, hits_addend) per descriptor of the rule */
  uint64_t over_limit;                  /* += over_limit_delta */
  uint64_t near_limit;                  /* += near_limit_delta */
  uint64_t over_limit_with_local_cache; /* += over_limit_delta when RL_FLAG_LOCAL_CACHE_HIT */
  uint64_t shadow_mode;                 /* += 1 when RL_FLAG_SHADOW (the current, parity-unpinned definition) */
  uint64_t reserved[3];                 /* 0 */
} rl_rule_stat;
enum { RL_RULE_STATS_CLEAR = 1u };
int rl_rule_stats_add_device(rl_engine* e, const rl_batch* device_batch, const rl_status* d_out);
int rl_rule_stats_read(rl_engine* e, uint32_t first_rule, uint32_t n, rl_rule_stat* out, uint32_t flags);

/* ---- Local-cache gauges and the table census --------------------------------
 * The reference publishes eight ratelimit.localcache.* gauges from freecache
 * (src/limiter/local_cache_stats.go:20-43). The device's local over-limit cache is the frz word
 * of a key string's table slot, so its gauges come from two places: lookup counters a kernel adds
 * to behind each batch (hitCount, missCount, lookupCount), and a census of the table (entryCount,
 * expiredCount). evacuateCount, overwriteCount and averageAccessTime are 0: the device cache
 * never evicts (parity unpinned there).
 *
 * Lookup counters. The reference makes one freecache Get per descriptor with a limit
 * (fixed_cache_impl.go:55-66). Contribution of descriptor i: nothing when rule_id[i] is
 * RL_NIL_RULE or at or above the loaded rule count; otherwise lookups += 1, and hits += 1 when
 * its status carries RL_FLAG_LOCAL_CACHE_HIT. misses = lookups - hits, computed at the read.
 * With rl_config.local_cache == 0 nothing is counted and nothing is launched (the reference
 * makes no Get with a nil cache), and the read returns zeros.
 *
 * rl_cache_stats_add_device folds the statuses d_out[n_desc] of one device batch in. It reads
 * n_desc, rule_id and the statuses' code_flags (the other arrays may be NULL; n_desc <= 2^30), is
 * ordered on the engine stream, returns at once and is legal with batches in flight. A routed
 * origin calls it on the statuses rl_route_unpack left in device memory.
 * RL_CFG_CACHE_STATS makes it automatic under RL_CFG_RULE_STATS' rules, word for word: every
 * batch completed through rl_submit, rl_submit_device or rl_submit_pipelined is folded in exactly
 * once from its final statuses, reruns and LSD fallbacks included; a batch whose rl_wait returns
 * an error adds nothing; the raw forms and rl_submit_routed are not counted at the owner. With
 * both flags set both kernels run and the batch completes behind the last.
 * rl_cache_stats_read synchronises the engine stream and copies the counters out; with
 * RL_CACHE_STATS_CLEAR it zeroes them afterwards. RL_ESTATE while a batch is in flight or a
 * restore is open. rl_reset, restore and rl_resize leave the counters alone.
 *
 * rl_census: one read-only streaming pass over the counter table, evaluated per slot with the
 * predicates rl_peek applies per key, at the time `now`. It writes nothing to the table, the
 * occupancy, the hot set or any stat. live[] / prev[] are exact and equal what an
 * rl_snapshot_begin at the same moment puts in its header ("What is live" above); the occupancy
 * of rl_get_occupancy may over-count. RL_ESTATE while a batch is in flight or a restore is open
 * (the rl_peek rule); an open snapshot does not block it. RL_EINVAL for now outside
 * [0, 0xFFFD0000] or a wrong struct_size. Legal on a router's engine between steps: each rank
 * reports its shard.
 * One limit: the census counts slots. For a `now` older than the table's newest request time, or
 * with EXPIRE jitter, Redis may still hold keys whose slots are no longer live (their window
 * generation was superseded); those are not counted. */
typedef struct rl_cache_stats {  /* 64 B */
  uint64_t hits;        /* ratelimit.localcache.hitCount */
  uint64_t misses;      /* ratelimit.localcache.missCount = lookups - hits */
  uint64_t lookups;     /* ratelimit.localcache.lookupCount */
  uint64_t reserved[5]; /* 0 */
} rl_cache_stats;
enum { RL_CACHE_STATS_CLEAR = 1u };
int rl_cache_stats_add_device(rl_engine* e, const rl_batch* device_batch, const rl_status* d_out);
int rl_cache_stats_read(rl_engine* e, rl_cache_stats* out, uint32_t flags);

#define RL_CENSUS_LOG2_BINS 33
typedef struct rl_census_report {       /* 832 B; per region r = (home unit - 1) * 2 + window parity */
  uint32_t struct_size;                 /* in: = sizeof(rl_census_report) */
  uint32_t reserved0;                   /* 0 */
  uint64_t slots[8];                    /* the region's size */
  uint64_t live[8];                     /* slots of the region's newest window generation */
  uint64_t prev[8];                     /* slots of generation gen - 2 (lag regions; else 0) */
  uint64_t stale[8];                    /* claimed slots (generation != 0) that are not live: reusable */
  uint64_t keys_main[8];                /* live-or-prev slots with now < expiry: what GET on the main store finds */
  uint64_t keys_per_second[8];          /* live-or-prev slots with a non-zero per-second counter */
  uint64_t cached[8];                   /* local_cache on: live-or-prev slots with now < the local-cache
                                           deadline (entryCount: what a lookup at `now` would hit); else 0 */
  uint64_t cache_expired[8];            /* local_cache on: the same slots with 0 < deadline <= now */
  uint64_t count_log2[RL_CENSUS_LOG2_BINS]; /* over the slots counted in keys_main: bit length of the counter */
  uint64_t reserved[6];                 /* 0 */
} rl_census_report;
int rl_census(rl_engine* e, int64_t now, rl_census_report* out);

/* ---- Descriptor-tree resolution (GetLimit) ------------------------
 * Replaces rateLimitConfigImpl.GetLimit (src/config/config_impl.go:274-323) per descriptor,
 * batched on the device: it yields the rule id each descriptor of an rl_batch carries.
 * The tree is the loaded YAML config (loadDescriptors, config_impl.go:115-165) flattened:
 * node i has a parent (a node before it, or RL_TREE_ROOT for a domain), its map key in
 * `names` (the domain name, or finalKey = key["_" value], config_impl.go:126-129) and the
 * rule id of its limit (RL_NIL_RULE = no rate_limit). Stats keys (FullKey) stay on the host. */
#define RL_TREE_ROOT 0xFFFFFFFFu
typedef struct rl_tree_node {
  uint32_t parent;
  uint32_t name_off;
  uint32_t name_len;
  uint32_t rule;
} rl_tree_node;

/* Replace the tree. RL_EINVAL on a forward parent, an empty key, or a duplicate (parent,
 * name) — the reference's "duplicate descriptor composite key" / "duplicate domain" panics.
 * Not while a batch is in flight. */
int rl_load_tree(rl_engine* e, const rl_tree_node* nodes, uint32_t n_nodes, const uint8_t* names,
                 uint32_t names_len);

/* One resolution batch. Strings are (offset, length) ranges of `bytes`. override_rule (may
 * be NULL) holds, per descriptor, the rule id the host registered for descriptor.Limit
 * (config_impl.go:286-296; RL_NIL_RULE = no override): it applies when the domain exists. */
typedef struct rl_resolve_batch {
  uint32_t n_desc;
  uint32_t n_entries;
  uint32_t bytes_len;
  uint32_t reserved;            /* 0 */
  const uint8_t* bytes;
  const uint32_t* domain;       /* [2 n_desc]: domain (off, len) per descriptor */
  const uint32_t* entry_first;  /* [n_desc + 1]: entries of descriptor i are [entry_first[i], entry_first[i+1]) */
  const uint32_t* entry;        /* [4 n_entries]: key off, key len, value off, value len */
  const uint32_t* override_rule;
} rl_resolve_batch;

/* Host memory in and out; synchronous. rule_out[n_desc]. */
int rl_resolve(rl_engine* e, const rl_resolve_batch* batch, uint32_t* rule_out);
/* Device memory in and out, asynchronous: ordered before the engine's next submit (run on the
 * stream that submit's first kernel uses, so with batches in flight it runs beside their
 * decisions, as the next batch's fingerprint pass does). It is NOT ordered after batches
 * already in flight: d_rule_out must not be the rule_id array of a batch still in flight
 * (give each batch in flight its own, as rl_batch inputs are). Two kernels: a level-pipelined
 * walk, then the exact walk for the descriptors it leaves (rl_resolve.hip). */
int rl_resolve_device(rl_engine* e, const rl_resolve_batch* device_batch, uint32_t* d_rule_out);

#ifdef __cplusplus
}
#endif
#endif /* RL_HIP_H */
