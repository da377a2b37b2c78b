// rl_census.h — what the engine (rl_engine.cpp) and the counting kernels of rl_census.hip share.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_common.h"
#include "rl_snapshot.h"

namespace rlhip {

// Per-region count words of a census, in rl_census_report's order from live[] on.
enum : int { CF_LIVE = 0, CF_PREV, CF_STALE, CF_MAIN, CF_PS, CF_CACHED, CF_EXPIRED, CENSUS_FIELDS };
constexpr int CENSUS_HIST0 = 8 * CENSUS_FIELDS;  // word region * CENSUS_FIELDS + field, then the histogram
constexpr int CENSUS_WORDS = CENSUS_HIST0 + RL_CENSUS_LOG2_BINS;

// Control block of one census, zeroed before it. As in SnapCtl / EngineCtl, every word that
// more than one block adds to lives on a 256-B line of its own.
struct CensusCtl {
  unsigned long long w[CENSUS_WORDS][32];
};
static_assert(sizeof(CensusCtl) == CENSUS_WORDS * 256, "CensusCtl layout");

// The lookup counters (rl_cache_stats): word 0 = lookups, 1 = hits, a line each.
struct CacheStatCtl {
  unsigned long long w[2][32];
};
static_assert(sizeof(CacheStatCtl) == 512, "CacheStatCtl layout");

void launch_census(hipStream_t st, const TableDesc& tab, uint64_t n_slots, const SnapGens& gens, uint32_t now,
                   CensusCtl* ctl, uint32_t max_blocks);
void launch_cache_stats(hipStream_t s, const rl_batch& b, const rl_status* out, uint32_t n_rules, CacheStatCtl* acc,
                        const EngineCtl* ctl, uint32_t max_blocks);

}  // namespace rlhip
