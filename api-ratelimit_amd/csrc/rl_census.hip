// rl_census.hip — the two counting kernels behind the local-cache gauges (rl_hip.h "Local-cache
// gauges and the table census").
//   k_census       one read-only streaming pass over the counter table: per (region, field)
//                  counts and a histogram of the live counters' bit lengths
//   k_cache_stats  one streaming pass over a batch's rule ids and status words: local-cache
//                  lookups and hits
// Neither writes the table; no block waits for another and nothing spins.
#include <hip/hip_runtime.h>

#include "rl_census.h"
#include "rl_device.h"

namespace rlhip {
namespace census {

constexpr int NT = 1024;                 // threads per block (16 waves), k_snap_export's shape
constexpr int PER = 4;                   // slots per lane and tile
constexpr int TILE = NT * PER;           // 4096 consecutive slots
static_assert(CENSUS_WORDS <= NT, "one lane per count word at the flush");

// Census. A block takes tiles of TILE consecutive slots (grid-stride): every lane reads PER
// slots (two 16-B loads each, all eight issued before the first use) and classifies them with
// the predicates peek_key applies to a found slot (rl_peek.h). A wave's 64 slots of one pass are
// consecutive, so they lie in one region unless a region is smaller than a wave: the wave sums
// each field by ballot/popcount per region present (a loop of at most 8 rounds) and lanes 0..6
// add the sums to the tile's LDS words; the histogram takes one LDS add per counted lane. After
// the tile every non-zero LDS word takes ONE 64-bit global add, each word on a 256-B line of its
// own (CensusCtl). Every loop is bounded by the slot count.
__global__ __launch_bounds__(NT) void k_census(const TableDesc tab, const uint64_t n_slots, const SnapGens gens,
                                                const uint32_t now, CensusCtl* ctl) {
  __shared__ uint32_t sh[CENSUS_WORDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t n_tiles = (n_slots + TILE - 1) / TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (tid < (uint32_t)CENSUS_WORDS) sh[tid] = 0u;
    __syncthreads();
    const uint64_t i0 = tile * TILE + tid;
    uint4 a[PER], b[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      a[k] = make_uint4(0u, 0u, 0u, 0u);
      b[k] = a[k];
      if (i < n_slots) {
        const uint4* p = reinterpret_cast<const uint4*>(tab.slots + i);
        a[k] = p[0];
        b[k] = p[1];
      }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      const bool in = i < n_slots;
      const uint32_t r = snap::region_of_slot(tab, i);
      const uint32_t g = a[k].x;  // the claim word's generation; b = count, exp, pcount, frz
      const uint32_t c = in ? snap::gen_class(g, snap::gen_of_region(gens, r), lazy_region(tab.lag, r)) : 2u;
      const bool lp = c < 2u;
      bool f[CENSUS_FIELDS];
      f[CF_LIVE] = c == 0u;
      f[CF_PREV] = c == 1u;
      f[CF_STALE] = in && g != 0u && c == 2u;
      f[CF_MAIN] = lp && now < b[k].y;
      f[CF_PS] = lp && b[k].z != 0u;
      f[CF_CACHED] = lp && tab.local_cache && now < b[k].w;
      f[CF_EXPIRED] = lp && tab.local_cache && b[k].w != 0u && b[k].w <= now;
      // per region present in the wave (claimed slots only: a never-claimed one counts nowhere)
      uint64_t rem = __ballot(in && g != 0u);
      while (rem) {  // at most 8 rounds: every round removes one region's lanes
        const uint32_t r0 = __shfl(r, __ffsll((unsigned long long)rem) - 1);
        const uint64_t m = rem & __ballot(r == r0);
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < CENSUS_FIELDS; ++q) {
          const uint32_t n = (uint32_t)__popcll(m & __ballot(f[q]));
          mine = lane == (uint32_t)q ? n : mine;
        }
        if (lane < (uint32_t)CENSUS_FIELDS && mine) atomicAdd(&sh[r0 * CENSUS_FIELDS + lane], mine);
        rem &= ~m;
      }
      // bit length of the main store's counter, 0..32 (__clz(0) = 32): one LDS add per counted lane,
      // nothing returned and nothing waited for (a ballot loop per length present measured slower,
      // DESIGN.md §6)
      if (f[CF_MAIN]) atomicAdd(&sh[CENSUS_HIST0 + 32u - (uint32_t)__clz(b[k].x)], 1u);
    }
    __syncthreads();
    if (tid < (uint32_t)CENSUS_WORDS && sh[tid]) atomicAdd(&ctl->w[tid][0], (unsigned long long)sh[tid]);
    __syncthreads();  // sh is cleared by the next tile
  }
}

}  // namespace census

namespace cstat {

constexpr int NT = 512;
constexpr int U = 4;  // descriptors per thread and pass: their loads go out together
constexpr int NW = NT / 64;

// Lookup counters of one batch (fixed_cache_impl.go:55-66: one freecache Get per descriptor with
// a limit). Reads rule_id and the statuses' first word only. A few persistent blocks stride over
// the batch; every wave keeps its two sums as wave-uniform popcounts of ballots, the block adds
// them up in LDS and issues one global add per non-zero counter, each counter on a 256-B line of
// its own. ctl: as in k_rule_stats, the batch's control block (automatic mode) or null; a batch
// with a non-zero error word there is not counted.
__global__ __launch_bounds__(NT) void k_cache_stats(const uint32_t n_desc, const uint32_t* __restrict__ rule,
                                                     const rl_status* __restrict__ st, const uint32_t n_rules,
                                                     CacheStatCtl* __restrict__ acc, const EngineCtl* __restrict__ ctl) {
  __shared__ uint32_t s_sum[2][NW];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  if (ctl && __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // kernel-uniform
  uint32_t looks = 0, hits = 0;  // wave-uniform; below 2^30 (n_desc <= 2^30, host-checked)
  const uint32_t stride = gridDim.x * (uint32_t)(NT * U);  // at most 2^21: no index wraps
  for (uint32_t base = blockIdx.x * (uint32_t)(NT * U); base < n_desc; base += stride) {
    uint32_t r[U], cf[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = base + u * NT + tid;
      ok[u] = i < n_desc;
      const uint32_t ic = ok[u] ? i : 0u;  // clamped: n_desc >= 1 in a launched kernel
      r[u] = rule[ic];
      cf[u] = st[ic].code_flags;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // RL_NIL_RULE is never below n_rules: a nil limit and an unknown rule id add nothing
      const bool look = ok[u] && r[u] < n_rules;
      looks += (uint32_t)__popcll(__ballot(look));
      hits += (uint32_t)__popcll(__ballot(look && ((cf[u] >> 8) & RL_FLAG_LOCAL_CACHE_HIT)));
    }
  }
  if ((tid & 63u) == 0u) {
    s_sum[0][wave] = looks;
    s_sum[1][wave] = hits;
  }
  __syncthreads();
  if (tid < 2u) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += s_sum[tid][w];
    if (v) atomicAdd(&acc->w[tid][0], v);
  }
}

}  // namespace cstat

// One census of tab (n_slots slots) at `now` into ctl (zeroed by the caller, on the stream).
void launch_census(hipStream_t st, const TableDesc& tab, uint64_t n_slots, const SnapGens& gens, uint32_t now,
                   CensusCtl* ctl, uint32_t max_blocks) {
  const uint64_t tiles = (n_slots + census::TILE - 1) / census::TILE;
  uint32_t grid = (uint32_t)(tiles < 1024 ? (tiles ? tiles : 1) : 1024);
  if (grid > max_blocks) grid = max_blocks;
  hipLaunchKernelGGL(census::k_census, dim3(grid), dim3(census::NT), 0, st, tab, n_slots, gens, now, ctl);
}

// Folds one batch's statuses into acc. max_blocks: the persistent grid's bound. Launches nothing
// for an empty batch.
void launch_cache_stats(hipStream_t s, const rl_batch& b, const rl_status* out, uint32_t n_rules, CacheStatCtl* acc,
                        const EngineCtl* ctl, uint32_t max_blocks) {
  if (!b.n_desc || !n_rules) return;
  const uint32_t per = cstat::NT * cstat::U;
  uint32_t grid = (b.n_desc + per - 1u) / per;
  if (grid > max_blocks) grid = max_blocks;
  hipLaunchKernelGGL(cstat::k_cache_stats, dim3(grid), dim3(cstat::NT), 0, s, b.n_desc, b.rule_id, out, n_rules, acc,
                     ctl);
}

}  // namespace rlhip
