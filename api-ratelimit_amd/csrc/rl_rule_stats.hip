// rl_rule_stats.hip — per-rule stat counters summed on the device (rl_hip.h "Rule stats",
// DESIGN.md §4d).
//   k_rule_stats<true>   rule ids below RS_K summed per block in LDS (64-bit LDS adds), flushed
//                        with one global add per non-zero sum; ids from RS_K up go to global adds
//   k_rule_stats<false>  every sum goes to a global add (the A/B partner)
// One streaming pass over rule_id, req_of and the statuses plus a gather of hits_addend. Both
// forms first sum inside the wave when every counted lane of it carries one rule. A few
// persistent blocks stride over the batch, so a rule's row sees at most one add per block and
// counter from the flush. No block waits for another and nothing spins.
#include <hip/hip_runtime.h>

#include "rl_common.h"

namespace rlhip {
namespace rstat {

constexpr int NT = 512;
constexpr int U = 4;               // descriptors per thread and pass: their loads go out together
constexpr uint32_t RS_K = 1024;    // rule ids summed in LDS (RS_K * NC * 8 B = 40 KiB)
constexpr int NC = 5;              // counters per rule: rl_rule_stat's first five words
constexpr int ROW = sizeof(rl_rule_stat) / 8;
static_assert(sizeof(rl_rule_stat) == 64 && ROW == 8, "rl_rule_stat is eight 64-bit words");

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ctl: the batch's control block (automatic mode) or null. A batch the device refused, handed
// to the other pipeline or found malformed has a non-zero error word there once the kernels
// before this one on the stream are done: it is not counted (the rerun's launch counts it).
template <bool LDS>
__global__ __launch_bounds__(NT) void k_rule_stats(const uint32_t n_desc, const uint32_t n_req,
                                                   const uint32_t* __restrict__ rule, const uint32_t* __restrict__ req_of,
                                                   const uint32_t* __restrict__ hits, const rl_status* __restrict__ st,
                                                   const uint32_t n_rules, unsigned long long* __restrict__ tab,
                                                   const EngineCtl* __restrict__ ctl) {
  __shared__ unsigned long long s_acc[LDS ? NC * RS_K : 1];
  const uint32_t tid = threadIdx.x;
  if (ctl && __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // kernel-uniform
  const uint32_t kuse = n_rules < RS_K ? n_rules : RS_K;  // rows of s_acc in use (n_rules >= 1)
  const uint32_t n_acc = LDS ? NC * kuse : 0u;
  for (uint32_t e = tid; e < n_acc; e += NT) s_acc[(e / kuse) * RS_K + e % kuse] = 0ull;
  __syncthreads();

  auto add = [&](uint32_t r, int c, unsigned long long v) {
    if (LDS && r < RS_K) atomicAdd(&s_acc[c * RS_K + r], v);
    else atomicAdd(&tab[(size_t)r * ROW + c], v);
  };

  // n_desc <= 2^30 (host-checked) and the grid's stride is at most 2^21: no index wraps
  const uint32_t stride = gridDim.x * (uint32_t)(NT * U);
  for (uint32_t base = blockIdx.x * (uint32_t)(NT * U); base < n_desc; base += stride) {
    // two dependent levels of loads, each issued together: (rule id, request index, the status
    // words: none depends on another), then the gather of hits_addend
    uint32_t r[U], q[U], cf[U], ov[U], nr[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = base + u * NT + tid;
      ok[u] = i < n_desc;
      const uint32_t ic = ok[u] ? i : 0u;  // clamped: n_desc >= 1 in a launched kernel
      r[u] = rule[ic];
      q[u] = req_of[ic];
      cf[u] = st[ic].code_flags;
      ov[u] = st[ic].over_limit_delta;
      nr[u] = st[ic].near_limit_delta;
    }
    uint32_t h[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // RL_NIL_RULE is never below n_rules: a nil limit, an unknown rule id and a request index
      // past n_req add nothing and index nothing
      ok[u] = ok[u] && r[u] < n_rules && q[u] < n_req;
      h[u] = ok[u] ? hits[q[u]] : 0u;  // (n_req may be 0: then nothing is read)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned long long m = __ballot(ok[u]);
      if (!m) continue;  // wave-uniform
      const uint32_t fl = cf[u] >> 8;
      const bool lim = ok[u] && (fl & RL_FLAG_HAS_LIMIT);
      unsigned long long v[NC];
      v[0] = ok[u] ? (h[u] > 1u ? h[u] : 1u) : 0u;
      v[1] = lim ? ov[u] : 0u;
      v[2] = lim ? nr[u] : 0u;
      v[3] = (lim && (fl & RL_FLAG_LOCAL_CACHE_HIT)) ? ov[u] : 0u;
      v[4] = (lim && (fl & RL_FLAG_SHADOW)) ? 1u : 0u;
      // the rule of the wave's first counted lane; one rule in the whole wave: sum in the wave
      const uint32_t r0 = __shfl(r[u], __ffsll((long long)m) - 1);
      if (__ballot(ok[u] && r[u] == r0) == m) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (!__ballot(v[c] != 0ull)) continue;  // wave-uniform
          const unsigned long long s = wave_sum(v[c]);
          if ((tid & 63u) == 0u) add(r0, c, s);
        }
      } else if (ok[u]) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (v[c]) add(r[u], c, v[c]);
      }
    }
  }
  if (!LDS) return;
  __syncthreads();
  for (uint32_t e = tid; e < n_acc; e += NT) {
    const uint32_t c = e / kuse, rr = e % kuse;
    const unsigned long long v = s_acc[c * RS_K + rr];
    if (v) atomicAdd(&tab[(size_t)rr * ROW + c], v);
  }
}

}  // namespace rstat

// Folds one batch's statuses into tab[n_rules] (rl_rule_stat rows). variant 0: LDS form, 1: global
// adds only; max_blocks: the persistent grid's bound. Launches nothing for an empty batch.
void launch_rule_stats(hipStream_t s, const rl_batch& b, const rl_status* out, uint32_t n_rules, rl_rule_stat* tab,
                       const EngineCtl* ctl, int variant, uint32_t max_blocks) {
  if (!b.n_desc || !n_rules) return;
  const uint32_t per = rstat::NT * rstat::U;
  uint32_t grid = (b.n_desc + per - 1u) / per;
  if (grid > max_blocks) grid = max_blocks;
  unsigned long long* t = reinterpret_cast<unsigned long long*>(tab);
  if (variant == 1)
    hipLaunchKernelGGL(rstat::k_rule_stats<false>, dim3(grid), dim3(rstat::NT), 0, s, b.n_desc, b.n_req, b.rule_id,
                       b.req_of, b.hits_addend, out, n_rules, t, ctl);
  else
    hipLaunchKernelGGL(rstat::k_rule_stats<true>, dim3(grid), dim3(rstat::NT), 0, s, b.n_desc, b.n_req, b.rule_id,
                       b.req_of, b.hits_addend, out, n_rules, t, ctl);
}

}  // namespace rlhip
