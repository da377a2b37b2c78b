// rl_peek_routed.hip — peek / forget where the keys are routed to their owners (rl_hip.h "Routed
// peek / forget").
//   k_peek_routed<false>  owner: one lane per routed record (RRec: prefix lanes, request time,
//                         rule id), the state a routed record of the same key would read before
//                         its INCRBY, as an rl_peek_reply
//   k_peek_routed<true>   the same lookup, then the clears of k_peek<true>; writes no reply
//   k_peek_unpack         origin: each descriptor's reply from its record's (perm), or NIL
#include <hip/hip_runtime.h>

#include "rl_peek.h"

namespace rlhip {
namespace peek {

// Three dependent levels, each one run of loads waited for once (latency-bound, random 32-B
// reads, like k_peek): rl_peek.h's rec_front (the record, then the rule entry), then the key's
// first table slot (peek_key). A record that is not ok gets RL_PEEK_BAD and zeros. No LDS, no lane
// waits for another; the one loop is the probe, bounded by the region size.
template <bool FORGET>
__global__ __launch_bounds__(NT) void k_peek_routed(const RRec* __restrict__ recs, const uint32_t n,
                                                    const DevRule* __restrict__ rules, const uint32_t n_rules,
                                                    const TableDesc tab, rl_peek_reply* __restrict__ out) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const RecFront f = rec_front(recs, rules, n_rules, i, true, false);
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = RL_PEEK_BAD;
  if (f.ok) rep = peek_key<FORGET>(FpState{f.rc.a, f.rc.b}, f.rc.now, f.rr, tab, rep);
  if (!FORGET) out[i] = rep;
}

// One lane per descriptor. perm: the strided form of the pack (owner * stride + position, an
// index into back), or RL_ROUTE_LOCAL for a descriptor without a limit.
__global__ __launch_bounds__(NT) void k_peek_unpack(const uint32_t n, const uint32_t* __restrict__ perm,
                                                    const rl_peek_reply* __restrict__ back,
                                                    rl_peek_reply* __restrict__ out) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i];
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = RL_PEEK_NIL;
  if (p != RL_ROUTE_LOCAL) rep = back[p];
  out[i] = rep;
}

}  // namespace peek

void launch_peek_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                        const TableDesc& tab, rl_peek_reply* out, bool forget) {
  if (!n) return;
  const uint32_t grid = (n + peek::NT - 1u) / peek::NT;
  if (forget)
    hipLaunchKernelGGL(peek::k_peek_routed<true>, dim3(grid), dim3(peek::NT), 0, st, recs, n, rules, n_rules, tab, out);
  else
    hipLaunchKernelGGL(peek::k_peek_routed<false>, dim3(grid), dim3(peek::NT), 0, st, recs, n, rules, n_rules, tab, out);
}

void launch_peek_unpack(hipStream_t st, uint32_t n, const uint32_t* perm, const rl_peek_reply* back,
                        rl_peek_reply* out) {
  if (!n) return;
  hipLaunchKernelGGL(peek::k_peek_unpack, dim3((n + peek::NT - 1u) / peek::NT), dim3(peek::NT), 0, st, n, perm, back,
                     out);
}

}  // namespace rlhip
