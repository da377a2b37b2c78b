// rl_peek.hip — read and clear counters by key (rl_hip.h "Peek / forget").
//   k_peek<false>  one lane per descriptor: the state a submit of the same descriptor would read
//                  before its INCRBY (Redis GET + TTL, freecache Get), as an rl_peek_reply
//   k_peek<true>   the same lookup, then DEL on the descriptor's store and the string's
//                  local-cache entry, as separate 32-bit stores; writes no reply
// rl_forget runs the first and then the second: every duplicate of a call reports the state
// before the call, and two descriptors that clear the two stores of one string lose nothing.
#include <hip/hip_runtime.h>

#include "rl_peek.h"

namespace rlhip {
namespace peek {

// The first two load levels are rl_peek.h's desc_front, the third and everything behind it its
// peek_key. No LDS, no lane waits for another; the loops are bounded by the prefix length (hash)
// and the region size (probe).
template <bool FORGET>
__global__ __launch_bounds__(NT) void k_peek(const DevBatch in, const DevRule* __restrict__ rules, const uint32_t n_rules,
                                             const uint64_t seed, const TableDesc tab, rl_peek_reply* __restrict__ out) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= in.n_desc) return;
  const DescFront f = desc_front(in, rules, n_rules, i);
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = f.nil ? RL_PEEK_NIL : RL_PEEK_BAD;
  if (f.ok) {
    const FpState s = prefix_state_pre(f.w0, f.w1, in.blob, f.o0, f.len, seed);
    rep = peek_key<FORGET>(s, f.now, f.rr, tab, rep);
  }
  if (!FORGET) out[i] = rep;
}

}  // namespace peek

void launch_peek(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                 const TableDesc& tab, rl_peek_reply* out, bool forget) {
  if (!b.n_desc) return;
  const DevBatch in = make_dev_batch(b);
  const uint32_t grid = (b.n_desc + peek::NT - 1u) / peek::NT;
  if (forget)
    hipLaunchKernelGGL(peek::k_peek<true>, dim3(grid), dim3(peek::NT), 0, st, in, rules, n_rules, seed, tab, out);
  else
    hipLaunchKernelGGL(peek::k_peek<false>, dim3(grid), dim3(peek::NT), 0, st, in, rules, n_rules, seed, tab, out);
}

}  // namespace rlhip
