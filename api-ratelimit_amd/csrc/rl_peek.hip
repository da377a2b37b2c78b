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

// The loads of a lane go out in three dependent levels, each issued as one run and waited for
// once (the kernel is latency-bound: random 32-B reads): (offsets, rule id, request index),
// then (now, the rule entry, the prefix's first 32 bytes), then the key's first table slot.
// Every load of the first two levels is unconditional at a clamped index (rl_tile.h load_descs):
// clamped reads stay inside the arrays (n_desc >= 1 in a launched kernel, n_req >= 1 and a rule
// table allocation exist, both host-checked) and inside the blob's RL_BLOB_SLACK readable bytes.
// No LDS, no lane waits for another; the loops are bounded by the prefix length (hash) and the
// region size (probe). The third level and everything behind it is rl_peek.h's peek_key.
template <bool FORGET>
__global__ __launch_bounds__(NT) void k_peek(const DevBatch in, const DevRule* __restrict__ rules, const uint32_t n_rules,
                                             const uint64_t seed, const TableDesc tab, rl_peek_reply* __restrict__ out) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= in.n_desc) return;
  const uint32_t rl = in.rule[i];
  const uint32_t q = in.req_of[i];
  const uint32_t qp = in.req_of[i ? i - 1u : 0u];
  const uint32_t oa = in.off[i];
  const uint32_t ob = in.off[i + 1u];

  const bool nil = rl == RL_NIL_RULE;
  const bool rule_ok = rl < n_rules, q_ok = q < in.n_req;
  const bool lay = oa <= ob && ob <= in.blob_bytes && qp <= q;
  bool ok = !nil && rule_ok && q_ok && lay;
  const uint32_t o0 = ok ? oa : 0u, len = ok ? ob - oa : 0u;
  const int64_t now = in.now[q_ok ? q : 0u];
  const DevRule rr = rules[rule_ok ? rl : 0u];  // never indexed with a bad id
  const u32x4* p = reinterpret_cast<const u32x4*>(in.blob + (o0 & ~3u));
  const u32x4 w0 = p[0];
  const u32x4 w1 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint32_t*>(p) + 4);

  ok = ok && now >= 0 && now <= MAX_NOW;
  // One use of the level's other loads beside the time check: without it the compiler sinks the
  // rule and prefix loads behind the branch on `ok`, where they wait a round trip of their own.
  asm volatile("" ::"v"(rr.unit), "v"(rr.div), "v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y),
               "v"(w1.z), "v"(w1.w));
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = nil ? RL_PEEK_NIL : RL_PEEK_BAD;
  if (ok) {
    const FpState s = prefix_state_pre(w0, w1, in.blob, o0, len, seed);
    rep = peek_key<FORGET>(s, (uint32_t)now, rr, tab, rep);
  }
  if (!FORGET) out[i] = rep;
}

}  // namespace peek

// out: n_desc replies (peek; unused by the forget launch). Launches nothing for an empty batch.
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
