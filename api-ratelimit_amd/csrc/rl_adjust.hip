// rl_adjust.hip — signed counter corrections by key (rl_hip.h "Adjust").
//   k_adjust_index  one lane per descriptor: k_peek's lookup (rl_peek.h peek_key_slot) and reply;
//                   a descriptor whose counter is found adds its delta, its rule's limit and one
//                   to its (slot, store) pair's entry of the call's scratch index
//   k_adjust_apply  one lane per index entry: count = clamp(count + net, 0, 2^32 - 1) as one 32-bit
//                   store, and the string's local-cache deadline cleared where the pair qualifies
// (adjust_key and block_add3 live in rl_adjust_key.h, shared with the record form of the first
// kernel, rl_adjust_routed.hip)
// The first kernel writes nothing to the table, so every reply is the state before the call; the
// second writes each counter word from exactly one lane, so the result depends on neither the
// descriptor order nor scheduling. Nothing is ever claimed. Kernel boundaries order the two: no
// lane waits for another lane or block, and every loop is bounded by the prefix length (hash), the
// region size (probe) or the index size (insert).
// FLIGHT: the forms an adjust in flight runs (rl_hip.h "Adjust in flight"), queued on the engine
// stream between decision batches. Both read the poison word first (k4_place sets it for a batch
// the engine will rerun, rl_kernels_v4.hip): behind such a batch they write nothing, neither table
// nor replies, leave the word as it is for the batch behind them and set ADJ_ERR_POISON, and the
// engine runs the adjust again behind the batch's rerun. The device form's descriptors come
// unchecked: a malformed one sets ADJ_ERR_BADREC, after which the applying pass writes nothing.
#include <hip/hip_runtime.h>

#include "rl_adjust.h"
#include "rl_adjust_key.h"
#include "rl_peek.h"

namespace rlhip {
namespace adjust {

// The loads go out as rl_peek.h's desc_front sends them, with the delta beside the first level.
// The front is written out here: through desc_front the kernel compiled to another load order and
// measured 1 % slower ("By-key refactor"). A thread past n_desc reads descriptor
// n_desc - 1 and uses nothing of it (`live`): it stays for the block's sums.
template <bool FLIGHT>
__global__ __launch_bounds__(NT) void k_adjust_index(const DevBatch in, const DevRule* __restrict__ rules,
                                                     const uint32_t n_rules, const uint64_t seed, const TableDesc tab,
                                                     const int32_t* __restrict__ delta, rl_peek_reply* __restrict__ out,
                                                     const AdjScratch sc, const uint32_t* __restrict__ poison) {
  const uint32_t gi = blockIdx.x * NT + threadIdx.x;
  if constexpr (FLIGHT) {
    if (*poison) {  // the same word for every thread: the whole grid leaves
      if (gi == 0u) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_POISON);
      return;
    }
  }
  const bool live = gi < in.n_desc;
  const uint32_t i = live ? gi : in.n_desc - 1u;  // n_desc >= 1 in a launched kernel
  const uint32_t rl = in.rule[i];
  const uint32_t q = in.req_of[i];
  const uint32_t qp = in.req_of[i ? i - 1u : 0u];
  const uint32_t oa = in.off[i];
  const uint32_t ob = in.off[i + 1u];
  const int32_t dl = delta[i];

  const bool nil = rl == RL_NIL_RULE;
  const bool rule_ok = rl < n_rules, q_ok = q < in.n_req;
  const bool lay = oa <= ob && ob <= in.blob_bytes && qp <= q;
  bool ok = live && !nil && rule_ok && q_ok && lay;
  const uint32_t o0 = ok ? oa : 0u, len = ok ? ob - oa : 0u;
  const int64_t now = in.now[q_ok ? q : 0u];
  const DevRule rr = rules[rule_ok ? rl : 0u];  // never indexed with a bad id
  const u32x4* p = reinterpret_cast<const u32x4*>(in.blob + (o0 & ~3u));
  const u32x4 w0 = p[0];
  const u32x4 w1 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint32_t*>(p) + 4);

  ok = ok && now >= 0 && now <= MAX_NOW;
  if constexpr (FLIGHT) {
    if (live && !nil && !ok) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_BADREC);
  }
  // (k_peek: keeps the level's loads in front of the branch on `ok`)
  asm volatile("" ::"v"(rr.unit), "v"(rr.div), "v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y),
               "v"(w1.z), "v"(w1.w));
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = nil ? RL_PEEK_NIL : RL_PEEK_BAD;  // the host refused a malformed descriptor before the launch
  bool applied = false;
  if (ok) {
    const FpState s = prefix_state_pre(w0, w1, in.blob, o0, len, seed);
    applied = adjust_key<false>(s, (uint32_t)now, rr, dl, false, tab, sc, rep);
  }
  if (live && out) out[i] = rep;
  block_add3(live && nil, live && !nil && !applied, applied, ADJ_NIL, ADJ_ABSENT, ADJ_APPLIED, sc.ctl);
}

// Entries are disjoint (one per (slot, store) pair), so a counter word is read and written by one
// lane: plain loads and stores. The local-cache word is shared by a string's two pairs: atomicExch,
// so that a deadline cleared by both counts once. After an index overflow nothing is written.
// PER_KEY (a routed plan's commit, rl_adjust_routed.hip): a pair's cache part also needs the
// entry's count, there "found records of the pair that came without RL_ADJUST_KEEP_CACHE", to be
// non-zero; the host form's flag is the call's, folded into clear_cache.
template <bool PER_KEY, bool FLIGHT>
__global__ __launch_bounds__(NT) void k_adjust_apply(const bool clear_cache, const AdjScratch sc,
                                                     const uint32_t* __restrict__ poison) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if constexpr (FLIGHT) {
    if (*poison) {
      if (i == 0u) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_POISON);
      return;
    }
  }
  bool floored = false, capped = false, unfrozen = false;
  if (i < (1u << sc.log2_entries) && !sc.ctl->w[ADJ_ERR][0]) {
    const uint4 a = reinterpret_cast<const uint4*>(sc.index + i)[0];
    const uint2 b = reinterpret_cast<const uint2*>(sc.index + i)[2];
    const bool release = !PER_KEY || b.y != 0u;
    const unsigned long long pair = (unsigned long long)a.x | ((unsigned long long)a.y << 32);
    if (pair) {
      const long long net = (long long)((unsigned long long)a.z | ((unsigned long long)a.w << 32));
      const uint32_t lim = ~b.x;
      Slot* slot = reinterpret_cast<Slot*>((uintptr_t)(pair & ~31ull));
      uint32_t* word = (pair & ADJ_PS) ? &slot->pcount : &slot->count;
      const uint32_t cnt = *word;
      const long long sum = (long long)cnt + net;  // |net| <= 2^29 * 2^31: no overflow
      floored = sum < 0;
      capped = sum > 0xFFFFFFFFll;
      const uint32_t nw = floored ? 0u : capped ? 0xFFFFFFFFu : (uint32_t)sum;
      if (nw != cnt) *word = nw;
      if (clear_cache && net < 0 && nw <= lim && release) unfrozen = atomicExch(&slot->frz, 0u) != 0u;
    }
  }
  block_add3(floored, capped, unfrozen, ADJ_FLOORED, ADJ_CAPPED, ADJ_UNFROZEN, sc.ctl);
}

}  // namespace adjust

void launch_adjust_index(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                         const TableDesc& tab, const int32_t* delta, rl_peek_reply* out, const AdjScratch& sc) {
  if (!b.n_desc) return;
  const DevBatch in = make_dev_batch(b);
  const uint32_t grid = (b.n_desc + adjust::NT - 1u) / adjust::NT;
  hipLaunchKernelGGL(adjust::k_adjust_index<false>, dim3(grid), dim3(adjust::NT), 0, st, in, rules, n_rules, seed, tab,
                     delta, out, sc, nullptr);
}
void launch_adjust_apply(hipStream_t st, bool clear_cache, bool per_key, const AdjScratch& sc) {
  const uint32_t grid = ((1u << sc.log2_entries) + adjust::NT - 1u) / adjust::NT;
  if (per_key)
    hipLaunchKernelGGL((adjust::k_adjust_apply<true, false>), dim3(grid), dim3(adjust::NT), 0, st, clear_cache, sc,
                       nullptr);
  else
    hipLaunchKernelGGL((adjust::k_adjust_apply<false, false>), dim3(grid), dim3(adjust::NT), 0, st, clear_cache, sc,
                       nullptr);
}
void launch_adjust_flight(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                          const TableDesc& tab, const int32_t* delta, rl_peek_reply* out, bool clear_cache,
                          const AdjScratch& sc, const uint32_t* poison, int pass) {
  if (!b.n_desc) return;
  if (pass == 0) {
    const DevBatch in = make_dev_batch(b);
    const uint32_t grid = (b.n_desc + adjust::NT - 1u) / adjust::NT;
    hipLaunchKernelGGL(adjust::k_adjust_index<true>, dim3(grid), dim3(adjust::NT), 0, st, in, rules, n_rules, seed, tab,
                       delta, out, sc, poison);
  } else {
    const uint32_t grid = ((1u << sc.log2_entries) + adjust::NT - 1u) / adjust::NT;
    hipLaunchKernelGGL((adjust::k_adjust_apply<false, true>), dim3(grid), dim3(adjust::NT), 0, st, clear_cache, sc,
                       poison);
  }
}

}  // namespace rlhip
