// rl_adjust_routed.hip — adjust where the keys are routed to their owners (rl_hip.h "Routed
// adjust").
//   k_adjust_index_routed  owner: one lane per routed record (RRec); the record form of
//                          k_adjust_index (rl_adjust.hip), as k_peek_routed is the record form of
//                          k_peek. The record's h word is the signed delta, bit 16 of its rule
//                          word RL_ADJUST_KEEP_CACHE
//   k_adjust_pack          origin: each descriptor's delta and the call's keep bit into its
//                          record's h and rule words (perm), behind the plain pack
// k_adjust_apply (rl_adjust.hip) runs behind k_adjust_index_routed at the commit, with the entry's
// count of records without the flag deciding each pair's cache part.
#include <hip/hip_runtime.h>

#include "rl_adjust.h"
#include "rl_adjust_key.h"
#include "rl_peek.h"

namespace rlhip {
namespace adjust {

constexpr uint32_t RREC_KEEP = 1u << 16;  // rule word: this record's RL_ADJUST_KEEP_CACHE

// k_peek_routed's three dependent levels, each one run of loads waited for once: rl_peek.h's
// rec_front with the keep word (the record, then the rule entry), then the key's first table slot
// (peek_key_slot, inside adjust_key); then adjust_key's index probe.
//
// The owner's host never sees the records, so what rl_adjust checks on the host is checked here:
// a record that is not ok gets RL_PEEK_BAD, sets ADJ_ERR_BADREC and indexes nothing. A thread past
// n reads record n - 1 and uses nothing of it: it stays for the block's sums. No lane waits for
// another; the loops are the probe (bounded by the region size) and the insert (bounded by the
// index size).
__global__ __launch_bounds__(NT) void k_adjust_index_routed(const RRec* __restrict__ recs, const uint32_t n,
                                                            const DevRule* __restrict__ rules, const uint32_t n_rules,
                                                            const TableDesc tab, rl_peek_reply* __restrict__ out,
                                                            const AdjScratch sc) {
  const uint32_t gi = blockIdx.x * NT + threadIdx.x;
  const bool live = gi < n;
  const uint32_t i = live ? gi : n - 1u;  // n >= 1: the launch is skipped for an empty call
  const peek::RecFront f = peek::rec_front(recs, rules, n_rules, i, live, true);
  const RRec& rc = f.rc;
  const bool ok = f.ok;
  rl_peek_reply rep;
  rep.count = rep.ttl_s = rep.cached_s = 0u;
  rep.flags = RL_PEEK_BAD;
  bool applied = false;
  if (ok) applied = adjust_key<true>(FpState{rc.a, rc.b}, rc.now, f.rr, (int32_t)rc.h, !(rc.rule & RREC_KEEP), tab, sc, rep);
  if (live && out) out[i] = rep;
  if (live && !ok) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_BADREC);
  block_add3(false, ok && !applied, applied, ADJ_NIL, ADJ_ABSENT, ADJ_APPLIED, sc.ctl);
}

// One lane per descriptor. The two words are computed from the batch and stored whole: the record
// is not read, and nothing else of the send buffer is touched.
__global__ __launch_bounds__(NT) void k_adjust_pack(const uint32_t n, const uint32_t cap,
                                                    const uint32_t* __restrict__ perm,
                                                    const uint32_t* __restrict__ rule_id,
                                                    const int32_t* __restrict__ delta, const uint32_t keep,
                                                    RRec* __restrict__ send) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i];
  const uint32_t rl = rule_id[i];
  const int32_t d = delta[i];
  if (p < cap) {  // (RL_ROUTE_LOCAL is above every cap)
    send[p].h = (uint32_t)d;
    send[p].rule = rl | keep << 16;
  }
}

}  // namespace adjust

void launch_adjust_index_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                                const TableDesc& tab, rl_peek_reply* out, const AdjScratch& sc) {
  if (!n) return;
  hipLaunchKernelGGL(adjust::k_adjust_index_routed, dim3((n + adjust::NT - 1u) / adjust::NT), dim3(adjust::NT), 0, st,
                     recs, n, rules, n_rules, tab, out, sc);
}

void launch_adjust_pack(hipStream_t st, uint32_t n, uint32_t cap, const uint32_t* perm, const uint32_t* rule_id,
                        const int32_t* delta, uint32_t keep, RRec* send) {
  if (!n) return;
  hipLaunchKernelGGL(adjust::k_adjust_pack, dim3((n + adjust::NT - 1u) / adjust::NT), dim3(adjust::NT), 0, st, n, cap,
                     perm, rule_id, delta, keep, send);
}

}  // namespace rlhip
