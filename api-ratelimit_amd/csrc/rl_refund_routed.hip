// rl_refund_routed.hip — refund where the keys are routed to their owners (rl_hip.h "Routed
// refund").
//   k_refund_owed          origin, behind k_refund_mark (rl_refund.hip): one lane per descriptor
//                          streams its status word, rule id, request index and its request's rej
//                          word and hits_addend, and writes what it is owed and the rule id the
//                          plain pack then sees: its own when it is owed, else RL_NIL_RULE, so that
//                          an unowed descriptor stays at home (perm == RL_ROUTE_LOCAL). No rule
//                          entry, no prefix byte and no table slot is read
//   k_refund_index_routed  owner: one lane per routed record (RRec); the record form of
//                          k_refund_index (rl_refund.hip), as k_adjust_index_routed is of
//                          k_adjust_index. The record's h word is the amount, a full uint32, bit 16
//                          of its rule word RL_REFUND_KEEP_CACHE
// k_adjust_pack (rl_adjust_routed.hip) writes the amounts into the records: it stores the 32 bits of
// its delta word whole. k_adjust_apply's per-key form (rl_adjust.hip) runs behind
// k_refund_index_routed at the commit. Neither kernel here writes to the table; no lane waits for
// another lane or block, and every loop is bounded: by the region size (probe), the index size
// (insert) or the 64 lanes of a wave (combine).
#include <hip/hip_runtime.h>

#include "rl_peek.h"
#include "rl_refund.h"
#include "rl_refund_key.h"

namespace rlhip {
namespace refund {

constexpr uint32_t RREC_KEEP = 1u << 16;  // rule word: this record's RL_REFUND_KEEP_CACHE

// Two flags summed over the block into counts[0] and counts[1] (rl_refund.hip block_add4's
// pattern): a ballot per wave, the wave sums through LDS, one add per word and block.
RL_DEV void block_add2(const bool a, const bool b, uint32_t* __restrict__ counts) {
  __shared__ uint32_t sh[NT / 64][2];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t ca = (uint32_t)__popcll(__ballot(a)), cb = (uint32_t)__popcll(__ballot(b));
  if (lane == 0u) {
    sh[wave][0] = ca;
    sh[wave][1] = cb;
  }
  __syncthreads();
  if (threadIdx.x < 2u) {
    uint32_t sum = 0;
    for (int w = 0; w < NT / 64; ++w) sum += sh[w][threadIdx.x];
    if (sum) atomicAdd(counts + threadIdx.x, sum);
  }
}

// rule_out may be rule_in (neither is __restrict__): a lane reads its word before it writes it,
// and reads no other lane's. A thread past n_desc reads nothing and stays for the block's sums.
// A descriptor whose request index is not below n_req keeps its rule id, so that the pack behind
// refuses the batch as it refuses any other with such a descriptor.
__global__ __launch_bounds__(NT) void k_refund_owed(const uint32_t n_desc, const uint32_t n_req, const uint32_t* rule_in,
                                                    const uint32_t* __restrict__ req_of,
                                                    const uint32_t* __restrict__ hits_addend,
                                                    const rl_status* __restrict__ st,
                                                    const uint32_t* __restrict__ rej, uint32_t* rule_out,
                                                    uint32_t* __restrict__ amount, uint32_t* __restrict__ counts) {
  const uint32_t gi = blockIdx.x * NT + threadIdx.x;
  const bool live = gi < n_desc;
  bool owed = false, first_of_rejected = false;
  if (live) {
    const uint32_t rl = rule_in[gi];
    const uint32_t q = req_of[gi];
    const uint32_t qp = req_of[gi ? gi - 1u : 0u];
    const uint32_t cf = st[gi].code_flags;
    const bool q_ok = q < n_req;
    const uint32_t qc = q_ok ? q : 0u;  // n_req >= 1 (host-checked)
    const uint32_t hits = hits_addend[qc];
    const uint32_t rj = rej[qc];
    // owed: a counted descriptor of a rejected request (no INCRBY happened for a nil rule or a
    // local-cache hit): rl_refund_pipelined's rule
    owed = q_ok && rj != 0u && rl != RL_NIL_RULE && !((cf >> 8) & (uint32_t)RL_FLAG_LOCAL_CACHE_HIT);
    amount[gi] = owed ? (hits > 1u ? hits : 1u) : 0u;  // utils.Max(1, HitsAddend)
    rule_out[gi] = owed || !q_ok ? rl : RL_NIL_RULE;
    // (requests come in order: a request's first descriptor counts it, as in k_refund_index)
    first_of_rejected = q_ok && rj != 0u && (gi == 0u || qp != q);
  }
  block_add2(first_of_rejected, owed, counts);
}

// k_adjust_index_routed's front and lookup (rl_peek.h rec_front with the keep word, then
// peek_key_slot at the record's own time), then k_refund_index's combine: the wave's lanes of one
// (slot, store) pair leave as one atomic set. The owner's host never sees the records, so a record
// that is not ok gets RL_PEEK_BAD, sets ADJ_ERR_BADREC and indexes nothing. A thread past n reads
// record n - 1 and uses nothing of it: it stays for the wave's combine and the block's sums.
__global__ __launch_bounds__(NT) void k_refund_index_routed(const RRec* __restrict__ recs, const uint32_t n,
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
  unsigned long long pair = 0ull;
  if (ok) {
    Slot* slot = nullptr;
    bool ps = false;
    rep = peek::peek_key_slot(FpState{rc.a, rc.b}, rc.now, f.rr, tab, rep, slot, ps);
    if (slot) pair = (unsigned long long)reinterpret_cast<uintptr_t>(slot) | (ps ? ADJ_PS : 0ull);
  }
  if (live && out) out[i] = rep;
  if (live && !ok) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_BADREC);
  const bool found = pair != 0ull;
  const unsigned long long amt = (unsigned long long)rc.h;  // the full uint32: never an int32
  const uint32_t lim_c = ~f.rr.L;
  const bool rel = found && !(rc.rule & RREC_KEEP);  // came without the keep bit

  // Combine (k_refund_index): each round takes the lowest lane still waiting as leader and retires
  // every lane of its pair, so there are at most 64 rounds. A pair alone in its wave, the common
  // case away from a hot key, skips the reductions.
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(found);
  for (int round = 0; round < 64 && todo; ++round) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long lp = shfl64(pair, leader);
    const bool mine = pair == lp;  // (lp != 0: never a lane without a pair)
    const unsigned long long grp = __ballot(mine);
    if (grp == (1ull << leader)) {
      if (mine) index_add(pair, amt, lim_c, rel ? 1u : 0u, sc);
    } else {
      const uint32_t n_rel = (uint32_t)__popcll(__ballot(mine && rel));
      unsigned long long sum = mine ? amt : 0ull;
      uint32_t lc = mine ? lim_c : 0u;
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        sum += shfl64(sum, (int)(lane ^ (uint32_t)o));
        const uint32_t olc = (uint32_t)__shfl((int)lc, (int)(lane ^ (uint32_t)o));
        lc = olc > lc ? olc : lc;
      }
      if (lane == (uint32_t)leader) index_add(pair, sum, lc, n_rel, sc);
    }
    todo &= ~grp;
  }
  adjust::block_add3(false, ok && !found, found, ADJ_NIL, ADJ_ABSENT, ADJ_APPLIED, sc.ctl);
}

}  // namespace refund

void launch_refund_owed(hipStream_t st_, const rl_batch& b, const rl_status* st, const uint32_t* rej, uint32_t* rule_out,
                        uint32_t* amount, uint32_t* counts) {
  if (!b.n_desc) return;
  const uint32_t grid = (b.n_desc + refund::NT - 1u) / refund::NT;
  hipLaunchKernelGGL(refund::k_refund_owed, dim3(grid), dim3(refund::NT), 0, st_, b.n_desc, b.n_req, b.rule_id, b.req_of,
                     b.hits_addend, st, rej, rule_out, amount, counts);
}

void launch_refund_index_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                                const TableDesc& tab, rl_peek_reply* out, const AdjScratch& sc) {
  if (!n) return;
  hipLaunchKernelGGL(refund::k_refund_index_routed, dim3((n + refund::NT - 1u) / refund::NT), dim3(refund::NT), 0, st,
                     recs, n, rules, n_rules, tab, out, sc);
}

}  // namespace rlhip
