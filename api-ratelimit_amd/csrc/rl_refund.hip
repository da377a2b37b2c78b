// rl_refund.hip — a rejected request's hits given back on the device (rl_hip.h "Refund").
//   k_refund_mark   one lane per descriptor streams the statuses' code words and req_of: an
//                   over-limit descriptor stores 1 to its request's word of the zeroed rej array
//   k_refund_index  one lane per descriptor: the amount its status, its rule and its request's rej
//                   word give it; a lane that is owed something looks its counter up (rl_peek.h
//                   peek_key_slot) and, where it is found, the lanes of the wave that hold one
//                   (slot, store) pair sum their amounts, and one of them adds the sum to the
//                   pair's entry of the call's scratch index (rl_adjust.h AdjEntry)
// The applying pass is k_adjust_apply's flight form over that index, unchanged (rl_adjust.hip).
// Neither kernel writes to the table. A lane that is owed nothing reads no rule entry, no prefix
// byte and no table slot. Kernel boundaries order the three; no lane waits for another lane or
// block, and every loop is bounded: by the prefix length (hash), the region size (probe), the index
// size (insert) or the 64 lanes of a wave (combine).
// Both kernels read the poison word first (rl_adjust.hip FLIGHT): behind a batch the engine will
// rerun they write nothing and set ADJ_ERR_POISON, and the engine runs the whole refund again
// behind the rerun, this file's marking pass included, because the statuses are final only then.
// Then they read the refunded batch's own error word: a batch that failed (table full, window
// span, spin limit, bad input) wrote no status, and what its status array holds is an earlier
// batch's. Behind such a batch both kernels write nothing and set ADJ_ERR_BATCH, after which the
// applying pass writes nothing either (it reads the refund's error word).
#include <hip/hip_runtime.h>

#include "rl_adjust_key.h"
#include "rl_peek.h"
#include "rl_refund.h"
#include "rl_refund_key.h"

namespace rlhip {
namespace refund {

// True when the whole grid leaves (both words are the same for every thread): thread 0 says why.
// An error word that only asks for the rerun (ERR_FALLBACK, without a bad-input bit: settle()'s
// condition in rl_engine.cpp) counts as the poison word does.
RL_DEV bool refund_leaves(const uint32_t gi, const uint32_t* __restrict__ poison,
                          const uint32_t* __restrict__ batch_err, AdjCtl* ctl) {
  uint32_t why = *poison ? ADJ_ERR_POISON : 0u;
  if (!why && batch_err) {
    const uint32_t be = __hip_atomic_load(batch_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (be) why = (be & ERR_FALLBACK) && !(be & (ERR_BAD_INPUT | ERR_BAD_TIME)) ? ADJ_ERR_POISON : ADJ_ERR_BATCH;
  }
  if (why && gi == 0u) atomicOr(&ctl->w[ADJ_ERR][0], why);
  return why != 0u;
}

__global__ __launch_bounds__(NT) void k_refund_mark(const uint32_t n_desc, const uint32_t n_req,
                                                    const uint32_t* __restrict__ req_of,
                                                    const rl_status* __restrict__ st, uint32_t* __restrict__ rej,
                                                    AdjCtl* __restrict__ ctl, const uint32_t* __restrict__ poison,
                                                    const uint32_t* __restrict__ batch_err) {
  const uint32_t gi = blockIdx.x * NT + threadIdx.x;
  if (refund_leaves(gi, poison, batch_err, ctl)) return;
  if (gi >= n_desc) return;
  const uint32_t cf = st[gi].code_flags;
  const uint32_t q = req_of[gi];
  // every marking lane stores the same value: a plain store (a request index that is not below
  // n_req marks nothing; k_refund_index reports it)
  if ((cf & 0xFFu) == (uint32_t)RL_CODE_OVER_LIMIT && q < n_req) rej[q] = 1u;
}

// Four flags summed over the block (rl_adjust_key.h block_add3, with a word more): a ballot per
// wave, the wave sums through LDS, one add per word and block on the word's own line.
RL_DEV void block_add4(const bool a, const bool b, const bool c, const bool d, RefCtl* ctl) {
  __shared__ uint32_t sh[NT / 64][4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t ca = (uint32_t)__popcll(__ballot(a)), cb = (uint32_t)__popcll(__ballot(b)),
                 cc = (uint32_t)__popcll(__ballot(c)), cd = (uint32_t)__popcll(__ballot(d));
  if (lane == 0u) {
    sh[wave][0] = ca;
    sh[wave][1] = cb;
    sh[wave][2] = cc;
    sh[wave][3] = cd;
  }
  __syncthreads();
  if (threadIdx.x < 4u) {
    uint32_t sum = 0;
    for (int w = 0; w < NT / 64; ++w) sum += sh[w][threadIdx.x];
    uint32_t* word = threadIdx.x == 0u   ? &ctl->a.w[ADJ_NIL][0]
                     : threadIdx.x == 1u ? &ctl->a.w[ADJ_ABSENT][0]
                     : threadIdx.x == 2u ? &ctl->a.w[ADJ_APPLIED][0]
                                         : &ctl->rejected[0];
    if (sum) atomicAdd(word, sum);
  }
}

// A thread past n_desc reads descriptor n_desc - 1 and uses nothing of it (`live`): it stays for
// the wave's combine and the block's sums.
__global__ __launch_bounds__(NT) void k_refund_index(const DevBatch in, const rl_status* __restrict__ st,
                                                     const DevRule* __restrict__ rules, const uint32_t n_rules,
                                                     const uint64_t seed, const TableDesc tab,
                                                     const uint32_t* __restrict__ rej, uint32_t* __restrict__ amount,
                                                     const AdjScratch sc, const uint32_t* __restrict__ poison,
                                                     const uint32_t* __restrict__ batch_err) {
  const uint32_t gi = blockIdx.x * NT + threadIdx.x;
  if (refund_leaves(gi, poison, batch_err, sc.ctl)) return;
  const bool live = gi < in.n_desc;
  const uint32_t i = live ? gi : in.n_desc - 1u;  // n_desc >= 1 in a launched kernel
  // the streamed level: what every descriptor reads
  const uint32_t rl = in.rule[i];
  const uint32_t q = in.req_of[i];
  const uint32_t qp = in.req_of[i ? i - 1u : 0u];
  const uint32_t oa = in.off[i];
  const uint32_t ob = in.off[i + 1u];
  const uint32_t cf = st[i].code_flags;

  // rl_peek_device's checks (rl_peek.h desc_front), so that what it answers RL_PEEK_BAD is refused
  const bool nil = rl == RL_NIL_RULE;
  const bool rule_ok = rl < n_rules, q_ok = q < in.n_req;
  const bool lay = oa <= ob && ob <= in.blob_bytes && qp <= q;
  const uint32_t qc = q_ok ? q : 0u;  // n_req >= 1 (host-checked)
  const int64_t now = in.now[qc];
  const uint32_t hits = in.hits[qc];
  const uint32_t rj = rej[qc];
  const bool ok = live && !nil && rule_ok && q_ok && lay && now >= 0 && now <= MAX_NOW;
  if (live && !nil && !ok) atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_BADREC);

  // owed: a counted descriptor of a rejected request (no INCRBY happened for a nil rule or a
  // local-cache hit)
  const bool owed = ok && rj != 0u && !((cf >> 8) & (uint32_t)RL_FLAG_LOCAL_CACHE_HIT);
  const uint32_t amt = owed ? (hits > 1u ? hits : 1u) : 0u;  // utils.Max(1, HitsAddend)
  if (live && amount) amount[i] = amt;
  // (requests come in order, checked above: a request's first descriptor counts it)
  const bool first_of_rejected = live && q_ok && rj != 0u && (gi == 0u || qp != q);

  unsigned long long pair = 0ull;
  uint32_t lim_c = 0u;
  if (owed) {
    const DevRule rr = rules[rl];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(in.blob + (oa & ~3u));
    const u32x4 w0 = *reinterpret_cast<const u32x4*>(p);
    const u32x4 w1 = *reinterpret_cast<const u32x4*>(p + 4);
    const FpState s = prefix_state_pre(w0, w1, in.blob, oa, ob - oa, seed);
    Slot* slot = nullptr;
    bool ps = false;
    rl_peek_reply rep;
    rep.count = rep.ttl_s = rep.cached_s = rep.flags = 0u;
    rep = peek::peek_key_slot(s, (uint32_t)now, rr, tab, rep, slot, ps);
    if (slot) pair = (unsigned long long)reinterpret_cast<uintptr_t>(slot) | (ps ? ADJ_PS : 0ull);
    lim_c = ~rr.L;
  }
  const bool found = pair != 0ull;

  // Combine: the wave's lanes of one pair leave as one atomic set. Each round takes the lowest lane
  // still waiting as leader and retires every lane of its pair, so there are at most 64 rounds.
  // A pair alone in its wave, the common case away from a hot key, skips the reductions.
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(found);
  for (int round = 0; round < 64 && todo; ++round) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long lp = shfl64(pair, leader);
    const bool mine = pair == lp;  // (lp != 0: never a lane without a pair)
    const unsigned long long grp = __ballot(mine);
    if (grp == (1ull << leader)) {
      if (mine) index_add(pair, (unsigned long long)amt, lim_c, 0u, sc);
    } else {
      unsigned long long sum = mine ? (unsigned long long)amt : 0ull;
      uint32_t lc = mine ? lim_c : 0u;
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        sum += shfl64(sum, (int)(lane ^ (uint32_t)o));
        const uint32_t olc = (uint32_t)__shfl((int)lc, (int)(lane ^ (uint32_t)o));
        lc = olc > lc ? olc : lc;
      }
      if (lane == (uint32_t)leader) index_add(pair, sum, lc, 0u, sc);
    }
    todo &= ~grp;
  }
  block_add4(live && !owed, owed && !found, found, first_of_rejected, reinterpret_cast<RefCtl*>(sc.ctl));
}

}  // namespace refund

void launch_refund_flight(hipStream_t st_, const rl_batch& b, const rl_status* st, const DevRule* rules,
                          uint32_t n_rules, uint64_t seed, const TableDesc& tab, uint32_t* rej, uint32_t* amount,
                          const AdjScratch& sc, const uint32_t* poison, const uint32_t* batch_err, int pass) {
  if (!b.n_desc) return;
  const uint32_t grid = (b.n_desc + refund::NT - 1u) / refund::NT;
  if (pass == 0)
    hipLaunchKernelGGL(refund::k_refund_mark, dim3(grid), dim3(refund::NT), 0, st_, b.n_desc, b.n_req, b.req_of, st, rej,
                       sc.ctl, poison, batch_err);
  else
    hipLaunchKernelGGL(refund::k_refund_index, dim3(grid), dim3(refund::NT), 0, st_, make_dev_batch(b), st, rules,
                       n_rules, seed, tab, rej, amount, sc, poison, batch_err);
}

}  // namespace rlhip
