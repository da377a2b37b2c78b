// rl_set_routed.hip — set where the keys are routed to their owners (rl_hip.h "Routed set",
// DESIGN.md §4f).
//   k_set_index_routed  owner: one lane per routed record (RRec) and its value; the record form of
//                       k_set_index (rl_set.hip), as k_peek_routed is the record form of k_peek
//   k_set_values_pack   origin: each descriptor's value to its record's place (perm) in a buffer
//                       laid out like the strided record buffer
// k_set_plan and k_set_apply (rl_set.hip) run behind k_set_index_routed unchanged.
#include <hip/hip_runtime.h>

#include "rl_peek.h"
#include "rl_set.h"
#include "rl_set_index.h"

namespace rlhip {
namespace set {

constexpr int NTR = peek::NT;

// Two dependent levels of loads, each waited for once: the record (32 B) with its value (16 B),
// then the rule entry at a clamped id (rl_peek.h rec_front); then set_index_tail's index probe.
// Record index i is origin-major, then descriptor order inside the origin (the pack keeps serial
// order inside an owner's group, the exchange is origin-major), so "largest index wins" is "the
// last SET wins, the origins' batches one after another in shard order".
//
// The owner's host sees neither records nor values, so what rl_set checks on the host is checked
// here: a malformed record or value sets an error bit and indexes nothing, and the window
// generations of the records that write something go, per region, into the control block (largest,
// and largest complement) for the host to compare. Per wave and region that is one atomicMax pair
// in the common case: the first lane of the region's ballot issues it, a lane whose generation
// differs from that lane's issues its own. (Reading the words first and skipping an atomicMax that
// could not raise its word measured no faster at 10^6 records of one region) No
// lane returns early (the ballots and the shuffle cover the whole wave), no lane waits for another,
// every loop is bounded.
__global__ __launch_bounds__(NTR) void k_set_index_routed(const RRec* __restrict__ recs,
                                                          const rl_peek_reply* __restrict__ values, const uint32_t n,
                                                          const DevRule* __restrict__ rules, const uint32_t n_rules,
                                                          const TableDesc tab, const SetScratch sc) {
  const uint32_t i = blockIdx.x * NTR + threadIdx.x;
  const bool in = i < n;
  const uint32_t ic = in ? i : n - 1u;  // n >= 1: the launch is skipped for an empty call
  const rl_peek_reply v = values[ic];
  const peek::RecFront f = peek::rec_front(recs, rules, n_rules, ic, true, false);
  const RRec& rc = f.rc;
  const DevRule& rr = f.rr;
  const bool rec_ok = f.ok;
  const uint32_t t = rc.now;
  const bool wc = !(v.flags & RL_SET_KEEP_COUNTER);
  const bool wf = !(v.flags & RL_SET_KEEP_CACHE) && tab.local_cache;
  const bool ps = per_second_store(tab, rr.unit);
  // only the parts the record writes count
  const bool chk_ttl = wc && (v.flags & RL_PEEK_FOUND) && !ps;
  const bool chk_frz = wf && (v.flags & RL_PEEK_LOCAL_CACHED);
  const bool val_ok = !(chk_ttl && (!v.ttl_s || (uint64_t)t + v.ttl_s >= (1ull << 32))) &&
                      !(chk_frz && (!v.cached_s || (uint64_t)t + v.cached_s >= (1ull << 32)));
  if (in && !(rec_ok && val_ok)) atomicOr(&sc.ctl->err, !rec_ok ? SET_ERR_BADREC : SET_ERR_BADVAL);
  const bool on = in && rec_ok && val_ok && (wc || wf);
  const peek::KeyIdent id = peek::key_ident(FpState{rc.a, rc.b}, t, rr);  // (pure arithmetic, any lane)

  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = 0; r < 8; ++r) {
    const bool mine = on && id.pl.region == r;
    const uint64_t m = __ballot(mine);
    if (!m) continue;  // wave-uniform
    const uint32_t first = (uint32_t)(__ffsll((unsigned long long)m) - 1);
    const uint32_t g0 = (uint32_t)__shfl((int)id.pl.gen, (int)first);
    if (mine && (lane == first || id.pl.gen != g0)) {
      atomicMax(&sc.ctl->gen_max[r][0], id.pl.gen);
      atomicMax(&sc.ctl->gen_minc[r][0], ~id.pl.gen);
    }
  }

  SetDesc d;
  d.ent = SETD_NONE;
  d.tag = 0u;
  if (on) d = set_index_tail(i, id, t, v, wc, wf, ps, sc);
  if (in) sc.desc[i] = d;
}

// One lane per descriptor. perm: the strided form of the plain pack (owner * stride + position), or
// RL_ROUTE_LOCAL for a descriptor without a limit; cap: the records vsend has room for.
__global__ __launch_bounds__(NTR) void k_set_values_pack(const uint32_t n, const uint32_t cap,
                                                         const uint32_t* __restrict__ perm,
                                                         const rl_peek_reply* __restrict__ values,
                                                         rl_peek_reply* __restrict__ vsend) {
  const uint32_t i = blockIdx.x * NTR + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i];
  const rl_peek_reply v = values[i];
  if (p < cap) vsend[p] = v;  // (RL_ROUTE_LOCAL is above every cap)
}

}  // namespace set

void launch_set_index_routed(hipStream_t st, const RRec* recs, const rl_peek_reply* values, uint32_t n,
                             const DevRule* rules, uint32_t n_rules, const TableDesc& tab, const SetScratch& sc) {
  if (!n) return;
  hipLaunchKernelGGL(set::k_set_index_routed, dim3((n + set::NTR - 1u) / set::NTR), dim3(set::NTR), 0, st, recs, values,
                     n, rules, n_rules, tab, sc);
}

void launch_set_values_pack(hipStream_t st, uint32_t n, uint32_t cap, const uint32_t* perm, const rl_peek_reply* values,
                            rl_peek_reply* vsend) {
  if (!n) return;
  hipLaunchKernelGGL(set::k_set_values_pack, dim3((n + set::NTR - 1u) / set::NTR), dim3(set::NTR), 0, st, n, cap, perm,
                     values, vsend);
}

}  // namespace rlhip
