// rl_merge.hip — fold the records of a snapshot into a live counter table (rl_hip.h "Merge",
// DESIGN.md §4g). A record is one table slot, verbatim (rl_snapshot.hip): its claim word carries
// the window generation and the tag, its sort key the region and the bits its place is taken from.
//   k_merge_plan   one lane per record, read-only on the table: classify it against the region's
//                  target generation, enter its identity into the call's scratch index (one 64-bit
//                  CAS elects the identity's first lane, which stores tag and generation beside the
//                  key), look it up and count, per (region, class), the slots the call would claim
//   k_merge_check  one lane per record, behind the kernel boundary that completes the index: a
//                  record that met an occupied entry has either that entry's identity (a duplicate)
//                  or another one on the same 64-bit sort key (mixed)
//   k_merge_apply  one lane per record that applies and leaves something: claim or find its slot
//                  (table_claim_pre, the pipelines' claim) and write the folded state
// No LDS, no lane waits for another lane or block, and every loop is bounded by the index size
// (insert) or the region size (probe). A record's key selects its region by its top three bits and
// its slot by masked bits, so any 32 bytes address only the table.
#include <hip/hip_runtime.h>

#include "rl_decide.h"
#include "rl_merge.h"

namespace rlhip {
namespace merge {

constexpr int NT = 256;

// Per-wave sum of one count row, one add per wave and non-zero word (rl_snapshot.hip
// count_classes). Every lane of the wave calls it.
RL_DEV void count_rows(bool on, uint32_t row, uint32_t (*cnt)[64]) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t c = 0; c < (uint32_t)SNAP_CLASSES; ++c) {
    const uint64_t m = __ballot(on && row == c);
    if (m && lane == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(&cnt[c][0], (uint32_t)__popcll(m));
  }
}
RL_DEV void count_one(bool on, uint32_t* word) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t m = __ballot(on);
  if (m && lane == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(word, (uint32_t)__popcll(m));
}

// A record as a lane holds it, with its first probe slot read ahead: both 16-B loads of the
// record go out first (at a clamped index: no load behind the bounds branch), then the slot's
// two, which depend only on the key (k_peek's load levels).
struct Rec {
  bool valid;
  uint64_t key;
  uint32_t gen, tag, region;
  MergeState st;
  SlotView pre;
  uint32_t cls;   // MERGE_NEWEST / MERGE_PREVIOUS / MERGE_OVER
  bool leaves;
};
RL_DEV Rec load_rec(const TableDesc& tab, const MergeArgs& a, uint32_t i) {
  Rec r;
  r.valid = i < a.n;
  const uint4* p = reinterpret_cast<const uint4*>(a.recs + (r.valid ? i : 0u));  // n > 0 (launch_*)
  const uint4 w0 = p[0];
  const uint4 w1 = p[1];
  r.gen = w0.x;
  r.tag = w0.y;
  r.key = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
  r.region = key_region(r.key);
  r.pre = load_slot(slot_first(tab, r.key));
  r.st = MergeState{w1.x, w1.y, w1.z, w1.w};
  r.cls = merge_class(r.gen, snap::gen_of_region(a.T, r.region), lazy_region(tab.lag, r.region));
  r.leaves = merge_leaves(r.st, a.now, tab.local_cache != 0u);
  return r;
}

__global__ __launch_bounds__(NT) void k_merge_plan(const TableDesc tab, const MergeArgs a) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  const Rec r = load_rec(tab, a, i);
  const bool over = r.valid && r.cls == MERGE_OVER;
  const bool empty = r.valid && !over && !r.leaves;
  const bool applies = r.valid && !over && r.leaves;
  if (r.valid) {
    // every record enters the index: an identity twice in one call is refused whatever its class
    const unsigned long long key1 = r.key + 1ull;  // 0 = empty: NIL_KEY is never a sort key
    const uint32_t lg = a.log2_entries;
    const uint32_t mask = (1u << lg) - 1u;
    uint32_t pos = (uint32_t)((key1 * K0) >> (64 - lg));
    SetDesc d;
    d.ent = SETD_NONE;
    d.tag = 0u;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
      // the CAS is the read: it returns the word from the L2, never a line cached before an insert
      const unsigned long long old = atomicCAS(&a.index[pos].key1, 0ull, key1);
      if (old == 0ull) {
        a.index[pos].tag = r.tag;  // read by k_merge_check only, behind the kernel boundary
        a.index[pos].gen = r.gen;
        d.ent = pos | SETD_LEADER;
        break;
      }
      if (old == key1) {
        d.ent = pos;
        break;
      }
      pos = (pos + 1u) & mask;
    }
    if (d.ent == SETD_NONE) atomicOr(&a.ctl->err, MERGE_ERR_INDEX);
    a.desc[i] = d;
  }
  bool absent = false;
  if (applies) {
    Slot* slot = nullptr;
    KeyState ks;
    absent = !table_find(tab, r.key, r.tag, r.gen, r.pre, slot, ks);
  }
  count_rows(absent, r.region * 2u + r.cls, a.ctl->plan);
  count_one(over, &a.ctl->over[0]);
  count_one(empty, &a.ctl->empty[0]);
}

__global__ __launch_bounds__(NT) void k_merge_check(const MergeArgs a) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= a.n) return;
  const SetDesc d = a.desc[i];
  const uint4 w0 = reinterpret_cast<const uint4*>(a.recs + i)[0];
  if (d.ent == SETD_NONE || (d.ent & SETD_LEADER)) return;
  const SetEntry* e = a.index + d.ent;  // d.ent < 2^log2_entries: a position the probe visited
  atomicOr(&a.ctl->err, e->tag == w0.y && e->gen == w0.x ? MERGE_ERR_DUP : MERGE_ERR_MIXED);
}

// Identities are unique within the call (k_merge_check ran first and the engine refused the call
// otherwise) and nothing else is in flight, so exactly one lane looks a given slot up, claims it
// and writes its state: the read-ahead of an existing slot is current, and the fold needs no
// atomics. That is why the duplicate check must precede this kernel.
__global__ __launch_bounds__(NT) void k_merge_apply(const TableDesc tab, const MergeArgs a) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  const Rec r = load_rec(tab, a, i);
  bool claimed = false, folded = false;
  if (r.valid && r.cls != MERGE_OVER && r.leaves) {
    Slot* slot = nullptr;
    bool existed = false;
    KeyState ks{0, 0, 0, 0};
    if (!table_claim_pre(tab, r.key, r.tag, r.gen, r.pre, slot, existed, ks)) {
      atomicOr(&a.ctl->err, MERGE_ERR_FULL);  // unreachable: the engine checked the exact claim count
    } else {
      if (!existed) slot->key = r.key;
      const MergeState s = merge_fold(MergeState{ks.count, ks.exp, ks.pcount, ks.frz}, existed, r.st, a.now);
      write_state(slot, KeyState{s.count, s.exp, s.pcount, s.frz});
      claimed = !existed;
      folded = existed;
    }
  }
  count_rows(claimed, r.region * 2u + r.cls, a.ctl->claim);
  count_one(folded, &a.ctl->folded[0]);
}

}  // namespace merge

void launch_merge_plan(hipStream_t st, const TableDesc& tab, const MergeArgs& a) {
  if (!a.n) return;
  const uint32_t grid = (a.n + merge::NT - 1u) / merge::NT;
  hipLaunchKernelGGL(merge::k_merge_plan, dim3(grid), dim3(merge::NT), 0, st, tab, a);
  hipLaunchKernelGGL(merge::k_merge_check, dim3(grid), dim3(merge::NT), 0, st, a);
}
void launch_merge_apply(hipStream_t st, const TableDesc& tab, const MergeArgs& a) {
  if (!a.n) return;
  const uint32_t grid = (a.n + merge::NT - 1u) / merge::NT;
  hipLaunchKernelGGL(merge::k_merge_apply, dim3(grid), dim3(merge::NT), 0, st, tab, a);
}

}  // namespace rlhip

extern "C" {
void rlx_merge_fold_host(const uint32_t S[4], int found, const uint32_t R[4], uint32_t now, uint32_t out[4]) {
  const rlhip::MergeState o = rlhip::merge_fold(rlhip::MergeState{S[0], S[1], S[2], S[3]}, found != 0,
                                                rlhip::MergeState{R[0], R[1], R[2], R[3]}, now);
  out[0] = o.count;
  out[1] = o.exp;
  out[2] = o.pcount;
  out[3] = o.frz;
}
uint32_t rlx_merge_class_host(uint32_t g, uint32_t T, int lazy) { return rlhip::merge_class(g, T, lazy != 0); }
int rlx_merge_leaves_host(const uint32_t R[4], uint32_t now, int local_cache) {
  return rlhip::merge_leaves(rlhip::MergeState{R[0], R[1], R[2], R[3]}, now, local_cache != 0) ? 1 : 0;
}
}
