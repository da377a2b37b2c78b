// rl_merge.h — what the engine (rl_engine.cpp) and the merge kernels (rl_merge.hip) share, and
// the rule of the merge itself (rl_hip.h "Merge") as host/device functions, so the
// kernels, the engine's host pass and the tests' host restatements agree by construction.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_common.h"
#include "rl_set.h"
#include "rl_snapshot.h"

namespace rlhip {

// The per-key state of a record or slot (rl_common.h Slot's last four words).
struct MergeState {
  uint32_t count, exp, pcount, frz;
};

// Class of a record of generation g in a region whose target generation is T: 0 = applies as the
// newest generation, 1 = applies as a lag region's previous one (T - 2), 2 = over.
constexpr uint32_t MERGE_NEWEST = 0u, MERGE_PREVIOUS = 1u, MERGE_OVER = 2u;
__host__ __device__ __forceinline__ uint32_t merge_class(uint32_t g, uint32_t T, bool lazy) {
  if (g == 0u) return MERGE_OVER;
  if (g == T) return MERGE_NEWEST;
  return lazy && g + 2u == T ? MERGE_PREVIOUS : MERGE_OVER;
}

// A record leaves something at `now`: a main counter still alive, a per-second counter, or (local
// cache on) a cache entry still held.
__host__ __device__ __forceinline__ bool merge_leaves(const MergeState& r, uint32_t now, bool local_cache) {
  return now < r.exp || r.pcount != 0u || (local_cache && now < r.frz);
}

// Slot state S (found: the identity is in the table; otherwise S is ignored) and record R -> the
// slot's state afterwards. Counters add in their own width (INCRBY commutes), the expiry and the
// local-cache deadline take the later one; a main counter that is dead at `now` on either side
// contributes nothing, and a dead record leaves the slot's main words as they are.
__host__ __device__ __forceinline__ MergeState merge_fold(const MergeState& S, bool found, const MergeState& R,
                                                          uint32_t now) {
  MergeState o = found ? S : MergeState{0u, 0u, 0u, 0u};
  const bool aR = now < R.exp, aS = found && now < S.exp;
  if (aR && aS) {
    o.count = S.count + R.count;
    o.exp = S.exp > R.exp ? S.exp : R.exp;
  } else if (aR) {
    o.count = R.count;
    o.exp = R.exp;
  }
  o.pcount += R.pcount;
  o.frz = o.frz > R.frz ? o.frz : R.frz;
  return o;
}

// Control block of one call, zeroed at its start. As in SnapCtl and SetCtl, every word that more
// than one block adds to lives on a 256-B line of its own. Count rows: region * 2 + class.
struct MergeCtl {
  uint32_t err;                       // MERGE_ERR_*, atomicOr, only on an error
  uint32_t pad0[63];
  uint32_t plan[SNAP_CLASSES][64];    // k_merge_plan: absent identities that apply and leave something
  uint32_t claim[SNAP_CLASSES][64];   // k_merge_apply: slots claimed
  uint32_t folded[64];                // k_merge_apply: records folded into an existing slot
  uint32_t over[64];                  // k_merge_plan: records whose generation is over
  uint32_t empty[64];                 // k_merge_plan: records that leave nothing
};
static_assert(sizeof(MergeCtl) == (1 + 2 * SNAP_CLASSES + 3) * 256, "MergeCtl layout");
enum : uint32_t {
  MERGE_ERR_INDEX = 1u,  // the index had no entry left (unreachable: 2^k >= 2 n)
  MERGE_ERR_MIXED = 2u,  // two identities share one 64-bit sort key in this call: split the call
  MERGE_ERR_DUP = 4u,    // one identity (claim word, key) twice in this call
  MERGE_ERR_FULL = 8u,   // no free slot in a region (unreachable below the load limit)
};

// The scratch is rl_set's (SetScratch: the index of 2^log2_entries entries, zeroed by the caller
// on the stream, and the per-record desc array); ctl is the merge's own. T: the target generation
// per region, by value.
struct MergeArgs {
  const Slot* recs;  // n records in device memory
  uint32_t n;
  uint32_t now;
  SnapGens T;
  SetEntry* index;
  uint32_t log2_entries;
  SetDesc* desc;
  MergeCtl* ctl;
};
// k_merge_plan, then k_merge_check behind it (the index is complete at the kernel boundary).
// Neither writes the table.
void launch_merge_plan(hipStream_t st, const TableDesc& tab, const MergeArgs& a);
void launch_merge_apply(hipStream_t st, const TableDesc& tab, const MergeArgs& a);

}  // namespace rlhip

// Host restatements of the rule for tests that run without a GPU (exported from the library
// beside rlhip::resolve_one_host). S, R, out: {count, exp, pcount, frz}.
extern "C" {
void rlx_merge_fold_host(const uint32_t S[4], int found, const uint32_t R[4], uint32_t now, uint32_t out[4]);
uint32_t rlx_merge_class_host(uint32_t g, uint32_t T, int lazy);
int rlx_merge_leaves_host(const uint32_t R[4], uint32_t now, int local_cache);
}
