// rl_snapshot.h — what the engine (rl_engine.cpp) and the snapshot kernels (rl_snapshot.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_common.h"

namespace rlhip {

// Per region: the newest window generation (RegionOcc.gen at rl_snapshot_begin, or the
// snapshot header's at restore), passed by value.
struct SnapGens {
  uint32_t gen[8];
};

// (region, generation class) count words: region * 2 + class, class 0 = the region's newest
// generation, 1 = a lag region's previous one (gen - 2).
constexpr int SNAP_CLASSES = 16;

// Control block of one snapshot or restore, zeroed at its begin. As in EngineCtl, every word
// that more than one block adds to lives on a 256-B line of its own.
struct SnapCtl {
  uint32_t err;                  // SNAP_ERR_*, atomicOr, only on an error
  uint32_t pad0[63];
  unsigned long long cursor;     // export: records reserved so far (one add per tile)
  uint32_t pad1[62];
  uint32_t cnt[SNAP_CLASSES][64];  // records exported / imported per (region, class)
};
static_assert(sizeof(SnapCtl) == (2 + SNAP_CLASSES) * 256, "SnapCtl layout");

enum : uint32_t {
  SNAP_ERR_OVERFLOW = 1u,  // export: more live slots than the buffer holds (none written past it)
  SNAP_ERR_GEN = 2u,       // import: a record's generation is not live under the header
  SNAP_ERR_FULL = 4u,      // import: no free slot in the record's region
  SNAP_ERR_DUP = 8u,       // import: the identity (claim word, key) occurs twice
};

// What every streaming table pass shares (k_snap_export, k_rehash, rl_census.hip k_census).
namespace snap {
// Region of a table slot index, and that region's newest generation, by select chains over
// constant indices (the by-value arguments stay in scalar registers, rl_decide.h region_geom).
__device__ __forceinline__ uint32_t region_of_slot(const TableDesc& tab, uint64_t i) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k) r += i >= tab.region_base[k] ? 1u : 0u;
  return r;
}
__device__ __forceinline__ uint32_t gen_of_region(const SnapGens& g, uint32_t region) {
  uint32_t v = g.gen[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) v = region == (uint32_t)k ? g.gen[k] : v;
  return v;
}
// Generation class of a slot of generation g in a region whose newest generation is G:
// 0 = the newest, 1 = a lag region's previous one (G - 2), 2 = not live (rl_hip.h "What is live").
__device__ __forceinline__ uint32_t gen_class(uint32_t g, uint32_t G, bool lazy) {
  if (g == 0u) return 2u;
  if (g == G) return 0u;
  return lazy && g + 2u == G ? 1u : 2u;
}
}  // namespace snap

void launch_snap_export(hipStream_t st, const TableDesc& tab, uint64_t n_slots, const SnapGens& gens, Slot* out,
                        uint64_t cap, SnapCtl* ctl);
// Import n records (device memory), then check the chunk for duplicate identities.
void launch_snap_import(hipStream_t st, const TableDesc& tab, const Slot* recs, uint32_t n, const SnapGens& gens,
                        SnapCtl* ctl);
// rl_resize: move every live slot of src (n_slots slots) into dst, a zeroed table of another
// geometry; counts per (region, class) in ctl->cnt, SNAP_ERR_FULL / _DUP / _GEN in ctl->err.
void launch_rehash(hipStream_t st, const TableDesc& src, uint64_t n_slots, const SnapGens& gens, const TableDesc& dst,
                   SnapCtl* ctl);

}  // namespace rlhip
