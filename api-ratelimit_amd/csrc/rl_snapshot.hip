// rl_snapshot.hip — snapshot / restore of the counter table (rl_hip.h "Snapshot / restore",
// DESIGN.md §4a). A record is one live Slot, verbatim (32 B): the claim word carries the
// window generation and the tag, the sort key carries the region and the bits a slot's place
// is taken from (slot_first), so a record can be re-inserted into a region of any size.
//   k_snap_export  one streaming pass over the table: live slots -> a packed record array
//   k_snap_import  one lane per record: claim a slot under the new geometry, write the state
//   k_snap_verify  one lane per record, after the import of the same chunk: the identity
//                  occurs exactly once on its probe chain (duplicates inside one chunk)
//   k_rehash       rl_resize: export's read side and import's claim side in one
//                  pass, old table -> new table
#include <hip/hip_runtime.h>

#include "rl_decide.h"
#include "rl_snapshot.h"

namespace rlhip {
namespace snap {

constexpr int NT = 1024;                 // threads per export block (16 waves)
constexpr int PER = 4;                   // slots per lane and tile
constexpr int TILE = NT * PER;           // slots per reservation
constexpr int NW = NT / 64;
static_assert(TILE >= 4096, "one returning atomic per >= 4096 slots");

// Export. A block takes tiles of TILE consecutive slots (grid-stride): every lane reads PER
// slots (two 16-B loads each, all issued before the first use), the live ones are counted per
// wave by ballot, the tile's total takes ONE reservation on the output cursor, and every live
// lane stores its record at reservation + wave prefix + rank within the wave. Per (region,
// class) counts are summed in LDS and added once per tile and non-zero word, each word on a
// 256-B line of its own (SnapCtl). No lane waits for another block: every loop is bounded by
// the slot count.
__global__ __launch_bounds__(NT) void k_snap_export(const TableDesc tab, const uint64_t n_slots, const SnapGens gens,
                                                     Slot* __restrict__ out, const uint64_t cap, SnapCtl* ctl) {
  __shared__ uint32_t sh_wcnt[PER][NW];   // live lanes per (pass, wave)
  __shared__ uint32_t sh_cls[SNAP_CLASSES];
  __shared__ unsigned long long sh_base;
  __shared__ uint32_t sh_ok;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint64_t n_tiles = (n_slots + TILE - 1) / TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (tid < (uint32_t)SNAP_CLASSES) sh_cls[tid] = 0u;
    __syncthreads();
    const uint64_t i0 = tile * TILE + tid;
    uint4 a[PER], b[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      a[k] = make_uint4(0u, 0u, 0u, 0u);
      b[k] = a[k];
      if (i < n_slots) {
        const uint4* p = reinterpret_cast<const uint4*>(tab.slots + i);
        a[k] = p[0];
        b[k] = p[1];
      }
    }
    uint32_t rank[PER];
    bool live[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      const uint32_t r = region_of_slot(tab, i);
      const uint32_t c = i < n_slots ? gen_class(a[k].x, gen_of_region(gens, r), lazy_region(tab.lag, r)) : 2u;
      live[k] = c < 2u;
      const uint64_t m = __ballot(live[k]);
      rank[k] = (uint32_t)__popcll(m & lanemask_lt());
      if (lane == 0) sh_wcnt[k][wave] = (uint32_t)__popcll(m);
      if (live[k]) atomicAdd(&sh_cls[r * 2u + c], 1u);
    }
    __syncthreads();
    // exclusive prefix of this lane's (pass, wave) cells in pass-major order, and the total
    uint32_t before[PER], total = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      before[k] = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const uint32_t v = sh_wcnt[k][w];
        before[k] += (uint32_t)w < wave ? v : 0u;
        total += v;
      }
    }
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      uint32_t row = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) row += sh_wcnt[k][w];
      before[k] += acc;
      acc += row;
    }
    if (tid == 0) {
      unsigned long long base = 0;
      uint32_t ok = 1u;
      if (total) {
        base = atomicAdd(&ctl->cursor, (unsigned long long)total);
        if (base + total > cap) {  // never with the mirror's conservative count; nothing is written past cap
          ok = 0u;
          atomicOr(&ctl->err, SNAP_ERR_OVERFLOW);
        }
      }
      sh_base = base;
      sh_ok = ok;
    }
    if (tid < (uint32_t)SNAP_CLASSES && sh_cls[tid]) atomicAdd(&ctl->cnt[tid][0], sh_cls[tid]);
    __syncthreads();
    if (sh_ok) {
      const unsigned long long base = sh_base;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        if (live[k]) {
          uint4* q = reinterpret_cast<uint4*>(out + base + before[k] + rank[k]);
          q[0] = a[k];
          q[1] = b[k];
        }
      }
    }
    __syncthreads();  // sh_base / sh_wcnt are rewritten by the next tile
  }
}

// Per-wave sum of one (region, class) count, one add per non-zero word (count_inserts).
RL_DEV void count_classes(bool ok, uint32_t cls, SnapCtl* ctl) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t c = 0; c < (uint32_t)SNAP_CLASSES; ++c) {
    const uint64_t m = __ballot(ok && cls == c);
    if (m && lane == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(&ctl->cnt[c][0], (uint32_t)__popcll(m));
  }
}

// Import: one lane per record. The region is the key's, the generation the record's; it must be
// the header's newest generation of the region or, in a lag region, the one before it. The slot
// is claimed with table_claim under this engine's geometry (probe bounded by the region size;
// rl_restore_begin's capacity check leaves a free slot), then key and state are written. An
// identity already in the table (an earlier chunk's) is a duplicate. Generations G and G - 2 of
// a lag region import side by side: slot_free_for keeps them apart.
__global__ __launch_bounds__(256) void k_snap_import(const TableDesc tab, const Slot* __restrict__ recs, const uint32_t n,
                                                      const SnapGens gens, SnapCtl* ctl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  uint32_t cls = 0;
  if (i < n) {
    const SlotView v = load_slot(recs + i);
    const uint32_t r = key_region(v.key);
    const uint32_t G = (uint32_t)v.ctrl;
    const uint32_t c = gen_class(G, gen_of_region(gens, r), lazy_region(tab.lag, r));
    if (c == 2u) {
      atomicOr(&ctl->err, SNAP_ERR_GEN);
    } else {
      Slot* slot = nullptr;
      bool existed = false;
      KeyState ks{0, 0, 0, 0};
      if (!table_claim(tab, v.key, v.ctrl >> 32, G, slot, existed, ks)) {
        atomicOr(&ctl->err, SNAP_ERR_FULL);
      } else if (existed) {
        atomicOr(&ctl->err, SNAP_ERR_DUP);
      } else {
        slot->key = v.key;
        write_state(slot, v.st);
        ok = true;
        cls = r * 2u + c;
      }
    }
  }
  count_classes(ok, cls, ctl);
}

// After k_snap_import of the same records (a kernel boundary: every claim and key of the chunk
// is visible): each record's identity must occur exactly once on its probe chain. Two equal
// records of one chunk can both claim a slot — the second sees the first one's claim word before
// its key — and are found here. The table was cleared by rl_restore_begin, so a chain ends at the
// first never-claimed slot; the walk is bounded by the region size.
__global__ __launch_bounds__(256) void k_snap_verify(const TableDesc tab, const Slot* __restrict__ recs, const uint32_t n,
                                                      SnapCtl* ctl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SlotView v = load_slot(recs + i);
  uint64_t rb;
  uint32_t lg;
  region_geom(tab, key_region(v.key), rb, lg);
  const uint64_t mask = (1ull << lg) - 1ull;
  const Slot* rbase = tab.slots + rb;
  uint64_t pos = (v.key << 3) >> (64 - lg);
  uint32_t found = 0;
  for (uint64_t probe = 0; probe <= mask; ++probe, ++pos) {
    const uint4 a = reinterpret_cast<const uint4*>(rbase + (pos & mask))[0];
    if (a.x == 0u) break;
    const uint64_t ctrl = (uint64_t)a.x | ((uint64_t)a.y << 32), key = (uint64_t)a.z | ((uint64_t)a.w << 32);
    found += ctrl == v.ctrl && key == v.key ? 1u : 0u;
  }
  if (found > 1u) atomicOr(&ctl->err, SNAP_ERR_DUP);
}

// Rehash (rl_resize): one pass from the old table straight into the new one, no record buffer in
// between. Source side as k_snap_export: a block takes tiles of TILE consecutive old slots, every
// lane reads PER slots with two 16-B loads each, all issued before the first use, and a slot is
// live by gen_class against its region's newest generation (lag regions keep gen - 2). Destination
// side as k_snap_import: the slot's place under the new geometry is slot_first of its key; a lane
// reads the first probe slot of each of its live slots ahead — up to PER random loads in flight
// together — and only then claims them one after another (table_claim_pre), so the random accesses
// overlap instead of chaining; then it writes key and state. A read-ahead may predate a claim of
// that slot (by another lane, or by this lane's earlier claim): table_claim_pre's CAS then fails
// and the slot is examined again with the word the CAS returned. The new table was zeroed and is
// below its load limit (rl_resize checks the mirror first), so a free slot exists in every region;
// a failed claim is SNAP_ERR_FULL. The source is a table, so identities are unique: finding one
// already in the new table is SNAP_ERR_DUP, and no k_snap_verify pass is needed — two lanes can
// only both claim a slot for the same identity, and there are no two such lanes. Per (region,
// class) counts of the slots moved are summed in LDS and added once per tile and non-zero word.
// No lane waits for another block: the tile loop is bounded by the old slot count, the probe by
// the new region's size.
__global__ __launch_bounds__(NT) void k_rehash(const TableDesc src, const uint64_t n_slots, const SnapGens gens,
                                                const TableDesc dst, SnapCtl* ctl) {
  __shared__ uint32_t sh_cls[SNAP_CLASSES];
  const uint32_t tid = threadIdx.x;
  const uint64_t n_tiles = (n_slots + TILE - 1) / TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (tid < (uint32_t)SNAP_CLASSES) sh_cls[tid] = 0u;
    __syncthreads();
    const uint64_t i0 = tile * TILE + tid;
    uint4 a[PER], b[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      a[k] = make_uint4(0u, 0u, 0u, 0u);
      b[k] = a[k];
      if (i < n_slots) {
        const uint4* p = reinterpret_cast<const uint4*>(src.slots + i);
        a[k] = p[0];
        b[k] = p[1];
      }
    }
    uint32_t cls[PER];  // region * 2 + class; SNAP_CLASSES = not live
    uint64_t key[PER];
    SlotView pre[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const uint64_t i = i0 + (uint64_t)k * NT;
      const uint32_t r = region_of_slot(src, i);
      const uint32_t c = i < n_slots ? gen_class(a[k].x, gen_of_region(gens, r), lazy_region(src.lag, r)) : 2u;
      key[k] = (uint64_t)a[k].z | ((uint64_t)a[k].w << 32);
      cls[k] = c < 2u ? r * 2u + c : (uint32_t)SNAP_CLASSES;
      if (c < 2u && key_region(key[k]) != r) {  // a slot outside its key's region: never written by this engine
        atomicOr(&ctl->err, SNAP_ERR_GEN);
        cls[k] = (uint32_t)SNAP_CLASSES;
      }
      // a lane without a live slot reads the table's first slot: no load behind a branch
      pre[k] = load_slot(cls[k] < (uint32_t)SNAP_CLASSES ? slot_first(dst, key[k]) : dst.slots);
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (cls[k] >= (uint32_t)SNAP_CLASSES) continue;
      Slot* slot = nullptr;
      bool existed = false;
      KeyState ks{0, 0, 0, 0};
      if (!table_claim_pre(dst, key[k], a[k].y, a[k].x, pre[k], slot, existed, ks)) {
        atomicOr(&ctl->err, SNAP_ERR_FULL);
      } else if (existed) {
        atomicOr(&ctl->err, SNAP_ERR_DUP);
      } else {
        slot->key = key[k];
        write_state(slot, KeyState{b[k].x, b[k].y, b[k].z, b[k].w});
        atomicAdd(&sh_cls[cls[k]], 1u);
      }
    }
    __syncthreads();
    if (tid < (uint32_t)SNAP_CLASSES && sh_cls[tid]) atomicAdd(&ctl->cnt[tid][0], sh_cls[tid]);
    __syncthreads();  // sh_cls is cleared by the next tile
  }
}

}  // namespace snap

void launch_rehash(hipStream_t st, const TableDesc& src, uint64_t n_slots, const SnapGens& gens, const TableDesc& dst,
                   SnapCtl* ctl) {
  const uint64_t tiles = (n_slots + snap::TILE - 1) / snap::TILE;
  const uint32_t grid = (uint32_t)(tiles < 1024 ? (tiles ? tiles : 1) : 1024);
  hipLaunchKernelGGL(snap::k_rehash, dim3(grid), dim3(snap::NT), 0, st, src, n_slots, gens, dst, ctl);
}

void launch_snap_export(hipStream_t st, const TableDesc& tab, uint64_t n_slots, const SnapGens& gens, Slot* out,
                        uint64_t cap, SnapCtl* ctl) {
  const uint64_t tiles = (n_slots + snap::TILE - 1) / snap::TILE;
  const uint32_t grid = (uint32_t)(tiles < 1024 ? (tiles ? tiles : 1) : 1024);
  hipLaunchKernelGGL(snap::k_snap_export, dim3(grid), dim3(snap::NT), 0, st, tab, n_slots, gens, out, cap, ctl);
}

void launch_snap_import(hipStream_t st, const TableDesc& tab, const Slot* recs, uint32_t n, const SnapGens& gens,
                        SnapCtl* ctl) {
  if (!n) return;
  const uint32_t grid = (n + 255u) / 256u;
  hipLaunchKernelGGL(snap::k_snap_import, dim3(grid), dim3(256), 0, st, tab, recs, n, gens, ctl);
  hipLaunchKernelGGL(snap::k_snap_verify, dim3(grid), dim3(256), 0, st, tab, recs, n, ctl);
}

}  // namespace rlhip
