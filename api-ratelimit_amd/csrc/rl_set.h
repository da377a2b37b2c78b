// rl_set.h — what the engine (rl_engine.cpp) and the set kernels (rl_set.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_common.h"

namespace rlhip {

// One entry of the call's scratch index (32 B): one key string of the call. key1 is the claim word
// (sort key + 1, so 0 = empty: NIL_KEY is never a sort key), taken with a 64-bit CAS; tag and gen
// are stored beside it by the lane whose CAS inserted the entry (the string's leader) and read
// only by the kernels behind k_set_index. The winner words hold, per part, the largest descriptor
// index + 1 that writes the part (atomicMax; 0 = no descriptor of the call writes it).
struct __attribute__((aligned(32))) SetEntry {
  unsigned long long key1;
  uint32_t tag, gen;
  uint32_t win_main, win_ps, win_cache;
  uint32_t pad;
};
static_assert(sizeof(SetEntry) == 32, "SetEntry is 32 B");

// Per descriptor, written by k_set_index (16 B): what its parts store, as absolute seconds.
struct __attribute__((aligned(16))) SetVal {
  uint32_t count;  // the counter (0: DEL)
  uint32_t exp;    // main store: t + ttl_s (0: DEL)
  uint32_t frz;    // t + cached_s (0: no cache entry)
  uint32_t keeps;  // SETV_KEEPS: the counter part leaves something in the slot
};
constexpr uint32_t SETV_KEEPS = 1u;
// Per descriptor (8 B): its index entry | SETD_LEADER, or SETD_NONE (writes nothing); its tag.
struct __attribute__((aligned(8))) SetDesc {
  uint32_t ent, tag;
};
constexpr uint32_t SETD_LEADER = 0x80000000u, SETD_NONE = 0xFFFFFFFFu;
constexpr uint32_t SET_MAX_DESC = 1u << 29;  // the index (2^k >= 2 n entries) is addressed in 31 bits

// Control block of one call, zeroed at its start. As in EngineCtl and SnapCtl, every word that
// more than one block adds to lives on a 256-B line of its own.
struct SetCtl {
  uint32_t err;         // SET_ERR_*, atomicOr, only on an error
  uint32_t pad0[63];
  uint32_t plan[8][64];   // k_set_plan: strings per region that the call would claim a slot for
  uint32_t claim[8][64];  // k_set_apply: slots per region it claimed
  // k_set_index_routed: per region, over the records that write something, the largest window
  // generation and the largest complement of one (~smallest; both atomicMax, so zero = none)
  uint32_t gen_max[8][64];
  uint32_t gen_minc[8][64];
};
static_assert(sizeof(SetCtl) == 33 * 256, "SetCtl layout");
enum : uint32_t {
  SET_ERR_INDEX = 1u,  // the index had no entry left for a string (unreachable: 2^k >= 2 n)
  SET_ERR_MIXED = 2u,  // two identities share one 64-bit sort key in this call: split the call
  SET_ERR_FULL = 4u,   // no free slot in a region (unreachable below the load limit)
  // the record form only (the host form's host checks refuse these before any launch):
  SET_ERR_BADREC = 8u,   // a record's rule id is not below n_rules, or its time is above MAX_NOW
  SET_ERR_BADVAL = 16u,  // a part the record writes: ttl_s / cached_s zero, or its sum with the time not below 2^32
};

struct SetScratch {
  SetEntry* index;
  uint32_t log2_entries;
  SetVal* val;
  SetDesc* desc;
  SetCtl* ctl;
};

// values: n_desc rl_peek_reply in device memory. The index (2^log2_entries entries) and the
// control block are zeroed on the stream by the caller before launch_set_index.
void launch_set_index(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                      const TableDesc& tab, const rl_peek_reply* values, const SetScratch& sc);
// The record form (rl_set_routed.hip): n routed records (RRec) with one value each beside them.
void launch_set_index_routed(hipStream_t st, const RRec* recs, const rl_peek_reply* values, uint32_t n,
                             const DevRule* rules, uint32_t n_rules, const TableDesc& tab, const SetScratch& sc);
// Origin: vsend[perm[i]] = values[i] for every descriptor the pack gave a record (perm: its strided
// form, below cap = the records vsend has room for).
void launch_set_values_pack(hipStream_t st, uint32_t n, uint32_t cap, const uint32_t* perm, const rl_peek_reply* values,
                            rl_peek_reply* vsend);
void launch_set_plan(hipStream_t st, uint32_t n_desc, const TableDesc& tab, const SetScratch& sc);
void launch_set_apply(hipStream_t st, uint32_t n_desc, const TableDesc& tab, const SetScratch& sc);

}  // namespace rlhip
