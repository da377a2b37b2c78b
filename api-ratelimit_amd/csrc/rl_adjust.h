// rl_adjust.h — what the engine (rl_engine.cpp) and the adjust kernels (rl_adjust.hip,
// rl_adjust_routed.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_common.h"
#include "rl_set.h"

namespace rlhip {

// One entry of the call's scratch index (32 B): one (string, store) pair of the call whose counter
// was found. pair is the claim word, taken with a 64-bit CAS: the slot's address with the store in
// its lowest bit (slots are 32-B aligned, so 0 = empty). Only found slots enter, so the address is
// the identity: no tag to compare, and two identities never meet on one word. The other words are
// summed over the pair's found descriptors by k_adjust_index and read by k_adjust_apply.
struct __attribute__((aligned(32))) AdjEntry {
  unsigned long long pair;  // (uintptr_t)Slot* | ADJ_PS
  long long net;            // sum of the deltas (atomicAdd)
  uint32_t lim_c;           // ~(the smallest requests_per_unit): the minimum as an atomicMax, so that
                            // the zeroed entry is "none"
  uint32_t n;               // descriptors of the pair; the record form: those that came without
                            // RL_ADJUST_KEEP_CACHE (non-zero: the pair's cache part may run)
  uint32_t pad[2];
};
static_assert(sizeof(AdjEntry) == sizeof(SetEntry), "the adjust index lives in rl_set's index allocation");
constexpr unsigned long long ADJ_PS = 1ull;

// Control block of one call, zeroed at its start: every word is added to by more than one block,
// so each owns a 256-B line (the SetCtl / EngineCtl rule). It lives in SetCtl's allocation.
enum : int { ADJ_ERR, ADJ_NIL, ADJ_ABSENT, ADJ_APPLIED, ADJ_FLOORED, ADJ_CAPPED, ADJ_UNFROZEN, ADJ_WORDS };
struct AdjCtl {
  uint32_t w[ADJ_WORDS][64];  // w[k][0] is the word
};
static_assert(sizeof(AdjCtl) <= sizeof(SetCtl), "the adjust control block lives in rl_set's");
constexpr uint32_t ADJ_ERR_INDEX = 1u;  // the index had no entry left for a pair (unreachable: 2^k >= 2 n)
constexpr uint32_t ADJ_ERR_BADREC = 2u;  // the record form: a malformed record (rule id, time or rule word's upper bits);
                                         // a flight: a malformed descriptor of a device batch
constexpr uint32_t ADJ_ERR_POISON = 4u;  // a flight behind a batch the engine reruns: nothing ran, the engine runs it again

struct AdjScratch {
  AdjEntry* index;
  uint32_t log2_entries;
  AdjCtl* ctl;
};

// delta: n_desc words in device memory; out: n_desc replies in device memory, or nullptr. The index
// (2^log2_entries entries) and the control block are zeroed on the stream by the caller first.
void launch_adjust_index(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                         const TableDesc& tab, const int32_t* delta, rl_peek_reply* out, const AdjScratch& sc);
// clear_cache: the call's cache part is on (the local cache is on and RL_ADJUST_KEEP_CACHE is not set).
// per_key: a pair's cache part also needs its entry's count to be non-zero (a routed plan's commit).
void launch_adjust_apply(hipStream_t st, bool clear_cache, bool per_key, const AdjScratch& sc);

// An adjust in flight (rl_engine.cpp adjust_queue): pass 0 is the index kernel, pass 1 the applying
// one, both in the form that reads the engine's poison word first (rl_adjust.hip FLIGHT). Launches
// nothing for n_desc == 0.
void launch_adjust_flight(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                          const TableDesc& tab, const int32_t* delta, rl_peek_reply* out, bool clear_cache,
                          const AdjScratch& sc, const uint32_t* poison, int pass);

// The record form (rl_adjust_routed.hip): n routed records (RRec) whose h word is the delta and
// whose rule word's bit 16 is RL_ADJUST_KEEP_CACHE. out: n replies in device memory, or nullptr.
// A malformed record sets ADJ_ERR_BADREC and indexes nothing. Launches nothing for n == 0.
void launch_adjust_index_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                                const TableDesc& tab, rl_peek_reply* out, const AdjScratch& sc);
// Origin: descriptor i's delta and the call's keep bit into its record's h and rule words (perm:
// the strided form of the plain pack, or RL_ROUTE_LOCAL; cap: the records send has room for).
void launch_adjust_pack(hipStream_t st, uint32_t n, uint32_t cap, const uint32_t* perm, const uint32_t* rule_id,
                        const int32_t* delta, uint32_t keep, RRec* send);

}  // namespace rlhip
