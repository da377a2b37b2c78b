// rl_set_index.h — the tail both index kernels end in (rl_set.hip k_set_index: from a descriptor;
// rl_set_routed.hip k_set_index_routed: from a routed record), one function so the two cannot
// drift: what the descriptor's parts store, the string's entry in the call's scratch index, the
// winner words.
#pragma once
#include "rl_peek.h"
#include "rl_set.h"

namespace rlhip {
namespace set {

// i: the descriptor's (record's) index in the call, the serial order "the last SET wins" is taken
// in. t: its request time; ps: its counter lives in the per-second store; wc / wf: it writes the
// counter / the cache entry (at least one). The sums t + ttl_s and t + cached_s are below 2^32
// (checked by the caller). Every read of the index probe is the CAS itself (it returns the word
// from the L2, never a line this CU cached before another lane's insert); the loop is bounded by
// the index size.
__device__ __forceinline__ SetDesc set_index_tail(const uint32_t i, const peek::KeyIdent& id, const uint32_t t,
                                                  const rl_peek_reply& v, const bool wc, const bool wf, const bool ps,
                                                  const SetScratch& sc) {
  SetDesc d;
  d.ent = SETD_NONE;
  d.tag = 0u;
  const bool found = (v.flags & RL_PEEK_FOUND) != 0;
  SetVal sv;
  sv.count = found ? v.count : 0u;
  sv.exp = found && !ps ? t + v.ttl_s : 0u;
  sv.frz = (v.flags & RL_PEEK_LOCAL_CACHED) ? t + v.cached_s : 0u;
  sv.keeps = (found && (!ps || v.count)) ? SETV_KEEPS : 0u;
  sc.val[i] = sv;

  const unsigned long long key1 = id.key + 1ull;
  const uint32_t lg = sc.log2_entries;
  const uint32_t mask = (1u << lg) - 1u;
  uint32_t pos = (uint32_t)((key1 * K0) >> (64 - lg));
  bool placed = false, leader = false;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long old = atomicCAS(&sc.index[pos].key1, 0ull, key1);
    if (old == 0ull || old == key1) {
      placed = true;
      leader = old == 0ull;
      break;
    }
    pos = (pos + 1u) & mask;
  }
  if (!placed) {
    atomicOr(&sc.ctl->err, SET_ERR_INDEX);
  } else {
    SetEntry* e = sc.index + pos;
    if (leader) {
      e->tag = (uint32_t)id.lo;
      e->gen = id.pl.gen;
    }
    if (wc) atomicMax(ps ? &e->win_ps : &e->win_main, i + 1u);
    if (wf) atomicMax(&e->win_cache, i + 1u);
    d.ent = pos | (leader ? SETD_LEADER : 0u);
    d.tag = (uint32_t)id.lo;
  }
  return d;
}

}  // namespace set
}  // namespace rlhip
