// rl_refund_key.h — the device code both refund index kernels end in (rl_refund.hip k_refund_index:
// from a descriptor; rl_refund_routed.hip k_refund_index_routed: from a routed record), one function
// so the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_adjust_key.h"
#include "rl_refund.h"

namespace rlhip {
namespace refund {

constexpr int NT = adjust::NT;

// One pair's sum into the call's index: adjust_key's insert (rl_adjust_key.h), with the wave's sum
// and limit complement for one descriptor's. The amounts leave as a negative 64-bit net. n_rel is
// added to the entry's count when it is not 0: only the record form's applying pass reads the count
// (k_adjust_apply PER_KEY: the pair's found records that came without the keep bit), so the flight
// form passes 0, and on a hot key every atomic here is one more turn at a single L2 address.
RL_DEV void index_add(const unsigned long long pair, const unsigned long long sum, const uint32_t lim_c,
                      const uint32_t n_rel, const AdjScratch& sc) {
  const uint32_t lg = sc.log2_entries;
  const uint32_t mask = (1u << lg) - 1u;
  uint32_t pos = (uint32_t)((pair * K0) >> (64 - lg));
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long old = atomicCAS(&sc.index[pos].pair, 0ull, pair);
    if (old == 0ull || old == pair) {
      AdjEntry* e = sc.index + pos;
      atomicAdd(reinterpret_cast<unsigned long long*>(&e->net), 0ull - sum);
      atomicMax(&e->lim_c, lim_c);
      if (n_rel) atomicAdd(&e->n, n_rel);
      return;
    }
    pos = (pos + 1u) & mask;
  }
  atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_INDEX);
}

RL_DEV unsigned long long shfl64(const unsigned long long v, const int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

}  // namespace refund
}  // namespace rlhip
