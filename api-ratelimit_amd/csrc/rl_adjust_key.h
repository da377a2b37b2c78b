// rl_adjust_key.h — the device code both adjust index kernels end in (rl_adjust.hip k_adjust_index:
// from a descriptor; rl_adjust_routed.hip k_adjust_index_routed: from a routed record), one function
// so the two cannot drift, and the block sum every adjust kernel closes with.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_adjust.h"
#include "rl_peek.h"

namespace rlhip {
namespace adjust {

constexpr int NT = peek::NT;

// Three flags summed over the block: a ballot per wave, the wave sums through LDS, then one add
// per word and block on the word's own line. Every thread of the block calls it.
RL_DEV void block_add3(const bool a, const bool b, const bool c, const int wa, const int wb, const int wc,
                       AdjCtl* ctl) {
  __shared__ uint32_t sh[NT / 64][3];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t ca = (uint32_t)__popcll(__ballot(a)), cb = (uint32_t)__popcll(__ballot(b)),
                 cc = (uint32_t)__popcll(__ballot(c));
  if (lane == 0u) {
    sh[wave][0] = ca;
    sh[wave][1] = cb;
    sh[wave][2] = cc;
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    uint32_t sum = 0;
    for (int w = 0; w < NT / 64; ++w) sum += sh[w][threadIdx.x];
    const int word = threadIdx.x == 0u ? wa : threadIdx.x == 1u ? wb : wc;
    if (sum) atomicAdd(&ctl->w[word][0], sum);
  }
}

// The lookup-and-accumulate step of one key: from its prefix state, its time t (in [0, MAX_NOW],
// checked by the caller), its rule and its delta. rep goes in and out by value, as in peek_key.
// Returns true when the counter was found (the delta entered its pair's sum). Every read of the
// index probe is the CAS itself (rl_set_index.h: it returns the word from the L2).
// PER_KEY (the record form): the release of the local cache is decided per record; release says
// that this one came without RL_ADJUST_KEEP_CACHE, and the entry's count then counts only those,
// so that n != 0 is "some found record of the pair did". (A pad word or-ed beside the count, a
// fourth atomic per found record, measured 1.19x k_adjust_index at 10^6 records, DESIGN.md §6
// "Routed adjust"; this way the record form issues the host form's three, or two.) The host
// form decides it per call and counts every descriptor.
template <bool PER_KEY>
RL_DEV bool adjust_key(const FpState& s, const uint32_t t, const DevRule& rr, const int32_t delta, const bool release,
                       const TableDesc& tab, const AdjScratch& sc, rl_peek_reply& rep) {
  Slot* slot = nullptr;
  bool ps = false;
  rep = peek::peek_key_slot(s, t, rr, tab, rep, slot, ps);
  if (!slot) return false;
  const unsigned long long pair = (unsigned long long)reinterpret_cast<uintptr_t>(slot) | (ps ? ADJ_PS : 0ull);
  const uint32_t lg = sc.log2_entries;
  const uint32_t mask = (1u << lg) - 1u;
  uint32_t pos = (uint32_t)((pair * K0) >> (64 - lg));
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long old = atomicCAS(&sc.index[pos].pair, 0ull, pair);
    if (old == 0ull || old == pair) {
      AdjEntry* e = sc.index + pos;
      if (delta) atomicAdd(reinterpret_cast<unsigned long long*>(&e->net), (unsigned long long)(long long)delta);
      atomicMax(&e->lim_c, ~rr.L);
      if (!PER_KEY || release) atomicAdd(&e->n, 1u);
      return true;
    }
    pos = (pos + 1u) & mask;
  }
  atomicOr(&sc.ctl->w[ADJ_ERR][0], ADJ_ERR_INDEX);
  return true;
}

}  // namespace adjust
}  // namespace rlhip
