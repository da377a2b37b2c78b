// rl_peek.h — the lookup both peek kernels end in (rl_peek.hip k_peek: from a descriptor;
// rl_peek_routed.hip k_peek_routed: from a routed record), one function so the two cannot drift,
// and the key identity it starts from, which rl_set.hip shares; and that lookup's sibling that
// also hands back the slot (rl_adjust.hip).
#pragma once
#include "rl_decide.h"

namespace rlhip {
namespace peek {

constexpr int NT = 256;

// A key string's identity from its prefix state, its request time and its rule: the window start,
// the table place (region, window generation), the sort key and the fingerprint's low lane (the
// slot's tag). One function for every by-key entry point (peek, forget, rl_set.hip's set).
struct KeyIdent {
  uint32_t ws;
  Place pl;
  uint64_t key, lo;
};
__device__ __forceinline__ KeyIdent key_ident(const FpState& s, const uint32_t n32, const DevRule& rr) {
  // now / divider by 32-bit multiply-high (rl_tile.h key_of: exact for every 32-bit now)
  const uint32_t q60 = __umulhi(n32, 0x88888889u) >> 5, q3600 = __umulhi(n32, 0x91A2B3C5u) >> 11,
                 q86400 = __umulhi(n32 >> 7, 0xC22E4507u) >> 9;
  const uint32_t unit = rr.unit;
  const uint32_t widx = unit == RL_UNIT_SECOND ? n32 : unit == RL_UNIT_MINUTE ? q60 : unit == RL_UNIT_HOUR ? q3600 : q86400;
  KeyIdent k;
  k.ws = widx * rr.div;  // (now/divider)*divider  cache_key.go:66-68
  uint64_t hi;
  fp_final(s, (uint64_t)k.ws, hi, k.lo);
  k.pl = place_of(k.ws);
  k.key = make_sort_key(k.pl.region, hi);
  return k;
}

// From a key's prefix state, its request time (in [0, MAX_NOW], checked by the caller) and its
// rule: the window start, the key string's identity and table place, the lookup (issued first:
// the key's first slot, then table_find's bounded probe), the store choice, and the reply
// (!FORGET: rep with its words filled in) or the clears (FORGET: separate 32-bit stores, rep as
// it came). The reply goes in and out by value: by reference k_peek compiled to a longer probe
// loop and measured 1 % slower than before the function existed ("Peek").
template <bool FORGET>
__device__ __forceinline__ rl_peek_reply peek_key(const FpState& s, const uint32_t n32, const DevRule& rr,
                                                  const TableDesc& tab, rl_peek_reply rep) {
  const KeyIdent id = key_ident(s, n32, rr);
  const uint32_t unit = rr.unit;
  const Place pl = id.pl;
  const uint64_t key = id.key, lo = id.lo;
  const SlotView pre = load_slot(slot_first(tab, key));
  Slot* slot = nullptr;
  KeyState st{0, 0, 0, 0};
  const bool have = table_find(tab, key, lo, pl.gen, pre, slot, st);
  const bool ps = per_second_store(tab, unit);
  if (!FORGET) {
    rep.flags = ps ? RL_PEEK_PER_SECOND : 0u;
    if (have) {
      if (ps) {
        if (st.pcount) {
          rep.flags |= RL_PEEK_FOUND;
          rep.count = st.pcount;
        }
      } else if (n32 < st.exp) {
        rep.flags |= RL_PEEK_FOUND;
        rep.count = st.count;
        rep.ttl_s = st.exp - n32;
      }
      if (tab.local_cache && n32 < st.frz) {
        rep.flags |= RL_PEEK_LOCAL_CACHED;
        rep.cached_s = st.frz - n32;
      }
    }
  } else if (have) {
    // DEL on the descriptor's store, and the string leaves the local cache. One 32-bit store
    // per word: another lane of this launch may be clearing the other store of this slot. The
    // claim word and the key stay: the slot remains the string's for its generation (open
    // addressing without tombstones), and the next INCRBY starts from 0.
    if (ps) {
      slot->pcount = 0u;
    } else {
      slot->count = 0u;
      slot->exp = 0u;
    }
    slot->frz = 0u;
  }
  return rep;
}

// peek_key<false>'s lookup and reply for a caller that then writes the counter it found
// (rl_adjust.hip): `found` is the string's slot when the reply says RL_PEEK_FOUND and nullptr
// otherwise, ps the descriptor's store. A sibling rather than a parameter of peek_key: k_peek was
// measured sensitive to that function's shape.
__device__ __forceinline__ rl_peek_reply peek_key_slot(const FpState& s, const uint32_t n32, const DevRule& rr,
                                                       const TableDesc& tab, rl_peek_reply rep, Slot*& found,
                                                       bool& ps) {
  const KeyIdent id = key_ident(s, n32, rr);
  const SlotView pre = load_slot(slot_first(tab, id.key));
  Slot* slot = nullptr;
  KeyState st{0, 0, 0, 0};
  const bool have = table_find(tab, id.key, id.lo, id.pl.gen, pre, slot, st);
  ps = per_second_store(tab, rr.unit);
  found = nullptr;
  rep.flags = ps ? RL_PEEK_PER_SECOND : 0u;
  if (have) {
    if (ps) {
      if (st.pcount) {
        rep.flags |= RL_PEEK_FOUND;
        rep.count = st.pcount;
        found = slot;
      }
    } else if (n32 < st.exp) {
      rep.flags |= RL_PEEK_FOUND;
      rep.count = st.count;
      rep.ttl_s = st.exp - n32;
      found = slot;
    }
    if (tab.local_cache && n32 < st.frz) {
      rep.flags |= RL_PEEK_LOCAL_CACHED;
      rep.cached_s = st.frz - n32;
    }
  }
  return rep;
}

}  // namespace peek
}  // namespace rlhip
