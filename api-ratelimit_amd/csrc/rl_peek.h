// rl_peek.h — what the by-key kernels share, and the peek launchers.
//   desc_front / rec_front    the loads and checks a descriptor kernel (k_peek, k_set_index;
//                             k_adjust_index writes the same out) or a record kernel (the three
//                             *_routed forms) starts with
//   key_ident                 the key string's identity behind either front
//   peek_key / peek_key_slot  the lookup both peek kernels end in, one function so that the two
//                             cannot drift, and its sibling that also hands back the slot
//                             (rl_adjust.hip)
#pragma once
#include "rl_decide.h"

namespace rlhip {

// out: n_desc replies (peek; unused by the forget launch). Launches nothing for an empty batch.
void launch_peek(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                 const TableDesc& tab, rl_peek_reply* out, bool forget);
// The record form: n routed records (RRec); out: n replies (unused by the forget launch).
void launch_peek_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                        const TableDesc& tab, rl_peek_reply* out, bool forget);
// Origin: out[i] = back[perm[i]], or NIL where perm[i] is RL_ROUTE_LOCAL.
void launch_peek_unpack(hipStream_t st, uint32_t n, const uint32_t* perm, const rl_peek_reply* back,
                        rl_peek_reply* out);

namespace peek {

constexpr int NT = 256;

// The front of a descriptor kernel. The loads of a lane go out in three dependent levels, each
// issued as one run and waited for once (the kernels are latency-bound: random 32-B reads):
// (offsets, rule id, request index, and the caller's own per-descriptor word), then (now, the rule
// entry, the prefix's first 32 bytes), then the key's first table slot (behind `ok`, the caller's).
// Every load of the first two levels is unconditional at a clamped index (rl_tile.h load_descs):
// clamped reads stay inside the arrays (n_desc >= 1 in a launched kernel, n_req >= 1 and a rule
// table allocation exist, both host-checked) and inside the blob's RL_BLOB_SLACK readable bytes.
struct DescFront {
  bool ok, nil;      // ok: well-formed, with a rule and a time in [0, MAX_NOW]; nil: RL_NIL_RULE
  uint32_t now;      // the request time (when ok)
  uint32_t o0, len;  // the prefix in the blob (0, 0 unless the layout checks passed)
  DevRule rr;        // the rule entry (entry 0 for a bad id)
  u32x4 w0, w1;      // the prefix's first 32 bytes, from its 4-byte-aligned start
};
__device__ __forceinline__ DescFront desc_front(const DevBatch& in, const DevRule* __restrict__ rules,
                                                const uint32_t n_rules, const uint32_t i) {
  const uint32_t rl = in.rule[i];
  const uint32_t q = in.req_of[i];
  const uint32_t qp = in.req_of[i ? i - 1u : 0u];
  const uint32_t oa = in.off[i];
  const uint32_t ob = in.off[i + 1u];

  const bool nil = rl == RL_NIL_RULE;
  const bool rule_ok = rl < n_rules, q_ok = q < in.n_req;
  const bool lay = oa <= ob && ob <= in.blob_bytes && qp <= q;
  bool ok = !nil && rule_ok && q_ok && lay;
  const uint32_t o0 = ok ? oa : 0u, len = ok ? ob - oa : 0u;
  const int64_t now = in.now[q_ok ? q : 0u];
  const DevRule rr = rules[rule_ok ? rl : 0u];  // never indexed with a bad id
  const u32x4* p = reinterpret_cast<const u32x4*>(in.blob + (o0 & ~3u));
  const u32x4 w0 = p[0];
  const u32x4 w1 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint32_t*>(p) + 4);

  ok = ok && now >= 0 && now <= MAX_NOW;
  // One use of the level's other loads beside the time check: without it the compiler sinks the
  // rule and prefix loads behind the branch on `ok`, where they wait a round trip of their own.
  asm volatile("" ::"v"(rr.unit), "v"(rr.div), "v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y),
               "v"(w1.z), "v"(w1.w));
  return DescFront{ok, nil, (uint32_t)now, o0, len, rr, w0, w1};
}

// The front of a record kernel: the record (32 B), then the rule entry at a clamped id; the key's
// first table slot or the index probe is the caller's, behind `ok`. The identity comes from the
// record exactly as the owner's decision path takes it (rl_tile.h load_routed / key_of): the rule
// from the rule word, the window start from rec.now and the rule's unit, fp_final over the
// record's lanes: no prefix hashing, no blob. ok: the rule id is below n_rules (RL_NIL_RULE is
// not: a pack never sends one) and the time is not above MAX_NOW; a record that is not ok indexes
// nothing (the rule table holds >= 1 entry, host-checked). live: false for a thread that reads
// record i and uses nothing of it (it stays for a block sum). keep_word (the adjust form): the rule
// word is the rule id with RL_ADJUST_KEEP_CACHE in bit 16, and a bit above that is malformed.
struct RecFront {
  bool ok;
  RRec rc;
  DevRule rr;  // entry 0 for a bad id
};
__device__ __forceinline__ RecFront rec_front(const RRec* __restrict__ recs, const DevRule* __restrict__ rules,
                                              const uint32_t n_rules, const uint32_t i, const bool live,
                                              const bool keep_word) {
  RecFront f;
  f.rc = recs[i];
  const uint32_t rl = keep_word ? f.rc.rule & 0xFFFFu : rrec_rule(f.rc.rule);
  const bool rule_ok = !(keep_word && (f.rc.rule >> 17)) && rl < n_rules;
  f.rr = rules[rule_ok ? rl : 0u];  // never indexed with a bad id
  f.ok = live && rule_ok && (int64_t)f.rc.now <= MAX_NOW;
  // One use of the record's lanes and the rule entry ahead of the branch on `ok` (desc_front):
  // without it the compiler loads only the record's upper half first and fetches the lanes behind
  // the branch, a round trip of their own.
  asm volatile("" ::"v"(f.rc.a), "v"(f.rc.b), "v"(f.rr.unit), "v"(f.rr.div));
  return f;
}

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
