// rl_set.hip — write counters by key (rl_hip.h "Set").
//   k_set_index  one lane per descriptor: the key string's identity (rl_peek.h key_ident, as k_peek),
//                what the descriptor's parts store (SetVal), and the string's entry in the call's
//                scratch index: one 64-bit CAS elects the string's leader, atomicMax per part
//                elects the last descriptor that writes it
//   k_set_plan   checks that every descriptor of an entry has the entry's identity; leaders look
//                their string up (no write) and count, per region, the slots the call would claim
//   k_set_apply  leaders claim (table_claim_pre, the pipelines' claim) or find their string's slot
//                and store the winning parts as separate 32-bit stores
// The table's claim is only safe when one lane claims a given identity (rl_decide.h
// table_claim_pre), which is what the index is for. Kernel boundaries order the three: no lane
// waits for another lane or block, and every loop is bounded by the prefix length (hash), the
// index size (insert) or the region size (probe).
#include <hip/hip_runtime.h>

#include "rl_peek.h"
#include "rl_set.h"
#include "rl_set_index.h"

namespace rlhip {
namespace set {

constexpr int NT = peek::NT;

// One add per wave and region on the region's own line (rl_decide.h count_inserts). Every lane of
// the wave calls it.
RL_DEV void count_regions(bool on, uint32_t region, uint32_t (*cnt)[64]) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = 0; r < 8; ++r) {
    const uint64_t m = __ballot(on && region == r);
    if (m && lane == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(&cnt[r][0], (uint32_t)__popcll(m));
  }
}

// The value is read beside the first level of rl_peek.h's desc_front; behind the front comes the
// index probe (rl_set_index.h set_index_tail, shared with k_set_index_routed).
__global__ __launch_bounds__(NT) void k_set_index(const DevBatch in, const DevRule* __restrict__ rules,
                                                  const uint32_t n_rules, const uint64_t seed, const TableDesc tab,
                                                  const rl_peek_reply* __restrict__ values, const SetScratch sc) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= in.n_desc) return;
  const rl_peek_reply v = values[i];
  const peek::DescFront f = peek::desc_front(in, rules, n_rules, i);
  const bool wc = !(v.flags & RL_SET_KEEP_COUNTER);
  const bool wf = !(v.flags & RL_SET_KEEP_CACHE) && tab.local_cache;
  SetDesc d;
  d.ent = SETD_NONE;
  d.tag = 0u;
  if (f.ok && (wc || wf)) {  // the host refused a malformed descriptor (and value) before the launch
    const FpState s = prefix_state_pre(f.w0, f.w1, in.blob, f.o0, f.len, seed);
    const peek::KeyIdent id = peek::key_ident(s, f.now, f.rr);
    d = set_index_tail(i, id, f.now, v, wc, wf, per_second_store(tab, f.rr.unit), sc);
  }
  sc.desc[i] = d;
}

// What a leader reads of its string: the entry, then (issued together) the up to three winning
// values at clamped indices and the key's first table slot.
struct Lead {
  uint64_t key;
  uint32_t tag, gen, region;
  bool wm, wp, wf, keeps;
  SetVal vm, vp, vf;
  SlotView pre;
};
RL_DEV Lead load_lead(const SetEntry* __restrict__ ep, const SetVal* __restrict__ val, const TableDesc& tab) {
  const uint4 a = reinterpret_cast<const uint4*>(ep)[0];
  const uint4 b = reinterpret_cast<const uint4*>(ep)[1];
  Lead L;
  L.key = ((uint64_t)a.x | ((uint64_t)a.y << 32)) - 1ull;
  L.tag = a.z;
  L.gen = a.w;
  L.region = key_region(L.key);
  L.wm = b.x != 0u;
  L.wp = b.y != 0u;
  L.wf = b.z != 0u;
  L.vm = val[L.wm ? b.x - 1u : 0u];  // winner words are descriptor indices + 1 <= n_desc
  L.vp = val[L.wp ? b.y - 1u : 0u];
  L.vf = val[L.wf ? b.z - 1u : 0u];
  L.pre = load_slot(slot_first(tab, L.key));
  L.keeps = (L.wm && L.vm.keeps) || (L.wp && L.vp.keeps) || (L.wf && L.vf.frz);
  return L;
}

__global__ __launch_bounds__(NT) void k_set_plan(const uint32_t n_desc, const TableDesc tab, const SetScratch sc) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  bool claims = false;
  uint32_t region = 0;
  if (i < n_desc) {
    const SetDesc d = sc.desc[i];
    if (d.ent != SETD_NONE) {
      const SetEntry* ep = sc.index + (d.ent & ~SETD_LEADER);
      if (d.ent & SETD_LEADER) {
        const Lead L = load_lead(ep, sc.val, tab);
        region = L.region;
        if (L.keeps) {
          Slot* slot = nullptr;
          KeyState st;
          claims = !table_find(tab, L.key, L.tag, L.gen, L.pre, slot, st);
        }
      } else if (ep->tag != d.tag) {
        // two identities met on one CAS word: the table keeps them apart, so must the call
        atomicOr(&sc.ctl->err, SET_ERR_MIXED);
      }
    }
  }
  count_regions(claims, region, sc.ctl->plan);
}

__global__ __launch_bounds__(NT) void k_set_apply(const uint32_t n_desc, const TableDesc tab, const SetScratch sc) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  bool claimed = false;
  uint32_t region = 0;
  if (i < n_desc) {
    const SetDesc d = sc.desc[i];
    if (d.ent != SETD_NONE && (d.ent & SETD_LEADER)) {
      const Lead L = load_lead(sc.index + (d.ent & ~SETD_LEADER), sc.val, tab);
      region = L.region;
      Slot* slot = nullptr;
      KeyState st;
      if (L.keeps) {
        bool existed = false;
        if (!table_claim_pre(tab, L.key, L.tag, L.gen, L.pre, slot, existed, st)) {
          atomicOr(&sc.ctl->err, SET_ERR_FULL);  // unreachable below the load limit
          slot = nullptr;
        } else if (!existed) {
          slot_reset(slot, L.key);
          claimed = true;
        }
      } else if (!table_find(tab, L.key, L.tag, L.gen, L.pre, slot, st)) {
        slot = nullptr;  // a DEL of an absent string: nothing is claimed
      }
      if (slot) {
        // one 32-bit store per word, as forget: only this lane writes this string in this launch
        if (L.wm) {
          slot->count = L.vm.count;
          slot->exp = L.vm.exp;
        }
        if (L.wp) slot->pcount = L.vp.count;
        if (L.wf) slot->frz = L.vf.frz;
      }
    }
  }
  count_regions(claimed, region, sc.ctl->claim);
}

}  // namespace set

void launch_set_index(hipStream_t st, const rl_batch& b, const DevRule* rules, uint32_t n_rules, uint64_t seed,
                      const TableDesc& tab, const rl_peek_reply* values, const SetScratch& sc) {
  if (!b.n_desc) return;
  const DevBatch in = make_dev_batch(b);
  const uint32_t grid = (b.n_desc + set::NT - 1u) / set::NT;
  hipLaunchKernelGGL(set::k_set_index, dim3(grid), dim3(set::NT), 0, st, in, rules, n_rules, seed, tab, values, sc);
}
void launch_set_plan(hipStream_t st, uint32_t n_desc, const TableDesc& tab, const SetScratch& sc) {
  if (!n_desc) return;
  hipLaunchKernelGGL(set::k_set_plan, dim3((n_desc + set::NT - 1u) / set::NT), dim3(set::NT), 0, st, n_desc, tab, sc);
}
void launch_set_apply(hipStream_t st, uint32_t n_desc, const TableDesc& tab, const SetScratch& sc) {
  if (!n_desc) return;
  hipLaunchKernelGGL(set::k_set_apply, dim3((n_desc + set::NT - 1u) / set::NT), dim3(set::NT), 0, st, n_desc, tab, sc);
}

}  // namespace rlhip
