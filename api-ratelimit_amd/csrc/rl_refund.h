// rl_refund.h — what the engine (rl_engine.cpp) and the refund kernels (rl_refund.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "rl_adjust.h"

namespace rlhip {

// A refund's control block: an adjust's (the applying pass is k_adjust_apply's flight form, so the
// error word and its three counters are where that kernel puts them) and one word more on a line
// of its own. The index kernel's counters take the adjust names' places: ADJ_NIL counts the
// skipped descriptors, ADJ_ABSENT the owed ones whose counter was not found, ADJ_APPLIED the
// refunded ones. It lives in SetCtl's allocation, as AdjCtl does.
struct RefCtl {
  AdjCtl a;
  uint32_t rejected[64];  // rejected[0]: requests with an over-limit descriptor
};
static_assert(sizeof(RefCtl) <= sizeof(SetCtl), "the refund control block lives in rl_set's");
// beside rl_adjust.h's ADJ_ERR_*: the refunded batch's own error word was set, so its statuses were
// never written (the batch failed: table full, window span, spin limit, bad input); nothing ran
constexpr uint32_t ADJ_ERR_BATCH = 8u;

// A refund in flight (rl_engine.cpp adjust_queue): pass 0 is k_refund_mark, pass 1 k_refund_index;
// the applying pass is launch_adjust_flight's pass 1 over the same index. Every kernel reads the
// engine's poison word first. rej: n_req words, zeroed on the stream by the caller before pass 0,
// as are the index and the control block. st: the batch's n_desc statuses; amount: n_desc words, or
// nullptr. batch_err: the error word of the control block of the batch whose statuses these are
// (EngineCtl::err, complete once the batch's kernels ahead on the stream are done), or nullptr for
// statuses the caller vouches for. Launches nothing for n_desc == 0.
void launch_refund_flight(hipStream_t st_, const rl_batch& b, const rl_status* st, const DevRule* rules,
                          uint32_t n_rules, uint64_t seed, const TableDesc& tab, uint32_t* rej, uint32_t* amount,
                          const AdjScratch& sc, const uint32_t* poison, const uint32_t* batch_err, int pass);

// The origin side of a routed refund (rl_refund_routed.hip), behind the marking pass
// (launch_refund_flight's pass 0 over the same rej, with a poison word that reads 0 and no batch
// error word: only b.n_desc, b.n_req and b.req_of are read and the scratch view is not touched).
// k_refund_owed: amount[i] and rule_out[i] for every descriptor (rule_out may be b.rule_id), the
// rejected requests added to counts[0] and the owed descriptors to counts[1] (zeroed on the stream
// by the caller). Reads rule_id, req_of and hits_addend of the batch. Launches nothing for
// n_desc == 0.
void launch_refund_owed(hipStream_t st_, const rl_batch& b, const rl_status* st, const uint32_t* rej, uint32_t* rule_out,
                        uint32_t* amount, uint32_t* counts);
// The owner side: the record form of k_refund_index over n routed records (RRec) whose h word is
// the amount and whose rule word's bit 16 is RL_REFUND_KEEP_CACHE. out: n replies in device memory,
// or nullptr. The index and the control block (an AdjCtl) are zeroed on the stream by the caller
// first. A malformed record sets ADJ_ERR_BADREC and indexes nothing. Launches nothing for n == 0.
void launch_refund_index_routed(hipStream_t st, const RRec* recs, uint32_t n, const DevRule* rules, uint32_t n_rules,
                                const TableDesc& tab, rl_peek_reply* out, const AdjScratch& sc);

}  // namespace rlhip
