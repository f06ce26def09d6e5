// Lane-group family: fused T-step rollout kernel and its launcher (device code: mapf_lg.hpp; the launch's plan: mapf_plan.hip).
#include "mapf_lg.hpp"
#include "mapf_plan.hpp"

#include <type_traits>

namespace mapf {

// MV_LDS: the whole move table (V*6 entries of 16 B) is staged into LDS once per block and the two gathers of
// every step become ds_read_b128 (a random 64-lane gather through the vector-memory pipe touches up to 64 cache
// lines).  RECORD: all five trajectory arrays are written every step (the C ABI substitutes scratch for absent
// ones), STREAM: actions come from memory, else from the in-kernel policy stream.  Both are compile-time so the
// loop body has no uniform branches around its memory operations.  DENSE (A == 2L and the env count fills every
// block) additionally removes the per-lane predicates: every lane owns two real agents, the action prefetch is
// clamped instead of guarded, and the four per-env scalars are stored by ALL lanes with per-lane addresses (even
// lanes of a group write done, odd lanes collision, the last lane prob, the others reward -- duplicates carry
// identical data), so the
// loop contains no exec-masked memory operation and the compiler can wait for the prefetched action word with a
// counted vmcnt(N) instead of draining every store.  Start cells stay in two registers per lane, so an
// auto-reset touches no memory.
#define MAPF_ROLLOUT_TABLE_KERNEL 0
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL

// Launches the planned instance of lg_rollout_kernel, or of lg_rollout_kernel_table (TABLE: then STREAM is false): (MV_LDS,
// DENSE) pick the kernel, the plan gives its geometry and its LDS segment (the move table, or nothing).
template <int L, bool FULL, bool RECORD, bool STREAM, bool TABLE>
static hipError_t launch_instance(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table) {
    auto pick = [&](auto mv_lds) {   // (DENSE exists for full groups only)
        constexpr bool MV_LDS = decltype(mv_lds)::value;
        if constexpr (TABLE) return plan.dense ? lg_rollout_kernel_table<L, FULL, MV_LDS, RECORD, FULL> : lg_rollout_kernel_table<L, FULL, MV_LDS, RECORD, false>;
        else return plan.dense ? lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, FULL> : lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false>;
    };
    const auto kern = plan.mv_lds ? pick(std::true_type{}) : pick(std::false_type{});
    if (plan.lds_bytes > 32 * 1024) {
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes - kLdsReserve))) return e;
    }
    char name[kKernelNameBytes];
    lg_rollout_kernel_name(name, plan, RECORD, STREAM, TABLE);
    note_kernel("%s", name);
    if constexpr (TABLE) hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, args, A, *table);
    else hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, args, A);
    return hipGetLastError();
}

// the instance's other arguments: the plan's L and FULL, RECORD and STREAM from the arrays the launch names (under TABLE no launch
// streams its actions, and both arms of P name the one table instance)
template <bool TABLE>
static hipError_t launch_planned(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table) {
    const bool record = args.rec_local != nullptr, streamed = !TABLE && args.actions != nullptr;
    switch (plan.L) {
#define P(N, FULL, RECORD) (streamed ? launch_instance<N, FULL, RECORD, !TABLE, TABLE>(plan, args, A, stream, table)  \
                                     : launch_instance<N, FULL, RECORD, false, TABLE>(plan, args, A, stream, table))
#define X(N)                                                                                                         \
    case N:                                                                                                          \
        if (plan.full) return record ? P(N, true, true) : P(N, true, false);                                         \
        return record ? P(N, false, true) : P(N, false, false);
        MAPF_FOR_EACH_L(X)
#undef X
#undef P
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rollout_lg(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, const TablePolicy *table,
                             const EpisodeLimit *limit) {
    if (args.n_envs == 0) return hipSuccess;
    if (limit) return launch_rollout_lg_limit(n_agents, args, tune, stream, table, *limit);   // (before any packed plan is consulted)
    hipError_t packed_status;
    if (try_launch_rollout_lq(n_agents, args, tune, stream, &packed_status, table)) return packed_status;
    const LgRolloutPlan plan = plan_rollout_lg(n_agents, args, tune);
    return table ? launch_planned<true>(plan, args, uint32_t(n_agents), stream, table) : launch_planned<false>(plan, args, uint32_t(n_agents), stream, table);
}

}  // namespace mapf
