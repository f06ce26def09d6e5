// Packed family: the launcher of its fused rollout kernels, once for every family of instances.  The launcher takes ONE plan
// (mapf_plan.hpp) and launches the instance it names; which kernels those instances are is the including unit's say, through a
// family type:
//   Family::kernel<Q, K, RECORD, STREAM, SOC, COMPACT, TERM, BITMAP, TABLE>() returns the address of an instance of
//       lq_rollout_kernel (mapf_lq_rollout_kernel.hpp).  mapf_lq_rollout.hip: the plain instances, whose TABLE is 0, and the table
//       instances, whose STREAM is false; mapf_lq_limit.hip: the table instances under an episode step limit;
//   Family::kTable -- the instances follow the table policy: MAPF_LQ_ROLLOUT_TABLE_INSTANCES, built for 512 threads, TABLE = 1
//       (action bytes gathered from global memory) or 2 (staged into LDS); Family::kLimit -- ... under an episode step limit.
// The kernels' arguments are (args, A, where the bitmaps begin[, the table policy, where its LDS copy begins[, extra...]]): the
// launcher forms all but `extra`, which is nothing or the episode limit.
#pragma once
#include "mapf_lq.hpp"
#include "mapf_plan.hpp"

#include <type_traits>

namespace mapf {

// Launches the planned instance: FORM's traits (mapf_layout.hpp) give the kernel's (COMPACT, BITMAP); the launch's criteria and
// may-be-terminal pick among (SOC, TERM) -- the instance without terminal handling exists for Makespan only -- and the plan's
// table_lds among TABLE; the plan gives the block, where the bitmaps begin (lds_bytes), the launch's dynamic LDS segment
// (lds_total) and the name the launch notes.
template <class Family, int Q, int K, bool RECORD, bool STREAM, TableForm FORM, class... Extra>
hipError_t launch_lq_rollout_instance(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table, const Extra &...extra) {
    constexpr TableFormTraits form = table_form_traits(FORM);
    constexpr bool COMPACT = form.compact; constexpr int BITMAP = form.bitmap;   // the kernel's template arguments
    const bool soc = args.c.criteria != 0u, term = rollout_may_be_terminal(args);
    auto pick = [&](auto tag) {
        constexpr int T = decltype(tag)::value;
        // (in this order the kernels keep their places in the objects' device code)
        return !soc ? (term ? Family::template kernel<Q, K, RECORD, STREAM, false, COMPACT, true, BITMAP, T>()
                            : Family::template kernel<Q, K, RECORD, STREAM, false, COMPACT, false, BITMAP, T>())
                    : Family::template kernel<Q, K, RECORD, STREAM, true, COMPACT, true, BITMAP, T>();
    };
    auto kern = plan.table_lds ? pick(std::integral_constant<int, 2>{}) : pick(std::integral_constant<int, 1>{});   // (no table: one kernel)
    if (Family::kTable && (!table || plan.lds_total > kLdsBytes || plan.block > 512u)) return hipErrorInvalidValue;   // (the table instances are built for 512 threads)
    if (plan.lds_total > 32 * 1024) {
        // (these kernels have no static LDS object: the dynamic segment may be the CU's whole 160 KB -- the limit every form's
        // "does it fit" test in plan_rollout_lq compares against)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    char name[kKernelNameBytes];
    lq_rollout_kernel_name(name, plan, RECORD, STREAM, Family::kTable, soc, term, table ? table->table_bytes : 0u);
    note_kernel(name);
    const dim3 grid(unsigned(args.n_envs / (plan.block / unsigned(Q)))), block(plan.block);
    if constexpr (Family::kTable) {   // (the bitmaps follow the table image, the policy table's LDS copy follows them at table_at)
        hipLaunchKernelGGL(kern, grid, block, plan.lds_total, stream, args, A, uint32_t(plan.lds_bytes), *table, plan.table_at, extra...);
    } else {
        hipLaunchKernelGGL(kern, grid, block, plan.lds_total, stream, args, A, uint32_t(plan.lds_bytes));
    }
    return hipGetLastError();
}

// The instances of one object -- K agents per lane, recording or not -- by the family's list in mapf_layout.hpp (what
// lq_rollout_instance_exists answers from), in the list's order: a launch whose (Q, form) is in none of this K's lines is refused.
// (The lines of the other K's are discarded, not instantiated.  A table family has no STREAM: both arms name its one instance.)
template <class Family, int K, bool RECORD, class... Extra>
hipError_t launch_lq_rollout(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table, const Extra &...extra) {
    if (plan.limit != Family::kLimit) return hipErrorInvalidValue;   // (the plan names the other family)
    const bool streamed = !Family::kTable && args.actions != nullptr;
#define X(KK, QQ, FF)                                                                                                                                    \
    if constexpr (KK == K) {                                                                                                                             \
        if (plan.Q == QQ && plan.form == TableForm::FF)                                                                                                  \
            return streamed ? launch_lq_rollout_instance<Family, QQ, K, RECORD, !Family::kTable, TableForm::FF>(plan, args, A, stream, table, extra...)  \
                            : launch_lq_rollout_instance<Family, QQ, K, RECORD, false, TableForm::FF>(plan, args, A, stream, table, extra...);           \
    }
    if constexpr (Family::kTable) { MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X) } else { MAPF_LQ_ROLLOUT_INSTANCES(X) }
#undef X
    return hipErrorInvalidValue;
}

// A unit of this family is compiled once per (agents per lane, recording) pair -- -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0 -- so that its
// kernel instances build in parallel; each object exports ONE launcher, MAPF_LQ_LAUNCHER(prefix) { body over K, RECORD and the
// arguments }: <prefix><K>_r<RECORD>, all of one signature (prototypes: mapf_kernels.hpp; the router: mapf_dispatch.hip).
#if !defined(MAPF_LQ_K) || !defined(MAPF_LQ_RECORD)
#error "compile with -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0"
#endif
#define MAPF_LQ_CAT3(a, b, c) a##b##_r##c
#define MAPF_LQ_NAME(prefix, k, r) MAPF_LQ_CAT3(prefix, k, r)
#define MAPF_LQ_LAUNCHER(prefix)                                                                                                                         \
    hipError_t MAPF_LQ_NAME(prefix, MAPF_LQ_K, MAPF_LQ_RECORD)(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream,               \
                                                               const TablePolicy *table, const EpisodeLimit *limit)
constexpr int kLqK = MAPF_LQ_K;
constexpr bool kLqRecord = MAPF_LQ_RECORD != 0;

}  // namespace mapf
