// Packed table-policy rollout under an episode step limit (include/mapf_hip.h mapf_set_episode_limit; EpisodeLimit in
// mapf_kernels.hpp): lq_rollout_kernel_table_limit, the limit form of lq_rollout_kernel_table (mapf_lq_rollout.hip), and its
// launcher.  A translation unit of its own: the packed kernels that exist without the limit keep their code.  Reached only with
// MAPF_TUNE limit_packed=1 (mapf_capi.hip rollout_impl); every launch this family declines -- and every launch under a limit
// without the key -- is the lane-group limit instance's (mapf_lg_limit.hip).
//
// The four rules of the limit are mapf_lg_limit.hip's.  In the packed body they hang on the group-uniform code of the step
// (code16, from which every select of the reset logic is derived): a live step ended its episode exactly when code16 != 4 * 16,
// so `truncated` needs no outcome row.  Nothing else of a step changes: reward, prob, done, collision, the totals and every
// Philox counter are those of lq_rollout_kernel_table.
//
// Only the table instances have a limit form: built for 512 threads they have 256 vector registers per lane and use at most
// 122; the streamed and in-kernel-policy instances sit at 128 of 128 in their 1024-thread forms.
#include "mapf_lq.hpp"
#include "mapf_plan.hpp"

#include <type_traits>

namespace mapf {

namespace {

#define MAPF_ROLLOUT_LIMIT 1
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lq_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#undef MAPF_ROLLOUT_LIMIT

#undef env_id

// launch_impl_table's twin (mapf_lq_rollout.hip): the same instance choice, geometry and name, plus the limit
template <int Q, int K, bool RECORD, TableForm FORM>
hipError_t launch_impl_table_limit(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy &tp, const EpisodeLimit &lim) {
    constexpr TableFormTraits form = table_form_traits(FORM);
    constexpr bool COMPACT = form.compact; constexpr int BITMAP = form.bitmap;
    const bool term = !(args.auto_reset && !args.start_terminal_any), table_lds = plan.table_lds;
    auto pick = [&](auto tag) {
        constexpr int T = decltype(tag)::value;
        return args.c.criteria != 0u ? lq_rollout_kernel_table_limit<Q, K, RECORD, true, COMPACT, true, BITMAP, T>
               : term            ? lq_rollout_kernel_table_limit<Q, K, RECORD, false, COMPACT, true, BITMAP, T>
                                 : lq_rollout_kernel_table_limit<Q, K, RECORD, false, COMPACT, false, BITMAP, T>;
    };
    auto kern = table_lds ? pick(std::integral_constant<int, 2>{}) : pick(std::integral_constant<int, 1>{});
    const unsigned block = plan.block;
    if (!plan.limit || plan.lds_total > kLdsBytes || block > 512u) return hipErrorInvalidValue;   // (built for 512 threads, as the table instances)
    if (plan.lds_total > 32 * 1024) {
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    const unsigned grid = unsigned(args.n_envs / (block / unsigned(Q)));
    note_kernel("lq_rollout_kernel_table_limit<Q=%d,K=%d,%s,TABLE,%s%s%s%s,%s,LIMIT> block=%u (packed layout: %d agents per lane%s%s; episode step limit; table policy: %u action bytes %s)",
                Q, K, RECORD ? "RECORD" : "TOTALS", args.c.criteria != 0u ? "SOC" : "MAKESPAN", COMPACT ? ",COMPACT" : "",
                (args.c.criteria == 0u && !term) ? ",NO_TERMINAL" : "", form.tag, table_lds ? "TABLE_LDS" : "TABLE_GLOBAL", block, K,
                form.note, BITMAP ? kBitmapNote : "", tp.table_bytes, table_lds ? "staged into LDS behind the image" : "gathered from global memory");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), plan.lds_total, stream, args, A, uint32_t(plan.lds_bytes), tp, plan.table_at, lim);
    return hipGetLastError();
}

// exactly the table instances (MAPF_LQ_ROLLOUT_TABLE_INSTANCES, mapf_layout.hpp) of this object's K
template <int K, bool R>
hipError_t launch_planned_limit(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy &table, const EpisodeLimit &lim) {
#define X(KK, QQ, FF)                                                                                                                                 \
    if constexpr (KK == K) {                                                                                                                          \
        if (plan.Q == QQ && plan.form == TableForm::FF) return launch_impl_table_limit<QQ, K, R, TableForm::FF>(plan, args, A, stream, table, lim);   \
    }
    MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X)
#undef X
    return hipErrorInvalidValue;
}

}  // namespace

// This file is compiled once per (agents per lane, recording) pair -- -DMAPF_LQ_K=4|2 -DMAPF_LQ_RECORD=1|0 -- as mapf_lq_rollout.hip
// is; each object exports one launcher (prototypes: mapf_kernels.hpp; the router: mapf_dispatch.hip).
#if !defined(MAPF_LQ_K) || !defined(MAPF_LQ_RECORD) || (MAPF_LQ_K != 4 && MAPF_LQ_K != 2)
#error "compile with -DMAPF_LQ_K=4|2 -DMAPF_LQ_RECORD=1|0"
#endif
#define MAPF_LQ_CAT3(a, b, c) a##b##_r##c
#define MAPF_LQ_NAME(k, r) MAPF_LQ_CAT3(launch_rollout_lq_limit_k, k, r)

hipError_t MAPF_LQ_NAME(MAPF_LQ_K, MAPF_LQ_RECORD)(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy &table,
                                                   const EpisodeLimit &limit) {
    return launch_planned_limit<MAPF_LQ_K, MAPF_LQ_RECORD != 0>(plan, args, A, stream, table, limit);
}

}  // namespace mapf
