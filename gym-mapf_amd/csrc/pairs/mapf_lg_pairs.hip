// Lane-group family under the conflict matrix (include/mapf_hip.h mapf_set_conflict_pairs; ConflictPairs in mapf_kernels.hpp): the
// forms of the fused rollout kernels that count, per agent pair, the vertex conflicts and the swaps of every live step, the
// families that name them to the shared launcher (mapf_lg_launch.hpp), and the launchers that take the route's plan.  Compiled once
// per form (the Makefile's second table, MAPF_PAIRS_FORM: 0 plain, 1 under an episode step limit, 2 under an episode budget), each a
// unit of its own: the kernels that exist without the matrix (mapf_lg_rollout.hip, mapf_lg_limit.hip, mapf_lg_budget.hip) keep their code.
//
// Per env and step (the header has the definition): the step is the one of the instance without the matrix -- state, outputs,
// totals, ages, counts and both Philox streams are bit for bit the same.  A step that was not a no-op and reports a collision
// then adds one count per conflicting pair to the env's slot (lg_count_pairs, mapf_lg_rollout_kernel.hpp).
#include "../mapf_lg_launch.hpp"
#include "../mapf_lg_rollout_kernel.hpp"

#ifndef MAPF_PAIRS_FORM
#error "MAPF_PAIRS_FORM: 0 plain, 1 limit, 2 budget (the Makefile compiles this unit once per form)"
#endif

namespace mapf {

// the instances of lg_rollout_kernel (mapf_lg_rollout_kernel.hpp) with the ConflictPairs argument, behind the blocks of the form
// and, where the launch follows one, the table policy; guarded only, as the limit instances are.
// each form: 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table)
template <class... Form>
struct LgRolloutPairsFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        if constexpr (TABLE) return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, TablePolicy, Form..., ConflictPairs>;
        else return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false, Form..., ConflictPairs>;
    }
};

// the route's plan, marked `pairs` (the dispatcher has checked the blocks), to the shared launcher (mapf_lg_launch.hpp)
#if MAPF_PAIRS_FORM == 0
hipError_t launch_rollout_lg_pairs(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, const ConflictPairs &pairs) {
    using Family = LgRolloutPairsFamily<>;
    return table ? launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, *table, pairs)
                 : launch_lg_rollout<Family, false>(plan, args, uint32_t(n_agents), stream, pairs);
}
#elif MAPF_PAIRS_FORM == 1
hipError_t launch_rollout_lg_pairs_limit(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                         const EpisodeLimit &limit, const ConflictPairs &pairs) {
    using Family = LgRolloutPairsFamily<EpisodeLimit>;
    return table ? launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, *table, limit, pairs)
                 : launch_lg_rollout<Family, false>(plan, args, uint32_t(n_agents), stream, limit, pairs);
}
#else
hipError_t launch_rollout_lg_pairs_budget(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                          const EpisodeLimit &limit, const EpisodeBudget &budget, const ConflictPairs &pairs) {
    using Family = LgRolloutPairsFamily<EpisodeLimit, EpisodeBudget>;
    return table ? launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, *table, limit, budget, pairs)
                 : launch_lg_rollout<Family, false>(plan, args, uint32_t(n_agents), stream, limit, budget, pairs);
}
#endif

}  // namespace mapf
