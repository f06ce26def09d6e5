// Lane-group family under an episode budget (include/mapf_hip.h mapf_set_episode_budget; EpisodeBudget in mapf_kernels.hpp): the
// budget forms of the fused rollout kernels, the family that names them to the shared launcher (mapf_lg_launch.hpp), and the
// launcher that takes the route's budget plan.  A translation unit of its own: the kernels that exist without the budget (mapf_lg_rollout.hip, mapf_lg_limit.hip) keep
// their code.
//
// Per env and step of an auto-reset rollout under a budget B (the header has the definition): an env with no episode left is PARKED
// and the step does nothing -- no state, age, count or total changes, nothing is drawn, a recording launch writes the env's cells
// and zeros.  Any other step is the limit kernels' step (with max_steps == 0: the step without a limit); it counts as a live step
// unless the env was terminal on entry, and takes one from the env's episodes left when it reports done or truncated.
#include "mapf_lg_launch.hpp"
#include "mapf_lg_rollout_kernel.hpp"

namespace mapf {

// the budget instances of lg_rollout_kernel (mapf_lg_rollout_kernel.hpp): its EpisodeLimit and EpisodeBudget arguments, behind the
// table policy where the launch follows one; guarded only, as the limit instances are.
// 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table)
struct LgRolloutBudgetFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        if constexpr (TABLE) return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, TablePolicy, EpisodeLimit, EpisodeBudget>;
        else return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false, EpisodeLimit, EpisodeBudget>;
    }
};

// the route's limit plan, marked `budget` (the dispatcher has checked the limit and budget blocks), to the shared launcher (mapf_lg_launch.hpp)
hipError_t launch_rollout_lg_budget(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                    const EpisodeLimit &limit, const EpisodeBudget &budget) {
    return table ? launch_lg_rollout<LgRolloutBudgetFamily, true>(plan, args, uint32_t(n_agents), stream, *table, limit, budget)
                 : launch_lg_rollout<LgRolloutBudgetFamily, false>(plan, args, uint32_t(n_agents), stream, limit, budget);
}

}  // namespace mapf
