// Lane-group family under the episode log (include/mapf_hip.h mapf_set_episode_log; EpisodeLog in csrc/mapf_kernels.hpp): the budget
// forms of the fused rollout kernels that record every finished episode per env -- its return, its live steps and how it ended --
// the families that name them to the shared launcher (csrc/mapf_lg_launch.hpp), and the launchers that take the route's plan.
// Compiled once per (policy arm, conflict matrix) -- the Makefile's fourth table: MAPF_LOG_JOINT 0 streamed actions, the in-kernel
// policy and the table policy, 1 the joint table policy; MAPF_LOG_PAIRS 1: with the conflict matrix last -- each a unit of its own:
// the kernels that exist without the log keep their code.  The source lies beside csrc/ and csrc_joint/, not below them: the tests
// that pin the first three tables also pin which .hip files those directories hold.
//
// Per env and step (the header has the definition): the step is the one of the budget instance without the log -- state, outputs,
// totals, ages, counts of episodes left, the conflict matrix and both Philox streams are bit for bit the same.  A step that is not
// parked adds its reward to the env's running return and, if live, one to its running length; a step that reports done or truncated
// stores {return, length, done | collision << 1 | truncated << 2} as the env's next record while it has room, counts the episode
// and begins the next one.
#include "../csrc/mapf_lg_launch.hpp"
#include "../csrc/mapf_lg_rollout_kernel.hpp"

#if !defined(MAPF_LOG_JOINT) || !defined(MAPF_LOG_PAIRS)
#error "MAPF_LOG_JOINT: 0 | 1; MAPF_LOG_PAIRS: 0 | 1 (the Makefile compiles this unit once per pair of them)"
#endif

namespace mapf {

// the instances of lg_rollout_kernel (csrc/mapf_lg_rollout_kernel.hpp) with the EpisodeLog argument behind EpisodeLimit and
// EpisodeBudget, in front of the conflict matrix where the unit counts pairs; guarded only, as the budget instances are.
#if MAPF_LOG_JOINT
// each joint unit: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances
template <class... Tail>
struct LgRolloutLogFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        static_assert(TABLE && !STREAM, "the joint launches run without streamed actions");
        return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, JointPolicy, EpisodeLimit, EpisodeBudget, EpisodeLog, Tail...>;
    }
};
#else
// each unit without the joint policy: 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table) = 168 instances
template <class... Tail>
struct LgRolloutLogFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        if constexpr (TABLE) return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, TablePolicy, EpisodeLimit, EpisodeBudget, EpisodeLog, Tail...>;
        else return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false, EpisodeLimit, EpisodeBudget, EpisodeLog, Tail...>;
    }
};
#endif

#if MAPF_LOG_PAIRS
using LogFamily = LgRolloutLogFamily<ConflictPairs>;
#define MAPF_LOG_TAIL_ARG , *pairs
#else
using LogFamily = LgRolloutLogFamily<>;
#define MAPF_LOG_TAIL_ARG
#endif

// the route's budget plan, marked `log` (the dispatcher has checked the blocks), to the shared launcher
#define MAPF_LOG_SIGNATURE(form)                                                                                                             \
    hipError_t launch_rollout_lg_log_##form(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, \
                                            const JointPolicy *joint, const EpisodeLimit *limit, const EpisodeBudget *budget, const EpisodeLog *log,       \
                                            const ConflictPairs *pairs)
#define MAPF_LOG_REFUSES (!limit || !budget || !log || !plan.log || (pairs != nullptr) != bool(MAPF_LOG_PAIRS) || (joint != nullptr) != bool(MAPF_LOG_JOINT))

#if MAPF_LOG_JOINT
#if MAPF_LOG_PAIRS
MAPF_LOG_SIGNATURE(joint_pairs_budget) {
#else
MAPF_LOG_SIGNATURE(joint_budget) {
#endif
    if (MAPF_LOG_REFUSES || table || !plan.joint) return hipErrorInvalidValue;
    return launch_lg_rollout<LogFamily, true>(plan, args, uint32_t(n_agents), stream, *joint, *limit, *budget, *log MAPF_LOG_TAIL_ARG);
}
#else
#if MAPF_LOG_PAIRS
MAPF_LOG_SIGNATURE(pairs_budget) {
#else
MAPF_LOG_SIGNATURE(budget) {
#endif
    if (MAPF_LOG_REFUSES) return hipErrorInvalidValue;
    return table ? launch_lg_rollout<LogFamily, true>(plan, args, uint32_t(n_agents), stream, *table, *limit, *budget, *log MAPF_LOG_TAIL_ARG)
                 : launch_lg_rollout<LogFamily, false>(plan, args, uint32_t(n_agents), stream, *limit, *budget, *log MAPF_LOG_TAIL_ARG);
}
#endif

#if !MAPF_LOG_JOINT && !MAPF_LOG_PAIRS
// mapf_reset(mask): a reset env's running episode is dropped (one more kernel of this unit, beside its 168 rollout instances)
__global__ void reset_log_partials_kernel(EpisodeLogPartial *partial, const uint8_t *mask, uint64_t n_envs) {
    const uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e < n_envs && mask[e]) partial[e] = EpisodeLogPartial{0.0, 0u, 0u};
}

hipError_t launch_reset_log_partials(EpisodeLogPartial *partial, const uint8_t *mask, uint64_t n_envs, hipStream_t stream) {
    if (n_envs == 0) return hipSuccess;
    if (!mask) return hipMemsetAsync(partial, 0, n_envs * sizeof(EpisodeLogPartial), stream);
    const uint64_t grid = (n_envs + 255u) / 256u;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reset_log_partials_kernel, dim3(unsigned(grid)), dim3(256), 0, stream, partial, mask, n_envs);
    return hipGetLastError();
}
#endif

}  // namespace mapf
