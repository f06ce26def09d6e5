// Lane-group family under an episode step limit (include/mapf_hip.h mapf_set_episode_limit; EpisodeLimit in mapf_kernels.hpp):
// the limit forms of the fused rollout kernels and of the single step, the families that name them to the shared launchers
// (mapf_lg_launch.hpp), and the launchers that take the route's limit plans.  A translation unit of its own: the kernels that exist without the limit
// (mapf_lg_rollout.hip, mapf_lg_kernels.hip) keep their code.
//
// Per env and step taken under a limit N (the header has the definition): a step from a terminal state is the usual no-op and
// leaves the age alone; any other step ages the episode by one (saturating) and is TRUNCATED when it did not return done and the
// age has reached N.  With auto-reset a done or truncated env goes back to its start cells and its age to 0; without it the
// age is kept and the env reports truncated on every later live step.  Nothing else of the step changes: reward, prob, done,
// collision, the totals and every Philox counter are those of the kernels without the limit.
#include "mapf_lg_launch.hpp"
#include "mapf_lg_rollout_kernel.hpp"
#include "mapf_lg_step_kernel.hpp"

namespace mapf {

// the limit instances of lg_rollout_kernel (mapf_lg_rollout_kernel.hpp): its EpisodeLimit argument, behind the table policy where
// the launch follows one; guarded only, whatever the plan's `dense` (plan_rollout_lg clears it for them)
struct LgRolloutLimitFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        if constexpr (TABLE) return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, TablePolicy, EpisodeLimit>;
        else return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false, EpisodeLimit>;
    }
};

// the limit instances of lg_step_kernel (mapf_lg_step_kernel.hpp; mapf_lg_kernels.hip has the plain ones)
struct LgStepLimitFamily {
    template <int L, bool FULL, bool EXT_UNIFORMS>
    static auto kernel() { return lg_step_kernel<L, FULL, EXT_UNIFORMS, EpisodeLimit>; }
};

// mapf_reset(mask) on a handle with a limit: the ages of the envs it resets go to 0 (one thread per env)
__global__ void __launch_bounds__(256) reset_ages_kernel(uint32_t *age, const uint8_t *mask, uint64_t n_envs) {
    const uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= n_envs) return;
    if (mask[e] != 0) age[e] = 0u;
}

hipError_t launch_reset_ages(uint32_t *age, const uint8_t *mask, uint64_t n_envs, hipStream_t stream) {
    if (n_envs == 0) return hipSuccess;
    if (!mask) return hipMemsetAsync(age, 0, n_envs * sizeof(uint32_t), stream);
    const uint64_t grid = (n_envs + 255u) / 256u;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reset_ages_kernel, dim3(unsigned(grid)), dim3(256), 0, stream, age, mask, n_envs);
    return hipGetLastError();
}

// ------------------------------------------------------------------- launchers
// the limit plan the route made (the dispatcher has checked the limit block) to the shared launcher (mapf_lg_launch.hpp)
hipError_t launch_rollout_lg_limit(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                   const EpisodeLimit &limit) {
    return table ? launch_lg_rollout<LgRolloutLimitFamily, true>(plan, args, uint32_t(n_agents), stream, *table, limit)
                 : launch_lg_rollout<LgRolloutLimitFamily, false>(plan, args, uint32_t(n_agents), stream, limit);
}

hipError_t launch_step_lg_limit(const LgStepPlan &plan, int n_agents, const StepArgs &args, hipStream_t stream, const EpisodeLimit &limit) {
    return launch_lg_step<LgStepLimitFamily>(plan, args, uint32_t(n_agents), stream, limit);
}

}  // namespace mapf
