// Routes a launch to the translation unit that holds the kernels specialised for its shape: the thread-per-env family by agent
// count, the packed rollout by its plan (mapf_plan.hpp).  Holds no kernel itself.
#include "mapf_kernels.hpp"
#include "mapf_plan.hpp"

#include <cstdlib>

namespace mapf {

// The tuning of a handle: the device's CU count and the MAPF_TUNE override, both asked ONCE, at mapf_create.
RolloutTuning default_rollout_tuning(int device, std::string *err) {
    int n_cu = 256;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu <= 0) n_cu = 256;
    return rollout_tuning_for(n_cu, getenv("MAPF_TUNE"), err);
}

#define MAPF_ROUTE(fn, A, ...)                          \
    switch (((A) - 1) / 4) {                            \
        case 0: return fn##_g0(A, __VA_ARGS__);         \
        case 1: return fn##_g1(A, __VA_ARGS__);         \
        case 2: return fn##_g2(A, __VA_ARGS__);         \
        case 3: return fn##_g3(A, __VA_ARGS__);         \
        default: return hipErrorInvalidValue;           \
    }

hipError_t launch_step(int n_agents, const StepArgs &args, hipStream_t stream) {
    if (n_agents < 1) return hipErrorInvalidValue;
    MAPF_ROUTE(launch_step, n_agents, args, stream)
}

hipError_t launch_rollout(int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table) {
    if (n_agents < 1) return hipErrorInvalidValue;
    MAPF_ROUTE(launch_rollout, n_agents, args, stream, table)
}

// true when a packed layout took the launch (*err = its status); false = not applicable, use the lane-group kernel.  Under an
// episode step limit the packed instances are the table policy's (mapf_lq_limit.hip), opted into by MAPF_TUNE limit_packed=1
bool try_launch_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, hipError_t *err, const TablePolicy *table,
                           const EpisodeLimit *limit) {
    LqPlan plan;
    if (limit && (args.n_envs == 0 || args.actions != nullptr || !table || !tune.limit_packed)) return false;
    if (table ? !plan_rollout_lq_table(n_agents, args, tune, table->table_bytes, &plan, limit != nullptr) : !plan_rollout_lq(n_agents, args, tune, &plan)) return false;
    const bool record = args.rec_local != nullptr;
    // the object that holds the plan's instance: [under a limit][8, 4, 2 agents per lane][recording]
    using Launcher = hipError_t (*)(const LqPlan &, const RolloutArgs &, uint32_t, hipStream_t, const TablePolicy *, const EpisodeLimit *);
    static constexpr Launcher objects[2][3][2] = {
        {{launch_rollout_lq_k8_r0, launch_rollout_lq_k8_r1}, {launch_rollout_lq_k4_r0, launch_rollout_lq_k4_r1}, {launch_rollout_lq_k2_r0, launch_rollout_lq_k2_r1}},
        {{nullptr, nullptr}, {launch_rollout_lq_limit_k4_r0, launch_rollout_lq_limit_k4_r1}, {launch_rollout_lq_limit_k2_r0, launch_rollout_lq_limit_k2_r1}}};
    const Launcher launch = objects[limit ? 1 : 0][plan.K == 8 ? 0 : (plan.K == 4 ? 1 : 2)][record ? 1 : 0];
    // what the limit kernels rely on: ages, a limit, and the truncated trajectory exactly when the launch records
    const bool incomplete = limit && (!limit->age || limit->max_steps == 0u || (limit->rec_truncated != nullptr) != record);
    *err = (incomplete || !launch) ? hipErrorInvalidValue : launch(plan, args, uint32_t(n_agents), stream, table, limit);   // (no limit object with eight per lane)
    return true;
}

}  // namespace mapf
