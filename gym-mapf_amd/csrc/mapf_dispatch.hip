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

// true when a packed layout took the launch (*err = its status); false = not applicable, use the lane-group kernel
bool try_launch_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, hipError_t *err, const TablePolicy *table) {
    LqPlan plan;
    if (table ? !plan_rollout_lq_table(n_agents, args, tune, table->table_bytes, &plan) : !plan_rollout_lq(n_agents, args, tune, &plan)) return false;
    const bool record = args.rec_local != nullptr;
    const uint32_t A = uint32_t(n_agents);
    if (plan.K == 8) *err = record ? launch_rollout_lq_k8_r1(plan, args, A, stream, table) : launch_rollout_lq_k8_r0(plan, args, A, stream, table);
    else if (plan.K == 4) *err = record ? launch_rollout_lq_k4_r1(plan, args, A, stream, table) : launch_rollout_lq_k4_r0(plan, args, A, stream, table);
    else *err = record ? launch_rollout_lq_k2_r1(plan, args, A, stream, table) : launch_rollout_lq_k2_r0(plan, args, A, stream, table);
    return true;
}

// ... under an episode step limit: the packed table instances' limit forms (mapf_lq_limit.hip), with launch_rollout_lg_limit's pre-checks
bool try_launch_rollout_lq_limit(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, hipError_t *err, const TablePolicy &table,
                                 const EpisodeLimit &limit) {
    LqPlan plan;
    if (args.n_envs == 0 || args.actions != nullptr || !tune.limit_packed || !plan_rollout_lq_table(n_agents, args, tune, table.table_bytes, &plan, true)) return false;
    const bool record = args.rec_local != nullptr;
    const uint32_t A = uint32_t(n_agents);
    // what the kernels rely on: ages, a limit, and the truncated trajectory exactly when the launch records
    if (!limit.age || limit.max_steps == 0u || (limit.rec_truncated != nullptr) != record) *err = hipErrorInvalidValue;
    else if (plan.K == 4) *err = record ? launch_rollout_lq_limit_k4_r1(plan, args, A, stream, table, limit) : launch_rollout_lq_limit_k4_r0(plan, args, A, stream, table, limit);
    else if (plan.K == 2) *err = record ? launch_rollout_lq_limit_k2_r1(plan, args, A, stream, table, limit) : launch_rollout_lq_limit_k2_r0(plan, args, A, stream, table, limit);
    else *err = hipErrorInvalidValue;   // (plan_rollout_lq_table plans no other K)
    return true;
}

}  // namespace mapf
