// The dispatcher: launch_rollout, launch_step and launch_transitions, the planned launch entries the C ABI calls.  Each asks the
// planner (route_rollout / route_step, mapf_plan.hpp: which family takes the launch, and that family's plan; plan_transitions) ONCE,
// the first two check the limit / budget block once, and hands the plan to the family's launcher -- the one place where a launch
// meets its translation unit.  Holds no kernel itself.
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

// What the limit and budget kernels rely on: ages and a limit; of a rollout, the truncated trajectory exactly when the launch
// records; under a budget the counts and auto-reset as well, and the limit itself may then be 0 (a budget without a limit).
static bool limit_block_complete(const EpisodeLimit *limit, const EpisodeBudget *budget, bool rollout, bool record, bool auto_reset) {
    if (!limit) return budget == nullptr;
    if (!limit->age || (rollout && (limit->rec_truncated != nullptr) != record)) return false;
    return budget ? (budget->left && auto_reset) : limit->max_steps != 0u;
}

// the thread-per-env object that holds the kernels of the launch's agent count
#define MAPF_TPE_GROUP(fn, A, ...)                      \
    switch (((A) - 1) / 4) {                            \
        case 0: return fn##_g0(__VA_ARGS__);            \
        case 1: return fn##_g1(__VA_ARGS__);            \
        case 2: return fn##_g2(__VA_ARGS__);            \
        case 3: return fn##_g3(__VA_ARGS__);            \
        default: return hipErrorInvalidValue;           \
    }

// the packed rollout object that holds the plan's instance: [under a limit][8, 4, 2 agents per lane][recording]
static hipError_t launch_rollout_lq(const LqPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, const EpisodeLimit *limit) {
    using Launcher = hipError_t (*)(const LqPlan &, const RolloutArgs &, uint32_t, hipStream_t, const TablePolicy *, const EpisodeLimit *);
    static constexpr Launcher objects[2][3][2] = {
        {{launch_rollout_lq_k8_r0, launch_rollout_lq_k8_r1}, {launch_rollout_lq_k4_r0, launch_rollout_lq_k4_r1}, {launch_rollout_lq_k2_r0, launch_rollout_lq_k2_r1}},
        {{nullptr, nullptr}, {launch_rollout_lq_limit_k4_r0, launch_rollout_lq_limit_k4_r1}, {launch_rollout_lq_limit_k2_r0, launch_rollout_lq_limit_k2_r1}}};
    const Launcher launch = objects[plan.limit ? 1 : 0][plan.K == 8 ? 0 : (plan.K == 4 ? 1 : 2)][args.rec_local ? 1 : 0];
    return launch ? launch(plan, args, uint32_t(n_agents), stream, table, limit) : hipErrorInvalidValue;   // (no limit object with eight per lane)
}

hipError_t launch_rollout(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, FamilyPreference prefer, hipStream_t stream, const TablePolicy *table,
                          const EpisodeLimit *limit, const EpisodeBudget *budget, const ConflictPairs *pairs, const JointPolicy *joint, const EpisodeLog *log, const GroupPolicy *group) {
    if (n_agents < 1 || (joint && (table || args.actions)) || (group && (table || joint || args.actions))) return hipErrorInvalidValue;   // (one policy per launch: the C ABI passes at most one)
    if (args.n_envs == 0) return hipSuccess;
    const RolloutRoute r = route_rollout(n_agents, args, tune, prefer, table != nullptr, table ? table->table_bytes : 0u, limit != nullptr, budget != nullptr,
                                         pairs != nullptr, joint != nullptr, log != nullptr, group != nullptr);
    if (!limit_block_complete(limit, budget, true, args.rec_local != nullptr, args.auto_reset)) return hipErrorInvalidValue;
    if (pairs && !(pairs->matrix && pairs->n_slots != 0u)) return hipErrorInvalidValue;
    if (log && !(budget && log->partial && log->records && log->capacity != 0u)) return hipErrorInvalidValue;   // (a log comes with a budget only)
    switch (r.family) {
        case KernelFamily::ThreadPerEnv: MAPF_TPE_GROUP(launch_rollout, n_agents, r.tpe, n_agents, args, stream, table)
        case KernelFamily::Packed: return launch_rollout_lq(r.lq, n_agents, args, stream, table, limit);
        case KernelFamily::LaneGroup: break;
    }
    if (joint && !(joint->table && joint->offset && joint->partner && joint->table_bytes != 0u)) return hipErrorInvalidValue;
    if (group) {   // the route took the lane-group plan of the launch's form, marked `group`: the unit of that form
        if (!(group->table && group->rows && group->members && group->book && group->slots)) return hipErrorInvalidValue;
        if (log) return pairs ? launch_rollout_lg_group_log_pairs_budget(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs)
                              : launch_rollout_lg_group_log_budget(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs);
        if (pairs) return budget ? launch_rollout_lg_group_pairs_budget(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs)
                          : (limit ? launch_rollout_lg_group_pairs_limit(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs)
                                   : launch_rollout_lg_group_pairs_plain(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs));
        return budget ? launch_rollout_lg_group_budget(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs)
                      : (limit ? launch_rollout_lg_group_limit(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs)
                               : launch_rollout_lg_group_plain(r.lg, n_agents, args, stream, *group, limit, budget, log, pairs));
    }
    if (log) {   // the route took the lane-group budget plan, marked `log`: the unit of the launch's policy arm, with the matrix or without
        if (joint) return pairs ? launch_rollout_lg_log_joint_pairs_budget(r.lg, n_agents, args, stream, table, joint, limit, budget, log, pairs)
                                : launch_rollout_lg_log_joint_budget(r.lg, n_agents, args, stream, table, joint, limit, budget, log, pairs);
        return pairs ? launch_rollout_lg_log_pairs_budget(r.lg, n_agents, args, stream, table, joint, limit, budget, log, pairs)
                     : launch_rollout_lg_log_budget(r.lg, n_agents, args, stream, table, joint, limit, budget, log, pairs);
    }
    if (joint) {   // the route took the lane-group plan of the launch's form, marked `joint`: the unit of that form
        if (pairs) return budget ? launch_rollout_lg_joint_pairs_budget(r.lg, n_agents, args, stream, *joint, limit, budget, pairs)
                          : (limit ? launch_rollout_lg_joint_pairs_limit(r.lg, n_agents, args, stream, *joint, limit, budget, pairs)
                                   : launch_rollout_lg_joint_pairs_plain(r.lg, n_agents, args, stream, *joint, limit, budget, pairs));
        return budget ? launch_rollout_lg_joint_budget(r.lg, n_agents, args, stream, *joint, limit, budget, pairs)
                      : (limit ? launch_rollout_lg_joint_limit(r.lg, n_agents, args, stream, *joint, limit, budget, pairs)
                               : launch_rollout_lg_joint_plain(r.lg, n_agents, args, stream, *joint, limit, budget, pairs));
    }
    if (pairs) {   // the route took the lane-group plan of the launch's form, marked `pairs`
        if (budget) return launch_rollout_lg_pairs_budget(r.lg, n_agents, args, stream, table, *limit, *budget, *pairs);
        return limit ? launch_rollout_lg_pairs_limit(r.lg, n_agents, args, stream, table, *limit, *pairs) : launch_rollout_lg_pairs(r.lg, n_agents, args, stream, table, *pairs);
    }
    if (budget) return launch_rollout_lg_budget(r.lg, n_agents, args, stream, table, *limit, *budget);
    return limit ? launch_rollout_lg_limit(r.lg, n_agents, args, stream, table, *limit) : launch_rollout_lg(r.lg, n_agents, args, stream, table);
}

// the route of a step launch (the caller supplies uniforms: a pointer is there -- but the diagnostic build of the packed step,
// `make step_stamps`, receives its stamp buffer through `uniforms`)
static StepRoute route_of(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, const EpisodeLimit *limit) {
#ifdef MAPF_STEP_STAMPS
    const bool ext_uniforms = false;
#else
    const bool ext_uniforms = args.uniforms != nullptr;
#endif
    return route_step(n_agents, args, tune, prefer, limit != nullptr, ext_uniforms);
}

bool step_is_thread_per_env(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, const EpisodeLimit *limit) {
    return route_of(n_agents, args, tune, prefer, limit).family == KernelFamily::ThreadPerEnv;
}

hipError_t launch_step(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, hipStream_t stream, const EpisodeLimit *limit) {
    if (n_agents < 1) return hipErrorInvalidValue;
    if (args.n_envs == 0) return hipSuccess;
    const StepRoute r = route_of(n_agents, args, tune, prefer, limit);
    if (!limit_block_complete(limit, nullptr, false, false, args.auto_reset)) return hipErrorInvalidValue;
    switch (r.family) {
        case KernelFamily::ThreadPerEnv: MAPF_TPE_GROUP(launch_step, n_agents, r.tpe, n_agents, args, stream)
        case KernelFamily::Packed: return launch_step_lq(r.lq, n_agents, args, stream);
        case KernelFamily::LaneGroup: break;
    }
    return limit ? launch_step_lg_limit(r.lg, n_agents, args, stream, *limit) : launch_step_lg(r.lg, n_agents, args, stream);
}

// env.P[s][a]: no route -- the agent count names the family -- but one plan, made here from the call's five shape facts
hipError_t launch_transitions(const TransitionsArgs &args, hipStream_t stream) {
    if (args.n_queries == 0 || args.max_branches == 0) return hipSuccess;
    const bool all_out = args.out_next && args.out_prob && args.out_reward && args.out_done && args.out_collision;
    TransitionsPlan plan;
    if (!plan_transitions(args.n_agents, args.n_queries, args.max_branches, args.compact, all_out, &plan)) return hipErrorInvalidValue;
    if (plan.scan_passes != 0) {
        if (hipError_t e = launch_transitions_scan(plan, args, stream)) return e;
    }
    return plan.wide ? launch_transitions_wide(plan, args, stream) : launch_transitions_rows(plan, args, stream);
}

}  // namespace mapf
