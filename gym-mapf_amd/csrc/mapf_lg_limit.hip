// Lane-group family under an episode step limit (include/mapf_hip.h mapf_set_episode_limit; EpisodeLimit in mapf_kernels.hpp):
// the limit forms of the fused rollout kernels and of the single step, and their launchers.  A translation unit of its own: the
// kernels that exist without the limit (mapf_lg_rollout.hip, mapf_lg_kernels.hip) keep their code.
//
// Per env and step taken under a limit N (the header has the definition): a step from a terminal state is the usual no-op and
// leaves the age alone; any other step ages the episode by one (saturating) and is TRUNCATED when it did not return done and the
// age has reached N.  With auto-reset a done or truncated env goes back to its start cells and its age to 0; without it the
// age is kept and the env reports truncated on every later live step.  Nothing else of the step changes: reward, prob, done,
// collision, the totals and every Philox counter are those of the kernels without the limit.
#include "mapf_lg.hpp"
#include "mapf_plan.hpp"

#include <type_traits>

namespace mapf {

// lg_rollout_kernel_limit_guarded (streamed actions, the policy stream, the greedy policy) and
// lg_rollout_kernel_table_limit_guarded (the table policy): the body of the rollout kernels with its limit sections
#define MAPF_ROLLOUT_LIMIT 1
#define MAPF_ROLLOUT_TABLE_KERNEL 0
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#undef MAPF_ROLLOUT_LIMIT

// lg_step_kernel (mapf_lg_kernels.hip) with the env's age: every lane of the group reads it, the leader writes it back and
// reports the step's truncated byte (lim.rec_truncated: [E] or null)
template <int L, bool FULL, bool EXT_UNIFORMS>
__global__ void __launch_bounds__(256) lg_step_kernel_limit(const StepArgs p, const uint32_t n_agents, const EpisodeLimit lim) {
    bool live;
    const LaneCtx<L> x = lane_ctx<L>(n_agents, p.n_envs, live);
    const uint32_t e = x.e;

    uint32_t cur0, cur1, goal0, goal1, act0, act1;
    load_pair<uint16_t>(p.state, e, n_agents, x.g, x.v0, x.v1, cur0, cur1);
    load_pair<uint16_t>(p.goal, p.goal_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, goal0, goal1);
    load_pair<uint8_t>(p.actions, e, n_agents, x.g, x.v0, x.v1, act0, act1);
    const uint32_t age = *at(lim.age, e);   // (lanes past the last env: env 0's, never written back)
    double u0 = 0.0, u1 = 0.0;
    if (EXT_UNIFORMS) {
        const double *up = at(p.uniforms, e * n_agents + 2u * x.g);
        if (x.v0) u0 = up[0];
        if (x.v1) u1 = up[1];
    }
    const SlipRow *rows = p.slip;   // (read from global memory on the exact paths only, as in lg_step_kernel)

    uint32_t next0, next1;
    EnvOut o;
#ifdef MAPF_STAMPS
    StampCtx st{};
#endif
    uint32_t word = 0u;
    const uint64_t t = first_step_index(p);
    if (!EXT_UNIFORMS && p.c.need_rng) word = quad_step_word(slip_words(p.c, p.env_id_offset + e, t >> 1, x.g >> 1, 0u, 0u), t, x.g & 1u);
    lg_transition<L, FULL, EXT_UNIFORMS, false, false, false, !EXT_UNIFORMS>(p.c, p.mv, rows, nullptr, x, n_agents, cur0, cur1, goal0, goal1, act0, act1,
                                                u0, u1, p.env_id_offset + e, t, word, false, next0, next1, o STAMP_ARG);
    if (!live) return;

    const uint32_t aged = o.was_terminal ? age : (age + (age != 0xFFFFFFFFu ? 1u : 0u));
    const bool truncated = !o.was_terminal && !o.done() && aged >= lim.max_steps;
    const bool back = p.auto_reset && (o.done() || truncated);

    if (p.out_local) store_cells(p.out_local, e, n_agents, x.g, x.v0, x.v1, next0, next1);
    if (x.g == uint32_t(L - 1) && p.out_prob) *at(p.out_prob, e) = o.prob;   // the product chain ends in the last lane
    if (x.g == 0u) {
        if (p.out_reward) *at(p.out_reward, e) = o.reward;
        if (p.out_done) *at(p.out_done, e) = o.done() ? 1 : 0;
        if (p.out_collision) *at(p.out_collision, e) = o.collision() ? 1 : 0;
        if (p.out_was_terminal) *at(p.out_was_terminal, e) = o.was_terminal ? 1 : 0;
        if (lim.rec_truncated) *at(lim.rec_truncated, e) = truncated ? 1 : 0;
        *at(lim.age, e) = back ? 0u : aged;
    }
    if (back) {
        uint32_t s0, s1;
        load_pair<uint16_t>(p.start, p.start_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, s0, s1);
        store_cells(p.state, e, n_agents, x.g, x.v0, x.v1, s0, s1);
    } else if (!o.was_terminal) {
        store_cells(p.state, e, n_agents, x.g, x.v0, x.v1, next0, next1);
    }
    signal_step_done(p.done_flag, p.done_seq);
}

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
// Launches the planned limit instance: MV_LDS picks the kernel, the plan gives its geometry and its LDS segment.
template <int L, bool FULL, bool RECORD, bool STREAM, bool TABLE>
static hipError_t launch_limit_instance(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table,
                                        const EpisodeLimit &limit) {
    auto pick = [&](auto mv_lds) {
        constexpr bool MV_LDS = decltype(mv_lds)::value;
        if constexpr (TABLE) return lg_rollout_kernel_table_limit_guarded<L, FULL, MV_LDS, RECORD>;
        else return lg_rollout_kernel_limit_guarded<L, FULL, MV_LDS, RECORD, STREAM>;
    };
    const auto kern = plan.mv_lds ? pick(std::true_type{}) : pick(std::false_type{});
    if (plan.lds_bytes > 32 * 1024) {
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes - kLdsReserve))) return e;
    }
    char name[kKernelNameBytes];
    lg_rollout_limit_kernel_name(name, plan, RECORD, STREAM, TABLE);
    note_kernel("%s", name);
    if constexpr (TABLE) hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, args, A, *table, limit);
    else hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, args, A, limit);
    return hipGetLastError();
}

template <bool TABLE>
static hipError_t launch_limit_planned(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table,
                                       const EpisodeLimit &limit) {
    const bool record = args.rec_local != nullptr, streamed = !TABLE && args.actions != nullptr;
    switch (plan.L) {
#define P(N, FULL, RECORD) (streamed ? launch_limit_instance<N, FULL, RECORD, !TABLE, TABLE>(plan, args, A, stream, table, limit)  \
                                     : launch_limit_instance<N, FULL, RECORD, false, TABLE>(plan, args, A, stream, table, limit))
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

hipError_t launch_rollout_lg_limit(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, const TablePolicy *table,
                                   const EpisodeLimit &limit) {
    if (args.n_envs == 0) return hipSuccess;
    // what the kernels rely on: ages, a limit, and the truncated trajectory exactly when the launch records
    if (!limit.age || limit.max_steps == 0u || (limit.rec_truncated != nullptr) != (args.rec_local != nullptr)) return hipErrorInvalidValue;
    const LgRolloutPlan plan = plan_rollout_lg_limit(n_agents, args, tune);
    return table ? launch_limit_planned<true>(plan, args, uint32_t(n_agents), stream, table, limit)
                 : launch_limit_planned<false>(plan, args, uint32_t(n_agents), stream, table, limit);
}

hipError_t launch_step_lg_limit(int n_agents, const StepArgs &args, hipStream_t stream, const EpisodeLimit &limit) {
    if (args.n_envs == 0) return hipSuccess;
    if (!limit.age || limit.max_steps == 0u) return hipErrorInvalidValue;
    const LgStepPlan plan = plan_step_lg(n_agents, args);
    const bool ext = args.uniforms != nullptr;
    void (*kern)(const StepArgs, const uint32_t, const EpisodeLimit) = nullptr;
    switch (plan.L) {
#define X(N)                                                                                                               \
    case N:                                                                                                                \
        kern = ext ? (plan.full ? lg_step_kernel_limit<N, true, true> : lg_step_kernel_limit<N, false, true>)              \
                   : (plan.full ? lg_step_kernel_limit<N, true, false> : lg_step_kernel_limit<N, false, false>);           \
        break;
        MAPF_FOR_EACH_L(X)
#undef X
        default: return hipErrorInvalidValue;
    }
    char name[kKernelNameBytes];
    lg_step_limit_kernel_name(name, plan, ext);
    note_kernel("%s", name);
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), 0, stream, args, uint32_t(n_agents), limit);
    return hipGetLastError();
}

}  // namespace mapf
