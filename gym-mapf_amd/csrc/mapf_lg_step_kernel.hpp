// The lane-group single-step kernel: one template for the instances of mapf_lg_kernels.hip (the plain step) and of
// mapf_lg_limit.hip, whose trailing EpisodeLimit argument (kernel_arg, mapf_device.hpp; include/mapf_hip.h mapf_set_episode_limit)
// makes them the step under an episode step limit.  The limit's sections are `if constexpr`: the plain step compiles to the code
// it had as a kernel of its own (tools/compare_kernels.py, profiles/kernel_templates_device_listings.txt).
// The limit sections: every lane of the group reads the env's age; a step from a terminal state leaves it alone, any other step
// ages the episode by one (saturating) and is TRUNCATED when it did not return done and the age has reached lim.max_steps; the
// leader writes the age back (0 when the env goes back to its start cells) and reports the step's truncated byte
// (lim.rec_truncated: [E] or null); with auto-reset the env goes back on done OR truncated.
#pragma once
#include "mapf_lg.hpp"

namespace mapf {

template <int L, bool FULL, bool EXT_UNIFORMS, class... Extra>
__global__ void __launch_bounds__(256) lg_step_kernel(const StepArgs p, const uint32_t n_agents, const Extra... extra) {
    constexpr bool LIMIT = has_kernel_arg<EpisodeLimit, Extra...>;
    const auto lim = kernel_arg<EpisodeLimit>(extra...);   // by value: an empty tag in the plain step
    bool live;
    const LaneCtx<L> x = lane_ctx<L>(n_agents, p.n_envs, live);
    const uint32_t e = x.e;

    uint32_t cur0, cur1, goal0, goal1, act0, act1;
    load_pair<uint16_t>(p.state, e, n_agents, x.g, x.v0, x.v1, cur0, cur1);
    load_pair<uint16_t>(p.goal, p.goal_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, goal0, goal1);
    load_pair<uint8_t>(p.actions, e, n_agents, x.g, x.v0, x.v1, act0, act1);
    uint32_t age = 0u;
    if constexpr (LIMIT) age = *at(lim.age, e);   // (lanes past the last env: env 0's, never written back)
    double u0 = 0.0, u1 = 0.0;
    if (EXT_UNIFORMS) {
        const double *up = at(p.uniforms, e * n_agents + 2u * x.g);
        if (x.v0) u0 = up[0];
        if (x.v1) u1 = up[1];
    }
    // A single step is launch-latency bound: the sampled probability is rebuilt from its members (no third dependent
    // memory round trip); the 8 slip rows are only read on the exact-tie path and for caller-supplied uniforms,
    // straight from global memory (they stay in L1/L2) rather than staged into LDS behind a barrier.
    const SlipRow *rows = p.slip;

    uint32_t next0, next1;
    EnvOut o;
#ifdef MAPF_STAMPS
    StampCtx st{};
#endif
    uint32_t word = 0u;   // this step's slip word of my pair: the call of my quad (g >> 1), word 2 * (t & 1) + (g & 1)
    const uint64_t t = first_step_index(p);
    if (!EXT_UNIFORMS && p.c.need_rng) word = quad_step_word(slip_words(p.c, p.env_id_offset + e, t >> 1, x.g >> 1, 0u, 0u), t, x.g & 1u);
    lg_transition<L, FULL, EXT_UNIFORMS, false, false, false, !EXT_UNIFORMS>(p.c, p.mv, rows, nullptr, x, n_agents, cur0, cur1, goal0, goal1, act0, act1,
                                                u0, u1, p.env_id_offset + e, t, word, false, next0, next1, o STAMP_ARG);
    if (!live) return;

    uint32_t aged = 0u;
    bool truncated = false;
    if constexpr (LIMIT) {
        aged = o.was_terminal ? age : (age + (age != 0xFFFFFFFFu ? 1u : 0u));
        truncated = !o.was_terminal && !o.done() && aged >= lim.max_steps;
    }
    const bool back = p.auto_reset && (o.done() || truncated);

    if (p.out_local) store_cells(p.out_local, e, n_agents, x.g, x.v0, x.v1, next0, next1);
    if (x.g == uint32_t(L - 1) && p.out_prob) *at(p.out_prob, e) = o.prob;   // the product chain ends in the last lane
    if (x.g == 0u) {
        if (p.out_reward) *at(p.out_reward, e) = o.reward;
        if (p.out_done) *at(p.out_done, e) = o.done() ? 1 : 0;
        if (p.out_collision) *at(p.out_collision, e) = o.collision() ? 1 : 0;
        if (p.out_was_terminal) *at(p.out_was_terminal, e) = o.was_terminal ? 1 : 0;
        if constexpr (LIMIT) {
            if (lim.rec_truncated) *at(lim.rec_truncated, e) = truncated ? 1 : 0;
            *at(lim.age, e) = back ? 0u : aged;
        }
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

}  // namespace mapf
