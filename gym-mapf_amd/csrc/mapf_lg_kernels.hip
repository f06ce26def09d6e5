// Lane-group family: single-step kernel, run-time-A helper kernels and their launchers (device code: mapf_lg.hpp; the step's
// plan: the route's, mapf_plan.hip; its launcher proper: mapf_lg_launch.hpp).
#include "mapf_lg_launch.hpp"
#include "mapf_lg_step_kernel.hpp"

namespace mapf {

// the plain instances of lg_step_kernel (mapf_lg_step_kernel.hpp): no argument behind (args, A)
struct LgStepFamily {
    template <int L, bool FULL, bool EXT_UNIFORMS>
    static auto kernel() { return lg_step_kernel<L, FULL, EXT_UNIFORMS>; }
};

// ------------------------------------------------------- run-time-A helper kernels
// masked MapfEnv.reset (mapf_env.py:290-293): one thread per cell
__global__ void __launch_bounds__(256) reset_kernel(uint16_t *state, const uint16_t *start, bool start_broadcast,
                                                    const uint8_t *mask, uint64_t n_envs, uint32_t n_agents) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_envs * n_agents) return;
    const uint64_t e = i / n_agents;
    if (mask && mask[e] == 0) return;
    state[i] = start[start_broadcast ? i - e * n_agents : i];
}

// MapfEnv.is_terminal (mapf_env.py:210-223) of the stored state: one thread per env
__global__ void __launch_bounds__(256) query_terminal_kernel(const uint16_t *state, const uint16_t *goal,
                                                             bool goal_broadcast, uint8_t *out, uint64_t n_envs,
                                                             uint32_t n_agents) {
    const uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= n_envs) return;
    const uint16_t *cur = state + e * n_agents, *g = goal + (goal_broadcast ? 0 : e * n_agents);
    bool dup = false, all_goal = true;
    for (uint32_t i = 0; i < n_agents; ++i) {
        all_goal &= (cur[i] == g[i]);
        for (uint32_t j = i + 1; j < n_agents; ++j) dup |= (cur[i] == cur[j]);
    }
    out[e] = (dup || all_goal) ? 1 : 0;
}

// policy stream (oracle/philox.py random_actions_np): one thread per (four-step block, env, agent quad) -- one Philox
// call, whose word t & 3 holds the quad's four action bytes of step t
__global__ void __launch_bounds__(256) fill_actions_kernel(uint8_t *actions, EnvConsts c, uint64_t env_id_offset,
                                                           uint64_t n_envs, uint64_t t0, uint64_t n_steps,
                                                           uint32_t n_agents) {
    const uint32_t quads = (n_agents + 3u) / 4u;
    const uint64_t m0 = t0 >> 2, n_blocks = ((t0 + n_steps - 1u) >> 2) - m0 + 1u;
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_blocks * n_envs * quads) return;
    const uint64_t row = i / quads;                              // (block, env)
    const uint32_t q = uint32_t(i - row * quads);
    const uint64_t blk = row / n_envs, e = row - blk * n_envs;
    const uint64_t m = m0 + blk;
    const Words4 w = policy_words(c, env_id_offset + e, m, q);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t t = 4u * m + j;
        if (t < t0 || t >= t0 + n_steps) continue;
        const uint32_t word = pick_word(w, j);
        uint8_t *dst = actions + ((t - t0) * n_envs + e) * n_agents + 4u * q;
        if ((n_agents & 3u) == 0u) {                            // a quad's four bytes as one store
            *reinterpret_cast<uint32_t *>(dst) = policy_action_rt(word, 0u) | (policy_action_rt(word, 1u) << 8) |
                                                 (policy_action_rt(word, 2u) << 16) | (policy_action_rt(word, 3u) << 24);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (4u * q + k < n_agents) dst[k] = uint8_t(policy_action_rt(word, k));
        }
    }
}

// the device-side step index of a recorded graph (StepArgs::t_dev): advanced by the graph's last node
__global__ void __launch_bounds__(64) advance_step_index_kernel(uint64_t *t_dev, uint64_t n, bool set) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) *t_dev = set ? n : *t_dev + n;
}

hipError_t launch_advance_step_index(uint64_t *t_dev, uint64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(advance_step_index_kernel, dim3(1), dim3(64), 0, stream, t_dev, n, false);
    return hipGetLastError();
}

hipError_t launch_set_step_index(uint64_t *t_dev, uint64_t value, hipStream_t stream) {
    hipLaunchKernelGGL(advance_step_index_kernel, dim3(1), dim3(64), 0, stream, t_dev, value, true);
    return hipGetLastError();
}

static inline hipError_t grid_1d(uint64_t n, unsigned block, unsigned &grid) {
    const uint64_t g = (n + block - 1) / block;
    if (g > 0x7FFFFFFFull) return hipErrorInvalidValue;
    grid = unsigned(g);
    return hipSuccess;
}

hipError_t launch_reset(int n_agents, uint16_t *state, const uint16_t *start, bool start_broadcast,
                        const uint8_t *mask, uint64_t n_envs, hipStream_t stream) {
    if (n_envs == 0) return hipSuccess;
    unsigned grid;
    if (hipError_t e = grid_1d(n_envs * uint64_t(n_agents), 256, grid)) return e;
    hipLaunchKernelGGL(reset_kernel, dim3(grid), dim3(256), 0, stream, state, start, start_broadcast, mask, n_envs,
                       uint32_t(n_agents));
    return hipGetLastError();
}

hipError_t launch_query_terminal(int n_agents, const uint16_t *state, const uint16_t *goal, bool goal_broadcast,
                                 uint8_t *out, uint64_t n_envs, hipStream_t stream) {
    if (n_envs == 0) return hipSuccess;
    unsigned grid;
    if (hipError_t e = grid_1d(n_envs, 256, grid)) return e;
    hipLaunchKernelGGL(query_terminal_kernel, dim3(grid), dim3(256), 0, stream, state, goal, goal_broadcast, out,
                       n_envs, uint32_t(n_agents));
    return hipGetLastError();
}

hipError_t launch_fill_actions(int n_agents, uint8_t *actions, const EnvConsts &c, uint64_t env_id_offset,
                               uint64_t n_envs, uint64_t t0, uint64_t n_steps, hipStream_t stream) {
    if (n_envs == 0 || n_steps == 0) return hipSuccess;
    const uint64_t n_blocks = ((t0 + n_steps - 1u) >> 2) - (t0 >> 2) + 1u;
    unsigned grid;
    if (hipError_t e = grid_1d(n_blocks * n_envs * uint64_t((n_agents + 3) / 4), 256, grid)) return e;
    hipLaunchKernelGGL(fill_actions_kernel, dim3(grid), dim3(256), 0, stream, actions, c, env_id_offset, n_envs, t0,
                       n_steps, uint32_t(n_agents));
    return hipGetLastError();
}

// ------------------------------------------------------------------- launchers
hipError_t launch_step_lg(const LgStepPlan &plan, int n_agents, const StepArgs &args, hipStream_t stream) {
    return launch_lg_step<LgStepFamily>(plan, args, uint32_t(n_agents), stream);
}

}  // namespace mapf
