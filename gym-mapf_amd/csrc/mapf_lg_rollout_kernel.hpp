// The lane-group rollout kernel: one template for every instance of mapf_lg_rollout.hip, mapf_lg_limit.hip and mapf_lg_budget.hip.
// What an instance does beyond the plain rollout is read from the types of its trailing arguments (kernel_arg, mapf_device.hpp),
// which follow (p, n_agents) in this order:
//   TablePolicy   -- the table policy (MAPF_POLICY_TABLE): agent i of env e on cell c takes tp.table[tp.rows[e * A + i] * V + c],
//     gathered from global memory; the row bases wait in two registers per lane as the greedy policy's goal coordinates do.  Such an
//     instance runs the launches without streamed actions: STREAM is false.
//   JointPolicy   -- the joint table policy (MAPF_POLICY_JOINT), in TablePolicy's place and never beside it: an agent merged with a
//     partner takes jp.table[jp.offset[e * A + i] + c_i * V + c_j], a solo agent jp.table[jp.offset[e * A + i] + c_i].  Per agent a
//     segment base, a row stride (V, or 0 when solo) and a selector -- the lane that holds the partner and which half of its cell
//     word -- wait in registers; the step reads the partner lane's cells with one ds_bpermute per agent (a solo agent is its own
//     partner, so one formula serves both), then gathers the byte from global memory.  STREAM is false.
//   GroupPolicy   -- the group policy (MAPF_POLICY_GROUP), in TablePolicy's / JointPolicy's place and never beside either: every agent has
//     a solo row; an agent of a group of 2..4 takes its byte of the entry of the group's current joint cell where the group's book has
//     one, else its row's byte.  Per agent a row base, the book's number (none: solo, a ghost slot, a lane past the last env) and ONE
//     register of four 7-bit selectors (the lane that holds each member and the half of its cell word), the agent's position in the
//     list and the group's size wait in registers; the step reads the members' cell words with ds_bpermute, forms the key and runs the
//     bounded probe loop of mapf_group_table.hpp over the open-addressing table in global memory.  STREAM is false.
//   EpisodeLimit  -- the episode step limit (include/mapf_hip.h mapf_set_episode_limit): the env's age is carried in a register
//     beside `terminal`, truncations are counted like episodes, the truncated byte is stored with the delayed flag bytes, and the
//     env goes back to its start cells on done OR truncated.  These instances have no DENSE form: always the guarded one.
//   EpisodeBudget -- the episode budget (include/mapf_hip.h mapf_set_episode_budget), behind the limit: a per-env count of episodes
//     left beside the age.  An env whose count is 0 is PARKED: it folds into the `terminal` the transition is told, so its step
//     draws and moves nothing, and its done bit is cleared before anything counts or records it.
//   EpisodeLog    -- the episode log (include/mapf_hip.h mapf_set_episode_log), behind the budget: the env's running return, its live
//     steps and its count of ended episodes are carried in the leader lane's registers as the age and the episodes left are, and a
//     step that reports done or truncated stores the finished episode's 16-byte record with ONE global store (while the env's count
//     is below the capacity).  The block itself waits in LDS, as the conflict matrix's does.  Budget instances only
//     (../csrc_log/mapf_lg_log.hip).
//   ConflictPairs -- the conflict matrix (include/mapf_hip.h mapf_set_conflict_pairs), last: the step's fast path is the one of the
//     instance without it; a wave in which some env's step collided then takes the attributed pass (lg_count_pairs below), which
//     finds the pairs the minima folded away and counts them with atomic adds.  Guarded instances only (pairs/mapf_lg_pairs.hip).
// A mode's sections are `if constexpr`: an instance without the mode compiles to the code it had when the modes were separate
// kernels (tools/compare_kernels.py, profiles/kernel_templates_device_listings.txt).  Which instances exist is each unit's say,
// through its family struct.
#pragma once
#include "mapf_lg.hpp"

namespace mapf {

// The attributed pass of a step under the conflict matrix: which agent pairs of (prev, next) conflict, counted into the env's
// slot of the matrix.  Entered by the WHOLE wave (the cross-lane reads need every lane) when some env of the wave reports a
// collision; only the lanes of such an env (`collided`) test and count.  The pair tests of pair_tests, unmerged: my own pair, then
// rotations 1 .. L/2 against group position og, whose agents 2og, 2og+1 are known; a ghost slot's index is n_agents or more and
// drops out by that (pair_apply masks the same slots).  A
// rotation below L/2 meets every lane pair once; the half rotation meets it from both sides (a group of two lanes has only that
// one), so there the lower position counts.  One rolled loop of ds_bpermute reads at every group size: this path runs on a few
// steps in a thousand, and a rolled loop keeps its registers out of the step loop's budget.
// Every hit is one 64-bit atomic add without a return value (relaxed, agent scope) on M[slot][min][max] (vertex) or
// M[slot][max][min] (swap): integer adds commute, so the matrix does not depend on the order the waves run in.
template <int L>
__device__ __forceinline__ void lg_count_pairs(const LaneCtx<L> &x, const uint32_t n_agents, const bool collided, const uint32_t e,
                                               const uint32_t cur0, const uint32_t cur1, const uint32_t next0, const uint32_t next1,
                                               const ConflictPairs &cp_lds) {
    using gu64 = __attribute__((address_space(1))) unsigned long long *;
    using gslot = const __attribute__((address_space(1))) uint32_t *;
    const ConflictPairs cp = cp_lds;   // (the kernel keeps the block in LDS; what it points to is global memory)
    // per-lane facts as integers, not wave masks: the step loop around this pass has no scalar register pair to spare
    uint32_t counting = collided ? 1u : 0u;
    asm volatile("" : "+v"(counting));
    // the slot is loaded here, not held across the step loop (a slot past the matrix -- the host has refused those -- is clamped)
    uint32_t slot_base = 0u;
    if (counting != 0u && cp.slot) slot_base = min(*(gslot)at(cp.slot, e), cp.n_slots - 1u) * n_agents * n_agents;
    const gu64 m = (gu64)cp.matrix + slot_base;
    // agents i and j (an index from n_agents on: a ghost slot, or a pair that the other side counts) with their cells
    auto count = [&](uint32_t i, uint32_t j, uint32_t prev_i, uint32_t next_i, uint32_t prev_j, uint32_t next_j) __attribute__((always_inline)) {
        const uint32_t lo = min(i, j), hi = max(i, j);
        const bool both = counting != 0u && hi < n_agents;
        if (both && next_i == next_j)   // vertex conflict (mapf_env.py:386-387): the upper triangle
            (void)__hip_atomic_fetch_add(m + (lo * n_agents + hi), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (both && prev_i == next_j && prev_j == next_i)   // swap (:382-384): the lower triangle
            (void)__hip_atomic_fetch_add(m + (hi * n_agents + lo), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    count(2u * x.g, 2u * x.g + 1u, cur0, next0, cur1, next1);
    if constexpr (L > 1) {
        const uint32_t pk_prev = cur0 | (cur1 << 16), pk_next = next0 | (next1 << 16);
#pragma unroll 1
        for (uint32_t s = 1; s <= uint32_t(L / 2); ++s) {
            const uint32_t og = (x.g + s) & uint32_t(L - 1);
            const int src = int(x.base + og);
            const uint32_t o_prev = uint32_t(__shfl(int(pk_prev), src, 64)), o_next = uint32_t(__shfl(int(pk_next), src, 64));
            const uint32_t j0 = (s < uint32_t(L / 2) || x.g < og) ? 2u * og : 0xFFFFu;   // the half rotation: the lower position counts
            count(2u * x.g, j0, cur0, next0, o_prev & 0xFFFFu, o_next & 0xFFFFu);
            count(2u * x.g, j0 + 1u, cur0, next0, o_prev >> 16, o_next >> 16);
            count(2u * x.g + 1u, j0, cur1, next1, o_prev & 0xFFFFu, o_next & 0xFFFFu);
            count(2u * x.g + 1u, j0 + 1u, cur1, next1, o_prev >> 16, o_next >> 16);
        }
    }
}

// a pointer every lane holds the same value of, moved into scalar registers (two v_readfirstlane)
template <class T>
__device__ __forceinline__ T *uniform_pointer(T *ptr) {
    const uint64_t bits = reinterpret_cast<uint64_t>(ptr);
    // (the builtin returns a signed int: each half goes through uint32_t, else a low word with bit 31 set sign-extends over the high one)
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(bits >> 32)))), lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(bits))));
    return reinterpret_cast<T *>((uint64_t(hi) << 32) | uint64_t(lo));
}

template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool DENSE, class... Extra>
__global__ void __launch_bounds__(rollout_max_block<L>()) lg_rollout_kernel(const RolloutArgs p, const uint32_t n_agents, const Extra... extra) {
    constexpr bool TABLE = has_kernel_arg<TablePolicy, Extra...>, LIMIT = has_kernel_arg<EpisodeLimit, Extra...>,
                   BUDGET = has_kernel_arg<EpisodeBudget, Extra...>, PAIRS = has_kernel_arg<ConflictPairs, Extra...>,
                   JOINT = has_kernel_arg<JointPolicy, Extra...>, LOG = has_kernel_arg<EpisodeLog, Extra...>,
                   GROUP = has_kernel_arg<GroupPolicy, Extra...>;
    static_assert(BUDGET || !LOG, "a log instance is a budget instance");
    static_assert(!(TABLE && STREAM), "a table instance runs the launches without streamed actions");
    static_assert(!(JOINT && (TABLE || STREAM || DENSE)), "a joint instance: no table policy beside it, no streamed actions, guarded");
    static_assert(!(GROUP && (TABLE || JOINT || STREAM || DENSE)), "a group instance: no other table policy beside it, no streamed actions, guarded");
    static_assert(!(LIMIT && DENSE) && (LIMIT || !BUDGET), "the limit instances are guarded; a budget instance takes the limit block too");
    static_assert(!(PAIRS && DENSE), "the instances that count conflicting pairs are guarded");
    const auto tp = kernel_arg<TablePolicy>(extra...);       // by value: an empty tag where the instance has no such argument
    const auto jp = kernel_arg<JointPolicy>(extra...);
    const auto gp = kernel_arg<GroupPolicy>(extra...);
    const auto lim = kernel_arg<EpisodeLimit>(extra...);
    const auto bud = kernel_arg<EpisodeBudget>(extra...);
    __shared__ SlipRow slip[8];
    __shared__ OutcomeRow outcome[16];
    // the conflict matrix's block waits in LDS (kPairsLdsBytes behind the table image: the planner leaves room), not in five scalar
    // registers across the step loop, which has none to spare: the attributed pass reads it back
    const ConflictPairs *cp = nullptr;
    if constexpr (PAIRS) {
        __shared__ ConflictPairs cp_lds;
        static_assert(sizeof(ConflictPairs) <= kPairsLdsBytes, "the room plan_rollout_lg leaves");
        if (threadIdx.x == 0u) cp_lds = kernel_arg<ConflictPairs>(extra...);   // (the staging below ends with __syncthreads())
        cp = &cp_lds;
    }
    // the episode log's block waits there too (kLogLdsBytes, planned likewise): a step that ends an episode reads where the record
    // goes, the launch's end where the partials and the counts lie -- no address of the log occupies a register across the step loop.
    // A log instance carries four registers per lane more than its budget instance (the running return, its steps, the count); it
    // gets them back, and more, from the addresses of the ages, the episodes left and their two totals, which wait here as well
    // and are formed again at the launch's end instead of being parked in eight VGPRs
    struct LogLds { EpisodeLog log; uint32_t *age, *out_truncations, *left, *out_live_steps; };
    const LogLds *lg = nullptr;
    if constexpr (LOG) {
        __shared__ LogLds lg_lds;
        static_assert(sizeof(LogLds) <= kLogLdsBytes, "the room plan_rollout_lg leaves");
        if (threadIdx.x == 0u) lg_lds = LogLds{kernel_arg<EpisodeLog>(extra...), lim.age, lim.out_truncations, bud.left, bud.out_live_steps};   // (the staging below ends with __syncthreads())
        lg = &lg_lds;
    }
    // the group policy's scalars wait there as well (kGroupLdsBytes, planned likewise): the step reads the two table addresses, the
    // mask and the probe bound back instead of holding six scalar registers across the step loop.  A group instance carries its
    // selectors, books and rows in five registers per lane and needs more in the probe; it gets them back from the addresses of the
    // totals, the ages and the episodes left, which wait here too and are formed again at the launch's end
    struct GroupLds {
        const uint8_t *table; const GroupSlot *slots; uint32_t mask, max_probe;
        double *out_returns; uint32_t *out_episodes, *out_collisions, *age, *out_truncations, *left, *out_live_steps;
    };
    const GroupLds *gl = nullptr;
    if constexpr (GROUP) {
        __shared__ GroupLds gl_lds;
        static_assert(sizeof(GroupLds) <= kGroupLdsBytes, "the room route_rollout leaves");
        if (threadIdx.x == 0u) {   // (the staging below ends with __syncthreads())
            GroupLds v{gp.table, gp.slots, gp.mask, gp.max_probe, p.out_returns, p.out_episodes, p.out_collisions, nullptr, nullptr, nullptr, nullptr};
            if constexpr (LIMIT) { v.age = lim.age; v.out_truncations = lim.out_truncations; }
            if constexpr (BUDGET) { v.left = bud.left; v.out_live_steps = bud.out_live_steps; }
            gl_lds = v;
        }
        gl = &gl_lds;
    }
    extern __shared__ __attribute__((aligned(16))) MoveEntry lds_mv[];
    bool live_rt;
    LaneCtx<L> x = lane_ctx<L>(n_agents, p.n_envs, live_rt);
    const bool live = DENSE || live_rt;
    if (DENSE) { x.v0 = true; x.v1 = true; }
    const uint32_t e = x.e;
    const bool leader = live && x.g == 0u;
    const bool tail = live && x.g == uint32_t(L - 1);   // holds the step's probability product

    uint32_t cur0, cur1, goal0, goal1, start0 = 0u, start1 = 0u;
    load_pair<uint16_t>(p.state, e, n_agents, x.g, x.v0, x.v1, cur0, cur1);
    load_pair<uint16_t>(p.goal, p.goal_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, goal0, goal1);
    if (p.auto_reset) load_pair<uint16_t>(p.start, p.start_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, start0, start1);
    if (MV_LDS) {   // batches of four independent loads per thread, then the four LDS writes (not load-wait-write)
        const uint32_t n_words = p.c.n_cells * kMvCols;
        for (uint32_t w0 = threadIdx.x; w0 < n_words; w0 += 4u * blockDim.x) {
            MoveEntry part[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t w = w0 + k * blockDim.x;
                part[k] = p.mv[w < n_words ? w : n_words - 1u];
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t w = w0 + k * blockDim.x;
                if (w < n_words) lds_mv[w] = part[k];
            }
        }
    }
    stage_outcome_table(p.c, outcome);
    stage_slip_table(p.slip, slip);   // ends with __syncthreads()
    const MoveEntry *mv = MV_LDS ? lds_mv : p.mv;

    // is_terminal is carried from step to step instead of re-deriving it from the cells every step
    uint32_t terminal = lg_is_terminal<L, FULL>(x, n_agents, cur0, cur1, goal0, goal1) ? 1u : 0u;   // an integer: no wave-mask phi
    const uint32_t start_terminal = (p.auto_reset && lg_is_terminal<L, FULL>(x, n_agents, start0, start1, goal0, goal1)) ? 1u : 0u;

    // per-env totals and the scalar trajectory arrays: their addresses are parked in VGPRs so that seven base
    // pointers do not occupy SGPRs across the step loop (it already keeps ~100 scalars live).  They stay typed as
    // GLOBAL pointers: a generic pointer would turn the stores into flat_store, which also counts on lgkmcnt and
    // would chain every LDS wait of the loop to the stores' completion.
    using gf64 = __attribute__((address_space(1))) double *;
    using gu32 = __attribute__((address_space(1))) uint32_t *;
    using gu8 = __attribute__((address_space(1))) uint8_t *;
    using gu16 = __attribute__((address_space(1))) uint16_t *;
    // (a GROUP instance uses these addresses, and those of the ages and the episodes left below, for the initial loads only: it
    // forms them again from its LDS block at the launch's end, so the values pinned here die before the step loop)
    gf64 ret_p = (gf64)(p.out_returns ? at(p.out_returns, e) : nullptr);
    gu32 epi_p = (gu32)(p.out_episodes ? at(p.out_episodes, e) : nullptr);
    gu32 col_p = (gu32)(p.out_collisions ? at(p.out_collisions, e) : nullptr);
    gu8 done_base = (gu8)(RECORD ? p.rec_done : nullptr), coll_base = (gu8)(RECORD ? p.rec_collision : nullptr);
    gf64 reward_base = (gf64)(RECORD ? p.rec_reward : nullptr), prob_base = (gf64)(RECORD ? p.rec_prob : nullptr);
    asm volatile("" : "+v"(ret_p), "+v"(epi_p), "+v"(col_p), "+v"(done_base), "+v"(coll_base), "+v"(reward_base),
                 "+v"(prob_base));
    double ret = (p.accumulate && ret_p && leader) ? *ret_p : 0.0;
    uint32_t episodes = (p.accumulate && epi_p && leader) ? *epi_p : 0u;
    uint32_t collisions = (p.accumulate && col_p && leader) ? *col_p : 0u;
    // what only a mode's sections use: dead, and gone from the code, in an instance without the mode
    gu32 age_p = nullptr, trn_p = nullptr, left_p = nullptr, liv_p = nullptr;
    gu8 trunc_lane = nullptr;
    uint32_t age = 0u, truncations = 0u, max_steps = 0u, left = 0u, live_steps = 0u;
    uint32_t idle = 0u;                        // budget: steps that were parked or terminal on entry: live steps = n_steps - idle
    if constexpr (LIMIT) {
        // the env's age: read once by every lane of the group (one address per group: each lane decides `back` itself), written
        // back once by the leader; lanes past the last env read env 0's and write nothing
        age_p = (gu32)at(lim.age, e);
        trn_p = (gu32)(lim.out_truncations ? at(lim.out_truncations, e) : nullptr);
        trunc_lane = (gu8)(RECORD ? lim.rec_truncated : nullptr) + e;      // the delayed step's row
        asm volatile("" : "+v"(age_p), "+v"(trn_p), "+v"(trunc_lane));
        age = *age_p;
        truncations = (p.accumulate && trn_p && leader) ? *trn_p : 0u;
        max_steps = lim.max_steps;
    }
    if constexpr (BUDGET) {
        // the env's episodes left: read and written back like the age (lanes past the last env are parked: they write nothing anyway)
        left_p = (gu32)at(bud.left, e);
        liv_p = (gu32)(bud.out_live_steps ? at(bud.out_live_steps, e) : nullptr);
        asm volatile("" : "+v"(left_p), "+v"(liv_p));
        left = live ? *left_p : 0u;
        live_steps = (p.accumulate && liv_p && leader) ? *liv_p : 0u;
    }
    // the episode log: the leader's partial episode (one 16-byte word) and the env's count, read once here and written back once at
    // the end like the age and the episodes left -- four registers across the step loop; the other lanes carry zeros and store nothing
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    using gw4 = __attribute__((address_space(1))) u32x4 *;
    double log_acc = 0.0;
    uint32_t log_len = 0u, log_count = 0u;
    if constexpr (LOG) {
        if (leader) {
            const EpisodeLog la = kernel_arg<EpisodeLog>(extra...);
            const u32x4 part = *(gw4)at(la.partial, e);
            log_acc = __hiloint2double(int(part.y), int(part.x));
            log_len = part.z;
            log_count = *(gu32)at(episode_log_counts(la.partial, p.n_envs), e);
        }
    }
    const uint64_t env_id = p.env_id_offset + e;
    const uint32_t n_envs = uint32_t(p.n_envs);

#ifdef MAPF_STAMPS
    StampCtx st{};
    { unsigned long long _t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); st.last = _t; }
#endif
    // Software pipeline of the loop's memory operations.  The compiler waits for the prefetched action word with
    // vmcnt(0), i.e. for EVERYTHING outstanding, so each iteration is ordered: (1) use the word loaded one
    // iteration ago, (2) only then issue the next load and the PREVIOUS step's trajectory stores, (3) compute.
    // Whatever the wait at (1) sees was issued a whole transition earlier and has long completed.
    uint32_t raw = 0u;
    if (STREAM && p.n_steps > 0) raw = load_actions_raw<FULL>(p.actions, e, n_agents, x.g, x.v0, x.v1);
    // consume the first word here, so that the wait at the loop head is the back edge's counted one
    if (DENSE) asm volatile("" : "+v"(raw));
    Words4 rng{0u, 0u, 0u, 0u}, pol{0u, 0u, 0u, 0u};   // the slip / policy words of the current four-step block
    // step s-1's results, stored during step s (DENSE: the very first store writes zeros into step 0's row, which
    // step 1 then overwrites with the real values)
    uint32_t d_next0 = 0u, d_next1 = 0u, d_flags = 0u;
    double d_reward = 0.0, d_prob = 0.0;
    // Addresses advance by one step's worth of elements per iteration (wave-uniform strides added to per-lane
    // pointers) -- no per-step row * width multiplications.
    const uint64_t step_rows = n_envs, step_cells = uint64_t(n_envs) * n_agents;
    const bool odd = (x.g & 1u) != 0u;
    const uint32_t flag_shift = (x.g & 1u) * 8u;
    const uint32_t lane_cell = e * n_agents + 2u * x.g;
    gf64 reward_lane = reward_base + e, prob_lane = prob_base + e;      // the delayed step's row
    gu8 done_lane = done_base + e, coll_lane = coll_base + e;
    gu16 rec_lane = (gu16)(RECORD ? p.rec_local : nullptr) + lane_cell;
    const bool wide_is_prob = x.g == uint32_t(L - 1);   // the probability product ends in the group's last lane
    if (DENSE && L > 1) {   // last lane writes prob, the others reward; even lanes write done, odd lanes collision
        reward_lane = wide_is_prob ? prob_lane : reward_lane;
        done_lane = odd ? coll_lane : done_lane;
    }
    asm volatile("" : "+v"(reward_lane), "+v"(prob_lane), "+v"(done_lane), "+v"(coll_lane), "+v"(rec_lane));

    auto store_record = [&]() __attribute__((always_inline)) {
        const uint32_t cells = d_next0 | (d_next1 << 16);
        if (DENSE) {
            *(gu32)rec_lane = cells;
            *reward_lane = (L > 1 && wide_is_prob) ? d_prob : d_reward;
            *done_lane = uint8_t(L > 1 ? d_flags >> flag_shift : d_flags);   // flag_shift: 8 in odd lanes
            if (L == 1) {
                *prob_lane = d_prob;
                *coll_lane = uint8_t(d_flags >> 8);
            }
        } else {
            if (FULL || (n_agents & 1u) == 0u) {
                if (x.v0) *(gu32)rec_lane = cells;
            } else {
                if (x.v0) rec_lane[0] = uint16_t(d_next0);
                if (x.v1) rec_lane[1] = uint16_t(d_next1);
            }
            if (tail) *prob_lane = d_prob;
            if (leader) {
                *reward_lane = d_reward;
                *done_lane = uint8_t(d_flags & 1u);
                *coll_lane = uint8_t(d_flags >> 8);
                if constexpr (LIMIT) *trunc_lane = uint8_t(d_flags >> 24);   // byte 3 truncated
            }
        }
    };
    auto advance_record = [&]() __attribute__((always_inline)) {
        rec_lane += step_cells;
        reward_lane += step_rows;
        done_lane += step_rows;
        if (!(DENSE && L > 1)) { prob_lane += step_rows; coll_lane += step_rows; }
        if constexpr (LIMIT) trunc_lane += step_rows;
    };
    const uint8_t *act_lane = STREAM ? p.actions + lane_cell : nullptr;   // the row being prefetched

    uint32_t goal_rc0 = 0u, goal_rc1 = 0u;   // greedy policy: my agents' goal coordinates
    if (!STREAM && p.policy_cells) { goal_rc0 = p.policy_cells[goal0].x; goal_rc1 = p.policy_cells[goal1].x; }

    uint32_t row_base0 = 0u, row_base1 = 0u;   // table policy: my agents' rows (ghost slots: row 0, whose bytes are never used)
    if constexpr (TABLE) {
        load_pair<uint16_t>(tp.rows, tp.rows_broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, row_base0, row_base1);
        row_base0 *= p.c.n_cells;
        row_base1 *= p.c.n_cells;
    }

    // joint table policy: per agent the segment's base, the row stride (V merged, 0 solo) and the selector: the lane that holds
    // the partner's cell | the half of that lane's cell word << 10 (so that sel >> 6 is the shift, 0 or 16; __shfl keeps the low
    // six bits).  A solo agent is its own partner: base + cur * 0 + its own cell.  Ghost slots and the lanes past the last env are
    // solo on offset 0 (their cell is 0: byte 0, never used).  Integers in VGPRs: the step loop has no scalar registers to spare
    uint32_t jbase0 = 0u, jbase1 = 0u, jstride0 = 0u, jstride1 = 0u, jsel0 = 0u, jsel1 = 0u;
    if constexpr (JOINT) {
        const uint32_t me0 = 2u * x.g, me1 = 2u * x.g + 1u, jrow = (jp.broadcast ? 0u : e) * n_agents + me0;
        uint32_t partner0, partner1;
        load_pair<uint16_t>(jp.partner, jp.broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, partner0, partner1);
        if (x.v0) jbase0 = *at(jp.offset, jrow);
        if (x.v1) jbase1 = *at(jp.offset, jrow + 1u);
        // (a partner the host has refused -- not below A -- would name a lane outside the group: such an agent is solo here)
        partner0 = (x.v0 && partner0 < n_agents) ? partner0 : me0;
        partner1 = (x.v1 && partner1 < n_agents) ? partner1 : me1;
        jstride0 = partner0 != me0 ? p.c.n_cells : 0u;
        jstride1 = partner1 != me1 ? p.c.n_cells : 0u;
        jsel0 = (x.base + (partner0 >> 1)) | ((partner0 & 1u) << 10);
        jsel1 = (x.base + (partner1 >> 1)) | ((partner1 & 1u) << 10);
        asm volatile("" : "+v"(jbase0), "+v"(jbase1), "+v"(jstride0), "+v"(jstride1), "+v"(jsel0), "+v"(jsel1));
    }

    // group policy: per agent the row's base, the group's book (kGroupEmptyBook: none -- a solo agent, a ghost slot, a lane past the
    // last env) and one register of selectors: bits 7k .. 7k+6 name the lane that holds member k's cell (6 bits) and the half of that
    // lane's cell word (bit 6), bits 28-29 the agent's own position in the list, bits 30-31 the group's size - 1.  Positions past the
    // group's size select the agent's own lane; their cell in the key is 0xFFFF.  (A list the host has refused -- a member not below A,
    // a list without the agent -- leaves the agent on its row.)  Integers in VGPRs, as the joint policy's
    uint32_t grows = 0u, gbook0 = kGroupEmptyBook, gbook1 = kGroupEmptyBook, gsel0 = 0u, gsel1 = 0u;
    if constexpr (GROUP) {
        uint32_t grow0, grow1;   // (both rows in one register: row0 | row1 << 16; ghost slots: row 0, whose bytes are never used)
        load_pair<uint16_t>(gp.rows, gp.broadcast ? 0 : e, n_agents, x.g, x.v0, x.v1, grow0, grow1);
        grows = grow0 | (grow1 << 16);
        auto prepare = [&](const bool valid, const uint32_t me, uint32_t &book, uint32_t &sel) __attribute__((always_inline)) {
            const uint32_t self = (x.base + (me >> 1)) | ((me & 1u) << 6);
            sel = self * 0x204081u;   // self at bits 0, 7, 14 and 21
            if (!valid) return;
            const uint32_t idx = (gp.broadcast ? 0u : e) * n_agents + me;
            const uint2 w = *reinterpret_cast<const uint2 *>(at(gp.members, idx * 4u));   // (four u16: 8 bytes, 8-byte aligned)
            const uint32_t member[4] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
            uint32_t size = 0u, pos = 4u;
            bool open = true;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                open = open && member[k] < n_agents;
                if (open) {
                    ++size;
                    sel = (sel & ~(0x7Fu << (7u * k))) | (((x.base + (member[k] >> 1)) | ((member[k] & 1u) << 6)) << (7u * k));
                    if (member[k] == me) pos = k;
                }
            }
            if (size >= 2u && pos < 4u) book = *at(gp.book, idx);
            sel |= ((pos & 3u) << 28) | ((max(size, 1u) - 1u) << 30);
        };
        prepare(x.v0, 2u * x.g, gbook0, gsel0);
        prepare(x.v1, 2u * x.g + 1u, gbook1, gsel1);
        asm volatile("" : "+v"(grows), "+v"(gbook0), "+v"(gbook1), "+v"(gsel0), "+v"(gsel1));
    }

    const uint64_t t_first = first_step_index(p);
    for (uint32_t s = 0; s < p.n_steps; ++s) {
        const uint64_t t = t_first + s;
        // budget: a parked step is the terminal no-op: nothing drawn, nothing moved ...
        const bool parked = BUDGET && left == 0u;
        const bool no_op = parked || terminal != 0u;
        uint32_t act0, act1;
        if (STREAM) {
            act0 = raw & 0xFFu; act1 = (raw >> 8) & 0xFFu;   // only the low half-word of `raw` is defined
            asm volatile("" : "+v"(act0), "+v"(act1));       // (1) pins the wait for `raw` here, ahead of (2)
            if (DENSE) {                                     // clamped, not guarded: the last step re-reads its own row
                act_lane += (s + 1u < p.n_steps) ? step_cells : 0u;
                raw = *reinterpret_cast<const uint16_t *>(act_lane);
            } else if (s + 1 < p.n_steps) {
                act_lane += step_cells;
                raw = load_actions_raw<FULL>(act_lane, 0u, 0u, 0u, x.v0, x.v1);
            }
        } else if constexpr (TABLE) {   // table policy: the byte of (my row, my cell) -- ghost slots read byte 0 of row 0
            act0 = tp.table[row_base0 + cur0];
            act1 = tp.table[row_base1 + cur1];
        } else if constexpr (JOINT) {   // joint table policy: the byte of (my segment, my cell, my partner's cell)
            // every lane is active here (the loop bound is the wave's): the cross-lane read needs that.  The partner lane is a run-time
            // value, so ds_bpermute (no DPP control word fits); a group of one lane holds both cells itself
            const uint32_t pk = cur0 | (cur1 << 16);
            uint32_t o0 = pk, o1 = pk;
            if constexpr (L > 1) {
                o0 = uint32_t(__shfl(int(pk), int(jsel0), 64));
                o1 = uint32_t(__shfl(int(pk), int(jsel1), 64));
            }
            act0 = jp.table[jbase0 + cur0 * jstride0 + ((o0 >> (jsel0 >> 6)) & 0xFFFFu)];
            act1 = jp.table[jbase1 + cur1 * jstride1 + ((o1 >> (jsel1 >> 6)) & 0xFFFFu)];
        } else if constexpr (GROUP) {   // group policy: the byte of the entry of (my group's book, its members' cells), else of (my row, my cell)
            // the row bytes first: their latency overlaps the probe.  Every lane is active here, as the cross-lane reads need it; the
            // probe loop behind them is plain divergent code without a cross-lane operation: only the agents with a book enter it
            using gslot = const __attribute__((address_space(1))) u32x4 *;   // (one probe: one global_load_dwordx4)
            using gbyte = const __attribute__((address_space(1))) uint8_t *;
            const uint32_t pk = cur0 | (cur1 << 16);
            // (the block is the same for every lane: the addresses and the two integers go through scalar registers for the section only)
            const GroupLds g = *gl;
            const gbyte g_table = (gbyte)uniform_pointer(g.table);
            const gslot g_slots = (gslot)uniform_pointer(g.slots);
            const uint32_t g_mask = __builtin_amdgcn_readfirstlane(g.mask), g_max_probe = __builtin_amdgcn_readfirstlane(g.max_probe);
            const uint32_t row_act0 = g_table[(grows & 0xFFFFu) * p.c.n_cells + cur0], row_act1 = g_table[(grows >> 16) * p.c.n_cells + cur1];
            auto group_action = [&](uint32_t sel, const uint32_t book, const uint32_t row_act) __attribute__((always_inline)) {
                // (opaque here, so that the four lane addresses and shifts are extracted in the step and not hoisted out of the loop
                // into eight registers per agent)
                asm volatile("" : "+v"(sel));
                uint32_t cell[4];
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    uint32_t w = pk;   // (a group of one lane holds both cells itself)
                    if constexpr (L > 1) w = uint32_t(__shfl(int(pk), int((sel >> (7u * k)) & 63u), 64));
                    cell[k] = (w >> (((sel >> (7u * k + 6u)) & 1u) * 16u)) & 0xFFFFu;
                    if (k > (sel >> 30)) cell[k] = kGroupPad;
                }
                uint32_t act = row_act;
                if (book != kGroupEmptyBook) {
                    const uint32_t found = group_lookup([&](uint32_t i) { const u32x4 s = g_slots[i]; return GroupSlot{s.x, s.y, s.z, s.w}; },
                                                        g_mask, g_max_probe, cell[0] | (cell[1] << 16), cell[2] | (cell[3] << 16), book);
                    // (an entry's bytes are 0..4: the host has checked them; min: a wrong table still indexes the move table in bounds)
                    if (found != kGroupMiss) act = min((found >> (((sel >> 28) & 3u) * 8u)) & 0xFFu, 4u);
                }
                return act;
            };
            act0 = group_action(gsel0, gbook0, row_act0);
            act1 = group_action(gsel1, gbook1, row_act1);
        } else if (p.policy_cells) {   // greedy policy (ghost slots read cell 0: their actions are never used)
            act0 = greedy_action(p.policy_cells, p.c.n_cells, cur0, goal_rc0);
            act1 = greedy_action(p.policy_cells, p.c.n_cells, cur1, goal_rc1);
        } else {   // policy stream: one Philox call covers agents 4q..4q+3 for the four steps of a block; this lane's
            // agents are bytes 2(g&1), 2(g&1)+1 of the step's word
            if ((t & 3u) == 0u || s == 0u) pol = policy_words(p.c, env_id, t >> 2, x.g >> 1);
            const uint32_t mine = step_word(pol, t) >> (16u * (x.g & 1u));
            act0 = policy_action_rt(mine, 0u);
            act1 = policy_action_rt(mine, 1u);
        }
        if (RECORD && (DENSE || s > 0)) {                    // (2) the previous step's outputs
            store_record();
            if (!DENSE || s > 0) advance_record();
        }
        uint32_t next0, next1;
        EnvOut o;
        STAMP(0);   // loop top: action fetch / policy / delayed stores
        // my pair's words of a four-step block (one slip-stream call per lane, traded with the neighbour lane): refresh when
        // t is a multiple of 4 (and at the first step)
        if (p.c.need_rng && ((t & 3u) == 0u || s == 0u)) rng = pair_block_words<(L > 1)>(p.c, env_id, t, x.g);
        lg_transition<L, FULL, false, true, MV_LDS, true>(p.c, mv, slip, outcome, x, n_agents, cur0, cur1, goal0, goal1, act0, act1, 0.0, 0.0,
                                            env_id, t, step_word(rng, t), no_op, next0, next1, o STAMP_ARG);
        if constexpr (PAIRS) {
            // status byte 1 is the collision of a step that was not a no-op (a no-op reports kTerminalStatus).  __any: the branch is
            // the wave's, as the cross-lane reads of the pass need it; cur and next are still the cells on entry and the sampled ones
            const bool collided = live && (o.status & 0xFF00u) != 0u;
            if (__builtin_expect(__any(collided), 0)) lg_count_pairs<L>(x, n_agents, collided, e, cur0, cur1, next0, next1, *cp);
        }
        if constexpr (BUDGET) {
            // ... but it reports no done: a no-op's status is kTerminalStatus, whose byte 0 goes and whose byte 2 stays (the carried `terminal`
            // is 1 from here on).  Its reward is +0.0, and ret + 0.0 would turn an accumulated -0.0 into +0.0: what is added is -0.0
            o.status -= parked ? 1u : 0u;
            ret = __dadd_rn(ret, __hiloint2double(parked ? int(0x80000000u) : __double2hiint(o.reward), __double2loint(o.reward)));
        } else {
            STAMP(6);   // reward / selects
            ret = __dadd_rn(ret, o.reward);
        }
        episodes += o.status & 0xFFu;
        collisions += (o.status >> 8) & 0xFFu;
        if (RECORD) {
            d_next0 = next0; d_next1 = next1; d_reward = o.reward; d_prob = o.prob;
            d_flags = o.status;                            // byte 0 done, byte 1 collision
        }
        bool back;
        if constexpr (LIMIT) {
            uint32_t aged, truncated;
            if constexpr (BUDGET) {
                // the limit's rules below, switched off as a whole by max_steps == 0 (a budget without a limit: the ages stay zero); a step
                // that was neither parked nor terminal on entry is a live step, and one that reports done or truncated takes an episode
                // from the env's count (a parked step reports neither, so the count stops at 0)
                const bool ageing = !no_op && max_steps != 0u;
                aged = ageing ? (age + (age != 0xFFFFFFFFu ? 1u : 0u)) : age;
                truncated = (ageing && (o.status & 0xFFu) == 0u && aged >= max_steps) ? 1u : 0u;
                idle += no_op ? 1u : 0u;
            } else {
                // a live step ages the episode (saturating); it is truncated when it did not end the episode and the age has reached
                // the limit.  A step from a terminal state (a no-op) leaves the age alone and is never truncated.
                aged = terminal != 0u ? age : (age + (age != 0xFFFFFFFFu ? 1u : 0u));
                truncated = (terminal == 0u && (o.status & 0xFFu) == 0u && aged >= max_steps) ? 1u : 0u;
            }
            truncations += truncated;
            if (RECORD) d_flags |= truncated << 24;
            back = p.auto_reset && ((o.status & 0xFFu) != 0u || truncated != 0u);   // done or truncated: start cells, age 0
            age = back ? 0u : aged;
            if constexpr (BUDGET) left -= back ? 1u : 0u;   // (the budget instances run auto-reset launches only: back == done || truncated)
            if constexpr (LOG) {
                // the running episode takes the step's reward (a parked step: -0.0, which changes no sum; a terminal-on-entry no-op its
                // +0.0) and, if the step was live, one step; a step that ends it (never a parked one: `back` is false there) stores
                // the record while the env has room, counts it, and begins the next episode from +0.0
                log_acc = __dadd_rn(log_acc, __hiloint2double(parked ? int(0x80000000u) : __double2hiint(o.reward), __double2loint(o.reward)));
                log_len += no_op ? 0u : 1u;
                if (back) {
                    // (index e * C + count < E * C: the host keeps E * C * 16 within 2^31 bytes, so the byte offset fits 32 bits)
                    if (const uint32_t cap = lg->log.capacity; leader && log_count < cap) {
                        const uint32_t how = (o.status & 1u) | ((o.status >> 7) & 2u) | (truncated << 2);   // done | collision << 1 | truncated << 2
                        *(gw4)at(lg->log.records, e * cap + log_count) = u32x4{uint32_t(__double2loint(log_acc)), uint32_t(__double2hiint(log_acc)), log_len, how};
                    }
                    log_count += log_count != 0xFFFFFFFFu ? 1u : 0u;
                    log_acc = 0.0;
                    log_len = 0u;
                }
            }
        } else {
            back = p.auto_reset && (o.status & 0xFFu) != 0u;   // MapfEnv.reset(): start cells, no reseed
        }
        cur0 = back ? start0 : next0;
        cur1 = back ? start1 : next1;
        terminal = back ? start_terminal : (o.status >> 16);
        STAMP(7);   // reset handling
    }
    if (RECORD && p.n_steps > 0) store_record();             // flush the last step's outputs
#ifdef MAPF_STAMPS
    if (live && x.lane == 0u && epi_p) {   // diagnostic build: segment sums replace the episode counts
        for (int k = 0; k < 8; ++k) epi_p[k] = uint32_t(st.seg[k]);
        return;
    }
#endif
    if (!live) return;
    store_cells<FULL>(p.state, e, n_agents, x.g, x.v0, x.v1, cur0, cur1);
    if (leader) {
        if constexpr (GROUP) {   // (the addresses the step loop did not carry)
            ret_p = (gf64)(gl->out_returns ? at(gl->out_returns, e) : nullptr);
            epi_p = (gu32)(gl->out_episodes ? at(gl->out_episodes, e) : nullptr);
            col_p = (gu32)(gl->out_collisions ? at(gl->out_collisions, e) : nullptr);
            if constexpr (LIMIT && !LOG) {
                age_p = (gu32)at(gl->age, e);
                trn_p = (gu32)(gl->out_truncations ? at(gl->out_truncations, e) : nullptr);
            }
            if constexpr (BUDGET && !LOG) {
                left_p = (gu32)at(gl->left, e);
                liv_p = (gu32)(gl->out_live_steps ? at(gl->out_live_steps, e) : nullptr);
            }
        }
        if constexpr (LOG) {   // (the addresses the step loop did not carry)
            age_p = (gu32)at(lg->age, e);
            trn_p = (gu32)(lg->out_truncations ? at(lg->out_truncations, e) : nullptr);
            left_p = (gu32)at(lg->left, e);
            liv_p = (gu32)(lg->out_live_steps ? at(lg->out_live_steps, e) : nullptr);
        }
        if (ret_p) *ret_p = ret;
        if (epi_p) *epi_p = episodes;
        if (col_p) *col_p = collisions;
        if constexpr (LIMIT) {
            *age_p = age;
            if (trn_p) *trn_p = truncations;
        }
        if constexpr (BUDGET) {
            *left_p = left;
            if (liv_p) *liv_p = live_steps + (p.n_steps - idle);
        }
        if constexpr (LOG) {
            EpisodeLogPartial *const partial = lg->log.partial;
            *(gw4)at(partial, e) = u32x4{uint32_t(__double2loint(log_acc)), uint32_t(__double2hiint(log_acc)), log_len, 0u};
            *(gu32)at(episode_log_counts(partial, p.n_envs), e) = log_count;
        }
    }
}

}  // namespace mapf
