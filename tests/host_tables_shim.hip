// Test shim (tests/test_host_tables.py): a C face on the host-only units of the library -- the table builders
// (mapf_tables.hip) and the launch planner (mapf_plan.hip) -- so that they can be driven through ctypes without a
// device.  Test code, compiled into the test's tmp dir; not part of libmapf_hip.so.
#include "mapf_plan.hpp"
#include "mapf_tables.hpp"

#include <cstdio>
#include <cstring>

using namespace mapf;

extern "C" {

// [0] kMvCols, [1] kDeltaCols, [2] kDeltaRowBias, [3] sizeof(SlipRow), [4] sizeof(OutcomeRow), [5] delta_table_words(V)
void shim_sizes(uint32_t V, uint64_t out[6]) {
    out[0] = kMvCols; out[1] = kDeltaCols; out[2] = kDeltaRowBias; out[3] = sizeof(SlipRow); out[4] = sizeof(OutcomeRow);
    out[5] = delta_table_words(V);
}

// rows: 8 SlipRows; consts: p_cand[3]; flags: need_rng, top_tie.  1 = built, 0 = refused
int shim_slip_tables(double fail_prob, void *rows, double *p_cand, uint32_t *flags) {
    SlipRow slip[8];
    EnvConsts c{};
    std::string err;
    if (!build_slip_tables(fail_prob, slip, &c, &err)) return 0;
    std::memcpy(rows, slip, sizeof(slip));
    std::memcpy(p_cand, c.p_cand, sizeof(c.p_cand));
    flags[0] = c.need_rng; flags[1] = c.top_tie;
    return 1;
}

void shim_outcome_rows(double r_clash, double r_goal, double r_living, void *rows) {
    EnvConsts c{};
    c.r_clash = r_clash; c.r_goal = r_goal; c.r_living = r_living;
    OutcomeRow out[16];
    build_outcome_rows(c, out);
    std::memcpy(rows, out, sizeof(out));
}

uint32_t shim_outcome_status(uint32_t f) { return outcome_status(f); }

// mv: u32[V * kMvCols * 4], mv8: u32[V * kMvCols * 2], mv4: u32[delta_table_words(V)] (written only when the result is 1)
int shim_move_tables(const uint16_t *nbr, uint32_t V, double fail_prob, uint32_t *mv, uint32_t *mv8, uint32_t *mv4) {
    SlipRow slip[8];
    EnvConsts c{};
    std::string err;
    if (!build_slip_tables(fail_prob, slip, &c, &err)) return -1;
    const MoveTables t = build_move_tables(nbr, V, fail_prob, slip);
    if (t.mv.size() != size_t(V) * kMvCols || t.mv8.size() != t.mv.size() || t.mv4.size() != (t.delta8 ? delta_table_words(V) : 0u)) return -2;
    std::memcpy(mv, t.mv.data(), t.mv.size() * sizeof(MoveEntry));
    std::memcpy(mv8, t.mv8.data(), t.mv8.size() * sizeof(CompactEntry));
    if (t.delta8) std::memcpy(mv4, t.mv4.data(), t.mv4.size() * sizeof(uint32_t));
    return t.delta8 ? 1 : 0;
}

// scen: u8[E], rows: u16[256 * 2 * A]; returns the number of pairs (0 = no table)
uint32_t shim_scen_table(const uint16_t *start, int start_broadcast, const uint16_t *goal, int goal_broadcast, uint64_t E, uint32_t A, uint8_t *scen,
                         uint16_t *rows) {
    const ScenTable t = build_scen_table(start, start_broadcast != 0, goal, goal_broadcast != 0, E, A);
    if (t.n == 0) return (t.scen.empty() && t.rows.empty()) ? 0u : ~0u;
    if (t.scen.size() != E || t.rows.size() != size_t(t.n) * 2 * A || t.n > 256u) return ~0u;
    std::memcpy(scen, t.scen.data(), t.scen.size());
    std::memcpy(rows, t.rows.data(), t.rows.size() * sizeof(uint16_t));
    return t.n;
}

// cells: u32[V * 2] (cell_rc, nine 3-bit actions); 1 = built, 0 = refused (err receives the text)
int shim_greedy_cells(const uint16_t *nbr, uint32_t V, const uint32_t *cell_rc, uint32_t *cells, char *err, size_t err_cap) {
    std::vector<uint2> out;
    std::string why;
    if (!build_greedy_cells(nbr, V, cell_rc, &out, &why)) {
        std::snprintf(err, err_cap, "%s", why.c_str());
        return 0;
    }
    std::memcpy(cells, out.data(), out.size() * sizeof(uint2));
    return 1;
}

// (what the two entries below share: 1 = a packed form, 0 = none, -1 = bad tune)
static int step_lq(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, int n_cu, const char *tune, StepPlan *plan) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    static const uint32_t present = 0;
    StepArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    args.mv4 = has_delta_rows ? &present : nullptr;
    return plan_step_lq(n_agents, args, t, plan) ? 1 : 0;
}
// plan_step_lq over a shape: out = K, Q, form (StepForm's number), block, grid, n_chunks, lds_bytes, lds_limit
int shim_plan_step(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, int n_cu, const char *tune, uint64_t out[8]) {
    StepPlan plan;
    const int rc = step_lq(n_cells, n_agents, n_envs, has_delta_rows, n_cu, tune, &plan);
    if (rc != 1) return rc;
    out[0] = uint64_t(plan.K); out[1] = uint64_t(plan.Q); out[2] = uint64_t(int(plan.big)); out[3] = plan.block; out[4] = plan.grid;
    out[5] = plan.n_chunks; out[6] = plan.lds_bytes; out[7] = uint64_t(plan.lds_limit);
    return 1;
}
// ... and the name the launcher notes for that plan (kKernelNameBytes)
int shim_lq_step_name(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, int n_cu, const char *tune, int scen, int may_be_terminal, char *name) {
    StepPlan plan;
    const int rc = step_lq(n_cells, n_agents, n_envs, has_delta_rows, n_cu, tune, &plan);
    if (rc == 1) lq_step_kernel_name(name, plan, scen != 0, may_be_terminal != 0);
    return rc;
}
// does the launcher hold the packed step instance (K, Q, form)?
int shim_step_instance_exists(int K, int Q, int form) { return form >= 0 && form <= 3 && lq_step_instance_exists(K, Q, StepForm(form)) ? 1 : 0; }

// (only the fields a rollout plan reads: the shape, and which optional arrays are present -- never dereferenced)
static RolloutArgs rollout_shape(uint32_t n_cells, uint64_t n_envs, uint32_t n_steps, int has_delta_rows, bool streamed) {
    static const uint32_t present = 0;
    RolloutArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    args.n_steps = n_steps;
    args.actions = streamed ? reinterpret_cast<const uint8_t *>(&present) : nullptr;
    args.mv_delta8 = has_delta_rows != 0;
    args.mv4 = has_delta_rows ? &present : nullptr;
    return args;
}

// plan_rollout_lq_table over a shape (a launch without streamed actions, under a policy table of table_bytes; limited: under an
// episode step limit with limit_packed=1): out = K, Q, form, block, lds_bytes, lds_total, table_lds, table_at, limit;
// 1 = a packed table instance, 0 = none, -1 = bad tune; *limit_packed (may be null) = what the tune string says of the key
int shim_plan_rollout_table(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int has_delta_rows, uint64_t table_bytes, int n_cu,
                            const char *tune, int limited, uint64_t out[9], int *limit_packed) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    if (limit_packed) *limit_packed = t.limit_packed ? 1 : 0;
    LqPlan plan;
    if (!plan_rollout_lq_table(n_agents, rollout_shape(n_cells, n_envs, n_steps, has_delta_rows, false), t, size_t(table_bytes), &plan, limited != 0)) return 0;
    out[0] = uint64_t(plan.K); out[1] = uint64_t(plan.Q); out[2] = uint64_t(int(plan.form)); out[3] = plan.block; out[4] = plan.lds_bytes;
    out[5] = plan.lds_total; out[6] = plan.table_lds ? 1u : 0u; out[7] = plan.table_at; out[8] = plan.limit ? 1u : 0u;
    return 1;
}

// The packed plan of a one-step launch as route_rollout makes it (policy: 0 streamed actions, 1 the in-kernel policy, 2 the
// table policy of table_bytes; limited: ... under an episode step limit) and the name the launcher notes for it (kKernelNameBytes);
// 1 = planned, 0 = no packed form, -1 = bad tune
int shim_lq_rollout_name(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, uint64_t table_bytes, int n_cu, const char *tune, int policy,
                         int limited, int record, int soc, int may_be_terminal, char *name) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    const RolloutArgs args = rollout_shape(n_cells, n_envs, 1, has_delta_rows, policy == 0);
    LqPlan plan;
    if (policy == 2 ? !plan_rollout_lq_table(n_agents, args, t, size_t(table_bytes), &plan, limited != 0) : !plan_rollout_lq(n_agents, args, t, &plan)) return 0;
    lq_rollout_kernel_name(name, plan, record != 0, policy == 0, policy == 2, soc != 0, may_be_terminal != 0, uint32_t(table_bytes));
    return 1;
}

// (what the two entries below share; limited: the plan of a launch under an episode step limit)
static int rollout_lg(uint32_t n_cells, int n_agents, uint64_t n_envs, int record, int policy, const char *tune, bool limited, uint64_t out[7], char *name) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(256, tune, &err);
    if (!err.empty()) return -1;
    RolloutArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    const LgRolloutPlan plan = plan_rollout_lg(n_agents, args, t, limited);
    out[0] = uint64_t(plan.L); out[1] = plan.full ? 1u : 0u; out[2] = plan.mv_lds ? 1u : 0u; out[3] = plan.dense ? 1u : 0u; out[4] = plan.block;
    out[5] = plan.grid; out[6] = plan.lds_bytes;
    lg_rollout_kernel_name(name, plan, record != 0, policy == 0, policy == 2);
    return 1;
}
// plan_rollout_lg over a shape (policy: 0 streamed actions, 1 the in-kernel policy stream, 2 the table policy): out = L, full, mv_lds, dense,
// block, grid, lds_bytes; name (kKernelNameBytes) = what the launcher notes for that plan; 1 = planned, -1 = bad tune
int shim_plan_rollout_lg(uint32_t n_cells, int n_agents, uint64_t n_envs, int record, int policy, const char *tune, uint64_t out[7], char *name) {
    return rollout_lg(n_cells, n_agents, n_envs, record, policy, tune, false, out, name);
}
// ... under an episode step limit: the plan that names the limit instance
int shim_plan_limit_rollout_lg(uint32_t n_cells, int n_agents, uint64_t n_envs, int record, int policy, const char *tune, uint64_t out[7], char *name) {
    return rollout_lg(n_cells, n_agents, n_envs, record, policy, tune, true, out, name);
}

// (likewise for the single step)
static int step_lg(int n_agents, uint64_t n_envs, int ext_uniforms, bool limited, uint64_t out[4], char *name) {
    StepArgs args{};
    args.n_envs = n_envs;
    const LgStepPlan plan = plan_step_lg(n_agents, args, limited);
    out[0] = uint64_t(plan.L); out[1] = plan.full ? 1u : 0u; out[2] = plan.block; out[3] = plan.grid;
    lg_step_kernel_name(name, plan, ext_uniforms != 0);
    return 1;
}
// plan_step_lg: out = L, full, block, grid; name as above
int shim_plan_step_lg(int n_agents, uint64_t n_envs, int ext_uniforms, uint64_t out[4], char *name) { return step_lg(n_agents, n_envs, ext_uniforms, false, out, name); }
// ... under an episode step limit
int shim_plan_limit_step_lg(int n_agents, uint64_t n_envs, int ext_uniforms, uint64_t out[4], char *name) { return step_lg(n_agents, n_envs, ext_uniforms, true, out, name); }

// route_rollout over a one-step launch (prefer: FamilyPreference's number -- 0 auto, 1 thread-per-env, 2 lane-group; policy: 0 streamed
// actions, 1 the in-kernel policy, 2 the table policy of table_bytes; limited / budgeted: under an episode step limit / budget):
// returns the family (KernelFamily's number: 0 thread-per-env, 1 packed, 2 lane-group; -1 = bad tune), its plan in the layout of the
// entries above -- thread-per-env: block, grid; packed: shim_plan_rollout_table's nine; lane-group: shim_plan_rollout_lg's seven, then
// limit, budget -- and the name its launcher notes (kKernelNameBytes)
int shim_route_rollout(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, uint64_t table_bytes, int n_cu, const char *tune, int prefer, int policy,
                       int limited, int budgeted, int record, int soc, int may_be_terminal, uint64_t out[9], char *name) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    const RolloutRoute r = route_rollout(n_agents, rollout_shape(n_cells, n_envs, 1, has_delta_rows, policy == 0), t, FamilyPreference(prefer), policy == 2,
                                         size_t(table_bytes), limited != 0, budgeted != 0);
    std::memset(out, 0, 9 * sizeof(uint64_t));
    if (r.family == KernelFamily::ThreadPerEnv) {
        out[0] = r.tpe.block; out[1] = r.tpe.grid;
        tpe_rollout_kernel_name(name, n_agents, r.tpe, policy == 2);
    } else if (r.family == KernelFamily::Packed) {
        out[0] = uint64_t(r.lq.K); out[1] = uint64_t(r.lq.Q); out[2] = uint64_t(int(r.lq.form)); out[3] = r.lq.block; out[4] = r.lq.lds_bytes;
        out[5] = r.lq.lds_total; out[6] = r.lq.table_lds ? 1u : 0u; out[7] = r.lq.table_at; out[8] = r.lq.limit ? 1u : 0u;
        lq_rollout_kernel_name(name, r.lq, record != 0, policy == 0, policy == 2, soc != 0, may_be_terminal != 0, uint32_t(table_bytes));
    } else {
        out[0] = uint64_t(r.lg.L); out[1] = r.lg.full ? 1u : 0u; out[2] = r.lg.mv_lds ? 1u : 0u; out[3] = r.lg.dense ? 1u : 0u; out[4] = r.lg.block;
        out[5] = r.lg.grid; out[6] = r.lg.lds_bytes; out[7] = r.lg.limit ? 1u : 0u; out[8] = r.lg.budget ? 1u : 0u;
        lg_rollout_kernel_name(name, r.lg, record != 0, policy == 0, policy == 2);
    }
    return int(r.family);
}
// route_step likewise (uniforms: the caller supplies them; scen: rows from the scenario table): thread-per-env: block, grid; packed:
// shim_plan_step's eight; lane-group: shim_plan_step_lg's four, then limit
int shim_route_step(uint32_t n_cells, int n_agents, uint64_t n_envs, int has_delta_rows, int n_cu, const char *tune, int prefer, int limited, int uniforms, int scen,
                    int may_be_terminal, uint64_t out[8], char *name) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    static const uint32_t present = 0;
    StepArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    args.mv4 = has_delta_rows ? &present : nullptr;
    const StepRoute r = route_step(n_agents, args, t, FamilyPreference(prefer), limited != 0, uniforms != 0);
    std::memset(out, 0, 8 * sizeof(uint64_t));
    if (r.family == KernelFamily::ThreadPerEnv) {
        out[0] = r.tpe.block; out[1] = r.tpe.grid;
        tpe_step_kernel_name(name, n_agents, r.tpe, uniforms != 0);
    } else if (r.family == KernelFamily::Packed) {
        out[0] = uint64_t(r.lq.K); out[1] = uint64_t(r.lq.Q); out[2] = uint64_t(int(r.lq.big)); out[3] = r.lq.block; out[4] = r.lq.grid;
        out[5] = r.lq.n_chunks; out[6] = r.lq.lds_bytes; out[7] = uint64_t(r.lq.lds_limit);
        lq_step_kernel_name(name, r.lq, scen != 0, may_be_terminal != 0);
    } else {
        out[0] = uint64_t(r.lg.L); out[1] = r.lg.full ? 1u : 0u; out[2] = r.lg.block; out[3] = r.lg.grid; out[4] = r.lg.limit ? 1u : 0u;
        lg_step_kernel_name(name, r.lg, uniforms != 0);
    }
    return int(r.family);
}

// plan_transitions over a call's five shape facts: out = wide, max_a, all_out, qw_log2, pieces_max, rows_per_wave, unscanned_blocks,
// lanes_log2, walks, chunk, chunks_per_query, scan_passes, scan_blocks, block, grid, lds_bytes; 1 = planned, 0 = the call fits no grid
int shim_plan_transitions(uint32_t n_agents, uint64_t n_queries, uint32_t max_branches, int compact, int all_out, uint64_t out[16]) {
    TransitionsPlan p;
    if (!plan_transitions(n_agents, n_queries, max_branches, compact != 0, all_out != 0, &p)) return 0;
    const uint64_t fields[16] = {p.wide ? 1u : 0u, uint64_t(p.max_a), p.all_out ? 1u : 0u, p.qw_log2, p.pieces_max, p.rows_per_wave, p.unscanned_blocks, p.lanes_log2,
                                 p.walks, p.chunk, p.chunks_per_query, uint64_t(p.scan_passes), p.scan_blocks, p.block, p.grid, p.lds_bytes};
    std::memcpy(out, fields, sizeof(fields));
    return 1;
}
// ... and the name the launcher notes for that plan (kKernelNameBytes)
int shim_transitions_kernel_name(uint32_t n_agents, uint64_t n_queries, uint32_t max_branches, int compact, int all_out, char *name) {
    TransitionsPlan p;
    if (!plan_transitions(n_agents, n_queries, max_branches, compact != 0, all_out != 0, &p)) return 0;
    transitions_kernel_name(name, p, n_agents, compact != 0);
    return 1;
}
// the layout's say on a wave's dynamic LDS in transitions_rows_kernel<max_a>, and the scan's block count
uint64_t shim_transitions_wave_lds_bytes(int max_a, uint32_t qw_log2) { return transitions_wave_lds_bytes(max_a, qw_log2); }
uint64_t shim_transitions_scan_blocks(uint64_t n_queries) { return transitions_scan_blocks(n_queries); }

// does the launcher hold the packed rollout instance (K, Q, form)?  (table: of lq_rollout_kernel_table)
int shim_rollout_instance_exists(int K, int Q, int form, int table) {
    return form >= 0 && form < kTableForms && lq_rollout_instance_exists(K, Q, TableForm(form), table != 0) ? 1 : 0;
}
// how many table instances (MAPF_LQ_ROLLOUT_TABLE_INSTANCES) there are with K agents per lane (0: in all)
int shim_table_instance_count(int K) {
    int n = 0;
#define X(KK, QQ, FF) n += (KK == K || K == 0) ? 1 : 0;
    MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X)
#undef X
    return n;
}

}  // extern "C"
