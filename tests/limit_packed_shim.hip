// Test shim (tests/test_limit_packed_host.py): a C face on plan_rollout_lq_table's limited form (mapf_plan.hip) and on the list of
// packed table instances (mapf_layout.hpp), driven through ctypes without a device.  Test code, compiled into the test's tmp
// dir; not part of libmapf_hip.so.
#include "mapf_plan.hpp"

using namespace mapf;

extern "C" {

// plan_rollout_lq_table over a shape (a launch without streamed actions, under a policy table of table_bytes; limited: under an
// episode step limit with limit_packed=1): out = K, Q, form, block, lds_bytes, lds_total, table_lds, table_at, limit;
// 1 = a packed table instance, 0 = none, -1 = bad tune; *limit_packed = what the tune string says of the key
int lp_plan_rollout_table(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int has_delta_rows, uint64_t table_bytes, int n_cu,
                          const char *tune, int limited, uint64_t out[9], int *limit_packed) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    if (limit_packed) *limit_packed = t.limit_packed ? 1 : 0;
    static const uint32_t present = 0;
    RolloutArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    args.n_steps = n_steps;
    args.mv_delta8 = has_delta_rows != 0;
    args.mv4 = has_delta_rows ? &present : nullptr;
    LqPlan plan;
    if (!plan_rollout_lq_table(n_agents, args, t, size_t(table_bytes), &plan, limited != 0)) return 0;
    out[0] = uint64_t(plan.K); out[1] = uint64_t(plan.Q); out[2] = uint64_t(int(plan.form)); out[3] = plan.block; out[4] = plan.lds_bytes;
    out[5] = plan.lds_total; out[6] = plan.table_lds ? 1u : 0u; out[7] = plan.table_at; out[8] = plan.limit ? 1u : 0u;
    return 1;
}

// is (K, Q, form) one of MAPF_LQ_ROLLOUT_TABLE_INSTANCES?  ... and how many there are
int lp_table_instance_exists(int K, int Q, int form) { return form >= 0 && form < kTableForms && lq_rollout_instance_exists(K, Q, TableForm(form), true) ? 1 : 0; }
int lp_table_instance_count(int K) {
    int n = 0;
#define X(KK, QQ, FF) n += (KK == K || K == 0) ? 1 : 0;
    MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X)
#undef X
    return n;
}

}  // extern "C"
