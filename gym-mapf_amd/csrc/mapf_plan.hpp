// Launch planning of the packed kernels: which form, block, grid and LDS image a launch of a given shape takes.  Pure
// integer arithmetic over the launch's shape, the tuning and the LDS layout (mapf_layout.hpp) -- no kernel, no runtime
// call -- so it can be swept without a device (mapf_debug_rollout_plan, tests/test_cabi_and_host.py).
#pragma once
#include "mapf_layout.hpp"

namespace mapf {

// the defaults of a device with n_cu compute units, overridden by `text` (MAPF_TUNE: "key=value,...", may be null)
RolloutTuning rollout_tuning_for(int n_cu, const char *text, std::string *err);

// What try_launch_rollout_lq decides before it launches, from the launch's shape (args.c.n_cells, n_envs, n_steps, c.top_tie,
// actions / mv4 / mv_delta8 present or not) and the tuning (its n_cu included): false = no packed form applies.
struct LqPlan {
    int K = 0, Q = 0;                // agents per lane, lanes per env
    TableForm form = TableForm::FullRows;   // how the move table lies in LDS (mapf_layout.hpp; DESIGN.md 4.1 lists the six forms)
    unsigned block = 0;              // threads per block
    size_t lds_bytes = 0;            // table_image_bytes(form): the kernel's LDS image without the bitmaps (what the launcher is handed)
    size_t lds_total = 0;            // launch_lds_bytes(form, ...): with them -- the dynamic LDS segment of the launch, <= 160 KB
};
bool plan_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, LqPlan *plan);
// ... under the table policy (args.actions == null): the packed table instances exist for two and four agents per lane over full
// 16-byte rows and for the 32-agent bitmap form over delta rows, in blocks of at most 512 threads; *table_lds = the action bytes are
// staged into LDS behind the image (and the bitmaps) at byte *table_at, plan->lds_total then includes them.  false = lane-group kernel.
bool plan_rollout_lq_table(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, size_t table_bytes, LqPlan *plan,
                           bool *table_lds, uint32_t *table_at);

// The forms of the packed single step: the plain step, or a resident grid with the move table in LDS (the values: the kernel's BIG)
enum class StepForm : int { Plain = 0, FullRows = 1, DeltaRows = 2, DeltaRowsBitmap = 3 };   // (16-byte rows; 4-byte delta rows; ... + per-env occupancy bitmaps)
// What try_launch_step_lq (mapf_lq_step.hip) launches: the instance lq_step_kernel<Q, K, ., ., form> and its geometry.
struct StepPlan {
    int K = 0, Q = 0;                // agents per lane (2, 4; 8 in the large-batch form), lanes per env
    StepForm big = StepForm::Plain;   // the form (the name of the kernel's template argument)
    unsigned block = 0, grid = 0;
    unsigned n_chunks = 0;           // the kernel's last argument: chunks of `block` lanes the resident grid walks (plain step: the grid)
    size_t lds_bytes = 0;            // dynamic LDS segment (0 for the plain step: its 1 KB image is static)
    int lds_limit = 0;               // what the launcher raises the instance's dynamic-LDS limit to when lds_bytes > 32 KB
};
bool plan_step_lq(int n_agents, const StepArgs &args, const RolloutTuning &tune, StepPlan *plan);

}  // namespace mapf
