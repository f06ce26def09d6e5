// Launch planning: which kernel family takes a launch (route_rollout, route_step -- the ONE statement of the routing order), and
// which form, block, grid and LDS image a launch of a given shape takes within its family.  Pure integer arithmetic over the
// launch's shape, the tuning and the LDS layout (mapf_layout.hpp) -- no kernel, no runtime call -- so it can be swept without a
// device (mapf_debug_rollout_plan, tests/test_plan_decisions.py).  The dispatcher (mapf_dispatch.hip) asks the route once per launch
// and hands its plan to the family's launcher; a launcher takes ONE plan and launches the instance it names: it decides neither the
// instance nor the family.  The name a launch notes is formatted here as well, one function per planned family -- thread-per-env,
// the packed rollout, the packed step, the lane-group rollout and step, env.P[s][a] (which no route precedes: its instance follows
// from the agent count) -- so a shape's name can be asked for without a launch.
#pragma once
#include "mapf_layout.hpp"

namespace mapf {

// the defaults of a device with n_cu compute units, overridden by `text` (MAPF_TUNE: "key=value,...", may be null)
RolloutTuning rollout_tuning_for(int n_cu, const char *text, std::string *err);

// The packed rollout's plan, from the launch's shape (args.c.n_cells, n_envs, n_steps, c.top_tie,
// actions / mv4 / mv_delta8 present or not) and the tuning (its n_cu included): false = no packed form applies.  The whole plan:
// the packed family's one launcher (mapf_lq_launch.hpp) is handed nothing else.
struct LqPlan {
    int K = 0, Q = 0;                // agents per lane, lanes per env
    TableForm form = TableForm::FullRows;   // how the move table lies in LDS (mapf_layout.hpp; DESIGN.md 4.1 lists the six forms)
    unsigned block = 0;              // threads per block
    size_t lds_bytes = 0;            // table_image_bytes(form): the kernel's LDS image without the bitmaps, i.e. where the bitmaps begin
    size_t lds_total = 0;            // the dynamic LDS segment of the launch, <= 160 KB: launch_lds_bytes(form, ...), with the bitmaps (and the policy table)
    bool table_lds = false;          // table policy: the action bytes are staged into LDS behind the image (and the bitmaps) ...
    uint32_t table_at = 0;           // ... at this byte, a multiple of 16 (lds_total then includes them)
    bool limit = false;              // the family the plan names: lq_rollout_kernel_table_limit (mapf_lq_limit.hip), the table instances under
                                     // an episode step limit -- the same K, Q, form, block and LDS segment as without it
};
bool plan_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, LqPlan *plan);
// ... under the table policy (args.actions == null): the packed table instances exist for two and four agents per lane over full
// 16-byte rows and for the 32-agent bitmap form over delta rows, in blocks of at most 512 threads.  false = lane-group kernel.
// (limited: the launch runs under an episode step limit and the handle's tuning has limit_packed=1 -- the plan is the unlimited
// one, marked `limit`: no LDS is added and the block is unchanged.  Where it declines, the lane-group limit instance takes the launch)
bool plan_rollout_lq_table(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, size_t table_bytes, LqPlan *plan, bool limited = false);
// TERM of the packed rollout instances: may an env be terminal when a step of the launch begins?  With auto-reset on and no env whose
// START state is itself terminal it cannot -- the ONE statement of that rule: the instance pick and the name read this value
inline bool rollout_may_be_terminal(const RolloutArgs &args) { return !(args.auto_reset && !args.start_terminal_any); }
// The name the launcher notes for a packed plan (mapf_last_kernel; kKernelNameBytes as the lane-group names below), from the plan
// and what the launch says: recording or not; streamed actions, the in-kernel policy or the table policy (then table_bytes action
// bytes); criteria; may-be-terminal.  A limit plan's name says _table_limit, LIMIT and "; episode step limit".
void lq_rollout_kernel_name(char *name, const LqPlan &plan, bool record, bool streamed, bool table_policy, bool soc, bool may_be_terminal, uint32_t table_bytes);

// What launch_step_lq (mapf_lq_step.hip) launches: the instance lq_step_kernel<Q, K, ., ., form> (StepForm and the list of the
// instances: mapf_layout.hpp -- a plan names one of MAPF_LQ_STEP_INSTANCES or there is none) and its geometry.
struct StepPlan {
    int K = 0, Q = 0;                // agents per lane (2, 4; 8 in the large-batch form), lanes per env
    StepForm big = StepForm::Plain;   // the form, under the name of the kernel's template argument (BIG): any of the four, not one BIG form.
                                     // The name is what tests/host_tables_shim.hip reads the field by, this commit's and earlier ones'
    unsigned block = 0, grid = 0;
    unsigned n_chunks = 0;           // the kernel's last argument: chunks of `block` lanes the resident grid walks (plain step: the grid)
    size_t lds_bytes = 0;            // dynamic LDS segment (0 for the plain step: its 1 KB image is static)
    int lds_limit = 0;               // what the launcher raises the instance's dynamic-LDS limit to when lds_bytes > 32 KB
};
bool plan_step_lq(int n_agents, const StepArgs &args, const RolloutTuning &tune, StepPlan *plan);
// The name the launcher notes for a step plan (mapf_last_kernel; kKernelNameBytes as the other names), from the plan and what the
// launch says: start / goal rows from the scenario table or not, and whether an env may be terminal when the step begins.
void lq_step_kernel_name(char *name, const StepPlan &plan, bool scen, bool may_be_terminal);

// The lane-group family (mapf_lg.hpp) takes every launch the packed kernels decline: odd teams, ragged batches, large maps,
// caller-supplied uniforms.  L lanes per env: the power of two >= ceil(A / 2) (two agents per lane).
int lg_group_size(int n_agents);
// Largest block of a rollout kernel: groups of 16 lanes unroll 8 rotation rounds and need more than the 128 registers a
// 1024-thread block leaves per lane.  The kernels' __launch_bounds__ (rollout_max_block, mapf_lg_rollout.hip) read it too.
constexpr unsigned kLgRolloutMaxBlock = 1024u, kLgRolloutMaxBlock16 = 512u;
// static LDS the instances that count conflicting pairs keep beyond kLdsReserve (their ConflictPairs block): a pairs plan stages the
// move table into LDS only where this fits as well
constexpr size_t kPairsLdsBytes = 32;
// ... and the instances that keep an episode log (their EpisodeLog block and four addresses of the limit and the budget), likewise
constexpr size_t kLogLdsBytes = 64;
// ... and the instances that follow a group policy (the policy's two table addresses, mask and probe bound, and seven addresses of the
// totals, the limit and the budget), likewise
constexpr size_t kGroupLdsBytes = 96;
// The instance lg_rollout_kernel<L, full, mv_lds, ., ., dense> (or lg_rollout_kernel_table<L, full, mv_lds, ., dense>) and its geometry;
// under `limit` the instance of the same fields among the limit kernels (mapf_lg_limit.hip), which are never dense
struct LgRolloutPlan {
    int L = 0;                       // lanes per env
    bool full = false;               // A == 2L: no ghost slots
    bool mv_lds = false;             // the whole move table is staged into LDS once per block
    bool dense = false;              // full groups and the env count fills every block: no per-lane predicates
    bool limit = false;              // the family the plan names: the instances under an episode step limit, or those without
    bool budget = false;             // ... or, of a limit plan, the instances under an episode budget (mapf_lg_budget.hip): their launcher sets it
    bool pairs = false;              // ... and, of any of the three, the instances that count conflicting pairs (pairs/mapf_lg_pairs.hip): never dense
    bool joint = false;              // ... and, of any of the six, the instances that follow a joint table policy (csrc_joint/mapf_lg_joint.hip): never dense
    unsigned block = 0, grid = 0;
    size_t lds_bytes = 0;            // dynamic LDS segment: the move table, or 0 (the launcher raises the limit beyond 32 KB)
    bool log = false;                // ... and, of a budget plan, the instances that keep an episode log (csrc_log/mapf_lg_log.hip): never dense
    bool group = false;              // ... and, of any of the eight, the instances that follow a group policy (csrc_group/mapf_lg_group.hip): never dense
};
// (limited: the launch runs under an episode step limit (EpisodeLimit, mapf_kernels.hpp).  Apart from the packed table instances
// behind MAPF_TUNE limit_packed=1 (LqPlan::limit) the limit instances exist in the lane-group family only, so no other packed plan
// and no thread-per-env kernel is consulted and this plan takes the launch: the same plan, marked `limit` and never dense -- the
// limit instances have the guarded form only)
LgRolloutPlan plan_rollout_lg(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, bool limited = false);
struct LgStepPlan { int L = 0; bool full = false; bool limit = false; unsigned block = 0, grid = 0; };
LgStepPlan plan_step_lg(int n_agents, const StepArgs &args, bool limited = false);
// The names the launchers note for these plans (mapf_last_kernel; at most kKernelNameBytes with the terminator).  A limit plan's
// name says _limit_guarded (the step: _limit) and LIMIT, and has no DENSE / GUARDED field; a budget plan's says _budget_guarded and BUDGET.
// A pairs plan's name says _pairs behind the kernel's name and PAIRS behind the form (GUARDED, LIMIT or BUDGET).
// A log plan's name says _log behind _budget_guarded and LOG behind BUDGET.
// A joint plan's name (its launcher passes table_policy) says _joint and JOINT where a table launch says _table and TABLE, and ends with the joint policy's note.
// A group plan's name likewise says _group and GROUP, and ends with the group policy's note.
void lg_rollout_kernel_name(char *name, const LgRolloutPlan &plan, bool record, bool streamed, bool table_policy);
void lg_step_kernel_name(char *name, const LgStepPlan &plan, bool ext_uniforms);

// The thread-per-env family (mapf_kernels.hip): one thread per env, kernels specialised by agent count
struct TpePlan { unsigned block = 0, grid = 0; };
TpePlan plan_tpe(uint64_t n_envs);
void tpe_step_kernel_name(char *name, int n_agents, const TpePlan &plan, bool ext_uniforms);
void tpe_rollout_kernel_name(char *name, int n_agents, const TpePlan &plan, bool table_policy);

// env.P[s][a] (mapf_transitions.hip).  The scan of the windows' lengths works in blocks of kScanBlock queries (the C ABI sizes
// TransitionsArgs::block_base from it); a call of at most kFusedScanBlocks of them leaves the scan's second pass to the rows
// kernel's waves.
constexpr uint32_t kScanBlock = 256, kFusedScanBlocks = 256;
constexpr uint64_t transitions_scan_blocks(uint64_t n_queries) { return (n_queries + kScanBlock - 1) / kScanBlock; }
// What launch_transitions (mapf_dispatch.hip) launches: the scan passes, then transitions_rows_kernel<max_a, all_out> (teams of up
// to eight) or transitions_kernel<max_a, EXACT> (`wide`: 9 to 16 agents), with every argument the kernel takes beside the call's arrays.
struct TransitionsPlan {
    bool wide = false;               // the family
    int max_a = 0;                   // the instance: 2, 4, 6 or 8 agent slots -- wide: the exact agent count, 9..16
    bool all_out = false;            // rows: all five output arrays are given, ALL_OUT (the wide kernels test each pointer)
    uint32_t qw_log2 = 0, pieces_max = 0, rows_per_wave = 0, unscanned_blocks = 0;   // rows: the kernel's arguments
    uint32_t lanes_log2 = 0, walks = 0, chunk = 0, chunks_per_query = 0;             // wide: the kernel's arguments (chunk = walks << lanes_log2)
    int scan_passes = 0;             // 0: no scan; 1: the count pass (transitions_count_kernel); 2: ... and the block-totals pass
    unsigned scan_blocks = 0;        // the count pass's grid (0 without a scan)
    unsigned block = 0, grid = 0;
    size_t lds_bytes = 0;            // rows: waves per block x transitions_wave_lds_bytes (mapf_layout.hpp)
};
// (all_out: as above; false = the launch does not fit a grid: more than 2^31 - 1 blocks or scan blocks, or more than 16 agents)
bool plan_transitions(uint32_t n_agents, uint64_t n_queries, uint32_t max_branches, bool compact, bool all_out, TransitionsPlan *plan);
void transitions_kernel_name(char *name, const TransitionsPlan &plan, uint32_t n_agents, bool compact);

// ------------------------------------------------------------------- the route
// Which family takes a launch, with that family's plan (the other plans stay as constructed).  The rules, each written once, in
// route_rollout / route_step, in this order:
//   a joint table policy takes the lane-group plan of its form (plain, limit or budget; with the conflict matrix or without), marked
//     `joint` and never dense, before anything else: whatever the handle prefers, limit_packed and the tuning say;
//   a group policy likewise takes the lane-group plan of its form (with the episode log where the handle keeps one), marked `group`
//     and never dense, before anything else;
//   a conflict matrix takes the lane-group plan of its form (plain, limit or budget), marked `pairs` and never dense, before
//     anything else: whatever the handle prefers and whatever limit_packed says;
//   a budget takes the lane-group budget plan (a limit plan marked `budget`) before anything else;
//   an episode log comes with a budget only and marks that launch's plan -- the budget's, with the conflict matrix and the joint
//     table policy where the launch has those -- `log`: same geometry, the instances of csrc_log/mapf_lg_log.hip;
//   a limit never goes to thread-per-env, and the step under a limit has the lane-group limit instance only;
//   thread-per-env takes what the handle prefers it for (FamilyPreference; Auto: A <= 2) where its kernels exist: steps up to
//     kTpeMaxAgents, rollouts up to kTpeRolloutMaxAgents;
//   packed comes before lane-group.  Under a limit it applies only to a table-policy launch without streamed actions, with
//     limit_packed=1, on a handle not created with MAPF_FLAG_LANE_GROUP; the packed step declines caller-supplied uniforms;
//   lane-group takes everything else.
enum class KernelFamily { ThreadPerEnv, Packed, LaneGroup };
struct RolloutRoute { KernelFamily family = KernelFamily::LaneGroup; TpePlan tpe; LqPlan lq; LgRolloutPlan lg; };
struct StepRoute { KernelFamily family = KernelFamily::LaneGroup; TpePlan tpe; StepPlan lq; LgStepPlan lg; };
// (table_policy: the launch follows the table policy, of table_bytes action bytes; limited / budgeted: it runs under an episode
// step limit / an episode budget; pairs: the handle counts conflicting pairs; joint: the launch follows the joint table policy;
// logged: the handle keeps an episode log (beside a budget only); group: the launch follows the group policy.  args is never dereferenced)
RolloutRoute route_rollout(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, FamilyPreference prefer, bool table_policy, size_t table_bytes,
                           bool limited, bool budgeted, bool pairs = false, bool joint = false, bool logged = false,
                           bool group = false);
// (ext_uniforms: the caller supplies the uniforms)
StepRoute route_step(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, bool limited, bool ext_uniforms);

}  // namespace mapf
