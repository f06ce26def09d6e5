// Argument blocks and launcher prototypes shared by the kernel files, the dispatcher (mapf_dispatch.hip) and the C ABI
// (mapf_capi.hip).  The tables these blocks point to are built on the host by mapf_tables.hip; which packed form a launch
// takes, and which family takes it, is planned by mapf_plan.hip (mapf_plan.hpp) over the LDS layout of mapf_layout.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "mapf_group_table.hpp"

namespace mapf {

// Merged slip distribution of one agent for one equality pattern of its three candidate cells
// (m = intended move, r = right slip, l = left slip; code = (m==r) | (m==l) << 1 | (r==l) << 2).
// Built on the host by replaying single_agent_movements (mapf_env.py:163-184): drop p <= 0, merge equal
// cells in first-seen order with old + new, then cumsum left to right.
// Move table row of one (cell, action): everything the fast sampling path needs in ONE 16-byte read.
//   x = c0 | c1 << 16, y = c2 | code << 16 | members << 19 : the merged movement list's cells in list order, the
//       equality code of the three candidates (selects the SlipRow with the list's probabilities / full-width
//       thresholds) and SlipRow::members of that code (which candidates merged into each slot);
//   z = t0 | t1 << 16 : top 16 bits of the first two cumulative thresholds, saturated to 65535 (65535 past the end of
//       the list too).  The last threshold of a list is always 65535 (its cumulative sum is 1 up to rounding), so
//       away from ties the sampled slot is the number of passed thresholds among these two; hi16 equal to t0, t1 or
//       65535 is a tie and is resolved by the exact 53-bit path;
//   w = code * sizeof(SlipRow) : byte offset of the code's row (the sampled probability is q[slot] at its start).
using MoveEntry = uint4;
// Columns per cell: the five actions (STAY, UP, RIGHT, DOWN, LEFT).  MAPF_MV_COLS=6 (experiment builds) appends STAY again,
// so that an action byte is extracted and clamped by ONE v_min_u32 with a byte select -- measured on the packed single step
// (profiles/r04_step_table_forms.txt): the 20 % larger table costs more (+0.10 us per launch at 65536 envs: every launch
// re-fetches the table into eight L2s and its gathers are bound by the texture path's line rate) than the two vector
// instructions per agent save, so the shipped table has five columns.
#ifndef MAPF_MV_COLS
#define MAPF_MV_COLS 5
#endif
constexpr uint32_t kMvCols = MAPF_MV_COLS;
static_assert(kMvCols == 5 || kMvCols == 6, "five action columns, optionally STAY again");

struct SlipRow {
    double q[3];                   // merged probabilities, list order
    uint32_t th[3];                // top 16 bits of the thresholds, saturated to 65535 (65535 past the list end too): the
                                   // fast path of slip_move_hi; MoveEntry::z carries th[0], th[1] of the entry's code;
                                   // th[2] = th[0] | th[1] << 16 (that same word, for the COMPACT rollout form)
    uint32_t n;                    // list length, 1..3
    uint64_t thr[3];               // ceil(cum[k] * 2^53): cum[k] > u  <=>  mant(u) < thr[k]; 0 past the list end
    double cum[3];                 // running float64 sums (for caller-supplied uniforms); -inf past the list end
    uint32_t th_biased;            // (th[0] | th[1] << 16) ^ 0x80008000: MoveEntry::z as sample_slot_packed wants it, for
                                   // kernels that gather 8-byte rows and fetch the thresholds from the LDS copy of this row
    uint32_t members;              // bits 3k..3k+2: which candidates (m, r, l) merged into list slot k
};

// 8-byte form of a move-table row, for kernels that are bound by the rate of their table gathers (the packed single step:
// half the table bytes to re-fetch per launch, half the bytes per gathered lane):
//   x = c0 | c1 << 16 (as MoveEntry::x), y = c2 | (code * sizeof(SlipRow)) << 16.
// The thresholds (MoveEntry::z) are SlipRow::th_biased of the code's row, its members (exact path) SlipRow::members.
using CompactEntry = uint2;

// 4-byte DELTA form of a move-table row, for maps on which every candidate cell lies within +-127 ids of its own cell (ids run
// down the columns, so every map of at most 127 rows; mapf_create checks): bytes 0..2 = the three list cells minus the row's
// own cell (signed), byte 3 = (byte offset of the code's slip row + kDeltaRowBias) / 8.  SIX columns per cell (column 5 = STAY
// again: an action byte is extracted and clamped by one v_min_u32), padded with zero words to a multiple of 16 bytes -- the
// image the 32-agent rollout and the LDS-table single step keep in LDS (24 bytes per cell: 79 KB on a 64x64 map, where the
// 16-byte rows take 316 KB), built once on the host.
constexpr uint32_t kDeltaCols = 6, kDeltaRowBias = 16;
__host__ __device__ constexpr size_t delta_table_words(uint32_t n_cells) { return (size_t(n_cells) * kDeltaCols + 3u) & ~size_t(3); }

struct EnvConsts {
    double r_clash, r_goal, r_living;
    double p_cand[3];              // probabilities of the three candidates: intended move, right slip, left slip
    uint32_t need_rng;             // 0 when every slip list has one entry (e.g. fail_prob == 0)
    uint32_t top_tie;              // 1 when some list's last cumulative sum rounds below 1.0 (a uniform can lie past it)
    uint32_t criteria;             // 0 Makespan, 1 SoC
    uint32_t n_cells;              // V
    uint32_t seed_lo, seed_hi;     // slip-stream Philox key
    uint32_t pol_lo, pol_hi;       // policy-stream Philox key (seed + 1)
};

// Outcome of a transition as a function of the group's reduced facts f = vertex | swap << 1 | off_goal_next << 2
// (calc_transition_reward_from_local_states, mapf_env.py:225-235: collision before goal; is_terminal,
// :210-223: a swap alone leaves a non-terminal state): done | collision << 8 | next_terminal << 16 (EnvOut::status).
__host__ __device__ constexpr uint32_t outcome_status(uint32_t f) {
    const bool vertex = (f & 1u) != 0u, coll = (f & 3u) != 0u, goal_next = (f & 4u) == 0u;
    return ((coll || goal_next) ? 1u : 0u) | (coll ? 0x100u : 0u) | ((vertex || goal_next) ? 0x10000u : 0u);
}
constexpr uint32_t kTerminalStatus = 0x10001u;   // a step from a terminal state: done, no collision, still terminal

// LDS outcome table of the rollout kernel (Makespan: the living reward is a constant, so the whole reward is a
// function of f): rows 0..7 = f, rows 8..15 = "the state was terminal" (mapf_env.py:239-240: reward 0, done).
struct OutcomeRow {
    double reward;
    uint32_t status, pad;   // pad: done | collision << 16 (the packed rollout sums it and stores its bytes)
};
static_assert(sizeof(OutcomeRow) == 16, "read as one 16-byte LDS word");
// The 1 KB table image every step / rollout kernel keeps in LDS: the eight slip rows, then the sixteen outcome rows.  The
// handle's device copy (StepArgs::slip, RolloutArgs::slip) holds exactly this image -- the outcome rows built on the host
// with the same float64 additions (build_outcome_rows in mapf_tables.hip) -- so a wave can stage it with one 16-byte load
// and one 16-byte LDS write per lane.
struct TableImage {
    SlipRow slip[8];
    OutcomeRow outcome[16];
};
static_assert(sizeof(TableImage) == 1024, "64 lanes x 16 bytes");

struct StepArgs {
    EnvConsts c;
    const MoveEntry *mv;           // [V*5] move table (see MoveEntry, kMvCols)
    const uint2 *mv8;              // [V*5] the same table with 8-byte rows (CompactEntry: cells + the code's slip-row offset)
    const uint32_t *mv4;           // [delta_table_words(V)] the same table as 4-byte delta rows, six columns; null when the map's ids do not allow them
    const SlipRow *slip;           // [8] device copy of the slip table (the first part of a TableImage)
    uint16_t *state;               // [E*A] persistent env state
    const uint16_t *start, *goal;  // [E*A] or [A]
    const uint8_t *actions;        // [E*A]
    const double *uniforms;        // [E*A] or null
    uint16_t *out_local;
    double *out_reward, *out_prob;
    uint8_t *out_done, *out_collision, *out_was_terminal;
    uint64_t n_envs, env_id_offset, t;
    // Step index of a launch = t + (t_dev ? *t_dev : 0).  Plain launches bake the handle's index into t (t_dev null); a launch
    // recorded into a hipGraph (mapf_graph_begin .. mapf_graph_end) carries its offset inside the recording in t and reads
    // the recording's first index from device memory, which the graph's last node advances -- so a replay draws fresh numbers.
    const uint64_t *t_dev;
    // Scenario table (mapf_create builds it when the batch has at most 256 distinct (start row, goal row) pairs): scen[e]
    // names env e's pair, scen_rows[(2 * scen + 0 | 1) * A ..] are its start / goal cells -- the packed single step reads
    // one byte per env instead of two A-cell rows.  Null when the rows are broadcast or too varied.
    const uint8_t *scen;
    const uint16_t *scen_rows;
    uint32_t *done_flag;           // one-wave launches only (else null): host-visible word that receives done_seq
    uint32_t done_seq;             //   after every output of the step has been written (system-scope release)
    bool start_broadcast, goal_broadcast, auto_reset;
    bool state_not_terminal;       // host promise: no env is terminal when this step begins (see mapf_handle_s::may_be_terminal)
};

struct RolloutArgs {
    EnvConsts c;
    const MoveEntry *mv;
    const uint32_t *mv4;           // see StepArgs (non-null <=> mv_delta8)
    const SlipRow *slip;
    uint16_t *state;
    const uint16_t *start, *goal;
    const uint8_t *actions;        // [T*E*A] or null (on-device policy)
    const uint2 *policy_cells;     // greedy policy: [V] {row | col << 16, nine 3-bit actions}; null = random policy stream
    double *out_returns;
    uint32_t *out_episodes, *out_collisions;
    uint16_t *rec_local;
    double *rec_reward, *rec_prob;
    uint8_t *rec_done, *rec_collision;
    uint64_t n_envs, env_id_offset, t;
    const uint64_t *t_dev;         // see StepArgs: first step index = t + (t_dev ? *t_dev : 0)
    uint32_t n_steps;
    bool start_broadcast, goal_broadcast, auto_reset, accumulate;
    bool start_terminal_any;       // some env's START state is terminal (two starts coincide / every start is its goal)
    bool mv_delta8;                // every candidate cell of the move table lies within +-127 ids of its own cell (mapf_create looks)
};

// Table policy (include/mapf_hip.h MAPF_POLICY_TABLE): the device copies mapf_set_policy_table made.  Handed to the
// table instances of the rollout kernels as an argument of their own -- RolloutArgs, and with it every kernel that exists
// without the table policy, stays as it is.
struct TablePolicy {
    const uint8_t *table;          // [n_rows * V] action bytes 0..4 (the allocation is padded to a multiple of 16 bytes)
    const uint16_t *rows;          // [E*A] or [A]: the row an agent follows
    uint32_t table_bytes;          // n_rows * V (< 2^31)
    uint32_t rows_broadcast;       // rows is [A]
};

// Joint table policy (include/mapf_hip.h MAPF_POLICY_JOINT): the device copies mapf_set_policy_joint made.  A solo agent i of env e
// (partner[e,i] == i) on cell c takes table[offset[e,i] + c]; an agent merged with j = partner[e,i], which stands on c_j, takes
// table[offset[e,i] + c * V + c_j].  One more block beside the others: the joint instances (csrc_joint/mapf_lg_joint.hip) take it
// first, where the table instances take TablePolicy -- never both.
struct JointPolicy {
    const uint8_t *table;          // [table_bytes] action bytes 0..4 (the allocation is padded to a multiple of 16 bytes)
    const uint32_t *offset;        // [E*A] or [A]: where the agent's segment begins (V bytes solo, V*V bytes merged)
    const uint16_t *partner;       // [E*A] or [A]: the agent it is merged with, or itself
    uint32_t table_bytes;          // < 2^31
    uint32_t broadcast;            // offset and partner are [A]
};

// Group policy (include/mapf_hip.h MAPF_POLICY_GROUP): the device copies mapf_set_policy_group made.  Every agent has a solo row, as
// under TablePolicy; an agent of a group of 2..4 takes its byte of the entry of the group's current joint cell where the group's
// book has one (the open-addressing table of mapf_group_table.hpp), else the byte of its row.  One more block beside the others: the
// group instances (csrc_group/mapf_lg_group.hip) take it first, where the table instances take TablePolicy -- never beside it or
// JointPolicy.
struct GroupPolicy {
    const uint8_t *table;          // [n_rows * V] the solo rows' action bytes 0..4 (the allocation is padded to a multiple of 16 bytes)
    const uint16_t *rows;          // [E*A] or [A]: the row an agent follows where its group's book has no entry
    const uint16_t *members;       // [E*A*4] or [A*4]: the agents of the agent's group, ascending, 0xFFFF behind the last
    const uint32_t *book;          // [E*A] or [A]: the group's book (ignored for a solo agent)
    const GroupSlot *slots;        // [mask + 1] all books' entries
    uint32_t mask;                 // capacity - 1, the capacity a power of two
    uint32_t max_probe;            // the longest probe chain the builder produced: the bound of the kernel's probe loop
    uint32_t broadcast;            // rows, members and book are per agent, shared by all envs
};

// Episode step limit (include/mapf_hip.h mapf_set_episode_limit): the handle's per-env ages, the limit and where a launch
// reports its truncations.  Travels beside the argument blocks as the table policy does -- StepArgs, RolloutArgs, and with them
// every kernel that exists without the limit, stay as they are; the limit instances are kernels of their own (mapf_lg_limit.hip).
struct EpisodeLimit {
    uint32_t *age;                 // [E] live steps since the episode began, saturating
    uint32_t max_steps;            // N >= 1
    uint32_t *out_truncations;     // rollout: [E] or null (RolloutArgs::accumulate applies)
    uint8_t *rec_truncated;        // rollout: [T*E], non-null exactly when the launch records; single step: [E] or null
};

// Episode budget (include/mapf_hip.h mapf_set_episode_budget): the handle's per-env counts of episodes left and where a launch
// reports its live steps.  A block of its own beside EpisodeLimit, which stays as it is; the budget instances (mapf_lg_budget.hip)
// take both -- the limit block with max_steps == 0 on a handle without a limit: the ages are then left alone and nothing truncates.
struct EpisodeBudget {
    uint32_t *left;                // [E] episodes the env may still end (done or truncated); 0 = parked
    uint32_t *out_live_steps;      // [E] or null (RolloutArgs::accumulate applies): steps neither parked nor terminal on entry
};

// Conflict matrix (include/mapf_hip.h mapf_set_conflict_pairs): the handle's per-slot counts of vertex conflicts (upper triangle) and
// swaps (lower triangle) per agent pair, and the slot of every env.  One more block beside the others: the instances that count
// (pairs/mapf_lg_pairs.hip) take it last, behind the table policy, the limit and the budget where the launch has those.
struct ConflictPairs {
    unsigned long long *matrix;    // [n_slots * A * A] counts, row-major per slot; the diagonal is never written
    const uint32_t *slot;          // [E] the env's slot, < n_slots; null = every env in slot 0
    uint32_t n_slots;              // >= 1, n_slots * A * A * 8 <= 2^30 bytes (so an entry's index fits 32 bits)
};

// Episode log (include/mapf_hip.h mapf_set_episode_log): the handle's per-env partial episode -- the running return and its live
// steps -- its count of ended episodes and the records of the first `capacity` of them.  One more block beside the others: the
// log instances (../csrc_log/mapf_lg_log.hip) take it behind the budget and before the conflict matrix.  Two pointers, so that the
// step loop carries two addresses per lane: the counts lie behind the partials in ONE allocation.
struct EpisodeLogPartial { double acc; uint32_t len, pad; };   // the running return (+0.0 when an episode begins) and its live steps
static_assert(sizeof(EpisodeLogPartial) == 16, "read and written as one 16-byte word");
struct EpisodeLog {
    EpisodeLogPartial *partial;    // [E] partials, then u32 count[E] at byte E * 16: episodes ended since the last clear, saturating
    uint4 *records;                // [E * capacity] mapf_episode_record {f64 ret, u32 steps, u32 outcome}: env e's k-th ended episode at e * capacity + k
    uint32_t capacity;             // C >= 1, E * C * 16 <= 2^31 bytes (so a record's byte offset fits 32 bits)
};
// where the counts of a log of n_envs envs begin
__host__ __device__ inline uint32_t *episode_log_counts(EpisodeLogPartial *partial, uint64_t n_envs) { return reinterpret_cast<uint32_t *>(partial + n_envs); }

// Every launcher names the kernel instance (and block size) that took the launch; the C ABI keeps the name of a
// handle's last step / rollout launch (mapf_last_kernel) so a benchmark labels its numbers with what actually ran.
constexpr size_t kKernelNameBytes = 160;   // what is kept of a name, the terminator included
void note_kernel(const char *name);

struct TransitionsArgs {
    EnvConsts c;
    const MoveEntry *mv;
    const SlipRow *slip;
    const uint16_t *goal;          // [E*A] or [A]
    const uint16_t *local;         // [N*A] query states
    const uint8_t *actions;        // [N*A] query joint actions
    const uint32_t *env_index;     // [N] env whose goals apply, or null (env 0)
    uint32_t *out_count;           // [N] number of branches (product of list lengths; 1 for a terminal state)
    uint16_t *out_next;            // [N*M*A]
    double *out_prob, *out_reward; // [N*M]
    uint8_t *out_done, *out_collision;
    uint64_t n_queries;
    uint64_t first_branch;         // first branch of the returned window (0 = from the start)
    uint32_t max_branches, n_agents;
    bool goal_broadcast;
    // The scan of the windows' lengths (launch_transitions makes it when the output is compacted or a query's window is cut
    // into several waves' pieces): query q's window starts at row block_base[q / 256] + rel[q] of the COMPACTED arrays,
    // block_base[number of blocks] = the rows in total.  compact: the output arrays ARE compacted (mapf_transitions_compact;
    // out_offset[q] receives q's first row, out_offset[N] the total) -- else reserved rows (row j of query q's window at
    // q * max_branches + j).  Rows at or beyond `capacity` are not written.
    uint32_t *rel;                 // scratch u32[N]
    uint64_t *block_base;          // scratch u64[transitions_scan_blocks(N) + 1] (mapf_plan.hpp)
    uint64_t *out_offset;
    uint64_t capacity;
    bool compact;
};
constexpr int kTransitionsMaxAgents = 16;   // 3^16 = 43 M branches per query, returned in windows
// The dispatcher's entry (mapf_dispatch.hip): hipSuccess for an empty call before anything is noted; else plan_transitions
// (mapf_plan.hpp) once, hipErrorInvalidValue where it declines, then the launchers of mapf_transitions.hip, which take that plan and
// decide nothing: the scan passes it names, then its family's instance under its name
hipError_t launch_transitions(const TransitionsArgs &args, hipStream_t stream);
struct TransitionsPlan;
hipError_t launch_transitions_scan(const TransitionsPlan &plan, const TransitionsArgs &args, hipStream_t stream);
hipError_t launch_transitions_rows(const TransitionsPlan &plan, const TransitionsArgs &args, hipStream_t stream);
hipError_t launch_transitions_wide(const TransitionsPlan &plan, const TransitionsArgs &args, hipStream_t stream);
// calc_transition_reward_from_local_states for N (prev = args.local, args.actions, next) triples; fills
// args.out_reward / out_done / out_collision [N] (max_branches, out_count, out_next, out_prob unused)
hipError_t launch_transition_rewards(const TransitionsArgs &args, const uint16_t *next, hipStream_t stream);

hipError_t launch_reset(int n_agents, uint16_t *state, const uint16_t *start, bool start_broadcast,
                        const uint8_t *mask, uint64_t n_envs, hipStream_t stream);
hipError_t launch_fill_actions(int n_agents, uint8_t *actions, const EnvConsts &c, uint64_t env_id_offset,
                               uint64_t n_envs, uint64_t t0, uint64_t n_steps, hipStream_t stream);

// *t_dev += n from one thread: the last node of a recorded graph (mapf_graph_end)
hipError_t launch_advance_step_index(uint64_t *t_dev, uint64_t n, hipStream_t stream);
// *t_dev = value (mapf_graph_launch, when the host side moved the step index since the last replay)
hipError_t launch_set_step_index(uint64_t *t_dev, uint64_t value, hipStream_t stream);

hipError_t launch_query_terminal(int n_agents, const uint16_t *state, const uint16_t *goal, bool goal_broadcast,
                                 uint8_t *out, uint64_t n_envs, hipStream_t stream);

constexpr int kTpeMaxAgents = 16;         // thread-per-env step kernels are specialised for A = 1..16
#ifndef MAPF_TPE_ROLLOUT_MAX              // (tools/exp/tpe_spill_repro.sh builds a library that dispatches the spilling ones)
#define MAPF_TPE_ROLLOUT_MAX 6
#endif
constexpr int kTpeRolloutMaxAgents = MAPF_TPE_ROLLOUT_MAX;   // ... their rollout form is dispatched only where it is spill-free
// Layout choices of the kernels, fixed per handle at mapf_create (the MAPF_TUNE override -- "key=value,..." -- is read
// there, so a process can hold handles with different settings: the tests do).  The key of each field is named beside it.
struct RolloutTuning {
    int n_cu = 256;                  // compute units of the handle's device (asked once, at mapf_create; 256 when the query fails)
    bool quad_lanes = true;          // quad_lanes=0 forces the pair layout
    uint64_t quad_min_lanes = 0;     // four agents per lane need at least this many lanes (quad_min_lanes; default: one
                                     // wave on every SIMD of the device); below that two agents per lane
    uint64_t oct_min_lanes = 0;      // eight agents per lane need at least this many lanes (oct_min_lanes; default:
                                     //   two waves on every SIMD)
    int force_k = 0;                 // k=2|4|8 pins the agents per lane of the packed layout (tests)
    size_t mv_lds_max_bytes = 0;     // largest move table staged into LDS (mv_lds_max_bytes; default: two blocks per CU)
    bool bitmap_pairs = true;        // bitmap_pairs=0: the 32-agent rollout keeps the all-pairs collision tests (tests compare both)
    bool bitmap_delta_rows = true;   // bitmap_delta=0: the bitmap form never uses the 4-byte delta rows (tests compare the tables)
    bool bitmap_stay_column = true;  // bitmap_staycol=0: the bitmap form always stages the four-column table (tests)
    unsigned bitmap_block = 0;       // bitmap_block=512|1024: block size of the bitmap form (experiments / tests; 0 = by batch)
    int step_big = 1;                // step_big: the packed single step's resident-grid / LDS-table form -- 0 never, 1 for batches
                                     //   of at least four times what the device holds at once (default), 2 whenever it fits (tests)
    unsigned step_block = 0;         // step_block=64|128|256|512: block size of the plain packed single step (experiments; 0 = by batch)
    int step_delta = 1;              // step_delta: the single step's LDS table of 4-byte delta rows -- 0 never, 1 where the 16-byte rows
                                     //   do not fit and the batch gives every CU a block (default), 2 whenever it fits (tests, experiments)
    unsigned step_grid = 0;          // step_grid=n: at most n blocks in the grid of the single step's resident forms, so that a block walks many
                                     //   chunks of a small batch (tests; 0 = by the device's CU count; the plain step ignores it)
    bool scen_table = true;          // scen_table=0: never build the scenario table (StepArgs::scen) -- tests compare both forms
    int policy_table_lds = -1;       // policy_table_lds=0|1: the packed rollout under the table policy gathers its action bytes from global
                                     //   memory / from a copy staged into LDS behind the table image whenever that fits (default: by shape)
    bool limit_packed = false;       // limit_packed=1: a table-policy rollout under an episode step limit takes the packed limit instance
                                     //   (mapf_lq_limit.hip) where the packed table plan applies; default 0: always the lane-group limit instance
                                     //   (never on a handle created with MAPF_FLAG_LANE_GROUP; read by route_rollout alone, mapf_plan.hpp)
};
RolloutTuning default_rollout_tuning(int device, std::string *err);   // (asks the device, reads MAPF_TUNE: mapf_dispatch.hip)
// The kernel family a handle prefers, from its create flags: MAPF_FLAG_THREAD_PER_ENV, MAPF_FLAG_LANE_GROUP, or neither (Auto).
// What a launch then takes is route_rollout's / route_step's say (mapf_plan.hpp).
enum class FamilyPreference { Auto, ThreadPerEnv, LaneGroup };

// The dispatcher (mapf_dispatch.hip): the only launch entries the C ABI calls.  Each returns hipSuccess for an empty batch before
// anything is noted; else it asks the route (mapf_plan.hpp) once, checks the limit / budget block once (hipErrorInvalidValue when
// it is incomplete) and hands the plan to the family's launcher below.
// (table: the table policy of an actions == null launch, or null: streamed actions take precedence over it as over the other
// policies, and the C ABI, which applies that rule, never passes both.  A recording launch names all five rec_* arrays: the C ABI
// substitutes scratch for absent ones.  limit / budget: those of a handle that has them, or null; with a budget `limit` is
// non-null too, max_steps 0 on a handle without a limit.  pairs: the conflict matrix of a handle that counts, or null.
// joint: the joint table policy of an actions == null launch, or null -- never beside `table`.  log: the episode log of a handle
// that keeps one, or null; only beside a budget.  group: the group policy of an actions == null launch, or null -- never beside
// `table` or `joint`)
hipError_t launch_step(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, hipStream_t stream, const EpisodeLimit *limit = nullptr);
hipError_t launch_rollout(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, FamilyPreference prefer, hipStream_t stream,
                          const TablePolicy *table = nullptr, const EpisodeLimit *limit = nullptr, const EpisodeBudget *budget = nullptr,
                          const ConflictPairs *pairs = nullptr, const JointPolicy *joint = nullptr, const EpisodeLog *log = nullptr,
                          const GroupPolicy *group = nullptr);
// is the step launch_step would launch a thread-per-env one (one thread per env), else lg_group_size(A) threads per env?
bool step_is_thread_per_env(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, const EpisodeLimit *limit);

// The family launchers: each takes the plan the route made (mapf_plan.hpp), launches the instance it names under the plan's name
// and decides nothing -- it calls no planner and no other family's launcher.  A family without an instance for what it is handed
// returns hipErrorInvalidValue: a missing kernel is an error, never another policy.
struct TpePlan; struct LqPlan; struct StepPlan; struct LgRolloutPlan; struct LgStepPlan;
// lane-group (any A up to 128, run-time A): mapf_lg_rollout.hip, mapf_lg_kernels.hip; its limit instances and the masked zeroing
// of the ages: mapf_lg_limit.hip; its budget instances: mapf_lg_budget.hip
hipError_t launch_rollout_lg(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table);
hipError_t launch_rollout_lg_limit(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, const EpisodeLimit &limit);
hipError_t launch_rollout_lg_budget(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                    const EpisodeLimit &limit, const EpisodeBudget &budget);
// ... and the instances of the three that count conflicting pairs: pairs/mapf_lg_pairs.hip, compiled once per form (plain, limit, budget)
hipError_t launch_rollout_lg_pairs(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, const ConflictPairs &pairs);
hipError_t launch_rollout_lg_pairs_limit(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, const EpisodeLimit &limit,
                                         const ConflictPairs &pairs);
hipError_t launch_rollout_lg_pairs_budget(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table,
                                          const EpisodeLimit &limit, const EpisodeBudget &budget, const ConflictPairs &pairs);
// ... and the instances that follow a joint table policy: csrc_joint/mapf_lg_joint.hip, compiled once per form (plain, limit, budget;
// each with and without the conflict matrix).  ONE signature: a form is handed the blocks it takes and refuses a launch that
// lacks one of them or brings another
#define MAPF_LG_JOINT_LAUNCHERS(X) X(plain) X(limit) X(budget) X(pairs_plain) X(pairs_limit) X(pairs_budget)
#define X(form)                                                                                                                              \
    hipError_t launch_rollout_lg_joint_##form(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const JointPolicy &joint, \
                                              const EpisodeLimit *limit, const EpisodeBudget *budget, const ConflictPairs *pairs);
MAPF_LG_JOINT_LAUNCHERS(X)
#undef X
// ... and the budget instances that keep an episode log: ../csrc_log/mapf_lg_log.hip, compiled once per (policy arm, conflict matrix):
// streamed actions / in-kernel policy / table policy, or the joint table policy; each without and with the matrix.  ONE signature,
// as the joint launchers have: a unit refuses a launch that lacks one of its blocks or brings another.  The masked zeroing of the
// partials (mapf_reset) lives in the first of them
#define MAPF_LG_LOG_LAUNCHERS(X) X(budget) X(pairs_budget) X(joint_budget) X(joint_pairs_budget)
#define X(form)                                                                                                                                \
    hipError_t launch_rollout_lg_log_##form(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table, \
                                            const JointPolicy *joint, const EpisodeLimit *limit, const EpisodeBudget *budget, const EpisodeLog *log,       \
                                            const ConflictPairs *pairs);
MAPF_LG_LOG_LAUNCHERS(X)
#undef X
// ... and the instances that follow a group policy: ../csrc_group/mapf_lg_group.hip, compiled once per form (plain, limit, budget, each
// without and with the conflict matrix; the budget form with the episode log, likewise).  ONE signature again
#define MAPF_LG_GROUP_LAUNCHERS(X) X(plain) X(limit) X(budget) X(pairs_plain) X(pairs_limit) X(pairs_budget) X(log_budget) X(log_pairs_budget)
#define X(form)                                                                                                                              \
    hipError_t launch_rollout_lg_group_##form(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const GroupPolicy &group, \
                                              const EpisodeLimit *limit, const EpisodeBudget *budget, const EpisodeLog *log, const ConflictPairs *pairs);
MAPF_LG_GROUP_LAUNCHERS(X)
#undef X
hipError_t launch_reset_log_partials(EpisodeLogPartial *partial, const uint8_t *mask, uint64_t n_envs, hipStream_t stream);
hipError_t launch_step_lg(const LgStepPlan &plan, int n_agents, const StepArgs &args, hipStream_t stream);
hipError_t launch_step_lg_limit(const LgStepPlan &plan, int n_agents, const StepArgs &args, hipStream_t stream, const EpisodeLimit &limit);
hipError_t launch_reset_ages(uint32_t *age, const uint8_t *mask, uint64_t n_envs, hipStream_t stream);
// packed single step (mapf_lq_step.hip): one of MAPF_LQ_STEP_INSTANCES (mapf_layout.hpp)
hipError_t launch_step_lq(const StepPlan &plan, int n_agents, const StepArgs &args, hipStream_t stream);
// packed rollout (2, 4 or 8 agents per lane): mapf_lq_rollout.hip compiled once per (agents per lane, recording) pair, mapf_lq_limit.hip
// (the table policy's instances under an episode step limit) once per (four or two agents per lane, recording) pair; the dispatcher
// keeps the table of these objects.  ONE signature (table: the table policy, or null; limit: the episode limit, or null): an
// object without limit instances refuses a limit, the limit objects refuse a launch without a table or without a limit
#define MAPF_LQ_LAUNCHERS(X) X(rollout_lq_k8_r1) X(rollout_lq_k8_r0) X(rollout_lq_k4_r1) X(rollout_lq_k4_r0) X(rollout_lq_k2_r1) X(rollout_lq_k2_r0) \
    X(rollout_lq_limit_k4_r1) X(rollout_lq_limit_k4_r0) X(rollout_lq_limit_k2_r1) X(rollout_lq_limit_k2_r0)
#define X(name) \
    hipError_t launch_##name(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table, const EpisodeLimit *limit);
MAPF_LQ_LAUNCHERS(X)
#undef X
// thread-per-env (mapf_kernels.hip): group g holds the kernels specialised for A in 4g+1 .. 4g+4
#define X(g)                                                                                                        \
    hipError_t launch_step_g##g(const TpePlan &plan, int n_agents, const StepArgs &args, hipStream_t stream);      \
    hipError_t launch_rollout_g##g(const TpePlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table);
X(0) X(1) X(2) X(3)
#undef X

}  // namespace mapf
