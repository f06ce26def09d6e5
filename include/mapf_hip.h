/*
 * mapf_hip.h -- C ABI of libmapf_hip.so: the MI355X (gfx950) implementation of
 * gym-mapf's batched MapfEnv.step() hot path.
 *
 * The reference has no FFI; its hot path sits behind a Python class
 * (gym_mapf/envs/mapf_env.py:115 `class MapfEnv`).  Each entry point below
 * names the reference method/lines it replaces.  The reference-side binding
 * (ctypes) a maintainer would add is shown in INTEGRATION.md and implemented in
 * gym-mapf_amd/gym_mapf_amd/_native.py.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative
 *     MAPF_E* code, and mapf_last_error() (thread-local) holds the message;
 *   - the handle owns its device buffers and (unless one is supplied) its HIP
 *     stream; the caller owns every array it passes in;
 *   - array arguments are HOST pointers unless the handle was created with
 *     MAPF_FLAG_DEVICE_PTRS, in which case they are DEVICE pointers (e.g.
 *     torch tensors' data_ptr()) and calls only enqueue work -- use
 *     mapf_sync() before reading results;
 *   - one handle is driven by one host thread at a time;
 *   - layouts are env-major: x[e*A + i] is agent i of env e.  Cells are
 *     "local ids": the index of a free cell in the reference's column-major
 *     enumeration (mapf_env.py:142 valid_locations, grid.py:37-40), uint16
 *     (every reference map has <= 65536 free cells);
 *   - actions: 0 STAY, 1 UP, 2 RIGHT, 3 DOWN, 4 LEFT
 *     (gym_mapf/envs/__init__.py:26 ACTIONS); values > 4 are treated as STAY.
 */
#ifndef MAPF_HIP_H
#define MAPF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAPF_ABI_VERSION 6

/* status codes */
#define MAPF_OK            0
#define MAPF_EINVAL       -1  /* bad argument / descriptor                   */
#define MAPF_EHIP         -2  /* HIP runtime error (message has the detail)  */
#define MAPF_ENODEVICE    -3  /* no usable HIP device                        */
#define MAPF_EUNSUPPORTED -4  /* e.g. n_agents beyond MAPF_MAX_AGENTS        */

#define MAPF_MAX_AGENTS 128

/* optimisation criteria: mapf_env.py:31-33 OptimizationCriteria */
#define MAPF_MAKESPAN 0
#define MAPF_SOC      1

/* mapf_desc.flags */
#define MAPF_FLAG_DEVICE_PTRS     0x1u  /* array args of step/rollout/... are device pointers */
#define MAPF_FLAG_START_BROADCAST 0x2u  /* desc.start is [A], shared by all envs              */
#define MAPF_FLAG_GOAL_BROADCAST  0x4u  /* desc.goal  is [A], shared by all envs              */
/* Kernel family (default: chosen from A and E).  Both compute identical results.
 *   THREAD_PER_ENV: one lane owns all A agents of an env (A <= 16 only);
 *   LANE_GROUP:     an env is spread over pow2(ceil(A/2)) adjacent lanes, two agents per lane. */
#define MAPF_FLAG_THREAD_PER_ENV  0x10u
#define MAPF_FLAG_LANE_GROUP      0x20u

/* step_flags / rollout flags */
#define MAPF_STEP_AUTO_RESET      0x1u  /* after a step returns done, the env's stored state
                                           goes back to its start cells (mapf_env.py:290-293
                                           reset(), no reseed) -- the outputs still report the
                                           state step() returned                              */

typedef struct mapf_handle_s *mapf_handle_t;

/*
 * Everything MapfEnv.__init__ (mapf_env.py:116-161) derives from its
 * arguments, precomputed by the host wrapper and uploaded once.
 * desc.nbr / start / goal are always HOST pointers.
 */
typedef struct mapf_desc {
    uint32_t struct_size;    /* = sizeof(mapf_desc)                                        */
    uint32_t n_cells;        /* V = len(valid_locations), 1..65536                         */
    uint32_t n_agents;       /* A, 1..MAPF_MAX_AGENTS                                      */
    uint32_t criteria;       /* MAPF_MAKESPAN | MAPF_SOC                                   */
    uint64_t n_envs;         /* E: envs owned by this handle (this rank's shard)           */
    uint64_t env_id_offset;  /* global id of local env 0 (RNG counters use global ids)     */
    uint64_t seed;           /* Philox key (slip stream); policy stream uses seed + 1      */
    const uint16_t *nbr;     /* [V*5]: nbr[v*5+a] = cell reached from v by noise-free a    */
                             /*        (mapf_env.py:43-94 execute_action, folded to a table) */
    const uint16_t *start;   /* [E*A] or [A]: start cells (mapf_env.py:128 agents_starts)   */
    const uint16_t *goal;    /* [E*A] or [A]: goal cells                                    */
    double fail_prob;        /* mapf_env.py:130; right_fail = left_fail = fail_prob / 2     */
    double r_clash;          /* reward_of_collision                                         */
    double r_goal;           /* reward_of_goal                                              */
    double r_living;         /* reward_of_living                                            */
    int32_t device;          /* HIP device ordinal                                          */
    uint32_t flags;          /* MAPF_FLAG_*                                                 */
    void *stream;            /* hipStream_t to enqueue on, or NULL: the handle creates one  */
} mapf_desc;

/*
 * Kernel-dispatch overrides (tests, A/B measurements; none is needed for correct or fast operation): ONE environment
 * variable, MAPF_TUNE="key=value,key=value,...", read by mapf_create -- so a process can hold handles created under
 * different settings; an unknown key or a malformed item fails mapf_create with MAPF_EINVAL.  Keys (integers):
 *   quad_lanes=0         never the packed rollout / step layouts: the lane-group kernels take every launch
 *   k=2|4|8              pin the packed layout's agents per lane (default: by batch -- 8 from two waves per SIMD of that form
 *                        on, 4 from one, else 2; 32 agents on 64x64 maps: 4 with occupancy bitmaps)
 *   quad_min_lanes=n, oct_min_lanes=n   lane counts from which four / eight agents per lane are used
 *   mv_lds_max_bytes=n   largest full move table the rollout kernels stage into LDS (default: half of the 160 KB); above it
 *                        8-byte / 4-byte rows, 0 = always gather from global memory
 *   scen_table=0         never build the scenario table (<= 256 distinct (start row, goal row) pairs: one byte per env)
 *   bitmap_pairs=0       32 agents: all agent pairs instead of the per-env LDS occupancy bitmaps
 *   bitmap_block=512|1024, bitmap_staycol=0, bitmap_delta=0   forms of the 32-agent bitmap rollout (block size; four-column
 *                        table with made-up STAY rows; never 4-byte delta rows)
 *   step_big=0|1|2       the single step's resident grid with the move table in LDS: never / by batch (default) / whenever it fits
 *   step_delta=0|1|2     ... with 4-byte delta rows (64x64 maps): never / from one full residency on (default) / whenever it fits
 *   step_block=64|128|256|512   block size of the plain packed single step
 *   step_grid=n          at most n blocks in the grid of the single step's resident forms (step_big, step_delta): each block then walks
 *                        more chunks of the batch (tests; 0, the default: by the device's CU count; the plain step ignores it)
 *   policy_table_lds=0|1 the packed rollout under MAPF_POLICY_TABLE: action bytes gathered from global memory / from a copy of the
 *                        policy table staged into LDS behind the table image whenever one block's segment fits (default: by shape)
 *   limit_packed=0|1     a rollout under MAPF_POLICY_TABLE and an episode step limit (mapf_set_episode_limit): always the lane-group
 *                        limit kernels (0, the default) / the packed table kernels' limit forms wherever the packed table plan
 *                        applies (1; not on a handle created with MAPF_FLAG_LANE_GROUP).  Same results either way.  A handle with an
 *                        episode budget (mapf_set_episode_budget) takes the lane-group budget kernels whatever this key says.
 */

/* Replaces MapfEnv.__init__'s state setup; state = start cells, step index t = 0. */
int mapf_create(const mapf_desc *desc, mapf_handle_t *out_handle);
int mapf_destroy(mapf_handle_t h);

/*
 * MapfEnv.reset() (mapf_env.py:290-293) for every env, or for the envs whose
 * mask byte is non-zero (mask: u8[E] or NULL).  Does not touch the RNG counters.
 */
int mapf_reset(mapf_handle_t h, const uint8_t *mask);

/*
 * MapfEnv.step() (mapf_env.py:237-266) for all E envs in one kernel launch.
 *   actions   u8 [E*A]   per-agent actions (the decoded joint action, :242-243)
 *   uniforms  f64[E*A]   the rand() values the reference would draw in agent order
 *                        (:255), or NULL: drawn on device from Philox4x32-10 keyed by
 *                        (seed; global env id, step index t, agent) -- the exact counter layout is
 *                        oracle/philox.py's (since ABI 4: one call per agent QUAD per two steps; ABI 3
 *                        used one per agent pair per four steps, so the same seed draws other
 *                        numbers than it did there)
 *   out_local u16[E*A]   the state step() returns, as per-agent cells
 *   out_reward f64[E], out_done u8[E], out_collision u8[E], out_prob f64[E]
 *   out_was_terminal u8[E]: 1 where the env was already terminal, i.e. the reference
 *                        returned (s, 0, True, {"prob": 0}) and drew nothing (:239-240)
 * Any out_* may be NULL.  Increments the handle's step index t.
 */
int mapf_step(mapf_handle_t h, const uint8_t *actions, const double *uniforms,
              uint16_t *out_local, double *out_reward, uint8_t *out_done,
              uint8_t *out_collision, double *out_prob, uint8_t *out_was_terminal,
              uint32_t step_flags);

/*
 * T fused steps in ONE launch (the caller-side loop around step()):
 * state stays in registers, actions are streamed from `actions` u8[T*E*A] (step-major) or,
 * when NULL, drawn from the policy stream (uniform over the 5 actions, key seed + 1).
 * Every reward is added, in step order, to out_returns f64[E]; out_episodes u32[E] counts
 * steps that returned done; out_collisions u32[E] counts collision steps.  Optional
 * trajectory recording (any pointer may be NULL), step-major like `actions`:
 *   rec_local u16[T*E*A], rec_reward f64[T*E], rec_done u8[T*E], rec_collision u8[T*E],
 *   rec_prob f64[T*E].
 * Advances t by T.  Equivalent to T mapf_step calls with the same flags.
 */
typedef struct mapf_rollout_io {
    uint32_t struct_size;
    uint32_t n_steps;           /* T */
    uint32_t step_flags;        /* MAPF_STEP_* */
    uint32_t accumulate;        /* 0: out_* are overwritten; 1: added to existing values */
    const uint8_t *actions;     /* [T*E*A] or NULL */
    double   *out_returns;      /* [E] or NULL */
    uint32_t *out_episodes;     /* [E] or NULL */
    uint32_t *out_collisions;   /* [E] or NULL */
    uint16_t *rec_local;
    double   *rec_reward;
    uint8_t  *rec_done;
    uint8_t  *rec_collision;
    double   *rec_prob;
} mapf_rollout_io;
int mapf_rollout(mapf_handle_t h, const mapf_rollout_io *io);

/*
 * Episode step limit (ABI 6): "n episodes of at most max_steps steps" inside the fused rollout and the single step -- what a
 * planner's evaluation loop or gym's TimeLimit wrapper does around MapfEnv.step (mapf_env.py:237-266) on the host; the
 * reference itself has no limit.  THE DEFINITION.  A handle has a limit N (u32; 0 = none, the default) and a per-env age a
 * (u32[E], device memory, all zero at mapf_create).  For every env and every step taken while N > 0:
 *   1. the env is terminal on entry (the no-op of mapf_env.py:239-240): outputs as without a limit, truncated = 0, a unchanged;
 *   2. otherwise a' = a + 1, saturating at 2^32 - 1; transition, reward, prob, done and collision are exactly those without a
 *      limit; truncated = !done && a' >= N;
 *   3. with MAPF_STEP_AUTO_RESET and done || truncated: the state becomes the start cells (as the reset on done) and a' = 0;
 *   4. without auto-reset the state is the next state and a' is kept: a truncated env goes on living and reports
 *      truncated = 1 on every later live step until someone resets it.
 * Truncation changes no reward, no done, no collision, no returns / episodes / collisions total and no Philox counter (the
 * streams are keyed by (env, step index, agent), not by episode).  The ages go back to zero: for the envs a mapf_reset(mask)
 * resets; for all envs in mapf_set_state with cells (with only t they stay) and in EVERY mapf_set_episode_limit call.
 * With N == 0 every launch, kernel instance and output is what it is without this feature.
 *
 * mapf_set_episode_limit: refused (MAPF_EINVAL) while recording and while recorded graphs live, as mapf_set_policy_table is;
 *   a handle with a limit refuses mapf_graph_begin with MAPF_EUNSUPPORTED.
 * mapf_episode_steps: out_age u32[E] receives the ages, then set_age u32[E] replaces them (either may be NULL, not both; set_age
 *   needs a limit); HOST pointers, or DEVICE pointers on a MAPF_FLAG_DEVICE_PTRS handle (then only enqueued).
 * mapf_rollout keeps its argument block (mapf_rollout_io stays as it is, its struct_size check an equality): on a handle with a
 *   limit it applies the limit and reports no truncation.  mapf_rollout_limited is mapf_rollout plus out_truncations u32[E]
 *   (counts the truncated steps per env; io->accumulate applies to it) and rec_truncated u8[T*E] (the flag per step, step-major,
 *   recorded like rec_done); either may be NULL, non-NULL on a handle without a limit is MAPF_EINVAL.
 * mapf_step keeps its signature: on a handle with a limit it applies the limit and reports no flag; mapf_step_limited is
 *   mapf_step plus out_truncated u8[E] (NULL allowed; non-NULL on a handle without a limit: MAPF_EINVAL).
 * Everything is validated on the host before any device work.  Limit launches run the lane-group kernels' limit instances
 * whatever the handle's family flag, and mapf_last_kernel says LIMIT.
 * Out of scope: limit forms of the packed (lq_*) rollout and step kernels and of the thread-per-env family (a handle with a
 * limit gives up their speed: README has the numbers), recorded graphs, the multi-map / union-map wrappers and the scalar
 * MapfEnv of the Python package, a "time-out reward".
 */
int mapf_set_episode_limit(mapf_handle_t h, uint32_t max_steps);
int mapf_episode_steps(mapf_handle_t h, uint32_t *out_age, const uint32_t *set_age);
int mapf_rollout_limited(mapf_handle_t h, const mapf_rollout_io *io, uint32_t *out_truncations, uint8_t *rec_truncated);
int mapf_step_limited(mapf_handle_t h, const uint8_t *actions, const double *uniforms,
                      uint16_t *out_local, double *out_reward, uint8_t *out_done,
                      uint8_t *out_collision, double *out_prob, uint8_t *out_was_terminal,
                      uint8_t *out_truncated, uint32_t step_flags);

/*
 * Episode budget (ABI 6, new symbols only): fused rollouts that stop each env after n episodes -- the other half of "n episodes of
 * at most max_steps steps".  A rollout with auto-reset runs every env for exactly T steps, so envs whose episodes end quickly run
 * more of them (pooled returns / episodes over-weight short episodes) and returns[e] ends with the rewards of an episode the launch
 * cut off.  THE DEFINITION.  A handle has an episode budget B (u32; 0 = none, the default) and a per-env count left (u32[E], device
 * memory, all zero at mapf_create).  An env is PARKED when B > 0 and left[e] == 0.  The budget applies to mapf_rollout* launches that
 * carry MAPF_STEP_AUTO_RESET.  For every env and step of such a launch:
 *   0. parked on entry: nothing happens.  State, age and left are unchanged, nothing is drawn from either stream, no total changes
 *      (returns stays bit for bit what it was, an accumulated -0.0 included); a recording launch writes the env's current cells,
 *      reward +0.0, prob +0.0, done 0, collision 0, truncated 0.  A parked row is recognisable by done == 0 && prob == 0;
 *   1. otherwise the four rules of the episode limit apply unchanged (with N == 0 truncated is always 0 and the ages stay zero);
 *      rule 1, the terminal-on-entry no-op, is part of this;
 *   2. live_steps[e] counts the steps that were neither parked nor terminal on entry;
 *   3. a step that reports done or truncated takes one from left[e] -- the terminal no-op too, which episodes counts as well.  The
 *      env goes back to its start cells and age 0 as under auto-reset, also when left reaches 0: a parked env stands on its start
 *      cells with age 0, and re-arming it begins a fresh batch of episodes.
 * Since arming, B - left[e] == episodes[e] + truncations[e], which is B once the env is parked.  Truncation and parking change no
 * Philox counter; the step index advances by T as always.
 *
 * mapf_set_episode_budget: sets B and left[e] = n_episodes for every env (every call re-arms all envs); touches neither state nor
 *   ages; refused (MAPF_EINVAL) while recording and while recorded graphs live, as mapf_set_episode_limit is.
 * mapf_episodes_left: out_left u32[E] receives the counts, then set_left u32[E] replaces them (per-env budgets, re-arming single
 *   envs; needs a budget); the pointer rules of mapf_episode_steps.
 * mapf_rollout_budgeted is mapf_rollout_limited plus out_live_steps u32[E] (io->accumulate applies to it; NULL allowed, non-NULL on a
 *   handle without a budget: MAPF_EINVAL).  The truncation pointers need a limit, as there.  mapf_rollout and mapf_rollout_limited
 *   on a handle with a budget apply the budget and report no live steps.
 * On a handle with a budget a rollout without MAPF_STEP_AUTO_RESET returns MAPF_EINVAL; mapf_step, mapf_step_limited and
 *   mapf_graph_begin return MAPF_EUNSUPPORTED.  mapf_reset(mask), mapf_set_state and mapf_set_episode_limit leave left alone.
 * Everything is validated on the host before any device work.  Budget launches run the lane-group kernels' budget instances
 * whatever the handle's family flag or limit_packed, and mapf_last_kernel says BUDGET; with B == 0 every launch, kernel instance
 * and name is what it is without this feature.
 * Out of scope: budget forms of the packed (lq_*) and thread-per-env kernels (a handle with a budget takes the lane-group speed),
 * the single step and recorded graphs, the multi-map / union-map wrappers and the scalar MapfEnv, discounting.  (The per-episode
 * log is mapf_set_episode_log, below.)
 * No policy is computed on the device.
 */
int mapf_set_episode_budget(mapf_handle_t h, uint32_t n_episodes);
int mapf_episodes_left(mapf_handle_t h, uint32_t *out_left, const uint32_t *set_left);
int mapf_rollout_budgeted(mapf_handle_t h, const mapf_rollout_io *io, uint32_t *out_truncations, uint8_t *rec_truncated, uint32_t *out_live_steps);

/*
 * Conflict matrix (ABI 6, new symbols only): fused rollouts that count WHICH agent pairs collide -- what a planner that solves
 * agents or groups apart and joins their policies needs to know before it merges groups and replans.  A totals-only rollout
 * reports one collisions count per env; the pairs behind it otherwise cost a recording rollout and an O(T * E * A^2) pass over it.
 * THE DEFINITION.  A handle has a conflict matrix M, or none (the default).  M is u64[n_slots, A, A] in device memory, and every env
 * has a slot, slot[e] < n_slots.  For every env e and every step of a mapf_rollout, mapf_rollout_limited or mapf_rollout_budgeted
 * launch -- any action source, recording or not, auto-reset or not -- that is not a no-op on entry (a no-op: an env that is
 * terminal on entry, mapf_env.py:239-240, or parked by the budget), with prev the cells on entry and next the sampled cells
 * before any reset, for every i < j < A:
 *   next[i] == next[j], a vertex conflict (mapf_env.py:386-387):            M[slot[e]][i][j] += 1  (the upper triangle);
 *   prev[i] == next[j] && prev[j] == next[i], a swap (mapf_env.py:382-384): M[slot[e]][j][i] += 1  (the lower triangle).
 * ALL conflicting pairs of a step count, not the first one only; the diagonal is never written.  A non-terminal state has
 * distinct cells, so a pair is never both, and a live step reports collision exactly when it adds at least one count.
 * The mode changes nothing else: state, outputs, totals, ages, left, both Philox streams and the step index are bit for bit those
 * of the same launch with the mode off.  Counts of shards add: the matrices of two handles that split a batch by env_id_offset
 * sum to the whole batch's matrix.
 *
 * mapf_set_conflict_pairs: n_slots == 0 switches the mode off and frees M; otherwise it allocates M, and slot_of_env u32[E] -- a
 *   HOST pointer in every handle mode -- is copied (NULL: every env in slot 0).  Every call zeroes M.  MAPF_EINVAL for a null
 *   handle, a slot >= n_slots, or n_slots * A * A * 8 > 2^30 bytes; refused (MAPF_EINVAL) while recording and while recorded
 *   graphs live, as mapf_set_episode_limit is.  A handle with the mode on refuses mapf_graph_begin with MAPF_EUNSUPPORTED.
 * mapf_conflict_pairs: out u64[n_slots * A * A] receives M -- a HOST pointer, or a DEVICE pointer on a MAPF_FLAG_DEVICE_PTRS
 *   handle (then only enqueued) -- and then M is zeroed if zero != 0.  out == NULL is allowed with zero; both absent, or the mode
 *   off, is MAPF_EINVAL.
 * mapf_step* count nothing and stay as they are (a single step hands back the cells: the caller can count for itself).
 *   mapf_reset, mapf_set_state, mapf_set_episode_limit and mapf_set_episode_budget leave M alone.
 * Everything is validated on the host before any device work.  Launches of a handle with the mode on run the lane-group kernels'
 * instances that count, whatever the handle's family flag or limit_packed, and mapf_last_kernel says PAIRS, next to LIMIT or
 * BUDGET where those apply; with the mode off every launch, kernel instance and name is what it is without this feature.
 * Out of scope: packed (lq_*) and thread-per-env forms (a handle with the mode on takes the lane-group speed, as one with a budget
 * does), the single step and recorded graphs, the multi-map / union-map wrappers and the scalar MapfEnv, per-step logs of
 * conflicts, anything that merges groups or replans on the device.  (How each episode ended -- by a collision or not -- is in the
 * episode log, below; which pair collided in which episode is not.)
 */
int mapf_set_conflict_pairs(mapf_handle_t h, uint32_t n_slots, const uint32_t *slot_of_env);
int mapf_conflict_pairs(mapf_handle_t h, uint64_t *out, int zero);

/*
 * Episode log (ABI 6, new symbols only): fused rollouts that record EVERY FINISHED EPISODE per env -- its return, its length and
 * how it ended -- where the totals of a budgeted evaluation keep one sum per env.  What comparing two plans needs: the spread of
 * the returns (a standard error per start state), the distribution of the episode lengths, which episode ended how.  The route to
 * those is otherwise a recording rollout and a pass over its [T, E] arrays.
 * THE DEFINITION.  A handle has an episode log of capacity C (0 = none, the default).  Per env it keeps acc, an f64 running return;
 * len, a u32 count of running live steps; count, a u32 count of episodes ended since the last clear; and C records of 16 bytes.
 * The log applies to the launches the budget applies to: mapf_rollout* with MAPF_STEP_AUTO_RESET on a handle with B > 0.  For
 * every env and step, after the budget's rules have produced the step's reward, done, collision and truncated:
 *   parked on entry: nothing changes.
 *   otherwise: acc = acc + reward -- ONE float64 add, in step order; the terminal-on-entry no-op adds its +0.0 -- and len += 1 if
 *     the step was live (neither parked nor terminal on entry).
 *   if the step reports done or truncated: the record {acc, len, done | collision << 1 | truncated << 2} is stored at
 *     records[e][count] if count < C; then count += 1 (saturating), acc = +0.0, len = 0.  Episodes beyond C are counted and not
 *     stored: the caller sees count > C.
 * A terminal-start no-op therefore logs {+0.0, 0, 1}.  An env's record returns, summed, need not be bit-equal to the totals'
 * out_returns: the additions associate differently.
 * The log changes nothing else: state, outputs, totals, ages, left, the conflict matrix, both Philox streams and the step index
 * are bit for bit those of the same launch with the log off.  Records of shards (env_id_offset) concatenate.
 * acc and len are zeroed in every mapf_set_episode_log call, for the envs a mapf_reset(mask) resets, and for all envs in
 * mapf_set_state with cells.  mapf_set_episode_limit, mapf_set_episode_budget, mapf_episodes_left(set_left) and a clear leave them
 * alone: an episode that spans a clear or a re-arm is logged whole.
 *
 * mapf_set_episode_log: allocates and zeroes the records, the counts and the partials; capacity 0 frees them and switches the mode
 *   off.  MAPF_EINVAL for a null handle, capacity > 0 on a handle without a budget, E * C * 16 > 2^31 bytes; refused (MAPF_EINVAL)
 *   while recording and while recorded graphs live, as mapf_set_episode_budget is.  With a log on, mapf_set_episode_budget(h, 0) is
 *   MAPF_EINVAL (switch the log off first) and mapf_graph_begin is MAPF_EUNSUPPORTED.
 * mapf_episode_log: out_records [E * C] and out_count u32[E] receive the records (env e's k-th at e * C + k; the slots from
 *   count on are zero) and the counts -- HOST pointers, or DEVICE pointers on a MAPF_FLAG_DEVICE_PTRS handle (then only enqueued),
 *   the rules of mapf_conflict_pairs; either may be NULL.  With clear != 0 records and counts are then zeroed; the partials are not.
 *   All three absent, or the mode off, is MAPF_EINVAL.
 * Everything is validated on the host before any device work, pointers first.  Launches of a handle with the mode on run the
 * lane-group kernels' log instances -- always the budget plan -- and mapf_last_kernel says LOG next to BUDGET; with the mode off
 * every launch, kernel instance and name is what it is without this feature.
 * Out of scope, as for the budget: packed and thread-per-env forms, the single step and recorded graphs, the multi-map /
 * union-map wrappers and the scalar MapfEnv, discounting.
 */
typedef struct mapf_episode_record { double ret; uint32_t steps; uint32_t outcome; } mapf_episode_record;
#define MAPF_EPISODE_DONE      0x1u          /* outcome bits: the last step reported done ... */
#define MAPF_EPISODE_COLLISION 0x2u          /* ... by a collision (3 = done | collision; 1 alone: on the goals) */
#define MAPF_EPISODE_TRUNCATED 0x4u          /* the episode step limit cut it */
int mapf_set_episode_log(mapf_handle_t h, uint32_t capacity);
int mapf_episode_log(mapf_handle_t h, mapf_episode_record *out_records, uint32_t *out_count, int clear);

/* Synthetic policy used by bench/rollout: fills actions u8[n_steps*E*A] for step indices
 * t0 .. t0+n_steps-1 from the policy stream (oracle/philox.py random_actions_np; ABI 5: key seed + 1, ONE Philox
 * call per agent quad per FOUR steps -- counter (env, t >> 2, quad), word t & 3, byte agent & 3, action =
 * (byte * 5) >> 8; ABI <= 4 drew one call per quad per step and a 32-bit word per action). */
int mapf_fill_random_actions(mapf_handle_t h, uint8_t *actions, uint64_t t0, uint32_t n_steps);

/*
 * On-device policy of mapf_rollout calls that pass actions == NULL (the reference has no policy; this stands in
 * for the caller-side `a = policy(s)` of the loop around MapfEnv.step).
 *   MAPF_POLICY_RANDOM (default): the uniform-random policy stream, as mapf_fill_random_actions.
 *   MAPF_POLICY_GREEDY: every agent takes the first action in ACTIONS order (STAY, UP, RIGHT, DOWN, LEFT) whose
 *     intended target cell is closest (Manhattan distance over grid rows / columns) to its goal -- i.e. the first
 *     unblocked move that brings it one step closer, else STAY.  Slip still applies.  cell_rc u32[V] (HOST
 *     pointer, copied): row | col << 16 of every free cell (rows and columns below 65536).
 */
#define MAPF_POLICY_RANDOM 0
#define MAPF_POLICY_GREEDY 1
int mapf_set_policy(mapf_handle_t h, int policy, const uint32_t *cell_rc);

/*
 * MAPF_POLICY_TABLE: a per-agent lookup-table policy followed INSIDE the fused rollout -- the caller's plan.  It stands
 * in for the caller-side `a = policy(s)` of the loop around MapfEnv.step (reference mapf_env.py:237-266) when the
 * joint policy is a join of single-agent policies, which is what the reference's planning workflow produces: each
 * agent is solved on its own local view (gym_mapf/envs/utils.py:get_local_view) and a single-agent policy of a local
 * view is a function cell -> action, i.e. one row of V bytes.
 *   table u8[n_rows * V]: table[r * V + cell] is the action (0..4, the action codes above) of an agent that follows
 *     row r and stands on `cell`.  1 <= n_rows <= 65536.
 *   row_index u16[E * A] (u16[A] with MAPF_POLICY_ROWS_BROADCAST): the row agent i of local env e follows.
 * Both are HOST pointers in every handle mode and are copied (as cell_rc above).  In mapf_rollout calls with
 * actions == NULL agent i of env e on cell c then takes table[row_index[e * A + i] * V + c]; slip, collisions, reward,
 * termination, auto-reset and the slip stream's counters are exactly those of a mapf_step with that action, the policy
 * stream is not drawn (as under MAPF_POLICY_GREEDY), an env that is terminal on entry is a no-op.  Everything is
 * validated on the host before any device work (MAPF_EINVAL: null handle / table / row_index, n_rows out of range, a
 * table byte > 4, a row index >= n_rows, unknown flag bits); refused while recording and while recorded graphs live.
 * mapf_set_policy(h, MAPF_POLICY_RANDOM | MAPF_POLICY_GREEDY, ...) leaves table mode and frees the copies.
 * mapf_last_kernel(h, MAPF_KERNEL_ROLLOUT) of a table launch says TABLE where a streamed one says STREAM.
 * Out of scope: a policy argument for the single mapf_step, the multi-map / union-map wrappers and the scalar MapfEnv
 * of the Python package, anything that COMPUTES a policy on the device.  Tables over the joint states of merged agent
 * PAIRS are MAPF_POLICY_JOINT, below.
 */
#define MAPF_POLICY_TABLE 2
#define MAPF_POLICY_ROWS_BROADCAST 0x1u      /* row_index is [A], shared by all envs */
int mapf_set_policy_table(mapf_handle_t h, const uint8_t *table, uint32_t n_rows,
                          const uint16_t *row_index, uint32_t flags);

/*
 * MAPF_POLICY_JOINT: the table policy for plans in which some agent pairs were merged and replanned jointly (the
 * reference's get_local_view(env, [i, j])): a merged agent's action is a function of its own cell AND its partner's.
 *   table u8[table_bytes]: action codes 0..4.  1 <= table_bytes <= 2^31 - 1.
 *   offset u32[E * A] (u32[A] with MAPF_POLICY_ROWS_BROADCAST): where the segment of agent i of local env e begins.
 *   partner u16[E * A] (u16[A] likewise): the agent that i is merged with, or i itself.
 * All three are HOST pointers in every handle mode and are copied, as in mapf_set_policy_table.
 *   Solo agent: partner[e,i] == i.  On cell c it takes table[offset[e,i] + c]; its segment is V bytes.
 *   Merged agent: partner[e,i] == j != i.  On cell c_i, with j on c_j, it takes table[offset[e,i] + c_i * V + c_j]; its
 *     segment is V * V bytes.
 * Each agent has its own segment: a pair's joint plan is two [V, V] byte arrays, each indexed by (own cell, partner's
 * cell).  Segments may be shared between agents and envs, and they may overlap.
 * Everything else is as under MAPF_POLICY_TABLE: the cells are those on entry to the step, after any auto-reset; slip,
 * collisions, reward, termination, both Philox streams' counters, the episode limit, the episode budget and the conflict
 * matrix are exactly those of a mapf_step with these actions; the policy stream is not drawn; a terminal or parked step
 * is a no-op.  A rollout with streamed actions ignores the policy; mapf_step* are unaffected.
 * Validated on the host before any device work, MAPF_EINVAL with a mapf_last_error that names the offending index: null
 * handle or pointer; table_bytes 0 or above 2^31 - 1; a table byte above 4; partner[e,i] >= A;
 * partner[e, partner[e,i]] != i; a segment that ends past table_bytes (computed in 64 bits); unknown flag bits.  Refused
 * while recording and while recorded graphs live; mapf_graph_begin refuses a handle in joint mode.
 * mapf_set_policy(h, MAPF_POLICY_RANDOM | MAPF_POLICY_GREEDY, ...) and mapf_set_policy_table leave joint mode and free
 * the copies; mapf_set_policy_joint leaves table mode.  mapf_set_policy(h, MAPF_POLICY_JOINT, ...) is MAPF_EINVAL.
 * mapf_last_kernel(h, MAPF_KERNEL_ROLLOUT) of a joint launch says _joint and JOINT: always a lane-group kernel.
 * Groups of three or more, whose dense form would cost V^3 bytes per agent, are MAPF_POLICY_GROUP, below (sparse books).
 * Out of scope: a policy argument for mapf_step, packed and thread-per-env forms,
 * the multi-map / union-map wrappers and the scalar MapfEnv, graph recording of joint launches, anything that computes
 * a policy on the device.
 */
#define MAPF_POLICY_JOINT 3
int mapf_set_policy_joint(mapf_handle_t h, const uint8_t *table, uint64_t table_bytes,
                          const uint32_t *offset, const uint16_t *partner, uint32_t flags);

/*
 * MAPF_POLICY_GROUP: the table policy for plans in which groups of two to four agents were merged and replanned jointly
 * on the joint cells the planner visited (RTDP, a windowed joint search, a local repair around the conflict cells): the
 * form is SPARSE.  Every agent has a solo row, as under MAPF_POLICY_TABLE; every group has a BOOK of entries (joint cell ->
 * the members' actions).  An agent of a group takes its action from the entry of the group's current joint cell if the
 * book has one, and otherwise from its solo row.  Also serves a pair with a small repair book in place of 2 * V * V bytes.
 *   table u8[n_rows * V], row_index u16[E * A]: the solo rows, MAPF_POLICY_TABLE's two arrays.
 *   members u16[E * A * 4]: members[e,i] lists the agents of i's group in ascending order, padded at the end with 0xFFFF.
 *     The list contains i; every agent in it carries the identical list; its size G is 1..4, G == 1 a solo agent.
 *   book u32[E * A]: book[e,i] names the group's book: the same for all members and below n_books; ignored for a solo agent.
 *   entries mapf_group_entry[n_entries], book_begin u32[n_books + 1]: book b is entries[book_begin[b] .. book_begin[b+1]);
 *     book_begin[0] == 0, book_begin[n_books] == n_entries, non-decreasing.  n_books == 0 with n_entries == 0 is legal: every
 *     group then falls back to its rows, and book is not read.
 * With MAPF_POLICY_ROWS_BROADCAST row_index, members and book are [A], [A * 4] and [A] TOGETHER, shared by all envs.
 * All pointers are HOST pointers in every handle mode and are copied.
 *   The key of a group in a step is the four u16 (c[m0], c[m1], ...): the members' cells on entry to the step, after any
 *   auto-reset, with 0xFFFF at the padded positions.  An entry matches when its four cells equal the key; an entry of another
 *   arity never matches.
 *   Agent i at position p of its group, G >= 2, with a matching entry in the group's book, takes entry.action[p].  Every other
 *   agent-step takes table[row_index[e,i] * V + c_i].
 * Everything else is as under MAPF_POLICY_JOINT: slip, collisions, reward and termination are exactly those of a mapf_step
 * with these actions, and so are both Philox streams' counters, the episode limit, the episode budget, the conflict matrix
 * and the episode log; the policy stream is not drawn; terminal and parked steps are no-ops; a rollout with streamed
 * actions ignores the policy; mapf_step* are unaffected.
 * Validated on the host before any device work, MAPF_EINVAL with a mapf_last_error that names the offending index: null
 * handle or pointer (entries and book_begin may be NULL only when n_entries == 0 && n_books == 0); the table policy's own
 * checks; a member >= A that is not padding, padding that is not trailing, a list that is not ascending, a list without i;
 * a member whose list (or book) differs; book[e,i] >= n_books for G >= 2 (n_books > 0); a broken book_begin; an entry cell >= V that is
 * not 0xFFFF, padding in an entry that is not trailing; an action above 4, a nonzero action at a padded position; two
 * entries of one book with the same four cells; n_entries > 2^24; unknown flag bits.  V = 65536 would make cell 0xFFFF
 * ambiguous: the mode needs V <= 65535 (MAPF_EUNSUPPORTED otherwise).
 * Refused while recording and while recorded graphs live; mapf_graph_begin refuses a handle in the mode; a refused call
 * leaves the previous policy in force.  mapf_set_policy(h, MAPF_POLICY_RANDOM | MAPF_POLICY_GREEDY, ...),
 * mapf_set_policy_table and mapf_set_policy_joint leave the mode and free the copies; mapf_set_policy(h,
 * MAPF_POLICY_GROUP, ...) is MAPF_EINVAL.  mapf_last_kernel(h, MAPF_KERNEL_ROLLOUT) of a group launch says _group and GROUP
 * where a joint launch says _joint and JOINT: always a lane-group kernel.
 * On the device all books lie in one open-addressing table of 16-byte slots (capacity: a power of two >= 2 * n_entries,
 * linear probing); a lookup reads at most as many slots as the longest chain the host produced while building it.
 * Out of scope: groups of five or more; packed and thread-per-env forms; the single step; recorded graphs; the multi-map
 * and union-map wrappers and the scalar MapfEnv; anything that computes or repairs a plan on the device.
 */
#define MAPF_POLICY_GROUP 4
typedef struct mapf_group_entry { uint16_t cell[4]; uint8_t action[4]; } mapf_group_entry;   /* 12 bytes */
int mapf_set_policy_group(mapf_handle_t h, const uint8_t *table, uint32_t n_rows, const uint16_t *row_index,
                          const uint16_t *members, const uint32_t *book,
                          const mapf_group_entry *entries, uint64_t n_entries,
                          const uint32_t *book_begin, uint32_t n_books, uint32_t flags);
/* The device table of a handle in the mode (MAPF_EINVAL otherwise): its slots, and the longest probe chain.  No device touched. */
int mapf_policy_group_stats(mapf_handle_t h, uint64_t *slots, uint32_t *max_probe);

/*
 * MapfEnv.P[s][a] (mapf_env.py:448-478 _get_transitions): for each of n_queries (state, joint action) pairs,
 * every branch of the joint slip distribution, in the reference's order (itertools.product over the agents'
 * merged movement lists, agent 0 slowest).  Does not touch the handle's env state or step index.
 *   local u16[N*A], actions u8[N*A]; env_index u32[N] selects whose goals apply (NULL: env 0)
 *   max_branches M: rows reserved per query (3^A always suffices); out_count u32[N] reports the true number
 *   out_next u16[N*M*A], out_prob f64[N*M], out_reward f64[N*M], out_done u8[N*M], out_collision u8[N*M]
 * Rows b >= out_count[q] are left untouched.  A terminal state yields one branch (prob 1.0, reward 0, done).
 * Supported for n_agents <= 16 (3^A branches per query: up to 43 M -- page through them with
 * mapf_transitions_window; planners decompose larger problems with get_local_view).  Any out_* may be NULL.
 */
int mapf_transitions(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                     const uint32_t *env_index, uint32_t max_branches, uint32_t *out_count, uint16_t *out_next,
                     double *out_prob, double *out_reward, uint8_t *out_done, uint8_t *out_collision);
/* The same enumeration, one WINDOW at a time: row j of query q's outputs holds branch first_branch + j (rows whose
 * branch index is >= out_count[q] are left untouched); out_count always reports the full branch count.  The reference
 * builds the whole list at once (mapf_env.py:465-476); for more than ~8 agents that list does not fit anywhere. */
int mapf_transitions_window(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                            const uint32_t *env_index, uint64_t first_branch, uint32_t max_branches, uint32_t *out_count,
                            uint16_t *out_next, double *out_prob, double *out_reward, uint8_t *out_done,
                            uint8_t *out_collision);

/*
 * The same enumeration with COMPACTED rows (ABI 5): the window [first_branch, first_branch + max_branches) of every query,
 * back to back -- query q's rows are rows out_offset[q] .. out_offset[q + 1] - 1 of every output array, in the reference's
 * branch order (mapf_env.py:465-476 builds exactly such a list per (s, a); a query reserves 3^A rows in the calls above and
 * a room map fills a fifth of them, so a planner that sweeps many states wants them dense).
 *   out_offset u64[N + 1] (required): exclusive scan of the windows' lengths; out_offset[N] = the number of rows needed;
 *   capacity_rows: rows the out_* arrays hold -- rows at or beyond it are NOT written (no overrun): a caller checks
 *     out_offset[N] <= capacity_rows (after mapf_sync in device-pointer mode) and calls again with larger arrays if not;
 *   out_count u32[N] (optional): the FULL branch count of every query, as above;
 *   out_next u16[R*A], out_prob f64[R], out_reward f64[R], out_done u8[R], out_collision u8[R] with R = capacity_rows.
 * Three launches: window lengths + block-local scan, scan of the block totals, rows.  n_agents <= 16.
 */
int mapf_transitions_compact(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                             const uint32_t *env_index, uint64_t first_branch, uint32_t max_branches, uint64_t capacity_rows,
                             uint64_t *out_offset, uint32_t *out_count, uint16_t *out_next, double *out_prob, double *out_reward,
                             uint8_t *out_done, uint8_t *out_collision);

/*
 * MapfEnv.calc_transition_reward_from_local_states (mapf_env.py:225-235, with _living_reward :436-446 and
 * _is_collision_transition_from_local_states :378-389) for n_queries given transitions:
 *   prev_local u16[N*A], actions u8[N*A] (the decoded joint action), next_local u16[N*A];
 *   env_index u32[N] selects whose goals apply (NULL: env 0);
 *   out_reward f64[N], out_done u8[N], out_collision u8[N]  (the method's (reward, done, collision) triple).
 * Like the reference method it does not test is_terminal(prev).  Any n_agents; any out_* may be NULL.
 */
int mapf_transition_rewards(mapf_handle_t h, uint64_t n_queries, const uint16_t *prev_local, const uint8_t *actions,
                            const uint16_t *next_local, const uint32_t *env_index, double *out_reward, uint8_t *out_done,
                            uint8_t *out_collision);

/* MapfEnv.is_terminal (mapf_env.py:210-223) of every env's CURRENT state: out_terminal u8[E] is 1
 * where two agents share a cell or every agent is on its goal (a step there is a no-op). */
int mapf_query_terminal(mapf_handle_t h, uint8_t *out_terminal);

/* env.s as per-agent cells + the step index (the whole mutable state: the RNG is
 * counter-based).  set_state validates cells < V. */
int mapf_get_state(mapf_handle_t h, uint16_t *local, uint64_t *t);
int mapf_set_state(mapf_handle_t h, const uint16_t *local, uint64_t t);

/*
 * The handle's state buffer itself: out_state receives a DEVICE pointer to u16[E*A], env.s of every env as per-agent cells
 * -- after a step with MAPF_STEP_AUTO_RESET that is the state the next step starts from (a finished episode shows its start
 * cells, the usual vector-env convention; mapf_step's out_local reports the state step() itself returned).  A caller that
 * reads the next observation here passes out_local = NULL to mapf_step and the step writes the cells ONCE.  The pointer
 * stays valid for the handle's lifetime; its contents change with every step / rollout / reset / set_state enqueued on
 * the handle's stream (read it on that stream or after mapf_sync).  No reference counterpart: MapfEnv.s (mapf_env.py:265).
 */
int mapf_state_view(mapf_handle_t h, const uint16_t **out_state);

/*
 * The view is READ-ONLY (const): the library tracks on the host whether some env can be terminal (after a step that
 * auto-reset every finished episode none can) and then runs the step instance without is_terminal(prev)
 * (mapf_env.py:238-240).  A caller that writes the state buffer itself (custom reset, curriculum) -- through a
 * cast of this pointer, or a framework tensor that wraps it -- must say so BEFORE the next step / rollout:
 * mapf_invalidate_state makes the next launches test is_terminal(prev) again, as mapf_set_state does.  (ABI 4.)
 */
int mapf_invalidate_state(mapf_handle_t h);

/*
 * Recording the caller-side loop around MapfEnv.step (mapf_env.py:237-266) into a hipGraph.  Between mapf_graph_begin and
 * mapf_graph_end every mapf_step / mapf_rollout / mapf_reset / mapf_fill_random_actions call on a MAPF_FLAG_DEVICE_PTRS
 * handle is recorded on the handle's stream instead of executed (work the caller enqueues on that stream in between --
 * e.g. its policy network -- is recorded with it).  mapf_graph_launch replays the recording n_replays times; the step
 * index t is kept in device memory for recorded launches and advanced by the recording's last node, so every replay draws
 * fresh random numbers: K replays of an N-step recording produce exactly the results of K*N mapf_step calls with the same
 * arguments.  The arrays named in recorded calls must stay allocated while the graph lives.  Calls that wait for the
 * stream or move the step index from the host (mapf_sync, mapf_timer_*, mapf_get_state, mapf_set_state, mapf_set_policy)
 * fail with MAPF_EINVAL while recording, as does recording on a host-pointer handle.  A mapf_step / mapf_rollout enqueued while
 * the CALLER captures the stream it gave the handle (hipStreamBeginCapture, torch.cuda.graph) is refused too: it would
 * bake its step index -- and random numbers -- into the caller's graph; record it here instead.  Recordings that are
 * still alive are destroyed with their handle.
 */
typedef struct mapf_graph_s *mapf_graph_t;
int mapf_graph_begin(mapf_handle_t h);
int mapf_graph_end(mapf_handle_t h, mapf_graph_t *out_graph);
int mapf_graph_launch(mapf_handle_t h, mapf_graph_t graph, uint32_t n_replays);
int mapf_graph_steps(mapf_graph_t graph, uint64_t *out_steps);   /* env-steps one replay advances the handle by */
int mapf_graph_destroy(mapf_handle_t h, mapf_graph_t graph);

/* Block until everything enqueued on the handle's stream has finished. */
int mapf_sync(mapf_handle_t h);

/* HIP-event timing on the handle's stream: begin records an event, end records another,
 * waits for it and returns the elapsed milliseconds between the two. */
int mapf_timer_begin(mapf_handle_t h);
int mapf_timer_end(mapf_handle_t h, double *out_ms);

/* The hipStream_t the handle enqueues on (for interop with other libraries). */
int mapf_get_stream(mapf_handle_t h, void **out_stream);

/* Which kernel instance took the handle's most recent mapf_step (MAPF_KERNEL_STEP), mapf_rollout
 * (MAPF_KERNEL_ROLLOUT) or mapf_transitions (MAPF_KERNEL_TRANSITIONS) launch, e.g. "lq_rollout_kernel<Q=2,RECORD,STREAM> block=512": the library chooses the
 * lane layout from A, E and the table size, so measurements label themselves with what actually ran (no reference
 * counterpart: the reference has one code path, mapf_env.py:237-266).  "" before the first launch.  The string is
 * owned by the handle and valid until its next launch of that kind. */
#define MAPF_KERNEL_STEP    0
#define MAPF_KERNEL_ROLLOUT 1
#define MAPF_KERNEL_TRANSITIONS 2   /* mapf_transitions / mapf_transitions_window */
const char *mapf_last_kernel(mapf_handle_t h, int which);

int mapf_device_count(int *out_count);
const char *mapf_last_error(void);
const char *mapf_version(void);
/* MAPF_ABI_VERSION of the loaded library: a binding written against another number must refuse to drive it (the Philox
 * counter layouts are part of the ABI: the same seed draws other numbers under another version). */
int mapf_abi_version(void);

/* Diagnostic, no device needed and none touched: which packed rollout form (agents per lane, lanes per env, table rows,
 * block size, LDS bytes) a mapf_rollout launch of this shape would take on a device with n_cu compute units -- the
 * arithmetic the launcher runs before every launch (no reference counterpart: the reference has one code path).
 * n_cells = cells of the map incl. the blocked id; streamed = actions given (1) or drawn in the kernel (0); delta_rows = the
 * map admits 4-byte delta rows (every neighbour id within +-127 of its cell); tune = a MAPF_TUNE string or NULL for the
 * defaults (the MAPF_TUNE environment variable is NOT read).
 * out[0..5] = {agents per lane K, lanes per env Q, form (0..5: how the move table lies in LDS -- the table of the six forms
 * in DESIGN.md 4.1, TableForm in csrc/mapf_layout.hpp), threads per block, LDS bytes of the table image, LDS bytes of the
 * launch}.  Returns 1 when a packed form applies, 0 when the lane-group kernel takes the launch,
 * MAPF_EINVAL (< 0) for a malformed tune string or null out. */
int mapf_debug_rollout_plan(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int streamed, int delta_rows,
                            int n_cu, const char *tune, uint64_t out[6]);
/* The same question for a handle with an episode limit of max_steps (0: exactly the call above).  With a limit no packed form
 * is consulted: returns 0 and out[0..5] = {agents per lane (2), lanes per env L, move table in LDS (0 | 1), threads per block,
 * LDS bytes of the launch, blocks} of the lane-group limit instance that takes the launch. */
int mapf_debug_rollout_plan_limited(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int streamed, int delta_rows,
                                    int n_cu, const char *tune, uint32_t max_steps, uint64_t out[6]);

/* Diagnostic, no device needed and none touched: validates a group plan for a batch of n_envs envs of n_agents agents on a map
 * of n_cells cells exactly as mapf_set_policy_group does (same return codes and mapf_last_error texts), builds the device table
 * on the host, and looks n_keys keys up through the probe function the kernel uses.  key_cells u16[n_keys * 4], key_book
 * u32[n_keys]; out_actions u32[n_keys]: the entry's four action bytes (action[0] lowest) or 0xFFFFFFFF where the book has no
 * such entry; out_probes u32[n_keys] (may be NULL): slots read; out_slots, out_max_probe (may be NULL): as
 * mapf_policy_group_stats reports them. */
int mapf_debug_policy_group(uint32_t n_cells, uint32_t n_agents, uint64_t n_envs, const uint8_t *table, uint32_t n_rows,
                            const uint16_t *row_index, const uint16_t *members, const uint32_t *book,
                            const mapf_group_entry *entries, uint64_t n_entries, const uint32_t *book_begin, uint32_t n_books,
                            uint32_t flags, uint64_t n_keys, const uint16_t *key_cells, const uint32_t *key_book,
                            uint32_t *out_actions, uint32_t *out_probes, uint64_t *out_slots, uint32_t *out_max_probe);

#ifdef __cplusplus
}
#endif
#endif /* MAPF_HIP_H */
