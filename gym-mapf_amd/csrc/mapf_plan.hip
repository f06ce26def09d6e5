// Launch planning (mapf_plan.hpp) -- the family that takes a launch, and its plan within each family: host-only integer arithmetic, no kernel and no runtime call.
#include "mapf_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace mapf {

// Defaults of the layout choices: a move table is staged into LDS while two blocks per CU still fit (a table that
// allows only one block per CU starves the SIMDs of waves); four agents per lane need one wave on every SIMD.
// ONE override: the environment variable MAPF_TUNE, "key=value,key=value,...", read by default_rollout_tuning (mapf_dispatch.hip) at handle creation, so a process
// can hold handles with different settings (the tests and the A/B tools do).  Keys (include/mapf_hip.h documents them):
//   quad_lanes, k, quad_min_lanes, oct_min_lanes, mv_lds_max_bytes, scen_table, bitmap_pairs, bitmap_block, bitmap_staycol,
//   bitmap_delta, step_big, step_block, step_delta, step_grid, policy_table_lds, limit_packed.
// An unknown key or a malformed item is an error (*err names it): a typo must not silently measure the default.
RolloutTuning rollout_tuning_for(int n_cu, const char *text, std::string *err) {
    RolloutTuning t;
    t.n_cu = n_cu;
    // measured on 8 agents x 32768 envs (one wave per SIMD with four agents per lane, two with two): 517 G vs 467 G
    // agent-steps/s -- fewer, fatter waves win as long as no SIMD stays empty
    t.quad_min_lanes = uint64_t(n_cu) * 4u * 64u;        // CUs x SIMDs x lanes
    t.oct_min_lanes = uint64_t(n_cu) * 4u * 64u * 2u;    // (eight agents per lane: see plan_rollout_lq)
    t.mv_lds_max_bytes = (kLdsBytes - kLdsReserve) / 2;
    if (!text) return t;
    std::string items(text);
    size_t pos = 0;
    while (pos <= items.size()) {
        size_t end = items.find(',', pos);
        if (end == std::string::npos) end = items.size();
        const std::string item = items.substr(pos, end - pos);
        pos = end + 1;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        char *rest = nullptr;
        const std::string key = item.substr(0, eq), val = eq == std::string::npos ? "" : item.substr(eq + 1);
        const unsigned long long v = val.empty() ? 0 : strtoull(val.c_str(), &rest, 10);
        if (eq == std::string::npos || val.empty() || (rest && *rest)) { if (err) *err = "MAPF_TUNE: malformed item '" + item + "' (want key=integer)"; return t; }
        if (key == "quad_lanes") t.quad_lanes = v != 0;
        else if (key == "k") t.force_k = int(v);
        else if (key == "quad_min_lanes") t.quad_min_lanes = v;
        else if (key == "oct_min_lanes") t.oct_min_lanes = v;
        else if (key == "mv_lds_max_bytes") t.mv_lds_max_bytes = size_t(v);
        else if (key == "scen_table") t.scen_table = v != 0;
        else if (key == "bitmap_pairs") t.bitmap_pairs = v != 0;
        else if (key == "bitmap_block") t.bitmap_block = unsigned(v);
        else if (key == "bitmap_staycol") t.bitmap_stay_column = v != 0;
        else if (key == "bitmap_delta") t.bitmap_delta_rows = v != 0;
        else if (key == "step_big") t.step_big = int(v);
        else if (key == "step_block") t.step_block = unsigned(v);
        else if (key == "step_delta") t.step_delta = int(v);
        else if (key == "step_grid") t.step_grid = unsigned(v);
        else if (key == "policy_table_lds") t.policy_table_lds = v != 0 ? 1 : 0;
        else if (key == "limit_packed") t.limit_packed = v != 0;
        else { if (err) *err = "MAPF_TUNE: unknown key '" + key + "'"; return t; }
    }
    return t;
}

// does the K-agents-per-lane layout apply to this launch?  (full groups, power-of-two group size, full blocks; `image`: the
// LDS image that decides how many blocks share a CU)
static bool layout_fits(int n_agents, int K, const RolloutArgs &args, size_t image, unsigned *block_out, int *q_out) {
    if (n_agents < K || n_agents % K != 0) return false;
    const int Q = n_agents / K;
    // (eight per lane exist up to Q = 4: asked HERE, so that larger teams go on to four per lane; all other existence: first_candidate)
    if (Q > 16 || (Q & (Q - 1)) != 0 || (K == 8 && Q > 4)) return false;
    const size_t copies = kLdsBytes / image;       // blocks per CU by LDS
    unsigned block = copies >= 4 ? 256u : 512u;
    // a small batch is spread over the CUs in smaller blocks (down to one wave): every block stages its own table copy,
    // which is cheap next to a rollout's steps, and an idle CU is not
    const uint64_t lanes = args.n_envs * uint64_t(Q);
    while (block > 64u && lanes < 256u * uint64_t(block)) block /= 2u;
    const uint64_t per_block = block / unsigned(Q);
    if (args.n_envs % per_block != 0 || lanes < 64 * 16) return false;
    *block_out = block;
    *q_out = Q;
    return true;
}

// One block per CU (a table that fills most of its LDS): 1024 threads -- four waves per SIMD -- once the batch gives every CU a
// block of that size and the launch fits, else 512 (two waves per SIMD).  `pinned`: MAPF_TUNE's say (0 = by batch).
static unsigned one_block_per_cu(TableForm form, int Q, const RolloutArgs &args, const RolloutTuning &tune, unsigned pinned) {
    if (Q < 1 || Q > 16) return 512u;                               // (no such layout: layout_fits refuses it)
    const bool want = pinned == 1024u || (pinned == 0u && args.n_envs * uint64_t(Q) >= uint64_t(tune.n_cu) * 1024u);
    return want && args.n_envs % (1024u / unsigned(Q)) == 0 && launch_lds_bytes(form, args.c.n_cells, 1024u, Q) <= kLdsBytes ? 1024u : 512u;
}

// One entry of the planner's ordered list: the first candidate that applies takes the launch.
struct Candidate {
    TableForm form; int K;  // the form, agents per lane
    bool admitted;          // the tuning and the launch's shape allow it
    uint64_t min_lanes;     // ... from this many lanes (n_envs * Q) on
    TableForm rule_image;   // the form whose image layout_fits looks at (its own, but for the five 8-byte columns)
    unsigned block;         // its block rule: 0 = what layout_fits picks, else this many threads
};

// the first candidate of `list` that applies: its layout fits, the batch is large enough, its block rule leaves whole blocks and
// its launch fits the CU's LDS.  What is planned must be an instance the launcher holds.
static bool first_candidate(const Candidate *list, size_t n, int n_agents, const RolloutArgs &args, LqPlan *plan) {
    for (const Candidate *c = list; c != list + n; ++c) {
        unsigned block = 0; int Q = 0;
        if (!c->admitted || !layout_fits(n_agents, c->K, args, table_image_bytes(c->rule_image, args.c.n_cells), &block, &Q) ||
            args.n_envs * uint64_t(Q) < c->min_lanes) continue;
        if (c->block) block = c->block;
        if (args.n_envs % (block / unsigned(Q)) != 0 || launch_lds_bytes(c->form, args.c.n_cells, block, Q) > kLdsBytes) continue;
        if (!lq_rollout_instance_exists(c->K, Q, c->form, false)) return false;
        *plan = LqPlan{c->K, Q, c->form, block, table_image_bytes(c->form, args.c.n_cells), launch_lds_bytes(c->form, args.c.n_cells, block, Q), false, 0u};
        return true;
    }
    return false;
}

// the dispatch decision (see LqPlan): which packed form, block size and LDS image a launch of this shape takes
bool plan_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, LqPlan *plan) {
    using F = TableForm;
    // top_tie: a three-entry list whose last cumulative sum rounds below 1.0 needs a third compare per agent (hi = 65535);
    // the packed sampling does two, so such a table (none arises from fail_prob / 2 splits) stays with the lane-group kernel
    if (!tune.quad_lanes || args.c.top_tie || args.n_steps > 65535u) return false;   // (per-launch counts are 16-bit)
    const uint32_t V = args.c.n_cells;
    const int k = tune.force_k;                                    // MAPF_TUNE k=2|4|8 pins the agents per lane
    const bool team32 = n_agents == 32, bitmaps = tune.bitmap_pairs && team32 && k != 8 && k != 2;
    const uint64_t quad_min = k == 4 ? 0u : tune.quad_min_lanes, oct_min = k == 8 ? 0u : tune.oct_min_lanes;
    const size_t full = table_image_bytes(F::FullRows, V);
    if (full <= tune.mv_lds_max_bytes && full <= kLdsBytes - kLdsReserve) {
        const Candidate list[] = {
            // 32 agents: four per lane with the occupancy bitmaps behind the full table (O(A) collision tests, see below) wherever that
            // form applies -- 496 agent pairs per env are most of either all-pairs form's step
            {F::FullRowsBitmap, 4, tune.bitmap_pairs && team32 && (k == 0 || k == 4), quad_min, F::FullRows, 0u},
            // Eight agents per lane halve the waves again (at 8 agents nothing crosses lanes any more): worth it from two waves
            // per SIMD of THAT form on, i.e. 131072 envs at 8 agents.
            {F::FullRows, 8, k == 0 || k == 8, oct_min, F::FullRows, 0u},
            // Four agents per lane halve the waves: that form needs tune.quad_min_lanes lanes (default: enough to put one
            // wave on every SIMD); below that the two-agents-per-lane form of the same kernel runs.
            {F::FullRows, 4, k != 2 && k != 8, quad_min, F::FullRows, 0u},
            {F::FullRows, 2, k != 4 && k != 8, 0u, F::FullRows, 0u},
        };
        return first_candidate(list, sizeof(list) / sizeof(list[0]), n_agents, args, plan);
    }
    // the full table is too large: 8-byte rows (or 4-byte ones), one block per CU, four agents per lane, group sizes 4 / 8 / 16 only
    if (tune.mv_lds_max_bytes == 0 || table_image_bytes(F::Rows8, V) > kLdsBytes - kLdsReserve) return false;
    // 32 agents: four per lane, collisions through per-env occupancy bitmaps behind the table (one bit per cell) -- O(A)
    // instead of 496 pair tests per env.  64 envs per 512-thread block; 128 per 1024-thread block (four waves per SIMD)
    // once the batch gives every CU a block of that size and 128 bitmaps fit (C5's share of one GPU: 481 G against 377 G
    // for the all-pairs form; C5 whole: profiles/r04_c5_one_bit_bitmap_ab.txt).  MAPF_TUNE k=8 / bitmap_pairs=0 keep the
    // all-pairs forms reachable (eight agents per lane, Q = 4, one 512-thread block per CU; four per lane below).
    // (in-kernel policy behind 8-byte rows: that instance is built for 512 threads)
    const unsigned rows8_bitmap_block = args.actions == nullptr ? 512u : one_block_per_cu(F::Rows8x4Bitmap, 8, args, tune, tune.bitmap_block);
    const Candidate list[] = {
        // ... behind 4-byte delta rows where the map's ids allow them (six columns in 79 KB on the 64x64 maps: 128 bitmaps fit, no
        // STAY row to make up, one-instruction action clamp)
        {F::DeltaRowsBitmap, 4, bitmaps && tune.bitmap_delta_rows && args.mv_delta8 && args.mv4, 0u, F::DeltaRowsBitmap,
         one_block_per_cu(F::DeltaRowsBitmap, 8, args, tune, tune.bitmap_block)},
        // where the five-column table (STAY included: four selects per agent-step less) still leaves room for the block's
        // bitmaps -- 64 of them on the 64x64 maps, not 128 -- it is the one staged (C5's share: profiles/r04_c5_stay_column_ab.txt);
        // it takes the block the four-column table would
        {F::Rows8x5Bitmap, 4, bitmaps && tune.bitmap_stay_column, 0u, F::Rows8x4Bitmap, rows8_bitmap_block},
        {F::Rows8x4Bitmap, 4, bitmaps, 0u, F::Rows8x4Bitmap, rows8_bitmap_block},
        {F::Rows8, 8, (k == 0 || k == 8) && team32, oct_min, F::Rows8, 512u},
        {F::Rows8, 4, k != 8, 0u, F::Rows8, one_block_per_cu(F::Rows8, n_agents / 4, args, tune, 0u)},
    };
    return first_candidate(list, sizeof(list) / sizeof(list[0]), n_agents, args, plan);
}

// ... under the table policy.  Which of the two table forms: the LDS copy whenever image + bitmaps + policy table fit the CU's LDS
// at the residency the launch would have without it (blocks per CU: what the image alone allows, but no more than the grid
// gives every CU); MAPF_TUNE policy_table_lds=0 never, =1 whenever one block's segment fits.  DESIGN.md has the measurements.
// (limited: the same plan names the limit instance of the same fields, lq_rollout_kernel_table_limit -- one exists for every table instance)
bool plan_rollout_lq_table(int n_agents, const RolloutArgs &args, const RolloutTuning &tune_in, const size_t table_bytes, LqPlan *plan, const bool limited) {
    RolloutTuning tune = tune_in;
    const int n_cu = tune.n_cu;
    if (args.actions != nullptr || tune.force_k == 8) return false;
    if (!plan_rollout_lq(n_agents, args, tune, plan)) return false;
    if (plan->K == 8) {                                         // (no table instance with eight agents per lane: four)
        tune.force_k = 4;
        if (!plan_rollout_lq(n_agents, args, tune, plan)) return false;
    }
    if (!lq_rollout_instance_exists(plan->K, plan->Q, plan->form, true)) return false;
    if (plan->block > 512u) {                                   // the table instances are built for 512 threads (delta rows: 64 bitmaps)
        plan->block = 512u;
        if (args.n_envs % (512u / unsigned(plan->Q)) != 0) return false;
        plan->lds_total = launch_lds_bytes(plan->form, args.c.n_cells, 512u, plan->Q);
    }
    const size_t at16 = (plan->lds_total + 15u) & ~size_t(15), with_table = at16 + ((table_bytes + 15u) & ~size_t(15));
    const uint64_t grid = args.n_envs / (plan->block / unsigned(plan->Q));
    uint64_t resident = std::min<uint64_t>(std::min<uint64_t>(kLdsBytes / plan->lds_total, 2048u / plan->block), (grid + uint64_t(n_cu) - 1u) / uint64_t(n_cu));
    if (resident < 1u) resident = 1u;
    const bool lds = tune.policy_table_lds == 0 ? false : (tune.policy_table_lds == 1 ? with_table <= kLdsBytes : with_table * resident <= kLdsBytes);
    if (lds) {
        plan->table_lds = true;
        plan->table_at = uint32_t(at16);
        plan->lds_total = with_table;
    }
    plan->limit = limited;
    return true;
}

// (the table family's two parts: behind the form's tag, and at the note's end)
void lq_rollout_kernel_name(char *name, const LqPlan &plan, bool record, bool streamed, bool table_policy, bool soc, bool may_be_terminal, uint32_t table_bytes) {
    const TableFormTraits form = table_form_traits(plan.form);
    char tag[32] = "", note[128] = "";
    if (table_policy) {
        snprintf(tag, sizeof(tag), ",%s%s", plan.table_lds ? "TABLE_LDS" : "TABLE_GLOBAL", plan.limit ? ",LIMIT" : "");
        snprintf(note, sizeof(note), "%s; table policy: %u action bytes %s", plan.limit ? "; episode step limit" : "", table_bytes,
                 plan.table_lds ? "staged into LDS behind the image" : "gathered from global memory");
    }
    snprintf(name, kKernelNameBytes, "lq_rollout_kernel%s%s<Q=%d,K=%d,%s,%s,%s%s%s%s%s> block=%u (packed layout: %d agents per lane%s%s%s)", table_policy ? "_table" : "",
             plan.limit ? "_limit" : "", plan.Q, plan.K, record ? "RECORD" : "TOTALS", table_policy ? "TABLE" : (streamed ? "STREAM" : "POLICY"), soc ? "SOC" : "MAKESPAN",
             form.compact ? ",COMPACT" : "", (!soc && !may_be_terminal) ? ",NO_TERMINAL" : "", form.tag, tag, plan.block, plan.K, form.note,
             form.bitmap ? kBitmapNote : "", note);
}

// what a step plan names must be an instance the launcher holds (MAPF_LQ_STEP_INSTANCES), as first_candidate asks for the rollouts
static bool step_instance_planned(const StepPlan &plan) { return lq_step_instance_exists(plan.K, plan.Q, plan.big); }

// The packed single step (mapf_lq_step.hip): full groups of K = 4 or 2 agents per lane (8 over the LDS table), Q = A / K lanes per
// env a power of two.  The forms are tried in this order, and a form whose divisibility test fails falls through to the next one:
// eight agents per lane over the LDS table, delta rows (with or without bitmaps), BIG, the plain step.  A form that applies but has
// no instance declines.  false = not applicable, use lg_step_kernel (*plan is then unspecified).
bool plan_step_lq(int n_agents, const StepArgs &args, const RolloutTuning &tune, StepPlan *plan) {
    // top_tie: a three-entry list whose last cumulative sum rounds below 1.0 needs a third compare per agent; the packed
    // sampling does two (as in the packed rollout), so such a table stays with the lane-group kernel
    if (!tune.quad_lanes || args.c.top_tie) return false;
    int K = 0;
    if (tune.force_k != 2 && n_agents % 4 == 0) K = 4;
    else if (tune.force_k != 4 && n_agents % 2 == 0 && n_agents >= 4) K = 2;
    else return false;
    const int Q = n_agents / K;
    if (Q > 16 || (Q & (Q - 1)) != 0) return false;
    const uint64_t lanes = args.n_envs * uint64_t(Q);
    // The BIG form (resident grid, move table in LDS): batches several times what the device holds at once
    // (profiles/r04_single_step_scaling.txt), a table that leaves room for two 1024-thread blocks per CU.
    // MAPF_TUNE step_big=0 never, =2 whenever it fits.
    const size_t big_lds = kStepMoveAt + size_t(args.c.n_cells) * kBigCols * sizeof(MoveEntry);
    const int n_cu = tune.n_cu;
    // MAPF_TUNE step_grid=n: at most n blocks in a resident form's grid (the kernel strides by its grid: a block then walks more
    // chunks than any batch a test can afford gives it on a whole device); 0 = the grid below
    auto capped = [&tune](unsigned grid) { return tune.step_grid != 0u && tune.step_grid < grid ? tune.step_grid : grid; };
    const uint64_t resident_lanes = uint64_t(n_cu) * 2048u;
    const bool big_fits = K == 4 && Q <= 8 && tune.step_big != 0 && args.n_envs > 0 && args.n_envs % (1024u / unsigned(Q)) == 0 &&
                          2u * big_lds <= kLdsBytes;
    const bool big = big_fits && (tune.step_big == 2 || lanes >= 4u * resident_lanes);
    // ... with EIGHT agents per lane where the team allows it (8, 16, 32 agents): the large-batch step is bound by its vector
    // instructions once the gathers are gone, and what a lane does once per env (lane context, flags, outcome row, stores,
    // the hand-over of the probability product) is then paid for 64 envs per wave instead of 32
    // (measured, 8 agents: 0.289 against 0.262 at 0.5 M envs, 0.35 / 0.41 / 0.42 at 1 / 2 / 4 M -- this form from TWICE the
    // device's resident lanes on, the four-agents-per-lane form below from four times)
    if (big_fits && (tune.step_big == 2 || lanes >= 2u * resident_lanes) && Q >= 2 && args.n_envs % (1024u / unsigned(Q / 2)) == 0 &&
        tune.force_k != 4) {
        const int Q8 = Q / 2;
        const unsigned block = 1024u, n_chunks = unsigned(args.n_envs * uint64_t(Q8) / block), grid = capped(n_chunks < unsigned(n_cu) ? n_chunks : unsigned(n_cu));
        *plan = StepPlan{8, Q8, StepForm::FullRows, block, grid, n_chunks, big_lds, int(kLdsBytes - kLdsReserve)};
        return step_instance_planned(*plan);
    }
    // The delta-row forms (StepForm::DeltaRows, DeltaRowsBitmap): where the 16-byte rows do not fit (64x64 maps) but the 4-byte ones do, from a batch of one
    // full residency on (65536 envs of 32 agents) -- below that the table copy per block (79 KB through the XCD's L2 for each of
    // its 32 CUs: 1.8 us in front of the first instruction that needs a row, profiles/r05_step_stamps_c5_share.txt) costs more
    // than the gathers it replaces: configs[4]'s share of one GPU (16384 envs) runs 4.95 us plain against 5.7-5.9 us.
    const size_t delta_lds = kStepMoveAt + delta_table_words(args.c.n_cells) * sizeof(uint32_t);
    if (K == 4 && Q <= 8 && args.mv4 && tune.step_delta != 0 && delta_lds <= kLdsBytes && args.n_envs > 0 &&
        (tune.step_delta == 2 || (!big_fits && lanes >= resident_lanes))) {
        // 32 agents: the occupancy bitmaps of a chunk's envs behind the table -- one block per CU then, so 1024 threads as soon as
        // every CU gets such a block (measured on configs[4]'s map, profiles/r05_step32_forms.txt: 131072 envs 15.6 us with
        // bitmaps in 1024-thread blocks, 18.0 without, 21.5 for the plain step; at 65536 envs 512-thread blocks with bitmaps
        // 11.7, without 10.8, plain 11.9)
        const size_t per_env = bitmap_stride(args.c.n_cells);
        const bool bitmaps_1024 = Q == 8 && tune.bitmap_pairs && delta_lds + (1024u / 8u) * per_env <= kLdsBytes && args.n_envs % (1024u / 8u) == 0 &&
                                  lanes >= uint64_t(n_cu) * 1024u;
        unsigned block = (bitmaps_1024 || lanes >= 2u * resident_lanes) ? 1024u : 512u;
        if (args.n_envs % (block / unsigned(Q)) != 0) block = 512u;
        bool bitmaps = Q == 8 && tune.bitmap_pairs && delta_lds + (block / 8u) * per_env <= kLdsBytes;
        if (!bitmaps && Q == 8 && tune.bitmap_pairs && block == 1024u && delta_lds + (512u / 8u) * per_env <= kLdsBytes) { block = 512u; bitmaps = true; }
        const size_t form_lds = delta_lds + (bitmaps ? (block / 8u) * per_env : 0u);
        if (args.n_envs % (block / unsigned(Q)) == 0) {
            unsigned per_cu = unsigned(kLdsBytes / form_lds);
            if (per_cu > 2048u / block) per_cu = 2048u / block;
            const unsigned n_chunks = unsigned(lanes / block), grid = capped(n_chunks < per_cu * unsigned(n_cu) ? n_chunks : per_cu * unsigned(n_cu));
            *plan = StepPlan{K, Q, bitmaps ? StepForm::DeltaRowsBitmap : StepForm::DeltaRows, block, grid, n_chunks, form_lds, int(kLdsBytes)};
            return step_instance_planned(*plan);
        }
    }
    if (big) {
        const unsigned block = 1024u, n_chunks = unsigned(lanes / block), grid = capped(n_chunks < 2u * unsigned(n_cu) ? n_chunks : 2u * unsigned(n_cu));
        *plan = StepPlan{K, Q, StepForm::FullRows, block, grid, n_chunks, big_lds, int(kLdsBytes - kLdsReserve)};
        return step_instance_planned(*plan);
    }
    unsigned block = 256u;
    while (block > 64u && lanes < 256u * uint64_t(block)) block /= 2u;   // small batches: spread over the CUs
    // from two 256-thread blocks per CU on, four 128-thread blocks measure 3 % faster (65536 and 131072 envs of 8 agents: 3.22
    // against 3.33 us, 4.45 against 4.60; equal at 262144; at ONE block per CU -- 32768 envs -- 256 threads are 1 % ahead)
    if (lanes >= 512u * 256u) block = 128u;
    if (tune.step_block == 64u || tune.step_block == 128u || tune.step_block == 256u || tune.step_block == 512u) block = tune.step_block;
    const uint64_t per_block = block / unsigned(Q);
    if (args.n_envs == 0 || args.n_envs % per_block != 0) return false;
    const unsigned grid = unsigned(args.n_envs / per_block);
    *plan = StepPlan{K, Q, StepForm::Plain, block, grid, grid, 0, 0};
    return step_instance_planned(*plan);
}

// (the tags in the kernel's argument order, the form's notes in front of the scenario table's)
void lq_step_kernel_name(char *name, const StepPlan &plan, bool scen, bool may_be_terminal) {
    const StepFormTraits form = step_form_traits(plan.big);
    snprintf(name, kKernelNameBytes, "lq_step_kernel<Q=%d,K=%d%s%s%s> block=%u%s (packed layout: %d agents per lane%s%s%s)", plan.Q, plan.K, scen ? ",SCEN" : "",
             may_be_terminal ? "" : ",NO_TERMINAL", form.tag, plan.block, form.resident ? " resident grid" : "", plan.K, form.note,
             form.bitmap ? kBitmapNote : "", scen ? ", start / goal rows from the scenario table" : "");
}

// ------------------------------------------------------------------- the lane-group family
int lg_group_size(int n_agents) {
    int pairs = (n_agents + 1) / 2, L = 1;
    while (L < pairs) L <<= 1;
    return L;
}

// the geometry of a launch without a table in LDS (the single step; the rollout over a table in global memory)
static void lg_geometry(int L, uint64_t n_envs, unsigned &grid, unsigned &block) {
    const uint64_t threads = n_envs * uint64_t(L);
    // one-wave blocks keep >= ~2 blocks per CU at small sizes; from two waves per SIMD upward four-wave blocks launch
    // faster (measured at 65536 envs x 8 agents: 5.29 us per step instead of 5.67)
    block = threads < (uint64_t(1) << 17) ? 64u : 256u;
    const uint64_t per_block = block / unsigned(L);
    grid = unsigned((n_envs + per_block - 1) / per_block);
}

// MV_LDS: the move table goes to LDS while the tuning's limit (default: two blocks per CU) and the CU's LDS hold it beside the
// 1 KB table image, from 256 waves on.  DENSE: full groups and no ragged last block.
LgRolloutPlan plan_rollout_lg(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, bool limited) {
    LgRolloutPlan plan;
    plan.L = lg_group_size(n_agents);
    plan.full = n_agents == 2 * plan.L;
    plan.limit = limited;
    const size_t mv_bytes = size_t(args.c.n_cells) * kMvCols * sizeof(MoveEntry);
    const uint64_t threads = args.n_envs * uint64_t(plan.L);
    plan.mv_lds = mv_bytes + kLdsReserve <= tune.mv_lds_max_bytes && mv_bytes + kLdsReserve <= kLdsBytes && threads >= 64 * 256;
    if (plan.mv_lds) {
        // block size: as many waves as can share one table copy while >= 16 waves stay resident per CU
        const size_t copies = (kLdsBytes - kLdsReserve) / (mv_bytes + sizeof(SlipRow) * 8);   // blocks per CU by LDS
        const unsigned cap = plan.L == 16 ? kLgRolloutMaxBlock16 : kLgRolloutMaxBlock;
        plan.block = std::min(copies >= 4 ? 256u : (copies >= 2 ? 512u : 1024u), cap);
        const uint64_t per_block = plan.block / unsigned(plan.L);
        plan.grid = unsigned((args.n_envs + per_block - 1) / per_block);
        plan.lds_bytes = mv_bytes;
    } else {
        lg_geometry(plan.L, args.n_envs, plan.grid, plan.block);
    }
    plan.dense = !limited && plan.full && args.n_envs % (plan.block / unsigned(plan.L)) == 0;   // (the limit instances: guarded only)
    return plan;
}

LgStepPlan plan_step_lg(int n_agents, const StepArgs &args, bool limited) {
    LgStepPlan plan;
    plan.L = lg_group_size(n_agents);
    plan.full = n_agents == 2 * plan.L;
    plan.limit = limited;
    lg_geometry(plan.L, args.n_envs, plan.grid, plan.block);
    return plan;
}

// (a limit plan: _limit_guarded and LIMIT where the others say DENSE or GUARDED, and the note; a budget plan: _budget_guarded, BUDGET;
// a budget plan that keeps an episode log: _budget_guarded_log, BUDGET,LOG)
void lg_rollout_kernel_name(char *name, const LgRolloutPlan &plan, bool record, bool streamed, bool table_policy) {
    const bool log = plan.log && plan.budget;
    const char *family = plan.budget ? (log ? "_budget_guarded_log" : "_budget_guarded") : (plan.limit ? "_limit_guarded" : "");
    const char *form = plan.budget ? (log ? "BUDGET,LOG" : "BUDGET") : (plan.limit ? "LIMIT" : (plan.dense ? "DENSE" : "GUARDED"));
    const char *note = plan.budget ? (log ? "; episode budget; episode log" : "; episode budget") : (plan.limit ? "; episode step limit" : "");
    const bool joint = plan.joint && table_policy;   // (the joint launcher passes table_policy: a launch without streamed actions)
    if (plan.group && table_policy) {                // (the group launcher likewise)
        snprintf(name, kKernelNameBytes, "lg_rollout_kernel_group%s%s<L=%d,%s,%s,%s,GROUP,%s%s> block=%u (pair layout: 2 agents per lane%s%s; group policy: books probed in global memory)",
                 family, plan.pairs ? "_pairs" : "", plan.L, plan.full ? "FULL" : "RAGGED", plan.mv_lds ? "MV_LDS" : "MV_GLOBAL", record ? "RECORD" : "TOTALS", form,
                 plan.pairs ? ",PAIRS" : "", plan.block, note, plan.pairs ? "; conflict matrix" : "");
        return;
    }
    snprintf(name, kKernelNameBytes, "lg_rollout_kernel%s%s%s<L=%d,%s,%s,%s,%s,%s%s> block=%u (pair layout: 2 agents per lane%s%s%s)", joint ? "_joint" : (table_policy ? "_table" : ""),
             family, plan.pairs ? "_pairs" : "", plan.L, plan.full ? "FULL" : "RAGGED", plan.mv_lds ? "MV_LDS" : "MV_GLOBAL", record ? "RECORD" : "TOTALS",
             joint ? "JOINT" : (table_policy ? "TABLE" : (streamed ? "STREAM" : "POLICY")), form, plan.pairs ? ",PAIRS" : "", plan.block, note, plan.pairs ? "; conflict matrix" : "",
             joint ? "; joint policy: action bytes gathered from global memory" : (table_policy ? "; table policy: action bytes gathered from global memory" : ""));
}

void lg_step_kernel_name(char *name, const LgStepPlan &plan, bool ext_uniforms) {
    snprintf(name, kKernelNameBytes, "lg_step_kernel%s<L=%d,%s,%s%s> block=%u (pair layout: 2 agents per lane%s)", plan.limit ? "_limit" : "", plan.L,
             plan.full ? "FULL" : "RAGGED", ext_uniforms ? "EXT_UNIFORMS" : "PHILOX", plan.limit ? ",LIMIT" : "", plan.block,
             plan.limit ? "; episode step limit" : "");
}

// ------------------------------------------------------------------- the thread-per-env family
TpePlan plan_tpe(uint64_t n_envs) {
    TpePlan plan;
    plan.block = n_envs <= (1u << 18) ? 64u : 256u;
    plan.grid = unsigned((n_envs + plan.block - 1) / plan.block);
    return plan;
}

void tpe_step_kernel_name(char *name, int n_agents, const TpePlan &plan, bool ext_uniforms) {
    snprintf(name, kKernelNameBytes, "step_kernel<A=%d,%s> block=%u (thread per env)", n_agents, ext_uniforms ? "EXT_UNIFORMS" : "PHILOX", plan.block);
}

void tpe_rollout_kernel_name(char *name, int n_agents, const TpePlan &plan, bool table_policy) {
    if (table_policy) snprintf(name, kKernelNameBytes, "rollout_kernel_table<A=%d,TABLE> block=%u (thread per env, table policy: action bytes gathered from global memory)", n_agents, plan.block);
    else snprintf(name, kKernelNameBytes, "rollout_kernel<A=%d> block=%u (thread per env)", n_agents, plan.block);
}

// ------------------------------------------------------------------- env.P[s][a]
// the rows family (transitions_rows_kernel<max_a>): queries per wave, pieces, the scan it needs, waves per block
static bool plan_transitions_rows(uint32_t n_agents, uint64_t n_queries, uint32_t max_branches, bool compact, TransitionsPlan *plan) {
    const int max_a = plan->max_a;
    const bool coop = transitions_cooperative(max_a);
    // queries per wave: as many as keep a block's LDS near 32 KB (five or more blocks per CU), fewer while that leaves the
    // device short of waves (16 per SIMD queued) -- set-up uses one lane per query, so small teams want many per wave
    uint32_t qw_log2 = 6;
    while (qw_log2 > 2 && 4u * (transitions_records_bytes(max_a) + 4u) * (1u << qw_log2) > 36u * 1024u) --qw_log2;
    while (qw_log2 > (max_a >= 8 ? 2u : 3u) && (n_queries >> qw_log2) < 16384u) --qw_log2;
    if (coop && qw_log2 > 3u) qw_log2 = 3u;                          // (cooperative set-up: a query's group has a lane per agent)
    // rows per wave: a batch's windows can hold QW x min(3^A, max_branches) rows; beyond two pieces' worth they are cut into
    // pieces -- which needs the scan, as compacted rows do.  Pieces of 1024 rows (16 sweeps) while the call is small, so that it
    // still makes ~24 K waves' worth of work (a room map fills about a fifth of the rows a query can have), up to 4096 for large
    // calls, where fewer set-ups per row count (profiles/r05_transitions_launch_shapes.txt: 20000 queries of 8 agents 0.43 of the
    // roofline with 1024-row pieces, 0.37 with 4096; 200000 queries 0.54 against 0.60-0.68)
    uint64_t most = 1;
    for (uint32_t i = 0; i < n_agents && most < max_branches; ++i) most *= 3u;
    if (most > max_branches) most = max_branches;
    const uint64_t est_rows = n_queries * most / 5u;
    uint32_t rows_per_wave = 1024u;
    while (rows_per_wave < 4096u && est_rows / (2u * rows_per_wave) >= 24576u) rows_per_wave *= 2u;
    most <<= qw_log2;
    // (the small teams' batches -- at most 64 x 81 rows, set up by one lane per query -- stay whole: their waves all do the same work)
    const uint32_t pieces_max = (coop && most > 2u * rows_per_wave) ? uint32_t((most + rows_per_wave - 1) / rows_per_wave) : 1u;
    // the scan: pass 2 is left to the rows kernel's waves (unscanned_blocks != 0) in a call of at most kFusedScanBlocks scan blocks
    const uint64_t scan_blocks = transitions_scan_blocks(n_queries);
    const uint32_t unscanned_blocks = scan_blocks <= kFusedScanBlocks ? uint32_t(scan_blocks) : 0u;
    if (compact || pieces_max > 1u) {
        if (scan_blocks > 0x7FFFFFFFull) return false;
        plan->scan_passes = unscanned_blocks == 0u ? 2 : 1;
        plan->scan_blocks = unsigned(scan_blocks);
    }
    const uint64_t waves = ((n_queries + (1u << qw_log2) - 1) >> qw_log2) * pieces_max;
    // waves per block: ONE for the large teams -- their waves live for very different times (a piece that does not exist leaves
    // at once, a full one sweeps 64 times) and a block keeps its place until its last wave is done: four waves per block
    // measured 0.407 ms against 0.277 ms at 8 agents x 20000 queries (profiles/r05_transitions_launch_shapes.txt); the small
    // teams' waves all do the same work and share a block's slip table
    const unsigned wpb = coop ? 1u : 4u;
    const uint64_t grid64 = (waves + wpb - 1) / wpb;
    if (grid64 > 0x7FFFFFFFull) return false;
    plan->qw_log2 = qw_log2; plan->pieces_max = pieces_max; plan->rows_per_wave = rows_per_wave; plan->unscanned_blocks = unscanned_blocks;
    plan->block = 64u * wpb;
    plan->grid = unsigned(grid64);
    plan->lds_bytes = wpb * transitions_wave_lds_bytes(max_a, qw_log2);
    return true;
}

bool plan_transitions(uint32_t n_agents, uint64_t n_queries, uint32_t max_branches, bool compact, bool all_out, TransitionsPlan *plan) {
    *plan = TransitionsPlan{};
    if (n_agents <= 8u) {
        plan->max_a = n_agents <= 2u ? 2 : (n_agents <= 4u ? 4 : (n_agents <= 6u ? 6 : 8));
        plan->all_out = all_out;
        return plan_transitions_rows(n_agents, n_queries, max_branches, compact, plan);
    }
    if (n_agents > uint32_t(kTransitionsMaxAgents)) return false;
    plan->wide = true;
    plan->max_a = int(n_agents);
    if (compact) {   // (the wide kernels read the scanned totals: both passes)
        const uint64_t scan_blocks = transitions_scan_blocks(n_queries);
        if (scan_blocks > 0x7FFFFFFFull) return false;
        plan->scan_passes = 2;
        plan->scan_blocks = unsigned(scan_blocks);
    }
    // lanes per group: a wave; a group walks up to 16 x lanes rows, a long window is cut into that many-row chunks (so
    // that a single query of a large team still fills the device)
    while (plan->lanes_log2 < 6 && (1u << plan->lanes_log2) < max_branches) ++plan->lanes_log2;
    const uint32_t lanes = 1u << plan->lanes_log2;
    plan->walks = std::min<uint32_t>(16u, (max_branches + lanes - 1) / lanes);
    plan->chunk = lanes * plan->walks;
    plan->chunks_per_query = (max_branches + plan->chunk - 1) / plan->chunk;
    const uint64_t threads = n_queries * uint64_t(plan->chunks_per_query) * lanes;
    const uint64_t grid64 = (threads + 255) / 256;
    if (grid64 > 0x7FFFFFFFull) return false;
    plan->block = 256u;
    plan->grid = unsigned(grid64);
    return true;
}

void transitions_kernel_name(char *name, const TransitionsPlan &plan, uint32_t n_agents, bool compact) {
    const char *rows = compact ? "compacted" : "reserved";
    char pieces[40] = "";
    if (plan.wide) {
        snprintf(name, kKernelNameBytes, "transitions_kernel<%d,EXACT> %u agents, %u lanes x %u rows per group, %u groups per query, %s rows", plan.max_a, n_agents,
                 1u << plan.lanes_log2, plan.walks, plan.chunks_per_query, rows);
        return;
    }
    if (plan.pieces_max > 1u) snprintf(pieces, sizeof(pieces), " in pieces of %u rows", plan.rows_per_wave);
    snprintf(name, kKernelNameBytes, "transitions_rows_kernel<%d> %u agents, %u queries per wave%s, %s rows", plan.max_a, n_agents, 1u << plan.qw_log2, pieces, rows);
}

// ------------------------------------------------------------------- the route (mapf_plan.hpp lists the rules)
// thread-per-env is what the handle prefers: by flag, or an env of at most one agent pair (lane groups from two pairs on)
static bool prefers_tpe(FamilyPreference prefer, int n_agents) {
    return prefer == FamilyPreference::ThreadPerEnv || (prefer == FamilyPreference::Auto && n_agents <= 2);
}

RolloutRoute route_rollout(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, FamilyPreference prefer, bool table_policy, size_t table_bytes,
                           bool limited, bool budgeted, bool pairs, bool joint, bool logged, bool group) {
    RolloutRoute r;
    logged = logged && budgeted;   // (a log launch is a budget launch: one of the three branches below, whose plan takes the mark)
    RolloutTuning with_log = tune;   // (kLogLdsBytes of static LDS more than the others, as the matrix has: the largest tables stay in global memory)
    if (logged) with_log.mv_lds_max_bytes = std::min(tune.mv_lds_max_bytes, kLdsBytes - kPairsLdsBytes - kLogLdsBytes);
    if (joint || group) {   // the joint and the group instances exist in the lane-group family only, guarded, one form per (limit, budget, pairs)
        RolloutTuning t = logged ? with_log : tune;   // (with the matrix: its block's static LDS, as below)
        if (pairs) t.mv_lds_max_bytes = std::min(t.mv_lds_max_bytes, kLdsBytes - kPairsLdsBytes);
        // (a group instance: kGroupLdsBytes more again, beside the matrix's and the log's)
        if (group && !joint) t.mv_lds_max_bytes = std::min(t.mv_lds_max_bytes, kLdsBytes - kPairsLdsBytes - kLogLdsBytes - kGroupLdsBytes);
        r.lg = plan_rollout_lg(n_agents, args, t, limited || budgeted);
        r.lg.budget = budgeted;
        r.lg.pairs = pairs;
        r.lg.log = logged;
        r.lg.dense = false;
        r.lg.joint = joint;
        r.lg.group = group && !joint;   // (one policy per launch: the dispatcher refuses both)
        return r;
    }
    if (pairs) {   // the instances that count exist in the lane-group family only, guarded, one form per (limit, budget)
        RolloutTuning t = logged ? with_log : tune;   // (kPairsLdsBytes of static LDS more than the others: the largest tables stay in global memory)
        t.mv_lds_max_bytes = std::min(t.mv_lds_max_bytes, kLdsBytes - kPairsLdsBytes);
        r.lg = plan_rollout_lg(n_agents, args, t, limited || budgeted);
        r.lg.budget = budgeted;
        r.lg.dense = false;
        r.lg.pairs = true;
        r.lg.log = logged;
        return r;
    }
    if (budgeted) {   // the budget instances exist in the lane-group family only -- no packed plan, whatever the tuning says
        r.lg = plan_rollout_lg(n_agents, args, logged ? with_log : tune, true);
        r.lg.budget = true;
        r.lg.log = logged;
        return r;
    }
    // (the thread-per-env rollout specialisations beyond kTpeRolloutMaxAgents need SGPR spills and are not dispatched)
    if (!limited && prefers_tpe(prefer, n_agents) && n_agents <= kTpeRolloutMaxAgents) {
        r.family = KernelFamily::ThreadPerEnv;
        r.tpe = plan_tpe(args.n_envs);
        return r;
    }
    // under a limit the packed instances are the table policy's (mapf_lq_limit.hip), opted into by MAPF_TUNE limit_packed=1
    const bool packed_allowed = !limited || (table_policy && args.actions == nullptr && tune.limit_packed && prefer != FamilyPreference::LaneGroup);
    if (packed_allowed && (table_policy ? plan_rollout_lq_table(n_agents, args, tune, table_bytes, &r.lq, limited) : plan_rollout_lq(n_agents, args, tune, &r.lq))) {
        r.family = KernelFamily::Packed;
        return r;
    }
    r.lq = LqPlan{};
    r.lg = plan_rollout_lg(n_agents, args, tune, limited);
    return r;
}

StepRoute route_step(int n_agents, const StepArgs &args, const RolloutTuning &tune, FamilyPreference prefer, bool limited, bool ext_uniforms) {
    StepRoute r;
    if (limited) {   // the step's limit instances exist in the lane-group family only
        r.lg = plan_step_lg(n_agents, args, true);
        return r;
    }
    if (prefers_tpe(prefer, n_agents) && n_agents <= kTpeMaxAgents) {
        r.family = KernelFamily::ThreadPerEnv;
        r.tpe = plan_tpe(args.n_envs);
        return r;
    }
    if (!ext_uniforms && plan_step_lq(n_agents, args, tune, &r.lq)) {
        r.family = KernelFamily::Packed;
        return r;
    }
    r.lq = StepPlan{};
    r.lg = plan_step_lg(n_agents, args);
    return r;
}

}  // namespace mapf
