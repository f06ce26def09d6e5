// Packed-lane rollout kernel: K = 2, 4 or 8 agents per lane (one, two or four packed cell pairs), Q = A/K lanes per env.
//
// Why a second lane layout beside mapf_lg.hpp's: there everything that is per ENV -- flag reduction, outcome lookup,
// totals, reset handling, the hand-over steps of the probability product -- is replicated over the L = A/2 lanes of a
// group, and that part is about 40 % of a step's vector instructions at A = 8.  Four agents per lane halve the lanes
// per env, so the replicated part halves, the in-lane half of the pair tests needs no cross-lane move at all, and
// each lane carries two independent Philox calls / four independent table gathers.
//
// How the step loop is written (measured: tools/microbench/single_wave_latency.hip, profiles/r02_single_wave_costs.txt).
// At the sizes that matter only one or two waves share a SIMD, and a wave alone issues ONE instruction per ~4.6 cycles
// whatever its kind or dependences; a scalar branch costs ~12 cycles when it falls through and ~25 when taken, and a
// vector compare whose mask goes through a scalar AND/OR back into a vector select ~15 on top.  So the loop
//   * is unrolled by FOUR steps aligned to the slip stream's call blocks (two calls of two steps each, refreshed
//     together in lockstep): which word a step uses, and whether it refreshes the calls, are compile-time facts there
//     (generic steps run before / after the aligned part of a launch);
//   * derives the per-env facts with integer arithmetic in vector registers (zero-half-word tests, min / shifts)
//     and feeds selects from VCC written by the instruction before them -- no scalar mask algebra in the loop;
//   * keeps the auto-reset / terminal bookkeeping as one integer code = vertex | swap << 1 | off_goal << 2 |
//     was_terminal << 3 per env that indexes the LDS outcome table and, compared against wave-uniform constants,
//     drives every select;
//   * samples an agent's list slot with packed 16-bit arithmetic (sample_slot_packed in mapf_lq.hpp): both threshold
//     compares are one saturating v_pk_sub_i16 of bias-shifted operands, and the slot's probability address and cell
//     selector each come out of one v_dot2_i32_i16 of the sign halves -- the kernel is bound by vector-instruction issue
//     (SQ_ACTIVE_INST_VALU ~ 98 % of the SIMD's cycles at two waves per SIMD), so instructions are what is saved;
//   * owns the whole LDS image (slip rows at 0, outcome rows at 768, move table at 1024), so every LDS address is a
//     register plus an immediate offset, and stages the move table with SIX columns per cell (column 5 = STAY again):
//     an action byte is extracted and clamped by one v_min_u32 with a byte select, a table address is
//     cell * 96 + action * 16.
//
// COMPACT form for maps whose full table does not fit (64x64 maps: ~3300 free cells): the LDS table keeps only the first
// 8 bytes of each 16-byte row (the three cells and the equality code; five columns), one block per CU owns up to 158 KB
// of it, and the code's thresholds come from a second, dependent LDS read of the code's slip row.
//
// 32 agents on such maps (BASELINE configs[4]): four agents per lane, eight lanes per env, and two things that are O(A)
// instead of what the other instances do -- the vertex / swap facts through a per-env ONE-BIT occupancy bitmap in LDS behind
// the table (BITMAP, bitmap_pair_tests in mapf_lq.hpp: three LDS operations per agent instead of 496 agent pairs per env;
// behind 4-byte delta rows where the map's ids allow them, else 128 bitmaps behind a four-column table of 8-byte rows in
// 1024-thread blocks, 64 behind the five-column one in 512-thread blocks), and the
// ordered probability product as a systolic chain over the steps (SYS below: one hand-over per step and lane instead of
// seven).  DESIGN.md section 4.1 has the measurements of each step.
//
// Scope: the fused rollout of FULL groups only (A = K * Q, Q a power of two <= 16), every block full, move table in
// LDS -- the bench configurations and their neighbours.  Everything else (odd agent counts, ragged batches, tables
// beyond the LDS budget, single steps) stays with mapf_lg_rollout.hip; launch_rollout_lg() picks.  Same stream,
// same arithmetic, same outputs: the parity tests run all layouts against the oracle.
#include "mapf_lq.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>

namespace mapf {

namespace {

constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
static_assert(sizeof(SlipRow) * 8 + sizeof(OutcomeRow) * 16 <= kLdsReserve, "static LDS of the rollout kernel");

// RECORD: all five trajectory arrays are written every step; STREAM: actions come from memory, else from the
// in-kernel policy.  Memory pipeline and store scheme as lg_rollout_kernel<DENSE>.
constexpr uint32_t kSlipAt = 0, kOutcomeAt = sizeof(SlipRow) * 8, kMoveAt = kLdsReserve, kMoveCols = 6;
constexpr uint32_t kCompactCols = 5, kCompactEntry = 8;   // COMPACT: cells + code only, no sixth column
constexpr uint32_t kBitmapCols = 4;                       // COMPACT + BITMAP == 1: no STAY column either
constexpr uint32_t kDeltaEntry = 4;                       // COMPACT + BITMAP == 3: 4-byte delta rows, six columns (kDeltaCols, mapf_kernels.hpp: STAY twice, as the full table)
static_assert(kOutcomeAt + sizeof(OutcomeRow) * 16 <= kMoveAt, "LDS image: slip rows, outcome rows, then the move table");
// The LDS copy of a table row carries its slip row's byte offset PLUS kRowBias, so that sample_slot_packed's probability
// address -- that operand minus 8 per threshold not passed -- is never negative and packs into an unsigned field (the
// systolic probability chain below files four of them per word); the immediates of the LDS reads absorb the bias.
constexpr uint32_t kRowBias = kDeltaRowBias;              // (the host-built delta rows carry it too)
// index (in doubles from kSlipAt) of a +0.0: the all-equal code's list has ONE entry, so thr[1] of its row is the integer 0
constexpr uint32_t kZeroFactor = (7u * uint32_t(sizeof(SlipRow)) + uint32_t(offsetof(SlipRow, thr)) + 8u) / 8u;
static_assert(offsetof(SlipRow, thr) % 8 == 0 && kZeroFactor < 128u, "a zero factor the packed probability indices can name");

// TERM = an env may be terminal when a step begins.  With auto-reset on and no env whose START state is itself
// terminal (the handle knows: mapf_create looks) that cannot happen after the launch's first step -- a done env is back
// on its start cells -- and the !TERM instance runs every later step without the was-terminal selects.
// BITMAP = the vertex / swap facts come from a per-env LDS occupancy bitmap (bitmap_pair_tests in mapf_lq.hpp) instead of
// all agent pairs: O(A) instead of O(A^2) -- the 32-agent configurations, where 496 pairs were three quarters of a step.
// The bitmaps (one per env of the block, ceil(V / 32) words each) follow the move table in the LDS image at `bitmap_base`.
// BITMAP == 1: the table has FOUR columns (the moves; a STAY row is made up in registers) -- the form that leaves room for 128
// bitmaps, i.e. 1024-thread blocks; BITMAP == 2: five columns (STAY included: no selects per agent), 64 bitmaps, 512 threads.
// BITMAP == 3: 4-BYTE rows -- the three candidates as signed byte DELTAS against the row's own cell (a neighbour's id differs
// from a cell's by less than a column's height, which mapf_create checks: RolloutArgs::mv_delta8) plus the slip row's offset
// in the fourth byte -- so that SIX columns (STAY twice: an action byte is extracted and clamped by one v_min_u32, and no STAY
// row is made up) take half the room of the five 8-byte ones: 128 bitmaps fit behind them on the 64x64 maps.
// (the four-column form with the in-kernel policy holds its actions across the table reads -- the made-up STAY row asks for
// them -- and does not fit the 128 registers of a 1024-thread block: launched with 512 threads, see try_launch_rollout_lq)
#define MAPF_ROLLOUT_TABLE_KERNEL 0
#include "mapf_lq_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lq_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL

#undef env_id

// bytes of one env's occupancy bitmap (BITMAP instances)
static size_t bitmap_stride(uint32_t n_cells) { return (size_t((n_cells + 31u) / 32u) * 4u + 15u) & ~size_t(15); }   // one bit per cell

template <int Q, int K, bool RECORD, bool STREAM, bool COMPACT = false, int BITMAP = 0>
hipError_t launch_impl(const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream) {
    // (criteria, may-be-terminal): the instance without terminal handling exists for Makespan only
    const bool term = !(args.auto_reset && !args.start_terminal_any);
    auto kern = args.c.criteria != 0u ? lq_rollout_kernel<Q, K, RECORD, STREAM, true, COMPACT, true, BITMAP>
                : term            ? lq_rollout_kernel<Q, K, RECORD, STREAM, false, COMPACT, true, BITMAP>
                                  : lq_rollout_kernel<Q, K, RECORD, STREAM, false, COMPACT, false, BITMAP>;
    const uint32_t bitmap_base = uint32_t(lds_bytes);           // the bitmaps follow the table
    if (BITMAP) lds_bytes += size_t(block / unsigned(Q)) * bitmap_stride(args.c.n_cells);
    if (lds_bytes > 32 * 1024) {
        // (this kernel has no static LDS object: its dynamic segment may be the CU's whole 160 KB -- the limit every form's
        // "does it fit" test in try_launch_rollout_lq compares against)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    const unsigned grid = unsigned(args.n_envs / (block / unsigned(Q)));
    note_kernel("lq_rollout_kernel<Q=%d,K=%d,%s,%s,%s%s%s%s> block=%u (packed layout: %d agents per lane%s%s)", Q, K, RECORD ? "RECORD" : "TOTALS",
                STREAM ? "STREAM" : "POLICY", args.c.criteria != 0u ? "SOC" : "MAKESPAN", COMPACT ? ",COMPACT" : "",
                (args.c.criteria == 0u && !term) ? ",NO_TERMINAL" : "", (BITMAP == 2 && COMPACT) ? ",BITMAP5" : (BITMAP == 3 ? ",BITMAPD" : (BITMAP ? ",BITMAP" : "")), block, K,
                COMPACT ? (BITMAP == 3 ? ", 4-byte delta rows" : (BITMAP == 1 ? ", 8-byte table rows without the STAY column" : ", 8-byte table rows")) : "",
                BITMAP ? ", collisions through per-env occupancy bitmaps" : "");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds_bytes, stream, args, A, bitmap_base);
    return hipGetLastError();
}

#if MAPF_LQ_K != 8
// the launcher of the table instances; table_lds / table_at / lds_total: plan_rollout_lq_table's answers
template <int Q, int K, bool RECORD, bool COMPACT = false, int BITMAP = 0>
hipError_t launch_impl_table(const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream, const TablePolicy &tp, bool table_lds,
                             uint32_t table_at) {
    const bool term = !(args.auto_reset && !args.start_terminal_any);
    auto pick = [&](auto tag) {
        constexpr int T = decltype(tag)::value;
        return args.c.criteria != 0u ? lq_rollout_kernel_table<Q, K, RECORD, true, COMPACT, true, BITMAP, T>
               : term            ? lq_rollout_kernel_table<Q, K, RECORD, false, COMPACT, true, BITMAP, T>
                                 : lq_rollout_kernel_table<Q, K, RECORD, false, COMPACT, false, BITMAP, T>;
    };
    auto kern = table_lds ? pick(std::integral_constant<int, 2>{}) : pick(std::integral_constant<int, 1>{});
    const uint32_t bitmap_base = uint32_t(lds_bytes);           // the bitmaps follow the image, the policy table follows them
    if (BITMAP) lds_bytes += size_t(block / unsigned(Q)) * bitmap_stride(args.c.n_cells);
    if (table_lds) {
        if (table_at < lds_bytes || (table_at & 15u) != 0u) return hipErrorInvalidValue;
        lds_bytes = size_t(table_at) + ((size_t(tp.table_bytes) + 15u) & ~size_t(15));
    }
    if (lds_bytes > kLdsBytes || block > 512u) return hipErrorInvalidValue;
    if (lds_bytes > 32 * 1024) {
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    const unsigned grid = unsigned(args.n_envs / (block / unsigned(Q)));
    note_kernel("lq_rollout_kernel_table<Q=%d,K=%d,%s,TABLE,%s%s%s%s,%s> block=%u (packed layout: %d agents per lane%s%s; table policy: %u action bytes %s)", Q, K,
                RECORD ? "RECORD" : "TOTALS", args.c.criteria != 0u ? "SOC" : "MAKESPAN", COMPACT ? ",COMPACT" : "",
                (args.c.criteria == 0u && !term) ? ",NO_TERMINAL" : "", BITMAP == 3 ? ",BITMAPD" : "", table_lds ? "TABLE_LDS" : "TABLE_GLOBAL", block, K,
                BITMAP == 3 ? ", 4-byte delta rows" : "", BITMAP ? ", collisions through per-env occupancy bitmaps" : "", tp.table_bytes,
                table_lds ? "staged into LDS behind the image" : "gathered from global memory");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds_bytes, stream, args, A, bitmap_base, tp, table_lds ? table_at : 0u);
    return hipGetLastError();
}
#endif

}  // namespace

// This file is compiled once per (agents per lane, recording) pair -- -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0 -- so that
// its kernel instances build in parallel; each object exports one launcher, the K=4 / RECORD=1 object also the router.
#if !defined(MAPF_LQ_K) || !defined(MAPF_LQ_RECORD)
#error "compile with -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0"
#endif
#define MAPF_LQ_CAT3(a, b, c) a##b##_r##c
#define MAPF_LQ_NAME(k, r) MAPF_LQ_CAT3(launch_rollout_lq_k, k, r)

hipError_t MAPF_LQ_NAME(MAPF_LQ_K, MAPF_LQ_RECORD)(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                                   const TablePolicy *table, bool table_lds, uint32_t table_at) {
    constexpr int K = MAPF_LQ_K;
    constexpr bool R = MAPF_LQ_RECORD != 0;
    const bool stream_actions = args.actions != nullptr;
    if (table && !stream_actions) {
        // the table instances: what plan_rollout_lq_table plans, nothing else is instantiated
#if MAPF_LQ_K == 8
        return hipErrorInvalidValue;
#else
#if MAPF_LQ_K == 4
        if (form == 5 && Q == 8) return launch_impl_table<8, K, R, true, 3>(args, A, block, lds_bytes, stream, *table, table_lds, table_at);
#endif
        if (form != 0) return hipErrorInvalidValue;
        switch (Q) {
#define X(QQ) case QQ: return launch_impl_table<QQ, K, R>(args, A, block, lds_bytes, stream, *table, table_lds, table_at);
#if MAPF_LQ_K == 4
            X(1) X(2) X(4) X(8)
#else
            X(2) X(4) X(8) X(16)
#endif
#undef X
            default: return hipErrorInvalidValue;
        }
#endif
    }
    // form: 0 full table rows, 1 8-byte rows, 2 / 3 8-byte rows + occupancy bitmaps (four / five columns), 4 full rows + bitmaps,
    // 5 4-byte delta rows + bitmaps
    const bool compact = (form >= 1 && form <= 3) || form == 5, bitmap = form >= 2;
    (void)bitmap;
#if MAPF_LQ_K == 8
    // eight agents per lane: 8, 16 and 32 agents (Q = 1, 2, 4); 8-byte table rows for the 32-agent maps only
    if (compact) {
        if (Q != 4 || bitmap) return hipErrorInvalidValue;
        return stream_actions ? launch_impl<4, K, R, true, true>(args, A, block, lds_bytes, stream)
                              : launch_impl<4, K, R, false, true>(args, A, block, lds_bytes, stream);
    }
    switch (Q) {
#define X(QQ)                                                                                                        \
    case QQ: return stream_actions ? launch_impl<QQ, K, R, true>(args, A, block, lds_bytes, stream)                        \
                                   : launch_impl<QQ, K, R, false>(args, A, block, lds_bytes, stream);
        X(1) X(2) X(4)
#undef X
        default: return hipErrorInvalidValue;
    }
}
#else
#if MAPF_LQ_K == 4
    if (bitmap) {    // 32 agents only (that is where the 496 pairs dominate)
        if (Q != 8) return hipErrorInvalidValue;
        if (form == 5) return stream_actions ? launch_impl<8, K, R, true, true, 3>(args, A, block, lds_bytes, stream)
                                             : launch_impl<8, K, R, false, true, 3>(args, A, block, lds_bytes, stream);
        if (form == 4) return stream_actions ? launch_impl<8, K, R, true, false, 2>(args, A, block, lds_bytes, stream)
                                             : launch_impl<8, K, R, false, false, 2>(args, A, block, lds_bytes, stream);
        if (form == 3) return stream_actions ? launch_impl<8, K, R, true, true, 2>(args, A, block, lds_bytes, stream)
                                             : launch_impl<8, K, R, false, true, 2>(args, A, block, lds_bytes, stream);
        return stream_actions ? launch_impl<8, K, R, true, true, 1>(args, A, block, lds_bytes, stream)
                              : launch_impl<8, K, R, false, true, 1>(args, A, block, lds_bytes, stream);
    }
    if (compact) {   // instantiated for the group sizes whose maps need it: 16, 32 and 64 agents
        switch (Q) {
#define X(QQ)                                                                                                        \
    case QQ: return stream_actions ? launch_impl<QQ, K, R, true, true>(args, A, block, lds_bytes, stream)                  \
                                   : launch_impl<QQ, K, R, false, true>(args, A, block, lds_bytes, stream);
            X(4) X(8) X(16)
#undef X
            default: return hipErrorInvalidValue;
        }
    }
#else
    if (compact) return hipErrorInvalidValue;
#endif
    switch (Q) {
#define X(QQ)                                                                                                        \
    case QQ: return stream_actions ? launch_impl<QQ, K, R, true>(args, A, block, lds_bytes, stream)                        \
                                   : launch_impl<QQ, K, R, false>(args, A, block, lds_bytes, stream);
#if MAPF_LQ_K == 4
        X(1)
#endif
        X(2) X(4) X(8) X(16)
#undef X
        default: return hipErrorInvalidValue;
    }
}
#endif

#if MAPF_LQ_K == 4 && MAPF_LQ_RECORD == 1
hipError_t launch_rollout_lq_k8_r1(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                   const TablePolicy *table, bool table_lds, uint32_t table_at);
hipError_t launch_rollout_lq_k8_r0(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                   const TablePolicy *table, bool table_lds, uint32_t table_at);
hipError_t launch_rollout_lq_k4_r0(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                   const TablePolicy *table, bool table_lds, uint32_t table_at);
hipError_t launch_rollout_lq_k2_r1(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                   const TablePolicy *table, bool table_lds, uint32_t table_at);
hipError_t launch_rollout_lq_k2_r0(int Q, int form, const RolloutArgs &args, uint32_t A, unsigned block, size_t lds_bytes, hipStream_t stream,
                                   const TablePolicy *table, bool table_lds, uint32_t table_at);

// does the K-agents-per-lane form apply to this launch?  (full groups, power-of-two group size, full blocks)
static bool layout_fits(int n_agents, int K, const RolloutArgs &args, size_t lds_bytes, unsigned *block_out, int *q_out) {
    if (n_agents < K || n_agents % K != 0) return false;
    const int Q = n_agents / K;
    if (Q > 16 || (Q & (Q - 1)) != 0 || (K == 2 && Q < 2) || (K == 8 && Q > 4)) return false;
    const size_t copies = kLdsBytes / lds_bytes;   // blocks per CU by LDS
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

// the dispatch decision (see LqPlan): which packed form, block size and LDS image a launch of this shape takes
bool plan_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, const int n_cu, LqPlan *plan) {
    // top_tie: a three-entry list whose last cumulative sum rounds below 1.0 needs a third compare per agent (hi = 65535);
    // the packed sampling does two, so such a table (none arises from fail_prob / 2 splits) stays with the lane-group kernel
    if (!tune.quad_lanes || args.c.top_tie || args.n_steps > 65535u) return false;   // (per-launch counts are 16-bit)
    unsigned block = 0;
    int Q = 0, K = 0;
    bool compact = false, bitmap = false, stay_column = false, full_rows_bitmap = false, delta_rows = false;
    size_t lds_bytes = kMoveAt + size_t(args.c.n_cells) * kMoveCols * sizeof(MoveEntry);   // the kernel's whole LDS image
    if (lds_bytes <= tune.mv_lds_max_bytes && lds_bytes <= kLdsBytes - kLdsReserve) {
        // Four agents per lane halve the waves: that form needs tune.quad_min_lanes lanes (default: enough to put one
        // wave on every SIMD); below that the two-agents-per-lane form of the same kernel runs.
        // Eight agents per lane halve them again (at 8 agents nothing crosses lanes any more): worth it from two waves
        // per SIMD of THAT form on, i.e. 131072 envs at 8 agents.
        // 32 agents: four per lane with the occupancy bitmaps behind the full table (O(A) collision tests, see below) wherever that
        // form applies -- 496 agent pairs per env are most of either all-pairs form's step
        if (tune.bitmap_pairs && n_agents == 32 && (tune.force_k == 0 || tune.force_k == 4) && layout_fits(n_agents, 4, args, lds_bytes, &block, &Q) &&
            lds_bytes + (block / 8u) * bitmap_stride(args.c.n_cells) <= kLdsBytes &&
            (tune.force_k == 4 || args.n_envs * uint64_t(Q) >= tune.quad_min_lanes)) {
            K = 4;
            bitmap = true;
            full_rows_bitmap = true;
        } else
        if ((tune.force_k == 0 || tune.force_k == 8) && layout_fits(n_agents, 8, args, lds_bytes, &block, &Q) &&
            (tune.force_k == 8 || args.n_envs * uint64_t(Q) >= tune.oct_min_lanes) && block <= 512u) K = 8;
        else if (tune.force_k != 2 && tune.force_k != 8 && layout_fits(n_agents, 4, args, lds_bytes, &block, &Q) &&
                 (tune.force_k == 4 || args.n_envs * uint64_t(Q) >= tune.quad_min_lanes)) K = 4;
        else if (tune.force_k != 4 && tune.force_k != 8 && layout_fits(n_agents, 2, args, lds_bytes, &block, &Q)) K = 2;
        else return false;
    } else {
        // the full table is too large: 8-byte rows, one block per CU (512 threads = two waves per SIMD; 1024 when the
        // batch gives every CU a block of that size), four agents per lane, group sizes 4 / 8 / 16 only
        lds_bytes = kMoveAt + size_t(args.c.n_cells) * kCompactCols * kCompactEntry;
        if (tune.mv_lds_max_bytes == 0 || lds_bytes > kLdsBytes - kLdsReserve) return false;
        const size_t bitmap_lds = kMoveAt + size_t(args.c.n_cells) * kBitmapCols * kCompactEntry;   // (no STAY column in that form)
        // 32 agents: four per lane, collisions through per-env occupancy bitmaps behind the table (one bit per cell) -- O(A)
        // instead of 496 pair tests per env.  64 envs per 512-thread block; 128 per 1024-thread block (four waves per SIMD)
        // once the batch gives every CU a block of that size and 128 bitmaps fit (C5's share of one GPU: 481 G against 377 G
        // for the all-pairs form; C5 whole: profiles/r04_c5_one_bit_bitmap_ab.txt).  MAPF_TUNE k=8 / bitmap_pairs=0 keep the
        // all-pairs forms reachable (eight agents per lane, Q = 4, one 512-thread block per CU; four per lane below).
        const size_t per_env = bitmap_stride(args.c.n_cells);
        unsigned bitmap_block = 512u;
        if (tune.bitmap_block == 1024u || (tune.bitmap_block == 0u && args.n_envs * 8u >= uint64_t(n_cu) * 1024u)) bitmap_block = 1024u;
        if (bitmap_block == 1024u && (args.n_envs % (1024u / 8u) != 0 || bitmap_lds + (1024u / 8u) * per_env > kLdsBytes)) bitmap_block = 512u;
        if (args.actions == nullptr) bitmap_block = 512u;           // (in-kernel policy behind 8-byte rows: that instance is built for 512 threads)
        // ... behind 4-byte delta rows where the map's ids allow them (six columns in 79 KB on the 64x64 maps: 128 bitmaps fit, no
        // STAY row to make up, one-instruction action clamp)
        const size_t delta_lds = kMoveAt + delta_table_words(args.c.n_cells) * kDeltaEntry;   // (the host-built image, zero-padded to 16 bytes)
        unsigned delta_block = (tune.bitmap_block == 1024u || (tune.bitmap_block == 0u && args.n_envs * 8u >= uint64_t(n_cu) * 1024u)) ? 1024u : 512u;
        if (delta_block == 1024u && (args.n_envs % (1024u / 8u) != 0 || delta_lds + (1024u / 8u) * per_env > kLdsBytes)) delta_block = 512u;
        if (tune.bitmap_pairs && tune.bitmap_delta_rows && args.mv_delta8 && args.mv4 && n_agents == 32 && tune.force_k != 8 && tune.force_k != 2 &&
            layout_fits(n_agents, 4, args, delta_lds, &block, &Q) && args.n_envs % (delta_block / 8u) == 0 &&
            delta_lds + (delta_block / 8u) * per_env <= kLdsBytes) {
            block = delta_block;
            K = 4;
            bitmap = true;
            delta_rows = true;
            lds_bytes = delta_lds;
        } else
        if (tune.bitmap_pairs && n_agents == 32 && tune.force_k != 8 && tune.force_k != 2 && layout_fits(n_agents, 4, args, bitmap_lds, &block, &Q) &&
            args.n_envs % (bitmap_block / 8u) == 0 && bitmap_lds + (bitmap_block / 8u) * per_env <= kLdsBytes) {
            block = bitmap_block;
            K = 4;
            bitmap = true;
            // where the five-column table (STAY included: four selects per agent-step less) still leaves room for the block's
            // bitmaps -- 64 of them on the 64x64 maps, not 128 -- it is the one staged (C5's share: profiles/r04_c5_stay_column_ab.txt)
            stay_column = tune.bitmap_stay_column && lds_bytes + (bitmap_block / 8u) * per_env <= kLdsBytes;
            if (!stay_column) lds_bytes = bitmap_lds;
        } else if ((tune.force_k == 0 || tune.force_k == 8) && n_agents == 32 && layout_fits(n_agents, 8, args, lds_bytes, &block, &Q) &&
                   args.n_envs % (512u / 4u) == 0 && (tune.force_k == 8 || args.n_envs * 4u >= tune.oct_min_lanes)) {
            block = 512u;
            K = 8;
        } else {
            if (tune.force_k == 8 || !layout_fits(n_agents, 4, args, lds_bytes, &block, &Q) || Q < 4) return false;
            block = 512u;
            if (args.n_envs % (1024u / unsigned(Q)) == 0 && args.n_envs * uint64_t(Q) >= uint64_t(n_cu) * 1024u) block = 1024u;
            if (args.n_envs % (block / unsigned(Q)) != 0) return false;
            K = 4;
        }
        compact = true;
    }
    plan->K = K;
    plan->Q = Q;
    plan->form = delta_rows ? 5 : (full_rows_bitmap ? 4 : (bitmap ? (stay_column ? 3 : 2) : (compact ? 1 : 0)));
    plan->block = block;
    plan->lds_bytes = lds_bytes;
    plan->lds_total = lds_bytes + (bitmap ? size_t(block / unsigned(Q)) * bitmap_stride(args.c.n_cells) : 0u);   // (as launch_impl adds them)
    return true;
}

// ... under the table policy.  Which of the two table forms: the LDS copy whenever image + bitmaps + policy table fit the CU's LDS
// at the residency the launch would have without it (blocks per CU: what the image alone allows, but no more than the grid
// gives every CU); MAPF_TUNE policy_table_lds=0 never, =1 whenever one block's segment fits.  DESIGN.md has the measurements.
bool plan_rollout_lq_table(int n_agents, const RolloutArgs &args, const RolloutTuning &tune_in, const int n_cu, const size_t table_bytes, LqPlan *plan,
                           bool *table_lds, uint32_t *table_at) {
    RolloutTuning tune = tune_in;
    *table_lds = false;
    *table_at = 0u;
    if (args.actions != nullptr || tune.force_k == 8) return false;
    if (!plan_rollout_lq(n_agents, args, tune, n_cu, plan)) return false;
    if (plan->K == 8) {                                         // (no table instance with eight agents per lane: four)
        tune.force_k = 4;
        if (!plan_rollout_lq(n_agents, args, tune, n_cu, plan)) return false;
    }
    if (plan->form != 0 && plan->form != 5) return false;
    if (plan->K == 4 ? (plan->form == 5 ? plan->Q != 8 : plan->Q > 8) : (plan->K != 2 || plan->Q < 2)) return false;
    if (plan->block > 512u) {                                   // the table instances are built for 512 threads (delta rows: 64 bitmaps)
        plan->block = 512u;
        if (args.n_envs % (512u / unsigned(plan->Q)) != 0) return false;
        plan->lds_total = plan->lds_bytes + (plan->form == 5 ? size_t(512u / unsigned(plan->Q)) * bitmap_stride(args.c.n_cells) : 0u);
    }
    const size_t at16 = (plan->lds_total + 15u) & ~size_t(15), with_table = at16 + ((table_bytes + 15u) & ~size_t(15));
    const uint64_t grid = args.n_envs / (plan->block / unsigned(plan->Q));
    uint64_t resident = std::min<uint64_t>(std::min<uint64_t>(kLdsBytes / plan->lds_total, 2048u / plan->block), (grid + uint64_t(n_cu) - 1u) / uint64_t(n_cu));
    if (resident < 1u) resident = 1u;
    const bool lds = tune.policy_table_lds == 0 ? false : (tune.policy_table_lds == 1 ? with_table <= kLdsBytes : with_table * resident <= kLdsBytes);
    if (lds) {
        *table_lds = true;
        *table_at = uint32_t(at16);
        plan->lds_total = with_table;
    }
    return true;
}

// the device's CU count, asked once per device
static int device_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// true when a packed layout took the launch (*err = its status); false = not applicable, use the lane-group kernel
bool try_launch_rollout_lq(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, hipError_t *err, const TablePolicy *table) {
    LqPlan plan;
    bool table_lds = false;
    uint32_t table_at = 0u;
    if (table && args.actions) table = nullptr;
    if (table ? !plan_rollout_lq_table(n_agents, args, tune, device_cu_count(), table->table_bytes, &plan, &table_lds, &table_at)
              : !plan_rollout_lq(n_agents, args, tune, device_cu_count(), &plan)) return false;
    const bool record = args.rec_local != nullptr;
    const uint32_t A = uint32_t(n_agents);
    const int K = plan.K, Q = plan.Q, form = plan.form;
    const unsigned block = plan.block;
    const size_t lds_bytes = plan.lds_bytes;
    if (record && !(args.rec_reward && args.rec_prob && args.rec_done && args.rec_collision)) {
        *err = hipErrorInvalidValue;
        return true;
    }
#define LQ_ARGS Q, form, args, A, block, lds_bytes, stream, table, table_lds, table_at
    if (K == 8) *err = record ? launch_rollout_lq_k8_r1(LQ_ARGS) : launch_rollout_lq_k8_r0(LQ_ARGS);
    else if (K == 4) *err = record ? launch_rollout_lq_k4_r1(LQ_ARGS) : launch_rollout_lq_k4_r0(LQ_ARGS);
    else *err = record ? launch_rollout_lq_k2_r1(LQ_ARGS) : launch_rollout_lq_k2_r0(LQ_ARGS);
#undef LQ_ARGS
    return true;
}
#endif

}  // namespace mapf
