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
#include "mapf_plan.hpp"

#include <type_traits>

namespace mapf {

namespace {

// RECORD: all five trajectory arrays are written every step; STREAM: actions come from memory, else from the
// in-kernel policy.  Memory pipeline and store scheme as lg_rollout_kernel<DENSE>.
// (the LDS image -- kSlipAt, kOutcomeAt, kMoveAt, the column counts and entry sizes of each table form: mapf_layout.hpp)
// (kRowBias, kZeroFactor -- the bias of a table row's slip-row offset, the index of a zero factor: mapf_lq.hpp, shared with mapf_lq_limit.hip)

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
// them -- and does not fit the 128 registers of a 1024-thread block: launched with 512 threads, see plan_rollout_lq)
#define MAPF_ROLLOUT_TABLE_KERNEL 0
#include "mapf_lq_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lq_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL

#undef env_id

// One family of instances, launched as planned: FORM's traits (mapf_layout.hpp) give the kernel's (COMPACT, BITMAP) and what the
// kernel's name says; the plan (mapf_plan.hpp) gives the block, where the bitmaps begin (lds_bytes) and the launch's dynamic LDS segment (lds_total)
template <int Q, int K, bool RECORD, bool STREAM, TableForm FORM>
hipError_t launch_impl(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream) {
    constexpr TableFormTraits form = table_form_traits(FORM);
    constexpr bool COMPACT = form.compact; constexpr int BITMAP = form.bitmap;   // the kernel's template arguments
    // (criteria, may-be-terminal): the instance without terminal handling exists for Makespan only
    const bool term = !(args.auto_reset && !args.start_terminal_any);
    auto kern = args.c.criteria != 0u ? lq_rollout_kernel<Q, K, RECORD, STREAM, true, COMPACT, true, BITMAP>
                : term            ? lq_rollout_kernel<Q, K, RECORD, STREAM, false, COMPACT, true, BITMAP>
                                  : lq_rollout_kernel<Q, K, RECORD, STREAM, false, COMPACT, false, BITMAP>;
    if (plan.lds_total > 32 * 1024) {
        // (this kernel has no static LDS object: its dynamic segment may be the CU's whole 160 KB -- the limit every form's
        // "does it fit" test in plan_rollout_lq compares against)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    const unsigned block = plan.block, grid = unsigned(args.n_envs / (block / unsigned(Q)));
    note_kernel("lq_rollout_kernel<Q=%d,K=%d,%s,%s,%s%s%s%s> block=%u (packed layout: %d agents per lane%s%s)", Q, K, RECORD ? "RECORD" : "TOTALS",
                STREAM ? "STREAM" : "POLICY", args.c.criteria != 0u ? "SOC" : "MAKESPAN", COMPACT ? ",COMPACT" : "",
                (args.c.criteria == 0u && !term) ? ",NO_TERMINAL" : "", form.tag, block, K, form.note, BITMAP ? kBitmapNote : "");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), plan.lds_total, stream, args, A, uint32_t(plan.lds_bytes));   // (the bitmaps follow the table)
    return hipGetLastError();
}

// the launcher of the table instances (plan_rollout_lq_table's plan: the bitmaps follow the image, the policy table follows them at table_at)
template <int Q, int K, bool RECORD, TableForm FORM>
hipError_t launch_impl_table(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy &tp) {
    constexpr TableFormTraits form = table_form_traits(FORM);
    constexpr bool COMPACT = form.compact; constexpr int BITMAP = form.bitmap;
    const bool term = !(args.auto_reset && !args.start_terminal_any), table_lds = plan.table_lds;
    auto pick = [&](auto tag) {
        constexpr int T = decltype(tag)::value;
        return args.c.criteria != 0u ? lq_rollout_kernel_table<Q, K, RECORD, true, COMPACT, true, BITMAP, T>
               : term            ? lq_rollout_kernel_table<Q, K, RECORD, false, COMPACT, true, BITMAP, T>
                                 : lq_rollout_kernel_table<Q, K, RECORD, false, COMPACT, false, BITMAP, T>;
    };
    auto kern = table_lds ? pick(std::integral_constant<int, 2>{}) : pick(std::integral_constant<int, 1>{});
    const unsigned block = plan.block;
    if (plan.lds_total > kLdsBytes || block > 512u) return hipErrorInvalidValue;   // (the table instances are built for 512 threads)
    if (plan.lds_total > 32 * 1024) {
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes))) return e;
    }
    const unsigned grid = unsigned(args.n_envs / (block / unsigned(Q)));
    note_kernel("lq_rollout_kernel_table<Q=%d,K=%d,%s,TABLE,%s%s%s%s,%s> block=%u (packed layout: %d agents per lane%s%s; table policy: %u action bytes %s)", Q, K,
                RECORD ? "RECORD" : "TOTALS", args.c.criteria != 0u ? "SOC" : "MAKESPAN", COMPACT ? ",COMPACT" : "",
                (args.c.criteria == 0u && !term) ? ",NO_TERMINAL" : "", form.tag, table_lds ? "TABLE_LDS" : "TABLE_GLOBAL", block, K,
                form.note, BITMAP ? kBitmapNote : "", tp.table_bytes, table_lds ? "staged into LDS behind the image" : "gathered from global memory");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), plan.lds_total, stream, args, A, uint32_t(plan.lds_bytes), tp, plan.table_at);
    return hipGetLastError();
}

// The instances of one object -- K agents per lane, recording or not -- by the lists of mapf_layout.hpp (what lq_rollout_instance_exists
// answers from): a launch whose (Q, form) is in none of this K's lines is refused.  (A template, so that the lines of the other
// K's are discarded, not instantiated.)
template <int K, bool R>
hipError_t launch_planned(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table) {
    if (table) {
#define X(KK, QQ, FF)                                                                                                                        \
    if constexpr (KK == K) {                                                                                                                 \
        if (plan.Q == QQ && plan.form == TableForm::FF) return launch_impl_table<QQ, K, R, TableForm::FF>(plan, args, A, stream, *table);    \
    }
        MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X)
#undef X
        return hipErrorInvalidValue;
    }
#define X(KK, QQ, FF)                                                                                                                        \
    if constexpr (KK == K) {                                                                                                                 \
        if (plan.Q == QQ && plan.form == TableForm::FF) return args.actions ? launch_impl<QQ, K, R, true, TableForm::FF>(plan, args, A, stream)     \
                                                                            : launch_impl<QQ, K, R, false, TableForm::FF>(plan, args, A, stream);   \
    }
    MAPF_LQ_ROLLOUT_INSTANCES(X)
#undef X
    return hipErrorInvalidValue;
}

}  // namespace

// This file is compiled once per (agents per lane, recording) pair -- -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0 -- so that
// its kernel instances build in parallel; each object exports one launcher (prototypes: mapf_kernels.hpp; the router: mapf_dispatch.hip).
#if !defined(MAPF_LQ_K) || !defined(MAPF_LQ_RECORD)
#error "compile with -DMAPF_LQ_K=8|4|2 -DMAPF_LQ_RECORD=1|0"
#endif
#define MAPF_LQ_CAT3(a, b, c) a##b##_r##c
#define MAPF_LQ_NAME(k, r) MAPF_LQ_CAT3(launch_rollout_lq_k, k, r)

hipError_t MAPF_LQ_NAME(MAPF_LQ_K, MAPF_LQ_RECORD)(const LqPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const TablePolicy *table) {
    return launch_planned<MAPF_LQ_K, MAPF_LQ_RECORD != 0>(plan, args, A, stream, table);
}

}  // namespace mapf
