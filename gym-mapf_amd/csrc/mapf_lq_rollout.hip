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
// beyond the LDS budget, single steps) stays with mapf_lg_rollout.hip; route_rollout (mapf_plan.hip) picks.  Same stream,
// same arithmetic, same outputs: the parity tests run all layouts against the oracle.
#include "mapf_lq_launch.hpp"
#include "mapf_lq_rollout_kernel.hpp"

namespace mapf {

namespace {

// RECORD: all five trajectory arrays are written every step; STREAM: actions come from memory, else from the
// in-kernel policy.  Memory pipeline and store scheme as lg_rollout_kernel<DENSE>.
// (the LDS image -- kSlipAt, kOutcomeAt, kMoveAt, the column counts and entry sizes of each table form: mapf_layout.hpp)
// (kRowBias, kZeroFactor -- the bias of a table row's slip-row offset, the index of a zero factor: mapf_lq.hpp, shared with mapf_lq_limit.hip)
// (the launcher: mapf_lq_launch.hpp, shared with mapf_lq_limit.hip too)

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
// (The kernel: mapf_lq_rollout_kernel.hpp.)

// The instances of lq_rollout_kernel without an episode limit: the plain ones (streamed actions, the in-kernel policies: TABLE is 0
// whatever the launcher asks for) and those that follow the table policy (its block and where its LDS copy begins as arguments)
struct LqFamily {
    static constexpr bool kTable = false, kLimit = false;
    template <int Q, int K, bool RECORD, bool STREAM, bool SOC, bool COMPACT, bool TERM, int BITMAP, int TABLE>
    static auto kernel() { return lq_rollout_kernel<Q, K, RECORD, STREAM, SOC, COMPACT, TERM, BITMAP, 0>; }
};
struct LqTableFamily {
    static constexpr bool kTable = true, kLimit = false;
    template <int Q, int K, bool RECORD, bool STREAM, bool SOC, bool COMPACT, bool TERM, int BITMAP, int TABLE>
    static auto kernel() { return lq_rollout_kernel<Q, K, RECORD, false, SOC, COMPACT, TERM, BITMAP, TABLE, TablePolicy, uint32_t>; }
};

}  // namespace

// (table: the table policy, or null; this object has no limit instances)
MAPF_LQ_LAUNCHER(launch_rollout_lq_k) {
    if (limit) return hipErrorInvalidValue;
    return table ? launch_lq_rollout<LqTableFamily, kLqK, kLqRecord>(plan, args, A, stream, table)
                 : launch_lq_rollout<LqFamily, kLqK, kLqRecord>(plan, args, A, stream, table);
}

}  // namespace mapf
