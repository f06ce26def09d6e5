// LDS layout of the kernels that keep the move table in LDS: ONE definition for the kernels (mapf_lg_rollout.hip,
// mapf_lq_rollout.hip, mapf_lq_step.hip) and for the launch planner (mapf_plan.hip), which decides whether an image fits.
// Also the forms of the packed kernels and the lists of their instances (MAPF_LQ_ROLLOUT_INSTANCES, ..._TABLE_INSTANCES,
// MAPF_LQ_STEP_INSTANCES): the planner asks them, the launchers are generated from them.  At the end, a wave's LDS in the env.P
// rows kernel (mapf_transitions.hip), for that kernel and for plan_transitions.
#pragma once
#include "mapf_kernels.hpp"

#include <cstddef>

namespace mapf {

// The CU has 160 KiB of LDS; the first 1 KB of every image is the table image (slip rows, then outcome rows)
constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
static_assert(sizeof(SlipRow) * 8 + sizeof(OutcomeRow) * 16 <= kLdsReserve, "static LDS of the rollout kernel");

// packed rollout (mapf_lq_rollout.hip): slip rows at 0, outcome rows behind them, move table at 1024 with SIX columns per cell
constexpr uint32_t kSlipAt = 0, kOutcomeAt = sizeof(SlipRow) * 8, kMoveAt = kLdsReserve, kMoveCols = 6;
constexpr uint32_t kCompactCols = 5, kCompactEntry = 8;   // 8-byte rows: cells + code only, no sixth column
constexpr uint32_t kBitmapCols = 4;                       // ... in front of 128 bitmaps: no STAY column either
constexpr uint32_t kDeltaEntry = 4;                       // 4-byte delta rows, six columns (kDeltaCols, mapf_kernels.hpp: STAY twice, as the full table)
static_assert(kOutcomeAt + sizeof(OutcomeRow) * 16 <= kMoveAt, "LDS image: slip rows, outcome rows, then the move table");

// packed single step, LDS-table forms (mapf_lq_step.hip BIG): the same image, the table at the same place
#ifndef MAPF_BIG_COLS
#define MAPF_BIG_COLS 6
#endif
constexpr uint32_t kStepMoveAt = kMoveAt, kBigCols = MAPF_BIG_COLS;

// bytes of one env's occupancy bitmap (BITMAP instances): one bit per cell, padded to 16 bytes
constexpr size_t bitmap_stride(uint32_t n_cells) { return (size_t((n_cells + 31u) / 32u) * 4u + 15u) & ~size_t(15); }

// The six forms in which the packed rollout keeps the move table in LDS -- ONE description for the planner, the launcher and the
// kernels (DESIGN.md 4.1 has the table).  The values are the ABI's `form` numbers (mapf_debug_rollout_plan's out[2]).
enum class TableForm : int { FullRows = 0, Rows8 = 1, Rows8x4Bitmap = 2, Rows8x5Bitmap = 3, FullRowsBitmap = 4, DeltaRowsBitmap = 5 };
constexpr int kTableForms = 6;
struct TableFormTraits {
    bool compact; int bitmap;        // the kernel's (COMPACT, BITMAP) template arguments (BITMAP != 0: per-env occupancy bitmaps follow the table)
    uint32_t cols, entry_bytes;      // columns per cell, bytes per entry
    const char *tag, *note;          // what the kernel's name (mapf_last_kernel) says about the form: the tag among its arguments, the note in its parentheses
};
constexpr TableFormTraits table_form_traits(TableForm form) {
    switch (form) {
        case TableForm::Rows8:           return {true, 0, kCompactCols, kCompactEntry, "", ", 8-byte table rows"};
        case TableForm::Rows8x4Bitmap:   return {true, 1, kBitmapCols, kCompactEntry, ",BITMAP", ", 8-byte table rows without the STAY column"};
        case TableForm::Rows8x5Bitmap:   return {true, 2, kCompactCols, kCompactEntry, ",BITMAP5", ", 8-byte table rows"};
        case TableForm::FullRowsBitmap:  return {false, 2, kMoveCols, uint32_t(sizeof(MoveEntry)), ",BITMAP", ""};
        case TableForm::DeltaRowsBitmap: return {true, 3, kDeltaCols, kDeltaEntry, ",BITMAPD", ", 4-byte delta rows"};
        default:                         return {false, 0, kMoveCols, uint32_t(sizeof(MoveEntry)), "", ""};   // FullRows
    }
}
constexpr const char *kBitmapNote = ", collisions through per-env occupancy bitmaps";   // ... and, in the parentheses, about a form with bitmaps
// ... and back: the form a kernel instance <COMPACT, BITMAP> reads
constexpr int find_table_form(bool compact, int bitmap) {
    for (int f = 0; f < kTableForms; ++f)
        if (table_form_traits(TableForm(f)).compact == compact && table_form_traits(TableForm(f)).bitmap == bitmap) return f;
    return -1;
}
template <bool COMPACT, int BITMAP>
constexpr TableForm table_form_of() {
    static_assert(find_table_form(COMPACT, BITMAP) >= 0, "(COMPACT, BITMAP) names none of the six table forms");
    return TableForm(find_table_form(COMPACT, BITMAP));
}
// the kernel's LDS image up to the table's end (delta rows: the host-built image, zero-padded to 16 bytes), and the dynamic LDS
// segment of a launch: the image, then one bitmap per env of the block where the form has them
constexpr size_t table_image_bytes(TableForm form, uint32_t n_cells) {
    const TableFormTraits f = table_form_traits(form);
    return kMoveAt + (form == TableForm::DeltaRowsBitmap ? delta_table_words(n_cells) : size_t(n_cells) * f.cols) * f.entry_bytes;
}
constexpr size_t launch_lds_bytes(TableForm form, uint32_t n_cells, unsigned block, int Q) {
    return table_image_bytes(form, n_cells) + (table_form_traits(form).bitmap ? size_t(block / unsigned(Q)) * bitmap_stride(n_cells) : 0u);
}

// Which instances of the packed rollout kernels exist: X(K, Q, form) per family (each: streamed actions and the in-kernel policies, every criteria /
// terminal variant, recording or not).  mapf_lq_launch.hpp generates a family's dispatch from its list, in this order; mapf_plan.hip plans nothing else.
#define MAPF_LQ_ROLLOUT_INSTANCES(X)                                                                                       \
    X(8, 4, Rows8) X(8, 1, FullRows) X(8, 2, FullRows) X(8, 4, FullRows)                                                   \
    X(4, 8, DeltaRowsBitmap) X(4, 8, FullRowsBitmap) X(4, 8, Rows8x5Bitmap) X(4, 8, Rows8x4Bitmap)                         \
    X(4, 4, Rows8) X(4, 8, Rows8) X(4, 16, Rows8)                                                                          \
    X(4, 1, FullRows) X(4, 2, FullRows) X(4, 4, FullRows) X(4, 8, FullRows) X(4, 16, FullRows)                             \
    X(2, 2, FullRows) X(2, 4, FullRows) X(2, 8, FullRows) X(2, 16, FullRows)
// ... of lq_rollout_kernel_table (the table policy): full rows with two or four agents per lane, the 32-agent delta-row form
#define MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X)                                                                                 \
    X(4, 8, DeltaRowsBitmap) X(4, 1, FullRows) X(4, 2, FullRows) X(4, 4, FullRows) X(4, 8, FullRows)                       \
    X(2, 2, FullRows) X(2, 4, FullRows) X(2, 8, FullRows) X(2, 16, FullRows)
constexpr bool lq_rollout_instance_exists(int K, int Q, TableForm form, bool table_policy) {
#define X(KK, QQ, FF) if (K == KK && Q == QQ && form == TableForm::FF) return true;
    if (table_policy) { MAPF_LQ_ROLLOUT_TABLE_INSTANCES(X) } else { MAPF_LQ_ROLLOUT_INSTANCES(X) }
#undef X
    return false;
}

// The forms of the packed single step (mapf_lq_step.hip): the plain step, or a resident grid with the move table in LDS.  The values
// are the kernel's BIG template argument and the `form` number of a step plan (mapf_plan.hpp).
enum class StepForm : int { Plain = 0, FullRows = 1, DeltaRows = 2, DeltaRowsBitmap = 3 };   // (16-byte rows; 4-byte delta rows; ... + per-env occupancy bitmaps)
struct StepFormTraits {
    bool resident, bitmap;           // a resident grid walks the batch in chunks; per-env occupancy bitmaps follow the table (kBitmapNote)
    const char *tag, *note;          // what the kernel's name says about the form, as TableFormTraits
};
constexpr StepFormTraits step_form_traits(StepForm form) {
    switch (form) {
        case StepForm::FullRows:        return {true, false, ",BIG", ", move table in LDS"};
        case StepForm::DeltaRows:       return {true, false, ",DELTA", ", 4-byte delta rows of the move table in LDS"};
        case StepForm::DeltaRowsBitmap: return {true, true, ",DELTA,BITMAP", ", 4-byte delta rows of the move table in LDS"};
        default:                        return {false, false, "", ""};   // Plain
    }
}
// Which instances of lq_step_kernel exist: X(Q, K, form), each with and without the scenario table and terminal handling, in the order
// plan_step_lq tries their forms.  mapf_lq_step.hip generates its dispatch from the list, in this order (which is what keeps the
// kernels' places in the object); mapf_plan.hip plans nothing else.
#define MAPF_LQ_STEP_INSTANCES(X)                                                                                          \
    X(1, 8, FullRows) X(2, 8, FullRows) X(4, 8, FullRows)                                                                  \
    X(8, 4, DeltaRowsBitmap)                                                                                               \
    X(1, 4, DeltaRows) X(2, 4, DeltaRows) X(4, 4, DeltaRows) X(8, 4, DeltaRows)                                            \
    X(1, 4, FullRows) X(2, 4, FullRows) X(4, 4, FullRows) X(8, 4, FullRows)                                                \
    X(1, 4, Plain) X(2, 4, Plain) X(4, 4, Plain) X(8, 4, Plain) X(16, 4, Plain)                                            \
    X(2, 2, Plain) X(4, 2, Plain) X(8, 2, Plain) X(16, 2, Plain)
constexpr bool lq_step_instance_exists(int K, int Q, StepForm form) {
#define X(QQ, KK, FF) if (Q == QQ && K == KK && form == StepForm::FF) return true;
    MAPF_LQ_STEP_INSTANCES(X)
#undef X
    return false;
}

// env.P[s][a] for teams of up to eight agents (transitions_rows_kernel<MAXA>, mapf_transitions.hip): a wave's dynamic LDS holds,
// for its 2^qw_log2 queries, the prefix slots (4 bytes a query), then the queries -- a 48-byte header (QueryHeader) and one 16-byte
// record per (agent, list entry) each -- then the scratch of the cooperative set-up, which the 6- and 8-agent instances have:
// 16 bytes per (query, agent)
constexpr uint32_t kQueryHeader = 48, kRecord = 16;
constexpr bool transitions_cooperative(int max_a) { return max_a >= 6; }
constexpr uint32_t transitions_records_bytes(int max_a) { return kQueryHeader + uint32_t(max_a) * 3u * kRecord; }   // header + records
constexpr uint32_t transitions_scratch_bytes(int max_a) { return transitions_cooperative(max_a) ? uint32_t(max_a) * 16u : 0u; }
constexpr uint32_t transitions_query_lds_bytes(int max_a) { return transitions_records_bytes(max_a) + 4u + transitions_scratch_bytes(max_a); }
constexpr size_t transitions_wave_lds_bytes(int max_a, uint32_t qw_log2) { return size_t(transitions_query_lds_bytes(max_a)) << qw_log2; }

}  // namespace mapf
