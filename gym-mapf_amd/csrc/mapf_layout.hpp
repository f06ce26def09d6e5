// LDS layout of the kernels that keep the move table in LDS: ONE definition for the kernels (mapf_lg_rollout.hip,
// mapf_lq_rollout.hip, mapf_lq_step.hip) and for the launch planner (mapf_plan.hip), which decides whether an image fits.
#pragma once
#include "mapf_kernels.hpp"

#include <cstddef>

namespace mapf {

// The CU has 160 KiB of LDS; the first 1 KB of every image is the table image (slip rows, then outcome rows)
constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
static_assert(sizeof(SlipRow) * 8 + sizeof(OutcomeRow) * 16 <= kLdsReserve, "static LDS of the rollout kernel");

// packed rollout (mapf_lq_rollout.hip): slip rows at 0, outcome rows behind them, move table at 1024 with SIX columns per cell
constexpr uint32_t kSlipAt = 0, kOutcomeAt = sizeof(SlipRow) * 8, kMoveAt = kLdsReserve, kMoveCols = 6;
constexpr uint32_t kCompactCols = 5, kCompactEntry = 8;   // COMPACT: cells + code only, no sixth column
constexpr uint32_t kBitmapCols = 4;                       // COMPACT + BITMAP == 1: no STAY column either
constexpr uint32_t kDeltaEntry = 4;                       // COMPACT + BITMAP == 3: 4-byte delta rows, six columns (kDeltaCols, mapf_kernels.hpp: STAY twice, as the full table)
static_assert(kOutcomeAt + sizeof(OutcomeRow) * 16 <= kMoveAt, "LDS image: slip rows, outcome rows, then the move table");

// packed single step, LDS-table forms (mapf_lq_step.hip BIG): the same image, the table at the same place
#ifndef MAPF_BIG_COLS
#define MAPF_BIG_COLS 6
#endif
constexpr uint32_t kStepMoveAt = kMoveAt, kBigCols = MAPF_BIG_COLS;

// bytes of one env's occupancy bitmap (BITMAP instances): one bit per cell, padded to 16 bytes
inline size_t bitmap_stride(uint32_t n_cells) { return (size_t((n_cells + 31u) / 32u) * 4u + 15u) & ~size_t(15); }

}  // namespace mapf
