// Lane-group family: fused T-step rollout kernel and its launcher (device code: mapf_lg.hpp).
#include "mapf_lg.hpp"

#include <cstdlib>
#include <string>

namespace mapf {

// Largest block a rollout kernel may be launched with: groups of 16 lanes unroll 8 rotation rounds and need more
// than the 128 registers a 1024-thread block leaves per lane.
template <int L> constexpr unsigned rollout_max_block() { return L == 16 ? 512u : 1024u; }

// raw (still packed) action bytes of a lane's two slots: byte 0 = agent 2g, byte 1 = agent 2g+1.  Kept packed so
// that a prefetch issued one step ahead is not forced to complete by an unpack.
template <bool EVEN>
__device__ __forceinline__ uint32_t load_actions_raw(const uint8_t *base, uint32_t row, uint32_t n_agents, uint32_t g,
                                                     bool v0, bool v1) {
    const uint8_t *p = at(base, row * n_agents + 2u * g);
    uint32_t raw = 0u;
    if (EVEN || (n_agents & 1u) == 0u) {
        if (v0) raw = *reinterpret_cast<const uint16_t *>(p);
    } else {
        uint32_t lo = 0u, hi = 0u;
        if (v0) lo = p[0];
        if (v1) hi = p[1];
        raw = lo | (hi << 8);
    }
    return raw;
}

// MV_LDS: the whole move table (V*6 entries of 16 B) is staged into LDS once per block and the two gathers of
// every step become ds_read_b128 (a random 64-lane gather through the vector-memory pipe touches up to 64 cache
// lines).  RECORD: all five trajectory arrays are written every step (the C ABI substitutes scratch for absent
// ones), STREAM: actions come from memory, else from the in-kernel policy stream.  Both are compile-time so the
// loop body has no uniform branches around its memory operations.  DENSE (A == 2L and the env count fills every
// block) additionally removes the per-lane predicates: every lane owns two real agents, the action prefetch is
// clamped instead of guarded, and the four per-env scalars are stored by ALL lanes with per-lane addresses (even
// lanes of a group write done, odd lanes collision, the last lane prob, the others reward -- duplicates carry
// identical data), so the
// loop contains no exec-masked memory operation and the compiler can wait for the prefetched action word with a
// counted vmcnt(N) instead of draining every store.  Start cells stay in two registers per lane, so an
// auto-reset touches no memory.
#define MAPF_ROLLOUT_TABLE_KERNEL 0
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL
#define MAPF_ROLLOUT_TABLE_KERNEL 1
#include "mapf_lg_rollout_kernel.inc"
#undef MAPF_ROLLOUT_TABLE_KERNEL

// LDS budget for the move table: the CU has 160 KiB; keep room for the slip rows and the outcome table
static constexpr size_t kLdsBytes = 160 * 1024, kLdsReserve = 1024;
static_assert(sizeof(SlipRow) * 8 + sizeof(OutcomeRow) * 16 <= kLdsReserve, "static LDS of the rollout kernel");

// Defaults of the layout choices: a move table is staged into LDS while two blocks per CU still fit (a table that
// allows only one block per CU starves the SIMDs of waves); four agents per lane need one wave on every SIMD.
// ONE override: the environment variable MAPF_TUNE, "key=value,key=value,...", read here -- at handle creation, so a process
// can hold handles with different settings (the tests and the A/B tools do).  Keys (include/mapf_hip.h documents them):
//   quad_lanes, k, quad_min_lanes, oct_min_lanes, mv_lds_max_bytes, scen_table, bitmap_pairs, bitmap_block, bitmap_staycol,
//   bitmap_delta, step_big, step_block, step_delta, policy_table_lds.
// An unknown key or a malformed item is an error (*err names it): a typo must not silently measure the default.
RolloutTuning default_rollout_tuning(int device, std::string *err) {
    int n_cu = 256;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) n_cu = 256;
    return rollout_tuning_for(n_cu, getenv("MAPF_TUNE"), err);
}

RolloutTuning rollout_tuning_for(int n_cu, const char *text, std::string *err) {
    RolloutTuning t;
    // measured on 8 agents x 32768 envs (one wave per SIMD with four agents per lane, two with two): 517 G vs 467 G
    // agent-steps/s -- fewer, fatter waves win as long as no SIMD stays empty
    t.quad_min_lanes = uint64_t(n_cu) * 4u * 64u;        // CUs x SIMDs x lanes
    t.oct_min_lanes = uint64_t(n_cu) * 4u * 64u * 2u;    // (eight agents per lane: see try_launch_rollout_lq)
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
        else if (key == "policy_table_lds") t.policy_table_lds = v != 0 ? 1 : 0;
        else { if (err) *err = "MAPF_TUNE: unknown key '" + key + "'"; return t; }
    }
    return t;
}

// the table instances: the same two geometries as launch_rollout_lg_impl below
template <int L, bool FULL, bool RECORD>
static hipError_t launch_rollout_lg_table(const RolloutArgs &args, uint32_t A, const RolloutTuning &tune, hipStream_t stream, const TablePolicy &tp) {
    const size_t mv_bytes = size_t(args.c.n_cells) * kMvCols * sizeof(MoveEntry);
    const uint64_t threads = args.n_envs * uint64_t(L);
    if (mv_bytes + kLdsReserve <= tune.mv_lds_max_bytes && mv_bytes + kLdsReserve <= kLdsBytes && threads >= 64 * 256) {
        const size_t copies = (kLdsBytes - kLdsReserve) / (mv_bytes + sizeof(SlipRow) * 8);   // blocks per CU by LDS
        unsigned block = copies >= 4 ? 256u : (copies >= 2 ? 512u : 1024u);
        if (block > rollout_max_block<L>()) block = rollout_max_block<L>();
        const uint64_t per_block = block / unsigned(L);
        const unsigned grid = unsigned((args.n_envs + per_block - 1) / per_block);
        const bool dense = FULL && args.n_envs % per_block == 0;
        auto kern = dense ? lg_rollout_kernel_table<L, FULL, true, RECORD, FULL> : lg_rollout_kernel_table<L, FULL, true, RECORD, false>;
        if (mv_bytes > 32 * 1024) {
            if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes - kLdsReserve))) return e;
        }
        note_kernel("lg_rollout_kernel_table<L=%d,%s,MV_LDS,%s,TABLE,%s> block=%u (pair layout: 2 agents per lane; table policy: action bytes gathered from global memory)", L,
                    FULL ? "FULL" : "RAGGED", RECORD ? "RECORD" : "TOTALS", dense ? "DENSE" : "GUARDED", block);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), mv_bytes, stream, args, A, tp);
    } else {
        unsigned grid, block;
        lg_geometry(L, args.n_envs, grid, block);
        const bool dense = FULL && args.n_envs % (block / unsigned(L)) == 0;
        note_kernel("lg_rollout_kernel_table<L=%d,%s,MV_GLOBAL,%s,TABLE,%s> block=%u (pair layout: 2 agents per lane; table policy: action bytes gathered from global memory)", L,
                    FULL ? "FULL" : "RAGGED", RECORD ? "RECORD" : "TOTALS", dense ? "DENSE" : "GUARDED", block);
        if (dense) hipLaunchKernelGGL((lg_rollout_kernel_table<L, FULL, false, RECORD, FULL>), dim3(grid), dim3(block), 0, stream, args, A, tp);
        else hipLaunchKernelGGL((lg_rollout_kernel_table<L, FULL, false, RECORD, false>), dim3(grid), dim3(block), 0, stream, args, A, tp);
    }
    return hipGetLastError();
}

template <int L, bool FULL, bool RECORD, bool STREAM>
static hipError_t launch_rollout_lg_impl(const RolloutArgs &args, uint32_t A, const RolloutTuning &tune, hipStream_t stream) {
    const size_t mv_bytes = size_t(args.c.n_cells) * kMvCols * sizeof(MoveEntry);
    const uint64_t threads = args.n_envs * uint64_t(L);
    if (mv_bytes + kLdsReserve <= tune.mv_lds_max_bytes && mv_bytes + kLdsReserve <= kLdsBytes && threads >= 64 * 256) {
        // block size: as many waves as can share one table copy while >= 16 waves stay resident per CU
        const size_t copies = (kLdsBytes - kLdsReserve) / (mv_bytes + sizeof(SlipRow) * 8);   // blocks per CU by LDS
        unsigned block = copies >= 4 ? 256u : (copies >= 2 ? 512u : 1024u);
        if (block > rollout_max_block<L>()) block = rollout_max_block<L>();
        const uint64_t per_block = block / unsigned(L);
        const unsigned grid = unsigned((args.n_envs + per_block - 1) / per_block);
        const bool dense = FULL && args.n_envs % per_block == 0;
        auto kern = dense ? lg_rollout_kernel<L, FULL, true, RECORD, STREAM, FULL> : lg_rollout_kernel<L, FULL, true, RECORD, STREAM, false>;
        if (mv_bytes > 32 * 1024) {
            if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes - kLdsReserve))) return e;
        }
        note_kernel("lg_rollout_kernel<L=%d,%s,MV_LDS,%s,%s,%s> block=%u (pair layout: 2 agents per lane)", L,
                    FULL ? "FULL" : "RAGGED", RECORD ? "RECORD" : "TOTALS", STREAM ? "STREAM" : "POLICY", dense ? "DENSE" : "GUARDED", block);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), mv_bytes, stream, args, A);
    } else {
        unsigned grid, block;
        lg_geometry(L, args.n_envs, grid, block);
        note_kernel("lg_rollout_kernel<L=%d,%s,MV_GLOBAL,%s,%s,%s> block=%u (pair layout: 2 agents per lane)", L,
                    FULL ? "FULL" : "RAGGED", RECORD ? "RECORD" : "TOTALS", STREAM ? "STREAM" : "POLICY",
                    (FULL && args.n_envs % (block / unsigned(L)) == 0) ? "DENSE" : "GUARDED", block);
        if (FULL && args.n_envs % (block / unsigned(L)) == 0)
            hipLaunchKernelGGL((lg_rollout_kernel<L, FULL, false, RECORD, STREAM, FULL>), dim3(grid), dim3(block), 0, stream, args, A);
        else
            hipLaunchKernelGGL((lg_rollout_kernel<L, FULL, false, RECORD, STREAM, false>), dim3(grid), dim3(block), 0, stream, args, A);
    }
    return hipGetLastError();
}

hipError_t launch_rollout_lg(int n_agents, const RolloutArgs &args, const RolloutTuning &tune, hipStream_t stream, const TablePolicy *table) {
    if (args.n_envs == 0) return hipSuccess;
    if (args.actions) table = nullptr;                          // (streamed actions take precedence, as over the other policies)
    const int L = lg_group_size(n_agents);
    const bool full = n_agents == 2 * L;
    const uint32_t A = uint32_t(n_agents);
    // the record variant writes all five trajectory arrays: the C ABI passes either all of them or none
    const bool record = args.rec_local != nullptr, stream_actions = args.actions != nullptr;
    if (record && !(args.rec_reward && args.rec_prob && args.rec_done && args.rec_collision)) return hipErrorInvalidValue;
    hipError_t quad_status;
    if (try_launch_rollout_lq(n_agents, args, tune, stream, &quad_status, table)) return quad_status;
    if (table) {
        switch (L) {
#define X(N)                                                                                                         \
    case N:                                                                                                          \
        if (full) return record ? launch_rollout_lg_table<N, true, true>(args, A, tune, stream, *table)                          \
                                : launch_rollout_lg_table<N, true, false>(args, A, tune, stream, *table);                        \
        return record ? launch_rollout_lg_table<N, false, true>(args, A, tune, stream, *table)                                   \
                      : launch_rollout_lg_table<N, false, false>(args, A, tune, stream, *table);
            MAPF_FOR_EACH_L(X)
#undef X
            default: return hipErrorInvalidValue;
        }
    }
    switch (L) {
#define X(N)                                                                                                         \
    case N:                                                                                                          \
        if (full) return record ? (stream_actions ? launch_rollout_lg_impl<N, true, true, true>(args, A, tune, stream)          \
                                                  : launch_rollout_lg_impl<N, true, true, false>(args, A, tune, stream))        \
                                : (stream_actions ? launch_rollout_lg_impl<N, true, false, true>(args, A, tune, stream)         \
                                                  : launch_rollout_lg_impl<N, true, false, false>(args, A, tune, stream));      \
        return record ? (stream_actions ? launch_rollout_lg_impl<N, false, true, true>(args, A, tune, stream)                   \
                                        : launch_rollout_lg_impl<N, false, true, false>(args, A, tune, stream))                 \
                      : (stream_actions ? launch_rollout_lg_impl<N, false, false, true>(args, A, tune, stream)                  \
                                        : launch_rollout_lg_impl<N, false, false, false>(args, A, tune, stream));
        MAPF_FOR_EACH_L(X)
#undef X
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mapf
