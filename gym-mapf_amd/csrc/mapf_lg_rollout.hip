// Lane-group family: fused T-step rollout kernel and its launcher (device code: mapf_lg.hpp).
#include "mapf_lg.hpp"
#include "mapf_layout.hpp"

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

// (LDS budget for the move table -- kLdsBytes, kLdsReserve: mapf_layout.hpp)

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
