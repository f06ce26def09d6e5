// Lane-group family: fused T-step rollout kernel and the launcher of its instances without an episode limit (device code:
// mapf_lg.hpp; the launch's plan: the route's, mapf_plan.hip; the launcher proper: mapf_lg_launch.hpp).
#include "mapf_lg_launch.hpp"
#include "mapf_lg_rollout_kernel.hpp"

namespace mapf {

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
// auto-reset touches no memory.  (The kernel: mapf_lg_rollout_kernel.hpp.)

// The instances without an episode limit: lg_rollout_kernel with no further argument, or with the table policy (TABLE: then STREAM
// is false); DENSE exists for full groups only.
struct LgRolloutFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool dense) {
        if constexpr (TABLE) return dense ? lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, FULL, TablePolicy> : lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, TablePolicy>;
        else return dense ? lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, FULL> : lg_rollout_kernel<L, FULL, MV_LDS, RECORD, STREAM, false>;
    }
};

hipError_t launch_rollout_lg(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const TablePolicy *table) {
    return table ? launch_lg_rollout<LgRolloutFamily, true>(plan, args, uint32_t(n_agents), stream, *table)
                 : launch_lg_rollout<LgRolloutFamily, false>(plan, args, uint32_t(n_agents), stream);
}

}  // namespace mapf
