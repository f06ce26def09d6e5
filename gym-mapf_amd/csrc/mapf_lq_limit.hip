// Packed table-policy rollout under an episode step limit (include/mapf_hip.h mapf_set_episode_limit; EpisodeLimit in
// mapf_kernels.hpp): the instances of lq_rollout_kernel (mapf_lq_rollout_kernel.hpp) that take an EpisodeLimit behind the table
// policy -- the limit forms of mapf_lq_rollout.hip's table instances -- and the family that names them to the shared launcher
// (mapf_lq_launch.hpp).  A translation unit of its own, compiled beside the others.  Reached only with MAPF_TUNE limit_packed=1 (route_rollout, mapf_plan.hip); every launch
// this family declines -- and every launch under a limit without the key -- is the lane-group limit instance's (mapf_lg_limit.hip).
//
// The four rules of the limit are mapf_lg_limit.hip's.  In the packed body they hang on the group-uniform code of the step
// (code16, from which every select of the reset logic is derived): a live step ended its episode exactly when code16 != 4 * 16,
// so `truncated` needs no outcome row.  Nothing else of a step changes: reward, prob, done, collision, the totals and every
// Philox counter are those of the table instances without the limit.
//
// Only the table instances have a limit form: built for 512 threads they have 256 vector registers per lane and use at most
// 122; the streamed and in-kernel-policy instances sit at 128 of 128 in their 1024-thread forms.
#include "mapf_lq_launch.hpp"
#include "mapf_lq_rollout_kernel.hpp"

namespace mapf {

namespace {

// exactly the table instances (MAPF_LQ_ROLLOUT_TABLE_INSTANCES, mapf_layout.hpp), built for 512 threads as they are, with the
// EpisodeLimit argument behind the table policy's two
struct LqTableLimitFamily {
    static constexpr bool kTable = true, kLimit = true;
    template <int Q, int K, bool RECORD, bool STREAM, bool SOC, bool COMPACT, bool TERM, int BITMAP, int TABLE>
    static auto kernel() { return lq_rollout_kernel<Q, K, RECORD, false, SOC, COMPACT, TERM, BITMAP, TABLE, TablePolicy, uint32_t, EpisodeLimit>; }
};

}  // namespace

static_assert(kLqK == 4 || kLqK == 2, "compile with -DMAPF_LQ_K=4|2: the table instances have four or two agents per lane");

// (every launch here follows the table policy under a limit: without either it is not this object's)
MAPF_LQ_LAUNCHER(launch_rollout_lq_limit_k) {
    if (!table || !limit) return hipErrorInvalidValue;
    return launch_lq_rollout<LqTableLimitFamily, kLqK, kLqRecord>(plan, args, A, stream, table, *limit);
}

}  // namespace mapf
