// Lane-group family under the joint table policy (include/mapf_hip.h MAPF_POLICY_JOINT, mapf_set_policy_joint; JointPolicy in
// csrc/mapf_kernels.hpp): the forms of the fused rollout kernels whose agents follow a table over their own cell and, where they
// are merged with a partner, the partner's cell too; the family that names them to the shared launcher (csrc/mapf_lg_launch.hpp),
// and the launcher that takes the route's plan.  Compiled once per form (the Makefile's third table: MAPF_JOINT_FORM 0 plain,
// 1 under an episode step limit, 2 under an episode budget; MAPF_JOINT_PAIRS 1: with the conflict matrix last), each a unit of its own:
// the kernels that exist without the mode keep their code.  The source lies beside csrc/, not below it: the tests that pin the
// first two tables also pin which .hip files csrc/ holds.
//
// Per env and step (the header has the definition): the step is a mapf_step with the gathered actions -- slip, collisions, reward,
// termination, both Philox streams' counters, limit, budget and conflict counting are those of the instance without the mode; the
// policy stream is not drawn.
#include "../csrc/mapf_lg_launch.hpp"
#include "../csrc/mapf_lg_rollout_kernel.hpp"

#if !defined(MAPF_JOINT_FORM) || !defined(MAPF_JOINT_PAIRS)
#error "MAPF_JOINT_FORM: 0 plain, 1 limit, 2 budget; MAPF_JOINT_PAIRS: 0 | 1 (the Makefile compiles this unit once per form)"
#endif

namespace mapf {

// the instances of lg_rollout_kernel (csrc/mapf_lg_rollout_kernel.hpp) with the JointPolicy argument first, then the blocks of the
// form; guarded only, never streamed (the launcher's TABLE arm: a launch without streamed actions).
// each form: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances
template <class... Form>
struct LgRolloutJointFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        static_assert(TABLE && !STREAM, "the joint launches run without streamed actions");
        return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, JointPolicy, Form...>;
    }
};

// the route's plan, marked `joint` (the dispatcher has checked the blocks), to the shared launcher
#if MAPF_JOINT_PAIRS
#define MAPF_JOINT_NAME(form) launch_rollout_lg_joint_pairs_##form
#define MAPF_JOINT_TAIL , ConflictPairs
#define MAPF_JOINT_TAIL_ARG , *pairs
#else
#define MAPF_JOINT_NAME(form) launch_rollout_lg_joint_##form
#define MAPF_JOINT_TAIL
#define MAPF_JOINT_TAIL_ARG
#endif
#define MAPF_JOINT_SIGNATURE(form)                                                                                                   \
    hipError_t MAPF_JOINT_NAME(form)(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const JointPolicy &joint, \
                                     const EpisodeLimit *limit, const EpisodeBudget *budget, const ConflictPairs *pairs)

#if MAPF_JOINT_FORM == 0
MAPF_JOINT_SIGNATURE(plain) {
    if (limit || budget || (pairs != nullptr) != bool(MAPF_JOINT_PAIRS) || !plan.joint) return hipErrorInvalidValue;
#if MAPF_JOINT_PAIRS
    using Family = LgRolloutJointFamily<ConflictPairs>;
#else
    using Family = LgRolloutJointFamily<>;
#endif
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, joint MAPF_JOINT_TAIL_ARG);
}
#elif MAPF_JOINT_FORM == 1
MAPF_JOINT_SIGNATURE(limit) {
    if (!limit || budget || (pairs != nullptr) != bool(MAPF_JOINT_PAIRS) || !plan.joint) return hipErrorInvalidValue;
    using Family = LgRolloutJointFamily<EpisodeLimit MAPF_JOINT_TAIL>;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, joint, *limit MAPF_JOINT_TAIL_ARG);
}
#else
MAPF_JOINT_SIGNATURE(budget) {
    if (!limit || !budget || (pairs != nullptr) != bool(MAPF_JOINT_PAIRS) || !plan.joint) return hipErrorInvalidValue;
    using Family = LgRolloutJointFamily<EpisodeLimit, EpisodeBudget MAPF_JOINT_TAIL>;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, joint, *limit, *budget MAPF_JOINT_TAIL_ARG);
}
#endif

}  // namespace mapf
