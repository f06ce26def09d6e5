// Lane-group family under the group policy (include/mapf_hip.h MAPF_POLICY_GROUP, mapf_set_policy_group; GroupPolicy in
// csrc/mapf_kernels.hpp, the device table in csrc/mapf_group_table.hpp): the forms of the fused rollout kernels whose agents follow
// a solo row and, where they are merged into a group of two to four, the entry of the group's current joint cell in the group's book
// if it has one; the family that names them to the shared launcher (csrc/mapf_lg_launch.hpp), and the launchers that take the
// route's plan.  Compiled once per form (the Makefile's fifth table: MAPF_GROUP_FORM 0 plain, 1 under an episode step limit, 2 under
// an episode budget; MAPF_GROUP_PAIRS 1: with the conflict matrix last; MAPF_GROUP_LOG 1, budget form only: with the episode log
// behind the budget), each a unit of its own: the kernels that exist without the mode keep their code.  The source lies beside
// csrc/, csrc_joint/ and csrc_log/, not below them: the tests that pin the first four tables also pin which .hip files those hold.
//
// Per env and step (the header has the definition): the step is a mapf_step with the looked-up actions -- slip, collisions, reward,
// termination, both Philox streams' counters, limit, budget, conflict counting and the log are those of the instance without the
// mode; the policy stream is not drawn.
#include "../csrc/mapf_lg_launch.hpp"
#include "../csrc/mapf_lg_rollout_kernel.hpp"

#if !defined(MAPF_GROUP_FORM) || !defined(MAPF_GROUP_PAIRS) || !defined(MAPF_GROUP_LOG)
#error "MAPF_GROUP_FORM: 0 plain, 1 limit, 2 budget; MAPF_GROUP_PAIRS: 0 | 1; MAPF_GROUP_LOG: 0 | 1 (the Makefile compiles this unit once per form)"
#endif
#if MAPF_GROUP_LOG && MAPF_GROUP_FORM != 2
#error "the episode log comes with the budget form only"
#endif

namespace mapf {

// the instances of lg_rollout_kernel (csrc/mapf_lg_rollout_kernel.hpp) with the GroupPolicy argument first, then the blocks of the
// form; guarded only, never streamed (the launcher's TABLE arm: a launch without streamed actions).
// each form: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances
template <class... Form>
struct LgRolloutGroupFamily {
    template <int L, bool FULL, bool MV_LDS, bool RECORD, bool STREAM, bool TABLE>
    static auto kernel(bool) {
        static_assert(TABLE && !STREAM, "the group launches run without streamed actions");
        return lg_rollout_kernel<L, FULL, MV_LDS, RECORD, false, false, GroupPolicy, Form...>;
    }
};

// the route's plan, marked `group` (the dispatcher has checked the blocks), to the shared launcher
#if MAPF_GROUP_PAIRS
#define MAPF_GROUP_TAIL , ConflictPairs
#define MAPF_GROUP_TAIL_ARG , *pairs
#else
#define MAPF_GROUP_TAIL
#define MAPF_GROUP_TAIL_ARG
#endif
#define MAPF_GROUP_SIGNATURE(form)                                                                                                           \
    hipError_t launch_rollout_lg_group_##form(const LgRolloutPlan &plan, int n_agents, const RolloutArgs &args, hipStream_t stream, const GroupPolicy &group, \
                                              const EpisodeLimit *limit, const EpisodeBudget *budget, const EpisodeLog *log, const ConflictPairs *pairs)
#define MAPF_GROUP_REFUSES ((pairs != nullptr) != bool(MAPF_GROUP_PAIRS) || (log != nullptr) != bool(MAPF_GROUP_LOG) || plan.log != bool(MAPF_GROUP_LOG) || !plan.group)

#if MAPF_GROUP_FORM == 0
#if MAPF_GROUP_PAIRS
MAPF_GROUP_SIGNATURE(pairs_plain) {
    using Family = LgRolloutGroupFamily<ConflictPairs>;
#else
MAPF_GROUP_SIGNATURE(plain) {
    using Family = LgRolloutGroupFamily<>;
#endif
    if (limit || budget || MAPF_GROUP_REFUSES) return hipErrorInvalidValue;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, group MAPF_GROUP_TAIL_ARG);
}
#elif MAPF_GROUP_FORM == 1
#if MAPF_GROUP_PAIRS
MAPF_GROUP_SIGNATURE(pairs_limit) {
#else
MAPF_GROUP_SIGNATURE(limit) {
#endif
    if (!limit || budget || MAPF_GROUP_REFUSES) return hipErrorInvalidValue;
    using Family = LgRolloutGroupFamily<EpisodeLimit MAPF_GROUP_TAIL>;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, group, *limit MAPF_GROUP_TAIL_ARG);
}
#elif MAPF_GROUP_LOG
#if MAPF_GROUP_PAIRS
MAPF_GROUP_SIGNATURE(log_pairs_budget) {
#else
MAPF_GROUP_SIGNATURE(log_budget) {
#endif
    if (!limit || !budget || MAPF_GROUP_REFUSES) return hipErrorInvalidValue;
    using Family = LgRolloutGroupFamily<EpisodeLimit, EpisodeBudget, EpisodeLog MAPF_GROUP_TAIL>;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, group, *limit, *budget, *log MAPF_GROUP_TAIL_ARG);
}
#else
#if MAPF_GROUP_PAIRS
MAPF_GROUP_SIGNATURE(pairs_budget) {
#else
MAPF_GROUP_SIGNATURE(budget) {
#endif
    if (!limit || !budget || MAPF_GROUP_REFUSES) return hipErrorInvalidValue;
    using Family = LgRolloutGroupFamily<EpisodeLimit, EpisodeBudget MAPF_GROUP_TAIL>;
    return launch_lg_rollout<Family, true>(plan, args, uint32_t(n_agents), stream, group, *limit, *budget MAPF_GROUP_TAIL_ARG);
}
#endif

}  // namespace mapf
