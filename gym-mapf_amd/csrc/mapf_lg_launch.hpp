// Lane-group family: the launchers of its fused rollout and single-step kernels, once for every family of instances.  A launcher
// takes ONE plan (mapf_plan.hpp) and launches the instance it names; which kernels those instances are is the including unit's
// say, through a family type:
//   rollout -- Family::kernel<L, FULL, MV_LDS, RECORD, STREAM, TABLE>(dense) returns the address of an instance of lg_rollout_kernel
//              (mapf_lg_rollout_kernel.hpp).  mapf_lg_rollout.hip: the plain and the table instances, DENSE for full groups only;
//              mapf_lg_limit.hip: the limit instances, guarded only; mapf_lg_budget.hip: the budget instances, guarded only;
//              pairs/mapf_lg_pairs.hip: the instances of the three that count conflicting pairs, guarded only;
//              ../csrc_joint/mapf_lg_joint.hip: the instances that follow a joint table policy, guarded only and never streamed -- it
//              launches through the TABLE arm (no streamed actions) and its plan is marked `joint`, which the name reads;
//              ../csrc_group/mapf_lg_group.hip: the instances that follow a group policy, likewise (plan marked `group`);
//   step    -- Family::kernel<L, FULL, EXT_UNIFORMS>() likewise, of lg_step_kernel (mapf_lg_step_kernel.hpp).  mapf_lg_kernels.hip:
//              the plain instances; mapf_lg_limit.hip: the limit instances.
// `extra` are the kernel's arguments behind (args, A): nothing, the table policy, the episode limit, or both in that order; the
// budget instances take the episode budget behind the limit, the instances that count pairs the conflict matrix last; the joint
// instances take the joint table policy first, in the table policy's place.
#pragma once
#include "mapf_lg.hpp"
#include "mapf_plan.hpp"

namespace mapf {

// Launches the planned instance: (MV_LDS, dense) pick the kernel, the plan gives its geometry and its LDS segment (the move
// table, or nothing) and the name the launch notes.
template <class Family, int L, bool FULL, bool RECORD, bool STREAM, bool TABLE, class... Extra>
hipError_t launch_lg_rollout_instance(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const Extra &...extra) {
    const auto kern = plan.mv_lds ? Family::template kernel<L, FULL, true, RECORD, STREAM, TABLE>(plan.dense)
                                  : Family::template kernel<L, FULL, false, RECORD, STREAM, TABLE>(plan.dense);
    if (plan.lds_bytes > 32 * 1024) {
        // (the most a CU has beside the instance's static LDS: kLdsReserve, and kPairsLdsBytes more in the instances that count pairs,
        // kLogLdsBytes more in those that keep an episode log, kGroupLdsBytes more in those that follow a group policy)
        if (hipError_t e = allow_large_lds(reinterpret_cast<const void *>(kern), int(kLdsBytes - kLdsReserve - (plan.pairs ? kPairsLdsBytes : 0) - (plan.log ? kLogLdsBytes : 0) -
                                                                                         (plan.group ? kGroupLdsBytes : 0)))) return e;
    }
    char name[kKernelNameBytes];
    lg_rollout_kernel_name(name, plan, RECORD, STREAM, TABLE);
    note_kernel(name);
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, args, A, extra...);
    return hipGetLastError();
}

// the instance's other arguments: the plan's L and FULL, RECORD and STREAM from the arrays the launch names (under TABLE no launch
// streams its actions, and both arms of P name the one table instance)
template <class Family, bool TABLE, class... Extra>
hipError_t launch_lg_rollout(const LgRolloutPlan &plan, const RolloutArgs &args, uint32_t A, hipStream_t stream, const Extra &...extra) {
    const bool record = args.rec_local != nullptr, streamed = !TABLE && args.actions != nullptr;
    switch (plan.L) {
#define P(N, FULL, RECORD) (streamed ? launch_lg_rollout_instance<Family, N, FULL, RECORD, !TABLE, TABLE>(plan, args, A, stream, extra...)  \
                                     : launch_lg_rollout_instance<Family, N, FULL, RECORD, false, TABLE>(plan, args, A, stream, extra...))
#define X(N)                                                                                                         \
    case N:                                                                                                          \
        if (plan.full) return record ? P(N, true, true) : P(N, true, false);                                         \
        return record ? P(N, false, true) : P(N, false, false);
        MAPF_FOR_EACH_L(X)
#undef X
#undef P
        default: return hipErrorInvalidValue;
    }
}

// the single step: the plan's L and FULL, EXT_UNIFORMS from the launch's arrays
template <class Family, class... Extra>
hipError_t launch_lg_step(const LgStepPlan &plan, const StepArgs &args, uint32_t A, hipStream_t stream, const Extra &...extra) {
    const bool ext = args.uniforms != nullptr;
    void (*kern)(const StepArgs, const uint32_t, const Extra...) = nullptr;
    switch (plan.L) {
#define X(N)                                                                                                                       \
    case N:                                                                                                                        \
        kern = ext ? (plan.full ? Family::template kernel<N, true, true>() : Family::template kernel<N, false, true>())            \
                   : (plan.full ? Family::template kernel<N, true, false>() : Family::template kernel<N, false, false>());         \
        break;
        MAPF_FOR_EACH_L(X)
#undef X
        default: return hipErrorInvalidValue;
    }
    char name[kKernelNameBytes];
    lg_step_kernel_name(name, plan, ext);
    note_kernel(name);
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.block), 0, stream, args, A, extra...);
    return hipGetLastError();
}

}  // namespace mapf
