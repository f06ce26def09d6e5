// C ABI of libmapf_hip.so (declared in include/mapf_hip.h): the handle and what it owns, host<->device staging for the
// host-pointer mode, argument validation, and the launches.  The tables a handle uploads are built by mapf_tables.hip,
// which form a launch takes is planned by mapf_plan.hip.
#include "mapf_hip.h"
#include "mapf_kernels.hpp"
#include "mapf_plan.hpp"
#include "mapf_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_last_error;
thread_local char g_noted_kernel[mapf::kKernelNameBytes] = "";

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(MAPF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(_e, #expr);    \
    } while (0)

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// Move-only owner of hipMalloc memory (reads as the pointer it owns)
template <typename T>
struct DevicePtr {
    T *ptr = nullptr;
    DevicePtr() = default;
    DevicePtr(DevicePtr &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)) {}
    DevicePtr &operator=(DevicePtr &&o) noexcept { std::swap(ptr, o.ptr); return *this; }
    ~DevicePtr() { reset(); }
    void reset() { if (ptr) (void)hipFree(ptr); ptr = nullptr; }
    hipError_t alloc(size_t count) { reset(); return hipMalloc(reinterpret_cast<void **>(&ptr), count * sizeof(T)); }
    hipError_t upload(const T *src, size_t count) {   // a fresh allocation holding src[0 .. count)
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemcpy(ptr, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    operator T *() const { return ptr; }
};

// Scratch device buffer that grows on demand (host-pointer mode staging).
struct DeviceBuf : NoCopy {
    void *ptr = nullptr;
    size_t cap = 0;
    ~DeviceBuf() { if (ptr) (void)hipFree(ptr); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (ptr) { (void)hipFree(ptr); ptr = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
};

// Pinned host block mapped into the device's address space: for tiny host-mode calls (the scalar MapfEnv.step()
// regime: one env, a handful of agents) the kernel reads its inputs from and writes its outputs to this block
// directly, so a call is one launch + one stream sync instead of up to nine hipMemcpyAsync round trips.
struct PinnedBlock : NoCopy {
    char *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    ~PinnedBlock() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&host), bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) { host = nullptr; return e; }
        e = hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), host, 0);
        if (e != hipSuccess) { (void)hipHostFree(host); host = dev = nullptr; return e; }
        cap = bytes;
        return hipSuccess;
    }
    void release() { if (host) (void)hipHostFree(host); host = dev = nullptr; cap = 0; }
};

// The stream and the timer events of a handle.  A BASE of the handle, so that it is destroyed after every member: buffers
// go before the events, the stream last and only if the handle created it.
struct StreamAndEvents : NoCopy {
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool own_stream = false;
    ~StreamAndEvents() {
        if (ev_begin) (void)hipEventDestroy(ev_begin);
        if (ev_end) (void)hipEventDestroy(ev_end);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};
constexpr size_t kZeroCopyMaxBytes = 16 * 1024;   // beyond this the DMA copies win over PCIe-direct accesses

}  // namespace

namespace mapf {
void note_kernel(const char *name) { snprintf(g_noted_kernel, sizeof(g_noted_kernel), "%s", name); }
}  // namespace mapf

struct mapf_graph_s {
    mapf_handle_t owner = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t steps = 0;               // env-steps one replay advances the handle by
    bool ends_may_be_terminal = true; // mapf_handle_s::may_be_terminal after a replay (conservative: true unless the
                                      // recording's last state-changing call auto-resets every finished episode)
    ~mapf_graph_s() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

struct mapf_handle_s : StreamAndEvents {
    int device = 0;
    std::string last_step_kernel, last_rollout_kernel, last_transitions_kernel;
    uint32_t V = 0, A = 0, flags = 0;
    uint64_t E = 0, env_id_offset = 0, t = 0;
    mapf::EnvConsts c{};
    bool start_broadcast = false, goal_broadcast = false, device_ptrs = false;
    bool stream_exposed = false;   // mapf_get_stream was called: somebody else may capture the stream (check_foreign_capture)
    mapf::FamilyPreference prefer = mapf::FamilyPreference::Auto;   // the kernel family the create flags ask for (what a launch takes: mapf_plan.hpp's route)
    bool start_terminal_any = true;   // is_terminal(start) for some env (looked up once at create)
    bool mv_delta8 = false;           // every neighbour id lies within +-127 of its cell's id (the 4-byte delta rows of the bitmap rollout)
    // Can some env be terminal right now?  Not after a call that auto-reset every finished episode (unless a START state
    // is itself terminal) or after a full reset; yes after steps without auto-reset and after set_state.  The packed
    // single step runs its instance without is_terminal(prev) when the answer is no.  While recording a graph the
    // question is asked about the recording's own history only (cap_may_be_terminal: the first recorded step cannot know
    // what precedes a replay).
    bool may_be_terminal = true, cap_may_be_terminal = true;
    mapf::RolloutTuning tune;
    DevicePtr<mapf::MoveEntry> mv;
    DevicePtr<mapf::CompactEntry> mv8;   // the 8-byte-row form of the move table (the packed single step gathers from it)
    DevicePtr<uint32_t> mv4;          // the 4-byte delta-row form (kernels that keep the table of a 64x64 map in LDS); null unless mv_delta8
    DevicePtr<mapf::TableImage> slip; // the 1 KB table image: slip rows, then the outcome rows
    std::vector<uint16_t> nbr;        // host copy of the neighbour table (policy tables are derived from it)
    DevicePtr<uint2> policy_cells;    // greedy policy table (mapf_set_policy); null = random policy stream
    // table policy (mapf_set_policy_table): device copies of the action bytes and of the agents' row indices, and the view of
    // them the kernels are handed; table.table null = off
    DevicePtr<uint8_t> table_bytes;
    DevicePtr<uint16_t> table_rows;
    mapf::TablePolicy table{};
    // joint table policy (mapf_set_policy_joint): device copies of the action bytes, the agents' segment offsets and partners, and
    // the view of them the kernels are handed; joint.table null = off.  At most one of table / joint is on
    DevicePtr<uint8_t> joint_bytes;
    DevicePtr<uint32_t> joint_offset;
    DevicePtr<uint16_t> joint_partner;
    mapf::JointPolicy joint{};
    // group policy (mapf_set_policy_group): device copies of the solo rows, the agents' row indices, member lists and books, and of the
    // open-addressing table of all books, and the view of them the kernels are handed; group.table null = off.  At most one of
    // table / joint / group is on
    DevicePtr<uint8_t> group_bytes;
    DevicePtr<uint16_t> group_rows, group_members;
    DevicePtr<uint32_t> group_book;
    DevicePtr<mapf::GroupSlot> group_slots;
    mapf::GroupPolicy group{};
    DevicePtr<uint16_t> state, start, goal;
    // episode step limit (mapf_set_episode_limit): N (0 = none) and the per-env ages, which are all zero while N == 0 -- only the
    // limit kernels and mapf_episode_steps write them, and only a handle with a limit runs those
    uint32_t episode_limit = 0;
    DevicePtr<uint32_t> age;
    DeviceBuf s_trunc, s_rtrunc, s_age, x_trunc;   // staging of out_truncations / rec_truncated / the ages; stand-in for rec_truncated
    // episode budget (mapf_set_episode_budget): B (0 = none) and the per-env episodes left, which are all zero while B == 0 -- only the
    // budget kernels, mapf_set_episode_budget and mapf_episodes_left write them
    uint32_t episode_budget = 0;
    DevicePtr<uint32_t> left;
    DeviceBuf s_live;                 // staging of out_live_steps
    // conflict matrix (mapf_set_conflict_pairs): the counts u64[n_slots * A * A] and the envs' slots (null: all in slot 0);
    // n_slots 0 = the mode is off and both are null.  Only the kernels that count, mapf_set_conflict_pairs and mapf_conflict_pairs write M
    uint32_t pair_slots = 0;
    DevicePtr<unsigned long long> pair_counts;
    DevicePtr<uint32_t> pair_slot_of_env;
    size_t pair_bytes() const { return size_t(pair_slots) * A * A * sizeof(unsigned long long); }
    // episode log (mapf_set_episode_log): the capacity C (0 = the mode is off and both are null), the per-env partials with the counts
    // behind them in one allocation (EpisodeLog, mapf_kernels.hpp), and the records [E * C].  Only the log kernels and the entry points
    // the header names write them
    uint32_t log_capacity = 0;
    DevicePtr<uint4> log_heads;       // E partials of 16 bytes, then E counts of 4: E * 20 bytes, as uint4 words (rounded up)
    DevicePtr<uint4> log_records;
    mapf::EpisodeLogPartial *log_partials() const { return reinterpret_cast<mapf::EpisodeLogPartial *>(log_heads.ptr); }
    uint32_t *log_counts() const { return mapf::episode_log_counts(log_partials(), E); }
    size_t log_record_bytes() const { return size_t(E) * log_capacity * sizeof(mapf_episode_record); }
    // host-pointer mode staging
    DeviceBuf s_actions, s_uniforms, s_local, s_reward, s_prob, s_done, s_coll, s_term, s_mask, s_ret, s_epi, s_ncoll;
    DeviceBuf x_local, x_reward, x_prob, x_done, x_coll;   // stand-ins for trajectory arrays the caller left out
    DeviceBuf q_local, q_actions, q_env, q_count, q_next, q_prob, q_reward, q_done, q_coll, q_next_in, q_offset;   // mapf_transitions staging
    DeviceBuf q_rel, q_blocks;        // mapf_transitions_compact: the scan's scratch (in-block offsets, block bases)
    PinnedBlock pinned;               // zero-copy staging of tiny host-mode steps
    // scenario table (StepArgs::scen): built at create when the batch has <= 256 distinct (start row, goal row) pairs
    DevicePtr<uint8_t> scen;
    DevicePtr<uint16_t> scen_rows;
    uint32_t n_scen = 0;
    // recording into a hipGraph (mapf_graph_begin .. mapf_graph_end): recorded launches take their step index from
    // *t_dev + their offset inside the recording; t_dev_value = what *t_dev holds once the stream has drained
    DevicePtr<uint64_t> t_dev;
    uint64_t t_dev_value = 0, cap_steps = 0;
    bool capturing = false;
    std::vector<mapf_graph_s *> graphs;   // recordings that are still alive (destroyed with the handle at the latest)

    const mapf::SlipRow *slip_rows() const { return slip.ptr ? slip.ptr->slip : nullptr; }
    // what a step / rollout / reset advances, reads and writes: the recording's own counter and flag while a graph is recorded
    uint64_t &steps() { return capturing ? cap_steps : t; }
    bool &terminal_possible() { return capturing ? cap_may_be_terminal : may_be_terminal; }
    void drop_policy_table() {
        table_bytes.reset();
        table_rows.reset();
        table = mapf::TablePolicy{};
    }
    void drop_policy_joint() {
        joint_bytes.reset();
        joint_offset.reset();
        joint_partner.reset();
        joint = mapf::JointPolicy{};
    }
    void drop_policy_group() {
        group_bytes.reset();
        group_rows.reset();
        group_members.reset();
        group_book.reset();
        group_slots.reset();
        group = mapf::GroupPolicy{};
    }
    // Teardown: the stream drains, then the recordings go (they name the handle's buffers), then the members -- every
    // buffer -- and last the base: events, and the stream if the handle created it.
    ~mapf_handle_s() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (mapf_graph_s *g : graphs) delete g;
    }
};

namespace {

int check_handle(mapf_handle_t h) {
    if (!h) return fail(MAPF_EINVAL, "null handle");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return MAPF_OK;
}

// entry points that wait for the stream, move the step index from the host side or free what a recorded node uses
// cannot run between mapf_graph_begin and mapf_graph_end
int check_not_recording(mapf_handle_t h, const char *what) {
    if (h->capturing) return fail(MAPF_EINVAL, std::string(what) + ": not allowed while a graph is being recorded (call mapf_graph_end first)");
    return MAPF_OK;
}

// A step or rollout enqueued while somebody ELSE is capturing the stream (a caller-owned stream under torch.cuda.graph /
// hipStreamBeginCapture) would bake the handle's current step index into the captured launch: every replay would reuse
// the same random numbers, silently.  Only mapf_graph_begin knows how to record a launch (device-side step index).
int check_foreign_capture(mapf_handle_t h, const char *what) {
    // (nobody else can capture a stream the handle created -- until mapf_get_stream has handed it out)
    if (h->capturing || (h->own_stream && !h->stream_exposed)) return MAPF_OK;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &status) != hipSuccess) { (void)hipGetLastError(); return MAPF_OK; }
    if (status != hipStreamCaptureStatusNone)
        return fail(MAPF_EINVAL, std::string(what) + ": the stream is being captured outside mapf_graph_begin -- the launch would bake its "
                                 "step index (and random numbers) into the graph; record it between mapf_graph_begin and mapf_graph_end");
    return MAPF_OK;
}

// The lane-group kernels address every array with 32-bit byte offsets (one SGPR base + one VGPR offset per
// access): the largest array of a call must stay below 4 GiB.  rows = E (step) or T*E (rollout).
int check_extent(mapf_handle_t h, uint64_t rows, bool has_uniforms) {
    const uint64_t limit = uint64_t(1) << 32;
    const uint64_t per_agent = has_uniforms ? sizeof(double) : sizeof(uint16_t);
    if (rows * h->A * per_agent >= limit || rows * sizeof(double) >= limit)
        return fail(MAPF_EINVAL, "call too large: every array of one call must stay below 4 GiB (use fewer steps per rollout)");
    return MAPF_OK;
}

bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// One array of a call, named ONCE: the caller's pointer (host memory, or device memory for a MAPF_FLAG_DEVICE_PTRS handle), its
// size, the handle's staging buffer for it, which way it travels, the field of the launch's argument block that receives the
// device pointer, and its name in the alignment error.  A call lists its arrays in a fixed-size array on its stack; stage_arrays()
// before the launch and fetch_arrays() after it walk that list.
struct CallArray {
    DeviceBuf *buf;
    const void *user;
    size_t bytes;
    void *slot;                       // a `T *` / `const T *` field (every object pointer has one representation)
    const char *name;
    bool upload, download;
};
template <typename T>
CallArray input(DeviceBuf &buf, const T *user, size_t count, const T **slot, const char *name) { return {&buf, user, count * sizeof(T), slot, name, true, false}; }
template <typename T>
CallArray output(DeviceBuf &buf, T *user, size_t count, T **slot, const char *name, bool upload_too = false) { return {&buf, user, count * sizeof(T), slot, name, upload_too, true}; }

// host mode: every array gets its staging buffer (inputs are copied there); device mode: the caller's pointers pass through
int stage_arrays(mapf_handle_t h, const CallArray *arrays, size_t n) {
    for (const CallArray *e = arrays; e != arrays + n; ++e) {
        void *dev = nullptr;
        if (e->user && h->device_ptrs) {
            if (misaligned(e->user)) return fail(MAPF_EINVAL, std::string(e->name) + ": device pointer must be 16-byte aligned");
            dev = const_cast<void *>(e->user);
        } else if (e->user) {
            HIP_TRY(e->buf->reserve(e->bytes));
            if (e->upload) HIP_TRY(hipMemcpyAsync(e->buf->ptr, e->user, e->bytes, hipMemcpyHostToDevice, h->stream));
            dev = e->buf->ptr;
        }
        std::memcpy(e->slot, &dev, sizeof(dev));
    }
    return MAPF_OK;
}

// host mode: the outputs travel back (enqueued; the caller waits for the stream)
int fetch_arrays(mapf_handle_t h, const CallArray *arrays, size_t n) {
    if (h->device_ptrs) return MAPF_OK;
    for (const CallArray *e = arrays; e != arrays + n; ++e)
        if (e->user && e->download)
            HIP_TRY(hipMemcpyAsync(const_cast<void *>(e->user), e->buf->ptr, e->bytes, hipMemcpyDeviceToHost, h->stream));
    return MAPF_OK;
}
template <size_t N> int stage_arrays(mapf_handle_t h, const CallArray (&arrays)[N]) { return stage_arrays(h, arrays, N); }
template <size_t N> int fetch_arrays(mapf_handle_t h, const CallArray (&arrays)[N]) { return fetch_arrays(h, arrays, N); }

// a recorded launch: offset inside the recording + the device-side index (see StepArgs::t_dev)
template <typename Args> void fill_step_index(mapf_handle_t h, Args &a) { a.t = h->steps(); a.t_dev = h->capturing ? h->t_dev.ptr : nullptr; }

// The handle's part of an argument block.  What StepArgs, RolloutArgs and TransitionsArgs share by name -- the tables and the
// goals -- is all a query block takes ...
template <typename Args> Args query_args_from_handle(mapf_handle_t h) {
    Args a{};
    a.c = h->c; a.mv = h->mv; a.slip = h->slip_rows(); a.goal = h->goal; a.goal_broadcast = h->goal_broadcast;
    return a;
}
// ... a launch that moves the batch (StepArgs, RolloutArgs) also takes its state, its ids and the step index
template <typename Args> Args args_from_handle(mapf_handle_t h) {
    Args a = query_args_from_handle<Args>(h);
    a.mv4 = h->mv4; a.state = h->state; a.start = h->start; a.start_broadcast = h->start_broadcast;
    a.n_envs = h->E; a.env_id_offset = h->env_id_offset;
    fill_step_index(h, a);
    return a;
}

// after a state-changing launch of n steps: the kernel that took it, the step index, and may-be-terminal -- every finished
// episode is back on its start cells (auto-reset), or anything goes
void after_launch(mapf_handle_t h, std::string &last_kernel, uint64_t n_steps, bool auto_reset) {
    if (last_kernel != g_noted_kernel) last_kernel = g_noted_kernel;
    h->steps() += n_steps;
    if (n_steps) h->terminal_possible() = auto_reset ? h->start_terminal_any : true;
}

// (limit: the handle's episode limit, or null)
int launch_step_and_advance(mapf_handle_t h, const mapf::StepArgs &a, const mapf::EpisodeLimit *limit) {
    HIP_TRY(mapf::launch_step(int(h->A), a, h->tune, h->prefer, h->stream, limit));
    after_launch(h, h->last_step_kernel, 1, a.auto_reset);
    return MAPF_OK;
}
// The two mapf_debug_rollout_plan* entries (`who`: the one the shape message names): the null / shape checks, the tuning parse, and
// the plan the route gives a launch of that shape on a handle that prefers the lane-group family, without a table policy -- under an
// episode limit (max_steps != 0) the lane-group limit plan, else the packed one (zeros and 0 where no packed form applies)
int debug_rollout_plan(const char *who, uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int streamed, int delta_rows, int n_cu,
                       const char *tune, uint32_t max_steps, uint64_t out[6]) {
    if (!out) return fail(MAPF_EINVAL, "out is null");
    if (n_agents < 1 || n_cells < 2 || n_cu < 1) return fail(MAPF_EINVAL, std::string(who) + ": n_agents >= 1, n_cells >= 2, n_cu >= 1");
    std::string tune_error;
    const mapf::RolloutTuning t = mapf::rollout_tuning_for(n_cu, tune, &tune_error);
    if (!tune_error.empty()) return fail(MAPF_EINVAL, tune_error);
    // only the fields the plan reads: the shape, and which optional arrays are present (never dereferenced)
    static const uint8_t present = 0;
    mapf::RolloutArgs args{};
    args.c.n_cells = n_cells;
    args.n_envs = n_envs;
    args.n_steps = n_steps;
    args.actions = streamed ? &present : nullptr;
    args.mv_delta8 = delta_rows != 0;
    args.mv4 = delta_rows ? reinterpret_cast<const uint32_t *>(&present) : nullptr;
    const mapf::RolloutRoute r = mapf::route_rollout(n_agents, args, t, mapf::FamilyPreference::LaneGroup, false, 0u, max_steps != 0u, false);
    if (max_steps != 0u) {
        out[0] = 2; out[1] = uint64_t(r.lg.L); out[2] = r.lg.mv_lds ? 1 : 0;
        out[3] = r.lg.block; out[4] = r.lg.lds_bytes; out[5] = r.lg.grid;
        return 0;
    }
    out[0] = uint64_t(r.lq.K); out[1] = uint64_t(r.lq.Q); out[2] = uint64_t(int(r.lq.form));
    out[3] = r.lq.block; out[4] = r.lq.lds_bytes; out[5] = r.lq.lds_total;
    return r.family == mapf::KernelFamily::Packed ? 1 : 0;
}
}  // namespace

extern "C" {

const char *mapf_last_error(void) { return g_last_error.c_str(); }

const char *mapf_version(void) { return "mapf_hip 0.6.0 (abi 6, gfx950)"; }

int mapf_abi_version(void) { return MAPF_ABI_VERSION; }

int mapf_debug_rollout_plan(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int streamed, int delta_rows,
                            int n_cu, const char *tune, uint64_t out[6]) {
    return debug_rollout_plan("mapf_debug_rollout_plan", n_cells, n_agents, n_envs, n_steps, streamed, delta_rows, n_cu, tune, 0u, out);
}

int mapf_debug_rollout_plan_limited(uint32_t n_cells, int n_agents, uint64_t n_envs, uint32_t n_steps, int streamed, int delta_rows,
                                    int n_cu, const char *tune, uint32_t max_steps, uint64_t out[6]) {
    return debug_rollout_plan(max_steps ? "mapf_debug_rollout_plan_limited" : "mapf_debug_rollout_plan", n_cells, n_agents, n_envs, n_steps, streamed, delta_rows,
                              n_cu, tune, max_steps, out);
}

int mapf_device_count(int *out_count) {
    if (!out_count) return fail(MAPF_EINVAL, "out_count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out_count = 0; (void)hipGetLastError(); return fail(MAPF_ENODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *out_count = n;
    return MAPF_OK;
}

int mapf_create(const mapf_desc *d, mapf_handle_t *out_handle) {
    if (!d || !out_handle) return fail(MAPF_EINVAL, "null descriptor or output");
    *out_handle = nullptr;
    if (d->struct_size != sizeof(mapf_desc)) return fail(MAPF_EINVAL, "mapf_desc.struct_size does not match this library");
    if (d->n_cells == 0 || d->n_cells > 65536u) return fail(MAPF_EINVAL, "n_cells must be in 1..65536 (uint16 local ids)");
    if (d->n_agents == 0) return fail(MAPF_EINVAL, "n_agents must be >= 1");
    if (d->n_agents > MAPF_MAX_AGENTS) return fail(MAPF_EUNSUPPORTED, "n_agents beyond MAPF_MAX_AGENTS (128)");
    if ((d->flags & MAPF_FLAG_THREAD_PER_ENV) && (d->flags & MAPF_FLAG_LANE_GROUP))
        return fail(MAPF_EINVAL, "MAPF_FLAG_THREAD_PER_ENV and MAPF_FLAG_LANE_GROUP are exclusive");
    if ((d->flags & MAPF_FLAG_THREAD_PER_ENV) && d->n_agents > uint32_t(mapf::kTpeMaxAgents))
        return fail(MAPF_EUNSUPPORTED, "thread-per-env kernels exist for n_agents <= 16 only");
    if (d->criteria > MAPF_SOC) return fail(MAPF_EINVAL, "criteria must be MAPF_MAKESPAN or MAPF_SOC");
    if (!d->nbr || !d->start || !d->goal) return fail(MAPF_EINVAL, "nbr/start/goal must be non-null host pointers");
    if (!std::isfinite(d->fail_prob) || !std::isfinite(d->r_clash) || !std::isfinite(d->r_goal) || !std::isfinite(d->r_living))
        return fail(MAPF_EINVAL, "fail_prob and rewards must be finite");
    if (d->n_envs > (uint64_t(1) << 31)) return fail(MAPF_EINVAL, "n_envs too large for one handle");

    const uint32_t V = d->n_cells, A = d->n_agents;
    const uint64_t E = d->n_envs;
    const bool sb = d->flags & MAPF_FLAG_START_BROADCAST, gb = d->flags & MAPF_FLAG_GOAL_BROADCAST;
    for (uint64_t i = 0; i < uint64_t(V) * 5; ++i)
        if (d->nbr[i] >= V) return fail(MAPF_EINVAL, "nbr entry out of range");
    for (uint32_t v = 0; v < V; ++v)
        if (d->nbr[uint64_t(v) * 5] != v) return fail(MAPF_EINVAL, "nbr[v][STAY] must be v");
    const uint64_t n_start = (sb ? 1 : E) * A, n_goal = (gb ? 1 : E) * A;
    for (uint64_t i = 0; i < n_start; ++i)
        if (d->start[i] >= V) return fail(MAPF_EINVAL, "start cell out of range");
    for (uint64_t i = 0; i < n_goal; ++i)
        if (d->goal[i] >= V) return fail(MAPF_EINVAL, "goal cell out of range");

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return fail(MAPF_ENODEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                        "); this library has no CPU fallback");
    }
    if (d->device < 0 || d->device >= n_dev) return fail(MAPF_EINVAL, "device ordinal out of range");
    HIP_TRY(hipSetDevice(d->device));

    std::unique_ptr<mapf_handle_s> h(new (std::nothrow) mapf_handle_s());   // (a failure below tears down what exists so far)
    if (!h) return fail(MAPF_EHIP, "out of host memory");
    h->device = d->device; h->V = V; h->A = A; h->E = E; h->flags = d->flags;
    h->env_id_offset = d->env_id_offset; h->t = 0;
    h->start_broadcast = sb; h->goal_broadcast = gb;
    h->device_ptrs = d->flags & MAPF_FLAG_DEVICE_PTRS;
    if (d->flags & MAPF_FLAG_THREAD_PER_ENV) h->prefer = mapf::FamilyPreference::ThreadPerEnv;
    else if (d->flags & MAPF_FLAG_LANE_GROUP) h->prefer = mapf::FamilyPreference::LaneGroup;
    std::string error;
    h->tune = mapf::default_rollout_tuning(d->device, &error);
    if (!error.empty()) return fail(MAPF_EINVAL, error);

    // the host tables (mapf_tables.hip): table image, the move table in its three forms, the scenario table
    mapf::TableImage image;
    if (!mapf::build_slip_tables(d->fail_prob, image.slip, &h->c, &error)) return fail(MAPF_EINVAL, error);
    h->c.r_clash = d->r_clash; h->c.r_goal = d->r_goal; h->c.r_living = d->r_living;
    h->c.criteria = d->criteria; h->c.n_cells = V;
    h->c.seed_lo = uint32_t(d->seed); h->c.seed_hi = uint32_t(d->seed >> 32);
    const uint64_t pol = d->seed + 1;
    h->c.pol_lo = uint32_t(pol); h->c.pol_hi = uint32_t(pol >> 32);
    mapf::build_outcome_rows(h->c, image.outcome);
    const mapf::MoveTables moves = mapf::build_move_tables(d->nbr, V, d->fail_prob, image.slip);
    h->mv_delta8 = moves.delta8;
    h->nbr.assign(d->nbr, d->nbr + size_t(V) * 5);
    mapf::ScenTable scen;
    if (!(sb && gb) && E > 0 && h->tune.scen_table) scen = mapf::build_scen_table(d->start, sb, d->goal, gb, E, A);

    // allocate and upload
    if (d->stream) { h->stream = static_cast<hipStream_t>(d->stream); h->own_stream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    HIP_TRY(hipEventCreate(&h->ev_begin));
    HIP_TRY(hipEventCreate(&h->ev_end));
    HIP_TRY(h->mv.upload(moves.mv.data(), moves.mv.size()));
    HIP_TRY(h->mv8.upload(moves.mv8.data(), moves.mv8.size()));
    if (moves.delta8) HIP_TRY(h->mv4.upload(moves.mv4.data(), moves.mv4.size()));
    HIP_TRY(h->slip.upload(&image, 1));
    HIP_TRY(h->state.alloc((E ? E : 1) * A));
    HIP_TRY(h->start.alloc((sb ? 1 : (E ? E : 1)) * A));
    HIP_TRY(h->goal.alloc((gb ? 1 : (E ? E : 1)) * A));
    if (n_start) HIP_TRY(hipMemcpy(h->start, d->start, n_start * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (n_goal) HIP_TRY(hipMemcpy(h->goal, d->goal, n_goal * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(h->t_dev.alloc(1));
    HIP_TRY(hipMemset(h->t_dev, 0, sizeof(uint64_t)));
    HIP_TRY(h->age.alloc(E ? E : 1));
    HIP_TRY(hipMemset(h->age, 0, (E ? E : 1) * sizeof(uint32_t)));
    HIP_TRY(h->left.alloc(E ? E : 1));
    HIP_TRY(hipMemset(h->left, 0, (E ? E : 1) * sizeof(uint32_t)));
    if (scen.n) {
        h->n_scen = scen.n;
        HIP_TRY(h->scen.upload(scen.scen.data(), scen.scen.size()));
        HIP_TRY(h->scen_rows.upload(scen.rows.data(), scen.rows.size()));
    }

    HIP_TRY(mapf::launch_reset(int(A), h->state, h->start, sb, nullptr, E, h->stream));
    {   // is any env's start state terminal?  (the rollout kernels specialise on "no": state == start right now)
        std::vector<uint8_t> flags(E ? E : 1, 0);
        HIP_TRY(h->s_term.reserve(E ? E : 1));
        HIP_TRY(mapf::launch_query_terminal(int(A), h->state, h->goal, gb, static_cast<uint8_t *>(h->s_term.ptr), E, h->stream));
        if (E) HIP_TRY(hipMemcpyAsync(flags.data(), h->s_term.ptr, E, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->start_terminal_any = false;
        for (uint64_t e = 0; e < E; ++e) h->start_terminal_any |= flags[e] != 0;
        h->may_be_terminal = h->start_terminal_any;
    }
    *out_handle = h.release();
    return MAPF_OK;
}

int mapf_destroy(mapf_handle_t h) {
    if (!h) return fail(MAPF_EINVAL, "null handle");
    if (h->capturing) {   // an open recording dies with the handle
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(h->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        h->capturing = false;
    }
    delete h;
    return MAPF_OK;
}

int mapf_sync(mapf_handle_t h) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_sync")) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

const char *mapf_last_kernel(mapf_handle_t h, int which) {
    if (!h) return "";
    if (which == MAPF_KERNEL_TRANSITIONS) return h->last_transitions_kernel.c_str();
    return which == MAPF_KERNEL_ROLLOUT ? h->last_rollout_kernel.c_str() : h->last_step_kernel.c_str();
}

int mapf_get_stream(mapf_handle_t h, void **out_stream) {
    if (!h || !out_stream) return fail(MAPF_EINVAL, "null handle or output");
    *out_stream = static_cast<void *>(h->stream);
    h->stream_exposed = true;
    return MAPF_OK;
}

int mapf_timer_begin(mapf_handle_t h) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_timer_begin")) return rc;
    HIP_TRY(hipEventRecord(h->ev_begin, h->stream));
    return MAPF_OK;
}

int mapf_timer_end(mapf_handle_t h, double *out_ms) {
    if (int rc = check_handle(h)) return rc;
    if (!out_ms) return fail(MAPF_EINVAL, "out_ms is null");
    if (int rc = check_not_recording(h, "mapf_timer_end")) return rc;
    HIP_TRY(hipEventRecord(h->ev_end, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev_end));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_begin, h->ev_end));
    *out_ms = double(ms);
    return MAPF_OK;
}

int mapf_reset(mapf_handle_t h, const uint8_t *mask) {
    if (int rc = check_handle(h)) return rc;
    const uint8_t *d_mask = nullptr;
    const CallArray io[] = {input(h->s_mask, mask, size_t(h->E), &d_mask, "mask")};
    if (int rc = stage_arrays(h, io)) return rc;
    HIP_TRY(mapf::launch_reset(int(h->A), h->state, h->start, h->start_broadcast, d_mask, h->E, h->stream));
    if (h->episode_limit) HIP_TRY(mapf::launch_reset_ages(h->age, d_mask, h->E, h->stream));   // a reset env's episode begins again
    if (h->log_capacity) HIP_TRY(mapf::launch_reset_log_partials(h->log_partials(), d_mask, h->E, h->stream));   // ... and its running record is dropped
    if (!mask) h->terminal_possible() = h->start_terminal_any;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

namespace {
// mapf_step and mapf_step_limited (out_truncated: null from mapf_step)
int step_impl(mapf_handle_t h, const uint8_t *actions, const double *uniforms, uint16_t *out_local,
              double *out_reward, uint8_t *out_done, uint8_t *out_collision, double *out_prob,
              uint8_t *out_was_terminal, uint8_t *out_truncated, uint32_t step_flags) {
    if (int rc = check_handle(h)) return rc;
    if (!actions) return fail(MAPF_EINVAL, "actions is null");
    if (out_truncated && !h->episode_limit) return fail(MAPF_EINVAL, "step_limited: out_truncated on a handle without an episode limit (mapf_set_episode_limit)");
    if (h->episode_budget) return fail(MAPF_EUNSUPPORTED, "step: a handle with an episode budget takes fused rollouts only (mapf_set_episode_budget(h, 0) first)");
    if (step_flags & ~MAPF_STEP_AUTO_RESET) return fail(MAPF_EINVAL, "unknown step flag");
    if (int rc = check_foreign_capture(h, "mapf_step")) return rc;
    if (int rc = check_extent(h, h->E, uniforms != nullptr)) return rc;
    const size_t E = size_t(h->E), EA = E * h->A;
    mapf::StepArgs a = args_from_handle<mapf::StepArgs>(h);
    a.mv8 = h->mv8; a.scen = h->scen; a.scen_rows = h->scen_rows;
    a.auto_reset = step_flags & MAPF_STEP_AUTO_RESET;
    a.state_not_terminal = !h->terminal_possible();
    mapf::EpisodeLimit lim{h->age, h->episode_limit, nullptr, nullptr};
    const mapf::EpisodeLimit *limit = h->episode_limit ? &lim : nullptr;
    const CallArray io[] = {input(h->s_actions, actions, EA, &a.actions, "actions"), input(h->s_uniforms, uniforms, EA, &a.uniforms, "uniforms"),
                            output(h->s_local, out_local, EA, &a.out_local, "out_local"), output(h->s_reward, out_reward, E, &a.out_reward, "out_reward"),
                            output(h->s_prob, out_prob, E, &a.out_prob, "out_prob"), output(h->s_done, out_done, E, &a.out_done, "out_done"),
                            output(h->s_coll, out_collision, E, &a.out_collision, "out_collision"),
                            output(h->s_term, out_was_terminal, E, &a.out_was_terminal, "out_was_terminal"),
                            output(h->s_rtrunc, out_truncated, E, &lim.rec_truncated, "out_truncated")};
    if (!h->device_ptrs) {
        // tiny host-mode call: inputs and outputs live in one pinned, device-mapped block -- a 16-byte aligned slot per array
        // of the list (none for an absent one), then the flag word
        constexpr size_t n_io = sizeof(io) / sizeof(io[0]);
        const auto slot = [](size_t &off, size_t bytes) { const size_t at = off; off += (bytes + 15u) & ~size_t(15); return at; };
        size_t total = 0, at[n_io];
        for (size_t i = 0; i < n_io; ++i) at[i] = slot(total, io[i].user ? io[i].bytes : 0);
        const size_t o_flag = slot(total, sizeof(uint32_t));
        if (total <= kZeroCopyMaxBytes && E > 0) {
            HIP_TRY(h->pinned.reserve(kZeroCopyMaxBytes));
            char *hp = h->pinned.host, *dp = h->pinned.dev;
            for (size_t i = 0; i < n_io; ++i) {
                if (io[i].user && io[i].upload) std::memcpy(hp + at[i], io[i].user, io[i].bytes);
                void *dev = io[i].user ? dp + at[i] : nullptr;
                std::memcpy(io[i].slot, &dev, sizeof(dev));
            }
            const uint64_t launch_threads = mapf::step_is_thread_per_env(int(h->A), a, h->tune, h->prefer, limit) ? E : E * uint64_t(mapf::lg_group_size(int(h->A)));
            const bool flagged = launch_threads <= 64;             // one wave: see below
            const uint32_t seq = uint32_t(h->t) + 1u;
            if (flagged) {
                *reinterpret_cast<volatile uint32_t *>(hp + o_flag) = seq - 1u;
                a.done_flag = reinterpret_cast<uint32_t *>(dp + o_flag);
                a.done_seq = seq;
            }
            if (int rc = launch_step_and_advance(h, a, limit)) return rc;
            // A one-wave launch signals its end itself: its last instruction stores the call's sequence number into the
            // pinned block (system-scope release after all outputs), and the host spins on that word instead of paying the
            // sleeping stream wait (~6 us of a ~16 us call).  Anything larger, or a slow launch, uses hipStreamSynchronize.
            bool signalled = false;
            if (flagged) {
                volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(hp + o_flag);
                for (int spin = 0; spin < 200000 && !signalled; ++spin) signalled = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
            }
            if (!signalled) HIP_TRY(hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < n_io; ++i)
                if (io[i].user && io[i].download) std::memcpy(const_cast<void *>(io[i].user), hp + at[i], io[i].bytes);
            return MAPF_OK;
        }
    }
    if (int rc = stage_arrays(h, io)) return rc;
    if (int rc = launch_step_and_advance(h, a, limit)) return rc;
    if (int rc = fetch_arrays(h, io)) return rc;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}
}  // namespace

int mapf_step(mapf_handle_t h, const uint8_t *actions, const double *uniforms, uint16_t *out_local,
              double *out_reward, uint8_t *out_done, uint8_t *out_collision, double *out_prob,
              uint8_t *out_was_terminal, uint32_t step_flags) {
    return step_impl(h, actions, uniforms, out_local, out_reward, out_done, out_collision, out_prob, out_was_terminal, nullptr, step_flags);
}

int mapf_step_limited(mapf_handle_t h, const uint8_t *actions, const double *uniforms, uint16_t *out_local,
                      double *out_reward, uint8_t *out_done, uint8_t *out_collision, double *out_prob,
                      uint8_t *out_was_terminal, uint8_t *out_truncated, uint32_t step_flags) {
    return step_impl(h, actions, uniforms, out_local, out_reward, out_done, out_collision, out_prob, out_was_terminal, out_truncated, step_flags);
}

namespace {
// The recording rollout kernels write all five trajectory arrays (no per-array branches in the step loop): when
// the caller asked for only some of them, the others go to handle-owned scratch.
// A stand-in buffer that a RECORDED rollout node names must not move: DeviceBuf::reserve() frees and reallocates on growth,
// and the next replay of that node would write into freed memory.  So while a graph is being recorded or recorded graphs
// of the handle are alive, a stand-in may be allocated (nothing names it yet) but not grown.
int reserve_stand_in(mapf_handle_t h, DeviceBuf &buf, size_t bytes, const char *name) {
    if (buf.ptr && bytes > buf.cap && (h->capturing || !h->graphs.empty()))
        return fail(MAPF_EINVAL, std::string("rollout: the handle's stand-in for ") + name + " would have to grow while a recorded graph names it -- pass all "
                                 "five rec_* arrays, record the longest rollout first, or destroy the handle's graphs");
    HIP_TRY(buf.reserve(bytes));
    return MAPF_OK;
}
int complete_recording(mapf_handle_t h, mapf::RolloutArgs &a, size_t TE, size_t TEA) {
    if (!(a.rec_local || a.rec_reward || a.rec_prob || a.rec_done || a.rec_collision)) return MAPF_OK;
    const struct { void *field; DeviceBuf *buf; size_t bytes; const char *name; } rows[] = {
        {&a.rec_local, &h->x_local, TEA * sizeof(uint16_t), "rec_local"}, {&a.rec_reward, &h->x_reward, TE * sizeof(double), "rec_reward"},
        {&a.rec_prob, &h->x_prob, TE * sizeof(double), "rec_prob"}, {&a.rec_done, &h->x_done, TE, "rec_done"},
        {&a.rec_collision, &h->x_coll, TE, "rec_collision"}};
    for (const auto &r : rows) {
        void *given = nullptr;
        std::memcpy(&given, r.field, sizeof(given));   // (typed pointer fields: memcpy, where a void ** cast would alias)
        if (given) continue;
        if (int rc = reserve_stand_in(h, *r.buf, r.bytes, r.name)) return rc;
        std::memcpy(r.field, &r.buf->ptr, sizeof(void *));
    }
    return MAPF_OK;
}
}  // namespace

namespace {
// mapf_rollout, mapf_rollout_limited and mapf_rollout_budgeted (out_truncations, rec_truncated: null from mapf_rollout; out_live_steps:
// null from both)
int rollout_impl(mapf_handle_t h, const mapf_rollout_io *io, uint32_t *out_truncations, uint8_t *rec_truncated, uint32_t *out_live_steps) {
    if (int rc = check_handle(h)) return rc;
    if (!io || io->struct_size != sizeof(mapf_rollout_io)) return fail(MAPF_EINVAL, "bad mapf_rollout_io");
    if (io->step_flags & ~MAPF_STEP_AUTO_RESET) return fail(MAPF_EINVAL, "unknown step flag");
    if ((out_truncations || rec_truncated) && !h->episode_limit)
        return fail(MAPF_EINVAL, "rollout_limited: out_truncations / rec_truncated on a handle without an episode limit (mapf_set_episode_limit)");
    if (out_live_steps && !h->episode_budget)
        return fail(MAPF_EINVAL, "rollout_budgeted: out_live_steps on a handle without an episode budget (mapf_set_episode_budget)");
    if (h->episode_budget && !(io->step_flags & MAPF_STEP_AUTO_RESET))
        return fail(MAPF_EINVAL, "rollout: step_flags without MAPF_STEP_AUTO_RESET on a handle with an episode budget (mapf_set_episode_budget)");
    if (int rc = check_foreign_capture(h, "mapf_rollout")) return rc;
    if (int rc = check_extent(h, uint64_t(h->E) * io->n_steps, false)) return rc;
    const size_t E = size_t(h->E), T = io->n_steps, TE = T * E, TEA = TE * h->A;
    mapf::RolloutArgs a = args_from_handle<mapf::RolloutArgs>(h);
    a.n_steps = io->n_steps;
    a.policy_cells = h->policy_cells;
    // (the table policy travels beside the argument block: its kernels are instances of their own; streamed actions take
    // precedence over it, as over the other policies -- the ONE place that rule is applied: no launcher sees both)
    const mapf::TablePolicy *table = (h->table.table && !io->actions) ? &h->table : nullptr;
    const mapf::JointPolicy *joint = (h->joint.table && !io->actions) ? &h->joint : nullptr;   // (the joint table policy likewise)
    const mapf::GroupPolicy *group = (h->group.table && !io->actions) ? &h->group : nullptr;   // (and the group policy)
    a.auto_reset = io->step_flags & MAPF_STEP_AUTO_RESET;
    a.accumulate = io->accumulate != 0;
    a.start_terminal_any = h->start_terminal_any;
    a.mv_delta8 = h->mv_delta8;
    // (the episode limit travels beside the argument block too: its kernels are the lane-group family's limit instances -- and the
    // packed table instances' where the handle's tuning opts into them: the route picks, as it does without a limit)
    // (... and the episode budget beside the limit: its kernels are the lane-group family's budget instances, which take the limit
    // block too -- with max_steps 0 on a handle without a limit)
    mapf::EpisodeLimit lim{h->age, h->episode_limit, nullptr, nullptr};
    mapf::EpisodeBudget bud{h->left, nullptr};
    const mapf::EpisodeBudget *budget = h->episode_budget ? &bud : nullptr;
    const mapf::EpisodeLimit *limit = (h->episode_limit || budget) ? &lim : nullptr;
    // (... and the conflict matrix last: the lane-group instances that count, in the form the limit and the budget name)
    const mapf::ConflictPairs cp{h->pair_counts, h->pair_slot_of_env, h->pair_slots};
    const mapf::ConflictPairs *pairs = h->pair_slots ? &cp : nullptr;
    // (... and the episode log beside the budget: the lane-group budget instances that keep one)
    const mapf::EpisodeLog lg{h->log_partials(), h->log_records, h->log_capacity};
    const mapf::EpisodeLog *log = (h->log_capacity && budget) ? &lg : nullptr;
    // (the totals are inputs too when the call accumulates)
    const CallArray arrays[] = {input(h->s_actions, io->actions, TEA, &a.actions, "actions"),
                                output(h->s_ret, io->out_returns, E, &a.out_returns, "out_returns", a.accumulate),
                                output(h->s_epi, io->out_episodes, E, &a.out_episodes, "out_episodes", a.accumulate),
                                output(h->s_ncoll, io->out_collisions, E, &a.out_collisions, "out_collisions", a.accumulate),
                                output(h->s_local, io->rec_local, TEA, &a.rec_local, "rec_local"), output(h->s_reward, io->rec_reward, TE, &a.rec_reward, "rec_reward"),
                                output(h->s_prob, io->rec_prob, TE, &a.rec_prob, "rec_prob"), output(h->s_done, io->rec_done, TE, &a.rec_done, "rec_done"),
                                output(h->s_coll, io->rec_collision, TE, &a.rec_collision, "rec_collision"),
                                output(h->s_trunc, out_truncations, E, &lim.out_truncations, "out_truncations", a.accumulate),
                                output(h->s_rtrunc, rec_truncated, TE, &lim.rec_truncated, "rec_truncated"),
                                output(h->s_live, out_live_steps, E, &bud.out_live_steps, "out_live_steps", a.accumulate)};
    if (int rc = stage_arrays(h, arrays)) return rc;
    if (limit && lim.rec_truncated && !a.rec_local) {   // the truncated bytes alone make the launch a recording one
        if (int rc = reserve_stand_in(h, h->x_local, TEA * sizeof(uint16_t), "rec_local")) return rc;
        a.rec_local = static_cast<uint16_t *>(h->x_local.ptr);
    }
    if (int rc = complete_recording(h, a, TE, TEA)) return rc;
    if (limit && a.rec_local && !lim.rec_truncated) {   // ... and a recording limit launch writes them: a stand-in when absent
        if (int rc = reserve_stand_in(h, h->x_trunc, TE, "rec_truncated")) return rc;
        lim.rec_truncated = static_cast<uint8_t *>(h->x_trunc.ptr);
    }
    HIP_TRY(mapf::launch_rollout(int(h->A), a, h->tune, h->prefer, h->stream, table, limit, budget, pairs, joint, log, group));
    after_launch(h, h->last_rollout_kernel, io->n_steps, a.auto_reset);
    if (int rc = fetch_arrays(h, arrays)) return rc;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

}  // namespace

int mapf_rollout(mapf_handle_t h, const mapf_rollout_io *io) { return rollout_impl(h, io, nullptr, nullptr, nullptr); }

int mapf_rollout_limited(mapf_handle_t h, const mapf_rollout_io *io, uint32_t *out_truncations, uint8_t *rec_truncated) {
    return rollout_impl(h, io, out_truncations, rec_truncated, nullptr);
}

int mapf_rollout_budgeted(mapf_handle_t h, const mapf_rollout_io *io, uint32_t *out_truncations, uint8_t *rec_truncated, uint32_t *out_live_steps) {
    return rollout_impl(h, io, out_truncations, rec_truncated, out_live_steps);
}

int mapf_set_conflict_pairs(mapf_handle_t h, uint32_t n_slots, const uint32_t *slot_of_env) {
    if (!h) return fail(MAPF_EINVAL, "set_conflict_pairs: null handle");
    if (int rc = check_not_recording(h, "mapf_set_conflict_pairs")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_conflict_pairs: recorded graphs hold launches without a conflict matrix (destroy them first)");
    const uint64_t entries = uint64_t(n_slots) * h->A * h->A;
    if (entries * sizeof(uint64_t) > (uint64_t(1) << 30)) return fail(MAPF_EINVAL, "set_conflict_pairs: n_slots * A * A * 8 bytes must not exceed 2^30");
    if (n_slots && slot_of_env)
        for (uint64_t e = 0; e < h->E; ++e)
            if (slot_of_env[e] >= n_slots) return fail(MAPF_EINVAL, "set_conflict_pairs: slot_of_env[" + std::to_string(e) + "] is not below n_slots");
    if (int rc = check_handle(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // (no launch may still count into what is freed here)
    h->pair_slots = 0;
    h->pair_counts.reset();
    h->pair_slot_of_env.reset();
    if (n_slots == 0) return MAPF_OK;
    HIP_TRY(h->pair_counts.alloc(size_t(entries)));
    if (slot_of_env && h->E) HIP_TRY(h->pair_slot_of_env.upload(slot_of_env, size_t(h->E)));
    HIP_TRY(hipMemsetAsync(h->pair_counts, 0, size_t(entries) * sizeof(uint64_t), h->stream));   // every call: counts from zero
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->pair_slots = n_slots;
    return MAPF_OK;
}

int mapf_conflict_pairs(mapf_handle_t h, uint64_t *out, int zero) {
    if (!h) return fail(MAPF_EINVAL, "conflict_pairs: null handle");
    if (!out && !zero) return fail(MAPF_EINVAL, "conflict_pairs: out is null and zero is 0");
    if (!h->pair_slots) return fail(MAPF_EINVAL, "conflict_pairs: the handle has no conflict matrix (mapf_set_conflict_pairs)");
    if (int rc = check_not_recording(h, "mapf_conflict_pairs")) return rc;
    if (h->device_ptrs && misaligned(out)) return fail(MAPF_EINVAL, "conflict_pairs: device pointer must be 16-byte aligned");
    if (int rc = check_handle(h)) return rc;
    const size_t bytes = h->pair_bytes();
    // (out receives the counts as they are before they are zeroed)
    if (out && bytes) HIP_TRY(hipMemcpyAsync(out, h->pair_counts, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (zero && bytes) HIP_TRY(hipMemsetAsync(h->pair_counts, 0, bytes, h->stream));
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_set_episode_budget(mapf_handle_t h, uint32_t n_episodes) {
    if (!h) return fail(MAPF_EINVAL, "set_episode_budget: null handle");
    if (int rc = check_not_recording(h, "mapf_set_episode_budget")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_episode_budget: recorded graphs hold launches without a budget (destroy them first)");
    if (n_episodes == 0 && h->log_capacity) return fail(MAPF_EINVAL, "set_episode_budget: the handle keeps an episode log, which needs a budget (mapf_set_episode_log(h, 0) first)");
    if (int rc = check_handle(h)) return rc;
    // every call re-arms every env: left[e] = n_episodes (state and ages stay)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->left.ptr), int(n_episodes), h->E ? size_t(h->E) : 1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->episode_budget = n_episodes;
    return MAPF_OK;
}

int mapf_set_episode_log(mapf_handle_t h, uint32_t capacity) {
    if (!h) return fail(MAPF_EINVAL, "set_episode_log: null handle");
    if (int rc = check_not_recording(h, "mapf_set_episode_log")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_episode_log: recorded graphs hold launches without an episode log (destroy them first)");
    if (capacity && !h->episode_budget) return fail(MAPF_EINVAL, "set_episode_log: a handle without an episode budget (mapf_set_episode_budget first)");
    if (uint64_t(h->E) * capacity * sizeof(mapf_episode_record) > (uint64_t(1) << 31))
        return fail(MAPF_EINVAL, "set_episode_log: E * capacity * 16 bytes must not exceed 2^31");
    if (int rc = check_handle(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // (no launch may still log into what is freed here)
    h->log_capacity = 0;
    h->log_heads.reset();
    h->log_records.reset();
    if (capacity == 0) return MAPF_OK;
    const size_t E = size_t(h->E), head_words = (E * (sizeof(mapf::EpisodeLogPartial) + sizeof(uint32_t)) + 15u) / 16u, record_words = E * capacity;
    HIP_TRY(h->log_heads.alloc(head_words ? head_words : 1));
    HIP_TRY(h->log_records.alloc(record_words ? record_words : 1));
    // every call: no episode running, none counted, no record
    HIP_TRY(hipMemsetAsync(h->log_heads, 0, (head_words ? head_words : 1) * sizeof(uint4), h->stream));
    HIP_TRY(hipMemsetAsync(h->log_records, 0, (record_words ? record_words : 1) * sizeof(uint4), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->log_capacity = capacity;
    return MAPF_OK;
}

int mapf_episode_log(mapf_handle_t h, mapf_episode_record *out_records, uint32_t *out_count, int clear) {
    if (!h) return fail(MAPF_EINVAL, "episode_log: null handle");
    if (!out_records && !out_count && !clear) return fail(MAPF_EINVAL, "episode_log: out_records and out_count are null and clear is 0");
    if (!h->log_capacity) return fail(MAPF_EINVAL, "episode_log: the handle has no episode log (mapf_set_episode_log)");
    if (int rc = check_not_recording(h, "mapf_episode_log")) return rc;
    if (h->device_ptrs && (misaligned(out_records) || misaligned(out_count))) return fail(MAPF_EINVAL, "episode_log: device pointer must be 16-byte aligned");
    if (int rc = check_handle(h)) return rc;
    const size_t record_bytes = h->log_record_bytes(), count_bytes = size_t(h->E) * sizeof(uint32_t);
    const hipMemcpyKind kind = h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    // (the outputs receive the log as it is before it is cleared; the partials -- the running episodes -- stay)
    if (out_records && record_bytes) HIP_TRY(hipMemcpyAsync(out_records, h->log_records, record_bytes, kind, h->stream));
    if (out_count && count_bytes) HIP_TRY(hipMemcpyAsync(out_count, h->log_counts(), count_bytes, kind, h->stream));
    if (clear && record_bytes) HIP_TRY(hipMemsetAsync(h->log_records, 0, record_bytes, h->stream));
    if (clear && count_bytes) HIP_TRY(hipMemsetAsync(h->log_counts(), 0, count_bytes, h->stream));
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_episodes_left(mapf_handle_t h, uint32_t *out_left, const uint32_t *set_left) {
    if (!h) return fail(MAPF_EINVAL, "episodes_left: null handle");
    if (!out_left && !set_left) return fail(MAPF_EINVAL, "episodes_left: out_left and set_left are both null");
    if (set_left && !h->episode_budget) return fail(MAPF_EINVAL, "episodes_left: set_left on a handle without an episode budget (mapf_set_episode_budget)");
    if (int rc = check_not_recording(h, "mapf_episodes_left")) return rc;
    if (h->device_ptrs && (misaligned(out_left) || misaligned(set_left))) return fail(MAPF_EINVAL, "episodes_left: device pointer must be 16-byte aligned");
    if (int rc = check_handle(h)) return rc;
    const size_t bytes = size_t(h->E) * sizeof(uint32_t);
    // (out_left receives the counts as they are before set_left replaces them)
    if (out_left && bytes) HIP_TRY(hipMemcpyAsync(out_left, h->left, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (set_left && bytes) HIP_TRY(hipMemcpyAsync(h->left, set_left, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_set_episode_limit(mapf_handle_t h, uint32_t max_steps) {
    if (!h) return fail(MAPF_EINVAL, "set_episode_limit: null handle");
    if (int rc = check_not_recording(h, "mapf_set_episode_limit")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_episode_limit: recorded graphs hold launches without a limit (destroy them first)");
    if (int rc = check_handle(h)) return rc;
    HIP_TRY(hipMemsetAsync(h->age, 0, (h->E ? size_t(h->E) : 1) * sizeof(uint32_t), h->stream));   // every call: new episodes
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->episode_limit = max_steps;
    return MAPF_OK;
}

int mapf_episode_steps(mapf_handle_t h, uint32_t *out_age, const uint32_t *set_age) {
    if (!h) return fail(MAPF_EINVAL, "episode_steps: null handle");
    if (!out_age && !set_age) return fail(MAPF_EINVAL, "episode_steps: out_age and set_age are both null");
    if (set_age && !h->episode_limit) return fail(MAPF_EINVAL, "episode_steps: set_age on a handle without an episode limit (mapf_set_episode_limit)");
    if (int rc = check_not_recording(h, "mapf_episode_steps")) return rc;
    if (h->device_ptrs && (misaligned(out_age) || misaligned(set_age))) return fail(MAPF_EINVAL, "episode_steps: device pointer must be 16-byte aligned");
    if (int rc = check_handle(h)) return rc;
    const size_t bytes = size_t(h->E) * sizeof(uint32_t);
    // (out_age receives the ages as they are before set_age replaces them)
    if (out_age && bytes) HIP_TRY(hipMemcpyAsync(out_age, h->age, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (set_age && bytes) HIP_TRY(hipMemcpyAsync(h->age, set_age, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_set_policy_table(mapf_handle_t h, const uint8_t *table, uint32_t n_rows, const uint16_t *row_index, uint32_t flags) {
    if (!h) return fail(MAPF_EINVAL, "set_policy_table: null handle");
    if (!table) return fail(MAPF_EINVAL, "set_policy_table: table is null");
    if (!row_index) return fail(MAPF_EINVAL, "set_policy_table: row_index is null");
    if (n_rows == 0 || n_rows > 65536u) return fail(MAPF_EINVAL, "set_policy_table: n_rows must be 1..65536");
    if (flags & ~MAPF_POLICY_ROWS_BROADCAST) return fail(MAPF_EINVAL, "set_policy_table: unknown bits in flags");
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_set_policy")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_policy: recorded graphs hold the current policy table (destroy them first)");
    const uint64_t bytes = uint64_t(n_rows) * h->V;
    if (bytes > 0x7FFFFFFFull) return fail(MAPF_EINVAL, "set_policy_table: table (n_rows * V bytes) exceeds 2 GiB");
    // the kernels index the move table with these bytes unclamped: every one is checked here
    for (uint64_t i = 0; i < bytes; ++i)
        if (table[i] > 4u)
            return fail(MAPF_EINVAL, "set_policy_table: table[" + std::to_string(i) + "] = " + std::to_string(unsigned(table[i])) + " is not an action (0..4)");
    const bool broadcast = (flags & MAPF_POLICY_ROWS_BROADCAST) != 0u;
    const uint64_t n_index = broadcast ? uint64_t(h->A) : uint64_t(h->E) * h->A;
    for (uint64_t i = 0; i < n_index; ++i)
        if (row_index[i] >= n_rows)
            return fail(MAPF_EINVAL, "set_policy_table: row_index[" + std::to_string(i) + "] = " + std::to_string(unsigned(row_index[i])) + " is not below n_rows");
    HIP_TRY(hipStreamSynchronize(h->stream));   // no launch may still be reading the old copies
    h->drop_policy_table();
    h->drop_policy_joint();
    h->drop_policy_group();
    h->policy_cells.reset();   // (one policy at a time)
    // the table's allocation is padded to whole 16-byte words (the LDS form stages it sixteen bytes at a time); the row indices
    // by one agent row (the packed kernels load an agent pair's two indices as one word)
    const size_t padded = (size_t(bytes) + 15u) & ~size_t(15), n_rows_padded = size_t(n_index) + 16u;
    DevicePtr<uint8_t> d_table;
    DevicePtr<uint16_t> d_rows;
    HIP_TRY(d_table.alloc(padded));
    if (hipError_t e = d_rows.alloc(n_rows_padded)) return hip_fail(e, "hipMalloc");
    hipError_t e = hipMemset(d_table, 0, padded);
    if (e == hipSuccess) e = hipMemset(d_rows, 0, n_rows_padded * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d_table, table, size_t(bytes), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rows, row_index, size_t(n_index) * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "set_policy_table: copying the table");
    h->table_bytes = std::move(d_table);
    h->table_rows = std::move(d_rows);
    h->table.table = h->table_bytes;
    h->table.rows = h->table_rows;
    h->table.table_bytes = uint32_t(bytes);
    h->table.rows_broadcast = broadcast ? 1u : 0u;
    return MAPF_OK;
}

int mapf_set_policy_joint(mapf_handle_t h, const uint8_t *table, uint64_t table_bytes, const uint32_t *offset, const uint16_t *partner, uint32_t flags) {
    if (!h) return fail(MAPF_EINVAL, "set_policy_joint: null handle");
    if (!table) return fail(MAPF_EINVAL, "set_policy_joint: table is null");
    if (!offset) return fail(MAPF_EINVAL, "set_policy_joint: offset is null");
    if (!partner) return fail(MAPF_EINVAL, "set_policy_joint: partner is null");
    if (table_bytes == 0 || table_bytes > 0x7FFFFFFFull) return fail(MAPF_EINVAL, "set_policy_joint: table_bytes must be 1..2^31-1");
    if (flags & ~MAPF_POLICY_ROWS_BROADCAST) return fail(MAPF_EINVAL, "set_policy_joint: unknown bits in flags");
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_set_policy")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_policy: recorded graphs hold the current policy table (destroy them first)");
    // the kernels index the move table with these bytes unclamped, and the policy table with offset + cell * V + cell: all checked here
    for (uint64_t i = 0; i < table_bytes; ++i)
        if (table[i] > 4u)
            return fail(MAPF_EINVAL, "set_policy_joint: table[" + std::to_string(i) + "] = " + std::to_string(unsigned(table[i])) + " is not an action (0..4)");
    const bool broadcast = (flags & MAPF_POLICY_ROWS_BROADCAST) != 0u;
    const uint64_t A = h->A, V = h->V, n_index = broadcast ? A : uint64_t(h->E) * A;
    for (uint64_t i = 0; i < n_index; ++i) {
        const uint64_t row = i - i % A, me = i % A, other = partner[i];
        if (other >= A)
            return fail(MAPF_EINVAL, "set_policy_joint: partner[" + std::to_string(i) + "] = " + std::to_string(other) + " is not below n_agents");
        if (partner[row + other] != me)
            return fail(MAPF_EINVAL, "set_policy_joint: partner[" + std::to_string(i) + "] = " + std::to_string(other) + " but partner[" + std::to_string(row + other) +
                                         "] = " + std::to_string(unsigned(partner[row + other])) + ": the merge is not mutual");
        const uint64_t segment = other == me ? V : V * V;
        if (uint64_t(offset[i]) + segment > table_bytes)
            return fail(MAPF_EINVAL, "set_policy_joint: offset[" + std::to_string(i) + "] = " + std::to_string(offset[i]) + ": the segment of " + std::to_string(segment) +
                                         " bytes ends past table_bytes");
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // no launch may still be reading the old copies
    // the allocations are padded as the table policy's are: the table to whole 16-byte words, the index arrays by one agent row
    const size_t padded = (size_t(table_bytes) + 15u) & ~size_t(15), n_padded = size_t(n_index) + 16u;
    DevicePtr<uint8_t> d_table;
    DevicePtr<uint32_t> d_offset;
    DevicePtr<uint16_t> d_partner;
    HIP_TRY(d_table.alloc(padded));
    if (hipError_t e = d_offset.alloc(n_padded)) return hip_fail(e, "hipMalloc");
    if (hipError_t e = d_partner.alloc(n_padded)) return hip_fail(e, "hipMalloc");
    hipError_t e = hipMemset(d_table, 0, padded);
    if (e == hipSuccess) e = hipMemset(d_offset, 0, n_padded * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_partner, 0, n_padded * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d_table, table, size_t(table_bytes), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_offset, offset, size_t(n_index) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_partner, partner, size_t(n_index) * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "set_policy_joint: copying the table");   // (the previous policy stays in force)
    h->drop_policy_table();    // (one policy at a time)
    h->drop_policy_joint();
    h->drop_policy_group();
    h->policy_cells.reset();
    h->joint_bytes = std::move(d_table);
    h->joint_offset = std::move(d_offset);
    h->joint_partner = std::move(d_partner);
    h->joint.table = h->joint_bytes;
    h->joint.offset = h->joint_offset;
    h->joint.partner = h->joint_partner;
    h->joint.table_bytes = uint32_t(table_bytes);
    h->joint.broadcast = broadcast ? 1u : 0u;
    return MAPF_OK;
}

// what mapf_set_policy_group and mapf_debug_policy_group share: the pointer and range checks that need no handle, the header's rules
// about the arrays, and the table of all books -- all on the host
static int group_plan_checked(const mapf::GroupPlanArrays &g, uint32_t flags, mapf::GroupTable *built) {
    if (!g.table) return fail(MAPF_EINVAL, "set_policy_group: table is null");
    if (!g.row_index) return fail(MAPF_EINVAL, "set_policy_group: row_index is null");
    if (!g.members) return fail(MAPF_EINVAL, "set_policy_group: members is null");
    if (!g.book) return fail(MAPF_EINVAL, "set_policy_group: book is null");
    if (!g.entries && !(g.n_entries == 0 && g.n_books == 0)) return fail(MAPF_EINVAL, "set_policy_group: entries is null (allowed only with n_entries == 0 and n_books == 0)");
    if (!g.book_begin && !(g.n_entries == 0 && g.n_books == 0)) return fail(MAPF_EINVAL, "set_policy_group: book_begin is null (allowed only with n_entries == 0 and n_books == 0)");
    if (flags & ~MAPF_POLICY_ROWS_BROADCAST) return fail(MAPF_EINVAL, "set_policy_group: unknown bits in flags");
    if (g.V > 65535u) return fail(MAPF_EUNSUPPORTED, "set_policy_group: the mode needs V <= 65535 (cell 0xFFFF is the padding of keys)");
    std::string error;
    if (!mapf::validate_group_plan(g, &error)) return fail(MAPF_EINVAL, error);
    if (!mapf::build_group_table(reinterpret_cast<const mapf::GroupEntry *>(g.entries), g.n_entries, g.book_begin, g.n_books, built, &error)) return fail(MAPF_EINVAL, error);
    return MAPF_OK;
}

int mapf_set_policy_group(mapf_handle_t h, const uint8_t *table, uint32_t n_rows, const uint16_t *row_index, const uint16_t *members, const uint32_t *book,
                          const mapf_group_entry *entries, uint64_t n_entries, const uint32_t *book_begin, uint32_t n_books, uint32_t flags) {
    static_assert(sizeof(mapf_group_entry) == sizeof(mapf::GroupEntry) && sizeof(mapf_group_entry) == 12, "one layout");
    if (!h) return fail(MAPF_EINVAL, "set_policy_group: null handle");
    mapf::GroupPlanArrays g;
    g.table = table; g.n_rows = n_rows; g.row_index = row_index; g.members = members; g.book = book;
    g.entries = reinterpret_cast<const mapf::GroupEntry *>(entries); g.n_entries = n_entries; g.book_begin = book_begin; g.n_books = n_books;
    g.broadcast = (flags & MAPF_POLICY_ROWS_BROADCAST) != 0u;
    if (!table || !row_index || !members || !book || (flags & ~MAPF_POLICY_ROWS_BROADCAST)) return group_plan_checked(g, flags, nullptr);   // (fails before the handle is read)
    g.V = h->V; g.A = h->A; g.E = h->E;
    if (int rc = check_not_recording(h, "mapf_set_policy")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_policy: recorded graphs hold the current policy table (destroy them first)");
    mapf::GroupTable built;
    if (int rc = group_plan_checked(g, flags, &built)) return rc;   // all of it on the host, before any device work
    if (int rc = check_handle(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));   // no launch may still be reading the old copies
    // the allocations are padded as the table policy's are: the table to whole 16-byte words, the index arrays by one agent row
    const uint64_t bytes = uint64_t(n_rows) * h->V, n_index = g.broadcast ? uint64_t(h->A) : uint64_t(h->E) * h->A;
    const size_t padded = (size_t(bytes) + 15u) & ~size_t(15), n_padded = size_t(n_index) + 16u;
    DevicePtr<uint8_t> d_table;
    DevicePtr<uint16_t> d_rows, d_members;
    DevicePtr<uint32_t> d_book;
    DevicePtr<mapf::GroupSlot> d_slots;
    HIP_TRY(d_table.alloc(padded));
    if (hipError_t e = d_rows.alloc(n_padded)) return hip_fail(e, "hipMalloc");
    if (hipError_t e = d_members.alloc(n_padded * 4u)) return hip_fail(e, "hipMalloc");
    if (hipError_t e = d_book.alloc(n_padded)) return hip_fail(e, "hipMalloc");
    if (hipError_t e = d_slots.alloc(built.slots.size())) return hip_fail(e, "hipMalloc");
    hipError_t e = hipMemset(d_table, 0, padded);
    if (e == hipSuccess) e = hipMemset(d_rows, 0, n_padded * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemset(d_members, 0xFF, n_padded * 4u * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemset(d_book, 0, n_padded * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_table, table, size_t(bytes), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rows, row_index, size_t(n_index) * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_members, members, size_t(n_index) * 4u * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_book, book, size_t(n_index) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_slots, built.slots.data(), built.slots.size() * sizeof(mapf::GroupSlot), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "set_policy_group: copying the plan");   // (the previous policy stays in force)
    h->drop_policy_table();    // (one policy at a time)
    h->drop_policy_joint();
    h->drop_policy_group();
    h->policy_cells.reset();
    h->group_bytes = std::move(d_table);
    h->group_rows = std::move(d_rows);
    h->group_members = std::move(d_members);
    h->group_book = std::move(d_book);
    h->group_slots = std::move(d_slots);
    h->group.table = h->group_bytes;
    h->group.rows = h->group_rows;
    h->group.members = h->group_members;
    h->group.book = h->group_book;
    h->group.slots = h->group_slots;
    h->group.mask = uint32_t(built.slots.size() - 1u);
    h->group.max_probe = built.max_probe;
    h->group.broadcast = g.broadcast ? 1u : 0u;
    return MAPF_OK;
}

int mapf_policy_group_stats(mapf_handle_t h, uint64_t *slots, uint32_t *max_probe) {
    if (!h) return fail(MAPF_EINVAL, "policy_group_stats: null handle");
    if (!h->group.table) return fail(MAPF_EINVAL, "policy_group_stats: the handle is not under the group policy (mapf_set_policy_group)");
    if (slots) *slots = uint64_t(h->group.mask) + 1u;
    if (max_probe) *max_probe = h->group.max_probe;
    return MAPF_OK;
}

int mapf_debug_policy_group(uint32_t n_cells, uint32_t n_agents, uint64_t n_envs, const uint8_t *table, uint32_t n_rows, const uint16_t *row_index,
                            const uint16_t *members, const uint32_t *book, const mapf_group_entry *entries, uint64_t n_entries, const uint32_t *book_begin,
                            uint32_t n_books, uint32_t flags, uint64_t n_keys, const uint16_t *key_cells, const uint32_t *key_book, uint32_t *out_actions,
                            uint32_t *out_probes, uint64_t *out_slots, uint32_t *out_max_probe) {
    mapf::GroupPlanArrays g;
    g.V = n_cells; g.A = n_agents; g.E = n_envs;
    g.table = table; g.n_rows = n_rows; g.row_index = row_index; g.members = members; g.book = book;
    g.entries = reinterpret_cast<const mapf::GroupEntry *>(entries); g.n_entries = n_entries; g.book_begin = book_begin; g.n_books = n_books;
    g.broadcast = (flags & MAPF_POLICY_ROWS_BROADCAST) != 0u;
    if (n_agents < 1 || n_agents > MAPF_MAX_AGENTS) return fail(MAPF_EINVAL, "debug_policy_group: n_agents must be 1..MAPF_MAX_AGENTS");
    if (n_keys != 0 && (!key_cells || !key_book || !out_actions)) return fail(MAPF_EINVAL, "debug_policy_group: key_cells, key_book or out_actions is null");
    mapf::GroupTable built;
    if (int rc = group_plan_checked(g, flags, &built)) return rc;
    if (out_slots) *out_slots = built.slots.size();
    if (out_max_probe) *out_max_probe = built.max_probe;
    for (uint64_t k = 0; k < n_keys; ++k) {
        uint32_t probes = 0;
        out_actions[k] = mapf::lookup_group_table(built, key_cells + 4u * k, key_book[k], &probes);
        if (out_probes) out_probes[k] = probes;
    }
    return MAPF_OK;
}

int mapf_set_policy(mapf_handle_t h, int policy, const uint32_t *cell_rc) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_set_policy")) return rc;
    if (!h->graphs.empty()) return fail(MAPF_EINVAL, "set_policy: recorded graphs hold the current policy table (destroy them first)");
    if (policy == MAPF_POLICY_TABLE) return fail(MAPF_EINVAL, "set_policy: MAPF_POLICY_TABLE is set through mapf_set_policy_table (it takes the table and the row indices)");
    if (policy == MAPF_POLICY_JOINT) return fail(MAPF_EINVAL, "set_policy: MAPF_POLICY_JOINT is set through mapf_set_policy_joint (it takes the table, the offsets and the partners)");
    if (policy == MAPF_POLICY_GROUP) return fail(MAPF_EINVAL, "set_policy: MAPF_POLICY_GROUP is set through mapf_set_policy_group (it takes the rows, the groups and the books)");
    if (policy != MAPF_POLICY_RANDOM && policy != MAPF_POLICY_GREEDY) return fail(MAPF_EINVAL, "set_policy: unknown policy");
    if (policy == MAPF_POLICY_GREEDY && !cell_rc) return fail(MAPF_EINVAL, "set_policy: the greedy policy needs cell_rc");
    HIP_TRY(hipStreamSynchronize(h->stream));   // no launch may still be reading the old table
    h->drop_policy_table();                     // either policy leaves table mode
    h->drop_policy_joint();                     // ... and joint mode
    h->drop_policy_group();                     // ... and group mode
    if (policy == MAPF_POLICY_RANDOM) {
        h->policy_cells.reset();
        return MAPF_OK;
    }
    std::vector<uint2> cells;
    std::string error;
    if (!mapf::build_greedy_cells(h->nbr.data(), h->V, cell_rc, &cells, &error)) return fail(MAPF_EINVAL, error);
    if (!h->policy_cells) HIP_TRY(h->policy_cells.alloc(cells.size()));
    HIP_TRY(hipMemcpy(h->policy_cells, cells.data(), cells.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return MAPF_OK;
}

int mapf_fill_random_actions(mapf_handle_t h, uint8_t *actions, uint64_t t0, uint32_t n_steps) {
    if (int rc = check_handle(h)) return rc;
    if (!actions) return fail(MAPF_EINVAL, "actions is null");
    const size_t n = size_t(n_steps) * size_t(h->E) * h->A;
    uint8_t *d_actions = nullptr;
    const CallArray io[] = {output(h->s_actions, actions, n, &d_actions, "actions")};
    if (int rc = stage_arrays(h, io)) return rc;
    HIP_TRY(mapf::launch_fill_actions(int(h->A), d_actions, h->c, h->env_id_offset, h->E, t0, n_steps, h->stream));
    if (int rc = fetch_arrays(h, io)) return rc;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

namespace {
// the scan's scratch (handle-owned; a growing buffer is reallocated behind hipFree's implicit device synchronisation)
int transitions_scratch(mapf_handle_t h, mapf::TransitionsArgs &a) {
    HIP_TRY(h->q_rel.reserve((a.n_queries ? a.n_queries : 1) * sizeof(uint32_t)));
    HIP_TRY(h->q_blocks.reserve((mapf::transitions_scan_blocks(a.n_queries) + 1) * sizeof(uint64_t)));
    a.rel = static_cast<uint32_t *>(h->q_rel.ptr);
    a.block_base = static_cast<uint64_t *>(h->q_blocks.ptr);
    return MAPF_OK;
}

// mapf_transitions / _window (reserved rows: query q's window at q * max_branches) and _compact (rows packed, out_offset required)
int transitions_impl(mapf_handle_t h, bool compact, uint64_t n_queries, const uint16_t *local, const uint8_t *actions, const uint32_t *env_index,
                     uint64_t first_branch, uint32_t max_branches, uint64_t capacity_rows, uint64_t *out_offset, uint32_t *out_count, uint16_t *out_next,
                     double *out_prob, double *out_reward, uint8_t *out_done, uint8_t *out_collision) {
    if (int rc = check_handle(h)) return rc;
    if (!local || !actions) return fail(MAPF_EINVAL, "local / actions are null");
    if (compact && !out_offset) return fail(MAPF_EINVAL, "transitions_compact: out_offset (u64[n_queries + 1]) is required");
    if (max_branches == 0) return fail(MAPF_EINVAL, "max_branches must be >= 1");
    if (h->A > uint32_t(mapf::kTransitionsMaxAgents)) return fail(MAPF_EUNSUPPORTED, "mapf_transitions supports n_agents <= 16 (3^A branches per query)");
    const size_t N = size_t(n_queries), NA = N * h->A, R = compact ? size_t(capacity_rows) : N * max_branches;   // R: rows of the output arrays
    if (!h->device_ptrs) {
        for (size_t i = 0; i < NA; ++i) if (local[i] >= h->V) return fail(MAPF_EINVAL, "transitions: cell out of range");
        if (env_index) for (size_t i = 0; i < N; ++i) if (env_index[i] >= h->E) return fail(MAPF_EINVAL, "transitions: env_index out of range");
    }
    mapf::TransitionsArgs a = query_args_from_handle<mapf::TransitionsArgs>(h);
    a.n_queries = n_queries; a.max_branches = max_branches; a.n_agents = h->A; a.first_branch = first_branch;
    a.capacity = compact ? capacity_rows : ~uint64_t(0);
    enum { kOffset = 3, kCount, kNext, kProb, kReward, kDone, kColl };
    CallArray io[] = {input(h->q_local, local, NA, &a.local, "local"), input(h->q_actions, actions, NA, &a.actions, "actions"),
                      input(h->q_env, env_index, N, &a.env_index, "env_index"), output(h->q_offset, out_offset, N + 1, &a.out_offset, "out_offset"),
                      output(h->q_count, out_count, N, &a.out_count, "out_count"), output(h->q_next, out_next, R * h->A, &a.out_next, "out_next"),
                      output(h->q_prob, out_prob, R, &a.out_prob, "out_prob"), output(h->q_reward, out_reward, R, &a.out_reward, "out_reward"),
                      output(h->q_done, out_done, R, &a.out_done, "out_done"), output(h->q_coll, out_collision, R, &a.out_collision, "out_collision")};
    if (int rc = stage_arrays(h, io)) return rc;
    if (int rc = transitions_scratch(h, a)) return rc;
    a.compact = compact;
    if (compact && N == 0) HIP_TRY(hipMemsetAsync(a.out_offset, 0, sizeof(uint64_t), h->stream));
    HIP_TRY(mapf::launch_transitions(a, h->stream));
    if (h->last_transitions_kernel != g_noted_kernel) h->last_transitions_kernel = g_noted_kernel;
    if (h->device_ptrs) return MAPF_OK;
    if (compact) {
        // host arrays: the offsets first -- only the rows that exist (and fit) are copied back
        if (int rc = fetch_arrays(h, io + kOffset, 1)) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        const size_t rows = size_t(std::min<uint64_t>(out_offset[N], capacity_rows));
        io[kNext].bytes = rows * h->A * sizeof(uint16_t);
        io[kProb].bytes = io[kReward].bytes = rows * sizeof(double);
        io[kDone].bytes = io[kColl].bytes = rows;
    }
    if (int rc = fetch_arrays(h, io + kCount, size_t(kColl - kCount + 1))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}
}  // namespace

int mapf_transitions_window(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                            const uint32_t *env_index, uint64_t first_branch, uint32_t max_branches, uint32_t *out_count, uint16_t *out_next,
                            double *out_prob, double *out_reward, uint8_t *out_done, uint8_t *out_collision) {
    return transitions_impl(h, false, n_queries, local, actions, env_index, first_branch, max_branches, 0, nullptr, out_count, out_next, out_prob,
                            out_reward, out_done, out_collision);
}

int mapf_transitions(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                     const uint32_t *env_index, uint32_t max_branches, uint32_t *out_count, uint16_t *out_next,
                     double *out_prob, double *out_reward, uint8_t *out_done, uint8_t *out_collision) {
    return transitions_impl(h, false, n_queries, local, actions, env_index, 0, max_branches, 0, nullptr, out_count, out_next, out_prob,
                            out_reward, out_done, out_collision);
}

int mapf_transitions_compact(mapf_handle_t h, uint64_t n_queries, const uint16_t *local, const uint8_t *actions,
                             const uint32_t *env_index, uint64_t first_branch, uint32_t max_branches, uint64_t capacity_rows,
                             uint64_t *out_offset, uint32_t *out_count, uint16_t *out_next, double *out_prob, double *out_reward,
                             uint8_t *out_done, uint8_t *out_collision) {
    return transitions_impl(h, true, n_queries, local, actions, env_index, first_branch, max_branches, capacity_rows, out_offset, out_count, out_next,
                            out_prob, out_reward, out_done, out_collision);
}

int mapf_transition_rewards(mapf_handle_t h, uint64_t n_queries, const uint16_t *prev_local, const uint8_t *actions,
                            const uint16_t *next_local, const uint32_t *env_index, double *out_reward, uint8_t *out_done,
                            uint8_t *out_collision) {
    if (int rc = check_handle(h)) return rc;
    if (!prev_local || !actions || !next_local) return fail(MAPF_EINVAL, "prev_local / actions / next_local are null");
    const size_t N = size_t(n_queries), NA = N * h->A;
    if (!h->device_ptrs) {
        for (size_t i = 0; i < NA; ++i)
            if (prev_local[i] >= h->V || next_local[i] >= h->V) return fail(MAPF_EINVAL, "transition_rewards: cell out of range");
        if (env_index) for (size_t i = 0; i < N; ++i) if (env_index[i] >= h->E) return fail(MAPF_EINVAL, "transition_rewards: env_index out of range");
    }
    mapf::TransitionsArgs a = query_args_from_handle<mapf::TransitionsArgs>(h);
    a.n_queries = n_queries; a.max_branches = 1; a.n_agents = h->A; a.capacity = ~uint64_t(0);
    const uint16_t *d_next = nullptr;
    const CallArray io[] = {input(h->q_local, prev_local, NA, &a.local, "prev_local"), input(h->q_actions, actions, NA, &a.actions, "actions"),
                            input(h->q_next_in, next_local, NA, &d_next, "next_local"), input(h->q_env, env_index, N, &a.env_index, "env_index"),
                            output(h->q_reward, out_reward, N, &a.out_reward, "out_reward"), output(h->q_done, out_done, N, &a.out_done, "out_done"),
                            output(h->q_coll, out_collision, N, &a.out_collision, "out_collision")};
    if (int rc = stage_arrays(h, io)) return rc;
    HIP_TRY(mapf::launch_transition_rewards(a, d_next, h->stream));
    if (int rc = fetch_arrays(h, io)) return rc;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_query_terminal(mapf_handle_t h, uint8_t *out_terminal) {
    if (int rc = check_handle(h)) return rc;
    if (!out_terminal) return fail(MAPF_EINVAL, "out_terminal is null");
    uint8_t *d_out = nullptr;
    const CallArray io[] = {output(h->s_term, out_terminal, size_t(h->E), &d_out, "out_terminal")};
    if (int rc = stage_arrays(h, io)) return rc;
    HIP_TRY(mapf::launch_query_terminal(int(h->A), h->state, h->goal, h->goal_broadcast, d_out, h->E, h->stream));
    if (int rc = fetch_arrays(h, io)) return rc;
    if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    return MAPF_OK;
}

int mapf_get_state(mapf_handle_t h, uint16_t *local, uint64_t *t) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_get_state")) return rc;
    if (t) *t = h->t;
    if (local) {
        const size_t bytes = size_t(h->E) * h->A * sizeof(uint16_t);
        HIP_TRY(hipMemcpyAsync(local, h->state, bytes, h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return MAPF_OK;
}

int mapf_set_state(mapf_handle_t h, const uint16_t *local, uint64_t t) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_set_state")) return rc;
    if (local) {
        const size_t n = size_t(h->E) * h->A;
        if (!h->device_ptrs) {
            for (size_t i = 0; i < n; ++i)
                if (local[i] >= h->V) return fail(MAPF_EINVAL, "set_state: cell out of range");
        }
        HIP_TRY(hipMemcpyAsync(h->state, local, n * sizeof(uint16_t),
                               h->device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        h->may_be_terminal = true;   // (an arbitrary state)
        if (h->episode_limit) HIP_TRY(hipMemsetAsync(h->age, 0, size_t(h->E) * sizeof(uint32_t), h->stream));   // (... of new episodes)
        if (h->log_capacity) HIP_TRY(mapf::launch_reset_log_partials(h->log_partials(), nullptr, h->E, h->stream));   // (... whose running records begin again)
        if (!h->device_ptrs) HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->t = t;
    return MAPF_OK;
}

int mapf_state_view(mapf_handle_t h, const uint16_t **out_state) {
    if (int rc = check_handle(h)) return rc;
    if (!out_state) return fail(MAPF_EINVAL, "out_state is null");
    *out_state = h->state;
    return MAPF_OK;
}

int mapf_invalidate_state(mapf_handle_t h) {
    if (int rc = check_handle(h)) return rc;
    h->may_be_terminal = true;
    h->cap_may_be_terminal = true;
    for (mapf_graph_s *g : h->graphs) g->ends_may_be_terminal = true;   // (conservative: a replay may run over edited state too)
    return MAPF_OK;
}

int mapf_graph_begin(mapf_handle_t h) {
    if (int rc = check_handle(h)) return rc;
    if (!h->device_ptrs) return fail(MAPF_EINVAL, "graph_begin: only handles created with MAPF_FLAG_DEVICE_PTRS can be recorded (host-pointer calls wait for the stream)");
    if (h->capturing) return fail(MAPF_EINVAL, "graph_begin: already recording");
    if (h->episode_limit) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle with an episode limit cannot be recorded (mapf_set_episode_limit(h, 0) first)");
    if (h->episode_budget) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle with an episode budget cannot be recorded (mapf_set_episode_budget(h, 0) first)");
    if (h->log_capacity) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle with an episode log cannot be recorded (mapf_set_episode_log(h, 0) first)");
    if (h->pair_slots) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle with a conflict matrix cannot be recorded (mapf_set_conflict_pairs(h, 0, NULL) first)");
    if (h->group.table) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle under the group policy cannot be recorded (mapf_set_policy or mapf_set_policy_table first)");
    if (h->joint.table) return fail(MAPF_EUNSUPPORTED, "graph_begin: a handle under the joint table policy cannot be recorded (mapf_set_policy or mapf_set_policy_table first)");
    HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
    h->capturing = true;
    h->cap_steps = 0;
    h->cap_may_be_terminal = true;   // whatever precedes a replay: the first recorded step tests is_terminal itself
    return MAPF_OK;
}

int mapf_graph_end(mapf_handle_t h, mapf_graph_t *out_graph) {
    if (int rc = check_handle(h)) return rc;
    if (!h->capturing) return fail(MAPF_EINVAL, "graph_end: not recording");
    hipError_t adv = hipSuccess;
    if (out_graph && h->cap_steps) adv = mapf::launch_advance_step_index(h->t_dev, h->cap_steps, h->stream);   // the recording's last node
    hipGraph_t graph = nullptr;
    const hipError_t end = hipStreamEndCapture(h->stream, &graph);
    h->capturing = false;
    if (out_graph) *out_graph = nullptr;
    if (adv != hipSuccess || end != hipSuccess || !graph || !out_graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        if (!out_graph) return fail(MAPF_EINVAL, "graph_end: out_graph is null (the recording was dropped)");
        return hip_fail(adv != hipSuccess ? adv : (end != hipSuccess ? end : hipErrorUnknown), "graph_end: the recording failed");
    }
    mapf_graph_t g = new (std::nothrow) mapf_graph_s();
    if (!g) { (void)hipGraphDestroy(graph); return fail(MAPF_EHIP, "out of host memory"); }
    g->owner = h; g->graph = graph; g->steps = h->cap_steps;
    g->ends_may_be_terminal = h->cap_may_be_terminal;
    const hipError_t inst = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (inst != hipSuccess) { delete g; return hip_fail(inst, "hipGraphInstantiate"); }   // (the recording goes with it)
    h->graphs.push_back(g);
    *out_graph = g;
    return MAPF_OK;
}

int mapf_graph_launch(mapf_handle_t h, mapf_graph_t g, uint32_t n_replays) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_not_recording(h, "mapf_graph_launch")) return rc;
    if (!g || std::find(h->graphs.begin(), h->graphs.end(), g) == h->graphs.end()) return fail(MAPF_EINVAL, "graph_launch: not a live graph of this handle");
    // the device-side index must hold the handle's step index when the first recorded launch reads it
    if (h->t_dev_value != h->t) {
        HIP_TRY(mapf::launch_set_step_index(h->t_dev, h->t, h->stream));
        h->t_dev_value = h->t;
    }
    for (uint32_t r = 0; r < n_replays; ++r) HIP_TRY(hipGraphLaunch(g->exec, h->stream));
    h->t += uint64_t(n_replays) * g->steps;
    h->t_dev_value = h->t;
    if (n_replays) h->may_be_terminal = g->ends_may_be_terminal;
    return MAPF_OK;
}

int mapf_graph_steps(mapf_graph_t g, uint64_t *out_steps) {
    if (!g || !out_steps) return fail(MAPF_EINVAL, "null graph or output");
    *out_steps = g->steps;
    return MAPF_OK;
}

int mapf_graph_destroy(mapf_handle_t h, mapf_graph_t g) {
    if (int rc = check_handle(h)) return rc;
    const auto it = g ? std::find(h->graphs.begin(), h->graphs.end(), g) : h->graphs.end();
    if (it == h->graphs.end()) return fail(MAPF_EINVAL, "graph_destroy: not a live graph of this handle");
    HIP_TRY(hipStreamSynchronize(h->stream));   // no replay may still be running
    h->graphs.erase(it);
    delete g;
    return MAPF_OK;
}

}  // extern "C"
