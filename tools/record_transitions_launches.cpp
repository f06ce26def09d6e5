// Records what a commit's env.P[s][a] launchers hand to the runtime, without a device: linked with that commit's
// mapf_transitions.hip object IN PLACE of the HIP runtime, this program defines the few runtime entries the object calls
// (kernel registration, the launch-configuration push / pop, hipLaunchKernel, hipGetLastError) and note_kernel, calls
// launch_transitions for every shape on its standard input and prints, per shape, the return code, the noted name and every
// launch: kernel, grid, block, dynamic LDS bytes and the kernel's scalar arguments.  It recorded tests/golden/transitions_plans.json
// from the commit whose launchers still computed these themselves (tests/golden/generation_info.json says how); against a
// later commit, link mapf_plan.hip and mapf_dispatch.hip's launch_transitions as well.
//
//   hipcc --cuda-host-only -fuse-cuid=none -fPIE -O1 -std=c++17 -I include -c gym-mapf_amd/csrc/mapf_transitions.hip -o tr.o
//   c++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I include -I gym-mapf_amd/csrc tr.o tools/record_transitions_launches.cpp -o record_transitions_launches
//   stdin:  n_agents n_queries max_branches compact all_out        (one shape per line)
//   stdout: rc=0;name=...;count g=.. b=.. lds=..;totals g=.. b=.. lds=.. n=.. total=0|1;rows<8,1> g=.. b=.. lds=.. 3 6 1024 1
#include "mapf_kernels.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

// host stub -> mangled device name (filled by the object's constructor: made on first use)
static std::map<const void *, std::string> &kernels() { static std::map<const void *, std::string> m; return m; }
static std::string g_line, g_name;
static struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_config;
static mapf::TransitionsArgs g_args;

namespace mapf {
void note_kernel(const char *fmt, ...) {
    char text[kKernelNameBytes];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
    g_name = text;
}
}  // namespace mapf

extern "C" {
extern const char __hip_fatbin[1] = {0};   // (the host-only object names its device code; there is none)
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) { kernels()[host] = device_name; }
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_config = {grid, block, lds, stream}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *stream) {
    *grid = g_config.grid; *block = g_config.block; *lds = g_config.lds; *stream = g_config.stream;
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipLaunchKernel(const void *host, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t) {
    const std::string &dev = kernels()[host];
    char text[256], shape[96];
    snprintf(shape, sizeof(shape), "g=%u,%u,%u b=%u,%u,%u lds=%zu", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    int n = 0, flag = 0;
    auto u32 = [&](int i) { return *static_cast<const uint32_t *>(args[i]); };
    const bool same_args = dev.find("scan_block_totals") != std::string::npos || memcmp(args[0], &g_args, sizeof(g_args)) == 0;
    if (dev.find("transitions_count_kernel") != std::string::npos)
        snprintf(text, sizeof(text), ";count %s rel=%d base=%d", shape, *static_cast<uint32_t **>(args[1]) == g_args.rel, *static_cast<uint64_t **>(args[2]) == g_args.block_base);
    else if (dev.find("scan_block_totals_kernel") != std::string::npos)
        snprintf(text, sizeof(text), ";totals %s base=%d n=%u total=%d", shape, *static_cast<uint64_t **>(args[0]) == g_args.block_base, u32(1),
                 *static_cast<uint64_t **>(args[2]) == nullptr ? 0 : (*static_cast<uint64_t **>(args[2]) == g_args.out_offset + g_args.n_queries ? 1 : -1));
    else if (sscanf(dev.c_str() + (dev.find("transitions_rows_kernelILi") == std::string::npos ? dev.size() : dev.find("transitions_rows_kernelILi")),
                    "transitions_rows_kernelILi%dELb%d", &n, &flag) == 2)
        snprintf(text, sizeof(text), ";rows<%d,%d> %s %u %u %u %u", n, flag, shape, u32(1), u32(2), u32(3), u32(4));
    else if (sscanf(dev.c_str() + (dev.find("transitions_kernelILi") == std::string::npos ? dev.size() : dev.find("transitions_kernelILi")),
                    "transitions_kernelILi%dELb%d", &n, &flag) == 2)
        snprintf(text, sizeof(text), ";wide<%d,%d> %s %u %u %u", n, flag, shape, u32(1), u32(2), u32(3));
    else
        snprintf(text, sizeof(text), ";UNKNOWN %s", dev.c_str());
    g_line += text;
    if (!same_args) g_line += " ARGS-CHANGED";
    return hipSuccess;
}
}

int main() {
    static unsigned char somewhere[64];   // (the arrays are never dereferenced on the host: present or not is all a launcher reads)
    unsigned A, M, compact, all_out;
    unsigned long long N;
    while (scanf("%u %llu %u %u %u", &A, &N, &M, &compact, &all_out) == 5) {
        mapf::TransitionsArgs a{};
        a.n_agents = A; a.n_queries = N; a.max_branches = M; a.compact = compact != 0;
        a.out_next = reinterpret_cast<uint16_t *>(somewhere); a.out_prob = reinterpret_cast<double *>(somewhere); a.out_reward = reinterpret_cast<double *>(somewhere);
        a.out_collision = somewhere; a.out_done = all_out ? somewhere : nullptr;
        a.rel = reinterpret_cast<uint32_t *>(somewhere + 8); a.block_base = reinterpret_cast<uint64_t *>(somewhere + 16);
        a.out_offset = reinterpret_cast<uint64_t *>(somewhere + 24);
        a.capacity = ~0ull;
        g_args = a; g_line.clear(); g_name.clear();
        const hipError_t rc = mapf::launch_transitions(a, nullptr);
        printf("rc=%d;name=%s%s\n", int(rc), g_name.c_str(), g_line.c_str());
    }
    return 0;
}
