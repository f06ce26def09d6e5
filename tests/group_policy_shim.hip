// Host-side access to the group policy's planning for tests/test_group_policy_host.py: route_rollout with the `group` fact, compiled
// with csrc/mapf_plan.hip and csrc/mapf_tables.hip into a shared object (no kernel, no device).  With GROUP_SHIM_MAIN the same file is
// a stand-alone program that builds the device table of random books on the host and checks every lookup against a std::map -- the
// program the host builder and lookup are run through under the address and undefined-behaviour sanitizers.
#include "mapf_plan.hpp"
#include "mapf_tables.hpp"

#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>

using namespace mapf;

extern "C" {

// route_rollout over a one-step launch under the group policy (prefer: FamilyPreference's number; the facts as 0 | 1).  Returns the
// family's number (KernelFamily), out = {L, full, mv_lds, dense, limit, budget, pairs, log, group, joint, block, grid, lds_bytes} and
// the name the launcher would note; -1 for a malformed tune string
int gshim_route_group(uint32_t n_cells, int n_agents, uint64_t n_envs, int n_cu, const char *tune, int prefer, int limited, int budgeted, int pairs, int logged,
                      int record, uint64_t out[13], char *name) {
    std::string err;
    const RolloutTuning t = rollout_tuning_for(n_cu, tune, &err);
    if (!err.empty()) return -1;
    RolloutArgs a{};
    a.c.n_cells = n_cells;
    a.n_envs = n_envs;
    a.n_steps = 1;
    a.auto_reset = true;
    const RolloutRoute r = route_rollout(n_agents, a, t, FamilyPreference(prefer), false, 0, limited != 0, budgeted != 0, pairs != 0, false, logged != 0, true);
    const LgRolloutPlan &p = r.lg;
    const uint64_t fields[13] = {uint64_t(p.L), p.full, p.mv_lds, p.dense, p.limit, p.budget, p.pairs, p.log, p.group, p.joint, p.block, p.grid, p.lds_bytes};
    memcpy(out, fields, sizeof(fields));
    lg_rollout_kernel_name(name, p, record != 0, false, true);
    return int(r.family);
}

uint64_t gshim_group_lds_bytes() { return kGroupLdsBytes; }

}  // extern "C"

#ifdef GROUP_SHIM_MAIN
int main() {
    std::mt19937_64 rng(12345);
    const uint32_t V = 65535, n_books = 7;
    long checked = 0;
    for (uint64_t n_entries : {uint64_t(0), uint64_t(1), uint64_t(37), uint64_t(4000), uint64_t(100000)}) {
        std::vector<std::map<std::array<uint16_t, 4>, std::array<uint8_t, 4>>> want(n_books);
        std::vector<GroupEntry> entries;
        std::vector<uint32_t> begin(n_books + 1, 0);
        for (uint32_t b = 0; b < n_books; ++b) {
            const uint64_t share = n_entries / n_books + (b < n_entries % n_books ? 1 : 0);
            while (want[b].size() < share) {
                const uint32_t arity = 1 + uint32_t(rng() % 4);
                std::array<uint16_t, 4> cell{0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
                std::array<uint8_t, 4> action{0, 0, 0, 0};
                for (uint32_t k = 0; k < arity; ++k) {
                    const uint64_t pick = rng() % 8;
                    cell[k] = pick == 0 ? 0 : (pick == 1 ? uint16_t(V - 1) : uint16_t(rng() % (pick < 4 ? 64 : V)));   // (small cells: near misses between books)
                    action[k] = uint8_t(rng() % 5);
                }
                if (want[b].emplace(cell, action).second) {
                    GroupEntry e;
                    memcpy(e.cell, cell.data(), sizeof(e.cell));
                    memcpy(e.action, action.data(), sizeof(e.action));
                    entries.push_back(e);
                }
            }
            begin[b + 1] = uint32_t(entries.size());
        }
        GroupTable table;
        std::string err;
        if (!build_group_table(entries.data(), entries.size(), begin.data(), n_books, &table, &err)) { printf("build failed: %s\n", err.c_str()); return 1; }
        const size_t slots = table.slots.size();
        if ((slots & (slots - 1)) != 0 || slots < 2 * entries.size()) { printf("capacity %zu for %zu entries\n", slots, entries.size()); return 1; }
        // every entry under its own book, under every other book, and random keys
        for (uint32_t b = 0; b < n_books; ++b)
            for (const auto &kv : want[b])
                for (uint32_t other = 0; other < n_books; ++other) {
                    uint32_t probes = 0;
                    const uint32_t got = lookup_group_table(table, kv.first.data(), other, &probes);
                    const auto it = want[other].find(kv.first);
                    uint32_t expect = kGroupMiss;
                    if (it != want[other].end()) memcpy(&expect, it->second.data(), 4);
                    if (got != expect || probes > table.max_probe) { printf("lookup: got %08x want %08x after %u probes (bound %u)\n", got, expect, probes, table.max_probe); return 1; }
                    ++checked;
                }
        for (int k = 0; k < 100000; ++k) {
            uint16_t cell[4];
            for (uint16_t &c : cell) c = uint16_t(rng() % 4 == 0 ? 0xFFFF : rng() % 64);
            const uint32_t b = uint32_t(rng() % (n_books + 2));
            uint32_t probes = 0, expect = kGroupMiss;
            const uint32_t got = lookup_group_table(table, cell, b, &probes);
            if (b < n_books) {
                const auto it = want[b].find({cell[0], cell[1], cell[2], cell[3]});
                if (it != want[b].end()) memcpy(&expect, it->second.data(), 4);
            }
            if (got != expect || probes > table.max_probe) { printf("random key: got %08x want %08x\n", got, expect); return 1; }
            ++checked;
        }
        // a duplicate is refused and named
        if (begin[n_books - 1] != begin[n_books]) {
            std::vector<GroupEntry> twice(entries);
            twice.push_back(entries[begin[n_books - 1]]);   // (the first entry of the last book again, at that book's end)
            std::vector<uint32_t> more(begin);
            more[n_books] += 1;
            GroupTable again;
            if (build_group_table(twice.data(), twice.size(), more.data(), n_books, &again, &err)) { printf("duplicate accepted\n"); return 1; }
        }
        printf("%llu entries: %zu slots, longest chain %u\n", (unsigned long long)entries.size(), slots, table.max_probe);
    }
    printf("ok: %ld lookups\n", checked);
    return 0;
}
#endif
