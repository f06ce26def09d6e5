// Host construction of every table the kernels read (mapf_kernels.hpp describes their layouts): plain host arithmetic
// into vectors / PODs that the caller (mapf_create, mapf_set_policy) uploads.  No kernel, no runtime call -- so the
// tables can be checked without a device (tests/test_host_tables.py).
#pragma once
#include "mapf_kernels.hpp"

#include <string>
#include <vector>

namespace mapf {

// The eight slip rows of a fail_prob, and what the kernels' constants say about them: c->p_cand, c->need_rng (some list
// has more than one entry), c->top_tie.  false (*err = why) when a merged probability is not reproducible from its members.
bool build_slip_tables(double fail_prob, SlipRow (&rows)[8], EnvConsts *c, std::string *err);
// The sixteen outcome rows of the table image (reads c.r_clash, r_goal, r_living)
void build_outcome_rows(const EnvConsts &c, OutcomeRow (&rows)[16]);

// The move table of a neighbour table nbr[V][5] in its three forms
struct MoveTables {
    std::vector<MoveEntry> mv;        // [V * kMvCols] 16-byte rows
    std::vector<CompactEntry> mv8;    // [V * kMvCols] 8-byte rows
    bool delta8 = false;              // every neighbour id lies within +-127 of its cell's id
    std::vector<uint32_t> mv4;        // [delta_table_words(V)] 4-byte delta rows; empty unless delta8
};
MoveTables build_move_tables(const uint16_t *nbr, uint32_t V, double fail_prob, const SlipRow (&slip)[8]);

// Scenario table (StepArgs::scen): the distinct (start row, goal row) pairs of the batch and one byte per env naming its
// pair; n == 0 (and empty vectors) when there are more than 256 pairs.  start / goal: [E*A], or [A] when broadcast.
struct ScenTable {
    std::vector<uint8_t> scen;        // [E]
    std::vector<uint16_t> rows;       // [n * 2 * A]: pair i's start cells, then its goal cells
    uint32_t n = 0;
};
ScenTable build_scen_table(const uint16_t *start, bool start_broadcast, const uint16_t *goal, bool goal_broadcast, uint64_t E, uint32_t A);

// Greedy policy cells (RolloutArgs::policy_cells) from cell_rc[V] = row | col << 16; false (*err = why) when cell_rc does
// not match the neighbour table.
bool build_greedy_cells(const uint16_t *nbr, uint32_t V, const uint32_t *cell_rc, std::vector<uint2> *cells, std::string *err);

// Group policy (include/mapf_hip.h MAPF_POLICY_GROUP): what mapf_set_policy_group is handed, as host arrays -- the header names them.
// An entry is the header's mapf_group_entry: four u16 cells, then four action bytes.
struct GroupEntry { uint16_t cell[4]; uint8_t action[4]; };
static_assert(sizeof(GroupEntry) == 12, "mapf_group_entry");
struct GroupPlanArrays {
    uint32_t V = 0, A = 0;
    uint64_t E = 0;
    const uint8_t *table = nullptr;        // [n_rows * V]
    uint32_t n_rows = 0;
    const uint16_t *row_index = nullptr;   // [E*A], or [A] when broadcast
    const uint16_t *members = nullptr;     // [E*A*4] / [A*4]
    const uint32_t *book = nullptr;        // [E*A] / [A]
    const GroupEntry *entries = nullptr;   // [n_entries]
    uint64_t n_entries = 0;
    const uint32_t *book_begin = nullptr;  // [n_books + 1]
    uint32_t n_books = 0;
    bool broadcast = false;
};
// Every rule of the header about these arrays (the pointers are non-null where the header demands it: the caller has looked), in the
// header's order; false (*err names the offending index) at the first one broken.
bool validate_group_plan(const GroupPlanArrays &plan, std::string *err);
// The device table of all books (mapf_group_table.hpp): capacity a power of two >= 2 * n_entries, linear probing; max_probe is the
// longest chain produced -- the slots a lookup reads, at most, before it meets an entry that is there.  false (*err names the second
// entry) when two entries of one book have the same four cells.
struct GroupTable {
    std::vector<GroupSlot> slots;
    uint32_t max_probe = 0;
};
bool build_group_table(const GroupEntry *entries, uint64_t n_entries, const uint32_t *book_begin, uint32_t n_books, GroupTable *out, std::string *err);
// The host lookup through the shared probe function: the entry's four action bytes as one word, or kGroupMiss; *probes: slots read
uint32_t lookup_group_table(const GroupTable &table, const uint16_t cell[4], uint32_t book, uint32_t *probes);

}  // namespace mapf
