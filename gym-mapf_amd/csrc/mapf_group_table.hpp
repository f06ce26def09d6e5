// The device table of the group policy (include/mapf_hip.h MAPF_POLICY_GROUP, mapf_set_policy_group): ONE statement of the slot
// layout, the hash and the probe step, for the host builder (mapf_tables.hip), the host lookup (mapf_debug_policy_group) and the
// kernel (the GROUP sections of mapf_lg_rollout_kernel.hpp) -- as mapf_layout.hpp is for the packed table forms.
//
// All books of a plan lie in one open-addressing table of 16-byte slots; its capacity is a power of two >= 2 * n_entries (at least
// one slot), probing is linear.  A key is three words: the members' cells on entry to the step, two per word in list order with
// 0xFFFF at the padded positions, and the book's number.  A probe is one 16-byte load.
#pragma once
#include <stdint.h>

// (host and device where the compiler knows the two words, plain functions in a plain C++ unit: a macro of this header's own)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAPF_HD __host__ __device__
#else
#define MAPF_HD
#endif

namespace mapf {

struct GroupSlot {
    uint32_t c01, c23;             // cell[0] | cell[1] << 16, cell[2] | cell[3] << 16
    uint32_t book;                 // the book the entry belongs to; kGroupEmptyBook: the slot is empty
    uint32_t actions;              // action[0] | action[1] << 8 | action[2] << 16 | action[3] << 24
};
static_assert(sizeof(GroupSlot) == 16, "one probe is one 16-byte load");
constexpr uint32_t kGroupEmptyBook = 0xFFFFFFFFu;   // (a book's number is below n_books, a u32: never this value)
constexpr uint32_t kGroupMiss = 0xFFFFFFFFu;        // what a lookup that finds no entry returns (an action byte is 0..4)
constexpr uint32_t kGroupPad = 0xFFFFu;             // the cell of a padded position
constexpr uint64_t kGroupMaxEntries = uint64_t(1) << 24;

// a fixed 32-bit mix of the three key words
MAPF_HD inline uint32_t group_hash(uint32_t c01, uint32_t c23, uint32_t book) {
    uint32_t h = c01 * 0x9E3779B1u;
    h ^= h >> 15;
    h = (h + c23) * 0x85EBCA77u;
    h ^= h >> 13;
    h = (h + book) * 0xC2B2AE3Du;
    return h ^ (h >> 16);
}

// The lookup: from the key's home slot onward, at most max_probe slots (the longest chain the builder produced: no entry lies
// further from its home), ending at an empty slot as well -- so no table, however wrong, makes the loop run on.  `load(i)` reads
// slot i.  *probes (host callers) receives the slots read.
template <class Load>
MAPF_HD inline uint32_t group_lookup(Load load, uint32_t mask, uint32_t max_probe, uint32_t c01, uint32_t c23, uint32_t book,
                                                 uint32_t *probes = nullptr) {
    uint32_t i = group_hash(c01, c23, book) & mask, found = kGroupMiss, k = 0;
    for (; k < max_probe; ++k, i = (i + 1u) & mask) {
        const GroupSlot s = load(i);
        if (s.book == kGroupEmptyBook) { ++k; break; }
        if (s.c01 == c01 && s.c23 == c23 && s.book == book) { found = s.actions; ++k; break; }
    }
    if (probes) *probes = k;
    return found;
}

}  // namespace mapf
