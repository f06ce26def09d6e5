// Host construction of the tables the kernels read (mapf_tables.hpp): host-only, no kernel and no runtime call.
#include "mapf_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace mapf {

// Replay single_agent_movements (mapf_env.py:163-184) for each equality pattern of the candidate cells
// (m intended, r right slip, l left slip), in IEEE double and the reference's evaluation order -- the
// same operations CPython performs: rf = lf = fail_prob / 2 (:131-132), p0 = 1 - rf - lf (:167), drop
// p <= 0 (:172), merge equal cells with old + new in first-seen order (:177-182); cum = np.cumsum.
// c->need_rng: some list has more than one entry, i.e. a uniform is actually consumed.
bool build_slip_tables(double fail_prob, SlipRow (&rows)[8], EnvConsts *c, std::string *err) {
    double (&cand_p)[3] = c->p_cand;
    const double rf = fail_prob / 2, lf = fail_prob / 2;
    cand_p[0] = (1 - rf) - lf; cand_p[1] = rf; cand_p[2] = lf;
    bool any_multi = false;
    for (unsigned code = 0; code < 8; ++code) {
        // representative cells realising the pattern (inconsistent codes cannot occur at run time)
        const int m = 0, r = (code & 1u) ? 0 : 1, l = (code & 2u) ? 0 : ((code & 4u) ? r : 2);
        const int cand_cell[3] = {m, r, l};
        int cells[3] = {-1, -1, -1}, members[3] = {0, 0, 0}, n = 0;
        double q[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) {
            if (!(cand_p[k] > 0)) continue;
            int hit = -1;
            for (int j = 0; j < n; ++j) if (cells[j] == cand_cell[k]) { hit = j; break; }
            if (hit >= 0) { q[hit] = q[hit] + cand_p[k]; members[hit] |= 1 << k; }
            else { cells[n] = cand_cell[k]; q[n] = cand_p[k]; members[n] = 1 << k; ++n; }
        }
        SlipRow &row = rows[code];
        std::memset(&row, 0, sizeof(row));
        row.n = uint32_t(n);
        double run = 0.0;
        for (int k = 0; k < 3; ++k) {
            if (k < n) {
                run = (k == 0) ? q[0] : run + q[k];
                row.cum[k] = run;
                row.q[k] = q[k];
                const double scaled = std::ceil(std::ldexp(run, 53));          // exact: power-of-two scaling
                row.thr[k] = scaled >= 9007199254740992.0 ? (uint64_t(1) << 53) : (scaled <= 0 ? 0 : uint64_t(scaled));
                row.th[k] = uint32_t(row.thr[k] >> 37) > 65535u ? 65535u : uint32_t(row.thr[k] >> 37);   // saturated (see SlipRow)
                row.members |= uint32_t(members[k]) << (3 * k);
            } else {
                row.cum[k] = -HUGE_VAL;
                row.q[k] = 0.0;
                row.thr[k] = 0;
                row.th[k] = 65535u;
            }
        }
        // th[2] is never compared against (a list's last threshold is 65535 by construction): it carries th[0] | th[1] << 16,
        // the word MoveEntry::z holds, for kernels that keep only the cells of a row in LDS (mapf_lq_rollout.hip COMPACT)
        row.th[2] = row.th[0] | (row.th[1] << 16);
        row.th_biased = row.th[2] ^ 0x80008000u;   // (sample_slot_packed compares bias-shifted half-words)
        any_multi |= n > 1;
    }
    c->need_rng = any_multi ? 1u : 0u;
    c->top_tie = 0u;
    for (unsigned code = 0; code < 8; ++code)
        if (rows[code].n == 3 && rows[code].thr[2] < (uint64_t(1) << 53)) c->top_tie = 1u;   // (shorter lists compare against their last threshold, 65535)
    // the single-step kernels rebuild a merged probability from its members instead of reading the row: the ordered
    // sum ((m ? p_m : 0) + (r ? p_r : 0)) + (l ? p_l : 0) must reproduce the table bit for bit
    for (unsigned code = 0; code < 8; ++code)
        for (unsigned k = 0; k < rows[code].n; ++k) {
            const unsigned mem = (rows[code].members >> (3 * k)) & 7u;
            const double q = (((mem & 1u) ? c->p_cand[0] : 0.0) + ((mem & 2u) ? c->p_cand[1] : 0.0)) + ((mem & 4u) ? c->p_cand[2] : 0.0);
            if (std::memcmp(&q, &rows[code].q[k], sizeof(q)) != 0) {
                *err = "create: merged slip probabilities are not reproducible from their members";
                return false;
            }
        }
    return true;
}

// The sixteen outcome rows of the table image (mapf_kernels.hpp TableImage; device twin: stage_outcome_rows in mapf_lg.hpp):
// rows 0..7 = f = vertex | swap << 1 | off_goal << 2, rows 8..15 = the state was terminal (mapf_env.py:239-240).  Makespan's
// reward is a function of f: r_clash + living / r_goal + living / living (calc_transition_reward_from_local_states,
// mapf_env.py:225-235; one float64 addition each, as the reference's `reward + living_reward`).
void build_outcome_rows(const EnvConsts &c, OutcomeRow (&rows)[16]) {
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t st = outcome_status(i & 7u);
        const double r = (st & 0x100u) ? c.r_clash + c.r_living : ((st & 1u) ? c.r_goal + c.r_living : c.r_living);
        rows[i].reward = i < 8u ? r : 0.0;
        rows[i].status = i < 8u ? st : kTerminalStatus;
        rows[i].pad = (rows[i].status & 1u) | ((rows[i].status & 0x100u) << 8);
    }
}

MoveTables build_move_tables(const uint16_t *nbr, uint32_t V, double fail_prob, const SlipRow (&slip)[8]) {
    MoveTables t;
    t.delta8 = true;
    for (uint32_t v = 0; v < V && t.delta8; ++v)
        for (uint32_t a = 0; a < 5; ++a) {
            const int64_t delta = int64_t(nbr[uint64_t(v) * 5 + a]) - int64_t(v);
            if (delta < -127 || delta > 127) t.delta8 = false;
        }
    // Move table: for every (cell, action) the merged movement list of single_agent_movements
    // (mapf_env.py:163-184) -- its cells in list order and the equality code of the three candidates.
    const double rf_ = fail_prob / 2, lf_ = fail_prob / 2;
    const bool keep[3] = {((1 - rf_) - lf_) > 0, rf_ > 0, lf_ > 0};
    static const uint8_t kSlipRight[5] = {0, 2, 3, 4, 1}, kSlipLeft[5] = {0, 4, 1, 2, 3};   // __init__.py:19-25
    std::vector<MoveEntry> &packed = t.mv;
    packed.resize(size_t(V) * kMvCols);   // column 5 = STAY again (kMvCols)
    for (uint32_t v = 0; v < V; ++v) {
        const uint16_t *r = nbr + uint64_t(v) * 5;
        for (uint32_t col = 0; col < kMvCols; ++col) {
            const uint32_t a = col < 5 ? col : 0;
            const uint16_t cand[3] = {r[a], r[kSlipRight[a]], r[kSlipLeft[a]]};
            const uint64_t code = (cand[0] == cand[1] ? 1u : 0u) | (cand[0] == cand[2] ? 2u : 0u) | (cand[1] == cand[2] ? 4u : 0u);
            uint16_t cells[3] = {0, 0, 0};
            int n = 0;
            for (int k = 0; k < 3; ++k) {
                if (!keep[k]) continue;
                bool seen = false;
                for (int j = 0; j < n; ++j) seen |= (cells[j] == cand[k]);
                if (!seen) cells[n++] = cand[k];
            }
            // top 16 bits of the list's cumulative thresholds, saturated (see MoveEntry)
            uint32_t t16[3];
            // (past the list end: 65535 as well -- `hi < 65535` only fails in a tie, and an earlier slot has matched by then)
            for (int k = 0; k < 3; ++k)
                t16[k] = slip[code].th[k];
            packed[size_t(v) * kMvCols + col] = make_uint4(uint32_t(cells[0]) | (uint32_t(cells[1]) << 16),
                                                    uint32_t(cells[2]) | (uint32_t(code) << 16) | (slip[code].members << 19),
                                                    t16[0] | (t16[1] << 16), uint32_t(code * sizeof(SlipRow)));
        }
    }
    t.mv8.resize(packed.size());
    for (size_t i = 0; i < packed.size(); ++i) t.mv8[i] = make_uint2(packed[i].x, (packed[i].y & 0xFFFFu) | (packed[i].w << 16));
    if (t.delta8) {   // 4-byte delta rows, six columns (mapf_kernels.hpp kDeltaCols); the padding words stay zero
        std::vector<uint32_t> &delta = t.mv4;
        delta.assign(delta_table_words(V), 0u);
        for (uint32_t v = 0; v < V; ++v)
            for (uint32_t col = 0; col < kDeltaCols; ++col) {
                const MoveEntry &e = packed[size_t(v) * kMvCols + (col < kMvCols ? col : 0u)];
                delta[size_t(v) * kDeltaCols + col] = ((e.x - v) & 0xFFu) | ((((e.x >> 16) - v) & 0xFFu) << 8) | (((e.y - v) & 0xFFu) << 16) |
                                                            (((e.w + kDeltaRowBias) >> 3) << 24);
            }
    }
    return t;
}

ScenTable build_scen_table(const uint16_t *start, bool sb, const uint16_t *goal, bool gb, uint64_t E, uint32_t A) {
    // Scenario table: the distinct (start row, goal row) pairs of the batch, when there are few (the BASELINE
    // configurations draw every env's rows from 6 or 25 scenario files), and one byte per env naming its pair.
    ScenTable t;
    const size_t row = size_t(A) * sizeof(uint16_t);
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<uint8_t> scen(E);
    std::vector<uint16_t> rows;
    bool few = true;
    std::string key(2 * row, '\0');
    for (uint64_t e = 0; e < E && few; ++e) {
        std::memcpy(&key[0], start + (sb ? 0 : e * A), row);
        std::memcpy(&key[row], goal + (gb ? 0 : e * A), row);
        auto it = ids.find(key);
        if (it == ids.end()) {
            if (ids.size() == 256) { few = false; break; }
            it = ids.emplace(key, uint32_t(ids.size())).first;
            rows.insert(rows.end(), reinterpret_cast<const uint16_t *>(key.data()), reinterpret_cast<const uint16_t *>(key.data()) + 2 * A);
        }
        scen[e] = uint8_t(it->second);
    }
    if (few) {
        t.n = uint32_t(ids.size());
        t.scen.swap(scen);
        t.rows.swap(rows);
    }
    return t;
}

bool build_greedy_cells(const uint16_t *nbr, uint32_t V, const uint32_t *cell_rc, std::vector<uint2> *out, std::string *err) {
    // For every cell and every direction (sign of goal row - row, sign of goal col - col) the first action in
    // ACTIONS order that is not blocked and lands one step closer; whether a move helps is read off the
    // coordinates of its target, so no axis convention is assumed.
    std::vector<uint2> &cells = *out;
    cells.resize(V);
    for (uint32_t v = 0; v < V; ++v) {
        const int r = int(cell_rc[v] & 0xFFFFu), c = int(cell_rc[v] >> 16);
        uint32_t best = 0;
        for (int sr = -1; sr <= 1; ++sr)
            for (int sc = -1; sc <= 1; ++sc) {
                uint32_t pick = 0;   // STAY
                for (uint32_t a = 1; a < 5 && pick == 0; ++a) {
                    const uint32_t tgt = nbr[size_t(v) * 5 + a];
                    if (tgt == v) continue;   // blocked
                    const int dr = int(cell_rc[tgt] & 0xFFFFu) - r, dc = int(cell_rc[tgt] >> 16) - c;
                    if ((std::abs(dr) + std::abs(dc)) != 1) {
                        *err = "set_policy: cell_rc does not match the neighbour table (a move must change one coordinate by one)";
                        return false;
                    }
                    if ((dr != 0 && dr == sr) || (dc != 0 && dc == sc)) pick = a;
                }
                best |= pick << (3 * (3 * (sr + 1) + (sc + 1)));
            }
        cells[v] = make_uint2(cell_rc[v], best);
    }
    return true;
}

// ------------------------------------------------------------------- the group policy
bool validate_group_plan(const GroupPlanArrays &g, std::string *err) {
    const auto say = [&](const std::string &what) { *err = "set_policy_group: " + what; return false; };
    const auto num = [](uint64_t v) { return std::to_string(v); };
    const uint64_t A = g.A, V = g.V;
    // the table policy's own checks
    if (g.n_rows == 0 || g.n_rows > 65536u) return say("n_rows must be 1..65536");
    const uint64_t bytes = uint64_t(g.n_rows) * V;
    if (bytes > 0x7FFFFFFFull) return say("table (n_rows * V bytes) exceeds 2 GiB");
    for (uint64_t i = 0; i < bytes; ++i)
        if (g.table[i] > 4u) return say("table[" + num(i) + "] = " + num(g.table[i]) + " is not an action (0..4)");
    const uint64_t n_index = g.broadcast ? A : g.E * A;
    for (uint64_t i = 0; i < n_index; ++i)
        if (g.row_index[i] >= g.n_rows) return say("row_index[" + num(i) + "] = " + num(g.row_index[i]) + " is not below n_rows");
    // the books' ranges
    if (g.n_entries > kGroupMaxEntries) return say("n_entries = " + num(g.n_entries) + " exceeds 2^24");
    if (g.book_begin) {
        if (g.book_begin[0] != 0u) return say("book_begin[0] = " + num(g.book_begin[0]) + " is not 0");
        for (uint32_t b = 0; b < g.n_books; ++b)
            if (g.book_begin[b + 1] < g.book_begin[b]) return say("book_begin[" + num(b + 1) + "] = " + num(g.book_begin[b + 1]) + " is below book_begin[" + num(b) + "]");
        if (g.book_begin[g.n_books] != g.n_entries) return say("book_begin[" + num(g.n_books) + "] = " + num(g.book_begin[g.n_books]) + " is not n_entries");
    }
    // the groups
    for (uint64_t i = 0; i < n_index; ++i) {
        const uint64_t row = i - i % A, me = i % A;
        const uint16_t *list = g.members + i * 4u;
        uint32_t size = 0;
        bool has_me = false;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint64_t at = i * 4u + k;
            if (list[k] == kGroupPad) continue;
            if (list[k] >= A) return say("members[" + num(at) + "] = " + num(list[k]) + " is not below n_agents");
            if (size != k) return say("members[" + num(at) + "] = " + num(list[k]) + " follows padding: padding must be trailing");
            if (k > 0 && list[k] <= list[k - 1]) return say("members[" + num(at) + "] = " + num(list[k]) + " is not above members[" + num(at - 1) + "]: the list must be ascending");
            has_me = has_me || list[k] == me;
            ++size;
        }
        if (!has_me) return say("members[" + num(i * 4u) + "..]: the list of agent " + num(me) + " does not contain it");
        // (without books every group falls back to its rows, and `book` is not read)
        const bool booked = size >= 2u && g.n_books != 0u;
        if (booked && g.book[i] >= g.n_books) return say("book[" + num(i) + "] = " + num(g.book[i]) + " is not below n_books");
        for (uint32_t k = 0; k < size; ++k) {
            const uint64_t other = row + list[k];
            if (memcmp(g.members + other * 4u, list, 4 * sizeof(uint16_t)) != 0)
                return say("members[" + num(other * 4u) + "..]: agent " + num(list[k]) + " is a member of agent " + num(me) + "'s group (members[" + num(i * 4u) + "..]) but its list differs");
            if (booked && g.book[other] != g.book[i])
                return say("book[" + num(other) + "] = " + num(g.book[other]) + " differs from book[" + num(i) + "] = " + num(g.book[i]) + " of the same group");
        }
    }
    // the entries
    for (uint64_t n = 0; n < g.n_entries; ++n) {
        const GroupEntry &entry = g.entries[n];
        uint32_t size = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            const std::string at = "entries[" + num(n) + "]";
            if (entry.action[k] > 4u) return say(at + ".action[" + num(k) + "] = " + num(entry.action[k]) + " is not an action (0..4)");
            if (entry.cell[k] == kGroupPad) {
                if (entry.action[k] != 0u) return say(at + ".action[" + num(k) + "] = " + num(entry.action[k]) + " at a padded position must be 0");
                continue;
            }
            if (entry.cell[k] >= V) return say(at + ".cell[" + num(k) + "] = " + num(entry.cell[k]) + " is not a cell (below V) and not padding");
            if (size != k) return say(at + ".cell[" + num(k) + "] = " + num(entry.cell[k]) + " follows padding: padding must be trailing");
            ++size;
        }
    }
    return true;
}

bool build_group_table(const GroupEntry *entries, uint64_t n_entries, const uint32_t *book_begin, uint32_t n_books, GroupTable *out, std::string *err) {
    uint64_t capacity = 1;
    while (capacity < 2u * n_entries) capacity <<= 1;
    out->slots.assign(size_t(capacity), GroupSlot{0u, 0u, kGroupEmptyBook, 0u});
    out->max_probe = 0;
    const uint32_t mask = uint32_t(capacity - 1u);
    for (uint32_t b = 0; b < n_books; ++b)
        for (uint64_t n = book_begin[b]; n < book_begin[b + 1]; ++n) {
            const GroupEntry &entry = entries[n];
            const GroupSlot s{uint32_t(entry.cell[0]) | uint32_t(entry.cell[1]) << 16, uint32_t(entry.cell[2]) | uint32_t(entry.cell[3]) << 16, b,
                              uint32_t(entry.action[0]) | uint32_t(entry.action[1]) << 8 | uint32_t(entry.action[2]) << 16 | uint32_t(entry.action[3]) << 24};
            uint32_t i = group_hash(s.c01, s.c23, s.book) & mask, chain = 1;
            for (; out->slots[i].book != kGroupEmptyBook; i = (i + 1u) & mask, ++chain)   // (at most half the slots are taken: an empty one comes)
                if (out->slots[i].c01 == s.c01 && out->slots[i].c23 == s.c23 && out->slots[i].book == b) {
                    *err = "set_policy_group: entries[" + std::to_string(n) + "] has the same four cells as an earlier entry of book " + std::to_string(b);
                    return false;
                }
            out->slots[i] = s;
            out->max_probe = std::max(out->max_probe, chain);
        }
    return true;
}

uint32_t lookup_group_table(const GroupTable &table, const uint16_t cell[4], uint32_t book, uint32_t *probes) {
    return group_lookup([&](uint32_t i) { return table.slots[i]; }, uint32_t(table.slots.size() - 1u), table.max_probe, uint32_t(cell[0]) | uint32_t(cell[1]) << 16,
                        uint32_t(cell[2]) | uint32_t(cell[3]) << 16, book, probes);
}

}  // namespace mapf
