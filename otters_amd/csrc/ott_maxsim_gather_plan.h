// ott_maxsim_gather_plan.h — what the host decides for ott_query_maxsim_groups (ott_maxsim_gather.hip) before it
// launches anything: how many tokens share a pass of the gather kernel and what that costs in LDS, the slot arrays of a list of
// groups (ascending, duplicate-free, with each group's extent in the group-to-rows index), the sizes of the two tables, which of
// the two routes a query takes and the 2 GiB refusal; and for ott_query_maxsim_groups_batch (ott_maxsim_batch.hip)
// the slots of a batch of queries, its stride and token width, its route and the split of the slots over the workgroups.  HIP-free:
// tests/test_maxsim_groups_cpu.py and tests/test_maxsim_batch_cpu.py compile it with the host compiler and hold it to a plain
// Python restatement.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ott {

// ---- the gather kernel's geometry ---------------------------------------------------------------------------------------------------
constexpr uint32_t MG_WAVES = 4;                        // waves of a workgroup; a workgroup walks the rows of one listed group at a time
constexpr uint32_t MG_STEP_ROWS = 8 * MG_WAVES;         // eight lanes per row (lane c = chain c of the reference's f32x8): 32 rows per step
constexpr uint32_t MG_DIMQ_MAX = 2048;                  // query floats per token the kernel keeps in LDS
constexpr uint32_t MG_PAD = 4;                          // floats behind the tokens of one dim: the eight 16-B reads of a wave fall in eight bank groups
constexpr uint32_t MG_LDS_MAX = 100 * 1024;             // what the kernel's opt-in asks for: the largest of the three widths below (98.4 KB)

// Tokens per pass: 32 while dimq <= 512, 16 while <= 1024, 8 while <= 2048 — the token floats themselves stay within 64 KB — and no
// wider than the query needs (8, 16 or 32 accumulators per lane: a 3-token query does not pay for 32).  0: the kernel does not serve dimq.
inline uint32_t mg_tokens_cap(uint32_t dimq) { return dimq <= 512 ? 32u : dimq <= 1024 ? 16u : dimq <= MG_DIMQ_MAX ? 8u : 0u; }
inline uint32_t mg_tokens_per_pass(uint32_t dimq, uint32_t nq) {
    const uint32_t cap = mg_tokens_cap(dimq);
    uint32_t w = 8;
    while (w < nq && w < cap) w <<= 1;
    return w < cap ? w : cap;
}
inline uint32_t mg_passes(uint32_t dimq, uint32_t nq) {
    const uint32_t nt = mg_tokens_per_pass(dimq, nq);
    return nt ? (nq + nt - 1) / nt : 0u;
}
// Dynamic LDS of a workgroup: the pass's tokens transposed, [dimq][nt + MG_PAD] (a lane reads four tokens of its dim with one 16-B
// load), the tokens' inverse norms [nt], and the waves' running maxima [MG_WAVES][nt].
inline uint64_t mg_lds_bytes(uint32_t dimq, uint32_t nt) { return ((uint64_t)dimq * (nt + MG_PAD) + nt + (uint64_t)MG_WAVES * nt) * 4; }

// ---- the tables ---------------------------------------------------------------------------------------------------------------------
constexpr uint64_t MG_TABLE_MAX = 1ull << 31;  // bytes of a table of 4-byte ordinals: 2 GiB, ott_query_maxsim's limit
// gather route: ordinals [nq][n_slots] only when the tokens take more than one pass (one pass sums in the kernel); keys [n_slots]
inline uint64_t mg_table_bytes(uint32_t nq, uint64_t n_slots, uint32_t passes) { return passes > 1 ? (uint64_t)nq * n_slots * 4 : 0ull; }
inline uint64_t mg_key_bytes(uint64_t n_slots) { return n_slots * 8; }
// mask route: ott_query_maxsim's own table over every group of the store; above 2 GiB the query is refused
inline bool mg_sweep_table_fits(uint32_t nq, uint32_t n_groups) { return (uint64_t)nq * n_groups * 4 <= MG_TABLE_MAX; }

// ---- the list -----------------------------------------------------------------------------------------------------------------------
// Slot i of a query = the i-th smallest distinct listed group: ascending ids keep "ties go to the lower group" in slot order too.
// Every listed id is < n_groups (the caller has checked).  A list that is not short against the store's groups (n_groups <= 64 x
// its length) is ordered through a bitmap over the groups and one scan of its words, O(list + n_groups / 64), where a sort of
// 50 000 ids took 2 of a query's 3.7 ms; a short list of a store of many groups is sorted.
// With the index's extents (`starts`: [n_groups + 1] prefix sums of the groups' row counts; nullptr = not known) every slot gets its
// rows' place in the index and `rows` the number of listed rows.
struct MgSlots {
    std::vector<uint32_t> gid, start, count;
    uint64_t rows = 0;
};
inline void mg_slots(const uint32_t* groups, uint64_t n_listed, uint32_t n_groups, const uint32_t* starts, MgSlots& out) {
    if ((uint64_t)n_groups <= 64 * n_listed) {
        std::vector<uint64_t> bits(((size_t)n_groups + 63) / 64, 0ull);
        for (uint64_t i = 0; i < n_listed; i++) bits[groups[i] >> 6] |= 1ull << (groups[i] & 63);
        out.gid.clear();
        for (size_t w = 0; w < bits.size(); w++)
            for (uint64_t m = bits[w]; m != 0; m &= m - 1) out.gid.push_back((uint32_t)(w * 64 + (size_t)__builtin_ctzll(m)));
    } else {
        out.gid.assign(groups, groups + n_listed);
        std::sort(out.gid.begin(), out.gid.end());
        out.gid.erase(std::unique(out.gid.begin(), out.gid.end()), out.gid.end());
    }
    out.start.clear();
    out.count.clear();
    out.rows = 0;
    if (!starts) return;
    out.start.reserve(out.gid.size());
    out.count.reserve(out.gid.size());
    for (const uint32_t g : out.gid) {
        out.start.push_back(starts[g]);
        out.count.push_back(starts[g + 1] - starts[g]);
        out.rows += starts[g + 1] - starts[g];
    }
}

// ---- the route ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t MG_INDEX_MAX_GROUPS = 1u << 26;  // the index is built for stores of up to 2^26 groups (its counters and the host's extents: 256 MB each)
constexpr uint64_t MG_MAX_SLOTS = 1ull << 24;       // launch limit: listed groups of one query (the tables' slots)
constexpr uint64_t MG_MAX_ROWS = 1ull << 30;        // launch limit: listed rows of one query
// Option group_gather = -1: the gather while the listed groups hold at most this many rows.  Measured on 2M x 128 in documents of 20,
// 32 tokens, cosine top-10, contiguous and shuffled layouts (profiles/maxsim_rerank/README.md): the gather was faster than the mask
// route at every measured size, the largest being 50 000 documents = 1 000 000 rows (half the store).
constexpr uint64_t MG_AUTO_MAX_ROWS = 1000000;

// May this query ask for the index at all (it is built by the first query that may)?  Decided from the store and the descriptor alone.
inline bool mg_wants_index(bool multi_gpu, bool path_mfma, uint32_t dimq, int group_gather) {
    return !multi_gpu && !path_mfma && mg_tokens_cap(dimq) != 0 && group_gather != 0;
}
// ... and, once the index is there and the list's extents are known: the gather, or the mask route?
inline bool mg_takes_gather(bool wants_index, bool have_index, int group_gather, uint64_t n_slots, uint64_t listed_rows) {
    if (!wants_index || !have_index) return false;
    if (n_slots > MG_MAX_SLOTS || listed_rows > MG_MAX_ROWS) return false;
    return group_gather == 1 || listed_rows <= MG_AUTO_MAX_ROWS;
}

// ---- a batch of queries, each with its own tokens and its own list (ott_query_maxsim_groups_batch) ----------------
// The slots of every query (mg_slots: ascending, duplicate-free, with extents) back to back in query order: slot i belongs to query
// query[i] and is that query's pos[i]-th slot, so its key goes to keys[query[i] * S + pos[i]] with the stride S = the largest number
// of distinct listed groups of any query.  NT: the token width every query of the batch runs at (the widest query decides; a
// narrower query's block is zero padded and its sum stops at its own tokens).
struct MgBatch {
    std::vector<uint32_t> gid, start, count, query, pos;  // [T]; start / count only with the index's extents
    std::vector<uint32_t> tokens, distinct;               // [B]
    std::vector<uint64_t> rows_of;                        // [B] listed rows of the query (0 without the extents)
    uint32_t S = 0, NT = 0, max_tokens = 0;
    uint64_t rows = 0;      // listed rows of all queries
    uint64_t compared = 0;  // sum over the queries of listed rows x tokens
};
inline void mg_batch_build(const uint32_t* groups, const uint32_t* tokens_per_query, const uint64_t* listed_per_query, uint32_t n_queries, uint32_t n_groups,
                           const uint32_t* starts, uint32_t dimq, MgBatch& out) {
    out = MgBatch();
    out.tokens.assign(tokens_per_query, tokens_per_query + n_queries);
    out.distinct.resize(n_queries);
    out.rows_of.resize(n_queries);
    MgSlots sl;
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_queries; b++) {
        mg_slots(groups + at, listed_per_query[b], n_groups, starts, sl);
        at += listed_per_query[b];
        const uint32_t n = (uint32_t)sl.gid.size();  // (distinct ids of a store of fewer than 2^32 groups)
        out.distinct[b] = n;
        out.rows_of[b] = sl.rows;
        out.rows += sl.rows;
        out.compared += sl.rows * tokens_per_query[b];
        out.S = std::max(out.S, n);
        out.max_tokens = std::max(out.max_tokens, tokens_per_query[b]);
        out.gid.insert(out.gid.end(), sl.gid.begin(), sl.gid.end());
        out.start.insert(out.start.end(), sl.start.begin(), sl.start.end());
        out.count.insert(out.count.end(), sl.count.begin(), sl.count.end());
        out.query.insert(out.query.end(), n, b);
        for (uint32_t i = 0; i < n; i++) out.pos.push_back(i);
    }
    out.NT = mg_tokens_per_pass(dimq, out.max_tokens);
}
// The batched gather serves the batch when every query fits one token pass (the sum is made in the kernel; the [nq][n_slots] table
// of a second pass is not carried over), the key table and the rows stay within the launch limits, and the option says so: 1, or -1
// and every query alone would take the gather — a batch of queries that each prefer the gather only loses per-call overheads.
// Everything else is answered query by query (the loop route).
inline bool mg_batch_takes_gather(bool wants_index, bool have_index, int group_gather, uint32_t dimq, const MgBatch& mb) {
    if (!wants_index || !have_index) return false;
    if (mb.max_tokens > mg_tokens_cap(dimq)) return false;
    if ((uint64_t)mb.tokens.size() * mb.S > MG_MAX_SLOTS || mb.rows > MG_MAX_ROWS) return false;
    if (group_gather == 1) return true;
    for (const uint64_t r : mb.rows_of)
        if (r > MG_AUTO_MAX_ROWS) return false;
    return true;
}
// Workgroup w of n_workgroups walks the contiguous slots [first[w], first[w + 1]) (first: n_workgroups + 1 entries), balanced by
// listed rows: slot i weighs counts[i] + 1 (an empty group still costs a visit), P[i] = the weight before slot i, W = the total, and
// first[w] = the number of slots with P[i] x n_workgroups < w x W.  Every slot belongs to exactly one workgroup, first never
// decreases, and a workgroup's weight differs from W / n_workgroups by less than the heaviest slot's.
inline void mg_batch_split(const uint32_t* counts, uint64_t T, uint32_t n_workgroups, uint32_t* first) {
    uint64_t W = 0;
    for (uint64_t i = 0; i < T; i++) W += (uint64_t)counts[i] + 1;  // (at most MG_MAX_ROWS + MG_MAX_SLOTS: the products below fit 64 bits)
    uint64_t i = 0, P = 0;
    for (uint32_t w = 0; w <= n_workgroups; w++) {
        while (i < T && P * n_workgroups < (uint64_t)w * W) P += (uint64_t)counts[i++] + 1;
        first[w] = (uint32_t)i;
    }
}

}  // namespace ott
