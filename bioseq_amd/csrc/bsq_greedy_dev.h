// Greedy representatives of an edge list (include/bsq.h, "greedy representatives"): what the kernels of bsq_greedy.hip and the CPU twin of
// bsq_greedy_host.cpp share -- the order of two nodes, the states, the round stamps, the layout of the caller-owned scratch and the
// argument rules.  Plain C++ over <cstdint>, bsq.h and bsq_sketch_dev.h (the list's own convention, edge_links): the twin compiles
// without the HIP headers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bsq.h"
#include "bsq_sketch_dev.h"

namespace bsq_greedyd {

using bsq_sketchd::edge_links;  // row != col and both inside 0 .. n - 1: every other entry is ignored and never dereferenced
using bsq_sketchd::kMaxRows;    // n <= 2^31 - 1: a node index fits the 32-bit words of the scratch

// u comes before v when (key[u], u) < (key[v], v); key == nullptr is index order
BSQ_SKETCH_HD bool before(const int64_t *key, int64_t u, int64_t v) {
    if (!key) return u < v;
    const int64_t ku = key[u], kv = key[v];
    return ku < kv || (ku == kv && u < v);
}

// a node's state word
constexpr uint32_t kUndecided = 0, kRep = 1, kMember = 2;
// Round t (0-based over the whole run) stamps mark[v] with stamp(t) where an earlier neighbour of v is still UNDECIDED and with
// stamp(t) + 1 where one is REP: stamps grow with t and the clean mark is 0 < stamp(0), so nothing is cleared between rounds.
BSQ_SKETCH_HD uint32_t stamp(int64_t t) { return static_cast<uint32_t>(2 * (t + 1)); }
constexpr int64_t kMaxRounds = (int64_t(1) << 30) - 1;  // round0 + rounds: stamp(kMaxRounds - 1) + 1 = 2^31 - 1, the last value of 31 bits

// the words an assignment starts from: no weight, no key and no index seen yet
constexpr int32_t kNoWeight = INT32_MIN;
constexpr int64_t kNoKey = INT64_MAX;
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

// The scratch: a head of 64 bytes, then one int64 and five 32-bit words per node.  Every word of it is a whole 32- or 64-bit word of
// ONE node or one counter: no two nodes share a word.
//   count[2]   head, uint32: count[t & 1] = the nodes round t left UNDECIDED; round t reads count[(t - 1) & 1] and zeroes its own word
//   best_key   int64[n]   the assignment's smallest key among a member's candidates
//   state      uint32[n]  kUndecided / kRep / kMember            (the run: kept from call to call)
//   mark       uint32[n]  the round stamps                       (the run: kept from call to call)
//   best_w     int32[n]   the assignment's largest weight        (the assignment's words are cleared by every call)
//   best_i     uint32[n]  the assignment's first candidate
//   pending    uint32[n]  1: a member with an earlier neighbour that is still UNDECIDED -- its representative is not final yet
constexpr size_t kHeadBytes = 64;
struct Scratch {
    uint32_t *count;
    int64_t *best_key;
    uint32_t *state, *mark;
    int32_t *best_w;
    uint32_t *best_i, *pending;
};
inline size_t scratch_bytes(int64_t n) { return kHeadBytes + static_cast<size_t>(n) * (sizeof(int64_t) + 5 * sizeof(uint32_t)); }
inline Scratch carve(void *scratch, int64_t n) {
    char *p = static_cast<char *>(scratch);
    Scratch s;
    s.count = reinterpret_cast<uint32_t *>(p);
    s.best_key = reinterpret_cast<int64_t *>(p + kHeadBytes);
    s.state = reinterpret_cast<uint32_t *>(s.best_key + n);
    s.mark = s.state + n;
    s.best_w = reinterpret_cast<int32_t *>(s.mark + n);
    s.best_i = reinterpret_cast<uint32_t *>(s.best_w + n);
    s.pending = s.best_i + n;
    return s;
}

// The rules of the list and the order that the device call and the twin share.  Host only.
inline bsq_status check_list(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, const char **why) {
    if (n_pairs < 0 || n < 0) return *why = "negative n_pairs or n", BSQ_ERR_INVALID_ARG;
    if (n > kMaxRows) return *why = "n exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && (!row || !col)) return *why = "row or col is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_greedyd
