// Greedy representatives of an edge list, the CPU side (include/bsq.h, "greedy representatives"): bsq_greedy_pairs_host, the rule as the
// plain sequential visit -- order the nodes, collect every node's earlier neighbours, walk the order once -- and not a restatement of
// the rounds of bsq_greedy.hip, and the host-only bsq_greedy_scratch_bytes.  Plain C++: neither this file nor bsq_greedy_dev.h needs
// the HIP headers.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "bsq.h"
#include "bsq_greedy_dev.h"

extern "C" {

int64_t bsq_greedy_scratch_bytes(int64_t n, int64_t n_pairs) {
    if (n < 0 || n > bsq_greedyd::kMaxRows || n_pairs < 0) return -BSQ_ERR_INVALID_ARG;
    return static_cast<int64_t>(bsq_greedyd::scratch_bytes(n));  // (no copy of the list is kept: the size does not depend on n_pairs)
}

bsq_status bsq_greedy_pairs_host(const int64_t *row, const int64_t *col, const int32_t *weight_or_null, int64_t n_pairs, int64_t n,
                                 const int64_t *key_or_null, int64_t *rep) {
    const char *why = "";
    const bsq_status st = bsq_greedyd::check_list(row, col, n_pairs, n, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n == 0) return BSQ_OK;
    if (!rep) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "rep is null");
    const int64_t *key = key_or_null;
    // the order, and each node's place in it
    std::vector<int64_t> order(static_cast<size_t>(n)), place(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) order[static_cast<size_t>(i)] = i;
    if (key) std::sort(order.begin(), order.end(), [key](int64_t u, int64_t v) { return bsq_greedyd::before(key, u, v); });
    for (int64_t p = 0; p < n; ++p) place[static_cast<size_t>(order[static_cast<size_t>(p)])] = p;
    // the earlier neighbours of every node, as a CSR over the later end of each entry
    std::vector<int64_t> first(static_cast<size_t>(n) + 1, 0);
    for (int64_t k = 0; k < n_pairs; ++k)
        if (bsq_greedyd::edge_links(row[k], col[k], n))
            ++first[static_cast<size_t>(place[static_cast<size_t>(row[k])] < place[static_cast<size_t>(col[k])] ? col[k] : row[k]) + 1];
    for (int64_t i = 0; i < n; ++i) first[static_cast<size_t>(i) + 1] += first[static_cast<size_t>(i)];
    std::vector<int64_t> fill(first.begin(), first.end() - 1), nb(static_cast<size_t>(first[static_cast<size_t>(n)]));
    std::vector<int32_t> nw(weight_or_null ? nb.size() : 0);
    for (int64_t k = 0; k < n_pairs; ++k) {
        if (!bsq_greedyd::edge_links(row[k], col[k], n)) continue;
        const bool fwd = place[static_cast<size_t>(row[k])] < place[static_cast<size_t>(col[k])];
        const int64_t u = fwd ? row[k] : col[k], v = fwd ? col[k] : row[k], at = fill[static_cast<size_t>(v)]++;
        nb[static_cast<size_t>(at)] = u;
        if (weight_or_null) nw[static_cast<size_t>(at)] = weight_or_null[k];
    }
    // the visit: rep[v] < 0 until v is visited; a visited u is a representative iff rep[u] == u
    for (int64_t i = 0; i < n; ++i) rep[i] = -1;
    for (int64_t p = 0; p < n; ++p) {
        const int64_t v = order[static_cast<size_t>(p)];
        int64_t best = -1;
        int32_t best_w = 0;
        for (int64_t e = first[static_cast<size_t>(v)]; e < first[static_cast<size_t>(v) + 1]; ++e) {
            const int64_t u = nb[static_cast<size_t>(e)];
            if (rep[u] != u) continue;
            const int32_t w = weight_or_null ? nw[static_cast<size_t>(e)] : 0;
            if (best < 0 || w > best_w || (w == best_w && place[static_cast<size_t>(u)] < place[static_cast<size_t>(best)])) best = u, best_w = w;
        }
        rep[v] = best < 0 ? v : best;
    }
    return BSQ_OK;
}

}  // extern "C"
