// Stand-alone check of bsq_greedy_pairs_host and bsq_greedy_scratch_bytes (bsq_greedy_host.cpp) for a sanitizer build
// (tests/test_greedy_native.py compiles both with -fsanitize=address,undefined): generated edge lists with duplicates, both orientations,
// self-entries and indices out of range at both ends of int64, with and without keys and weights, against a reference of its own written
// from the rule of include/bsq.h ("greedy representatives") -- the nodes sorted by (key, index), and for every node in turn a scan of the
// WHOLE list for its entries, no adjacency structure.  Every input and output array is a heap block of its exact size, so a read past
// the list, the key or the weights, a node looked up from an index out of range, or a write past rep is an error.  Needs no HIP header.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "bsq.h"

namespace bsq_internal {
static std::string g_last;
bsq_status set_error(bsq_status st, const char *msg) {
    g_last = msg;
    return st;
}
}  // namespace bsq_internal

namespace {

uint64_t next(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

std::vector<int64_t> reference(int64_t n, const std::vector<int64_t> &row, const std::vector<int64_t> &col, const int64_t *key, const int32_t *weight) {
    std::vector<int64_t> order(static_cast<size_t>(n)), rep(static_cast<size_t>(n), -1);
    for (int64_t i = 0; i < n; ++i) order[size_t(i)] = i;
    auto before = [key](int64_t u, int64_t v) { return key && key[u] != key[v] ? key[u] < key[v] : u < v; };
    std::stable_sort(order.begin(), order.end(), before);
    for (int64_t v : order) {
        int64_t best = -1, best_w = 0;
        for (size_t k = 0; k < row.size(); ++k) {
            const int64_t i = row[k], j = col[k];
            if (i == j || i < 0 || j < 0 || i >= n || j >= n || (i != v && j != v)) continue;
            const int64_t u = i == v ? j : i, w = weight ? weight[k] : 0;
            if (rep[size_t(u)] != u) continue;  // (not visited yet, or a member)
            if (best < 0 || w > best_w || (w == best_w && u != best && before(u, best))) best = u, best_w = w;
        }
        rep[size_t(v)] = best < 0 ? v : best;
    }
    return rep;
}

int check(int64_t n, int64_t m, uint64_t seed, bool has_key, bool has_weight, int64_t *members) {
    uint64_t state = seed;
    std::vector<int64_t> row, col;
    const int64_t junk[8][2] = {{0, 0}, {n - 1, n - 1}, {-1, 0}, {0, n}, {INT64_MIN, 0}, {INT64_MAX, n - 1}, {n - 1, INT64_MIN}, {0, INT64_MAX}};
    for (const auto &p : junk) row.push_back(p[0]), col.push_back(p[1]);
    for (int64_t k = 0; k < m; ++k) row.push_back(int64_t(next(state) % uint64_t(n))), col.push_back(int64_t(next(state) % uint64_t(n)));
    for (int64_t k = 0; k < m / 4; ++k) row.push_back(col[size_t(8 + k)]), col.push_back(row[size_t(8 + k)]);  // duplicates, ends exchanged
    for (const auto &p : junk) row.push_back(p[1]), col.push_back(p[0]);
    const size_t len = row.size();
    int64_t *r = new int64_t[len], *c = new int64_t[len], *key = has_key ? new int64_t[size_t(n)] : nullptr, *rep = new int64_t[size_t(n)];  // (exact sizes)
    int32_t *w = has_weight ? new int32_t[len] : nullptr;
    for (size_t k = 0; k < len; ++k) r[k] = row[k], c[k] = col[k];
    for (int64_t i = 0; has_key && i < n; ++i) key[i] = i % 11 == 0 ? INT64_MIN : i % 13 == 0 ? INT64_MAX : int64_t(next(state) % 5) - 2;
    for (size_t k = 0; has_weight && k < len; ++k) w[k] = k % 17 == 0 ? INT32_MIN : k % 19 == 0 ? INT32_MAX : int32_t(next(state) % 4) - 2;
    const std::vector<int64_t> want = reference(n, row, col, key, w);
    int bad = bsq_greedy_pairs_host(r, c, w, int64_t(len), n, key, rep) != BSQ_OK;
    for (int64_t i = 0; i < n; ++i) bad += rep[i] != want[size_t(i)], *members += want[size_t(i)] != i;
    if (bad) std::printf("FAILED: n %lld m %lld key %d weight %d: %d mismatches\n", (long long)n, (long long)m, int(has_key), int(has_weight), bad);
    delete[] r;
    delete[] c;
    delete[] key;
    delete[] rep;
    delete[] w;
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t members = 0;
    const int64_t shapes[6][2] = {{1, 0}, {2, 3}, {5, 40}, {64, 100}, {257, 2000}, {1000, 1500}};
    for (const auto &s : shapes)
        for (int mode = 0; mode < 4; ++mode) bad += check(s[0], s[1], uint64_t(s[0] * 977 + s[1]), mode & 1, mode & 2, &members);
    if (members < 1000) ++bad;  // (a check of nothing)
    // the header's known answers
    {
        const int64_t a[4] = {0, 1, 2, 3}, b[4] = {1, 2, 3, 4}, key[5] = {0, 0, 0, -1, 0}, want[5] = {0, 0, 2, 2, 4}, want_key[5] = {0, 0, 3, 3, 3};
        int64_t rep[5];
        bad += bsq_greedy_pairs_host(a, b, nullptr, 4, 5, nullptr, rep) != BSQ_OK;
        for (int i = 0; i < 5; ++i) bad += rep[i] != want[i];
        bad += bsq_greedy_pairs_host(a, b, nullptr, 4, 5, key, rep) != BSQ_OK;
        for (int i = 0; i < 5; ++i) bad += rep[i] != want_key[i];
        const int64_t r2[2] = {0, 1}, c2[2] = {2, 2};
        const int32_t w2[2] = {1, 5};
        bad += bsq_greedy_pairs_host(r2, c2, w2, 2, 3, nullptr, rep) != BSQ_OK || rep[0] != 0 || rep[1] != 1 || rep[2] != 1;
    }
    // the argument rules: a refusal writes nothing
    int64_t rep[4] = {7, 7, 7, 7}, edges[2] = {0, 1};
    bad += bsq_greedy_pairs_host(edges, edges, nullptr, -1, 4, nullptr, rep) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(edges, edges, nullptr, 2, -1, nullptr, rep) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(edges, edges, nullptr, 2, int64_t(1) << 31, nullptr, rep) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(nullptr, edges, nullptr, 2, 4, nullptr, rep) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(edges, nullptr, nullptr, 2, 4, nullptr, rep) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(edges, edges, nullptr, 2, 4, nullptr, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_greedy_pairs_host(edges, edges, nullptr, 2, 0, nullptr, rep) != BSQ_OK;
    for (int64_t v : rep) bad += v != 7;
    bad += bsq_greedy_pairs_host(nullptr, nullptr, nullptr, 0, 4, nullptr, rep) != BSQ_OK;  // no entries: every node its own representative
    for (int k = 0; k < 4; ++k) bad += rep[k] != k;
    bad += bsq_greedy_scratch_bytes(10, 99) != 64 + 280 || bsq_greedy_scratch_bytes(-1, 0) >= 0 || bsq_greedy_scratch_bytes(0, -1) >= 0;
    bad += bsq_greedy_scratch_bytes(int64_t(1) << 31, 0) >= 0 || bsq_greedy_scratch_bytes((int64_t(1) << 31) - 1, 0) != 64 + 28 * ((int64_t(1) << 31) - 1);
    if (bad) {
        std::printf("GREEDY_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("GREEDY_HOST_OK\n");
    return 0;
}
