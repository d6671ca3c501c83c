// Stand-alone check of bsq_sketch_clusters_host and bsq_cluster_pairs_host (bsq_sketch_host.cpp) for a sanitizer build
// (tests/test_sketch_clusters_native.py compiles both with -fsanitize=address,undefined): generated sketch matrices of both element types
// and edge lists with padding, self-edges and indices out of range, against a reference of its own written from the rule of include/bsq.h
// ("sketch clusters") -- the smallest index reachable over links, by repeated sweeps over the adjacency until nothing changes, no
// union-find.  Every input and output array is a heap block of its exact size, so a read past a matrix or a list, a parent looked up
// from an index out of range, or a write past the labels is an error.  Needs no HIP header.
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

const uint32_t EMPTY = 0xFFFFFFFFu;

uint64_t next(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

// (B, S) rows that each copy one of `kinds` base rows and then change `edits` buckets, so that rows of one kind are linked in chains
// and stars at a middle threshold; row 1 EMPTY throughout
std::vector<uint32_t> matrix(int64_t B, int64_t S, int64_t kinds, int64_t edits, uint64_t seed) {
    std::vector<uint32_t> m(size_t(B * S));
    uint64_t state = seed;
    for (int64_t i = 0; i < B; ++i) {
        const uint64_t kind = next(state) % uint64_t(kinds);
        for (int64_t t = 0; t < S; ++t) m[size_t(i * S + t)] = uint32_t(kind * 1000 + uint64_t(t)) | (t % 5 == 4 ? EMPTY : 0u);
        for (int64_t e = 0; e < edits; ++e) m[size_t(i * S) + size_t(next(state) % uint64_t(S))] = uint32_t(next(state) % 7) + 0x80000000u;
    }
    if (B > 2)
        for (int64_t t = 0; t < S; ++t) m[size_t(S + t)] = EMPTY;
    return m;
}

bool passes(const std::vector<uint32_t> &a, int64_t S, int64_t i, int64_t j, const bsq_sketch_pairs &r) {
    int64_t m = 0, e = 0;
    for (int64_t t = 0; t < S; ++t) {
        const uint32_t x = a[size_t(i * S + t)], y = a[size_t(j * S + t)];
        m += x == y && x != EMPTY;
        e += x != EMPTY || y != EMPTY;
    }
    return m >= r.min_match && m * 65536 >= int64_t(r.jaccard_q16) * e;
}

// the smallest index reachable: every link hands the smaller label to both ends until a sweep changes nothing
std::vector<int64_t> reference(int64_t n, const std::vector<int64_t> &row, const std::vector<int64_t> &col) {
    std::vector<int64_t> label(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) label[size_t(i)] = i;
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t k = 0; k < row.size(); ++k) {
            const int64_t i = row[k], j = col[k];
            if (i == j || i < 0 || j < 0 || i >= n || j >= n) continue;
            const int64_t low = label[size_t(i)] < label[size_t(j)] ? label[size_t(i)] : label[size_t(j)];
            changed |= label[size_t(i)] != low || label[size_t(j)] != low;
            label[size_t(i)] = label[size_t(j)] = low;
        }
    }
    return label;
}

int check_list(int64_t n, const std::vector<int64_t> &row, const std::vector<int64_t> &col, const std::vector<int64_t> &want) {
    int64_t *r = new int64_t[row.size()], *c = new int64_t[col.size()], *labels = new int64_t[size_t(n)];  // (exact sizes)
    for (size_t k = 0; k < row.size(); ++k) r[k] = row[k], c[k] = col[k];
    int bad = bsq_cluster_pairs_host(r, c, int64_t(row.size()), n, labels) != BSQ_OK;
    for (int64_t i = 0; i < n; ++i) bad += labels[i] != want[size_t(i)];
    delete[] r;
    delete[] c;
    delete[] labels;
    return bad;
}

template <typename T>
int check_type(const std::vector<uint32_t> &ua, int64_t B, int64_t S, const bsq_sketch_pairs &r, bsq_dtype t, const std::vector<int64_t> &want) {
    T *a = new T[ua.size()];
    for (size_t k = 0; k < ua.size(); ++k) a[k] = sizeof(T) == 8 && ua[k] == EMPTY ? T(~uint64_t(0)) : T(ua[k]);
    int64_t *labels = new int64_t[size_t(B)];
    int bad = bsq_sketch_clusters_host(a, B, S, t, &r, labels) != BSQ_OK;
    for (int64_t i = 0; i < B; ++i) bad += labels[i] != want[size_t(i)];
    delete[] a;
    delete[] labels;
    return bad;
}

int check(int64_t B, int64_t S, int64_t kinds, int64_t edits, bsq_sketch_pairs r, int64_t *linked, int64_t *clusters) {
    const std::vector<uint32_t> a = matrix(B, S, kinds, edits, uint64_t(B * 131 + S));
    std::vector<int64_t> row, col;
    for (int64_t i = 0; i < B; ++i)
        for (int64_t j = i + 1; j < B; ++j)
            if (passes(a, S, i, j, r)) row.push_back(i), col.push_back(j);
    const std::vector<int64_t> want = reference(B, row, col);
    *linked += int64_t(row.size());
    for (int64_t i = 0; i < B; ++i) *clusters += want[size_t(i)] == i;
    int bad = check_type<int32_t>(a, B, S, r, BSQ_I32, want) + check_type<uint64_t>(a, B, S, r, BSQ_U64, want);
    bad += check_list(B, row, col, want);
    // the list backwards with its ends exchanged, padded with (0, 0), self-edges and indices out of range on both sides
    std::vector<int64_t> r2, c2;
    const int64_t junk[6][2] = {{0, 0}, {B - 1, B - 1}, {-1, 0}, {0, B}, {INT64_MIN, 0}, {INT64_MAX, B - 1}};
    for (const auto &p : junk) r2.push_back(p[0]), c2.push_back(p[1]);
    for (size_t k = row.size(); k-- > 0;) r2.push_back(col[k]), c2.push_back(row[k]);
    for (const auto &p : junk) r2.push_back(p[1]), c2.push_back(p[0]);
    bad += check_list(B, r2, c2, want);
    if (bad) std::printf("FAILED: %lld x %lld min_match %d T %d: %d mismatches\n", (long long)B, (long long)S, r.min_match, r.jaccard_q16, bad);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t linked = 0, clusters = 0;
    const int64_t shapes[5][4] = {{1, 1, 1, 0}, {3, 7, 2, 1}, {65, 100, 6, 30}, {7, 16384, 2, 5000}, {200, 33, 9, 9}};
    for (const auto &s : shapes) {
        const int32_t S = int32_t(s[1]);
        for (const bsq_sketch_pairs &r : {bsq_sketch_pairs{0, 0, 1, 0}, bsq_sketch_pairs{S < 2 ? S : 2, 32768, 1, 0}, bsq_sketch_pairs{1, 45000, 1, 3},
                                          bsq_sketch_pairs{1, 65536, 1, 64}, bsq_sketch_pairs{S, 65536, 1, 0}})
            bad += check(s[0], s[1], s[2], s[3], r, &linked, &clusters);
    }
    if (linked < 1000 || clusters < 300) ++bad;  // (a check of nothing)
    // the argument rules: a refusal writes nothing
    const std::vector<uint32_t> m = matrix(4, 8, 2, 1, 1);
    int64_t labels[4] = {7, 7, 7, 7}, edges[2] = {0, 1};
    const bsq_sketch_pairs rules[8] = {{1, 0, 0, 0}, {1, 0, 2, 0}, {-1, 0, 1, 0}, {9, 0, 1, 0}, {1, -1, 1, 0}, {1, 65537, 1, 0}, {1, 0, 1, -1}, {1, 0, 1, 65}};
    for (const bsq_sketch_pairs &r : rules) bad += bsq_sketch_clusters_host(m.data(), 4, 8, BSQ_I32, &r, labels) != BSQ_ERR_INVALID_ARG;
    const bsq_sketch_pairs ok = {1, 0, 1, 0};
    bad += bsq_sketch_clusters_host(m.data(), 4, 8, BSQ_F32, &ok, labels) != BSQ_ERR_DTYPE;
    bad += bsq_sketch_clusters_host(m.data(), 4, 0, BSQ_I32, &ok, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_clusters_host(m.data(), -1, 8, BSQ_I32, &ok, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_clusters_host(m.data(), 4, 8, BSQ_I32, &ok, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_clusters_host(m.data(), 4, 8, BSQ_I32, nullptr, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_clusters_host(m.data(), 0, 8, BSQ_I32, &ok, labels) != BSQ_OK;  // B == 0 writes nothing
    bad += bsq_cluster_pairs_host(edges, edges, -1, 4, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_cluster_pairs_host(edges, edges, 2, -1, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_cluster_pairs_host(nullptr, edges, 2, 4, labels) != BSQ_ERR_INVALID_ARG;
    bad += bsq_cluster_pairs_host(edges, edges, 2, 4, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_cluster_pairs_host(edges, edges, 2, 0, labels) != BSQ_OK;
    for (int64_t v : labels) bad += v != 7;
    bad += bsq_cluster_pairs_host(nullptr, nullptr, 0, 4, labels) != BSQ_OK;  // no edges: every node its own label
    for (int k = 0; k < 4; ++k) bad += labels[k] != k;
    if (bad) {
        std::printf("SKETCH_CLUSTERS_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("SKETCH_CLUSTERS_HOST_OK\n");
    return 0;
}
