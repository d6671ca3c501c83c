// Stand-alone check of bsq_sketch_pairs_host (bsq_sketch_host.cpp) for a sanitizer build (tests/test_sketch_pairs_native.py compiles both
// with -fsanitize=address,undefined): generated sketch matrices of both element types through the pair list -- cross and upper, every
// kind of threshold, cut at several capacities -- against plain loops written from the rule of include/bsq.h ("sketch pairs").  Every
// input and output array is a heap block of its exact size, so a read past a matrix or a write past a capacity is an error.  Needs no
// HIP header.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

struct Pair {
    int64_t i, j;
    int32_t match, either;
};

uint64_t next(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

// (B, S) values from a small set with EMPTY in it, so that matches are plentiful; row 1 EMPTY throughout, rows 0 and B - 1 equal
std::vector<uint32_t> matrix(int64_t B, int64_t S, uint64_t seed) {
    static const uint32_t values[6] = {EMPTY, 0u, 1u, 2u, 0x80000000u, 0xFFFFFFFEu};
    std::vector<uint32_t> m(size_t(B * S));
    uint64_t state = seed;
    for (uint32_t &v : m) v = values[next(state) % 6];
    if (B > 2) {
        for (int64_t t = 0; t < S; ++t) m[size_t(S + t)] = EMPTY;
        for (int64_t t = 0; t < S; ++t) m[size_t((B - 1) * S + t)] = m[size_t(t)];
    }
    return m;
}

// the rule, word for word
std::vector<Pair> reference(const std::vector<uint32_t> &a, int64_t Ba, const std::vector<uint32_t> &b, int64_t Bb, int64_t S, const bsq_sketch_pairs &r,
                            std::vector<int64_t> *offsets) {
    std::vector<Pair> out;
    offsets->assign(size_t(Ba) + 1, 0);
    for (int64_t i = 0; i < Ba; ++i) {
        for (int64_t j = 0; j < Bb; ++j) {
            if (r.upper && j <= i) continue;
            int64_t m = 0, e = 0;
            for (int64_t t = 0; t < S; ++t) {
                const uint32_t x = a[size_t(i * S + t)], y = b[size_t(j * S + t)];
                m += x == y && x != EMPTY;
                e += x != EMPTY || y != EMPTY;
            }
            if (m >= r.min_match && m * 65536 >= int64_t(r.jaccard_q16) * e) out.push_back({i, j, int32_t(m), int32_t(e)});
        }
        (*offsets)[size_t(i) + 1] = int64_t(out.size());
    }
    return out;
}

template <typename T>
int check_type(const std::vector<uint32_t> &ua, int64_t Ba, const std::vector<uint32_t> &ub, int64_t Bb, int64_t S, const bsq_sketch_pairs &r,
               bsq_dtype t) {
    T *a = new T[ua.size()], *b = new T[ub.size()];  // (exact sizes)
    for (size_t k = 0; k < ua.size(); ++k) a[k] = sizeof(T) == 8 && ua[k] == EMPTY ? T(~uint64_t(0)) : T(ua[k]);
    for (size_t k = 0; k < ub.size(); ++k) b[k] = sizeof(T) == 8 && ub[k] == EMPTY ? T(~uint64_t(0)) : T(ub[k]);
    std::vector<int64_t> want_offsets;
    const std::vector<Pair> want = reference(ua, Ba, ub, Bb, S, r, &want_offsets);
    const int64_t total = int64_t(want.size());
    int bad = 0;
    for (int64_t cap : {int64_t(0), int64_t(1), total - 1, total, total + 7}) {
        if (cap < 0) continue;
        int64_t *offsets = new int64_t[size_t(Ba) + 1], *row = new int64_t[size_t(cap)], *col = new int64_t[size_t(cap)];
        int32_t *match = new int32_t[size_t(cap)], *either = new int32_t[size_t(cap)];
        for (int64_t k = 0; k < cap; ++k) row[k] = col[k] = -7, match[k] = either[k] = -7;
        const bool with_either = cap != 1;
        if (bsq_sketch_pairs_host(a, Ba, r.upper ? a : b, Bb, S, t, &r, offsets, cap, cap ? row : nullptr, cap ? col : nullptr, cap ? match : nullptr,
                                  with_either && cap ? either : nullptr) != BSQ_OK)
            ++bad;
        for (int64_t i = 0; i <= Ba; ++i) bad += offsets[i] != want_offsets[size_t(i)];
        for (int64_t k = 0; k < cap; ++k) {
            if (k < total) {
                const Pair &p = want[size_t(k)];
                bad += row[k] != p.i || col[k] != p.j || match[k] != p.match || (with_either && either[k] != p.either);
            } else {
                bad += row[k] != -7 || col[k] != -7 || match[k] != -7 || either[k] != -7;  // (nothing is written behind the list)
            }
        }
        delete[] offsets;
        delete[] row;
        delete[] col;
        delete[] match;
        delete[] either;
    }
    delete[] a;
    delete[] b;
    return bad;
}

int check(int64_t Ba, int64_t Bb, int64_t S, bsq_sketch_pairs r, int64_t *listed) {
    const std::vector<uint32_t> a = matrix(Ba, S, uint64_t(Ba * 131 + S)), b = r.upper ? a : matrix(Bb, S, uint64_t(Bb * 17 + S + 1));
    std::vector<int64_t> offsets;
    *listed += int64_t(reference(a, Ba, b, Bb, S, r, &offsets).size());
    const int bad = check_type<int32_t>(a, Ba, b, Bb, S, r, BSQ_I32) + check_type<uint64_t>(a, Ba, b, Bb, S, r, BSQ_U64);
    if (bad) std::printf("FAILED: %lld x %lld x %lld min_match %d T %d upper %d: %d mismatches\n", (long long)Ba, (long long)Bb, (long long)S,
                         r.min_match, r.jaccard_q16, r.upper, bad);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t listed = 0;
    const int64_t shapes[5][3] = {{1, 1, 1}, {3, 5, 7}, {65, 130, 100}, {7, 9, 16384}, {70, 70, 33}};
    for (const auto &s : shapes)
        for (int32_t upper = 0; upper < 2; ++upper) {
            if (upper && s[0] != s[1]) continue;
            const int32_t S = int32_t(s[2]);
            for (const bsq_sketch_pairs &r : {bsq_sketch_pairs{0, 0, upper, 0}, bsq_sketch_pairs{S < 2 ? S : 2, 16384, upper, 0},
                                              bsq_sketch_pairs{1, 65536, upper, 3}, bsq_sketch_pairs{S, 65536, upper, 64}})
                bad += check(s[0], s[1], s[2], r, &listed);
        }
    if (listed < 1000) ++bad;  // (a check of nothing)
    // the argument rules: a refusal writes nothing
    const std::vector<uint32_t> m = matrix(4, 8, 1);
    int64_t offsets[5] = {7, 7, 7, 7, 7}, row[4] = {7, 7, 7, 7}, col[4] = {7, 7, 7, 7};
    int32_t match[4] = {7, 7, 7, 7};
    const bsq_sketch_pairs rules[8] = {{-1, 0, 0, 0}, {9, 0, 0, 0}, {1, -1, 0, 0}, {1, 65537, 0, 0}, {1, 0, 2, 0}, {1, 0, 1, 0}, {1, 0, 0, -1}, {1, 0, 0, 65}};
    for (const bsq_sketch_pairs &r : rules)
        bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), r.upper == 1 ? 3 : 4, 8, BSQ_I32, &r, offsets, 4, row, col, match, nullptr) != BSQ_ERR_INVALID_ARG;
    const bsq_sketch_pairs ok = {1, 0, 0, 0};
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 8, BSQ_F32, &ok, offsets, 4, row, col, match, nullptr) != BSQ_ERR_DTYPE;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 0, BSQ_I32, &ok, offsets, 4, row, col, match, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 8, BSQ_I32, &ok, nullptr, 4, row, col, match, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 8, BSQ_I32, &ok, offsets, -1, row, col, match, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 8, BSQ_I32, &ok, offsets, 4, row, nullptr, match, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 4, 8, BSQ_I32, nullptr, offsets, 4, row, col, match, nullptr) != BSQ_ERR_INVALID_ARG;
    for (int k = 0; k < 4; ++k) bad += row[k] != 7 || col[k] != 7 || match[k] != 7;
    for (int64_t v : offsets) bad += v != 7;
    bad += bsq_sketch_pairs_host(m.data(), 4, m.data(), 0, 8, BSQ_I32, &ok, offsets, 4, row, col, match, nullptr) != BSQ_OK;  // an empty side
    for (int64_t v : offsets) bad += v != 0;
    bad += bsq_sketch_pairs_segments(200, 330, 64) != 6 || bsq_sketch_pairs_segments(200, 330, 0) != 6 || bsq_sketch_pairs_segments(5, 5, 65) != 0;
    if (bad) {
        std::printf("SKETCH_PAIRS_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("SKETCH_PAIRS_HOST_OK\n");
    return 0;
}
