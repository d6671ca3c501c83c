// Stand-alone check of bsq_edit_pairs_host (bsq_edit_host.cpp) for a sanitizer build (tests/test_edit_native.py compiles both with
// -fsanitize=address,undefined): generated pairs of rows -- unrelated, mutated copies, runs of one letter -- around the block edges of
// the bit-vector code, through both stores and every code, against the plain dynamic programme written from the rule of include/bsq.h
// ("edit distance of row pairs").  Every input and output array is a heap block of its exact size, so a read past a store or a write
// past dist is an error.  Needs no HIP header.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bsq.h"
#include "bsq_edit_dev.h"

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

// a descriptor made by hand (bsq_alphabet.cpp is not linked): `letters` are the classes 0 .. in both cases, everything else unmapped
bsq_desc make_desc(const char *letters) {
    bsq_desc d;
    std::memset(&d, 0, sizeof d);
    std::memset(d.lut, -1, sizeof d.lut);
    int32_t n = 0;
    for (const char *p = letters; *p; ++p, ++n) d.lut[uint8_t(*p)] = d.lut[uint8_t(*p | 0x20)] = int8_t(n);
    d.nchars = n;
    return d;
}

// the rule, word for word: classes, then the table row by row
int32_t plain_dp(const bsq_desc &d, const std::vector<uint8_t> &x, const std::vector<uint8_t> &y) {
    auto cls = [&](uint8_t c) { return d.lut[c] >= 0 ? int32_t(d.lut[c]) : d.nchars; };
    std::vector<int32_t> prev(y.size() + 1), cur(y.size() + 1);
    for (size_t j = 0; j <= y.size(); ++j) prev[j] = int32_t(j);
    for (size_t i = 1; i <= x.size(); ++i) {
        cur[0] = int32_t(i);
        for (size_t j = 1; j <= y.size(); ++j)
            cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + (cls(x[i - 1]) != cls(y[j - 1])));
        prev.swap(cur);
    }
    return prev[y.size()];
}

std::vector<uint8_t> random_row(uint64_t &state, int64_t n, const char *letters, bool junk) {
    const size_t L = std::strlen(letters);
    std::vector<uint8_t> r(static_cast<size_t>(n));
    for (uint8_t &c : r) {
        c = uint8_t(letters[next(state) % L]);
        if (junk && next(state) % 16 == 0) c = uint8_t(next(state) % 256);  // unmapped bytes, lower case, bytes >= 0x80
    }
    return r;
}

std::vector<uint8_t> mutated(uint64_t &state, const std::vector<uint8_t> &x, int64_t n, const char *letters) {
    const size_t L = std::strlen(letters);
    std::vector<uint8_t> r;
    for (uint8_t c : x) {
        const uint64_t u = next(state) % 100;
        if (u < 3) continue;
        r.push_back(u < 6 ? uint8_t(letters[next(state) % L]) : c);
        if (next(state) % 100 < 3) r.push_back(uint8_t(letters[next(state) % L]));
    }
    while (int64_t(r.size()) < n) r.push_back(uint8_t(letters[next(state) % L]));
    r.resize(static_cast<size_t>(n));
    return r;
}

struct Store {
    uint8_t *chars;  // exact size (one byte when there is no character: a valid, distinct address)
    int64_t *offsets;
    int64_t B;
    explicit Store(const std::vector<std::vector<uint8_t>> &rows) : B(int64_t(rows.size())) {
        offsets = new int64_t[size_t(B) + 1];
        offsets[0] = 0;
        for (int64_t i = 0; i < B; ++i) offsets[i + 1] = offsets[i] + int64_t(rows[size_t(i)].size());
        chars = new uint8_t[size_t(offsets[B] ? offsets[B] : 1)];
        for (int64_t i = 0; i < B; ++i)
            if (!rows[size_t(i)].empty()) std::memcpy(chars + offsets[i], rows[size_t(i)].data(), rows[size_t(i)].size());
    }
    ~Store() {
        delete[] chars;
        delete[] offsets;
    }
};

int check_alphabet(const char *letters, bool junk, int64_t *cells, int64_t *inside) {
    const bsq_desc d = make_desc(letters);
    uint64_t state = 0x1234 + std::strlen(letters);
    std::vector<std::vector<uint8_t>> ra, rb;
    const int64_t ms[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 257};
    for (int64_t m : ms)
        for (int64_t n : {m, m + 1, m + 70, 2 * m + 3}) {
            ra.push_back(random_row(state, m, letters, junk));
            rb.push_back(random_row(state, n, letters, junk));
            ra.push_back(random_row(state, m, letters, junk));
            rb.push_back(mutated(state, ra.back(), n, letters));
            ra.push_back(std::vector<uint8_t>(size_t(m), uint8_t('A')));
            rb.push_back(std::vector<uint8_t>(size_t(n), uint8_t('A')));
        }
    rb.push_back(random_row(state, 31, letters, junk));  // Ba != Bb
    const Store A(ra), B(rb);
    // the list: (k, k), both stores swapped, repeated and crossed indices, bad indices
    std::vector<int64_t> row, col;
    for (int64_t k = 0; k < A.B; ++k) row.push_back(k), col.push_back(k);
    for (int64_t k = 0; k < A.B; k += 5) row.push_back(k), col.push_back((k * 7 + 3) % B.B);
    const int64_t bad_rows[] = {-1, A.B, int64_t(1) << 40, 0, 0}, bad_cols[] = {0, 0, 0, B.B, -5};
    for (int k = 0; k < 5; ++k) row.push_back(bad_rows[k]), col.push_back(bad_cols[k]);
    const int64_t n_pairs = int64_t(row.size());
    int64_t *prow = new int64_t[size_t(n_pairs)], *pcol = new int64_t[size_t(n_pairs)];
    std::copy(row.begin(), row.end(), prow);
    std::copy(col.begin(), col.end(), pcol);
    int bad = 0;
    for (int32_t max_len : {4096, 128, 64, 1}) {
        const bsq_edit e = {max_len, 0};
        int32_t *dist = new int32_t[size_t(n_pairs)], *swapped = new int32_t[size_t(n_pairs)];
        bad += bsq_edit_pairs_host(&d, A.chars, A.offsets, A.B, B.chars, B.offsets, B.B, prow, pcol, n_pairs, &e, dist) != BSQ_OK;
        bad += bsq_edit_pairs_host(&d, B.chars, B.offsets, B.B, A.chars, A.offsets, A.B, pcol, prow, n_pairs, &e, swapped) != BSQ_OK;
        for (int64_t k = 0; k < n_pairs; ++k) {
            int32_t want;
            if (row[size_t(k)] < 0 || row[size_t(k)] >= A.B || col[size_t(k)] < 0 || col[size_t(k)] >= B.B) {
                want = BSQ_EDIT_BAD_INDEX;
            } else {
                const std::vector<uint8_t> &x = ra[size_t(row[size_t(k)])], &y = rb[size_t(col[size_t(k)])];
                if (int64_t(std::min(x.size(), y.size())) > max_len) {
                    want = BSQ_EDIT_TOO_LONG;
                } else {
                    want = plain_dp(d, x, y);
                    *cells += int64_t(x.size() * y.size());
                    *inside += want > 0 && want < int32_t(std::max(x.size(), y.size()));
                }
            }
            if (dist[k] != want || swapped[k] != want) {
                if (!bad) std::printf("FAILED: %s max_len %d pair %lld (%lld, %lld): %d / %d, want %d\n", letters, max_len, (long long)k,
                                      (long long)row[size_t(k)], (long long)col[size_t(k)], dist[k], swapped[k], want);
                ++bad;
            }
        }
        delete[] dist;
        delete[] swapped;
    }
    // one store on both sides: a row against itself is 0 whatever it holds
    {
        int32_t *dist = new int32_t[size_t(A.B)];
        bad += bsq_edit_pairs_host(&d, A.chars, A.offsets, A.B, A.chars, A.offsets, A.B, prow, prow, A.B, nullptr, dist) != BSQ_OK;
        for (int64_t k = 0; k < A.B; ++k) bad += dist[k] != 0;
        delete[] dist;
    }
    delete[] prow;
    delete[] pcol;
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t cells = 0, inside = 0;
    bad += check_alphabet("ACGT", true, &cells, &inside);
    bad += check_alphabet("ACGTN", false, &cells, &inside);
    bad += check_alphabet("ACDEFGHIKLMNPQRSTVWY", true, &cells, &inside);
    if (cells < 1000000 || inside < 100) ++bad;  // (a check of nothing)
    // the longest pattern: 4096 x 4100, and one character more on the shorter side
    {
        const bsq_desc d = make_desc("ACGT");
        uint64_t state = 99;
        std::vector<std::vector<uint8_t>> rows;
        rows.push_back(random_row(state, 4096, "ACGT", false));
        rows.push_back(mutated(state, rows[0], 4100, "ACGT"));
        rows.push_back(random_row(state, 4097, "ACGT", false));
        const Store S(rows);
        int64_t *row = new int64_t[3]{0, 1, 2}, *col = new int64_t[3]{1, 2, 1};
        int32_t *dist = new int32_t[3];
        bad += bsq_edit_pairs_host(&d, S.chars, S.offsets, 3, S.chars, S.offsets, 3, row, col, 3, nullptr, dist) != BSQ_OK;
        bad += dist[0] != plain_dp(d, rows[0], rows[1]) || dist[0] <= 0 || dist[0] >= 4100 || dist[1] != BSQ_EDIT_TOO_LONG || dist[2] != BSQ_EDIT_TOO_LONG;
        delete[] row;
        delete[] col;
        delete[] dist;
    }
    // the identity test at its boundary and its ends
    bad += !bsq_editd::identity_passes(32, 128, 100, 49152) || bsq_editd::identity_passes(33, 128, 100, 49152);
    bad += !bsq_editd::identity_passes(0, 0, 0, 65536) || bsq_editd::identity_passes(-1, 0, 0, 0) || bsq_editd::identity_passes(-2, 5, 5, 0);
    bad += !bsq_editd::identity_passes(2147483646, 1, 2147483646, 0) || bsq_editd::identity_passes(1, 2147483646, 2147483646, 65536);
    // the argument rules: a refusal writes nothing
    {
        const bsq_desc d = make_desc("ACGT");
        bsq_desc wide = d, none = d;
        wide.nchars = 31;
        none.nchars = 0;
        uint8_t chars[4] = {'A', 'C', 'G', 'T'};
        int64_t offsets[3] = {0, 2, 4}, row[2] = {0, 1}, col[2] = {1, 0};
        int32_t dist[2] = {7, 7};
        const bsq_edit rules[6] = {{0, 0}, {4097, 0}, {257, 1}, {1025, 2}, {100, 4}, {100, -1}};
        for (const bsq_edit &e : rules) bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &e, dist) != BSQ_ERR_INVALID_ARG;
        for (const bsq_edit &e : rules) bad += bsq_edit_pairs_kernel_name(&e)[0] != 0;
        const bsq_edit ok = {100, 0};
        bad += bsq_edit_pairs_host(nullptr, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&wide, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&none, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, nullptr, offsets, 2, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, nullptr, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, chars, offsets, -1, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, col, 2, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, -1, &ok, dist) != BSQ_ERR_INVALID_ARG;
        bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += dist[0] != 7 || dist[1] != 7;
        bad += bsq_edit_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, nullptr, 0, &ok, nullptr) != BSQ_OK;  // nothing to do
        bad += bsq_edit_pairs_host(&d, nullptr, nullptr, 0, chars, offsets, 2, row, col, 2, &ok, dist) != BSQ_OK;            // a store without rows
        bad += dist[0] != BSQ_EDIT_BAD_INDEX || dist[1] != BSQ_EDIT_BAD_INDEX;
        bad += std::strcmp(bsq_edit_pairs_kernel_name(&ok), "k_edit_pairs<4>") != 0 || std::strcmp(bsq_edit_pairs_kernel_name(nullptr), "k_edit_pairs<64>") != 0;
    }
    if (bad) {
        std::printf("EDIT_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("EDIT_HOST_OK\n");
    return 0;
}
