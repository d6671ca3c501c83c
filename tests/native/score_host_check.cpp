// Stand-alone check of bsq_score_pairs_host (bsq_score_host.cpp) for a sanitizer build (tests/test_score_native.py compiles both with
// -fsanitize=address,undefined): generated pairs of rows -- unrelated, mutated copies, runs of one letter -- around the 64-row edges,
// through both stores, both modes, with and without ends and every code, against Gotoh's recurrence written row by row from the
// rule of include/bsq.h ("scored alignment of row pairs").  Every input and output array is a heap block of its exact size, so a read
// past a store or a write past score or ends is an error.  Needs no HIP header.
#include <algorithm>
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

struct Answer {
    int32_t score, end_a, end_b;
};

// the rule, word for word, in 64-bit integers
Answer plain_gotoh(const bsq_desc &d, const bsq_score &s, const std::vector<uint8_t> &x, const std::vector<uint8_t> &y) {
    auto cls = [&](uint8_t c) { return d.lut[c] >= 0 ? int32_t(d.lut[c]) : d.nchars; };
    const bool local = s.mode == 0;
    const int64_t la = int64_t(x.size()), lb = int64_t(y.size()), o = s.gap_open, e = s.gap_extend, inf = -(int64_t(1) << 40);
    const size_t W = size_t(lb) + 1;
    std::vector<int64_t> H(W, 0), F(W, inf), Hup(W), Fup(W);  // row i and row i - 1 of H and F; E runs along the row as a scalar
    if (!local)
        for (int64_t j = 1; j <= lb; ++j) H[size_t(j)] = -(o + j * e);
    Answer best = {0, 0, 0};
    for (int64_t i = 1; i <= la; ++i) {
        Hup.swap(H);
        Fup.swap(F);
        H[0] = local ? 0 : -(o + i * e);
        int64_t E = inf;
        for (size_t j = 1; j < W; ++j) {
            E = std::max(E, H[j - 1] - o) - e;
            F[j] = std::max(Fup[j], Hup[j] - o) - e;
            int64_t h = std::max(Hup[j - 1] + s.matrix[cls(x[size_t(i - 1)])][cls(y[j - 1])], std::max(E, F[j]));
            if (local) h = std::max<int64_t>(h, 0);
            H[j] = h;
            if (local && h > best.score) best = {int32_t(h), int32_t(i), int32_t(j)};  // (row-major order: the smallest end_a, then end_b)
        }
    }
    if (local) return best;
    return {int32_t(H[size_t(lb)]), int32_t(la), int32_t(lb)};
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

// an asymmetric matrix with a positive diagonal; what lies at an index > nchars is poison that must not be read into a score
void fill_matrix(bsq_score *s, int32_t nchars, uint64_t &state) {
    std::memset(s->matrix, 99, sizeof s->matrix);
    for (int32_t r = 0; r <= nchars; ++r)
        for (int32_t c = 0; c <= nchars; ++c) s->matrix[r][c] = int8_t(r == c ? 2 + int(next(state) % 5) : -int(next(state) % 6));
}

int check_alphabet(const char *letters, bool junk, int64_t *cells, int64_t *inside) {
    const bsq_desc d = make_desc(letters);
    uint64_t state = 0x4321 + std::strlen(letters);
    std::vector<std::vector<uint8_t>> ra, rb;
    const int64_t ms[] = {0, 1, 2, 63, 64, 65, 127, 129, 200};
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
    const int32_t gaps[3][2] = {{5, 2}, {0, 1}, {3, 0}};
    int turn = 0;
    for (int32_t max_len : {4096, 128, 64})
        for (int32_t mode : {0, 1}) {
            bsq_score s = {max_len, 0, mode, gaps[turn % 3][0], gaps[turn % 3][1], {}}, st;
            ++turn;
            fill_matrix(&s, d.nchars, state);
            st = s;  // the transposed matrix for the swapped stores
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) st.matrix[r][c] = s.matrix[c][r];
            int32_t *score = new int32_t[size_t(n_pairs)], *ends = new int32_t[size_t(2 * n_pairs)], *swapped = new int32_t[size_t(n_pairs)],
                    *swapped_ends = new int32_t[size_t(2 * n_pairs)], *alone = new int32_t[size_t(n_pairs)];
            bad += bsq_score_pairs_host(&d, A.chars, A.offsets, A.B, B.chars, B.offsets, B.B, prow, pcol, n_pairs, &s, score, ends) != BSQ_OK;
            bad += bsq_score_pairs_host(&d, B.chars, B.offsets, B.B, A.chars, A.offsets, A.B, pcol, prow, n_pairs, &st, swapped, swapped_ends) != BSQ_OK;
            bad += bsq_score_pairs_host(&d, A.chars, A.offsets, A.B, B.chars, B.offsets, B.B, prow, pcol, n_pairs, &s, alone, nullptr) != BSQ_OK;
            for (int64_t k = 0; k < n_pairs; ++k) {
                Answer want = {0, -1, -1}, back = {0, -1, -1};  // back: the stores swapped (its ends obey the tie rule in ITS A / B terms)
                if (row[size_t(k)] < 0 || row[size_t(k)] >= A.B || col[size_t(k)] < 0 || col[size_t(k)] >= B.B) {
                    want.score = back.score = BSQ_SCORE_BAD_INDEX;
                } else {
                    const std::vector<uint8_t> &x = ra[size_t(row[size_t(k)])], &y = rb[size_t(col[size_t(k)])];
                    if (int64_t(std::min(x.size(), y.size())) > max_len) {
                        want.score = back.score = BSQ_SCORE_TOO_LONG;
                    } else {
                        want = plain_gotoh(d, s, x, y);
                        back = plain_gotoh(d, st, y, x);
                        *cells += int64_t(x.size() * y.size());
                        *inside += want.score > 0 && want.end_a > 0;
                    }
                }
                const bool ok = score[k] == want.score && ends[2 * k] == want.end_a && ends[2 * k + 1] == want.end_b && swapped[k] == want.score &&
                                back.score == want.score && swapped_ends[2 * k] == back.end_a && swapped_ends[2 * k + 1] == back.end_b && alone[k] == want.score;
                if (!ok) {
                    if (!bad) std::printf("FAILED: %s max_len %d mode %d pair %lld (%lld, %lld): %d (%d, %d) / %d (%d, %d), want %d (%d, %d)\n", letters, max_len,
                                          mode, (long long)k, (long long)row[size_t(k)], (long long)col[size_t(k)], score[k], ends[2 * k], ends[2 * k + 1],
                                          swapped[k], swapped_ends[2 * k], swapped_ends[2 * k + 1], want.score, want.end_a, want.end_b);
                    ++bad;
                }
            }
            delete[] score;
            delete[] ends;
            delete[] swapped;
            delete[] swapped_ends;
            delete[] alone;
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
    bad += check_alphabet("ACDEFGHIKLMNPQRSTVWY", true, &cells, &inside);
    if (cells < 1000000 || inside < 100) ++bad;  // (a check of nothing)
    // the longest pattern: 4096 x 4100, and one character more on the shorter side; BLOSUM-like costs {11, 1}
    {
        const bsq_desc d = make_desc("ACGT");
        uint64_t state = 99;
        std::vector<std::vector<uint8_t>> rows;
        rows.push_back(random_row(state, 4096, "ACGT", false));
        rows.push_back(mutated(state, rows[0], 4100, "ACGT"));
        rows.push_back(random_row(state, 4097, "ACGT", false));
        const Store S(rows);
        bsq_score s = {4096, 0, 0, 11, 1, {}};
        fill_matrix(&s, d.nchars, state);
        int64_t *row = new int64_t[3]{0, 1, 2}, *col = new int64_t[3]{1, 2, 1};
        int32_t *score = new int32_t[3], *ends = new int32_t[6];
        bad += bsq_score_pairs_host(&d, S.chars, S.offsets, 3, S.chars, S.offsets, 3, row, col, 3, &s, score, ends) != BSQ_OK;
        const Answer want = plain_gotoh(d, s, rows[0], rows[1]);
        bad += score[0] != want.score || ends[0] != want.end_a || ends[1] != want.end_b || want.score <= 0;
        bad += score[1] != BSQ_SCORE_TOO_LONG || score[2] != BSQ_SCORE_TOO_LONG || ends[2] != -1 || ends[5] != -1;
        delete[] row;
        delete[] col;
        delete[] score;
        delete[] ends;
    }
    // the argument rules: a refusal writes nothing
    {
        const bsq_desc d = make_desc("ACGT");
        bsq_desc wide = d, none = d;
        wide.nchars = 31;
        none.nchars = 0;
        uint8_t chars[4] = {'A', 'C', 'G', 'T'};
        int64_t offsets[3] = {0, 2, 4}, row[2] = {0, 1}, col[2] = {1, 0};
        int32_t score[2] = {7, 7}, ends[4] = {7, 7, 7, 7};
        const bsq_score rules[11] = {{0, 0, 0, 1, 1, {}},   {4097, 0, 0, 1, 1, {}}, {257, 1, 0, 1, 1, {}}, {1025, 2, 0, 1, 1, {}}, {100, 4, 0, 1, 1, {}},
                                     {100, -1, 0, 1, 1, {}}, {100, 0, 2, 1, 1, {}},  {100, 0, -1, 1, 1, {}}, {100, 0, 0, 128, 1, {}}, {100, 0, 0, -1, 1, {}},
                                     {100, 0, 1, 1, 128, {}}};
        for (const bsq_score &s : rules) bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &s, score, ends) != BSQ_ERR_INVALID_ARG;
        for (const bsq_score &s : rules) bad += bsq_score_pairs_kernel_name(&s, 1)[0] != 0;
        const bsq_score ok = {100, 0, 0, 1, 1, {}};
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, nullptr, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(nullptr, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&wide, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&none, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, nullptr, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, nullptr, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, chars, offsets, -1, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, col, 2, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, -1, &ok, score, ends) != BSQ_ERR_INVALID_ARG;
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, nullptr, ends) != BSQ_ERR_INVALID_ARG;
        bad += score[0] != 7 || score[1] != 7 || ends[0] != 7 || ends[3] != 7;
        bad += bsq_score_pairs_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, nullptr, 0, &ok, nullptr, nullptr) != BSQ_OK;  // nothing to do
        bad += bsq_score_pairs_host(&d, nullptr, nullptr, 0, chars, offsets, 2, row, col, 2, &ok, score, ends) != BSQ_OK;            // a store without rows
        bad += score[0] != BSQ_SCORE_BAD_INDEX || score[1] != BSQ_SCORE_BAD_INDEX || ends[0] != -1 || ends[3] != -1;
        bad += std::strcmp(bsq_score_pairs_kernel_name(&ok, 0), "k_score_pairs<4, local>") != 0;
        bad += std::strcmp(bsq_score_pairs_kernel_name(&ok, 1), "k_score_pairs<4, local+ends>") != 0 || bsq_score_pairs_kernel_name(nullptr, 0)[0] != 0;
    }
    if (bad) {
        std::printf("SCORE_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("SCORE_HOST_OK\n");
    return 0;
}
