// Stand-alone check of bsq_align_stats_host (bsq_align_stats_host.cpp) for a sanitizer build (tests/test_align_stats_native.py compiles
// both with -fsanitize=address,undefined): generated pairs of rows -- unrelated, mutated copies, runs of one letter, two-letter rows full
// of ties -- around the 32-row edges, through both stores, both modes and every code, against the rule of include/bsq.h ("alignment
// statistics of row pairs") written out row by row with the tuples as plain structs in A / B terms.  Every input and output
// array is a heap block of its exact size, so a read past a store or a write past score or stats is an error.  Needs no HIP header.
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

struct Path {
    int64_t sa, sb, matches, diag;
};
struct State {
    int64_t v;
    Path p;
};
struct Answer {
    int32_t score;
    int32_t stats[6];
};

// the rule, word for word, in 64-bit integers, row by row
Answer plain_stats(const bsq_desc &d, const bsq_score &s, const std::vector<uint8_t> &x, const std::vector<uint8_t> &y) {
    auto cls = [&](uint8_t c) { return d.lut[c] >= 0 ? int32_t(d.lut[c]) : d.nchars; };
    const bool local = s.mode == 0;
    const int64_t la = int64_t(x.size()), lb = int64_t(y.size()), o = s.gap_open, e = s.gap_extend, inf = -(int64_t(1) << 40);
    Answer out = {0, {0, 0, 0, 0, 0, 0}};
    if (la == 0 || lb == 0) {
        if (!local) {
            out.score = la + lb == 0 ? 0 : int32_t(-(o + (la + lb) * e));
            out.stats[2] = int32_t(la), out.stats[3] = int32_t(lb), out.stats[5] = int32_t(la + lb);
        }
        return out;
    }
    const size_t W = size_t(lb) + 1;
    std::vector<State> H(W), F(W), Hup(W), Fup(W);  // row i and row i - 1 of H and F; E runs along the row
    for (int64_t j = 0; j <= lb; ++j) {
        H[size_t(j)] = {local || j == 0 ? 0 : -(o + j * e), {0, local ? j : 0, 0, 0}};
        F[size_t(j)] = {inf, {0, 0, 0, 0}};
    }
    State best = {0, {0, 0, 0, 0}};
    int64_t bi = 0, bj = 0;
    for (int64_t i = 1; i <= la; ++i) {
        Hup.swap(H);
        Fup.swap(F);
        H[0] = {local ? 0 : -(o + i * e), {local ? i : 0, 0, 0, 0}};
        State E = {inf, {0, 0, 0, 0}};
        for (size_t j = 1; j < W; ++j) {
            E = H[j - 1].v - o >= E.v ? State{H[j - 1].v - o - e, H[j - 1].p} : State{E.v - e, E.p};
            F[j] = Hup[j].v - o >= Fup[j].v ? State{Hup[j].v - o - e, Hup[j].p} : State{Fup[j].v - e, Fup[j].p};
            const State &hd = Hup[j - 1];
            const int32_t cx = cls(x[size_t(i - 1)]), cy = cls(y[j - 1]);
            const int64_t dv = hd.v + s.matrix[cx][cy], top = std::max(dv, std::max(E.v, F[j].v));
            if (local && top <= 0) H[j] = {0, {i, int64_t(j), 0, 0}};
            else if (dv == top) H[j] = {dv, {hd.p.sa, hd.p.sb, hd.p.matches + (cx == cy), hd.p.diag + 1}};
            else if (E.v == top) H[j] = {top, E.p};
            else H[j] = {top, F[j].p};
            if (local && H[j].v > best.v) best = H[j], bi = i, bj = int64_t(j);  // (row-major order: the smallest end_a, then end_b)
        }
    }
    if (local && best.v == 0) return out;
    if (!local) best = H[size_t(lb)], bi = la, bj = lb;
    out.score = int32_t(best.v);
    const int64_t st[6] = {best.p.sa, best.p.sb, bi, bj, best.p.matches, (bi - best.p.sa) + (bj - best.p.sb) - best.p.diag};
    for (int q = 0; q < 6; ++q) out.stats[q] = int32_t(st[q]);
    return out;
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

// an asymmetric matrix with a positive diagonal (small = true: +1 / -1 .. 0, so that most cells tie); what lies at an index > nchars is
// poison that must not be read into a score
void fill_matrix(bsq_score *s, int32_t nchars, uint64_t &state, bool small) {
    std::memset(s->matrix, 99, sizeof s->matrix);
    for (int32_t r = 0; r <= nchars; ++r)
        for (int32_t c = 0; c <= nchars; ++c)
            s->matrix[r][c] = small ? int8_t(r == c ? 1 : -int(next(state) % 2)) : int8_t(r == c ? 2 + int(next(state) % 5) : -int(next(state) % 6));
}

int check_alphabet(const char *letters, bool junk, bool small, int64_t *cells, int64_t *inside) {
    const bsq_desc d = make_desc(letters);
    uint64_t state = 0x4321 + std::strlen(letters);
    std::vector<std::vector<uint8_t>> ra, rb;
    const int64_t ms[] = {0, 1, 2, 31, 32, 33, 63, 65, 100};
    for (int64_t m : ms)
        for (int64_t n : {m, m + 1, m + 40, 2 * m + 3}) {
            ra.push_back(random_row(state, m, letters, junk));
            rb.push_back(random_row(state, n, letters, junk));
            ra.push_back(random_row(state, m, letters, junk));
            rb.push_back(mutated(state, ra.back(), n, letters));
            ra.push_back(std::vector<uint8_t>(size_t(m), uint8_t(letters[0])));
            rb.push_back(std::vector<uint8_t>(size_t(n), uint8_t(letters[0])));
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
    const int32_t gaps[4][2] = {{5, 2}, {0, 1}, {1, 1}, {3, 0}};
    int turn = 0;
    for (int32_t max_len : {2048, 64, 32})
        for (int32_t mode : {0, 1}) {
            bsq_score s = {max_len, 0, mode, gaps[turn % 4][0], gaps[turn % 4][1], {}}, st;
            ++turn;
            fill_matrix(&s, d.nchars, state, small);
            st = s;  // the transposed matrix for the swapped stores
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) st.matrix[r][c] = s.matrix[c][r];
            int32_t *score = new int32_t[size_t(n_pairs)], *stats = new int32_t[size_t(6 * n_pairs)], *swapped = new int32_t[size_t(n_pairs)],
                    *swapped_stats = new int32_t[size_t(6 * n_pairs)];
            bad += bsq_align_stats_host(&d, A.chars, A.offsets, A.B, B.chars, B.offsets, B.B, prow, pcol, n_pairs, &s, score, stats) != BSQ_OK;
            bad += bsq_align_stats_host(&d, B.chars, B.offsets, B.B, A.chars, A.offsets, A.B, pcol, prow, n_pairs, &st, swapped, swapped_stats) != BSQ_OK;
            for (int64_t k = 0; k < n_pairs; ++k) {
                Answer want = {0, {-1, -1, -1, -1, -1, -1}}, back = want;  // back: the stores swapped (its ties are broken in ITS A / B terms)
                if (row[size_t(k)] < 0 || row[size_t(k)] >= A.B || col[size_t(k)] < 0 || col[size_t(k)] >= B.B) {
                    want.score = back.score = BSQ_SCORE_BAD_INDEX;
                } else {
                    const std::vector<uint8_t> &x = ra[size_t(row[size_t(k)])], &y = rb[size_t(col[size_t(k)])];
                    if (int64_t(std::min(x.size(), y.size())) > max_len) {
                        want.score = back.score = BSQ_SCORE_TOO_LONG;
                    } else {
                        want = plain_stats(d, s, x, y);
                        back = plain_stats(d, st, y, x);
                        *cells += int64_t(x.size() * y.size());
                        *inside += want.score > 0 && want.stats[0] > 0 && want.stats[5] > want.stats[4];
                    }
                }
                const bool ok = score[k] == want.score && std::memcmp(stats + 6 * k, want.stats, sizeof want.stats) == 0 && swapped[k] == back.score &&
                                back.score == want.score && std::memcmp(swapped_stats + 6 * k, back.stats, sizeof back.stats) == 0;
                if (!ok) {
                    if (!bad) std::printf("FAILED: %s max_len %d mode %d pair %lld (%lld, %lld): %d (%d, %d, %d, %d, %d, %d), want %d (%d, %d, %d, %d, %d, %d)\n",
                                          letters, max_len, mode, (long long)k, (long long)row[size_t(k)], (long long)col[size_t(k)], score[k], stats[6 * k],
                                          stats[6 * k + 1], stats[6 * k + 2], stats[6 * k + 3], stats[6 * k + 4], stats[6 * k + 5], want.score, want.stats[0],
                                          want.stats[1], want.stats[2], want.stats[3], want.stats[4], want.stats[5]);
                    ++bad;
                }
            }
            delete[] score;
            delete[] stats;
            delete[] swapped;
            delete[] swapped_stats;
        }
    delete[] prow;
    delete[] pcol;
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t cells = 0, inside = 0;
    bad += check_alphabet("ACGT", true, false, &cells, &inside);
    bad += check_alphabet("AC", false, true, &cells, &inside);
    bad += check_alphabet("ACDEFGHIKLMNPQRSTVWY", true, false, &cells, &inside);
    if (cells < 1000000 || inside < 100) ++bad;  // (a check of nothing)
    // the longest pattern: 2048 x 2060, and one character more on the shorter side; BLOSUM-like costs {11, 1}
    {
        const bsq_desc d = make_desc("ACGT");
        uint64_t state = 99;
        std::vector<std::vector<uint8_t>> rows;
        rows.push_back(random_row(state, 2048, "ACGT", false));
        rows.push_back(mutated(state, rows[0], 2060, "ACGT"));
        rows.push_back(random_row(state, 2049, "ACGT", false));
        const Store S(rows);
        bsq_score s = {2048, 0, 0, 11, 1, {}};
        fill_matrix(&s, d.nchars, state, false);
        int64_t *row = new int64_t[3]{0, 1, 2}, *col = new int64_t[3]{1, 2, 1};
        int32_t *score = new int32_t[3], *stats = new int32_t[18];
        bad += bsq_align_stats_host(&d, S.chars, S.offsets, 3, S.chars, S.offsets, 3, row, col, 3, &s, score, stats) != BSQ_OK;
        const Answer want = plain_stats(d, s, rows[0], rows[1]);
        bad += score[0] != want.score || std::memcmp(stats, want.stats, sizeof want.stats) != 0 || want.score <= 0 || want.stats[4] < 1500;
        bad += score[1] != BSQ_SCORE_TOO_LONG || score[2] != BSQ_SCORE_TOO_LONG || stats[6] != -1 || stats[17] != -1;
        delete[] row;
        delete[] col;
        delete[] score;
        delete[] stats;
    }
    // the argument rules: a refusal writes nothing
    {
        const bsq_desc d = make_desc("ACGT");
        bsq_desc wide = d, none = d;
        wide.nchars = 31;
        none.nchars = 0;
        uint8_t chars[4] = {'A', 'C', 'G', 'T'};
        int64_t offsets[3] = {0, 2, 4}, row[2] = {0, 1}, col[2] = {1, 0};
        int32_t score[2] = {7, 7}, stats[12] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7};
        const bsq_score rules[12] = {{0, 0, 0, 1, 1, {}},   {2049, 0, 0, 1, 1, {}},  {4096, 0, 0, 1, 1, {}}, {129, 1, 0, 1, 1, {}}, {513, 2, 0, 1, 1, {}},
                                     {100, 4, 0, 1, 1, {}}, {100, -1, 0, 1, 1, {}},  {100, 0, 2, 1, 1, {}},  {100, 0, -1, 1, 1, {}}, {100, 0, 0, 128, 1, {}},
                                     {100, 0, 0, -1, 1, {}}, {100, 0, 1, 1, 128, {}}};
        for (const bsq_score &s : rules) bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &s, score, stats) != BSQ_ERR_INVALID_ARG;
        for (const bsq_score &s : rules) bad += bsq_align_stats_kernel_name(&s)[0] != 0;
        const bsq_score ok = {100, 0, 0, 1, 1, {}};
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, nullptr, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(nullptr, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&wide, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&none, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, nullptr, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, nullptr, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, -1, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, col, 2, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, -1, &ok, score, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, nullptr, stats) != BSQ_ERR_INVALID_ARG;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, row, col, 2, &ok, score, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += score[0] != 7 || score[1] != 7 || stats[0] != 7 || stats[11] != 7;
        bad += bsq_align_stats_host(&d, chars, offsets, 2, chars, offsets, 2, nullptr, nullptr, 0, &ok, nullptr, nullptr) != BSQ_OK;  // nothing to do
        bad += bsq_align_stats_host(&d, nullptr, nullptr, 0, chars, offsets, 2, row, col, 2, &ok, score, stats) != BSQ_OK;            // a store without rows
        bad += score[0] != BSQ_SCORE_BAD_INDEX || score[1] != BSQ_SCORE_BAD_INDEX || stats[0] != -1 || stats[11] != -1;
        bad += std::strcmp(bsq_align_stats_kernel_name(&ok), "k_align_stats<4, local>") != 0 || bsq_align_stats_kernel_name(nullptr)[0] != 0;
        const bsq_score wide_ok = {2048, 0, 1, 1, 1, {}};
        bad += std::strcmp(bsq_align_stats_kernel_name(&wide_ok), "k_align_stats<64, global>") != 0;
    }
    if (bad) {
        std::printf("ALIGN_STATS_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("ALIGN_STATS_HOST_OK\n");
    return 0;
}
