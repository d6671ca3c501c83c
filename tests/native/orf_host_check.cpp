// Stand-alone check of bsq_orf_host.cpp for a sanitizer build (tests/test_orfs_host.py compiles both with -fsanitize=address,undefined):
// hand-made rows -- every length around the walk's pieces, stops and starts at the piece edges, rows of nothing but stops, rows
// without one -- through bsq_orf_count_host and bsq_orf_emit_host, against a plain loop written from the rule of include/bsq.h.  Every
// input and output array is a heap block of its exact size, so a read past a row's batch or a write at or past max_orfs is an error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bsq.h"
#include "bsq_internal.h"

namespace bsq_internal {
static std::string g_last;
bsq_status set_error(bsq_status st, const char *msg) {
    g_last = msg;
    return st;
}
}  // namespace bsq_internal

namespace {

struct Orf {
    int64_t row, start, length;
    bool operator==(const Orf &o) const { return row == o.row && start == o.start && length == o.length; }
};

// the rule, word for word: terminators, segments, s
std::vector<Orf> reference(const std::vector<std::string> &rows, const bsq_orf &o) {
    std::vector<Orf> out;
    for (size_t r = 0; r < rows.size(); ++r) {
        const std::string &row = rows[r];
        const int64_t m = int64_t(row.size());
        int64_t p = -1;
        for (int64_t e = 0; e <= m; ++e) {
            if (e < m && uint8_t(row[size_t(e)]) != o.stop) continue;
            int64_t s = p + 1;
            if (o.start >= 0) {
                while (s < e && uint8_t(row[size_t(s)]) != uint8_t(o.start)) ++s;
                if (s == e) s = -1;
            }
            if (s >= 0 && e - s >= o.min_len) out.push_back(Orf{int64_t(r), s, e - s});
            p = e;
        }
    }
    return out;
}

std::vector<std::string> hand_rows(int64_t ml) {
    std::vector<std::string> rows;
    const size_t n = size_t(ml);
    for (size_t len : {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 5000}) {
        rows.push_back(std::string(len, 'A'));
        rows.push_back(std::string(len, '*'));
        rows.push_back(std::string(len, 'M'));
        if (!len) continue;
        std::string r(len, 'A');
        r[0] = '*';
        rows.push_back(r);
        r[0] = 'A';
        r[len - 1] = '*';
        rows.push_back(r);
        for (size_t k = 0; k < len; ++k) r[k] = (k * 2654435761u >> 7) % 19 == 0 ? '*' : (k * 40503u >> 3) % 11 == 0 ? 'M' : 'A';
        rows.push_back(r);
    }
    for (size_t at : {64, 256, 192, 512}) {
        for (int which = 1; which <= 3; ++which) {
            std::string r(at + 50, 'A');
            if (which & 1) r[at - 1] = '*';
            if (which & 2) r[at] = '*';
            rows.push_back(r);
            r[at / 2] = 'M';
            rows.push_back(r);
        }
    }
    const std::string A(n, 'A'), A1(n - 1, 'A');
    rows.push_back("*" + A + "*" + A1 + "*" + A);
    rows.push_back(A1 + "*" + A1);
    rows.push_back("A**A***" + A + "**");
    rows.push_back("*" + std::string(2 * 64 + 4, 'A') + "*AAA");
    rows.push_back("*AAM" + A1 + "*AAM" + (n >= 2 ? std::string(n - 2, 'A') : std::string()) + "*");
    rows.push_back("*" + A + "AAAM" + A + "*");
    rows.push_back("AAAAAM" + std::string(700, 'A') + "*" + A);
    {
        std::string r(64 + n + 20, 'A');
        const size_t k = n / 2 < 63 ? n / 2 : 63;
        r[63 - k] = 'M';
        r[63 - k + n] = '*';
        rows.push_back(r);
    }
    return rows;
}

int check(const std::vector<std::string> &rows, const bsq_orf &o) {
    const int64_t n = int64_t(rows.size());
    std::vector<int64_t> offsets(size_t(n) + 1, 0);
    for (int64_t i = 0; i < n; ++i) offsets[size_t(i) + 1] = offsets[size_t(i)] + int64_t(rows[size_t(i)].size());
    const size_t total = size_t(offsets[size_t(n)]);
    uint8_t *chars = new uint8_t[total ? total : 1];  // (exact size: the last row ends where the block does)
    for (int64_t i = 0; i < n; ++i) std::memcpy(chars + offsets[size_t(i)], rows[size_t(i)].data(), rows[size_t(i)].size());
    const std::vector<Orf> exp = reference(rows, o);
    int bad = 0;
    int64_t *orf_offsets = new int64_t[size_t(n) + 1];
    int64_t residues = -1, want = 0;
    if (bsq_orf_count_host(chars, offsets.data(), n, &o, orf_offsets, &residues) != BSQ_OK) ++bad;
    for (const Orf &x : exp) want += x.length;
    if (orf_offsets[n] != int64_t(exp.size()) || residues != want) ++bad;
    for (int64_t i = 0, k = 0; i < n; ++i) {
        if (orf_offsets[i] != k) ++bad;
        while (size_t(k) < exp.size() && exp[size_t(k)].row == i) ++k;
    }
    for (int64_t cap : {int64_t(exp.size()), int64_t(exp.size()) - 1, int64_t(exp.size()) / 2, int64_t(0)}) {
        if (cap < 0) continue;
        int64_t *row = new int64_t[size_t(cap) + 1], *start = new int64_t[size_t(cap) + 1], *length = new int64_t[size_t(cap) + 1];
        // (one spare entry: new int64_t[0] may not be dereferenced, and the entry at max_orfs must stay as it is)
        row[cap] = start[cap] = length[cap] = -7;
        if (bsq_orf_emit_host(chars, offsets.data(), n, &o, orf_offsets, cap, row, start, length) != BSQ_OK) ++bad;
        for (int64_t k = 0; k < cap; ++k)
            if (!(Orf{row[k], start[k], length[k]} == exp[size_t(k)])) ++bad;
        if (row[cap] != -7 || start[cap] != -7 || length[cap] != -7) ++bad;
        delete[] row;
        delete[] start;
        delete[] length;
    }
    delete[] orf_offsets;
    delete[] chars;
    if (bad) std::printf("FAILED: stop %d start %d min_len %lld: %d mismatches\n", int(o.stop), int(o.start), (long long)o.min_len, bad);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    for (int64_t ml : {1, 5, 30}) {
        const std::vector<std::string> rows = hand_rows(ml);
        for (int32_t start : {-1, int32_t('M')}) bad += check(rows, bsq_orf{uint8_t('*'), start, ml});
        bad += check(rows, bsq_orf{uint8_t('A'), int32_t('*'), ml});
        bad += check(rows, bsq_orf{uint8_t(0), -1, ml});
    }
    bad += check({}, bsq_orf{uint8_t('*'), -1, 1});
    // the argument rules
    const int64_t offs[2] = {0, 1};
    const uint8_t ch[1] = {'A'};
    int64_t oo[2], out[1];
    const bsq_orf rules[] = {{uint8_t('*'), -1, 0}, {uint8_t('*'), -2, 1}, {uint8_t('*'), 256, 1}, {uint8_t('*'), int32_t('*'), 1}};
    for (const bsq_orf &r : rules) {
        bad += bsq_orf_count_host(ch, offs, 1, &r, oo, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += bsq_orf_emit_host(ch, offs, 1, &r, oo, 1, out, out, out) != BSQ_ERR_INVALID_ARG;
    }
    const bsq_orf ok{uint8_t('*'), -1, 1};
    bad += bsq_orf_count_host(ch, offs, 1, nullptr, oo, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_orf_count_host(nullptr, offs, 1, &ok, oo, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_orf_count_host(ch, offs, -1, &ok, oo, nullptr) != BSQ_ERR_INVALID_ARG;
    bad += bsq_orf_emit_host(ch, offs, 1, &ok, oo, -1, out, out, out) != BSQ_ERR_INVALID_ARG;
    bad += bsq_orf_emit_host(ch, offs, 1, &ok, oo, 1, out, nullptr, out) != BSQ_ERR_INVALID_ARG;
    if (bad) {
        std::printf("ORF_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("ORF_HOST_OK\n");
    return 0;
}
