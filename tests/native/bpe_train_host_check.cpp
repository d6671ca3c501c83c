// Stand-alone check of the BPE training twin (bsq_bpe_train_host.cpp: bsq_bpe_train_host and the sizes) under ASan / UBSan: its own main,
// exact-size heap arrays -- a read past the characters or the offsets, or a write past merges or counts, is an error -- and its own
// programme of the rule for the answers: rows as vectors, a std::map of counts per step, every pair of a row walked left to right.
// Built and run by tests/test_bpe_train_host.py; no Python, no device.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
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

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {  // xorshift64*: the same rows on every run
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return static_cast<uint32_t>(((g_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

bsq_desc make_desc(const char *letters) {
    bsq_desc d;
    std::memset(&d, 0, sizeof d);
    for (int c = 0; c < 256; ++c) d.lut[c] = -1;
    int n = 0;
    for (const char *p = letters; *p; ++p, ++n) d.lut[static_cast<uint8_t>(*p)] = static_cast<int8_t>(n);
    d.nchars = n;
    return d;
}

using Rows = std::vector<std::vector<int32_t>>;

// the rule: per step a map of the counts (without overlap: of a run of equal symbols every second pair), the largest count, the smallest
// pair among equals, stop below 2, replace left to right
void plain_train(Rows rows, int32_t C, int32_t n_merges, std::vector<int32_t> *merges, std::vector<int64_t> *counts) {
    for (int32_t m = 0; m < n_merges; ++m) {
        std::map<std::pair<int32_t, int32_t>, int64_t> cnt;
        for (const auto &row : rows) {
            bool prev = false;
            for (size_t q = 0; q + 1 < row.size(); ++q) {
                const int32_t a = row[q], b = row[q + 1];
                if (a < 0 || b < 0) {
                    prev = false;
                    continue;
                }
                const bool skip = a == b && prev && q > 0 && row[q - 1] == a;
                prev = a == b && !skip;
                if (!skip) ++cnt[{a, b}];
            }
        }
        std::pair<int32_t, int32_t> best{0, 0};
        int64_t top = 0;
        for (const auto &kv : cnt)  // (ascending pairs: the first maximum is the smallest pair)
            if (kv.second > top) best = kv.first, top = kv.second;
        if (top < 2) return;
        merges->push_back(best.first);
        merges->push_back(best.second);
        counts->push_back(top);
        for (auto &row : rows) {
            std::vector<int32_t> out;
            for (size_t q = 0; q < row.size();) {
                if (q + 1 < row.size() && row[q] == best.first && row[q + 1] == best.second) out.push_back(C + m), q += 2;
                else out.push_back(row[q]), q += 1;
            }
            row.swap(out);
        }
    }
}

int g_failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, bsq_internal::g_last.c_str());
        ++g_failures;
    }
}

void run_case(const bsq_desc &d, const std::vector<std::string> &text, int32_t n_merges, int32_t max_chars, const char *what) {
    std::vector<int64_t> offs_v(1, 0);
    std::string all;
    Rows rows;
    int64_t too_long = 0;
    for (const auto &s : text) {
        all += s;
        offs_v.push_back(static_cast<int64_t>(all.size()));
        if (static_cast<int32_t>(s.size()) > max_chars) {
            ++too_long;
            continue;
        }
        std::vector<int32_t> row;
        for (const char c : s) row.push_back(d.lut[static_cast<uint8_t>(c)]);
        rows.push_back(row);
    }
    // exact-size heap copies
    uint8_t *chars = new uint8_t[all.size() ? all.size() : 1];
    std::memcpy(chars, all.data(), all.size());
    int64_t *offs = new int64_t[offs_v.size()];
    std::memcpy(offs, offs_v.data(), offs_v.size() * sizeof(int64_t));
    int32_t *merges = new int32_t[n_merges ? 2 * n_merges : 1];
    int64_t *counts = new int64_t[n_merges ? n_merges : 1];
    int64_t made = -1, skipped = -1;
    const bsq_bpe_train cfg{max_chars, 0, n_merges, 0, 0};
    const bsq_status st = bsq_bpe_train_host(&d, chars, offs, static_cast<int64_t>(text.size()), static_cast<int64_t>(all.size()), &cfg, merges, counts,
                                             &made, &skipped);
    expect(st == BSQ_OK, what);
    std::vector<int32_t> exp_m;
    std::vector<int64_t> exp_c;
    plain_train(rows, d.nchars, n_merges, &exp_m, &exp_c);
    expect(made == static_cast<int64_t>(exp_c.size()) && skipped == too_long, what);
    if (made == static_cast<int64_t>(exp_c.size()) && made > 0) {
        expect(std::memcmp(merges, exp_m.data(), exp_m.size() * sizeof(int32_t)) == 0, what);
        expect(std::memcmp(counts, exp_c.data(), exp_c.size() * sizeof(int64_t)) == 0, what);
    }
    delete[] chars;
    delete[] offs;
    delete[] merges;
    delete[] counts;
}

std::string random_row(const char *letters, uint32_t n, uint32_t unmapped_percent) {
    const uint32_t A = static_cast<uint32_t>(std::strlen(letters));
    std::string s;
    for (uint32_t i = 0; i < n; ++i) s += rnd(100) < unmapped_percent ? '#' : letters[rnd(A)];
    return s;
}

std::string repeats_row(const char *letters, uint32_t n) {
    const uint32_t A = static_cast<uint32_t>(std::strlen(letters));
    std::string s;
    while (s.size() < n) {
        std::string unit;
        for (uint32_t k = 1 + rnd(3); k > 0; --k) unit += letters[rnd(A)];
        for (uint32_t k = 1 + rnd(30); k > 0; --k) s += unit;
    }
    return s.substr(0, n);
}

}  // namespace

int main() {
    const bsq_desc dna = make_desc("ACGT"), amino = make_desc("ACDEFGHIKLMNPQRSTVWY");
    run_case(dna, {"AAAAAAA"}, 10, 8192, "AAAAAAA");
    run_case(dna, {"ACGACGACG", "CGCG"}, 10, 8192, "ACGACGACG CGCG");
    run_case(dna, {"ACACAC", "ACACAC"}, 10, 8192, "ACACAC x 2");
    run_case(dna, {"AAAAANAAAA"}, 10, 8192, "a barrier");
    run_case(dna, {std::string(8192, 'A')}, 40, 8192, "8192 A");
    run_case(dna, {}, 10, 8192, "no rows");
    run_case(dna, {"", "", "A", ""}, 10, 8192, "empty rows");
    run_case(dna, {"ACACAC"}, 0, 8192, "no merges");
    for (int round = 0; round < 6; ++round) {
        const bsq_desc &d = round % 2 ? amino : dna;
        const char *letters = round % 2 ? "ACDEFGHIKLMNPQRSTVWY" : "ACGT";
        std::vector<std::string> text;
        for (int k = 0; k < 40; ++k) text.push_back(k % 3 == 0 ? repeats_row(letters, rnd(200)) : random_row(letters, rnd(200), k % 3 == 1 ? 3 : 0));
        run_case(d, text, 120, round < 4 ? 8192 : 100, "random rows");
    }
    if (g_failures) return 1;
    std::printf("BPE_TRAIN_HOST_OK\n");
    return 0;
}
