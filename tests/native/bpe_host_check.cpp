// Stand-alone check of the BPE host twin (bsq_bpe_host.cpp: bsq_bpe_table_build, bsq_bpe_tokenize_host and the sizes) under ASan / UBSan:
// its own main, exact-size heap arrays -- a read past the characters, the offsets or the table, or a write past tokens or lengths, is an
// error -- and its own one-merge-at-a-time programme for the answers.  Built and run by tests/test_bpe_native.py; no Python, no device.
#include <algorithm>
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

bsq_desc make_desc(const char *letters, int eos, int bos, int padchar) {
    bsq_desc d;
    std::memset(&d, 0, sizeof d);
    for (int c = 0; c < 256; ++c) d.lut[c] = -1;
    int n = 0;
    for (const char *p = letters; *p; ++p, ++n) {
        d.lut[static_cast<uint8_t>(*p)] = static_cast<int8_t>(n);
        d.lut[static_cast<uint8_t>(*p + 32)] = static_cast<int8_t>(n);  // lower case folds
    }
    d.nchars = n;
    d.eos = eos;
    d.bos = bos;
    d.padchar = padchar;
    return d;
}

// the rule, one merge at a time: the occurrence of lowest rank, leftmost among equals
std::vector<int32_t> plain_ids(const bsq_desc &d, const std::vector<int32_t> &merges, const uint8_t *seq, int64_t L) {
    const int32_t M = static_cast<int32_t>(merges.size() / 2), V = d.nchars + M;
    std::map<std::pair<int32_t, int32_t>, int32_t> rank;
    for (int32_t m = 0; m < M; ++m) rank[{merges[2 * m], merges[2 * m + 1]}] = m;
    std::vector<int32_t> sym;
    for (int64_t i = 0; i < L; ++i) sym.push_back(d.lut[seq[i]] < 0 ? V : d.lut[seq[i]]);
    for (;;) {
        int32_t best = -1;
        size_t at = 0;
        for (size_t i = 0; i + 1 < sym.size(); ++i) {
            const auto it = rank.find({sym[i], sym[i + 1]});
            if (it != rank.end() && (best < 0 || it->second < best)) best = it->second, at = i;
        }
        if (best < 0) return sym;
        sym[at] = d.nchars + best;
        sym.erase(sym.begin() + static_cast<std::ptrdiff_t>(at) + 1);
    }
}

std::vector<int32_t> random_table(int32_t C, int32_t M) {
    std::vector<int32_t> out;
    std::map<std::pair<int32_t, int32_t>, int> seen;
    while (static_cast<int32_t>(out.size() / 2) < M) {
        const int32_t hi = C + static_cast<int32_t>(out.size() / 2), lo = std::min(hi, C + 6);
        const int32_t l = static_cast<int32_t>(rnd(static_cast<uint32_t>(rnd(4) ? lo : hi))), r = static_cast<int32_t>(rnd(static_cast<uint32_t>(rnd(4) ? lo : hi)));
        if (seen.count({l, r})) continue;
        seen[{l, r}] = 1;
        out.push_back(l);
        out.push_back(r);
    }
    return out;
}

template <typename T>
int check_batch(const bsq_desc &d, const std::vector<int32_t> &merges, const std::vector<std::string> &rows, int64_t P, int32_t batch_first,
                bsq_dtype t, int32_t max_chars, int32_t form) {
    const int64_t M = static_cast<int64_t>(merges.size() / 2), B = static_cast<int64_t>(rows.size());
    const int64_t nbytes = bsq_bpe_table_bytes(d.nchars, M);
    if (nbytes <= 0) return std::printf("table_bytes %lld\n", static_cast<long long>(nbytes)), 1;
    std::vector<uint8_t> table(static_cast<size_t>(nbytes));  // (exact size: a probe past the capacity is a heap overflow)
    if (bsq_bpe_table_build(&d, merges.data(), M, table.data()) != BSQ_OK) return std::printf("build: %s\n", bsq_internal::g_last.c_str()), 1;
    std::vector<int64_t> offs(static_cast<size_t>(B) + 1, 0);
    for (int64_t b = 0; b < B; ++b) offs[static_cast<size_t>(b) + 1] = offs[static_cast<size_t>(b)] + static_cast<int64_t>(rows[static_cast<size_t>(b)].size());
    std::vector<uint8_t> chars(static_cast<size_t>(std::max<int64_t>(offs.back(), 1)));
    for (int64_t b = 0; b < B; ++b) std::memcpy(chars.data() + offs[static_cast<size_t>(b)], rows[static_cast<size_t>(b)].data(), rows[static_cast<size_t>(b)].size());
    std::vector<T> tokens(static_cast<size_t>(B * P));
    std::vector<int32_t> lengths(static_cast<size_t>(B));
    const bsq_bpe bpe = {max_chars, form, 0};
    if (bsq_bpe_tokenize_host(&d, chars.data(), offs.data(), B, P, batch_first, table.data(), M, &bpe, t, tokens.data(), lengths.data()) != BSQ_OK)
        return std::printf("tokenize: %s\n", bsq_internal::g_last.c_str()), 1;
    const int32_t V = d.nchars + static_cast<int32_t>(M), bos = d.bos ? 1 : 0, eos = d.eos ? 1 : 0;
    const int32_t pad_store = d.padchar ? V + 1 + bos + eos : 0;
    int bad = 0;
    for (int64_t b = 0; b < B; ++b) {
        const std::string &row = rows[static_cast<size_t>(b)];
        const bool too_long = static_cast<int64_t>(row.size()) > max_chars;
        std::vector<int32_t> ids;
        if (!too_long) ids = plain_ids(d, merges, reinterpret_cast<const uint8_t *>(row.data()), static_cast<int64_t>(row.size()));
        if (lengths[static_cast<size_t>(b)] != (too_long ? -1 : static_cast<int32_t>(ids.size()))) ++bad;
        const int64_t nn = std::min<int64_t>(static_cast<int64_t>(ids.size()), std::max<int64_t>(P - bos - eos, 0));
        for (int64_t pos = 0; pos < P; ++pos) {
            const int64_t j = pos - bos;
            const int32_t want = j < 0 ? V + 1 : (j < nn ? ids[static_cast<size_t>(j)] : ((eos && j == nn) ? V + 1 + bos : pad_store));
            if (tokens[static_cast<size_t>(batch_first ? b * P + pos : pos * B + b)] != static_cast<T>(want)) ++bad;
        }
    }
    if (bad) std::printf("%d wrong values (M %lld, P %lld, dtype %d)\n", bad, static_cast<long long>(M), static_cast<long long>(P), static_cast<int>(t));
    return bad;
}

std::vector<std::string> fuzz_rows(const char *letters, int count, int max_len) {
    const int A = static_cast<int>(std::strlen(letters));
    std::vector<std::string> rows;
    for (int k = 0; k < count; ++k) {
        std::string s;
        const int n = static_cast<int>(rnd(static_cast<uint32_t>(max_len) + 1));
        while (static_cast<int>(s.size()) < n) {
            if (k % 3 == 0) {  // runs and short repeats
                std::string unit;
                for (uint32_t u = 1 + rnd(3); u > 0; --u) unit += letters[rnd(static_cast<uint32_t>(A))];
                for (uint32_t rep = 1 + rnd(40); rep > 0; --rep) s += unit;
            } else {
                s += (k % 3 == 1 && rnd(30) == 0) ? 'N' : letters[rnd(static_cast<uint32_t>(A))];
            }
        }
        s.resize(static_cast<size_t>(n));
        rows.push_back(s);
    }
    return rows;
}

}  // namespace

int main() {
    int bad = 0;
    // the header's known answers
    const bsq_desc dna = make_desc("ACGT", 0, 0, 0);
    const std::vector<int32_t> known = {0, 0, 1, 2, 4, 0, 5, 3, 4, 4, 3, 3};
    const std::vector<std::string> rows = {"AAAAAAA", "AAAAA", "ACGTACGT", "AAACGTNAAAA", "TTTTT", "CGCGT", "N", "", "aaacgtnaaaa"};
    const std::vector<std::vector<int32_t>> want = {{8, 6}, {4, 6}, {0, 7, 0, 7}, {6, 7, 10, 8}, {9, 9, 3}, {5, 7}, {10}, {}, {6, 7, 10, 8}};
    for (size_t k = 0; k < rows.size(); ++k)
        if (plain_ids(dna, known, reinterpret_cast<const uint8_t *>(rows[k].data()), static_cast<int64_t>(rows[k].size())) != want[k]) ++bad;
    bad += check_batch<int32_t>(dna, known, rows, 5, 1, BSQ_I32, 8192, 0);
    if (bsq_bpe_vocab_size(&dna, 6) != 11 || bsq_bpe_unk_id(&dna, 6) != 10 || bsq_bpe_bos_id(&dna, 6) != -1 || bsq_bpe_pad_id(&dna, 6) != 11) ++bad;
    // fuzz: every element type, both layouts, flags, tables of 0 .. 3000 merges, rows around the 64-position words, cut rows, too-long rows
    const bsq_desc dna_f = make_desc("ACGT", 1, 1, 1), amino = make_desc("ACDEFGHIKLMNPQRSTVWY", 1, 0, 1);
    const int Ms[] = {0, 1, 2, 3, 17, 300, 3000};
    for (int M : Ms) {
        const std::vector<int32_t> t4 = random_table(4, M), t20 = random_table(20, M);
        const std::vector<std::string> r4 = fuzz_rows("ACGT", 30, 200), r20 = fuzz_rows("ACDEFGHIKLMNPQRSTVWY", 20, 200);
        bad += check_batch<int32_t>(dna_f, t4, r4, 50, 1, BSQ_I32, 8192, 0);
        bad += check_batch<uint64_t>(dna_f, t4, r4, 50, 0, BSQ_U64, 150, 1);
        bad += check_batch<int16_t>(amino, t20, r20, 1, 1, BSQ_I16, 8192, 2);
        bad += check_batch<float>(amino, t20, r20, 300, 0, BSQ_F32, 8192, 0);
        bad += check_batch<double>(dna, t4, r4, 64, 1, BSQ_F64, 64, 0);
        if (M <= 100) bad += check_batch<int8_t>(dna, t4, r4, 64, 1, BSQ_I8, 8192, 0);
    }
    // poly-A rows of every length under (A,A), (AA,AA), (AA,A), and one of 8192
    std::vector<std::string> poly;
    for (int n = 1; n <= 200; ++n) poly.push_back(std::string(static_cast<size_t>(n), 'A'));
    bad += check_batch<int8_t>(dna, {0, 0, 4, 4, 4, 0}, poly, 70, 1, BSQ_I8, 8192, 0);
    bad += check_batch<int8_t>(dna, {0, 0, 4, 4, 4, 0}, {std::string(8192, 'A'), std::string(8193, 'A'), std::string(1025, 'A')}, 4100, 1, BSQ_I8, 8192, 0);
    // refusals write nothing
    {
        std::vector<uint8_t> table(static_cast<size_t>(bsq_bpe_table_bytes(4, 2)), 0xAB);
        const int32_t forward[] = {0, 0, 5, 0}, twice[] = {0, 1, 0, 1};
        if (bsq_bpe_table_build(&dna, forward, 2, table.data()) != BSQ_ERR_INVALID_ARG || bsq_bpe_table_build(&dna, twice, 2, table.data()) != BSQ_ERR_INVALID_ARG) ++bad;
        if (std::count(table.begin(), table.end(), 0xAB) != static_cast<std::ptrdiff_t>(table.size())) ++bad;
        if (bsq_bpe_table_bytes(4, 65529) >= 0 || bsq_bpe_table_bytes(4, 65528) != (1 << 20) || bsq_bpe_table_bytes(0, 1) >= 0) ++bad;
        const int32_t ok[] = {0, 0, 4, 0};
        if (bsq_bpe_table_build(&dna, ok, 2, table.data()) != BSQ_OK) ++bad;
        const uint8_t chars[4] = {'A', 'A', 'A', 'C'};
        const int64_t offs[2] = {0, 4};
        int8_t tokens[3] = {99, 99, 99};
        int32_t length = 99;
        const bsq_bpe bad_bpe[] = {{0, 0, 0}, {8193, 0, 0}, {1025, 1, 0}, {8, 3, 0}, {8, 0, 1}};
        for (const bsq_bpe &b : bad_bpe)
            if (bsq_bpe_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, &b, BSQ_I8, tokens, &length) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_bpe_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 200, nullptr, BSQ_I8, tokens, &length) != BSQ_ERR_DTYPE) ++bad;
        if (tokens[0] != 99 || tokens[1] != 99 || tokens[2] != 99 || length != 99) ++bad;
        if (bsq_bpe_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, BSQ_I8, tokens, &length) != BSQ_OK) ++bad;
        if (tokens[0] != 5 || tokens[1] != 1 || tokens[2] != 0 || length != 2) ++bad;
        if (std::strcmp(bsq_bpe_kernel_name(nullptr), "k_bpe_block") != 0 || std::strcmp(bsq_bpe_kernel_name(&bad_bpe[2]), "") != 0) ++bad;
    }
    if (bad) {
        std::printf("BPE_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("BPE_HOST_OK\n");
    return 0;
}
