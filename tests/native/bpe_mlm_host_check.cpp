// Stand-alone check of the BPE masked-LM host twin (bsq_bpe_mlm_host.cpp: bsq_bpe_mlm_tokenize_host) under ASan / UBSan: its own main,
// exact-size heap arrays -- a read past the characters, the offsets or the table, or a write past inputs, labels or lengths, is an
// error -- and its own one-merge-at-a-time programme and its own statement of the draw for the answers.  Built and run by
// tests/test_bpe_mlm_native.py; no Python, no device.
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
std::vector<int32_t> plain_ids(const bsq_desc &d, const std::vector<int32_t> &merges, const std::string &row) {
    const int32_t M = static_cast<int32_t>(merges.size() / 2), V = d.nchars + M;
    std::map<std::pair<int32_t, int32_t>, int32_t> rank;
    for (int32_t m = 0; m < M; ++m) rank[{merges[2 * m], merges[2 * m + 1]}] = m;
    std::vector<int32_t> sym;
    for (char c : row) sym.push_back(d.lut[static_cast<uint8_t>(c)] < 0 ? V : d.lut[static_cast<uint8_t>(c)]);
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

// the draw as the header states it
uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint32_t threshold(double p) { return static_cast<uint32_t>(p * 65536.0 + 0.5); }
void draw(const bsq_bpe_mlm &m, uint64_t row, int64_t j, int64_t id, int64_t V, int64_t *input, int64_t *label) {
    const uint64_t h = mix64((m.seed ^ 0x4250454D4C4D534Bull) + 0x9E3779B97F4A7C15ull * (row + 1));
    const uint64_t w = mix64(h + 0xD1342543DE82EF95ull * (static_cast<uint64_t>(j >> 2) + 1));
    *input = id;
    *label = m.ignore_index;
    if (id == V || ((w >> (16 * (j & 3))) & 0xFFFF) >= threshold(m.frac)) return;
    const uint64_t v = mix64(~h + 0xD1342543DE82EF95ull * (static_cast<uint64_t>(j) + 1));
    const uint64_t cat = v & 0xFFFF, r = (v >> 16) & 0xFFFFFFFFull;
    *label = id;
    if (cat < threshold(m.mask_prob)) *input = m.mask_token;
    else if (cat < threshold(m.mask_prob) + threshold(m.random_prob)) *input = static_cast<int64_t>((r * static_cast<uint64_t>(V)) >> 32);
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

// TI / TL: the element types of in_dt / lab_dt; either output may be left out
template <typename TI, typename TL>
int check_batch(const bsq_desc &d, const std::vector<int32_t> &merges, const std::vector<std::string> &rows, int64_t P, int32_t batch_first,
                bsq_dtype in_dt, bsq_dtype lab_dt, int32_t max_chars, bsq_bpe_mlm m, bool want_in = true, bool want_lab = true) {
    const int64_t M = static_cast<int64_t>(merges.size() / 2), B = static_cast<int64_t>(rows.size());
    std::vector<uint8_t> table(static_cast<size_t>(bsq_bpe_table_bytes(d.nchars, M)));  // (exact size)
    if (bsq_bpe_table_build(&d, merges.data(), M, table.data()) != BSQ_OK) return std::printf("build: %s\n", bsq_internal::g_last.c_str()), 1;
    std::vector<int64_t> offs(static_cast<size_t>(B) + 1, 0);
    for (int64_t b = 0; b < B; ++b) offs[static_cast<size_t>(b) + 1] = offs[static_cast<size_t>(b)] + static_cast<int64_t>(rows[static_cast<size_t>(b)].size());
    std::vector<uint8_t> chars(static_cast<size_t>(std::max<int64_t>(offs.back(), 1)));
    for (int64_t b = 0; b < B; ++b) std::memcpy(chars.data() + offs[static_cast<size_t>(b)], rows[static_cast<size_t>(b)].data(), rows[static_cast<size_t>(b)].size());
    std::vector<TI> inputs(static_cast<size_t>(want_in ? B * P : 0));
    std::vector<TL> labels(static_cast<size_t>(want_lab ? B * P : 0));
    std::vector<int32_t> lengths(static_cast<size_t>(B));
    const bsq_bpe bpe = {max_chars, 0, 0};
    if (bsq_bpe_mlm_tokenize_host(&d, chars.data(), offs.data(), B, P, batch_first, table.data(), M, &bpe, &m, in_dt, want_in ? inputs.data() : nullptr,
                                  lab_dt, want_lab ? labels.data() : nullptr, lengths.data()) != BSQ_OK)
        return std::printf("tokenize: %s\n", bsq_internal::g_last.c_str()), 1;
    const int32_t V = d.nchars + static_cast<int32_t>(M), bos = d.bos ? 1 : 0, eos = d.eos ? 1 : 0;
    const int32_t pad_store = d.padchar ? V + 1 + bos + eos : 0;
    int bad = 0;
    for (int64_t b = 0; b < B; ++b) {
        const std::string &row = rows[static_cast<size_t>(b)];
        const bool too_long = static_cast<int64_t>(row.size()) > max_chars;
        std::vector<int32_t> ids;
        if (!too_long) ids = plain_ids(d, merges, row);
        if (lengths[static_cast<size_t>(b)] != (too_long ? -1 : static_cast<int32_t>(ids.size()))) ++bad;
        const int64_t nn = std::min<int64_t>(static_cast<int64_t>(ids.size()), std::max<int64_t>(P - bos - eos, 0));
        for (int64_t pos = 0; pos < P; ++pos) {
            const int64_t j = pos - bos;
            int64_t in = j < 0 ? V + 1 : ((eos && j == nn) ? V + 1 + bos : pad_store), lab = m.ignore_index;
            if (j >= 0 && j < nn) draw(m, static_cast<uint64_t>(m.first_row + b), j, ids[static_cast<size_t>(j)], V, &in, &lab);
            const size_t e = static_cast<size_t>(batch_first ? b * P + pos : pos * B + b);
            if (want_in && inputs[e] != static_cast<TI>(in)) ++bad;
            if (want_lab && labels[e] != static_cast<TL>(lab)) ++bad;
        }
    }
    if (bad) std::printf("%d wrong values (M %lld, P %lld, dtypes %d %d)\n", bad, static_cast<long long>(M), static_cast<long long>(P), static_cast<int>(in_dt), static_cast<int>(lab_dt));
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
    // the header's known answers: frac 0.5, seed 7, first_row 0
    const bsq_desc dna = make_desc("ACGT", 0, 0, 0);
    const std::vector<int32_t> known = {0, 0, 1, 2, 4, 0, 5, 3, 4, 4, 3, 3};
    const std::vector<std::string> rows = {"AAAAAAA", "ACGTACGT", "AAACGTNAAAA", "TTTTT"};
    {
        std::vector<uint8_t> table(static_cast<size_t>(bsq_bpe_table_bytes(4, 6)));
        if (bsq_bpe_table_build(&dna, known.data(), 6, table.data()) != BSQ_OK) ++bad;
        const std::string all = rows[0] + rows[1] + rows[2] + rows[3];
        std::vector<uint8_t> chars(all.begin(), all.end());
        const std::vector<int64_t> offs = {0, 7, 15, 26, 31};
        std::vector<int32_t> inputs(16), lengths(4);
        std::vector<int8_t> labels(16);
        const bsq_bpe_mlm m = {0.5, 0.8, 0.1, 11, -100, 7, 0};
        if (bsq_bpe_mlm_tokenize_host(&dna, chars.data(), offs.data(), 4, 4, 1, table.data(), 6, nullptr, &m, BSQ_I32, inputs.data(), BSQ_I8, labels.data(),
                                      lengths.data()) != BSQ_OK)
            ++bad;
        const int32_t want_in[16] = {11, 11, 0, 0, 0, 7, 11, 7, 6, 11, 10, 11, 2, 9, 3, 0};
        const int8_t want_lab[16] = {8, 6, -100, -100, -100, -100, 0, 7, -100, 7, -100, 8, 9, -100, -100, -100};
        for (int k = 0; k < 16; ++k)
            if (inputs[static_cast<size_t>(k)] != want_in[k] || labels[static_cast<size_t>(k)] != want_lab[k]) ++bad;
        if (lengths != std::vector<int32_t>{2, 4, 4, 3}) ++bad;
    }
    // fuzz: element types on both sides, both layouts, flags, tables of 0 .. 3000 merges, cut rows, too-long rows, each output left out
    const bsq_desc dna_f = make_desc("ACGT", 1, 1, 1), amino = make_desc("ACDEFGHIKLMNPQRSTVWY", 1, 0, 1);
    const int Ms[] = {0, 1, 3, 17, 300, 3000};
    for (int M : Ms) {
        const std::vector<int32_t> t4 = random_table(4, M), t20 = random_table(20, M);
        const std::vector<std::string> r4 = fuzz_rows("ACGT", 30, 200), r20 = fuzz_rows("ACDEFGHIKLMNPQRSTVWY", 20, 200);
        const int64_t v4 = 4 + M + 4, v20 = 20 + M + 3;
        bad += check_batch<int32_t, uint64_t>(dna_f, t4, r4, 50, 1, BSQ_I32, BSQ_U64, 8192, {0.15, 0.8, 0.1, v4, -100, 1, 0});
        bad += check_batch<uint64_t, int16_t>(dna_f, t4, r4, 50, 0, BSQ_U64, BSQ_I16, 150, {0.5, 0.5, 0.5, v4 + 9, -1, 2, 1000});
        bad += check_batch<int16_t, float>(amino, t20, r20, 1, 1, BSQ_I16, BSQ_F32, 8192, {1.0, 0.8, 0.1, v20, -100, 3, 7});
        bad += check_batch<float, double>(amino, t20, r20, 300, 0, BSQ_F32, BSQ_F64, 8192, {0.9, 0.0, 1.0, v20, -100, 4, 0}, true, false);
        bad += check_batch<double, int32_t>(dna, t4, r4, 64, 1, BSQ_F64, BSQ_I32, 64, {0.3, 1.0, 0.0, 4 + M + 1, 70000, 5, int64_t(1) << 40}, false, true);
        if (M <= 100) bad += check_batch<int8_t, int8_t>(dna, t4, r4, 64, 1, BSQ_I8, BSQ_I8, 8192, {0.0, 0.8, 0.1, 4 + M + 1, -100, 6, 0});
    }
    // rows at the bound of both forms, and one past the call's reach
    bad += check_batch<int16_t, int16_t>(dna, {0, 0, 4, 4, 4, 0}, {std::string(8192, 'A'), std::string(8193, 'A'), std::string(1025, 'C'), std::string(1024, 'A')},
                                         2100, 1, BSQ_I16, BSQ_I16, 8192, {0.15, 0.8, 0.1, 8, -100, 7, 0});
    // refusals write nothing
    {
        std::vector<uint8_t> table(static_cast<size_t>(bsq_bpe_table_bytes(4, 2)));
        const int32_t ok[] = {0, 0, 4, 0};
        if (bsq_bpe_table_build(&dna, ok, 2, table.data()) != BSQ_OK) ++bad;
        const uint8_t chars[4] = {'A', 'A', 'A', 'C'};
        const int64_t offs[2] = {0, 4};
        int8_t inputs[3] = {99, 99, 99}, labels[3] = {99, 99, 99};
        int32_t length = 99;
        const bsq_bpe_mlm good = {0.5, 0.8, 0.1, 7, -100, 1, 0};
        const bsq_bpe_mlm bad_m[] = {{-0.5, 0.8, 0.1, 7, -100, 1, 0}, {0.5, 0.8, 0.3, 7, -100, 1, 0}, {0.5, 0.8, 0.1, -1, -100, 1, 0}, {0.5, 0.8, 0.1, 7, -100, 1, -1}};
        for (const bsq_bpe_mlm &m : bad_m)
            if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, &m, BSQ_I8, inputs, BSQ_I8, labels, &length) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, nullptr, BSQ_I8, inputs, BSQ_I8, labels, &length) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, &good, BSQ_I8, nullptr, BSQ_I8, nullptr, &length) != BSQ_ERR_INVALID_ARG) ++bad;
        const bsq_bpe_mlm wide = {0.5, 0.8, 0.1, 200, -100, 1, 0}, low = {0.5, 0.8, 0.1, 7, -200, 1, 0};
        if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, &wide, BSQ_I8, inputs, BSQ_I8, labels, &length) != BSQ_ERR_DTYPE) ++bad;
        if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, &low, BSQ_I8, inputs, BSQ_I8, labels, &length) != BSQ_ERR_DTYPE) ++bad;
        for (int k = 0; k < 3; ++k)
            if (inputs[k] != 99 || labels[k] != 99) ++bad;
        if (length != 99) ++bad;
        const bsq_bpe_mlm none = {0.0, 0.8, 0.1, 7, -100, 1, 0};
        if (bsq_bpe_mlm_tokenize_host(&dna, chars, offs, 1, 3, 1, table.data(), 2, nullptr, &none, BSQ_I8, inputs, BSQ_I8, labels, &length) != BSQ_OK) ++bad;
        if (inputs[0] != 5 || inputs[1] != 1 || inputs[2] != 0 || labels[0] != -100 || labels[2] != -100 || length != 2) ++bad;
        const bsq_bpe wave = {1024, 0, 0}, refused = {1025, 1, 0};
        if (std::strcmp(bsq_bpe_mlm_kernel_name(nullptr), "k_bpe_mlm_block") != 0 || std::strcmp(bsq_bpe_mlm_kernel_name(&wave), "k_bpe_mlm_wave") != 0 ||
            std::strcmp(bsq_bpe_mlm_kernel_name(&refused), "") != 0)
            ++bad;
    }
    if (bad) {
        std::printf("BPE_MLM_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("BPE_MLM_HOST_OK\n");
    return 0;
}
