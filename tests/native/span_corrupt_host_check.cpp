// Stand-alone check of the span-corruption host twin (bsq_span_host.cpp: bsq_span_corrupt_host) under ASan / UBSan: its own main,
// exact-size heap arrays -- a read past the characters or the offsets, or a write past inputs, labels or the two length arrays, is an
// error -- and its own statement of the rule of include/bsq.h ("span corruption") for the answers: a loop over a row's positions.
// Built and run by tests/test_span_corrupt_native.py; no Python, no device.
#include <algorithm>
#include <cmath>
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

// the rule as the header states it
uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
bool anchor(uint64_t h, int64_t a, uint32_t t) {
    if (a < 0) return false;
    const uint64_t w = mix64(h + 0xD1342543DE82EF95ull * (static_cast<uint64_t>(a >> 2) + 1));
    return ((w >> (16 * (a & 3))) & 0xFFFF) < t;
}
void bodies(const bsq_desc &d, const bsq_span_corrupt &m, const std::string &row, uint64_t key, std::vector<int64_t> *in, std::vector<int64_t> *tgt) {
    const uint64_t h = mix64((m.seed ^ 0x5350414E43525054ull) + 0x9E3779B97F4A7C15ull * (key + 1));
    const uint32_t t = static_cast<uint32_t>(std::floor(m.anchor_prob * 65536.0 + 0.5));
    const int64_t L = static_cast<int64_t>(row.size());
    int64_t g = -1;
    bool prev = false;
    for (int64_t j = 0; j < L; ++j) {
        const int32_t id = d.lut[static_cast<uint8_t>(row[static_cast<size_t>(j)])];
        bool cand = false;
        for (int64_t a = std::max<int64_t>(0, j - m.span + 1); a <= j; ++a) cand |= anchor(h, a, t);
        cand = cand && id >= 0;
        if (cand && !prev) ++g;
        if (cand && g < m.max_sentinels) {
            if (!prev) {
                in->push_back(m.sentinel_first + g * m.sentinel_step);
                tgt->push_back(m.sentinel_first + g * m.sentinel_step);
            }
            tgt->push_back(id);
        } else {
            in->push_back(id < 0 ? 0 : id);
        }
        prev = cand;
    }
}

// TI / TL: the element types of in_dt / lab_dt; either matrix and either length array may be left out
template <typename TI, typename TL>
int check_batch(const bsq_desc &d, const std::vector<std::string> &rows, int64_t P_in, int64_t P_tgt, bsq_dtype in_dt, bsq_dtype lab_dt, bsq_span_corrupt m,
                bool want_in = true, bool want_lab = true) {
    const int64_t B = static_cast<int64_t>(rows.size());
    std::vector<int64_t> offs(static_cast<size_t>(B) + 1, 0);
    for (int64_t b = 0; b < B; ++b) offs[static_cast<size_t>(b) + 1] = offs[static_cast<size_t>(b)] + static_cast<int64_t>(rows[static_cast<size_t>(b)].size());
    std::vector<uint8_t> chars(static_cast<size_t>(std::max<int64_t>(offs.back(), 1)));  // (exact size)
    for (int64_t b = 0; b < B; ++b) std::memcpy(chars.data() + offs[static_cast<size_t>(b)], rows[static_cast<size_t>(b)].data(), rows[static_cast<size_t>(b)].size());
    std::vector<TI> inputs(static_cast<size_t>(want_in ? B * P_in : 0));
    std::vector<TL> labels(static_cast<size_t>(want_lab ? B * P_tgt : 0));
    std::vector<int32_t> in_len(static_cast<size_t>(want_in ? B : 0)), tgt_len(static_cast<size_t>(want_lab ? B : 0));
    if (bsq_span_corrupt_host(&d, chars.data(), offs.data(), B, P_in, P_tgt, &m, in_dt, want_in ? inputs.data() : nullptr, lab_dt,
                              want_lab ? labels.data() : nullptr, want_in ? in_len.data() : nullptr, want_lab ? tgt_len.data() : nullptr) != BSQ_OK)
        return std::printf("span_corrupt: %s\n", bsq_internal::g_last.c_str()), 1;
    const int32_t bos = d.bos ? 1 : 0, eos = d.eos ? 1 : 0;
    const int64_t bos_id = d.nchars, eos_id = d.nchars + bos, pad = d.padchar ? d.nchars + bos + eos : 0;
    int bad = 0;
    for (int64_t b = 0; b < B; ++b) {
        std::vector<int64_t> in, tgt;
        bodies(d, m, rows[static_cast<size_t>(b)], static_cast<uint64_t>(m.first_row + b), &in, &tgt);
        std::vector<int64_t> row_in, row_tgt;
        if (bos) row_in.push_back(bos_id);
        for (int64_t e = 0; e < std::min<int64_t>(static_cast<int64_t>(in.size()), std::max<int64_t>(P_in - bos - eos, 0)); ++e) row_in.push_back(in[static_cast<size_t>(e)]);
        if (eos) row_in.push_back(eos_id);
        row_in.resize(static_cast<size_t>(std::max<int64_t>(static_cast<int64_t>(row_in.size()), P_in)), pad);
        for (int64_t e = 0; e < std::min<int64_t>(static_cast<int64_t>(tgt.size()), std::max<int64_t>(P_tgt - eos, 0)); ++e) row_tgt.push_back(tgt[static_cast<size_t>(e)]);
        if (eos) row_tgt.push_back(eos_id);
        row_tgt.resize(static_cast<size_t>(std::max<int64_t>(static_cast<int64_t>(row_tgt.size()), P_tgt)), m.ignore_index);
        for (int64_t e = 0; want_in && e < P_in; ++e)
            if (inputs[static_cast<size_t>(b * P_in + e)] != static_cast<TI>(row_in[static_cast<size_t>(e)])) ++bad;
        for (int64_t e = 0; want_lab && e < P_tgt; ++e)
            if (labels[static_cast<size_t>(b * P_tgt + e)] != static_cast<TL>(row_tgt[static_cast<size_t>(e)])) ++bad;
        if (want_in && in_len[static_cast<size_t>(b)] != static_cast<int32_t>(in.size())) ++bad;
        if (want_lab && tgt_len[static_cast<size_t>(b)] != static_cast<int32_t>(tgt.size())) ++bad;
    }
    if (bad) std::printf("%d wrong values (P %lld %lld, dtypes %d %d, span %d)\n", bad, static_cast<long long>(P_in), static_cast<long long>(P_tgt), static_cast<int>(in_dt), static_cast<int>(lab_dt), m.span);
    return bad;
}

std::vector<std::string> fuzz_rows(const char *letters, int count, int max_len) {
    const int A = static_cast<int>(std::strlen(letters));
    std::vector<std::string> rows = {"", "A", std::string(40, 'N')};
    for (int k = 0; k < count; ++k) {
        std::string s;
        const int n = static_cast<int>(rnd(static_cast<uint32_t>(max_len) + 1));
        while (static_cast<int>(s.size()) < n) s += rnd(k % 3 == 1 ? 6 : 40) == 0 ? '*' : letters[rnd(static_cast<uint32_t>(A))];
        rows.push_back(s);
    }
    return rows;
}

}  // namespace

int main() {
    int bad = 0;
    // the header's known answers
    const bsq_desc dna = make_desc("ACGT", 0, 0, 0), dna_f = make_desc("ACGT", 1, 1, 1), amino = make_desc("ACDEFGHIKLMNPQRSTVWY", 1, 0, 1);
    {
        const std::string all = "ACGTACGTACGTACGTACGTACGNNCGTACGTACACTTTTTTTTTTTTTTTTTTTTTTTT";
        const std::vector<uint8_t> chars(all.begin(), all.end());
        const std::vector<int64_t> offs = {0, 20, 34, 36, 36, 60};
        std::vector<int32_t> inputs(5 * 16), in_len(5), tgt_len(5);
        std::vector<int16_t> labels(5 * 10);
        const bsq_span_corrupt m = {0.2, 3, 100, 4, 1, -100, 7, 0};
        if (bsq_span_corrupt_host(&dna, chars.data(), offs.data(), 5, 16, 10, &m, BSQ_I32, inputs.data(), BSQ_I16, labels.data(), in_len.data(), tgt_len.data()) != BSQ_OK)
            ++bad;
        const int32_t want_in[3][16] = {{0, 1, 2, 3, 4, 3, 0, 5, 1, 2, 3, 0, 6, 0, 0, 0}, {4, 0, 0, 5, 3, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {3, 3, 4, 3, 5, 3, 3, 3, 3, 6, 3, 0, 0, 0, 0, 0}};
        const int16_t want_lab[3][10] = {{4, 0, 1, 2, 5, 1, 2, 3, 0, 6}, {4, 0, 1, 2, 5, 1, 2, 6, 1, 2}, {4, 3, 3, 3, 3, 5, 3, 3, 3, 6}};
        const int rows_of[3] = {0, 1, 4}, want_len[3][2] = {{13, 13}, {7, 13}, {11, 19}};
        for (int r = 0; r < 3; ++r) {
            for (int e = 0; e < 16; ++e)
                if (inputs[static_cast<size_t>(rows_of[r] * 16 + e)] != want_in[r][e]) ++bad;
            for (int e = 0; e < 10; ++e)
                if (labels[static_cast<size_t>(rows_of[r] * 10 + e)] != want_lab[r][e]) ++bad;
            if (in_len[static_cast<size_t>(rows_of[r])] != want_len[r][0] || tgt_len[static_cast<size_t>(rows_of[r])] != want_len[r][1]) ++bad;
        }
        if (bad) std::printf("known answers: %d wrong\n", bad);
    }
    // fuzz: element types on both sides, flags, spans, both steps, the cutoff, widths down to 1, rows of several tiles, each matrix left out
    const std::vector<std::string> r4 = fuzz_rows("ACGT", 30, 300), r20 = fuzz_rows("ACDEFGHIKLMNPQRSTVWY", 20, 300);
    std::vector<std::string> longs = {std::string(1023, 'A'), std::string(1024, 'C'), std::string(1025, 'G'), std::string(2051, 'T'), std::string(1030, 'A')};
    for (int k = 1016; k < 1028; ++k) longs[4][static_cast<size_t>(k)] = 'N';  // unmapped bytes across the seam of two tiles
    const int spans[] = {1, 3, 16};
    for (int span : spans) {
        bad += check_batch<int32_t, uint64_t>(dna_f, r4, 320, 200, BSQ_I32, BSQ_U64, {0.15, span, 100, 7, 1, -100, 1, 0});
        bad += check_batch<uint64_t, int16_t>(dna_f, r4, 50, 31, BSQ_U64, BSQ_I16, {0.5, span, 2, 300, -1, -1, 2, 1000});
        bad += check_batch<int16_t, float>(amino, r20, 1, 1, BSQ_I16, BSQ_F32, {1.0, span, 100, 22, 1, -100, 3, 7});
        bad += check_batch<float, double>(amino, r20, 300, 2, BSQ_F32, BSQ_F64, {0.9, span, 1, 1000, -1, -100, 4, 0}, true, false);
        bad += check_batch<double, int32_t>(dna, r4, 64, 8, BSQ_F64, BSQ_I32, {0.3, span, 65535, 4, 1, 70000, 5, int64_t(1) << 40}, false, true);
        bad += check_batch<int8_t, int8_t>(dna, r4, 2, 16, BSQ_I8, BSQ_I8, {0.0, span, 100, 27, 1, -100, 6, 0});
        bad += check_batch<int16_t, int16_t>(dna, longs, 2100, 2100, BSQ_I16, BSQ_I16, {1.0, span, 100, 4, 1, -100, 7, 0});
        bad += check_batch<int16_t, int16_t>(dna_f, longs, 1024, 1025, BSQ_I16, BSQ_I16, {0.05, span, 3, 2000, -1, -100, 8, 0});
    }
    // refusals write nothing
    {
        const uint8_t chars[4] = {'A', 'A', 'A', 'C'};
        const int64_t offs[2] = {0, 4};
        int8_t inputs[3] = {99, 99, 99}, labels[3] = {99, 99, 99};
        int32_t lens[2] = {99, 99};
        const bsq_span_corrupt bad_m[] = {{-0.5, 3, 100, 7, 1, -100, 1, 0}, {0.5, 0, 100, 7, 1, -100, 1, 0}, {0.5, 17, 100, 7, 1, -100, 1, 0}, {0.5, 3, 0, 7, 1, -100, 1, 0},
                                          {0.5, 3, 65536, 7, 1, -100, 1, 0}, {0.5, 3, 100, 7, 0, -100, 1, 0}, {0.5, 3, 100, 6, 1, -100, 1, 0}, {0.5, 3, 100, 50, -1, -100, 1, 0},
                                          {0.5, 3, 100, (int64_t(1) << 31) - 50, 1, -100, 1, 0}, {0.5, 3, 100, 7, 1, -100, 1, -1}};
        for (const bsq_span_corrupt &m : bad_m)
            if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, &m, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_INVALID_ARG) ++bad;
        const bsq_span_corrupt good = {0.5, 3, 10, 7, 1, -100, 1, 0}, wide = {0.5, 3, 100, 100, 1, -100, 1, 0}, low = {0.5, 3, 10, 7, 1, -200, 1, 0};
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, nullptr, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, &good, BSQ_I8, nullptr, BSQ_I8, nullptr, lens, lens + 1) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 0, 3, &good, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 0, &good, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_INVALID_ARG) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, &wide, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_DTYPE) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, &low, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_ERR_DTYPE) ++bad;
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 0, 3, 3, &good, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_OK) ++bad;
        for (int k = 0; k < 3; ++k)
            if (inputs[k] != 99 || labels[k] != 99) ++bad;
        if (lens[0] != 99 || lens[1] != 99) ++bad;
        const bsq_span_corrupt none = {0.0, 3, 10, 7, 1, -100, 1, 0};
        if (bsq_span_corrupt_host(&dna_f, chars, offs, 1, 3, 3, &none, BSQ_I8, inputs, BSQ_I8, labels, lens, lens + 1) != BSQ_OK) ++bad;
        if (inputs[0] != 4 || inputs[1] != 0 || inputs[2] != 5 || labels[0] != 5 || labels[1] != -100 || labels[2] != -100 || lens[0] != 4 || lens[1] != 0) ++bad;
    }
    if (bad) {
        std::printf("SPAN_CORRUPT_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("SPAN_CORRUPT_HOST_OK\n");
    return 0;
}
