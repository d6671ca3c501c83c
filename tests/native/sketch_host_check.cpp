// Stand-alone check of bsq_sketch_host.cpp for a sanitizer build (tests/test_minhash_host.py compiles both with
// -fsanitize=address,undefined): hand-made and generated rows -- every length around k, rows of unmapped characters, the largest k of an
// alphabet, where a word uses all 64 bits -- through bsq_minhash_host and bsq_sketch_compare_host, against plain loops written from the
// rule of include/bsq.h.  Every input and output array is a heap block of its exact size, so a read past a row's batch or a write past
// the (B, S) block is an error.  Needs no HIP header.
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

uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bsq_desc make_desc(const char *letters) {
    bsq_desc d;
    std::memset(&d, 0, sizeof(d));
    std::memset(d.lut, -1, sizeof(d.lut));
    int32_t n = 0;
    for (const char *c = letters; *c; ++c) d.lut[uint8_t(*c)] = int8_t(n++);
    d.nchars = n;
    return d;
}

// the rule, word for word
std::vector<uint32_t> reference(const bsq_desc &d, const std::vector<std::string> &rows, const bsq_minhash &m) {
    const size_t S = size_t(m.buckets);
    std::vector<uint32_t> out(rows.size() * S, EMPTY);
    const uint64_t salt = mix64(m.seed ^ 0x534B455443485F5Full);
    for (size_t r = 0; r < rows.size(); ++r) {
        const std::string &row = rows[r];
        for (size_t j = 0; j + size_t(m.k) <= row.size(); ++j) {
            unsigned __int128 fw = 0, rc = 0;
            bool whole = true;
            for (int32_t i = 0; i < m.k; ++i) {
                const int32_t a = d.lut[uint8_t(row[j + size_t(i)])], z = d.lut[uint8_t(row[j + size_t(m.k - 1 - i)])];
                whole = whole && a >= 0;
                fw = fw * unsigned(d.nchars) + unsigned(a < 0 ? 0 : a);
                rc = rc * 4 + unsigned(3 - (z < 0 ? 0 : z));
            }
            if (!whole) continue;
            if ((fw >> 64) != 0) std::printf("a word left 64 bits\n");
            uint64_t word = uint64_t(fw);
            if (m.canonical && uint64_t(rc) < word) word = uint64_t(rc);
            const uint64_t h = mix64(word ^ salt);
            const size_t bucket = size_t(((h >> 32) * uint64_t(S)) >> 32);
            const uint32_t v = uint32_t(h) < 0xFFFFFFFEu ? uint32_t(h) : 0xFFFFFFFEu;
            if (v < out[r * S + bucket]) out[r * S + bucket] = v;
        }
    }
    return out;
}

std::vector<std::string> make_rows(const char *letters, int32_t k) {
    std::vector<std::string> rows;
    const size_t A = std::strlen(letters), K = size_t(k);
    uint64_t state = 12345;
    for (size_t len : {size_t(0), size_t(1), K - 1, K, K + 1, K + 15, K + 16, 2 * K + 3, size_t(700), size_t(3000)}) {
        std::string r(len, 'x');
        for (size_t i = 0; i < len; ++i) {
            state = mix64(state + i + len);
            r[i] = state % 53 == 0 ? '#' : letters[state % A];
        }
        rows.push_back(r);
    }
    rows.push_back(std::string(200, '#'));
    rows.push_back(std::string(200, letters[0]));
    rows.push_back(std::string(200, letters[A - 1]));
    return rows;
}

int check(const char *letters, const bsq_minhash &m) {
    const bsq_desc d = make_desc(letters);
    const std::vector<std::string> rows = make_rows(letters, m.k);
    const int64_t n = int64_t(rows.size());
    std::vector<int64_t> offsets(size_t(n) + 1, 0);
    for (int64_t i = 0; i < n; ++i) offsets[size_t(i) + 1] = offsets[size_t(i)] + int64_t(rows[size_t(i)].size());
    const size_t total = size_t(offsets[size_t(n)]), S = size_t(m.buckets);
    uint8_t *chars = new uint8_t[total];  // (exact size: the last row ends where the block does)
    for (int64_t i = 0; i < n; ++i) std::memcpy(chars + offsets[size_t(i)], rows[size_t(i)].data(), rows[size_t(i)].size());
    const std::vector<uint32_t> exp = reference(d, rows, m);
    int bad = 0;
    int32_t *o32 = new int32_t[size_t(n) * S];
    uint64_t *o64 = new uint64_t[size_t(n) * S];
    if (bsq_minhash_host(&d, chars, offsets.data(), n, &m, BSQ_I32, o32) != BSQ_OK) ++bad;
    if (bsq_minhash_host(&d, chars, offsets.data(), n, &m, BSQ_U64, o64) != BSQ_OK) ++bad;
    size_t filled = 0;
    for (size_t e = 0; e < size_t(n) * S; ++e) {
        if (uint32_t(o32[e]) != exp[e]) ++bad;
        if (o64[e] != (exp[e] == EMPTY ? ~uint64_t(0) : uint64_t(exp[e]))) ++bad;
        filled += exp[e] != EMPTY;
    }
    if (filled == 0) ++bad;  // (a check of nothing)
    // the comparison of the batch with itself and with its first rows, both types, with and without `either`
    const int64_t Bb = n < 3 ? n : 3;
    int32_t *match = new int32_t[size_t(n * Bb)], *either = new int32_t[size_t(n * Bb)], *match64 = new int32_t[size_t(n * Bb)];
    if (bsq_sketch_compare_host(o32, n, o32, Bb, int64_t(S), BSQ_I32, match, either) != BSQ_OK) ++bad;
    if (bsq_sketch_compare_host(o64, n, o64, Bb, int64_t(S), BSQ_U64, match64, nullptr) != BSQ_OK) ++bad;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < Bb; ++j) {
            int32_t mm = 0, ee = 0;
            for (size_t t = 0; t < S; ++t) {
                const uint32_t x = exp[size_t(i) * S + t], y = exp[size_t(j) * S + t];
                mm += x == y && x != EMPTY;
                ee += x != EMPTY || y != EMPTY;
            }
            if (match[i * Bb + j] != mm || either[i * Bb + j] != ee || match64[i * Bb + j] != mm) ++bad;
        }
    delete[] match;
    delete[] either;
    delete[] match64;
    delete[] o32;
    delete[] o64;
    delete[] chars;
    if (bad) std::printf("FAILED: %s k %d S %d canonical %d: %d mismatches\n", letters, m.k, m.buckets, m.canonical, bad);
    return bad;
}

bsq_minhash rule(int32_t k, int32_t S, int32_t canonical, uint64_t seed) {
    bsq_minhash m;
    std::memset(&m, 0, sizeof(m));
    m.k = k, m.buckets = S, m.canonical = canonical, m.seed = seed;
    return m;
}

}  // namespace

int main() {
    int bad = 0;
    for (int32_t k : {1, 3, 16, 17, 21, 31, 32})
        for (int32_t S : {1, 5, 1024}) {
            bad += check("ACGT", rule(k, S, 0, 0));
            bad += check("ACGT", rule(k, S, 1, ~uint64_t(0)));
        }
    bad += check("ACGTN", rule(27, 64, 0, 1));
    bad += check("ACDEFGHIKLMNPQRSTVWY", rule(14, 64, 0, 2));
    bad += check("RY", rule(32, 16384, 0, 3));
    // the argument rules
    const bsq_desc dna = make_desc("ACGT"), dna5 = make_desc("ACGTN"), amino = make_desc("ACDEFGHIKLMNPQRSTVWY");
    const int64_t offs[2] = {0, 4};
    const uint8_t ch[4] = {'A', 'C', 'G', 'T'};
    int32_t out[4] = {7, 7, 7, 7};
    bsq_minhash r = rule(0, 4, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(33, 4, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(28, 4, 0, 0);
    bad += bsq_minhash_host(&dna5, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(15, 4, 0, 0);
    bad += bsq_minhash_host(&amino, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(32, 4, 0, 0);
    bad += bsq_minhash_host(&amino, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(3, 0, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(3, (1 << 14) + 1, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(3, 4, 1, 0);
    bad += bsq_minhash_host(&amino, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    r = rule(3, 4, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_F32, out) != BSQ_ERR_DTYPE;
    r.reserved = 1;
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_ERR_INVALID_ARG;
    for (int32_t v : out) bad += v != 7;
    r = rule(3, 4, 0, 0);
    bad += bsq_minhash_host(&dna, ch, offs, 1, &r, BSQ_I32, out) != BSQ_OK;
    if (bad) {
        std::printf("SKETCH_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("SKETCH_HOST_OK\n");
    return 0;
}
