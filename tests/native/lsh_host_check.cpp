// Stand-alone check of bsq_lsh_keys_host, bsq_sketch_compare_list_host and bsq_lsh_pairs_host (bsq_lsh_host.cpp) for a sanitizer build
// (tests/test_lsh_native.py compiles both with -fsanitize=address,undefined): generated sketch matrices of both element types with
// EMPTY buckets, planted identical groups on either side of max_bucket and an ignored tail, against a reference of its own written from
// the rule of include/bsq.h ("LSH candidates of a sketch matrix") -- the key chain restated, and every PAIR of rows tested for a shared
// band key, with the centre rule decided by counting a key's rows: no sort, no runs.  Every input and output array is a heap block of
// its exact size, so a read past a row, a row looked up from an index out of range (both ends of int64 in the list compare), or a write
// past an output is an error.  Needs no HIP header.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
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

constexpr uint32_t E = 0xFFFFFFFFu;

uint64_t next(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int64_t ref_key(const std::vector<uint32_t> &v, int64_t S, int64_t i, int r, int t, uint64_t seed) {
    uint64_t h = mix(mix(seed ^ 0x4C53485F42414E44ull) + 0x9E3779B97F4A7C15ull * uint64_t(t + 1));
    bool all_empty = true;
    for (int q = 0; q < r; ++q) {
        const uint32_t x = v[size_t(i * S + t * r + q)];
        all_empty = all_empty && x == E;
        h = mix(h ^ x);
    }
    return all_empty ? -1 : int64_t(h >> 1);
}

void ref_counts(const std::vector<uint32_t> &v, int64_t S, int64_t i, int64_t j, int32_t *m, int32_t *e) {
    *m = *e = 0;
    for (int64_t s = 0; s < S; ++s) {
        const uint32_t x = v[size_t(i * S + s)], y = v[size_t(j * S + s)];
        *m += x == y && x != E;
        *e += x != E || y != E;
    }
}

// the candidates of the N rows of v, by pairs: (i, j), i < j, share band t's key, and either the key has at most max_bucket rows or i is
// the smallest row that holds it
std::set<std::pair<int64_t, int64_t>> ref_candidates(const std::vector<uint32_t> &v, int64_t N, int64_t S, int r, int max_bucket, uint64_t seed,
                                                     int64_t *before_union) {
    std::set<std::pair<int64_t, int64_t>> out;
    *before_union = 0;
    for (int t = 0; t < S / r; ++t) {
        std::vector<int64_t> key(static_cast<size_t>(N));
        for (int64_t i = 0; i < N; ++i) key[size_t(i)] = ref_key(v, S, i, r, t, seed);
        for (int64_t j = 0; j < N; ++j) {
            if (key[size_t(j)] == -1) continue;
            int64_t holders = 0, smallest = -1;
            for (int64_t i = 0; i < N; ++i)
                if (key[size_t(i)] == key[size_t(j)]) {
                    ++holders;
                    if (smallest < 0) smallest = i;
                }
            for (int64_t i = 0; i < j; ++i)
                if (key[size_t(i)] == key[size_t(j)] && (holders <= max_bucket || i == smallest)) out.insert({i, j}), ++*before_union;
        }
    }
    return out;
}

template <typename T>
T *matrix_of(const std::vector<uint32_t> &v) {  // an exact-size heap block in the element type
    T *p = new T[v.size()];
    for (size_t k = 0; k < v.size(); ++k) p[k] = sizeof(T) == 8 && v[k] == E ? T(~uint64_t(0)) : T(v[k]);
    return p;
}

template <typename T>
int check(int64_t Ba, int64_t Bb, int64_t S, int r, int max_bucket, uint64_t seed, bsq_dtype t, int64_t *listed) {
    const int64_t N = Ba + Bb;
    uint64_t state = seed * 977 + uint64_t(N);
    std::vector<uint32_t> v(size_t(N * S));
    for (auto &x : v) x = next(state) % 4 == 0 ? E : uint32_t(next(state) % 0xFFFFFFFFull);
    // identical groups of max_bucket and max_bucket + 1 rows (scattered over both matrices), a row EMPTY throughout, near-copies
    for (int64_t k = 1; k <= 2 * max_bucket && 3 * k + 1 < N; ++k) {
        const int64_t src = k <= max_bucket ? 0 : 1, dst = 3 * k + (k <= max_bucket ? 0 : 1);
        if (dst < N && k != max_bucket) std::copy(v.begin() + src * S, v.begin() + (src + 1) * S, v.begin() + dst * S);
    }
    if (N > 2) std::fill(v.begin() + 2 * S, v.begin() + 3 * S, E);
    for (int64_t i = 5; i < N; i += 4)
        for (int64_t s = 0; s < S; ++s)
            if (next(state) % 5 != 0) v[size_t(i * S + s)] = v[size_t((i - 1) * S + s)];
    T *a = matrix_of<T>(std::vector<uint32_t>(v.begin(), v.begin() + Ba * S));
    T *b = Bb ? matrix_of<T>(std::vector<uint32_t>(v.begin() + Ba * S, v.end())) : nullptr;
    const bsq_lsh lsh{r, max_bucket, seed, 0};
    int bad = 0;
    // keys: a then b through the pitch, exact size
    const int64_t bands = S / r;
    int64_t *keys = new int64_t[size_t(bands * N)];
    bad += bsq_lsh_keys_host(a, Ba, S, t, &lsh, keys, N) != BSQ_OK;
    if (Bb) bad += bsq_lsh_keys_host(b, Bb, S, t, &lsh, keys + Ba, N) != BSQ_OK;
    for (int tt = 0; tt < bands; ++tt)
        for (int64_t i = 0; i < N; ++i) bad += keys[tt * N + i] != ref_key(v, S, i, r, tt, seed);
    delete[] keys;
    // the whole rule
    int64_t before = 0;
    const auto cand = ref_candidates(v, N, S, r, max_bucket, seed, &before);
    const bsq_sketch_pairs rule{1, 32768, 0, 0};
    std::vector<std::pair<int64_t, int64_t>> want;
    for (const auto &p : cand) {
        if (Bb && !(p.first < Ba && p.second >= Ba)) continue;
        int32_t m, e;
        ref_counts(v, S, p.first, p.second, &m, &e);
        if (m >= 1 && int64_t(m) * 65536 >= int64_t(32768) * e) want.push_back({p.first, Bb ? p.second - Ba : p.second});
    }
    int64_t total = -1, *offs = new int64_t[size_t(Ba + 1)];
    bad += bsq_lsh_pairs_host(a, Ba, b, Bb, S, t, &lsh, &rule, -1, &total, offs, 0, nullptr, nullptr, nullptr, nullptr) != BSQ_OK;
    bad += total != before || offs[Ba] != int64_t(want.size());
    const size_t n = want.size();
    int64_t *row = new int64_t[n], *col = new int64_t[n];
    int32_t *match = new int32_t[n], *either = new int32_t[n];
    bad += bsq_lsh_pairs_host(a, Ba, b, Bb, S, t, &lsh, &rule, before, &total, offs, int64_t(n), row, col, match, either) != BSQ_OK;
    for (size_t k = 0; k < n; ++k) {
        int32_t m, e;
        ref_counts(v, S, want[k].first, want[k].second + (Bb ? Ba : 0), &m, &e);
        bad += row[k] != want[k].first || col[k] != want[k].second || match[k] != m || either[k] != e;
    }
    for (int64_t i = 0; i <= Ba; ++i) {
        int64_t below = 0;
        for (const auto &p : want) below += p.first < i;
        bad += offs[i] != below;
    }
    // a limit below the candidates: only the count is written
    if (before > 0) {
        offs[0] = -7;
        bad += bsq_lsh_pairs_host(a, Ba, b, Bb, S, t, &lsh, &rule, before - 1, &total, offs, int64_t(n), row, col, match, either) != BSQ_OK;
        bad += total != before || offs[0] != -7;
        offs[0] = 0;
    }
    // the candidates alone, without match and either
    bad += bsq_lsh_pairs_host(a, Ba, b, Bb, S, t, &lsh, nullptr, -1, &total, offs, 0, nullptr, nullptr, nullptr, nullptr) != BSQ_OK;
    int64_t crossing = 0;
    for (const auto &p : cand) crossing += !Bb || (p.first < Ba && p.second >= Ba);
    bad += offs[Ba] != crossing;
    // the list compare over the listed pairs and junk indices at both ends of int64
    const int64_t junk[6][2] = {{-1, 0}, {0, -1}, {Ba, 0}, {0, Bb ? Bb : Ba}, {INT64_MIN, 0}, {0, INT64_MAX}};
    const size_t len = n + 6;
    int64_t *lr = new int64_t[len], *lc = new int64_t[len];
    int32_t *lm = new int32_t[len], *le = new int32_t[len];
    for (size_t k = 0; k < n; ++k) lr[k] = row[k], lc[k] = col[k];
    for (size_t k = 0; k < 6; ++k) lr[n + k] = junk[k][0], lc[n + k] = junk[k][1];
    bad += bsq_sketch_compare_list_host(a, Ba, Bb ? b : a, Bb ? Bb : Ba, S, t, lr, lc, int64_t(len), lm, le) != BSQ_OK;
    for (size_t k = 0; k < n; ++k) bad += lm[k] != match[k] || le[k] != either[k];
    for (size_t k = n; k < len; ++k) bad += lm[k] != -1 || le[k] != -1;
    bad += bsq_sketch_compare_list_host(a, Ba, Bb ? b : a, Bb ? Bb : Ba, S, t, lr, lc, int64_t(len), lm, nullptr) != BSQ_OK;
    *listed += int64_t(n);
    if (bad) std::printf("FAILED: Ba %lld Bb %lld S %lld r %d max_bucket %d type %d: %d mismatches\n", (long long)Ba, (long long)Bb, (long long)S, r,
                         max_bucket, int(t), bad);
    delete[] a;
    delete[] b;
    delete[] offs;
    delete[] row;
    delete[] col;
    delete[] match;
    delete[] either;
    delete[] lr;
    delete[] lc;
    delete[] lm;
    delete[] le;
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    int64_t listed = 0;
    // (Ba, Bb, S, r, max_bucket)
    const int64_t shapes[8][5] = {{1, 0, 4, 2, 2}, {40, 0, 8, 2, 4}, {40, 0, 8, 3, 4}, {25, 30, 8, 1, 4}, {64, 0, 16, 16, 3}, {30, 35, 7, 2, 2}, {50, 0, 5, 5, 32},
                                  {0, 20, 8, 2, 4}};
    for (const auto &s : shapes) {
        bad += check<int32_t>(s[0], s[1], s[2], int(s[3]), int(s[4]), uint64_t(s[0] + 3), BSQ_I32, &listed);
        bad += check<uint64_t>(s[0], s[1], s[2], int(s[3]), int(s[4]), uint64_t(s[1] + 11), BSQ_U64, &listed);
    }
    if (listed < 200) ++bad;  // (a check of nothing)
    // a header known answer: (7 E 9 E) twice, r = 1, band 0
    {
        const int32_t m[8] = {7, -1, 9, -1, 7, -1, 9, -1};
        const bsq_lsh lsh{1, 32, 0, 0};
        int64_t keys[8];
        bad += bsq_lsh_keys_host(m, 2, 4, BSQ_I32, &lsh, keys, 2) != BSQ_OK;
        bad += keys[0] != 5027150649341863934ll || keys[1] != keys[0] || keys[2] != -1 || keys[4] != 4432986889740121373ll || keys[6] != -1;
    }
    // the argument rules: a refusal writes nothing
    {
        const int32_t m[4] = {1, 2, 3, 4};
        int64_t keys[2] = {-7, -7}, total = -7, offs[2] = {-7, -7};
        const bsq_lsh zero{0, 32, 0, 0}, wide{5, 32, 0, 0}, small{2, 1, 0, 0}, reserved{2, 32, 0, 1}, good{2, 32, 0, 0};
        for (const bsq_lsh *l : {&zero, &wide, &small, &reserved, static_cast<const bsq_lsh *>(nullptr)}) {
            bad += bsq_lsh_keys_host(m, 1, 4, BSQ_I32, l, keys, 1) != BSQ_ERR_INVALID_ARG;
            bad += bsq_lsh_pairs_host(m, 1, nullptr, 0, 4, BSQ_I32, l, nullptr, -1, &total, offs, 0, nullptr, nullptr, nullptr, nullptr) != BSQ_ERR_INVALID_ARG;
        }
        bad += bsq_lsh_keys_host(m, 1, 4, BSQ_I8, &good, keys, 1) != BSQ_ERR_DTYPE;
        bad += bsq_lsh_keys_host(m, 1, 4, BSQ_I32, &good, keys, 0) != BSQ_ERR_INVALID_ARG;
        bad += bsq_lsh_keys_host(m, -1, 4, BSQ_I32, &good, keys, 1) != BSQ_ERR_INVALID_ARG;
        bad += bsq_lsh_keys_host(nullptr, 1, 4, BSQ_I32, &good, keys, 1) != BSQ_ERR_INVALID_ARG;
        bad += bsq_lsh_pairs_host(m, 1, nullptr, 1, 4, BSQ_I32, &good, nullptr, -1, &total, offs, 0, nullptr, nullptr, nullptr, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += bsq_lsh_pairs_host(m, 1, nullptr, 0, 4, BSQ_I32, &good, nullptr, -1, nullptr, offs, 0, nullptr, nullptr, nullptr, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += bsq_sketch_compare_list_host(m, 1, m, 1, 4, BSQ_I32, nullptr, nullptr, 1, nullptr, nullptr) != BSQ_ERR_INVALID_ARG;
        bad += keys[0] != -7 || keys[1] != -7 || total != -7 || offs[0] != -7 || offs[1] != -7;
        bad += bsq_lsh_keys_host(nullptr, 0, 4, BSQ_I32, &good, nullptr, 0) != BSQ_OK;
    }
    if (bad) {
        std::printf("LSH_HOST_FAILED %d\n", bad);
        return 1;
    }
    std::printf("LSH_HOST_OK %lld pairs listed\n", (long long)listed);
    return 0;
}
