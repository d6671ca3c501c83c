// MinHash sketches of a packed batch, the all-pairs comparison of sketches and the thresholded pair list (include/bsq.h, "MinHash
// sketch", "sketch pairs"): what the kernels of bsq_sketch.hip and the CPU twins of bsq_sketch_host.cpp share -- the limits, the wide
// geometry of a (tokenizer, bsq_minhash) pair, the reverse complement of a 64-bit word, the hash, the bucket and value of a hash, the
// value of one output element, the choice of kernel, the selection of a pair, the segments of a strip, the find and union of the
// clusters ("sketch clusters") and the argument rules.  Plain C++
// over <cstdint> and bsq.h alone: the host twins compile without the HIP headers.
#pragma once
#include <cstdint>

#include "bsq.h"
#include "bsq_row_table.h"

#if defined(__HIPCC__)
#define BSQ_SKETCH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BSQ_SKETCH_HD inline
#endif

namespace bsq_sketchd {

constexpr int32_t kMaxK = 32;                          // a word is one unsigned 64-bit value: A^k <= 2^64
constexpr int64_t kMaxBuckets = int64_t(1) << 14;      // S: the largest u32 table one workgroup keeps in LDS (64 KiB)
constexpr int64_t kMaxWindows = int64_t(1) << 30;      // windows a row sketches: window indices stay far inside 32 bits
constexpr uint32_t kEmpty = 0xFFFFFFFFu;               // a bucket no window fell into
constexpr uint64_t kDomain = 0x534B455443485F5Full;    // the sketch's own hash domain ("SKETCH__")
// The choice between the forms at S <= 1024, from the mean row length total_chars / B.  The starting values were the spectrum's
// (bsq_kmer_spectrum_dev.h: 2048, 4096 rows, 16384); scripts/minhash_lab.py on an MI355X measured this kernel over the same grid of row
// lengths and row counts (profiles/r19/minhash_lab.txt: DNA4, k = 21, canonical, S = 1024, int32, cold; wave / block time, < 1: the wave
// form wins):
//     128 Mi characters in rows of L     L = 256: 0.47   512: 0.47   1024: 0.48   2048: 0.71   4096: 0.99   8192: 1.04   16384: 1.09   65536: 1.40
//     few rows of L = 1024 / 4096 / 16384     B = 64: 1.08 / 2.49 / 3.33     B = 512: 1.02 / 2.20 / 2.81     B = 4096: 0.62 / 1.14 / 1.18
// A window costs this kernel more arithmetic than it costs the spectrum (two 64-bit multiplications), so a long row is worth a
// workgroup's four waves earlier: in a batch of many rows the two forms meet at ~4 K characters per row (0.99 at 32 768 rows, 1.14 at
// 4 096), not at ~16 K; a batch of few rows still leaves most CUs idle and takes the block form from ~2 K characters on (at 1024
// characters the two are within 12 % either way).  Hence 2048 and 4096 rows stay and the third constant is 4096.
constexpr int64_t kBlockChars = 2048;      // mean characters per row from which the block form is taken ...
constexpr int64_t kManyRows = 4096;        // ... in a batch of fewer rows than this;
constexpr int64_t kBlockCharsMany = 4096;  // ... in a batch of at least that many rows

// splitmix64's finalizer (bsq_mlm_dev.h has the same text; that header needs the HIP runtime, this one must not)
BSQ_SKETCH_HD uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A (tokenizer, bsq_minhash) pair checked and reduced to what a row reads (made on the host)
struct Geometry {
    uint64_t lead;  // A^(k-1): the weight of a window's first character
    uint64_t mask;  // A == 4: the low 2k bits, what a word keeps when it rolls by a shift
    uint64_t salt;  // s' = mix64(seed ^ kDomain)
    int32_t k, A, S;
    int32_t canonical;  // 0 / 1
};

// windows of a row of length L (as read from the offsets: a negative one counts as 0), clamped to kMaxWindows
BSQ_SKETCH_HD int64_t row_windows(int64_t L, int32_t k) {
    const int64_t n = L < k ? 0 : L - k + 1;
    return n < kMaxWindows ? n : kMaxWindows;
}

// id(rc(w)) from id(w) over A = 4 with A, C, G, T = 0 .. 3: the k digits of v in reverse order, each complemented (3 - c)
BSQ_SKETCH_HD uint64_t rc_word(uint64_t v, int32_t k) {
    uint64_t r = 0;
    for (int32_t i = 0; i < k; ++i) {
        r = (r << 2) | (3u - (v & 3u));
        v >>= 2;
    }
    return r;
}

BSQ_SKETCH_HD uint64_t hash_of(uint64_t word, uint64_t salt) { return mix64(word ^ salt); }
BSQ_SKETCH_HD uint32_t bucket_of(uint64_t h, uint32_t S) { return static_cast<uint32_t>(((h >> 32) * S) >> 32); }
BSQ_SKETCH_HD uint32_t value_of(uint64_t h) {
    const uint32_t v = static_cast<uint32_t>(h);
    return v < 0xFFFFFFFEu ? v : 0xFFFFFFFEu;
}

// one output element from a table entry: BSQ_I32 the 32 bits as they are (EMPTY reads -1), BSQ_U64 the value as int64 bits, EMPTY as -1
template <typename T>
BSQ_SKETCH_HD T element(uint32_t v) {
    if constexpr (sizeof(T) == 8) return v == kEmpty ? ~T(0) : static_cast<T>(v);
    else return static_cast<T>(v);
}

// the word of the window w[0 .. k) and whether every character of it is mapped: the lexicographic Horner sum as an unsigned 64-bit value,
// min(id(w), id(rc(w))) when canonical.  The plain loop of the CPU twin; the kernels roll the same value.
template <typename Lut>
BSQ_SKETCH_HD bool window_word(const Geometry &g, const Lut &lut, const uint8_t *w, uint64_t *word) {
    uint64_t v = 0;
    for (int32_t i = 0; i < g.k; ++i) {
        const int32_t id = lut[w[i]];
        if (id < 0) return false;
        v = v * static_cast<uint64_t>(g.A) + static_cast<uint64_t>(id);
    }
    if (g.canonical) {
        const uint64_t r = rc_word(v, g.k);
        v = r < v ? r : v;
    }
    *word = v;
    return true;
}

// The kernel a call takes and its name (bsq_row_table.h): a pure predicate of (S, B, total_chars, form); Form::none: form = 1 cannot take this S.
using bsq_rowtab::Form;
using bsq_rowtab::kMaxRows;  // rows of a call: a row is a workgroup (or a wave) of one launch
inline Form form_of(int64_t S, int64_t B, int64_t total_chars, int32_t form) {
    return bsq_rowtab::form_of(S, B, total_chars, form, {kBlockChars, kManyRows, kBlockCharsMany});
}
constexpr const char *kFormNames[4] = {"k_minhash_wave", "k_minhash_block<1024>", "k_minhash_block<4096>", "k_minhash_block<16384>"};
inline const char *form_name(Form f) { return bsq_rowtab::form_name(f, kFormNames); }

// The argument rules that do not depend on a pointer to the batch: BSQ_OK and the geometry, or a status and a reason.  Host only.
inline bsq_status check(const bsq_desc *d, const bsq_minhash *m, int64_t B, bsq_dtype t, Geometry *g, const char **why) {
    if (!d || !m || B < 0) return *why = "null pointer or B < 0", BSQ_ERR_INVALID_ARG;
    if (B > kMaxRows) return *why = "B exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (m->k < 1 || m->k > kMaxK) return *why = "k must lie in 1 .. 32", BSQ_ERR_INVALID_ARG;
    if (d->nchars < 1) return *why = "the alphabet has no classes", BSQ_ERR_INVALID_ARG;
    // A^k <= 2^64 without a product that could overflow: A^(k-1) is built under a division guard, then compared with floor(2^64 / A)
    const uint64_t A = static_cast<uint64_t>(d->nchars), top = ~uint64_t(0);
    uint64_t lead = 1;
    for (int32_t i = 1; i < m->k; ++i) {
        if (lead > top / A) return *why = "nchars^k exceeds 2^64: a word no longer fits 64 bits", BSQ_ERR_INVALID_ARG;
        lead *= A;
    }
    if (A > 1 && lead > top / A + (top % A == A - 1 ? 1 : 0)) return *why = "nchars^k exceeds 2^64: a word no longer fits 64 bits", BSQ_ERR_INVALID_ARG;
    if (m->buckets < 1 || m->buckets > kMaxBuckets) return *why = "buckets must lie in 1 .. 2^14", BSQ_ERR_INVALID_ARG;
    if ((m->canonical | 1) != 1 || m->form < 0 || m->form > 2 || m->reserved != 0 || m->total_chars < 0)
        return *why = "canonical must be 0 / 1, form 0 .. 2, reserved 0 and total_chars >= 0", BSQ_ERR_INVALID_ARG;
    if (m->canonical && !bsq_rowtab::has_strands(d))
        return *why = "canonical needs the four classes A, C, G, T = 0, 1, 2, 3 (DNA, DNA4)", BSQ_ERR_INVALID_ARG;
    if (t != BSQ_I32 && t != BSQ_U64) return *why = "a sketch takes BSQ_I32 or BSQ_U64", BSQ_ERR_DTYPE;
    if (form_of(m->buckets, B, m->total_chars, m->form) == Form::none)
        return *why = "form = 1 (a wave per row) takes buckets <= 1024", BSQ_ERR_INVALID_ARG;
    g->lead = lead;
    g->mask = m->k == 32 ? top : (uint64_t(1) << (2 * m->k)) - 1;
    g->salt = mix64(m->seed ^ kDomain);
    g->k = m->k;
    g->A = d->nchars;
    g->S = m->buckets;
    g->canonical = m->canonical;
    return BSQ_OK;
}

// The comparison's rules: BSQ_OK, or a status and a reason.  Host only.
constexpr int kCmpTile = 64;  // rows of a and rows of b of one workgroup's output tile
inline bsq_status check_compare(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const int32_t *match, const char **why) {
    if (Ba < 0 || Bb < 0) return *why = "negative row count", BSQ_ERR_INVALID_ARG;
    if (S < 1 || S > kMaxBuckets) return *why = "S must lie in 1 .. 2^14", BSQ_ERR_INVALID_ARG;
    if (t != BSQ_I32 && t != BSQ_U64) return *why = "sketches are BSQ_I32 or BSQ_U64", BSQ_ERR_DTYPE;
    if (Ba > kMaxRows || Bb > kMaxRows || ((Ba + kCmpTile - 1) / kCmpTile) * ((Bb + kCmpTile - 1) / kCmpTile) > kMaxRows)
        return *why = "too many rows: the 64 x 64 tiles of the (Ba, Bb) output must number at most 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (Ba > 0 && Bb > 0 && (!a || !b || !match)) return *why = "a, b or match is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

// ---- sketch pairs (include/bsq.h, "sketch pairs"): the selection, the segments and the argument rules ----
constexpr int32_t kMaxSegments = 64;  // segments of the j tiles a strip of 64 rows of `a` is cut into
constexpr int32_t kQ16 = 65536;       // jaccard_q16 = 65536: match == either
// Workgroups (strip, segment) a call aims for when the library chooses the segments.  k_sketch_pairs takes ~250 VGPRs and 18.5 KB of LDS:
// two workgroups per CU, 512 on an MI355X at once, so 4096 is eight rounds of that.  scripts/sketch_pairs_lab.py on an MI355X, the count
// call, cross, int32 (profiles/r20/sketch_pairs_lab.txt; us, * the choice):
//     8192 x 8192 x 1024 (128 strips)   segments 1: 23110   2: 12053   4: 7012   8: 6934   16: 6721   32*: 6567   64: 6303
//     4096 x 4096 x 128  (64 strips)    segments 1: 1259    2: 606     4: 307    8: 210    16: 212    32: 215     64*: 227
//     262144 x 262144 x 128, upper (4096 strips)   segments 1*: 415 ms   2: 616 ms
// Wide sketches would take still more workgroups and narrow ones fewer; either choice is within 8 % of the best of its row, and once
// the strips alone reach the target a second segment costs half as much again.
constexpr int64_t kPairsGroups = 4096;

// pass(i, j): both products are at most 2^30, so the 32-bit arithmetic is exact
BSQ_SKETCH_HD bool pair_passes(int32_t match, int32_t either, int32_t min_match, int32_t jaccard_q16) {
    return match >= min_match && match * kQ16 >= jaccard_q16 * either;
}

// A checked bsq_sketch_pairs and the geometry of its call (made on the host)
struct PairsRule {
    int32_t min_match, jaccard_q16, upper;
    int32_t nseg;      // segments of a strip: 1 .. min(64, tiles_j)
    int64_t tiles_j;   // 64-row tiles of b
    int64_t strips;    // 64-row strips of a
};

// the j tiles [first, last) of segment `seg` of `nseg`: consecutive, every segment at least one tile (nseg <= tiles_j)
BSQ_SKETCH_HD int64_t segment_first_tile(int64_t seg, int64_t nseg, int64_t tiles_j) { return seg * tiles_j / nseg; }

// segments of a call: `segments` > 0 forces min(segments, tiles_j); 0: enough that strips * nseg reaches kPairsGroups, 1 once the strips
// alone do, never more than 64 or the number of j tiles.  An empty side gives 1.
inline int32_t pairs_segments(int64_t Ba, int64_t Bb, int32_t segments) {
    const int64_t strips = (Ba + kCmpTile - 1) / kCmpTile, tiles_j = (Bb + kCmpTile - 1) / kCmpTile;
    if (strips == 0 || tiles_j == 0) return 1;
    int64_t n = segments > 0 ? segments : (kPairsGroups + strips - 1) / strips;
    if (n > kMaxSegments) n = kMaxSegments;
    if (n > tiles_j) n = tiles_j;
    return static_cast<int32_t>(n);
}

// The rules both calls and the CPU twin share: BSQ_OK and the checked rule, or a status and a reason.  Host only.
inline bsq_status check_pairs(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                              PairsRule *r, const char **why) {
    if (!rule) return *why = "the rule is null", BSQ_ERR_INVALID_ARG;
    const bsq_status st = check_compare(a, Ba, b, Bb, S, t, &rule->min_match, why);  // (the outputs are the caller's to check)
    if (st != BSQ_OK) return st;
    if (rule->min_match < 0 || rule->min_match > S) return *why = "min_match must lie in 0 .. S", BSQ_ERR_INVALID_ARG;
    if (rule->jaccard_q16 < 0 || rule->jaccard_q16 > kQ16) return *why = "jaccard_q16 must lie in 0 .. 65536", BSQ_ERR_INVALID_ARG;
    if ((rule->upper | 1) != 1) return *why = "upper must be 0 / 1", BSQ_ERR_INVALID_ARG;
    if (rule->upper && Ba != Bb) return *why = "upper lists the pairs i < j of ONE matrix: Ba must equal Bb", BSQ_ERR_INVALID_ARG;
    if (rule->segments < 0 || rule->segments > kMaxSegments) return *why = "segments must lie in 0 .. 64", BSQ_ERR_INVALID_ARG;
    r->min_match = rule->min_match;
    r->jaccard_q16 = rule->jaccard_q16;
    r->upper = rule->upper;
    r->nseg = pairs_segments(Ba, Bb, rule->segments);
    r->tiles_j = (Bb + kCmpTile - 1) / kCmpTile;
    r->strips = (Ba + kCmpTile - 1) / kCmpTile;
    return BSQ_OK;
}

// ---- sketch clusters (include/bsq.h, "sketch clusters"): the union-find, the edge rule and the argument rules ----
// One text of find and union over a `parent` array reached through an accessor P: load(x), store(x, v) and swap_root(hi, lo), which
// sets parent[hi] from hi to lo and says whether it did.  The kernels pass accessors made of agent-scope atomics on global memory
// and of workgroup-scope atomics on LDS (bsq_sketch.hip), the CPU twins the plain SeqParent below.  The invariant is parent[x] <= x:
// a root is hooked under a SMALLER root only, and only while it is a root (the swap expects parent[hi] == hi), so there is no cycle
// and the last root of a component is its smallest member, in whatever order the unions arrive.  A node that has left the roots never
// returns to them: path halving (HALVE) may store any ancestor over its parent, a stale one included, and the swap on it fails
// either way.  Nothing here waits: a failed swap means that another union has just succeeded on that root.
template <bool HALVE, typename P>
BSQ_SKETCH_HD int64_t uf_find(const P &m, int64_t x) {
    int64_t p = m.load(x);
    while (p != x) {
        const int64_t g = m.load(p);
        if (HALVE && g != p) m.store(x, g);
        x = p;
        p = g;
    }
    return x;
}

template <typename P>
BSQ_SKETCH_HD void uf_union(const P &m, int64_t a, int64_t b) {
    for (;;) {
        a = uf_find<true>(m, a);
        b = uf_find<true>(m, b);
        if (a == b) return;
        const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
        if (m.swap_root(hi, lo)) return;
        a = lo;  // (hi has just been hooked elsewhere: again, from where this attempt stood)
        b = hi;
    }
}

// the accessor of the CPU twins: one thread, so the swap always finds what find left
struct SeqParent {
    int64_t *p;
    int64_t load(int64_t x) const { return p[x]; }
    void store(int64_t x, int64_t v) const { p[x] = v; }
    bool swap_root(int64_t hi, int64_t lo) const { return p[hi] = lo, true; }
};

// an entry of an explicit edge list links two nodes: not a self-edge, both ends inside 0 .. n - 1 (anything else is ignored unread)
BSQ_SKETCH_HD bool edge_links(int64_t row, int64_t col, int64_t n) {
    return row != col && static_cast<uint64_t>(row) < static_cast<uint64_t>(n) && static_cast<uint64_t>(col) < static_cast<uint64_t>(n);
}

// The rules of the clustering calls: the pair list's, on one matrix, with upper == 1.  Host only.
inline bsq_status check_clusters(const void *a, int64_t B, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule, PairsRule *r, const char **why) {
    const bsq_status st = check_pairs(a, B, a, B, S, t, rule, r, why);
    if (st != BSQ_OK) return st;
    if (rule->upper != 1) return *why = "sketch clusters take a rule with upper == 1: the links i < j of ONE matrix", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

inline bsq_status check_cluster_pairs(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, const char **why) {
    if (n_pairs < 0 || n < 0) return *why = "negative n_pairs or n", BSQ_ERR_INVALID_ARG;
    if (n > kMaxRows) return *why = "n exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && (!row || !col)) return *why = "row or col is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

}  // namespace bsq_sketchd
