// Shared by the kernel families that walk the table of a listed pair of rows: the edit distance (bsq_edit.hip), the scored alignment
// (bsq_score.hip) and the alignment statistics (bsq_align_stats.hip), and by their CPU twins; gfx950 only on the device side.  Each family
// keeps its parameter block, its cell or block step, what a lane keeps in registers, what it exchanges per step, its result write, its
// argument rules' own messages and its __global__ entry points; the way from a pair list to a walk is here, once:
//   G = 4, 16 or 64 lanes per pair; a wave holds 64 / G pairs and a workgroup four waves that never meet after the tables are staged.
//   The shorter row of a pair is the pattern (A's when the lengths are equal), the longer the text; lane b of the pair's group owns the
//   pattern's rows ROWS b + 1 .. ROWS b + ROWS.  The group walks the anti-diagonals of the (lane, column) grid: at step t lane b takes
//   text column t - b, so a group runs n + lanes with rows - 1 steps and a wave runs until its slowest group is done (wave_max); a lane
//   outside its columns keeps its state.  The text is fetched G characters at a time, a byte per lane, one tile ahead of its use, and
//   mapped to classes once (TextTile); lane 0 of the group takes the class of column t from lane t % G of the tile, in the cross-lane
//   read that also moves the column's class up one lane.  No lane issues a global load that the step waits for, none reads a character
//   twice.  No global atomic, no waiting on other waves.
//   A pair that walks nothing -- an index outside its store (never dereferenced), a side beyond the limits, an empty side -- is written
//   by lane 0 of its group before the walk, in the family's own codes (Kind).
// The scaffold is a template on a family's parameter block (chars_a .. n_pairs, max_len, nchars, lut and matrix are read from it), never an
// embedded common struct: the blocks keep their member order, which with -amdgpu-kernarg-preload-count=14 is part of the tuning
// (bsq_row_table.h).
// Measured against the parent on an MI355X (profiles/r28/pair_walk_lab.txt): k_align_stats is on all of this and no slower; k_edit_pairs
// and k_score_pairs keep the text tile, and the score the class packing, written out in their kernels -- with TextTile and pack_classes
// their step loops compiled to other instruction forms and ran 1.5 - 4 % slower.  Those two helpers have one user until that is solved.
// The plain C++ part (limits, class_of, resolve, lanes_of, check_pairs, fill) needs <cstdint> and bsq.h alone: the CPU twins compile it
// without HIP.
#pragma once
#include <cstdint>

#include "bsq.h"

#if defined(__HIPCC__)
#define BSQ_EDIT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BSQ_EDIT_HD inline
#endif

namespace bsq_pairs {

constexpr int64_t kMaxPairs = (int64_t(1) << 31) - 1;  // pairs of a call: at least four of them per workgroup of one launch
constexpr int64_t kMaxRows = (int64_t(1) << 31) - 1;   // rows of a store
// classes of an alphabet, the unmapped one included (every alphabet of the package but BYTES): the edit kernel's four tables of classes x
// 64 words and the byte table fit the 64 KiB of LDS a workgroup gets without asking; index 31 of a staged score matrix is free
constexpr int32_t kMaxClasses = 31;

// the class of a byte: its id, or nchars for every byte the alphabet does not map
template <typename Lut>
BSQ_EDIT_HD uint32_t class_of(const Lut &lut, int32_t nchars, uint8_t byte) {
    const int32_t id = lut[byte];
    return static_cast<uint32_t>(id >= 0 ? id : nchars);
}

enum class Kind { none, bad_index, too_long, empty, live };  // none: no pair (a group behind the list's end)

// what resolve() fills for an empty or live pair; the pattern as (pat, pat_at, pat_total) for bsq_rowtab::load16
struct Pair {
    const uint8_t *pat = nullptr, *text = nullptr;  // the pattern's store, the text's first character
    int64_t pat_at = 0, pat_total = 0;              // the pattern's first character in its store, the store's characters
    uint32_t m = 0, n = 0;                          // characters of the pattern and of the text
    bool a_short = true;                            // the pattern is A's row
    BSQ_EDIT_HD int32_t la() const { return static_cast<int32_t>(a_short ? m : n); }
    BSQ_EDIT_HD int32_t lb() const { return static_cast<int32_t>(a_short ? n : m); }
};

// The pair (row i of A, row j of B): the index check, the lengths as read from the offsets (a negative one counts as 0), the shorter row
// as the pattern, the limits on the two sides.
BSQ_EDIT_HD Kind resolve(const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b, const int64_t *offsets_b, int64_t Bb,
                         int64_t i, int64_t j, int64_t max_len, int64_t max_long, Pair &q) {
    if (i < 0 || i >= Ba || j < 0 || j >= Bb) return Kind::bad_index;
    const int64_t sa = offsets_a[i], sb = offsets_b[j];
    int64_t la = offsets_a[i + 1] - sa, lb = offsets_b[j + 1] - sb;
    la = la < 0 ? 0 : la;
    lb = lb < 0 ? 0 : lb;
    q.a_short = la <= lb;
    const int64_t m = q.a_short ? la : lb, n = q.a_short ? lb : la;
    if (m > max_len || n > max_long) return Kind::too_long;
    q.m = static_cast<uint32_t>(m), q.n = static_cast<uint32_t>(n);
    q.pat = q.a_short ? chars_a : chars_b;
    q.pat_at = q.a_short ? sa : sb;
    q.pat_total = q.a_short ? offsets_a[Ba] : offsets_b[Bb];
    q.text = q.a_short ? chars_b + sb : chars_a + sa;
    return m == 0 ? Kind::empty : Kind::live;
}

// lanes per pair of the kernel a call takes (4, 16 or 64: the smallest that holds max_len at `rows` pattern rows a lane unless `form`
// 1 .. 3 names one), 0 for a max_len outside 1 .. cap_len or a form that cannot hold it
inline int32_t lanes_of(int32_t max_len, int32_t form, int32_t rows, int32_t cap_len) {
    if (max_len < 1 || max_len > cap_len || form < 0 || form > 3) return 0;
    const int32_t least = max_len <= 4 * rows ? 1 : (max_len <= 16 * rows ? 2 : 3);
    if (form != 0 && form < least) return 0;
    return 1 << (2 * (form != 0 ? form : least));
}
// 0, 1, 2 for 4, 16, 64 lanes (a family's table of kernel names), -1 otherwise
inline int lanes_index(int32_t lanes) { return lanes == 4 ? 0 : (lanes == 16 ? 1 : (lanes == 64 ? 2 : -1)); }

// The argument rules of a family's device call and CPU twin: BSQ_OK, or a status and a reason.  refused: the family's reason when its
// rule struct does not pass, else null; null_out: its reason when row, col or one of its outputs is null, else null.  Host only.
inline bsq_status check_pairs(const bsq_desc *d, const void *chars_a, const void *offsets_a, int64_t Ba, const void *chars_b, const void *offsets_b,
                              int64_t Bb, int64_t n_pairs, const char *refused, const char *null_out, const char **why) {
    if (!d) return *why = "the descriptor is null", BSQ_ERR_INVALID_ARG;
    if (d->nchars < 1 || d->nchars + 1 > kMaxClasses) return *why = "the alphabet must have 1 .. 30 classes (BYTES has 256)", BSQ_ERR_INVALID_ARG;
    if (refused) return *why = refused, BSQ_ERR_INVALID_ARG;
    if (Ba < 0 || Bb < 0 || n_pairs < 0) return *why = "negative Ba, Bb or n_pairs", BSQ_ERR_INVALID_ARG;
    if (Ba > kMaxRows || Bb > kMaxRows || n_pairs > kMaxPairs) return *why = "Ba, Bb or n_pairs exceeds 2^31 - 1", BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && null_out) return *why = null_out, BSQ_ERR_INVALID_ARG;
    if (n_pairs > 0 && ((Ba > 0 && (!chars_a || !offsets_a)) || (Bb > 0 && (!chars_b || !offsets_b))))
        return *why = "chars or offsets of a store with rows is null", BSQ_ERR_INVALID_ARG;
    return BSQ_OK;
}

// the members every family's parameter block has, from the arguments of its entry point; fill_scores: those of the two that score
template <typename P>
void fill(P &p, const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b, const int64_t *offsets_b,
          int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, int32_t max_len) {
    p.chars_a = chars_a, p.chars_b = chars_b, p.offsets_a = offsets_a, p.offsets_b = offsets_b;
    p.row = row, p.col = col;
    p.Ba = Ba, p.Bb = Bb, p.n_pairs = n_pairs;
    p.max_len = max_len, p.nchars = d->nchars;
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
}
template <typename P>
void fill_scores(P &p, const bsq_score *sc) {
    p.gap_open = sc->gap_open, p.gap_extend = sc->gap_extend;
    for (int r = 0; r < 32; ++r)  // (bsq_score::matrix is 32 x 32)
        for (int c = 0; c < 32; ++c) p.matrix[r][c] = sc->matrix[r][c];
}

}  // namespace bsq_pairs

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bsq_device.h"
#include "bsq_row_table.h"

namespace bsq_pairs {

using bsq_dev::kThreads;

// the pair of this lane's group
template <int G>
__device__ __forceinline__ int64_t pair_index() {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    return (static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave) * (64 / G) + lane / G;
}

template <typename P>
__device__ __forceinline__ Kind resolve(const P &p, int64_t k, int64_t max_long, Pair &q) {
    if (k >= p.n_pairs) return Kind::none;
    return resolve(p.chars_a, p.offsets_a, p.Ba, p.chars_b, p.offsets_b, p.Bb, p.row[k], p.col[k], p.max_len, max_long, q);
}

// the steps of the wave's slowest group, wave-uniform.  (A wave that gets 0 returns: no workgroup barrier may follow.)
__device__ __forceinline__ uint32_t wave_max(uint32_t steps) {
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const uint32_t o = __shfl_xor(steps, x);
        steps = o > steps ? o : steps;
    }
    return __builtin_amdgcn_readfirstlane(steps);
}

// A text tile: column T + b of the tile that starts at T, as a byte ahead of its use and as a class (`tile`) while in use.
template <int G>
struct TextTile {
    const uint8_t *text;
    uint32_t n, ahead, tile;
    // n: the text's characters, 0 for a lane whose group walks nothing
    __device__ __forceinline__ TextTile(const uint8_t *text_, uint32_t n_, int b) : text(text_), n(n_), ahead(fetch(b)), tile(0) {}
    __device__ __forceinline__ uint32_t fetch(uint32_t at) const { return at < n ? text[at] : 0u; }
    // before step t of every lane: every G steps the byte fetched a tile ago becomes the class in use and the next one is asked for
    __device__ __forceinline__ void step(uint32_t t, int b, const uint8_t *s_cls) {
        if ((t & (G - 1)) == 0) {  // (uniform)
            tile = s_cls[ahead];
            ahead = fetch(t + G + b);
        }
    }
};

// s_cls[byte] = the byte's class, by the workgroup's 256 threads; the caller's __syncthreads() follows
template <typename P>
__device__ __forceinline__ void stage_classes(const P &p, uint8_t *s_cls) {
    s_cls[threadIdx.x] = static_cast<uint8_t>(class_of(p.lut, p.nchars, static_cast<uint8_t>(threadIdx.x)));  // (kThreads == 256)
}

// p.matrix in both orientations, DIM x DIM each, read as [column class][row class]: s_mat[0] is [B's class][A's class] for a pattern from
// A, s_mat[1] is [A's class][B's class]; `pad` wherever an index is no class of the alphabet.  The caller's __syncthreads() follows.
template <int DIM, typename P>
__device__ __forceinline__ void stage_matrix(const P &p, int8_t *s_mat, int32_t pad) {
    for (unsigned q = threadIdx.x; q < DIM * DIM; q += kThreads) {
        const int c = static_cast<int>(q / DIM), r = static_cast<int>(q % DIM);
        const bool real = c <= p.nchars && r <= p.nchars;
        s_mat[q] = real ? p.matrix[r][c] : static_cast<int8_t>(pad);
        s_mat[DIM * DIM + q] = real ? p.matrix[c][r] : static_cast<int8_t>(pad);
    }
}

// the classes of lane b's ROWS pattern rows, four to a word; behind the `mine` rows that exist the class `pad`
template <int ROWS>
__device__ __forceinline__ void pack_classes(const Pair &q, int b, int32_t mine, const uint8_t *s_cls, uint32_t pad, uint32_t (&pc)[ROWS / 4]) {
#pragma unroll
    for (int g = 0; g < ROWS / 16; ++g) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (16 * g < mine) bsq_rowtab::load16(q.pat, q.pat_at + ROWS * b + 16 * g, q.pat_total, mine - 16 * g, w);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t packed = 0;
#pragma unroll
            for (int z = 0; z < 4; ++z) {
                const int r = 16 * g + 4 * c + z;
                const uint32_t cls = r < mine ? s_cls[(w[c] >> (8 * z)) & 0xFFu] : pad;
                packed |= cls << (8 * z);
            }
            pc[4 * g + c] = packed;
        }
    }
}

// f(std::integral_constant<int, G>) for the G of `lanes` (4, 16, else 64)
template <typename F>
void for_lanes(int32_t lanes, F f) {
    if (lanes == 4) f(std::integral_constant<int, 4>{});
    else if (lanes == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}

// the launch of a family's kernel of G lanes per pair: four waves of 64 / G pairs per workgroup; n_pairs <= kMaxPairs fits the grid
template <int G, typename P>
void launch(void (*kernel)(P), const P &p, size_t lds, hipStream_t s) {
    constexpr int64_t per_group = (kThreads / 64) * (64 / G);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((p.n_pairs + per_group - 1) / per_group)), dim3(kThreads), lds, s, p);
}

}  // namespace bsq_pairs
#endif
