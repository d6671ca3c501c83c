// MinHash sketches of a packed batch and the all-pairs comparison of sketches on the device (gfx950): include/bsq.h ("MinHash sketch")
// documents the rule, bsq_sketch_dev.h holds what the kernels and the CPU twins (bsq_sketch_host.cpp) share.  The sketch kernels are per-row
// reductions over the scaffold of bsq_row_table.h (the table in LDS, its fill, the two forms, the row store, the launch), as the spectrum's
// are (bsq_kmer_spectrum.hip), with `min` in place of `add` over a wide rolling word in place of a dense id: a table of S u32 buckets,
// filled with EMPTY, updated with LDS atomics (ds_min_u32, no return value); nothing is counted per row.
//
// k_minhash_wave<T, MODE>         row_table_wave: S <= 1024, a wave per row.
// k_minhash_block<T, BINS, MODE>  row_table_block<BINS>: a workgroup per row, long rows and every S above 1024.
// Both sweep a row in pieces of (lanes x 16) windows: a lane takes 16 consecutive windows, 16 + k - 1 <= 47 characters from three 16-byte
// loads -- the 16 that start a window, the next 16 (the warm-up of k > 17 only) and, k - 1 further than the first, the 16 that end one --
// so that every register index is static.  MODE 0: any alphabet, the word rolls by a multiplication; 1: four classes, the word rolls by
// a shift and a mask; 2: canonical, a second word rolls the reverse complement in from the top.
// Loads are 16 bytes wide where they end at or before offsets[B], byte by byte behind that bound otherwise.
//
// k_sketch_compare<T>   a workgroup per 64 x 64 tile of the (Ba, Bb) outputs, tiles linearised in blockIdx.x; 64 rows of a and of b go
//            through LDS in chunks of 32 buckets (bucket-major, so that a thread's four rows of a side are one 16-byte read), a thread
//            keeps a 4 x 4 register tile of equal-bucket counts and one of both-EMPTY counts (from a 32-bit EMPTY mask per row and chunk:
//            a popcount per pair and chunk), which give `match` and `either`.  An input element is read once per tile pair.
// k_sketch_pairs<T, EMIT>   the thresholded pair list (include/bsq.h, "sketch pairs"): the same tile arithmetic (cmp_tile) by a workgroup per
//            (strip of 64 rows, segment of j tiles), with a ragged, ordered output; its comment stands in front of it.
// k_cluster_init, k_sketch_link<T>, k_cluster_link_pairs, k_cluster_labels   the clusters (include/bsq.h, "sketch clusters"): the same
//            walk of upper tiles, every passing pair a union in a lock-free union-find; their comment stands in front of them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_kmer_lane.h"
#include "bsq_ragged_out.h"
#include "bsq_row_table.h"
#include "bsq_sketch_dev.h"

namespace {

// (kThreads = 256 is bsq_ragged_out.h's, which also has a Form of its own: the row table's is named in full)
using bsq_kmerd::byte_of;
using bsq_rowtab::load16;
using bsq_sketchd::Geometry;
using bsq_sketchd::kEmpty;
using bsq_sketchd::PairsRule;
static_assert(kThreads == bsq_dev::kThreads, "one workgroup size");

constexpr int kRun = 16;  // windows of a lane's run
struct SketchParams {
    const uint8_t *chars;
    const int64_t *offsets;
    void *out;
    int64_t B;
    uint64_t lead, mask, salt;
    int32_t S, k, A;
    int8_t lut[256];
};

// The rolling words of a lane: fw the Horner sum of the last k characters, rc (MODE 2) that of their reverse complement, run the mapped
// characters in a row up to the current one (a window is whole from run >= k on).  An unmapped character enters as digit 0.
template <int MODE>
struct Roll {
    uint64_t fw = 0, rc = 0;
    int32_t run = 0;
    // `gone`: the digit that leaves the window (MODE 0 beyond the warm-up; 0 before)
    __device__ __forceinline__ void push(const SketchParams &p, int32_t id, uint32_t gone, int32_t rshift) {
        const uint64_t dgt = static_cast<uint64_t>(id < 0 ? 0 : id);
        if constexpr (MODE == 0) {
            fw = (fw - gone * p.lead) * static_cast<uint32_t>(p.A) + dgt;
        } else {
            fw = ((fw << 2) | dgt) & p.mask;
            if constexpr (MODE == 2) rc = (rc >> 2) | ((3u - dgt) << rshift);
        }
        run = id < 0 ? 0 : run + 1;
    }
    __device__ __forceinline__ uint64_t word() const {
        if constexpr (MODE == 2) return rc < fw ? rc : fw;
        else return fw;
    }
};

// The windows [0, n) of the row at `start` into `tab`, by NL lanes (lane: 0 .. NL - 1)
template <int MODE, int NL>
__device__ __forceinline__ void sweep(const SketchParams &p, const int8_t *s_lut, uint32_t *tab, int64_t start, int64_t total, int32_t n, int lane) {
    const int32_t k = p.k, km1 = k - 1, rshift = 2 * km1;
    const uint32_t S = static_cast<uint32_t>(p.S);
    for (int32_t j0 = lane * kRun; j0 < n; j0 += NL * kRun) {
        // W0: the characters j0 .. j0 + 15 (each starts a window of the run), W1: j0 + 16 .. j0 + 31 (the warm-up reaches them when k > 17),
        // M: j0 + k - 1 .. j0 + k + 14 (each ends one); a character behind the row's last window belongs to no sketched window
        const int32_t chars_left = n + km1 - j0;  // characters of the row's windows from j0 on (> km1)
        uint32_t W0[4], W1[4] = {0, 0, 0, 0}, M[4];
        load16(p.chars, start + j0, total, chars_left, W0);
        if (km1 > 16) load16(p.chars, start + j0 + 16, total, chars_left - 16, W1);  // (uniform)
        load16(p.chars, start + j0 + km1, total, chars_left - km1, M);
        Roll<MODE> r;
#pragma unroll
        for (int c = 0; c < bsq_sketchd::kMaxK - 1; ++c) {
            if (c < km1) {  // (uniform)
                const uint32_t byte = c < 16 ? byte_of(W0, c & 15) : byte_of(W1, c & 15);
                r.push(p, s_lut[byte], 0u, rshift);
            }
        }
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
            uint32_t gone = 0;
            if constexpr (MODE == 0) {
                if (q > 0) {  // the character that leaves the window
                    const int32_t g = s_lut[byte_of(W0, q > 0 ? q - 1 : 0)];
                    gone = static_cast<uint32_t>(g < 0 ? 0 : g);
                }
            }
            r.push(p, s_lut[byte_of(M, q)], gone, rshift);
            if (r.run >= k && j0 + q < n) {
                const uint64_t h = bsq_sketchd::hash_of(r.word(), p.salt);
                atomicMin(tab + bsq_sketchd::bucket_of(h, S), bsq_sketchd::value_of(h));
            }
        }
    }
}

// A row through the scaffold (bsq_row_table.h): BINS = 0 the wave form, else the block form of that many buckets.  Nothing is counted.
template <typename T, int BINS, int MODE>
__device__ __forceinline__ void minhash_row(const SketchParams &p) {
    __shared__ int8_t s_lut[256];
    constexpr int NL = BINS ? kThreads : 64;
    const auto windows = [k = p.k](int64_t L) { return static_cast<int32_t>(bsq_sketchd::row_windows(L, k)); };
    const auto sweep_row = [=](uint32_t *tab, int64_t start, int64_t total, int32_t n, int lane) {
        sweep<MODE, NL>(p, s_lut, tab, start, total, n, lane);
        return 0u;
    };
    const auto finish = [](uint32_t) { return [](uint32_t v) { return bsq_sketchd::element<T>(v); }; };
    if constexpr (BINS == 0) bsq_rowtab::row_table_wave<T, false>(p, p.S, kEmpty, s_lut, windows, sweep_row, finish);
    else bsq_rowtab::row_table_block<T, BINS>(p, p.S, kEmpty, s_lut, windows, sweep_row, finish);
}

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void k_minhash_wave(const SketchParams p) {
    minhash_row<T, 0, MODE>(p);
}

template <typename T, int BINS, int MODE>
__global__ __launch_bounds__(kThreads) void k_minhash_block(const SketchParams p) {
    minhash_row<T, BINS, MODE>(p);
}

// ---- the comparison ----
constexpr int kTile = bsq_sketchd::kCmpTile;  // 64 rows of a x 64 rows of b per workgroup
constexpr int kChunkS = 32;                   // buckets staged at a time
// The staged image is [bucket][row], a bucket's 64 rows 68 dwords apart, row r at (r & 15) * 4 + (r >> 4): the four rows ty + 16 r of a
// thread (tx + 16 c on the b side) are one aligned 16-byte read, the sixteen such reads of a wave's b side cover one 256-byte bank row,
// and the 32 buckets of a row a staging wave writes fall on eight banks (pitch 68 = 4 mod 32) instead of one.
constexpr int kPitch = kTile + 4;
__device__ __forceinline__ int cmp_slot(int row) { return (row & 15) * 4 + (row >> 4); }

// The tile (i0, j0) by the whole workgroup, what k_sketch_compare and k_sketch_pairs share: the staging and the 4 x 4 register tile.
// eq counts the buckets in which the two rows hold the same 32 bits, both the two rows' EMPTY ones among them (and the padding, which
// is EMPTY on both sides); both counts those: match = eq - both, either = buckets staged - both.  Returns the buckets staged.  Thread
// (tx, ty) holds rows i0 + ty + 16 r against rows j0 + tx + 16 c; the last barrier of the call stands behind every read of the stage.
template <typename T>
__device__ __forceinline__ int32_t cmp_tile(const T *a, int64_t Ba, const T *b, int64_t Bb, int32_t S, int64_t i0, int64_t j0,
                                            int32_t (&eq)[4][4], int32_t (&both)[4][4]) {
    __shared__ __align__(16) uint32_t s_a[kChunkS * kPitch], s_b[kChunkS * kPitch];
    __shared__ uint32_t s_ea[kTile], s_eb[kTile];  // bit t: the row's bucket t of the chunk is EMPTY
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) eq[r][c] = both[r][c] = 0;
    int32_t staged = 0;
    for (int32_t t0 = 0; t0 < S; t0 += kChunkS, staged += kChunkS) {
        // stage: 64 rows x 32 buckets of each side, the low 32 bits of an element; EMPTY outside the matrices
#pragma unroll
        for (int s = 0; s < kTile * kChunkS / kThreads; ++s) {
            const int el = tid + s * kThreads, row = el / kChunkS, col = el % kChunkS;  // (a wave: two whole rows)
            const bool in = t0 + col < S;
            const uint32_t va = in && i0 + row < Ba ? static_cast<uint32_t>(a[(i0 + row) * S + t0 + col]) : kEmpty;
            const uint32_t vb = in && j0 + row < Bb ? static_cast<uint32_t>(b[(j0 + row) * S + t0 + col]) : kEmpty;
            s_a[col * kPitch + cmp_slot(row)] = va;
            s_b[col * kPitch + cmp_slot(row)] = vb;
            const uint64_t ea = __ballot(va == kEmpty), eb = __ballot(vb == kEmpty);
            if (col == 0) {
                const bool high = (tid & 32) != 0;
                s_ea[row] = static_cast<uint32_t>(high ? ea >> 32 : ea);
                s_eb[row] = static_cast<uint32_t>(high ? eb >> 32 : eb);
            }
        }
        __syncthreads();
        {
            uint32_t ma[4], mb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ma[r] = s_ea[ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) mb[c] = s_eb[tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) both[r][c] += __popc(ma[r] & mb[c]);
        }
#pragma unroll 4
        for (int t = 0; t < kChunkS; ++t) {
            const uint4 a4 = *reinterpret_cast<const uint4 *>(s_a + t * kPitch + ty * 4);
            const uint4 b4 = *reinterpret_cast<const uint4 *>(s_b + t * kPitch + tx * 4);
            const uint32_t va[4] = {a4.x, a4.y, a4.z, a4.w}, vb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) eq[r][c] += va[r] == vb[c];
        }
        __syncthreads();
    }
    return staged;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sketch_compare(const T *a, int64_t Ba, const T *b, int64_t Bb, int32_t S, uint32_t tiles_j,
                                                             int32_t *match, int32_t *either) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t ti = blockIdx.x / tiles_j, tj = blockIdx.x - ti * tiles_j;
    const int64_t i0 = static_cast<int64_t>(ti) * kTile, j0 = static_cast<int64_t>(tj) * kTile;
    int32_t eq[4][4], both[4][4];
    const int32_t staged = cmp_tile(a, Ba, b, Bb, S, i0, j0, eq, both);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t j = j0 + tx + 16 * c;
            if (i < Ba && j < Bb) {
                match[i * Bb + j] = eq[r][c] - both[r][c];
                if (either) either[i * Bb + j] = staged - both[r][c];
            }
        }
    }
}

// ---- the pair list (include/bsq.h, "sketch pairs") ----
// k_sketch_pairs<T, EMIT>   a workgroup per (strip of 64 rows of a, segment of consecutive j tiles): it walks its tiles in ascending j
//            with cmp_tile and, after each, ORs its 16 pass flags into a 64-bit hit mask per row in LDS (two words, LDS atomics).  The rank
//            of column c inside its row is the row's running cursor (LDS) + popc(mask below c): no global atomic decides a rank, so the
//            order is (i, j).  EMIT = false: the per-(row, segment) counts -> seg_offsets[1 + row * nseg + segment].  EMIT = true: the
//            cursor starts at seg_offsets[row * nseg + segment], the scanned start, and every passing pair of rank < max_pairs is stored.
//            upper: tiles left of the strip's diagonal tile are skipped, the diagonal tile keeps j > i.
// The counts of the n = Ba * nseg (row, segment) entries become starts in place by the scaffold of bsq_ragged_out.h, whose offsets array
// seg_offsets is (entry k + 1: the length of k, then its end), so that entry row * nseg + segment is where that (row, segment) starts and
// the (i, segment, j) order is the (i, j) order:
// k_sketch_pairs_sums       the sums of every 64 counts -> the stream's scratch (lengths_step);
// k_sketch_pairs_scan       beyond 2^20 entries: those sums scanned once by one workgroup (scan_inclusive_block);
// k_sketch_pairs_place<SCANNED>   counts -> ends in place, a workgroup per 64 entries (place_offsets), seg_offsets[0] <- 0, and
//            pair_offsets[i] <- entry i * nseg, the one in front of row i (i <= Ba: the last is the total), by the thread that wrote it.
// One workgroup scanning all n entries (scan_inclusive_block on seg_offsets itself) took 360 us at n = 262 144, more than the count of
// 4096 x 4096 x 128 itself (profiles/r20/sketch_pairs_lab.txt): hence the split.
struct PairsOut {
    int64_t *row, *col;
    int32_t *match, *either;
    int64_t max_pairs;
};

template <typename T, bool EMIT>
__global__ __launch_bounds__(kThreads) void k_sketch_pairs(const T *a, int64_t Ba, const T *b, int64_t Bb, int32_t S, const PairsRule r,
                                                           int64_t *seg_offsets, const PairsOut out) {
    __shared__ uint32_t s_hit[kTile][2];  // bit c of a row: column j0 + c of the tile passes
    __shared__ int64_t s_cur[kTile];      // the pairs of a row in front of the tile: from the segment's first tile (count), of all (emit)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t nseg = static_cast<uint32_t>(r.nseg), strip = blockIdx.x / nseg, seg = blockIdx.x - strip * nseg;
    const int64_t i0 = static_cast<int64_t>(strip) * kTile;
    int64_t tj = bsq_sketchd::segment_first_tile(seg, nseg, r.tiles_j);
    const int64_t tj_end = bsq_sketchd::segment_first_tile(seg + 1, nseg, r.tiles_j);
    if (r.upper && tj < strip) tj = strip;
    if constexpr (EMIT) {  // ranks grow with (row, segment): where the first row's start is cut, every pair of the workgroup is (uniform)
        if (seg_offsets[i0 * nseg + seg] >= out.max_pairs) return;
    }
    if (tid < kTile) {  // (row tid is this thread's from here to the end: no barrier is needed for s_cur and the clearing of s_hit)
        int64_t start = 0;
        if constexpr (EMIT) {
            if (i0 + tid < Ba) start = seg_offsets[(i0 + tid) * nseg + seg];
        }
        s_cur[tid] = start;
        s_hit[tid][0] = s_hit[tid][1] = 0;
    }
    for (; tj < tj_end; ++tj) {
        const int64_t j0 = tj * kTile;
        int32_t eq[4][4], both[4][4];
        const int32_t staged = cmp_tile(a, Ba, b, Bb, S, i0, j0, eq, both);  // (its barriers: s_cur and the cleared s_hit are visible)
        const bool diagonal = r.upper && tj == strip;
        uint32_t flags = 0;  // bit 4 r + c
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t i = i0 + ty + 16 * rr;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t j = j0 + tx + 16 * c;
                const bool hit = i < Ba && j < Bb && (!diagonal || j > i) &&
                                 bsq_sketchd::pair_passes(eq[rr][c] - both[rr][c], staged - both[rr][c], r.min_match, r.jaccard_q16);
                flags |= static_cast<uint32_t>(hit) << (4 * rr + c);
                (c < 2 ? lo : hi) |= static_cast<uint32_t>(hit) << (tx + 16 * (c & 1));
            }
            if (lo) atomicOr(&s_hit[ty + 16 * rr][0], lo);
            if (hi) atomicOr(&s_hit[ty + 16 * rr][1], hi);
        }
        __syncthreads();
        if constexpr (EMIT) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                if ((flags >> (4 * rr)) & 15u) {
                    const int row = ty + 16 * rr;
                    const uint64_t mask = s_hit[row][0] | static_cast<uint64_t>(s_hit[row][1]) << 32;
                    const int64_t first = s_cur[row];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int64_t at = first + __popcll(mask & ((uint64_t(1) << (tx + 16 * c)) - 1));
                        // (unsigned: a start that is not the count call's -- a negative one -- writes nothing either)
                        if (((flags >> (4 * rr + c)) & 1u) && static_cast<uint64_t>(at) < static_cast<uint64_t>(out.max_pairs)) {
                            out.row[at] = i0 + row;
                            out.col[at] = j0 + tx + 16 * c;
                            out.match[at] = eq[rr][c] - both[rr][c];
                            if (out.either) out.either[at] = staged - both[rr][c];
                        }
                    }
                }
            }
            __syncthreads();  // (every read of s_cur and s_hit is done)
        }
        if (tid < kTile) {
            s_cur[tid] += __popc(s_hit[tid][0]) + __popc(s_hit[tid][1]);
            s_hit[tid][0] = s_hit[tid][1] = 0;
        }
    }
    if constexpr (!EMIT) {
        if (tid < kTile && i0 + tid < Ba) seg_offsets[1 + (i0 + tid) * nseg + seg] = s_cur[tid];
    }
}

__global__ __launch_bounds__(kThreads) void k_sketch_pairs_sums(int64_t n, int64_t *seg_offsets, int64_t *sums) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    lengths_step(k, n, seg_offsets, sums, [=](int64_t e) { return seg_offsets[e + 1]; });  // (writes the count back where it read it)
}

__global__ __launch_bounds__(1024) void k_sketch_pairs_scan(int64_t *sums, int64_t groups) { scan_inclusive_block(sums, groups); }

template <bool SCANNED>
__global__ __launch_bounds__(kThreads) void k_sketch_pairs_place(int64_t n, int64_t nseg, int64_t *seg_offsets, const int64_t *sums,
                                                                 int64_t *pair_offsets) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_d0[kPlaceS];
    place_offsets<SCANNED>(n, seg_offsets, sums, s_part, s_d0);
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kPlaceS + threadIdx.x;
    if (threadIdx.x < kPlaceS && k < n) {  // (the thread that wrote the end of entry k; nobody reads entry 0 in this launch)
        if (k == 0) seg_offsets[0] = 0;
        if (k % nseg == 0) pair_offsets[k / nseg] = s_d0[threadIdx.x];
        if (k == n - 1) pair_offsets[n / nseg] = seg_offsets[n];
    }
}

// ---- the clusters (include/bsq.h, "sketch clusters") ----
// The connected components of the "passes" graph by a lock-free union-find over `parent` (int64, a word per row), whose find and
// union text is bsq_sketch_dev.h's; three launches on one stream:
// k_cluster_init        parent[i] <- i.
// k_sketch_link<T>      k_sketch_pairs' geometry, upper: a workgroup per (strip of 64 rows, run of j tiles) walks its tiles in ascending j
//            with cmp_tile; every passing (i, j) is a union.  A tile without a hit costs one barrier more.  A tile with hits: the roots
//            of its 64 rows and 64 columns are found once (128 finds -> LDS); a hit whose two cached roots are equal is dropped there;
//            the others are united in a union-find of the tile's 128 nodes in LDS, and each node that ends below another hands ONE
//            union of the two cached roots to global memory -- at most 127 per tile, none in a store whose rows are one component already.
// k_cluster_link_pairs  the same union, an edge of an explicit list per lane (grid-stride).
// k_cluster_labels      behind the kernel boundary parent is final: labels[i] <- the root of i.
// Workgroups of one link launch talk through `parent` alone, so EVERY access to it there is an agent-scope atomic on the global address
// space (GlobalParent: relaxed loads, stores and compare-and-swaps, which are served by L2 and never by a CU's L1 or the scalar cache); the
// word is all that is communicated, so relaxed order is enough, and a parent that is no longer current was once true and costs a retry.
// No lane waits for another: every loop ends by the invariant parent[x] <= x or repeats after a swap that lost to a union that won.
struct GlobalParent {
    using Word = __attribute__((address_space(1))) int64_t;
    int64_t *p;
    __device__ __forceinline__ Word *at(int64_t x) const { return (Word *)(p + x); }
    __device__ __forceinline__ int64_t load(int64_t x) const { return __hip_atomic_load(at(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(int64_t x, int64_t v) const { __hip_atomic_store(at(x), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ bool swap_root(int64_t hi, int64_t lo) const {
        int64_t expected = hi;
        return __hip_atomic_compare_exchange_strong(at(hi), &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the tile's 128 nodes in LDS (rows 0 .. 63, columns 64 .. 127): the same text over workgroup-scope atomics
struct TileParent {
    int32_t *p;
    __device__ __forceinline__ int64_t load(int64_t x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void store(int64_t x, int64_t v) const {
        __hip_atomic_store(p + x, static_cast<int32_t>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ bool swap_root(int64_t hi, int64_t lo) const {
        int32_t expected = static_cast<int32_t>(hi);
        return __hip_atomic_compare_exchange_strong(p + hi, &expected, static_cast<int32_t>(lo), __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

__global__ __launch_bounds__(kThreads) void k_cluster_init(int64_t n, int64_t *parent) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(kThreads) void k_cluster_labels(int64_t n, int64_t *parent, int64_t *labels) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) labels[i] = bsq_sketchd::uf_find<false>(GlobalParent{parent}, i);
}

__global__ __launch_bounds__(kThreads) void k_cluster_link_pairs(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, int64_t *parent) {
    const GlobalParent global{parent};
    for (int64_t k = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n_pairs; k += static_cast<int64_t>(gridDim.x) * kThreads) {
        const int64_t i = row[k], j = col[k];
        if (bsq_sketchd::edge_links(i, j, n)) bsq_sketchd::uf_union(global, i, j);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sketch_link(const T *a, int64_t B, int32_t S, const PairsRule r, int64_t *parent) {
    __shared__ int64_t s_root[2 * kTile];  // the root of row i0 + t (t < 64), of column j0 + t - 64, found once per tile with hits
    __shared__ int32_t s_node[2 * kTile];  // the tile's own union-find over those 128 nodes
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t nseg = static_cast<uint32_t>(r.nseg), strip = blockIdx.x / nseg, seg = blockIdx.x - strip * nseg;
    const int64_t i0 = static_cast<int64_t>(strip) * kTile;
    int64_t tj = bsq_sketchd::segment_first_tile(seg, nseg, r.tiles_j);
    const int64_t tj_end = bsq_sketchd::segment_first_tile(seg + 1, nseg, r.tiles_j);
    if (tj < strip) tj = strip;  // (upper: the tiles left of the diagonal tile are another strip's)
    const GlobalParent global{parent};
    const TileParent local{s_node};
    for (; tj < tj_end; ++tj) {
        const int64_t j0 = tj * kTile;
        int32_t eq[4][4], both[4][4];
        const int32_t staged = cmp_tile(a, B, a, B, S, i0, j0, eq, both);  // (its barriers stand behind the last tile's reads of s_root and s_node)
        const bool diagonal = tj == strip;
        uint32_t flags = 0;  // bit 4 r + c
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t i = i0 + ty + 16 * rr;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t j = j0 + tx + 16 * c;
                const bool hit = i < B && j < B && (!diagonal || j > i) &&
                                 bsq_sketchd::pair_passes(eq[rr][c] - both[rr][c], staged - both[rr][c], r.min_match, r.jaccard_q16);
                flags |= static_cast<uint32_t>(hit) << (4 * rr + c);
            }
        }
        if (!__syncthreads_or(flags != 0)) continue;  // (uniform)
        if (tid < 2 * kTile) {
            const int64_t node = tid < kTile ? i0 + tid : j0 + tid - kTile;
            s_root[tid] = node < B ? bsq_sketchd::uf_find<true>(global, node) : -1;  // (a node outside the matrix has no hit)
            s_node[tid] = tid;
        }
        __syncthreads();
        for (uint32_t left = flags; left; left &= left - 1) {  // a thread's hits, one set bit at a time
            const int bit = __ffs(left) - 1, row = ty + 16 * (bit >> 2), col = kTile + tx + 16 * (bit & 3);
            if (s_root[row] != s_root[col]) bsq_sketchd::uf_union(local, row, col);
        }
        __syncthreads();
        if (tid < 2 * kTile) {  // (s_node is final: plain finds)
            const int64_t top = bsq_sketchd::uf_find<false>(local, tid);
            if (top != tid && s_root[tid] != s_root[top]) bsq_sketchd::uf_union(global, s_root[tid], s_root[top]);
        }
    }
}

template <typename T, int MODE>
void launch_minhash(bsq_rowtab::Form form, int64_t B, hipStream_t s, const SketchParams &p) {
    bsq_rowtab::launch(form, B, s, p, k_minhash_wave<T, MODE>, k_minhash_block<T, 1024, MODE>, k_minhash_block<T, 4096, MODE>,
                       k_minhash_block<T, 16384, MODE>);
}

template <typename T>
void launch_minhash(bsq_rowtab::Form form, int64_t B, hipStream_t s, const SketchParams &p, int mode) {
    if (mode == 0) launch_minhash<T, 0>(form, B, s, p);
    else if (mode == 1) launch_minhash<T, 1>(form, B, s, p);
    else launch_minhash<T, 2>(form, B, s, p);
}

}  // namespace

extern "C" {

const char *bsq_minhash_kernel_name(const bsq_desc *d, const bsq_minhash *m, int64_t B, bsq_dtype t) {
    Geometry g;
    const char *why = "";
    if (bsq_sketchd::check(d, m, B, t, &g, &why) != BSQ_OK) return "";
    return bsq_sketchd::form_name(bsq_sketchd::form_of(g.S, B, m->total_chars, m->form));
}

bsq_status bsq_minhash_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const bsq_minhash *m, bsq_dtype t,
                              void *out, void *hip_stream) {
    Geometry g;
    const bsq_status st = bsq_rowtab::check_all(B, chars, offsets, out, [&](const char **why) { return bsq_sketchd::check(d, m, B, t, &g, why); });
    if (st != BSQ_OK || B == 0) return st;
    SketchParams p;
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.out = out;
    p.B = B;
    p.lead = g.lead;
    p.mask = g.mask;
    p.salt = g.salt;
    p.S = g.S;
    p.k = g.k;
    p.A = g.A;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bsq_rowtab::Form form = bsq_sketchd::form_of(g.S, B, m->total_chars, m->form);
    const int mode = g.canonical ? 2 : (g.A == 4 ? 1 : 0);
    if (t == BSQ_I32) launch_minhash<int32_t>(form, B, s, p, mode);
    else launch_minhash<uint64_t>(form, B, s, p, mode);
    return bsq_internal::check_launch(bsq_sketchd::form_name(form));
}

bsq_status bsq_sketch_compare_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, int32_t *match,
                                     int32_t *either_or_null, void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_sketchd::check_compare(a, Ba, b, Bb, S, t, match, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (Ba == 0 || Bb == 0) return BSQ_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t tiles_i = (Ba + kTile - 1) / kTile, tiles_j = (Bb + kTile - 1) / kTile;  // (their product fits 31 bits: check_compare)
    const dim3 grid(static_cast<unsigned>(tiles_i * tiles_j)), block(kThreads);
    if (t == BSQ_I32)
        hipLaunchKernelGGL((k_sketch_compare<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb,
                           static_cast<int32_t>(S), static_cast<uint32_t>(tiles_j), match, either_or_null);
    else
        hipLaunchKernelGGL((k_sketch_compare<uint64_t>), grid, block, 0, s, static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb,
                           static_cast<int32_t>(S), static_cast<uint32_t>(tiles_j), match, either_or_null);
    return bsq_internal::check_launch("k_sketch_compare");
}

const char *bsq_sketch_pairs_kernel_name(int64_t Ba, int64_t Bb, int32_t segments) {
    const int32_t nseg = bsq_sketch_pairs_segments(Ba, Bb, segments);
    if (nseg == 0 || Ba > bsq_sketchd::kMaxRows || Bb > bsq_sketchd::kMaxRows) return "";
    if (Ba == 0 || Bb == 0) return "hipMemsetAsync";
    return form_of(Ba * nseg) != Form::ScanPlace ? "k_sketch_pairs<count>+k_sketch_pairs_sums+k_sketch_pairs_place;k_sketch_pairs<emit>"
                                                 : "k_sketch_pairs<count>+k_sketch_pairs_sums+k_sketch_pairs_scan+k_sketch_pairs_place;k_sketch_pairs<emit>";
}

bsq_status bsq_sketch_pairs_count_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                         int64_t *seg_offsets, int64_t *pair_offsets, void *hip_stream) {
    const char *why = "";
    PairsRule r;
    const bsq_status st = bsq_sketchd::check_pairs(a, Ba, b, Bb, S, t, rule, &r, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (!seg_offsets || !pair_offsets) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "seg_offsets or pair_offsets is null");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (Ba == 0 || Bb == 0) {  // (one segment: Ba + 1 entries each)
        hipError_t e = hipMemsetAsync(pair_offsets, 0, static_cast<size_t>(Ba + 1) * sizeof(int64_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(seg_offsets, 0, static_cast<size_t>(Ba + 1) * sizeof(int64_t), s);
        return e != hipSuccess ? bsq_internal::set_hip_error("hipMemsetAsync(sketch pairs)", e) : BSQ_OK;
    }
    const dim3 grid(static_cast<unsigned>(r.strips * r.nseg)), block(kThreads);  // (at most tiles_i * tiles_j: check_compare)
    const PairsOut none{nullptr, nullptr, nullptr, nullptr, 0};
    const int64_t n = Ba * r.nseg, nseg = r.nseg;  // the (row, segment) entries
    return with_wave_sums(n, s, "k_sketch_pairs<count> / k_sketch_pairs_sums / k_sketch_pairs_place", [&](int64_t *sums) {
        if (t == BSQ_I32)
            hipLaunchKernelGGL((k_sketch_pairs<int32_t, false>), grid, block, 0, s, static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b),
                               Bb, static_cast<int32_t>(S), r, seg_offsets, none);
        else
            hipLaunchKernelGGL((k_sketch_pairs<uint64_t, false>), grid, block, 0, s, static_cast<const uint64_t *>(a), Ba,
                               static_cast<const uint64_t *>(b), Bb, static_cast<int32_t>(S), r, seg_offsets, none);
        hipLaunchKernelGGL(k_sketch_pairs_sums, lengths_grid(n), block, 0, s, n, seg_offsets, sums);
        if (form_of(n) != Form::ScanPlace) {
            hipLaunchKernelGGL(k_sketch_pairs_place<false>, place_grid(n), block, 0, s, n, nseg, seg_offsets, sums, pair_offsets);
        } else {
            hipLaunchKernelGGL(k_sketch_pairs_scan, dim3(1), dim3(1024), 0, s, sums, (n + kPlaceS - 1) / kPlaceS);
            hipLaunchKernelGGL(k_sketch_pairs_place<true>, place_grid(n), block, 0, s, n, nseg, seg_offsets, sums, pair_offsets);
        }
    });
}

bsq_status bsq_sketch_pairs_emit_device(const void *a, int64_t Ba, const void *b, int64_t Bb, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule,
                                        const int64_t *seg_offsets, int64_t max_pairs, int64_t *row, int64_t *col, int32_t *match,
                                        int32_t *either_or_null, void *hip_stream) {
    const char *why = "";
    PairsRule r;
    const bsq_status st = bsq_sketchd::check_pairs(a, Ba, b, Bb, S, t, rule, &r, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (!seg_offsets || max_pairs < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "seg_offsets is null or max_pairs negative");
    if (max_pairs > 0 && (!row || !col || !match)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "an output array is null");
    if (Ba == 0 || Bb == 0 || max_pairs == 0) return BSQ_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 grid(static_cast<unsigned>(r.strips * r.nseg)), block(kThreads);
    const PairsOut out{row, col, match, either_or_null, max_pairs};
    int64_t *segs = const_cast<int64_t *>(seg_offsets);  // (the emit instantiation only reads them)
    if (t == BSQ_I32)
        hipLaunchKernelGGL((k_sketch_pairs<int32_t, true>), grid, block, 0, s, static_cast<const int32_t *>(a), Ba, static_cast<const int32_t *>(b), Bb,
                           static_cast<int32_t>(S), r, segs, out);
    else
        hipLaunchKernelGGL((k_sketch_pairs<uint64_t, true>), grid, block, 0, s, static_cast<const uint64_t *>(a), Ba, static_cast<const uint64_t *>(b), Bb,
                           static_cast<int32_t>(S), r, segs, out);
    return bsq_internal::check_launch("k_sketch_pairs<emit>");
}

const char *bsq_sketch_clusters_kernel_name(int64_t B, int32_t segments) {
    if (B <= 0 || B > bsq_sketchd::kMaxRows || bsq_sketch_pairs_segments(B, B, segments) == 0) return "";
    const int64_t tiles = (B + kTile - 1) / kTile;
    return tiles * tiles > bsq_sketchd::kMaxRows ? "" : "k_cluster_init+k_sketch_link+k_cluster_labels";
}

bsq_status bsq_sketch_clusters_device(const void *a, int64_t B, int64_t S, bsq_dtype t, const bsq_sketch_pairs *rule, int64_t *parent_scratch,
                                      int64_t *labels, void *hip_stream) {
    const char *why = "";
    PairsRule r;
    const bsq_status st = bsq_sketchd::check_clusters(a, B, S, t, rule, &r, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (B == 0) return BSQ_OK;
    if (!parent_scratch || !labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "parent_scratch or labels is null");
    if (parent_scratch == labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "labels must not be the parent scratch");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 rows(static_cast<unsigned>((B + kThreads - 1) / kThreads)), grid(static_cast<unsigned>(r.strips * r.nseg)), block(kThreads);
    hipLaunchKernelGGL(k_cluster_init, rows, block, 0, s, B, parent_scratch);
    if (t == BSQ_I32)
        hipLaunchKernelGGL((k_sketch_link<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(a), B, static_cast<int32_t>(S), r, parent_scratch);
    else
        hipLaunchKernelGGL((k_sketch_link<uint64_t>), grid, block, 0, s, static_cast<const uint64_t *>(a), B, static_cast<int32_t>(S), r, parent_scratch);
    hipLaunchKernelGGL(k_cluster_labels, rows, block, 0, s, B, parent_scratch, labels);
    return bsq_internal::check_launch("k_cluster_init / k_sketch_link / k_cluster_labels");
}

bsq_status bsq_cluster_pairs_device(const int64_t *row, const int64_t *col, int64_t n_pairs, int64_t n, int64_t *parent_scratch, int64_t *labels,
                                    void *hip_stream) {
    const char *why = "";
    const bsq_status st = bsq_sketchd::check_cluster_pairs(row, col, n_pairs, n, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n == 0) return BSQ_OK;
    if (!parent_scratch || !labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "parent_scratch or labels is null");
    if (parent_scratch == labels) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "labels must not be the parent scratch");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 nodes(static_cast<unsigned>((n + kThreads - 1) / kThreads)), block(kThreads);
    hipLaunchKernelGGL(k_cluster_init, nodes, block, 0, s, n, parent_scratch);
    if (n_pairs > 0) {  // (a lane per edge up to 2^20 workgroups, a stride of the grid beyond)
        const int64_t groups = (n_pairs + kThreads - 1) / kThreads, most = int64_t(1) << 20;
        hipLaunchKernelGGL(k_cluster_link_pairs, dim3(static_cast<unsigned>(groups < most ? groups : most)), block, 0, s, row, col, n_pairs, n,
                           parent_scratch);
    }
    hipLaunchKernelGGL(k_cluster_labels, nodes, block, 0, s, n, parent_scratch, labels);
    return bsq_internal::check_launch("k_cluster_init / k_cluster_link_pairs / k_cluster_labels");
}

}  // extern "C"
