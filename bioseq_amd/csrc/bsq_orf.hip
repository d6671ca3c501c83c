// Open reading frames of a packed residue batch resident in HBM (gfx950): the stop-free stretches of at least min_len residues of every
// row -- in practice of the six-frame rows bsq_translate_packed_device wrote --, counted, numbered by (row, start) and handed out as
// (row, start, length) view rows for bsq_views_packed_device.  The rule is bsq_orf_dev.h (include/bsq.h, "open reading frames",
// documents it); the host twins compile the same text.
//
// bsq_orf_count_device:  k_orf_count    the ORFs and the summed ORF length of every row; per-row counts -> orf_offsets[r + 1], the
//                                       count and the summed length of a workgroup's 64 rows -> the stream's scratch;
//                        k_orf_scan     beyond 2^20 rows: the 64-row sums scanned once by one workgroup (scan_inclusive_block);
//                        k_orf_offsets  counts -> offsets in place, a workgroup per 64 rows (place_offsets of bsq_ragged_out.h as it is),
//                                       and the summed lengths of 256 groups -> ONE atomicAdd on the total (an atomic per workgroup of
//                                       k_orf_count cost the count of a 1 M-read batch 0.9 ms of its 1.4: profiles/r18/orf_lab.txt).
// bsq_orf_emit_device:   k_orf_emit     walks the rows that have an ORF again and writes ORF k of row r at orf_offsets[r] + k: the
//                                       placement is a prefix count, never an atomic, so the order is the contract's.
//
// ROWS AND LANES.  A row is owned by FOUR lanes of one wave (a wave: 16 rows, a workgroup: 64 rows -- one group of the scaffold's sum
// hierarchy) and walked in pieces of 64 residues: a lane owns 16 consecutive residues, ONE unaligned 16-byte load, and builds its stop
// and start masks with word compares (mask16); four shuffles inside the quad give every lane the piece's two 64-bit masks, and the
// four lanes run the rule's bit arithmetic (piece_step) in step.  A round is kUnroll pieces, every load of a round issued before its
// first use (issuing the next round's loads ahead as well changed no measured figure: the walk is bound by vector issue).  Four lanes:
// a 50-residue frame of a 150-base read fills them (three loads and a two-byte tail) and sixteen reads share a wave; a 60 000-residue
// contig frame keeps kUnroll x 64 bytes per row and 4 KiB per wave in flight.
//
// No load touches a byte outside its own row: a lane takes the 16-byte load only when its sixteen residues are whole inside the row;
// the at most 15 residues left are byte loads of the one lane they fall to.  A row is never split across waves.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_orf_dev.h"
#include "bsq_ragged_out.h"

namespace {

using bsq_orfs::Carry;
using bsq_orfs::kChunk;
using bsq_orfs::kPiece;
using bsq_orfs::Rule;

constexpr int kQuad = kPiece / kChunk;  // lanes of a row
constexpr int kUnroll = 4;              // pieces of a round: the loads a lane issues together
constexpr int kRound = kPiece * kUnroll;
constexpr int64_t kMaxRows = ((int64_t(1) << 31) - 1) * kPlaceS;  // a grid of 2^31 - 1 workgroups
static_assert(kQuad == 4 && kThreads / kQuad == kPlaceS, "a workgroup owns the 64 rows of one group of the scaffold");

// a lane's sixteen residues of each of the kUnroll pieces from base0 on: the 16-byte load where they are whole inside the row, else zeros
__device__ __forceinline__ void load_round(v_u32x4u *x, const uint8_t *row, int64_t m, int64_t base0, int sub) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int64_t at = base0 + u * kPiece + sub * kChunk;
        x[u] = v_u32x4u{0u, 0u, 0u, 0u};
        if (at + kChunk <= m) x[u] = *reinterpret_cast<const v_u32x4u *>(row + at);
    }
}

// Every ORF of row[0 .. m) in order of its start, by the row's four lanes in step (sub = lane in the quad): emit(start, length) runs
// in all four.  Control flow is uniform over the quad, so the shuffles meet the lanes they read.
template <class Emit>
__device__ __forceinline__ void walk_row(const Rule &r, const uint8_t *row, int64_t m, int sub, Emit &emit) {
    Carry c = bsq_orfs::row_begin();
    for (int64_t base0 = 0; base0 < m; base0 += kRound) {
        v_u32x4u x[kUnroll];
        load_round(x, row, m, base0, sub);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t base = base0 + u * kPiece;
            if (base >= m) break;
            const int64_t at = base + sub * kChunk;
            const int64_t left = m - at;  // residues of this lane's sixteen inside the row
            uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
            if (left > 0 && left < kChunk) {  // the tail: byte loads inside the row (unrolled: every word index is a constant)
#pragma unroll
                for (int k = 0; k < kChunk - 1; ++k)
                    if (k < left) w[k >> 2] |= uint32_t(row[at + k]) << (8 * (k & 3));
            }
            const uint32_t live = bsq_orfs::low_bits16(left);
            uint32_t mine = bsq_orfs::mask16(w, r.stop4) & live;
            if (r.start_mode) mine |= (bsq_orfs::mask16(w, r.start4) & live) << 16;
            uint64_t S = 0, T = 0;
#pragma unroll
            for (int q = 0; q < kQuad; ++q) {
                const uint32_t theirs = __shfl(mine, q, kQuad);
                S |= uint64_t(theirs & 0xFFFFu) << (q * kChunk);
                T |= uint64_t(theirs >> 16) << (q * kChunk);
            }
            bsq_orfs::piece_step(r, c, S, T, base, emit);
        }
    }
    bsq_orfs::row_end(r, c, m, emit);
}

__device__ __forceinline__ int64_t row_len(const int64_t *offsets, int64_t i, int64_t *o0) {
    *o0 = offsets[i];
    const int64_t m = offsets[i + 1] - *o0;
    return m > 0 ? m : 0;
}

__global__ __launch_bounds__(kThreads) void k_orf_count(Rule r, const uint8_t *chars, const int64_t *offsets, int64_t n, int64_t *orf_offsets,
                                                        int64_t *group_sums, int64_t *group_residues) {
    __shared__ int64_t s_count[kThreads / 64], s_res[kThreads / 64];
    const int tid = threadIdx.x, sub = tid & (kQuad - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPlaceS + tid / kQuad;
    int64_t count = 0, res = 0;
    if (i < n) {
        int64_t o0;
        const int64_t m = row_len(offsets, i, &o0);
        auto emit = [&](int64_t, int64_t len) {
            ++count;
            res += len;
        };
        walk_row(r, chars + o0, m, sub, emit);
        if (sub == 0) orf_offsets[i + 1] = count;
    }
    if (i == 0 && sub == 0) orf_offsets[0] = 0;
    const int64_t wc = wave_sum(sub == 0 ? count : 0), wr = wave_sum(sub == 0 ? res : 0);
    if ((tid & 63) == 0) {
        s_count[tid >> 6] = wc;
        s_res[tid >> 6] = wr;
    }
    __syncthreads();
    if (tid == 0) {
        group_sums[blockIdx.x] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
        group_residues[blockIdx.x] = s_res[0] + s_res[1] + s_res[2] + s_res[3];
    }
}

__global__ __launch_bounds__(1024) void k_orf_scan(int64_t *v, int64_t n) { scan_inclusive_block(v, n); }

// SCANNED: k_orf_scan ran (place_offsets)
// The summed ORF length rides along: workgroup b adds up the residues of the groups [256 b, 256 b + 256) and, when there are any, adds them
// to *residues -- one atomic per 16 384 rows, and an integer sum, so the order of the additions does not show.
template <bool SCANNED>
__global__ __launch_bounds__(kThreads) void k_orf_offsets(int64_t n, int64_t *orf_offsets, const int64_t *group_sums, const int64_t *group_residues,
                                                          unsigned long long *residues) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_d0[kPlaceS];
    __shared__ int64_t s_res[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + tid;
    const int64_t mine = wave_sum(residues && g < (n + kPlaceS - 1) / kPlaceS ? group_residues[g] : 0);
    if ((tid & 63) == 0) s_res[tid >> 6] = mine;
    place_offsets<SCANNED>(n, orf_offsets, group_sums, s_part, s_d0);  // (its barriers stand between the two uses of s_res)
    if (tid == 0) {
        const int64_t total = s_res[0] + s_res[1] + s_res[2] + s_res[3];
        if (total) atomicAdd(residues, static_cast<unsigned long long>(total));
    }
}

__global__ __launch_bounds__(kThreads) void k_orf_emit(Rule r, const uint8_t *chars, const int64_t *offsets, int64_t n, const int64_t *orf_offsets,
                                                       int64_t max_orfs, int64_t *out_row, int64_t *out_start, int64_t *out_length) {
    const int tid = threadIdx.x, sub = tid & (kQuad - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPlaceS + tid / kQuad;
    if (i >= n) return;
    int64_t rank = orf_offsets[i];
    if (rank < 0 || rank >= max_orfs || orf_offsets[i + 1] == rank) return;  // (uniform over the quad)
    int64_t o0;
    const int64_t m = row_len(offsets, i, &o0);
    auto emit = [&](int64_t s, int64_t len) {
        if (sub == 0 && rank < max_orfs) {
            out_row[rank] = i;
            out_start[rank] = s;
            out_length[rank] = len;
        }
        ++rank;
    };
    walk_row(r, chars + o0, m, sub, emit);
}

// the checks both device calls run first; BSQ_OK and the rule
bsq_status check(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, const int64_t *orf_offsets, Rule *r) {
    if (!offsets || !orf_offsets || n_rows < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "null pointer or negative size");
    if (n_rows > 0 && !chars) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "chars is null");
    if (n_rows > kMaxRows) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "too many rows");
    const char *why = "";
    if (bsq_orfs::make_rule(o, r, &why) != BSQ_OK) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, why);
    return BSQ_OK;
}

}  // namespace

extern "C" {

bsq_status bsq_orf_count_device(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, int64_t *orf_offsets,
                                int64_t *residues_or_null, void *hip_stream) {
    Rule r;
    const bsq_status st = check(chars, offsets, n_rows, o, orf_offsets, &r);
    if (st != BSQ_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipError_t e = residues_or_null ? hipMemsetAsync(residues_or_null, 0, sizeof(int64_t), s) : hipSuccess;
    if (e == hipSuccess && n_rows == 0) e = hipMemsetAsync(orf_offsets, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return bsq_internal::set_hip_error("hipMemsetAsync(orf count)", e);
    if (n_rows == 0) return BSQ_OK;
    unsigned long long *residues = reinterpret_cast<unsigned long long *>(residues_or_null);
    // the scratch holds two entries per 64-row group, counts then residues: with_wave_sums sizes it by rows, so ask for twice the rows
    const int64_t groups = (n_rows + kPlaceS - 1) / kPlaceS;
    return with_wave_sums(2 * groups * kPlaceS, s, "k_orf_count / k_orf_offsets", [&](int64_t *sums) {
        const dim3 grid = place_grid(n_rows), block(kThreads);
        hipLaunchKernelGGL(k_orf_count, grid, block, 0, s, r, chars, offsets, n_rows, orf_offsets, sums, sums + groups);
        if (form_of(n_rows) != Form::ScanPlace) {
            hipLaunchKernelGGL(k_orf_offsets<false>, grid, block, 0, s, n_rows, orf_offsets, sums, sums + groups, residues);
        } else {
            hipLaunchKernelGGL(k_orf_scan, dim3(1), dim3(1024), 0, s, sums, groups);
            hipLaunchKernelGGL(k_orf_offsets<true>, grid, block, 0, s, n_rows, orf_offsets, sums, sums + groups, residues);
        }
    });
}

bsq_status bsq_orf_emit_device(const uint8_t *chars, const int64_t *offsets, int64_t n_rows, const bsq_orf *o, const int64_t *orf_offsets,
                               int64_t max_orfs, int64_t *out_row, int64_t *out_start, int64_t *out_length, void *hip_stream) {
    Rule r;
    const bsq_status st = check(chars, offsets, n_rows, o, orf_offsets, &r);
    if (st != BSQ_OK) return st;
    if (max_orfs < 0) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "max_orfs is negative");
    if (max_orfs > 0 && (!out_row || !out_start || !out_length)) return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "an output array is null");
    if (n_rows == 0 || max_orfs == 0) return BSQ_OK;
    hipLaunchKernelGGL(k_orf_emit, place_grid(n_rows), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), r, chars, offsets, n_rows,
                       orf_offsets, max_orfs, out_row, out_start, out_length);
    return bsq_internal::check_launch("k_orf_emit");
}

const char *bsq_orf_kernel_name(int64_t n_rows) {
    if (n_rows < 0 || n_rows > kMaxRows) return "";
    if (n_rows == 0) return "hipMemsetAsync";
    return form_of(n_rows) != Form::ScanPlace ? "k_orf_count+k_orf_offsets;k_orf_emit" : "k_orf_count+k_orf_scan+k_orf_offsets;k_orf_emit";
}

}  // extern "C"
