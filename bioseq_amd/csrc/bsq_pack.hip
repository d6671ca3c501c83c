// Sequence packing on the device (gfx950): include/bsq.h ("sequence packing") has the rules, bsq_pack_dev.h the arithmetic of the plan and
// the value of one position as host + device code, bsq_pack_host.cpp the CPU twins.
//
// THE PLAN (bsq_pack_plan_device), stream-ordered, no read-back, no host loop over sequences:
//   k_pack_next    a[i] = next_head(i): one binary search per sequence over the closed-form prefix; mark[0] = 1
//   k_pack_jump    one round of pointer jumping, four hops: ceil(log4 B) launches mark the chain of row heads
//   k_pack_heads   (heads, last head) of every block of 4096 sequences;  k_pack_sums  their exclusive scan, one workgroup
//   k_pack_place   the scan inside the block, then starts[i] = row * P + S_i - S_head, the rows = N rule, n_rows, n_placed
// Stream mode has no rows to find: k_pack_place alone.
//
// THE ENCODE (bsq_pack_tokenize_device), one launch, output-driven:
//   k_pack_flat<T, PERM>  the (rows, P) matrix is one flat stream.  A lane owns 16 consecutive positions (the piece mapping and the
//            stores of k_kmer_bp: bsq_piece_store.h -- 16-byte non-temporal stores, whole 1-KiB runs per wave whatever the lengths
//            are), a wave 1024.  The wave finds the sequences at the start of its first row and at its first position by a 64-ary search in
//            `starts` (find_wave: its lanes probe together); the lanes gallop from there to their own first position and walk forward
//            (bsq_packd::Cursor).  A lane whose 16 positions lie
//            inside the characters of one run -- nearly all of them -- takes one unaligned 16-byte load and the register-table
//            lookup (<perm>: v_perm_b32 on the folded alphabet table, as k_tokens_bp8) or four LDS-table reads per word (<lut>: an
//            alphabet that does not fold); every other lane (run boundaries, BOS / EOS, PAD gaps, row ends) goes position by
//            position.  segment_ids and position_ids come out of the same walk.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_internal.h"
#include "bsq_pack_dev.h"
#include "bsq_pack_flat.h"
#include "bsq_piece_store.h"

namespace {

using namespace bsq_dev;  // kThreads, Div64, write_out
using bsq_packd::Cursor;
using bsq_packd::Ids;
using namespace bsq_packf;  // lookup4_perm, nonletter_mask, find_wave, fold_table

constexpr int kPer = 16;                       // sequences per thread of the scan kernels
constexpr int64_t kScanBlock = kThreads * kPer;  // sequences per block

// ---- plan ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pack_next(const int64_t *offsets, int64_t B, int64_t be, int64_t P, int32_t *a, uint8_t *mark) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i > B) return;
    a[i] = static_cast<int32_t>(i < B ? bsq_packd::next_head(offsets, B, be, P, i) : B);
    mark[i] = i == 0;
}

__global__ __launch_bounds__(kThreads) void k_pack_jump(const int32_t *from, int32_t *to, uint8_t *mark, int64_t B) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i <= B) bsq_packd::jump_round(from, to, mark, i);
}

// Inclusive scan over the block's threads of (cnt: sum, head: max); s_c / s_h: kThreads entries each, left holding the inclusive values.
__device__ __forceinline__ void block_scan(int64_t cnt, int64_t head, int64_t *s_c, int64_t *s_h) {
    const int t = threadIdx.x;
    s_c[t] = cnt, s_h[t] = head;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kThreads; d += d) {
        const int64_t c = t >= d ? s_c[t - d] : 0, h = t >= d ? s_h[t - d] : -1;
        __syncthreads();
        s_c[t] += c;
        s_h[t] = s_h[t] > h ? s_h[t] : h;
        __syncthreads();
    }
}

__device__ __forceinline__ void count_heads(const uint8_t *mark, int64_t B, int64_t i0, int64_t &cnt, int64_t &head) {
    cnt = 0, head = -1;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (i0 + k < B && mark[i0 + k]) ++cnt, head = i0 + k;
}

__global__ __launch_bounds__(kThreads) void k_pack_heads(const uint8_t *mark, int64_t B, int64_t *bcount, int64_t *bhead) {
    __shared__ int64_t s_c[kThreads], s_h[kThreads];
    int64_t cnt, head;
    count_heads(mark, B, (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kPer, cnt, head);
    block_scan(cnt, head, s_c, s_h);
    if (threadIdx.x == kThreads - 1) bcount[blockIdx.x] = s_c[kThreads - 1], bhead[blockIdx.x] = s_h[kThreads - 1];
}

// bcount / bhead: per-block totals -> what lies in front of each block (exclusive), in place; one workgroup walks the tiles.
__global__ __launch_bounds__(kThreads) void k_pack_sums(int64_t *bcount, int64_t *bhead, int64_t nblk) {
    __shared__ int64_t s_c[kThreads], s_h[kThreads];
    int64_t carry_c = 0, carry_h = -1;
    for (int64_t b0 = 0; b0 < nblk; b0 += kThreads) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t c = b < nblk ? bcount[b] : 0, h = b < nblk ? bhead[b] : -1;
        block_scan(c, h, s_c, s_h);
        const int64_t ec = carry_c + s_c[threadIdx.x] - c;
        int64_t eh = threadIdx.x > 0 ? s_h[threadIdx.x - 1] : -1;
        eh = eh > carry_h ? eh : carry_h;
        if (b < nblk) bcount[b] = ec, bhead[b] = eh;
        const int64_t tc = s_c[kThreads - 1], th = s_h[kThreads - 1];
        __syncthreads();  // (the next tile's block_scan overwrites s_c / s_h)
        carry_c += tc;
        carry_h = th > carry_h ? th : carry_h;
    }
}

struct PlaceParams {
    const int64_t *offsets;
    const uint8_t *mark;      // null in stream mode
    const int64_t *bcount, *bhead;
    int64_t *starts, *n_rows;
    unsigned long long *n_placed;  // zeroed before the launch
    int64_t B, P, be, limit;  // limit: positions of the matrix that runs must end in (INT64_MAX: no limit)
    int32_t nextfit;
};

__global__ __launch_bounds__(kThreads) void k_pack_place(const PlaceParams p) {
    __shared__ int64_t s_c[kThreads], s_h[kThreads];
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kPer;
    if (p.B == 0) {
        if (i0 == 0) p.starts[0] = 0, *p.n_rows = 0;
        return;
    }
    int64_t heads = 0, head = 0;
    if (p.nextfit) {
        int64_t cnt, last;
        count_heads(p.mark, p.B, i0, cnt, last);
        block_scan(cnt, last, s_c, s_h);
        heads = p.bcount[blockIdx.x] + s_c[threadIdx.x] - cnt;
        const int64_t h = threadIdx.x > 0 ? s_h[threadIdx.x - 1] : -1, hb = p.bhead[blockIdx.x];
        head = h > hb ? h : hb;
        __syncthreads();
    }
    // this thread's sequences and the one behind them: whether a run is the last one placed shows at its successor
    int64_t placed = 0, prev_end = -1;
    bool prev_in = false;
    for (int k = 0; k <= kPer; ++k) {
        const int64_t i = i0 + k;
        if (i > p.B || (i == p.B && k == 0)) break;
        bool in = false;
        int64_t start = 0, end = 0;
        if (i < p.B) {
            if (p.nextfit && p.mark[i]) ++heads, head = i;
            start = bsq_packd::place(p.offsets, p.be, p.P, p.nextfit, i, heads, head < 0 ? 0 : head);
            end = start + bsq_packd::taken(p.offsets, p.be, p.P, p.nextfit, i);
            in = end <= p.limit;  // (well-formed offsets: ends never decrease, so the placed runs are the prefix the CPU twin counts; offsets
                                  //  that validation would refuse -- negative lengths -- are memory-safe here but may place other runs than the twin)
            if (k < kPer) {
                p.starts[i] = in ? start : -1;
                placed += in;
                if (i == p.B - 1)
                    *p.n_rows = p.nextfit ? heads : bsq_packd::stream_rows(bsq_packd::prefix(p.offsets, p.B, p.be), p.P);
            }
        }
        if (k > 0 && prev_in && !in) p.starts[p.B] = prev_end;
        if (i == 0 && !in) p.starts[p.B] = 0;
        prev_in = in, prev_end = end;
    }
    if (placed) atomicAdd(p.n_placed, static_cast<unsigned long long>(placed));
}

// ---- encode --------------------------------------------------------------------------------------------------------------------
struct PackParams {
    const uint8_t *chars;
    const int64_t *offsets, *starts;
    void *tokens;
    int32_t *seg, *pos;  // either may be null
    int64_t B, P, total, npieces;
    Div64 div_P;
    Ids ids;
    uint32_t tab[8];  // PERM: token value of letter (c & 31), 0 for an unmapped one
    int8_t lut[256];
};

template <typename T, bool PERM>
__global__ __launch_bounds__(kThreads) void k_pack_flat(const PackParams p) {
    __shared__ int8_t s_lut[256];
    __shared__ __align__(16) uint4 s_out[kThreads * (sizeof(T) > 4 ? sizeof(T) : 4)];
    s_lut[threadIdx.x] = p.lut[threadIdx.x];  // (kThreads == 256)
    __syncthreads();
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads;
    const bool staged = (first + kThreads) * 16 <= p.total;  // (block-uniform: every piece of the block is whole)
    int64_t gid = first + threadIdx.x;
    const bool valid = gid < p.npieces;
    if (!valid) gid = p.npieces - 1;  // (a thread past the end computes the last piece again and stores nothing)
    const int64_t q0 = gid * 16;
    const uint32_t n_el = static_cast<uint32_t>(p.total - q0 < 16 ? p.total - q0 : 16);
    const int64_t be = p.ids.bos + p.ids.eos, B = p.B, P = p.P;
    const int64_t nchars = B > 0 ? p.offsets[B] : 0;

    // the wave's seeds (wave-uniform, found by the 64 lanes together): the sequence at column 0 of the row its first position lies in
    // and the one at that position; every lane then gallops the few sequences from there to its own row start and position
    int64_t gw = first + (threadIdx.x & ~63u);
    gw = gw < p.npieces ? gw : p.npieces - 1;
    const int64_t row_w = static_cast<int64_t>(div64(static_cast<uint64_t>(gw * 16), p.div_P));
    const int64_t seed_row = find_wave(p.starts, B, static_cast<uint64_t>(row_w * P));
    const int64_t seed = find_wave(p.starts, B, static_cast<uint64_t>(gw * 16));
    const int64_t row0 = static_cast<int64_t>(div64(static_cast<uint64_t>(q0), p.div_P));
    int64_t col = q0 - row0 * P;
    int64_t i_first = row0 == row_w ? seed_row : bsq_packd::find(p.starts, B, seed_row, static_cast<uint64_t>(row0 * P));
    Cursor c = bsq_packd::cursor_at(p.offsets, p.starts, B, be, bsq_packd::find(p.starts, B, seed, static_cast<uint64_t>(q0)));

    T v[16];
    int32_t sg[16], ps[16];
    const int64_t j0 = q0 - c.s - p.ids.bos, a0 = c.off + j0;
    const bool fast = c.i >= 0 && n_el == 16 && j0 >= 0 && j0 + 16 <= c.L && static_cast<uint64_t>(q0) + 16 <= c.e && col + 16 <= P &&
                      a0 >= 0 && a0 + 16 <= nchars;
    if (fast) {
        const u32x4_unaligned x = *reinterpret_cast<const u32x4_unaligned *>(p.chars + a0);
        const uint32_t cw[4] = {x.x, x.y, x.z, x.w};
        const int32_t s = static_cast<int32_t>(1 + c.i - i_first), k0 = static_cast<int32_t>(q0 - c.s);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t w;
            if constexpr (PERM) {
                w = lookup4_perm(cw[u], p.tab) & ~nonletter_mask(cw[u]);
            } else {
                w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int32_t id = s_lut[(cw[u] >> (8 * b)) & 0xFFu];
                    w |= static_cast<uint32_t>(id < 0 ? 0 : id) << (8 * b);
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                v[4 * u + b] = static_cast<T>(static_cast<int32_t>((w >> (8 * b)) & 0xFFu));
                sg[4 * u + b] = s;
                ps[4 * u + b] = k0 + 4 * u + b;
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const int64_t q = q0 + k;
            int32_t x = p.ids.pad_store, s = 0, n = 0;
            if (k < n_el) {
                if (static_cast<uint64_t>(q) >= c.next) c = bsq_packd::cursor_at(p.offsets, p.starts, B, be, bsq_packd::find(p.starts, B, c.i, static_cast<uint64_t>(q)));
                if (col == P) col = 0;
                if (col == 0) i_first = c.i;
                if (c.i >= 0 && static_cast<uint64_t>(q) < c.e) {
                    x = bsq_packd::run_token(p.ids, s_lut, p.chars, c.off, c.L, nchars, q - c.s);
                    s = static_cast<int32_t>(1 + c.i - i_first);
                    n = static_cast<int32_t>(q - c.s);
                }
                ++col;
            }
            v[k] = static_cast<T>(x), sg[k] = s, ps[k] = n;
        }
    }
    write_out(static_cast<T *>(p.tokens), gid, q0, v, n_el, valid, staged, s_out);
    if (p.seg) write_out(p.seg, gid, q0, sg, n_el, valid, staged, s_out);
    if (p.pos) write_out(p.pos, gid, q0, ps, n_el, valid, staged, s_out);
}

const char *form_name(bool perm) { return perm ? "k_pack_flat<perm>" : "k_pack_flat<lut>"; }

using bsq_internal::check_launch;

}  // namespace

extern "C" {

const char *bsq_pack_kernel_name(const bsq_desc *d, int64_t B, int64_t rows, int64_t P, bsq_dtype t) {
    static const int64_t one[2] = {0, 0};
    static const uint8_t none[1] = {0};
    if (bsq_pack_host::check_encode(d, none, one, B, one, rows, P, t, none) != BSQ_OK) return "";
    uint32_t tab[8];
    return form_name(fold_table(d, tab));
}

bsq_status bsq_pack_plan_device(const int64_t *offsets, int64_t B, int64_t P, int32_t bos, int32_t eos, int32_t mode, int64_t max_rows,
                                int64_t *starts, int64_t *n_rows, int64_t *n_placed_or_null, void *hip_stream) {
    bsq_status st = bsq_pack_host::check_plan(offsets, B, P, bos, eos, mode, max_rows, starts, n_rows);
    if (st != BSQ_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t nblk = B == 0 ? 1 : (B + kScanBlock - 1) / kScanBlock;
    const bool nextfit = mode == BSQ_PACK_NEXTFIT && B > 0;
    // scratch: the two jump tables, the marks, the per-block scan values and a stand-in for n_placed
    const size_t n1 = static_cast<size_t>(B) + 1;
    const size_t tab_bytes = (n1 * sizeof(int32_t) + 15) & ~size_t(15), mark_bytes = (n1 + 15) & ~size_t(15);
    const size_t blk_bytes = static_cast<size_t>(nblk) * sizeof(int64_t);
    const size_t need = (nextfit ? 2 * tab_bytes + mark_bytes + 2 * blk_bytes : 0) + 16;
    std::lock_guard<std::mutex> scratch_turn(bsq_internal::workspace_mutex());
    void *ws = nullptr;
    st = bsq_internal::workspace_acquire(need, s, &ws);
    if (st != BSQ_OK) return st;
    char *at = static_cast<char *>(ws);
    PlaceParams p;
    p.n_placed = reinterpret_cast<unsigned long long *>(n_placed_or_null ? n_placed_or_null : reinterpret_cast<int64_t *>(at));
    at += 16;
    p.offsets = offsets;
    p.mark = nullptr;
    p.bcount = p.bhead = nullptr;
    p.starts = starts;
    p.n_rows = n_rows;
    p.B = B;
    p.P = P;
    p.be = bos + eos;
    p.limit = max_rows > 0 ? max_rows * P : INT64_MAX;
    p.nextfit = nextfit;
    hipError_t e = hipMemsetAsync(p.n_placed, 0, sizeof(int64_t), s);
    if (e == hipSuccess && nextfit) {
        int32_t *a = reinterpret_cast<int32_t *>(at), *b = reinterpret_cast<int32_t *>(at + tab_bytes);
        uint8_t *mark = reinterpret_cast<uint8_t *>(at + 2 * tab_bytes);
        int64_t *bcount = reinterpret_cast<int64_t *>(at + 2 * tab_bytes + mark_bytes), *bhead = bcount + nblk;
        const unsigned grid = static_cast<unsigned>((B + 1 + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(k_pack_next, dim3(grid), dim3(kThreads), 0, s, offsets, B, p.be, P, a, mark);
        for (int32_t r = bsq_packd::jump_rounds(B); r > 0; --r) {
            hipLaunchKernelGGL(k_pack_jump, dim3(grid), dim3(kThreads), 0, s, a, b, mark, B);
            int32_t *t = a;
            a = b, b = t;
        }
        hipLaunchKernelGGL(k_pack_heads, dim3(static_cast<unsigned>(nblk)), dim3(kThreads), 0, s, mark, B, bcount, bhead);
        hipLaunchKernelGGL(k_pack_sums, dim3(1), dim3(kThreads), 0, s, bcount, bhead, nblk);
        p.mark = mark;
        p.bcount = bcount;
        p.bhead = bhead;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pack_place, dim3(static_cast<unsigned>(nblk)), dim3(kThreads), 0, s, p);
        e = hipGetLastError();
    }
    bsq_internal::workspace_release(ws, s);
    return e != hipSuccess ? bsq_internal::set_hip_error("bsq_pack_plan_device", e) : BSQ_OK;
}

bsq_status bsq_pack_tokenize_device(const bsq_desc *d, const uint8_t *chars, const int64_t *offsets, int64_t B, const int64_t *starts,
                                    int64_t rows, int64_t P, bsq_dtype t, void *tokens, int32_t *segment_ids_or_null,
                                    int32_t *position_ids_or_null, void *hip_stream) {
    bsq_status st = bsq_pack_host::check_encode(d, chars, offsets, B, starts, rows, P, t, tokens);
    if (st != BSQ_OK || rows == 0) return st;
    PackParams p;
    const bool perm = fold_table(d, p.tab);
    std::memcpy(p.lut, d->lut, 256);
    p.chars = chars;
    p.offsets = offsets;
    p.starts = starts;
    p.tokens = tokens;
    p.seg = segment_ids_or_null;
    p.pos = position_ids_or_null;
    p.B = B;
    p.P = P;
    p.total = rows * P;
    p.npieces = (p.total + 15) / 16;
    p.div_P = div64_constants(static_cast<uint64_t>(P));
    p.ids = bsq_packd::make_ids(d);
    const unsigned grid = static_cast<unsigned>((p.npieces + kThreads - 1) / kThreads);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    st = bsq_internal::with_value_type(t, [&](auto tag) {
        using T = decltype(tag);
        if (perm) hipLaunchKernelGGL((k_pack_flat<T, true>), dim3(grid), dim3(kThreads), 0, s, p);
        else hipLaunchKernelGGL((k_pack_flat<T, false>), dim3(grid), dim3(kThreads), 0, s, p);
        return BSQ_OK;
    });
    return st != BSQ_OK ? st : check_launch(form_name(perm));
}

}  // extern "C"
