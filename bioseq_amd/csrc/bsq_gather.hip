// Index-list batches out of a packed store that lives in HBM (SURVEY.md section 8 row f-3 under a shuffling sampler).
//
// The reference's FlatFileDataset.__getitem__ (/root/reference/bioseq/loaders.py:76-104) fetches ONE sequence per call from
// the memory-mapped file, tokenises it on the host and lets the DataLoader stack the results; a shuffled epoch therefore
// touches the host for every sample.  Here the whole FlatFile is uploaded once (FlatFile.to_device) and a batch of
// arbitrary, repeated or empty sequence indices is rebuilt ON THE DEVICE as a packed batch (chars, offsets) that the
// encode kernels consume as they are: ONE launch for loader-sized batches (k_gather_small), two beyond 4096 indices (k_gather_lengths2 +
// k_gather_place, round 6), no host round trip, no H2D copy.  The three launches of rounds 2-5 stay behind knob "gather_small" = 1:
//   k_gather_lengths  out_offsets[i + 1] <- length of sequence index[i]   (bad indices: length 0, position recorded)
//   k_gather_scan     in-place inclusive prefix sum -> out_offsets[i + 1] = end of output sequence i  (one workgroup;
//                     a batch is 10^3 .. 10^6 sequences: 8 MB at most, microseconds)
//   k_gather_chars    16 lanes per output sequence copy its characters with unaligned 16-byte loads / stores
// The offsets scaffold of the launch classes (front sums, scans, the cut at the capacity, the scratch of the sums) is bsq_ragged_out.h,
// shared with the views and the translation and described there; this file keeps the index look-up, the copy loops, the knob and the
// order of its launches.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_internal.h"
#include "bsq_ragged_out.h"

namespace {

__global__ __launch_bounds__(kThreads) void k_gather_lengths(const int64_t *offsets, int64_t n_store, const int64_t *index,
                                                             int64_t n, int64_t *out_offsets, unsigned long long *first_bad) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i == 0) out_offsets[0] = 0;
    if (i >= n) return;
    const int64_t j = index[i];
    int64_t len = 0;
    if (j >= 0 && j < n_store) {
        len = offsets[j + 1] - offsets[j];
        if (len < 0) len = 0;
    } else if (first_bad) {
        atomicMin(first_bad, static_cast<unsigned long long>(i));
    }
    out_offsets[i + 1] = len;
}

__global__ __launch_bounds__(1024) void k_gather_scan(int64_t *v, int64_t n) { scan_inclusive_block(v, n); }

// 16 lanes per output sequence.  capacity: bytes of out_chars; a batch that does not fit is cut there (never a write
// past the buffer) and recorded in first_bad as position n + i.
__global__ __launch_bounds__(kThreads) void k_gather_chars(const uint8_t *chars, const int64_t *offsets, int64_t n_store,
                                                           const int64_t *index, int64_t n, const int64_t *out_offsets,
                                                           uint8_t *out_chars, int64_t capacity, unsigned long long *first_bad) {
    const int sub = threadIdx.x & 15;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kThreads / 16) + (threadIdx.x >> 4);
    if (i >= n) return;
    const int64_t j = index[i];
    if (j < 0 || j >= n_store) return;
    const int64_t src0 = offsets[j], d0 = out_offsets[i];
    const int64_t len = cut_at_capacity(d0, out_offsets[i + 1] - d0, capacity, n, i, sub, first_bad);
    const uint8_t *src = chars + src0;
    uint8_t *dst = out_chars + d0;
    const int64_t body = len & ~int64_t(15);
    for (int64_t p = sub * 16; p < body; p += 256)
        *reinterpret_cast<v_u32x4u *>(dst + p) = *reinterpret_cast<const v_u32x4u *>(src + p);
    if (sub < (len & 15)) dst[body + sub] = src[body + sub];
}

// Loader-sized batches (n <= kSmallN: what a training step asks for) in ONE launch instead of memset + three (the `small` class of
// bsq_ragged_out.h; profiles/r04/loader_step_lab.txt).  first_bad may be null (a caller that vouches for its indices).
__global__ __launch_bounds__(kThreads) void k_gather_small(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index,
                                                           int64_t n, int64_t *out_offsets, uint8_t *out_chars, int64_t capacity,
                                                           unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_len[16];
    const int tid = threadIdx.x, sub = tid & 15, g = tid >> 4;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * 16;
    small_front_sum<int(kSmallN / kThreads)>(first, s_part, [=](int64_t j) {
        const int64_t src = index[j];
        int64_t l = 0;
        if (src >= 0 && src < n_store) l = offsets[src + 1] - offsets[src];
        return l > 0 ? l : 0;
    });
    const int64_t i = first + g;
    const bool live = i < n;
    const int64_t src = live ? index[i] : -1;
    const bool ok = live && src >= 0 && src < n_store;
    int64_t src0 = 0, len = 0;
    if (ok) {
        src0 = offsets[src];
        len = offsets[src + 1] - src0;
        if (len < 0) len = 0;
    }
    if (sub == 0) {
        s_len[g] = len;
        if (live && !ok && first_bad) atomicMin(first_bad, static_cast<unsigned long long>(i));
    }
    __syncthreads();
    int64_t d0 = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int q = 0; q < g; ++q) d0 += s_len[q];
    if (tid == 0 && blockIdx.x == 0) out_offsets[0] = 0;
    if (!live) return;
    if (sub == 0) out_offsets[i + 1] = d0 + len;
    if (!ok || !chars || !out_chars) return;
    len = cut_at_capacity(d0, len, capacity, n, i, sub, first_bad);
    const uint8_t *sp = chars + src0;
    uint8_t *dst = out_chars + d0;
    const int64_t body = len & ~int64_t(15);
    for (int64_t p = sub * 16; p < body; p += 256)
        *reinterpret_cast<v_u32x4u *>(dst + p) = *reinterpret_cast<const v_u32x4u *>(sp + p);
    if (sub < (len & 15)) dst[body + sub] = sp[body + sub];
}

// Lists beyond kSmallN in TWO launches (round 6; rounds 2-5: three, the middle one a prefix sum by ONE workgroup walking the list in
// pieces of 1024 -- 16 384 indices of BASELINE config 5's store took 31 us, twice the encode that follows them): the `place` class of
// bsq_ragged_out.h, lists of up to 2^20 indices.  The place kernel stages the source position of its 64 sequences (and their lengths)
// in LDS next to the scan, so that index is read once.
__global__ __launch_bounds__(kThreads) void k_gather_lengths2(const int64_t *offsets, int64_t n_store, const int64_t *index, int64_t n,
                                                              int64_t *out_offsets, int64_t *wave_sums, unsigned long long *first_bad) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i == 0) out_offsets[0] = 0;
    lengths_step(i, n, out_offsets, wave_sums, [=](int64_t i) {
        const int64_t j = index[i];
        int64_t len = 0;
        if (j >= 0 && j < n_store) {
            len = offsets[j + 1] - offsets[j];
            if (len < 0) len = 0;
        } else if (first_bad) {
            atomicMin(first_bad, static_cast<unsigned long long>(i));
        }
        return len;
    });
}

__global__ __launch_bounds__(kThreads) void k_gather_place(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index,
                                                           int64_t n, int64_t *out_offsets, const int64_t *wave_sums, uint8_t *out_chars,
                                                           int64_t capacity, unsigned long long *first_bad) {
    __shared__ int64_t s_part[kThreads / 64];
    __shared__ int64_t s_src0[kPlaceS], s_d0[kPlaceS], s_len[kPlaceS];
    const int tid = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kPlaceS;
    place_offsets<false>(n, out_offsets, wave_sums, s_part, s_d0, [=](int t, int64_t i, int64_t len) {
        const int64_t src = i < n ? index[i] : -1;
        s_src0[t] = (src >= 0 && src < n_store) ? offsets[src] : -1;  // -1: nothing to copy
        s_len[t] = len;
    });
    if (!chars || !out_chars) return;
    const int sub = tid & 15;
#pragma unroll
    for (int r = 0; r < kPlaceS / (kThreads / 16); ++r) {
        const int g = r * (kThreads / 16) + (tid >> 4);
        const int64_t i = first + g;
        const int64_t src0 = s_src0[g];
        if (i >= n || src0 < 0) continue;
        const int64_t d0 = s_d0[g];
        const int64_t l = cut_at_capacity(d0, s_len[g], capacity, n, i, sub, first_bad);
        const uint8_t *sp = chars + src0;
        uint8_t *dst = out_chars + d0;
        const int64_t body = l & ~int64_t(15);
        for (int64_t p = sub * 16; p < body; p += 256)
            *reinterpret_cast<v_u32x4u *>(dst + p) = *reinterpret_cast<const v_u32x4u *>(sp + p);
        if (sub < (l & 15)) dst[body + sub] = sp[body + sub];
    }
}

}  // namespace

extern "C" {

bsq_status bsq_gather_packed_device(const uint8_t *chars, const int64_t *offsets, int64_t n_store, const int64_t *index,
                                    int64_t n, uint8_t *out_chars, int64_t out_capacity, int64_t *out_offsets,
                                    int64_t *status_dev, void *hip_stream) {
    if (!offsets || !out_offsets || n_store < 0 || n < 0 || out_capacity < 0 || (n > 0 && !index))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "bsq_gather_packed_device: null pointer or negative size");
    if ((n + kThreads - 1) / kThreads >= (int64_t(1) << 31) || (n + 15) / 16 >= (int64_t(1) << 31) || (n + kPlaceS - 1) / kPlaceS >= (int64_t(1) << 31))
        return bsq_internal::set_error(BSQ_ERR_INVALID_ARG, "index list too long");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bsq_status st = ragged_reset("gather", n, out_offsets, status_dev, s);
    if (st != BSQ_OK || n == 0) return st;
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(status_dev);
    const bool classic = bsq_internal::tuning().gather_small == 1;  // the three launches of rounds 2-5, whatever the size
    if (!classic && form_of(n) == Form::Small) {
        hipLaunchKernelGGL(k_gather_small, small_grid(n), dim3(kThreads), 0, s, chars, offsets, n_store, index, n, out_offsets, out_chars,
                           out_chars ? out_capacity : 0, bad);
        return bsq_internal::check_launch("k_gather_small");
    }
    if (!classic && form_of(n) == Form::Place)  // beyond kPlaceSumMax the gather has no scanned place: the three launches again
        return with_wave_sums(n, s, "k_gather_lengths2 / k_gather_place", [&](int64_t *sums) {
            hipLaunchKernelGGL(k_gather_lengths2, lengths_grid(n), dim3(kThreads), 0, s, offsets, n_store, index, n, out_offsets, sums, bad);
            hipLaunchKernelGGL(k_gather_place, place_grid(n), dim3(kThreads), 0, s, chars, offsets, n_store, index, n, out_offsets,
                               static_cast<const int64_t *>(sums), out_capacity > 0 ? out_chars : nullptr, out_capacity, bad);
        });
    hipLaunchKernelGGL(k_gather_lengths, lengths_grid(n), dim3(kThreads), 0, s, offsets, n_store, index, n, out_offsets, bad);
    hipLaunchKernelGGL(k_gather_scan, dim3(1), dim3(1024), 0, s, out_offsets + 1, n);
    if (chars && out_chars && out_capacity > 0)
        hipLaunchKernelGGL(k_gather_chars, small_grid(n), dim3(kThreads), 0, s, chars, offsets, n_store, index, n, out_offsets, out_chars,
                           out_capacity, bad);
    return bsq_internal::check_launch("k_gather_*");
}

}  // extern "C"
