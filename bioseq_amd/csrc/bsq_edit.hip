// Edit distance of row pairs on the device (include/bsq.h, "edit distance of row pairs"): k_edit_pairs<G>, G = 4, 16 or 64 lanes per
// pair, a wave holds 64 / G pairs and a workgroup four waves that never meet after the byte table is staged.
//
// The shorter row of a pair is the pattern, cut into blocks of 64 characters; lane b of the pair's group owns block b: its vertical
// deltas Pv, Mv in registers and its column of the pair's match table in LDS -- tab[class][lane], one 64-bit word per class with bit i
// set where pattern character 64 b + i has that class.  A lane reads and writes its own column only (plain read-modify-write, no
// atomic, no barrier), and consecutive lanes read consecutive words.
// The longer row is the text.  The group walks the anti-diagonals of the (block, column) grid: at step t lane b takes column t - b
// through the block step of bsq_edit_dev.h, so a group runs n + blocks - 1 steps.  What a lane needs for a column -- its class and
// the horizontal delta that left the block below -- is one 32-bit value that moves up one lane per step.  The text is fetched G
// characters at a time, a byte per lane, one tile ahead of its use, and mapped to classes once; lane 0 of the group takes the class of
// column t from lane t % G of the tile.  Both movements are ONE ds_bpermute per step: a lane offers (tile class << 16) | (class,
// delta) and reads either its lower neighbour or, as lane 0, the tile's lane.  No lane issues a global load that the step waits for,
// none reads a character twice.
// A wave runs until its slowest group is done; a lane outside its columns keeps its state (the update is a select, so no lane is
// switched off around the cross-lane read).  No global atomic, no waiting on other waves.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsq.h"
#include "bsq_device.h"
#include "bsq_edit_dev.h"
#include "bsq_internal.h"
#include "bsq_row_table.h"

namespace {

using bsq_dev::kThreads;

struct EditParams {
    const uint8_t *chars_a, *chars_b;
    const int64_t *offsets_a, *offsets_b;
    const int64_t *row, *col;
    int32_t *dist;
    int64_t Ba, Bb, n_pairs;
    int32_t max_len, nchars;
    int8_t lut[256];
};

template <int G>
__global__ __launch_bounds__(kThreads) void k_edit_pairs(const EditParams p) {
    extern __shared__ __align__(16) uint64_t s_dyn[];  // four waves' tables of classes x 64 words, then the 256 classes of the bytes
    const int32_t C = p.nchars + 1;
    uint8_t *s_cls = reinterpret_cast<uint8_t *>(s_dyn + static_cast<size_t>(kThreads) * C);
    s_cls[threadIdx.x] = static_cast<uint8_t>(bsq_editd::class_of(p.lut, p.nchars, static_cast<uint8_t>(threadIdx.x)));  // (kThreads == 256)
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = lane & (G - 1), base = lane & ~(G - 1);
    uint64_t *tab = s_dyn + static_cast<size_t>(wave) * 64 * C + lane;  // tab[c * 64]: this lane's word of class c
    const int64_t k = (static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + wave) * (64 / G) + lane / G;

    // the pair of this lane's group: its pattern (m characters, nb blocks) and text (n characters); steps = 0: nothing to walk
    const uint8_t *pat = nullptr, *text = nullptr;
    int64_t pat_at = 0, pat_total = 0;
    uint32_t m = 0, n = 0, nb = 0, steps = 0;
    int32_t code = 0;  // what lane 0 writes when the group walks nothing
    bool live = false;
    if (k < p.n_pairs) {
        const int64_t i = p.row[k], j = p.col[k];
        if (i < 0 || i >= p.Ba || j < 0 || j >= p.Bb) {
            code = BSQ_EDIT_BAD_INDEX;
        } else {
            const int64_t sa = p.offsets_a[i], sb = p.offsets_b[j];
            int64_t la = p.offsets_a[i + 1] - sa, lb = p.offsets_b[j + 1] - sb;
            la = la < 0 ? 0 : la;
            lb = lb < 0 ? 0 : lb;
            const bool a_short = la <= lb;
            const int64_t mm = a_short ? la : lb, nn = a_short ? lb : la;
            if (mm > p.max_len || nn > bsq_editd::kMaxLong) {
                code = BSQ_EDIT_TOO_LONG;
            } else if (mm == 0) {
                code = static_cast<int32_t>(nn);
            } else {
                live = true;
                m = static_cast<uint32_t>(mm), n = static_cast<uint32_t>(nn), nb = (m + 63) >> 6;
                steps = n + nb - 1;
                pat = a_short ? p.chars_a : p.chars_b;
                pat_at = a_short ? sa : sb;
                pat_total = a_short ? p.offsets_a[p.Ba] : p.offsets_b[p.Bb];
                text = a_short ? p.chars_b + sb : p.chars_a + sa;
            }
        }
        if (!live && b == 0) p.dist[k] = code;
    }
    uint32_t wave_steps = steps;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const uint32_t o = __shfl_xor(wave_steps, x);
        wave_steps = o > wave_steps ? o : wave_steps;
    }
    wave_steps = __builtin_amdgcn_readfirstlane(wave_steps);
    if (wave_steps == 0) return;  // (no workgroup barrier follows)

    // this lane's column of the table: the classes of pattern characters 64 b .. 64 b + 63
    for (int32_t c = 0; c < C; ++c) tab[c * 64] = 0;
    if (live && static_cast<uint32_t>(b) < nb) {
        const int32_t mine = static_cast<int32_t>(m) - 64 * b < 64 ? static_cast<int32_t>(m) - 64 * b : 64;
        for (int q = 0; q < 4; ++q) {
            if (16 * q >= mine) break;
            uint32_t w[4];
            bsq_rowtab::load16(pat, pat_at + 64 * b + 16 * q, pat_total, mine - 16 * q, w);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (16 * q + c < mine) tab[s_cls[(w[c >> 2] >> (8 * (c & 3))) & 0xFFu] * 64] |= uint64_t(1) << (16 * q + c);
        }
    }

    const uint32_t top = static_cast<uint32_t>(b) + 1 == nb ? (m - 1) & 63u : 63u;
    const int src = b == 0 ? base : lane - 1;  // (lane 0 of a group adds t % G)
    uint64_t pv = ~uint64_t(0), mv = 0;
    int32_t score = static_cast<int32_t>(m);
    // a text tile: column T + b of the tile that starts at T, as a byte ahead of its use and as a class while in use
    auto fetch = [&](uint32_t at) -> uint32_t { return at < n ? text[at] : 0u; };  // (n == 0 for a lane without a text)
    uint32_t ahead = fetch(b), tile = 0, out = 0;
    for (uint32_t t = 0; t < wave_steps; ++t) {
        if ((t & (G - 1)) == 0) {  // (uniform)
            tile = s_cls[ahead];
            ahead = fetch(t + G + b);
        }
        const uint32_t got = __shfl((tile << 16) | out, b == 0 ? src + static_cast<int>(t & (G - 1)) : src);
        const uint32_t cls = b == 0 ? got >> 16 : (got >> 2) & 0x3FFFu;
        const int32_t hin = b == 0 ? 1 : static_cast<int32_t>(got & 3u) - 1;
        uint64_t npv = pv, nmv = mv;
        const int32_t hout = bsq_editd::block_step(npv, nmv, tab[cls * 64], hin, top);
        const bool on = t >= static_cast<uint32_t>(b) && t - b < n && static_cast<uint32_t>(b) < nb;
        pv = on ? npv : pv;
        mv = on ? nmv : mv;
        score += on ? hout : 0;
        out = (cls << 2) | static_cast<uint32_t>(hout + 1);
    }
    if (live && static_cast<uint32_t>(b) + 1 == nb) p.dist[k] = score;
}

template <int G>
void launch(const EditParams &p, hipStream_t s) {
    const int64_t per_group = (kThreads / 64) * (64 / G);
    const size_t lds = static_cast<size_t>(kThreads) * (p.nchars + 1) * sizeof(uint64_t) + 256;
    hipLaunchKernelGGL(k_edit_pairs<G>, dim3(static_cast<unsigned>((p.n_pairs + per_group - 1) / per_group)), dim3(kThreads), lds, s, p);
}

}  // namespace

extern "C" {

bsq_status bsq_edit_pairs_device(const bsq_desc *d, const uint8_t *chars_a, const int64_t *offsets_a, int64_t Ba, const uint8_t *chars_b,
                                 const int64_t *offsets_b, int64_t Bb, const int64_t *row, const int64_t *col, int64_t n_pairs, const bsq_edit *e,
                                 int32_t *dist, void *hip_stream) {
    const char *why = "";
    int32_t lanes = 0;
    const bsq_status st = bsq_editd::check(d, chars_a, offsets_a, Ba, chars_b, offsets_b, Bb, row, col, n_pairs, e, dist, &lanes, &why);
    if (st != BSQ_OK) return bsq_internal::set_error(st, why);
    if (n_pairs == 0) return BSQ_OK;
    EditParams p;
    p.chars_a = chars_a, p.chars_b = chars_b, p.offsets_a = offsets_a, p.offsets_b = offsets_b;
    p.row = row, p.col = col, p.dist = dist;
    p.Ba = Ba, p.Bb = Bb, p.n_pairs = n_pairs;
    p.max_len = e ? e->max_len : bsq_editd::kMaxLen, p.nchars = d->nchars;
    for (int c = 0; c < 256; ++c) p.lut[c] = d->lut[c];
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (lanes == 4) launch<4>(p, s);
    else if (lanes == 16) launch<16>(p, s);
    else launch<64>(p, s);
    return bsq_internal::check_launch(bsq_editd::kernel_name(lanes));
}

}  // extern "C"
