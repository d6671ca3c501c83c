// A FRAGMENT of a function body, not a header: the statements of the chunk-owner one-hot kernel (no include guard: it is meant to be
// included twice; the design notes are in bsq_onehot.hip, above CFields).
// Expects in scope: the template parameters ST, NT;  uint32_t blk, the block of one batch's grid;  const int8_t *plut, the 256-entry
// alphabet table;  p, a CParams or a CFields;  and what bsq_tiles.h declares.
// Included by k_onehot_chunks (blk = blockIdx.x, plut = p.lut) and by onehot_chunks_body, which k_onehot_chunks_multi calls.
    __shared__ __align__(16) uint8_t s_img[4][kChunk];
    __shared__ __align__(16) uint8_t s_lut4[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t *img = s_img[wave];
    uint8_t *lut = s_lut4[wave];
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<uint4 *>(img + u * 1024 + lane * 16) = uint4{0, 0, 0, 0};
    {   // wave-private copy of the alphabet table (unmapped / >= 0x80 -> kNone): no workgroup barrier needed
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane * 4 + q;
            const int8_t v = plut[idx];
            const uint32_t e = (idx < 128 && v >= 0) ? static_cast<uint32_t>(v) : kNone;
            w |= e << (8 * q);
        }
        reinterpret_cast<uint32_t *>(lut)[lane] = w;
    }
    const int32_t cls = static_cast<int32_t>(blk & 7u);
    const int64_t group = static_cast<int64_t>(blk >> 3);
    const int32_t rowbytes = p.C * static_cast<int32_t>(sizeof(ST));
    const ST one = static_cast<ST>(p.one_bits);
    int64_t j = (group * 4 + wave) * p.cpw;
    for (int32_t it = 0; it < p.cpw; ++it, ++j) {
        const int64_t k = cls + 8 * j;
        if (k >= p.nchunks) break;  // wave-uniform
        int64_t lo = k * kChunk - p.head, hi = lo + kChunk;
        if (lo < 0) lo = 0;
        if (hi > p.total) hi = p.total;
        const int32_t len = static_cast<int32_t>(hi - lo);
        int64_t skip64, b_lo;
        const int64_t r_lo = div_by(lo, rowbytes, p.inv_rowbytes, &skip64);
        const int32_t skip = static_cast<int32_t>(skip64);
        const int32_t nr = static_cast<int32_t>(fast_div(static_cast<uint32_t>(skip + len + rowbytes - 1), p.rb_magic,
                                                         p.rb_shift, p.rb_pow2));
        const int64_t t_lo = div_by(r_lo, p.B, p.inv_B, &b_lo);
        for (int32_t i0 = 0; i0 < nr; i0 += 64) {
            const int32_t i = i0 + lane;
            if (i < nr) {
                int64_t b = b_lo + i, t = t_lo;
                if (b >= p.B) {  // the chunk runs over the end of position t's rows
                    const int64_t q = b / p.B;
                    t += q;
                    b -= q * p.B;
                }
                uint32_t tk;
                const int64_t start = p.offsets[b];
                int64_t L = p.offsets[b + 1] - start;
                L = L > p.room ? p.room : L;
                const int64_t jj = t - p.bos;
                if (jj < 0) {
                    tk = p.bos_id;
                } else if (jj < L) {
                    tk = lut[p.chars[start + jj]];
                    if (p.mask && p.mask[start + jj] == 0) tk = kNone;
                } else {
                    tk = (jj == L) ? p.at_len_id : p.fill_id;
                }
                const int32_t pos = i * rowbytes - skip + static_cast<int32_t>(tk) * static_cast<int32_t>(sizeof(ST));
                if (tk != kNone && pos >= 0 && pos < len) *reinterpret_cast<ST *>(img + pos) = one;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint8_t *g = p.out + lo;
        if (len == kChunk) {
            const uint4 v0 = *reinterpret_cast<const uint4 *>(img + lane * 16);
            const uint4 v1 = *reinterpret_cast<const uint4 *>(img + 1024 + lane * 16);
            const uint4 v2 = *reinterpret_cast<const uint4 *>(img + 2048 + lane * 16);
            const uint4 v3 = *reinterpret_cast<const uint4 *>(img + 3072 + lane * 16);
            store16<NT>(g + lane * 16, v0);
            store16<NT>(g + 1024 + lane * 16, v1);
            store16<NT>(g + 2048 + lane * 16, v2);
            store16<NT>(g + 3072 + lane * 16, v3);
        } else {
            for (int32_t o = lane * static_cast<int32_t>(sizeof(ST)); o < len; o += 64 * static_cast<int32_t>(sizeof(ST)))
                *reinterpret_cast<ST *>(g + o) = *reinterpret_cast<const ST *>(img + o);
        }
        if (it + 1 < p.cpw) {  // image is reused: wipe it (wave-private, in-order LDS)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<uint4 *>(img + u * 1024 + lane * 16) = uint4{0, 0, 0, 0};
        }
    }
