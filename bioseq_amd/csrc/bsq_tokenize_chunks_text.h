// A FRAGMENT of a function body, not a header: the statements of the (B,P) / (B,C,P) chunk-stream kernel (no include guard: it is meant to
// be included twice; the design notes are in bsq_tokens.hip, above k_tokenize_chunks).
// Expects in scope: the template parameters T, NT, HOT, NCH, RG;  uint32_t blk, the block of one batch's grid;  const int8_t *plut, the
// 256-entry alphabet table;  p, a TParams or a TFields;  and what bsq_tokens.hip declares before it (ChunkState, UBytes, bsq_tiles.h).
// Included by k_tokenize_chunks (blk = blockIdx.x, plut = p.lut) and by tokenize_chunks_body, which k_tokenize_chunks_multi calls.
    __shared__ __align__(16) uint8_t s_lut4[4][256];
    constexpr int SZ = static_cast<int>(sizeof(T));
    constexpr int EPL = 16 / SZ;  // elements (= characters) per lane per store
    using State = ChunkState<T, HOT>;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t *lut = s_lut4[wave];
    {   // wave-private table: token VALUES (unmapped / >= 0x80 -> 0, the memset value of tokenize.h:427),
        // or raw ids with kNone for the one-hot mode
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane * 4 + q;
            const int8_t v = plut[idx];
            const uint32_t e = (idx < 128 && v >= 0) ? static_cast<uint32_t>(v) : (HOT ? kNone : 0u);
            w |= e << (8 * q);
        }
        reinterpret_cast<uint32_t *>(lut)[lane] = w;
    }
    const int64_t nrows = HOT ? p.B * p.C : p.B;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);  // scalar: chunk-level arithmetic stays on the SALU
    // chunks of this wave: class = blockIdx % 8 (pinned to the XCD), NCH consecutive slots of that class
    const int64_t slot0 = (static_cast<int64_t>(blk >> 3) * 4 + wave_s) * NCH;
    const int64_t k0 = static_cast<int64_t>(blk & 7u) + 8 * slot0;
    if (k0 >= p.nchunks) return;
    const int64_t total_chars = p.offsets[p.B];
    const uint32_t Pu = static_cast<uint32_t>(p.P), PPR = p.ppr;
    const bool has_mask = HOT && p.mask != nullptr;
    const bool small = nrows * int64_t(PPR) < (int64_t(1) << 31) && !p.wide_index;  // 32-bit piece indices: divide by reciprocal

    // stage A: (row, position) of the lane's four stores -- element e0 + u*EPS with e0 = lo/SZ + lane*EPL -- without a
    // per-lane division (the chunk's first element is wave-uniform, the lane's share adds < 1024 positions, the
    // stores advance by (step_q, step_r)) -- and the offsets of their sequences (8 independent loads).
    auto stage_a = [&](State &c, int64_t k) {
        c.valid = k < p.nchunks;
        if (!c.valid) return;
        c.lo = k * kChunk;  // !RG: chunks are relative to `out` (16-byte aligned)
        const int64_t g0 = k * (kChunk / 16);  // first piece of the chunk
        uint32_t tc;
        if (small) {
            const uint32_t q = fast_div(static_cast<uint32_t>(g0), p.magic, p.shift, p.pow2);
            c.bc = q;
            tc = static_cast<uint32_t>(g0) - q * PPR;
        } else {
            c.bc = g0 / PPR;
            tc = static_cast<uint32_t>(g0 - c.bc * PPR);
        }
        const uint32_t tl = tc + static_cast<uint32_t>(lane);  // < ppr + 64
        const uint32_t ql = fast_div(tl, p.magic, p.shift, p.pow2);
        int64_t bu = c.bc + ql;
        uint32_t tu = tl - ql * PPR;  // piece of the row
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t b = bu;  // row of the flat matrix
            c.t0[u] = static_cast<int32_t>(tu * EPL);
            c.row[u] = b;
            c.live[u] = b < nrows;
            if constexpr (RG) {
                // the row starts `sm` elements into a 16-byte line of the output: head = the elements up to the next line
                const uint32_t sm = (p.a0e + (static_cast<uint32_t>(b) & (EPL - 1)) * p.pmod) & (EPL - 1);
                const int32_t h = static_cast<int32_t>((EPL - sm) & (EPL - 1));
                const int32_t t0 = tu == 0 ? 0 : h + static_cast<int32_t>(tu - 1) * EPL;
                const int32_t left = static_cast<int32_t>(Pu) - t0;
                c.t0[u] = t0;
                c.cnt[u] = tu == 0 ? (h < left ? h : left) : (left > EPL ? EPL : left);
                c.live[u] = c.live[u] && c.cnt[u] > 0;
            }
            b = c.live[u] ? b : nrows - 1;
            c.chan[u] = 0;
            if constexpr (HOT) {  // row = sequence * C + channel
                int64_t seq;
                if (nrows < (int64_t(1) << 31) && !p.wide_index)  // wave-uniform
                    seq = fast_div(static_cast<uint32_t>(b), p.magic_c, p.shift_c, p.pow2_c);
                else
                    seq = b / p.C;
                c.chan[u] = static_cast<uint32_t>(b - seq * p.C);
                b = seq;
            }
            c.start[u] = p.offsets[b];
            c.stop[u] = p.offsets[b + 1];
            bu += p.step_q;
            tu += p.step_r;
            if (tu >= PPR) {
                tu -= PPR;
                bu += 1;
            }
        }
    };

    // stage B: the characters.  Loads are UNCONDITIONAL (lanes that must not touch their own address read the
    // first bytes of the window instead) so that all four are in flight together.  Addresses are 32-bit
    // offsets from a wave-uniform base: the rows of a chunk are consecutive sequences, their characters lie
    // within 2^31 bytes of the first one's (off0), so "is [a, a + EPL) inside the buffer" is one unsigned
    // compare of (rel - lo_b) against span, and the load takes the scalar-base + 32-bit-offset form.
    auto stage_b = [&](State &c) {
        if (!c.valid) return;
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // lengths from the low words (a valid length is < 2^31; else clamped to `room`)
            const uint32_t len = static_cast<uint32_t>(c.stop[u]) - static_cast<uint32_t>(c.start[u]);
            c.L[u] = static_cast<int32_t>(len > static_cast<uint32_t>(p.room) ? static_cast<uint32_t>(p.room) : len);
        }
        int64_t seq0 = c.bc;
        if constexpr (HOT)
            seq0 = (nrows < (int64_t(1) << 31) && !p.wide_index) ? int64_t(fast_div(static_cast<uint32_t>(c.bc), p.magic_c, p.shift_c, p.pow2_c))
                                                : c.bc / p.C;
        const int64_t off0 = p.offsets[seq0];
        const int64_t lo_b64 = -off0, hi_b64 = total_chars - off0 - EPL;  // valid range of a vector's first byte, relative to off0
        const bool can_vec = hi_b64 >= lo_b64;                            // wave-uniform (the buffer holds >= EPL bytes)
        const int32_t lo_b = lo_b64 < INT32_MIN ? INT32_MIN : static_cast<int32_t>(lo_b64);
        const int32_t hi_b = hi_b64 > INT32_MAX ? INT32_MAX : (hi_b64 < lo_b ? lo_b : static_cast<int32_t>(hi_b64));
        const uint32_t span = static_cast<uint32_t>(hi_b) - static_cast<uint32_t>(lo_b);
        uint32_t uoff[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t j0 = c.t0[u] - p.bos;
            const uint32_t rel = static_cast<uint32_t>(c.start[u]) - static_cast<uint32_t>(off0) + static_cast<uint32_t>(j0);
            const uint32_t d = rel - static_cast<uint32_t>(lo_b);  // offset from the lowest valid address
            const bool need = c.live[u] && j0 < c.L[u] && j0 + EPL > 0;
            const bool fast = can_vec && need && d <= span;
            c.slow[u] = need && !fast;
            uoff[u] = fast ? d : 0u;
        }
        if (can_vec) {
            const uint8_t *cbase = p.chars + (off0 + lo_b);  // wave-uniform, inside the buffer
#pragma unroll
            for (int u = 0; u < 4; ++u) c.cw[u] = *reinterpret_cast<const UBytes<EPL> *>(cbase + uoff[u]);
            if (has_mask) {
                const uint8_t *mbase = p.mask + (off0 + lo_b);
#pragma unroll
                for (int u = 0; u < 4; ++u) c.mw[u] = *reinterpret_cast<const UBytes<EPL> *>(mbase + uoff[u]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) c.cw[u].clear();
        }
    };

    // stage C: the rare byte-wise edge reads, then LUT lookups packed 4 (or 2) per word with BOS / EOS / PAD folded in
    // as word masks, and the four 16-byte stores.
    constexpr int WB = EPL >= 4 ? 4 : EPL;  // characters per word
    const uint32_t ones = WB == 4 ? 0x01010101u : 0x0101u;
    const uint32_t fill_v = (!HOT && p.fill_id == kNone) ? 0u : p.fill_id;
    const uint32_t at_len_v = (!HOT && p.at_len_id == kNone) ? 0u : p.at_len_id;
    const uint32_t fill_w = fill_v * ones, at_len_w = at_len_v * ones;
    const T hot_one = static_cast<T>(p.one_bits);
    auto stage_c = [&](State &c) {
        if (!c.valid) return;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c.slow[u]) {  // first / last bytes of the buffer: never read outside it
                const int32_t j0 = c.t0[u] - p.bos;
                c.cw[u].clear();
                if (has_mask) c.mw[u].clear();
#pragma unroll
                for (int i = 0; i < EPL; ++i)
                    if (j0 + i >= 0 && j0 + i < c.L[u]) {
                        c.cw[u].set_byte(i, p.chars[c.start[u] + j0 + i]);
                        if (has_mask) c.mw[u].set_byte(i, p.mask[c.start[u] + j0 + i]);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!c.live[u]) continue;
            const int32_t j0 = c.t0[u] - p.bos;
            alignas(16) T vals[EPL];
            uint32_t packed[EPL / WB];
#pragma unroll
            for (int q = 0; q < EPL / WB; ++q) {
                uint32_t w = 0;
#pragma unroll
                for (int i = 0; i < WB; ++i) {
                    uint32_t tk = lut[c.cw[u].byte(q * WB + i)];
                    if (has_mask && c.mw[u].byte(q * WB + i) == 0) tk = kNone;
                    w |= tk << (8 * i);
                }
                const int32_t jf = j0 + q * WB;  // character index of the word's first byte
                const int32_t nv = c.L[u] - jf;  // characters of the sequence left from there
                // Branch-free (nearly every wave holds a lane that straddles or lies beyond L): the first nvc bytes stay,
                // the rest is fill, byte nv (if it is one of this word's) is the token at position bos + L.
                const int32_t nvc = nv < 0 ? 0 : (nv > WB ? WB : nv);
                const uint32_t keep = static_cast<uint32_t>(uint64_t(1) << (8 * nvc)) - 1u;  // low nvc bytes (nvc = 4: all)
                w = (w & keep) | (fill_w & ~keep);
                const uint32_t at = static_cast<uint32_t>(nv) < static_cast<uint32_t>(WB) ? (0xFFu << (8 * nvc)) : 0u;
                w = (w & ~at) | (at_len_w & at);
                if (q == 0 && jf < 0) w = (w & ~0xFFu) | p.bos_id;  // position 0 with BOS (j0 >= -1: only the first word)
                packed[q] = w;
                if constexpr (HOT || SZ != 1) {
#pragma unroll
                    for (int i = 0; i < WB; ++i) {
                        const uint32_t tk = (w >> (8 * i)) & 0xFFu;
                        if constexpr (HOT)
                            vals[q * WB + i] = tk == c.chan[u] ? hot_one : T(0);
                        else
                            vals[q * WB + i] = id_as<T>(tk);
                    }
                }
            }
            uint4 o;
            if constexpr (!HOT && SZ == 1)  // 8-bit tokens: the packed words ARE the 16 output bytes
                o = uint4{packed[0], packed[1], packed[2], packed[3]};
            else
                o = *reinterpret_cast<const uint4 *>(vals);
            if constexpr (!RG) {
                store16<NT>(p.out + c.lo + u * 1024 + lane * 16, o);
            } else {
                uint8_t *dst = p.out + (c.row[u] * p.P + c.t0[u]) * SZ;
                // (skipping the partial stores when no lane of the wave holds a head / tail -- a ballot -- measured 2-7 %
                // slower: profiles/r02/cliff_lab5.txt vs cliff_lab6.txt)
                if (c.cnt[u] == EPL) store16<NT>(dst, o);  // a whole piece: 16-byte aligned by construction
                else store_head_bytes_var<SZ>(dst, o, static_cast<uint32_t>(c.cnt[u]) * SZ);
            }
        }
    };

    State st[NCH];
    stage_a(st[0], k0);
    if constexpr (NCH > 1) stage_a(st[1], k0 + 8);
    stage_b(st[0]);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (j + 1 < NCH) stage_b(st[j + 1]);
        if (j + 2 < NCH) stage_a(st[j + 2], k0 + 8 * (j + 2));
        stage_c(st[j]);
    }
