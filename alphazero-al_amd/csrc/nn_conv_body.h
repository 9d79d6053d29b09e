// nn_conv_body.h - the text of the kernels of nn_conv.hip, included as the body of each of them (not a header in the
// usual sense: no declarations of its own).  The including kernel provides CIN, NORM, RESID, EMBED, STEM, CHAINED as constant
// expressions and x, w, bias, gamma, beta, y, B, eps, dbg, batch_dev, em (EmbedIn), st (StemIn) as variables.
//
// STEM (C_in 64, normalised, residual only): the raw tile is not staged from HBM; wave s computes the folded stem of
// sample s into it (P0) - the bits k_stem (nn_stem.hip) would have stored, in the slots stage_tile would have filled.
// Everything from P1 on is the same text for every kernel, and a kernel without STEM compiles to what it was before
// P0 existed (the text is included, not called: no inlining decision sits between the kernel and its body).
    static_assert(!EMBED || (CIN == 32 && !NORM && !RESID), "the embedding is fused into the stem only");
    static_assert(!STEM || (CIN == 64 && NORM && RESID && !EMBED), "the folded stem is fused into the first residual block only");
    constexpr int NRAW = STEM ? 1 : 2;            // raw buffers: nothing to prefetch from HBM when the tile is computed here
    const int64_t rows_total = B;                                     // rows of the feature tensor a gather index may name
    if (batch_dev != nullptr && *batch_dev < B) B = *batch_dev;       // compact batch whose size only the device knows
    constexpr int K = 9 * CIN;
    constexpr int KSTEPS = K / 32;                // 18 (C_in 64) or 9 (C_in 32)
    constexpr int KPT = CIN / 32;                 // k steps per tap
    constexpr int VPC = CIN / 8;                  // 16-byte vectors per input cell
    constexpr int VPS = CELLS * VPC;              // vectors per input sample
    constexpr int PER = (VPS + 63) / 64;          // vectors per lane of a sample's wavefront
    constexpr int SB = VPS * 16;                  // bytes per raw sample
    constexpr int OVPS = CELLS * COUT / 8;        // vectors per output sample
    constexpr int OPER = (OVPS + 63) / 64;
    constexpr int OSB = OVPS * 16;                // bytes per output sample
    // Lane l of a sample's wavefront owns vectors l, l + 64, ...: only the LAST one can lie past the sample, and only in
    // the lanes from LASTN (OLASTN) on - 16 of 64 at 64 channels (5 * 64 + 16 = 336), 40 of 64 at 32 (2 * 64 + 40 = 168)
    constexpr int LASTN = VPS - 64 * (PER - 1), OLASTN = OVPS - 64 * (OPER - 1);
    static_assert(LASTN > 0 && LASTN < 64 && OLASTN > 0 && OLASTN < 64 && (PER == 6 || PER == 3), "stage_sample's two forms");

    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t *img = smem;                                          // TS * PCELLS * CELLB, swizzled
    uint8_t *rawb = smem + TS * PCELLS * CELLB;                   // 2 x TS x SB: raw tiles, double buffered (STEM: one)
    uint8_t *outs = rawb + NRAW * TS * SB;                        // TS x OSB output tile (unless RESID: in place)
    // (no static __shared__ objects: the image must sit at LDS address 0 for the compiler to
    // fold the window's row displacements into the ds_read offset fields)
    float *s_gam = reinterpret_cast<float *>(outs + (RESID ? 0 : TS * OSB)), *s_bet = s_gam + CIN;
    uint8_t *dump = reinterpret_cast<uint8_t *>(s_gam + 2 * CIN);         // 4 x 8 x 16 B: results of dummy tokens
    uint8_t *s_pm = dump + 512, *s_fr = s_pm + PMAPB;                     // STEM: pmap and the table fragments

    // CHAINED (an inclusion behind another one in the same kernel): the thread id as an opaque copy, so that nothing
    // this inclusion derives from it is one value with the earlier inclusion's and kept in registers across that one's
    // tile loop, where the resident weights leave no room for it
    int tid = threadIdx.x;
    if (CHAINED) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mh = wave & 1, th = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;

    // ---- weights: this wave's A fragments, resident for the whole kernel.  MFMA row r of m tile
    // mt stands for output channel 32*mh + 8*(r>>2) + 4*mt + (r&3): with the C layout (rows
    // 4*(lane>>4)+reg) a lane then ends up with EIGHT CONSECUTIVE channels of its token - chunk
    // 4*mh + (lane>>4) - i.e. one 16-byte vector of the output row.
    bf16x8 aw[2][KSTEPS];
    float bia[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int o = mh * 32 + (l15 >> 2) * 8 + mt * 4 + (l15 & 3);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            aw[mt][s] = *reinterpret_cast<const bf16x8 *>(w + static_cast<size_t>(o) * K + s * 32 + l4 * 8);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            bia[mt][r] = __uint_as_float(static_cast<uint32_t>(bias[mh * 32 + l4 * 8 + mt * 4 + r]) << 16);
    }
    if (NORM && tid < CIN) {
        s_gam[tid] = __uint_as_float(static_cast<uint32_t>(gamma[tid]) << 16);
        s_bet[tid] = __uint_as_float(static_cast<uint32_t>(beta[tid]) << 16);
    }
    // ---- zero the padded images (the halo is never written again) and the raw buffers (slots
    // of samples past the batch are never filled)
    {
        V8 z; z.w[0] = z.w[1] = z.w[2] = z.w[3] = 0;
        constexpr int NV = (TS * PCELLS * CELLB + NRAW * TS * SB) / 16;
        for (int i = tid; i < NV; i += 256) reinterpret_cast<V8 *>(smem)[i] = z;
    }
    if (STEM) {
        for (int i = tid; i < PMAPB / 16; i += 256) reinterpret_cast<V8 *>(s_pm)[i] = reinterpret_cast<const V8 *>(st.pmap)[i];
        for (int i = tid; i < FRAGB / 16; i += 256) reinterpret_cast<V8 *>(s_fr)[i] = reinterpret_cast<const V8 *>(st.wfrag)[i];
    }
    __syncthreads();

    // Raw tiles go from HBM straight into LDS (global_load_lds_dwordx4: no registers held while
    // the previous tile is multiplied).  Wave s stages sample s; an instruction fills 1 KiB in
    // lane order, so slot j of a sample holds cell j / VPC; within a 64-channel cell the chunk
    // order is XORed with (cell & 7) through the SOURCE address.  That is also the layout of the
    // output tile, so the residual block updates the raw tile in place, and it leaves every
    // lane with one fixed channel chunk in P1.
    auto swz_in = [](int cell) { return VPC == 8 ? (cell & 7) : 0; };
    // The same layout seen from a lane (l < 64): vector l + 64 i of a sample is cell l / VPC + (64 / VPC) i - a multiple
    // of 8 cells on, so the key does not depend on i - and sits tok_off(l) + 1024 i bytes into the sample, in HBM on
    // either side of the kernel; in LDS (lane order) it is at 16 l + 1024 i.
    auto tok_off = [](uint32_t l, int vpc) { return vpc == 8 ? ((l >> 3) << 7) | (((l & 7) ^ ((l >> 3) & 7)) << 4) : l << 4; };
    const uint32_t raw_lds = lds_addr(rawb);
    if (EMBED) {                                   // the raw buffers are free: the position table lives there
        for (int i = tid; i < CELLS * CIN / 8; i += 256)
            reinterpret_cast<V8 *>(rawb)[i] = reinterpret_cast<const V8 *>(em.pos)[i];
        __syncthreads();
    }
    auto stage_tile = [&](int64_t tile, int buf, uint32_t lane) {
        const int64_t b = tile * TS + wave;
        if (EMBED || STEM || b >= B) return;
        // one statement for the sample: its base in SGPRs, one offset per lane, 1024 i in the offset fields; the last
        // vector in lanes 0 .. LASTN - 1 only (another lane would read past the sample and write the next wave's slot)
        stage_sample<PER>(x + b * (CELLS * CIN), tok_off(lane, VPC), raw_lds + (buf * TS + wave) * SB, (1ull << LASTN) - 1);
    };

    const int64_t ntiles = (B + TS - 1) / TS;
    // EMBED: the two planes of this wave's sample at this lane's cells, one tile ahead
    float pl_own[PER], pl_opp[PER];
    auto load_planes = [&](int64_t tile, uint32_t lane) {
        const int64_t b = tile * TS + wave;
        const bool live = b < B;
        int64_t row = !live ? 0 : (em.gather != nullptr ? em.gather[b] : b);
        if (row < 0 || row >= rows_total) row = 0;                    // never dereference an index outside the rows
        if (em.features != nullptr) {
            const float *fs = em.features + row * (3 * CELLS);
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const uint32_t s = lane + 64 * i;
                const bool ok = live && s < VPS;
                pl_own[i] = ok ? fs[s / VPC] : 0.0f;
                pl_opp[i] = ok ? fs[CELLS + s / VPC] : 0.0f;
            }
        } else {
            // the planes MCTS_cpp.py:15-20 builds from the (symmetrised) grid, straight from the bitboards
            const bool p1 = em.turn[row] > 0, mir = em.sym[row] != 0;
            const uint64_t own = p1 ? em.bb_p1[row] : em.bb_p2[row], opp = p1 ? em.bb_p2[row] : em.bb_p1[row];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const uint32_t s = lane + 64 * i;
                const bool ok = live && s < VPS;
                const int cell = ok ? s / VPC : 0;
                const int r = cell / COLS, c = cell - r * COLS;
                const int bit = (mir ? COLS - 1 - c : c) * 7 + (5 - r);
                pl_own[i] = (ok && ((own >> bit) & 1ull)) ? 1.0f : 0.0f;
                pl_opp[i] = (ok && ((opp >> bit) & 1ull)) ? 1.0f : 0.0f;
            }
        }
    };
    // STEM: the position of this wave's sample, one tile ahead, in ONE register - lanes 0..5 hold the dwords of the
    // two bitboards, the side to move and the symmetry id (the sample is wave-uniform: read back with v_readlane
    // when the tile is computed); the compact row index it depends on is requested two tiles ahead
    auto request_row = [&](int64_t tile) {
        const int64_t b = tile * TS + wave;
        int32_t r = 0;
        if (tile < ntiles && b < B && st.gather != nullptr) r = st.gather[b];
        return r;
    };
    auto request_pos = [&](int64_t tile, int32_t rowv, uint32_t lane) {
        const int64_t b = tile * TS + wave;
        uint32_t v = 0;
        if (tile < ntiles && b < B) {
            int64_t row = st.gather != nullptr ? static_cast<int64_t>(__builtin_amdgcn_readfirstlane(rowv)) : b;
            if (row < 0 || row >= rows_total) row = 0;                    // never dereference an index outside the rows
            const uint32_t *p1 = reinterpret_cast<const uint32_t *>(st.bb_p1 + row), *p2 = reinterpret_cast<const uint32_t *>(st.bb_p2 + row);
            const uint32_t *src = lane < 2 ? p1 + lane
                                : lane < 4 ? p2 + (lane - 2)
                                : lane == 4 ? reinterpret_cast<const uint32_t *>(st.turn + row) : reinterpret_cast<const uint32_t *>(st.sym + row);
            if (lane < 6) v = *src;
        }
        return v;
    };
    int32_t rowv = 0;
    uint32_t posv = 0;
    if (STEM) {
        rowv = request_row(blockIdx.x);
        posv = request_pos(blockIdx.x, rowv, lane);
        rowv = request_row(static_cast<int64_t>(blockIdx.x) + gridDim.x);
    }
    if (EMBED && static_cast<int64_t>(blockIdx.x) < ntiles) load_planes(blockIdx.x, lane);
    if (static_cast<int64_t>(blockIdx.x) < ntiles) stage_tile(blockIdx.x, 0, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    int par = 0;
    const bool prof = dbg & 16;
    unsigned long long tp[7] = {0, 0, 0, 0, 0, 0, 0}, tl = prof ? __builtin_amdgcn_s_memtime() : 0;
    auto stamp = [&](int k) {
        if (prof) {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            tp[k] += now - tl;
            tl = now;
        }
    };
    // where this lane's vectors of its sample go in the padded, swizzled image: six dividing address chains that
    // do not depend on the tile - kept in registers across the tile loop (the rest of P1's and P3's lane
    // arithmetic is cheap and is recomputed per tile, see lane_t below)
    uint32_t img_off[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int sl = lane + 64 * i;
        const int cell = sl / VPC;
        const int r = cell / COLS, c = cell - r * COLS;
        const int p = (r + 1) * PCOLS + (c + 1);
        const int ck = (lane % VPC) ^ swz_in(lane / VPC);
        img_off[i] = static_cast<uint32_t>((wave * PCELLS + p) * CELLB + ((ck ^ (p & 7)) << 4));
    }
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1) {
        const int64_t b0 = tile * TS;
        uint8_t *rawt = rawb + (STEM ? 0 : par) * TS * SB;
        uint8_t *outt = RESID ? rawt : outs;
        // Opaque copy of the lane id: everything P1, P3 and the staging derive from it is
        // recomputed per tile (a few VALU ops) instead of being hoisted out of the tile loop,
        // where ~40 loop-invariant addresses would push the resident weights into scratch.
        // The copy is masked to what a lane id is, 0 .. 63, and unsigned: of a lane's vectors only the last one needs
        // a bounds test, and its divisions are shifts.
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        const uint32_t lane_t = static_cast<uint32_t>(lane_o) & 63u;

        // ---- P0 (STEM): this wave's sample from its position to the raw tile - k_stem's arithmetic (nn_stem.hip) with
        // the tables in LDS and the 16-byte store going to cell tok, chunk (4 m + g) ^ (tok & 7) of the raw tile.  The
        // slot was last read by this wave (P3 of the previous tile) and is next read by this wave (P1): the LDS
        // executes a wave's accesses in order, no barrier.
        if (STEM) {
            const uint32_t w0 = __builtin_amdgcn_readlane(posv, 0), w1 = __builtin_amdgcn_readlane(posv, 1);
            const uint32_t w2 = __builtin_amdgcn_readlane(posv, 2), w3 = __builtin_amdgcn_readlane(posv, 3);
            const bool p1 = static_cast<int32_t>(__builtin_amdgcn_readlane(posv, 4)) > 0, mir = __builtin_amdgcn_readlane(posv, 5) != 0;
            if (b0 + wave < B) {
                const uint64_t bb1 = (static_cast<uint64_t>(w1) << 32) | w0, bb2 = (static_cast<uint64_t>(w3) << 32) | w2;
                const uint64_t own = p1 ? bb1 : bb2, opp = p1 ? bb2 : bb1;
                const int g = lane_t >> 4, tl = lane_t & 15;
                // the cell this lane tests when the board masks are built (cell order: 7 * row + column, row 0 on top)
                const int my_r = lane_t / COLS, my_c = static_cast<int>(lane_t) - my_r * COLS;
                const int bit = (mir ? COLS - 1 - my_c : my_c) * 7 + (5 - my_r);
                const bool own_here = lane_t < CELLS && ((own >> bit) & 1ull);
                const bool opp_here = lane_t < CELLS && ((opp >> bit) & 1ull);
                // boards in cell order, moved up by 8 so that the window of cell n is bits n .. n + 16 of the word
                const uint64_t om8 = __ballot(own_here) << 8, pm8 = __ballot(opp_here) << 8;
                // this lane's four taps: where each one's neighbour sits in the 3x3 window word (bit 7 dy + dx); taps
                // 9..15 do not exist: bit 31 of the window word is always zero
                int sh[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int tp4 = g * 4 + j;
                    sh[j] = tp4 < 9 ? (tp4 / 3) * 7 + tp4 % 3 : 31;
                }
                bf16x8 bq[3];
                int tok[3];
#pragma unroll
                for (int tt = 0; tt < 3; ++tt) {
                    // which window bits exist for this lane's token (column 0 has no left neighbours, column 6 no right ones)
                    const int token = tt * 16 + tl;
                    tok[tt] = token;
                    const int c = token % COLS;
                    uint32_t m = 0x1C387u;                                      // bits 0-2, 7-9, 14-16
                    if (c == 0) m &= ~0x4081u;                                  // bits 0, 7, 14
                    if (c == COLS - 1) m &= ~0x10204u;                          // bits 2, 9, 16
                    const uint32_t cmask = token < CELLS ? m : 0u;
                    const uint32_t wo = static_cast<uint32_t>(om8 >> token) & cmask;
                    const uint32_t wp = static_cast<uint32_t>(pm8 >> token) & cmask;
                    uint32_t d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)                             // bf16 1.0 = 0x3F80: own in the low half, opp in the high half
                        d[j] = (((wo >> sh[j]) & 1u) | (((wp >> sh[j]) & 1u) << 16)) * 0x3F80u;
                    bq[tt] = __builtin_bit_cast(bf16x8, uint4{d[0], d[1], d[2], d[3]});
                }
                const float *s_p = reinterpret_cast<const float *>(s_pm);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    // fragments [part][channel tile][lane]: tiles 2 m and 2 m + 1 are this lane's eight channels 32 m + 8 g ..
                    const bf16x8 h0 = *reinterpret_cast<const bf16x8 *>(s_fr + ((0 * 4 + 2 * m) * 64 + lane_t) * 16);
                    const bf16x8 h1 = *reinterpret_cast<const bf16x8 *>(s_fr + ((0 * 4 + 2 * m + 1) * 64 + lane_t) * 16);
                    const bf16x8 l0 = *reinterpret_cast<const bf16x8 *>(s_fr + ((1 * 4 + 2 * m) * 64 + lane_t) * 16);
                    const bf16x8 l1 = *reinterpret_cast<const bf16x8 *>(s_fr + ((1 * 4 + 2 * m + 1) * 64 + lane_t) * 16);
                    const int ch = m * 32 + g * 8;
#pragma unroll
                    for (int tt = 0; tt < 3; ++tt) {
                        f32x4 a0 = *reinterpret_cast<const f32x4 *>(&s_p[tok[tt] * PROW + ch]);
                        f32x4 a1 = *reinterpret_cast<const f32x4 *>(&s_p[tok[tt] * PROW + ch + 4]);
                        a0 = MFMA32(h0, bq[tt], a0);
                        a1 = MFMA32(h1, bq[tt], a1);
                        a0 = MFMA32(l0, bq[tt], a0);
                        a1 = MFMA32(l1, bq[tt], a1);
                        const f32x2 s0 = silu2(f32x2{a0[0], a0[1]}), s1 = silu2(f32x2{a0[2], a0[3]});
                        const f32x2 s2 = silu2(f32x2{a1[0], a1[1]}), s3 = silu2(f32x2{a1[2], a1[3]});
                        V8 o;
                        o.w[0] = pack2(s0.x, s0.y); o.w[1] = pack2(s1.x, s1.y); o.w[2] = pack2(s2.x, s2.y); o.w[3] = pack2(s3.x, s3.y);
                        if (tt < 2 || tok[tt] < CELLS)
                            *reinterpret_cast<V8 *>(rawt + wave * SB + tok[tt] * 128 + (((4 * m + g) ^ (tok[tt] & 7)) << 4)) = o;
                    }
                }
            }
            stamp(6);
        }
        // ---- P1: GroupNorm statistics of this wave's sample (one pass, fp32), then the
        // normalised vectors go to the padded image
        {
            const int ck = (lane_t % VPC) ^ swz_in(lane_t / VPC);   // the channel chunk of every slot this lane owns
            const bool last_ok = lane_t < LASTN;                    // the only vector of a lane that can lie past the sample
            const uint8_t *rawl = rawt + wave * SB + lane_t * 16;   // this lane's vectors: 1 KiB apart
            V8 raw[PER];
            if (EMBED) {
                // tokens = pos[cell] + own * emb_own + opp * emb_opp (fp32 on the bf16 tables, rounded once:
                // the arithmetic of k_embed, nn_kernels.hip)
                const V8 eo = *reinterpret_cast<const V8 *>(em.emb_own + ck * 8), ep = *reinterpret_cast<const V8 *>(em.emb_opp + ck * 8);
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (i < PER - 1 || last_ok) {
                        const V8 ps = *reinterpret_cast<const V8 *>(rawb + lane_t * 16 + i * 1024);
                        const f32x2 own = {pl_own[i], pl_own[i]}, opp = {pl_opp[i], pl_opp[i]};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            // p + own*a + opp*o evaluated left to right, as k_embed does
                            const f32x2 v = unpack2(ps.w[q]) + own * unpack2(eo.w[q]) + opp * unpack2(ep.w[q]);
                            raw[i].w[q] = pack2(v.x, v.y);
                        }
                    } else {
                        raw[i].w[0] = raw[i].w[1] = raw[i].w[2] = raw[i].w[3] = 0;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (i < PER - 1 || last_ok) raw[i] = *reinterpret_cast<const V8 *>(rawl + i * 1024);
                    else raw[i].w[0] = raw[i].w[1] = raw[i].w[2] = raw[i].w[3] = 0;
                }
            }
            f32x2 sc[4], sh[4];
            if (NORM) {
                f32x2 sum2 = {0.0f, 0.0f}, sq2 = {0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < PER; ++i) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x2 f = unpack2(raw[i].w[q]);              // vectors past the sample are zero
                        sum2 += f;
                        sq2 = __builtin_elementwise_fma(f, f, sq2);
                    }
                }
                const float sum = wave_sum(sum2.x + sum2.y), sq = wave_sum(sq2.x + sq2.y);
                const float mean = sum * (1.0f / (CELLS * CIN));
                const float var = fmaxf(sq * (1.0f / (CELLS * CIN)) - mean * mean, 0.0f);
                const float rstd = rsqrtf(var + eps);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x2 gq = *reinterpret_cast<const f32x2 *>(&s_gam[ck * 8 + 2 * q]);
                    const f32x2 bq = *reinterpret_cast<const f32x2 *>(&s_bet[ck * 8 + 2 * q]);
                    sc[q] = gq * f32x2{rstd, rstd};
                    sh[q] = bq - sc[q] * f32x2{mean, mean};
                }
            }
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (i < PER - 1 || last_ok) {
                    V8 out = raw[i];
                    if (NORM) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x2 f = __builtin_elementwise_fma(unpack2(raw[i].w[q]), sc[q], sh[q]);
                            out.w[q] = pack2(f.x, f.y);
                        }
                    }
                    *reinterpret_cast<V8 *>(img + img_off[i]) = out;
                }
            }
        }
        stamp(0);
        lds_barrier();
        stamp(1);
        // the next tile travels from HBM into the other raw buffer while this one is multiplied
        // (every wave finished reading that buffer - P3 of the previous tile - before the barrier)
        if (tile + gridDim.x < ntiles) {
            stage_tile(tile + gridDim.x, par ^ 1, lane_t);
            if (EMBED) load_planes(tile + gridDim.x, lane_t);
        }
        if (STEM) {
            posv = request_pos(tile + gridDim.x, rowv, lane_t);
            rowv = request_row(tile + 2 * static_cast<int64_t>(gridDim.x));
        }

        // ---- P2: wave (mh, th) owns samples 2*th and 2*th+1 of the tile, each as three token
        // tiles of 16 over a 6 x 8 token grid: token t sits at image cell t + 9, its 8th column is
        // the halo cell (a dummy token whose result is dropped), so a tile's cells are
        // consecutive - every B-fragment read is bank-conflict free and needs no division.
        // The loop is software pipelined by one tile: the epilogue of tile i-1 (VALU) is issued
        // inside the MFMA stream of tile i, where an MFMA leaves half of its 16 issue cycles free.
        // Token tile `it` of this wave's pair of samples starts (it / 3) * PCELLS + (it % 3) * 16 cells after
        // tile 0 - a multiple of 8 either way, so the swizzle key (cell & 7) of a lane's cell is the same in
        // every tile and its byte offset differs by a CONSTANT: the three column offsets are computed once
        // per 4-sample tile and every fragment read carries tile and row displacement in its offset field.
        uint32_t col[3][KPT];
        {
            const uint32_t pc = static_cast<uint32_t>(2 * th * PCELLS + l15 + 9 - PCOLS - 1);   // row above, dx = -1
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const uint32_t p = pc + d;
                const uint32_t o = (p * CELLB + ((l4 ^ (p & 7)) << 4)) & 0xffffu;
#pragma unroll
                for (int ks = 0; ks < KPT; ++ks) col[d][ks] = o ^ (ks << 6);
            }
        }
        auto fetch = [&](int it, int tap, bf16x8 (&xf)[KPT]) {
            const int dy = tap / 3, d = tap % 3;
            const int disp = (dy * PCOLS + (it / 3) * PCELLS + (it % 3) * 16) * CELLB;
#pragma unroll
            for (int ks = 0; ks < KPT; ++ks)
                xf[ks] = *reinterpret_cast<const bf16x8 *>(&smem[col[d][ks] + disp]);   // img = smem + 0
        };
        // Epilogue of one token tile on its accumulators, cut into 36 single-instruction steps so
        // that it can be issued INSIDE the next tile's MFMA stream.  This lane holds channels
        // 8*(4*mh+l4) .. +7 of token (lane & 15): the bias is already in; SiLU, residual, and the
        // vector goes to the output tile in LDS (dummy tokens: to a scratch slot).
        struct Epi { V8 *slot; V8 rr, o; f32x2 t, v; };
        auto epi_begin = [&](int it, Epi &e) {
            const int smp = 2 * th + it / 3, t = (it % 3) * 16 + l15;
            const int cell = (t >> 3) * COLS + (t & 7);
            // branch-free on purpose: a branch would end the scheduling region
            const uint32_t m = (t & 7) == 7 ? 0xffffffffu : 0u;
            const uint32_t off_real = static_cast<uint32_t>(outt - smem) + smp * OSB + cell * 128 + (((mh * 4 + l4) ^ (cell & 7)) << 4);
            const uint32_t off_dump = static_cast<uint32_t>(dump - smem) + (wave * 8 + (l15 >> 3) + 2 * l4) * 16;
            e.slot = reinterpret_cast<V8 *>(&smem[(off_real & ~m) | (off_dump & m)]);
            if (RESID) e.rr = *e.slot;
        };
        auto epi_step = [&](int step, const f32x4 (&acc)[2], Epi &e) {       // step 0..35, constant after unrolling
            const int q = step / 9;
            const f32x2 x = {acc[q >> 1][2 * (q & 1)], acc[q >> 1][2 * (q & 1) + 1]};
            switch (step % 9) {
            // SiLU = x / (1 + 2^(-x log2 e)) on the hardware exp2 / reciprocal (about 1 ulp each; the
            // result is rounded to bf16 right after)
            case 0: e.t = x * f32x2{-1.44269504f, -1.44269504f}; break;
            case 1: e.t.x = __builtin_amdgcn_exp2f(e.t.x); break;
            case 2: e.t.y = __builtin_amdgcn_exp2f(e.t.y); break;
            case 3: e.t += f32x2{1.0f, 1.0f}; break;
            case 4: e.t.x = __builtin_amdgcn_rcpf(e.t.x); break;
            case 5: e.t.y = __builtin_amdgcn_rcpf(e.t.y); break;
            case 6: e.v = x * e.t; break;
            case 7: if (RESID) e.v += unpack2(e.rr.w[q]); break;
            default: e.o.w[q] = pack2(e.v.x, e.v.y); break;
            }
        };
        auto epi_end = [&](Epi &e) { *e.slot = e.o; };

        // One pipelined block: the 36 (18) MFMAs of token tile `it` (B fragments read one tap
        // ahead), each followed by one or two epilogue steps of the previous tile.  The
        // scheduling barriers pin that order: a wave issues in order, so a VALU instruction
        // hides in an MFMA's free issue cycles only if it sits right behind it in the stream.
        auto block = [&](int it, f32x4 (&acc)[2], bool with_epi, const f32x4 (&pacc)[2]) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt] = f32x4{bia[mt][0], bia[mt][1], bia[mt][2], bia[mt][3]};
            Epi e;
            if (with_epi) epi_begin(it - 1, e);
            bf16x8 xa[KPT], xb[KPT];
            fetch(it, 0, xa);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                bf16x8 (&cur)[KPT] = (tap & 1) ? xb : xa;
                bf16x8 (&nxt)[KPT] = (tap & 1) ? xa : xb;
                if (tap + 1 < 9) fetch(it, tap + 1, nxt);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < KPT; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const int s = tap * KPT + ks;
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[mt][s], cur[ks], acc[mt], 0, 0, 0);
                        if (with_epi) {
                            __builtin_amdgcn_sched_barrier(0);
                            constexpr int PER_SLOT = 36 / (18 * KPT);          // 1 (C_in 64) or 2 (C_in 32)
                            const int slot = (tap * KPT + ks) * 2 + mt;
#pragma unroll
                            for (int j = 0; j < PER_SLOT; ++j) epi_step(slot * PER_SLOT + j, pacc, e);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
            }
            if (with_epi) epi_end(e);
        };
        if (!(dbg & 1)) {
            // az_nn_debug bit 5: the matrix phase at a higher issue priority than the other workgroup's load / store phases
            if ((dbg >> 5) & 3) {
                if (((dbg >> 5) & 3) == 1) __builtin_amdgcn_s_setprio(1);
                else if (((dbg >> 5) & 3) == 2) __builtin_amdgcn_s_setprio(2);
                else __builtin_amdgcn_s_setprio(3);
            }
            f32x4 acc_a[2], acc_b[2];
            block(0, acc_a, false, acc_b);
            // unrolled: the tile number is a constant in every read's offset field; the accumulator sets alternate
            block(1, acc_b, true, acc_a);
            block(2, acc_a, true, acc_b);
            block(3, acc_b, true, acc_a);
            block(4, acc_a, true, acc_b);
            block(5, acc_b, true, acc_a);
            {   // drain: the last tile's epilogue on its own
                Epi e;
                epi_begin(5, e);
#pragma unroll
                for (int step = 0; step < 36; ++step) epi_step(step, acc_b, e);
                epi_end(e);
            }
            if ((dbg >> 5) & 3) __builtin_amdgcn_s_setprio(0);
        }
        // the staged tile has landed; every wave is done with img and has written its outputs
        stamp(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(3);
        lds_barrier();
        stamp(4);

        // ---- P3: the output tile leaves as whole 128-byte rows (wave = sample, 16 bytes per lane)
        if (b0 + wave < B && !(dbg & 2)) {
            // the sample's (wave-uniform) base, one offset per lane on either side, 1024 i as a constant
            // (the base is the sample's MIDDLE: a store's offset field holds -4096 .. 4095, which then reaches all six)
            constexpr int MID = (OPER / 2) * 1024;
            uint8_t *ym = reinterpret_cast<uint8_t *>(y + (b0 + wave) * (CELLS * COUT)) + MID;
            uint32_t outl = static_cast<uint32_t>(outt - smem) + wave * OSB + lane_t * 16;
            // (opaque, or the compiler folds MID back into the constants and builds a 64-bit address per lane for the
            // vectors past 4095, and adds the LDS constants in registers instead of offset fields)
            asm volatile("" : "+s"(ym), "+v"(outl));
            auto *ymg = (__attribute__((address_space(1))) uint8_t *)ym;      // still global memory, which the statement hid
            const uint32_t yo = tok_off(lane_t, COUT / 8);
#pragma unroll
            for (int i = 0; i < OPER; ++i) {
                if (i < OPER - 1 || lane_t < OLASTN) {
                    const V8 v = *reinterpret_cast<const V8 *>(&smem[outl + i * 1024]);
                    // (a built-in vector type: a struct has no assignment into a named address space)
                    *reinterpret_cast<__attribute__((address_space(1))) f32x4 *>(ymg + yo + (i * 1024 - MID)) = __builtin_bit_cast(f32x4, v);
                }
            }
        }
        // (the next tile's P1 writes img and reads the other raw buffer; its barrier orders these
        // reads of the output tile before the staging that overwrites it)
        stamp(5);
    }
    if (prof && lane == 0 && blockIdx.x < 512)
        for (int k = 0; k < (STEM ? 7 : 6); ++k) g_prof[(blockIdx.x * 4 + wave) * 8 + k] = tp[k];
