// attention_long_body.h -- the STATEMENTS of a (KV head, sequence, range) workgroup of the long-context decode kernels, included INSIDE
// the kernel definitions of attention_long.hip and attention_window.hip (no include guard: it is text, not declarations): the rotation,
// the writer, the walk of the range's pages through wave-private LDS-DMA rings, the wave merge and the record.  Text, not an inlined
// function, so that attention_long.hip's kernels compile to the instructions they compiled to before the window kernels existed.
// The including kernel provides its parameters under the names used here (decode_long_kernel's), `INT4`, a `constexpr bool WINDOW`
// and - read under WINDOW only - `int window` >= 1: the new token at position tl sees the cached tokens [max(0, tl + 1 - window), tl).
// The comments on mapping, data movement and arithmetic stand in attention_long.hip, the window's in attention_window.hip.
    using L = Lds<INT4>;
    constexpr int DHB = L::DHB, PAGE_BYTES = L::PAGE_BYTES;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    _Float16 (*s_q)[DH] = reinterpret_cast<_Float16 (*)[DH]>(smem + L::Q);
    int64_t (*s_win)[WIN] = reinterpret_cast<int64_t (*)[WIN]>(smem + L::WINDOW);
    _Float16* s_knew = reinterpret_cast<_Float16*>(smem + L::KNEW);
    float* s_cur = reinterpret_cast<float*>(smem + L::CUR);
    float (*s_m)[16] = reinterpret_cast<float (*)[16]>(smem + L::ML);
    float (*s_l)[16] = s_m + NW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, tg = lane >> 4;
    const int hkv = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int tl = lengths ? lengths[b] - 1 : timestep;          // position of the new token = number of cached tokens
    float* const rec = ws ? ws + (((size_t)b * num_kv_heads + hkv) * S + z) * G * (DH + 2) : nullptr;

    // ---- this workgroup's range ----------------------------------------------------------------------------------------------
    // WINDOW: the pages [p_first, p_first + npages) that hold a visible cached token, [lo, tl) with lo = max(0, tl + 1 - window).
    // lo >= tl (window = 1, or nothing cached) leaves no page; otherwise token lo is cached, visible and sits in page p_first, so
    // the first page - the only one that can hold tokens below lo - always keeps a key.
    int npages = min((tl + PAGE_TOK - 1) >> 6, max_blocks);
    [[maybe_unused]] int lo = 0, p_first = 0;
    if constexpr (WINDOW) {
        lo = max(0, tl + 1 - window), p_first = lo >> 6;
        npages = lo < tl ? max(0, npages - p_first) : 0;
    }
    const int nr = max(1, min(S, npages / min_pages));
    if (tl < 0 || z >= nr) {                                     // nothing to read: the empty record (S > 1, or tl < 0)
        if (rec)
            for (int o = tid; o < G * (DH + 2); o += TPB) rec[o] = o % (DH + 2) == DH ? -3.0e38f : 0.f;
        return;
    }
    int p_begin = z * npages / nr, p_end = (z + 1) * npages / nr;
    if constexpr (WINDOW) p_begin += p_first, p_end += p_first;
    const bool writer = z == nr - 1;                             // the range that ends at the last page: the new token is its
    const int64_t* ktab = kv_pointers + (size_t)b * 2 * max_blocks;
    const int64_t* vtab = ktab + max_blocks;
    const float qk_scale = 0.08838834764831845f * 1.4426950408889634f;   // 1 / sqrt(128), scores in the log2 domain

    // ---- RoPE of the G query heads and of k; the writer quantises and stores the new token -------------------------------------
    const _Float16* qb = q + (size_t)b * q_stride0 + (size_t)hkv * G * DH;
    const _Float16* kb = k + (size_t)b * kv_stride0 + (size_t)hkv * DH;
    const _Float16* vb = v + (size_t)b * kv_stride0 + (size_t)hkv * DH;
    if (tid < 64) {
        RopeCS cs;
        if (rope_tab && tl < rope_tab_len) {
            const float2 t = rope_tab[(size_t)tl * 64 + tid];
            cs.c = t.x, cs.s = t.y;
        } else {
            cs = rope_coef_any(tid, tl, rope_base, DH, rope_tab);
        }
        for (int h = 0; h < G; ++h) {
            _Float16 a, bb;
            rope_pair((float)qb[h * DH + tid], (float)qb[h * DH + 64 + tid], cs, a, bb);
            s_q[h][tid] = a, s_q[h][64 + tid] = bb;
        }
        _Float16 a, bb;
        rope_pair((float)kb[tid], (float)kb[64 + tid], cs, a, bb);
        s_knew[tid] = a, s_knew[64 + tid] = bb;
    } else {
        for (int i = tid - 64; i < (16 - G) * DH; i += TPB - 64) s_q[G + i / DH][i % DH] = (_Float16)0.f;
    }
    __syncthreads();
    if (writer) {
        const int blk = tl >> 6, slot = tl & 63;
        if (wave < 2 && blk < max_blocks) {
            uint8_t* pg = reinterpret_cast<uint8_t*>(wave == 0 ? ktab[blk] : vtab[blk]);
            __half* sc = reinterpret_cast<__half*>(pg + (size_t)num_kv_heads * PAGE_BYTES);
            const _Float16 x0 = wave == 0 ? s_knew[2 * lane] : vb[2 * lane], x1 = wave == 0 ? s_knew[2 * lane + 1] : vb[2 * lane + 1];
            wave_quant_write<INT4>(x0, x1, pg + ((size_t)hkv * PAGE_TOK + slot) * DHB, sc + hkv * PAGE_TOK + slot,
                                   sc + (num_kv_heads + hkv) * PAGE_TOK + slot, lane);
        } else if (wave >= 2) {
            for (int h = wave - 2; h < G; h += NW - 2) {
                const float d = wave_sum((float)s_q[h][lane] * (float)s_knew[lane] + (float)s_q[h][64 + lane] * (float)s_knew[64 + lane]);
                if (lane == 0) s_cur[h] = d * qk_scale;
            }
        }
    }
    // B operand of Q.K^T for the whole walk: head li, dims 32 tg + 8 w .. + 7
    h8 qB[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) qB[w] = *reinterpret_cast<const h8*>(&s_q[li][32 * tg + 8 * w]);

    v4f acc[8];                      // acc[e][r]: out dim 8 (4 tg + r) + e of head li
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (v4f){0.f, 0.f, 0.f, 0.f};
    float m_run = -3.0e38f, l_part = 0.f;

    uint8_t* const ring = smem + wave * (DEPTH * L::STAGE);
    for (int wbase = p_begin; wbase < p_end; wbase += WIN) {
        const int wend = min(wbase + WIN, p_end);
        __syncthreads();                                         // the window before is consumed (first pass: s_cur, s_q are written)
        if (tid < wend - wbase) {
            s_win[0][tid] = ktab[wbase + tid];
            s_win[1][tid] = vtab[wbase + tid];
        }
        __syncthreads();
        // one stage: K page, k scales | zeros, V page, v scales | zeros
        auto issue = [&](int p, int st) {
            uint8_t* const stage = ring + st * L::STAGE;
            const uint8_t* kpage = reinterpret_cast<const uint8_t*>(s_win[0][p - wbase]);
            const uint8_t* vpage = reinterpret_cast<const uint8_t*>(s_win[1][p - wbase]);
            const u32 meta = (u32)(num_kv_heads * PAGE_BYTES + ((lane >> 5) * num_kv_heads + hkv) * (PAGE_TOK * 2) + (lane & 31) * 4);
            const uint8_t* kd = kpage + (u32)(hkv * PAGE_BYTES);
            const uint8_t* vd = vpage + (u32)(hkv * PAGE_BYTES);
#pragma unroll
            for (int e = 0; e < L::NDMA; ++e) {
                u32 off;
                if (INT4) {
                    off = e * 1024 + lane * 16;
                } else {
                    const int row = 8 * e + (lane >> 3);
                    off = row * DHB + (((lane & 7) ^ ((row >> 1) & 7)) * 16);
                }
                __builtin_amdgcn_global_load_lds((gptr_t)(kd + off), (lptr_t)(stage + e * 1024), 16, 0, NT_AUX);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)(kpage + meta), (lptr_t)(stage + 2 * PAGE_BYTES), 4, 0, 0);
#pragma unroll
            for (int e = 0; e < L::NDMA; ++e) {
                constexpr int CPR = DHB / 16;                    // 16-byte chunks per token row
                const int slot = (64 / L::NDMA) * e + lane / CPR;
                const int tok = (slot & ~3) | ((slot - (slot >> 2)) & 3);
                const u32 off = tok * DHB + (lane % CPR) * 16;
                __builtin_amdgcn_global_load_lds((gptr_t)(vd + off), (lptr_t)(stage + PAGE_BYTES + e * 1024), 16, 0, NT_AUX);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)(vpage + meta), (lptr_t)(stage + 2 * PAGE_BYTES + 256), 4, 0, 0);
        };
        int p = wbase + wave;
        if (p < wend) issue(p, 0);
        if (p + NW < wend) issue(p + NW, 1);
        for (int st = 0; p < wend; p += NW, st ^= 1) {
            // page p landed?  Younger VMEM instructions at this point: the NVM of page p + NW, where there is one.
            if (p + NW < wend) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L::NVM) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int valid = min(PAGE_TOK, tl - p * PAGE_TOK);
            const lds_u8 kl = (lds_u8)(ring + st * L::STAGE), vl = kl + PAGE_BYTES, ml = kl + 2 * PAGE_BYTES;

            // ---------------- Q.K^T: 4 tiles of 16 tokens; sc[t][r] = token 16 t + 4 tg + r, head li ----------------
            float sc[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int row = 16 * t + li;
                const _Float16 ks = LDS_AT(_Float16, ml + 2 * row), kz = LDS_AT(_Float16, ml + 128 + 2 * row);
                v4f c = {0.f, 0.f, 0.f, 0.f};
                if (INT4) {
                    const v4u raw = LDS_AT(v4u, kl + row * DHB + tg * 16);
#pragma unroll
                    for (int w = 0; w < 4; ++w) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<true>(raw[w], 0, ks, kz), qB[w], c, 0, 0, 0);
                } else {
                    const int sw = (row >> 1) & 7;
                    const v4u ra = LDS_AT(v4u, kl + row * DHB + (((2 * tg) ^ sw) * 16));
                    const v4u rb = LDS_AT(v4u, kl + row * DHB + (((2 * tg + 1) ^ sw) * 16));
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(ra[0], ra[1], ks, kz), qB[0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(ra[2], ra[3], ks, kz), qB[1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(rb[0], rb[1], ks, kz), qB[2], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(dequant8<false>(rb[2], rb[3], ks, kz), qB[3], c, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = c[r];
                    sc[t][r] = 16 * t + 4 * tg + r < valid ? s * qk_scale : -3.0e38f;      // (a select: unwritten slots may hold NaN)
                }
            }
            // WINDOW: the lower edge.  Only page p_first holds tokens below lo (wave 0 of range 0 meets it, as its first page): one
            // wave-uniform compare per page, the 16 selects behind it on that page alone.  Such a token is written (below tl): its V is finite
            // and its probability exactly 0 - the page keeps token lo, so m_new is a real score.
            if constexpr (WINDOW) if (p == p_first) {
                const int first = lo - p_first * PAGE_TOK;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (16 * t + 4 * tg + r < first) sc[t][r] = -3.0e38f;
            }
            // ---------------- online softmax of head li over the page (its 64 scores sit in the 4 lanes li + 16 tg) ----------------
            float mx = sc[0][0];
#pragma unroll
            for (int j = 1; j < 16; ++j) mx = fmaxf(mx, sc[j >> 2][j & 3]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            l_part *= alpha;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] *= alpha;
            u32 pk[4][2];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float pe[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pe[r] = __builtin_amdgcn_exp2f(sc[t][r] - m_new);   // 0 for masked tokens
                    l_part += pe[r];
                }
                pk[t][0] = pack_h2(pe[0], pe[1]), pk[t][1] = pack_h2(pe[2], pe[3]);
            }
            // ---------------- P.V: two half pages; the lane's 8 tokens of half hp are 32 hp + 16 jh + 4 tg + r ----------------
#pragma unroll
            for (int hp = 0; hp < 2; ++hp) {
                const h8 pB = __builtin_bit_cast(h8, (v4u){pk[2 * hp][0], pk[2 * hp][1], pk[2 * hp + 1][0], pk[2 * hp + 1][1]});
                h8 d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = j & 3, tok = 32 * hp + 16 * (j >> 2) + 4 * tg + r;
                    const int slot = 32 * hp + 16 * (j >> 2) + 4 * tg + ((r + tg) & 3);
                    _Float16 vs = LDS_AT(_Float16, ml + 256 + 2 * tok), vz = LDS_AT(_Float16, ml + 384 + 2 * tok);
                    if (tok >= valid) vs = (_Float16)0.f, vz = (_Float16)0.f;      // unwritten slots de-quantise to 0, not to NaN
                    if (INT4) {
                        d[j] = dequant8<true>(LDS_AT(u32, vl + slot * DHB + 4 * li), 0, vs, vz);
                    } else {
                        const v2u raw = LDS_AT(v2u, vl + slot * DHB + 8 * li);
                        d[j] = dequant8<false>(raw.x, raw.y, vs, vz);
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const h8 a_e = {d[0][e], d[1][e], d[2][e], d[3][e], d[4][e], d[5][e], d[6][e], d[7][e]};
                    acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_e, pB, acc[e], 0, 0, 0);
                }
            }
            // the stage is consumed: page p + 2 NW takes it
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (p + 2 * NW < wend) issue(p + 2 * NW, st);
        }
    }

    // ---- waves -> LDS (the dead rings), then one result per head: `out`, or the range's record -------------------------------------
    l_part += __shfl_xor(l_part, 16, 64);
    l_part += __shfl_xor(l_part, 32, 64);
    __syncthreads();                                             // every wave has drained its ring (and passed the prologue)
    float (*s_o)[8][OS] = reinterpret_cast<float (*)[8][OS]>(smem);
    if (li < G) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = acc[e][r];
                s_o[wave][li][8 * (4 * tg + r) + e] = x;
            }
        if (tg == 0) s_m[wave][li] = m_run, s_l[wave][li] = l_part;
    }
    __syncthreads();
    for (int o = tid; o < G * DH; o += TPB) {
        const int h = o / DH, d = o % DH;
        float M = writer ? s_cur[h] : -3.0e38f;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, s_m[w][h]);
        const float pc = writer ? __builtin_amdgcn_exp2f(s_cur[h] - M) : 0.f;      // the new token's own term
        float num = pc * (float)vb[d], den = pc;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float f = __builtin_amdgcn_exp2f(s_m[w][h] - M);
            num += f * s_o[w][h][d];
            den += f * s_l[w][h];
        }
        if (!rec) {
            out[((size_t)b * num_heads + (size_t)hkv * G + h) * DH + d] = (_Float16)(num / (den + 1.e-6f));
        } else {                                                 // un-normalised: [O(128) | m | l], m in natural-log units (the merge's)
            float* pw = rec + h * (DH + 2);
            pw[d] = num;
            if (d == 0) pw[DH] = M * 0.6931471805599453f, pw[DH + 1] = den;
        }
    }
