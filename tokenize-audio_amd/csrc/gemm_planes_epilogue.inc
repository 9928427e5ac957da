// The staged epilogue of one wave's (TM x TN tiles of MF x MF) block of a planes GEMM, textually included by
// gemm_planes_kernel (gemm_planes.h) and gemm_planes256_kernel (gemm_planes256.h) -- one text, and the device code of
// the kernels that had it inline stays what it was.  The including scope provides the constants MF, TM, TN, JH, EPI,
// OUTP, FL, F16 and: p (GemmArgs), acc[TM][TN], lane, float* stg (the wave's private fp32 staging of TM MF rows x
// (TN MF / JH + 4) floats), long long cel (the item's first C / planes / R element), int Mb (its valid output rows),
// int rbase, cb0 (the block's first row and column), float omx (the running max|planes value|).
{
    constexpr int ONS = OUTP & 7;
    constexpr bool OELU = (OUTP & 8) != 0;
    constexpr int NACC = MF == 32 ? 16 : 4;
    constexpr int RW = TM * MF, TNC = TN / JH, CWC = TNC * MF, LDE = CWC + 4;
    const int N = p.N;
    const int hsel = MF == 32 ? lane >> 5 : lane >> 4;
    const float* __restrict__ Rb = p.R ? p.R + cel : nullptr;
    const int cbase = cb0 + (lane & (MF - 1));
    const float us = F16 ? p.unscale : 1.0f;  // 1 / (activation scale x weight scale): exact power of two
#pragma unroll
    for (int jh = 0; jh < JH; ++jh) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = jh * TNC; j < (jh + 1) * TNC; ++j) {
            const int col = cbase + j * MF;
            float bias = 0.0f, scale = 0.0f;
            if (col < N) {
                if (EPI == EPI_BIAS || EPI == EPI_BIAS_ELU || EPI == EPI_BIAS_RES_ELU || EPI == EPI_BIAS_OUT)
                    bias = p.bias[col];
                if (EPI == EPI_SCALE_RES) scale = p.scale[col];
            }
#pragma unroll
            for (int r = 0; r < NACC; ++r) {
                const int lrow = MF == 32 ? i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel : i * 16 + 4 * hsel + r;
                const int row = rbase + lrow;
                const bool ok = row < Mb && col < N;
                float v = F16 ? acc[i][j][r] * us : acc[i][j][r];
                if (EPI == EPI_BIAS || EPI == EPI_BIAS_OUT) {
                    v = v + bias;
                } else if (EPI == EPI_BIAS_ELU) {
                    v = elu1(v + bias);
                } else if (EPI == EPI_BIAS_RES_ELU) {
                    // + R and ELU in phase 2 (vector R loads).  fp16 planes: acc * unscale + bias as one FMA -- the same
                    // value (the power-of-two unscale makes the product exact) in one instruction, as res1_stream and
                    // the fused blocks form it
                    v = F16 ? __builtin_fmaf(acc[i][j][r], us, bias) : v + bias;
                } else if (EPI == EPI_GELU) {
                    // f16x3: the branch-free erfc form (fc1 0.583 -> 0.561-0.565 ms per B = 32 step; codes bitwise
                    // equal on the bench batches, profiles/r6g1_ab_gelu.txt); the bf16 modes keep OCML's erff
                    v = F16 ? gelu_fast(v) : gelu_erf(v);
                } else if (EPI == EPI_SCALE_RES) {
                    v = scale * v;  // + R in phase 2
                } else if (EPI == EPI_ROPE) {
                    if (ok && col < p.rope_cols) {
                        // head_dim = 64: the pair (d, d + 32) sits in tiles j, j + 32/MF of the same lane
                        constexpr int PJ = 32 / MF;
                        const int d = col % 64;
                        const int pos = p.rope_pos ? p.rope_pos[row] : row;  // packed rows: the item's own position
                        const float c = p.rope_cos[(long long)pos * 32 + (d & 31)];
                        const float sn = p.rope_sin[(long long)pos * 32 + (d & 31)];
                        if (((j / PJ) & 1) == 0) {
                            const float x2 = F16 ? acc[i][j + PJ][r] * us : acc[i][j + PJ][r];
                            v = rope_lo(v, x2, c, sn);
                        } else {
                            const float x1 = F16 ? acc[i][j - PJ][r] * us : acc[i][j - PJ][r];
                            v = rope_hi(v, x1, c, sn);
                        }
                    }
                }
                stg[lrow * LDE + (j - jh * TNC) * MF + (lane & (MF - 1))] = v;
            }
        }
    }
    float* __restrict__ Cb = p.C ? p.C + cel : nullptr;
    static_assert(!F16 || ONS == 0 || ONS == 2, "fp16 output planes: 2");
    __bf16* __restrict__ Cpb = ONS ? reinterpret_cast<__bf16*>(p.Cp) + cel : nullptr;
    constexpr bool SC1 = (FL & FL_SC1OUT) != 0;
    static_assert(!SC1 || !ONS || F16, "sc1 output stores: fp32 and fp16 planes");
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    // (SC1: buffer resources over the item's output; a null base only ever meets a store that is not issued)
    const __amdgpu_buffer_rsrc_t c_rs = make_rsrc(SC1 ? (void*)Cb : nullptr, SC1 ? 0x7fffffffLL : 0);
    const __amdgpu_buffer_rsrc_t cp_rs = make_rsrc(SC1 ? (void*)Cpb : nullptr, SC1 ? 0x7fffffffLL : 0);
    constexpr int LPR = CWC / 8;  // lanes per row
    constexpr int RPS = 64 / LPR;  // rows per pass
    // (16 x 16 wave tiles: one pass of 32 lanes, the upper half idle)
    static_assert(RW % RPS == 0 || RW < RPS, "epilogue: a wave's tile holds whole passes of 64 lanes x 8 columns");
    constexpr int NPS = RW < RPS ? 1 : RW / RPS;
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
        const int lr = ps * RPS + lane / LPR, lc = (lane % LPR) * 8;
        if (RW < RPS && lr >= RW) continue;
        f32x4 v0 = *reinterpret_cast<const f32x4*>(stg + lr * LDE + lc);
        f32x4 v1 = *reinterpret_cast<const f32x4*>(stg + lr * LDE + lc + 4);
        const int row = rbase + lr, col = cb0 + jh * CWC + lc;
        if (row >= Mb || col >= N) continue;  // N % 8 == 0: a lane's 8 columns are all in or all out
        const long long off = (long long)row * p.ldc + col;
        if (EPI == EPI_BIAS_RES_ELU || EPI == EPI_SCALE_RES) {
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(Rb + off);
            const f32x4 r1 = *reinterpret_cast<const f32x4*>(Rb + off + 4);
            v0 = r0 + v0;  // R + (acc + bias) / R + scale * acc: the reference's operation order
            v1 = r1 + v1;
            if (EPI == EPI_BIAS_RES_ELU) {
                v0.x = elu1(v0.x); v0.y = elu1(v0.y); v0.z = elu1(v0.z); v0.w = elu1(v0.w);
                v1.x = elu1(v1.x); v1.y = elu1(v1.y); v1.z = elu1(v1.z); v1.w = elu1(v1.w);
            }
        }
        if (ONS) {
            // planes out (of ELU(v) when OELU: the next residual block's conv input), fp32 v beside
            float pv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            if (OELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) pv[e] = elu1(pv[e]);
            }
            if constexpr (SC1) {  // store_act8's fp16 split, stored sc1
                uint4 ha, hb;
                split2_f16s(pv[0], pv[1], p.out_scale, ha.x, hb.x);
                split2_f16s(pv[2], pv[3], p.out_scale, ha.y, hb.y);
                split2_f16s(pv[4], pv[5], p.out_scale, ha.z, hb.z);
                split2_f16s(pv[6], pv[7], p.out_scale, ha.w, hb.w);
#pragma unroll
                for (int e = 0; e < 8; ++e) omx = fmaxf(omx, fabsf(pv[e]));
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ha), cp_rs, (int)(off * 2), 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hb), cp_rs,
                                                       (int)((off + p.c_pstride) * 2), 0, 16);
            } else {
                store_act8(Cpb, p.c_pstride, ONS, off, pv, F16 ? p.out_scale : 0.0f, &omx);
            }
        }
        if (Cb) {
            if constexpr (SC1) {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v0), c_rs, (int)(off * 4), 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v1), c_rs, (int)(off * 4 + 16), 0, 16);
            } else {
                *reinterpret_cast<f32x4*>(Cb + off) = v0;
                *reinterpret_cast<f32x4*>(Cb + off + 4) = v1;
            }
        }
    }
    asm volatile("" ::: "memory");  // this pass's staging reads precede the next pass's writes (same wave)
    }
}
