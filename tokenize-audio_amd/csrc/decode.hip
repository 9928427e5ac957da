// Decode path (MimiModel.decode, TF/modeling_mimi.py:1388-1458): the stages that are not a GEMM.
//
//   rvq_decode_kernel    codes -> the two RVQ sums (semantic | acoustic), the gather + add of
//                        MimiResidualVectorQuantizer.decode (:1070-1078) on the engine's fp32 codebook rows
//   upsample_dw_kernel   the depthwise causal transposed conv 12.5 -> 25 Hz (MimiModel.upsample, :1208-1216, :399-405)
//   final_conv_kernel    decoder.layers.14: ELU'd [B][L][64] -> waveform [B][L] (k = 3, causal, Cout = 1)
//
// All three are memory-bound streams: 16-byte loads and stores, consecutive lanes on consecutive addresses.  The
// transposed convs of the SEANet decoder run as GEMMs (gemm.hip ROLE_UPCONV), its residual blocks as the fused
// blocks of resblock.hip, the transformer as the encoder's launches on the decoder_transformer weights (engine.cpp).
//
// Each stage is one `template <bool RG>` body under two thin kernels.  RG = false: a uniform batch, [B][rows][C]
// tensors.  RG = true (mimi_decode_ragged): item b = blockIdx.y has tlen[b] rows of this stage starting at row toff[b]
// of the packed tensor (the stage's own table: lengths and offsets already times its rate factor).  The grid covers
// the longest item; a workgroup (or wave) whose rows start at or past its item's length exits before any load, so
// nothing past an item's length is read, computed or stored.  Only where a row and its item come from differs: per
// row the arithmetic is one text, so an item's values are the bits of its own uniform launch.
#include "kernels.h"

namespace mimi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// codes [B][K][T] int32 -> out [B*T][2*D] fp32 = (sum over the semantic levels | sum over the acoustic levels) of
// cb_rows[level][code][:], each half accumulated in fp32 in level order starting from 0.0 as the reference sums them
// (quantized_out = 0.0; quantized_out = quantized_out + layer.decode(indices)), so each half holds torch's bits.
// One wave per (frame, half): lane l holds columns 4l .. 4l+3 (D = 256).  K <= nsem leaves the acoustic half zero.
// BOUNDS BEFORE LOAD: a code outside [0, ncodes) never forms an address -- the wave raises *flag and gathers row 0
// (the host then fails the call: the output is unspecified but every access was in bounds).
// RG: T = the codes' padded row stride (columns >= tlen[b] are never read), out [sum tlen][2*D]; frames unused.
// ------------------------------------------------------------------------------------------------
template <bool RG>
__device__ __forceinline__ void rvq_decode_body(const int32_t* __restrict__ codes, long long frames, int T, int K,
                                                int nsem, int ncodes, const float* __restrict__ cb_rows,
                                                float* __restrict__ out, unsigned* __restrict__ flag,
                                                const int* __restrict__ tlen, const int* __restrict__ toff) {
    constexpr int D = 256;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    long long b, frame;
    int t;
    if constexpr (RG) {
        b = blockIdx.y;
        t = (int)blockIdx.x * 2 + (wave >> 1);
        if (t >= tlen[b]) return;
        frame = (long long)toff[b] + t;
    } else {
        frame = (long long)blockIdx.x * 2 + (wave >> 1);
        if (frame >= frames) return;
        b = frame / T;
        t = (int)(frame - b * T);
    }
    const int half = wave & 1;
    const int lv0 = half ? nsem : 0;
    const int lv1 = half ? K : (K < nsem ? K : nsem);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    bool bad = false;
    for (int lv = lv0; lv < lv1; ++lv) {
        const int32_t code = codes[(b * K + lv) * (long long)T + t];
        unsigned c = (unsigned)code;
        if (c >= (unsigned)ncodes) {  // (negative codes wrap above ncodes)
            bad = true;
            c = 0u;
        }
        const f32x4 v = *reinterpret_cast<const f32x4*>(cb_rows + ((long long)lv * ncodes + c) * D + 4 * lane);
        acc = acc + v;
    }
    if (bad && lane == 0) atomicOr(flag, 1u);
    *reinterpret_cast<f32x4*>(out + frame * (2 * D) + half * D + 4 * lane) = acc;
}

__global__ __launch_bounds__(256) void rvq_decode_kernel(const int32_t* __restrict__ codes, long long frames, int T,
                                                         int K, int nsem, int ncodes, const float* __restrict__ cb_rows,
                                                         float* __restrict__ out, unsigned* __restrict__ flag) {
    rvq_decode_body<false>(codes, frames, T, K, nsem, ncodes, cb_rows, out, flag, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void rvq_decode_ragged_kernel(const int32_t* __restrict__ codes, int Ts, int K, int nsem,
                                                                int ncodes, const float* __restrict__ cb_rows,
                                                                float* __restrict__ out, unsigned* __restrict__ flag,
                                                                const int* __restrict__ tlen,
                                                                const int* __restrict__ toff) {
    rvq_decode_body<true>(codes, 0, Ts, K, nsem, ncodes, cb_rows, out, flag, tlen, toff);
}

hipError_t launch_rvq_decode(const int32_t* codes, long long frames, int T, int K, int nsem, int ncodes, int D,
                             const float* cb_rows, float* out, unsigned* flag, hipStream_t s, const int* tlen,
                             const int* toff, int max_tlen) {
    if (D != 256 || frames <= 0 || T <= 0 || K < 1 || nsem < 1 || ncodes < 1 || !codes || !cb_rows || !out || !flag ||
        frames % T != 0 || !tlen != !toff)
        return hipErrorInvalidValue;
    if (tlen) {
        const long long batch = frames / T;
        if (batch > 65535 || max_tlen <= 0 || max_tlen > T) return hipErrorInvalidValue;
        hipLaunchKernelGGL(rvq_decode_ragged_kernel, dim3((unsigned)((max_tlen + 1) / 2), (unsigned)batch), dim3(256), 0,
                           s, codes, T, K, nsem, ncodes, cb_rows, out, flag, tlen, toff);
    } else {
        const long long blocks = (frames + 1) / 2;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(rvq_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, s, codes, frames, T, K, nsem, ncodes,
                           cb_rows, out, flag);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// x [B][T][C] -> y [B][2T][C], depthwise (groups = C), k = 4, stride 2, no bias, causal (the 2 trailing outputs of
// conv_transpose1d trimmed): y[2t + p][c] = w[c][p] x[t][c] + w[c][p + 2] x[t - 1][c], x[-1] = 0.
// One thread per (b, t, 4 channels): two 16-B loads of x, four of w (w[c][0..3] is one float4), two 16-B stores.
// RG: x [sum tlen][C] -> y [2 sum tlen][C]; x[t - 1] = 0 at each item's first frame (t is the position in the item);
// rows and T unused.
// HS (a step of a decode stream): item b's T rows start at x + b * xbs and x[-1] is the row in front of them, the
// stream's carry (zeros on a fresh stream): always read, never replaced by zero.  y as the uniform form.
// ------------------------------------------------------------------------------------------------
template <bool RG, bool HS = false>
__device__ __forceinline__ void upsample_dw_body(const float* __restrict__ x, const float* __restrict__ w,
                                                 float* __restrict__ y, long long rows, int T, int C4,
                                                 const int* __restrict__ tlen, const int* __restrict__ toff,
                                                 long long xbs = 0, const int* __restrict__ xoff = nullptr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    long long row;
    int c4, t;
    long long xrow = 0;  // RG and HS: the row of x that holds the item's frame t
    if constexpr (RG) {
        const int b = blockIdx.y;
        t = (int)(i / C4);
        if (t >= tlen[b]) return;
        c4 = (int)(i - (long long)t * C4);
        row = (long long)toff[b] + t;
        if constexpr (HS) xrow = (long long)xoff[b] + t;
    } else {
        if (i >= rows * C4) return;
        row = i / C4;  // b * T + t
        c4 = (int)(i - row * C4);
        t = (int)(row % T);
    }
    const int C = C4 * 4;
    const float* xr = x + row * C + 4 * c4;
    if constexpr (HS && RG)
        xr = x + xrow * C + 4 * c4;
    else if constexpr (HS)
        xr = x + (row / T) * xbs + (long long)t * C + 4 * c4;
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(xr);
    f32x4 x0 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HS || t > 0) x0 = *reinterpret_cast<const f32x4*>(xr - C);
    f32x4 o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const f32x4 wc = *reinterpret_cast<const f32x4*>(w + (long long)(4 * c4 + e) * 4);
        o0[e] = wc[0] * x1[e] + wc[2] * x0[e];
        o1[e] = wc[1] * x1[e] + wc[3] * x0[e];
    }
    float* yo = y + (2 * row) * C + 4 * c4;  // item b's rows start at twice its input's: 2 (b T + t) = 2 b T + 2 t
    *reinterpret_cast<f32x4*>(yo) = o0;
    *reinterpret_cast<f32x4*>(yo + C) = o1;
}

__global__ __launch_bounds__(256) void upsample_dw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          float* __restrict__ y, long long rows, int T, int C4) {
    upsample_dw_body<false>(x, w, y, rows, T, C4, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void upsample_dw_ragged_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 float* __restrict__ y, int C4,
                                                                 const int* __restrict__ tlen,
                                                                 const int* __restrict__ toff) {
    upsample_dw_body<true>(x, w, y, 0, 0, C4, tlen, toff);
}

__global__ __launch_bounds__(256) void upsample_dw_hist_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               float* __restrict__ y, long long rows, int T, int C4,
                                                               long long xbs) {
    upsample_dw_body<false, true>(x, w, y, rows, T, C4, nullptr, nullptr, xbs);
}

// RG and HS together (a ragged step of a decode stream): item b's tlen[b] frames sit at rows xoff[b] .. of x, each
// item's carry row right in front of its first (x = the packed [carry | chunk] blocks); y packed, rows 2 toff[b] ..
__global__ __launch_bounds__(256) void upsample_dw_hist_ragged_kernel(const float* __restrict__ x,
                                                                      const float* __restrict__ w, float* __restrict__ y,
                                                                      int C4, const int* __restrict__ tlen,
                                                                      const int* __restrict__ toff,
                                                                      const int* __restrict__ xoff) {
    upsample_dw_body<true, true>(x, w, y, 0, 0, C4, tlen, toff, 0, xoff);
}

hipError_t launch_upsample_dw_hist_ragged(const float* x, const float* w, float* y, int batch, long long max_T, int C,
                                          const int* tlen, const int* toff, const int* xoff, hipStream_t s) {
    if (batch <= 0 || batch > 65535 || max_T <= 0 || max_T > 0x7fffffffLL || C <= 0 || C % 4 || !x || !w || !y || !tlen ||
        !toff || !xoff)
        return hipErrorInvalidValue;
    const long long blocks = (max_T * (C / 4) + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample_dw_hist_ragged_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, s, x, w, y,
                       C / 4, tlen, toff, xoff);
    return hipGetLastError();
}

hipError_t launch_upsample_dw_hist(const float* x, const float* w, float* y, int batch, long long T, int C,
                                   long long x_bstride, hipStream_t s) {
    if (batch <= 0 || T <= 0 || T > 0x7fffffffLL || C <= 0 || C % 4 || !x || !w || !y || x_bstride < (T + 1) * C ||
        x_bstride % 4)
        return hipErrorInvalidValue;
    const long long blocks = ((long long)batch * T * (C / 4) + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample_dw_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, w, y, (long long)batch * T,
                       (int)T, C / 4, x_bstride);
    return hipGetLastError();
}

hipError_t launch_upsample_dw(const float* x, const float* w, float* y, int batch, long long T, int C, hipStream_t s,
                              const int* tlen, const int* toff) {
    if (batch <= 0 || T <= 0 || T > 0x7fffffffLL || C <= 0 || C % 4 || !x || !w || !y || !tlen != !toff ||
        (tlen && batch > 65535))
        return hipErrorInvalidValue;
    const long long n = (tlen ? 1 : (long long)batch) * T * (C / 4);  // threads along x: ragged items go along y
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (tlen)
        hipLaunchKernelGGL(upsample_dw_ragged_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, s, x, w, y,
                           C / 4, tlen, toff);
    else
        hipLaunchKernelGGL(upsample_dw_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, w, y, (long long)batch * T,
                           (int)T, C / 4);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// x [B][L][64] (already ELU'd by the last residual block's epilogue) -> y [B][L]:
//   y[l] = bias + sum_{k < 3} sum_{c < 64} w[k][c] x[l - 2 + k][c],  x[< 0] = 0       (the mirror of conv0)
// A streaming reduction over 192 values per sample, 256 B of input per sample: HBM-bound.  A workgroup takes a
// contiguous tile of FC_TILE samples: its FC_TILE + 2 rows go to LDS with 16-B loads, consecutive lanes on
// consecutive 16 B (a wave reads 1 KiB = 4 whole rows per load); then thread i reads its three rows from LDS (row
// stride 68 floats: conflict-free ds_read_b128) against the weights (LDS broadcasts) in four running sums.
// RG: x [sum llen][64] packed -> y [B][Ls] padded (Ls = y's row stride); samples >= llen[b] of row b are left untouched.
// ------------------------------------------------------------------------------------------------
constexpr int FC_TILE = 128, FC_C = 64, FC_LD = 68;

// HS (a step of a decode stream): item b's L rows start at x + b * xbs and rows -2, -1 in front of them are the
// stream's carry: read instead of zeros.  y as the uniform form.
template <bool RG, bool HS = false>
__device__ __forceinline__ void final_conv_body(const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ bias, float* __restrict__ y, long long Ls,
                                                const int* __restrict__ llen, const int* __restrict__ loff,
                                                long long xbs = 0) {
    __shared__ __attribute__((aligned(16))) float xs[(FC_TILE + 2) * FC_LD];
    __shared__ __attribute__((aligned(16))) float ws[3 * FC_C];
    const int tid = threadIdx.x;
    const long long l0 = (long long)blockIdx.x * FC_TILE;
    long long L;
    const float* __restrict__ xb;
    if constexpr (RG) {
        L = llen[blockIdx.y];
        if (l0 >= L) return;
        xb = x + (long long)loff[blockIdx.y] * FC_C;
    } else {
        L = Ls;  // every item fills its row
        xb = x + (long long)blockIdx.y * (HS ? xbs : L * FC_C);
    }
    for (int i = tid; i < 3 * FC_C; i += FC_TILE) ws[i] = w[i];
    for (int idx = tid; idx < (FC_TILE + 2) * (FC_C / 4); idx += FC_TILE) {
        const int r = idx >> 4, c4 = idx & 15;
        const long long g = l0 - 2 + r;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g >= (HS ? -2 : 0) && g < L) v = *reinterpret_cast<const f32x4*>(xb + g * FC_C + 4 * c4);
        *reinterpret_cast<f32x4*>(xs + r * FC_LD + 4 * c4) = v;
    }
    __syncthreads();
    const long long l = l0 + tid;
    if (l >= L) return;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c4 = 0; c4 < FC_C / 4; ++c4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + (tid + k) * FC_LD + 4 * c4);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + k * FC_C + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(xv[e], wv[e], acc[e]);
        }
    y[(long long)blockIdx.y * Ls + l] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + bias[0];
}

__global__ __launch_bounds__(FC_TILE) void final_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y,
                                                             long long L) {
    final_conv_body<false>(x, w, bias, y, L, nullptr, nullptr);
}

__global__ __launch_bounds__(FC_TILE) void final_conv_ragged_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ y,
                                                                    long long Ls, const int* __restrict__ llen,
                                                                    const int* __restrict__ loff) {
    final_conv_body<true>(x, w, bias, y, Ls, llen, loff);
}

__global__ __launch_bounds__(FC_TILE) void final_conv_hist_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ y,
                                                                  long long L, long long xbs) {
    final_conv_body<false, true>(x, w, bias, y, L, nullptr, nullptr, xbs);
}

// RG and HS together (a ragged step of a decode stream): item b's llen[b] rows start at row loff[b] of x with its two
// carry rows in front of them; y the caller's padded [B][Ls], samples >= llen[b] of row b left untouched
__global__ __launch_bounds__(FC_TILE) void final_conv_hist_ragged_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ w,
                                                                         const float* __restrict__ bias,
                                                                         float* __restrict__ y, long long Ls,
                                                                         const int* __restrict__ llen,
                                                                         const int* __restrict__ loff) {
    final_conv_body<true, true>(x, w, bias, y, Ls, llen, loff);
}

hipError_t launch_final_conv_hist_ragged(const float* x, const float* w, const float* bias, float* y, int batch,
                                         long long Ls, int C, int ksize, const int* llen, const int* loff,
                                         long long max_llen, hipStream_t s) {
    if (C != FC_C || ksize != 3 || batch <= 0 || batch > 65535 || Ls <= 0 || !x || !w || !bias || !y || !llen || !loff ||
        max_llen <= 0 || max_llen > Ls)
        return hipErrorInvalidValue;
    const long long tiles = (max_llen + FC_TILE - 1) / FC_TILE;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(final_conv_hist_ragged_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(FC_TILE), 0, s, x, w,
                       bias, y, Ls, llen, loff);
    return hipGetLastError();
}

hipError_t launch_final_conv_hist(const float* x, const float* w, const float* bias, float* y, int batch, long long L,
                                  int C, int ksize, long long x_bstride, hipStream_t s) {
    if (C != FC_C || ksize != 3 || batch <= 0 || batch > 65535 || L <= 0 || !x || !w || !bias || !y ||
        x_bstride < (L + 2) * FC_C || x_bstride % 4)
        return hipErrorInvalidValue;
    const long long tiles = (L + FC_TILE - 1) / FC_TILE;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(final_conv_hist_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(FC_TILE), 0, s, x, w, bias, y,
                       L, x_bstride);
    return hipGetLastError();
}

hipError_t launch_final_conv(const float* x, const float* w, const float* bias, float* y, int batch, long long L, int C,
                             int ksize, hipStream_t s, const int* llen, const int* loff, long long max_llen) {
    if (C != FC_C || ksize != 3 || batch <= 0 || batch > 65535 || L <= 0 || !x || !w || !bias || !y || !llen != !loff ||
        (llen && (max_llen <= 0 || max_llen > L)))
        return hipErrorInvalidValue;
    const long long tiles = ((llen ? max_llen : L) + FC_TILE - 1) / FC_TILE;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)batch);
    if (llen)
        hipLaunchKernelGGL(final_conv_ragged_kernel, grid, dim3(FC_TILE), 0, s, x, w, bias, y, L, llen, loff);
    else
        hipLaunchKernelGGL(final_conv_kernel, grid, dim3(FC_TILE), 0, s, x, w, bias, y, L);
    return hipGetLastError();
}

}  // namespace mimi
