// Streamed decode (mimi_decode_stream_*, engine.cpp "decode stream"): the attention of one step against a ring of the
// past rows' rotated keys and values, and the strided copies that move the stages' carries.
//
//   attention_stream_kernel         a step's R = 2n query rows per (item, head) at absolute rows pos0 .. pos0 + R - 1
//   attention_stream_append_kernel  the step's k / v rows into their ring slots (row r in slot r % cap)
//   stream_carry_kernel             n strided copies in one launch, from a by-value table
//   stream_ds_rows_kernel           (encode stream) the transformer's rows behind the downsample's carry, which on an
//                                   item at row 0 is two copies of its first row (replicate padding)
// and under the same bodies their slot forms (SL: a step over a subset of the stream's slots, each slot at its own
// position): item b of the step takes its first row from pos_tab[b] and its rings / carries from slot slot_tab[b];
// the step's own rows in the workspace stay indexed by b.  The tables are device memory (a step may list 65535 slots).
// A RAGGED step (every listed slot its own number of frames; engine.cpp StreamLayout) packs the items' rows: item b's
// rlen[b] rows start at row roff[b] of qkv / out.  attention_stream_ragged_kernel is the slot body with the item's rows
// and first row from those tables (the grid covers the longest item; a wave past its item's rows exits before any load
// of a row); attention_stream_append_ragged_kernel runs a 2-D grid with the item uniform per workgroup;
// stream_carry_ragged_kernel takes both sides' element offsets and the count per (copy, item) from tables the host
// worked out.  Lane assignment, fmaf chains, butterfly and P.V order stay functions of the absolute row alone, so a
// row's bits are those of the slot form.
// One launcher per body (launch_attention_stream, launch_attention_stream_append, launch_stream_carry,
// launch_stream_ds_rows): null tables launch the lock-step kernel at the scalar pos0, non-null tables the slot kernel,
// and *kname receives the name of the one launched.
//
// CHUNKING DOES NOT MOVE A BIT.  Query row a (absolute) attends keys jlo = max(0, a - W + 1) .. a.  One WAVE owns the
// row.  Key jlo + t belongs to lane t % 64; a lane's score is one fmaf chain over d = 0 .. 63; the maximum is exact
// whatever its order; lane l sums its exp(s - m) for t = l, l + 64, ... in that order and the 64 partial sums go
// through one xor butterfly; P.V is, per output dim d = lane, one fmaf chain over t = 0 .. a - jlo, oldest key first.
// Every one of these orders is a function of a alone: not of pos0 (where the chunk starts), not of R (how long it
// is), not of the ring slot a key sits in, nor of whether a key is read from the ring or from the step's own rows
// (the ring holds copies of the very words the q/k/v GEMM stored).  So a row's output is the same bits under any
// split of the sequence into steps.  For the same reason the slot form moves no bit: giving every item of a step its
// own pos0 and its own ring changes where a row's keys are read from, never which keys nor in which order.
//
// Scores live in the wave's own slice of LDS (W floats): written and read by the same wave, LDS order, no barrier;
// waves without a row exit before any load.
#include "kernels.h"

namespace mimi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// SL: pos0 is pos_tab[b] and the ring is slot slot_tab[b]'s; b = blockIdx.z is uniform, so both are scalar loads
// RG (a ragged step: SL with a frame count per item): item b has rlen[b] rows starting at row roff[b] of the packed
// qkv / out; the grid covers the longest item and a wave past its item's rows exits before any load of a row
template <bool SL, bool RG = false>
__device__ __forceinline__ void attention_stream_body(float* sc_all, const float* __restrict__ qkv,
                                                      const float* __restrict__ kring,
                                                      const float* __restrict__ vring, float* __restrict__ out, int R,
                                                      int H, int window, int cap, long long pos0,
                                                      const long long* __restrict__ pos_tab,
                                                      const int* __restrict__ slot_tab, float scale,
                                                      const int* __restrict__ rlen = nullptr,
                                                      const int* __restrict__ roff = nullptr) {
    static_assert(SL || !RG, "a ragged step is a slot step");
    constexpr int D = 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;  // the query's row in the step
    if constexpr (!RG)
        if (i >= R) return;
    const int h = blockIdx.y, b = blockIdx.z;
    long long r0 = (long long)b * R;  // the item's first row in qkv / out
    if constexpr (RG) {
        if (i >= rlen[b]) return;
        r0 = roff[b];
    }
    int rb = b;  // the item's place among the rings
    if constexpr (SL) {
        pos0 = pos_tab[b];
        rb = slot_tab[b];
    }
    float* sc = sc_all + wave * window;
    const long long ld = 3LL * H * D;
    const float* step = qkv + r0 * ld;                            // the item's rows of this step
    const long long ring = ((long long)rb * H + h) * cap * D;     // the (item, head)'s ring
    const long long a = pos0 + i;
    const long long jlo = a - window + 1 > 0 ? a - window + 1 : 0;
    const int cnt = (int)(a - jlo) + 1;  // 1 .. window keys, oldest first
    // row j's key / value: the step's own rows from pos0 on, the ring before
    auto krow = [&](long long j) {
        return j >= pos0 ? step + (j - pos0) * ld + (long long)H * D + h * D : kring + ring + (j % cap) * D;
    };
    auto vrow = [&](long long j) {
        return j >= pos0 ? step + (j - pos0) * ld + 2LL * H * D + h * D : vring + ring + (j % cap) * D;
    };

    f32x4 q[D / 4];
    {
        const float* qr = step + (long long)i * ld + h * D;
#pragma unroll
        for (int c = 0; c < D / 4; ++c) q[c] = *reinterpret_cast<const f32x4*>(qr + 4 * c) * scale;
    }
    float m = -INFINITY;
    for (int t = lane; t < cnt; t += 64) {
        const float* kr = krow(jlo + t);
        f32x4 kv[D / 4];
#pragma unroll
        for (int c = 0; c < D / 4; ++c) kv[c] = *reinterpret_cast<const f32x4*>(kr + 4 * c);
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < D / 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_fmaf(q[c][e], kv[c][e], s);
        sc[t] = s;
        m = fmaxf(m, s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));  // (lane 0 always has key jlo: m is finite)
    float l = 0.0f;
    for (int t = lane; t < cnt; t += 64) {
        const float p = __expf(sc[t] - m);
        sc[t] = p;
        l += p;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) l += __shfl_xor(l, o);
    // P.V: lane = output dim; a wave reads one 256-B value row per key, four rows in flight
    float acc = 0.0f;
    int t = 0;
    for (; t + 4 <= cnt; t += 4) {
        const float v0 = vrow(jlo + t)[lane], v1 = vrow(jlo + t + 1)[lane];
        const float v2 = vrow(jlo + t + 2)[lane], v3 = vrow(jlo + t + 3)[lane];
        acc = __builtin_fmaf(sc[t], v0, acc);
        acc = __builtin_fmaf(sc[t + 1], v1, acc);
        acc = __builtin_fmaf(sc[t + 2], v2, acc);
        acc = __builtin_fmaf(sc[t + 3], v3, acc);
    }
    for (; t < cnt; ++t) acc = __builtin_fmaf(sc[t], vrow(jlo + t)[lane], acc);
    out[(r0 + i) * (H * D) + h * D + lane] = acc * (1.0f / l);
}

__global__ __launch_bounds__(256) void attention_stream_kernel(const float* __restrict__ qkv,
                                                               const float* __restrict__ kring,
                                                               const float* __restrict__ vring,
                                                               float* __restrict__ out, int R, int H, int window,
                                                               int cap, long long pos0, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sc_all[];
    attention_stream_body<false>(sc_all, qkv, kring, vring, out, R, H, window, cap, pos0, nullptr, nullptr, scale);
}

__global__ __launch_bounds__(256) void attention_stream_slots_kernel(const float* __restrict__ qkv,
                                                                     const float* __restrict__ kring,
                                                                     const float* __restrict__ vring,
                                                                     float* __restrict__ out, int R, int H, int window,
                                                                     int cap, const long long* __restrict__ pos_tab,
                                                                     const int* __restrict__ slot_tab, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sc_all[];
    attention_stream_body<true>(sc_all, qkv, kring, vring, out, R, H, window, cap, 0, pos_tab, slot_tab, scale);
}

__global__ __launch_bounds__(256) void attention_stream_ragged_kernel(const float* __restrict__ qkv,
                                                                      const float* __restrict__ kring,
                                                                      const float* __restrict__ vring,
                                                                      float* __restrict__ out, int H, int window, int cap,
                                                                      const long long* __restrict__ pos_tab,
                                                                      const int* __restrict__ slot_tab,
                                                                      const int* __restrict__ rlen,
                                                                      const int* __restrict__ roff, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sc_all[];
    attention_stream_body<true, true>(sc_all, qkv, kring, vring, out, 0, H, window, cap, 0, pos_tab, slot_tab, scale,
                                      rlen, roff);
}

// pos_tab / slot_tab both null: the lock-step kernel at pos0; both set: the slot kernel (pos0 unused)
hipError_t launch_attention_stream(const float* qkv, const float* kring, const float* vring, float* out, int batch,
                                   int R, int H, int D, int window, int cap, long long pos0, const long long* pos_tab,
                                   const int* slot_tab, float scale, hipStream_t s, const char** kname) {
    const bool sl = pos_tab || slot_tab;
    if (D != 64 || batch <= 0 || batch > 65535 || R <= 0 || H <= 0 || H > 65535 || window < 1 || cap < window - 1 ||
        cap < 1 || (sl ? !pos_tab || !slot_tab : pos0 < 0) || !qkv || !kring || !vring || !out)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)4 * window * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((R + 3) / 4), (unsigned)H, (unsigned)batch);
    if (sl)
        hipLaunchKernelGGL(attention_stream_slots_kernel, grid, dim3(256), lds, s, qkv, kring, vring, out, R, H, window,
                           cap, pos_tab, slot_tab, scale);
    else
        hipLaunchKernelGGL(attention_stream_kernel, grid, dim3(256), lds, s, qkv, kring, vring, out, R, H, window, cap,
                           pos0, scale);
    if (kname) *kname = sl ? "mimi::attention_stream_slots_kernel" : "mimi::attention_stream_kernel";
    return hipGetLastError();
}

// the ragged step: R = the longest item's rows (the grid); every table holds `batch` entries checked by the caller
hipError_t launch_attention_stream_ragged(const float* qkv, const float* kring, const float* vring, float* out,
                                          int batch, int R, int H, int D, int window, int cap, const long long* pos_tab,
                                          const int* slot_tab, const int* rlen, const int* roff, float scale,
                                          hipStream_t s, const char** kname) {
    if (D != 64 || batch <= 0 || batch > 65535 || R <= 0 || H <= 0 || H > 65535 || window < 1 || cap < window - 1 ||
        cap < 1 || !pos_tab || !slot_tab || !rlen || !roff || !qkv || !kring || !vring || !out)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)4 * window * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((R + 3) / 4), (unsigned)H, (unsigned)batch);
    hipLaunchKernelGGL(attention_stream_ragged_kernel, grid, dim3(256), lds, s, qkv, kring, vring, out, H, window, cap,
                       pos_tab, slot_tab, rlen, roff, scale);
    if (kname) *kname = "mimi::attention_stream_ragged_kernel";
    return hipGetLastError();
}

// one thread per 16 B of the step's k and v rows: [b][row][k | v][head][16 float4]
// SL: item b's rows go to slot slot_tab[b], ring index (pos_tab[b] + i) % cap
template <bool SL>
__device__ __forceinline__ void attention_stream_append_body(const float* __restrict__ qkv, float* __restrict__ kring,
                                                             float* __restrict__ vring, int batch, int R, int H, int cap,
                                                             long long pos0, const long long* __restrict__ pos_tab,
                                                             const int* __restrict__ slot_tab) {
    constexpr int D = 64;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)batch * R * 2 * H * (D / 4);
    if (idx >= total) return;
    const int c4 = (int)(idx % (D / 4));
    long long r = idx / (D / 4);
    const int h = (int)(r % H);
    r /= H;
    const int kv = (int)(r % 2);
    r /= 2;
    const int i = (int)(r % R);
    const int b = (int)(r / R);
    int rb = b;  // b < batch here: idx < total
    if constexpr (SL) {
        pos0 = pos_tab[b];
        rb = slot_tab[b];
    }
    const float* src = qkv + ((long long)b * R + i) * (3LL * H * D) + (long long)(1 + kv) * H * D + h * D + 4 * c4;
    float* dst = (kv ? vring : kring) + (((long long)rb * H + h) * cap + (pos0 + i) % cap) * D + 4 * c4;
    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
}

__global__ __launch_bounds__(256) void attention_stream_append_kernel(const float* __restrict__ qkv,
                                                                      float* __restrict__ kring,
                                                                      float* __restrict__ vring, int batch, int R, int H,
                                                                      int cap, long long pos0) {
    attention_stream_append_body<false>(qkv, kring, vring, batch, R, H, cap, pos0, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void attention_stream_append_slots_kernel(const float* __restrict__ qkv,
                                                                            float* __restrict__ kring,
                                                                            float* __restrict__ vring, int batch, int R,
                                                                            int H, int cap,
                                                                            const long long* __restrict__ pos_tab,
                                                                            const int* __restrict__ slot_tab) {
    attention_stream_append_body<true>(qkv, kring, vring, batch, R, H, cap, 0, pos_tab, slot_tab);
}

hipError_t launch_attention_stream_append(const float* qkv, float* kring, float* vring, int batch, int R, int H, int D,
                                          int cap, long long pos0, const long long* pos_tab, const int* slot_tab,
                                          hipStream_t s, const char** kname) {
    const bool sl = pos_tab || slot_tab;
    // R <= cap: no two rows of the step share a slot
    if (D != 64 || batch <= 0 || R <= 0 || R > cap || H <= 0 || (sl ? !pos_tab || !slot_tab : pos0 < 0) || !qkv ||
        !kring || !vring)
        return hipErrorInvalidValue;
    const long long total = (long long)batch * R * 2 * H * (D / 4);
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (sl)
        hipLaunchKernelGGL(attention_stream_append_slots_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qkv, kring,
                           vring, batch, R, H, cap, pos_tab, slot_tab);
    else
        hipLaunchKernelGGL(attention_stream_append_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qkv, kring, vring,
                           batch, R, H, cap, pos0);
    if (kname) *kname = sl ? "mimi::attention_stream_append_slots_kernel" : "mimi::attention_stream_append_kernel";
    return hipGetLastError();
}

// The ragged step's append: item b = blockIdx.y (uniform per workgroup: its table entries are scalar loads) has rlen[b]
// rows at row roff[b] of the packed qkv; blockIdx.x covers the longest item's [row][k | v][head][16 float4] and a thread
// past its item's exits before any load of a row.
__global__ __launch_bounds__(256) void attention_stream_append_ragged_kernel(
    const float* __restrict__ qkv, float* __restrict__ kring, float* __restrict__ vring, int H, int cap,
    const long long* __restrict__ pos_tab, const int* __restrict__ slot_tab, const int* __restrict__ rlen,
    const int* __restrict__ roff) {
    constexpr int D = 64;
    const int b = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rlen[b] * 2 * H * (D / 4)) return;
    const int c4 = (int)(idx % (D / 4));
    long long r = idx / (D / 4);
    const int h = (int)(r % H);
    r /= H;
    const int kv = (int)(r % 2);
    const int i = (int)(r / 2);
    const long long pos0 = pos_tab[b];
    const int rb = slot_tab[b];
    const float* src = qkv + ((long long)roff[b] + i) * (3LL * H * D) + (long long)(1 + kv) * H * D + h * D + 4 * c4;
    float* dst = (kv ? vring : kring) + (((long long)rb * H + h) * cap + (pos0 + i) % cap) * D + 4 * c4;
    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
}

// R = the longest item's rows (the grid; R <= cap: no two rows of an item share a ring slot)
hipError_t launch_attention_stream_append_ragged(const float* qkv, float* kring, float* vring, int batch, int R, int H,
                                                 int D, int cap, const long long* pos_tab, const int* slot_tab,
                                                 const int* rlen, const int* roff, hipStream_t s, const char** kname) {
    if (D != 64 || batch <= 0 || batch > 65535 || R <= 0 || R > cap || H <= 0 || !pos_tab || !slot_tab || !rlen ||
        !roff || !qkv || !kring || !vring)
        return hipErrorInvalidValue;
    const long long blocks = ((long long)R * 2 * H * (D / 4) + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_stream_append_ragged_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, s,
                       qkv, kring, vring, H, cap, pos_tab, slot_tab, rlen, roff);
    if (kname) *kname = "mimi::attention_stream_append_ragged_kernel";
    return hipGetLastError();
}

// copy blockIdx.z of the table, item blockIdx.y; 16 B per thread, grid-stride along x
// SL: the stream's side of the copy (c.state) is slot slot_tab[item]'s, the workspace side the item's
template <bool SL>
__device__ __forceinline__ void stream_carry_body(const CarryTable& t, const int* __restrict__ slot_tab) {
    const CarryCopy& c = t.c[blockIdx.z];
    long long sb = blockIdx.y, db = blockIdx.y;
    if constexpr (SL) {
        const int slot = slot_tab[blockIdx.y];
        if (c.state == CARRY_STATE_SRC) sb = slot;
        if (c.state == CARRY_STATE_DST) db = slot;
    }
    const float* __restrict__ src = c.src + sb * c.src_bstride;
    float* __restrict__ dst = c.dst + db * c.dst_bstride;
    const int n4 = c.count / 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256)
        *reinterpret_cast<f32x4*>(dst + 4LL * i) = *reinterpret_cast<const f32x4*>(src + 4LL * i);
}

__global__ __launch_bounds__(256) void stream_carry_kernel(CarryTable t) { stream_carry_body<false>(t, nullptr); }

__global__ __launch_bounds__(256) void stream_carry_slots_kernel(CarryTable t, const int* __restrict__ slot_tab) {
    stream_carry_body<true>(t, slot_tab);
}

hipError_t launch_stream_carry(const CarryTable& t, int batch, const int* slot_tab, hipStream_t s, const char** kname) {
    if (t.n < 1 || t.n > CARRY_MAX || batch <= 0 || batch > 65535) return hipErrorInvalidValue;
    int most = 0;
    for (int d = 0; d < t.n; ++d) {
        const CarryCopy& c = t.c[d];
        if (!c.src || !c.dst || c.count <= 0 || c.count % 4 || c.src_bstride % 4 || c.dst_bstride % 4 ||
            (reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst)) % 16)
            return hipErrorInvalidValue;
        most = c.count > most ? c.count : most;
    }
    const int blocks = (most / 4 + 255) / 256;
    const dim3 grid((unsigned)(blocks < 64 ? blocks : 64), (unsigned)batch, (unsigned)t.n);
    if (slot_tab)
        hipLaunchKernelGGL(stream_carry_slots_kernel, grid, dim3(256), 0, s, t, slot_tab);
    else
        hipLaunchKernelGGL(stream_carry_kernel, grid, dim3(256), 0, s, t);
    if (kname) *kname = slot_tab ? "mimi::stream_carry_slots_kernel" : "mimi::stream_carry_kernel";
    return hipGetLastError();
}

// The ragged step's copies: copy d of the table moves, for item b, cnt[d][b] floats (a multiple of 4, 0 allowed) from
// t.c[d].src + off[d][0][b] to t.c[d].dst + off[d][1][b] -- element offsets the host worked out for both sides (the
// state side: the item's slot; the workspace side: the item's block in the packed tensor), so the kernel indexes by
// nothing but the item's place.  off: [t.n][2][batch] int64, cnt: [t.n][batch] int32, device memory.
__global__ __launch_bounds__(256) void stream_carry_ragged_kernel(CarryTable t, const long long* __restrict__ off,
                                                                  const int* __restrict__ cnt) {
    const int d = blockIdx.z, b = blockIdx.y, m = gridDim.y;
    const CarryCopy& c = t.c[d];
    const float* __restrict__ src = c.src + off[((long long)d * 2) * m + b];
    float* __restrict__ dst = c.dst + off[((long long)d * 2 + 1) * m + b];
    const int n4 = cnt[(long long)d * m + b] / 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256)
        *reinterpret_cast<f32x4*>(dst + 4LL * i) = *reinterpret_cast<const f32x4*>(src + 4LL * i);
}

// most: the largest count of any (copy, item), which sizes the grid; the caller has checked every offset and count
// (multiples of 4 inside their buffers)
hipError_t launch_stream_carry_ragged(const CarryTable& t, int batch, const long long* off, const int* cnt, int most,
                                      hipStream_t s, const char** kname) {
    if (t.n < 1 || t.n > CARRY_MAX || batch <= 0 || batch > 65535 || !off || !cnt || most <= 0 || most % 4)
        return hipErrorInvalidValue;
    for (int d = 0; d < t.n; ++d)
        if (!t.c[d].src || !t.c[d].dst ||
            (reinterpret_cast<uintptr_t>(t.c[d].src) | reinterpret_cast<uintptr_t>(t.c[d].dst)) % 16)
            return hipErrorInvalidValue;
    const int blocks = (most / 4 + 255) / 256;
    const dim3 grid((unsigned)(blocks < 64 ? blocks : 64), (unsigned)batch, (unsigned)t.n);
    hipLaunchKernelGGL(stream_carry_ragged_kernel, grid, dim3(256), 0, s, t, off, cnt);
    if (kname) *kname = "mimi::stream_carry_ragged_kernel";
    return hipGetLastError();
}

// Encode stream: item b's R transformer rows (flat [batch][R][C]) go behind the downsample's 2 carry rows in
// dst [batch][2 + R][C].  An item whose first row is absolute row 0 -- a fresh or reset slot -- has no past: its two
// carry rows are copies of its row 0 (the reference pads the downsample with mode = "replicate"), written here over
// whatever carry-in put there.  16 B per thread; the row of dst is uniform per 16 B, the position per workgroup.
// SL: the item's position is pos_tab[b] (b = blockIdx.y is uniform: a scalar load); both sides stay indexed by b.
template <bool SL>
__device__ __forceinline__ void stream_ds_rows_body(const float* __restrict__ src, float* __restrict__ dst, int R, int C,
                                                    long long pos0, const long long* __restrict__ pos_tab) {
    const int b = blockIdx.y;
    if constexpr (SL) pos0 = pos_tab[b];
    const bool fresh = pos0 == 0;
    const int c4 = C / 4;
    const long long n4 = (long long)(2 + R) * c4;
    const float* __restrict__ sb = src + (long long)b * R * C;
    float* __restrict__ db = dst + (long long)b * (2 + R) * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long r = i / c4;  // the row of dst: 0, 1 the carry, 2 + j row j of the step
        const int c = (int)(i % c4) * 4;
        if (r < 2 && !fresh) continue;
        const long long sr = r < 2 ? 0 : r - 2;
        *reinterpret_cast<f32x4*>(db + r * C + c) = *reinterpret_cast<const f32x4*>(sb + sr * C + c);
    }
}

__global__ __launch_bounds__(256) void stream_ds_rows_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int R, int C, long long pos0) {
    stream_ds_rows_body<false>(src, dst, R, C, pos0, nullptr);
}

__global__ __launch_bounds__(256) void stream_ds_rows_slots_kernel(const float* __restrict__ src,
                                                                   float* __restrict__ dst, int R, int C,
                                                                   const long long* __restrict__ pos_tab) {
    stream_ds_rows_body<true>(src, dst, R, C, 0, pos_tab);
}

// The ragged step's form: item b's rlen[b] rows at row roff[b] of the packed src, its block [2 + rlen[b]][C] at row
// doff[b] of dst; the replicate fill is per item, from the item's own position and its own first row.
__global__ __launch_bounds__(256) void stream_ds_rows_ragged_kernel(const float* __restrict__ src,
                                                                    float* __restrict__ dst, int C,
                                                                    const long long* __restrict__ pos_tab,
                                                                    const int* __restrict__ rlen,
                                                                    const int* __restrict__ roff,
                                                                    const int* __restrict__ doff) {
    const int b = blockIdx.y;
    const bool fresh = pos_tab[b] == 0;
    const int c4 = C / 4;
    const long long n4 = (long long)(2 + rlen[b]) * c4;
    const float* __restrict__ sb = src + (long long)roff[b] * C;
    float* __restrict__ db = dst + (long long)doff[b] * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long r = i / c4;
        const int c = (int)(i % c4) * 4;
        if (r < 2 && !fresh) continue;
        const long long sr = r < 2 ? 0 : r - 2;
        *reinterpret_cast<f32x4*>(db + r * C + c) = *reinterpret_cast<const f32x4*>(sb + sr * C + c);
    }
}

hipError_t launch_stream_ds_rows_ragged(const float* src, float* dst, int batch, int max_R, int C,
                                        const long long* pos_tab, const int* rlen, const int* roff, const int* doff,
                                        hipStream_t s, const char** kname) {
    if (!src || !dst || batch <= 0 || batch > 65535 || max_R <= 0 || C <= 0 || C % 4 || !pos_tab || !rlen || !roff ||
        !doff || (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16)
        return hipErrorInvalidValue;
    const long long blocks = ((long long)(2 + max_R) * (C / 4) + 255) / 256;
    const dim3 grid((unsigned)(blocks < 64 ? blocks : 64), (unsigned)batch);
    hipLaunchKernelGGL(stream_ds_rows_ragged_kernel, grid, dim3(256), 0, s, src, dst, C, pos_tab, rlen, roff, doff);
    if (kname) *kname = "mimi::stream_ds_rows_ragged_kernel";
    return hipGetLastError();
}

hipError_t launch_stream_ds_rows(const float* src, float* dst, int batch, int R, int C, long long pos0,
                                 const long long* pos_tab, hipStream_t s, const char** kname) {
    if (!src || !dst || batch <= 0 || batch > 65535 || R <= 0 || C <= 0 || C % 4 ||
        (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 || (!pos_tab && pos0 < 0))
        return hipErrorInvalidValue;
    const long long blocks = ((long long)(2 + R) * (C / 4) + 255) / 256;
    const dim3 grid((unsigned)(blocks < 64 ? blocks : 64), (unsigned)batch);
    if (pos_tab)
        hipLaunchKernelGGL(stream_ds_rows_slots_kernel, grid, dim3(256), 0, s, src, dst, R, C, pos_tab);
    else
        hipLaunchKernelGGL(stream_ds_rows_kernel, grid, dim3(256), 0, s, src, dst, R, C, pos0);
    if (kname) *kname = pos_tab ? "mimi::stream_ds_rows_slots_kernel" : "mimi::stream_ds_rows_kernel";
    return hipGetLastError();
}

}  // namespace mimi
