// 256 x 256 tile of the fp16-planes GEMM (PREC_F16X3: 2 planes per operand, 3 products, v_mfma_f32_16x16x32_f16) on a
// staggered, phase-interleaved schedule.  Uniform batches only (no ragged rows, no LayerNorm prologue).  Included by
// gemm.hip and tools/gemm_bench.hip.
//
// Geometry: 8 waves as 2 (M) x 4 (N), each owning 128 x 64 outputs (acc[8][4] of f32x4); 512 threads, one workgroup per
// CU, no loader waves: every wave issues 2 of the 16 1-KiB LDS-DMA pieces of each half-tile.  BK = 32.
//
// LDS ring: 2 K steps x 4 half-tiles x 16 KiB.  A half-tile holds both planes of 128 image rows x 64 B, in the order
// the waves consume them within a K step (wm = wave / 4, wn = wave % 4):
//   r = 0  Bs0: image row wn * 32 + x = tile column wn * 64 + x        (x < 32)   read in phase 0
//   r = 1  As0: image row wm * 64 + y = tile row    wm * 128 + y       (y < 64)   read in phase 0
//   r = 2  Bs1: image row wn * 32 + x = tile column wn * 64 + 32 + x              read in phase 1
//   r = 3  As1: image row wm * 64 + y = tile row    wm * 128 + 64 + y             read in phase 2
// so each half-tile is read in exactly one phase of its K step.  Rows are chunk-swizzled as chunk_swz<32, 16>
// (gemm_planes.h), applied on the DMA source address and on the fragment read.
//
// Schedule: 4 phases per K step, one per quadrant (64 x 32) of the wave's block -- (As0, Bs0), (As0, Bs1), (As1, Bs1),
// (As1, Bs0); A and B fragments stay in registers across the phases that share them (12 + 4 + 8 + 0 ds_read_b128 per
// K step for 96 MFMAs).  A phase is: fragment reads, this wave's 2 pieces of one half-tile, counted vmcnt, raw
// s_barrier, lgkmcnt(0), 24 MFMAs under s_setprio(1), raw s_barrier.  Waves 4-7 (the SIMD partners of waves 0-3) pass
// one extra barrier before the loop and waves 0-3 one after it, so one group's MFMAs run over the other group's
// fragment reads and DMA issue.
//
// Counts.  Number the half-tiles h = 4 kt + r in issue order and the phases p = 4 kt + q; G0 = waves 0-3, G1 = 4-7;
// the workgroup's barriers g = 0, 1, ...: G0 runs phase p between barriers 2p - 1 and 2p + 1 (reads before 2p, MFMAs
// after), G1 between 2p and 2p + 2.
//   issue:  phase p issues half-tile h = p + 6 (the prologue issues h = 0 .. 5).
//   RAW:    after its issue, phase p waits until this wave's pieces of every h <= p + 2 have landed (at most 4 younger
//           half-tiles, 8 pieces, stay in flight: vmcnt(8), less in the tail), BEFORE its first barrier.  Half-tile h is
//           read in phase h (r = 0) or h - 1 (r = 1, 2, 3), i.e. a read of phase p + 1 touches h <= p + 2: one whole
//           phase after the wait that retired it, which covers the delayed group too (G0's reads of phase p + 1 come
//           after barrier 2p + 1, where every G1 wave has done its phase-p wait; G1's after 2p + 2).
//   WAR:    half-tile h + 8 lands on h's bytes and is issued in phase h + 2, two phases after h's last read (phase <= h):
//           G1's reads of phase h are retired by its lgkmcnt(0) before barrier 2h + 2, G0 issues in phase h + 2 after
//           barrier 2h + 3, G1 after 2h + 4.
// The asm memory clobbers and sched_barriers pin the issue order those counts assume.
//
// Same bits as the kernels it replaces: the K-step order of KOrderT (FL_PAIR: the pair order of the tap-pair kernel --
// per chain start j, 128-B channel block, 32-channel half: tap j then tap j + s; here each tap's A half-tile is fetched
// on its own, the shared A image of the pair kernel does not fit the half-tile ring), per K step mma_split's product
// order on one accumulator per output starting from 0, and the epilogue text of gemm_planes_kernel
// (gemm_planes_epilogue.inc).
#pragma once
#include "gemm_planes.h"

namespace mimi {

// FL: FL_PAIR (K order of the k = 2s convs), FL_PERSIST (one workgroup per CU loops over the tiles; a tile's stores
// drain under the next tile's first stages), FL_SC1OUT, FL_DIAG_NODMA / FL_DIAG_NOMMA (tools/gemm_bench.hip)
template <int EPI, int OUTP, int TAG, int FL = 0>
__global__ __launch_bounds__(512) void gemm_planes256_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 256, BN = 256, BK = 32, MF = 16, NW = 8;
    constexpr int TM = 8, TN = 4;                // 16 x 16 tiles per wave: 128 x 64
    constexpr int PL = 128 * BK;                 // fp16 per plane of a half-tile
    constexpr int HT = 2 * PL;                   // fp16 per half-tile (16 KiB)
    constexpr int RING = 8 * HT;                 // 2 K steps x 4 half-tiles (128 KiB)
    constexpr bool PAIR = (FL & FL_PAIR) != 0;
    constexpr int ONS = OUTP & 7;
    constexpr int JH = 2, LDE = TN * MF / JH + 4;  // epilogue staging in 2 passes of 32 columns (144 KiB)
    constexpr int LDS_EL = RING > NW * TM * MF * LDE * 2 ? RING : NW * TM * MF * LDE * 2;
    static_assert(LDS_EL * 2 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) __bf16 lds[LDS_EL];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const bool late = wave >= 4;  // the delayed group: SIMD partners are waves w and w + 4
    const int M = p.M, N = p.N, K = p.K;
    const int MT = (M + BM - 1) / BM, NTn = (N + BN - 1) / BN;
    const int ntiles = MT * NTn * p.batch;
    const int KT = K / BK;        // >= 2 (checked by the launcher)
    const int NH = 4 * KT;        // half-tiles per tile
    const int ncg = (p.ncg > 1 && NTn % p.ncg == 0) ? p.ncg : 1;  // XCD column groups, as gemm_planes_kernel
    float omx = 0.0f;

    // DMA: this wave's pieces of a half-tile are image rows [16 wave, 16 wave + 16) of plane 0 and of plane 1
    const int prow = wave * 16 + (lane >> 2), pch = lane & 3;
    const int csrc = (pch ^ chunk_swz<BK, MF>(prow)) * 8;  // source chunk (elements) landing lane-linear
    const int a_trow = (prow >> 6) * 128 + (prow & 63);     // tile row of this lane's As0 row (As1: + 64)
    const int b_tcol = (prow >> 5) * 64 + (prow & 31);      // tile column of its Bs0 row (Bs1: + 32)
    const __bf16* __restrict__ Wp = reinterpret_cast<const __bf16*>(p.Wsplit);
    const int w_pl = N * K;  // (elements; the launcher checks 2 N K < 2^31)

    // fragment reads: image row of 16 x 16 tile 0 of this wave in an A / a B half-tile, and its chunk
    const int fr = lane & 15, hsel = lane >> 4;
    const int a_frag = (wm * 64 + fr) * BK + ((hsel ^ chunk_swz<BK, MF>(fr)) * 8);  // (+ i * 16 rows: same swizzle)
    const int b_frag = (wn * 32 + fr) * BK + ((hsel ^ chunk_swz<BK, MF>(fr)) * 8);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int b, mt, nt;
    {
        const int logical = xcd_remap(tile, ntiles);
        int rest;
        if (ncg > 1) {
            const int NG = NTn / ncg, per = ntiles / ncg;
            const int cg = logical / per, w = logical - cg * per;
            nt = cg * NG + w % NG;
            rest = w / NG;
        } else {
            nt = logical % NTn;
            rest = logical / NTn;
        }
        // (the divisions run on the VALU: back to SGPRs, or every buffer resource made from b sits in VGPRs and each
        // LDS-DMA becomes a readfirstlane loop)
        mt = __builtin_amdgcn_readfirstlane(rest % MT);
        b = __builtin_amdgcn_readfirstlane(rest / MT);
        nt = __builtin_amdgcn_readfirstlane(nt);
    }
    const int m0 = mt * BM, n0 = nt * BN;
    const __bf16* __restrict__ Abase = reinterpret_cast<const __bf16*>(p.Ap) + (long long)b * p.a_bstride;
    const __amdgpu_buffer_rsrc_t ars0 = make_rsrc(Abase, p.a_len * 2);
    const __amdgpu_buffer_rsrc_t ars1 = make_rsrc(Abase + p.a_pstride, p.a_len * 2);
    // byte offsets into an A plane (negative or past the end: the buffer range check loads 0 -- the causal padding;
    // rows past M only feed outputs that are never stored) and element offsets into the weight planes
    int a_src[2], b_src[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = m0 + a_trow + h * 64;
        a_src[h] = m < M ? (int)((p.a_off + (long long)m * p.a_rs + csrc) * 2) : -16;
        int n = n0 + b_tcol + h * 32;
        n = n < N ? n : N - 1;  // columns past N are never stored
        b_src[h] = n * K + csrc;
    }

    // K offsets in issue order: one per K step (4 half-tiles)
    KOrderT<BK> ko;
    ko.init(p, PAIR);
    const int ktap = PAIR ? ko.s * ko.cin : 0;  // K offset from a chain's first tap to its second
    int kstep = 0;
    auto k_of_issue = [&]() {  // the K offset (elements) of the K step being issued
        return PAIR ? ko.offset() + (kstep & 1) * ktap : ko.offset();
    };
    auto k_advance = [&]() {
        if (!PAIR || (kstep & 1)) ko.next();
        ++kstep;
    };
    // this wave's 2 pieces of half-tile h = 4 kt + r (r compile-time), K offset k0
    auto issue = [&](int slot, auto rc, int k0) {
        constexpr int r = decltype(rc)::value;
        __bf16* dst = lds + (slot * 4 + r) * HT + wave * 16 * BK;
        if constexpr (r & 1) {  // A
            const int off = a_src[r >> 1] + k0 * 2;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ars0, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ars1, (__attribute__((address_space(3))) void*)(dst + PL), 16, off,
                                                     0, 0, 0);
        } else {
            const __bf16* src = Wp + b_src[r >> 1] + k0;
            __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(src + w_pl), (__attribute__((address_space(3))) void*)(dst + PL),
                                             16, 0, 0);
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0f;

    // prologue: half-tiles 0 .. 5 (K step 0 and Bs0, As0 of K step 1), then 0 and 1 landed (4 younger in flight)
    {
        const int k0 = k_of_issue();
        k_advance();
        issue(0, std::integral_constant<int, 0>(), k0);
        issue(0, std::integral_constant<int, 1>(), k0);
        issue(0, std::integral_constant<int, 2>(), k0);
        issue(0, std::integral_constant<int, 3>(), k0);
    }
    int kiss = k_of_issue();  // K offset of the step whose half-tiles are being issued (K step 1 from here)
    k_advance();
    issue(1, std::integral_constant<int, 0>(), kiss);
    issue(1, std::integral_constant<int, 1>(), kiss);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (late) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    bf16x8 af[2][4], bf[2][2][2];  // A [plane][i] of the current 64-row half; B [column half][plane][j]
    auto read_a = [&](const __bf16* ht) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int i = 0; i < 4; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(ht + pl * PL + a_frag + i * 16 * BK);
    };
    auto read_b = [&](const __bf16* ht, int sb) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[sb][pl][j] = *reinterpret_cast<const bf16x8*>(ht + pl * PL + b_frag + j * 16 * BK);
    };
    // the 24 MFMAs of quadrant (sa, sb): per output tile mma_split's order -- lo x hi, hi x lo, hi x hi
    auto mma_quad = [&](auto sac, auto sbc) {
        constexpr int sa = decltype(sac)::value, sb = decltype(sbc)::value;
        if (FL & FL_DIAG_NOMMA) return;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x4& c = acc[sa * 4 + i][sb * 2 + j];
                c = mfma16<true>(af[1][i], bf[sb][0][j], c);
                c = mfma16<true>(af[0][i], bf[sb][1][j], c);
                c = mfma16<true>(af[0][i], bf[sb][0][j], c);
            }
    };
    // the part of a phase after its fragment reads: issue half-tile p + 6, counted wait, barrier, MFMAs, barrier
    auto phase_tail = [&](int pphase, int slot_iss, auto rc, auto sac, auto sbc) {
        const int h = pphase + 6;
        if (!(FL & FL_DIAG_NODMA) && h < NH) issue(slot_iss, rc, kiss);
        wait_stages<2, 4>(min(4, max(0, NH - 3 - pphase)));
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        mma_quad(sac, sbc);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;

    for (int kt = 0; kt < KT; ++kt) {
        const __bf16* st = lds + (kt & 1) * 4 * HT;  // this K step's half-tiles
        const int s1 = (kt + 1) & 1, s2 = kt & 1;    // ring slots of K steps kt + 1 and kt + 2
        const int p0 = 4 * kt;
        // phase 0: Bs0, As0 -> quadrant (0, 0); issues Bs1 of K step kt + 1
        read_b(st + 0 * HT, 0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(st + 1 * HT);
        asm volatile("" ::: "memory");
        phase_tail(p0 + 0, s1, I2(), I0(), I0());
        // phase 1: Bs1 -> quadrant (0, 1); issues As1 of K step kt + 1
        read_b(st + 2 * HT, 1);
        asm volatile("" ::: "memory");
        phase_tail(p0 + 1, s1, I3(), I0(), I1());
        // phase 2: As1 -> quadrant (1, 1); issues Bs0 of K step kt + 2
        read_a(st + 3 * HT);
        asm volatile("" ::: "memory");
        if (kt + 2 < KT) {
            kiss = k_of_issue();
            k_advance();
        }
        phase_tail(p0 + 2, s2, I0(), I1(), I1());
        // phase 3: quadrant (1, 0) on the Bs0 fragments of phase 0; issues As0 of K step kt + 2
        phase_tail(p0 + 3, s2, I1(), I1(), I0());
    }
    if (!late) __builtin_amdgcn_s_barrier();

    // ---- epilogue (gemm_planes.h): staged through the (now idle) ring, wave-private
    __syncthreads();
    {
    constexpr bool F16 = true;
    float* stg = reinterpret_cast<float*>(lds) + wave * (TM * MF * LDE);
    const long long cel = (long long)b * p.c_bstride;
    const int rbase = m0 + wm * TM * MF, cb0 = n0 + wn * TN * MF;
    const int Mb = M;
#include "gemm_planes_epilogue.inc"
    }
    if (FL & FL_PERSIST) {
        // the staging reads are done before the next tile's DMA lands in the ring; the stores keep draining
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    }  // tiles
    if (ONS) amax_commit(p.out_amax, omx);
#endif
}

}  // namespace mimi
