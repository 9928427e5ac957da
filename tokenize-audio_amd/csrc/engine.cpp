// Mimi encode engine (and, opt-in, the decode pass: see "decode" below): weights, workspace, stage sequencing and
// the C ABI of include/mimi_hip.h.
//
// Data layout in HBM (all fp32, channels-last so that every conv is a plain GEMM, see gemm.hip):
//   audio            [B][L]
//   SEANet stage s   x_s [B][T_s][C_s]  (C_s = 64 << s, T_0 = L, T_{s+1} = ceil(T_s / ratio_s))
//   transformer      [B][T][512]  (T = T_4 frames at 25 Hz), fused qkv [B][T][1536], mlp [B][T][2048]
//   quantizer input  [B*T'][512]  (T' = ceil(T/2) frames at 12.5 Hz), projections [B*T'][512]
//   codes            int32 [B][K][T']
// Weights are re-laid out once at finalize: conv W[co][ci][k] -> W'[co][k*Cin + ci]; q/k/v fused into
// one [1536][512]; the two input_proj stacked into one [512][512]; codebooks materialised as
// embed = embed_sum / clamp(cluster_usage, eps) (TF/modeling_mimi.py:979-983) in row layout (for the
// residual update) and in MFMA-fragment layout (for the distance GEMM), with |e|^2 in torch's order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mimi_hip.h"
#include "host_io.h"
#include "kernels.h"

using namespace mimi;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int set_err(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            return set_err(_e == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP,        \
                           "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                            \
    } while (0)

extern "C" const char* mimi_last_error(void) { return g_last_error.c_str(); }

namespace mimi {
// for the host-side C ABI files (flac.cpp): one thread-local last error behind mimi_last_error
int set_last_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
}  // namespace mimi

int mimi::set_error_message(int code, const char* msg) {
    g_last_error = msg;
    return code;
}

// ------------------------------------------------------------------------------------------------
// config / length math
// ------------------------------------------------------------------------------------------------
// mimi_config_default and mimi_config_from_json: config_json.cpp (host-only)

// MimiConv1d output length, reproducing the reference's float32 tensor arithmetic
// (TF/modeling_mimi.py:269-279): n_frames = ceil(float32(L - s) / float32(s) + 1) - 1; out = n_frames + 1.
static int64_t conv_out_len(int64_t length, int kernel, int stride) {
    const int64_t pt = kernel - stride;
    volatile float num = (float)(length - kernel + pt);
    volatile float q = num / (float)stride;
    volatile float nf = q + 1.0f;
    const int64_t n_frames = (int64_t)std::ceil((float)nf) - 1;
    return n_frames + 1;
}

struct StagePlan {
    int64_t T[5];  // T[0] = conv0 out; T[s+1] = down conv s out
    int64_t frames25, frames12;
};

static StagePlan plan_lengths(const mimi_config& c, int64_t L) {
    StagePlan p{};
    int64_t t = conv_out_len(L, c.kernel_size, 1);
    p.T[0] = t;
    for (int s = 0; s < c.num_ratios; ++s) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - s];
        t = conv_out_len(t, c.residual_kernel_size, 1);
        t = conv_out_len(t, 1, 1);
        t = conv_out_len(t, 2 * ratio, ratio);
        p.T[s + 1] = t;
    }
    t = conv_out_len(t, c.last_kernel_size, 1);
    p.frames25 = t;
    p.frames12 = conv_out_len(t, c.downsample_kernel, c.downsample_stride);
    return p;
}

extern "C" int64_t mimi_encoded_length_cfg(const mimi_config* cfg, int64_t length) {
    mimi_config d;
    if (!cfg) {
        mimi_config_default(&d);
        cfg = &d;
    }
    if (length < 0) return -1;
    return plan_lengths(*cfg, length).frames12;
}

extern "C" int64_t mimi_encoded_length(int64_t length) { return mimi_encoded_length_cfg(nullptr, length); }

// ------------------------------------------------------------------------------------------------
// host-ingest resampler (no engine handle: pure function of its device buffers)
// ------------------------------------------------------------------------------------------------
extern "C" int mimi_resample_poly(const float* dev_in, const int64_t* dev_in_off, const int64_t* dev_in_len,
                                  int32_t nclips, float* dev_out, const int64_t* dev_out_off,
                                  const int64_t* dev_out_len, int64_t max_out, const float* dev_filter,
                                  int32_t filter_len, int32_t up, int32_t down, int64_t pre_remove, void* stream) {
    if (nclips < 0 || up < 1 || down < 1 || pre_remove < 0 || max_out < 0)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "mimi_resample_poly: bad sizes (nclips %d, up %d, down %d)",
                       nclips, up, down);
    if (filter_len < 1 || filter_len > MIMI_RESAMPLE_MAX_TAPS)
        return set_err(MIMI_ERR_UNSUPPORTED, "mimi_resample_poly: filter of %d taps (max %d)", filter_len,
                       MIMI_RESAMPLE_MAX_TAPS);
    if (nclips == 0 || max_out == 0) return MIMI_OK;
    if (!dev_in || !dev_in_off || !dev_in_len || !dev_out || !dev_out_off || !dev_out_len || !dev_filter)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "mimi_resample_poly: null buffer");
    const hipError_t e = launch_resample_poly(dev_in, reinterpret_cast<const long long*>(dev_in_off),
                                              reinterpret_cast<const long long*>(dev_in_len), nclips, dev_out,
                                              reinterpret_cast<const long long*>(dev_out_off),
                                              reinterpret_cast<const long long*>(dev_out_len), max_out, dev_filter,
                                              filter_len, up, down, pre_remove, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(MIMI_ERR_HIP, "resample_poly launch: %s", hipGetErrorString(e));
    return MIMI_OK;
}

extern "C" int mimi_split_check(const float* dev_in, int64_t npairs, float scale, uint32_t* dev_out, void* stream) {
    if (npairs < 0 || (npairs > 0 && (!dev_in || !dev_out)) || !(scale > 0.0f))
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "mimi_split_check: bad arguments");
    const hipError_t e = launch_split_check(dev_in, npairs, scale, dev_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(MIMI_ERR_HIP, "split_check launch: %s", hipGetErrorString(e));
    return MIMI_OK;
}

extern "C" int mimi_gelu_check(const float* dev_in, int64_t n, float* dev_out, void* stream) {
    if (n < 0 || (n > 0 && (!dev_in || !dev_out))) return set_err(MIMI_ERR_INVALID_ARGUMENT, "mimi_gelu_check: bad arguments");
    const hipError_t e = launch_gelu_check(dev_in, n, dev_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_err(MIMI_ERR_HIP, "gelu_check launch: %s", hipGetErrorString(e));
    return MIMI_OK;
}

// ------------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------------
struct DevConv {
    int cin = 0, cout = 0, k = 0, stride = 1;
    float* w = nullptr;      // [cout][k*cin]
    void* wsplit = nullptr;  // bf16 planes [3][cout][k*cin] of w (split-bf16 precision modes)
    void* wh = nullptr;      // fp16 planes [2][cout][k*cin] of w * wscale (PREC_F16X3)
    float wscale = 1.0f;
    float* wfrag = nullptr;  // w in 32x32x2-MFMA fragment order [cout/32][k*cin/8][64][4] (stage-0 block)
    float* b = nullptr;      // [cout] or null
};

#ifndef MIMI_LN_CHECK_SKIP
#define MIMI_LN_CHECK_SKIP 1  // (A/B) 0: every LayerNorm output keeps its range-check atomics
#endif
struct DevXfmr {
    float *ln1_w, *ln1_b, *wqkv, *wo, *ls1, *ln2_w, *ln2_b, *w1, *w2, *ls2;
    void *wqkv_s, *wo_s, *w1_s, *w2_s;  // bf16 planes
    void *wqkv_h, *wo_h, *w1_h, *w2_h;  // fp16 planes (x scale)
    float wqkv_hs, wo_hs, w1_hs, w2_hs;
    // The size a LayerNorm output is held to: max_c |gamma_c| sqrt(D) (1 + 2^-10) + |beta_c|.  In exact arithmetic a
    // normalised value is at most sqrt(D - 1); the device subtracts a rounded mean, so its deviations need not sum to
    // zero and only sqrt(D) holds (one deviation carries all of D var).  The margin 2^-10 covers the roundings of the
    // two D-term reductions, rsqrt and ln_affine's two operations: (2 D + 8) 2^-24 < 2^-13 for D <= 16384.  Not covered
    // by the margin, and not a proof: ln_affine forms x rstd + (-mean rstd), whose cancellation error is
    // 2^-24 (|x| + |mean|) rstd |gamma|.  That term is left to the factor 2 between the skip's limit (2^14) and the
    // fp16 plane limit (2^15): it stays below another sqrt(D) |gamma| while (|x| + |mean|) rstd < 2^24 sqrt(D), i.e.
    // |mean| / std below ~1.9e8 at D = 512 (tests/test_encode_adversarial.py runs the device at 1e3 and on one-hot
    // rows).  Where bound x scale stays under 2^14 the output's max |x| atomics are skipped.
    float ln1_bound = INFINITY, ln2_bound = INFINITY;
};

struct ProfEvent {
    std::string name;  // "stage|kernel symbol"

    hipEvent_t ev;
    double flops;
    double bytes;
};

struct ProfStat {
    double ms = 0, flops = 0, bytes = 0;
    int64_t launches = 0;
};

constexpr int kMaxActSlots = 256;  // plane-format tensors per encode (~41 for kyutai/mimi)

struct mimi_engine {
    mimi_config cfg;
    int device = 0;
    std::mutex mu;
    bool finalized = false;
    int levels_available = 0;
    int precision = PREC_F16X3;
    // planes path: residual blocks of stages >= kUnfuseFrom run as two plane GEMMs (k3 -> h planes, k1 + skip);
    // stages 0 and 1 run the fused fp16 blocks (resblock.hip)
    static constexpr int kUnfuseFrom = 2;

    std::unordered_map<std::string, std::vector<float>> host_w;
    std::unordered_map<std::string, std::vector<int64_t>> expected;  // name -> shape
    std::vector<void*> allocations;

    DevConv conv0;
    std::vector<DevConv> res3, res1, down;
    // PREC_F16X3 fused stage-0 block: conv0 / W3 / W1 fp16-plane A fragments (resblock.hip r0h) and their scales
    void* res0_h16 = nullptr;
    float res0_wsc[3] = {1.0f, 1.0f, 1.0f};
    // ... and the stage-1 (C = 128) block: W3 / W1 16x16x32 fragments and scales
    void* res1_h16 = nullptr;
    float res1_wsc[2] = {1.0f, 1.0f};
    DevConv final_conv;
    std::vector<DevXfmr> xf;
    DevConv ds;
    float* inproj = nullptr;  // [2*vq][hidden]
    void* inproj_h = nullptr;   // its fp16 planes (PREC_F16X3)
    float inproj_hs = 1.0f;
    float* ds_fix = nullptr;    // [2][hidden in][hidden out]: W_0 + W_1 and W_3 of the downsample (replicate edges)
    float* cb_rows = nullptr;
    float* cb_frag = nullptr;
    float* cb_norm = nullptr;
    void* cb_h16 = nullptr;       // fp16 planes for the approximate distances (ops.hip rvq_level_h16_kernel)
    float* cb_unscale = nullptr;  // [level]
    float* cb_emax = nullptr;     // [level]

    float* rope_cos = nullptr;
    float* rope_sin = nullptr;
    int64_t rope_T = 0;

    // (the workspace, its ws_free event and the maxima buffers are per lane: see Lane below)

    // PREC_F16X3 activation scales (see "activation scales" above calibrate_scales): plane-format tensor `name`
    // is stored as fp16 planes of x * act_scale[slot_of[name]], a power of two fixed at mimi_finalize from a
    // calibration encode -- never from the caller's audio, so codes are a pure function of each item's input.
    // Its producer max-reduces |x| into amax_dev[slot] for the overflow check.
    std::map<std::string, int> slot_of;
    std::vector<float> act_scale;
    bool calibrated = false;  // calibrate_scales has run (lazily, before the first f16x3 encode)
    unsigned* amax_host = nullptr;  // pinned (read_amax: filled and read under the lock, behind a stream sync)
    int32_t* item_codes = nullptr;  // one item's codes (per-item overflow fallback)
    // encodes enqueued by mimi_encode_async and not yet waited (see encode_async_locked)
    struct Pending {
        int64_t id = 0;  // ticket; 0 = free
        bool claimed = false;  // a mimi_encode_wait is synchronising on it (outside the engine lock)
        hipEvent_t done = nullptr;
        unsigned* amax = nullptr;  // pinned [kMaxActSlots]: this encode's per-tensor maxima (f16x3)
        int nslots = 0;
        bool h16 = false;
        const float* audio = nullptr;
        int B = 0, K = 0;
        int64_t L = 0;
        int32_t* codes = nullptr;
        hipStream_t s = nullptr;      // the stream it ran on: its lane's own, or the caller's
        int lane = 0;                 // the lane whose workspace it ran in (re-runs at the wait go through it)
        bool ragged = false;          // a ragged batch (lens: the items' lengths, for the overflow fallback)
        std::vector<int64_t> lens;
        int* rg_pinned = nullptr;     // pinned image of its RaggedTable (read by the encode's async upload)
        size_t rg_cap = 0;
        bool chain = false;           // the encode ran the persistent RVQ chain: chain_word holds its give-up flag
        unsigned* chain_word = nullptr;  // pinned, copied from the chain's flag behind the encode
    };
    static constexpr int kMaxPending = 16;
    Pending pend[kMaxPending];
    // mimi_encode_host's buffers: one set per concurrent caller, claimed under mu, grown on demand
    struct HostIo {
        bool busy = false;
        float* d_audio = nullptr;
        float* h_audio = nullptr;    // pinned staging of the caller's samples (the H2D then runs under the launches)
        size_t audio_cap = 0;        // bytes (both audio buffers)
        int32_t* d_codes = nullptr;
        int32_t* h_codes = nullptr;  // pinned
        size_t codes_cap = 0;        // bytes (both code buffers)
        hipEvent_t done = nullptr;   // the codes' D2H
    };
    HostIo hostio[kMaxPending];
    int64_t next_ticket = 1;
    size_t item_codes_cap = 0;
    int f16_reruns = 0;             // encodes that took the overflow fallback (diagnostic)
    std::vector<float> last_amax;   // per-slot max|x| of the last waited f16x3 encode (diagnostic)
    int profiling = 0;  // 1: every stage between events; 2: the first stage of each pass only (two events)
    std::vector<ProfEvent> pending;  // recorded since last read; first event of each encode named ""
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, ProfStat> prof;
    std::vector<std::string> prof_order;
    std::vector<std::string> last_seq;  // "stage|kernel" of the last profiled encode, in launch order

    // hipGraph replay of the f16x3 encode (see graph_encode): one captured graph per (batch, length, K), the
    // audio / codes pointers passed through io_dev
    struct Graph {
        int B = 0, K = 0;
        int64_t L = 0;
        int ws_gen = 0, rope_gen = 0;
        hipGraph_t g = nullptr;
        hipGraphExec_t x = nullptr;
        uint64_t used = 0;
        unsigned* chain_flag = nullptr;  // the captured RVQ chain's give-up flag (null: no chain in the graph)
        size_t chain_clear = 0;          // bytes from chain_flag zeroed before each replay (set_io_kernel)
    };
    static constexpr int kMaxGraphs = 8;
    // A lane: everything one encode mutates, so that two encodes in two lanes run side by side (the second one's
    // kernels fill the CUs the first one's ring fills, epilogues and kernel boundaries leave idle).  Weights, scales,
    // rope tables, tickets and counters are shared.  Lane 0 exists from mimi_create and serves every encode that runs
    // on the caller's stream; a lane's stream and lane 1's buffers are made on first use (lane_prepare).
    struct Lane {
        void* ws = nullptr;
        size_t ws_bytes = 0;
        int ws_gen = 0;
        hipEvent_t ws_free = nullptr;  // recorded at the end of every encode in this lane: the next one (any stream) waits on it
        unsigned* amax_dev = nullptr;  // [kMaxActSlots][AMAX_SLOT_WORDS] sub-slots, then [kMaxActSlots] reduced
        unsigned* amax_red = nullptr;
        void** io_dev = nullptr;  // [audio, codes, pinned maxima, pinned give-up word] of the replay
        std::vector<Graph> graphs;
        std::map<std::tuple<int, int64_t, int>, int> graph_seen;  // eager encodes per shape (capture on the 2nd)
        hipStream_t stream = nullptr;   // non-blocking: the encodes that take the lane run here, not on the caller's
        hipEvent_t in_ready = nullptr;  // recorded on the caller's stream at submit: the inputs are ready
        int tickets = 0;                // encodes submitted to this lane and not yet waited
        int64_t encodes = 0;            // encodes submitted to this lane (mimi_lane_encodes)
        bool excl = false;              // its last encode may hold the persistent RVQ chain (wants the GPU to itself)
    };
    static constexpr int kLanes = 2;
    Lane lanes[kLanes];
    // which encodes take a lane (mimi_set_option "lanes"): 0 none (every encode on the caller's stream in lane 0), 1 f16x3
    // uniform batches on the per-level RVQ kernels, 2 ragged and chain-eligible encodes too
    int lanes_opt = 1;
    bool graphs_enabled = true;
    hipStream_t cap_stream = nullptr;
    int rope_gen = 0;
    uint64_t graph_clock = 0;
    int64_t graph_replays = 0, graph_captures = 0;

    bool taps = false;
    int stage0_fused = 1;  // 0: stage-0 block + down conv 0 as two kernels; 1: one fused kernel
    // LayerNorm prologue on small grids (gemm_planes.h FL_LNA): 0 off, 1 fc1 (default), 2 fc1 and q/k/v.  Batch 1
    // (rocprofv3, profiles/r3j_*): fc1 15.0 us with it vs 10.1 + 5.2 us (+ a launch gap) for fc1 + LayerNorm; q/k/v
    // 20.8 vs 10.4 + 5.2 us -- its one compute wave and 16-row tiles leave the prologue's chain exposed
    int ln_fused = 1;
    int rvq_form = 0;  // RVQ level-kernel form (mimi_set_option "rvq_form"; RvqArgs::form)
    int ln_rpw = 1;  // LayerNorm rows per wave (mimi_set_option "ln_rpw": 1 (A/B r4h: 0.186 vs 0.200 ms per B = 32 step for 2), 2, 4, 8; the same bits)
    int rvq_xcd = 1;  // large grids: a frame tile's RVQ slices on one XCD (mimi_set_option "rvq_xcd"; same bits)
    int rvq_chain = 1;  // small grids: the persistent all-levels RVQ (mimi_set_option "rvq_chain"; RvqArgs::chain)
    // The chain is taken only where its give-up flag is read back (PassCtx::chain_ok: the main encode path, whose ticket
    // carries the flag to mimi_encode_wait, and mimi_rvq_encode, which checks it itself); every fallback and internal
    // pass runs the per-level kernels
    int rvq_chain_fault = 0;    // tests only (mimi_set_option "rvq_chain_fault"; RvqArgs::chain_fault)
    int64_t chain_reruns = 0;   // encodes re-run without the chain after a sweep gave up (diagnostic)
    // q/k/v + attention as one kernel (qkv_attn.hip) for items of <= 256 frames: 0 off, 1 when the batch has at least
    // 256 (item, head) pairs (one workgroup per CU), 2 whenever the items fit (mimi_set_option "qkv_attn"; same bits)
    int qkv_attn = 1;
    int qkv_attn_xcd = 1;  // its workgroups: an item's heads on one XCD (mimi_set_option "qkv_attn_xcd"; same bits)
    int attn_band_split = 1;  // items over 256 frames: the banded attention's decomposition (0 / 1 auto / 2; same bits)
    // transformer GEMMs with sc1 output stores (gemm_planes.h FL_SC1OUT; mimi_set_option "sc1_out"): bit 0 q/k/v,
    // bit 1 fc1, bit 2 o_proj and fc2 (large batches; the same bits either way)
    int sc1_out = 2;  // (A/B, round 4: fc1 0.594 -> 0.576 ms per B = 32 step; q/k/v, o_proj and fc2 slower with it)
    // fc1's tile order in XCD column groups (GemmArgs::ncg, gemm_planes.h; mimi_set_option "fc1_cg": 0 / 1 none, 2, 4;
    // same bits): each XCD re-serves 1 / fc1_cg of W1 from its L2.  (A/B r4y: 2 groups cut fc1's fetch 85 -> 54 MB per
    // launch but not its time, 0.59-0.60 vs 0.61-0.62 ms per step; profiles/r4y_ab_fc1_cg.txt)
    int fc1_cg = 1;
    // 256 x 256 staggered planes-GEMM tile (gemm_planes256.h; mimi_set_option "gemm256", launch_gemm's g256; same bits):
    // bit 0 fc1, bit 1 the k = 2s down convs, bit 2 (tests) both on any grid
    int gemm256 = 3;  // (A/B per role at B = 32 x 10 s: profiles/g256_ab_roles.txt)
    // stage-1 fp16 block form (resblock.hip resblock128_h16_kernel; mimi_set_option "res1_form"; same bits): 0 one
    // 8-wave workgroup per CU, 1 two 4-wave workgroups per CU (each wave both 16-step tiles of its M tile; their block
    // chains interleave on the SIMDs: 0.59 -> 0.555 ms per B = 32 step, profiles/r4aa_ab_res1_form.txt)
    int res1_form = 1;
    // the k1 conv + skip + ELU as the streaming kernel (res1_stream.hip) instead of the planes GEMM (mimi_set_option
    // "res1_stream": 1 stage 2 (default), 2 stages 2 and 3, 0 off; same bits): res1_s2 0.229-0.231 -> 0.218-0.221 ms
    // per B = 32 step (round 5); stage 3 measured slower on it, 0.116-0.117 vs 0.109-0.113 (round 6, r6d / r6e)
    int res1_stream = 1;
    struct Tap {
        float* d = nullptr;
        size_t cap = 0;
        int64_t dims[3] = {0, 0, 0};
    };
    std::map<std::string, Tap> tapmap;

    // ---- decode path (mimi_enable_decode; see "decode" below).  fp32-MFMA arithmetic whatever `precision` says ----
    bool decode_enabled = false;  // the decode-path tensors are expected, read and uploaded
    DevConv dec_first, dec_last;  // decoder.layers.0 (hidden -> 16 x filters, k 7) and the last conv (filters -> 1, k 3)
    std::vector<DevConv> dec_up;  // transposed convs as causal k = 2 convs with r * Cout phase-major output channels
    std::vector<DevConv> dec_res3, dec_res1;
    std::vector<DevXfmr> dxf;     // decoder_transformer (fp32 weights only)
    float* outproj = nullptr;     // [hidden][2 * vq]: (semantic | acoustic) output_proj side by side along K
    float* upsample_w = nullptr;  // [hidden][4]
    void* dws = nullptr;          // decode's own workspace (encode's buffers and captured graphs stay untouched)
    size_t dws_bytes = 0;
    unsigned* dec_flag = nullptr;       // device word: a code outside [0, codebook_size) was seen
    unsigned* dec_flag_host = nullptr;  // pinned
    int* dec_rg_host = nullptr;         // pinned: the host image of a ragged decode's length tables (DecLayout)
    size_t dec_rg_cap = 0;              // ints
};

static int dev_alloc(mimi_engine* e, void** p, size_t bytes) {
    hipError_t err = hipMalloc(p, bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return set_err(err == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP, "hipMalloc(%zu): %s",
                       bytes, hipGetErrorString(err));
    }
    e->allocations.push_back(*p);
    return MIMI_OK;
}

static int upload(mimi_engine* e, float** dst, const std::vector<float>& host) {
    int rc = dev_alloc(e, reinterpret_cast<void**>(dst), host.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*dst, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return MIMI_OK;
}

// x = x0 + x1 + x2 with x_p = bf16_rne(x - x0 - ... - x_{p-1}) (each subtraction exact in fp32)
static uint16_t f2bf_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFF + ((u >> 16) & 1);
    return (uint16_t)(u >> 16);
}
static float bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static int upload_split(mimi_engine* e, void** dst, const std::vector<float>& host) {
    const size_t n = host.size();
    std::vector<uint16_t> planes(3 * n);
    for (size_t i = 0; i < n; ++i) {
        float r = host[i];
        for (int p = 0; p < 3; ++p) {
            const uint16_t h = f2bf_rne(r);
            planes[p * n + i] = h;
            r = r - bf2f(h);
        }
    }
    int rc = dev_alloc(e, dst, planes.size() * sizeof(uint16_t));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*dst, planes.data(), planes.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return MIMI_OK;
}

// fp16 planes of w * scale: h0 = fp16(w s), h1 = fp16(w s - h0) (22-bit significand), scale a power of two
// putting max|w| s in [2^13, 2^14): every weight >= 2^-17 max|w| keeps its full 22 bits, and no product of a
// plane with an activation plane (|x s_x| < 2^15) can overflow the fp32 accumulator
static int upload_f16(mimi_engine* e, void** dst, const std::vector<float>& host, float* scale) {
    const size_t n = host.size();
    float wmax = 0.0f;
    for (float v : host) wmax = std::max(wmax, std::fabs(v));
    const float sc = wmax > 0.0f && std::isfinite(wmax) ? std::ldexp(1.0f, 13 - std::ilogb(wmax)) : 1.0f;
    std::vector<_Float16> planes(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const float t = host[i] * sc;
        const _Float16 h0 = (_Float16)t;
        planes[i] = h0;
        planes[n + i] = (_Float16)(t - (float)h0);
    }
    int rc = dev_alloc(e, dst, planes.size() * sizeof(_Float16));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(*dst, planes.data(), planes.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    *scale = sc;
    return MIMI_OK;
}

// power of two putting max|w| s in [2^13, 2^14) (see upload_f16)
static float f16_weight_scale(const std::vector<float>& w) {
    float wmax = 0.0f;
    for (float v : w) wmax = std::max(wmax, std::fabs(v));
    return wmax > 0.0f && std::isfinite(wmax) ? std::ldexp(1.0f, 13 - std::ilogb(wmax)) : 1.0f;
}

// Appends W [M][K] (row-major) * sc as fp16 planes in 32x32x16-MFMA A-fragment order, [mt][ks][plane] 1-KB
// fragments of [64 lanes][8 halves]: lane (i, h) holds W[32 mt + i][16 ks + 8 h + e].
static void append_afrags_h16(std::vector<_Float16>& out, const std::vector<float>& w, int M, int K, float sc) {
    for (int mt = 0; mt < M / 32; ++mt)
        for (int ks = 0; ks < K / 16; ++ks)
            for (int pl = 0; pl < 2; ++pl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const float t = w[(size_t)(32 * mt + (lane & 31)) * K + 16 * ks + 8 * (lane >> 5) + e] * sc;
                        const _Float16 h0 = (_Float16)t;
                        out.push_back(pl == 0 ? h0 : (_Float16)(t - (float)h0));
                    }
}

// W [N][K] -> Wf[nt][kq][lane][s] = W[32*nt + (lane & 31)][8*kq + 4*(lane >> 5) + s]: a wave's B fragment
// for one 8-wide K quad of one 32-column tile is one contiguous 1 KB load.
static std::vector<float> frag_layout(const std::vector<float>& w, int N, int K) {
    std::vector<float> f((size_t)N * K);
    for (int nt = 0; nt < N / 32; ++nt)
        for (int kq = 0; kq < K / 8; ++kq)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s)
                    f[(((size_t)nt * (K / 8) + kq) * 64 + lane) * 4 + s] =
                        w[(size_t)(32 * nt + (lane & 31)) * K + 8 * kq + 4 * (lane >> 5) + s];
    return f;
}

static std::string conv_name_first() { return "encoder.layers.0.conv"; }

static void build_expected(mimi_engine* e) {
    const mimi_config& c = e->cfg;
    auto& ex = e->expected;
    ex.clear();
    ex[conv_name_first() + ".weight"] = {c.num_filters, c.audio_channels, c.kernel_size};
    ex[conv_name_first() + ".bias"] = {c.num_filters};
    int idx = 1;
    int C = c.num_filters;
    for (int s = 0; s < c.num_ratios; ++s) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - s];
        const std::string p = "encoder.layers." + std::to_string(idx) + ".block.";
        ex[p + "1.conv.weight"] = {C / c.compress, C, c.residual_kernel_size};
        ex[p + "1.conv.bias"] = {C / c.compress};
        ex[p + "3.conv.weight"] = {C, C / c.compress, 1};
        ex[p + "3.conv.bias"] = {C};
        idx += 2;
        const std::string d = "encoder.layers." + std::to_string(idx) + ".conv.";
        ex[d + "weight"] = {2 * C, C, 2 * ratio};
        ex[d + "bias"] = {2 * C};
        idx += 1;
        C *= 2;
    }
    idx += 1;
    const std::string f = "encoder.layers." + std::to_string(idx) + ".conv.";
    ex[f + "weight"] = {c.hidden_size, C, c.last_kernel_size};
    ex[f + "bias"] = {c.hidden_size};
    const int h = c.hidden_size;
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string p = "encoder_transformer.layers." + std::to_string(l) + ".";
        for (const char* n : {"q_proj", "k_proj", "v_proj"})
            ex[p + "self_attn." + n + ".weight"] = {c.num_attention_heads * c.head_dim, h};
        ex[p + "self_attn.o_proj.weight"] = {h, c.num_attention_heads * c.head_dim};
        ex[p + "mlp.fc1.weight"] = {c.intermediate_size, h};
        ex[p + "mlp.fc2.weight"] = {h, c.intermediate_size};
        for (const char* n : {"input_layernorm", "post_attention_layernorm"}) {
            ex[p + n + ".weight"] = {h};
            ex[p + n + ".bias"] = {h};
        }
        ex[p + "self_attn_layer_scale.scale"] = {h};
        ex[p + "mlp_layer_scale.scale"] = {h};
    }
    ex["downsample.conv.weight"] = {h, h, c.downsample_kernel};
    for (const char* q : {"semantic", "acoustic"})
        ex[std::string("quantizer.") + q + "_residual_vector_quantizer.input_proj.weight"] = {c.vq_hidden_dim, h, 1};
}

static std::string codebook_prefix(const mimi_config& c, int level) {
    if (level < c.num_semantic_quantizers)
        return "quantizer.semantic_residual_vector_quantizer.layers." + std::to_string(level) + ".codebook.";
    return "quantizer.acoustic_residual_vector_quantizer.layers." + std::to_string(level - c.num_semantic_quantizers) +
           ".codebook.";
}

static int check_supported(const mimi_config& c) {
    if (c.audio_channels != 1) return set_err(MIMI_ERR_UNSUPPORTED, "audio_channels must be 1");
    if (c.num_filters != 64 || c.kernel_size != 7)
        return set_err(MIMI_ERR_UNSUPPORTED, "first conv must be 1->64, k=7");
    if (c.hidden_size != 512 || c.head_dim != 64 || c.num_attention_heads * c.head_dim != c.hidden_size)
        return set_err(MIMI_ERR_UNSUPPORTED, "transformer must be 512 wide with 64-dim heads");
    if (c.codebook_dim != 256 || c.vq_hidden_dim != 256 || c.codebook_size % 256 != 0)
        return set_err(MIMI_ERR_UNSUPPORTED, "codebooks must be [n*256][256]");
    if (c.num_ratios < 1 || c.num_ratios > 8) return set_err(MIMI_ERR_UNSUPPORTED, "num_ratios out of range");
    if (c.residual_kernel_size * c.num_filters / c.compress % 32 != 0 && c.compress != 2)
        return set_err(MIMI_ERR_UNSUPPORTED, "compress must be 2");
    if (c.num_semantic_quantizers < 1 || c.num_semantic_quantizers >= c.num_quantizers)
        return set_err(MIMI_ERR_UNSUPPORTED, "num_semantic_quantizers out of range");
    return MIMI_OK;
}

extern "C" int mimi_create(const mimi_config* cfg, int device, mimi_engine** out) {
    if (!out) return set_err(MIMI_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    std::unique_ptr<mimi_engine> e(new mimi_engine());
    if (cfg)
        e->cfg = *cfg;
    else
        mimi_config_default(&e->cfg);
    int rc = check_supported(e->cfg);
    if (rc) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_err(MIMI_ERR_INVALID_ARGUMENT, "device %d of %d", device, ndev);
    e->device = device;
    HIP_TRY(hipSetDevice(device));
    mimi_engine::Lane& l0 = e->lanes[0];  // (lane 1's event and buffers: lane_prepare, on its first use)
    HIP_TRY(hipEventCreateWithFlags(&l0.ws_free, hipEventDisableTiming));
    HIP_TRY(hipMalloc(&l0.amax_dev, ((size_t)kMaxActSlots * AMAX_SLOT_WORDS + kMaxActSlots) * sizeof(unsigned)));
    l0.amax_red = l0.amax_dev + (size_t)kMaxActSlots * AMAX_SLOT_WORDS;
    HIP_TRY(hipMemset(l0.amax_dev, 0, ((size_t)kMaxActSlots * AMAX_SLOT_WORDS + kMaxActSlots) * sizeof(unsigned)));
    HIP_TRY(hipHostMalloc(&e->amax_host, kMaxActSlots * sizeof(unsigned), hipHostMallocDefault));
    build_expected(e.get());
    *out = e.release();
    return MIMI_OK;
}

// The one-call constructor: a checkpoint directory in the HF layout (config.json + *.safetensors,
// what MimiModel.from_pretrained("kyutai/mimi") reads: emilia-mimi/process_shard.py:57-60) or a lone .safetensors
// file (default config) -> a finalized engine.  config_json.cpp parses the config and picks the file; on any failure
// the half-built engine is released and the first error is the one mimi_last_error reports.
extern "C" int mimi_create_from_dir(const char* weights_dir, int device, mimi_engine** out) {
    return mimi_create_from_dir_flags(weights_dir, device, 0, out);
}

extern "C" int mimi_create_from_dir_flags(const char* weights_dir, int device, uint32_t flags, mimi_engine** out) {
    if (!out) return set_err(MIMI_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!weights_dir) return set_err(MIMI_ERR_INVALID_ARGUMENT, "weights_dir is NULL");
    std::string cfg_path, st_path;
    int rc = mimi::find_checkpoint(weights_dir, cfg_path, st_path);
    if (rc) return rc;
    mimi_config cfg;
    mimi_config_default(&cfg);
    if (!cfg_path.empty() && (rc = mimi_config_from_json(cfg_path.c_str(), &cfg))) return rc;
    mimi_engine* e = nullptr;
    if (flags & ~(uint32_t)MIMI_CREATE_DECODE) return set_err(MIMI_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if ((rc = mimi_create(&cfg, device, &e))) return rc;
    if (((flags & MIMI_CREATE_DECODE) && (rc = mimi_enable_decode(e))) ||
        (rc = mimi_load_safetensors(e, st_path.c_str())) || (rc = mimi_finalize(e))) {
        const std::string msg = g_last_error;
        mimi_destroy(e);
        g_last_error = msg;
        return rc;
    }
    *out = e;
    return MIMI_OK;
}

extern "C" int mimi_set_weight(mimi_engine* e, const char* name, const float* data, int64_t numel) {
    if (!e || !name || (!data && numel > 0)) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null argument");
    if (e->finalized) return set_err(MIMI_ERR_STATE, "weights are frozen after mimi_finalize");
    std::lock_guard<std::mutex> lk(e->mu);
    e->host_w[name].assign(data, data + numel);
    return MIMI_OK;
}

// Checkpoint files: safetensors.cpp (host-only, bounds-checked; built under ASan/UBSan by tools/asan).  A tensor
// is read when the encode path needs it (the names build_expected lists, the quantizer's codebooks, weight-norm
// factors of a conv); the decoder / upsample tensors of a full checkpoint are skipped unread unless
// mimi_enable_decode has put the decode-path names into `expected`.
extern "C" int mimi_load_safetensors(mimi_engine* e, const char* path) {
    if (!e || !path) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null argument");
    if (e->finalized) return set_err(MIMI_ERR_STATE, "weights are frozen after mimi_finalize");
    std::lock_guard<std::mutex> lk(e->mu);
    auto wanted = [&](const std::string& name) {
        // (the decode half of a checkpoint is read only after mimi_enable_decode: its names are then in `expected`)
        if (!e->decode_enabled && (name.rfind("decoder", 0) == 0 || name.rfind("upsample", 0) == 0)) return false;
        const bool quant = name.rfind("quantizer.", 0) == 0 &&  // input_proj + codebooks (not output_proj)
                           (name.find(".codebook.") != std::string::npos || name.find("input_proj") != std::string::npos);
        return e->expected.count(name) > 0 || quant ||
               name.find("weight_g") != std::string::npos || name.find("weight_v") != std::string::npos ||
               name.find("original0") != std::string::npos || name.find("original1") != std::string::npos;
    };
    std::map<std::string, std::vector<float>> got;
    std::string err;
    const int rc = st_load(path, wanted, got, err);
    if (rc) return set_err(rc, "%s", err.c_str());
    for (auto& kv : got) e->host_w[kv.first] = std::move(kv.second);
    return MIMI_OK;
}

// weight-norm checkpoints store weight_g [cout,1,1] and weight_v [cout,cin,k]: w = g * v / ||v|| per cout
static bool resolve_weight_norm(mimi_engine* e, const std::string& wname, const std::vector<int64_t>& shape) {
    const std::string base = wname.substr(0, wname.size() - std::string("weight").size());
    const std::string gk[] = {base + "weight_g", base + "parametrizations.weight.original0"};
    const std::string vk[] = {base + "weight_v", base + "parametrizations.weight.original1"};
    for (int i = 0; i < 2; ++i) {
        auto g = e->host_w.find(gk[i]);
        auto v = e->host_w.find(vk[i]);
        if (g == e->host_w.end() || v == e->host_w.end()) continue;
        const int64_t cout = shape[0];
        const int64_t per = (int64_t)v->second.size() / cout;
        std::vector<float> w(v->second.size());
        for (int64_t o = 0; o < cout; ++o) {
            double n2 = 0;
            for (int64_t j = 0; j < per; ++j) n2 += (double)v->second[o * per + j] * v->second[o * per + j];
            const float s = (float)(g->second[o] / std::sqrt(n2));
            for (int64_t j = 0; j < per; ++j) w[o * per + j] = v->second[o * per + j] * s;
        }
        e->host_w[wname] = std::move(w);
        return true;
    }
    return false;
}

static int get_w(mimi_engine* e, const std::string& name, std::vector<float>** out) {
    auto it = e->host_w.find(name);
    auto ex = e->expected.find(name);
    if (it == e->host_w.end() && ex != e->expected.end() && resolve_weight_norm(e, name, ex->second))
        it = e->host_w.find(name);
    if (it == e->host_w.end()) return set_err(MIMI_ERR_WEIGHTS, "missing parameter %s", name.c_str());
    if (ex != e->expected.end()) {
        int64_t n = 1;
        for (int64_t d : ex->second) n *= d;
        if ((int64_t)it->second.size() != n)
            return set_err(MIMI_ERR_WEIGHTS, "parameter %s has %zu elements, expected %lld", name.c_str(),
                           it->second.size(), (long long)n);
    }
    *out = &it->second;
    return MIMI_OK;
}

// W[co][ci][k] -> W'[co][k*cin + ci]
static std::vector<float> relayout_conv(const std::vector<float>& w, int cout, int cin, int k) {
    std::vector<float> o((size_t)cout * cin * k);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int kk = 0; kk < k; ++kk) o[((size_t)co * k + kk) * cin + ci] = w[((size_t)co * cin + ci) * k + kk];
    return o;
}

// As append_afrags_h16 for the 16x16x32 MFMA: fragments [mt][ks][plane], lane (i, q) holding
// W[16 mt + i][32 ks + 8 q + e] (i = lane & 15, q = lane >> 4).
static void append_afrags16_h16(std::vector<_Float16>& out, const std::vector<float>& w, int M, int K, float sc) {
    for (int mt = 0; mt < M / 16; ++mt)
        for (int ks = 0; ks < K / 32; ++ks)
            for (int pl = 0; pl < 2; ++pl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const float t = w[(size_t)(16 * mt + (lane & 15)) * K + 32 * ks + 8 * (lane >> 4) + e] * sc;
                        const _Float16 h0 = (_Float16)t;
                        out.push_back(pl == 0 ? h0 : (_Float16)(t - (float)h0));
                    }
}

// The stage-1 (C = 128) fp16 block's weight image (resblock.hip resblock128_h16_kernel): W3 [64][384] then
// W1 [128][64] as 16x16x32 A fragments.
static int make_res1_h16(mimi_engine* e) {
    const mimi_config& c = e->cfg;
    if (c.num_filters != 64 || c.residual_kernel_size != 3 || c.compress != 2 || c.num_ratios < 2) return MIMI_OK;
    std::vector<float>*w3, *w1;
    int rc;
    if ((rc = get_w(e, "encoder.layers.4.block.1.conv.weight", &w3)) ||
        (rc = get_w(e, "encoder.layers.4.block.3.conv.weight", &w1)))
        return rc;
    const std::vector<float> w3l = relayout_conv(*w3, 64, 128, 3);  // [64][3*128], tap-major
    const std::vector<float>& w1l = *w1;                             // [128][64][1]
    const float s3 = f16_weight_scale(w3l), s1 = f16_weight_scale(w1l);
    std::vector<_Float16> img;
    img.reserve((size_t)RES1_H16_FRAGS * 512);
    append_afrags16_h16(img, w3l, 64, 384, s3);
    append_afrags16_h16(img, w1l, 128, 64, s1);
    if (img.size() != (size_t)RES1_H16_FRAGS * 512) return set_err(MIMI_ERR_WEIGHTS, "res1 fp16 image size");
    if ((rc = dev_alloc(e, &e->res1_h16, img.size() * sizeof(_Float16)))) return rc;
    HIP_TRY(hipMemcpy(e->res1_h16, img.data(), img.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    e->res1_wsc[0] = s3;
    e->res1_wsc[1] = s1;
    return MIMI_OK;
}

// The stage-0 fp16 block's weight image (resblock.hip resblock0_h16_kernel): 4 conv0 fragments
// [mt][variant] -- variant 0: every lane (i, h) holds w_hi[32 mt + i][0..6], 0; variant 1: lanes h = 0 hold
// w_lo, lanes h = 1 zeros (against the audio taps' hi | lo planes: w_hi a_hi + w_hi a_lo, then w_lo a_hi) --
// then W3 [32][192] and W1 [64][32] as append_afrags_h16.
static int make_res0_h16(mimi_engine* e) {
    const mimi_config& c = e->cfg;
    if (c.num_filters != 64 || c.kernel_size != 7 || c.residual_kernel_size != 3 || c.compress != 2) return MIMI_OK;
    std::vector<float>*w0, *w3, *w1;
    int rc;
    if ((rc = get_w(e, "encoder.layers.0.conv.weight", &w0)) || (rc = get_w(e, "encoder.layers.1.block.1.conv.weight", &w3)) ||
        (rc = get_w(e, "encoder.layers.1.block.3.conv.weight", &w1)))
        return rc;
    const std::vector<float> w3l = relayout_conv(*w3, 32, 64, 3);  // [32][3*64], tap-major
    const std::vector<float>& w1l = *w1;                            // [64][32][1]
    const float s0 = f16_weight_scale(*w0), s3 = f16_weight_scale(w3l), s1 = f16_weight_scale(w1l);
    std::vector<_Float16> img;
    img.reserve((size_t)RES0_H16_FRAGS * 512);
    for (int mt = 0; mt < 2; ++mt)
        for (int var = 0; var < 2; ++var)
            for (int lane = 0; lane < 64; ++lane)
                for (int k = 0; k < 8; ++k) {
                    _Float16 v = (_Float16)0.0f;
                    if (k < 7) {
                        const float t = (*w0)[(size_t)(32 * mt + (lane & 31)) * 7 + k] * s0;
                        const _Float16 h0 = (_Float16)t;
                        if (var == 0) v = h0;
                        else if ((lane >> 5) == 0) v = (_Float16)(t - (float)h0);
                    }
                    img.push_back(v);
                }
    append_afrags_h16(img, w3l, 32, 192, s3);
    append_afrags_h16(img, w1l, 64, 32, s1);
    if (img.size() != (size_t)RES0_H16_FRAGS * 512) return set_err(MIMI_ERR_WEIGHTS, "res0 fp16 image size");
    if ((rc = dev_alloc(e, &e->res0_h16, img.size() * sizeof(_Float16)))) return rc;
    HIP_TRY(hipMemcpy(e->res0_h16, img.data(), img.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    e->res0_wsc[0] = s0;
    e->res0_wsc[1] = s3;
    e->res0_wsc[2] = s1;
    return MIMI_OK;
}

static int make_conv(mimi_engine* e, DevConv& dc, const std::string& prefix, int cin, int cout, int k, int stride,
                     bool bias) {
    std::vector<float>* w;
    int rc = get_w(e, prefix + "weight", &w);
    if (rc) return rc;
    if ((int64_t)w->size() != (int64_t)cin * cout * k)
        return set_err(MIMI_ERR_WEIGHTS, "%sweight: bad size", prefix.c_str());
    dc.cin = cin;
    dc.cout = cout;
    dc.k = k;
    dc.stride = stride;
    const std::vector<float> wl = cin == 1 ? *w : relayout_conv(*w, cout, cin, k);
    rc = upload(e, &dc.w, wl);
    if (rc) return rc;
    if (cin % 4 == 0 && (k * cin) % 32 == 0 &&
        ((rc = upload_split(e, &dc.wsplit, wl)) || (rc = upload_f16(e, &dc.wh, wl, &dc.wscale))))
        return rc;
    if (cout % 32 == 0 && (k * cin) % 8 == 0 && (rc = upload(e, &dc.wfrag, frag_layout(wl, cout, k * cin)))) return rc;
    if (bias) {
        std::vector<float>* b;
        rc = get_w(e, prefix + "bias", &b);
        if (rc) return rc;
        rc = upload(e, &dc.b, *b);
        if (rc) return rc;
    }
    return MIMI_OK;
}

// sum of squares in torch's x.pow(2).sum(-1) order for rows of 8*m floats (see ops.hip)
static float torch_sqsum_host(const float* r, int D) {
    float lanes[8];
    for (int l = 0; l < 8; ++l) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int blk = 0; blk < D / 8; ++blk) {
            volatile float sq = r[blk * 8 + l] * r[blk * 8 + l];
            a[blk & 3] = a[blk & 3] + sq;
        }
        volatile float t = a[0] + a[1];
        t = t + a[2];
        t = t + a[3];
        lanes[l] = t;
    }
    volatile float tot = lanes[0];
    for (int l = 1; l < 8; ++l) tot = tot + lanes[l];
    return tot;
}

static int calibrate_scales(mimi_engine* e);
static int finalize_decode(mimi_engine* e);

extern "C" int mimi_finalize(mimi_engine* e) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->finalized) return MIMI_OK;
    HIP_TRY(hipSetDevice(e->device));
    const mimi_config& c = e->cfg;
    int rc = make_conv(e, e->conv0, "encoder.layers.0.conv.", 1, c.num_filters, c.kernel_size, 1, true);
    if (rc) return rc;
    int idx = 1, C = c.num_filters;
    e->res3.resize(c.num_ratios);
    e->res1.resize(c.num_ratios);
    e->down.resize(c.num_ratios);
    for (int s = 0; s < c.num_ratios; ++s) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - s];
        const std::string p = "encoder.layers." + std::to_string(idx) + ".block.";
        if ((rc = make_conv(e, e->res3[s], p + "1.conv.", C, C / c.compress, c.residual_kernel_size, 1, true))) return rc;
        if ((rc = make_conv(e, e->res1[s], p + "3.conv.", C / c.compress, C, 1, 1, true))) return rc;
        idx += 2;
        if ((rc = make_conv(e, e->down[s], "encoder.layers." + std::to_string(idx) + ".conv.", C, 2 * C, 2 * ratio,
                            ratio, true)))
            return rc;
        idx += 1;
        C *= 2;
    }
    if ((rc = make_res0_h16(e)) || (rc = make_res1_h16(e))) return rc;
    idx += 1;
    if ((rc = make_conv(e, e->final_conv, "encoder.layers." + std::to_string(idx) + ".conv.", C, c.hidden_size,
                        c.last_kernel_size, 1, true)))
        return rc;
    const int h = c.hidden_size;
    e->xf.resize(c.num_hidden_layers);
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string p = "encoder_transformer.layers." + std::to_string(l) + ".";
        DevXfmr& x = e->xf[l];
        std::vector<float>*q, *k, *v, *t;
        if ((rc = get_w(e, p + "self_attn.q_proj.weight", &q)) || (rc = get_w(e, p + "self_attn.k_proj.weight", &k)) ||
            (rc = get_w(e, p + "self_attn.v_proj.weight", &v)))
            return rc;
        std::vector<float> qkv;
        qkv.reserve(q->size() * 3);
        qkv.insert(qkv.end(), q->begin(), q->end());
        qkv.insert(qkv.end(), k->begin(), k->end());
        qkv.insert(qkv.end(), v->begin(), v->end());
        if ((rc = upload(e, &x.wqkv, qkv)) || (rc = upload_split(e, &x.wqkv_s, qkv)) ||
            (rc = upload_f16(e, &x.wqkv_h, qkv, &x.wqkv_hs)))
            return rc;
        struct {
            const char* n;
            float** d;
        } simple[] = {{"self_attn.o_proj.weight", &x.wo},
                      {"mlp.fc1.weight", &x.w1},
                      {"mlp.fc2.weight", &x.w2},
                      {"input_layernorm.weight", &x.ln1_w},
                      {"input_layernorm.bias", &x.ln1_b},
                      {"post_attention_layernorm.weight", &x.ln2_w},
                      {"post_attention_layernorm.bias", &x.ln2_b},
                      {"self_attn_layer_scale.scale", &x.ls1},
                      {"mlp_layer_scale.scale", &x.ls2}};
        for (auto& sp : simple) {
            if ((rc = get_w(e, p + sp.n, &t))) return rc;
            if ((rc = upload(e, sp.d, *t))) return rc;
            void** sd = sp.d == &x.wo ? &x.wo_s : sp.d == &x.w1 ? &x.w1_s : sp.d == &x.w2 ? &x.w2_s : nullptr;
            void** hd = sp.d == &x.wo ? &x.wo_h : sp.d == &x.w1 ? &x.w1_h : sp.d == &x.w2 ? &x.w2_h : nullptr;
            float* hs = sp.d == &x.wo ? &x.wo_hs : sp.d == &x.w1 ? &x.w1_hs : sp.d == &x.w2 ? &x.w2_hs : nullptr;
            if (sd && ((rc = upload_split(e, sd, *t)) || (rc = upload_f16(e, hd, *t, hs)))) return rc;
        }
        for (int k = 0; k < 2; ++k) {
            std::vector<float>*g, *bb;
            const std::string n = k ? "post_attention_layernorm." : "input_layernorm.";
            if ((rc = get_w(e, p + n + "weight", &g)) || (rc = get_w(e, p + n + "bias", &bb))) return rc;
            double bound = 0.0;
            const double r = std::sqrt((double)h) * (1.0 + 1.0 / 1024.0);  // (DevXfmr::ln1_bound: sqrt(D) and the margin)
            for (size_t i = 0; i < g->size() && i < bb->size(); ++i) {
                const double v = std::fabs((double)(*g)[i]) * r + std::fabs((double)(*bb)[i]);
                bound = std::isfinite(v) ? std::max(bound, v) : INFINITY;
            }
            (k ? x.ln2_bound : x.ln1_bound) = (float)bound;
        }
    }
    if ((rc = make_conv(e, e->ds, "downsample.conv.", h, h, c.downsample_kernel, c.downsample_stride, false))) return rc;
    if (c.downsample_kernel == 4 && c.downsample_stride == 2) {  // replicate-edge terms of the planes downsample
        std::vector<float>* w;
        if ((rc = get_w(e, "downsample.conv.weight", &w))) return rc;
        const std::vector<float> wl = relayout_conv(*w, h, h, 4);  // [co][kk*h + ci]
        std::vector<float> fix((size_t)2 * h * h);
        for (int co = 0; co < h; ++co)
            for (int ci = 0; ci < h; ++ci) {
                const size_t r = (size_t)co * 4 * h;
                fix[(size_t)ci * h + co] = wl[r + ci] + wl[r + h + ci];  // [edge][ci][co]
                fix[(size_t)h * h + (size_t)ci * h + co] = wl[r + 3 * h + ci];
            }
        if ((rc = upload(e, &e->ds_fix, fix))) return rc;
    }
    {
        std::vector<float>*ps, *pa;
        if ((rc = get_w(e, "quantizer.semantic_residual_vector_quantizer.input_proj.weight", &ps)) ||
            (rc = get_w(e, "quantizer.acoustic_residual_vector_quantizer.input_proj.weight", &pa)))
            return rc;
        std::vector<float> both(*ps);
        both.insert(both.end(), pa->begin(), pa->end());
        if ((rc = upload(e, &e->inproj, both)) || (rc = upload_f16(e, &e->inproj_h, both, &e->inproj_hs))) return rc;
    }
    // codebooks: as many consecutive levels as the checkpoint provides (32 for kyutai/mimi)
    const int n = c.codebook_size, D = c.codebook_dim;
    int L = 0;
    while (L < c.num_quantizers && e->host_w.count(codebook_prefix(c, L) + "embed_sum")) ++L;
    if (L <= c.num_semantic_quantizers) return set_err(MIMI_ERR_WEIGHTS, "no acoustic codebooks found");
    std::vector<float> rows((size_t)L * n * D), frag((size_t)L * n * D), norms((size_t)L * n);
    for (int lv = 0; lv < L; ++lv) {
        std::vector<float>*es, *us;
        const std::string p = codebook_prefix(c, lv);
        if ((rc = get_w(e, p + "embed_sum", &es)) || (rc = get_w(e, p + "cluster_usage", &us))) return rc;
        if ((int64_t)es->size() != (int64_t)n * D || (int64_t)us->size() != n)
            return set_err(MIMI_ERR_WEIGHTS, "%s: bad codebook shape", p.c_str());
        float* R = rows.data() + (size_t)lv * n * D;
        for (int j = 0; j < n; ++j) {
            const float u = std::max((*us)[j], c.codebook_eps);
            for (int d = 0; d < D; ++d) {
                volatile float q = (*es)[(size_t)j * D + d] / u;
                R[(size_t)j * D + d] = q;
            }
            norms[(size_t)lv * n + j] = torch_sqsum_host(R + (size_t)j * D, D);
        }
        // fragment layout: [jt][u][lane][s] = embed[32*jt + (lane&31)][8u + 2s + (lane>>5)]
        float* F = frag.data() + (size_t)lv * n * D;
        for (int jt = 0; jt < n / 32; ++jt)
            for (int u = 0; u < D / 8; ++u)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s)
                        F[(((size_t)jt * (D / 8) + u) * 64 + lane) * 4 + s] =
                            R[(size_t)(32 * jt + (lane & 31)) * D + 8 * u + 2 * s + (lane >> 5)];
    }
    if ((rc = upload(e, &e->cb_rows, rows)) || (rc = upload(e, &e->cb_frag, frag)) || (rc = upload(e, &e->cb_norm, norms)))
        return rc;
    {
        // fp16 planes of embed * cs (cs: power of two putting max|embed| in [2^13, 2^14)) in 32x32x16 B-fragment
        // order [level][code tile][k step][plane][lane (j, h)][8]: embed[32 ct + j][16 ks + 8 h + q]
        std::vector<_Float16> h16((size_t)L * n * D * 2);
        std::vector<float> unsc(L), emax(L);
        for (int lv = 0; lv < L; ++lv) {
            const float* R = rows.data() + (size_t)lv * n * D;
            float amax = 0.0f, nmax = 0.0f;
            for (size_t i = 0; i < (size_t)n * D; ++i) amax = std::max(amax, std::fabs(R[i]));
            for (int j = 0; j < n; ++j) nmax = std::max(nmax, norms[(size_t)lv * n + j]);
            const float cs = amax > 0.0f && std::isfinite(amax) ? std::ldexp(1.0f, 13 - std::ilogb(amax)) : 1.0f;
            unsc[lv] = 1.0f / cs;
            emax[lv] = std::sqrt(nmax) * (1.0f + 1e-6f);
            _Float16* H = h16.data() + (size_t)lv * n * D * 2;
            size_t o = 0;
            for (int ct = 0; ct < n / 32; ++ct)
                for (int ks = 0; ks < D / 16; ++ks)
                    for (int pl = 0; pl < 2; ++pl)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int q = 0; q < 8; ++q) {
                                const float t = R[(size_t)(32 * ct + (lane & 31)) * D + 16 * ks + 8 * (lane >> 5) + q] * cs;
                                const _Float16 hi = (_Float16)t;
                                H[o++] = pl == 0 ? hi : (_Float16)(t - (float)hi);
                            }
        }
        if ((rc = dev_alloc(e, &e->cb_h16, h16.size() * sizeof(_Float16)))) return rc;
        HIP_TRY(hipMemcpy(e->cb_h16, h16.data(), h16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        if ((rc = upload(e, &e->cb_unscale, unsc)) || (rc = upload(e, &e->cb_emax, emax))) return rc;
    }
    e->levels_available = L;
    if (e->decode_enabled && (rc = finalize_decode(e))) return rc;
    e->host_w.clear();
    e->finalized = true;  // (the f16x3 activation scales are calibrated before the first f16x3 encode)
    return MIMI_OK;
}

// ------------------------------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------------------------------
struct Workspace {
    float *x, *y;                  // SEANet ping-pong (the residual blocks keep their hidden tile on chip)
    float *t0, *t1, *qkv, *att, *ff;  // transformer
    float *dsout, *proj;
    float* rvq;  // rvq_work_bytes(frames)
    float *xe, *h;  // planes path, unfused residual blocks: ELU(x) planes, hidden planes
    int* rg;        // ragged batches: the per-item length table (RaggedTable)
};

// Ragged batches (mimi_encode_ragged): item b is encoded exactly as it would be alone at its own length L_b --
// every kernel reads only its item's valid rows (the rest read as zero: the item's own extra padding) and
// computes / stores / max-reduces only its valid rows.  The per-item lengths of every stage live in one small
// device table, stage-major: T[0..4][B] (conv0 / down-conv outputs), T25[B], F[B] (12.5 Hz frames), then the
// fused blocks' tile prefixes st0[B + 1], st1[B + 1] (32-step tiles over T[0] / T[1]), then the transformer
// section's PACKED row layout: toff[B] (item b's first row: the items' 25 Hz frames back to back, R rows in all).
// Behind the table, in the workspace only, rpos[R]: the position of each packed row inside its item (RoPE), written
// on the device from toff (launch_ragged_rows) -- the host table stays a few hundred bytes.
struct RaggedTable {
    enum { NST = 7 };
    int B = 0;
    int64_t R = 0;                // packed transformer rows: sum of the items' 25 Hz frames
    std::vector<StagePlan> plan;  // per item
    std::vector<int64_t> len;     // samples per item
    int minT25 = 0, maxT25 = 0;
    static size_t ints(int B) { return (size_t)NST * B + 2 * ((size_t)B + 1) + (size_t)B; }  // the host table
    static size_t toff_at(int B) { return (size_t)NST * B + 2 * ((size_t)B + 1); }
    void fill(int* h) const {  // the device image (host side)
        int* toff = h + toff_at(B);
        int64_t r = 0;
        for (int b = 0; b < B; ++b) {
            toff[b] = (int)r;
            r += plan[b].frames25;
        }
        for (int b = 0; b < B; ++b) {
            for (int st = 0; st < 5; ++st) h[st * B + b] = (int)plan[b].T[st];
            h[5 * B + b] = (int)plan[b].frames25;
            h[6 * B + b] = (int)plan[b].frames12;
        }
        unsigned* s0 = reinterpret_cast<unsigned*>(h + NST * B);
        unsigned* s1 = s0 + B + 1;
        s0[0] = s1[0] = 0;
        for (int b = 0; b < B; ++b) {
            s0[b + 1] = s0[b] + (unsigned)((plan[b].T[0] + 31) / 32);
            s1[b + 1] = s1[b] + (unsigned)((plan[b].T[1] + 31) / 32);
        }
    }
    double rows(int st) const {  // valid rows of stage st (0..4: T, 5: T25, 6: F) summed over the items
        double r = 0;
        for (const auto& p : plan) r += st < 5 ? (double)p.T[st] : st == 5 ? (double)p.frames25 : (double)p.frames12;
        return r;
    }
};

// Planes of the split-bf16 path: activations consumed only by GEMMs (resblock outputs, the last down conv's
// output, LayerNorm / attention / GELU outputs) are stored as NS bf16 planes instead of fp32 so the GEMMs
// only move bytes (gemm_planes.h).  0 = fp32 activations (f32 mode, or a clip so long that a batch item's
// plane exceeds the 2 GiB buffer-resource range).
static int act_planes(const mimi_engine* e, const StagePlan& p, int prec) {
    const int ns = prec == PREC_BF16X6 ? 3 : (prec == PREC_BF16X3 || prec == PREC_F16X3) ? 2 : 0;
    if (ns == 0) return 0;
    const mimi_config& c = e->cfg;
    int C = c.num_filters;
    for (int si = 0; si <= c.num_ratios; ++si) {
        if ((double)p.T[si] * C * 2 * 2 >= 2147483647.0) return 0;  // k*Cin span of the last row included
        C *= 2;
    }
    if ((double)p.frames25 * c.intermediate_size * 2 >= 2147483647.0) return 0;
    return ns;
}

static size_t ws_layout(const mimi_engine* e, int B, const StagePlan& p, int prec, bool ragged = false,
                        Workspace* w = nullptr, void* ws_base = nullptr) {
    const mimi_config& c = e->cfg;
    const int ns = act_planes(e, p, prec);
    // a plane-format buffer of n values takes ns * n bf16 = ns * n / 2 floats
    auto act = [&](size_t n) { return ns ? (n * ns + 1) / 2 : n; };
    size_t xmax = 0, ymax = 0, xemax = 0;
    int C = c.num_filters;
    for (int s = 0; s < c.num_ratios; ++s) {
        // x at stage 0 only holds the conv0 tap (the stage-0 block recomputes conv0 from the audio)
        if (s > 0 || e->taps) xmax = std::max(xmax, (size_t)p.T[s] * C);
        ymax = std::max(ymax, (size_t)p.T[s] * C);
        if (ns && s >= mimi_engine::kUnfuseFrom && s > 0) xemax = std::max(xemax, (size_t)p.T[s] * C);
        C *= 2;
    }
    xmax = std::max(xmax, act((size_t)p.T[c.num_ratios] * C));  // last down conv's (planes) output
    const size_t T = (size_t)p.frames25, Hd = (size_t)c.hidden_size;
    const size_t sizes[] = {xmax * B,
                            act(ymax * B),
                            T * Hd * B,
                            act(T * Hd * B),
                            T * 3 * Hd * B,
                            act(T * Hd * B),
                            act(T * (size_t)c.intermediate_size * B),
                            (size_t)p.frames12 * Hd * B,
                            (size_t)p.frames12 * 2 * c.vq_hidden_dim * B,
                            rvq_work_bytes((long long)p.frames12 * B) / sizeof(float),
                            act(xemax * B),
                            act(xemax / 2 * B),
                            ragged ? RaggedTable::ints(B) + (size_t)B * p.frames25 : 0};  // (+ rpos)
    size_t off = 0;
    float* rgp = nullptr;
    float** ptrs[] = {&w->x, &w->y, &w->t0, &w->t1, &w->qkv, &w->att, &w->ff, &w->dsout, &w->proj, &w->rvq,
                      &w->xe, &w->h, &rgp};
    char* base = reinterpret_cast<char*>(ws_base);
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
        if (w) *ptrs[i] = reinterpret_cast<float*>(base + off);
        off += ((sizes[i] * sizeof(float) + 255) / 256) * 256;
    }
    if (w) w->rg = reinterpret_cast<int*>(rgp);
    return off;
}

extern "C" int64_t mimi_workspace_bytes(const mimi_engine* e, int32_t batch, int64_t length) {
    if (!e || batch <= 0 || length <= 0) return -1;
    return (int64_t)ws_layout(e, batch, plan_lengths(e->cfg, length), e->precision);
}

// every lane's work done (each encode ends with its lane's ws_free, on whichever stream it ran)
static void drain_lanes(mimi_engine* e) {
    for (auto& l : e->lanes)
        if (l.ws_free) (void)hipEventSynchronize(l.ws_free);
}

// the lane's workspace (the other lane's encodes, workspace and graphs are untouched by a regrow)
static int ensure_ws(mimi_engine::Lane& lane, size_t bytes, hipStream_t s) {
    if (bytes <= lane.ws_bytes) return MIMI_OK;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventSynchronize(lane.ws_free));  // (the lane's last encode may have run on another stream)
    if (lane.ws) {
        HIP_TRY(hipFree(lane.ws));
        lane.ws = nullptr;
        lane.ws_bytes = 0;
    }
    hipError_t err = hipMalloc(&lane.ws, bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();  // clear it: the launch checks (hipGetLastError) must not see this failure
        lane.ws = nullptr;
        return set_err(err == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP,
                       "workspace hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(err));
    }
    lane.ws_bytes = bytes;
    ++lane.ws_gen;  // captured graphs address the old workspace
    return MIMI_OK;
}

static int ensure_rope(mimi_engine* e, int64_t T) {
    if (T <= e->rope_T) return MIMI_OK;
    const int half = e->cfg.head_dim / 2;
    const int64_t Tn = std::max<int64_t>(T, 256);
    std::vector<float> cs((size_t)Tn * half), sn((size_t)Tn * half);
    for (int d = 0; d < half; ++d) {
        // inv_freq = 1 / theta^(2d / dim) in float32 (TF/modeling_mimi.py:546), freq = inv_freq * pos in float32
        const float expo = (float)(2 * d) / (float)e->cfg.head_dim;
        const float pw = (float)std::pow((double)e->cfg.rope_theta, (double)expo);
        const float inv = 1.0f / pw;
        for (int64_t t = 0; t < Tn; ++t) {
            volatile float fr = inv * (float)t;
            cs[(size_t)t * half + d] = (float)std::cos((double)fr);
            sn[(size_t)t * half + d] = (float)std::sin((double)fr);
        }
    }
    if (e->rope_cos) {
        drain_lanes(e);  // the tables are shared: an encode in flight in either lane may still read them
        HIP_TRY(hipFree(e->rope_cos));
        HIP_TRY(hipFree(e->rope_sin));
    }
    HIP_TRY(hipMalloc(&e->rope_cos, cs.size() * 4));
    HIP_TRY(hipMalloc(&e->rope_sin, sn.size() * 4));
    HIP_TRY(hipMemcpy(e->rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    e->rope_T = Tn;
    ++e->rope_gen;
    return MIMI_OK;
}

static hipEvent_t pool_event(mimi_engine* e) {
    if (!e->event_pool.empty()) {
        hipEvent_t ev = e->event_pool.back();
        e->event_pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

struct Recorder {
    mimi_engine* e;
    hipStream_t s;
    int marks = 0;
    void begin() {
        if (!e->profiling) return;
        ProfEvent pe{"", pool_event(e), 0, 0};
        (void)hipEventRecord(pe.ev, s);
        e->pending.push_back(pe);
    }
    void mark(const std::string& name, double flops, double bytes, const char* kernel) {
        if (!e->profiling) return;
        if (e->profiling == 2 && marks++ >= 1) return;  // level 2: the pass's first stage only
        ProfEvent pe{name + "|" + kernel, pool_event(e), flops, bytes};
        (void)hipEventRecord(pe.ev, s);
        e->pending.push_back(pe);
    }
};

// the tap `name` as [b][t][ch] floats: its buffer grown to hold them, its dims set; *d = where the caller puts them
static int tap_buffer(mimi_engine* e, const char* name, int64_t b, int64_t t, int64_t ch, float** d) {
    auto& tp = e->tapmap[name];
    const size_t n = (size_t)(b * t * ch);
    if (tp.cap < n) {
        if (tp.d) HIP_TRY(hipFree(tp.d));
        HIP_TRY(hipMalloc(&tp.d, n * 4));
        tp.cap = n;
    }
    tp.dims[0] = b;
    tp.dims[1] = t;
    tp.dims[2] = ch;
    *d = tp.d;
    return MIMI_OK;
}

static int save_tap(mimi_engine* e, const char* name, const float* src, int64_t b, int64_t t, int64_t ch,
                    hipStream_t s) {
    if (!e->taps) return MIMI_OK;
    float* d;
    int rc;
    if ((rc = tap_buffer(e, name, b, t, ch, &d))) return rc;
    HIP_TRY(hipMemcpyAsync(d, src, (size_t)(b * t * ch) * 4, hipMemcpyDeviceToDevice, s));
    return MIMI_OK;
}

// tap of a plane-format activation (materialised as fp32 only when taps are on)
static int save_tap_planes(mimi_engine* e, const char* name, const void* planes, int ns, int64_t b, int64_t t,
                           int64_t ch, hipStream_t s, float hscale = 0.0f) {
    if (!e->taps) return MIMI_OK;
    if (ns == 0) return save_tap(e, name, reinterpret_cast<const float*>(planes), b, t, ch, s);
    float* d;
    int rc;
    if ((rc = tap_buffer(e, name, b, t, ch, &d))) return rc;
    const long long n = b * t * ch;
    HIP_TRY(launch_planes_to_f32(planes, n, ns, d, n, s, hscale));
    return MIMI_OK;
}

// layer l's tap of a decoder transformer stage, under the encode pass's name ("qkv3"); nothing is formatted when taps
// are off
static int save_tap_layer(mimi_engine* e, const char* stage, size_t l, const float* src, int64_t b, int64_t t,
                          int64_t ch, hipStream_t s) {
    if (!e->taps) return MIMI_OK;
    char nm[48];
    snprintf(nm, sizeof nm, "%s%d", stage, (int)l);
    return save_tap(e, nm, src, b, t, ch, s);
}

// A operand of a GEMM read from plane-format activations (plane stride = the activation's element count)
static void planes_in(GemmArgs& a, const void* planes, long long n) {
    a.Ap = planes;
    a.a_pstride = n;
}

static GemmArgs conv_args(const DevConv& cv, const float* in, int64_t Tin, float* out, int64_t Tout, int B) {
    GemmArgs a{};
    a.A = in;
    a.a_bstride = Tin * cv.cin;
    a.a_off = -(int64_t)(cv.k - cv.stride) * cv.cin;  // causal left pad
    a.a_rs = cv.stride * cv.cin;
    a.a_cin = cv.cin;
    a.a_len = Tin * cv.cin;
    a.W = cv.w;
    a.Wsplit = cv.wsplit;
    a.M = (int)Tout;
    a.N = cv.cout;
    a.K = cv.k * cv.cin;
    a.batch = B;
    a.bias = cv.b;
    a.C = out;
    a.c_bstride = Tout * cv.cout;
    a.ldc = cv.cout;
    return a;
}

static GemmArgs linear_args(const float* in, int64_t rows, int K, const float* W, int N, float* out) {
    GemmArgs a{};
    a.A = in;
    a.a_bstride = 0;
    a.a_off = 0;
    a.a_rs = K;
    a.a_cin = K;
    a.a_len = rows * K;
    a.W = W;
    a.M = (int)rows;
    a.N = N;
    a.K = K;
    a.batch = 1;
    a.C = out;
    a.c_bstride = 0;
    a.ldc = N;
    return a;
}

#define LAUNCH_TRY(expr, what)                                                                           \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) return set_err(MIMI_ERR_HIP, "launch %s: %s", what, hipGetErrorString(_e)); \
    } while (0)

static const char* ln_kname(int rpw) {
    switch (rpw) {
        case 1: return "mimi::layernorm_kernel<512, 1>";
        case 4: return "mimi::layernorm_kernel<512, 4>";
        case 8: return "mimi::layernorm_kernel<512, 8>";
        default: return "mimi::layernorm_kernel<512, 2>";
    }
}

// What an encode pass runs in and how: filled by the caller of the pass, read by everything the pass calls.  Nothing a
// pass needs about its lane, stream or mode lives on the engine, so passes in different lanes share no such state.
struct PassCtx {
    mimi_engine::Lane& lane;  // its workspace, ws_free, maxima buffers and io_dev
    hipStream_t s;
    int prec;
    const RaggedTable* rg = nullptr;  // a ragged batch: its length table ...
    const int* rg_pinned = nullptr;   // ... and the table's pinned host image, alive until the encode is waited
    bool capturing = false;    // inside capture_graph's stream capture: audio / codes through io_dev, no event calls
    bool chain_ok = false;     // the persistent RVQ chain may run: the caller reads its give-up flag back
    bool calibrating = false;  // calibrate_scales' pass: new tensor names are expected, every range check stays on
};

// What a pass hands back to its caller.
struct PassOut {
    unsigned* chain_flag = nullptr;  // the give-up flag word of the RVQ chain it launched (null: no chain ran)
    size_t chain_clear = 0;          // (capture) bytes from chain_flag that each replay zeroes first
    bool uncalibrated = false;       // it named a plane tensor the calibration did not see
};

static int run_rvq(mimi_engine* e, const PassCtx& ctx, const float* proj, int64_t frames, int K, int32_t* codes,
                   int frames_per_item, void* work, Recorder& rec, PassOut* out, const int* flen = nullptr,
                   double valid_share = 1.0) {
    RvqArgs r{};
    r.flen = flen;
    r.work = work;
    r.proj = proj;
    r.frames = frames;
    r.D = e->cfg.codebook_dim;
    r.ncodes = e->cfg.codebook_size;
    r.levels = K;
    r.nsem = e->cfg.num_semantic_quantizers;
    r.cb_frag = e->cb_frag;
    r.cb_rows = e->cb_rows;
    r.cb_norm = e->cb_norm;
    r.cb_h16 = e->cb_h16;
    r.cb_unscale = e->cb_unscale;
    r.cb_emax = e->cb_emax;
    r.codes = codes;
    r.codes_ref = ctx.capturing ? reinterpret_cast<int32_t* const*>(ctx.lane.io_dev + 1) : nullptr;
    r.frames_per_item = frames_per_item;
    r.form = e->rvq_form;
    r.chain = e->rvq_chain;
    r.chain_fault = e->rvq_chain_fault;
    r.xcd_group_ok = e->rvq_xcd;
    const char* kname = "?";
    out->chain_flag = nullptr;
    out->chain_clear = 0;  // (capturing: the replay's set_io_kernel zeroes the chain's words instead of a memset node)
    LAUNCH_TRY(launch_rvq(r, ctx.s, &kname, ctx.chain_ok ? &out->chain_flag : nullptr,
                          ctx.capturing ? &out->chain_clear : nullptr),
               "rvq");
    rec.mark("rvq", 2.0 * frames * valid_share * r.D * r.ncodes * K,
             (double)frames * (2 * r.D) * 4 + (double)frames * K * 4, kname);
    return MIMI_OK;
}

// One pass of the whole encode at precision ctx.prec, behind the lane's last encode.  On fp16 planes it zeroes the
// lane's maxima first, and a tensor without a calibrated scale is an error of this encode only (its name is known
// from here on).  Inside a capture only the stages are legal: the replay waits outside its graph and needs no reset
// node (capture_graph), which reads out->uncalibrated itself.
static int encode_pass(mimi_engine* e, const PassCtx& ctx, const float* audio, int B, int64_t L, int K, int32_t* codes,
                       PassOut* out = nullptr) {
    const mimi_config& c = e->cfg;
    const StagePlan p = plan_lengths(c, L);
    hipStream_t s = ctx.s;
    const int prec = ctx.prec;
    const RaggedTable* rg = ctx.rg;
    PassOut unread;
    if (!out) out = &unread;
    *out = PassOut{};
    Workspace w{};
    int rc = ensure_ws(ctx.lane, ws_layout(e, B, p, prec, rg != nullptr), s);
    if (rc) return rc;
    ws_layout(e, B, p, prec, rg != nullptr, &w, ctx.lane.ws);
    if ((rc = ensure_rope(e, p.frames25))) return rc;
    const int ns = act_planes(e, p, prec);  // 0: fp32 activations; 2/3: plane-format GEMM inputs
    // fp16 planes: each plane-format tensor takes the next activation-scale slot (launch order)
    const bool h16 = prec == PREC_F16X3 && ns == 2;
    struct Act {
        float scale = 0.0f;  // > 0: fp16 planes of x * scale
        unsigned* amax = nullptr;
    };
    // the activation-scale slot of plane tensor `name` (fixed names, so a tensor keeps its scale whatever the
    // batch, length or code path); new names only while calibrating
    auto new_act = [&](const std::string& name) {
        Act a;
        if (!h16) return a;
        auto it = e->slot_of.find(name);
        int slot;
        if (it != e->slot_of.end()) {
            slot = it->second;
        } else {
            if (!ctx.calibrating) out->uncalibrated = true;
            if ((int)e->slot_of.size() >= kMaxActSlots) return a;
            slot = (int)e->slot_of.size();
            e->slot_of[name] = slot;
            e->act_scale.resize(slot + 1, 1.0f);
        }
        a.scale = e->act_scale[slot];
        a.amax = ctx.lane.amax_dev + (size_t)slot * AMAX_SLOT_WORDS;
        return a;
    };
    // a LayerNorm output whose bound (DevXfmr::ln*_bound) times its scale stays under half the fp16 plane limit
    // (2^15) needs no range check (calibration still records its maximum: it sets the scale)
    auto ln_check_free = [&](const Act& a, float bound) {
        return MIMI_LN_CHECK_SKIP && !ctx.calibrating && a.amax && a.scale > 0.0f && bound * a.scale < 16384.0f;
    };
    // fp16 weight planes + 1 / (activation scale x weight scale) for a GEMM reading plane tensor `in`
    auto use_h = [&](GemmArgs& a, const void* wh, float wscale, const Act& in) {
        if (!h16) return;
        a.Wsplit = wh;
        a.unscale = 1.0f / (in.scale * wscale);
    };
    auto out_act = [&](GemmArgs& a, const Act& o) {
        a.out_scale = o.scale;
        a.out_amax = o.amax;
    };
    Recorder rec{e, s};
    const char* kname = "?";
    if (!ctx.capturing) {
        // (the lane's last encode may have run on another stream, and the maxima buffers are part of its workspace)
        HIP_TRY(hipStreamWaitEvent(s, ctx.lane.ws_free, 0));
        if (h16) HIP_TRY(hipMemsetAsync(ctx.lane.amax_dev, 0, (size_t)kMaxActSlots * AMAX_SLOT_WORDS * sizeof(unsigned), s));
    }
    // ragged batches: the length table (pinned host image, alive until the encode is waited) -> workspace
    const int* dT[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const int *dT25 = nullptr, *dF = nullptr;
    const unsigned *dst0 = nullptr, *dst1 = nullptr;
    const int *dToff = nullptr, *dRpos = nullptr;  // the transformer section's packed rows (RaggedTable)
    if (rg) {
        if (!ctx.rg_pinned || rg->B != B || !w.rg) return set_err(MIMI_ERR_STATE, "ragged encode without its length table");
        HIP_TRY(hipMemcpyAsync(w.rg, ctx.rg_pinned, RaggedTable::ints(B) * sizeof(int), hipMemcpyHostToDevice, s));
        for (int st = 0; st < 5; ++st) dT[st] = w.rg + st * B;
        dT25 = w.rg + 5 * B;
        dF = w.rg + 6 * B;
        dst0 = reinterpret_cast<const unsigned*>(w.rg + RaggedTable::NST * B);
        dst1 = dst0 + B + 1;
        dToff = w.rg + RaggedTable::toff_at(B);
        dRpos = w.rg + RaggedTable::ints(B);
        LAUNCH_TRY(launch_ragged_rows(w.rg + 5 * B, dToff, B, w.rg + RaggedTable::ints(B), s), "ragged rows");
    }
    // (profile bookkeeping) a GEMM's algorithmic FLOPs over the items' valid rows
    auto rows_of = [&](int st, double uniform) { return rg ? rg->rows(st) : uniform; };
    rec.begin();
    auto gemm_flops = [](const GemmArgs& a) { return 2.0 * a.batch * (double)a.M * a.N * a.K; };
    auto gemm_bytes = [](const GemmArgs& a, bool res) {
        // algorithmic: activation span read once, output written once (+ residual read), weights once
        const double in = (double)a.batch * a.a_len * 4, out = (double)a.batch * a.M * a.N * 4;
        return in + out * (res ? 2 : 1) + (double)a.N * a.K * 4;
    };

    // ---- SEANet encoder ----
    // conv0 is fused into the stage-0 residual block (x0 is recomputed per tile from the audio); the standalone
    // conv0 kernel only runs to materialise the "conv0" tap for per-stage parity tests.
    if (e->taps) {
        LAUNCH_TRY(launch_conv0(audio, L, B, e->conv0.w, e->conv0.b, w.x, c.num_filters, c.kernel_size, s), "conv0");
        if ((rc = save_tap(e, "conv0", w.x, B, p.T[0], c.num_filters, s))) return rc;
    }
    int C = c.num_filters;
    char nm[64];
    Act yact, xact, xeact, hact;  // the tensors currently held by y, x (last down conv), xe, h
    const auto nmf = [](const char* fmt, int i) {
        char b[48];
        snprintf(b, sizeof b, fmt, i);
        return std::string(b);
    };
    for (int si = 0; si < c.num_ratios; ++si) {
        const int64_t T = p.T[si];
        const bool unf = ns && si > 0 && si >= mimi_engine::kUnfuseFrom;
        if (!unf) {
            ResArgs ra{};
            ra.x = w.x;
            if (si == 0) {
                ra.audio = audio;
                ra.audio_ref = ctx.capturing ? const_cast<const float* const*>(reinterpret_cast<float**>(ctx.lane.io_dev)) : nullptr;
                ra.w0 = e->conv0.w;
                ra.b0 = e->conv0.b;
                ra.w3frag = e->res3[0].wfrag;
                ra.w1frag = e->res1[0].wfrag;
            }
            ra.T = T;
            ra.batch = B;
            if (rg) {
                ra.ilen = dT[si];
                ra.istart = si == 0 ? dst0 : dst1;
            }
            ra.w3 = e->res3[si].w;
            ra.b3 = e->res3[si].b;
            ra.w1 = e->res1[si].w;
            ra.b1 = e->res1[si].b;
            ra.y = w.y;
            ra.yp = w.y;
            ra.y_pstride = (long long)B * T * C;
            ra.yns = ns;
            yact = new_act(nmf("y%d", si));
            ra.yscale = yact.scale;
            ra.yamax = yact.amax;
            if (h16 && (si > 1 || (si == 0 && !e->res0_h16) || (si == 1 && !(C == 128 && e->res1_h16))))
                return set_err(MIMI_ERR_UNSUPPORTED, "f16x3: no fp16 fused block for stage %d", si);
            if (h16 && (unsigned long long)B * (unsigned long long)((T + 31) / 32) >= (1ull << 32))
                return set_err(MIMI_ERR_UNSUPPORTED, "f16x3: %d x %lld steps exceed the block index range", B,
                               (long long)T);
            if (si == 0 && h16) {
                // fp16-plane stage-0 block: audio, ELU(x0) and ELU(h) are split in-kernel, each at its own scale
                const Act aa = new_act("s0.audio"), xa = new_act("s0.x"), ha = new_act("s0.h");
                ra.wh16 = e->res0_h16;
                ra.ascale = aa.scale;
                ra.xscale = xa.scale;
                ra.hscale = ha.scale;
                ra.unscale0 = 1.0f / (aa.scale * e->res0_wsc[0]);
                ra.unscale1 = 1.0f / (xa.scale * e->res0_wsc[1]);
                ra.unscale2 = 1.0f / (ha.scale * e->res0_wsc[2]);
                ra.aamax = aa.amax;
                ra.xamax = xa.amax;
                ra.hamax = ha.amax;
            }
            if (si == 1 && h16) {
                // fp16-plane stage-1 block: ELU(x) and ELU(h) split in-kernel at their own scales
                const Act xa = new_act("s1.x"), ha = new_act("s1.h");
                ra.wh16 = e->res1_h16;
                ra.xscale = xa.scale;
                ra.hscale = ha.scale;
                ra.unscale1 = 1.0f / (xa.scale * e->res1_wsc[0]);
                ra.unscale2 = 1.0f / (ha.scale * e->res1_wsc[1]);
                ra.xamax = xa.amax;
                ra.hamax = ha.amax;
                ra.form = e->res1_form;
            }
            if (rg && !(h16 && (si == 0 || si == 1))) return set_err(MIMI_ERR_UNSUPPORTED, "ragged: fp16 blocks only");
            const double H = C / c.compress;
            const double BT = rows_of(si, (double)B * T);
            const double fl = 2.0 * BT * (3.0 * C * H + H * C) + (si == 0 ? 2.0 * BT * C * c.kernel_size : 0.0);
            const DevConv& dc0 = e->down[0];
            bool t1_ceil = p.T[1] == (T + 3) / 4;  // the kernel's output steps: ceil(T0 / 4) per item
            if (rg)
                for (int b = 0; b < B; ++b) t1_ceil = t1_ceil && rg->plan[b].T[1] == (rg->plan[b].T[0] + 3) / 4;
            if (si == 0 && h16 && e->stage0_fused && C == 64 && dc0.cin == 64 && dc0.cout == 128 &&
                dc0.k == 8 && dc0.stride == 4 && dc0.wh && dc0.b && t1_ceil) {
                // y stays on chip: the block's output feeds down conv 0 in the same kernel (x1 = its fp32 output)
                ra.wdown = dc0.wh;
                ra.bdown = dc0.b;
                ra.unscale_d = 1.0f / (yact.scale * dc0.wscale);
                ra.xout = w.x;
                ra.T1 = p.T[1];
                ra.yp = e->taps ? w.y : nullptr;  // taps only: y planes to HBM as well
                LAUNCH_TRY(launch_stage0_fused(ra, s, &kname), "stage 0 + down conv 0");
                const double BT1 = rows_of(1, (double)B * p.T[1]);
                const double fld = 2.0 * BT1 * 128.0 * 512.0;
                // HBM: audio in, x1 out, both weight sets (y never leaves the CU)
                const double by = BT * 4 + BT1 * 128 * 4 + (3.0 * C * H + H * C) * 4 + 128.0 * 512 * 4;
                rec.mark("res_down_s0", fl + fld, by, kname);
                if ((rc = save_tap_planes(e, "res0_elu", w.y, ns, B, T, C, s, yact.scale))) return rc;
                if ((rc = save_tap_planes(e, "down0", w.x, 0, B, p.T[1], 2 * C, s, 0.0f))) return rc;
                C *= 2;
                continue;
            }
            LAUNCH_TRY(launch_resblock(C, ra, s, &kname), "resblock");
            snprintf(nm, sizeof nm, "res_s%d", si);
            const double by = BT * 4 * (si == 0 ? 1 + C : 2 * C) + (3.0 * C * H + H * C) * 4;
            rec.mark(nm, fl, by, kname);
        } else {
            // two plane GEMMs: h = ELU(b3 + W3 (*) ELU(x)) from the ELU(x) planes the down conv wrote, then
            // y = ELU(x + b1 + W1 . h) with the fp32 x as the skip
            const int Hh = C / c.compress;
            GemmArgs a3 = conv_args(e->res3[si], nullptr, T, nullptr, T, B);
            planes_in(a3, w.xe, (long long)B * T * C);
            use_h(a3, e->res3[si].wh, e->res3[si].wscale, xeact);
            a3.Cp = w.h;
            a3.c_pstride = (long long)B * T * Hh;
            if (rg) a3.a_rows = a3.m_rows = dT[si];
            hact = new_act(nmf("h%d", si));
            out_act(a3, hact);
            LAUNCH_TRY(launch_gemm(ROLE_RES3P, a3, s, &kname, prec), "res3");
            snprintf(nm, sizeof nm, "res3_s%d", si);
            rec.mark(nm, gemm_flops(a3) * rows_of(si, (double)B * T) / ((double)B * T), gemm_bytes(a3, false), kname);
            // (taps only) h, so that the k3 and the k1 conv of an unfused block can each be checked on its own input
            if ((rc = save_tap_planes(e, nmf("h%d", si).c_str(), w.h, ns, B, T, Hh, s, hact.scale))) return rc;
            GemmArgs a1 = conv_args(e->res1[si], nullptr, T, nullptr, T, B);
            planes_in(a1, w.h, (long long)B * T * Hh);
            use_h(a1, e->res1[si].wh, e->res1[si].wscale, hact);
            a1.R = w.x;
            a1.Cp = w.y;
            a1.c_pstride = (long long)B * T * C;
            if (rg) a1.a_rows = a1.m_rows = dT[si];
            yact = new_act(nmf("y%d", si));
            out_act(a1, yact);
            if (h16 && e->res1_stream && res1_stream_ok(a1) && (e->res1_stream == 2 || a1.K == 128))
                LAUNCH_TRY(launch_res1_stream(a1, s, &kname), "res1 stream");
            else
                LAUNCH_TRY(launch_gemm(ROLE_RES1P, a1, s, &kname, prec), "res1");
            snprintf(nm, sizeof nm, "res1_s%d", si);
            rec.mark(nm, gemm_flops(a1) * rows_of(si, (double)B * T) / ((double)B * T), gemm_bytes(a1, true), kname);
        }
        snprintf(nm, sizeof nm, "res%d_elu", si);
        if ((rc = save_tap_planes(e, nm, w.y, ns, B, T, C, s, yact.scale))) return rc;
        const bool last = si == c.num_ratios - 1;
        const bool next_unf = ns && !last && si + 1 >= mimi_engine::kUnfuseFrom;
        GemmArgs ad = conv_args(e->down[si], w.y, T, w.x, p.T[si + 1], B);
        int role = last ? ROLE_DOWN_ELU : ROLE_DOWN;
        if (ns) {
            planes_in(ad, w.y, (long long)B * T * C);
            use_h(ad, e->down[si].wh, e->down[si].wscale, yact);
            if (last) {  // only the final conv reads it: planes out
                ad.Cp = w.x;
                ad.c_pstride = (long long)B * p.T[si + 1] * 2 * C;
                ad.C = nullptr;
                xact = new_act("x_last");
                out_act(ad, xact);
            } else if (next_unf) {  // fp32 x (the skip) + ELU(x) planes (the next k3 conv's input)
                ad.Cp = w.xe;
                ad.c_pstride = (long long)B * p.T[si + 1] * 2 * C;
                role = ROLE_DOWN_XE;
                xeact = new_act(nmf("xe%d", si + 1));
                out_act(ad, xeact);
            }
        }
        if (rg) {
            ad.a_rows = dT[si];
            ad.m_rows = dT[si + 1];
        }
        LAUNCH_TRY(launch_gemm(role, ad, s, &kname, prec, rg ? 0 : e->gemm256), "down");
        snprintf(nm, sizeof nm, "down_s%d", si);
        rec.mark(nm, gemm_flops(ad) * rows_of(si + 1, (double)B * p.T[si + 1]) / ((double)B * p.T[si + 1]),
                 gemm_bytes(ad, false), kname);
        snprintf(nm, sizeof nm, last ? "down%d_elu" : "down%d", si);
        if ((rc = save_tap_planes(e, nm, w.x, last ? ns : 0, B, p.T[si + 1], 2 * C, s, last ? xact.scale : 0.0f)))
            return rc;
        C *= 2;
    }
    const int64_t T = p.frames25;
    const int Hd = c.hidden_size;
    GemmArgs af = conv_args(e->final_conv, w.x, p.T[c.num_ratios], w.t0, T, B);
    if (ns) planes_in(af, w.x, (long long)B * p.T[c.num_ratios] * C);
    use_h(af, e->final_conv.wh, e->final_conv.wscale, xact);
    if (rg) {  // ragged: the output rows packed (item b's frames from row toff[b] on) for the transformer section
        af.a_rows = dT[c.num_ratios];
        af.m_rows = dT25;
        af.c_boff = dToff;
    }
    LAUNCH_TRY(launch_gemm(ROLE_FINAL, af, s, &kname, prec), "final");
    const double rT25 = rows_of(5, (double)B * p.frames25) / ((double)B * p.frames25);  // ragged share of the rows
    rec.mark("final", gemm_flops(af) * rT25, gemm_bytes(af, false), kname);
    // ---- transformer (x in t0) ----
    // rows: B x T, or for a ragged batch the items' frames PACKED back to back (R rows): every row-local stage
    // (LayerNorm, q/k/v, o_proj, fc1, fc2) then runs the uniform kernels over exactly the valid rows -- no per-item
    // tiles half empty -- and computes each row with the same instruction sequence as the per-item form; attention
    // and the downsample address the items through toff, RoPE takes each row's position from rpos
    const int64_t rows = rg ? rg->R : (int64_t)B * T;
    const int64_t tapB = rg ? 1 : B, tapT = rg ? rg->R : T;  // (ragged taps of the transformer section: packed)
    if ((rc = save_tap(e, "encoder", w.t0, tapB, tapT, Hd, s))) return rc;
    const int H = c.num_attention_heads, Dh = c.head_dim;
    // f16x3: downsample + input projections on fp16 planes too (zero-padded GEMM + replicate-edge fix)
    const bool ds_planes = h16 && e->ds_fix && e->inproj_h && c.downsample_kernel == 4 && c.downsample_stride == 2;
    Act dsin, dsouta;
    double att_flops = 0;
    auto att_fl = [&](int64_t Tn) {
        double f = 0;
        for (int64_t i = 0; i < Tn; ++i) f += 4.0 * Dh * std::min<int64_t>(i + 1, c.sliding_window);
        return f * H;
    };
    if (rg) {
        for (const auto& pb : rg->plan) att_flops += att_fl(pb.frames25);
    } else {
        att_flops = att_fl(T) * B;
    }
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const DevXfmr& x = e->xf[l];
        const long long nact = rows * Hd;
        Act t1a = new_act(nmf("xf%d.ln1", l));
        if (ln_check_free(t1a, x.ln1_bound)) t1a.amax = nullptr;
        // LayerNorm + fc1 (ln_fused >= 1) / q/k/v (ln_fused 2): on small grids one launch whose tiles compute their
        // rows' LayerNorm (the same bits as the LayerNorm kernel's planes, gemm_planes.h FL_LNA)
        auto ln_into = [&](GemmArgs& g, int role, const float* lw, const float* lb, const Act& act) {
            if (!h16 || e->ln_fused < (role == ROLE_QKV ? 2 : 1) || !gemm_ln_prologue_ok(role, g, prec, rg ? 0 : e->gemm256)) return false;
            if (role == ROLE_QKV) g.ln_tile = e->ln_fused - 2;  // (2: 16x64, 3: 32x64, 4: 16x128 tiles)
            g.ln_x = w.t0;
            g.ln_g = lw;
            g.ln_b = lb;
            g.ln_eps = c.norm_eps;
            g.ln_scale = act.scale;
            g.ln_amax = act.amax;
            return true;
        };
        GemmArgs aq = linear_args(w.t1, T, Hd, x.wqkv, 3 * H * Dh, w.qkv);
        aq.Wsplit = x.wqkv_s;
        aq.batch = B;
        aq.a_bstride = T * Hd;
        aq.c_bstride = T * 3 * H * Dh;
        aq.rope_cos = e->rope_cos;
        aq.rope_sin = e->rope_sin;
        aq.rope_cols = 2 * H * Dh;
        if (rg) {  // packed rows: one flat GEMM, RoPE positions from rpos
            aq = linear_args(w.t1, rows, Hd, x.wqkv, 3 * H * Dh, w.qkv);
            aq.Wsplit = x.wqkv_s;
            aq.rope_cos = e->rope_cos;
            aq.rope_sin = e->rope_sin;
            aq.rope_cols = 2 * H * Dh;
            aq.rope_pos = dRpos;
        }
        if (ns) planes_in(aq, w.t1, nact);
        use_h(aq, x.wqkv_h, x.wqkv_hs, t1a);
        // q/k/v + attention in one kernel (qkv_attn.hip): large batches of items <= 256 frames, fp16 planes
        const bool fuse_qa = h16 && ns && e->qkv_attn && Dh == 64 && (rg ? rg->maxT25 <= 256 : T <= 256) &&
                             (e->qkv_attn == 2 || (long long)B * H >= 256);
        if (fuse_qa || !ln_into(aq, ROLE_QKV, x.ln1_w, x.ln1_b, t1a)) {
            LAUNCH_TRY(launch_layernorm(w.t0, x.ln1_w, x.ln1_b, w.t1, rows, Hd, c.norm_eps, s, w.t1, nact, ns, t1a.scale,
                                        t1a.amax, nullptr, 0, e->ln_rpw),
                       "ln1");
            rec.mark("layernorm", 0, 2.0 * rows * Hd * 4, ln_kname(e->ln_rpw));
        }
        const Act atta = new_act(nmf("xf%d.att", l));
        if (fuse_qa) {
            QkvAttnArgs qa{};
            qa.Ap = aq.Ap;
            qa.a_pstride = aq.a_pstride;
            qa.a_rows = rows;
            qa.Wp = aq.Wsplit;
            qa.unscale = aq.unscale;
            qa.rope_cos = e->rope_cos;
            qa.rope_sin = e->rope_sin;
            qa.K = Hd;
            qa.Ts = (int)T;
            qa.H = H;
            qa.window = c.sliding_window;
            qa.scale = 1.0f / std::sqrt((float)Dh);
            qa.outp = w.att;
            qa.out_pstride = nact;
            qa.oscale = atta.scale;
            qa.oamax = atta.amax;
            qa.tlen = rg ? dT25 : nullptr;
            qa.toff = rg ? dToff : nullptr;
            qa.qkv = e->taps ? w.qkv : nullptr;  // (the q/k/v tap, as the GEMM would have stored it)
            qa.xcd = e->qkv_attn_xcd;
            LAUNCH_TRY(launch_qkv_attention(qa, B, s), "qkv_attention");
            rec.mark("qkv_attention", gemm_flops(aq) + att_flops, (double)rows * Hd * 4 * 2 + 3.0 * H * Dh * Hd * 4,
                     "mimi::qkv_attention_h16_kernel<512>");
            if ((rc = save_tap(e, nmf("qkv%d", l).c_str(), w.qkv, tapB, tapT, 3 * H * Dh, s))) return rc;
        } else {
            aq.sc1 = (e->sc1_out & 1) != 0;
            LAUNCH_TRY(launch_gemm(ROLE_QKV, aq, s, &kname, prec), "qkv");
            rec.mark("qkv", gemm_flops(aq), gemm_bytes(aq, false), kname);
            if ((rc = save_tap(e, nmf("qkv%d", l).c_str(), w.qkv, tapB, tapT, 3 * H * Dh, s))) return rc;
            // fp16-plane attention in f16x3 mode (also for the no-plane long clips: the same arithmetic as their
            // prefixes); true fp32 in f32 mode and the bf16 modes
            const bool ah16 = prec == PREC_F16X3;
            const char* akn = ah16 ? (T <= 256 ? "mimi::attention_t256_h16_kernel" : "mimi::attention_band_h16_kernel")
                                   : (T <= 256 ? "mimi::attention_t256_kernel" : "mimi::attention_kernel");
            LAUNCH_TRY(launch_attention(w.qkv, w.att, B, (int)T, H, Dh, c.sliding_window, 1.0f / std::sqrt((float)Dh),
                                        s, w.att, nact, ns, atta.scale, atta.amax, ah16, rg ? dT25 : nullptr,
                                        rg ? rg->maxT25 : 0, rg ? rg->minT25 : 0, dToff, &akn, e->attn_band_split),
                       "attention");
            rec.mark("attention", att_flops, (double)rows * 4 * Hd * 4, akn);
        }
        if ((rc = save_tap_planes(e, nmf("att%d", l).c_str(), w.att, ns, tapB, tapT, H * Dh, s, atta.scale))) return rc;
        GemmArgs ao = linear_args(w.att, rows, H * Dh, x.wo, Hd, w.t0);
        ao.Wsplit = x.wo_s;
        ao.R = w.t0;
        ao.scale = x.ls1;
        if (ns) planes_in(ao, w.att, nact);
        use_h(ao, x.wo_h, x.wo_hs, atta);
        ao.sc1 = (e->sc1_out & 4) != 0;
        Act t1b = new_act(nmf("xf%d.ln2", l));
        if (ln_check_free(t1b, x.ln2_bound)) t1b.amax = nullptr;
        LAUNCH_TRY(launch_gemm(ROLE_OPROJ, ao, s, &kname, prec), "o_proj");
        rec.mark("o_proj", gemm_flops(ao), gemm_bytes(ao, true), kname);
        if ((rc = save_tap(e, nmf("oproj%d", l).c_str(), w.t0, tapB, tapT, Hd, s))) return rc;
        GemmArgs a1 = linear_args(w.t1, rows, Hd, x.w1, c.intermediate_size, w.ff);
        a1.Wsplit = x.w1_s;
        Act ffa;
        if (ns) {
            planes_in(a1, w.t1, nact);
            use_h(a1, x.w1_h, x.w1_hs, t1b);
            a1.Cp = w.ff;  // only fc2 reads it: planes out
            a1.c_pstride = rows * c.intermediate_size;
            a1.C = nullptr;
            ffa = new_act(nmf("xf%d.ff", l));
            out_act(a1, ffa);
        }
        if (!ln_into(a1, ROLE_FC1, x.ln2_w, x.ln2_b, t1b)) {
            LAUNCH_TRY(launch_layernorm(w.t0, x.ln2_w, x.ln2_b, w.t1, rows, Hd, c.norm_eps, s, w.t1, nact, ns, t1b.scale,
                                        t1b.amax, nullptr, 0, e->ln_rpw),
                       "ln2");
            rec.mark("layernorm", 0, 2.0 * rows * Hd * 4, ln_kname(e->ln_rpw));
        }
        a1.sc1 = (e->sc1_out & 2) != 0;
        a1.ncg = e->fc1_cg;
        LAUNCH_TRY(launch_gemm(ROLE_FC1, a1, s, &kname, prec, rg ? 0 : e->gemm256), "fc1");
        rec.mark("fc1", gemm_flops(a1), gemm_bytes(a1, false), kname);
        if ((rc = save_tap_planes(e, nmf("ff%d", l).c_str(), w.ff, ns, tapB, tapT, c.intermediate_size, s, ffa.scale)))
            return rc;
        GemmArgs a2 = linear_args(w.ff, rows, c.intermediate_size, x.w2, Hd, w.t0);
        a2.Wsplit = x.w2_s;
        a2.R = w.t0;
        a2.scale = x.ls2;
        if (ns) planes_in(a2, w.ff, rows * (long long)c.intermediate_size);
        use_h(a2, x.w2_h, x.w2_hs, ffa);
        if (ds_planes && l == c.num_hidden_layers - 1) {  // + planes of the encoder output: the downsample's A
            a2.Cp = w.t1;
            a2.c_pstride = nact;
            dsin = new_act("ds.in");
            out_act(a2, dsin);
        }
        a2.sc1 = (e->sc1_out & 4) != 0;
        LAUNCH_TRY(launch_gemm(ROLE_FC2, a2, s, &kname, prec), "fc2");
        rec.mark("fc2", gemm_flops(a2), gemm_bytes(a2, true), kname);
        snprintf(nm, sizeof nm, "xfmr%d", l);
        if ((rc = save_tap(e, nm, w.t0, tapB, tapT, Hd, s))) return rc;
    }

    // ---- downsample (replicate pad) + input projections + RVQ ----
    const int64_t T2 = p.frames12;
    GemmArgs ad = conv_args(e->ds, w.t0, T, w.dsout, T2, B);
    if (ds_planes) {
        planes_in(ad, w.t1, rows * Hd);
        use_h(ad, e->ds.wh, e->ds.wscale, dsin);
        ad.Cp = w.att;  // planes of the downsample output (the input projection's A); fp32 C beside
        ad.c_pstride = (long long)B * T2 * Hd;
        dsouta = new_act("ds.out");
        out_act(ad, dsouta);
    }
    if (rg) {  // the packed encoder output in, per-item frames out
        if (!ds_planes) return set_err(MIMI_ERR_UNSUPPORTED, "ragged: planes downsample only");
        ad.a_rows = dT25;
        ad.m_rows = dF;
        ad.a_boff = dToff;
    }
    LAUNCH_TRY(launch_gemm(ROLE_DOWNSAMPLE, ad, s, &kname, prec), "downsample");
    if ((rc = save_tap(e, "ds_gemm", w.dsout, B, T2, Hd, s))) return rc;  // (before the replicate-pad rows)
    if (ds_planes)
        LAUNCH_TRY(launch_ds_edge_fix(w.t0, e->ds_fix, w.dsout, w.att, ad.c_pstride, dsouta.scale, dsouta.amax, B,
                                      (int)T, (int)T2, Hd, Hd, s, rg ? dT25 : nullptr, rg ? dF : nullptr, dToff),
                   "downsample edges");
    const double rF = rows_of(6, (double)B * T2) / ((double)B * T2);
    rec.mark("downsample", gemm_flops(ad) * rF, gemm_bytes(ad, false), kname);
    if ((rc = save_tap(e, "downsample", w.dsout, B, T2, Hd, s))) return rc;
    const int Dq = c.vq_hidden_dim;
    GemmArgs ap = linear_args(w.dsout, (int64_t)B * T2, Hd, e->inproj, 2 * Dq, w.proj);
    if (ds_planes) {
        planes_in(ap, w.att, (long long)B * T2 * Hd);
        use_h(ap, e->inproj_h, e->inproj_hs, dsouta);
    }
    if (rg) {  // ragged: per item (batch B, M = T2 frames each, the valid ones per item) -- the same instruction
               // sequence per output as the flattened [B x T2] form
        ap.batch = B;
        ap.M = (int)T2;
        ap.a_bstride = T2 * Hd;
        ap.c_bstride = T2 * 2 * Dq;
        ap.a_len = T2 * Hd;
        ap.a_rows = ap.m_rows = dF;
    }
    LAUNCH_TRY(launch_gemm(ROLE_INPROJ, ap, s, &kname, ds_planes ? PREC_F16X3 : PREC_F32), "input_proj");
    rec.mark("input_proj", gemm_flops(ap) * rF, gemm_bytes(ap, false), kname);
    if ((rc = save_tap(e, "proj", w.proj, B, T2, 2 * Dq, s))) return rc;
    if ((rc = run_rvq(e, ctx, w.proj, (int64_t)B * T2, K, codes, (int)T2, w.rvq, rec, out, rg ? dF : nullptr, rF)))
        return rc;
    if (ctx.capturing) return MIMI_OK;
    HIP_TRY(hipEventRecord(ctx.lane.ws_free, s));
    if (out->uncalibrated) return set_err(MIMI_ERR_STATE, "f16x3: an activation has no calibrated scale");
    return MIMI_OK;
}

// Activation scales (PREC_F16X3).  A plane tensor with max|x| = a stored at scale s keeps every element's full
// 22-bit significand down to 2^-3 / s (h1 = fp16(x s - h0) normal) and an absolute error <= 2^-25 / s below;
// a s < 2^15 keeps x s (and h0) finite.  The scales are FIXED per tensor name: mimi_finalize runs a calibration
// encode on three full-scale 10 s signals (calibrate_scales) and puts every tensor's calibration maximum at
// a s in [2^7, 2^8).  They never follow the caller's audio, so an item's codes are a pure function of its own
// samples and the padded length -- not of its batch-mates or of what the engine encoded before (the reference
// is a pure function of the batch too, TF/modeling_mimi.py:1297-1386).  A tensor 2^7 x louder than the
// calibration's loudest would overflow: every encode reads the per-tensor maxima back, and on an overflow each
// item is re-encoded alone (at the same padded length) and, if it overflows alone, in the scale-free bf16x6
// arithmetic -- so the fallback too depends on the item alone.  Quieter tensors need no action: their
// absolute error stays <= 2^-25 / s = 2^-32..2^-33 of the calibration maximum.
constexpr float kF16Overflow = 32768.0f;  // a s >= 2^15: x s may round to an fp16 infinity

// folds and reads back the per-slot maxima of the lane's last pass (synchronises s)
static int read_amax(mimi_engine* e, mimi_engine::Lane& lane, hipStream_t s, int* n) {
    const int ns = (int)e->slot_of.size();
    *n = ns;
    if (ns == 0) return MIMI_OK;
    LAUNCH_TRY(launch_amax_reduce(lane.amax_dev, ns, lane.amax_red, s), "amax_reduce");
    HIP_TRY(hipMemcpyAsync(e->amax_host, lane.amax_red, ns * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MIMI_OK;
}

static float amax_word(const unsigned* amax, int i) {
    float a;
    std::memcpy(&a, &amax[i], 4);
    return a;
}

// Whether any of n per-tensor maxima of a B-item pass overflows its scale.  A non-finite maximum is not an overflow
// of the scale: it comes from a non-finite input, which the reference propagates too -- so an item alone keeps its
// f16x3 codes.  In a batch the maxima are per tensor over all items, and +inf orders above every finite value: one
// item's Inf would hide a loud batch-mate's overflow, so there it sends every item to its own pass (where the item
// that owns the Inf is alone, and a loud one is seen).
static bool f16_overflow(const unsigned* amax, int n, const std::vector<float>& act_scale, int B) {
    for (int i = 0; i < n; ++i) {
        const float a = amax_word(amax, i);
        if (!std::isfinite(a)) {
            if (B > 1) return true;
            continue;
        }
        if (a * act_scale[i] >= kF16Overflow) return true;
    }
    return false;
}

// one f16x3 pass and its overflow check
static int f16_pass(mimi_engine* e, mimi_engine::Lane& lane, hipStream_t s, const float* audio, int B, int64_t L,
                    int K, int32_t* codes, bool* overflow) {
    *overflow = false;
    int rc = encode_pass(e, PassCtx{lane, s, PREC_F16X3}, audio, B, L, K, codes);
    if (rc) return rc;
    int n = 0;
    if ((rc = read_amax(e, lane, s, &n))) return rc;
    *overflow = f16_overflow(e->amax_host, n, e->act_scale, B);
    return MIMI_OK;
}

static int calibrate_scales(mimi_engine* e) {
    const int B = 3;
    const int64_t L = 240000;
    std::vector<float> h((size_t)B * L);
    uint64_t st = 0x243F6A8885A308D3ull;  // splitmix64
    auto uni = [&]() {
        uint64_t z = (st += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    };
    const double fs = 24000.0, pi = 3.14159265358979323846;
    float pk = 0.0f;
    for (int64_t i = 0; i < L; ++i) {
        const double t = i / fs;
        h[i] = (float)(2.0 * uni() - 1.0);  // white noise, U[-1, 1]
        // harmonic mix of a gliding 90..250 Hz fundamental under a 4 Hz syllable envelope
        const double f0 = 170.0 + 80.0 * std::sin(2 * pi * 0.3 * t);
        double v = 0.0;
        for (int k = 1; k <= 12; ++k) v += std::sin(2 * pi * f0 * k * t + 0.7 * k) / k;
        v *= 0.55 + 0.45 * std::sin(2 * pi * 4.0 * t);
        h[L + i] = (float)v;
        pk = std::max(pk, std::fabs(h[L + i]));
        // logarithmic sine sweep 50 Hz -> 11 kHz over the clip, amplitude 1
        const double T = L / fs, k = std::log(11000.0 / 50.0);
        h[2 * L + i] = (float)std::sin(2 * pi * 50.0 * T / k * (std::exp(t / T * k) - 1.0));
    }
    for (int64_t i = 0; i < L; ++i) h[L + i] /= pk;
    const int K = e->cfg.num_semantic_quantizers;
    const int64_t T2 = plan_lengths(e->cfg, L).frames12;
    float* d_audio = nullptr;
    int32_t* d_codes = nullptr;
    hipStream_t s = nullptr;
    int rc = MIMI_OK;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (hipMalloc(&d_audio, h.size() * 4) != hipSuccess || hipMalloc(&d_codes, (size_t)B * K * T2 * 4) != hipSuccess) {
        rc = set_err(MIMI_ERR_OUT_OF_MEMORY, "calibration buffers");
    } else if (hipMemcpy(d_audio, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        rc = set_err(MIMI_ERR_HIP, "calibration upload");
    }
    PassCtx ctx{e->lanes[0], s, PREC_F16X3};
    ctx.calibrating = true;
    for (int it = 0; rc == MIMI_OK && it < 8; ++it) {
        int n = 0;
        if ((rc = encode_pass(e, ctx, d_audio, B, L, K, d_codes)) || (rc = read_amax(e, ctx.lane, s, &n))) break;
        bool changed = false;
        for (int i = 0; i < n; ++i) {
            const float a = amax_word(e->amax_host, i);
            if (!(a > 0.0f) || !std::isfinite(a)) continue;
            const float as = a * e->act_scale[i];
            if (as < 64.0f || as >= 512.0f) {  // hysteresis band around the [2^7, 2^8) target
                e->act_scale[i] = std::ldexp(1.0f, 7 - std::ilogb(a));
                changed = true;
            }
        }
        if (!changed) break;
    }
    if (rc == MIMI_OK) e->calibrated = true;
    (void)hipStreamSynchronize(s);
    if (d_audio) (void)hipFree(d_audio);
    if (d_codes) (void)hipFree(d_codes);
    (void)hipStreamDestroy(s);
    return rc;
}

// e->item_codes with room for one item's `per` codes (synchronises s before it grows)
static int ensure_item_codes(mimi_engine* e, size_t per, hipStream_t s) {
    if (e->item_codes_cap >= per) return MIMI_OK;
    HIP_TRY(hipStreamSynchronize(s));
    if (e->item_codes) HIP_TRY(hipFree(e->item_codes));
    e->item_codes = nullptr;
    e->item_codes_cap = 0;
    HIP_TRY(hipMalloc(&e->item_codes, per * sizeof(int32_t)));
    e->item_codes_cap = per;
    return MIMI_OK;
}

// One item alone at length L into e->item_codes: the f16x3 pass, then bf16x6 if the item overflows alone (*ovf).
static int encode_item(mimi_engine* e, mimi_engine::Lane& lane, hipStream_t s, const float* audio, int64_t L, int K,
                       bool* ovf) {
    const int rc = f16_pass(e, lane, s, audio, 1, L, K, e->item_codes, ovf);
    if (rc || !*ovf) return rc;
    return encode_pass(e, PassCtx{lane, s, PREC_BF16X6}, audio, 1, L, K, e->item_codes);
}

// Per-item overflow fallback of one f16x3 encode (see "activation scales"): every item re-encoded alone at the
// same padded length, in bf16x6 where it overflows alone.  Synchronises s.
static int overflow_fallback(mimi_engine* e, mimi_engine::Lane& lane, hipStream_t s, const float* audio, int B,
                             int64_t L, int K, int32_t* codes) {
    ++e->f16_reruns;  // (once per encode, however many of its items overflow alone)
    int rc;
    if (B == 1) {  // the item was alone already
        if ((rc = encode_pass(e, PassCtx{lane, s, PREC_BF16X6}, audio, 1, L, K, codes))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        return MIMI_OK;
    }
    const size_t per = (size_t)K * plan_lengths(e->cfg, L).frames12;
    if ((rc = ensure_item_codes(e, per, s))) return rc;
    bool ovf = false;
    for (int b = 0; b < B; ++b) {
        if ((rc = encode_item(e, lane, s, audio + (int64_t)b * L, L, K, &ovf))) return rc;
        HIP_TRY(hipMemcpyAsync(codes + b * per, e->item_codes, per * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return MIMI_OK;
}

// Ragged batch, item by item (each alone at its own length: the definition of the ragged result): the f16x3
// overflow fallback of a ragged encode, and the whole ragged encode where the batched form does not apply
// (precision modes other than f16x3, clips too long for the plane buffers).  Item b's codes go to
// codes[b][k][0 .. F_b) of the [B][K][Fmax] output.  Synchronises s.
static int ragged_item_by_item(mimi_engine* e, mimi_engine::Lane& lane, hipStream_t s, const float* audio, int B,
                               int64_t L, const int64_t* lens, int K, int32_t* codes, int prec) {
    const int64_t Fmax = plan_lengths(e->cfg, L).frames12;
    int rc = ensure_item_codes(e, (size_t)K * Fmax, s);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        const float* ab = audio + (int64_t)b * L;
        const int64_t Fb = plan_lengths(e->cfg, lens[b]).frames12;
        if (prec == PREC_F16X3 && act_planes(e, plan_lengths(e->cfg, lens[b]), prec) == 2) {
            bool ovf = false;
            rc = encode_item(e, lane, s, ab, lens[b], K, &ovf);
            if (ovf) ++e->f16_reruns;  // (once per item that overflows alone)
            if (rc) return rc;
        } else if ((rc = encode_pass(e, PassCtx{lane, s, prec}, ab, 1, lens[b], K, e->item_codes))) {
            return rc;
        }
        HIP_TRY(hipMemcpy2DAsync(codes + (int64_t)b * K * Fmax, Fmax * sizeof(int32_t), e->item_codes,
                                 Fb * sizeof(int32_t), Fb * sizeof(int32_t), K, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return MIMI_OK;
}

// ---- hipGraph replay (f16x3).  A small batch is launch-bound: ~80 kernels per encode, each a few
// microseconds of GPU time.  The second encode of a (batch, length, K) shape captures the whole pass -- the
// maxima reset, every kernel, the maxima fold -- into a graph on a private stream; later encodes of that shape
// replay it on the caller's stream behind one set_io_kernel that writes this call's audio / codes pointers
// into io_dev (the stage-0 block and the RVQ kernels read them from there; every other operand lives in the
// engine: weights, workspace, rope tables).  A graph is dropped when the workspace or the rope tables it
// addresses are reallocated.  The replay is the same kernels with the same arguments: bit-identical codes.
static void destroy_graph(mimi_engine::Graph& g) {
    if (g.x) (void)hipGraphExecDestroy(g.x);
    if (g.g) (void)hipGraphDestroy(g.g);
    g.x = nullptr;
    g.g = nullptr;
}

// Every lane's graphs, once nothing replays them any more.  clear_seen: the shapes' eager counts too.
static void drop_graphs(mimi_engine* e, bool clear_seen = false) {
    drain_lanes(e);
    for (auto& l : e->lanes) {
        for (auto& g : l.graphs) destroy_graph(g);
        l.graphs.clear();
        if (clear_seen) l.graph_seen.clear();
    }
}

// Captures the f16x3 pass of (B, L, K) into a new graph.  On any failure the capture is abandoned and the
// caller runs the eager pass (the error is cleared: a graph is an optimisation, never a requirement).
static mimi_engine::Graph* capture_graph(mimi_engine* e, mimi_engine::Lane& lane, const float* audio, int B,
                                          int64_t L, int K, int32_t* codes) {
    if (!lane.io_dev && hipMalloc(&lane.io_dev, 4 * sizeof(void*)) != hipSuccess) {
        (void)hipGetLastError();
        lane.io_dev = nullptr;
        return nullptr;
    }
    if (!e->cap_stream && hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        e->cap_stream = nullptr;
        return nullptr;
    }
    hipStream_t cs = e->cap_stream;
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    PassCtx ctx{lane, cs, PREC_F16X3};
    ctx.capturing = true;
    ctx.chain_ok = true;  // (the submitter reads the flag back through the ticket, as after an eager pass)
    PassOut out;
    // (no maxima reset node: amax_reduce_kernel leaves every sub-slot at 0 as it reads it, so a replay starts
    // from the zeros the previous encode's fold left behind)
    int rc = encode_pass(e, ctx, audio, B, L, K, codes, &out);
    // (+ the ticket's host words from inside the graph: destinations through io_dev, set before each replay)
    if (!rc && launch_amax_reduce(lane.amax_dev, (int)e->slot_of.size(), lane.amax_red, cs, nullptr, out.chain_flag,
                                  nullptr, lane.io_dev) != hipSuccess)
        rc = MIMI_ERR_HIP;
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(cs, &g);
    hipGraphExec_t x = nullptr;
    if (rc || ec != hipSuccess || !g || out.uncalibrated || hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        return nullptr;
    }
    if ((int)lane.graphs.size() >= mimi_engine::kMaxGraphs) {  // evict the least recently used
        size_t lru = 0;
        for (size_t i = 1; i < lane.graphs.size(); ++i)
            if (lane.graphs[i].used < lane.graphs[lru].used) lru = i;
        destroy_graph(lane.graphs[lru]);
        lane.graphs.erase(lane.graphs.begin() + (long)lru);
    }
    mimi_engine::Graph ng;
    ng.B = B;
    ng.L = L;
    ng.K = K;
    ng.ws_gen = lane.ws_gen;
    ng.rope_gen = e->rope_gen;
    ng.g = g;
    ng.x = x;
    ng.chain_flag = out.chain_flag;
    ng.chain_clear = out.chain_clear;
    lane.graphs.push_back(ng);
    ++e->graph_captures;
    return &lane.graphs.back();
}

// Runs the f16x3 pass of (B, L, K) as a graph replay on s when it can (*replayed: the graph); otherwise leaves
// everything to the eager path.
static int graph_encode(mimi_engine* e, mimi_engine::Lane& lane, const float* audio, int B, int64_t L, int K,
                        int32_t* codes, hipStream_t s, mimi_engine::Graph** replayed, unsigned* host_amax,
                        unsigned* host_flag) {
    *replayed = nullptr;
    if (!e->graphs_enabled || e->profiling || e->taps) return MIMI_OK;
    // sizes first: nothing may be allocated inside a capture, and a reallocation retires the graphs
    const StagePlan p = plan_lengths(e->cfg, L);
    int rc = ensure_ws(lane, ws_layout(e, B, p, PREC_F16X3), s);
    if (rc) return rc;
    if ((rc = ensure_rope(e, p.frames25))) return rc;
    mimi_engine::Graph* gr = nullptr;
    for (auto it = lane.graphs.begin(); it != lane.graphs.end();) {
        if (it->ws_gen != lane.ws_gen || it->rope_gen != e->rope_gen) {
            destroy_graph(*it);
            it = lane.graphs.erase(it);
            continue;
        }
        if (it->B == B && it->L == L && it->K == K) gr = &*it;
        ++it;
    }
    if (!gr) {
        const auto key = std::make_tuple(B, L, K);
        if (lane.graph_seen.size() > 256) lane.graph_seen.clear();
        if (++lane.graph_seen[key] < 2) return MIMI_OK;  // a shape seen once runs eagerly
        gr = capture_graph(e, lane, audio, B, L, K, codes);
        if (!gr) {
            e->graphs_enabled = false;  // capture unsupported here: stay eager from now on
            return MIMI_OK;
        }
    }
    gr->used = ++e->graph_clock;
    HIP_TRY(hipStreamWaitEvent(s, lane.ws_free, 0));
    LAUNCH_TRY(launch_set_io(lane.io_dev, audio, codes, s, host_amax, host_flag, gr->chain_flag, gr->chain_clear),
               "set_io");
    HIP_TRY(hipGraphLaunch(gr->x, s));
    ++e->graph_replays;
    *replayed = gr;
    return MIMI_OK;
}

// ---- lanes.  An encode is ~80 dependent launches; behind every one-tile-per-CU kernel all CUs fill their rings
// together and later run their epilogues together, and nothing else is resident.  Callers that keep two encodes
// enqueued (mimi_encode_async, waited one behind) get the second one's kernels into those phases: an encode that
// takes a lane runs on the lane's own stream, ordered after the caller's stream at the call, in the lane's own
// workspace; mimi_encode_wait synchronises the host on it.  Nothing is enqueued on the caller's stream behind it
// (that would order the next encode's inputs behind this encode and serialise the lanes again).

// Makes lane li usable on its own stream (first use: lane 1's buffers and event, the lane's stream).  false: it cannot
// be (the error is cleared) -- the encode then runs where it would have without lanes.
static bool lane_prepare(mimi_engine* e, int li) {
    mimi_engine::Lane& l = e->lanes[li];
    bool ok = true;
    if (!l.stream) ok = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) == hipSuccess;
    if (ok && !l.in_ready) ok = hipEventCreateWithFlags(&l.in_ready, hipEventDisableTiming) == hipSuccess;
    if (ok && !l.ws_free) ok = hipEventCreateWithFlags(&l.ws_free, hipEventDisableTiming) == hipSuccess;
    if (ok && !l.amax_dev) {
        const size_t bytes = ((size_t)kMaxActSlots * AMAX_SLOT_WORDS + kMaxActSlots) * sizeof(unsigned);
        ok = hipMalloc(&l.amax_dev, bytes) == hipSuccess;
        if (ok) {
            l.amax_red = l.amax_dev + (size_t)kMaxActSlots * AMAX_SLOT_WORDS;
            // (on the lane's stream: everything that touches these words runs there, behind this)
            ok = hipMemsetAsync(l.amax_dev, 0, bytes, l.stream) == hipSuccess;
        } else {
            l.amax_dev = nullptr;
        }
    }
    if (!ok) (void)hipGetLastError();
    return ok;
}

// The lane of a new encode that may take one: the lowest-numbered lane with no un-waited ticket, else the one with
// fewer tickets.  A caller that never overlaps encodes therefore stays in lane 0: one workspace, one graph per shape.
static int choose_lane(const mimi_engine* e) {
    for (int i = 0; i < mimi_engine::kLanes; ++i)
        if (e->lanes[i].tickets == 0) return i;
    int best = 0;
    for (int i = 1; i < mimi_engine::kLanes; ++i)
        if (e->lanes[i].tickets < e->lanes[best].tickets) best = i;
    return best;
}

// A free ticket slot, with its event and pinned words (made on the slot's first use).
static int claim_ticket(mimi_engine* e, mimi_engine::Pending** slot) {
    mimi_engine::Pending* P = nullptr;
    for (auto& q : e->pend)
        if (q.id == 0) {
            P = &q;
            break;
        }
    if (!P)
        return set_err(MIMI_ERR_STATE, "%d encodes in flight: call mimi_encode_wait first", mimi_engine::kMaxPending);
    if (!P->done) HIP_TRY(hipEventCreateWithFlags(&P->done, hipEventDisableTiming));
    if (!P->amax) HIP_TRY(hipHostMalloc(&P->amax, kMaxActSlots * sizeof(unsigned), hipHostMallocDefault));
    if (!P->chain_word) HIP_TRY(hipHostMalloc(&P->chain_word, 16, hipHostMallocDefault));
    // the slot's last ticket was waited, so nothing in flight writes this word: clear it here rather than trust that
    // a kernel of this encode writes it (amax_reduce skips its launch when there is nothing to reduce)
    P->chain_word[0] = 0u;
    P->chain = false;
    *slot = P;
    return MIMI_OK;
}

// Makes P the ticket of the encode just enqueued on s in lane li (lengths: a ragged batch's, kept for the fallbacks
// at the wait).
static int issue_ticket(mimi_engine* e, mimi_engine::Pending* P, int li, bool excl, hipStream_t s, const float* audio,
                        int B, int64_t L, int K, int32_t* codes, int nslots, bool h16, const int64_t* lengths,
                        int64_t* ticket) {
    HIP_TRY(hipEventRecord(P->done, s));
    mimi_engine::Lane& lane = e->lanes[li];
    P->lane = li;
    ++lane.tickets;
    ++lane.encodes;
    lane.excl = excl;
    P->nslots = nslots;
    P->h16 = h16;
    P->audio = audio;
    P->B = B;
    P->L = L;
    P->K = K;
    P->codes = codes;
    P->s = s;
    P->ragged = lengths != nullptr;
    if (lengths) P->lens.assign(lengths, lengths + B);
    P->claimed = false;
    P->id = e->next_ticket++;
    *ticket = P->id;
    return MIMI_OK;
}

// The length table of a ragged batch, and its device image into the ticket's pinned buffer.
static int fill_ragged(const mimi_config& c, const int64_t* lengths, int B, RaggedTable* rt, mimi_engine::Pending* P) {
    rt->B = B;
    rt->len.assign(lengths, lengths + B);
    rt->plan.resize(B);
    for (int b = 0; b < B; ++b) rt->plan[b] = plan_lengths(c, lengths[b]);
    rt->minT25 = rt->maxT25 = (int)rt->plan[0].frames25;
    for (const auto& pb : rt->plan) {
        rt->minT25 = std::min<int>(rt->minT25, (int)pb.frames25);
        rt->maxT25 = std::max<int>(rt->maxT25, (int)pb.frames25);
        rt->R += pb.frames25;
    }
    const size_t need = RaggedTable::ints(B) * sizeof(int);
    if (P->rg_cap < need) {
        if (P->rg_pinned) HIP_TRY(hipHostFree(P->rg_pinned));
        P->rg_pinned = nullptr;
        P->rg_cap = 0;
        HIP_TRY(hipHostMalloc(&P->rg_pinned, need, hipHostMallocDefault));
        P->rg_cap = need;
    }
    rt->fill(P->rg_pinned);
    return MIMI_OK;
}

// Enqueues one encode and returns its ticket without waiting: on its lane's stream behind the caller's stream s when
// it takes a lane (may_lane and the "lanes" rule), else on s in lane 0.  In f16x3 the per-tensor maxima are folded
// and copied to this ticket's pinned slot behind the encode; mimi_encode_wait checks them.
static int encode_async_locked(mimi_engine* e, const float* audio, int B, int64_t L, int K, int32_t* codes,
                               hipStream_t s, int64_t* ticket, const int64_t* lengths = nullptr,
                               bool may_lane = false) {
    mimi_engine::Pending* P = nullptr;
    int rc = claim_ticket(e, &P);
    if (rc) return rc;
    const int prec = e->precision;
    const bool h16 = prec == PREC_F16X3 && act_planes(e, plan_lengths(e->cfg, L), prec) == 2;
    int n = 0;
    // Calibrate whenever f16x3 is on, not only when this batch's longest item gets planes: a ragged batch whose
    // longest item is past the plane limit runs its short items through the planes path item by item.
    if (prec == PREC_F16X3 && !e->calibrated && (rc = calibrate_scales(e))) return rc;
    RaggedTable rt;
    if (lengths) {
        const mimi_config& c = e->cfg;
        const bool batched = h16 && e->res0_h16 && e->res1_h16 && e->ds_fix && e->inproj_h &&
                             c.downsample_kernel == 4 && c.downsample_stride == 2 && c.num_ratios >= 2;
        if (!batched) {  // item by item, synchronously (the ticket's event is then already complete)
            if ((rc = ragged_item_by_item(e, e->lanes[0], s, audio, B, L, lengths, K, codes, prec))) return rc;
            return issue_ticket(e, P, 0, false, s, audio, B, L, K, codes, 0, false, nullptr, ticket);
        }
        if ((rc = fill_ragged(c, lengths, B, &rt, P))) return rc;
    }
    // ---- the lane.  By default only what gains: f16x3 uniform batches on the per-level RVQ kernels (large grids).
    // The persistent RVQ chain's slice workgroups spin on their peers and need the whole grid resident; another lane's
    // LDS-heavy kernels on the same CUs would push it into give-ups and re-runs, so an encode that may launch it stays on
    // the caller's stream in lane 0 and runs with the other lane idle.  Taps, per-stage profiling and every caller that
    // goes on using s behind the call (may_lane false) stay there too.
    const int64_t rvq_frames = (int64_t)B * plan_lengths(e->cfg, L).frames12;
    const bool chain_el = h16 && e->rvq_chain != 0 && (rvq_frames + 31) / 32 * 8 < 256;  // (launch_rvq's small grids)
    bool laned = may_lane && e->lanes_opt > 0 && h16 && !e->taps && e->profiling != 1 &&
                 (e->lanes_opt == 2 || (!lengths && !chain_el));
    int li = laned ? choose_lane(e) : 0;
    if (laned && !lane_prepare(e, li)) {  // (without a stream for lane 0 either: on the caller's)
        if (li == 0 || !lane_prepare(e, 0)) laned = false;
        li = 0;
    }
    if (laned && li != 0) {  // lane 1's workspace, on its first use and when it grows: never at the encode's cost
        const size_t need = ws_layout(e, B, plan_lengths(e->cfg, L), PREC_F16X3, lengths != nullptr);
        if (ensure_ws(e->lanes[li], need, e->lanes[li].stream) != MIMI_OK) {
            (void)hipGetLastError();
            li = 0;
            if (!lane_prepare(e, 0)) laned = false;
        }
    }
    mimi_engine::Lane& lane = e->lanes[li];
    if (laned) {  // the whole encode on the lane's stream, behind everything enqueued on the caller's so far
        HIP_TRY(hipEventRecord(lane.in_ready, s));
        s = lane.stream;
        HIP_TRY(hipStreamWaitEvent(s, lane.in_ready, 0));
    }
    // an encode that may hold the chain wants the GPU to itself: it waits for the other lane, and the other lane's next
    // encode waits for it
    const bool excl = chain_el && !laned && e->lanes_opt > 0;
    for (auto& o : e->lanes)
        if (&o != &lane && o.ws_free && (excl || o.excl)) HIP_TRY(hipStreamWaitEvent(s, o.ws_free, 0));
    if (h16) {
        mimi_engine::Graph* replayed = nullptr;
        if (!lengths && (rc = graph_encode(e, lane, audio, B, L, K, codes, s, &replayed, P->amax, P->chain_word)))
            return rc;
        unsigned* cflag = replayed ? replayed->chain_flag : nullptr;
        n = (int)e->slot_of.size();
        if (!replayed) {
            PassCtx ctx{lane, s, PREC_F16X3, lengths ? &rt : nullptr, P->rg_pinned};
            ctx.chain_ok = true;  // the chain is allowed inside this pass only (its flag is read back through the ticket)
            PassOut out;
            if ((rc = encode_pass(e, ctx, audio, B, L, K, codes, &out))) return rc;
            cflag = out.chain_flag;
            // the maxima and (chain) the give-up flag also into the ticket's pinned words, before ws_free (the next
            // encode's memset node zeroes the flag); a replay's graph ends with the same kernel (capture_graph)
            LAUNCH_TRY(launch_amax_reduce(lane.amax_dev, n, lane.amax_red, s, P->amax, cflag, cflag ? P->chain_word : nullptr),
                       "amax_reduce");
        }
        P->chain = cflag != nullptr;
        HIP_TRY(hipEventRecord(lane.ws_free, s));
    } else if ((rc = encode_pass(e, PassCtx{lane, s, prec}, audio, B, L, K, codes))) {
        return rc;
    }
    return issue_ticket(e, P, li, excl, s, audio, B, L, K, codes, n, h16, lengths, ticket);
}

// Waits for ticket's encode and runs its f16x3 overflow check.  The engine lock is NOT held while the host
// synchronises on the encode's event (other threads keep enqueueing on the engine meanwhile): the slot is claimed
// under the lock -- so it is neither reused nor waited twice -- and released, with the overflow check and any
// fallback, under the lock again.
static int encode_wait(mimi_engine* e, int64_t ticket) {
    mimi_engine::Pending q;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        mimi_engine::Pending* P = nullptr;
        for (auto& x : e->pend)
            if (ticket > 0 && x.id == ticket && !x.claimed) P = &x;
        if (!P) return set_err(MIMI_ERR_INVALID_ARGUMENT, "ticket %lld is not an encode in flight", (long long)ticket);
        P->claimed = true;
        q = *P;
    }
    HIP_TRY(hipSetDevice(e->device));
    const hipError_t se = hipEventSynchronize(q.done);
    std::lock_guard<std::mutex> lk(e->mu);
    mimi_engine::Pending* P = nullptr;
    for (auto& x : e->pend)
        if (x.id == ticket) P = &x;
    bool ovf = false;
    const bool chain_gave_up = q.chain && se == hipSuccess && P->chain_word[0] != 0u;
    if (q.h16 && se == hipSuccess) {
        e->last_amax.resize(q.nslots);
        for (int i = 0; i < q.nslots; ++i) e->last_amax[i] = amax_word(P->amax, i);
        ovf = f16_overflow(P->amax, q.nslots, e->act_scale, q.B);
    }
    P->claimed = false;
    P->id = 0;
    mimi_engine::Lane& lane = e->lanes[q.lane];  // the re-runs below: on the encode's stream, in its lane's workspace
    --lane.tickets;
    if (se != hipSuccess)
        return set_err(se == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP, "hipEventSynchronize: %s",
                       hipGetErrorString(se));
    if (!chain_gave_up && !ovf) return MIMI_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (chain_gave_up) ++e->chain_reruns;  // the persistent RVQ gave up (its codes are not kept)
    if (q.ragged) {  // each item alone at its own length (the ragged result's definition), bf16x6 if it overflows
        if (!chain_gave_up) ++e->f16_reruns;
        return ragged_item_by_item(e, lane, q.s, q.audio, q.B, q.L, q.lens.data(), q.K, q.codes, PREC_F16X3);
    }
    if (chain_gave_up) {  // the whole encode again, without the chain
        const int rc = f16_pass(e, lane, q.s, q.audio, q.B, q.L, q.K, q.codes, &ovf);
        if (rc || !ovf) return rc;
    }
    return overflow_fallback(e, lane, q.s, q.audio, q.B, q.L, q.K, q.codes);
}

static int check_encode_args(mimi_engine* e, const float* audio, int32_t batch, int64_t length, int32_t* K,
                             int32_t* codes) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    if (!e->finalized) return set_err(MIMI_ERR_STATE, "mimi_finalize has not been called");
    if (*K <= 0) *K = e->cfg.num_quantizers;
    if (*K > e->cfg.num_quantizers)
        return set_err(MIMI_ERR_INVALID_ARGUMENT,
                       "The number of quantizers (i.e codebooks) asked should be lower than the total number of "
                       "quantizers %d, but is currently %d.",
                       e->cfg.num_quantizers, *K);
    if (*K < e->cfg.num_semantic_quantizers)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "num_quantizers %d below the semantic quantizers %d", *K,
                       e->cfg.num_semantic_quantizers);
    if (*K > e->levels_available)
        return set_err(MIMI_ERR_WEIGHTS, "num_quantizers %d but the checkpoint has %d codebooks", *K, e->levels_available);
    if (batch <= 0 || length <= 0 || !audio || !codes)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "batch=%d length=%lld", batch, (long long)length);
    if (length > (int64_t)1 << 31) return set_err(MIMI_ERR_INVALID_ARGUMENT, "length %lld too large", (long long)length);
    return MIMI_OK;
}

extern "C" int mimi_encode_async(mimi_engine* e, const float* audio, int32_t batch, int64_t length, int32_t K,
                                 int32_t* codes, void* stream, int64_t* ticket) {
    int rc = check_encode_args(e, audio, batch, length, &K, codes);
    if (rc) return rc;
    if (!ticket) return set_err(MIMI_ERR_INVALID_ARGUMENT, "ticket is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    (void)hipGetLastError();  // a failure left by an unrelated earlier call must not fail this encode's launches
    return encode_async_locked(e, audio, batch, length, K, codes, reinterpret_cast<hipStream_t>(stream), ticket,
                               nullptr, true);
}

static int check_ragged(mimi_engine* e, const int64_t* lengths, int32_t batch, int64_t max_length) {
    if (!lengths) return set_err(MIMI_ERR_INVALID_ARGUMENT, "lengths is NULL");
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 1 || lengths[b] > max_length)
            return set_err(MIMI_ERR_INVALID_ARGUMENT, "lengths[%d] = %lld outside [1, %lld]", b, (long long)lengths[b],
                           (long long)max_length);
    (void)e;
    return MIMI_OK;
}

extern "C" int mimi_encode_ragged_async(mimi_engine* e, const float* audio, const int64_t* lengths, int32_t batch,
                                        int64_t max_length, int32_t K, int32_t* codes, void* stream, int64_t* ticket) {
    int rc = check_encode_args(e, audio, batch, max_length, &K, codes);
    if (rc || (rc = check_ragged(e, lengths, batch, max_length))) return rc;
    if (!ticket) return set_err(MIMI_ERR_INVALID_ARGUMENT, "ticket is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    (void)hipGetLastError();
    return encode_async_locked(e, audio, batch, max_length, K, codes, reinterpret_cast<hipStream_t>(stream), ticket,
                               lengths, true);
}

extern "C" int mimi_encode_ragged(mimi_engine* e, const float* audio, const int64_t* lengths, int32_t batch,
                                  int64_t max_length, int32_t K, int32_t* codes, void* stream) {
    int64_t ticket = 0;
    const int rc = mimi_encode_ragged_async(e, audio, lengths, batch, max_length, K, codes, stream, &ticket);
    if (rc) return rc;
    return encode_wait(e, ticket);
}

extern "C" int mimi_encode_wait(mimi_engine* e, int64_t ticket) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    return encode_wait(e, ticket);
}

extern "C" int mimi_encode(mimi_engine* e, const float* audio, int32_t batch, int64_t length, int32_t K,
                           int32_t* codes, void* stream) {
    int rc = check_encode_args(e, audio, batch, length, &K, codes);
    if (rc) return rc;
    int64_t ticket = 0;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        HIP_TRY(hipSetDevice(e->device));
        (void)hipGetLastError();  // a failure left by an unrelated earlier call must not fail this encode's launches
        // NULL stream = the HIP null stream, as in every HIP API
        // (a lane's stream only beside another encode in flight, another thread's: alone, this call runs on the
        // caller's stream as it always did -- it is waited right here, so there is nothing to overlap it with)
        bool others = false;
        for (const auto& l : e->lanes) others = others || l.tickets > 0;
        if ((rc = encode_async_locked(e, audio, batch, length, K, codes, reinterpret_cast<hipStream_t>(stream),
                                      &ticket, nullptr, others)))
            return rc;
    }
    return encode_wait(e, ticket);
}

// Host audio in, host codes out (the per-utterance callers' path: MimiEncoder.encode_audio_chunk once per utterance,
// `librispeech-mimi/process_librispeech_dev-test.py:136-141`, `mls-en-mimi-pretrain/process_shard.py:302-307`).  The
// same encode as mimi_encode on a device copy of the audio, with no framework tensors around it: the H2D copy, the
// encode and the codes' D2H into pinned memory are enqueued on `stream` in one call and the host synchronises once
// (twice when the encode had to be re-run: a chain give-up or an f16x3 overflow re-encodes on the stream inside
// mimi_encode_wait, after which the codes are copied again).
static int host_io_grow(mimi_engine::HostIo* io, size_t ab, size_t cb) {
    if (!io->done) HIP_TRY(hipEventCreateWithFlags(&io->done, hipEventDisableTiming));
    if (io->audio_cap < ab) {
        if (io->d_audio) HIP_TRY(hipFree(io->d_audio));  // (hipFree waits for the device)
        if (io->h_audio) HIP_TRY(hipHostFree(io->h_audio));
        io->d_audio = nullptr;
        io->h_audio = nullptr;
        io->audio_cap = 0;
        const size_t cap = std::max(ab, (size_t)1 << 22);
        HIP_TRY(hipMalloc(&io->d_audio, cap));
        HIP_TRY(hipHostMalloc(&io->h_audio, cap, hipHostMallocDefault));
        io->audio_cap = cap;
    }
    if (io->codes_cap < cb) {
        if (io->d_codes) HIP_TRY(hipFree(io->d_codes));
        if (io->h_codes) HIP_TRY(hipHostFree(io->h_codes));
        io->d_codes = nullptr;
        io->h_codes = nullptr;
        io->codes_cap = 0;
        const size_t cap = std::max(cb, (size_t)1 << 16);
        HIP_TRY(hipMalloc(&io->d_codes, cap));
        HIP_TRY(hipHostMalloc(&io->h_codes, cap, hipHostMallocDefault));
        io->codes_cap = cap;
    }
    return MIMI_OK;
}

extern "C" int mimi_encode_host(mimi_engine* e, const float* host_audio, int32_t batch, int64_t length, int32_t K,
                                int32_t* host_codes, void* stream) {
    int rc = check_encode_args(e, host_audio, batch, length, &K, host_codes);
    if (rc) return rc;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t ab = (size_t)batch * (size_t)length * sizeof(float);
    const size_t cb = (size_t)batch * K * (size_t)mimi_encoded_length_cfg(&e->cfg, length) * sizeof(int32_t);
    mimi_engine::HostIo* io = nullptr;
    int64_t ticket = 0, reruns = 0;
    {  // claim a staging slot and size it under the engine lock (a re-allocation's hipFree must not land inside
       // another thread's graph capture on this engine) ...
        std::lock_guard<std::mutex> lk(e->mu);
        HIP_TRY(hipSetDevice(e->device));
        for (auto& h : e->hostio)
            if (!h.busy) {
                io = &h;
                break;
            }
        if (!io)
            return set_err(MIMI_ERR_STATE, "%d host encodes in flight", mimi_engine::kMaxPending);
        if ((rc = host_io_grow(io, ab, cb))) return rc;
        io->busy = true;  // (from here on every exit path releases it)
    }
    // ... then copy the caller's samples into its pinned buffer without the lock: other threads' encodes on this
    // engine are not held up behind a host memcpy of up to several MB (the slot's previous H2D finished before its
    // last call returned)
    if (const hipError_t de = hipSetDevice(e->device); de != hipSuccess) {
        std::lock_guard<std::mutex> lk(e->mu);
        io->busy = false;
        return set_err(MIMI_ERR_HIP, "mimi_encode_host: hipSetDevice: %s", hipGetErrorString(de));
    }
    std::memcpy(io->h_audio, host_audio, ab);
    {
        std::lock_guard<std::mutex> lk(e->mu);
        (void)hipGetLastError();
        const hipError_t ce = hipMemcpyAsync(io->d_audio, io->h_audio, ab, hipMemcpyHostToDevice, s);
        if (ce != hipSuccess) rc = set_err(MIMI_ERR_HIP, "mimi_encode_host: H2D copy: %s", hipGetErrorString(ce));
        if (!rc) rc = encode_async_locked(e, io->d_audio, batch, length, K, io->d_codes, s, &ticket);
        if (rc) {
            (void)hipStreamSynchronize(s);  // (the slot is released: nothing of this call is left in flight)
            io->busy = false;
            return rc;
        }
        reruns = e->chain_reruns + e->f16_reruns;
        hipError_t de = hipMemcpyAsync(io->h_codes, io->d_codes, cb, hipMemcpyDeviceToHost, s);
        if (de == hipSuccess) de = hipEventRecord(io->done, s);
        if (de != hipSuccess) rc = set_err(MIMI_ERR_HIP, "mimi_encode_host: D2H copy: %s", hipGetErrorString(de));
    }
    const int wrc = encode_wait(e, ticket);  // (always: it frees the ticket)
    if (!rc) rc = wrc;
    if (!rc) {
        bool again;
        {
            std::lock_guard<std::mutex> lk(e->mu);
            again = e->chain_reruns + e->f16_reruns != reruns;  // (another thread's re-run only costs a copy)
        }
        hipError_t he = hipSuccess;
        if (again) he = hipMemcpyAsync(io->h_codes, io->d_codes, cb, hipMemcpyDeviceToHost, s);
        if (again && he == hipSuccess) he = hipEventRecord(io->done, s);
        if (he == hipSuccess) he = hipEventSynchronize(io->done);
        if (he != hipSuccess)
            rc = set_err(he == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP, "mimi_encode_host: %s",
                         hipGetErrorString(he));
        else
            std::memcpy(host_codes, io->h_codes, cb);
    } else {
        (void)hipStreamSynchronize(s);  // the buffers are reused: nothing of this call may still be in flight
    }
    std::lock_guard<std::mutex> lk(e->mu);
    io->busy = false;
    return rc;
}

extern "C" int mimi_rvq_encode(mimi_engine* e, const float* emb, int64_t frames, int32_t K, int32_t* codes,
                               void* stream) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    if (!e->finalized) return set_err(MIMI_ERR_STATE, "mimi_finalize has not been called");
    if (K <= 0) K = e->cfg.num_quantizers;
    if (K > e->levels_available || K < e->cfg.num_semantic_quantizers)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "num_quantizers %d out of range", K);
    if (frames <= 0 || !emb || !codes) return set_err(MIMI_ERR_INVALID_ARGUMENT, "frames=%lld", (long long)frames);
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);  // NULL = the HIP null stream, as in every HIP API
    const int Hd = e->cfg.hidden_size, Dq = e->cfg.vq_hidden_dim;
    const size_t projb = ((size_t)frames * 2 * Dq * sizeof(float) + 255) / 256 * 256;
    const size_t need = projb + rvq_work_bytes(frames);
    mimi_engine::Lane& lane = e->lanes[0];  // it borrows lane 0's workspace, ordered by ws_free like an encode there
    int rc = ensure_ws(lane, std::max(need, lane.ws_bytes), s);
    if (rc) return rc;
    float* proj = reinterpret_cast<float*>(lane.ws);
    void* work = reinterpret_cast<char*>(lane.ws) + projb;
    HIP_TRY(hipStreamWaitEvent(s, lane.ws_free, 0));
    Recorder rec{e, s};
    rec.begin();
    GemmArgs ap = linear_args(emb, frames, Hd, e->inproj, 2 * Dq, proj);
    const char* kname = "?";
    LAUNCH_TRY(launch_gemm(ROLE_INPROJ, ap, s, &kname), "input_proj");
    rec.mark("input_proj", 2.0 * frames * Hd * 2 * Dq, 0, kname);
    if ((rc = save_tap(e, "proj", proj, 1, frames, 2 * Dq, s))) return rc;  // (the quantizer's own input)
    PassCtx ctx{lane, s, e->precision};
    ctx.chain_ok = true;  // (checked right here: a give-up re-runs the levels on the per-level kernels)
    PassOut out;
    if ((rc = run_rvq(e, ctx, proj, frames, K, codes, 0, work, rec, &out))) return rc;
    if (out.chain_flag) {
        unsigned flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, out.chain_flag, sizeof flag, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (flag) {
            ++e->chain_reruns;
            ctx.chain_ok = false;
            if ((rc = run_rvq(e, ctx, proj, frames, K, codes, 0, work, rec, &out))) return rc;
        }
    }
    HIP_TRY(hipEventRecord(lane.ws_free, s));
    return MIMI_OK;
}

// ------------------------------------------------------------------------------------------------
// decode (MimiModel.decode, TF/modeling_mimi.py:1388-1458): codes [B][K][T] -> waveform [B][1920 T]
// ------------------------------------------------------------------------------------------------
// The mirror of the encode pass, all activations fp32 channels-last:
//   codes --rvq_decode_kernel--> (semantic sum | acoustic sum) [B T][2 Dq]
//         --GEMM, W = [W_sem | W_ac] along K--> embedding [B T][512]      (the two output_proj and their sum, one pass)
//         --upsample_dw_kernel--> [B][2T][512] --decoder_transformer (the encoder's launches, other weights)-->
//         --decoder.layers.0 (k 7, bias + ELU)--> [B][2T][1024]
//         --4 x ( transposed conv as GEMM (ROLE_UPCONV, raw) ; fused residual block + trailing ELU )-->
//         [B][1920 T][64] --final_conv_kernel--> waveform.
// A causal MimiConvTranspose1d (kernel 2r, stride r, the k - s extra outputs trimmed on the right, :399-405) is exactly
// a causal k = 2 convolution with r Cout output channels in phase-major order,
//   out[t r + p][co] = b[co] + sum_ci ( W[ci][co][p] x[t][ci] + W[ci][co][p + r] x[t - 1][ci] ),   x[-1] = 0,
// so the channels-last GEMM output [T][r Cout] IS the up-sampled tensor [T r][Cout]: no pixel-shuffle pass.
// ARITHMETIC: decode always runs the fp32-MFMA GEMMs and the fp32 attention / residual-block kernels (PREC_F32),
// whatever mimi_set_precision says: no activation scales, so no calibration, no overflow read-back, no fallback.
// A mixed-length batch (mimi_decode_ragged) runs the same pass (decode_pass) over packed rows: DecLayout below.
// Chunk by chunk on a KV cache: "decode stream" below (mimi_decode_stream_*).
// The other direction chunk by chunk: "encode stream" further below (mimi_encode_stream_*).
// Not built here: f16x3 decode, hipGraph capture of decode or of a stream's step.

static int64_t decode_upsampling(const mimi_config& c) {
    int64_t f = 2;  // upsample: 12.5 -> 25 Hz
    for (int i = 0; i < c.num_ratios; ++i) f *= c.upsampling_ratios[i];
    return f;
}

extern "C" int64_t mimi_decoded_length_cfg(const mimi_config* cfg, int64_t frames) {
    mimi_config d;
    if (!cfg) {
        mimi_config_default(&d);
        cfg = &d;
    }
    if (frames < 0) return -1;
    return frames * decode_upsampling(*cfg);
}

extern "C" int64_t mimi_decoded_length(int64_t frames) { return mimi_decoded_length_cfg(nullptr, frames); }

// W [Cin][Cout][2r] (ConvTranspose1d layout) -> W'[p Cout + co][tap Cin + ci]: tap 0 multiplies x[t - 1] and holds
// W[ci][co][p + r], tap 1 multiplies x[t] and holds W[ci][co][p]
static void relayout_upconv(const float* w, int cin, int cout, int r, float* o) {
    for (int p = 0; p < r; ++p)
        for (int co = 0; co < cout; ++co) {
            float* row = o + ((size_t)p * cout + co) * 2 * cin;
            for (int ci = 0; ci < cin; ++ci) {
                const float* src = w + ((size_t)ci * cout + co) * 2 * r;
                row[ci] = src[p + r];
                row[cin + ci] = src[p];
            }
        }
}

extern "C" int mimi_upconv_relayout(const float* w, int32_t cin, int32_t cout, int32_t ratio, float* out) {
    if (!w || !out || cin < 1 || cout < 1 || ratio < 1) return set_err(MIMI_ERR_INVALID_ARGUMENT, "mimi_upconv_relayout: bad arguments");
    relayout_upconv(w, cin, cout, ratio, out);
    return MIMI_OK;
}

static void build_expected_decode(mimi_engine* e) {
    const mimi_config& c = e->cfg;
    auto& ex = e->expected;
    const int h = c.hidden_size;
    int C = c.num_filters << c.num_ratios;
    ex["decoder.layers.0.conv.weight"] = {C, h, c.kernel_size};
    ex["decoder.layers.0.conv.bias"] = {C};
    int idx = 1;
    for (int s = 0; s < c.num_ratios; ++s) {
        const int r = c.upsampling_ratios[s];
        idx += 1;  // ELU
        const std::string u = "decoder.layers." + std::to_string(idx) + ".conv.";
        ex[u + "weight"] = {C, C / 2, 2 * r};
        ex[u + "bias"] = {C / 2};
        idx += 1;
        C /= 2;
        const std::string p = "decoder.layers." + std::to_string(idx) + ".block.";
        ex[p + "1.conv.weight"] = {C / c.compress, C, c.residual_kernel_size};
        ex[p + "1.conv.bias"] = {C / c.compress};
        ex[p + "3.conv.weight"] = {C, C / c.compress, 1};
        ex[p + "3.conv.bias"] = {C};
        idx += 1;
    }
    idx += 1;  // ELU
    const std::string f = "decoder.layers." + std::to_string(idx) + ".conv.";
    ex[f + "weight"] = {c.audio_channels, C, c.last_kernel_size};
    ex[f + "bias"] = {c.audio_channels};
    ex["upsample.conv.weight"] = {h, 1, c.downsample_kernel};
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string p = "decoder_transformer.layers." + std::to_string(l) + ".";
        for (const char* n : {"q_proj", "k_proj", "v_proj"})
            ex[p + "self_attn." + n + ".weight"] = {c.num_attention_heads * c.head_dim, h};
        ex[p + "self_attn.o_proj.weight"] = {h, c.num_attention_heads * c.head_dim};
        ex[p + "mlp.fc1.weight"] = {c.intermediate_size, h};
        ex[p + "mlp.fc2.weight"] = {h, c.intermediate_size};
        for (const char* n : {"input_layernorm", "post_attention_layernorm"}) {
            ex[p + n + ".weight"] = {h};
            ex[p + n + ".bias"] = {h};
        }
        ex[p + "self_attn_layer_scale.scale"] = {h};
        ex[p + "mlp_layer_scale.scale"] = {h};
    }
    for (const char* q : {"semantic", "acoustic"})
        ex[std::string("quantizer.") + q + "_residual_vector_quantizer.output_proj.weight"] = {h, c.vq_hidden_dim, 1};
}

extern "C" int mimi_enable_decode(mimi_engine* e) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->decode_enabled) return MIMI_OK;
    if (e->finalized) return set_err(MIMI_ERR_STATE, "mimi_enable_decode must come before mimi_finalize");
    const mimi_config& c = e->cfg;
    // the kernels behind the decode pass: fused residual blocks at C = 64 .. 512, the 64 -> 1 k = 3 last conv, the
    // k = 4 stride-2 depthwise upsample
    if (c.num_ratios > 4 || c.num_filters != 64 || c.last_kernel_size != 3 || c.audio_channels != 1 ||
        c.residual_kernel_size != 3 || c.compress != 2 || c.downsample_kernel != 4 || c.downsample_stride != 2)
        return set_err(MIMI_ERR_UNSUPPORTED, "decode: config outside the kyutai/mimi decoder family");
    build_expected_decode(e);
    e->decode_enabled = true;
    return MIMI_OK;
}

static int finalize_decode(mimi_engine* e) {
    const mimi_config& c = e->cfg;
    const int h = c.hidden_size, n = c.num_ratios;
    int rc;
    int C = c.num_filters << n;
    if ((rc = make_conv(e, e->dec_first, "decoder.layers.0.conv.", h, C, c.kernel_size, 1, true))) return rc;
    e->dec_up.resize(n);
    e->dec_res3.resize(n);
    e->dec_res1.resize(n);
    int idx = 1;
    for (int s = 0; s < n; ++s) {
        const int r = c.upsampling_ratios[s];
        idx += 1;
        const std::string u = "decoder.layers." + std::to_string(idx) + ".conv.";
        std::vector<float>*w, *b;
        if ((rc = get_w(e, u + "weight", &w)) || (rc = get_w(e, u + "bias", &b))) return rc;
        const int cin = C, cout = C / 2;
        std::vector<float> wl((size_t)r * cout * 2 * cin), bl((size_t)r * cout);
        relayout_upconv(w->data(), cin, cout, r, wl.data());
        for (int p = 0; p < r; ++p)
            for (int co = 0; co < cout; ++co) bl[(size_t)p * cout + co] = (*b)[co];
        DevConv& dc = e->dec_up[s];
        dc.cin = cin;
        dc.cout = r * cout;
        dc.k = 2;
        dc.stride = 1;
        if ((rc = upload(e, &dc.w, wl)) || (rc = upload(e, &dc.b, bl))) return rc;
        idx += 1;
        C = cout;
        const std::string p = "decoder.layers." + std::to_string(idx) + ".block.";
        if ((rc = make_conv(e, e->dec_res3[s], p + "1.conv.", C, C / c.compress, c.residual_kernel_size, 1, true))) return rc;
        if ((rc = make_conv(e, e->dec_res1[s], p + "3.conv.", C / c.compress, C, 1, 1, true))) return rc;
        idx += 1;
    }
    idx += 1;
    if ((rc = make_conv(e, e->dec_last, "decoder.layers." + std::to_string(idx) + ".conv.", C, 1, c.last_kernel_size, 1, true)))
        return rc;
    std::vector<float>* t;
    if ((rc = get_w(e, "upsample.conv.weight", &t)) || (rc = upload(e, &e->upsample_w, *t))) return rc;
    e->dxf.resize(c.num_hidden_layers);
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string p = "decoder_transformer.layers." + std::to_string(l) + ".";
        DevXfmr& x = e->dxf[l];
        std::vector<float>*q, *k, *v;
        if ((rc = get_w(e, p + "self_attn.q_proj.weight", &q)) || (rc = get_w(e, p + "self_attn.k_proj.weight", &k)) ||
            (rc = get_w(e, p + "self_attn.v_proj.weight", &v)))
            return rc;
        std::vector<float> qkv(*q);
        qkv.insert(qkv.end(), k->begin(), k->end());
        qkv.insert(qkv.end(), v->begin(), v->end());
        if ((rc = upload(e, &x.wqkv, qkv))) return rc;
        struct {
            const char* n;
            float** d;
        } simple[] = {{"self_attn.o_proj.weight", &x.wo},
                      {"mlp.fc1.weight", &x.w1},
                      {"mlp.fc2.weight", &x.w2},
                      {"input_layernorm.weight", &x.ln1_w},
                      {"input_layernorm.bias", &x.ln1_b},
                      {"post_attention_layernorm.weight", &x.ln2_w},
                      {"post_attention_layernorm.bias", &x.ln2_b},
                      {"self_attn_layer_scale.scale", &x.ls1},
                      {"mlp_layer_scale.scale", &x.ls2}};
        for (auto& sp : simple)
            if ((rc = get_w(e, p + sp.n, &t)) || (rc = upload(e, sp.d, *t))) return rc;
    }
    {
        // [W_sem | W_ac] along K: one GEMM computes output_proj_sem(sem) + output_proj_ac(ac)
        std::vector<float>*ps, *pa;
        if ((rc = get_w(e, "quantizer.semantic_residual_vector_quantizer.output_proj.weight", &ps)) ||
            (rc = get_w(e, "quantizer.acoustic_residual_vector_quantizer.output_proj.weight", &pa)))
            return rc;
        const int Dq = c.vq_hidden_dim;
        std::vector<float> both((size_t)h * 2 * Dq);
        for (int o = 0; o < h; ++o)
            for (int d = 0; d < Dq; ++d) {
                both[(size_t)o * 2 * Dq + d] = (*ps)[(size_t)o * Dq + d];
                both[(size_t)o * 2 * Dq + Dq + d] = (*pa)[(size_t)o * Dq + d];
            }
        if ((rc = upload(e, &e->outproj, both))) return rc;
    }
    if ((rc = dev_alloc(e, reinterpret_cast<void**>(&e->dec_flag), 256))) return rc;
    HIP_TRY(hipMemset(e->dec_flag, 0, 256));
    HIP_TRY(hipHostMalloc(&e->dec_flag_host, sizeof(unsigned), hipHostMallocDefault));
    return MIMI_OK;
}

// The layout of one decode pass.  Every stage's tensor is [rows][C]: stage 0 the 12.5 Hz frames, 1 the 25 Hz ones, 2 ..
// behind each up conv; a stage's rows are f[st] per frame (1, 2, 2 r0, 2 r0 r1, ...: integers).
//   uniform (mimi_decode): item b's rows of a stage are rows b f T .. of [B][f T][C]; no tables.
//   ragged (mimi_decode_ragged): the rows are PACKED, item b's at row f toff[b] of one [f sumT][C] tensor (toff = the
//     prefix sum of the frame lengths) -- the transformer-section layout of encode's RaggedTable carried through the
//     whole pass.  One (tlen, toff) pair describes every stage; the device image holds it once per stage already
//     multiplied, [stage][tlen | toff][B] ints, so that the kernels index an int table as the encode-side ragged
//     kernels do.  Uploaded once per call from pinned memory.
// A uniform batch is the ragged one whose items all have T frames: both have f sumT rows per stage.
struct DecLayout {
    int B = 0, nst = 0;
    bool ragged = false;
    int64_t sumT = 0, maxT = 0, minT = 0;  // frames: of all items, of the longest and of the shortest
    int64_t stride = 0;                    // frames per item of the caller's padded codes and waveform
    std::vector<int64_t> f;                // rate factor per stage
    const int* dev = nullptr;              // ragged: the tables' device image
    int64_t rows(int st) const { return f[st] * sumT; }  // of the whole tensor
    int64_t len(int st) const { return f[st] * maxT; }   // of the longest item: what a launch covers
    const int* tlen(int st) const { return ragged ? dev + (size_t)(2 * st) * B : nullptr; }
    const int* toff(int st) const { return ragged ? dev + (size_t)(2 * st + 1) * B : nullptr; }
    size_t ints() const { return ragged ? (size_t)2 * nst * B : 0; }
};

// lengths: the items' frames (ragged: codes rows of `stride` frames), or null for a uniform batch of `stride` frames each
static int plan_decode(const mimi_engine* e, const int64_t* lengths, int32_t batch, int64_t stride, DecLayout* L) {
    const mimi_config& c = e->cfg;
    L->B = batch;
    L->nst = 2 + c.num_ratios;
    L->ragged = lengths != nullptr;
    L->stride = stride;
    L->f.assign(1, 1);
    L->f.push_back(2);
    for (int i = 0; i < c.num_ratios; ++i) L->f.push_back(L->f.back() * c.upsampling_ratios[i]);
    L->sumT = lengths ? 0 : batch * stride;
    L->maxT = lengths ? 0 : stride;
    L->minT = lengths ? INT64_MAX : stride;
    for (int b = 0; lengths && b < batch; ++b) {
        if (lengths[b] < 1) return 1;
        L->sumT += lengths[b];
        L->maxT = std::max(L->maxT, lengths[b]);
        L->minT = std::min(L->minT, lengths[b]);
        if (L->sumT > 0x7fffffffLL) return 2;
    }
    return 0;
}

static size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// decode's workspace: two ping-pong regions (P: RVQ sums + embedding, then the SEANet's ELU'd tensors; Q: the
// transformer's buffers, then the raw up-conv outputs), with taps on the raw decoder.layers.0 output, and a ragged
// pass's tables.  Every size is per frame, so a ragged pass has the activations of the B = 1 decode of sumT frames.
struct DecodeWs {
    float *p, *q, *tap;
    int* tab;
    size_t bytes;
};
static DecodeWs decode_ws_layout(const mimi_engine* e, const DecLayout& L, bool taps) {
    const mimi_config& c = e->cfg;
    const size_t h = c.hidden_size, T = (size_t)L.sumT, T2 = 2 * T;
    size_t C = (size_t)c.num_filters << c.num_ratios, len = T2;
    size_t pmax = std::max(T * (h + 2 * c.vq_hidden_dim), T2 * C);
    size_t qmax = T2 * (3 * h + 3 * (size_t)c.num_attention_heads * c.head_dim + c.intermediate_size);
    for (int s = 0; s < c.num_ratios; ++s) {
        len *= c.upsampling_ratios[s];
        C /= 2;
        pmax = std::max(pmax, len * C);
        qmax = std::max(qmax, len * C);
    }
    DecodeWs w{};
    char* base = reinterpret_cast<char*>(e->dws);
    size_t off = 0;
    w.p = reinterpret_cast<float*>(base + off);
    off += pad256(pmax * sizeof(float));
    w.q = reinterpret_cast<float*>(base + off);
    off += pad256(qmax * sizeof(float));
    w.tap = reinterpret_cast<float*>(base + off);
    if (taps) off += pad256(T2 * ((size_t)c.num_filters << c.num_ratios) * sizeof(float));
    w.tab = reinterpret_cast<int*>(base + off);
    off += pad256(L.ints() * sizeof(int));
    w.bytes = off;
    return w;
}

static int ensure_dws(mimi_engine* e, size_t bytes) {
    if (bytes <= e->dws_bytes) return MIMI_OK;
    // (every decode synchronises its stream before it returns: nothing reads the old buffer)
    if (e->dws) {
        HIP_TRY(hipFree(e->dws));
        e->dws = nullptr;
        e->dws_bytes = 0;
    }
    hipError_t err = hipMalloc(&e->dws, bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        e->dws = nullptr;
        return set_err(err == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP,
                       "decode workspace hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(err));
    }
    e->dws_bytes = bytes;
    return MIMI_OK;
}

extern "C" int64_t mimi_decode_workspace_bytes(const mimi_engine* e, int32_t batch, int64_t frames) {
    if (!e || batch <= 0 || frames <= 0) return -1;
    DecLayout L;
    plan_decode(e, nullptr, batch, frames, &L);
    return (int64_t)decode_ws_layout(e, L, e->taps).bytes;
}

// codes -> (semantic | acoustic) sums in `sums` -> embedding [frames][hidden] in `emb` (the rows of L's stage 0)
static int run_dequantize(mimi_engine* e, const int32_t* codes, const DecLayout& L, int K, float* sums, float* emb,
                          hipStream_t s, Recorder& rec) {
    const mimi_config& c = e->cfg;
    const int Dq = c.vq_hidden_dim;
    const int64_t frames = L.rows(0);
    LAUNCH_TRY(launch_rvq_decode(codes, L.B * L.stride, (int)L.stride, K, c.num_semantic_quantizers, c.codebook_size,
                                 c.codebook_dim, e->cb_rows, sums, e->dec_flag, s, L.tlen(0), L.toff(0), (int)L.maxT),
               "rvq_decode");
    rec.mark("dec_rvq", (double)frames * K * Dq, (double)frames * (K * Dq + 2 * Dq) * 4,
             L.ragged ? "mimi::rvq_decode_ragged_kernel" : "mimi::rvq_decode_kernel");
    GemmArgs ap = linear_args(sums, frames, 2 * Dq, e->outproj, c.hidden_size, emb);
    const char* kname = "?";
    LAUNCH_TRY(launch_gemm(ROLE_INPROJ, ap, s, &kname, PREC_F32), "output_proj");
    rec.mark("dec_output_proj", 2.0 * frames * 2 * Dq * c.hidden_size, (double)frames * (2 * Dq + c.hidden_size) * 4, kname);
    return MIMI_OK;
}

// the bounds flag of the decode just enqueued on s (synchronises s)
static int read_decode_flag(mimi_engine* e, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(e->dec_flag_host, e->dec_flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*e->dec_flag_host)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "code outside [0, codebook_size): [0, %d)", e->cfg.codebook_size);
    return MIMI_OK;
}

static int check_decode_state(mimi_engine* e, int32_t K) {
    if (!e->finalized) return set_err(MIMI_ERR_STATE, "mimi_finalize has not been called");
    if (!e->decode_enabled)
        return set_err(MIMI_ERR_STATE, "engine was built without the decode weights (mimi_enable_decode / MIMI_CREATE_DECODE)");
    if (K < 1 || K > e->levels_available)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "num_quantizers %d outside [1, %d]", K, e->levels_available);
    return MIMI_OK;
}

extern "C" int mimi_rvq_decode(mimi_engine* e, const int32_t* dev_codes, int64_t frames, int32_t K, float* dev_embedding,
                               void* stream) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_decode_state(e, K);
    if (rc) return rc;
    if (frames <= 0 || frames > 0x7fffffffLL || !dev_codes || !dev_embedding)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "frames=%lld", (long long)frames);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = ensure_dws(e, pad256((size_t)frames * 2 * e->cfg.vq_hidden_dim * sizeof(float))))) return rc;
    HIP_TRY(hipMemsetAsync(e->dec_flag, 0, sizeof(unsigned), s));
    Recorder rec{e, s};
    rec.begin();
    DecLayout L;
    plan_decode(e, nullptr, 1, frames, &L);
    if ((rc = run_dequantize(e, dev_codes, L, K, reinterpret_cast<float*>(e->dws), dev_embedding, s, rec))) return rc;
    return read_decode_flag(e, s);
}

// The fp32 transformer layer loop of the one-shot decode (uniform and ragged), the decode stream and the encode stream
// (lock-step and slot steps): the encoder's fp32 launches (LayerNorm, q/k/v + RoPE, attention, o_proj, fc1, fc2) on the
// weight set xf over `rows` flat rows, residual stream in t0 (in place), every stage recorded as stage_prefix + its
// name and tapped as [tapB][tapT][C] under the encode pass's names ("qkv3").  What differs between the callers arrives
// as two callables:
//   qkv_args(x)   the GemmArgs of layer x's q/k/v GEMM (t1 -> qkv): how the rows are batched and which RoPE table
//   attention(l)  everything between q/k/v and o_proj of layer l (qkv -> att), with its records
template <class QkvArgs, class Attention>
static int transformer_f32(mimi_engine* e, const std::vector<DevXfmr>& xf, float* t0, float* t1, float* qkv, float* att,
                           float* ff, int64_t rows, int64_t tapB, int64_t tapT, const char* stage_prefix, Recorder& rec,
                           hipStream_t s, QkvArgs qkv_args, Attention attention) {
    const mimi_config& c = e->cfg;
    const int Hd = c.hidden_size, H = c.num_attention_heads, Dh = c.head_dim;
    const std::string sp = stage_prefix;
    const char* kname = "?";
    int rc;
    auto tap = [&](const char* stage, size_t l, const float* src, int C) {
        return save_tap_layer(e, stage, l, src, tapB, tapT, C, s);
    };
    auto fl = [](const GemmArgs& a) { return 2.0 * a.batch * (double)a.M * a.N * a.K; };
    auto by = [](const GemmArgs& a, bool res) {
        return ((double)a.batch * a.M * (a.K + a.N * (res ? 2 : 1)) + (double)a.N * a.K) * 4;
    };
    for (size_t l = 0; l < xf.size(); ++l) {
        const DevXfmr& x = xf[l];
        LAUNCH_TRY(launch_layernorm(t0, x.ln1_w, x.ln1_b, t1, rows, Hd, c.norm_eps, s, nullptr, 0, 0, 0.0f, nullptr,
                                    nullptr, 0, e->ln_rpw),
                   "ln1");
        rec.mark(sp + "layernorm", 0, 2.0 * rows * Hd * 4, ln_kname(e->ln_rpw));
        const GemmArgs aq = qkv_args(x);
        LAUNCH_TRY(launch_gemm(ROLE_QKV, aq, s, &kname, PREC_F32), "qkv");
        rec.mark(sp + "qkv", fl(aq), by(aq, false), kname);
        if ((rc = tap("qkv", l, qkv, 3 * H * Dh))) return rc;
        if ((rc = attention(l))) return rc;
        if ((rc = tap("att", l, att, H * Dh))) return rc;
        GemmArgs ao = linear_args(att, rows, H * Dh, x.wo, Hd, t0);
        ao.R = t0;
        ao.scale = x.ls1;
        LAUNCH_TRY(launch_gemm(ROLE_OPROJ, ao, s, &kname, PREC_F32), "o_proj");
        rec.mark(sp + "o_proj", fl(ao), by(ao, true), kname);
        if ((rc = tap("oproj", l, t0, Hd))) return rc;
        LAUNCH_TRY(launch_layernorm(t0, x.ln2_w, x.ln2_b, t1, rows, Hd, c.norm_eps, s, nullptr, 0, 0, 0.0f, nullptr,
                                    nullptr, 0, e->ln_rpw),
                   "ln2");
        rec.mark(sp + "layernorm", 0, 2.0 * rows * Hd * 4, ln_kname(e->ln_rpw));
        GemmArgs a1 = linear_args(t1, rows, Hd, x.w1, c.intermediate_size, ff);
        LAUNCH_TRY(launch_gemm(ROLE_FC1, a1, s, &kname, PREC_F32), "fc1");
        rec.mark(sp + "fc1", fl(a1), by(a1, false), kname);
        if ((rc = tap("ff", l, ff, c.intermediate_size))) return rc;
        GemmArgs a2 = linear_args(ff, rows, c.intermediate_size, x.w2, Hd, t0);
        a2.R = t0;
        a2.scale = x.ls2;
        LAUNCH_TRY(launch_gemm(ROLE_FC2, a2, s, &kname, PREC_F32), "fc2");
        rec.mark(sp + "fc2", fl(a2), by(a2, true), kname);
        if ((rc = tap("xfmr", l, t0, Hd))) return rc;
    }
    return MIMI_OK;
}

// The decode pass on the layout L (its tables, if any, already on the device; the workspace w sized for it): every
// launch from the codes to the last conv, with its profile record and tap.  A stage either runs on all rows at once
// (the flat-row GEMMs and LayerNorm) or per item, where a ragged batch takes an item's base and length from the
// tables and otherwise runs the uniform batch's arithmetic: item b's samples are bitwise those of its own B = 1 pass.
// The caller takes the "audio" tap and reads the bounds flag.
static int decode_pass(mimi_engine* e, const int32_t* dev_codes, const DecLayout& L, const DecodeWs& w, int K,
                       float* dev_audio, hipStream_t s) {
    const mimi_config& c = e->cfg;
    const int B = L.B, Hd = c.hidden_size, Dq = c.vq_hidden_dim;
    int rc;
    if ((rc = ensure_rope(e, L.len(1)))) return rc;
    HIP_TRY(hipMemsetAsync(e->dec_flag, 0, sizeof(unsigned), s));
    Recorder rec{e, s};
    rec.begin();
    const char* kname = "?";
    // a conv over stage st's rows as a GEMM per item
    auto conv = [&](const DevConv& cv, const float* in, float* out, int st) {
        GemmArgs a = conv_args(cv, in, L.len(st), out, L.len(st), B);
        a.a_rows = a.m_rows = L.tlen(st);
        a.a_boff = a.c_boff = L.toff(st);
        return a;
    };
    auto fl = [&](const GemmArgs& a, int st) { return 2.0 * (double)L.rows(st) * a.N * a.K; };
    auto by = [&](const GemmArgs& a, int st) { return ((double)L.rows(st) * (a.a_rs + a.N) + (double)a.N * a.K) * 4; };
    auto tap = [&](const char* name, const float* src, int st, int C) {  // a ragged pass's taps are packed
        return L.ragged ? save_tap(e, name, src, 1, L.rows(st), C, s) : save_tap(e, name, src, B, L.len(st), C, s);
    };

    // ---- quantizer.decode + upsample ----
    float* sums = w.p;
    float* emb = w.p + (size_t)L.rows(0) * 2 * Dq;
    if ((rc = run_dequantize(e, dev_codes, L, K, sums, emb, s, rec))) return rc;
    if ((rc = tap("quantized", emb, 0, Hd))) return rc;
    float* t0 = w.q;
    float* t1 = t0 + (size_t)L.rows(1) * Hd;
    float* qkv = t1 + (size_t)L.rows(1) * Hd;
    float* att = qkv + (size_t)L.rows(1) * 3 * c.num_attention_heads * c.head_dim;
    float* ff = att + (size_t)L.rows(1) * Hd;
    LAUNCH_TRY(launch_upsample_dw(emb, e->upsample_w, t0, B, L.len(0), Hd, s, L.tlen(0), L.toff(0)), "upsample");
    rec.mark("dec_upsample", 4.0 * L.rows(1) * Hd, 3.0 * L.rows(0) * Hd * 4,
             L.ragged ? "mimi::upsample_dw_ragged_kernel" : "mimi::upsample_dw_kernel");
    if ((rc = tap("upsample", t0, 1, Hd))) return rc;

    // ---- decoder transformer ----
    // The flat-row stages run on all rows whatever the layout; q/k/v and attention run per item (T = the longest
    // item's rows), a ragged batch's from the tables (2 tlen[b] rows at 2 toff[b]).  A ragged pass's taps are packed.
    {
        const int H = c.num_attention_heads, Dh = c.head_dim;
        const int64_t T = L.len(1), rows = L.rows(1);
        auto qkv_args = [&](const DevXfmr& x) {
            GemmArgs aq = linear_args(t1, T, Hd, x.wqkv, 3 * H * Dh, qkv);
            aq.batch = B;
            aq.a_bstride = T * Hd;
            aq.c_bstride = T * 3 * H * Dh;
            aq.rope_cos = e->rope_cos;
            aq.rope_sin = e->rope_sin;
            aq.rope_cols = 2 * H * Dh;
            // ragged, per item: rows, zero padding and RoPE position relative to the item's first row
            aq.a_rows = aq.m_rows = L.tlen(1);
            aq.a_boff = aq.c_boff = L.toff(1);
            return aq;
        };
        double att_flops = 0;
        for (int64_t i = 0; i < T; ++i) att_flops += 4.0 * Dh * std::min<int64_t>(i + 1, c.sliding_window);
        att_flops *= (double)H * B;
        const float sc = 1.0f / std::sqrt((float)Dh);
        const char* akn = T <= 256 ? "mimi::attention_t256_kernel" : "mimi::attention_kernel";
        auto att_mark = [&] { rec.mark("dec_attention", att_flops, (double)rows * 4 * Hd * 4, akn); };
        auto attention = [&](size_t) {
            LAUNCH_TRY(launch_attention(qkv, att, B, (int)T, H, Dh, c.sliding_window, sc, s, att, rows * Hd, 0, 0.0f,
                                        nullptr, false, nullptr, 0, 0, nullptr, &akn, e->attn_band_split),
                       "attention");
            att_mark();
            return (int)MIMI_OK;
        };
        // each item the kernel it would run alone: one launch per 256-row regime present (and one record each), each
        // kernel exiting on the other's items
        const int lo = (int)(2 * L.minT), hi = (int)(2 * L.maxT);
        auto attention_ragged = [&](size_t) {
            if (lo <= 256) {
                LAUNCH_TRY(launch_attention(qkv, att, B, 0, H, Dh, c.sliding_window, sc, s, nullptr, 0, 0, 0.0f, nullptr,
                                            false, L.tlen(1), std::min(hi, 256), lo, L.toff(1), &akn),
                           "attention");
                att_mark();
            }
            if (hi > 256) {
                LAUNCH_TRY(launch_attention(qkv, att, B, 0, H, Dh, c.sliding_window, sc, s, nullptr, 0, 0, 0.0f, nullptr,
                                            false, L.tlen(1), hi, std::max(lo, 257), L.toff(1), &akn),
                           "attention");
                att_mark();
            }
            return (int)MIMI_OK;
        };
        rc = L.ragged ? transformer_f32(e, e->dxf, t0, t1, qkv, att, ff, rows, 1, rows, "dec_", rec, s, qkv_args,
                                        attention_ragged)
                      : transformer_f32(e, e->dxf, t0, t1, qkv, att, ff, rows, B, T, "dec_", rec, s, qkv_args, attention);
        if (rc) return rc;
    }
    char nm[64];

    // ---- SEANet decoder ----
    int C = c.num_filters << c.num_ratios;
    if (e->taps) {  // the raw layer-0 output (the pass itself only needs its ELU)
        GemmArgs at = conv(e->dec_first, t0, w.tap, 1);
        LAUNCH_TRY(launch_gemm(ROLE_DOWN, at, s, &kname, PREC_F32), "decoder conv 0 (tap)");
        rec.mark("dec_conv0_tap", fl(at, 1), by(at, 1), kname);
        if ((rc = tap("dconv0", w.tap, 1, C))) return rc;
    }
    float* xe = w.p;  // ELU'd input of the next up conv
    GemmArgs a0 = conv(e->dec_first, t0, xe, 1);
    LAUNCH_TRY(launch_gemm(ROLE_DOWN_ELU, a0, s, &kname, PREC_F32), "decoder conv 0");
    rec.mark("dec_conv0", fl(a0, 1), by(a0, 1), kname);
    if ((rc = tap("dconv0_elu", xe, 1, C))) return rc;  // what the pass itself computes and up conv 0 reads
    for (int si = 0; si < c.num_ratios; ++si) {
        const int st = 1 + si;  // the up conv's input (and GEMM rows); its output is stage st + 1
        // [len][C] -> [len][r * C/2] = [len * r][C/2]
        GemmArgs au = conv(e->dec_up[si], xe, w.q, st);
        LAUNCH_TRY(launch_gemm(ROLE_UPCONV, au, s, &kname, PREC_F32), "up conv");
        snprintf(nm, sizeof nm, "dec_up_s%d", si);
        rec.mark(nm, fl(au, st), by(au, st), kname);
        C /= 2;
        snprintf(nm, sizeof nm, "up%d", si);
        if ((rc = tap(nm, w.q, st + 1, C))) return rc;
        ResArgs ra{};
        ra.x = w.q;
        ra.T = L.len(st + 1);
        ra.batch = B;
        ra.w3 = e->dec_res3[si].w;
        ra.b3 = e->dec_res3[si].b;
        ra.w1 = e->dec_res1[si].w;
        ra.b1 = e->dec_res1[si].b;
        ra.y = xe;
        ra.ilen = L.tlen(st + 1);
        ra.ioff = L.toff(st + 1);
        LAUNCH_TRY(launch_resblock(C, ra, s, &kname), "decoder resblock");
        snprintf(nm, sizeof nm, "dec_res_s%d", si);
        const double Hh = C / c.compress, rows = (double)L.rows(st + 1);
        rec.mark(nm, 2.0 * rows * (3.0 * C * Hh + Hh * C), rows * 2 * C * 4, kname);
        snprintf(nm, sizeof nm, "dres%d_elu", si);
        if ((rc = tap(nm, xe, st + 1, C))) return rc;
    }
    const int last = L.nst - 1;
    LAUNCH_TRY(launch_final_conv(xe, e->dec_last.w, e->dec_last.b, dev_audio, B, L.f[last] * L.stride, C,
                                 c.last_kernel_size, s, L.tlen(last), L.toff(last), L.len(last)),
               "final conv");
    rec.mark("dec_final", 2.0 * L.rows(last) * C * c.last_kernel_size, (double)L.rows(last) * (C + 1) * 4,
             L.ragged ? "mimi::final_conv_ragged_kernel" : "mimi::final_conv_kernel");
    return MIMI_OK;
}

extern "C" int mimi_decode(mimi_engine* e, const int32_t* dev_codes, int32_t batch, int64_t frames, int32_t K,
                           float* dev_audio, void* stream) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_decode_state(e, K);
    if (rc) return rc;
    const int64_t up = decode_upsampling(e->cfg);
    if (batch <= 0 || batch > 65535 || frames <= 0 || !dev_codes || !dev_audio)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "batch=%d frames=%lld", batch, (long long)frames);
    // the GEMMs index an item's rows with 32-bit M and the rvq kernel B * T frames with 32-bit blocks
    if (frames * up > 0x7fffffffLL || (int64_t)batch * frames > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "decode of %lld frames per item exceeds the 32-bit row range", (long long)frames);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DecLayout L;
    plan_decode(e, nullptr, batch, frames, &L);
    if ((rc = ensure_dws(e, decode_ws_layout(e, L, e->taps).bytes))) return rc;
    if ((rc = decode_pass(e, dev_codes, L, decode_ws_layout(e, L, e->taps), K, dev_audio, s))) return rc;
    if ((rc = save_tap(e, "audio", dev_audio, batch, up * frames, 1, s))) return rc;
    return read_decode_flag(e, s);
}

// ---- ragged decode: B items of frame_lengths[b] frames in one pass over packed rows (DecLayout) ----
// The caller's codes are padded [B][K][max_frames] and its waveform padded [B][up max_frames]: the columns past an
// item's length are never read, the samples past it never written.
extern "C" int64_t mimi_decode_ragged_workspace_bytes(const mimi_engine* e, const int64_t* frame_lengths, int32_t batch) {
    if (!e || !frame_lengths || batch <= 0) return -1;
    DecLayout L;
    if (plan_decode(e, frame_lengths, batch, 0, &L)) return -1;
    return (int64_t)decode_ws_layout(e, L, e->taps).bytes;
}

// the "audio" tap of a ragged decode: the items' samples packed, as every other tap of the pass
static int save_tap_audio_ragged(mimi_engine* e, const float* audio, const int64_t* lengths, const DecLayout& L,
                                 hipStream_t s) {
    if (!e->taps) return MIMI_OK;
    const int64_t up = L.f.back();
    float* d;
    int rc;
    if ((rc = tap_buffer(e, "audio", 1, up * L.sumT, 1, &d))) return rc;
    int64_t off = 0;
    for (int b = 0; b < L.B; ++b) {
        HIP_TRY(hipMemcpyAsync(d + up * off, audio + (size_t)b * (up * L.stride), (size_t)(up * lengths[b]) * 4,
                               hipMemcpyDeviceToDevice, s));
        off += lengths[b];
    }
    return MIMI_OK;
}

static int decode_ragged_locked(mimi_engine* e, const int32_t* dev_codes, const int64_t* lengths, int K,
                                float* dev_audio, hipStream_t s, DecLayout& L) {
    int rc;
    if ((rc = ensure_dws(e, decode_ws_layout(e, L, e->taps).bytes))) return rc;
    const DecodeWs w = decode_ws_layout(e, L, e->taps);
    const size_t nints = L.ints();
    if (e->dec_rg_cap < nints) {
        if (e->dec_rg_host) HIP_TRY(hipHostFree(e->dec_rg_host));
        e->dec_rg_host = nullptr;
        e->dec_rg_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->dec_rg_host), nints * sizeof(int), hipHostMallocDefault));
        e->dec_rg_cap = nints;
    }
    int* h = e->dec_rg_host;
    for (int st = 0; st < L.nst; ++st) {
        int64_t off = 0;
        for (int b = 0; b < L.B; ++b) {
            h[(size_t)(2 * st) * L.B + b] = (int)(L.f[st] * lengths[b]);
            h[(size_t)(2 * st + 1) * L.B + b] = (int)(L.f[st] * off);
            off += lengths[b];
        }
    }
    HIP_TRY(hipMemcpyAsync(w.tab, h, nints * sizeof(int), hipMemcpyHostToDevice, s));
    L.dev = w.tab;
    if ((rc = decode_pass(e, dev_codes, L, w, K, dev_audio, s))) return rc;
    if ((rc = save_tap_audio_ragged(e, dev_audio, lengths, L, s))) return rc;
    return read_decode_flag(e, s);
}

extern "C" int mimi_decode_ragged(mimi_engine* e, const int32_t* dev_codes, const int64_t* frame_lengths, int32_t batch,
                                  int64_t max_frames, int32_t K, float* dev_audio, void* stream) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_decode_state(e, K);
    if (rc) return rc;
    if (batch <= 0 || batch > 65535 || max_frames <= 0 || !dev_codes || !dev_audio)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "batch=%d max_frames=%lld", batch, (long long)max_frames);
    if ((rc = check_ragged(e, frame_lengths, batch, max_frames))) return rc;
    DecLayout L;
    // the kernels index packed rows with 32-bit ints at every rate, the caller's padded waveform rows too
    if (plan_decode(e, frame_lengths, batch, max_frames, &L) || L.sumT * decode_upsampling(e->cfg) > 0x7fffffffLL ||
        max_frames * decode_upsampling(e->cfg) > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "ragged decode of %lld frames in all exceeds the 32-bit row range",
                       (long long)L.sumT);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = decode_ragged_locked(e, dev_codes, frame_lengths, K, dev_audio, s, L);
    // the tables' pinned host image and the workspace are reused by the next call: nothing of this one stays in flight
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

// ================================================================================================
// decode stream (mimi_decode_stream_*): the decode pass n frames at a time on a KV cache.  DESIGN.md 3.7.1.
//
// Every stage of the decoder is causal, so the samples of frames [p, p + n) of a sequence depend on its past only
// through (per item) the rows each stage reads from in front of the chunk:
//   upsample              1 row  [hidden]   of the output_proj embedding
//   attention, per layer  the rotated k and v rows (P - W, P): a ring of cap = W - 1 + 2 max_step_frames rows
//   decoder.layers.0      k - 1 = 6 rows [hidden] of the transformer output
//   up conv s             1 row  [C_s]      of the ELU'd tensor it reads
//   residual block s      2 rows [C_s / 2]  of the up conv's raw output
//   last conv             k - 1 = 2 rows [filters] of the last block's ELU'd output
// The stream owns these (`carry`, `kring`, `vring`: zero on a fresh or reset stream -- causal padding is zero and
// ELU(0) = 0, so the first step is no special case) and the RoPE rows of the step.  A step runs in the engine's decode
// workspace, which it only uses between taking and leaving the engine mutex: every stage's tensor there is, per item,
// [H carry rows | the chunk's rows], so the GEMM convs read the carry where a one-shot pass reads padding (conv_args
// with a_off moved by H rows) and the per-item kernels run their history forms.  One stream_carry_kernel launch in
// front copies the carries in, one at the end copies the last H rows of every [carry | chunk] out (the two never
// overlap, whatever n), one in the middle moves the transformer's flat rows behind decoder.layers.0's carry.
// Per row every kernel computes what it computes in mimi_decode and attention_stream_kernel reduces in an order
// that is a function of the row's absolute position alone (attn_stream.hip): the samples are the same bits under any
// split of the sequence into steps.
//
// SLOTS.  The state is laid out per item, so item b of it is a slot: its own position, carries and rings.
// mimi_decode_stream_step_slots advances the m slots it lists, each from its own position: item i of the step's
// workspace is slot slots[i] of the state.  What is indirected through the step's device tables (slot_tab, pos_tab:
// uploaded with the step from pinned memory, like the RoPE rows) is exactly what touches the state -- the state side of
// carry-in and carry-out, the rings' base and the position in the attention and the append -- and every other kernel
// works on the workspace, indexed by the item's place in the step.  The q/k/v GEMM runs over the flat m * 2n rows with a
// table of m * 2n RoPE rows in step order (a row's bits do not depend on the tile family, tests/test_decode_kernels.py).
// mimi_decode_stream_step on slots that all stand at one position is the lock-step pass it always was (same launches,
// same names); once the positions differ it is a slot step over 0 .. B - 1.
// ================================================================================================
// What a decode stream and an encode stream have in common: the slots' bookkeeping, the one state allocation (carries |
// k rings | v rings | RoPE cos | RoPE sin), the pinned images of a step's RoPE rows and slot tables.  The stream_*
// helpers below are the parts of create / reset / step that do not depend on the direction (`what`: "decode" /
// "encode", for the messages).
//
// THE LAYOUT OF A STEP (StreamLayout).  Item i of a step brings frames[i] frames; off = the prefix sum of frames.  A
// stage whose tensor has H carry rows per item and f rows per frame holds item i's block [H + f frames[i]][C] at row
// H i + f off[i] of one packed tensor of H m + f sum rows.  With equal counts n this is [m][H + f n][C], the layout the
// lock-step and slot steps always had, and they run on the scalars alone.  With unequal counts (`ragged`) the kernels
// take each item's rows and first row from device tables, already multiplied per stage: one image per step (StreamRag),
// filled in pinned memory the stream owns and uploaded beside slot_tab / pos_tab.  The flat-row stages (the RVQ sums,
// LayerNorm, q/k/v, o_proj, fc1, fc2) have H = 0: item i's rows at f off[i], no gaps, and run on all f sum rows as ever.
struct StreamStage {
    int H;      // carry rows in front of every item's chunk
    int64_t f;  // rows per frame
    int C;      // channels
};
struct StreamLayout {
    int m = 0;
    bool ragged = false;                    // counts given per item: the *_ragged kernels and the tables
    int64_t sum = 0, maxn = 0, stride = 0;  // frames: of all items, of the longest, per item of the caller's padded rows
    std::vector<int32_t> frames, off;
    std::vector<StreamStage> st;  // the stages that have a carry, in the order of the stream's carries
    int64_t len(size_t j, int i) const { return st[j].f * frames[i]; }
    int64_t base(size_t j, int i) const { return (int64_t)st[j].H * i + st[j].f * off[i]; }  // the block's first row
    int64_t rows(size_t j) const { return (int64_t)st[j].H * m + st[j].f * sum; }             // of the whole tensor
};

// frames: the items' counts (each in [1, stride], checked by the caller), or null for n = stride frames each
static void plan_stream(const std::vector<StreamStage>& stages, const int32_t* frames, int m, int64_t stride,
                        StreamLayout* L) {
    L->m = m;
    L->st = stages;
    L->stride = stride;
    L->frames.assign(m, (int32_t)stride);
    L->off.assign(m, 0);
    L->sum = L->maxn = 0;
    for (int i = 0; i < m; ++i) {
        if (frames) L->frames[i] = frames[i];
        L->off[i] = (int32_t)L->sum;
        L->sum += L->frames[i];
        L->maxn = std::max<int64_t>(L->maxn, L->frames[i]);
    }
    L->ragged = frames != nullptr;
}

// The device image of a ragged step's tables for nc carry stages and nr ratios, m entries per table, int64 tables first:
//   eoff [nr][m]       up conv s: item i's first output element (its block of stage 3 + 2 s behind the 2 carry rows)
//   coff [2 nc + 1][2][m]  the carry copies' (source, destination) element offsets: carry-in x nc, the transformer's
//                      rows, carry-out x nc
//   len | base | alen [nc][3][m]  per stage: the item's rows, its block's first row, H + rows
//   off1 | off2 | frames [3][m]  the item's first row in the flat tensors at 12.5 and 25 Hz, and its frames
//   cnt [2 nc + 1][m]   the carry copies' floats
// (an encode stream: nr = 0 up convs, and behind the image, 8-byte aligned, the RVQ's code map: per packed frame the
// place of its level-0 code in the caller's padded [m][K][max_frames], int64 [sum])
static size_t stream_rag_bytes(size_t nc, size_t nr, size_t m) {
    return (nr + 2 * (2 * nc + 1)) * m * sizeof(int64_t) + (3 * nc + 3 + 2 * nc + 1) * m * sizeof(int32_t);
}
static size_t stream_rag_map_at(size_t nc, size_t nr, size_t m) { return (stream_rag_bytes(nc, nr, m) + 7) / 8 * 8; }
struct StreamRag {
    const char* dev = nullptr;  // null: not a ragged step
    size_t nc = 0, nr = 0, m = 0;
    const long long* i64() const { return reinterpret_cast<const long long*>(dev); }
    const int* i32() const { return reinterpret_cast<const int*>(dev + (nr + 2 * (2 * nc + 1)) * m * sizeof(int64_t)); }
    const long long* eoff(size_t s) const { return i64() + s * m; }
    const long long* coff(size_t copy) const { return i64() + (nr + 2 * copy) * m; }
    const int* len(size_t j) const { return i32() + (3 * j) * m; }
    const int* base(size_t j) const { return i32() + (3 * j + 1) * m; }
    const int* alen(size_t j) const { return i32() + (3 * j + 2) * m; }
    const int* off1() const { return i32() + (3 * nc) * m; }
    const int* off2() const { return i32() + (3 * nc + 1) * m; }
    const int* frames() const { return i32() + (3 * nc + 2) * m; }
    const int* cnt(size_t copy) const { return i32() + (3 * nc + 3 + copy) * m; }
    const long long* code_map() const { return reinterpret_cast<const long long*>(dev + stream_rag_map_at(nc, nr, m)); }
};

struct StreamBase {
    mimi_engine* e = nullptr;
    int B = 0, K = 0, max_n = 0, cap = 0;
    std::vector<int64_t> pos;  // per slot: frames decoded / encoded since its last reset
    std::vector<char> failed;  // per slot: a step that listed it failed after it had touched the state: refuse until reset
    float* state = nullptr;  // one allocation: carries | k rings | v rings | RoPE cos | RoPE sin
    size_t state_bytes = 0, zero_bytes = 0;  // zero_bytes: the carries and rings, what reset clears
    std::vector<size_t> carry_off;           // floats: per carry, in the order of the table above
    std::vector<int> carry_h, carry_c;       // rows and channels of each
    float *kring = nullptr, *vring = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    size_t ring_layer = 0;       // floats of one layer's ring
    float* rope_host = nullptr;  // pinned: [cos | sin] of the step's rows (a slot step: of every item's, in step order)
    // a slot step's tables, [B] first rows (int64) then [B] slots (int32): the pinned image and its device copy
    char *tab_host = nullptr, *tab_dev = nullptr;
    // a ragged step's tables (StreamLayout: per stage the items' rows and first rows, the carry copies' offsets and
    // counts): the pinned image and its device copy, sized for B items
    char *rag_host = nullptr, *rag_dev = nullptr;
    size_t rag_bytes = 0;
    int64_t max_pos() const { return *std::max_element(pos.begin(), pos.end()); }
};
struct mimi_decode_stream : StreamBase {};

// The RoPE rows of a stream step by ensure_rope's expressions, into a pinned image: item b's rows 2 pos0[b] ..
// 2 pos0[b] + R - 1 at table rows b R .. (cs, sn: [items * R][head_dim / 2]).  Shared by the decode and the encode stream.
// frames (a ragged step; else null): item b has 2 frames[b] rows, at table rows 2 off[b] .. (off = the prefix sum)
static void stream_rope_rows(const mimi_config& c, const int64_t* pos0, int items, int R, float* cs, float* sn,
                             const int32_t* frames = nullptr) {
    const int half = c.head_dim / 2;
    for (int d = 0; d < half; ++d) {
        const float expo = (float)(2 * d) / (float)c.head_dim;
        const float pw = (float)std::pow((double)c.rope_theta, (double)expo);
        const float inv = 1.0f / pw;
        size_t row0 = 0;
        for (int b = 0; b < items; ++b) {
            const int64_t P = 2 * pos0[b];
            const int Rb = frames ? 2 * frames[b] : R;
            for (int i = 0; i < Rb; ++i) {
                volatile float fr = inv * (float)(P + i);
                cs[(row0 + i) * half + d] = (float)std::cos((double)fr);
                sn[(row0 + i) * half + d] = (float)std::sin((double)fr);
            }
            row0 += Rb;
        }
    }
}

// lays the state out for st->carry_h / carry_c (already planned) and allocates it, zeroed, with the pinned images
// (nr_up: the up convs of the stream's ragged step, whose tables' images the stream owns; code_map: with the RVQ's code
// map behind them, one entry per frame of a step)
static int stream_alloc(StreamBase* st, mimi_engine* e, const char* what, int batch, int K, int max_step_frames,
                        int nr_up, bool code_map) {
    const mimi_config& c = e->cfg;
    st->e = e;
    st->B = batch;
    st->K = K;
    st->max_n = max_step_frames;
    st->cap = c.sliding_window - 1 + 2 * max_step_frames;
    st->pos.assign(batch, 0);
    st->failed.assign(batch, 0);
    size_t off = 0;  // floats; every section a multiple of 64 floats
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 63) / 64 * 64;
        return at;
    };
    for (size_t i = 0; i < st->carry_h.size(); ++i)
        st->carry_off.push_back(take((size_t)batch * st->carry_h[i] * st->carry_c[i]));
    st->ring_layer = (size_t)batch * c.num_attention_heads * st->cap * c.head_dim;
    const size_t kr = take(st->ring_layer * c.num_hidden_layers), vr = take(st->ring_layer * c.num_hidden_layers);
    st->zero_bytes = off * sizeof(float);
    // the RoPE rows of every item of a slot step (at B = 1 the rows of the step, as before)
    const size_t rope_floats = (size_t)batch * 2 * max_step_frames * (c.head_dim / 2);
    const size_t tab_bytes = (size_t)batch * (sizeof(int64_t) + sizeof(int32_t));
    const size_t rc_ = take(rope_floats), rs_ = take(rope_floats);
    st->state_bytes = off * sizeof(float);
    st->rag_bytes = stream_rag_map_at(st->carry_h.size(), nr_up, batch) +
                    (code_map ? (size_t)batch * max_step_frames * sizeof(int64_t) : 0);
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&st->state), st->state_bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        st->state = nullptr;
        return set_err(err == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP,
                       "%s stream state hipMalloc(%zu bytes): %s", what, st->state_bytes, hipGetErrorString(err));
    }
    st->kring = st->state + kr;
    st->vring = st->state + vr;
    st->rope_cos = st->state + rc_;
    st->rope_sin = st->state + rs_;
    if ((err = hipMemset(st->state, 0, st->state_bytes)) != hipSuccess ||
        (err = hipHostMalloc(reinterpret_cast<void**>(&st->rope_host), 2 * rope_floats * sizeof(float),
                             hipHostMallocDefault)) != hipSuccess ||
        (err = hipHostMalloc(reinterpret_cast<void**>(&st->tab_host), tab_bytes, hipHostMallocDefault)) != hipSuccess ||
        (err = hipMalloc(reinterpret_cast<void**>(&st->tab_dev), tab_bytes)) != hipSuccess ||
        (st->rag_bytes &&
         ((err = hipHostMalloc(reinterpret_cast<void**>(&st->rag_host), st->rag_bytes, hipHostMallocDefault)) != hipSuccess ||
          (err = hipMalloc(reinterpret_cast<void**>(&st->rag_dev), st->rag_bytes)) != hipSuccess))) {
        (void)hipGetLastError();
        (void)hipFree(st->state);
        if (st->rope_host) (void)hipHostFree(st->rope_host);
        if (st->tab_host) (void)hipHostFree(st->tab_host);
        if (st->tab_dev) (void)hipFree(st->tab_dev);
        if (st->rag_host) (void)hipHostFree(st->rag_host);
        return set_err(MIMI_ERR_HIP, "%s stream state: %s", what, hipGetErrorString(err));
    }
    return MIMI_OK;
}

static void stream_free(StreamBase* st) {
    std::lock_guard<std::mutex> lk(st->e->mu);  // (every step has synchronised its stream before it returned)
    (void)hipSetDevice(st->e->device);
    if (st->state) (void)hipFree(st->state);
    if (st->rope_host) (void)hipHostFree(st->rope_host);
    if (st->tab_host) (void)hipHostFree(st->tab_host);
    if (st->tab_dev) (void)hipFree(st->tab_dev);
    if (st->rag_host) (void)hipHostFree(st->rag_host);
    if (st->rag_dev) (void)hipFree(st->rag_dev);
}

static int stream_reset_all(StreamBase* st) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    std::lock_guard<std::mutex> lk(st->e->mu);
    HIP_TRY(hipSetDevice(st->e->device));
    HIP_TRY(hipMemset(st->state, 0, st->zero_bytes));
    st->pos.assign(st->B, 0);
    st->failed.assign(st->B, 0);
    return MIMI_OK;
}

// One slot back to a fresh stream's: position 0 and zero carries.  Its rings keep their words: a query at row a reads
// ring rows [max(0, a - W + 1), pos0) only, and all of those are written again before they are read.
static int stream_reset_one(StreamBase* st, const char* what, int32_t slot) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    std::lock_guard<std::mutex> lk(st->e->mu);
    if (slot < 0 || slot >= st->B)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream: slot %d outside [0, %d)", what, slot, st->B);
    HIP_TRY(hipSetDevice(st->e->device));
    for (size_t i = 0; i < st->carry_h.size(); ++i) {
        const size_t hc = (size_t)st->carry_h[i] * st->carry_c[i];
        HIP_TRY(hipMemset(st->state + st->carry_off[i] + (size_t)slot * hc, 0, hc * sizeof(float)));
    }
    st->pos[slot] = 0;
    st->failed[slot] = 0;
    return MIMI_OK;
}

// The slot list of a step over all of the stream's slots: nullptr while they all stand at one position (the lock-step
// pass), otherwise 0 .. B - 1 (a slot step), kept in *all.
static const int32_t* stream_all_slots(const StreamBase* st, std::vector<int32_t>* all) {
    if (std::all_of(st->pos.begin(), st->pos.end(), [&](int64_t p) { return p == st->pos[0]; })) return nullptr;
    for (int b = 0; b < st->B; ++b) all->push_back(b);
    return all->data();
}

// the arguments of a slot step (the pointers apart): every table index is checked here -- the kernels index the rings
// and carries by slots[i] and read m entries
// frames (a ragged step; else null): per item, each in [1, n] (n = the caller's max_frames)
static int stream_check_slots(const StreamBase* st, const char* what, const int32_t* slots, int32_t m, int32_t n,
                              const int32_t* frames = nullptr) {
    if (m < 1 || m > st->B)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream step over %d slots outside [1, %d]", what, m, st->B);
    if (n < 1 || n > st->max_n)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream step of %d frames outside [1, %d]", what, n, st->max_n);
    for (int i = 0; frames && i < m; ++i)
        if (frames[i] < 1 || frames[i] > n)
            return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream step: item %d brings %d frames outside [1, %d]", what, i,
                           frames[i], n);
    std::vector<char> seen(st->B, 0);
    for (int i = 0; i < m; ++i) {
        if (slots[i] < 0 || slots[i] >= st->B)
            return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream: slot %d outside [0, %d)", what, slots[i], st->B);
        if (seen[slots[i]]) return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s stream: slot %d listed twice", what, slots[i]);
        seen[slots[i]] = 1;
    }
    return MIMI_OK;
}

// the listed slots' state before a step touches anything (slots == nullptr: all st->B in order)
static int stream_step_check(const StreamBase* st, const char* what, const int32_t* slots, int m, int n,
                             const int32_t* frames = nullptr) {
    auto slot_of = [&](int i) { return slots ? slots[i] : i; };
    for (int i = 0; i < m; ++i)
        if (st->failed[slot_of(i)])
            return set_err(MIMI_ERR_STATE, "%s stream: a step of slot %d failed; mimi_%s_stream_reset(_slot) first", what,
                           slot_of(i), what);
    // RoPE multiplies inv_freq by (float)row: exact only while the row fits float32's 24-bit significand
    for (int i = 0; i < m; ++i) {
        const int R = 2 * (frames ? frames[i] : n);  // a listed slot at its own count
        if (2 * st->pos[slot_of(i)] + R > (1LL << 24))
            return set_err(MIMI_ERR_UNSUPPORTED, "%s stream: row %lld no longer fits a float32 exactly", what,
                           (long long)(2 * st->pos[slot_of(i)] + R));
    }
    const int R = 2 * n;
    if (slots && (int64_t)m * R > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "%s stream: %d slots x %d rows exceed the 32-bit row range", what, m, R);
    return MIMI_OK;
}

// The pinned images of a step and their uploads on s (the previous step synchronised s before it returned: nothing
// reads them any more).  The tables: item i's first frame and its slot.  The RoPE rows: lock-step rows P .. P + R - 1, a
// slot step item i's rows 2 pos_i .. 2 pos_i + R - 1 at table rows i R ..  pos0: the items' first frames.  From here on
// a failure leaves the listed slots half-advanced: they are marked failed until stream_step_done.
// frames (a ragged step, slots set; else null): item i has 2 frames[i] RoPE rows, packed in step order.
static int stream_step_upload(StreamBase* st, const int32_t* slots, int m, int n, std::vector<int64_t>* pos0,
                              hipStream_t s, const int32_t* frames = nullptr) {
    const mimi_config& c = st->e->cfg;
    const int R = 2 * n, half = c.head_dim / 2;
    auto slot_of = [&](int i) { return slots ? slots[i] : i; };
    pos0->assign(m, 0);
    int64_t* row_img = reinterpret_cast<int64_t*>(st->tab_host);  // the kernels read positions in 25 Hz rows
    int32_t* slot_img = reinterpret_cast<int32_t*>(st->tab_host + (size_t)st->B * sizeof(int64_t));
    for (int i = 0; i < m; ++i) {
        (*pos0)[i] = st->pos[slot_of(i)];
        if (slots) {
            row_img[i] = 2 * (*pos0)[i];
            slot_img[i] = slots[i];
        }
    }
    const int items = slots ? m : 1;
    size_t rope_rows = (size_t)items * R;
    if (frames) {
        rope_rows = 0;
        for (int i = 0; i < m; ++i) rope_rows += 2 * (size_t)frames[i];
    }
    float* cs = st->rope_host;
    float* sn = cs + rope_rows * half;
    stream_rope_rows(c, pos0->data(), items, R, cs, sn, frames);
    for (int i = 0; i < m; ++i) st->failed[slot_of(i)] = 1;
    HIP_TRY(hipMemcpyAsync(st->rope_cos, cs, rope_rows * half * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st->rope_sin, sn, rope_rows * half * 4, hipMemcpyHostToDevice, s));
    if (slots) {
        // the device image holds [B] rows then [B] slots, the first m of each
        HIP_TRY(hipMemcpyAsync(st->tab_dev, row_img, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st->tab_dev + (size_t)st->B * sizeof(int64_t), slot_img, (size_t)m * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    }
    return MIMI_OK;
}

// the device tables of a step as the stream kernels' launchers take them: a slot step's, or nullptr for the lock-step
// kernels
struct StreamTabs {
    const long long* pos;
    const int* slot;
};
static StreamTabs stream_tabs(const StreamBase* st, bool slots) {
    if (!slots) return {nullptr, nullptr};
    return {reinterpret_cast<const long long*>(st->tab_dev),
            reinterpret_cast<const int*>(st->tab_dev + (size_t)st->B * sizeof(int64_t))};
}

static void stream_step_done(StreamBase* st, const int32_t* slots, int m, int n, const int32_t* frames = nullptr) {
    for (int i = 0; i < m; ++i) {
        const int b = slots ? slots[i] : i;
        st->failed[b] = 0;
        st->pos[b] += frames ? frames[i] : n;
    }
}


// the carries in stage order: upsample, decoder.layers.0, then per ratio (up conv, residual block), the last conv
static void stream_carry_plan(const mimi_config& c, std::vector<int>* h, std::vector<int>* ch) {
    h->assign(1, 1);
    ch->assign(1, c.hidden_size);
    h->push_back(c.kernel_size - 1);
    ch->push_back(c.hidden_size);
    int C = c.num_filters << c.num_ratios;
    for (int s = 0; s < c.num_ratios; ++s) {
        h->push_back(1);
        ch->push_back(C);
        C /= 2;
        h->push_back(2);
        ch->push_back(C);
    }
    h->push_back(c.last_kernel_size - 1);
    ch->push_back(C);
}

// the decode stream's stages in the order of its carries (stream_carry_plan), with their rates
static std::vector<StreamStage> stream_stages_decode(const mimi_config& c) {
    std::vector<int> h, ch;
    stream_carry_plan(c, &h, &ch);
    std::vector<StreamStage> st;
    int64_t f = 2;
    st.push_back({h[0], 1, ch[0]});  // the embedding in front of the upsample
    st.push_back({h[1], 2, ch[1]});  // the transformer output in front of decoder.layers.0
    for (int s = 0; s < c.num_ratios; ++s) {
        st.push_back({h[2 + 2 * s], f, ch[2 + 2 * s]});  // up conv s's ELU'd input
        f *= c.upsampling_ratios[s];
        st.push_back({h[3 + 2 * s], f, ch[3 + 2 * s]});  // its raw output, the residual block's input
    }
    st.push_back({h.back(), f, ch.back()});  // the last conv's ELU'd input
    return st;
}

// a step's workspace: flat-row buffers of the dequantizer and the transformer, then per stage its packed blocks (H m +
// f sum rows: [m][H + f n][C] when every item brings n frames).  B items, `sum` frames in all.
struct StreamWs {
    float *sums, *emb, *t0, *t1, *qkv, *att, *ff, *xin, *tap;
    std::vector<float*> xe, raw;  // xe[s]: ELU'd input of up conv s (xe[num_ratios]: of the last conv); raw[s]: its output
    size_t bytes;
};
static StreamWs stream_ws_layout(const mimi_config& c, void* ws, int B, int64_t sum, bool taps) {
    const size_t h = c.hidden_size, Bn = (size_t)sum;
    StreamWs w{};
    char* base = reinterpret_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t floats) {
        float* p = reinterpret_cast<float*>(base + off);
        off += pad256(floats * sizeof(float));
        return p;
    };
    const size_t BR = 2 * Bn;  // the 25 Hz rows of all items
    w.sums = take(Bn * 2 * c.vq_hidden_dim);
    w.emb = take(((size_t)B + Bn) * h);
    w.t0 = take(BR * h);
    w.t1 = take(BR * h);
    w.qkv = take(BR * 3 * c.num_attention_heads * c.head_dim);
    w.att = take(BR * h);
    w.ff = take(BR * c.intermediate_size);
    w.xin = take(((size_t)B * (c.kernel_size - 1) + BR) * h);
    size_t C = (size_t)c.num_filters << c.num_ratios, len = BR;
    w.tap = take(taps ? BR * C : 0);
    for (int s = 0; s < c.num_ratios; ++s) {
        w.xe.push_back(take(((size_t)B + len) * C));
        len *= c.upsampling_ratios[s];
        C /= 2;
        w.raw.push_back(take(((size_t)B * 2 + len) * C));
    }
    w.xe.push_back(take(((size_t)B * (c.last_kernel_size - 1) + len) * C));
    w.bytes = off;
    return w;
}

// The pinned image of a ragged decode step's tables (StreamRag) for the layout L and the listed slots.  Every offset is
// worked out here from L alone; before anything is written, every block is checked against its tensor (it ends where
// the next one starts, the last one at the tensor's end, inside the 32-bit row range), every row against the 16-byte
// copies (C a multiple of 4), every slot against the state and the stage list against the stream's carries.  The
// kernels index by nothing else.  *most: the largest count of any carry copy.
// dec: a decode stream (the transformer's rows are moved by a carry copy, the up convs take element offsets); else an
// encode stream (stage 0 is conv 0's 8 samples: no chunk rows, f = 0; K > 0 levels: the code map for rows of
// L.stride frames behind the image).
static int stream_rag_fill(const StreamBase* st, const StreamLayout& L, const int32_t* slots, char* img, int* most,
                           bool dec = true, int K = 0) {
    const size_t nc = L.st.size(), nr = dec ? st->e->cfg.num_ratios : 0, m = L.m;
    if (nc != st->carry_h.size() || nc != 3 + 2 * (size_t)st->e->cfg.num_ratios || !img || L.m < 1 || L.m > st->B ||
        stream_rag_map_at(nc, nr, m) + (dec ? 0 : (size_t)L.sum * sizeof(int64_t)) > st->rag_bytes)
        return set_err(MIMI_ERR_STATE, "stream: a ragged step's tables do not fit the stream");
    for (size_t j = 0; j < nc; ++j) {
        const StreamStage& g = L.st[j];
        if (g.C < 4 || g.C % 4 || g.H != st->carry_h[j] || g.C != st->carry_c[j] || g.f < ((dec || j) ? 1 : 0) ||
            L.rows(j) > 0x7fffffffLL)
            return set_err(MIMI_ERR_STATE, "decode stream: stage %zu of a ragged step (%d carry rows, %d channels)", j, g.H, g.C);
        for (int i = 0; i < L.m; ++i) {
            const int64_t end = L.base(j, i) + g.H + L.len(j, i);
            if (L.frames[i] < 1 || L.base(j, i) < 0 || end != (i + 1 < L.m ? L.base(j, i + 1) : L.rows(j)))
                return set_err(MIMI_ERR_STATE, "decode stream: item %d's block of stage %zu leaves its tensor", i, j);
        }
    }
    for (int i = 0; i < L.m; ++i)
        if (slots[i] < 0 || slots[i] >= st->B) return set_err(MIMI_ERR_STATE, "decode stream: slot %d", slots[i]);
    StreamRag r{img, nc, nr, m};
    long long* i64 = const_cast<long long*>(r.i64());
    int* i32 = const_cast<int*>(r.i32());
    auto coff = [&](size_t copy, int side, int i) -> long long& { return i64[(nr + 2 * copy + side) * m + i]; };
    auto cnt = [&](size_t copy, int i) -> int& { return i32[(3 * nc + 3 + copy) * m + i]; };
    *most = 0;
    for (int i = 0; i < L.m; ++i) {
        for (size_t j = 0; j < nc; ++j) {
            const int64_t C = L.st[j].C, H = L.st[j].H, hc = H * C;
            i32[(3 * j) * m + i] = (int)L.len(j, i);
            i32[(3 * j + 1) * m + i] = (int)L.base(j, i);
            i32[(3 * j + 2) * m + i] = (int)(H + L.len(j, i));
            // carry-in: the slot's rows of the state -> the head of the item's block; carry-out: the last H rows of the
            // item's own [carry | chunk] (also where the chunk is shorter than H) -> the slot's rows of the state
            coff(j, 0, i) = (int64_t)slots[i] * hc;
            coff(j, 1, i) = L.base(j, i) * C;
            coff(nc + 1 + j, 0, i) = (L.base(j, i) + L.len(j, i)) * C;
            coff(nc + 1 + j, 1, i) = (int64_t)slots[i] * hc;
            cnt(j, i) = cnt(nc + 1 + j, i) = (int)hc;
            *most = std::max(*most, (int)hc);
        }
        // decode: the transformer's flat rows behind decoder.layers.0's carry (stage 1)
        coff(nc, 0, i) = dec ? 2 * (int64_t)L.off[i] * L.st[1].C : 0;
        coff(nc, 1, i) = dec ? (L.base(1, i) + L.st[1].H) * L.st[1].C : 0;
        cnt(nc, i) = dec ? (int)(L.len(1, i) * L.st[1].C) : 0;
        *most = std::max(*most, cnt(nc, i));
        i32[(3 * nc) * m + i] = L.off[i];
        i32[(3 * nc + 1) * m + i] = 2 * L.off[i];
        i32[(3 * nc + 2) * m + i] = L.frames[i];
        for (size_t s = 0; s < nr; ++s) i64[s * m + i] = L.base(3 + 2 * s, i) * L.st[3 + 2 * s].C;
    }
    if (!dec) {  // packed frame off[i] + t -> codes[(i K + level) stride + t]
        long long* map = const_cast<long long*>(r.code_map());
        for (int i = 0; i < L.m; ++i)
            for (int t = 0; t < L.frames[i]; ++t) map[L.off[i] + t] = (int64_t)i * K * L.stride + t;
    }
    return MIMI_OK;
}

extern "C" int mimi_decode_stream_create(mimi_engine* e, int32_t batch, int32_t K, int32_t max_step_frames,
                                         mimi_decode_stream** out) {
    if (!e || !out) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine / out");
    *out = nullptr;
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_decode_state(e, K);
    if (rc) return rc;
    const mimi_config& c = e->cfg;
    if (batch <= 0 || batch > 65535 || max_step_frames < 1 || max_step_frames > (1 << 20))
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "batch=%d max_step_frames=%d", batch, max_step_frames);
    if (c.sliding_window < 1 || (size_t)4 * c.sliding_window * sizeof(float) > 64 * 1024)
        return set_err(MIMI_ERR_UNSUPPORTED, "decode stream: sliding_window %d", c.sliding_window);
    HIP_TRY(hipSetDevice(e->device));
    std::unique_ptr<mimi_decode_stream> st(new mimi_decode_stream);
    stream_carry_plan(c, &st->carry_h, &st->carry_c);
    if ((rc = stream_alloc(st.get(), e, "decode", batch, K, max_step_frames, c.num_ratios, false))) return rc;
    *out = st.release();
    return MIMI_OK;
}

extern "C" void mimi_decode_stream_destroy(mimi_decode_stream* st) {
    if (!st) return;
    stream_free(st);
    delete st;
}

extern "C" int mimi_decode_stream_reset(mimi_decode_stream* st) { return stream_reset_all(st); }

extern "C" int mimi_decode_stream_reset_slot(mimi_decode_stream* st, int32_t slot) {
    return stream_reset_one(st, "decode", slot);
}

// (the positions are only written under the engine mutex; a caller that reads them while another thread steps the
// stream sees one side or the other of that step, as before)
extern "C" int64_t mimi_decode_stream_position(const mimi_decode_stream* st) { return st ? st->max_pos() : -1; }

extern "C" int64_t mimi_decode_stream_slot_position(const mimi_decode_stream* st, int32_t slot) {
    return st && slot >= 0 && slot < st->B ? st->pos[slot] : -1;
}

extern "C" int64_t mimi_decode_stream_state_bytes(const mimi_decode_stream* st) {
    return st ? (int64_t)st->state_bytes : -1;
}

// a tap of a step: item b's `rows` rows of C floats start at src + b * bstride
static int save_tap_strided(mimi_engine* e, const char* name, const float* src, int64_t b, int64_t rows, int64_t ch,
                            int64_t bstride, hipStream_t s) {
    if (!e->taps) return MIMI_OK;
    if (bstride == rows * ch) return save_tap(e, name, src, b, rows, ch, s);
    float* d;
    int rc;
    if ((rc = tap_buffer(e, name, b, rows, ch, &d))) return rc;
    HIP_TRY(hipMemcpy2DAsync(d, (size_t)(rows * ch) * 4, src, (size_t)bstride * 4, (size_t)(rows * ch) * 4, (size_t)b,
                             hipMemcpyDeviceToDevice, s));
    return MIMI_OK;
}

// a tap of a ragged step's stage j (buf: its packed [carry | chunk] blocks): the items' chunks without their carry rows,
// packed [1][f sum][C] in step order as ragged decode's taps -- one device copy per item by the layout
static int save_tap_packed(mimi_engine* e, const char* name, const float* buf, const StreamLayout& L, size_t j,
                           hipStream_t s) {
    if (!e->taps) return MIMI_OK;
    const StreamStage& g = L.st[j];
    float* d;
    int rc;
    if ((rc = tap_buffer(e, name, 1, g.f * L.sum, g.C, &d))) return rc;
    for (int i = 0; i < L.m; ++i)
        HIP_TRY(hipMemcpyAsync(d + g.f * L.off[i] * g.C, buf + (L.base(j, i) + g.H) * g.C,
                               (size_t)(L.len(j, i) * g.C) * 4, hipMemcpyDeviceToDevice, s));
    return MIMI_OK;
}

// The two callables that make transformer_f32 the transformer section of a stream step, decode or encode: B items of
// R rows each, the step's RoPE rows in the stream's tables, the attention on the stream's rings.  pos_tab / slot_tab:
// the slot step's device tables, both nullptr in lock-step; pos0: per item (lock-step: [0] for all) the frame its first
// row belongs to.
// q/k/v.  Lock-step: batched, row m of an item is absolute row P + m and the tables hold rows P ..; slots: the flat
// rows, the tables hold every item's rows in step order
// (frows: the flat rows of all items, B R, or in a ragged step the sum of the items' rows)
static auto stream_qkv_args(const StreamBase* st, const float* t1, float* qkv, int B, int R, bool slots,
                            int64_t frows = 0) {
    const mimi_config& c = st->e->cfg;
    const int Hd = c.hidden_size, HD = c.num_attention_heads * c.head_dim;
    if (!frows) frows = (int64_t)B * R;
    return [=](const DevXfmr& x) {
        GemmArgs aq = linear_args(t1, slots ? frows : R, Hd, x.wqkv, 3 * HD, qkv);
        if (!slots) {
            aq.batch = B;
            aq.a_bstride = (int64_t)R * Hd;
            aq.c_bstride = (int64_t)R * 3 * HD;
        }
        aq.rope_cos = st->rope_cos;
        aq.rope_sin = st->rope_sin;
        aq.rope_cols = 2 * HD;
        return aq;
    };
}
// the attention on the rings, then the step's k / v rows into them
// (a ragged step: rlen / roff the items' rows and first rows in the packed qkv / att, frames the host's counts, R the
// longest item's rows)
static auto stream_attention(const StreamBase* st, const float* qkv, float* att, int B, int R, const int64_t* pos0,
                             const long long* pos_tab, const int* slot_tab, const char* prefix, Recorder& rec,
                             hipStream_t s, const int* rlen = nullptr, const int* roff = nullptr,
                             const int32_t* frames = nullptr) {
    const mimi_config& c = st->e->cfg;
    const int Hd = c.hidden_size, H = c.num_attention_heads, Dh = c.head_dim, W = c.sliding_window;
    const int64_t P = 2 * pos0[0];  // lock-step: the absolute 25 Hz row of the step's first
    int64_t frows = (int64_t)B * R;
    double att_flops = 0;
    for (int b = 0; b < (pos_tab ? B : 1); ++b)
        for (int i = 0; i < (frames ? 2 * frames[b] : R); ++i)
            att_flops += 4.0 * Dh * std::min<int64_t>(2 * pos0[b] + i + 1, W);
    att_flops *= (double)H * (pos_tab ? 1 : B);
    if (frames) {
        frows = 0;
        for (int b = 0; b < B; ++b) frows += 2 * (int64_t)frames[b];
    }
    const std::string pre(prefix);
    return [=, &rec](size_t l) {
        float* kr = st->kring + l * st->ring_layer;
        float* vr = st->vring + l * st->ring_layer;
        const char* kname = "?";
        const float sc = 1.0f / std::sqrt((float)Dh);
        if (rlen)
            LAUNCH_TRY(launch_attention_stream_ragged(qkv, kr, vr, att, B, R, H, Dh, W, st->cap, pos_tab, slot_tab, rlen,
                                                      roff, sc, s, &kname),
                       "attention (stream)");
        else
            LAUNCH_TRY(launch_attention_stream(qkv, kr, vr, att, B, R, H, Dh, W, st->cap, P, pos_tab, slot_tab, sc, s,
                                               &kname),
                       "attention (stream)");
        rec.mark(pre + "attention", att_flops, (double)frows * 4 * Hd * 4, kname);
        if (rlen)
            LAUNCH_TRY(launch_attention_stream_append_ragged(qkv, kr, vr, B, R, H, Dh, st->cap, pos_tab, slot_tab, rlen,
                                                             roff, s, &kname),
                       "kv append");
        else
            LAUNCH_TRY(launch_attention_stream_append(qkv, kr, vr, B, R, H, Dh, st->cap, P, pos_tab, slot_tab, s, &kname),
                       "kv append");
        rec.mark(pre + "kv_append", 0, (double)frows * 4 * H * Dh * 4, kname);
        return (int)MIMI_OK;
    };
}

// the launches of one step over B items (the workspace w sized for it, the step's RoPE rows already enqueued).
// slots == nullptr: the lock-step pass, B = st->B items that all stand at frame pos0[0].  Otherwise item i is slot
// slots[i] at frame pos0[i] (host copies of the tables already enqueued to st->tab_dev).
// L: the step's layout.  Equal counts (!L.ragged): everything below runs on the scalars n = L.maxn, exactly the lock-step
// / slot step.  Unequal counts (slots set, rg the tables' device image, carry_most the largest carry copy): the same
// launches in the same order, each in its ragged form -- the flat-row stages unchanged on the sum of the rows, the convs
// through the GEMM's packed-rows form, the per-item kernels with the item's rows and first row from the tables.
static int stream_pass(mimi_decode_stream* st, const int32_t* dev_codes, const StreamLayout& L, const StreamRag& rg,
                       int carry_most, const int32_t* slots, const int64_t* pos0, const StreamWs& w, float* dev_audio,
                       hipStream_t s) {
    mimi_engine* e = st->e;
    const mimi_config& c = e->cfg;
    const int B = L.m, n = (int)L.maxn;
    const bool RG = L.ragged;
    const int K = st->K, Hd = c.hidden_size, Dq = c.vq_hidden_dim;
    const int R = 2 * n, H0 = c.kernel_size - 1, HL = c.last_kernel_size - 1;
    const StreamTabs tabs = stream_tabs(st, slots != nullptr);
    const char* kname = "?";
    const size_t nc = L.st.size();
    // a carry launch: `copy` = its first copy in the ragged tables (carry-in 0, the transformer's rows nc, carry-out nc + 1)
    auto carry = [&](const CarryTable& t, size_t copy) {
        if (RG) return launch_stream_carry_ragged(t, B, rg.coff(copy), rg.cnt(copy), carry_most, s, &kname);
        return launch_stream_carry(t, B, tabs.slot, s, &kname);
    };
    int rc;
    HIP_TRY(hipMemsetAsync(e->dec_flag, 0, sizeof(unsigned), s));
    Recorder rec{e, s};
    rec.begin();
    char nm[64];
    // where each carry's rows sit in the workspace, in the order of stream_carry_plan: in front of the item's chunk
    std::vector<float*> where = {w.emb, w.xin};
    std::vector<int64_t> rows = {n, R};  // the chunk's rows behind each carry
    {
        int64_t len = R;
        for (int si = 0; si < c.num_ratios; ++si) {
            where.push_back(w.xe[si]);
            rows.push_back(len);
            len *= c.upsampling_ratios[si];
            where.push_back(w.raw[si]);
            rows.push_back(len);
        }
        where.push_back(w.xe[c.num_ratios]);
        rows.push_back(len);
    }
    CarryTable in{}, outc{};
    for (size_t i = 0; i < where.size(); ++i) {
        const int64_t hc = (int64_t)st->carry_h[i] * st->carry_c[i], bs = (st->carry_h[i] + rows[i]) * st->carry_c[i];
        in.c[i] = {st->state + st->carry_off[i], where[i], hc, bs, (int)hc, CARRY_STATE_SRC};
        outc.c[i] = {where[i] + rows[i] * st->carry_c[i], st->state + st->carry_off[i], bs, hc, (int)hc, CARRY_STATE_DST};
    }
    in.n = outc.n = (int)where.size();
    if (RG)  // the tables hold every offset from its tensor's first element
        for (size_t i = 0; i < where.size(); ++i) {
            in.c[i].dst = where[i];
            outc.c[i].src = where[i];
        }
    LAUNCH_TRY(carry(in, 0), "stream carry (in)");
    rec.mark("dec_carry", 0, 0, kname);

    // ---- quantizer.decode + upsample ----
    const int64_t Sn = L.sum, SR = 2 * L.sum;  // the frames and the 25 Hz rows of all items
    LAUNCH_TRY(launch_rvq_decode(dev_codes, (long long)B * L.stride, (int)L.stride, K, c.num_semantic_quantizers,
                                 c.codebook_size, c.codebook_dim, e->cb_rows, w.sums, e->dec_flag, s,
                                 RG ? rg.len(0) : nullptr, RG ? rg.off1() : nullptr, RG ? n : 0),
               "rvq_decode");
    rec.mark("dec_rvq", (double)Sn * K * Dq, (double)Sn * (K * Dq + 2 * Dq) * 4,
             RG ? "mimi::rvq_decode_ragged_kernel" : "mimi::rvq_decode_kernel");
    const int64_t emb_bs = (int64_t)(1 + n) * Hd;
    GemmArgs ap = linear_args(w.sums, n, 2 * Dq, e->outproj, Hd, w.emb + Hd);
    ap.batch = B;
    ap.a_bstride = (int64_t)n * 2 * Dq;
    ap.c_bstride = emb_bs;
    if (RG) {  // the packed sums -> each item's block of the embedding, behind its carry row
        ap.a_rows = ap.m_rows = rg.len(0);
        ap.a_boff = rg.off1();
        ap.c_boff = rg.base(0);
    }
    LAUNCH_TRY(launch_gemm(ROLE_INPROJ, ap, s, &kname, PREC_F32), "output_proj");
    rec.mark("dec_output_proj", 2.0 * Sn * 2 * Dq * Hd, (double)Sn * (2 * Dq + Hd) * 4, kname);
    if (RG) {
        LAUNCH_TRY(launch_upsample_dw_hist_ragged(w.emb + Hd, e->upsample_w, w.t0, B, n, Hd, rg.len(0), rg.off1(),
                                                  rg.base(0), s),
                   "upsample");
        rec.mark("dec_upsample", 4.0 * SR * Hd, 3.0 * Sn * Hd * 4, "mimi::upsample_dw_hist_ragged_kernel");
        if ((rc = save_tap_packed(e, "quantized", w.emb, L, 0, s))) return rc;
    } else {
        if ((rc = save_tap_strided(e, "quantized", w.emb + Hd, B, n, Hd, emb_bs, s))) return rc;
        LAUNCH_TRY(launch_upsample_dw_hist(w.emb + Hd, e->upsample_w, w.t0, B, n, Hd, emb_bs, s), "upsample");
        rec.mark("dec_upsample", 4.0 * B * R * Hd, 3.0 * B * n * Hd * 4, "mimi::upsample_dw_hist_kernel");
    }
    // (a ragged step's flat tensors are packed: tapped as one item of all rows, as ragged decode's)
    if ((rc = RG ? save_tap(e, "upsample", w.t0, 1, SR, Hd, s) : save_tap(e, "upsample", w.t0, B, R, Hd, s))) return rc;

    // ---- decoder transformer with the stream's RoPE rows and ring attention ----
    if ((rc = transformer_f32(e, e->dxf, w.t0, w.t1, w.qkv, w.att, w.ff, SR, RG ? 1 : B, RG ? SR : R, "dec_", rec, s,
                              stream_qkv_args(st, w.t1, w.qkv, B, R, slots != nullptr, SR),
                              stream_attention(st, w.qkv, w.att, B, R, pos0, tabs.pos, tabs.slot, "dec_", rec, s,
                                               RG ? rg.len(1) : nullptr, RG ? rg.off2() : nullptr,
                                               RG ? L.frames.data() : nullptr))))
        return rc;
    {  // the transformer's flat rows behind decoder.layers.0's carry
        CarryTable mv{};
        mv.c[0] = {w.t0, w.xin + (int64_t)H0 * Hd, (int64_t)R * Hd, (int64_t)(H0 + R) * Hd, R * Hd};
        if (RG) mv.c[0].dst = w.xin;
        mv.n = 1;
        LAUNCH_TRY(carry(mv, nc), "stream carry (transformer rows)");  // (no state side: by the item's place either way)
        rec.mark("dec_carry", 0, 2.0 * SR * Hd * 4, kname);
    }

    // ---- SEANet decoder ----
    // a conv over `len` rows per item whose input has hh carry rows in front: the carry is read where conv_args pads
    // (`len`: of the longest item, what the launch covers.)  A ragged step: stage `sin`'s blocks -> stage `sout`'s, the
    // item's rows and first rows from the tables; out already points behind the first block's carry rows
    auto conv = [&](const DevConv& cv, const float* in, int hh, int64_t len, float* out, int64_t out_bs, size_t sin,
                    size_t sout) {
        GemmArgs a = conv_args(cv, in, hh + len, out, len, B);
        a.a_off += (int64_t)hh * cv.cin;
        a.c_bstride = out_bs;
        if (RG) {
            a.a_rows = rg.alen(sin);
            a.a_boff = rg.base(sin);
            a.m_rows = rg.len(sin);
            a.c_boff = rg.base(sout);
        }
        return a;
    };
    // (B a.M = the rows of all items with equal counts; a ragged step's are stage sin's f times the sum of the counts)
    auto mrows = [&](const GemmArgs& a, size_t sin) { return RG ? (double)(L.st[sin].f * L.sum) : (double)B * a.M; };
    auto fl = [&](const GemmArgs& a, size_t sin) { return 2.0 * mrows(a, sin) * a.N * a.K; };
    auto by = [&](const GemmArgs& a, size_t sin) { return (mrows(a, sin) * (a.a_rs + a.N) + (double)a.N * a.K) * 4; };
    int C = c.num_filters << c.num_ratios;
    // a stage's tap: [B][rows][C] with equal counts, packed [1][f sum][C] in a ragged step (buf: the stage's tensor)
    auto tap_stage = [&](const char* name, const float* buf, size_t j) {
        const StreamStage& g = L.st[j];
        if (RG) return save_tap_packed(e, name, buf, L, j, s);
        return save_tap_strided(e, name, buf + (int64_t)g.H * g.C, B, g.f * n, g.C, (g.H + g.f * n) * g.C, s);
    };
    if (e->taps) {  // the raw layer-0 output (the pass itself only needs its ELU)
        GemmArgs at = conv(e->dec_first, w.xin, H0, R, w.tap, (int64_t)R * C, 1, 1);
        if (RG) at.c_boff = rg.off2();  // packed, no carry rows
        LAUNCH_TRY(launch_gemm(ROLE_DOWN, at, s, &kname, PREC_F32), "decoder conv 0 (tap)");
        rec.mark("dec_conv0_tap", fl(at, 1), by(at, 1), kname);
        if ((rc = RG ? save_tap(e, "dconv0", w.tap, 1, SR, C, s) : save_tap(e, "dconv0", w.tap, B, R, C, s))) return rc;
    }
    int64_t len = R;
    GemmArgs a0 = conv(e->dec_first, w.xin, H0, R, w.xe[0] + C, (1 + len) * C, 1, 2);
    LAUNCH_TRY(launch_gemm(ROLE_DOWN_ELU, a0, s, &kname, PREC_F32), "decoder conv 0");
    rec.mark("dec_conv0", fl(a0, 1), by(a0, 1), kname);
    if ((rc = tap_stage("dconv0_elu", w.xe[0], 2))) return rc;
    for (int si = 0; si < c.num_ratios; ++si) {
        const int r = c.upsampling_ratios[si], Co = C / 2;
        const int64_t olen = len * r;
        const size_t sx = 2 + 2 * si;  // the stage of the up conv's input; its output is sx + 1, the block's sx + 2
        // [len][C] -> [len][r * C/2] = [len * r][C/2], behind the residual block's 2 carry rows
        GemmArgs au = conv(e->dec_up[si], w.xe[si], 1, len, w.raw[si] + 2 * Co, (2 + olen) * Co, sx, sx + 1);
        if (RG) {  // a block of 2 + r len rows of Co starts at no multiple of the GEMM's r Co output row
            au.c_boff = nullptr;
            au.c_eoff = rg.eoff(si);
        }
        LAUNCH_TRY(launch_gemm(ROLE_UPCONV, au, s, &kname, PREC_F32), "up conv");
        snprintf(nm, sizeof nm, "dec_up_s%d", si);
        rec.mark(nm, fl(au, sx), by(au, sx), kname);
        snprintf(nm, sizeof nm, "up%d", si);
        if ((rc = tap_stage(nm, w.raw[si], sx + 1))) return rc;
        const int hn = si + 1 < c.num_ratios ? 1 : HL;  // the carry rows of the stage that reads this block's output
        ResArgs ra{};
        ra.x = w.raw[si] + 2 * Co;
        ra.T = olen;
        ra.batch = B;
        ra.w3 = e->dec_res3[si].w;
        ra.b3 = e->dec_res3[si].b;
        ra.w1 = e->dec_res1[si].w;
        ra.b1 = e->dec_res1[si].b;
        ra.y = w.xe[si + 1] + (int64_t)hn * Co;
        ra.hist = 2;
        ra.x_bstride = (2 + olen) * Co;
        ra.y_bstride = (hn + olen) * Co;
        if (RG) {
            ra.ilen = rg.len(sx + 1);
            ra.ioff = rg.base(sx + 1);
            ra.yoff = rg.base(sx + 2);
        }
        LAUNCH_TRY(launch_resblock(Co, ra, s, &kname), "decoder resblock");
        snprintf(nm, sizeof nm, "dec_res_s%d", si);
        const double Hh = Co / c.compress, orows = RG ? (double)(L.st[sx + 1].f * L.sum) : (double)B * olen;
        rec.mark(nm, 2.0 * orows * (3.0 * Co * Hh + Hh * Co), orows * 2 * Co * 4, kname);
        snprintf(nm, sizeof nm, "dres%d_elu", si);
        if ((rc = tap_stage(nm, w.xe[si + 1], sx + 2))) return rc;
        C = Co;
        len = olen;
    }
    if (RG) {  // the caller's padded rows: samples past an item's length are left alone
        const double lrows = (double)(L.st[nc - 1].f * L.sum);
        LAUNCH_TRY(launch_final_conv_hist_ragged(w.xe[c.num_ratios] + (int64_t)HL * C, e->dec_last.w, e->dec_last.b,
                                                 dev_audio, B, L.st[nc - 1].f * L.stride, C, c.last_kernel_size,
                                                 rg.len(nc - 1), rg.base(nc - 1), len, s),
                   "final conv");
        rec.mark("dec_final", 2.0 * lrows * C * c.last_kernel_size, lrows * (C + 1) * 4,
                 "mimi::final_conv_hist_ragged_kernel");
    } else {
        LAUNCH_TRY(launch_final_conv_hist(w.xe[c.num_ratios] + (int64_t)HL * C, e->dec_last.w, e->dec_last.b, dev_audio,
                                          B, len, C, c.last_kernel_size, (HL + len) * C, s),
                   "final conv");
        rec.mark("dec_final", 2.0 * B * len * C * c.last_kernel_size, (double)B * len * (C + 1) * 4,
                 "mimi::final_conv_hist_kernel");
    }
    LAUNCH_TRY(carry(outc, nc + 1), "stream carry (out)");
    rec.mark("dec_carry", 0, 0, kname);
    return MIMI_OK;
}

// One step over the m listed slots (slots == nullptr: all st->B in order, at one position: the lock-step pass).
// Called with the engine mutex held and every argument checked but the slots' state.
// frames (mimi_decode_stream_step_ragged; else null): item i advances by frames[i] <= n frames, the caller's rows hold n.
// Counts that are all n make the slot step itself: frames is dropped here and nothing below knows the difference.
static int stream_step_locked(mimi_decode_stream* st, const int32_t* slots, int m, const int32_t* dev_codes, int n,
                              float* dev_audio, hipStream_t s, const int32_t* frames = nullptr) {
    mimi_engine* e = st->e;
    int rc;
    if (frames && std::all_of(frames, frames + m, [&](int32_t f) { return f == n; })) frames = nullptr;
    if ((rc = stream_step_check(st, "decode", slots, m, n, frames))) return rc;
    StreamLayout L;
    plan_stream(stream_stages_decode(e->cfg), frames, m, n, &L);
    if (L.rows(L.st.size() - 1) > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "decode stream: %lld rows exceed the 32-bit row range",
                       (long long)L.rows(L.st.size() - 1));
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_dws(e, stream_ws_layout(e->cfg, nullptr, m, L.sum, e->taps).bytes))) return rc;  // (state untouched so far)
    const StreamWs w = stream_ws_layout(e->cfg, e->dws, m, L.sum, e->taps);
    std::vector<int64_t> pos0;  // frames
    // a ragged step's tables: built and checked before anything is enqueued or a slot is marked (the previous step
    // synchronised s before it returned: nothing reads the image any more)
    StreamRag rg{};
    int carry_most = 0;
    if (L.ragged && (rc = stream_rag_fill(st, L, slots, st->rag_host, &carry_most))) return rc;
    if ((rc = stream_step_upload(st, slots, m, n, &pos0, s, frames))) return rc;
    if (L.ragged) {
        const size_t bytes = stream_rag_bytes(L.st.size(), e->cfg.num_ratios, m);
        HIP_TRY(hipMemcpyAsync(st->rag_dev, st->rag_host, bytes, hipMemcpyHostToDevice, s));
        rg = StreamRag{st->rag_dev, L.st.size(), (size_t)e->cfg.num_ratios, (size_t)m};
    }
    if ((rc = stream_pass(st, dev_codes, L, rg, carry_most, slots, pos0.data(), w, dev_audio, s))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    if (L.ragged && e->taps) {  // the padded rows' valid samples, packed [1][1920 sum][1]
        const int64_t up = decode_upsampling(e->cfg);
        float* d;
        if ((rc = tap_buffer(e, "audio", 1, up * L.sum, 1, &d))) return rc;
        for (int i = 0; i < m; ++i)
            HIP_TRY(hipMemcpyAsync(d + up * L.off[i], dev_audio + (int64_t)i * up * n, (size_t)(up * L.frames[i]) * 4,
                                   hipMemcpyDeviceToDevice, s));
    } else if ((rc = save_tap(e, "audio", dev_audio, m, decode_upsampling(e->cfg) * n, 1, s))) {
        return rc;
    }
    if ((rc = read_decode_flag(e, s))) return rc;
    stream_step_done(st, slots, m, n, frames);
    return MIMI_OK;
}

extern "C" int mimi_decode_stream_step(mimi_decode_stream* st, const int32_t* dev_codes, int32_t n, float* dev_audio,
                                       void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    for (int b = 0; b < st->B; ++b)
        if (st->failed[b])
            return set_err(MIMI_ERR_STATE, "decode stream: a step of slot %d failed; mimi_decode_stream_reset(_slot) first", b);
    if (n < 1 || n > st->max_n || !dev_codes || !dev_audio)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "decode stream step of %d frames outside [1, %d]", n, st->max_n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> all;
    return stream_step_locked(st, stream_all_slots(st, &all), st->B, dev_codes, n, dev_audio, s);
}

extern "C" int mimi_decode_stream_step_slots(mimi_decode_stream* st, const int32_t* slots, int32_t m,
                                             const int32_t* dev_codes, int32_t n, float* dev_audio, void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!slots || !dev_codes || !dev_audio) return set_err(MIMI_ERR_INVALID_ARGUMENT, "decode stream step: null argument");
    int rc;
    if ((rc = stream_check_slots(st, "decode", slots, m, n))) return rc;
    return stream_step_locked(st, slots, m, dev_codes, n, dev_audio, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mimi_decode_stream_step_ragged(mimi_decode_stream* st, const int32_t* slots, const int32_t* frames,
                                              int32_t m, int32_t max_frames, const int32_t* dev_codes, float* dev_audio,
                                              void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!slots || !frames || !dev_codes || !dev_audio)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "decode stream step: null argument");
    int rc;
    if ((rc = stream_check_slots(st, "decode", slots, m, max_frames, frames))) return rc;
    return stream_step_locked(st, slots, m, dev_codes, max_frames, dev_audio, reinterpret_cast<hipStream_t>(stream),
                              frames);
}

static int encode_step_layout(const mimi_config& c, const int32_t* frames, int32_t m, int32_t max_frames,
                              std::vector<StreamStage>* st, StreamLayout* L, std::vector<int64_t>* byte_offset,
                              int64_t* bytes);  // (with the encode stream, below)
// The layout of a ragged step without a device: what stream_step_locked plans, from the configuration alone.
extern "C" int mimi_stream_step_layout(const mimi_config* cfg, int32_t direction, const int32_t* frames, int32_t m,
                                       int32_t max_frames, int32_t taps, int32_t* n_stages, int32_t* carry_rows,
                                       int32_t* rate, int32_t* channels, int64_t* byte_offset, int64_t* first_row,
                                       int64_t* row_count, int64_t* workspace_bytes) {
    if (!cfg || !frames || !n_stages || !carry_rows || !rate || !channels || !byte_offset || !first_row || !row_count ||
        !workspace_bytes)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: null argument");
    if (direction != MIMI_STREAM_DECODE && direction != MIMI_STREAM_ENCODE)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: direction %d", direction);
    if (m < 1 || m > 65535) return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout over %d items outside [1, 65535]", m);
    if (max_frames < 1 || max_frames > (1 << 20))
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: max_frames %d outside [1, 2^20]", max_frames);
    for (int i = 0; i < m; ++i)
        if (frames[i] < 1 || frames[i] > max_frames)
            return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: item %d brings %d frames outside [1, %d]", i,
                           frames[i], max_frames);
    // every field the stage list and the workspace are made of
    bool ok = cfg->num_ratios >= 1 && cfg->num_ratios <= 6 && cfg->hidden_size >= 4 && cfg->hidden_size <= (1 << 16) &&
              cfg->hidden_size % 4 == 0 && cfg->num_filters >= 4 && cfg->num_filters <= (1 << 12) &&
              cfg->num_filters % 4 == 0 && cfg->kernel_size >= 1 && cfg->kernel_size <= 64 &&
              cfg->last_kernel_size >= 1 && cfg->last_kernel_size <= 64 && cfg->vq_hidden_dim >= 1 &&
              cfg->vq_hidden_dim <= (1 << 16) && cfg->num_attention_heads >= 1 && cfg->num_attention_heads <= 4096 &&
              cfg->head_dim >= 1 && cfg->head_dim <= 4096 && cfg->intermediate_size >= 1 &&
              cfg->intermediate_size <= (1 << 20);
    for (int s = 0; ok && s < cfg->num_ratios; ++s) ok = cfg->upsampling_ratios[s] >= 1 && cfg->upsampling_ratios[s] <= 64;
    if (!ok)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: a configuration field outside the range a stream takes");
    if (direction == MIMI_STREAM_ENCODE) {
        std::vector<StreamStage> est;
        StreamLayout EL;
        std::vector<int64_t> at;
        int64_t bytes = 0;
        int rc;
        if ((rc = encode_step_layout(*cfg, frames, m, max_frames, &est, &EL, &at, &bytes))) return rc;
        if (est.size() > MIMI_STREAM_MAX_STAGES) return set_err(MIMI_ERR_UNSUPPORTED, "stream step layout: %zu stages", est.size());
        if (EL.rows(1) > 0x7fffffffLL || EL.rows(2) > 0x7fffffffLL)
            return set_err(MIMI_ERR_UNSUPPORTED, "stream step layout: %lld rows exceed the 32-bit row range", (long long)EL.rows(2));
        *n_stages = (int32_t)est.size();
        for (size_t j = 0; j < est.size(); ++j) {
            carry_rows[j] = est[j].H;
            rate[j] = (int32_t)est[j].f;
            channels[j] = est[j].C;
            byte_offset[j] = at[j];
            for (int i = 0; i < m; ++i) {
                first_row[j * m + i] = EL.base(j, i);
                row_count[j * m + i] = est[j].H + EL.len(j, i);
            }
        }
        *workspace_bytes = bytes;
        return MIMI_OK;
    }
    StreamLayout L;
    plan_stream(stream_stages_decode(*cfg), frames, m, max_frames, &L);
    const size_t nc = L.st.size();
    if (nc > MIMI_STREAM_MAX_STAGES) return set_err(MIMI_ERR_UNSUPPORTED, "stream step layout: %zu stages", nc);
    if (L.rows(nc - 1) > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "stream step layout: %lld rows exceed the 32-bit row range",
                       (long long)L.rows(nc - 1));
    const StreamWs w = stream_ws_layout(*cfg, nullptr, m, L.sum, taps != 0);
    std::vector<const float*> where = {w.emb, w.xin};
    for (int s = 0; s < cfg->num_ratios; ++s) {
        where.push_back(w.xe[s]);
        where.push_back(w.raw[s]);
    }
    where.push_back(w.xe[cfg->num_ratios]);
    *n_stages = (int32_t)nc;
    for (size_t j = 0; j < nc; ++j) {
        carry_rows[j] = L.st[j].H;
        rate[j] = (int32_t)L.st[j].f;
        channels[j] = L.st[j].C;
        byte_offset[j] = (int64_t)reinterpret_cast<uintptr_t>(where[j]);  // (laid out from a null base)
        for (int i = 0; i < m; ++i) {
            first_row[j * m + i] = L.base(j, i);
            row_count[j * m + i] = L.st[j].H + L.len(j, i);
        }
    }
    *workspace_bytes = (int64_t)w.bytes;
    return MIMI_OK;
}

// ================================================================================================
// encode stream (mimi_encode_stream_*): the encode pass n frames at a time on a KV cache.  DESIGN.md 3.7.2.
//
// Every stage of the encoder is causal and, fed whole frames (F = 1920 samples), every strided length divides exactly
// (F n -> 480 n -> 96 n -> 16 n -> 2 n -> 2 n -> n): no conv ever pads on the right.  So the codes of frames [p, p + n)
// depend on the past only through (per item) the rows each stage reads from in front of the chunk:
//   conv 0 (k = 7)         6 samples of audio (kept as the last 8: 16-byte copies)
//   residual block s       2 rows [C_s]    of its raw input (conv 0 / down conv s - 1 output)
//   down conv s            r_s rows [C_s]  of the block's ELU'd output (k = 2 r_s, stride r_s)
//   final conv (k = 3)     2 rows [1024]   of the ELU'd down conv 3 output
//   attention, per layer   the rotated k and v rows (P - W, P): the decode stream's ring, cap = W - 1 + 2 max_step_frames
//   downsample (k 4, s 2)  2 rows [hidden] of the transformer output
// All zero on a fresh or reset slot (causal padding is zero, ELU(0) = 0) but the downsample's: the reference pads it
// with copies of the sequence's FIRST ROW (F.pad(mode = "replicate"); MimiConv1dPaddingCache when streaming), so on a
// step that finds a slot at position 0 stream_ds_rows_kernel fills that slot's two carry rows from row 0 of the step's
// transformer output instead of the state -- per item, from the step's position (table), never from what a previous
// session left.  The downsample GEMM then reads its carry like every other conv and never reaches its replicate pad.
//
// The step runs in the engine's decode workspace (as a decode stream's does: used only between taking and leaving the
// engine mutex, every step synchronises its stream before it returns), on fp32 MFMA whatever mimi_set_precision says:
// no activation scales, no calibration, no lanes, no graphs.  Layout and carries as in the decode stream: every stage's
// tensor is per item [H carry rows | the chunk's rows]; one carry launch in front, one at the end.  The transformer
// section is transformer_f32 with the decode stream's callables; the RVQ runs the per-level kernels (the persistent
// chain needs its give-up flag read back: off here).  Slots as in the decode stream: what touches the state is
// indirected through slot_tab / pos_tab (the carry kernel, the attention and the append), the downsample fill reads
// pos_tab by the item's place, everything else works on the workspace by the item's place in the step.
// Profiling stages: encs_carry, encs_conv0, encs_res_s<s>, encs_down_s<s>, encs_final, encs_layernorm, encs_qkv,
// encs_attention, encs_kv_append, encs_o_proj, encs_fc1, encs_fc2, encs_ds_rows, encs_downsample, encs_input_proj, encs_rvq.
// ================================================================================================
struct mimi_encode_stream : StreamBase {
    int64_t F = 0;  // samples per frame
};

static int64_t frame_samples(const mimi_config& c) {
    int64_t f = c.downsample_stride;
    for (int i = 0; i < c.num_ratios; ++i) f *= c.upsampling_ratios[i];
    return f;
}

extern "C" int64_t mimi_frame_samples_cfg(const mimi_config* cfg) {
    mimi_config def;
    if (!cfg) {
        mimi_config_default(&def);
        cfg = &def;
    }
    if (cfg->num_ratios < 1 || cfg->num_ratios > 8) return -1;
    return frame_samples(*cfg);
}

// the encoder's ratio of stage s (the config lists the decoder's order)
static int enc_ratio(const mimi_config& c, int s) { return c.upsampling_ratios[c.num_ratios - 1 - s]; }

// the carries in stage order: conv 0, then per stage (residual block, down conv), the final conv, the downsample
static void enc_stream_carry_plan(const mimi_config& c, std::vector<int>* h, std::vector<int>* ch) {
    h->assign(1, 1);
    ch->assign(1, 8);
    int C = c.num_filters;
    for (int s = 0; s < c.num_ratios; ++s) {
        h->push_back(c.residual_kernel_size - 1);
        ch->push_back(C);
        h->push_back(enc_ratio(c, s));
        ch->push_back(C);
        C *= 2;
    }
    h->push_back(c.last_kernel_size - 1);
    ch->push_back(C);
    h->push_back(c.downsample_kernel - c.downsample_stride);
    ch->push_back(c.hidden_size);
}

// a step's workspace: per SEANet stage its [B][H + rows][C], then the flat-row buffers of the transformer and the rest
struct EncStreamWs {
    float *a_hist, *a_tail;       // [B][8]: conv 0's carry in, and the chunk's last 8 samples
    std::vector<float*> x, y;     // x[s]: raw input of block s behind its 2 carry rows; y[s]: its ELU'd output behind r_s
    float* xl;                    // ELU'd down conv 3 output behind the final conv's carry
    float *t0, *t1, *qkv, *att, *ff, *dsin, *dsout, *proj;
    void* rvq;
    size_t bytes;
    std::vector<size_t> at;  // every buffer's byte offset, in the order they are taken
};
// the encode stream's stages in the order of its carries (enc_stream_carry_plan), with their rates: conv 0's 8 samples
// (no chunk rows of its own: the audio stays in the caller's rows), then every [carry | chunk] tensor
static std::vector<StreamStage> stream_stages_encode(const mimi_config& c) {
    std::vector<int> h, ch;
    enc_stream_carry_plan(c, &h, &ch);
    std::vector<StreamStage> st;
    st.push_back({h[0], 0, ch[0]});
    int64_t f = frame_samples(c);
    for (int s = 0; s < c.num_ratios; ++s) {
        st.push_back({h[1 + 2 * s], f, ch[1 + 2 * s]});  // block s's raw input
        st.push_back({h[2 + 2 * s], f, ch[2 + 2 * s]});  // its ELU'd output, down conv s's input
        f /= enc_ratio(c, s);
    }
    st.push_back({h[h.size() - 2], f, ch[ch.size() - 2]});  // the final conv's input
    st.push_back({h.back(), f, ch.back()});                  // the downsample's input
    return st;
}

// B items, `sum` frames in all: every stage's tensor holds H B + f sum rows ([B][H + f n][C] when every item brings n)
static EncStreamWs enc_stream_ws_layout(const mimi_config& c, void* ws, int B, int64_t sum) {
    const size_t h = c.hidden_size, SR = 2 * (size_t)sum;
    EncStreamWs w{};
    // (sized before the workspace exists: without a base only the byte count is formed, no pointer)
    char* base = reinterpret_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t floats) {
        w.at.push_back(off);
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += pad256(floats * sizeof(float));
        return p;
    };
    w.a_hist = take((size_t)B * 8);
    w.a_tail = take((size_t)B * 8);
    size_t C = c.num_filters, len = (size_t)frame_samples(c) * sum;  // the rows of all items
    for (int s = 0; s < c.num_ratios; ++s) {
        w.x.push_back(take(((size_t)B * (c.residual_kernel_size - 1) + len) * C));
        w.y.push_back(take(((size_t)B * enc_ratio(c, s) + len) * C));
        len /= enc_ratio(c, s);
        C *= 2;
    }
    w.xl = take(((size_t)B * (c.last_kernel_size - 1) + len) * C);
    w.t0 = take(SR * h);
    w.t1 = take(SR * h);
    w.qkv = take(SR * 3 * c.num_attention_heads * c.head_dim);
    w.att = take(SR * h);
    w.ff = take(SR * c.intermediate_size);
    w.dsin = take(((size_t)B * (c.downsample_kernel - c.downsample_stride) + SR) * h);
    w.dsout = take((size_t)sum * h);
    w.proj = take((size_t)sum * 2 * c.vq_hidden_dim);
    w.rvq = base ? base + off : nullptr;
    off += pad256(rvq_work_bytes((long long)sum));
    w.bytes = off;
    return w;
}

extern "C" int mimi_encode_stream_create(mimi_engine* e, int32_t batch, int32_t K, int32_t max_step_frames,
                                         mimi_encode_stream** out) {
    if (!e || !out) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine / out");
    *out = nullptr;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->finalized) return set_err(MIMI_ERR_STATE, "mimi_finalize has not been called");
    const mimi_config& c = e->cfg;
    if (K <= 0) K = c.num_quantizers;
    if (K > c.num_quantizers || K < c.num_semantic_quantizers)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "num_quantizers %d outside [%d, %d]", K, c.num_semantic_quantizers,
                       c.num_quantizers);
    if (K > e->levels_available)
        return set_err(MIMI_ERR_WEIGHTS, "num_quantizers %d but the checkpoint has %d codebooks", K, e->levels_available);
    if (batch <= 0 || batch > 65535 || max_step_frames < 1 || max_step_frames > (1 << 15))
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "batch=%d max_step_frames=%d", batch, max_step_frames);
    if (c.sliding_window < 1 || (size_t)4 * c.sliding_window * sizeof(float) > 64 * 1024)
        return set_err(MIMI_ERR_UNSUPPORTED, "encode stream: sliding_window %d", c.sliding_window);
    // the history kernels' shapes: conv 0 as launch_conv0 takes it, k = 3 / k = 1 blocks, a k = 4 / stride 2 downsample
    if (c.num_filters != 64 || c.kernel_size != 7 || c.residual_kernel_size != 3 || c.compress != 2 ||
        c.downsample_kernel != 4 || c.downsample_stride != 2 || c.last_kernel_size < 2 || c.num_ratios > 4 ||
        c.num_attention_heads * c.head_dim != c.hidden_size)
        return set_err(MIMI_ERR_UNSUPPORTED, "encode stream: a config outside the kyutai/mimi shapes");
    HIP_TRY(hipSetDevice(e->device));
    std::unique_ptr<mimi_encode_stream> st(new mimi_encode_stream);
    st->F = frame_samples(c);
    enc_stream_carry_plan(c, &st->carry_h, &st->carry_c);
    int rc;
    if ((rc = stream_alloc(st.get(), e, "encode", batch, K, max_step_frames, 0, true))) return rc;
    *out = st.release();
    return MIMI_OK;
}

extern "C" void mimi_encode_stream_destroy(mimi_encode_stream* st) {
    if (!st) return;
    stream_free(st);
    delete st;
}

extern "C" int mimi_encode_stream_reset(mimi_encode_stream* st) { return stream_reset_all(st); }

// (the downsample's carry is zeroed with the others: the slot's first step fills it from its own first row whatever it
// holds)
extern "C" int mimi_encode_stream_reset_slot(mimi_encode_stream* st, int32_t slot) {
    return stream_reset_one(st, "encode", slot);
}

extern "C" int64_t mimi_encode_stream_position(const mimi_encode_stream* st) { return st ? st->max_pos() : -1; }

extern "C" int64_t mimi_encode_stream_slot_position(const mimi_encode_stream* st, int32_t slot) {
    return st && slot >= 0 && slot < st->B ? st->pos[slot] : -1;
}

extern "C" int64_t mimi_encode_stream_state_bytes(const mimi_encode_stream* st) {
    return st ? (int64_t)st->state_bytes : -1;
}

// the launches of one step over B items (the workspace w sized for it, the step's RoPE rows and tables already
// enqueued).  slots == nullptr: the lock-step pass, B = st->B items that all stand at frame pos0[0].  Otherwise item i
// is slot slots[i] at frame pos0[i].
// LY: the step's layout (StreamLayout, stream_stages_encode).  Equal counts (!LY.ragged): everything runs on the scalars
// n = LY.maxn, exactly the lock-step / slot step.  Unequal counts (slots set, rg the tables' device image, carry_most the
// largest carry copy): the same launches in the same order, each in its ragged form, as the decode stream's.
static int encode_stream_pass(mimi_encode_stream* st, const float* dev_audio, const StreamLayout& LY, const StreamRag& rg,
                              int carry_most, const int32_t* slots, const int64_t* pos0, const EncStreamWs& w,
                              int32_t* dev_codes, hipStream_t s) {
    mimi_engine* e = st->e;
    const mimi_config& c = e->cfg;
    const int B = LY.m, n = (int)LY.maxn;
    const bool RG = LY.ragged;
    const size_t nc = LY.st.size();
    const int64_t Sn = LY.sum, SR = 2 * LY.sum;  // the frames and the 25 Hz rows of all items
    const int K = st->K, Hd = c.hidden_size, Dq = c.vq_hidden_dim;
    const int R = 2 * n, HR = c.residual_kernel_size - 1, HL = c.last_kernel_size - 1;
    const int HD = c.downsample_kernel - c.downsample_stride;
    const int64_t L = st->F * n;
    const StreamTabs tabs = stream_tabs(st, slots != nullptr);
    const char* kname = "?";
    auto carry = [&](const CarryTable& t, size_t copy) {
        if (RG) return launch_stream_carry_ragged(t, B, rg.coff(copy), rg.cnt(copy), carry_most, s, &kname);
        return launch_stream_carry(t, B, tabs.slot, s, &kname);
    };
    int rc;
    Recorder rec{e, s};
    rec.begin();
    char nm[64];
    // where each carry's rows sit in the workspace, in the order of enc_stream_carry_plan: in front of the item's chunk
    // (conv 0's apart: in from a_hist, out from a_tail, which conv0_hist_kernel fills)
    std::vector<float*> where = {nullptr};
    std::vector<int64_t> rows = {0};  // the chunk's rows behind each carry
    {
        int64_t len = L;
        for (int si = 0; si < c.num_ratios; ++si) {
            where.push_back(w.x[si]);
            rows.push_back(len);
            where.push_back(w.y[si]);
            rows.push_back(len);
            len /= enc_ratio(c, si);
        }
        where.push_back(w.xl);
        rows.push_back(len);
        where.push_back(w.dsin);
        rows.push_back(len);
    }
    if (where.size() != st->carry_h.size() || where.size() > (size_t)CARRY_MAX)
        return set_err(MIMI_ERR_STATE, "encode stream: %zu carries", where.size());
    CarryTable in{}, outc{};
    in.c[0] = {st->state + st->carry_off[0], w.a_hist, 8, 8, 8, CARRY_STATE_SRC};
    outc.c[0] = {w.a_tail, st->state + st->carry_off[0], 8, 8, 8, CARRY_STATE_DST};
    for (size_t i = 1; i < where.size(); ++i) {
        const int64_t hc = (int64_t)st->carry_h[i] * st->carry_c[i], bs = (st->carry_h[i] + rows[i]) * st->carry_c[i];
        in.c[i] = {st->state + st->carry_off[i], where[i], hc, bs, (int)hc, CARRY_STATE_SRC};
        outc.c[i] = {where[i] + rows[i] * st->carry_c[i], st->state + st->carry_off[i], bs, hc, (int)hc, CARRY_STATE_DST};
    }
    in.n = outc.n = (int)where.size();
    if (RG)  // the tables hold every offset from its tensor's first element
        for (size_t i = 1; i < where.size(); ++i) outc.c[i].src = where[i];
    LAUNCH_TRY(carry(in, 0), "encode stream carry (in)");
    rec.mark("encs_carry", 0, 0, kname);
    // a stage's tap: [B][rows][C] with equal counts, packed [1][f sum][C] in a ragged step (buf: the stage's tensor)
    auto tap_stage = [&](const char* name, const float* buf, size_t j) {
        const StreamStage& g = LY.st[j];
        if (RG) return save_tap_packed(e, name, buf, LY, j, s);
        return save_tap_strided(e, name, buf + (int64_t)g.H * g.C, B, g.f * n, g.C, (g.H + g.f * n) * g.C, s);
    };
    auto tap_flat = [&](const char* name, const float* src, int64_t f, int64_t ch) {  // a flat tensor of f rows per frame
        return RG ? save_tap(e, name, src, 1, f * Sn, ch, s) : save_tap(e, name, src, B, f * n, ch, s);
    };

    // ---- SEANet encoder ----
    int C = c.num_filters;
    int64_t len = L;
    if (RG) {  // the caller's padded rows: nothing past an item's samples is read
        LAUNCH_TRY(launch_conv0_hist_ragged(dev_audio, st->F * LY.stride, L, B, e->conv0.w, e->conv0.b,
                                            w.x[0] + (int64_t)HR * C, C, c.kernel_size, w.a_hist, w.a_tail, rg.len(1),
                                            rg.base(1), s),
                   "conv0 (history)");
        rec.mark("encs_conv0", 2.0 * st->F * Sn * C * c.kernel_size, (double)st->F * Sn * (1 + C) * 4,
                 "mimi::conv0_hist_ragged_kernel<64, 7>");
    } else {
        LAUNCH_TRY(launch_conv0_hist(dev_audio, L, B, e->conv0.w, e->conv0.b, w.x[0] + (int64_t)HR * C, C,
                                     c.kernel_size, (HR + len) * C, w.a_hist, w.a_tail, s),
                   "conv0 (history)");
        rec.mark("encs_conv0", 2.0 * B * len * C * c.kernel_size, (double)B * len * (1 + C) * 4,
                 "mimi::conv0_hist_kernel<64, 7>");
    }
    if ((rc = tap_stage("conv0", w.x[0], 1))) return rc;
    // a conv over olen output rows per item whose input has hh carry rows in front of its ilen rows: the carry is
    // read where conv_args pads
    // A ragged step: stage sin's blocks -> olens / obase, the items' output rows and first output rows (device tables)
    auto conv = [&](const DevConv& cv, const float* inp, int hh, int64_t ilen, float* out, int64_t olen, int64_t out_bs,
                    size_t sin, const int* olens, const int* obase) {
        GemmArgs a = conv_args(cv, inp, hh + ilen, out, olen, B);
        a.a_off += (int64_t)hh * cv.cin;
        a.c_bstride = out_bs;
        if (RG) {
            a.a_rows = rg.alen(sin);
            a.a_boff = rg.base(sin);
            a.m_rows = olens;
            a.c_boff = obase;
        }
        return a;
    };
    // (B a.M = the output rows of all items with equal counts; orows: a ragged step's)
    auto fl = [&](const GemmArgs& a, double orows) { return 2.0 * (RG ? orows : (double)B * a.M) * a.N * a.K; };
    auto by = [&](const GemmArgs& a, double orows) {
        return ((RG ? orows : (double)B * a.M) * (a.a_rs + a.N) + (double)a.N * a.K) * 4;
    };
    for (int si = 0; si < c.num_ratios; ++si) {
        const int r = enc_ratio(c, si);
        const bool last = si == c.num_ratios - 1;
        if (e->down[si].k != 2 * r || e->down[si].stride != r || len % r)
            return set_err(MIMI_ERR_UNSUPPORTED, "encode stream: down conv %d is not k = 2 r, stride r", si);
        ResArgs ra{};
        ra.x = w.x[si] + (int64_t)HR * C;
        ra.T = len;
        ra.batch = B;
        ra.w3 = e->res3[si].w;
        ra.b3 = e->res3[si].b;
        ra.w1 = e->res1[si].w;
        ra.b1 = e->res1[si].b;
        ra.y = w.y[si] + (int64_t)r * C;
        ra.hist = 2;
        ra.x_bstride = (HR + len) * C;
        ra.y_bstride = (r + len) * C;
        const size_t sx = 1 + 2 * si;  // the stage of the block's input; its output is sx + 1, the down conv's sx + 2
        if (RG) {
            ra.ilen = rg.len(sx);
            ra.ioff = rg.base(sx);
            ra.yoff = rg.base(sx + 1);
        }
        LAUNCH_TRY(launch_resblock(C, ra, s, &kname), "encoder resblock (history)");
        snprintf(nm, sizeof nm, "encs_res_s%d", si);
        const double Hh = C / c.compress, rrows = RG ? (double)(LY.st[sx].f * Sn) : (double)B * len;
        rec.mark(nm, 2.0 * rrows * (3.0 * C * Hh + Hh * C), rrows * 2 * C * 4, kname);
        snprintf(nm, sizeof nm, "res%d_elu", si);
        if ((rc = tap_stage(nm, w.y[si], sx + 1))) return rc;
        // [r + len][C] -> [len / r][2 C], behind the next block's (the final conv's) carry rows
        const int64_t olen = len / r;
        const int hn = last ? HL : HR;
        float* obuf = last ? w.xl : w.x[si + 1];
        float* out = obuf + (int64_t)hn * 2 * C;
        GemmArgs ad = conv(e->down[si], w.y[si], r, len, out, olen, (hn + olen) * 2 * C, sx + 1, RG ? rg.len(sx + 2) : nullptr,
                           RG ? rg.base(sx + 2) : nullptr);
        LAUNCH_TRY(launch_gemm(last ? ROLE_DOWN_ELU : ROLE_DOWN, ad, s, &kname, PREC_F32), "down conv");
        snprintf(nm, sizeof nm, "encs_down_s%d", si);
        rec.mark(nm, fl(ad, (double)(LY.st[sx + 2].f * Sn)), by(ad, (double)(LY.st[sx + 2].f * Sn)), kname);
        snprintf(nm, sizeof nm, last ? "down%d_elu" : "down%d", si);
        if ((rc = tap_stage(nm, obuf, sx + 2))) return rc;
        C *= 2;
        len = olen;
    }
    if (len != R) return set_err(MIMI_ERR_STATE, "encode stream: %lld rows for %d frames", (long long)len, n);
    // (a ragged step: the final conv's output is the packed flat rows, item i's at row 2 off[i])
    GemmArgs af = conv(e->final_conv, w.xl, HL, R, w.t0, R, (int64_t)R * Hd, nc - 2, RG ? rg.len(nc - 2) : nullptr,
                       RG ? rg.off2() : nullptr);
    LAUNCH_TRY(launch_gemm(ROLE_FINAL, af, s, &kname, PREC_F32), "final conv");
    rec.mark("encs_final", fl(af, (double)SR), by(af, (double)SR), kname);
    if ((rc = tap_flat("encoder", w.t0, 2, Hd))) return rc;

    // ---- encoder transformer on the stream's rings ----
    if ((rc = transformer_f32(e, e->xf, w.t0, w.t1, w.qkv, w.att, w.ff, SR, RG ? 1 : B, RG ? SR : R, "encs_", rec, s,
                              stream_qkv_args(st, w.t1, w.qkv, B, R, slots != nullptr, SR),
                              stream_attention(st, w.qkv, w.att, B, R, pos0, tabs.pos, tabs.slot, "encs_", rec, s,
                                               RG ? rg.len(nc - 1) : nullptr, RG ? rg.off2() : nullptr,
                                               RG ? LY.frames.data() : nullptr))))
        return rc;
    // ---- downsample behind its carry (a slot at position 0: two copies of its first row) + projections + RVQ ----
    if (RG)  // (the replicate fill is per item: from its own position and its own first row)
        LAUNCH_TRY(launch_stream_ds_rows_ragged(w.t0, w.dsin, B, R, Hd, tabs.pos, rg.len(nc - 1), rg.off2(),
                                                rg.base(nc - 1), s, &kname),
                   "downsample rows");
    else
        LAUNCH_TRY(launch_stream_ds_rows(w.t0, w.dsin, B, R, Hd, 2 * pos0[0], tabs.pos, s, &kname), "downsample rows");
    rec.mark("encs_ds_rows", 0, 2.0 * SR * Hd * 4, kname);
    GemmArgs ad = conv(e->ds, w.dsin, HD, R, w.dsout, n, (int64_t)n * Hd, nc - 1, RG ? rg.frames() : nullptr,
                       RG ? rg.off1() : nullptr);
    LAUNCH_TRY(launch_gemm(ROLE_DOWNSAMPLE, ad, s, &kname, PREC_F32), "downsample");
    rec.mark("encs_downsample", fl(ad, (double)Sn), by(ad, (double)Sn), kname);
    if ((rc = tap_flat("downsample", w.dsout, 1, Hd))) return rc;
    GemmArgs ap = linear_args(w.dsout, Sn, Hd, e->inproj, 2 * Dq, w.proj);
    LAUNCH_TRY(launch_gemm(ROLE_INPROJ, ap, s, &kname, PREC_F32), "input_proj");
    rec.mark("encs_input_proj", 2.0 * Sn * Hd * 2 * Dq, ((double)Sn * (Hd + 2 * Dq) + 2.0 * Dq * Hd) * 4, kname);
    if ((rc = tap_flat("proj", w.proj, 1, 2 * Dq))) return rc;
    {
        RvqArgs r{};
        r.work = w.rvq;
        r.proj = w.proj;
        r.frames = Sn;
        r.D = c.codebook_dim;
        r.ncodes = c.codebook_size;
        r.levels = K;
        r.nsem = c.num_semantic_quantizers;
        r.cb_frag = e->cb_frag;
        r.cb_rows = e->cb_rows;
        r.cb_norm = e->cb_norm;
        r.cb_h16 = e->cb_h16;
        r.cb_unscale = e->cb_unscale;
        r.cb_emax = e->cb_emax;
        r.codes = dev_codes;
        r.frames_per_item = n;
        if (RG) {  // the packed frames' codes go to the caller's padded [m][K][stride]; entries past an item's are left alone
            r.code_map = rg.code_map();
            r.code_stride = (int)LY.stride;
        }
        r.form = e->rvq_form;
        r.chain = 0;  // the per-level kernels: nobody reads a give-up flag back here
        r.xcd_group_ok = e->rvq_xcd;
        LAUNCH_TRY(launch_rvq(r, s, &kname, nullptr, nullptr), "rvq");
        rec.mark("encs_rvq", 2.0 * Sn * r.D * r.ncodes * K, (double)Sn * (2 * r.D + K) * 4, kname);
    }
    LAUNCH_TRY(carry(outc, nc + 1), "encode stream carry (out)");
    rec.mark("encs_carry", 0, 0, kname);
    return MIMI_OK;
}

// One step over the m listed slots (slots == nullptr: all st->B in order, at one position: the lock-step pass).
// Called with the engine mutex held and every argument checked but the slots' state.
// frames (mimi_encode_stream_step_ragged; else null): item i advances by frames[i] <= n frames, the caller's rows hold n.
// Counts that are all n make the slot step itself: frames is dropped here and nothing below knows the difference.
static int encode_stream_step_locked(mimi_encode_stream* st, const int32_t* slots, int m, const float* dev_audio, int n,
                                     int32_t* dev_codes, hipStream_t s, const int32_t* frames = nullptr) {
    mimi_engine* e = st->e;
    int rc;
    if (frames && std::all_of(frames, frames + m, [&](int32_t f) { return f == n; })) frames = nullptr;
    if ((rc = stream_step_check(st, "encode", slots, m, n, frames))) return rc;
    if (st->F * n > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "encode stream: %d frames exceed the 32-bit row range", n);
    StreamLayout LY;
    plan_stream(stream_stages_encode(e->cfg), frames, m, n, &LY);
    if (LY.rows(1) > 0x7fffffffLL || LY.rows(2) > 0x7fffffffLL)
        return set_err(MIMI_ERR_UNSUPPORTED, "encode stream: %lld rows exceed the 32-bit row range", (long long)LY.rows(2));
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_dws(e, enc_stream_ws_layout(e->cfg, nullptr, m, LY.sum).bytes))) return rc;  // (state untouched so far)
    const EncStreamWs w = enc_stream_ws_layout(e->cfg, e->dws, m, LY.sum);
    // a ragged step's tables: built and checked before anything is enqueued or a slot is marked
    StreamRag rg{};
    int carry_most = 0;
    if (LY.ragged && (rc = stream_rag_fill(st, LY, slots, st->rag_host, &carry_most, false, st->K))) return rc;
    std::vector<int64_t> pos0;  // frames
    if ((rc = stream_step_upload(st, slots, m, n, &pos0, s, frames))) return rc;
    if (LY.ragged) {
        const size_t bytes = stream_rag_map_at(LY.st.size(), 0, m) + (size_t)LY.sum * sizeof(int64_t);
        HIP_TRY(hipMemcpyAsync(st->rag_dev, st->rag_host, bytes, hipMemcpyHostToDevice, s));
        rg = StreamRag{st->rag_dev, LY.st.size(), 0, (size_t)m};
    }
    rc = encode_stream_pass(st, dev_audio, LY, rg, carry_most, slots, pos0.data(), w, dev_codes, s);
    // the workspace and the pinned images are free for the next call under the mutex, whatever its stream
    const hipError_t se = hipStreamSynchronize(s);
    if (rc) return rc;
    if (se != hipSuccess) return set_err(MIMI_ERR_HIP, "encode stream step: %s", hipGetErrorString(se));
    stream_step_done(st, slots, m, n, frames);
    return MIMI_OK;
}

extern "C" int mimi_encode_stream_step(mimi_encode_stream* st, const float* dev_audio, int32_t n, int32_t* dev_codes,
                                       void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!dev_audio || !dev_codes) return set_err(MIMI_ERR_INVALID_ARGUMENT, "encode stream step: null argument");
    if (n < 1 || n > st->max_n)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "encode stream step of %d frames outside [1, %d]", n, st->max_n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> all;
    return encode_stream_step_locked(st, stream_all_slots(st, &all), st->B, dev_audio, n, dev_codes, s);
}

extern "C" int mimi_encode_stream_step_slots(mimi_encode_stream* st, const int32_t* slots, int32_t m,
                                             const float* dev_audio, int32_t n, int32_t* dev_codes, void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!slots || !dev_audio || !dev_codes) return set_err(MIMI_ERR_INVALID_ARGUMENT, "encode stream step: null argument");
    int rc;
    if ((rc = stream_check_slots(st, "encode", slots, m, n))) return rc;
    return encode_stream_step_locked(st, slots, m, dev_audio, n, dev_codes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mimi_encode_stream_step_ragged(mimi_encode_stream* st, const int32_t* slots, const int32_t* frames,
                                              int32_t m, int32_t max_frames, const float* dev_audio, int32_t* dev_codes,
                                              void* stream) {
    if (!st) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    mimi_engine* e = st->e;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!slots || !frames || !dev_audio || !dev_codes)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "encode stream step: null argument");
    int rc;
    if ((rc = stream_check_slots(st, "encode", slots, m, max_frames, frames))) return rc;
    return encode_stream_step_locked(st, slots, m, dev_audio, max_frames, dev_codes,
                                     reinterpret_cast<hipStream_t>(stream), frames);
}

// the encode half of mimi_stream_step_layout (arguments checked there)
static int encode_step_layout(const mimi_config& c, const int32_t* frames, int32_t m, int32_t max_frames,
                              std::vector<StreamStage>* st, StreamLayout* L, std::vector<int64_t>* byte_offset,
                              int64_t* bytes) {
    if (c.residual_kernel_size < 1 || c.residual_kernel_size > 64 || c.downsample_kernel < c.downsample_stride ||
        c.downsample_stride < 1 || c.downsample_kernel > 64)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "stream step layout: a configuration field outside the range a stream takes");
    *st = stream_stages_encode(c);
    plan_stream(*st, frames, m, max_frames, L);
    const EncStreamWs w = enc_stream_ws_layout(c, nullptr, m, L->sum);
    const size_t nr = c.num_ratios;
    byte_offset->assign(1, (int64_t)w.at[0]);  // conv 0's carry in; then x[s], y[s] ..., the final conv's, the downsample's
    for (size_t j = 0; j < 2 * nr + 1; ++j) byte_offset->push_back((int64_t)w.at[2 + j]);
    byte_offset->push_back((int64_t)w.at[2 + 2 * nr + 1 + 5]);
    *bytes = (int64_t)w.bytes;
    return MIMI_OK;
}

extern "C" void mimi_destroy(mimi_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    // this engine's work only (every encode ends with ws_free on its stream; a device-wide sync would wait for
    // other engines and is refused while one of them captures a graph)
    drain_lanes(e);
    for (auto& q : e->pend)
        if (q.id && q.done) (void)hipEventSynchronize(q.done);
    for (void* p : e->allocations) (void)hipFree(p);
    if (e->rope_cos) (void)hipFree(e->rope_cos);
    if (e->rope_sin) (void)hipFree(e->rope_sin);
    for (auto& kv : e->tapmap)
        if (kv.second.d) (void)hipFree(kv.second.d);
    for (auto& pe : e->pending) (void)hipEventDestroy(pe.ev);
    for (auto ev : e->event_pool) (void)hipEventDestroy(ev);
    if (e->amax_host) (void)hipHostFree(e->amax_host);
    if (e->item_codes) (void)hipFree(e->item_codes);
    if (e->dws) (void)hipFree(e->dws);
    if (e->dec_flag_host) (void)hipHostFree(e->dec_flag_host);
    if (e->dec_rg_host) (void)hipHostFree(e->dec_rg_host);
    for (auto& q : e->pend) {
        if (q.done) (void)hipEventDestroy(q.done);
        if (q.amax) (void)hipHostFree(q.amax);
        if (q.rg_pinned) (void)hipHostFree(q.rg_pinned);
        if (q.chain_word) (void)hipHostFree(q.chain_word);
    }
    for (auto& h : e->hostio) {
        if (h.done) (void)hipEventDestroy(h.done);
        if (h.h_audio) (void)hipHostFree(h.h_audio);
        if (h.d_audio) (void)hipFree(h.d_audio);
        if (h.d_codes) (void)hipFree(h.d_codes);
        if (h.h_codes) (void)hipHostFree(h.h_codes);
    }
    drop_graphs(e);
    for (auto& l : e->lanes) {
        if (l.ws) (void)hipFree(l.ws);
        if (l.amax_dev) (void)hipFree(l.amax_dev);
        if (l.io_dev) (void)hipFree(l.io_dev);
        if (l.ws_free) (void)hipEventDestroy(l.ws_free);
        if (l.in_ready) (void)hipEventDestroy(l.in_ready);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    delete e;
}

// ------------------------------------------------------------------------------------------------
// instrumentation
// ------------------------------------------------------------------------------------------------
extern "C" int mimi_set_precision(mimi_engine* e, int32_t mode) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    if (mode < MIMI_PRECISION_F32 || mode > MIMI_PRECISION_F16X3)
        return set_err(MIMI_ERR_INVALID_ARGUMENT, "precision mode %d", mode);
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->precision != mode) {  // (the encodes in flight in either lane finish in the mode they were submitted in)
        HIP_TRY(hipSetDevice(e->device));
        drain_lanes(e);
    }
    e->precision = mode;
    return MIMI_OK;
}

extern "C" int mimi_set_graphs(mimi_engine* e, int32_t enable) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    e->graphs_enabled = enable != 0;
    if (!enable) drop_graphs(e, true);
    return MIMI_OK;
}

extern "C" int64_t mimi_graph_replays(const mimi_engine* e) { return e ? e->graph_replays : -1; }

extern "C" int64_t mimi_graph_captures(const mimi_engine* e) { return e ? e->graph_captures : -1; }

extern "C" int64_t mimi_lane_encodes(const mimi_engine* e, int32_t lane) {
    return e && lane >= 0 && lane < mimi_engine::kLanes ? e->lanes[lane].encodes : -1;
}

// mimi_set_option keys: engine field, allowed values (bit v of `allowed` set: value v accepted), what they select.
// Every key changes the kernel sequence (never the bits an encode produces), so a change drops captured graphs.
struct EngineOption {
    const char* key;
    int mimi_engine::*field;
    unsigned allowed;
    const char* values;
};
static const EngineOption kEngineOptions[] = {
    {"stage0_fused", &mimi_engine::stage0_fused, 0x3u, "0 or 1"},
    {"rvq_form", &mimi_engine::rvq_form, 0x7fu, "0..6"},
    {"ln_rpw", &mimi_engine::ln_rpw, 0x117u, "0, 1, 2, 4 or 8"},
    {"rvq_xcd", &mimi_engine::rvq_xcd, 0x3u, "0 or 1"},
    {"rvq_chain", &mimi_engine::rvq_chain, 0x3u, "0 or 1"},
    {"rvq_chain_fault", &mimi_engine::rvq_chain_fault, 0x7u, "0, 1 or 2"},
    {"sc1_out", &mimi_engine::sc1_out, 0xffu, "0..7"},
    {"ln_fused", &mimi_engine::ln_fused, 0x1fu, "0 .. 4"},
    {"qkv_attn", &mimi_engine::qkv_attn, 0x7u, "0, 1 or 2"},
    {"qkv_attn_xcd", &mimi_engine::qkv_attn_xcd, 0x3u, "0 or 1"},
    {"attn_band_split", &mimi_engine::attn_band_split, 0x7u, "0, 1 or 2"},
    {"fc1_cg", &mimi_engine::fc1_cg, 0x17u, "0, 1, 2 or 4"},
    {"gemm256", &mimi_engine::gemm256, 0xffu, "0..7"},
    {"res1_form", &mimi_engine::res1_form, 0x3u, "0 or 1"},
    {"res1_stream", &mimi_engine::res1_stream, 0x7u, "0, 1 or 2"},
    {"lanes", &mimi_engine::lanes_opt, 0x7u, "0, 1 or 2"},
};

extern "C" int mimi_set_option(mimi_engine* e, const char* key, int64_t value) {
    if (!e || !key) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine or key");
    std::lock_guard<std::mutex> lk(e->mu);
    for (const EngineOption& o : kEngineOptions) {
        if (strcmp(key, o.key)) continue;
        if (value < 0 || value > 31 || !((o.allowed >> value) & 1u))
            return set_err(MIMI_ERR_INVALID_ARGUMENT, "%s %lld (%s)", key, (long long)value, o.values);
        HIP_TRY(hipSetDevice(e->device));
        drain_lanes(e);
        // captured graphs hold the other kernel sequence (both lanes drained first: drop_graphs)
        if (e->*o.field != (int)value) drop_graphs(e, true);
        e->*o.field = (int)value;
        return MIMI_OK;
    }
    return set_err(MIMI_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}

extern "C" int mimi_act_scales(mimi_engine* e, int32_t max_n, char* names, float* scales, float* last_max,
                               int32_t* n) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int i = 0;
    for (const auto& kv : e->slot_of) {
        const int slot = kv.second;
        if (i >= max_n) break;
        if (names) {
            std::strncpy(names + 64 * i, kv.first.c_str(), 63);
            names[64 * i + 63] = 0;
        }
        if (scales) scales[i] = slot < (int)e->act_scale.size() ? e->act_scale[slot] : 0.0f;
        if (last_max) {
            last_max[i] = slot < (int)e->last_amax.size() ? e->last_amax[slot] : -1.0f;
            // a LayerNorm output whose range check encode_pass skips (ln_check_free: the same rule) records no maximum
            int l = -1, k = 0;
            if (MIMI_LN_CHECK_SKIP && e->calibrated && std::sscanf(kv.first.c_str(), "xf%d.ln%d", &l, &k) == 2 && l >= 0 &&
                l < (int)e->xf.size() && (k == 1 || k == 2) && slot < (int)e->act_scale.size() && e->act_scale[slot] > 0.0f &&
                (k == 1 ? e->xf[l].ln1_bound : e->xf[l].ln2_bound) * e->act_scale[slot] < 16384.0f)
                last_max[i] = -1.0f;
        }
        ++i;
    }
    if (n) *n = i;
    return MIMI_OK;
}

extern "C" int mimi_get_precision(const mimi_engine* e) { return e ? e->precision : -1; }

extern "C" int mimi_calibrate(mimi_engine* e) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    if (!e->finalized) return set_err(MIMI_ERR_STATE, "mimi_finalize has not been called");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->calibrated) return MIMI_OK;
    HIP_TRY(hipSetDevice(e->device));
    (void)hipGetLastError();
    return calibrate_scales(e);
}

extern "C" int64_t mimi_f16_reruns(const mimi_engine* e) { return e ? e->f16_reruns : -1; }

extern "C" int64_t mimi_rvq_chain_reruns(const mimi_engine* e) { return e ? e->chain_reruns : -1; }

extern "C" int mimi_set_profiling(mimi_engine* e, int enable) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    if (enable < 0 || enable > 2) return set_err(MIMI_ERR_INVALID_ARGUMENT, "profiling level %d (0, 1 or 2)", enable);
    std::lock_guard<std::mutex> lk(e->mu);
    e->profiling = enable;
    return MIMI_OK;
}

static int resolve_pending(mimi_engine* e) {
    HIP_TRY(hipSetDevice(e->device));
    hipEvent_t prev = nullptr;
    std::vector<std::string> seq;
    for (auto& pe : e->pending) {
        HIP_TRY(hipEventSynchronize(pe.ev));
        if (pe.name.empty()) {
            prev = pe.ev;
            if (!seq.empty()) e->last_seq = std::move(seq);
            seq.clear();
            continue;
        }
        seq.push_back(pe.name);
        float ms = 0;
        if (prev) HIP_TRY(hipEventElapsedTime(&ms, prev, pe.ev));
        if (!e->prof.count(pe.name)) e->prof_order.push_back(pe.name);
        ProfStat& st = e->prof[pe.name];
        st.ms += ms;
        st.flops += pe.flops;
        st.bytes += pe.bytes;
        st.launches += 1;
        prev = pe.ev;
    }
    if (!seq.empty()) e->last_seq = std::move(seq);
    for (auto& pe : e->pending) e->event_pool.push_back(pe.ev);
    e->pending.clear();
    return MIMI_OK;
}

extern "C" int mimi_profile_sequence(mimi_engine* e, int32_t max_stages, char* names, int32_t* n_stages) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = resolve_pending(e);
    if (rc) return rc;
    int i = 0;
    for (const auto& n : e->last_seq) {
        if (i >= max_stages) break;
        if (names) {
            std::strncpy(names + 128 * i, n.c_str(), 127);
            names[128 * i + 127] = 0;
        }
        ++i;
    }
    if (n_stages) *n_stages = i;
    return MIMI_OK;
}

extern "C" int mimi_profile_read(mimi_engine* e, int32_t max_stages, char* names, double* total_ms, int64_t* launches,
                                 double* flops, int32_t* n_stages) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = resolve_pending(e);
    if (rc) return rc;
    int i = 0;
    for (const auto& n : e->prof_order) {
        if (i >= max_stages) break;
        const ProfStat& st = e->prof[n];
        if (names) {
            std::strncpy(names + 128 * i, n.c_str(), 127);
            names[128 * i + 127] = 0;
        }
        if (total_ms) total_ms[i] = st.ms;
        if (launches) launches[i] = st.launches;
        if (flops) flops[2 * i] = st.flops, flops[2 * i + 1] = st.bytes;
        ++i;
    }
    if (n_stages) *n_stages = i;
    return MIMI_OK;
}

extern "C" int mimi_profile_reset(mimi_engine* e) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = resolve_pending(e);
    e->prof.clear();
    e->prof_order.clear();
    return rc;
}

extern "C" int mimi_set_taps(mimi_engine* e, int enable) {
    if (!e) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    e->taps = enable != 0;
    return MIMI_OK;
}

extern "C" int mimi_get_tap(mimi_engine* e, const char* name, float* dst, int64_t cap, int64_t* numel, int64_t dims[3]) {
    if (!e || !name) return set_err(MIMI_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    auto it = e->tapmap.find(name);
    if (it == e->tapmap.end()) return set_err(MIMI_ERR_INVALID_ARGUMENT, "no tap named %s", name);
    const auto& tp = it->second;
    const int64_t n = tp.dims[0] * tp.dims[1] * tp.dims[2];
    if (numel) *numel = n;
    if (dims) std::memcpy(dims, tp.dims, sizeof(tp.dims));
    if (dst) {
        if (cap < n) return set_err(MIMI_ERR_INVALID_ARGUMENT, "tap %s needs %lld floats", name, (long long)n);
        HIP_TRY(hipSetDevice(e->device));
        // the taps were copied inside the last encode: wait for it alone (a device-wide sync is refused while any
        // other engine in the process captures a graph)
        drain_lanes(e);
        if (!e->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        HIP_TRY(hipMemcpyWithStream(dst, tp.d, n * 4, hipMemcpyDeviceToHost, e->cap_stream));
    }
    return MIMI_OK;
}
