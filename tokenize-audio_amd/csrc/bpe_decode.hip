// Codec-BPE decoding of token ids that are already in device memory: ids -> the code characters they spell -> the
// reference converter's drop rules -> codes laid out as mimi_decode_ragged takes them (mimi_bpe_decode_plan,
// mimi_bpe_decode_write; mimi_hip/bpe.py Encoder.decode_device drives them, Encoder.decode_ids states the contract).
//
// An id spells a sequence of alphabet indices (special ids: none).  Per sequence of ids the spellings are
// concatenated; character i has codebook cb_i = index_i / codebook_size; with expected = cb_0 at the start a
// character is kept iff cb_i == expected and a kept one advances expected to (expected + 1) % K; of the kept ones the
// first min((K - cb_0) % K, kept) and then the last remaining % K are dropped; the rest are T = remaining / K frames.
//
// The filter is a scan: character i is the map f_i(e) = e == cb_i ? (e + 1) % K : e on [0, K), the state before
// character i is f_{i-1} o ... o f_0, and the first character of a sequence is the constant map to (cb_0 + 1) % K,
// which absorbs everything to its left, so no segmented scan is needed.  A map is a u64 of K <= 16 nibbles.  The
// operator does not commute: `combine(earlier, later)` keeps that order in the shuffle steps, across the waves, across
// the rows of a tile and in the tile carry.
//
// All sequences of a call lie end to end, first in a space of ids, then in a space of N characters.  Kernels, in
// stream order (kernel boundaries are the only grid-wide ordering; no workgroup waits on another):
//   1. scan (+) over the ids of the spelling lengths, an id checked against [0, n_tokens) BEFORE the table load
//      -> id_start[j] = first character of id j; cpos[s] = first character of sequence s;
//      -> read-back of N and the bad-id flag (N sizes the character buffers);
//   2. scan (map composition) over the characters: a character finds its sequence and its id by binary search, loads
//      its alphabet index, the apply pass stores index | codebook | keep bit;
//   3. scan (+) of the keep bits -> rank[p] = kept characters before p; per sequence: cb_0, kept, the begin drop, T;
//   4. read-back of the n_seq frame counts;
//   5. (mimi_bpe_decode_write) a kept character of rank r in [begin, begin + K T) of its sequence goes to
//      codes[seq][(r - begin) % K][(r - begin) / K].
// Each scan is the three passes of bpe_words.hip (reduce per tile, one workgroup over the tile values, apply), here
// over any associative operator.
#include <algorithm>
#include <vector>

#include "bpe_model.h"
#include "bpe_scan.h"

namespace {

using mimi::bpe::fail;
// the operators, the workgroup scan and the binary search: bpe_scan.h (shared with bpe_decode_stream.hip)
using mimi::bpe::AddOp;
using mimi::bpe::block_exclusive;
using mimi::bpe::char_map;
using mimi::bpe::find_in;
using mimi::bpe::kMaxK;
using mimi::bpe::MapOp;
using mimi::bpe::u64;

constexpr int kThreads = mimi::bpe::kScanThreads;
constexpr int kTile = MIMI_BPE_DECODE_SCAN_TILE;
constexpr int kItems = kTile / kThreads;  // rows of kThreads positions per tile
static_assert(kTile % kThreads == 0 && kThreads == 256, "tile layout");

// info word of a character: alphabet index (17 bits) | codebook << 17 (4 bits) | first of its sequence << 21 | keep << 22
constexpr int kCbShift = 17, kFirstShift = 21, kKeepShift = 22;
constexpr unsigned kIdxMask = (1u << kCbShift) - 1;

// pass 1: partials[tile] = the tile's values combined in position order (row by row: the operator need not commute)
template <typename Op, typename Src>
__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(Op op, Src src, int n, u64* partials) {
    __shared__ u64 wtot[kThreads / 64];
    const long long base = (long long)blockIdx.x * kTile;
    u64 acc = op.identity();
#pragma unroll 1
    for (int i = 0; i < kItems; ++i) {
        const long long p = base + i * kThreads + threadIdx.x;
        const u64 v = p < n ? src((int)p) : op.identity();
        u64 total;
        (void)block_exclusive(op, v, wtot, total);
        acc = op.combine(acc, total);
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// pass 2, one workgroup: partials -> their exclusive scan, in place; *total = all of them
template <typename Op>
__global__ __launch_bounds__(kThreads) void scan_partials_kernel(Op op, u64* partials, int n_tiles, u64* total_out) {
    __shared__ u64 wtot[kThreads / 64];
    u64 carry = op.identity();
    for (int base = 0; base < n_tiles; base += kThreads) {
        const int i = base + threadIdx.x;
        const u64 v = i < n_tiles ? partials[i] : op.identity();
        u64 total;
        const u64 e = block_exclusive(op, v, wtot, total);
        if (i < n_tiles) partials[i] = op.combine(carry, e);
        carry = op.combine(carry, total);
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// pass 3: sink(p, the values before p combined)
template <typename Op, typename Src, typename Sink>
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(Op op, Src src, Sink sink, int n, const u64* partials) {
    __shared__ u64 wtot[kThreads / 64];
    const long long base = (long long)blockIdx.x * kTile;
    u64 carry = partials[blockIdx.x];
#pragma unroll 1
    for (int i = 0; i < kItems; ++i) {
        const long long p = base + i * kThreads + threadIdx.x;
        const u64 v = p < n ? src((int)p) : op.identity();
        u64 total;
        const u64 e = block_exclusive(op, v, wtot, total);
        if (p < n) sink((int)p, op.combine(carry, e));
        carry = op.combine(carry, total);
    }
}

// ---- value sources and sinks ---------------------------------------------------------------------------------
// 1. the spelling length of id j
struct LengthSrc {
    const int* ids;
    const int* spell_off;  // [n_tokens + 1]
    int n_tokens;
    unsigned* ctl;
    __device__ u64 operator()(int j) const {
        const int id = ids[j];
        if ((unsigned)id >= (unsigned)n_tokens) {  // before the table load
            atomicOr(ctl, 1u);
            return 0;
        }
        return (u64)(unsigned)(spell_off[id + 1] - spell_off[id]);
    }
};

struct StoreInt {
    int* out;
    __device__ void operator()(int p, u64 before) const { out[p] = (int)before; }
};

// 2. the map of character p; classify stores the info word, the apply pass reads it back
struct ClassifySrc {
    const int* ids;
    const int* id_start;  // [n_ids + 1]
    const int* cpos;      // [n_seq + 1]
    const int* spell_off;
    const int* spell_idx;
    int n_ids, n_seq, K, codebook_size;
    unsigned* info;
    __device__ u64 operator()(int p) const {
        const int s = find_in(cpos, n_seq, p);
        const int j = find_in(id_start, n_ids, p);
        const unsigned idx = (unsigned)spell_idx[spell_off[ids[j]] + (p - id_start[j])];
        const unsigned cb = idx / (unsigned)codebook_size;
        const bool first = p == cpos[s];
        info[p] = idx | (cb << kCbShift) | ((unsigned)first << kFirstShift);
        return char_map(cb, first, K);
    }
};

struct MapSrc {
    const unsigned* info;
    int K;
    __device__ u64 operator()(int p) const {
        const unsigned v = info[p];
        return char_map((v >> kCbShift) & 15u, (v >> kFirstShift) & 1u, K);
    }
};

// the state before a character that is not the first of its sequence is a constant map: any entry is `expected`
struct KeepSink {
    unsigned* info;
    __device__ void operator()(int p, u64 before) const {
        const unsigned v = info[p];
        const bool keep = ((v >> kFirstShift) & 1u) || ((unsigned)before & 15u) == ((v >> kCbShift) & 15u);
        info[p] = v | ((unsigned)keep << kKeepShift);
    }
};

// 3. the keep bit
struct KeepSrc {
    const unsigned* info;
    __device__ u64 operator()(int p) const { return (u64)((info[p] >> kKeepShift) & 1u); }
};

// cpos[s] = the first character of sequence s; id_start[n_ids] = cpos[n_seq] = n close the binary searches
__global__ __launch_bounds__(kThreads) void seq_starts_kernel(int* id_start, const int* seq_ids, int n_ids, int n_seq,
                                                              int n, int* cpos) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s == 0) id_start[n_ids] = n;
    if (s > n_seq) return;
    const int j = seq_ids[s];
    cpos[s] = j < n_ids ? id_start[j] : n;
}

// per sequence: the rank of its first written character and its frames
__global__ __launch_bounds__(kThreads) void seq_plan_kernel(const unsigned* info, const int* rank, const u64* kept_total,
                                                            const int* cpos, int n_seq, int n, int K, int* begin_rank,
                                                            long long* frames) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= n_seq) return;
    const int c0 = cpos[s], c1 = cpos[s + 1];
    if (c0 == c1) {
        begin_rank[s] = 0;
        frames[s] = 0;
        return;
    }
    const int r0 = rank[c0], r1 = c1 < n ? rank[c1] : (int)*kept_total;
    const int kept = r1 - r0;
    const int cb0 = (int)((info[c0] >> kCbShift) & 15u);
    const int begin = min((K - cb0) % K, kept);
    begin_rank[s] = r0 + begin;
    frames[s] = (kept - begin) / K;
}

struct WriteArgs {
    const unsigned* info;
    const int* rank;
    const int* cpos;
    const int* begin_rank;
    const long long* frames;
    int n, n_seq, K, codebook_size;
    int* codes;
    long long item_stride, row_stride;
};

__global__ __launch_bounds__(kThreads) void write_kernel(WriteArgs a) {
    const long long pl = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pl >= a.n) return;
    const int p = (int)pl;
    const unsigned v = a.info[p];
    if (!((v >> kKeepShift) & 1u)) return;
    const int s = find_in(a.cpos, a.n_seq, p);
    const long long r = (long long)a.rank[p] - a.begin_rank[s];
    if (r < 0 || r >= (long long)a.K * a.frames[s]) return;
    const int k = (int)(r % a.K);
    const long long t = r / a.K;
    a.codes[(long long)s * a.item_stride + (long long)k * a.row_stride + t] = (int)(v & kIdxMask) - k * a.codebook_size;
}

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the three passes over n >= 0 values on s.  Reduce reads through `first` (which may have side effects: the classify),
// apply through `again`; *total = all n values combined
template <typename Op, typename First, typename Again, typename Sink>
int scan_on_stream(const Op& op, const First& first, const Again& again, const Sink& sink, int n, u64* partials,
                   u64* total, hipStream_t s) {
    const unsigned tiles = blocks_for(n, kTile);
    if (tiles > 0)
        hipLaunchKernelGGL((scan_reduce_kernel<Op, First>), dim3(tiles), dim3(kThreads), 0, s, op, first, n, partials);
    hipLaunchKernelGGL((scan_partials_kernel<Op>), dim3(1), dim3(kThreads), 0, s, op, partials, (int)tiles, total);
    if (tiles > 0)
        hipLaunchKernelGGL((scan_apply_kernel<Op, Again, Sink>), dim3(tiles), dim3(kThreads), 0, s, op, again, sink, n,
                           partials);
    ENC_TRY(hipGetLastError());
    return MIMI_OK;
}

// control words (dec_ctl, u64 each): the bad-id flag, the character count, the kept count, the map scan's total
enum { CTL_BAD = 0, CTL_CHARS = 1, CTL_KEPT = 2, CTL_MAP = 3, CTL_WORDS = 4 };

// everything on s; `table` is the caller's so that it outlives the copy queued here (the caller synchronises s, also
// when this fails half way)
int plan_on_stream(mimi_bpe_model* m, const int32_t* dev_ids, const std::vector<int>& table, int n_ids, int n_seq,
                   int64_t* frame_lengths, hipStream_t s) {
    const int K = m->num_codebooks;
    ENC_TRY(hipSetDevice(m->device));
    ENC_TRY(m->dec_seq_ids.reserve((size_t)(n_seq + 1) * 4));
    ENC_TRY(m->dec_id_start.reserve((size_t)(n_ids + 1) * 4));
    ENC_TRY(m->dec_cpos.reserve((size_t)(n_seq + 1) * 4));
    ENC_TRY(m->dec_begin.reserve((size_t)std::max(n_seq, 1) * 4));
    ENC_TRY(m->dec_frames.reserve((size_t)std::max(n_seq, 1) * 8));
    ENC_TRY(m->dec_partials.reserve((size_t)(blocks_for(n_ids, kTile) + 1) * 8));
    ENC_TRY(m->dec_ctl.reserve(CTL_WORDS * 8));
    u64* dctl = (u64*)m->dec_ctl.p;
    int* id_start = (int*)m->dec_id_start.p;
    int* cpos = (int*)m->dec_cpos.p;
    ENC_TRY(hipMemcpyAsync(m->dec_seq_ids.p, table.data(), (size_t)(n_seq + 1) * 4, hipMemcpyHostToDevice, s));
    ENC_TRY(hipMemsetAsync(dctl, 0, CTL_WORDS * 8, s));

    // 1: the characters of every id and every sequence
    const LengthSrc lengths{dev_ids, (const int*)m->spell_off, m->n_tokens, (unsigned*)(dctl + CTL_BAD)};
    int rc = scan_on_stream(AddOp{}, lengths, lengths, StoreInt{id_start}, n_ids, (u64*)m->dec_partials.p,
                            dctl + CTL_CHARS, s);
    if (rc != MIMI_OK) return rc;
    u64 head[2] = {0, 0};  // the flag, the character count
    ENC_TRY(hipMemcpyAsync(head, dctl, sizeof head, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipStreamSynchronize(s));
    if (head[CTL_BAD]) return fail(MIMI_ERR_INVALID_ARGUMENT, "a token id is outside [0, %d)", m->n_tokens);
    if (head[CTL_CHARS] >= (1ull << 31)) return fail(MIMI_ERR_UNSUPPORTED, "the ids spell 2^31 characters or more");
    const int N = (int)head[CTL_CHARS];
    hipLaunchKernelGGL(seq_starts_kernel, dim3(blocks_for((long long)n_seq + 1, kThreads)), dim3(kThreads), 0, s,
                       id_start, (const int*)m->dec_seq_ids.p, n_ids, n_seq, N, cpos);
    ENC_TRY(hipGetLastError());

    if (N > 0) {
        ENC_TRY(m->dec_info.reserve((size_t)N * 4));
        ENC_TRY(m->dec_rank.reserve((size_t)N * 4));
        ENC_TRY(m->dec_partials.reserve((size_t)(blocks_for(N, kTile) + 1) * 8));
        unsigned* info = (unsigned*)m->dec_info.p;
        u64* partials = (u64*)m->dec_partials.p;
        // 2: the filter
        const ClassifySrc classify{dev_ids, id_start, cpos, (const int*)m->spell_off, (const int*)m->spell_idx,
                                   n_ids,   n_seq,    K,    m->codebook_size,         info};
        rc = scan_on_stream(MapOp{K}, classify, MapSrc{info, K}, KeepSink{info}, N, partials, dctl + CTL_MAP, s);
        if (rc != MIMI_OK) return rc;
        // 3: the kept ranks
        const KeepSrc keep{info};
        rc = scan_on_stream(AddOp{}, keep, keep, StoreInt{(int*)m->dec_rank.p}, N, partials, dctl + CTL_KEPT, s);
        if (rc != MIMI_OK) return rc;
    }
    hipLaunchKernelGGL(seq_plan_kernel, dim3(blocks_for(n_seq, kThreads)), dim3(kThreads), 0, s,
                       (const unsigned*)m->dec_info.p, (const int*)m->dec_rank.p, (const u64*)(dctl + CTL_KEPT),
                       (const int*)cpos, n_seq, N, K, (int*)m->dec_begin.p, (long long*)m->dec_frames.p);
    ENC_TRY(hipGetLastError());
    // 4: the frame counts
    ENC_TRY(hipMemcpyAsync(frame_lengths, m->dec_frames.p, (size_t)n_seq * 8, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipStreamSynchronize(s));
    m->plan_chars = N;
    return MIMI_OK;
}

}  // namespace

extern "C" int mimi_bpe_model_set_spellings(mimi_bpe_model* m, const int64_t* spell_offsets,
                                            const int32_t* spell_index) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (!spell_offsets) return fail(MIMI_ERR_INVALID_ARGUMENT, "null spelling offsets");
    std::lock_guard<std::mutex> lock(m->mu);
    m->plan_valid = false;
    if (!m->alphabet) return fail(MIMI_ERR_STATE, "mimi_bpe_model_set_alphabet has not been called");
    const int n = m->n_tokens;
    const int64_t n_base = (int64_t)m->num_codebooks * m->codebook_size;
    if (spell_offsets[0] != 0) return fail(MIMI_ERR_INVALID_ARGUMENT, "spelling offsets must start at 0");
    for (int i = 0; i < n; ++i)
        if (spell_offsets[i + 1] < spell_offsets[i])
            return fail(MIMI_ERR_INVALID_ARGUMENT, "spelling offsets must be non-decreasing");
    const int64_t total = spell_offsets[n];
    if (total >= (1ll << 31)) return fail(MIMI_ERR_UNSUPPORTED, "the spellings hold 2^31 characters or more");
    if (total > 0 && !spell_index) return fail(MIMI_ERR_INVALID_ARGUMENT, "null spelling indices");
    for (int64_t i = 0; i < total; ++i)
        if (spell_index[i] < 0 || spell_index[i] >= n_base)
            return fail(MIMI_ERR_INVALID_ARGUMENT, "spelling index %d at %lld is outside the alphabet of %lld",
                        spell_index[i], (long long)i, (long long)n_base);
    std::vector<int> off((size_t)n + 1);
    for (int i = 0; i <= n; ++i) off[i] = (int)spell_offsets[i];
    ENC_TRY(hipSetDevice(m->device));
    int *dev_off = nullptr, *dev_idx = nullptr;
    ENC_TRY(hipMalloc(&dev_off, off.size() * 4));
    hipError_t e = hipMalloc(&dev_idx, (size_t)std::max<int64_t>(total, 1) * 4);
    if (e == hipSuccess) e = hipMemcpy(dev_off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && total > 0) e = hipMemcpy(dev_idx, spell_index, (size_t)total * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev_off);
        if (dev_idx) (void)hipFree(dev_idx);
        ENC_TRY(e);
    }
    if (m->spell_off) (void)hipFree(m->spell_off);
    if (m->spell_idx) (void)hipFree(m->spell_idx);
    m->spell_off = dev_off;
    m->spell_idx = dev_idx;
    ++m->spell_version;
    return MIMI_OK;
}

extern "C" int mimi_bpe_decode_plan(mimi_bpe_model* m, const int32_t* dev_ids, const int64_t* seq_offsets,
                                    int64_t n_seq, int64_t* frame_lengths, void* stream) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (n_seq < 0 || !seq_offsets || (n_seq > 0 && !frame_lengths))
        return fail(MIMI_ERR_INVALID_ARGUMENT, "bad sequence arguments");
    if (n_seq > 0x3fffffffll) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^30 sequences");
    std::lock_guard<std::mutex> lock(m->mu);
    m->plan_valid = false;
    if (!m->spell_off) return fail(MIMI_ERR_STATE, "mimi_bpe_model_set_spellings has not been called");
    if (m->num_codebooks > kMaxK)
        return fail(MIMI_ERR_UNSUPPORTED, "%d codebooks: the device filter packs at most %d", m->num_codebooks, kMaxK);
    if (seq_offsets[0] != 0) return fail(MIMI_ERR_INVALID_ARGUMENT, "sequence offsets must start at 0");
    for (int64_t s = 0; s < n_seq; ++s)
        if (seq_offsets[s + 1] < seq_offsets[s])
            return fail(MIMI_ERR_INVALID_ARGUMENT, "sequence offsets must be non-decreasing");
    const int64_t n_ids = seq_offsets[n_seq];
    if (n_ids >= (1ll << 31)) return fail(MIMI_ERR_UNSUPPORTED, "2^31 ids or more");
    if (n_ids > 0 && !dev_ids) return fail(MIMI_ERR_INVALID_ARGUMENT, "null ids");
    m->plan_seqs = (int)n_seq;
    m->plan_chars = 0;
    m->plan_max_frames = 0;
    if (n_seq == 0) {
        m->plan_valid = true;
        return MIMI_OK;
    }
    std::vector<int> table((size_t)n_seq + 1);
    for (int64_t s = 0; s <= n_seq; ++s) table[s] = (int)seq_offsets[s];
    hipStream_t s = (hipStream_t)stream;
    const int rc = plan_on_stream(m, dev_ids, table, (int)n_ids, (int)n_seq, frame_lengths, s);
    if (rc != MIMI_OK) {
        (void)hipStreamSynchronize(s);  // nothing queued above may still read the host arrays
        return rc;
    }
    for (int64_t i = 0; i < n_seq; ++i) m->plan_max_frames = std::max<int64_t>(m->plan_max_frames, frame_lengths[i]);
    m->plan_valid = true;
    return MIMI_OK;
}

extern "C" int mimi_bpe_decode_write(mimi_bpe_model* m, int32_t* dev_codes, int64_t item_stride, int64_t row_stride,
                                     int64_t max_frames, void* stream) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (item_stride < 0 || row_stride < 0 || max_frames < 0) return fail(MIMI_ERR_INVALID_ARGUMENT, "bad layout arguments");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->plan_valid) return fail(MIMI_ERR_STATE, "no plan: mimi_bpe_decode_plan must be the model's last call");
    if (max_frames < m->plan_max_frames)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "max_frames %lld is below the plan's longest sequence of %lld frames",
                    (long long)max_frames, (long long)m->plan_max_frames);
    if (m->plan_chars == 0 || m->plan_max_frames == 0) return MIMI_OK;
    if (!dev_codes) return fail(MIMI_ERR_INVALID_ARGUMENT, "null codes");
    hipStream_t s = (hipStream_t)stream;
    ENC_TRY(hipSetDevice(m->device));
    const WriteArgs a{(const unsigned*)m->dec_info.p,
                      (const int*)m->dec_rank.p,
                      (const int*)m->dec_cpos.p,
                      (const int*)m->dec_begin.p,
                      (const long long*)m->dec_frames.p,
                      m->plan_chars,
                      m->plan_seqs,
                      m->num_codebooks,
                      m->codebook_size,
                      dev_codes,
                      item_stride,
                      row_stride};
    hipLaunchKernelGGL(write_kernel, dim3(blocks_for(m->plan_chars, kThreads)), dim3(kThreads), 0, s, a);
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipStreamSynchronize(s));
    return MIMI_OK;
}
