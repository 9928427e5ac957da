// Codec-BPE encoding of codes that are already in device memory: the word model of mimi_hip/bpe.py CharModel.words
// on the GPU, then the merge kernels of bpe_encode.hip, then the ids packed per sequence (mimi_bpe_encode_codes;
// mimi_hip/bpe.py Encoder.encode_device drives it).
//
// The string of a sequence holds, at position (frame t, codebook k) = t * K + k, the character with alphabet index
// k * codebook_size + code.  A character has a class (keep / drop x starter / mark, or split) and a combining
// class; inside each run of non-starters the kept marks are stably sorted by combining class, dropped characters
// vanish, split characters vanish and cut the word, a kept character's symbol is n_special + index.  Runs and
// words never cross a sequence.
//
// All sequences of a call lie end to end in one position space of N = K * (sum of frames) positions.  Kernels, in
// stream order (kernel boundaries are the only grid-wide ordering; no workgroup waits on another):
//   1. classify + reduce: one thread per position finds its sequence (binary search of the sequence starts), reads
//      its code, checks it against [0, codebook_size) BEFORE the alphabet load, stores index | class | ccc, and the
//      workgroup sums (keep bit | split bit << 32) of its tile of kTile positions;
//   2. one workgroup scans the tile sums (kThreads at a time with a carry);
//   3. apply: exclusive scan of the packed bits per position -> scan[p] = kept before p | splits before p << 32,
//      scan[N] = the totals;
//   4. scatter: a kept character's symbol goes to its kept rank; a kept mark first ranks itself inside its run (a
//      walk of at most MIMI_BPE_WORDS_MAX_RUN non-starters to the nearest starter-class character or sequence end on
//      either side: destination = run's first kept slot + kept marks of the run with smaller ccc + earlier ones with
//      equal ccc); a split character writes the offset of the word after it.  Word index = splits before + sequence;
//   5. per sequence: the offset of its first word; per word: length -> one atomic into its form's list and an
//      atomic max of the longest word;  -> the call's one mid-way read-back (flags, three counts, longest);
//   6. the merge kernels (bpe_encode.hip launch_forms) on the model's symbols / offsets / out_ids / out_lens;
//   7. pack: the same three scan passes over the words' output lengths, one thread per kept symbol copies its id to
//      the packed place, one thread per sequence writes the sequence offset.
#include <algorithm>
#include <vector>

#include "bpe_model.h"

namespace {

using mimi::bpe::fail;
using mimi::bpe::kLdsCap;
using mimi::bpe::kSmallCap;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kItems = MIMI_BPE_WORDS_SCAN_TILE / kThreads;  // positions per thread of a scan tile
constexpr int kTile = MIMI_BPE_WORDS_SCAN_TILE;
constexpr int kMaxRun = MIMI_BPE_WORDS_MAX_RUN;
constexpr int kMaxBlocks = 4096;  // grid of the grid-stride kernels
static_assert(kTile % kThreads == 0 && kThreads == 256, "tile layout");

// character classes: mimi_hip/bpe.py
enum : unsigned { KEEP_STARTER = 0, KEEP_MARK = 1, DROP_STARTER = 2, DROP_MARK = 3, SPLIT = 4 };
// info word of a position: alphabet index (17 bits) | class << 17 | ccc << 24
constexpr int kClsShift = 17, kCccShift = 24;
constexpr unsigned kIdxMask = (1u << kClsShift) - 1;

// control words (the model's `bad` buffer, 8 x u32)
enum { CTL_BAD_SYMBOL = 0, CTL_BAD_CODE = 1, CTL_LONG_RUN = 2, CTL_COUNT0 = 3, CTL_LONGEST = 6, CTL_KEPT = 7, CTL_WORDS = 8 };

__device__ __forceinline__ unsigned cls_of(unsigned info) { return (info >> kClsShift) & 7u; }
__device__ __forceinline__ bool is_mark(unsigned info) { return (cls_of(info) | 2u) == 3u; }  // KEEP_MARK, DROP_MARK
__device__ __forceinline__ u64 bits_of(unsigned info) {
    const unsigned c = cls_of(info);
    return (u64)(c <= KEEP_MARK) | ((u64)(c == SPLIT) << 32);
}

struct Seqs {
    const int* pos;    // [n_seq + 1] first position of each sequence, pos[n_seq] = N
    const int* item;   // [n_seq]
    const int* frame;  // [n_seq] first frame in the item
    int n_seq;
};

// the sequence that holds position p < pos[n_seq]: the last s with pos[s] <= p (empty sequences are skipped)
__device__ __forceinline__ int seq_of(const Seqs& q, int p) {
    int lo = 0, hi = q.n_seq;  // pos[lo] <= p < pos[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (q.pos[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// exclusive scan of one value per thread over the workgroup; total = the workgroup's sum.  wsum: 4 words of LDS
__device__ __forceinline__ u64 block_exclusive(u64 v, u64* wsum, u64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        const u64 s = wsum[i];
        if (i < wave) base += s;
        all += s;
    }
    __syncthreads();  // wsum is reused by the next call
    total = all;
    return base + x - v;
}

// ---- value sources of the scan passes -------------------------------------------------------------------------
struct ClassifySrc {
    const int* codes;
    long long item_stride, row_stride;
    Seqs q;
    const unsigned short* alphabet;
    int K, codebook_size;
    unsigned* info;
    unsigned* ctl;
    __device__ u64 operator()(int p) const {
        const int s = seq_of(q, p);
        const int local = p - q.pos[s];
        const int t = q.frame[s] + local / K, k = local % K;
        int code = codes[(long long)q.item[s] * item_stride + (long long)k * row_stride + t];
        if ((unsigned)code >= (unsigned)codebook_size) {  // before the table load
            atomicOr(ctl + CTL_BAD_CODE, 1u);
            code = 0;
        }
        const unsigned idx = (unsigned)(k * codebook_size + code);
        const unsigned e = alphabet[idx];
        const unsigned v = idx | ((e & 0xffu) << kClsShift) | ((e >> 8) << kCccShift);
        info[p] = v;
        return bits_of(v);
    }
};

struct InfoSrc {
    const unsigned* info;
    __device__ u64 operator()(int p) const { return bits_of(info[p]); }
};

struct LensSrc {
    const int* lens;
    __device__ u64 operator()(int p) const { return (u64)(unsigned)lens[p]; }
};

// pass 1: partials[tile] = sum of the tile's values
template <typename Src>
__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(Src src, int n, u64* partials) {
    __shared__ u64 wsum[kThreads / 64];
    const long long base = (long long)blockIdx.x * kTile;
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const long long p = base + i * kThreads + threadIdx.x;
        if (p < n) v += src((int)p);
    }
    u64 total;
    (void)block_exclusive(v, wsum, total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// pass 2, one workgroup: partials -> their exclusive scan, in place; out[n] = the grand total
__global__ __launch_bounds__(kThreads) void scan_partials_kernel(u64* partials, int n_tiles, u64* out, int n) {
    __shared__ u64 wsum[kThreads / 64];
    u64 carry = 0;
    for (int base = 0; base < n_tiles; base += kThreads) {
        const int i = base + threadIdx.x;
        const u64 v = i < n_tiles ? partials[i] : 0;
        u64 total;
        const u64 e = block_exclusive(v, wsum, total);
        if (i < n_tiles) partials[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// pass 3: out[p] = sum of the values before p
template <typename Src>
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(Src src, int n, const u64* partials, u64* out) {
    __shared__ u64 wsum[kThreads / 64];
    const long long base = (long long)blockIdx.x * kTile;
    u64 carry = partials[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const long long p = base + i * kThreads + threadIdx.x;
        const u64 v = p < n ? src((int)p) : 0;
        u64 total;
        const u64 e = block_exclusive(v, wsum, total);
        if (p < n) out[p] = carry + e;
        carry += total;
    }
}

struct ScatterArgs {
    const unsigned* info;
    const u64* scan;  // [N + 1]
    Seqs q;
    int n, n_special;
    int* symbols;
    int* symword;
    long long* offsets;
    int* word_first;  // [n_seq + 1]
    unsigned* ctl;
};

__global__ __launch_bounds__(kThreads) void scatter_kernel(ScatterArgs a) {
    const long long pl = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pl >= a.n) return;
    const int p = (int)pl;
    const unsigned v = a.info[p];
    const unsigned c = cls_of(v);
    if (c != KEEP_STARTER && c != KEEP_MARK && c != SPLIT) return;
    const u64 e = a.scan[p];
    const int kept = (int)(unsigned)e, splits = (int)(e >> 32);
    const int s = seq_of(a.q, p);
    const int word = splits + s;
    if (c == SPLIT) {
        a.offsets[word + 1] = kept;
        return;
    }
    int dest = kept;
    if (c == KEEP_MARK) {
        // the run of non-starters around p inside [lo, hi): rank among its kept marks
        const int lo = a.q.pos[s], hi = a.q.pos[s + 1];
        const unsigned my = v >> kCccShift;
        int len = 1, rank = 0, first = p;
        bool over = false;
        for (int r = p - 1; r >= lo; --r) {
            const unsigned u = a.info[r];
            if (!is_mark(u)) break;
            if (++len > kMaxRun) {
                over = true;
                break;
            }
            first = r;
            rank += cls_of(u) == KEEP_MARK && (u >> kCccShift) <= my;
        }
        for (int r = p + 1; r < hi && !over; ++r) {
            const unsigned u = a.info[r];
            if (!is_mark(u)) break;
            if (++len > kMaxRun) {
                over = true;
                break;
            }
            rank += cls_of(u) == KEEP_MARK && (u >> kCccShift) < my;
        }
        if (over)
            atomicOr(a.ctl + CTL_LONG_RUN, 1u);  // (dest stays the character's own kept rank: in bounds)
        else
            dest = (int)(unsigned)a.scan[first] + rank;
    }
    a.symbols[dest] = a.n_special + (int)(v & kIdxMask);
    a.symword[dest] = word;
}

// the first word of each sequence and its offset; s = n_seq gives the end (word count, symbol count)
__global__ __launch_bounds__(kThreads) void seq_words_kernel(ScatterArgs a) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s > a.q.n_seq) return;
    const u64 e = a.scan[a.q.pos[s]];
    const int word = (int)(e >> 32) + s;
    a.offsets[word] = (long long)(unsigned)e;
    a.word_first[s] = word;
}

// each word into the list of its merge-kernel form (one atomic per word), and the longest word
struct Lists {
    int* at[3];
};

__global__ __launch_bounds__(kThreads) void word_lists_kernel(const long long* offsets, const u64* scan_total, int n_seq,
                                                              Lists lists, unsigned* ctl) {
    const long long n_words = (long long)(*scan_total >> 32) + n_seq;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[CTL_KEPT] = (unsigned)*scan_total;
    for (long long w = (long long)blockIdx.x * kThreads + threadIdx.x; w < n_words;
         w += (long long)gridDim.x * kThreads) {
        const long long len = offsets[w + 1] - offsets[w];
        const int f = len <= kSmallCap ? 0 : len <= kLdsCap ? 1 : 2;
        const unsigned at = atomicAdd(ctl + CTL_COUNT0 + f, 1u);
        lists.at[f][at] = (int)w;
        if (f == 2) atomicMax(ctl + CTL_LONGEST, (unsigned)len);
    }
}

struct PackArgs {
    const int* ids;  // the merge kernels' output: word w at offsets[w], out_lens[w] of them
    const long long* offsets;
    const int* out_lens;
    const int* symword;
    const u64* packed;  // [n_words + 1] exclusive scan of out_lens
    int n_kept;
    int* out;
    const int* word_first;
    long long* seq_offsets;
    int n_seq;
};

__global__ __launch_bounds__(kThreads) void pack_kernel(PackArgs a) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.n_kept;
         i += (long long)gridDim.x * kThreads) {
        const int w = a.symword[i];
        const long long j = i - a.offsets[w];
        if (j < a.out_lens[w]) a.out[(long long)a.packed[w] + j] = a.ids[i];
    }
}

__global__ __launch_bounds__(kThreads) void seq_offsets_kernel(PackArgs a) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s > a.n_seq) return;
    a.seq_offsets[s] = (long long)a.packed[a.word_first[s]];
}

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the three scan passes over n values on s: out[0 .. n] = exclusive scan and total.  Reduce reads through `first`
// (which may have side effects: the classify), apply through `again`
template <typename First, typename Again>
int scan_on_stream(const First& first, const Again& again, int n, u64* partials, u64* out, hipStream_t s) {
    const unsigned tiles = blocks_for(n, kTile);
    if (tiles > 0) hipLaunchKernelGGL(scan_reduce_kernel<First>, dim3(tiles), dim3(kThreads), 0, s, first, n, partials);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kThreads), 0, s, partials, (int)tiles, out, n);
    if (tiles > 0)
        hipLaunchKernelGGL(scan_apply_kernel<Again>, dim3(tiles), dim3(kThreads), 0, s, again, n, partials, out);
    ENC_TRY(hipGetLastError());
    return MIMI_OK;
}

// everything on s; `table` and `ctl` are the caller's so that they outlive every copy queued here (the caller
// synchronises s, also when this fails half way).  *done = 0: stopped after the word model (a flag in ctl is set)
int encode_codes_on_stream(mimi_bpe_model* m, const int32_t* dev_codes, int64_t item_stride, int64_t row_stride,
                           const std::vector<int>& table, int N, int n_seq, int32_t* dev_out_ids,
                           int64_t* seq_offsets, hipStream_t s, unsigned* ctl, bool* done) {
    *done = false;
    const int64_t max_words = (int64_t)N + n_seq;      // every position a split character
    const int64_t max_long = N / (kSmallCap + 1) + 1;  // words of each of the two longer forms
    ENC_TRY(hipSetDevice(m->device));
    ENC_TRY(m->seqs.reserve(table.size() * 4));
    ENC_TRY(m->info.reserve((size_t)N * 4));
    ENC_TRY(m->scan.reserve((size_t)(max_words + 1) * 8));
    ENC_TRY(m->partials.reserve((size_t)(blocks_for(max_words, kTile) + 1) * 8));
    ENC_TRY(m->symbols.reserve((size_t)N * 4));
    ENC_TRY(m->out_ids.reserve((size_t)N * 4));
    ENC_TRY(m->symword.reserve((size_t)N * 4));
    ENC_TRY(m->offsets.reserve((size_t)(max_words + 1) * 8));
    ENC_TRY(m->out_lens.reserve((size_t)max_words * 4));
    ENC_TRY(m->words.reserve((size_t)(max_words + 2 * max_long) * 4));
    ENC_TRY(m->word_first.reserve((size_t)(n_seq + 1) * 4));
    ENC_TRY(m->seq_out.reserve((size_t)(n_seq + 1) * 8));
    ENC_TRY(m->bad.reserve(CTL_WORDS * 4));

    ENC_TRY(hipMemcpyAsync(m->seqs.p, table.data(), table.size() * 4, hipMemcpyHostToDevice, s));
    ENC_TRY(hipMemsetAsync(m->bad.p, 0, CTL_WORDS * 4, s));
    unsigned* dctl = (unsigned*)m->bad.p;
    const int* seqs = (const int*)m->seqs.p;
    const Seqs q{seqs, seqs + n_seq + 1, seqs + 2 * n_seq + 1, n_seq};
    u64* scan = (u64*)m->scan.p;
    u64* partials = (u64*)m->partials.p;
    long long* offsets = (long long*)m->offsets.p;

    // 1-3: classify and the scans of the keep and split bits
    const ClassifySrc classify{dev_codes, item_stride, row_stride, q, m->alphabet, m->num_codebooks,
                               m->codebook_size, (unsigned*)m->info.p, dctl};
    const InfoSrc bits{(const unsigned*)m->info.p};
    int rc = scan_on_stream(classify, bits, N, partials, scan, s);
    if (rc != MIMI_OK) return rc;
    // 4-5: symbols, word offsets, word lists
    const ScatterArgs sa{bits.info, scan, q, N, m->n_special, (int*)m->symbols.p, (int*)m->symword.p, offsets,
                         (int*)m->word_first.p, dctl};
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, s, sa);
    hipLaunchKernelGGL(seq_words_kernel, dim3(blocks_for((long long)n_seq + 1, kThreads)), dim3(kThreads), 0, s, sa);
    int* words = (int*)m->words.p;
    const Lists lists{{words, words + max_words, words + max_words + max_long}};
    hipLaunchKernelGGL(word_lists_kernel, dim3(std::min<unsigned>(blocks_for(max_words, kThreads), kMaxBlocks)),
                       dim3(kThreads), 0, s, (const long long*)offsets, (const u64*)(scan + N), n_seq, lists, dctl);
    ENC_TRY(hipGetLastError());
    // the one mid-way read-back: the flags, the three counts, the longest word
    ENC_TRY(hipMemcpyAsync(ctl, dctl, CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipStreamSynchronize(s));
    if (ctl[CTL_BAD_CODE] || ctl[CTL_LONG_RUN]) return MIMI_OK;
    // 6: the merge kernels
    const int64_t counts[3] = {ctl[CTL_COUNT0], ctl[CTL_COUNT0 + 1], ctl[CTL_COUNT0 + 2]};
    const int64_t n_words = counts[0] + counts[1] + counts[2];
    if (n_words > max_words || counts[1] > max_long || counts[2] > max_long)
        return fail(MIMI_ERR_STATE, "word counts %lld / %lld / %lld exceed their bounds", (long long)counts[0],
                    (long long)counts[1], (long long)counts[2]);
    const int* const list_at[3] = {lists.at[0], lists.at[1], lists.at[2]};
    rc = mimi::bpe::launch_forms(m, list_at, counts, (int64_t)ctl[CTL_LONGEST], s);
    if (rc != MIMI_OK) return rc;
    // 7: pack; the position scan is done with (the symbol count came back in ctl), its buffer takes the word scan
    const int n_kept = (int)ctl[CTL_KEPT];
    const LensSrc lens{(const int*)m->out_lens.p};
    rc = scan_on_stream(lens, lens, (int)n_words, partials, scan, s);
    if (rc != MIMI_OK) return rc;
    const PackArgs pa{(const int*)m->out_ids.p, offsets, lens.lens, (const int*)m->symword.p, scan, n_kept, dev_out_ids,
                      (const int*)m->word_first.p, (long long*)m->seq_out.p, n_seq};
    if (n_kept > 0)
        hipLaunchKernelGGL(pack_kernel, dim3(std::min<unsigned>(blocks_for(n_kept, kThreads), kMaxBlocks)),
                           dim3(kThreads), 0, s, pa);
    hipLaunchKernelGGL(seq_offsets_kernel, dim3(blocks_for((long long)n_seq + 1, kThreads)), dim3(kThreads), 0, s, pa);
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipMemcpyAsync(seq_offsets, m->seq_out.p, (size_t)(n_seq + 1) * 8, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipMemcpyAsync(ctl, dctl, 4, hipMemcpyDeviceToHost, s));  // the merge kernels' flag
    *done = true;
    return MIMI_OK;
}

}  // namespace

extern "C" int mimi_bpe_model_set_alphabet(mimi_bpe_model* m, int32_t n_special, int32_t num_codebooks,
                                           int32_t codebook_size, const uint8_t* cls, const uint8_t* ccc) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (!cls || !ccc) return fail(MIMI_ERR_INVALID_ARGUMENT, "null class arrays");
    if (n_special < 0 || num_codebooks < 1 || codebook_size < 1)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "bad alphabet shape %d x %d, %d special tokens", num_codebooks,
                    codebook_size, n_special);
    const int64_t n_base = (int64_t)num_codebooks * codebook_size;
    if ((int64_t)n_special + n_base > m->n_tokens)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "%d special tokens + %lld code characters exceed the model's %d tokens",
                    n_special, (long long)n_base, m->n_tokens);
    std::vector<unsigned short> table((size_t)n_base);
    for (int64_t i = 0; i < n_base; ++i) {
        if (cls[i] > SPLIT) return fail(MIMI_ERR_INVALID_ARGUMENT, "class %d of character %lld", cls[i], (long long)i);
        table[i] = (unsigned short)(cls[i] | (ccc[i] << 8));
    }
    std::lock_guard<std::mutex> lock(m->mu);
    m->plan_valid = false;
    ENC_TRY(hipSetDevice(m->device));
    unsigned short* dev = nullptr;
    ENC_TRY(hipMalloc(&dev, (size_t)n_base * 2));
    const hipError_t e = hipMemcpy(dev, table.data(), (size_t)n_base * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        ENC_TRY(e);
    }
    if (m->alphabet) (void)hipFree(m->alphabet);
    // spellings were checked against the alphabet they were set under (bpe_decode.hip): a new one drops them
    if (m->spell_off) (void)hipFree(m->spell_off);
    if (m->spell_idx) (void)hipFree(m->spell_idx);
    m->spell_off = m->spell_idx = nullptr;
    m->alphabet = dev;
    m->n_special = n_special;
    m->num_codebooks = num_codebooks;
    m->codebook_size = codebook_size;
    return MIMI_OK;
}

extern "C" int mimi_bpe_encode_codes(mimi_bpe_model* m, const int32_t* dev_codes, int32_t batch, int64_t item_stride,
                                     int64_t row_stride, const int64_t* frame_lengths, int64_t chunk_frames,
                                     int32_t* dev_out_ids, int64_t out_capacity, int64_t* seq_offsets, int64_t n_seq,
                                     void* stream) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (batch < 0 || chunk_frames < 0 || n_seq < 0 || item_stride < 0 || row_stride < 0 || !seq_offsets ||
        (batch > 0 && !frame_lengths))
        return fail(MIMI_ERR_INVALID_ARGUMENT, "bad batch arguments");
    if (n_seq > 0x3fffffffll) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^30 sequences");
    std::lock_guard<std::mutex> lock(m->mu);
    m->plan_valid = false;
    if (!m->alphabet) return fail(MIMI_ERR_STATE, "mimi_bpe_model_set_alphabet has not been called");
    const int K = m->num_codebooks;
    // the sequences: pos [n_seq + 1] | item [n_seq] | first frame [n_seq]
    int64_t count = 0, frames = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t T = frame_lengths[b];
        if (T < 0 || T > 0x7fffffffll) return fail(MIMI_ERR_INVALID_ARGUMENT, "frame length %lld of item %d", (long long)T, b);
        count += chunk_frames > 0 && T > 0 ? (T + chunk_frames - 1) / chunk_frames : 1;
        frames += T;
    }
    if (count != n_seq)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "n_seq %lld, the items give %lld sequences", (long long)n_seq,
                    (long long)count);
    const int64_t n_positions = frames * K;
    if (n_positions + n_seq >= (1ll << 31)) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^31 characters and sequences");
    if (out_capacity < n_positions)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "out_capacity %lld is below %d x %lld frames", (long long)out_capacity, K,
                    (long long)frames);
    if (n_positions > 0 && (!dev_codes || !dev_out_ids)) return fail(MIMI_ERR_INVALID_ARGUMENT, "null codes or out ids");
    m->last_words[0] = m->last_words[1] = m->last_words[2] = 0;
    if (n_positions == 0) {  // only empty sequences, one empty word each
        for (int64_t s = 0; s <= n_seq; ++s) seq_offsets[s] = 0;
        m->last_words[0] = n_seq;
        return MIMI_OK;
    }
    std::vector<int> table((size_t)(3 * n_seq + 1));
    int* pos = table.data();
    int* item = pos + n_seq + 1;
    int* frame = item + n_seq;
    int64_t at = 0, sq = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t T = frame_lengths[b];
        const int64_t step = chunk_frames > 0 && T > 0 ? chunk_frames : std::max<int64_t>(T, 1);
        for (int64_t f = 0; f == 0 || f < T; f += step, ++sq) {
            pos[sq] = (int)at;
            item[sq] = b;
            frame[sq] = (int)f;
            at += std::min(step, T - f) * K;
        }
    }
    pos[n_seq] = (int)at;
    hipStream_t s = (hipStream_t)stream;
    unsigned ctl[CTL_WORDS] = {0};
    bool done = false;
    const int rc = encode_codes_on_stream(m, dev_codes, item_stride, row_stride, table, (int)n_positions, (int)n_seq,
                                          dev_out_ids, seq_offsets, s, ctl, &done);
    if (rc != MIMI_OK) {
        (void)hipStreamSynchronize(s);  // nothing queued above may still read the host arrays
        return rc;
    }
    ENC_TRY(hipStreamSynchronize(s));
    if (ctl[CTL_BAD_CODE]) return fail(MIMI_ERR_INVALID_ARGUMENT, "a code is outside [0, %d)", m->codebook_size);
    if (ctl[CTL_LONG_RUN])
        return fail(MIMI_ERR_UNSUPPORTED,
                    "a run of combining marks is longer than MIMI_BPE_WORDS_MAX_RUN = %d characters", kMaxRun);
    if (!done) return fail(MIMI_ERR_STATE, "the encode stopped without a reason");
    if (ctl[CTL_BAD_SYMBOL]) return fail(MIMI_ERR_INVALID_ARGUMENT, "a symbol id is outside [0, %d)", m->n_tokens);
    return MIMI_OK;
}
