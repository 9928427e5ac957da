// Codec-BPE encoding on the GPU: words of symbol ids -> token ids (mimi_hip/bpe.py Encoder drives it).
//
// The reference applies its trained tokenizer one document at a time (pretraining-data/estimate_tokens.py:75,
// tokenizer(text)["input_ids"]); a 30 s chunk is one 3000-character word there, so HF tokenizers cannot go
// parallel inside it.  The rule is tokenizers' BPE model for one word (Word::merge_all, no dropout,
// ignore_merges off), restated in tests/bpe_encode_ref.py: among the adjacent pairs that have a merge take the
// lowest rank, on equal rank the leftmost, merge that one occurrence, repeat until no adjacent pair has a merge.
//
// Merge table: open addressing (linear probing) over 16-byte slots {right << 32 | left, rank << 32 | new id},
// built on the host at model creation, capacity a power of two >= 2 x merges; every probe loop is bounded by the
// capacity.  A 128k-vocabulary table is 4 MiB: it stays in L2.
//
// One 256-thread workgroup per word.  Per position p of the word: sym[p] (-1 once merged away), links nxt / prv
// to the live neighbours, and the cached (rank, new id) of the pair (p, nxt[p]).  Pairs are looked up once at
// the start, then only left and right of a merge.  One round: every thread takes the minimum of the packed key
// rank << 32 | p over its positions, a wave reduction and four LDS words give the round's pair, lanes 0 and 1 of
// wave 0 look up the two pairs the merge forms and lane 0 relinks.  At most n - 1 rounds for n symbols; no
// workgroup waits on another.  The arrays live in LDS for words up to MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS (16 bytes
// per symbol; a 3072-symbol form at 48 KiB keeps three workgroups on a CU, the 8192-symbol form holds the
// 6000-symbol 60 s x 8-codebook chunk); longer words run the same body on a global workspace sized from the
// longest word of the call.
//
// Merging every occurrence of the round's pair at once would be valid only where no pair formed in a round can
// out-rank the round (the trainer reuses ids, so a formed pair can have a lower rank than the merge forming it).
// Model creation makes that check and reports it (MIMI_BPE_INFO_FORMED_PAIR_OUTRANKS); the kernel merges one
// occurrence per round for every model, which is right without the proof.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "bpe_model.h"

namespace {

using mimi::bpe::fail;
using mimi::bpe::kLdsCap;
using mimi::bpe::kSmallCap;

constexpr unsigned kNoRank = 0xffffffffu;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr unsigned long long kMiss = ~0ull;  // rank half = kNoRank
constexpr unsigned kMaxId = (1u << 17) - 1;
constexpr int kThreads = 256;
constexpr int kMaxGlobalGroups = 1024;  // workgroups (and workspace slabs) of the global form

struct Slot {
    unsigned long long key, val;
};

struct TableView {
    const ulonglong2* slots;
    unsigned mask;
};

__host__ __device__ inline unsigned long long mix(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// (left in the low half: two adjacent symbols loaded as a pair are the key as they stand, with no half swap)
__host__ __device__ inline unsigned long long pair_key(int a, int b) {
    return ((unsigned long long)(unsigned)b << 32) | (unsigned)a;
}

// rank << 32 | new id of the merge (a, b), kMiss when there is none
__device__ __forceinline__ unsigned long long lookup(const TableView& t, int a, int b) {
    const unsigned long long key = pair_key(a, b);
    unsigned h = (unsigned)mix(key) & t.mask;
    for (unsigned probe = 0; probe <= t.mask; ++probe) {
        const ulonglong2 s = t.slots[h];
        if (s.x == key) return s.y;
        if (s.x == kEmptyKey) return kMiss;
        h = (h + 1) & t.mask;
    }
    return kMiss;
}

struct EncodeArgs {
    const int* symbols;        // every word, concatenated
    const long long* offsets;  // [all words + 1]
    const int* words;          // the words of this launch
    int n_words;
    int n_tokens;
    TableView t;
    int* out_ids;   // word w's ids at out_ids + offsets[w]
    int* out_lens;  // [all words]
    unsigned* bad;
};

template <typename Link>
struct Arrays {
    int* sym;
    unsigned* rank;
    int* nid;
    Link* nxt;
    Link* prv;
};

// One word, by the whole workgroup.  red: 4 words, scan: kThreads words of LDS.
template <typename Link>
__device__ void encode_word(const EncodeArgs& a, int w, const Arrays<Link>& A, unsigned long long* red,
                            unsigned* scan) {
    constexpr Link kEnd = (Link) ~(Link)0;
    const int tid = threadIdx.x;
    const long long off = a.offsets[w];
    const int n = (int)(a.offsets[w + 1] - off);
    const int* in = a.symbols + off;
    int* out = a.out_ids + off;

    // symbols and links; an id outside [0, n_tokens) is reported before any table access
    bool bad = false;
    for (int p = tid; p < n; p += kThreads) {
        const int s = in[p];
        if ((unsigned)s >= (unsigned)a.n_tokens) bad = true;
        A.sym[p] = s;
        A.nxt[p] = p + 1 < n ? (Link)(p + 1) : kEnd;
        A.prv[p] = p > 0 ? (Link)(p - 1) : kEnd;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            atomicOr(a.bad, 1u);
            a.out_lens[w] = 0;
        }
        return;
    }
    for (int p = tid; p < n; p += kThreads) {
        unsigned long long v = kMiss;
        if (p + 1 < n) v = lookup(a.t, A.sym[p], A.sym[p + 1]);
        A.rank[p] = (unsigned)(v >> 32);
        A.nid[p] = (int)(unsigned)v;
    }
    __syncthreads();

    for (int round = 0; round + 1 < n; ++round) {
        unsigned long long m = ~0ull;
        for (int p = tid; p < n; p += kThreads) {
            const unsigned long long k = ((unsigned long long)A.rank[p] << 32) | (unsigned)p;
            m = k < m ? k : m;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long x = __shfl_xor(m, o);
            m = x < m ? x : m;
        }
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kThreads / 64; ++i) m = red[i] < m ? red[i] : m;
        if ((unsigned)(m >> 32) == kNoRank) break;  // the same m in every thread
        if (tid < 64) {
            // wave 0, converged: every LDS read of the merge comes before the shuffle, every write after it
            const int p = (int)(unsigned)m;
            const Link q = A.nxt[p];
            const Link R = A.nxt[q], L = A.prv[p];
            const int id = A.nid[p];
            unsigned long long v = kMiss;
            if (tid == 0 && R != kEnd) v = lookup(a.t, id, A.sym[R]);
            if (tid == 1 && L != kEnd) v = lookup(a.t, A.sym[L], id);
            const unsigned long long vl = __shfl(v, 1);
            if (tid == 0) {
                A.sym[p] = id;
                A.nxt[p] = R;
                if (R != kEnd) A.prv[R] = (Link)p;
                A.sym[q] = -1;
                A.rank[q] = kNoRank;
                A.rank[p] = (unsigned)(v >> 32);
                A.nid[p] = (int)(unsigned)v;
                if (L != kEnd) {
                    A.rank[L] = (unsigned)(vl >> 32);
                    A.nid[L] = (int)(unsigned)vl;
                }
            }
        }
        __syncthreads();
    }

    // pack the live symbols: each thread owns a contiguous stretch, an inclusive scan of the 256 counts
    const int chunk = (n + kThreads - 1) / kThreads;
    const int p0 = min(n, tid * chunk), p1 = min(n, p0 + chunk);
    unsigned cnt = 0;
    for (int p = p0; p < p1; ++p) cnt += A.sym[p] >= 0;
    scan[tid] = cnt;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < kThreads; o <<= 1) {
        const unsigned x = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += x;
        __syncthreads();
    }
    unsigned k = scan[tid] - cnt;
    for (int p = p0; p < p1; ++p) {
        const int s = A.sym[p];
        if (s >= 0) out[k++] = s;
    }
    if (tid == kThreads - 1) a.out_lens[w] = (int)scan[tid];
    __syncthreads();  // the arrays and scan are reused by the next word of a grid-stride loop
}

template <int CAP>
__global__ __launch_bounds__(kThreads) void bpe_encode_lds_kernel(EncodeArgs a) {
    __shared__ int sym[CAP];
    __shared__ unsigned rank[CAP];
    __shared__ int nid[CAP];
    __shared__ unsigned short nxt[CAP];
    __shared__ unsigned short prv[CAP];
    __shared__ unsigned long long red[kThreads / 64];
    __shared__ unsigned scan[kThreads];
    if ((int)blockIdx.x >= a.n_words) return;
    const int w = a.words[blockIdx.x];
    if (a.offsets[w + 1] - a.offsets[w] > CAP) return;  // (the host sorts the words by length: never taken)
    const Arrays<unsigned short> A{sym, rank, nid, nxt, prv};
    encode_word<unsigned short>(a, w, A, red, scan);
}

// words above the LDS cap: the same body on a slab of `stride` positions per workgroup
__global__ __launch_bounds__(kThreads) void bpe_encode_global_kernel(EncodeArgs a, int* ws, long long stride) {
    __shared__ unsigned long long red[kThreads / 64];
    __shared__ unsigned scan[kThreads];
    int* slab = ws + (long long)blockIdx.x * 5 * stride;
    const Arrays<int> A{slab, reinterpret_cast<unsigned*>(slab + stride), slab + 2 * stride, slab + 3 * stride,
                        slab + 4 * stride};
    for (int i = blockIdx.x; i < a.n_words; i += gridDim.x) {
        const int w = a.words[i];
        if (a.offsets[w + 1] - a.offsets[w] > stride) continue;
        encode_word<int>(a, w, A, red, scan);
    }
}

}  // namespace

extern "C" void mimi_bpe_model_destroy(mimi_bpe_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    m->release_buffers();
    if (m->slots) (void)hipFree(m->slots);
    if (m->alphabet) (void)hipFree(m->alphabet);
    if (m->spell_off) (void)hipFree(m->spell_off);
    if (m->spell_idx) (void)hipFree(m->spell_idx);
    delete m;
}

extern "C" int mimi_bpe_model_create(int device, const int32_t* merges, int64_t n_merges, int32_t n_tokens,
                                     mimi_bpe_model** out) {
    if (!out) return fail(MIMI_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n_merges < 0 || (n_merges > 0 && !merges)) return fail(MIMI_ERR_INVALID_ARGUMENT, "bad merges arguments");
    if (n_tokens < 1 || (unsigned)n_tokens > kMaxId + 1)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "n_tokens %d must be in [1, %u]", n_tokens, kMaxId + 1);
    if (n_merges > (1ll << 30)) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^30 merges");
    unsigned long long cap = 1024;
    while (cap < 2ull * (unsigned long long)n_merges) cap <<= 1;
    std::vector<Slot> table(cap, Slot{kEmptyKey, 0});
    // formed[id] = the last rank whose merge produces id: a merge with such an id on either side and a lower
    // rank of its own is a pair that a round can form and that out-ranks that round
    std::vector<int64_t> formed(n_tokens, -1);
    int64_t n_pairs = 0;
    for (int64_t r = 0; r < n_merges; ++r) {
        const int32_t a = merges[3 * r], b = merges[3 * r + 1], c = merges[3 * r + 2];
        if (a < 0 || b < 0 || c < 0 || a >= n_tokens || b >= n_tokens || c >= n_tokens)
            return fail(MIMI_ERR_INVALID_ARGUMENT, "merge %lld (%d, %d) -> %d outside [0, %d)", (long long)r, a, b, c,
                        n_tokens);
        formed[c] = r;
        const unsigned long long key = pair_key(a, b);
        unsigned long long h = mix(key) & (cap - 1);
        for (unsigned long long probe = 0; probe < cap; ++probe) {
            if (table[h].key == kEmptyKey) {
                table[h].key = key;
                ++n_pairs;
            }
            if (table[h].key == key) {  // a repeated pair keeps its last rank, as tokenizers' merge map
                table[h].val = ((unsigned long long)r << 32) | (unsigned)c;
                break;
            }
            h = (h + 1) & (cap - 1);
        }
    }
    bool outranks = false;
    for (int64_t r = 0; r < n_merges && !outranks; ++r)
        outranks = formed[merges[3 * r]] > r || formed[merges[3 * r + 1]] > r;
    std::unique_ptr<mimi_bpe_model> m(new mimi_bpe_model());
    m->device = device;
    m->n_tokens = n_tokens;
    m->n_merges = n_merges;
    m->n_pairs = n_pairs;
    m->outranks = outranks;
    m->mask = (unsigned)(cap - 1);
    ENC_TRY(hipSetDevice(device));
    ENC_TRY(hipMalloc(&m->slots, cap * sizeof(Slot)));
    const hipError_t e = hipMemcpy(m->slots, table.data(), cap * sizeof(Slot), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->slots);
        m->slots = nullptr;
        ENC_TRY(e);
    }
    *out = m.release();
    return MIMI_OK;
}

extern "C" int mimi_bpe_model_info(const mimi_bpe_model* m, int32_t what, int64_t* value) {
    if (!m || !value) return fail(MIMI_ERR_INVALID_ARGUMENT, "null argument");
    switch (what) {
        case MIMI_BPE_INFO_PAIRS: *value = m->n_pairs; break;
        case MIMI_BPE_INFO_FORMED_PAIR_OUTRANKS: *value = m->outranks ? 1 : 0; break;
        case MIMI_BPE_INFO_TABLE_SLOTS: *value = (int64_t)m->mask + 1; break;
        case MIMI_BPE_INFO_LAST_WORDS_LDS_SMALL: *value = m->last_words[0]; break;
        case MIMI_BPE_INFO_LAST_WORDS_LDS: *value = m->last_words[1]; break;
        case MIMI_BPE_INFO_LAST_WORDS_GLOBAL: *value = m->last_words[2]; break;
        default: return fail(MIMI_ERR_INVALID_ARGUMENT, "unknown info key %d", what);
    }
    return MIMI_OK;
}

// (declared in bpe_model.h)
int mimi::bpe::launch_forms(mimi_bpe_model* m, const int* const lists[3], const int64_t counts[3], int64_t longest,
                            hipStream_t s) {
    const long long stride = (longest + 63) / 64 * 64;
    const int groups = (int)std::min<int64_t>(counts[2], kMaxGlobalGroups);
    if (groups > 0) ENC_TRY(m->ws.reserve((size_t)groups * 5 * (size_t)stride * 4));
    EncodeArgs a{};
    a.symbols = (const int*)m->symbols.p;
    a.offsets = (const long long*)m->offsets.p;
    a.n_tokens = m->n_tokens;
    a.t = TableView{m->slots, m->mask};
    a.out_ids = (int*)m->out_ids.p;
    a.out_lens = (int*)m->out_lens.p;
    a.bad = (unsigned*)m->bad.p;
    for (int f = 0; f < 3; ++f) {
        const int64_t nw = counts[f];
        m->last_words[f] = nw;
        if (nw == 0) continue;
        a.words = lists[f];
        a.n_words = (int)nw;
        if (f == 0)
            hipLaunchKernelGGL(bpe_encode_lds_kernel<kSmallCap>, dim3((unsigned)nw), dim3(kThreads), 0, s, a);
        else if (f == 1)
            hipLaunchKernelGGL(bpe_encode_lds_kernel<kLdsCap>, dim3((unsigned)nw), dim3(kThreads), 0, s, a);
        else
            hipLaunchKernelGGL(bpe_encode_global_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, a,
                               (int*)m->ws.p, stride);
        ENC_TRY(hipGetLastError());
    }
    return MIMI_OK;
}

// the copies in, the launches and the copies out, all on s; `lists` and `bad` are the caller's so that they
// outlive every copy queued here (the caller synchronises s, also when this fails half way)
static int encode_on_stream(mimi_bpe_model* m, const int32_t* symbols, const int64_t* word_offsets, int64_t n_words,
                            int32_t* out_ids, int32_t* out_lens, hipStream_t s, std::vector<int>* list,
                            unsigned* bad) {
    if (word_offsets[0] != 0) return fail(MIMI_ERR_INVALID_ARGUMENT, "word offsets must start at 0");
    const int64_t n_symbols = word_offsets[n_words];
    if (n_symbols >= (1ll << 31)) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^31 symbols");
    if (n_symbols > 0 && (!symbols || !out_ids)) return fail(MIMI_ERR_INVALID_ARGUMENT, "null symbols or out_ids");
    // the words of each kernel form
    int64_t longest = 0;
    for (int64_t w = 0; w < n_words; ++w) {
        const int64_t n = word_offsets[w + 1] - word_offsets[w];
        if (n < 0) return fail(MIMI_ERR_INVALID_ARGUMENT, "word offsets must be non-decreasing");
        list[n <= kSmallCap ? 0 : n <= kLdsCap ? 1 : 2].push_back((int)w);
        longest = std::max(longest, n);
    }
    ENC_TRY(hipSetDevice(m->device));
    const size_t sym_bytes = (size_t)std::max<int64_t>(n_symbols, 1) * 4;
    ENC_TRY(m->symbols.reserve(sym_bytes));
    ENC_TRY(m->out_ids.reserve(sym_bytes));
    ENC_TRY(m->offsets.reserve((size_t)(n_words + 1) * 8));
    ENC_TRY(m->words.reserve((size_t)n_words * 4));
    ENC_TRY(m->out_lens.reserve((size_t)n_words * 4));
    ENC_TRY(m->bad.reserve(4));
    if (n_symbols > 0) ENC_TRY(hipMemcpyAsync(m->symbols.p, symbols, (size_t)n_symbols * 4, hipMemcpyHostToDevice, s));
    ENC_TRY(hipMemcpyAsync(m->offsets.p, word_offsets, (size_t)(n_words + 1) * 8, hipMemcpyHostToDevice, s));
    ENC_TRY(hipMemsetAsync(m->bad.p, 0, 4, s));
    const int* lists[3];
    int64_t counts[3];
    size_t at = 0;
    for (int f = 0; f < 3; ++f) {
        const size_t nw = list[f].size();
        lists[f] = (const int*)m->words.p + at;
        counts[f] = (int64_t)nw;
        if (nw > 0) ENC_TRY(hipMemcpyAsync((int*)m->words.p + at, list[f].data(), nw * 4, hipMemcpyHostToDevice, s));
        at += nw;
    }
    const int rc = mimi::bpe::launch_forms(m, lists, counts, longest, s);
    if (rc != MIMI_OK) return rc;
    ENC_TRY(hipMemcpyAsync(bad, m->bad.p, 4, hipMemcpyDeviceToHost, s));
    ENC_TRY(hipMemcpyAsync(out_lens, m->out_lens.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, s));
    if (n_symbols > 0) ENC_TRY(hipMemcpyAsync(out_ids, m->out_ids.p, (size_t)n_symbols * 4, hipMemcpyDeviceToHost, s));
    return MIMI_OK;
}

extern "C" int mimi_bpe_encode(mimi_bpe_model* m, const int32_t* symbols, const int64_t* word_offsets,
                               int64_t n_words, int32_t* out_ids, int32_t* out_lens, void* stream) {
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (n_words < 0 || (n_words > 0 && (!word_offsets || !out_lens)))
        return fail(MIMI_ERR_INVALID_ARGUMENT, "bad word arguments");
    if (n_words > 0x7ffffffell) return fail(MIMI_ERR_UNSUPPORTED, "more than 2^31 - 2 words");
    std::lock_guard<std::mutex> lock(m->mu);
    m->plan_valid = false;
    m->last_words[0] = m->last_words[1] = m->last_words[2] = 0;
    if (n_words == 0) return MIMI_OK;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> list[3];
    unsigned bad = 0;
    const int rc = encode_on_stream(m, symbols, word_offsets, n_words, out_ids, out_lens, s, list, &bad);
    if (rc != MIMI_OK) {
        (void)hipStreamSynchronize(s);  // nothing queued above may still read the host arrays
        return rc;
    }
    ENC_TRY(hipStreamSynchronize(s));
    if (bad) return fail(MIMI_ERR_INVALID_ARGUMENT, "a symbol id is outside [0, %d)", m->n_tokens);
    return MIMI_OK;
}
