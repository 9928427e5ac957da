// Codec-BPE decoding chunk by chunk: a pool of slots, each the filter state of one session; a step takes a ragged batch
// of new token ids for any subset of the slots and writes the whole frames those ids complete, laid out as
// mimi_decode_stream_step_ragged takes them (mimi_bpe_decode_stream_*; mimi_hip/bpe.py IdStream drives them).
//
// The rules of bpe_decode.hip are causal -- the keep filter looks only leftwards, the begin drop depends on the first
// character and on how many were kept so far, the end drop is "the partial last frame is not out yet" -- so a slot
// needs only: `expected` (or "fresh": no character seen since the reset), the begin-drop characters still owed, and at
// most K - 1 pending codes.  Per character (alphabet index idx, codebook cb = idx / codebook_size) of the new ids:
//     fresh: expected = cb, owed = (K - cb) % K
//     cb != expected: dropped;  else expected = (expected + 1) % K and, if owed, --owed and dropped;
//     else pend += idx - len(pend) * codebook_size; K pending codes are one frame.
//
// One launch per step, one workgroup per listed item, no workgroup waits on another.  The workgroup walks the item's
// ids in tiles of kThreads (a + scan of the spelling lengths, as pass 1 of the batch form, held in LDS) and the tile's
// characters in rows of kThreads: a character finds its id by binary search in the tile, loads its alphabet index,
// the MapOp scan (bpe_scan.h) gives `expected` before it -- the carry into a row is the constant map to the slot's
// `expected`, the first character of a fresh slot is the `first` map --, a + scan of the keep bits gives its rank.  A
// kept character past the owed ones is number q of the slot's open frames (q counts from the pending codes): the
// frames a row completes go to codes[item][q % K][q / K], the pending codes in front of them to their column, what
// is left is the new pending codes (LDS, then the slot's record).  Every carry -- between rows, between tiles and
// between steps -- is combine(earlier, later) in that order: the operator does not commute.
#include <algorithm>
#include <vector>

#include "bpe_model.h"
#include "bpe_scan.h"

namespace {

using mimi::bpe::AddOp;
using mimi::bpe::block_exclusive;
using mimi::bpe::char_map;
using mimi::bpe::fail;
using mimi::bpe::find_in;
using mimi::bpe::kIdentityMap;
using mimi::bpe::kMaxK;
using mimi::bpe::MapOp;
using mimi::bpe::u64;

constexpr int kThreads = mimi::bpe::kScanThreads;
constexpr int kItemWords = 4;  // per item, host -> device: slot, ids, start fresh, unused
constexpr int kOutWords = 4;   // per item, device -> host: frames, pending codes (-1: fresh), bad id, unused
constexpr int kMaxStepIds = 1 << 20;

// a slot's device record: expected (-1: fresh), owed, npend, pend[K]
__host__ __device__ inline int record_words(int K) { return 3 + K; }

struct StepArgs {
    const int* items;  // [m][kItemWords]
    const int* ids;    // row i: the ids of item i
    long long ids_row_stride;
    const int* spell_off;  // [n_tokens + 1]
    const int* spell_idx;
    int n_tokens, K, codebook_size;
    int* state;  // [slots][record_words(K)]
    int* codes;  // [m][K][max_frames]
    int max_frames;
    int* out;  // [m][kOutWords]
};

__global__ __launch_bounds__(kThreads) void bpe_decode_stream_step_kernel(StepArgs a) {
    __shared__ u64 wtot[kThreads / 64];
    __shared__ int id_start[kThreads + 1];  // first character of each id of the tile; [kThreads] = the tile's characters
    __shared__ int id_spell[kThreads];      // spell_off of each id of the tile
    __shared__ int pend[kMaxK];
    __shared__ int first_cb;
    const int tid = threadIdx.x, item = blockIdx.x, K = a.K;
    const int slot = a.items[item * kItemWords], count = a.items[item * kItemWords + 1];
    const bool restart = a.items[item * kItemWords + 2] != 0;
    int* rec = a.state + (long long)slot * record_words(K);
    const int* ids = a.ids + (long long)item * a.ids_row_stride;
    int* codes = a.codes + (long long)item * K * a.max_frames;

    const int expected0 = restart ? -1 : rec[0];
    bool fresh = expected0 < 0;
    int owed = restart ? 0 : rec[1];
    int q0 = restart ? 0 : rec[2];  // the slot's open-frame characters so far: the pending codes, then this step's
    if (tid < kMaxK) pend[tid] = !restart && tid < K ? rec[3 + tid] : 0;
    __syncthreads();

    const AddOp add{};
    const MapOp maps{K};
    u64 carry = fresh ? kIdentityMap : (u64)expected0 * 0x1111111111111111ull;  // the constant map to `expected`
    int bad = 0;
#pragma unroll 1
    for (int base = 0; base < count; base += kThreads) {
        // the tile's ids: an id is checked against [0, n_tokens) BEFORE the table load
        int len = 0, spell = 0;
        if (base + tid < count) {
            const int id = ids[base + tid];
            if ((unsigned)id >= (unsigned)a.n_tokens) {
                bad = 1;
            } else {
                spell = a.spell_off[id];
                len = a.spell_off[id + 1] - spell;
            }
        }
        u64 chars;
        const u64 start = block_exclusive(add, (u64)(unsigned)len, wtot, chars);
        id_start[tid] = (int)start;
        id_spell[tid] = spell;
        if (tid == 0) id_start[kThreads] = (int)chars;
        __syncthreads();
        const int n = (int)chars;
#pragma unroll 1
        for (int row = 0; row < n; row += kThreads) {
            const int p = row + tid;
            const bool live = p < n;
            const bool first = fresh && p == 0;  // of the slot's session (fresh is uniform over the workgroup)
            unsigned idx = 0, cb = 0;
            if (live) {
                const int j = find_in(id_start, kThreads, p);
                idx = (unsigned)a.spell_idx[id_spell[j] + (p - id_start[j])];
                cb = idx / (unsigned)a.codebook_size;
            }
            if (first) first_cb = (int)cb;
            u64 row_map;
            const u64 before = block_exclusive(maps, live ? char_map(cb, first, K) : kIdentityMap, wtot, row_map);
            if (fresh) owed = (K - first_cb) % K;
            // the state before a character that is not the first of its session is a constant map
            const bool keep = live && (first || ((unsigned)maps.combine(carry, before) & 15u) == cb);
            carry = maps.combine(carry, row_map);
            fresh = false;
            u64 kept;
            const int rank = (int)block_exclusive(add, (u64)keep, wtot, kept);
            const int drop = min(owed, (int)kept);
            const int q1 = q0 + (int)kept - drop;
            const int frame0 = q0 / K, frame1 = q1 / K, npend = q0 % K;
            const int old = tid < npend ? pend[tid] : 0;
            __syncthreads();  // pend is read before this row's tail overwrites it
            if (frame1 > frame0 && tid < npend && frame0 < a.max_frames)
                codes[(long long)tid * a.max_frames + frame0] = old;
            if (keep && rank >= drop) {
                const int q = q0 + (rank - drop);
                const int k = q % K, t = q / K;
                const int code = (int)idx - k * a.codebook_size;
                if (t >= frame1) pend[k] = code;
                else if (t < a.max_frames) codes[(long long)k * a.max_frames + t] = code;
            }
            __syncthreads();
            owed -= drop;
            q0 = q1;
        }
    }
    const int any_bad = __syncthreads_or(bad);
    if (tid == 0) {
        rec[0] = fresh ? -1 : (int)((unsigned)carry & 15u);
        rec[1] = owed;
        rec[2] = q0 % K;
        a.out[item * kOutWords] = q0 / K;
        a.out[item * kOutWords + 1] = fresh ? -1 : q0 % K;
        a.out[item * kOutWords + 2] = any_bad;
    }
    if (tid < K) rec[3 + tid] = pend[tid];
}

}  // namespace

struct mimi_bpe_decode_stream {
    mimi_bpe_model* model = nullptr;
    int slots = 0, max_step_ids = 0, K = 0, codebook_size = 0, n_tokens = 0, lmax = 0;
    int64_t spell_version = 0;
    std::mutex mu;
    int *state = nullptr, *dev_items = nullptr, *dev_out = nullptr;  // device
    int* host = nullptr;  // pinned: [slots][kItemWords] items, then [slots][kOutWords] results
    std::vector<int> pending;  // per slot: npend, -1 fresh
    std::vector<char> restart, refused, listed;
};

namespace {

void release(mimi_bpe_decode_stream* st) {
    if (st->state) (void)hipFree(st->state);
    if (st->dev_items) (void)hipFree(st->dev_items);
    if (st->dev_out) (void)hipFree(st->dev_out);
    if (st->host) (void)hipHostFree(st->host);
    delete st;
}

int64_t max_frames_for(const mimi_bpe_decode_stream* st, int64_t ids) {
    return (st->K - 1 + ids * st->lmax) / st->K;
}

int alloc_stream(mimi_bpe_decode_stream* st) {
    const size_t n = (size_t)st->slots;
    ENC_TRY(hipMalloc(&st->state, n * record_words(st->K) * 4));
    ENC_TRY(hipMemset(st->state, 0, n * record_words(st->K) * 4));
    ENC_TRY(hipMalloc(&st->dev_items, n * kItemWords * 4));
    ENC_TRY(hipMalloc(&st->dev_out, n * kOutWords * 4));
    ENC_TRY(hipHostMalloc(reinterpret_cast<void**>(&st->host), n * (kItemWords + kOutWords) * 4, hipHostMallocDefault));
    return MIMI_OK;
}

void reset_one(mimi_bpe_decode_stream* st, int slot) {
    st->pending[slot] = -1;
    st->restart[slot] = 1;  // the next step of the slot ignores its device record
    st->refused[slot] = 0;
}

}  // namespace

extern "C" int mimi_bpe_decode_stream_create(mimi_bpe_model* m, int32_t slots, int32_t max_step_ids,
                                             mimi_bpe_decode_stream** out) {
    if (!out) return fail(MIMI_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!m) return fail(MIMI_ERR_INVALID_ARGUMENT, "null model");
    if (slots < 1) return fail(MIMI_ERR_INVALID_ARGUMENT, "a stream has at least 1 slot, got %d", slots);
    if (max_step_ids < 1 || max_step_ids > kMaxStepIds)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "max_step_ids %d must be in [1, %d]", max_step_ids, kMaxStepIds);
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->spell_off) return fail(MIMI_ERR_STATE, "mimi_bpe_model_set_spellings has not been called");
    if (m->num_codebooks > kMaxK)
        return fail(MIMI_ERR_UNSUPPORTED, "%d codebooks: the device filter packs at most %d", m->num_codebooks, kMaxK);
    ENC_TRY(hipSetDevice(m->device));
    std::vector<int> off((size_t)m->n_tokens + 1);
    ENC_TRY(hipMemcpy(off.data(), m->spell_off, off.size() * 4, hipMemcpyDeviceToHost));
    int lmax = 0;
    for (int i = 0; i < m->n_tokens; ++i) lmax = std::max(lmax, off[i + 1] - off[i]);
    if ((int64_t)max_step_ids * lmax + m->num_codebooks >= (1ll << 31))
        return fail(MIMI_ERR_UNSUPPORTED, "%d ids of up to %d characters spell 2^31 characters or more", max_step_ids,
                    lmax);
    mimi_bpe_decode_stream* st = new mimi_bpe_decode_stream;
    st->model = m;
    st->slots = slots;
    st->max_step_ids = max_step_ids;
    st->K = m->num_codebooks;
    st->codebook_size = m->codebook_size;
    st->n_tokens = m->n_tokens;
    st->lmax = lmax;
    st->spell_version = m->spell_version;
    st->pending.assign((size_t)slots, -1);
    st->restart.assign((size_t)slots, 1);
    st->refused.assign((size_t)slots, 0);
    st->listed.assign((size_t)slots, 0);
    const int rc = alloc_stream(st);
    if (rc != MIMI_OK) {
        release(st);
        return rc;
    }
    *out = st;
    return MIMI_OK;
}

extern "C" int64_t mimi_bpe_decode_stream_max_frames(const mimi_bpe_decode_stream* st, int32_t ids) {
    if (!st || ids < 0) return -1;
    return max_frames_for(st, ids);
}

extern "C" int mimi_bpe_decode_stream_step(mimi_bpe_decode_stream* st, const int32_t* slots, const int32_t* counts,
                                           int32_t m, const int32_t* dev_ids, int64_t ids_row_stride,
                                           int32_t* dev_codes, int32_t max_frames, int32_t* frames_out, void* stream) {
    if (!st) return fail(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    if (!slots || !counts || !frames_out) return fail(MIMI_ERR_INVALID_ARGUMENT, "null slots, counts or frames_out");
    std::lock_guard<std::mutex> lock(st->mu);
    if (m < 1 || m > st->slots) return fail(MIMI_ERR_INVALID_ARGUMENT, "a step lists 1 .. %d slots, got %d", st->slots, m);
    int longest = 0, ok = 0;  // ok: the leading items whose slot is in range and not listed before
    while (ok < m && slots[ok] >= 0 && slots[ok] < st->slots && !st->listed[slots[ok]]) st->listed[slots[ok++]] = 1;
    for (int i = 0; i < ok; ++i) st->listed[slots[i]] = 0;
    if (ok < m)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "slots must be distinct and in [0, %d): item %d is slot %d", st->slots,
                    ok, slots[ok]);
    for (int i = 0; i < m; ++i) {
        if (counts[i] < 0 || counts[i] > st->max_step_ids)
            return fail(MIMI_ERR_INVALID_ARGUMENT, "item %d brings %d ids, a step takes 0 .. %d per slot", i, counts[i],
                        st->max_step_ids);
        longest = std::max(longest, counts[i]);
    }
    if (max_frames < 0 || max_frames < max_frames_for(st, longest))
        return fail(MIMI_ERR_INVALID_ARGUMENT, "max_frames %d is below the %lld frames that %d ids can complete",
                    max_frames, (long long)max_frames_for(st, longest), longest);
    if (longest > 0 && !dev_ids) return fail(MIMI_ERR_INVALID_ARGUMENT, "null ids");
    if (m > 1 && ids_row_stride < longest)
        return fail(MIMI_ERR_INVALID_ARGUMENT, "ids_row_stride %lld is below the longest item's %d ids",
                    (long long)ids_row_stride, longest);
    if (max_frames > 0 && !dev_codes) return fail(MIMI_ERR_INVALID_ARGUMENT, "null codes");
    for (int i = 0; i < m; ++i)
        if (st->refused[slots[i]])
            return fail(MIMI_ERR_STATE, "slot %d took a token id outside [0, %d): reset it", slots[i], st->n_tokens);

    mimi_bpe_model* mod = st->model;
    std::lock_guard<std::mutex> model_lock(mod->mu);  // set_spellings / set_alphabet free the tables
    if (!mod->spell_off || mod->spell_version != st->spell_version)
        return fail(MIMI_ERR_STATE, "the model's spellings were replaced after this stream was made");
    ENC_TRY(hipSetDevice(mod->device));
    hipStream_t s = (hipStream_t)stream;
    int* items = st->host;
    int* result = st->host + (size_t)st->slots * kItemWords;
    for (int i = 0; i < m; ++i) {
        items[i * kItemWords] = slots[i];
        items[i * kItemWords + 1] = counts[i];
        items[i * kItemWords + 2] = st->restart[slots[i]];
        items[i * kItemWords + 3] = 0;
    }
    const StepArgs a{st->dev_items,       dev_ids,         ids_row_stride, mod->spell_off, mod->spell_idx,
                     st->n_tokens,        st->K,           st->codebook_size, st->state,   dev_codes,
                     max_frames,          st->dev_out};
    hipError_t e = hipMemcpyAsync(st->dev_items, items, (size_t)m * kItemWords * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bpe_decode_stream_step_kernel, dim3((unsigned)m), dim3(kThreads), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(result, st->dev_out, (size_t)m * kOutWords * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // also when something failed: nothing queued may still read `items`
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        for (int i = 0; i < m; ++i) st->refused[slots[i]] = 1;  // their records may be half written
        ENC_TRY(e);
    }
    bool bad = false;
    for (int i = 0; i < m; ++i) bad = bad || result[i * kOutWords + 2] != 0;
    if (bad) {
        for (int i = 0; i < m; ++i) st->refused[slots[i]] = 1;
        return fail(MIMI_ERR_INVALID_ARGUMENT, "a token id is outside [0, %d)", st->n_tokens);
    }
    for (int i = 0; i < m; ++i) {
        frames_out[i] = result[i * kOutWords];
        st->pending[slots[i]] = result[i * kOutWords + 1];
        st->restart[slots[i]] = 0;
    }
    return MIMI_OK;
}

extern "C" int mimi_bpe_decode_stream_reset(mimi_bpe_decode_stream* st) {
    if (!st) return fail(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    std::lock_guard<std::mutex> lock(st->mu);
    for (int b = 0; b < st->slots; ++b) reset_one(st, b);
    return MIMI_OK;
}

extern "C" int mimi_bpe_decode_stream_reset_slot(mimi_bpe_decode_stream* st, int32_t slot) {
    if (!st) return fail(MIMI_ERR_INVALID_ARGUMENT, "null stream");
    std::lock_guard<std::mutex> lock(st->mu);
    if (slot < 0 || slot >= st->slots) return fail(MIMI_ERR_INVALID_ARGUMENT, "slot %d is outside [0, %d)", slot, st->slots);
    reset_one(st, slot);
    return MIMI_OK;
}

extern "C" int32_t mimi_bpe_decode_stream_slot_pending(mimi_bpe_decode_stream* st, int32_t slot) {
    if (!st) return -2;
    std::lock_guard<std::mutex> lock(st->mu);
    if (slot < 0 || slot >= st->slots) return -2;
    return st->pending[slot];
}

extern "C" void mimi_bpe_decode_stream_destroy(mimi_bpe_decode_stream* st) {
    if (!st) return;
    (void)hipSetDevice(st->model->device);
    release(st);
}
