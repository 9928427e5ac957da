// The device BPE model shared by bpe_encode.hip (merge table, merge kernels, host-word entry), bpe_words.hip
// (device word model, device-to-device entry), bpe_decode.hip (ids back to codes) and bpe_decode_stream.hip (the same,
// chunk by chunk per slot).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "../../include/mimi_hip.h"
#include "kernels.h"

namespace mimi {
namespace bpe {

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return mimi::set_error_message(code, buf);
}

// a device buffer that grows on demand; a failed growth leaves it empty and usable
struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// words of each merge-kernel form: at most kSmallCap symbols, at most MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS, longer
constexpr int kSmallCap = 3072;
constexpr int kLdsCap = MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS;

}  // namespace bpe
}  // namespace mimi

struct mimi_bpe_model {
    int device = 0;
    int n_tokens = 0;
    int64_t n_merges = 0, n_pairs = 0;
    bool outranks = false;
    ulonglong2* slots = nullptr;
    unsigned mask = 0;
    std::mutex mu;  // one encode at a time per model (the buffers below)
    mimi::bpe::Buffer symbols, offsets, words, out_ids, out_lens, bad, ws;
    int64_t last_words[3] = {0, 0, 0};  // of the last encode: small LDS form, large LDS form, global form
    // device word model (bpe_words.hip): the alphabet table (class | ccc << 8 per code character) and its buffers
    unsigned short* alphabet = nullptr;
    int n_special = 0, num_codebooks = 0, codebook_size = 0;
    mimi::bpe::Buffer seqs, info, scan, partials, symword, word_first, seq_out;
    // decoder (bpe_decode.hip): the spelling of every id (offsets [n_tokens + 1], alphabet indices), the buffers of
    // the last mimi_bpe_decode_plan and what mimi_bpe_decode_write needs of it.  Any other call clears plan_valid
    int* spell_off = nullptr;
    int* spell_idx = nullptr;
    int64_t spell_version = 0;  // counts mimi_bpe_model_set_spellings calls: a decode stream serves the tables it was made on
    mimi::bpe::Buffer dec_seq_ids, dec_id_start, dec_cpos, dec_info, dec_rank, dec_begin, dec_frames, dec_partials,
        dec_ctl;
    bool plan_valid = false;
    int plan_chars = 0, plan_seqs = 0;
    int64_t plan_max_frames = 0;
    void release_buffers() {
        for (mimi::bpe::Buffer* b : {&symbols, &offsets, &words, &out_ids, &out_lens, &bad, &ws, &seqs, &info, &scan,
                                     &partials, &symword, &word_first, &seq_out, &dec_seq_ids, &dec_id_start, &dec_cpos,
                                     &dec_info, &dec_rank, &dec_begin, &dec_frames, &dec_partials, &dec_ctl})
            b->release();
    }
};

#define ENC_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            (void)hipGetLastError();                                                                    \
            return mimi::bpe::fail(_e == hipErrorOutOfMemory ? MIMI_ERR_OUT_OF_MEMORY : MIMI_ERR_HIP,   \
                                   "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                               \
    } while (0)

namespace mimi {
namespace bpe {

// The merge kernels over the model's device buffers, on s: symbols, offsets, out_ids, out_lens and bad hold the
// call's words (bad cleared); lists[f] is the device list of the counts[f] words of form f, `longest` the longest
// word of the call.  Sizes the global workspace and sets last_words.
int launch_forms(mimi_bpe_model* m, const int* const lists[3], const int64_t counts[3], int64_t longest,
                 hipStream_t s);

}  // namespace bpe
}  // namespace mimi
