/*
 * mimi_hip.h — C ABI of the MI355X-native Mimi encode engine (libmimi_hip.so).
 *
 * Drop-in boundary.  The reference's encode path is Python over third-party
 * ``transformers.MimiModel`` (no native FFI of its own); the entry points below are what a binding of that
 * path binds, one for one:
 *
 *   mimi_create_from_dir (one call), or mimi_config_from_json + mimi_create / mimi_load_safetensors /
 *   mimi_set_weight / mimi_finalize
 *       replace ``MimiModel.from_pretrained(model_id).to(device).eval()``
 *       (/root/reference/emilia-mimi/process_shard.py:57-60; TF/modeling_mimi.py:1186-1228)
 *   mimi_encode
 *       replaces ``MimiModel.encode(input_values, padding_mask, num_quantizers)``
 *       (/root/reference/emilia-mimi/process_shard.py:82-85, :124-127; TF/modeling_mimi.py:1297-1386)
 *   mimi_rvq_encode
 *       replaces ``MimiSplitResidualVectorQuantizer.encode`` (TF/modeling_mimi.py:1099-1126) on a given
 *       pre-quantizer embedding (used by the bit-exact quantizer parity test)
 *   mimi_encoded_length
 *       replaces ``MimiModel.get_encoded_length`` (TF/modeling_mimi.py:1265-1278)
 *   mimi_enable_decode / mimi_create_from_dir_flags(MIMI_CREATE_DECODE) + mimi_decode
 *       replace ``MimiModel.decode(audio_codes).audio_values`` (librispeech-mimi/utils.py:72-81 ``str_to_audio``;
 *       TF/modeling_mimi.py:1408-1458); mimi_rvq_decode replaces ``MimiSplitResidualVectorQuantizer.decode``
 *       (TF/modeling_mimi.py:1128-1137)
 *
 * Conventions: plain pointers and sizes, no exceptions, no torch types.  Every function returns a
 * mimi_status; on failure ``mimi_last_error()`` (thread-local) describes it.  Device pointers are HIP
 * device memory on the engine's device; ``stream`` is a hipStream_t (NULL = the HIP null stream);
 * work is enqueued asynchronously on it, ordered after earlier work on that stream.
 * One engine may be shared by several host threads (calls are serialised by a per-engine mutex).
 */
#ifndef MIMI_HIP_H
#define MIMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mimi_engine mimi_engine;

typedef enum mimi_status {
    MIMI_OK = 0,
    MIMI_ERR_INVALID_ARGUMENT = 1, /* ValueError in the reference (e.g. K > 32, channels not in {1,2}) */
    MIMI_ERR_HIP = 2,              /* a HIP runtime call failed */
    MIMI_ERR_OUT_OF_MEMORY = 3,    /* workspace allocation failed (reference: torch OOM) */
    MIMI_ERR_WEIGHTS = 4,          /* missing / mis-shaped parameter */
    MIMI_ERR_UNSUPPORTED = 5,      /* config outside the implemented architecture family */
    MIMI_ERR_IO = 6,               /* checkpoint file unreadable / malformed */
    MIMI_ERR_STATE = 7             /* call order violated (e.g. encode before finalize) */
} mimi_status;

/* Encode-path fields of MimiConfig (TF/configuration_mimi.py:86-123). */
typedef struct mimi_config {
    int32_t sampling_rate;          /* 24000 */
    int32_t audio_channels;         /* 1 */
    int32_t hidden_size;            /* 512 */
    int32_t num_filters;            /* 64 */
    int32_t num_ratios;             /* 4 */
    int32_t upsampling_ratios[8];   /* {8, 6, 5, 4}; the encoder uses them reversed */
    int32_t kernel_size;            /* 7 */
    int32_t last_kernel_size;       /* 3 */
    int32_t residual_kernel_size;   /* 3 */
    int32_t compress;               /* 2 */
    int32_t codebook_size;          /* 2048 */
    int32_t codebook_dim;           /* 256 */
    int32_t num_quantizers;         /* 32 */
    int32_t num_semantic_quantizers;/* 1 */
    int32_t vq_hidden_dim;          /* 256 */
    int32_t num_hidden_layers;      /* 8 */
    int32_t intermediate_size;      /* 2048 */
    int32_t num_attention_heads;    /* 8 */
    int32_t head_dim;               /* 64 */
    int32_t sliding_window;         /* 250 */
    int32_t downsample_kernel;      /* 4 = 2 * encodec_frame_rate / frame_rate */
    int32_t downsample_stride;      /* 2 */
    float norm_eps;                 /* 1e-5 */
    float rope_theta;               /* 10000 */
    float codebook_eps;             /* 1e-5 (MimiEuclideanCodebook epsilon) */
} mimi_config;

/* Fill *cfg with the kyutai/mimi defaults. */
void mimi_config_default(mimi_config* cfg);

/*
 * Read a checkpoint's HF config.json (path = the file, or a directory holding it) into *cfg: the encode-path
 * fields of MimiConfig (TF/configuration_mimi.py:86-175; unknown keys ignored, absent keys keep the defaults,
 * rope_theta at the top level or in rope_parameters, head_dim null -> hidden_size / num_attention_heads, the
 * downsample kernel from frame_rate).  MIMI_ERR_IO: unreadable file, malformed JSON or a field of the wrong type;
 * MIMI_ERR_UNSUPPORTED: an architecture outside the kyutai/mimi family (stereo, non-causal convs, GQA, ...).
 * Host-only: no device is touched.
 */
int mimi_config_from_json(const char* path, mimi_config* cfg);

/*
 * The one-call constructor: weights_dir is a checkpoint directory in the HF layout (config.json, optional, and
 * *.safetensors -- the first in byte order, as the Python host's sorted glob picks it) or a lone .safetensors file
 * (default config).  Reads the config, creates the engine on `device`, loads the safetensors file and finalizes:
 * = mimi_config_from_json + mimi_create + mimi_load_safetensors + mimi_finalize, with the engine released again on
 * any failure (*out stays NULL; mimi_last_error names the first failure).
 */
int mimi_create_from_dir(const char* weights_dir, int device, mimi_engine** out);

/* Create an engine on HIP device `device` (cfg NULL = defaults).  Weights are supplied next. */
int mimi_create(const mimi_config* cfg, int device, mimi_engine** out);

/* Supply one parameter by its HF name, fp32, host memory, copied. */
int mimi_set_weight(mimi_engine* e, const char* name, const float* host_data, int64_t numel);

/* Read every encode-path parameter from a safetensors file (F32 tensors, HF names); after mimi_enable_decode the
 * decode-path parameters too (otherwise the decoder half of a full checkpoint is skipped unread). */
int mimi_load_safetensors(mimi_engine* e, const char* path);

/* Check all parameters are present, re-lay them out for the kernels and upload them. */
int mimi_finalize(mimi_engine* e);

/*
 * Encode `batch` mono waveforms of `length` samples (device f32, [batch][length], already padded to a
 * common length by the caller as EncodecFeatureExtractor does) into `num_quantizers` codebooks.
 * dev_codes: device int32 [batch][num_quantizers][mimi_encoded_length(length)].
 * num_quantizers <= 0 means config.num_quantizers (the reference default, TF/modeling_mimi.py:1335).
 */
int mimi_encode(mimi_engine* e, const float* dev_audio, int32_t batch, int64_t length,
                int32_t num_quantizers, int32_t* dev_codes, void* stream);

/*
 * mimi_encode in two halves, for callers that overlap host work (ingest, H2D of the next batch, writing
 * codes) with the encode: mimi_encode_async enqueues the encode on `stream` and returns a ticket without
 * waiting; mimi_encode_wait(ticket) waits for it on the host and, in f16x3, applies the overflow check (and the
 * per-item fallback when a fixed activation scale overflowed) before returning.  dev_codes is valid once the
 * wait returns; dev_audio and dev_codes must stay allocated, and dev_audio unmodified, until then (the wait may
 * re-encode from dev_audio: a fixed f16x3 scale overflowed, or the persistent RVQ chain gave up).  At most 16 encodes per engine may be
 * in flight; each ticket is waited exactly once.  mimi_encode = mimi_encode_async + mimi_encode_wait.
 *
 * The encode runs on a stream of the engine's, ordered after `stream` at the call (everything enqueued on `stream`
 * before the call is visible to it), or on `stream` itself; nothing enqueued on `stream` AFTER the call is ordered
 * behind the encode.  Only mimi_encode_wait orders anything behind it: read dev_codes, and reuse dev_audio, after the
 * wait has returned.  Two encodes kept in flight (enqueue the next, then wait for the previous) run side by side in the
 * engine's two lanes -- each lane its own workspace, maxima, captured graphs and stream -- so the second workspace
 * exists only for callers that overlap encodes (option "lanes" below; mimi_lane_encodes counts per lane).
 */
int mimi_encode_async(mimi_engine* e, const float* dev_audio, int32_t batch, int64_t length, int32_t num_quantizers,
                      int32_t* dev_codes, void* stream, int64_t* ticket);
int mimi_encode_wait(mimi_engine* e, int64_t ticket);

/*
 * mimi_encode from and to HOST memory in one call: host_audio f32 [batch][length] (any host memory), host_codes
 * int32 [batch][num_quantizers][mimi_encoded_length(length)].  The engine copies the audio to its own device buffer,
 * encodes and copies the codes back on `stream`, synchronising the host once -- the per-utterance caller's path
 * (MimiEncoder.encode_audio_chunk once per utterance: librispeech-mimi/process_librispeech_dev-test.py:136-141,
 * mls-en-mimi-pretrain/process_shard.py:302-307) without a framework tensor per step.  Same codes as mimi_encode.
 */
int mimi_encode_host(mimi_engine* e, const float* host_audio, int32_t batch, int64_t length, int32_t num_quantizers,
                     int32_t* host_codes, void* stream);

/*
 * Ragged batch: item b's samples are dev_audio[b][0 .. lengths[b]) (rows max_length apart; samples past lengths[b]
 * are never read), lengths a HOST int64 array, 1 <= lengths[b] <= max_length.  Each item is encoded exactly as
 * mimi_encode(dev_audio[b], 1, lengths[b], ...) would encode it alone -- its codes, frames [0,
 * mimi_encoded_length(lengths[b])) of dev_codes[b], are bit for bit those -- while the batch runs as one pass
 * whose kernels skip every item's rows past its own length.  Frames past an item's own are unspecified.
 * dev_codes: device int32 [batch][num_quantizers][mimi_encoded_length(max_length)].
 *   - per-utterance callers (batch-1 semantics: mls-en-mimi-pretrain/process_shard.py:302-307,
 *     librispeech-mimi/process_librispeech_dev-test.py:136-141) pass each utterance's length;
 *   - pad-to-longest callers (EncodecFeatureExtractor padding, emilia-mimi/process_shard.py:113-139) pass
 *     min(max_length, 1920 ceil(L_b / 1920)) over the zero-padded batch: every frame the caller keeps,
 *     ceil(L_b / 1920), depends only on samples below that length (all convs causal, no extra padding at a
 *     multiple of 1920), so the kept frames are the padded batch's -- without the padding's compute.
 * In f16x3 the overflow check applies per batch; a fallback re-encodes each item alone at its length.
 */
int mimi_encode_ragged(mimi_engine* e, const float* dev_audio, const int64_t* lengths, int32_t batch,
                       int64_t max_length, int32_t num_quantizers, int32_t* dev_codes, void* stream);
int mimi_encode_ragged_async(mimi_engine* e, const float* dev_audio, const int64_t* lengths, int32_t batch,
                             int64_t max_length, int32_t num_quantizers, int32_t* dev_codes, void* stream,
                             int64_t* ticket);

/*
 * The quantizer alone: dev_embedding is the pre-quantizer embedding, device f32 [frames][hidden_size]
 * (frame-major, i.e. the reference's [B, 512, T] transposed to [B*T, 512]).  dev_codes: int32
 * [num_quantizers][frames].
 */
int mimi_rvq_encode(mimi_engine* e, const float* dev_embedding, int64_t frames, int32_t num_quantizers,
                    int32_t* dev_codes, void* stream);

/*
 * ---- decode: codes -> waveform (replaces mimi_model.decode(codes).audio_values of str_to_audio,
 * librispeech-mimi/utils.py:58-81; MimiModel.decode, TF/modeling_mimi.py:1388-1458) ----
 *
 * Decode weights are opt-in, so that encode-only users and partial checkpoints load as before.
 * mimi_enable_decode (before mimi_finalize) adds the decode-path parameters -- decoder.*, upsample.conv.weight,
 * decoder_transformer.*, the quantizer's two output_proj.weight -- to the expected set: mimi_load_safetensors then
 * reads them (F32; weight-norm forms resolved as for encode) and mimi_finalize checks, re-lays out and uploads them
 * (a missing or mis-shaped one: MIMI_ERR_WEIGHTS naming it).  After mimi_finalize: MIMI_ERR_STATE.
 * mimi_create_from_dir_flags = mimi_create_from_dir with flags; MIMI_CREATE_DECODE calls mimi_enable_decode.
 *
 * ARITHMETIC: decode always runs the fp32-MFMA form of the GEMMs (MIMI_PRECISION_F32) and the fp32 attention and
 * residual-block kernels, whatever mimi_set_precision says -- no activation scales, hence no calibration, overflow
 * read-back or fallback.  Mixed-length batches: mimi_decode_ragged.  Chunk by chunk on a KV cache:
 * mimi_decode_stream_*.  Not provided: f16x3 decode, hipGraph replay of decode.
 */
enum { MIMI_CREATE_DECODE = 1 };
int mimi_enable_decode(mimi_engine* e);
int mimi_create_from_dir_flags(const char* weights_dir, int device, uint32_t flags, mimi_engine** out);

/* Samples produced for `frames` 12.5 Hz frames: frames x 2 x prod(upsampling_ratios) = 1920 x frames by default
 * (the length of MimiModel.decode(codes).audio_values, TF/modeling_mimi.py:1388-1406). */
int64_t mimi_decoded_length(int64_t frames);
int64_t mimi_decoded_length_cfg(const mimi_config* cfg, int64_t frames);

/*
 * MimiModel.decode (TF/modeling_mimi.py:1408-1458): dev_codes device int32 [batch][num_quantizers][frames],
 * 1 <= num_quantizers <= the checkpoint's levels; dev_audio device f32 [batch][mimi_decoded_length(frames)].
 * Synchronises `stream` once, to read the bounds flag: a code outside [0, codebook_size) is never used as an index
 * (the kernel substitutes 0) and the call returns MIMI_ERR_INVALID_ARGUMENT ("code outside [0, codebook_size)") with
 * dev_audio unspecified.  An engine without decode weights: MIMI_ERR_STATE.  Serialised by the engine's mutex like
 * encode.  Grows a decode workspace of its own (MIMI_ERR_OUT_OF_MEMORY leaves the engine usable).  An item's samples
 * do not depend on its batch-mates.
 */
int mimi_decode(mimi_engine* e, const int32_t* dev_codes, int32_t batch, int64_t frames, int32_t num_quantizers,
                float* dev_audio, void* stream);

/*
 * The quantizer's decode alone, the mirror of mimi_rvq_encode (MimiSplitResidualVectorQuantizer.decode,
 * TF/modeling_mimi.py:1128-1137): dev_codes int32 [num_quantizers][frames] -> dev_embedding f32
 * [frames][hidden_size] (the reference's [B, 512, T] transposed).  Bounds flag and errors as mimi_decode.
 */
int mimi_rvq_decode(mimi_engine* e, const int32_t* dev_codes, int64_t frames, int32_t num_quantizers,
                    float* dev_embedding, void* stream);

/* Device bytes mimi_decode's workspace needs for (batch, frames); grown on demand. */
int64_t mimi_decode_workspace_bytes(const mimi_engine* e, int32_t batch, int64_t frames);

/*
 * Ragged decode: a mixed-length batch of codes in one pass, the mirror of mimi_encode_ragged.  dev_codes device int32
 * [batch][num_quantizers][max_frames], item b's codes being [:, :frame_lengths[b]]; codes past an item's length are
 * NEVER READ (any bit pattern there neither raises the bounds flag nor changes a sample).  dev_audio device f32
 * [batch][mimi_decoded_length(max_frames)]: item b's samples are the first mimi_decoded_length(frame_lengths[b]) of its
 * row, the rest of the row is left untouched.  frame_lengths: host, [batch], each in [1, max_frames] (else
 * MIMI_ERR_INVALID_ARGUMENT, nothing launched); it need not outlive the call.
 * CONTRACT: item b's samples are bitwise those of mimi_decode on that item alone at its own length, whatever its
 * batch-mates, their lengths, the batch size and the engine's history.  Every stage works on packed rows (item b's
 * rows of a stage at rate factor f start at row f x sum(frame_lengths[:b])): the number of launches does not depend on
 * batch, no stage touches rows past an item's length, and every item gets the attention kernel it would run alone.
 * State, num_quantizers, bad-code (inside an item's length), MIMI_ERR_UNSUPPORTED (a row index past 32 bits, at any
 * rate, over the sum of the lengths) and MIMI_ERR_OUT_OF_MEMORY behaviour as mimi_decode; synchronous, serialised by
 * the engine's mutex, fp32 MFMA always, no lane, no graph; shares mimi_decode's workspace.  Taps are stored packed,
 * [1][f x sum of lengths][channels]; profiling records mimi_decode's stages (with items on both sides of the
 * 256-row attention threshold, two dec_attention records per layer).
 */
int mimi_decode_ragged(mimi_engine* e, const int32_t* dev_codes, const int64_t* frame_lengths /* host, [batch] */,
                       int32_t batch, int64_t max_frames, int32_t num_quantizers, float* dev_audio, void* stream);

/* Device bytes mimi_decode_ragged's workspace needs: mimi_decode_workspace_bytes(e, 1, sum of frame_lengths) plus the
 * int tables (under 4096 + 256 x batch bytes).  -1 on a NULL argument, batch <= 0 or a length < 1. */
int64_t mimi_decode_ragged_workspace_bytes(const mimi_engine* e, const int64_t* frame_lengths, int32_t batch);

/*
 * Streaming decode: codes to audio chunk by chunk on a KV cache.  A decode stream holds the decoder's state for `batch`
 * items (SLOTS: each with its own position, stepped all together or any subset at a time, see below): per item the few rows every causal stage reads from in front of a chunk (1 row of the
 * embedding for the upsample, 6 of the transformer output for decoder.layers.0, 1 per up conv, 2 per residual block,
 * 2 for the last conv) and, per transformer layer, a ring of the rotated key / value rows of the last
 * sliding_window - 1 + 2 max_step_frames 25 Hz rows.  All of it is device memory owned by the stream
 * (mimi_decode_stream_state_bytes: constant over the stream's life); a step's cost does not depend on the position.
 *
 * mimi_decode_stream_step: dev_codes device int32 [batch][num_quantizers][n], 1 <= n <= max_step_frames, the next n
 * frames of every item; dev_audio device f32 [batch][mimi_decoded_length(n)].
 * CONTRACT: the samples of frames [p, p + n) are bitwise the same under ANY split of the sequence into steps (one
 * step of everything included), and an item's do not depend on its batch-mates or on other streams; against
 * MimiModel.decode of the whole sequence they are within the project's activation tolerance (the per-row arithmetic
 * is mimi_decode's; the attention reduces in another order).
 * Errors: an engine without decode weights and num_quantizers as mimi_decode; n outside [1, max_step_frames]:
 * MIMI_ERR_INVALID_ARGUMENT, state untouched; a code outside [0, codebook_size): MIMI_ERR_INVALID_ARGUMENT as
 * mimi_decode (never used as an index), after which the stream returns MIMI_ERR_STATE until mimi_decode_stream_reset
 * (the engine and other streams stay usable); a position whose 25 Hz row no longer fits a float32 exactly (2^24 rows,
 * 7.8 days of audio): MIMI_ERR_UNSUPPORTED.  Synchronises `stream` once to read the bounds flag.  Serialised by the
 * engine's mutex: steps of several streams may interleave with each other and with mimi_decode, mimi_decode_ragged and
 * mimi_encode*; a step runs in mimi_decode's workspace and never grows the engine's shared RoPE tables (captured
 * encode graphs survive).  Taps and profiling as mimi_decode, holding the step's rows; the history forms record as
 * upsample_dw_hist_kernel, resblock_hist_kernel<...>, final_conv_hist_kernel and attention_stream_kernel.
 * mimi_decode_stream_reset: back to position 0 with zero state (a fresh stream).  Destroy every stream before its
 * engine.
 *
 * SLOTS.  Item b of the state is slot b: its own position, carries and rings, so sessions that start and end at
 * different times share one stream.  mimi_decode_stream_step_slots advances the m slots it lists (`slots`: host, m
 * distinct values in [0, batch), any order, need not outlive the call), all by the same n frames: item i of dev_codes
 * [m][num_quantizers][n] and of dev_audio [m][mimi_decoded_length(n)] belongs to slot slots[i], whose position moves
 * from p to p + n.  Nothing of an unlisted slot is read or written.  CONTRACT: a listed slot's samples are bitwise those
 * of a batch = 1 stream fed that slot's sequence since its last reset, under any split of that sequence into steps,
 * whatever the other slots are and where they stand, in any order of `slots`, whatever was called in between.  The
 * launches are those of a lock-step step (the same count, whatever m, n and the positions); the kernels that touch the
 * state record as attention_stream_slots_kernel, attention_stream_append_slots_kernel and stream_carry_slots_kernel.
 * mimi_decode_stream_step means "all slots, in order 0 .. batch - 1" and is allowed at any time: while all slots stand
 * at one position it is the lock-step pass (the kernels and bits it always had), otherwise a slot step.
 * Errors of step_slots, with nothing launched and no state touched, MIMI_ERR_INVALID_ARGUMENT: m outside [1, batch], a
 * slot outside [0, batch), a slot listed twice, n outside [1, max_step_frames], a NULL pointer; MIMI_ERR_UNSUPPORTED: a
 * listed slot past the 2^24-row limit.  A code outside [0, codebook_size) fails the call as above; the flag is one word,
 * so every slot LISTED IN THAT CALL (mimi_decode_stream_step: every slot) then returns MIMI_ERR_STATE when listed again,
 * until mimi_decode_stream_reset_slot on it or mimi_decode_stream_reset; unlisted slots stay usable and their samples
 * are unaffected.
 * mimi_decode_stream_reset_slot: the slot back to position 0 with zero carries -- what follows equals a fresh stream;
 * its neighbours are untouched.  (The slot's rings are not cleared: a query reads only ring rows written since the
 * reset.)  mimi_decode_stream_position: the largest slot position (the position, on a stream stepped in lock-step);
 * mimi_decode_stream_slot_position: one slot's, -1 for NULL or a slot out of range.  mimi_decode_stream_state_bytes
 * counts the state; a slot step's two tables (12 bytes per slot) are a separate allocation.
 *
 * A COUNT PER SLOT.  mimi_decode_stream_step_ragged is step_slots with item i (slot slots[i]) advancing by its own
 * frames[i] frames (`frames`: host, [m], need not outlive the call), 1 <= frames[i] <= max_frames <= max_step_frames; a
 * slot with nothing to do is not listed.  The I/O layout is mimi_decode_ragged's: dev_codes [m][num_quantizers]
 * [max_frames] and dev_audio [m][1920 max_frames], padded rows.  Codes past an item's frames[i] are never read (any
 * value), samples past 1920 frames[i] never written; afterwards slot slots[i] stands frames[i] further.  CONTRACT as
 * step_slots, over per-item counts: a listed slot's samples are bitwise those of a batch = 1 stream fed that slot's
 * sequence since its last reset, under any split, in any order of `slots`, whatever counts its neighbours bring.
 * Counts that all equal max_frames make the call step_slots itself (the same launches under the same recorded names).
 * Otherwise the launches are those of a slot step plus one more small host-to-device copy (the step's tables: per
 * stage the items' rows and first rows, see mimi_stream_step_layout), whatever the counts, and the per-item kernels
 * record as rvq_decode_ragged_kernel, upsample_dw_hist_ragged_kernel, attention_stream_ragged_kernel,
 * attention_stream_append_ragged_kernel, stream_carry_ragged_kernel, resblock_hist_ragged_kernel<...>,
 * final_conv_hist_ragged_kernel and the packed-rows GEMM instantiations; the workspace is sized by the sum of the
 * counts.  Errors as step_slots (the 2^24-row limit per listed slot at its own count; a bad code inside an item's
 * frames fails every slot listed in that call), and MIMI_ERR_INVALID_ARGUMENT with nothing launched and no state
 * touched also for a NULL `frames`, a count outside [1, max_frames] and max_frames outside [1, max_step_frames].
 * Taps of a step with unequal counts: every stage and "audio" without carry rows or padding, packed
 * [1][sum of rows][C] as mimi_decode_ragged's.
 * Not provided: a count of 0, hipGraph capture of a step, f16x3 arithmetic.
 */
typedef struct mimi_decode_stream mimi_decode_stream;
int mimi_decode_stream_create(mimi_engine* e, int32_t batch, int32_t num_quantizers, int32_t max_step_frames,
                              mimi_decode_stream** out);
int mimi_decode_stream_step(mimi_decode_stream* st, const int32_t* dev_codes /* [batch][num_quantizers][n] */, int32_t n,
                            float* dev_audio /* [batch][1920 n] */, void* stream);
int mimi_decode_stream_step_slots(mimi_decode_stream* st, const int32_t* slots /* host, [m] */, int32_t m,
                                  const int32_t* dev_codes /* [m][num_quantizers][n] */, int32_t n,
                                  float* dev_audio /* [m][1920 n] */, void* stream);
int mimi_decode_stream_step_ragged(mimi_decode_stream* st, const int32_t* slots /* host, [m] */,
                                   const int32_t* frames /* host, [m] */, int32_t m, int32_t max_frames,
                                   const int32_t* dev_codes /* [m][num_quantizers][max_frames] */,
                                   float* dev_audio /* [m][1920 max_frames] */, void* stream);
/*
 * The layout of a ragged stream step, host-only (no device, no engine): for `direction` and the items' counts
 * (`frames`: [m], each in [1, max_frames]) the stages that carry rows from step to step, in the order of the stream's
 * carries, and the step's workspace.  Stage j has carry_rows[j] = H rows per item in front of the chunk, rate[j] = f
 * rows per frame and channels[j] floats per row; item i's block [H + f frames[i]][C] starts at row first_row[j * m + i]
 * = H i + f off[i] (off = the prefix sum of frames) of one packed tensor that begins byte_offset[j] bytes into the
 * workspace, and has row_count[j * m + i] rows: blocks in order, back to back.  The arrays of stages hold
 * MIMI_STREAM_MAX_STAGES entries, first_row and row_count MIMI_STREAM_MAX_STAGES * m.  *workspace_bytes: what the step
 * needs of the engine's decode workspace (taps != 0: with the engine's taps on) -- sized by the sum of the counts, so
 * never more than the step of m items at max_frames each, and equal to it when every count is max_frames.
 * MIMI_STREAM_DECODE: the embedding (H 1, f 1), the transformer output (6, 2), then per ratio the up conv's input (1)
 * and output (2), the last conv's input (2).  MIMI_STREAM_ENCODE: conv 0's carry (one row of 8 samples per item, f 0:
 * the audio itself stays in the caller's rows), then per ratio the residual block's input (H 2, f 1920 / the ratios so
 * far) and the down conv's (H r), the final conv's input (2, 2) and the downsample's (2, 2).  MIMI_ERR_INVALID_ARGUMENT: a NULL pointer, another direction, m outside [1, 65535], max_frames
 * outside [1, 2^20], a count outside [1, max_frames].
 */
#define MIMI_STREAM_DECODE 0
#define MIMI_STREAM_ENCODE 1
#define MIMI_STREAM_MAX_STAGES 16
int mimi_stream_step_layout(const mimi_config* cfg, int32_t direction, const int32_t* frames /* [m] */, int32_t m,
                            int32_t max_frames, int32_t taps, int32_t* n_stages, int32_t* carry_rows, int32_t* rate,
                            int32_t* channels, int64_t* byte_offset, int64_t* first_row, int64_t* row_count,
                            int64_t* workspace_bytes);
int mimi_decode_stream_reset(mimi_decode_stream* st);
int mimi_decode_stream_reset_slot(mimi_decode_stream* st, int32_t slot);
int64_t mimi_decode_stream_position(const mimi_decode_stream* st);    /* frames decoded so far (the largest slot's) */
int64_t mimi_decode_stream_slot_position(const mimi_decode_stream* st, int32_t slot); /* -1: NULL / out of range */
int64_t mimi_decode_stream_state_bytes(const mimi_decode_stream* st); /* constant over the stream's life */
void mimi_decode_stream_destroy(mimi_decode_stream* st);

/*
 * Streaming encode: audio to codes chunk by chunk on a KV cache -- the decode stream's other direction.  An encode
 * stream holds the encoder's state for `batch` items (SLOTS, as in the decode stream): per item the rows every causal
 * stage reads from in front of a chunk (6 samples of audio for conv 0, kept as the last 8; per stage s 2 rows [C_s] of
 * the residual block's raw input and r_s rows [C_s] of its ELU'd output for the k = 2 r_s, stride r_s down conv, with
 * C_s = 64, 128, 256, 512 and r_s = 4, 5, 6, 8; 2 rows [1024] for the final conv; 2 rows [512] of the transformer output
 * for the downsample) and, per transformer layer, a ring of the rotated key / value rows of the last
 * sliding_window - 1 + 2 max_step_frames 25 Hz rows.  One device allocation owned by the stream
 * (mimi_encode_stream_state_bytes: constant over its life).  A fresh or reset slot is all zeros at position 0, with one
 * exception: the reference pads the downsample with copies of the sequence's FIRST ROW (mode = "replicate"), so on a
 * step that finds a slot at position 0 that slot's downsample carry is filled from row 0 of that step's transformer
 * output -- never from what a previous session left.
 *
 * mimi_frame_samples_cfg: F = 2 x prod(upsampling_ratios) = 1920 samples, one 12.5 Hz frame (cfg NULL: the defaults).
 * mimi_encode_stream_step: dev_audio device f32 [batch][F n], 1 <= n <= max_step_frames, the next n WHOLE frames of
 * every item; dev_codes device int32 [batch][num_quantizers][n].  Fed whole frames every strided length divides
 * exactly, so no conv pads on the right, which is what MimiModel.encode(use_streaming=True) computes with its
 * MimiConv1dPaddingCache: the codes of frames [p, p + n) are those of mimi_encode of any sequence that contains those
 * frames whole (the pre-quantizer embedding within the project's activation tolerance; codes differ only at near-ties).
 * BIT CONTRACT: (1) a slot's codes for frames [p, p + n) are bitwise the same under ANY split of its sequence into steps;
 * (2) they are bitwise those of a batch = 1 stream fed that sequence since its last reset; (3) whatever the other slots
 * do, in any order of `slots`, whatever was called in between.  (Per output row every kernel runs the same instruction
 * sequence whatever the chunk -- conv 0's history form keeps one fmaf chain per output in tap order -- and the stream
 * attention's reduction order is a function of the query's absolute row alone.)
 * Arithmetic: fp32 MFMA always, whatever mimi_set_precision says: no activation scales, no calibration, no overflow
 * read-back, no lanes, no graphs.  A step runs under the engine mutex on the caller's stream, in mimi_decode's
 * workspace (grown on demand; MIMI_ERR_OUT_OF_MEMORY leaves the state untouched), with RoPE rows built on the host per
 * step in pinned memory the stream owns: the engine's shared RoPE table never grows and captured encode graphs survive.
 * It synchronises `stream` before it returns.  The RVQ runs the per-level kernels.  Works on an encode-only engine.
 * The number of launches depends on num_quantizers only: not on m, n or the positions.
 * Taps under mimi_encode's names, holding the step's rows: conv0, res{s}_elu, down{s} / down3_elu, encoder, the per-layer
 * qkv / att / oproj / ff / xfmr, downsample, proj.  Profiling stages are prefixed encs_; the history and stream forms
 * record as conv0_hist_kernel<64, 7>, resblock_hist_kernel<...>, attention_stream_kernel,
 * attention_stream_append_kernel, stream_carry_kernel and stream_ds_rows_kernel (a slot step: the *_slots_kernel forms).
 *
 * mimi_encode_stream_step_slots: the m listed slots (`slots`: host, m distinct values in [0, batch), any order), all by
 * the same n frames: item i of dev_audio [m][F n] and dev_codes [m][num_quantizers][n] belongs to slot slots[i]; nothing
 * of an unlisted slot is read or written.  mimi_encode_stream_step means "all slots, in order 0 .. batch - 1": while
 * all slots share a position it is the lock-step pass under the lock-step kernel names, otherwise a slot step.
 * Errors, with nothing launched and no state touched: MIMI_ERR_INVALID_ARGUMENT for m outside [1, batch], a slot out
 * of range or listed twice, n outside [1, max_step_frames], a NULL pointer; MIMI_ERR_UNSUPPORTED for a listed slot past
 * 2^24 25 Hz rows.  There is no bounds flag: audio has no invalid values to index with.  Non-finite samples make that
 * slot's codes unspecified -- but inside [0, codebook_size) -- from that step until mimi_encode_stream_reset_slot (the
 * carries and the ring hold them); other slots are bitwise unaffected; the engine does not look for them.  A step that
 * fails after it touched the state (a HIP error) makes its listed slots return MIMI_ERR_STATE until reset.
 * mimi_encode_stream_reset / _reset_slot: back to position 0 and a fresh state (all slots / one, its neighbours
 * untouched).  mimi_encode_stream_position: the largest slot position; _slot_position: one slot's, -1 for NULL or a slot
 * out of range.  Destroy every stream before its engine.
 * Not provided: a tail shorter than a frame (the caller keeps it for the next step; mimi_encode's last, right-padded
 * frame of a length that is not a multiple of F has no streamed equivalent here), a count of 0 in a ragged step
 * (mimi_encode_stream_step_ragged, below), f16x3 arithmetic, hipGraph capture of a step, the reference's encoder_past_key_values / padding_cache objects.
 */
typedef struct mimi_encode_stream mimi_encode_stream;
int mimi_encode_stream_create(mimi_engine* e, int32_t batch, int32_t num_quantizers, int32_t max_step_frames,
                              mimi_encode_stream** out);
int mimi_encode_stream_step(mimi_encode_stream* st, const float* dev_audio /* [batch][F n] */, int32_t n,
                            int32_t* dev_codes /* [batch][num_quantizers][n] */, void* stream);
int mimi_encode_stream_step_slots(mimi_encode_stream* st, const int32_t* slots /* host, [m] */, int32_t m,
                                  const float* dev_audio /* [m][F n] */, int32_t n,
                                  int32_t* dev_codes /* [m][num_quantizers][n] */, void* stream);
/* A count per slot, as mimi_decode_stream_step_ragged: item i (slot slots[i]) advances by frames[i] whole frames, 1 <=
 * frames[i] <= max_frames <= max_step_frames.  dev_audio [m][F max_frames] and dev_codes [m][num_quantizers][max_frames]
 * are padded rows: audio past F frames[i] samples is never read (NaN there is harmless), codes past frames[i] are never
 * written.  A listed slot's codes are bitwise those of a batch = 1 stream fed that slot's audio since its last reset,
 * whatever counts its neighbours bring; a fresh slot's replicate padding comes from its own first row.  Counts that all
 * equal max_frames make the call step_slots itself.  Otherwise the launches are those of a slot step plus one small
 * host-to-device copy, recorded as conv0_hist_ragged_kernel, resblock_hist_ragged_kernel<...>, the packed-rows GEMMs
 * (..., 102> / 103> / 104> / 109>), attention_stream_ragged_kernel, attention_stream_append_ragged_kernel,
 * stream_ds_rows_ragged_kernel and stream_carry_ragged_kernel; the RVQ kernels store through a per-frame map into the
 * padded rows.  Errors as step_slots, and MIMI_ERR_INVALID_ARGUMENT with nothing launched and no state touched for a
 * NULL pointer, a count outside [1, max_frames] and max_frames outside [1, max_step_frames].  Taps of a step with unequal
 * counts are packed [1][sum of rows][C]. */
int mimi_encode_stream_step_ragged(mimi_encode_stream* st, const int32_t* slots /* host, [m] */,
                                   const int32_t* frames /* host, [m] */, int32_t m, int32_t max_frames,
                                   const float* dev_audio /* [m][F max_frames] */,
                                   int32_t* dev_codes /* [m][num_quantizers][max_frames] */, void* stream);
int mimi_encode_stream_reset(mimi_encode_stream* st);
int mimi_encode_stream_reset_slot(mimi_encode_stream* st, int32_t slot);
int64_t mimi_encode_stream_position(const mimi_encode_stream* st);    /* frames encoded so far (the largest slot's) */
int64_t mimi_encode_stream_slot_position(const mimi_encode_stream* st, int32_t slot); /* -1: NULL / out of range */
int64_t mimi_encode_stream_state_bytes(const mimi_encode_stream* st); /* constant over the stream's life */
void mimi_encode_stream_destroy(mimi_encode_stream* st);
int64_t mimi_frame_samples_cfg(const mimi_config* cfg);               /* F: samples of one frame */

/*
 * Host-only: the weight re-layout that turns a causal MimiConvTranspose1d (kernel 2 ratio, stride ratio, weight
 * [cin][cout][2 ratio]; TF/modeling_mimi.py:349-405) into a causal k = 2 convolution with ratio x cout phase-major
 * output channels: out [ratio * cout][2 * cin], out[p cout + co][ci] = w[ci][co][p + ratio] (the x[t - 1] tap),
 * out[p cout + co][cin + ci] = w[ci][co][p] (the x[t] tap).  What mimi_finalize applies; tests check it against
 * torch's conv_transpose1d.  No device is touched.
 */
int mimi_upconv_relayout(const float* w, int32_t cin, int32_t cout, int32_t ratio, float* out);

/*
 * Arithmetic of the conv / linear GEMMs (the residual VQ distances are always exact fp32):
 *   MIMI_PRECISION_F32     v_mfma_f32_32x32x2_f32 (fp32 MFMA)
 *   MIMI_PRECISION_BF16X6  fp32 emulated on the bf16 matrix cores: both operands split into 3 bf16 planes,
 *                          6 plane products accumulated in fp32 (~fp32 accuracy, 2.7x MFMA rate)
 *   MIMI_PRECISION_BF16X3  2 planes, 3 products (~1e-5 relative, 5.3x MFMA rate)
 *   MIMI_PRECISION_F16X3   (default) fp32 emulated on the fp16 matrix cores: both operands split into 2 fp16
 *                          planes (22-bit significand) at power-of-two scales, 3 products.  Activation scales
 *                          are fixed per tensor by a calibration encode on built-in signals, run once before
 *                          the engine's first f16x3 encode or by mimi_calibrate (never from the caller's audio:
 *                          an item's codes depend on its own samples and the padded length only).  mimi_encode reads the activations' maxima back after the encode (it
 *                          synchronises its stream in this mode); on an overflow of a fixed scale each item is
 *                          re-encoded alone, and in bf16x6 if it overflows alone.
 */
enum { MIMI_PRECISION_F32 = 0, MIMI_PRECISION_BF16X6 = 1, MIMI_PRECISION_BF16X3 = 2, MIMI_PRECISION_F16X3 = 3 };
/* default: MIMI_PRECISION_F16X3 */
int mimi_set_precision(mimi_engine* e, int32_t mode);
int mimi_get_precision(const mimi_engine* e);
/* MIMI_PRECISION_F16X3: run the activation-scale calibration now (idempotent; otherwise it runs inside the first
 * f16x3 encode).  Synchronises the device. */
int mimi_calibrate(mimi_engine* e);
/* MIMI_PRECISION_F16X3: encodes that took the overflow fallback so far (diagnostic). */
int64_t mimi_f16_reruns(const mimi_engine* e);
/* Encodes (and mimi_rvq_encode calls) re-run on the per-level RVQ kernels because a sweep of the persistent RVQ
 * chain gave up waiting for a peer workgroup (its codes are never returned; diagnostic). */
int64_t mimi_rvq_chain_reruns(const mimi_engine* e);
/* hipGraph replay of MIMI_PRECISION_F16X3 encodes (default on): the second encode of a (batch, length, K) shape
 * captures the whole pass into a graph, later ones replay it (same kernels and arguments: identical codes).
 * Never used while profiling or taps are on.  enable = 0 drops the captured graphs.  Replays so far, and graphs
 * captured so far (a graph retired by a workspace or RoPE-table reallocation is captured again: diagnostic): */
int mimi_set_graphs(mimi_engine* e, int32_t enable);
int64_t mimi_graph_replays(const mimi_engine* e);
int64_t mimi_graph_captures(const mimi_engine* e);
/* Kernel-variant options (tuning / A-B checks; every setting gives identical codes).  key "stage0_fused":
 * 0 = stage-0 residual block and down conv 0 as two kernels (y through HBM), 1 = one fused kernel (y stays on
 * chip; default).  key "ln_fused": on small grids (batch 1-4) 0 = LayerNorm launches before q/k/v and fc1, 1 = fc1
 * computes the LayerNorm of its own rows (default), 2-4 = fc1 and q/k/v do (q/k/v tile variants).  key "qkv_attn":
 * q/k/v projection + RoPE + attention as one kernel for items of <= 256 frames, 0 = off, 1 = when the batch has
 * >= 256 (item, head) pairs (default), 2 = whenever the items fit; "qkv_attn_xcd" 0/1 its workgroup placement.
 * RVQ: "rvq_form" 0-6 (level-kernel form, 0 = default), "rvq_chain" 0/1 (one persistent launch for all levels on
 * small grids, default 1; taken only where its give-up flag is read back: mimi_encode_wait re-runs an encode whose
 * chain gave up), "rvq_chain_fault" 0/1/2 (tests only: 1 = zero spin budget, 2 = every sweep gives up), "rvq_xcd"
 * 0/1.  "sc1_out" 0-7 (sc1 output stores: bit 0 q/k/v, 1 fc1 (default 2), 2 o_proj + fc2), "ln_rpw" 0/1/2/4/8
 * (LayerNorm rows per wave), "fc1_cg" 0/1/2/4 (fc1's tile order in XCD column groups, default 1 = none), "res1_form"
 * 0/1 (stage-1 block as one 8-wave or two 4-wave workgroups per CU, default 1), "res1_stream" 0/1/2 (the k = 1
 * residual conv as the streaming kernel with register-resident weights: 1 stage 2 (default), 2 stages 2 and 3 (stage 3
 * uniform batches; measured slower there), 0 off), "attn_band_split" 0/1/2 (items
 * over 256 frames: the banded attention as 128-query workgroups, by grid size (default), or one 32-query tile per
 * workgroup), "gemm256" 0-7 (uniform f16x3 batches: the 256 x 256 staggered planes-GEMM tile for bit 0 fc1, bit 1 the
 * k = 2s down convs with fp32 output, each from 256 such tiles up; bit 2 (tests) both on any grid; default 3).
 * "lanes" 0/1/2 (which encodes run on a lane's own stream, see mimi_encode_async: 0 none -- every encode on the
 * caller's stream in one workspace; 1 (default) f16x3 uniform batches whose RVQ runs the per-level kernels; 2 ragged
 * batches and encodes that may launch the persistent RVQ chain too.  mimi_encode_host, mimi_rvq_encode, decode,
 * calibration, taps and profiling level 1 never take one).
 * Unknown keys and values:
 * MIMI_ERR_INVALID_ARGUMENT.  A call waits for the encodes in flight; a change drops the captured graphs. */
int mimi_set_option(mimi_engine* e, const char* key, int64_t value);
/* Encodes submitted to lane 0 / 1 so far (diagnostic; -1: no such lane).  Encodes that take no lane count in lane 0. */
int64_t mimi_lane_encodes(const mimi_engine* e, int32_t lane);
/* MIMI_PRECISION_F16X3 diagnostics: per plane tensor (64-char names), its fixed activation scale and the max|x|
 * of the last waited encode (-1: not produced by it, or a LayerNorm output whose range check the engine skips: its
 * bound times its scale is below 2^14, so no maximum is recorded); an overflow is max * scale >= 2^15. */
int mimi_act_scales(mimi_engine* e, int32_t max_n, char* names, float* scales, float* last_max, int32_t* n);

/* Frames produced for `length` samples with the default config (reference float32 length math). */
int64_t mimi_encoded_length(int64_t length);
int64_t mimi_encoded_length_cfg(const mimi_config* cfg, int64_t length);

/*
 * Host-ingest resampler (replaces the resampling inside librosa.load(path, sr=24000):
 * librispeech-mimi/utils.py:84-87, emilia-mimi/process_shard.py:479-482, yodas2-mimi/process_shard.py:389),
 * bit-exact with librosa's res_type='polyphase' = scipy.signal.resample_poly on float32 input, and the engine of
 * the soxr_hq-spec mode (mimi_hip.ingest: a linear-phase Kaiser FIR designed to libsoxr's published HQ quality
 * spec, same polyphase arithmetic; parity with libsoxr itself unpinned).  nclips clips
 * packed in dev_in at dev_in_off[i] (dev_in_len[i] samples) -> dev_out at dev_out_off[i] (dev_out_len[i]
 * samples, max_out = their maximum), all int64 arrays on the device.  dev_filter: the up-scaled Kaiser(5.0)
 * low-pass with its zero pre-padding, or any other FIR (filter_len taps, <= MIMI_RESAMPLE_MAX_TAPS); pre_remove: leading
 * outputs of the full upfirdn skipped (resample_poly's n_pre_remove).  No engine handle needed.
 */
#define MIMI_RESAMPLE_MAX_TAPS 65536
int mimi_resample_poly(const float* dev_in, const int64_t* dev_in_off, const int64_t* dev_in_len, int32_t nclips,
                       float* dev_out, const int64_t* dev_out_off, const int64_t* dev_out_len, int64_t max_out,
                       const float* dev_filter, int32_t filter_len, int32_t up, int32_t down, int64_t pre_remove,
                       void* stream);

/*
 * FLAC decode for host ingest (replaces libFLAC behind librosa.load -> soundfile -> libsndfile on the LibriSpeech
 * path: librispeech-mimi/process_librispeech_dev-test.py:136, utils.py:84-87).  `data` holds a whole .flac file
 * (an ID3v2 tag in front is skipped).  mimi_flac_info reads STREAMINFO.  mimi_flac_decode decodes every frame
 * into `out`, planar int32 [channels][cap_per_channel] at the stream's bit depth (out = NULL: count only), and
 * sets *n_samples (per channel); CRC-8 / CRC-16 mismatches, malformed frames and a sample count that differs
 * from STREAMINFO's return MIMI_ERR_IO.  Host-only, re-entrant (no engine handle).
 */
int mimi_flac_info(const uint8_t* data, int64_t nbytes, int32_t* sample_rate, int32_t* channels,
                   int32_t* bits_per_sample, int64_t* total_samples);
int mimi_flac_decode(const uint8_t* data, int64_t nbytes, int32_t* out, int64_t cap_per_channel, int64_t* n_samples);

/*
 * Codec-BPE training over code strings (replaces the BpeTrainer run of codec-bpe/bpe_trainer.py:147-156; driven
 * by mimi_hip/bpe.py).  The corpus: words of symbol ids (0 .. n_initial_tokens-1 = special tokens, then the
 * alphabet), concatenated in `symbols`, word w = symbols[word_offsets[w] .. word_offsets[w+1]), occurring
 * word_counts[w] times; all host memory, copied.  max_token_length <= 0: unlimited; else a pair formed by a
 * merge is counted only when its merged length is below it.  Then, per step: mimi_bpe_best gives the pair of
 * highest count (ties: smallest (left, right); count 0 when none is left), the caller decides the new token's
 * id (a new one, or the id of an existing token with the same spelling) and length, and mimi_bpe_merge applies
 * it to every word.  Ids up to 131071.
 *
 * mimi_bpe_create_opts: the same with options (NULL or all zero: mimi_bpe_create exactly).  min_table_slots: the
 * floor of the pair table's size and the room it gets beyond 4x the initial pairs (default 2^20); a power of two,
 * at least 8 * vocab_size: one merge forms at most 2 * vocab_size distinct new pairs, mimi_bpe_best doubles the
 * table once more than half its slots hold a key, so the load stays <= 1/2 + 2/8 = 3/4 and an update never meets a
 * full table (it would be dropped).  grid_blocks: workgroups of every launch (default: 8 per compute unit); >= 1.
 * Anything else returns MIMI_ERR_INVALID_ARGUMENT before any device call.  Both exist so that tests reach the
 * table's growth and the kernels' grid-stride loops on small corpora.
 *
 * mimi_bpe_info: *value = the figure named by `what` (MIMI_BPE_TRAIN_INFO_*).
 *
 * Read-back for tests; both synchronise the handle's stream and change nothing.  mimi_bpe_read_pairs: every pair
 * with a positive count, unordered, into left / right / count (capacity `cap` entries each); *n_pairs receives
 * their number; all three arrays NULL: the number alone; cap too small: MIMI_ERR_INVALID_ARGUMENT.
 * mimi_bpe_read_words: the current symbols of every word, concatenated in word order into symbols (capacity cap),
 * word w's current length into word_lengths[w] (n_words = the corpus's), *n_symbols = the live symbols; both arrays
 * NULL: the number alone.  The host walks the forward links from each word's first position and returns
 * MIMI_ERR_STATE when a back link disagrees (prv[nxt[p]] != p), a dead symbol is linked, a link leaves its word or
 * cycles, or a live symbol is unreachable.
 */
typedef struct mimi_bpe mimi_bpe;
typedef struct mimi_bpe_options {
    int64_t min_table_slots; /* 0: 2^20 */
    int32_t grid_blocks;     /* 0: 8 per compute unit */
    int32_t reserved;        /* 0 */
} mimi_bpe_options;
#define MIMI_BPE_TRAIN_INFO_TABLE_SLOTS 0     /* capacity of the pair table */
#define MIMI_BPE_TRAIN_INFO_NKEYS 1           /* keys inserted since the table was last rebuilt (dead ones included) */
#define MIMI_BPE_TRAIN_INFO_GROWTH_REHASHES 2 /* doublings by mimi_bpe_best so far */
#define MIMI_BPE_TRAIN_INFO_GRID_BLOCKS 3     /* workgroups per launch */
#define MIMI_BPE_TRAIN_INFO_SYMBOLS 4         /* symbols of the corpus (positions, live or dead) */
int mimi_bpe_create(int device, const int32_t* symbols, int64_t n_symbols, const int64_t* word_offsets,
                    const int64_t* word_counts, int64_t n_words, int32_t n_initial_tokens, int32_t vocab_size,
                    int32_t max_token_length, mimi_bpe** out);
int mimi_bpe_create_opts(int device, const int32_t* symbols, int64_t n_symbols, const int64_t* word_offsets,
                         const int64_t* word_counts, int64_t n_words, int32_t n_initial_tokens, int32_t vocab_size,
                         int32_t max_token_length, const mimi_bpe_options* opts, mimi_bpe** out);
int mimi_bpe_info(mimi_bpe* h, int32_t what, int64_t* value);
int mimi_bpe_read_pairs(mimi_bpe* h, int32_t* left, int32_t* right, int64_t* count, int64_t cap, int64_t* n_pairs);
int mimi_bpe_read_words(mimi_bpe* h, int32_t* symbols, int64_t cap, int64_t* word_lengths, int64_t n_words,
                        int64_t* n_symbols);
int mimi_bpe_best(mimi_bpe* h, int32_t* left, int32_t* right, int64_t* count);
int mimi_bpe_merge(mimi_bpe* h, int32_t left, int32_t right, int32_t new_id, int32_t new_len);
void mimi_bpe_destroy(mimi_bpe* h);

/*
 * Codec-BPE encoding: words of symbol ids -> token ids (replaces the tokenizer call of
 * pretraining-data/estimate_tokens.py:75, tokenizer(text)["input_ids"]; driven by mimi_hip/bpe.py Encoder).  The
 * rule is HF tokenizers' BPE model for one word (no dropout, ignore_merges off): among the adjacent pairs that
 * have a merge take the lowest rank, on equal rank the leftmost, merge that one occurrence, repeat.
 *
 * mimi_bpe_model_create: merges[n_merges][3] = (left id, right id, new id) in rank order, ids in the trainer's
 * convention (special tokens, then the alphabet, then the learned tokens; a new id may be the id of an existing
 * token with the same spelling), all in [0, n_tokens), n_tokens <= 131072; host memory, copied into a device hash
 * table.  A pair that occurs twice keeps its last rank, as tokenizers' merge map does.
 *
 * mimi_bpe_encode: word w = symbols[word_offsets[w] .. word_offsets[w+1]) (host arrays, word_offsets[0] = 0);
 * its ids are written to out_ids + word_offsets[w] (out_ids has the capacity of symbols) and their number to
 * out_lens[w]; a word of length 0 gives nothing, a word of length 1 itself.  Runs on `stream` (a hipStream_t, NULL =
 * the default stream) and synchronises it before returning.  A symbol id outside [0, n_tokens) returns
 * MIMI_ERR_INVALID_ARGUMENT (checked on the device before any table access; the outputs are then undefined); a
 * failed allocation returns MIMI_ERR_OUT_OF_MEMORY and leaves the model usable.  One encode at a time per model
 * (calls on one model are serialised).  Words up to MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS symbols run with their state in
 * LDS, longer words on a device workspace sized from the longest word of the call.
 *
 * mimi_bpe_model_info: *value = the model property or last-encode figure named by `what` (MIMI_BPE_INFO_*).
 */
#define MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS 8192
#define MIMI_BPE_INFO_PAIRS 0                 /* distinct pairs in the merge table */
#define MIMI_BPE_INFO_FORMED_PAIR_OUTRANKS 1  /* 1: some merge forms a pair of lower rank than its own */
#define MIMI_BPE_INFO_TABLE_SLOTS 2           /* capacity of the merge table */
#define MIMI_BPE_INFO_LAST_WORDS_LDS_SMALL 3  /* last encode: words run by the 3072-symbol LDS form */
#define MIMI_BPE_INFO_LAST_WORDS_LDS 4        /* last encode: words run by the MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS form */
#define MIMI_BPE_INFO_LAST_WORDS_GLOBAL 5     /* last encode: words run on the global workspace */
typedef struct mimi_bpe_model mimi_bpe_model;
int mimi_bpe_model_create(int device, const int32_t* merges, int64_t n_merges, int32_t n_tokens,
                          mimi_bpe_model** out);
void mimi_bpe_model_destroy(mimi_bpe_model* m);
int mimi_bpe_encode(mimi_bpe_model* m, const int32_t* symbols, const int64_t* word_offsets, int64_t n_words,
                    int32_t* out_ids, int32_t* out_lens, void* stream);
int mimi_bpe_model_info(const mimi_bpe_model* m, int32_t what, int64_t* value);

/*
 * Codec-BPE encoding of codes that are already in device memory: the word model (what tokenizers' NFKC normalizer and
 * Metaspace pre-tokenizer do to a string of code characters; mimi_hip/bpe.py CharModel.words) runs on the device, then
 * the merge kernels of mimi_bpe_encode, then the ids are packed per sequence -- device memory in, device memory out.
 *
 * mimi_bpe_model_set_alphabet: the code alphabet of the model: num_codebooks x codebook_size characters, character
 * k * codebook_size + code has symbol id n_special + its index, class cls[index] (0 keep starter, 1 keep mark, 2 drop
 * starter, 3 drop mark, 4 split) and combining class ccc[index]; cls and ccc are host arrays, copied into one device
 * table of 2 bytes per character.  A class above 4 or n_special + num_codebooks * codebook_size > n_tokens returns
 * MIMI_ERR_INVALID_ARGUMENT.  Call it once before mimi_bpe_encode_codes (else MIMI_ERR_STATE).
 *
 * mimi_bpe_encode_codes: dev_codes is device int32, codebook k of item b at dev_codes + b * item_stride +
 * k * row_stride, frame_lengths[b] frames of it (host array; frames beyond are never read), k < num_codebooks (an
 * item may have more rows: an engine's [B][K'][Tmax] output is used as it stands).  Item b gives
 * max(1, ceil(T_b / chunk_frames)) sequences of chunk_frames frames (the last one shorter), chunk_frames = 0: the
 * whole item; an empty item gives one empty sequence; sequences count in item order, then chunk order, and n_seq
 * must equal their number.  Each sequence is a string of its own: position (frame t, codebook k) is character t *
 * num_codebooks + k.  Inside each run of marks (classes 1 and 3 between starter-class characters or the ends of the
 * sequence) the kept marks are stably sorted by ccc; then dropped characters vanish, split characters vanish and
 * cut the word, and the words are encoded as by mimi_bpe_encode.  On return dev_out_ids (device int32, out_capacity
 * >= num_codebooks * sum of frame_lengths, which bounds the token count) holds the ids of sequence s, packed, at
 * [seq_offsets[s], seq_offsets[s + 1]) (seq_offsets: host, n_seq + 1 entries).  Runs on `stream` and synchronises it
 * twice: once mid-way to read back 32 bytes (flags, the word count of each kernel form, the longest word), once at
 * the end.  A code outside [0, codebook_size) returns MIMI_ERR_INVALID_ARGUMENT (checked on the device before the
 * table load); a run of more than MIMI_BPE_WORDS_MAX_RUN marks returns MIMI_ERR_UNSUPPORTED (the caller may run the
 * host word model instead); in both cases the outputs are undefined and the model stays usable.  Serialised with
 * mimi_bpe_encode by the model's mutex; MIMI_BPE_INFO_LAST_WORDS_* report this call as they do that one.  The device
 * buffers grow with the call and are kept: 40 bytes per character.
 */
#define MIMI_BPE_WORDS_MAX_RUN 64     /* longest run of marks the device word model orders */
#define MIMI_BPE_WORDS_SCAN_TILE 2048 /* characters per workgroup of the classify / scan kernels */
int mimi_bpe_model_set_alphabet(mimi_bpe_model* m, int32_t n_special, int32_t num_codebooks, int32_t codebook_size,
                                const uint8_t* cls, const uint8_t* ccc);
int mimi_bpe_encode_codes(mimi_bpe_model* m, const int32_t* dev_codes, int32_t batch, int64_t item_stride,
                          int64_t row_stride, const int64_t* frame_lengths, int64_t chunk_frames,
                          int32_t* dev_out_ids, int64_t out_capacity, int64_t* seq_offsets, int64_t n_seq,
                          void* stream);

/*
 * Codec-BPE decoding of token ids that are already in device memory, the inverse of mimi_bpe_encode_codes: ids ->
 * the code characters they spell -> the drop rules of the reference's pretraining-data/converter.py chars_to_codes
 * (default flags) -> codes laid out as mimi_decode_ragged takes them; device memory in, device memory out
 * (mimi_hip/bpe.py Encoder.decode_device drives it, Encoder.decode_ids is the host statement of the same rules).
 *
 * mimi_bpe_model_set_spellings: token id i spells the alphabet indices spell_index[spell_offsets[i] ..
 * spell_offsets[i + 1]) (host arrays, n_tokens + 1 offsets starting at 0; an id that gives no character -- a special
 * token -- has an empty spelling).  Requires mimi_bpe_model_set_alphabet (else MIMI_ERR_STATE; a later set_alphabet
 * drops the spellings); an index outside [0, num_codebooks * codebook_size) or decreasing offsets return
 * MIMI_ERR_INVALID_ARGUMENT.  Copied into device memory.
 *
 * mimi_bpe_decode_plan: sequence s is dev_ids[seq_offsets[s] .. seq_offsets[s + 1]) (dev_ids: device int32;
 * seq_offsets: host, n_seq + 1 entries from 0, non-decreasing).  Per sequence the spellings are concatenated (character
 * i has codebook cb_i = index_i / codebook_size), then with expected = cb_0 a character is kept iff cb_i == expected,
 * a kept one advancing expected to (expected + 1) % num_codebooks; of the kept characters the first
 * min((num_codebooks - cb_0) % num_codebooks, kept) and then the last remaining % num_codebooks are dropped; the rest
 * are frame_lengths[s] = remaining / num_codebooks frames (host out, n_seq entries; 0 for a sequence that spells
 * nothing).  The plan (every character's alphabet index, keep bit and kept rank, every sequence's first rank and frame
 * count) stays in the model's buffers, 8 bytes per character and 4 per id.  Runs on `stream` and synchronises it
 * twice: once to read back the character count that sizes those buffers (with the bad-id flag), once for the frame
 * counts.  An id outside [0, n_tokens) returns MIMI_ERR_INVALID_ARGUMENT (checked on the device before any table
 * load) and the model stays usable; num_codebooks > 16 (a filter state map is 16 nibbles) or 2^31 characters or more
 * return MIMI_ERR_UNSUPPORTED (the caller may run the host rules instead); without spellings: MIMI_ERR_STATE.
 *
 * mimi_bpe_decode_write: writes the last plan's codes: frame t of codebook k of sequence s to dev_codes +
 * s * item_stride + k * row_stride + t (device int32), t < frame_lengths[s]; nothing else is written (rows past a
 * sequence's frames keep what they held; mimi_decode_ragged never reads them).  Without a plan -- none made, the last
 * one failed, or any other call on the model since -- it returns MIMI_ERR_STATE; max_frames (the frames a row of
 * dev_codes holds) below the plan's largest frame count returns MIMI_ERR_INVALID_ARGUMENT with nothing launched.  A
 * plan may be written more than once.  Runs on `stream` and synchronises it.  Both calls are serialised with the
 * encode calls by the model's mutex.
 */
#define MIMI_BPE_DECODE_SCAN_TILE 2048 /* ids / characters per workgroup of the decode scan kernels */
int mimi_bpe_model_set_spellings(mimi_bpe_model* m, const int64_t* spell_offsets, const int32_t* spell_index);
int mimi_bpe_decode_plan(mimi_bpe_model* m, const int32_t* dev_ids, const int64_t* seq_offsets, int64_t n_seq,
                         int64_t* frame_lengths, void* stream);
int mimi_bpe_decode_write(mimi_bpe_model* m, int32_t* dev_codes, int64_t item_stride, int64_t row_stride,
                          int64_t max_frames, void* stream);

/*
 * Codec-BPE decoding chunk by chunk: a pool of `slots` sessions, each with its own filter state in device memory;
 * a step takes a few new token ids for any subset of the slots and writes the whole frames those ids complete, laid
 * out as mimi_decode_stream_step_ragged takes them (mimi_hip/bpe.py IdStream drives it).  The rules above are causal,
 * so this is exact: per slot, with K = num_codebooks, and for each character (alphabet index idx, cb = idx /
 * codebook_size) that the slot's new ids spell, in order:
 *     fresh (no character since the reset): expected = cb, owed = (K - cb) % K
 *     cb != expected: dropped;  else expected = (expected + 1) % K and, if owed > 0, --owed and dropped;
 *     else the code idx - npend * codebook_size joins the npend pending ones; K pending codes are emitted as a frame.
 * After any sequence of steps the frames a slot has emitted are mimi_bpe_decode_plan / _write's (and
 * Encoder.decode_ids') of all the ids it was fed since its reset, whatever the split into steps and whatever the
 * other slots were fed.  A reset is also how a session ends: the pending partial frame is discarded, which is the
 * batch form's end drop.
 *
 * mimi_bpe_decode_stream_create: needs mimi_bpe_model_set_spellings (else MIMI_ERR_STATE) and records Lmax, the
 * longest spelling; num_codebooks > 16 returns MIMI_ERR_UNSUPPORTED (a filter state map is 16 nibbles), as does
 * max_step_ids * Lmax of 2^31 or more.  slots >= 1; 1 <= max_step_ids <= 2^20.  Device memory: 3 + K int32 per slot,
 * plus 32 bytes per slot of step bookkeeping.
 * mimi_bpe_decode_stream_max_frames: host only; (K - 1 + ids * Lmax) / K, the most frames an item that brings `ids`
 * ids can complete (-1 for a NULL stream or negative ids).
 * mimi_bpe_decode_stream_step: item i is slot slots[i] (host, m distinct slots in any order, 1 <= m <= slots) and
 * brings counts[i] ids (host, 0 <= counts[i] <= max_step_ids) from dev_ids + i * ids_row_stride (device int32; ids
 * past an item's count are never read).  Writes frames_out[i] (host) whole frames to dev_codes[i][k][t], t <
 * frames_out[i] (device int32 [m][K][max_frames]); columns past an item's frames are never written.  max_frames must
 * be at least max_frames(the largest count).  One kernel launch on `stream`, which the call synchronises to read the
 * frame counts back through a pinned buffer the stream owns.  Argument errors (a slot list that is not distinct or in
 * range, a count out of range, max_frames too small, NULL pointers) return MIMI_ERR_INVALID_ARGUMENT with every slot
 * untouched.  An id outside [0, n_tokens) (checked on the device before any table load) returns
 * MIMI_ERR_INVALID_ARGUMENT; the outputs are undefined and the slots listed in that call then refuse with
 * MIMI_ERR_STATE until they are reset -- the rule mimi_decode_stream_step has for a bad code.  Spellings replaced on
 * the model after the stream was made: MIMI_ERR_STATE.
 * mimi_bpe_decode_stream_reset / _reset_slot: all slots / one slot back to fresh (host only: the next step of the
 * slot ignores its device record).
 * mimi_bpe_decode_stream_slot_pending: host only; the codes pending in the slot's partial frame, 0 .. K - 1, or -1 for
 * a fresh slot (-2 for a NULL stream or a slot out of range).
 *
 * Lifetime and locking: the stream has its own mutex (one step at a time) and holds the model's while it launches
 * and until the step has finished, because mimi_bpe_model_set_spellings frees the tables the kernel reads; so a step
 * is serialised with the model's encode and decode calls.  A stream must be destroyed before its model.
 */
typedef struct mimi_bpe_decode_stream mimi_bpe_decode_stream;
int mimi_bpe_decode_stream_create(mimi_bpe_model* m, int32_t slots, int32_t max_step_ids,
                                  mimi_bpe_decode_stream** out);
int64_t mimi_bpe_decode_stream_max_frames(const mimi_bpe_decode_stream* st, int32_t ids);
int mimi_bpe_decode_stream_step(mimi_bpe_decode_stream* st, const int32_t* slots, const int32_t* counts, int32_t m,
                                const int32_t* dev_ids, int64_t ids_row_stride, int32_t* dev_codes,
                                int32_t max_frames, int32_t* frames_out, void* stream);
int mimi_bpe_decode_stream_reset(mimi_bpe_decode_stream* st);
int mimi_bpe_decode_stream_reset_slot(mimi_bpe_decode_stream* st, int32_t slot);
int32_t mimi_bpe_decode_stream_slot_pending(mimi_bpe_decode_stream* st, int32_t slot);
void mimi_bpe_decode_stream_destroy(mimi_bpe_decode_stream* st);

/*
 * Diagnostic: the fp16 plane split the kernels use (two v_fma_mix per value: hi = fp16(v s), lo = fp16(v s - hi))
 * against the conversion form it replaces, on npairs value pairs of dev_in (device f32 [2 npairs], s a power of two):
 * dev_out (device u32 [npairs][4]) = the kernels' (hi, lo) words and the conversion form's (hi, lo) words.  Tests
 * require them equal on edge values (zeros of both signs, fp32 / fp16 subnormals, rounding ties, fp16 overflow).
 */
int mimi_split_check(const float* dev_in, int64_t npairs, float scale, uint32_t* dev_out, void* stream);

/*
 * Diagnostic: fc1's f16x3 GELU epilogue (the branch-free erfc form, gemm_kernel.h gelu_fast) on n values:
 * dev_out[i] = GELU(dev_in[i]) (device f32 [n] each).  Replaces torch's GELU(approximate='none') at
 * TF/modeling_mimi.py:602-615 (MimiMLP fc1 -> activation); tests bound it against float64 and torch.
 */
int mimi_gelu_check(const float* dev_in, int64_t n, float* dev_out, void* stream);

/* Device bytes the workspace needs for (batch, length); the engine grows it on demand. */
int64_t mimi_workspace_bytes(const mimi_engine* e, int32_t batch, int64_t length);

/* Release everything. */
void mimi_destroy(mimi_engine* e);

/* Thread-local description of the last failure in this thread. */
const char* mimi_last_error(void);

/* ---- instrumentation (bench / tests) ---- */

/* enable = 1: every encode records HIP events between its stages on the stream it runs on (one per stage);
 * 2: only around its first stage (two events per encode: the light form a timed region can carry); 0: off. */
int mimi_set_profiling(mimi_engine* e, int enable);
/* Per-stage totals accumulated over all profiled encodes since the last reset: names (128 chars
 * each, "stage|kernel symbol"), device ms (event pairs on the launch stream), launch counts, and algorithmic work as
 * (flops, bytes) pairs in flops_bytes[2*i], flops_bytes[2*i+1].  Synchronises the recorded events. */
int mimi_profile_read(mimi_engine* e, int32_t max_stages, char* names /* max_stages*128 */,
                      double* total_ms, int64_t* launches, double* flops_bytes, int32_t* n_stages);
int mimi_profile_reset(mimi_engine* e);
/* The "stage|kernel symbol" names of the last profiled encode, in launch order (one entry per stage event; a
 * stage's first dispatch is its named kernel).  Lets a rocprofv3 counter pass key its dispatches by stage. */
int mimi_profile_sequence(mimi_engine* e, int32_t max_stages, char* names /* max_stages*128 */, int32_t* n_stages);

/* When enabled, mimi_encode keeps a copy of each stage's output (for per-stage parity tests); mimi_decode keeps
 * "quantized" (after the two output_proj, summed), "upsample", "xfmr7", "dconv0" (raw decoder.layers.0 output, from a
 * launch of its own that only taps make), "dconv0_elu" (the bias + ELU output the pass itself computes), "up0".."up3"
 * (each transposed conv's raw output), "dres0_elu".."dres3_elu" (ELU of each residual block's output: the form the
 * fused block stores) and "audio", all [batch][time][channels].  mimi_set_profiling records decode's stages too
 * (names "dec_..."). */
int mimi_set_taps(mimi_engine* e, int enable);
/* Copy tap `name` to host: dst holds cap floats; *numel receives the element count; dims[0..2] the
 * [batch][time][channels] shape.  Synchronises. */
int mimi_get_tap(mimi_engine* e, const char* name, float* host_dst, int64_t cap, int64_t* numel,
                 int64_t dims[3]);

#ifdef __cplusplus
}
#endif
#endif /* MIMI_HIP_H */
