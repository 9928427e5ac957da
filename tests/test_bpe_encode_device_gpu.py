"""Device-to-device codec-BPE encoding on the GPU (``bpe_words.hip`` through ``mimi_bpe_encode_codes`` /
``bpe.Encoder.encode_device``): codes in device memory -> token ids in device memory.  Every comparison is exact
equality of id arrays; the expected ids are the committed ``tokenizers`` fixtures, live ``tokenizers``
(``bpe_encode_ref.hf_tokenizer``) or the host path ``encode_codes`` (pinned to ``tokenizers`` by
tests/test_bpe_encode_gpu.py and, for the mark-run alphabet, tests/test_bpe_encode_device.py) -- never the new code."""
import numpy as np
import pytest
import torch

import bpe_encode_cases as cases
import bpe_encode_ref as ref
from mimi_hip import _lib, bpe, synthetic
from test_bpe_encode_device import MARK_N, MARK_OFFSET, MARK_STARTERS, mark_run_string

pytestmark = pytest.mark.gpu

OFFSET, CBS = cases.OFFSET, 2048
LDS_MAX = _lib.BPE_ENCODE_LDS_MAX_SYMBOLS
CAP = _lib.BPE_WORDS_MAX_RUN
TILE = _lib.BPE_WORDS_SCAN_TILE  # positions per workgroup of the classify / scan kernels
ROW = 256                        # positions per workgroup-wide scan step inside a tile (the workgroup's threads)
PARTIALS_PASS = 256              # tile sums the scan-of-partials workgroup takes per pass
INT32_MAX = 2 ** 31 - 1


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def dev(codes, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(codes)).to("cuda:0", dtype)


def assert_seqs(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and np.array_equal(g, w), (tag, i, g.tolist()[:40], np.asarray(w).tolist()[:40])


def chunks_of(codes, cf):
    """``[K, T]`` -> the chunks ``encode_device(chunk_frames=cf)`` cuts (one empty chunk for T = 0)."""
    T = codes.shape[1]
    step = cf or max(T, 1)
    return [codes[:, f:f + step] for f in range(0, max(T, 1), step)]


def forms(enc):
    return enc.info("last_words_lds_small"), enc.info("last_words_lds"), enc.info("last_words_global")


_encoders = {}


def trained_encoder(case):
    if case not in _encoders:
        meta, arrays = cases.fixture()
        c = meta["trained"][case]
        _encoders[case] = bpe.Encoder(c["num_codebooks"], CBS, arrays[f"{case}_merges"], c["n_tokens"], 1,
                                      unicode_offset=OFFSET)
    return _encoders[case]


def trained_codes(case):
    """The 3000-character fixture string of a trained model as ``[K, 3000 / K]`` codes, and its tokenizers ids."""
    meta, arrays = cases.fixture()
    K = meta["trained"][case]["num_codebooks"]
    codes = arrays[f"{case}_cps3"].astype(np.int64).reshape(-1, K).T - OFFSET - CBS * np.arange(K)[:, None]
    assert codes.min() >= 0 and codes.max() < CBS
    return np.ascontiguousarray(codes), arrays[f"{case}_ids3"]


# ---- every character class ----------------------------------------------------------------------------------------
def test_every_character_class():
    need_gpu()
    _, arrays = cases.fixture()
    enc = trained_encoder("k8_recipe")
    codes = arrays["chars_codes"].astype(np.int64)
    cls = enc._chars.cls[(codes + CBS * np.arange(8)[:, None]).T.reshape(-1)]
    assert set(cls.tolist()) == {0, 1, 2, 3, 4}
    assert_seqs(enc.encode_device(dev(codes), to_host=True), [arrays["chars_ids"]], "chars")
    assert enc.last_stats["word_model"] == "device" and enc.last_stats["words"] > 1
    for cf in (1, 7, 120, 121):
        want = enc.encode_codes(chunks_of(codes, cf))
        assert_seqs(enc.encode_device(dev(codes), chunk_frames=cf, to_host=True), want, f"chars cf={cf}")
        assert enc.last_stats["word_model"] == "device"


# ---- trained models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k8_recipe", "k8_unlimited", "k2_ngram2", "k2_unlimited"])
def test_trained_models(case):
    need_gpu()
    enc = trained_encoder(case)
    codes, want = trained_codes(case)
    ids, offs, item = enc.encode_device(dev(codes))
    assert ids.dtype == torch.int32 and ids.is_cuda and offs.dtype == np.int64 and offs.tolist() == [0, len(want)]
    assert item.tolist() == [0]
    assert np.array_equal(ids.cpu().numpy(), want)
    for frames in (1, 12, 13):
        assert_seqs(enc.encode_device(dev(codes[:, :frames]), to_host=True), enc.encode_codes([codes[:, :frames]]),
                    f"{case} prefix {frames}")


# ---- batch and padding ----------------------------------------------------------------------------------------------
def test_batch_padding_rows_dtypes_and_empty_items():
    need_gpu()
    enc = trained_encoder("k8_recipe")
    utt, ids3 = trained_codes("k8_recipe")
    assert utt.shape == (8, 375)
    items = [utt, utt[:, 100:101], utt[:, 200:300]]
    lengths = [375, 1, 100]
    own = [enc.encode_device(dev(c)[None], to_host=True)[0] for c in items]
    assert np.array_equal(own[0], ids3)
    assert_seqs(own, enc.encode_codes(items), "own")
    for pad in (-1, 2048, INT32_MAX):
        for rows, dtype in ((8, torch.int32), (8, torch.int64), (9, torch.int32)):
            batch = np.full((3, rows, 375), pad, np.int64)
            if rows == 9:
                batch[:, 8] = 2048  # a row beyond num_codebooks: ignored
            for b, c in enumerate(items):
                batch[b, :8, :c.shape[1]] = c
            got = enc.encode_device(dev(batch, dtype), lengths, to_host=True)
            assert_seqs(got, own, f"pad {pad} rows {rows} {dtype}")
            assert enc.last_stats["word_model"] == "device"
    # a view whose item and row strides are not those of a packed tensor
    wide = dev(batch, torch.int32)
    assert_seqs(enc.encode_device(wide[:, :, :120], [120, 1, 100], to_host=True),
                [enc.encode_codes([utt[:, :120]])[0], own[1], own[2]], "strided view")
    empty = np.zeros(0, np.int32)
    ids, offs, item = enc.encode_device(dev(batch, torch.int32), [375, 0, 100])
    assert item.tolist() == [0, 1, 2] and offs.tolist() == [0, len(own[0]), len(own[0]), len(own[0]) + len(own[2])]
    assert np.array_equal(ids.cpu().numpy(), np.concatenate([own[0], own[2]]))
    assert_seqs(enc.encode_device(dev(batch, torch.int32), [0, 0, 0], chunk_frames=7, to_host=True), [empty] * 3,
                "all empty")
    assert forms(enc) == (3, 0, 0)
    ids, offs, item = enc.encode_device(dev(np.zeros((0, 8, 5), np.int64)))
    assert ids.numel() == 0 and ids.is_cuda and offs.tolist() == [0] and item.size == 0
    assert enc.encode_device(dev(np.zeros((0, 8, 5), np.int64)), to_host=True) == []
    # chunking a batch: sequences in item order, then chunk order
    ids, offs, item = enc.encode_device(dev(batch, torch.int32), lengths, chunk_frames=150)
    assert item.tolist() == [0, 0, 0, 1, 2]
    want = enc.encode_codes(chunks_of(items[0], 150) + [items[1], items[2]])
    flat = ids.cpu().numpy()
    assert_seqs([flat[offs[i]:offs[i + 1]] for i in range(5)], want, "batch chunks")


# ---- mark runs ------------------------------------------------------------------------------------------------------
# symbol ids of the mark alphabet: starters 1 .. 27, marks 28 .. 91; six marks of distinct combining classes and a
# second one of class 230 for the hand merges
def _mark_models():
    enc0 = bpe.Encoder(1, MARK_N, [], 1 + MARK_N, 1, unicode_offset=MARK_OFFSET)
    ccc = enc0._chars.ccc
    by = {}
    for i in range(MARK_STARTERS, MARK_N):
        by.setdefault(int(ccc[i]), []).append(1 + i)
    m1, m202, m216, m220, m230, m232 = (by[c][0] for c in (1, 202, 216, 220, 230, 232))
    m230b = by[230][1]
    nxt = 1 + MARK_N
    tri = [(m230, m230b, nxt), (m1, m202, nxt + 1), (m220, m230, nxt + 2), (1, m1, nxt + 3), (nxt + 3, m202, nxt + 4),
           (m230b, m230, nxt + 5), (m216, m220, nxt + 6), (nxt + 6, m230, nxt + 7), (m232, 2, nxt + 8),
           (m230, m230, nxt + 9)]
    pool = np.array([m1, m202, m216, m220, m230, m230b, m232], np.int64) - 1
    enc1 = bpe.Encoder(1, MARK_N, tri, nxt + len(tri), 1, unicode_offset=MARK_OFFSET)
    toks = []
    for e, t in ((enc0, []), (enc1, tri)):
        spell = ref.spellings(t, cases.SPECIALS, MARK_N, MARK_OFFSET, e.n_tokens)
        toks.append(ref.hf_tokenizer(spell, t, cases.SPECIALS))
    return (enc0, toks[0]), (enc1, toks[1]), pool


_marks = None


def mark_models():
    global _marks
    if _marks is None:
        _marks = _mark_models()
    return _marks


def pooled(rng, idx, pool):
    """The marks of a sequence redrawn from `pool` (alphabet indices), so that the hand merges meet them; starters
    from the first three."""
    out = idx.copy()
    marks = out >= MARK_STARTERS
    out[marks] = rng.choice(pool, size=int(marks.sum()))
    out[~marks] = rng.integers(0, 3, size=int((~marks).sum()))
    return out


def encode_mark_seqs(enc, seqs, **kw):
    """Alphabet-index sequences as one padded ``[B, 1, Tmax]`` batch through ``encode_device``."""
    T = max(len(s) for s in seqs)
    batch = np.full((len(seqs), 1, T), -7, np.int64)
    for b, s in enumerate(seqs):
        batch[b, 0, :len(s)] = s
    return enc.encode_device(dev(batch), [len(s) for s in seqs], to_host=True, **kw)


def check_mark_seqs(enc, tok, seqs, tag, model="device"):
    hf = [np.array(ref.hf_ids(tok, "".join(chr(MARK_OFFSET + int(i)) for i in s)), np.int32) for s in seqs]
    host = enc.encode_codes([s[None] for s in seqs])
    assert_seqs(host, hf, tag + " host vs tokenizers")
    got = encode_mark_seqs(enc, seqs)
    assert enc.last_stats["word_model"] == model, tag
    assert_seqs(got, hf, tag)


@pytest.mark.parametrize("R", [1, 2, 5, CAP - 1, CAP])
def test_mark_runs_are_ordered_on_the_device(R):
    need_gpu()
    (enc0, tok0), (enc1, tok1), pool = mark_models()
    rng = np.random.default_rng(100 + R)
    seqs = [mark_run_string(rng, 4, R) for _ in range(3)]
    check_mark_seqs(enc0, tok0, seqs, f"R={R}")
    check_mark_seqs(enc1, tok1, [pooled(rng, s, pool) for s in seqs], f"R={R} merges")


def test_a_run_above_the_cap_goes_through_the_host_model_and_the_encoder_stays_usable():
    need_gpu()
    (enc0, tok0), (enc1, tok1), pool = mark_models()
    rng = np.random.default_rng(7)
    long = [mark_run_string(rng, 4, CAP + 1), mark_run_string(rng, 2, 5)]
    check_mark_seqs(enc0, tok0, long, "cap + 1", model="host")
    check_mark_seqs(enc1, tok1, [pooled(rng, s, pool) for s in long], "cap + 1 merges", model="host")
    short = [mark_run_string(rng, 4, 5)]
    check_mark_seqs(enc0, tok0, short, "after", model="device")
    check_mark_seqs(enc1, tok1, [pooled(rng, s, pool) for s in short], "after merges", model="device")


def test_mark_runs_at_sequence_ends_tile_boundaries_and_chunk_cuts():
    need_gpu()
    (enc0, tok0), (enc1, tok1), pool = mark_models()
    rng = np.random.default_rng(11)
    seqs = [mark_run_string(rng, 3, 4, lead=False),                          # starts with a run
            mark_run_string(rng, 3, 4, tail=False),                          # ends with a run
            rng.integers(MARK_STARTERS, MARK_N, size=CAP).astype(np.int64),  # is a single run
            rng.integers(MARK_STARTERS, MARK_N, size=1).astype(np.int64)]
    check_mark_seqs(enc0, tok0, seqs, "ends")
    check_mark_seqs(enc1, tok1, [pooled(rng, s, pool) for s in seqs], "ends merges")
    # one sequence with a run of 6 marks across every boundary of the classify / scan kernels in its first tiles:
    # each ROW positions (one workgroup-wide scan step) and each TILE positions (one workgroup), the run starting
    # 1 .. 5 positions before the boundary; a short sequence in front shifts nothing (item 0 starts at position 0)
    n = 2 * TILE + 40
    idx = rng.integers(0, MARK_STARTERS, size=n).astype(np.int64)
    for j, edge in enumerate(list(range(ROW, 2 * TILE + 1, ROW))):
        lo = edge - 1 - j % 5
        idx[lo:lo + 6] = rng.integers(MARK_STARTERS, MARK_N, size=6)
    assert idx[TILE - 1] >= MARK_STARTERS and idx[TILE] >= MARK_STARTERS
    check_mark_seqs(enc0, tok0, [idx], "tiles")
    check_mark_seqs(enc1, tok1, [pooled(rng, idx, pool)], "tiles merges")
    # the same behind a sequence of 3 positions: every boundary now falls elsewhere in the runs
    check_mark_seqs(enc0, tok0, [idx[:3], idx], "tiles shifted")
    # a run cut in two by chunk_frames: each chunk is a string of its own
    cut = rng.integers(0, MARK_STARTERS, size=60).astype(np.int64)
    cut[20:30] = rng.integers(MARK_STARTERS, MARK_N, size=10)
    for enc, seq in ((enc0, cut), (enc1, pooled(rng, cut, pool))):
        want = enc.encode_codes(chunks_of(seq[None], 25))
        got = enc.encode_device(dev(seq[None]), chunk_frames=25, to_host=True)
        assert enc.last_stats["word_model"] == "device"
        assert_seqs(got, want, "run cut by chunk_frames")
    # (the cut changes the order of the marks, so treating the run as one would show)
    words = enc0._chars.words
    assert not np.array_equal(np.concatenate([words(c + MARK_OFFSET)[0] for c in (cut[:25], cut[25:50], cut[50:])]),
                              words(cut + MARK_OFFSET)[0])


# ---- scan boundaries ------------------------------------------------------------------------------------------------
def split_encoder():
    """K = 1 over the characters of the recipe's codebook 3 (U+F800-FFFF: every class), with merges over a few kept
    characters so that a missed or misplaced word cut changes the ids."""
    probe = bpe.CharModel(OFFSET + 3 * CBS, CBS)
    pick = {c: np.nonzero(probe.cls == c)[0] for c in range(5)}
    keep = pick[0][:5] + 1
    mark = pick[1][:2] + 1
    nxt = 1 + CBS
    tri = [(keep[0], keep[1], nxt), (keep[1], keep[0], nxt + 1), (nxt, keep[2], nxt + 2), (keep[0], keep[0], nxt + 3),
           (keep[3], mark[0], nxt + 4), (nxt + 3, keep[1], nxt + 5), (keep[2], keep[2], nxt + 6),
           (mark[1], keep[4], nxt + 7), (nxt + 1, nxt + 1, nxt + 8)]
    enc = bpe.Encoder(1, CBS, tri, nxt + len(tri), 1, unicode_offset=OFFSET + 3 * CBS)
    # codes to draw from: mostly the kept characters of the merges, some of every other class
    pool = np.concatenate([np.repeat(pick[0][:5], 6), pick[1][:2], pick[2][:1], pick[3][:1], pick[4][:2]])
    return enc, pool, int(pick[4][0])


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, PARTIALS_PASS * TILE + 1])
def test_scan_boundaries(n):
    """Total positions just below, at and just above one tile, and one more than the tiles one pass of the
    scan-of-partials workgroup takes; split characters on both sides of each tile boundary."""
    need_gpu()
    enc, pool, split = split_encoder()
    rng = np.random.default_rng(n)
    codes = rng.choice(pool, size=n).astype(np.int64)
    for edge in range(TILE, n + 1, TILE):
        for p in (edge - 2, edge - 1, edge, edge + 2):
            if p < n and (edge // TILE) % 3 != 2:
                codes[p] = split
    codes[max(0, n - 2):] = split if n % 2 else codes[0]
    want = enc.encode_codes([codes[None]])
    assert enc.last_stats["words"] > n // 100
    assert_seqs(enc.encode_device(dev(codes[None]), to_host=True), want, f"n={n}")
    assert enc.last_stats["word_model"] == "device" and enc.last_stats["words"] == len(enc._chars.words(
        codes + enc.unicode_offset))
    if n <= TILE + 1:
        assert_seqs(enc.encode_device(dev(codes[None]), chunk_frames=TILE // 2 + 1, to_host=True),
                    enc.encode_codes(chunks_of(codes[None], TILE // 2 + 1)), f"n={n} chunks")


# ---- merge-kernel forms from device symbols -------------------------------------------------------------------------
def test_merge_kernel_forms_from_device_symbols():
    need_gpu()
    meta, arrays = cases.fixture()
    c = meta["trained"]["k2_unlimited"]
    enc = bpe.Encoder(1, 2 * CBS, arrays["k2_unlimited_merges"], c["n_tokens"], 1, unicode_offset=OFFSET)
    lengths = meta["threshold"]["lengths"]
    assert lengths[:5] == [3072, 3073, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1] and lengths[5] > 65536
    ran = [(1, 0, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1)]
    seqs = [arrays[f"thr_cps{i}"].astype(np.int64) - OFFSET for i in range(len(lengths))]
    want = [arrays[f"thr_ids{i}"] for i in range(len(lengths))]
    for s, ids, form, L in zip(seqs, want, ran, lengths):
        assert len(s) == L
        assert_seqs(enc.encode_device(dev(s[None]), to_host=True), [ids], L)
        assert forms(enc) == form, (L, forms(enc))
    # all forms in one call, empty items between them
    order = [0, None, 4, 3, None, 1, None, 5, None, 2, None]
    batch = np.full((len(order), 1, max(lengths)), 2 * CBS, np.int64)
    lens, mixed_want = [], []
    for b, i in enumerate(order):
        if i is not None:
            batch[b, 0, :lengths[i]] = seqs[i]
        lens.append(0 if i is None else lengths[i])
        mixed_want.append(np.zeros(0, np.int32) if i is None else want[i])
    assert_seqs(enc.encode_device(dev(batch), lens, to_host=True), mixed_want, "mixed")
    assert forms(enc) == (6, 3, 2)


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_a_code_out_of_range_is_an_error_and_the_encoder_stays_usable():
    need_gpu()
    enc = trained_encoder("k8_recipe")
    utt, ids3 = trained_codes("k8_recipe")
    for bad, where in ((-1, (0, 0)), (2048, (7, 374)), (-1, (3, 200)), (2048, (2, 17)), (INT32_MAX, (5, 5))):
        broken = utt.copy()
        broken[where] = bad
        with pytest.raises(ValueError, match="outside"):
            enc.encode_device(dev(broken))
        assert_seqs(enc.encode_device(dev(utt), to_host=True), [ids3], "after a bad code")
    # beyond an item's length the same values are never read
    assert_seqs(enc.encode_device(dev(broken), [5], to_host=True), enc.encode_codes([utt[:, :5]]), "bad code in padding")


# ---- streams and repeats --------------------------------------------------------------------------------------------
def test_streams_repeats_buffer_reuse_and_to_host():
    need_gpu()
    enc = trained_encoder("k8_recipe")
    utt, ids3 = trained_codes("k8_recipe")
    codes = dev(utt)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for s in (stream, stream.cuda_stream, None):
        assert_seqs(enc.encode_device(codes, stream=s, to_host=True), [ids3], f"stream {s}")
    int64 = dev(utt, torch.int64)
    assert_seqs(enc.encode_device(int64, stream=stream, to_host=True), [ids3], "int64 on a stream")
    a = enc.encode_device(codes, chunk_frames=100)
    b = enc.encode_device(codes, chunk_frames=100)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a small call after a larger one (the model's buffers are reused), then the larger one again
    small = enc.encode_device(codes[:, :9], to_host=True)
    assert_seqs(small, enc.encode_codes([utt[:, :9]]), "small after large")
    ids, offs, item = enc.encode_device(codes, chunk_frames=100)
    assert torch.equal(ids, a[0]) and np.array_equal(offs, a[1])
    flat = ids.cpu().numpy()
    assert_seqs(enc.encode_device(codes, chunk_frames=100, to_host=True),
                [flat[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], "to_host")
    assert_seqs([flat[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], enc.encode_codes(chunks_of(utt, 100)),
                "chunks of 100")


# ---- pipeline -------------------------------------------------------------------------------------------------------
def test_engine_codes_feed_the_encoder_without_leaving_the_device(state_dict):
    need_gpu()
    from mimi_hip.config import encoded_length
    from mimi_hip.model import MimiHipModel
    K, FR = 8, 12.5
    model = MimiHipModel(state_dict, device="cuda:0")
    enc = trained_encoder("k8_recipe")
    samples = [24000, 72000, 40001]
    audio = np.zeros((3, max(samples)), np.float32)
    for i, L in enumerate(samples):
        audio[i, :L] = synthetic.speech_like(L, 9, i)
    x = torch.from_numpy(audio).cuda()
    codes = model.encode_ragged(x, samples, K)  # int32 [3, 8, Tmax] on the device; frames past an item unspecified
    frames = [encoded_length(L, model.config) for L in samples]
    assert codes.is_cuda and codes.dtype == torch.int32 and codes.shape == (3, K, max(frames))
    host = codes.cpu().numpy()
    for cf in (int(30 * FR), 10):
        got = enc.encode_device(codes, frames, chunk_frames=cf, to_host=True)
        assert enc.last_stats["word_model"] == "device"
        want = enc.encode_codes([c for b in range(3) for c in chunks_of(host[b][:, :frames[b]].astype(np.int64), cf)])
        assert_seqs(got, want, f"pipeline cf={cf}")
    # the uniform entry: MimiHipModel.encode's codes (int64 on the device) go in as they are
    out = model.encode(x[:1, None, :samples[0]], num_quantizers=K).audio_codes
    assert out.is_cuda and out.dtype == torch.int64
    assert_seqs(enc.encode_device(out, to_host=True), enc.encode_codes([out[0].cpu().numpy()]), "model.encode")
    # the engine's next encode gives the same codes as before
    again = model.encode_ragged(x, samples, K).cpu().numpy()
    for b in range(3):
        assert np.array_equal(again[b][:, :frames[b]], host[b][:, :frames[b]])
