"""Codec-BPE encoding on the GPU (``bpe_encode.hip`` through ``mimi_bpe_encode`` / ``bpe.Encoder``): every
comparison is exact equality of id arrays with HF ``tokenizers`` 0.22.2 -- the committed fixture
(tests/golden/make_bpe_encode_golden.py) or, end to end, the tokenizer ``Trainer`` assembles."""
import numpy as np
import pytest
import torch

import bpe_encode_cases as cases
import bpe_encode_ref as ref
from mimi_hip import _lib, bpe, synthetic
from mimi_hip.codes import codes_to_chars

pytestmark = pytest.mark.gpu

OFFSET, CBS = cases.OFFSET, 2048
LDS_MAX = _lib.BPE_ENCODE_LDS_MAX_SYMBOLS


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def letters_encoder(tri, n_tokens):
    return bpe.Encoder(1, len(cases.LETTERS), tri, n_tokens, cases.N_SPECIAL, unicode_offset=OFFSET)


def assert_words(got, want, tag):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and np.array_equal(g, w), (tag, i, g.tolist(), w.tolist())


_encoders = {}


def trained_encoder(case):
    if case not in _encoders:
        meta, arrays = cases.fixture()
        c = meta["trained"][case]
        _encoders[case] = bpe.Encoder(c["num_codebooks"], CBS, arrays[f"{case}_merges"], c["n_tokens"], 1,
                                      unicode_offset=OFFSET)
    return _encoders[case]


@pytest.mark.parametrize("name", sorted(cases.HAND_MODELS))
def test_hand_models(name):
    """The local-minimum counterexample, (a,a) runs of 1..9 with (aa,a) / (a,aa) at various ranks, a reused id and a
    formed pair that out-ranks its round (flag set, result still equal), words of length 0, 1 and 2, no applicable
    merge, no merges at all."""
    need_gpu()
    _, arrays = cases.fixture()
    tri, n_tokens, _ = cases.model_triples(cases.HAND_MODELS[name])
    enc = letters_encoder(tri, n_tokens)
    words = cases.hand_words(name)
    want = cases.split(arrays[f"hand_{name}_ids"], arrays[f"hand_{name}_lens"])
    assert_words(enc.encode_words(words), want, name)
    assert enc.formed_pair_outranks == (name in cases.OUTRANKS) == ref.formed_pair_outranks(tri)
    if name.startswith("reuse_outrank"):
        assert enc.formed_pair_outranks
    assert enc.info("pairs") == len(tri) and enc.info("last_words_lds_small") == len(words)
    # each word alone, and through the string front end
    for w, ids in zip(words, want):
        assert_words(enc.encode_words([w]), [ids], name)
    got = enc.encode_strs([cases.to_str(w) for w in words])
    assert_words(got, want, name)


def test_300_random_words_in_one_call_and_batch_independence():
    need_gpu()
    meta, arrays = cases.fixture()
    enc = letters_encoder(arrays["random_merges"], meta["random"]["n_tokens"])
    words = cases.split(arrays["random_words"], arrays["random_wlens"])
    want = cases.split(arrays["random_ids"], arrays["random_lens"])
    assert len(words) == 300 and min(map(len, words)) == 0 and max(map(len, words)) == 40
    first = enc.encode_words(words)
    assert_words(first, want, "batch")
    assert enc.info("last_words_lds_small") == 300 and enc.info("last_words_global") == 0
    assert_words(enc.encode_words(words), first, "repeated call")
    for i in (0, 17, 150, 299):
        assert_words(enc.encode_words([words[i]]), [want[i]], f"word {i} alone")


@pytest.mark.parametrize("case", ["k8_recipe", "k8_unlimited", "k2_ngram2", "k2_unlimited"])
def test_trained_models(case):
    """tokenizers-trained merges, K = 2 and K = 8, with and without the n-gram limit; code strings of 1, 7, 100 and
    3000 characters (the K = 8 ones run into the characters NFKC rewrites)."""
    need_gpu()
    meta, arrays = cases.fixture()
    c = meta["trained"][case]
    enc = trained_encoder(case)
    strings = ["".join(map(chr, arrays[f"{case}_cps{i}"])) for i in range(len(c["lengths"]))]
    want = [arrays[f"{case}_ids{i}"] for i in range(len(c["lengths"]))]
    assert_words(enc.encode_strs(strings), want, case)
    assert enc.last_stats["symbols"] <= sum(c["lengths"]) and enc.last_stats["tokens"] == sum(c["n_ids"])
    # the same sequences as [K, T] code arrays (also with rows beyond num_codebooks and a batch dimension)
    K = c["num_codebooks"]
    i = len(c["lengths"]) - 1
    codes = (arrays[f"{case}_cps{i}"].astype(np.int64).reshape(-1, K).T - OFFSET - CBS * np.arange(K)[:, None])
    assert codes.min() >= 0 and codes.max() < CBS
    padded = np.concatenate([codes, np.zeros((1, codes.shape[1]), np.int64)])
    keep = padded.copy()
    got = enc.encode_codes([codes, padded, padded[None], padded[None, None]])
    assert_words(got, [want[i]] * 4, case)
    assert np.array_equal(padded, keep)  # the caller's codes are not rewritten


def test_kernel_form_boundaries():
    """One word just below, at and just above each change of kernel form (3072: small / large LDS form;
    MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS: LDS / global workspace), and one beyond 16-bit positions; the form that ran is
    what the call reports."""
    need_gpu()
    meta, arrays = cases.fixture()
    enc = trained_encoder(meta["threshold"]["model"])
    lengths = meta["threshold"]["lengths"]
    assert lengths[:5] == [3072, 3073, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1] and lengths[5] > 65536
    forms = ["small", "lds", "lds", "lds", "global", "global"]
    words = [arrays[f"thr_cps{i}"].astype(np.int32) - OFFSET + 1 for i in range(len(lengths))]
    want = [arrays[f"thr_ids{i}"] for i in range(len(lengths))]
    for w, ids, form, L in zip(words, want, forms, lengths):
        assert_words(enc.encode_words([w]), [ids], L)
        ran = (enc.info("last_words_lds_small"), enc.info("last_words_lds"), enc.info("last_words_global"))
        assert ran == {"small": (1, 0, 0), "lds": (0, 1, 0), "global": (0, 0, 1)}[form], (L, ran)
    # all forms in one call, short words between them
    mixed = [words[0], np.zeros(0, np.int32), words[4], words[3], words[1][:5], words[5], words[2]]
    mixed_want = [want[0], np.zeros(0, np.int32), want[4], want[3], enc.encode_words([words[1][:5]])[0], want[5],
                  want[2]]
    assert_words(enc.encode_words(mixed), mixed_want, "mixed")
    assert (enc.info("last_words_lds_small"), enc.info("last_words_lds"), enc.info("last_words_global")) == (3, 2, 2)


def test_every_character_class():
    need_gpu()
    _, arrays = cases.fixture()
    enc = trained_encoder("k8_recipe")
    codes = arrays["chars_codes"].astype(np.int64)
    assert_words(enc.encode_codes([codes]), [arrays["chars_ids"]], "chars")
    assert enc.last_stats["words"] > 1  # the splitting characters cut the sequence
    assert_words(enc.encode_strs([codes_to_chars(codes, CBS)]), [arrays["chars_ids"]], "chars str")


def test_bad_symbol_id_is_an_error_and_the_model_stays_usable():
    need_gpu()
    meta, arrays = cases.fixture()
    enc = letters_encoder(arrays["random_merges"], meta["random"]["n_tokens"])
    words = cases.split(arrays["random_words"], arrays["random_wlens"])
    want = cases.split(arrays["random_ids"], arrays["random_lens"])
    for bad in (meta["random"]["n_tokens"], -1, 1 << 20):
        broken = [w.copy() for w in words[:20]]
        broken[7] = np.append(broken[7], np.int32(bad))
        with pytest.raises(ValueError, match="outside"):
            enc.encode_words(broken)
        assert_words(enc.encode_words(words[:20]), want[:20], "after a bad id")
    # the highest valid id passes through
    top = np.array([meta["random"]["n_tokens"] - 1], np.int32)
    assert_words(enc.encode_words([top]), [top], "top id")


def test_non_default_stream():
    need_gpu()
    meta, arrays = cases.fixture()
    enc = letters_encoder(arrays["random_merges"], meta["random"]["n_tokens"])
    words = cases.split(arrays["random_words"], arrays["random_wlens"])
    want = cases.split(arrays["random_ids"], arrays["random_lens"])
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    assert_words(enc.encode_words(words, stream=stream), want, "stream")
    assert_words(enc.encode_words(words, stream=stream.cuda_stream), want, "raw stream")
    assert_words(enc.encode_words(words), want, "default stream")


def test_encode_train_then_encode_codes(state_dict):
    """End to end on the pattern of tests/test_pipeline_gpu.py: encode synthetic clips, train, then
    ``Encoder.from_trainer(...).encode_codes`` over the 30 s chunks equals the ids of the tokenizer the trainer
    assembled (live ``tokenizers``), and ``from_tokenizer`` of that object gives the same."""
    need_gpu()
    from mimi_hip.encoder import MimiEncoder
    from mimi_hip.model import MimiHipModel
    NCB, FR, CHUNK_S = 8, 12.5, 30
    model = MimiHipModel(state_dict, device="cuda:0")
    mimi = MimiEncoder(device="cuda:0", model=model, num_quantizers=NCB, concurrency=2)
    lengths = synthetic.random_lengths(6, 10.0, 20.0, seed=43)
    audio = [synthetic.speech_like(L, 43, i) for i, L in enumerate(lengths)]
    audio += audio[:3]
    codes = mimi.encode_audio_chunks(audio, 24000)
    tr = bpe.Trainer(NCB, CBS, codec_framerate=FR, chunk_size_secs=CHUNK_S, vocab_size=NCB * CBS + 1 + 300,
                     min_frequency=2, pad_token="<pad>", max_token_codebook_ngrams=2)
    tok = tr.train_codes([c.copy() for c in codes])
    assert len(tr.last_merges) > 0
    step = int(CHUNK_S * FR)
    chunks = [c[:, i:i + step].copy() for c in codes for i in range(0, c.shape[1], step)]
    want = [np.array(ref.hf_ids(tok, codes_to_chars(c.copy(), CBS)), np.int32) for c in chunks]
    enc = bpe.Encoder.from_trainer(tr)
    got = enc.encode_codes(chunks)
    assert_words(got, want, "from_trainer")
    assert sum(map(len, got)) < sum(c.size for c in chunks)  # merges applied
    enc2 = bpe.Encoder.from_tokenizer(tok, NCB, CBS)
    assert np.array_equal(enc.merges, enc2.merges)
    assert_words(enc2.encode_codes(chunks), want, "from_tokenizer")
