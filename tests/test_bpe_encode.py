"""Codec-BPE encoding, CPU side: the plain-Python restatement of the merge rule (tests/bpe_encode_ref.py) and the
host character model are pinned against HF ``tokenizers`` 0.22.2 -- the committed fixture
(tests/golden/make_bpe_encode_golden.py) and, where ``tokenizers`` is importable, the library itself; plus the
``bpe.Encoder`` argument checks, its constructors, and the C ABI's new exports."""
import json
import os
import random
import re

import numpy as np
import pytest

import bpe_encode_cases as cases
import bpe_encode_ref as ref
from mimi_hip import _lib, bpe
from mimi_hip.codes import codes_to_chars, codes_to_codepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mimi_hip.h")
NEW = ("mimi_bpe_model_create", "mimi_bpe_model_destroy", "mimi_bpe_encode")
OFFSET, CBS = cases.OFFSET, 2048


def ref_encode_codepoints(cps, chars, table, n_special):
    out = []
    for w in chars.words(np.asarray(cps, dtype=np.int64)):
        out += ref.encode_word(w + n_special, table)
    return out


def test_library_exports_the_encode_symbols():
    with open(HEADER) as f:
        text = f.read()
    lib = _lib.load()
    for sym in NEW + ("mimi_bpe_model_info",):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"^\w[\w\s\*]*\b%s\(" % sym, text, re.M), sym  # a declaration, not a mention in a comment
        assert getattr(lib, sym).argtypes is not None
    m = re.search(r"#define MIMI_BPE_ENCODE_LDS_MAX_SYMBOLS (\d+)", text)
    assert int(m.group(1)) == _lib.BPE_ENCODE_LDS_MAX_SYMBOLS == bpe.Encoder.LDS_MAX_SYMBOLS
    for key, value in _lib.BPE_INFO.items():
        assert re.search(r"#define MIMI_BPE_INFO_%s %d\b" % (key.upper(), value), text), key
    assert "estimate_tokens.py:75" in text


def test_null_model_calls_fail_without_gpu_work():
    lib = _lib.load()
    assert lib.mimi_bpe_encode(None, None, None, 0, None, None, None) == 1
    assert lib.mimi_bpe_model_create(0, None, 1, 8, None) == 1
    lib.mimi_bpe_model_destroy(None)


@pytest.mark.parametrize("name", sorted(cases.HAND_MODELS))
def test_restatement_matches_fixture_on_hand_models(name):
    meta, arrays = cases.fixture()
    tri, n_tokens, _ = cases.model_triples(cases.HAND_MODELS[name])
    assert n_tokens == meta["hand"][name]["n_tokens"]
    table = ref.merge_table(tri)
    words = cases.hand_words(name)
    want = cases.split(arrays[f"hand_{name}_ids"], arrays[f"hand_{name}_lens"])
    assert len(words) == len(want)
    for w, ids in zip(words, want):
        assert ref.encode_word(w, table) == ids.tolist() == ref.encode_word_naive(w, table), (name, w)
    assert ref.formed_pair_outranks(tri) == (name in cases.OUTRANKS)


def test_local_minimum_counterexample():
    """merges 1:(w,x)->p, 2:(p,a)->z, 3:(a,b)->n: ``w x a b`` gives ``z b``, not ``p n``."""
    tri, _, spell = cases.model_triples(cases.HAND_MODELS["local_min"])
    got = ref.encode_word(cases.word("abcd"), ref.merge_table(tri))
    assert [spell[i] for i in got] == ["abc", "d"]


def test_restatement_matches_fixture_on_random_words():
    meta, arrays = cases.fixture()
    tri, n_tokens, _, words = cases.random_model_and_words()
    assert np.array_equal(tri, arrays["random_merges"]) and n_tokens == meta["random"]["n_tokens"]
    assert all(np.array_equal(a, b) for a, b in zip(words, cases.split(arrays["random_words"], arrays["random_wlens"])))
    table = ref.merge_table(tri)
    for w, ids in zip(words, cases.split(arrays["random_ids"], arrays["random_lens"])):
        assert ref.encode_word(w, table) == ids.tolist()


@pytest.mark.parametrize("case", ["k8_recipe", "k8_unlimited", "k2_ngram2", "k2_unlimited"])
def test_restatement_and_host_model_match_fixture_on_trained_models(case):
    meta, arrays = cases.fixture()
    c = meta["trained"][case]
    chars = bpe.CharModel(OFFSET, c["num_codebooks"] * CBS)
    table = ref.merge_table(arrays[f"{case}_merges"])
    for i, L in enumerate(c["lengths"]):
        cps = arrays[f"{case}_cps{i}"]
        assert cps.size == L
        got = ref_encode_codepoints(cps, chars, table, 1)
        assert got == arrays[f"{case}_ids{i}"].tolist(), (case, L)
    assert c["n_ids"][-1] < 0.7 * c["lengths"][-1]  # merges do apply


def test_restatement_matches_fixture_around_the_kernel_form_boundaries():
    meta, arrays = cases.fixture()
    table = ref.merge_table(arrays["k2_unlimited_merges"])
    assert meta["threshold"]["lengths"][:5] == [3072, 3073, _lib.BPE_ENCODE_LDS_MAX_SYMBOLS - 1,
                                                _lib.BPE_ENCODE_LDS_MAX_SYMBOLS, _lib.BPE_ENCODE_LDS_MAX_SYMBOLS + 1]
    for i, L in enumerate(meta["threshold"]["lengths"]):
        w = arrays[f"thr_cps{i}"].astype(np.int64) - OFFSET + 1
        assert w.size == L
        assert ref.encode_word(w, table) == arrays[f"thr_ids{i}"].tolist(), L


def test_host_model_matches_fixture_on_every_character_class():
    meta, arrays = cases.fixture()
    codes = arrays["chars_codes"].astype(np.int64)
    cps = codes_to_codepoints(codes, CBS)
    chars = bpe.CharModel(OFFSET, 8 * CBS)
    cls = set(chars.cls[cps - OFFSET].tolist())
    assert cls == {bpe.KEEP_STARTER, bpe.KEEP_MARK, bpe.DROP_STARTER, bpe.DROP_MARK, bpe.SPLIT}
    words = chars.words(cps)
    assert len(words) > 1
    keep = np.isin(chars.cls[cps - OFFSET], (bpe.KEEP_STARTER, bpe.KEEP_MARK))
    assert (np.concatenate(words) != (cps - OFFSET)[keep]).any()  # some marks were out of canonical order
    got = ref_encode_codepoints(cps, chars, ref.merge_table(arrays["k8_recipe_merges"]), 1)
    assert got == arrays["chars_ids"].tolist()


# ---- live tokenizers ---------------------------------------------------------------------------------
def letters_tokenizer(spell, tri):
    sp = [s if i < cases.N_SPECIAL else "".join(chr(OFFSET + cases.LETTERS.index(c)) for c in s)
          for i, s in enumerate(spell)]
    return ref.hf_tokenizer(sp, tri, cases.SPECIALS)


def test_restatement_matches_live_tokenizers_on_hand_models():
    tokenizers = pytest.importorskip("tokenizers")
    rng = random.Random(5)
    for name, pairs in cases.HAND_MODELS.items():
        tri, _, spell = cases.model_triples(pairs)
        tok, table = letters_tokenizer(spell, tri), ref.merge_table(tri)
        letters = "abc" if name.startswith(("runs", "reuse")) else cases.LETTERS
        words = cases.hand_words(name) + [cases.word("".join(rng.choice(letters) for _ in range(rng.randint(0, 30))))
                                          for _ in range(200)]
        for w in words:
            assert ref.hf_ids(tok, cases.to_str(w)) == ref.encode_word(w, table), (name, w, tokenizers.__version__)


def test_fixture_matches_live_tokenizers():
    tokenizers = pytest.importorskip("tokenizers")
    meta, arrays = cases.fixture()
    if tokenizers.__version__ != meta["tokenizers"]:
        pytest.skip(f"fixture made with tokenizers {meta['tokenizers']}")
    for case, c in meta["trained"].items():
        tri = arrays[f"{case}_merges"]
        spell = ref.spellings(tri, cases.SPECIALS, c["num_codebooks"] * CBS, OFFSET, c["n_tokens"])
        tok = ref.hf_tokenizer(spell, tri, cases.SPECIALS)
        for i in range(len(c["lengths"])):
            s = "".join(map(chr, arrays[f"{case}_cps{i}"]))
            assert ref.hf_ids(tok, s) == arrays[f"{case}_ids{i}"].tolist()
        if case == "k8_recipe":
            s = codes_to_chars(arrays["chars_codes"].astype(np.int64), CBS)
            assert ref.hf_ids(tok, s) == arrays["chars_ids"].tolist()


def test_host_model_matches_live_tokenizers_per_character_class():
    """Each class of the character model on its own (and all together) against tokenizers' encode: the
    characters NFKC rewrites and the Metaspace mark give no id under ``unk_token=None``, splits only cut the word,
    marks are reordered before the merges see them."""
    pytest.importorskip("tokenizers")
    _, arrays = cases.fixture()
    tri = arrays["k8_recipe_merges"]
    spell = ref.spellings(tri, cases.SPECIALS, 8 * CBS, OFFSET, int(tri.max()) + 1)
    tok, table = ref.hf_tokenizer(spell, tri, cases.SPECIALS), ref.merge_table(tri)
    chars = bpe.CharModel(OFFSET, 8 * CBS)
    base = arrays["chars_codes"].astype(np.int64)
    plain = np.nonzero(chars.cls == bpe.KEEP_STARTER)[0]
    rng = np.random.default_rng(2)
    for classes in ([bpe.KEEP_MARK], [bpe.DROP_STARTER], [bpe.DROP_MARK], [bpe.SPLIT],
                    [bpe.KEEP_MARK, bpe.DROP_MARK], [1, 2, 3, 4]):
        pool = np.nonzero(np.isin(chars.cls, classes))[0]
        for _ in range(40):
            idx = codes_to_codepoints(base[:, :int(rng.integers(1, 40))].copy(), CBS) - OFFSET
            idx = np.where(np.isin(chars.cls[idx], (bpe.KEEP_STARTER,)), idx, plain[idx % plain.size])
            hit = rng.random(idx.size) < 0.3
            idx[hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
            cps = idx + OFFSET
            assert ref.hf_ids(tok, "".join(map(chr, cps))) == ref_encode_codepoints(cps, chars, table, 1), classes


# ---- bpe.Encoder: arguments and constructors -----------------------------------------------------------
def trainer_with_fixture_model(case="k8_recipe"):
    meta, arrays = cases.fixture()
    c = meta["trained"][case]
    K = c["num_codebooks"]
    tri = arrays[f"{case}_merges"]
    tr = bpe.Trainer(K, CBS, codec_framerate=12.5, chunk_size_secs=30, vocab_size=c["n_tokens"], pad_token="<pad>")
    spell = [()] + [(i,) for i in range(K * CBS)]
    for a, b, n in tri:
        if n == len(spell):
            spell.append(spell[a] + spell[b])
        assert spell[n] == spell[a] + spell[b]
    tr.last_tokens = spell[1 + K * CBS:]
    tr.last_merges = [(int(a), int(b)) for a, b, _ in tri]
    return tr, tri, c


def test_encoder_argument_checks():
    with pytest.raises(NotImplementedError, match="unk_token"):
        bpe.Encoder(1, 6, [], 7, 1, unk_token="<unk>")
    with pytest.raises(ValueError, match="below"):
        bpe.Encoder(1, 6, [], 6, 1)
    with pytest.raises(ValueError, match="merge ids outside"):
        bpe.Encoder(1, 6, [(1, 2, 7)], 7, 1)
    with pytest.raises(ValueError, match="131071"):
        bpe.Encoder(8, 2048, [], (1 << 17) + 1, 1)
    with pytest.raises(ValueError, match="outside valid code points"):
        bpe.Encoder(8, 2048, [], 20000, 1, unicode_offset=0x10F000)
    enc = bpe.Encoder(1, 6, [(1, 2, 7)], 8, 1)
    assert enc.merges.dtype == np.int32 and enc.merges.shape == (1, 3)
    with pytest.raises(ValueError, match="outside the trainer's alphabet"):
        enc._chars.words(np.array([0x41]))


def test_from_trainer_gives_the_fixture_table():
    tr, tri, c = trainer_with_fixture_model()
    enc = bpe.Encoder.from_trainer(tr)
    assert np.array_equal(enc.merges, tri) and enc.n_tokens == c["n_tokens"] and enc.n_special == 1
    tr.unk_token = "<unk>"
    with pytest.raises(NotImplementedError, match="unk_token"):
        bpe.Encoder.from_trainer(tr)


def test_from_tokenizer_and_from_trainer_give_the_same_table(tmp_path):
    pytest.importorskip("tokenizers")
    tr, tri, c = trainer_with_fixture_model()
    tok = tr._assemble(tr.last_tokens, tr.last_merges)  # a PreTrainedTokenizerFast where transformers is importable
    backend = getattr(tok, "backend_tokenizer", tok)
    path = tmp_path / "tokenizer.json"
    backend.save(str(path))
    a = bpe.Encoder.from_trainer(tr)
    for source in (tok, backend, str(path)):
        b = bpe.Encoder.from_tokenizer(source, 8, CBS)
        assert np.array_equal(a.merges, b.merges) and (a.n_tokens, a.n_special) == (b.n_tokens, b.n_special)
        assert b.unicode_offset == OFFSET
    with pytest.raises(ValueError, match="code point order"):
        bpe.Encoder.from_tokenizer(backend, 8, CBS, unicode_offset=0xE001)
    j = json.loads(backend.to_str())
    j["model"]["unk_token"] = "<pad>"
    path.write_text(json.dumps(j), encoding="utf-8")
    with pytest.raises(NotImplementedError, match="unk_token"):
        bpe.Encoder.from_tokenizer(str(path), 8, CBS)
