"""Codec-BPE encoding fixtures: what HF ``tokenizers`` 0.22.2 gives for the cases of ``tests/test_bpe_encode.py``
and ``tests/test_bpe_encode_gpu.py`` (outputs are committed; needs ``tokenizers`` only).

    python tests/golden/make_bpe_encode_golden.py

Every expected id array is ``tok.encode(text, add_special_tokens=False).ids`` of the tokenizer
``mimi_hip.bpe.Trainer`` assembles (BPE with ``unk_token=None``, NFKC, Metaspace without prefix):

* hand-built models over a 6-letter alphabet and a small trained one with 300 random words
  (``tests/bpe_encode_cases.py``);
* trained models: K = 8 (the ``tokenizers``-trained merges of ``bpe.npz``, recipe and unlimited) and K = 2
  (trained here on a low-entropy Markov source, 2-gram limit and unlimited), each with code strings of 1, 7, 100
  and 3000 characters;
* single words around the kernel-form boundaries of the GPU encoder (3072 / 3073, 8191 / 8192 / 8193 and 70001
  characters) under the unlimited K = 2 model;
* one K = 8 code array holding every character class of the NFKC model (kept, dropped, splitting, and combining
  marks out of canonical order).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bpe_encode_cases as cases  # noqa: E402
import bpe_encode_ref as ref  # noqa: E402

OFFSET, CBS = 0xE000, 2048
SEQ_LENGTHS = (1, 7, 100, 3000)
THRESHOLD_LENGTHS = (3072, 3073, 8191, 8192, 8193, 70001)


K2_VALUES = np.stack([np.random.default_rng(100 + k).permutation(CBS)[:10] for k in range(2)])


def k2_codes(rng, T):
    """Low-entropy two-codebook codes: 10 Zipf-weighted values per codebook, frames often repeated."""
    vals = K2_VALUES
    p = 1.0 / np.arange(1, 11) ** 1.2
    p /= p.sum()
    codes = np.empty((2, T), np.int64)
    for t in range(T):
        if t > 0 and rng.random() < 0.3:
            codes[:, t] = codes[:, t - 1]
        else:
            codes[:, t] = vals[np.arange(2), rng.choice(10, 2, p=p)]
    return codes


def codepoints(codes):
    K = codes.shape[0]
    return (codes + OFFSET + CBS * np.arange(K)[:, None]).T.reshape(-1).astype(np.uint32)


def text(cps):
    return "".join(chr(int(c)) for c in cps)


def train_k2(strings, n_merges, max_len):
    from tokenizers import Tokenizer, pre_tokenizers, trainers
    from tokenizers.models import BPE
    from tokenizers.normalizers import NFKC
    tok = Tokenizer(BPE(unk_token=None))
    tok.normalizer = NFKC()
    tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="never")
    alphabet = [chr(i) for i in range(OFFSET, OFFSET + 2 * CBS)]
    tok.train_from_iterator(strings, trainer=trainers.BpeTrainer(
        vocab_size=1 + len(alphabet) + n_merges, min_frequency=2, special_tokens=["<pad>"],
        limit_alphabet=len(alphabet), initial_alphabet=alphabet, max_token_length=max_len, show_progress=False))
    j = json.loads(tok.to_str())
    vocab = j["model"]["vocab"]
    tri = np.array([(vocab[a], vocab[b], vocab[a + b]) for a, b in map(tuple, j["model"]["merges"])], np.int32)
    return tri.reshape(-1, 3), len(vocab)


def char_class_codes(base, rng):
    """A K = 8 code array dense in the characters NFKC rewrites, splits on and reorders (as
    tests/test_bpe.py::test_char_model_matches_tokenizers_pretokenization), over frames of the training corpus so
    that merges still apply."""
    from mimi_hip import bpe
    m = bpe.CharModel(OFFSET, 8 * CBS)
    # per codebook, the codes of each class other than the plain one (a class first, then one of its characters:
    # only 2 characters are dropped marks and 21 split)
    by_cb = []
    for k in range(8):
        cls_k = m.cls[k * CBS:(k + 1) * CBS]
        by_cb.append([np.nonzero(cls_k == c)[0] for c in range(1, 5) if (cls_k == c).any()])
    codes = base.copy()
    for t in range(codes.shape[1]):
        for k in range(8):
            if by_cb[k] and rng.random() < 0.3:
                group = by_cb[k][rng.integers(len(by_cb[k]))]
                codes[k, t] = group[rng.integers(len(group))]
    cps = codepoints(codes).astype(np.int64)
    cls = m.cls[cps - OFFSET]
    assert set(cls.tolist()) == {bpe.KEEP_STARTER, bpe.KEEP_MARK, bpe.DROP_STARTER, bpe.DROP_MARK, bpe.SPLIT}
    # some marks do come out of canonical order: the words differ from the unsorted ones
    kept = np.concatenate([w for w in m.words(cps)])
    unsorted = (cps - OFFSET)[(cls == bpe.KEEP_STARTER) | (cls == bpe.KEEP_MARK)]
    assert kept.size == unsorted.size and (kept != unsorted).any(), "no mark was reordered"
    return codes


def main():
    import tokenizers
    arrays, meta = {}, {"tokenizers": tokenizers.__version__, "unicode_offset": OFFSET, "codebook_size": CBS,
                        "special_tokens": cases.SPECIALS, "hand": {}, "trained": {}}

    def letters_tok(spell, tri):
        sp = [s if i < cases.N_SPECIAL else "".join(chr(OFFSET + cases.LETTERS.index(c)) for c in s)
              for i, s in enumerate(spell)]
        return ref.hf_tokenizer(sp, tri, cases.SPECIALS)

    def put_words(prefix, tok, words):
        ids = [np.array(ref.hf_ids(tok, cases.to_str(w)), np.int32) for w in words]
        arrays[prefix + "_ids"] = np.concatenate(ids) if ids else np.zeros(0, np.int32)
        arrays[prefix + "_lens"] = np.array([len(i) for i in ids], np.int32)

    # hand-built models
    for name, pairs in cases.HAND_MODELS.items():
        tri, n_tokens, spell = cases.model_triples(pairs)
        put_words("hand_" + name, letters_tok(spell, tri), cases.hand_words(name))
        meta["hand"][name] = {"n_tokens": n_tokens, "n_words": len(cases.hand_words(name))}
    tri, n_tokens, spell, words = cases.random_model_and_words()
    arrays["random_merges"] = tri
    arrays["random_words"] = np.concatenate(words).astype(np.int32)
    arrays["random_wlens"] = np.array([len(w) for w in words], np.int32)
    put_words("random", letters_tok(spell, tri), words)
    meta["random"] = {"n_tokens": n_tokens, "n_words": len(words)}

    # trained models
    with np.load(os.path.join(HERE, "bpe.npz")) as z:
        k8 = {k: z[k] for k in z.files}
    with open(os.path.join(HERE, "bpe_meta.json")) as f:
        k8_meta = json.load(f)
    rng = np.random.default_rng(21)
    k2_train = [text(codepoints(k2_codes(rng, int(rng.integers(40, 400))))) for _ in range(60)]
    models = {}
    for name in ("recipe", "unlimited"):
        models["k8_" + name] = (8, k8[name + "_merges"], k8_meta["cases"][name]["final_vocab"])
    for name, max_len in (("ngram2", 2 * 2 + 1), ("unlimited", None)):
        tri, n_tokens = train_k2(k2_train, 800, max_len)
        arrays[f"k2_{name}_merges"] = tri
        models["k2_" + name] = (2, tri, n_tokens)
    long_utt = max((k8[f"utt{i}"] for i in range(k8_meta["n_utterances"])), key=lambda u: u.shape[1]).astype(np.int64)
    assert long_utt.shape[1] >= 375
    toks = {}
    for case, (K, tri, n_tokens) in models.items():
        spell = ref.spellings(tri, cases.SPECIALS, K * CBS, OFFSET, n_tokens)
        tok = toks[case] = ref.hf_tokenizer(spell, tri, cases.SPECIALS)
        full = codepoints(long_utt[:, 20:20 + 375]) if K == 8 else codepoints(k2_codes(rng, 1500))
        assert full.size == 3000
        for i, L in enumerate(SEQ_LENGTHS):
            arrays[f"{case}_cps{i}"] = full[:L]
            arrays[f"{case}_ids{i}"] = np.array(ref.hf_ids(tok, text(full[:L])), np.int32)
        meta["trained"][case] = {"num_codebooks": K, "n_tokens": int(n_tokens), "n_merges": int(len(tri)),
                                 "lengths": list(SEQ_LENGTHS),
                                 "n_ids": [int(arrays[f"{case}_ids{i}"].size) for i in range(len(SEQ_LENGTHS))]}

    # kernel-form boundaries: single words (K = 2 code characters are all plain private-use characters)
    for i, L in enumerate(THRESHOLD_LENGTHS):
        cps = codepoints(k2_codes(rng, (L + 1) // 2))[:L]
        arrays[f"thr_cps{i}"] = cps
        arrays[f"thr_ids{i}"] = np.array(ref.hf_ids(toks["k2_unlimited"], text(cps)), np.int32)
    meta["threshold"] = {"model": "k2_unlimited", "lengths": list(THRESHOLD_LENGTHS),
                         "n_ids": [int(arrays[f"thr_ids{i}"].size) for i in range(len(THRESHOLD_LENGTHS))]}

    # every character class
    codes = char_class_codes(long_utt[:, 100:220], rng)
    arrays["chars_codes"] = codes.astype(np.int16)
    arrays["chars_ids"] = np.array(ref.hf_ids(toks["k8_recipe"], text(codepoints(codes))), np.int32)
    meta["chars"] = {"model": "k8_recipe", "frames": int(codes.shape[1]), "n_ids": int(arrays["chars_ids"].size)}

    np.savez_compressed(os.path.join(HERE, "bpe_encode.npz"), **arrays)
    with open(os.path.join(HERE, "bpe_encode_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: meta[k] for k in ("trained", "threshold", "chars")}))
    print("bytes", os.path.getsize(os.path.join(HERE, "bpe_encode.npz")))


if __name__ == "__main__":
    main()
