"""Codec-BPE decoding fixtures: what HF ``tokenizers`` 0.22.2 ``decode(ids, skip_special_tokens=True)`` followed by the
reference's ``pretraining-data/converter.py`` ``chars_to_codes`` (default flags: drop inconsistent, drop hanging)
gives for crafted id sequences (outputs are committed; needs ``tokenizers`` and the reference checkout).

    python tests/golden/make_bpe_decode_golden.py /path/to/reference

The tokenizers are those of the four trained cases of ``bpe_encode.npz`` (K = 8 recipe / unlimited, K = 2 2-gram /
unlimited).  Per case, from its 3000-character stream ``*_ids3``:

* the stream as it is; with 10 % and with 40 % of its ids deleted at random; with its ids shuffled;
* a stream starting at every codebook phase;
* special ids at the start, in the middle and at the end; an all-special stream;
* a single alphabet id, a single learned id;
* a stream whose kept count is below K.

An id sequence that decodes to the empty string is recorded with zero frames (the reference raises ``IndexError``
there; ``Encoder.decode_ids`` defines ``T = 0``).  Asserted here and again in ``tests/test_bpe_decode.py``: over the
deleted and shuffled sequences together the reference keeps between 20 % and 80 % of the characters, so neither
branch of the filter goes unexercised.
"""
import importlib.util
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
CASES = ("k8_recipe", "k8_unlimited", "k2_ngram2", "k2_unlimited")
MIXED = ("del10", "del40", "shuffled")  # the entries of the kept-fraction condition


def load_converter(reference_root):
    path = os.path.join(reference_root, "pretraining-data", "converter.py")
    spec = importlib.util.spec_from_file_location("reference_converter", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def text(cps):
    return "".join(chr(int(c)) for c in cps)


def sequences(case, K, tok, arrays, rng):
    ids3 = arrays[f"{case}_ids3"].astype(np.int64)
    cps3 = arrays[f"{case}_cps3"]
    n = ids3.size
    learned = ids3[ids3 >= cases.N_SPECIAL + K * CBS]
    out = {"ids3": ids3,
           "del10": ids3[rng.random(n) >= 0.1],
           "del40": ids3[rng.random(n) >= 0.4],
           "shuffled": rng.permutation(ids3)}
    for phase in range(K):
        out[f"phase{phase}"] = np.array(ref.hf_ids(tok, text(cps3[phase:phase + 21 * K + 3])), np.int64)
    pad = np.zeros(1, np.int64)
    out["special_start"] = np.concatenate([pad, pad, ids3[:60]])
    out["special_middle"] = np.concatenate([ids3[:30], pad, ids3[30:31], pad, pad, ids3[31:60]])
    out["special_end"] = np.concatenate([ids3[:60], pad])
    out["all_special"] = np.zeros(3, np.int64)
    out["single_alphabet"] = np.array([cases.N_SPECIAL + CBS + 5 if K > 1 else cases.N_SPECIAL + 5], np.int64)
    out["single_learned"] = learned[:1]
    assert out["single_learned"].size == 1
    # fewer kept characters than a frame: K - 1 characters from codebook 0 on
    out["below_k"] = np.array(ref.hf_ids(tok, text(cps3[:K - 1])), np.int64)
    return out


def main():
    import tokenizers
    conv = load_converter(sys.argv[1])
    meta_enc, enc = cases.fixture()
    rng = np.random.default_rng(31)
    arrays, meta = {}, {"tokenizers": tokenizers.__version__, "unicode_offset": OFFSET, "codebook_size": CBS,
                        "mixed": list(MIXED), "cases": {}}
    chars_in = chars_kept = 0
    for case in CASES:
        info = meta_enc["trained"][case]
        K, n_tokens = info["num_codebooks"], info["n_tokens"]
        tri = enc[f"{case}_merges"]
        spell = ref.spellings(tri, cases.SPECIALS, K * CBS, OFFSET, n_tokens)
        tok = ref.hf_tokenizer(spell, tri, cases.SPECIALS)
        entries = {}
        for name, ids in sequences(case, K, tok, enc, rng).items():
            chars = tok.decode([int(i) for i in ids], skip_special_tokens=True)
            if chars:
                codes = np.array(conv.chars_to_codes(chars, K, CBS, unicode_offset=OFFSET), np.int64).reshape(K, -1)
            else:
                codes = np.zeros((K, 0), np.int64)
            assert codes.size == 0 or (0 <= codes.min() and codes.max() < CBS)
            arrays[f"{case}_{name}_ids"] = ids.astype(np.int32)
            arrays[f"{case}_{name}_codes"] = codes.astype(np.int16)
            entries[name] = {"n_ids": int(ids.size), "chars": len(chars), "frames": int(codes.shape[1])}
            if name in MIXED:
                chars_in += len(chars)
                chars_kept += codes.size
        assert entries["below_k"]["frames"] == 0 and entries["below_k"]["chars"] > 0
        assert entries["ids3"]["frames"] > 0
        meta["cases"][case] = {"num_codebooks": K, "n_tokens": int(n_tokens), "entries": entries}
    frac = chars_kept / chars_in
    assert 0.2 <= frac <= 0.8, frac
    meta["mixed_kept_fraction"] = frac
    np.savez_compressed(os.path.join(HERE, "bpe_decode.npz"), **arrays)
    with open(os.path.join(HERE, "bpe_decode_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({"kept_fraction": frac, "entries": sum(len(c["entries"]) for c in meta["cases"].values())}))
    print("bytes", os.path.getsize(os.path.join(HERE, "bpe_decode.npz")))


if __name__ == "__main__":
    main()
