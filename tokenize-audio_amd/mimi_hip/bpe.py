"""Codec-BPE training over emitted Mimi codes, with the merge loop on the GPU.

Mirrors the reference recipe's trainer (``/root/reference/codec-bpe/bpe_trainer.py``, which replaces codec_bpe's
``core/trainer.py``; run as ``python -m codec_bpe.train_tokenizer`` in ``codec-bpe/train_bpe_recipe.txt:18-28``):

* ``Trainer(num_codebooks, codebook_size, codec_framerate, chunk_size_secs, vocab_size, min_frequency,
  special_tokens, bos/eos/unk/pad_token, max_token_codebook_ngrams, unicode_offset)`` -- same arguments, checks
  and error messages (``bpe_trainer.py:12-71``);
* ``train(codes_path, codes_filter, num_files)`` -- ``.npy`` code files (one array, or an object array of
  per-utterance ``[num_codebooks, T]`` arrays), cut into ``chunk_size_secs`` chunks, each chunk one
  training sequence of ``codes_to_chars`` characters (``bpe_trainer.py:73-105``), base alphabet = all
  ``num_codebooks * codebook_size`` code characters, tokens at most ``max_token_codebook_ngrams *
  num_codebooks`` characters (``:107-166``).

The reference trains through HF ``tokenizers`` (codec_bpe's ``SentencePieceBPETokenizer``: NFKC normalizer,
Metaspace pre-tokenizer, ``BpeTrainer``).  Here:

1. host (numpy): codes -> code points per chunk -> the normalizer's effect on them -> words.  The code
   characters run into Unicode blocks that NFKC rewrites (codebook 3 at offset 0xE000 covers U+F800-U+FFFF:
   1,539 characters change, 21 into text containing a space, where the pre-tokenizer splits the chunk) and
   into combining marks that NFKC reorders.  ``data/bpe_unicode.json`` records what ``tokenizers`` does with
   every such character (``tools/make_bpe_unicode.py``); per chunk: characters NFKC replaces are dropped (their
   replacements are never code characters, so the trainer's alphabet filter drops them), those whose
   replacement holds a space split the word, and the surviving combining marks are stably sorted by combining
   class inside each run between starters -- exactly the words ``tokenizers`` trains on
   (``tests/test_bpe.py`` checks it against ``tokenizers`` itself);
2. GPU (``bpe.hip`` through ``mimi_bpe_*``): pair counts in a device hash table, one merge per step applied to
   every word in parallel (left-to-right occurrence rule, count deltas), best pair by a packed 64-bit max
   (count, then smallest pair) -- the ``BpeTrainer`` rules restated in ``oracle/bpe_ref.py``;
3. the trained vocabulary and merges are assembled into the same ``tokenizers`` BPE tokenizer (NFKC,
   Metaspace) and, when ``transformers`` is importable, a ``PreTrainedTokenizerFast`` as the reference returns.

One quirk is kept rather than fixed: the reference adds the offsets in the codes' own dtype
(``codes_to_chars(..., copy_before_conversion=False)``); on uint16 files with 8 codebooks that overflows
(numpy >= 2 raises OverflowError, numpy 1.x wraps codebooks 4-7 to U+0000-U+1FFF).  ``codes_to_codepoints``
does the same add, so the same inputs fail or wrap the same way.
"""
from __future__ import annotations

import ctypes
import glob
import json
import os
import time
import warnings
import weakref
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .codes import UNICODE_OFFSET, codes_to_codepoints

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "bpe_unicode.json")

# character classes of the normalizer model
KEEP_STARTER, KEEP_MARK, DROP_STARTER, DROP_MARK, SPLIT = 0, 1, 2, 3, 4


def validate_unicode_offset(unicode_offset: int, num_codebooks: int, codebook_size: int) -> int:
    end = unicode_offset + num_codebooks * codebook_size
    if unicode_offset < 0 or end > 0x110000 or (unicode_offset < 0xE000 and end > 0xD800):
        raise ValueError(f"unicode_offset {unicode_offset:#x} puts the {num_codebooks} x {codebook_size} code "
                         f"characters outside valid code points")
    return unicode_offset


_unicode = None


def _unicode_data():
    global _unicode
    if _unicode is None:
        with open(_DATA) as f:
            d = json.load(f)
        _unicode = ({int(k): v for k, v in d["nfkc"].items()}, {int(k): v for k, v in d["ccc"].items()})
    return _unicode


class CharModel:
    """Class and combining class of each code character under tokenizers' NFKC (see module docstring)."""

    def __init__(self, first: int, count: int):
        nfkc, ccc = _unicode_data()
        self.first, self.count = first, count
        self.cls = np.zeros(count, np.uint8)
        self.ccc = np.zeros(count, np.uint8)
        for cp in range(first, first + count):
            out = nfkc.get(cp)
            i = cp - first
            if out is None:
                c = ccc.get(cp, 0)
                self.ccc[i] = c
                self.cls[i] = KEEP_MARK if c else KEEP_STARTER
                continue
            if any(first <= o < first + count for o in out):
                raise NotImplementedError(f"NFKC maps code character {cp:#x} onto another code character")
            if 0x20 in out:
                self.cls[i] = SPLIT
            elif any(ccc.get(o, 0) == 0 for o in out):
                self.cls[i] = DROP_STARTER
            else:
                self.cls[i] = DROP_MARK

    def words(self, cps: np.ndarray) -> List[np.ndarray]:
        """Code points of one training sequence -> the alphabet indices of each of its words (tokenizers'
        NFKC + Metaspace split + alphabet filter)."""
        idx = cps.astype(np.int64) - self.first
        if idx.size == 0:
            return [idx]
        if idx.min() < 0 or idx.max() >= self.count:
            raise ValueError("code characters outside the trainer's alphabet")
        cls = self.cls[idx]
        marks = np.nonzero(cls == KEEP_MARK)[0]
        if marks.size > 1:
            # canonical ordering: stable sort of the kept marks by combining class inside each run of
            # non-starters (dropped marks take part in the run but do not survive, so they cannot reorder)
            starter = (cls == KEEP_STARTER) | (cls == DROP_STARTER) | (cls == SPLIT)
            run = np.cumsum(starter)[marks]
            key = run.astype(np.int64) * 256 + self.ccc[idx[marks]]
            order = np.argsort(key, kind="stable")
            if (order != np.arange(order.size)).any():
                idx = idx.copy()
                idx[marks] = idx[marks[order]]
        keep = (cls == KEEP_STARTER) | (cls == KEEP_MARK)
        splits = np.nonzero(cls == SPLIT)[0]
        if splits.size == 0:
            return [idx[keep]]
        out, start = [], 0
        for s in splits:
            seg = slice(start, s)
            out.append(idx[seg][keep[seg]])
            start = s + 1
        out.append(idx[start:][keep[start:]])
        return out


def get_codes_files(codes_path: str, codes_filter: Optional[Union[str, List[str]]] = None,
                    num_files: Optional[int] = None) -> List[str]:
    """``.npy`` files under codes_path (sorted); codes_filter keeps paths containing (any of) the filter
    string(s); num_files keeps the first n."""
    files = sorted(glob.glob(os.path.join(codes_path, "**", "*.npy"), recursive=True))
    if codes_filter:
        flt = [codes_filter] if isinstance(codes_filter, str) else list(codes_filter)
        files = [f for f in files if any(x in f for x in flt)]
    if num_files is not None:
        files = files[:num_files]
    if not files:
        raise ValueError(f"no codes files found in {codes_path}")
    return files


def _utterances(codes_file: str) -> List[np.ndarray]:
    codes_data = np.load(codes_file, allow_pickle=True)  # the reference's loader (object arrays of utterances)
    if isinstance(codes_data, np.ndarray) and codes_data.dtype == object and len(codes_data.shape) == 0:
        codes_list = codes_data.item()
        if not isinstance(codes_list, list):
            codes_list = [codes_list]
    elif isinstance(codes_data, np.ndarray) and codes_data.dtype == object and len(codes_data.shape) == 1:
        codes_list = list(codes_data)
    else:
        codes_list = [codes_data]
    return codes_list


class Trainer:
    def __init__(self, num_codebooks: int, codebook_size: int, codec_framerate: Optional[float] = None,
                 chunk_size_secs: Optional[int] = None, vocab_size: int = 30000, min_frequency: int = 2,
                 special_tokens: Optional[List[str]] = None, bos_token: Optional[str] = None,
                 eos_token: Optional[str] = None, unk_token: Optional[str] = None, pad_token: Optional[str] = None,
                 max_token_codebook_ngrams: Optional[int] = None, unicode_offset: int = UNICODE_OFFSET,
                 device: Union[int, str] = 0):
        if chunk_size_secs is not None:
            if codec_framerate is None:
                raise ValueError("If chunk_size_secs is set, codec_framerate must also be set.")
            if chunk_size_secs < 1:
                raise ValueError("chunk_size_secs must be a positive integer >= 1.")
        if eos_token is None and pad_token is None:
            raise ValueError(
                "Either pad_token or eos_token should be set, otherwise padded batching will not work with this "
                "tokenizer.")
        if max_token_codebook_ngrams is not None and max_token_codebook_ngrams < 0:
            raise ValueError("max_token_codebook_ngrams must be a non-negative integer (0 or greater).")
        self.num_codebooks = num_codebooks
        self.codebook_size = codebook_size
        self.codec_framerate = codec_framerate
        self.chunk_size_secs = chunk_size_secs
        self.vocab_size = vocab_size
        self.min_frequency = min_frequency
        self.special_tokens = list(special_tokens) if special_tokens is not None else []
        self.bos_token, self.eos_token, self.unk_token, self.pad_token = bos_token, eos_token, unk_token, pad_token
        self.max_token_codebook_ngrams = max_token_codebook_ngrams
        self.unicode_offset = validate_unicode_offset(unicode_offset, num_codebooks, codebook_size)
        self.device = device if isinstance(device, int) else int(str(device).split(":")[-1] or 0)
        for special_token in [self.eos_token, self.bos_token, self.unk_token, self.pad_token]:
            if special_token is not None and special_token not in self.special_tokens:
                self.special_tokens.insert(0, special_token)
        min_vocab_size = self.num_codebooks * self.codebook_size + len(self.special_tokens)
        if self.vocab_size < min_vocab_size:
            raise ValueError(
                f"vocab_size is set to {self.vocab_size} but it must be at least {min_vocab_size} to accommodate "
                f"{self.num_codebooks} x {self.codebook_size} codes and {len(self.special_tokens)} special token(s).\n"
                f"Consider setting vocab_size to {min_vocab_size} + K, where K is the number of tokens you want to "
                "reserve for codebook ngrams (learned merges). K should be a sufficiently large number (e.g. >= "
                "10,000) to allow for wide coverage of the most common codebook ngrams in your training data.")
        self._model = None
        self.last_stats: Dict[str, float] = {}
        # the last training's learned tokens (alphabet-index tuples) and merges (left id, right id), ids counted
        # from the special tokens: oracle/bpe_ref.train_bpe's convention
        self.last_tokens: List[Tuple[int, ...]] = []
        self.last_merges: List[Tuple[int, int]] = []

    # ---- corpus ----------------------------------------------------------------------------------
    def iterate_codepoints(self, codes_list: Iterable[np.ndarray]) -> Iterable[np.ndarray]:
        """``_iterate_and_convert`` (bpe_trainer.py:73-105): per utterance, shape handling, first
        num_codebooks rows, chunks of int(chunk_size_secs * codec_framerate) frames -> code points."""
        for codes in codes_list:
            if len(codes.shape) == 4:
                codes = codes[0, 0]
            elif len(codes.shape) == 3:
                codes = codes[0]
            codes = codes[:self.num_codebooks]
            chunk_size = int(self.chunk_size_secs * self.codec_framerate) if self.chunk_size_secs else codes.shape[1]
            for i in range(0, codes.shape[1], chunk_size):
                yield codes_to_codepoints(codes[:, i:i + chunk_size], self.codebook_size,
                                          copy_before_conversion=False, unicode_offset=self.unicode_offset)

    def words(self, codes_list: Iterable[np.ndarray]) -> Tuple[List[np.ndarray], np.ndarray]:
        """Distinct training words (alphabet indices) and their counts."""
        if self._model is None:
            self._model = CharModel(self.unicode_offset, self.num_codebooks * self.codebook_size)
        counts: Dict[bytes, int] = {}
        arrays: Dict[bytes, np.ndarray] = {}
        for cps in self.iterate_codepoints(codes_list):
            for w in self._model.words(cps):
                k = w.astype(np.int32).tobytes()
                if k in counts:
                    counts[k] += 1
                else:
                    counts[k] = 1
                    arrays[k] = w.astype(np.int32)
        keys = list(counts)
        return [arrays[k] for k in keys], np.array([counts[k] for k in keys], dtype=np.int64)

    # ---- training --------------------------------------------------------------------------------
    def _max_token_length(self) -> Optional[int]:
        if self.max_token_codebook_ngrams is None:
            return None
        return max(1, self.max_token_codebook_ngrams * self.num_codebooks)

    def train_codes(self, codes_list: Iterable[np.ndarray]):
        """Train on in-memory code arrays; returns the tokenizer (see ``train``)."""
        n_base = self.num_codebooks * self.codebook_size
        max_len = self._max_token_length()
        if max_len == 1:
            tokens, merges = [], []
        else:
            t0 = time.perf_counter()
            words, counts = self.words(codes_list)
            corpus_s = time.perf_counter() - t0
            # tokenizers treats max_token_length as exclusive: codec_bpe passes the limit + 1
            tokens, merges = train_words_gpu(words, counts, n_base, len(self.special_tokens), self.vocab_size,
                                             self.min_frequency, max_len + 1 if max_len is not None else None,
                                             self.device, self.last_stats)
            self.last_stats["corpus_s"] = corpus_s  # host: chunks -> code points -> words (NFKC model)
        self.last_tokens, self.last_merges = tokens, merges
        t0 = time.perf_counter()
        tok = self._assemble(tokens, merges)
        self.last_stats["assemble_s"] = time.perf_counter() - t0  # tokenizers / transformers objects
        return tok

    def train(self, codes_path: str, codes_filter: Optional[Union[str, List[str]]] = None,
              num_files: Optional[int] = None):
        """``Trainer.train`` (bpe_trainer.py:107-166): BPE over the code files under codes_path."""
        if self._max_token_length() == 1:
            return self._assemble([], [])
        codes_files = get_codes_files(codes_path, codes_filter, num_files)
        if not self.chunk_size_secs and codes_files[0].split("_")[-1].startswith("c"):
            warnings.warn(
                "The codes files do not have start timestamps, indicating they represent full-length encoded audio "
                "files rather than chunks. It is recommended to set `--chunk_size_secs` to a small value (e.g. 30) "
                "to avoid the tokenizer training on very long sequences. Training on very long sequences of audio "
                "codes can lead to memory issues and poor BPE merges.")
        return self.train_codes(u for f in codes_files for u in _utterances(f))

    # ---- output ----------------------------------------------------------------------------------
    def vocab_and_merges(self, tokens: Sequence[Tuple[int, ...]], merges: Sequence[Tuple[int, int]]):
        """token strings in id order and merges as string pairs (tokenizers' BPE model content)."""
        base = self.unicode_offset
        n_base = self.num_codebooks * self.codebook_size
        strs = list(self.special_tokens) + [chr(base + i) for i in range(n_base)]
        strs += ["".join(chr(base + i) for i in t) for t in tokens]
        merge_strs = [(strs[a], strs[b]) for a, b in merges]
        return strs, merge_strs

    def _assemble(self, tokens, merges):
        from tokenizers import Tokenizer, decoders, pre_tokenizers
        from tokenizers.models import BPE
        from tokenizers.normalizers import NFKC
        strs, merge_strs = self.vocab_and_merges(tokens, merges)
        vocab = {}
        for i, s in enumerate(strs):
            vocab.setdefault(s, i)
        tok = Tokenizer(BPE(vocab, merge_strs, unk_token=self.unk_token))
        if self.special_tokens:
            tok.add_special_tokens(list(self.special_tokens))
        tok.normalizer = NFKC()
        tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="never")
        tok.decoder = decoders.Metaspace(replacement="▁", prepend_scheme="never")
        try:
            from transformers import PreTrainedTokenizerFast
        except Exception:  # pragma: no cover - transformers absent: the tokenizers object
            return tok
        return PreTrainedTokenizerFast(tokenizer_object=tok, bos_token=self.bos_token, eos_token=self.eos_token,
                                       unk_token=self.unk_token, pad_token=self.pad_token,
                                       clean_up_tokenization_spaces=False,
                                       model_input_names=["input_ids", "attention_mask"])


def train_words_gpu(words: Sequence[np.ndarray], counts: np.ndarray, n_base: int, n_special: int, vocab_size: int,
                    min_frequency: int, max_token_length: Optional[int], device: int = 0,
                    stats: Optional[dict] = None, *, min_table_slots: Optional[int] = None,
                    grid_blocks: Optional[int] = None) -> Tuple[List[Tuple[int, ...]], List[Tuple[int, int]]]:
    """The merge loop on the GPU (``mimi_bpe_*``).  words: alphabet indices (0 .. n_base-1).  Returns
    (tokens beyond the alphabet as tuples of alphabet indices, merges as (left id, right id)) with ids counted
    from the special tokens, as ``oracle/bpe_ref.train_bpe``.  min_table_slots / grid_blocks: the options of
    ``mimi_bpe_create_opts`` (None: the defaults; a value it refuses raises ``ValueError`` before any device call);
    with a dict in ``stats`` the table's final ``table_slots`` and ``growth_rehashes`` are recorded too."""
    import time

    from . import _lib
    lib = _lib.load()
    lens = np.array([len(w) for w in words], dtype=np.int64)
    offs = np.zeros(len(words) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    sym = (np.concatenate(words).astype(np.int32) if len(words) else np.zeros(0, np.int32)) + np.int32(n_special)
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    if vocab_size > (1 << 17) - 1:
        raise ValueError("vocab_size above 131071 is not supported by the GPU trainer")
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    opts = _lib.BpeOptionsC(int(min_table_slots or 0), int(grid_blocks or 0), 0)
    if (min_table_slots is not None and min_table_slots < 1) or (grid_blocks is not None and grid_blocks < 1):
        raise ValueError("min_table_slots and grid_blocks must be >= 1 (None: the default)")
    try:
        _lib.check(lib.mimi_bpe_create_opts(device, sym.ctypes.data, sym.size, offs.ctypes.data, cnt.ctypes.data,
                                            len(words), n_special + n_base, vocab_size, max_token_length or 0,
                                            ctypes.byref(opts), ctypes.byref(h)))
    except _lib.MimiHipError as e:
        if e.status == 1:
            raise ValueError(str(e)) from None
        raise
    tokens: List[Tuple[int, ...]] = []
    merges: List[Tuple[int, int]] = []
    spell: List[Tuple[int, ...]] = [()] * n_special + [(i,) for i in range(n_base)]
    tok_id: Dict[Tuple[int, ...], int] = {t: i for i, t in enumerate(spell) if i >= n_special}
    a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    try:
        while len(spell) < vocab_size:
            _lib.check(lib.mimi_bpe_best(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
            if c.value < 1 or c.value < min_frequency:
                break
            new = spell[a.value] + spell[b.value]
            nid = tok_id.get(new)
            if nid is None:
                nid = len(spell)
                spell.append(new)
                tok_id[new] = nid
                tokens.append(new)
            merges.append((a.value, b.value))
            if stats is not None and "trace" in stats:
                stats["trace"].append(c.value)
            _lib.check(lib.mimi_bpe_merge(h, a.value, b.value, nid, len(new)))
        if stats is not None:
            v = ctypes.c_int64()
            for key in ("table_slots", "growth_rehashes"):
                _lib.check(lib.mimi_bpe_info(h, _lib.BPE_TRAIN_INFO[key], ctypes.byref(v)))
                stats[key] = v.value
    finally:
        lib.mimi_bpe_destroy(h)
    if stats is not None:
        stats.update({"seconds": time.perf_counter() - t0, "merges": len(merges), "symbols": int(sym.size),
                      "words": len(words)})
    return tokens, merges


def spelling_table(spellings: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """Per-id spellings (alphabet indices) -> (offsets int64 [n + 1], indices int32), the layout of
    ``mimi_bpe_model_set_spellings``."""
    lens = np.fromiter((len(t) for t in spellings), dtype=np.int64, count=len(spellings))
    off = np.zeros(len(spellings) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    idx = np.fromiter((i for t in spellings for i in t), dtype=np.int32, count=int(off[-1]))
    return off, idx


def filter_keep(cb: np.ndarray, num_codebooks: int, commuted: bool = False) -> np.ndarray:
    """The keep mask of ``Encoder.decode_ids``' step 2 for the codebooks ``cb`` of one sequence's characters, as a
    scan: character i is the map ``f_i(e) = (e + 1) % K if e == cb_i else e`` on ``[0, K)``, the first character the
    constant map to ``(cb_0 + 1) % K`` (``expected`` starts as ``cb_0``, so it is kept), ``expected`` before
    character i is ``(f_{i-1} o ... o f_0)`` of anything, and a character is kept iff it equals its codebook.  The
    inclusive scan doubles its reach per pass (log2 n passes of one fancy-index each).  The operator does not
    commute; ``commuted=True`` composes in the wrong order, which tests use to show that their streams tell the two
    apart."""
    K = int(num_codebooks)
    cb = np.asarray(cb, dtype=np.int64)
    n = cb.size
    if n == 0:
        return np.zeros(0, dtype=bool)
    maps = np.tile(np.arange(K, dtype=np.int64), (n, 1))
    maps[np.arange(n), cb] = (cb + 1) % K
    maps[0, :] = (cb[0] + 1) % K
    o = 1
    while o < n:
        earlier, later = maps[:-o], maps[o:]
        if commuted:
            earlier, later = later, earlier
        maps[o:] = np.take_along_axis(later, earlier, axis=1)  # later(earlier(e))
        o *= 2
    expected = np.empty(n, dtype=np.int64)
    expected[0] = cb[0]
    expected[1:] = maps[:-1, 0]
    return cb == expected


class Encoder:
    """Apply a trained codec-BPE model on the GPU: codes (or ``codes_to_chars`` strings) -> token ids.

    Replaces the tokenizer call of the reference's ``pretraining-data/estimate_tokens.py:75``
    (``tokenizer(text)["input_ids"]``) for code strings.  The result equals
    ``tok.encode(codes_to_chars(...), add_special_tokens=False).ids`` of the tokenizer ``Trainer`` assembles with
    ``unk_token=None`` (the recipe's setting: ``train_bpe_recipe.txt`` passes only ``--pad_token``).  In that
    model the characters NFKC rewrites and the Metaspace ``▁`` are not in the vocabulary and give no id, so
    ``CharModel`` (drop, split, mark reordering) is the whole host model; the merges run in ``bpe_encode.hip``
    (``mimi_bpe_encode``), one workgroup per word, all words of a call in one launch per kernel form.

    A model with an ``unk_token`` raises ``NotImplementedError`` at construction: there every dropped character
    would give the unknown id, which this host model does not produce.  Characters outside the
    ``num_codebooks x codebook_size`` code alphabet raise ``ValueError`` (``CharModel.words``).  ``encode_codes``
    / ``encode_strs`` / ``encode_words`` read host arrays and run ``CharModel`` on the host; ``encode_device``
    takes codes in device memory, runs the same word model in ``bpe_words.hip`` and leaves the ids on the device.
    Merging the vocabulary into a text tokenizer (the reference's ``extend_tokenizer`` step) is not part of this
    class.

    merges: ``(left id, right id, new id)`` in rank order; ids count the special tokens first, then the alphabet in
    code point order, then the learned tokens -- the trainer's convention.
    """

    LDS_MAX_SYMBOLS = 8192  # _lib.BPE_ENCODE_LDS_MAX_SYMBOLS: longer words run on a global workspace
    WORDS_MAX_RUN = 64  # _lib.BPE_WORDS_MAX_RUN: the longest run of marks the device word model orders

    def __init__(self, num_codebooks: int, codebook_size: int, merges, n_tokens: int, n_special: int,
                 unicode_offset: int = UNICODE_OFFSET, device: Union[int, str] = 0, unk_token: Optional[str] = None,
                 spellings: Optional[Sequence[Sequence[int]]] = None):
        from . import _lib
        if unk_token is not None:
            raise NotImplementedError("bpe.Encoder supports models without an unk_token only (the recipe's setting)")
        self.num_codebooks, self.codebook_size = num_codebooks, codebook_size
        self.unicode_offset = validate_unicode_offset(unicode_offset, num_codebooks, codebook_size)
        self.n_special, self.n_tokens = int(n_special), int(n_tokens)
        n_base = num_codebooks * codebook_size
        if self.n_special < 0 or self.n_tokens < self.n_special + n_base:
            raise ValueError(f"n_tokens {n_tokens} is below {n_special} special tokens + {n_base} code characters")
        if self.n_tokens > (1 << 17):
            raise ValueError("token ids above 131071 are not supported by the GPU encoder")
        self.merges = np.ascontiguousarray(np.asarray(merges, dtype=np.int64).reshape(-1, 3).astype(np.int32))
        if self.merges.size and (self.merges.min() < 0 or self.merges.max() >= self.n_tokens):
            raise ValueError("merge ids outside [0, n_tokens)")
        self.device = device if isinstance(device, int) else int(str(device).split(":")[-1] or 0)
        self._chars = CharModel(self.unicode_offset, n_base)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()  # the device model (merge table), made on first use
        self.last_stats: Dict[str, float] = {}
        # the decoder's spelling table (decode_ids / decode_device): given (from_trainer, from_tokenizer), or built
        # from the merges on first use
        self._spell: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._spell_on_device = False
        self._streams = weakref.WeakSet()  # open IdStreams: closed before the device model
        if spellings is not None:
            if len(spellings) != self.n_tokens:
                raise ValueError(f"{len(spellings)} spellings for {self.n_tokens} tokens")
            off, idx = spelling_table(spellings)
            if idx.size and (idx.min() < 0 or idx.max() >= n_base):
                raise ValueError("spelling indices outside the code alphabet")
            self._spell = (off, idx)

    def spellings(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(offsets int64 [n_tokens + 1], alphabet indices int32)``: id i spells ``indices[offsets[i]:offsets[i + 1]]``.
        A special id spells nothing, an alphabet id itself; without spellings given at construction a learned id
        spells ``spell[left] + spell[right]`` of its merge, taken in rank order (an id that no merge forms spells
        nothing, as ``tokenizers`` decodes an id that its vocabulary lacks)."""
        if self._spell is None:
            n_base = self.num_codebooks * self.codebook_size
            spell: List[Tuple[int, ...]] = [()] * self.n_special + [(i,) for i in range(n_base)]
            spell += [()] * (self.n_tokens - len(spell))
            for a, b, c in self.merges.tolist():
                if c >= self.n_special + n_base:
                    spell[c] = spell[a] + spell[b]
            self._spell = spelling_table(spell)
        return self._spell

    def _model(self):
        from . import _lib
        if not self._h:
            _lib.check(self._lib.mimi_bpe_model_create(self.device, self.merges.ctypes.data, len(self.merges),
                                                       self.n_tokens, ctypes.byref(self._h)))
            # the device word model's alphabet (encode_device): class and combining class of every code character
            cls, ccc = np.ascontiguousarray(self._chars.cls), np.ascontiguousarray(self._chars.ccc)
            _lib.check(self._lib.mimi_bpe_model_set_alphabet(self._h, self.n_special, self.num_codebooks,
                                                             self.codebook_size, cls.ctypes.data, ccc.ctypes.data))
        return self._h

    def _decode_model(self):
        from . import _lib
        h = self._model()
        if not self._spell_on_device:
            off, idx = self.spellings()
            _lib.check(self._lib.mimi_bpe_model_set_spellings(h, off.ctypes.data, idx.ctypes.data))
            self._spell_on_device = True
        return h

    def close(self) -> None:
        for st in list(getattr(self, "_streams", ())):
            st.close()
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.mimi_bpe_model_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._spell_on_device = False

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ---- construction ----------------------------------------------------------------------------
    @classmethod
    def from_trainer(cls, trainer: "Trainer") -> "Encoder":
        """The model of ``trainer``'s last training (``last_tokens`` / ``last_merges``); no ``tokenizers`` import."""
        n_sp, n_base = len(trainer.special_tokens), trainer.num_codebooks * trainer.codebook_size
        spell: List[Tuple[int, ...]] = [()] * n_sp + [(i,) for i in range(n_base)] + list(trainer.last_tokens)
        tok_id: Dict[Tuple[int, ...], int] = {}
        for i in range(n_sp, len(spell)):
            tok_id.setdefault(spell[i], i)
        merges = [(a, b, tok_id[spell[a] + spell[b]]) for a, b in trainer.last_merges]
        return cls(trainer.num_codebooks, trainer.codebook_size, merges, len(spell), n_sp,
                   unicode_offset=trainer.unicode_offset, device=trainer.device, unk_token=trainer.unk_token,
                   spellings=spell)

    @classmethod
    def from_tokenizer(cls, tokenizer, num_codebooks: int, codebook_size: int,
                       unicode_offset: int = UNICODE_OFFSET, device: Union[int, str] = 0) -> "Encoder":
        """From a ``tokenizers.Tokenizer``, a ``PreTrainedTokenizerFast`` or the path of a ``tokenizer.json``: the
        BPE model's vocab and merges are read from the JSON."""
        if isinstance(tokenizer, (str, os.PathLike)):
            with open(tokenizer, encoding="utf-8") as f:
                j = json.load(f)
        else:
            backend = getattr(tokenizer, "backend_tokenizer", tokenizer)
            j = json.loads(backend.to_str())
        model = j["model"]
        if model.get("type", "BPE") != "BPE":
            raise ValueError(f"not a BPE model: {model.get('type')}")
        if model.get("unk_token") is not None:
            raise NotImplementedError("bpe.Encoder supports models without an unk_token only (the recipe's setting)")
        for key in ("dropout", "continuing_subword_prefix", "end_of_word_suffix"):
            if model.get(key):
                raise NotImplementedError(f"BPE model option {key} is not supported")
        if model.get("byte_fallback") or model.get("ignore_merges"):
            raise NotImplementedError("byte_fallback / ignore_merges models are not supported")
        vocab = model["vocab"]
        n_base = num_codebooks * codebook_size
        validate_unicode_offset(unicode_offset, num_codebooks, codebook_size)
        n_sp = vocab.get(chr(unicode_offset))
        if n_sp is None or any(vocab.get(chr(unicode_offset + i)) != n_sp + i for i in range(n_base)):
            raise ValueError("the vocabulary does not hold the code characters in code point order after the "
                             "special tokens")
        n_tokens = max(max(vocab.values()), max((t["id"] for t in j.get("added_tokens", [])), default=0)) + 1
        merges = []
        for m in model["merges"]:
            a, b = m.split(" ") if isinstance(m, str) else m
            merges.append((vocab[a], vocab[b], vocab[a + b]))
        # what each id decodes to: an id at or above n_special must be a string of code characters (an id that the
        # vocabulary lacks decodes to nothing, in tokenizers too)
        spell: List[Tuple[int, ...]] = [()] * n_tokens
        entries = list(vocab.items()) + [(t["content"], t["id"]) for t in j.get("added_tokens", [])]
        for text, i in entries:
            if i < n_sp:
                continue
            t = tuple(ord(ch) - unicode_offset for ch in text)
            if not t or min(t) < 0 or max(t) >= n_base:
                raise NotImplementedError(f"token {i} ({text!r}) is not a string of code characters: decoding it to "
                                          f"codes is not defined")
            spell[i] = t
        return cls(num_codebooks, codebook_size, merges, n_tokens, n_sp, unicode_offset=unicode_offset,
                   device=device, spellings=spell)

    # ---- model properties --------------------------------------------------------------------------
    def info(self, key: str) -> int:
        """``mimi_bpe_model_info``: "pairs", "formed_pair_outranks", "table_slots", and of the last encode
        "last_words_lds_small", "last_words_lds", "last_words_global" (words run by each kernel form)."""
        from . import _lib
        v = ctypes.c_int64()
        _lib.check(self._lib.mimi_bpe_model_info(self._model(), _lib.BPE_INFO[key], ctypes.byref(v)))
        return v.value

    @property
    def formed_pair_outranks(self) -> bool:
        """Some merge forms a pair whose own merge has a lower rank (an id reused by a later merge): merging
        every occurrence of a round's pair at once would be wrong for this model."""
        return bool(self.info("formed_pair_outranks"))

    # ---- encoding ----------------------------------------------------------------------------------
    def _encode_flat(self, sym: np.ndarray, offs: np.ndarray, stream=None) -> Tuple[np.ndarray, np.ndarray]:
        """``mimi_bpe_encode``: (out_ids with word w's ids at offs[w], out_lens)."""
        from . import _lib
        n_words = len(offs) - 1
        out = np.empty(max(sym.size, 1), dtype=np.int32)
        out_lens = np.zeros(max(n_words, 1), dtype=np.int32)
        s = getattr(stream, "cuda_stream", stream)
        try:
            _lib.check(self._lib.mimi_bpe_encode(self._model(), sym.ctypes.data, offs.ctypes.data, n_words,
                                                 out.ctypes.data, out_lens.ctypes.data,
                                                 ctypes.c_void_p(int(s)) if s else None))
        except _lib.MimiHipError as e:
            if e.status == 1:
                raise ValueError(str(e)) from None
            raise
        return out, out_lens[:n_words]

    def encode_words(self, words: Sequence[np.ndarray], stream=None) -> List[np.ndarray]:
        """Words of symbol ids (special tokens first, then the alphabet) -> each word's token ids; one GPU call.
        stream: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` value (default: the default stream)."""
        lens = np.array([len(w) for w in words], dtype=np.int64)
        offs = np.zeros(len(words) + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        sym = np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.int32) for w in words])
                                   if len(words) else np.zeros(0, np.int32), dtype=np.int32)
        out, out_lens = self._encode_flat(sym, offs, stream)
        return [out[offs[w]:offs[w] + out_lens[w]].copy() for w in range(len(words))]

    def _encode_codepoints(self, seqs: Sequence[np.ndarray], stream=None) -> List[np.ndarray]:
        # (per sequence: one pass over all sequences' characters at once was measured slower, its arrays leave
        # the cache)
        t0 = time.perf_counter()
        words: List[np.ndarray] = []
        nwords = []
        for cps in seqs:
            ws = self._chars.words(cps)
            nwords.append(len(ws))
            words.extend(w.astype(np.int32) + np.int32(self.n_special) for w in ws)
        t1 = time.perf_counter()
        ids = self.encode_words(words, stream)
        out, at = [], 0
        for n in nwords:
            out.append(np.concatenate(ids[at:at + n]).astype(np.int32) if n else np.zeros(0, np.int32))
            at += n
        self.last_stats = {"host_words_s": t1 - t0, "encode_s": time.perf_counter() - t1, "words": len(words),
                           "symbols": int(sum(len(w) for w in words)), "tokens": int(sum(len(o) for o in out))}
        return out

    def encode_codes(self, codes_list: Iterable[np.ndarray], stream=None) -> List[np.ndarray]:
        """Each ``[K', T]`` code array (first ``num_codebooks`` rows; leading batch dimensions as
        ``Trainer.iterate_codepoints``) is one sequence -> its ``int32`` token ids."""
        seqs = []
        for codes in codes_list:
            if len(codes.shape) == 4:
                codes = codes[0, 0]
            elif len(codes.shape) == 3:
                codes = codes[0]
            # (a copy: the caller's codes stay as they are; the offsets are still added in the codes' own dtype)
            seqs.append(codes_to_codepoints(codes[:self.num_codebooks], self.codebook_size,
                                            unicode_offset=self.unicode_offset))
        return self._encode_codepoints(seqs, stream)

    def encode_strs(self, strings: Iterable[str], stream=None) -> List[np.ndarray]:
        """``codes_to_chars`` strings -> ``int32`` token ids, one array per string."""
        return self._encode_codepoints(
            [np.frombuffer(s.encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int64) for s in strings],
            stream)

    def encode_device(self, codes, lengths=None, chunk_frames: int = 0, stream=None, to_host: bool = False):
        """Codes in device memory -> token ids in device memory: the word model, the merges and the packing all run
        on the GPU (``mimi_bpe_encode_codes``), so ``MimiHipModel.encode(...).audio_codes`` can be passed as it is.

        codes: a CUDA ``torch.Tensor`` ``[B, K', T]`` or ``[K', T]``, int32 or int64 (int64 is narrowed by a torch
        op), ``K' >= num_codebooks`` (further rows are ignored).  lengths: frames of each item (default ``T``);
        frames beyond an item's length are never read.  chunk_frames > 0 cuts every item into sequences of that many
        frames, each a string of its own as ``Trainer.iterate_codepoints`` cuts them; 0: one sequence per item.  An
        item of length 0 gives one empty sequence.  stream: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` value
        (default: the current stream of the codes' device); the call synchronises it.

        Returns ``(ids, seq_offsets, seq_item)``: ``ids`` an int32 device tensor holding sequence s at
        ``ids[seq_offsets[s]:seq_offsets[s + 1]]``, ``seq_offsets`` a host int64 array of ``n_seq + 1`` entries,
        ``seq_item`` the item of each sequence (host int64 array).  With ``to_host=True``: a list of int32 numpy
        arrays, one per sequence.  ``last_stats["word_model"]`` is ``"device"``, or ``"host"`` when a run of more
        than ``WORDS_MAX_RUN`` marks made the call go through ``encode_codes`` on ``.cpu()`` codes instead (same
        result; the recipe's alphabet has runs of at most 5).

        Unlike ``encode_codes``, a code outside ``[0, codebook_size)`` is always a ``ValueError``: there the offset
        add can carry such a code into a neighbouring codebook's characters, here it is checked on the device
        before any table is read.  Argument errors raise ``ValueError`` before any device call."""
        import torch

        from . import _lib
        if not isinstance(codes, torch.Tensor):
            raise ValueError("codes must be a CUDA torch.Tensor (host arrays: encode_codes)")
        if codes.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"codes must be int32 or int64, not {codes.dtype}")
        if codes.dim() == 2:
            codes = codes[None]
        if codes.dim() != 3:
            raise ValueError("codes must have shape [B, K', T] or [K', T]")
        B, Kp, T = codes.shape
        if Kp < self.num_codebooks:
            raise ValueError(f"codes have {Kp} codebook rows, the model needs {self.num_codebooks}")
        chunk_frames = int(chunk_frames)
        if chunk_frames < 0:
            raise ValueError("chunk_frames must be >= 0")
        if lengths is None:
            lens = np.full(B, T, dtype=np.int64)
        else:
            if isinstance(lengths, torch.Tensor):
                lengths = lengths.cpu().numpy()
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
            if lens.size != B:
                raise ValueError(f"{lens.size} lengths for {B} items")
            if B and (lens.min() < 0 or lens.max() > T):
                raise ValueError(f"lengths must be in [0, {T}]")
        if not codes.is_cuda:
            raise ValueError("codes must be a CUDA torch.Tensor (host arrays: encode_codes)")
        if codes.device.index != self.device:
            raise ValueError(f"codes are on {codes.device}, the encoder on device {self.device}")
        if chunk_frames:
            per_item = np.maximum(1, -(-lens // chunk_frames))
        else:
            per_item = np.ones(B, dtype=np.int64)
        seq_item = np.repeat(np.arange(B, dtype=np.int64), per_item)
        n_seq = int(seq_item.size)
        seq_offsets = np.zeros(n_seq + 1, dtype=np.int64)
        capacity = self.num_codebooks * int(lens.sum())
        t0 = time.perf_counter()
        with torch.cuda.device(codes.device):
            if codes.dtype != torch.int32:
                codes = codes.to(torch.int32)
            if T and codes.stride(2) != 1:
                codes = codes.contiguous()
            ids = torch.empty(max(capacity, 1), dtype=torch.int32, device=codes.device)
            if stream is None:
                stream = torch.cuda.current_stream(codes.device)
            s = getattr(stream, "cuda_stream", stream)
            current = torch.cuda.current_stream(codes.device)
            if int(s or 0) != current.cuda_stream:
                current.synchronize()  # the narrowing / copy above ran there
            model_mode = "device"
            if n_seq:
                try:
                    _lib.check(self._lib.mimi_bpe_encode_codes(
                        self._model(), ctypes.c_void_p(codes.data_ptr()), B, codes.stride(0), codes.stride(1),
                        lens.ctypes.data, chunk_frames, ctypes.c_void_p(ids.data_ptr()), capacity,
                        seq_offsets.ctypes.data, n_seq, ctypes.c_void_p(int(s)) if s else None))
                except _lib.MimiHipError as e:
                    if e.status == 1:
                        raise ValueError(str(e)) from None
                    if e.status != 5 or "MIMI_BPE_WORDS_MAX_RUN" not in str(e):
                        raise
                    # a run of marks above the device cap: the host word model on the same chunks
                    model_mode = "host"
                    host = codes[:, :self.num_codebooks].cpu().numpy()
                    chunks = []
                    for b in range(B):
                        Tb = int(lens[b])
                        step = chunk_frames or max(Tb, 1)
                        chunks += [host[b][:, f:min(f + step, Tb)] for f in range(0, max(Tb, 1), step)]
                    out = self.encode_codes(chunks)
                    np.cumsum([len(o) for o in out], out=seq_offsets[1:])
                    flat = np.concatenate(out) if out else np.zeros(0, np.int32)
                    ids[:flat.size].copy_(torch.from_numpy(flat))
            ids = ids[:int(seq_offsets[-1])]
        stats = {"word_model": model_mode, "device_call_s": time.perf_counter() - t0, "sequences": n_seq,
                 "tokens": int(seq_offsets[-1])}
        if model_mode == "host":
            self.last_stats.update(stats)
        else:
            stats.update(words=sum(self.info(k) for k in ("last_words_lds_small", "last_words_lds",
                                                          "last_words_global")) if n_seq else 0)
            self.last_stats = stats
        if to_host:
            flat = ids.cpu().numpy()
            return [flat[seq_offsets[i]:seq_offsets[i + 1]].copy() for i in range(n_seq)]
        return ids, seq_offsets, seq_item

    # ---- decoding ----------------------------------------------------------------------------------
    def _decode_one(self, ids: np.ndarray) -> np.ndarray:
        K, cbs = self.num_codebooks, self.codebook_size
        ids = np.asarray(ids).reshape(-1).astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= self.n_tokens):
            raise ValueError(f"a token id is outside [0, {self.n_tokens})")
        off, idx = self.spellings()
        # 1. expand: the spellings, concatenated
        first, lens = off[ids], off[ids + 1] - off[ids]
        total = int(lens.sum())
        if total == 0:
            return np.zeros((K, 0), dtype=np.int64)
        at = np.arange(total, dtype=np.int64) + np.repeat(first - (np.cumsum(lens) - lens), lens)
        return self.indices_to_codes(idx[at])

    def indices_to_codes(self, index: np.ndarray) -> np.ndarray:
        """Steps 2-4 of ``decode_ids`` on one sequence's alphabet indices (code point - ``unicode_offset`` of each
        character of a decoded string): the reference's drop rules, then the frames ``[num_codebooks, T]``."""
        K, cbs = self.num_codebooks, self.codebook_size
        index = np.asarray(index).reshape(-1).astype(np.int64)
        total = index.size
        if total == 0:
            return np.zeros((K, 0), dtype=np.int64)
        if index.min() < 0 or index.max() >= K * cbs:
            raise ValueError("characters outside the code alphabet")
        # 2. drop inconsistent (a stream that already cycles keeps everything)
        cb = index // cbs
        cb0 = int(cb[0])
        if not np.array_equal(cb, (cb0 + np.arange(total)) % K):
            index = index[filter_keep(cb, K)]
        # 3. drop hanging: the kept characters cycle from cb_0
        kept = index.size
        begin = min((K - cb0) % K, kept)
        T = (kept - begin) // K
        # 4. frames
        frames = index[begin:begin + K * T].reshape(T, K)
        return np.ascontiguousarray((frames - np.arange(K, dtype=np.int64) * cbs).T)

    def decode_ids(self, seqs: Iterable[np.ndarray]) -> List[np.ndarray]:
        """Token ids -> codes on the host, one int64 ``[num_codebooks, T]`` array per id sequence: what
        ``tokenizers``' ``decode(ids, skip_special_tokens=True)`` followed by the reference's
        ``pretraining-data/converter.py`` ``chars_to_codes`` (default flags) gives, and the statement of what
        ``decode_device`` computes.  Per sequence:

        1. the ids' spellings (``spellings()``) are concatenated; special ids give nothing; an id outside
           ``[0, n_tokens)`` is a ``ValueError``;
        2. character i has codebook ``cb_i = index_i // codebook_size``; ``expected`` starts as ``cb_0``; a character
           is kept iff ``cb_i == expected``; a kept one advances ``expected`` to ``(expected + 1) % K``
           (``filter_keep``);
        3. of the kept characters the first ``min((K - cb_0) % K, kept)`` are dropped, then the last
           ``remaining % K``;
        4. the ``T = remaining // K`` frames give ``codes[k][t] = index - k * codebook_size``.  A sequence that spells
           nothing gives ``T = 0`` (the reference raises ``IndexError`` on an empty string)."""
        return [self._decode_one(ids) for ids in seqs]

    def decode_device(self, ids, seq_offsets=None, stream=None, to_host: bool = False, lengths=None, out=None):
        """Token ids in device memory -> codes in device memory (``mimi_bpe_decode_plan`` / ``_write``): the rules of
        ``decode_ids`` on the GPU, the codes laid out as ``MimiHipModel.decode_ragged`` takes them.

        ids: a CUDA ``torch.Tensor``, int32 or int64 (int64 is narrowed by a torch op), either 1-D with
        ``seq_offsets`` (host, ``n_seq + 1`` entries from 0: sequence s is ``ids[seq_offsets[s]:seq_offsets[s + 1]]``;
        default: one sequence of all ids) -- what ``encode_device`` returns, as it stands -- or 2-D ``[B, L]`` with
        ``lengths`` (ids of each row, default ``L``; ids past a row's length are never decoded, whatever they are).
        stream: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` value (default: the current stream of the ids'
        device); the call synchronises it.  out: an int32 CUDA tensor ``[n_seq, K, >= Tmax]`` with unit stride along
        frames to write into instead of a new one; only the frames of each sequence are written.

        Returns ``(codes, frame_lengths)``: ``codes`` int32 ``[n_seq, K, Tmax]`` on the device (rows past a
        sequence's frames are zero in a tensor made here), ``frame_lengths`` a host int64 array.  With
        ``to_host=True``: a list of ``[K, T]`` int64 numpy arrays, equal to ``decode_ids``'.  ``last_stats["filter"]``
        is ``"device"``, or ``"host"`` when the library answered ``MIMI_ERR_UNSUPPORTED`` (more than 16 codebooks, 2^31
        characters) and the call went through ``decode_ids`` on ``.cpu()`` ids instead: same result.  An id outside
        ``[0, n_tokens)`` inside a sequence is a ``ValueError`` (checked on the device before any table is read).
        Argument errors raise ``ValueError`` before any device call."""
        import torch

        from . import _lib
        K = self.num_codebooks
        if not isinstance(ids, torch.Tensor):
            raise ValueError("ids must be a CUDA torch.Tensor (host arrays: decode_ids)")
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"ids must be int32 or int64, not {ids.dtype}")
        if ids.dim() == 1:
            if lengths is not None:
                raise ValueError("lengths go with 2-D ids; 1-D ids take seq_offsets")
            if seq_offsets is None:
                offs = np.array([0, ids.numel()], dtype=np.int64)
            else:
                if isinstance(seq_offsets, torch.Tensor):
                    seq_offsets = seq_offsets.cpu().numpy()
                offs = np.ascontiguousarray(np.asarray(seq_offsets, dtype=np.int64).reshape(-1))
                if offs.size < 1 or offs[0] != 0 or (np.diff(offs) < 0).any() or offs[-1] > ids.numel():
                    raise ValueError("seq_offsets must start at 0, not decrease and end inside ids")
            row_lens = None
        elif ids.dim() == 2:
            if seq_offsets is not None:
                raise ValueError("seq_offsets go with 1-D ids; 2-D ids take lengths")
            B, L = ids.shape
            if lengths is None:
                row_lens = np.full(B, L, dtype=np.int64)
            else:
                if isinstance(lengths, torch.Tensor):
                    lengths = lengths.cpu().numpy()
                row_lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
                if row_lens.size != B:
                    raise ValueError(f"{row_lens.size} lengths for {B} rows")
                if B and (row_lens.min() < 0 or row_lens.max() > L):
                    raise ValueError(f"lengths must be in [0, {L}]")
            offs = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(row_lens, out=offs[1:])
        else:
            raise ValueError("ids must have shape [n] or [B, L]")
        n_seq = int(offs.size - 1)
        if not ids.is_cuda:
            raise ValueError("ids must be a CUDA torch.Tensor (host arrays: decode_ids)")
        if ids.device.index != self.device:
            raise ValueError(f"ids are on {ids.device}, the encoder on device {self.device}")
        if out is not None:
            if (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 3 or not out.is_cuda
                    or out.device != ids.device or out.shape[0] < n_seq or out.shape[1] < K
                    or (out.shape[2] > 1 and out.stride(2) != 1)):
                raise ValueError(f"out must be an int32 CUDA tensor [>= {n_seq}, >= {K}, T] with unit frame stride")
        frames = np.zeros(n_seq, dtype=np.int64)
        t0 = time.perf_counter()
        with torch.cuda.device(ids.device):
            if row_lens is not None:  # the rows' ids end to end
                if (row_lens == ids.shape[1]).all():
                    ids = ids.reshape(-1)
                else:
                    keep = torch.arange(ids.shape[1], device=ids.device)[None, :] < \
                        torch.from_numpy(row_lens).to(ids.device)[:, None]
                    ids = ids[keep]
            if ids.dtype != torch.int32:  # (an id beyond int32 stays outside [0, n_tokens))
                ids = ids.clamp(-1, 0x7fffffff).to(torch.int32)
            if not ids.is_contiguous():
                ids = ids.contiguous()
            if stream is None:
                stream = torch.cuda.current_stream(ids.device)
            s = getattr(stream, "cuda_stream", stream)
            sp = ctypes.c_void_p(int(s)) if s else None
            current = torch.cuda.current_stream(ids.device)
            if int(s or 0) != current.cuda_stream:
                current.synchronize()  # the narrowing / copy above ran there
            mode = "device"
            host: Optional[List[np.ndarray]] = None
            if n_seq:
                try:
                    _lib.check(self._lib.mimi_bpe_decode_plan(self._decode_model(), ctypes.c_void_p(ids.data_ptr()),
                                                              offs.ctypes.data, n_seq, frames.ctypes.data, sp))
                except _lib.MimiHipError as e:
                    if e.status == 1:
                        raise ValueError(str(e)) from None
                    if e.status != 5:
                        raise
                    mode = "host"
                    flat = ids.cpu().numpy()
                    host = self.decode_ids([flat[offs[i]:offs[i + 1]] for i in range(n_seq)])
                    frames = np.array([c.shape[1] for c in host], dtype=np.int64)
            t_max = int(frames.max()) if n_seq else 0
            if out is None:
                codes = torch.zeros((n_seq, K, t_max), dtype=torch.int32, device=ids.device)
                if int(s or 0) != current.cuda_stream:
                    current.synchronize()  # the fill ran there
            else:
                if out.shape[2] < t_max:
                    raise ValueError(f"out holds {out.shape[2]} frames per row, the longest sequence has {t_max}")
                codes = out
            if n_seq and t_max:
                if host is None:
                    try:
                        _lib.check(self._lib.mimi_bpe_decode_write(self._decode_model(),
                                                                   ctypes.c_void_p(codes.data_ptr()), codes.stride(0),
                                                                   codes.stride(1), codes.shape[2], sp))
                    except _lib.MimiHipError as e:
                        if e.status == 1:
                            raise ValueError(str(e)) from None
                        raise
                else:
                    for i, c in enumerate(host):
                        codes[i, :K, :c.shape[1]].copy_(torch.from_numpy(c.astype(np.int32)))
            if out is not None:
                codes = out[:n_seq, :K, :t_max]
        self.last_stats = {"filter": mode, "device_call_s": time.perf_counter() - t0, "sequences": n_seq,
                           "ids": int(offs[-1]), "frames": int(frames.sum())}
        if to_host:
            if host is not None:
                return host
            h = codes.cpu().numpy().astype(np.int64)
            return [np.ascontiguousarray(h[i, :, :int(frames[i])]) for i in range(n_seq)]
        return codes, frames

    def decode_stream(self, slots: int, max_step_ids: int) -> "IdStream":
        """An ``IdStream`` of ``slots`` sessions whose steps bring at most ``max_step_ids`` ids per slot: token ids ->
        codes chunk by chunk, the filter state of every session in device memory.  ``NotImplementedError`` for more
        than 16 codebooks (the device filter's state map is 16 nibbles; ``decode_ids`` has no such limit)."""
        return IdStream(self, slots, max_step_ids)


class IdStream:
    """Streaming ``Encoder.decode_device`` (``Encoder.decode_stream``; ``mimi_bpe_decode_stream_*``,
    ``bpe_decode_stream.hip``): ``slots`` sessions, each with its own filter state in device memory.  ``step`` takes a
    few new token ids for any subset of the slots and returns the whole frames those ids complete, laid out as
    ``DecodeStream.step(codes, slots=, frames=)`` takes them.  ``decode_ids``' rules are causal, so after any sequence
    of steps the frames a slot has emitted, end to end, equal ``decode_ids([every id it was fed since its reset])[0]``
    -- whatever the split into steps and whatever the other slots were fed; the partial last frame stays pending
    (``pending``) until later ids complete it, and ``reset(slot)``, which is also how a session ends, discards it.
    One kernel launch and one synchronisation per step.  A context manager; ``close()`` frees the state (closing the
    encoder closes its streams).  The other direction, codes -> ids chunk by chunk, is not provided: BPE merges are
    not prefix-stable."""

    def __init__(self, encoder: "Encoder", slots: int, max_step_ids: int):
        self._enc, self.slots, self.max_step_ids = encoder, int(slots), int(max_step_ids)
        self.num_codebooks = encoder.num_codebooks
        self._h = None
        if self.slots < 1 or self.max_step_ids < 1:
            raise ValueError(f"a stream has at least 1 slot and takes at least 1 id per step, got {slots}, {max_step_ids}")
        if self.num_codebooks > 16:
            raise NotImplementedError(f"{self.num_codebooks} codebooks: the device filter packs at most 16 "
                                      f"(decode_ids has no such limit)")
        h = ctypes.c_void_p()
        self._call("create", encoder._decode_model(), self.slots, self.max_step_ids, ctypes.byref(h))
        self._h = h
        encoder._streams.add(self)

    def _call(self, name: str, *args):
        """``mimi_bpe_decode_stream_<name>(*args)``; an invalid argument (status 1) is a ``ValueError``."""
        from . import _lib
        try:
            _lib.check(getattr(self._enc._lib, f"mimi_bpe_decode_stream_{name}")(*args))
        except _lib.MimiHipError as err:
            if err.status == 1:
                raise ValueError(str(err)) from None
            raise

    def _handle(self):
        if self._h is None:
            raise RuntimeError("this IdStream is closed")
        return self._h

    def max_frames(self, ids: int) -> int:
        """The most frames an item that brings ``ids`` ids can complete: ``(K - 1 + ids * Lmax) // K``, ``Lmax`` the
        longest spelling."""
        if ids < 0:
            raise ValueError(f"ids must be at least 0, got {ids}")
        return int(self._enc._lib.mimi_bpe_decode_stream_max_frames(self._handle(), int(ids)))

    @property
    def pending(self) -> List[int]:
        """Per slot: the codes waiting in its partial frame, ``0 .. K - 1``, or ``-1`` for a fresh slot (no character
        since its reset)."""
        h = self._handle()
        return [int(self._enc._lib.mimi_bpe_decode_stream_slot_pending(h, b)) for b in range(self.slots)]

    def reset(self, slot: Optional[int] = None):
        """All slots, or only ``slot``, back to fresh: the pending partial frame is discarded and what follows equals
        a new stream (``ValueError`` for a slot outside ``[0, slots)``)."""
        if slot is None:
            self._call("reset", self._handle())
        else:
            self._call("reset_slot", self._handle(), int(slot))

    def step(self, ids, slots: Optional[Sequence[int]] = None, counts: Optional[Sequence[int]] = None, out=None):
        """New ids: a CUDA int32 / int64 tensor ``[m, L]``, padded; item ``i`` is slot ``slots[i]`` (``m`` distinct
        ints in ``[0, slots)``, any order; default: slots ``0 .. slots - 1``) and brings ``counts[i]`` ids, ``0 ..
        min(L, max_step_ids)`` (default ``L``); ids past an item's count are never read.  Returns ``(codes, frames)``:
        ``frames`` a host list, the whole frames each item completed, ``codes`` int32 ``[m, K, max(frames)]`` on the
        device (``max(frames)`` may be 0), item ``i``'s frames in ``codes[i, :, :frames[i]]`` -- zero past them in a
        tensor made here; with ``out`` (contiguous int32 CUDA ``[m, K, >= max_frames(max(counts))]``) ``codes`` is a
        view of it and nothing past an item's frames is written.  Runs on the current stream and synchronises it.
        Argument errors raise ``ValueError`` before any device call, the state untouched.  An id outside ``[0,
        n_tokens)`` is a ``ValueError`` too (checked on the device); the slots of that call then refuse until
        ``reset``."""
        import torch
        h = self._handle()
        K = self.num_codebooks
        if not isinstance(ids, torch.Tensor) or not ids.is_cuda:
            raise ValueError("ids must be a CUDA torch.Tensor")
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"ids must be int32 or int64, not {ids.dtype}")
        if ids.device.index != self._enc.device:
            raise ValueError(f"ids are on {ids.device}, the encoder on device {self._enc.device}")
        if slots is None:
            slots = list(range(self.slots))
        else:
            slots = [int(x) for x in slots]
            if not 1 <= len(slots) <= self.slots:
                raise ValueError(f"a step lists 1 .. {self.slots} slots, got {len(slots)}")
            if min(slots) < 0 or max(slots) >= self.slots or len(set(slots)) != len(slots):
                raise ValueError(f"slots must be distinct and in [0, {self.slots}), got {slots}")
        m = len(slots)
        if ids.dim() != 2 or ids.shape[0] != m:
            raise ValueError(f"ids must be [{m}, L], got {tuple(ids.shape)}")
        L = int(ids.shape[1])
        top = min(L, self.max_step_ids)
        if counts is None:
            counts = [L] * m
        else:
            counts = [int(x) for x in (counts.tolist() if hasattr(counts, "tolist") else counts)]
        if len(counts) != m or min(counts) < 0 or max(counts) > top:
            raise ValueError(f"counts must be {m} counts in [0, {top}], got {counts}")
        cap = self.max_frames(max(counts))
        if out is not None:
            if (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 3
                    or out.device != ids.device or out.shape[0] != m or out.shape[1] != K or out.shape[2] < cap
                    or not out.is_contiguous()):
                raise ValueError(f"out must be a contiguous int32 [{m}, {K}, >= {cap}] tensor on {ids.device}")
        with torch.cuda.device(ids.device):
            if ids.dtype != torch.int32:  # (an id beyond int32 stays outside [0, n_tokens))
                ids = ids.clamp(-1, 0x7fffffff).to(torch.int32)
            if not ids.is_contiguous():
                ids = ids.contiguous()
            codes = torch.zeros((m, K, cap), dtype=torch.int32, device=ids.device) if out is None else out
            i32 = ctypes.c_int32 * m
            frames = i32()
            s = torch.cuda.current_stream(ids.device).cuda_stream
            self._call("step", h, i32(*slots), i32(*counts), m, ctypes.c_void_p(ids.data_ptr()) if L else None,
                       L, ctypes.c_void_p(codes.data_ptr()) if codes.shape[2] else None,
                       codes.shape[2], frames, ctypes.c_void_p(int(s)) if s else None)
        frames = list(frames)
        return codes[:, :, :max(frames)], frames

    def close(self):
        h, self._h = self._h, None
        if h is not None and self._enc._h:
            self._enc._lib.mimi_bpe_decode_stream_destroy(h)
        self._enc._streams.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
