"""The models that audit the codec-BPE trainer (``tests/bpe_train_ref.py``), checked without a GPU:

* the reference (rewrite + recount) gives the merges of ``oracle.bpe_ref.train_bpe`` and of live ``tokenizers`` on
  every audit corpus, and the oracle's positive counts equal the recount at every step;
* the fault-free emulation of ``bpe.hip`` equals the reference in full state (words, positive pairs, winner) at every
  step of every corpus and forced schedule, at every table / grid setting the GPU test uses;
* every fault of ``FAULTS`` that can change a result is caught by a corpus, by state no later than by the merge list;
  the table printed here says at which step, and which faults the corpora of ``tests/test_bpe.py`` let through;
* the argument checks of ``mimi_bpe_create`` / ``mimi_bpe_create_opts`` that return before any device call.
"""
import ctypes

import numpy as np
import pytest

import bpe_train_ref as R
from oracle.bpe_ref import train_bpe

CORPORA = {c["name"]: c for c in R.all_corpora()}
_REF = {}


def reference(c, forced=()):
    key = (c["name"], tuple(forced))
    if key not in _REF:
        _REF[key] = R.trajectory(R.Reference(c["words"], c["counts"], c["maxlen"]), c, forced)
    return _REF[key]


@pytest.mark.parametrize("name", list(CORPORA))
def test_reference_matches_oracle_counts_and_merges(name):
    c = CORPORA[name]
    ref = reference(c)
    trace = []
    _, merges = train_bpe(c["words"], c["counts"], c["n_initial"] - 1, 1, c["vocab_size"], c["min_frequency"],
                          c["maxlen"] or None, pairs_trace=trace)
    assert merges == R.merges_of(ref)
    states = [s[1] for k, _, s in ref if k != "best"]  # after 0, 1, 2, ... merges
    assert len(trace) == len(states)
    for step, (got, want) in enumerate(zip(trace, states)):
        assert got == want, (name, step)


@pytest.mark.parametrize("name", list(CORPORA))
def test_reference_matches_live_tokenizers(name):
    pytest.importorskip("tokenizers")
    import json

    from tokenizers import Tokenizer, pre_tokenizers, trainers
    from tokenizers.models import BPE
    c = CORPORA[name]
    n_base = c["n_initial"] - 1
    ch = lambda i: chr(0xE000 + i - 1)  # noqa: E731  (id 0 is the special token)
    seqs = [s for w, k in zip(c["words"], c["counts"]) for s in ["".join(map(ch, w))] * k if w]
    tok = Tokenizer(BPE(unk_token=None))
    tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="never")
    tok.train_from_iterator(seqs, trainer=trainers.BpeTrainer(
        vocab_size=c["vocab_size"], min_frequency=c["min_frequency"], special_tokens=["<pad>"],
        limit_alphabet=n_base, initial_alphabet=[ch(i) for i in range(1, n_base + 1)],
        max_token_length=c["maxlen"] or None, show_progress=False))
    got = [tuple(m) for m in json.loads(tok.to_str())["model"]["merges"]]
    spell = {}
    want = []
    for kind, p, _ in reference(c):
        if kind == "merge":
            a, b, nid, _ = p
            sa, sb = spell.get(a) or ch(a), spell.get(b) or ch(b)
            spell.setdefault(nid, sa + sb)
            want.append((sa, sb))
    assert got == want


SETTINGS = [{}, {"small": True}, {"small": True, "grid_blocks": 1}, {"small": True, "grid_blocks": 3}]


def emulation(c, setting=None, faults=()):
    kw = dict(setting or {})
    if kw.pop("small", False):
        kw["min_table_slots"] = R.small_table(c["vocab_size"])
    return R.Emulation(c["words"], c["counts"], c["maxlen"], faults=faults, **kw)


@pytest.mark.parametrize("name", list(CORPORA))
def test_emulation_equals_reference_in_full_state(name):
    c = CORPORA[name]
    for setting in SETTINGS if name not in ("growth", "runs") else SETTINGS[:2]:
        assert R.first_difference(reference(c), R.trajectory(emulation(c, setting), c)) == (None, None), setting


@pytest.mark.parametrize("name", list(R.forced_schedules()))
def test_emulation_equals_reference_on_forced_schedules(name):
    c, f = R.forced_corpus(), R.forced_schedules()[name]
    ref = reference(c, f)
    assert len(R.merges_of(ref)) >= len(f) + 5  # training resumes after the forced merges
    for setting in SETTINGS:
        assert R.first_difference(ref, R.trajectory(emulation(c, setting), c, f)) == (None, None)
    if name in ("existing_id", "aa_existing_id"):  # the reused id does occur before the merge that reuses it
        w = R.Reference(c["words"], c["counts"], c["maxlen"])
        w.merge(*f[0])
        assert any(5 in x for x in w.words()) and f[1][:2] in w.pairs()


def test_growth_prediction():
    c = CORPORA["growth"]
    e = emulation(c, {"small": True})
    keys0 = len(e.pairs())
    for _ in R.drive(e, c):
        pass
    assert (R.small_table(c["vocab_size"]), keys0, e.rehashes) == (1024, 64, 3) and len(e.pairs()) > 4000
    d = emulation(c)
    for _ in R.drive(d, c):
        pass
    assert (d.slots, d.rehashes) == (1 << 21, 0)  # the default table never grows here: what the old tests ran


# fault -> {corpus: (first state step, first merge-list step)}; step s = the state after s merges, None = never.
# Seeded corpora and integer arithmetic: the figures are exact.  "table" entries are caught by the predicted
# (table_slots, growth_rehashes) alone.
EXPECTED = {
    "parity_dropped": {"runs": (1, 2), "overlap": (2, 3)},
    "parity_from_right": {"runs": (1, 10), "overlap": (2, 3)},
    "flagR_dropped": {"overlap": (1, 1), "strided": (1, None)},
    "lpartner_ignored": {"overlap": (1, 1), "strided": (1, None)},
    "le_maxlen": {"lengths3": (1, 5), "lengths9": (22, None)},
    "pair_not_zeroed": {"ties": (1, 1), "one_pair": (1, 1)},
    "ties_largest": {"ties": (0, 0), "highid": (2, 2)},
    "ties_left_only": {"ties": (0, 0)},
    "id16": {"highid": (0, 0), "ties": (None, None), "strided": (None, None)},
    "rebuild_gt1": {"highid": (0, None), "growth": (27, None)},
    "rebuild_keeps_nkeys": {"growth": "table", "strided": "table"},
    "single_pass": {"strided": (0, 0), "lengths2": (0, 1)},
    "prv_not_relinked": {"overlap": (1, 2), "lengths2": (1, None)},
    "len_not_written": {"lengths4": (2, 13), "lengths9": (22, None)},
}


def run_fault(c, fault, setting):
    ref = reference(c)
    e = emulation(c, setting, [fault])
    traj = R.trajectory(e, c, max_merges=len(R.merges_of(ref)) + 2)
    g = emulation(c, setting)
    for _ in R.drive(g, c):
        pass
    return R.first_difference(ref, traj), (e.slots, e.rehashes), (g.slots, g.rehashes)


def test_every_fault_is_caught_by_state():
    lines = []
    for fault, where in EXPECTED.items():
        num = R.FAULTS[fault][0]
        caught = False
        for name, want in where.items():
            setting = {"small": True, "grid_blocks": 1} if fault == "single_pass" else {"small": True}
            diff, table, table_ok = run_fault(CORPORA[name], fault, setting)
            lines.append(f"{num:2d} {fault:20s} {name:9s} state {diff[0]!s:5s} merges {diff[1]!s:5s} "
                         f"table {table} (fault-free {table_ok})")
            if want == "table":
                assert diff == (None, None) and table != table_ok, (fault, name, diff, table)
                caught = True
                continue
            assert diff == want, (fault, name, diff)
            state, merge = diff
            if state is not None:
                caught = True
                # the argument for the state audit: never later than the merge list, often the only witness
                assert merge is None or state <= merge
        assert caught, fault
    print("\nfault, corpus, first step the state / the merge list differs, (table_slots, growth_rehashes)")
    print("\n".join(lines))
    # strictly earlier, or state only, for at least one corpus of every fault that is not a tie rule
    for fault, where in EXPECTED.items():
        if fault in ("ties_largest", "ties_left_only", "id16", "rebuild_keeps_nkeys", "pair_not_zeroed"):
            continue
        assert any(w[0] is not None and (w[1] is None or w[0] < w[1]) for w in where.values()), fault
    assert set(EXPECTED) == set(R.FAULTS) - {"no_11_exemption"}


def test_the_11_exemption_is_dead_code_in_the_kernels():
    """Fault 6 changes nothing, anywhere: delta_kernel only tests pairs that hold the new id, whose length
    mimi_bpe_merge requires to be >= 2, so `lx == 1 && ly == 1` is never true there (the initial pairs, all of length
    1 + 1, are counted by count_pairs_kernel without the test).  No corpus can catch it; this pins that finding."""
    for name in ("lengths2", "lengths3", "lengths4", "lengths5", "lengths9"):
        c = CORPORA[name]
        assert R.first_difference(reference(c), R.trajectory(emulation(c, None, ["no_11_exemption"]), c)) == (None, None)
    c = R.forced_corpus()
    for f in R.forced_schedules().values():
        assert R.first_difference(reference(c, f), R.trajectory(emulation(c, None, ["no_11_exemption"]), c, f)) \
            == (None, None)


# ---- the corpora of tests/test_bpe.py: which faults its merge-list comparison lets through -----------------------
def old_random_corpora():
    """The corpora of test_gpu_trainer_matches_oracle_on_random_corpora (seed 11) and
    test_gpu_trainer_counts_beyond_2_30 (seed 12), generated as there."""
    out = []
    rng = np.random.default_rng(11)
    for case in range(12):
        nalpha = int(rng.integers(2, 12))
        words = [rng.integers(0, max(1, int(rng.integers(1, nalpha + 1))), size=int(rng.integers(0, 60))).astype(np.int32)
                 for _ in range(int(rng.integers(1, 50)))]
        counts = rng.integers(1, 4, size=len(words))
        ml = [None, 2, 3, 5, 9][case % 5]
        vs = 1 + nalpha + int(rng.integers(0, 80))
        out.append({"name": f"seed11_{case}", "words": [(w + 1).tolist() for w in words], "counts": counts.tolist(),
                    "n_initial": 1 + nalpha, "vocab_size": vs, "min_frequency": 1 + case % 3, "maxlen": ml or 0})
    rng = np.random.default_rng(12)
    for case in range(4):
        words = [rng.integers(0, 6, size=int(rng.integers(2, 20))).astype(np.int32) for _ in range(12)]
        counts = rng.integers((1 << 31) - 1000, (1 << 31) - 1, size=len(words))
        counts[case] = 3
        out.append({"name": f"seed12_{case}", "words": [(w + 1).tolist() for w in words], "counts": counts.tolist(),
                    "n_initial": 7, "vocab_size": 37, "min_frequency": 2, "maxlen": 0})
    return out


def fixture_corpora():
    from test_bpe import fixture, trainer_for
    meta, utts, arrays = fixture()
    out = []
    for case in ("recipe", "unlimited"):
        tr = trainer_for(meta, case)
        words, counts = tr.words([u.copy() for u in utts])
        n_sp, ml = len(tr.special_tokens), tr._max_token_length()
        out.append(({"name": "fixture_" + case, "words": [(w + n_sp).tolist() for w in words],
                     "counts": counts.tolist(), "n_initial": n_sp + tr.num_codebooks * tr.codebook_size,
                     "vocab_size": tr.vocab_size, "min_frequency": tr.min_frequency,
                     "maxlen": ml + 1 if ml is not None else 0},
                    [tuple(m[:2]) for m in arrays[case + "_merges"].tolist()]))
    return out


def merge_list(c, faults, cap=None):
    e = R.Emulation(c["words"], c["counts"], c["maxlen"], faults=faults)
    return [p[:2] for k, p in R.drive(e, c, max_merges=cap) if k == "merge"]


def test_which_faults_the_old_corpora_let_through():
    old = old_random_corpora()
    base = {c["name"]: merge_list(c, ()) for c in old}
    for c in old:  # the emulation is the oracle on them
        _, m = train_bpe(c["words"], c["counts"], c["n_initial"] - 1, 1, c["vocab_size"], c["min_frequency"],
                         c["maxlen"] or None)
        assert m == base[c["name"]]
    fix = fixture_corpora()
    for c, m in fix:
        assert merge_list(c, ()) == m
    unnoticed_random, unnoticed = [], []
    for fault in R.FAULTS:
        if all(merge_list(c, [fault], len(base[c["name"]]) + 2) == base[c["name"]] for c in old):
            unnoticed_random.append(fault)
            if all(merge_list(c, [fault], len(m) + 2) == m for c, m in fix):
                unnoticed.append(fault)
    print("\npass the random corpora of tests/test_bpe.py unnoticed:", unnoticed_random)
    print("pass the fixture too:", unnoticed)
    assert unnoticed_random == EXPECT_UNNOTICED_RANDOM
    assert unnoticed == EXPECT_UNNOTICED


# In the order of FAULTS.  6 is dead code (above); 10 needs an id above 65535; 11 and 12 need a rebuild that matters
# (the default table never grows on those corpora, and the post-count rebuild only drops count-1 pairs that never
# become winners there); 13 needs more than grid x 256 = 524 288 symbols at the default grid.  Both lists are equal:
# the 82 536-symbol fixture adds nothing to what the random corpora catch.
EXPECT_UNNOTICED_RANDOM = ["no_11_exemption", "id16", "rebuild_gt1", "rebuild_keeps_nkeys", "single_pass"]
EXPECT_UNNOTICED = ["no_11_exemption", "id16", "rebuild_gt1", "rebuild_keeps_nkeys", "single_pass"]


# ---- argument checks that return before any device call ----------------------------------------------------------
def _create(lib, sym, offs, cnt, n_words, n_initial, vocab, opts=None, n_symbols=None, out=True):
    from mimi_hip import _lib
    sym, offs, cnt = np.asarray(sym, np.int32), np.asarray(offs, np.int64), np.asarray(cnt, np.int64)
    h = ctypes.c_void_p()
    o = _lib.BpeOptionsC(*opts, 0) if opts else None
    n = sym.size if n_symbols is None else n_symbols
    rc = lib.mimi_bpe_create_opts(0, sym.ctypes.data, n, offs.ctypes.data, cnt.ctypes.data, n_words, n_initial, vocab,
                                  0, ctypes.byref(o) if o else None, ctypes.byref(h) if out else None)
    assert not h.value
    return rc, (lib.mimi_last_error() or b"").decode()


def test_create_argument_checks_need_no_device():
    from mimi_hip import _lib, bpe
    lib = _lib.load()
    for s in ("mimi_bpe_create_opts", "mimi_bpe_info", "mimi_bpe_read_pairs", "mimi_bpe_read_words"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s)
    ok = ([1, 2, 1], [0, 3], [1], 1, 4, 16)
    bad_opts = {(1000, 0): "power of two", (64, 0): "below 8 x vocab_size", (-1024, 0): "power of two",
                (0, -1): "grid_blocks", (1 << 20, (1 << 20) + 1): "grid_blocks"}
    for opts, msg in bad_opts.items():
        rc, err = _create(lib, *ok, opts=opts)
        assert rc == 1 and msg in err, (opts, rc, err)
    assert _create(lib, *ok, opts=(128, 1), out=False)[0] == 1
    # vocab_size: 131071 is the last one the id packing holds
    rc, err = _create(lib, [1], [0, 1], [1], 1, 4, 131072)
    assert rc == 1 and "vocab_size" in err
    assert _create(lib, [1], [0, 1], [1], 1, 0, 16)[0] == 1 and _create(lib, [1], [0, 1], [1], 1, 17, 16)[0] == 1
    # the corpus checks of mimi_bpe_create
    assert _create(lib, [1, 2], [1, 2], [1], 1, 4, 16) == (1, "word offsets must run from 0 to n_symbols")
    assert _create(lib, [1, 2], [0, 1], [1], 1, 4, 16) == (1, "word offsets must run from 0 to n_symbols")
    assert _create(lib, [1, 2], [0, 2, 1, 2], [1, 1, 1], 3, 4, 16) == (1, "word offsets must be non-decreasing")
    assert _create(lib, [1, 4], [0, 2], [1], 1, 4, 16) == (1, "symbol 4 outside the initial tokens")
    assert _create(lib, [1, -1], [0, 2], [1], 1, 4, 16) == (1, "symbol -1 outside the initial tokens")
    assert _create(lib, [1, 2], [0, 2], [-1], 1, 4, 16)[0] == 5
    assert _create(lib, [1, 2], [0, 2], [1 << 31], 1, 4, 16)[0] == 5
    assert _create(lib, [1, 2], [0, 2], [1], 1, 4, 16, n_symbols=-1)[0] == 1
    assert _create(lib, [1, 2], [0, 2], [1], -1, 4, 16)[0] == 1
    assert _create(lib, [1, 2], [0, 2], [1], 0, 4, 16)[0] == 1  # symbols that belong to no word
    h = ctypes.c_void_p()
    assert lib.mimi_bpe_create_opts(0, None, 2, None, None, 1, 4, 16, 0, None, ctypes.byref(h)) == 1
    assert lib.mimi_bpe_create_opts(0, None, 0, None, None, 1, 4, 16, 0, None, ctypes.byref(h)) == 1
    assert lib.mimi_bpe_create(0, None, 2, None, None, 1, 4, 16, 0, ctypes.byref(h)) == 1
    v = ctypes.c_int64()
    assert lib.mimi_bpe_info(None, 0, ctypes.byref(v)) == 1
    assert lib.mimi_bpe_read_pairs(None, None, None, None, 0, ctypes.byref(v)) == 1
    assert lib.mimi_bpe_read_words(None, None, 0, None, 0, ctypes.byref(v)) == 1
    # train_words_gpu: ValueError before any device call
    words, counts = [np.array([0, 1, 0], np.int32)], np.array([1])
    with pytest.raises(ValueError, match="131071"):
        bpe.train_words_gpu(words, counts, 3, 1, 131072, 1, None)
    with pytest.raises(ValueError, match="power of two"):
        bpe.train_words_gpu(words, counts, 3, 1, 16, 1, None, min_table_slots=1000)
    with pytest.raises(ValueError, match="below 8 x vocab_size"):
        bpe.train_words_gpu(words, counts, 3, 1, 16, 1, None, min_table_slots=64)
    with pytest.raises(ValueError, match="grid_blocks"):
        bpe.train_words_gpu(words, counts, 3, 1, 16, 1, None, grid_blocks=-1)
    with pytest.raises(ValueError, match="grid_blocks"):
        bpe.train_words_gpu(words, counts, 3, 1, 16, 1, None, grid_blocks=0)
