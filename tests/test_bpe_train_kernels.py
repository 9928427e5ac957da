"""The codec-BPE trainer's device state after every merge (``csrc/bpe.hip`` through the C entries), against
``tests/bpe_train_ref.Reference``: a from-scratch rewrite and recount that shares nothing with the kernels.

``mimi_bpe_best`` must give the reference's (left, right, count) at every step, and after ``mimi_bpe_merge`` the words
(``mimi_bpe_read_words``, which also checks the links) and every positive pair count (``mimi_bpe_read_pairs``) must
equal the reference's exactly -- under the default options, under the smallest table ``mimi_bpe_create_opts`` accepts
(so the table grows in ``mimi_bpe_best``), and under ``grid_blocks`` 1 and 3 (so every grid-stride loop goes round).
The figures printed here (slots, rehashes, strides) are recorded in ``profiles/bpe_train_state.txt``."""
import ctypes

import numpy as np
import pytest

import bpe_train_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip import _lib
    return _lib.load()


class Gpu:
    """One mimi_bpe handle with the interface of the reference models."""

    def __init__(self, lib, c, min_table_slots=None, grid_blocks=None):
        from mimi_hip import _lib
        self._lib, self._check, self._info = lib, _lib.check, _lib.BPE_TRAIN_INFO
        words = c["words"]
        self.n_words = len(words)
        offs = np.zeros(len(words) + 1, dtype=np.int64)
        np.cumsum([len(w) for w in words], out=offs[1:])
        sym = np.array([x for w in words for x in w], dtype=np.int32)
        cnt = np.array(c["counts"], dtype=np.int64)
        self.n = int(sym.size)
        self.h = ctypes.c_void_p()
        opts = _lib.BpeOptionsC(int(min_table_slots or 0), int(grid_blocks or 0), 0)
        self._check(lib.mimi_bpe_create_opts(0, sym.ctypes.data, sym.size, offs.ctypes.data, cnt.ctypes.data,
                                             len(words), c["n_initial"], c["vocab_size"], c["maxlen"],
                                             ctypes.byref(opts), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self._lib.mimi_bpe_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def best(self):
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self._lib.mimi_bpe_best(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return (a.value, b.value, c.value)

    def merge(self, a, b, nid, nlen):
        self._check(self._lib.mimi_bpe_merge(self.h, a, b, nid, nlen))

    def info(self, key):
        v = ctypes.c_int64()
        self._check(self._lib.mimi_bpe_info(self.h, self._info[key], ctypes.byref(v)))
        return v.value

    def words(self):
        sym = np.empty(max(self.n, 1), dtype=np.int32)
        lens = np.zeros(max(self.n_words, 1), dtype=np.int64)
        n = ctypes.c_int64()
        self._check(self._lib.mimi_bpe_read_words(self.h, sym.ctypes.data, self.n, lens.ctypes.data, self.n_words,
                                                  ctypes.byref(n)))
        out, at = [], 0
        for k in lens[:self.n_words].tolist():
            out.append(sym[at:at + k].tolist())
            at += k
        assert at == n.value
        return out

    def pairs(self):
        n = ctypes.c_int64()
        self._check(self._lib.mimi_bpe_read_pairs(self.h, None, None, None, 0, ctypes.byref(n)))
        cap = max(n.value, 1)
        left, right = np.empty(cap, np.int32), np.empty(cap, np.int32)
        cnt = np.empty(cap, np.int64)
        self._check(self._lib.mimi_bpe_read_pairs(self.h, left.ctypes.data, right.ctypes.data, cnt.ctypes.data, cap,
                                                  ctypes.byref(n)))
        out = dict(zip(zip(left[:n.value].tolist(), right[:n.value].tolist()), cnt[:n.value].tolist()))
        assert len(out) == n.value, "a pair is in the table twice"
        return out


_REF = {}


def reference(c, forced=()):
    """The reference's trajectory of a corpus (computed once, shared, never changed)."""
    key = (c["name"], tuple(forced))
    if key not in _REF:
        _REF[key] = R.trajectory(R.Reference(c["words"], c["counts"], c["maxlen"]), c, forced)
    return _REF[key]


def audit(g, c, forced=(), sparse=False, also=()):
    """Run handle g through c in step with the reference; compare every winner, and the whole state after the
    merges chosen by `sparse` (the first 16, every 8th, the last one) and after merge numbers in `also`.  Returns the
    merges."""
    ref = reference(c, forced)
    w, p = ref[0][2]
    assert g.words() == w and g.pairs() == p, (c["name"], "creation")
    i, step, n_merges = 1, 0, len(R.merges_of(ref))
    rehashes = g.info("growth_rehashes")
    for kind, payload in R.drive(g, c, forced):
        rk, rp, rs = ref[i]
        i += 1
        assert (kind, payload) == (rk, rp), (c["name"], "step", step, "device", kind, payload, "reference", rk, rp)
        if kind == "best":
            # the state after a growth rehash is audited at the next merge whatever `sparse` says
            grown, rehashes = g.info("growth_rehashes") != rehashes, g.info("growth_rehashes")
            also = set(also) | ({step + 1} if grown else set())
            continue
        step += 1
        if not sparse or step <= 16 or step % 8 == 0 or step == n_merges or step in also:
            assert g.words() == rs[0], (c["name"], "words after merge", step, payload)
            got = g.pairs()
            if got != rs[1]:
                diff = {k: (got.get(k), rs[1].get(k)) for k in set(got) | set(rs[1]) if got.get(k) != rs[1].get(k)}
                raise AssertionError((c["name"], "pairs after merge", step, payload, "(device, reference)", diff))
    assert i == len(ref)
    return R.merges_of(ref)


CORPORA = {c["name"]: c for c in R.all_corpora()}
SPARSE = ("growth", "strided", "runs")
SETTINGS = {"default": lambda c: {}, "small_table": lambda c: {"min_table_slots": R.small_table(c["vocab_size"])},
            "small_table_grid1": lambda c: {"min_table_slots": R.small_table(c["vocab_size"]), "grid_blocks": 1},
            "small_table_grid3": lambda c: {"min_table_slots": R.small_table(c["vocab_size"]), "grid_blocks": 3}}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(CORPORA))
def test_state_after_every_merge(lib, name, setting):
    c = CORPORA[name]
    kw = SETTINGS[setting](c)
    emu = R.Emulation(c["words"], c["counts"], c["maxlen"], **kw)
    for _ in R.drive(emu, c):
        pass
    with Gpu(lib, c, **kw) as g:
        if "grid_blocks" in kw:
            assert g.info("grid_blocks") == kw["grid_blocks"]
        assert g.info("symbols") == sum(map(len, c["words"]))
        audit(g, c, sparse=name in SPARSE)
        got = (g.info("table_slots"), g.info("growth_rehashes"), g.info("nkeys"))
        print(f"{name} {setting}: symbols {g.info('symbols')} grid_blocks {g.info('grid_blocks')} table_slots {got[0]} "
              f"growth_rehashes {got[1]} nkeys {got[2]} merges {len(R.merges_of(reference(c)))}")
        # the table's bookkeeping is exactly the emulation's
        assert got == (emu.slots, emu.rehashes, emu.nkeys), (got, (emu.slots, emu.rehashes, emu.nkeys))


def test_growth_rehashes_are_predicted_and_merges_equal_the_oracle(lib):
    from oracle.bpe_ref import train_bpe
    c = CORPORA["growth"]
    slots = R.small_table(c["vocab_size"])
    assert slots == 1024
    emu = R.Emulation(c["words"], c["counts"], c["maxlen"], min_table_slots=slots)
    grow_steps, step = [], 0
    for kind, _ in R.drive(emu, c):
        if kind == "merge":
            step += 1
        elif emu.rehashes > len(grow_steps):
            grow_steps.append(step)  # this best() doubled the table: audit the state after the next merge
    assert emu.rehashes >= 2, emu.rehashes
    with Gpu(lib, c, min_table_slots=slots) as g:
        merges = audit(g, c, sparse=True, also=[s + 1 for s in grow_steps])
        assert (g.info("table_slots"), g.info("growth_rehashes")) == (emu.slots, emu.rehashes)
        print(f"growth: table_slots {emu.slots} after {emu.rehashes} growth rehashes, at merges {grow_steps}")
    _, om = train_bpe(c["words"], c["counts"], c["n_initial"] - 1, 1, c["vocab_size"], c["min_frequency"], None)
    assert merges == om


def test_every_loop_strides(lib):
    """grid_blocks 1: 256 threads over 6-8 k symbols (>= 20 rounds of count / mark), over the starts of a merge and,
    at the small table, over the slots in both best sweeps and in the rehash."""
    c = CORPORA["strided"]
    with Gpu(lib, c, min_table_slots=R.small_table(c["vocab_size"]), grid_blocks=1) as g:
        assert g.info("grid_blocks") == 1
        rounds = g.info("symbols") // 256
        assert rounds >= 20, rounds
        assert g.info("table_slots") // 256 >= 2
        audit(g, c, sparse=True)
        assert g.info("growth_rehashes") >= 1
        print(f"strided grid_blocks 1: {rounds} rounds over the symbols, {g.info('table_slots') // 256} over the table")


def test_high_ids_win_and_tie_as_the_reference(lib):
    c = CORPORA["highid"]
    ref = reference(c)
    winners = [p for k, p, _ in ref if k == "best"]
    sides = {(a < 65536, b < 65536) for a, b, _ in winners if a >= 0}
    assert sides == {(True, True), (True, False), (False, True), (False, False)}, sides
    assert any(131070 in (a, b) for a, b, _ in winners), "no winner holds the last id"
    with Gpu(lib, c) as g:
        audit(g, c)


FORCED = R.forced_schedules()


@pytest.mark.parametrize("name", list(FORCED))
def test_forced_schedules(lib, name):
    c = R.forced_corpus()
    with Gpu(lib, c, min_table_slots=R.small_table(c["vocab_size"]), grid_blocks=1) as g:
        audit(g, c, FORCED[name])
    with Gpu(lib, c) as g:
        audit(g, c, FORCED[name])


def test_two_handles_interleaved(lib):
    c1, c2 = R.forced_corpus(), CORPORA["overlap"]
    f1 = FORCED["aa_existing_id"]
    r1, r2 = reference(c1, f1), reference(c2)
    with Gpu(lib, c1, min_table_slots=R.small_table(c1["vocab_size"])) as g1, Gpu(lib, c2) as g2:
        d1, d2 = R.drive(g1, c1, f1), R.drive(g2, c2)
        i1 = i2 = 1
        while d1 is not None or d2 is not None:
            for which in (1, 2):
                d, g, ref, i = (d1, g1, r1, i1) if which == 1 else (d2, g2, r2, i2)
                if d is None:
                    continue
                ev = next(d, None)
                if ev is None:
                    assert i == len(ref)
                    if which == 1:
                        d1 = None
                    else:
                        d2 = None
                    continue
                assert ev == ref[i][:2], (which, i, ev, ref[i][:2])
                if ev[0] == "merge":
                    assert (g.words(), g.pairs()) == ref[i][2], (which, i, ev)
                if which == 1:
                    i1 += 1
                else:
                    i2 += 1


def test_same_corpus_twice_gives_the_same_state(lib):
    """The order of the starts list differs from run to run (an atomic counter hands out its slots); the state
    must not."""
    c = CORPORA["overlap"]
    runs = []
    for _ in range(2):
        with Gpu(lib, c, grid_blocks=3) as g:
            states = []
            for kind, payload in R.drive(g, c):
                states.append((kind, payload, (g.words(), g.pairs()) if kind == "merge" else None))
            runs.append(states)
    assert runs[0] == runs[1]
