"""The id stream on the GPU (``bpe_decode_stream.hip`` through ``mimi_bpe_decode_stream_*`` / ``bpe.IdStream``): token
ids chunk by chunk per slot -> the whole frames they complete.  Every comparison is exact integer equality; the
expected frames are ``Encoder.decode_ids`` of everything a session was fed (pinned to the ``tokenizers`` fixture by
tests/test_bpe_decode.py) or the contract class of tests/bpe_decode_stream_ref.py (pinned to ``decode_ids`` by
tests/test_bpe_decode_stream_ref.py) -- never the new kernel."""
import ctypes

import numpy as np
import pytest
import torch

import bpe_decode_cases as cases
import bpe_decode_stream_ref as ref
from mimi_hip import _lib, bpe

pytestmark = pytest.mark.gpu

TILE = 256  # ids per tile and characters per row of the step kernel (its workgroup's threads)
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.array(a)).to("cuda:0", dtype)


def step(st, slots, chunks, fill=0, width=None, out=None):
    """One IdStream step of the chunks (padded with `fill`); the frames of each item on the host, int64 [K, T]."""
    ids, counts = ref.pad_ids(chunks, fill, width)
    codes, frames = st.step(dev(ids), slots=slots, counts=counts, out=out)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == (len(slots), st.num_codebooks, max(frames))
    h = codes.cpu().numpy().astype(np.int64)
    for i, f in enumerate(frames):
        assert (h[i, :, f:] == 0).all() or out is not None  # zero past an item's frames in a tensor made by the call
    return [np.ascontiguousarray(h[i, :, :f]) for i, f in enumerate(frames)]


def feed(st, slot, ids, cuts):
    """`ids` to one slot in pieces that end at `cuts`: the frames end to end."""
    out, a = [], 0
    for b in list(cuts) + [len(ids)]:
        out.append(step(st, [slot], [ids[a:b]])[0])
        a = b
    return np.concatenate(out, axis=1)


def alphabet_ids(enc, cb, rng):
    cb = np.asarray(cb, np.int64)
    return (enc.n_special + cb * enc.codebook_size + rng.integers(0, enc.codebook_size, size=cb.size)).astype(np.int32)


def cycle(enc, rng, n, phase=0):
    return alphabet_ids(enc, (phase + np.arange(n)) % enc.num_codebooks, rng)


# ---- the schedule ----------------------------------------------------------------------------------------------------
def test_schedule_equals_the_reference_pool_at_every_step():
    enc = ref.schedule_encoder()
    sessions = ref.make_sessions(enc)
    pool = ref.PoolRef(enc, ref.SCHED_SLOTS)
    want_log, want = ref.play(sessions, pool.step, pool.reset)
    check = ref.PoolRef(enc, ref.SCHED_SLOTS)  # stepped beside the stream for `pending`
    with enc.decode_stream(ref.SCHED_SLOTS, 32) as st:
        assert st.pending == [-1] * ref.SCHED_SLOTS

        def one(slots, chunks):
            got = step(st, slots, chunks)
            check.step(slots, chunks)
            assert st.pending == check.pending, (slots, st.pending, check.pending)
            return got

        def reset(slot):
            st.reset(slot)
            check.reset(slot)
            assert st.pending == check.pending

        log, got = ref.play(sessions, one, reset)
    for i, ((slots, names, _, frames), (_, _, _, wframes)) in enumerate(zip(log, want_log)):
        for n, f, w in zip(names, frames, wframes):
            assert f.shape == w.shape and np.array_equal(f, w), (i, slots, n)
    for name in sessions:
        assert np.array_equal(got[name], enc.decode_ids([ref.session_ids(sessions, name)])[0]), name
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("K", (1, 2, 8, 16))
def test_codebook_counts_under_every_split(K):
    enc = cases.hand_encoder(K, seed=K, chain=2)
    rng = np.random.default_rng(K)
    n = 60
    with enc.decode_stream(2, n) as st:
        for trial in range(2):
            ids = cases.random_ids(enc, rng, n, special=0.1)
            if trial:  # a stream that mostly cycles, from a codebook that need not be 0
                ids = cycle(enc, rng, n, phase=int(rng.integers(K)))
                ids[rng.integers(0, n, size=4)] = cases.random_ids(enc, rng, 4)
            want = enc.decode_ids([ids])[0]
            for name, cuts in ref.splits(n, seed=trial).items():
                st.reset(1)
                got = feed(st, 1, ids, cuts)
                assert got.shape == want.shape and np.array_equal(got, want), (K, trial, name)


# ---- carries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (TILE + 1, 2 * TILE + 1))
def test_a_step_crosses_the_id_tile(n):
    enc = cases.trained_encoder("k8_recipe")
    rng = np.random.default_rng(n)
    head = cycle(enc, rng, 13, phase=3)
    body = cycle(enc, rng, n, phase=(3 + 13) % 8)
    body[rng.integers(0, n, size=9)] = cases.random_ids(enc, rng, 9)             # learned ids and specials among them
    body[[TILE - 1, TILE]] = alphabet_ids(enc, [(3 + 13 + TILE) % 8, 0], rng)    # a dropped character first in tile 2
    with enc.decode_stream(2, n) as st:
        got = feed(st, 0, np.concatenate([head, body]), [13])
    want = enc.decode_ids([np.concatenate([head, body])])[0]
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("chars", (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1))
def test_a_step_spells_a_row_boundary(chars):
    """Learned ids of a trained model (several characters each, all kept) that spell `chars` characters in one step,
    behind 3 pending codes and in front of a short step."""
    enc = cases.trained_encoder("k8_recipe")
    rng = np.random.default_rng(chars)
    head = cycle(enc, rng, 5 + 3, phase=3)  # 5 owed, 3 pending
    body = ref.cycling_ids(enc, rng, chars, phase=(3 + 8) % 8)
    assert cases.spelled_length(enc, body) == chars and len(body) < 0.8 * chars  # learned ids among them
    rest = cycle(enc, rng, 11, phase=(3 + chars) % 8)
    ids = np.concatenate([head, body, rest])
    with enc.decode_stream(1, len(body)) as st:
        got = feed(st, 0, ids, [len(head), len(head) + len(body)])
    want = enc.decode_ids([ids])[0]
    assert want.shape == (8, (3 + chars + 11) // 8)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("npend", range(8))
def test_one_id_of_eight_frames_behind_pending_codes(npend):
    """An id that spells 64 = 8 K cycling characters behind `npend` pending codes: its first `npend` characters are
    dropped (the slot expects codebook `npend`), the rest complete 8 frames, the pending codes in column 0."""
    enc, chain = ref.frame_chain_encoder(8, doublings=3)
    rng = np.random.default_rng(npend)
    ids = np.concatenate([cycle(enc, rng, npend), [chain], cycle(enc, rng, 8)]).astype(np.int32)
    with enc.decode_stream(1, 8) as st:
        if npend:
            assert step(st, [0], [ids[:npend]])[0].shape == (8, 0)
        assert st.pending == [npend if npend else -1]
        mid = step(st, [0], [ids[npend:npend + 1]])[0]
        assert mid.shape == (8, 8) and st.pending == [0]
        tail = step(st, [0], [ids[npend + 1:]])[0]
    want = enc.decode_ids([ids])[0]
    assert want.shape == (8, 9)
    assert np.array_equal(np.concatenate([mid, tail], axis=1), want)


def test_a_codebook_awaited_across_row_tile_and_step():
    enc = cases.hand_encoder(8, seed=1)
    rng = np.random.default_rng(5)
    head = cycle(enc, rng, 8 + 5)                                    # expected = 5, 5 codes pending
    other = np.array([0, 1, 2, 3, 4, 6, 7])
    junk1 = alphabet_ids(enc, other[rng.integers(0, 7, size=2 * TILE + 40)], rng)  # past two rows and two id tiles
    junk2 = alphabet_ids(enc, other[rng.integers(0, 7, size=9)], rng)
    tail = cycle(enc, rng, 19, phase=5)
    ids = np.concatenate([head, junk1, junk2, tail])
    cuts = [len(head) + len(junk1), len(head) + len(junk1) + len(junk2)]
    with enc.decode_stream(1, cuts[0]) as st:
        a = step(st, [0], [ids[:cuts[0]]])[0]
        assert st.pending == [5]
        b = step(st, [0], [ids[cuts[0]:cuts[1]]])[0]
        assert b.shape == (8, 0) and st.pending == [5]
        c = step(st, [0], [ids[cuts[1]:]])[0]
    want = enc.decode_ids([ids])[0]
    assert want.shape == (8, 4)
    assert np.array_equal(np.concatenate([a, b, c], axis=1), want)


# ---- what a step must not touch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", (INT32_MAX, -1))
def test_ids_past_the_count_are_never_read(fill):
    enc = ref.schedule_encoder()
    sessions = ref.make_sessions(enc)
    with enc.decode_stream(ref.SCHED_SLOTS, 32) as st:
        _, got = ref.play(sessions, lambda s, c: step(st, s, c, fill=fill, width=32), st.reset)
    for name in sessions:
        assert np.array_equal(got[name], enc.decode_ids([ref.session_ids(sessions, name)])[0]), (fill, name)


def test_columns_past_the_frames_are_never_written():
    enc = ref.schedule_encoder()
    rng = np.random.default_rng(2)
    chunks = [cycle(enc, rng, 21), cycle(enc, rng, 3, phase=2), np.zeros(0, np.int32)]
    with enc.decode_stream(3, 32) as st:
        cap = st.max_frames(21)
        out = torch.full((3, 8, cap + 2), -7, dtype=torch.int32, device="cuda:0")
        ids, counts = ref.pad_ids(chunks)
        codes, frames = st.step(dev(ids), slots=[2, 0, 1], counts=counts, out=out)
        assert frames == [2, 0, 0] and codes.data_ptr() == out.data_ptr() and tuple(codes.shape) == (3, 8, 2)
        h = out.cpu().numpy()
        assert np.array_equal(h[0, :, :2], enc.decode_ids([chunks[0]])[0])
        assert (h[0, :, 2:] == -7).all() and (h[1:] == -7).all()
        assert st.pending == [0, -1, 5]  # slot 0: 3 characters from codebook 2, all of them owed


@pytest.mark.parametrize("neighbour", ("random", "specials", "bad_id"))
def test_a_neighbour_does_not_change_a_slot(neighbour):
    enc = ref.schedule_encoder()
    rng = np.random.default_rng(7)
    ids = cycle(enc, rng, 50, phase=6)
    ids[[9, 30]] = cases.random_ids(enc, rng, 2)
    want = enc.decode_ids([ids])[0]
    parts = []
    with enc.decode_stream(2, 8) as st:
        for a in range(0, 50, 5):
            if neighbour == "bad_id":  # in a call of its own: a call with a bad id has no result
                with pytest.raises(ValueError, match="outside"):
                    st.step(dev([[3, enc.n_tokens, 4]]), slots=[1])
                st.reset(1)
                parts.append(step(st, [0], [ids[a:a + 5]])[0])
            else:
                other = cases.random_ids(enc, rng, 7) if neighbour == "random" else rng.integers(0, 2, size=4)
                parts.append(step(st, [1, 0], [other.astype(np.int32), ids[a:a + 5]])[1])
    assert np.array_equal(np.concatenate(parts, axis=1), want)


def test_a_bad_id_stops_the_calls_slots_until_reset():
    enc = ref.schedule_encoder()
    rng = np.random.default_rng(8)
    seq = [cycle(enc, rng, 30, phase=s) for s in range(3)]
    with enc.decode_stream(3, 32) as st:
        got = {s: [step(st, [s], [seq[s][:10]])[0]] for s in range(3)}
        for bad in (enc.n_tokens, -1, INT32_MAX):
            st.reset(0), st.reset(2)
            ids = np.stack([seq[2][:4], seq[0][:4]])
            ids[1, 2] = bad
            with pytest.raises(ValueError, match="outside"):
                st.step(dev(ids), slots=[2, 0])
            for slots in ([0], [2], [1, 2]):
                with pytest.raises(_lib.MimiHipError, match="reset"):
                    st.step(dev(np.stack([seq[s][:2] for s in slots])), slots=slots)
        got[1].append(step(st, [1], [seq[1][10:]])[0])  # the unlisted slot goes on
        st.reset(0)
        got[0] = [step(st, [0], [seq[0]])[0]]
        with pytest.raises(_lib.MimiHipError, match="reset"):
            st.step(dev(seq[2][None, :2]), slots=[2])  # still refuses: only slot 0 was reset
        st.reset()
        got[2] = [step(st, [2], [seq[2]])[0]]
        assert st.pending[1] == -1
    for s in range(3):
        assert np.array_equal(np.concatenate(got[s], axis=1), enc.decode_ids([seq[s]])[0]), s


def test_argument_errors_leave_every_slot_as_it_was():
    enc = ref.schedule_encoder()
    rng = np.random.default_rng(9)
    with enc.decode_stream(3, 16) as st:
        step(st, [0, 2], [cycle(enc, rng, 11), cycle(enc, rng, 5, phase=1)])
        before = st.pending
        assert before == [3, -1, 0]
        ids = dev(np.stack([cycle(enc, rng, 8)] * 2))
        bad_calls = [
            dict(ids=ids, slots=[0, 0]), dict(ids=ids, slots=[0, 3]), dict(ids=ids, slots=[-1, 1]),
            dict(ids=ids, slots=[]), dict(ids=ids, slots=[0, 1, 2]), dict(ids=ids[0], slots=[0]),
            dict(ids=ids, slots=[0, 1], counts=[1]), dict(ids=ids, slots=[0, 1], counts=[9, 1]),
            dict(ids=ids, slots=[0, 1], counts=[-1, 1]), dict(ids=ids.cpu(), slots=[0, 1]),
            dict(ids=ids.float(), slots=[0, 1]), dict(ids=dev(np.zeros((2, 17))), slots=[0, 1]),
            dict(ids=ids, slots=[0, 1], out=torch.zeros((2, 8, 1), dtype=torch.int32, device="cuda:0")),
            dict(ids=ids, slots=[0, 1], out=torch.zeros((2, 8, 64), dtype=torch.int64, device="cuda:0")),
        ]
        for kw in bad_calls:
            with pytest.raises(ValueError):
                st.step(**kw)
            assert st.pending == before, kw
        with pytest.raises(ValueError):
            st.reset(3)
        with pytest.raises(ValueError):
            st.max_frames(-1)
        assert st.pending == before
        rest = cycle(enc, rng, 5, phase=3)  # the slot goes on where it was
        assert step(st, [0], [rest])[0].shape == (8, 1)
    with pytest.raises(ValueError):
        enc.decode_stream(0, 4)
    with pytest.raises(ValueError):
        enc.decode_stream(1, 0)


def test_more_than_16_codebooks_is_not_implemented():
    enc = cases.hand_encoder(17)
    with pytest.raises(NotImplementedError):
        enc.decode_stream(1, 4)
    lib, h = _lib.load(), ctypes.c_void_p()
    assert lib.mimi_bpe_decode_stream_create(enc._decode_model(), 1, 4, ctypes.byref(h)) == 5 and not h


def test_closing_the_encoder_closes_its_streams():
    enc = cases.hand_encoder(2, seed=4)
    st = enc.decode_stream(1, 4)
    enc.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.pending


# ---- the C ABI alone -------------------------------------------------------------------------------------------------
def test_through_ctypes_alone():
    enc, chain = ref.frame_chain_encoder(8, doublings=1)  # the id spells 16 characters: Lmax
    lib, h = _lib.load(), ctypes.c_void_p()
    m = enc._decode_model()
    assert lib.mimi_bpe_decode_stream_create(m, 2, 4, ctypes.byref(h)) == 0
    try:
        assert lib.mimi_bpe_decode_stream_max_frames(h, 0) == 0
        assert lib.mimi_bpe_decode_stream_max_frames(h, 3) == (7 + 3 * 16) // 8
        assert [lib.mimi_bpe_decode_stream_slot_pending(h, s) for s in (0, 1, 2)] == [-1, -1, -2]
        two = ctypes.c_int32 * 2
        ids = dev([[2 + 4 * 3 + 1, 0, 0, 0], [chain, 2, 2 + 4 + 3, 0]])  # slot 1: (3, 1); slot 0: 2 frames, (0, 0), (1, 3)
        codes = torch.full((2, 8, 6), -1, dtype=torch.int32, device="cuda:0")
        frames = two()
        args = (ctypes.c_void_p(ids.data_ptr()), 4, ctypes.c_void_p(codes.data_ptr()))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or None)
        torch.cuda.synchronize()
        assert lib.mimi_bpe_decode_stream_step(h, two(1, 0), two(1, 3), 2, *args, 5, frames, stream) == 1  # max_frames
        assert lib.mimi_bpe_decode_stream_step(h, two(1, 1), two(1, 3), 2, *args, 6, frames, stream) == 1
        assert lib.mimi_bpe_decode_stream_step(h, two(1, 0), two(1, 5), 2, *args, 6, frames, stream) == 1
        assert [lib.mimi_bpe_decode_stream_slot_pending(h, s) for s in (0, 1)] == [-1, -1]
        assert lib.mimi_bpe_decode_stream_step(h, two(1, 0), two(1, 3), 2, *args, 6, frames, stream) == 0
        assert list(frames) == [0, 2]
        assert [lib.mimi_bpe_decode_stream_slot_pending(h, s) for s in (0, 1)] == [2, 0]  # slot 1: 5 owed, 1 paid
        got = codes.cpu().numpy()
        assert (got[0] == -1).all() and (got[1, :, :2] == 0).all() and (got[1, :, 2:] == -1).all()
        assert lib.mimi_bpe_decode_stream_reset_slot(h, 2) == 1
        assert lib.mimi_bpe_decode_stream_reset_slot(h, 0) == 0
        assert [lib.mimi_bpe_decode_stream_slot_pending(h, s) for s in (0, 1)] == [-1, 0]
        assert lib.mimi_bpe_decode_stream_reset(h) == 0
        assert lib.mimi_bpe_decode_stream_slot_pending(h, 1) == -1
    finally:
        lib.mimi_bpe_decode_stream_destroy(h)
