"""Codec-BPE decoding on the GPU (``bpe_decode.hip`` through ``mimi_bpe_decode_plan`` / ``mimi_bpe_decode_write`` /
``bpe.Encoder.decode_device`` / ``codes.ids_to_audio``): token ids in device memory -> codes in device memory.  Every
comparison is exact integer equality; the expected codes are the committed fixture (``tokenizers`` ``decode`` followed
by the reference converter) or the host rules ``decode_ids`` (pinned to that fixture and to a per-character loop by
tests/test_bpe_decode.py) -- never the new kernels."""
import ctypes

import numpy as np
import pytest
import torch

import bpe_decode_cases as cases
import bpe_encode_cases as enc_cases
from mimi_hip import _lib, bpe, synthetic

pytestmark = pytest.mark.gpu

OFFSET, CBS = cases.OFFSET, cases.CBS
TILE = _lib.BPE_DECODE_SCAN_TILE  # positions per workgroup of the scan kernels
ROW = 256                         # positions per workgroup-wide scan step inside a tile (the workgroup's threads)
PARTIALS_PASS = 256               # tile values the scan-of-partials workgroup takes per pass
INT32_MAX = 2 ** 31 - 1


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.array(a)).to("cuda:0", dtype)  # (a copy: fixture arrays are read-only)


def offsets_of(seqs):
    offs = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    return offs


def flat_of(seqs):
    return np.concatenate([np.asarray(s, np.int32) for s in seqs]) if seqs else np.zeros(0, np.int32)


def run(enc, seqs, **kw):
    """decode_device of the sequences in one call, on the host as a list of [K, T] arrays."""
    got = enc.decode_device(dev(flat_of(seqs)), offsets_of(seqs), to_host=True, **kw)
    assert enc.last_stats["filter"] == "device"
    return got


def assert_codes(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (tag, i, g.shape, w.shape)


def alphabet_ids(enc, cb, rng):
    """Alphabet ids whose characters have the codebooks `cb`, with random codes."""
    cb = np.asarray(cb, np.int64)
    return (enc.n_special + cb * enc.codebook_size + rng.integers(0, enc.codebook_size, size=cb.size)).astype(np.int32)


def noisy_cycle(enc, rng, n, p_delete, phase=0):
    """n characters cycling through the codebooks from `phase`, a share deleted: alphabet ids."""
    cb = (phase + np.arange(n)) % enc.num_codebooks
    return alphabet_ids(enc, cb[rng.random(n) >= p_delete], rng)


# ---- the fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES)
def test_every_fixture_entry_one_per_call_and_all_in_one_call(case):
    need_gpu()
    enc = cases.trained_encoder(case)
    entries = cases.entries(case)
    for name, ids, want in entries:
        codes, frames = enc.decode_device(dev(ids), [0, ids.size])
        assert enc.last_stats["filter"] == "device"
        assert codes.dtype == torch.int32 and codes.is_cuda and tuple(codes.shape) == (1,) + want.shape
        assert frames.dtype == np.int64 and frames.tolist() == [want.shape[1]]
        assert np.array_equal(codes[0].cpu().numpy(), want), (case, name)
    assert_codes(run(enc, [ids for _, ids, _ in entries]), [w for _, _, w in entries], case)


# ---- every K ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 16])
def test_hand_built_models(K):
    need_gpu()
    enc = cases.hand_encoder(K, seed=K)
    rng = np.random.default_rng(200 + K)
    seqs = [cases.random_ids(enc, rng, int(rng.integers(0, 500))) for _ in range(30)]
    seqs += [noisy_cycle(enc, rng, int(rng.integers(1, 3000)), p, int(rng.integers(K))) for p in (0.0, 0.1, 0.4) * 4]
    want = enc.decode_ids(seqs)
    assert sum(w.shape[1] > 0 for w in want) > 20
    assert_codes(run(enc, seqs), want, f"K={K}")


def test_seventeen_codebooks_take_the_host_path():
    need_gpu()
    enc = cases.hand_encoder(17, seed=17)
    rng = np.random.default_rng(217)
    seqs = [cases.random_ids(enc, rng, 200), noisy_cycle(enc, rng, 500, 0.1, 3), np.zeros(0, np.int32)]
    want = enc.decode_ids(seqs)
    assert want[1].shape[1] > 5
    codes, frames = enc.decode_device(dev(flat_of(seqs)), offsets_of(seqs))
    assert enc.last_stats["filter"] == "host"
    assert codes.is_cuda and codes.dtype == torch.int32 and frames.tolist() == [w.shape[1] for w in want]
    for i, w in enumerate(want):
        assert np.array_equal(codes[i, :, :w.shape[1]].cpu().numpy(), w)
    assert_codes(enc.decode_device(dev(flat_of(seqs)), offsets_of(seqs), to_host=True), want, "K=17")


# ---- the state carried over boundaries ----------------------------------------------------------------------------
def test_filter_waits_for_a_codebook_across_tile_carries():
    """A sequence lacks codebook 5 for more than two tiles of characters: `expected` stays 5 over every row, wave and
    tile carry in between and everything there is dropped."""
    need_gpu()
    enc = cases.hand_encoder(8, seed=1)
    rng = np.random.default_rng(1)
    head = alphabet_ids(enc, np.arange(8 * 3 + 5) % 8, rng)                    # ... ends with codebook 4
    others = np.array([0, 1, 2, 3, 4, 6, 7])
    gap = alphabet_ids(enc, others[rng.integers(0, 7, size=2 * TILE + 300)], rng)
    tail = alphabet_ids(enc, (5 + np.arange(8 * 4 + 3)) % 8, rng)
    seq = np.concatenate([head, gap, tail])
    want = enc.decode_ids([seq])
    assert want[0].shape[1] == 3 + 1 + 4  # the gap gives nothing: 3 frames, one across the gap, 4 after it
    for lead in (0, 1, TILE - 7):  # the gap against different tile phases
        pre = [noisy_cycle(enc, rng, lead, 0.2)] if lead else []
        assert_codes(run(enc, pre + [seq]), enc.decode_ids(pre) + want, f"lead {lead}")


def test_sequences_at_tile_and_row_boundaries():
    need_gpu()
    enc = cases.hand_encoder(8, seed=2)
    rng = np.random.default_rng(2)

    def chars(n, p=0.3):  # n characters exactly (alphabet ids), not consistent
        return noisy_cycle(enc, rng, 4 * n, p, int(rng.integers(8)))[:n]

    # starts at TILE - 1, TILE, TILE + 1; then one straddling the row boundary at 2 TILE + ROW
    lens = [TILE - 1, 1, 1, TILE + 200 - (TILE + 1), ROW + 0, 100, 3 * ROW]
    seqs = [chars(n) for n in lens]
    starts = offsets_of(seqs)
    assert starts[1:4].tolist() == [TILE - 1, TILE, TILE + 1]
    assert starts[5] < TILE + 2 * ROW < starts[6] and starts[5] // TILE == (starts[6] - 1) // TILE
    assert_codes(run(enc, seqs), enc.decode_ids(seqs), "boundaries")
    # a sequence that begins exactly with a tile and one that ends exactly with it, alone in the call
    for lens in ([TILE, TILE], [TILE + 1, TILE - 1], [ROW, ROW, ROW]):
        seqs = [chars(n) for n in lens]
        assert_codes(run(enc, seqs), enc.decode_ids(seqs), str(lens))


def test_a_spelling_straddles_a_tile_boundary():
    need_gpu()
    enc = cases.hand_encoder(8, seed=3, chain=12)  # tokens up to 40 characters and a chain up to 4096
    off, _ = enc.spellings()
    rng = np.random.default_rng(3)
    seqs = [cases.random_ids(enc, rng, 700) for _ in range(4)]
    big = enc.n_tokens - 1
    assert off[big + 1] - off[big] == 2 * TILE
    seqs.append(np.array([enc.n_special + 9, big, enc.n_special + 1, big - 1, 3], np.int32))  # > a tile in one id
    flat = flat_of(seqs)
    lens = off[flat.astype(np.int64) + 1] - off[flat.astype(np.int64)]
    first = np.cumsum(lens) - lens
    straddle = (lens > 1) & (first // TILE != (first + lens - 1) // TILE)
    assert straddle.sum() >= 3 and first[-1] > 3 * TILE
    assert_codes(run(enc, seqs), enc.decode_ids(seqs), "straddle")


def test_more_tiles_than_one_pass_of_the_partials_scan():
    """PARTIALS_PASS + 1 tiles of characters, the last tile holding one character: the carry of the scan over the tile
    values crosses its own pass boundary, for the id scan, the filter scan and the rank scan."""
    need_gpu()
    enc = cases.hand_encoder(8, seed=4)
    rng = np.random.default_rng(4)
    n = PARTIALS_PASS * TILE + 1
    a = noisy_cycle(enc, rng, 1000, 0.1)
    b = noisy_cycle(enc, rng, 2 * n, 0.1, 3)[:n - a.size]
    assert a.size + b.size == n and cases.spelled_length(enc, b) == b.size
    want = enc.decode_ids([a, b])
    assert want[1].shape[1] > n // 64
    codes, frames = enc.decode_device(dev(np.concatenate([a, b])), [0, a.size, n])
    assert enc.last_stats["filter"] == "device"
    assert frames.tolist() == [w.shape[1] for w in want]
    for i, w in enumerate(want):
        assert torch.equal(codes[i, :, :w.shape[1]], dev(w)), i


def test_order_of_composition():
    """200 random streams of 1-3 tiles that are not consistent: a scan that composed the maps in the other order
    would keep other characters (asserted on the host's own scan first, for at least half of them)."""
    need_gpu()
    enc = cases.hand_encoder(4, seed=5)
    rng = np.random.default_rng(5)
    seqs, differ = [], 0
    for _ in range(200):
        cb = rng.integers(0, 4, size=int(rng.integers(TILE, 3 * TILE + 1)))
        differ += not np.array_equal(bpe.filter_keep(cb, 4), bpe.filter_keep(cb, 4, commuted=True))
        seqs.append(alphabet_ids(enc, cb, rng))
    assert differ >= 100, differ
    assert_codes(run(enc, seqs), enc.decode_ids(seqs), "order")


# ---- batch behaviour ------------------------------------------------------------------------------------------------
def test_empty_sequences_int64_and_the_strided_2d_view():
    need_gpu()
    enc = cases.trained_encoder("k8_recipe")
    ids3 = dict((n, i) for n, i, _ in cases.entries("k8_recipe"))["ids3"]
    empty = np.zeros(0, np.int32)
    seqs = [empty, ids3[:200], empty, empty, ids3[200:230], np.zeros(4, np.int32), ids3[230:], empty]
    want = enc.decode_ids(seqs)
    assert [w.shape[1] > 0 for w in want] == [False, True, False, False, True, False, True, False]
    assert_codes(run(enc, seqs), want, "empties")
    got = enc.decode_device(dev(flat_of(seqs), torch.int64), offsets_of(seqs), to_host=True)
    assert_codes(got, want, "int64")
    # [B, L] with lengths: a strided view (every second column of a wider tensor), padding of -1 and INT32_MAX past
    # the lengths, which no kernel may read as an id
    L = max(len(s) for s in seqs)
    for dtype, pad in ((torch.int32, -1), (torch.int32, INT32_MAX), (torch.int64, 2 ** 40)):
        wide = np.full((len(seqs), 2 * L), pad, np.int64)
        for i, s in enumerate(seqs):
            wide[i, 0:2 * len(s):2] = s
        view = dev(wide, dtype)[:, ::2]
        assert view.stride(1) == 2
        got = enc.decode_device(view, lengths=[len(s) for s in seqs], to_host=True)
        assert enc.last_stats["filter"] == "device"
        assert_codes(got, want, f"2-D {dtype} {pad}")
    full = np.stack([ids3[:64], ids3[64:128]])
    assert_codes(enc.decode_device(dev(full), to_host=True), enc.decode_ids(list(full)), "2-D full rows")
    # nothing at all
    codes, frames = enc.decode_device(dev(empty), [0])
    assert tuple(codes.shape) == (0, 8, 0) and frames.size == 0
    codes, frames = enc.decode_device(dev(empty), [0, 0, 0])
    assert tuple(codes.shape) == (2, 8, 0) and frames.tolist() == [0, 0]


def test_a_bad_id_is_a_value_error_and_the_model_stays_usable():
    need_gpu()
    enc = cases.hand_encoder(8, seed=6)
    rng = np.random.default_rng(6)
    good = noisy_cycle(enc, rng, 3 * TILE, 0.1)
    want = enc.decode_ids([good])
    for bad in (-1, enc.n_tokens, INT32_MAX, -2 ** 31):
        ids = good.copy()
        ids[TILE + 17] = bad
        with pytest.raises(ValueError, match="outside"):
            enc.decode_device(dev(ids), [0, ids.size])
        # the same id past the end of the last sequence is never read
        assert_codes(enc.decode_device(dev(ids), [0, TILE + 17], to_host=True), enc.decode_ids([good[:TILE + 17]]), bad)
        assert_codes(run(enc, [good]), want, "after a bad id")
    with pytest.raises(ValueError, match="outside"):
        enc.decode_device(dev(np.array([2 ** 32 + 5], np.int64), torch.int64))  # not narrowed into range


def test_write_keeps_the_padding_and_checks_its_plan():
    need_gpu()
    enc = cases.hand_encoder(8, seed=7)
    rng = np.random.default_rng(7)
    seqs = [noisy_cycle(enc, rng, n, 0.1) for n in (400, 0, 90, 1000)]
    want = enc.decode_ids(seqs)
    t_max = max(w.shape[1] for w in want)
    out = torch.full((5, 9, t_max + 3), -7, dtype=torch.int32, device="cuda:0")
    codes, frames = enc.decode_device(dev(flat_of(seqs)), offsets_of(seqs), out=out)
    assert tuple(codes.shape) == (4, 8, t_max) and codes.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    written = np.zeros(host.shape, bool)
    for i, w in enumerate(want):
        assert np.array_equal(host[i, :8, :w.shape[1]], w)
        written[i, :8, :w.shape[1]] = True
    assert (host[~written] == -7).all()  # rows past a sequence's frames, the ninth row, the fifth item
    # the C ABI: a plan may be written twice; too few frames per row launch nothing; any other call drops the plan
    lib, h = enc._lib, enc._decode_model()
    ptr = ctypes.c_void_p(out.data_ptr())
    out.fill_(-9)
    assert lib.mimi_bpe_decode_write(h, ptr, out.stride(0), out.stride(1), t_max, None) == 0
    assert np.array_equal(out.cpu().numpy()[written], host[written])
    out.fill_(-9)
    assert lib.mimi_bpe_decode_write(h, ptr, out.stride(0), out.stride(1), t_max - 1, None) == 1
    assert b"max_frames" in lib.mimi_last_error()
    torch.cuda.synchronize()
    assert (out == -9).all()
    enc.encode_words([np.array([enc.n_special, enc.n_special + 1], np.int32)])
    assert lib.mimi_bpe_decode_write(h, ptr, out.stride(0), out.stride(1), t_max, None) == 7
    assert b"no plan" in lib.mimi_last_error()
    with pytest.raises(ValueError, match="frames per row"):
        enc.decode_device(dev(flat_of(seqs)), offsets_of(seqs), out=out[:, :, :t_max - 1])
    fresh = cases.hand_encoder(8, seed=7)
    assert lib.mimi_bpe_decode_write(fresh._decode_model(), ptr, out.stride(0), out.stride(1), t_max, None) == 7
    torch.cuda.synchronize()
    assert (out == -9).all()


# ---- round trip and end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k8_recipe", "k2_unlimited"])
def test_round_trip_on_the_device(case):
    need_gpu()
    enc = cases.trained_encoder(case)
    K = enc.num_codebooks
    _, arrays = enc_cases.fixture()
    utt = arrays[f"{case}_cps3"].astype(np.int64).reshape(-1, K).T - OFFSET - CBS * np.arange(K)[:, None]
    items = [utt, utt[:, 10:11], utt[:, 50:180]]
    batch = np.zeros((3, K, utt.shape[1]), np.int64)
    for i, c in enumerate(items):
        batch[i, :, :c.shape[1]] = c
    lens = [c.shape[1] for c in items]
    encoded = enc.encode_device(dev(batch), lengths=lens, chunk_frames=100)
    want = enc.decode_ids(enc.encode_codes([c[:, f:f + 100] for c in items for f in range(0, c.shape[1], 100)]))
    got = enc.decode_device(*encoded[:2], to_host=True)
    assert enc.last_stats["filter"] == "device"
    assert_codes(got, want, case)
    # frames of kept starters only come back as they went in
    plain = enc._chars.cls.reshape(K, CBS) == bpe.KEEP_STARTER
    stable = utt[:, plain[np.arange(K)[:, None], utt].all(axis=0)]
    assert stable.shape[1] >= 20
    got = enc.decode_device(*enc.encode_device(dev(stable))[:2], to_host=True)
    assert_codes(got, [stable], case + " stable")


def test_ids_to_audio_equals_strs_to_audio_of_the_decoded_strings(state_dict):
    need_gpu()
    from mimi_hip import codes_to_chars, strs_to_audio
    from mimi_hip.codes import ids_to_audio
    from mimi_hip.model import MimiHipModel
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    enc = cases.trained_encoder("k8_recipe")
    rng = np.random.default_rng(8)
    stray = np.array([0, enc.n_special + 3 * CBS + 9], np.int32)  # a special id and a misplaced character
    seqs = []
    for T in (1, 0, 7, 40, 13, 22):
        ids = alphabet_ids(enc, np.arange(8 * T) % 8, rng)
        seqs.append(np.insert(ids, [ids.size // 2] * 2, stray) if T else np.zeros(2, np.int32))
    want_codes = enc.decode_ids(seqs)
    assert [c.shape[1] for c in want_codes] == [1, 0, 7, 40, 13, 22]
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    try:
        strs = [codes_to_chars(c, codebook_size=CBS) for c in want_codes]
        for kw in ({}, {"max_batch_frames": 50}):  # one batch; then two: [1, 7, 40] around the empty one | [13, 22]
            want = strs_to_audio(strs, m, "cuda:0", **kw)
            got = ids_to_audio(dev(flat_of(seqs)), offsets_of(seqs), enc, m, **kw)
            assert len(got) == 6
            for g, w in zip(got, want):
                assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == w.shape
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert got[1].shape == (1, 0) and got[3].shape == (1, 1920 * 40)
    finally:
        m.close()
