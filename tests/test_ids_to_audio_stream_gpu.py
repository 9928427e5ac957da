"""``codes.IdsToAudioStream`` on the GPU: token ids a few at a time per slot -> samples.  The oracle for bits is a fresh
``batch = 1`` ``DecodeStream`` on the same engine stepped over ``Encoder.decode_ids`` of everything the session was
fed -- never the id stream's kernel."""
import numpy as np
import pytest
import torch

import bpe_decode_cases as cases
import bpe_decode_stream_ref as ref
from mimi_hip import codes as codes_mod
from mimi_hip import synthetic

pytestmark = pytest.mark.gpu

FRAME, K, CBS, BATCH = 1920, 8, 2048, 3


@pytest.fixture(scope="module")
def dec(state_dict):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mimi_hip.model import MimiHipModel
    sd = dict(state_dict)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    yield m
    m.close()


def solo(m, codes, max_step_frames=7):
    """[K, T] codes through a fresh batch = 1 decode stream: float32 [1920 T] on the host."""
    out = [torch.zeros(0)]
    with m.decode_stream(batch=1, num_quantizers=K, max_step_frames=max_step_frames) as st:
        for at in range(0, codes.shape[1], max_step_frames):
            out.append(st.step(torch.from_numpy(codes[None, :, at:at + max_step_frames])).cpu().reshape(-1))
    return torch.cat(out)


def session(enc, rng, frames, phase, learned):
    """Ids of about `frames` frames that start on codebook `phase`, some specials and stray ids among them."""
    ids = ref.cycling_ids(enc, rng, 8 * frames + 5, phase) if learned else \
        (enc.n_special + ((phase + np.arange(8 * frames + 5)) % K) * CBS + rng.integers(0, CBS, 8 * frames + 5)).astype(np.int32)
    where = rng.integers(3, len(ids), size=3)
    ids[where] = cases.random_ids(enc, rng, 3, special=0.5)
    return ids


@pytest.mark.parametrize("model", ("k8_recipe", "hand"))
def test_staggered_sessions_equal_solo_streams(dec, model):
    enc = cases.trained_encoder(model) if model == "k8_recipe" else cases.hand_encoder(8, cbs=CBS)
    rng = np.random.default_rng(11)
    ids = {n: session(enc, rng, f, p, model == "k8_recipe") for n, f, p in (("a", 9, 0), ("b", 20, 5), ("c", 18, 2), ("d", 12, 7))}
    start = {"a": 0, "b": 2, "c": 5}                    # the step a session starts at; d takes a's slot after its reset
    slot_of = {"a": 0, "b": 2, "c": 1, "d": 0}
    at = {n: 0 for n in ids}
    parts = {n: [] for n in ids}
    emitted = {n: 0 for n in ids}
    with codes_mod.IdsToAudioStream(enc, dec, BATCH, 3, max_step_frames=2) as st:
        assert st.positions == [0, 0, 0]
        i, reset_done = 0, False
        while any(at[n] < len(ids[n]) for n in ids):
            if at["a"] == len(ids["a"]) and not reset_done:
                st.reset(0)
                reset_done, start["d"] = True, i
                assert st.positions[0] == 0 and st.pending[0] == -1
            live = [n for n in ids if n in start and start[n] <= i and at[n] < len(ids[n])]
            live = live[i % len(live):] + live[:i % len(live)]  # item order rotates: not slot order
            take = [int(rng.integers(1, 4)) for _ in live]
            chunks = [ids[n][at[n]:at[n] + t] for n, t in zip(live, take)]
            padded, counts = ref.pad_ids(chunks, fill=-1)
            audio = st.step(torch.from_numpy(padded).cuda(), slots=[slot_of[n] for n in live], counts=counts)
            for n, c, y, f in zip(live, counts, audio, st.last_frames):
                assert y.dtype == torch.float32 and tuple(y.shape) == (FRAME * f,)
                at[n] += c
                emitted[n] += f
                parts[n].append(y.cpu())
            pos = st.positions
            for n in live:
                assert pos[slot_of[n]] == emitted[n], (i, n)
            i += 1
    for n in ids:
        want_codes = enc.decode_ids([ids[n]])[0]
        assert want_codes.shape[1] >= 5 and emitted[n] == want_codes.shape[1], n
        got = torch.cat(parts[n])
        want = solo(dec, want_codes)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), n


def test_a_step_of_more_frames_than_a_window(dec):
    enc, chain = ref.frame_chain_encoder(8, cbs=CBS, doublings=2)  # the id spells 32 characters: 4 frames
    rng = np.random.default_rng(12)
    cyc = lambda n, phase=0: (enc.n_special + ((phase + np.arange(n)) % K) * CBS + rng.integers(0, CBS, n)).astype(np.int32)
    a = np.concatenate([cyc(3), [chain], cyc(2)]).astype(np.int32)   # 3 pending, then 4 frames in one id
    b = np.concatenate([cyc(6), cyc(3, 6), cyc(2, 1)]).astype(np.int32)
    with codes_mod.IdsToAudioStream(enc, dec, BATCH, 3, max_step_frames=2) as st:
        first = st.step(torch.from_numpy(np.stack([b[:3], a[:3]])).cuda(), slots=[2, 0])
        assert st.last_frames == [0, 0] and all(y.numel() == 0 for y in first)
        first = st.step(torch.from_numpy(np.stack([b[3:6], b[3:6]])).cuda(), slots=[2, 1], counts=[3, 0])
        assert st.last_frames == [0, 0] and st.pending == [3, -1, 6]
        # slot 0 completes 4 frames (two windows), slot 2 one frame (the first window only), slot 1 none
        ids = np.stack([a[3:6], np.zeros(3, np.int32), b[6:9]])
        y0, y1, y2 = st.step(torch.from_numpy(ids).cuda(), slots=[0, 1, 2], counts=[3, 1, 3])
        assert st.last_frames == [4, 0, 1] and st.positions == [4, 0, 1]
        assert tuple(y0.shape) == (4 * FRAME,) and y1.numel() == 0 and tuple(y2.shape) == (FRAME,)
    for y, ids in ((y0, a), (y2, b[:9])):
        want = solo(dec, enc.decode_ids([ids])[0], max_step_frames=2)
        assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32))


def test_mismatched_models_are_refused(dec):
    with pytest.raises(ValueError):
        codes_mod.IdsToAudioStream(cases.hand_encoder(8, cbs=4), dec, 2, 3)
    with pytest.raises(ValueError):
        codes_mod.IdsToAudioStream(cases.hand_encoder(8, cbs=CBS), dec, 0, 3)
