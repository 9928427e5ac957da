"""Codes of fixed synthetic batches from the engine library named by MIMI_HIP_LIB (A/B builds): writes
gpurun_out/<tag>_codes.npz with B = 32 x 10 s (K = 32), a ragged 17-item batch and a batch-1 clip, and every stage tap
(sha-256 of the fp32 values, planes reconstructed) of a B = 32 x 1 s batch (the fused q/k/v + attention path) and a B = 2 x 3 s batch
(the two-kernel path), so builds that must give the same bits can be compared file to file (tools/cmp_codes.py).
Beside them the profiled launch sequence and records of one pass each of the three batches, and the engine's counters
(f16_reruns, rvq_chain_reruns, graph_replays, graph_captures, lane_encodes) with every result of a fixed script on a
fresh engine: three synchronous encodes of one shape (eager, capture, replay), four asynchronous ones kept two in flight,
a ragged batch, the quantizer alone, and a loud clip and a loud pair that take the overflow fallback.

`lib_codes.py <tag> decode` writes the decode path's entries instead: the uniform decode of B = 3 x T = 13 x K = 8 and of
B = 2 x T = 129 x K = 1, the ragged decode of T = [13, 1, 129, 2, 64, 65, 5, 3] at K = 8 (an odd T, 1- to 3-frame items,
both sides of 256 rows and of the 1024-row tile change), the sha-256 of every tap and the profiled launch sequence and
records of one uniform and one ragged pass, and the workspace sizes with taps off and on.

`lib_codes.py <tag> stream` writes the streams' entries: per direction (dec_ / enc_; K = 8, max_step_frames 3, random
codes / 1920 n samples of speech-like audio per item) a batch-2 stream in lock-step steps of n = 1, 2, 3, 1 and a batch-3
stream through slots [0] n = 2, [0, 1] n = 1, [2, 0] n = 3, reset(1), [1, 2] n = 1 and a plain step of n = 1 with the
positions diverged -- every step's result and the positions -- and one more lock-step step and one more slot step with
taps and profiling on: the launch sequence, the records and the sha-256 of a tap of each section of the pass."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tokenize-audio_amd"))
from mimi_hip import synthetic  # noqa: E402
from mimi_hip.model import MimiHipModel  # noqa: E402

tag = sys.argv[1]
out = {}


def tap_sha(m, t):
    a = np.ascontiguousarray(m.get_tap(t))
    return np.array([hashlib.sha256(a.tobytes()).hexdigest() + f" {a.shape}"])


def text(rows):
    return np.array([repr(r) for r in rows])


def profiled(m, name, fn):
    """One pass with per-stage profiling on: the launch sequence and the records (no times: they are not bits)."""
    m.set_profiling(1)
    m.profile_reset()
    fn()
    prof = m.profile_read()
    out[f"{name}_sequence"] = text(m.profile_sequence())
    out[f"{name}_records"] = text((k, v["kernel"], v["launches"], v["flops"], v["bytes"]) for k, v in prof.items())
    m.set_profiling(0)
    m.profile_reset()


def traced(m, name, fn, taps):
    """One pass with taps and profiling on: the sha-256 of the listed taps, the launch sequence and the records."""
    m.set_taps(True)
    m.set_profiling(1)
    m.profile_reset()
    fn()
    prof = m.profile_read()
    out[f"{name}_sequence"] = text(m.profile_sequence())
    out[f"{name}_records"] = text((k, v["kernel"], v["launches"], v["flops"], v["bytes"]) for k, v in prof.items())
    m.set_profiling(0)
    for t in taps:
        out[f"{name}_{t}"] = tap_sha(m, t)
    m.set_taps(False)


def counters_script():
    m = MimiHipModel(synthetic.make_state_dict(seed=0), device="cuda:0")

    def clip(B, L, seed):
        return torch.from_numpy(synthetic.clip_batch(B, L, seed=seed)).cuda()

    x = clip(2, 24000, 510)  # (a small grid: the persistent RVQ chain, also inside the captured graph)
    for i in range(3):
        out[f"script_sync{i}"] = m.encode_int32(x, 8).cpu().numpy()
    fly = []
    for i in range(4):  # (large grids: the per-level RVQ kernels, so both lanes take encodes)
        fly.append(m.encode_async(clip(32, 72000, 520 + i), 8))
        if len(fly) == 2:
            out[f"script_async{i - 1}"] = fly.pop(0).wait().cpu().numpy()
    out["script_async3"] = fly.pop(0).wait().cpu().numpy()
    lens = [48000, 1, 13441, 24000, 30001]
    xr = np.zeros((len(lens), max(lens)), np.float32)
    for i, n in enumerate(lens):
        xr[i, :n] = synthetic.speech_like(n, 530, i)
    out["script_ragged"] = m.encode_ragged(torch.from_numpy(xr).cuda(), lens, 8).cpu().numpy()
    emb = torch.from_numpy(np.random.default_rng(540).standard_normal((1, 512, 13)).astype(np.float32)).cuda()
    out["script_quantize"] = m.quantize(emb, 8).cpu().numpy()
    loud = synthetic.speech_like(48000, 5, 1) * np.float32(3e4)
    out["script_loud"] = m.encode_int32(torch.from_numpy(loud)[None].cuda(), 8).cpu().numpy()
    pair = np.stack([loud, synthetic.speech_like(48000, 5, 2)])
    out["script_loud_pair"] = m.encode_int32(torch.from_numpy(pair).cuda(), 8).cpu().numpy()
    out["script_counters"] = np.array([m.f16_reruns, m.rvq_chain_reruns, m.graph_replays, m.graph_captures,
                                       *m.lane_encodes], dtype=np.int64)
    print(tag, "counters (f16_reruns, rvq_chain_reruns, graph_replays, graph_captures, lane_encodes)",
          out["script_counters"].tolist())
    m.close()


def encode_section():
    m = MimiHipModel(synthetic.make_state_dict(seed=0), device="cuda:0")
    x = torch.from_numpy(synthetic.clip_batch(32, 240000, seed=501)).cuda()
    out["b32"] = m.encode_int32(x, 32).cpu().numpy()
    rng = np.random.default_rng(502)
    lengths = [int(v) for v in rng.integers(1, 300000, 17)]
    clips = [synthetic.speech_like(L, 503, i) for i, L in enumerate(lengths)]
    xr = np.zeros((len(clips), max(lengths)), np.float32)
    for i, c in enumerate(clips):
        xr[i, :len(c)] = c
    xr = torch.from_numpy(xr).cuda()
    out["ragged"] = m.encode_ragged(xr, lengths, 32).cpu().numpy()
    x1 = torch.from_numpy(synthetic.clip_batch(1, 240000, seed=504)).cuda()
    out["b1"] = m.encode_int32(x1, 32).cpu().numpy()
    profiled(m, "b32", lambda: m.encode_int32(x, 32))
    profiled(m, "ragged", lambda: m.encode_ragged(xr, lengths, 32))
    profiled(m, "b1", lambda: m.encode_int32(x1, 32))
    TAPS = (["conv0", "encoder", "ds_gemm", "downsample", "proj"] + [f"res{i}_elu" for i in range(4)] +
            [f"down{i}" for i in range(3)] + ["down3_elu"] +
            [f"{n}{l}" for l in range(8) for n in ("qkv", "att", "oproj", "ff", "xfmr")])
    for name, (B, L, seed) in {"tb32": (32, 24000, 505), "tb2": (2, 72000, 506)}.items():
        m.set_taps(True)
        out[name] = m.encode_int32(torch.from_numpy(synthetic.clip_batch(B, L, seed=seed)).cuda(), 32).cpu().numpy()
        for t in TAPS:
            try:
                out[f"{name}_{t}"] = tap_sha(m, t)
            except Exception:  # (a tap the path does not produce, e.g. q/k/v under the fused attention)
                pass
        m.set_taps(False)
    counters_script()


def decode_section():
    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    LENS = [13, 1, 129, 2, 64, 65, 5, 3]
    TAPS = (["quantized", "upsample", f"xfmr{m.config.num_hidden_layers - 1}", "dconv0", "dconv0_elu"] +
            [f"up{i}" for i in range(4)] + [f"dres{i}_elu" for i in range(4)] + ["audio"])
    rng = np.random.default_rng(601)

    def codes(B, K, T):
        return torch.from_numpy(rng.integers(0, m.config.codebook_size, (B, K, T)).astype(np.int32)).cuda()

    cu, c1, cr = codes(3, 8, 13), codes(2, 1, 129), codes(len(LENS), 8, max(LENS))
    out["u_b3_t13_k8"] = m.decode(cu).audio_values.cpu().numpy()
    out["u_b2_t129_k1"] = m.decode(c1).audio_values.cpu().numpy()
    buf = torch.zeros((len(LENS), m.get_decoded_length(max(LENS))), dtype=torch.float32, device="cuda:0")
    m.decode_ragged(cr, LENS, out=buf)
    out["ragged"] = buf.cpu().numpy()  # (the samples past an item's length stay 0: never written)
    traced(m, "tu", lambda: m.decode(cu), TAPS)
    traced(m, "tr", lambda: m.decode_ragged(cr, LENS), TAPS)
    for taps in (False, True):
        m.set_taps(taps)
        out[f"workspace_taps{int(taps)}"] = np.array(
            [m.decode_workspace_bytes(B, T) for B, T in ((1, 13), (3, 13), (32, 125))] +
            [m.decode_ragged_workspace_bytes(LENS)], dtype=np.int64)
    m.set_taps(False)
    print(tag, "workspace", out["workspace_taps0"].tolist(), out["workspace_taps1"].tolist())


def stream_section():
    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    K, F = 8, 1920
    rng = np.random.default_rng(701)
    clips = iter(range(1 << 20))

    def codes(items, n):
        return torch.from_numpy(rng.integers(0, m.config.codebook_size, (items, K, n)).astype(np.int32)).cuda()

    def audio(items, n):
        return torch.from_numpy(np.stack([synthetic.speech_like(F * n, 702, next(clips)) for _ in range(items)])).cuda()

    # the slot schedule: (slots, n), a reset, then a plain step that finds the positions diverged
    SLOTS = [([0], 2), ([0, 1], 1), ([2, 0], 3), "reset 1", ([1, 2], 1), (None, 1)]
    for d, open_stream, chunk, taps in (
            ("dec", m.decode_stream, codes, ["quantized", "upsample", "qkv0", "att0", "xfmr7", "dres1_elu", "audio"]),
            ("enc", m.encode_stream, audio,
             ["conv0", "res1_elu", "encoder", "qkv0", "att0", "xfmr7", "downsample", "proj"])):
        with open_stream(batch=2, num_quantizers=K, max_step_frames=3) as st:  # lock-step
            for i, n in enumerate((1, 2, 3, 1)):
                out[f"{d}_lock{i}_n{n}"] = st.step(chunk(2, n)).cpu().numpy()
            x = chunk(2, 2)
            traced(m, f"{d}_tlock", lambda: st.step(x), taps)
            out[f"{d}_lock_positions"] = np.array(st.positions, dtype=np.int64)
        with open_stream(batch=3, num_quantizers=K, max_step_frames=3) as st:  # slots
            for i, op in enumerate(SLOTS):
                if op == "reset 1":
                    st.reset(1)
                else:
                    slots, n = op
                    out[f"{d}_slots{i}_n{n}"] = st.step(chunk(3 if slots is None else len(slots), n),
                                                        slots=slots).cpu().numpy()
                out[f"{d}_slots{i}_positions"] = np.array(st.positions, dtype=np.int64)
            x = chunk(2, 2)
            traced(m, f"{d}_tslots", lambda: st.step(x, slots=[2, 0]), taps)
            out[f"{d}_slots_positions"] = np.array(st.positions, dtype=np.int64)
    m.close()


if sys.argv[2:] == ["decode"]:
    decode_section()
elif sys.argv[2:] == ["stream"]:
    stream_section()
else:
    encode_section()
os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
np.savez(os.path.join(ROOT, "gpurun_out", f"{tag}_codes.npz"), **out)
print(tag, {k: v.shape for k, v in out.items()})
