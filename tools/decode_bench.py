"""Decode throughput beside its two yardsticks, measured in one run (a measurement tool, not a target).

    python tools/decode_bench.py [--batch 32] [--frames 125] [--k 8] [--steps 20] [--warmup 5] [--json-out FILE]

Reports, as audio-seconds per second (one frame = 0.08 s of audio):

* the engine's decode of B x T x K codes and of B = 1, HIP-event timed on the device after warm-up (the call
  synchronises its stream once per decode to read the bounds flag; the events bracket the whole loop);
* yardstick 1: ``tests/decode_ref.py`` (the torch-CPU restatement of ``MimiModel.decode``) at B = 1 on
  ``--cpu-threads`` threads -- the reference path;
* yardstick 2: the engine's own ENCODE of the same shape in the GEMM arithmetic decode uses (``set_precision("f32")``),
  since decode is its mirror;
* the per-stage table of one profiled decode (``mimi_profile_read``).

``--ragged`` measures the mixed-length path instead (``ragged_bench``): one fixed mix of 32 lengths decoded as one
ragged batch, as a padded uniform batch and item by item.

Seeded synthetic weights (``synthetic:0``) and codes from the engine's own encode of speech-like clips.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAME_S = 1920 / 24000.0


def event_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps  # ms per call


def ragged_bench(m, a):
    """--ragged: one fixed mixed-length batch (B = 32, K = 8, T_b from default_rng(0).integers(25, 251): 2-20 s) decoded
    three ways in the same run, HIP-event timed after warm-up: (a) one ragged decode; (b) the uniform decode of the
    codes padded to Tmax, then trimmed; (c) the per-item B = 1 loop.  (b) and (c) are the yardsticks."""
    B, K = 32, 8
    lens = [int(t) for t in np.random.default_rng(0).integers(25, 251, B)]
    S, Tmax = sum(lens), max(lens)
    rng = np.random.default_rng(1)
    codes = torch.zeros((B, K, Tmax), dtype=torch.int32)
    for b, T in enumerate(lens):
        codes[b, :, :T] = torch.from_numpy(rng.integers(0, 2048, (K, T)).astype(np.int32))
    codes = codes.cuda()
    items = [codes[b:b + 1, :, :T].contiguous() for b, T in enumerate(lens)]
    out = {"mode": "ragged", "batch": B, "k": K, "lengths": lens, "sum_frames": S, "max_frames": Tmax,
           "fill_ratio": S / (B * Tmax), "audio_s": S * FRAME_S, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "note": "single run on a shared box"}
    buf = torch.empty((B, m.get_decoded_length(Tmax)), dtype=torch.float32, device="cuda:0")

    def padded():
        y = m.decode(codes).audio_values
        return [y[b, :, : 1920 * T] for b, T in enumerate(lens)]

    def loop():
        return [m.decode(c).audio_values[0] for c in items]

    ya = [y.clone() for y in m.decode_ragged(codes, lens, out=buf)]
    yc = loop()
    out["ragged_bitwise_equals_b1_loop"] = all(torch.equal(p, q) for p, q in zip(ya, yc))
    yb = padded()
    out["padded_max_rel_diff_vs_b1_loop"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(yb, yc))
    del ya, yb, yc
    for key, fn in (("ragged", lambda: m.decode_ragged(codes, lens, out=buf)), ("padded_uniform", padded),
                    ("b1_loop", loop)):
        ms = event_timed(fn, a.steps, a.warmup)
        out[key] = {"ms_per_step": ms, "audio_s_per_s": S * FRAME_S / (ms * 1e-3)}
    out["ragged_over_padded_time"] = out["ragged"]["ms_per_step"] / out["padded_uniform"]["ms_per_step"]
    out["workspace_bytes"] = {"ragged": m.decode_ragged_workspace_bytes(lens), "padded_uniform": m.decode_workspace_bytes(B, Tmax)}
    stages = {}
    for key, fn in (("ragged", lambda: m.decode_ragged(codes, lens, out=buf)), ("padded_uniform", lambda: m.decode(codes))):
        m.set_profiling(1)
        m.profile_reset()
        fn()
        prof = m.profile_read()
        m.set_profiling(0)
        stages[key] = {k: {"ms": v["ms"], "launches": v["launches"], "kernel": v["kernel"]} for k, v in prof.items()
                       if k.startswith("dec_")}
    out["stages"] = stages
    print(f"ragged decode mix: B = {B}, K = {K}, sum T = {S}, Tmax = {Tmax}, fill sum T / (B Tmax) = {out['fill_ratio']:.3f}, "
          f"{out['audio_s']:.1f} s of audio   [{out['date']}, {out['device']}; single run on a shared box]")
    for key, label in (("ragged", "(a) ragged decode"), ("padded_uniform", "(b) padded uniform + trim"),
                       ("b1_loop", "(c) B = 1 loop")):
        print(f"  {label:28s} {out[key]['ms_per_step']:9.3f} ms/step  {out[key]['audio_s_per_s']:10.0f} audio-s/s")
    print(f"  (a) / (b) time {out['ragged_over_padded_time']:.3f} (fill ratio {out['fill_ratio']:.3f});  ragged == B = 1 loop "
          f"bitwise: {out['ragged_bitwise_equals_b1_loop']};  workspace {out['workspace_bytes']['ragged'] / 2 ** 30:.2f} vs "
          f"{out['workspace_bytes']['padded_uniform'] / 2 ** 30:.2f} GiB")
    for key in ("ragged", "padded_uniform"):
        print(f"  per-stage, {key}:")
        agg = {}
        for k, v in stages[key].items():
            s = k.split("#")[0]
            agg[s] = agg.get(s, 0.0) + v["ms"]
        for s, msv in sorted(agg.items(), key=lambda kv: -kv[1]):
            print(f"    {s:18s} {msv:8.3f} ms")
    line = json.dumps(out)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")
    if not out["ragged"]["ms_per_step"] < out["b1_loop"]["ms_per_step"]:
        print("WARNING: the ragged decode is not faster than the B = 1 loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="the mixed-length mix: ragged vs padded uniform vs B = 1 loop")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()

    from mimi_hip import synthetic
    from mimi_hip.model import MimiHipModel
    import decode_ref

    B, T, K = a.batch, a.frames, a.k
    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    if a.ragged:
        ragged_bench(m, a)
        m.close()
        return
    L = 1920 * T
    audio = torch.from_numpy(synthetic.clip_batch(B, L, seed=3)).cuda()
    codes = m.encode_int32(audio, K)            # device int32 [B, K, T]
    codes1 = codes[:1].contiguous()
    out = {"batch": B, "frames": T, "k": K, "steps": a.steps, "warmup": a.warmup, "audio_s_per_item": T * FRAME_S,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}

    def rate(ms, items):
        return items * T * FRAME_S / (ms * 1e-3)

    ms = event_timed(lambda: m.decode(codes), a.steps, a.warmup)
    out["decode"] = {"ms_per_step": ms, "audio_s_per_s": rate(ms, B)}
    ms1 = event_timed(lambda: m.decode(codes1), a.steps, a.warmup)
    out["decode_b1"] = {"ms_per_step": ms1, "audio_s_per_s": rate(ms1, 1)}

    # yardstick 2: encode of the same shape in decode's arithmetic (fp32 MFMA), then the default mode for context
    enc = {}
    for mode in ("f32", "f16x3"):
        m.set_precision(mode)
        e_ms = event_timed(lambda: m.encode_int32(audio, K), a.steps, a.warmup)
        e1_ms = event_timed(lambda: m.encode_int32(audio[:1], K), a.steps, a.warmup)
        enc[mode] = {"ms_per_step": e_ms, "audio_s_per_s": rate(e_ms, B), "b1_ms_per_step": e1_ms,
                     "b1_audio_s_per_s": rate(e1_ms, 1)}
    out["encode_same_shape"] = enc

    # per-stage table of one profiled decode
    m.set_profiling(1)
    m.profile_reset()
    m.decode(codes)
    prof = m.profile_read()
    m.set_profiling(0)
    out["stages"] = {k: {"ms": v["ms"], "launches": v["launches"], "kernel": v["kernel"],
                         "gflops": v["flops"] / (v["ms"] * 1e6) if v["ms"] > 0 else None,
                         "gb_s": v["bytes"] / (v["ms"] * 1e6) if v["ms"] > 0 else None}
                     for k, v in prof.items() if k.startswith("dec_")}

    # yardstick 1: the CPU reference at B = 1
    torch.set_num_threads(a.cpu_threads)
    sdt = decode_ref.as_tensors(sd)
    c1 = codes1.cpu().long()
    decode_ref.decode(c1, sdt)
    t0 = time.perf_counter()
    for _ in range(a.cpu_reps):
        ref = decode_ref.decode(c1, sdt)
    cpu_s = (time.perf_counter() - t0) / a.cpu_reps
    out["cpu_reference_b1"] = {"threads": a.cpu_threads, "s_per_decode": cpu_s, "audio_s_per_s": T * FRAME_S / cpu_s}
    got = m.decode(codes1).audio_values.cpu()
    out["rel_err_vs_cpu_reference"] = float((got - ref).abs().max() / ref.abs().max())
    if out["decode_b1"]["audio_s_per_s"] < out["cpu_reference_b1"]["audio_s_per_s"]:
        out["warning"] = "decode at B = 1 is slower than the CPU reference: something is wrong"

    print(f"decode  B={B:3d}: {out['decode']['ms_per_step']:9.3f} ms/step  {out['decode']['audio_s_per_s']:10.0f} audio-s/s")
    print(f"decode  B=  1: {ms1:9.3f} ms/step  {out['decode_b1']['audio_s_per_s']:10.0f} audio-s/s")
    for mode, v in enc.items():
        print(f"encode {mode:>5} B={B:3d}: {v['ms_per_step']:9.3f} ms/step  {v['audio_s_per_s']:10.0f} audio-s/s;  "
              f"B=1: {v['b1_ms_per_step']:.3f} ms  {v['b1_audio_s_per_s']:.0f} audio-s/s")
    print(f"CPU reference B=1 ({a.cpu_threads} threads): {cpu_s:.3f} s/decode  {out['cpu_reference_b1']['audio_s_per_s']:.1f} "
          f"audio-s/s;  engine vs reference rel err {out['rel_err_vs_cpu_reference']:.2e}")
    for k, v in sorted(out["stages"].items(), key=lambda kv: -kv[1]["ms"]):
        print(f"  {k:18s} {v['ms']:8.3f} ms x{v['launches']:3d}  {v['gflops'] or 0:9.0f} GFLOP/s {v['gb_s'] or 0:8.0f} GB/s  "
              f"{v['kernel'][:70]}")
    line = json.dumps(out)
    print(line)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
