"""A ragged step of a decode stream and of an encode stream -- every session its own number of frames -- beside the
grouped-by-count slot steps a caller had to run before and beside the lock-step step at the largest count, measured in
one run (a measurement tool, not a target).

    python tools/stream_ragged_bench.py [--k 8] [--m 8] [--reps 5] [--span 48] [--seed 0] [--out FILE] [--json-out FILE]

One MI355X, HIP events, a warm-up pass and then ``--reps`` timed passes of ``--span`` ticks, the three ways taking turns
pass by pass so that drift of the box hits them alike.  ``--m`` sessions, every one 256 frames in (the window of 250
rows is full), counts drawn once from {1, 2, 4} with ``--seed``; per tick, in ms and in audio-seconds per second (one
frame = 0.08 s of audio):

  (a) one ``step(x, slots=..., frames=counts)`` on a ``batch = m`` stream;
  (b) one ``step(x, slots=group)`` per distinct count, over the slots that bring it: the calls a caller ran before
      a step took a count per slot -- the yardstick;
  (c) the lock-step ``step(x)`` of a ``batch = m`` stream at the largest count: the floor (it decodes more frames
      than (a) and (b) do; its audio rate counts the frames the sessions asked for).

A call synchronises its stream once, to read the bounds flag, so this is wall time per tick.  Seeded synthetic weights
(``synthetic:0``), random codes / speech-like audio.  Both directions, one after the other.  A single run on a shared
box: other people's work shares the host, so read the spread over the passes (printed as min .. max) before
reading a difference.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAME_S = 1920 / 24000.0
BASE = 256  # frames every session has behind it before anything is timed
COUNTS = (1, 2, 4)


def timed_pass(call, span):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(span):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / span


def stage_profile(model, call, reps=10):
    model.set_profiling(1)
    model.profile_reset()
    for _ in range(reps):
        call()
    prof = model.profile_read()
    model.set_profiling(0)
    agg = {}
    for k, v in prof.items():
        e = agg.setdefault(k.split("#")[0], {"ms": 0.0, "launches": 0, "kernel": v["kernel"]})
        e["ms"] += v["ms"] / reps
        e["launches"] += v["launches"] // reps
    return agg


def measure(model, direction, a, counts, rng):
    """One direction: (report lines, result record)."""
    from mimi_hip import synthetic
    K, M = a.k, a.m
    nmax = max(counts)
    groups = {c: [i for i in range(M) if counts[i] == c] for c in sorted(set(counts))}
    frames_asked = sum(counts)
    slots = list(range(M))
    if direction == "decode":
        x = torch.from_numpy(rng.integers(0, 2048, (M, K, nmax)).astype(np.int32)).cuda()
        grouped = {c: x[g][:, :, :c].contiguous() for c, g in groups.items()}
        out = torch.empty((M, 1, 1920 * nmax), dtype=torch.float32, device="cuda:0")
        outs = {c: torch.empty((len(g), 1, 1920 * c), dtype=torch.float32, device="cuda:0") for c, g in groups.items()}
        make = model.decode_stream
    else:
        x = torch.from_numpy(np.stack([synthetic.speech_like(1920 * nmax, 3, i) for i in range(M)])).cuda()
        grouped = {c: x[g][:, :1920 * c].contiguous() for c, g in groups.items()}
        out = torch.empty((M, K, nmax), dtype=torch.int32, device="cuda:0")
        outs = {c: torch.empty((len(g), K, c), dtype=torch.int32, device="cuda:0") for c, g in groups.items()}
        make = model.encode_stream
    streams = {key: make(batch=M, num_quantizers=K, max_step_frames=nmax) for key in "abc"}
    for st in streams.values():
        for _ in range(BASE // nmax):
            st.step(x, out=out)
        assert st.positions == [BASE // nmax * nmax] * M

    def ragged():
        streams["a"].step(x, out=out, slots=slots, frames=counts)

    def by_count():
        for c, g in groups.items():
            streams["b"].step(grouped[c], out=outs[c], slots=g)

    def lock_step():
        streams["c"].step(x, out=out)

    ways = (("a", f"one ragged step, counts {counts}", ragged),
            ("b", f"{len(groups)} slot steps, one per count {sorted(groups)}", by_count),
            ("c", f"lock-step step at n = {nmax}, batch = {M}", lock_step))
    for _, _, call in ways:
        timed_pass(call, a.span)
    ms = {key: [] for key, _, _ in ways}
    for _ in range(a.reps):
        for key, _, call in ways:
            ms[key].append(timed_pass(call, a.span))
    res = {"direction": direction, "ways": {}}
    lines = [f"{direction}: ms per tick: mean (min .. max over the passes) | audio-s per s, all sessions"]
    for key, name, _ in ways:
        mean = sum(ms[key]) / len(ms[key])
        rate = frames_asked * FRAME_S / (mean * 1e-3)
        res["ways"][key] = {"name": name, "ms_per_tick": mean, "ms_min": min(ms[key]), "ms_max": max(ms[key]),
                            "passes": ms[key], "audio_s_per_s": rate}
        lines.append(f"  ({key}) {name:<58} {mean:8.3f} ms ({min(ms[key]):.3f} .. {max(ms[key]):.3f}) {rate:9.1f}")
    w = res["ways"]
    res["b_over_a"] = w["b"]["ms_per_tick"] / w["a"]["ms_per_tick"]
    res["a_over_c"] = w["a"]["ms_per_tick"] / w["c"]["ms_per_tick"]
    res["spread"] = max((w[k]["ms_max"] - w[k]["ms_min"]) / w[k]["ms_per_tick"] for k in "abc")
    lines.append(f"  (b) / (a) = {res['b_over_a']:.2f};   (a) / (c) = {res['a_over_c']:.3f}   (pass-to-pass spread: up to "
                 f"{100 * res['spread']:.1f} %)")
    lines.append("")

    # where the time goes: one profiled tick each way (events between every launch)
    stages = {"a": stage_profile(model, ragged), "b": stage_profile(model, by_count),
              "c": stage_profile(model, lock_step)}
    res["stages"] = stages
    lines.append("per stage, one tick, profiling on (events between every launch): " + ", ".join(
        f"({k}) {sum(v['launches'] for v in stages[k].values())} launches "
        f"{sum(v['ms'] for v in stages[k].values()):.3f} ms" for k in "abc"))
    for s, v in sorted(stages["a"].items(), key=lambda kv: -kv[1]["ms"]):
        b, c = stages["b"].get(s, {"ms": float("nan")}), stages["c"].get(s, {"ms": float("nan")})
        lines.append(f"    {s:18s} (a) {v['ms']:8.4f} ms  (b) {b['ms']:8.4f} ms  (c) {c['ms']:8.4f} ms  {v['launches']:3d} "
                     f"launches  {v['kernel']}")
    lines.append("")
    for st in streams.values():
        st.close()
    return lines, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--m", type=int, default=8, help="sessions")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--span", type=int, default=48, help="ticks timed per pass")
    ap.add_argument("--seed", type=int, default=0, help="of the counts")
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_ragged_bench needs a HIP device: nothing is measured without one")

    from mimi_hip import synthetic
    from mimi_hip.model import MimiHipModel

    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    model = MimiHipModel(sd, device="cuda:0", decode=True)
    rng = np.random.default_rng(a.seed)
    counts = [int(c) for c in rng.choice(COUNTS, size=a.m)]
    res = {"k": a.k, "sessions": a.m, "counts": counts, "reps": a.reps, "span_ticks": a.span, "base_frames": BASE,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "note": "single run on a shared box", "directions": {}}
    lines = [f"stream ragged bench: K = {a.k}, m = {a.m} sessions {BASE} frames in, counts {counts} (seed {a.seed}), "
             f"warm-up pass + {a.reps} timed passes of {a.span} ticks   [{res['date']}, {res['device']}; single run on a "
             f"shared box]", ""]
    for direction in ("decode", "encode"):
        part, rec = measure(model, direction, a, counts, rng)
        lines += part
        res["directions"][direction] = rec
    model.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    print(json.dumps(res))
    for path, body in ((a.out, text), (a.json_out, json.dumps(res) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)


if __name__ == "__main__":
    main()
