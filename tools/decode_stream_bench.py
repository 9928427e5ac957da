"""A decode stream's step beside what it replaces, measured in one run (a measurement tool, not a target).

    python tools/decode_stream_bench.py [--k 8] [--reps 3] [--span 48] [--out FILE] [--json-out FILE]

One MI355X, HIP events, a warm-up pass and then ``--reps`` timed passes per shape.  Reports, in ms per step and in
audio-seconds per second (one frame = 0.08 s of audio, per item):

* a stream's step at n = 1, 2, 4 and 12 frames per step, for B = 1 and B = 8, in three bands of ``--span`` frames that
  start at frame 50 (before the 125-frame window fills), at frame 150 and at frame 400 (well past it).  A pass runs a
  fresh stream from frame 0 through the last band; only the bands are timed (events around each band, read after the
  pass; a step synchronises its stream once, to read the bounds flag, so this is wall time per step);
* from the one-shot code paths, in the same run: ``decode`` of the same total frames at once, and the loop streaming
  replaces -- at every step decode again the last 10 s of context (125 frames, fewer before the window fills) and
  keep the tail;
* the per-stage table of one profiled 1-frame step at B = 1 past the window (where a step's time goes).

Seeded synthetic weights (``synthetic:0``), random codes.  A single run on a shared box: other people's work shares
the host, so read differences of a few per cent as noise.
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
BANDS = (50, 150, 400)
WINDOW_FRAMES = 125


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
    return a.elapsed_time(b) / steps


def stream_pass(st, codes, out, n, span, timed):
    """One fresh run from frame 0 through the last band; {band: (ms, steps)} when timed."""
    st.reset()
    marks = []
    end = BANDS[-1] + span
    pos, band = 0, 0
    while pos < end:
        if band < len(BANDS) and pos >= BANDS[band]:
            steps = -(-span // n)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                st.step(codes, out=out)
            b.record()
            marks.append((BANDS[band], a, b, steps))
            pos += steps * n
            band += 1
        else:
            st.step(codes, out=out)
            pos += n
    torch.cuda.synchronize()
    return {bd: (a.elapsed_time(b), steps) for bd, a, b, steps in marks} if timed else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--span", type=int, default=48, help="frames timed per band")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--step-frames", type=int, nargs="+", default=[1, 2, 4, 12])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_stream_bench needs a HIP device: nothing is measured without one")

    from mimi_hip import synthetic
    from mimi_hip.model import MimiHipModel

    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    m = MimiHipModel(sd, device="cuda:0", decode=True)
    K = a.k
    rng = np.random.default_rng(0)
    total = BANDS[-1] + a.span
    res = {"k": K, "reps": a.reps, "span_frames": a.span, "bands_start_frame": list(BANDS), "total_frames": total,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "note": "single run on a shared box", "stream": [], "one_shot": [], "redecode_loop": []}
    lines = [f"decode stream bench: K = {K}, bands of {a.span} frames from frames {BANDS}, warm-up pass + {a.reps} timed "
             f"passes   [{res['date']}, {res['device']}; single run on a shared box]", ""]

    lines.append("a stream's step (ms per step | audio-s per s, all items):")
    lines.append(f"  {'B':>2} {'n':>3} {'state MiB':>10} " + " ".join(f"{'frame ' + str(b):>22}" for b in BANDS))
    for B in a.batches:
        for n in a.step_frames:
            codes = torch.from_numpy(rng.integers(0, 2048, (B, K, n)).astype(np.int32)).cuda()
            out = torch.empty((B, 1, 1920 * n), dtype=torch.float32, device="cuda:0")
            with m.decode_stream(batch=B, num_quantizers=K, max_step_frames=n) as st:
                stream_pass(st, codes, out, n, a.span, False)
                acc = {b: [0.0, 0] for b in BANDS}
                for _ in range(a.reps):
                    for b, (ms, steps) in stream_pass(st, codes, out, n, a.span, True).items():
                        acc[b][0] += ms
                        acc[b][1] += steps
                rec = {"batch": B, "step_frames": n, "state_bytes": st.state_bytes, "bands": {}}
            cells = []
            for b in BANDS:
                ms = acc[b][0] / acc[b][1]
                rate = B * n * FRAME_S / (ms * 1e-3)
                rec["bands"][str(b)] = {"ms_per_step": ms, "audio_s_per_s": rate, "steps_timed": acc[b][1]}
                cells.append(f"{ms:9.3f} ms {rate:9.1f}")
            res["stream"].append(rec)
            lines.append(f"  {B:>2} {n:>3} {rec['state_bytes'] / 2 ** 20:>10.2f} " + " ".join(f"{c:>22}" for c in cells))
    lines.append("")

    lines.append("the one-shot paths, same run:")
    for B in a.batches:
        codes = torch.from_numpy(rng.integers(0, 2048, (B, K, total)).astype(np.int32)).cuda()
        ms = event_timed(lambda: m.decode(codes), 10, 3)
        res["one_shot"].append({"batch": B, "frames": total, "ms": ms, "audio_s_per_s": B * total * FRAME_S / (ms * 1e-3)})
        lines.append(f"  decode of all {total} frames at once, B = {B}: {ms:9.3f} ms  "
                     f"{B * total * FRAME_S / (ms * 1e-3):10.1f} audio-s/s")
    lines.append("  the loop streaming replaces -- decode the last 10 s again at every step, keep the tail (ms per step | "
                 "audio-s per s):")
    for B in a.batches:
        for n in a.step_frames:
            cells = []
            for b in (50, 400):
                T = min(b + n, WINDOW_FRAMES)
                codes = torch.from_numpy(rng.integers(0, 2048, (B, K, T)).astype(np.int32)).cuda()
                ms = event_timed(lambda: m.decode(codes).audio_values[..., -1920 * n:], 10, 3)
                rate = B * n * FRAME_S / (ms * 1e-3)
                res["redecode_loop"].append({"batch": B, "step_frames": n, "at_frame": b, "context_frames": T,
                                             "ms_per_step": ms, "audio_s_per_s": rate})
                cells.append(f"frame {b}: {ms:9.3f} ms {rate:9.1f}")
            lines.append(f"    B = {B}, n = {n:>2}:  " + "   ".join(cells))
    lines.append("")

    # where a step's time goes: one profiled 1-frame step at B = 1 past the window
    codes = torch.from_numpy(rng.integers(0, 2048, (1, K, 1)).astype(np.int32)).cuda()
    with m.decode_stream(batch=1, num_quantizers=K, max_step_frames=1) as st:
        for _ in range(BANDS[-1]):
            st.step(codes)
        m.set_profiling(1)
        m.profile_reset()
        for _ in range(10):
            st.step(codes)
        prof = m.profile_read()
        m.set_profiling(0)
    agg = {}
    for k, v in prof.items():
        s = k.split("#")[0]
        e = agg.setdefault(s, {"ms": 0.0, "launches": 0, "kernel": v["kernel"]})
        e["ms"] += v["ms"] / 10
        e["launches"] += v["launches"] // 10
    res["step_stages_b1_n1"] = agg
    lines.append(f"per stage, one 1-frame step at B = 1 past the window (profiling on: events between every launch; "
                 f"{sum(v['launches'] for v in agg.values())} launches, {sum(v['ms'] for v in agg.values()):.3f} ms in all):")
    for s, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        lines.append(f"    {s:18s} {v['ms']:8.4f} ms  {v['launches']:3d} launches  {v['kernel']}")
    lines.append("")

    # what the write-up must show
    by = {(r["batch"], r["step_frames"]): r["bands"] for r in res["stream"]}
    grow = max(by[k]["400"]["ms_per_step"] / by[k]["150"]["ms_per_step"] for k in by)
    res["worst_frame400_over_frame150"] = grow
    lines.append(f"a step past the window does not grow with the position: frame 400 / frame 150 time, worst shape: {grow:.3f}")
    if (1, 1) in by:
        ms = by[(1, 1)]["400"]["ms_per_step"]
        res["b1_n1_ms_vs_80ms_of_audio"] = ms
        lines.append(f"a 1-frame step at B = 1 takes {ms:.3f} ms for the 80 ms of audio it produces "
                     f"({'real time with ' + format(80.0 / ms, '.1f') + ' x to spare' if ms < 80 else 'SLOWER THAN REAL TIME'})")
    m.close()
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
