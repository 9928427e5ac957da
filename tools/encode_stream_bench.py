"""An encode stream's step beside what it replaces, measured in one run (a measurement tool, not a target).

    python tools/encode_stream_bench.py [--k 8] [--reps 3] [--span 48] [--out FILE] [--json-out FILE]

One MI355X, HIP events, a warm-up pass and then ``--reps`` timed passes per shape; where two ways are compared they
take turns pass by pass.  Reports, in ms per step and in audio-seconds per second (one frame = 0.08 s of audio, per
item):

* a stream's step at n = 1, 2, 4 and 12 frames per step, for B = 1 and B = 8, in three bands of ``--span`` frames that
  start at frame 50 (before the 125-frame window fills), at frame 150 and at frame 400 (well past it).  A pass runs a
  fresh stream from frame 0 through the last band; only the bands are timed (events around each band, read after the
  pass; a step synchronises its stream before it returns, so this is wall time per step);
* the loop streaming replaces, in the same passes: at every step ``encode`` again the last 10 s of context (125 frames,
  fewer before the window fills) in f32 mode and keep the last frames' codes -- after each timed stream pass, 10
  re-encodes at each band's context;
* a slot step over 8 staggered slots (positions 0, 7, 14, ... frames apart) against eight ``batch = 1`` streams stepped
  one after the other, the two taking turns;
* the per-stage table of one profiled 1-frame step at B = 1 past the window (where a step's time goes).

Seeded synthetic weights (``synthetic:0``), synthetic speech-like audio.  A single run on a shared box: other people's
work shares the host, so read differences of a few per cent as noise.
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

FRAME = 1920
FRAME_S = FRAME / 24000.0
BANDS = (50, 150, 400)
WINDOW_FRAMES = 125
LOOP_STEPS = 10  # re-encodes timed per band and pass


def stream_pass(st, audio, out, n, span, timed):
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
                st.step(audio, out=out)
            b.record()
            marks.append((BANDS[band], a, b, steps))
            pos += steps * n
            band += 1
        else:
            st.step(audio, out=out)
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
        sys.exit("encode_stream_bench needs a HIP device: nothing is measured without one")

    from mimi_hip import synthetic
    from mimi_hip.model import MimiHipModel

    m = MimiHipModel(synthetic.make_state_dict(seed=0), device="cuda:0")
    K = a.k
    total = BANDS[-1] + a.span
    res = {"k": K, "reps": a.reps, "span_frames": a.span, "bands_start_frame": list(BANDS), "total_frames": total,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "note": "single run on a shared box", "stream": [], "reencode_loop": [], "slots": {}}
    lines = [f"encode stream bench: K = {K}, bands of {a.span} frames from frames {BANDS}, warm-up pass + {a.reps} timed "
             f"passes   [{res['date']}, {res['device']}; single run on a shared box]", ""]

    def clips(B, frames):
        return torch.from_numpy(np.stack([synthetic.speech_like(FRAME * frames, 3, i) for i in range(B)])).cuda()

    # the stream and the loop it replaces take turns: per timed pass one stream pass, then the re-encode at each band
    # (the engine in f32 mode for the re-encode; a stream step is fp32 whatever the mode)
    saved = m.precision
    m.set_precision("f32")
    lines.append("a stream's step | the loop streaming replaces -- encode the last 10 s again (f32 mode) at every step, keep "
                 "the last frames' codes; the two ways take turns pass by pass (ms per step, audio-s per s over all items):")
    lines.append(f"  {'B':>2} {'n':>3} {'state MiB':>10} " + " ".join(f"{'frame ' + str(b) + ': stream | re-encode':>44}" for b in BANDS))
    try:
        for B in a.batches:
            for n in a.step_frames:
                audio = clips(B, n)
                out = torch.empty((B, K, n), dtype=torch.int32, device="cuda:0")
                ctx = {b: clips(B, min(b + n, WINDOW_FRAMES)) for b in BANDS}

                def reencode(b, steps):
                    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ea.record()
                    for _ in range(steps):
                        m.encode_int32(ctx[b], K)[..., -n:]
                    eb.record()
                    torch.cuda.synchronize()
                    return ea.elapsed_time(eb)

                with m.encode_stream(batch=B, num_quantizers=K, max_step_frames=n) as st:
                    stream_pass(st, audio, out, n, a.span, False)
                    for b in BANDS:
                        reencode(b, 3)
                    acc = {b: [0.0, 0] for b in BANDS}
                    loop = {b: [0.0, 0] for b in BANDS}
                    for _ in range(a.reps):
                        for b, (ms, steps) in stream_pass(st, audio, out, n, a.span, True).items():
                            acc[b][0] += ms
                            acc[b][1] += steps
                        for b in BANDS:
                            loop[b][0] += reencode(b, LOOP_STEPS)
                            loop[b][1] += LOOP_STEPS
                    rec = {"batch": B, "step_frames": n, "state_bytes": st.state_bytes, "bands": {}}
                cells = []
                for b in BANDS:
                    ms = acc[b][0] / acc[b][1]
                    lms = loop[b][0] / loop[b][1]
                    rate = B * n * FRAME_S / (ms * 1e-3)
                    rec["bands"][str(b)] = {"ms_per_step": ms, "audio_s_per_s": rate, "steps_timed": acc[b][1]}
                    res["reencode_loop"].append({"batch": B, "step_frames": n, "at_frame": b,
                                                 "context_frames": min(b + n, WINDOW_FRAMES), "ms_per_step": lms,
                                                 "audio_s_per_s": B * n * FRAME_S / (lms * 1e-3), "steps_timed": loop[b][1]})
                    cells.append(f"{ms:7.3f} ms {rate:7.1f} | {lms:7.3f} ms {B * n * FRAME_S / (lms * 1e-3):7.1f}")
                res["stream"].append(rec)
                lines.append(f"  {B:>2} {n:>3} {rec['state_bytes'] / 2 ** 20:>10.2f} " + " ".join(f"{c:>44}" for c in cells))
    finally:
        m.set_precision(saved)
    lines.append("")

    # a slot step over 8 staggered slots against eight batch = 1 streams, taking turns
    S, n = 8, 1
    audio = clips(S, n)
    out = torch.empty((S, K, n), dtype=torch.int32, device="cuda:0")
    pool = m.encode_stream(batch=S, num_quantizers=K, max_step_frames=7)
    solos = [m.encode_stream(batch=1, num_quantizers=K, max_step_frames=7) for _ in range(S)]
    lead = clips(1, 7)
    for i in range(S):  # slot i starts 7 i frames ahead
        for _ in range(i):
            pool.step(lead, slots=[i])
            solos[i].step(lead)
    t_pool = t_solo = 0.0
    steps = a.span
    for rep in range(a.reps + 1):
        for way in ("pool", "solo"):
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            for _ in range(steps):
                if way == "pool":
                    pool.step(audio, slots=list(range(S)), out=out)
                else:
                    for i in range(S):
                        solos[i].step(audio[i:i + 1], out=out[i:i + 1])
            eb.record()
            torch.cuda.synchronize()
            if rep:  # (the first round is the warm-up)
                if way == "pool":
                    t_pool += ea.elapsed_time(eb)
                else:
                    t_solo += ea.elapsed_time(eb)
    assert pool.positions == [7 * i + (a.reps + 1) * steps for i in range(S)], pool.positions
    pool.close()
    for s in solos:
        s.close()
    ms_pool, ms_solo = t_pool / (a.reps * steps), t_solo / (a.reps * steps)
    res["slots"] = {"slots": S, "step_frames": n, "ms_per_slot_step": ms_pool, "ms_per_round_of_solo_steps": ms_solo}
    lines.append(f"8 sessions at 8 different positions, 1 frame each: one slot step {ms_pool:.3f} ms "
                 f"({S * n * FRAME_S / (ms_pool * 1e-3):.1f} audio-s/s) | eight batch = 1 streams in turn {ms_solo:.3f} ms "
                 f"({S * n * FRAME_S / (ms_solo * 1e-3):.1f} audio-s/s): {ms_solo / ms_pool:.2f} x")
    lines.append("")

    # where a step's time goes: one profiled 1-frame step at B = 1 past the window
    audio = clips(1, 1)
    with m.encode_stream(batch=1, num_quantizers=K, max_step_frames=1) as st:
        for _ in range(BANDS[-1]):
            st.step(audio)
        m.set_profiling(1)
        m.profile_reset()
        for _ in range(10):
            st.step(audio)
        prof = m.profile_read()
        m.set_profiling(0)
    agg = {}
    for k, v in prof.items():
        s = k.split("#")[0]
        e = agg.setdefault(s, {"ms": 0.0, "launches": 0, "kernel": v["kernel"]})
        e["ms"] += v["ms"] / 10
        e["launches"] += v["launches"] // 10
    res["step_stages_b1_n1"] = agg
    lines.append(f"per stage, one 1-frame step at B = 1 past the window (profiling on: events between every stage; "
                 f"{sum(v['launches'] for v in agg.values())} stages, {sum(v['ms'] for v in agg.values()):.3f} ms in all):")
    for s, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        lines.append(f"    {s:18s} {v['ms']:8.4f} ms  {v['launches']:3d} x  {v['kernel']}")
    lines.append("")

    # what the write-up must show
    by = {(r["batch"], r["step_frames"]): r["bands"] for r in res["stream"]}
    grow = max(by[k]["400"]["ms_per_step"] / by[k]["150"]["ms_per_step"] for k in by)
    res["worst_frame400_over_frame150"] = grow
    lines.append(f"a step past the window does not grow with the position: frame 400 / frame 150 time, worst shape: {grow:.3f}")
    if (1, 1) in by:
        ms = by[(1, 1)]["400"]["ms_per_step"]
        res["b1_n1_ms_vs_80ms_of_audio"] = ms
        lines.append(f"a 1-frame step at B = 1 takes {ms:.3f} ms for the 80 ms of audio it consumes "
                     f"({'real time with ' + format(80.0 / ms, '.1f') + ' x to spare' if ms < 80 else 'SLOWER THAN REAL TIME'})")
    loop = {(r["batch"], r["step_frames"], r["at_frame"]): r["ms_per_step"] for r in res["reencode_loop"]}
    for B in a.batches:
        if (B, 1) in by and (B, 1, 400) in loop:
            ratio = loop[(B, 1, 400)] / by[(B, 1)]["400"]["ms_per_step"]
            res[f"reencode_over_stream_b{B}_n1_frame400"] = ratio
            lines.append(f"re-encoding the last 10 s per frame costs {ratio:.2f} x a stream's 1-frame step at B = {B}")
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
