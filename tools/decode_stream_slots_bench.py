"""A slot step of a decode stream beside the lock-step step and beside one stream per session, measured in one run (a
measurement tool, not a target).

    python tools/decode_stream_slots_bench.py [--k 8] [--m 8] [--reps 5] [--span 48] [--out FILE] [--json-out FILE]

One MI355X, HIP events, a warm-up pass and then ``--reps`` timed passes of ``--span`` calls per shape, the three ways
taking turns pass by pass so that drift of the box hits them alike.  For n = 1 and n = 4 frames per call and ``--m``
sessions, every session past frame 250 (the window of 250 rows is full), in ms per call and in audio-seconds per
second (one frame = 0.08 s of audio, per session):

  (a) ``step(codes, slots=[0 .. m-1])`` on one ``batch = m`` stream whose slots stand ``--stagger`` frames apart;
  (b) the lock-step ``step(codes)`` of a ``batch = m`` stream -- the path a slot step leaves as it was;
  (c) ``m`` streams of ``batch = 1`` stepped one after another, at the same staggered positions: what a caller with
      sessions that started at different times had to do before.

A call synchronises its stream once, to read the bounds flag, so this is wall time per call.  Seeded synthetic weights
(``synthetic:0``), random codes.  A single run on a shared box: other people's work shares the host, so read the
spread over the passes (printed as min .. max) before reading a difference.
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


def timed_pass(call, span):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(span):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / span


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--m", type=int, default=8, help="sessions")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--span", type=int, default=48, help="calls timed per pass")
    ap.add_argument("--stagger", type=int, default=40, help="frames between neighbouring slots' positions")
    ap.add_argument("--step-frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_stream_slots_bench needs a HIP device: nothing is measured without one")

    from mimi_hip import synthetic
    from mimi_hip.model import MimiHipModel

    sd = synthetic.make_state_dict(seed=0)
    sd.update(synthetic.make_decoder_state_dict(seed=0))
    model = MimiHipModel(sd, device="cuda:0", decode=True)
    K, M = a.k, a.m
    rng = np.random.default_rng(0)
    res = {"k": K, "sessions": M, "reps": a.reps, "span_calls": a.span, "stagger_frames": a.stagger,
           "base_frames": BASE, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "note": "single run on a shared box", "shapes": []}
    lines = [f"decode stream slots bench: K = {K}, m = {M} sessions, slots {a.stagger} frames apart from frame {BASE}, "
             f"warm-up pass + {a.reps} timed passes of {a.span} calls   [{res['date']}, {res['device']}; single run on "
             f"a shared box]", "",
             "ms per call: mean (min .. max over the passes) | audio-s per s, all sessions"]
    for n in a.step_frames:
        assert BASE % n == 0 and a.stagger % n == 0, "frames per call must divide the base and the stagger"
        codes = torch.from_numpy(rng.integers(0, 2048, (M, K, n)).astype(np.int32)).cuda()
        ones = [codes[i:i + 1].contiguous() for i in range(M)]
        out = torch.empty((M, 1, 1920 * n), dtype=torch.float32, device="cuda:0")
        outs = [torch.empty((1, 1, 1920 * n), dtype=torch.float32, device="cuda:0") for _ in range(M)]
        slots = list(range(M))
        pool = model.decode_stream(batch=M, num_quantizers=K, max_step_frames=n)
        lock = model.decode_stream(batch=M, num_quantizers=K, max_step_frames=n)
        singles = [model.decode_stream(batch=1, num_quantizers=K, max_step_frames=n) for _ in range(M)]
        # the positions: slot i at BASE + i * stagger (the pool through slot steps over the slots still behind)
        for _ in range(BASE // n):
            pool.step(codes, out=out)
            lock.step(codes, out=out)
        for i in range(1, M):
            for _ in range(a.stagger // n):
                pool.step(codes[i:], out=out[i:], slots=slots[i:])
        for i, st in enumerate(singles):
            for _ in range((BASE + i * a.stagger) // n):
                st.step(ones[i], out=outs[i])
        assert pool.positions == [BASE + i * a.stagger for i in range(M)], pool.positions
        assert [st.position for st in singles] == pool.positions

        def one_by_one():
            for i, st in enumerate(singles):
                st.step(ones[i], out=outs[i])

        ways = (("a", f"step(slots) over {M} staggered slots", lambda: pool.step(codes, out=out, slots=slots)),
                ("b", f"lock-step step, batch = {M}", lambda: lock.step(codes, out=out)),
                ("c", f"{M} batch = 1 streams, one after another", one_by_one))
        for _, _, call in ways:
            timed_pass(call, a.span)
        ms = {key: [] for key, _, _ in ways}
        for _ in range(a.reps):
            for key, _, call in ways:
                ms[key].append(timed_pass(call, a.span))
        rec = {"step_frames": n, "pool_state_bytes": pool.state_bytes, "ways": {}}
        lines.append(f"n = {n}:")
        for key, name, _ in ways:
            mean = sum(ms[key]) / len(ms[key])
            rate = M * n * FRAME_S / (mean * 1e-3)
            rec["ways"][key] = {"name": name, "ms_per_call": mean, "ms_min": min(ms[key]), "ms_max": max(ms[key]),
                                "passes": ms[key], "audio_s_per_s": rate}
            lines.append(f"  ({key}) {name:<44} {mean:8.3f} ms ({min(ms[key]):.3f} .. {max(ms[key]):.3f}) {rate:9.1f}")
        w = rec["ways"]
        rec["a_over_b"] = w["a"]["ms_per_call"] / w["b"]["ms_per_call"]
        rec["c_over_a"] = w["c"]["ms_per_call"] / w["a"]["ms_per_call"]
        spread = max((w[k]["ms_max"] - w[k]["ms_min"]) / w[k]["ms_per_call"] for k in ("a", "b"))
        rec["spread_ab"] = spread
        lines.append(f"  (a) / (b) = {rec['a_over_b']:.3f}  (pass-to-pass spread of (a), (b): up to {100 * spread:.1f} %);   "
                     f"(c) / (a) = {rec['c_over_a']:.2f}")
        res["shapes"].append(rec)
        for st in [pool, lock] + singles:
            st.close()
    lines.append("")

    # where a slot step's time goes beside a lock-step step: one profiled 1-frame call each, m sessions past the window
    codes = torch.from_numpy(rng.integers(0, 2048, (M, K, 1)).astype(np.int32)).cuda()
    stages = {}
    for key in ("slots", "lock-step"):
        with model.decode_stream(batch=M, num_quantizers=K, max_step_frames=1) as st:
            for _ in range(BASE):
                st.step(codes)
            if key == "slots" and M > 1:
                st.step(codes[1:], slots=list(range(1, M)))
            kw = {"slots": list(range(M))} if key == "slots" else {}
            model.set_profiling(1)
            model.profile_reset()
            for _ in range(10):
                st.step(codes, **kw)
            prof = model.profile_read()
            model.set_profiling(0)
        agg = {}
        for k, v in prof.items():
            e = agg.setdefault(k.split("#")[0], {"ms": 0.0, "launches": 0, "kernel": v["kernel"]})
            e["ms"] += v["ms"] / 10
            e["launches"] += v["launches"] // 10
        stages[key] = agg
    res["step_stages_n1"] = stages
    lines.append(f"per stage, one 1-frame call over {M} sessions past the window, profiling on (events between every "
                 f"launch): slot step {sum(v['launches'] for v in stages['slots'].values())} launches "
                 f"{sum(v['ms'] for v in stages['slots'].values()):.3f} ms, lock-step step "
                 f"{sum(v['launches'] for v in stages['lock-step'].values())} launches "
                 f"{sum(v['ms'] for v in stages['lock-step'].values()):.3f} ms")
    for s, v in sorted(stages["slots"].items(), key=lambda kv: -kv[1]["ms"]):
        o = stages["lock-step"].get(s, {"ms": float("nan")})
        lines.append(f"    {s:18s} slots {v['ms']:8.4f} ms  lock-step {o['ms']:8.4f} ms  {v['launches']:3d} launches  {v['kernel']}")
    lines.append("")
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
