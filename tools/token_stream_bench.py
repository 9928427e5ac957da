"""A step of the id stream (``bpe.IdStream``, bpe_decode_stream.hip) beside what a caller had for the same job before
it, measured in one run (a measurement tool, not a target).

    python tools/token_stream_bench.py [--slots 128] [--reps 7] [--span 64] [--out FILE] [--json-out FILE]

The job: ``--slots`` sessions each receive a few new codec-BPE token ids per step (1 per slot, and 16 per slot), already
in device memory, and the whole frames those ids complete are wanted in device memory.  The model is the committed
recipe-like one (tests/golden, case ``k8_recipe``: K = 8, 2048 codes per codebook, trained with the recipe's settings);
every session's ids spell a stream that cycles through the codebooks, learned ids two times in three.

  (a) ``IdStream.step`` on one stream of ``--slots`` slots: one launch, one synchronisation;
  (b) ``Encoder.decode_device`` re-run over every session's whole id history (all sessions in one call, ``[slots, H]``
      ids), at histories of H = 100 and H = 1000 ids -- the device path there was; its cost grows with the history, the
      caller then still has to slice the new columns out;
  (c) the state machine on the host in Python (the contract class of tests/bpe_decode_stream_ref.py): the new ids
      copied to the host, one ``feed`` per slot, the frames packed and copied back to the device.

Then the share of an ``IdsToAudioStream.step`` (ids -> samples, synthetic decoder weights ``synthetic:0``) that its
id step takes: the same ids through the wrapper and through an ``IdStream`` alone.

Wall time per call (every call ends in a synchronisation of its stream), a warm-up pass and then ``--reps`` timed
passes of ``--span`` calls, the ways taking turns pass by pass so that drift of the box hits them alike.  A single run
on a shared box: other people's work shares the host, so read the spread over the passes (min .. max) before reading a
difference.
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


def timed_pass(call, span):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(span):
        call(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / span * 1e3


def session_ids(enc, slots, per_slot, seed=0):
    """int32 [slots, per_slot]: every row a stream that cycles through the codebooks (one long stream read at a
    different offset per slot)."""
    import bpe_decode_stream_ref as ref
    rng = np.random.default_rng(seed)
    long = ref.cycling_ids(enc, rng, 8 * 4096, phase=0)
    at = (np.arange(slots)[:, None] * 131 + np.arange(per_slot)[None, :]) % len(long)
    return long[at].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--span", type=int, default=64, help="calls timed per pass")
    ap.add_argument("--step-ids", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--histories", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--no-audio", action="store_true", help="skip the IdsToAudioStream part")
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("token_stream_bench needs a HIP device: nothing is measured without one")
    import bpe_decode_cases as cases
    import bpe_decode_stream_ref as ref
    from mimi_hip import codes as codes_mod

    enc = cases.trained_encoder("k8_recipe")
    S, K = a.slots, enc.num_codebooks
    passes = a.reps + 1
    result = {"slots": S, "reps": a.reps, "span": a.span, "device": torch.cuda.get_device_name(0), "rows": []}
    lines = [f"token_stream_bench: {S} slots, model k8_recipe (K = {K}, {enc.n_tokens} tokens), {a.reps} passes of "
             f"{a.span} calls after a warm-up pass, wall ms per call, median (min .. max) over the passes",
             f"device: {result['device']}; a single run on a shared box"]

    def report(name, n, samples, note=""):
        med, lo, hi = float(np.median(samples)), min(samples), max(samples)
        result["rows"].append({"way": name, "ids_per_slot": n, "ms_median": med, "ms_min": lo, "ms_max": hi})
        lines.append(f"  {name:<44} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f}){note}")
        return med

    for n in a.step_ids:
        lines.append(f"-- {n} new id(s) per slot per step")
        steps = passes * a.span
        ids = session_ids(enc, S, steps * n, seed=n)
        dev_ids = torch.from_numpy(ids).cuda().reshape(S, steps, n).permute(1, 0, 2).contiguous()  # [steps, S, n]
        hist = {H: torch.from_numpy(session_ids(enc, S, H, seed=H)).cuda() for H in a.histories}
        stream = enc.decode_stream(S, n)
        pool = ref.PoolRef(enc, S)
        all_slots = list(range(S))
        base = {"v": 0}

        def way_stream(i):
            stream.step(dev_ids[base["v"] + i])

        def way_host(i):
            h = dev_ids[base["v"] + i].cpu().numpy()
            frames = pool.step(all_slots, list(h))
            out = np.zeros((S, K, max(max(f.shape[1] for f in frames), 1)), np.int32)
            for s, f in enumerate(frames):
                out[s, :, :f.shape[1]] = f
            torch.from_numpy(out).cuda()

        ways = [("(a) IdStream.step", way_stream)]
        for H in a.histories:
            ways.append((f"(b) decode_device, history {H} ids", lambda i, H=H: enc.decode_device(hist[H])))
        ways.append(("(c) host state machine in Python", way_host))
        samples = {name: [] for name, _ in ways}
        for p in range(passes):
            base["v"] = p * a.span
            for name, call in ways:
                t = timed_pass(call, a.span)
                if p:
                    samples[name].append(t)
        ref_ms = None
        for name, _ in ways:
            med = report(name, n, samples[name], "" if ref_ms is None else f"   {np.median(samples[name]) / ref_ms:7.1f} x (a)")
            ref_ms = med if ref_ms is None else ref_ms
        stream.close()

    if not a.no_audio:
        from mimi_hip.model import MimiHipModel
        model = MimiHipModel.from_pretrained("synthetic:0", device="cuda:0", decode=True)
        lines.append("-- IdsToAudioStream.step (ids -> samples) and the id step alone on the same ids")
        for n in a.step_ids:
            steps = passes * a.span
            ids = session_ids(enc, S, steps * n, seed=100 + n)
            dev_ids = torch.from_numpy(ids).cuda().reshape(S, steps, n).permute(1, 0, 2).contiguous()
            both = codes_mod.IdsToAudioStream(enc, model, S, n, max_step_frames=max(2, 2 * n))
            alone = enc.decode_stream(S, n)
            base = {"v": 0}
            ways = [(f"IdsToAudioStream.step, {n} id(s) per slot", lambda i: both.step(dev_ids[base["v"] + i])),
                    (f"IdStream.step alone, {n} id(s) per slot", lambda i: alone.step(dev_ids[base["v"] + i]))]
            samples = {name: [] for name, _ in ways}
            for p in range(passes):
                base["v"] = p * a.span
                for name, call in ways:
                    t = timed_pass(call, a.span)
                    if p:
                        samples[name].append(t)
            whole = report(ways[0][0], n, samples[ways[0][0]])
            part = report(ways[1][0], n, samples[ways[1][0]])
            frames = sum(both.positions) / (steps * S)
            lines.append(f"  the id step is {100 * part / whole:.1f} % of the wrapper's step ({frames:.2f} frames per slot "
                         f"per step on average)")
            result["rows"][-1]["share_of_wrapper"] = part / whole
            both.close()
            alone.close()
        model.close()

    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
