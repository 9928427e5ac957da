"""Codec-BPE decoding rate, ids back to codes: ``Encoder.decode_device`` (bpe_decode.hip) against the host rules
``Encoder.decode_ids`` and against HF tokenizers' ``decode_batch`` followed by the same drop rules, on the same ids and
the same box.

The corpus is the one of ``tools/bpe_encode_bench.py`` (its ``corpus`` stage is reused): synthetic utterances U[10, 20] s
encoded by the engine (K = 8), cut into 30 s chunks, a model of up to ``--merges`` merges trained on them; the chunks,
``--repeat`` times over, are encoded by ``encode_device`` and those ids are decoded.

    python tools/bpe_decode_bench.py --out profiles/bpe_decode_bench.txt

Stages, each a child process under its own time limit (a failed stage ends the run): ``corpus`` (GPU: engine encode +
BPE training), ``ids`` (GPU: ``encode_device``, the ids saved), ``device`` (``decode_device`` on the ids uploaded once:
wall time with the codes left on the device, wall time with ``to_host=True``, HIP events around the call; codes
asserted equal to ``decode_ids``' on a sample), ``host`` (``decode_ids``), ``cpu`` (tokenizers ``decode_batch`` with
``--threads`` threads, then ``Encoder.indices_to_codes`` per string: the reference converter's rules as ``decode_ids``
restates them; the reference's own per-character Python loop is not timed here).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bpe_encode_bench as encode_bench  # noqa: E402

K, CBS, FR = encode_bench.K, encode_bench.CBS, encode_bench.FR


def encoder(args):
    from mimi_hip import bpe
    return bpe.Encoder.from_tokenizer(os.path.join(args.work, "tokenizer.json"), K, CBS)


def load_ids(args):
    with np.load(os.path.join(args.work, "decode_ids.npz")) as z:
        return z["ids"], z["offs"]


def stage_ids(args):
    import torch
    chunks = encode_bench.load_chunks(args)
    enc = encoder(args)
    frames = [c.shape[1] for c in chunks]
    padded = np.zeros((len(chunks), K, max(frames)), np.int32)
    for b, c in enumerate(chunks):
        padded[b, :, :c.shape[1]] = c
    ids, offs, _ = enc.encode_device(torch.from_numpy(padded).cuda(), frames)
    np.savez(os.path.join(args.work, "decode_ids.npz"), ids=ids.cpu().numpy(), offs=offs)
    return {"sequences": len(chunks), "tokens": int(offs[-1]), "frames_encoded": int(sum(frames))}


def rates(seconds, tokens, frames):
    return {"seconds": round(seconds, 5), "tokens_per_s": round(tokens / seconds),
            "audio_s_per_s": round(frames / FR / seconds)}


def stage_device(args):
    import torch
    ids, offs = load_ids(args)
    enc = encoder(args)
    dev_ids = torch.from_numpy(ids).cuda()  # uploaded once: a language model's output is already there
    enc.decode_device(dev_ids[:int(offs[8])], offs[:9])  # model and spellings upload
    codes, lens = enc.decode_device(dev_ids, offs)       # buffers
    torch.cuda.synchronize()
    tokens, frames = int(offs[-1]), int(lens.sum())
    wall, wall_host, dev_ms = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        codes, lens = enc.decode_device(dev_ids, offs)
        wall.append(time.perf_counter() - t0)
    stats = dict(enc.last_stats)
    for _ in range(args.runs):
        t0 = time.perf_counter()
        host = enc.decode_device(dev_ids, offs, to_host=True)
        wall_host.append(time.perf_counter() - t0)
    stream = torch.cuda.Stream()
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        enc.decode_device(dev_ids, offs, stream=stream)
        b.record(stream)
        b.synchronize()
        dev_ms.append(a.elapsed_time(b))
    sample = list(range(0, len(lens), max(1, len(lens) // 64)))
    want = enc.decode_ids([ids[offs[i]:offs[i + 1]] for i in sample])
    assert all(np.array_equal(host[i], w) for i, w in zip(sample, want)), "decode_device differs from decode_ids"
    np.save(os.path.join(args.work, "decode_frames.npy"), lens)
    off, _ = enc.spellings()
    return {"sequences": len(lens), "tokens": tokens, "characters": int((off[ids.astype(np.int64) + 1] -
                                                                         off[ids.astype(np.int64)]).sum()),
            "frames": frames, "filter": stats["filter"], "same_codes_as_decode_ids_on": len(sample),
            "wall": dict(rates(min(wall), tokens, frames), all_runs_ms=[round(x * 1e3, 2) for x in wall],
                         what="decode_device, codes left on the device (the call synchronises its stream)"),
            "wall_to_host": dict(rates(min(wall_host), tokens, frames),
                                 all_runs_ms=[round(x * 1e3, 2) for x in wall_host],
                                 what="decode_device(to_host=True): plus the copy out and one numpy array per sequence"),
            "device": dict(rates(min(dev_ms) / 1e3, tokens, frames), all_runs_ms=[round(x, 2) for x in dev_ms],
                           what="HIP events around decode_device on its stream: the output fill, kernels, both "
                                "read-backs")}


def stage_host(args):
    ids, offs = load_ids(args)
    enc = encoder(args)
    seqs = [ids[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    enc.decode_ids(seqs[:8])  # the spelling table
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = enc.decode_ids(seqs)
        times.append(time.perf_counter() - t0)
    frames = sum(c.shape[1] for c in out)
    lens = np.load(os.path.join(args.work, "decode_frames.npy"))
    return dict(rates(min(times), int(offs[-1]), frames), sequences=len(seqs), frames=frames,
                same_frame_counts_as_device=bool(np.array_equal(lens, [c.shape[1] for c in out])),
                all_runs_ms=[round(x * 1e3, 1) for x in times], what="decode_ids: vectorised numpy, one sequence at a time")


def stage_cpu(args):
    os.environ["RAYON_NUM_THREADS"] = str(args.threads)
    os.environ["TOKENIZERS_PARALLELISM"] = "true"
    try:
        import tokenizers
        from tokenizers import Tokenizer
    except ImportError:
        return {"tokenizers": None}
    ids, offs = load_ids(args)
    enc = encoder(args)
    tok = Tokenizer.from_file(os.path.join(args.work, "tokenizer.json"))
    seqs = [ids[offs[i]:offs[i + 1]].tolist() for i in range(len(offs) - 1)]
    t_decode, t_rules = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        strings = tok.decode_batch(seqs, skip_special_tokens=True)
        t1 = time.perf_counter()
        out = [enc.indices_to_codes(np.frombuffer(s.encode("utf-32-le"), dtype="<u4").astype(np.int64) -
                                    enc.unicode_offset) for s in strings]
        t2 = time.perf_counter()
        t_decode.append(t1 - t0)
        t_rules.append(t2 - t1)
    frames = sum(c.shape[1] for c in out)
    lens = np.load(os.path.join(args.work, "decode_frames.npy"))
    best = min(a + b for a, b in zip(t_decode, t_rules))
    return dict(rates(best, int(offs[-1]), frames), tokenizers=tokenizers.__version__, threads=args.threads,
                sequences=len(seqs), frames=frames, decode_batch_s=round(min(t_decode), 4),
                drop_rules_s=round(min(t_rules), 4),
                same_frame_counts_as_device=bool(np.array_equal(lens, [c.shape[1] for c in out])),
                what="tokenizers decode_batch, then the converter's rules as decode_ids restates them (numpy)")


STAGES = {"corpus": (encode_bench.stage_corpus, 420), "ids": (stage_ids, 240), "device": (stage_device, 240),
          "host": (stage_host, 420), "cpu": (stage_cpu, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--merges", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=8, help="the chunks are taken this many times over in one call")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--work", default=os.path.join(ROOT, "bench_out", "bpe_decode"))
    ap.add_argument("--stage", choices=tuple(STAGES) + ("all",), default="all")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    os.makedirs(args.work, exist_ok=True)
    if args.stage != "all":
        print(json.dumps({args.stage: STAGES[args.stage][0](args)}))
        return
    report = {"note": "single run on a shared box", "corpus_like": "tools/bpe_encode_bench.py",
              "settings": {"utts": args.utts, "merges_asked": args.merges, "repeat": args.repeat, "runs": args.runs}}
    for name, (_, limit) in STAGES.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--work", args.work, "--utts",
               str(args.utts), "--merges", str(args.merges), "--repeat", str(args.repeat), "--runs", str(args.runs),
               "--threads", str(args.threads)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            report[name] = {"failed": f"time limit of {limit} s"}
            break
        if r.returncode != 0:
            report[name] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            break
        report.update(json.loads(r.stdout.strip().splitlines()[-1]))
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if any("failed" in v for v in report.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
