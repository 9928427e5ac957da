"""Codec-BPE encoding rate: the GPU encoder (mimi_hip.bpe.Encoder, bpe_encode.hip) against HF tokenizers'
``encode_batch`` on the same strings and the same box.

The corpus is the one ``bench.py --workload mls --bpe`` trains on: synthetic utterances U[10, 20] s encoded by the
engine (K = 8), cut into 30 s chunks (``codec-bpe/train_bpe_recipe.txt:18-28``), a model of up to ``--merges``
merges trained on them by the GPU trainer; the chunks, ``--repeat`` times over, are then encoded.

    python tools/bpe_encode_bench.py --out profiles/bpe_encode_bench.txt

Four stages, each a child process under its own time limit (a failed stage ends the run): ``corpus`` (GPU: engine
encode + BPE training), ``gpu`` (the encoder with the host word model: HIP events around the device work of
``mimi_bpe_encode``, wall time including the host word preparation), ``device`` (``Encoder.encode_device`` on the same
chunks, uploaded once as one padded int32 tensor: wall time with the ids left on the device, wall time with
``to_host=True``, HIP events around the call; ids asserted equal to the ``gpu`` stage's), ``cpu`` (tokenizers with
``--threads`` threads; ids compared with the GPU's).

    python tools/bpe_encode_bench.py --out profiles/bpe_encode_device_bench.txt

``--stage gpu --work DIR`` runs the encoder stage alone on a saved corpus (e.g. under ``rocprofv3 --kernel-trace
--stats`` for the per-kernel split).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT):
    sys.path.insert(0, p)

K, CBS, FR, CHUNK_S = 8, 2048, 12.5, 30


def stage_corpus(args):
    from mimi_hip import bpe, synthetic
    from mimi_hip.encoder import MimiEncoder
    from mimi_hip.model import MimiHipModel
    model = MimiHipModel(synthetic.make_state_dict(seed=0, num_quantizers=K), device="cuda:0")
    enc = MimiEncoder(device="cuda:0", model=model, num_quantizers=K, concurrency=2)
    lengths = synthetic.random_lengths(args.utts, 10.0, 20.0, seed=77)
    audio = [synthetic.speech_like(L, 77, i) for i, L in enumerate(lengths)]
    codes = enc.encode_audio_chunks(audio, 24000)
    tr = bpe.Trainer(K, CBS, codec_framerate=FR, chunk_size_secs=CHUNK_S, vocab_size=K * CBS + 1 + args.merges,
                     min_frequency=2, pad_token="<pad>", max_token_codebook_ngrams=2)
    t0 = time.perf_counter()
    tok = tr.train_codes([c.copy() for c in codes])
    train_s = time.perf_counter() - t0
    getattr(tok, "backend_tokenizer", tok).save(os.path.join(args.work, "tokenizer.json"))
    step = int(CHUNK_S * FR)
    chunks = [c[:, i:i + step] for c in codes for i in range(0, c.shape[1], step)]
    np.savez(os.path.join(args.work, "corpus.npz"), frames=np.array([c.shape[1] for c in chunks]),
             codes=np.concatenate(chunks, axis=1).astype(np.int16))
    return {"utterances": len(codes), "chunks": len(chunks), "audio_s": round(sum(len(a) for a in audio) / 24000.0, 1),
            "merges": len(tr.last_merges), "train_s": round(train_s, 3)}


def load_chunks(args):
    with np.load(os.path.join(args.work, "corpus.npz")) as z:
        frames, codes = z["frames"], z["codes"].astype(np.int64)
    ends = np.cumsum(frames)
    return [codes[:, e - n:e] for e, n in zip(ends, frames)] * args.repeat


def stage_gpu(args):
    import torch

    from mimi_hip import bpe
    chunks = load_chunks(args)
    enc = bpe.Encoder.from_tokenizer(os.path.join(args.work, "tokenizer.json"), K, CBS)
    enc.encode_codes(chunks[:8])  # model upload, buffers
    best = None
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ids = enc.encode_codes(chunks)
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, dict(enc.last_stats))
    # the device work alone: the words prepared once, HIP events on the call's stream around mimi_bpe_encode
    words = []
    for c in chunks:
        cps = bpe.codes_to_codepoints(c, CBS)
        words.extend(w.astype(np.int32) + np.int32(enc.n_special) for w in enc._chars.words(cps))
    stream = torch.cuda.Stream()
    dev_ms = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        enc.encode_words(words, stream=stream)
        b.record(stream)
        b.synchronize()
        dev_ms.append(a.elapsed_time(b))
    np.savez(os.path.join(args.work, "gpu_ids.npz"), lens=np.array([len(i) for i in ids]), ids=np.concatenate(ids))
    wall, st = best
    symbols, tokens = st["symbols"], st["tokens"]
    audio_s = sum(c.shape[1] for c in chunks) / FR
    dev_s = min(dev_ms) / 1e3
    return {"sequences": len(chunks), "words": st["words"], "symbols": symbols, "tokens": tokens,
            "compression_symbols_per_token": round(symbols / tokens, 3), "audio_s": round(audio_s, 1),
            "longest_word": int(max(len(w) for w in words)),
            "words_by_form": [enc.info("last_words_lds_small"), enc.info("last_words_lds"),
                              enc.info("last_words_global")],
            "formed_pair_outranks": enc.formed_pair_outranks,
            "device": {"seconds": round(dev_s, 5), "tokens_per_s": round(tokens / dev_s), "audio_s_per_s": round(audio_s / dev_s),
                       "all_runs_ms": [round(x, 2) for x in dev_ms],
                       "what": "HIP events around mimi_bpe_encode: H2D, kernels, D2H"},
            "wall": {"seconds": round(wall, 4), "tokens_per_s": round(tokens / wall), "audio_s_per_s": round(audio_s / wall),
                     "host_words_s": round(st["host_words_s"], 4), "encode_call_s": round(st["encode_s"], 4),
                     "what": "encode_codes: code points, NFKC word model, the GPU call, per-sequence arrays"}}


def stage_device(args):
    import torch

    from mimi_hip import bpe
    chunks = load_chunks(args)
    enc = bpe.Encoder.from_tokenizer(os.path.join(args.work, "tokenizer.json"), K, CBS)
    frames = [c.shape[1] for c in chunks]
    padded = np.zeros((len(chunks), K, max(frames)), np.int32)
    for b, c in enumerate(chunks):
        padded[b, :, :c.shape[1]] = c
    codes = torch.from_numpy(padded).cuda()  # uploaded once: the engine's output is already there
    enc.encode_device(codes[:8], frames[:8])  # model upload
    enc.encode_device(codes, frames)          # buffers
    torch.cuda.synchronize()
    wall, wall_host, dev_ms = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ids, offs, _ = enc.encode_device(codes, frames)
        wall.append(time.perf_counter() - t0)
    stats = dict(enc.last_stats)
    forms = [enc.info("last_words_lds_small"), enc.info("last_words_lds"), enc.info("last_words_global")]
    for _ in range(args.runs):
        t0 = time.perf_counter()
        seqs = enc.encode_device(codes, frames, to_host=True)
        wall_host.append(time.perf_counter() - t0)
    stream = torch.cuda.Stream()
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        enc.encode_device(codes, frames, stream=stream)
        b.record(stream)
        b.synchronize()
        dev_ms.append(a.elapsed_time(b))
    with np.load(os.path.join(args.work, "gpu_ids.npz")) as z:
        want_lens, want_ids = z["lens"], z["ids"]
    assert np.array_equal(np.diff(offs), want_lens) and np.array_equal(ids.cpu().numpy(), want_ids), \
        "encode_device ids differ from the gpu stage's"
    assert np.array_equal([len(x) for x in seqs], want_lens) and np.array_equal(np.concatenate(seqs), want_ids)
    tokens = int(offs[-1])
    audio_s = sum(frames) / FR

    def rate(seconds):
        return {"seconds": round(seconds, 5), "tokens_per_s": round(tokens / seconds),
                "audio_s_per_s": round(audio_s / seconds)}
    return {"sequences": len(chunks), "words": stats["words"], "tokens": tokens, "word_model": stats["word_model"],
            "words_by_form": forms, "same_ids_as_gpu": True,
            "wall": dict(rate(min(wall)), all_runs_ms=[round(x * 1e3, 2) for x in wall],
                         what="encode_device, ids left on the device (the call synchronises its stream)"),
            "wall_to_host": dict(rate(min(wall_host)), all_runs_ms=[round(x * 1e3, 2) for x in wall_host],
                                 what="encode_device(to_host=True): plus the copy out and one numpy array per sequence"),
            "device": dict(rate(min(dev_ms) / 1e3), all_runs_ms=[round(x, 2) for x in dev_ms],
                           what="HIP events around encode_device on its stream: kernels, the mid-way read-back, "
                                "the offsets copy")}


def stage_cpu(args):
    os.environ["RAYON_NUM_THREADS"] = str(args.threads)
    os.environ["TOKENIZERS_PARALLELISM"] = "true"
    try:
        import tokenizers
        from tokenizers import Tokenizer
    except ImportError:
        return {"tokenizers": None}
    from mimi_hip.codes import codes_to_chars
    chunks = load_chunks(args)
    strings = [codes_to_chars(c, CBS) for c in chunks]
    tok = Tokenizer.from_file(os.path.join(args.work, "tokenizer.json"))
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        enc = tok.encode_batch(strings, add_special_tokens=False)
        times.append(time.perf_counter() - t0)
    ids = [e.ids for e in enc]
    tokens = sum(map(len, ids))
    audio_s = sum(c.shape[1] for c in chunks) / FR
    out = {"tokenizers": tokenizers.__version__, "threads": args.threads, "sequences": len(strings), "tokens": tokens,
           "seconds_first": round(times[0], 4), "seconds_best": round(min(times), 4),
           "tokens_per_s": round(tokens / min(times)), "audio_s_per_s": round(audio_s / min(times))}
    gpu = os.path.join(args.work, "gpu_ids.npz")
    if os.path.exists(gpu):
        with np.load(gpu) as z:
            out["same_ids_as_gpu"] = bool(np.array_equal(z["lens"], [len(i) for i in ids]) and
                                          np.array_equal(z["ids"], np.concatenate([np.asarray(i) for i in ids])))
    return out


STAGES = {"corpus": (stage_corpus, 420), "gpu": (stage_gpu, 240), "device": (stage_device, 240),
          "cpu": (stage_cpu, 420)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--merges", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=8, help="the chunks are encoded this many times over in one call")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--work", default=os.path.join(ROOT, "bench_out", "bpe_encode"))
    ap.add_argument("--stage", choices=tuple(STAGES) + ("all",), default="all")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    os.makedirs(args.work, exist_ok=True)
    if args.stage != "all":
        print(json.dumps({args.stage: STAGES[args.stage][0](args)}))
        return
    report = {"note": "single run on a shared box", "corpus_like": "bench.py --workload mls --bpe",
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
    if "gpu" in report and "device" in report["gpu"] and report.get("cpu", {}).get("tokens_per_s"):
        report["gpu_device_over_tokenizers"] = round(report["gpu"]["device"]["tokens_per_s"] / report["cpu"]["tokens_per_s"], 2)
        report["gpu_wall_over_tokenizers"] = round(report["gpu"]["wall"]["tokens_per_s"] / report["cpu"]["tokens_per_s"], 2)
    if "wall" in report.get("device", {}) and report.get("cpu", {}).get("tokens_per_s"):
        cpu = report["cpu"]["tokens_per_s"]
        for key in ("wall", "wall_to_host", "device"):
            report[f"device_{key}_over_tokenizers"] = round(report["device"][key]["tokens_per_s"] / cpu, 2)
        report["device_wall_over_gpu_wall"] = round(report["device"]["wall"]["tokens_per_s"] /
                                                    report["gpu"]["wall"]["tokens_per_s"], 2)
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if any("failed" in v for v in report.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
