"""Regenerates ``encode_stream_window_clip.npz``: the 130-frame clip of the streaming-encode tests' real-window case.

At the real window (250 rows) one key holds ~1/250 of a query's attention on natural input, and on the synthetic
checkpoint a window that is off by one row then moves the pre-quantizer embedding by 3e-4 .. 8e-4 only (speech-like
clips, noise, bursts and squares were tried): too little to tell such a kernel from a right one by 10 x the tolerance.
This clip is the project's speech-like clip (seed 24, index 0) after ``STEPS`` steps of gradient ascent, on the CPU
reference (``oracle/mimi_ref.py``), of how far a window of 249 and of 251 rows move the embedding: a few per cent of
full scale per sample, after which the rows that leave / enter the window carry enough of the last queries' attention.
Stored as float16 (every sample is then exact in float32).  Deterministic for a given torch build; the tests only need
the stored file, and check what it does (tests/test_encode_stream_ref.py) rather than how it was made.

    python tests/golden/make_window_clip.py [STEPS]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tokenize-audio_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mimi_hip import synthetic  # noqa: E402
from oracle import mimi_ref  # noqa: E402

FRAMES, SEED, LR = 130, 24, 3e-3


def pnorm(t, p=8):
    return (t.abs() ** p).sum() ** (1.0 / p)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 14
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "encode_stream_window_clip.npz")
    torch.manual_seed(0)
    sd = {k: torch.from_numpy(np.asarray(v)).float() for k, v in synthetic.make_state_dict(seed=0).items()}
    x = torch.from_numpy(synthetic.speech_like(1920 * FRAMES, SEED, 0))[None, None].clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=LR)
    cfgs = [mimi_ref.RefConfig(sliding_window=w) for w in (250, 249, 251)]
    for it in range(steps):
        opt.zero_grad()
        e = mimi_ref.seanet_encoder(x, sd, cfgs[0])
        outs = []
        for c in cfgs:
            y = mimi_ref.transformer(e.transpose(1, 2), sd, c).transpose(1, 2)
            outs.append(mimi_ref.causal_conv1d(y, sd["downsample.conv.weight"], None, stride=2, pad_mode="replicate"))
        d1, d2 = outs[1] - outs[0], outs[2] - outs[0]
        loss = -(torch.log(pnorm(d1)) + torch.log(pnorm(d2))) + 2 * torch.log(pnorm(outs[0]))
        loss.backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(-1.0, 1.0)
            m = float(outs[0].abs().max())
            print(it, "window 249: %.3e  window 251: %.3e" % (float(d1.abs().max()) / m, float(d2.abs().max()) / m), flush=True)
    np.savez_compressed(out, audio=x.detach().numpy()[0, 0].astype(np.float16), frames=FRAMES, seed=SEED, steps=steps)


if __name__ == "__main__":
    main()
