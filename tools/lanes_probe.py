"""Probe: small uniform batches (1 and 4 x 10 s, K = 8) kept one behind (encode_async) under the engine's lane settings --
the persistent RVQ chain without a lane (the default), the per-level kernels in lanes (rvq_chain = 0), the chain in
lanes (lanes = 2), lanes off -- alternated 3 times in one process: ms per encode, chain re-runs, lanes used.

    python tools/lanes_probe.py
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tokenize-audio_amd"))
from mimi_hip import synthetic  # noqa: E402
from mimi_hip.model import MimiHipModel  # noqa: E402

m = MimiHipModel(synthetic.make_state_dict(seed=0, num_quantizers=8), device="cuda:0")
L, K, N = 240000, 8, 60
for B in (1, 4):
    x = torch.from_numpy(synthetic.clip_batch(B, L, seed=3000 + B)).cuda()
    outs = [torch.empty((B, K, 125), dtype=torch.int32, device="cuda") for _ in range(2)]
    ref = m.encode_int32(x, K).clone()

    def run(n):
        held = None
        for i in range(n):
            t = m.encode_async(x, K, out=outs[i & 1])
            if held is not None:
                held.wait()
            held = t
        held.wait()

    for rnd in range(3):
        for name, lanes, chain in (("lanes1_chain (default: no lane)", 1, 1), ("lanes1_perlevel (laned)", 1, 0),
                                   ("lanes2_chain (laned)", 2, 1), ("lanes0_chain", 0, 1)):
            m.set_option("lanes", lanes)
            m.set_option("rvq_chain", chain)
            run(6)
            torch.cuda.synchronize()
            r0, l0 = m.rvq_chain_reruns, m.lane_encodes
            t0 = time.perf_counter()
            run(N)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / N
            l1 = m.lane_encodes
            same = bool(torch.equal(outs[0], ref) and torch.equal(outs[1], ref))
            print(f"B={B} round {rnd + 1} {name}: {dt * 1e3:.3f} ms per encode, chain re-runs {m.rvq_chain_reruns - r0}, "
                  f"lanes used {(l1[0] - l0[0], l1[1] - l0[1])}, codes equal {same}", flush=True)
