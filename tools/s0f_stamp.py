"""Runs B = 32 x 10 s f16x3 encodes with the in-kernel phase-stamp build of the fused stage-0 kernel
(MIMI_HIP_LIB=tools/bin/libmimi_hip_st.so, built with -DS0F_STAMP=1, e.g. tools/build_variant.sh st stage0_fused.hip
"-DS0F_STAMP=1" and the result copied to tools/bin); the kernel prints per-wave cycle sums of workgroup 0, six slots:

  block waves  0 descriptor (+ halo without S0F_HELP) and slab head, 1 conv0, 2 slab ELU + split,
               3 GEMM1 + the kept block's y epilogue + h (S0F_DEFER = 0: GEMM1 + h; a round without a block: the kept
               epilogue alone), 4 GEMM2 + z (S0F_DEFER = 0: GEMM2 + y), 5 barrier
  conv waves   0 halo copy + down-conv MFMA loop, 1 x1 stores, 2 audio split + barrier

Divide by the rounds run: R + 2 with S0F_DEFER (R + 1 without), R = the printed round count."""
import sys

import numpy as np
import torch

sys.path.insert(0, "tokenize-audio_amd")
from mimi_hip import synthetic  # noqa: E402
from mimi_hip.model import MimiHipModel  # noqa: E402

m = MimiHipModel(synthetic.make_state_dict(seed=0, num_quantizers=8), device="cuda:0")
m.set_graphs(False)
if len(sys.argv) > 1:
    m.set_option("stage0_fused", int(sys.argv[1]))
x = torch.from_numpy(np.stack([synthetic.speech_like(240000, 1, i) for i in range(32)])).cuda()
for _ in range(2):
    m.encode_int32(x, 8)
torch.cuda.synchronize()
