"""Generate the decode fixtures (run on the development machine only, like make_golden.py; outputs are committed).

    python tests/golden/make_decode_golden.py

``transformers`` 5.15.0 ``MimiModel`` is loaded with the seeded synthetic checkpoint, encode half
(``synthetic.make_state_dict``) + decode half (``synthetic.make_decoder_state_dict``): no key may be missing or
unexpected.  ``tests/decode_ref.py`` is then checked against it -- ``torch.equal`` on the waveform and on every
stage (quantizer.decode, upsample, decoder_transformer, decoder) -- and the fixtures are written from it:

* ``codes_T{T}`` (int16 [32, T]) and ``wave_T{T}_K{K}`` (float32 [1920 T]) for T in {1, 2, 3, 13}, K in {1, 8, 32};
  the codes are ``mimi_ref.encode`` of ``synthetic.speech_like`` clips (codes a user would hold);
* ``codes_rand`` / ``wave_rand``: T = 3, K = 8, uniformly random codes;
* ``tap_{name}_sub{s}``: the stage tensors of T = 13, K = 8 (channel-first), every s-th time step;
* ``codes_T129`` / ``wave_T129_K8_sub8``: 258 transformer frames (the reference builds its explicit sliding-window
  mask), every 8th sample (a full 129-frame waveform alone is ~1 MB).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tokenize-audio_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import decode_ref  # noqa: E402
from mimi_hip import synthetic  # noqa: E402
from oracle import mimi_ref  # noqa: E402

FRAMES = [1, 2, 3, 13]
KS = [1, 8, 32]
AUDIO_SEED = 11
TAP_CAP = 6000   # elements per stored stage tensor
LONG_T, LONG_SUB = 129, 8


def subsample(t, cap=TAP_CAP):
    sub = 1
    while t.numel() // sub > cap:
        sub *= 2
    return sub, t[..., ::sub]


def main():
    torch.set_num_threads(8)
    from transformers import MimiConfig as TMimiConfig, MimiModel

    enc_sd = synthetic.make_state_dict(seed=0)
    dec_sd = synthetic.make_decoder_state_dict(seed=0)
    assert not set(enc_sd) & set(dec_sd)
    sd = {**enc_sd, **dec_sd}
    model = MimiModel(TMimiConfig()).eval()
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and not res.missing_keys, (res.unexpected_keys, res.missing_keys)
    sdt = decode_ref.as_tensors(sd)
    rc = mimi_ref.RefConfig()

    meta = {"weights_seed": 0, "encode_state_dict_sha256": synthetic.state_dict_sha256(enc_sd),
            "state_dict_sha256": synthetic.state_dict_sha256(dec_sd), "audio_seed": AUDIO_SEED,
            "transformers": "5.15.0", "torch": torch.__version__, "frames": FRAMES, "ks": KS,
            "long_frames": LONG_T, "long_sub": LONG_SUB, "wave_absmax": {}}
    arrays = {}

    def codes_for(T, index):
        x = synthetic.speech_like(decode_ref.FRAME * T, AUDIO_SEED, index)
        c = mimi_ref.encode(torch.from_numpy(x)[None, None], enc_sd, 32)
        assert c.shape == (1, 32, T)
        return c

    with torch.no_grad():
        for i, T in enumerate(FRAMES):
            codes = codes_for(T, i)
            arrays[f"codes_T{T}"] = codes[0].numpy().astype(np.int16)
            for K in KS:
                ck = codes[:, :K]
                taps = {}
                y = decode_ref.decode(ck, sdt, rc, taps)
                hf = model.decode(ck).audio_values
                assert torch.equal(y, hf), f"decode_ref != transformers at T={T} K={K}"
                assert y.shape == (1, 1, decode_ref.FRAME * T) and decode_ref.decoded_length(T) == y.shape[-1]
                # stage by stage
                q = model.quantizer.decode(ck)
                assert torch.equal(q, taps["quantized"])
                u = model.upsample(q)
                assert torch.equal(u, taps["upsample"])
                t = model.decoder_transformer(u.transpose(1, 2), return_dict=False)[0].transpose(1, 2)
                assert torch.equal(t, taps["xfmr7"])
                assert torch.equal(model.decoder(t), y)
                arrays[f"wave_T{T}_K{K}"] = y[0, 0].numpy()
                meta["wave_absmax"][f"T{T}_K{K}"] = float(y.abs().max())
                if T == 13 and K == 8:
                    for name in decode_ref.TAP_NAMES:
                        sub, v = subsample(taps[name][0])
                        arrays[f"tap_{name}_sub{sub}"] = v.contiguous().numpy()
                        meta.setdefault("tap_absmax", {})[name] = float(taps[name].abs().max())
                # causal prefix: new codes in frame f leave samples [0, 1920 f) bit-identical
                if T > 1 and K == 8:
                    for f in sorted({1, T - 1}):
                        c2 = ck.clone()
                        c2[:, :, f] = (c2[:, :, f] + 977) % 2048
                        y2 = decode_ref.decode(c2, sdt, rc)
                        n = decode_ref.FRAME * f
                        assert torch.equal(y2[..., :n], y[..., :n]) and not torch.equal(y2, y), (T, f)
            print(f"T={T:3d} |wave| max {meta['wave_absmax'][f'T{T}_K8']:.3f}")

        g = np.random.default_rng(5)
        cr = torch.from_numpy(g.integers(0, 2048, (1, 8, 3)))
        y = decode_ref.decode(cr, sdt, rc)
        assert torch.equal(y, model.decode(cr).audio_values)
        arrays["codes_rand"] = cr[0].numpy().astype(np.int16)
        arrays["wave_rand"] = y[0, 0].numpy()

        codes = codes_for(LONG_T, 50)[:, :8]
        y = decode_ref.decode(codes, sdt, rc)
        assert torch.equal(y, model.decode(codes).audio_values), "decode_ref != transformers at T=129"
        assert y.shape[-1] == decode_ref.FRAME * LONG_T
        arrays[f"codes_T{LONG_T}"] = codes[0].numpy().astype(np.int16)
        arrays[f"wave_T{LONG_T}_K8_sub{LONG_SUB}"] = y[0, 0, ::LONG_SUB].contiguous().numpy()
        meta["wave_absmax"][f"T{LONG_T}_K8"] = float(y.abs().max())

    with open(os.path.join(OUT, "decode_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    path = os.path.join(OUT, "decode.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
