"""``MimiHipModel``: the ``MimiModel.encode`` / ``MimiModel.decode`` drop-in over the HIP engine.

Mirrors the model-level API every reference wrapper calls:

* ``model.encode(input_values[B, C, L], padding_mask=None, num_quantizers=None)`` ->
  ``MimiEncoderOutput`` with ``.audio_codes`` int64 ``[B, K, T]`` on the model's device, and tuple
  indexing (``out[0]`` is the codes; ``librispeech-mimi/utils.py:64-66`` does ``audio_codes[0][0]``).
  ``TF/modeling_mimi.py:1297-1386``: K defaults to ``config.num_quantizers`` (32), ``ValueError`` for
  K > 32 and for channels not in {1, 2}; ``padding_mask`` is accepted and ignored exactly as there
  (``:1244, :1247``).
* ``model.decode(audio_codes[B, K, T], padding_mask=None)`` (models built with ``decode=True``) ->
  ``MimiDecoderOutput`` with ``.audio_values`` float32 ``[B, 1, 1920 T]`` on the model's device
  (``TF/modeling_mimi.py:1408-1458``; ``librispeech-mimi/utils.py:72-81`` does ``.audio_values[0]``).
* ``model.decode_stream(batch, num_quantizers, max_step_frames)`` -> ``DecodeStream``: ``.step(codes[B, K, n])`` returns
  the ``1920 n`` samples of the next ``n`` frames from a KV cache and per-stage carries (the same bits under any split
  of a sequence into steps); ``.step(codes[m, K, n], slots=[...])`` advances only the listed slots, each at its own
  position, and ``.reset(slot)`` frees one.
* ``model.encode_stream(batch, num_quantizers, max_step_frames)`` -> ``EncodeStream``: ``.step(audio[B, 1920 n])``
  returns the int32 codes ``[B, K, n]`` of the next ``n`` whole frames, with the same slot interface and the same
  bit contract (``encode(use_streaming=True)`` and the reference's cache objects stay unprovided).
* ``.to(device)``, ``.eval()``, ``get_encoded_length``, ``from_pretrained(local_dir | "kyutai/mimi")``.

The arithmetic runs in ``libmimi_hip.so`` (HIP kernels for gfx950); torch only supplies device memory and
the current stream.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import glob
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .config import MimiConfig, encoded_length


@dataclass
class MimiEncoderOutput:
    """Same fields as ``transformers`` ``MimiEncoderOutput`` (``TF/modeling_mimi.py:167-187``)."""
    audio_codes: torch.Tensor
    encoder_past_key_values: Optional[object] = None
    padding_cache: Optional[object] = None

    def to_tuple(self):
        return tuple(v for v in (self.audio_codes, self.encoder_past_key_values, self.padding_cache)
                     if v is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return len(self.to_tuple())


@dataclass
class MimiDecoderOutput:
    """Same fields as ``transformers`` ``MimiDecoderOutput`` (``TF/modeling_mimi.py:190-207``)."""
    audio_values: torch.Tensor
    decoder_past_key_values: Optional[object] = None

    def to_tuple(self):
        return tuple(v for v in (self.audio_values, self.decoder_past_key_values) if v is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return len(self.to_tuple())


def _resolve_device(device) -> torch.device:
    d = torch.device(device) if not isinstance(device, torch.device) else device
    if d.type != "cuda":
        raise ValueError(f"MimiHipModel runs on a HIP device ('cuda' under ROCm), got {d}")
    if d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def resolve_checkpoint(name_or_path: str) -> str:
    """Map ``"kyutai/mimi"`` (a Hub name; no network here) or a local directory/file to a local path.

    Order: an existing path; ``$MIMI_HIP_CHECKPOINT``; the huggingface_hub cache (``$HF_HUB_CACHE``, else
    ``$HF_HOME/hub``, else ``~/.cache/huggingface/hub``), ``models--<org>--<name>/snapshots/<rev>`` with ``<rev>``
    from ``refs/main`` when present (the snapshot ``from_pretrained`` would load offline), else the newest."""
    if os.path.exists(name_or_path):
        return name_or_path
    env = os.environ.get("MIMI_HIP_CHECKPOINT")
    if env and os.path.exists(env):
        return env
    hub = os.environ.get("HF_HUB_CACHE") or os.path.join(
        os.environ.get("HF_HOME", os.path.expanduser("~/.cache/huggingface")), "hub")
    repo = os.path.join(hub, "models--" + name_or_path.replace("/", "--"))
    ref = os.path.join(repo, "refs", "main")
    if os.path.exists(ref):
        with open(ref) as f:
            snap = os.path.join(repo, "snapshots", f.read().strip())
        if os.path.isdir(snap):
            return snap
    snaps = sorted(glob.glob(os.path.join(repo, "snapshots", "*")), key=os.path.getmtime)
    if snaps:
        return snaps[-1]
    raise FileNotFoundError(
        f"checkpoint {name_or_path!r} is not available locally; pass a directory holding model.safetensors "
        f"(+ config.json), set MIMI_HIP_CHECKPOINT, or use 'synthetic:<seed>' for the seeded test checkpoint")


class EncodeTicket:
    """An encode in flight (``MimiHipModel.encode_async``)."""

    def __init__(self, model: "MimiHipModel", ticket: int, out: torch.Tensor, audio: torch.Tensor):
        self._model, self._ticket, self.out, self._audio = model, ticket, out, audio

    def wait(self) -> torch.Tensor:
        if self._ticket:
            t, self._ticket = self._ticket, 0
            _lib.check(self._model._lib.mimi_encode_wait(self._model._h, t))
            self._audio = None
        return self.out


class _Stream:
    """What ``DecodeStream`` and ``EncodeStream`` share: the handle, the slots' bookkeeping and the calls into
    ``mimi_{decode,encode}_stream_*`` (``_direction`` names which)."""

    _direction = ""

    def __init__(self, model: "MimiHipModel", batch: int, num_quantizers: int, max_step_frames: int):
        self._model, self.batch, self.num_quantizers = model, int(batch), int(num_quantizers)
        self.max_step_frames = int(max_step_frames)
        self._h = None
        h = ctypes.c_void_p()
        self._call("create", model._h, self.batch, self.num_quantizers, self.max_step_frames, ctypes.byref(h))
        self._h = h

    def _fn(self, name: str):
        return getattr(self._model._lib, f"mimi_{self._direction}_stream_{name}")

    def _call(self, name: str, *args):
        """``mimi_<direction>_stream_<name>(*args)``; an invalid argument (status 1) is a ``ValueError``."""
        try:
            _lib.check(self._fn(name)(*args))
        except _lib.MimiHipError as err:
            if err.status == 1:
                raise ValueError(str(err)) from None
            raise

    def _handle(self):
        if self._h is None:
            raise RuntimeError(f"this {type(self).__name__} is closed")
        return self._h

    @property
    def position(self) -> int:
        """Frames stepped so far (the furthest slot's)."""
        return int(self._fn("position")(self._handle()))

    @property
    def positions(self) -> List[int]:
        """Frames stepped by each slot since its last reset."""
        h = self._handle()
        return [int(self._fn("slot_position")(h, b)) for b in range(self.batch)]

    @property
    def state_bytes(self) -> int:
        return int(self._fn("state_bytes")(self._handle()))

    def _items(self, slots: Optional[Sequence[int]]):
        """The checked slot list of a step (``None``: all slots) and the number of items it takes."""
        if slots is None:
            return None, self.batch
        slots = [int(x) for x in slots]
        if not 1 <= len(slots) <= self.batch:
            raise ValueError(f"a step lists 1 .. {self.batch} slots, got {len(slots)}")
        if min(slots) < 0 or max(slots) >= self.batch or len(set(slots)) != len(slots):
            raise ValueError(f"slots must be distinct and in [0, {self.batch}), got {slots}")
        return slots, len(slots)

    def _step(self, slots: Optional[List[int]], src: torch.Tensor, n: int, out: torch.Tensor):
        """One step of ``n`` frames from the device tensor ``src`` into ``out``, over all slots or the listed ones."""
        io = (ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), self._model._stream())
        if slots is None:
            self._call("step", self._handle(), *io)
        else:
            self._call("step_slots", self._handle(), (ctypes.c_int32 * len(slots))(*slots), len(slots), *io)

    def reset(self, slot: Optional[int] = None):
        """Back to position 0 with a fresh state: what follows equals a fresh stream.  With ``slot`` only that slot, its
        neighbours untouched (``ValueError`` for a slot outside ``[0, batch)``)."""
        if slot is None:
            self._call("reset", self._handle())
        else:
            self._call("reset_slot", self._handle(), int(slot))

    def close(self):
        h, self._h = self._h, None
        if h is not None and self._model._h is not None:
            self._fn("destroy")(h)
        self._model._streams.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodeStream(_Stream):
    """Streaming decode (``MimiHipModel.decode_stream``): ``batch`` items, ``n`` new frames of codes in and their
    ``1920 n`` samples out per ``step``, on a KV cache and per-stage carries that the stream owns in device memory
    (``state_bytes``, constant).  The samples are bitwise the same under any split of a sequence into steps, and within
    the activation tolerance of ``decode`` of the whole sequence.

    Every item is a SLOT with its own position: ``step(codes)`` advances all of them, ``step(codes, slots=[...])`` only
    the listed ones (sessions that start and end at different times: a new session takes a free slot, ``reset(slot)``
    frees it).  A slot's samples are bitwise those of a ``batch=1`` stream fed the same sequence, whatever its
    neighbours do.  A context manager; ``close()`` frees the state (closing the model closes its streams)."""

    _direction = "decode"

    def step(self, codes: torch.Tensor, out: Optional[torch.Tensor] = None,
             slots: Optional[Sequence[int]] = None, frames: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The next ``n`` frames: int64 / int32 codes ``[B, K, n]`` on any device -> float32 ``[B, 1, 1920 n]`` on the
        model's device (``out`` if given).  With ``slots`` (``m`` distinct ints in ``[0, batch)``, any order) only those
        slots advance: ``codes`` is ``[m, K, n]``, item ``i`` the next frames of slot ``slots[i]``, the result
        ``[m, 1, 1920 n]``.  ``ValueError`` for ``n`` outside ``[1, max_step_frames]`` and a bad slot list (the state is
        untouched) and for a code outside ``[0, codebook_size)`` (the slots of that call then refuse until ``reset``).

        With ``frames`` (one int per item, each in ``[1, n]``) item ``i`` advances by its own ``frames[i]`` frames:
        ``codes`` is padded, ``[m, K, n]`` with columns past ``frames[i]`` never read, and so is the result, ``[m, 1,
        1920 n]`` -- zero past ``1920 frames[i]`` samples when this call allocates it, left untouched there in a
        caller's ``out``.  Without ``slots`` the items are slots ``0 .. batch - 1``.  Bad ``frames`` raise
        ``ValueError`` with the state untouched."""
        m = self._model
        self._handle()
        if not torch.is_tensor(codes):
            codes = torch.as_tensor(np.asarray(codes))
        slots, items = self._items(slots)
        if codes.dim() != 3 or codes.shape[0] != items or codes.shape[1] != self.num_quantizers:
            raise ValueError(f"codes must be [{items}, {self.num_quantizers}, n], got {tuple(codes.shape)}")
        n = int(codes.shape[2])
        if n < 1 or n > self.max_step_frames:
            raise ValueError(f"a step takes 1 .. {self.max_step_frames} frames, got {n}")
        if frames is not None:
            frames = [int(x) for x in frames]
            if len(frames) != items or min(frames) < 1 or max(frames) > n:
                raise ValueError(f"frames must be {items} counts in [1, {n}], got {frames}")
        L = m.get_decoded_length(n)
        if out is None:
            out = (torch.empty if frames is None else torch.zeros)((items, 1, L), dtype=torch.float32, device=m.device)
        elif (tuple(out.shape) != (items, 1, L) or out.dtype != torch.float32 or out.device != m.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{items}, 1, {L}] tensor on {m.device}")
        codes = codes.to(device=m.device, dtype=torch.int32).contiguous()
        if frames is None:
            self._step(slots, codes, n, out)
        else:
            if slots is None:
                slots = list(range(self.batch))
            i32 = ctypes.c_int32 * items
            self._call("step_ragged", self._handle(), i32(*slots), i32(*frames), items, n,
                       ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(out.data_ptr()), m._stream())
        return out


class EncodeStream(_Stream):
    """Streaming encode (``MimiHipModel.encode_stream``): ``batch`` items, ``n`` whole frames of audio (``frame_samples``
    = 1920 samples each) in and their codes ``[., K, n]`` out per ``step``, on a KV cache and per-stage carries that the
    stream owns in device memory (``state_bytes``, constant).  The codes of frames ``[p, p + n)`` are bitwise the same
    under any split of a sequence into steps; the pre-quantizer embedding is within the activation tolerance of
    ``encode`` of any sequence that holds those frames whole.  Always fp32 arithmetic, whatever ``set_precision`` says.

    Every item is a SLOT with its own position, as in ``DecodeStream``: ``step(audio)`` advances all of them,
    ``step(audio, slots=[...])`` only the listed ones, ``reset(slot)`` frees one.  A slot's codes are bitwise those of a
    ``batch=1`` stream fed the same sequence, whatever its neighbours do.  A tail shorter than a frame is the caller's
    to keep for the next step.  A context manager; ``close()`` frees the state (closing the model closes its streams)."""

    _direction = "encode"

    def __init__(self, model: "MimiHipModel", batch: int, num_quantizers: int, max_step_frames: int):
        self.frame_samples = int(model._lib.mimi_frame_samples_cfg(ctypes.byref(model._cfg_c)))
        super().__init__(model, batch, num_quantizers, max_step_frames)

    def step(self, audio: torch.Tensor, slots: Optional[Sequence[int]] = None,
             out: Optional[torch.Tensor] = None, frames: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The next ``n`` frames: float32 audio ``[B, F n]`` or ``[B, 1, F n]`` (``F = frame_samples``) on any device ->
        int32 codes ``[B, K, n]`` on the model's device (``out`` if given).  With ``slots`` (``m`` distinct ints in
        ``[0, batch)``, any order) only those slots advance: ``audio`` holds ``m`` items, item ``i`` the next frames of
        slot ``slots[i]``, the result is ``[m, K, n]``.  ``ValueError`` for a length that is not ``1 ..
        max_step_frames`` whole frames and for a bad slot list or ``out`` (the state is untouched).

        With ``frames`` (one int per item, each in ``[1, n]``) item ``i`` advances by its own ``frames[i]`` frames:
        ``audio`` is padded, ``[m, F n]`` with samples past ``F frames[i]`` never read (NaN there is harmless), and so
        is the result, ``[m, K, n]`` -- zero past ``frames[i]`` when this call allocates it, left untouched there in a
        caller's ``out``.  Without ``slots`` the items are slots ``0 .. batch - 1``.  Bad ``frames`` raise
        ``ValueError`` with the state untouched."""
        m = self._model
        self._handle()
        if not torch.is_tensor(audio):
            audio = torch.as_tensor(np.asarray(audio))
        slots, items = self._items(slots)
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.dim() != 2 or audio.shape[0] != items:
            raise ValueError(f"audio must be [{items}, F n] or [{items}, 1, F n], got {tuple(audio.shape)}")
        F = self.frame_samples
        L = int(audio.shape[1])
        if L % F or not 1 <= L // F <= self.max_step_frames:
            raise ValueError(f"a step takes 1 .. {self.max_step_frames} whole frames of {F} samples, got {L} samples")
        n = L // F
        if frames is not None:
            frames = [int(x) for x in frames]
            if len(frames) != items or min(frames) < 1 or max(frames) > n:
                raise ValueError(f"frames must be {items} counts in [1, {n}], got {frames}")
        fresh = out is None
        out = m._out(items, self.num_quantizers, n, out)
        audio = audio.to(device=m.device, dtype=torch.float32).contiguous()
        if frames is None:
            self._step(slots, audio, n, out)
        else:
            if fresh:
                out.zero_()
            if slots is None:
                slots = list(range(self.batch))
            i32 = ctypes.c_int32 * items
            self._call("step_ragged", self._handle(), i32(*slots), i32(*frames), items, n,
                       ctypes.c_void_p(audio.data_ptr()), ctypes.c_void_p(out.data_ptr()), m._stream())
        return out


class MimiHipModel:
    """Mimi on MI355X: encode always; decode (codes -> waveform) when built with ``decode=True``, which makes the
    decoder half of the checkpoint (``decoder*``, ``upsample*``, ``decoder_transformer*``, ``output_proj``) required.
    Decode runs in fp32-MFMA arithmetic whatever ``set_precision`` says."""

    def __init__(self, state_dict: Optional[Dict[str, np.ndarray]] = None, config: Optional[MimiConfig] = None,
                 device: Union[str, torch.device] = "cuda", safetensors_path: Optional[str] = None,
                 decode: bool = False):
        self.config = config or MimiConfig()
        self.config.validate_supported()
        self._lib = _lib.load()
        self.device = _resolve_device(device)
        self._cfg_c = _lib.config_from_py(self.config)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.mimi_create(ctypes.byref(self._cfg_c), self.device.index, ctypes.byref(handle)))
        self._h = handle
        self._lock = threading.Lock()
        self._streams = weakref.WeakSet()  # open DecodeStreams / EncodeStreams: closed before the engine
        self._src = (state_dict, config, safetensors_path)  # for clone()
        self.decode_enabled = bool(decode)
        try:
            if decode:
                _lib.check(self._lib.mimi_enable_decode(self._h))
            if safetensors_path is not None:
                _lib.check(self._lib.mimi_load_safetensors(self._h, safetensors_path.encode()))
            if state_dict is not None:
                for name, value in state_dict.items():
                    if not decode and name.startswith(("decoder", "upsample")):
                        continue
                    arr = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
                    arr = np.ascontiguousarray(arr, dtype=np.float32)
                    _lib.check(self._lib.mimi_set_weight(self._h, name.encode(), arr.ctypes.data, arr.size))
            _lib.check(self._lib.mimi_finalize(self._h))
        except Exception:
            self.close()
            raise

    # ---- construction helpers -------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, name_or_path: str = "kyutai/mimi", device="cuda", decode: bool = False,
                        **kw) -> "MimiHipModel":
        if name_or_path.startswith("synthetic"):
            from . import synthetic
            seed = int(name_or_path.split(":", 1)[1]) if ":" in name_or_path else 0
            sd = synthetic.make_state_dict(seed=seed)
            if decode:
                sd.update(synthetic.make_decoder_state_dict(seed=seed))
            return cls(sd, device=device, decode=decode)
        path = resolve_checkpoint(name_or_path)
        cfg = MimiConfig()
        if os.path.isdir(path):
            if os.path.exists(os.path.join(path, "config.json")):
                cfg = MimiConfig.from_json(path)
            files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
            if not files:
                raise FileNotFoundError(f"no .safetensors file in {path}")
            path = files[0]
        return cls(config=cfg, device=device, safetensors_path=path, decode=decode, **kw)

    def clone(self, device: Union[str, torch.device, None] = None) -> "MimiHipModel":
        """Another engine with the same weights and config (its own workspace; same calibration, so the same codes):
        independent encodes on several engines run concurrently (``MimiEncoder.encode_audio_chunks``)."""
        sd, cfg, path = self._src
        m = MimiHipModel(sd, config=cfg or self.config, device=device or self.device, safetensors_path=path,
                         decode=self.decode_enabled)
        m.set_precision(self.precision)
        return m

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            for st in list(getattr(self, "_streams", ())):
                st.close()
            self._lib.mimi_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- nn.Module-ish no-ops the wrappers call -------------------------------------------------
    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            d = _resolve_device(device)
            if d != self.device:
                raise ValueError(f"engine lives on {self.device}; create a new MimiHipModel for {d}")
        return self

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self

    def get_encoded_length(self, input_length):
        if torch.is_tensor(input_length):
            return input_length.new_tensor([encoded_length(int(x), self.config) for x in input_length.flatten()]
                                           ).view_as(input_length)
        return encoded_length(int(input_length), self.config)

    # ---- encode --------------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_k(self, K: int) -> int:
        """The reference's num_quantizers checks (TF/modeling_mimi.py:1335-1340); the C side would replace
        K <= 0 by config.num_quantizers, so a caller's 0 must not reach it with an output sized for 0 levels."""
        K = int(K)
        if K > self.config.num_quantizers:
            raise ValueError(
                f"The number of quantizers (i.e codebooks) asked should be lower than the total number of "
                f"quantizers {self.config.num_quantizers}, but is currently {K}.")
        if K < self.config.num_semantic_quantizers:
            raise ValueError(
                f"The number of quantizers (i.e codebooks) asked should be higher than the number of semantic "
                f"quantizers {self.config.num_semantic_quantizers}, but is currently {K}.")
        return K

    def _device_audio(self, audio: torch.Tensor) -> torch.Tensor:
        """device f32 [B, L], contiguous (the C ABI reads audio.data_ptr() as such)."""
        if audio.dim() != 2:
            raise ValueError(f"audio must be [batch, length], got {tuple(audio.shape)}")
        return audio.to(device=self.device, dtype=torch.float32).contiguous()

    def _out(self, B: int, K: int, T: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        if out is None:
            return torch.empty((B, K, T), dtype=torch.int32, device=self.device)
        if (tuple(out.shape) != (B, K, T) or out.dtype != torch.int32 or out.device != self.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int32 [{B}, {K}, {T}] tensor on {self.device}")
        return out

    def encode(self, input_values: torch.Tensor, padding_mask: Optional[torch.Tensor] = None,
               num_quantizers: Optional[int] = None, encoder_past_key_values=None, padding_cache=None,
               use_streaming: Optional[bool] = None, return_dict: Optional[bool] = None):
        if use_streaming:
            # (the reference's cache objects are not provided: the chunked path is encode_stream)
            raise NotImplementedError("streaming encode (padding cache / KV cache) is not on the batch path")
        K = self._check_k(self.config.num_quantizers if num_quantizers is None else num_quantizers)
        if not torch.is_tensor(input_values):
            input_values = torch.as_tensor(np.asarray(input_values))
        if input_values.dim() != 3:
            raise ValueError(f"input_values must be [batch, channels, length], got {tuple(input_values.shape)}")
        B, channels, L = input_values.shape
        if channels < 1 or channels > 2:
            raise ValueError(f"Number of audio channels must be 1 or 2, but got {channels}")
        if channels != self.config.audio_channels:
            raise ValueError(f"expected {self.config.audio_channels} audio channel(s), got {channels}")
        T = encoded_length(L, self.config)
        codes = torch.empty((B, K, T), dtype=torch.int32, device=self.device)
        if B == 0 or L == 0:
            return MimiEncoderOutput(codes.long())
        x = input_values.to(device=self.device, dtype=torch.float32).reshape(B, L).contiguous()
        # (no Python lock: the engine serialises enqueues itself and waits outside its lock, so threads sharing
        # one engine overlap -- the YODAS2 thread pool, yodas2-mimi/process_shard.py:691-717)
        _lib.check(self._lib.mimi_encode(self._h, ctypes.c_void_p(x.data_ptr()), B, L, K,
                                         ctypes.c_void_p(codes.data_ptr()), self._stream()))
        out = codes.long()
        if return_dict is False:
            return (out, None, None)
        return MimiEncoderOutput(out)

    def encode_stream(self, batch: int = 1, num_quantizers: Optional[int] = None,
                      max_step_frames: int = 1) -> EncodeStream:
        """A streaming encode of ``batch`` items (``mimi_encode_stream_*``): ``.step(audio[B, 1920 n])`` returns the int32
        codes ``[B, K, n]`` of the next ``n <= max_step_frames`` frames of all of them, ``.step(audio[m, 1920 n],
        slots=[...])`` of the listed slots only, each slot at its own position.  Works without the decode weights.
        Several streams may be open on one model and interleave with ``encode`` / ``decode`` / ``decode_stream``."""
        K = self._check_k(self.config.num_quantizers if num_quantizers is None else num_quantizers)
        if int(batch) < 1 or int(max_step_frames) < 1:
            raise ValueError(f"batch and max_step_frames must be >= 1, got {batch} and {max_step_frames}")
        st = EncodeStream(self, batch, K, max_step_frames)
        self._streams.add(st)
        return st

    def encode_int32(self, audio: torch.Tensor, num_quantizers: int, out: Optional[torch.Tensor] = None
                     ) -> torch.Tensor:
        """Lean path for the bench / shard driver: device f32 [B, L] in, device int32 [B, K, T] out."""
        K = self._check_k(num_quantizers)
        audio = self._device_audio(audio)
        B, L = audio.shape
        out = self._out(B, K, encoded_length(L, self.config), out)
        _lib.check(self._lib.mimi_encode(self._h, ctypes.c_void_p(audio.data_ptr()), B, L, K,
                                         ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def encode_host(self, audio: np.ndarray, num_quantizers: int) -> np.ndarray:
        """Host f32 [B, L] in, host int32 [B, K, T] out, in one C call (``mimi_encode_host``: the engine's own device
        and pinned buffers, one host synchronisation) on the current stream -- the per-utterance path of
        ``MimiEncoder.encode_audio_chunk``.  The same codes as ``encode_int32`` on a device copy."""
        K = self._check_k(num_quantizers)
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"audio must be a non-empty [batch, length] array, got {tuple(a.shape)}")
        B, L = a.shape
        out = np.empty((B, K, encoded_length(L, self.config)), dtype=np.int32)
        _lib.check(self._lib.mimi_encode_host(self._h, ctypes.c_void_p(a.ctypes.data), B, L, K,
                                              ctypes.c_void_p(out.ctypes.data), self._stream()))
        return out

    def encode_async(self, audio: torch.Tensor, num_quantizers: int, out: Optional[torch.Tensor] = None
                     ) -> "EncodeTicket":
        """Enqueue an encode of device f32 [B, L] on the current stream and return without waiting
        (``mimi_encode_async``); ``ticket.wait()`` returns the int32 [B, K, T] codes once they are final (the
        f16x3 overflow check runs there).  The ticket keeps ``audio`` alive until then."""
        K = self._check_k(num_quantizers)
        audio = self._device_audio(audio)
        B, L = audio.shape
        out = self._out(B, K, encoded_length(L, self.config), out)
        t = ctypes.c_int64()
        _lib.check(self._lib.mimi_encode_async(self._h, ctypes.c_void_p(audio.data_ptr()), B, L, K,
                                               ctypes.c_void_p(out.data_ptr()), self._stream(), ctypes.byref(t)))
        return EncodeTicket(self, t.value, out, audio)

    def encode_ragged_async(self, audio: torch.Tensor, lengths, num_quantizers: int,
                            out: Optional[torch.Tensor] = None) -> "EncodeTicket":
        """Ragged batch (``mimi_encode_ragged_async``): item b = ``audio[b, :lengths[b]]`` of a device f32 [B, Lmax]
        tensor, encoded exactly as it would be alone at its own length (bit for bit), in one pass that skips every
        item's rows past its length.  ``ticket.wait()`` returns int32 [B, K, T(Lmax)]; item b's codes are
        ``[:, :encoded_length(lengths[b])]`` (the frames past are unspecified)."""
        K = self._check_k(num_quantizers)
        audio = self._device_audio(audio)
        B, L = audio.shape
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if lens.shape != (B,) or (B and (int(lens.min()) < 1 or int(lens.max()) > L)):
            raise ValueError(f"lengths must be {B} values in [1, {L}]")
        out = self._out(B, K, encoded_length(L, self.config), out)
        t = ctypes.c_int64()
        _lib.check(self._lib.mimi_encode_ragged_async(self._h, ctypes.c_void_p(audio.data_ptr()),
                                                      ctypes.c_void_p(lens.ctypes.data), B, L, K,
                                                      ctypes.c_void_p(out.data_ptr()), self._stream(),
                                                      ctypes.byref(t)))
        return EncodeTicket(self, t.value, out, audio)

    def encode_ragged(self, audio: torch.Tensor, lengths, num_quantizers: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.encode_ragged_async(audio, lengths, num_quantizers, out).wait()

    def quantize(self, embedding: torch.Tensor, num_quantizers: int) -> torch.Tensor:
        """Quantizer alone on a pre-quantizer embedding [B, 512, T] -> int64 codes [B, K, T]."""
        B, C, T = embedding.shape
        emb = embedding.to(device=self.device, dtype=torch.float32).permute(0, 2, 1).contiguous()
        codes = torch.empty((num_quantizers, B * T), dtype=torch.int32, device=self.device)
        with self._lock:
            _lib.check(self._lib.mimi_rvq_encode(self._h, ctypes.c_void_p(emb.data_ptr()), B * T, num_quantizers,
                                                 ctypes.c_void_p(codes.data_ptr()), self._stream()))
        return codes.view(num_quantizers, B, T).permute(1, 0, 2).long()

    # ---- decode --------------------------------------------------------------------------------
    def get_decoded_length(self, frames: int) -> int:
        n = 2 * int(frames)
        for r in self.config.upsampling_ratios:
            n *= r
        return n

    def decode_workspace_bytes(self, batch: int, frames: int) -> int:
        """Bytes of decode's workspace for this shape at the current taps setting (``mimi_decode_workspace_bytes``)."""
        return int(self._lib.mimi_decode_workspace_bytes(self._h, int(batch), int(frames)))

    def _require_decode(self):
        if not self.decode_enabled:
            raise RuntimeError("this MimiHipModel holds the encode path only: construct it with decode=True "
                               "(MimiHipModel(..., decode=True) / from_pretrained(..., decode=True)) to decode")

    def _decode_codes(self, audio_codes) -> torch.Tensor:
        """The ``[B, K, T]`` codes of a decode call as a tensor, K within the model's levels."""
        self._require_decode()
        if not torch.is_tensor(audio_codes):
            audio_codes = torch.as_tensor(np.asarray(audio_codes))
        if audio_codes.dim() != 3:
            raise ValueError(f"audio_codes must be [batch, num_quantizers, frames], got {tuple(audio_codes.shape)}")
        K = audio_codes.shape[1]
        if K > self.config.num_quantizers or K < 1:
            raise ValueError(f"The number of quantizers (i.e codebooks) must be in [1, {self.config.num_quantizers}], "
                             f"but is currently {K}.")
        return audio_codes

    def _decode_call(self, fn, *args):
        """One decode entry point of the library on this model's stream; its MIMI_ERR_INVALID_ARGUMENT (a code outside
        ``[0, codebook_size)``, K over the levels) is a ``ValueError``."""
        try:
            _lib.check(fn(self._h, *args, self._stream()))
        except _lib.MimiHipError as err:
            if err.status == 1:
                raise ValueError(str(err)) from None
            raise

    def decode(self, audio_codes: torch.Tensor, padding_mask: Optional[torch.Tensor] = None,
               decoder_past_key_values=None, return_dict: Optional[bool] = None):
        """``MimiModel.decode`` (``TF/modeling_mimi.py:1408-1458``): int64 / int32 codes ``[B, K, T]`` on any device
        -> ``MimiDecoderOutput(audio_values [B, 1, 1920 T] float32 on the model's device, None)``; truncated to
        ``padding_mask.shape[-1]`` when that is shorter (``:1446-1447``)."""
        self._require_decode()
        if decoder_past_key_values is not None:
            raise NotImplementedError("streaming decode (KV cache) is not on the batch path")
        audio_codes = self._decode_codes(audio_codes)
        B, K, T = audio_codes.shape
        audio = torch.empty((B, 1, self.get_decoded_length(T)), dtype=torch.float32, device=self.device)
        if B and T:
            codes = audio_codes.to(device=self.device, dtype=torch.int32).contiguous()
            self._decode_call(self._lib.mimi_decode, ctypes.c_void_p(codes.data_ptr()), B, T, K,
                              ctypes.c_void_p(audio.data_ptr()))
        if padding_mask is not None and padding_mask.shape[-1] < audio.shape[-1]:
            audio = audio[..., : padding_mask.shape[-1]]
        if return_dict is False:
            return (audio, None)
        return MimiDecoderOutput(audio)

    def decode_stream(self, batch: int = 1, num_quantizers: Optional[int] = None,
                      max_step_frames: int = 16) -> DecodeStream:
        """A streaming decode of ``batch`` items (``mimi_decode_stream_*``): ``.step(codes[B, K, n])`` returns the
        ``1920 n`` samples of the next ``n <= max_step_frames`` frames of all of them, ``.step(codes[m, K, n],
        slots=[...])`` of the listed slots only, each slot at its own position.  Several streams may be open on one
        model and interleave with ``decode`` / ``decode_ragged`` / ``encode``."""
        self._require_decode()
        K = self.config.num_quantizers if num_quantizers is None else int(num_quantizers)
        if K > self.config.num_quantizers or K < 1:
            raise ValueError(f"The number of quantizers (i.e codebooks) must be in [1, {self.config.num_quantizers}], "
                             f"but is currently {K}.")
        if int(batch) < 1 or int(max_step_frames) < 1:
            raise ValueError(f"batch and max_step_frames must be >= 1, got {batch} and {max_step_frames}")
        st = DecodeStream(self, batch, K, max_step_frames)
        self._streams.add(st)
        return st

    def decode_ragged_workspace_bytes(self, lengths) -> int:
        """Bytes of a ragged decode's workspace at the current taps setting (``mimi_decode_ragged_workspace_bytes``)."""
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        return int(self._lib.mimi_decode_ragged_workspace_bytes(self._h, ctypes.c_void_p(lens.ctypes.data), lens.size))

    def decode_ragged(self, audio_codes: torch.Tensor, lengths, out: Optional[torch.Tensor] = None):
        """Mixed-length batch in one pass (``mimi_decode_ragged``): item b = ``audio_codes[b, :, :lengths[b]]`` of an
        int64 / int32 ``[B, K, Tmax]`` tensor on any device (the codes past an item's length are never read).
        Returns a list of B float32 device tensors ``[1, 1920 lengths[b]]``, views of one ``[B, 1920 Tmax]`` buffer
        (``out`` if given: the samples past an item's length are left as they were).  Item b is bit for bit
        ``decode(audio_codes[b:b + 1, :, :lengths[b]]).audio_values[0]``."""
        audio_codes = self._decode_codes(audio_codes)
        B, K, T = audio_codes.shape
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if lens.shape != (B,) or (B and (int(lens.min()) < 1 or int(lens.max()) > T)):
            raise ValueError(f"lengths must be {B} values in [1, {T}]")
        L = self.get_decoded_length(T)
        if out is None:
            out = torch.empty((B, L), dtype=torch.float32, device=self.device)
        elif (tuple(out.shape) != (B, L) or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{B}, {L}] tensor on {self.device}")
        if B:
            codes = audio_codes.to(device=self.device, dtype=torch.int32).contiguous()
            self._decode_call(self._lib.mimi_decode_ragged, ctypes.c_void_p(codes.data_ptr()),
                              ctypes.c_void_p(lens.ctypes.data), B, T, K, ctypes.c_void_p(out.data_ptr()))
        return [out[b:b + 1, : self.get_decoded_length(int(lens[b]))] for b in range(B)]

    def dequantize(self, codes: torch.Tensor) -> torch.Tensor:
        """Quantizer decode alone (``mimi_rvq_decode``): codes [B, K, T] -> float32 embedding [B, 512, T], the mirror
        of ``quantize``."""
        codes = self._decode_codes(codes)
        B, K, T = codes.shape
        c = codes.to(device=self.device, dtype=torch.int32).permute(1, 0, 2).contiguous()  # [K][B * T]
        emb = torch.empty((B * T, self.config.hidden_size), dtype=torch.float32, device=self.device)
        self._decode_call(self._lib.mimi_rvq_decode, ctypes.c_void_p(c.data_ptr()), B * T, K,
                          ctypes.c_void_p(emb.data_ptr()))
        return emb.view(B, T, -1).permute(0, 2, 1)

    # ---- instrumentation ------------------------------------------------------------------------
    def set_precision(self, mode: str):
        """'f16x3' (default: fp32 emulated on the fp16 matrix cores, 2 planes at calibrated fixed scales),
        'bf16x6' (3 bf16 planes), 'f32' (fp32 MFMA) or 'bf16x3' (2 bf16 planes, ~1e-5)."""
        _lib.check(self._lib.mimi_set_precision(self._h, _lib.PRECISIONS[mode]))

    @property
    def precision(self) -> str:
        v = self._lib.mimi_get_precision(self._h)
        return {i: k for k, i in _lib.PRECISIONS.items()}[v]

    def calibrate(self):
        """Run the f16x3 activation-scale calibration now (otherwise it runs inside the first f16x3 encode)."""
        _lib.check(self._lib.mimi_calibrate(self._h))

    @property
    def f16_reruns(self) -> int:
        """Encodes that took the f16x3 overflow fallback (per-item re-encode, bf16x6 where an item overflows)."""
        return int(self._lib.mimi_f16_reruns(self._h))

    @property
    def rvq_chain_reruns(self) -> int:
        """Encodes re-run on the per-level RVQ kernels because the persistent RVQ chain gave up (never returned)."""
        return int(self._lib.mimi_rvq_chain_reruns(self._h))

    def set_graphs(self, enable: bool = True):
        """hipGraph replay of repeated f16x3 encode shapes (default on; identical codes, fewer launches)."""
        _lib.check(self._lib.mimi_set_graphs(self._h, int(enable)))

    @property
    def graph_replays(self) -> int:
        return int(self._lib.mimi_graph_replays(self._h))

    @property
    def graph_captures(self) -> int:
        """Graphs captured so far (a graph retired by a workspace or RoPE-table reallocation is captured again)."""
        return int(self._lib.mimi_graph_captures(self._h))

    @property
    def lane_encodes(self):
        """Encodes submitted to each of the engine's two lanes (encodes that take no lane count in lane 0)."""
        return tuple(int(self._lib.mimi_lane_encodes(self._h, i)) for i in range(2))

    def set_option(self, key: str, value: int):
        """Kernel-variant option (identical codes either way): "stage0_fused" 0 = stage-0 block and down conv 0 as
        two kernels, 1 = one fused kernel (default); "ln_fused" 0 = LayerNorm launches before q/k/v and fc1, on small
        grids (batch 1-4) 1 = fc1 computes the LayerNorm of its rows itself (default), 2 = fc1 and q/k/v do."""
        _lib.check(self._lib.mimi_set_option(self._h, key.encode(), int(value)))

    def act_scales(self):
        """f16x3 diagnostics: {tensor: (fixed scale, max|x| of the last encode, headroom 2^15 / (scale * max))}."""
        n = 256
        names = ctypes.create_string_buffer(64 * n)
        sc = (ctypes.c_float * n)()
        mx = (ctypes.c_float * n)()
        cnt = ctypes.c_int32()
        _lib.check(self._lib.mimi_act_scales(self._h, n, names, sc, mx, ctypes.byref(cnt)))
        out = {}
        for i in range(cnt.value):
            name = names.raw[64 * i:64 * (i + 1)].split(b"\0", 1)[0].decode()
            head = 32768.0 / (sc[i] * mx[i]) if sc[i] > 0 and mx[i] > 0 else float("inf")
            out[name] = (sc[i], mx[i], head)
        return out

    def set_profiling(self, enable=True):
        """True / 1: events between every stage; 2: around each encode's first stage only; False / 0: off."""
        _lib.check(self._lib.mimi_set_profiling(self._h, int(enable)))

    def profile_reset(self):
        _lib.check(self._lib.mimi_profile_reset(self._h))

    def profile_read(self):
        n = 64
        names = ctypes.create_string_buffer(128 * n)
        ms = (ctypes.c_double * n)()
        launches = (ctypes.c_int64 * n)()
        fb = (ctypes.c_double * (2 * n))()
        cnt = ctypes.c_int32()
        _lib.check(self._lib.mimi_profile_read(self._h, n, names, ms, launches, fb, ctypes.byref(cnt)))
        out = {}
        for i in range(cnt.value):
            nm = names.raw[128 * i:128 * (i + 1)].split(b"\0", 1)[0].decode()
            stage, _, kernel = nm.partition("|")
            key, j = stage, 2
            while key in out:  # one stage run by two kernel symbols (e.g. the last layer's fc2): "fc2#2"
                key, j = f"{stage}#{j}", j + 1
            out[key] = dict(kernel=kernel, ms=ms[i], launches=launches[i], flops=fb[2 * i], bytes=fb[2 * i + 1])
        return out

    def profile_sequence(self):
        """[(stage, kernel symbol)] of the last profiled encode in launch order (mimi_profile_sequence)."""
        n = 512
        names = ctypes.create_string_buffer(128 * n)
        cnt = ctypes.c_int32()
        _lib.check(self._lib.mimi_profile_sequence(self._h, n, names, ctypes.byref(cnt)))
        out = []
        for i in range(cnt.value):
            nm = names.raw[128 * i:128 * (i + 1)].split(b"\0", 1)[0].decode()
            stage, _, kernel = nm.partition("|")
            out.append((stage, kernel))
        return out

    def set_taps(self, enable: bool = True):
        _lib.check(self._lib.mimi_set_taps(self._h, int(enable)))

    def get_tap(self, name: str) -> np.ndarray:
        numel = ctypes.c_int64()
        dims = (ctypes.c_int64 * 3)()
        _lib.check(self._lib.mimi_get_tap(self._h, name.encode(), None, 0, ctypes.byref(numel), dims))
        buf = np.empty(numel.value, dtype=np.float32)
        _lib.check(self._lib.mimi_get_tap(self._h, name.encode(), ctypes.c_void_p(buf.ctypes.data), buf.size,
                                          ctypes.byref(numel), dims))
        return buf.reshape(dims[0], dims[1], dims[2])
