"""Code <-> character serialisation, vectorised.

Same results as ``/root/reference/librispeech-mimi/utils.py:18-55`` (``codes_to_chars`` /
``chars_to_codes``; identical copies in the other ``*/utils.py``): codebook k's code c becomes the
character ``chr(unicode_offset + k*codebook_size + c)``, frames interleaved codebook-fastest
(``codes.T.reshape(-1)``).  The reference builds the string with a per-character ``chr`` loop
(``utils.py:36``), the host bottleneck at GPU encode rates; here the code points are formed in numpy and
the string is decoded from UTF-32 in one call.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

UNICODE_OFFSET: int = 0xE000
NUM_CODEBOOKS: int = 8
CODEBOOK_SIZE: int = 2048


def codes_to_codepoints(codes: Union[List[List[int]], np.ndarray, torch.Tensor], codebook_size: int,
                        copy_before_conversion: bool = True, unicode_offset: int = UNICODE_OFFSET) -> np.ndarray:
    """The code points ``codes_to_chars`` turns into characters, flat, in string order."""
    if isinstance(codes, list):
        codes = np.array(codes)
        copy_before_conversion = False
    elif isinstance(codes, torch.Tensor):
        codes = codes.cpu().numpy()
    if len(codes.shape) != 2:
        raise ValueError("codes must be a 2D array of shape (num_codebooks, seq_length).")
    if copy_before_conversion:
        codes = codes.copy()
    # the offset add stays in the codes' own dtype, row by row, exactly as the reference does it
    # (in place when copy_before_conversion=False; same overflow behaviour for narrow dtypes)
    for i in range(codes.shape[0]):
        codes[i] += unicode_offset + i * codebook_size
    return np.ascontiguousarray(codes.T.reshape(-1))


def codes_to_chars(codes: Union[List[List[int]], np.ndarray, torch.Tensor], codebook_size: int,
                   copy_before_conversion: bool = True, unicode_offset: int = UNICODE_OFFSET) -> str:
    flat = codes_to_codepoints(codes, codebook_size, copy_before_conversion, unicode_offset)
    if flat.size == 0:
        return ""
    if flat.dtype.kind not in "iu":
        return "".join([chr(c) for c in flat])  # chr() raises for floats exactly as the reference does
    lo, hi = int(flat.min()), int(flat.max())
    if lo < 0 or hi > 0x10FFFF or ((flat >= 0xD800) & (flat <= 0xDFFF)).any():
        return "".join([chr(c) for c in flat])  # out-of-range / surrogate code points: reference semantics
    return flat.astype("<u4").tobytes().decode("utf-32-le")


def chars_to_codes(chars: str, num_codebooks: int, codebook_size: int, return_tensors: Optional[str] = None,
                   unicode_offset: int = UNICODE_OFFSET):
    cp = np.frombuffer(chars.encode("utf-32-le"), dtype="<u4").astype(np.int64)
    codes = cp.reshape(-1, num_codebooks).T.copy()
    codes -= (unicode_offset + np.arange(num_codebooks, dtype=np.int64) * codebook_size)[:, None]
    if return_tensors is None:
        return codes.tolist()
    if return_tensors == "pt":
        return torch.tensor(codes)
    return codes


def audio_to_str(audio_numpy: np.ndarray, mimi_model, device: str) -> str:
    """``utils.audio_to_str`` (``librispeech-mimi/utils.py:58-69``) over the HIP model."""
    audio_tensor = torch.tensor(audio_numpy).to(device).unsqueeze(0)
    if len(audio_tensor.shape) == 2:
        audio_tensor = audio_tensor.unsqueeze(1)
    with torch.no_grad():
        audio_codes = mimi_model.encode(audio_tensor)
    codes = audio_codes[0][0].cpu()
    codes = codes[:NUM_CODEBOOKS, :]
    return codes_to_chars(codes, codebook_size=CODEBOOK_SIZE)


def str_to_audio(audio_str: str, mimi_model, device: str) -> np.ndarray:
    """``utils.str_to_audio`` (``librispeech-mimi/utils.py:72-81``) over the HIP model (built with ``decode=True``):
    the string's code points back to codes ``[1, 8, T]``, decoded; returns the ``[1, 1920 T]`` float32 array the
    reference returns (``.audio_values[0]``)."""
    codes = chars_to_codes(audio_str, num_codebooks=NUM_CODEBOOKS, codebook_size=CODEBOOK_SIZE, return_tensors="pt")
    codes = codes.to(device).unsqueeze(0)
    with torch.no_grad():
        audio_decoded = mimi_model.decode(codes).audio_values[0]
    return audio_decoded.cpu().numpy()


# strs_to_audio's default batch budget in 12.5 Hz frames: 320 s of audio, the B = 32 x 10 s shape the decode rate
# plateaus at.  The decode workspace takes ~0.94 MiB per frame (the [1920 T][64] tensors in front of the last conv, in
# both ping-pong regions), so this budget costs ~3.7 GiB of device memory; it grows with the budget, not with the
# number of strings
MAX_BATCH_FRAMES = 4000


def strs_to_audio(audio_strs: Sequence[str], mimi_model, device: str,
                  max_batch_frames: int = MAX_BATCH_FRAMES) -> List[np.ndarray]:
    """``[str_to_audio(s, mimi_model, device) for s in audio_strs]``, bit for bit, at the batched rate: the strings
    are cut, in order, into consecutive ragged batches whose frames sum to at most ``max_batch_frames`` (a single
    string longer than that runs alone) and each batch is one ``mimi_model.decode_ragged`` pass.  Returns float32
    arrays ``[1, 1920 T_i]`` in input order; an empty string gives a ``(1, 0)`` array and is not sent to the engine."""
    if max_batch_frames < 1:
        raise ValueError("max_batch_frames must be at least 1")
    items = [chars_to_codes(s, num_codebooks=NUM_CODEBOOKS, codebook_size=CODEBOOK_SIZE, return_tensors="np")
             for s in audio_strs]
    out: List[Optional[np.ndarray]] = [None] * len(items)
    batch: List[int] = []

    def flush():
        if not batch:
            return
        lens = [items[i].shape[1] for i in batch]
        codes = np.zeros((len(batch), NUM_CODEBOOKS, max(lens)), dtype=np.int64)
        for j, i in enumerate(batch):
            codes[j, :, : lens[j]] = items[i]
        with torch.no_grad():
            audio = mimi_model.decode_ragged(torch.from_numpy(codes).to(device), lens)
        for j, i in enumerate(batch):
            out[i] = audio[j].cpu().numpy()
        batch.clear()

    frames = 0
    for i, c in enumerate(items):
        T = c.shape[1]
        if T == 0:
            out[i] = np.zeros((1, 0), dtype=np.float32)
            continue
        if batch and frames + T > max_batch_frames:
            flush()
            frames = 0
        batch.append(i)
        frames += T
    flush()
    return out


def ids_to_audio(ids, seq_offsets, encoder, mimi_model, max_batch_frames: int = MAX_BATCH_FRAMES) -> List[np.ndarray]:
    """BPE token ids in device memory -> audio, without the ids or the codes leaving the device:
    ``encoder.decode_device(ids, seq_offsets)`` (a ``bpe.Encoder`` of 8 codebooks; ``ids`` / ``seq_offsets`` as
    ``encode_device`` returns them), then the sequences are cut, in order, into consecutive ragged batches exactly as
    ``strs_to_audio`` cuts its strings, each batch one ``mimi_model.decode_ragged`` on a slice of the device codes.
    Returns float32 arrays ``[1, 1920 T_i]`` in input order; a sequence of zero frames gives a ``(1, 0)`` array and is
    not sent to the engine.  Bit for bit ``strs_to_audio`` of the strings of ``encoder.decode_ids``' codes."""
    if max_batch_frames < 1:
        raise ValueError("max_batch_frames must be at least 1")
    if encoder.num_codebooks != NUM_CODEBOOKS or encoder.codebook_size != CODEBOOK_SIZE:
        raise ValueError(f"the encoder must have {NUM_CODEBOOKS} codebooks of {CODEBOOK_SIZE} codes")
    codes, lens = encoder.decode_device(ids, seq_offsets)
    out: List[Optional[np.ndarray]] = [None] * len(lens)
    batch: List[int] = []

    def flush():
        if not batch:
            return
        blens = [int(lens[i]) for i in batch]
        # a batch is consecutive but for zero-frame sequences: a slice when it has none inside, else a gather
        rows = codes[batch[0]:batch[-1] + 1] if batch[-1] - batch[0] + 1 == len(batch) else codes[batch]
        with torch.no_grad():
            audio = mimi_model.decode_ragged(rows[:, :, :max(blens)], blens)
        for j, i in enumerate(batch):
            out[i] = audio[j].cpu().numpy()
        batch.clear()

    frames = 0
    for i, T in enumerate(lens):
        T = int(T)
        if T == 0:
            out[i] = np.zeros((1, 0), dtype=np.float32)
            continue
        if batch and frames + T > max_batch_frames:
            flush()
            frames = 0
        batch.append(i)
        frames += T
    flush()
    return out


class IdsToAudioStream:
    """BPE token ids -> samples chunk by chunk, nothing leaving the device in between: an ``IdStream``
    (``encoder.decode_stream``, ids -> the whole frames they complete) in front of a ``DecodeStream``
    (``mimi_model.decode_stream``, frames -> samples), ``batch`` slots each, slot ``b`` of one feeding slot ``b`` of the
    other.  ``encoder``: a ``bpe.Encoder`` whose ``num_codebooks`` is the decode stream's ``num_quantizers`` and whose
    ``codebook_size`` is the model's; ``mimi_model`` is built with ``decode=True``.  A slot's samples, end to end, are
    bitwise those of a ``batch=1`` ``DecodeStream`` stepped over ``encoder.decode_ids`` of everything the slot was fed
    since its reset, whatever the split into steps and whatever its neighbours do.  A context manager; ``close()``
    closes both streams."""

    def __init__(self, encoder, mimi_model, batch: int, max_step_ids: int, max_step_frames: int = 16):
        if encoder.codebook_size != mimi_model.config.codebook_size:
            raise ValueError(f"the encoder has codebooks of {encoder.codebook_size} codes, the model of "
                             f"{mimi_model.config.codebook_size}")
        self.batch = int(batch)
        self.ids = encoder.decode_stream(batch, max_step_ids)
        try:
            self.audio = mimi_model.decode_stream(batch, num_quantizers=encoder.num_codebooks,
                                                  max_step_frames=max_step_frames)
        except Exception:
            self.ids.close()
            raise
        self.frame_samples = int(mimi_model.get_decoded_length(1))
        self._device = mimi_model.device
        self.last_frames: List[int] = []

    @property
    def positions(self) -> List[int]:
        """Frames each slot has emitted since its reset (the decode stream's positions)."""
        return self.audio.positions

    @property
    def pending(self) -> List[int]:
        """Codes waiting in each slot's partial frame (``IdStream.pending``)."""
        return self.ids.pending

    def step(self, ids, slots: Optional[Sequence[int]] = None, counts: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """``IdStream.step(ids, slots, counts)``, then the items that completed at least one frame go through
        ``DecodeStream.step(codes, slots=, frames=)`` in column windows of at most ``max_step_frames`` frames; a
        window leaves out the items that have no frame left by then.  Returns one float32 device tensor ``[1920
        frames_i]`` per item, empty for an item that completed no frame; ``last_frames`` holds the ``frames_i``.
        Errors are those of the two steps; an id step that raises leaves the decode stream untouched."""
        codes, frames = self.ids.step(ids, slots=slots, counts=counts)
        slots = list(range(self.batch)) if slots is None else [int(x) for x in slots]
        F, W = self.frame_samples, self.audio.max_step_frames
        out = [torch.empty(F * f, dtype=torch.float32, device=self._device) for f in frames]
        at = 0
        while True:
            sel = [i for i, f in enumerate(frames) if f > at]
            if not sel:
                break
            n = [min(W, frames[i] - at) for i in sel]
            rows = codes if len(sel) == len(frames) else codes[sel]
            audio = self.audio.step(rows[:, :, at:at + max(n)], slots=[slots[i] for i in sel], frames=n)
            for j, i in enumerate(sel):
                out[i][F * at:F * (at + n[j])] = audio[j, 0, :F * n[j]]
            at += max(n)
        self.last_frames = list(frames)
        return out

    def reset(self, slot: Optional[int] = None):
        """Both streams back to fresh, all slots or one: the pending partial frame is discarded, the next samples are
        those of a new session."""
        self.ids.reset(slot)
        self.audio.reset(slot)

    def close(self):
        self.ids.close()
        self.audio.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
