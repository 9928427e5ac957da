"""CPU: the layout of a ragged stream step (``mimi_stream_step_layout``, host-only: no device, no engine).

Both directions.  A stage with ``H`` carry rows and ``f`` rows per frame holds item ``i``'s block ``[H + f frames[i]][C]`` at row
``H i + f off[i]`` of one packed tensor (``off`` = the prefix sum of ``frames``).  The tables the entry returns are
compared with that statement written out in Python; the blocks are disjoint, in order and 16-byte aligned; the
workspace is sized by the sum of the counts; every bad argument is refused.
"""
import ctypes

import pytest

from mimi_hip import _lib
from mimi_hip.config import MimiConfig

S = _lib.STREAM_MAX_STAGES
# (the last: the big step of tests/stream_scale_ref.py at m = 129 -- item j is session 13 j + 16 mod 129 with
# 1 + (5 i mod 7) frames -- written out here so that this file stays host-only; tests/test_stream_scale_ref.py holds
# the schedule to the same expression)
SCALE = [1 + (5 * ((13 * j + 16) % 129)) % 7 for j in range(129)]
assert sum(SCALE) == 515
COUNTS = ([1], [7, 1, 3], [1, 1, 12], [3, 3, 3, 3], [12] * 5, [2, 11], [1, 2, 4, 1, 2, 4, 4, 1], SCALE)


def count_id(frames):
    return str(frames) if len(frames) < 16 else f"{len(frames)}items{sum(frames)}frames"


def layout(frames, nmax=None, direction=_lib.STREAM_DECODE, cfg=None, taps=0, m=None, tweak=None):
    """(status, stages [(H, f, C, byte offset)], first rows [stage][item], row counts [stage][item], bytes)
    ``tweak(c)`` edits the C configuration before the call."""
    lib = _lib.load()
    c = _lib.config_from_py(cfg or MimiConfig())
    if tweak:
        tweak(c)
    m = len(frames) if m is None else m
    nmax = max(frames, default=1) if nmax is None else nmax
    i32, i64 = ctypes.c_int32 * S, ctypes.c_int64 * S
    ns, H, f, C, off = ctypes.c_int32(), i32(), i32(), i32(), i64()
    rows, cnt = (ctypes.c_int64 * (S * max(m, 1)))(), (ctypes.c_int64 * (S * max(m, 1)))()
    ws = ctypes.c_int64()
    rc = lib.mimi_stream_step_layout(ctypes.byref(c), direction, (ctypes.c_int32 * max(len(frames), 1))(*frames), m,
                                     nmax, taps, ctypes.byref(ns), H, f, C, off, rows, cnt, ctypes.byref(ws))
    if rc:
        return rc, None, None, None, None
    n = ns.value
    return (rc, [(H[j], f[j], C[j], off[j]) for j in range(n)], [[rows[j * m + i] for i in range(m)] for j in range(n)],
            [[cnt[j * m + i] for i in range(m)] for j in range(n)], ws.value)


def decode_stages(cfg):
    """The decode stream's carry stages as DESIGN 3.7.1 lists them: (H, f, C)."""
    C = cfg.num_filters << len(cfg.upsampling_ratios)
    st, f = [(1, 1, cfg.hidden_size), (cfg.kernel_size - 1, 2, cfg.hidden_size)], 2
    for r in cfg.upsampling_ratios:
        st.append((1, f, C))
        f, C = f * r, C // 2
        st.append((2, f, C))
    st.append((cfg.last_kernel_size - 1, f, C))
    return st


def encode_stages(cfg):
    """The encode stream's carry stages as DESIGN 3.7.2 lists them: conv 0's 8 samples (one row per item, no chunk rows:
    f = 0), per ratio the residual block's input (2 carry rows) and the down conv's (r), the final conv's, the
    downsample's."""
    C, f, st = cfg.num_filters, 2 * 960, [(1, 0, 8)]
    assert f == 2 * __import__("math").prod(cfg.upsampling_ratios)
    for r in reversed(cfg.upsampling_ratios):
        st += [(cfg.residual_kernel_size - 1, f, C), (r, f, C)]
        f, C = f // r, 2 * C
    return st + [(cfg.last_kernel_size - 1, f, C), (2, f, cfg.hidden_size)]


DIRECTIONS = [(_lib.STREAM_DECODE, decode_stages), (_lib.STREAM_ENCODE, encode_stages)]


@pytest.mark.parametrize("direction,stages_of", DIRECTIONS, ids=["decode", "encode"])
@pytest.mark.parametrize("frames", COUNTS, ids=count_id)
def test_tables_are_the_stated_layout(frames, direction, stages_of):
    cfg = MimiConfig()
    rc, stages, first, count, ws = layout(frames, direction=direction)
    assert rc == 0
    assert [s[:3] for s in stages] == stages_of(cfg)
    off = [sum(frames[:i]) for i in range(len(frames))]
    for (H, f, C, _), rows, cnt in zip(stages, first, count):
        assert rows == [H * i + f * off[i] for i in range(len(frames))]
        assert cnt == [H + f * n for n in frames]


@pytest.mark.parametrize("direction", [_lib.STREAM_DECODE, _lib.STREAM_ENCODE], ids=["decode", "encode"])
@pytest.mark.parametrize("frames", COUNTS, ids=count_id)
def test_blocks_are_disjoint_in_order_and_aligned(frames, direction):
    rc, stages, first, count, ws = layout(frames, direction=direction)
    assert rc == 0
    spans = []
    for (H, f, C, base), rows, cnt in zip(stages, first, count):
        assert base % 16 == 0
        for i in range(len(frames)):
            lo = base + rows[i] * C * 4
            assert lo % 16 == 0
            if i:
                assert rows[i] == rows[i - 1] + cnt[i - 1]  # back to back: block i starts where block i - 1 ends
        spans.append((base, base + (rows[-1] + cnt[-1]) * C * 4))
    for (lo, hi), (nlo, _) in zip(spans, spans[1:]):
        assert lo < hi <= nlo  # the stages' tensors in order, none overlapping
    assert spans[-1][1] <= ws


@pytest.mark.parametrize("direction", [_lib.STREAM_DECODE, _lib.STREAM_ENCODE], ids=["decode", "encode"])
@pytest.mark.parametrize("taps", [0, 1])
def test_workspace_is_sized_by_the_sum(taps, direction):
    for frames in COUNTS:
        m, nmax = len(frames), max(frames)
        ws = layout(frames, taps=taps, direction=direction)[4]
        uniform = layout([nmax] * m, taps=taps, direction=direction)[4]
        assert ws <= uniform
        assert (ws == uniform) == (frames == [nmax] * m)
        # ... and by nothing but the sum: the same sum in one item less
        if m > 1 and frames[0] + frames[1] <= 12:
            merged = [frames[0] + frames[1]] + frames[2:]
            assert (layout(merged, nmax=12, taps=taps, direction=direction)[4]
                    < layout(frames, nmax=12, taps=taps, direction=direction)[4])  # one carry less


def test_small_config():
    cfg = MimiConfig(sliding_window=5)
    rc, stages, first, count, _ = layout([2, 11], cfg=cfg)
    assert rc == 0 and [s[:3] for s in stages] == decode_stages(cfg)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    assert layout([1, 2], direction=2)[0] == 1
    assert layout([1, 2], direction=-1)[0] == 1
    assert layout([], m=0)[0] == 1
    assert layout([1], m=-1)[0] == 1
    assert layout([1], m=65536)[0] == 1
    assert layout([0, 2])[0] == 1
    assert layout([-1, 2])[0] == 1
    assert layout([1, 3], nmax=2)[0] == 1
    assert layout([1, 2], nmax=0)[0] == 1
    assert layout([1, 2], nmax=(1 << 20) + 1)[0] == 1
    # a configuration whose stages would have negative carries or rates
    def ratio(i, v):
        return lambda c: c.upsampling_ratios.__setitem__(i, v)

    for name, tweak in (("kernel_size", lambda c: setattr(c, "kernel_size", 0)),
                        ("last_kernel_size", lambda c: setattr(c, "last_kernel_size", 0)),
                        ("hidden_size", lambda c: setattr(c, "hidden_size", 0)),
                        ("hidden_size % 4", lambda c: setattr(c, "hidden_size", 510)),
                        ("num_filters", lambda c: setattr(c, "num_filters", 0)),
                        ("num_ratios", lambda c: setattr(c, "num_ratios", 0)),
                        ("ratio 0", ratio(1, 0)), ("ratio < 0", ratio(2, -5))):
        assert layout([1, 2], tweak=tweak)[0] == 1, name
    # NULL pointers
    c = _lib.config_from_py(MimiConfig())
    i32, i64 = ctypes.c_int32 * S, ctypes.c_int64 * S
    good = [ctypes.byref(c), 0, (ctypes.c_int32 * 2)(1, 2), 2, 2, 0, ctypes.pointer(ctypes.c_int32()), i32(), i32(), i32(),
            i64(), (ctypes.c_int64 * (2 * S))(), (ctypes.c_int64 * (2 * S))(), ctypes.pointer(ctypes.c_int64())]
    assert lib.mimi_stream_step_layout(*good) == 0
    for k in (0, 2, 6, 7, 8, 9, 10, 11, 12, 13):
        args = list(good)
        args[k] = None
        assert lib.mimi_stream_step_layout(*args) == 1, k
    # the same through the encode direction
    assert layout([0, 2], direction=_lib.STREAM_ENCODE)[0] == 1
    assert layout([1, 3], nmax=2, direction=_lib.STREAM_ENCODE)[0] == 1
    assert layout([1, 2], direction=_lib.STREAM_ENCODE, tweak=ratio(0, 0))[0] == 1
    assert layout([1, 2], direction=_lib.STREAM_ENCODE, tweak=lambda c: setattr(c, "residual_kernel_size", 0))[0] == 1
    assert layout([1, 2], direction=_lib.STREAM_ENCODE, tweak=lambda c: setattr(c, "downsample_stride", 0))[0] == 1
