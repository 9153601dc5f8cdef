"""Objective quality measures on the GPU (cal_metrics.py of the reference).

`stoi` is the short-time objective intelligibility of Taal, Hendriks, Heusdens and Jensen (2011),
which the reference takes from the CPU library pystoi one file at a time (cal_metrics.py:57-63);
here a batch of rows is scored by csrc/stoi.hip without leaving the stream. PESQ, the reference's
other measure, is the ITU's program and has no counterpart here.

One deviation: the published implementation brings its input to 10 kHz with an Octave-style
Kaiser-windowed polyphase filter, which cannot be observed here; this one resamples with
encx.ops.resample (torchaudio.transforms.Resample's default windowed sinc), the filter of every
other rate conversion in this package. At 10 kHz input nothing is resampled.
"""
import math
import typing as tp

import torch

from . import ops
from ._lib import call, lib, ptr, stream

FS = 10000          # the rate the measure is defined at
# the score of a row with fewer than 30 analysis frames (cal_metrics.py:132): 1e-5 as the float32
# the kernel writes, so that both a device comparison and float(score) == NO_SCORE hold
NO_SCORE = float(torch.tensor(1e-5, dtype=torch.float32))
MAX_SAMPLES = 1 << 22


def stoi_frames(length: int) -> int:
    """Frames of a row of `length` samples at 10 kHz: ceil((length - 256) / 128), 0 below 257."""
    return int(lib.encx_stoi_frames(int(length)))


def stoi_10k(ref: torch.Tensor, deg: torch.Tensor, lengths: tp.Optional[torch.Tensor] = None,
             return_kept: bool = False):
    """encx_stoi on [B][T] rows already at 10 kHz -> float32 [B] (and, with return_kept, the
    int32 [B] count of frames each row kept after the silent-frame removal)."""
    ops._check(ref, 'ref')
    ops._check(deg, 'deg')
    if ref.dim() != 2 or ref.shape != deg.shape:
        raise ValueError(f'encx: stoi_10k takes two [B][T] tensors of one shape (got {tuple(ref.shape)}, '
                         f'{tuple(deg.shape)})')
    B, T = int(ref.shape[0]), int(ref.shape[1])
    if T > MAX_SAMPLES:
        raise ValueError(f'encx: stoi rows are limited to {MAX_SAMPLES} samples at 10 kHz (got {T})')
    ref, deg = ref.contiguous(), deg.contiguous()
    if lengths is not None:
        if not lengths.is_cuda or lengths.dtype != torch.int64 or lengths.shape != (B,):
            raise RuntimeError('encx: stoi lengths must be an int64 [B] tensor on the GPU (no CPU fallback)')
        lengths = lengths.contiguous()
    out = torch.empty(B, device=ref.device, dtype=torch.float32)
    if B == 0:
        return (out, torch.empty(0, device=ref.device, dtype=torch.int32)) if return_kept else out
    words = int(lib.encx_stoi_workspace_floats(B, T))
    assert words >= B
    ws = torch.empty(words, device=ref.device, dtype=torch.float32)
    call('encx_stoi', ptr(ref), ptr(deg), ptr(lengths), ptr(ws), ptr(out), B, T, stream())
    if return_kept:
        return out, ws[:B].view(torch.int32).clone()
    return out


def stoi(ref: torch.Tensor, deg: torch.Tensor, sr: int, extended: bool = False,
         lengths: tp.Optional[torch.Tensor] = None) -> torch.Tensor:
    """pystoi.stoi(ref, deg, sr, extended=False) for float32 GPU tensors [T] or [B][T] ->
    float32 [B] on the device (0-d for 1-D input). `lengths` (int64 [B] on the device): the
    samples of each row at `sr`; the rest of the row is ignored. A rate other than 10 kHz goes
    through ops.resample first, and the lengths through the same ceil(n L / o). A row too short
    for 30 analysis frames scores 1e-5, as in the published implementation."""
    if extended:
        raise NotImplementedError('encx: extended STOI is not implemented (the reference passes extended=False)')
    ops._check(ref, 'ref')
    ops._check(deg, 'deg')
    if ref.shape != deg.shape or ref.dim() not in (1, 2):
        raise ValueError(f'encx: stoi takes two [T] or [B][T] tensors of one shape (got {tuple(ref.shape)}, '
                         f'{tuple(deg.shape)})')
    sr = ops._rate(sr, 'sr')
    one = ref.dim() == 1
    if one:
        ref, deg = ref[None], deg[None]
        if lengths is not None:
            lengths = lengths.reshape(1)
    if sr != FS:
        # [B][T] -> [B][1][T]: every row a mono clip of its own. A row shorter than T is cut
        # before the filter sees what follows it: zero the tail, as a clip's end is.
        if lengths is not None:
            T = ref.shape[-1]
            live = torch.arange(T, device=ref.device)[None] < lengths[:, None]
            ref, deg = ref * live, deg * live
            g = math.gcd(sr, FS)
            o, n = sr // g, FS // g
            lengths = (lengths.clamp(0, T) * n + (o - 1)) // o   # encx_resample_out_len per row
        ref = ops.resample(ref[:, None], sr, FS)[:, 0]
        deg = ops.resample(deg[:, None], sr, FS)[:, 0]
    d = stoi_10k(ref, deg, lengths)
    return d[0] if one else d
