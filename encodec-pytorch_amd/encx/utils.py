"""utils.py of the reference: `convert_audio` and `save_audio`.

convert_audio runs on the GPU (encx.ops.resample: the channel conversion and
torchaudio.transforms.Resample's default filter in one HIP launch); save_audio is host work
through the standard library `wave` module (the image has no torchaudio or soundfile).
"""
import typing as tp
import wave
from pathlib import Path

import torch

from . import ops


def convert_audio(wav: torch.Tensor, sr: int, target_sr: int, target_channels: int):
    """utils.py:84-97 -> [..., target_channels, ceil(n L / o)] on wav's device (a GPU: there is
    no CPU path). Mono or stereo in; 1 channel out is the mean, 2 from 1 both the same, and any
    other target needs mono input, as in the reference."""
    assert wav.dim() >= 2, "Audio tensor must have at least 2 dimensions"
    assert wav.shape[-2] in [1, 2], "Audio must be mono or stereo."
    channels = wav.shape[-2]
    if target_channels not in (1, 2) and channels != 1:
        raise RuntimeError(f"Impossible to convert from {channels} to {target_channels}")
    if target_channels > 2:  # utils.py:92-93: mono.expand(target_channels, -1), a 2-D input only
        return ops.resample(wav, sr, target_sr).expand(target_channels, -1)
    return ops.resample(wav, sr, target_sr, channels=target_channels)


def _pcm16(wav: torch.Tensor) -> torch.Tensor:
    """float -> int16: round-half-even of x * 32768, clipped to [-32768, 32767]."""
    return torch.round(wav.detach().to('cpu', torch.float64) * 32768.0).clamp_(-32768, 32767).to(torch.int16)


def save_audio(wav: torch.Tensor, path: tp.Union[Path, str], sample_rate: int, rescale: bool = False):
    """utils.py:100-116: wav [C][T] (or [T]) limited to 0.99, by clamping or with `rescale` by
    the factor min(0.99 / max|wav|, 1), then written as 16-bit PCM WAV. The reference writes
    through torchaudio.save(encoding='PCM_S', bits_per_sample=16), whose float -> int16 rule cannot
    be observed here; this one is round-half-even of x * 32768 clipped to int16, the inverse of
    encx.data.read_wav's x / 32768."""
    limit = 0.99
    mx = wav.abs().max()
    if rescale:
        wav = wav * min(limit / mx, 1)
    else:
        wav = wav.clamp(-limit, limit)
    if wav.dim() == 1:
        wav = wav[None]
    pcm = _pcm16(wav).T.contiguous().numpy()  # frames interleaved [T][C]
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(wav.shape[0])
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(pcm.astype('<i2').tobytes())
