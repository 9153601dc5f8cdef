"""Training batches from clips resident in HBM (customAudioDataset.py of the reference).

The reference decodes every file per item on the host (librosa.load), crops a random
`tensor_cut` window, expands mono to `channels` and zero-pads the batch (collate_fn).
`CustomAudioDataset` keeps the same configuration fields, `__len__`, and random-crop rule,
but decodes each file once into an `AudioPool` in HBM (288 GB holds ~1000 h of 24 kHz
fp32 audio). `make_batch` then draws the crop starts on the host with Python's `random`, in the
reference's call order (so the same seed gives the same windows), and builds the
[B][C][Tmax] batch with one `encx_crop_collate` launch. There is no CPU batch path.

File decoding: PCM WAV through the standard library `wave` module (the image has no librosa
or soundfile), `read_wav`. A file at the model's sample rate is downmixed to mono on the host by
channel mean, as librosa.load(mono=True) does. A file at any other rate is resampled on the GPU
while the pool is built, with the mono downmix fused (encx.utils.convert_audio, csrc/resample.hip).
One deviation: the reference dataset resamples with librosa.load(sr=...), i.e. soxr, which cannot
be reproduced here; this loader uses the filter of the reference's other loaders instead
(utils.convert_audio: torchaudio.transforms.Resample's default windowed sinc).
"""
import random
import typing as tp
import wave

import numpy as np
import torch

from ._lib import call, stream, ensure_device


def read_wav(path: str) -> tp.Tuple[np.ndarray, int]:
    """-> (float32 [C][T] in [-1, 1), sample rate) of a PCM WAV file (8, 16 or 32 bits)."""
    with wave.open(path, 'rb') as w:
        sr, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, '<i2').astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, '<i4').astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f'{path}: unsupported sample width {width}')
    return np.ascontiguousarray(x.reshape(-1, ch).T, np.float32), sr


def load_wav(path: str, sample_rate: int, mono: bool) -> np.ndarray:
    """-> float32 [C][T] in [-1, 1) of a file at `sample_rate`. customAudioDataset.py:38-42
    (librosa.load(sr, mono)) without the rate conversion: a file at another rate is refused here
    (CustomAudioDataset resamples such files on the GPU)."""
    x, sr = read_wav(path)
    if sr != sample_rate:
        raise ValueError(f'{path}: sample rate {sr} != {sample_rate} (load_wav does not resample)')
    if mono:
        x = x.mean(0, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def load_clip(path: str, sample_rate: int, mono: bool, device) -> tp.Union[np.ndarray, torch.Tensor]:
    """One file of the dataset: load_wav's host array at the model's rate, else the file
    resampled to `sample_rate` on `device` (mono: the mean over the channels, before the
    filter) as a device tensor [C][T']."""
    x, sr = read_wav(path)
    if sr == sample_rate:
        return np.ascontiguousarray(x.mean(0, keepdims=True) if mono else x, np.float32)
    from .utils import convert_audio
    return convert_audio(torch.from_numpy(x).to(device), sr, sample_rate, 1 if mono else x.shape[0])


class AudioPool:
    """Decoded clips packed back to back in one device buffer; clip i is
    [channels[i]][lengths[i]] at offsets[i]. Clips may be host arrays or device tensors (files
    resampled on the GPU). With any device tensor among them the pool is one torch.cat of the
    per-clip tensors, so building it needs twice the pool's memory for a moment, and every such
    file was its own upload and resample launch; a pool of host arrays alone goes up in one copy."""

    def __init__(self, clips: tp.Sequence[tp.Union[np.ndarray, torch.Tensor]], device='cuda'):
        self.device = torch.device(device)
        arrs = [a[None] if a.ndim == 1 else a
                for a in (c if torch.is_tensor(c) else np.asarray(c, np.float32) for c in clips)]
        self.channels = np.array([a.shape[0] for a in arrs], np.int64)
        self.lengths = np.array([a.shape[1] for a in arrs], np.int64)
        sizes = self.channels * self.lengths
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        if any(torch.is_tensor(a) for a in arrs):
            # clips already on the device (resampled there) stay there; host runs go up in one copy each
            parts, run = [], []
            for a in arrs:
                if torch.is_tensor(a):
                    if run:
                        parts.append(torch.from_numpy(np.concatenate(run)).to(self.device))
                        run = []
                    parts.append(a.detach().to(self.device, torch.float32).reshape(-1))
                else:
                    run.append(a.reshape(-1))
            if run:
                parts.append(torch.from_numpy(np.concatenate(run)).to(self.device))
            self.data = torch.cat(parts)
            return
        flat = np.concatenate([a.reshape(-1) for a in arrs]) if arrs else np.zeros(0, np.float32)
        self.data = torch.from_numpy(flat).to(self.device)

    def __len__(self):
        return len(self.lengths)

    def gather(self, idx: tp.Sequence[int], starts: tp.Sequence[int], out_len: tp.Sequence[int],
               channels: int) -> torch.Tensor:
        """One encx_crop_collate launch -> [B][channels][max(out_len)] on the device."""
        ensure_device(self.device)
        idx = np.asarray(idx, np.int64)
        starts = np.asarray(starts, np.int64)
        out_len = np.asarray(out_len, np.int64)
        src = self.channels[idx]
        if not np.all((src == 1) | (src == channels)):
            raise ValueError('clip channel count must be 1 or the model channel count')
        if np.any(starts < 0) or np.any(starts + out_len > self.lengths[idx]):
            raise ValueError('crop window outside the clip')
        B, Tmax = len(idx), int(out_len.max()) if len(idx) else 0
        # pinned + non_blocking: a pageable H2D copy would block the host until the stream has
        # drained (the previous train step), leaving the GPU idle while the next step is enqueued
        meta = torch.from_numpy(np.stack([self.offsets[idx], self.lengths[idx], src, starts, out_len])
                                ).pin_memory().to(self.device, non_blocking=True)
        out = torch.empty(B, channels, Tmax, device=self.device, dtype=torch.float32)
        call('encx_crop_collate', self.data.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
             meta[2].data_ptr(), meta[3].data_ptr(), meta[4].data_ptr(), out.data_ptr(), B, channels,
             Tmax, stream())
        return out


class CustomAudioDataset:
    """customAudioDataset.py:15-69 over an AudioPool. `config` carries the reference's fields
    (datasets.train_csv_path / test_csv_path, fixed_length, tensor_cut, model.sample_rate,
    model.channels); `clips` may be given directly instead of reading the csv's files. A listed
    file whose rate differs from model.sample_rate is resampled on the device (load_clip)."""

    def __init__(self, config, transform=None, mode='train', clips=None, device='cuda'):
        assert mode in ['train', 'test'], 'dataset mode must be train or test'
        self.transform = transform
        self.fixed_length = config.datasets.fixed_length
        self.tensor_cut = config.datasets.tensor_cut
        self.sample_rate = config.model.sample_rate
        self.channels = config.model.channels
        if clips is None:
            import pandas as pd
            csv = config.datasets.train_csv_path if mode == 'train' else config.datasets.test_csv_path
            files = pd.read_csv(csv, on_bad_lines='skip').iloc[:, 0].tolist()
            clips = [load_clip(f, self.sample_rate, self.channels == 1, device) for f in files]
        self.pool = AudioPool(clips, device=device)

    def __len__(self):
        n = len(self.pool)
        return self.fixed_length if self.fixed_length and n > self.fixed_length else n

    def get(self, idx: tp.Optional[int] = None) -> torch.Tensor:
        """customAudioDataset.py:31-55: clip `idx` uncropped and untransformed, [channels][T] (a
        mono clip expanded); a random.randrange(len(self)) pick when idx is None."""
        if idx is None:
            idx = random.randrange(len(self))
        if not 0 <= idx < len(self.pool):
            raise IndexError(f'clip {idx} of {len(self.pool)}')
        L = int(self.pool.lengths[idx])
        return self.pool.gather([idx], [0], [L], self.channels)[0]

    def _window(self, i):
        L = int(self.pool.lengths[i])
        if self.tensor_cut > 0 and L > self.tensor_cut:
            start = random.randint(0, L - self.tensor_cut - 1)  # customAudioDataset.py:66
            return start, self.tensor_cut
        return 0, L

    def make_batch(self, indices: tp.Sequence[int], return_lengths: bool = False):
        """[dataset[i] for i in indices] + collate_fn (customAudioDataset.py:58-91) as one
        launch; crop starts drawn in item order like the reference's DataLoader does. With
        return_lengths also the items' lengths before the zero pad (a list)."""
        wins = [self._window(int(i)) for i in indices]
        out = self.pool.gather(indices, [w[0] for w in wins], [w[1] for w in wins], self.channels)
        if self.transform is not None:
            out = self.transform(out)
        return (out, [w[1] for w in wins]) if return_lengths else out

    def batches(self, batch_size: int, shuffle: bool = True, drop_last: bool = True):
        """DataLoader(shuffle) order over __len__ (train_multi_gpu.py:277-282)."""
        order = list(range(len(self)))
        if shuffle:
            random.shuffle(order)
        stop = len(order) - (len(order) % batch_size if drop_last else 0)
        for s in range(0, stop, batch_size):
            yield self.make_batch(order[s:s + batch_size])
