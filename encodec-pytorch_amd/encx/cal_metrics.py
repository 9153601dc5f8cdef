"""cal_metrics.py of the reference on the encx path: STOI of every degraded file under a folder
against its reference file, with the reference's arguments, pairing rule and output file.

Differences from the reference, by design:
  * STOI runs on the GPU (encx.metrics.stoi, csrc/stoi.hip) instead of pystoi on the host;
  * files are PCM WAV read with the standard library (encx.data.read_wav) and brought to mono at
    `--sr` on the GPU (encx.utils.convert_audio) instead of librosa.load(sr=...);
  * PESQ is the ITU's program and is not part of this package: no pesq_scores.txt is written,
    `PESQ: not available` is printed, and main() returns NaN for both PESQ means.

python encodec-pytorch_amd/encx/cal_metrics.py -r REF_DIR -d DEG_DIR [-s 16000] [-b 6] [-e wav] [-o ./results/]
"""
import argparse
import os
import sys
from pathlib import Path

import torch

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = 'encx'

from . import metrics  # noqa: E402
from .data import read_wav  # noqa: E402
from .utils import convert_audio  # noqa: E402


def get_parser():
    """The reference's options (cal_metrics.py:13-54): same names, types and defaults."""
    parser = argparse.ArgumentParser(description='Compute the STOI measure')
    parser.add_argument('-r', '--ref_dir', required=True, help='Reference wave folder.')
    parser.add_argument('-d', '--deg_dir', required=True, help='Degraded wave folder.')
    parser.add_argument('-s', '--sr', type=int, default=16000, help='encodec sample rate.')
    parser.add_argument('-b', '--bandwidth', type=float, default=6, help='encodec bandwidth.')
    parser.add_argument('-e', '--ext', default='wav', type=str, help='file extension')
    parser.add_argument('-o', '--output_result_path', default='./results/', type=Path)
    return parser


def load_mono(path, sr, device='cuda'):
    """librosa.load(path, sr=sr) of the reference (:120-121) -> float32 [T] on the device."""
    x, file_sr = read_wav(str(path))
    return convert_audio(torch.from_numpy(x).to(device), file_sr, sr, 1)[0]


def calculate_stoi(ref_wav, deg_wav, sr):
    """cal_metrics.py:57-63: both cut to the shorter, then STOI; a python float."""
    min_len = min(len(ref_wav), len(deg_wav))
    return float(metrics.stoi(ref_wav[:min_len].contiguous(), deg_wav[:min_len].contiguous(), sr, extended=False))


def main(argv=None):
    """-> (mean STOI, nan, nan): the reference's (STOI, NB PESQ, WB PESQ) with PESQ absent."""
    args = get_parser().parse_args(argv)
    stoi_scores = []
    args.output_result_path.mkdir(parents=True, exist_ok=True)
    with open(args.output_result_path / 'stoi_scores.txt', 'w') as s:
        for deg_wav_path in sorted(Path(args.deg_dir).rglob(f'*.{args.ext}')):
            relative_path = deg_wav_path.relative_to(args.deg_dir)
            ref_wav_path = Path(args.ref_dir) / relative_path.parents[0] / \
                deg_wav_path.name.replace(f'_bw{args.bandwidth}', '')
            ref_wav = load_mono(ref_wav_path, args.sr)
            deg_wav = load_mono(deg_wav_path, args.sr)
            stoi_score = calculate_stoi(ref_wav, deg_wav, sr=args.sr)
            if stoi_score != metrics.NO_SCORE:
                stoi_scores.append(stoi_score)
                s.write(f'{ref_wav_path}\t{deg_wav_path}\t{stoi_score}\n')
    mean_stoi = sum(stoi_scores) / len(stoi_scores) if stoi_scores else float('nan')
    print(f'STOI: {mean_stoi}')
    print('PESQ: not available')
    return mean_stoi, float('nan'), float('nan')


if __name__ == '__main__':
    main()
