"""Train the entropy-coding language model (encx.lm.LMModel) for a codec of your own.

The reference ships two pretrained LMs for Meta's codebooks and no way to train one; a codec
trained with train_multi_gpu.py needs its own. This command encodes the WAVs of a CSV with the
codec (no gradients), minimises the teacher-forced next-code cross-entropy `LMModel.nll` -- the
very log-probabilities the arithmetic coder of `compress(..., use_lm=True)` will code with --
with FlatAdam on one GPU, and saves {'lm_state_dict', 'lm_config'}. With --merge-into the LM is
also written into a copy of the codec checkpoint, which `main.py -l -c FILE` then codes with.

python encodec-pytorch_amd/encx/train_lm.py -c CKPT --csv files.csv -b 6 --out lm.pt \\
    [--merge-into codec_lm.pt] [--batch-size 32 --crop 48000 --epochs 10 --lr 3e-4]
"""
import argparse
import math
import os
import sys
import types

import torch

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = 'encx'

from .compress import MODELS  # noqa: E402
from .data import CustomAudioDataset  # noqa: E402
from .lm import LMModel  # noqa: E402
from .optim import FlatAdam  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser('train_lm', description='Train the entropy-coding LM of a codec on one GPU.')
    p.add_argument('-c', '--checkpoint', type=str, required=True, help='the codec checkpoint, as main.py -c')
    p.add_argument('-m', '--model_name', type=str, default='my_encodec', help='as main.py -m')
    p.add_argument('--csv', type=str, required=True, help='CSV whose first column lists PCM WAV files')
    p.add_argument('-b', '--bandwidth', type=float, default=6, choices=[1.5, 3., 6., 12., 24.])
    p.add_argument('--batch-size', type=int, default=32)
    p.add_argument('--crop', type=int, default=48000, help='samples per training clip (longer files are cropped)')
    p.add_argument('--epochs', type=int, default=10)
    p.add_argument('--lr', type=float, default=3e-4)
    p.add_argument('--dim', type=int, default=200)
    p.add_argument('--layers', type=int, default=5)
    p.add_argument('--heads', type=int, default=8)
    p.add_argument('--log-every', type=int, default=10)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', type=str, required=True, help="file for {'lm_state_dict', 'lm_config'}")
    p.add_argument('--merge-into', type=str, default=None,
                   help='also write the codec checkpoint with the LM added, for main.py -l -c')
    p.add_argument('-d', '--device', type=str, default='cuda')
    return p


def load_codec(args):
    from .main import load_weights
    if args.model_name == 'my_encodec':
        model = MODELS[args.model_name](args.checkpoint)
    elif args.model_name == 'encodec_bw':
        model = MODELS[args.model_name](args.checkpoint, [args.bandwidth])
    else:
        model = load_weights(args.model_name, args.checkpoint)
    model = model.to(args.device).eval()
    model.set_target_bandwidth(args.bandwidth)
    return model


def kbps(nats_per_code, K, frame_rate):
    """Bit rate the arithmetic coder approaches at this loss: K codes per frame."""
    return nats_per_code / math.log(2) * K * frame_rate / 1000


def train(args):
    import random
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = load_codec(args)
    cfg = types.SimpleNamespace(
        datasets=types.SimpleNamespace(train_csv_path=args.csv, test_csv_path=args.csv, fixed_length=0,
                                       tensor_cut=args.crop),
        model=types.SimpleNamespace(sample_rate=model.sample_rate, channels=model.channels))
    data = CustomAudioDataset(cfg, mode='train', device=args.device)
    lm_config = dict(n_q=model.quantizer.n_q, card=model.quantizer.bins, dim=args.dim, num_layers=args.layers,
                     num_heads=args.heads, past_context=int(3.5 * model.frame_rate))
    lm = LMModel(**lm_config).to(args.device)
    opt = FlatAdam(lm.parameters(), lr=args.lr)
    step, last = 0, float('nan')
    for epoch in range(args.epochs):
        for x in data.batches(min(args.batch_size, len(data)), shuffle=True, drop_last=True):
            with torch.no_grad():
                frames = model.encode(x)
            total = sum(c.numel() for c, _ in frames)
            opt.zero_grad()
            losses = []
            for codes, _ in frames:
                codes = codes.contiguous()
                loss = lm.nll(codes) * (codes.numel() / total)
                loss.backward()
                losses.append(loss.detach())
            opt.step()
            step += 1
            if step % args.log_every == 0 or step == 1:
                last = float(torch.stack(losses).sum())
                K = frames[0][0].shape[1]
                print(f'epoch {epoch} step {step}: {last:.4f} nats/code -> {kbps(last, K, model.frame_rate):.3f} kbit/s '
                      f'(un-modelled {K * math.log2(lm.card) * model.frame_rate / 1000:.3f} kbit/s)', flush=True)
    out = {'lm_state_dict': {k: v.detach().cpu().clone() for k, v in lm.state_dict().items()}, 'lm_config': lm_config}
    torch.save(out, args.out)
    if args.merge_into:
        ckpt = torch.load(args.checkpoint, map_location='cpu', weights_only=True)
        if not (isinstance(ckpt, dict) and 'model_state_dict' in ckpt):
            ckpt = {'model_state_dict': ckpt}
        ckpt.update(out)
        torch.save(ckpt, args.merge_into)
    return lm, last


if __name__ == '__main__':
    train(get_parser().parse_args())
