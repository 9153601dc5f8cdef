"""Command line of the codec on the encx path; the counterpart of the reference's main.py, with
its flags, defaults, `SUFFIX` and output naming.

  input.ecdc [out.wav]   decode; default output <stem><decompress_suffix>.wav
  input.wav  [out.ecdc]  encode; default output input.ecdc
  input.wav  out.wav     encode and decode again
  folder     out_folder  the wav -> wav cycle for every **/*.wav, written to the same relative
                         path under out_folder as <name>_bw<N>.wav

Differences from the reference, by design:
  * input is PCM WAV read with the standard library (encx.data.read_wav; the image has no
    torchaudio) and brought to the model's rate and channels on the GPU (encx.utils.convert_audio);
  * the reference's decode branch cannot run (main.py:97 passes no model and calls
    `args.device()`); here it does what it means to: decompress(model, bytes, device=args.device);
  * a checkpoint that carries an LM trained by encx/train_lm.py ('lm_state_dict', written by
    its --merge-into) codes with that LM under -l;
  * pretrained weights are remote-only, so `encodec_24khz` / `encodec_48khz` take theirs from
    `-c FILE` (a state dict, or a checkpoint holding `model_state_dict`), loaded with
    weights_only=True, and stop with a message without it.

python encodec-pytorch_amd/encx/main.py [-b 6] [-m my_encodec -c CKPT] input [output]
"""
import argparse
import os
import sys
from pathlib import Path

import torch

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = 'encx'

from .compress import MODELS, compress, decompress  # noqa: E402
from .data import read_wav  # noqa: E402
from .utils import convert_audio, save_audio  # noqa: E402

SUFFIX = '.ecdc'
LIMIT = 0.99  # save_audio's ceiling


def get_parser():
    """The reference's options (main.py:21-62): same names, types, defaults and choices."""
    p = argparse.ArgumentParser('encodec', description='Neural audio codec: .ecdc in is decoded to wav, wav in is '
                                'encoded to .ecdc, or to wav for a round trip through the codec.')
    p.add_argument('input', type=Path, help='a PCM WAV file, an .ecdc file, or a folder of WAV files')
    p.add_argument('output', type=Path, nargs='?', help='output file (folder in folder mode); derived from the input if absent')
    p.add_argument('-b', '--bandwidth', type=float, default=6, choices=[1.5, 3., 6., 12., 24.],
                   help='target bandwidth in kbps; the 48 kHz model has no 1.5')
    p.add_argument('-q', '--hq', action='store_true', help='the 48 kHz stereo model')
    p.add_argument('-l', '--lm', action='store_true', help='entropy-code the codes under the language model')
    p.add_argument('-f', '--force', action='store_true', help='overwrite an existing output')
    p.add_argument('-s', '--decompress_suffix', type=str, default='_decompressed',
                   help='appended to the stem of a decoded file when no output is given')
    p.add_argument('-r', '--rescale', action='store_true', help='scale the output down instead of clipping it')
    p.add_argument('-m', '--model_name', type=str, default='encodec_24khz',
                   help='encodec_24khz, encodec_48khz or my_encodec')
    p.add_argument('-c', '--checkpoint', type=str,
                   help='weights: the checkpoint of my_encodec, or a state dict / checkpoint for the other models')
    p.add_argument('-d', '--device', type=str, default='cuda')
    return p


def fatal(*args):
    print(*args, file=sys.stderr)
    sys.exit(1)


def check_output_exists(args):
    """main.py:70-74: the output's folder must exist, the output itself only with --force."""
    if not args.output.parent.exists():
        fatal(f"Output folder for {args.output} does not exist.")
    if args.output.exists() and not args.force:
        fatal(f"Output file {args.output} exist. Use -f / --force to overwrite.")


def check_clipping(wav, args):
    """main.py:77-86: warn when save_audio is going to clip."""
    if args.rescale:
        return
    mx = float(wav.abs().max())
    if mx > LIMIT:
        print(f"Clipping!! max scale {mx}, limit is {LIMIT}. Use -r / --rescale to scale the output instead.",
              file=sys.stderr)


def _write_wav(model, data, args):
    out, sr = decompress(model, data, device=args.device)
    check_clipping(out, args)
    save_audio(out, args.output, sr, rescale=args.rescale)


def main(args, model):
    """One file (main.py:89-119)."""
    decode = args.input.suffix.lower() == SUFFIX
    if args.output is None:
        if decode:
            args.output = args.input.with_name(args.input.stem + args.decompress_suffix).with_suffix('.wav')
        else:
            args.output = args.input.with_suffix(SUFFIX)
    kind = args.output.suffix.lower()
    if decode and kind != '.wav':
        fatal("Output extension must be .wav")
    if not decode and kind not in (SUFFIX, '.wav'):
        fatal(f"Output extension must be .wav or {SUFFIX}")
    check_output_exists(args)
    if decode:
        _write_wav(model, args.input.read_bytes(), args)
        return
    wav, sr = read_wav(str(args.input))
    wav = convert_audio(torch.from_numpy(wav).to(args.device), sr, model.sample_rate, model.channels)
    data = compress(model, wav, use_lm=args.lm)
    if kind == SUFFIX:
        args.output.write_bytes(data)
    else:
        _write_wav(model, data, args)


def load_weights(model_name, checkpoint):
    """encodec_24khz / encodec_48khz: the architecture, then the local file's state dict (or its
    'model_state_dict')."""
    if not checkpoint:
        fatal(f"The pretrained weights of {model_name} are remote-only and are not downloaded; "
              "give a local state dict or checkpoint with -c / --checkpoint.")
    if not os.path.exists(checkpoint):
        fatal(f"Checkpoint {checkpoint} does not exist.")
    model = MODELS[model_name](pretrained=False)
    ckpt = sd = torch.load(checkpoint, map_location='cpu', weights_only=True)
    if isinstance(sd, dict) and 'model_state_dict' in sd:
        sd = sd['model_state_dict']
    model.load_state_dict(sd)
    model.name = model_name
    model.install_lm(ckpt)  # an LM trained by encx/train_lm.py and merged into the file
    return model.eval()


def cli_main(args):
    """main.py:121-155: the model, its bandwidth, then the file or every wav under the folder."""
    model_name = 'encodec_48khz' if args.hq else args.model_name
    if model_name not in MODELS:
        fatal(f"Unknown model {model_name}; choose one of {', '.join(MODELS)}.")
    if model_name == 'my_encodec':
        model = MODELS[model_name](args.checkpoint)
    elif model_name == 'encodec_bw':
        model = MODELS[model_name](args.checkpoint, [args.bandwidth])
    else:
        model = load_weights(model_name, args.checkpoint)
    model = model.to(args.device)
    print(f"-------------USE {model_name} MODEL-------------")
    if args.bandwidth not in model.target_bandwidths:
        fatal(f"Bandwidth {args.bandwidth} is not supported by the model {model_name}")
    model.set_target_bandwidth(args.bandwidth)

    if args.input.is_file():
        main(args, model)
    elif args.input.is_dir():
        src, dst = args.input, args.output
        if dst is None:
            fatal("Folder mode needs an output folder.")
        for wav in sorted(src.glob('**/*.wav')):
            print(f"Processing {wav}")
            target = dst / wav.relative_to(src)
            target.parent.mkdir(parents=True, exist_ok=True)
            args.input = wav
            args.output = target.with_name(f"{target.stem}_bw{int(args.bandwidth)}.wav")
            main(args, model)


if __name__ == '__main__':
    args = get_parser().parse_args()
    if not args.input.exists():
        fatal(f"Input file {args.input} does not exist.")
    cli_main(args)
