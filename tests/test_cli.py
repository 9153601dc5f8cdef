"""encx/main.py, the reference's command line: parser defaults (CPU) and the file -> `.ecdc` ->
file paths in process against compress / decompress / convert_audio / save_audio (GPU)."""
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from fixtures import load, model_state, codebooks_from_stats

DEV = 'cuda:0'


def test_parser_defaults_match_the_reference():
    from encx.main import SUFFIX, get_parser
    assert SUFFIX == '.ecdc'
    a = get_parser().parse_args(['in.wav'])
    assert vars(a) == dict(input=Path('in.wav'), output=None, bandwidth=6, hq=False, lm=False, force=False,
                           decompress_suffix='_decompressed', rescale=False, model_name='encodec_24khz',
                           checkpoint=None, device='cuda')
    a = get_parser().parse_args(['-b', '1.5', '-q', '-l', '-f', '-s', '_x', '-r', '-m', 'my_encodec', '-c', 'ck.pt',
                                 '-d', 'cuda:1', 'a.ecdc', 'b.wav'])
    assert vars(a) == dict(input=Path('a.ecdc'), output=Path('b.wav'), bandwidth=1.5, hq=True, lm=True, force=True,
                           decompress_suffix='_x', rescale=True, model_name='my_encodec', checkpoint='ck.pt',
                           device='cuda:1')
    a = get_parser().parse_args(['--bandwidth', '24', '--hq', '--lm', '--force', '--decompress_suffix', 's',
                                 '--rescale', '--model_name', 'm', '--checkpoint', 'c', '--device', 'd', 'x'])
    assert a.bandwidth == 24.0 and a.hq and a.lm and a.force and a.rescale and a.device == 'd'
    with pytest.raises(SystemExit):
        get_parser().parse_args(['-b', '2', 'in.wav'])


def test_pretrained_models_need_a_local_checkpoint(tmp_path, capsys):
    """No GPU is reached: the missing -c ends in fatal() before the model is built."""
    from encx.main import cli_main, get_parser
    (tmp_path / 'a.wav').write_bytes(b'')
    for extra in ([], ['-q']):
        with pytest.raises(SystemExit) as e:
            cli_main(get_parser().parse_args(extra + ['-d', 'cpu', str(tmp_path / 'a.wav')]))
        assert e.value.code == 1
        assert 'remote-only' in capsys.readouterr().err


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A my_encodec checkpoint (24 kHz mono, non-causal, time_group_norm, normalised) with the
    synthetic weights and codebooks the .ecdc tests use (two filled codebooks, the rest zero)."""
    from oracle import encodec_oracle as O
    cfg = O.Config(sample_rate=24000, channels=1, causal=False, norm='time_group_norm', audio_normalize=True,
                   target_bandwidths=(1.5, 3., 6., 12., 24.))
    sd = dict(model_state(cfg, 131))
    stats = load('g1_eval24k.npz')['stats']
    for i, cb in enumerate(codebooks_from_stats(stats, 133, 2, cfg.n_q)):
        for k, v in cb.items():
            sd[f'quantizer.vq.layers.{i}._codebook.{k}'] = v
    path = tmp_path_factory.mktemp('ckpt') / 'my_encodec.pt'
    torch.save({'epoch': 0, 'model_state_dict': sd}, path)
    return str(path)


@pytest.fixture(scope='module')
def model(checkpoint):
    from encx.model import EncodecModel
    m = EncodecModel.my_encodec_model(checkpoint).to(DEV)
    m.set_target_bandwidth(6.0)
    return m


def write_input(path, seed=5):
    """0.5 s of 16 kHz stereo PCM16."""
    g = np.random.default_rng(seed)
    t = np.arange(8000) / 16000.0
    x = np.stack([0.4 * np.sin(2 * np.pi * 440 * t), 0.3 * np.sin(2 * np.pi * 1300 * t + 1.0)])
    x = x + 0.02 * g.standard_normal(x.shape)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray((x * 32768).round().astype('<i2').T).tobytes())


def run(*argv):
    from encx.main import cli_main, get_parser
    cli_main(get_parser().parse_args([str(a) for a in argv]))


def converted(path, model):
    from encx.data import read_wav
    from encx.utils import convert_audio
    x, sr = read_wav(str(path))
    assert sr == 16000 and x.shape == (2, 8000)
    wav = convert_audio(torch.from_numpy(x).to(DEV), sr, model.sample_rate, model.channels)
    assert wav.shape == (1, 12000)
    return wav


@pytest.mark.gpu
def test_gpu_cli_wav_to_ecdc_to_wav(tmp_path, checkpoint, model):
    from encx.compress import compress, decompress
    from encx.utils import save_audio
    src = tmp_path / 'in.wav'
    write_input(src)
    common = ['-m', 'my_encodec', '-c', checkpoint, '-d', DEV]
    # wav -> .ecdc, output inferred
    run(*common, src)
    data = (tmp_path / 'in.ecdc').read_bytes()
    assert data == compress(model, converted(src, model))
    # an existing output without -f: exit status 1, file untouched; with -f it is rewritten
    with pytest.raises(SystemExit) as e:
        run(*common, src)
    assert e.value.code == 1
    (tmp_path / 'in.ecdc').write_bytes(b'x')
    run(*common, '-f', src)
    assert (tmp_path / 'in.ecdc').read_bytes() == data
    # .ecdc -> wav, output inferred with the suffix
    run(*common, tmp_path / 'in.ecdc')
    out, sr = decompress(model, data)
    assert sr == 24000 and out.shape == (1, 12000)
    save_audio(out, tmp_path / 'want.wav', sr)
    assert (tmp_path / 'in_decompressed.wav').read_bytes() == (tmp_path / 'want.wav').read_bytes()
    # wav -> wav, rescaled
    run(*common, '-r', src, tmp_path / 'cycle.wav')
    save_audio(out, tmp_path / 'want_r.wav', sr, rescale=True)
    assert (tmp_path / 'cycle.wav').read_bytes() == (tmp_path / 'want_r.wav').read_bytes()
    # a wrong output extension
    with pytest.raises(SystemExit):
        run(*common, src, tmp_path / 'out.mp3')


@pytest.mark.gpu
def test_gpu_cli_folder_mode(tmp_path, checkpoint, model):
    from encx.compress import compress, decompress
    from encx.utils import save_audio
    (tmp_path / 'in' / 'sub').mkdir(parents=True)
    write_input(tmp_path / 'in' / 'a.wav', 1)
    write_input(tmp_path / 'in' / 'sub' / 'b.wav', 2)
    run('-m', 'my_encodec', '-c', checkpoint, '-d', DEV, tmp_path / 'in', tmp_path / 'out')
    for rel in ('a', 'sub/b'):
        got = tmp_path / 'out' / (rel + '_bw6.wav')
        assert got.exists()
        out, sr = decompress(model, compress(model, converted(tmp_path / 'in' / (rel + '.wav'), model)))
        save_audio(out, tmp_path / 'want.wav', sr)
        assert got.read_bytes() == (tmp_path / 'want.wav').read_bytes()
