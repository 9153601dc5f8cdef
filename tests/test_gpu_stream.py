"""Streaming codec (encx/streaming.py, csrc/stream.hip) on the GPU: delivered in chunks, the
causal model must produce what the offline model produces on the whole clip.

The clip is 27 latent frames (8640 samples) of the 24 kHz causal model of test_gpu_long.py.
Bounds are the project's own offline bounds (test_gpu_long.py: latent 1e-4, wave 1e-3, codes
equal wherever fp64 certifies them); streaming gets no extra margin. The kernels' reduction order
depends on the layer only, so slicing, batching and graph replay are checked bit for bit.

Measured on an MI355X (B = 1, schedule 7, 1, 1, 3, 8, 2, 5): see DESIGN.md §7."""
import numpy as np
import pytest
import torch

from oracle import encodec_oracle as O
from fixtures import load, T, model_state, codebooks_from_stats, rvq_certified
from synth import synth_wave

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOP, FRAMES = 320, 27
SCHEDULE = (7, 1, 1, 3, 8, 2, 5)
BW = 1.5


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def build(channels, seed):
    from encx.model import EncodecModel
    d = load('g1_eval24k.npz')
    cfg = O.Config(channels=channels, target_bandwidths=(1.5, 3., 6., 12., 24.), audio_normalize=False)
    p = model_state(cfg, seed)
    cbs = codebooks_from_stats(d['stats'], 77, 2, cfg.n_q)
    m = EncodecModel._get_model([1.5, 3., 6., 12., 24.], 24000, channels, causal=True, model_norm='weight_norm',
                                audio_normalize=False, name='encodec_24khz')
    sd = dict(p)
    for i, cb in enumerate(cbs):
        for k, v in cb.items():
            sd[f'quantizer.vq.layers.{i}._codebook.{k}'] = v
    m.load_state_dict(sd)
    m.eval()
    m.set_target_bandwidth(BW)
    return m.to(DEV), cfg, p, cbs


@pytest.fixture(scope='module')
def mono():
    """The model, three clips, and everything computed once and left unchanged: the oracle's
    latent / codes / wave of clip 0 and the streamed result of all three clips one by one."""
    m, cfg, p, cbs = build(1, 1)
    x = T(synth_wave((3, 1, FRAMES * HOP), 4321))
    ns = type('Ctx', (), {})()
    ns.m, ns.cfg, ns.p, ns.cbs, ns.x = m, cfg, p, cbs, x
    ns.n_q = O.rvq_num_quantizers(BW, cfg.frame_rate, n_q_max=cfg.n_q)
    with torch.no_grad():
        (codes_o, _, emb_o), = O.encodec_encode_eval(x[:1], p, cbs, cfg, BW)
        ns.codes_o = torch.as_tensor(codes_o).long()  # [1, n_q, 27]
        ns.emb_o = emb_o
        ns.y_o = O.encodec_decode_eval([(codes_o, None)], p, cbs, cfg, x.shape[-1])
    ns.solo = [run(m, x[b:b + 1], SCHEDULE) for b in range(3)]  # (emb, codes, wave) per clip
    return ns


def stream_encode(m, x, schedule, graphs=True, max_frames=8, enc=None):
    from encx.streaming import StreamEncoder
    enc = enc or StreamEncoder(m, x.shape[0], max_frames=max_frames, graphs=graphs)
    assert sum(schedule) * enc.hop_length == x.shape[-1]
    embs, codes, off, hop = [], [], 0, enc.hop_length
    for n in schedule:
        c, e = enc.encode(x[:, :, off * hop:(off + n) * hop].to(DEV), return_latent=True)
        assert c.shape == (x.shape[0], enc.n_q, n) and c.dtype == torch.int64
        embs.append(e)
        codes.append(c)
        off += n
    return torch.cat(embs, 2), torch.cat(codes, 2), enc


def stream_decode(m, codes, schedule, graphs=True, max_frames=8, dec=None):
    from encx.streaming import StreamDecoder
    dec = dec or StreamDecoder(m, codes.shape[0], codes.shape[1], max_frames=max_frames, graphs=graphs)
    ys, off = [], 0
    for n in schedule:
        y = dec.decode(codes[:, :, off:off + n].to(DEV))
        assert y.shape == (codes.shape[0], m.channels, n * dec.hop_length)
        ys.append(y)
        off += n
    return torch.cat(ys, 2), dec


def run(m, x, schedule, graphs=True, max_frames=8):
    """Encode in chunks, then decode the streamed codes in the same chunks."""
    emb, codes, _ = stream_encode(m, x, schedule, graphs, max_frames)
    y, _ = stream_decode(m, codes, schedule, graphs, max_frames)
    return emb, codes, y


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def test_streamed_clip_against_the_oracle_and_the_offline_model(mono):
    m, x = mono.m, mono.x[:1]
    emb, codes, _ = mono.solo[0]
    r_emb = rel(emb, mono.emb_o)
    with torch.no_grad():
        emb_off = m.encoder(x.to(DEV))
    r_emb_off = rel(emb, emb_off)
    print(f'latent: rel vs oracle {r_emb:.3e}, vs the offline encoder {r_emb_off:.3e}')
    assert r_emb < 1e-4, r_emb
    assert r_emb_off < 1e-4, r_emb_off
    # codes: the assertions of test_gpu_long.check_segments on the streamed latent
    embeds = [cb['embed'] for cb in mono.cbs[:mono.n_q]]
    mine = codes.transpose(0, 1).cpu()  # [n_q, B, T]
    assert mine.shape == (mono.n_q, 1, FRAMES)
    for factor in (256, 32):
        want, cert = rvq_certified(emb, embeds, factor)
        print(f'certified at {factor}: {float(cert.float().mean()):.3f} of the codes')
        assert cert.any()
        assert torch.equal(mine[cert], want[cert]), (factor, int((mine[cert] != want[cert]).sum()))
    # the decoder on the ORACLE's codes, in the same schedule
    y, _ = stream_decode(m, mono.codes_o, SCHEDULE)
    with torch.no_grad():
        y_off = m.decode([(mono.codes_o.to(DEV), None)])
    r_y, r_y_off = rel(y, mono.y_o), rel(y, y_off)
    print(f'wave: rel vs oracle {r_y:.3e}, vs the offline decoder {r_y_off:.3e}')
    assert y.shape == mono.y_o.shape
    assert r_y < 1e-3, r_y
    assert r_y_off < 1e-3, r_y_off


def test_schedule_invariance_bit_for_bit(mono):
    """7 + 20 x 1 (windows shorter than the history: overlapping rolls; the reflect fill at the
    smallest first chunk), 8 + 8 + 8 + 3 (windows longer than every history) and all 27 frames
    at once: identical latents, codes and wave."""
    m, x = mono.m, mono.x[:1]
    a = run(m, x, (7,) + (1,) * 20)
    b = run(m, x, (8, 8, 8, 3))
    c = run(m, x, (27,), max_frames=27)
    for name, i in (('latent', 0), ('codes', 1), ('wave', 2)):
        assert torch.equal(a[i], b[i]), name
        assert torch.equal(a[i], c[i]), name
        assert torch.equal(a[i], mono.solo[0][i]), name


def test_batch_independence(mono):
    """Three different clips in one batch: each stream equals the same clip run alone."""
    both = run(mono.m, mono.x, SCHEDULE)
    assert not torch.equal(mono.solo[0][0], mono.solo[1][0])
    for b in range(3):
        for name, i in (('latent', 0), ('codes', 1), ('wave', 2)):
            assert torch.equal(both[i][b:b + 1], mono.solo[b][i]), (b, name)


def test_graph_equals_eager_and_reset_reproduces(mono):
    m, x = mono.m, mono.x[:1]
    eager = run(m, x, SCHEDULE, graphs=False)
    assert same(eager, mono.solo[0])  # mono.solo ran with graphs
    emb, codes, enc = stream_encode(m, x, SCHEDULE)
    y, dec = stream_decode(m, codes, SCHEDULE)
    assert same((emb, codes, y), eager)
    enc.reset()
    dec.reset()
    emb2, codes2, _ = stream_encode(m, x, SCHEDULE, enc=enc)  # replays the first session's graphs
    y2, _ = stream_decode(m, codes2, SCHEDULE, dec=dec)
    assert same((emb2, codes2, y2), eager)


def test_stereo_causal_model_against_the_offline_model():
    m, cfg, p, cbs = build(2, 3)
    schedule = (7, 2, 1)
    x = T(synth_wave((2, 2, sum(schedule) * HOP), 4323))
    emb, codes, y = run(m, x, schedule)
    with torch.no_grad():
        emb_off = m.encoder(x.to(DEV))
        y_off = m.decode([(codes, None)])
    r_emb, r_y = rel(emb, emb_off), rel(y, y_off)
    print(f'stereo: latent rel {r_emb:.3e}, wave rel {r_y:.3e} vs the offline model')
    assert y.shape == x.shape
    assert r_emb < 1e-4, r_emb
    assert r_y < 1e-3, r_y


def test_refresh_weights_follows_a_changed_model_and_no_grad_is_recorded():
    """Weights are prepared once: a session keeps its weights until refresh_weights(), after
    which it equals a session built from the changed model (graphs keep replaying: the
    prepared buffers are refilled in place). Under grad mode nothing is recorded."""
    from encx.streaming import StreamEncoder, StreamDecoder
    m, _, _, _ = build(1, 1)
    x = T(synth_wave((1, 1, 8 * HOP), 4324)).to(DEV)
    enc = StreamEncoder(m, 1)
    dec = StreamDecoder(m, 1, enc.n_q)
    with torch.enable_grad():
        codes, emb = enc.encode(x, return_latent=True)
        y = dec.decode(codes)
    assert not emb.requires_grad and not y.requires_grad and emb.grad_fn is None and y.grad_fn is None
    with torch.no_grad():
        for mod in (m.encoder.model[0], m.decoder.model[0]):
            mod.conv.conv.weight_g.mul_(1.5)
            mod.conv.conv.bias.add_(0.1)
        from encx.modules.lstm import SLSTM
        for seq in (m.encoder.model, m.decoder.model):
            next(mod for mod in seq if isinstance(mod, SLSTM)).lstm.weight_hh_l1.mul_(0.5)
    enc.reset()
    dec.reset()
    codes_stale, emb_stale = enc.encode(x, return_latent=True)
    assert torch.equal(emb_stale, emb) and torch.equal(dec.decode(codes), y)  # still the prepared weights
    enc.refresh_weights()
    dec.refresh_weights()
    enc.reset()
    dec.reset()
    _, emb_new = enc.encode(x, return_latent=True)
    y_new = dec.decode(codes)
    _, emb_fresh = StreamEncoder(m, 1).encode(x, return_latent=True)
    y_fresh = StreamDecoder(m, 1, enc.n_q).decode(codes)
    assert not torch.equal(emb_new, emb) and not torch.equal(y_new, y)
    assert torch.equal(emb_new, emb_fresh) and torch.equal(y_new, y_fresh)


def test_first_chunk_too_short_is_refused_before_any_launch(mono):
    from encx.streaming import StreamEncoder, StreamDecoder
    enc = StreamEncoder(mono.m, 1, graphs=False)
    dec = StreamDecoder(mono.m, 1, mono.n_q, graphs=False)
    assert enc.min_first_frames == dec.min_first_frames == 7 and enc.hop_length == 320
    state = enc._s._arena.clone()
    with pytest.raises(ValueError, match='first chunk'):
        enc.encode(mono.x[:1, :, :6 * HOP].to(DEV))
    with pytest.raises(ValueError, match='first chunk'):
        dec.decode(mono.codes_o[:, :, :6].to(DEV))
    assert torch.equal(enc._s._arena, state)  # nothing ran
    # and the session is still usable: a 7-frame first chunk, then a 1-frame chunk
    enc.encode(mono.x[:1, :, :7 * HOP].to(DEV))
    assert enc.encode(mono.x[:1, :, 7 * HOP:8 * HOP].to(DEV)).shape == (1, mono.n_q, 1)
    with pytest.raises(ValueError):
        enc.encode(mono.x[:1, :, :9 * HOP].to(DEV))  # more than max_frames
