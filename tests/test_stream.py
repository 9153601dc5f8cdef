"""CPU checks of the streaming codec's host side (encx/streaming.py): the layer plan and its
per-layer history, the smallest first chunk, every refusal (raised on a CPU model, so before any
device call) and the argument validation of the new C entry points."""
import pytest
import torch

from encx.model import EncodecModel


def model(channels=1, causal=True, norm='weight_norm', **kw):
    m = EncodecModel._get_model([1.5, 3., 6., 12., 24.], 24000, channels, causal=causal, model_norm=norm, **kw)
    m.set_target_bandwidth(1.5)
    return m.eval()


def test_layer_plan_histories_of_the_24khz_model():
    from encx import streaming as S
    m = EncodecModel.encodec_model_24khz()
    enc, dec = S.encoder_plan(m), S.decoder_plan(m)
    for plan in (enc, dec):
        for L in plan.layers:
            if L.kind == 'conv':
                assert L.P == (L.K - 1) * L.dilation - (L.stride - 1), L.name
                assert plan.windows[L.src].P >= L.P
            elif L.kind == 'convtr':
                assert L.K == 2 * L.stride and L.P == 1 and plan.windows[L.src].fill == 'zero', L.name
    convs = lambda plan: [(L.K, L.stride, L.P) for L in plan.layers if L.kind == 'conv']
    block = [(1, 1, 0), (3, 1, 2), (1, 1, 0)]  # shortcut, k3, 1x1
    assert convs(enc) == ([(7, 1, 6)] + block + [(4, 2, 2)] + block + [(8, 4, 4)] + block + [(10, 5, 5)]
                          + block + [(16, 8, 8)] + [(7, 1, 6)])
    assert convs(dec) == [(7, 1, 6)] + block * 4 + [(7, 1, 6)]
    assert [(L.K, L.stride) for L in dec.layers if L.kind == 'convtr'] == [(16, 8), (10, 5), (8, 4), (4, 2)]
    assert [L.kind for L in enc.layers].count('lstm') == 1 and [L.kind for L in dec.layers].count('lstm') == 1
    # columns per latent frame: the encoder goes 320 -> 1, the decoder 1 -> 320
    assert (enc.windows[0].rate, enc.windows[enc.layers[-1].dst].rate) == (320, 1)
    assert (dec.windows[0].rate, dec.windows[dec.layers[-1].dst].rate) == (1, 320)
    assert enc.hop_length == dec.hop_length == 320
    # the residual sum: the shortcut writes the block's output, the last conv adds into it
    sc = [L for L in enc.layers if L.name.endswith('.shortcut')]
    assert len(sc) == 4 and all(not L.final and not L.add for L in sc)
    assert sum(L.add for L in enc.layers) == 4


def test_min_first_frames_is_7():
    from encx import streaming as S
    m = EncodecModel.encodec_model_24khz()
    assert S.encoder_plan(m).min_first_frames == 7
    assert S.decoder_plan(m).min_first_frames == 7
    assert S.encoder_plan(model(channels=2)).min_first_frames == 7


def _refused(m, batch=1):
    from encx import streaming as S
    with pytest.raises(NotImplementedError):
        S.StreamEncoder(m, batch)
    with pytest.raises(NotImplementedError):
        S.StreamDecoder(m, batch, 2)


def test_refusals_fire_on_a_cpu_model():
    _refused(model(causal=False))                               # needs the future
    _refused(model(causal=False, norm='time_group_norm'))       # GroupNorm is not causal
    _refused(model(norm='none'))                                # only weight_norm
    _refused(model(audio_normalize=True))                       # the scale needs the whole clip
    _refused(model(segment=1.0))
    _refused(model(channels=3))
    _refused(model(), batch=65)                                 # LSTM_MAX_BATCH
    _refused(model(), batch=0)
    from encx.modules.conv import SConv1d, SConvTranspose1d
    from encx import streaming as S
    m = model()
    next(c for c in m.decoder.modules() if isinstance(c, SConvTranspose1d)).trim_right_ratio = 0.5
    with pytest.raises(NotImplementedError, match='trim_right_ratio'):
        S.StreamDecoder(m, 1, 2)
    m = model()
    for c in m.modules():
        if isinstance(c, SConv1d):
            c.pad_mode = 'constant'
    _refused(m)


def test_supported_cpu_model_has_no_cpu_fallback():
    from encx import streaming as S
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.StreamEncoder(model(), 1)
    with pytest.raises(ValueError, match='max_frames'):
        S.StreamEncoder(model(), 1, max_frames=6)


def test_stream_entry_points_validate_before_any_device_call():
    """As test_abi.py does for encx_conv1d_fwd: NULL pointers / zero sizes -> ENCX_EINVAL."""
    from encx._lib import lib
    l = lib.load()
    assert l.encx_stream_conv1d(*([None] * 4 + [0] * 13 + [None])) == 9001
    assert l.encx_stream_convtr1d(*([None] * 4 + [0] * 10 + [None])) == 9001
    assert l.encx_stream_lstm(*([None] * 7 + [0] * 10 + [None])) == 9001
    assert l.encx_stream_roll(*([None] + [0] * 3 + [None])) == 9001
    # non-NULL pointers (never dereferenced) with a bad shape are refused too
    p = 4096
    assert l.encx_stream_conv1d(p, p, None, p, 1, 4, 4, 8, 3, 1, 1, 4 * 9, 9, 4 * 8, 8, 0, 0, None) == 9001  # row too short
    assert l.encx_stream_conv1d(p, p, None, p, 1, 4, 4, 8, 3, 1, 1, 4 * 10, 10, 4 * 8, 8, 7, 0, None) == 9001  # act
    assert l.encx_stream_convtr1d(p, p, None, p, 1, 4, 4, 8, 2, 4 * 8, 8, 4 * 16, 16, 0, None) == 9001  # no prev column
    assert l.encx_stream_lstm(p, p, p, p, p, p, p, 1, 65, 1, 32, 2, 32, 1, 32, 1, None) == 9001  # B > 64
    assert l.encx_stream_lstm(p, p, p, p, p, p, p, 1, 1, 1, 24, 2, 24, 1, 24, 1, None) == 9001  # H % 16
