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


def arch_model(name, **over):
    """fixtures.ARCHS[name] as an EncodecModel (two codebooks, no normalisation, no segments)."""
    import fixtures
    import encx.modules as M
    from encx.quantization import ResidualVectorQuantizer
    kw = {k: v for k, v in fixtures.ARCHS[name].items() if k != 'seed'}
    kw.update(over, ratios=list(kw['ratios']))
    enc, dec = M.SEANetEncoder(**kw), M.SEANetDecoder(**kw)
    m = EncodecModel(enc, dec, ResidualVectorQuantizer(dimension=kw['dimension'], n_q=2, bins=1024), [80.], 24000,
                     kw['channels'], normalize=False, segment=None)
    m.set_target_bandwidth(80.)
    return m.eval()


def test_layer_plan_of_a_dilated_three_block_model():
    """Arch A: ratios (3, 2), three blocks per stage with dilations 1, 2, 4, one LSTM layer."""
    from encx import streaming as S
    m = arch_model('A')
    enc, dec = S.encoder_plan(m), S.decoder_plan(m)
    for plan in (enc, dec):
        for L in plan.layers:
            if L.kind == 'conv':
                assert L.P == (L.K - 1) * L.dilation - (L.stride - 1), L.name
                assert plan.windows[L.src].P >= L.P
        k3 = [L for L in plan.layers if L.kind == 'conv' and L.K == 3]
        assert [L.dilation for L in k3] == [1, 2, 4] * 2
        # each dilated conv is the only consumer with a history of its block's input window
        assert [plan.windows[L.src].P for L in k3] == [2, 4, 8] * 2
        assert {L.module.lstm.num_layers for L in plan.layers if L.kind == 'lstm'} == {1}
    rates = lambda plan: [plan.windows[L.src].rate for L in plan.layers if L.kind == 'conv' and L.K == 3]
    assert rates(enc) == [6] * 3 + [3] * 3 and rates(dec) == [3] * 3 + [6] * 3
    assert [(L.K, L.stride, L.P) for L in enc.layers if L.kind == 'conv' and L.stride > 1] == [(4, 2, 2), (6, 3, 3)]
    assert [(L.K, L.stride) for L in dec.layers if L.kind == 'convtr'] == [(6, 3), (4, 2)]
    assert sorted({w.rate for w in enc.windows}) == sorted({w.rate for w in dec.windows}) == [1, 3, 6]
    assert (enc.windows[0].rate, enc.windows[enc.layers[-1].dst].rate) == (6, 1)
    assert (dec.windows[0].rate, dec.windows[dec.layers[-1].dst].rate) == (1, 6)
    assert enc.hop_length == dec.hop_length == 6
    # the smallest first chunk, from the plan's windows: every reflect-filled history of P columns
    # needs more than P columns, at `rate` columns per frame
    for plan in (enc, dec):
        want = max(w.P // w.rate + 1 for w in plan.windows if w.P and w.fill == 'reflect')
        assert plan.min_first_frames == want == 7  # the K = 7 conv at one column per frame


def test_identity_shortcut_is_refused_by_name():
    from encx import streaming as S
    m = arch_model('B')
    with pytest.raises(NotImplementedError, match=r'identity shortcut \(true_skip=True\)'):
        S.StreamEncoder(m, 1)
    with pytest.raises(NotImplementedError, match=r'identity shortcut \(true_skip=True\)'):
        S.StreamDecoder(m, 1, 2)


@pytest.mark.parametrize('lstm', [0, 3])
def test_plans_build_without_an_lstm_and_with_three_layers(lstm):
    from encx import streaming as S
    m = arch_model('A', lstm=lstm)
    for plan in (S.encoder_plan(m), S.decoder_plan(m)):
        ls = [L for L in plan.layers if L.kind == 'lstm']
        assert len(ls) == (1 if lstm else 0) and all(L.module.lstm.num_layers == lstm for L in ls)
        assert plan.hop_length == 6 and plan.min_first_frames == 7


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
