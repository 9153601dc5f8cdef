"""Streaming codec step time: encx.streaming.StreamEncoder.encode / StreamDecoder.decode for B
live streams advancing n latent frames per step (n * 320 samples each at 24 kHz), eager and as
the replayed HIP graph, at B in {1, 16, 64} and n in {1, 4}.

For comparison the offline kernels on a chunk of the same shape: model.encoder on [B, 1, n * 320]
and model.decoder on [B, 128, n] (plus the same RVQ calls). That is what the existing kernels
cost at this size; its result is NOT the stream's (every layer pads the chunk's own edges).

The model is the causal 24 kHz architecture with its default random initialisation and random
codebooks (nothing is read from outside the repository); the audio is seeded noise. A session is
started with one first chunk of min_first_frames frames, then steps of n frames are timed: device
events around blocks of steps, >= 0.3 s per variant, 5 rounds after a warm-up; median and the
rounds' min / max. `real_time` is the one derived condition: at B = 64, n = 1 an encode step plus
a decode step (graph replay) must take less than the frame period, 1000 / 75 = 13.33 ms.

--slots measures the per-slot entry points instead (encode_slots / decode_slots / restart, see
slots_section) and writes profiles/stream/stream_bench_slots.json; there the real-time condition
is the join step's encode plus decode against the frame period.

python tools/stream_bench.py [--batches 1,16,64] [--frames 1,4] [--rounds 5] [--out FILE]
--nq measures a bandwidth (n_q) per slot (nq_section: the fused quantizer against the step without
n_q) and writes profiles/stream/stream_bench_nq.json.

--conceal measures loss concealment (conceal_section: decode_slots with lost slots against the
same session's loss-free step) and writes profiles/stream/stream_bench_conceal.json.

python tools/stream_bench.py --slots [--rounds 5] [--slots-out FILE]
python tools/stream_bench.py --nq [--rounds 5] [--nq-out FILE]
python tools/stream_bench.py --conceal [--rounds 5] [--conceal-out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))

BANDWIDTH = 6.0  # n_q = 8


def stats(ms):
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def slots_section(args, torch, m, dev, hop, period_ms, measure, B=64, join=7):
    """Per-slot steps at B = 64 (graph replay), one session pair for all of it:
      sustained   every slot delivers 1 frame through encode_slots / decode_slots, against the
                  same through encode / decode (the slot table does not change: no upload);
      join        63 slots deliver 1 frame and one slot, restarted just before, its first 7; the
                  joining slot moves on by one every step, so every step uploads a new table;
      uniform     every slot delivers 7 frames through encode / decode: the join step computes
                  the same columns, so this is what it should cost."""
    from encx.streaming import StreamEncoder, StreamDecoder
    g = torch.Generator().manual_seed(6400)
    noise = lambda n: (0.1 * torch.randn(B, 1, n * hop, generator=g)).to(dev)
    enc = StreamEncoder(m, B)
    dec = StreamDecoder(m, B, enc.n_q)
    x1, x7 = noise(1), noise(join)
    ones = [1] * B
    c7 = enc.encode(x7)
    dec.decode(c7)
    c1 = enc.encode(x1)
    joins = [[join if b == j else 1 for b in range(B)] for j in range(B)]
    turn = {'enc': 0, 'dec': 0}

    def join_step(side, obj, fn, arg):
        j = turn[side] = (turn[side] + 1) % B
        obj.restart([j])
        fn(arg, joins[j])

    res = {}
    for key, fn in (('sustained_encode_slots', lambda: enc.encode_slots(x1, ones)),
                    ('sustained_encode', lambda: enc.encode(x1)),
                    ('sustained_decode_slots', lambda: dec.decode_slots(c1, ones)),
                    ('sustained_decode', lambda: dec.decode(c1)),
                    ('join_encode', lambda: join_step('enc', enc, enc.encode_slots, x7)),
                    ('uniform7_encode', lambda: enc.encode(x7)),
                    ('join_decode', lambda: join_step('dec', dec, dec.decode_slots, c7)),
                    ('uniform7_decode', lambda: dec.decode(c7))):
        res[key], _ = measure(fn)
        print(json.dumps({key: res[key]}), flush=True)
    ms = lambda k: res[k]['ms']
    join_ms = ms('join_encode') + ms('join_decode')
    return {'metric': f'ms per streaming step at B = {B} (graph replay), per-slot entry points',
            'device': torch.cuda.get_device_name(0), 'model': 'causal 24 kHz SEANet, random weights, n_q 8',
            'frame_period_ms': round(period_ms, 4), 'rounds': args.rounds,
            'timing': f'device events around blocks of steps, >= {args.min_seconds} s per variant, after warm-up',
            'steps': res,
            'sustained_slots_over_uniform': {s: round(ms(f'sustained_{s}_slots') / ms(f'sustained_{s}'), 4)
                                             for s in ('encode', 'decode')},
            'join_over_uniform7': {'encode': round(ms('join_encode') / ms('uniform7_encode'), 4),
                                   'decode': round(ms('join_decode') / ms('uniform7_decode'), 4),
                                   'encode_plus_decode': round(
                                       join_ms / (ms('uniform7_encode') + ms('uniform7_decode')), 4)},
            'real_time': {'B': B, 'step': f'join: 63 slots x 1 frame, one slot its first {join}',
                          'encode_plus_decode_graph_ms': round(join_ms, 4),
                          'frame_period_ms': round(period_ms, 4), 'met': join_ms < period_ms}}


def nq_section(args, torch, m, dev, hop, timed, B=64):
    """A bandwidth (n_q) per slot at B = 64, n = 1 and 8 frames per step, K_max = 8 and 32, eager
    and graph replay, encode step and decode step apart:
      a   encode_slots / decode_slots with n_q = K_max for every slot (the fused quantizer);
      b   the same with the slots cycling through 2, 4, 8, .., K_max codebooks;
      c   encode_slots / decode_slots without n_q at K_max (the per-layer quantizer kernels).
    The three run alternately, round by round, in one process (each round is one block of steps
    per case). The quantizer alone (q_*: the step's [B, 128, n] latent, launched back to back) is
    timed in the eager rounds."""
    from encx.streaming import StreamEncoder, StreamDecoder
    rows = []
    for K in (8, 32):
        ladder = [k for k in (2, 4, 8, 16, 32, 64) if k <= K]
        full, mixed = [K] * B, [ladder[b % len(ladder)] for b in range(B)]
        for n in (1, 8):
            g = torch.Generator().manual_seed(1000 * K + n)
            x = (0.1 * torch.randn(B, 1, n * hop, generator=g)).to(dev)
            frames = [n] * B
            for graphs in (False, True):
                enc, dec = StreamEncoder(m, B, graphs=graphs, n_q=K), StreamDecoder(m, B, K, graphs=graphs)
                enc_c, dec_c = StreamEncoder(m, B, graphs=graphs, n_q=K), StreamDecoder(m, B, K, graphs=graphs)
                mf = [enc.min_first_frames] * B
                first = (0.1 * torch.randn(B, 1, mf[0] * hop, generator=g)).to(dev)
                dec.decode_slots(enc.encode_slots(first, mf, n_q=full), mf, n_q=full)
                dec_c.decode_slots(enc_c.encode_slots(first, mf), mf)
                codes = enc_c.encode_slots(x, frames)
                fns = {'a_encode': lambda: enc.encode_slots(x, frames, n_q=full),
                       'b_encode': lambda: enc.encode_slots(x, frames, n_q=mixed),
                       'c_encode': lambda: enc_c.encode_slots(x, frames),
                       'a_decode': lambda: dec.decode_slots(codes, frames, n_q=full),
                       'b_decode': lambda: dec.decode_slots(codes, frames, n_q=mixed),
                       'c_decode': lambda: dec_c.decode_slots(codes, frames)}
                if not graphs:  # the quantizer alone on the step's [B, 128, n] latent, launched back to back
                    from encx import ops
                    lat = torch.randn(B, 128, n, generator=g).to(dev)
                    slots = torch.tensor([(n, 0)] * B, dtype=torch.int32, device=dev)
                    nqt = torch.tensor(full, dtype=torch.int32, device=dev)
                    cq = codes.permute(1, 0, 2).contiguous()
                    fns.update({'q_fused_encode': lambda: ops.stream_rvq_encode_slots(lat, enc._books, slots, nqt),
                                'q_layers_encode': lambda: ops.rvq_encode(lat, enc._embeds),
                                'q_fused_decode': lambda: ops.stream_rvq_decode_slots(codes, enc._books, slots, nqt),
                                'q_layers_decode': lambda: ops.rvq_decode(cq, enc._embeds)})
                iters = {}
                for k, fn in fns.items():
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    iters[k] = max(5, int(args.min_seconds * 1e3 / args.rounds / max(timed(fn, 5), 1e-3)) + 1)
                ms = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for k, fn in fns.items():
                        ms[k].append(timed(fn, iters[k]))
                row = {'K_max': K, 'n': n, 'mode': 'graph' if graphs else 'eager'}
                row.update({k: stats(v) for k, v in ms.items()})
                for side in ('encode', 'decode'):
                    row[f'a_over_c_{side}'] = round(row[f'a_{side}']['ms'] / row[f'c_{side}']['ms'], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {'metric': f'ms per streaming step at B = {B}: a = n_q K_max per slot (fused quantizer), b = slots '
                      'cycling 2, 4, .., K_max, c = the step without n_q at K_max (per-layer quantizer kernels)',
            'device': torch.cuda.get_device_name(0), 'model': 'causal 24 kHz SEANet, random weights',
            'rounds': args.rounds,
            'timing': f'device events around blocks of steps, >= {args.min_seconds} s per case, the cases '
                      'alternating round by round, after warm-up', 'rows': rows}


def conceal_section(args, torch, m, dev, hop, timed, B=64, K=8):
    """Loss concealment at B = 64 (graph replay), n = 1 and 4 frames per step, on the per-layer
    dequantizer (decode_slots without n_q) and on the fused one (with n_q): the decode step with
    none, one in eight and all of the slots lost, one session per (path, n). `none` is the
    session's loss-free decode_slots step, the step every session ran before; the cases alternate
    round by round, and each block is preceded by two untimed steps, so that the fade back to full
    level after a block of losses (one frame with the default conceal_recover) is not in it."""
    from encx.streaming import StreamDecoder
    shares = {'none': [False] * B, 'eighth': [b % 8 == 0 for b in range(B)], 'all': [True] * B}
    rows = []
    for path in ('layers', 'fused'):
        for n in (1, 4):
            g = torch.Generator().manual_seed(7000 + n)
            dec = StreamDecoder(m, B, K)
            mf, frames, nq = [dec.min_first_frames] * B, [n] * B, [K] * B
            kw = {'n_q': nq} if path == 'fused' else {}
            dec.decode_slots(torch.randint(0, 1024, (B, K, mf[0]), generator=g).to(dev), mf, **kw)
            codes = torch.randint(0, 1024, (B, K, n), generator=g).to(dev)
            fns = {k: (lambda lost=lost: dec.decode_slots(codes, frames, lost=lost, **kw)) for k, lost in shares.items()}

            def block(fn, iters):
                fn()
                fn()
                torch.cuda.synchronize()
                return timed(fn, iters)

            iters = {k: max(5, int(args.min_seconds * 1e3 / args.rounds / max(block(fn, 5), 1e-3)) + 1)
                     for k, fn in fns.items()}
            ms = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    ms[k].append(block(fn, iters[k]))
            row = {'path': path, 'n': n}
            row.update({k: stats(v) for k, v in ms.items()})
            for k in ('eighth', 'all'):
                row[f'{k}_over_none'] = round(row[k]['ms'] / row['none']['ms'], 4)
            row['none_spread'] = round((row['none']['max'] - row['none']['min']) / row['none']['ms'], 4)
            row['conceal_graphs'] = len(dec._s.graph_keys('conceal'))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {'metric': f'ms per decode_slots step at B = {B} (graph replay), n_q {K}: none / one in eight / all of '
                      'the slots lost; none is the loss-free step of the same session',
            'device': torch.cuda.get_device_name(0), 'model': 'causal 24 kHz SEANet, random weights',
            'rounds': args.rounds,
            'timing': f'device events around blocks of steps, >= {args.min_seconds} s per case, the cases '
                      'alternating round by round, two untimed steps before each block', 'rows': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--conceal', action='store_true', help='only the loss concealment section (B = 64)')
    ap.add_argument('--conceal-out', type=str,
                    default=os.path.join(ROOT, 'profiles', 'stream', 'stream_bench_conceal.json'))
    ap.add_argument('--nq', action='store_true', help='only the per-slot bandwidth section (B = 64)')
    ap.add_argument('--nq-out', type=str, default=os.path.join(ROOT, 'profiles', 'stream', 'stream_bench_nq.json'))
    ap.add_argument('--slots', action='store_true', help='only the per-slot section (B = 64)')
    ap.add_argument('--slots-out', type=str,
                    default=os.path.join(ROOT, 'profiles', 'stream', 'stream_bench_slots.json'))
    ap.add_argument('--batches', type=str, default='1,16,64')
    ap.add_argument('--frames', type=str, default='1,4')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'stream', 'stream_bench.json'))
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(',')]
    frames = [int(v) for v in args.frames.split(',')]

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_bench needs the GPU: nothing is measured without one')
    from encx.model import EncodecModel
    from encx.streaming import StreamEncoder, StreamDecoder
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = EncodecModel.encodec_model_24khz()
    for layer in m.quantizer.vq.layers:
        layer._codebook.embed.normal_()
        layer._codebook.inited.fill_(1.0)
    m.set_target_bandwidth(BANDWIDTH)
    m = m.to(dev)
    hop, period_ms = int(m.encoder.hop_length), 1e3 / m.frame_rate

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def measure(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        iters = max(5, int(args.min_seconds * 1e3 / args.rounds / max(timed(fn, 5), 1e-3)) + 1)
        return stats([timed(fn, iters) for _ in range(args.rounds)]), iters

    if args.conceal:
        with torch.no_grad():
            res = conceal_section(args, torch, m, dev, hop, timed)
        if args.conceal_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.conceal_out)), exist_ok=True)
            with open(args.conceal_out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return

    if args.nq:
        with torch.no_grad():
            res = nq_section(args, torch, m, dev, hop, timed)
        if args.nq_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.nq_out)), exist_ok=True)
            with open(args.nq_out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return

    if args.slots:
        with torch.no_grad():
            res = slots_section(args, torch, m, dev, hop, period_ms, measure)
        print(json.dumps(res), flush=True)
        if args.slots_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.slots_out)), exist_ok=True)
            with open(args.slots_out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return

    rows = []
    with torch.no_grad():
        for B in batches:
            for n in frames:
                g = torch.Generator().manual_seed(100 * B + n)
                x = (0.1 * torch.randn(B, 1, n * hop, generator=g)).to(dev)
                row = {'B': B, 'n': n, 'samples_per_step': n * hop}
                for graphs in (False, True):
                    enc = StreamEncoder(m, B, graphs=graphs)
                    dec = StreamDecoder(m, B, enc.n_q, graphs=graphs)
                    first = (0.1 * torch.randn(B, 1, enc.min_first_frames * hop, generator=g)).to(dev)
                    dec.decode(enc.encode(first))
                    codes = enc.encode(x)
                    mode = 'graph' if graphs else 'eager'
                    row[f'encode_{mode}'], it = measure(lambda: enc.encode(x))
                    row[f'decode_{mode}'], _ = measure(lambda: dec.decode(codes))
                    row[f'steps_per_round_{mode}'] = it
                # the offline kernels on a chunk of the same shape (wrong edges: for the cost only)
                embeds = [l._codebook.embed for l in m.quantizer.vq.layers[:enc.n_q]]
                from encx import ops
                cq = codes.permute(1, 0, 2).contiguous()
                for key, fn in (('offline_encode_same_shape', lambda: ops.rvq_encode(m.encoder(x), embeds)),
                                ('offline_decode_same_shape', lambda: m.decoder(ops.rvq_decode(cq, embeds)))):
                    try:
                        row[key], _ = measure(fn)
                    except (RuntimeError, NotImplementedError) as e:
                        if isinstance(e, RuntimeError) and 'code 9001' not in str(e):
                            raise  # only a refused shape (ENCX_EINVAL) is a result; anything else ends the run
                        row[key] = {'error': str(e)[:200]}
                step = row['encode_graph']['ms'] + row['decode_graph']['ms']
                row['encode_plus_decode_graph_ms'] = round(step, 4)
                row['frame_periods_per_step'] = round(step / (n * period_ms), 4)
                rows.append(row)
                print(json.dumps(row), flush=True)

    rt = [r for r in rows if r['B'] == 64 and r['n'] == 1]
    res = {'metric': 'ms per streaming step (B streams x n latent frames), encode and decode',
           'device': torch.cuda.get_device_name(0), 'model': 'causal 24 kHz SEANet, random weights, n_q 8',
           'frame_period_ms': round(period_ms, 4), 'rounds': args.rounds,
           'timing': f'device events around blocks of steps, >= {args.min_seconds} s per variant, after warm-up',
           'rows': rows,
           'real_time': None if not rt else {
               'B': 64, 'n': 1, 'encode_plus_decode_graph_ms': rt[0]['encode_plus_decode_graph_ms'],
               'frame_period_ms': round(period_ms, 4),
               'met': rt[0]['encode_plus_decode_graph_ms'] < period_ms}}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
