"""Streaming packets: what a step's packets cost and what they weigh (encx.streaming.StreamPacker /
StreamUnpacker, encx.lm.LMStreamEncoder / LMStreamDecoder).

Times. B in {1, 64} slots, every slot n in {1, 8} frames, K = 8 codebooks of 10 bits: pack_slots
and unpack_slots, raw and LM-coded (the 24 kHz LM's size: 32 x 1024, dim 200, 5 layers,
past_context 262, random weights), the LM form eager and as the replayed graph. Every call
includes the host copy of the packets (the bytes have to leave): a host clock around blocks of
calls, each of which ends in a device-to-host copy or a synchronise. After a warm-up, >= 0.3 s per
variant split over 5 rounds; the variants of one (B, n) alternate within each round; median
[min, max] of the rounds. Baselines, what the code before this layer can do, in the same process:
  raw  one ops.pack_codes / ops.unpack_codes per delivering slot;
  LM   lm.encode_streams / lm.decode_streams on each slot's chunk from a fresh state.
The LM unpack consumes a pre-coded sequence of 384 steps and restarts every slot (host only) when
it wraps, so its attention windows grow from 0 to min(262, 384 n) frames over the sequence.

Real time. At B = 64, n = 1 the codec's encode_slots + pack_slots + unpack_slots + decode_slots
(graphs) against the frame period, 1000 / 75 = 13.33 ms, raw and LM-coded.

Bytes. A small LM (1 codebook of 64, dim 64, 1 layer, past_context 20) trained here for 300 Adam
steps on first-order Markov code streams, then 4 unseen streams of 480 frames:
  (a) packets with the context carried, n = 1 and n = 8 (payload bytes; + 1 header byte each);
  (b) the same chunks each coded from a fresh state (lm.encode_streams per chunk);
  (c) each stream as one coder run (lm.encode_streams of the whole stream).
(a) - (c) is what flushing per packet costs, (b) - (a) what carrying the state buys.

Bandwidth per slot (--nq). LM-coded packets of format 2 (a codebook count per slot and step, the
short flush; include/encx.h) at B = 64, n in {1, 8}, K_max in {8, 32}, pack and unpack, graphs:
  (a) format 2, every slot at K_max;   (b) format 2, slots cycling through 2, 4, .., K_max;
  (c) format 2, every slot at 2;       (d) format 1 at K_max, the code before format 2: the baseline.
Same clock and rounds; the unpackers consume a pre-coded sequence of 96 steps. Recorded with every
row: (d)'s spread (max - min) / median, whether (a) is within that spread of (d), and whether (c)
is faster than (a) by more than it. Bytes: the trained toy LM's payload bytes per frame for format
2, format 1 and raw at n = 1 and n = 8; a format-2 payload longer than the format-1 payload of the
same packet stops the tool.

Redundant packets (--fec). Raw packets that repeat the first R = 2 codebooks of the slot's previous
packet (include/encx.h: REDUNDANT PACKET) at B = 64, n in {1, 8}, K = 8, every slot delivering:
  fused         pack_slots of a packer built with fec=2: one launch writes header, both sections and
                the history;
  two_launches  what the code before it can do for the same bytes: pack_slots of a slot_n_q packer on
                this step's codes, a second one on the kept codes of the previous step at 2 rows, and
                the host concatenation header + payload + payload.
The bytes of the two are compared before anything is timed. Same clock and rounds. The byte cost is
arithmetic: 2 header bytes + ceil(n_r K_r bits / 8) per packet, printed beside the raw packet's size.

python tools/stream_packet_bench.py [--rounds 5] [--out profiles/stream/stream_packets.json]
python tools/stream_packet_bench.py --fec [--out profiles/stream/stream_packets_fec.json]
python tools/stream_packet_bench.py --nq [--out profiles/stream/stream_packets_nq.json]
python tools/stream_packet_bench.py --nq --trace   # only 20 eager pack + unpack steps of (a) and of (d) at
                                                   # B = 64, n = 8, K_max = 32, for a kernel trace of its own
python tools/stream_packet_bench.py --trace   # only 20 LM steps and 20 raw packs at B = 64, n = 1,
                                              # for a kernel trace of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))

BANDWIDTH, K, BITS, CARD = 6.0, 8, 10, 1024
SEQ = 384  # pre-coded steps the LM unpack consumes before its slots restart


def stats(ms):
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def measure(torch, variants, rounds, min_seconds):
    """{name: fn} -> {name: stats}: warm-up, then `rounds` rounds in which the variants alternate."""
    iters = {}
    for name, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = max(time.perf_counter() - t0, 1e-6)
        iters[name] = max(1, int(min_seconds / rounds / one) + 1)
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters[name]):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / iters[name])
    return {name: dict(stats(v), calls_per_round=iters[name]) for name, v in ms.items()}


def timing_row(torch, m, lm, B, n, args):
    from encx import ops
    from encx.streaming import StreamPacker, StreamUnpacker
    dev = next(m.parameters()).device
    g = torch.Generator().manual_seed(1000 * B + n)
    frames = [n] * B
    codes = torch.randint(0, CARD, (B, K, n), generator=g).to(dev)
    v = {}
    # raw
    packer, unpacker = StreamPacker(m, B, K), StreamUnpacker(m, B, K)
    packets = packer.pack_slots(codes, frames)
    v['raw_pack'] = lambda: packer.pack_slots(codes, frames)
    v['raw_unpack'] = lambda: unpacker.unpack_slots(packets)
    def pack_one(b):  # the bytes and the error flag both have to reach the host, as in pack_slots
        out, err = ops.pack_codes(codes[b:b + 1], BITS)
        return out.cpu(), int(err.item())

    v['raw_pack_baseline'] = lambda: [pack_one(b) for b in range(B)]
    payloads = [torch.frombuffer(bytearray(p[1:]), dtype=torch.uint8).view(1, -1) for p in packets]
    v['raw_unpack_baseline'] = lambda: [ops.unpack_codes(p.to(dev), K, n, BITS) for p in payloads]
    # LM-coded: the packer runs on for ever; the unpacker consumes a pre-coded sequence
    for graphs in (False, True):
        mode = 'graph' if graphs else 'eager'
        lp = StreamPacker(m, B, K, use_lm=True, lm=lm, graphs=graphs)
        lu = StreamUnpacker(m, B, K, use_lm=True, lm=lm, graphs=graphs)
        seq = [lp.pack_slots(torch.randint(0, CARD, (B, K, n), generator=g).to(dev), frames) for _ in range(SEQ)]
        state = {'i': 0}

        def unpack(lu=lu, seq=seq, state=state):
            if state['i'] == SEQ:
                lu.restart(range(B))
                state['i'] = 0
            _, fr = lu.unpack_slots(seq[state['i']])
            assert fr == frames
            state['i'] += 1

        v[f'lm_pack_{mode}'] = lambda lp=lp: lp.pack_slots(codes, frames)
        v[f'lm_unpack_{mode}'] = unpack
    datas = [lm.encode_streams(codes[b:b + 1]) for b in range(B)]
    v['lm_pack_baseline'] = lambda: [lm.encode_streams(codes[b:b + 1]) for b in range(B)]
    v['lm_unpack_baseline'] = lambda: [lm.decode_streams(d, K, n) for d in datas]
    row = {'B': B, 'n': n}
    row.update(measure(torch, v, args.rounds, args.min_seconds))
    for k in ('raw_pack', 'raw_unpack'):
        row[f'{k}_baseline_over_slots'] = round(row[f'{k}_baseline']['ms'] / row[k]['ms'], 3)
    for k in ('lm_pack', 'lm_unpack'):
        row[f'{k}_baseline_over_slots_graph'] = round(row[f'{k}_baseline']['ms'] / row[f'{k}_graph']['ms'], 3)
    return row


def real_time(torch, m, lm, args, B=64):
    from encx.streaming import StreamEncoder, StreamDecoder, StreamPacker, StreamUnpacker
    dev = next(m.parameters()).device
    hop, period = int(m.encoder.hop_length), 1e3 / m.frame_rate
    g = torch.Generator().manual_seed(64)
    enc, dec = StreamEncoder(m, B), StreamDecoder(m, B, K)
    first = (0.1 * torch.randn(B, 1, enc.min_first_frames * hop, generator=g)).to(dev)
    dec.decode(enc.encode(first))
    x = (0.1 * torch.randn(B, 1, hop, generator=g)).to(dev)
    ones = [1] * B
    codes = enc.encode_slots(x, ones)
    v = {'encode_slots': lambda: enc.encode_slots(x, ones), 'decode_slots': lambda: dec.decode_slots(codes, ones)}
    rp, ru = StreamPacker(m, B, K), StreamUnpacker(m, B, K)
    packets = rp.pack_slots(codes, ones)
    v['raw_pack'] = lambda: rp.pack_slots(codes, ones)
    v['raw_unpack'] = lambda: ru.unpack_slots(packets)
    lp, lu = StreamPacker(m, B, K, use_lm=True, lm=lm), StreamUnpacker(m, B, K, use_lm=True, lm=lm)

    def lm_pair():  # the two sides stay in step: every packet is unpacked once
        lu.unpack_slots(lp.pack_slots(codes, ones))

    v['lm_pack_plus_unpack'] = lm_pair
    res = measure(torch, v, args.rounds, args.min_seconds)
    codec = res['encode_slots']['ms'] + res['decode_slots']['ms']
    raw = codec + res['raw_pack']['ms'] + res['raw_unpack']['ms']
    coded = codec + res['lm_pack_plus_unpack']['ms']
    return {'B': B, 'n': 1, 'steps': res, 'frame_period_ms': round(period, 4),
            'raw_total_ms': round(raw, 4), 'raw_share_of_period': round(raw / period, 4), 'raw_met': raw < period,
            'lm_total_ms': round(coded, 4), 'lm_share_of_period': round(coded / period, 4), 'lm_met': coded < period}


NQ_SEQ = 96  # pre-coded steps an --nq unpacker consumes before its slots restart


def nq_row(torch, m, lm, B, n, kmax, args):
    """One (n, K_max) row of --nq: variants a, b, c (format 2) and d (format 1), pack and unpack."""
    from encx.streaming import StreamPacker, StreamUnpacker
    dev = next(m.parameters()).device
    g = torch.Generator().manual_seed(100 * kmax + n)
    frames = [n] * B
    codes = torch.randint(0, CARD, (B, kmax, n), generator=g).to(dev)
    tables = {'a_f2_all_kmax': [kmax] * B,
              'b_f2_cycling': [2 * (1 + b % (kmax // 2)) for b in range(B)],
              'c_f2_all_2': [2] * B,
              'd_f1_kmax': None}
    v = {}
    for name, nq in tables.items():
        kw = dict(use_lm=True, lm=lm) if nq is None else dict(use_lm=True, lm=lm, lm_format=2)
        extra = () if nq is None else (nq,)
        lp, lu = StreamPacker(m, B, kmax, **kw), StreamUnpacker(m, B, kmax, **kw)
        seq = [lp.pack_slots(torch.randint(0, CARD, (B, kmax, n), generator=g).to(dev), frames, *extra)
               for _ in range(NQ_SEQ)]
        state = {'i': 0}

        def unpack(lu=lu, seq=seq, state=state):
            if state['i'] == NQ_SEQ:
                lu.restart(range(B))
                state['i'] = 0
            assert lu.unpack_slots(seq[state['i']])[1] == frames
            state['i'] += 1

        v[f'pack_{name}'] = lambda lp=lp, extra=extra: lp.pack_slots(codes, frames, *extra)
        v[f'unpack_{name}'] = unpack
    row = {'B': B, 'n': n, 'K_max': kmax}
    row.update(measure(torch, v, args.rounds, args.min_seconds))
    for side in ('pack', 'unpack'):
        a, c, d = (row[f'{side}_{k}'] for k in ('a_f2_all_kmax', 'c_f2_all_2', 'd_f1_kmax'))
        spread = (d['max'] - d['min']) / d['ms']
        row[f'{side}_d_spread'] = round(spread, 4)
        row[f'{side}_a_over_d'] = round(a['ms'] / d['ms'], 4)
        row[f'{side}_a_within_spread_of_d'] = a['ms'] <= d['ms'] * (1 + spread)
        row[f'{side}_c_gain_over_a'] = round(1 - c['ms'] / a['ms'], 4)
        row[f'{side}_c_faster_than_a_by_more_than_spread'] = 1 - c['ms'] / a['ms'] > spread
    return row


def nq_bytes(torch, dev, steps=300, B=4, T=480):
    """The trained toy LM of bytes_section: payload bytes per frame of format 2, format 1 and raw."""
    from encx.lm import LMStreamEncoder
    lm, codes, loss = toy_lm(torch, dev, steps, B, T)
    res = {'lm': '1 x 64, dim 64, 1 layer, past_context 20', 'train_steps': steps,
           'final_nll_nats_per_code': round(loss, 4), 'streams': B, 'frames_per_stream': T}
    per = lambda nbytes: round(nbytes / (B * T), 4)
    for n in (1, 8):
        e1, e2 = LMStreamEncoder(lm, B, 1, max_frames=8), LMStreamEncoder(lm, B, 1, max_frames=8, lm_format=2)
        f1 = f2 = 0
        for t in range(0, T, n):
            chunk = codes[:, :, t:t + n].contiguous()
            p1, p2 = e1.encode_slots(chunk, [n] * B), e2.encode_slots(chunk, [n] * B, [1] * B)
            for a, b in zip(p1, p2):
                if len(b) > len(a):
                    raise SystemExit(f'a format-2 payload of {len(b)} bytes against {len(a)} in format 1')
            f1, f2 = f1 + sum(map(len, p1)), f2 + sum(map(len, p2))
        packets = B * T // n
        res[f'n{n}'] = {'format2_payload': per(f2), 'format1_payload': per(f1), 'raw_payload': per(-(-n * 6 // 8) * packets),
                        'format2_with_header': per(f2 + 2 * packets), 'format1_with_header': per(f1 + packets),
                        'raw_with_header': per((1 + -(-n * 6 // 8)) * packets),
                        'saved_bytes_per_packet': round((f1 - f2) / packets, 4)}
    return res


FEC_R = 2  # codebooks of the previous packet a --fec packet repeats


def fec_row(torch, m, B, n, args):
    """One n of --fec: the fused packer against two variable-bandwidth packs and a host join."""
    from encx.streaming import StreamPacker, packet_bytes_nq, packet_bytes_fec
    dev = next(m.parameters()).device
    g = torch.Generator().manual_seed(7000 + n)
    frames, nq, kr = [n] * B, [K] * B, [FEC_R] * B
    prev, codes = (torch.randint(0, CARD, (B, K, n), generator=g).to(dev) for _ in range(2))
    fused = StreamPacker(m, B, K, slot_n_q=True, fec=FEC_R)
    main, red = StreamPacker(m, B, K, slot_n_q=True), StreamPacker(m, B, K, slot_n_q=True)
    hdr = bytes([n, K, n, FEC_R])

    def two_launches():
        a, b = main.pack_slots(codes, frames, nq), red.pack_slots(prev, frames, kr)
        return [hdr + p[2:] + q[2:] for p, q in zip(a, b)]

    fused.pack_slots(prev, frames, nq)  # the history now holds `prev`; in the timed calls it holds `codes`
    if fused.pack_slots(codes, frames, nq) != two_launches():
        raise SystemExit('--fec: the fused packer and the two launches disagree on the bytes')
    v = {'fused': lambda: fused.pack_slots(codes, frames, nq), 'two_launches': two_launches}
    row = {'B': B, 'n': n, 'K': K, 'R': FEC_R}
    row.update(measure(torch, v, args.rounds, args.min_seconds))
    f, t = row['fused'], row['two_launches']
    row['two_launches_over_fused'] = round(t['ms'] / f['ms'], 3)
    row['fused_ahead_beyond_the_spreads'] = f['max'] < t['min']
    row['bytes'] = {'variable_bandwidth_packet': packet_bytes_nq(n, K, BITS),
                    'redundant_packet': packet_bytes_fec(n, K, n, FEC_R, BITS),
                    'cost': 2 + (n * FEC_R * BITS + 7) // 8}
    return row


def markov(torch, B, T, seed):
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1234))
    g = torch.Generator().manual_seed(seed)
    c = torch.empty(B, 1, T, dtype=torch.int64)
    c[:, 0, 0] = torch.randint(0, 64, (B,), generator=g)
    for t in range(1, T):
        jump = torch.rand(B, generator=g) < 0.1
        c[:, 0, t] = torch.where(jump, torch.randint(0, 64, (B,), generator=g), perm[c[:, 0, t - 1]])
    return c


def toy_lm(torch, dev, steps, B, T):
    """The small LM of the bytes sections, trained here -> (lm, unseen streams [B, 1, T], final loss)."""
    from encx.lm import LMModel
    from encx.optim import FlatAdam
    torch.manual_seed(77)
    lm = LMModel(1, 64, dim=64, num_heads=2, num_layers=1, past_context=20).to(dev)
    opt = FlatAdam(lm.parameters(), lr=3e-3, eps=1e-5)
    batches = [markov(torch, 8, 48, s).to(dev) for s in range(30)]
    for i in range(steps):
        opt.zero_grad()
        loss = lm.nll(batches[i % len(batches)])
        loss.backward()
        opt.step()
    lm.invalidate_packed()
    lm.eval()
    return lm, markov(torch, B, T, 909).to(dev), float(loss.detach())


def bytes_section(torch, dev, steps=300, B=4, T=480):
    from encx.lm import LMStreamEncoder
    lm, codes, loss = toy_lm(torch, dev, steps, B, T)
    res = {'lm': '1 x 64, dim 64, 1 layer, past_context 20', 'train_steps': steps,
           'final_nll_nats_per_code': round(loss, 4), 'streams': B, 'frames_per_stream': T,
           'raw_bytes_per_frame': 6 / 8}
    per = lambda nbytes: round(nbytes / (B * T), 4)
    res['c_whole_stream_one_run'] = per(sum(len(d) for d in lm.encode_streams(codes)))
    for n in (1, 8):
        enc = LMStreamEncoder(lm, B, 1, max_frames=8)
        carried = sum(len(p) for t in range(0, T, n)
                      for p in enc.encode_slots(codes[:, :, t:t + n].contiguous(), [n] * B))
        chunks = codes.view(B, 1, T // n, n).permute(0, 2, 1, 3).reshape(B * (T // n), 1, n).contiguous()
        fresh = sum(len(d) for d in lm.encode_streams(chunks))
        res[f'n{n}'] = {'a_carried_payload': per(carried), 'a_carried_with_header': per(carried + B * T // n),
                        'b_fresh_state_payload': per(fresh),
                        'flush_cost_a_minus_c': round(per(carried) - res['c_whole_stream_one_run'], 4),
                        'carried_state_gain_b_minus_a': round(per(fresh) - per(carried), 4),
                        'a_with_header_below_raw_with_header': carried + B * T // n < B * T * 6 / 8 + B * T // n}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--trace', action='store_true', help='only a few B = 64, n = 1 steps, for a kernel trace')
    ap.add_argument('--nq', action='store_true', help='format-2 packets (a codebook count per slot) against format 1')
    ap.add_argument('--fec', action='store_true', help='redundant packets: the fused packer against two launches')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.out is None:
        name = 'stream_packets_fec.json' if args.fec else 'stream_packets_nq.json' if args.nq else 'stream_packets.json'
        args.out = os.path.join(ROOT, 'profiles', 'stream', name)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_packet_bench needs the GPU: nothing is measured without one')
    from encx.model import EncodecModel
    from encx.lm import LMModel
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = EncodecModel.encodec_model_24khz()
    for layer in m.quantizer.vq.layers:
        layer._codebook.embed.normal_()
        layer._codebook.inited.fill_(1.0)
    m.set_target_bandwidth(BANDWIDTH)
    m = m.to(dev).eval()
    lm = LMModel(32, CARD, dim=200, num_layers=5, past_context=262).to(dev).eval()

    if args.fec:
        with torch.no_grad():
            rows = [fec_row(torch, m, 64, n, args) for n in (1, 8)]
        for row in rows:
            print(json.dumps(row), flush=True)
        res = {'metric': 'ms per pack step (host copy of the packets included) and bytes per packet',
               'device': torch.cuda.get_device_name(0), 'B': 64, 'K': K, 'R': FEC_R, 'bits': BITS, 'rounds': args.rounds,
               'timing': f'host clock around blocks of calls ending in a synchronise, >= {args.min_seconds} s per '
                         'variant, variants alternating within a round, after warm-up',
               'rows': rows}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
        return
    with torch.no_grad():
        if args.trace and args.nq:
            from encx.streaming import StreamPacker, StreamUnpacker
            B, n, kmax = 64, 8, 32
            frames, nq = [n] * B, [kmax] * B
            codes = torch.randint(0, CARD, (B, kmax, n)).to(dev)
            kw = dict(use_lm=True, lm=lm, graphs=False)
            pa, ua = StreamPacker(m, B, kmax, lm_format=2, **kw), StreamUnpacker(m, B, kmax, lm_format=2, **kw)
            pd, ud = StreamPacker(m, B, kmax, **kw), StreamUnpacker(m, B, kmax, **kw)
            for _ in range(20):
                ua.unpack_slots(pa.pack_slots(codes, frames, nq))
                ud.unpack_slots(pd.pack_slots(codes, frames))
            torch.cuda.synchronize()
            return
        if args.trace:
            from encx.streaming import StreamPacker
            B, ones = 64, [1] * 64
            codes = torch.randint(0, CARD, (B, K, 1)).to(dev)
            rp, lp = StreamPacker(m, B, K), StreamPacker(m, B, K, use_lm=True, lm=lm, graphs=False)
            for _ in range(20):
                rp.pack_slots(codes, ones)
                lp.pack_slots(codes, ones)
            torch.cuda.synchronize()
            return
        if args.nq:
            rows = []
            for kmax in (8, 32):
                for n in (1, 8):
                    rows.append(nq_row(torch, m, lm, 64, n, kmax, args))
                    print(json.dumps(rows[-1]), flush=True)
    if args.nq:
        nbytes = nq_bytes(torch, dev)
        print(json.dumps(nbytes), flush=True)
        res = {'metric': 'ms per call (host copy of the packets included) and payload bytes per frame',
               'device': torch.cuda.get_device_name(0), 'B': 64, 'bits': BITS,
               'lm': '32 x 1024, dim 200, 5 layers, past_context 262, random weights', 'rounds': args.rounds,
               'timing': f'host clock around blocks of calls ending in a synchronise, >= {args.min_seconds} s per '
                         'variant, variants alternating within a round, after warm-up',
               'rows': rows, 'bytes': nbytes}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
        return
    with torch.no_grad():
        rows = []
        for B in (1, 64):
            for n in (1, 8):
                rows.append(timing_row(torch, m, lm, B, n, args))
                print(json.dumps(rows[-1]), flush=True)
        rt = real_time(torch, m, lm, args)
        print(json.dumps(rt), flush=True)
    nbytes = bytes_section(torch, dev)
    print(json.dumps(nbytes), flush=True)
    res = {'metric': 'ms per call (host copy of the packets included) and coded bytes per frame',
           'device': torch.cuda.get_device_name(0), 'K': K, 'bits': BITS,
           'lm': '32 x 1024, dim 200, 5 layers, past_context 262, random weights', 'rounds': args.rounds,
           'timing': f'host clock around blocks of calls ending in a synchronise, >= {args.min_seconds} s per '
                     'variant, variants alternating within a round, after warm-up',
           'rows': rows, 'real_time': rt, 'bytes': nbytes}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
