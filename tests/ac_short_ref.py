"""A restatement of oracle/ac_oracle.encode's loop with both ways to end a run -- TEST HELPER.

`encode(symbols, cdfs, bits, short=False)` is ac_oracle.encode (the reference's flush: the
max_bit + 1 pending bits of `low`), restated so that tests/test_stream_lm_nq.py can pin it to the
oracle byte for byte. `short=True` ends the run with the SHORT FLUSH of packet format 2
(include/encx.h): with W = max_bit + 1 and j the largest of 0..W for which v = ceil(low / 2^j) 2^j
<= high, the W bits of v go out most significant first and trailing zero bytes are dropped; the
decoder reads zero bits past the end, so it sees v followed by zeros: a value in [low, high].
`decode_padded` is ac_oracle.decode on the payload followed by zero bytes.
"""
from oracle import ac_oracle as A


def encode(symbols, cdfs, total_range_bits=24, short=False):
    low, high, max_bit = 0, 0, -1
    out = []
    for sym, cdf in zip(symbols, cdfs):
        sym = int(sym)
        while high - low + 1 < 2 ** total_range_bits:
            low *= 2
            high = high * 2 + 1
            max_bit += 1
        range_low = 0 if sym == 0 else int(cdf[sym - 1])
        range_high = int(cdf[sym]) - 1
        el, eh = A._eff(range_low, range_high, high - low + 1, total_range_bits)
        high = low + eh
        low = low + el
        assert low <= high < 2 ** (max_bit + 1)
        while max_bit >= 0:
            b1, b2 = low >> max_bit, high >> max_bit
            if b1 != b2:
                break
            low -= b1 << max_bit
            high -= b1 << max_bit
            max_bit -= 1
            out.append(b1)
        assert max_bit <= 61, max_bit
    W = max_bit + 1
    v = low
    if short:
        for j in range(W, -1, -1):
            v = -((-low) >> j) << j   # low rounded up to a multiple of 2^j
            if v <= high:
                break
        assert low <= v <= high
    out += [(v >> i) & 1 for i in range(W - 1, -1, -1)]
    data = A.pack_bits(out)
    return data.rstrip(b'\0') if short else data


def decode_padded(data, cdfs, total_range_bits=24):
    """What a format-2 decoder sees: the payload, then zero bits for ever."""
    pad = (len(cdfs) * (total_range_bits + 1) + 64) // 8 + 1
    return A.decode(bytes(data) + bytes(pad), cdfs, total_range_bits)
