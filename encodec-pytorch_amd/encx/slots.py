"""What the per-slot layers (encx/streaming.py, the live streams of encx/lm.py) share: the host
checks of a step's per-slot arguments, and the int32 tables in device memory that the kernels
read them from (include/encx.h: the slot table, nq, conceal)."""
import operator
import typing as tp

import torch


# ---------------------------------------------------------------------------- per-slot validation
def _ints(values, what):
    try:
        return [operator.index(v) for v in values]
    except TypeError:
        raise ValueError(f'encx streaming: {what} must be a sequence of ints') from None


def check_frames(started: tp.Sequence[bool], frames, min_first_frames: int, max_frames: int):
    """frames[b] = latent frames slot b delivers this step, checked against each slot's own state
    (started[b]: it has had its first chunk). -> (n_max, any_first): the columns the step
    computes and whether any slot is on its first chunk. Raises ValueError; host data only."""
    frames = _ints(frames, 'frames')
    if len(frames) != len(started):
        raise ValueError(f'encx streaming: frames for {len(frames)} slots, the session has {len(started)}')
    any_first = False
    for b, (on, f) in enumerate(zip(started, frames)):
        if not 0 <= f <= max_frames:
            raise ValueError(f'encx streaming: a chunk of {f} frames in slot {b} (0..max_frames={max_frames})')
        if f and not on:
            if f < min_first_frames:
                raise ValueError(f'encx streaming: the first chunk of slot {b} needs at least '
                                 f'{min_first_frames} frames (got {f})')
            any_first = True
    if not any(frames):
        raise ValueError('encx streaming: no slot delivers a frame')
    return max(frames), any_first


def check_n_q(frames, n_q, n_q_max: int) -> tp.List[int]:
    """n_q[b] = the codebooks slot b uses this step: an int in 1..n_q_max for a slot that delivers
    frames; whatever stands at a slot with 0 frames is ignored. -> the table the kernels read, with
    0 at the slots that sit out. Raises ValueError; host data only."""
    try:
        n_q = list(n_q)
    except TypeError:
        raise ValueError('encx streaming: n_q must be a sequence of ints') from None
    if len(n_q) != len(frames):
        raise ValueError(f'encx streaming: n_q for {len(n_q)} slots, the step has {len(frames)}')
    out = []
    for b, (f, q) in enumerate(zip(frames, n_q)):
        if not f:
            out.append(0)
            continue
        try:
            q = operator.index(q)
        except TypeError:
            raise ValueError(f'encx streaming: n_q of slot {b} is not an int') from None
        if not 1 <= q <= n_q_max:
            raise ValueError(f'encx streaming: n_q {q} in slot {b} (1..{n_q_max})')
        out.append(q)
    return out


def check_fec(frames, fec, fec_max: int) -> tp.List[int]:
    """fec[b] = the most codebooks of its previous packet slot b's packet repeats this step: an int
    in 0..fec_max (0: no copy) for a slot that delivers frames; whatever stands at a slot with 0
    frames is ignored. None: fec_max for every slot. -> the counts, 0 at the slots that sit out.
    Raises ValueError; host data only."""
    if fec is None:
        return [fec_max if f else 0 for f in frames]
    try:
        fec = list(fec)
    except TypeError:
        raise ValueError('encx streaming: fec must be a sequence of ints') from None
    if len(fec) != len(frames):
        raise ValueError(f'encx streaming: fec for {len(fec)} slots, the step has {len(frames)}')
    out = []
    for b, (f, r) in enumerate(zip(frames, fec)):
        if not f:
            out.append(0)
            continue
        try:
            r = operator.index(r)
        except TypeError:
            raise ValueError(f'encx streaming: fec of slot {b} is not an int') from None
        if not 0 <= r <= fec_max:
            raise ValueError(f'encx streaming: fec {r} in slot {b} (0..{fec_max})')
        out.append(r)
    return out


def check_restart(slots, batch: int) -> tp.List[int]:
    """The slot indices of a restart(), each in 0..batch-1 (ValueError otherwise)."""
    slots = _ints(slots, 'slots')
    for b in slots:
        if not 0 <= b < batch:
            raise ValueError(f'encx streaming: slot {b} (0..{batch - 1})')
    return slots


# ---------------------------------------------------------------------------- a table the kernels read
class DeviceTable:
    """An int32 table in device memory, [B, width] ([B] for width 1), refilled from the host
    before a step and read by its kernels, so that one captured graph serves every step. `t` is
    the device tensor, `host` the rows it was last given, `uploads` how often it was written."""

    def __init__(self, B: int, width: int, device):
        shape = (B,) if width == 1 else (B, width)
        self.t = torch.zeros(shape, device=device, dtype=torch.int32)
        self.host: tp.Optional[tuple] = None
        self.uploads = 0
        self._staging = [(torch.zeros(shape, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                         for _ in range(4)]
        self._staged = 0

    def data_ptr(self):
        return self.t.data_ptr()

    def put(self, rows):
        """Fill the table for this step (B ints, or B rows of `width` ints), only when it differs
        from the last upload. The host runs ahead of the device, so one pinned buffer would be
        rewritten while the copy of an earlier step still reads it: the staging buffers rotate,
        each guarded by the event of the copy that last read it."""
        rows = tuple(rows)
        if rows == self.host:
            return
        buf, ev = self._staging[self._staged]
        self._staged = (self._staged + 1) % len(self._staging)
        ev.synchronize()
        buf.copy_(torch.tensor(rows, dtype=torch.int32))
        self.t.copy_(buf, non_blocking=True)
        ev.record()
        self.host = rows
        self.uploads += 1

    def clear(self):
        """Zero the device copy, on the stream, and forget the host's: the next put uploads."""
        self.t.zero_()
        self.host = None
