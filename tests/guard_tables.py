"""Guard-banded device buffers for the bad-id tests (tests/test_gpu_bad_ids.py).

The ABI promises that an id outside [0, features_M) is read as row 0 by every
kernel (include/hhfm.h).  A kernel that forgets the clamp reads or writes a
neighbouring row instead.  The helpers here make such an access *visible* and
keep it *harmless*:

* ``guarded(t, pad_rows)`` puts a table inside a larger buffer of its own with
  ``pad_rows`` (or more) rows of quiet NaN in front of it and behind it.  A read
  of row −1 or row M then yields NaN (the output stops being finite); a write
  changes a pad, which ``pads_untouched`` finds by comparing bit patterns.
* ``guarded_workspace(nbytes)`` does the same for a byte workspace: guards of
  0xA5 bytes around the ``nbytes`` the entry point is told about.
* ``poisoned_workspace(nbytes, fill, zero_prefix)`` is the same buffer with its
  interior filled with a poison byte instead of zeros (the workspace-contract
  tests, tests/test_gpu_workspace_contract.py): a kernel that reads scratch it
  never wrote then computes with the poison.
* ``near_miss_ids(M, P)`` are the only bad ids the tests use: −P … −1 and
  M … M + P − 1.  With pads of at least ``P`` rows an unclamped access lands in
  memory this module allocated.

Nothing built from these helpers can fault the device, whether the code under
test is right or wrong: no id further than ``P`` rows outside the table ever
reaches a kernel that looks rows up.
"""
import numpy as np
import torch

PAD_ROWS = 8            # P: rows of padding, and the reach of the near-miss ids
PAD_ALIGN = 256         # pad bytes are a multiple of this: the view keeps the buffer's alignment
WS_GUARD = 4096         # guard bytes on each side of a workspace
WS_FILL = 0xA5
# Poison bytes for scratch that "may hold anything" (include/hhfm.h).  Two, so
# that a stale word is wrong whichever way the kernel compares it:
# 0xFF bytes: a 64-bit entry key above every real one (0xffff...), an fp32 /
#   bf16 NaN, int32 -1 (an id or offset below every range), and an arrival
#   counter that never reaches S (0xffffffff + S wraps far below it).
# 0x7F bytes: fp32 0x7f7f7f7f = +3.39e38, a finite score that beats every real
#   one where NaN would drop out of a max — the mirror of the 0x80 fill the
#   streaming path gives its threshold hints (-3.39e38) —, and a huge positive
#   key / index.
POISON_FF = 0xFF
POISON_7F = 0x7F
POISONS = (POISON_FF, POISON_7F)

# quiet NaN, as an integer of the element's width
_NAN_BITS = {torch.float32: (torch.int32, 0x7fc00000), torch.bfloat16: (torch.int16, 0x7fc0)}


def _pattern(dtype):
    if dtype == torch.uint8:
        return torch.uint8, WS_FILL
    return _NAN_BITS[dtype]


def pad_elems(t, pad_rows=PAD_ROWS):
    """Elements of one pad of ``guarded(t, pad_rows)``: at least ``pad_rows``
    rows (a row is ``t[0]``; an element for a vector), rounded up so that the
    pad's bytes are a multiple of 256."""
    row = t[0].numel() if t.dim() > 1 else 1
    nbytes = pad_rows * row * t.element_size()
    nbytes = (nbytes + PAD_ALIGN - 1) // PAD_ALIGN * PAD_ALIGN
    return nbytes // t.element_size()


def guarded(t, pad_rows=PAD_ROWS):
    """-> (view, buffer): ``view`` has ``t``'s contents, shape and dtype and
    lies inside the flat ``buffer`` between two quiet-NaN pads (fp32
    0x7fc00000, bf16 0x7fc0) of ``pad_elems(t, pad_rows)`` elements each."""
    t = t.contiguous()
    itype, bits = _NAN_BITS[t.dtype]
    pad, n = pad_elems(t, pad_rows), t.numel()
    buffer = torch.empty(pad + n + pad, dtype=t.dtype, device=t.device)
    buffer.view(itype).fill_(bits)
    view = buffer[pad:pad + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % PAD_ALIGN == buffer.data_ptr() % PAD_ALIGN
    return view, buffer


def guarded_workspace(nbytes, device, guard=WS_GUARD):
    """-> (view, buffer): a zero-filled uint8 workspace of exactly ``nbytes``
    (what the entry point is told) at ``buffer + guard``, with ``guard`` bytes
    of 0xA5 on each side."""
    assert guard % PAD_ALIGN == 0
    buffer = torch.full((guard + nbytes + guard,), WS_FILL, dtype=torch.uint8, device=device)
    view = buffer[guard:guard + nbytes]
    view.zero_()
    return view, buffer


def poisoned_workspace(nbytes, device, fill, zero_prefix=0, guard=WS_GUARD):
    """-> (view, buffer): ``guarded_workspace``'s layout (0xA5 guards on both
    sides of exactly ``nbytes``), the interior filled with the byte ``fill``
    except its first ``zero_prefix`` bytes, which are zero."""
    assert guard % PAD_ALIGN == 0 and 0 <= zero_prefix and 0 <= fill <= 0xFF
    buffer = torch.full((guard + nbytes + guard,), WS_FILL, dtype=torch.uint8, device=device)
    view = buffer[guard:guard + nbytes]
    view.fill_(fill)
    view[:min(zero_prefix, nbytes)].zero_()
    return view, buffer


def pads_untouched(buffer, view):
    """True when every element of ``buffer`` outside ``view`` still holds the
    fill pattern (compared as integers: NaN != NaN as floats)."""
    itype, bits = _pattern(buffer.dtype)
    off = (view.data_ptr() - buffer.data_ptr()) // buffer.element_size()
    n = view.numel()
    assert 0 < off and off + n < buffer.numel()
    raw = buffer.view(itype)
    return bool((raw[:off] == bits).all().item() and (raw[off + n:] == bits).all().item())


class Guards:
    """The (view, buffer) pairs of one test, checked together."""

    def __init__(self):
        self.pairs = []

    def table(self, t, pad_rows=PAD_ROWS):
        view, buffer = guarded(t, pad_rows)
        self.pairs.append((view, buffer))
        return view

    def workspace(self, nbytes, device):
        view, buffer = guarded_workspace(nbytes, device)
        self.pairs.append((view, buffer))
        return view

    def poisoned(self, nbytes, device, fill, zero_prefix=0):
        view, buffer = poisoned_workspace(nbytes, device, fill, zero_prefix)
        self.pairs.append((view, buffer))
        return view

    def assert_untouched(self):
        torch.cuda.synchronize()
        for n, (view, buffer) in enumerate(self.pairs):
            assert pads_untouched(buffer, view), f"guard pad {n} ({tuple(view.shape)}) was written"


def near_miss_ids(M, pad_rows=PAD_ROWS):
    """The bad ids of the tests: {−P … −1} ∪ {M … M + P − 1}."""
    return np.concatenate([np.arange(-pad_rows, 0), np.arange(M, M + pad_rows)]).astype(np.int32)


def plant(X, positions, M, rng, moved_id, pad_rows=PAD_ROWS):
    """The three batches of a bad-id case from in-range rows ``X``:
    -> (zeroed, bad, moved, rows) where ``positions`` [(row, column), ...]
    hold 0, a near-miss id and ``moved_id`` (an in-range id whose table row
    differs from row 0); ``rows`` are the distinct rows that hold one.  The
    near-miss ids cycle through the whole set, so both sides and both ends of
    the range are used."""
    ids = near_miss_ids(M, pad_rows)
    ids = ids[rng.permutation(len(ids))]
    zeroed, bad, moved = (np.array(X, dtype=np.int32, copy=True) for _ in range(3))
    for n, (r, c) in enumerate(positions):
        zeroed[r, c] = 0
        bad[r, c] = ids[n % len(ids)]
        moved[r, c] = moved_id
    assert ((bad >= -pad_rows) & (bad < M + pad_rows)).all()
    return zeroed, bad, moved, sorted({int(r) for r, _ in positions})
