"""The optional operands of "select from a row of n slots", and the one launch that takes them.

Every selection entry (ultra_filtered_topk / _above / _rank, ultra_nonzero_lists) comes in three forms: the parent, over all n
slots; its `_live` twin, over the slots below a live count; its `_alive` twin, over the slots below a live count (or NULL: all of
them) that a bitmap does not name.  The checks of the two operands and the choice among the three forms are here and nowhere
else: the wrappers in predict and query_exec, the captured steps and the eager loops all come through this module.

A GROWING graph: a predictor with entity_capacity=M serves rows of N + M slots; the selection then runs over
the LIVE ids -- `num_live`.  The selections take a count in [1, n]; ultra_nonzero_lists, whose lists may be empty, one in [0, n].
CANDIDATE lists: `among` -- per row an allow list, the dual of the known lists -- takes each selection to its
`_among` entry, of which there is one: the live count and the retired pair are its nullable operands.
RETIRED entities: their ids are taken out of the candidate set for good -- `retired`: for the kernels one
device bitmap (live.retired_words: id v is bit v & 31 of word v >> 5) and one device int64, both read at replay; for the
restatements the sorted id vector.  Neither operand is looked at on the host once it is a device tensor: the kernels clamp.
"""
import torch

from . import _lib


def live_int(num_live, n, lowest=1, exact=False):
    """`num_live` (an int, or a one-element integer tensor) as an int in [lowest, n] (ValueError otherwise).  exact
    (nonzero_lists): a bool is no count, and the message quotes the value as it was given."""
    live = int(num_live)
    if (exact and isinstance(num_live, bool)) or not lowest <= live <= n:
        raise ValueError("num_live must lie in [%d, %d] (the slots of a row), got %s"
                         % (lowest, n, repr(num_live) if exact else live))
    return live


def live_operand(num_live, n, dev, lowest=1, exact=False, whose="scores'"):
    """`num_live` as the device int64 the _live and _alive entries read: a one-element int64 tensor on `dev` is passed as it is
    (its value is not looked at on the host -- the kernels clamp it), an int is checked (live_int) and uploaded.  whose: the
    tensor `dev` belongs to, for the message.  None stays None: no live count."""
    if num_live is None:
        return None
    if torch.is_tensor(num_live):
        if num_live.numel() != 1 or num_live.dtype != torch.long or num_live.device != dev:
            raise ValueError("a tensor `num_live` is one int64 on the %s device" % whose)
        return num_live
    return torch.tensor(live_int(num_live, n, lowest, exact), dtype=torch.long, device=dev)


def retired_operand(retired, n, dev, bare=False):
    """`retired` of the kernels' wrappers as (bits, count), neither looked at on the host: the pair on `dev` -- bits at least
    ceil(n / 32) contiguous 32-bit words (int32 or uint32: live.retired_words), count one int64.  bare (nonzero_lists, whose
    entry takes no count): the bitmap alone is taken too, as (bits, None), and of a pair only the bitmap is used.  None stays
    None: nothing retired."""
    if retired is None:
        return None
    words = (n + 31) // 32
    try:
        bits, count = retired if not bare or (isinstance(retired, (tuple, list)) and len(retired) == 2) else (retired, None)
        ok = (torch.is_tensor(bits) and bits.dim() == 1 and bits.is_contiguous() and bits.dtype in (torch.int32, torch.uint32)
              and bits.numel() >= words and bits.device == dev)
        if ok and not bare:
            ok = torch.is_tensor(count) and count.numel() == 1 and count.dtype == torch.long and count.device == dev
    except (TypeError, ValueError):
        ok = False
    if ok:
        return bits, None if bare else count
    if bare:
        raise ValueError("`retired` is the bitmap on the matrix's device -- at least ceil(n / 32) = %d int32 or uint32 words -- "
                         "or the pair (bits, count) that holds it" % words)
    raise ValueError("`retired` is the pair (bits, count) on the scores' device: at least ceil(N / 32) = %d 32-bit words "
                     "and one int64 (the sorted id vector is the _reference functions' form)" % words)


def among_operand(among, batch, n, dev, capacity=None):
    """`among` of the kernels' wrappers -- the pair (span (batch, 2) int64, index int64), contiguous, on `dev`: row b's candidates
    are index[span[b, 0] : span[b, 1]], ids ascending and distinct within a span -- checked once, as the triple
    (span, index, capacity) that `launch` takes.  capacity (a host int, at least the longest span the call may meet; a captured
    caller passes it): None reads the longest span from the device, one host read.  None stays None: no candidate lists.  n: the
    slots of a row (the ids' range; they are not looked at on the host -- the kernels skip an id that is not eligible)."""
    if among is None:
        return None
    try:
        span, index = among
        ok = (torch.is_tensor(span) and torch.is_tensor(index) and span.shape == (batch, 2) and index.dim() == 1
              and span.dtype == torch.long and index.dtype == torch.long and span.device == dev and index.device == dev
              and span.is_contiguous() and index.is_contiguous())
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("`among` is the pair (span, index) on the scores' device: contiguous int64 tensors, span of shape "
                         "(batch, 2) = (%d, 2) and index 1-D (a list of per-row id vectors is the _reference functions' form)" % batch)
    if capacity is None:
        capacity = int((span[:, 1] - span[:, 0]).max()) if batch else 1
    elif isinstance(capacity, bool) or not isinstance(capacity, int):
        raise ValueError("among_capacity is an int, got %r" % (capacity,))
    return span, index, max(1, min(int(capacity), (1 << 31) - 1))


def launch(entry, args, n_live, dev, retired=None, among=None, among_at=3):
    """One launch of a selection entry on `dev`'s stream: `entry` without operands; its `_live` twin with the device scalar
    `n_live` appended to the same arguments; with `retired` = (bits, count) its `_alive` twin with the live count (or NULL: every
    slot), the bitmap and -- where the caller gives one: ultra_nonzero_lists_alive takes none -- the count appended.  The entry
    is looked up when it is called (the call-count tests wrap the attributes of _lib.lib).
    among (among_operand's triple, or None: everything above, unchanged): the `_among` entry -- ONE entry per selection, the
    live count, the bitmap and the retired count its nullable operands.  `args` are the parent's; among_at: the position of
    `batch` in them, where the known lists end -- (span, index) go in front of it and the capacity behind n, which follows it."""
    stream = _lib.stream_of(dev)
    if among is not None:
        span, index, capacity = among
        bits, count = (None, None) if retired is None else retired
        args = args[:among_at] + (span.data_ptr(), index.data_ptr()) + args[among_at:among_at + 2] + (capacity,) + args[among_at + 2:]
        _lib.check(getattr(_lib.lib, entry + "_among")(*args, _lib.ptr(n_live), _lib.ptr(bits), _lib.ptr(count), stream))
        return
    if retired is not None:
        bits, count = retired
        operands = (bits.data_ptr(),) if count is None else (bits.data_ptr(), count.data_ptr())
        _lib.check(getattr(_lib.lib, entry + "_alive")(*args, None if n_live is None else n_live.data_ptr(), *operands, stream))
    elif n_live is None:
        _lib.check(getattr(_lib.lib, entry)(*args, stream))
    else:
        _lib.check(getattr(_lib.lib, entry + "_live")(*args, n_live.data_ptr(), stream))
