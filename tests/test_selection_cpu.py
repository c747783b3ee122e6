"""The operand rules of ultra_amd/selection.py, off the GPU: what the live count and the retired operand take and refuse, with
the message of each caller -- the selections (predict.filtered_topk / _above / _rank) and query_exec.nonzero_lists."""
import pytest
import torch

from ultra_amd import selection
from ultra_amd.live import retired_words

CPU = torch.device("cpu")
LISTS = dict(lowest=0, exact=True, whose="matrix's")       # (how nonzero_lists asks)


def test_the_live_count_of_the_selections():
    n = 40
    for bad in (0, n + 1):
        with pytest.raises(ValueError, match=r"num_live must lie in \[1, 40\] \(the slots of a row\), got %d$" % bad):
            selection.live_operand(bad, n, CPU)
        with pytest.raises(ValueError, match=r"num_live must lie in \[1, 40\] \(the slots of a row\), got %d$" % bad):
            selection.live_int(bad, n)
    for ok in (1, n):
        got = selection.live_operand(ok, n, CPU)
        assert got.dtype == torch.long and got.numel() == 1 and int(got) == ok and selection.live_int(ok, n) == ok
    assert selection.live_int(torch.tensor([7]), n) == 7
    assert selection.live_operand(None, n, CPU) is None


def test_the_live_count_of_the_lists():
    n = 40
    for bad in (-1, n + 1, True):
        with pytest.raises(ValueError, match=r"num_live must lie in \[0, 40\] \(the slots of a row\), got %r$" % (bad,)):
            selection.live_operand(bad, n, CPU, **LISTS)
    for ok in (0, n):
        assert int(selection.live_operand(ok, n, CPU, **LISTS)) == ok
    with pytest.raises(ValueError):     # (an empty list is a list; an empty candidate set is none)
        selection.live_operand(0, n, CPU)


@pytest.mark.parametrize("kwargs, whose", [({}, "scores'"), (LISTS, "matrix's")])
def test_a_tensor_live_count_is_passed_through_unread(kwargs, whose):
    n = 40
    count = torch.tensor([n + 100])         # (beyond the row: the kernels clamp, the host does not look)
    assert selection.live_operand(count, n, CPU, **kwargs) is count
    for bad in (torch.tensor([3.0]), torch.tensor([3, 4]), torch.tensor([3], dtype=torch.int32), torch.tensor([3], device="meta")):
        with pytest.raises(ValueError, match="a tensor `num_live` is one int64 on the %s device" % whose):
            selection.live_operand(bad, n, CPU, **kwargs)


@pytest.mark.parametrize("n", [33, 64])
@pytest.mark.parametrize("bare", [False, True], ids=["pair", "bitmap"])
def test_the_retired_operand(n, bare):
    bits, count = retired_words([3, 32], n), torch.tensor([2])
    assert bits.dtype == torch.int32 and bits.numel() == 2 == (n + 31) // 32
    text = "bitmap on the matrix's device -- at least ceil" if bare else r"pair \(bits, count\) on the scores' device: at least ceil"
    for words in (bits, bits.view(torch.uint32)):
        got = selection.retired_operand((words, count), n, CPU, bare=bare)
        assert got[0] is words and got[1] is (None if bare else count)
    spread = torch.zeros(4, dtype=torch.int32)[::2]
    assert spread.numel() == 2 and not spread.is_contiguous()
    for bad in ((bits[:1], count), (spread, count), (bits.long(), count), (bits.to("meta"), count)):
        with pytest.raises(ValueError, match=text + r".* = 2 "):
            selection.retired_operand(bad, n, CPU, bare=bare)
    assert selection.retired_operand(None, n, CPU, bare=bare) is None
    if bare:        # the bitmap alone, and a pair's count is not looked at: the entry takes none
        for given in (bits, (bits, count.int())):
            got = selection.retired_operand(given, n, CPU, bare=True)
            assert got[0] is bits and got[1] is None
    else:
        for bad in ((bits, count.int()), (bits, torch.tensor([1, 1])), (bits, count.to("meta")), bits, (bits, 2)):
            with pytest.raises(ValueError, match=text):
                selection.retired_operand(bad, n, CPU)
