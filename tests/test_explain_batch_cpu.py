"""Batched path explanations on the CPU: explain.topk_average_length_batch against explain.topk_average_length on every
sample's own slices, over the restated beam search (tests/test_explain_cpu.py) on the golden `beam` cases, and the new C
entry points in the library's export table."""
import ctypes

import pytest
import torch

from tests.test_explain_cpu import load, restate_chain
from ultra_amd import explain


def _tails(case, num_sample):
    """The case's own tail first, then other nodes: one that some edge enters and one that none does where there is one."""
    ei, n = case["edge_index"], case["num_nodes"]
    deg = torch.bincount(ei[1], minlength=n)
    others = [int(v) for v in torch.argsort(deg, descending=True, stable=True) if int(v) != case["t"]]
    picks = [case["t"], others[0], others[-1]]
    return [picks[s % 3] for s in range(num_sample)]


def _stacked(case, tails, k):
    chains = [restate_chain(case["edge_index"], case["edge_type"], case["num_nodes"], case["edge_grads"], case["h"], t, k)
              for t in tails]
    distances = [torch.stack([c[0][i] for c in chains]) for i in range(len(case["edge_grads"]))]
    back_edges = [torch.stack([c[1][i] for c in chains]) for i in range(len(case["edge_grads"]))]
    return chains, distances, back_edges


CASES = [c["name"] for c in load()["beam"]]


@pytest.mark.parametrize("num_sample", (1, 3))
@pytest.mark.parametrize("name", CASES)
def test_topk_average_length_batch_matches_per_sample(name, num_sample):
    case = next(c for c in load()["beam"] if c["name"] == name)
    k = case["num_beam"]
    tails = _tails(case, num_sample)
    chains, distances, back_edges = _stacked(case, tails, k)
    got = explain.topk_average_length_batch(distances, back_edges, torch.tensor(tails), k)
    assert len(got) == num_sample
    for s, t in enumerate(tails):
        want = explain.topk_average_length(chains[s][0], chains[s][1], torch.tensor([t]), k)
        assert [list(p) for p in got[s][0]] == [list(p) for p in want[0]], (name, s)
        assert list(got[s][1]) == list(want[1]), (name, s)


def test_topk_average_length_batch_takes_a_smaller_k_than_the_beam():
    case = next(c for c in load()["beam"] if c["name"] == "close_k10")
    tails = _tails(case, 3)
    chains, distances, back_edges = _stacked(case, tails, case["num_beam"])
    got = explain.topk_average_length_batch(distances, back_edges, tails, 4)
    for s, t in enumerate(tails):
        want = explain.topk_average_length(chains[s][0], chains[s][1], t, 4)
        assert (list(got[s][0]), list(got[s][1])) == (list(want[0]), list(want[1]))


def test_empty_and_all_inf_layers_in_a_batch():
    """tests/test_explain_cpu.py::test_empty_and_all_inf_layers as a batch: a sample whose layers are all -inf beside one that
    reaches its tail, and the empty batch."""
    ei = torch.tensor([[0, 1], [1, 2]])
    et = torch.tensor([0, 1])
    grads = [torch.tensor([1.0, 2.0])] * 2
    chains = [restate_chain(ei, et, 3, grads, h, 2, 2) for h in (2, 0)]       # head 2 has no out-edges: all -inf
    assert all(torch.isinf(d).all() and not b.any() for d, b in zip(*chains[0]))
    distances = [torch.stack([c[0][i] for c in chains]) for i in range(2)]
    back_edges = [torch.stack([c[1][i] for c in chains]) for i in range(2)]
    got = explain.topk_average_length_batch(distances, back_edges, [2, 2], 2)
    assert (list(got[0][0]), list(got[0][1])) == ([], [])
    want = explain.topk_average_length(chains[1][0], chains[1][1], 2, 2)
    assert [list(p) for p in got[1][0]] == [list(p) for p in want[0]] == [[(0, 1, 0), (1, 2, 1)]]
    assert list(got[1][1]) == list(want[1]) == [1.5]
    assert explain.topk_average_length_batch([d[:0] for d in distances], [b[:0] for b in back_edges], [], 2) == []
    assert explain.topk_average_length_batch([], [], [1, 2], 2) == [([], []), ([], [])]


def test_topk_average_length_batch_rejects_mismatched_tails():
    d = [torch.full((2, 3, 2), float("-inf"))]
    b = [torch.zeros(2, 3, 2, 4, dtype=torch.long)]
    with pytest.raises(ValueError):
        explain.topk_average_length_batch(d, b, [0], 2)
    with pytest.raises(ValueError):
        explain.topk_average_length_batch(d, b, [0, 3], 2)


def test_new_entry_points_are_declared_and_exported():
    from tests.test_abi import declared_symbols
    from ultra_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_symbols()
    for name in ("ultra_rspmm_edge_grad_samples", "ultra_beam_search_layer_batch"):
        assert name in names and hasattr(lib, name)
    # argument checks that run before anything touches the device
    assert _lib.lib.ultra_beam_search_layer_batch(None, None, None, None, None, 0, 3, 0, 2, None, None, None, 65, None, None,
                                                  None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert b"num_beam" in _lib.lib.ultra_last_error()
    assert _lib.lib.ultra_beam_search_layer_batch(None, None, None, None, None, 0, 3, 0, 70000, None, None, None, 4, None,
                                                  None, None) == _lib.ULTRA_ERR_INVALID
    assert b"num_sample" in _lib.lib.ultra_last_error()
    assert _lib.lib.ultra_beam_search_layer_batch(None, None, None, None, None, 0, 3, 0, 0, None, None, None, 4, None, None,
                                                  None) == _lib.ULTRA_OK
