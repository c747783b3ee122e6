"""The reference of the relation-graph shape tests (tests/relgraph_cases.py) pinned without a GPU: against the torch
formulation tasks.build_relation_graph (itself pinned to the reference project's output in test_tasks.py), against the golden
relation graph, against itself on a filtered list, and its packed formats against their definitions and the host plan
builder.  And the conditions every case of the GPU file rests on."""
import os

import pytest
import torch

from tests import relgraph_cases as cases
from ultra_amd import tasks
from ultra_amd.data import Data


def torch_formulation(edge_index, edge_type, num_nodes, R):
    data = Data(edge_index=edge_index, edge_type=edge_type, num_nodes=num_nodes, num_relations=R)
    return tasks.build_relation_graph(data, node_chunk=128).relation_graph      # (several node chunks)


@pytest.mark.parametrize("R", [1, 31, 33, 2050])
def test_reference_equals_the_torch_formulation_on_wide_cases(R):
    case = cases.wide_case(R)
    ref = cases.cached_reference("wide", R)
    want = torch_formulation(case.edge_index, case.edge_type, case.num_nodes, R)
    assert torch.equal(ref.edge_index, want.edge_index) and torch.equal(ref.edge_type, want.edge_type)


def test_reference_equals_the_torch_formulation_on_a_cut_of_the_many_case():
    case = cases.many_case()
    at = torch.cat([torch.arange(2500), torch.arange(cases.MANY_EDGES - 2500, cases.MANY_EDGES)])      # (both kinds of edges)
    edge_index, edge_type = case.edge_index[:, at], case.edge_type[at]
    ref = cases.reference(edge_index, edge_type, case.num_nodes, case.num_relations)
    want = tasks.build_relation_graph(Data(edge_index=edge_index, edge_type=edge_type, num_nodes=case.num_nodes,
                                           num_relations=case.num_relations)).relation_graph
    assert ref.edge_index.shape[1] > 0
    assert torch.equal(ref.edge_index, want.edge_index) and torch.equal(ref.edge_type, want.edge_type)


def test_reference_equals_the_golden_relation_graph():
    # (read here, not through the helpers of the model tests: those need the built library, this file does not)
    g = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_ultra_3g_sum.pt"))
    ref = cases.reference(g["edge_index"], g["edge_type"], g["num_nodes"], g["num_relations"])
    assert ref.edge_index.shape[1] > 0
    assert torch.equal(ref.edge_index, g["rel_edge_index"]) and torch.equal(ref.edge_type, g["rel_edge_type"])


def keep_vector(num_edge, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([1.0, 0.5, 0.0, -0.0])[torch.randint(0, 4, (num_edge,), generator=g)]


@pytest.mark.parametrize("R", [33, 2050])
def test_reference_with_keep_equals_reference_of_the_filtered_list(R):
    case = cases.wide_case(R)
    keep = keep_vector(case.edge_index.shape[1], R)
    on = keep != 0
    assert 0 < int(on.sum()) < len(on) and bool((keep[~on].view(torch.int32) != 0).any())       # (a -0.0 among the dropped)
    got = cases.case_reference(case, keep)
    want = cases.reference(case.edge_index[:, on], case.edge_type[on], case.num_nodes, R)
    full = cases.cached_reference("wide", R)
    for name in ("adj", "counts", "hbits", "tbits", "edge_index", "edge_type"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.edge_index.shape[1] < full.edge_index.shape[1]


@pytest.mark.parametrize("R", [1, 31, 32, 33, 2050])
def test_packed_words_round_trip(R):
    g = torch.Generator().manual_seed(R)
    matrix = torch.rand(3, 5, R, generator=g) < 0.4
    matrix[0, 0], matrix[0, 1] = True, False
    words = cases.pack_bits(matrix)
    assert words.shape == (3, 5, (R + 31) // 32) and words.dtype == torch.int32
    assert torch.equal(cases.unpack_bits(words, R), matrix)
    # bit r & 31 of word r >> 5, spelled out; padding bits zero
    for r in {0, R // 2, R - 1}:
        assert torch.equal((words[..., r >> 5] >> (r & 31)) & 1, matrix[..., r].to(torch.int32))
    if R % 32:
        assert int((words[..., -1].to(torch.int64) & 0xffffffff).max()) < (1 << (R % 32))
    ref = cases.cached_reference("wide", R)
    rows = cases.unpack_bits(ref.adj, R)
    assert torch.equal(rows.sum(2).flatten(), ref.counts)
    assert torch.equal(rows.nonzero()[:, 1:].t(), ref.edge_index) and torch.equal(rows.nonzero()[:, 0], ref.edge_type)


@pytest.mark.parametrize("R", [16, 17, 100])
def test_byte_adjacency_equals_the_host_plan_builder(R):
    ref = cases.cached_reference("wide", R)
    try:
        from ultra_amd import _lib
    except (ImportError, OSError) as exc:
        pytest.skip("the library is not built: %s" % exc)
    from ultra_amd import rspmm
    dense = rspmm.Plan(ref.edge_index, ref.edge_type, R, 4, exact_order=True, dense=True).dense
    assert dense is not None
    want = dense.export(_lib.ARR_DENSE_ORDER)
    got = ref.dense
    assert got.dtype == torch.uint8 and got.shape == want.shape == (((R + 15) // 16) ** 2 * 1024,)
    assert int(got.sum()) == ref.edge_index.shape[1] and torch.equal(got, want)


@pytest.mark.parametrize("R", cases.WIDE_RELATIONS + (16, 17, 48, 100, 1025))
def test_conditions_hold_for_the_wide_cases(R):
    case = cases.wide_case(R)
    assert case.num_nodes == 300 and int(case.edge_index.max()) < 280 and int(case.edge_type.max()) == R - 1
    assert torch.equal(case.edge_index[:, -50:], case.edge_index[:, :50]) and torch.equal(case.edge_type[-50:], case.edge_type[:50])
    first = cases.wide_split(case)
    assert set(case.edge_index[0, first:-50].tolist()) == ({0, 2, 4} if R > 3 else {0, 4})      # (entity 2 starts at relation 3)
    assert cases.conditions(case, cases.cached_reference("wide", R))


def test_conditions_hold_for_the_many_case():
    case = cases.many_case()
    assert (case.num_relations, case.num_nodes, case.edge_index.shape[1]) == (40, 40000, 1200000)
    assert cases.conditions(case, cases.cached_reference("many"))
