"""Serving logical queries on a growing graph, the parts that need no GPU: the ultra_nonzero_lists_live symbol and
its argument checks, which answer before any GPU call; QueryPredictor(entity_capacity=) / add_entities / materialized / compact on
stub projections whose output for an entity depends on that entity and its edges alone, so every comparison with a fresh
predictor on the materialised graph is exact.

The queries are the golden file's 28 (two of each of the 14 types) with their ids folded into the 12-node fixture, plus three that
END in a negation.  In every one of the 14 types a negated branch is intersected with a positive one, so a reserved slot's
symbolic 1 - 0 = 1 meets a 0 and the final set is 0 there; only a query whose last operation is a negation (or a union with a
negated branch) leaves 1.0 in the reserved slots of the FINAL set -- those are the queries that list dead ids when the lists are
not cut at the live count."""
import os

import pytest
import torch
from torch import nn

from tests.test_query_exec_cpu import load, plain
from tests.test_query_live_cpu import N, R, same, twelve_node_graph
from ultra_amd import _lib, query_exec, query_predict
from ultra_amd.ultraquery import Query, UltraQuery, symbolic_traversal_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ultra_nonzero_lists_live"
K = 24          # more than any slot count of this file: count = live candidates


class ExactStub(nn.Module):
    """tests.test_query_live_cpu.EdgeListStub with a neural side made of multiplications, additions, floor and clamp only: each
    is rounded per element whatever the row length, so an entity's value has the same bits on the padded and on the materialised
    graph (torch's CPU sigmoid takes a vector path or a scalar one by an element's position in its row, one ulp apart).  The
    output for an entity depends on that entity's id, its own input and the edges into it."""

    def __init__(self, symbolic):
        super(ExactStub, self).__init__()
        self.symbolic = symbolic

    def forward(self, graph, h_prob, r_index):
        r_index = r_index.as_subclass(torch.Tensor)
        out = symbolic_traversal_reference(graph.edge_index, graph.edge_type, graph.num_nodes, h_prob, r_index)
        if self.symbolic:
            return out
        wave = torch.arange(h_prob.shape[1], dtype=torch.float32) * 0.37 + r_index.float().unsqueeze(1) * 0.11
        return (out * 0.5 + (wave - wave.floor()) * 0.3 + h_prob * 0.125 + 0.03125).clamp(0.015625, 0.984375)


def edge_list_model(logic="product"):
    uq = UltraQuery(nn.Module(), logic=logic)
    uq.model, uq.symbolic_model = ExactStub(False), ExactStub(True)
    return uq.eval()


def folded_queries():
    """(31, L) postfix rows: the golden queries with entity ids modulo 12 and relation ids modulo 4, then (0, (0, -2)),
    (5, (1, -2)) and the union of (2, (0,)) with (9, (1, -2))."""
    g = load()
    q = plain(g["query"]).clone()
    assert len(set(g["type"].tolist())) == 14
    flags = q & Query.operation
    q[flags == 0] %= N
    is_p = flags == Query.projection
    q[is_p] = Query.projection | ((q[is_p] & ~Query.operation) % R)
    P, NOT, S, U = Query.projection, Query.negation, Query.stop, Query.union | 2
    more = [[0, P | 0, NOT], [5, P | 1, NOT], [2, P | 0, 9, P | 1, NOT, U]]
    width = q.shape[1]
    return torch.cat([q, torch.tensor([row + [S] * (width - len(row)) for row in more])])


def ends_in_negation(queries):
    return list(range(len(queries) - 3, len(queries)))


def entailed_counts(graph, queries, batches, logic="product"):
    """Per query the size of its final symbolic set on `graph`, from the compiled program in plain torch."""
    out = torch.zeros(len(queries), dtype=torch.long)
    model = edge_list_model(logic)
    for index in batches:
        _, sym = query_exec.execute(model, graph, queries[index])
        out[index] = (sym != 0).sum(dim=-1)
    return out


def check_against_fresh(qp, queries):
    """answers / answer_sets of the growing predictor against a fresh one without a reserve on qp.materialized(), exactly; no id
    at or beyond num_entities; count = num_entities - entailed for every query, those that end in a negation included."""
    mat = qp.materialized()
    live = qp.num_entities
    assert int(mat.num_nodes) == live and mat is not qp.materialized()
    fresh = query_predict.QueryPredictor(edge_list_model(qp.model.logic), mat, k=qp.k, batch_size=qp.batch_size)
    assert fresh.graph is mat and fresh.live_count is None
    got = qp.answers(queries), qp.answer_sets(queries, probability=0.45)
    want = fresh.answers(queries), fresh.answer_sets(queries, probability=0.45)
    assert qp.batches(queries) == fresh.batches(queries)
    assert same(got[0], want[0])
    assert same(got[1], want[1])
    ids, _, count = got[0]
    assert int(ids.max()) < live and int(got[1][1].max()) < live
    entailed = entailed_counts(mat, queries, fresh.batches(queries), qp.model.logic)
    assert torch.equal(count, live - entailed)
    assert bool((ids >= 0).sum(dim=-1).eq(count).all())
    for i in ends_in_negation(queries):
        assert int(entailed[i]) > live // 2, "a query that ends in a negation entails most entities"
    return got


def test_the_symbol_is_exported_and_declared():
    assert hasattr(_lib.lib, ENTRY)
    with open(os.path.join(ROOT, "include", "ultra_nbfnet.h")) as f:
        header = f.read()
    assert "int32_t ultra_nonzero_lists_live(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out," in header
    assert _lib.lib.ultra_abi_version() == 7


def test_the_entry_validates_before_any_gpu_call():
    """On host tensors: a NULL n_live is ULTRA_ERR_INVALID; the other argument errors are ultra_nonzero_lists' own, under the
    twin's name.  Nothing is launched."""
    lib = _lib.lib
    x = torch.zeros(2, 8)
    counts, ptr, index = (torch.ones(n, dtype=torch.int64) for n in (2, 3, 16))
    live = torch.tensor([8], dtype=torch.int64)
    default = dict(x=x.data_ptr(), batch=2, n=8, counts=counts.data_ptr(), ptr=ptr.data_ptr(), index=index.data_ptr(),
                   capacity=16, live=live.data_ptr())

    def call(entry=ENTRY, **change):
        a = dict(default, **change)
        args = (a["x"], a["batch"], a["n"], a["counts"], a["ptr"], a["index"], a["capacity"])
        if entry == ENTRY:
            args += (a["live"],)
        return getattr(lib, entry)(*(args + (None,)))

    assert call(live=None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_nonzero_lists_live: n_live is NULL" in lib.ultra_last_error()
    for change in (dict(x=None), dict(counts=None), dict(ptr=None), dict(index=None), dict(batch=-1), dict(n=-1),
                   dict(capacity=15), dict(n=2 ** 31), dict(batch=2 ** 31, capacity=2 ** 62)):
        parent = call("ultra_nonzero_lists", **change)
        assert parent in (_lib.ULTRA_ERR_INVALID, _lib.ULTRA_ERR_UNSUPPORTED), change
        parent_message = lib.ultra_last_error()
        assert call(**change) == parent, change
        assert lib.ultra_last_error() == parent_message.replace(b"ultra_nonzero_lists:", b"ultra_nonzero_lists_live:"), change
    assert call(n=2 ** 31) == _lib.ULTRA_ERR_UNSUPPORTED and call(n=2 ** 31, live=None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert torch.equal(ptr, torch.ones(3, dtype=torch.int64)) and torch.equal(index, torch.ones(16, dtype=torch.int64))


def test_nonzero_lists_num_live_argument_rules():
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError):
        query_exec.nonzero_lists(x, num_live=4)         # (no CPU path, with or without a live count)
    # the anchors of a compiled program are the ids below num_live
    row = torch.tensor([[7, Query.projection | 1, Query.stop]])
    assert query_exec.compile(row, 10, 4).num_nodes == 10
    assert query_exec.compile(row, 10, 4, num_live=8).num_nodes == 10
    with pytest.raises(ValueError, match=r"outside \[0, 7\)"):
        query_exec.compile(row, 10, 4, num_live=7)
    with pytest.raises(ValueError):
        query_exec.compile(row, 10, 4, num_live=11)


def test_without_a_reserve_nothing_changes():
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=5)
    assert qp.graph is graph and qp.live_count is None and qp.entity_capacity == 0
    assert qp.num_entities == N and qp.num_slots == N and qp.materialized() is graph
    with pytest.raises(ValueError):
        qp.add_entities()
    assert qp.graph is graph and qp.delta is None
    for bad in (-1, 2.5, True, "4"):
        with pytest.raises(ValueError):
            query_predict.QueryPredictor(edge_list_model(), graph, entity_capacity=bad)


def test_a_reserve_of_four():
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=K, batch_size=4, entity_capacity=4)
    assert qp.graph is not graph and qp.graph.edge_index is graph.edge_index and qp.graph.edge_type is graph.edge_type
    assert (qp.num_entities, qp.num_slots, int(graph.num_nodes)) == (N, N + 4, N)
    rel, want = qp.graph.relation_graph, graph.relation_graph
    assert rel is not want and int(rel.num_nodes) == int(want.num_nodes)
    assert torch.equal(rel.edge_index, want.edge_index) and torch.equal(rel.edge_type, want.edge_type)
    scalar = qp.live_count
    assert scalar.dtype == torch.long and scalar.numel() == 1 and int(scalar) == N
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            qp.add_entities(bad)
    assert qp.add_entities(2).tolist() == [12, 13]
    assert qp.live_count is scalar and int(scalar) == 14 and qp.num_entities == 14 and qp.num_slots == N + 4
    assert qp.delta is None and int(qp.materialized().num_nodes) == 14
    for call in (qp.add_facts, qp.remove_facts):
        for dead in (14, 15):
            with pytest.raises(ValueError):
                call(0, 0, dead)
            with pytest.raises(ValueError):
                call(dead, 1, 3)
    for dead in (14, 15, 16):
        with pytest.raises(ValueError, match=r"\[0, 14\)"):
            qp.answers([(dead, (0,))])
        with pytest.raises(ValueError, match=r"\[0, 14\)"):
            qp.answer_sets([((1, (0,)), (dead, (1, -2)))])
    assert qp.delta is None
    assert qp.add_facts([12, 3], [0, 1], [13, 12]) == 2 and qp.delta.num_live == 14
    assert qp.remove_facts(12, 0, 13).tolist() == [1]
    ids, _, count = qp.answers([(12, (0,)), (13, (1,))])
    assert ids.shape == (2, K) and int(ids.max()) < 14
    # one more entity while a delta is held: its bound follows
    assert qp.add_entities().tolist() == [14] and qp.delta.num_live == 15 and int(scalar) == 15
    assert qp.add_facts(14, 0, 0) == 2


@pytest.mark.parametrize("logic", ["product", "godel"])
def test_answers_equal_a_fresh_predictor(logic):
    graph = twelve_node_graph()
    queries = folded_queries()
    qp = query_predict.QueryPredictor(edge_list_model(logic), graph, k=K, batch_size=4, entity_capacity=4)
    # an unused reserve, the negation types included: what a plain predictor on the graph itself answers
    unused = check_against_fresh(qp, queries)
    plain_qp = query_predict.QueryPredictor(edge_list_model(logic), graph, k=K, batch_size=4)
    assert same(unused[0], plain_qp.answers(queries)) and same(unused[1], plain_qp.answer_sets(queries, probability=0.45))
    # two entities, a fact old -> new and a fact new -> new
    new = qp.add_entities(2).tolist()
    check_against_fresh(qp, queries)                    # (entities without facts: isolated candidates)
    assert qp.add_facts([2, new[0]], [0, 1], [new[0], new[1]]) == 2
    asked = torch.cat([queries, torch.tensor([[new[0], Query.projection | 1, Query.stop] + [Query.stop] * (queries.shape[1] - 3),
                                              [2, Query.projection | 0, Query.projection | 1] + [Query.stop] * (queries.shape[1] - 3),
                                              [new[1], Query.projection | 3, Query.negation] + [Query.stop] * (queries.shape[1] - 3)])])
    asked = torch.cat([asked[:-6], asked[-3:], asked[-6:-3]])      # (the three that end in a negation stay last)
    got = check_against_fresh(qp, asked)
    ids, _, count = got[0]
    first = len(queries) - 3
    assert new[1] not in ids[first, :int(count[first])].tolist(), "the stated tail of (new, 1, ?) is entailed"
    assert new[1] not in ids[first + 1, :int(count[first + 1])].tolist(), "... and so is the end of the 2p path through it"
    # a retraction
    assert qp.remove_facts([0, new[0]], [0, 1], [1, new[1]]).tolist() == [3, 1]
    got = check_against_fresh(qp, asked)
    ids, _, count = got[0]
    assert new[1] in ids[first, :int(count[first])].tolist()
    # compact keeps the slots and the live count
    qp.compact()
    assert qp.delta is None and (qp.num_entities, qp.num_slots) == (14, 16)
    check_against_fresh(qp, asked)


def test_beyond_the_reserve_one_rebuild():
    graph = twelve_node_graph()
    queries = folded_queries()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=K, batch_size=4, entity_capacity=4)
    qp.add_facts(8, 1, 3)
    compactions = []
    compact = qp.compact
    qp.compact = lambda *args, **kwargs: (compactions.append(kwargs), compact(*args, **kwargs))[1]
    scalar = qp.live_count
    assert qp.add_entities(5).tolist() == [12, 13, 14, 15, 16]
    assert compactions == [{"slots": 21}]
    assert (qp.num_entities, qp.num_slots, int(scalar)) == (17, 21, 17) and qp.live_count is scalar and qp.delta is None
    assert qp.graph.edge_index.shape[1] == graph.edge_index.shape[1] + 2       # the held fact was folded in
    assert int(qp.graph.relation_graph.num_nodes) == R
    assert qp.add_facts(16, 0, 12) == 1
    check_against_fresh(qp, queries)
    assert qp.add_entities(4).tolist() == [17, 18, 19, 20] and len(compactions) == 1
    check_against_fresh(qp, queries)
