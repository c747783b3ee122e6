"""Serving logical queries on a changing graph, on the GPU: ultra_symbolic_traversal_edit_rows against the
traversal's torch restatement on the materialised edge list (hub segment, edge-less rows and relation, every kind of edit), its
replay from a captured graph after further edits, the two projections with `delta=` against themselves on the materialised graph,
and QueryPredictor.add_facts / remove_facts / compact end to end against a fresh predictor on `materialized()`."""
import ctypes

import pytest
import torch

from tests.test_grow_gpu import counted
from tests.test_query_exec_cpu import load
from tests.test_query_exec_gpu import _eager_answers, _same_answers
from tests.test_ultraquery_gpu import build_model, golden_graph
from ultra_amd import _lib, query_predict, rspmm, tasks
from ultra_amd.data import Data
from ultra_amd.ultraquery import Query, symbolic_traversal, symbolic_traversal_reference

pytestmark = pytest.mark.gpu

N, R = 40, 4
ENTRY = "ultra_symbolic_traversal_edit_rows"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def hub_graph(dev):
    """40 nodes, 4 relations (0, 1 direct; 2, 3 their inverses).  Node 0 receives 150 in-edges of relation 2 from the other 39
    nodes -- three or four parallel edges per source: a segment of three 64-lane trips.  The rest is sparse: a chain of relation 0
    (3 -> 4 three times), fifteen edges of relation 1 with distinct tails, two more edges of relation 2 into node 7; relation 3
    has no edge, nodes 26..39 have no in-edge, and most facts are stated in one direction only."""
    hub = torch.stack([torch.arange(150) % 39 + 1, torch.zeros(150, dtype=torch.long)])
    i = torch.arange(1, 21)
    chain = torch.stack([i, i + 1])
    j = torch.arange(1, 16)
    one = torch.stack([j, (3 * j) % 25 + 1])
    more = torch.tensor([[3, 3, 5, 6], [4, 4, 7, 7]])
    index = torch.cat([hub, chain, one, more], dim=1)
    kind = torch.cat([torch.full((150,), 2), torch.zeros(20, dtype=torch.long), torch.ones(15, dtype=torch.long),
                      torch.tensor([0, 0, 2, 2])])
    assert int(torch.bincount(index[1], minlength=N)[26:].sum()) == 0 and not bool((kind == 3).any())
    return Data(edge_index=index.to(dev), edge_type=kind.to(dev), num_nodes=N, num_relations=R)


def fuzzy_sets(batch, dtype, dev):
    gen = torch.Generator().manual_seed(7 + batch)
    h = torch.rand(batch, N, generator=gen).to(dtype)
    h[:, 5::11] = -0.5                                  # a few negative entries: the clamp at 0
    h[:, 17] = 2.0                                      # the hub row's maximum comes from source 17
    r = torch.tensor([2, 0, 2, 3, 1][:batch])           # two samples share relation 2; one asks for the edge-less relation 3
    return h.to(dev), r.to(dev)


def apply_edits(delta):
    delta.add([30, 0, 7, 20], [0, 0, 0, 1], [31, 33, 9, 22])
    # 30 -> 31 (0) and 31 -> 30 (2): into edge-less rows; 33 -> 0 (2): into the hub; 9 -> 7 (2): row 7, which also loses an edge;
    # 20 -> 22 (1) and 22 -> 20 (3): the first edge of the edge-less relation
    removed = delta.remove([0, 1, 3, 7, 3], [0, 1, 1, 0, 0], [17, 4, 10, 5, 4])
    # (17 -> 0, 2): the hub's maximum, four parallel edges under one key; (1 -> 4, 1) and (3 -> 10, 1): the last edge of relation 1
    # in rows 4 and 10 -- row 10 is touched by removals only; (5 -> 7, 2): row 7 holds both kinds; (3 -> 4, 0): three duplicates
    assert removed.tolist() == [0, 1, 1, 0, 3]          # (direct edges: the hub's and row 7's keys are inverse edges)
    delta.add(3, 0, 4)                                  # removed and stated again: one new edge, the tombstone stays
    return [0, 3, 4, 7, 9, 10, 20, 22, 30, 31, 33]      # the tails an added or a removed edge points into


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_edit_rows_equal_the_traversal_of_the_materialised_graph(dev, dtype, batch):
    data = hub_graph(dev)
    ei, et = data.edge_index, data.edge_type
    segment = int(((ei[1] == 0) & (et == 2)).sum())
    assert segment == 150 > 2 * 64                      # longer than TRAVERSAL_LANE_MAX: three 64-lane trips
    h, r = fuzzy_sets(batch, dtype, dev)
    before = symbolic_traversal(ei, et, N, h, r)
    delta = rspmm.GraphDelta(data, capacity=16)
    assert torch.equal(symbolic_traversal(ei, et, N, h, r, delta=delta), before)      # an empty delta: the base launch alone
    touched = apply_edits(delta)
    mat = delta.materialize()
    want = symbolic_traversal_reference(mat.edge_index, mat.edge_type, N, h, r)
    got = symbolic_traversal(ei, et, N, h, r, delta=delta)
    assert got.dtype == dtype and torch.equal(got, want)
    lay = delta.traversal
    assert lay.rows[:int(lay.count)].tolist() == touched
    # the untouched rows keep the bits the base launch gave them; the hub row dropped (its maximum's source is dead)
    untouched = torch.ones(N, dtype=torch.bool, device=dev)
    untouched[touched] = False
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(got[:, untouched].contiguous().view(bits), before[:, untouched].contiguous().view(bits))
    assert float(before[0, 0]) == 2.0 and 0.0 < float(got[0, 0]) < 2.0
    assert float(before[-1, 4 if batch == 5 else 0]) > 0
    if batch == 5:
        assert float(got[4, 4]) == 0.0 and float(got[4, 10]) == 0.0 and float(before[4, 10]) > 0      # relation 1: last edge gone
        assert float(before[3].abs().sum()) == 0.0 and float(got[3, 20]) == float(h[3, 22]) > 0     # relation 3: its first edge
    # whatever lies beyond the live parts of the buffers is never read: out-of-range ids there change nothing
    count, m, k = int(lay.count), 2 * len(delta), delta.num_removed
    far = 1 << 30
    lay.rows[count:] = far
    lay.add_ptr[count + 1:] = far
    lay.dead_ptr[count + 1:] = far
    lay.add_src[m:] = far
    lay.add_type[m:] = far
    lay.dead_src[k:] = far
    lay.dead_type[k:] = far
    assert torch.equal(symbolic_traversal(ei, et, N, h, r, delta=delta), want)


def test_a_null_dead_array_means_no_tombstones(dev):
    from ultra_amd.ultraquery import traversal_csr
    data = hub_graph(dev)
    ei, et = data.edge_index, data.edge_type
    h, r = fuzzy_sets(5, torch.float32, dev)
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add([30, 0], [0, 0], [31, 33])
    mat = delta.materialize()
    want = symbolic_traversal_reference(mat.edge_index, mat.edge_type, N, h, r)
    t = symbolic_traversal(ei, et, N, h, r)
    edits = delta.traversal_operand()
    edits.dead_ptr_dev = edits.dead_src_dev = edits.dead_type_dev = None
    csr = traversal_csr(ei, et, N)
    rc = _lib.lib.ultra_symbolic_traversal_edit_rows(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), N,
                                                     ctypes.byref(edits), r.data_ptr(), 5, _lib.F32, h.data_ptr(), t.data_ptr(),
                                                     _lib.stream_of(h))
    assert rc == _lib.ULTRA_OK and torch.equal(t, want)


def test_a_captured_launch_follows_the_buffers(dev):
    data = hub_graph(dev)
    ei, et = data.edge_index, data.edge_type
    h, r = fuzzy_sets(5, torch.float32, dev)
    delta = rspmm.GraphDelta(data, capacity=16)
    delta.add(30, 0, 31)
    out = []

    def step():
        out[:] = [symbolic_traversal(ei, et, N, h, r, delta=delta)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # (the CSR and the layout exist from here on)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    pinned = [t.data_ptr() for t in delta.traversal]
    apply_edits(delta)                                  # more facts and the first tombstones, into the same buffers
    assert [t.data_ptr() for t in delta.traversal] == pinned
    graph.replay()
    torch.cuda.synchronize()
    mat = delta.materialize()
    assert torch.equal(out[0], symbolic_traversal_reference(mat.edge_index, mat.edge_type, N, h, r))


def tiled(g, copies):
    """`copies` disjoint copies of the golden graph side by side: the same relations, copies * 200 nodes."""
    n = g["num_nodes"]
    index = torch.cat([g["edge_index"] + c * n for c in range(copies)], dim=1)
    data = Data(edge_index=index, edge_type=g["edge_type"].repeat(copies), num_nodes=copies * n, num_relations=g["num_relations"])
    return tasks.build_relation_graph(data)


def golden_edits(graph, delta):
    """Added facts (one repeated, one between far-apart nodes) and tombstones on stated facts of the golden edge list."""
    n, half = int(graph.num_nodes), int(graph.num_relations) // 2
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    direct = (et < half).nonzero().flatten()[[0, 57, 400, 1200]]
    delta.add([3, 3, n - 1, 150], [0, 0, 4, 5], [n - 2, n - 2, 7, 150])
    removed = delta.remove(ei[0, direct], et[direct], ei[1, direct])
    assert bool((removed >= 1).all())


@pytest.mark.parametrize("copies", [1, 8])
def test_projections_with_a_delta_equal_themselves_on_the_materialised_graph(dev, copies, monkeypatch):
    g = load()
    model = build_model(g, dev)
    graph = golden_graph(g, dev) if copies == 1 else tiled(g, copies).to(dev)
    n = int(graph.num_nodes)
    delta = rspmm.GraphDelta(graph, capacity=16)
    golden_edits(graph, delta)
    mat = delta.materialize(graph)
    gen = torch.Generator().manual_seed(3)
    h_prob = (torch.rand(4, n, generator=gen) * (torch.rand(4, n, generator=gen) < 0.1)).to(dev)
    h_prob[0] = 0.0
    h_prob[0, 3] = 1.0                                                  # a one-hot set at a head of an added fact
    r_index = torch.tensor([0, 4, 7, 11], device=dev)
    calls = counted(monkeypatch, ["ultra_rspmm_edit_rows", ENTRY])
    projection, symbolic = model.model, model.symbolic_model
    with torch.no_grad():
        got = projection.forward_delta(graph, h_prob, r_index, delta)
        engine_calls = calls["ultra_rspmm_edit_rows"]
        want = projection(mat, h_prob, r_index)
        base = projection(graph, h_prob, r_index)
        assert torch.equal(got, want) and not torch.equal(got, base)
        assert torch.equal(projection.forward_delta(graph, h_prob, r_index, rspmm.GraphDelta(graph, 2)), base)       # an empty delta
        # the entity model alone, on the relation representations of the delta's relation graph
        rel = projection.model.relation_model(delta.relation_graph, query=r_index)
        query = rel[torch.arange(4, device=dev), r_index]
        x = h_prob.unsqueeze(-1) * query.unsqueeze(1)
        entity = projection.model.entity_model
        assert torch.equal(entity(graph, x, rel, query, delta=delta), entity(mat, x, rel, query))
        assert torch.equal(symbolic(graph, h_prob, r_index, delta=delta), symbolic(mat, h_prob, r_index))
    assert calls[ENTRY] == 1
    print("copies=%d: ultra_rspmm_edit_rows calls of one projection with a delta: %d" % (copies, engine_calls))
    if copies > 1:
        assert engine_calls > 0, "the large copy takes the engine route"
    # the rules: eval mode, no keep vectors
    with torch.no_grad(), pytest.raises(ValueError):
        graph.traversal_keep = torch.ones(graph.edge_index.shape[1], device=dev)
        try:
            projection.forward_delta(graph, h_prob, r_index, delta)
        finally:
            del graph.traversal_keep
    projection.train()
    try:
        with torch.no_grad(), pytest.raises(ValueError):
            projection.forward_delta(graph, h_prob, r_index, delta)
    finally:
        projection.eval()


def same_sets(got, want):
    return (len(got) == len(want) == 4 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            and torch.equal(got[3], want[3]) and torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)))


def same_topk(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
            and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)))


def test_query_predictor_serves_the_live_graph(dev, monkeypatch):
    g = load()
    model, graph = build_model(g, dev), golden_graph(g, dev)
    nested = list(g["nested"])                                           # all 14 types, the negation types included
    assert len(set(g["type"].tolist())) == 14
    calls = counted(monkeypatch, [ENTRY])
    # never edited: today's entries, today's answers
    plain = query_predict.QueryPredictor(model, graph, k=5, batch_size=8)
    rows = [Query.from_nested(q).tolist() for q in nested]
    untouched = plain.answers(nested)
    plain.answer_sets(nested)
    assert calls[ENTRY] == 0 and plain.delta is None
    assert _same_answers(untouched, _eager_answers(model, graph, rows, plain.batches(nested), 5, True))
    # edited
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=8, delta_capacity=16)
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    direct = (et < 6).nonzero().flatten()[[0, 57, 400, 1200]]
    assert qp.add_facts([5, 78, 40, 62, 199], [0, 3, 3, 0, 5], [78, 150, 150, 27, 0]) == 5
    assert bool((qp.remove_facts(ei[0, direct], et[direct], ei[1, direct]) >= 1).all())
    assert qp.add_facts(int(ei[0, direct[0]]), int(et[direct[0]]), int(ei[1, direct[0]])) == 6       # retracted, stated again
    assert qp.graph is graph and qp.delta.edited
    for state in ("edited", "compacted"):
        mat = qp.materialized()
        fresh = query_predict.QueryPredictor(model, mat, k=5, batch_size=8)
        before = calls[ENTRY]
        got = qp.answers(nested)
        assert (calls[ENTRY] > before) == (state == "edited"), state
        assert same_topk(got, fresh.answers(nested)), state
        assert same_sets(qp.answer_sets(nested, probability=0.5), fresh.answer_sets(nested, probability=0.5)), state
        if state == "edited":
            assert not same_topk(got, untouched), "the edits change answers of the fixture"
            qp.compact()
            assert qp.delta is None and qp.graph is not graph
            assert torch.equal(qp.graph.edge_index, mat.edge_index) and torch.equal(qp.graph.edge_type, mat.edge_type)
    assert not model.training


def test_a_stated_fact_is_traversed_and_entailed(dev):
    """A 2p query whose only path runs through an added edge gains that path's tails as entailed answers, and loses them when the
    fact is retracted; likewise the 1p query of the fact itself."""
    g = load()
    model, graph = build_model(g, dev), golden_graph(g, dev)
    n = int(graph.num_nodes)
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    r1, r2 = 0, 1
    anchor = next(a for a in range(n) if not bool(((ei[0] == a) & (et == r1)).any()))       # no edge of r1 leaves it
    middle = int(ei[0][et == r2][0])
    tails = sorted(set(ei[1][(ei[0] == middle) & (et == r2)].tolist()))
    assert tails and middle != anchor
    qp = query_predict.QueryPredictor(model, graph, k=n, batch_size=4)
    queries = [(anchor, (r1, r2)), (anchor, (r1,))]

    def answers():
        ids, _, count = qp.answers(queries)
        return [ids[i, :int(count[i])].tolist() for i in range(2)], count.tolist()
    lists, count = answers()
    assert count == [n, n] and all(t in lists[0] for t in tails) and middle in lists[1]
    assert qp.add_facts(anchor, r1, middle) == 1
    lists, count = answers()
    assert count == [n - len(tails), n - 1] and not any(t in lists[0] for t in tails) and middle not in lists[1]
    assert qp.remove_facts(anchor, r1, middle).tolist() == [1]
    lists, count = answers()
    assert count == [n, n] and all(t in lists[0] for t in tails) and middle in lists[1]
