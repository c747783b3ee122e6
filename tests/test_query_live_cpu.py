"""Serving logical queries on a changing graph, the parts that need no GPU: the GraphDelta layout in the symbolic
traversal's direction, decoded on the host after every step of scripted edits; QueryPredictor.add_facts / remove_facts / compact /
materialized on stub projections that depend on the edge list they are handed; the 1p behaviour; the argument errors; and the
argument checks of ultra_symbolic_traversal_edit_rows, which answer before any GPU call."""
import ctypes

import pytest
import torch
from torch import nn

from tests.test_query_exec_cpu import random_queries
from ultra_amd import _lib, query_predict, rspmm, tasks
from ultra_amd.data import Data
from ultra_amd.ultraquery import UltraQuery, symbolic_traversal_reference

N, R = 12, 4


def twelve_node_graph(relation_graph=True):
    """12 nodes, 2 direct relations and their inverses.  The fact (0, 0, 1) is stated three times (parallel edges, both directions),
    (3, 0, 4) as its direct edge ONLY and (10, 1, 11) as its inverse edge only; node 8 has no edge."""
    h = torch.tensor([0, 0, 0, 2, 5, 6, 7, 9, 1, 2])
    t = torch.tensor([1, 1, 1, 1, 6, 7, 9, 1, 9, 5])
    r = torch.tensor([0, 0, 0, 0, 1, 1, 0, 1, 1, 0])
    index = torch.cat([torch.stack([h, t]), torch.stack([t, h]), torch.tensor([[3, 11], [4, 10]])], dim=1)
    kind = torch.cat([r, r + 2, torch.tensor([0, 3])])
    data = Data(edge_index=index, edge_type=kind, num_nodes=N, num_relations=R)
    return tasks.build_relation_graph(data) if relation_graph else data


def decoded_traversal(data, delta, h_prob):
    """The definition applied to the layout's arrays in plain Python: t[r, v] over the base edges minus the dead ones plus the added
    ones for the touched tails, the base graph's own traversal elsewhere; sample r asks for relation r.  Asserts the layout's
    orders on the way."""
    lay = delta.traversal
    count = int(lay.count)
    rows = lay.rows[:count].tolist()
    assert rows == sorted(set(rows)), rows
    add_ptr, dead_ptr = lay.add_ptr[:count + 1].tolist(), lay.dead_ptr[:count + 1].tolist()
    assert add_ptr[0] == 0 and dead_ptr[0] == 0
    assert add_ptr[-1] == 2 * len(delta) and dead_ptr[-1] == delta.num_removed
    add = list(zip(lay.add_type.tolist(), lay.add_src.tolist()))
    dead = list(zip(lay.dead_type.tolist(), lay.dead_src.tolist()))
    base = list(zip(data.edge_index[0].tolist(), data.edge_index[1].tolist(), data.edge_type.tolist()))
    out = symbolic_traversal_reference(data.edge_index, data.edge_type, N, h_prob, torch.arange(R))
    for k, v in enumerate(rows):
        mine, keys = add[add_ptr[k]:add_ptr[k + 1]], dead[dead_ptr[k]:dead_ptr[k + 1]]
        assert mine == sorted(mine), "added edges are sorted by (type, src) within a tail"
        assert keys == sorted(set(keys)), "dead keys are distinct and sorted by (type, src) within a tail"
        assert mine or keys, "a touched tail has an added edge or a dead key"
        for r in range(R):
            live = [u for (u, w, kind) in base if w == v and kind == r and (kind, u) not in keys]
            live += [u for (kind, u) in mine if kind == r]
            out[r, v] = max([0.0] + [float(h_prob[r, u]) for u in live])
    return out


def test_traversal_layout_follows_scripted_edits():
    data = twelve_node_graph()
    delta = rspmm.GraphDelta(data, capacity=8)
    assert delta.traversal is None            # laid out when first asked for: a Predictor never pays for it
    gen = torch.Generator().manual_seed(5)
    h_prob = torch.rand(R, N, generator=gen) - 0.2         # (some negative entries: the clamp at 0)
    pinned = []

    def check(step):
        operand = delta.traversal_operand()
        lay = delta.traversal
        now = [t.data_ptr() for t in lay] + [id(lay.count)]
        if pinned:
            assert now == pinned[0], "%s: the buffers and the count tensor stay where they are" % step
        else:
            pinned.append(now)
        assert (operand.row_dev, operand.count_dev, operand.dead_ptr_dev) == (lay.rows.data_ptr(), lay.count.data_ptr(),
                                                                              lay.dead_ptr.data_ptr())
        assert (operand.capacity_rows, operand.capacity_edges, operand.capacity_keys) == (16, 16, 16)
        assert all(t.dtype == torch.int32 for t in lay)
        mat = delta.materialize()
        want = symbolic_traversal_reference(mat.edge_index, mat.edge_type, N, h_prob, torch.arange(R))
        assert torch.equal(decoded_traversal(data, delta, h_prob), want), step

    delta.add(8, 1, 3)                                              # into the edge-less node 8 (inverse edge) and into 3
    check("add")
    delta.add([8, 2], [1, 0], [3, 1])                               # a duplicate of it; a copy of the base fact (2, 0, 1)
    check("add a duplicate")
    assert delta.remove(0, 0, 1).tolist() == [3]                    # three parallel base edges, one key per direction
    assert delta.num_removed == 2
    check("remove a base fact that has duplicates")
    version = delta.version
    assert delta.remove(4, 1, 8).tolist() == [0] and delta.version == version
    check("remove a fact stated nowhere")
    assert delta.remove(3, 0, 4).tolist() == [1] and delta.num_removed == 3      # stated as its direct edge only: ONE key
    check("remove a fact stated in one direction only")
    assert delta.remove(10, 1, 11).tolist() == [0] and delta.num_removed == 4    # ... as its inverse edge only: no direct edge went
    check("remove a fact stated as its inverse edge only")
    delta.remove(5, 1, 6)
    delta.add(5, 1, 6)
    check("remove then re-add")
    assert delta.remove(8, 1, 3).tolist() == [2] and len(delta) == 2             # both added copies
    check("remove an added fact")
    # the tombstones are not symmetric: tail 4 holds the key (3, 0), tail 3 holds no key of relation 2
    lay, count = delta.traversal, int(delta.traversal.count)
    rows, dead_ptr = lay.rows[:count].tolist(), lay.dead_ptr[:count + 1].tolist()
    k4 = rows.index(4)
    assert list(zip(lay.dead_src.tolist(), lay.dead_type.tolist()))[dead_ptr[k4]:dead_ptr[k4 + 1]] == [(3, 0)]
    assert 3 not in rows


class EdgeListStub(nn.Module):
    """A projection that depends on the edge list of the graph it is handed (and takes no `delta`): the symbolic one is the
    traversal's restatement, the neural one a deterministic function of it.  Records the graphs it saw."""

    def __init__(self, symbolic):
        super(EdgeListStub, self).__init__()
        self.symbolic = symbolic
        self.graphs = []

    def forward(self, graph, h_prob, r_index):
        self.graphs.append(graph)
        r_index = r_index.as_subclass(torch.Tensor)
        out = symbolic_traversal_reference(graph.edge_index, graph.edge_type, graph.num_nodes, h_prob, r_index)
        if self.symbolic:
            return out
        col = torch.arange(h_prob.shape[1], dtype=torch.float32)
        return torch.sigmoid(out * 3 - 1 + torch.sin(col * 0.37 + r_index.float().unsqueeze(1)) + 0.25 * h_prob)


def edge_list_model(logic="product"):
    uq = UltraQuery(nn.Module(), logic=logic)
    uq.model, uq.symbolic_model = EdgeListStub(False), EdgeListStub(True)
    return uq.eval()


def same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


def check_against_fresh(qp, queries):
    """answers / answer_sets of the edited predictor against a fresh one on qp.materialized(), exactly; every projection of the
    edited one saw the materialised edge list."""
    mat = qp.materialized()
    if qp.delta is not None and qp.delta.edited:
        want = qp.delta.materialize(qp.graph)
        assert torch.equal(mat.edge_index, want.edge_index) and torch.equal(mat.edge_type, want.edge_type)
        assert mat.relation_graph is qp.delta.relation_graph
    for stub in (qp.model.model, qp.model.symbolic_model):
        del stub.graphs[:]
    got = qp.answers(queries), qp.answer_sets(queries, probability=0.45)
    for stub in (qp.model.model, qp.model.symbolic_model):
        assert stub.graphs, "the projections ran"
        for graph in stub.graphs:
            assert torch.equal(graph.edge_index, mat.edge_index) and torch.equal(graph.edge_type, mat.edge_type)
    fresh = query_predict.QueryPredictor(edge_list_model(qp.model.logic), mat, k=qp.k, batch_size=qp.batch_size)
    assert same(got[0], fresh.answers(queries))
    assert same(got[1], fresh.answer_sets(queries, probability=0.45))
    return got


@pytest.mark.parametrize("logic", ["product", "godel"])
def test_query_predictor_serves_the_materialised_graph(logic):
    data = twelve_node_graph()
    queries = random_queries(9, N, R, seed=11)
    qp = query_predict.QueryPredictor(edge_list_model(logic), data, k=5, batch_size=4, delta_capacity=2)
    assert qp.delta is None and qp.materialized() is data
    check_against_fresh(qp, queries)
    assert qp.add_facts(8, 1, 3) == 1 and qp.delta is not None and qp.graph is data
    check_against_fresh(qp, queries)
    assert qp.remove_facts([0], [0], [1]).tolist() == [3]                 # one fact + one retraction: the capacity of 2 is full
    assert qp.graph is data and len(qp.delta) == 1 and qp.delta.num_removed == 2
    check_against_fresh(qp, queries)
    # the next fact does not fit: the delta is folded, the fact included, and the served graph is the materialised one
    surviving = qp.delta.materialize(data).edge_index[:, :-2]
    want = torch.cat([surviving, torch.tensor([[8, 4], [3, 2]]), torch.tensor([[3, 2], [8, 4]])], dim=1)
    assert qp.add_facts(4, 0, 2) == 0
    assert qp.delta is None and qp.graph is not data and torch.equal(qp.graph.edge_index, want)
    want_rel = tasks.build_relation_graph(Data(edge_index=want, edge_type=qp.graph.edge_type, num_nodes=N, num_relations=R))
    assert torch.equal(qp.graph.relation_graph.edge_index, want_rel.relation_graph.edge_index)
    check_against_fresh(qp, queries)
    # three retractions at once exceed the whole capacity: applied to a delta of their own and folded at once
    assert qp.remove_facts([5, 6, 9], [1, 1, 1], [6, 7, 1]).tolist() == [1, 1, 1]
    assert qp.delta is None and qp.graph.edge_index.shape[1] == want.shape[1] - 6
    check_against_fresh(qp, queries)
    # an explicit compact() with edits held
    qp.add_facts(1, 1, 0)
    held = qp.materialized()
    assert qp.delta.edited and held is not qp.graph
    qp.compact()
    assert qp.delta is None and torch.equal(qp.graph.edge_index, held.edge_index) and torch.equal(qp.graph.edge_type, held.edge_type)
    check_against_fresh(qp, queries)
    # an empty call changes nothing
    assert qp.add_facts([], [], []) == 0 and qp.remove_facts([], [], []).numel() == 0 and qp.delta is None


def test_a_stated_fact_is_entailed_and_a_retracted_one_is_not():
    data = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), data, k=N, batch_size=4)
    h, r, t = 2, 0, 8
    ids, _, count = qp.answers([(h, (r,))])
    assert t in ids[0, :int(count[0])].tolist()
    assert qp.add_facts(h, r, t) == 1
    ids2, _, count2 = qp.answers([(h, (r,))])
    assert t not in ids2[0, :int(count2[0])].tolist() and int(count2[0]) == int(count[0]) - 1
    assert qp.remove_facts(h, r, t).tolist() == [1]
    ids3, _, count3 = qp.answers([(h, (r,))])
    assert t in ids3[0, :int(count3[0])].tolist() and int(count3[0]) == int(count[0])
    # ... and a base fact: retracted, its tail is a candidate again
    ids4, _, count4 = qp.answers([(5, (1,))])
    assert 6 not in ids4[0, :int(count4[0])].tolist()
    qp.remove_facts(5, 1, 6)
    ids5, _, count5 = qp.answers([(5, (1,))])
    assert 6 in ids5[0, :int(count5[0])].tolist() and int(count5[0]) == int(count4[0]) + 1


def test_argument_errors():
    qp = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), k=3)
    for call in (qp.add_facts, qp.remove_facts):
        with pytest.raises(ValueError):
            call(0, 2, 1)                     # an inverse relation
        with pytest.raises(ValueError):
            call(0, 0, N)                     # an id out of range
        with pytest.raises(ValueError):
            call(-1, 0, 1)
        with pytest.raises(ValueError):
            call([0, 1], [0], [1, 2])         # mismatched lengths
    assert qp.delta is None
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), delta_capacity=bad)


def test_the_entry_validates_before_any_gpu_call():
    """ultra_symbolic_traversal_edit_rows on host tensors: ULTRA_ERR_INVALID for a NULL operand, a bad dtype, a batch or num_node
    outside the base entry's range and broken edits; ULTRA_OK where there is nothing to do.  Nothing is launched."""
    lib = _lib.lib
    data = twelve_node_graph()
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add(8, 1, 3)
    delta.remove(0, 0, 1)
    edits = delta.traversal_operand()
    row_ptr = torch.zeros(N + 1, dtype=torch.int64)
    src, kind = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    r_index = torch.zeros(2, dtype=torch.int64)
    h, t = torch.zeros(2, N), torch.zeros(2, N)
    default = dict(row_ptr=row_ptr.data_ptr(), src=src.data_ptr(), kind=kind.data_ptr(), num_node=N, edits=ctypes.byref(edits),
                   r=r_index.data_ptr(), batch=2, dtype=_lib.F32, h=h.data_ptr(), t=t.data_ptr())

    def call(**change):
        a = dict(default, **change)
        return lib.ultra_symbolic_traversal_edit_rows(a["row_ptr"], a["src"], a["kind"], a["num_node"], a["edits"], a["r"],
                                                      a["batch"], a["dtype"], a["h"], a["t"], None)
    for name in ("row_ptr", "src", "kind", "edits", "r", "h", "t"):
        assert call(**{name: None}) == _lib.ULTRA_ERR_INVALID, name
        assert b"ultra_symbolic_traversal_edit_rows" in lib.ultra_last_error()
    assert call(dtype=7) == _lib.ULTRA_ERR_INVALID and call(dtype=-1) == _lib.ULTRA_ERR_INVALID
    assert call(batch=-1) == _lib.ULTRA_ERR_INVALID and call(batch=65536) == _lib.ULTRA_ERR_INVALID
    assert call(num_node=0) == _lib.ULTRA_ERR_INVALID and call(num_node=2 ** 31) == _lib.ULTRA_ERR_INVALID
    fields = [name for name, _ in _lib.UltraTraversalEdits._fields_]

    def changed(**change):
        values = {name: getattr(edits, name) for name in fields}
        values.update(change)
        return ctypes.byref(_lib.UltraTraversalEdits(*[values[name] for name in fields]))
    for name in ("row_dev", "count_dev", "add_ptr_dev", "add_src_dev", "add_type_dev", "dead_src_dev", "dead_type_dev"):
        assert call(edits=changed(**{name: None})) == _lib.ULTRA_ERR_INVALID, name
    for name in ("capacity_rows", "capacity_edges", "capacity_keys"):
        assert call(edits=changed(**{name: -1})) == _lib.ULTRA_ERR_INVALID, name
    # nothing to do: no row, no sample -- also without tombstone arrays at all
    assert call(edits=changed(capacity_rows=0)) == _lib.ULTRA_OK
    assert call(edits=changed(capacity_rows=0, dead_ptr_dev=None, dead_src_dev=None, dead_type_dev=None)) == _lib.ULTRA_OK
    assert call(batch=0) == _lib.ULTRA_OK
    assert torch.equal(t, torch.zeros(2, N))
    assert lib.ultra_abi_version() == 7
