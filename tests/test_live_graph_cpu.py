"""Serving a changing graph, the parts that need no GPU: the materialised edge order, the arrays the delta
kernel reads (sorted by (row, col, id), ptr / touched rows, count) on a hand-written 6-node graph, the range errors, and the
Predictor on CPU tensors, where a delta is served by materialising."""
import ctypes

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data


def six_node_graph():
    """6 nodes, 2 direct relations (4 with inverses); node 5 has no edge."""
    h = torch.tensor([0, 0, 1, 2, 3])
    t = torch.tensor([1, 2, 2, 3, 4])
    r = torch.tensor([0, 1, 0, 1, 0])
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + 2]), num_nodes=6,
                num_relations=4)
    return tasks.build_relation_graph(data)


# (h, r, t): into the empty node 5, a self loop, a copy of the base edge (0, 1, 0), the same fact twice
FACTS = [(5, 1, 0), (3, 0, 3), (0, 0, 1), (2, 1, 4), (2, 1, 4)]


def test_materialize_has_the_defined_edge_order():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=8)
    assert len(delta) == 0 and delta.capacity == 8
    count = delta.count
    assert delta.add(*zip(*FACTS[:2])) == 2
    assert delta.add(*FACTS[2]) == 3                 # (a single fact as ints)
    assert delta.add(*zip(*FACTS[3:])) == 5 == len(delta)
    assert delta.count is count                      # the same tensor object across add() calls
    h, r, t = (torch.tensor(v) for v in zip(*FACTS))
    mat = delta.materialize(data)
    want_index = torch.cat([data.edge_index, torch.stack([h, t]), torch.stack([t, h])], dim=1)
    want_type = torch.cat([data.edge_type, r, r + 2])
    assert torch.equal(mat.edge_index, want_index) and torch.equal(mat.edge_type, want_type)
    assert (mat.num_nodes, mat.num_relations) == (6, 4)
    assert data.edge_index.shape[1] == 10            # the base graph is left alone
    # the relation graph is that of the materialised list
    want_rel = tasks.build_relation_graph(Data(edge_index=want_index, edge_type=want_type, num_nodes=6, num_relations=4)).relation_graph
    assert torch.equal(mat.relation_graph.edge_index, want_rel.edge_index)
    assert torch.equal(mat.relation_graph.edge_type, want_rel.edge_type)
    extra_index, extra_type = delta.edges()
    assert torch.equal(extra_index, want_index[:, 10:]) and torch.equal(extra_type, want_type[10:])


def test_prepared_arrays_on_the_six_node_graph():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=8)
    delta.add(*zip(*FACTS))
    m = len(FACTS)
    extra_index, extra_type = delta.edges()
    row, col = extra_index
    # brute force: the delta's edges sorted by (row, col, position in the materialised list)
    order = sorted(range(2 * m), key=lambda e: (int(row[e]), int(col[e]), e))
    touched = sorted(set(int(v) for v in row))
    assert int(delta.count) == len(touched) == 6
    assert delta.rows[:len(touched)].tolist() == touched
    ptr = delta.ptr[:len(touched) + 1].tolist()
    assert ptr[0] == 0 and ptr[-1] == 2 * m
    assert delta.col[:2 * m].tolist() == [int(col[e]) for e in order]
    assert delta.type[:2 * m].tolist() == [int(extra_type[e]) for e in order]
    for k, node in enumerate(touched):
        assert [int(row[e]) for e in order[ptr[k]:ptr[k + 1]]] == [node] * (ptr[k + 1] - ptr[k])
    # spelled out for row 2 <- {4, 4} (the fact stated twice, in insertion order) and row 3 <- {3, 3} (the self loop: its direct
    # edge, type 0, before its inverse, type 2)
    k2, k3 = touched.index(2), touched.index(3)
    assert delta.col[ptr[k2]:ptr[k2 + 1]].tolist() == [4, 4] and delta.type[ptr[k2]:ptr[k2 + 1]].tolist() == [1, 1]
    assert delta.col[ptr[k3]:ptr[k3 + 1]].tolist() == [3, 3] and delta.type[ptr[k3]:ptr[k3 + 1]].tolist() == [0, 2]
    assert delta.degree.tolist() == torch.bincount(extra_index[1], minlength=6).tolist()
    assert delta.col.dtype == delta.type.dtype == delta.rows.dtype == delta.ptr.dtype == delta.count.dtype == torch.int32
    assert delta.col.numel() == 16 and delta.ptr.numel() == 17


def merged_rows(plan, delta):
    """The kernel's walk on the host: per touched row, the (col, type) sequence of the two-way merge on col of the base plan's
    CSR row and the row's delta edges, base edges first at equal col."""
    row_ptr, col, typ = (plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    d_rows, d_ptr, d_col, d_type = (t.tolist() for t in (delta.rows, delta.ptr, delta.col, delta.type))
    out = {}
    for k in range(int(delta.count)):
        row = d_rows[k]
        i, ie, j, je = row_ptr[row], row_ptr[row + 1], d_ptr[k], d_ptr[k + 1]
        seq = []
        while i < ie or j < je:
            if i < ie and (j >= je or col[i] <= d_col[j]):
                seq.append((col[i], typ[i]))
                i += 1
            else:
                seq.append((d_col[j], d_type[j]))
                j += 1
        out[row] = seq
    return out


@pytest.mark.parametrize("graph", ["six", "random"])
def test_the_merge_is_the_sorted_order_of_a_plan_of_the_materialised_graph(graph):
    """What makes the sums bit-equal: walked as the kernel walks it, every touched row lists its edges exactly as a fresh
    reference-order plan of the concatenated edge list sorts them -- (row, col, edge id), the delta edges with the highest ids."""
    if graph == "six":
        data, facts = six_node_graph(), FACTS
    else:
        data = synthetic.make_kg(num_node=30, num_triple=400, num_relation_base=3, num_test=8, seed=5, relation_graph=False)
        g = torch.Generator().manual_seed(9)
        facts = list(zip(torch.randint(0, 30, (40,), generator=g).tolist(), torch.randint(0, 3, (40,), generator=g).tolist(),
                         torch.randint(0, 30, (40,), generator=g).tolist()))
    n, r = int(data.num_nodes), int(data.num_relations)
    delta = rspmm.GraphDelta(data, capacity=64)
    for lo in range(0, len(facts), 7):                   # (in several add() calls: the ids follow the materialised order)
        delta.add(*zip(*facts[lo:lo + 7]))
    mat = delta.materialize(data)
    base_plan = rspmm.Plan(data.edge_index, data.edge_type, n, r, exact_order=True)
    mat_plan = rspmm.Plan(mat.edge_index, mat.edge_type, n, r, exact_order=True)
    row_ptr, col, typ = (mat_plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    merged = merged_rows(base_plan, delta)
    assert sorted(merged) == sorted(set(mat.edge_index[0, data.edge_index.shape[1]:].tolist()))
    for row, seq in merged.items():
        assert seq == list(zip(col[row_ptr[row]:row_ptr[row + 1]], typ[row_ptr[row]:row_ptr[row + 1]])), row
    # ... and no other row of the materialised plan differs from the base plan's
    b_ptr, b_col, b_typ = (base_plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    for row in range(n):
        if row not in merged:
            assert (col[row_ptr[row]:row_ptr[row + 1]], typ[row_ptr[row]:row_ptr[row + 1]]) == \
                (b_col[b_ptr[row]:b_ptr[row + 1]], b_typ[b_ptr[row]:b_ptr[row + 1]])


def test_range_and_inverse_relation_errors():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=2)
    for bad in ((6, 0, 1), (-1, 0, 1), (0, 0, 6), (0, 2, 1), (0, 3, 1), (0, -1, 1)):
        with pytest.raises(ValueError):
            delta.add(*bad)
    with pytest.raises(ValueError):
        delta.add([0, 1], [0], [1, 2])
    assert len(delta) == 0 and int(delta.count) == 0
    delta.add([0, 1], [0, 1], [1, 2])
    with pytest.raises(ValueError):      # beyond the capacity: the caller compacts (Predictor.add_facts)
        delta.add(0, 0, 1)
    with pytest.raises(ValueError):
        rspmm.GraphDelta(data, capacity=0)


@pytest.fixture(scope="module")
def served():
    """A model that runs on CPU tensors: `rotate` messages take the unfused torch path there (the engine has no CPU path), so
    with a delta the forward takes the materialising route of models.py."""
    torch.manual_seed(5)
    model = models.Ultra(**synthetic.default_model_cfg(message_func="rotate"))
    data = synthetic.make_kg(num_node=40, num_triple=120, num_relation_base=3, num_test=8, seed=11)
    return model.eval(), data


def same_answers(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and torch.equal(got[2], want[2]))


def test_predictor_on_cpu_tensors_takes_the_materialising_route(served):
    model, data = served
    live = predict.Predictor(model, data, k=5, batch_size=4)
    h, t, r = data.target_triples[:6].unbind(-1)
    assert live.add_facts(h[:4], r[:4], t[:4]) == 4
    assert live.add_facts(int(h[4]), int(r[4]), int(t[4])) == 5
    mat = live.delta.materialize(data)
    assert mat.edge_index.shape[1] == data.edge_index.shape[1] + 10
    fresh = predict.Predictor(model, mat, k=5, batch_size=4)      # (its filter graph: the materialised graph, as the live one's)
    qh, qt, qr = data.target_triples[:7].unbind(-1)
    assert same_answers(live.tails(qh, qr), fresh.tails(qh, qr))
    assert same_answers(live.heads(qt, qr), fresh.heads(qt, qr))
    floor = 0.0
    for a, b in zip(live.tails_above(qh, qr, floor), fresh.tails_above(qh, qr, floor)):
        assert torch.equal(a, b)
    # ... and the facts changed the scores at all: the base graph answers differently
    base = predict.Predictor(model, data, k=5, batch_size=4)
    assert not torch.equal(base.tails(qh, qr)[1], live.tails(qh, qr)[1])


def test_an_added_facts_tail_leaves_its_own_answers(served):
    model, data = served
    n = int(data.num_nodes)
    probe = predict.Predictor(model, data, k=n, batch_size=2, filtered=True)
    h, r = torch.tensor([3]), torch.tensor([1])
    ids, _, count = probe.tails(h, r)
    tail = int(ids[0, 0])                                  # an entity the graph does not state as a tail of (3, 1, ?)
    assert probe.add_facts(3, 1, tail) == 1
    ids2, _, count2 = probe.tails(h, r)
    assert tail not in ids2[0, :int(count2[0])].tolist()
    assert int(count2[0]) == int(count[0]) - 1
    # the head side of the same fact: (?, 1, tail) no longer offers 3
    ids3, _, count3 = probe.heads(torch.tensor([tail]), r)
    assert 3 not in ids3[0, :int(count3[0])].tolist()


def test_compaction_on_cpu(served):
    model, data = served
    live = predict.Predictor(model, data, k=5, batch_size=4, delta_capacity=2)
    h, t, r = data.target_triples[:3].unbind(-1)
    assert live.add_facts(h[:2], r[:2], t[:2]) == 2
    assert live.add_facts(h[2:], r[2:], t[2:]) == 0       # the third fact exceeds the capacity: compacted
    assert live.data.edge_index.shape[1] == data.edge_index.shape[1] + 6 and len(live.delta) == 0
    whole = rspmm.GraphDelta(data, 4)
    whole.add(h, r, t)
    fresh = predict.Predictor(model, whole.materialize(data), k=5, batch_size=4)
    assert torch.equal(live.data.edge_index, fresh.data.edge_index) and torch.equal(live.data.edge_type, fresh.data.edge_type)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))


def test_the_entry_validates_on_the_host():
    """ultra_rspmm_delta_rows answers before anything is launched (host tensors here): ULTRA_ERR_INVALID for bad arguments,
    ULTRA_ERR_UNSUPPORTED for general-walk plans, rotate messages and rows that are no whole 16-byte chunks, ULTRA_OK where
    there is nothing to do."""
    lib = _lib.lib
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add(*zip(*FACTS[:2]))
    exact = rspmm.Plan(data.edge_index, data.edge_type, 6, 4, exact_order=True)
    loose = rspmm.Plan(data.edge_index, data.edge_type, 6, 4, exact_order=False)
    x, rel, out = torch.zeros(2, 6, 64), torch.zeros(2, 4, 64), torch.zeros(2, 6, 64)
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, out)]
    operand = ctypes.byref(delta.operand())

    def call(plan=exact, sum=0, mul=0, dtype=_lib.F32, relation=mats[0], input=mats[1], boundary=None, rows=None, output=mats[2],
             operand=operand):
        return lib.ultra_rspmm_delta_rows(plan._h if plan is not None else None, sum, mul, dtype, relation, input, boundary, rows,
                                          output, operand, None)
    assert call(plan=None) == _lib.ULTRA_ERR_INVALID
    assert call(sum=3) == _lib.ULTRA_ERR_INVALID and call(mul=5) == _lib.ULTRA_ERR_INVALID and call(dtype=7) == _lib.ULTRA_ERR_INVALID
    assert call(output=None) == _lib.ULTRA_ERR_INVALID and call(operand=None) == _lib.ULTRA_ERR_INVALID
    assert call(rows=torch.zeros(2, dtype=torch.long).data_ptr()) == _lib.ULTRA_ERR_INVALID      # point rows without values
    short = ctypes.byref(rspmm.as_mat(torch.zeros(2, 5, 64))[1])
    assert call(input=short) == _lib.ULTRA_ERR_INVALID and b"input" in lib.ultra_last_error()
    assert call(plan=loose) == _lib.ULTRA_ERR_UNSUPPORTED
    assert call(mul=_lib.MUL_CODES["rotate"]) == _lib.ULTRA_ERR_UNSUPPORTED
    odd = [ctypes.byref(rspmm.as_mat(torch.zeros(2, n, 6))[1]) for n in (4, 6, 6)]
    assert call(relation=odd[0], input=odd[1], output=odd[2]) == _lib.ULTRA_ERR_UNSUPPORTED
    empty = ctypes.byref(rspmm.UltraMat(out.data_ptr(), 0, 0, 6, 64, 64))
    assert call(output=empty) == _lib.ULTRA_OK                                                   # n_outer == 0
    none = _lib.UltraDelta(None, None, None, None, None, 0, 0)
    assert call(operand=ctypes.byref(none)) == _lib.ULTRA_OK                                     # capacity 0
    # Plan.delta_rows: None where the plan is not a reference-order one, before any operand is looked at
    assert loose.delta_rows(rel, x, out, delta) is None
    assert lib.ultra_abi_version() == 7
