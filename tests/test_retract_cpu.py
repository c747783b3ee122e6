"""Retracting facts from a served graph, the parts that need no GPU: what GraphDelta.remove returns and holds, the
arrays ultra_rspmm_edit_rows reads (union rows, both ptr arrays, sorted tombstone keys, signed degree, count) on a hand-written
6-node graph, the materialised edge order, the kernel's merge-with-tombstones restated on the host against a plan of the
materialised list, the range errors, the Predictor on CPU tensors, and the host-side validation of the new entry."""
import ctypes

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data


def six_node_graph():
    """6 nodes, 2 direct relations (4 with inverses); node 5 has no edge; the triple (0, 0, 1) is stated twice."""
    h = torch.tensor([0, 0, 1, 2, 3, 0])
    t = torch.tensor([1, 2, 2, 3, 4, 1])
    r = torch.tensor([0, 1, 0, 1, 0, 0])
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + 2]), num_nodes=6,
                num_relations=4)
    return tasks.build_relation_graph(data)


ADDED = [(5, 1, 0), (2, 1, 4), (2, 1, 4)]
# (h, r, t): the base triple stated twice, the delta fact stated twice, a fact stated nowhere, a base triple stated once
REMOVED = [(0, 0, 1), (2, 1, 4), (4, 1, 5), (2, 1, 3)]


def edited_delta():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=8)
    delta.add(*zip(*ADDED))
    counts = delta.remove(*zip(*REMOVED))
    return data, delta, counts


def materialized_by_hand(data, gone, facts):
    """[base edges equal to no triple of `gone` (h, r, t) nor its inverse, in base order ; direct ; inverse]."""
    half = data.num_relations // 2
    dead = set()
    for h, r, t in gone:
        dead |= {(h, t, r), (t, h, r + half)}
    keep = [e for e in range(data.edge_index.shape[1])
            if (int(data.edge_index[0, e]), int(data.edge_index[1, e]), int(data.edge_type[e])) not in dead]
    fh, fr, ft = (torch.tensor(v, dtype=torch.long) for v in (zip(*facts) if facts else ((), (), ())))
    index = torch.cat([data.edge_index[:, keep], torch.stack([fh, ft]), torch.stack([ft, fh])], dim=1)
    return index, torch.cat([data.edge_type[keep], fr, fr + half])


def test_remove_returns_the_direct_edges_each_fact_took_out():
    data, delta, counts = edited_delta()
    assert counts.dtype == torch.long and counts.tolist() == [2, 2, 0, 1]
    assert len(delta) == 1 and delta.facts[:1].tolist() == [[5, 1, 0]]
    assert delta.num_removed == 4 and delta.edited
    # a second retraction of the same facts finds nothing: no count, no capacity, no version
    version, keys = delta.version, list(delta.dead_keys)
    assert delta.remove(*zip(*REMOVED)).tolist() == [0, 0, 0, 0]
    assert delta.remove(4, 1, 5).tolist() == [0]
    assert delta.version == version and delta.dead_keys == keys and delta.num_removed == 4
    assert delta.remove([], [], []).numel() == 0
    empty = rspmm.GraphDelta(data, capacity=2)
    assert not empty.edited and empty.num_removed == 0
    assert empty.remove(4, 1, 5).tolist() == [0] and not empty.edited and empty.version == 0


def test_later_facts_move_up_in_insertion_order():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=8)
    delta.add(*zip(*[(5, 1, 0), (2, 1, 4), (3, 0, 3), (2, 1, 4), (1, 1, 5)]))
    assert delta.remove(2, 1, 4).tolist() == [2]
    assert len(delta) == 3 and delta.facts[:3].tolist() == [[5, 1, 0], [3, 0, 3], [1, 1, 5]]
    assert delta.num_removed == 0                    # the base graph never stated it: no tombstone
    # in one call the facts are retracted one after the other: the second copy of a fact finds nothing left
    assert delta.remove([0, 0], [0, 0], [1, 1]).tolist() == [2, 0]


def test_prepared_arrays_on_the_six_node_graph():
    data, delta, _ = edited_delta()
    count = delta.count
    # touched rows: 0 (the edge (0, 1, 0) twice; the added inverse edge 0 <- 5), 1 (its inverse twice), 2 and 3 ((2, 1, 3) and its
    # inverse), 5 (the added edge 5 <- 0)
    assert int(delta.count) == 5 and delta.rows[:5].tolist() == [0, 1, 2, 3, 5]
    assert delta.ptr[:6].tolist() == [0, 1, 1, 1, 1, 2]                      # rows 1, 2, 3: removals only, an empty range
    assert delta.col[:2].tolist() == [5, 0] and delta.type[:2].tolist() == [3, 1]
    assert delta.dead_ptr[:6].tolist() == [0, 1, 2, 3, 4, 4]
    assert delta.dead_col[:4].tolist() == [1, 0, 3, 2] and delta.dead_type[:4].tolist() == [0, 2, 1, 3]
    mat = delta.materialize(data)
    signed = torch.bincount(mat.edge_index[1], minlength=6) - torch.bincount(data.edge_index[1], minlength=6)
    assert delta.degree.tolist() == signed.tolist() == [-1, -2, -1, -1, 0, 1]
    for buf in (delta.dead_col, delta.dead_type, delta.dead_ptr):
        assert buf.dtype == torch.int32
    assert delta.dead_col.numel() == delta.dead_type.numel() == 16 and delta.dead_ptr.numel() == 17
    assert delta.rows.numel() == 16 and delta.ptr.numel() == 17 and delta.col.numel() == 16       # the sizes of an add-only delta
    # the buffers keep their addresses and `count` its identity across further edits
    addresses = [b.data_ptr() for b in (delta.rows, delta.ptr, delta.dead_ptr, delta.dead_col, delta.dead_type, delta.count)]
    delta.remove(3, 0, 4)
    delta.add(1, 0, 1)
    assert delta.count is count
    assert addresses == [b.data_ptr() for b in (delta.rows, delta.ptr, delta.dead_ptr, delta.dead_col, delta.dead_type, delta.count)]
    # a self loop: both of its keys land in one row, sorted by type
    loop = rspmm.GraphDelta(Data(edge_index=torch.tensor([[2, 2, 0], [2, 2, 1]]), edge_type=torch.tensor([1, 3, 0]), num_nodes=3,
                                 num_relations=4), capacity=2)
    assert loop.remove(2, 1, 2).tolist() == [1]
    assert int(loop.count) == 1 and loop.rows[:1].tolist() == [2] and loop.ptr[:2].tolist() == [0, 0]
    assert loop.dead_ptr[:2].tolist() == [0, 2] and loop.dead_col[:2].tolist() == [2, 2] and loop.dead_type[:2].tolist() == [1, 3]


def test_materialize_has_the_defined_edge_order():
    data, delta, _ = edited_delta()
    mat = delta.materialize(data)
    want_index, want_type = materialized_by_hand(data, REMOVED, [(5, 1, 0)])
    assert torch.equal(mat.edge_index, want_index) and torch.equal(mat.edge_type, want_type)
    assert mat.edge_index.shape[1] == 12 - 6 + 2
    assert data.edge_index.shape[1] == 12            # the base graph is left alone
    want_rel = tasks.build_relation_graph(Data(edge_index=want_index, edge_type=want_type, num_nodes=6, num_relations=4)).relation_graph
    assert torch.equal(mat.relation_graph.edge_index, want_rel.edge_index)
    assert torch.equal(mat.relation_graph.edge_type, want_rel.edge_type)


def test_remove_then_add_and_add_then_remove():
    data = six_node_graph()
    # remove, then add: tombstones apply to base edges only -- ONE new edge pair at the end of the list, both base copies gone
    delta = rspmm.GraphDelta(data, capacity=4)
    assert delta.remove(0, 0, 1).tolist() == [2]
    assert delta.add(0, 0, 1) == 1
    mat = delta.materialize(data)
    want_index, want_type = materialized_by_hand(data, [(0, 0, 1)], [(0, 0, 1)])
    assert torch.equal(mat.edge_index, want_index) and torch.equal(mat.edge_type, want_type)
    assert mat.edge_index.shape[1] == 12 - 4 + 2 and delta.num_removed == 2 and len(delta) == 1
    # add, then remove: the added copy and both base copies go
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add(0, 0, 1)
    assert delta.remove(0, 0, 1).tolist() == [3]
    mat = delta.materialize(data)
    want_index, want_type = materialized_by_hand(data, [(0, 0, 1)], [])
    assert torch.equal(mat.edge_index, want_index) and torch.equal(mat.edge_type, want_type)
    assert len(delta) == 0 and delta.num_removed == 2 and delta.edited


def test_a_relation_that_loses_its_last_edge_changes_the_relation_graph():
    h, t, r = torch.tensor([0, 1, 2, 3]), torch.tensor([1, 2, 3, 4]), torch.tensor([0, 0, 1, 2])
    data = tasks.build_relation_graph(Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]),
                                           edge_type=torch.cat([r, r + 3]), num_nodes=6, num_relations=6))
    delta = rspmm.GraphDelta(data, capacity=4)
    graph = delta.relation_graph
    assert delta.remove(0, 0, 1).tolist() == [1]     # relation 0 keeps the edge (1, 0, 2) ...
    delta.remove(3, 2, 4)                            # ... relation 2 loses its only one
    assert delta.relation_graph is not graph
    mat = delta.materialize(data)
    fresh = tasks.build_relation_graph(Data(edge_index=mat.edge_index, edge_type=mat.edge_type, num_nodes=6, num_relations=6))
    assert torch.equal(delta.relation_graph.edge_index, fresh.relation_graph.edge_index)
    assert torch.equal(delta.relation_graph.edge_type, fresh.relation_graph.edge_type)
    assert not (delta.relation_graph.edge_index.shape == graph.edge_index.shape and torch.equal(delta.relation_graph.edge_index, graph.edge_index)
                and torch.equal(delta.relation_graph.edge_type, graph.edge_type))


def merged_rows(plan, delta):
    """ultra_rspmm_edit_rows' walk on the host: per touched row, the (col, type) sequence of the merge on col of the base plan's CSR
    row -- without the edges whose (col, type) is among the row's keys -- and the row's delta edges, base edges first at equal col."""
    row_ptr, col, typ = (plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    d_rows, d_ptr, d_col, d_type = (t.tolist() for t in (delta.rows, delta.ptr, delta.col, delta.type))
    t_ptr, t_col, t_type = (t.tolist() for t in (delta.dead_ptr, delta.dead_col, delta.dead_type))
    out = {}
    for k in range(int(delta.count)):
        row = d_rows[k]
        keys = list(zip(t_col[t_ptr[k]:t_ptr[k + 1]], t_type[t_ptr[k]:t_ptr[k + 1]]))
        assert keys == sorted(set(keys))             # distinct, sorted by (col, type)
        base = [(col[i], typ[i]) for i in range(row_ptr[row], row_ptr[row + 1]) if (col[i], typ[i]) not in keys]
        i, j, je = 0, d_ptr[k], d_ptr[k + 1]
        seq = []
        while i < len(base) or j < je:
            if i < len(base) and (j >= je or base[i][0] <= d_col[j]):
                seq.append(base[i])
                i += 1
            else:
                seq.append((d_col[j], d_type[j]))
                j += 1
        out[row] = seq
    return out


@pytest.mark.parametrize("graph", ["six", "random"])
def test_the_merge_is_the_sorted_order_of_a_plan_of_the_materialised_graph(graph):
    """What makes the sums bit-equal: walked as the kernel walks it, every touched row lists its edges exactly as a fresh
    reference-order plan of the materialised list sorts them -- a subsequence of a sorted row is still sorted."""
    if graph == "six":
        data, delta, _ = edited_delta()
    else:
        data = synthetic.make_kg(num_node=30, num_triple=400, num_relation_base=3, num_test=8, seed=5, relation_graph=False)
        g = torch.Generator().manual_seed(9)
        delta = rspmm.GraphDelta(data, capacity=96)
        half = data.edge_index.shape[1] // 2
        for lo in range(0, 42, 7):                   # (in several calls, additions and retractions interleaved)
            delta.add(torch.randint(0, 30, (7,), generator=g), torch.randint(0, 3, (7,), generator=g), torch.randint(0, 30, (7,), generator=g))
            pick = torch.randint(0, half, (7,), generator=g)
            took = delta.remove(data.edge_index[0, pick], data.edge_type[pick], data.edge_index[1, pick])
            assert took.shape == (7,)
        assert delta.num_removed >= 40 and len(delta) >= 30
    n, r = int(data.num_nodes), int(data.num_relations)
    mat = delta.materialize(data)
    base_plan = rspmm.Plan(data.edge_index, data.edge_type, n, r, exact_order=True)
    mat_plan = rspmm.Plan(mat.edge_index, mat.edge_type, n, r, exact_order=True)
    row_ptr, col, typ = (mat_plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    merged = merged_rows(base_plan, delta)
    for row, seq in merged.items():
        assert seq == list(zip(col[row_ptr[row]:row_ptr[row + 1]], typ[row_ptr[row]:row_ptr[row + 1]])), row
    # ... and no other row of the materialised plan differs from the base plan's
    b_ptr, b_col, b_typ = (base_plan.export(which).tolist() for which in (_lib.ARR_ROW_PTR, _lib.ARR_COL, _lib.ARR_TYPE))
    changed = 0
    for row in range(n):
        same = (col[row_ptr[row]:row_ptr[row + 1]], typ[row_ptr[row]:row_ptr[row + 1]]) == \
            (b_col[b_ptr[row]:b_ptr[row + 1]], b_typ[b_ptr[row]:b_ptr[row + 1]])
        assert same or row in merged, row
        changed += not same
    assert changed >= 4
    signed = torch.bincount(mat.edge_index[1], minlength=n) - torch.bincount(data.edge_index[1], minlength=n)
    assert torch.equal(delta.degree, signed)


def test_range_inverse_relation_and_capacity_errors():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=2)
    for bad in ((6, 0, 1), (-1, 0, 1), (0, 0, 6), (0, 2, 1), (0, 3, 1), (0, -1, 1)):
        with pytest.raises(ValueError):
            delta.remove(*bad)
    with pytest.raises(ValueError):
        delta.remove([0, 1], [0], [1, 2])
    assert not delta.edited and int(delta.count) == 0
    # capacity counts edits: num_facts + num_removed / 2 <= capacity
    delta.add(5, 1, 0)
    assert delta.remove(0, 0, 1).tolist() == [2] and delta.num_removed == 2
    with pytest.raises(ValueError):                  # a third edit: the caller compacts (Predictor.remove_facts / add_facts)
        delta.remove(2, 1, 3)
    with pytest.raises(ValueError):
        delta.add(1, 1, 1)
    assert delta.num_removed == 2 and len(delta) == 1 and int(delta.count) == 3       # nothing was changed
    assert delta.remove(4, 1, 5).tolist() == [0]     # a fact stated nowhere needs no room
    assert delta.remove(5, 1, 0).tolist() == [1]     # nor does one that only frees a slot ...
    assert delta.remove(2, 1, 3).tolist() == [1]     # ... which the next retraction takes


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


def stated_triples(data, count):
    half = data.edge_index.shape[1] // 2
    return data.edge_index[0, :count], data.edge_type[:count], data.edge_index[1, :count], half


def test_predictor_on_cpu_tensors_takes_the_materialising_route(served):
    model, data = served
    h, r, t, _ = stated_triples(data, 4)
    assert bool((r < data.num_relations // 2).all())
    live = predict.Predictor(model, data, k=5, batch_size=4)
    base = predict.Predictor(model, data, k=5, batch_size=4)
    qh, qt, qr = data.target_triples[:7].unbind(-1)
    before = base.tails(qh, qr)
    took = live.remove_facts(h[:3], r[:3], t[:3])
    assert took.dtype == torch.long and bool((took >= 1).all())
    last = live.remove_facts(int(h[3]), int(r[3]), int(t[3]))            # (a single fact as ints)
    assert last.tolist() == [int(((data.edge_index[0] == h[3]) & (data.edge_index[1] == t[3]) & (data.edge_type == r[3])).sum())]
    assert live.add_facts(qh[:1], qr[:1], qt[:1]) == 1
    assert live.delta.num_removed == 8 and live.data is data             # no compaction: tombstones beside the base graph
    mat = live.delta.materialize(data)
    want_index, want_type = materialized_by_hand(data, list(zip(h.tolist(), r.tolist(), t.tolist())),
                                                 [(int(qh[0]), int(qr[0]), int(qt[0]))])
    assert torch.equal(mat.edge_index, want_index) and torch.equal(mat.edge_type, want_type)
    assert mat.edge_index.shape[1] == data.edge_index.shape[1] - 2 * int(took.sum() + last.sum()) + 2
    fresh = predict.Predictor(model, mat, k=5, batch_size=4)
    assert same_answers(live.tails(qh, qr), fresh.tails(qh, qr))
    assert same_answers(live.heads(qt, qr), fresh.heads(qt, qr))
    for a, b in zip(live.tails_above(qh, qr, 0.0), fresh.tails_above(qh, qr, 0.0)):
        assert torch.equal(a, b)
    assert not torch.equal(before[1], live.tails(qh, qr)[1])              # the edits changed the scores at all


@pytest.mark.parametrize("separate_filter", [False, True])
def test_a_retracted_tail_is_an_answer_again(served, separate_filter):
    model, data = served
    n = int(data.num_nodes)
    h, r, t, _ = stated_triples(data, 1)
    kwargs = {}
    if separate_filter:
        filtered = Data(edge_index=data.edge_index.clone(), edge_type=data.edge_type.clone(), num_nodes=n,
                        num_relations=data.num_relations)
        kwargs["filtered_data"] = filtered
    probe = predict.Predictor(model, data, k=n, batch_size=2, filtered=True, **kwargs)
    ids, _, count = probe.tails(h, r)
    assert int(t) not in ids[0, :int(count[0])].tolist()                  # stated: a known answer, left out
    assert int(probe.remove_facts(h, r, t)) >= 1
    ids2, _, count2 = probe.tails(h, r)
    assert int(t) in ids2[0, :int(count2[0])].tolist() and int(count2[0]) == int(count[0]) + 1
    # the head side of the same fact: (?, r, t) offers h again
    ids3, _, count3 = probe.heads(t, r)
    assert int(h) in ids3[0, :int(count3[0])].tolist()
    # stated again: known again
    probe.add_facts(h, r, t)
    ids4, _, count4 = probe.tails(h, r)
    assert int(t) not in ids4[0, :int(count4[0])].tolist() and int(count4[0]) == int(count[0])


def test_compaction_on_cpu(served):
    model, data = served
    h, r, t, _ = stated_triples(data, 6)
    live = predict.Predictor(model, data, k=5, batch_size=4, delta_capacity=2)
    assert live.add_facts(7, 0, 9) == 1
    took = live.remove_facts(h[:1], r[:1], t[:1])
    assert live.data is data and live.delta.num_removed == 2             # two edits fit
    took = torch.cat([took, live.remove_facts(h[1:3], r[1:3], t[1:3])])  # two more do not: compacted first, then held
    assert live.data is not data and len(live.delta) == 0 and live.delta.num_removed == 4
    took = torch.cat([took, live.remove_facts(h[3:], r[3:], t[3:])])     # a call larger than the whole capacity: folded at once
    assert not live.delta.edited
    whole = rspmm.GraphDelta(data, 8)
    whole.add(7, 0, 9)
    assert torch.equal(whole.remove(h, r, t), took)
    mat = whole.materialize(data)
    assert torch.equal(live.data.edge_index, mat.edge_index) and torch.equal(live.data.edge_type, mat.edge_type)
    live.compact()                                                       # nothing held: a no-op
    fresh = predict.Predictor(model, mat, k=5, batch_size=4)
    qh, qt, qr = data.target_triples[:5].unbind(-1)
    assert same_answers(live.tails(qh, qr), fresh.tails(qh, qr))
    # compact() folds tombstones that are held
    held = predict.Predictor(model, data, k=5, batch_size=4, delta_capacity=4)
    held.remove_facts(h[:2], r[:2], t[:2])
    two = rspmm.GraphDelta(data, 4)
    two.remove(h[:2], r[:2], t[:2])
    held.compact()
    assert not held.delta.edited and torch.equal(held.data.edge_index, two.materialize(data).edge_index)
    assert torch.equal(held.data.relation_graph.edge_index, two.materialize(data).relation_graph.edge_index)


def test_the_entry_validates_on_the_host():
    """ultra_rspmm_edit_rows answers before anything is launched (host tensors here): ULTRA_ERR_INVALID for bad arguments,
    ULTRA_ERR_UNSUPPORTED for general-walk plans, rotate messages and rows that are no whole 16-byte chunks, ULTRA_OK where
    there is nothing to do."""
    lib = _lib.lib
    data, delta, _ = edited_delta()
    exact = rspmm.Plan(data.edge_index, data.edge_type, 6, 4, exact_order=True)
    loose = rspmm.Plan(data.edge_index, data.edge_type, 6, 4, exact_order=False)
    x, rel, out = torch.zeros(2, 6, 64), torch.zeros(2, 4, 64), torch.zeros(2, 6, 64)
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, out)]
    operand, removed = ctypes.byref(delta.operand()), ctypes.byref(delta.removed_operand())

    def call(plan=exact, sum=0, mul=0, dtype=_lib.F32, relation=mats[0], input=mats[1], boundary=None, rows=None, output=mats[2],
             operand=operand, removed=removed):
        return lib.ultra_rspmm_edit_rows(plan._h if plan is not None else None, sum, mul, dtype, relation, input, boundary, rows,
                                         output, operand, removed, None)
    assert call(plan=None) == _lib.ULTRA_ERR_INVALID and b"ultra_rspmm_edit_rows" in lib.ultra_last_error()
    assert call(sum=3) == _lib.ULTRA_ERR_INVALID and call(mul=5) == _lib.ULTRA_ERR_INVALID and call(dtype=7) == _lib.ULTRA_ERR_INVALID
    assert call(output=None) == _lib.ULTRA_ERR_INVALID and call(operand=None) == _lib.ULTRA_ERR_INVALID
    assert call(rows=torch.zeros(2, dtype=torch.long).data_ptr()) == _lib.ULTRA_ERR_INVALID      # point rows without values
    # the tombstones: NULL arrays, a negative capacity
    keys = delta.removed_operand()
    no_ptr = _lib.UltraTombstones(None, keys.col_dev, keys.type_dev, keys.capacity_keys)
    no_col = _lib.UltraTombstones(keys.ptr_dev, None, keys.type_dev, keys.capacity_keys)
    no_type = _lib.UltraTombstones(keys.ptr_dev, keys.col_dev, None, keys.capacity_keys)
    negative = _lib.UltraTombstones(keys.ptr_dev, keys.col_dev, keys.type_dev, -1)
    for bad in (no_ptr, no_col, no_type, negative):
        assert call(removed=ctypes.byref(bad)) == _lib.ULTRA_ERR_INVALID and b"removed" in lib.ultra_last_error()
    rows = delta.operand()
    negative_rows = _lib.UltraDelta(rows.row_dev, rows.ptr_dev, rows.col_dev, rows.type_dev, rows.count_dev, -1, rows.capacity_edges)
    assert call(operand=ctypes.byref(negative_rows)) == _lib.ULTRA_ERR_INVALID
    assert call(plan=loose) == _lib.ULTRA_ERR_UNSUPPORTED
    assert call(mul=_lib.MUL_CODES["rotate"]) == _lib.ULTRA_ERR_UNSUPPORTED
    odd = [ctypes.byref(rspmm.as_mat(torch.zeros(2, n, 6))[1]) for n in (4, 6, 6)]
    assert call(relation=odd[0], input=odd[1], output=odd[2]) == _lib.ULTRA_ERR_UNSUPPORTED
    empty = ctypes.byref(rspmm.UltraMat(out.data_ptr(), 0, 0, 6, 64, 64))
    assert call(output=empty) == _lib.ULTRA_OK                                                   # n_outer == 0
    none = _lib.UltraDelta(None, None, None, None, None, 0, 0)
    assert call(operand=ctypes.byref(none)) == _lib.ULTRA_OK                                     # capacity 0
    # removed == NULL is ultra_rspmm_delta_rows, checks and messages included
    assert call(removed=None, plan=None) == _lib.ULTRA_ERR_INVALID and b"ultra_rspmm_delta_rows" in lib.ultra_last_error()
    assert call(removed=None, plan=loose) == _lib.ULTRA_ERR_UNSUPPORTED
    # Plan.edit_rows: None where the plan is not a reference-order one, before any operand is looked at
    assert loose.edit_rows(rel, x, out, delta) is None
    assert lib.ultra_abi_version() == 7
