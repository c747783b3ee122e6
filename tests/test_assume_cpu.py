"""What-if queries, the parts that need no GPU: the argument rules of `assuming=`, the layout of rspmm.AssumedFacts on
a hand-written graph, the entry's declaration and host-side checks, and the Predictor on CPU tensors -- where a what-if call runs
the per-query loop -- against predict.assume_reference: equality, isolation within a batch, nothing stated, and the assumed
answer filtered for its own query alone."""
import ctypes
import os
import re

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def same_answers(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and torch.equal(got[2], want[2]))


def edge_state(graph):
    return graph.edge_index.clone(), graph.edge_type.clone()


# ---- the overlay's layout ----
def six_node_graph():
    """6 nodes, 2 direct relations (4 with inverses); node 5 has no edge."""
    h = torch.tensor([0, 0, 1, 2, 3])
    t = torch.tensor([1, 2, 2, 3, 4])
    r = torch.tensor([0, 1, 0, 1, 0])
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + 2]), num_nodes=6,
                num_relations=4)
    return tasks.build_relation_graph(data)


def test_the_overlay_layout_on_a_hand_written_case():
    data = six_node_graph()
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add([2, 0], [1, 0], [4, 3])                     # shared: (2, 1, 4) and (0, 0, 3)
    delta.remove(0, 1, 2)                                 # tombstones at rows 0 and 2
    overlay = rspmm.AssumedFacts(data, delta, batch_size=3, per_query=2)
    assert overlay.capacity == 4 + 3 * 2 and overlay.col.numel() == overlay.owner.numel() == overlay.rows.numel() == 20
    assert overlay.ptr.numel() == overlay.dead_ptr.numel() == 21 and int(overlay.count) == int(delta.count)
    addresses = [t.data_ptr() for t in (overlay.col, overlay.type, overlay.owner, overlay.rows, overlay.ptr, overlay.dead_ptr,
                                        overlay.count)]
    # query 0: (2, 0, 4) -- the shared edge's (row, col), stated again -- and (5, 1, 0) into the edge-less row; query 1: nothing;
    # query 2: (2, 1, 4) twice -- the shared FACT itself, two more parallel edges
    assert overlay.fill([[(2, 0, 4), (5, 1, 0)], None, torch.tensor([[2, 1, 4], [2, 1, 4]])]) == 4 + 4 + 4
    assert addresses == [t.data_ptr() for t in (overlay.col, overlay.type, overlay.owner, overlay.rows, overlay.ptr,
                                                overlay.dead_ptr, overlay.count)]
    # brute force: (row, col, type, owner) in insertion order -- shared direct, shared inverse, then per query direct, inverse
    edges = [(2, 4, 1, -1), (0, 3, 0, -1), (4, 2, 3, -1), (3, 0, 2, -1),
             (2, 4, 0, 0), (5, 0, 1, 0), (4, 2, 2, 0), (0, 5, 3, 0),
             (2, 4, 1, 2), (2, 4, 1, 2), (4, 2, 3, 2), (4, 2, 3, 2)]
    order = sorted(range(len(edges)), key=lambda e: (edges[e][0], edges[e][1], e))
    key_rows = {0, 2}
    touched = sorted({e[0] for e in edges} | key_rows)
    assert touched == [0, 2, 3, 4, 5] and int(overlay.count) == 5 and overlay.rows[:5].tolist() == touched
    ptr = overlay.ptr[:6].tolist()
    assert ptr == [0, 2, 6, 7, 11, 12]
    assert overlay.col[:12].tolist() == [edges[e][1] for e in order]
    assert overlay.type[:12].tolist() == [edges[e][2] for e in order]
    assert overlay.owner[:12].tolist() == [edges[e][3] for e in order]
    # spelled out for row 2 <- col 4: the shared edge first, then query 0's, then query 2's two
    assert overlay.owner[ptr[1]:ptr[2]].tolist() == [-1, 0, 2, 2] and overlay.type[ptr[1]:ptr[2]].tolist() == [1, 0, 1, 1]
    # ... and row 4 <- col 2 the same way through the inverse edges
    assert overlay.owner[ptr[3]:ptr[4]].tolist() == [-1, 0, 2, 2] and overlay.type[ptr[3]:ptr[4]].tolist() == [3, 2, 3, 3]
    # the live subsequence of every sample is the sorted row of its own graph
    for s in range(3):
        own = [(r, c, t) for r, c, t, o in edges if o in (-1, s)]
        live = [(touched[k], int(overlay.col[j]), int(overlay.type[j])) for k in range(5) for j in range(ptr[k], ptr[k + 1])
                if int(overlay.owner[j]) in (-1, s)]
        assert live == sorted(own, key=lambda e: (e[0], e[1], own.index(e)))
    # the tombstone keys are the delta's arrays under this layout's ranges
    dead = overlay.dead_ptr[:6].tolist()
    assert dead == [0, 1, 2, 2, 2, 2]
    removed = overlay.removed_operand()
    assert removed.col_dev == delta.dead_col.data_ptr() and removed.type_dev == delta.dead_type.data_ptr()
    assert removed.ptr_dev == overlay.dead_ptr.data_ptr() and removed.capacity_keys == delta.dead_col.numel()
    assert [(touched[k], int(delta.dead_col[dead[k]]), int(delta.dead_type[dead[k]])) for k in (0, 1)] == [(0, 2, 1), (2, 0, 3)]
    # refilled: the delta as it is now, other owners
    delta.add(1, 1, 5)
    assert overlay.fill([None, [(0, 0, 3)], None]) == 6 + 2
    assert overlay.rows[:int(overlay.count)].tolist() == [0, 1, 2, 3, 4, 5]
    k0 = overlay.ptr[:2].tolist()
    assert overlay.col[k0[0]:k0[1]].tolist() == [3, 3] and overlay.owner[k0[0]:k0[1]].tolist() == [-1, 1]
    # nothing was stated
    assert len(delta) == 3 and delta.num_removed == 2
    assert overlay.edited and overlay.num_removed == 2 and overlay.relation_graph is delta.relation_graph
    with pytest.raises(RuntimeError, match="per sample"):
        overlay.materialize(data)


def test_the_overlay_checks_its_entries():
    data = six_node_graph()
    overlay = rspmm.AssumedFacts(data, None, batch_size=2, per_query=1)
    assert overlay.capacity == 2 and overlay.num_removed == 0 and overlay.relation_graph is data.relation_graph
    assert overlay.removed_operand().capacity_keys == 0
    assert overlay.fill([[(0, 1, 5)], []]) == 2 and overlay.owner[:2].tolist() == [0, 0]
    with pytest.raises(ValueError, match="one entry"):
        overlay.fill([None])
    with pytest.raises(ValueError, match="at most 1"):
        overlay.fill([[(0, 1, 5), (0, 1, 4)], None])
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        overlay.fill([[(0, 1)], None])
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError):
            rspmm.AssumedFacts(data, None, batch_size=bad, per_query=1)
        with pytest.raises(ValueError):
            rspmm.AssumedFacts(data, None, batch_size=1, per_query=bad)


# ---- the entry ----
def test_the_symbol_is_exported_and_declared():
    lib = _lib.lib
    assert hasattr(lib, "ultra_rspmm_edit_rows_owned") and lib.ultra_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    found = re.search(r"int32_t ultra_rspmm_edit_rows_owned\(([^;]*)\);", header)
    assert found, "the header declares the entry"
    args = [" ".join(a.split()) for a in found.group(1).split(",")]
    assert args == ["ultra_plan *plan", "int32_t sum", "int32_t mul", "int32_t dtype", "const ultra_mat *relation",
                    "const ultra_mat *input", "const ultra_mat *boundary", "const int64_t *point_rows_dev",
                    "const ultra_mat *output", "const ultra_delta *delta", "const int32_t *owner_dev",
                    "const ultra_tombstones *removed", "int64_t hub_len", "void *stream"]


def test_the_entry_validates_on_the_host():
    """The checks of ultra_rspmm_edit_rows_split, before anything is launched (host tensors here), plus the owner array."""
    lib = _lib.lib
    data = six_node_graph()
    n, r = 6, 4
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add(2, 1, 4)
    delta.remove(0, 1, 2)
    overlay = rspmm.AssumedFacts(data, delta, batch_size=2, per_query=2)
    overlay.fill([[(5, 1, 0)], None])
    exact = rspmm.Plan(data.edge_index, data.edge_type, n, r, exact_order=True)
    loose = rspmm.Plan(data.edge_index, data.edge_type, n, r, exact_order=False)
    x, rel, out = torch.zeros(2, n, 64), torch.zeros(2, r, 64), torch.zeros(2, n, 64)
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, out)]
    operand, removed = ctypes.byref(overlay.operand()), ctypes.byref(overlay.removed_operand())

    def call(plan=exact, sum=0, mul=0, dtype=_lib.F32, relation=mats[0], input=mats[1], boundary=None, rows=None, output=mats[2],
             operand=operand, owner=overlay.owner.data_ptr(), removed=removed, hub_len=-1):
        return lib.ultra_rspmm_edit_rows_owned(plan._h if plan is not None else None, sum, mul, dtype, relation, input, boundary,
                                               rows, output, operand, owner, removed, hub_len, None)

    def invalid(**kw):
        return call(**kw) == _lib.ULTRA_ERR_INVALID and b"ultra_rspmm_edit_rows_owned: " in lib.ultra_last_error()

    assert invalid(plan=None) and invalid(sum=3) and invalid(mul=5) and invalid(dtype=7)
    assert invalid(output=None) and invalid(operand=None) and invalid(relation=None) and invalid(input=None)
    assert invalid(owner=None) and b"owner_dev" in lib.ultra_last_error()
    assert invalid(rows=torch.zeros(2, dtype=torch.long).data_ptr())
    for hub_len in (-1, 0, 16, 1 << 40):
        assert call(plan=loose, hub_len=hub_len) == _lib.ULTRA_ERR_UNSUPPORTED
        assert call(mul=_lib.MUL_CODES["rotate"], hub_len=hub_len) == _lib.ULTRA_ERR_UNSUPPORTED
    empty = ctypes.byref(rspmm.UltraMat(out.data_ptr(), 0, 0, n, 64, 64))
    assert call(output=empty) == _lib.ULTRA_OK                                                    # n_outer == 0
    assert call(operand=ctypes.byref(_lib.UltraDelta(None, None, None, None, None, 0, 0)), owner=None) == _lib.ULTRA_OK
    # the plan method: host tensors are refused the way edit_rows_split refuses them, a general-walk plan serves nothing
    assert loose.edit_rows_owned(rel, x, out, overlay) is None
    with pytest.raises(RuntimeError, match="expected a GPU"):
        exact.edit_rows_owned(rel, x, out, overlay)


# ---- the Predictor on CPU tensors ----
@pytest.fixture(scope="module")
def served():
    # (RotatE messages: the layers that run on CPU tensors; such a model is outside assume_supported on any device, so this is
    # the per-query route)
    torch.manual_seed(7)
    model = models.Ultra(**synthetic.default_model_cfg(message_func="rotate")).eval()
    data = synthetic.make_kg(num_node=40, num_triple=150, num_relation_base=4, seed=11)
    return model, data


def make_predictor(served, **kwargs):
    model, data = served
    live = predict.Predictor(model, data, k=6, batch_size=3, delta_capacity=8, **kwargs)
    h, t, r = data.target_triples[:2].unbind(-1)
    live.add_facts([1, 2], [0, 1], [3, 1])
    live.remove_facts(h[:1], r[:1], t[:1])
    return live


def queries(data):
    h, t, r = data.target_triples[2:7].unbind(-1)
    # queries 0 and 1 ask the same (h, r)
    return torch.cat([h[:1], h]), torch.cat([r[:1], r]), torch.cat([t[:1], t])


def assumptions(h, r):
    """One entry per query of `queries`: query 0 assumes a fact at its own anchor and one elsewhere; 1 nothing; 2 a duplicate
    pair; 3 an empty tensor; 4 a self loop; 5 a list of tuples."""
    a = int(h[0])
    return [torch.tensor([[a, int(r[0]), 17], [20, 1, 21]]), None, torch.tensor([[5, 2, 6], [5, 2, 6]]),
            torch.zeros(0, 3, dtype=torch.long), torch.tensor([[9, 3, 9]]), [(int(h[5]), 0, 30), (31, 0, int(h[5]))]]


def test_support_is_what_the_layers_are(served):
    model, _ = served
    assert not predict.assume_supported(model)
    assert predict.assume_supported(models.Ultra(**synthetic.default_model_cfg()))
    for aggr, msg in (("mean", "distmult"), ("pna", "distmult"), ("sum", "rotate")):
        assert not predict.assume_supported(models.Ultra(**synthetic.default_model_cfg(aggregate_func=aggr, message_func=msg)))
    for aggr, msg in (("max", "transe"), ("min", "distmult")):
        assert predict.assume_supported(models.Ultra(**synthetic.default_model_cfg(aggregate_func=aggr, message_func=msg)))
    assert not predict.assume_supported(lambda data, batch: None)


def test_argument_errors(served):
    model, data = served
    live = predict.Predictor(model, data, k=6, batch_size=3, entity_capacity=2, assume_capacity=2)
    h, r = torch.tensor([1, 2]), torch.tensor([0, 1])
    direct = data.num_relations // 2
    with pytest.raises(ValueError, match="direct"):
        live.tails(h, r, assuming=torch.tensor([[1, direct, 2]]))                 # an inverse relation
    with pytest.raises(ValueError, match="existing entities"):
        live.tails(h, r, assuming=torch.tensor([[1, 0, data.num_nodes]]))         # an id in the reserve
    with pytest.raises(ValueError, match="existing entities"):
        live.heads(h, r, assuming=[None, [(data.num_nodes + 5, 0, 1)]])           # an id beyond the slots
    with pytest.raises(ValueError, match="assume_capacity"):
        live.tails(h, r, assuming=torch.tensor([[1, 0, 2], [1, 0, 3], [1, 0, 4]]))
    with pytest.raises(ValueError, match="one entry per query"):
        live.tails(h, r, assuming=[None])                                         # a wrong list length
    with pytest.raises(ValueError, match="one entry per query"):
        live.tails_above(h, r, 0.0, assuming=[None, None, None])
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        live.tails(h, r, assuming=torch.tensor([[1, 0]]))
    with pytest.raises(ValueError):
        live.tails(h, r, assuming="facts")
    live.remove_entities([5])
    with pytest.raises(ValueError, match="retired"):
        live.tails(h, r, assuming=[[(5, 0, 1)], None])                            # a retired id
    with pytest.raises(ValueError, match="retired"):
        live.heads_above(h, r, 0.0, assuming=torch.tensor([[1, 0, 5]]))
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="assume_capacity"):
            predict.Predictor(model, data, assume_capacity=bad)
    assert predict.Predictor(model, data).assume_capacity == 8
    with pytest.raises(ValueError, match="direct"):
        predict.assume_reference(model, data, data, h, r, torch.tensor([[1, direct, 2]]))


def test_ids_are_bounded_without_a_reserve_too(served):
    """A predictor WITHOUT an entity reserve: an id at or beyond num_nodes and a negative id are ValueErrors in the list form and in
    the single-tensor form, for heads and tails of a fact, in every call and in the reference -- before any forward runs and before
    an id can reach another query's known-answer keys (`sample * n + id`)."""
    model, data = served
    n = int(data.num_nodes)
    live = predict.Predictor(model, data, k=6, batch_size=3)
    assert not live.entity_capacity
    h, r = torch.tensor([1, 2]), torch.tensor([0, 1])
    for bad in ((1, 0, n), (n, 0, 1), (2, 1, -1), (-1, 1, 2), (1, 0, n + 3)):
        for assuming in ([None, [bad]], [[bad], None], torch.tensor([bad])):
            for ask in (live.tails, live.heads):
                with pytest.raises(ValueError, match="existing entities"):
                    ask(h, r, assuming=assuming)
            for ask in (live.tails_above, live.heads_above):
                with pytest.raises(ValueError, match="existing entities"):
                    ask(h, r, 0.0, assuming=assuming)
            with pytest.raises(ValueError, match="existing entities"):
                predict.assume_reference(model, data, data, h, r, assuming)
            with pytest.raises(ValueError, match="existing entities"):
                predict._assumed_lists(data, assuming, 2)
    # the ids at the edges of the range are fine
    live.tails(h, r, assuming=[[(0, 0, n - 1)], [(n - 1, 1, 0)]])
    assert not live.delta.edited


@pytest.mark.parametrize("mode", ["tail", "head"])
def test_the_predictor_equals_the_reference(served, mode):
    model, data = served
    live = make_predictor(served)
    h, r, t = queries(data)
    anchor = h if mode == "tail" else t
    assumed = assumptions(anchor, r)
    got = (live.tails if mode == "tail" else live.heads)(anchor, r, assuming=assumed)
    want = predict.assume_reference(model, live.materialized(), live.filter_graph, anchor, r, assumed, k=6, mode=mode)
    assert same_answers(got, want)
    plain = (live.tails if mode == "tail" else live.heads)(anchor, r)
    assert not same_answers(got, plain)
    # one tensor is assumed by every query
    shared = torch.tensor([[int(anchor[0]), int(r[0]), 17]])
    got = (live.tails if mode == "tail" else live.heads)(anchor, r, assuming=shared)
    assert same_answers(got, predict.assume_reference(model, live.materialized(), live.filter_graph, anchor, r,
                                                      [shared] * len(anchor), k=6, mode=mode))


def test_the_answer_sets_equal_the_reference(served):
    model, data = served
    live = make_predictor(served)
    h, r, _ = queries(data)
    assumed = assumptions(h, r)
    floor = -1.0
    got = live.tails_above(h, r, floor, assuming=assumed)
    want = predict.assume_reference(model, live.materialized(), live.filter_graph, h, r, assumed, mode="tail", min_score=floor)
    assert len(got) == len(want) == 4 and int(got[0][-1]) > 0
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert not torch.equal(got[2], live.tails_above(h, r, floor)[2])


def test_candidate_sets_and_assumptions_together(served):
    model, data = served
    live = make_predictor(served)
    h, r, t = queries(data)
    n = int(data.num_nodes)
    sets = [torch.arange(q, n, 2 + q) for q in range(len(h))]
    mat = live.materialized()
    for mode, anchor, ask in (("tail", h, live.tails), ("head", t, live.heads)):
        assumed = assumptions(anchor, r)
        got = ask(anchor, r, among=sets, assuming=assumed)
        assert same_answers(got, predict.assume_reference(model, mat, live.filter_graph, anchor, r, assumed, k=6, mode=mode, among=sets))
        assert not same_answers(got, ask(anchor, r, among=sets))
    assumed = assumptions(t, r)
    got = live.heads_above(t, r, -0.5, among=sets, assuming=assumed)
    want = predict.assume_reference(model, mat, live.filter_graph, t, r, assumed, mode="head", min_score=-0.5, among=sets)
    assert int(got[0][-1]) > 0 and all(torch.equal(a, b) for a, b in zip(got, want))


def test_a_query_never_sees_its_neighbours_facts(served):
    model, data = served
    live = make_predictor(served)
    h, r, _ = queries(data)
    assert int(h[0]) == int(h[1]) and int(r[0]) == int(r[1])
    assumed = assumptions(h, r)
    got = live.tails(h, r, assuming=assumed)
    plain = live.tails(h, r)
    for q in (1, 3):                # the queries that assume nothing: the call without the argument, bit for bit
        assert same_answers([part[q:q + 1] for part in got], [part[q:q + 1] for part in plain])
    assert not torch.equal(got[1][0], plain[1][0])


def test_nothing_is_stated(served):
    model, data = served
    live = make_predictor(served)
    h, r, t = queries(data)
    before = (edge_state(live.materialized()), edge_state(live.filter_graph), live.delta.edited, len(live.delta),
              live.delta.num_removed, live.delta.version, live.delta)
    plain = live.tails(h, r), live.heads(t, r)
    live.tails(h, r, assuming=assumptions(h, r))
    live.heads(t, r, assuming=assumptions(t, r))
    live.tails_above(h, r, 0.0, assuming=assumptions(h, r))
    after = (edge_state(live.materialized()), edge_state(live.filter_graph), live.delta.edited, len(live.delta),
             live.delta.num_removed, live.delta.version, live.delta)
    for (a_index, a_type), (b_index, b_type) in zip(before[:2], after[:2]):
        assert torch.equal(a_index, b_index) and torch.equal(a_type, b_type)
    assert before[2:6] == after[2:6] and before[6] is after[6]
    assert same_answers(live.tails(h, r), plain[0]) and same_answers(live.heads(t, r), plain[1])
    # all-empty assumptions: the call without the argument
    for empty in ([None] * len(h), torch.zeros(0, 3, dtype=torch.long), [[]] * len(h)):
        assert same_answers(live.tails(h, r, assuming=empty), plain[0])


def test_an_assumed_tail_is_known_for_its_own_query_only(served):
    model, data = served
    live = predict.Predictor(model, data, k=data.num_nodes, batch_size=3)
    h, r, _ = queries(data)
    h, r = h[:2], r[:2]
    ids, _, count = live.tails(h, r)
    fresh = int(ids[0, 0])                                  # the best tail of the shared (h, r) that is no known answer
    got, _, got_count = live.tails(h, r, assuming=[[(int(h[0]), int(r[0]), fresh)], None])
    assert fresh not in got[0, :int(got_count[0])].tolist() and int(got_count[0]) == int(count[0]) - 1
    assert fresh in got[1, :int(got_count[1])].tolist() and int(got_count[1]) == int(count[1])
    # ... and an assumed head likewise
    t = torch.tensor([fresh, fresh])
    heads, _, heads_count = live.heads(t, r, assuming=[None, [(int(h[0]), int(r[0]), fresh)]])
    assert int(h[0]) in heads[0, :int(heads_count[0])].tolist() or int(h[0]) in predict.known_answers(
        live.filter_graph, t[:1], r[:1], "head")[1].tolist()
    assert int(h[0]) not in heads[1, :int(heads_count[1])].tolist()
    # a fact that names another (h, r) is no known answer of the query
    other = live.tails(h, r, assuming=[[(int(h[0]), (int(r[0]) + 1) % (data.num_relations // 2), fresh)], None])
    assert int(other[2][0]) == int(count[0])
