"""What-if logical queries, the parts that need no GPU: the argument rules of QueryPredictor.answers(assuming=), the
traversal layout of rspmm.AssumedFacts on a hand-written case, the declaration and the host-side checks of
ultra_symbolic_traversal_edit_rows_owned, and the predictor on CPU tensors -- the stub projections of tests/test_query_live_cpu.py,
where a what-if call runs the per-query loop -- against query_predict.assume_reference: isolation within a batch, nothing stated,
and an assumed 1p tail left out for its own query alone."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_query_live_cpu import N, R, edge_list_model, twelve_node_graph
from ultra_amd import _lib, query_exec, query_predict, rspmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ultra_symbolic_traversal_edit_rows_owned"


def same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want))


def edited_predictor(**kwargs):
    kwargs.setdefault("k", 5)
    qp = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), batch_size=2, delta_capacity=4, **kwargs)
    qp.add_facts(8, 1, 3)
    qp.remove_facts(0, 0, 1)
    return qp


QUERIES = [(0, (0,)), (2, (0, 1)), (0, (0,)), ((5, (1,)), (6, (1,))), (9, (1, 0)), (7, (0, -2))]


def assumptions():
    """One entry per query of QUERIES: query 0 assumes a tail of its own and a fact elsewhere; query 2 -- the same query --
    nothing; 1 a first hop; 3 an empty tensor; 4 a duplicate pair; 5 a list of tuples."""
    return [torch.tensor([[0, 0, 8], [10, 1, 2]]), [(1, 1, 8)], None, torch.zeros(0, 3, dtype=torch.long),
            torch.tensor([[9, 1, 4], [9, 1, 4]]), [(7, 0, 3)]]


# ---- argument errors ----
def test_argument_errors():
    qp = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), k=5, batch_size=2, entity_capacity=2,
                                      assume_capacity=2)
    queries = QUERIES[:2]
    ran = [len(stub.graphs) for stub in (qp.model.model, qp.model.symbolic_model)]
    for ask in (qp.answers, lambda q, assuming: qp.answer_sets(q, 0.5, assuming=assuming)):
        with pytest.raises(ValueError, match="one entry per query"):
            ask(queries, assuming=[None])                                     # the entry count
        with pytest.raises(ValueError, match=r"\(m, 3\)"):
            ask(queries, assuming=torch.tensor([[1, 0]]))                     # the shape
        with pytest.raises(ValueError, match="assume_capacity"):
            ask(queries, assuming=torch.tensor([[1, 0, 2], [1, 0, 3], [1, 0, 4]]))
        with pytest.raises(ValueError, match="direct"):
            ask(queries, assuming=[None, [(1, R // 2, 2)]])                   # an inverse relation
        with pytest.raises(ValueError, match="existing entities"):
            ask(queries, assuming=torch.tensor([[1, 0, N]]))                  # an id in the reserve
        with pytest.raises(ValueError):
            ask(queries, assuming="facts")
    qp.retire_entities([5])
    with pytest.raises(ValueError, match="retired"):
        qp.answers(queries, assuming=[[(5, 0, 1)], None])                     # a retired id
    assert ran == [len(stub.graphs) for stub in (qp.model.model, qp.model.symbolic_model)], "nothing has run by then"
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="assume_capacity"):
            query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), assume_capacity=bad)
    assert query_predict.QueryPredictor(edge_list_model(), twelve_node_graph()).assume_capacity == 8
    with pytest.raises(ValueError, match="direct"):
        query_predict.assume_reference(edge_list_model(), twelve_node_graph(), queries, torch.tensor([[1, R // 2, 2]]))
    assert not query_predict.assume_supported(edge_list_model())


# ---- the overlay's traversal layout ----
def test_the_traversal_layout_on_a_hand_written_case():
    data = twelve_node_graph()
    delta = rspmm.GraphDelta(data, capacity=5)
    delta.add([8, 2], [1, 0], [3, 1])                   # shared: (8, 1, 3) and (2, 0, 1)
    delta.remove(0, 0, 1)                               # dead keys (0 -> 1, 0) at tail 1 and (1 -> 0, 2) at tail 0
    delta.remove(3, 0, 4)                               # stated as its direct edge only: ONE key, at tail 4 -- touched by it alone
    overlay = rspmm.AssumedFacts(data, delta, batch_size=3, per_query=2)
    assert overlay.traversal is None                    # laid out when first asked for
    operand = overlay.traversal_operand()
    lay = overlay.traversal
    cap = 2 * (5 + 3 * 2)
    assert [t.numel() for t in lay] == [cap, 1, cap + 1, cap, cap, cap, cap + 1] and all(t.dtype == torch.int32 for t in lay)
    assert lay.owner is overlay.traversal_owner
    pinned = [t.data_ptr() for t in lay]
    # query 0: (5, 0, 1) -- one more edge of relation 0 into tail 1 -- and (0, 0, 1), the retracted base fact assumed again;
    # query 1: nothing; query 2: (5, 0, 1) too and (6, 1, 10) into tails no other edit touches
    assert overlay.fill([[(5, 0, 1), (0, 0, 1)], None, torch.tensor([[5, 0, 1], [6, 1, 10]])]) == 4 + 4 + 4
    assert pinned == [t.data_ptr() for t in overlay.traversal], "fill() keeps the traversal view current in place"
    # brute force: (src, dst, type, owner) in insertion order -- shared direct, shared inverse, then per query direct, inverse
    edges = [(8, 3, 1, -1), (2, 1, 0, -1), (3, 8, 3, -1), (1, 2, 2, -1),
             (5, 1, 0, 0), (0, 1, 0, 0), (1, 5, 2, 0), (1, 0, 2, 0),
             (5, 1, 0, 2), (6, 10, 1, 2), (1, 5, 2, 2), (10, 6, 3, 2)]
    order = sorted(range(len(edges)), key=lambda e: (edges[e][1], edges[e][2], edges[e][0], e))
    key_tails = {0, 1, 4}
    touched = sorted({e[1] for e in edges} | key_tails)
    count = int(lay.count)
    assert touched == [0, 1, 2, 3, 4, 5, 6, 8, 10] and count == 9 and lay.rows[:count].tolist() == touched
    assert lay.add_src[:12].tolist() == [edges[e][0] for e in order]
    assert lay.add_type[:12].tolist() == [edges[e][2] for e in order]
    assert lay.owner[:12].tolist() == [edges[e][3] for e in order]
    add_ptr = lay.add_ptr[:count + 1].tolist()
    assert add_ptr == [0, 1, 5, 6, 7, 7, 9, 10, 11, 12]            # (tail 4: touched by a tombstone only, an empty range)
    # spelled out for tail 1, relation 0: sources 0, 2, 5, 5 with the owners carried along
    assert lay.add_src[add_ptr[1]:add_ptr[2]].tolist() == [0, 2, 5, 5] and lay.owner[add_ptr[1]:add_ptr[2]].tolist() == [0, -1, 0, 2]
    # the dead keys are the delta's own traversal arrays under THIS layout's (longer) tail list
    dead_ptr = lay.dead_ptr[:count + 1].tolist()
    assert dead_ptr == [0, 1, 2, 2, 2, 3, 3, 3, 3, 3]
    keys = delta.traversal
    assert (operand.dead_ptr_dev, operand.dead_src_dev, operand.dead_type_dev, operand.capacity_keys) == (
        lay.dead_ptr.data_ptr(), keys.dead_src.data_ptr(), keys.dead_type.data_ptr(), keys.dead_src.numel())
    assert (operand.row_dev, operand.count_dev, operand.add_ptr_dev, operand.add_src_dev, operand.add_type_dev) == (
        lay.rows.data_ptr(), lay.count.data_ptr(), lay.add_ptr.data_ptr(), lay.add_src.data_ptr(), lay.add_type.data_ptr())
    assert (operand.capacity_rows, operand.capacity_edges) == (cap, cap)
    dead = [(touched[k], int(keys.dead_src[j]), int(keys.dead_type[j])) for k in range(count) for j in range(dead_ptr[k], dead_ptr[k + 1])]
    assert dead == [(0, 1, 2), (1, 0, 0), (4, 3, 0)]
    assert int(delta.traversal.count) == 6 < count                  # the delta's own layout runs over fewer tails
    # the delta changes: the host list of keys is read again once, for the new version
    delta.remove(5, 1, 6)
    overlay.fill([None, [(3, 0, 4)], None])
    count = int(lay.count)
    rows, dead_ptr = lay.rows[:count].tolist(), lay.dead_ptr[:count + 1].tolist()
    assert rows == [0, 1, 2, 3, 4, 5, 6, 8] and dead_ptr[-1] == delta.num_removed == 5
    k4 = rows.index(4)
    assert lay.add_src[lay.add_ptr[k4]:lay.add_ptr[k4 + 1]].tolist() == [3] and lay.owner[int(lay.add_ptr[k4])] == 1
    assert (dead_ptr[k4], dead_ptr[k4 + 1]) == (2, 3) and (int(keys.dead_src[2]), int(keys.dead_type[2])) == (3, 0)
    # nothing was stated
    assert len(delta) == 2 and overlay.relation_graph is delta.relation_graph


def test_without_a_delta_the_dead_arrays_are_null():
    data = twelve_node_graph()
    overlay = rspmm.AssumedFacts(data, None, batch_size=2, per_query=1)
    overlay.fill([[(8, 1, 3)], None])
    operand = overlay.traversal_operand()
    assert operand.dead_ptr_dev is None and operand.dead_src_dev is None and operand.dead_type_dev is None
    assert operand.capacity_keys == 0 and operand.capacity_rows == operand.capacity_edges == 4
    lay = overlay.traversal
    assert int(lay.count) == 2 and lay.rows[:2].tolist() == [3, 8] and lay.add_ptr[:3].tolist() == [0, 1, 2]
    assert lay.add_src[:2].tolist() == [8, 3] and lay.add_type[:2].tolist() == [1, 3] and lay.owner[:2].tolist() == [0, 0]


# ---- the entry ----
def test_the_entry_is_declared_and_validates_on_the_host():
    lib = _lib.lib
    assert hasattr(lib, ENTRY) and lib.ultra_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ultra_nbfnet.h")).read()
    found = re.search(r"int32_t %s\(([^;]*)\);" % ENTRY, header)
    assert found, "the header declares the entry"
    assert [" ".join(a.split()) for a in found.group(1).split(",")] == [
        "const int64_t *row_ptr", "const int32_t *csr_src", "const int32_t *csr_type", "int64_t num_node",
        "const ultra_traversal_edits *edits", "const int32_t *owner_dev", "const int64_t *r_index", "int64_t batch", "int32_t dtype",
        "const void *h", "void *t", "void *stream"]
    data = twelve_node_graph()
    delta = rspmm.GraphDelta(data, capacity=4)
    delta.add(8, 1, 3)
    delta.remove(0, 0, 1)
    overlay = rspmm.AssumedFacts(data, delta, batch_size=2, per_query=2)
    overlay.fill([[(5, 0, 1)], None])
    edits = overlay.traversal_operand()
    row_ptr = torch.zeros(N + 1, dtype=torch.int64)
    src, kind = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    r_index = torch.zeros(2, dtype=torch.int64)
    h, t = torch.zeros(2, N), torch.zeros(2, N)
    default = dict(row_ptr=row_ptr.data_ptr(), src=src.data_ptr(), kind=kind.data_ptr(), num_node=N, edits=ctypes.byref(edits),
                   owner=overlay.traversal_owner.data_ptr(), r=r_index.data_ptr(), batch=2, dtype=_lib.F32, h=h.data_ptr(),
                   t=t.data_ptr())

    def call(**change):
        a = dict(default, **change)
        return getattr(lib, ENTRY)(a["row_ptr"], a["src"], a["kind"], a["num_node"], a["edits"], a["owner"], a["r"], a["batch"],
                                   a["dtype"], a["h"], a["t"], None)
    for name in ("row_ptr", "src", "kind", "edits", "owner", "r", "h", "t"):
        assert call(**{name: None}) == _lib.ULTRA_ERR_INVALID, name
        assert (ENTRY + ": ").encode() in lib.ultra_last_error()
    assert call(owner=None) == _lib.ULTRA_ERR_INVALID and b"owner_dev" in lib.ultra_last_error()
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
    # nothing to do: no row, no sample -- the owner array is still asked for
    assert call(edits=changed(capacity_rows=0)) == _lib.ULTRA_OK and call(batch=0) == _lib.ULTRA_OK
    assert call(edits=changed(capacity_rows=0), owner=None) == _lib.ULTRA_ERR_INVALID
    assert torch.equal(t, torch.zeros(2, N))


def test_an_overlay_is_served_in_lockstep_on_the_gpu_only():
    from ultra_amd import models
    data = twelve_node_graph()
    overlay = rspmm.AssumedFacts(data, None, batch_size=2, per_query=1)
    same_shape = query_exec.compile(query_predict.postfix_batch([(0, (0,)), (2, (0,))]), N, R)
    mixed = query_exec.compile(query_predict.postfix_batch([(0, (0,)), (2, (0, 1))]), N, R)
    assert query_exec.in_lockstep(same_shape) and not query_exec.in_lockstep(mixed)
    with pytest.raises(models.NotOnFusedPath):
        query_exec.execute(edge_list_model(), data, same_shape, delta=overlay)      # host tensors


# ---- the predictor on CPU tensors: the per-query loop ----
@pytest.mark.parametrize("filtered", [True, False])
def test_the_predictor_equals_the_reference(filtered):
    qp = edited_predictor(filtered=filtered)
    model = edge_list_model()
    got = qp.answers(QUERIES, assuming=assumptions())
    want = query_predict.assume_reference(model, qp.materialized(), QUERIES, assumptions(), k=5, filtered=filtered)
    assert same(got, want)
    assert not same(got, qp.answers(QUERIES))
    sets = qp.answer_sets(QUERIES, probability=0.45, assuming=assumptions())
    want = query_predict.assume_reference(model, qp.materialized(), QUERIES, assumptions(), filtered=filtered, probability=0.45)
    assert len(sets) == 4 and int(sets[0][-1]) > 0 and same(sets, want)
    # one tensor is assumed by every query; candidate sets follow their queries
    shared = torch.tensor([[0, 0, 8]])
    among = [torch.arange(q % 3, N, 2) for q in range(len(QUERIES))]
    got = qp.answers(QUERIES, among=among, assuming=shared)
    assert same(got, query_predict.assume_reference(model, qp.materialized(), QUERIES, [shared] * len(QUERIES), k=5,
                                                    filtered=filtered, among=among))
    # another logic, through the predictor's own
    godel = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), k=5, batch_size=2, logic="godel", filtered=filtered)
    assert same(godel.answers(QUERIES, assuming=assumptions()),
                query_predict.assume_reference(model, godel.materialized(), QUERIES, assumptions(), k=5, filtered=filtered,
                                               logic="godel"))
    assert model.logic == "product"


def test_a_reserve_and_a_retired_entity():
    qp = edited_predictor(entity_capacity=3)
    (new,) = qp.add_entities(1).tolist()
    qp.retire_entities([6])
    queries = [q for q in QUERIES if q != ((5, (1,)), (6, (1,)))] + [(new, (1,))]
    assumed = [[(new, 0, 1)], None, [(new, 0, 1), (2, 1, new)], None, [(new, 1, 4)], [(new, 1, 2)]]
    got = qp.answers(queries, assuming=assumed)
    mat = qp.materialized()
    assert int(mat.num_nodes) == N + 1 == qp.num_entities
    want = query_predict.assume_reference(edge_list_model(), mat, queries, assumed, k=5, retired=qp.retired_entities)
    assert same(got, want) and not bool((got[0] == 6).any()) and not bool((got[0] > new).any())
    with pytest.raises(ValueError, match="retired"):
        query_predict.assume_reference(edge_list_model(), mat, queries, [[(6, 0, 1)]] + [None] * 5, retired=qp.retired_entities)


def test_a_query_never_sees_its_neighbours_facts():
    qp = edited_predictor()
    assert QUERIES[0] == QUERIES[2] and qp.batches(QUERIES)[0] == [0, 2]      # the same query twice, in one batch
    got = qp.answers(QUERIES, assuming=assumptions())
    plain = qp.answers(QUERIES)
    for q in (2, 3):                # the queries that assume nothing: the call without the argument, bit for bit
        assert same([part[q:q + 1] for part in got], [part[q:q + 1] for part in plain])
    assert not same(got, plain), "the hypotheses change answers of the fixture"


def test_nothing_is_stated():
    qp = edited_predictor()
    state = lambda: (qp.materialized().edge_index.clone(), qp.materialized().edge_type.clone(), qp.delta.version, len(qp.delta),
                     qp.delta.num_removed, id(qp.delta), id(qp.graph))
    before = state()
    plain = qp.answers(QUERIES), qp.answer_sets(QUERIES, probability=0.45)
    qp.answers(QUERIES, assuming=assumptions())
    qp.answer_sets(QUERIES, probability=0.45, assuming=assumptions())
    after = state()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2:] == after[2:]
    assert same(qp.answers(QUERIES), plain[0]) and same(qp.answer_sets(QUERIES, probability=0.45), plain[1])
    # all-empty assumptions: exactly the call without the argument -- the projections see the graphs they see there
    for empty in ([None] * len(QUERIES), torch.zeros(0, 3, dtype=torch.long), [[]] * len(QUERIES)):
        assert same(qp.answers(QUERIES, assuming=empty), plain[0])
        assert same(qp.answer_sets(QUERIES, probability=0.45, assuming=empty), plain[1])
    # a never-edited predictor makes no delta for a hypothesis
    fresh = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), k=5, batch_size=2)
    fresh.answers(QUERIES, assuming=assumptions())
    assert fresh.delta is None and fresh.materialized() is fresh.graph


def test_an_assumed_tail_is_entailed_for_its_own_query_only():
    qp = query_predict.QueryPredictor(edge_list_model(), twelve_node_graph(), k=N, batch_size=2)
    queries = [(8, (0,)), (8, (0,)), (8, (0, 1))]                # node 8 has no edge
    ids, _, count = qp.answers(queries)
    assert count.tolist() == [N, N, N]
    got, _, got_count = qp.answers(queries, assuming=[[(8, 0, 5)], None, [(8, 0, 5)]])
    # 1p: the assumed tail 5 is entailed, for query 0 alone; 2p: what 5 reaches through relation 1 -- 6 -- is entailed through it
    assert got_count.tolist() == [N - 1, N, N - 1]
    assert 5 not in got[0, :N - 1].tolist() and 5 in got[1].tolist() and 6 not in got[2, :N - 1].tolist() and 5 in got[2].tolist()
    # a fact through another relation entails nothing for the query
    assert qp.answers(queries, assuming=[[(8, 1, 5)], None, None])[2].tolist() == [N, N, N]
