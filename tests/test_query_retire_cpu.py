"""Retiring entities under logical queries, the parts that need no GPU: the ultra_nonzero_lists_alive symbol and its
argument checks, which answer before any GPU call; the `retired` operand of query_exec.nonzero_lists and query_exec.compile;
QueryPredictor.retire_entities on the stub projections of tests/test_query_live_cpu.py, which run on host tensors.

THE DEFINITION every result is compared with (`definition` below; the GPU tests import it): a fresh QueryPredictor on
qp.materialized() -- the copy keeps the id space, the retired ids are isolated nodes of it -- with the retired ids taken out of
the candidates and out of the entailed lists.
  answers       the fresh predictor is asked for k + num_retired answers; the retired ids are dropped from every row and the
                first k kept: ids equal, scores bit for bit; count = min(k, num_entities - num_retired - |entailed alive ids|).
  answer_sets   predict.filtered_above_reference(fresh logits, threshold, ptr, known, retired=retired_entities), `known` the
                non-zero alive ids of the fresh symbolic sets; `size` never counts a retired id.

Scores: without a reserve the served graph and the materialised one have the same row length, so every comparison is bit for bit.
With a reserve the rows differ in length (N + M slots against num_entities) and torch's CPU sigmoid -- the stub's neural side --
takes its vector path or its scalar one by an element's position in its row, one ulp apart (tests/test_query_grow_cpu.py), so the
scores are compared with tests/test_grow_cpu.py's SCORE_TOL = 1e-5 and its reasoning: a probability moves in its last bits
(2^-24 ~ 6e-8), the logit's slope 1 / (p (1 - p)) is below 30 for the stub's p in [0.11, 0.97], a product of up to three such
factors triples it -- a few 1e-6 -- and 1e-5 is asked; ids, counts, offsets and sizes are compared exactly.  The same run on
tests/test_query_grow_cpu.py's ExactStub, whose arithmetic is rounded per element whatever the row length, is bit for bit."""
import os

import pytest
import torch

from tests.test_query_exec_cpu import load  # noqa: F401  (the golden queries, through folded_queries)
from tests.test_query_grow_cpu import edge_list_model as exact_model
from tests.test_query_grow_cpu import ends_in_negation, folded_queries
from tests.test_query_live_cpu import N, edge_list_model, twelve_node_graph
from ultra_amd import _lib, predict, query_exec, query_predict
from ultra_amd.live import retired_words
from ultra_amd.ultraquery import Query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, TWIN, PARENT = "ultra_nonzero_lists_alive", "ultra_nonzero_lists_live", "ultra_nonzero_lists"
SCORE_TOL = 1e-5        # (tests/test_grow_cpu.py's; the module docstring)
K = 5
PROBABILITY = 0.45


# ---- the definition ----
def postfix(qp, queries):
    """(n, L) int64 postfix rows of `queries` (nested tuples, lists or rows), padded with stop."""
    rows = qp._rows(queries)
    width = max(len(row) for row in rows)
    return torch.tensor([row + [Query.stop] * (width - len(row)) for row in rows], dtype=torch.long)


def definition(qp, queries, model, probability=PROBABILITY):
    """((ids, scores, count), (ptr, ids, scores, size)) as the module docstring defines them, from a fresh predictor on
    qp.materialized() under `model` (the served model, or an equal one that holds no state of the served predictor)."""
    mat = qp.materialized()
    retired = qp.retired_entities
    assert int(mat.num_nodes) == qp.num_entities
    if qp.num_retired:
        assert torch.equal(mat.retired_entities, retired), "the copy names the retired ids"
    dev = mat.edge_index.device
    rows = postfix(qp, queries)
    k, n = qp.k, len(rows)
    fresh = query_predict.QueryPredictor(model, mat, k=k + qp.num_retired, batch_size=qp.batch_size, filtered=qp.filtered,
                                         logic=qp.logic)
    assert fresh.num_retired == 0 and fresh.batches(rows) == qp.batches(rows)
    # answers: k + num_retired of the fresh predictor, the retired ids dropped, the first k kept
    ids, scores, _ = fresh.answers(rows)
    gone = torch.isin(ids, retired)
    order = torch.argsort(gone.to(torch.int8), dim=1, stable=True)[:, :k]
    assert not bool(gone.gather(1, order).any())
    ids, scores = ids.gather(1, order), scores.gather(1, order)
    # the fresh logits and symbolic sets, batch by batch as the predictors run them
    threshold = predict.logit_threshold(probability)
    count = torch.zeros(n, dtype=torch.long, device=dev)
    size = torch.zeros(n, dtype=torch.long, device=dev)
    lists = [None] * n
    was, logic = model.training, model.logic
    model.eval()
    if qp.logic is not None:
        model.logic = qp.logic
    try:
        with torch.no_grad():
            for index in fresh.batches(rows):
                logits, sym = query_exec.execute(model, mat, rows[index], symbolic_traversal=qp.filtered)
                ptr = known = None
                entailed = torch.zeros(len(index), dtype=torch.long, device=dev)
                if qp.filtered:
                    listed = sym != 0
                    listed[:, retired] = False
                    sample, known = listed.nonzero().t()
                    ptr = torch.searchsorted(sample.contiguous(), torch.arange(len(index) + 1, device=dev))
                    entailed = listed.sum(dim=1)
                b_ptr, b_ids, b_scores, b_size = predict.filtered_above_reference(logits, threshold, ptr, known, retired=retired)
                where = torch.tensor(index, dtype=torch.long, device=dev)
                count[where] = (qp.num_entities - qp.num_retired - entailed).clamp(max=k)
                size[where] = b_size
                for j, i in enumerate(index):
                    lists[i] = (b_ids[int(b_ptr[j]):int(b_ptr[j + 1])], b_scores[int(b_ptr[j]):int(b_ptr[j + 1])])
    finally:
        model.train(was)
        model.logic = logic
    out_ptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
    out_ptr[1:] = torch.tensor([len(a) for a, _ in lists], device=dev).cumsum(0)
    return (ids, scores, count), (out_ptr, torch.cat([a for a, _ in lists]), torch.cat([b for _, b in lists]), size)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def close(a, b):
    return a.shape == b.shape and torch.allclose(a, b, rtol=0.0, atol=SCORE_TOL, equal_nan=True)


def check_against_definition(qp, queries, model, scores=same_bits, what=""):
    """answers / answer_sets of `qp` against the definition: ids, counts, offsets and sizes exactly, the scores by `scores`; no
    retired id anywhere; the padding of a short row where the definition has it."""
    (ids, score, count), (ptr, set_ids, set_score, size) = want = definition(qp, queries, model)
    got = qp.answers(queries), qp.answer_sets(queries, probability=PROBABILITY)
    assert torch.equal(got[0][0], ids) and torch.equal(got[0][2], count), what
    assert scores(got[0][1], score), what
    assert torch.equal(got[1][0], ptr) and torch.equal(got[1][1], set_ids) and torch.equal(got[1][3], size), what
    assert scores(got[1][2], set_score), what
    retired = qp.retired_entities
    assert not bool(torch.isin(got[0][0], retired).any()) and not bool(torch.isin(got[1][1], retired).any()), what
    assert bool((got[0][0] >= 0).sum(dim=1).eq(count).all()), what
    assert int(size.max()) <= qp.num_entities - qp.num_retired, what
    return got, want


def reanchored(queries, retired):
    """`queries` (postfix rows) with every anchor that is one of `retired` moved to the next id that is not."""
    q = queries.clone()
    anchors = (q & Query.operation) == 0
    for v in sorted(retired):
        to = next(u for u in range(v + 1, v + N) if u % N not in retired) % N
        q[anchors & (q == v)] = to
    return q


def facts_at(graph, ids):
    """Per id the number of distinct direct triples of `graph` that name it, from the edge list in plain Python."""
    direct = int(graph.num_relations) // 2
    triples = set()
    for (u, v), kind in zip(graph.edge_index.t().tolist(), graph.edge_type.tolist()):
        triples.add((u, kind, v) if kind < direct else (v, kind - direct, u))
    return [sum(1 for h, _, t in triples if v in (h, t)) for v in ids]


# ---- the entry ----
def test_the_symbol_is_exported_and_declared():
    assert hasattr(_lib.lib, ENTRY)
    with open(os.path.join(ROOT, "include", "ultra_nbfnet.h")) as f:
        header = f.read()
    assert ("int32_t ultra_nonzero_lists_alive(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,\n"
            "                                  int64_t *index_out, int64_t capacity, const int64_t *n_live,\n"
            "                                  const uint32_t *retired_bits, void *stream);") in header
    assert _lib.lib.ultra_abi_version() == 7


def test_the_entry_validates_before_any_gpu_call():
    """On host tensors: a NULL bitmap is ULTRA_ERR_INVALID under the entry's own message, with a live count or without one; every
    other argument error is ultra_nonzero_lists' own, under this entry's name.  Nothing is launched."""
    lib = _lib.lib
    x = torch.zeros(2, 8)
    counts, ptr, index = (torch.ones(n, dtype=torch.int64) for n in (2, 3, 16))
    live = torch.tensor([8], dtype=torch.int64)
    bits = torch.zeros(1, dtype=torch.int32)
    default = dict(x=x.data_ptr(), batch=2, n=8, counts=counts.data_ptr(), ptr=ptr.data_ptr(), index=index.data_ptr(),
                   capacity=16, live=live.data_ptr(), bits=bits.data_ptr())

    def call(entry=ENTRY, **change):
        a = dict(default, **change)
        args = (a["x"], a["batch"], a["n"], a["counts"], a["ptr"], a["index"], a["capacity"])
        if entry == ENTRY:
            args += (a["live"], a["bits"])
        return getattr(lib, entry)(*(args + (None,)))

    for change in (dict(bits=None), dict(bits=None, live=None), dict(bits=None, batch=0)):
        assert call(**change) == _lib.ULTRA_ERR_INVALID, change
        assert lib.ultra_last_error() == b"ultra_nonzero_lists_alive: retired_bits is NULL", change
    for change in (dict(x=None), dict(counts=None), dict(ptr=None), dict(index=None), dict(batch=-1), dict(n=-1),
                   dict(capacity=15), dict(n=2 ** 31), dict(batch=2 ** 31, capacity=2 ** 62)):
        parent = call(PARENT, **change)
        assert parent in (_lib.ULTRA_ERR_INVALID, _lib.ULTRA_ERR_UNSUPPORTED), change
        parent_message = lib.ultra_last_error()
        for live_change in ({}, dict(live=None)):       # (n_live may be NULL here)
            assert call(**dict(change, **live_change)) == parent, change
            assert lib.ultra_last_error() == parent_message.replace(b"ultra_nonzero_lists:", b"ultra_nonzero_lists_alive:"), change
    assert torch.equal(ptr, torch.ones(3, dtype=torch.int64)) and torch.equal(index, torch.ones(16, dtype=torch.int64))
    assert torch.equal(counts, torch.ones(2, dtype=torch.int64))


def test_nonzero_lists_retired_argument_rules():
    x = torch.zeros(2, 40)
    bits = retired_words([3, 33], 40)
    assert bits.dtype == torch.int32 and bits.numel() == 2
    # no CPU path, with the bitmap or the pair: the RuntimeError of before
    for retired in (bits, (bits, torch.tensor([2])), bits.view(torch.uint32)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            query_exec.nonzero_lists(x, retired=retired)
        with pytest.raises(RuntimeError, match="no CPU path"):
            query_exec.nonzero_lists(x, num_live=36, retired=retired)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query_exec.nonzero_lists(x)
    # the operand's own rules: dtype, length, device, shape, and what is no bitmap at all
    for bad in (bits.long(), bits.float(), bits[:1], bits.to("meta"), bits.view(1, 2), (bits[:1], torch.tensor([2])),
                [3, 33], {3, 33}, 3, "bits", (bits, torch.tensor([2]), None)):
        with pytest.raises(ValueError, match="retired"):
            query_exec.nonzero_lists(x, retired=bad)


def test_compile_refuses_a_retired_anchor():
    P, S = Query.projection, Query.stop
    rows = torch.tensor([[4, P | 1, S, S, S, S], [2, P | 0, 7, P | 1, Query.intersection | 2, S]])
    assert query_exec.compile(rows, 10, 4).num_nodes == 10
    for retired in ({7}, [7, 9], torch.tensor([7]), frozenset([7])):
        with pytest.raises(ValueError, match=r"query 1: entity id 7 was retired"):
            query_exec.compile(rows, 10, 4, retired=retired)
        assert query_exec.compile(rows[:1], 10, 4, retired=retired).signature() == query_exec.compile(rows[:1], 10, 4).signature()
    # the same queries with other ids retired, and beside the live bound
    assert query_exec.compile(rows, 10, 4, retired={3, 5}).signature() == query_exec.compile(rows, 10, 4).signature()
    assert query_exec.compile(rows, 10, 4, retired=()).batch == 2
    with pytest.raises(ValueError, match=r"query 0: entity id 4 was retired"):
        query_exec.compile(rows, 12, 4, num_live=10, retired={4})
    with pytest.raises(ValueError, match=r"outside \[0, 7\)"):
        query_exec.compile(rows, 12, 4, num_live=7, retired={3})


# ---- QueryPredictor ----
def test_the_names():
    assert not hasattr(query_predict.QueryPredictor, "remove_entities")
    assert predict.Predictor.retire_entities is predict.Predictor.remove_entities
    assert callable(query_predict.QueryPredictor.retire_entities)


def test_retire_entities_arguments_and_counts():
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=K, batch_size=4)
    assert qp.num_retired == 0 and qp.retired_entities.numel() == 0 and qp.materialized() is graph
    for bad in (-1, N, [2, 2], [0, N + 3]):
        with pytest.raises(ValueError):
            qp.retire_entities(bad)
    assert qp.retire_entities([]).numel() == 0
    assert qp.num_retired == 0 and qp.delta is None and qp.graph is graph and qp.materialized() is graph
    # 8 has no edge; (3, 0, 4) is stated as its direct edge only, (10, 1, 11) as its inverse edge only; 1 is the hub
    want = facts_at(graph, [8, 3, 10, 1])
    assert want == [0, 1, 1, 4]
    got = qp.retire_entities(8)
    assert got.dtype == torch.long and got.tolist() == [0]
    assert qp.num_retired == 1 and qp.retired_entities.tolist() == [8] and qp.delta is None
    assert qp.retire_entities([3, 10]).tolist() == [1, 1]
    assert qp.retire_entities(torch.tensor([1])).tolist() == [4]
    assert qp.num_retired == 4 and qp.retired_entities.tolist() == [1, 3, 8, 10]
    assert qp.graph is graph and qp.delta.num_removed > 0, "the facts are tombstones beside the served graph"
    for again in (8, [0, 1]):
        with pytest.raises(ValueError):
            qp.retire_entities(again)
    assert qp.retired_entities.tolist() == [1, 3, 8, 10]
    # the copy keeps the id space and names the retired ids, also without a reserve
    mat = qp.materialized()
    assert int(mat.num_nodes) == N and mat.retired_entities.tolist() == [1, 3, 8, 10] and mat is not qp.materialized()
    assert facts_at(mat, [1, 3, 8, 10]) == [0, 0, 0, 0]
    # a fact between two ids of one call counts for both
    other = query_predict.QueryPredictor(edge_list_model(), graph, k=K)
    assert other.retire_entities([3, 4]).tolist() == [1, 1] and other.delta.num_removed == 1


def test_a_retired_id_is_no_anchor_and_no_argument():
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=K, batch_size=4)
    assert qp.retire_entities(8).tolist() == [0] and qp.delta is None      # (no fact: no edit, no delta yet)
    for call in (qp.add_facts, qp.remove_facts):
        with pytest.raises(ValueError, match="retired"):
            call(8, 0, 1)
        with pytest.raises(ValueError, match="retired"):
            call([0, 2], [0, 1], [1, 8])
    assert qp.delta is None
    # the lazily made delta knows the set, and a later retirement reaches the delta held
    assert qp.add_facts(0, 1, 2) == 1 and qp.delta.retired.tolist() == [8]
    assert qp.retire_entities(3).tolist() == [1] and qp.delta.retired.tolist() == [3, 8]
    for call in (qp.add_facts, qp.remove_facts):
        for dead in (3, 8):
            with pytest.raises(ValueError, match="retired"):
                call(dead, 0, 1)
            with pytest.raises(ValueError, match="retired"):
                call(0, 1, dead)
    assert len(qp.delta) == 1
    for dead in (3, 8):
        with pytest.raises(ValueError, match=r"entity id %d was retired" % dead):
            qp.answers([(dead, (0,))])
        with pytest.raises(ValueError, match=r"entity id %d was retired" % dead):
            qp.answer_sets([(2, (0,)), ((1, (0,)), (dead, (1, -2)))])
        with pytest.raises(ValueError, match="retired"):
            qp.batches([(dead, (0, 1))])
    assert qp.answers([(4, (0,))])[0].shape == (1, K)


@pytest.mark.parametrize("logic", ["product", "godel"])
def test_answers_equal_the_definition_without_a_reserve(logic):
    """Bit for bit: the served graph and the materialised one have the same rows."""
    graph = twelve_node_graph()
    model = edge_list_model(logic)
    qp = query_predict.QueryPredictor(model, graph, k=K, batch_size=4)
    queries = reanchored(folded_queries(), {1, 8, 3})
    assert len(queries) == 31 and ends_in_negation(queries) == [28, 29, 30]
    check_against_definition(qp, queries, edge_list_model(logic), what="nothing retired")
    for step, ids in enumerate((8, 1, [3])):
        qp.retire_entities(ids)
        (answers, sets), (want, _) = check_against_definition(qp, queries, edge_list_model(logic), what="retirement %d" % step)
    assert qp.live_count is None and qp.graph is graph and qp.num_retired == 3
    for i in ends_in_negation(queries):
        assert int(want[2][i]) < K, "a query that ends in a negation entails most entities: its row is short"
    # a held delta fact that names a retired entity leaves the delta; the set survives compact()
    assert qp.add_facts([2, 4], [1, 0], [6, 7]) == 2
    assert qp.retire_entities(6).tolist() == [3] and len(qp.delta) == 1
    check_against_definition(qp, reanchored(queries, {1, 8, 3, 6}), edge_list_model(logic), what="a held fact")
    qp.compact()
    assert qp.delta is None and qp.graph is not graph and qp.retired_entities.tolist() == [1, 3, 6, 8]
    assert qp.materialized().retired_entities.tolist() == [1, 3, 6, 8] and int(qp.graph.num_nodes) == N
    with pytest.raises(ValueError, match="retired"):
        qp.add_facts(0, 0, 6)
    check_against_definition(qp, reanchored(queries, {1, 8, 3, 6}), edge_list_model(logic), what="compacted")
    # filtered=False: no list, and still no retired id
    loose = query_predict.QueryPredictor(edge_list_model(logic), graph, k=N, batch_size=4, filtered=False)
    loose.retire_entities([1, 8])
    (answers, _), _ = check_against_definition(loose, queries, edge_list_model(logic), what="unfiltered")
    assert answers[2].tolist() == [N - 2] * len(queries)


@pytest.mark.parametrize("make,scores", [(edge_list_model, close), (exact_model, same_bits)], ids=["sigmoid", "exact"])
def test_answers_equal_the_definition_with_a_reserve(make, scores):
    """Rows of N + 4 slots against num_entities nodes: ids, counts, offsets and sizes exactly; the scores within SCORE_TOL on the
    stub with a sigmoid and bit for bit on the one rounded per element (the module docstring)."""
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(make(), graph, k=K, batch_size=4, entity_capacity=4)
    a, b = qp.add_entities(2).tolist()
    assert qp.add_facts([2, a], [0, 1], [a, b]) == 2        # a is the only midpoint of the path 2 -0-> a -1-> b
    P, S = Query.projection, Query.stop
    queries = reanchored(folded_queries(), {a, 8})
    width = queries.shape[1]
    two_p = torch.tensor([[2, P | 0, P | 1] + [S] * (width - 3)])
    queries = torch.cat([two_p, queries])                   # (the three that end in a negation stay last)
    wide = query_predict.QueryPredictor(make(), graph, k=N + 4, batch_size=4, entity_capacity=4)
    wide.add_entities(2)
    wide.add_facts([2, a], [0, 1], [a, b])
    ids, _, count = wide.answers(two_p)
    assert b not in ids[0, :int(count[0])].tolist(), "the end of the path is entailed"
    for p in (qp, wide):
        with pytest.raises(ValueError):
            p.retire_entities(b + 1)                        # (a reserved row is no entity)
        assert p.retire_entities([a, 8]).tolist() == [2, 0] and len(p.delta) == 0
    ids, _, count = wide.answers(two_p)
    assert b in ids[0, :int(count[0])].tolist() and a not in ids[0].tolist(), "... and is not once the midpoint is retired"
    assert qp.num_entities == N + 2 and int(qp.live_count) == N + 2 and qp.num_slots == N + 4
    check_against_definition(qp, queries, make(), scores, "retired in the reserve")
    counts = definition(wide, queries, make())[0][2]
    assert torch.equal(wide.answers(queries)[2], counts) and int(counts.max()) <= N + 2 - 2
    # beyond the reserve: one rebuild, a longer bitmap with the bits kept
    assert qp.add_entities(3).tolist() == [14, 15, 16] and qp.num_slots == 21 and qp.retired_entities.tolist() == [8, a]
    assert qp.add_facts(16, 0, 2) == 1
    with pytest.raises(ValueError, match="retired"):
        qp.add_facts(16, 0, a)
    check_against_definition(qp, queries, make(), scores, "after the overflow rebuild")


@pytest.mark.parametrize("capacity", [0, 4])
def test_a_final_negation_leaves_one_in_the_retired_slot(capacity):
    """What the list kernel is for: the final symbolic set of a query that ends in a negation holds 1 - 0 = 1.0 at a retired id
    -- nothing is zeroed on the way -- and the lists leave it out."""
    graph = twelve_node_graph()
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=N + capacity, batch_size=4, entity_capacity=capacity)
    queries = folded_queries()[-3:]
    qp.retire_entities([1, 8])
    program = query_exec.compile(queries, qp.num_slots, graph.num_relations)
    _, sym = query_exec.execute(qp.model, qp.graph, program, **qp._delta_kwargs())
    assert bool((sym[:, [1, 8]] == 1.0).all())
    ptr, known = qp._known_reference(sym, len(queries))
    lists = [known[int(ptr[i]):int(ptr[i + 1])].tolist() for i in range(len(queries))]
    for i, row in enumerate(lists):
        want = [v for v in range(N) if float(sym[i, v]) != 0 and v not in (1, 8)]
        assert row == want and len(row) > N // 2
    ids, _, count = qp.answers(queries)
    assert count.tolist() == [N - 2 - len(row) for row in lists]
    assert not bool(torch.isin(ids, torch.tensor([1, 8])).any()) and int(ids.max()) < N
