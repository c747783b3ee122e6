"""What-if logical queries on the GPU.

The kernel: ultra_symbolic_traversal_edit_rows_owned on tests/test_query_live_gpu.py's hub graph (a 150-edge segment into node 0)
over an rspmm.AssumedFacts overlay, per sample against the traversal's torch restatement on [materialised graph ; that sample's
direct edges ; its inverse edges] -- torch.equal; the early-out contract on a sentinel-filled output; every owner -1 against the
un-owned entry; owners that name no sample; NULL dead arrays; a captured launch that serves a refill.

End to end: QueryPredictor.answers / answer_sets (assuming=) on the golden graph and ultraquery weights against
query_predict.assume_reference, bit for bit, for seven query types under six states of the served graph; the 2p hypothesis that
entails for its own query alone; a `mean` model through the per-query loop; the command-line tool."""
import ctypes
import random

import pytest
import torch

from tests.test_grow_gpu import counted
from tests.test_query_exec_cpu import load
from tests.test_query_live_gpu import N, apply_edits, fuzzy_sets, hub_graph
from tests.test_ultraquery_gpu import build_model, golden_graph
from ultra_amd import _lib, query_predict, rspmm
from ultra_amd.ultraquery import _CSR_CACHE, symbolic_traversal, symbolic_traversal_reference, traversal_csr

pytestmark = pytest.mark.gpu

ENTRY, UNOWNED, RSPMM_OWNED = ("ultra_symbolic_traversal_edit_rows_owned", "ultra_symbolic_traversal_edit_rows",
                               "ultra_rspmm_edit_rows_owned")
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---- the kernel ----
def hub_facts():
    """Per sample of fuzzy_sets (relations 2, 0, 2, 3, 1) its assumed facts (h, r, t), at most 16 each.
      (0, 0, 17)   sample 0 only: the inverse edge 17 -> 0 of relation 2 -- one more parallel edge of the hub's maximum, which a base
                   edge states already, and under apply_edits' dead key (17 -> 0, 2): sample 0 gets 2.0 back, sample 2 does not
      (38, 0, 12)  samples 0 and 2: the same fact twice; the inverse edge 12 -> 38 of relation 2 into a tail without an in-edge
      (6, 0, 35)   sample 1 only: the tail 35 has no in-edge
      (a, 1, 25)   fourteen from EACH sample: 70 overlay edges of relation 1 into tail 25 with mixed owners -- two 64-lane trips"""
    facts = [[((3 * j + s) % N, 1, 25) for j in range(14)] for s in range(5)]
    facts[0] += [(0, 0, 17), (38, 0, 12)]
    facts[2] += [(38, 0, 12)]
    facts[1] += [(6, 0, 35)]
    return facts


def hub_case(dev, case):
    data = hub_graph(dev)
    delta = None
    if case != "no delta":
        delta = rspmm.GraphDelta(data, capacity=16)
        if case == "add-only":
            delta.add([30, 0], [0, 0], [31, 33])
        else:
            apply_edits(delta)
    overlay = rspmm.AssumedFacts(data, delta, 5, 16)
    return data, delta, overlay


def oracle(data, delta, facts, h, r):
    """Row b: the traversal's restatement on [materialised ; sample b's direct edges ; its inverse edges]."""
    mat = data if delta is None else delta.materialize()
    rows = []
    for b in range(h.shape[0]):
        index, kind = mat.edge_index, mat.edge_type
        if facts[b]:
            hh, rr, tt = torch.tensor(facts[b], device=h.device).unbind(1)
            index = torch.cat([index, torch.stack([torch.cat([hh, tt]), torch.cat([tt, hh])])], dim=1)
            kind = torch.cat([kind, rr, rr + 2])
        rows.append(symbolic_traversal_reference(index, kind, N, h[b:b + 1], r[b:b + 1]))
    return torch.cat(rows)


def call_entry(name, data, operand, owner, h, r, t):
    csr = traversal_csr(data.edge_index, data.edge_type, N)
    args = [csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), N, ctypes.byref(operand)]
    if owner is not None:
        args.append(owner.data_ptr())
    args += [r.data_ptr(), h.shape[0], _lib.F32 if h.dtype == torch.float32 else _lib.F64, h.data_ptr(), t.data_ptr(),
             _lib.stream_of(h)]
    return getattr(_lib.lib, name)(*args)


def early_out_pairs(overlay, delta, r, batch):
    """The (tail, sample) pairs the early-out rule names, from the layout on the host: no dead key of relation r[b] at the tail
    and no edge of that relation live for b; and the touched tails."""
    lay = overlay.traversal
    count = int(lay.count)
    rows, add_ptr, dead_ptr = lay.rows[:count].tolist(), lay.add_ptr[:count + 1].tolist(), lay.dead_ptr[:count + 1].tolist()
    kind, owner = lay.add_type.tolist(), lay.owner.tolist()
    dead_kind = [] if delta is None else delta.traversal.dead_type.tolist()
    skipped = set()
    for k, v in enumerate(rows):
        for b in range(batch):
            rel = int(r[b])
            dead = delta is not None and any(dead_kind[j] == rel for j in range(dead_ptr[k], dead_ptr[k + 1]))
            live = any(kind[j] == rel and owner[j] in (-1, b) for j in range(add_ptr[k], add_ptr[k + 1]))
            if not dead and not live:
                skipped.add((v, b))
    return skipped, rows


@pytest.mark.parametrize("case", ["no delta", "add-only", "tombstones"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_owned_edit_rows_equal_the_traversal_of_each_samples_graph(dev, dtype, batch, case):
    data, delta, overlay = hub_case(dev, case)
    ei, et = data.edge_index, data.edge_type
    facts = hub_facts()
    assert overlay.fill(facts) == (0 if delta is None else 2 * len(delta)) + 2 * sum(len(f) for f in facts)
    h, r = fuzzy_sets(batch, dtype, dev)
    want = oracle(data, delta, facts, h, r)
    got = symbolic_traversal(ei, et, N, h, r, delta=overlay)
    assert got.dtype == dtype and torch.equal(got, want)
    # the layout holds what the issue asks of it
    lay = overlay.traversal
    count = int(lay.count)
    rows, add_ptr = lay.rows[:count].tolist(), lay.add_ptr[:count + 1].tolist()
    k25 = rows.index(25)
    in25 = list(zip(lay.add_type[add_ptr[k25]:add_ptr[k25 + 1]].tolist(), lay.owner[add_ptr[k25]:add_ptr[k25 + 1]].tolist()))
    assert sum(1 for kind, _ in in25 if kind == 1) == 70 > 64 and {o for kind, o in in25 if kind == 1} == {0, 1, 2, 3, 4}
    assert 35 in rows and 38 in rows and int(torch.bincount(ei[1], minlength=N)[35]) == 0
    # the hypothesis at the hub is sample 0's alone
    if case == "tombstones":
        assert float(got[0, 0]) == 2.0
        if batch == 5:
            assert 0.0 < float(got[2, 0]) < 2.0 and float(got[2, 38]) == float(h[2, 12]) == float(want[2, 38])
    if batch == 5:
        assert float(got[1, 35]) == float(h[1, 6]) > 0 and float(got[0, 35]) == 0.0
        own = max(float(h[4, a]) for a, _, _ in facts[4])
        assert float(got[4, 25]) == max(own, float(h[4, 8]), 0.0)       # (8 -> 25 is the tail's one base edge of relation 1)
    # the C entry on a sentinel-filled output: the early-out pairs are not written, every other touched pair is the oracle's
    skipped, touched = early_out_pairs(overlay, delta, r, batch)
    t = torch.full_like(h, SENTINEL)
    assert call_entry(ENTRY, data, overlay.traversal_operand(), overlay.traversal_owner, h, r, t) == _lib.ULTRA_OK
    expect = torch.full_like(h, SENTINEL)
    for v in touched:
        for b in range(batch):
            if (v, b) not in skipped:
                expect[b, v] = want[b, v]
    assert torch.equal(t, expect)
    assert skipped and len(skipped) < len(touched) * batch
    if batch == 5:
        assert (0, 1) in skipped and (25, 0) in skipped and (25, 4) not in skipped and (35, 1) not in skipped
        assert ((0, 2) in skipped) == (case == "no delta")          # (with a delta the hub holds a shared edge or a dead key)
    # whatever lies beyond the live parts of the buffers is never read
    m = overlay.num_edges
    far = 1 << 30
    lay.rows[count:] = far
    lay.add_ptr[count + 1:] = far
    lay.dead_ptr[count + 1:] = far
    lay.add_src[m:] = far
    lay.add_type[m:] = far
    lay.owner[m:] = -1
    assert torch.equal(symbolic_traversal(ei, et, N, h, r, delta=overlay), want)


@pytest.mark.parametrize("case", ["add-only", "tombstones"])
def test_with_every_owner_shared_the_entry_is_the_unowned_one(dev, case):
    data, delta, overlay = hub_case(dev, case)
    overlay.fill(hub_facts())
    h, r = fuzzy_sets(5, torch.float32, dev)
    base = symbolic_traversal(data.edge_index, data.edge_type, N, h, r)
    operand = overlay.traversal_operand()
    shared = torch.full_like(overlay.traversal_owner, -1)
    owned, plain = base.clone(), base.clone()
    assert call_entry(ENTRY, data, operand, shared, h, r, owned) == _lib.ULTRA_OK
    assert call_entry(UNOWNED, data, operand, None, h, r, plain) == _lib.ULTRA_OK
    assert torch.equal(owned.view(torch.int32), plain.view(torch.int32)) and not torch.equal(owned, base)
    # the un-owned entry still writes every touched pair
    t = torch.full_like(h, SENTINEL)
    assert call_entry(UNOWNED, data, operand, None, h, r, t) == _lib.ULTRA_OK
    count = int(overlay.traversal.count)
    touched = overlay.traversal.rows[:count].long()
    assert not bool((t[:, touched] == SENTINEL).any()) and int((t != SENTINEL).sum()) == 5 * count


def test_an_owner_that_names_no_sample_is_live_nowhere(dev):
    data, delta, overlay = hub_case(dev, "tombstones")
    facts = hub_facts()
    overlay.fill(facts)
    h, r = fuzzy_sets(5, torch.float32, dev)
    owner = overlay.traversal_owner.clone()
    for sample, value in ((1, -2), (2, 5), (3, 1 << 30)):
        owner[overlay.traversal_owner == sample] = value
    t = symbolic_traversal(data.edge_index, data.edge_type, N, h, r)
    assert call_entry(ENTRY, data, overlay.traversal_operand(), owner, h, r, t) == _lib.ULTRA_OK
    seen = [facts[0], [], [], [], facts[4]]
    assert torch.equal(t, oracle(data, delta, seen, h, r))
    assert not torch.equal(t, oracle(data, delta, facts, h, r))


def test_null_dead_arrays_mean_no_tombstones(dev):
    data, delta, overlay = hub_case(dev, "add-only")
    facts = hub_facts()
    overlay.fill(facts)
    h, r = fuzzy_sets(5, torch.float32, dev)
    operand = overlay.traversal_operand()
    assert operand.dead_ptr_dev is not None
    operand.dead_ptr_dev = operand.dead_src_dev = operand.dead_type_dev = None
    t = symbolic_traversal(data.edge_index, data.edge_type, N, h, r)
    assert call_entry(ENTRY, data, operand, overlay.traversal_owner, h, r, t) == _lib.ULTRA_OK
    assert torch.equal(t, oracle(data, delta, facts, h, r))


def test_a_captured_launch_serves_a_refill(dev):
    data, delta, overlay = hub_case(dev, "add-only")
    ei, et = data.edge_index, data.edge_type
    h, r = fuzzy_sets(5, torch.float32, dev)
    overlay.fill([[(30, 0, 31)], None, None, None, None])
    out = []

    def step():
        out[:] = [symbolic_traversal(ei, et, N, h, r, delta=overlay)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # (the CSR and the layouts exist from here on)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    pinned = [t.data_ptr() for t in overlay.traversal]
    apply_edits(delta)                                  # the delta moves on: more facts, the first tombstones
    facts = hub_facts()
    facts = facts[1:] + facts[:1]                       # other facts, other owners
    overlay.fill(facts)
    assert [t.data_ptr() for t in overlay.traversal] == pinned
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], oracle(data, delta, facts, h, r))


# ---- end to end ----
TYPES = {
    "1p": lambda a, b, r: (a, (r[0],)),
    "2p": lambda a, b, r: (a, (r[0], r[1])),
    "2i": lambda a, b, r: ((a, (r[0],)), (b, (r[1],))),
    "2in": lambda a, b, r: ((a, (r[0],)), (b, (r[1], -2))),
    "ip": lambda a, b, r: (((a, (r[0],)), (b, (r[1],))), (r[2],)),
    "pi": lambda a, b, r: ((a, (r[0], r[1])), (b, (r[2],))),
    "2u": lambda a, b, r: ((a, (r[0],)), (b, (r[1],)), (-1,)),
}
PROBABILITY = 0.45


def typed_queries(name, count, n, num_relations, seed, banned=()):
    rng = random.Random(seed)
    ok = [v for v in range(n) if v not in banned]
    return [TYPES[name](rng.choice(ok), rng.choice(ok), [rng.randrange(num_relations) for _ in range(3)]) for _ in range(count)]


def anchors_of(query):
    if len(query) == 2 and isinstance(query[1][-1], int):
        return anchors_of(query[0]) if isinstance(query[0], tuple) else [query[0]]
    return [a for branch in query if branch != (-1,) for a in anchors_of(branch)]


def hypotheses(queries, n, half, seed, banned=(), heads=()):
    """One entry per query, in the list form: most queries assume one to three facts -- the first leaves one of the query's own
    anchors --, every fourth nothing (None, or an empty tensor); `heads`: ids some facts start from (a new entity)."""
    rng = random.Random(seed)
    ok = [v for v in range(n) if v not in banned]
    out = []
    for i, query in enumerate(queries):
        if i % 4 == 3:
            out.append(None if i % 8 == 3 else torch.zeros(0, 3, dtype=torch.long))
            continue
        facts = [(anchors_of(query)[0], rng.randrange(half), rng.choice(ok))]
        for _ in range(rng.randrange(3)):
            facts.append((rng.choice(list(heads) or ok), rng.randrange(half), rng.choice(ok)))
        out.append(torch.tensor(facts) if i % 2 else facts)
    return out


def same_topk(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
            and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)))


def same_sets(got, want):
    return (len(got) == len(want) == 4 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            and torch.equal(got[3], want[3]) and torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)))


def served_state(qp):
    mat = qp.materialized()
    delta = qp.delta
    return (mat.edge_index.clone(), mat.edge_type.clone(), None if delta is None else (id(delta), delta.version, len(delta),
            delta.num_removed), id(qp.graph), len(_CSR_CACHE), len(rspmm.cached_plans()))


def same_state(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]


def check_against_reference(qp, model, queries, assumed, what, **among):
    """answers / answer_sets (assuming=) against assume_reference on qp.materialized(), bit for bit; nothing stated."""
    qp.answers(queries)                                 # (the plan and the CSR of the served graph exist from here on)
    before = served_state(qp)
    got = qp.answers(queries, assuming=assumed, **among)
    sets = qp.answer_sets(queries, probability=PROBABILITY, assuming=assumed, **among)
    assert same_state(before, served_state(qp)), what
    kwargs = dict(retired=qp.retired_entities if qp.num_retired else None)
    if among:
        kwargs["among"] = among["among"]
    mat = qp.materialized()
    want = query_predict.assume_reference(model, mat, queries, assumed, k=qp.k, **kwargs)
    assert same_topk(got, want), what
    want = query_predict.assume_reference(model, mat, queries, assumed, probability=PROBABILITY, **kwargs)
    assert same_sets(sets, want), what
    return got


@pytest.fixture(scope="module")
def golden(dev):
    g = load()
    return g, build_model(g, dev), golden_graph(g, dev)


def stated(qp, graph):
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    assert qp.add_facts([5, 78, 40, 62, 199], [0, 3, 3, 0, 5], [78, 150, 150, 27, 0]) == 5
    return ei, et


@pytest.mark.parametrize("name", sorted(TYPES))
def test_every_query_type_equals_the_reference(golden, monkeypatch, name):
    """batch_size 4 with 7 queries of the type: the group is cut and the last batch is short.  A never-edited predictor, then
    stated facts, then tombstones."""
    g, model, graph = golden
    n, rels = g["num_nodes"], g["num_relations"]
    queries = typed_queries(name, 7, n, rels, seed=len(name) + 5)
    assumed = hypotheses(queries, n, rels // 2, seed=3)
    calls = counted(monkeypatch, [ENTRY, RSPMM_OWNED])
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, delta_capacity=16)
    assert [len(index) for index in qp.batches(queries)] == [4, 3] and query_predict.assume_supported(model)
    got = check_against_reference(qp, model, queries, assumed, "never edited")
    assert qp.delta is None and not qp._assume_loop_only
    assert calls[ENTRY] > 0 and calls[RSPMM_OWNED] > 0, "the engine route served the call"
    plain = qp.answers(queries)
    assert not same_topk(got, plain), "the hypotheses change answers of the fixture"
    for q in range(3, len(queries), 4):                 # the queries that assume nothing
        assert same_topk([part[q:q + 1] for part in got], [part[q:q + 1] for part in plain])
    ei, et = stated(qp, graph)
    check_against_reference(qp, model, queries, assumed, "stated facts")
    direct = (et < rels // 2).nonzero().flatten()[[0, 57, 400, 1200]]
    assert bool((qp.remove_facts(ei[0, direct], et[direct], ei[1, direct]) >= 1).all())
    # a retracted fact assumed again, by the first query alone
    again = list(assumed)
    again[0] = [(int(ei[0, direct[0]]), int(et[direct[0]]), int(ei[1, direct[0]]))] + list(again[0])[:2]
    check_against_reference(qp, model, queries, again, "tombstones")
    assert not qp._assume_loop_only and qp.graph is graph and not model.training


def test_the_tensor_form_and_candidate_sets(golden):
    g, model, graph = golden
    n, rels = g["num_nodes"], g["num_relations"]
    queries = typed_queries("2p", 6, n, rels, seed=21) + typed_queries("2i", 4, n, rels, seed=22)
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, delta_capacity=16)
    stated(qp, graph)
    shared = torch.tensor([[anchors_of(queries[0])[0], 2, 17], [17, 4, 90]], device=graph.edge_index.device)
    check_against_reference(qp, model, queries, shared, "one tensor for every query")
    among = [torch.arange(q % 3, n, 2 + q % 2) for q in range(len(queries))]
    assumed = hypotheses(queries, n, rels // 2, seed=8)
    check_against_reference(qp, model, queries, assumed, "among", among=among)
    assert not qp._assume_loop_only


def test_a_new_entity_and_a_retired_one(golden):
    g, model, graph = golden
    n, rels = g["num_nodes"], g["num_relations"]
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, delta_capacity=16, entity_capacity=4)
    stated(qp, graph)
    (new,) = qp.add_entities(1).tolist()
    assert new == n
    queries = typed_queries("2p", 6, n, rels, seed=31) + typed_queries("pi", 6, n, rels, seed=32)
    assumed = hypotheses(queries, n, rels // 2, seed=9, heads=[new])
    assert any(int(torch.as_tensor(f)[:, 0].eq(new).sum()) for f in assumed if f is not None and len(f))
    check_against_reference(qp, model, queries, assumed, "a new entity as a hypothesis' head")
    gone = 33
    qp.retire_entities([gone])
    queries = typed_queries("2p", 6, n, rels, seed=31, banned=[gone]) + typed_queries("2in", 6, n, rels, seed=33, banned=[gone])
    assumed = hypotheses(queries, n, rels // 2, seed=10, banned=[gone], heads=[new])
    got = check_against_reference(qp, model, queries, assumed, "a retired entity")
    assert not bool((got[0] == gone).any()) and not qp._assume_loop_only
    with pytest.raises(ValueError, match="retired"):
        qp.answers(queries, assuming=[[(gone, 0, 1)]] + [None] * (len(queries) - 1))


def test_a_hypothesis_is_traversed_and_entailed_for_its_own_query_alone(golden):
    """A 2p query (a, (r1, r2)) whose anchor has no r1 edge: assuming (a, r1, b) with (b, r2, c) stated, c is entailed -- absent
    from that query's answers, its count one less -- while the same query without the hypothesis, in the same batch, keeps c."""
    g, model, graph = golden
    n = g["num_nodes"]
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    r1, r2 = 0, 1
    a = next(v for v in range(n) if not bool(((ei[0] == v) & (et == r1)).any()))        # no edge of r1 leaves it
    b = next(v for v in range(n) if v != a and not bool(((ei[0] == v) & (et == r2)).any()))       # ... and none of r2 leaves b
    c = next(v for v in range(n) if v not in (a, b))
    qp = query_predict.QueryPredictor(model, graph, k=n, batch_size=4)
    assert qp.add_facts(b, r2, c) == 1
    queries = [(a, (r1, r2)), (a, (r1, r2)), (a, (r1,))]
    assert qp.batches(queries)[0] == [0, 1]
    ids, _, count = qp.answers(queries, assuming=[[(a, r1, b)], None, [(a, r1, b)]])
    lists = [ids[i, :int(count[i])].tolist() for i in range(3)]
    assert count.tolist() == [n - 1, n, n - 1]
    assert c not in lists[0] and c in lists[1] and b not in lists[2] and b in lists[0]
    assert same_topk((ids, _, count), query_predict.assume_reference(model, qp.materialized(), queries,
                                                                      [[(a, r1, b)], None, [(a, r1, b)]], k=n))
    assert qp.answers(queries)[2].tolist() == [n, n, n] and len(qp.delta) == 1


def test_a_mean_model_runs_the_loop_and_equals_the_reference(golden, dev, monkeypatch):
    from ultra_amd import models, synthetic
    from ultra_amd.ultraquery import UltraQuery
    g, _, graph = golden
    torch.manual_seed(5)
    cfg = synthetic.default_model_cfg(aggregate_func="mean")
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = UltraQuery(models.Ultra(**cfg)).to(dev).eval()
    assert not query_predict.assume_supported(model)
    n, rels = g["num_nodes"], g["num_relations"]
    queries = typed_queries("2p", 3, n, rels, seed=41) + typed_queries("2u", 2, n, rels, seed=42)
    assumed = hypotheses(queries, n, rels // 2, seed=11)
    calls = counted(monkeypatch, [ENTRY, RSPMM_OWNED])
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, delta_capacity=16)
    stated(qp, graph)
    got = qp.answers(queries, assuming=assumed)
    assert calls[ENTRY] == 0 and calls[RSPMM_OWNED] == 0
    assert same_topk(got, query_predict.assume_reference(model, qp.materialized(), queries, assumed, k=5))
    assert len(qp.delta) == 5 and not same_topk(got, qp.answers(queries))


def test_the_command_line_tool_assumes_by_name(dev, capsys):
    """tools/query_predict.py --assume H R T: a 2p query whose first hop only the hypothesis states -- by name, through the
    vocabulary -- loses the tails the second hop then entails; nothing is stated; an unknown name ends the tool."""
    import importlib.util
    import os
    from ultra_amd import data as udata
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_fixture")
    spec = importlib.util.spec_from_file_location("query_predict_tool", os.path.join(os.path.dirname(root), os.pardir, os.pardir,
                                                                                      "tools", "query_predict.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ent, rel = udata.read_vocab(root)
    data = udata.load_triples_dir(root)
    ei, et = data.edge_index, data.edge_type
    n = int(data.num_nodes)
    r1, r2 = 0, 1
    a = next(v for v in range(n) if not bool(((ei[0] == v) & (et == r1)).any()))        # no edge of r1 leaves it
    b = int(ei[0][et == r2][0])
    tails = sorted(set(ei[1][(ei[0] == b) & (et == r2)].tolist()))
    assert tails and a != b
    others = [v for v in range(n) if v not in tails and v not in (a, b)][:3]
    listed = ["--among"] + [ent[v] for v in tails + others]             # (a shortlist: the fixture has more entities than k allows)
    query = ["--data-root", root, "--query", repr((ent[a], (rel[r1], rel[r2]))), "-k", "64"]

    def answers(argv):
        torch.manual_seed(0)                            # (no checkpoint: the same random weights in every run)
        tool.main(argv)
        lines = capsys.readouterr().out.splitlines()
        return lines, [line.split()[1] for line in lines if line[:3].strip().isdigit()]
    assert len(tails) + 3 <= 64
    _, before = answers(query + listed)
    assert sorted(before) == sorted(ent[v] for v in tails + others)
    lines, after = answers(query + ["--assume", ent[a], rel[r1], ent[b]] + listed)
    assert any(line.startswith("assuming 1 fact(s)") for line in lines)
    assert sorted(after) == sorted(ent[v] for v in others)
    assert sorted(answers(query + listed)[1]) == sorted(before)          # nothing was stated: every run starts from the dataset
    with pytest.raises(SystemExit):
        tool.main(query + ["--assume", "no such entity", rel[r1], ent[b]])
    with pytest.raises(SystemExit):
        tool.main(query + ["--assume", ent[a], "no such relation", ent[b]])
