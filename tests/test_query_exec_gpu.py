"""The compiled query executor on the GPU: ultra_query_segment against `run_reference` bit for bit (with sentinels around
everything a program must not touch), the compiled executor against `UltraQuery.forward` with the ultraquery.pth weights,
evaluation through it, its freedom from host waits, ultra_nonzero_lists against torch.nonzero and QueryPredictor against the
eager route through `filtered_topk_reference`."""
import ctypes
import types

import pytest
import torch

from tests.test_query_exec_cpu import LOGICS, load, plain, random_queries, remap_entities, stub_model, stub_projection, type_rows
from tests.test_ultraquery_gpu import METRICS, build_model, golden_graph

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def same(a, b):
    """torch.equal with NaNs equal by position."""
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    return torch.equal(nan_a, nan_b) and torch.equal(torch.where(nan_a, torch.zeros_like(a), a),
                                                     torch.where(nan_b, torch.zeros_like(b), b))


def planted(fn):
    """The stub with NaN and +-inf planted in its output."""
    def call(h, r, symbolic):
        out = fn(h, r, symbolic).clone()
        n = out.shape[1]
        out[0, 1 % n] = float("nan")
        out[-1, n // 2] = float("inf")
        out[0, n - 1] = float("-inf")
        out[-1, 0] = -0.0
        return out
    return call


def stub_uq(logic, fn=stub_projection):
    return types.SimpleNamespace(training=False, logic=logic, model=lambda g, h, r: fn(h, r, False),
                                 symbolic_model=lambda g, h, r: fn(h, r, True))


def contract_run(program, logic, fn, symbolic, dev):
    """ultra_query_segment's contract, slot for slot, on sentinel-filled buffers: only live slots are loaded, only changed
    slots that are still live at the end of the segment are stored."""
    from ultra_amd import query_exec
    from ultra_amd.ultraquery import _logic
    conj, disj = _logic(logic)
    batch, n = program.batch, program.num_nodes
    count = 2 if symbolic else 1
    stacks = [torch.full((batch, 2, n), SENTINEL, device=dev) for _ in range(count)]
    inputs = [torch.full((batch, n), SENTINEL, device=dev) for _ in range(count)]
    results = [torch.full((batch, n), SENTINEL, device=dev) for _ in range(count)]
    outs = [None] * count
    last = len(program.segments) - 1
    for s, seg in enumerate(program.segments):
        targets = results if s == last else inputs
        for z in range(count):
            for b in range(batch):
                d = seg.entry_depth[b]
                reg = [stacks[z][b, j].clone() if j < d else None for j in range(2)]
                dirty = set()
                if seg.push_row[b] >= 0:
                    reg[d] = outs[z][seg.push_row[b]].clone()
                    dirty.add(d)
                    d += 1
                for kind, e in seg.ops[b]:
                    if kind == query_exec.PUSH_ENTITY:
                        reg[d] = torch.zeros(n, device=dev)
                        reg[d][e] = 1
                        dirty.add(d)
                        d += 1
                    elif kind == query_exec.NOT:
                        reg[d - 1] = 1 - reg[d - 1]
                        dirty.add(d - 1)
                    else:
                        reg[0] = (conj if kind == query_exec.AND else disj)(reg[0], reg[1])
                        dirty.add(0)
                        d = 1
                if seg.pop_row[b] >= 0:
                    targets[z][seg.pop_row[b]] = reg[d - 1]
                    d -= 1
                for j in range(d):
                    if j in dirty:
                        stacks[z][b, j] = reg[j]
        if s < last:
            rows = len(program.projections[s].samples)
            r_index = torch.tensor(program.projections[s].relations, dtype=torch.int64, device=dev)
            outs = [fn(inputs[z][:rows], r_index, z == 1) for z in range(count)]
    return stacks, inputs, results


def check_segment_kernel(query, n, num_relations, logic, symbolic, dev, fn=stub_projection):
    from ultra_amd import query_exec
    program = query_exec.compile(query, n, num_relations)
    want_prob, want_sym = query_exec.run_reference(program, logic, lambda h, r: fn(h, r, False),
                                                   (lambda h, r: fn(h, r, True)) if symbolic else None, device=dev)
    executor = query_exec.Executor()
    stacks, inputs = executor._get(dev, program.batch, n, symbolic)
    for t in stacks + inputs:
        t.fill_(SENTINEL)
    graph = types.SimpleNamespace(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev), num_nodes=n,
                                  num_relations=num_relations)
    prob, sym = executor.run(stub_uq(logic, fn), graph, program, symbolic)
    assert same(prob, want_prob)
    assert (sym is None) if not symbolic else same(sym, want_sym)
    c_stacks, c_inputs, c_results = contract_run(program, logic, fn, symbolic, dev)
    assert same(prob, c_results[0])
    for got, want in zip(stacks + inputs, c_stacks + c_inputs):
        assert same(got, want)
    return program


def golden_rows(g, batch, n, seed):
    """`batch` rows of the golden batch (all 14 types when batch allows), entity ids folded into [0, n)."""
    perm = torch.randperm(len(g["query"]), generator=torch.Generator().manual_seed(seed))[:batch]
    return remap_entities(plain(g["query"])[perm.sort().values if batch == len(g["query"]) else perm], n)


@pytest.mark.parametrize("symbolic", [False, True])
@pytest.mark.parametrize("logic", LOGICS)
@pytest.mark.parametrize("batch", [1, 5, 28])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 200, 4099])
def test_segment_kernel_matches_reference(dev, n, batch, logic, symbolic):
    g = load()
    r = g["num_relations"]
    check_segment_kernel(golden_rows(g, batch, n, seed=n + batch), n, r, logic, symbolic, dev)
    check_segment_kernel(random_queries(batch, n, r, seed=100 * n + batch), n, r, logic, symbolic, dev)


@pytest.mark.parametrize("logic", LOGICS)
def test_segment_kernel_every_type_alone(dev, logic):
    g = load()
    for n in (63, 200):
        for name in g["id2type"]:
            rows = remap_entities(type_rows(g, name), n)
            check_segment_kernel(torch.cat([rows, rows, rows[:1]]), n, g["num_relations"], logic, True, dev)


@pytest.mark.parametrize("logic", LOGICS)
def test_segment_kernel_propagates_nan_and_inf(dev, logic):
    g = load()
    for n in (65, 200):
        query = golden_rows(g, 28, n, seed=1)
        program = check_segment_kernel(query, n, g["num_relations"], logic, True, dev, fn=planted(stub_projection))
        assert len(program.projections) == 3
        check_segment_kernel(random_queries(5, n, 7, seed=n), n, 7, logic, True, dev, fn=planted(stub_projection))
    # the planted values reach the result of a 1p query untouched
    from ultra_amd import query_exec
    fn = planted(stub_projection)
    q = remap_entities(type_rows(g, "1p"), 65)
    graph = types.SimpleNamespace(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev), num_nodes=65,
                                  num_relations=g["num_relations"])
    prob, _ = query_exec.Executor().run(stub_uq(logic, fn), graph, query_exec.compile(q, 65, g["num_relations"]), False)
    assert torch.isnan(prob[0, 1]) and prob[1, 32] == float("inf") and prob[0, 64] == float("-inf")


def test_segment_kernel_grid_stride_rows(dev):
    """Rows longer than the grid cap covers at once (scalar and 16-byte paths)."""
    for n in (70001, 4 * 70000):
        check_segment_kernel(random_queries(2, n, 5, seed=n, max_len=6), n, 5, "product", True, dev)


def test_segment_refuses_bad_arguments(dev):
    from ultra_amd import _lib, query_exec
    words = torch.zeros(64, dtype=torch.int32, device=dev)
    stack = torch.zeros(2, 2, 8, device=dev)
    with pytest.raises(_lib.UltraError, match="depth 2"):
        query_exec.segment(words, 0, 2, 8, "product", torch.zeros(2, 3, 8, device=dev), None, None)
    with pytest.raises(_lib.UltraError, match="fp32"):
        query_exec.segment(words, 0, 2, 8, "product", stack.double(), None, None)
    with pytest.raises(_lib.UltraError, match="symbolic"):
        query_exec.segment(words, 0, 2, 8, "product", stack, None, torch.zeros(2, 8, device=dev), stack.clone(), None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query_exec.segment(words, 0, 2, 8, "product", stack.cpu(), None, None)
    query_exec.segment(words, 0, 0, 8, "product", stack, None, None)       # batch 0: nothing to do


def _compiled_vs_eager(model, graph, query, symbolic):
    from ultra_amd import query_exec
    dev = graph.edge_index.device
    query = query.to(dev)
    with torch.no_grad():
        want = model(graph, query, symbolic_traversal=symbolic)
        want_prob = model.stack.stack[torch.arange(len(want), device=dev), model.stack.SP]
        got, sym = query_exec.execute(model, graph, query, symbolic)
        assert torch.equal(query_exec.forward(model, graph, query, symbolic), want)
    assert torch.equal(got, want)
    if symbolic:
        st = model.symbolic_stack
        assert torch.equal(sym, st.stack[torch.arange(len(want), device=dev), st.SP - 1])
    else:
        assert sym is None
    return want_prob


@pytest.mark.parametrize("logic", LOGICS)
@pytest.mark.parametrize("symbolic", [True, False])
def test_compiled_executor_equals_eager_with_real_weights(dev, logic, symbolic):
    from ultra_amd import query_exec
    g = load()
    model, graph = build_model(g, dev, logic), golden_graph(g, dev)
    _compiled_vs_eager(model, graph, g["query"], symbolic)
    for name in g["id2type"]:
        _compiled_vs_eager(model, graph, type_rows(g, name), symbolic)
    # hence the golden's bound on the probabilities holds for the compiled route
    program = query_exec.compile(g["query"], g["num_nodes"], g["num_relations"])
    prob, _ = query_exec.Executor().run(model, graph, program, symbolic)
    err = (prob.cpu() - g["executor"][(logic, symbolic)]["prob"]).abs()
    per_type = {g["id2type"][t]: float(err[g["type"] == t].max()) for t in range(len(g["id2type"]))}
    assert err.max().item() <= 1e-5, per_type
    assert torch.isfinite(query_exec.logit(prob)).all()


def test_test_queries_compiled_equals_eager(dev):
    from ultra_amd.query_data import QueryDataset
    from ultra_amd.query_eval import test_queries
    g = load()
    ds = QueryDataset(g["nested"], g["type"].tolist(), [set(m.nonzero().flatten().tolist()) for m in g["easy_answer"]],
                      [set(m.nonzero().flatten().tolist()) for m in g["hard_answer"]], g["num_nodes"], g["id2type"])
    model, graph = build_model(g, dev), golden_graph(g, dev)
    eager = test_queries(model, graph, ds, 8, g["id2type"], METRICS, device=dev, compiled=False)
    compiled = test_queries(model, graph, ds, 8, g["id2type"], METRICS, device=dev, compiled=True)
    assert compiled == eager
    assert set(compiled) == set(g["metrics"])
    for k, v in g["metrics"].items():
        assert compiled[k] == pytest.approx(v, rel=1e-4, abs=1e-5), k


def test_executor_issues_no_host_wait(dev):
    from ultra_amd import query_exec
    g = load()
    n, r = g["num_nodes"], g["num_relations"]
    query = plain(g["query"]).to(dev)
    program = query_exec.compile(query, n, r)
    graph = types.SimpleNamespace(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev), num_nodes=n, num_relations=r)
    uq = stub_model("product")
    executor = query_exec.Executor()
    want, want_sym = query_exec.execute(uq, graph, program, True, executor=executor)        # (warm: buffers, pinned block)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    raised = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        got, got_sym = query_exec.execute(uq, graph, program, True, executor=executor)
        ptr, index = query_exec.nonzero_lists(got_sym)
        try:        # control: the interpreter waits for the device at every instruction
            stub_model("product")(graph, query, symbolic_traversal=True)
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not raised:
        pytest.skip("this torch build does not report synchronising calls: the check would pass vacuously")
    assert torch.equal(got, want) and torch.equal(got_sym, want_sym)
    assert int(ptr[-1]) == int((got_sym != 0).sum())


@pytest.mark.parametrize("batch", [1, 28])
@pytest.mark.parametrize("n", [1, 4097, 70000])
def test_nonzero_lists_match_torch_nonzero(dev, batch, n):
    from ultra_amd import _lib, query_exec
    gen = torch.Generator().manual_seed(n + batch)
    x = torch.rand(batch, n, generator=gen) * (torch.rand(batch, n, generator=gen) < 0.3)
    x[0] = 0.0                                          # an empty row (the first: ptr[1] = 0)
    if batch > 3:
        x[3] = 1.0                                      # a full row
        x[batch - 1] = 0.0                              # an empty last row
        x[5, ::7] = float("nan")                        # NaN counts
        x[5, 1::7] = -0.0                               # -0.0 does not
        x[6] = -0.0
        x[7, n - 1] = float("-inf")
    else:
        x[0, n - 1] = float("nan")
        x[0, 0] = -0.0
    xd = x.to(dev)
    sample, col = (x != 0).nonzero().t()
    want_ptr = torch.searchsorted(sample.contiguous(), torch.arange(batch + 1))
    for _ in range(2):
        ptr, index = query_exec.nonzero_lists(xd)
        assert ptr.dtype == index.dtype == torch.int64
        assert torch.equal(ptr.cpu(), want_ptr)
        assert torch.equal(index[:len(col)].cpu(), col)
    counts = torch.empty(batch, dtype=torch.int64, device=dev)
    rc = _lib.lib.ultra_nonzero_lists(xd.data_ptr(), batch, n, counts.data_ptr(), ptr.data_ptr(), index.data_ptr(),
                                      batch * n - 1, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.ULTRA_ERR_INVALID and b"index_out holds" in _lib.lib.ultra_last_error()


def _eager_answers(model, graph, rows, batches, k, filtered):
    """The expected rows of QueryPredictor.answers: eager forward on exactly its batches, selected by the reference."""
    from ultra_amd import predict
    dev = graph.edge_index.device
    n = len(rows)
    ids = torch.empty(n, k, dtype=torch.long)
    scores = torch.empty(n, k)
    count = torch.empty(n, dtype=torch.long)
    for index in batches:
        query = torch.tensor([rows[i] for i in index], dtype=torch.long, device=dev)
        with torch.no_grad():
            logits = model(graph, query, symbolic_traversal=filtered).cpu()
        ptr = known = None
        if filtered:
            st = model.symbolic_stack
            sym = st.stack[torch.arange(len(index), device=dev), st.SP - 1].cpu()
            sample, known = (sym != 0).nonzero().t()
            ptr = torch.searchsorted(sample.contiguous(), torch.arange(len(index) + 1))
        got = predict.filtered_topk_reference(logits, k, ptr, known)
        ids[index], scores[index], count[index] = got
    return ids, scores, count


def _same_answers(got, want):
    return (torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
            and torch.equal(got[1].cpu().view(torch.int32), want[1].view(torch.int32)))


def test_query_predictor_matches_eager_route(dev):
    from ultra_amd import query_predict
    from ultra_amd.ultraquery import Query
    g = load()
    model, graph = build_model(g, dev), golden_graph(g, dev)
    order = torch.randperm(3 * len(g["nested"]), generator=torch.Generator().manual_seed(5)).tolist()
    nested = [g["nested"][i % len(g["nested"])] for i in order]            # six of every type, mixed
    rows = [Query.from_nested(q).tolist() for q in nested]
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4)
    batches = qp.batches(nested)
    assert sorted(i for b in batches for i in b) == list(range(len(nested)))
    assert max(len(b) for b in batches) == 4 and min(len(b) for b in batches) == 2
    assert all(b == sorted(b) for b in batches)                             # input order within a group
    got = qp.answers(nested)
    want = _eager_answers(model, graph, rows, batches, 5, True)
    assert _same_answers(got, want)
    assert bool((got[2] == 5).all())
    # postfix rows give the same answers as nested tuples
    width = max(len(r) for r in rows)
    postfix = torch.tensor([r + [Query.stop] * (width - len(r)) for r in rows], dtype=torch.long)
    assert qp.batches(postfix) == batches
    assert _same_answers(qp.answers(postfix), want)
    # no filter: the plain top-k of the logits
    plain_qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, filtered=False)
    assert _same_answers(plain_qp.answers(nested), _eager_answers(model, graph, rows, batches, 5, False))
    assert not model.training


def test_query_predictor_pads_when_few_candidates_are_left(dev):
    from ultra_amd import query_predict, tasks
    from ultra_amd.data import Data
    g = load()
    heads = torch.tensor([0, 0, 0, 0, 5])
    tails = torch.tensor([1, 2, 3, 4, 0])
    rel = torch.tensor([0, 0, 0, 0, 1])
    tiny = Data(edge_index=torch.stack([torch.cat([heads, tails]), torch.cat([tails, heads])]),
                edge_type=torch.cat([rel, rel + 2]), num_nodes=6, num_relations=4)
    tasks.build_relation_graph(tiny)
    tiny = tiny.to(dev)
    model = build_model(g, dev)
    qp = query_predict.QueryPredictor(model, tiny, k=5, batch_size=4)
    queries = [(0, (0,)), (5, (1, 0))]                      # both entail {1, 2, 3, 4}: candidates 0 and 5
    ids, scores, count = qp.answers(queries)
    assert count.tolist() == [2, 2]
    assert sorted(ids[0, :2].tolist()) == [0, 5] and sorted(ids[1, :2].tolist()) == [0, 5]
    assert bool((ids[:, 2:] == -1).all()) and bool((scores[:, 2:] == float("-inf")).all())
    assert bool(torch.isfinite(scores[:, :2]).all()) and bool((scores[:, 0] >= scores[:, 1]).all())
    rows = [[0, (1 << 58) | 0, 1 << 62, 1 << 62], [5, (1 << 58) | 1, (1 << 58) | 0, 1 << 62]]
    assert _same_answers((ids, scores, count), _eager_answers(model, tiny, rows, qp.batches(queries), 5, True))
