"""Leave-one-out verification on a graph that holds edits, on the GPU: ultra_rspmm_edit_rows_samples against fresh
reference-order plans of every slice's filtered materialised list, the capture, the layer, and Predictor.verify_* against
predict.verify_reference on the materialised graph -- bit for bit, with the delta left a delta.

The kernel's graph: 48 nodes, 6 relations (3 direct), 300 directed edges with duplicates; rows 40 .. 45 have exactly 0, 1, 15, 16,
17 and 40 edges (the 16-pair trip of the base cursor and the DELTA_BATCH boundary lie between them), rows 0 .. 39 share the rest."""
import ctypes

import pytest
import torch

from tests.test_oracle_model import load_golden
from ultra_amd import _lib, layers, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

TOL = 1e-4      # tests/test_models_gpu.py
N, R, R_DIRECT, N_OUTER = 48, 6, 3, 4
ROW_0, ROW_1, ROW_15, ROW_16, ROW_17, ROW_40 = 40, 41, 42, 43, 44, 45
DEGREES = {ROW_0: 0, ROW_1: 1, ROW_15: 15, ROW_16: 16, ROW_17: 17, ROW_40: 40}
SENTINEL = -7.0


def _edges():
    """(row, col, type) of the base graph, in edge order."""
    g = torch.Generator().manual_seed(23)
    fixed = {                                                 # the edges the cases below name, per special row
        ROW_1: [(20, 4)],
        ROW_15: [(7, 2)],                                     # restated by the delta: a key hits both
        ROW_16: [(11, 1)],                                    # tombstoned: a key hits an edge that is also tombstoned
        ROW_17: [(30, 0), (31, 2), (31, 5)],                  # a base-only hit; two types at one col for the type = -1 key
        ROW_40: [(12, 0), (12, 0), (13, 1), (13, 1)],         # (12, 0) twice: tombstoned; (13, 1) twice: a key hits a duplicate
    }
    edges = []
    for row, degree in DEGREES.items():
        own = list(fixed.get(row, []))
        while len(own) < degree:
            col, kind = int(torch.randint(0, 40, (1,), generator=g)), int(torch.randint(0, R, (1,), generator=g))
            if col not in (7, 11, 12, 13, 30, 31, 47):       # (the named cols stay what `fixed` says)
                own.append((col, kind))
        edges += [(row, col, kind) for col, kind in own]
    rest = 300 - len(edges) - 6
    rows = torch.randint(0, 40, (rest,), generator=g).tolist()
    cols = torch.randint(0, N - 1, (rest,), generator=g).tolist()      # (col 47 is used by no base edge)
    kinds = torch.randint(0, R, (rest,), generator=g).tolist()
    edges += list(zip(rows, cols, kinds))
    edges += edges[100:106]                                   # six more duplicates among the ordinary rows
    order = torch.randperm(len(edges), generator=g).tolist()
    return [edges[i] for i in order]


EDGES = _edges()
ROW_2_FACT = next((row, kind, col) for row, col, kind in EDGES if row == 2 and kind < R_DIRECT)       # (h, r, t)
FACTS = [(ROW_0, 0, 5), (ROW_1, 1, 6), (ROW_15, 2, 7), (ROW_16, 0, 8), (ROW_17, 1, 9), (ROW_40, 2, 10)]     # (h, r, t)
GONE = [(ROW_16, 1, 11), (ROW_40, 0, 12), ROW_2_FACT]
# per outer slice its dead (row, col, type) keys; (0, 0, -2)-style padding is avoided: a padded key is one that hits nothing
KEYS = [
    [(ROW_17, 30, 0), (ROW_1, 6, 1), (ROW_15, 7, 2), (3, 1, 0)],              # base only; delta only; both; an untouched row
    [(ROW_40, 13, 1), (ROW_16, 11, 1), (ROW_17, 47, 5), (ROW_17, 31, -1)],    # a duplicate; also tombstoned; nothing; any type
    [(ROW_0, 5, 0), (ROW_1, 20, 4), (ROW_1, 6, 1), (ROW_40, 10, -1)],         # rows 40 and 41 edge-less in this slice alone
    [(47, 47, 0), (ROW_0, 5, 1), (ROW_16, 8, 3), (5, ROW_0, 3)],              # nothing (x3: wrong row, type, direction) ; F0's inverse
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def dead_mask(edge_index, edge_type, keys):
    """edge e is dead for the slice iff one of its keys has the edge's row and col and (a negative type or the edge's type)."""
    dead = torch.zeros(edge_index.shape[1], dtype=torch.bool, device=edge_index.device)
    for row, col, kind in keys:
        hit = (edge_index[0] == row) & (edge_index[1] == col)
        if kind >= 0:
            hit = hit & (edge_type == kind)
        dead |= hit
    return dead


def key_tensors(keys, dev):
    packed = torch.tensor(keys, dtype=torch.int32, device=dev)           # (n_outer, per_sample, 3)
    return tuple(packed[:, :, i].contiguous() for i in range(3))


def edited(data, facts=FACTS, gone=GONE):
    delta = rspmm.GraphDelta(data, capacity=16)
    if facts:
        delta.add(*zip(*facts))
    if gone:
        delta.remove(*zip(*gone))
    return delta


@pytest.fixture(scope="module")
def world(dev):
    """The base graph and its plan, the delta (6 facts, 3 retracted facts), the materialised list, per slice the fresh plan of
    its filtered list, the touched-row mask -- every property the cases rely on asserted; built once, left unchanged."""
    row, col, kind = (torch.tensor(v) for v in zip(*EDGES))
    data = Data(edge_index=torch.stack([row, col]), edge_type=kind, num_nodes=N, num_relations=R).to(dev)
    assert data.edge_index.shape[1] == 300
    degree = torch.bincount(data.edge_index[0], minlength=N)
    assert {r: int(degree[r]) for r in DEGREES} == DEGREES
    assert len(set(EDGES)) < len(EDGES) and not bool((data.edge_index[1] == 47).any())
    plan = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=True)
    delta = edited(data)
    assert len(delta) == 6 and delta.num_removed >= 3
    mat = delta.materialize(data)
    touched = torch.zeros(N, dtype=torch.bool, device=dev)
    touched[delta.rows[:int(delta.count)].long()] = True
    assert all(bool(touched[r]) for r in DEGREES) and not bool(touched[3]) and int(touched.sum()) < N
    base_dead = [dead_mask(data.edge_index, data.edge_type, keys) for keys in KEYS]
    mat_dead = [dead_mask(mat.edge_index, mat.edge_type, keys) for keys in KEYS]
    n_base = data.edge_index.shape[1] - (mat.edge_index.shape[1] - 12)        # base edges the tombstones took
    assert n_base == 4                                        # (43, 11, 1), (45, 12, 0) twice, row 2's fact
    parts = [rspmm.Plan(mat.edge_index[:, ~d], mat.edge_type[~d], N, R, exact_order=True) for d in mat_dead]
    rows_of = lambda s, row: int(((mat.edge_index[0] == row) & ~mat_dead[s]).sum())
    # the cases are what they say
    assert int(base_dead[0].sum()) == 2 and int(mat_dead[0].sum()) == 4       # (44,30,0) | F1 | (42,7,2) in both | row 3: a base edge or none
    assert int(mat_dead[0][-12:].sum()) == 2
    assert int(base_dead[1].sum()) == 5 and int(mat_dead[1].sum()) == 4       # (45,13,1) x2, (43,11,1) tombstoned, (44,31,*) x2
    assert rows_of(2, ROW_0) == 0 and rows_of(2, ROW_1) == 0 and rows_of(0, ROW_0) == 1 and rows_of(1, ROW_1) == 2
    assert int(mat_dead[3].sum()) == 1 and int(base_dead[3].sum()) == 0       # only (5, 40, 3), the inverse edge of fact 0
    return dict(data=data, plan=plan, delta=delta, mat=mat, touched=touched, parts=parts, base_dead=base_dead)


def operands(dev, d, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_OUTER, N, d, generator=g, dtype=dtype).to(dev)
    rel = torch.randn(N_OUTER, R, d, generator=g, dtype=dtype).to(dev)
    bnd = torch.randn(N_OUTER, N, d, generator=g, dtype=dtype).to(dev)
    rows = torch.tensor([ROW_15, 3, ROW_0, ROW_1], device=dev)      # slice 2: the point ON a row that is edge-less there; slice 3: off
    vals = torch.randn(N_OUTER, d, generator=g, dtype=dtype).to(dev)
    return x, rel, bnd, rows, vals


def slice_forward(part, s, rel, x, sum, mul, kind, bnd, rows, vals):
    """Plan.forward of slice s on the fresh plan of its filtered list.  A point boundary the plan does not take in closed form
    (min / max in fp64) goes in as the tensor it stands for: zeros but for the point's row."""
    if kind == "dense":
        return part.forward(rel[s:s + 1], x[s:s + 1], boundary=bnd[s:s + 1], sum=sum, mul=mul)
    if kind == "none":
        return part.forward(rel[s:s + 1], x[s:s + 1], sum=sum, mul=mul)
    out = part.forward(rel[s:s + 1], x[s:s + 1], sum=sum, mul=mul, point=(rows[s:s + 1], vals[s:s + 1]))
    if out is None:
        as_tensor = torch.zeros_like(x[s:s + 1])
        as_tensor[0, rows[s]] = vals[s]
        out = part.forward(rel[s:s + 1], x[s:s + 1], boundary=as_tensor, sum=sum, mul=mul)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
def test_kernel_equals_fresh_plans_of_every_slices_filtered_list(dev, world, sum, mul, d, dtype):
    plan, delta, touched = world["plan"], world["delta"], world["touched"]
    x, rel, bnd, rows, vals = operands(dev, d, seed=3, dtype=dtype)
    keys = key_tensors(KEYS, dev)
    for kind, kwargs in (("dense", dict(boundary=bnd)), ("point", dict(point=(rows, vals))), ("none", dict())):
        out = torch.full((N_OUTER, N, d), SENTINEL, dtype=dtype, device=dev)
        got = plan.edit_rows_samples(rel, x, out, delta, keys, sum=sum, mul=mul, **kwargs)
        assert got is out, kind
        want = torch.cat([slice_forward(world["parts"][s], s, rel, x, sum, mul, kind, bnd, rows, vals) for s in range(N_OUTER)])
        assert torch.equal(out[:, touched], want[:, touched]), (kind, (out != want)[:, touched].any(-1).nonzero()[:8].tolist())
        assert bool((out[:, ~touched] == SENTINEL).all()), kind              # nothing else was written
        assert bool(torch.isfinite(out).all()), kind                         # (an edge-less row holds the finite start value)
        # the keys acted, slice by slice: without them the touched rows are other numbers (a sum; a max may not miss an edge)
        if sum == "add":
            plain = plan.edit_rows(rel, x, torch.full_like(out, SENTINEL), delta, sum=sum, mul=mul, **kwargs)
            assert all(not torch.equal(out[s], plain[s]) for s in range(N_OUTER)), kind
        if kind != "point":
            # ... and behind the per-sample masked walk of the base plan the whole output is each slice's filtered graph
            keep = (~torch.stack(world["base_dead"])).to(dtype)
            full = plan.forward(rel, x, edge_weight=keep, sum=sum, mul=mul, keep=True, **kwargs)
            assert plan.edit_rows_samples(rel, x, full, delta, keys, sum=sum, mul=mul, **kwargs) is full
            assert torch.equal(full, want), kind


def raw_call(plan, rel, x, bnd, out, delta, removed, keys):
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, bnd, out)]
    return _lib.lib.ultra_rspmm_edit_rows_samples(plan._h, 0, 0, _lib.F32, mats[0], mats[1], mats[2], None, mats[3],
                                                  ctypes.byref(delta.operand()), removed,
                                                  None if keys is None else ctypes.byref(keys), _lib.stream_of(x))


def test_without_tombstones_and_with_bad_keys(dev, world):
    data, plan = world["data"], world["plan"]
    delta = edited(data, gone=[])                              # add-only
    x, rel, bnd, _, _ = operands(dev, 64, seed=4)
    row, col, kind = key_tensors(KEYS, dev)
    want = plan.edit_rows_samples(rel, x, torch.full_like(x, SENTINEL), delta, (row, col, kind), boundary=bnd)
    mat = delta.materialize(data)
    touched = delta.rows[:int(delta.count)].long()
    for s in range(N_OUTER):
        dead = dead_mask(mat.edge_index, mat.edge_type, KEYS[s])
        fresh = rspmm.Plan(mat.edge_index[:, ~dead], mat.edge_type[~dead], N, R, exact_order=True)
        assert torch.equal(want[s, touched], fresh.forward(rel[s:s + 1], x[s:s + 1], boundary=bnd[s:s + 1])[0, touched]), s
    good = _lib.UltraSampleKeys(row.data_ptr(), col.data_ptr(), kind.data_ptr(), row.shape[1])
    out = torch.full_like(x, SENTINEL)
    assert raw_call(plan, rel, x, bnd, out, delta, None, good) == _lib.ULTRA_OK          # removed == NULL: no tombstones
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    base = out.clone()
    for per_sample in (0, 9):
        bad = _lib.UltraSampleKeys(row.data_ptr(), col.data_ptr(), kind.data_ptr(), per_sample)
        assert raw_call(plan, rel, x, bnd, out, delta, None, bad) == _lib.ULTRA_ERR_INVALID
        assert b"per_sample" in _lib.lib.ultra_last_error()
    assert raw_call(plan, rel, x, bnd, out, delta, None, None) == _lib.ULTRA_ERR_INVALID
    loose = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=False)
    assert loose.edit_rows_samples(rel, x, out, delta, (row, col, kind), boundary=bnd) is None      # as edit_rows: a general-walk plan
    assert plan.edit_rows_samples(rel, x, out, delta, (row, col, kind), boundary=bnd, mul="rotate") is None
    with pytest.raises(RuntimeError, match="per_sample|1 .. 8"):
        plan.edit_rows_samples(rel, x, out, delta, tuple(t.repeat(1, 3) for t in (row, col, kind)), boundary=bnd)
    torch.cuda.synchronize()
    assert torch.equal(out, base)                                                         # nothing was launched


def test_the_call_records_into_a_graph_and_follows_the_buffers(dev, world):
    data, plan = world["data"], world["plan"]
    delta = edited(data, facts=FACTS[:5])
    x, rel, bnd, _, _ = operands(dev, 64, seed=6)
    keys = key_tensors(KEYS, dev)
    keep = torch.ones(N_OUTER, data.edge_index.shape[1], device=dev)
    out = torch.empty(N_OUTER, N, 64, device=dev)

    def load(listed):
        for buf, new in zip(keys, key_tensors(listed, dev)):
            buf.copy_(new)
        keep.copy_((~torch.stack([dead_mask(data.edge_index, data.edge_type, k) for k in listed])).float())

    def step():
        plan.forward(rel, x, edge_weight=keep, boundary=bnd, keep=True, out=out)
        assert plan.edit_rows_samples(rel, x, out, delta, keys, boundary=bnd) is out

    load(KEYS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for change in (False, True):
        if change:      # a fact more, other keys: the same buffers, the same recorded launches
            delta.add(*FACTS[5])
            load(KEYS[::-1])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        out.zero_()
        step()
        torch.cuda.synchronize()
        assert torch.equal(replayed, out), change
        mat = delta.materialize(data)
        listed = KEYS[::-1] if change else KEYS
        for s in range(N_OUTER):
            dead = dead_mask(mat.edge_index, mat.edge_type, listed[s])
            fresh = rspmm.Plan(mat.edge_index[:, ~dead], mat.edge_type[~dead], N, R, exact_order=True)
            assert torch.equal(replayed[s:s + 1], fresh.forward(rel[s:s + 1], x[s:s + 1], boundary=bnd[s:s + 1])), (change, s)


@pytest.mark.parametrize("aggr,msg", [("sum", "distmult"), ("max", "distmult"), ("sum", "transe")])
def test_layer_equals_the_layer_on_each_samples_filtered_graph(dev, world, aggr, msg):
    data, delta, mat = world["data"], world["delta"], world["mat"]
    torch.manual_seed(2)
    layer = layers.GeneralizedRelationalConv(64, 64, R, 64, message_func=msg, aggregate_func=aggr, layer_norm=True).to(dev).eval()
    x, _, bnd, rows, vals = operands(dev, 64, seed=5)
    keys = key_tensors(KEYS, dev)
    keep = (~torch.stack(world["base_dead"])).float()
    size = (N, N)
    with torch.no_grad():
        for boundary in (bnd, layers.PointBoundary(rows, vals, N)):
            got = layer._forward_impl(x, vals, boundary, data.edge_index, data.edge_type, size, edge_weight=keep, edge_keep=True,
                                      delta=delta, sample_keys=keys)
            dense_boundary = boundary if torch.is_tensor(boundary) else boundary.dense()
            for s in range(N_OUTER):
                dead = dead_mask(mat.edge_index, mat.edge_type, KEYS[s])
                want = layer(x[s:s + 1], vals[s:s + 1], dense_boundary[s:s + 1], mat.edge_index[:, ~dead], mat.edge_type[~dead], size)
                assert torch.equal(got[s:s + 1], want), (type(boundary).__name__, s)
            assert not torch.equal(got, layer(x, vals, boundary, data.edge_index, data.edge_type, size, delta=delta))
        with pytest.raises(RuntimeError, match="sample_keys"):
            layer._forward_impl(x, vals, bnd, data.edge_index, data.edge_type, size, edge_weight=keep, edge_keep=True, delta=delta)


# ---- the Predictor: the setup of test_verify_gpu.py ----
GRAPH_EDGES = [16, 35, 10, 23]      # tests/test_verify_gpu.py
# (h, r, t) stated nowhere in the graph, picked with the CPU oracle (oracle/ultra_oracle_model.py on the materialised graph with
# the golden ultra_3g sum weights): stated, its tail's logit is -1.7815; verified without itself, -0.8483 -- moved by 0.93
JUST_STATED = (3, 1, 25)
N_FACTS, VERIFY_BS = 11, 4


@pytest.fixture(scope="module")
def served(dev):
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=400, num_triple=3000, num_relation_base=5, num_test=21, seed=3)
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    facts = torch.stack([data.edge_index[0], data.edge_type, data.edge_index[1]], dim=-1)      # (h, r, t)
    stated = {tuple(f) for f in facts.tolist()}
    assert JUST_STATED not in stated
    absent = [(h, r, t) for h, t, r in data.target_triples.tolist() if (h, r, t) not in stated and (h, r, t) != JUST_STATED]
    return model, data.to(dev), [tuple(f) for f in facts.tolist()], absent


def assert_verified(got, want, what):
    for name, a, b in zip(("score", "rank", "num_negative"), got, want):
        a, b = a.cpu(), b.cpu()
        if name == "score":
            print("%s score: max |d| = %g" % (what, (a - b).abs().max().item()))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert a.dtype == torch.int64 and torch.equal(a, b), "%s %s: %s vs %s" % (what, name, a.tolist(), b.tolist())


def plan_of_facts(facts, absent):
    """What is stated, what is retracted, and the 11 facts to verify."""
    restated, retracted = facts[GRAPH_EDGES[0]], facts[GRAPH_EDGES[1]]
    first = [JUST_STATED, restated]                           # stated before the first capture
    later = absent[0]                                         # ... and after it
    gone = [retracted, absent[0]]                             # a base fact (tombstones) and a stated one (out of the delta)
    nowhere = absent[1]
    verify = [JUST_STATED, restated, retracted, nowhere, absent[0], facts[GRAPH_EDGES[2]], facts[GRAPH_EDGES[3]],
              facts[0], facts[9], facts[19], facts[31]]
    assert len(verify) == N_FACTS
    return first, later, gone, nowhere, verify


def test_predictor_verifies_on_the_live_graph(dev, served):
    model, gdata, facts, absent = served
    first, later, gone, nowhere, verify = plan_of_facts(facts, absent)
    h, r, t = (torch.tensor(v, device=dev) for v in zip(*verify))
    live = predict.Predictor(model, gdata, batch_size=VERIFY_BS, delta_capacity=16)
    live.verify_tails(h, r, t)                                # no edit held: the keep rows' route, captured
    unedited = live._steps["verify_tail"]
    assert live.add_facts(*zip(*first)) == 2
    got = live.verify_tails(h, r, t)
    step = live._steps["verify_tail"]
    assert step is not unedited and len(step.graphs) == 1 and step.keys is not None      # the first edits: another route
    assert live.delta.edited and live.data is gdata and len(live.delta) == 2
    assert_verified(got, predict.verify_reference(model, live.materialized(), live.filter_graph, h, r, t, "tail"), "added tail")
    # a further fact that keeps the relation-graph object: no plan, no capture
    graph = live.delta.relation_graph
    assert live.add_facts(*later) == 3 and live.delta.relation_graph is graph
    got = live.verify_tails(h, r, t)
    assert live._steps["verify_tail"] is step and live.delta.edited and len(live.delta) == 3
    assert_verified(got, predict.verify_reference(model, live.materialized(), live.filter_graph, h, r, t, "tail"), "one more fact")
    # the first tombstone: the layers' fix-up reads other arrays, the step is made again
    took = live.remove_facts(*zip(*gone)).tolist()
    assert took[0] >= 1 and took[1] == 1 and live.delta.num_removed >= 1 and len(live.delta) == 2
    mat = live.materialized()
    want = {mode: predict.verify_reference(model, mat, live.filter_graph, h, r, t, mode) for mode in ("tail", "head")}
    eager = predict.Predictor(model, gdata, batch_size=VERIFY_BS, delta_capacity=16, use_graph=False)
    eager.add_facts(*zip(*(first + [later])))
    eager.remove_facts(*zip(*gone))
    for mode in ("tail", "head"):
        call = live.verify_tails if mode == "tail" else live.verify_heads
        got = call(h, r, t)
        assert_verified(got, want[mode], "captured " + mode)
        assert_verified(call(h, r, t), got, "replayed " + mode)
        assert_verified((eager.verify_tails if mode == "tail" else eager.verify_heads)(h, r, t), got, "eager " + mode)
    assert live._steps["verify_tail"] is not step and len(live._steps["verify_tail"].graphs) == 1
    assert eager._steps == {} and not live._eager_only
    for p in (live, eager):                                   # still a delta beside the base graph's plan
        assert p.delta.edited and p.data is gdata and len(p.delta) == 2 and p.delta.num_removed >= 1
    # the mask acts on a DELTA edge: the just-stated fact scores otherwise when it sees itself (the oracle: by 0.93) ...
    with torch.no_grad():
        plain = model(gdata, predict._candidates(gdata, h, r, "tail"), delta=live.delta).gather(1, t.unsqueeze(-1)).flatten()
    score = live.verify_tails(h, r, t)[0]
    moved = (plain - score).abs()
    print("just stated: live %.4f, verified %.4f; restated base fact moved by %.4f" % (float(plain[0]), float(score[0]), float(moved[1])))
    assert float(moved[0]) > 10 * TOL and float(moved[1]) > 10 * TOL
    # ... and a fact stated nowhere, like a retracted one, sees the whole live graph: exactly the plain live forward
    assert verify[3] == nowhere and torch.equal(score[2:5].view(torch.int32), plain[2:5].view(torch.int32))
    live.close()


def test_predictor_with_reserved_rows_verifies_a_fact_about_a_new_entity(dev, served):
    model, gdata, facts, absent = served
    first, later, gone, nowhere, verify = plan_of_facts(facts, absent)
    live = predict.Predictor(model, gdata, batch_size=VERIFY_BS, delta_capacity=16, entity_capacity=8)
    new_id = int(live.add_entities(1)[0])
    assert new_id == gdata.num_nodes
    about_new = [(new_id, 2, 7), (11, 0, new_id)]
    live.add_facts(*zip(*(first + about_new)))
    live.remove_facts(*zip(*gone[:1]))
    verify = verify[:9] + about_new
    h, r, t = (torch.tensor(v, device=dev) for v in zip(*verify))
    fresh = predict.Predictor(model, live.materialized(), batch_size=VERIFY_BS)
    assert fresh.data.num_nodes == new_id + 1 and not (fresh.delta is not None and fresh.delta.edited)
    for mode in ("tail", "head"):
        got = (live.verify_tails if mode == "tail" else live.verify_heads)(h, r, t)
        assert_verified(got, (fresh.verify_tails if mode == "tail" else fresh.verify_heads)(h, r, t), "new entity " + mode)
        assert int(got[2].max()) < new_id + 1                 # ranked among the live ids only
    # with reserved rows DESIGN.md 19's rule stays: the edits were folded in first; the slot count and the live count stay
    assert not live.delta.edited and live.num_slots == gdata.num_nodes + 8
    assert live.num_entities == new_id + 1 and int(live.live_count) == new_id + 1 and not live._eager_only
    live.close(), fresh.close()
