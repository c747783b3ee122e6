"""Serving a changing graph on the GPU: added facts as a delta on the cached plan of the base graph.  Every result
on (base graph, delta) equals the same call on the materialised graph -- [base edges ; direct edges ; inverse edges] -- on a
fresh reference-order plan, bit for bit: the engine call (ultra_rspmm_delta_rows), the layer, Ultra.forward and the Predictor.

The graph: 300 nodes, 8 direct relations, 2,500 edges with inverses; node 7 heads 300 triples (a row longer than seg_len = 256:
a chain row), node 299 has no edge, node 30's sources lie in [120, 180], relation 7 is stated once.  The 12 facts hit the hub
row (also at a column the hub already has), the edge-less row, a self loop, a copy of an existing edge, one row with sources
below, between and above its base sources, and one fact stated twice."""
import os

import pytest
import torch

from ultra_amd import layers, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N, R_DIRECT, BATCH = 300, 8, 3
HUB, EMPTY, MERGE_ROW = 7, 299, 30


def _triples():
    g = torch.Generator().manual_seed(17)
    count = 946
    h = torch.randint(0, EMPTY, (count,), generator=g)
    t = torch.randint(0, EMPTY, (count,), generator=g)
    r = torch.randint(0, R_DIRECT - 1, (count,), generator=g)          # relations 0 .. 6
    keep = (h != MERGE_ROW) & (t != MERGE_ROW)
    h, t, r = h[keep], t[keep], r[keep]
    hub_t = torch.cat([torch.tensor([100]), torch.randint(0, EMPTY, (299,), generator=g)])
    hub_t[hub_t == MERGE_ROW] = 31
    extra_h = torch.tensor([MERGE_ROW, MERGE_ROW, 200])
    extra_t = torch.tensor([120, 180, 201])
    extra_r = torch.tensor([0, 1, 7])                                  # relation 7: one triple, (200, 7, 201)
    h = torch.cat([h, torch.full((300,), HUB), extra_h])
    t = torch.cat([t, hub_t, extra_t])
    r = torch.cat([r, torch.randint(0, R_DIRECT - 1, (300,), generator=g), extra_r])
    pad = 1250 - len(h)                                                # (the rows filtered out above, drawn again elsewhere)
    ph = torch.randint(100, 118, (pad,), generator=g)
    pt = torch.randint(200, 290, (pad,), generator=g)
    return torch.cat([h, ph]), torch.cat([t, pt]), torch.cat([r, torch.zeros(pad, dtype=torch.long)])


TRIPLES = _triples()

# (h, r, t)
FACTS = [
    (HUB, 0, 50),                 # into the hub row (and row 50)
    (HUB, 6, 100),                # the hub row again, at a column it already has (base edges first at equal col)
    (60, 1, HUB),                 # the hub row through the inverse edge
    (EMPTY, 1, 10),               # a row with no in-edges
    (20, 2, 20),                  # a self loop
    (int(TRIPLES[0][0]), int(TRIPLES[2][0]), int(TRIPLES[1][0])),       # a copy of an existing edge: the first base triple
    (MERGE_ROW, 3, 5),            # row 30: a source below its base sources ...
    (MERGE_ROW, 4, 150),          # ... between them ...
    (MERGE_ROW, 5, 250),          # ... and above
    (40, 6, 41),                  # the same fact ...
    (40, 6, 41),                  # ... twice
    (EMPTY, 2, EMPTY),            # a self loop on the edge-less row
]
RELGRAPH_FACT = (EMPTY, 7, 10)    # relation 7 gets a new head and a new tail: the relation graph changes


def live_graph():
    h, t, r = TRIPLES
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + R_DIRECT]),
                num_nodes=N, num_relations=2 * R_DIRECT, target_triples=torch.stack([h, t, r], dim=-1)[:16])
    return tasks.build_relation_graph(data)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """(base graph on the GPU, a delta with the 12 facts, its materialised graph, the base plan)."""
    data = tasks.build_relation_graph(live_graph().to(dev))      # (on the GPU: the relation graph keeps its adjacency bits)
    delta = rspmm.GraphDelta(data, capacity=16)
    assert delta.add(*zip(*FACTS)) == 12
    mat = delta.materialize(data)
    assert mat.edge_index.shape[1] == data.edge_index.shape[1] + 24 == 2524
    plan = rspmm.Plan(data.edge_index, data.edge_type, N, 2 * R_DIRECT, exact_order=True)
    assert plan.info()["n_chain_row"] >= 1                 # the hub row is a chain row: the case cannot silently be missing
    degree = torch.bincount(data.edge_index[0], minlength=N)
    assert int(degree[HUB]) > 256 and int(degree[EMPTY]) == 0
    cols = data.edge_index[1][data.edge_index[0] == MERGE_ROW]
    assert int(cols.min()) == 120 and int(cols.max()) == 180
    return data, delta, mat, plan


def operands(dev, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BATCH, N, d, generator=g).to(dev)
    rel = torch.randn(BATCH, 2 * R_DIRECT, d, generator=g).to(dev)
    bnd = torch.randn(BATCH, N, d, generator=g).to(dev)
    rows = torch.tensor([HUB, EMPTY, 5], device=dev)       # the point boundary sits on a touched row in two samples
    vals = torch.randn(BATCH, d, generator=g).to(dev)
    return x, rel, bnd, rows, vals


@pytest.fixture(scope="module")
def mat_plan(world):
    _, _, mat, _ = world
    return rspmm.Plan(mat.edge_index, mat.edge_type, N, 2 * R_DIRECT, exact_order=True)


@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
def test_engine_equals_a_fresh_plan_of_the_materialised_graph(dev, world, mat_plan, sum, mul, d):
    data, delta, mat, plan = world
    x, rel, bnd, rows, vals = operands(dev, d, seed=3)
    touched = torch.zeros(N, dtype=torch.bool, device=dev)
    touched[delta.rows[:int(delta.count)].long()] = True
    assert int(touched.sum()) == int(delta.count) and bool(touched[HUB]) and bool(touched[EMPTY])
    for kind, kwargs in (("dense", dict(boundary=bnd)), ("point", dict(point=(rows, vals))), ("none", dict())):
        out = plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
        assert out is not None, kind
        base = out.clone()
        got = plan.delta_rows(rel, x, out, delta, sum=sum, mul=mul, **kwargs)
        assert got is out, kind
        want = mat_plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
        assert torch.equal(out, want), (kind, (out != want).any(-1).nonzero()[:8].tolist())
        # nothing else was written: the untouched rows hold the base output's bits
        assert torch.equal(out[:, ~touched].view(torch.int32), base[:, ~touched].view(torch.int32)), kind
        assert not torch.equal(out[:, touched], base[:, touched]), kind


def test_empty_delta_leaves_the_output_alone(dev, world):
    data, _, _, plan = world
    empty = rspmm.GraphDelta(data, capacity=16)
    x, rel, bnd, _, _ = operands(dev, 64, seed=4)
    out = plan.forward(rel, x, boundary=bnd)
    base = out.clone()
    assert plan.delta_rows(rel, x, out, empty, boundary=bnd) is out
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), base.view(torch.int32))


def test_unsupported_calls_launch_nothing(dev, world):
    data, delta, _, plan = world
    x, rel, bnd, _, _ = operands(dev, 64, seed=4)
    out = plan.forward(rel, x, boundary=bnd)
    base = out.clone()
    loose = rspmm.Plan(data.edge_index, data.edge_type, N, 2 * R_DIRECT, exact_order=False)
    assert loose.delta_rows(rel, x, out, delta, boundary=bnd) is None               # a general-walk plan
    assert plan.delta_rows(rel, x, out, delta, boundary=bnd, mul="rotate") is None  # rotate messages
    odd = torch.zeros(BATCH, N, 68, device=dev)[:, :, 1:65]                         # rows that start off a 16-byte boundary
    assert plan.delta_rows(rel, odd, out, delta, boundary=bnd) is None
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), base.view(torch.int32))


@pytest.mark.parametrize("aggr,msg", [("sum", "distmult"), ("max", "distmult"), ("mean", "distmult"), ("sum", "transe"),
                                      ("mean", "transe")])
def test_layer_equals_the_layer_on_the_materialised_graph(dev, world, aggr, msg):
    data, delta, mat, _ = world
    torch.manual_seed(2)
    layer = layers.GeneralizedRelationalConv(64, 64, 2 * R_DIRECT, 64, message_func=msg, aggregate_func=aggr,
                                             layer_norm=True).to(dev).eval()
    x, _, bnd, rows, vals = operands(dev, 64, seed=5)
    query = vals
    size = (N, N)
    with torch.no_grad():
        for boundary in (bnd, layers.PointBoundary(rows, vals, N)):
            got = layer(x, query, boundary, data.edge_index, data.edge_type, size, delta=delta)
            want = layer(x, query, boundary, mat.edge_index, mat.edge_type, size)
            base = layer(x, query, boundary, data.edge_index, data.edge_type, size)
            assert torch.equal(got, want), type(boundary).__name__
            assert not torch.equal(got, base)


@pytest.mark.parametrize("aggr,msg", [("pna", "distmult"), ("sum", "rotate")])
def test_layer_kinds_without_a_delta_route_raise(dev, world, aggr, msg):
    data, delta, _, _ = world
    layer = layers.GeneralizedRelationalConv(64, 64, 2 * R_DIRECT, 64, message_func=msg, aggregate_func=aggr).to(dev).eval()
    x, _, bnd, _, vals = operands(dev, 64, seed=5)
    with torch.no_grad(), pytest.raises(RuntimeError, match="graph delta"):
        layer(x, vals, bnd, data.edge_index, data.edge_type, (N, N), delta=delta)
    sum_layer = layers.GeneralizedRelationalConv(64, 64, 2 * R_DIRECT, 64, aggregate_func="sum").to(dev)
    with pytest.raises(RuntimeError, match="no_grad"):      # grad mode
        sum_layer(x, vals, bnd, data.edge_index, data.edge_type, (N, N), delta=delta)
    with torch.no_grad(), pytest.raises(RuntimeError, match="keep masks"):
        sum_layer._forward_impl(x, vals, bnd, data.edge_index, data.edge_type, (N, N),
                                edge_weight=torch.ones(BATCH, data.edge_index.shape[1], device=dev), edge_keep=True, delta=delta)


@pytest.fixture(scope="module")
def model(dev):
    state = torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt"))
    net = models.Ultra(**synthetic.default_model_cfg())
    net.load_state_dict(state)
    return net.to(dev).eval()


def test_model_equals_the_model_on_the_materialised_graph(dev, world, model):
    data, _, _, _ = world
    batch = tasks.all_negative(data, data.target_triples[:BATCH])
    delta = rspmm.GraphDelta(data, capacity=16)
    delta.add(*zip(*FACTS))
    # the 12 facts use relations that already met at their entities: the relation graph object is kept ...
    assert delta.relation_graph is data.relation_graph
    with torch.no_grad():
        base = [model(data, b) for b in batch]
        for b, base_score in zip(batch, base):
            got = model(data, b, delta=delta)
            want = model(delta.materialize(data), b)
            assert torch.equal(got, want)
            assert not torch.equal(got, base_score)
        assert torch.equal(model(data, batch[0], delta=rspmm.GraphDelta(data, 4)), base[0])      # an empty delta: the normal path
        # ... and one fact that gives relation 7 a new head and tail changes it
        delta.add(*RELGRAPH_FACT)
        assert delta.relation_graph is not data.relation_graph
        assert not torch.equal(delta.relation_graph.adjacency_bits, data.relation_graph.adjacency_bits)
        mat = delta.materialize(data)
        fresh = tasks.build_relation_graph(Data(edge_index=mat.edge_index, edge_type=mat.edge_type, num_nodes=N,
                                                num_relations=2 * R_DIRECT)).relation_graph
        assert torch.equal(fresh.adjacency_bits, delta.relation_graph.adjacency_bits)
        for b in batch:
            assert torch.equal(model(data, b, delta=delta), model(mat, b))


def same_answers(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and torch.equal(got[2], want[2]))


def test_predictor_serves_the_live_graph(dev, world, model):
    data, _, _, _ = world
    h, t, r = data.target_triples[:7].unbind(-1)
    facts = [torch.tensor(v, device=dev) for v in zip(*FACTS)]
    live = predict.Predictor(model, data, k=5, batch_size=BATCH, delta_capacity=16)
    live.tails(h, r), live.heads(t, r)                        # captures with the empty delta: the normal path
    assert live.add_facts(facts[0][:8], facts[1][:8], facts[2][:8]) == 8
    fresh = predict.Predictor(model, live.delta.materialize(data), k=5, batch_size=BATCH)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))
    assert same_answers(live.heads(t, r), fresh.heads(t, r))
    for a, b in zip(live.tails_above(h, r, 0.0), fresh.tails_above(h, r, 0.0)):
        assert torch.equal(a, b)
    # an added fact's tail is a known answer now
    qh, qr = facts[0][:1], facts[1][:1]
    ids, _, count = predict.Predictor(model, data, k=200, batch_size=BATCH).tails(qh, qr)
    assert int(facts[2][0]) in ids[0, :int(count[0])].tolist()
    live_k = predict.Predictor(model, data, k=200, batch_size=BATCH, delta_capacity=16)
    live_k.add_facts(facts[0][:8], facts[1][:8], facts[2][:8])
    ids, _, count = live_k.tails(qh, qr)
    assert int(facts[2][0]) not in ids[0, :int(count[0])].tolist()
    # further facts that keep the relation graph: the SAME captured steps serve them
    steps = dict(live._steps)
    graph = live.delta.relation_graph
    assert live.add_facts(facts[0][8:], facts[1][8:], facts[2][8:]) == 12
    assert live.delta.relation_graph is graph
    fresh = predict.Predictor(model, live.delta.materialize(data), k=5, batch_size=BATCH)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))
    assert same_answers(live.heads(t, r), fresh.heads(t, r))
    assert set(live._steps) == set(steps) and all(live._steps[key] is steps[key] for key in steps)
    live.close(), fresh.close(), live_k.close()


def test_predictor_compacts_beyond_its_capacity(dev, world, model):
    data, _, _, _ = world
    h, t, r = data.target_triples[:5].unbind(-1)
    facts = [torch.tensor(v, device=dev) for v in zip(*FACTS)]
    live = predict.Predictor(model, data, k=5, batch_size=BATCH, delta_capacity=4)
    assert live.add_facts(facts[0][:3], facts[1][:3], facts[2][:3]) == 3
    live.tails(h, r)
    assert live.add_facts(facts[0][3:6], facts[1][3:6], facts[2][3:6]) == 0        # 6 > 4: compacted
    assert live.data.edge_index.shape[1] == data.edge_index.shape[1] + 12 and len(live.delta) == 0
    assert live.add_facts(facts[0][6:8], facts[1][6:8], facts[2][6:8]) == 2
    six = rspmm.GraphDelta(data, 16)
    six.add(facts[0][:6], facts[1][:6], facts[2][:6])
    assert torch.equal(live.data.edge_index, six.materialize(data).edge_index)     # compaction IS materialisation
    assert torch.equal(live.data.edge_type, six.materialize(data).edge_type)
    # the graph served now: the compacted graph is the base, facts 6 and 7 its delta
    served = predict.Predictor(model, live.delta.materialize(live.data), k=5, batch_size=BATCH)
    assert same_answers(live.tails(h, r), served.tails(h, r))
    assert same_answers(live.heads(t, r), served.heads(t, r))
    live.close(), served.close()


def test_the_call_records_into_a_graph_and_follows_the_delta(dev, world):
    data, _, _, plan = world
    delta = rspmm.GraphDelta(data, capacity=16)
    delta.add(*zip(*FACTS[:4]))
    x, rel, bnd, _, _ = operands(dev, 64, seed=6)
    out = torch.empty(BATCH, N, 64, device=dev)

    def step():
        plan.forward(rel, x, boundary=bnd, out=out)
        assert plan.delta_rows(rel, x, out, delta, boundary=bnd) is out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for upto in (4, 12):
        if upto > len(delta):
            delta.add(*zip(*FACTS[len(delta):upto]))
        out.zero_()
        graph.replay()
        mat = delta.materialize(data)
        want = rspmm.Plan(mat.edge_index, mat.edge_type, N, 2 * R_DIRECT, exact_order=True).forward(rel, x, boundary=bnd)
        assert torch.equal(out, want), upto
