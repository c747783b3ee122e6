"""Retracting facts from a served graph on the GPU: tombstones on the cached plan of the base graph, with or without
added facts beside them.  Every result on (base graph, delta) equals the same call on the materialised graph -- [base edges that
carry no tombstone ; direct edges ; inverse edges] -- on a fresh reference-order plan, bit for bit: the engine call
(ultra_rspmm_edit_rows), the layer, Ultra.forward and the Predictor.

The graph is the one of test_live_graph_gpu.py -- 300 nodes, 8 direct relations, node 7 heads 300 triples (a chain row), row 30 has
exactly the two edges to 120 and 180, relation 7 is stated once as (200, 7, 201) -- plus one triple stated twice and one self loop."""
import ctypes
import os

import pytest
import torch

from ultra_amd import _lib, layers, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N, R_DIRECT, BATCH = 300, 8, 3
HUB, EMPTY, MERGE_ROW = 7, 299, 30
DUP, LOOP, ONCE = (210, 3, 211), (220, 4, 220), (200, 7, 201)          # (h, r, t)
ROW_30 = [(MERGE_ROW, 0, 120), (MERGE_ROW, 1, 180)]
TWICE, NOWHERE = (40, 6, 41), (EMPTY, 5, EMPTY)


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
    more = torch.tensor([DUP, DUP, LOOP])                              # a triple stated twice, a self loop
    return (torch.cat([h, ph, more[:, 0]]), torch.cat([t, pt, more[:, 2]]),
            torch.cat([r, torch.zeros(pad, dtype=torch.long), more[:, 1]]))


TRIPLES = _triples()
_AT_100 = int(((TRIPLES[0] == HUB) & (TRIPLES[1] == 100)).nonzero()[0])
HUB_TRIPLE = (HUB, int(TRIPLES[2][_AT_100]), 100)                      # the hub's edge at column 100

# (h, r, t): the added facts of test_live_graph_gpu.py
FACTS = [
    (HUB, 0, 50), (HUB, 6, 100),                       # the hub row, the second at the column of HUB_TRIPLE
    (60, 1, HUB), (EMPTY, 1, 10), (20, 2, 20),
    (int(TRIPLES[0][0]), int(TRIPLES[2][0]), int(TRIPLES[1][0])),
    (MERGE_ROW, 3, 5), (MERGE_ROW, 4, 150), (MERGE_ROW, 5, 250),       # row 30: below, between and above its base sources
    TWICE, TWICE, (EMPTY, 2, EMPTY),
]

# name -> (facts added first, facts retracted then, the counts remove() returns)
CASES = {
    "hub": ([], [HUB_TRIPLE], None),
    "hub_with_facts": (FACTS, [HUB_TRIPLE], None),
    "row_30_emptied": ([], ROW_30, [1, 1]),
    "row_30_delta_only": (FACTS, ROW_30, [1, 1]),
    "stated_twice": ([], [DUP], [2]),
    "self_loop": ([], [LOOP], [1]),
    "stated_once": ([], [ONCE], [1]),
    "added_twice": ([TWICE, TWICE], [TWICE], [2]),
    "nowhere": ([], [NOWHERE], [0]),
    "all": (FACTS, [HUB_TRIPLE] + ROW_30 + [DUP, LOOP, ONCE, NOWHERE, TWICE, DUP], None),
}


def live_graph():
    h, t, r = TRIPLES
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + R_DIRECT]),
                num_nodes=N, num_relations=2 * R_DIRECT, target_triples=torch.stack([h, t, r], dim=-1)[:16])
    return tasks.build_relation_graph(data)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def edge_count(data, h, r, t):
    return int(((data.edge_index[0] == h) & (data.edge_index[1] == t) & (data.edge_type == r)).sum())


@pytest.fixture(scope="module")
def world(dev):
    """(base graph on the GPU, its reference-order plan), every property the cases rely on asserted."""
    data = tasks.build_relation_graph(live_graph().to(dev))
    plan = rspmm.Plan(data.edge_index, data.edge_type, N, 2 * R_DIRECT, exact_order=True)
    assert data.edge_index.shape[1] == 2 * 1253
    assert plan.info()["n_chain_row"] >= 1                 # the hub row is a chain row
    degree = torch.bincount(data.edge_index[0], minlength=N)
    assert int(degree[HUB]) > 256 and int(degree[EMPTY]) == 0
    rows_30 = data.edge_index[0] == MERGE_ROW
    assert sorted(zip(data.edge_index[1][rows_30].tolist(), data.edge_type[rows_30].tolist())) == [(120, 0), (180, 1)]
    assert edge_count(data, *HUB_TRIPLE) >= 1
    assert edge_count(data, *DUP) == 2 and edge_count(data, DUP[2], DUP[1] + R_DIRECT, DUP[0]) == 2
    assert edge_count(data, *LOOP) == 1 and edge_count(data, LOOP[0], LOOP[1] + R_DIRECT, LOOP[0]) == 1
    assert int((data.edge_type == 7).sum()) == 1 and edge_count(data, *ONCE) == 1
    assert edge_count(data, *TWICE) == 0 and edge_count(data, *NOWHERE) == 0
    return data, plan


@pytest.fixture(scope="module")
def cases(world):
    """name -> (delta, materialised graph, a fresh reference-order plan of it, touched-row mask): built once, left unchanged."""
    data, _ = world
    out = {}
    for name, (added, gone, counts) in CASES.items():
        delta = rspmm.GraphDelta(data, capacity=24)
        if added:
            delta.add(*zip(*added))
        took = delta.remove(*zip(*gone))
        if counts is not None:
            assert took.tolist() == counts, name
        mat = delta.materialize(data)
        touched = torch.zeros(N, dtype=torch.bool, device=data.edge_index.device)
        touched[delta.rows[:int(delta.count)].long()] = True
        assert int(touched.sum()) == int(delta.count), name
        out[name] = (delta, mat, rspmm.Plan(mat.edge_index, mat.edge_type, N, 2 * R_DIRECT, exact_order=True), touched)
    # the cases are what they say
    assert int((out["row_30_emptied"][1].edge_index[0] == MERGE_ROW).sum()) == 0              # no surviving edge
    delta_only, mat_only = out["row_30_delta_only"][:2]
    rows_30 = (mat_only.edge_index[0] == MERGE_ROW).nonzero()
    assert len(rows_30) == 3 and int(rows_30.min()) >= mat_only.edge_index.shape[1] - 2 * len(delta_only)     # delta edges only
    assert out["hub"][0].num_removed == 2 and len(out["hub"][0]) == 0
    assert out["self_loop"][0].num_removed == 2 and int(out["self_loop"][0].count) == 1      # both keys in one row
    assert out["self_loop"][0].dead_ptr[:2].tolist() == [0, 2]
    assert out["stated_twice"][1].edge_index.shape[1] == data.edge_index.shape[1] - 4
    assert out["stated_once"][0].relation_graph is not data.relation_graph                    # relation 7 lost its last edge
    assert out["added_twice"][0].num_removed == 0 and not out["added_twice"][0].edited
    assert not out["nowhere"][0].edited and int(out["nowhere"][0].count) == 0
    assert bool(out["all"][3][HUB]) and bool(out["all"][3][MERGE_ROW]) and out["all"][0].num_removed == 12
    return out


def operands(dev, d, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BATCH, N, d, generator=g, dtype=dtype).to(dev)
    rel = torch.randn(BATCH, 2 * R_DIRECT, d, generator=g, dtype=dtype).to(dev)
    bnd = torch.randn(BATCH, N, d, generator=g, dtype=dtype).to(dev)
    rows = torch.tensor([MERGE_ROW, HUB, 5], device=dev)   # the point sits ON the emptied row in sample 0 and OFF it in the others
    vals = torch.randn(BATCH, d, generator=g, dtype=dtype).to(dev)
    return x, rel, bnd, rows, vals


def check_engine(dev, world, cases, sum, mul, d, dtype=torch.float32, names=None, kinds=("dense", "point", "none")):
    data, plan = world
    x, rel, bnd, rows, vals = operands(dev, d, seed=3, dtype=dtype)
    for kind, kwargs in (("dense", dict(boundary=bnd)), ("point", dict(point=(rows, vals))), ("none", dict())):
        if kind not in kinds:
            continue
        base = plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
        assert base is not None, kind
        for name in names or CASES:
            delta, _, mat_plan, touched = cases[name]
            out = base.clone()
            got = plan.edit_rows(rel, x, out, delta, sum=sum, mul=mul, **kwargs)
            assert got is out, (name, kind)
            want = mat_plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
            assert torch.equal(out, want), (name, kind, (out != want).any(-1).nonzero()[:8].tolist())
            assert bool(torch.isfinite(out).all()), (name, kind)      # (an edge-less row holds the finite start value, no infinity)
            # nothing else was written: the untouched rows hold the base output's bits
            assert torch.equal(out[:, ~touched].view(torch.int64 if dtype == torch.float64 else torch.int32),
                               base[:, ~touched].view(torch.int64 if dtype == torch.float64 else torch.int32)), (name, kind)
            if delta.num_removed:
                assert not torch.equal(out[:, touched], base[:, touched]), (name, kind)


@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
def test_engine_equals_a_fresh_plan_of_the_materialised_graph(dev, world, cases, sum, mul, d):
    check_engine(dev, world, cases, sum, mul, d)


@pytest.mark.parametrize("sum", ["add", "max"])
def test_engine_in_fp64(dev, world, cases, sum):
    # (a point boundary under min / max is an fp32 form of plan.forward: fp64 takes it under add only)
    check_engine(dev, world, cases, sum, "mul", 32, dtype=torch.float64, names=["all", "row_30_emptied"],
                 kinds=("dense", "point", "none") if sum == "add" else ("dense", "none"))


def test_without_tombstones_the_entry_is_delta_rows(dev, world):
    """removed == NULL computes exactly ultra_rspmm_delta_rows; so does an add-only delta through Plan.edit_rows."""
    data, plan = world
    delta = rspmm.GraphDelta(data, capacity=16)
    delta.add(*zip(*FACTS))
    x, rel, bnd, _, _ = operands(dev, 64, seed=4)
    base = plan.forward(rel, x, boundary=bnd)
    want = plan.delta_rows(rel, x, base.clone(), delta, boundary=bnd)
    assert not torch.equal(want, base)
    assert torch.equal(plan.edit_rows(rel, x, base.clone(), delta, boundary=bnd), want)
    out = base.clone()
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, bnd, out)]
    rc = _lib.lib.ultra_rspmm_edit_rows(plan._h, 0, 0, _lib.F32, mats[0], mats[1], mats[2], None, mats[3],
                                        ctypes.byref(delta.operand()), None, _lib.stream_of(x))
    assert rc == _lib.ULTRA_OK
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_unsupported_calls_launch_nothing(dev, world, cases):
    data, plan = world
    delta = cases["all"][0]
    x, rel, bnd, _, _ = operands(dev, 64, seed=4)
    out = plan.forward(rel, x, boundary=bnd)
    base = out.clone()
    loose = rspmm.Plan(data.edge_index, data.edge_type, N, 2 * R_DIRECT, exact_order=False)
    assert loose.edit_rows(rel, x, out, delta, boundary=bnd) is None               # a general-walk plan
    assert plan.edit_rows(rel, x, out, delta, boundary=bnd, mul="rotate") is None  # rotate messages
    odd = torch.zeros(BATCH, N, 68, device=dev)[:, :, 1:65]                        # rows that start off a 16-byte boundary
    assert plan.edit_rows(rel, odd, out, delta, boundary=bnd) is None
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), base.view(torch.int32))


@pytest.mark.parametrize("aggr,msg", [("sum", "distmult"), ("max", "distmult"), ("mean", "distmult"), ("sum", "transe")])
def test_layer_equals_the_layer_on_the_materialised_graph(dev, world, cases, aggr, msg):
    data, _ = world
    torch.manual_seed(2)
    layer = layers.GeneralizedRelationalConv(64, 64, 2 * R_DIRECT, 64, message_func=msg, aggregate_func=aggr,
                                             layer_norm=True).to(dev).eval()
    x, _, bnd, rows, vals = operands(dev, 64, seed=5)
    size = (N, N)
    with torch.no_grad():
        for name in ("all", "row_30_emptied", "hub"):
            delta, mat, _, _ = cases[name]
            for boundary in (bnd, layers.PointBoundary(rows, vals, N)):
                got = layer(x, vals, boundary, data.edge_index, data.edge_type, size, delta=delta)
                want = layer(x, vals, boundary, mat.edge_index, mat.edge_type, size)
                base = layer(x, vals, boundary, data.edge_index, data.edge_type, size)
                assert torch.equal(got, want), (name, type(boundary).__name__)
                assert not torch.equal(got, base), name


@pytest.fixture(scope="module")
def model(dev):
    state = torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt"))
    net = models.Ultra(**synthetic.default_model_cfg())
    net.load_state_dict(state)
    return net.to(dev).eval()


def test_model_equals_the_model_on_the_materialised_graph(dev, world, cases, model):
    data, _ = world
    batch = tasks.all_negative(data, data.target_triples[:BATCH])
    with torch.no_grad():
        base = [model(data, b) for b in batch]
        for name in ("hub", "all", "stated_once"):       # (`all` and `stated_once`: the relation graph changed too)
            delta, mat, _, _ = cases[name]
            for b, base_score in zip(batch, base):
                got = model(data, b, delta=delta)
                assert torch.equal(got, model(mat, b)), name
                assert not torch.equal(got, base_score), name
        assert torch.equal(model(data, batch[0], delta=cases["nowhere"][0]), base[0])        # nothing held: the normal path


def same_answers(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and torch.equal(got[2], want[2]))


def test_predictor_serves_the_live_graph(dev, world, model):
    data, _ = world
    h, t, r = data.target_triples[:7].unbind(-1)
    facts = [torch.tensor(v, device=dev) for v in zip(*FACTS)]
    gone = [torch.tensor(v, device=dev) for v in zip(*([HUB_TRIPLE] + ROW_30 + [DUP]))]
    live = predict.Predictor(model, data, k=5, batch_size=BATCH, delta_capacity=24)
    live.tails(h, r), live.heads(t, r)                        # captures with the empty delta: the normal path
    assert live.add_facts(facts[0][:8], facts[1][:8], facts[2][:8]) == 8
    live.tails(h, r)                                          # ... with an add-only delta: ultra_rspmm_delta_rows
    add_only = dict(live._steps)
    assert live.remove_facts(gone[0][:3], gone[1][:3], gone[2][:3]).tolist() == [edge_count(data, *HUB_TRIPLE), 1, 1]
    assert live.data is data and live.delta.num_removed == 6
    fresh = predict.Predictor(model, live.delta.materialize(data), k=5, batch_size=BATCH)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))
    assert same_answers(live.heads(t, r), fresh.heads(t, r))
    assert live._steps["tail"] is not add_only["tail"]        # the first tombstone: the captured launches differ
    for a, b in zip(live.tails_above(h, r, 0.0), fresh.tails_above(h, r, 0.0)):
        assert torch.equal(a, b)
    # a retracted fact's tail is a candidate again (every entity above a floor no score reaches: all candidates)
    qh, qr, tail = gone[0][1:2], gone[1][1:2], int(gone[2][1])
    assert tail not in predict.Predictor(model, data, batch_size=BATCH).tails_above(qh, qr, -1e30)[1].tolist()
    live_k = predict.Predictor(model, data, k=200, batch_size=BATCH, delta_capacity=24)
    live_k.remove_facts(gone[0][:3], gone[1][:3], gone[2][:3])
    fresh_k = predict.Predictor(model, live_k.delta.materialize(data), k=200, batch_size=BATCH)
    assert same_answers(live_k.tails(qh, qr), fresh_k.tails(qh, qr))
    got, want = live_k.tails_above(qh, qr, -1e30), fresh_k.tails_above(qh, qr, -1e30)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and tail in got[1].tolist()
    # further edits that keep the relation graph: the SAME captured steps serve them
    steps, graph = dict(live._steps), live.delta.relation_graph
    assert live.remove_facts(gone[0][3:], gone[1][3:], gone[2][3:]).tolist() == [2]
    assert live.add_facts(facts[0][8:], facts[1][8:], facts[2][8:]) == 12
    assert live.remove_facts(*NOWHERE).tolist() == [0]
    assert live.delta.relation_graph is graph
    fresh = predict.Predictor(model, live.delta.materialize(data), k=5, batch_size=BATCH)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))
    assert same_answers(live.heads(t, r), fresh.heads(t, r))
    assert set(live._steps) == set(steps) and all(live._steps[key] is steps[key] for key in steps)
    # compact() folds the tombstones: the materialised graph becomes the served one
    mat = live.delta.materialize(data)
    live.compact()
    assert not live.delta.edited and torch.equal(live.data.edge_index, mat.edge_index) and torch.equal(live.data.edge_type, mat.edge_type)
    assert same_answers(live.tails(h, r), fresh.tails(h, r))
    live.close(), fresh.close(), live_k.close(), fresh_k.close()


def test_the_call_records_into_a_graph_and_follows_the_buffers(dev, world):
    data, plan = world
    delta = rspmm.GraphDelta(data, capacity=24)
    delta.remove(*HUB_TRIPLE)
    x, rel, bnd, _, _ = operands(dev, 64, seed=6)
    out = torch.empty(BATCH, N, 64, device=dev)

    def step():
        plan.forward(rel, x, boundary=bnd, out=out)
        assert plan.edit_rows(rel, x, out, delta, boundary=bnd) is out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for edit in (None, "remove", "add"):
        if edit == "remove":
            delta.remove(*zip(*(ROW_30 + [LOOP])))
        elif edit == "add":
            delta.add(*zip(*FACTS))
        out.zero_()
        graph.replay()
        mat = delta.materialize(data)
        want = rspmm.Plan(mat.edge_index, mat.edge_type, N, 2 * R_DIRECT, exact_order=True).forward(rel, x, boundary=bnd)
        assert torch.equal(out, want), edit
