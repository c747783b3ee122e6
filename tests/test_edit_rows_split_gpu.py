"""ultra_rspmm_edit_rows_split on the GPU (csrc/delta_kernels.hip): the hub-row walker -- one workgroup per (touched
row longer than hub_len, outer slice) -- and the split of the touched rows between it and the 16-lane walk.

The expected value never comes from the device: it is the CPU oracle (oracle/rspmm_oracle.py) on the materialised edge list, one
outer slice at a time, with the boundary combined afterwards (the helpers of tests/test_edit_rows_shapes_gpu.py).  `out` starts as
a sentinel fill: the touched rows must equal the oracle under torch.equal, every other element keeps the sentinel's bits.

1. every case of tests/test_edit_rows_shapes_cpu.py (rows of 0 .. 100 edges) at hub_len = -1 (seg_len: no hub), 16 (the rows of 17,
   18, 33 and 100 edges are hubs, the row of 16 is not) and 0 (every touched row with a base edge is a hub);
2. the long row of tests/test_edit_rows_split_cpu.py: 3 * HUB_TILE + 5 base edges, dead slots and added edges at the tile edges;
3. the live count lowered below the hub; 4. a captured launch that serves another row becoming the hub; 5. the layers."""
from types import SimpleNamespace

import pytest
import torch

from oracle import rspmm_oracle
from tests import test_edit_rows_shapes_cpu as shapes
from tests import test_edit_rows_shapes_gpu as small
from tests import test_edit_rows_split_cpu as long_row
from tests.test_verify_live_gpu import dead_mask
from ultra_amd import _lib, rspmm

pytestmark = pytest.mark.gpu

TILE = _lib.HUB_TILE
SENTINEL = small.SENTINEL
HUB_LENS = (-1, 16, 0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """tests/test_edit_rows_shapes_gpu.world: the base graph on the GPU with its reference-order plan; per case its delta, the
    materialised list on the host and the touched rows -- built once, left unchanged."""
    data = shapes.base_graph().to(dev)
    plan = rspmm.Plan(data.edge_index, data.edge_type, shapes.N, shapes.R, exact_order=True)
    cases = {}
    for name, case in shapes.CASES.items():
        delta = shapes.apply_case(data, case)
        mat = delta.materialize()
        touched = delta.rows[:int(delta.count)].long().cpu()
        cases[name] = SimpleNamespace(name=name, delta=delta, index=mat.edge_index.cpu(), kind=mat.edge_type.cpu(), touched=touched)
    return SimpleNamespace(data=data, plan=plan, cases=cases)


def run_split(plan, delta, t, keys, boundary, sum, mul, hub_len):
    buf = torch.full(t.out_shape, SENTINEL, dtype=t.dtype, device=t.x.device)
    out = t.view(buf, t.d)
    kw = {"none": {}, "dense": dict(boundary=t.bnd), "point": dict(point=(t.rows, t.vals))}[boundary]
    got = plan.edit_rows_split(t.rel, t.x, out, delta, keys=keys, sum=sum, mul=mul, hub_len=hub_len, **kw)
    return got, out, buf


def check_small(world, name, t, boundary, sum, mul, hub_len, keys=None, table=None, delta=None, live=None):
    """tests/test_edit_rows_shapes_gpu.check through the split entry."""
    case = world.cases[name]
    what = (name, hub_len, table, boundary, sum, mul, t.d, t.layout, live)
    got, out, buf = run_split(world.plan, case.delta if delta is None else delta, t, keys, boundary, sum, mul, hub_len)
    assert got is out, what
    host = buf.cpu()
    logical = t.view(host, t.d)
    written = case.touched if live is None else case.touched[:max(live, 0)]
    keep = torch.ones(host.shape, dtype=torch.bool)
    t.view(keep, t.d)[:, written] = False
    for s in range(t.B):
        want = small.expected(case, table, s, 0 if t.shared else s, t.d, t.dtype, sum, mul, boundary)[:len(written)]
        have = logical[s][written]
        assert torch.equal(have, want), what + (s, case.touched[(have != want).any(-1).nonzero().flatten()[:8]].tolist())
    small.assert_sentinel(host, keep, what)


def check_small_all(world, dev, name, t, boundary, sum, mul, tables, hub_len):
    if name in shapes.ADD_ONLY:
        assert world.cases[name].delta.num_removed == 0            # no tombstones passed: the add-only kernel's roles
    check_small(world, name, t, boundary, sum, mul, hub_len)
    for table, keys in tables.items():
        check_small(world, name, t, boundary, sum, mul, hub_len, keys=keys, table=table)


def test_the_small_cases_put_edgeless_rows_under_both_walkers():
    """At hub_len = 16 the row of 17 edges is a hub and `r17_all_dead` leaves it with no edge: the hub walker's epilogue; at 0 the
    row of one edge is a hub and `r1_emptied` empties it; the row of NO base edge is never a hub and stays with the 16-lane walk
    (`r0_delta_only`), like the rows of 16 edges and fewer at 16."""
    assert shapes.CASES["r17_all_dead"].survivors == {shapes.ROW_17: 0} and shapes.DEGREES[shapes.ROW_17] == 17 > 16
    assert shapes.CASES["r1_emptied"].survivors == {shapes.ROW_1: 0} and shapes.DEGREES[shapes.ROW_1] == 1 > 0
    assert shapes.DEGREES[shapes.ROW_0] == 0 and "r0_delta_only" in shapes.ADD_ONLY
    assert shapes.DEGREES[shapes.ROW_16] == 16 and "r16_dead_15_the_last" in shapes.CASES
    assert sorted(d for d in shapes.DEGREES.values() if d > 16) == [17, 18, 33, 100] and 100 > TILE      # two tiles


WIDTHS = [(torch.float32, d) for d in (4, 64, 68, 200)] + [(torch.float64, d) for d in (2, 32, 34)]


@pytest.mark.parametrize("hub_len", HUB_LENS)
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
@pytest.mark.parametrize("dtype,d", WIDTHS, ids=["%s-%d" % (str(dtype)[6:], d) for dtype, d in WIDTHS])
def test_small_cases(dev, world, dtype, d, sum, mul, hub_len):
    t = small.device_operands(dev, d, dtype, B=3)
    tables = {table: small.key_tensors(table, 3, dev) for table in shapes.KEY_TABLES}
    for name in shapes.CASES:
        for boundary in small.BOUNDARIES:
            check_small_all(world, dev, name, t, boundary, sum, mul, tables, hub_len)


@pytest.mark.parametrize("hub_len", HUB_LENS)
@pytest.mark.parametrize("layout,dtype,d", [("node_major", torch.float32, 68), ("padded", torch.float64, 34),
                                            ("shared_relation", torch.float32, 68), ("five_slices", torch.float64, 34)])
def test_small_layouts(dev, world, layout, dtype, d, hub_len):
    B = 5 if layout == "five_slices" else 3
    named = layout if layout in small.LAYOUTS else "contiguous"
    t = small.device_operands(dev, d, dtype, B, layout=named, shared_relation=layout == "shared_relation")
    tables = {table: small.key_tensors(table, B, dev) for table in shapes.KEY_TABLES}
    for boundary in small.BOUNDARIES:
        for sum in ("add", "max"):
            check_small_all(world, dev, "everything", t, boundary, sum, "mul", tables, hub_len)


def test_the_split_entry_equals_the_old_entries_and_refuses_what_they_refuse(dev, world):
    """hub_len above every row: bit for bit the three entries; rows that are no whole chunks: None, nothing written."""
    t = small.device_operands(dev, 68, torch.float32, B=3)
    keys = small.key_tensors("keys_8", 3, dev)
    case = world.cases["everything"]
    for use_keys in (None, keys):
        _, _, buf = run_split(world.plan, case.delta, t, use_keys, "dense", "add", "mul", 1 << 40)
        _, _, old = small.run(world.plan, "edit_rows" if use_keys is None else "edit_rows_samples", case.delta, t, keys, "dense", "add", "mul")
        assert torch.equal(buf.view(torch.int32), old.view(torch.int32))
    odd = small.device_operands(dev, 66, torch.float32, B=3)
    for hub_len in HUB_LENS:
        got, _, buf = run_split(world.plan, case.delta, odd, None, "dense", "add", "mul", hub_len)
        host = buf.cpu()
        assert got is None
        small.assert_sentinel(host, torch.ones(host.shape, dtype=torch.bool), hub_len)


# ---- 2. the long row ----
B_LONG = 5
POINT_ROWS = [long_row.HUB, 5, long_row.HUB_B, long_row.HUB, 399]


@pytest.fixture(scope="module")
def long_world(dev):
    data = long_row.base_graph().to(dev)
    plan = rspmm.Plan(data.edge_index, data.edge_type, long_row.N, long_row.R, exact_order=True)
    cases = {}
    for name, case in long_row.CASES.items():
        delta = long_row.apply_case(data, case)
        mat = delta.materialize()
        cases[name] = SimpleNamespace(name=name, delta=delta, index=mat.edge_index.cpu(), kind=mat.edge_type.cpu(),
                                      touched=delta.rows[:int(delta.count)].long().cpu())
        assert long_row.HUB in cases[name].touched.tolist()
    return SimpleNamespace(data=data, plan=plan, cases=cases)


_LONG_VALUES = {}


def long_values(d, dtype):
    if (d, dtype) not in _LONG_VALUES:
        g = torch.Generator().manual_seed(77 * d + int(dtype == torch.float64))
        x, rel, bnd = (torch.randn(B_LONG, n, d, generator=g, dtype=dtype) for n in (long_row.N, long_row.R, long_row.N))
        _LONG_VALUES[d, dtype] = SimpleNamespace(x=x, rel=rel, bnd=bnd, vals=torch.randn(B_LONG, d, generator=g, dtype=dtype))
    return _LONG_VALUES[d, dtype]


_LONG_WANT = {}


def long_expected(case, keyed, s, d, dtype, sum, mul, boundary, index=None, kind=None, touched=None):
    """The touched rows of slice s by the CPU oracle on the materialised list without the edges slice s's keys name, then the
    boundary.  The oracle's rows are cached before the boundary per (case, keyed, slice, width, dtype, sum, mul)."""
    v = long_values(d, dtype)
    touched = case.touched if touched is None else touched
    key = (case.name, keyed, s, d, dtype, sum, mul)
    if index is not None or key not in _LONG_WANT:
        cached = index is None
        index, kind = (case.index, case.kind) if cached else (index, kind)
        if keyed:
            dead = dead_mask(index, kind, long_row.KEYS[s])
            index, kind = index[:, ~dead], kind[~dead]
        full = rspmm_oracle.generalized_rspmm(index, kind, torch.ones(index.shape[1], dtype=dtype), v.rel[s], v.x[s], sum=sum, mul=mul)
        if cached:
            _LONG_WANT[key] = full
    else:
        full = _LONG_WANT[key]
    want = full[touched].clone()
    if boundary == "none":
        return want
    if boundary == "dense":
        bnd = v.bnd[s][touched]
    else:
        bnd = torch.zeros(len(touched), d, dtype=dtype)
        bnd[touched == POINT_ROWS[s]] = v.vals[s]
    return want + bnd if sum == "add" else (torch.max(want, bnd) if sum == "max" else torch.min(want, bnd))


def long_operands(dev, d, dtype):
    v = long_values(d, dtype)
    return SimpleNamespace(d=d, dtype=dtype, B=B_LONG, layout="contiguous", shared=False, rel=v.rel.to(dev), x=v.x.to(dev),
                           bnd=v.bnd.to(dev), vals=v.vals.to(dev), rows=torch.tensor(POINT_ROWS, device=dev),
                           out_shape=(B_LONG, long_row.N, d), view=lambda buf, d: buf)


def long_keys(dev):
    packed = torch.tensor(long_row.KEYS, dtype=torch.int32, device=dev)
    return tuple(packed[:, :, i].contiguous() for i in range(3))


def check_long(plan, case, t, boundary, sum, mul, hub_len, keys=None, delta=None, written=None, index=None, kind=None):
    what = (case.name, hub_len, keys is not None, boundary, sum, mul, t.d)
    got, out, buf = run_split(plan, case.delta if delta is None else delta, t, keys, boundary, sum, mul, hub_len)
    assert got is out, what
    host = buf.cpu()
    written = case.touched if written is None else written
    keep = torch.ones(host.shape, dtype=torch.bool)
    keep[:, written] = False
    for s in range(t.B):
        want = long_expected(case, keys is not None, s, t.d, t.dtype, sum, mul, boundary, index=index, kind=kind, touched=written)
        have = host[s][written]
        assert torch.equal(have, want), what + (s, written[(have != want).any(-1).nonzero().flatten()[:8]].tolist())
    small.assert_sentinel(host, keep, what)


@pytest.mark.parametrize("sum,mul", [("add", "mul"), ("max", "add"), ("min", "mul")])
@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (torch.float32, 68), (torch.float64, 34)],
                         ids=["float32-64", "float32-68", "float64-34"])
def test_the_long_row(dev, long_world, dtype, d, sum, mul):
    """The hub of 3 * HUB_TILE + 5 base edges through the hub walker (hub_len = -1: it exceeds seg_len; HUB_B does not and goes
    with the 16-lane walk; 16: both are hubs): every case, every boundary, with and without the per-slice keys."""
    t = long_operands(dev, d, dtype)
    keys = long_keys(dev)
    for hub_len in (-1, 16):
        for case in long_world.cases.values():
            for boundary in small.BOUNDARIES:
                check_long(long_world.plan, case, t, boundary, sum, mul, hub_len)
                check_long(long_world.plan, case, t, boundary, sum, mul, hub_len, keys=keys)


# ---- 3. the live count ----
def test_a_live_count_below_the_hub_leaves_its_row_alone(dev, long_world):
    t = long_operands(dev, 68, torch.float32)
    case = long_world.cases["added_and_dead"]
    delta = long_row.apply_case(long_world.data, long_row.CASES["added_and_dead"])
    touched = case.touched.tolist()
    at = touched.index(long_row.HUB)
    assert delta.rows[:int(delta.count)].tolist() == touched and at >= 1
    for live in (at, 1, 0, -3):
        delta.count.fill_(live)
        check_long(long_world.plan, case, t, "dense", "add", "mul", 16, delta=delta, written=case.touched[:max(live, 0)])
    delta.count.fill_(at + 1)                                         # ... and the hub is the last live row
    check_long(long_world.plan, case, t, "dense", "add", "mul", 16, delta=delta, written=case.touched[:at + 1])


# ---- 4. capture ----
def test_a_captured_launch_serves_another_row_becoming_the_hub(dev, long_world):
    data, plan = long_world.data, long_world.plan
    t = long_operands(dev, 64, torch.float32)
    delta = rspmm.GraphDelta(data, capacity=long_row.CAPACITY)
    delta.remove(*shapes.fact(*long_row.slot(long_row.HUB, TILE)))
    buf = torch.empty(t.out_shape, dtype=t.dtype, device=dev)

    def step():
        assert plan.edit_rows_split(t.rel, t.x, buf, delta, boundary=t.bnd, hub_len=16) is buf

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    case = SimpleNamespace(name="captured", delta=delta)
    for edit in ("hub_a", "hub_b", "added"):
        if edit == "hub_b":                                           # a fact of ANOTHER long row, no new capture
            delta.remove(*shapes.fact(*long_row.slot(long_row.HUB_B, TILE - 1)))
        elif edit == "added":
            delta.add(*zip(*[shapes.fact(long_row.HUB_B, 1, 4), shapes.fact(*long_row.ADD_EQUAL)]))
        touched = delta.rows[:int(delta.count)].long().cpu()
        assert (long_row.HUB_B in touched.tolist()) == (edit != "hub_a") and long_row.HUB in touched.tolist()
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        host = buf.cpu()
        mat = delta.materialize()
        keep = torch.ones(host.shape, dtype=torch.bool)
        keep[:, touched] = False
        for s in range(B_LONG):
            want = long_expected(case, False, s, 64, torch.float32, "add", "mul", "dense", index=mat.edge_index.cpu(),
                                 kind=mat.edge_type.cpu(), touched=touched)
            assert torch.equal(host[s][touched], want), (edit, s)
        small.assert_sentinel(host, keep, edit)


# ---- 5. through the layers ----
def counted(monkeypatch, names):
    calls = dict.fromkeys(names, 0)
    for name in names:
        def wrapper(*args, _name=name, _fn=getattr(_lib.lib, name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, wrapper)
    return calls


SPLIT, OLD = "ultra_rspmm_edit_rows_split", ("ultra_rspmm_delta_rows", "ultra_rspmm_edit_rows", "ultra_rspmm_edit_rows_samples")


@pytest.mark.parametrize("switch", [True, False])
def test_predictor_edits_into_a_hub(dev, monkeypatch, switch):
    """tests/test_retract_gpu.py's graph: node 7 heads 300 triples, a row longer than seg_len.  Facts added into and retracted from
    the hub: tails and verify_tails equal the fresh predictor on materialized(), bit for bit, by either route."""
    from tests import test_retract_gpu as retract
    import os
    from ultra_amd import models, predict, synthetic, tasks
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(retract.GOLDEN, "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    data = tasks.build_relation_graph(retract.live_graph().to(dev))
    assert rspmm.get_plan(data.edge_index, data.edge_type, retract.N, 2 * retract.R_DIRECT).has_hub_rows
    monkeypatch.setattr(rspmm, "EDIT_ROWS_HUB_SPLIT", switch)
    calls = counted(monkeypatch, (SPLIT,) + OLD)
    h, t, r = data.target_triples[:6].unbind(-1)
    live = predict.Predictor(model, data, k=5, batch_size=3, delta_capacity=24)
    facts = [torch.tensor(v, device=dev) for v in zip(*retract.FACTS[:3])]          # two of them into the hub row
    assert live.add_facts(*facts) == 3
    for state in ("added", "retracted"):
        if state == "retracted":
            live.remove_facts(*[torch.tensor([v], device=dev) for v in retract.HUB_TRIPLE])
        fresh = predict.Predictor(model, live.materialized(), k=5, batch_size=3)
        assert retract.same_answers(live.tails(h, r), fresh.tails(h, r)), state
        got, want = live.verify_tails(h, r, t), fresh.verify_tails(h, r, t)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), state
        fresh.close()
    live.close()
    if switch:
        assert calls[SPLIT] > 0 and all(calls[name] == 0 for name in OLD), calls
    else:
        assert calls[SPLIT] == 0 and all(calls[name] > 0 for name in OLD), calls


@pytest.mark.parametrize("switch", [True, False])
def test_query_predictor_edits_into_a_hub(dev, monkeypatch, switch):
    from tests.test_query_exec_cpu import load
    from tests.test_query_live_gpu import same_topk
    from tests.test_ultraquery_gpu import build_model, golden_graph
    from ultra_amd import query_predict, tasks
    from ultra_amd.data import Data
    g = load()
    model, graph = build_model(g, dev), golden_graph(g, dev)
    n, half = int(graph.num_nodes), int(graph.num_relations) // 2
    # node 0 heads 300 more triples: its row of the served direction grows past seg_len
    tails = torch.arange(300, device=dev) % (n - 1) + 1
    kinds = torch.arange(300, device=dev) % 2
    heads = torch.zeros(300, dtype=torch.long, device=dev)
    index = torch.cat([graph.edge_index, torch.stack([heads, tails]), torch.stack([tails, heads])], dim=1)
    kind = torch.cat([graph.edge_type, kinds, kinds + half])
    hub = tasks.build_relation_graph(Data(edge_index=index, edge_type=kind, num_nodes=n, num_relations=2 * half))
    monkeypatch.setattr(rspmm, "EDIT_ROWS_HUB_SPLIT", switch)
    calls = counted(monkeypatch, (SPLIT,) + OLD)
    qp = query_predict.QueryPredictor(model, hub, k=5, batch_size=8, delta_capacity=16)
    assert qp.add_facts([0, 5], [3, 0], [150, 0]) == 2
    assert bool((qp.remove_facts([0, 0], [0, 1], [1, 2]) >= 1).all())
    nested = list(g["nested"])[:8]
    fresh = query_predict.QueryPredictor(model, qp.materialized(), k=5, batch_size=8)
    assert same_topk(qp.answers(nested), fresh.answers(nested))
    if switch:
        assert calls[SPLIT] > 0 and all(calls[name] == 0 for name in OLD), calls
    else:
        assert calls[SPLIT] == 0 and calls["ultra_rspmm_edit_rows"] > 0, calls
