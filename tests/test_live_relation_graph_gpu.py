"""A relation graph kept current in place on the GPU.

The two entry points that read a byte adjacency handed in as an operand -- ultra_nbf_dense_layer_adjacency against
ultra_nbf_dense_layer, ultra_nbf_dense_layer0_adjacency against ultra_nbf_layer0, each on a fresh reference-order plan of the edge
list the bytes stand for, BIT FOR BIT -- at n = 15 (a ragged tile), 16 (exactly one), 17 (a tile boundary), 33 (past the 32-row
update tile) and 70 (five 16-row tiles: the four-tile form with a ragged last group).  Then the live object itself: its byte
adjacency against the export of a fresh plan after a sequence of additions, and Predictor(live_relation_graph=True) against a
fresh Predictor on the materialised graph while the relation-graph object and every captured step stay the same objects -- at
2 R' = 30, 32 and 34 relation-graph nodes, 60 entities, 400 edges, golden ultra_3g weights (test_relation_grow_gpu.py's setup)."""
import os

import pytest
import torch
from torch import nn

from ultra_amd import _lib, live, models, predict, rspmm, synthetic, tasks

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROW_COUNTS = (15, 16, 17, 33, 70)
N, K = 60, 3
SLOT_COUNTS = (15, 16, 17)      # R': 2 R' = 30, 32, 34


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits_equal(a, b):
    """torch.equal on the bit patterns: a -0 is not a +0."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the two entry points against the plan's ----
_CASES = {}


def case(n, dev):
    """Random cells (4, n, n) at fill 0.4 with node n // 2 isolated (no cell in its row or column: a reserved slot), as bit
    matrices, as the byte adjacency, and as a fresh reference-order plan of the emitted edge list.  Built once per n."""
    if n not in _CASES:
        g = torch.Generator().manual_seed(1000 + n)
        cells = torch.rand(4, n, n, generator=g) < 0.4
        iso = n // 2
        cells[:, iso, :] = False
        cells[:, :, iso] = False
        cells[0, 0, n - 1] = cells[2, 0, n - 1] = True      # (the last column is reached, through two types)
        words = (n + 31) // 32
        padded = torch.zeros(4, n, words * 32, dtype=torch.long)
        padded[:, :, :n] = cells
        packed = (padded.view(4, n, words, 32) << torch.arange(32)).sum(-1)
        adj = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32).to(dev)
        counts = cells.sum(-1).flatten().to(dev)
        emitted = tasks.relation_graph_from_bits(adj, counts)
        want_edges = cells.nonzero()
        assert torch.equal(emitted.edge_type.cpu(), want_edges[:, 0]) and torch.equal(emitted.edge_index.cpu(), want_edges[:, 1:].t())
        plan = rspmm.Plan(emitted.edge_index, emitted.edge_type, n, 4, exact_order=True, dense=True)
        assert plan.dense is not None and plan.exact
        a_ex = tasks.relation_graph_dense_adjacency(adj)
        assert torch.equal(a_ex.cpu(), plan.dense.export(_lib.ARR_DENSE_ORDER))
        _CASES[n] = (cells, a_ex, plan, iso)
    return _CASES[n]


def layer_operands(dev, n, bs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, n, 64, generator=g).to(dev)
    rel = (torch.randn(bs, 4, 64, generator=g) * 0.1).to(dev)
    point = ((torch.arange(bs) * 7 + n - 1) % n).to(dev), torch.randn(bs, 64, generator=g).to(dev)
    tensor_bnd = torch.randn(bs, n, 64, generator=g).to(dev)
    torch.manual_seed(seed)
    return x, rel, point, tensor_bnd, nn.Linear(128, 64).to(dev), nn.LayerNorm(64).to(dev)


def both_layers(a_ex, plan, n, ops, boundary):
    x, rel, point, tensor_bnd, lin, ln = ops
    if boundary == "point":     # LayerNorm, ReLU and residual with the point boundary; none of the three with the tensor
        kwargs = dict(layer_norm=ln, relu=True, residual=True, point=point)
    else:
        kwargs = dict(layer_norm=None, relu=False, residual=False, boundary=tensor_bnd)
    want = plan.fused_layer(rel, x, lin, **kwargs)
    got = rspmm.dense_layer_adjacency(a_ex, n, rel, x, lin, **kwargs)
    assert want is not None and torch.isfinite(got).all()
    return got, want


@pytest.mark.parametrize("boundary", ["dense", "point"])
@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_the_layer_on_an_adjacency_operand_equals_the_layer_on_a_fresh_plan(dev, n, bs, boundary):
    _, a_ex, plan, _ = case(n, dev)
    got, want = both_layers(a_ex, plan, n, layer_operands(dev, n, bs, seed=n + bs), boundary)
    assert torch.equal(got, want) and bits_equal(got, want)


@pytest.mark.parametrize("boundary", ["dense", "point"])
@pytest.mark.parametrize("bs", [1, 3])
def test_the_four_tile_form_on_an_adjacency_operand(dev, bs, boundary, monkeypatch):
    """n = 70 is five 16-row tiles: ULTRA_DOL_TILES=4 runs one full group of four and a ragged one, through either entry."""
    n = 70
    _, a_ex, plan, _ = case(n, dev)
    ops = layer_operands(dev, n, bs, seed=70 + bs)
    monkeypatch.setenv("ULTRA_DOL_TILES", "1")
    one, _ = both_layers(a_ex, plan, n, ops, boundary)
    monkeypatch.setenv("ULTRA_DOL_TILES", "4")
    got, want = both_layers(a_ex, plan, n, ops, boundary)
    assert torch.equal(got, want) and bits_equal(got, want) and bits_equal(got, one)


@pytest.mark.parametrize("values", ["ones", "random"])
@pytest.mark.parametrize("full", [True, False], ids=["ln_relu_residual", "plain"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_layer0_on_an_adjacency_operand_equals_layer0_on_a_fresh_plan(dev, n, full, values):
    """Sources: q = 0; q = n - 1 (the ragged column chunk) twice, two samples sharing one q; the isolated node, where only row q
    differs from the constant rows.  `plain` runs without LayerNorm, ReLU and residual and with -0 entries in the bias: the
    constant rows then hold the bias itself, signs included."""
    cells, a_ex, plan, iso = case(n, dev)
    src = torch.tensor([0, n - 1, iso, n - 1], device=dev)
    g = torch.Generator().manual_seed(7 * n + full)
    rel = (torch.randn(4, 4, 64, generator=g) * 0.5).to(dev)
    rel[3] = rel[1]       # (the two samples that share a source differ in nothing: their outputs must not either)
    vals = None if values == "ones" else torch.randn(4, 64, generator=g).to(dev)
    if vals is not None:
        vals[3] = vals[1]
    torch.manual_seed(n)
    lin, ln = nn.Linear(128, 64).to(dev), nn.LayerNorm(64).to(dev)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5), ln.bias.uniform_(-0.5, 0.5)
        if not full:
            lin.bias[::7] = -0.0
    kwargs = dict(layer_norm=ln if full else None, relu=full, residual=full)
    want = plan.layer0(rel, src, vals, lin, **kwargs)
    got = rspmm.dense_layer0_adjacency(a_ex, n, rel, src, vals, lin, **kwargs)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert torch.equal(got, want) and bits_equal(got, want)
    assert bits_equal(got[1], got[3])
    # the isolated source: every row but q holds the constant row, and q does not
    others = [i for i in range(n) if i != iso]
    assert bits_equal(got[2, others], got[2, others[:1]].expand(len(others), -1))
    assert not bits_equal(got[2, iso], got[2, others[0]])
    # a reached source: exactly the rows with a cell in column q (and q) can differ from the constant row
    reached = cells[:, :, 0].any(0)
    reached[0] = True
    constant = got[0, (~reached).nonzero()[0, 0]]
    assert bits_equal(got[0, ~reached.to(dev)], constant.expand(int((~reached).sum()), -1))
    if not full:
        assert bits_equal(constant, lin.bias.detach())


def test_the_wrappers_refuse_what_the_entry_points_do_not_serve(dev):
    _, a_ex, _, _ = case(17, dev)
    x, rel, point, _, lin, ln = layer_operands(dev, 17, 2, seed=3)
    with pytest.raises(RuntimeError, match="byte adjacency"):
        rspmm.dense_layer_adjacency(a_ex[:-1], 17, rel, x, lin, point=point)
    with pytest.raises(RuntimeError, match="byte adjacency"):
        rspmm.dense_layer0_adjacency(a_ex, 33, rel, point[0], None, lin)
    with pytest.raises(RuntimeError):       # (ULTRA_ERR_INVALID: too few relation rows)
        rspmm.dense_layer0_adjacency(a_ex, 17, rel[:, :3], point[0], None, lin)


# ---- the live object and the serving path ----
def load_model(dev, aggregate_func="sum"):
    net = models.Ultra(**synthetic.default_model_cfg(aggregate_func=aggregate_func))
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def model(dev):
    return load_model(dev)


def graph(slots, dev):
    """60 entities (the last two without edges), 200 triples = 400 edges over R = slots - K direct relations, every one in use."""
    data = synthetic.make_kg(N - 2, 200, slots - K, seed=100 + slots, relation_graph=False)
    data.num_nodes = N
    assert set(data.edge_type.tolist()) == set(range(2 * (slots - K))) and data.edge_index.shape[1] == 400
    return tasks.build_relation_graph(data.to(dev))


def same(got, want):
    return len(got) == len(want) and all(
        x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(got, want))


ANCHORS = [0, 7, 31, 57, 58]        # (58: an entity without edges)


def answers(p, anchors, relations):
    """(tails, heads, tails_above) of `p`, cloned: the steps' buffers are reused by the next call."""
    return [tuple(t.clone() for t in out) for out in (p.tails(anchors, relations), p.heads(anchors, relations),
                                                      p.tails_above(anchors, relations, 0.0))]


def fresh_answers(model, p, anchors, relations, verify=None):
    """The same calls on a fresh Predictor given p.materialized() -- and verify_tails of `verify` = (h, r, t) where asked."""
    fresh = predict.Predictor(model, p.materialized(), k=p.k, batch_size=p.batch_size)
    try:
        assert fresh.relation_capacity == 0 and not fresh.live_relation_graph
        out = answers(fresh, anchors, relations)
        if verify is not None:
            out.append(tuple(t.clone() for t in fresh.verify_tails(*verify)))
        return out
    finally:
        fresh.close()


def first_fact_through_a_new_relation(model, data, dev, slots, live=True):
    """Step 1: add_relations(1) and a first fact through it; the first answers record the captured steps."""
    p = predict.Predictor(model, data, k=5, batch_size=4, relation_capacity=K, live_relation_graph=live)
    assert p.data.num_relations == 2 * slots
    (a,) = p.add_relations(1).tolist()
    assert p.add_facts(0, a, 7) == 1
    anchors = torch.tensor(ANCHORS, device=dev)
    relations = torch.tensor([a, 0, 1, a, 2], device=dev)
    assert all(same(x, y) for x, y in zip(answers(p, anchors, relations), fresh_answers(model, p, anchors, relations)))
    return p, a, anchors, relations


def cells_of(rg):
    return rg.adjacency_bits.clone()


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_a_fact_that_changes_the_relation_graph_costs_no_plan_and_no_capture(dev, model, slots):
    data = graph(slots, dev)
    p, a, anchors, relations = first_fact_through_a_new_relation(model, data, dev, slots)
    rg, steps = p.delta.relation_graph, dict(p._steps)
    assert isinstance(rg, tasks.LiveRelationGraph) and rg.adjacency_bits is p.delta._resident[2]
    assert set(steps) == {"tail", "head"}
    address, version, before = rg.dense_adjacency.data_ptr(), rg.version, cells_of(rg)
    known = {id(plan): plan for plan in rspmm.cached_plans()}       # (held: an id is not handed out twice)
    with rspmm.record_plans() as used:
        # step 2: the new relation's first fact with entity 58 as its head -- new cells (58 has no edge: a's tail role at 7 meets
        # nothing new, its head role at 58 nothing at all, but 31 is the tail of other relations)
        assert p.add_facts([58, 31], [a, a], [31, 58]) == 3
        assert not torch.equal(cells_of(rg), before) and rg.version > version
        version, before = rg.version, cells_of(rg)
        # step 3: a repeated fact -- no new cell
        assert p.add_facts(0, a, 7) == 4
        assert torch.equal(cells_of(rg), before) and rg.version == version
        got = answers(p, anchors, relations)
    assert p.delta.relation_graph is rg and rg.dense_adjacency.data_ptr() == address
    assert set(p._steps) == set(steps) and all(p._steps[key] is steps[key] for key in steps)
    assert all(id(plan) in known for plan in used.plans), "a plan was built"
    assert {id(plan) for plan in rspmm.cached_plans()} <= set(known)
    facts = (torch.tensor([58, 0, 5], device=dev), torch.tensor([a, a, 0], device=dev), torch.tensor([31, 7, 9], device=dev))
    want = fresh_answers(model, p, anchors, relations, verify=facts)
    assert all(same(x, y) for x, y in zip(got, want[:3]))
    # (verify_* on a predictor with a reserve compacts first -- DESIGN.md 24's rule, untouched -- so it comes last)
    assert same(p.verify_tails(*facts), want[3])
    p.close()


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_the_byte_adjacency_equals_a_fresh_plans_after_additions(dev, slots):
    # (laid out over the slots as the Predictor does it: the last K direct relations have no edge)
    padded = live.with_relation_slots(graph(slots, dev), slots, slots - K)
    delta = rspmm.GraphDelta(padded, capacity=16, num_live_relations=slots, live_relation_graph=True)
    a = slots - K
    delta.add(0, a, 7)
    rg = delta.relation_graph
    assert isinstance(rg, tasks.LiveRelationGraph) and rg.num_nodes == 2 * slots
    for h, r, t in (([58, 31], [a, a], [31, 58]), (0, a, 7), ([3, 59], [a + 1, 0], [59, 4]), (12, a + 2, 13)):
        delta.add(h, r, t)
        assert delta.relation_graph is rg
        snap = rg.snapshot()
        want_bits = tasks.relation_graph_bits(delta.materialize())[0]
        assert torch.equal(rg.adjacency_bits, want_bits) and torch.equal(snap.adjacency_bits, want_bits)
        assert torch.equal(rg.edge_index, snap.edge_index) and torch.equal(rg.edge_type, snap.edge_type)
        plan = rspmm.Plan(snap.edge_index, snap.edge_type, snap.num_nodes, 4, exact_order=True, dense=True)
        assert torch.equal(rg.dense_adjacency.cpu(), plan.dense.export(_lib.ARR_DENSE_ORDER))


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_a_retraction_keeps_the_object_and_the_answers(dev, model, slots):
    data = graph(slots, dev)
    p, a, anchors, relations = first_fact_through_a_new_relation(model, data, dev, slots)
    assert p.add_facts([58, 31], [a, a], [31, 58]) == 3
    rg, address = p.delta.relation_graph, p.delta.relation_graph.dense_adjacency.data_ptr()
    before = cells_of(rg)
    # an added fact and a base fact leave: cells are CLEARED, which no OR can do
    h0, t0, r0 = int(data.edge_index[0, 0]), int(data.edge_index[1, 0]), int(data.edge_type[0])
    assert r0 < slots - K
    assert p.remove_facts([31, h0], [a, r0], [58, t0]).tolist()[0] == 1
    assert p.delta.relation_graph is rg and rg.dense_adjacency.data_ptr() == address and p.delta._resident is not None
    assert torch.equal(rg.adjacency_bits, tasks.relation_graph_bits(p.delta.materialize(p.data))[0])
    assert not torch.equal(cells_of(rg), before)
    assert all(same(x, y) for x, y in zip(answers(p, anchors, relations), fresh_answers(model, p, anchors, relations)))
    # ... and the next addition goes on in place
    assert p.add_facts(31, a, 58) == 3
    assert p.delta.relation_graph is rg
    assert all(same(x, y) for x, y in zip(answers(p, anchors, relations), fresh_answers(model, p, anchors, relations)))
    p.close()


def test_a_materialized_graph_is_not_written_by_a_later_addition(dev, model):
    slots = 17
    p, a, anchors, relations = first_fact_through_a_new_relation(model, graph(slots, dev), dev, slots)
    held = p.delta.materialize(p.data)
    rel = held.relation_graph
    assert not isinstance(rel, tasks.LiveRelationGraph)
    kept = (rel.edge_index.clone(), rel.edge_type.clone(), rel.adjacency_bits.clone(), held.edge_index.clone())
    assert p.add_facts([58, 31], [a, a], [31, 58]) == 3
    assert not torch.equal(p.delta.relation_graph.adjacency_bits, kept[2])
    assert held.relation_graph is rel and torch.equal(rel.edge_index, kept[0]) and torch.equal(rel.edge_type, kept[1])
    assert torch.equal(rel.adjacency_bits, kept[2]) and torch.equal(held.edge_index, kept[3])
    assert p.delta.materialize(p.data).relation_graph is not rel
    p.close()


def test_a_relation_table_does_not_outlive_an_in_place_change(dev, slots=16):
    model = load_model(dev)     # (its own: the table is held by the model)
    p, a, anchors, relations = first_fact_through_a_new_relation(model, graph(slots, dev), dev, slots)
    served = p.delta.live_view(p.data)       # (the graph the model is handed: the live relation graph in place of the base's)
    assert served.relation_graph is p.delta.relation_graph
    model.cache_relation_representations(served, chunk=4)
    p.close()       # (the steps are recorded again, gathering from the table)
    got = answers(p, anchors, relations)
    assert model._rel_table is not None
    # (a fresh predictor hands the model another relation graph: the table is dropped there, and filled again below)
    assert all(same(x, y) for x, y in zip(got, fresh_answers(model, p, anchors, relations)))
    model.cache_relation_representations(served, chunk=4)
    p.close()
    answers(p, anchors, relations)
    assert model._rel_table is not None
    assert p.add_facts([58, 31], [a, a], [31, 58]) == 3       # new cells, in place: the table is stale, under the same object
    assert p.delta.relation_graph is served.relation_graph
    got = answers(p, anchors, relations)
    assert all(same(x, y) for x, y in zip(got, fresh_answers(model, p, anchors, relations)))
    p.close()


def test_with_the_flag_off_the_object_changes_as_before(dev, model, slots=16):
    p, a, anchors, relations = first_fact_through_a_new_relation(model, graph(slots, dev), dev, slots, live=False)
    rg, steps = p.delta.relation_graph, dict(p._steps)
    assert not isinstance(rg, tasks.LiveRelationGraph)
    assert p.add_facts([58, 31], [a, a], [31, 58]) == 3
    assert p.delta.relation_graph is not rg and not isinstance(p.delta.relation_graph, tasks.LiveRelationGraph)
    p.tails(anchors, relations)
    assert p._steps["tail"] is not steps["tail"]
    p.close()


def test_a_max_aggregate_relation_model_is_refused(dev):
    net = load_model(dev, "max")
    with pytest.raises(ValueError, match=r"relation_model\.layers\.0 \(max aggregate"):
        predict.Predictor(net, graph(16, dev), relation_capacity=K, live_relation_graph=True)
