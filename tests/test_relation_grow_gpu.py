"""Serving a growing vocabulary on the GPU: Predictor(relation_capacity) against a fresh Predictor on the
materialised graph -- bit for bit, on reference-order plans (the default) -- the relation graph kept current from the delta's
edges (GraphDelta._add_to_relation_graph) against tasks.relation_graph_bits of the materialised list, and
ultra_relation_graph_add_edges through the C ABI against ultra_relation_graph_bits of the concatenated list.

Every case runs at 2 R' = 30 (one bit word), 32 (exactly one word) and 34 relation-graph nodes (two words; R' = 17 is no
multiple of 16, so the byte adjacency of the relation-graph layer has a ragged tile): the sizes at which a kernel here can go
wrong that a small shape can show.  Graphs: 60 entities, 400 edges; K = 3 reserved slots."""
import os

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N, K = 60, 3
SLOT_COUNTS = (15, 16, 17)      # R': 2 R' = 30, 32, 34


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def equals_fresh(model, p, anchors, relations):
    """tails, heads, tails_above, heads_above of `p` against a fresh Predictor on p.materialized(): ids, scores, counts, sizes."""
    fresh = predict.Predictor(model, p.materialized(), k=p.k, batch_size=p.batch_size)
    try:
        assert fresh.relation_capacity == 0 and fresh.data.num_relations == 2 * p.num_direct_relations
        assert same(p.tails(anchors, relations), fresh.tails(anchors, relations))
        assert same(p.heads(anchors, relations), fresh.heads(anchors, relations))
        assert same(p.tails_above(anchors, relations, 0.0), fresh.tails_above(anchors, relations, 0.0))
        assert same(p.heads_above(anchors, relations, 0.0), fresh.heads_above(anchors, relations, 0.0))
    finally:
        fresh.close()
    return True


def bits_are_current(p):
    """The delta's relation graph against today's route on the materialised list in slot numbering: the bit matrices word for
    word, the edge list element for element."""
    want = tasks.build_relation_graph(Data(**{k: getattr(p.delta.materialize(p.data), k)
                                              for k in ("edge_index", "edge_type", "num_nodes", "num_relations")})).relation_graph
    got = p.delta.relation_graph
    assert want.adjacency_bits.shape == (4, 2 * p.num_relation_slots, (2 * p.num_relation_slots + 31) // 32)
    assert torch.equal(got.adjacency_bits, want.adjacency_bits)
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(got.edge_type, want.edge_type)
    return True


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_a_reserve_equals_a_fresh_predictor_at_every_stage(dev, model, slots):
    data = graph(slots, dev)
    direct = slots - K
    p = predict.Predictor(model, data, k=5, batch_size=4, relation_capacity=K)
    assert p.data.num_relations == 2 * slots
    anchors = torch.tensor([0, 7, 31, 57, 58], device=dev)        # (58: an entity without edges)
    old = torch.tensor([0, 1, direct - 1, 2, 3], device=dev)
    assert equals_fresh(model, p, anchors, old)                     # before any edit
    a, b = p.add_relations(2).tolist()
    assert (a, b) == (direct, direct + 1)
    assert equals_fresh(model, p, anchors, old)                     # two relations without a fact
    assert p.delta._resident is None
    first = p.delta.relation_graph
    assert p.add_facts([0, 7, 31, 58], [a, a, b, b], [7, 12, 58, 59]) == 4
    assert p.delta.relation_graph is not first and p.delta._resident is not None
    assert bits_are_current(p)
    new = torch.tensor([a, a, b, b, a], device=dev)
    assert equals_fresh(model, p, anchors, new)                     # the new relations themselves ...
    assert equals_fresh(model, p, anchors, old)                     # ... and established ones
    # a fact that changes no adjacency cell: the relation-graph object, its plan and the captured steps stay
    steps, rel, bits = dict(p._steps), p.delta.relation_graph, p.delta.relation_graph.adjacency_bits.clone()
    assert set(steps) == {"tail", "head"}
    assert p.add_facts(0, a, 7) == 5
    assert p.delta.relation_graph is rel and torch.equal(rel.adjacency_bits, bits)
    assert bits_are_current(p)
    assert equals_fresh(model, p, anchors, new)
    assert set(p._steps) == set(steps) and all(p._steps[key] is steps[key] for key in steps)
    # the object an older capture holds is not written to when a later fact changes the graph
    assert p.add_facts(59, 0, 58) == 6
    assert p.delta.relation_graph is not rel and torch.equal(rel.adjacency_bits, bits)
    assert rel.adjacency_bits.data_ptr() != p.delta._resident[2].data_ptr()
    assert bits_are_current(p)
    # a retraction rebuilds from the edge list; the next addition seeds the resident state again
    assert p.remove_facts(31, b, 58).tolist() == [1]
    assert p.delta._resident is None and bits_are_current(p)
    assert p.add_facts(12, b, 31) == 6
    assert p.delta._resident is not None and bits_are_current(p)
    assert equals_fresh(model, p, anchors, new)
    # the forced full rebuild (the private switch) gives the same graph
    p.delta._full_rebuild = True
    assert p.add_facts(13, b, 58) == 7
    assert p.delta._resident is None and bits_are_current(p)
    p.close()


@pytest.mark.parametrize("aggregate_func", ["sum", "max"])
@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_an_unused_reserve_leaves_the_scores_alone(dev, slots, aggregate_func):
    """Reserved columns leave the relation model's bits alone: the same graph with and without a reserve, no edit."""
    net = load_model(dev, aggregate_func)
    data = graph(slots, dev)
    anchors = torch.tensor([0, 7, 31, 57, 58], device=dev)
    relations = torch.tensor([0, 1, slots - K - 1, 2, 3], device=dev)
    plain = predict.Predictor(net, data, k=5, batch_size=4)
    padded = predict.Predictor(net, data, k=5, batch_size=4, relation_capacity=K)
    assert plain.data is data and padded.data.num_relations == 2 * slots
    assert same(padded.tails(anchors, relations), plain.tails(anchors, relations))
    assert same(padded.heads(anchors, relations), plain.heads(anchors, relations))
    assert same(padded.tails_above(anchors, relations, 0.0), plain.tails_above(anchors, relations, 0.0))
    assert same(padded.heads_above(anchors, relations, 0.0), plain.heads_above(anchors, relations, 0.0))
    plain.close(), padded.close()


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_explanations_name_relations_in_the_compact_numbering(dev, model, slots):
    data = graph(slots, dev)
    p = predict.Predictor(model, data, k=3, batch_size=4, relation_capacity=K)
    (a,) = p.add_relations().tolist()
    p.add_facts([0, 7], [a, a], [7, 12])
    fresh = predict.Predictor(model, p.materialized(), k=3, batch_size=4)
    anchors, relations = torch.tensor([0, 31], device=dev), torch.tensor([a, 1], device=dev)
    live = p.num_direct_relations
    for got, want in ((p.explain_tails(anchors, relations), fresh.explain_tails(anchors, relations)),
                      (p.explain_heads(anchors, relations), fresh.explain_heads(anchors, relations))):
        assert same(got[:3], want[:3])
        assert p.num_relation_slots == slots and p.num_direct_relations == live == slots - K + 1      # (the slot counts stay)
        seen = 0
        for per_query, per_query_want in zip(got[3], want[3]):
            assert len(per_query) == len(per_query_want)
            for (paths, weights), (paths_want, weights_want) in zip(per_query, per_query_want):
                assert [list(path) for path in paths] == [list(path) for path in paths_want]
                assert len(weights) == len(weights_want)
                assert all(0 <= r < 2 * live for path in paths for _, _, r in path)
                seen += sum(len(path) for path in paths)
        assert seen > 0
    p.close(), fresh.close()


@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_both_reserves_together(dev, model, slots):
    data = graph(slots, dev)
    p = predict.Predictor(model, data, k=5, batch_size=4, relation_capacity=K, entity_capacity=2)
    (e,) = p.add_entities().tolist()
    (a,) = p.add_relations().tolist()
    assert (e, a) == (N, slots - K)
    assert p.add_facts([e, 7], [a, 0], [5, e]) == 2
    assert bits_are_current(p)
    got = p.materialized()
    assert got.num_nodes == N + 1 and got.num_relations == 2 * (slots - K + 1)
    anchors = torch.tensor([e, 5, 0, 58], device=dev)
    assert equals_fresh(model, p, anchors, torch.tensor([a, a, 0, 1], device=dev))
    p.close()


def test_a_relation_graph_that_is_not_the_lists_own_is_replaced_at_the_first_addition(dev):
    """The rebuild from the edge list replaces whatever relation graph the served graph was handed; so does the seed."""
    data = graph(16, dev)
    part = Data(edge_index=data.edge_index[:, :100], edge_type=data.edge_type[:100], num_nodes=N, num_relations=data.num_relations)
    data.relation_graph = tasks.build_relation_graph(part).relation_graph
    for full in (False, True):
        delta = rspmm.GraphDelta(data, capacity=4)
        delta._full_rebuild = full
        assert delta.relation_graph is data.relation_graph
        delta.add(int(data.edge_index[0, 0]), int(data.edge_type[0]), int(data.edge_index[1, 0]))      # (an edge the list holds)
        want = tasks.relation_graph_bits(delta.materialize(data))[0]
        assert delta.relation_graph is not data.relation_graph and (delta._resident is None) == full
        assert torch.equal(delta.relation_graph.adjacency_bits, want)


# ---- ultra_relation_graph_add_edges through the C ABI ----
def abi_base(rels, dev):
    """A sparse list: 40 triples among the entities below 50 over the direct relations below rels / 2 - 2, inverses included;
    the entities from 50 on have no edge and the last two direct relations (and their inverses) none either."""
    g = torch.Generator().manual_seed(rels)
    half = rels // 2
    h, t, r = (torch.randint(0, 50, (40,), generator=g), torch.randint(0, 50, (40,), generator=g),
               torch.randint(0, half - 2, (40,), generator=g))
    return Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]).to(dev), edge_type=torch.cat([r, r + half]).to(dev),
                num_nodes=N, num_relations=rels)


def fact_edges(facts, half, dev):
    h, r, t = (torch.tensor(v, dtype=torch.long) for v in zip(*facts))
    return torch.stack([torch.cat([h, t]), torch.cat([t, h])]).to(dev), torch.cat([r, r + half]).to(dev)


def abi_cases(base, dev):
    """name -> (edge_index, edge_type, changed)."""
    half = base.num_relations // 2
    first = (int(base.edge_index[0, 0]), int(base.edge_type[0]), int(base.edge_index[1, 0]))
    one = fact_edges([(3, half - 1, 4)], half, dev)
    return {
        "repeated_endpoint": fact_edges([(3, half - 2, 4), (3, half - 2, 5), (3, 0, 4), (3, half - 2, 4)], half, dev) + (1,),
        "empty_endpoint": fact_edges([(55, 0, 56), (55, half - 2, 57)], half, dev) + (1,),
        "first_role": fact_edges([(3, half - 1, 4)], half, dev) + (1,),
        "one_edge": (one[0][:, :1].contiguous(), one[1][:1].contiguous(), 1),
        "zero_edges": (torch.zeros(2, 0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev), 0),
        "an_edge_the_list_holds": fact_edges([first], half, dev) + (0,),
    }


def add_edges(edge_index, edge_type, num_nodes, state, changed):
    adj, counts, hbits, tbits = state
    rc = _lib.lib.ultra_relation_graph_add_edges(edge_index.data_ptr(), edge_type.data_ptr(), edge_index.shape[1], num_nodes,
                                                 adj.shape[1], hbits.data_ptr(), tbits.data_ptr(), adj.data_ptr(),
                                                 counts.data_ptr(), changed.data_ptr(), _lib.stream_of(adj.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", ["repeated_endpoint", "empty_endpoint", "first_role", "one_edge", "zero_edges",
                                  "an_edge_the_list_holds"])
@pytest.mark.parametrize("rels", [30, 32, 34])
def test_add_edges_equals_the_bits_of_the_concatenated_list(dev, rels, case):
    base = abi_base(rels, dev)
    edge_index, edge_type, want_changed = abi_cases(base, dev)[case]
    state = tasks.relation_graph_bits(base, incidence=True)
    before = state[0].clone()
    both = Data(edge_index=torch.cat([base.edge_index, edge_index], dim=1), edge_type=torch.cat([base.edge_type, edge_type]),
                num_nodes=N, num_relations=rels)
    want = tasks.relation_graph_bits(both, incidence=True)
    changed = torch.full((1,), 77, dtype=torch.int32, device=dev)      # (written whole by the call)
    assert add_edges(edge_index, edge_type, N, state, changed) == _lib.ULTRA_OK
    for got, expected in zip(state, want):
        assert torch.equal(got, expected)
    assert int(changed) == want_changed == int(not torch.equal(before, want[0]))
    # and once more: every OR is idempotent, nothing changes
    assert add_edges(edge_index, edge_type, N, state, changed) == _lib.ULTRA_OK
    assert int(changed) == 0 and all(torch.equal(got, expected) for got, expected in zip(state, want))


@pytest.mark.parametrize("rels", [30, 32, 34])
def test_add_edges_never_dereferences_an_index_outside_the_graph(dev, rels):
    """The index values live on the device and the call does not wait for it: an index out of range comes back in `changed`
    (RELGRAPH_OUT_OF_RANGE) with the bit sets untouched -- a good edge in the same call is not marked either -- and the wrapper's
    caller raises.  What the host can see is ULTRA_ERR_INVALID with nothing launched."""
    base = abi_base(rels, dev)
    half = rels // 2
    state = tasks.relation_graph_bits(base, incidence=True)
    before = [s.clone() for s in state]
    good = (3, half - 1, 4)
    for bad in ((N, 0, 4), (3, 0, N), (-1, 0, 4), (3, 0, -1), (3, rels, 4), (3, -1 - half, 4), (1 << 40, 0, 4)):
        edge_index, edge_type = fact_edges([good, bad], half, dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        assert add_edges(edge_index, edge_type, N, state, changed) == _lib.ULTRA_OK
        assert int(changed) == _lib.RELGRAPH_OUT_OF_RANGE
        assert all(torch.equal(got, kept) for got, kept in zip(state, before)), bad
    edge_index, edge_type = fact_edges([good], half, dev)
    changed = torch.full((1,), 77, dtype=torch.int32, device=dev)
    adj, counts, hbits, tbits = state
    stream = _lib.stream_of(dev)
    ptrs = [edge_index.data_ptr(), edge_type.data_ptr(), 2, N, rels, hbits.data_ptr(), tbits.data_ptr(), adj.data_ptr(),
            counts.data_ptr(), changed.data_ptr()]
    for at, value in ((0, None), (1, None), (2, -1), (3, 0), (4, 0), (4, (1 << 20) + 1), (5, None), (6, None), (7, None), (8, None),
                      (9, None)):
        args = list(ptrs)
        args[at] = value
        assert _lib.lib.ultra_relation_graph_add_edges(*args, stream) == _lib.ULTRA_ERR_INVALID, at
    torch.cuda.synchronize()
    assert int(changed) == 77 and all(torch.equal(got, kept) for got, kept in zip(state, before))
