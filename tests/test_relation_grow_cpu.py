"""Serving a growing vocabulary, the parts that need no GPU: reserved relation slots, the served numbering,
Predictor.add_relations, the live bound of the relation checks, materialized() in the compact numbering, compaction beyond the
reserve.

The graph: 40 entities, R = 6 direct relations, K = 3 reserved slots.  The model is the golden ultra_3g weights under `rotate`
messages -- the configuration that runs on CPU tensors.  Everything compared here is ids and graph fields, exactly; the scores'
bit-equality with a fresh predictor is asserted on the GPU (test_relation_grow_gpu.py)."""
import os

import pytest
import torch

from ultra_amd import models, predict, synthetic, tasks
from ultra_amd.data import Data
from ultra_amd.live import LiveGraph, compact_relations, with_relation_slots

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N, R, K = 40, 6, 3


@pytest.fixture(scope="module")
def model():
    m = models.Ultra(**synthetic.default_model_cfg(message_func="rotate"))
    m.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    return m.eval()


@pytest.fixture()
def data():
    g = synthetic.make_kg(N, 120, R, seed=7)
    assert g.num_nodes == N and g.num_relations == 2 * R and set(g.edge_type.tolist()) == set(range(2 * R))
    return g


def same_relation_graph(got, want):
    return (got.num_nodes == want.num_nodes and torch.equal(got.edge_index, want.edge_index)
            and torch.equal(got.edge_type, want.edge_type))


def test_constructor_argument_checks(model, data):
    for bad in (-1, 1.5, True, "3", None):
        with pytest.raises(ValueError):
            predict.Predictor(model, data, relation_capacity=bad)
        with pytest.raises(ValueError):
            LiveGraph(data, relation_capacity=bad)
    assert predict.Predictor(model, data, relation_capacity=0).data is data
    with pytest.raises(ValueError):
        with_relation_slots(data, R - 1, R)


def test_the_served_numbering(model, data):
    p = predict.Predictor(model, data, relation_capacity=K)
    served = p.data
    assert served is not data and served.num_relations == 2 * (R + K) == 18
    assert p.relation_capacity == K and p.num_direct_relations == R and p.num_relation_slots == R + K
    inverse = data.edge_type >= R
    assert torch.equal(served.edge_type[~inverse], data.edge_type[~inverse])
    assert torch.equal(served.edge_type[inverse], data.edge_type[inverse] - R + 9)      # r + 9
    assert torch.equal(served.edge_index, data.edge_index)      # (the edge order is untouched)
    assert data.num_relations == 2 * R and int(data.edge_type.max()) == 2 * R - 1       # (the caller's graph is left alone)
    rel = served.relation_graph
    assert rel.num_nodes == 18
    touched = torch.unique(rel.edge_index)
    isolated = sorted(set(range(18)) - set(touched.tolist()))
    assert isolated == [6, 7, 8, 15, 16, 17]
    # the live nodes' cells are the unpadded graph's, under the monotone map of the ids
    to_slot = torch.tensor([r if r < R else r + K for r in range(2 * R)])
    assert torch.equal(rel.edge_index, to_slot[data.relation_graph.edge_index])
    assert torch.equal(rel.edge_type, data.relation_graph.edge_type)
    # and the helper has an inverse
    back = compact_relations(served, R + K, R)
    assert back.num_relations == 2 * R and torch.equal(back.edge_type, data.edge_type)
    assert same_relation_graph(back.relation_graph, data.relation_graph)


def test_add_relations_hands_out_ids_and_the_reserve_is_no_relation(model, data):
    p = predict.Predictor(model, data, k=5, batch_size=4, relation_capacity=K)
    plan_graph, rel_graph = p.data, p.delta.relation_graph
    with pytest.raises(ValueError):
        p.add_facts(1, 6, 2)        # (a reserved slot is no relation yet)
    with pytest.raises(ValueError):
        p.tails([1], [6])
    assert p.add_relations(2).tolist() == [6, 7]
    assert p.num_direct_relations == 8 and p.delta.num_live_relations == 8 and p.num_relation_slots == 9
    assert p.data is plan_graph and p.delta.relation_graph is rel_graph      # (no plan, no relation graph)
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError):
            p.add_relations(bad)
    with pytest.raises(ValueError, match=r"= 8\)"):      # (the live count, never the slot count)
        p.add_facts(1, 8, 2)
    for query in (p.tails, p.heads):
        with pytest.raises(ValueError, match=r"\[0, 8\)"):
            query([1], [8])
    for query in (p.tails_above, p.heads_above):
        with pytest.raises(ValueError):
            query([1], [8], 0.0)
    for verify in (p.verify_tails, p.verify_heads):
        with pytest.raises(ValueError):
            verify([1], [8], [2])
    with pytest.raises(ValueError):
        p.remove_facts(1, 8, 2)
    assert p.add_facts(1, 7, 2) == 1
    ids, scores, count = p.tails([1, 3], [7, 0])
    assert ids.shape == (2, 5) and bool((ids < N).all())


@pytest.mark.parametrize("entity_capacity", [0, 2])
def test_materialized_equals_the_graph_built_by_hand(model, data, entity_capacity):
    p = predict.Predictor(model, data, relation_capacity=K, entity_capacity=entity_capacity)
    a, b = p.add_relations(2).tolist()
    assert (a, b) == (6, 7)
    tail = p.add_entities(1).tolist()[0] if entity_capacity else 11
    assert tail == (N if entity_capacity else 11)
    h = torch.tensor([3, 5, 9, 20, 0])
    r = torch.tensor([a, 2, b, 0, 5])
    t = torch.tensor([4, 6, tail, 21, 39])
    assert p.add_facts(h, r, t) == 5
    got = p.materialized()
    live = R + 2
    nodes = N + (1 if entity_capacity else 0)
    base_type = torch.where(data.edge_type >= R, data.edge_type - R + live, data.edge_type)
    want = Data(edge_index=torch.cat([data.edge_index, torch.stack([torch.cat([h, t]), torch.cat([t, h])])], dim=1),
                edge_type=torch.cat([base_type, r, r + live]), num_nodes=nodes, num_relations=2 * live)
    tasks.build_relation_graph(want)
    assert got.num_relations == 16 and got.num_nodes == nodes
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(got.edge_type, want.edge_type)
    assert same_relation_graph(got.relation_graph, want.relation_graph)
    # what is served keeps the slot numbering, and the caller's graph is untouched
    assert p.data.num_relations == 18 and p.num_direct_relations == 8
    assert data.num_relations == 2 * R
    # a fresh predictor takes the materialised graph as it is
    fresh = predict.Predictor(model, got, k=5, batch_size=4)
    assert fresh.data is got and fresh.num_direct_relations == 8


def test_the_filter_graph_is_renumbered_alike(model, data):
    filt = synthetic.make_kg(N, 160, R, seed=8, relation_graph=False)
    p = predict.Predictor(model, data, filtered_data=filt, relation_capacity=K)
    assert p.filter_graph.num_relations == 18
    assert torch.equal(p.filter_graph.edge_type, torch.where(filt.edge_type >= R, filt.edge_type + K, filt.edge_type))
    (a,) = p.add_relations().tolist()
    p.add_facts(1, a, 2)
    out = p.materialized().filtered_data
    assert out.num_relations == 14
    assert torch.equal(out.edge_type[:-2], torch.where(filt.edge_type >= R, filt.edge_type + 1, filt.edge_type))
    assert out.edge_type[-2:].tolist() == [a, a + 7] and out.edge_index[:, -2:].tolist() == [[1, 2], [2, 1]]


def test_add_relations_beyond_the_reserve_compacts_and_keeps_facts_and_ids(model, data):
    p = predict.Predictor(model, data, k=5, batch_size=4, relation_capacity=K)
    assert p.add_relations(3).tolist() == [6, 7, 8]
    p.add_facts([3, 5], [6, 8], [4, 6])
    before = p.materialized()
    served = p.data
    assert p.add_relations(2).tolist() == [9, 10]      # 11 > 9 slots: one compaction, 9 + 2 + 3 slots
    assert p.data is not served and p.num_relation_slots == 14 and p.num_direct_relations == 11
    assert p.data.num_relations == 28 and len(p.delta) == 0
    assert p.data.edge_index.shape[1] == data.edge_index.shape[1] + 4       # (the facts were folded in)
    # the same edges under the same direct ids; the inverse ids follow the slot count
    after = p.materialized()
    assert after.num_relations == 22 and torch.equal(after.edge_index, before.edge_index)
    direct = before.edge_type < 9
    assert torch.equal(after.edge_type[direct], before.edge_type[direct])
    assert torch.equal(after.edge_type[~direct], before.edge_type[~direct] + 2)
    assert int(p.data.edge_type[p.data.edge_type >= 11].min()) >= 14
    assert p.add_facts(1, 10, 2) == 1 and p.add_relations().tolist() == [11]
    assert p.num_relation_slots == 14      # (within the new reserve: nothing rebuilt)
    ids, _, _ = p.tails([3], [6])
    assert ids.shape == (1, 5)


def test_without_a_reserve_everything_is_as_it_was(model, data):
    p = predict.Predictor(model, data, k=5, batch_size=4)
    assert p.relation_capacity == 0 and p.data is data and p.num_direct_relations == R == p.num_relation_slots
    with pytest.raises(ValueError, match="relation_capacity > 0"):
        p.add_relations()
    with pytest.raises(ValueError):
        p.add_facts(1, R, 2)
    assert p.add_facts(1, 2, 3) == 1
    got = p.materialized()
    assert got.num_relations == 2 * R and got.edge_type[-2:].tolist() == [2, 2 + R]
    assert torch.equal(got.edge_type[:-2], data.edge_type)
    live = LiveGraph(data)
    with pytest.raises(ValueError):
        live.add_relations()
