"""The edit state of a served graph is held once (ultra_amd/live.py; DESIGN.md, "The live graph's state in one place"): one scripted
sequence of edits through a bare LiveGraph, through a CPU Predictor (the filter graph the served graph by default, the graph
handed in as `filtered_data`, and a separate filter graph) and through a CPU QueryPredictor on stub projections.  After every
step the owners agree with each other and with GraphDelta.materialize on the materialised edge list, the counts and the values
the calls return; a compaction happens at the same steps for all of them; and the rules that differ between the two predictors
hold.  No forward is run: everything here is host state."""
import pytest
import torch

from tests.test_query_live_cpu import N, edge_list_model, twelve_node_graph
from ultra_amd import models, predict, query_predict, rspmm, synthetic
from ultra_amd.data import Data
from ultra_amd.live import LiveGraph

CAPACITY, RESERVE = 3, 2
ROOM = 16       # (rows of the one big delta the owners are compared with: more than the sequence ever lays out)

# (call, arguments): with delta_capacity = 3 (six edges or keys) and entity_capacity = 2 the rule "2 * facts + keys <= 2 * capacity"
# gives the comments' outcomes.  The base graph states (0, 0, 1) three times and (5, 1, 6) once.
STEPS = [
    ("add_facts", ([8, 4], [1, 0], [3, 2])),                # 4 of 6 held
    ("remove_facts", ([5, 8], [1, 1], [6, 3])),             # a stated base fact and a just-added one: 4 + 4 > 6, compacts first
    ("add_entities", (1,)),                                 # id 12, inside the reserve
    ("add_facts", ([N], [0], [1])),                         # a fact on it: 4 keys + 2 = 6 fits
    ("add_entities", (2,)),                                 # 13 + 2 > 14 slots: beyond the reserve, one rebuild
    ("add_facts", ([13, 2, 9], [1, 1, 0], [0, 14, 9])),     # three facts: all of the capacity the rebuild emptied
    ("remove_facts", ([0, 2, 4, N], [0, 1, 1, 0], [1, 14, 8, 1])),      # four at once: more than the whole capacity, folded
    ("add_facts", ([1, 3, 6, 7], [0, 1, 0, 1], [2, 5, 6, 13])),         # four at once: more than the capacity, folded with a compaction
]
COMPACTS = [False, True, False, False, True, False, True, True]       # (what the rule gives; every owner must show it)


def separate_filter(data):
    return Data(edge_index=data.edge_index.clone(), edge_type=data.edge_type.clone(), num_nodes=N, num_relations=data.num_relations)


def owners(data, entity_capacity=RESERVE):
    model = models.Ultra(**synthetic.default_model_cfg()).eval()        # (its forward takes `delta`: the delta exists from the start)
    kwargs = dict(delta_capacity=CAPACITY, entity_capacity=entity_capacity)
    return {
        "live": LiveGraph(data, **kwargs),
        "predictor": predict.Predictor(model, data, k=3, **kwargs),
        "predictor_filter_is_graph": predict.Predictor(model, data, k=3, filtered_data=data, **kwargs),
        "predictor_separate_filter": predict.Predictor(model, data, k=3, filtered_data=separate_filter(data), **kwargs),
        "query": query_predict.QueryPredictor(edge_list_model(), data, k=3, **kwargs),
    }


def served(owner):
    return owner.data if isinstance(owner, predict.Predictor) else owner.graph


def state(owner):
    mat, delta = owner.materialized(), owner.delta
    return dict(edge_index=mat.edge_index, edge_type=mat.edge_type, num_nodes=int(mat.num_nodes), num_entities=owner.num_entities,
                num_slots=owner.num_slots, facts=0 if delta is None else len(delta), removed=0 if delta is None else delta.num_removed)


def same_state(a, b):
    return all(torch.equal(a[key], b[key]) if torch.is_tensor(a[key]) else a[key] == b[key] for key in a)


def edge_codes(graph):
    code = (graph.edge_index[0] * ROOM + graph.edge_index[1]) * int(graph.num_relations) + graph.edge_type
    return code.sort().values


def known_tails(owner, h, r):
    ptr, index = predict.known_answers(owner.filter_graph, torch.tensor([h]), torch.tensor([r]), "tail")
    return index.tolist()


def test_every_owner_keeps_the_same_state_through_one_sequence():
    data = twelve_node_graph()
    held = owners(data)
    predictors = [o for o in held.values() if isinstance(o, predict.Predictor)]
    qp = held["query"]
    # the whole sequence in one delta large enough never to fold, on the same edge list with room for every entity
    roomy = Data(edge_index=data.edge_index, edge_type=data.edge_type, num_nodes=ROOM, num_relations=data.num_relations)
    whole = rspmm.GraphDelta(roomy, capacity=64, num_live=N)
    assert qp.delta is None and held["live"].delta is None                      # made at the first edit ...
    assert all(p.delta is not None and not p.delta.edited for p in predictors)  # ... or held from the start
    counts = {name: owner.live_count for name, owner in held.items()}
    assert all(c is not None and int(c) == N for c in counts.values())
    for step, ((call, args), compacts) in enumerate(zip(STEPS, COMPACTS)):
        before = {name: served(owner) for name, owner in held.items()}
        got = {name: getattr(owner, call)(*args) for name, owner in held.items()}
        if call == "add_entities":
            whole.num_live += args[0]
            want = torch.arange(whole.num_live - args[0], whole.num_live)
        else:
            want = getattr(whole, "add" if call == "add_facts" else "remove")(*args)
        for name, owner in held.items():
            where = "step %d (%s), %s" % (step, call, name)
            # what the call returns: the ids, the retractions' counts; add_facts returns the facts its own delta holds (below)
            if call == "add_facts":
                assert got[name] == (0 if owner.delta is None else len(owner.delta)) == got["live"], where
            else:
                assert torch.equal(got[name], want), where
            # a compaction shows as a new served graph: at the same steps for every owner
            assert (served(owner) is not before[name]) == compacts, where
            now = state(owner)
            assert same_state(now, state(held["live"])), where
            # ... and GraphDelta.materialize: the owner's own delta on its served graph, and the one big delta as a multiset
            delta = owner.delta if owner.delta is not None else rspmm.GraphDelta(served(owner), 1, num_live=owner.num_entities)
            mat = delta.materialize(served(owner), num_nodes=owner.num_entities)
            assert torch.equal(now["edge_index"], mat.edge_index) and torch.equal(now["edge_type"], mat.edge_type), where
            assert now["num_nodes"] == owner.num_entities == whole.num_live == int(owner.live_count), where
            assert torch.equal(edge_codes(owner.materialized()), edge_codes(whole.materialize(num_nodes=whole.num_live))), where
            assert owner.live_count is counts[name], where        # one tensor for the owner's life, also beyond the reserve
        # the rules of one owner only
        if compacts and step != 1:
            assert qp.delta is None, step                 # None again after a compaction (at step 1 the retractions then made a new one)
        assert all(p.delta is not None for p in predictors), step
        if step == 0:
            assert all(known_tails(p, 8, 1) == [3] and 2 in known_tails(p, 4, 0) for p in predictors)      # a stated tail joins
        if step == 1:
            assert all(known_tails(p, 8, 1) == [] and 6 not in known_tails(p, 5, 1) for p in predictors)   # a retracted one leaves
            assert all(2 in known_tails(p, 4, 0) for p in predictors)
            assert qp.delta is not None and qp.delta.num_removed == 4
    assert [held["live"].num_entities, held["live"].num_slots] == [N + 3, N + 3 + RESERVE]
    sep = held["predictor_separate_filter"]
    assert sep.filter_graph is not sep.data and sep.materialized().filtered_data.num_nodes == N + 3
    assert known_tails(sep, 6, 0) == [6] and 1 not in known_tails(sep, 0, 0)       # the last call's fact joined, (0, 0, 1) is gone


def test_without_a_reserve_a_query_predictor_hands_out_the_served_graph_itself():
    data = twelve_node_graph()
    held = owners(data, entity_capacity=0)
    qp = held["query"]
    assert qp.delta is None and qp.materialized() is data and qp.graph is data and qp.live_count is None
    assert all(owner.materialized() is not served(owner) for name, owner in held.items() if name != "query")   # a new copy
    for owner in held.values():
        assert owner.add_facts(8, 1, 3) == 1 and owner.remove_facts(8, 1, 3).tolist() == [1]
        with pytest.raises(ValueError, match="this %s reserves no rows" % type(owner).__name__):
            owner.add_entities()
    assert qp.delta is not None and not qp.delta.edited and qp.materialized() is data       # nothing is edited
    assert all(owner.remove_facts(5, 1, 6).tolist() == [1] for owner in held.values())
    mat = qp.materialized()
    assert mat is not data and mat is qp.delta.materialize(data) and same_state(state(qp), state(held["live"]))
    qp.compact()
    assert qp.delta is None and qp.graph is not data and qp.materialized() is qp.graph


def test_the_capacities_are_validated_with_the_state():
    data = twelve_node_graph()
    model = models.Ultra(**synthetic.default_model_cfg())
    makers = (lambda **kw: LiveGraph(data, **kw), lambda **kw: predict.Predictor(model, data, **kw),
              lambda **kw: query_predict.QueryPredictor(edge_list_model(), data, **kw))
    for make in makers:
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="delta_capacity must be a positive int"):
                make(delta_capacity=bad)
        for bad in (-1, 1.0, True):
            with pytest.raises(ValueError, match="entity_capacity must be a non-negative int"):
                make(entity_capacity=bad)
