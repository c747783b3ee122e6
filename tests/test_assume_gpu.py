"""What-if queries on the GPU: facts assumed per query on the cached plan.  Ultra.forward(delta=overlay) and
Predictor.tails / heads / tails_above(assuming=) equal predict.assume_reference -- per query a copy of the materialised graph with
its facts appended, one forward, the extended known list -- bit for bit, with and without persistent edits, tombstones, an entity
reserve, a relation reserve and retired entities; queries of one batch never see each other's facts; later calls refill the
overlay of the one captured step and record nothing.  The graph is tests/test_edit_rows_owned_gpu.py's (a hub row, an edge-less
row), the weights the golden ultra_3g_model.pt, batch_size = 3."""
import os

import pytest
import torch

from tests.test_edit_rows_owned_gpu import EMPTY, HUB, MERGE_ROW, N, R_DIRECT, TRIPLES
from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd.data import Data
from ultra_amd.live import with_facts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BATCH, K = 3, 5
OWNED = "ultra_rspmm_edit_rows_owned"
OTHERS = ("ultra_rspmm_delta_rows", "ultra_rspmm_edit_rows", "ultra_rspmm_edit_rows_split", "ultra_rspmm_edit_rows_samples")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data(dev):
    h, t, r = TRIPLES
    graph = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + R_DIRECT]),
                 num_nodes=N, num_relations=2 * R_DIRECT, target_triples=torch.stack([h, t, r], dim=-1)[:16])
    return tasks.build_relation_graph(graph.to(dev))


@pytest.fixture(scope="module")
def model(dev):
    net = models.Ultra(**synthetic.default_model_cfg())
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    return net.to(dev).eval()


def same_answers(got, want):
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and torch.equal(got[2], want[2]))


def counted(monkeypatch, names):
    calls = dict.fromkeys(names, 0)
    for name in names:
        def wrapper(*args, _name=name, _fn=getattr(_lib.lib, name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, wrapper)
    return calls


def queries(data):
    """Seven queries (three batches, the last one short); queries 0 and 1 ask the same (h, r)."""
    h, t, r = data.target_triples[:6].unbind(-1)
    return torch.cat([h[:1], h]), torch.cat([r[:1], r]), torch.cat([t[:1], t])


def assumptions(anchor, r):
    """One entry per query: into the hub and at the query's own anchor; nothing; the edge-less row, twice the same fact; an
    empty tensor; a self loop and a fact next to a tombstone; a list of tuples into the hub through its inverse; nothing."""
    a = int(anchor[0])
    return [torch.tensor([[HUB, 0, 55], [a, int(r[0]), 17], [a, int(r[0]), 18]]), None,
            torch.tensor([[EMPTY, 1, 10], [5, 2, 6], [5, 2, 6]]), torch.zeros(0, 3, dtype=torch.long),
            torch.tensor([[9, 3, 9], [MERGE_ROW, 2, 150]]), [(60, 1, HUB), (int(anchor[5]), 0, 30)], None]


SECOND = [None, [(HUB, 3, 70)], None, [(EMPTY, 0, EMPTY)], None, None, torch.tensor([[MERGE_ROW, 1, 120], [1, 1, 2]])]


def edit(live, dev):
    """Persistent edits: two facts (one into the hub) and two retractions (one out of the hub, one at the merge row)."""
    live.add_facts(torch.tensor([HUB, 40], device=dev), torch.tensor([0, 6], device=dev), torch.tensor([50, 41], device=dev))
    hub_tail = int(TRIPLES[1][TRIPLES[0] == HUB][3])
    hub_rel = int(TRIPLES[2][TRIPLES[0] == HUB][3])
    removed = live.remove_facts(torch.tensor([HUB, MERGE_ROW], device=dev), torch.tensor([hub_rel, 0], device=dev),
                                torch.tensor([hub_tail, 120], device=dev))
    assert bool((removed >= 1).all())


CONFIGS = {
    "plain": ({}, False, False),
    "edited": ({}, True, False),
    "entity_reserve": ({"entity_capacity": 4}, True, False),
    "relation_reserve": ({"relation_capacity": 2}, True, False),
    "both_reserves_retired": ({"entity_capacity": 4, "relation_capacity": 2}, True, True),
    "live_relation_graph": ({"live_relation_graph": True}, True, False),
}


def reference(model, live, anchor, r, assumed, mode, min_score=None):
    mat = live.materialized()
    retired = mat.retired_entities if len(mat.retired_entities) else None
    return predict.assume_reference(model, mat, mat, anchor, r, assumed, k=K, mode=mode, min_score=min_score, retired=retired)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_predictor_equals_the_reference(dev, data, model, monkeypatch, name):
    kwargs, edited, retire = CONFIGS[name]
    live = predict.Predictor(model, data, k=K, batch_size=BATCH, delta_capacity=16, **kwargs)
    if edited:
        edit(live, dev)
    if retire:
        live.remove_entities([250])
    if "entity_capacity" in kwargs:
        assert live.add_entities(1).tolist() == [N]
    h, r, t = queries(data)
    calls = counted(monkeypatch, (OWNED,) + OTHERS)
    for mode, anchor in (("tail", h), ("head", t)):
        ask = live.tails if mode == "tail" else live.heads
        assumed = assumptions(anchor, r)
        if "entity_capacity" in kwargs:         # (the new entity takes part like any other)
            assumed[1] = [(N, 1, int(anchor[1]))]
        got = ask(anchor, r, assuming=assumed)
        assert same_answers(got, reference(model, live, anchor, r, assumed, mode)), (name, mode)
        step = live._steps[(mode, "assume")]
        graph = step.graph
        assert not same_answers(got, ask(anchor, r))
        # other assumptions: the same step, the same recorded graph, the overlay refilled
        before = calls[OWNED]
        got = ask(anchor, r, assuming=SECOND)
        assert same_answers(got, reference(model, live, anchor, r, SECOND, mode)), (name, mode, "second")
        assert live._steps[(mode, "assume")] is step and step.graph is graph and calls[OWNED] == before
    assert calls[OWNED] > 0
    # the answer sets (eager forwards over the overlay)
    assumed = assumptions(h, r)
    got = live.tails_above(h, r, 0.0, assuming=assumed)
    want = reference(model, live, h, r, assumed, "tail", min_score=0.0)
    assert all(torch.equal(a, b) for a, b in zip(got[:2] + got[3:], want[:2] + want[3:])), name
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), name
    live.close()


def test_the_forward_over_an_overlay_equals_the_forward_on_each_graph(dev, data, model):
    for edited in (False, True):
        delta = rspmm.GraphDelta(data, capacity=16)
        if edited:
            delta.add([HUB, 40], [0, 6], [50, 41])
            delta.remove(MERGE_ROW, 0, 120)
        overlay = rspmm.AssumedFacts(data, delta, BATCH, 4)
        facts = [torch.tensor([[HUB, 1, 60], [EMPTY, 2, 3]], device=dev), None, torch.tensor([[MERGE_ROW, 4, 150]], device=dev)]
        overlay.fill(facts)
        mat = delta.materialize(data)
        for batch in tasks.all_negative(data, data.target_triples[:BATCH]):
            with torch.no_grad():
                got = model(data, batch, delta=overlay)
                for s in range(BATCH):
                    graph = mat if facts[s] is None else with_facts(mat, *facts[s].unbind(1))
                    want = model(graph, batch[s:s + 1])
                    assert torch.equal(got[s:s + 1].view(torch.int32), want.view(torch.int32)), (edited, s)
                assert not torch.equal(got[0], model(data, batch[0:1], delta=delta)[0])
        assert len(delta) == (2 if edited else 0)


def test_candidate_sets_and_assumptions_together(dev, data, model):
    """among= with assuming=: the step under its own key (mode, "assume", "among"), the eager what-if path's sets, and
    heads_above(assuming=), each against assume_reference restricted to the same sets."""
    live = predict.Predictor(model, data, k=K, batch_size=BATCH, delta_capacity=16)
    edit(live, dev)
    h, r, t = queries(data)
    shortlist = torch.arange(0, N, 3, device=dev)
    live.define_set("thirds", shortlist)
    per_query = [torch.arange(q, N, 2 + q, device=dev) for q in range(len(h))]
    mat = live.materialized()
    for mode, anchor in (("tail", h), ("head", t)):
        ask = live.tails if mode == "tail" else live.heads
        assumed = assumptions(anchor, r)
        for among, sets in (("thirds", shortlist), (per_query, per_query)):
            got = ask(anchor, r, among=among, assuming=assumed)
            want = predict.assume_reference(model, mat, mat, anchor, r, assumed, k=K, mode=mode, among=sets)
            assert same_answers(got, want), (mode, among == "thirds")
            assert not same_answers(got, ask(anchor, r, among=among))
        step = live._steps[(mode, "assume", "among")]
        got = ask(anchor, r, among="thirds", assuming=SECOND)
        assert same_answers(got, predict.assume_reference(model, mat, mat, anchor, r, SECOND, k=K, mode=mode, among=shortlist))
        assert live._steps[(mode, "assume", "among")] is step
    assert set(key for key in live._steps if isinstance(key, tuple) and "assume" in key) == {
        ("tail", "assume", "among"), ("head", "assume", "among")}
    # the answer sets of the heads, with and without a candidate set
    assumed = assumptions(t, r)
    for kwargs, sets in (({}, None), ({"among": per_query}, per_query)):
        got = live.heads_above(t, r, -0.5, assuming=assumed, **kwargs)
        want = predict.assume_reference(model, mat, mat, t, r, assumed, mode="head", min_score=-0.5, among=sets)
        assert int(got[0][-1]) > 0 and all(torch.equal(a, b) for a, b in zip(got[:2] + got[3:], want[:2] + want[3:])), sets is None
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), sets is None
    assert not same_answers(live.heads_above(t, r, -0.5, assuming=assumed)[1:], live.heads_above(t, r, -0.5)[1:])
    live.close()


def test_isolation_within_one_batch(dev, data, model):
    live = predict.Predictor(model, data, k=K, batch_size=BATCH)
    h, r, _ = queries(data)
    assert int(h[0]) == int(h[1]) and int(r[0]) == int(r[1])
    plain = live.tails(h[:3], r[:3])
    fresh = int(plain[0][0, 0])
    got = live.tails(h[:3], r[:3], assuming=[[(int(h[0]), int(r[0]), fresh), (HUB, 2, int(h[0]))], None, None])
    for q in (1, 2):        # the queries that assume nothing: the call without the argument, bit for bit
        assert same_answers([part[q:q + 1] for part in got], [part[q:q + 1] for part in plain])
    assert not torch.equal(got[1][0], plain[1][0])
    # the assumed tail is a known answer of query 0 only
    assert fresh not in got[0][0].tolist() and fresh == int(got[0][1, 0])
    live.close()


def test_a_predictor_never_given_assumptions_holds_the_steps_of_before(dev, data, model):
    live = predict.Predictor(model, data, k=K, batch_size=BATCH)
    h, r, t = queries(data)
    plain = live.tails(h, r), live.heads(t, r)
    assert set(live._steps) == {"tail", "head"}
    steps = dict(live._steps)
    # all-empty assumptions: the route and the captures of the call without the argument
    assert same_answers(live.tails(h, r, assuming=[None] * len(h)), plain[0])
    assert same_answers(live.heads(t, r, assuming=torch.zeros(0, 3, dtype=torch.long)), plain[1])
    assert set(live._steps) == {"tail", "head"} and all(live._steps[key] is steps[key] for key in steps)
    # a what-if call adds its own key and leaves the others' captures alone; nothing is stated
    edges = live.materialized().edge_index.clone()
    live.tails(h, r, assuming=assumptions(h, r))
    assert set(live._steps) == {"tail", "head", ("tail", "assume")} and all(live._steps[key] is steps[key] for key in steps)
    assert not live.delta.edited and torch.equal(live.materialized().edge_index, edges)
    assert same_answers(live.tails(h, r), plain[0])
    live.close()


def test_the_command_line_tool_assumes_by_name(dev, capsys):
    """tools/predict.py --assume H R T: the best answer of a query, assumed as its tail, is left out of that run's answers; an
    unknown name ends the tool."""
    import importlib.util
    from ultra_amd import data as udata
    root = os.path.join(GOLDEN, "kg_fixture")
    spec = importlib.util.spec_from_file_location("predict_tool", os.path.join(os.path.dirname(GOLDEN), os.pardir, "tools", "predict.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ent, rel = udata.read_vocab(root)
    triple = udata.load_triples_dir(root).target_triples[0].tolist()
    query = ["--data-root", root, "--ckpt", os.path.join(GOLDEN, "ultra_3g_model.pt"), "--head", ent[triple[0]], "--relation",
             rel[triple[2]], "-k", "5"]

    def answers(argv):
        tool.main(argv)
        lines = capsys.readouterr().out.splitlines()
        return lines, [line.split()[1] for line in lines if line[:3].strip().isdigit()]
    _, before = answers(query)
    assert len(before) == 5
    lines, after = answers(query + ["--assume", ent[triple[0]], rel[triple[2]], before[0], "--assume", before[1], rel[0], before[2]])
    assert any(line.startswith("assuming 2 fact(s)") for line in lines)
    assert len(after) == 5 and before[0] not in after
    assert answers(query)[1] == before                                   # nothing was stated
    with pytest.raises(SystemExit):
        tool.main(query + ["--assume", "no such entity", rel[0], before[0]])
    with pytest.raises(SystemExit):
        tool.main(query + ["--assume", before[0], rel[0], before[1], "--explain"])


def test_a_model_outside_the_served_set_runs_the_loop(dev, data):
    torch.manual_seed(3)
    mean = models.Ultra(**synthetic.default_model_cfg(aggregate_func="mean")).to(dev).eval()
    assert not predict.assume_supported(mean)
    live = predict.Predictor(mean, data, k=K, batch_size=BATCH)
    h, r, _ = queries(data)
    assumed = assumptions(h, r)[:3]
    got = live.tails(h[:3], r[:3], assuming=assumed)
    assert same_answers(got, reference(mean, live, h[:3], r[:3], assumed, "tail"))
    assert ("tail", "assume") not in live._steps
    live.close()
