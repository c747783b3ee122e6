"""Explanations on a graph that holds edits, the parts that need no GPU: GraphDelta's destination-keyed layout
against materialize(), the keep vector against surviving(), predict.explain_live_supported, and the argument rules of
Predictor.explain_tails / explain_heads(compact=)."""
import pytest
import torch

from ultra_amd import models, predict, rspmm, synthetic
from ultra_amd.data import Data


def make_model(message_func="distmult", aggregate_func="sum", seed=0):
    torch.manual_seed(seed)
    return models.Ultra(**synthetic.default_model_cfg(message_func=message_func, aggregate_func=aggregate_func)).eval()


def _graph(seed):
    """N = 40, R = 3 direct relations, loader form [direct ; inverse], with parallel edges (ten direct edges stated twice)."""
    g = torch.Generator().manual_seed(seed)
    h, t = torch.randint(0, 40, (2, 110), generator=g)
    r = torch.randint(0, 3, (110,), generator=g)
    h, t, r = torch.cat([h, h[:10]]), torch.cat([t, t[:10]]), torch.cat([r, r[:10]])
    return Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + 3]), num_nodes=40,
                num_relations=6)


def _facts(data):
    direct = data.edge_type < 3
    return list(zip(data.edge_index[0][direct].tolist(), data.edge_type[direct].tolist(), data.edge_index[1][direct].tolist()))


def _quiet_fact(data, busy):
    """A base fact whose two ends no edit of `busy` touches: its rows are touched by this removal only."""
    nodes = {v for f in busy for v in (f[0], f[2])}
    for f in _facts(data):
        if f[0] not in nodes and f[2] not in nodes and f[0] != f[2]:
            return f
    raise AssertionError("no quiet fact")


def _edit(data, delta):
    """Parallel edges (a base fact stated again), a fact added twice, a fact removed and then added again, a duplicated base
    fact removed (one key, two slots), and a row touched by removals only.  Returns the fact of that row."""
    base = _facts(data)
    twice = (7, 1, 22)
    adds = [base[20], twice, twice, (3, 0, 3), (22, 2, 7)]          # (a self loop too)
    delta.add(*zip(*adds))
    again = base[30]
    delta.remove(*zip(*[again, base[2]]))                            # base[2] is one of the ten duplicated facts
    delta.add(*zip(*[again]))
    quiet = _quiet_fact(data, adds + [again, base[2]])
    delta.remove(*zip(*[quiet]))
    return quiet


def _in_edges(edge_index, edge_type, v):
    at = (edge_index[1] == v).nonzero().flatten()
    return list(zip(edge_index[0][at].tolist(), edge_type[at].tolist()))


def _check_layout(data, delta):
    lay, mat = delta.explain, delta.materialize()
    m2 = 2 * len(delta)
    add_index, add_type = delta.edges()
    count = int(lay.count)
    rows = lay.rows[:count].tolist()
    assert rows == sorted(set(rows))
    dead_dst = [(k // 6) % 40 for k in delta.dead_keys]
    assert set(rows) == set(add_index[1].tolist()) | set(dead_dst)
    assert int(lay.add_ptr[0]) == 0 and int(lay.add_ptr[count]) == m2 and int(lay.dead_ptr[count]) == len(delta.dead_keys)
    seen = []
    for k, v in enumerate(rows):
        a0, a1 = int(lay.add_ptr[k]), int(lay.add_ptr[k + 1])
        d0, d1 = int(lay.dead_ptr[k]), int(lay.dead_ptr[k + 1])
        dead = list(zip(lay.dead_src[d0:d1].tolist(), lay.dead_type[d0:d1].tolist()))
        assert dead == sorted(set(dead))                              # (distinct and sorted: a binary search finds them)
        js = lay.add_j[a0:a1].tolist()
        assert js == sorted(js) and lay.add_dst[a0:a1].tolist() == [v] * len(js)
        for at, j in zip(range(a0, a1), js):
            assert (int(lay.add_src[at]), int(lay.add_type[at])) == (int(add_index[0][j]), int(add_type[j]))
        seen += js
        base = [e for e in _in_edges(data.edge_index, data.edge_type, v) if e not in set(dead)]
        added = list(zip(lay.add_src[a0:a1].tolist(), lay.add_type[a0:a1].tolist()))
        assert base + added == _in_edges(mat.edge_index, mat.edge_type, v), v
    assert sorted(seen) == list(range(m2))
    # the transpose: the same 2 m edges, grouped by source, ascending j within a source
    src_count = int(lay.src_count)
    sources = lay.src_rows[:src_count].tolist()
    assert sources == sorted(set(add_index[0].tolist())) and int(lay.src_ptr[src_count]) == m2
    seen = []
    for k, u in enumerate(sources):
        s0, s1 = int(lay.src_ptr[k]), int(lay.src_ptr[k + 1])
        js = lay.src_j[s0:s1].tolist()
        assert js == sorted(js) and s1 > s0
        for at, j in zip(range(s0, s1), js):
            assert (u, int(lay.src_dst[at]), int(lay.src_type[at])) == (int(add_index[0][j]), int(add_index[1][j]), int(add_type[j]))
        seen += js
    assert sorted(seen) == list(range(m2))
    # the keep vector is surviving()'s mask
    keep = delta.keep_vector()
    assert keep.dtype == torch.float32 and keep.shape == (data.edge_index.shape[1],)
    kept_index, kept_type = delta.surviving(data.edge_index, data.edge_type)
    assert torch.equal(data.edge_index[:, keep.bool()], kept_index) and torch.equal(data.edge_type[keep.bool()], kept_type)
    assert set(keep.tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_destination_layout_equals_the_materialised_rows(seed):
    data = _graph(seed)
    delta = rspmm.GraphDelta(data, capacity=12)
    assert delta.explain is None                                       # (laid out when first asked for)
    operand = delta.explain_operand()
    assert int(delta.explain.count) == 0 and operand.capacity_rows == operand.capacity_edges == operand.capacity_keys == 24
    pointers = [t.data_ptr() for t in delta.explain]
    count = delta.explain.count
    assert torch.equal(delta.keep_vector(), torch.ones(data.edge_index.shape[1]))
    quiet = _edit(data, delta)
    assert delta.explain.count is count and [t.data_ptr() for t in delta.explain] == pointers
    _check_layout(data, delta)
    # the quiet fact's rows hold tombstones and no added edge
    lay = delta.explain
    rows = lay.rows[:int(lay.count)].tolist()
    for v in (quiet[0], quiet[2]):
        k = rows.index(v)
        assert int(lay.add_ptr[k]) == int(lay.add_ptr[k + 1]) and int(lay.dead_ptr[k]) < int(lay.dead_ptr[k + 1])
    # every added fact retracted: the touched rows are the tombstoned ones alone
    held = delta.facts[:len(delta)].tolist()
    delta.remove(*zip(*[tuple(f) for f in held]))
    assert len(delta) == 0 and delta.num_removed > 0
    _check_layout(data, delta)
    assert int(lay.count) == len({(k // 6) % 40 for k in delta.dead_keys}) and int(lay.src_count) == 0
    assert [t.data_ptr() for t in delta.explain] == pointers
    # ... and the keep vector follows the version
    version_keep = delta.keep_vector()
    assert delta.keep_vector() is version_keep
    delta.add(1, 0, 2)
    assert delta.keep_vector() is not version_keep
    _check_layout(data, delta)


def test_a_delta_laid_out_late_holds_the_edits_made_before():
    data = _graph(5)
    delta = rspmm.GraphDelta(data, capacity=12)
    _edit(data, delta)
    assert delta.explain is None
    delta.explain_operand()
    _check_layout(data, delta)


# ---- the predicate and the argument rules ----
def test_explain_live_supported_names_what_it_does_not_serve():
    assert predict.explain_live_supported(make_model())
    assert predict.explain_live_supported(make_model().entity_model)
    for kwargs, word in (({"aggregate_func": "mean"}, "mean"), ({"message_func": "rotate"}, "rotate"),
                         ({"aggregate_func": "max"}, "max")):
        model = make_model(**kwargs)
        assert not predict.explain_live_supported(model)
        assert "entity layer 0" in predict.explain_live_blocker(model) and word in predict.explain_live_blocker(model)

    class Scores(torch.nn.Module):
        def forward(self, data, batch):
            return torch.zeros(batch.shape[:2])

    assert not predict.explain_live_supported(Scores())


@pytest.fixture(scope="module")
def kg():
    return synthetic.make_kg(num_node=40, num_triple=120, num_relation_base=3, num_test=8, seed=11)


def test_compact_false_on_an_unsupported_model_raises(kg):
    for kwargs in ({"aggregate_func": "mean"}, {"message_func": "rotate"}):
        predictor = predict.Predictor(make_model(**kwargs), kg, k=3, batch_size=2, delta_capacity=8, use_graph=False)
        for call in (predictor.explain_tails, predictor.explain_heads):
            with pytest.raises(ValueError, match="entity layer 0"):
                call([0], [1], compact=False)


def test_compact_must_be_a_bool(kg):
    predictor = predict.Predictor(make_model(), kg, k=3, batch_size=2, delta_capacity=8, use_graph=False)
    for bad in (0, 1, None, "no"):
        with pytest.raises(ValueError, match="compact"):
            predictor.explain_tails([0], [1], compact=bad)
        with pytest.raises(ValueError, match="compact"):
            predictor.explain_heads([0], [1], compact=bad)


class _Recorder(object):
    """Stands in for the model's answers and explanations: records what visualize_batch is called with."""

    def __init__(self, predictor, monkeypatch):
        self.calls = []

        def run(anchor, relation, mode):
            n = len(torch.as_tensor(anchor).flatten())
            return torch.arange(3).repeat(n, 1) + 5, torch.zeros(n, 3), torch.full((n,), 2)

        def visualize_batch(data, triples, chunk=16, delta=None):
            self.calls.append((data, triples.clone(), chunk, delta))
            return [([[(0, 1, 0)]], [1.0])] * len(triples)

        monkeypatch.setattr(predictor, "_run", run)
        monkeypatch.setattr(predictor.model, "visualize_batch", visualize_batch, raising=False)


def test_an_unedited_delta_takes_the_compacting_call(kg, monkeypatch):
    predictor = predict.Predictor(make_model(), kg, k=3, batch_size=2, delta_capacity=8, use_graph=False)
    seen = _Recorder(predictor, monkeypatch)
    assert predictor.delta is not None and not predictor.delta.edited
    out_true = predictor.explain_tails([0, 4], [1, 2], chunk=5, compact=True)
    out_false = predictor.explain_tails([0, 4], [1, 2], chunk=5, compact=False)
    (data0, triples0, chunk0, delta0), (data1, triples1, chunk1, delta1) = seen.calls
    assert data0 is data1 is predictor.data and torch.equal(triples0, triples1) and chunk0 == chunk1 == 5
    assert delta0 is None and delta1 is None                        # (no delta is handed over)
    assert out_true[3] == out_false[3]


def test_an_edited_delta_stays_a_delta_with_compact_false(kg, monkeypatch):
    predictor = predict.Predictor(make_model(), kg, k=3, batch_size=2, delta_capacity=8, use_graph=False)
    seen = _Recorder(predictor, monkeypatch)
    predictor.add_facts([0], [1], [9])
    data, delta = predictor.data, predictor.delta
    ids, scores, count, why = predictor.explain_heads([0, 4], [1, 2], compact=False)
    assert predictor.delta is delta and delta.edited and predictor.data is data
    (seen_data, triples, _, seen_delta), = seen.calls
    assert seen_data is data and seen_delta is delta
    assert triples.tolist() == [[0, 5, 4], [0, 6, 4], [4, 5, 5], [4, 6, 5]]      # (the inverse relation, two answers a query)
    assert [len(w) for w in why] == [2, 2]
    # ... and the default still folds the edits in first
    predictor.explain_heads([0, 4], [1, 2])
    assert not predictor.delta.edited and seen.calls[-1][3] is None
    assert predictor.data.edge_index.shape[1] == kg.edge_index.shape[1] + 2
