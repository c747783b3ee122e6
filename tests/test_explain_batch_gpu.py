"""Batched path explanations on the GPU: the per-sample edge-weight gradient (ultra_rspmm_edge_grad_samples) against an exact
restatement and against the engine's own backward, the batched beam-search layer (ultra_beam_search_layer_batch) against
the plain-torch restatement of tests/test_explain_cpu.py and against the single-sample entry, edge_grads_batch /
visualize_batch against the reference's recorded gradients and paths (tests/golden/gen_explain_golden.py), and
Predictor.explain_tails / explain_heads."""
import copy
import ctypes
import os

import pytest
import torch

from tests.test_explain_cpu import load, restate_layer
from ultra_amd import _lib, explain, models, predict, rspmm, synthetic
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BEAMS = (1, 3, 10, 16)
SAMPLES = (1, 3, 5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ultra_3g(dev):
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(HERE, "golden", "ultra_3g_model.pt")))
    return model.to(dev).eval()


# ---- 1, 2: the per-sample edge-weight gradient ----
def _edge_graph(num_edge, seed=2):
    """N = 37, R = 5, unsorted, with a run of parallel edges and repeated (row, col, type) triples."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, 37, (2, num_edge), generator=g)
    et = torch.randint(0, 5, (num_edge,), generator=g)
    if num_edge >= 60:
        ei[:, 20:40] = ei[:, 19:20]         # parallel edges, types differ
        ei[:, 50:56] = ei[:, 49:50]         # the same edge six more times
        et[50:56] = et[49]
    return ei, et


def _quarters(shape, g):
    return torch.randint(-4, 5, shape, generator=g).float() / 4


def _restate_edge_grads(ei, et, rel, x, og, mul):
    """weight_grad[o, e] = sum_d og[o, row_e, d] * BINARY(rel[o, type_e, d], x[o, col_e, d]) in fp64."""
    rel, x, og = rel.double(), x.double(), og.double()
    if rel.dim() == 2:
        rel = rel.unsqueeze(0).expand(x.shape[0], -1, -1)
    r, xi = rel[:, et], x[:, ei[1]]
    return torch.einsum("oed,oed->oe", og[:, ei[0]], r * xi if mul == "mul" else r + xi)


@pytest.mark.parametrize("mul", ("mul", "add"))
@pytest.mark.parametrize("row_len", (64, 32))
def test_edge_grad_samples_are_exact_on_quarters(dev, row_len, mul):
    """Operands in {-4 .. 4} / 4: every product is a multiple of 1/64 below 2 in size and every sum of 64 of them a multiple
    of 1/64 below 128 -- exact in fp32 in any order, so the kernel must return the fp64 restatement's values exactly."""
    ei, et = _edge_graph(500)
    plan = rspmm.get_plan(ei.to(dev), et.to(dev), 37, 5, exact_order=False)
    g = torch.Generator().manual_seed(row_len)
    for num_sample in SAMPLES:
        rel, x, og = (_quarters((num_sample, n, row_len), g) for n in (5, 37, 37))
        want = _restate_edge_grads(ei, et, rel, x, og, mul)
        got = plan.edge_grad_samples(rel.to(dev), x.to(dev), og.to(dev), mul=mul)
        assert got.shape == (num_sample, 500) and got.dtype == torch.float32
        assert torch.equal(got.cpu().double(), want), (num_sample, row_len, mul)
        # one relation table for every sample (outer stride 0)
        want0 = _restate_edge_grads(ei, et, rel[0], x, og, mul)
        got0 = plan.edge_grad_samples(rel[0].to(dev), x.to(dev), og.to(dev), mul=mul)
        assert torch.equal(got0.cpu().double(), want0), (num_sample, row_len, mul)


@pytest.mark.parametrize("num_edge", (0, 1))
def test_edge_grad_samples_of_tiny_graphs(dev, num_edge):
    ei, et = _edge_graph(num_edge)
    plan = rspmm.Plan(ei.to(dev), et.to(dev), 37, 5)
    g = torch.Generator().manual_seed(3)
    rel, x, og = (_quarters((3, n, 64), g) for n in (5, 37, 37))
    for mul in ("mul", "add"):
        got = plan.edge_grad_samples(rel.to(dev), x.to(dev), og.to(dev), mul=mul)
        assert got.shape == (3, num_edge)
        assert torch.equal(got.cpu().double(), _restate_edge_grads(ei, et, rel, x, og, mul))


@pytest.mark.parametrize("mul", ("mul", "add"))
@pytest.mark.parametrize("row_len", (64, 32))
def test_edge_grad_samples_match_the_engine_backward_bit_for_bit(dev, row_len, mul):
    """Slice s is the weight_grad of ultra_rspmm_backward for sample s alone (2-D operands, weights that require grad -- the
    call of layers.edge_grad_layer), and two runs agree."""
    ei, et = _edge_graph(500)
    ei, et = ei.to(dev), et.to(dev)
    plan = rspmm.get_plan(ei, et, 37, 5, exact_order=False)
    g = torch.Generator().manual_seed(100 + row_len)
    for num_sample in SAMPLES:
        rel, x, og = (torch.randn((num_sample, n, row_len), generator=g).to(dev) for n in (5, 37, 37))
        got = plan.edge_grad_samples(rel, x, og, mul=mul)
        again = plan.edge_grad_samples(rel, x, og, mul=mul)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        for s in range(num_sample):
            weight = torch.ones(500, device=dev, requires_grad=True)
            out = rspmm.plan_rspmm(plan, rel[s], x[s], weight, sum="add", mul=mul)
            want, = torch.autograd.grad(out, weight, og[s])
            assert torch.equal(got[s].view(torch.int32), want.view(torch.int32)), (num_sample, s, row_len, mul)


# ---- 3, 4: the batched beam-search layer ----
def _hub_graph():
    """The graph of tests/test_explain_gpu.py::test_kernel_matches_restatement_with_hub_rows (n = 300, E = 6000, in-degrees 257 /
    743 / 3000 at rows 8 / 9 / 7), with the out-edges of node 299 moved to node 298: a head without out-edges."""
    g = torch.Generator().manual_seed(5)
    n = 300
    src = torch.randint(0, n, (6000,), generator=g)
    dst = torch.cat([torch.randint(0, n, (2000,), generator=g), torch.full((3000,), 7), torch.full((257,), 8),
                     torch.full((743,), 9)])
    src[100:120] = src[99]
    dst[100:120] = dst[99]
    ei = torch.stack([src, dst[torch.randperm(6000, generator=g)]])
    et = torch.randint(0, 5, (6000,), generator=g)
    et[100:120] = et[99]
    ei[0][ei[0] == 299] = 298
    grads = [torch.randint(-40, 41, (5, 6000), generator=g).float() / 8 for _ in range(4)]
    # sample 1: the tail is the 3,000-edge hub row; sample 2: the head has no out-edges (every layer all -inf)
    return dict(name="hub", edge_index=ei, edge_type=et, num_nodes=n, grads=grads, heads=[3, 11, 299, 8, 250],
                tails=[7, 7, 9, 120, 8])


def _golden_beam_graph(case):
    """A golden `beam` graph with five samples: the case's own triple and gradients first, then the gradients permuted among
    the edges, other heads -- one without out-edges where the graph has such a node -- and other tails."""
    ei, n = case["edge_index"], case["num_nodes"]
    g = torch.Generator().manual_seed(len(case["name"]))
    grads = [torch.stack([x] + [x[torch.randperm(x.numel(), generator=g)] for _ in range(4)]) for x in case["edge_grads"]]
    out_deg = torch.bincount(ei[0], minlength=n)
    dead = (out_deg == 0).nonzero().flatten().tolist()
    busy = torch.argsort(out_deg, descending=True, stable=True).tolist()
    heads = [case["h"], busy[0], dead[0] if dead else busy[1], busy[2], case["t"]]
    tails = [case["t"], busy[3], case["t"], case["h"], busy[0]]
    return dict(name=case["name"], edge_index=ei, edge_type=case["edge_type"], num_nodes=n, grads=grads, heads=heads,
                tails=tails)


_GRAPHS = {}


def _beam_graphs(dev):
    if not _GRAPHS:
        for graph in [_golden_beam_graph(c) for c in load()["beam"]] + [_hub_graph()]:
            graph["edge_index"], graph["edge_type"] = graph["edge_index"].to(dev), graph["edge_type"].to(dev)
            graph["grads"] = [x.to(dev) for x in graph["grads"]]
            graph["data"] = Data(edge_index=graph["edge_index"], edge_type=graph["edge_type"], num_nodes=graph["num_nodes"],
                                 num_relations=int(graph["edge_type"].max()) + 1)
            _GRAPHS[graph["name"]] = graph
    return list(_GRAPHS.values())


_RESTATED = {}


def _restated(graph, k):
    """The restated chain of all five samples of a graph, computed once per beam width: per layer the (5, N, K) input and the
    (5, N, K) / (5, N, K, 4) output.  Never modified."""
    key = (graph["name"], k)
    if key not in _RESTATED:
        n, dev = graph["num_nodes"], graph["edge_index"].device
        dist = torch.full((5, n, k), float("-inf"), device=dev)
        dist[torch.arange(5, device=dev), torch.tensor(graph["heads"], device=dev), 0] = 0
        layers = []
        for grad in graph["grads"]:
            outs = [restate_layer(graph["edge_index"], graph["edge_type"], grad[s], dist[s], graph["tails"][s], k)
                    for s in range(5)]
            want_d, want_b = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
            layers.append((dist, want_d, want_b))
            dist = want_d
        _RESTATED[key] = layers
    return _RESTATED[key]


def test_beam_graphs_cover_the_cases(dev):
    graphs = _beam_graphs(dev)
    assert len(graphs) == len(load()["beam"]) + 1
    hub = _GRAPHS["hub"]
    csr = explain.beam_csr(hub["edge_index"], hub["edge_type"], hub["num_nodes"])
    assert csr.num_hub >= 3 and set(csr.hub_rows.tolist()) >= {7, 8, 9} and hub["tails"][1] == 7
    assert not (hub["edge_index"][0] == 299).any() and hub["heads"][2] == 299
    assert all(torch.isinf(want_d[2]).all() and not want_b[2].any() for _, want_d, want_b in _restated(hub, 3))
    assert any(torch.isfinite(want_d[1][7]).any() for _, want_d, _ in _restated(hub, 3))      # the hub tail is reached


@pytest.mark.parametrize("k", BEAMS)
def test_batched_layer_matches_restatement(dev, k):
    """Every layer, every sample: distance bits and back edges of the restatement, on the restatement's previous layer."""
    for graph in _beam_graphs(dev):
        csr = explain.beam_csr(graph["edge_index"], graph["edge_type"], graph["num_nodes"])
        for num_sample in SAMPLES:
            tails = torch.tensor(graph["tails"][:num_sample], device=dev)
            for i, (dist_in, want_d, want_b) in enumerate(_restated(graph, k)):
                got_d, got_b = explain.beam_search_layer_batch(csr, graph["grads"][i][:num_sample], dist_in[:num_sample], tails, k)
                got_b = got_b * torch.isfinite(got_d).flatten(1).any(1).view(-1, 1, 1, 1)     # (the all -inf rule, per sample)
                where = (graph["name"], k, num_sample, i)
                assert torch.equal(got_d.view(torch.int32), want_d[:num_sample].view(torch.int32)), where
                assert torch.equal(got_b, want_b[:num_sample]), where


@pytest.mark.parametrize("k", BEAMS)
def test_batched_search_matches_single_entry(dev, k):
    """The whole chain through beam_search_distance_batch: sample s is beam_search_distance of triple s, bit for bit."""
    for graph in _beam_graphs(dev):
        singles = [explain.beam_search_distance(graph["data"], [x[s] for x in graph["grads"]], graph["heads"][s],
                                                graph["tails"][s], k) for s in range(5)]
        for num_sample in SAMPLES:
            dists, backs = explain.beam_search_distance_batch(graph["data"], [x[:num_sample] for x in graph["grads"]],
                                                              graph["heads"][:num_sample], graph["tails"][:num_sample], k)
            assert len(dists) == len(backs) == len(graph["grads"])
            for i in range(len(dists)):
                for s in range(num_sample):
                    where = (graph["name"], k, num_sample, i, s)
                    assert torch.equal(dists[i][s].view(torch.int32), singles[s][0][i].view(torch.int32)), where
                    assert torch.equal(backs[i][s], singles[s][1][i]), where
        # ... and the paths read from the tables
        got = explain.topk_average_length_batch(dists, backs, graph["tails"], k)
        for s in range(5):
            want = explain.topk_average_length(singles[s][0], singles[s][1], graph["tails"][s], k)
            assert (list(got[s][0]), list(got[s][1])) == (list(want[0]), list(want[1])), (graph["name"], k, s)


# ---- 5 .. 7: the models ----
def _golden_data(vis, dev):
    rel_graph = Data(edge_index=vis["rel_edge_index"], edge_type=vis["rel_edge_type"], num_nodes=vis["num_relations"],
                     num_relations=4)
    data = Data(edge_index=vis["edge_index"], edge_type=vis["edge_type"], num_nodes=vis["num_nodes"],
                num_relations=vis["num_relations"])
    data.relation_graph = rel_graph
    return synthetic.to_device(data, dev)


def test_edge_grads_batch_match_reference_and_single_triples(dev, monkeypatch):
    """All 8 golden triples as one batch, the reference's relation representations installed.  Against the reference's
    gradients: the tolerance of test_edge_grads_match_reference_and_unfused_route.  Against edge_grads of each triple alone:
    bit for bit -- measured on the MI355X, every kernel of the forward and the backward gives a sample the same bits
    whatever else is in the batch."""
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    ent = _ultra_3g(dev).entity_model
    batch = torch.cat([tr["batch"] for tr in vis["triples"]]).to(dev)
    reps = torch.cat([tr["relation_representations"] for tr in vis["triples"]]).to(dev)
    assert batch.shape == (8, 3) and reps.shape[0] == 8
    ent.query = reps

    def no_fallback(*args):
        raise AssertionError("edge_grads_batch explained this sum / DistMult model triple by triple")

    with monkeypatch.context() as patch:         # (the batched route itself, not the per-triple loop behind it)
        patch.setattr(ent, "edge_grads", no_fallback)
        got, scores = ent.edge_grads_batch(data, batch)
    assert len(got) == 6 and all(g.shape == (8, data.num_edges) for g in got) and scores.shape == (8,)
    worst, unequal, unequal_scores = 0.0, 0, 0
    for s, tr in enumerate(vis["triples"]):
        ent.query = tr["relation_representations"].to(dev)
        single, score = ent.edge_grads(data, tr["batch"].to(dev))
        for i, want in enumerate(tr["edge_grads"]):
            want = want.to(dev)
            atol = 1e-6 * float(want.abs().max())
            torch.testing.assert_close(got[i][s], want, rtol=1e-4, atol=atol)
            torch.testing.assert_close(got[i][s], single[i], rtol=1e-4, atol=atol)
            worst = max(worst, float((got[i][s] - single[i]).abs().max()))
            unequal += int(not torch.equal(got[i][s].view(torch.int32), single[i].view(torch.int32)))
        torch.testing.assert_close(scores[s:s + 1], score, rtol=1e-5, atol=1e-6)
        unequal_scores += int(not torch.equal(scores[s:s + 1], score))
    print("edge_grads_batch vs edge_grads: max |difference| = %g, %d of 48 (layer, triple) pairs and %d of 8 scores differ in bits"
          % (worst, unequal, unequal_scores))
    assert unequal == 0


def _compare_paths(paths, weights, want_paths, want_weights):
    """The rule of tests/test_explain_gpu.py::_assert_paths_match; returns how many paths were compared."""
    assert len(paths) == len(want_paths)
    w, ww = torch.tensor(list(weights), dtype=torch.float64), torch.tensor(list(want_weights), dtype=torch.float64)
    torch.testing.assert_close(w, ww, rtol=1e-4, atol=1e-6 * float(ww.abs().max()))
    tol = 1e-4 * ww.abs() + 1e-6 * float(ww.abs().max())
    compared = 0
    for i in range(len(ww)):
        separated = all(abs(float(ww[i] - ww[j])) > float(tol[i]) for j in (i - 1, i + 1) if 0 <= j < len(ww))
        if separated:
            assert list(paths[i]) == list(want_paths[i]), i
            compared += 1
    return compared


def test_ultra_visualize_batch_returns_reference_paths(dev):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    batch = torch.cat([tr["batch"] for tr in vis["triples"]]).to(dev)
    got = model.visualize_batch(data, batch)
    assert len(got) == 8
    compared = 0
    for (paths, weights), tr in zip(got, vis["triples"]):
        assert all(isinstance(p, list) and all(isinstance(e, tuple) and len(e) == 3 for e in p) for p in paths)
        compared += _compare_paths(paths, weights, tr["paths"], tr["weights"])
    assert sum(len(tr["paths"]) for tr in vis["triples"]) == 80
    assert compared >= 72, compared        # (the golden weights alone separate 76 of the 80)
    # chunks of 3 (3 + 3 + 2 triples) against the one chunk of 8, and a repeated triple
    assert model.visualize_batch(data, batch, chunk=3) == got
    again = model.visualize_batch(data, batch[[2, 5, 2, 0, 2]])
    assert again == [got[2], got[5], got[2], got[0], got[2]]
    assert model.visualize_batch(data, batch[:0]) == []


def test_visualize_batch_leaves_the_model_as_it_was(dev):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    golden = torch.load(os.path.join(HERE, "golden", "model_ultra_3g_sum.pt"))
    t_batch = golden["t_batch"].to(dev)
    batch = torch.cat([tr["batch"] for tr in vis["triples"]]).to(dev)
    with torch.no_grad():
        before = model(data, t_batch)
    ent = model.entity_model
    installed = (ent.query, [l.relation for l in ent.layers], ent._last_hidden_on_rows)
    params = copy.deepcopy(model.state_dict())
    model.visualize_batch(data, batch[:3])
    assert not model.training
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, params[k]) for k, v in model.state_dict().items())
    assert ent.query is installed[0] and all(l.relation is r for l, r in zip(ent.layers, installed[1]))
    assert ent._last_hidden_on_rows == installed[2]
    with torch.no_grad():
        after = model(data, t_batch)
    assert torch.equal(before, after)
    model.train()
    model.visualize_batch(data, batch[3:5], chunk=1)
    assert model.training
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, params[k]) for k, v in model.state_dict().items())


# ---- 8: serving ----
def _all_but(keep, num_node):
    return torch.tensor([v for v in range(num_node) if v not in keep])


def test_predictor_explains_its_answers(dev):
    """The golden graph with the ultra_3g weights, k = 3, two queries a direction; the second query of each direction knows
    every answer but two (a filter graph made for it), so its count -- and its list of explanations -- is 2."""
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    n, num_direct = data.num_nodes, data.num_relations // 2
    triples = torch.cat([tr["batch"] for tr in vis["triples"]])
    (h0, _, r0), (h1, _, r1) = triples[0].tolist(), triples[1].tolist()
    r0, r1 = r0 % num_direct, r1 % num_direct
    others = [v for v in range(n) if v != h1]
    open_t, open_h = {others[5], others[9]}, {others[4], others[17]}      # the two answers each direction does not know yet
    known_t, known_h = _all_but(open_t, n), _all_but(open_h, n)
    filt = Data(edge_index=torch.cat([torch.stack([torch.full_like(known_t, h1), known_t]),
                                      torch.stack([known_h, torch.full_like(known_h, h1)])], dim=1),
                edge_type=torch.full((len(known_t) + len(known_h),), r1), num_nodes=n, num_relations=data.num_relations)
    predictor = predict.Predictor(model, data, k=3, batch_size=2, filtered_data=synthetic.to_device(filt, dev))
    anchor, relation = torch.tensor([h0, h1], device=dev), torch.tensor([r0, r1], device=dev)
    for mode in ("tail", "head"):
        ids, scores, count = (predictor.tails if mode == "tail" else predictor.heads)(anchor, relation)
        ids, scores, count = ids.clone(), scores.clone(), count.clone()
        e_ids, e_scores, e_count, why = (predictor.explain_tails if mode == "tail" else predictor.explain_heads)(anchor, relation)
        assert torch.equal(e_ids, ids) and torch.equal(e_count, count)
        assert torch.equal(e_scores.view(torch.int32), scores.view(torch.int32))
        assert count.tolist() == [3, 2] and [len(w) for w in why] == [3, 2]
        assert set(ids[1, :2].tolist()) == (open_t if mode == "tail" else open_h)
        for i in range(2):
            r = int(relation[i]) + (num_direct if mode == "head" else 0)
            documented = torch.tensor([[int(anchor[i]), int(ids[i, j]), r] for j in range(int(count[i]))], device=dev)
            assert why[i] == model.visualize_batch(data, documented)
            for j, (paths, weights) in enumerate(why[i]):
                assert len(paths) == len(weights)
                for path in paths:
                    assert path[0][0] == int(anchor[i]) and path[-1][1] == int(ids[i, j])
                    assert all(a[1] == b[0] for a, b in zip(path, path[1:]))
        assert any(paths for per_query in why for paths, _ in per_query)      # (something was explained)
    predictor.close()

    class Scores(torch.nn.Module):
        def forward(self, data, batch):
            return torch.zeros(batch.shape[:2], device=batch.device)

    with pytest.raises(TypeError, match="Ultra"):
        predict.Predictor(Scores(), data, k=3, batch_size=2, use_graph=False).explain_tails(anchor, relation)


# ---- 9: arguments ----
def test_invalid_arguments_raise(dev):
    case = load()["beam"][0]
    ei, et = case["edge_index"].to(dev), case["edge_type"].to(dev)
    n = case["num_nodes"]
    data = Data(edge_index=ei, edge_type=et, num_nodes=n, num_relations=int(et.max()) + 1)
    csr = explain.beam_csr(ei, et, n)
    g = torch.stack([case["edge_grads"][0]] * 2).to(dev)
    d = torch.full((2, n, 4), float("-inf"), device=dev)
    tails = torch.tensor([case["t"], 0], device=dev)
    # S = 0: empty results
    d0, b0 = explain.beam_search_layer_batch(csr, g[:0], d[:0], tails[:0], 4)
    assert d0.shape == (0, n, 4) and b0.shape == (0, n, 4, 4)
    dists, backs = explain.beam_search_distance_batch(data, [g[:0]] * 2, [], [], 4)
    assert [x.shape for x in dists] == [(0, n, 4)] * 2 and explain.topk_average_length_batch(dists, backs, [], 4) == []
    for k in (0, 65, 100):
        with pytest.raises(ValueError):
            explain.beam_search_layer_batch(csr, g, torch.full((2, n, k), float("-inf"), device=dev), tails, k)
        with pytest.raises(ValueError):
            explain.beam_search_distance_batch(data, [g], [0, 1], tails, k)
    with pytest.raises(TypeError):
        explain.beam_search_layer_batch(csr, g.double(), d, tails, 4)
    with pytest.raises(TypeError):
        explain.beam_search_layer_batch(csr, g, d.half(), tails, 4)
    for bad_g, bad_d, bad_t in ((g[:, :-1], d, tails), (g[0], d, tails), (g, d[:, :-1], tails), (g, d[:1], tails),
                                (g, d, tails[:1]), (g, d, torch.tensor([0, n], device=dev)),
                                (g, d, torch.tensor([-1, 0], device=dev)), (g, d, [0, n])):
        with pytest.raises(ValueError):
            explain.beam_search_layer_batch(csr, bad_g, bad_d, bad_t, 4)
    with pytest.raises(ValueError):
        explain.beam_search_distance_batch(data, [g], [0, n], tails, 4)
    with pytest.raises(ValueError):
        explain.beam_search_distance_batch(data, [g], [0, 1], [0, n], 4)
    with pytest.raises(ValueError):
        explain.beam_search_distance_batch(data, [g], [0, 1, 2], tails, 4)
    # the C entry point itself
    out_d, out_b = torch.empty_like(d), torch.empty(2, n, 4, 4, dtype=torch.int64, device=dev)

    def call(num_sample, dist_in, tails_ptr, k):
        return _lib.lib.ultra_beam_search_layer_batch(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(),
                                                      csr.eid.data_ptr(), None, 0, n, csr.num_edge, num_sample, g.data_ptr(),
                                                      dist_in, tails_ptr, k, out_d.data_ptr(), out_b.data_ptr(), None)

    assert call(2, d.data_ptr(), tails.data_ptr(), 65) == _lib.ULTRA_ERR_UNSUPPORTED and b"num_beam" in _lib.lib.ultra_last_error()
    assert call(2, None, tails.data_ptr(), 4) == _lib.ULTRA_ERR_INVALID and b"dist_in" in _lib.lib.ultra_last_error()
    assert call(2, d.data_ptr(), None, 4) == _lib.ULTRA_ERR_INVALID and b"tails" in _lib.lib.ultra_last_error()
    assert call(-1, d.data_ptr(), tails.data_ptr(), 4) == _lib.ULTRA_ERR_INVALID and b"num_sample" in _lib.lib.ultra_last_error()
    assert call(0, None, None, 4) == _lib.ULTRA_OK
    # the edge-gradient entry: what it does not serve answers ULTRA_ERR_UNSUPPORTED (Python: None, the callers fall back)
    ei2, et2 = _edge_graph(500)
    plan = rspmm.get_plan(ei2.to(dev), et2.to(dev), 37, 5, exact_order=False)
    rel, x = torch.randn(2, 5, 64, device=dev), torch.randn(2, 37, 64, device=dev)
    assert plan.edge_grad_samples(rel, x, x, sum="max") is None
    assert plan.edge_grad_samples(rel, x, x, mul="rotate") is None
    assert plan.edge_grad_samples(rel.double(), x.double(), x.double()) is None
    with pytest.raises(ValueError):
        plan.edge_grad_samples(rel, x, x[:, :-1])
    with pytest.raises(ValueError):
        plan.edge_grad_samples(rel, x[:1], x)
    with pytest.raises(ValueError):
        plan.edge_grad_samples(rel[:, :4], x, x)
    _, mrel = rspmm.as_mat(rel)
    _, mx = rspmm.as_mat(x)
    out = torch.empty(2, 500, device=dev)

    def grads(sum, mul, dtype, mog, stride=500):
        return _lib.lib.ultra_rspmm_edge_grad_samples(plan._h, sum, mul, dtype, ctypes.byref(mrel), ctypes.byref(mx), mog,
                                                      out.data_ptr(), stride, None)

    for args, word in (((1, 0, _lib.F32), b"sum"), ((0, 2, _lib.F32), b"mul"), ((0, 0, _lib.F64), b"dtype")):
        assert grads(*args, ctypes.byref(mx)) == _lib.ULTRA_ERR_UNSUPPORTED and word in _lib.lib.ultra_last_error()
    assert grads(0, 0, _lib.F32, None) == _lib.ULTRA_ERR_INVALID and b"output_grad" in _lib.lib.ultra_last_error()
    assert grads(0, 0, _lib.F32, ctypes.byref(mx), stride=499) == _lib.ULTRA_ERR_INVALID
    assert b"weight_grad_stride" in _lib.lib.ultra_last_error()
    _, short = rspmm.as_mat(x[:, :-1])
    assert grads(0, 0, _lib.F32, ctypes.byref(short)) == _lib.ULTRA_ERR_INVALID and b"output_grad" in _lib.lib.ultra_last_error()
    # the models: a batch is (S, 3), with the representations of its S query relations installed
    vis = load()["visualize"]
    model = _ultra_3g(dev)
    gdata = _golden_data(vis, dev)
    with pytest.raises(ValueError):
        model.visualize_batch(gdata, torch.zeros(3, dtype=torch.long, device=dev))
    with pytest.raises(ValueError):
        model.visualize_batch(gdata, torch.zeros(2, 3, dtype=torch.long, device=dev), chunk=0)
    model.entity_model.query = vis["triples"][0]["relation_representations"].to(dev)
    with pytest.raises(ValueError):
        model.entity_model.edge_grads_batch(gdata, torch.zeros(2, 3, dtype=torch.long, device=dev))
