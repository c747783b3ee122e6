"""Path explanations on the GPU: the HIP beam search (csrc/beam_search.hip) bit for bit against the plain-torch restatement
of tests/test_explain_cpu.py, the edge gradients of the plan-based rspmm route against the reference's and the unfused
route's, and Ultra.visualize against the reference's paths (tests/golden/gen_explain_golden.py)."""
import copy
import os

import pytest
import torch

from tests.test_explain_cpu import load, restate_layer
from ultra_amd import _lib, explain, models, synthetic
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BEAMS = (1, 3, 10, 16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ultra_3g(dev):
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(HERE, "golden", "ultra_3g_model.pt")))
    return model.to(dev).eval()


def _check_layers(ei, et, num_node, grads, h, t, k):
    """Every layer of the kernel against the restatement on the same inputs (the restatement's previous layer)."""
    csr = explain.beam_csr(ei, et, num_node)
    dist_in = torch.full((num_node, k), float("-inf"), device=ei.device)
    dist_in[h, 0] = 0
    for i, g in enumerate(grads):
        want_d, want_b = restate_layer(ei, et, g, dist_in, t, k)
        got_d, got_b = explain.beam_search_layer(csr, g, dist_in, t, k)
        got_b = got_b * torch.isfinite(got_d).any()      # (the all -inf rule of beam_search_distance)
        assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)), (k, i)     # bits, -inf included
        assert torch.equal(got_b, want_b), (k, i)
        dist_in = want_d
    return csr


@pytest.mark.parametrize("k", BEAMS)
def test_kernel_matches_restatement_on_golden_graphs(dev, k):
    for case in load()["beam"]:
        ei, et = case["edge_index"].to(dev), case["edge_type"].to(dev)
        grads = [g.to(dev) for g in case["edge_grads"]]
        _check_layers(ei, et, case["num_nodes"], grads, case["h"], case["t"], k)


@pytest.mark.parametrize("k", BEAMS)
def test_kernel_matches_restatement_with_hub_rows(dev, k):
    """Rows above ULTRA_BEAM_HUB_DEGREE (one workgroup each): in-degrees of 257 to 3,000 with parallel and repeated edges."""
    g = torch.Generator().manual_seed(5)
    n = 300
    src = torch.randint(0, n, (6000,), generator=g)
    dst = torch.cat([torch.randint(0, n, (2000,), generator=g), torch.full((3000,), 7), torch.full((257,), 8),
                     torch.full((743,), 9)])
    src[100:120] = src[99]          # a run of parallel edges
    dst[100:120] = dst[99]
    ei = torch.stack([src, dst[torch.randperm(6000, generator=g)]])
    et = torch.randint(0, 5, (6000,), generator=g)
    et[100:120] = et[99]
    grads = [(torch.randint(-40, 41, (6000,), generator=g).float() / 8) for _ in range(4)]
    csr = _check_layers(ei.to(dev), et.to(dev), n, [x.to(dev) for x in grads], 3, 7, k)
    assert csr.num_hub >= 3


def test_kernel_matches_restatement_at_fb15k237_shape(dev):
    """2 triples at FB15k237's size with edge gradients computed on the GPU (ultra_3g weights, a random relation graph)."""
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=True)
    data = synthetic.to_device(kg, dev)
    model = _ultra_3g(dev)
    csr = explain.beam_csr(data.edge_index, data.edge_type, data.num_nodes)
    assert csr.num_hub > 0
    for triple in kg.target_triples[:2]:
        batch = triple.view(1, 3).to(dev)
        with torch.no_grad():
            rel = model.relation_model(data.relation_graph, query=batch[:, 2])
        model.entity_model.query = rel
        grads, _ = model.entity_model.edge_grads(data, batch)
        h, t = int(triple[0]), int(triple[1])
        for k in BEAMS:
            _check_layers(data.edge_index, data.edge_type, data.num_nodes, grads, h, t, k)


def _golden_data(vis, dev):
    rel_graph = Data(edge_index=vis["rel_edge_index"], edge_type=vis["rel_edge_type"], num_nodes=vis["num_relations"],
                     num_relations=4)
    data = Data(edge_index=vis["edge_index"], edge_type=vis["edge_type"], num_nodes=vis["num_nodes"],
                num_relations=vis["num_relations"])
    data.relation_graph = rel_graph
    return synthetic.to_device(data, dev)


def test_edge_grads_match_reference_and_unfused_route(dev):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    ent = model.entity_model
    for tr in vis["triples"]:
        batch = tr["batch"].to(dev)
        ent.query = tr["relation_representations"].to(dev)      # (the reference's relation model output)
        got, _ = ent.edge_grads(data, batch)
        # the existing unfused route (separate_grad=True alone)
        h_index, t_index, r_index = batch.unbind(-1)
        with torch.enable_grad():
            hiddens, weights, query = ent._bellmanford_hidden(data, h_index, r_index, separate_grad=True)
            feature = torch.cat([hiddens[-1][:, t_index], query.unsqueeze(1)], dim=-1).squeeze(0)
            unfused = torch.autograd.grad(ent.mlp(feature).squeeze(-1), weights)
        assert len(got) == len(tr["edge_grads"]) == 6
        # (that route gives every layer its own weights; the reference clones layer i's weights from layer i - 1's
        # (models.py:150-152), so its gradient of layer i is the sum over layers i .. 5)
        unfused = torch.stack(unfused).flip(0).cumsum(0).flip(0)
        for g, u, want in zip(got, unfused, tr["edge_grads"]):
            want = want.to(dev)
            atol = 1e-6 * float(want.abs().max())
            torch.testing.assert_close(g, want, rtol=1e-4, atol=atol)
            torch.testing.assert_close(g, u, rtol=1e-4, atol=atol)


def _assert_paths_match(paths, weights, want_paths, want_weights):
    assert len(paths) == len(want_paths)
    w, ww = torch.tensor(list(weights), dtype=torch.float64), torch.tensor(list(want_weights), dtype=torch.float64)
    torch.testing.assert_close(w, ww, rtol=1e-4, atol=1e-6 * float(ww.abs().max()))
    tol = 1e-4 * ww.abs() + 1e-6 * float(ww.abs().max())
    for i in range(len(ww)):
        separated = all(abs(float(ww[i] - ww[j])) > float(tol[i]) for j in (i - 1, i + 1) if 0 <= j < len(ww))
        if separated:
            assert list(paths[i]) == list(want_paths[i]), i


def test_ultra_visualize_returns_reference_paths(dev):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    assert (model.entity_model.num_beam, model.entity_model.path_topk) == (vis["num_beam"], vis["path_topk"])
    for tr in vis["triples"]:
        paths, weights = model.visualize(data, tr["batch"].to(dev))
        assert all(isinstance(p, list) and all(isinstance(e, tuple) and len(e) == 3 for e in p) for p in paths)
        _assert_paths_match(paths, weights, tr["paths"], tr["weights"])


def test_visualize_leaves_the_model_as_it_was(dev):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    golden = torch.load(os.path.join(HERE, "golden", "model_ultra_3g_sum.pt"))
    t_batch = golden["t_batch"].to(dev)
    with torch.no_grad():
        before = model(data, t_batch)
    params = copy.deepcopy(model.state_dict())
    model.visualize(data, vis["triples"][0]["batch"].to(dev))
    assert not model.training
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, params[k]) for k, v in model.state_dict().items())
    with torch.no_grad():
        after = model(data, t_batch)
    assert torch.equal(before, after)
    model.train()
    model.visualize(data, vis["triples"][1]["batch"].to(dev))
    assert model.training


def test_invalid_arguments_raise(dev):
    case = load()["beam"][0]
    ei, et = case["edge_index"].to(dev), case["edge_type"].to(dev)
    n = case["num_nodes"]
    csr = explain.beam_csr(ei, et, n)
    g = case["edge_grads"][0].to(dev)
    d = torch.full((n, 4), float("-inf"), device=dev)
    for k in (0, 65, 100):
        with pytest.raises(ValueError):
            explain.beam_search_layer(csr, g, torch.full((n, k), float("-inf"), device=dev), case["t"], k)
    with pytest.raises(TypeError):
        explain.beam_search_layer(csr, g.double(), d, case["t"], 4)
    with pytest.raises(TypeError):
        explain.beam_search_layer(csr, g, d.half(), case["t"], 4)
    with pytest.raises(ValueError):
        explain.beam_search_layer(csr, g[:-1], d, case["t"], 4)
    with pytest.raises(ValueError):
        explain.beam_search_layer(csr, g, d[:-1], case["t"], 4)
    with pytest.raises(ValueError):
        explain.beam_search_layer(csr, g, d, n, 4)
    # the C entry point itself: num_beam outside [1, 64] is ULTRA_ERR_UNSUPPORTED, a NULL operand ULTRA_ERR_INVALID
    out_d, out_b = torch.empty_like(d), torch.empty(n, 4, 4, dtype=torch.int64, device=dev)
    rc = _lib.lib.ultra_beam_search_layer(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), csr.eid.data_ptr(),
                                          None, 0, n, csr.num_edge, g.data_ptr(), d.data_ptr(), case["t"], 65, out_d.data_ptr(),
                                          out_b.data_ptr(), None)
    assert rc == _lib.ULTRA_ERR_UNSUPPORTED and b"num_beam" in _lib.lib.ultra_last_error()
    rc = _lib.lib.ultra_beam_search_layer(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), csr.eid.data_ptr(),
                                          None, 0, n, csr.num_edge, g.data_ptr(), None, case["t"], 4, out_d.data_ptr(),
                                          out_b.data_ptr(), None)
    assert rc == _lib.ULTRA_ERR_INVALID
    with pytest.raises(AssertionError):
        _ultra_3g(dev).visualize(_golden_data(load()["visualize"], dev), torch.zeros(2, 3, dtype=torch.long, device=dev))
