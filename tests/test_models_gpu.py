"""Model-level parity on the GPU: Ultra.forward through the HIP engine vs (a) golden scores recorded
from the reference and (b) the CPU oracle model on a larger seeded graph.  Tolerance: fp32 scores
within 1e-4 (BASELINE north_star), rankings / metrics identical."""
import copy
import os

import pytest
import torch

from oracle import ultra_oracle_model
from tests.test_oracle_model import MODELS, load_golden
from ultra_amd import models, synthetic, tasks

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def build(state, cfg, dev):
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    return model.to(dev).eval()


@pytest.mark.parametrize("ckpt,aggr", MODELS)
def test_scores_match_reference_golden(dev, ckpt, aggr):
    g, state, data, cfg = load_golden(ckpt, aggr)
    model = build(state, cfg, dev)
    gdata = data.to(dev)
    batch = g["batch"].to(dev)
    pos_h, pos_t, _ = batch.t()
    with torch.no_grad():
        t_pred = model(gdata, g["t_batch"].to(dev))
        h_pred = model(gdata, g["h_batch"].to(dev))
        neg_pred = model(gdata, g["neg_batch"].to(dev))
        t_mask, h_mask = tasks.strict_negative_mask(gdata, batch)
        t_rank = tasks.compute_ranking(t_pred, pos_t, t_mask)
        h_rank = tasks.compute_ranking(h_pred, pos_h, h_mask)
    for got, want in ((t_pred, g["t_pred"]), (h_pred, g["h_pred"]), (neg_pred, g["neg_pred"])):
        err = (got.cpu() - want).abs().max().item()
        assert err <= TOL, "max |gpu - reference| = %g" % err
    assert torch.equal(t_rank.cpu(), g["t_rank"]) and torch.equal(h_rank.cpu(), g["h_rank"])


@pytest.mark.parametrize("ckpt,aggr", MODELS)
def test_scores_and_rankings_match_oracle_on_larger_graph(dev, ckpt, aggr):
    _, state, _, cfg = load_golden(ckpt, aggr)
    data = synthetic.make_kg(num_node=3000, num_triple=24000, num_relation_base=20, num_test=64, seed=11)
    batch = data.target_triples[:8]
    t_batch, h_batch = tasks.all_negative(data, batch)
    fn = ultra_oracle_model.reference_rspmm_fn()
    want_t = ultra_oracle_model.ultra_forward(state, cfg, data, t_batch, rspmm_fn=fn)
    want_h = ultra_oracle_model.ultra_forward(state, cfg, data, h_batch, rspmm_fn=fn)
    model = build(state, cfg, dev)
    gdata = data.to(dev)
    with torch.no_grad():
        got_t = model(gdata, t_batch.to(dev)).cpu()
        got_h = model(gdata, h_batch.to(dev)).cpu()
    assert (got_t - want_t).abs().max().item() <= TOL
    assert (got_h - want_h).abs().max().item() <= TOL
    t_mask, h_mask = tasks.strict_negative_mask(data, batch)
    pos_h, pos_t, _ = batch.t()
    for got, want, pos, mask in ((got_t, want_t, pos_t, t_mask), (got_h, want_h, pos_h, h_mask)):
        r_got = tasks.compute_ranking(got, pos, mask)
        r_want = tasks.compute_ranking(want, pos, mask)
        assert torch.equal(r_got, r_want), "rank mismatches: %d" % (r_got != r_want).sum().item()


def test_mean_and_transe_paths_run_and_match_oracle(dev):
    _, state, _, _ = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=400, num_triple=3000, num_relation_base=5, num_test=16, seed=2)
    batch = data.target_triples[:3]
    t_batch, _ = tasks.all_negative(data, batch)
    for aggr, msg in (("mean", "distmult"), ("sum", "transe"), ("max", "transe")):
        cfg = synthetic.default_model_cfg(aggregate_func=aggr, message_func=msg)
        want = ultra_oracle_model.ultra_forward(state, cfg, data, t_batch)
        model = build(state, cfg, dev)
        with torch.no_grad():
            got = model(data.to(dev), t_batch.to(dev)).cpu()
        assert (got - want).abs().max().item() <= TOL, (aggr, msg)


def test_training_step_gradients_match_cpu_autograd(dev):
    """fwd + bwd through the HIP autograd path vs torch autograd over the oracle model with a
    differentiable index_add restatement of rspmm (CPU, fp32)."""
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=300, num_triple=2400, num_relation_base=5, num_test=16, seed=4)
    batch = data.target_triples[:4]
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 8, strict=True)
    if os.environ.get("ULTRA_GRAD_PARITY_SHAPE"):
        # one-off long run (profiles/r6_experiments.txt): a BASELINE-sized graph, one query with 256 strict negatives -- ~ 5 GB of
        # saved fp64 messages on the CPU side
        data = synthetic.make_kg(**synthetic.SHAPES[os.environ["ULTRA_GRAD_PARITY_SHAPE"]], seed=1234)
        neg = tasks.negative_sampling(data, data.target_triples[:1], 256, strict=True)

    def torch_rspmm(edge_index, edge_type, edge_weight, relation, input, sum="add", mul="mul"):
        msg = relation[edge_type] * input[edge_index[1]] if mul == "mul" else relation[edge_type] + input[edge_index[1]]
        return torch.zeros_like(input).index_add(0, edge_index[0], msg * edge_weight.unsqueeze(-1))

    def cpu_grads(dtype):
        sd = {k: v.clone().to(dtype).requires_grad_() for k, v in state.items()}
        with torch.enable_grad():
            rel = ultra_oracle_model.rel_nbfnet(sd, data.relation_graph, neg[:, 0, 2], cfg["rel_model_cfg"], torch_rspmm)
            out = ultra_oracle_model.entity_nbfnet(sd, data, rel, neg, cfg["entity_model_cfg"], torch_rspmm)
            target = torch.zeros_like(out)
            target[:, 0] = 1
            loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
            loss.backward()
        return loss.item(), {k: v.grad.double() for k, v in sd.items()}, target.float()

    loss32, g32, target = cpu_grads(torch.float32)      # the reference's arithmetic
    loss64, g64, _ = cpu_grads(torch.float64)           # what both fp32 runs approximate

    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).eval()     # eval: keep the edge set fixed (remove_easy_edges is training-only)
    got = model(data.to(dev), neg.to(dev))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(got, target.to(dev))
    loss.backward()
    assert abs(loss.item() - loss32) <= 1e-5
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        scale = max(g64[name].abs().max().item(), 1e-6)
        err_gpu = (p.grad.cpu().double() - g64[name]).abs().max().item()
        err_cpu = (g32[name] - g64[name]).abs().max().item()
        # fp32 backprop through 12 layers: the GPU may not be further from the fp64 gradient than a few
        # times the reference's own fp32 path
        assert err_gpu <= 4 * err_cpu + 1e-4 * scale + 1e-7, \
            "%s: |gpu - fp64| = %g, |cpu fp32 - fp64| = %g (scale %g)" % (name, err_gpu, err_cpu, scale)



def reference_easy_edge_keep(edge_index, edge_type, h_index, t_index, r_index, num_relations, remove_one_hop=False):
    """base_nbfnet.py:54-77 as a plain loop: an edge is dropped when it is some (h, t, r) of the batch -- negatives included --
    or its inverse (t, h, r + R/2); with remove_one_hop when it joins such a pair under any type."""
    half = num_relations // 2
    easy = set()
    for h, t, r in zip(h_index.flatten().tolist(), t_index.flatten().tolist(), r_index.flatten().tolist()):
        easy.add((h, t) if remove_one_hop else (h, t, r))
        easy.add((t, h) if remove_one_hop else (t, h, r + half))
    keep = []
    for a, b, r in zip(edge_index[0].tolist(), edge_index[1].tolist(), edge_type.tolist()):
        keep.append(((a, b) if remove_one_hop else (a, b, r)) not in easy)
    return torch.tensor(keep, dtype=torch.bool)


def test_easy_edge_loop_matches_reference_golden():
    """The loop above keeps exactly the edges the reference's remove_easy_edges kept (tests/golden/easy_edges.pt)."""
    from tests.test_tasks import easy_edges_golden
    data, cases = easy_edges_golden()
    for case in cases:
        h, t, r = case["batch"].unbind(-1)
        keep = reference_easy_edge_keep(data.edge_index, data.edge_type, h, t, r, data.num_relations, case["remove_one_hop"])
        assert torch.equal(keep, case["keep"])


class OracleRSPMM(torch.autograd.Function):
    """rspmm_oracle.rspmm_forward / rspmm_backward as an autograd node: the reference's min / max tie rule (every tying edge
    gets the full gradient), which neither an index_add restatement nor scatter_reduce (it splits ties) has."""

    @staticmethod
    def forward(ctx, edge_index, edge_type, edge_weight, relation, input, sum, mul):
        from oracle import rspmm_oracle
        ei, et, ew, _ = rspmm_oracle.sort_edges(edge_index, edge_type, edge_weight)
        out = rspmm_oracle.rspmm_forward(ei, et, ew, relation, input, sum=sum, mul=mul)
        ctx.save_for_backward(ei, et, ew, relation, input, out)
        ctx.sum, ctx.mul = sum, mul
        return out

    @staticmethod
    def backward(ctx, output_grad):
        from oracle import rspmm_oracle
        ei, et, ew, relation, input, out = ctx.saved_tensors
        _, rel_grad, x_grad = rspmm_oracle.rspmm_backward(ei, et, ew, relation, input, out, output_grad.contiguous(),
                                                          sum=ctx.sum, mul=ctx.mul)
        return None, None, None, rel_grad, x_grad, None, None


def oracle_rspmm(edge_index, edge_type, edge_weight, relation, input, sum="add", mul="mul"):
    return OracleRSPMM.apply(edge_index, edge_type, edge_weight, relation, input, sum, mul)


TRAIN_ROUTES = [("ultra_3g", "sum", "rows"), ("ultra_3g", "sum", "whole_graph"), ("ultra_3g", "sum", "old_routes"),
                ("ultra_50g", "max", "default"), ("ultra_3g", "mean", "default")]


@pytest.mark.parametrize("ckpt,aggr,route", TRAIN_ROUTES)
def test_train_mode_step_gradients_match_cpu_oracle(dev, monkeypatch, ckpt, aggr, route):
    """The training step as train() runs it: model.train() (the batch's own edges are dropped by the keep-mask kernels), the
    self-adversarial loss at temperature 0.5 (train.ranking_loss, script/run.py:66-77), .backward().  Against torch autograd
    over the CPU oracle model on the graph the reference's remove_easy_edges leaves, its rspmm an autograd node over the C
    oracle (the reference's tie rule), in fp32 and fp64: the GPU may not be further from fp64 than a few times the CPU fp32
    path.  sum / mean: max-abs per parameter; max: Frobenius norm per parameter, near-ties may fall either way between two
    fp32 paths."""
    from ultra_amd import dense, layers, rspmm, train
    _, state, _, cfg = load_golden(ckpt, "sum" if aggr == "mean" else aggr)
    if aggr == "mean":
        cfg = {k: dict(v) for k, v in cfg.items()}
        cfg["entity_model_cfg"]["aggregate_func"] = "mean"
    if route in ("rows", "whole_graph"):
        monkeypatch.setattr(layers, "LAST_LAYER_ON_ROWS", route == "rows")
    if route == "old_routes":      # (monkeypatch restores every switch afterwards)
        for mod, name in ((models, "EASY_EDGE_KEEP_KERNEL"), (dense, "READOUT_TRAIN_NODE"), (models, "RELATION_PROJECTION_NODE"),
                          (dense, "ROWS_BACKWARD_GATHER"), (rspmm, "DENSE_RELATION_GRAD"), (train, "FUSED_LOSS")):
            assert hasattr(mod, name)
            monkeypatch.setattr(mod, name, False)
    _train_step_against_the_cpu_oracle(dev, state, cfg, aggr)


FUSED_TRAINING_NODES = ("ConvUpdateFunction", "TrainLayerFunction", "TrainRowsLayerFunction", "ReadoutTrainFunction",
                        "RelationProjectionFunction")


def _autograd_node_names(root):
    """The class names of every autograd node reachable from `root` (a grad_fn)."""
    names, seen, stack = set(), set(), [root]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return names


def train_step_inputs():
    """(data, the graph the reference's remove_easy_edges leaves, batch with its negatives) of the train-mode step tests."""
    data = synthetic.make_kg(num_node=300, num_triple=2400, num_relation_base=5, num_test=16, seed=4)
    # the batch: graph edges, so that the training forward has easy edges to drop
    pick = torch.tensor([0, 7, 900, 1900])
    batch = torch.stack([data.edge_index[0, pick], data.edge_index[1, pick], data.edge_type[pick]], dim=-1)
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 8, strict=True)
    h, t, r = neg.unbind(-1)
    keep = reference_easy_edge_keep(data.edge_index, data.edge_type, h, t, r, data.num_relations)
    assert 0 < int((~keep).sum()) < 100
    filtered = copy.copy(data)
    filtered.edge_index, filtered.edge_type = data.edge_index[:, keep], data.edge_type[keep]
    return data, filtered, neg


def cpu_train_step(state, cfg, data, filtered, neg, dtype):
    """The step on the CPU oracle model in `dtype`: (loss, scores, fp64 copies of the parameter gradients)."""
    from oracle import ultra_oracle_model as om
    from tests.test_train_gpu import reference_loss
    sd = {k: v.clone().to(dtype).requires_grad_() for k, v in state.items()}
    with torch.enable_grad():
        rel = om.rel_nbfnet(sd, data.relation_graph, neg[:, 0, 2], cfg["rel_model_cfg"], oracle_rspmm)
        pred = om.entity_nbfnet(sd, filtered, rel, neg, cfg["entity_model_cfg"], oracle_rspmm)
        loss = reference_loss(pred, 0.5, neg.shape[1] - 1)
        loss.backward()
    return loss.item(), pred.detach(), {k: v.grad.double() for k, v in sd.items()}


# (hidden size, layers, aggregate, message, layer_norm, short_cut) of the training steps at widths other than 64
OTHER_HIDDEN_SIZES = [(32, 3, "sum", "distmult", True, True), (128, 2, "max", "distmult", True, False),
                      (48, 2, "sum", "transe", False, False)]


def random_model(dim, layers_n, aggr, message, layer_norm, short_cut):
    """(state dict, cfg) of an Ultra with random weights under a fixed seed, as
    test_shapes_outside_the_fused_kernels_match_the_oracle builds its models."""
    torch.manual_seed(dim + layers_n)
    def one(cls):
        return {"class": cls, "input_dim": dim, "hidden_dims": [dim] * layers_n, "message_func": message,
                "aggregate_func": aggr, "short_cut": short_cut, "layer_norm": layer_norm}
    cfg = {"rel_model_cfg": one("RelNBFNet"), "entity_model_cfg": one("EntityNBFNet")}
    model = models.Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(cfg["entity_model_cfg"]))
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, cfg


def _train_step_against_the_cpu_oracle(dev, state, cfg, aggr, generic_routes_only=False):
    """One training step of Ultra(**cfg) with the weights `state` against the CPU oracle model in fp32 and fp64 (see
    test_train_mode_step_gradients_match_cpu_oracle).  generic_routes_only: no fused 64-wide training node may be in the
    graph, and the score and loss checks are relative to the scores' size -- see where score_scale is set."""
    from ultra_amd import dense, train
    data, filtered, neg = train_step_inputs()
    num_negative = neg.shape[1] - 1
    loss32, pred32, g32 = cpu_train_step(state, cfg, data, filtered, neg, torch.float32)
    loss64, _, g64 = cpu_train_step(state, cfg, data, filtered, neg, torch.float64)

    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).train()
    gdata = data.to(dev)
    pred = model(gdata, neg.to(dev))
    loss = train.ranking_loss(pred, 0.5, num_negative)
    if generic_routes_only:
        assert all(hasattr(dense, name) for name in FUSED_TRAINING_NODES)
        nodes = _autograd_node_names(loss.grad_fn)
        assert any(n.startswith("_PlanRSPMM") for n in nodes), sorted(nodes)        # (the walk does see custom nodes)
        fused = sorted(n for n in nodes if any(n.startswith(f) for f in FUSED_TRAINING_NODES))
        assert not fused, "a fused 64-wide training node in a model of another width: %s" % fused
    loss.backward()
    # the masked route really ran: the scores are the filtered graph's, not the full graph's
    with torch.no_grad():
        model.eval()
        full = model(gdata, neg.to(dev)).cpu()
        model.train()
    # The checkpoints' scores are O(1) and are held to the absolute TOL and 1e-5.  The random-weight models are held to the
    # same figures times max(1, max |score|): that is 1.0 at hidden 32 and 128 (max |score| 0.64 and 0.083), so nothing
    # changes there, and 54 at hidden 48 / TransE / no LayerNorm (max |score| 53.95), where the CPU oracle's own fp32
    # scores are 4.2e-4 and its fp32 loss 2.1e-5 from its fp64 ones -- no fp32 path meets the absolute figures there.
    # tests/test_backward_bounds_cpu.py pins these scales and that the CPU fp32 path meets the scaled figures.
    score_scale = max(1.0, pred32.abs().max().item()) if generic_routes_only else 1.0
    assert (pred.detach().cpu() - pred32).abs().max().item() <= TOL * score_scale
    assert (full - pred32).abs().max().item() > 10 * TOL * score_scale, "dropping the easy edges did not change the scores"
    assert abs(loss.item() - loss32) <= 1e-5 * score_scale, (loss.item(), loss32)      # (the loss is 1-Lipschitz in the scores)
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        got, want, cpu = p.grad.cpu().double(), g64[name], g32[name]
        if aggr == "max":
            scale = max(want.norm().item(), 1e-6)
            err_gpu, err_cpu = (got - want).norm().item(), (cpu - want).norm().item()
        else:
            scale = max(want.abs().max().item(), 1e-6)
            err_gpu, err_cpu = (got - want).abs().max().item(), (cpu - want).abs().max().item()
        assert err_gpu <= 4 * err_cpu + 1e-4 * scale + 1e-7, \
            "%s: |gpu - fp64| = %g, |cpu fp32 - fp64| = %g (scale %g)" % (name, err_gpu, err_cpu, scale)


@pytest.mark.parametrize("dim,layers_n,aggr,message,layer_norm,short_cut", OTHER_HIDDEN_SIZES)
def test_train_mode_step_at_other_hidden_sizes_matches_cpu_oracle(dev, dim, layers_n, aggr, message, layer_norm, short_cut):
    """test_train_mode_step_gradients_match_cpu_oracle for models built as test_shapes_outside_the_fused_kernels_match_the_oracle
    builds them (random weights under a fixed seed): at hidden sizes other than 64 the training step falls through the
    fused conv-update, whole-layer, listed-rows, readout and relation-projection nodes to the generic rspmm backward --
    the same data, batch, negatives, easy-edge filtering and acceptance rule for the gradients."""
    state, cfg = random_model(dim, layers_n, aggr, message, layer_norm, short_cut)
    _train_step_against_the_cpu_oracle(dev, state, cfg, aggr, generic_routes_only=True)


def test_training_mode_removes_easy_edges(dev):
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=200, num_triple=1500, num_relation_base=4, num_test=16, seed=6)
    # use graph edges as the batch so that remove_easy_edges has something to remove
    batch = torch.stack([data.edge_index[0, :4], data.edge_index[1, :4], data.edge_type[:4]], dim=-1)
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 4, strict=True)
    model = build(state, cfg, dev).train()
    out_train = model(data.to(dev), neg.to(dev))
    model.eval()
    with torch.no_grad():
        out_eval = model(data.to(dev), neg.to(dev))
    assert out_train.shape == out_eval.shape == (4, 5)
    assert not torch.allclose(out_train.detach(), out_eval)      # the direct edges were dropped in training mode
    # ... exactly the edges the reference drops: the training scores are the eval scores of the filtered graph
    h, t, r = neg.unbind(-1)
    keep = reference_easy_edge_keep(data.edge_index, data.edge_type, h, t, r, data.num_relations)
    assert int((~keep).sum()) > 0
    filtered = copy.copy(data)
    filtered.edge_index, filtered.edge_type = data.edge_index[:, keep], data.edge_type[keep]
    with torch.no_grad():
        out_filtered = model(filtered.to(dev), neg.to(dev))
    assert (out_train.detach() - out_filtered).abs().max().item() <= 1e-5


def test_graph_capture_replays_the_same_scores(dev):
    """hipGraph capture of the inference forward (ultra_amd/graph.py): replay == eager, for new batches too."""
    from ultra_amd.graph import GraphedForward
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=500, num_triple=4000, num_relation_base=6, num_test=64, seed=8).to(dev)
    model = build(state, cfg, dev)
    batches = [tasks.all_negative(data, data.target_triples[i * 4:(i + 1) * 4])[0] for i in range(3)]
    graphed = GraphedForward(model, data, batches[0])
    for b in batches:
        with torch.no_grad():
            want = model(data, b).clone()
        got = graphed(b, check=True).clone()
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        graphed(batches[0][:2])
    # the deferred input check still fires: rows must share head and relation
    bad = batches[0].clone()
    bad[0, 5, 0] += 1
    with pytest.raises(AssertionError):
        with torch.no_grad():
            model(data, bad)
    with pytest.raises(AssertionError):
        graphed(bad, check=True)


def test_query_nbfnet_matches_reference_golden(dev):
    """QueryNBFNet (UltraQuery's entity reasoner, models.py:212-275) on the same kernels."""
    import os
    from tests.test_oracle_model import GOLDEN
    from ultra_amd.data import Data
    g = torch.load(os.path.join(GOLDEN, "query_nbfnet_ultra_3g.pt"))
    state = torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt"))
    cfg = synthetic.default_model_cfg()
    qnet = models.QueryNBFNet(**{k: v for k, v in cfg["entity_model_cfg"].items() if k != "class"})
    rnet = models.RelNBFNet(**{k: v for k, v in cfg["rel_model_cfg"].items() if k != "class"})
    qnet.load_state_dict({k[len("entity_model."):]: v for k, v in state.items() if k.startswith("entity_model.")})
    rnet.load_state_dict({k[len("relation_model."):]: v for k, v in state.items() if k.startswith("relation_model.")})
    qnet, rnet = qnet.to(dev).eval(), rnet.to(dev).eval()
    data = Data(edge_index=g["edge_index"], edge_type=g["edge_type"], num_nodes=g["num_nodes"],
                num_relations=g["num_relations"],
                relation_graph=Data(edge_index=g["rel_edge_index"], edge_type=g["rel_edge_type"],
                                    num_nodes=g["num_relations"], num_relations=4)).to(dev)
    with torch.no_grad():
        rel_repr = rnet(data.relation_graph, query=g["query_rels"].to(dev))
        assert (rel_repr.cpu() - g["rel_repr"]).abs().max().item() <= TOL
        query = rel_repr[torch.arange(3, device=dev), g["query_rels"].to(dev)]
        score = qnet(data, g["node_features"].to(dev), rel_repr, query)
    assert score.shape == g["score"].shape
    assert (score.cpu() - g["score"]).abs().max().item() <= TOL


def test_training_edge_dropout_by_weight_equals_edge_removal(dev):
    """sum aggregation: masking the batch's edges with 0/1 weights on the cached plan == rebuilding the graph
    without them (base_nbfnet.py:54-77), forward and gradients."""
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=200, num_triple=1500, num_relation_base=4, num_test=16, seed=6).to(dev)
    batch = torch.stack([data.edge_index[0, :4], data.edge_index[1, :4], data.edge_type[:4]], dim=-1)
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 4, strict=True)
    model = build(state, cfg, dev).train()
    ent = model.entity_model
    out_masked = model(data, neg)
    out_masked.sum().backward()
    g_masked = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()
    h, t, r = neg.unbind(-1)
    removed = ent.remove_easy_edges(data, h, t, r)
    assert removed.num_edges < data.num_edges
    ent.eval()                       # eval mode on the edge-removed graph = the reference's training forward
    out_removed = model(removed, neg)
    out_removed.sum().backward()
    ent.train()
    assert (out_masked - out_removed).abs().max().item() <= 1e-5
    for n, p in model.named_parameters():
        scale = max(p.grad.abs().max().item(), 1e-6)
        assert (p.grad - g_masked[n]).abs().max().item() <= 1e-4 * scale + 1e-7, n


@pytest.mark.parametrize("ckpt", ["ultra_3g"])
def test_onehot_layer0_path_matches_dense_path(dev, ckpt):
    """Layer 0 through the row-sparse forward == layer 0 through the dense forward (scores to fp32 round-off)."""
    from ultra_amd import layers
    _, state, _, cfg = load_golden(ckpt, "sum")
    data = synthetic.make_kg(num_node=1500, num_triple=20000, num_relation_base=6, num_test=16, seed=14).to(dev)
    model = build(state, cfg, dev)
    t_batch, h_batch = tasks.all_negative(data, data.target_triples[:6])
    try:
        with torch.no_grad():
            layers.POINT_BOUNDARY_FAST_PATH = False      # materialised boundary: the row-sparse rspmm serves layer 0
            layers.ONEHOT_FAST_PATH = True
            a_t, a_h = model(data, t_batch).clone(), model(data, h_batch).clone()
            layers.ONEHOT_FAST_PATH = False
            b_t, b_h = model(data, t_batch).clone(), model(data, h_batch).clone()
    finally:
        layers.ONEHOT_FAST_PATH = True
        layers.POINT_BOUNDARY_FAST_PATH = True
    assert (a_t - b_t).abs().max().item() <= 2e-5 and (a_h - b_h).abs().max().item() <= 2e-5


@pytest.mark.parametrize("ckpt,aggr", [("ultra_3g", "sum"), ("ultra_50g", "max")])
def test_closed_form_boundary_path_matches_materialised_boundary(dev, ckpt, aggr):
    """PointBoundary (layer 0 on its special rows, boundary added to one row per sample) == the (batch, N, d) tensor path.
    With the max aggregate the closed form does not apply (max(agg, 0) touches every row): both settings then take the
    tensor path and must agree exactly."""
    from ultra_amd import layers
    _, state, _, cfg = load_golden(ckpt, aggr)
    data = synthetic.make_kg(num_node=1500, num_triple=20000, num_relation_base=6, num_test=16, seed=15).to(dev)
    model = build(state, cfg, dev)
    t_batch, h_batch = tasks.all_negative(data, data.target_triples[:6])
    try:
        with torch.no_grad():
            layers.POINT_BOUNDARY_FAST_PATH = True
            a_t, a_h = model(data, t_batch).clone(), model(data, h_batch).clone()
            layers.POINT_BOUNDARY_FAST_PATH = False
            layers.ONEHOT_FAST_PATH = False
            b_t, b_h = model(data, t_batch).clone(), model(data, h_batch).clone()
    finally:
        layers.ONEHOT_FAST_PATH = True
        layers.POINT_BOUNDARY_FAST_PATH = True
    tol = 2e-5 if aggr == "sum" else 2e-5
    assert (a_t - b_t).abs().max().item() <= tol and (a_h - b_h).abs().max().item() <= tol


@pytest.mark.parametrize("bs", [1, 2, 5])
def test_every_combination_of_fast_path_switches_scores_the_same(dev, bs):
    """The four inference fast paths are independent: all 16 on/off combinations give the same scores as the generic
    path.  (Regression: with the prologue and the closed-form boundary both off, the strided head / relation index
    views reached a kernel through contiguous temporaries that were freed inside the argument list.)"""
    import itertools
    from ultra_amd import layers, models
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=1500, num_triple=20000, num_relation_base=6, num_test=16, seed=16).to(dev)
    model = build(state, cfg, dev)
    t_batch, h_batch = tasks.all_negative(data, data.target_triples[3:3 + bs])
    outs = {}
    try:
        for combo in itertools.product([True, False], repeat=4):
            layers.ONEHOT_FAST_PATH, layers.POINT_BOUNDARY_FAST_PATH, layers.FUSED_DENSE_LAYER, models.PROLOGUE_FAST_PATH = combo
            with torch.no_grad():
                outs[combo] = torch.cat([model(data, t_batch), model(data, h_batch)]).clone()
    finally:
        layers.ONEHOT_FAST_PATH = layers.POINT_BOUNDARY_FAST_PATH = layers.FUSED_DENSE_LAYER = True
        models.PROLOGUE_FAST_PATH = True
    base = outs[(False, False, False, False)]
    for combo, out in outs.items():
        err = (out - base).abs().max().item()
        assert err <= 3e-5, "switches %s: max |d| = %g" % (combo, err)


@pytest.mark.parametrize("dim,layers_n,layer_norm,short_cut,message", [(32, 3, True, True, "distmult"), (64, 2, False, False, "distmult"),
                                                                     (48, 2, True, False, "transe"), (128, 2, True, True, "distmult")])
def test_shapes_outside_the_fused_kernels_match_the_oracle(dev, dim, layers_n, layer_norm, short_cut, message):
    """Hidden sizes other than the checkpoints' 64 (and LayerNorm / short-cut variants) take the generic rspmm kernels with
    the torch update / readout chain; randomly initialised weights, scores against the CPU oracle model."""
    torch.manual_seed(dim + layers_n)
    def one(cls):
        return {"class": cls, "input_dim": dim, "hidden_dims": [dim] * layers_n, "message_func": message,
                "aggregate_func": "sum", "short_cut": short_cut, "layer_norm": layer_norm}
    cfg = {"rel_model_cfg": one("RelNBFNet"), "entity_model_cfg": one("EntityNBFNet")}
    model = models.Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(cfg["entity_model_cfg"])).eval()
    data_cpu = synthetic.make_kg(num_node=400, num_triple=5000, num_relation_base=5, num_test=8, seed=dim)
    t_batch, h_batch = tasks.all_negative(data_cpu, data_cpu.target_triples[:3])
    want_t = ultra_oracle_model.ultra_forward(model.state_dict(), cfg, data_cpu, t_batch)
    want_h = ultra_oracle_model.ultra_forward(model.state_dict(), cfg, data_cpu, h_batch)
    data = data_cpu.to(dev)
    model = model.to(dev)
    with torch.no_grad():
        got_t = model(data, t_batch.to(dev)).cpu()
        got_h = model(data, h_batch.to(dev)).cpu()
    scale = max(1.0, want_t.abs().max().item(), want_h.abs().max().item())
    assert (got_t - want_t).abs().max().item() <= 1e-4 * scale
    assert (got_h - want_h).abs().max().item() <= 1e-4 * scale


def test_mixed_tail_and_head_rows_in_one_batch(dev):
    """base_nbfnet.py:79-86 converts head-prediction rows per ROW: one batch may hold both kinds (training batches do).
    Scores of a mixed batch == scores of the same rows scored in pure batches, on the fast and on the generic path."""
    from ultra_amd import layers
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=900, num_triple=9000, num_relation_base=5, num_test=16, seed=21).to(dev)
    model = build(state, cfg, dev)
    t_batch, h_batch = tasks.all_negative(data, data.target_triples[:6])
    mixed = torch.cat([t_batch[:2], h_batch[2:4], t_batch[4:5], h_batch[5:6]])
    with torch.no_grad():
        want = torch.cat([model(data, t_batch)[:2], model(data, h_batch)[2:4], model(data, t_batch)[4:5], model(data, h_batch)[5:6]])
        got = model(data, mixed)
        try:
            models.PROLOGUE_FAST_PATH = False
            layers.POINT_BOUNDARY_FAST_PATH = False
            generic = model(data, mixed)
        finally:
            models.PROLOGUE_FAST_PATH = True
            layers.POINT_BOUNDARY_FAST_PATH = True
    assert (got - want).abs().max().item() <= 2e-5
    assert (generic - want).abs().max().item() <= 2e-5


def test_sparse_relation_graph_takes_the_edge_walk(dev):
    """Many relations, few triples: the relation graph is far from complete, gets no dense-format plan and runs through the
    edge-walk kernels (point boundary, layer-0 kernels); scores against the CPU oracle model."""
    from ultra_amd import rspmm
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data_cpu = synthetic.make_kg(num_node=500, num_triple=1500, num_relation_base=150, num_test=8, seed=23)
    rg = data_cpu.relation_graph
    fill = rg.num_edges / float(rg.num_nodes ** 2 * 4)
    assert fill < 0.25, fill
    t_batch, h_batch = tasks.all_negative(data_cpu, data_cpu.target_triples[:4])
    want_t = ultra_oracle_model.ultra_forward(state, cfg, data_cpu, t_batch)
    want_h = ultra_oracle_model.ultra_forward(state, cfg, data_cpu, h_batch)
    data = data_cpu.to(dev)
    model = build(state, cfg, dev)
    with torch.no_grad():
        got_t, got_h = model(data, t_batch.to(dev)).cpu(), model(data, h_batch.to(dev)).cpu()
    assert rspmm.get_plan(data.relation_graph.edge_index, data.relation_graph.edge_type, rg.num_nodes, 4).dense is None
    assert (got_t - want_t).abs().max().item() <= 1e-4 and (got_h - want_h).abs().max().item() <= 1e-4


@pytest.mark.parametrize("threshold,key", [(0.0, "t_prob"), (0.3, "t_prob_thr03")])
def test_relation_projection_matches_reference_golden(dev, threshold, key):
    """RelationProjection (ultraquery.py:245-277) against the output of the reference class itself (executed from the
    reference file by tests/golden/gen_golden.py around the reference's Ultra(RelNBFNet, QueryNBFNet))."""
    import os

    from ultra_amd.data import Data
    from ultra_amd.ultraquery import RelationProjection
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "relation_projection_ultra_3g.pt"))
    state = torch.load(os.path.join(os.path.dirname(__file__), "golden", "ultra_3g_model.pt"))
    rel_graph = Data(edge_index=g["rel_edge_index"], edge_type=g["rel_edge_type"], num_nodes=g["num_relations"],
                     num_relations=4)
    data = Data(edge_index=g["edge_index"], edge_type=g["edge_type"], num_nodes=g["num_nodes"],
                num_relations=g["num_relations"], relation_graph=rel_graph).to(dev)
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    proj = RelationProjection(model.to(dev).eval(), threshold=threshold)
    with torch.no_grad():
        got = proj(data, g["h_prob"].to(dev), g["r_index"].to(dev)).cpu()
    assert got.shape == g[key].shape
    assert (got - g[key]).abs().max().item() <= 1e-5, (got - g[key]).abs().max().item()


@pytest.mark.parametrize("share_chip", ["auto", True, False])
def test_two_batches_in_flight_score_like_one_at_a_time(dev, share_chip):
    """graph.PipelinedForward: captured forwards replayed round-robin on two streams (own buffers each) return, batch for
    batch, the bits of the one-at-a-time forward -- with whole-chip aggregation launches and with the shared-chip ones (three
    quarters of the CUs as workgroups: the schedule for fewer partitions moves rows between workgroups, not inside their sums)."""
    from ultra_amd import graph as ugraph, models, rspmm, synthetic, tasks
    data = synthetic.make_kg(num_node=900, num_triple=6000, num_relation_base=11, seed=5).to(dev)
    torch.manual_seed(3)
    model = models.Ultra(**synthetic.default_model_cfg()).to(dev).eval()
    bs = 4
    batches = [tasks.all_negative(data, data.target_triples[i * bs:(i + 1) * bs])[0] for i in range(6)]
    with torch.no_grad():
        want = [model(data, b).clone() for b in batches]
    piped = ugraph.PipelinedForward(model, data, batches[0], depth=2, share_chip=share_chip)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert piped.launch_grid == (0 if share_chip is False else ugraph.shared_launch_grid(dev))      # (a small graph: "auto" shares)
    assert 0 < ugraph.shared_launch_grid(dev) < cus
    t = rspmm.get_tuning()
    assert t["grid"] == 0, "the launch size of the captures must not leak into the process's tuning"
    for rep in range(3):
        got = []
        for i, b in enumerate(batches):
            out = piped(b)
            if i >= 1:          # the previous slot's output: still in place (the slot is reused two calls later)
                piped.join()
                got.append((i - 1, prev.clone()))
            prev = out
        piped.join()
        got.append((len(batches) - 1, prev.clone()))
        for i, g in got:
            assert torch.equal(g, want[i]), "batch %d, repetition %d" % (i, rep)
    # back to back without joining in between: only the last two are still readable
    for b in batches:
        out = piped(b)
    piped.join()
    assert torch.equal(out, want[-1])
