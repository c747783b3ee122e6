"""Multi-graph pre-training on the GPU: the easy-edge filter for batches of any size (ultra_easy_edge_keep_table), the batch-64
x 513 step against the fp64 oracle, captured steps over three graphs against the same eager steps, the loop of
ultra_amd.pretrain, and two ranks that start from different seeds."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from tests.test_launch_gpu import ROOT, _env, _free_port
from tests.test_models_gpu import TOL, oracle_rspmm, reference_easy_edge_keep
from tests.test_oracle_model import load_golden
from ultra_amd import _lib, dense, models, pretrain, synthetic, tasks, train

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(data, rows, cols, seed):
    """(rows, cols, 3) triples: a third graph edges (dropped), a third random ids (mostly not in the graph), the rest repeats
    of earlier entries (duplicate keys), a few negative ids (skipped)."""
    g = torch.Generator().manual_seed(seed)
    n = rows * cols
    e = torch.randint(0, data.num_edges, (n,), generator=g)
    out = torch.stack([data.edge_index[0, e], data.edge_index[1, e], data.edge_type[e] % (data.num_relations // 2)], dim=-1)
    rnd = torch.rand(n, generator=g)
    out[rnd < 1 / 3, 0] = torch.randint(0, data.num_nodes, (int((rnd < 1 / 3).sum()),), generator=g)
    dup = rnd > 2 / 3
    out[dup] = out[torch.randint(0, n, (int(dup.sum()),), generator=g) // 3]
    out[:5, :2] = -1
    return out.view(rows, cols, 3).contiguous()


@pytest.fixture(scope="module")
def fb(dev):
    data = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], relation_graph=False)
    return data, data.to(dev)


@pytest.mark.parametrize("remove_one_hop", [False, True])
@pytest.mark.parametrize("rows,cols", [(64, 513), (8, 257), (3, 5)])
def test_table_filter_equals_easy_edge_mask(dev, fb, remove_one_hop, rows, cols):
    """32,832 triples (65,664 keys, pre-training's batch) and <= 4,096: the table route's vector is easy_edge_mask's, for the
    columns of a (rows, cols, 3) batch (stride 3), for contiguous vectors (stride 1) and for other layouts (copied)."""
    data, gdata = fb
    batch = _batch(data, rows, cols, seed=rows + cols).to(dev)
    net = models.EntityNBFNet(64, [64], remove_one_hop=remove_one_hop)
    h, t, r = batch.unbind(-1)
    want = net.easy_edge_mask(gdata, h, t, r).float()
    edge_type = None if remove_one_hop else gdata.edge_type
    for args in ((h, t, r), (h.contiguous(), t.contiguous(), r.contiguous()), (h.t(), t.t(), r.t())):
        got = dense.easy_edge_keep_table(gdata.edge_index, edge_type, *args, gdata.num_nodes, gdata.num_relations)
        assert torch.equal(got, want)
    assert int((want == 0).sum()) > 0
    if rows * cols > 4096:
        # the model's chain: neither LDS route takes 65,664 keys, the table does (no edge_match, no host synchronisation)
        assert dense.easy_edge_keep(gdata.edge_index, edge_type, h, t, r, gdata.num_nodes, gdata.num_relations) is None
        assert torch.equal(net.easy_edge_keep(gdata, h, t, r), want)


def test_table_filter_matches_the_reference_golden(dev):
    """The edges the REFERENCE's remove_easy_edges keeps (tests/golden/easy_edges.pt) through the table route."""
    from tests.test_tasks import easy_edges_golden
    data, cases = easy_edges_golden()
    gdata = data.to(dev)
    assert {c["remove_one_hop"] for c in cases} == {False, True}
    for case in cases:
        h, t, r = case["batch"].to(dev).unbind(-1)
        got = dense.easy_edge_keep_table(gdata.edge_index, None if case["remove_one_hop"] else gdata.edge_type, h, t, r,
                                         gdata.num_nodes, gdata.num_relations)
        assert torch.equal(got.bool().cpu(), case["keep"])


def test_table_filter_records_into_a_cuda_graph(dev, fb):
    data, gdata = fb
    static = _batch(data, 64, 513, seed=1).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h, t, r = static.unbind(-1)
        dense.easy_edge_keep_table(gdata.edge_index, gdata.edge_type, h, t, r, gdata.num_nodes, gdata.num_relations)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h, t, r = static.unbind(-1)
        out = dense.easy_edge_keep_table(gdata.edge_index, gdata.edge_type, h, t, r, gdata.num_nodes, gdata.num_relations)
    net = models.EntityNBFNet(64, [64])
    for seed in (2, 3):
        fresh = _batch(data, 64, 513, seed=seed).to(dev)
        static.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        want = net.easy_edge_mask(gdata, *fresh.unbind(-1)).float()
        assert torch.equal(out, want)


def test_table_workspace_and_refusals():
    lib = _lib.lib
    assert lib.ultra_easy_edge_keep_table_workspace(0) == 8 * 1024
    assert lib.ultra_easy_edge_keep_table_workspace(32832) == 8 * 262144           # >= 2 slots per key, a power of two
    assert lib.ultra_easy_edge_keep_table_workspace(-1) == -1
    x = torch.zeros(4, dtype=torch.long)
    assert lib.ultra_easy_edge_keep_table(x.data_ptr(), x.data_ptr(), None, 4, x.data_ptr(), x.data_ptr(), None, 2, 1, 4, 2, 1,
                                          x.data_ptr(), 16, x.data_ptr(), None) == _lib.ULTRA_ERR_INVALID
    assert b"workspace" in lib.ultra_last_error()


class _GatherWatch(object):
    """dense.lib with the rows backward gather's return codes noted (ULTRA_ERR_UNSUPPORTED = the float-atomic scatter ran)."""

    def __init__(self, lib):
        self._lib, self.codes = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ultra_rspmm_rows_backward_gather":
            return fn

        def watched(*args):
            rc = fn(*args)
            self.codes.append(rc)
            return rc
        return watched


def test_batch64_step_gradients_match_fp64_oracle(dev, monkeypatch):
    """One bs-64 x 513 step as pre-training runs it (strict negatives, temperature 1) on a graph of 2,100 nodes -- the last layer
    on the candidates' rows (4 x 513 <= 2,100), its backward the gather -- against torch autograd over the CPU oracle model on
    the graph the reference's remove_easy_edges leaves, in fp32 and fp64 (tolerances of test_models_gpu's train-mode test)."""
    from oracle import ultra_oracle_model as om
    from tests.test_train_gpu import reference_loss
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=2100, num_triple=9000, num_relation_base=5, num_test=16, seed=6)
    pick = torch.arange(64) * 97
    batch = torch.stack([data.edge_index[0, pick], data.edge_index[1, pick], data.edge_type[pick]], dim=-1)
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 512, strict=True)
    assert neg.shape == (64, 513, 3)
    h, t, r = neg.unbind(-1)
    keep = reference_easy_edge_keep(data.edge_index, data.edge_type, h, t, r, data.num_relations)
    filtered = copy.copy(data)
    filtered.edge_index, filtered.edge_type = data.edge_index[:, keep], data.edge_type[keep]

    def cpu_step(dtype):
        sd = {k: v.clone().to(dtype).requires_grad_() for k, v in state.items()}
        with torch.enable_grad():
            rel = om.rel_nbfnet(sd, data.relation_graph, neg[:, 0, 2], cfg["rel_model_cfg"], oracle_rspmm)
            pred = om.entity_nbfnet(sd, filtered, rel, neg, cfg["entity_model_cfg"], oracle_rspmm)
            loss = reference_loss(pred, 1.0, 512)
            loss.backward()
        return loss.item(), pred.detach(), {k: v.grad.double() for k, v in sd.items()}

    loss32, pred32, g32 = cpu_step(torch.float32)
    loss64, _, g64 = cpu_step(torch.float64)

    calls = []
    real_table = dense.easy_edge_keep_table
    monkeypatch.setattr(dense, "easy_edge_keep_table", lambda *a, **k: calls.append(1) or real_table(*a, **k))
    watch = _GatherWatch(dense.lib)
    monkeypatch.setattr(dense, "lib", watch)
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).train()
    pred = model(data.to(dev), neg.to(dev))
    assert calls, "the 65,664-key filter did not take the table route"
    assert model.entity_model._last_hidden_on_rows, "the last layer did not run on the candidates' rows"
    loss = train.ranking_loss(pred, 1.0, 512)
    loss.backward()
    assert watch.codes and all(rc == _lib.ULTRA_OK for rc in watch.codes), watch.codes     # no float-atomic scatter
    assert (pred.detach().cpu() - pred32).abs().max().item() <= TOL
    assert abs(loss.item() - loss32) <= 1e-5, (loss.item(), loss32)
    for name, p in model.named_parameters():
        got, want, cpu = p.grad.cpu().double(), g64[name], g32[name]
        scale = max(want.abs().max().item(), 1e-6)
        err_gpu, err_cpu = (got - want).abs().max().item(), (cpu - want).abs().max().item()
        assert err_gpu <= 4 * err_cpu + 1e-4 * scale + 1e-7, \
            "%s: |gpu - fp64| = %g, |cpu fp32 - fp64| = %g (scale %g)" % (name, err_gpu, err_cpu, scale)


def _three_graphs(dev):
    shapes = ((2100, 9000, 5, 7), (2600, 6000, 3, 8), (3300, 12000, 7, 9))
    return [synthetic.make_split(n, m, r, num_valid=40, num_test=40, seed=s) for n, m, r, s in shapes]


def _fresh(dev):
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    return model.to(dev).train()


def test_captured_steps_over_three_graphs_equal_eager_steps(dev):
    """Seven bs-64 x 513 steps over three graphs of different sizes in a fixed order, through PretrainTrainer's captured steps
    (one per graph, one optimiser) and through train.train_step: the same losses, parameters and AdamW state, bit for bit.
    The seventh is a short batch (eager inside the trainer too)."""
    splits = _three_graphs(dev)
    graphs = [s[0].to(dev) for s in splits]
    order = [0, 2, 1, 2, 0, 1, 0]
    torch.manual_seed(5)
    batches = []
    for k, gid in enumerate(order):
        rows = 64 if k < len(order) - 1 else 22
        pos = pretrain.target_triples(graphs[gid])[torch.randperm(graphs[gid].target_edge_index.shape[1], device=dev)[:rows]]
        batches.append(tasks.negative_sampling(graphs[gid], pos, 512, strict=True))

    eager = _fresh(dev)
    opt = train.make_adamw(eager, lr=5e-3)
    want = [train.train_step(eager, graphs[gid], b, opt, 1.0, 512).item() for gid, b in zip(order, batches)]

    model = _fresh(dev)
    before = [p.detach().clone() for p in model.parameters()]
    opt2 = train.make_adamw(model, lr=5e-3, capturable=True)
    torch.cuda.reset_peak_memory_stats(dev)
    trainer = pretrain.PretrainTrainer(model, graphs, opt2, 64, 512, 1.0)
    for p, b in zip(model.parameters(), before):
        assert torch.equal(p, b)            # the warm-ups left no trace
    got = [trainer.step(gid, b).item() for gid, b in zip(order, batches)]
    trainer.check()
    assert got == want, (got, want)
    for (name, p), q in zip(model.named_parameters(), eager.parameters()):
        assert torch.equal(p, q), name
    for p, q in zip(model.parameters(), eager.parameters()):
        s1, s2 = opt2.state[p], opt.state[q]
        assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
        assert int(s1["step"].item()) == int(s2["step"].item()) == len(order)
    print("peak memory with three captures: %.2f GB" % (torch.cuda.max_memory_allocated(dev) / 1e9))


def test_train_and_validate_writes_loadable_checkpoints(dev, tmp_path):
    splits = _three_graphs(dev)
    train_data = [s[0].to(dev) for s in splits]
    valid_data = [s[1].to(dev) for s in splits]
    test_data = [s[2].to(dev) for s in splits]
    filt = pretrain.filter_graphs(train_data, valid_data, test_data)
    cfg = {"train": {"num_epoch": 2, "batch_size": 16, "log_interval": 5},
           "task": {"num_negative": 32, "strict_negative": True, "adversarial_temperature": 1, "metric": ["mr", "mrr"]},
           "optimizer": {"class": "AdamW", "lr": 5e-4}}
    model = _fresh(dev)
    stats = {}
    best = pretrain.train_and_validate(cfg, model, train_data, valid_data, filt, batch_per_epoch=6, working_dir=str(tmp_path),
                                       stats=stats)
    assert sorted(os.listdir(tmp_path)) == ["model_epoch_1.pth", "model_epoch_2.pth"]
    results = [r for _, r in stats["valid"]]
    assert best == max(results)
    best_epoch = stats["valid"][results.index(best)][0]
    _, _, _, cfg_m = load_golden("ultra_3g", "sum")
    for k in (1, 2):
        state = torch.load(tmp_path / ("model_epoch_%d.pth" % k), map_location="cpu")
        assert set(state) == {"model", "optimizer"}
        models.Ultra(**cfg_m).load_state_dict(state["model"], strict=True)
    reloaded = torch.load(tmp_path / ("model_epoch_%d.pth" % best_epoch), map_location="cpu")["model"]
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), reloaded[k]), k
    per_graph, mean = pretrain.test(cfg, model, valid_data, filt)
    assert len(per_graph) == 3 and mean == pytest.approx(sum(float(r["mrr"]) for r in per_graph) / 3)
    assert mean == pytest.approx(best)
    assert all(l == l for l in stats["epoch_loss"])


TWO_RANKS = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from ultra_amd import models, pretrain, synthetic, tasks, train
rank = int(os.environ["RANK"])
dev = torch.device("cuda", 0)                            # both ranks on the one GPU of the box: gloo carries the collectives
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
torch.manual_seed(11 + rank)                             # seed + rank (pretrain.py:230): different initial weights
model = models.Ultra(**synthetic.default_model_cfg()).to(dev).train()
graphs = [synthetic.make_split(n, m, 4, num_valid=8, num_test=8, seed=s)[0].to(dev) for n, m, s in ((600, 3000, 1), (900, 4000, 2))]
opt = train.make_adamw(model, lr=5e-3, capturable=True)
trainer = pretrain.PretrainTrainer(model, graphs, opt, 8, 16, 1.0)
for k in range(3):
    gid = (k + rank) %% 2                                 # every rank its own graph
    rows = 8 if k < 2 else 5                             # the third: a short batch, eager
    pos = pretrain.target_triples(graphs[gid])[k * 8 + rank * 3:k * 8 + rank * 3 + rows]
    trainer.step(gid, tasks.negative_sampling(graphs[gid], pos, 16, strict=True))
flat = torch.cat([p.detach().flatten() for p in model.parameters()])
parts = [torch.empty_like(flat) for _ in range(2)]
dist.all_gather(parts, flat)
assert torch.equal(parts[0], parts[1]), "parameters differ across ranks"
print("PRE2_OK rank %%d" %% rank)
dist.destroy_process_group()
"""


def test_two_ranks_seeded_differently_hold_identical_parameters(tmp_path):
    script = tmp_path / "pretrain_two.py"
    script.write_text(TWO_RANKS % ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.count("PRE2_OK") == 2, (r.stdout + r.stderr)[-3000:]
