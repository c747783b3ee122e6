"""Leave-one-out verification on the GPU: the per-sample masked walk (ultra_rspmm_forward_masked_samples and the per-slice
loop behind it) against each sample's filtered graph, the mask kernel (ultra_leave_one_out_keep) against the torch
restatement, the `edge_keep=` forward against a forward per filtered copy of the graph, and Predictor.verify_* against
predict.verify_reference."""
import collections
import gc

import pytest
import torch

from tests.test_oracle_model import load_golden
from ultra_amd import _lib, dense, models, predict, rspmm, synthetic, tasks

pytestmark = pytest.mark.gpu

TOL = 1e-4      # tests/test_models_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- 1 / 2: the walk with one keep mask per outer slice ----
N, E, R, BS = 400, 9000, 6, 3


@pytest.fixture(scope="module")
def walk():
    """The graph of test_masked_forward_equals_the_filtered_graph (700 edges into row 7: the chain path), three keep rows that
    differ, the operands, and the plans of the full graph and of every sample's filtered graph -- built once, never written."""
    gen = torch.Generator().manual_seed(3)
    ei = torch.randint(0, N, (2, E), generator=gen)
    ei[0, :700] = 7
    et = torch.randint(0, R, (E,), generator=gen)
    keep = torch.ones(BS, E, dtype=torch.bool)                       # sample 0 keeps everything
    keep[1] = torch.rand(E, generator=gen) > 0.3                     # sample 1 drops ~ 30 % at random ...
    keep[1, ei[0] == 11] = False                                     # ... and every edge of row 11
    keep[2, (ei[0] == 7) & (torch.rand(E, generator=gen) < 0.5)] = False      # sample 2 drops edges of the hub row only
    assert keep[1].sum() < 0.75 * E and 0 < (~keep[2]).sum() < 700 and not (~keep[2] & (ei[0] != 7)).any()
    rel = torch.randn(BS, R, 64, generator=gen)
    x = torch.randn(BS, N, 64, generator=gen).relu()                 # exact zeros: 0-weight and absent differ under max
    bnd = torch.randn(BS, N, 64, generator=gen)
    plans = {}
    for exact in (True, False):
        plans[exact] = (rspmm.Plan(ei, et, N, R, exact_order=exact),
                        [rspmm.Plan(ei[:, keep[s]], et[keep[s]], N, R, exact_order=exact) for s in range(BS)])
    return dict(ei=ei, et=et, keep=keep, rel=rel, x=x, bnd=bnd, plans=plans)


WALK_CASES = [(s, m, ex, torch.float32) for s in ("add", "min", "max") for m in ("mul", "add") for ex in (True, False)] \
    + [("add", "mul", True, torch.float64), ("add", "mul", False, torch.float64)]


@pytest.mark.parametrize("sum,mul,exact,dtype", WALK_CASES)
def test_per_sample_masked_forward_equals_each_samples_filtered_graph(dev, walk, sum, mul, exact, dtype):
    full, parts = walk["plans"][exact]
    rel, x, bnd = (walk[k].to(dev, dtype) for k in ("rel", "x", "bnd"))
    keep = walk["keep"].to(dev, dtype)
    for boundary in (bnd, None):
        want = torch.cat([parts[s].forward(rel[s:s + 1], x[s:s + 1], boundary=None if boundary is None else boundary[s:s + 1],
                                           sum=sum, mul=mul) for s in range(BS)])
        got = full.forward(rel, x, edge_weight=keep, boundary=boundary, sum=sum, mul=mul, keep=True)
        # which route served it: the entry point itself on reference-order plans, the per-slice loop elsewhere
        probe = torch.empty_like(got)
        rc = full.masked_samples_entry(rel, x, keep, boundary, sum, mul, probe)
        if exact:
            assert rc == _lib.ULTRA_OK and torch.equal(probe, got)
        else:
            assert rc == _lib.ULTRA_ERR_UNSUPPORTED
        err = (got - want).abs().max().item()
        print("%s %s exact=%s %s boundary=%s: max |d| = %g" % (sum, mul, exact, dtype, boundary is not None, err))
        if exact or sum != "add":
            assert torch.equal(got, want)
        else:
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-4)
    if sum != "add":      # the mask is not a zero weight: sample 1's row 11 lost every edge
        assert not torch.equal(got, full.forward(rel, x, sum=sum, mul=mul))


@pytest.mark.parametrize("exact", [True, False])
def test_keep_rows_may_be_a_strided_view(dev, walk, exact):
    full, parts = walk["plans"][exact]
    rel, x = walk["rel"].to(dev), walk["x"].to(dev)
    wide = torch.full((BS, E + 7), float("nan"), device=dev)         # (padding that must never be read as a weight)
    wide[:, :E] = walk["keep"].to(dev, torch.float32)
    view = wide[:, :E]
    assert view.stride(0) == E + 7
    got = full.forward(rel, x, edge_weight=view, sum="add", mul="mul", keep=True)
    want = torch.cat([parts[s].forward(rel[s:s + 1], x[s:s + 1]) for s in range(BS)])
    if exact:
        assert torch.equal(got, want)
    else:
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("sum", ["add", "max"])
def test_per_sample_call_agrees_with_the_shared_route(dev, walk, exact, sum):
    full, _ = walk["plans"][exact]
    rel, x, bnd = walk["rel"].to(dev), walk["x"].to(dev), walk["bnd"].to(dev)
    row = walk["keep"][1].to(dev, torch.float32)
    same = row.unsqueeze(0).expand(BS, -1).contiguous()
    shared = full.forward(rel, x, edge_weight=row, boundary=bnd, sum=sum, mul="mul", keep=True)
    assert torch.equal(full.forward(rel, x, edge_weight=same, boundary=bnd, sum=sum, mul="mul", keep=True), shared)
    ones = torch.ones(BS, E, device=dev)
    plain = full.forward(rel, x, boundary=bnd, sum=sum, mul="mul")
    assert torch.equal(full.forward(rel, x, edge_weight=ones, boundary=bnd, sum=sum, mul="mul", keep=True), plain)


# ---- 3: the mask kernel ----
@pytest.mark.parametrize("n_sample", [1, 3, 64])
@pytest.mark.parametrize("columns", [True, False])
@pytest.mark.parametrize("remove_one_hop", [False, True])
def test_mask_kernel_equals_the_torch_restatement(dev, n_sample, columns, remove_one_hop):
    data = synthetic.make_kg(num_node=60, num_triple=400, num_relation_base=3, seed=5, relation_graph=False)
    gen = torch.Generator().manual_seed(n_sample)
    num_edge = data.edge_index.shape[1]
    pick = torch.randint(0, num_edge // 2, (n_sample,), generator=gen)
    triples = torch.stack([data.edge_index[0, pick], data.edge_index[1, pick], data.edge_type[pick]], dim=-1)
    if n_sample > 1:
        triples[n_sample // 2] = torch.tensor([59, 58, 1])  # (likely) not a fact: whatever the restatement says
    net = models.EntityNBFNet(64, [64], remove_one_hop=remove_one_hop)
    want = net.leave_one_out_keep(data, triples)             # CPU: the restatement via tasks.edge_match
    assert (want == 0).any()
    gdata = data.to(dev)
    gt = triples.to(dev)
    if columns:
        h, t, r = gt.unbind(-1)                              # stride 3
    else:
        h, t, r = (c.contiguous() for c in gt.unbind(-1))    # stride 1
    buf = torch.full((n_sample, num_edge + 5), -7.0, device=dev)
    got = dense.leave_one_out_keep(gdata.edge_index, None if remove_one_hop else gdata.edge_type, h, t, r, data.num_nodes,
                                   data.num_relations, out=buf)
    assert got is not None and got.shape == (n_sample, num_edge)
    assert torch.equal(got.cpu(), want)
    assert bool((buf[:, num_edge:] == -7.0).all())           # the padding of a row is not touched
    assert torch.equal(net.leave_one_out_keep(gdata, gt).cpu(), want)


# ---- 4 - 6: model and predictor ----
GRAPH_EDGES = [16, 35, 10, 23]      # direct edges whose score the ORACLE moves by 0.8 .. 1.3 when the fact is removed (10: stated twice)


@pytest.fixture(scope="module")
def served(dev):
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=400, num_triple=3000, num_relation_base=5, num_test=21, seed=3)
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    facts = torch.stack([data.edge_index[0], data.edge_index[1], data.edge_type], dim=-1)      # (h, t, r)
    stated = {tuple(f) for f in facts.tolist()}
    absent = next(tr for tr in data.target_triples.tolist() if tuple(tr) not in stated)
    return model, data.to(dev), facts, torch.tensor(absent)


def filtered_copy(model, gdata, triple):
    return model.entity_model.remove_easy_edges(gdata, triple[0:1], triple[1:2], triple[2:3])


def test_edge_keep_forward_equals_a_forward_per_filtered_graph(dev, served):
    model, gdata, facts, absent = served
    batch = torch.cat([facts[GRAPH_EDGES], absent.unsqueeze(0)]).to(dev)                # four facts of the graph, one that is not
    t_batch, _ = tasks.all_negative(gdata, batch)
    keep = model.entity_model.leave_one_out_keep(gdata, batch)
    assert (keep == 0).sum(dim=1).tolist() == [2, 2, 4, 2, 0]
    with torch.no_grad():
        got = model(gdata, t_batch, edge_keep=keep)
        plain = model(gdata, t_batch)
        want = torch.cat([model(filtered_copy(model, gdata, batch[s]), t_batch[s:s + 1]) for s in range(len(batch))])
    err = (got - want).abs().max().item()
    print("edge_keep forward vs per-sample filtered graphs: max |d| = %g, bits equal: %s" % (err, torch.equal(got, want)))
    assert torch.equal(got, want)
    # the mask acted: the positives of the four stated facts moved, the fifth sample saw the whole graph
    pos = batch[:, 1:2]
    moved = (got.gather(1, pos) - plain.gather(1, pos)).abs().flatten()
    print("positives moved by", moved.tolist())
    assert bool((moved[:4] > 10 * TOL).all())
    assert torch.equal(got[4], plain[4])


N_FACTS, VERIFY_BS = 11, 4


@pytest.fixture(scope="module")
def verified(dev, served):
    """11 facts -- eight of the graph (a duplicate among them), three that are not -- and what the reference loop says."""
    model, gdata, facts, absent = served
    triples = torch.cat([facts[GRAPH_EDGES], facts[[0, 9, 19, 31]], gdata.target_triples[:2].cpu(), absent.unsqueeze(0)]).to(dev)
    assert len(triples) == N_FACTS
    h, t, r = triples.unbind(-1)
    want = {mode: predict.verify_reference(model, gdata, gdata, h, r, t, mode) for mode in ("tail", "head")}
    return h, r, t, want


def assert_verified(got, want, what):
    for name, a, b in zip(("score", "rank", "num_negative"), got, want):
        a, b = a.cpu(), b.cpu()
        if name == "score":
            print("%s score: max |d| = %g" % (what, (a - b).abs().max().item()))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert a.dtype == torch.int64 and torch.equal(a, b), "%s %s: %s vs %s" % (what, name, a.tolist(), b.tolist())


@pytest.mark.parametrize("mode", ["tail", "head"])
def test_predictor_verifies_like_the_reference_loop(dev, served, verified, mode):
    model, gdata, _, _ = served
    h, r, t, want = verified
    predictor = predict.Predictor(model, gdata, batch_size=VERIFY_BS)
    call = predictor.verify_tails if mode == "tail" else predictor.verify_heads
    got = call(h, r, t)
    assert_verified(got, want[mode], "captured " + mode)
    step = predictor._steps["verify_" + mode]
    assert len(step.graphs) == 1 and step.plans
    again = call(h, r, t)                                                  # the same call twice: the same bits, the same capture
    assert_verified(again, got, "replayed " + mode)
    assert predictor._steps["verify_" + mode] is step
    eager = predict.Predictor(model, gdata, batch_size=VERIFY_BS, use_graph=False)
    assert_verified((eager.verify_tails if mode == "tail" else eager.verify_heads)(h, r, t), got, "eager " + mode)
    assert eager._steps == {}
    if mode == "tail":      # the stated facts cannot see themselves: the unmasked scores are other numbers (GRAPH_EDGES)
        with torch.no_grad():
            plain = model(gdata, predict._candidates(gdata, h[:4], r[:4], mode)).gather(1, t[:4].unsqueeze(-1)).flatten()
        assert bool(((plain - got[0][:4]).abs() > 10 * TOL).all())
    predictor.close()


def test_a_changed_parameter_recaptures(dev, served, verified):
    model, gdata, _, _ = served
    h, r, t, _ = verified
    predictor = predict.Predictor(model, gdata, batch_size=VERIFY_BS)
    before = predictor.verify_tails(h, r, t)
    step = predictor._steps["verify_tail"]
    weight = model.entity_model.mlp[-1].bias
    saved = weight.detach().clone()
    with torch.no_grad():
        weight.add_(0.5)
    try:
        after = predictor.verify_tails(h, r, t)
        assert predictor._steps["verify_tail"] is not step and step.plans == []       # the stale capture let go of its plans
        eager = predict.Predictor(model, gdata, batch_size=VERIFY_BS, use_graph=False).verify_tails(h, r, t)
        assert_verified(after, eager, "re-captured")
        assert not torch.equal(after[0], before[0])
    finally:
        with torch.no_grad():
            weight.copy_(saved)
        predictor.close()


def test_no_plan_stays_pinned_after_verifying(dev, served, verified, monkeypatch):
    model, gdata, _, _ = served
    h, r, t, _ = verified
    pins = collections.Counter()
    plain_pin = rspmm.Plan.pin

    def counting_pin(self, delta=1):
        pins[id(self)] += delta
        return plain_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_pin)
    predictor = predict.Predictor(model, gdata, batch_size=VERIFY_BS)
    predictor.verify_tails(h, r, t)
    predictor.verify_heads(h, r, t)
    assert pins and all(v > 0 for v in pins.values())       # the captures hold their plans ...
    predictor.close()
    del predictor
    gc.collect()
    assert all(v == 0 for v in pins.values())               # ... and let go of them


def test_a_model_outside_the_fused_path_is_verified_without_a_capture(dev, served, verified, monkeypatch):
    model, gdata, _, _ = served
    h, r, t, _ = verified
    pins = collections.Counter()
    plain_pin = rspmm.Plan.pin

    def counting_pin(self, delta=1):
        pins[id(self)] += delta
        return plain_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_pin)
    monkeypatch.setattr(dense, "readout_supported", lambda *args, **kwargs: False)      # (the generic readout: not captured)
    want = predict.verify_reference(model, gdata, gdata, h, r, t, "tail")
    predictor = predict.Predictor(model, gdata, batch_size=VERIFY_BS)
    for _ in range(2):
        assert_verified(predictor.verify_tails(h, r, t), want, "outside the fused path")
    assert predictor._eager_only and predictor._steps == {}
    assert all(v == 0 for v in pins.values())
