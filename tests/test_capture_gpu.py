"""graph.Capture on the GPU, through the four captured steps that inherit it: a capture that fails leaves no plan pinned, no
stale graph to replay and (the training step) no trace of its warm-up; a re-capture leaks no pin.  The refused captures raise on
the host, from torch.cuda.CUDAGraph(), before anything is recorded.  (Captured against eager results, bit for bit: test_eval_gpu,
test_train_gpu, test_predict_gpu.)"""
import collections
import gc

import pytest
import torch

from tests.test_oracle_model import load_golden
from ultra_amd import dense, graph, models, predict, rspmm, synthetic, tasks, train

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def setting(dev):
    """(data, the 8 first test triples, fresh() -> a new model with the golden ultra_3g weights, in eval mode)."""
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=700, num_triple=6000, num_relation_base=9, num_test=16, seed=4).to(dev)
    triples = torch.cat([data.target_edge_index, data.target_edge_type.unsqueeze(0)]).t().contiguous()[:8]

    def fresh():
        model = models.Ultra(**cfg)
        model.load_state_dict(state)
        return model.to(dev).eval()
    return data, triples, fresh


@pytest.fixture
def pins(monkeypatch):
    """Counter of the pins every plan holds, by id."""
    count = collections.Counter()
    plain_pin = rspmm.Plan.pin

    def counting_pin(self, delta=1):
        count[id(self)] += delta
        return plain_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_pin)
    return count


def refuse_captures(monkeypatch):
    def no_graph(*args, **kwargs):
        raise RuntimeError("capture refused")
    monkeypatch.setattr(torch.cuda, "CUDAGraph", no_graph)


def train_batch(data, triples):
    torch.manual_seed(4)
    return tasks.negative_sampling(data, triples, 32, strict=True)


def build(kind, setting):
    data, triples, fresh = setting
    model = fresh()
    if kind == "forward":
        return graph.GraphedForward(model, data, tasks.all_negative(data, triples)[0])
    if kind == "eval":
        return graph.GraphedEvalStep(model, data, 8, tasks.known_answers(data, triples, "tail")[1],
                                     tasks.known_answers(data, triples, "head")[1])
    if kind == "predict":
        return predict._GraphedPredictStep(model, data, 8, 10, "tail", None)
    model.train()
    return train.GraphedTrainStep(model, data, train.make_adamw(model, lr=5e-3, capturable=True), train_batch(data, triples),
                                  num_negative=32)


@pytest.mark.parametrize("kind", ["forward", "eval", "predict", "train"])
def test_a_failed_capture_leaves_no_plan_pinned(setting, pins, monkeypatch, kind):
    refuse_captures(monkeypatch)
    with pytest.raises(RuntimeError, match="capture refused"):
        build(kind, setting)
    assert pins and all(v == 0 for v in pins.values()), pins
    assert not models.generic_path_capturable()


def test_a_forward_outside_the_fused_path_leaves_no_plan_pinned(setting, pins, monkeypatch):
    monkeypatch.setattr(dense, "readout_supported", lambda *args, **kwargs: False)      # (the generic readout: not captured)
    with pytest.raises(models.NotOnFusedPath):
        build("forward", setting)
    assert pins and all(v == 0 for v in pins.values()), pins


def optimizer_state(opt):
    return [{k: v.clone() for k, v in opt.state.get(p, {}).items() if torch.is_tensor(v)}
            for group in opt.param_groups for p in group["params"]]


def test_a_failed_capture_of_the_training_step_leaves_no_trace(setting, pins, monkeypatch):
    data, triples, fresh = setting
    batch = train_batch(data, triples)
    model = fresh().train()
    opt = train.make_adamw(model, lr=5e-3, capturable=True)
    before = [p.detach().clone() for p in model.parameters()]
    pin_calls = collections.Counter()
    counted_pin = rspmm.Plan.pin

    def counting_calls(self, delta=1):
        pin_calls[id(self)] += 1
        return counted_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_calls)

    def refused():
        held = {plan: n for plan, n in pins.items() if n}       # (the pins of a captured step that is alive stay)
        calls = sum(pin_calls.values())
        with monkeypatch.context() as patch:
            refuse_captures(patch)
            with pytest.raises(RuntimeError, match="capture refused"):
                train.GraphedTrainStep(model, data, opt, batch, num_negative=32)
        assert not models.generic_path_capturable()
        assert sum(pin_calls.values()) > calls                  # the refused capture had pinned its plans ...
        assert {plan: n for plan, n in pins.items() if n} == held, pins      # ... and let go of every one

    # an optimiser without state: the warm-up's steps created it, and it is back at zero
    refused()
    for (name, p), was in zip(model.named_parameters(), before):
        assert torch.equal(p, was), name
    for state in optimizer_state(opt):
        for key, value in state.items():
            assert not value.any(), key
    # an optimiser two steps into training: parameters, moments and step counters are what they were
    step = train.GraphedTrainStep(model, data, opt, batch, num_negative=32)
    step(batch)
    step(batch)
    torch.cuda.synchronize()
    before, state_before = [p.detach().clone() for p in model.parameters()], optimizer_state(opt)
    stepped = [int(state["step"]) for state in state_before if state]       # (a parameter outside the step has no state)
    assert stepped and all(n == 2 for n in stepped)
    refused()
    for (name, p), was in zip(model.named_parameters(), before):
        assert torch.equal(p, was), name
    for state, was in zip(optimizer_state(opt), state_before):
        assert state.keys() == was.keys()
        for key in was:
            assert torch.equal(state[key], was[key]), key
    del step
    gc.collect()
    assert all(v == 0 for v in pins.values()), pins


def update_in_place(model):
    """An optimizer-style update (as in test_graph_survives_plan_cache_eviction_and_weight_updates)."""
    for prm in model.entity_model.layers[0].relation_projection.parameters():
        prm.mul_(1.05)
    model.entity_model.mlp[0].weight.add_(0.01)


def test_a_recapture_leaks_no_pin(setting, pins):
    data, triples, fresh = setting
    model = fresh()
    t_batch = tasks.all_negative(data, triples)[0]
    with torch.no_grad():
        graphed = graph.GraphedForward(model, data, t_batch)
        want = model(data, t_batch).clone()
        assert torch.equal(graphed(t_batch), want)
        update_in_place(model)
        new = model(data, t_batch).clone()
        assert not torch.equal(new, want)
        assert torch.equal(graphed(t_batch), new)       # (re-captured)
    assert pins and all(v == 1 for v in pins.values()), pins
    assert len(graphed.plans) == len(pins) and len(graphed.graphs) == 1
    del graphed
    gc.collect()
    assert all(v == 0 for v in pins.values()), pins


def test_a_failed_recapture_cannot_replay_the_old_graph(setting, pins, monkeypatch):
    data, triples, fresh = setting
    model = fresh()
    t_batch = tasks.all_negative(data, triples)[0]
    with torch.no_grad():
        graphed = graph.GraphedForward(model, data, t_batch)
        want = model(data, t_batch).clone()
        assert torch.equal(graphed(t_batch), want)
        update_in_place(model)
        new = model(data, t_batch).clone()
        assert not torch.equal(new, want)
        with monkeypatch.context() as patch:
            refuse_captures(patch)
            for _ in range(2):          # (the second call must not find the old graph either)
                with pytest.raises(RuntimeError, match="capture refused"):
                    graphed(t_batch)
                assert pins and all(v == 0 for v in pins.values()), pins
                assert graphed.graphs == [] and graphed.plans == []
        assert torch.equal(graphed(t_batch), new)       # (captures are possible again: made again, with the new weights)
    assert all(v == 1 for v in pins.values()), pins
