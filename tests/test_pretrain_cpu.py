"""Multi-graph pre-training without a GPU: the engine's seeded run (ultra_amd.pretrain.run) draws from the global CPU generator
exactly what the reference's script/pretrain.py draws -- the fast_test subsets, the model's initial state, and the (graph id,
batch) sequence of its DataLoader over two epochs, short last batches included (tests/golden/pretrain.pt.xz, recorded from the
reference by tests/golden/gen_pretrain_golden.py).  The step is a stand-in here, as in the recording: what is under test is the
order in which the run consumes the generator."""
import io
import lzma
import os
import types

import pytest
import torch

from ultra_amd import models, pretrain, synthetic, tasks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain.pt.xz")


@pytest.fixture(scope="module")
def golden():
    with lzma.open(GOLDEN, "rb") as f:
        return torch.load(io.BytesIO(f.read()), weights_only=False)


def _splits(golden):
    splits = [synthetic.make_split(n, m, r, num_valid=v, num_test=t, seed=s, relation_graph=False)
              for n, m, r, v, t, s in golden["shapes"]]
    for (train, valid, test), g in zip(splits, golden["graphs"]):
        assert torch.equal(train.edge_index, g["edge_index"]) and torch.equal(train.edge_type, g["edge_type"])
        assert torch.equal(train.target_triples, g["train"]) and torch.equal(valid.target_triples, g["valid"])
        assert torch.equal(test.target_triples, g["test"])
    return [s[0] for s in splits], [s[1] for s in splits], [s[2] for s in splits]


class Stand(torch.nn.Module):
    """The golden run's one-parameter stand-in for the model (Ultra's forward draws nothing)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(()))

    def forward(self, graph, batch):
        return batch[..., 0].to(torch.float32) * 0 + self.w


def test_seeded_run_draws_what_the_reference_draws(golden, tmp_path, monkeypatch):
    train, valid, test = _splits(golden)
    seen, subsets, states = [], [], []

    def record(graph, batch, num_negative, strict=True):
        # (run() moves the graphs to the device, i.e. copies them: told apart by their node counts, which differ)
        seen.append(([g.num_nodes for g in train].index(graph.num_nodes), batch.clone()))
        return torch.stack([batch, batch], dim=1)

    real_subsets, real_ultra = pretrain.fast_test_subsets, models.Ultra

    def subsets_rec(graphs, k):
        out = real_subsets(graphs, k)
        subsets.extend(out)
        return out

    def ultra_rec(**kwargs):
        states.append(real_ultra(**kwargs).state_dict())
        return Stand()

    monkeypatch.setattr(tasks, "negative_sampling", record)
    monkeypatch.setattr(pretrain, "fast_test_subsets", subsets_rec)
    monkeypatch.setattr(pretrain, "models", types.SimpleNamespace(Ultra=ultra_rec))
    mcfg = synthetic.default_model_cfg()
    cfg = {"train": {"num_epoch": golden["num_epoch"], "batch_size": golden["batch_size"], "log_interval": 1000,
                     "fast_test": golden["fast_test_size"]},
           "task": {"num_negative": 1, "strict_negative": True, "adversarial_temperature": 1, "metric": ["mrr"]},
           "optimizer": {"class": "SGD", "lr": 0.0},
           "model": {"relation_model": mcfg["rel_model_cfg"], "entity_model": mcfg["entity_model_cfg"]}}
    pretrain.run(cfg, golden["seed"], train, valid, test, torch.device("cpu"), working_dir=str(tmp_path), capture=False)

    # the fast_test subsets
    assert len(subsets) == len(golden["fast_test"])
    for got, want in zip(subsets, golden["fast_test"]):
        assert torch.equal(got.target_edge_index, want["target_edge_index"])
        assert torch.equal(got.target_edge_type, want["target_edge_type"])
    # the seeded initial state: the same 82 tensors as the reference's Ultra under the same seed
    state, = states
    assert list(state) == list(golden["init_digest"]) and len(state) == 82
    for k, v in state.items():
        d = golden["init_digest"][k]
        assert tuple(v.shape) == d["shape"], k
        assert torch.equal(v.flatten()[:8], d["head"]), k
        assert float(v.double().sum()) == d["sum"] and float((v.double() ** 2).sum()) == d["sumsq"], k
    # the (graph id, batch) sequence over two epochs, the short last batches included
    want = golden["batches"]
    assert len(seen) == len(want)
    assert [g for g, _ in seen] == [g for g, _ in want]
    for (_, got), (_, b) in zip(seen, want):
        assert torch.equal(got, b)
    rows = [len(b) for _, b in want]
    assert rows.count(golden["batch_size"]) == len(rows) - golden["num_epoch"] and rows[-1] < golden["batch_size"]
    # a checkpoint per chunk of ceil(num_epoch / 10) epochs
    assert sorted(os.listdir(tmp_path)) == ["model_epoch_%d.pth" % (e + 1) for e in range(golden["num_epoch"])]


def test_collator_picks_graphs_by_edge_count():
    graphs = [synthetic.make_split(40, m, 2, num_valid=8, num_test=8, seed=s, relation_graph=False)[0]
              for m, s in ((300, 1), (100, 2))]
    torch.manual_seed(0)
    picks = [pretrain.multigraph_collator([None] * 4, graphs)[0] for _ in range(2000)]
    share = picks.count(0) / len(picks)
    assert abs(share - 0.75) < 0.04, share


def test_example_batch_has_the_training_layout():
    graph = synthetic.make_split(50, 200, 3, num_valid=8, num_test=8, seed=3, relation_graph=False)[0]
    b = pretrain.example_batch(graph, 6, 9)
    assert b.shape == (6, 10, 3)
    assert (b[:3, :, 0] == b[:3, :1, 0]).all() and (b[3:, :, 1] == b[3:, :1, 1]).all() and (b[:, :, 2] == b[:, :1, 2]).all()
    assert torch.equal(b[:, 0], pretrain.target_triples(graph)[:6])


def test_split_helper_and_codex_m_shape():
    train, valid, test = synthetic.make_split(30, 100, 3, num_valid=10, num_test=12, seed=9, relation_graph=False)
    assert train.edge_index is valid.edge_index is test.edge_index
    assert train.target_edge_index.shape == (2, 100) and valid.target_edge_index.shape == (2, 10)
    assert test.target_edge_type.shape == (12,)
    assert torch.equal(train.edge_index[:, :100], train.target_edge_index)
    assert synthetic.SHAPES["codex_m"] == dict(num_node=17050, num_triple=185584, num_relation_base=51, num_test=10311)


def test_load_triples_dir_split(tmp_path):
    from ultra_amd import data
    rows = {"train.txt": ["a r b", "b r c", "c s a"], "valid.txt": ["a s c"], "test.txt": ["b s a", "c r b"]}
    for name, lines in rows.items():
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    t = data.load_triples_dir(str(tmp_path), relation_graph=False)
    tr = data.load_triples_dir(str(tmp_path), relation_graph=False, split="train")
    va = data.load_triples_dir(str(tmp_path), relation_graph=False, split="valid")
    assert t.target_edge_index.shape[1] == 2 and tr.target_edge_index.shape[1] == 3 and va.target_edge_index.shape[1] == 1
    assert torch.equal(tr.edge_index, t.edge_index) and torch.equal(va.edge_type, t.edge_type)
    with pytest.raises(ValueError):
        data.load_triples_dir(str(tmp_path), relation_graph=False, split="dev")
