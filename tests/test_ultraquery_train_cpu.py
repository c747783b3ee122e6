"""UltraQuery training without a GPU: the torch restatements of traversal dropout and of the query loss against the reference's
recorded outputs (tests/golden/ultraquery_train.pt.xz, tests/golden/gen_ultraquery_train_golden.py), and the BetaE train split."""
import io
import lzma
import os
import pickle

import pytest
import torch

from ultra_amd import query_data
from ultra_amd.query_train import query_loss_reference, traversal_dropout_reference

HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def load():
    if "g" not in _CACHE:
        with open(os.path.join(HERE, "golden", "ultraquery_train.pt.xz"), "rb") as f:
            _CACHE["g"] = torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)
    return _CACHE["g"]


def test_dropout_restatement_equals_reference_kept_edges():
    g = load()
    gen = torch.Generator().manual_seed(0)
    E = g["edge_index"].shape[1]
    for case in g["dropout"]:
        for (ratio, more), kept in case["kept"].items():
            u1, u2 = torch.rand(E, generator=gen), torch.rand(E, generator=gen)
            keep, _ = traversal_dropout_reference(g["edge_index"], g["edge_type"], g["num_nodes"], g["num_relations"],
                                                  case["sym"], case["r_index"], ratio, more, case["inverse_rel_plus_one"],
                                                  u1, u2)
            assert torch.equal(keep.bool(), kept), (case["sym"].shape, ratio, more)


def test_dropout_multiplicity_is_reference_match_count():
    g = load()
    E = g["edge_index"].shape[1]
    for case in g["dropout"]:
        _, k = traversal_dropout_reference(g["edge_index"], g["edge_type"], g["num_nodes"], g["num_relations"], case["sym"],
                                           case["r_index"], 1.0, 0.0, case["inverse_rel_plus_one"], torch.zeros(E))
        assert torch.equal(k.long(), torch.bincount(case["match"], minlength=E)), case["sym"].shape
    # duplicates are real: some edge is matched more than once in the recorded lists
    assert any(int(torch.bincount(c["match"]).max()) > 1 for c in g["dropout"])


def _run_query_loss(pred, target, temperature):
    """run_query.py:94-114 step by step (variadic softmax over each row's negatives)."""
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, target, reduction="none")
    is_pos, is_neg = target > 0.5, target <= 0.5
    num_pos, num_neg = is_pos.sum(-1), is_neg.sum(-1)
    w = torch.zeros_like(pred)
    w[is_pos] = (1 / num_pos.to(pred.dtype)).repeat_interleave(num_pos)
    with torch.no_grad():
        if temperature > 0:
            logit = pred[is_neg] / temperature
            seg = torch.arange(len(pred)).repeat_interleave(num_neg)
            mx = torch.full((len(pred),), float("-inf"), dtype=pred.dtype).scatter_reduce(0, seg, logit, "amax")
            e = (logit - mx[seg]).exp()
            w[is_neg] = e / torch.zeros(len(pred), dtype=pred.dtype).index_add_(0, seg, e)[seg]
        else:
            w[is_neg] = (1 / num_neg.to(pred.dtype)).repeat_interleave(num_neg)
    return ((loss * w).sum(-1) / w.sum(-1)).mean()


@pytest.mark.parametrize("temperature", [0.2, 0.0])
@pytest.mark.parametrize("positives", ["one", "many"])
def test_loss_restatement(temperature, positives):
    gen = torch.Generator().manual_seed(4)
    pred = (torch.randn(6, 300, generator=gen, dtype=torch.float64) * 4).requires_grad_()
    target = torch.zeros(6, 300, dtype=torch.float64)
    if positives == "one":
        target[torch.arange(6), torch.randint(0, 300, (6,), generator=gen)] = 1
    else:
        target[torch.rand(6, 300, generator=gen) < 0.3] = 1
    ref = _run_query_loss(pred, target, temperature)
    got = query_loss_reference(pred, target, temperature)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0)
    g_ref, = torch.autograd.grad(ref, pred)
    g_got, = torch.autograd.grad(got, pred)
    torch.testing.assert_close(g_got, g_ref, rtol=1e-10, atol=1e-15)


def test_loss_restatement_gives_the_reference_logged_loss():
    t = load()["train"]
    loss = query_loss_reference(t["pred"], t["target"], t["temperature"])
    assert abs(float(loss) - t["logged_loss"]) <= 1e-5 * abs(t["logged_loss"]) + 1e-6     # (logged with %g)


def test_load_betae_train_split(tmp_path):
    with open(tmp_path / "train.txt", "w") as f:
        f.write("0 0 1\n1 1 0\n1 0 2\n2 1 1\n")
    with open(tmp_path / "stats.txt", "w") as f:
        f.write("numentity: 3\nnumrelations: 2\n")
    q1p, q2p = (0, (0,)), (0, (0, 0))
    with open(tmp_path / "train-queries.pkl", "wb") as f:
        pickle.dump({("e", ("r",)): {q1p}, ("e", ("r", "r")): {q2p}}, f)
    with open(tmp_path / "train-answers.pkl", "wb") as f:
        pickle.dump({q1p: {1}, q2p: {2}}, f)
    graph, ds = query_data.load_betae(str(tmp_path), split="train")
    assert len(ds) == 2 and graph.num_nodes == 3
    items = {ds.id2type[it["type"]]: it for it in (ds[i] for i in range(len(ds)))}
    assert items["1p"]["easy_answer"].nonzero().flatten().tolist() == [1]
    assert items["2p"]["easy_answer"].nonzero().flatten().tolist() == [2]
    assert not items["1p"]["hard_answer"].any() and not items["2p"]["hard_answer"].any()
