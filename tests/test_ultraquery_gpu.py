"""UltraQuery on the GPU: the executor with the ultraquery.pth weights against the reference's recorded outputs
(tests/golden/gen_ultraquery_golden.py), the symbolic-traversal kernel bit for bit and the answer-ranking kernel integer for
integer against their torch restatements, and test_queries against the reference's metrics."""
import io
import lzma
import os

import pytest
import torch

from ultra_amd import synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ultraquery.pt.xz")
METRICS = ["mrr", "hits@1", "hits@3", "hits@10", "mape", "spearmanr", "auroc"]
_GOLDEN = []


def load():
    if not _GOLDEN:
        with open(GOLDEN, "rb") as f:
            _GOLDEN.append(torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False))
    return _GOLDEN[0]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def golden_graph(g, dev):
    from ultra_amd.data import Data
    rel = Data(edge_index=g["rel_edge_index"], edge_type=g["rel_edge_type"], num_nodes=g["num_relations"], num_relations=4)
    return Data(edge_index=g["edge_index"], edge_type=g["edge_type"], num_nodes=g["num_nodes"],
                num_relations=g["num_relations"], relation_graph=rel).to(dev)


def build_model(g, dev, logic="product"):
    from ultra_amd import models
    from ultra_amd.ultraquery import UltraQuery
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = UltraQuery(models.Ultra(**cfg), logic=logic)
    model.load_state_dict(g["weights"], strict=True)
    return model.to(dev).eval()


@pytest.mark.parametrize("logic", ["product", "godel", "lukasiewicz"])
@pytest.mark.parametrize("symbolic", [True, False])
def test_ultraquery_matches_reference_golden(dev, logic, symbolic):
    g = load()
    want = g["executor"][(logic, symbolic)]
    model = build_model(g, dev, logic)
    with torch.no_grad():
        logit = model(golden_graph(g, dev), g["query"].to(dev), symbolic_traversal=symbolic)
    prob = model.stack.stack[torch.arange(len(logit), device=dev), model.stack.SP].cpu()
    err = (prob - want["prob"]).abs()
    per_type = {g["id2type"][t]: float(err[g["type"] == t].max()) for t in range(len(g["id2type"]))}
    assert err.max().item() <= 1e-5, per_type
    assert torch.isfinite(logit).all()
    if symbolic:
        assert torch.equal(model.symbolic_stack.stack.cpu(), want["symbolic_stack"])
        assert torch.equal(model.symbolic_stack.SP.cpu(), want["symbolic_sp"])


def test_symbolic_traversal_kernel_on_golden_graph(dev):
    from ultra_amd.ultraquery import symbolic_traversal
    g = load()
    t = g["traversal"]
    ei, et = g["edge_index"].to(dev), g["edge_type"].to(dev)
    got = symbolic_traversal(ei, et, g["num_nodes"], t["h"].to(dev), t["r_index"].to(dev)).cpu()
    assert torch.equal(got, t["t"])
    got64 = symbolic_traversal(ei, et, g["num_nodes"], t["h"].double().to(dev), t["r_index"].to(dev)).cpu()
    assert torch.equal(got64, t["t64"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_symbolic_traversal_kernel_at_fb15k237_size(dev, dtype):
    """64 queries over the FB15k237-shaped graph: hub rows (thousands of in-edges of one relation), rows without an edge of
    the relation, one relation repeated across the batch, a relation without edges."""
    from ultra_amd.ultraquery import symbolic_traversal, symbolic_traversal_reference
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=1, relation_graph=False)
    ei, et = kg.edge_index.to(dev), kg.edge_type.to(dev)
    n = kg.num_nodes
    gen = torch.Generator().manual_seed(2)
    h = (torch.rand(64, n, generator=gen) * (torch.rand(64, n, generator=gen) < 0.3)).to(dtype)
    h[:8] = 1.0                                                    # dense sets: every hub edge counts
    r = torch.randint(0, kg.num_relations, (64,), generator=gen)
    hub_rel = kg.num_relations // 2                                # the inverse of the most frequent relation: into the hubs
    r[::5] = hub_rel
    r[1] = kg.num_relations + 3                                    # no edge at all
    h, r = h.to(dev), r.to(dev)
    got = symbolic_traversal(ei, et, n, h, r)
    want = symbolic_traversal_reference(ei, et, n, h, r)
    assert torch.equal(got, want)
    assert got[1].abs().sum().item() == 0
    indeg = torch.bincount(kg.edge_index[1][kg.edge_type == hub_rel], minlength=n)
    assert indeg.max().item() > 64, "the fixture must hold hub segments"


def _ranking_case(dev, pred, easy, hard, limit=None):
    from ultra_amd.query_eval import batch_evaluate, batch_evaluate_reference
    got = batch_evaluate(pred.to(dev), (None, easy.to(dev), hard.to(dev)), None if limit is None else limit.to(dev))
    want = batch_evaluate_reference(pred, (None, easy, hard), limit)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    return want


def test_answer_ranking_kernel_matches_restatement(dev):
    """FB15k237 N; quantised scores (many ties); an all-tied row; zero easy answers; queries with more answers than the LDS
    path holds; LDS-resident queries of 600 and 1900 answers; NaN scores; with and without restricted (-inf) nodes."""
    from ultra_amd import _lib
    n = synthetic.SHAPES["fb15k237"]["num_node"]
    gen = torch.Generator().manual_seed(7)
    B = 12
    pred = (torch.randn(B, n, generator=gen) * 4).round() / 4          # ~100 distinct values per row
    pred[3] = 0.5                                                       # all tied
    pred[4] = torch.randn(n, generator=gen)                             # tie-free
    easy = torch.rand(B, n, generator=gen) < 0.002
    hard = (torch.rand(B, n, generator=gen) < 0.002) & ~easy
    easy[5] = False                                                     # zero easy answers
    easy[6] = False
    hard[6] = False                                                     # no answer at all
    big = torch.randperm(n, generator=gen)[:_lib.RANKING_LDS_ANSWERS + 2000]
    easy[7] = False
    easy[7, big[:-40]] = True                                           # thousands of easy answers (global path)
    hard[7] = False
    hard[7, big[-40:]] = True
    hard[8] = False
    hard[8, big] = True                                                 # thousands of hard answers
    easy[8] = False
    mid = torch.randperm(n, generator=gen)
    easy[9], hard[9] = False, False
    easy[9, mid[:1500]] = True                                          # LDS path, several 256-answer scan chunks
    hard[9, mid[1500:1900]] = True
    easy[10], hard[10] = False, False
    easy[10, mid[:300]] = True
    hard[10, mid[300:600]] = True
    pred[11, ::97] = float("nan")                                       # NaN scores: above every number, as torch sorts
    pred[11, mid[:40]] = float("nan")
    hard[11, mid[:20]] = True
    easy[11, mid[20:30]] = True
    _ranking_case(dev, pred, easy, hard)
    limit = torch.randperm(n, generator=gen)[: n // 2].sort().values
    want = _ranking_case(dev, pred, easy, hard, limit)
    assert want[0].numel() > 0


@pytest.mark.parametrize("case", ["model", "random", "random_restricted"])
def test_answer_ranking_kernel_on_golden_cases(dev, case):
    """The golden cases (up to 900 answers a query, -inf ties under restrict_nodes) through the kernel: equal to the
    restatement, and to the reference's ranks wherever the hard answer's score is not tied."""
    c = load()["ranking"][case]
    want = _ranking_case(dev, c["pred"], c["easy_answer"], c["hard_answer"], c["limit_nodes"])
    tied = c["tied"]
    assert torch.equal(want[0][~tied], c["ranking"][~tied])


def test_test_queries_on_golden_set_matches_reference_metrics(dev):
    from ultra_amd.query_data import QueryDataset
    from ultra_amd.query_eval import test_queries
    g = load()
    ds = QueryDataset(g["nested"], g["type"].tolist(), [set(m.nonzero().flatten().tolist()) for m in g["easy_answer"]],
                      [set(m.nonzero().flatten().tolist()) for m in g["hard_answer"]], g["num_nodes"], g["id2type"])
    model = build_model(g, dev)
    got = test_queries(model, golden_graph(g, dev), ds, 8, g["id2type"], METRICS, device=dev)
    assert set(got) == set(g["metrics"])
    for k, v in g["metrics"].items():
        assert got[k] == pytest.approx(v, rel=1e-4, abs=1e-5), k
