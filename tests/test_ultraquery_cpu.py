"""Complex logical queries on the CPU: the postfix encoding, the stack, and the torch restatements of symbolic traversal and
answer ranking against the reference's recorded outputs (tests/golden/gen_ultraquery_golden.py, ultraquery.pt.xz); evaluate()
against the reference's metrics; a gloo world-2 test_queries run against world 1.

The restatements are the contracts the HIP kernels are held to bit for bit and integer for integer
(tests/test_ultraquery_gpu.py).  On hard answers whose score ties another node's, the reference's rank follows its unstable
argsort; there the restatement's rank must lie in the tie block's [optimistic, pessimistic] range."""
import io
import lzma
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz")
METRICS = ["mrr", "hits@1", "hits@3", "hits@10", "mape", "spearmanr", "auroc"]
_GOLDEN = []


def load():
    if not _GOLDEN:
        with open(GOLDEN, "rb") as f:
            _GOLDEN.append(torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False))
    return _GOLDEN[0]


def test_from_nested_matches_reference_postfix_for_all_structures():
    from ultra_amd.query_data import ID2TYPE
    from ultra_amd.ultraquery import Query
    g = load()
    assert sorted(set(g["id2type"])) == ID2TYPE and len(ID2TYPE) == 14
    assert sorted(set(g["type"].tolist())) == list(range(14))
    for nested, want in zip(g["nested"], g["reference_postfix"]):
        assert Query.from_nested(nested).tolist() == want
    with pytest.raises(ValueError):
        Query.from_nested(g["nested"][0], binary_op=False)


def test_query_predicates_and_readable():
    from ultra_amd.ultraquery import Query
    q = Query.from_nested(((5, (1,)), (7, (2, -2))))          # 2in
    assert q.is_operand().tolist() == [True, False, True, False, False, False, False]
    assert q.is_projection().sum().item() == 2 and q.is_negation().sum().item() == 1
    assert q.is_intersection()[5].item() and q.is_stop()[-1].item()
    assert q[5].get_operand().item() == 2 and q[1].get_operand().item() == 1
    assert q.get_operation()[5].item() == Query.intersection
    assert q.to_readable() == "A <- projection_1(5)\nB <- projection_2(7)\nC <- negation(B)\nD <- intersection(A, C)"


def test_stack_overflow_and_underflow_raise():
    from ultra_amd.ultraquery import Stack
    s = Stack(3, 2, 4)
    everyone = torch.ones(3, dtype=torch.bool)
    some = torch.tensor([True, False, True])
    s.push(everyone, torch.ones(3, 4))
    s.push(some, torch.full((2, 4), 2.0))
    with pytest.raises(ValueError, match="overflow"):
        s.push(some, torch.zeros(2, 4))
    assert s.pop(some).tolist() == [[2.0] * 4] * 2
    assert s.pop().tolist() == [[1.0] * 4] * 3
    with pytest.raises(ValueError, match="underflow"):
        s.pop(some)


def test_ultraquery_refuses_training_mode():
    from torch import nn

    from ultra_amd.ultraquery import UltraQuery
    model = UltraQuery(nn.Module())
    model.train()
    with pytest.raises(NotImplementedError, match="traversal dropout"):
        model(None, torch.zeros(1, 3, dtype=torch.long))


def test_symbolic_traversal_restatement_matches_reference():
    from ultra_amd.ultraquery import symbolic_traversal_reference
    g = load()
    t = g["traversal"]
    got = symbolic_traversal_reference(g["edge_index"], g["edge_type"], g["num_nodes"], t["h"], t["r_index"])
    assert torch.equal(got, t["t"])
    got64 = symbolic_traversal_reference(g["edge_index"], g["edge_type"], g["num_nodes"], t["h"].double(), t["r_index"])
    assert got64.dtype == torch.float64 and torch.equal(got64, t["t64"])
    # and the final symbolic stacks of the executor are made of these steps: every entry is exactly 0 or 1 for product logic
    st = g["executor"][("product", True)]["symbolic_stack"]
    assert bool(((st == 0) | (st == 1)).all())


def tie_bounds(pred, easy, hard, limit=None):
    """Per hard answer (list order): the optimistic and pessimistic filtered rank over its tie block."""
    if limit is not None:
        keep = torch.zeros(pred.shape[1], dtype=torch.bool)
        keep[limit] = True
        pred = pred.masked_fill(~keep, float("-inf"))
    lo, hi = [], []
    for b in range(pred.shape[0]):
        other = ~(easy[b] | hard[b])
        for a in hard[b].nonzero().flatten().tolist():
            p = pred[b, a]
            lo.append(1 + int((other & (pred[b] > p)).sum()))
            hi.append(1 + int((other & (pred[b] >= p)).sum()))
    return torch.tensor(lo, dtype=torch.long), torch.tensor(hi, dtype=torch.long)


@pytest.mark.parametrize("case", ["model", "random", "random_restricted"])
def test_ranking_restatement_matches_reference(case):
    from ultra_amd.query_eval import batch_evaluate
    c = load()["ranking"][case]
    pred = c["pred"].clone()
    ranking, answer_ranking = batch_evaluate(pred, (None, c["easy_answer"], c["hard_answer"]), c["limit_nodes"])
    assert torch.equal(pred, c["pred"]), "batch_evaluate must not modify pred"
    assert ranking.shape == c["ranking"].shape and answer_ranking.shape == c["answer_ranking"].shape
    tied = c["tied"]
    assert torch.equal(ranking[~tied], c["ranking"][~tied])
    lo, hi = tie_bounds(c["pred"], c["easy_answer"], c["hard_answer"], c["limit_nodes"])
    assert bool(((ranking >= lo) & (ranking <= hi)).all())
    assert bool(((c["ranking"] >= lo) & (c["ranking"] <= hi)).all())
    if case == "random_restricted":
        assert tied.any(), "the restricted case must exercise -inf ties"
    # unfiltered positions: exact wherever the answer's score is unique in its row
    p = c["pred"]
    if c["limit_nodes"] is not None:
        keep = torch.zeros(p.shape[1], dtype=torch.bool)
        keep[c["limit_nodes"]] = True
        p = p.masked_fill(~keep, float("-inf"))
    sample, col = torch.cat([c["easy_answer"], c["hard_answer"]], -1).nonzero().t()
    ent = col % p.shape[1]
    unique = (p[sample] == p[sample, ent].unsqueeze(1)).sum(1) == 1
    assert torch.equal(answer_ranking[unique], c["answer_ranking"][unique])


def test_ranking_rejects_overlapping_answer_sets():
    from ultra_amd.query_eval import batch_evaluate
    easy = torch.zeros(1, 5, dtype=torch.bool)
    easy[0, 2] = True
    with pytest.raises(ValueError, match="disjoint"):
        batch_evaluate(torch.zeros(1, 5), (None, easy, easy.clone()))


def test_evaluate_matches_reference_metrics():
    """The metrics run_query.py reports: gather_results (num_pred truncated to int64, at every world size), then evaluate."""
    from ultra_amd.query_eval import evaluate, gather_results
    g = load()
    c = g["ranking"]["model"]
    pred, target = gather_results((c["ranking"], g["num_pred"]),
                                  (g["type"], c["answer_ranking"], g["easy_answer"].sum(-1), g["hard_answer"].sum(-1)))
    assert pred[1].dtype == torch.int64 and torch.equal(pred[1], g["gathered_num_pred"])
    got = evaluate(pred, target, METRICS, g["id2type"])
    assert set(got) == set(g["metrics"])
    for k, v in g["metrics"].items():
        assert got[k] == pytest.approx(v, rel=1e-5, abs=1e-6), k


class GoldenLogits(object):
    """A stand-in model: the golden executor's logits of every query, looked up by its postfix row."""

    def __init__(self, g):
        self.rows = {tuple(q.tolist()): i for i, q in enumerate(g["query"])}
        self.logit = g["executor"][("product", False)]["logit"]

    def __call__(self, graph, query, symbolic_traversal=True):
        return self.logit[[self.rows[tuple(q.tolist())] for q in query.as_subclass(torch.Tensor)]]


def _queries(g):
    from ultra_amd.query_data import QueryDataset
    ds = QueryDataset(g["nested"], g["type"].tolist(), [set(m.nonzero().flatten().tolist()) for m in g["easy_answer"]],
                      [set(m.nonzero().flatten().tolist()) for m in g["hard_answer"]], g["num_nodes"], g["id2type"])
    return ds


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ultra_amd.query_eval import test_queries
    g = load()
    res = test_queries(GoldenLogits(g), None, _queries(g), 4, g["id2type"], METRICS)
    torch.save(res, os.path.join(out_dir, "r%d.pt" % rank))
    dist.monitored_barrier()
    dist.destroy_process_group()


def test_test_queries_world_two_equals_world_one(tmp_path):
    from ultra_amd.query_eval import test_queries
    g = load()
    assert len(g["query"]) % 2 == 0     # (DistributedSampler pads an odd count with a repeated query)
    one = test_queries(GoldenLogits(g), None, _queries(g), 4, g["id2type"], METRICS)
    for k, v in g["metrics"].items():
        assert one[k] == pytest.approx(v, rel=1e-5, abs=1e-6), k
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        two = torch.load(os.path.join(tmp_path, "r%d.pt" % r))
        assert set(two) == set(one)
        for k in one:
            assert two[k] == pytest.approx(one[k], rel=1e-6, abs=1e-7), k
