"""QueryPredictor.answers / answer_sets(among=) on the GPU: one 1p, one 2i and one 2in query on a graph of 200
nodes, against the same predictor's full ranking (k = 200) restricted to the sets on the host, bit for bit."""
import pytest
import torch

from tests.test_ultraquery_gpu import build_model, load
from ultra_amd import query_predict, synthetic

pytestmark = pytest.mark.gpu

NODES = 200
QUERIES = [(3, (0,)), ((5, (1,)), (9, (2,))), ((7, (0,)), (11, (3, -2)))]        # 1p, 2i, 2in


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def served(dev):
    graph = synthetic.make_kg(num_node=NODES, num_triple=1200, num_relation_base=4, num_test=8, seed=17).to(dev)
    model = build_model(load(), dev)
    full = query_predict.QueryPredictor(model, graph, k=NODES, batch_size=4)
    return model, graph, full


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def restricted(full, allowed, k):
    ids, scores, _ = (t.cpu() for t in full)
    out_ids = torch.full((len(ids), k), -1, dtype=torch.long)
    out_scores = torch.full((len(ids), k), float("-inf"))
    count = torch.zeros(len(ids), dtype=torch.long)
    for b in range(len(ids)):
        keep = [j for j in range(ids.shape[1]) if int(ids[b, j]) in allowed[b]][:k]
        out_ids[b, :len(keep)], out_scores[b, :len(keep)], count[b] = ids[b, keep], scores[b, keep], len(keep)
    return out_ids, out_scores, count


@pytest.mark.parametrize("form", ["named", "shared", "per_query"])
def test_answers_among_equal_the_full_ranking_restricted(served, form):
    model, graph, full = served
    want_full = full.answers(QUERIES)
    assert int(want_full[2].min()) > 20          # (the entailed answers are left out; plenty of candidates stay)
    qp = query_predict.QueryPredictor(model, graph, k=10, batch_size=4)
    third = set(range(0, NODES, 3))
    if form == "named":
        qp.define_set("third", sorted(third))
        among, allowed = "third", [third] * 3
    elif form == "shared":
        among, allowed = torch.tensor(sorted(third)), [third] * 3
    else:
        qp.define_set("third", sorted(third))
        among, allowed = [[1, 5, 150, 199], "third", list(range(NODES))], [{1, 5, 150, 199}, third, set(range(NODES))]
    ids, scores, count = qp.answers(QUERIES, among=among)
    w_ids, w_scores, w_count = restricted(want_full, allowed, 10)
    assert torch.equal(ids.cpu(), w_ids) and same_bits(scores.cpu(), w_scores) and torch.equal(count.cpu(), w_count)


def test_answer_sets_among_equal_the_full_sets_restricted(served):
    model, graph, full = served
    qp = query_predict.QueryPredictor(model, graph, k=10, batch_size=4)
    third = set(range(0, NODES, 3))
    qp.define_set("third", sorted(third))
    allowed = [{1, 5, 150, 199}, third, set(range(NODES))]
    among = [[1, 5, 150, 199], "third", list(range(NODES))]
    for probability in (0.05, 0.5):
        out, ids, scores, size = (t.cpu() for t in qp.answer_sets(QUERIES, probability, among=among))
        w_out, w_ids, w_scores, w_size = (t.cpu() for t in full.answer_sets(QUERIES, probability))
        for b in range(3):
            keep = [j for j in range(int(w_out[b]), int(w_out[b + 1])) if int(w_ids[j]) in allowed[b]]
            assert ids[int(out[b]):int(out[b + 1])].tolist() == w_ids[keep].tolist()
            assert same_bits(scores[int(out[b]):int(out[b + 1])], w_scores[keep])
            assert len(keep) <= int(size[b]) <= min(int(w_size[b]), len(allowed[b]))
        assert int(size[2]) == int(w_size[2])           # every id listed: the parent's count
    with pytest.raises(KeyError):
        qp.answers(QUERIES, among="nope")
    with pytest.raises(ValueError):
        qp.answers(QUERIES, among=["third"])
