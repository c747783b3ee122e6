"""Serving link-prediction queries on the GPU: ultra_filtered_topk against the plain-torch restatement
(predict.filtered_topk_reference, itself pinned to a brute-force sort in tests/test_predict_cpu.py), and the Predictor
against the restatement applied to the model's scores.  Ids and counts compare with torch.equal, scores on their bits."""
import collections
import gc

import pytest
import torch

from tests.test_predict_cpu import random_known, special_mix
from ultra_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK = _lib.TOPK_CHUNK
SIZES = [1, 2, 63, 64, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 40 * CHUNK + 5]
KS = [1, 2, 10, 64, 255, 256]
PATTERNS = ["random", "quantised", "equal", "special", "ascending", "descending", "crowded"]
KNOWN = ["null", "empty", "random", "everything", "top-k", "one chunk"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_scores(pattern, batch, n, gen):
    if pattern == "random":
        return torch.randn(batch, n, generator=gen)
    if pattern == "quantised":      # five values: ties span chunk boundaries
        return torch.randint(-2, 3, (batch, n), generator=gen).float() / 2
    if pattern == "equal":
        return torch.full((batch, n), 0.25)
    if pattern == "special":
        pred = special_mix((batch, n), gen)
        bits = pred.view(torch.int32)
        u = torch.rand(batch, n, generator=gen)
        bits[u < 0.02] = 0x7fc12345                 # NaNs with a payload, of either sign: they tie with every other NaN
        bits[(u >= 0.02) & (u < 0.04)] = -4194303   # 0xffc00001
        pred[(u >= 0.04) & (u < 0.06)] = float("inf")
        return pred
    if pattern == "crowded":        # the winners sit 256 ids apart: in the slots of one thread of the selection
        pred = torch.randn(batch, n, generator=gen)
        pred[:, 3::256] += 100.0
        return pred
    ramp = torch.arange(n, dtype=torch.float32).unsqueeze(0) + torch.arange(batch, dtype=torch.float32).unsqueeze(1)
    return ramp if pattern == "ascending" else -ramp      # ascending: the winners sit in the last chunk


def lists_of(rows):
    ptr = torch.zeros(len(rows) + 1, dtype=torch.long)
    ptr[1:] = torch.tensor([len(r) for r in rows]).cumsum(0)
    return ptr, torch.cat(rows)


def make_known(kind, batch, n, gen, top=None):
    """(ptr, index) on the CPU; None, None for the NULL filter."""
    if kind == "null":
        return None, None
    if kind == "empty":
        return torch.zeros(batch + 1, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    if kind == "random":
        return random_known(batch, n, 0.3, gen)
    if kind == "everything":        # count 0, an all-padding row
        return lists_of([torch.arange(n) for _ in range(batch)])
    if kind == "top-k":             # exactly the ids of the unfiltered answer
        return lists_of([row[row >= 0].sort().values for row in top])
    lo = ((n + CHUNK - 1) // CHUNK // 2) * CHUNK       # all of one chunk (the middle one)
    return lists_of([torch.arange(lo, min(n, lo + CHUNK)) for _ in range(batch)])


def cut(ref, k):
    """The answer for a smaller k from the restatement's answer for ULTRA_TOPK_MAX: a prefix, by definition."""
    ids, scores, count = ref
    return ids[:, :k], scores[:, :k], count.clamp(max=k)


def assert_same(got, want):
    ids, scores, count = (t.cpu() for t in got)
    assert torch.equal(ids, want[0])
    assert torch.equal(count, want[2])
    assert torch.equal(scores.view(torch.int32), want[1].contiguous().view(torch.int32))


def on(dev, *tensors):
    return [None if t is None else t.to(dev) for t in tensors]


@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement(dev, n, pattern, batch):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(1000 * batch + n)
    pred = make_scores(pattern, batch, n, gen)
    g_pred = pred.to(dev)
    unfiltered = predict.filtered_topk_reference(pred, _lib.TOPK_MAX)
    for kind in KNOWN:
        if kind == "top-k":
            continue
        ptr, index = make_known(kind, batch, n, gen)
        ref = unfiltered if kind in ("null", "empty") else predict.filtered_topk_reference(pred, _lib.TOPK_MAX, ptr, index)
        g_ptr, g_index = on(dev, ptr, index)
        for k in KS:        # (including k > n)
            got = predict.filtered_topk(g_pred, k, g_ptr, g_index)
            assert_same(got, cut(ref, k))
            if pattern == "equal" and kind in ("null", "empty"):
                m = min(k, n)
                assert got[0][:, :m].cpu().tolist() == [list(range(m))] * batch
    for k in KS:            # the first k winners knocked out: the answer is the next k
        ptr, index = make_known("top-k", batch, n, gen, top=unfiltered[0][:, :k])
        ref = predict.filtered_topk_reference(pred, k, ptr, index)
        g_ptr, g_index = on(dev, ptr, index)
        assert_same(predict.filtered_topk(g_pred, k, g_ptr, g_index), ref)
        assert int((ref[2] - (n - (ptr[1:] - ptr[:-1])).clamp(max=k)).abs().max()) == 0


def test_all_equal_scores_return_the_first_ids_that_are_not_known(dev):
    from ultra_amd import predict
    n, batch, k = 2 * CHUNK + 3, 3, 64
    gen = torch.Generator().manual_seed(5)
    pred = torch.full((batch, n), -1.5)
    ptr, index = random_known(batch, n, 0.3, gen)
    ids, scores, count = predict.filtered_topk(pred.to(dev), k, ptr.to(dev), index.to(dev))
    for b in range(batch):
        known = set(index[int(ptr[b]):int(ptr[b + 1])].tolist())
        assert ids[b].cpu().tolist() == [i for i in range(n) if i not in known][:k]
    assert count.cpu().tolist() == [k] * batch and bool((scores == -1.5).all())


@pytest.mark.parametrize("n,k", [(65, 10), (CHUNK + 1, 256), (40 * CHUNK + 5, 64)])
def test_the_same_call_twice_gives_the_same_bits(dev, n, k):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(n)
    pred = special_mix((8, n), gen).to(dev)
    ptr, index = on(dev, *random_known(8, n, 0.3, gen))
    first = predict.filtered_topk(pred, k, ptr, index)
    for _ in range(3):
        again = predict.filtered_topk(pred, k, ptr, index)
        assert_same(again, [t.cpu() for t in first])


@pytest.mark.parametrize("n", [257, 2 * CHUNK + 3])
def test_a_captured_call_replayed_on_fresh_inputs_equals_the_eager_call(dev, n):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(n)
    batch, k = 8, 10
    ptr0, index0 = random_known(batch, n, 0.3, gen)
    pred = torch.randn(batch, n, generator=gen).to(dev)
    ptr = ptr0.to(dev)
    index = torch.zeros(batch * n, dtype=torch.long, device=dev)
    index[:index0.numel()] = index0.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        predict.filtered_topk(pred, k, ptr, index)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = predict.filtered_topk(pred, k, ptr, index)
    for _ in range(2):
        fresh = special_mix((batch, n), gen)
        ptr1, index1 = random_known(batch, n, 0.3, gen)
        pred.copy_(fresh.to(dev))
        ptr.copy_(ptr1.to(dev))
        index[:index1.numel()] = index1.to(dev)
        graph.replay()
        eager = predict.filtered_topk(pred, k, ptr, index)
        assert_same(out, [t.cpu() for t in eager])
        assert_same(out, predict.filtered_topk_reference(fresh, k, ptr1, index1))


# ---- model level: the setting of tests/test_eval_gpu.py ----

@pytest.fixture(scope="module")
def served(dev):
    """(model, data, triples, {mode: (scores, ptr, index)}): the golden ultra_3g weights on a 400-node graph, the scores of
    its 21 test queries in both directions (batches of 8, 8 and 5) and the known lists of the filter graph, computed once."""
    from tests.test_oracle_model import load_golden
    from ultra_amd import models, predict, synthetic, tasks
    _, state, _, cfg = load_golden("ultra_3g", "sum")
    data = synthetic.make_kg(num_node=400, num_triple=3000, num_relation_base=5, num_test=21, seed=3).to(dev)
    model = models.Ultra(**cfg)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    triples = torch.cat([data.target_edge_index, data.target_edge_type.unsqueeze(0)]).t().contiguous()
    t_pred, h_pred = [], []
    with torch.no_grad():
        for s in range(0, len(triples), 8):
            t_batch, h_batch = tasks.all_negative(data, triples[s:s + 8])
            t_pred.append(model(data, t_batch).float())
            h_pred.append(model(data, h_batch).float())
    ref = {"tail": (torch.cat(t_pred).cpu(),) + tuple(t.cpu() for t in predict.known_answers(data, triples[:, 0], triples[:, 2], "tail")),
           "head": (torch.cat(h_pred).cpu(),) + tuple(t.cpu() for t in predict.known_answers(data, triples[:, 1], triples[:, 2], "head"))}
    return model, data, triples, ref


def test_predictor_equals_the_restatement_on_the_models_scores(dev, served):
    from ultra_amd import predict
    model, data, triples, ref = served
    for use_graph in (True, False):
        predictor = predict.Predictor(model, data, k=10, batch_size=8, use_graph=use_graph)
        for _ in range(2):      # (the second call reuses the captures)
            assert_same(predictor.tails(triples[:, 0], triples[:, 2]), predict.filtered_topk_reference(ref["tail"][0], 10, *ref["tail"][1:]))
            assert_same(predictor.heads(triples[:, 1], triples[:, 2]), predict.filtered_topk_reference(ref["head"][0], 10, *ref["head"][1:]))
        assert len(predictor._steps) == (2 if use_graph else 0)
        # a single query, and none at all
        assert_same(predictor.tails(triples[:1, 0], triples[:1, 2]),
                    predict.filtered_topk_reference(ref["tail"][0][:1], 10, ref["tail"][1][:2], ref["tail"][2]))
        empty = predictor.heads(triples[:0, 1], triples[:0, 2])
        assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10) and empty[2].shape == (0,)


def test_unfiltered_predictor_returns_the_raw_topk(dev, served):
    from ultra_amd import predict
    model, data, triples, ref = served
    for use_graph in (True, False):
        predictor = predict.Predictor(model, data, k=256, batch_size=8, filtered=False, use_graph=use_graph)
        assert_same(predictor.tails(triples[:, 0], triples[:, 2]), predict.filtered_topk_reference(ref["tail"][0], 256))
        assert_same(predictor.heads(triples[:, 1], triples[:, 2]), predict.filtered_topk_reference(ref["head"][0], 256))


def test_position_in_the_list_against_the_filtered_rank(dev, served):
    """Filtered with the known answers minus the positive, the positive's 0-based position p in a k = 256 list satisfies
    p + 1 <= filtered rank (ties count against the positive in the rank, by id in the list), with equality where the row's
    scores are distinct; a positive that is not among the 256 has a rank beyond them."""
    from ultra_amd import predict, tasks
    model, data, triples, ref = served
    for mode, col in (("tail", 1), ("head", 0)):
        pred, ptr, index = ref[mode]
        rows = []
        for b in range(len(triples)):
            rows.append(torch.tensor([i for i in index[int(ptr[b]):int(ptr[b + 1])].tolist() if i != int(triples[b, col])],
                                     dtype=torch.long))
        p_ptr, p_index = lists_of(rows)
        g_pred = pred.to(dev)
        ids, _, count = predict.filtered_topk(g_pred, 256, p_ptr.to(dev), p_index.to(dev))
        rank, num_neg = tasks.filtered_ranking(data, triples, g_pred, mode=mode)
        ids, rank = ids.cpu(), rank.cpu()
        assert torch.equal(count.cpu(), (num_neg.cpu() + 1).clamp(max=256))
        for b in range(len(triples)):
            where = (ids[b] == triples[b, col].cpu()).nonzero().flatten()
            if where.numel() == 0:
                assert int(rank[b]) > 256
                continue
            assert where.numel() == 1
            p = int(where[0])
            assert p + 1 <= int(rank[b])
            if pred[b].unique().numel() == pred.shape[1]:
                assert p + 1 == int(rank[b])


def test_no_plan_stays_pinned_after_the_predictor_is_gone(dev, served, monkeypatch):
    from ultra_amd import predict, rspmm
    model, data, triples, _ = served
    pins = collections.Counter()
    plain_pin = rspmm.Plan.pin

    def counting_pin(self, delta=1):
        pins[id(self)] += delta
        return plain_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_pin)
    predictor = predict.Predictor(model, data, k=10, batch_size=8)
    predictor.tails(triples[:, 0], triples[:, 2])
    predictor.heads(triples[:, 1], triples[:, 2])
    assert pins and all(v > 0 for v in pins.values())       # the captures hold their plans ...
    del predictor
    gc.collect()
    assert all(v == 0 for v in pins.values())               # ... and let go of them

    # a capture that fails leaves nothing pinned either
    pins.clear()

    def no_graph(*args, **kwargs):
        raise RuntimeError("capture refused")
    monkeypatch.setattr(torch.cuda, "CUDAGraph", no_graph)
    predictor = predict.Predictor(model, data, k=10, batch_size=8)
    with pytest.raises(RuntimeError, match="capture refused"):
        predictor.tails(triples[:, 0], triples[:, 2])
    assert pins and all(v == 0 for v in pins.values())
    assert predictor._steps == {}


def test_a_model_outside_the_fused_path_is_served_without_a_capture(dev, served, monkeypatch):
    """models.NotOnFusedPath from the capture: the predictor runs batch by batch instead, with the same answers as
    use_graph=False, and keeps no capture and no pinned plan."""
    from ultra_amd import dense, predict, rspmm
    model, data, triples, _ = served
    pins = collections.Counter()
    plain_pin = rspmm.Plan.pin

    def counting_pin(self, delta=1):
        pins[id(self)] += delta
        return plain_pin(self, delta)
    monkeypatch.setattr(rspmm.Plan, "pin", counting_pin)
    monkeypatch.setattr(dense, "readout_supported", lambda *args, **kwargs: False)      # (the generic readout: not captured)
    want = predict.Predictor(model, data, k=10, batch_size=8, use_graph=False).heads(triples[:, 1], triples[:, 2])
    predictor = predict.Predictor(model, data, k=10, batch_size=8)
    for _ in range(2):
        assert_same(predictor.heads(triples[:, 1], triples[:, 2]), [t.cpu() for t in want])
    assert predictor._eager_only and predictor._steps == {}
    assert all(v == 0 for v in pins.values())
