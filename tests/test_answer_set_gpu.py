"""Serving answer sets on the GPU: ultra_filtered_above against the plain-torch restatement (predict.filtered_above_reference,
itself pinned to a brute-force sort in tests/test_answer_set_cpu.py), QueryPredictor.answer_sets against the restatement
applied to the executor's logits, and Predictor.tails_above / heads_above against the restatement applied to the model's
scores.  Offsets, sizes and ids compare with torch.equal, scores on their bits."""
import pytest
import torch

from tests.test_predict_cpu import random_known, special_mix
from tests.test_predict_gpu import PATTERNS, make_known, make_scores, on, served  # noqa: F401  (served: a fixture)
from tests.test_query_exec_cpu import load
from tests.test_ultraquery_gpu import build_model, golden_graph
from ultra_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK = _lib.TOPK_CHUNK
INF = float("inf")
SIZES = [1, 2, 63, 64, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 5 * CHUNK + 5, 40 * CHUNK + 5]
KNOWN = ["null", "empty", "random", "everything", "one chunk"]
BELOW_A_QUARTER = float(torch.nextafter(torch.tensor(0.25), torch.tensor(-INF)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def thresholds_of(pattern, pred):
    """[(threshold, expectation)]: expectation "empty" / "everything" where the lists are known beforehand, else None."""
    finite = pred[0][torch.isfinite(pred[0])]
    median = float(finite.median()) if finite.numel() else 0.0
    has_inf = bool((pred == INF).any())
    out = [(-INF, None), (0.0, None), (median, None), (3e38, None if has_inf else "empty")]
    if pattern == "quantised":
        out += [(0.5, None), (-1.0, None), (1.0, "empty")]       # thresholds that equal stored scores
    if pattern == "equal":
        out += [(0.25, "empty"), (BELOW_A_QUARTER, "everything")]
    return out


def assert_same(got, want):
    """got: (ptr, ids, scores, size) with full-capacity ids / scores; want: the restatement's (on the CPU)."""
    ptr, ids, scores, size = (t.cpu() for t in got)
    assert torch.equal(ptr, want[0])
    assert torch.equal(size, want[3])
    total = int(ptr[-1])
    assert torch.equal(ids[:total], want[1])
    assert torch.equal(scores[:total].view(torch.int32), want[2].contiguous().view(torch.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,batch", [(n, batch) for batch in (1, 3, 8) for n in SIZES
                                     if not (n == 40 * CHUNK + 5 and batch == 8)])      # (six merge levels: batch 1 and 3)
def test_kernel_equals_the_restatement(dev, n, batch, pattern):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(1000 * batch + n)
    pred = make_scores(pattern, batch, n, gen)
    g_pred = pred.to(dev)
    cases = thresholds_of(pattern, pred)
    for kind in KNOWN:
        ptr, index = make_known(kind, batch, n, gen)
        g_ptr, g_index = on(dev, ptr, index)
        for threshold, expect in cases:
            want = predict.filtered_above_reference(pred, threshold, ptr, index)
            got = predict.filtered_above(g_pred, threshold, g_ptr, g_index)
            assert got[1].shape == got[2].shape == (batch * n,)
            assert_same(got, want)
            if expect == "empty":
                assert want[0].tolist() == [0] * (batch + 1) and want[3].tolist() == [0] * batch
            if expect == "everything":
                assert want[3].tolist() == [n] * batch
                if kind in ("null", "empty"):
                    assert got[1].cpu().tolist() == list(range(n)) * batch
                if kind == "everything":
                    assert want[0].tolist() == [0] * (batch + 1)


def raw_call(pred, threshold, ptr, index, fill):
    """The C entry point on buffers the test owns: outputs pre-filled with 0xFF bytes, the workspace with `fill` (a byte value or
    a generator for random bytes)."""
    dev = pred.device
    batch, n = pred.shape
    ff = lambda count: torch.full((count * 8,), 0xFF, dtype=torch.uint8, device=dev)      # noqa: E731
    out_ptr, size = ff(batch + 1).view(torch.long), ff(batch).view(torch.long)
    ids = ff(batch * n).view(torch.long)
    scores = torch.full((batch * n * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32)
    need = _lib.lib.ultra_filtered_above_workspace(batch, n)
    assert need > 0 and need % 8 == 0
    if isinstance(fill, int):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
    else:
        ws = torch.randint(0, 256, (need,), generator=fill, dtype=torch.uint8).to(dev)
    _lib.check(_lib.lib.ultra_filtered_above(pred.data_ptr(), None if ptr is None else ptr.data_ptr(),
                                             None if ptr is None else index.data_ptr(), batch, n, threshold, out_ptr.data_ptr(),
                                             ids.data_ptr(), scores.data_ptr(), ids.numel(), size.data_ptr(), ws.data_ptr(), need,
                                             _lib.stream_of(dev)))
    return out_ptr, ids, scores, size


@pytest.mark.parametrize("n", [65, CHUNK + 1, 5 * CHUNK + 5])
def test_prefilled_outputs_are_all_written_and_the_workspace_contents_do_not_matter(dev, n):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(n)
    batch = 3
    pred = special_mix((batch, n), gen)
    ptr, index = random_known(batch, n, 0.3, gen)
    want = predict.filtered_above_reference(pred, -0.5, ptr, index)
    assert int(want[0][-1]) > 0
    g_pred, g_ptr, g_index = on(dev, pred, ptr, index)
    for fill in (0xFF, 0x00, gen):
        got = raw_call(g_pred, -0.5, g_ptr, g_index, fill)
        assert_same(got, want)      # (an entry left unwritten would read id -1 and a NaN's bits)


@pytest.mark.parametrize("n", [65, CHUNK + 1, 40 * CHUNK + 5])
def test_the_same_call_twice_gives_the_same_bits(dev, n):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(n)
    batch = 3
    pred = special_mix((batch, n), gen).to(dev)
    ptr, index = on(dev, *random_known(batch, n, 0.3, gen))
    first = [t.cpu() for t in predict.filtered_above(pred, -0.5, ptr, index)]
    total = int(first[0][-1])
    for _ in range(3):
        again = [t.cpu() for t in predict.filtered_above(pred, -0.5, ptr, index)]
        assert torch.equal(again[0], first[0]) and torch.equal(again[3], first[3])
        assert torch.equal(again[1][:total], first[1][:total])
        assert torch.equal(again[2][:total].view(torch.int32), first[2][:total].view(torch.int32))


@pytest.mark.parametrize("n", [257, 5 * CHUNK + 5])
def test_a_captured_call_replayed_on_fresh_scores_equals_the_restatement(dev, n):
    from ultra_amd import predict
    gen = torch.Generator().manual_seed(n)
    batch = 3
    ptr0, index0 = random_known(batch, n, 0.3, gen)
    pred = torch.randn(batch, n, generator=gen).to(dev)
    ptr = ptr0.to(dev)
    index = torch.zeros(batch * n, dtype=torch.long, device=dev)
    index[:index0.numel()] = index0.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        predict.filtered_above(pred, 0.0, ptr, index)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = predict.filtered_above(pred, 0.0, ptr, index)
    for _ in range(2):      # the lengths of the lists change from replay to replay
        fresh = special_mix((batch, n), gen)
        ptr1, index1 = random_known(batch, n, 0.3, gen)
        pred.copy_(fresh.to(dev))
        ptr.copy_(ptr1.to(dev))
        index[:index1.numel()] = index1.to(dev)
        graph.replay()
        assert_same(out, predict.filtered_above_reference(fresh, 0.0, ptr1, index1))


def test_bad_arguments_raise_before_anything_is_launched(dev):
    from ultra_amd import predict
    pred = torch.zeros(2, 5, device=dev)
    ptr = torch.zeros(3, dtype=torch.long, device=dev)
    index = torch.zeros(0, dtype=torch.long, device=dev)
    for bad in (float("nan"), INF, 1e39):
        with pytest.raises(ValueError):
            predict.filtered_above(pred, bad)
    with pytest.raises(TypeError):
        predict.filtered_above(pred, "0")
    with pytest.raises(TypeError):
        predict.filtered_above(pred.double(), 0.0)
    with pytest.raises(TypeError):
        predict.filtered_above(pred[0], 0.0)
    with pytest.raises(ValueError):
        predict.filtered_above(pred, 0.0, ptr[:2], index)
    with pytest.raises(ValueError):
        predict.filtered_above(pred, 0.0, ptr.int(), index)
    with pytest.raises(ValueError):
        predict.filtered_above(pred, 0.0, ptr.cpu(), index.cpu())
    with pytest.raises(ValueError):
        predict.filtered_above(torch.zeros(2, 0, device=dev), 0.0)
    out_ptr, ids, scores, size = predict.filtered_above(torch.zeros(0, 5, device=dev), 0.0)      # no rows: nothing to do
    assert out_ptr.tolist() == [0] and ids.numel() == scores.numel() == size.numel() == 0


# ---- QueryPredictor.answer_sets on the golden UltraQuery model ----

@pytest.mark.parametrize("filtered", [True, False])
def test_answer_sets_equal_the_restatement_on_the_executors_logits(dev, filtered):
    from ultra_amd import predict, query_exec, query_predict
    g = load()
    model, graph = build_model(g, dev), golden_graph(g, dev)
    order = torch.randperm(2 * len(g["nested"]), generator=torch.Generator().manual_seed(5)).tolist()
    nested = [g["nested"][i % len(g["nested"])] for i in order]            # two of every type, mixed
    n = len(nested)
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=4, filtered=filtered)
    runs = []
    for index, program in qp._programs(nested):
        with torch.no_grad():
            logits, sym = query_exec.execute(model, graph, program, symbolic_traversal=filtered)
        runs.append((index, logits.cpu(), None if sym is None else sym.cpu()))
    assert [index for index, _, _ in runs] == qp.batches(nested)
    for probability in (0.5, 0.9):
        threshold = predict.logit_threshold(probability)
        want = [None] * n
        for index, logits, sym in runs:
            for row, i in enumerate(index):
                known = (sym[row] != 0).nonzero().flatten() if filtered else None
                want[i] = predict.filtered_above_reference(logits[row:row + 1], threshold,
                                                           None if known is None else torch.tensor([0, len(known)]), known)
        ptr, ids, scores, size = (t.cpu() for t in qp.answer_sets(nested, probability=probability))
        assert ptr.shape == (n + 1,) and int(ptr[0]) == 0 and ids.shape == scores.shape == (int(ptr[-1]),)
        for i in range(n):
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            assert torch.equal(ids[lo:hi], want[i][1]), i
            assert torch.equal(scores[lo:hi].view(torch.int32), want[i][2].view(torch.int32)), i
            assert int(size[i]) == int(want[i][3][0]), i
    assert not model.training


# ---- Predictor.tails_above / heads_above on the graph of tests/test_predict_gpu.py ----

def test_predictor_sets_equal_the_restatement_on_the_models_scores(dev, served):  # noqa: F811
    from ultra_amd import predict
    model, data, triples, ref = served
    assert len(triples) % 8 != 0        # the last batch is a short one
    for filtered in (True, False):
        predictor = predict.Predictor(model, data, k=10, batch_size=8, filtered=filtered)
        for mode, col in (("tail", 0), ("head", 1)):
            pred, ptr, index = ref[mode]
            if not filtered:
                ptr = index = None
            call = predictor.tails_above if mode == "tail" else predictor.heads_above
            for min_score in (float(pred.median()), -INF, float(pred.max())):
                want = predict.filtered_above_reference(pred, min_score, ptr, index)
                got = [t.cpu() for t in call(triples[:, col], triples[:, 2], min_score)]
                assert got[1].shape == got[2].shape == (int(want[0][-1]),)
                assert_same(got, want)
        # a single query, and none at all
        pred, ptr, index = ref["tail"]
        one = predictor.tails_above(triples[:1, 0], triples[:1, 2], float(pred.median()))
        assert_same([t.cpu() for t in one],
                    predict.filtered_above_reference(pred[:1], float(pred.median()), ptr[:2] if filtered else None, index))
        none = predictor.heads_above(triples[:0, 1], triples[:0, 2], 0.0)
        assert none[0].tolist() == [0] and none[1].numel() == none[2].numel() == none[3].numel() == 0
    with pytest.raises(ValueError):
        predictor.tails_above(triples[:, 0], triples[:, 2], float("nan"))
