"""Retiring entities on the GPU: the ultra_filtered_*_alive entries against the `retired=` restatements -- ids,
score bits, counts, ptr, size, rank, num_negative, bit for bit --, one recorded hipGraph serving a later retirement, and
Predictor.remove_entities end to end against the definition: a fresh Predictor on materialized(), asked for k + num_retired
answers, the retired ids dropped."""
import os

import pytest
import torch

from ultra_amd import _lib, models, predict, synthetic, tasks
from ultra_amd import data as udata
from ultra_amd.live import retired_words

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ALIVE_SYMBOLS = ("ultra_filtered_topk_alive", "ultra_filtered_above_alive", "ultra_filtered_rank_alive")
LIVE_SYMBOLS = ("ultra_filtered_topk_live", "ultra_filtered_above_live", "ultra_filtered_rank_live")
PARENT_SYMBOLS = ("ultra_filtered_topk", "ultra_filtered_above", "ultra_filtered_rank")

# one partial chunk with a partial last word; a chunk edge (one chunk and five candidates); three chunks
N_CANDS, BATCH, N_MAX = (70, 4101, 8200), 3, 8200
KS = (1, 10, 256)
THRESHOLD = 0.25
OTHERS = (8, -5)        # the two ids beside the lists' that the "all but" set leaves alive: 8 and live - 5
LIVES = tuple(n - reserve for n in N_CANDS for reserve in (0, 7))
# every id some "all but" set leaves alive: row 1 of the scores holds -1.0 there, so its answer set is empty then
LEFT_ALIVE = sorted({1, 2, 5, 7, 8, 33, 40, 60, 4094, 4097, 8000} | {live - d for live in LIVES for d in (2, 5)})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want):
    return len(got) == len(want) and all(x.shape == y.shape and torch.equal(bits(x), bits(y)) for x, y in zip(got, want))


@pytest.fixture(scope="module")
def scores(dev):
    """(BATCH, N_MAX) scores from {-1, -.5, 0, .5, 1} with NaN, -inf, +inf and -0.0 among them: heavy ties.  Built once, left
    unchanged; a test takes the first n_cand columns."""
    gen = torch.Generator().manual_seed(2805)
    pred = torch.randint(-2, 3, (BATCH, N_MAX), generator=gen).float() / 2
    u = torch.rand(BATCH, N_MAX, generator=gen)
    pred[u < 0.03] = float("nan")
    pred[(u >= 0.03) & (u < 0.06)] = float("-inf")
    pred[(u >= 0.06) & (u < 0.08)] = float("inf")
    pred[(u >= 0.08) & (u < 0.12)] = -0.0
    pred[1, LEFT_ALIVE] = -1.0
    return pred.to(dev)


def lists(live, dev):
    """The known lists (ptr, index) of the top-k and the answer sets, and (pos, ptr, index) of the rank, whose lists hold the
    positives.  No id of them is in a retired set below; row 1 of the first is empty."""
    rows = [[1, 5, 40], [], [2, 33, 60, 4094, 4097, 8000, live - 2]]
    rows = [sorted(set(v for v in row if v < live - 1)) for row in rows]
    pos = [5, 7, 2]
    r_rows = [sorted(set(row + [p])) for row, p in zip(rows, pos)]

    def ragged(rows):
        ptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0).to(dev)
        return ptr, torch.tensor([v for r in rows for v in r], dtype=torch.long, device=dev)
    return ragged(rows), (torch.tensor(pos, device=dev),) + ragged(r_rows)


def retired_sets(live, known):
    """name -> sorted ids below `live`: the cases of the issue.  `known`: every id of the lists (they stay alive)."""
    alive = set(known) | {OTHERS[0], live + OTHERS[1]}
    sets = {"empty": [], "zero": [0], "word_edge": [31, 32], "chunk_edge": [4095, 4096], "last": [live - 1],
            "all_but": [v for v in range(live) if v not in alive]}
    return {name: [v for v in ids if v < live] for name, ids in sets.items()}


def operands(ids, n_cand, dev, count=None):
    """(bitmap over n_cand slots, count) on the device."""
    words = retired_words(torch.tensor(ids, dtype=torch.long), n_cand).to(dev)
    return words, torch.tensor([len(ids) if count is None else count], dtype=torch.long, device=dev)


def above_lists(out):
    total = int(out[0][-1])
    return out[0], out[1][:total], out[2][:total], out[3]


def rank_call(pred, pos, ptr, index, n_live=None, retired=None):
    rank, neg = predict.filtered_rank(pred, pos, ptr, index, num_live=n_live, retired=retired,
                                      out=(torch.full_like(pos, -7), torch.full_like(pos, -7)))
    torch.cuda.synchronize()
    return rank, neg


@pytest.mark.parametrize("n_cand", (70, 4101))
def test_filtered_rank_equals_its_restatement(dev, scores, n_cand):
    """predict.filtered_rank, the wrapper of the three rank entries: without operands, with a live count, with a retired set --
    rank and num_negative bit for bit; `out=` is written and handed back; a CPU tensor is the RuntimeError of the other wrappers."""
    pred = scores[:, :n_cand].contiguous()
    for live, gone in ((None, None), (n_cand - 7, None), (None, [31, 32])):
        pos, ptr, index = lists(n_cand if live is None else live, dev)[1]
        kw = {} if live is None else {"num_live": live}
        want = predict.filtered_rank_reference(pred, pos, ptr, index, **kw,
                                               **({} if gone is None else {"retired": torch.tensor(gone, device=dev)}))
        retired = None if gone is None else operands(gone, n_cand, dev)
        assert same(predict.filtered_rank(pred, pos, ptr, index, retired=retired, **kw), want), (live, gone)
        out = torch.full_like(pos, -7), torch.full_like(pos, -7)
        got = predict.filtered_rank(pred, pos, ptr, index, retired=retired, out=out, **kw)
        assert got[0] is out[0] and got[1] is out[1] and same(out, want), (live, gone)
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict.filtered_rank(pred.cpu(), pos.cpu(), ptr.cpu(), index.cpu())


@pytest.mark.parametrize("reserve", [0, 7], ids=["no_n_live", "n_live"])
@pytest.mark.parametrize("n_cand", N_CANDS)
def test_the_alive_entries_equal_the_restatements(dev, scores, n_cand, reserve):
    pred = scores[:, :n_cand].contiguous()
    live = n_cand - reserve
    n_live = torch.tensor([live], dtype=torch.long, device=dev) if reserve else None
    live_kw = {"num_live": n_live} if reserve else {}
    ref_kw = {"num_live": live} if reserve else {}
    (ptr, index), (pos, r_ptr, r_index) = lists(live, dev)
    for name, ids in retired_sets(live, index.tolist() + pos.tolist()).items():
        gone = torch.tensor(ids, dtype=torch.long, device=dev)
        pair = operands(ids, n_cand, dev)
        left = live - len(ids)
        want_top = {(k, f): predict.filtered_topk_reference(pred, k, *known, retired=gone, **ref_kw)
                    for k in KS for f, known in (("all", (None, None)), ("known", (ptr, index)))}
        want_above = {f: predict.filtered_above_reference(pred, THRESHOLD, *known, retired=gone, **ref_kw)
                      for f, known in (("all", (None, None)), ("known", (ptr, index)))}
        want_rank = predict.filtered_rank_reference(pred, pos, r_ptr, r_index, retired=gone, **ref_kw)
        assert want_rank[1].tolist() == [left - int(r_ptr[b + 1] - r_ptr[b]) for b in range(BATCH)]
        if name == "all_but":       # count < k, the padding, an empty answer set
            assert left == len(set(index.tolist() + pos.tolist())) + 2 and set(range(live)) - set(ids) <= set(LEFT_ALIVE)
            ids_, top_, count_ = want_top[(256, "known")]
            assert count_.tolist() == [left - int(ptr[b + 1] - ptr[b]) for b in range(BATCH)] and int(count_.max()) < 256
            assert int(want_top[(10, "known")][2].min()) < 10
            assert bool(ids_[:, -1].eq(-1).all()) and bool(top_[:, -1].eq(float("-inf")).all())
            out_ptr, _, _, size = want_above["known"]
            assert int(out_ptr[2] - out_ptr[1]) == 0 and int(size[1]) == 0
        for fill in (float("nan"), float("inf")):      # whatever a retired slot holds reaches no output
            poisoned = pred.clone()
            poisoned[:, gone] = fill
            for f, known in (("all", (None, None)), ("known", (ptr, index))):
                for k in KS:
                    got = predict.filtered_topk(poisoned, k, *known, retired=pair, **live_kw)
                    assert same(got, want_top[(k, f)]), (name, fill, k, f)
                    assert not bool(torch.isin(got[0], gone).any())
                got = above_lists(predict.filtered_above(poisoned, THRESHOLD, *known, retired=pair, **live_kw))
                assert same(got, want_above[f]), (name, fill, f)
            assert same(rank_call(poisoned, pos, r_ptr, r_index, n_live, pair), want_rank), (name, fill)


def test_a_bit_at_or_beyond_the_live_count_changes_nothing(dev, scores):
    n_cand, live = 4101, 4094
    pred = scores[:, :n_cand].contiguous()
    pred[:, live:] = float("inf")
    n_live = torch.tensor([live], dtype=torch.long, device=dev)
    (ptr, index), (pos, r_ptr, r_index) = lists(live, dev)
    inside = [31, 4000]
    clean = operands(inside, n_cand, dev)
    dirty = operands(inside + [live, live + 1, 4096, n_cand - 1], n_cand, dev, count=len(inside))
    assert not torch.equal(clean[0], dirty[0])
    for k in KS:
        assert same(predict.filtered_topk(pred, k, ptr, index, num_live=n_live, retired=dirty),
                    predict.filtered_topk(pred, k, ptr, index, num_live=n_live, retired=clean)), k
    assert same(above_lists(predict.filtered_above(pred, THRESHOLD, ptr, index, num_live=n_live, retired=dirty)),
                above_lists(predict.filtered_above(pred, THRESHOLD, ptr, index, num_live=n_live, retired=clean)))
    assert same(rank_call(pred, pos, r_ptr, r_index, n_live, dirty), rank_call(pred, pos, r_ptr, r_index, n_live, clean))
    want = predict.filtered_topk_reference(pred, 10, ptr, index, num_live=live, retired=torch.tensor(inside, device=dev))
    assert same(predict.filtered_topk(pred, 10, ptr, index, num_live=n_live, retired=dirty), want)


@pytest.mark.parametrize("n_cand", N_CANDS)
def test_with_nothing_retired_the_alive_entries_are_their_twins_and_parents(dev, scores, n_cand):
    pred = scores[:, :n_cand].contiguous()
    none = operands([], n_cand, dev)
    for live in (n_cand, n_cand - 7):
        n_live = torch.tensor([live], dtype=torch.long, device=dev)
        (ptr, index), (pos, r_ptr, r_index) = lists(live, dev)
        twins = [{"num_live": n_live}] + ([{}] if live == n_cand else [])       # (the parent: every slot is live)
        for kw in twins:
            for k in KS:
                assert same(predict.filtered_topk(pred, k, ptr, index, num_live=n_live, retired=none),
                            predict.filtered_topk(pred, k, ptr, index, **kw)), (live, k)
            assert same(above_lists(predict.filtered_above(pred, THRESHOLD, ptr, index, num_live=n_live, retired=none)),
                        above_lists(predict.filtered_above(pred, THRESHOLD, ptr, index, **kw))), live
            assert same(rank_call(pred, pos, r_ptr, r_index, n_live, none),
                        rank_call(pred, pos, r_ptr, r_index, kw.get("num_live"))), live
        if live == n_cand:      # a NULL live count: every slot is below the bound
            assert same(predict.filtered_topk(pred, 10, ptr, index, retired=none), predict.filtered_topk(pred, 10, ptr, index))
            assert same(rank_call(pred, pos, r_ptr, r_index, None, none), rank_call(pred, pos, r_ptr, r_index))


def test_null_retired_operands_are_invalid_and_nothing_is_launched(dev, scores):
    lib, n_cand, k = _lib.lib, 70, 10
    pred = scores[:, :n_cand].contiguous()
    (ptr, index), (pos, r_ptr, r_index) = lists(n_cand, dev)
    words, count = operands([3], n_cand, dev)
    ids = torch.full((BATCH, k), -7, dtype=torch.long, device=dev)
    top = torch.full((BATCH, k), -7.0, device=dev)
    cnt = torch.full((BATCH,), -7, dtype=torch.long, device=dev)
    ws = torch.empty(max(1, lib.ultra_filtered_topk_workspace(BATCH, n_cand, k) // 8), dtype=torch.long, device=dev)
    a_ptr = torch.full((BATCH + 1,), -7, dtype=torch.long, device=dev)
    a_ids = torch.full((BATCH * n_cand,), -7, dtype=torch.long, device=dev)
    a_scores = torch.empty(BATCH * n_cand, dtype=torch.float32, device=dev)
    a_size = torch.full((BATCH,), -7, dtype=torch.long, device=dev)
    a_ws = torch.empty(lib.ultra_filtered_above_workspace(BATCH, n_cand) // 8, dtype=torch.long, device=dev)
    rank, neg = torch.full((BATCH,), -7, dtype=torch.long, device=dev), torch.full((BATCH,), -7, dtype=torch.long, device=dev)
    stream = _lib.stream_of(dev)
    for b, c in ((None, count.data_ptr()), (words.data_ptr(), None), (None, None)):
        assert lib.ultra_filtered_topk_alive(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, n_cand, k, ids.data_ptr(),
                                             top.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel() * 8, None, b, c,
                                             stream) == _lib.ULTRA_ERR_INVALID
        assert lib.ultra_filtered_above_alive(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, n_cand, THRESHOLD,
                                              a_ptr.data_ptr(), a_ids.data_ptr(), a_scores.data_ptr(), a_ids.numel(),
                                              a_size.data_ptr(), a_ws.data_ptr(), a_ws.numel() * 8, None, b, c,
                                              stream) == _lib.ULTRA_ERR_INVALID
        assert lib.ultra_filtered_rank_alive(pred.data_ptr(), pos.data_ptr(), r_ptr.data_ptr(), r_index.data_ptr(), BATCH, n_cand,
                                             rank.data_ptr(), neg.data_ptr(), None, b, c, stream) == _lib.ULTRA_ERR_INVALID
    torch.cuda.synchronize()
    for out in (ids, cnt, a_ptr, a_ids, a_size, rank, neg):
        assert bool(out.eq(-7).all())
    assert bool(top.eq(-7.0).all())
    # the Python wrappers refuse a bitmap shorter than the row and operands of the wrong kind
    for bad in ((words[:2], count), (words, count.int()), (words.cpu(), count), words, (words.long(), count)):
        with pytest.raises(ValueError):
            predict.filtered_topk(pred, k, ptr, index, retired=bad)
        with pytest.raises(ValueError):
            predict.filtered_above(pred, THRESHOLD, ptr, index, retired=bad)


def test_one_capture_serves_a_later_retirement(dev, scores):
    """The three _alive calls recorded once into a graph; one more bit is set and the count raised through the resident tensors
    and the same graph replayed -- no new capture, the same buffers."""
    lib, k, n_cand, live = _lib.lib, 10, 8200, 8193
    pred = scores[:, :n_cand].contiguous()
    n_live = torch.tensor([live], dtype=torch.long, device=dev)
    (ptr, index), (pos, r_ptr, r_index) = lists(live, dev)
    first = [31, 4096]
    words, count = operands(first, n_cand, dev)
    ids = torch.empty(BATCH, k, dtype=torch.long, device=dev)
    top = torch.empty(BATCH, k, dtype=torch.float32, device=dev)
    cnt = torch.empty(BATCH, dtype=torch.long, device=dev)
    ws = torch.empty(max(1, lib.ultra_filtered_topk_workspace(BATCH, n_cand, k) // 8), dtype=torch.long, device=dev)
    a_ptr = torch.zeros(BATCH + 1, dtype=torch.long, device=dev)
    a_ids = torch.empty(BATCH * n_cand, dtype=torch.long, device=dev)
    a_scores = torch.empty(BATCH * n_cand, dtype=torch.float32, device=dev)
    a_size = torch.empty(BATCH, dtype=torch.long, device=dev)
    a_ws = torch.empty(lib.ultra_filtered_above_workspace(BATCH, n_cand) // 8, dtype=torch.long, device=dev)
    rank, neg = torch.empty(BATCH, dtype=torch.long, device=dev), torch.empty(BATCH, dtype=torch.long, device=dev)

    def step():
        stream = _lib.stream_of(dev)
        _lib.check(lib.ultra_filtered_topk_alive(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, n_cand, k,
                                                 ids.data_ptr(), top.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                 n_live.data_ptr(), words.data_ptr(), count.data_ptr(), stream))
        _lib.check(lib.ultra_filtered_above_alive(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, n_cand, THRESHOLD,
                                                  a_ptr.data_ptr(), a_ids.data_ptr(), a_scores.data_ptr(), a_ids.numel(),
                                                  a_size.data_ptr(), a_ws.data_ptr(), a_ws.numel() * 8, n_live.data_ptr(),
                                                  words.data_ptr(), count.data_ptr(), stream))
        _lib.check(lib.ultra_filtered_rank_alive(pred.data_ptr(), pos.data_ptr(), r_ptr.data_ptr(), r_index.data_ptr(), BATCH,
                                                 n_cand, rank.data_ptr(), neg.data_ptr(), n_live.data_ptr(), words.data_ptr(),
                                                 count.data_ptr(), stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    # the id retired later is the best answer of row 1 while it is alive: its leaving is seen
    best = int(predict.filtered_topk_reference(pred, 1, ptr, index, num_live=live,
                                               retired=torch.tensor(first, device=dev))[0][1, 0])
    negs = {}
    for gone in (first, sorted(first + [best])):
        words.copy_(retired_words(torch.tensor(gone), n_cand).to(dev))      # (the resident tensors, on the device)
        count.fill_(len(gone))
        ids.fill_(-7), a_ws.fill_(-1), ws.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        retired = torch.tensor(gone, device=dev)
        assert same((ids, top, cnt), predict.filtered_topk_reference(pred, k, ptr, index, num_live=live, retired=retired)), gone
        assert same(above_lists((a_ptr, a_ids, a_scores, a_size)),
                    predict.filtered_above_reference(pred, THRESHOLD, ptr, index, num_live=live, retired=retired)), gone
        assert same((rank, neg), predict.filtered_rank_reference(pred, pos, r_ptr, r_index, num_live=live, retired=retired)), gone
        assert (best in ids[1].tolist()) == (best not in gone)
        negs[len(gone)] = neg.clone()
    assert torch.equal(negs[3], negs[2] - 1)


# ---- end to end ----
@pytest.fixture(scope="module")
def model(dev):
    net = models.Ultra(**synthetic.default_model_cfg())
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def fixture_graph(dev):
    data = tasks.build_relation_graph(udata.load_triples_dir(os.path.join(GOLDEN, "kg_fixture")).to(dev))
    assert data.num_nodes == 300 and data.filtered_data is not None
    return data


def pick(data):
    """(a leaf, an entity of about the median degree, the next one, a second leaf) of the fixture graph."""
    deg = torch.bincount(data.edge_index.flatten(), minlength=int(data.num_nodes)).cpu()
    order = torch.argsort(deg, stable=True)
    order = order[deg[order] > 0]
    return int(order[0]), int(order[len(order) // 2]), int(order[len(order) // 2 + 1]), int(order[1])


def counted(monkeypatch, names):
    calls = dict.fromkeys(names, 0)
    for name in names:
        def wrapper(*args, _name=name, _fn=getattr(_lib.lib, name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, wrapper)
    return calls


def definition(fresh, live, call, anchor, relation):
    """The fresh predictor asked for k + num_retired answers, the retired ids dropped, the first k: (ids, scores)."""
    ids, scores, _ = getattr(fresh, call)(anchor, relation)
    k, retired = live.k, live.retired_entities
    out_ids = torch.full((len(anchor), k), -1, dtype=torch.long, device=ids.device)
    out_scores = torch.full((len(anchor), k), float("-inf"), device=ids.device)
    for b in range(len(anchor)):
        keep = (ids[b] >= 0) & ~torch.isin(ids[b], retired)
        m = min(k, int(keep.sum()))
        out_ids[b, :m], out_scores[b, :m] = ids[b][keep][:m], scores[b][keep][:m]
    return out_ids, out_scores


def verify_definition(model, mat, filter_graph, h, r, t, retired):
    """verify_tails in the terms of predict.verify_reference -- one filtered copy of the graph and one forward per fact -- ranked
    by the `retired=` restatement."""
    ent = predict._entity_model(model)
    score, rank, neg = [], [], []
    with torch.no_grad():
        for i in range(len(h)):
            batch = torch.stack([h[i:i + 1], t[i:i + 1], r[i:i + 1]], dim=-1)
            without = ent.remove_easy_edges(mat, h[i:i + 1], t[i:i + 1], r[i:i + 1])
            pred = model(without, tasks.all_negative(mat, batch)[0]).float()
            ptr, index = tasks.known_answers(filter_graph, batch, "tail")
            b_rank, b_neg = predict.filtered_rank_reference(pred, t[i:i + 1], ptr, index, retired=retired)
            score.append(pred[0, t[i]]), rank.append(b_rank[0]), neg.append(b_neg[0])
    return torch.stack(score), torch.stack(rank), torch.stack(neg)


@pytest.mark.parametrize("setup", ["plain", "reserve", "after_add_facts"])
def test_predictor_retires_entities(dev, model, fixture_graph, monkeypatch, setup):
    data = fixture_graph
    leaf, median, named, leaf2 = pick(data)
    calls = counted(monkeypatch, ALIVE_SYMBOLS + LIVE_SYMBOLS + PARENT_SYMBOLS)
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=8 if setup == "reserve" else 0)
    n = 300
    if setup == "reserve":
        (new,) = live.add_entities().tolist()
        n = 301
        live.add_facts([new, leaf2], [1, 3], [median, named])
    else:
        live.add_facts(leaf2, 3, named)                 # the held delta fact that names `named`
    if setup == "after_add_facts":
        live.add_facts([5, 9], [0, 2], [9, 11])
    h, t, r = data.target_triples[:12].unbind(-1)
    ok = ~(torch.isin(h, torch.tensor([leaf, median, named, leaf2], device=dev))
           | torch.isin(t, torch.tensor([leaf, median, named, leaf2], device=dev)))
    h, t, r = h[ok][:6], t[ok][:6], r[ok][:6]
    live.tails(h, r)
    assert all(calls[name] == 0 for name in ALIVE_SYMBOLS), calls
    held = len(live.delta)
    counts = live.remove_entities([leaf, median, named])
    assert bool((counts > 0).all()) and live.num_retired == 3 and len(live.delta) < held
    assert live.retired_entities.tolist() == sorted([leaf, median, named]) and live.num_entities == n
    for name in calls:
        calls[name] = 0

    def check(verify):
        retired = live.retired_entities
        got = {call: getattr(live, call)(anchor, r) for call, anchor in (("tails", h), ("heads", t))}
        sets = {thr: live.tails_above(h, r, thr) for thr in (0.0, -1e30)}
        verified = live.verify_tails(h[:3], r[:3], t[:3]) if verify else None
        saved = dict(calls)         # (the fresh predictor below calls the parents: not this predictor's calls)
        mat = live.materialized()
        assert mat.num_nodes == n and not bool(torch.isin(mat.edge_index, retired).any())
        assert torch.equal(mat.retired_entities, retired)
        fresh = predict.Predictor(model, mat, k=10 + live.num_retired, batch_size=4)
        for call, anchor, mode in (("tails", h, "tail"), ("heads", t, "head")):
            ids, top, count = got[call]
            assert same((ids, top), definition(fresh, live, call, anchor, r)), call
            assert not bool(torch.isin(ids, retired).any())
            ptr, index = predict.known_answers(live.filter_graph, anchor, r, mode)
            assert not bool(torch.isin(index, retired).any())
            assert count.tolist() == [min(10, n - live.num_retired - int(ptr[b + 1] - ptr[b])) for b in range(len(anchor))]
        with torch.no_grad():
            pred = model(mat, predict._candidates(mat, h, r, "tail")).float()
        ptr, index = predict.known_answers(live.filter_graph, h, r, "tail")
        for thr, out in sets.items():
            assert same(out, predict.filtered_above_reference(pred, thr, ptr, index, retired=retired)), thr
            assert not bool(torch.isin(out[1], retired).any())
        assert sets[-1e30][3].tolist() == [n - live.num_retired] * len(h)
        if verify:
            assert same(verified, verify_definition(model, mat, live.filter_graph, h[:3], r[:3], t[:3], retired))
            assert int(verified[2].max()) < n - live.num_retired
        fresh.close()
        calls.update(saved)

    check(verify=setup != "reserve")        # (with a reserve verify_* compacts first, DESIGN.md 19's rule: kept for the end)
    assert all(calls[name] > 0 for name in ALIVE_SYMBOLS[:2]), calls
    assert all(calls[name] == 0 for name in LIVE_SYMBOLS + PARENT_SYMBOLS), calls
    assert all(step.retired is not None and step.retired[0] is live._live.retired_bits for step in live._steps.values())
    for victim in (leaf, median, named):
        with pytest.raises(ValueError, match="retired"):
            live.tails([victim], [0])
        with pytest.raises(ValueError, match="retired"):
            live.verify_tails([victim], [0], [int(h[0])])
        with pytest.raises(ValueError, match="retired"):
            live.add_facts(int(h[0]), 0, victim)
    # a second retirement costs no new capture: the same step objects, the same recorded graphs
    live.tails(h, r), live.heads(t, r)
    if setup != "reserve":
        live.verify_tails(h[:3], r[:3], t[:3])
    steps = {key: (step, step.graph) for key, step in live._steps.items()}
    assert {"tail", "head"} <= set(steps) and (setup == "reserve" or "verify_tail" in steps)
    bits_before, count_before = live._live.retired_bits, live._live.retired_count
    assert int(live.remove_entities(leaf2)) > 0 and live.num_retired == 4
    assert live._live.retired_bits is bits_before and live._live.retired_count is count_before and int(count_before) == 4
    live.tails(h, r), live.heads(t, r)
    if setup != "reserve":
        live.verify_tails(h[:3], r[:3], t[:3])
    assert set(live._steps) == set(steps)
    assert all(live._steps[key] is step and live._steps[key].graph is graph for key, (step, graph) in steps.items())
    check(verify=True)
    assert all(calls[name] > 0 for name in ALIVE_SYMBOLS), calls
    assert all(calls[name] == 0 for name in LIVE_SYMBOLS + PARENT_SYMBOLS), calls
    live.close()


def test_a_predictor_that_never_retires_calls_no_alive_entry(dev, model, fixture_graph, monkeypatch):
    data = fixture_graph
    calls = counted(monkeypatch, ALIVE_SYMBOLS)
    h, t, r = data.target_triples[:6].unbind(-1)
    for kwargs in ({}, {"entity_capacity": 8}):
        plain = predict.Predictor(model, data, k=10, batch_size=4, **kwargs)
        plain.add_facts(5, 0, 9), plain.remove_facts(int(h[0]), int(r[0]), int(t[0]))
        plain.tails(h, r), plain.heads(t, r), plain.tails_above(h, r, 0.0), plain.verify_tails(h[1:], r[1:], t[1:])
        assert plain.num_retired == 0 and all(step.retired is None for step in plain._steps.values())
        plain.close()
    assert all(calls[name] == 0 for name in ALIVE_SYMBOLS), calls


def test_the_command_line_tool_retires_by_name(dev, capsys):
    """tools/predict.py --remove-entity NAME: the best answer of a query, retired by name, is no answer any more, and the name
    no longer resolves in an option that follows it."""
    import importlib.util
    root = os.path.join(GOLDEN, "kg_fixture")
    spec = importlib.util.spec_from_file_location("predict_tool", os.path.join(os.path.dirname(GOLDEN), os.pardir, "tools", "predict.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ent, rel = udata.read_vocab(root)
    triple = udata.load_triples_dir(root).target_triples[0].tolist()
    query = ["--data-root", root, "--ckpt", os.path.join(GOLDEN, "ultra_3g_model.pt"), "--head", ent[triple[0]], "--relation",
             rel[triple[2]], "-k", "5"]

    def answers(argv):
        tool.main(argv)
        lines = capsys.readouterr().out.splitlines()
        return lines, [line.split()[1] for line in lines if line[:3].strip().isdigit()]
    _, before = answers(query)
    assert len(before) == 5
    victim = before[0]
    lines, after = answers(query + ["--remove-entity", victim])
    assert any(line.startswith("entity %r retired" % victim) for line in lines)
    assert len(after) == 5 and victim not in after and after[:4] != before[:4]
    with pytest.raises(SystemExit):
        tool.main(query + ["--remove-entity", victim, "--add-fact", victim, rel[0], ent[triple[0]]])
    with pytest.raises(SystemExit):
        tool.main(query + ["--remove-entity", ent[triple[0]]])           # the query's own head
