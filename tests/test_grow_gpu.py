"""Serving a growing graph on the GPU: the live-count twins of the selection entries against the plain-torch
restatements on the sliced scores, delta edges into rows WITHOUT base edges (reserved rows) through ultra_rspmm_delta_rows /
_edit_rows, and Predictor(entity_capacity) end to end against a fresh Predictor on the materialised graph -- bit for bit."""
import os

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd import data as udata
from ultra_amd.live import with_slots
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LIVE_SYMBOLS = ("ultra_filtered_topk_live", "ultra_filtered_above_live", "ultra_filtered_rank_live")
PARENT_SYMBOLS = ("ultra_filtered_topk", "ultra_filtered_above", "ultra_filtered_rank")

# ---- the selection kernels: two chunks, the second partly or wholly dead ----
N_CAND, BATCH = _lib.TOPK_CHUNK + 300, 3
LIVE_COUNTS = (1, 4095, 4096, 4097, 4396)
KS = (1, 10, 256)
THRESHOLD = 0.25


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
    """(BATCH, N_CAND) scores from {-1, -.5, 0, .5, 1} with NaN, -inf, +inf and -0.0 among them: heavy ties, every special value
    among the LIVE ids too.  Built once, left unchanged."""
    gen = torch.Generator().manual_seed(1905)
    pred = torch.randint(-2, 3, (BATCH, N_CAND), generator=gen).float() / 2
    u = torch.rand(BATCH, N_CAND, generator=gen)
    pred[u < 0.03] = float("nan")
    pred[(u >= 0.03) & (u < 0.06)] = float("-inf")
    pred[(u >= 0.06) & (u < 0.08)] = float("inf")
    pred[(u >= 0.08) & (u < 0.12)] = -0.0
    pred[:, 0] = torch.tensor([0.5, float("nan"), -1.0])       # (what n_live == 1 selects from)
    return pred.to(dev)


def known_lists(n_live, dev, seed):
    """(ptr, index): row 0 ends at the last live id, row 1 is empty, row 2 holds about a fifth of the live ids."""
    gen = torch.Generator().manual_seed(seed)
    last = torch.tensor([n_live - 1])
    rows = [torch.unique(torch.cat([torch.nonzero(torch.rand(n_live, generator=gen) < 0.01).flatten(), last])),
            torch.zeros(0, dtype=torch.long),
            torch.nonzero(torch.rand(n_live, generator=gen) < 0.2).flatten()]
    ptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0)
    return ptr.to(dev), torch.cat(rows).to(dev)


def with_dead(scores, n_live, fill):
    pred = scores.clone()
    pred[:, n_live:] = fill
    return pred


def above_lists(out):
    """(ptr, ids, scores, size) with the full-capacity buffers cut at the total."""
    total = int(out[0][-1])
    return out[0], out[1][:total], out[2][:total], out[3]


def rank_reference(pred, pos, ptr, index):
    """(rank, num_negative) of tasks.py:94-141 in plain torch; the known lists hold the positives."""
    rank, neg = [], []
    for q in range(pred.shape[0]):
        mask = torch.ones(pred.shape[1], dtype=torch.bool, device=pred.device)
        mask[index[int(ptr[q]):int(ptr[q + 1])]] = False
        rank.append(1 + int((mask & (pred[q] >= pred[q, pos[q]])).sum()))
        neg.append(int(mask.sum()))
    return torch.tensor(rank, device=pred.device), torch.tensor(neg, device=pred.device)


def rank_call(pred, pos, ptr, index, n_live=None):
    rank, neg = torch.empty_like(pos), torch.empty_like(pos)
    args = (pred.data_ptr(), pos.data_ptr(), ptr.data_ptr(), index.data_ptr(), pred.shape[0], pred.shape[1], rank.data_ptr(),
            neg.data_ptr())
    if n_live is None:
        _lib.check(_lib.lib.ultra_filtered_rank(*args, _lib.stream_of(pred.device)))
    else:
        _lib.check(_lib.lib.ultra_filtered_rank_live(*args, n_live.data_ptr(), _lib.stream_of(pred.device)))
    torch.cuda.synchronize()
    return rank, neg


def rank_lists(n_live, dev, seed):
    """Positives (the last live id in row 0) and known lists that hold them."""
    ptr, index = known_lists(n_live, dev, seed)
    pos = torch.tensor([n_live - 1, n_live // 2, 0], device=dev)
    rows = [torch.unique(torch.cat([index[int(ptr[q]):int(ptr[q + 1])], pos[q:q + 1]])) for q in range(BATCH)]
    ptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0).to(dev)
    return pos, ptr, torch.cat(rows)


@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["dead_nan", "dead_inf"])
@pytest.mark.parametrize("n_live", LIVE_COUNTS)
def test_the_live_entries_equal_the_restatements_on_the_sliced_scores(dev, scores, n_live, fill):
    pred = with_dead(scores, n_live, fill)
    live = pred[:, :n_live]
    ptr, index = known_lists(n_live, dev, seed=n_live)
    assert int(index[int(ptr[1]) - 1]) == n_live - 1                        # row 0 ends at the last live id
    count = torch.tensor(n_live, dtype=torch.long, device=dev)
    for known in ((None, None), (ptr, index)):
        for k in KS:
            want = predict.filtered_topk_reference(live, k, *known)
            assert same(predict.filtered_topk(pred, k, *known, num_live=n_live), want), (k, known[0] is None)
            assert same(predict.filtered_topk(pred, k, *known, num_live=count), want), (k, known[0] is None)      # the device scalar
            assert int(want[0].max()) < n_live
            if k > n_live:                                                  # the padding: id -1, score -inf
                assert want[0][:, n_live:].eq(-1).all() and want[1][:, n_live:].eq(float("-inf")).all()
        # above: with +inf in the dead slots every one of them would be a member of this threshold
        want = predict.filtered_above_reference(live, THRESHOLD, *known)
        got = above_lists(predict.filtered_above(pred, THRESHOLD, *known, num_live=count))
        assert same(got, want), known[0] is None
        assert got[1].numel() == 0 or int(got[1].max()) < n_live
        if fill == float("inf") and n_live < N_CAND:
            assert int(predict.filtered_above_reference(pred, THRESHOLD)[3][0]) >= int(want[3][0]) + N_CAND - n_live
    pos, r_ptr, r_index = rank_lists(n_live, dev, seed=n_live)
    want = rank_reference(live, pos, r_ptr, r_index)
    assert same(rank_call(pred, pos, r_ptr, r_index, n_live=count), want)
    assert same(rank_call(live.contiguous(), pos, r_ptr, r_index), want)    # the twin: the parent on the sliced scores
    # the parents on the very same buffers: every slot is a candidate, NaN and +inf included, as before
    for k in KS:
        assert same(predict.filtered_topk(pred, k, ptr, index), predict.filtered_topk_reference(pred, k, ptr, index)), k
    assert same(above_lists(predict.filtered_above(pred, THRESHOLD, ptr, index)),
                predict.filtered_above_reference(pred, THRESHOLD, ptr, index))
    assert same(rank_call(pred, pos, r_ptr, r_index), rank_reference(pred, pos, r_ptr, r_index))


def test_a_live_count_out_of_range_is_clamped_on_the_device(dev, scores):
    """1 <= *n_live <= n_cand is the caller's contract; a value outside it is clamped to [0, n_cand], never used as an index."""
    pred = with_dead(scores, N_CAND, 0.0)
    ptr, index = known_lists(N_CAND, dev, seed=3)
    whole = predict.filtered_topk_reference(pred, 10, ptr, index)
    big = torch.tensor(1 << 40, dtype=torch.long, device=dev)
    assert same(predict.filtered_topk(pred, 10, ptr, index, num_live=big), whole)
    none = torch.tensor(-5, dtype=torch.long, device=dev)
    ids, score, count = predict.filtered_topk(pred, 10, None, None, num_live=none)
    assert ids.eq(-1).all() and score.eq(float("-inf")).all() and count.eq(0).all()
    out = above_lists(predict.filtered_above(pred, THRESHOLD, None, None, num_live=none))
    assert out[0].eq(0).all() and out[1].numel() == 0 and out[3].eq(0).all()
    for bad in (0, N_CAND + 1):
        with pytest.raises(ValueError):
            predict.filtered_topk(pred, 10, num_live=bad)                   # an int is checked on the host
        with pytest.raises(ValueError):
            predict.filtered_above(pred, THRESHOLD, num_live=bad)


def test_one_capture_serves_a_later_live_count(dev, scores):
    """The three _live calls recorded once into a graph; the live count is overwritten on the device from 4095 to 4097 and the
    same graph replayed -- no new capture, the same buffers."""
    lib, k = _lib.lib, 10
    pred = with_dead(scores, 4095, float("nan"))
    pred[:, 4095:4097] = float("inf")            # the two slots that come alive later: members of any threshold, above any positive
    ptr, index = known_lists(4095, dev, seed=8)
    pos, r_ptr, r_index = rank_lists(4095, dev, seed=8)
    n_live = torch.tensor([4095], dtype=torch.long, device=dev)
    ids = torch.empty(BATCH, k, dtype=torch.long, device=dev)
    top = torch.empty(BATCH, k, dtype=torch.float32, device=dev)
    count = torch.empty(BATCH, dtype=torch.long, device=dev)
    ws = torch.empty(max(1, lib.ultra_filtered_topk_workspace(BATCH, N_CAND, k) // 8), dtype=torch.long, device=dev)
    a_ptr = torch.zeros(BATCH + 1, dtype=torch.long, device=dev)
    a_ids = torch.empty(BATCH * N_CAND, dtype=torch.long, device=dev)
    a_scores = torch.empty(BATCH * N_CAND, dtype=torch.float32, device=dev)
    a_size = torch.empty(BATCH, dtype=torch.long, device=dev)
    a_ws = torch.empty(lib.ultra_filtered_above_workspace(BATCH, N_CAND) // 8, dtype=torch.long, device=dev)
    rank, neg = torch.empty(BATCH, dtype=torch.long, device=dev), torch.empty(BATCH, dtype=torch.long, device=dev)

    def step():
        stream = _lib.stream_of(dev)
        _lib.check(lib.ultra_filtered_topk_live(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, N_CAND, k, ids.data_ptr(),
                                                top.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 8, n_live.data_ptr(),
                                                stream))
        _lib.check(lib.ultra_filtered_above_live(pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), BATCH, N_CAND, THRESHOLD,
                                                 a_ptr.data_ptr(), a_ids.data_ptr(), a_scores.data_ptr(), a_ids.numel(),
                                                 a_size.data_ptr(), a_ws.data_ptr(), a_ws.numel() * 8, n_live.data_ptr(), stream))
        _lib.check(lib.ultra_filtered_rank_live(pred.data_ptr(), pos.data_ptr(), r_ptr.data_ptr(), r_index.data_ptr(), BATCH, N_CAND,
                                                rank.data_ptr(), neg.data_ptr(), n_live.data_ptr(), stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    sizes = {}
    for live in (4095, 4097):
        n_live.fill_(live)                       # (on the device)
        ids.fill_(-7), a_ws.fill_(-1), ws.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert same((ids, top, count), predict.filtered_topk_reference(pred[:, :live], k, ptr, index)), live
        assert same(above_lists((a_ptr, a_ids, a_scores, a_size)), predict.filtered_above_reference(pred[:, :live], THRESHOLD, ptr, index)), live
        assert same((rank, neg), rank_reference(pred[:, :live], pos, r_ptr, r_index)), live
        sizes[live] = (a_size.clone(), neg.clone())
    assert torch.equal(sizes[4097][0], sizes[4095][0] + 2) and torch.equal(sizes[4097][1], sizes[4095][1] + 2)


# ---- delta edges into rows without base edges ----
G_NODES, G_SLOTS, G_DIRECT, G_BATCH, G_D = 40, 48, 3, 2, 64
# (h, r, t): row 40 gets ONE edge; row 41 three, from distinct sources; row 47 two parallel ones
G_FACTS = [(40, 0, 5), (41, 0, 3), (41, 1, 9), (2, 2, 41), (47, 1, 6), (47, 1, 6)]


@pytest.fixture(scope="module")
def reserved(dev):
    """(graph of 40 nodes padded to 48 on the GPU, its reference-order plan, {name: (delta, fresh plan of the materialised list
    on 48 nodes)}): add-only, and the same with one tombstone elsewhere."""
    base = synthetic.make_kg(num_node=G_NODES, num_triple=160, num_relation_base=G_DIRECT, num_test=8, seed=23, relation_graph=False)
    data = Data(edge_index=base.edge_index.to(dev), edge_type=base.edge_type.to(dev), num_nodes=G_SLOTS, num_relations=2 * G_DIRECT)
    assert int(data.edge_index.max()) < G_NODES and base.num_relations == 2 * G_DIRECT
    plan = rspmm.Plan(data.edge_index, data.edge_type, G_SLOTS, 2 * G_DIRECT, exact_order=True)
    row_ptr = plan.export(_lib.ARR_ROW_PTR).tolist()
    assert all(row_ptr[r] == row_ptr[r + 1] for r in range(G_NODES, G_SLOTS))       # the reserved rows: no base edge at all
    deltas = {}
    for name in ("added", "added_and_tombstone"):
        delta = rspmm.GraphDelta(data, capacity=8, num_live=G_SLOTS)
        delta.add(*zip(*G_FACTS))
        if name == "added_and_tombstone":
            h, t, r = int(data.edge_index[0, 0]), int(data.edge_index[1, 0]), int(data.edge_type[0])
            assert r < G_DIRECT and int(delta.remove(h, r, t)) >= 1 and delta.num_removed == 2
        touched = delta.rows[:int(delta.count)].tolist()
        assert {40, 41, 47} <= set(touched)
        at = {row: k for k, row in enumerate(touched)}
        ptr = delta.ptr.tolist()
        assert [ptr[at[r] + 1] - ptr[at[r]] for r in (40, 41, 47)] == [1, 3, 2]
        mat = delta.materialize(data)
        assert mat.num_nodes == G_SLOTS
        deltas[name] = (delta, rspmm.Plan(mat.edge_index, mat.edge_type, G_SLOTS, 2 * G_DIRECT, exact_order=True))
    return data, plan, deltas


@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
def test_delta_edges_into_rows_without_base_edges(dev, reserved, sum, mul):
    data, plan, deltas = reserved
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(G_BATCH, G_SLOTS, G_D, generator=gen).to(dev)
    rel = torch.randn(G_BATCH, 2 * G_DIRECT, G_D, generator=gen).to(dev)
    bnd = torch.randn(G_BATCH, G_SLOTS, G_D, generator=gen).to(dev)
    rows = torch.tensor([40, 5], device=dev)                # the point sits ON a reserved row in sample 0 and OFF one in sample 1
    vals = torch.randn(G_BATCH, G_D, generator=gen).to(dev)
    for kind, kwargs in (("none", {}), ("dense", dict(boundary=bnd)), ("point", dict(point=(rows, vals)))):
        base = plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
        for name, (delta, mat_plan) in deltas.items():
            fix = plan.edit_rows if delta.num_removed else plan.delta_rows
            out = base.clone()
            assert fix(rel, x, out, delta, sum=sum, mul=mul, **kwargs) is out, (name, kind)
            want = mat_plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (name, kind, (out != want).any(-1).nonzero()[:8].tolist())
            assert bool(torch.isfinite(out).all()), (name, kind)
            assert not torch.equal(out[:, [40, 41, 47]], base[:, [40, 41, 47]]), (name, kind)
        # an add-only delta through edit_rows is delta_rows (removed == NULL)
        delta = deltas["added"][0]
        assert torch.equal(plan.edit_rows(rel, x, base.clone(), delta, sum=sum, mul=mul, **kwargs),
                           plan.delta_rows(rel, x, base.clone(), delta, sum=sum, mul=mul, **kwargs)), kind


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


def grow(live):
    """Three entities in two calls, five facts (old-new, new-new, new-old, a repeated one, one about the third entity), one
    retraction of a fact about a new entity: the edits of test_grow_cpu.py.  Returns (the new ids, the captured steps and the
    identity of their graphs after the first call's edits)."""
    a, b = live.add_entities(2).tolist()
    assert live.add_facts([5, a, b, a], [0, 1, 2, 1], [a, b, 7, b]) == 4
    assert live.remove_facts(b, 2, 7).tolist() == [1]
    probe = torch.tensor([5, a], device=live.data.edge_index.device)
    live.tails(probe, probe * 0), live.heads(probe, probe * 0)
    steps = {key: (step, step.graph) for key, step in live._steps.items()}
    (c,) = live.add_entities().tolist()
    assert live.add_facts(c, 3, 10) == 4
    return (a, b, c), steps


def test_padding_leaves_the_engine_scores_bit_equal(dev, model, fixture_graph):
    """The premise, on the engine: reserved rows change no score of an entity by a bit, and the relation graph not at all."""
    data = fixture_graph
    padded = with_slots(data, 308, relation_graph=True)
    assert torch.equal(padded.relation_graph.adjacency_bits, data.relation_graph.adjacency_bits)
    assert torch.equal(padded.relation_graph.edge_index, data.relation_graph.edge_index)
    h, t, r = data.target_triples[:4].unbind(-1)
    with torch.no_grad():
        for mode, anchor in (("tail", h), ("head", t)):
            want = model(data, predict._candidates(data, anchor, r, mode))
            got = model(padded, predict._candidates(padded, anchor, r, mode))
            assert got.shape == (4, 308) and torch.equal(got[:, :300].view(torch.int32), want.view(torch.int32)), mode
            assert bool(torch.isfinite(got).all())


def test_predictor_serves_the_growing_graph(dev, model, fixture_graph):
    data = fixture_graph
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=8)
    scalar = live.live_count
    assert live.data is not data and live.num_slots == 308 and scalar.is_cuda and int(scalar) == 300
    (a, b, c), steps = grow(live)
    assert (a, b, c) == (300, 301, 302) and live.num_entities == 303 and int(scalar) == 303 and live.live_count is scalar
    assert steps["tail"][0].n_live is scalar
    mat = live.materialized()
    assert mat.num_nodes == 303 and mat.edge_index.shape[1] == data.edge_index.shape[1] + 8
    fresh = predict.Predictor(model, mat, k=10, batch_size=4)
    assert fresh.entity_capacity == 0 and fresh.live_count is None
    qh = torch.tensor([5, a, b, c, 10, 7, int(data.target_triples[0, 0])], device=dev)
    qr = torch.tensor([0, 1, 2, 3, 3, 2, int(data.target_triples[0, 2])], device=dev)
    for call in ("tails", "heads"):
        got = getattr(live, call)(qh, qr)
        assert same(got, getattr(fresh, call)(qh, qr)), call
        assert int(got[0].max()) < 303 and bool((got[2] == 10).all())
    # the second add_entities and the fact after it made no new capture: the same step objects, the same recorded graphs
    assert set(live._steps) == set(steps)
    assert all(live._steps[key] is step and live._steps[key].graph is graph for key, (step, graph) in steps.items())
    for thr in (0.0, -1e30):
        got = live.tails_above(qh, qr, thr)
        assert same(got, fresh.tails_above(qh, qr, thr)), thr
        assert got[1].numel() == 0 or int(got[1].max()) < 303
    assert got[3].tolist() == [303] * len(qh)                # every live entity lies above -1e30; no reserved row is counted
    assert same(live.heads_above(qh, qr, 0.0), fresh.heads_above(qh, qr, 0.0))
    lists = [got[1][int(got[0][i]):int(got[0][i + 1])].tolist() for i in range(3)]
    assert a not in lists[0] and b not in lists[1] and 7 in lists[2] and c in lists[0]       # stated: known; retracted: a candidate
    # ids in the reserve are no entities
    for call in (live.tails, live.heads):
        with pytest.raises(ValueError):
            call([303], [0])
    with pytest.raises(ValueError):
        live.verify_tails([5], [0], [303])
    # verify_*: compacts first (the slot count and the live count stay), then ranks among the live ids only
    vh = torch.tensor([5, a, c, int(data.target_triples[1, 0])], device=dev)
    vr = torch.tensor([0, 1, 3, int(data.target_triples[1, 2])], device=dev)
    vt = torch.tensor([a, b, 10, int(data.target_triples[1, 1])], device=dev)
    got = live.verify_tails(vh, vr, vt)
    assert not live.delta.edited and live.num_slots == 308 and live.num_entities == 303 and int(scalar) == 303
    assert same(got, fresh.verify_tails(vh, vr, vt))
    assert int(got[2].max()) < 303
    assert same(live.verify_heads(vh, vr, vt), fresh.verify_heads(vh, vr, vt))
    assert same(live.tails(qh, qr), fresh.tails(qh, qr))
    # beyond the reserve: one rebuild, then the same answers
    more = live.add_entities(6)
    assert more.tolist() == list(range(303, 309)) and live.num_slots == 309 + 8 and int(scalar) == 309 and live.live_count is scalar
    live.add_facts(more[-1:], [2], [b])
    fresh = predict.Predictor(model, live.materialized(), k=10, batch_size=4)
    qh2, qr2 = torch.cat([qh, more[-1:]]), torch.cat([qr, qr[:1] * 0 + 2])
    assert same(live.tails(qh2, qr2), fresh.tails(qh2, qr2))
    assert same(live.heads(qh2, qr2), fresh.heads(qh2, qr2))
    assert same(live.tails_above(qh2, qr2, 0.0), fresh.tails_above(qh2, qr2, 0.0))
    live.close(), fresh.close()


def counted(monkeypatch, names):
    calls = dict.fromkeys(names, 0)
    for name in names:
        def wrapper(*args, _name=name, _fn=getattr(_lib.lib, name)):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, wrapper)
    return calls


def test_a_default_predictor_never_calls_a_live_entry(dev, model, fixture_graph, monkeypatch):
    """entity_capacity=0: the graph itself, today's entries, today's answers -- the restatements on the model's own scores."""
    data = fixture_graph
    calls = counted(monkeypatch, LIVE_SYMBOLS + PARENT_SYMBOLS)
    plain = predict.Predictor(model, data, k=10, batch_size=4)
    assert plain.data is data and plain.live_count is None
    h, t, r = data.target_triples[:6].unbind(-1)
    got = {"tail": plain.tails(h, r), "head": plain.heads(t, r)}
    assert all(step.n_live is None for step in plain._steps.values())
    sets = plain.tails_above(h, r, 0.0)
    verified = plain.verify_tails(h, r, t)
    assert all(calls[name] == 0 for name in LIVE_SYMBOLS), calls
    assert all(calls[name] > 0 for name in PARENT_SYMBOLS), calls
    with torch.no_grad():
        for mode, anchor in (("tail", h), ("head", t)):
            pred = model(data, predict._candidates(data, anchor, r, mode)).float()
            ptr, index = predict.known_answers(plain.filter_graph, anchor, r, mode)
            assert same(got[mode], predict.filtered_topk_reference(pred, 10, ptr, index)), mode
            if mode == "tail":
                assert same(sets, predict.filtered_above_reference(pred, 0.0, ptr, index))
    assert same([v[:3] for v in verified], predict.verify_reference(model, data, plain.filter_graph, h[:3], r[:3], t[:3]))
    with pytest.raises(ValueError):
        plain.add_entities()
    # ... and a predictor with a reserve takes the twins, and only them
    for name in calls:
        calls[name] = 0
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=8)
    live.tails(h, r), live.tails_above(h, r, 0.0), live.verify_tails(h, r, t)
    assert all(calls[name] > 0 for name in LIVE_SYMBOLS), calls
    assert all(calls[name] == 0 for name in PARENT_SYMBOLS), calls
    plain.close(), live.close()
