"""Serving a growing graph, the parts that need no GPU: reserved rows, Predictor.add_entities, the live bound of
GraphDelta.check, materialize(num_nodes=...), the `num_live` restatements, the host-side checks of the _live entries.

The model is the golden ultra_3g weights under `rotate` messages: the configuration that runs on CPU tensors (the engine has no
CPU path), so every forward with a delta takes the materialising route of models.py.

Ids, counts, offsets and sizes are compared exactly.  SCORES are compared with SCORE_TOL here, not bit for bit: the contract
compares graphs of different row counts (N + M slots against num_entities nodes), and the host BLAS picks its blocking -- the
association of a row's dot products -- by the number of rows, so a score moves in its last bits (measured: at most 4.8e-7 at
scores near 4, one or two ulp).  The engine pins the summation order per row; the bit-equality of the scores is asserted where
it holds by construction, in test_grow_gpu.py.  The bound: a re-associated fp32 sum of n terms moves by at most about
n * 2^-24 of the sum of its terms' magnitudes; the model's dot products have 64 to 128 terms of order one, and the logits here
lie within +-16, so 128 * 2^-24 * 16 ~ 1.2e-4 bounds one such sum and 1e-5 -- twenty times what was measured -- is asked.  The
tests run torch on one thread, which keeps the row partition out of it."""
import ctypes
import os

import pytest
import torch

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks
from ultra_amd import data as udata
from ultra_amd.live import with_slots
from ultra_amd.data import Data

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LIVE_SYMBOLS = ("ultra_filtered_topk_live", "ultra_filtered_above_live", "ultra_filtered_rank_live")


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def served():
    model = models.Ultra(**synthetic.default_model_cfg(message_func="rotate"))
    model.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    data = udata.load_triples_dir(os.path.join(GOLDEN, "kg_fixture"))
    assert data.num_nodes == 300 and data.num_relations == 14 and data.filtered_data is not None
    return model.eval(), data


SCORE_TOL = 1e-5


def close(got, want):
    return got.shape == want.shape and torch.allclose(got, want, rtol=0.0, atol=SCORE_TOL, equal_nan=True)


def same_answers(got, want):
    """(ids, scores, count): ids and count exactly, scores within SCORE_TOL."""
    return torch.equal(got[0], want[0]) and close(got[1], want[1]) and torch.equal(got[2], want[2])


def same_sets(got, want):
    """(ptr, ids, scores, size): everything but the scores exactly."""
    return (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and close(got[2], want[2])
            and torch.equal(got[3], want[3]))


def grow(live):
    """Three entities in two calls, five facts (old-new, new-new, new-old, a repeated one, one about the third entity), one
    retraction of a fact about a new entity.  Returns the new ids."""
    a, b = live.add_entities(2).tolist()
    assert live.add_facts([5, a, b, a], [0, 1, 2, 1], [a, b, 7, b]) == 4          # (a, 1, b) twice: two parallel edges
    (c,) = live.add_entities().tolist()
    assert live.add_facts(c, 3, 10) == 5
    assert live.remove_facts(b, 2, 7).tolist() == [1]
    return a, b, c


def test_padding_leaves_the_scores_of_the_entities_alone(served):
    """The premise: rows without edges change no other row."""
    model, data = served
    n = int(data.num_nodes)
    h, _, r = data.target_triples[:4].unbind(-1)
    padded = with_slots(data, n + 8, relation_graph=True)
    assert padded is not data and padded.num_nodes == n + 8 and padded.edge_index is data.edge_index
    with torch.no_grad():
        want = model(data, predict._candidates(data, h, r, "tail"))
        got = model(padded, predict._candidates(padded, h, r, "tail"))
    assert got.shape == (4, n + 8) and close(got[:, :n], want) and float(want.abs().max()) < 16
    assert bool(torch.isfinite(got[:, n:]).all())


def test_the_relation_graph_of_a_padded_graph_is_that_of_the_graph(served):
    _, data = served
    padded = with_slots(data, int(data.num_nodes) + 8, relation_graph=True)
    assert padded.relation_graph is not data.relation_graph
    assert torch.equal(padded.relation_graph.edge_index, data.relation_graph.edge_index)
    assert torch.equal(padded.relation_graph.edge_type, data.relation_graph.edge_type)
    # (the bit matrices exist on the GPU only: test_grow_gpu.py compares adjacency_bits there)


def test_a_predictor_without_a_reserve_serves_the_graph_itself(served):
    model, data = served
    plain = predict.Predictor(model, data, k=5, batch_size=4)
    assert plain.data is data and plain.entity_capacity == 0 and plain.num_entities == 300 and plain.live_count is None
    with pytest.raises(ValueError):
        plain.add_entities()
    with pytest.raises(ValueError):
        plain.add_facts(300, 0, 1)
    for bad in (-1, 1.5, True, "8"):
        with pytest.raises(ValueError):
            predict.Predictor(model, data, entity_capacity=bad)


def test_add_entities_hands_out_the_reserved_rows(served):
    model, data = served
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=8)
    assert live.data is not data and live.num_slots == 308 and live.num_entities == 300
    assert live.data.edge_index is data.edge_index and live.filter_graph.num_nodes == 308
    scalar = live.live_count
    assert scalar.dtype == torch.long and scalar.numel() == 1 and int(scalar) == 300
    # a reserved row is no entity until it is handed out
    with pytest.raises(ValueError):
        live.add_facts(300, 0, 1)
    with pytest.raises(ValueError):
        live.remove_facts(1, 0, 307)
    for call in (live.tails, live.heads):
        with pytest.raises(ValueError):
            call([300], [0])
    with pytest.raises(ValueError):
        live.tails_above([5, 300], [0, 0], 0.0)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            live.add_entities(bad)
    served_graph, delta = live.data, live.delta
    a, b, c = grow(live)
    assert (a, b, c) == (300, 301, 302) and live.num_entities == 303 and int(live.live_count) == 303
    assert live.live_count is scalar and live.data is served_graph and live.delta is delta      # no rebuild, no new delta
    assert live.num_slots == 308 and live.delta.num_nodes == 308 and live.delta.num_live == 303
    with pytest.raises(ValueError):
        live.add_facts(303, 0, 1)
    with pytest.raises(ValueError):
        live.tails([303], [0])

    mat = live.materialized()
    assert mat.num_nodes == 303 and mat.edge_index.shape[1] == data.edge_index.shape[1] + 2 * 4
    assert mat.edge_index[:, -8:].tolist() == [[5, a, a, c, a, b, b, 10], [a, b, b, 10, 5, a, a, c]]
    assert mat.edge_type[-8:].tolist() == [0, 1, 1, 3, 7, 8, 8, 10]
    fresh = predict.Predictor(model, mat, k=10, batch_size=4)
    assert fresh.entity_capacity == 0 and fresh.data is mat
    qh = torch.tensor([5, a, b, c, 10, 7, int(data.target_triples[0, 0])])
    qr = torch.tensor([0, 1, 2, 3, 3, 2, int(data.target_triples[0, 2])])
    for call in ("tails", "heads"):
        got, want = getattr(live, call)(qh, qr), getattr(fresh, call)(qh, qr)
        assert same_answers(got, want), call
        assert int(got[0].max()) < 303 and bool((got[2] == 10).all())
    # a stated tail is a known answer, a retracted one a candidate again; an entity without a fact in that role is a candidate
    ptr, ids, _, size = live.tails_above(torch.tensor([5, a, b]), torch.tensor([0, 1, 2]), -1e30)
    lists = [ids[int(ptr[i]):int(ptr[i + 1])].tolist() for i in range(3)]
    assert a not in lists[0] and b not in lists[1] and 7 in lists[2]
    assert c in lists[0] and c in lists[1] and c in lists[2] and int(ids.max()) < 303 and size.tolist() == [303] * 3
    for thr in (0.0, -1e30):
        got, want = live.tails_above(qh, qr, thr), fresh.tails_above(qh, qr, thr)
        assert len(got) == 4 and same_sets(got, want), thr
        assert got[1].numel() == 0 or int(got[1].max()) < 303
    assert got[3].tolist() == [303] * len(qh)                 # size: every LIVE entity lies above -1e30, no reserved row is counted
    assert same_sets(live.heads_above(qh, qr, -1e30), fresh.heads_above(qh, qr, -1e30))
    # the answers differ from those of the graph before the edits at all
    base = predict.Predictor(model, data, k=10, batch_size=4)
    assert not torch.equal(base.tails(qh[:1], qr[:1])[1], live.tails(qh[:1], qr[:1])[1])


def test_beyond_the_reserve_the_graph_is_compacted_and_reserved_anew(served):
    model, data = served
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=2)
    scalar = live.live_count
    a, b = live.add_entities(2).tolist()
    live.add_facts([5, a], [0, 1], [a, b])
    first = live.data
    assert live.num_slots == 302 and len(live.delta) == 2
    assert live.add_entities(3).tolist() == [302, 303, 304]                      # 302 + 3 > 302: one rebuild
    assert live.data is not first and live.num_slots == 302 + 3 + 2 and live.num_entities == 305
    assert live.live_count is scalar and int(scalar) == 305 and not live.delta.edited and live.delta.num_live == 305
    assert live.data.edge_index.shape[1] == data.edge_index.shape[1] + 4        # the facts were folded into the graph
    assert live.filter_graph.num_nodes == 307
    live.add_facts(304, 2, b)
    fresh = predict.Predictor(model, live.materialized(), k=10, batch_size=4)
    qh, qr = torch.tensor([5, a, 304, b]), torch.tensor([0, 1, 2, 2])
    assert same_answers(live.tails(qh, qr), fresh.tails(qh, qr))
    assert same_answers(live.heads(qh, qr), fresh.heads(qh, qr))
    # compact() keeps the slot count and the live count
    live.compact()
    assert live.num_slots == 307 and live.num_entities == 305 and int(scalar) == 305 and not live.delta.edited
    assert same_answers(live.tails(qh, qr), fresh.tails(qh, qr))
    with pytest.raises(ValueError):
        live.tails([305], [0])
    # a reserve that ends exactly at the slot count is no overflow
    assert live.add_entities(2).tolist() == [305, 306] and live.num_slots == 307


def test_graph_delta_takes_the_live_bound():
    h, t, r = torch.tensor([0, 1, 2]), torch.tensor([1, 2, 3]), torch.tensor([0, 1, 0])
    data = tasks.build_relation_graph(Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]),
                                           edge_type=torch.cat([r, r + 2]), num_nodes=8, num_relations=4))
    delta = rspmm.GraphDelta(data, capacity=4, num_live=5)
    assert delta.num_nodes == 8 and delta.num_live == 5 and delta.degree.numel() == 8
    delta.add(4, 1, 0)                                       # row 4: no base edge at all
    for bad in ((5, 0, 1), (0, 0, 5), (7, 0, 7)):
        with pytest.raises(ValueError):
            delta.add(*bad)
        with pytest.raises(ValueError):
            delta.remove(*bad)
    delta.num_live = 6
    delta.add(5, 0, 4)
    assert delta.rows[:int(delta.count)].tolist() == [0, 4, 5] and delta.ptr[:4].tolist() == [0, 1, 3, 4]
    whole = delta.materialize(data)
    assert whole.num_nodes == 8 and delta.materialize(data) is whole
    cut = delta.materialize(data, num_nodes=6)
    assert cut.num_nodes == 6 and cut is not whole and whole.num_nodes == 8
    assert torch.equal(cut.edge_index, whole.edge_index) and torch.equal(cut.edge_type, whole.edge_type)
    assert cut.relation_graph is delta.relation_graph
    assert delta.materialize(data, num_nodes=8) is whole
    with pytest.raises(ValueError):
        delta.materialize(data, num_nodes=5)                 # the edge (5, 4) names id 5
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            rspmm.GraphDelta(data, capacity=4, num_live=bad)
    assert rspmm.GraphDelta(data, capacity=4).num_live == 8


def test_the_restatements_with_num_live_are_their_parents_on_the_sliced_scores():
    gen = torch.Generator().manual_seed(19)
    pred = torch.randint(-3, 4, (3, 40), generator=gen).float() / 2
    pred[0, 3], pred[1, 7], pred[2, 0] = float("nan"), float("inf"), float("-inf")
    for live in (1, 17, 39, 40):
        dead = pred.clone()
        dead[:, live:] = float("nan")                        # what a dead slot holds does not matter
        rows = [torch.nonzero(torch.rand(live, generator=gen) < 0.2).flatten() for _ in range(3)]
        rows[0] = torch.unique(torch.cat([rows[0], torch.tensor([live - 1])]))      # a known list that ends at the last live id
        ptr = torch.tensor([0] + [len(x) for x in rows]).cumsum(0)
        index = torch.cat(rows)
        for k in (1, 5, 64):
            for known in ((None, None), (ptr, index)):
                got = predict.filtered_topk_reference(dead, k, *known, num_live=live)
                want = predict.filtered_topk_reference(pred[:, :live], k, *known)
                assert all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x,
                                       y.view(torch.int32) if y.is_floating_point() else y) for x, y in zip(got, want))
                assert int(got[0].max()) < live
        for thr in (0.0, -1e30):
            for known in ((None, None), (ptr, index)):
                got = predict.filtered_above_reference(dead, thr, *known, num_live=live)
                want = predict.filtered_above_reference(pred[:, :live], thr, *known)
                assert all(torch.equal(x, y) for x, y in zip(got, want))
    for bad in (0, 41, -1):
        with pytest.raises(ValueError):
            predict.filtered_topk_reference(pred, 3, num_live=bad)
        with pytest.raises(ValueError):
            predict.filtered_above_reference(pred, 0.0, num_live=bad)


def test_the_live_entries_are_exported_and_validate_on_the_host():
    lib = _lib.lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in LIVE_SYMBOLS:
        assert hasattr(raw, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ultra_nbfnet.h")).read()
    for name in LIVE_SYMBOLS:
        assert name + "(" in header, name
    assert lib.ultra_abi_version() == 7
    host = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(host)
    need = lib.ultra_filtered_topk_workspace(1, 100, 10)
    # a NULL live count is ULTRA_ERR_INVALID; the parents' rules come first and hold under the twin's name
    assert lib.ultra_filtered_topk_live(p, None, None, 1, 100, 10, p, p, p, p, need, None, None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_filtered_topk_live" in lib.ultra_last_error() and b"n_live" in lib.ultra_last_error()
    assert lib.ultra_filtered_topk_live(p, None, None, 1, 100, 0, p, p, p, p, need, None, None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_filtered_topk_live(p, None, None, 1, 2 ** 31, 10, p, p, p, p, need, p, None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_filtered_topk_live(None, None, None, 1, 100, 10, None, None, None, None, 0, p, None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_filtered_topk_live" in lib.ultra_last_error()
    assert lib.ultra_filtered_topk_live(p, None, None, 1, 100, 10, p, p, p, p, need - 1, p, None) == _lib.ULTRA_ERR_INVALID
    assert b"workspace" in lib.ultra_last_error()
    assert lib.ultra_filtered_topk_live(p, None, None, 0, 100, 10, p, p, p, p, need, p, None) == _lib.ULTRA_OK      # batch 0
    need = lib.ultra_filtered_above_workspace(1, 100)
    assert lib.ultra_filtered_above_live(p, None, None, 1, 100, 0.0, p, p, p, 100, p, p, need, None, None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_filtered_above_live" in lib.ultra_last_error() and b"n_live" in lib.ultra_last_error()
    assert lib.ultra_filtered_above_live(p, None, None, 1, 100, float("nan"), p, p, p, 100, p, p, need, None, None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_filtered_above_live(p, None, None, 1, 100, 0.0, p, p, p, 99, p, p, need, p, None) == _lib.ULTRA_ERR_INVALID
    assert b"capacity" in lib.ultra_last_error()
    assert lib.ultra_filtered_above_live(p, None, None, 0, 100, 0.0, p, p, p, 100, p, p, need, p, None) == _lib.ULTRA_OK
    assert lib.ultra_filtered_rank_live(p, p, p, p, 1, 100, p, p, None, None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_filtered_rank_live" in lib.ultra_last_error() and b"n_live" in lib.ultra_last_error()
    # the parents answer as before, under their own names
    assert lib.ultra_filtered_topk(None, None, None, 1, 100, 10, None, None, None, None, 0, None) == _lib.ULTRA_ERR_INVALID
    assert b"ultra_filtered_topk:" in lib.ultra_last_error()
    # the Python wrappers check an int `num_live` before anything else is looked at on the device
    with pytest.raises(RuntimeError):
        predict.filtered_topk(torch.zeros(1, 4), 2, num_live=3)                 # (no CPU path, as without num_live)
