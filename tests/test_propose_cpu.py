"""Link discovery -- the best k (query, answer) pairs over many queries --, the parts that need no GPU:
merge_pairs_reference over successive batches against ONE stable sort of everything (written out in this file), Predictor's
best_tails / propose_tails / propose_heads on the CPU route against best_reference, the argument errors, and the host side of
ultra_topk_pairs_merge.

The model is the golden ultra_3g weights under `rotate` messages, the configuration that runs on CPU tensors (test_grow_cpu.py).
The predictor and best_reference walk the SAME graph object through the same host route (after an edit: the predictor's own
materialized() graph, or its served graph with the live count and the retired ids as operands), so scores are compared bit for
bit."""
import ctypes
import os

import pytest
import torch

from ultra_amd import _lib, models, predict, synthetic
from ultra_amd import data as udata

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAN, INF = float("nan"), float("inf")
VALUES = [NAN, INF, 2.0, 0.5, 0.5, 0.25, 0.0, -0.0, -1.5, -INF]       # what a slot may hold: ties, both zeros, the specials


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def a_batch(batch, k_row, seed, all_pads_row=None):
    """(ids, scores) as a row-wise selection writes them: per row some distinct ids with scores out of VALUES in the stable
    descending order (equal scores by ascending id), then -1 / -inf pads.  Row `all_pads_row` holds pads alone; a -inf drawn from
    VALUES is a genuine candidate beside the pads."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((batch, k_row), -1, dtype=torch.long)
    scores = torch.full((batch, k_row), -INF)
    for b in range(batch):
        m = 0 if b == all_pads_row else int(torch.randint(1, k_row + 1, (1,), generator=g))
        row_ids = torch.sort(torch.randperm(1000, generator=g)[:m]).values
        row_scores = torch.tensor(VALUES)[torch.randint(0, len(VALUES), (m,), generator=g)]
        order = torch.sort(row_scores, descending=True, stable=True).indices
        ids[b, :m], scores[b, :m] = row_ids[order], row_scores[order]
    return ids, scores


def one_sort(batches, k, min_score):
    """The expectation: the rows of every batch -- (ids, scores, query_base, n_rows) -- laid end to end, pads and non-members
    dropped, one stable descending sort, the first k."""
    query, answer, score = [], [], []
    for ids, scores, base, n_rows in batches:
        rows = ids.shape[0] if n_rows is None else n_rows
        for b in range(rows):
            for j in range(ids.shape[1]):
                if int(ids[b, j]) < 0:
                    continue
                if min_score is not None and not float(scores[b, j]) > min_score:        # (false for a NaN)
                    continue
                query.append(base + b)
                answer.append(int(ids[b, j]))
                score.append(scores[b, j])
    score = torch.stack(score) if score else torch.zeros(0)
    order = torch.sort(score, descending=True, stable=True).indices[:k]
    m = len(order)
    out = (torch.full((k,), -1, dtype=torch.long), torch.full((k,), -1, dtype=torch.long), torch.full((k,), -INF), m)
    out[0][:m], out[1][:m], out[2][:m] = torch.tensor(query, dtype=torch.long)[order], torch.tensor(answer, dtype=torch.long)[order], score[order]
    return out


def poison(ids, scores, n_rows):
    """Garbage in the rows at and beyond n_rows: ids that look present, NaN and +inf scores."""
    ids, scores = ids.clone(), scores.clone()
    ids[n_rows:] = 7
    scores[n_rows:] = NAN
    scores[n_rows:, ::2] = INF
    return ids, scores


@pytest.mark.parametrize("min_score", [None, -INF, 0.0, 0.5])
@pytest.mark.parametrize("k", [1, 7, 256])
@pytest.mark.parametrize("n_rows", [None, 0, 1, 5])
def test_three_successive_merges_equal_one_stable_sort(n_rows, k, min_score):
    """Ties across queries and ids, NaN, +-inf, +-0.0, a genuine -inf beside pads, a row of pads alone, n_rows in {0, 1, batch}
    with garbage in the ignored rows, k beyond the number of candidates (256), min_score None / -inf / 0.0 / a value some scores
    equal (0.5: excluded)."""
    batch, k_row = 5, 6
    batches, best, base = [], predict.empty_pairs(k), 0
    for step in range(3):
        ids, scores = a_batch(batch, k_row, seed=10 * step + k, all_pads_row=2 if step == 1 else None)
        rows = n_rows if step == 1 else None              # the middle batch is the short one
        if rows is not None:
            ids, scores = poison(ids, scores, rows)
        batches.append((ids, scores, base, rows))
        best = predict.merge_pairs_reference(best, ids, scores, base, rows, min_score)
        base += batch if rows is None else rows
        so_far = one_sort(batches, k, min_score)          # ... and every intermediate list is the sort of what came so far
        assert torch.equal(best[0], so_far[0]) and torch.equal(best[1], so_far[1]) and same_bits(best[2], so_far[2])
        assert int(best[3]) == so_far[3]
    assert bool((best[0][int(best[3]):] == -1).all()) and bool((best[1][int(best[3]):] == -1).all())
    assert bool((best[2][int(best[3]):] == -INF).all())
    if k == 256:
        assert int(best[3]) < k                           # fewer candidates than slots
    if min_score == 0.5:
        assert not bool((best[2][:int(best[3])] == 0.5).any()) and not bool(best[2].isnan().any())
    if min_score is None and n_rows != 0:
        assert bool(best[2][0].isnan())                   # NaN ranks first


def test_the_order_among_equal_scores_is_query_then_id():
    ids = torch.tensor([[4, 9, -1], [2, 4, 11], [3, -1, -1]])
    scores = torch.tensor([[1.0, 1.0, -INF], [1.0, 1.0, 0.0], [1.0, -INF, -INF]])
    best = predict.merge_pairs_reference(predict.empty_pairs(4), ids[:1], scores[:1], 0)
    best = predict.merge_pairs_reference(best, ids[1:], scores[1:], 1)
    assert best[0].tolist() == [0, 0, 1, 1] and best[1].tolist() == [4, 9, 2, 4] and int(best[3]) == 4
    best = predict.merge_pairs_reference(predict.empty_pairs(8), ids, scores, 20)
    assert best[0].tolist() == [20, 20, 21, 21, 22, 21, -1, -1] and best[1].tolist() == [4, 9, 2, 4, 3, 11, -1, -1]
    zeros = predict.merge_pairs_reference(predict.empty_pairs(2), torch.tensor([[5], [3]]), torch.tensor([[-0.0], [0.0]]), 0)
    assert zeros[0].tolist() == [0, 1] and same_bits(zeros[2], torch.tensor([-0.0, 0.0]))       # -0.0 == +0.0: the query decides


def test_merge_pairs_argument_errors():
    best = predict.empty_pairs(4)
    ids, scores = torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 3)
    with pytest.raises(ValueError):
        predict.empty_pairs(0)
    with pytest.raises(ValueError):
        predict.empty_pairs(257)
    with pytest.raises(TypeError):
        predict.merge_pairs_reference(best, ids, scores[:, :2], 0)
    with pytest.raises(TypeError):
        predict.merge_pairs_reference(best, ids.int(), scores, 0)
    with pytest.raises(ValueError):
        predict.merge_pairs_reference(best[:3], ids, scores, 0)
    with pytest.raises(ValueError):
        predict.merge_pairs_reference(best, ids, scores, 0, min_score=NAN)
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict.merge_pairs(best, ids, scores, 0)


def test_the_library_exports_the_entry_and_answers_bad_arguments_before_any_pointer():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ultra_topk_pairs_merge")
    assert _lib.lib.ultra_abi_version() == 7
    call = _lib.lib.ultra_topk_pairs_merge
    p = 8          # (a pointer that is never looked at)
    for batch, k_row, k in ((1, 0, 5), (1, 257, 5), (1, 5, 0), (1, 5, 257), (-1, 5, 5), (65536, 5, 5)):
        assert call(None, None, batch, k_row, None, None, None, None, None, None, None, k, None) == _lib.ULTRA_ERR_UNSUPPORTED
        assert b"ultra_topk_pairs_merge" in _lib.lib.ultra_last_error()
    for missing in (0, 1, 4, 7, 8, 9, 10):
        args = [p, p, 1, 5, p, None, None, p, p, p, p, 5, None]
        args[missing] = None
        assert call(*args) == _lib.ULTRA_ERR_INVALID, missing
        assert b"NULL" in _lib.lib.ultra_last_error()
    assert call(p, p, 0, 5, p, None, None, p, p, p, p, 5, None) == _lib.ULTRA_OK          # batch 0: nothing is launched


# ---- Predictor, the CPU route ----
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
    assert data.num_nodes == 300 and data.filtered_data is not None
    return model.eval(), data


HEADS = [5, 3, 3, 17, 100, 42, 7, 5, 250]          # duplicates, not ascending; 7 distinct: batch_size 4 leaves a short batch
DISTINCT = sorted(set(HEADS))


def equal_pairs(got, want, anchors=None):
    """`got` of a Predictor call against best_reference's (query, ids, scores, count); anchors: got[0] names entities."""
    first = want[0] if anchors is None else torch.where(want[0] >= 0, anchors[want[0].clamp(min=0)], want[0])
    return (torch.equal(got[0], first) and torch.equal(got[1], want[1]) and same_bits(got[2], want[2])
            and int(got[3]) == int(want[3]))


def reference(model, p, anchors, r, k, mode="tail", **kwargs):
    """best_reference on the graph the predictor serves -- its edits folded in, its rows kept --, with its live count and retired
    ids."""
    graph = p.data if p.delta is None else p.delta.materialize(p.data)
    select = {}
    if p.entity_capacity:
        select["num_live"] = p.num_entities
    if p.num_retired:
        select["retired"] = p.retired_entities
    return predict.best_reference(model, graph, p.filter_graph, anchors, torch.full_like(anchors, r), k, mode, **select, **kwargs)


def stated(graph, heads, r, tails):
    """Which of the triples (heads[i], r, tails[i]) are edges of `graph`?"""
    key = (graph.edge_index[0] * graph.num_nodes + graph.edge_index[1]) * graph.num_relations + graph.edge_type
    return torch.isin((heads * graph.num_nodes + tails) * graph.num_relations + r, key)


def test_propose_tails_and_best_tails_equal_best_reference(served):
    model, data = served
    p = predict.Predictor(model, data, k=10, batch_size=4)
    anchors = torch.tensor(DISTINCT)
    got = p.propose_tails(2, heads=HEADS, k=12)
    assert equal_pairs(got, reference(model, p, anchors, 2, 12), anchors)
    assert int(got[3]) == 12 and not bool(stated(p.filter_graph, got[0], 2, got[1]).any())       # no stated fact is proposed
    got = p.propose_tails(2, heads=HEADS)                                   # k defaults to the predictor's
    assert got[0].shape == (10,) and equal_pairs(got, reference(model, p, anchors, 2, 10), anchors)
    capped = p.propose_tails(2, heads=HEADS, k=12, per_head=2)
    assert equal_pairs(capped, reference(model, p, anchors, 2, 12, per_query=2), anchors)
    assert int(torch.bincount(capped[0][:int(capped[3])]).max()) <= 2
    p.define_set("some", HEADS)
    assert equal_pairs(p.propose_tails(2, heads="some", k=12), reference(model, p, anchors, 2, 12), anchors)
    shortlist = list(range(0, 300, 7))
    got = p.propose_tails(2, heads=HEADS, k=12, among=shortlist)
    assert equal_pairs(got, reference(model, p, anchors, 2, 12, among=torch.tensor(shortlist)), anchors)
    assert bool(torch.isin(got[1][:int(got[3])], torch.tensor(shortlist)).all())
    # a floor: the median of the unfloored proposals, so that some scores fall on either side of it
    floor = float(capped[2][6])
    got = p.propose_tails(2, heads=HEADS, k=12, per_head=2, min_score=floor)
    assert equal_pairs(got, reference(model, p, anchors, 2, 12, per_query=2, min_score=floor), anchors)
    assert 0 < int(got[3]) < 12 and bool((got[2][:int(got[3])] > floor).all()) and bool((got[0][int(got[3]):] == -1).all())
    # the other direction, and any query list through best_tails
    got = p.propose_heads(2, tails=HEADS, k=12)
    want = reference(model, p, anchors, 2, 12, mode="head")
    assert torch.equal(got[0], want[1]) and same_bits(got[2], want[2]) and int(got[3]) == int(want[3])
    assert torch.equal(got[1], torch.where(want[0] >= 0, anchors[want[0].clamp(min=0)], want[0]))
    assert not bool(stated(p.filter_graph, got[0], 2, got[1]).any())
    h, r = torch.tensor([9, 9, 4, 30, 9]), torch.tensor([0, 3, 1, 1, 0])      # repeated queries, several relations
    got = p.best_tails(h, r, k=9, per_query=4)
    want = predict.best_reference(model, p.data, p.filter_graph, h, r, 9, per_query=4)
    assert equal_pairs(got, want)
    assert equal_pairs(p.best_heads(h, r, k=9), predict.best_reference(model, p.data, p.filter_graph, h, r, 9, "head"))
    empty = p.best_tails([], [], k=3)
    assert empty[0].tolist() == [-1] * 3 and int(empty[3]) == 0


def test_proposals_follow_the_live_graph(served):
    model, data = served
    p = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=4)
    anchors = torch.tensor(DISTINCT)
    first = p.propose_tails(2, heads=HEADS, k=6)
    assert equal_pairs(first, reference(model, p, anchors, 2, 6), anchors)
    h0, t0 = int(first[0][0]), int(first[1][0])
    p.add_facts(h0, 2, t0)                                  # the best proposal is stated: it is proposed no more
    after = p.propose_tails(2, heads=HEADS, k=6)
    assert equal_pairs(after, reference(model, p, anchors, 2, 6), anchors)
    assert (h0, t0) not in set(zip(after[0].tolist(), after[1].tolist()))
    p.remove_facts(h0, 2, t0)
    again = p.propose_tails(2, heads=HEADS, k=6)
    assert equal_pairs(again, reference(model, p, anchors, 2, 6), anchors)
    assert (h0, t0) in set(zip(again[0].tolist(), again[1].tolist()))
    (new,) = p.add_entities().tolist()
    assert new == 300
    grown = torch.tensor(DISTINCT + [new])
    got = p.propose_tails(2, heads=HEADS + [new], k=6)
    assert equal_pairs(got, reference(model, p, grown, 2, 6), grown)
    victim = int(again[1][1])                               # a proposed tail is retired: never proposed again
    gone_head = 42
    p.remove_entities([victim, gone_head])
    kept = torch.tensor([v for v in DISTINCT if v not in (victim, gone_head)])
    got = p.propose_tails(2, heads=kept, k=6)
    assert equal_pairs(got, reference(model, p, kept, 2, 6), kept)
    assert victim not in got[1].tolist()
    with pytest.raises(ValueError, match="retired"):
        p.propose_tails(2, heads=HEADS)
    with pytest.raises(ValueError):
        p.propose_tails(2, heads=[3, 302])                  # a reserved row
    with pytest.raises(ValueError):
        p.best_tails([gone_head], [2])
    p.define_set("some", HEADS + [302])                     # by name: the ids that are in use
    assert equal_pairs(p.propose_tails(2, heads="some", k=6), reference(model, p, kept, 2, 6), kept)


def test_every_entity_in_use_is_a_head_by_default(served):
    model, _ = served
    small = synthetic.make_kg(num_node=24, num_triple=90, num_relation_base=3, num_test=4, seed=5)
    p = predict.Predictor(model, small, k=5, batch_size=4, entity_capacity=2)
    p.remove_entities([7])
    everyone = torch.tensor([v for v in range(24) if v != 7])
    got = p.propose_tails(1, k=30)
    assert equal_pairs(got, reference(model, p, everyone, 1, 30), everyone)
    assert 7 not in got[0].tolist() and 7 not in got[1].tolist() and int(got[1].max()) < 24


def test_argument_errors(served):
    model, data = served
    p = predict.Predictor(model, data, k=10, batch_size=4)
    for k in (0, 257, 2.0):
        with pytest.raises(ValueError):
            p.propose_tails(2, heads=HEADS, k=k)
        with pytest.raises(ValueError):
            p.best_tails([1], [2], k=k)
    for per in (0, 11, True):
        with pytest.raises(ValueError, match="per_head"):
            p.propose_tails(2, heads=HEADS, per_head=per)
    with pytest.raises(ValueError):
        p.propose_tails(7, heads=HEADS)                     # an inverse relation
    with pytest.raises(ValueError):
        p.propose_tails([1, 2], heads=HEADS)                # one relation a call
    with pytest.raises(ValueError):
        p.propose_tails(2, heads=[1, 300])
    with pytest.raises(KeyError):
        p.propose_tails(2, heads="nobody")
    with pytest.raises(ValueError):
        p.propose_tails(2, heads=HEADS, min_score=NAN)
    with pytest.raises(TypeError):
        p.best_tails([1], [2], assuming=torch.zeros(0, 3, dtype=torch.long))
