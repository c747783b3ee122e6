"""Candidate sets, the parts that need no GPU: CandidateSets' normalisation, errors and span assembly; the
_reference functions with among= against the parent references under the complement list (counts recomputed by sets in this
file); the argument-order error codes of the three _among entries, which answer before any GPU call; Predictor and
QueryPredictor with among= on the CPU route against a host restatement."""
import pytest
import torch

from tests.test_query_grow_cpu import edge_list_model, folded_queries
from tests.test_query_live_cpu import N as QN, twelve_node_graph
from ultra_amd import _lib, models, predict, query_predict, synthetic
from ultra_amd.candidates import CandidateSets, span_rows

OK, INVALID, UNSUPPORTED = _lib.ULTRA_OK, _lib.ULTRA_ERR_INVALID, _lib.ULTRA_ERR_UNSUPPORTED


# ---- CandidateSets ----
def test_define_set_sorts_deduplicates_and_replaces():
    sets = CandidateSets(20)
    assert sets.define_set("drug", [7, 3, 3, 19, 0, 7]) == 4
    assert sets.resolve("drug", 2)[0][1].tolist() == [0, 3, 7, 19]
    assert sets.resolve("drug", 2)[0][1].dtype == torch.long
    assert sets.define_set("drug", torch.tensor([5, 4], dtype=torch.int32)) == 2          # replaced
    assert sets.define_set("empty", []) == 0
    assert sets.sets() == {"drug": 2, "empty": 0}
    sets.drop_set("empty")
    assert sets.sets() == {"drug": 2}
    with pytest.raises(KeyError):
        sets.drop_set("empty")


def test_the_three_errors():
    sets = CandidateSets(lambda: 20)
    sets.define_set("a", [1, 2])
    with pytest.raises(ValueError, match=r"\[0, 20\)"):
        sets.define_set("b", [1, 20])
    with pytest.raises(ValueError, match=r"\[0, 20\)"):
        sets.resolve([-1, 2], 3)
    with pytest.raises(KeyError, match="nope"):
        sets.resolve("nope", 3)
    with pytest.raises(KeyError, match="nope"):
        sets.resolve(["a", "nope", "a"], 3)
    with pytest.raises(ValueError, match="2 sets for 3 queries"):
        sets.resolve(["a", [1, 2, 3]], 3)
    with pytest.raises(ValueError):
        sets.define_set("f", [0.5, 1.0])
    with pytest.raises(ValueError):
        sets.define_set("", [1])


def test_the_slot_count_is_read_when_a_set_is_defined():
    slots = [10]
    sets = CandidateSets(lambda: slots[0])
    with pytest.raises(ValueError):
        sets.define_set("late", [12])
    slots[0] = 16
    assert sets.define_set("late", [12]) == 1


def test_a_set_named_by_eight_queries_is_stored_once():
    sets = CandidateSets(100)
    sets.define_set("type", [9, 1, 5])
    span, index, longest = sets.assemble("type", 8, torch.device("cpu"))
    assert index.tolist() == [1, 5, 9] and longest == 3
    assert span.shape == (8, 2) and span.dtype == torch.long and span.tolist() == [[0, 3]] * 8
    span, index, longest = sets.assemble(["type"] * 8, 8, torch.device("cpu"))
    assert index.tolist() == [1, 5, 9] and span.tolist() == [[0, 3]] * 8


def test_assembly_of_the_accepted_forms():
    sets = CandidateSets(100)
    sets.define_set("type", [9, 1, 5])
    cpu = torch.device("cpu")
    span, index, longest = sets.assemble([4, 2, 2], 2, cpu)                   # one vector for every query
    assert index.tolist() == [2, 4] and span.tolist() == [[0, 2]] * 2 and longest == 2
    span, index, longest = sets.assemble(torch.tensor([4, 2]), 3, cpu)
    assert index.tolist() == [2, 4] and span.tolist() == [[0, 2]] * 3
    shortlist = torch.tensor([50, 40, 60, 70])
    span, index, longest = sets.assemble(["type", shortlist, [], "type", shortlist], 5, cpu)     # one per query
    assert index.tolist() == [1, 5, 9, 40, 50, 60, 70] and longest == 4
    assert span.tolist() == [[0, 3], [3, 7], [7, 7], [0, 3], [3, 7]]
    assert [v.tolist() for v in span_rows(span, index)] == [[1, 5, 9], [40, 50, 60, 70], [], [1, 5, 9], [40, 50, 60, 70]]
    span, index, longest = sets.assemble([], 0, cpu)
    assert span.shape == (0, 2) and index.numel() == 0 and longest == 0


# ---- the _reference functions: among= against the parent under the complement list ----
def _case(seed, batch=4, n=37):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(-3, 4, (batch, n), generator=g).float() * 0.5           # ties abound
    pred[0, 5], pred[1, 0], pred[2, n - 1], pred[3, 7] = float("nan"), float("inf"), float("-inf"), -0.0
    known = [torch.randperm(n, generator=g)[:int(c)].sort().values for c in torch.randint(0, 9, (batch,), generator=g)]
    among = [torch.randperm(n, generator=g)[:int(c)] for c in (0, 1, 12, n)]       # unsorted: the references go by sets
    among[2] = torch.cat([among[2], among[2][:3]])                                    # ... and repeats do not matter
    ptr = torch.tensor([0] + [len(v) for v in known]).cumsum(0)
    return pred, ptr, torch.cat(known), known, among


def _complement_lists(known, among, n, live, retired):
    """known(b) u complement(eligible ids of among(b)) as (ptr, index) over the ids a parent reference with the same num_live /
    retired may list (alive ones), and the eligible sets."""
    gone = set(retired.tolist()) if retired is not None else set()
    lists, eligible = [], []
    for kn, am in zip(known, among):
        ok = {v for v in am.tolist() if 0 <= v < live and v not in gone}
        eligible.append(ok)
        lists.append(sorted(v for v in range(live) if v not in gone and (v not in ok or v in set(kn.tolist()))))
    ptr = torch.tensor([0] + [len(v) for v in lists]).cumsum(0)
    return ptr, torch.tensor([v for row in lists for v in row], dtype=torch.long), eligible


@pytest.mark.parametrize("num_live, retired", [(None, None), (30, None), (None, [2, 11, 36]), (33, [0, 11, 20, 35])])
@pytest.mark.parametrize("seed", [0, 1])
def test_references_with_among_equal_the_parents_under_the_complement(seed, num_live, retired):
    pred, ptr, index, known, among = _case(seed)
    n = pred.shape[1]
    retired = None if retired is None else torch.tensor(retired)
    live = n if num_live is None else num_live
    gone = set() if retired is None else set(retired.tolist())
    # (the parents want known ids that are alive: drop the others from the lists given to BOTH sides)
    known = [torch.tensor([v for v in kn.tolist() if v < live and v not in gone], dtype=torch.long) for kn in known]
    ptr, index = torch.tensor([0] + [len(v) for v in known]).cumsum(0), torch.cat(known)
    c_ptr, c_index, eligible = _complement_lists(known, among, n, live, retired)
    left = [ok - set(kn.tolist()) for ok, kn in zip(eligible, known)]             # eligible and not known
    kwargs = dict(num_live=num_live, retired=retired)
    for k in (1, 5, 40):
        ids, scores, count = predict.filtered_topk_reference(pred, k, ptr, index, among=among, **kwargs)
        w_ids, w_scores, _ = predict.filtered_topk_reference(pred, k, c_ptr, c_index, **kwargs)
        assert torch.equal(ids, w_ids) and torch.equal(scores.view(torch.int32), w_scores.view(torch.int32))
        assert count.tolist() == [min(k, len(s)) for s in left]
    for threshold in (float("-inf"), 0.0, 0.75, 10.0):
        out, ids, scores, size = predict.filtered_above_reference(pred, threshold, ptr, index, among=among, **kwargs)
        w_out, w_ids, w_scores, _ = predict.filtered_above_reference(pred, threshold, c_ptr, c_index, **kwargs)
        assert torch.equal(out, w_out) and torch.equal(ids, w_ids)
        assert torch.equal(scores.view(torch.int32), w_scores.view(torch.int32))
        assert size.tolist() == [sum(1 for v in ok if float(pred[b, v]) > threshold) for b, ok in enumerate(eligible)]
    # rank: pos is a known id (the parent's contract), listed or not
    pos = torch.tensor([int(kn[0]) if len(kn) else -1 for kn in known])
    rows = [b for b in range(len(known)) if pos[b] >= 0]
    sub = lambda p, i, rows: (torch.tensor([0] + [int(p[b + 1] - p[b]) for b in rows]).cumsum(0),
                              torch.cat([i[int(p[b]):int(p[b + 1])] for b in rows]))
    rank, negative = predict.filtered_rank_reference(pred[rows], pos[rows], *sub(ptr, index, rows), among=[among[b] for b in rows],
                                                     **kwargs)
    # the complement list holds pos too (it is known): the parent's contract
    w_rank, _ = predict.filtered_rank_reference(pred[rows], pos[rows], *sub(c_ptr, c_index, rows), **kwargs)
    assert torch.equal(rank, w_rank)
    assert negative.tolist() == [len(left[b]) for b in rows]
    with pytest.raises(ValueError, match="one id vector per row"):
        predict.filtered_topk_reference(pred, 3, ptr, index, among=among[:2])


# ---- the entries' argument checks: no GPU needed ----
def _topk(k=1, n_cand=10, capacity=4, span=None, listed=None, score=None, outs=None, ws=None, ws_bytes=0, batch=1):
    return _lib.lib.ultra_filtered_topk_among(score, None, None, span, listed, batch, n_cand, capacity, k, outs, outs, outs, ws,
                                              ws_bytes, None, None, None, None)


def _above(threshold=0.0, n_cand=10, capacity=4, span=None, listed=None, score=None, outs=None, ws=None, ws_bytes=0, batch=1,
           room=4):
    return _lib.lib.ultra_filtered_above_among(score, None, None, span, listed, batch, n_cand, capacity, threshold, outs, outs, outs,
                                               room, outs, ws, ws_bytes, None, None, None, None)


def _rank(n_cand=10, capacity=4, span=None, listed=None, score=None, outs=None, batch=1):
    return _lib.lib.ultra_filtered_rank_among(score, outs, outs, outs, span, listed, batch, n_cand, capacity, outs, outs, None, None,
                                              None, None)


def test_unsupported_is_decided_before_any_pointer_is_looked_at():
    for k in (0, -1, _lib.TOPK_MAX + 1):
        assert _topk(k=k) == UNSUPPORTED
    assert _topk(n_cand=1 << 31) == UNSUPPORTED
    assert _above(threshold=float("nan")) == UNSUPPORTED
    assert _above(threshold=float("inf")) == UNSUPPORTED
    assert _above(n_cand=1 << 31) == UNSUPPORTED
    assert _rank(n_cand=1 << 31) == UNSUPPORTED
    assert b"ultra_filtered_rank_among" in _lib.lib.ultra_last_error()


def test_invalid_operands_launch_nothing():
    buf = torch.zeros(64, dtype=torch.long)         # a host buffer: only its address is looked at -- nothing is launched
    p = buf.data_ptr()
    everything = dict(span=p, listed=p, score=p, outs=p)
    assert _topk() == INVALID and _above(threshold=float("-inf")) == INVALID and _rank() == INVALID        # NULL everything
    for call in (_topk, _above, _rank):
        assert call(**dict(everything, span=None)) == INVALID
        assert call(**dict(everything, listed=None)) == INVALID
        assert call(capacity=0, **everything) == INVALID
        assert call(capacity=-3, **everything) == INVALID
        assert call(capacity=1 << 31, **everything) == INVALID
        assert call(n_cand=0, **everything) == INVALID
        assert call(**dict(everything, outs=None)) == INVALID
    # a short workspace, a misaligned one
    need = _lib.lib.ultra_filtered_topk_among_workspace(1, 4, 1)
    assert need == 16        # one chunk: k keys and the chunk's count
    assert _topk(ws=p, ws_bytes=need - 8, **everything) == INVALID
    assert _topk(ws=p + 4, ws_bytes=need, **everything) == INVALID
    need = _lib.lib.ultra_filtered_above_among_workspace(1, 4)
    assert need == _lib.lib.ultra_filtered_above_workspace(1, 4) > 0
    assert _above(ws=p, ws_bytes=need - 8, **everything) == INVALID
    assert _above(ws=p + 4, ws_bytes=need, **everything) == INVALID
    assert _above(ws=p, ws_bytes=need, room=3, **everything) == INVALID          # capacity < batch * among_capacity
    assert b"batch * among_capacity" in _lib.lib.ultra_last_error()
    assert _above(batch=_lib.ABOVE_MAX_BATCH + 1, **everything) == INVALID
    # UNSUPPORTED still comes first
    assert _topk(k=0, **dict(everything, span=None)) == UNSUPPORTED
    # an empty batch is fine
    assert _topk(batch=0, ws=p, ws_bytes=0, **everything) == OK
    assert _above(batch=0, ws=p, ws_bytes=64, room=0, **everything) == OK
    assert _rank(batch=0, **everything) == OK


def test_workspace_functions_answer_minus_one_out_of_range():
    ws = _lib.lib.ultra_filtered_topk_among_workspace
    assert ws(-1, 10, 1) == -1 and ws(1, -1, 1) == -1 and ws(1, 10, 0) == -1 and ws(1, 10, _lib.TOPK_MAX + 1) == -1
    assert ws(1, 1 << 31, 1) == -1
    chunk = _lib.TOPK_CHUNK
    assert ws(3, chunk, 10) == 3 * 11 * 8 and ws(3, chunk + 1, 10) == 3 * 2 * 11 * 8 and ws(0, chunk, 10) == 0
    ws = _lib.lib.ultra_filtered_above_among_workspace
    assert ws(-1, 10) == -1 and ws(1, -1) == -1 and ws(_lib.ABOVE_MAX_BATCH + 1, 10) == -1 and ws(1, 1 << 31) == -1


def test_selection_checks_the_among_pair_once():
    from ultra_amd import selection
    cpu = torch.device("cpu")
    span, index = torch.tensor([[0, 2], [1, 4]]), torch.arange(5)
    assert selection.among_operand(None, 2, 9, cpu) is None
    got = selection.among_operand((span, index), 2, 9, cpu)
    assert got[0] is span and got[1] is index and got[2] == 3           # the longest span
    assert selection.among_operand((span, index), 2, 9, cpu, capacity=4096)[2] == 4096
    for bad in ((span, index.int()), (span[:1], index), (span.t().contiguous().t(), index), [span], (span.tolist(), index)):
        with pytest.raises(ValueError, match="pair"):
            selection.among_operand(bad, 2, 9, cpu)
    with pytest.raises(ValueError, match="among_capacity"):
        selection.among_operand((span, index), 2, 9, cpu, capacity=2.0)


# ---- the predictors on the CPU route ----
@pytest.fixture(scope="module")
def kg():
    return synthetic.make_kg(num_node=40, num_triple=120, num_relation_base=3, num_test=8, seed=11)


@pytest.fixture(scope="module")
def rotate_model():
    torch.manual_seed(0)     # (sum / RotatE: its layers run in plain torch off the GPU)
    return models.Ultra(**synthetic.default_model_cfg(message_func="rotate", aggregate_func="sum")).eval()


def _restricted(ids, scores, allowed, k):
    """The rows of a full ranking (ids, scores) cut down to the `allowed` ids of each row, padded to k."""
    out_ids = torch.full((len(ids), k), -1, dtype=torch.long)
    out_scores = torch.full((len(ids), k), float("-inf"))
    count = torch.zeros(len(ids), dtype=torch.long)
    for b in range(len(ids)):
        keep = [j for j in range(ids.shape[1]) if int(ids[b, j]) in allowed[b]][:k]
        out_ids[b, :len(keep)], out_scores[b, :len(keep)], count[b] = ids[b, keep], scores[b, keep], len(keep)
    return out_ids, out_scores, count


def test_predictor_on_the_cpu_route(kg, rotate_model, monkeypatch):
    n = int(kg.num_nodes)
    h, r = torch.tensor([0, 3, 7, 9, 12, 20]), torch.tensor([0, 1, 2, 0, 1, 2])
    full = predict.Predictor(rotate_model, kg, k=n, batch_size=4).tails(h, r)
    p = predict.Predictor(rotate_model, kg, k=5, batch_size=4)
    assert p.define_set("even", range(0, n, 2)) == n // 2 and p.sets() == {"even": n // 2}
    even = set(range(0, n, 2))
    got = p.tails(h, r, among="even")
    want = _restricted(full[0], full[1], [even] * 6, 5)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    shortlists = [[1, 5, 39], "even", [], [4, 4, 2], torch.arange(n), [0]]
    allowed = [{1, 5, 39}, even, set(), {2, 4}, set(range(n)), {0}]
    got = p.tails(h, r, among=shortlists)
    want = _restricted(full[0], full[1], allowed, 5)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert p.tails(h, r, among="even")[2].max() <= 5
    # the answer sets and the type-constrained rank
    out, ids, scores, size = p.tails_above(h, r, -1e30, among=shortlists)
    w_out, w_ids, w_scores, w_size = p.tails_above(h, r, -1e30)
    for b in range(6):
        keep = [int(j) for j in range(int(w_out[b]), int(w_out[b + 1])) if int(w_ids[j]) in allowed[b]]
        assert ids[int(out[b]):int(out[b + 1])].tolist() == w_ids[keep].tolist()
        assert torch.equal(scores[int(out[b]):int(out[b + 1])], w_scores[keep])
    with pytest.raises(KeyError):
        p.tails(h, r, among="odd")
    with pytest.raises(ValueError, match="2 sets for 6 queries"):
        p.tails(h, r, among=["even", "even"])
    with pytest.raises(ValueError, match=r"\[0, 40\)"):
        p.tails(h, r, among=[0, n])
    # the type-constrained rank: off the GPU verify_* runs the definition loop on a graph that holds an edit (RotatE: the gate
    # of the layer route is held open, as tests/test_verify_live_cpu.py does)
    monkeypatch.setattr(predict, "delta_samples_supported", lambda m: True)
    joined = set(zip(*kg.edge_index.tolist()))
    a, b = next((a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in joined and (b, a) not in joined)
    p.add_facts([a], [0], [b])
    direct = kg.edge_type < kg.num_relations // 2
    hh, rr, tt = kg.edge_index[0][direct][:6], kg.edge_type[direct][:6], kg.edge_index[1][direct][:6]
    score, rank, negative = p.verify_tails(hh, rr, tt, among=shortlists)
    w_score, w_rank, w_negative = p.verify_tails(hh, rr, tt)
    assert p.delta.edited and torch.equal(score, w_score)
    assert bool((negative <= torch.tensor([len(s) for s in allowed])).all()) and int(negative[2]) == 0 and int(rank[2]) == 1
    assert bool((rank >= 1).all()) and bool((rank <= negative + 1).all())
    assert torch.equal(rank[4], w_rank[4]) and torch.equal(negative[4], w_negative[4])       # every id listed: the parent's
    p.drop_set("even")
    assert p.sets() == {}


def test_reserved_and_retired_ids_in_a_set_are_absent_until_alive(kg, rotate_model):
    n = int(kg.num_nodes)
    p = predict.Predictor(rotate_model, kg, k=6, batch_size=4, entity_capacity=4)
    p.define_set("s", [2, 5, 8, n, n + 1])                # two ids of the reserve
    h, r = torch.tensor([0, 3]), torch.tensor([0, 1])
    ids, _, count = p.tails(h, r, among="s")
    assert int(ids.max()) < n and int(count.max()) <= 3
    new = int(p.add_entities(1)[0])
    assert new == n
    ids2, _, count2 = p.tails(h, r, among="s")
    assert bool((ids2 == n).any(dim=-1).all()) and torch.equal(count2, count + 1)      # no define_set in between
    p.remove_entities([5])
    ids3, _, _ = p.tails(h, r, among="s")
    assert not bool((ids3 == 5).any()) and p.sets() == {"s": 5}
    fresh = predict.Predictor(rotate_model, p.materialized(), k=n + 1, batch_size=4)
    full = fresh.tails(h, r)
    want = _restricted(full[0], full[1], [{2, 8, n}] * 2, 6)       # (5 is retired: a fresh predictor would list it)
    got = p.tails(h, r, among="s")
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


def test_query_predictor_on_the_cpu_route():
    graph = twelve_node_graph()
    queries = folded_queries()
    n = len(queries)
    full = query_predict.QueryPredictor(edge_list_model(), graph, k=QN, batch_size=8).answers(queries)
    qp = query_predict.QueryPredictor(edge_list_model(), graph, k=4, batch_size=8)
    qp.define_set("low", [0, 1, 2, 3, 4, 5])
    low = set(range(6))
    got = qp.answers(queries, among="low")
    want = _restricted(full[0], full[1], [low] * n, 4)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    per_query = [[i % QN, (i + 3) % QN, 11] if i % 3 else "low" for i in range(n)]       # follows the query through the grouping
    allowed = [{i % QN, (i + 3) % QN, 11} if i % 3 else low for i in range(n)]
    got = qp.answers(queries, among=per_query)
    want = _restricted(full[0], full[1], allowed, 4)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    out, ids, scores, size = qp.answer_sets(queries, probability=0.45, among=per_query)
    w_out, w_ids, w_scores, _ = qp.answer_sets(queries, probability=0.45)
    for b in range(n):
        keep = [j for j in range(int(w_out[b]), int(w_out[b + 1])) if int(w_ids[j]) in allowed[b]]
        assert ids[int(out[b]):int(out[b + 1])].tolist() == w_ids[keep].tolist()
        assert int(size[b]) >= int(out[b + 1] - out[b]) and int(size[b]) <= len(allowed[b])
    with pytest.raises(ValueError, match="queries"):
        qp.answers(queries, among=["low"])


def test_the_tools_name_an_unknown_entity(tmp_path):
    """--among NAME ... / --among-file FILE of tools/predict.py and tools/query_predict.py: names through the vocabulary."""
    from ultra_amd.candidates import named_ids
    vocab = ["/m/a", "/m/b", "/m/c"]
    listed = tmp_path / "set.txt"
    listed.write_text("/m/c\n\n/m/a\n")
    assert named_ids(vocab) is None
    assert named_ids(vocab, ["/m/b"]) == [1]
    assert named_ids(vocab, ["/m/b"], str(listed)) == [1, 2, 0]
    with pytest.raises(ValueError, match="'/m/zz'"):
        named_ids(vocab, ["/m/a", "/m/zz"])
