"""The selections among a candidate list per row, kernels and predictors, on the GPU.

The expectation is never the code under test: it is the PARENT kernel (ultra_filtered_topk / _above / _rank and their _alive
twins) given known u complement(among) as its list -- or, for the predictors, a fresh predictor's full ranking restricted on the
host.  count, size and num_negative are recomputed here from boolean masks."""
import pytest
import torch

from ultra_amd import _lib, models, predict, synthetic
from ultra_amd.live import retired_words

pytestmark = pytest.mark.gpu

N, BATCH, CHUNK = 9000, 3, 4096
SPECIAL = {17: float("nan"), 4100: float("inf"), 8000: float("-inf"), 333: -0.0}      # placed inside the longer lists
RETIRED = [5, 31, 32, 4096, 8990]          # listed below; their slots hold NaN / +inf in the `alive` variant
LIVE = N - 5                                # ... and so do the slots at and beyond the live count


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def scores(dev, variant, seed=3):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(0, 20, (BATCH, N), generator=g).float() * 0.25          # quantised: ties abound
    for v, x in SPECIAL.items():
        pred[:, v] = x
    pred[1, 333] = 0.0                     # (+0.0 and -0.0 tie, the id decides)
    if variant == "alive":
        pred[:, RETIRED] = float("nan")
        pred[:, LIVE:] = float("inf")
        pred[0, RETIRED[1]] = float("inf")
    return pred.to(dev)


def a_list(length, seed):
    """`length` ascending distinct ids: 0 and N - 1, the special ids, retired ids and ids beyond LIVE first, then random ones."""
    g = torch.Generator().manual_seed(seed)
    first = [0, N - 1] + list(SPECIAL) + RETIRED + [LIVE, LIVE + 2]
    rest = [v for v in torch.randperm(N, generator=g).tolist() if v not in set(first)]
    return torch.tensor(sorted((first + rest)[:length]), dtype=torch.long)


def operands(variant, dev):
    """(kwargs of the wrappers, (N) bool mask of the ids that exist)."""
    alive = torch.ones(N, dtype=torch.bool)
    if variant == "plain":
        return {}, alive
    alive[LIVE:] = False
    alive[RETIRED] = False
    retired = (retired_words(RETIRED, N, device=dev), torch.tensor([len(RETIRED)], dtype=torch.long, device=dev))
    return {"num_live": torch.tensor([LIVE], dtype=torch.long, device=dev), "retired": retired}, alive


def lists_of(masks, dev):
    """(ptr, index) on the device: per row the ids whose mask is set, ascending."""
    rows, ids = torch.stack(masks).nonzero().t()
    ptr = torch.searchsorted(rows.contiguous(), torch.arange(len(masks) + 1))
    return ptr.to(dev), ids.contiguous().to(dev)


def case(lengths, variant, dev, seed, known_mode="mixed"):
    """One call's operands: lists of the given lengths (stored back to back), known lists, and the masks of the expectation."""
    lists = [a_list(length, seed + i) for i, length in enumerate(lengths)]
    span = torch.tensor([0] + [len(v) for v in lists]).cumsum(0)
    span = torch.stack([span[:-1], span[1:]], dim=1)
    kwargs, alive = operands(variant, dev)
    g = torch.Generator().manual_seed(seed + 100)
    known, listed = [], []
    for b, ids in enumerate(lists):
        in_list = torch.zeros(N, dtype=torch.bool)
        in_list[ids] = True
        listed.append(in_list)
        kn = torch.zeros(N, dtype=torch.bool)
        if known_mode == "all" or (known_mode == "mixed" and b == 1 and len(ids) > 1):
            kn |= in_list                                       # covering all of the list: count 0, all padding
            kn[torch.randperm(N, generator=g)[:40]] = True
        else:
            kn[torch.randperm(N, generator=g)[:60]] = True      # outside the list, mostly
            if len(ids):
                kn[ids[torch.randperm(len(ids), generator=g)[:max(1, len(ids) // 3)]]] = True      # inside it
        known.append(kn & alive)                                # (the parents want known ids that exist)
    return lists, span.to(dev), torch.cat(lists).to(dev), known, listed, alive, kwargs


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_call(pred, span, index, known, listed, alive, kwargs, k, thresholds, dev, capacity=None):
    """The three _among entries on one batch against the parents under known u complement(among)."""
    ptr, kidx = lists_of(known, dev)
    left = [li & alive & ~kn for li, kn in zip(listed, known)]                    # eligible and not known
    c_ptr, c_idx = lists_of([alive & ~m for m in left], dev)                      # the parents' deny list
    among = dict(among=(span, index), among_capacity=capacity)
    ids, top, count = predict.filtered_topk(pred, k, ptr, kidx, **kwargs, **among)
    w_ids, w_top, _ = predict.filtered_topk(pred, k, c_ptr, c_idx, **kwargs)
    assert torch.equal(ids, w_ids), (k, ids, w_ids)
    assert same_bits(top, w_top)
    assert count.tolist() == [min(k, int(m.sum())) for m in left]
    assert bool(((ids >= 0).sum(dim=-1) == count).all())
    host = pred.cpu()
    for threshold in thresholds:
        out, a_ids, a_scores, size = predict.filtered_above(pred, threshold, ptr, kidx, **kwargs, **among)
        w_out, w_a_ids, w_a_scores, _ = predict.filtered_above(pred, threshold, c_ptr, c_idx, **kwargs)
        total = int(out[-1])
        assert torch.equal(out, w_out) and torch.equal(a_ids[:total], w_a_ids[:total]), threshold
        assert same_bits(a_scores[:total], w_a_scores[:total])
        members = [int((li & alive & (host[b] > threshold)).sum()) for b, li in enumerate(listed)]
        assert size.tolist() == members, threshold
    # the rank: pos a known id (the parent's contract) -- inside its span where the row has one, outside it otherwise
    rows = [b for b in range(len(known)) if bool(known[b].any())]
    for inside in (True, False):
        pos = []
        for b in rows:
            pool = (known[b] & listed[b]) if inside and bool((known[b] & listed[b]).any()) else (known[b] & ~listed[b])
            pool = pool if bool(pool.any()) else known[b]
            pos.append(int(pool.nonzero()[0]))
        pos = torch.tensor(pos, device=dev)
        sub = torch.tensor(rows, device=dev)
        r_ptr, r_idx = lists_of([known[b] for b in rows], dev)
        rc_ptr, rc_idx = lists_of([alive & ~left[b] for b in rows], dev)
        rank, negative = predict.filtered_rank(pred[sub].contiguous(), pos, r_ptr, r_idx, **kwargs, among=(span[sub].contiguous(), index),
                                               among_capacity=capacity)
        w_rank, _ = predict.filtered_rank(pred[sub].contiguous(), pos, rc_ptr, rc_idx, **kwargs)
        assert torch.equal(rank, w_rank), (inside, rank, w_rank)
        assert negative.tolist() == [int(left[b].sum()) for b in rows]


def span_lengths(k):
    return [0, 1, k - 1, k, k + 1, 4095, 4096, 4097, 8193]


@pytest.mark.parametrize("variant", ["plain", "alive"])
@pytest.mark.parametrize("k", [1, 10, 256])
def test_the_matrix_against_the_parents(k, variant, dev):
    """Span lengths 0, 1, k - 1, k, k + 1, the chunk edge and two partial lists into the merge, three rows a call; known ids inside
    the list, outside it and covering it; ids 0 and N - 1, NaN, +inf, -inf and -0.0 listed; in the `alive` variant listed ids
    beyond the live count and retired ones, with NaN / +inf in every such slot."""
    pred = scores(dev, variant)
    lengths = span_lengths(k)
    for at in range(0, len(lengths), BATCH):
        lists, span, index, known, listed, alive, kwargs = case(lengths[at:at + BATCH], variant, dev, seed=10 * at + k)
        # thresholds with (nearly) no member, about 5 % and every number
        check_call(pred, span, index, known, listed, alive, kwargs, k, (100.0, 4.5, -1.0), dev)
        if variant == "alive":
            ids, _, _ = predict.filtered_topk(pred, k, *lists_of(known, dev), **kwargs, among=(span, index))
            gone = torch.tensor(RETIRED + list(range(LIVE, N)), device=dev)
            assert not bool(torch.isin(ids, gone).any())


def test_known_covering_every_list_gives_all_padding(dev):
    pred = scores(dev, "plain")
    lists, span, index, known, listed, alive, kwargs = case([7, 4097, 300], "plain", dev, seed=5, known_mode="all")
    ids, top, count = predict.filtered_topk(pred, 10, *lists_of(known, dev), among=(span, index))
    assert count.tolist() == [0, 0, 0] and bool((ids == -1).all()) and bool((top == float("-inf")).all())
    out, _, _, size = predict.filtered_above(pred, -1.0, *lists_of(known, dev), among=(span, index))
    assert out.tolist() == [0, 0, 0, 0] and int(size.sum()) > 0
    check_call(pred, span, index, known, listed, alive, kwargs, 10, (-1.0,), dev)


@pytest.mark.parametrize("variant", ["plain", "alive"])
def test_one_span_shared_by_all_rows_and_two_overlapping_spans(variant, dev):
    pred = scores(dev, variant)
    lists, _, _, known, _, alive, kwargs = case([5000, 5000, 5000], variant, dev, seed=77)
    ids = lists[0]
    index = ids.to(dev)
    in_list = torch.zeros(N, dtype=torch.bool)
    in_list[ids] = True
    shared = torch.tensor([[0, 5000]] * BATCH, device=dev)
    check_call(pred, shared, index, known, [in_list] * BATCH, alive, kwargs, 10, (4.5,), dev)
    overlap = torch.tensor([[0, 4200], [100, 5000], [4100, 4300]], device=dev)
    listed = []
    for b, e in overlap.tolist():
        m = torch.zeros(N, dtype=torch.bool)
        m[ids[b:e]] = True
        listed.append(m)
    check_call(pred, overlap, index, known, listed, alive, kwargs, 10, (4.5,), dev)


@pytest.mark.parametrize("variant", ["plain", "alive"])
def test_among_every_id_returns_the_parents_bits(variant, dev):
    pred = scores(dev, variant)
    _, _, _, known, _, alive, kwargs = case([1, 1, 1], variant, dev, seed=9)
    ptr, kidx = lists_of(known, dev)
    among = (torch.tensor([[0, N]] * BATCH, device=dev), torch.arange(N, device=dev))
    for k in (1, 10, 256):
        got = predict.filtered_topk(pred, k, ptr, kidx, **kwargs, among=among)
        want = predict.filtered_topk(pred, k, ptr, kidx, **kwargs)
        assert torch.equal(got[0], want[0]) and same_bits(got[1], want[1]) and torch.equal(got[2], want[2])
    got = predict.filtered_above(pred, 4.5, ptr, kidx, **kwargs, among=among)
    want = predict.filtered_above(pred, 4.5, ptr, kidx, **kwargs)
    total = int(want[0][-1])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1][:total], want[1][:total]) and torch.equal(got[3], want[3])
    assert same_bits(got[2][:total], want[2][:total])
    pos = torch.stack([kn.nonzero()[0, 0] for kn in known]).to(dev)
    assert all(torch.equal(a, b) for a, b in zip(predict.filtered_rank(pred, pos, ptr, kidx, **kwargs, among=among),
                                                 predict.filtered_rank(pred, pos, ptr, kidx, **kwargs)))


def test_a_span_longer_than_the_capacity_is_cut(dev):
    """... and nothing behind the cut is used: the ids there are the row's best (+inf), or no ids at all."""
    pred = scores(dev, "plain")
    lists, span, index, known, listed, alive, kwargs = case([5000, 4097, 20], "plain", dev, seed=21)
    pred[0, lists[0][4096:]] = float("inf")
    index = index.clone()
    index[4096 + 5000:5000 + 4097] = 1 << 40          # row 1: the entry behind the cut is no id
    cut = []
    for ids in lists:
        m = torch.zeros(N, dtype=torch.bool)
        m[ids[:4096]] = True
        cut.append(m)
    check_call(pred, span, index, known, cut, alive, kwargs, 10, (4.5,), dev, capacity=4096)
    ids, _, _ = predict.filtered_topk(pred, 10, None, None, among=(span, index), among_capacity=4096)
    assert not bool(torch.isin(ids[0], lists[0][4096:].to(dev)).any())
    ids, top, count = predict.filtered_topk(pred, 10, None, None, among=(span, index), among_capacity=8)
    assert count.tolist() == [8, 8, 8] and bool((ids[:, 8:] == -1).all())
    assert bool(torch.isin(ids[2, :8], lists[2][:8].to(dev)).all())


def test_ids_that_are_no_ids_are_never_an_index(dev):
    """A negative id and an id >= N inside a list: absent, never loaded, never counted."""
    pred = scores(dev, "plain")
    index = torch.tensor([-(1 << 40), -1, 3, 8, N - 1, N, N + 5, 1 << 35], device=dev)
    span = torch.tensor([[0, 8]] * BATCH, device=dev)
    ids, _, count = predict.filtered_topk(pred, 10, None, None, among=(span, index))
    assert count.tolist() == [3] * BATCH and sorted(ids[0, :3].tolist()) == [3, 8, N - 1]
    _, _, _, size = predict.filtered_above(pred, -1.0, None, None, among=(span, index))
    assert size.tolist() == [3] * BATCH
    span = torch.tensor([[0, 8], [5, 2], [-4, 3]], device=dev)          # an inverted and a negative span are empty
    assert predict.filtered_topk(pred, 10, None, None, among=(span, index), among_capacity=8)[2].tolist() == [3, 0, 0]


def test_two_runs_give_equal_bits(dev):
    pred = scores(dev, "alive")
    lists, span, index, known, listed, alive, kwargs = case([8193, 4097, 300], "alive", dev, seed=31)
    ptr, kidx = lists_of(known, dev)

    def run():
        a = predict.filtered_topk(pred, 256, ptr, kidx, **kwargs, among=(span, index))
        b = predict.filtered_above(pred, 2.0, ptr, kidx, **kwargs, among=(span, index))
        total = int(b[0][-1])
        return [t.clone() for t in a] + [b[0].clone(), b[1][:total].clone(), b[2][:total].clone(), b[3].clone()]

    first, second = run(), run()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(first, second))


def test_a_recorded_call_serves_new_spans_lists_live_count_and_retired_set(dev):
    """torch.cuda.graph around the three wrappers with a fixed capacity; then the spans, the list contents, the live count and
    the retired bitmap are rewritten in place: the replay gives the new expectation, and nothing is recorded again."""
    k, capacity = 10, 2 * CHUNK + 100
    pred = scores(dev, "alive")
    lists, span, index, known, listed, alive, kwargs = case([8193, 4097, 300], "alive", dev, seed=41)
    index = torch.cat([index, index.new_zeros(4096)])
    ptr, kidx = lists_of(known, dev)
    pos = torch.stack([kn.nonzero()[0, 0] for kn in known]).to(dev)
    among = dict(among=(span, index), among_capacity=capacity)
    out = {}

    def step():
        out["topk"] = predict.filtered_topk(pred, k, ptr, kidx, **kwargs, **among)
        out["above"] = predict.filtered_above(pred, 4.5, ptr, kidx, **kwargs, **among)
        out["rank"] = predict.filtered_rank(pred, pos, ptr, kidx, **kwargs, **among)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()

    def verify(listed, alive, live_kwargs):
        graph.replay()
        torch.cuda.synchronize()
        left = [li & alive & ~kn for li, kn in zip(listed, known)]
        c_ptr, c_idx = lists_of([alive & ~m for m in left], dev)
        w = predict.filtered_topk(pred, k, c_ptr, c_idx, **live_kwargs)
        assert torch.equal(out["topk"][0], w[0]) and same_bits(out["topk"][1], w[1])
        assert out["topk"][2].tolist() == [min(k, int(m.sum())) for m in left]
        w = predict.filtered_above(pred, 4.5, c_ptr, c_idx, **live_kwargs)
        total = int(w[0][-1])
        assert torch.equal(out["above"][0], w[0]) and torch.equal(out["above"][1][:total], w[1][:total])
        host = pred.cpu()
        assert out["above"][3].tolist() == [int((li & alive & (host[b] > 4.5)).sum()) for b, li in enumerate(listed)]
        w = predict.filtered_rank(pred, pos, c_ptr, c_idx, **live_kwargs)
        assert torch.equal(out["rank"][0], w[0]) and out["rank"][1].tolist() == [int(m.sum()) for m in left]

    verify(listed, alive, kwargs)
    # new lists of other lengths, in place; two more ids retired, the live count lowered -- the known ids stay alive
    new_lists = [a_list(length, 900 + i) for i, length in enumerate([20, 8200, 4096])]
    offsets = torch.tensor([0] + [len(v) for v in new_lists]).cumsum(0)
    span.copy_(torch.stack([offsets[:-1], offsets[1:]], dim=1))
    index[:int(offsets[-1])].copy_(torch.cat(new_lists))
    free = [v for v in range(100, 200) if not any(bool(kn[v]) for kn in known)][:2]
    live = LIVE - 1 if not any(bool(kn[LIVE - 1]) for kn in known) else LIVE
    kwargs["num_live"].fill_(live)
    kwargs["retired"][0].copy_(retired_words(RETIRED + free, N, device=dev))
    kwargs["retired"][1].fill_(len(RETIRED) + 2)
    alive = alive.clone()
    alive[free] = False
    alive[live:] = False
    listed = []
    for ids in new_lists:
        m = torch.zeros(N, dtype=torch.bool)
        m[ids] = True
        listed.append(m)
    verify(listed, alive, kwargs)


# ---- the predictors ----
NODES, K_FULL, BS = 200, 200, 4


@pytest.fixture(scope="module")
def served(dev):
    torch.manual_seed(0)
    kg = synthetic.make_kg(num_node=NODES, num_triple=1200, num_relation_base=4, num_test=8, seed=13).to(dev)
    model = models.Ultra(**synthetic.default_model_cfg()).to(dev).eval()
    h = torch.tensor([0, 3, 7, 9, 12, 20], device=dev)          # 6 queries, batch_size 4: the last batch is padded
    r = torch.tensor([0, 1, 2, 3, 1, 2], device=dev)
    full = predict.Predictor(model, kg, k=K_FULL, batch_size=BS)
    yield kg, model, h, r, full.tails(h, r), full
    full.close()


@pytest.fixture
def make_predictor():
    """predict.Predictor, closed when the test ends: a captured step left to the garbage collector would unpin its plans in the
    middle of a later test."""
    made = []

    def make(*args, **kwargs):
        made.append(predict.Predictor(*args, **kwargs))
        return made[-1]

    yield make
    for p in made:
        p.close()


def restrict(full, allowed, k, dev):
    """The rows of a full ranking (ids, scores, count) cut down to the `allowed` ids of each row (a list of sets), padded to k."""
    ids, scores, _ = (t.cpu() for t in full)
    out_ids = torch.full((len(ids), k), -1, dtype=torch.long)
    out_scores = torch.full((len(ids), k), float("-inf"))
    count = torch.zeros(len(ids), dtype=torch.long)
    for b in range(len(ids)):
        keep = [j for j in range(ids.shape[1]) if int(ids[b, j]) in allowed[b]][:k]
        out_ids[b, :len(keep)], out_scores[b, :len(keep)], count[b] = ids[b, keep], scores[b, keep], len(keep)
    return out_ids.to(dev), out_scores.to(dev), count.to(dev)


def equal_answers(got, want):
    return torch.equal(got[0], want[0]) and same_bits(got[1], want[1]) and torch.equal(got[2], want[2])


def captures(counter):
    return counter["n"]


@pytest.fixture
def capture_count(monkeypatch):
    """Counts the hipGraph captures made from here on (torch.cuda.CUDAGraph objects created)."""
    counter = {"n": 0}
    real = torch.cuda.CUDAGraph

    def counting(*args, **kwargs):
        counter["n"] += 1
        return real(*args, **kwargs)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", counting)
    return counter


def test_tails_among_equal_the_full_ranking_restricted(served, dev, capture_count, make_predictor):
    kg, model, h, r, full, _ = served
    p = make_predictor(model, kg, k=10, batch_size=BS)
    shared = set(range(0, NODES, 3))
    got = p.tails(h, r, among=sorted(shared))                              # one set for every query
    assert equal_answers(got, restrict(full, [shared] * 6, 10, dev))
    after_first = captures(capture_count)
    assert after_first >= 1 and ("tail", "among") in p._steps and "tail" not in p._steps
    other = set(range(1, NODES, 3))
    got = p.tails(h, r, among=torch.tensor(sorted(other), device=dev))     # another set of the same size
    assert equal_answers(got, restrict(full, [other] * 6, 10, dev))
    assert captures(capture_count) == after_first, "a second call with another set of the same size records nothing"
    per_query = [[1, 5, 199], sorted(shared), [], [4, 4, 2], list(range(NODES)), [0]]
    allowed = [{1, 5, 199}, shared, set(), {2, 4}, set(range(NODES)), {0}]
    got = p.tails(h, r, among=per_query)                                   # one per query, the last batch padded
    assert equal_answers(got, restrict(full, allowed, 10, dev))
    p.define_set("third", sorted(shared))
    got = p.tails(h, r, among="third")                                     # a named set
    assert equal_answers(got, restrict(full, [shared] * 6, 10, dev))
    got = p.tails(h, r, among=["third", [1, 5, 199], "third", [], "third", [0]])
    assert equal_answers(got, restrict(full, [shared, {1, 5, 199}, shared, set(), shared, {0}], 10, dev))
    assert captures(capture_count) == after_first
    assert equal_answers(p.heads(h, r, among="third"),
                         restrict(make_predictor(model, kg, k=K_FULL, batch_size=BS).heads(h, r), [shared] * 6, 10, dev))


def test_tails_above_and_verify_tails_among(served, dev, capture_count, make_predictor):
    kg, model, h, r, full, full_predictor = served
    p = make_predictor(model, kg, k=10, batch_size=BS)
    shared = set(range(0, NODES, 3))
    allowed = [{1, 5, 199}, shared, set(), {2, 4}, set(range(NODES)), {0}]
    per_query = [sorted(s) for s in allowed]
    threshold = float(full[1][:, 20].median())
    out, ids, scores, size = p.tails_above(h, r, threshold, among=per_query)
    w_out, w_ids, w_scores, w_size = full_predictor.tails_above(h, r, threshold)
    known_ptr, known_idx = predict.known_answers(kg, h, r, "tail")
    for b in range(6):
        lo, hi = int(w_out[b]), int(w_out[b + 1])
        keep = [j for j in range(lo, hi) if int(w_ids[j]) in allowed[b]]
        assert ids[int(out[b]):int(out[b + 1])].tolist() == w_ids[keep].tolist()
        assert same_bits(scores[int(out[b]):int(out[b + 1])], w_scores[keep])
        # size counts the members before the known filter: the listed members plus the known ids of the set above the threshold
        row = dict(zip(full[0][b].tolist(), full[1][b].tolist()))
        known = set(known_idx[int(known_ptr[b]):int(known_ptr[b + 1])].tolist())
        assert int(size[b]) >= len(keep) and int(size[b]) <= len(keep) + len(known & allowed[b])
        assert all(row[v] > threshold for v in w_ids[keep].tolist())
    # the type-constrained filtered rank of stated facts
    direct = kg.edge_type < kg.num_relations // 2
    hh, rr, tt = kg.edge_index[0][direct][:6], kg.edge_type[direct][:6], kg.edge_index[1][direct][:6]
    before = captures(capture_count)
    score, rank, negative = p.verify_tails(hh, rr, tt, among=per_query)
    first = captures(capture_count)
    assert first > before
    w_score, w_rank, w_negative = p.verify_tails(hh, rr, tt)
    assert same_bits(score, w_score)
    assert torch.equal(rank[4], w_rank[4]) and torch.equal(negative[4], w_negative[4])        # every id listed: the parent's
    assert int(negative[2]) == 0 and int(rank[2]) == 1                                         # an empty set
    v_ptr, v_idx = predict.known_answers(kg, hh, rr, "tail")
    for b in range(6):
        known = set(v_idx[int(v_ptr[b]):int(v_ptr[b + 1])].tolist())
        assert int(negative[b]) == len(allowed[b] - known)
        assert 1 <= int(rank[b]) <= int(negative[b]) + 1 and int(rank[b]) <= int(w_rank[b])
    after = captures(capture_count)
    p.verify_tails(hh, rr, tt, among=[sorted(set(range(1, NODES, 3)))] * 6)
    assert captures(capture_count) == after


def test_a_predictor_never_given_a_set_calls_the_parents_entries(served, dev, capture_count, monkeypatch, make_predictor):
    kg, model, h, r, full, _ = served
    calls = []
    for name in ("ultra_filtered_topk", "ultra_filtered_topk_live", "ultra_filtered_topk_alive", "ultra_filtered_topk_among",
                 "ultra_filtered_rank", "ultra_filtered_rank_live", "ultra_filtered_rank_alive", "ultra_filtered_rank_among",
                 "ultra_filtered_above", "ultra_filtered_above_live", "ultra_filtered_above_alive", "ultra_filtered_above_among"):
        real = getattr(_lib.lib, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append(_name)
            return _real(*args)

        monkeypatch.setattr(_lib.lib, name, wrapped)
    p = make_predictor(model, kg, k=10, batch_size=BS)
    got = p.tails(h, r)
    assert equal_answers(got, (full[0][:, :10].contiguous(), full[1][:, :10].contiguous(), full[2].clamp(max=10)))
    after_tails = captures(capture_count)
    direct = kg.edge_type < kg.num_relations // 2
    p.verify_tails(kg.edge_index[0][direct][:6], kg.edge_type[direct][:6], kg.edge_index[1][direct][:6])
    after_verify = captures(capture_count)
    p.tails_above(h, r, 0.0)
    p.tails(h, r)
    p.verify_tails(kg.edge_index[0][direct][:6], kg.edge_type[direct][:6], kg.edge_index[1][direct][:6])
    assert set(calls) == {"ultra_filtered_topk", "ultra_filtered_rank", "ultra_filtered_above"}
    # one capture per captured step, as ever: the answer sets run eagerly, a repeated call records nothing
    assert (after_tails, after_verify, captures(capture_count)) == (1, 2, 2) and sorted(p._steps) == ["tail", "verify_tail"]
    p.tails(h, r, among=[0, 1, 2])
    assert "ultra_filtered_topk_among" in calls and sorted(map(str, p._steps)) == sorted(map(str, ["tail", "verify_tail", ("tail", "among")]))


def test_new_and_retired_entities_in_a_named_set(served, dev, make_predictor):
    kg, model, h, r, _, _ = served
    p = make_predictor(model, kg, k=10, batch_size=BS, entity_capacity=4)
    named = [2, 5, 8, 50, 120, NODES]                   # NODES: the first id of the reserve
    p.define_set("s", named)
    got = p.tails(h, r, among="s")
    assert int(got[0].max()) < NODES
    assert int(p.add_entities(1)[0]) == NODES
    with_new = p.tails(h, r, among="s")                 # no define_set in between
    fresh = make_predictor(model, p.materialized(), k=K_FULL + 1, batch_size=BS)
    assert equal_answers(with_new, restrict(fresh.tails(h, r), [set(named)] * 6, 10, dev))
    assert bool((with_new[0] == NODES).any(dim=-1).all())
    p.remove_entities([50])
    without = p.tails(h, r, among="s")
    assert not bool((without[0] == 50).any()) and p.sets() == {"s": 6}
    fresh = make_predictor(model, p.materialized(), k=K_FULL + 1, batch_size=BS)
    assert equal_answers(without, restrict(fresh.tails(h, r), [set(named) - {50}] * 6, 10, dev))
