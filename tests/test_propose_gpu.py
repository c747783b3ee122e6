"""Link discovery on the GPU: ultra_topk_pairs_merge against merge_pairs_reference (computed on the host; all
four outputs equal, scores compared as bits), and Predictor.propose_tails / propose_heads / best_tails against best_reference --
one forward per query, one stable sort -- bit for bit."""
import pytest
import torch

from ultra_amd import _lib, models, predict, synthetic

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
VALUES = [NAN, INF, 2.0, 0.5, 0.5, 0.25, 0.0, -0.0, -1.5, -INF]       # what a slot may hold: ties, both zeros, the specials


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def poison(ids, scores, n_rows):
    """Garbage in the rows at and beyond n_rows: ids that look present, NaN and +inf scores."""
    ids, scores = ids.clone(), scores.clone()
    ids[n_rows:] = 7
    scores[n_rows:] = NAN
    scores[n_rows:, ::2] = INF
    return ids, scores


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def a_batch(batch, k_row, seed, pool, short=True):
    """(ids, scores) as a row-wise selection writes them: per row distinct ids, scores drawn from `pool`, in the stable descending
    order; short: every row keeps a random number of its slots (0 .. k_row), the rest are -1 / -inf pads."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.sort(torch.randperm(4 * k_row + 50, generator=g)[:k_row]).values for _ in range(batch)])
    scores = torch.as_tensor(pool, dtype=torch.float32)[torch.randint(0, len(pool), (batch, k_row), generator=g)]
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    ids, scores = ids.gather(1, order), scores.gather(1, order)
    if short:
        pad = torch.arange(k_row)[None] >= torch.randint(0, k_row + 1, (batch, 1), generator=g)
        ids[pad], scores[pad] = -1, -INF
    return ids, scores


QUANTISED = [0.25 * v for v in range(-6, 7)]


def check_merge(best, ids, scores, base, dev, n_rows=None, min_score=None):
    """One kernel merge of host operands against the definition; returns the new running list (host)."""
    want = predict.merge_pairs_reference(best, ids, scores, base, n_rows, min_score)
    on_dev = tuple(t.to(dev) for t in best)
    got = predict.merge_pairs(on_dev, ids.to(dev), scores.to(dev), base, n_rows, min_score)
    assert all(a is b for a, b in zip(got, on_dev))                     # in place
    got = tuple(t.cpu() for t in got)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (got, want)
    assert same_bits(got[2], want[2]) and torch.equal(got[3], want[3])
    return want


def test_the_smallest_shape(dev):
    best = check_merge(predict.empty_pairs(1), torch.tensor([[4]]), torch.tensor([[0.5]]), 0, dev)
    assert best[1].tolist() == [4]
    best = check_merge(best, torch.tensor([[9]]), torch.tensor([[0.5]]), 1, dev)         # a tie: the earlier query stays
    assert best[0].tolist() == [0]
    best = check_merge(best, torch.tensor([[2]]), torch.tensor([[0.75]]), 2, dev)
    assert best[0].tolist() == [2] and best[1].tolist() == [2]
    check_merge(best, torch.tensor([[-1]]), torch.tensor([[-INF]]), 3, dev)              # a pad


def test_the_largest_stream_five_trips(dev):
    """(64, 256, 256): 256 + 64 * 256 = 16,640 positions, five trips of 4096 with the survivors carried along."""
    g = torch.Generator().manual_seed(1)
    ids, scores = a_batch(64, 256, 2, torch.randn(4000, generator=g).tolist(), short=False)
    first = check_merge(predict.empty_pairs(256), ids[:3], scores[:3], 0, dev)           # a full running list to start from
    best = check_merge(first, ids, scores, 3, dev)
    assert int(best[3]) == 256 and int(best[0].max()) > 40                               # winners from the last trips too


@pytest.mark.parametrize("k", [10, 256])
def test_all_scores_equal_position_alone_decides(k, dev):
    """Every key shares its score word: more than TOPK_MAX keys pass the floor of the threads' maxima, so the radix select
    runs, down to the position bytes."""
    ids, scores = a_batch(64, 256, 3, [1.0], short=False)
    best = check_merge(predict.empty_pairs(k), ids, scores, 100, dev)
    assert best[0].tolist() == [100 + j // 256 for j in range(k)] and torch.equal(best[1], ids.reshape(-1)[:k])
    again = check_merge(best, ids, scores, 164, dev)                                      # the running list is earlier: it stays
    assert torch.equal(again[0], best[0]) and torch.equal(again[1], best[1])


@pytest.mark.parametrize("min_score", [None, -INF, 0.0, 0.5])
@pytest.mark.parametrize("shape", [(9, 40, 50), (5, 6, 7), (7, 256, 3), (33, 3, 256)])
def test_quantised_scores_with_special_values_four_chained_merges(shape, min_score, dev):
    """Ties across queries and ids, NaN, +-inf, +-0.0, genuine -inf beside pads, rows of pads alone; min_score None / -inf / 0.0 /
    a value some scores equal."""
    batch, k_row, k = shape
    best, base = predict.empty_pairs(k), 0
    for step in range(4):
        ids, scores = a_batch(batch, k_row, 20 + step, VALUES + QUANTISED)
        ids[1], scores[1] = -1, -INF                                                      # a row of pads alone
        best = check_merge(best, ids, scores, base, dev, None, min_score)
        base += batch
    if min_score is None:
        assert bool(best[2][0].isnan())


def test_a_full_running_list_with_old_new_and_interleaved_winners(dev):
    """The update is in place: every survivor is read before any slot is written -- whichever list the winners come from."""
    k = 256
    old_ids, old_scores = a_batch(2, 256, 5, [100.0 + 0.5 * v for v in range(40)], short=False)
    full = check_merge(predict.empty_pairs(k), old_ids, old_scores, 0, dev)
    assert int(full[3]) == k
    low = a_batch(8, 200, 6, [0.5 * v for v in range(40)])
    assert all(torch.equal(a, b) for a, b in zip(check_merge(full, *low, 2, dev), full))              # every winner old
    high = a_batch(8, 200, 7, [500.0 + 0.5 * v for v in range(40)], short=False)
    new = check_merge(full, *high, 2, dev)                                                            # every winner new
    assert int(new[0].min()) >= 2
    mixed = a_batch(8, 200, 8, [90.0 + 0.5 * v for v in range(60)])
    both = check_merge(full, *mixed, 2, dev)                                                          # interleaved
    assert 0 < int((both[0] < 2).sum()) < k
    # a list that is a reversal target: the new winners all rank ABOVE the old ones, which move down inside the same buffers
    few = a_batch(1, 100, 9, [500.0], short=False)
    moved = check_merge(full, *few, 2, dev)
    assert moved[0][:100].tolist() == [2] * 100 and torch.equal(moved[1][100:], full[1][:156])


@pytest.mark.parametrize("n_rows", [0, 1, 5, 6, 99, -3])
def test_rows_beyond_n_rows_are_never_read(n_rows, dev):
    ids, scores = a_batch(6, 30, 11, VALUES + QUANTISED)
    first = check_merge(predict.empty_pairs(20), *a_batch(3, 30, 12, QUANTISED), 0, dev)
    ids, scores = poison(ids, scores, max(0, min(n_rows, 6)))              # ids that look present, NaN / +inf scores
    best = check_merge(first, ids, scores, 3, dev, n_rows=n_rows)
    if n_rows <= 0:
        assert all(torch.equal(a, b) for a, b in zip(best, first))
    assert int(best[0].max()) < 3 + max(0, min(n_rows, 6)) or n_rows <= 0


def test_argument_cases(dev):
    best = tuple(t.to(dev) for t in predict.empty_pairs(5))
    ids, scores = (t.to(dev) for t in a_batch(2, 5, 13, QUANTISED, short=False))
    where = torch.tensor([0], device=dev)
    call = _lib.lib.ultra_topk_pairs_merge
    stream = _lib.stream_of(scores)

    def args(batch=2, k_row=5, k=5, **null):
        a = dict(ids=ids.data_ptr(), scores=scores.data_ptr(), batch=batch, k_row=k_row, base=where.data_ptr(), n_rows=None,
                 min_score=None, q=best[0].data_ptr(), i=best[1].data_ptr(), s=best[2].data_ptr(), c=best[3].data_ptr(), k=k)
        a.update(null)
        return list(a.values()) + [stream]

    for bad in (dict(k=0), dict(k=257), dict(k_row=0), dict(k_row=257), dict(batch=-1), dict(batch=65536)):
        assert call(*args(**bad)) == _lib.ULTRA_ERR_UNSUPPORTED, bad
    for name in ("ids", "scores", "base", "q", "i", "s", "c"):
        assert call(*args(**{name: None})) == _lib.ULTRA_ERR_INVALID, name
    assert call(*args(batch=0)) == _lib.ULTRA_OK
    torch.cuda.synchronize()
    assert int(best[3]) == 0 and bool((best[0] == -1).all())                # nothing ran
    assert call(*args()) == _lib.ULTRA_OK
    torch.cuda.synchronize()
    assert int(best[3]) == 5
    with pytest.raises(TypeError):
        predict.merge_pairs(best, ids, scores.double(), 0)
    with pytest.raises(ValueError):
        predict.merge_pairs(best, ids, scores, torch.tensor([0]))           # a host tensor is no device operand


def test_one_capture_replayed_with_new_operands(dev):
    """torch.cuda.graph around one merge; then scores, query_base, n_rows and min_score are rewritten in place and the count is
    carried from replay to replay: nothing is recorded again."""
    batch, k_row, k = 6, 20, 32
    ids = torch.zeros(batch, k_row, dtype=torch.long, device=dev)
    scores = torch.zeros(batch, k_row, device=dev)
    base, rows = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(1, dtype=torch.long, device=dev)
    low = torch.zeros(1, device=dev)
    best = tuple(t.to(dev) for t in predict.empty_pairs(k))
    first = a_batch(batch, k_row, 30, QUANTISED)
    ids.copy_(first[0]), scores.copy_(first[1]), rows.fill_(batch), low.fill_(-INF)

    def step():
        predict.merge_pairs(best, ids, scores, base, rows, low)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    want = predict.empty_pairs(k)
    best[3].fill_(0)                                                        # (the warm-up and the capture's own run are undone)
    at = 0
    for replay, (n_rows, floor) in enumerate([(batch, -INF), (4, 0.25), (batch, -0.5)]):
        b_ids, b_scores = a_batch(batch, k_row, 31 + replay, QUANTISED + [NAN, INF])
        b_ids, b_scores = poison(b_ids, b_scores, n_rows)
        ids.copy_(b_ids), scores.copy_(b_scores), base.fill_(at), rows.fill_(n_rows), low.fill_(floor)
        graph.replay()
        torch.cuda.synchronize()
        want = predict.merge_pairs_reference(want, b_ids, b_scores, at, n_rows, floor)
        got = tuple(t.cpu() for t in best)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and same_bits(got[2], want[2])
        assert torch.equal(got[3], want[3]), replay
        at += n_rows
    assert int(want[3]) > 0


# ---- the predictors ----
NODES, BS, K = 203, 4, 16
SOME = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200, 202, 7, 7, 150, 99, 61]       # 18 distinct: the last batch is padded


@pytest.fixture(scope="module")
def served(dev):
    torch.manual_seed(0)
    kg = synthetic.make_kg(num_node=NODES, num_triple=1300, num_relation_base=4, num_test=8, seed=17).to(dev)
    degree = torch.bincount(kg.edge_index[0], minlength=NODES)
    assert int(degree.max()) >= 8 * int(degree.median())                    # a hub
    model = models.Ultra(**synthetic.default_model_cfg()).to(dev).eval()
    return kg, model


@pytest.fixture
def make_predictor():
    """predict.Predictor, closed when the test ends (test_among_gpu.py)."""
    made = []

    def make(*args, **kwargs):
        made.append(predict.Predictor(*args, **kwargs))
        return made[-1]

    yield make
    for p in made:
        p.close()


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


def equal_pairs(got, want, anchors=None, swap=False):
    """`got` of a Predictor call against best_reference's (query, ids, scores, count); anchors: the call names entities, in
    got[0] (propose_tails) or with swap in got[1] (propose_heads)."""
    named = want[0] if anchors is None else torch.where(want[0] >= 0, anchors[want[0].clamp(min=0)], want[0])
    first, second = (want[1], named) if swap else (named, want[1])
    return (torch.equal(got[0], first) and torch.equal(got[1], second) and same_bits(got[2], want[2])
            and int(got[3]) == int(want[3]))


def anchors_of(ids, dev):
    return torch.unique(torch.tensor(ids, device=dev))


def test_propose_over_every_head_on_the_static_graph(served, dev, make_predictor, capture_count):
    kg, model = served
    p = make_predictor(model, kg, k=K, batch_size=BS)
    before = p.tails(torch.tensor([0, 9], device=dev), torch.tensor([1, 2], device=dev))
    step = p._steps["tail"]
    everyone = torch.arange(NODES, device=dev)
    assert NODES % BS != 0
    got = p.propose_tails(1)
    assert equal_pairs(got, reference(model, p, everyone, 1, K), everyone)
    assert int(got[3]) == K
    key = (kg.edge_index[0] * NODES + kg.edge_index[1]) * kg.num_relations + kg.edge_type
    assert not bool(torch.isin((got[0] * NODES + got[1]) * kg.num_relations + 1, key).any())          # no stated fact
    made = capture_count["n"]
    assert made >= 1 and sorted(map(str, p._steps)) == sorted(map(str, ["tail", ("tail", "best", K, K)]))
    steps = dict(p._steps)
    some = anchors_of(SOME, dev)
    got = p.propose_tails(2, heads=SOME)                                    # another relation, other heads: nothing is recorded
    assert equal_pairs(got, reference(model, p, some, 2, K), some)
    assert capture_count["n"] == made and dict(p._steps) == steps
    after = p.tails(torch.tensor([0, 9], device=dev), torch.tensor([1, 2], device=dev))
    assert p._steps["tail"] is step and capture_count["n"] == made
    assert torch.equal(before[0], after[0]) and same_bits(before[1], after[1]) and torch.equal(before[2], after[2])


def test_captured_equals_eager_and_the_other_direction(served, dev, make_predictor):
    kg, model = served
    p = make_predictor(model, kg, k=K, batch_size=BS)
    eager = make_predictor(model, kg, k=K, batch_size=BS, use_graph=False)
    anchors = anchors_of(SOME, dev)
    assert len(anchors) % BS != 0
    want = reference(model, p, anchors, 0, K)
    got = p.propose_tails(0, heads=SOME)
    assert equal_pairs(got, want, anchors) and equal_pairs(eager.propose_tails(0, heads=SOME), want, anchors)
    assert not eager._steps
    want = reference(model, p, anchors, 0, K, mode="head")
    assert equal_pairs(p.propose_heads(0, tails=SOME), want, anchors, swap=True)
    assert equal_pairs(eager.propose_heads(0, tails=SOME), want, anchors, swap=True)
    h = torch.tensor([9, 9, 0, 30, 9, 100, 2], device=dev)                  # repeated queries, several relations
    r = torch.tensor([0, 3, 1, 1, 0, 2, 2], device=dev)
    want = predict.best_reference(model, kg, p.filter_graph, h, r, 40, per_query=9)
    assert equal_pairs(p.best_tails(h, r, k=40, per_query=9), want)
    assert equal_pairs(eager.best_tails(h, r, k=40, per_query=9), want)
    assert equal_pairs(p.best_heads(h, r, k=3), predict.best_reference(model, kg, p.filter_graph, h, r, 3, "head"))


def test_among_per_head_and_a_floor(served, dev, make_predictor, capture_count):
    kg, model = served
    p = make_predictor(model, kg, k=K, batch_size=BS)
    anchors = anchors_of(SOME, dev)
    shortlist = list(range(0, NODES, 3))
    got = p.propose_tails(1, heads=SOME, among=shortlist)
    assert equal_pairs(got, reference(model, p, anchors, 1, K, among=torch.tensor(shortlist, device=dev)), anchors)
    assert bool(torch.isin(got[1], torch.tensor(shortlist, device=dev)).all())
    capped = p.propose_tails(1, heads=SOME, per_head=2)
    assert equal_pairs(capped, reference(model, p, anchors, 1, K, per_query=2), anchors)
    assert int(torch.bincount(capped[0]).max()) <= 2
    made = capture_count["n"]
    for floor in (0.0, float(capped[2][K // 2])):                           # the second one cuts the list in the middle
        got = p.propose_tails(1, heads=SOME, per_head=2, min_score=floor)
        assert equal_pairs(got, reference(model, p, anchors, 1, K, per_query=2, min_score=floor), anchors)
        m = int(got[3])
        assert bool((got[2][:m] > floor).all()) and bool((got[0][m:] == -1).all()) and bool((got[2][m:] == -INF).all())
    assert 0 < m < K
    assert capture_count["n"] == made + 1, "a new floor rewrites one device float and records nothing"
    made = capture_count["n"]
    p.propose_tails(1, heads=SOME, k=8)                                     # another k is another step; the first one is kept
    assert p._steps[("tail", "best", 8, 8)].k_best == 8 and capture_count["n"] == made + 1
    p.propose_tails(1, heads=SOME, per_head=2)                              # ... so going back to it records nothing
    p.propose_tails(1, heads=SOME, k=8)
    assert capture_count["n"] == made + 1


def test_proposals_follow_the_live_graph(served, dev, make_predictor, capture_count):
    """add_facts, remove_facts, add_entities into a reserve, remove_entities: bit for bit best_reference on the graph served."""
    kg, model = served
    p = make_predictor(model, kg, k=K, batch_size=BS, entity_capacity=5)
    anchors = anchors_of(SOME, dev)
    first = p.propose_tails(1, heads=SOME)
    assert equal_pairs(first, reference(model, p, anchors, 1, K), anchors)
    h0, t0 = int(first[0][0]), int(first[1][0])
    p.add_facts([h0, 3], [1, 2], [t0, 150])                                 # the best proposal is stated: proposed no more
    got = p.propose_tails(1, heads=SOME)
    assert equal_pairs(got, reference(model, p, anchors, 1, K), anchors)
    assert (h0, t0) not in set(zip(got[0].tolist(), got[1].tolist()))
    hub_edge = int((kg.edge_type[kg.edge_index[0] == 0] < 4).nonzero()[0])
    hub_t, hub_r = int(kg.edge_index[1][kg.edge_index[0] == 0][hub_edge]), int(kg.edge_type[kg.edge_index[0] == 0][hub_edge])
    p.remove_facts([h0, 0], [1, hub_r], [t0, hub_t])                        # ... and retracted again; a fact under the hub goes
    got = p.propose_tails(1, heads=SOME)
    assert equal_pairs(got, reference(model, p, anchors, 1, K), anchors)
    assert (h0, t0) in set(zip(got[0].tolist(), got[1].tolist()))
    made = capture_count["n"]
    new = p.add_entities(2)
    assert new.tolist() == [NODES, NODES + 1]
    p.add_facts([NODES], [1], [int(first[1][1])])
    grown = anchors_of(SOME + [NODES, NODES + 1], dev)
    got = p.propose_tails(1, heads=SOME + [NODES, NODES + 1])
    assert equal_pairs(got, reference(model, p, grown, 1, K), grown)
    assert capture_count["n"] == made, "new entities and further facts cost no capture"
    everyone = torch.arange(NODES + 2, device=dev)
    assert equal_pairs(p.propose_tails(1), reference(model, p, everyone, 1, K), everyone)
    victim = next(v for v in got[1].tolist() if v != 144)
    p.remove_entities([victim, 144])
    kept = torch.tensor([v for v in range(NODES + 2) if v not in (victim, 144)], device=dev)
    got = p.propose_tails(1)                                                # every entity in use: not the retired ones
    assert equal_pairs(got, reference(model, p, kept, 1, K), kept)
    assert victim not in got[1].tolist() and 144 not in got[0].tolist()
    some = torch.tensor([v for v in sorted(set(SOME)) if v not in (victim, 144)], device=dev)
    assert equal_pairs(p.propose_heads(1, tails=some), reference(model, p, some, 1, K, mode="head"), some, swap=True)
    with pytest.raises(ValueError, match="retired"):
        p.propose_tails(1, heads=SOME)
    with pytest.raises(ValueError):
        p.propose_tails(1, heads=[NODES + 3])


def test_the_command_line_tool_proposes_by_name(dev, capsys):
    """tools/predict.py --propose RELATION: the named triples are Predictor.propose_tails' on the same weights; a stated fact is
    not printed; the options it would ignore and an unknown relation end the tool."""
    import importlib.util
    import os
    from ultra_amd import data as udata
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    root = os.path.join(golden, "kg_fixture")
    spec = importlib.util.spec_from_file_location("predict_tool", os.path.join(os.path.dirname(golden), os.pardir, "tools", "predict.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ent, rel = udata.read_vocab(root)
    ckpt = os.path.join(golden, "ultra_3g_model.pt")
    base = ["--data-root", root, "--ckpt", ckpt, "--propose", rel[2]]

    def triples(argv):
        tool.main(argv)
        lines = capsys.readouterr().out.splitlines()
        return [tuple(line.split()[1:4]) for line in lines if line[:3].strip().isdigit()]

    got = triples(base + ["--propose-k", "6"])
    data = udata.load_triples_dir(root).to(dev)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    p = predict.Predictor(model.to(dev).eval(), data, k=6, batch_size=8)
    heads, tails, _, count = p.propose_tails(2)
    p.close()
    assert int(count) == 6 and got == [(ent[h], rel[2], ent[t]) for h, t in zip(heads.tolist(), tails.tolist())]
    # the best proposal, stated first, is proposed no more; a floor above every logit leaves nothing
    after = triples(base + ["--propose-k", "6", "--add-fact", got[0][0], rel[2], got[0][2]])
    assert got[0] not in after and len(after) == 6
    assert triples(base + ["--min-score", "1e30"]) == []
    for bad in (["-k", "3"], ["--head", ent[0]], ["--verify"], ["--propose-k", "0"]):
        with pytest.raises(SystemExit):
            tool.main(base + bad)
    with pytest.raises(SystemExit):
        tool.main(["--data-root", root, "--propose", "no such relation"])
