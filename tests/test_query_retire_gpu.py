"""Retiring entities under logical queries, on the GPU: ultra_nonzero_lists_alive against torch.nonzero on the live
prefix with the retired columns deleted (the matrix and tile geometry of tests/test_query_grow_gpu.py; retired slots poisoned; bits
beyond the live count; the launch replayed from a captured graph under a later bitmap and count), and
QueryPredictor.retire_entities end to end against the definition of tests/test_query_retire_cpu.py -- a fresh predictor on
`materialized()` asked for k + num_retired answers, the retired ids dropped -- ids, counts, offsets and sizes equal, scores bit
for bit.

Beside the golden file's 28 queries the end-to-end tests ask three that END in a negation: only those leave 1 - 0 = 1.0 in a
retired slot of the FINAL symbolic set -- the ids the parent and the _live twin would list as entailed answers."""
import pytest
import torch

from tests.test_grow_gpu import counted
from tests.test_query_exec_cpu import load
from tests.test_query_retire_cpu import check_against_definition, postfix
from tests.test_ultraquery_gpu import build_model, golden_graph
from ultra_amd import _lib, query_exec, query_predict, tasks
from ultra_amd.live import retired_words
from ultra_amd.ultraquery import Query

pytestmark = pytest.mark.gpu

ENTRY, TWIN, PARENT = "ultra_nonzero_lists_alive", "ultra_nonzero_lists_live", "ultra_nonzero_lists"
ALIVE_ENTRIES = (ENTRY, "ultra_filtered_topk_alive", "ultra_filtered_above_alive")
LIVE_ENTRIES = (TWIN, "ultra_filtered_topk_live", "ultra_filtered_above_live")
PARENT_ENTRIES = (PARENT, "ultra_filtered_topk", "ultra_filtered_above")
BATCH, SLOTS = 3, 2 * 1024 + 4          # two 1,024-id tiles of the fill kernel plus four
WORDS = (SLOTS + 31) // 32
LIVE_COUNTS = (1, 1023, 1025, 2051, 2052, None)      # (None: n_live == NULL, every slot is below the bound)
POISONS = (1.0, float("nan"), float("inf"))
RESERVE = 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---- the kernel ----
@pytest.fixture(scope="module")
def matrix():
    """tests/test_query_grow_gpu.py's (3, 2052) fp32 matrix on the host, left unchanged: row 0 all zero, row 1 dense, row 2 sparse
    with a NaN at id 0, a -0.0 at id 1 and one of each on both sides of the tile boundary."""
    gen = torch.Generator().manual_seed(2101)
    x = torch.zeros(BATCH, SLOTS)
    x[1] = torch.rand(SLOTS, generator=gen) + 0.5
    x[2] = torch.rand(SLOTS, generator=gen) * (torch.rand(SLOTS, generator=gen) < 0.1)
    x[2, [0, 1022, 1024]] = float("nan")
    x[2, [1, 1023, 1025]] = -0.0
    x[2, 2051] = 0.25
    return x


def retired_set(name, live):
    """The ids of the retired set `name` under `live` live ids (all below SLOTS; some may lie at or beyond `live`)."""
    if name == "id 0":
        return [0]
    if name == "the last live id":
        return [live - 1]
    if name == "one whole word":
        return list(range(32, 64))
    if name == "the tile edge":
        return [1023, 1024]
    if name == "the first tile":
        return list(range(1024))
    if name == "every live id":
        return list(range(live))
    assert name == "one per cent"
    return torch.randperm(SLOTS, generator=torch.Generator().manual_seed(2901))[:SLOTS // 100].tolist()


SETS = ("id 0", "the last live id", "one whole word", "the tile edge", "the first tile", "every live id", "one per cent")


def restatement(x, n_live, retired=()):
    """(ptr, index) in plain torch on the host: torch.nonzero of x[:, :n_live] with the retired columns deleted."""
    n_live = x.shape[1] if n_live is None else n_live
    keep = torch.ones(n_live, dtype=torch.bool)
    keep[torch.tensor([v for v in retired if v < n_live], dtype=torch.long)] = False
    cols = keep.nonzero().flatten()
    sample, at = (x[:, cols] != 0).nonzero().t()
    return torch.searchsorted(sample.contiguous(), torch.arange(x.shape[0] + 1)), cols[at]


class Buffers(object):
    """counts / ptr / index of one raw call, pre-filled with ones."""

    def __init__(self, dev, batch=BATCH, n=SLOTS):
        self.batch, self.n = batch, n
        self.counts = torch.ones(max(1, batch), dtype=torch.int64, device=dev)
        self.ptr = torch.ones(batch + 1, dtype=torch.int64, device=dev)
        self.index = torch.ones(max(1, batch * n), dtype=torch.int64, device=dev)

    def call(self, x, live=None, bits=None, entry=None):
        args = (x.data_ptr(), self.batch, self.n, self.counts.data_ptr(), self.ptr.data_ptr(), self.index.data_ptr(),
                self.batch * self.n)
        if entry is None:
            entry = ENTRY if bits is not None else PARENT if live is None else TWIN
        if entry == ENTRY:
            args += (None if live is None else live.data_ptr(), bits.data_ptr())
        elif entry == TWIN:
            args += (live.data_ptr(),)
        _lib.check(getattr(_lib.lib, entry)(*(args + (_lib.stream_of(x),))))
        return self

    def check(self, want, what):
        want_ptr, want_index = want
        total = len(want_index)
        assert torch.equal(self.ptr.cpu(), want_ptr), what
        assert torch.equal(self.index[:total].cpu(), want_index), what
        assert bool((self.index[total:] == 1).all()), "%s: nothing is written beyond the lists" % what


def scalar(dev, n_live):
    return None if n_live is None else torch.full((1,), n_live, dtype=torch.int64, device=dev)


@pytest.mark.parametrize("name", SETS)
def test_alive_lists_equal_torch_nonzero_without_the_retired_columns(dev, matrix, name):
    for n_live in LIVE_COUNTS:
        live = SLOTS if n_live is None else n_live
        retired = retired_set(name, live)
        what = "%s, n_live=%s" % (name, n_live)
        want = restatement(matrix, n_live, retired)
        if name == "every live id":
            assert len(want[1]) == 0 and want[0].tolist() == [0] * (BATCH + 1)
        bits = retired_words(retired, SLOTS, device=dev)
        assert bits.numel() == WORDS and bits.dtype == torch.int32
        Buffers(dev).call(matrix.to(dev), scalar(dev, n_live), bits).check(want, what)
        # whatever a retired slot holds reaches neither a count nor a list
        for poison in POISONS:
            x = matrix.clone()
            x[:, retired] = poison
            Buffers(dev).call(x.to(dev), scalar(dev, n_live), bits).check(want, "%s, retired slots hold %r" % (what, poison))
        # bits at ids >= n_live (and in the last word's tail beyond n) are never looked at
        if n_live is not None:
            beyond = list(range(n_live, WORDS * 32))
            wide = retired_words(sorted(set(retired) | set(beyond)), WORDS * 32, device=dev)
            assert wide.numel() == WORDS
            Buffers(dev).call(matrix.to(dev), scalar(dev, n_live), wide).check(want, "%s, bits beyond the live count" % what)


@pytest.mark.parametrize("n", [1, 31, 33])
def test_rows_shorter_than_a_word_or_one_past_it(dev, n):
    gen = torch.Generator().manual_seed(n)
    x = torch.rand(1, n, generator=gen) + 0.5
    if n > 1:
        x[0, n // 2] = 0.0
    for retired in ([], [0], [n - 1], list(range(n)), list(range(0, n, 2))):
        bits = retired_words(retired, n, device=dev)
        assert bits.numel() == (n + 31) // 32
        for n_live in (None, n, max(1, n - 1)):
            want = restatement(x, n_live, retired)
            Buffers(dev, 1, n).call(x.to(dev), scalar(dev, n_live), bits).check(want, "n=%d, %s, n_live=%s" % (n, retired, n_live))


def test_an_all_zero_bitmap_is_the_twin_and_the_parent(dev, matrix):
    xd = matrix.to(dev)
    bits = torch.zeros(WORDS, dtype=torch.int32, device=dev)
    for n_live in LIVE_COUNTS:
        live = scalar(dev, n_live)
        other = Buffers(dev).call(xd, live)             # (the parent where n_live is None, the twin otherwise)
        other.check(restatement(matrix, n_live), "the %s after the change, n_live=%s" % (PARENT if live is None else TWIN, n_live))
        mine = Buffers(dev).call(xd, live, bits)
        assert torch.equal(mine.ptr, other.ptr) and torch.equal(mine.index, other.index), n_live
        assert torch.equal(mine.counts, other.counts), n_live


def test_a_captured_launch_reads_the_bitmap_and_the_count_at_replay(dev, matrix):
    x = matrix.clone()
    x[:, 1024:] = 0.0
    x[0, 1024], x[1, 1026], x[2, 1025] = 0.5, float("nan"), 1.0
    xd = x.to(dev)
    retired = [3, 1000]
    live = torch.full((1,), 1024, dtype=torch.int64, device=dev)
    bits = retired_words(retired, SLOTS, device=dev)
    buffers = Buffers(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buffers.call(xd, live, bits)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    buffers.check(restatement(x, 1024, retired), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buffers.call(xd, live, bits)
    # one more retirement in the resident bitmap, and three more live ids
    assert float(x[1, 517]) != 0.0
    bits.copy_(retired_words(retired + [517], SLOTS, device=dev))
    live.fill_(1027)
    buffers.ptr.fill_(1)
    buffers.index.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    want = restatement(x, 1027, retired + [517])
    before = restatement(x, 1024, retired)
    assert len(want[1]) == len(before[1]) + 3 - int((x[:, 517] != 0).sum())
    assert 517 not in want[1].tolist() and {1024, 1025, 1026} <= set(want[1].tolist())
    buffers.check(want, "replayed with id 517 retired and 1027 live ids")


def test_an_empty_batch_and_the_python_entry(dev, matrix):
    xd = matrix.to(dev)
    retired = retired_set("one per cent", SLOTS)
    bits = retired_words(retired, SLOTS, device=dev)
    empty = Buffers(dev, batch=0).call(xd, None, bits)
    assert empty.ptr.tolist() == [0]
    empty = Buffers(dev, batch=0).call(xd, scalar(dev, 5), bits)
    assert empty.ptr.tolist() == [0]
    count = torch.full((1,), len(retired), dtype=torch.int64, device=dev)
    for n_live in (None, 1025):
        want_ptr, want_index = restatement(matrix, n_live, retired)
        for operand in (bits, (bits, count), bits.view(torch.uint32)):
            for num_live in ((None,) if n_live is None else (n_live, scalar(dev, n_live))):
                ptr, index = query_exec.nonzero_lists(xd, num_live=num_live, retired=operand)
                assert torch.equal(ptr.cpu(), want_ptr) and torch.equal(index[:len(want_index)].cpu(), want_index)
    for bad in (bits.cpu(), bits[:WORDS - 1], bits.long(), (bits.cpu(), count)):
        with pytest.raises(ValueError, match="retired"):
            query_exec.nonzero_lists(xd, retired=bad)


# ---- end to end ----
@pytest.fixture(scope="module")
def served(dev):
    """(model, graph, queries): the golden ultraquery weights, the 200-node golden graph with the relation graph the package
    builds for it, and the 28 golden queries plus three that end in a negation."""
    g = load()
    assert len(set(g["type"].tolist())) == 14
    model, graph = build_model(g, dev), tasks.build_relation_graph(golden_graph(g, dev))
    queries = list(g["nested"]) + [(3, (0, -2)), (150, (7, -2)), ((5, (1,)), (78, (4, -2)), (-1,))]
    return model, graph, queries


def predictor(served, **kwargs):
    model, graph, _ = served
    kwargs.setdefault("k", 5)
    return query_predict.QueryPredictor(model, graph, batch_size=8, **kwargs)


def chosen(served, qp):
    """(leaf, median, spare, anchor, r1, r2): three entities no query is anchored at -- one of the smallest degree above zero, one
    of the median degree and one more of a small degree -- and an anchor that no edge of r1 leaves, for a 2p path stated
    through one midpoint."""
    _, graph, queries = served
    n = int(graph.num_nodes)
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    rows = postfix(qp, queries)
    anchors = set(rows[(rows & Query.operation) == 0].tolist())
    degree = torch.bincount(ei[0], minlength=n)
    free = sorted((v for v in range(n) if v not in anchors and int(degree[v]) > 0), key=lambda v: (int(degree[v]), v))
    leaf, spare, median = free[0], free[1], free[len(free) // 2]
    assert len({leaf, spare, median}) == 3
    r1, r2 = 0, 1
    anchor = next(a for a in range(n) if a not in (leaf, median, spare) and not bool(((ei[0] == a) & (et == r1)).any()))
    return leaf, median, spare, anchor, r1, r2


def final_sets(qp, queries):
    """The final symbolic sets of `queries` on the served graph with its edits, through the compiled executor."""
    program = query_exec.compile(postfix(qp, queries), qp.num_slots, qp.graph.num_relations)
    was = qp.model.training
    qp.model.eval()
    with torch.no_grad():
        _, sym = query_exec.execute(qp.model, qp.graph, program, **qp._delta_kwargs())
    qp.model.train(was)
    return sym


@pytest.mark.parametrize("capacity", [0, RESERVE])
def test_retired_entities_end_to_end(dev, served, capacity):
    model, graph, queries = served
    n = int(graph.num_nodes)
    kwargs = dict(entity_capacity=capacity) if capacity else {}
    qp = predictor(served, delta_capacity=64, **kwargs)
    wide = predictor(served, k=n + capacity, delta_capacity=64, **kwargs)        # (k = num_slots: count = the candidates left)
    assert wide.k == wide.num_slots
    leaf, median, spare, anchor, r1, r2 = chosen(served, qp)
    ei = graph.edge_index.cpu()
    # the 2p path anchor -r1-> mid -r2-> tail, stated through ONE midpoint (no other edge of r1 leaves the anchor): a new entity
    # where there is a reserve, an entity of the graph where there is none
    if capacity:
        for p in (qp, wide):
            assert p.add_entities(2).tolist() == [n, n + 1]
        mid, tail = n, n + 1
    else:
        mid = spare
        tail = next(v for v in range(n) if v not in (leaf, median, anchor, mid) and not bool(((ei[0] == mid) & (ei[1] == v)).any()))
    asked = queries[:-3] + [(anchor, (r1, r2))] + queries[-3:]       # (the three that end in a negation stay last)
    path, negations = len(asked) - 4, [len(asked) - 3, len(asked) - 2, len(asked) - 1]
    for p in (qp, wide):
        assert p.add_facts([anchor, mid], [r1, r2], [mid, tail]) == 2
    ids, _, count = wide.answers(asked)
    assert tail not in ids[path, :int(count[path])].tolist(), "the end of the stated path is entailed"
    check_against_definition(qp, asked, model, what="nothing retired")
    gone = []
    for step, v in enumerate((leaf, median, mid)):
        for p in (qp, wide):
            held = 0 if p.delta is None else len(p.delta)
            facts = p.retire_entities(v)
            assert facts.shape == (1,) and int(facts) >= (2 if v == mid else 1)
            if v == mid:
                assert held == 2 and len(p.delta) == 0, "the held facts that name the retired entity have left the delta"
        gone.append(v)
        assert qp.retired_entities.tolist() == sorted(gone) and qp.num_retired == step + 1
        check_against_definition(qp, asked, model, what="retired %s" % gone)
        # k = num_slots: every candidate left is an answer
        (w_ids, _, w_count), _ = check_against_definition(wide, asked, model, what="k = num_slots, retired %s" % gone)[0]
        sym = final_sets(wide, asked)
        assert bool((sym[negations][:, gone] == 1.0).all()), "nothing is zeroed on the way: 1 - 0 in the retired slots"
        alive = (sym[:, :wide.num_entities] != 0)
        alive[:, gone] = False
        assert torch.equal(w_count, wide.num_entities - wide.num_retired - alive.sum(dim=1))
        assert not bool(torch.isin(w_ids, torch.tensor(gone, device=dev)).any())
        # the _alive lists hold num_retired ids fewer per such row than the lists of before
        live = wide._live.num_live_for(True)
        ptr, _ = query_exec.nonzero_lists(sym, **live)
        alive_ptr, _ = query_exec.nonzero_lists(sym, retired=wide._live.retired_operand, **live)
        fewer = (ptr[1:] - ptr[:-1]) - (alive_ptr[1:] - alive_ptr[:-1])
        assert fewer[negations].tolist() == [len(gone)] * 3 and int(fewer.min()) >= 0
    ids, _, count = wide.answers(asked)
    assert count[path].item() == wide.num_entities - 3, "the 2p answer that ran through the midpoint is no longer entailed"
    assert tail in ids[path, :int(count[path])].tolist() and mid not in ids[path].tolist()
    for p in (qp, wide):
        with pytest.raises(ValueError):
            p.answers([(mid, (r2,))])
        with pytest.raises(ValueError):
            p.add_facts(anchor, r1, mid)
    # compacted: the set stays
    bits = qp._live.retired_bits
    qp.compact()
    assert qp.delta is None and qp._live.retired_bits is bits and qp.retired_entities.tolist() == sorted(gone)
    check_against_definition(qp, asked, model, what="compacted")
    if capacity:
        # beyond the reserve: one rebuild, a longer bitmap with the bits kept
        new = qp.add_entities(capacity).tolist()
        assert new[-1] == n + capacity + 1 and qp.num_slots == qp.num_entities + capacity
        assert qp._live.retired_bits.numel() == (qp.num_slots + 31) // 32 and qp.retired_entities.tolist() == sorted(gone)
        assert qp.add_facts(3, 0, new[-1]) == 1
        check_against_definition(qp, asked + [(new[-1], (6,))], model, what="after the overflow rebuild")


@pytest.mark.parametrize("capacity", [0, RESERVE])
def test_entry_counts(dev, served, monkeypatch, capacity):
    model, graph, queries = served
    kwargs = dict(entity_capacity=capacity) if capacity else {}
    calls = counted(monkeypatch, ALIVE_ENTRIES + LIVE_ENTRIES + PARENT_ENTRIES)
    used, unused = (LIVE_ENTRIES, PARENT_ENTRIES) if capacity else (PARENT_ENTRIES, LIVE_ENTRIES)
    qp = predictor(served, **kwargs)
    leaf, median = chosen(served, qp)[:2]
    want = qp.answers(queries), qp.answer_sets(queries, probability=0.5)
    assert all(calls[name] == 0 for name in ALIVE_ENTRIES + unused), calls
    assert all(calls[name] > 0 for name in used), calls
    batches = len(qp.batches(queries))
    assert calls[used[0]] == 2 * batches and calls[used[1]] == batches and calls[used[2]] == batches, "the entries of before"
    before = dict(calls)
    qp.retire_entities(leaf)
    got = qp.answers(queries), qp.answer_sets(queries, probability=0.5)
    assert all(calls[name] == before[name] for name in LIVE_ENTRIES + PARENT_ENTRIES), calls
    assert calls[ENTRY] == 2 * batches and calls[ALIVE_ENTRIES[1]] == batches and calls[ALIVE_ENTRIES[2]] == batches, calls
    assert got[0][0].shape == want[0][0].shape
    # filtered=False: no list entry at all, the selection still _alive, and no retired id is an answer
    loose = predictor(served, filtered=False, k=int(graph.num_nodes) + capacity, **kwargs)
    loose.retire_entities([leaf, median])
    before = dict(calls)
    (ids, _, count), (_, set_ids, _, _) = loose.answers(queries), loose.answer_sets(queries, probability=0.5)
    assert all(calls[name] == before[name] for name in (ENTRY, TWIN, PARENT)), calls
    assert all(calls[name] == before[name] for name in LIVE_ENTRIES + PARENT_ENTRIES), calls
    assert calls[ALIVE_ENTRIES[1]] == before[ALIVE_ENTRIES[1]] + batches and calls[ALIVE_ENTRIES[2]] == before[ALIVE_ENTRIES[2]] + batches
    retired = torch.tensor([leaf, median], device=dev)
    assert not bool(torch.isin(ids, retired).any()) and not bool(torch.isin(set_ids, retired).any())
    assert count.tolist() == [loose.num_entities - 2] * len(queries)
    check_against_definition(loose, queries, model, what="unfiltered")
