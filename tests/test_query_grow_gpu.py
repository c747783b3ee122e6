"""Serving logical queries on a growing graph, on the GPU: ultra_nonzero_lists_live against torch.nonzero on the
live prefix (dead slots filled with NaN and with 1.0, the count clamped, the launch replayed from a captured graph under a later
count), and QueryPredictor(entity_capacity=) end to end against a fresh predictor on `materialized()` -- ids, counts, offsets and
sizes equal, scores bit for bit.

Beside the golden file's 28 queries (two of each of the 14 types) the end-to-end tests ask three that END in a negation.  Every
one of the 14 types intersects its negated branch with a positive one, so a reserved slot's symbolic 1 - 0 = 1 meets a 0 there;
only a query whose last operation is a negation, or a union with a negated branch, leaves 1.0 in the reserved slots of the final
set -- the ids ultra_nonzero_lists would list as entailed answers."""
import pytest
import torch

from tests.test_grow_gpu import counted
from tests.test_query_exec_cpu import load
from tests.test_query_live_gpu import same_sets, same_topk
from tests.test_ultraquery_gpu import build_model, golden_graph
from ultra_amd import _lib, query_exec, query_predict, tasks

pytestmark = pytest.mark.gpu

ENTRY, PARENT = "ultra_nonzero_lists_live", "ultra_nonzero_lists"
LIVE_ENTRIES = (ENTRY, "ultra_filtered_topk_live", "ultra_filtered_above_live")
PARENT_ENTRIES = (PARENT, "ultra_filtered_topk", "ultra_filtered_above")
BATCH, SLOTS = 3, 2 * 1024 + 4          # two 1,024-id tiles of the fill kernel plus four
LIVE_COUNTS = (1, 1023, 1024, 1025, 2051, 2052)
RESERVE = 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---- the kernel ----
@pytest.fixture(scope="module")
def matrix():
    """(3, 2052) fp32 on the host, left unchanged: row 0 all zero, row 1 dense, row 2 sparse with a NaN at id 0 (what one live id
    sees), a -0.0 at id 1 and one of each on both sides of the tile boundary."""
    gen = torch.Generator().manual_seed(2101)
    x = torch.zeros(BATCH, SLOTS)
    x[1] = torch.rand(SLOTS, generator=gen) + 0.5
    x[2] = torch.rand(SLOTS, generator=gen) * (torch.rand(SLOTS, generator=gen) < 0.1)
    x[2, [0, 1022, 1024]] = float("nan")
    x[2, [1, 1023, 1025]] = -0.0
    x[2, 2051] = 0.25
    return x


def restatement(x, n_live):
    """(ptr, index) of x[:, :n_live] in plain torch on the host."""
    sample, col = (x[:, :n_live] != 0).nonzero().t()
    return torch.searchsorted(sample.contiguous(), torch.arange(x.shape[0] + 1)), col


class Buffers(object):
    """counts / ptr / index of one raw call, pre-filled with ones."""

    def __init__(self, dev, batch=BATCH, n=SLOTS):
        self.batch, self.n = batch, n
        self.counts = torch.ones(max(1, batch), dtype=torch.int64, device=dev)
        self.ptr = torch.ones(batch + 1, dtype=torch.int64, device=dev)
        self.index = torch.ones(max(1, batch * n), dtype=torch.int64, device=dev)

    def call(self, x, live=None):
        args = (x.data_ptr(), self.batch, self.n, self.counts.data_ptr(), self.ptr.data_ptr(), self.index.data_ptr(),
                self.batch * self.n)
        if live is None:
            _lib.check(_lib.lib.ultra_nonzero_lists(*(args + (_lib.stream_of(x),))))
        else:
            _lib.check(_lib.lib.ultra_nonzero_lists_live(*(args + (live.data_ptr(), _lib.stream_of(x)))))

    def check(self, want, what):
        want_ptr, want_index = want
        total = len(want_index)
        assert torch.equal(self.ptr.cpu(), want_ptr), what
        assert torch.equal(self.index[:total].cpu(), want_index), what
        assert bool((self.index[total:] == 1).all()), "%s: nothing is written beyond the lists" % what


@pytest.mark.parametrize("fill", [float("nan"), 1.0])
def test_live_lists_equal_torch_nonzero_on_the_live_prefix(dev, matrix, fill):
    live = torch.zeros(1, dtype=torch.int64, device=dev)
    for n_live in LIVE_COUNTS:
        x = matrix.clone()
        x[:, n_live:] = fill
        assert float(x[0, :n_live].abs().sum()) == 0.0 and bool(x[2, :n_live].isnan().any())
        xd = x.to(dev)
        live.fill_(n_live)
        twin = Buffers(dev)
        twin.call(xd, live)
        twin.check(restatement(x, n_live), "n_live=%d" % n_live)
        # the parent on the same matrix lists every slot, the filled ones included
        parent = Buffers(dev)
        parent.call(xd)
        parent.check(restatement(x, SLOTS), "parent, n_live=%d" % n_live)
        # the Python entry: the device scalar as it is, or an int
        for num_live in (live, n_live):
            ptr, index = query_exec.nonzero_lists(xd, num_live=num_live)
            want_ptr, want_index = restatement(x, n_live)
            assert torch.equal(ptr.cpu(), want_ptr) and torch.equal(index[:len(want_index)].cpu(), want_index)
    with pytest.raises(ValueError):
        query_exec.nonzero_lists(xd, num_live=SLOTS + 1)
    with pytest.raises(ValueError):
        query_exec.nonzero_lists(xd, num_live=live.to(torch.int32))


def test_the_live_count_is_clamped(dev, matrix):
    xd = matrix.to(dev)
    live = torch.full((1,), SLOTS + 5, dtype=torch.int64, device=dev)
    over = Buffers(dev)
    over.call(xd, live)
    over.check(restatement(matrix, SLOTS), "n_live = n + 5 is n")
    live.fill_(-3)
    under = Buffers(dev)
    under.call(xd, live)
    assert torch.equal(under.ptr.cpu(), torch.zeros(BATCH + 1, dtype=torch.int64))
    assert bool((under.index == 1).all()), "no id is written"
    # an empty batch: ptr_out = [0], written by a kernel
    empty = Buffers(dev, batch=0)
    empty.call(xd, live)
    assert empty.ptr.tolist() == [0]


def test_a_captured_launch_reads_the_count_at_replay(dev, matrix):
    x = matrix.clone()
    x[:, 1024:] = 0.0
    xd = x.to(dev)
    live = torch.full((1,), 1024, dtype=torch.int64, device=dev)
    buffers = Buffers(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buffers.call(xd, live)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buffers.call(xd, live)
    live.fill_(1027)
    xd[0, 1024], xd[1, 1026], xd[2, 1025] = 0.5, float("nan"), 1.0
    x[0, 1024], x[1, 1026], x[2, 1025] = 0.5, float("nan"), 1.0
    buffers.ptr.fill_(1)
    buffers.index.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    want = restatement(x, 1027)
    assert len(want[1]) == len(restatement(x, 1024)[1]) + 3
    buffers.check(want, "replayed at 1027")


# ---- end to end ----
@pytest.fixture(scope="module")
def served(dev):
    """(model, graph, queries): the golden ultraquery weights, the 200-node golden graph with the relation graph the package
    builds for it (what a reserve builds for its padded copy), and the 28 golden queries plus three that end in a negation."""
    g = load()
    assert len(set(g["type"].tolist())) == 14
    model, graph = build_model(g, dev), tasks.build_relation_graph(golden_graph(g, dev))
    queries = list(g["nested"]) + [(3, (0, -2)), (150, (7, -2)), ((5, (1,)), (78, (4, -2)), (-1,))]
    return model, graph, queries


def predictor(served, **kwargs):
    model, graph, _ = served
    return query_predict.QueryPredictor(model, graph, k=5, batch_size=8, **kwargs)


def check_against_fresh(qp, queries, what):
    mat = qp.materialized()
    assert int(mat.num_nodes) == qp.num_entities
    fresh = query_predict.QueryPredictor(qp.model, mat, k=qp.k, batch_size=qp.batch_size)
    got, sets = qp.answers(queries), qp.answer_sets(queries, probability=0.5)
    assert same_topk(got, fresh.answers(queries)), what
    assert same_sets(sets, fresh.answer_sets(queries, probability=0.5)), what
    assert int(got[0].max()) < qp.num_entities and int(sets[1].max()) < qp.num_entities, what
    return got


def test_an_unused_reserve_changes_no_answer(dev, served, monkeypatch):
    model, graph, queries = served
    n = int(graph.num_nodes)
    calls = counted(monkeypatch, LIVE_ENTRIES + PARENT_ENTRIES)
    # a default predictor: the graph itself, the parents' entries
    plain = predictor(served)
    assert plain.graph is graph and plain.live_count is None
    want, want_sets = plain.answers(queries), plain.answer_sets(queries, probability=0.5)
    assert all(calls[name] == 0 for name in LIVE_ENTRIES), calls
    assert all(calls[name] > 0 for name in PARENT_ENTRIES), calls
    before = dict(calls)
    # a reserve: the twins, never a parent
    qp = predictor(served, entity_capacity=RESERVE)
    assert qp.num_slots == n + RESERVE and qp.num_entities == n and qp.graph.edge_index is graph.edge_index
    assert torch.equal(qp.graph.relation_graph.edge_index, graph.relation_graph.edge_index)
    assert torch.equal(qp.graph.relation_graph.edge_type, graph.relation_graph.edge_type)
    got, sets = qp.answers(queries), qp.answer_sets(queries, probability=0.5)
    assert all(calls[name] == before[name] for name in PARENT_ENTRIES), calls
    assert all(calls[name] > 0 for name in LIVE_ENTRIES), calls
    assert same_topk(got, want), "ids, scores (bit for bit) and counts of the plain graph, the negation types included"
    assert same_sets(sets, want_sets)
    assert int(got[0].max()) < n and int(sets[1].max()) < n
    check_against_fresh(qp, queries, "unused reserve")
    # what the twin is for: the final sets of the queries that end in a negation hold 1.0 in every reserved slot
    program = query_exec.compile(torch.stack([torch.tensor(row) for row in qp._rows(queries[-3:-1])]), qp.num_slots,
                                 graph.num_relations)
    _, sym = query_exec.execute(model, qp.graph, program)
    assert bool((sym[:, n:] == 1.0).all())
    ptr, _ = query_exec.nonzero_lists(sym)
    live_ptr, _ = query_exec.nonzero_lists(sym, num_live=qp.live_count)
    assert (ptr[-1] - live_ptr[-1]).item() == 2 * RESERVE
    # filtered=False skips the lists and still selects among live ids only
    loose = predictor(served, entity_capacity=RESERVE, filtered=False)
    plain_loose = predictor(served, filtered=False)
    before = calls[ENTRY]
    assert same_topk(loose.answers(queries), plain_loose.answers(queries)) and calls[ENTRY] == before


def test_new_entities_and_their_facts(dev, served):
    model, graph, queries = served
    n = int(graph.num_nodes)
    ei, et = graph.edge_index.cpu(), graph.edge_type.cpu()
    r1, r2 = 0, 1
    anchor = next(a for a in range(n) if not bool(((ei[0] == a) & (et == r1)).any()))       # no edge of r1 leaves it
    qp = predictor(served, entity_capacity=RESERVE, delta_capacity=16)
    wide = query_predict.QueryPredictor(model, graph, k=n + RESERVE, batch_size=8, entity_capacity=RESERVE)    # (count = live candidates)
    asked = [(n, (r2,)), (anchor, (r1, r2))]        # 1p anchored at the first new entity; 2p whose only path runs through it
    with pytest.raises(ValueError):
        qp.answers(asked)
    for p in (qp, wide):
        assert p.add_entities(2).tolist() == [n, n + 1] and int(p.live_count) == n + 2
        with pytest.raises(ValueError):
            p.add_facts(0, 0, n + 2)
    assert wide.answers(asked)[2].tolist() == [n + 2, n + 2]
    check_against_fresh(qp, queries + asked, "entities without facts")
    direct = int((et < 6).nonzero().flatten()[57])
    tails = [17, 90, n + 1]
    for p in (qp, wide):
        # old -> new; new -> old (twice, through r2); new -> new; and a base fact retracted
        assert p.add_facts([anchor, n, n, n], [r1, r2, r2, r2], [n] + tails) == 4
        assert p.remove_facts(int(ei[0, direct]), int(et[direct]), int(ei[1, direct])).tolist()[0] >= 1
        assert p.graph.edge_index is graph.edge_index and p.delta.edited
    got = check_against_fresh(qp, queries + asked, "edited")
    touched = qp.delta.traversal.rows[:int(qp.delta.traversal.count)].tolist()
    assert n in touched and n + 1 in touched, "reserved rows are touched tails of the traversal fix-up"
    ids, _, count = wide.answers(asked)
    assert count.tolist() == [n + 2 - len(tails)] * 2
    for i in range(2):
        assert not set(tails) & set(ids[i, :int(count[i])].tolist()), "the stated tails are entailed"
    # compacted: the slots and the live count stay
    qp.compact()
    assert qp.delta is None and (qp.num_entities, qp.num_slots) == (n + 2, n + RESERVE)
    assert same_topk(check_against_fresh(qp, queries + asked, "compacted"), got)


def test_beyond_the_reserve(dev, served):
    model, graph, queries = served
    n = int(graph.num_nodes)
    qp = predictor(served, entity_capacity=RESERVE)
    scalar = qp.live_count
    new = qp.add_entities(RESERVE + 1).tolist()
    assert new == list(range(n, n + RESERVE + 1))
    assert (qp.num_entities, qp.num_slots) == (n + RESERVE + 1, n + 2 * RESERVE + 1) and qp.live_count is scalar
    assert int(scalar) == n + RESERVE + 1
    assert qp.add_facts([3, new[-1]], [0, 2], [new[-1], new[0]]) == 2
    check_against_fresh(qp, queries + [(new[-1], (2,)), (3, (0, 2))], "after the overflow rebuild")
