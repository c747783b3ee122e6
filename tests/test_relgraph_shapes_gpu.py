"""The kernels of csrc/relgraph.hip against the definition of the relation graph (tests/relgraph_cases.py: four fp32 matrix
products over dense incidence matrices on the CPU), at the sizes where they take a path no other test takes.

Relation counts: a bit set of R relations has W = ceil(R / 32) words and a wave walks 64 of them per pass, so 2048 relations
are exactly one pass; 2049 and 2050 start a second one with a partial word, 2080 with a whole one, 3210 (a transductive
benchmark graph with its inverses) has 37 words in it, 4100 needs a third.  1, 31, 32, 33: the edges of one word.
The many case (40 relations, 40,000 entities, 1,200,000 edges) crosses the launch caps: 4096 x 256 threads over edges, 8192 x 4
waves over entities and endpoints, one block of 1024 over the added edges' indices.

Every comparison is exact."""
import pytest
import torch

from tests import relgraph_cases as cases
from ultra_amd import _lib, query_train, rspmm, tasks
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu

STATE = ("adj", "counts", "hbits", "tbits")
UNWRITTEN = 0x7fffffff


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def wide(R):
    return cases.checked("wide", R)


def on_gpu(case, dev, upto=None):
    return Data(edge_index=case.edge_index[:, :upto].contiguous().to(dev), edge_type=case.edge_type[:upto].contiguous().to(dev),
                num_nodes=case.num_nodes, num_relations=case.num_relations)


def state_equals(got, ref):
    """(adj, counts, hbits, tbits) on the GPU against the reference's, shapes and dtypes included."""
    for name, x in zip(STATE, got):
        want = getattr(ref, name)
        assert x.shape == want.shape and x.dtype == want.dtype, name
        assert torch.equal(x.cpu(), want), name
    return True


def upload_state(ref, dev):
    return tuple(getattr(ref, name).to(dev) for name in STATE)


# ---- 1. bits ----
@pytest.mark.parametrize("R", cases.WIDE_RELATIONS)
def test_bits_equal_the_definition(dev, R):
    case, ref = wide(R)
    assert state_equals(tasks.relation_graph_bits(on_gpu(case, dev), incidence=True), ref)


def test_bits_equal_the_definition_past_one_grid_pass(dev):
    case, ref = cases.checked("many")
    assert state_equals(tasks.relation_graph_bits(on_gpu(case, dev), incidence=True), ref)


@pytest.mark.parametrize("R", [33, 2050])
def test_bits_of_a_graph_without_edges(dev, R):
    empty = Data(edge_index=torch.zeros(2, 0, dtype=torch.long, device=dev), edge_type=torch.zeros(0, dtype=torch.long, device=dev),
                 num_nodes=7, num_relations=R)
    got = tasks.relation_graph_bits(empty, incidence=True)
    ref = cases.reference(empty.edge_index, empty.edge_type, 7, R)
    assert int(ref.counts.sum()) == 0 and state_equals(got, ref)
    rg = tasks.relation_graph_from_bits(got[0], got[1])
    assert rg.edge_index.shape == (2, 0) and rg.edge_type.shape == (0,)
    assert rg.edge_index.dtype == rg.edge_type.dtype == torch.int64


# ---- 2. emit ----
def emit_into_prefilled(adj, counts):
    """ultra_relation_graph_emit into outputs that hold -1 everywhere."""
    dev = adj.device
    offsets = torch.cumsum(counts, 0) - counts
    total = int(counts.sum())
    edge_index = torch.full((2, total), -1, dtype=torch.int64, device=dev)
    edge_type = torch.full((total,), -1, dtype=torch.int64, device=dev)
    assert _lib.lib.ultra_relation_graph_emit(adj.data_ptr(), offsets.data_ptr(), adj.shape[1], total, edge_index.data_ptr(),
                                              edge_type.data_ptr(), _lib.stream_of(dev)) == _lib.ULTRA_OK
    return edge_index, edge_type


def list_equals(edge_index, edge_type, ref):
    assert edge_index.shape == ref.edge_index.shape and edge_type.shape == ref.edge_type.shape
    assert edge_index.dtype == edge_type.dtype == torch.int64
    assert torch.equal(edge_index.cpu(), ref.edge_index) and torch.equal(edge_type.cpu(), ref.edge_type)
    return True


@pytest.mark.parametrize("R", cases.WIDE_RELATIONS)
def test_emit_equals_the_definition(dev, R):
    case, ref = wide(R)
    # from the kernel's own bits ...
    rg = tasks.relation_graph_from_bits(*tasks.relation_graph_bits(on_gpu(case, dev)))
    assert list_equals(rg.edge_index, rg.edge_type, ref)
    # ... and, separately, from the reference's words and counts
    adj, counts = ref.adj.to(dev), ref.counts.to(dev)
    rg = tasks.relation_graph_from_bits(adj, counts)
    assert list_equals(rg.edge_index, rg.edge_type, ref) and rg.adjacency_bits is adj
    assert list_equals(*emit_into_prefilled(adj, counts), ref)      # (equal to the list: no -1 is left)


def test_emit_equals_the_definition_on_the_many_case(dev):
    case, ref = cases.checked("many")
    assert list_equals(*emit_into_prefilled(ref.adj.to(dev), ref.counts.to(dev)), ref)


# ---- 3. keep ----
def keep_vector(case, seed):
    """1.0, 0.5, +0.0 and -0.0 at random (half the edges dropped); entity 0's edges of relations 2047 and 2048 dropped, one by
    each zero."""
    g = torch.Generator().manual_seed(seed)
    keep = torch.tensor([1.0, 0.5, 0.0, -0.0])[torch.randint(0, 4, (case.edge_index.shape[1],), generator=g)]
    for relation, zero in ((2047, 0.0), (2048, -0.0)):
        keep[(case.edge_index[0] == 0) & (case.edge_type == relation)] = zero
    dropped = keep == 0
    assert 0.4 < float(dropped.float().mean()) < 0.6
    bits = keep[dropped].view(torch.int32)
    assert bool((bits == 0).any()) and bool((bits != 0).any())       # both zeros
    if case.num_relations > 2048:
        assert int(((case.edge_index[0] == 0) & ((case.edge_type == 2047) | (case.edge_type == 2048)) & dropped).sum()) == 2
    return keep


@pytest.mark.parametrize("R", [33, 2050, 4100])
def test_dropped_edges_equal_the_definition(dev, R):
    case, full = wide(R)
    keep = keep_vector(case, R)
    ref = cases.case_reference(case, keep)
    graph = on_gpu(case, dev)
    adj, counts = query_train.relation_graph_bits_keep(graph, keep.to(dev))
    assert state_equals((adj, counts), ref)
    rg = query_train.build_dropped_relation_graph(graph, keep.to(dev))
    assert list_equals(rg.edge_index, rg.edge_type, ref)
    # which edges of the full relation graph the dropped one still holds
    code = lambda r: (r.edge_type * R + r.edge_index[0]) * R + r.edge_index[1]
    want = torch.isin(code(full), code(ref)).float()
    assert int(want.sum()) == ref.edge_index.shape[1] < len(want)
    graph.relation_graph = Data(edge_index=full.edge_index.to(dev), edge_type=full.edge_type.to(dev), num_nodes=R, num_relations=4)
    assert torch.equal(query_train.relation_graph_keep(graph, keep.to(dev)).cpu(), want)
    # the kernel alone, on the reference's words, into an output that holds NaN (the wrapper above allocates its own output,
    # so a prefill can only be handed to the entry point itself); records outside the graph come back 0 (each of them an edge
    # the dropped graph holds but for the one field)
    (a, b), k = ref.edge_index[:, -1].tolist(), int(ref.edge_type[-1])
    bad = torch.tensor([[-1, b, k], [R, b, k], [a, -1, k], [a, R, k], [a, b, -1], [a, b, 4]]).t()
    n, adj = len(want), ref.adj.to(dev)
    rei = torch.cat([full.edge_index, bad[:2]], dim=1).contiguous().to(dev)
    ret = torch.cat([full.edge_type, bad[2]]).to(dev)
    for count in (n, n + bad.shape[1]):
        index = rei[:, :count].contiguous()
        out = torch.full((count,), float("nan"), dtype=torch.float32, device=dev)
        assert _lib.lib.ultra_relation_graph_edge_keep(adj.data_ptr(), R, index.data_ptr(), ret.data_ptr(), count, out.data_ptr(),
                                                       _lib.stream_of(dev)) == _lib.ULTRA_OK
        assert torch.equal(out[:n].cpu(), want) and torch.equal(out[n:].cpu(), torch.zeros(count - n))


def test_dropped_edges_equal_the_definition_past_one_grid_pass(dev):
    """The keep-aware instance of the per-edge kernel has its own grid-stride loop."""
    case, _ = cases.checked("many")
    keep = keep_vector(case, 5)
    ref = cases.case_reference(case, keep)
    assert int(ref.counts.view(4, -1)[:, cases.MANY_RELATIONS - 2:].min()) > 0      # (the relations of the late edges alone)
    assert state_equals(query_train.relation_graph_bits_keep(on_gpu(case, dev), keep.to(dev)), ref)


# ---- 4. add edges ----
def add_edges(edge_index, edge_type, num_nodes, state):
    """tasks.relation_graph_add_edges on (adj, counts, hbits, tbits); returns the status word, prefilled before the call."""
    adj, counts, hbits, tbits = state
    changed = torch.full((1,), UNWRITTEN, dtype=torch.int32, device=adj.device)
    tasks.relation_graph_add_edges(edge_index, edge_type, num_nodes, hbits, tbits, adj, counts, changed)
    return int(changed)


def added_edges_equal_the_definition(case, ref, split, dev):
    before = cases.reference(case.edge_index[:, :split], case.edge_type[:split], case.num_nodes, case.num_relations)
    state = upload_state(before, dev)
    edge_index, edge_type = case.edge_index[:, split:].contiguous().to(dev), case.edge_type[split:].contiguous().to(dev)
    status = add_edges(edge_index, edge_type, case.num_nodes, state)
    assert state_equals(state, ref)
    assert status == (0 if torch.equal(before.adj, ref.adj) else _lib.RELGRAPH_CHANGED)
    return state, status


@pytest.mark.parametrize("R", [33, 2048, 2050, 4100])
def test_added_edges_equal_the_definition(dev, R):
    case, ref = wide(R)
    split = cases.wide_split(case)      # the added ones: entity 0's, entity 2's, the self loop, the 50 repeats
    state, status = added_edges_equal_the_definition(case, ref, split, dev)
    assert R == 33 or status == _lib.RELGRAPH_CHANGED       # (33 relations: the other entities already carry every pair)
    # every added edge a duplicate: the first 50 again, then the whole list
    for upto in (50, None):
        again = on_gpu(case, dev, upto)
        assert add_edges(again.edge_index, again.edge_type, case.num_nodes, state) == 0
        assert state_equals(state, ref)


def test_added_edges_equal_the_definition_past_one_grid_pass(dev):
    case, ref = cases.checked("many")
    # (the added edges past one grid pass of the per-edge kernel matter: the list without them has other bit sets)
    upto = 100000 + cases.MANY_EDGE_STRIDE
    short = cases.reference(case.edge_index[:, :upto], case.edge_type[:upto], case.num_nodes, case.num_relations)
    assert not torch.equal(short.hbits, ref.hbits) and not torch.equal(short.tbits, ref.tbits)
    _, status = added_edges_equal_the_definition(case, ref, 100000, dev)
    assert status == _lib.RELGRAPH_CHANGED


def test_an_index_out_of_range_in_the_last_of_many_added_edges(dev):
    case, _ = cases.checked("many")
    before = cases.reference(case.edge_index[:, :100000], case.edge_type[:100000], case.num_nodes, case.num_relations)
    state = upload_state(before, dev)
    edge_index, edge_type = case.edge_index[:, 100000:].contiguous().to(dev), case.edge_type[100000:].contiguous().to(dev)
    assert edge_index.shape[1] == 1100000
    edge_index[1, -1] = case.num_nodes
    assert add_edges(edge_index, edge_type, case.num_nodes, state) == _lib.RELGRAPH_OUT_OF_RANGE
    assert state_equals(state, before)


# ---- 5. dense adjacency ----
@pytest.mark.parametrize("R", [1, 16, 17, 33, 48, 100, 1025, 2050])
def test_dense_adjacency_equals_the_definition(dev, R):
    _, ref = wide(R)
    got = tasks.relation_graph_dense_adjacency(ref.adj.to(dev))
    want = ref.dense
    assert got.dtype == torch.uint8 and got.shape == want.shape == (((R + 15) // 16) ** 2 * 1024,)
    assert int(want.sum()) == ref.edge_index.shape[1]
    assert torch.equal(got.cpu(), want)


# ---- 6. the consumer ----
def test_a_graph_delta_keeps_a_wide_relation_graph_current(dev):
    """GraphDelta on 2050 relation slots (1025 direct, 1025 inverse): appended facts whose inverse edges carry the relations
    2047, 2048 and 2049, through the seed and through the resident route.  What is checked is the graph's content, in current();
    `_resident` and the identity of the relation-graph object are read only to know that the route under test -- the bits kept
    resident and updated by ultra_relation_graph_add_edges, not the rebuild from the edge list -- is the one that ran."""
    R = 2050
    case, _ = wide(R)
    data = tasks.build_relation_graph(on_gpu(case, dev))
    delta = rspmm.GraphDelta(data, capacity=16)

    def current():
        full = delta.materialize(data)
        ref = cases.reference(full.edge_index, full.edge_type, case.num_nodes, R)
        got = delta.relation_graph
        assert list_equals(got.edge_index, got.edge_type, ref)
        assert got.adjacency_bits.shape == ref.adj.shape and torch.equal(got.adjacency_bits.cpu(), ref.adj)
        return got

    first = current()
    assert delta.add([281, 0], [1023, 1024], [282, 2]) == 2         # (281, 282: entities without an edge); seeds the state
    assert delta._resident is not None
    second = current()
    assert second is not first and int(delta.edges()[1].max()) == 2049
    assert delta.add(2, 1022, 0) == 3                                # the resident route; inverse relation 2047
    third = current()
    assert third is not second
    assert delta.add(281, 1023, 282) == 4                            # a fact the list holds: nothing changes
    assert current() is third
    assert delta.add([10, 283], [5, 1024], [281, 2]) == 6
    assert current() is not third and delta._resident is not None
