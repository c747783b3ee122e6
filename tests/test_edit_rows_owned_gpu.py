"""ultra_rspmm_edit_rows_owned on the GPU (csrc/delta_kernels.hip): delta edges that are live in ONE outer slice each,
beside those live in all.  Per slice s the recomputed rows equal Plan([surviving base ; delta edges with owner in {-1, s}],
exact_order=True).forward on slice s as integer views (-0.0 and NaN count), and a (touched row, slice) with no tombstone key and
no live edge is NOT written: it is poisoned before the call and holds the poison after it.

The graph has the shape of tests/test_live_graph_gpu.py: 300 nodes, 8 direct relations, 2,500 edges with inverses; node 7 heads
300 triples (a row longer than seg_len = 256: a hub) whose other ends lie in [3, 293); node 299 has no edge; node 30's sources are
120 and 180.  n_outer = 3; the overlay is laid out for five queries, so owners 3 and 4 name no slice (4 is rewritten to -2).

ONE overlay holds every case:
  shared (owner -1)   (30, 3, 150), (HUB, 0, 50); tombstones (30, 0, 120) -- rows 30 and 120, where no slice owns anything
  slice 0             (30, 4, 150) twice -- owners -1, 0, 0, 1 at one (row, col) --, the hub below its first column and above its last
  slice 1             (30, 5, 150), (30, 6, 180) -- a base column --, the hub at the columns of base slots TILE - 1 and TILE, and
                      (210, 0, 211): rows touched by slice 1 only
  slice 2             (EMPTY, 1, 10): the edge-less row gets its one edge in slice 2 only
  owner 3 = n_outer   (HUB, 5, 2), (30, 2, 160), (220, 1, 221): live nowhere
  owner -2            (HUB, 6, 298), (EMPTY, 2, 12): live nowhere"""
import pytest
import torch

from ultra_amd import _lib, rspmm, tasks
from ultra_amd.data import Data
from ultra_amd.live import with_facts

pytestmark = pytest.mark.gpu

N, R_DIRECT, OUTER, QUERIES = 300, 8, 3, 5
HUB, EMPTY, MERGE_ROW = 7, 299, 30
TILE = _lib.HUB_TILE


def _triples():
    g = torch.Generator().manual_seed(17)
    count = 946
    h = torch.randint(0, EMPTY, (count,), generator=g)
    t = torch.randint(0, EMPTY, (count,), generator=g)
    r = torch.randint(0, R_DIRECT - 1, (count,), generator=g)
    keep = (h != MERGE_ROW) & (t != MERGE_ROW) & (h != HUB) & (t != HUB)
    h, t, r = h[keep], t[keep], r[keep]
    hub_t = torch.randperm(300, generator=g) % 290 + 3              # (3 .. 292, the first ten twice, in no order)
    hub_t[hub_t == MERGE_ROW] = 31
    hub_t[hub_t == HUB] = 8
    extra_h = torch.tensor([MERGE_ROW, MERGE_ROW, 200])
    extra_t = torch.tensor([120, 180, 201])
    extra_r = torch.tensor([0, 1, 7])
    h = torch.cat([h, torch.full((300,), HUB), extra_h])
    t = torch.cat([t, hub_t, extra_t])
    r = torch.cat([r, torch.randint(0, R_DIRECT - 1, (300,), generator=g), extra_r])
    pad = 1250 - len(h)
    ph = torch.randint(100, 118, (pad,), generator=g)
    pt = torch.randint(230, 290, (pad,), generator=g)
    return torch.cat([h, ph]), torch.cat([t, pt]), torch.cat([r, torch.zeros(pad, dtype=torch.long)])


TRIPLES = _triples()
HUB_COLS = sorted(TRIPLES[1][TRIPLES[0] == HUB].tolist())
SHARED = [(MERGE_ROW, 3, 150), (HUB, 0, 50)]
DEAD = (MERGE_ROW, 0, 120)
OWNED = [
    [(MERGE_ROW, 4, 150), (MERGE_ROW, 4, 150), (HUB, 1, 1), (HUB, 2, 297)],
    [(MERGE_ROW, 5, 150), (MERGE_ROW, 6, 180), (HUB, 3, HUB_COLS[TILE - 1]), (HUB, 4, HUB_COLS[TILE]), (210, 0, 211)],
    [(EMPTY, 1, 10)],
    [(HUB, 5, 2), (MERGE_ROW, 2, 160), (220, 1, 221)],
    [(HUB, 6, 298), (EMPTY, 2, 12)],
]
OTHER = [[(EMPTY, 3, 20)], None, [(HUB, 2, 0), (MERGE_ROW, 1, 120)], None, None]       # the capture test's second filling
POISON = {torch.float32: torch.tensor(0x7FC12345, dtype=torch.int32).view(torch.float32),
          torch.float64: torch.tensor(0x7FF8000012345678, dtype=torch.int64).view(torch.float64)}


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rows_of(facts):
    return {v for h, _, t in facts for v in (h, t)}


class World(object):
    """The base graph and its plan, a delta with the shared edits, the overlay filled with `owned` (owner 4 rewritten to -2),
    the per-slice oracle plans, and the (row, slice) pairs the contract leaves unwritten -- worked out from the facts."""

    def __init__(self, dev, owned=OWNED, shared=SHARED, dead=DEAD):
        h, t, r = TRIPLES
        data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]), edge_type=torch.cat([r, r + R_DIRECT]),
                    num_nodes=N, num_relations=2 * R_DIRECT)
        self.data = data = tasks.build_relation_graph(data.to(dev))
        self.plan = rspmm.Plan(data.edge_index, data.edge_type, N, 2 * R_DIRECT, exact_order=True)
        self.delta = delta = rspmm.GraphDelta(data, capacity=8)
        if shared:
            delta.add(*zip(*shared))
        if dead is not None:
            assert int(delta.remove(*dead)[0]) == 1
        self.overlay = rspmm.AssumedFacts(data, delta, batch_size=QUERIES, per_query=8)
        self.fill(owned)

    def fill(self, owned):
        overlay, data, dev = self.overlay, self.data, self.data.edge_index.device
        overlay.fill(owned)
        overlay.owner[overlay.owner == 4] = -2
        mat = self.delta.materialize(data)
        self.oracles = []
        for s in range(OUTER):
            graph = mat
            if owned[s]:
                graph = with_facts(mat, *(torch.tensor(v, device=dev) for v in zip(*owned[s])))
            self.oracles.append(rspmm.Plan(graph.edge_index, graph.edge_type, N, 2 * R_DIRECT, exact_order=True))
        self.touched = overlay.rows[:int(overlay.count)].tolist()
        key_rows = {int(k) // (2 * R_DIRECT * N) for k in self.delta.dead_keys}
        shared_rows = rows_of(self.delta.facts[:len(self.delta)].tolist())       # ((h, r, t) rows)
        everywhere = key_rows | {int(v) for v in shared_rows}
        assert set(self.touched) == everywhere | set().union(*[rows_of(f or []) for f in owned])
        # (touched row, slice) pairs with no tombstone key and no live edge: not written
        self.unwritten = torch.zeros(OUTER, N, dtype=torch.bool, device=dev)
        for s in range(OUTER):
            live = everywhere | rows_of(owned[s] or [])
            quiet = [row for row in self.touched if row not in live]
            if quiet:
                self.unwritten[s, quiet] = True

    def want(self, rel, x, sum, mul, boundary=None, point=None):
        out = []
        for s, oracle in enumerate(self.oracles):
            kwargs = {}
            if boundary is not None:
                kwargs["boundary"] = boundary[s:s + 1]
            if point is not None:
                kwargs["point"] = (point[0][s:s + 1], point[1][s:s + 1])
            out.append(oracle.forward(rel[s:s + 1], x[s:s + 1], sum=sum, mul=mul, **kwargs))
        return torch.cat(out)


@pytest.fixture(scope="module")
def world(dev):
    w = World(dev)
    degree = torch.bincount(w.data.edge_index[0], minlength=N)
    assert int(degree[HUB]) == 300 > w.plan.info()["seg_len"] and w.plan.has_hub_rows and int(degree[EMPTY]) == 0
    assert HUB_COLS[0] >= 3 and HUB_COLS[-1] < 296 and len(HUB_COLS) == 300 > 3 * TILE
    # slice 1's edge at the column of base slot TILE - 1 goes between that slot and slot TILE: the first tile's edge
    assert HUB_COLS[TILE - 2] < HUB_COLS[TILE - 1] < HUB_COLS[TILE] < HUB_COLS[TILE + 1]
    cols = w.data.edge_index[1][w.data.edge_index[0] == MERGE_ROW]
    assert sorted(cols.tolist()) == [120, 180]
    # what the cases rely on: row 120 holds a tombstone and no edge of the overlay; rows 210 / 211 are slice 1's alone; the
    # edge-less row is slice 2's alone (and owner -2's, which is nobody's); rows 220 / 221 are nobody's
    unwritten = {(s, row) for s, row in w.unwritten.nonzero().tolist()}
    assert all((s, 120) not in unwritten and (s, MERGE_ROW) not in unwritten and (s, HUB) not in unwritten for s in range(OUTER))
    assert {(0, 210), (2, 210), (0, 211), (2, 211)} <= unwritten and (1, 210) not in unwritten
    assert {(0, EMPTY), (1, EMPTY)} <= unwritten and (2, EMPTY) not in unwritten
    assert all((s, row) in unwritten for s in range(OUTER) for row in (220, 221, 2, 160, 298, 12))
    owners = w.overlay.owner[:w.overlay.num_edges].tolist()
    assert set(owners) == {-2, -1, 0, 1, 2, 3}
    k = w.touched.index(MERGE_ROW)
    lo, hi = int(w.overlay.ptr[k]), int(w.overlay.ptr[k + 1])
    assert list(zip(w.overlay.col[lo:hi].tolist(), w.overlay.owner[lo:hi].tolist())) == [
        (150, -1), (150, 0), (150, 0), (150, 1), (160, 3), (180, 1)]
    return w


def operands(dev, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(OUTER, N, d, generator=g, dtype=dtype).to(dev)
    rel = torch.randn(OUTER, 2 * R_DIRECT, d, generator=g, dtype=dtype).to(dev)
    bnd = torch.randn(OUTER, N, d, generator=g, dtype=dtype).to(dev)
    vals = torch.randn(OUTER, d, generator=g, dtype=dtype).to(dev)
    x[0, 50, :4] = -0.0                      # (signed zeros and a NaN source: compared as bits)
    x[1, 150, 1] = float("nan")
    return x, rel, bnd, vals


def boundaries(dev, bnd, vals):
    on = torch.tensor([HUB, MERGE_ROW, EMPTY], device=dev)         # on a touched row in every slice
    off = torch.tensor([5, 6, 8], device=dev)
    return (("none", {}), ("dense", {"boundary": bnd}), ("point_on", {"point": (on, vals)}), ("point_off", {"point": (off, vals)}))


def run_owned(w, rel, x, sum, mul, kwargs, hub_len=None):
    """forward on the base plan, the unwritten pairs poisoned, the owned entry: (out, base)."""
    out = w.plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
    assert out is not None
    base = out.clone()
    out[w.unwritten] = POISON[x.dtype].to(out.device)
    assert w.plan.edit_rows_owned(rel, x, out, w.overlay, sum=sum, mul=mul, hub_len=hub_len, **kwargs) is out
    return out, base


def check(w, out, base, want, what):
    poison = bits(POISON[out.dtype]).item()
    held = bits(out[w.unwritten])
    assert held.numel() > 0 and bool((held == poison).all()), ("a quiet (row, slice) was written", what)
    got = torch.where(w.unwritten.unsqueeze(-1), base, out)
    same = (bits(got) == bits(want)).all(-1)
    assert bool(same.all()), (what, (~same).nonzero()[:8].tolist())
    touched = torch.zeros(N, dtype=torch.bool, device=out.device)
    touched[torch.tensor(w.touched, device=out.device)] = True
    assert torch.equal(bits(out[:, ~touched]), bits(base[:, ~touched])), ("an untouched row was written", what)


@pytest.mark.parametrize("d,dtype", [(32, torch.float32), (64, torch.float32), (80, torch.float32),
                                     (32, torch.float64), (64, torch.float64), (80, torch.float64)])
@pytest.mark.parametrize("sum,mul", [("add", "mul"), ("add", "add"), ("max", "mul"), ("max", "add"), ("min", "mul"), ("min", "add")])
def test_every_slice_equals_a_fresh_plan_of_its_own_graph(dev, world, sum, mul, d, dtype):
    x, rel, bnd, vals = operands(dev, d, dtype, seed=3)
    if sum != "add":                          # (min / max propagate a NaN by their own rule: keep the row's stream finite)
        x = torch.nan_to_num(x, nan=0.5)
    for kind, kwargs in boundaries(dev, bnd, vals):
        want = world.want(rel, x, sum, mul, **kwargs)
        for hub_len in (None, 0):
            out, base = run_owned(world, rel, x, sum, mul, kwargs, hub_len)
            check(world, out, base, want, (kind, hub_len))
        if sum == "add":        # (a maximum or minimum may stay what it was)
            # the slices really differ on the rows they own, and the hub changed in slices 0 and 1
            assert not torch.equal(bits(out[0, MERGE_ROW]), bits(out[1, MERGE_ROW])), kind
            assert not torch.equal(bits(out[0, HUB]), bits(base[0, HUB])) and not torch.equal(bits(out[1, HUB]), bits(base[1, HUB])), kind


def test_all_owners_shared_gives_the_bits_of_the_split_entry(dev, world):
    shared = World(dev, owned=[None] * QUERIES)
    assert set(shared.overlay.owner[:shared.overlay.num_edges].tolist()) == {-1} and not bool(shared.unwritten.any())
    for dtype, (sum, mul) in ((torch.float32, ("add", "mul")), (torch.float64, ("max", "add")), (torch.float32, ("min", "mul"))):
        x, rel, bnd, vals = operands(dev, 64, dtype, seed=4)
        for kind, kwargs in boundaries(dev, bnd, vals):
            out = shared.plan.forward(rel, x, sum=sum, mul=mul, **kwargs)
            ref = out.clone()
            assert shared.plan.edit_rows_owned(rel, x, out, shared.overlay, sum=sum, mul=mul, **kwargs) is out
            assert shared.plan.edit_rows_split(rel, x, ref, shared.delta, sum=sum, mul=mul, **kwargs) is ref
            assert torch.equal(bits(out), bits(ref)), (kind, sum, mul)


def test_no_tombstones_and_an_empty_overlay(dev):
    w = World(dev, shared=[], dead=None, owned=[[(210, 0, 211)], None, [(HUB, 1, 1)], None, None])
    assert w.delta.num_removed == 0 and len(w.delta) == 0
    x, rel, bnd, vals = operands(dev, 64, torch.float32, seed=5)
    out, base = run_owned(w, rel, x, "add", "mul", {"boundary": bnd})
    check(w, out, base, w.want(rel, x, "add", "mul", boundary=bnd), "no tombstones")
    # the hub is slice 2's alone: slices 0 and 1 were not walked
    assert bool(w.unwritten[0, HUB]) and bool(w.unwritten[1, HUB]) and not bool(w.unwritten[2, HUB])
    w.fill([None] * QUERIES)
    assert int(w.overlay.count) == 0
    out = w.plan.forward(rel, x, boundary=bnd)
    base = out.clone()
    assert w.plan.edit_rows_owned(rel, x, out, w.overlay, boundary=bnd) is out
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(base))


def test_unsupported_calls_launch_nothing(dev, world):
    x, rel, bnd, _ = operands(dev, 64, torch.float32, seed=6)
    out = world.plan.forward(rel, x, boundary=bnd)
    base = out.clone()
    loose = rspmm.Plan(world.data.edge_index, world.data.edge_type, N, 2 * R_DIRECT, exact_order=False)
    assert loose.edit_rows_owned(rel, x, out, world.overlay, boundary=bnd) is None
    assert world.plan.edit_rows_owned(rel, x, out, world.overlay, boundary=bnd, mul="rotate") is None
    odd = torch.zeros(OUTER, N, 68, device=dev)[:, :, 1:65]
    assert world.plan.edit_rows_owned(rel, odd, out, world.overlay, boundary=bnd) is None
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(base))


def test_a_recorded_launch_serves_other_owners_and_edges(dev):
    w = World(dev)
    x, rel, bnd, _ = operands(dev, 64, torch.float32, seed=7)
    out = torch.empty(OUTER, N, 64, device=dev)

    def step():
        w.plan.forward(rel, x, boundary=bnd, out=out)
        assert w.plan.edit_rows_owned(rel, x, out, w.overlay, boundary=bnd) is out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    addresses = (w.overlay.col.data_ptr(), w.overlay.owner.data_ptr(), w.overlay.rows.data_ptr(), w.overlay.count.data_ptr())
    for owned in (OWNED, OTHER, OWNED):
        w.fill(owned)
        out.zero_()
        graph.replay()
        assert torch.equal(bits(out), bits(w.want(rel, x, "add", "mul", boundary=bnd))), owned is OTHER
    # ... and a shared fact stated meanwhile, a retraction included
    w.delta.add(EMPTY, 4, 40)
    w.delta.remove(MERGE_ROW, 1, 180)
    w.fill(OTHER)
    graph.replay()
    assert torch.equal(bits(out), bits(w.want(rel, x, "add", "mul", boundary=bnd)))
    assert addresses == (w.overlay.col.data_ptr(), w.overlay.owner.data_ptr(), w.overlay.rows.data_ptr(), w.overlay.count.data_ptr())
