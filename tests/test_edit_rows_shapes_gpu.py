"""The edit-row kernels (csrc/delta_kernels.hip: ultra_rspmm_delta_rows, ultra_rspmm_edit_rows, ultra_rspmm_edit_rows_samples) at the
shapes they accept and the neighbouring files do not run: rows of one lane, of a partial trip, of a second trip of one lane, of
several trips with a partial last one (a trip is sixteen 16-byte chunks: 64 fp32 or 32 fp64 elements, and every trip restarts the
whole merge), strided layouts, and dead edges placed next to the 16-pair reload of the base cursor and the batches of eight of the
gather (the graph, the cases and the key tables of tests/test_edit_rows_shapes_cpu.py).

The expected value never comes from the device: it is the CPU oracle (oracle/rspmm_oracle.py, the reference's sequential loop) on
the materialised edge list, one outer slice at a time, with the boundary combined afterwards as tests/test_order_gpu.py combines
it.  `out` starts as a sentinel fill: the touched rows must equal the oracle under torch.equal, every other element -- the padding
of a padded `out` included -- must keep the sentinel's bits."""
from types import SimpleNamespace

import pytest
import torch

from oracle import rspmm_oracle
from tests import test_edit_rows_shapes_cpu as shapes
from tests.test_verify_live_gpu import dead_mask
from ultra_amd import layers, rspmm

pytestmark = pytest.mark.gpu

N, R = shapes.N, shapes.R
SENTINEL = -7.0
B_MAX = 5
# the point boundary's rows: ON the row that `r1_emptied` leaves without an edge in slice 0, off it in the others
POINT_ROWS = [shapes.ROW_1, 5, shapes.ROW_33, shapes.ROW_17, shapes.ROW_0]
BOUNDARIES = ("none", "dense", "point")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """The base graph on the GPU with its reference-order plan; per case its delta, the materialised list on the host and the
    touched rows (ascending, as the delta holds them) -- built once, left unchanged."""
    data = shapes.base_graph().to(dev)
    plan = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=True)
    cases = {}
    for name, case in shapes.CASES.items():
        delta = shapes.apply_case(data, case)
        mat = delta.materialize()
        touched = delta.rows[:int(delta.count)].long().cpu()
        cases[name] = SimpleNamespace(name=name, delta=delta, index=mat.edge_index.cpu(), kind=mat.edge_type.cpu(), touched=touched)
    assert len(cases["nothing"].touched) == 0 and len(cases["everything"].touched) > 16
    return SimpleNamespace(data=data, plan=plan, cases=cases)


_VALUES = {}


def values(d, dtype):
    """The operands' values on the host, B_MAX slices, one set per (width, dtype): finite, fixed seed."""
    if (d, dtype) not in _VALUES:
        g = torch.Generator().manual_seed(1000 * d + int(dtype == torch.float64))
        x, rel, bnd = (torch.randn(B_MAX, n, d, generator=g, dtype=dtype) for n in (N, R, N))
        _VALUES[d, dtype] = SimpleNamespace(x=x, rel=rel, bnd=bnd, vals=torch.randn(B_MAX, d, generator=g, dtype=dtype))
    return _VALUES[d, dtype]


_WANT = {}


def oracle_rows(case, table, s, rel_slice, d, dtype, sum, mul):
    """The touched rows of slice s on the case's materialised list -- without the edges that slice s's keys of `table` name --
    by the CPU oracle, before the boundary.  Cached: every boundary, kernel and layout of one (case, slice, width, dtype, sum,
    mul) shares it."""
    key = (case.name, table, s, rel_slice, d, dtype, sum, mul)
    if key not in _WANT:
        index, kind = case.index, case.kind
        if table is not None:
            dead = dead_mask(index, kind, shapes.KEY_TABLES[table][s])
            index, kind = index[:, ~dead], kind[~dead]
        v = values(d, dtype)
        full = rspmm_oracle.generalized_rspmm(index, kind, torch.ones(index.shape[1], dtype=dtype), v.rel[rel_slice], v.x[s],
                                              sum=sum, mul=mul)
        _WANT[key] = full[case.touched].clone()
    return _WANT[key]


def expected(case, table, s, rel_slice, d, dtype, sum, mul, boundary):
    want = oracle_rows(case, table, s, rel_slice, d, dtype, sum, mul)
    if boundary == "none":
        return want
    v = values(d, dtype)
    if boundary == "dense":
        bnd = v.bnd[s][case.touched]
    else:       # a point boundary is its dense equivalent: zeros, with vals[s] at rows[s]
        bnd = torch.zeros(len(case.touched), d, dtype=dtype)
        bnd[case.touched == POINT_ROWS[s]] = v.vals[s]
    return want + bnd if sum == "add" else (torch.max(want, bnd) if sum == "max" else torch.min(want, bnd))


LAYOUTS = {
    # name -> (the buffer's shape for a logical (B, n, d) operand, the logical view of the buffer)
    "contiguous": (lambda B, n, d, pad: (B, n, d), lambda buf, d: buf),
    "node_major": (lambda B, n, d, pad: (n, B, d), lambda buf, d: buf.transpose(0, 1)),
    "padded": (lambda B, n, d, pad: (B, n, d + pad), lambda buf, d: buf[:, :, :d]),
    "two_dim": (lambda B, n, d, pad: (n, d), lambda buf, d: buf),
}


def device_operands(dev, d, dtype, B, layout="contiguous", shared_relation=False):
    """The values of `values(d, dtype)` on the device in the given layout (two_dim: slice 0 alone, as (rows, d) matrices)."""
    v = values(d, dtype)
    shape_of, view = LAYOUTS[layout]
    pad = 16 // v.x.element_size()

    def load(t):
        buf = torch.zeros(shape_of(B, t.shape[1], d, pad), dtype=dtype, device=dev)
        view(buf, d).copy_(t[0] if layout == "two_dim" else t[:B])
        return view(buf, d)

    rel = v.rel[:1].to(dev).expand(B, -1, -1) if shared_relation else load(v.rel)
    return SimpleNamespace(d=d, dtype=dtype, B=B, layout=layout, shared=shared_relation, rel=rel, x=load(v.x), bnd=load(v.bnd),
                           vals=v.vals[:B].to(dev), rows=torch.tensor(POINT_ROWS[:B], device=dev),
                           out_shape=shape_of(B, N, d, pad), view=view)


def key_tensors(table, B, dev):
    packed = torch.tensor(shapes.KEY_TABLES[table][:B], dtype=torch.int32, device=dev)           # (B, per_sample, 3)
    return tuple(packed[:, :, i].contiguous() for i in range(3))


def run(plan, kernel, delta, t, keys, boundary, sum, mul):
    """One call on a sentinel-filled `out` in t's layout: (what the call returned, the logical `out`, the whole buffer)."""
    buf = torch.full(t.out_shape, SENTINEL, dtype=t.dtype, device=t.x.device)
    out = t.view(buf, t.d)
    kw = {"none": {}, "dense": dict(boundary=t.bnd), "point": dict(point=(t.rows, t.vals))}[boundary]
    if kernel == "delta_rows":
        got = plan.delta_rows(t.rel, t.x, out, delta, sum=sum, mul=mul, **kw)
    elif kernel == "edit_rows":
        got = plan.edit_rows(t.rel, t.x, out, delta, sum=sum, mul=mul, **kw)
    else:
        got = plan.edit_rows_samples(t.rel, t.x, out, delta, keys, sum=sum, mul=mul, **kw)
    return got, out, buf


def assert_sentinel(buf, keep, what):
    """Every element of the buffer on the host where `keep` holds still has the sentinel's bits."""
    bits = torch.int64 if buf.dtype == torch.float64 else torch.int32
    fill = torch.full((1,), SENTINEL, dtype=buf.dtype).view(bits)
    assert bool((buf.contiguous().view(bits)[keep.contiguous()] == fill).all()), what


def check(world, name, kernel, t, boundary, sum, mul, keys=None, table=None, delta=None, live=None):
    """Run `kernel` on the case and compare: it returned `out`; the touched rows (the first `live` of them where the count was
    lowered) equal the oracle in every slice; nothing else of the buffer was written."""
    case = world.cases[name]
    what = (name, kernel, table, boundary, sum, mul, t.d, t.layout, live)
    got, out, buf = run(world.plan, kernel, case.delta if delta is None else delta, t, keys, boundary, sum, mul)
    assert got is out, what
    host = buf.cpu()
    logical = t.view(host, t.d)
    written = case.touched if live is None else case.touched[:max(live, 0)]
    keep = torch.ones(host.shape, dtype=torch.bool)
    if t.layout == "two_dim":
        logical = logical[None]
        t.view(keep, t.d)[written] = False
    else:
        t.view(keep, t.d)[:, written] = False
    for s in range(1 if t.layout == "two_dim" else t.B):
        want = expected(case, table, s, 0 if t.shared else s, t.d, t.dtype, sum, mul, boundary)[:len(written)]
        have = logical[s][written]
        assert torch.equal(have, want), what + (s, case.touched[(have != want).any(-1).nonzero().flatten()[:8]].tolist())
    assert_sentinel(host, keep, what)


def check_all_kernels(world, dev, name, t, boundary, sum, mul, tables):
    if name in shapes.ADD_ONLY:
        check(world, name, "delta_rows", t, boundary, sum, mul)
    check(world, name, "edit_rows", t, boundary, sum, mul)
    for table, keys in tables.items():
        check(world, name, "edit_rows_samples", t, boundary, sum, mul, keys=keys, table=table)


WIDTHS = [(torch.float32, d) for d in (4, 60, 64, 68, 128, 200)] + [(torch.float64, d) for d in (2, 30, 32, 34, 64, 72)]


@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "max", "min"])
@pytest.mark.parametrize("dtype,d", WIDTHS, ids=["%s-%d" % (str(dtype)[6:], d) for dtype, d in WIDTHS])
def test_widths(dev, world, dtype, d, sum, mul):
    """One lane, a partial single trip, a full trip, a second trip of one lane, two full trips, several trips with a partial last
    one: every case, every boundary, all three kernels, both key tables."""
    t = device_operands(dev, d, dtype, B=3)
    tables = {table: key_tensors(table, 3, dev) for table in shapes.KEY_TABLES}
    for name in shapes.CASES:
        for boundary in BOUNDARIES:
            check_all_kernels(world, dev, name, t, boundary, sum, mul, tables)


@pytest.mark.parametrize("sum", ["add", "max"])
@pytest.mark.parametrize("dtype,d", [(torch.float32, 68), (torch.float64, 34)], ids=["float32-68", "float64-34"])
@pytest.mark.parametrize("layout", ["contiguous", "node_major", "shared_relation", "two_dim", "five_slices", "padded"])
def test_layouts(dev, world, layout, dtype, d, sum):
    """as_mat passes any strides through: node-major views, a relation shared by the slices (stride_outer == 0), 2-D operands
    (n_outer == 1), five slices (a workgroup's sixteen groups then straddle touched rows), rows with padding between them."""
    B = {"five_slices": 5, "two_dim": 1}.get(layout, 3)
    named = layout if layout in LAYOUTS else "contiguous"
    t = device_operands(dev, d, dtype, B, layout=named, shared_relation=layout == "shared_relation")
    if layout == "node_major":
        assert t.x.stride(0) == d and t.x.stride(1) == 3 * d and t.rel.stride(0) == d
    if layout == "shared_relation":
        assert t.rel.stride(0) == 0
    if layout == "two_dim":
        assert t.x.dim() == 2 and t.rel.dim() == 2
    if layout == "padded":
        assert t.x.stride(1) > d and t.rel.stride(1) > d and t.bnd.stride(1) > d
    tables = {table: key_tensors(table, B, dev) for table in shapes.KEY_TABLES}
    for boundary in BOUNDARIES:
        check(world, "everything", "edit_rows", t, boundary, sum, "mul")
        for table, keys in tables.items():
            check(world, "everything", "edit_rows_samples", t, boundary, sum, "mul", keys=keys, table=table)


@pytest.mark.parametrize("dtype,d", [(torch.float32, 68), (torch.float64, 34)], ids=["float32-68", "float64-34"])
def test_live_count(dev, world, dtype, d):
    """The grid is sized by the capacity and the live number of touched rows is read on the device: with the count lowered in
    place only the first k touched rows are written, with a negative count none."""
    t = device_operands(dev, d, dtype, B=3)
    keys = key_tensors("keys_8", 3, dev)
    for name, kernels in (("everything", ("edit_rows", "edit_rows_samples")), ("r0_delta_only", ("delta_rows",))):
        delta = shapes.apply_case(world.data, shapes.CASES[name])           # a delta of the test's own
        count = int(delta.count)
        assert delta.rows[:count].tolist() == world.cases[name].touched.tolist()
        for live in (count - 2, 1, 0, -3):
            assert live < count
            delta.count.fill_(live)
            for kernel in kernels:
                sampled = kernel == "edit_rows_samples"
                check(world, name, kernel, t, "dense", "add", "mul", keys=keys if sampled else None,
                      table="keys_8" if sampled else None, delta=delta, live=live)


@pytest.mark.parametrize("dtype,d", [(torch.float32, 66), (torch.float64, 33)], ids=["float32-66", "float64-33"])
def test_rows_that_are_no_whole_chunks_are_refused(dev, world, dtype, d):
    t = device_operands(dev, d, dtype, B=3)
    keys = key_tensors("keys_8", 3, dev)
    for name, kernel in (("r0_delta_only", "delta_rows"), ("everything", "edit_rows"), ("everything", "edit_rows_samples")):
        for boundary in BOUNDARIES:
            got, _, buf = run(world.plan, kernel, world.cases[name].delta, t, keys, boundary, "add", "mul")
            assert got is None, (kernel, boundary)
            host = buf.cpu()
            assert_sentinel(host, torch.ones(host.shape, dtype=torch.bool), (kernel, boundary))


@pytest.mark.parametrize("aggr", ["sum", "max"])
def test_a_layer_of_width_128_equals_the_layer_on_the_materialised_graph(dev, world, aggr):
    data, case = world.data, world.cases["everything"]
    torch.manual_seed(2)
    layer = layers.GeneralizedRelationalConv(128, 128, R, 128, message_func="distmult", aggregate_func=aggr,
                                             layer_norm=True).to(dev).eval()
    v = values(128, torch.float32)
    x, bnd, vals = v.x[:3].to(dev), v.bnd[:3].to(dev), v.vals[:3].to(dev)
    rows = torch.tensor(POINT_ROWS[:3], device=dev)
    index, kind = case.index.to(dev), case.kind.to(dev)
    size = (N, N)
    with torch.no_grad():
        for boundary in (bnd, layers.PointBoundary(rows, vals, N)):
            got = layer._forward_impl(x, vals, boundary, data.edge_index, data.edge_type, size, delta=case.delta)
            assert got is not None, type(boundary).__name__                 # served by _propagate_delta, not materialised
            want = layer(x, vals, boundary, index, kind, size)
            assert torch.equal(got, want), type(boundary).__name__
            assert torch.equal(layer(x, vals, boundary, data.edge_index, data.edge_type, size, delta=case.delta), want)
            assert not torch.equal(got, layer(x, vals, boundary, data.edge_index, data.edge_type, size))
