"""The min / max rspmm backward (rspmm_minmax_bwd_gather_kernel + rspmm_fixup_kernel, the atomic rspmm_edge_bwd_kernel for
unaligned / odd-length rows) against an fp64 restatement of the reference's tie rule: EVERY edge whose message equals the
forward output gets the full output gradient (rspmm.cu:153-214, operator.cuh:62-64, 75-77).

The restatement computes each message in the kernel's dtype, one rounding per operation like operator.cuh, takes the tie
mask against the forward output (itself checked against the C oracle first) and sums the gradient terms in fp64, with
sum |term| and the number of terms per element: an fp32 result may differ from the exact sum by the rounding of its own
n terms, c * n * 2^-24 * sum |term|, which one missing or doubled edge term exceeds.  The graphs and features are built
so that ties are common, as they are after a ReLU.

The case builders take a `width`: the first 64 columns are the tensors they have always drawn (pinned by fingerprint in
test_backward_bounds_cpu.py), the columns past 64 come from a second generator, so the kernels' span loops (ceil(d / 64)
spans a slice) are walked at partial, two and three spans with the same cases."""
import resource
import time

import pytest
import torch

from oracle import rspmm_oracle
from tests.helpers import C_ROUND, assert_within       # noqa: F401  (the bound of this file, shared with tests/add_backward.py)
from ultra_amd import rspmm, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the restatement ----

def message(rel, x, typ, col, mul):
    """rel[:, type] (x) x[:, col] in the operands' dtype: (bs, E, d)."""
    return rel[:, typ] * x[:, col] if mul == "mul" else rel[:, typ] + x[:, col]


def restate_backward(row, col, typ, w, rel, x, out, og, mul, chunk=1 << 18):
    """Gradients of out[b, row] = min/max over the edges of w * (rel[b, type] (x) x[b, col]) for the given (filtered) edge list,
    operands batch-major (bs, ., d) in the kernel's dtype.  Returns fp64 (want, mass, count) for input and relation, and the
    per-edge weight gradient with its mass; count[i] is the number of tying terms that reach element i."""
    bs, num_in, d = x.shape
    num_rel = rel.shape[1]
    f64 = torch.float64
    acc = {k: torch.zeros(bs, n, d, dtype=f64) for k, n in (("x", num_in), ("rel", num_rel))}
    mass = {k: torch.zeros_like(v) for k, v in acc.items()}
    count = {k: torch.zeros_like(v) for k, v in acc.items()}
    wgrad = torch.zeros(row.numel(), dtype=f64)
    wmass = torch.zeros(row.numel(), dtype=f64)
    for s in range(0, row.numel(), chunk):
        r, c, t = row[s:s + chunk], col[s:s + chunk], typ[s:s + chunk]
        xb = message(rel, x, t, c, mul)
        ww = None if w is None else w[s:s + chunk].view(1, -1, 1)
        y = xb if ww is None else ww * xb
        tie = out[:, r] == y                                  # +0.0 == -0.0: both tie
        del y
        t_og = og[:, r].to(f64) * tie
        tw = t_og if ww is None else t_og * ww.to(f64)
        if mul == "mul":
            terms = {"x": tw * rel[:, t].to(f64), "rel": tw * x[:, c].to(f64)}
        else:
            terms = {"x": tw, "rel": tw}
        del tw
        tie64 = tie.to(f64)
        for k, idx in (("x", c), ("rel", t)):
            acc[k].index_add_(1, idx, terms[k])
            mass[k].index_add_(1, idx, terms[k].abs())
            count[k].index_add_(1, idx, tie64)
        del terms, tie64
        wt = t_og * xb.to(f64)
        wgrad[s:s + chunk] = wt.sum(dim=(0, 2))
        wmass[s:s + chunk] = wt.abs().sum(dim=(0, 2))
        del wt, t_og, xb, tie
    return acc, mass, count, wgrad, wmass


def oracle_forward(row, col, typ, w, rel, x, sum, mul):
    """rspmm_oracle.rspmm_forward on the (sorted) edge list, batch folded into the feature axis as the reference's layer does
    (layers.py:189-230)."""
    bs, n, d = x.shape
    ei, et, ew, _ = rspmm_oracle.sort_edges(torch.stack([row, col]), typ, torch.ones(row.numel(), dtype=x.dtype) if w is None else w)
    out = rspmm_oracle.rspmm_forward(ei, et, ew, rel.transpose(0, 1).reshape(rel.shape[1], bs * d),
                                     x.transpose(0, 1).reshape(n, bs * d), sum=sum, mul=mul)
    return out.view(n, bs, d).transpose(0, 1)


# ---- graphs and features: each case targets one edge of the tie rule ----

def _edges(g, num_node, num_edge, num_rel, rows=None):
    row = torch.randint(0, num_node, (num_edge,), generator=g) if rows is None else rows
    return row, torch.randint(0, num_node, (num_edge,), generator=g), torch.randint(0, num_rel, (num_edge,), generator=g)


def _relu_like(g, shape, zero_share=0.4):
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    v[torch.rand(shape, generator=g) < zero_share] = 0.0
    return v


def _columns(g, rows, width, draw):
    """(rows, max(width, 64)) features: the first 64 columns are draw(g, (rows, 64)), whatever the width -- the tensors and
    the generator state every width-64 case has always had -- and the columns past 64 come from a generator of their own."""
    v = draw(g, (rows, 64))
    if width > 64:
        v = torch.cat([v, draw(torch.Generator().manual_seed(1000 * width + rows), (rows, width - 64))], dim=1)
    return v


def _randn(g, shape):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _rand01(g, shape):
    return torch.rand(shape, generator=g, dtype=torch.float64) + 0.1


def case_relu_zeros(g, width=64):
    """~40 % exact zeros and whole zero rows of x: rows whose maximum is an exact 0 reached by many edges (every zero-row
    neighbour's message is +-0); the min aggregate sees the same from below."""
    n, r = 300, 6
    row, col, typ = _edges(g, n, 4000, r)
    x = _columns(g, n, width, _relu_like).abs()
    x[torch.randperm(n, generator=g)[:60]] = 0.0
    rel = _columns(g, r, width, _randn)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel)


def case_all_negative(g, width=64):
    """Rows whose messages are all negative (mul: positive x, negative relations; add: both negative): the maximum is the
    least negative message, not a 0 that an absent edge would bring in."""
    n, r = 200, 4
    row, col, typ = _edges(g, n, 2500, r)
    x = _columns(g, n, width, _rand01)
    rel = -_columns(g, r, width, _rand01)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel, x_add=-x)


def case_signed_zeros(g, width=64):
    """+0.0 and -0.0 messages in one row (x rows of +0.0 and of -0.0 times positive relations) next to negative messages (the
    other x rows are negative): under max the two zeros compare equal, so both edges tie, whichever of them the forward kept."""
    n, r = 160, 4
    row, col, typ = _edges(g, n, 2000, r)
    x = -_columns(g, n, width, _rand01)
    x[0::6] = 0.0
    x[3::6] = -0.0
    rel = _columns(g, r, width, _rand01)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel)


def case_copies(g, width=64):
    """Distinct edges with identical messages: copied x rows (cols 2k and 2k+1 hold the same features) and copied relation
    rows (types 0 / 1 and 2 / 3), plus exact duplicate (row, col, type) edges."""
    n, r = 200, 4
    row, col, typ = _edges(g, n, 2500, r)
    dup = torch.randint(0, row.numel(), (400,), generator=g)
    row, col, typ = torch.cat([row, row[dup]]), torch.cat([col, col[dup]]), torch.cat([typ, typ[dup]])
    x = _columns(g, n, width, lambda gen, shape: _relu_like(gen, shape, 0.1))
    x[1::2] = x[0::2]
    rel = _columns(g, r, width, _randn)
    rel[1], rel[3] = rel[0], rel[2]
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel)


def case_empty(g, width=64):
    """Empty rows (no in-edges), nodes that are no edge's source and unused relation types: their gradients must be written
    as 0, not left as whatever the allocator held."""
    n, r = 150, 7
    row, col, typ = _edges(g, n, 900, r)
    row = row % 100            # rows 100.. receive nothing
    col = col % 120 + 30       # nodes 0..29 send nothing
    typ = typ % 5              # types 5, 6 unused
    x = _columns(g, n, width, _relu_like)
    rel = _columns(g, r, width, _randn)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel)


def case_hub(g, width=64):
    """A hub row (4000 in-edges) and a hub source node (3000 out-edges) far past the segment length: with
    Plan(seg_len=16, g_max=4) both the transposed plan (input gradient) and the relation-major plan (few types over many
    edges) cut rows into items with partial slots, and rspmm_fixup_kernel folds them."""
    n, r = 400, 3
    row, col, typ = _edges(g, n, 3000, r)
    hub_row = torch.full((4000,), 7, dtype=torch.long)
    hub_col = torch.full((3000,), 11, dtype=torch.long)
    row = torch.cat([row, hub_row, torch.randint(0, n, (3000,), generator=g)])
    col = torch.cat([col, torch.randint(0, n, (4000,), generator=g), hub_col])
    typ = torch.cat([typ, torch.randint(0, r, (7000,), generator=g)])
    x = _columns(g, n, width, _relu_like)
    rel = _columns(g, r, width, _randn)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel, split=True)


def case_tiny(g, width=64):
    """A dozen nodes: small enough that a batch of over a thousand samples keeps the restatement's (batch, E, d) fp64
    temporaries in the tens of MB.  Node 11 receives nothing, node 0 sends nothing."""
    n, r = 12, 3
    row, col, typ = _edges(g, n, 60, r)
    row = row % 11
    col = col % 11 + 1
    x = _columns(g, n, width, _relu_like)
    rel = _columns(g, r, width, _randn)
    return dict(n=n, r=r, edges=(row, col, typ), x=x, rel=rel)


CASES = {"relu_zeros": case_relu_zeros, "all_negative": case_all_negative, "signed_zeros": case_signed_zeros,
         "copies": case_copies, "empty": case_empty, "hub": case_hub}
LAYOUTS = ("2d", "batch", "shared")
WEIGHTS = ("none", "random", "keep")


def operands(spec, layout, mul, dtype, g, bs=3, d=64):
    """(rel leaf, rel as the kernel sees it, x leaf, x as the kernel sees it) for one layout; the leaves are what autograd
    differentiates (shared: the (R, d) table whose gradient is the batch sum of the expanded view's)."""
    x = spec["x_add"] if (mul == "add" and "x_add" in spec) else spec["x"]
    rel = spec["rel"]
    assert x.shape[1] >= d and rel.shape[1] >= d, "build the case with width >= d"
    x, rel = x[:, :d], rel[:, :d]
    if layout == "2d":
        xs, rels = x.unsqueeze(0), rel.unsqueeze(0)
    else:
        # the other samples: the same structure, features permuted over nodes / scaled (zeros stay zeros)
        xs = torch.stack([x] + [x[torch.randperm(x.shape[0], generator=g)] * (1 + 0.5 * k) for k in range(1, bs)])
        if layout == "batch":
            rels = torch.stack([rel] + [rel * (1 - 0.25 * k) for k in range(1, bs)])
        else:
            rels = rel.unsqueeze(0)
    xs, rels = xs.to(dtype), rels.to(dtype)
    return rels, xs


def to_dev(t, dev, unaligned=False):
    if not unaligned:
        return t.to(dev)
    big = torch.zeros(t.shape[:-1] + (t.shape[-1] + 1,), dtype=t.dtype, device=dev)
    big[..., 1:] = t.to(dev)
    return big[..., 1:]          # rows 4 bytes off 16-byte alignment: the atomic edge kernel


def run_case(dev, spec, sum, mul, dtype, layout, weights, plan_kw=None, d=64, unaligned=False, seed=0, bs=3):
    g = torch.Generator().manual_seed(seed)
    row, col, typ = spec["edges"]
    n, r = spec["n"], spec["r"]
    rels, xs = operands(spec, layout, mul, dtype, g, bs=bs, d=d)
    bs = xs.shape[0]
    E = row.numel()
    w = None
    if weights == "random":
        w = (torch.rand(E, generator=g, dtype=torch.float64) + 0.5).to(dtype)
    elif weights == "keep":
        w = (torch.rand(E, generator=g) > 0.3).to(dtype)
    og = torch.randn(bs, n, d, generator=g, dtype=torch.float64).to(dtype)

    plan = rspmm.Plan(torch.stack([row, col]).to(dev), typ.to(dev), n, r, **(plan_kw or {}))
    # ---- the GPU: forward + autograd backward through plan_rspmm, as the model calls it ----
    x_leaf = to_dev(xs[0] if layout == "2d" else xs, dev, unaligned).detach().requires_grad_()
    if layout == "shared":
        rel_leaf = rels[0].to(dev).requires_grad_()
        rel_in = rel_leaf.unsqueeze(0).expand(bs, -1, -1)
        assert rel_in.stride(0) == 0
    else:
        rel_leaf = (rels[0] if layout == "2d" else rels).to(dev).requires_grad_()
        rel_in = rel_leaf
    keep = weights == "keep"
    w_dev = None
    if w is not None:
        w_dev = w.to(dev)
        if not keep:
            w_dev.requires_grad_()
    out = rspmm.plan_rspmm(plan, rel_in, x_leaf, edge_weight=w_dev, sum=sum, mul=mul, keep=keep)
    out.backward(og[0].to(dev) if layout == "2d" else og.to(dev))

    # ---- the reference: the filtered edge list (keep: dropped edges are absent, not messages of value 0) ----
    if keep:
        sel = w.bool()
        row_f, col_f, typ_f, w_f = row[sel], col[sel], typ[sel], None
    else:
        row_f, col_f, typ_f, w_f = row, col, typ, w
    rel_b = rels.expand(bs, -1, -1).contiguous()
    want_out = oracle_forward(row_f, col_f, typ_f, w_f, rel_b, xs, sum, mul)
    got_out = out.detach().cpu().view(bs, n, d)
    # (value equality: the two zeros are the same maximum; which sign a re-associating plan keeps is not part of the contract)
    assert torch.equal(got_out, want_out), "forward differs from the C oracle"
    acc, mass, count, wg, wmass = restate_backward(row_f, col_f, typ_f, w_f, rel_b, xs, want_out, og, mul)
    eps = torch.finfo(dtype).eps / 2
    got_x = x_leaf.grad.cpu().view(bs, n, d)
    assert_within(got_x, acc["x"], mass["x"], count["x"], eps, "input grad")
    got_rel = rel_leaf.grad.cpu()
    if layout == "shared":
        want_rel, mass_rel, count_rel = acc["rel"].sum(0), mass["rel"].sum(0), count["rel"].sum(0)
    else:
        want_rel, mass_rel, count_rel = acc["rel"], mass["rel"], count["rel"]
    assert_within(got_rel.view(want_rel.shape), want_rel, mass_rel, count_rel, eps, "relation grad")
    # per-edge weight gradient: a sum over bs * d entries, so a tie credited to the wrong edge shows edge by edge
    if weights == "random":
        assert_within(w_dev.grad.cpu(), wg, wmass, torch.full_like(wg, bs * d), eps, "weight grad")
    elif weights == "none":
        wgrad, rgrad, xgrad = plan.backward(rel_in.detach(), x_leaf.detach(), out.detach(),
                                            (og[0] if layout == "2d" else og).to(dev), need_weight_grad=True, sum=sum, mul=mul)
        assert_within(wgrad.cpu(), wg, wmass, torch.full_like(wg, bs * d), eps, "weight grad (Plan.backward)")
        assert_within(xgrad.cpu().view(bs, n, d), acc["x"], mass["x"], count["x"], eps, "input grad (Plan.backward)")
        if not unaligned and d % 4 == 0:      # the gather kernels: deterministic, the autograd call's bits
            assert torch.equal(xgrad, x_leaf.grad)
    return plan


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["max", "min"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_minmax_backward_matches_tie_restatement(dev, case, sum, mul, dtype):
    spec = CASES[case](torch.Generator().manual_seed(sorted(CASES).index(case)))
    for layout in LAYOUTS:
        for weights in WEIGHTS:
            try:
                run_case(dev, spec, sum, mul, dtype, layout, weights, seed=len(layout) * 7 + len(weights))
            except AssertionError as e:
                raise AssertionError("%s / %s: %s" % (layout, weights, e))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["max", "min"])
@pytest.mark.parametrize("case", ["relu_zeros", "copies", "empty"])
@pytest.mark.parametrize("d", [4, 72, 128, 200])
def test_minmax_backward_at_wide_and_partial_rows(dev, d, case, sum, mul, dtype):
    """Row lengths other than 64 on the gather route (d % 4 == 0): one active lane of a span (4), a partial second span
    (72), two whole spans (128), three whole spans and 8 elements (200).  rspmm_minmax_bwd_gather_kernel and
    rspmm_fixup_kernel walk ceil(d / 64) spans a slice and rspmm_edge_bwd_kernel sums the weight gradient over them; the
    `empty` case's untouched rows must come out 0 in every span.  run_case keeps the bit equality of Plan.backward with
    the autograd call."""
    spec = CASES[case](torch.Generator().manual_seed(sorted(CASES).index(case)), width=d)
    for layout in LAYOUTS:
        for weights in WEIGHTS:
            try:
                run_case(dev, spec, sum, mul, dtype, layout, weights, d=d, seed=len(layout) * 7 + len(weights))
            except AssertionError as e:
                raise AssertionError("%s / %s: %s" % (layout, weights, e))


@pytest.mark.parametrize("layout", ["batch", "shared"])
def test_more_spans_than_the_gather_grid(dev, layout):
    """1100 samples of d = 72: 2200 spans for the 2048 workgroups of backward_gather, so smod == 2048, nparts == 1 and the
    kernels' `span += smod` stride takes a second turn (every other test has at most a dozen spans)."""
    bs, d = 1100, 72
    assert bs * -(-d // 64) > 2048
    spec = case_tiny(torch.Generator().manual_seed(17), width=d)
    for weights in WEIGHTS:
        try:
            run_case(dev, spec, "max", "mul", torch.float32, layout, weights, d=d, bs=bs, seed=23)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (weights, e))


def _assert_derived_plans_split_rows(spec, kw):
    """The plans the backward derives (ensure_backward_plans: same seg_len / g_max, re-associating) have partial slots."""
    row, col, typ = spec["edges"]
    derived = (rspmm.Plan(torch.stack([col, row]), typ, spec["n"], spec["r"], type_runs=False, dense=False, **kw),
               rspmm.Plan(torch.stack([typ, col]), row, spec["r"], spec["n"], num_in=spec["n"], type_runs=False, dense=False, **kw))
    for p in derived:
        info = p.info()
        assert info["n_partial_slot"] > 0 and info["n_split_row"] > 0, info


@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["max", "min"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_split_rows_run_the_fixup_at_a_wide_row(dev, sum, dtype, mul):
    """test_split_rows_run_the_fixup at d = 136: rspmm_fixup_kernel folds the partial slots of three spans a slice, the
    last of them 8 elements long."""
    d = 136
    spec = case_hub(torch.Generator().manual_seed(99), width=d)
    kw = dict(seg_len=16, g_max=4)
    _assert_derived_plans_split_rows(spec, kw)
    for layout in LAYOUTS:
        for weights in WEIGHTS:
            try:
                run_case(dev, spec, sum, mul, dtype, layout, weights, plan_kw=kw, d=d, seed=5)
            except AssertionError as e:
                raise AssertionError("%s / %s: %s" % (layout, weights, e))


@pytest.mark.parametrize("sum", ["max", "min"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_split_rows_run_the_fixup(dev, sum, dtype):
    """Plan(seg_len=16, g_max=4): the hub rows of the transposed and relation-major plans are cut into items whose partial
    sums rspmm_fixup_kernel adds; every layout and weighting against the restatement."""
    spec = case_hub(torch.Generator().manual_seed(99))
    kw = dict(seg_len=16, g_max=4)
    _assert_derived_plans_split_rows(spec, kw)
    for mul in ("mul", "add"):
        for layout in LAYOUTS:
            for weights in WEIGHTS:
                try:
                    run_case(dev, spec, sum, mul, dtype, layout, weights, plan_kw=kw, seed=5)
                except AssertionError as e:
                    raise AssertionError("%s / %s / %s: %s" % (mul, layout, weights, e))


@pytest.mark.parametrize("shape", ["d62", "d130", "unaligned"])
@pytest.mark.parametrize("sum", ["max", "min"])
def test_atomic_fallback_within_tolerance(dev, shape, sum):
    """A row length that is not a multiple of 4, or rows off 16-byte alignment, take the reference's atomic scatter
    (rspmm_edge_bwd_kernel): not bit-deterministic, so compared within the rounding bound only."""
    d = {"d62": 62, "d130": 130, "unaligned": 64}[shape]        # 130: nine 16-element spans of the scalar kernel, the last of 2
    for name in ("relu_zeros", "signed_zeros", "copies", "empty"):
        spec = CASES[name](torch.Generator().manual_seed(31), width=d)
        for mul in ("mul", "add"):
            for dtype in (torch.float32, torch.float64):
                for layout, weights in (("2d", "none"), ("2d", "random"), ("batch", "keep"), ("shared", "random")):
                    if shape != "unaligned" and layout != "2d":
                        continue
                    try:
                        run_case(dev, spec, sum, mul, dtype, layout, weights, d=d, unaligned=shape == "unaligned", seed=3)
                    except AssertionError as e:
                        raise AssertionError("%s / %s / %s / %s / %s: %s" % (name, mul, dtype, layout, weights, e))


def test_yago310_edge_count(dev):
    """One max / fp32 case at YAGO3-10's size (synthetic.SHAPES["yago310"], both directions, batch 1, d = 64) with ReLU-like
    inputs; the restatement runs in chunks of edges.  Prints its wall time and the process's peak host memory."""
    t0 = time.time()
    data = synthetic.make_kg(**synthetic.SHAPES["yago310"], seed=1234)
    g = torch.Generator().manual_seed(0)
    n, r = data.num_nodes, data.num_relations
    row, col = data.edge_index
    spec = dict(n=n, r=r, edges=(row, col, data.edge_type), x=_relu_like(g, (n, 64)).abs(),
                rel=torch.randn(r, 64, generator=g, dtype=torch.float64))
    spec["x"][torch.randperm(n, generator=g)[:n // 8]] = 0.0
    run_case(dev, spec, "max", "mul", torch.float32, "2d", "none")
    print("\nyago310 max/f32 backward: %d edges, %.1f s, peak host RSS %.2f GB"
          % (row.numel(), time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))
