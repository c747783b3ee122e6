"""RotatE messages on the rspmm engine (ULTRA_MUL_ROTATE): operator, gradients, keep vectors, layer and model on the GPU.

Yardsticks:
  * tests/golden/rotate.pt.xz -- the UNCHANGED reference layer run on the CPU (gen_rotate_golden.py).  On its `sorted` edge list
    the reference's scatter_add_ IS the engine's reference order (the generator asserts it), so reference-order plans are
    pinned to the reference bit for bit there; max / min do not depend on the order (but for the sign of a zero, which
    torch.equal ignores).
  * `sequential` below -- the engine's own definition restated in torch on the CPU: every row's messages in sorted
    (target, source, edge id) order, one after the other, the boundary last.  Holds for every graph: torch.equal.
  * re-associating plans and every gradient: the project's data-dependent bound (tests/helpers.assert_sum_close:
    (2 + sqrt(n)) * eps * sum |terms|) with n = 2 * the largest number of edges a destination sums (two products an edge) and
    the mass of the complex product: sum |w| (|b_re| |a_re| + |b_im| |a_im|) for the real half, sum |w| (|b_re| |a_im| +
    |b_im| |a_re|) for the imaginary half (+ |boundary|).
"""
import io
import lzma
import os

import pytest
import torch

from tests import helpers
from ultra_amd import _lib, layers, models, rspmm, synthetic, tasks

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotate.pt.xz")
AGGRS = ("sum", "mean", "max", "min")
SUM_OF = {"sum": "add", "mean": "add", "max": "max", "min": "min"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with lzma.open(GOLDEN, "rb") as f:
        return torch.load(io.BytesIO(f.read()))


# ---- restatements (CPU) ----
def rot(r, x, conj_r=False, conj_x=False):
    """ROT(r, x) on (real | imaginary) halves of the last axis; products and sums as separate torch ops."""
    x_re, x_im = x.chunk(2, dim=-1)
    r_re, r_im = r.chunk(2, dim=-1)
    if conj_r:
        return torch.cat([x_re * r_re + x_im * r_im, x_im * r_re - x_re * r_im], dim=-1)
    if conj_x:
        return torch.cat([r_re * x_re + r_im * x_im, r_im * x_re - r_re * x_im], dim=-1)
    return torch.cat([x_re * r_re - x_im * r_im, x_re * r_im + x_im * r_re], dim=-1)


def rot_mass(a, b):
    a_re, a_im = a.abs().chunk(2, dim=-1)
    b_re, b_im = b.abs().chunk(2, dim=-1)
    return torch.cat([b_re * a_re + b_im * a_im, b_re * a_im + b_im * a_re], dim=-1)


def sorted_order(ei, num_node):
    """Plan order of edge list ei = (target, source): by target, source, edge id."""
    E = ei.shape[1]
    return torch.sort((ei[0] * num_node + ei[1]) * max(E, 1) + torch.arange(E))[1]


def sequential(ei, typ, w, rel, x, num_node, sum="add", boundary=None, point=None, keep=False):
    """The engine's definition: rel (B, R, d), x (B, N, d); ei = (target, source).  Every row's weighted messages in plan order,
    one after the other from the identity, then the boundary (a point boundary: its row only)."""
    if keep and w is not None:       # a dropped edge is absent
        sel = w != 0
        ei, typ, w = ei[:, sel], typ[sel], None
    order = sorted_order(ei, max(num_node, x.shape[1]))
    tgt, src, typ = ei[0][order], ei[1][order], typ[order]
    msg = rot(rel[:, typ], x[:, src])
    if w is not None:
        msg = msg * w[order].view(1, -1, 1)
    count = torch.bincount(tgt, minlength=num_node)
    start = count.cumsum(0) - count
    fin = torch.finfo(x.dtype)
    ident = {"add": 0.0, "min": fin.max, "max": fin.min}[sum]
    op = {"add": torch.add, "min": torch.minimum, "max": torch.maximum}[sum]
    acc = torch.full((x.shape[0], num_node, x.shape[2]), ident, dtype=x.dtype)
    for k in range(int(count.max()) if count.numel() else 0):
        nodes = (count > k).nonzero().flatten()
        acc[:, nodes] = op(acc[:, nodes], msg[:, start[nodes] + k])
    if boundary is not None:
        acc = op(acc, boundary)
    if point is not None:
        rows, vals = point
        b = torch.arange(x.shape[0])
        acc[b, rows] = op(acc[b, rows], vals)
    return acc


def assert_within(got, want, mass, n, what=""):
    eps = torch.finfo(got.dtype).eps
    bound = (2.0 + float(n) ** 0.5) * eps * mass.to(got.dtype) + 10 * torch.finfo(got.dtype).tiny
    diff = (got - want.to(got.dtype)).abs()
    bad = diff > bound
    assert not bad.any(), "%s: max excess %g at %s" % (what, (diff - bound).max().item(), bad.nonzero()[0].tolist())


def scatter_rows(values, index, n):
    return torch.zeros(values.shape[0], n, values.shape[2], dtype=values.dtype).index_add_(1, index, values)


def operands(seed, bs, d, dtype, n=50, r=7, unit=False, ints=False):
    ei, typ = helpers.random_graph(n, 400, r, seed=seed, hub=(3, 300), empty_rows=4, duplicates=20)
    g = torch.Generator().manual_seed(seed + 100)
    E = ei.shape[1]
    if ints:       # forced ties: values from a small integer set
        rel = torch.randint(-1, 2, (bs, r, d), generator=g).to(dtype)
        x = torch.randint(-1, 2, (bs, n, d), generator=g).to(dtype)
        bnd = torch.randint(-3, 4, (bs, n, d), generator=g).to(dtype)
        og = torch.randint(-2, 3, (bs, n, d), generator=g).to(dtype)
    else:
        rel = torch.randn(bs, r, d, generator=g, dtype=torch.float64).to(dtype)
        x = torch.randn(bs, n, d, generator=g, dtype=torch.float64).to(dtype)
        bnd = torch.randn(bs, n, d, generator=g, dtype=torch.float64).to(dtype)
        og = torch.randn(bs, n, d, generator=g, dtype=torch.float64).to(dtype)
    w = None if unit else (torch.rand(E, generator=g, dtype=torch.float64) + 0.5).to(dtype)
    return ei, typ, w, rel, x, bnd, og, n, r


def flipped(g, order):
    """The golden's (source, target) list as the engine's (target, source) rows."""
    return g["graph"][order]["edge_index"].flip(0).contiguous(), g["graph"][order]["edge_type"]


def dv(t, dev):
    return None if t is None else t.to(dev)


# ---- the operator against the reference ----
@pytest.mark.parametrize("aggr", AGGRS)
def test_exact_order_plan_equals_the_reference_aggregate(dev, golden, aggr):
    g = golden
    assert g["sorted_scatter_is_sequential"]
    n, r = g["num_node"], g["num_relation"]
    rel = g["state"]["relation.weight"].expand(g["x"].shape[0], -1, -1)
    for order in ("sorted", "shuffled") if aggr in ("max", "min") else ("sorted",):
        ei, typ = flipped(g, order)
        plan = rspmm.Plan(ei, typ, n, r, exact_order=True)
        assert plan.info()["n_chain_row"] >= 1
        got = plan.forward(rel.to(dev), g["x"].to(dev), boundary=g["boundary"].to(dev), sum=SUM_OF[aggr], mul="rotate").cpu()
        if aggr == "mean":
            got = got / (torch.bincount(ei[0], minlength=n) + 1).to(got.dtype).view(1, -1, 1)
        assert torch.equal(got, g[aggr]["sorted"]["aggregate"]), (aggr, order, (got - g[aggr]["sorted"]["aggregate"]).abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [64, 32, 40, 128, 34])     # 64: the lane exchange; 34: one element a lane
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_exact_order_plan_equals_the_sequential_restatement(dev, dtype, d, sum):
    for bs, unit in ((1, True), (3, False)):
        ei, typ, w, rel, x, bnd, _, n, r = operands(11 + bs, bs, d, dtype, unit=unit)
        plan = rspmm.Plan(ei, typ, n, r, exact_order=True)
        assert plan.info()["n_chain_row"] >= 1
        want = sequential(ei, typ, w, rel, x, n, sum=sum, boundary=bnd)
        got = plan.forward(rel.to(dev), x.to(dev), edge_weight=dv(w, dev), boundary=bnd.to(dev), sum=sum, mul="rotate").cpu()
        assert torch.equal(got, want), (bs, (got - want).abs().max())
        # no boundary: rows without in-edges keep the identity
        want = sequential(ei, typ, w, rel, x, n, sum=sum)
        got = plan.forward(rel.to(dev), x.to(dev), edge_weight=dv(w, dev), sum=sum, mul="rotate").cpu()
        assert torch.equal(got, want)
        # a relation table shared by the samples (stride 0), as the layer passes it
        shared = rel[:1].expand(bs, -1, -1)
        want = sequential(ei, typ, w, shared, x, n, sum=sum, boundary=bnd)
        got = plan.forward(shared.to(dev)[:1].expand(bs, -1, -1), x.to(dev), edge_weight=dv(w, dev), boundary=bnd.to(dev), sum=sum,
                           mul="rotate").cpu()
        assert torch.equal(got, want)
        # point boundary: served under add; under min / max correct or a clean "unsupported" (None)
        rows = torch.tensor([3, 7, 49][:bs])
        vals = bnd[torch.arange(bs), rows]
        got = plan.forward(rel.to(dev), x.to(dev), edge_weight=dv(w, dev), sum=sum, mul="rotate", point=(rows.to(dev), vals.to(dev)))
        if sum == "add":
            assert torch.equal(got.cpu(), sequential(ei, typ, w, rel, x, n, sum=sum, point=(rows, vals)))
        elif got is not None:
            dense = torch.zeros_like(bnd)
            dense[torch.arange(bs), rows] = vals
            assert torch.equal(got.cpu(), sequential(ei, typ, w, rel, x, n, sum=sum, boundary=dense))


def test_exact_order_plan_on_the_shuffled_golden_graph(dev, golden):
    g = golden
    n, r = g["num_node"], g["num_relation"]
    ei, typ = flipped(g, "shuffled")
    rel = g["state"]["relation.weight"].expand(g["x"].shape[0], -1, -1).contiguous()
    plan = rspmm.Plan(ei, typ, n, r, exact_order=True)
    for sum in ("add", "min", "max"):
        want = sequential(ei, typ, None, rel, g["x"], n, sum=sum, boundary=g["boundary"])
        got = plan.forward(rel.to(dev), g["x"].to(dev), boundary=g["boundary"].to(dev), sum=sum, mul="rotate").cpu()
        assert torch.equal(got, want), sum


def test_2d_operands_and_odd_rows(dev):
    """(N, D): the whole row is one complex vector; generalized_rspmm takes mul="rotate"; an odd row length is refused."""
    ei, typ, w, rel, x, _, _, n, r = operands(5, 1, 64, torch.float32)
    want = sequential(ei, typ, w, rel, x, n)[0]
    got = rspmm.generalized_rspmm(ei.to(dev), typ.to(dev), w.to(dev), rel[0].to(dev), x[0].to(dev), sum="add", mul="rotate").cpu()
    assert torch.equal(got, want)
    assert rspmm.RSPMMMaxRotateFunction.__name__ == "RSPMMMaxRotateFunction"
    plan = rspmm.Plan(ei, typ, n, r)
    with pytest.raises(_lib.UltraError):
        plan.forward(rel[0, :, :63].contiguous().to(dev), x[0, :, :63].contiguous().to(dev), mul="rotate")


# ---- re-associating plans and gradients ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [64, 40])
def test_reassociating_plan_and_add_gradients_within_the_bound(dev, dtype, d):
    bs = 3
    ei, typ, w, rel, x, bnd, og, n, r = operands(21, bs, d, dtype)
    plan = rspmm.Plan(ei, typ, n, r, exact_order=False, seg_len=64, g_max=16)
    assert plan.info()["n_split_row"] >= 1 and plan.info()["n_wave_item"] >= 1
    tgt, src = ei
    wv = w.view(1, -1, 1)
    deg = int(torch.bincount(tgt, minlength=n).max())
    mass = scatter_rows(rot_mass(rel[:, typ], x[:, src]) * wv, tgt, n) + bnd.abs()
    want = sequential(ei, typ, w, rel, x, n, boundary=bnd)
    rel_d, x_d, w_d, bnd_d = (t.to(dev).requires_grad_() for t in (rel, x, w, bnd))
    out = rspmm.plan_rspmm(plan, rel_d, x_d, w_d, sum="add", mul="rotate", boundary=bnd_d)
    assert_within(out.detach().cpu(), want, mass, 2 * deg + 1, "forward")
    for s in ("min", "max"):       # order-free
        got = plan.forward(rel.to(dev), x.to(dev), edge_weight=w.to(dev), boundary=bnd.to(dev), sum=s, mul="rotate").cpu()
        assert torch.equal(got, sequential(ei, typ, w, rel, x, n, sum=s, boundary=bnd)), s
    out.backward(og.to(dev))
    # fp64 autograd of the torch restatement
    rel6, x6, w6, bnd6 = (t.double().requires_grad_() for t in (rel, x, w, bnd))
    (scatter_rows(rot(rel6[:, typ], x6[:, src]) * w6.view(1, -1, 1), tgt, n) + bnd6).backward(og.double())
    g_t = og[:, tgt]
    assert_within(x_d.grad.cpu(), x6.grad, scatter_rows(rot_mass(rel[:, typ], g_t) * wv, src, n),
                  2 * int(torch.bincount(src, minlength=n).max()), "input_grad")
    assert_within(rel_d.grad.cpu(), rel6.grad, scatter_rows(rot_mass(x[:, src], g_t) * wv, typ, r),
                  2 * int(torch.bincount(typ, minlength=r).max()), "relation_grad")
    assert torch.equal(bnd_d.grad.cpu(), og)
    wmass = (rot_mass(rel[:, typ], x[:, src]) * g_t.abs()).sum(dim=(0, 2))
    eps = torch.finfo(dtype).eps
    assert ((w_d.grad.cpu() - w6.grad.to(dtype)).abs() <= (2 + (2 * bs * d) ** 0.5) * eps * wmass + 1e-30).all(), "weight_grad"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [64, 40, 34])
@pytest.mark.parametrize("sum", ["min", "max"])
def test_minmax_gradients_with_forced_ties(dev, dtype, d, sum):
    """Small integers: every product and sum is exact, ties abound.  Every tying edge gets the full gradient, per ELEMENT: a
    tying real element sends gradient to both halves of x and rel (operator.cuh:62-64 applied to the complex product)."""
    bs = 2
    ei, typ, _, rel, x, _, og, n, r = operands(31, bs, d, dtype, ints=True)
    tgt, src = ei
    plan = rspmm.Plan(ei, typ, n, r, exact_order=False, seg_len=64, g_max=16)
    rel_d, x_d = rel.to(dev).requires_grad_(), x.to(dev).requires_grad_()
    w_d = torch.ones(ei.shape[1], dtype=dtype, device=dev).requires_grad_()
    out = rspmm.plan_rspmm(plan, rel_d, x_d, w_d, sum=sum, mul="rotate")
    want = sequential(ei, typ, None, rel, x, n, sum=sum)
    assert torch.equal(out.detach().cpu(), want)
    out.backward(og.to(dev))
    msg = rot(rel[:, typ], x[:, src])
    tie = (msg == want[:, tgt]).to(dtype)
    assert tie.sum() >= 1.5 * (want.numel() - bs * 4 * d), "the operands force too few ties"      # (4 rows have no in-edges)
    gt = og[:, tgt] * tie
    assert torch.equal(x_d.grad.cpu(), scatter_rows(rot(rel[:, typ], gt, conj_r=True), src, n))
    assert torch.equal(rel_d.grad.cpu(), scatter_rows(rot(gt, x[:, src], conj_x=True), typ, r))
    assert torch.equal(w_d.grad.cpu(), (gt * msg).sum(dim=(0, 2)))
    # two runs, the same bits (a gather in a fixed order: no atomics)
    again = plan.backward(rel.to(dev), x.to(dev), out.detach(), og.to(dev), sum=sum, mul="rotate")
    assert torch.equal(again[1], rel_d.grad) and torch.equal(again[2], x_d.grad)


# ---- keep vectors ----
@pytest.mark.parametrize("sum", ["add", "max"])
def test_keep_vector_equals_the_filtered_graph(dev, sum):
    bs, d = 3, 64
    ei, typ, _, rel, x, bnd, og, n, r = operands(41, bs, d, torch.float32)
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(ei.shape[1], generator=g) > 0.3).float()
    sel = keep.bool()
    full = rspmm.Plan(ei, typ, n, r, exact_order=True)
    filt = rspmm.Plan(ei[:, sel].contiguous(), typ[sel].contiguous(), n, r, exact_order=True)
    a = full.forward(rel.to(dev), x.to(dev), edge_weight=keep.to(dev), boundary=bnd.to(dev), sum=sum, mul="rotate", keep=True)
    b = filt.forward(rel.to(dev), x.to(dev), boundary=bnd.to(dev), sum=sum, mul="rotate")
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), sequential(ei, typ, keep, rel, x, n, sum=sum, boundary=bnd, keep=True))
    if sum == "max":     # "absent", not "zero": a zero weight would enter the maximum with the value 0
        z = full.forward(rel.to(dev), x.to(dev), edge_weight=keep.to(dev), boundary=bnd.to(dev), sum=sum, mul="rotate")
        assert not torch.equal(z, a)
    # backward: dropped edges get no weight gradient, the other gradients are the filtered graph's
    out = full.forward(rel.to(dev), x.to(dev), edge_weight=keep.to(dev), sum=sum, mul="rotate", keep=True)
    wg, rg, xg = full.backward(rel.to(dev), x.to(dev), out, og.to(dev), edge_weight=keep.to(dev), need_weight_grad=True, sum=sum,
                               mul="rotate", keep=True)
    assert (wg.cpu()[~sel] == 0).all() and (wg.cpu()[sel] != 0).any()
    out_f = filt.forward(rel.to(dev), x.to(dev), sum=sum, mul="rotate")
    _, rg_f, xg_f = filt.backward(rel.to(dev), x.to(dev), out_f, og.to(dev), sum=sum, mul="rotate")
    tgt, src = ei[:, sel]
    g_t = og[:, tgt]
    assert_within(xg.cpu(), xg_f.cpu(), scatter_rows(rot_mass(rel[:, typ[sel]], g_t), src, n),
                  2 * int(torch.bincount(src, minlength=n).max()), "input_grad")
    assert_within(rg.cpu(), rg_f.cpu(), scatter_rows(rot_mass(x[:, src], g_t), typ[sel], r),
                  2 * int(torch.bincount(typ[sel], minlength=r).max()), "relation_grad")


# ---- the layer ----
def golden_layer(g, aggr, dev):
    layer = layers.GeneralizedRelationalConv(64, 64, g["num_relation"], 64, "rotate", aggr, True, "relu")
    layer.load_state_dict(g["state"])
    return layer.to(dev)


@pytest.mark.parametrize("aggr", AGGRS)
def test_layer_matches_the_reference_layer(dev, golden, aggr, monkeypatch):
    g = golden
    n = g["num_node"]
    layer = golden_layer(g, aggr, dev)
    for order in ("sorted", "shuffled"):
        ei, typ = g["graph"][order]["edge_index"].to(dev), g["graph"][order]["edge_type"].to(dev)
        want = g[aggr][order]["out"]
        tol = 1e-4 * max(1.0, want.abs().max().item())
        for fused in (True, False):
            monkeypatch.setattr(layers, "FUSED_ROTATE", fused)
            with torch.no_grad():
                got = layer(g["x"].to(dev), g["query"].to(dev), g["boundary"].to(dev), ei, typ, (n, n)).cpu()
            err = (got - want).abs().max().item()
            print("rotate layer %s / %s / fused=%s: max |got - reference| = %.3g, bit-equal end to end: %s; reference fp32 to fp64: %.3g"
                  % (aggr, order, fused, err, torch.equal(got, want), (g[aggr]["sorted"]["out"].double() - g[aggr]["out64"]).abs().max()))
            assert err <= tol, (aggr, order, fused, err)


def test_fused_rotate_layer_is_reproducible_and_takes_the_engine(dev, golden, monkeypatch):
    g = golden
    n = g["num_node"]
    layer = golden_layer(g, "sum", dev)
    ei, typ = g["graph"]["shuffled"]["edge_index"].to(dev), g["graph"]["shuffled"]["edge_type"].to(dev)
    args = (g["x"].to(dev), g["query"].to(dev), g["boundary"].to(dev), ei, typ, (n, n))
    calls = []
    inner = rspmm.Plan.forward
    monkeypatch.setattr(rspmm.Plan, "forward", lambda self, *a, **k: (calls.append(k.get("mul")), inner(self, *a, **k))[1])
    with torch.no_grad():
        a, b = layer(*args), layer(*args)
    assert torch.equal(a, b) and calls == ["rotate", "rotate"]
    monkeypatch.setattr(layers, "FUSED_ROTATE", False)
    with pytest.raises(RuntimeError):      # a keep vector still has no meaning on the unfused route
        layer._forward_impl(*args, edge_weight=torch.ones(ei.shape[1], device=dev), edge_keep=True)


@pytest.mark.parametrize("aggr", ["sum", "max"])
def test_layer_gradients_match_the_reference_layer(dev, golden, aggr):
    """d out.backward(og) of the fused layer against the reference layer's CPU autograd (golden), at the tolerance of the
    project's train-mode test: 1e-4 of the gradient's scale (max: Frobenius norm -- near-ties may fall either way).
    max: the golden graph has duplicate edges, whose messages tie EXACTLY.  torch's scatter_reduce("amax") backward -- what the
    reference's unfused route ends in -- splits the gradient evenly among the ties; the engine follows the reference's rspmm rule,
    every tying edge in full (operator.cuh:62-64; pinned by test_minmax_gradients_with_forced_ties).  The two differ on this
    graph by construction (measured: |x.grad difference| = 10.1 against a norm of 31.9), so under max the golden pins what no tie
    rule touches -- the gradients of the update's parameters, which see the aggregate's VALUES and the output gradient only --
    and the input / boundary / relation gradients are pinned under sum."""
    g = golden
    n = g["num_node"]
    layer = golden_layer(g, aggr, dev)
    ei, typ = g["graph"]["sorted"]["edge_index"].to(dev), g["graph"]["sorted"]["edge_type"].to(dev)
    x, bnd = g["x"].to(dev).requires_grad_(), g["boundary"].to(dev).requires_grad_()
    layer(x, g["query"].to(dev), bnd, ei, typ, (n, n)).backward(g["og"].to(dev))
    got = {"x": x.grad, "boundary": bnd.grad}
    got.update({"params." + k: p.grad for k, p in layer.named_parameters()})
    want = {"x": g["grads"][aggr]["x"], "boundary": g["grads"][aggr]["boundary"]}
    want.update({"params." + k: v for k, v in g["grads"][aggr]["params"].items()})
    assert set(want) <= set(got)
    for k, w in want.items():
        if aggr == "max" and not (k.startswith("params.linear") or k.startswith("params.layer_norm")):
            continue
        diff = got[k].cpu() - w
        if aggr == "max":
            assert diff.norm().item() <= 1e-4 * max(w.norm().item(), 1e-6) + 1e-7, k
        else:
            assert diff.abs().max().item() <= 1e-4 * max(w.abs().max().item(), 1e-6) + 1e-7, k


def test_fused_rotate_forward_allocates_no_edge_sized_tensor(dev, monkeypatch):
    """A condition, not a measurement: N = 2,000, |E| = 200,000, batch 4, d = 64, fp32, no_grad -- the layer's forward raises the
    peak by less than ONE (batch, |E|, d) tensor (205 MB; the fused route needs a few node-sized ones of 2 MB), the unfused
    route by more: the bound bites."""
    n, e, r, bs, d = 2000, 200000, 8, 4, 64
    g = torch.Generator().manual_seed(2)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    typ = torch.randint(0, r, (e,), generator=g).to(dev)
    torch.manual_seed(3)
    layer = layers.GeneralizedRelationalConv(d, d, r, d, "rotate", "sum", True, "relu").to(dev)
    x, bnd, query = (torch.randn(s, generator=g).to(dev) for s in ((bs, n, d), (bs, n, d), (bs, d)))
    edge_sized = e * bs * d * 4
    peaks = {}
    for fused in (True, False):
        monkeypatch.setattr(layers, "FUSED_ROTATE", fused)
        with torch.no_grad():
            if fused:
                layer(x, query, bnd, ei, typ, (n, n))      # (the plan is built before the peak is reset)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.max_memory_allocated()
            out = layer(x, query, bnd, ei, typ, (n, n))
            torch.cuda.synchronize()
            peaks[fused] = torch.cuda.max_memory_allocated() - base
            del out
    print("rotate layer forward, peak above the operands: fused %.1f MB, unfused %.1f MB (one edge-sized tensor: %.1f MB)"
          % (peaks[True] / 1e6, peaks[False] / 1e6, edge_sized / 1e6))
    assert peaks[True] < edge_sized
    assert peaks[False] > edge_sized


# ---- the model ----
@pytest.mark.parametrize("aggr", AGGRS)
def test_training_step_keep_vector_route_against_edge_removal(dev, aggr, monkeypatch):
    """Ultra with a rotate entity model in train() mode on a batch of graph edges: the keep-vector route on the engine against
    the reference's route -- remove_easy_edges + the unfused layer (FUSED_ROTATE = False) -- at the tolerances of
    tests/test_models_gpu.py's train-mode test: scores 1e-4, loss 1e-5, every parameter gradient within 1e-4 of its scale
    (max / min: Frobenius norm).  That test also allows 4 x the distance of a CPU fp32 run from fp64; the model has no fp64
    route on the GPU (its relation model's kernels are fp32), so this one goes without that allowance: the stricter bound.
    max / min: scores and loss against that route as well, but NOT the gradients -- the hidden states are ReLU outputs, so many
    messages are exact zeros that tie, and at a tie torch's amax / amin backward (the unfused route) splits the gradient evenly
    where the engine gives it to every tying edge in full (the reference's rspmm rule, operator.cuh:62-64; pinned by
    test_minmax_gradients_with_forced_ties).  Measured on this step: relation_model.layers.0.layer_norm.weight differs by a
    Frobenius norm of 0.173 at a scale of 0.044 between the two rules.  Their gradients are therefore compared, at the same
    tolerance, with the route that shares the tie rule: the engine on the graph remove_easy_edges leaves (the entity model in
    eval() mode on the filtered copy, as test_training_edge_dropout_by_weight_equals_edge_removal does for DistMult) -- which
    is what the keep vector has to reproduce."""
    from ultra_amd import train
    cfg = synthetic.default_model_cfg(aggregate_func=aggr)
    cfg = {k: dict(v) for k, v in cfg.items()}
    cfg["entity_model_cfg"]["message_func"] = "rotate"
    if aggr == "min":       # (the relation model's DistMult layers have no min aggregate)
        cfg["rel_model_cfg"]["aggregate_func"] = "sum"
    torch.manual_seed(17)
    model = models.Ultra(**cfg)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    data = synthetic.make_kg(num_node=300, num_triple=2400, num_relation_base=5, num_test=16, seed=4)
    # repeated triples are dropped: their messages tie exactly, and at a tie torch's amax / amin backward (the unfused route)
    # splits the gradient where the rspmm rule gives it in full (operator.cuh:62-64) -- the two routes agree off ties only
    key = (data.edge_index[0] * data.num_nodes + data.edge_index[1]) * data.num_relations + data.edge_type
    first = torch.zeros(key.numel(), dtype=torch.bool)
    first[torch.sort(key, stable=True)[1][torch.cat([torch.ones(1, dtype=torch.bool), key.sort()[0].diff() != 0])]] = True
    data.edge_index, data.edge_type = data.edge_index[:, first].contiguous(), data.edge_type[first].contiguous()
    pick = torch.tensor([0, 7, 900, 1900])
    batch = torch.stack([data.edge_index[0, pick], data.edge_index[1, pick], data.edge_type[pick]], dim=-1)
    assert (batch[:, 2] < data.num_relations // 2).all()
    torch.manual_seed(0)
    neg = tasks.negative_sampling(data, batch, 8, strict=True)
    num_negative = neg.shape[1] - 1
    gdata = data.to(dev)

    def step(fused, removed=False):
        monkeypatch.setattr(layers, "FUSED_ROTATE", fused)
        m = models.Ultra(**cfg)
        m.load_state_dict(state)
        m = m.to(dev).train()
        used = []
        graph = gdata
        if removed:       # the engine on the filtered copy of the graph
            graph = m.entity_model.remove_easy_edges(gdata, *neg.to(dev).unbind(-1))
            assert graph.num_edges < gdata.num_edges
            m.entity_model.eval()
        elif fused:
            inner = m.entity_model.remove_easy_edges
            monkeypatch.setattr(m.entity_model, "remove_easy_edges", lambda *a, **k: (used.append(1), inner(*a, **k))[1])
        pred = m(graph, neg.to(dev))
        loss = train.ranking_loss(pred, 0.5, num_negative)
        loss.backward()
        assert not used, "the fused route rebuilt the graph"
        return loss.item(), pred.detach().cpu(), {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None}

    loss_f, pred_f, g_f = step(True)
    loss_u, pred_u, g_u = step(False)
    assert (pred_f - pred_u).abs().max().item() <= 1e-4
    assert abs(loss_f - loss_u) <= 1e-5, (loss_f, loss_u)
    assert set(g_f) == set(g_u)
    if aggr in ("max", "min"):
        _, pred_r, g_u = step(True, removed=True)
        assert (pred_f - pred_r).abs().max().item() <= 1e-4
    for name, want in g_u.items():
        if aggr in ("max", "min"):
            scale, err = max(want.norm().item(), 1e-6), (g_f[name] - want).norm().item()
        else:
            scale, err = max(want.abs().max().item(), 1e-6), (g_f[name] - want).abs().max().item()
        assert err <= 1e-4 * scale + 1e-7, "%s: |keep vector - edge removal| = %g (scale %g)" % (name, err, scale)
