"""The backward of rspmm under sum == "add" against the C oracle in fp64, shared by the GPU test (test_rspmm_gpu.py) and
the CPU self-check of its bound (test_backward_bounds_cpu.py).

Operands are batch-major (bs, rows, d) in the dtype of the code under test; the oracle sees them in fp64 with the batch
folded into the feature axis, as the reference's layer calls it (layers.py:189-230).  Every gradient element is a sum of
known terms, so each is held to a bound on those terms (helpers.assert_sum_close's random-walk bound for the input and
relation gradients -- see check() for the one kind of sum it does not describe --, helpers.assert_within's worst case for
the weight gradient):
  input_grad[b, col]     = sum over the edges out of col of  w * d msg / d x   * output_grad[b, row]
                           -- an rspmm over the transposed edge list with output_grad as the input;
  relation_grad[b, type] = sum over the edges of that type of  w * d msg / d rel * output_grad[b, row]
                           -- an rspmm over the (type, col) list with output_grad in the relation operand's place;
  weight_grad[e]         = sum over (b, d) of  msg * output_grad[b, row]: bs * d terms (assert_within of the min / max file).
Under mul == "add" the message's derivative is 1: the terms are w * output_grad, a product with a table of ones."""
import torch

from oracle import rspmm_oracle
from tests import helpers
from tests.helpers import assert_within

SHAPES = [(torch.float32, 30), (torch.float32, 128), (torch.float32, 200), (torch.float64, 72)]
CASES = [1, 6, 7]      # of helpers.RSPMM_CASES: hub; relation slice larger than the x slice; dense, type-run twin
LAYOUTS = ("2d", "batch", "shared")
WEIGHTS = ("none", "random", "keep")


def fold(t):
    """(bs, rows, d) -> (rows, bs * d)"""
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def unfold(t, bs):
    """(rows, bs * d) -> (bs, rows, d)"""
    return t.view(t.shape[0], bs, -1).transpose(0, 1)


def make_operands(case, d, dtype, layout, weights, mul, seed=0):
    """Seeded operands of one call on helpers.RSPMM_CASES[case]: rel (bs, R, d) -- (1, R, d) for the shared table --, x, og and base (bs, N, d), w (E,)
    or None; 2d is a batch of one."""
    case = helpers.RSPMM_CASES[case]
    ei, et = helpers.random_graph(**case)
    N, R, E = case["num_node"], case["num_relation"], ei.shape[1]
    bs = 1 if layout == "2d" else 3
    g = torch.Generator().manual_seed(1000 * case["seed"] + seed)
    draw = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
    rel = draw(1 if layout == "shared" else bs, R, d)
    x, og, base = draw(bs, N, d), draw(bs, N, d), draw(bs, N, d)
    w = None
    if weights == "random":
        w = (torch.rand(E, generator=g, dtype=torch.float64) + 0.5).to(dtype)
    elif weights == "keep":
        w = (torch.rand(E, generator=g) > 0.3).to(dtype)
    return dict(ei=ei, et=et, N=N, R=R, E=E, bs=bs, d=d, rel=rel, x=x, og=og, base=base, w=w, layout=layout,
                weights=weights, mul=mul)


def oracle_backward(ops, dtype):
    """rspmm_oracle.rspmm_backward in `dtype` on the folded operands: (weight_grad in the caller's edge order, relation_grad
    (bs, R, d), input_grad (bs, N, d))."""
    bs, E = ops["bs"], ops["E"]
    w = torch.ones(E, dtype=dtype) if ops["w"] is None else ops["w"].to(dtype)
    sei, set_, sw, order = rspmm_oracle.sort_edges(ops["ei"], ops["et"], w)
    rel = fold(ops["rel"].expand(bs, -1, -1).to(dtype))
    x, og = fold(ops["x"].to(dtype)), fold(ops["og"].to(dtype))
    return _oracle_backward(sei, set_, sw, order, rel, x, og, bs, ops["mul"])


def _oracle_backward(sei, set_, sw, order, rel, x, og, bs, mul):
    out = rspmm_oracle.rspmm_forward(sei, set_, sw, rel, x, sum="add", mul=mul)
    wg_s, rg, xg = rspmm_oracle.rspmm_backward(sei, set_, sw, rel, x, out, og, sum="add", mul=mul)
    wg = torch.empty_like(wg_s)
    wg[order] = wg_s
    return wg, unfold(rg, bs), unfold(xg, bs)


def check(ops, dtype, got_w, got_rel, got_x, got_total=None):
    """got_* as the code under test returned them in `dtype`: weight_grad (E,) or None, the relation LEAF's gradient
    ((R, d) for the 2d and shared layouts: shared is the batch sum), input_grad and, where given, base + input_grad."""
    f64 = torch.float64
    bs, N, R, E, d, mul = ops["bs"], ops["N"], ops["R"], ops["E"], ops["d"], ops["mul"]
    assert R <= N, "the oracle's output has as many rows as its input: the (type, col) list needs R <= N"
    row, col = ops["ei"]
    typ = ops["et"]
    want_w, want_rel, want_x = oracle_backward(ops, f64)
    w = torch.ones(E, dtype=f64) if ops["w"] is None else ops["w"].to(f64)
    rel = fold(ops["rel"].expand(bs, -1, -1).to(f64))
    x, og = fold(ops["x"].to(f64)), fold(ops["og"].to(f64))
    ones = torch.ones_like(x)
    # input gradient: the transposed list, output_grad as input; mul == "add": relation table of ones
    t_ei = torch.stack([col, row])
    t_rel = rel if mul == "mul" else torch.ones_like(rel)
    kw = dict(mul="mul", dtype=dtype)
    helpers.assert_sum_close(fold(got_x.view(bs, N, d)), fold(want_x), t_ei, typ, w, t_rel, og, **kw)
    if got_total is not None:
        base = fold(ops["base"].to(f64))
        helpers.assert_sum_close(fold(got_total.view(bs, N, d)), fold(want_x) + base, t_ei, typ, w, t_rel, og, boundary=base, **kw)
    # relation gradient: the (type, col) list, output_grad (indexed by the edge's row) in the relation operand's place, under
    # the same random-walk bound k eps mass, k = 2 + sqrt(n), n the largest number of terms of an element -- except where
    # the terms are not independent draws: under mul == "add" a term is w * output_grad[row], so a type most of whose
    # edges enter ONE row (the hub of RSPMM_CASES[1]: about 233 of each type's 308 to 351 edges) sums mostly copies of one
    # number, and adding one number over and over rounds the same way at every step.  The oracle's own sequential fp32
    # backward is off by 2.46e-3 there (d = 128, seed 1, type 2, column 42: 351 terms, mass 627.3; the random walk allows
    # (2 + sqrt(351)) eps mass = 1.55e-3, the worst case 352 eps mass = 2.63e-2), 1.3 to 1.6 times the random-walk bound at
    # d = 30, 128 and 200, while it is within it on every other graph and under mul == "mul" (<= 0.91 of it).  So the
    # types whose terms are in their majority copies of one row's -- decided from the edge list, under mul == "add" only
    # -- take the worst case k = n + 1 (assert_within's bound); every other element keeps the random walk.
    r_ei = torch.stack([typ, col])
    r_x = x if mul == "mul" else ones
    n_type = torch.bincount(typ, minlength=R)
    copies = torch.bincount(typ * N + row, minlength=R * N).view(R, N).max(1).values      # of one row among a type's terms
    n_term = (bs if ops["layout"] == "shared" else 1) * n_type.to(f64)      # (shared: the leaf's gradient is the batch sum)
    k = torch.full((R,), 2.0 + float(n_term.max()) ** 0.5, dtype=f64)
    if mul == "add":
        k = torch.where(2 * copies > n_type, n_term + 1, k)
    if ops["layout"] == "shared":
        mass = unfold(rspmm_oracle.generalized_rspmm(r_ei, row, w, og.abs(), r_x.abs(), sum="add", mul="mul"), bs)[:, :R].sum(0)
        bound = k.view(R, 1) * torch.finfo(dtype).eps * mass + 10 * torch.finfo(f64).tiny
        diff = (got_rel.to(f64) - want_rel.sum(0)).abs()
        bad = diff > bound
        assert not bad.any(), "shared relation grad: max excess %g at %s" % ((diff - bound).max().item(), bad.nonzero()[0].tolist())
    else:
        pad = lambda t, fill: torch.cat([t, torch.full((N - R,) + t.shape[1:], fill, dtype=f64)])
        helpers.assert_sum_close(pad(fold(got_rel.view(bs, R, d).to(f64)), 0.0), pad(fold(want_rel), 0.0), r_ei, row, w, og, r_x,
                                 k=pad(k.view(R, 1), 1.0), **kw)
    # weight gradient: bs * d terms an edge, worst-case bound
    if got_w is not None:
        if ops["weights"] == "keep":      # a dropped edge is absent: its weight gradient is zero
            want_w = want_w * (w != 0)
        msg = rel[typ] * x[col] if mul == "mul" else rel[typ] + x[col]
        mass = (og[row] * msg).abs().sum(1)
        assert_within(got_w, want_w, mass, torch.full_like(mass, bs * d), torch.finfo(dtype).eps / 2, "weight grad")
