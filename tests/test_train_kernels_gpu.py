"""The small kernels every training step runs -- ranking_loss_kernel, query_loss_kernel, strict_negative_kernel and the two hash
filters of the easy edges -- against the plain restatements of tests/test_train_kernels_cpu.py, at the shapes, draws and table
fills where such kernels go wrong.

The two losses are held, element by element, to the fp64 reference within a few times the error of torch's own fp32 op chain
plus a floor of 16 ulp of the element's weight scale s_i (which bounds the element's gradient):

    |got_i - want_i| <= 4 |torch32_i - want_i| + 16 eps32 s_i,     s_i = w_i / (sum_j w_j * rows)

The factor 4 allows for the kernels' sums and their exp argument running in another, equally valid order; the floor for sigmoid,
exp, two divisions and the scale at 1-2 ulp each.  With ULTRA_TRAIN_KERNELS_RECORD=<file> the largest |got_i - want_i| / s_i seen
per kernel and temperature, and torch's, are written to that file (profiles/train_kernels_tests.txt is such a record).
"""
import os

import numpy as np
import pytest
import torch

from tests.test_train_gpu import reference_loss
from tests.test_train_kernels_cpu import (EPS32, QUERY_SHAPES, QUERY_TARGETS, QUERY_TEMPERATURES, RANKING_FALLBACK_SHAPES,
                                          RANKING_OTHER_NUM_NEGATIVE, RANKING_SHAPES, RANKING_TEMPERATURES, SAMPLER_DRAWS,
                                          SAMPLER_NODES, WRAP_TABLES, brute_strict_negatives, capacity_case, query_case,
                                          query_weights, ranking_logits, ranking_weights, sampler_graph, sampler_rand, valid_ids,
                                          weight_scale, wrap_case)
from ultra_amd import _lib, dense, models, query_train, tasks, train
from ultra_amd.query_train import query_loss_reference

pytestmark = pytest.mark.gpu

_RECORD = {}
FLT_MIN = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    path = os.environ.get("ULTRA_TRAIN_KERNELS_RECORD")
    if path and _RECORD:
        with open(path, "w") as f:
            f.write("largest |x_i - fp64_i| / s_i over the elements with s_i >= FLT_MIN of all cases, in units of eps32 = 2^-23 "
                    "(s_i = w_i / (sum_j w_j * rows); the tests allow 4 x torch's error of that element + 16)\n")
            f.write("%-14s %-6s %-12s %-12s %s\n" % ("kernel", "T", "kernel", "torch fp32", "worst case of the kernel"))
            for (kernel, temperature), (got, plain, where) in sorted(_RECORD.items()):
                f.write("%-14s %-6g %-12.3f %-12.3f %s\n" % (kernel, temperature, got, plain, where))


def _record(kernel, temperature, got, plain, want, scale, where):
    live = scale >= FLT_MIN          # (below it fp32 holds neither the weight nor the gradient to full precision)
    if not bool(live.any()):
        return
    mine = float(((got - want).abs()[live] / scale[live]).max()) / EPS32
    theirs = float(((plain - want).abs()[live] / scale[live]).max()) / EPS32
    old = _RECORD.get((kernel, temperature), (-1.0, -1.0, ""))
    _RECORD[(kernel, temperature)] = (max(old[0], mine), max(old[1], theirs), where if mine > old[0] else old[2])


def _assert_elements(got, plain, want, scale, where):
    """|got_i - want_i| <= 4 |plain_i - want_i| + 16 eps32 s_i for every element; all fp64 on the CPU."""
    err, bound = (got - want).abs(), 4 * (plain - want).abs() + 16 * EPS32 * scale
    if bool((err > bound).any()):
        i = int((err - bound).argmax())
        r, c = divmod(i, got.shape[1])
        raise AssertionError("%s: element (%d, %d): kernel %.9g, torch fp32 %.9g, fp64 %.17g, s_i %.9g: |err| %.3g = %.2f eps32 s_i, "
                             "torch's %.2f eps32 s_i; %d elements over the bound"
                             % (where, r, c, got[r, c], plain[r, c], want[r, c], scale[r, c], err[r, c],
                                err[r, c] / (EPS32 * scale[r, c]) if scale[r, c] > 0 else float("inf"),
                                (plain - want).abs()[r, c] / (EPS32 * scale[r, c]) if scale[r, c] > 0 else float("inf"),
                                int((err > bound).sum())))


def _assert_loss(got, plain, want, where):
    assert abs(got - want) <= 4 * abs(plain - want) + 16 * EPS32 * abs(want), \
        "%s: loss %.9g, torch fp32 %.9g, fp64 %.17g" % (where, got, plain, want)


# ---- A. ranking_loss_kernel ----
def _ranking(pred, temperature, num_negative, fused, times=1.0):
    train.FUSED_LOSS = fused
    try:
        p = pred.clone().requires_grad_()
        loss = train.ranking_loss(p, temperature, num_negative)
        (loss * times if times != 1.0 else loss).backward()
    finally:
        train.FUSED_LOSS = True
    return loss, p.grad


def _check_ranking(dev, rows, n, temperature, num_negative, kernel_route):
    for name, logits in ranking_logits(rows, n).items():
        where = "ranking_loss (%d, %d) T=%g num_negative=%d %s" % (rows, n, temperature, num_negative, name)
        p64 = logits.double().requires_grad_()
        want = reference_loss(p64, temperature, num_negative)
        want.backward()
        scale = weight_scale(ranking_weights(logits.double(), temperature, num_negative), rows)
        pred = logits.to(dev)
        plain, plain_grad = _ranking(pred, temperature, num_negative, fused=False)
        got, got_grad = _ranking(pred, temperature, num_negative, fused=True)
        assert (type(got.grad_fn).__name__ == "_RankingLossBackward") == kernel_route, where
        assert type(plain.grad_fn).__name__ != "_RankingLossBackward"
        assert got.dtype == torch.float32 and got_grad.dtype == torch.float32 and got_grad.shape == pred.shape
        got64, plain64 = got_grad.double().cpu(), plain_grad.double().cpu()
        if kernel_route:
            _record("ranking_loss", temperature, got64, plain64, p64.grad, scale, where)
        _assert_elements(got64, plain64, p64.grad, scale, where)
        _assert_loss(got.item(), plain.item(), want.item(), where)
        # the same bits on every run; an incoming gradient scales the stored one
        again, again_grad = _ranking(pred, temperature, num_negative, fused=True)
        assert torch.equal(again, got) and torch.equal(again_grad, got_grad), where
        if kernel_route:
            _, tripled = _ranking(pred, temperature, num_negative, fused=True, times=3.0)
            assert torch.equal(tripled, got_grad * 3), where


@pytest.mark.parametrize("temperature", RANKING_TEMPERATURES)
@pytest.mark.parametrize("rows,n", RANKING_SHAPES)
def test_ranking_loss_kernel_element_by_element(dev, rows, n, temperature):
    """One workgroup, one wave per row: a single row, fewer rows than waves, rows of 64 / 65 / 66 / 129 columns (the lanes'
    stride), the most rows and the most columns the kernel takes; all-equal, saturated and one-negative-dominates rows."""
    _check_ranking(dev, rows, n, temperature, n - 1, kernel_route=True)


@pytest.mark.parametrize("rows,n", [(2, 3), (64, 33), (4096, 33)])
def test_ranking_loss_kernel_uniform_weight_is_one_over_num_negative(dev, rows, n):
    """Temperature 0 with a num_negative that is not n - 1, as pre-training calls it."""
    _check_ranking(dev, rows, n, 0.0, RANKING_OTHER_NUM_NEGATIVE, kernel_route=True)


@pytest.mark.parametrize("temperature", RANKING_TEMPERATURES)
@pytest.mark.parametrize("rows,n", RANKING_FALLBACK_SHAPES)
def test_ranking_loss_beyond_the_kernel_takes_the_torch_route(dev, rows, n, temperature):
    """4097 rows or columns: train._fused_loss hands over to the op chain, which is held to the same bound."""
    _check_ranking(dev, rows, n, temperature, n - 1, kernel_route=False)


def test_ranking_loss_entry_refuses_what_the_kernel_cannot_hold(dev):
    pred = torch.zeros(4, 4, device=dev)
    loss, grad = torch.zeros((), device=dev), torch.zeros(4, 4, device=dev)
    call = lambda p, rows, n: _lib.lib.ultra_ranking_loss(p, rows, n, 1.0, 0.5, loss.data_ptr(), grad.data_ptr(), _lib.stream_of(pred))
    assert call(pred.data_ptr(), 4097, 2) == _lib.ULTRA_ERR_INVALID and call(pred.data_ptr(), 0, 4) == _lib.ULTRA_ERR_INVALID
    assert call(pred.data_ptr(), 4, 1) == _lib.ULTRA_ERR_INVALID and call(None, 4, 4) == _lib.ULTRA_ERR_INVALID
    assert call(pred.data_ptr(), 4, 4) == _lib.ULTRA_OK


# ---- B. query_loss_kernel ----
def _query_entry(pred, target, temperature, work):
    """ultra_query_loss itself on a workspace the test owns: (loss, grad)."""
    rows, n = pred.shape
    loss = torch.full((), float("nan"), dtype=torch.float32, device=pred.device)
    grad = torch.full_like(pred, float("nan"))
    _lib.check(_lib.lib.ultra_query_loss(pred.data_ptr(), target.data_ptr(), rows, n, float(temperature), work.data_ptr(),
                                         loss.data_ptr(), grad.data_ptr(), _lib.stream_of(pred)))
    return loss, grad


def _row_order_mean(row_loss):
    """sum(row_loss) / rows accumulated in fp32 in row order, as the last workgroup does."""
    s = np.float32(0)
    for v in row_loss.cpu().numpy():
        s = np.float32(s + v)
    return np.float32(s / np.float32(len(row_loss)))


@pytest.mark.parametrize("temperature", QUERY_TEMPERATURES)
@pytest.mark.parametrize("kind", QUERY_TARGETS)
@pytest.mark.parametrize("rows,n", QUERY_SHAPES)
def test_query_loss_kernel_element_by_element(dev, rows, n, kind, temperature):
    """One workgroup of 256 threads per row: rows of 1, 2, 255, 256, 257 and 1000 columns (threads without an element, one each,
    several each), up to 1200 workgroups; one positive, about 1 % and about half positives per row, a row without a positive
    and a row of positives only.  The loss is, bit for bit, the row losses of the workspace summed in row order."""
    logits, truth = query_case(rows, n, kind)
    where = "query_loss (%d, %d) T=%g %s" % (rows, n, temperature, kind)
    p64 = logits.double().requires_grad_()
    want = query_loss_reference(p64, truth.double(), temperature)
    want.backward()
    scale = weight_scale(query_weights(logits.double(), truth, temperature), rows)
    pred, target = logits.to(dev), truth.to(dev)
    p32 = pred.clone().requires_grad_()
    plain = query_loss_reference(p32, target.float(), temperature)
    plain.backward()
    p = pred.clone().requires_grad_()
    got = query_train.query_loss(p, target, temperature)
    got.backward()
    got64, plain64 = p.grad.double().cpu(), p32.grad.double().cpu()
    _record("query_loss", temperature, got64, plain64, p64.grad, scale, where)
    _assert_elements(got64, plain64, p64.grad, scale, where)
    _assert_loss(got.item(), plain.item(), want.item(), where)
    # the same bits again, also through the entry; the counter is back at zero and the scalar is the row losses in row order
    work = torch.zeros(rows + 1, dtype=torch.float32, device=dev)
    loss, grad = _query_entry(pred, target.to(torch.uint8), temperature, work)
    assert torch.equal(loss, got.detach()) and torch.equal(grad, p.grad), where
    assert int(work.view(torch.int32)[rows]) == 0
    assert loss.cpu().numpy().view(np.int32) == _row_order_mean(work[:rows]).view(np.int32), where
    p3 = pred.clone().requires_grad_()
    (query_train.query_loss(p3, target, temperature) * 3).backward()
    assert torch.equal(p3.grad, grad * 3), where


def test_query_loss_workspace_is_left_ready_for_the_next_call(dev):
    """The completion counter behind the row losses reads 0 after a call, so a second call on the same, not re-zeroed workspace
    gives the same bits, and a third one on other logits their answer, not the first one's."""
    rows, n = 257, 300
    logits, truth = query_case(rows, n, "percent")
    pred, target = logits.to(dev), truth.to(dev).to(torch.uint8)
    work = torch.zeros(rows + 1, dtype=torch.float32, device=dev)
    for temperature in (0.0, 0.2):
        first = _query_entry(pred, target, temperature, work)
        assert int(work.view(torch.int32)[rows]) == 0
        rows_first = work[:rows].clone()
        second = _query_entry(pred, target, temperature, work)
        assert int(work.view(torch.int32)[rows]) == 0
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and torch.equal(work[:rows], rows_first)
        other = (pred * 0.5 + 1.0).contiguous()
        third = _query_entry(other, target, temperature, work)
        fresh = _query_entry(other, target, temperature, torch.zeros(rows + 1, dtype=torch.float32, device=dev))
        assert int(work.view(torch.int32)[rows]) == 0
        assert torch.equal(third[0], fresh[0]) and torch.equal(third[1], fresh[1]) and not torch.equal(third[0], first[0])
        want = query_loss_reference(other.double(), target.double(), temperature)
        assert abs(third[0].item() - want.item()) <= 64 * EPS32 * abs(want.item())
        assert third[0].cpu().numpy().view(np.int32) == _row_order_mean(work[:rows]).view(np.int32)


def test_query_loss_entry_refuses_bad_arguments(dev):
    pred = torch.zeros(4, 4, device=dev)
    target = torch.zeros(4, 4, dtype=torch.uint8, device=dev)
    work, loss, grad = torch.zeros(5, device=dev), torch.zeros((), device=dev), torch.zeros(4, 4, device=dev)
    good = [pred.data_ptr(), target.data_ptr(), 4, 4, 0.0, work.data_ptr(), loss.data_ptr(), grad.data_ptr()]
    assert _lib.lib.ultra_query_loss(*good, _lib.stream_of(pred)) == _lib.ULTRA_OK
    for slot, bad in ((0, None), (1, None), (5, None), (6, None), (7, None), (2, 0), (3, 0), (2, -1)):
        args = list(good)
        args[slot] = bad
        assert _lib.lib.ultra_query_loss(*args, _lib.stream_of(pred)) == _lib.ULTRA_ERR_INVALID, (slot, bad)
    torch.cuda.synchronize()


# ---- C. strict_negative_kernel on chosen draws ----
@pytest.mark.parametrize("known", [0, 1])
@pytest.mark.parametrize("num_node", SAMPLER_NODES)
def test_strict_sampler_kernel_on_chosen_draws(dev, num_node, known):
    """Hand-built graphs (sampler_graph: first / last / missing key ranges, solid runs of known answers at either end, count == 1,
    a hub, positives that are known answers or no edge at all) and draws where a bisection goes wrong: 0, the largest fp32 below
    1, and j / count with both fp32 neighbours; 1, 255, 256, 257 and 700 draws per row (the 256 threads' stride).  The ids equal
    the brute-force restatement's, id for id, are valid, and come out the same twice.

    Rows without any valid id (count == 0) are not tested: the reference indexes out of range there (tasks.py:60-61), so there
    is nothing to compare with."""
    data, anchor, relation, positive = sampler_graph(num_node, known)
    gdata = data.to(dev)
    for n_draw in SAMPLER_DRAWS:
        rand = sampler_rand(data, anchor, relation, positive, known, n_draw)
        want = brute_strict_negatives(data, anchor, relation, positive, rand, known)
        got = tasks._strict_negatives_gpu(gdata, anchor.to(dev), relation.to(dev), positive.to(dev), n_draw, known, rand=rand)
        assert got.shape == (len(anchor), n_draw) and got.dtype == torch.long
        bad = (got.cpu() != want).nonzero()
        assert len(bad) == 0, "n_draw %d: row %s (anchor, relation, positive) = %s, draw %r: got %d, want %d" % (
            n_draw, bad[0].tolist(), (int(anchor[bad[0, 0]]), int(relation[bad[0, 0]]), int(positive[bad[0, 0]])),
            float(rand[bad[0, 0], bad[0, 1]]), int(got[bad[0, 0], bad[0, 1]]), int(want[bad[0, 0], bad[0, 1]]))
        for q in range(len(anchor)):
            assert set(got[q].tolist()) <= set(valid_ids(data, int(anchor[q]), int(relation[q]), int(positive[q]), known))
        again = tasks._strict_negatives_gpu(gdata, anchor.to(dev), relation.to(dev), positive.to(dev), n_draw, known, rand=rand)
        assert torch.equal(again, got)


# ---- D. the two hash filters of the easy edges ----
def _keep(route, data, h, t, r, typed):
    fn = dense.easy_edge_keep if route == "lds" else dense.easy_edge_keep_table
    return fn(data.edge_index, data.edge_type if typed else None, h, t, r, data.num_nodes, data.num_relations)


@pytest.mark.parametrize("typed", [True, False])
@pytest.mark.parametrize("route,log2_slots,shape", WRAP_TABLES)
def test_edge_filters_probe_across_the_end_of_the_table(dev, route, log2_slots, shape, typed):
    """wrap_case: 48 listed keys start in the table's last 8 slots, so the run of occupied slots goes on through slot 0.  Every
    listed triple and its inverse is dropped wherever the probing put it; unlisted edges whose slot lies inside that run, before
    and after the wrap, and unlisted edges on an empty slot are kept.  Both layouts of h / t / r; the same vector twice."""
    case = wrap_case(log2_slots, shape, typed)
    assert case["wraps"] and case["n_cluster"] >= 40 and case["n_before"] >= 40 and case["n_after"] >= 40
    if route == "table":
        assert _lib.lib.ultra_easy_edge_keep_table_workspace(shape[0] * shape[1]) == 8 << log2_slots
    data, batch, want = case["data"].to(dev), case["batch"].to(dev), case["keep"]
    model = models.EntityNBFNet(64, [64] * 2, remove_one_hop=not typed)
    assert torch.equal(model.easy_edge_mask(data, *batch.unbind(-1)).cpu(), want.bool())
    h, t, r = batch.unbind(-1)                                       # (columns of the contiguous (rows, cols, 3) batch)
    assert not h.is_contiguous()
    strided = _keep(route, data, h, t, r, typed)
    packed = _keep(route, data, h.contiguous(), t.contiguous(), r.contiguous(), typed)
    for got in (strided, packed):
        assert got is not None and got.dtype == torch.float32
        wrong = (got.cpu() != want).nonzero().flatten().tolist()
        assert not wrong, "%d edges differ, the first: edge %d, want %g" % (len(wrong), wrong[0], float(want[wrong[0]]))
    assert torch.equal(_keep(route, data, h, t, r, typed), strided)


@pytest.mark.parametrize("typed", [True, False])
def test_lds_edge_filter_at_its_declared_capacity(dev, typed):
    """4096 distinct triples with 8192 distinct keys -- the LDS table half full, as declared -- are served by the LDS route and
    give easy_edge_mask; one triple more is declined, not truncated.  The global table gives the same vector."""
    batch, data = capacity_case(4096, typed)
    data, batch = data.to(dev), batch.to(dev)
    h, t, r = batch.unbind(-1)
    model = models.EntityNBFNet(64, [64] * 2, remove_one_hop=not typed)
    want = model.easy_edge_mask(data, h, t, r)
    assert 0 < int((~want).sum()) < want.numel()
    got = _keep("lds", data, h, t, r, typed)
    assert got is not None and torch.equal(got.bool(), want) and torch.equal(got, want.float())
    assert torch.equal(_keep("lds", data, h, t, r, typed), got)
    assert torch.equal(_keep("table", data, h, t, r, typed), got)
    more, more_data = capacity_case(4097, typed)
    more, more_data = more.to(dev), more_data.to(dev)
    assert _keep("lds", more_data, *more.unbind(-1), typed) is None
    got = _keep("table", more_data, *more.unbind(-1), typed)
    assert torch.equal(got.bool(), model.easy_edge_mask(more_data, *more.unbind(-1)))
