"""Serving answer sets, the parts that need no GPU: the plain-torch restatement (predict.filtered_above_reference) against a
brute-force Python sort, logit_threshold, the C entry point's argument checks, and QueryPredictor.answer_sets on the stub
projections of tests/test_query_exec_cpu.py against `answers`."""
import ctypes
import math
import os
import re
import struct
import types

import pytest
import torch

from tests.test_predict_cpu import SPECIAL_ROW, random_known, special_mix
from tests.test_query_exec_cpu import load, stub_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def fp32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def brute_force_above(row, threshold, known=()):
    """(size, ids) of one row (a list of Python floats holding fp32 values): membership by the strict comparison with the
    fp32 threshold (Python floats compare exactly; a NaN is above nothing), then an explicit sort key: the value descending
    (-0.0 == 0.0 as Python floats), then the id."""
    threshold = fp32(threshold)
    members = [i for i in range(len(row)) if row[i] > threshold]
    known = set(int(i) for i in known)
    kept = sorted((i for i in members if i not in known), key=lambda i: (-row[i], i))
    return len(members), kept


def check_against_brute_force(pred, threshold, ptr, index):
    from ultra_amd import predict
    out_ptr, ids, scores, size = predict.filtered_above_reference(pred, threshold, ptr, index)
    batch = pred.shape[0]
    assert out_ptr.shape == (batch + 1,) and size.shape == (batch,) and ids.shape == scores.shape == (int(out_ptr[-1]),)
    assert out_ptr.dtype == ids.dtype == size.dtype == torch.long and scores.dtype == pred.dtype
    assert int(out_ptr[0]) == 0
    for b in range(batch):
        known = [] if ptr is None else index[int(ptr[b]):int(ptr[b + 1])].tolist()
        want_size, want = brute_force_above(pred[b].tolist(), threshold, known)
        lo, hi = int(out_ptr[b]), int(out_ptr[b + 1])
        assert int(size[b]) == want_size
        assert ids[lo:hi].tolist() == want
        assert torch.equal(scores[lo:hi].view(torch.int32), pred[b, want].view(torch.int32))      # the stored bits
    return out_ptr, ids, scores, size


def test_restatement_on_the_special_value_row():
    from ultra_amd import predict
    pred = torch.tensor([SPECIAL_ROW])      # [0., -0., nan, inf, 1., 1., -inf, nan, -1., 0.]
    # -inf: everything except -inf and NaN; -0.0 == +0.0, ties by id; -0.0 comes back as -0.0
    out_ptr, ids, scores, size = check_against_brute_force(pred, -INF, None, None)
    assert ids.tolist() == [3, 4, 5, 0, 1, 9, 8] and size.tolist() == [7] and out_ptr.tolist() == [0, 7]
    assert math.copysign(1.0, float(scores[4])) == -1.0
    # strict: a threshold equal to a stored score leaves that score out; +-0 are not above 0.0 nor above -0.0
    for threshold, want in ((0.0, [3, 4, 5]), (-0.0, [3, 4, 5]), (1.0, [3]), (-1.0, [3, 4, 5, 0, 1, 9]), (0.5, [3, 4, 5]),
                            (3e38, [3]), (-3e38, [3, 4, 5, 0, 1, 9, 8])):
        out_ptr, ids, _, size = check_against_brute_force(pred, threshold, None, None)
        assert ids.tolist() == want and size.tolist() == [len(want)]
    # a filtered member is removed, and still counted by size
    out_ptr, ids, _, size = check_against_brute_force(pred, -1.0, torch.tensor([0, 3]), torch.tensor([2, 3, 9]))
    assert ids.tolist() == [4, 5, 0, 1] and size.tolist() == [6]
    # everything known: an empty list, the size unchanged
    out_ptr, ids, scores, size = check_against_brute_force(pred, -INF, torch.tensor([0, 10]), torch.arange(10))
    assert ids.numel() == 0 and scores.numel() == 0 and out_ptr.tolist() == [0, 0] and size.tolist() == [7]
    # an empty result
    row = torch.tensor([[0.5, -1.0, float("nan"), -INF]])
    out_ptr, ids, _, size = check_against_brute_force(row, 0.5, None, None)
    assert ids.numel() == 0 and out_ptr.tolist() == [0, 0] and size.tolist() == [0]
    # the threshold is rounded to fp32 first: 0.1 (fp64) lies below fp32(0.1), which a stored fp32 0.1 does not exceed
    tenth = torch.tensor([[0.1]])
    assert predict.filtered_above_reference(tenth, 0.1)[3].tolist() == [0]
    assert predict.filtered_above_reference(tenth, 0.0999999)[3].tolist() == [1]


def test_restatement_on_random_rows_with_ties_and_special_values():
    gen = torch.Generator().manual_seed(20250101)
    rows = 0
    for case in range(50):
        n = int(torch.randint(1, 70, (1,), generator=gen))
        pred = special_mix((4, n), gen)
        pred[torch.rand(4, n, generator=gen) < 0.05] = INF
        ptr, index = random_known(4, n, 0.3, gen)
        threshold = [-INF, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0][case % 8]       # most of them equal stored scores
        check_against_brute_force(pred, threshold, ptr, index)
        check_against_brute_force(pred, threshold, None, None)
        rows += 4
    assert rows == 200


def test_restatement_refuses_thresholds_without_a_meaning():
    from ultra_amd import predict
    pred = torch.zeros(1, 3)
    for bad in (float("nan"), INF, 1e39):       # (1e39 rounds to +inf in fp32)
        with pytest.raises(ValueError):
            predict.filtered_above_reference(pred, bad)
    with pytest.raises(TypeError):
        predict.filtered_above_reference(pred, "0.5")


def test_logit_threshold():
    from ultra_amd import predict
    zero = predict.logit_threshold(0.5)
    assert zero == 0.0 and math.copysign(1.0, zero) == 1.0
    ps = [1e-6, 0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 1 - 1e-6]
    values = [predict.logit_threshold(p) for p in ps]
    assert values == sorted(values) and len(set(values)) == len(values)
    for p, v in zip(ps, values):
        assert v == fp32(math.log(p / (1 - p)))         # fp64, rounded to fp32
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            predict.logit_threshold(bad)


def test_above_entry_point_checks_its_arguments_without_a_gpu():
    from ultra_amd import _lib
    lib = _lib.lib
    assert lib.ultra_abi_version() == 7
    host = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(host)
    big = 1 << 40

    def call(score=p, batch=1, n=100, threshold=0.0, out=p, capacity=big, ws=p, ws_bytes=big):
        return lib.ultra_filtered_above(score, None, None, batch, n, threshold, out, out, out, capacity, out, ws, ws_bytes, None)
    # n_cand >= 2^31, a NaN or +inf threshold: decided before any pointer is looked at
    assert call(score=None, out=None, ws=None, n=2 ** 31) == _lib.ULTRA_ERR_UNSUPPORTED
    assert call(score=None, out=None, ws=None, threshold=float("nan")) == _lib.ULTRA_ERR_UNSUPPORTED
    assert call(score=None, out=None, ws=None, threshold=INF) == _lib.ULTRA_ERR_UNSUPPORTED
    assert b"ultra_filtered_above" in lib.ultra_last_error()
    # NULL score or outputs (a finite and a -inf threshold are both fine), nothing launched
    for threshold in (0.0, -INF, 3e38):
        assert call(score=None, threshold=threshold) == _lib.ULTRA_ERR_INVALID
        assert call(out=None, threshold=threshold) == _lib.ULTRA_ERR_INVALID
    for name in ("ptr", "ids", "scores", "size"):
        args = dict(ptr=p, ids=p, scores=p, size=p)
        args[name] = None
        assert lib.ultra_filtered_above(p, None, None, 1, 100, 0.0, args["ptr"], args["ids"], args["scores"], big, args["size"],
                                        p, big, None) == _lib.ULTRA_ERR_INVALID, name
    # an empty candidate set, batch outside [0, 65535]
    assert call(n=0) == _lib.ULTRA_ERR_INVALID
    assert call(n=-1) == _lib.ULTRA_ERR_INVALID
    assert call(batch=-1) == _lib.ULTRA_ERR_INVALID
    assert call(batch=65536) == _lib.ULTRA_ERR_INVALID
    # capacity below batch * n_cand: decided on the host
    assert call(batch=3, n=100, capacity=299) == _lib.ULTRA_ERR_INVALID
    assert b"capacity" in lib.ultra_last_error()
    # a workspace that is too small
    need = lib.ultra_filtered_above_workspace(3, 100)
    assert need > 0
    assert call(batch=3, n=100, capacity=300, ws_bytes=need - 1) == _lib.ULTRA_ERR_INVALID
    assert b"workspace" in lib.ultra_last_error()
    assert call(batch=3, n=100, capacity=300, ws=None) == _lib.ULTRA_ERR_INVALID
    # batch 0
    assert call(batch=0, capacity=0) == _lib.ULTRA_OK


def test_above_workspace_query():
    from ultra_amd import _lib
    lib = _lib.lib
    c = _lib.TOPK_CHUNK
    ns = (1, 2, c - 1, c, c + 1, 2 * c + 3, 40 * c + 5, 2 * 10 ** 6)
    for batch in (0, 1, 3, 8, 65535):
        sizes = [lib.ultra_filtered_above_workspace(batch, n) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for n in ns:
        sizes = [lib.ultra_filtered_above_workspace(batch, n) for batch in (0, 1, 3, 8, 16, 65535)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # room for two key buffers of batch * n_cand keys
    assert lib.ultra_filtered_above_workspace(8, 2 * 10 ** 6) >= 2 * 8 * 2 * 10 ** 6 * 8
    assert lib.ultra_filtered_above_workspace(8, 2 * 10 ** 6) < 2 * 8 * 2 * 10 ** 6 * 8 + (1 << 20)
    assert lib.ultra_filtered_above_workspace(-1, 100) == -1
    assert lib.ultra_filtered_above_workspace(65536, 100) == -1
    assert lib.ultra_filtered_above_workspace(8, -1) == -1
    assert lib.ultra_filtered_above_workspace(8, 2 ** 31) == -1


def test_above_entry_points_bound_as_declared():
    from ultra_amd import _lib
    text = open(os.path.join(ROOT, "include", "ultra_nbfnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, kind in (("ultra_filtered_above", "int32_t"), ("ultra_filtered_above_workspace", "int64_t")):
        params = re.search(r"%s %s\((.*?)\);" % (kind, name), text, flags=re.S).group(1)
        assert len(getattr(_lib.lib, name).argtypes) == params.count(",") + 1, name
    assert _lib.lib.ultra_filtered_above_workspace.restype is ctypes.c_int64


def test_filtered_above_has_no_cpu_path_and_checks_its_arguments_first():
    from ultra_amd import predict
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict.filtered_above(torch.zeros(2, 5), 0.0)
    for bad in (float("nan"), INF):
        with pytest.raises(ValueError):
            predict.filtered_above(torch.zeros(2, 5), bad)
    with pytest.raises(TypeError):
        predict.filtered_above(torch.zeros(2, 5), None)


# ---- QueryPredictor.answer_sets on the stub projections ----

def stub_setting(logic="product"):
    g = load()
    graph = types.SimpleNamespace(num_nodes=g["num_nodes"], num_relations=g["num_relations"],
                                  edge_index=torch.zeros(2, 0, dtype=torch.long))
    order = torch.randperm(2 * len(g["nested"]), generator=torch.Generator().manual_seed(7)).tolist()
    nested = [g["nested"][i % len(g["nested"])] for i in order]        # two of every structure, mixed
    return g, graph, stub_model(logic), nested


@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("probability", [0.5, 0.6])
def test_answer_sets_come_in_input_order_and_agree_with_answers(filtered, probability):
    from ultra_amd import predict, query_exec, query_predict
    g, graph, model, nested = stub_setting()
    k = 7
    qp = query_predict.QueryPredictor(model, graph, k=k, batch_size=3, filtered=filtered)
    batches = qp.batches(nested)
    assert len(batches) > 1 and any(b != list(range(b[0], b[0] + len(b))) for b in batches)      # input order is not batch order
    ptr, ids, scores, size = qp.answer_sets(nested, probability=probability)
    threshold = predict.logit_threshold(probability)
    n = len(nested)
    assert ptr.shape == (n + 1,) and size.shape == (n,) and int(ptr[0]) == 0 and ids.shape == scores.shape == (int(ptr[-1]),)
    # the same batches straight from the executor, every row selected on its own
    lengths, seen = set(), []
    for index, program in qp._programs(nested):
        logits, sym = query_exec.execute(model, graph, program, symbolic_traversal=filtered)
        for row, i in enumerate(index):
            known = (sym[row] != 0).nonzero().flatten() if filtered else None
            want = predict.filtered_above_reference(logits[row:row + 1], threshold,
                                                    None if known is None else torch.tensor([0, len(known)]), known)
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            assert ids[lo:hi].tolist() == want[1].tolist(), i
            assert torch.equal(scores[lo:hi].view(torch.int32), want[2].view(torch.int32))
            assert int(size[i]) == int(want[3][0]) == int((logits[row] > threshold).sum())
            lengths.add(hi - lo)
            seen.append(i)
    assert sorted(seen) == list(range(n))
    assert len(lengths) > 1 and max(lengths) > k       # the sets differ in length and outgrow the best-k list
    # the first min(k, len) ids of a set are the ids of `answers` whose score exceeds the threshold
    top_ids, top_scores, count = qp.answers(nested)
    for i in range(n):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        above = [int(v) for v, s in zip(top_ids[i, :int(count[i])], top_scores[i, :int(count[i])]) if float(s) > threshold]
        assert ids[lo:hi][:k].tolist() == above, i
    assert not model.training


def test_answer_sets_of_no_query_and_bad_probabilities():
    from ultra_amd import query_predict
    g, graph, model, nested = stub_setting()
    qp = query_predict.QueryPredictor(model, graph, k=5, batch_size=3)
    ptr, ids, scores, size = qp.answer_sets([])
    assert ptr.tolist() == [0] and ids.numel() == scores.numel() == size.numel() == 0
    for bad in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError):
            qp.answer_sets(nested, probability=bad)
