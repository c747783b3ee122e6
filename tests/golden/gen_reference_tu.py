"""Record what the reference's own compiled rspmm.cpp TU (oracle/_ref, oracle/build_ref.py) returns, so that the tests that
pin the C oracle to it run wherever the repository is checked out, with or without the reference sources.

    python tests/golden/gen_reference_tu.py

Needs oracle/_ref and oracle/_build built (build() does that where the reference checkout exists).  Output (small, committed):

  reference_tu.pt.xz              a torch.save'd dict, xz-compressed (tests/helpers.py load_reference_tu):
                                  ops:         for every case of tests/test_oracle.py::test_c_oracle_matches_reference_tu, the
                                               SHA-256 of the operands the case regenerates (test_oracle.case_inputs), per
                                               (sum, mul) the SHA-256 of the TU's forward output -- the C oracle reproduces
                                               those bits, which is checked here before anything is written -- and the
                                               TU's backward gradients in full;
                                  empty_rows:  the TU's output of test_reference_empty_row_identities per sum;
                                  model_calls: for every checkpoint / batch of test_oracle_model.py, per rspmm call the oracle
                                               model makes with the TU as its kernel: shape, sum, mul and the values at
                                               helpers.sample_index(call number, numel)
  reference_tu_signatures.json    the TU module's rspmm_* exports and the first line of each docstring (its pybind11 signature)
"""
import io
import json
import lzma
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import build_ref, rspmm_oracle, ultra_oracle_model  # noqa: E402
from tests import helpers  # noqa: E402
from tests.test_oracle import CASES, case_inputs  # noqa: E402
from tests.test_oracle_model import MODELS, load_golden  # noqa: E402

BATCH_KEYS = ("t_batch", "h_batch", "neg_batch")


def gen_ops(ref):
    ops = {}
    for ci, case in enumerate(CASES):
        for dtype in (torch.float32, torch.float64):
            ei, et, w, rel, x, og = case_inputs(case, dtype)
            rec = dict(inputs=helpers.fingerprint(ei, et, w, rel, x, og), out={})
            for sum in ("add", "min", "max"):
                for mul in ("mul", "add"):
                    fwd = getattr(ref, "rspmm_%s_%s_forward_cpu" % (sum, mul))(ei, et, w, rel, x)
                    bwd = getattr(ref, "rspmm_%s_%s_backward_cpu" % (sum, mul))(ei, et, w, rel, x, fwd, og)
                    mine = rspmm_oracle.rspmm_forward(ei, et, w, rel, x, sum=sum, mul=mul)
                    assert torch.equal(mine, fwd), "case %d %s %s %s: the C oracle's forward is not the TU's bits" % (
                        ci, sum, mul, dtype)
                    rec["out"][(sum, mul)] = dict(forward=helpers.fingerprint(fwd), backward=tuple(b.clone() for b in bwd))
            ops[(ci, str(dtype).split(".")[-1])] = rec
    return ops


def gen_empty_rows(ref):
    ei, et, w = torch.tensor([[0, 0], [1, 2]]), torch.tensor([0, 0]), torch.ones(2)
    rel, x = torch.ones(1, 4), torch.arange(12.).view(3, 4)
    return {sum: getattr(ref, "rspmm_%s_mul_forward_cpu" % sum)(ei, et, w, rel, x) for sum in ("add", "min", "max")}


def gen_model_calls():
    tu = ultra_oracle_model.reference_rspmm_fn()
    out = {}
    for ckpt, aggr in MODELS:
        g, state, data, cfg = load_golden(ckpt, aggr)
        for key in BATCH_KEYS:
            calls = []

            def fn(*args, **kwargs):
                res = tu(*args, **kwargs)
                idx = helpers.sample_index(len(calls), res.numel())
                calls.append(dict(shape=tuple(res.shape), sum=kwargs.get("sum", "add"), mul=kwargs.get("mul", "mul"),
                                  value=res.reshape(-1)[idx].clone()))
                return res
            ultra_oracle_model.ultra_forward(state, cfg, data, g[key], rspmm_fn=fn)
            out[(ckpt, aggr, key)] = calls
            print(ckpt, aggr, key, "%d rspmm calls" % len(calls))
    return out


def gen_signatures(ref):
    return {n: getattr(ref, n).__doc__.splitlines()[0] for n in sorted(dir(ref)) if n.startswith("rspmm_")}


if __name__ == "__main__":
    assert build_ref.available(), "oracle/_ref is not built: run build() where the reference checkout exists"
    ref = build_ref.load()
    buf = io.BytesIO()
    torch.save(dict(ops=gen_ops(ref), empty_rows=gen_empty_rows(ref), model_calls=gen_model_calls()), buf)
    with open(helpers.REFERENCE_TU, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    with open(os.path.join(HERE, "reference_tu_signatures.json"), "w") as f:
        json.dump(gen_signatures(ref), f, indent=1)
        f.write("\n")
