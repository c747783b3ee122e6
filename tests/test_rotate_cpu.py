"""RotatE on the rspmm engine, the parts that need no GPU: the operator code, the ABI, the host-side refusal of odd rows, the
golden of the reference layer (tests/golden/gen_rotate_golden.py) and the unchanged unfused CPU layer against it."""
import ctypes
import io
import lzma
import os
import re

import torch

from ultra_amd import _lib, layers, rspmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rotate.pt.xz")


def load_golden():
    with lzma.open(GOLDEN, "rb") as f:
        return torch.load(io.BytesIO(f.read()))


def test_rotate_is_operator_code_2():
    assert _lib.MUL_CODES["rotate"] == 2
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    assert re.search(r"ULTRA_MUL_ROTATE\s*=\s*2\b", header)
    for s in ("Add", "Min", "Max"):
        assert hasattr(rspmm, "RSPMM%sRotateFunction" % s)


def test_abi_stays_7_and_every_declared_symbol_is_exported():
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.ultra_abi_version.restype = ctypes.c_int32
    assert lib.ultra_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "ultra_rspmm.h")).read()
    assert re.search(r"#define ULTRA_ABI_VERSION 7\b", header)
    assert not [n for n in declared_symbols() if not hasattr(lib, n)]
    # the reference exports no rotate functions: neither does the reference-shaped surface
    assert not hasattr(lib, "ultra_rspmm_add_rotate_forward_cuda")
    try:
        rspmm.rspmm.rspmm_add_rotate_forward_cuda
    except AttributeError:
        pass
    else:
        raise AssertionError("the reference-shaped namespace grew a rotate export")


def test_odd_rows_are_refused_on_the_host():
    """The row-length check of ULTRA_MUL_ROTATE runs before any HIP call: ULTRA_ERR_INVALID without a GPU."""
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    et = torch.tensor([0, 1, 0])
    plan = rspmm.Plan(ei, et, 3, 2)
    buf = torch.zeros(3, 5)
    mat = _lib.UltraMat(buf.data_ptr(), 1, 0, 3, 5, 5)
    ref = ctypes.byref(mat)
    rc = _lib.lib.ultra_rspmm_forward(plan._h, 0, _lib.MUL_CODES["rotate"], _lib.F32, None, ref, ref, None, ref, None)
    assert rc == _lib.ULTRA_ERR_INVALID and b"even" in _lib.lib.ultra_last_error()
    rc = _lib.lib.ultra_rspmm_backward(plan._h, 0, _lib.MUL_CODES["rotate"], _lib.F32, None, ref, ref, ref, ref, None, ref, ref, None)
    assert rc == _lib.ULTRA_ERR_INVALID and b"even" in _lib.lib.ultra_last_error()
    rc = _lib.lib.ultra_rspmm_forward(plan._h, 0, 3, _lib.F32, None, ref, ref, None, ref, None)
    assert rc == _lib.ULTRA_ERR_INVALID      # (the internal operator codes are not part of the ABI)


def test_golden_loads_and_its_flag_is_true():
    g = load_golden()
    assert g["sorted_scatter_is_sequential"] is True
    assert os.path.getsize(GOLDEN) < 1 << 20
    n = g["num_node"]
    indeg = torch.bincount(g["graph"]["sorted"]["edge_index"][1], minlength=n)
    assert indeg.max() > 256 and (indeg == 0).any() and g["num_relation"] >= 6
    a, b = g["graph"]["sorted"], g["graph"]["shuffled"]
    key = lambda q: sorted(zip(q["edge_index"][0].tolist(), q["edge_index"][1].tolist(), q["edge_type"].tolist()))
    assert key(a) == key(b) and len(set(key(a))) < len(key(a))          # the same multigraph, with duplicate edges
    t, s = a["edge_index"][1], a["edge_index"][0]
    assert ((t * n + s).diff() >= 0).all()
    for aggr in ("sum", "mean", "max", "min"):
        assert g[aggr]["sorted"]["out"].shape == g["x"].shape and g[aggr]["out64"].dtype == torch.float64


def test_cpu_layer_equals_the_reference_on_the_sorted_graph():
    """CPU tensors keep the unfused route (unchanged): its sum is the reference's scatter_add_, bit for bit."""
    g = load_golden()
    n = g["num_node"]
    e = g["graph"]["sorted"]
    for aggr in ("sum", "mean", "max", "min"):
        layer = layers.GeneralizedRelationalConv(64, 64, g["num_relation"], 64, "rotate", aggr, True, "relu")
        layer.load_state_dict(g["state"])
        assert not layer.rotate_fused(g["x"], g["state"]["relation.weight"])
        with torch.no_grad():
            got = layer(g["x"], g["query"], g["boundary"], e["edge_index"], e["edge_type"], (n, n))
        assert torch.equal(got, g[aggr]["sorted"]["out"]), aggr
