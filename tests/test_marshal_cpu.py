"""The Python side's operand marshalling, where no kernel runs: the layer update's arguments (_lib.update_args) against the
flag bits of include/ultra_nbfnet.h, and the point boundary as the entry points take it (rspmm._point_operand) -- on CPU
tensors, of which as_mat reads pointers and strides only."""
import itertools
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_flags():
    text = open(os.path.join(ROOT, "include", "ultra_nbfnet.h")).read()
    return {name: int(value) for name, value in re.findall(r"#define ULTRA_((?:CONV|LAYER0)_[A-Z_]+)\s+(\d+)", text)}


def test_update_args_match_the_header():
    from ultra_amd import _lib, dense
    bits = header_flags()
    assert sorted(bits) == ["CONV_LAYER_NORM", "CONV_RELU", "CONV_RESIDUAL", "LAYER0_MAX", "LAYER0_ONLY_FILL", "LAYER0_SKIP_FILL"]
    for name, value in bits.items():
        assert getattr(_lib, name) == value
    assert (dense.CONV_LAYER_NORM, dense.CONV_RELU, dense.CONV_RESIDUAL) == (1, 2, 4)
    linear, bare = nn.Linear(128, 64), nn.Linear(128, 64, bias=False)
    norm = nn.LayerNorm(64, eps=3e-4)
    for with_norm, relu, residual in itertools.product((False, True), repeat=3):
        ln = norm if with_norm else None
        weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(linear, ln, relu, residual)
        assert weight is linear.weight and bias is linear.bias
        assert flags == (bits["CONV_LAYER_NORM"] * with_norm | bits["CONV_RELU"] * relu | bits["CONV_RESIDUAL"] * residual)
        if with_norm:
            assert ln_weight is norm.weight and ln_bias is norm.bias and eps == 3e-4
        else:
            assert ln_weight is None and ln_bias is None and eps == 1e-5
        assert type(eps) is float and type(flags) is int
    assert _lib.update_args(bare, None, True)[:4] == (bare.weight, None, None, None)
    flags = _lib.update_args(linear, norm, True, extra_flags=_lib.LAYER0_MAX | _lib.LAYER0_SKIP_FILL)[5]
    assert flags == bits["CONV_LAYER_NORM"] | bits["CONV_RELU"] | bits["LAYER0_MAX"] | bits["LAYER0_SKIP_FILL"]
    assert _lib.update_args(linear, None, False, extra_flags=_lib.LAYER0_ONLY_FILL)[5] == bits["LAYER0_ONLY_FILL"]


def test_layer_hands_its_own_update():
    from ultra_amd import _lib
    from ultra_amd.layers import GeneralizedRelationalConv
    layer = GeneralizedRelationalConv(64, 64, 4, 64, "distmult", "sum", True, "relu")
    assert layer.update_args(True) == _lib.update_args(layer.linear, layer.layer_norm, True, True)
    plain = GeneralizedRelationalConv(64, 64, 4, 64, "distmult", "sum", False, None)
    assert plain.update_args() == (plain.linear.weight, plain.linear.bias, None, None, 1e-5, 0)


def test_point_operand():
    from ultra_amd import rspmm
    vals = torch.arange(3 * 64, dtype=torch.float32).view(3, 64)
    rows, held, rows_ptr, ref = rspmm._point_operand((torch.tensor([4, 0, 2], dtype=torch.int32), vals), torch.empty(3, 5, 64))
    mat = ref._obj
    assert rows.dtype == torch.int64 and rows.tolist() == [4, 0, 2] and rows_ptr == rows.data_ptr()
    assert (mat.n_outer, mat.n_row, mat.row_len) == (3, 1, 64)
    assert (mat.ptr, mat.stride_outer) == (vals.data_ptr(), 64) and held.data_ptr() == vals.data_ptr()      # (no copy)
    rows, held, rows_ptr, ref = rspmm._point_operand((torch.tensor([1]), vals[:1]), torch.empty(5, 64))
    mat = ref._obj
    assert (mat.n_outer, mat.n_row, mat.row_len, mat.ptr) == (1, 1, 64, vals.data_ptr()) and rows_ptr == rows.data_ptr()
    with pytest.raises(RuntimeError, match=r"Expected one boundary row per outer slice \(3\), got 2"):
        rspmm._point_operand((torch.tensor([4, 0]), vals), torch.empty(3, 5, 64))
