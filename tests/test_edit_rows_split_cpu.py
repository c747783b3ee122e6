"""ultra_rspmm_edit_rows_split (csrc/delta_kernels.hip), the parts that need no GPU: the symbol and its declaration,
the argument checks it shares with the other edit-row entries, Plan.edit_rows_split on host tensors, and the LONG-ROW graph of
tests/test_edit_rows_split_gpu.py -- one hub of 3 * HUB_TILE + 5 base edges whose named slots sit at the tile edges of the hub
walker -- with every property its cases promise asserted on GraphDelta's arrays and the documented merge order restated in plain
Python against the CPU oracle on the materialised list.

The graph: 400 nodes, 6 relations (3 direct).  Row HUB holds the slots 0 .. 3 * HUB_TILE + 4 in edge order, columns ascending from
10; the slots HUB_TILE - 2 .. HUB_TILE + 2 share ONE column (a run that straddles the first tile edge) with types 0, 1, 2, 3, 1 --
slot HUB_TILE - 1 and slot HUB_TILE + 2 are the same (col, type) stated twice -- and slots 40 and 41 are another duplicate.  Row
HUB_B holds 2 * HUB_TILE + 3 slots (the second hub of the capture test).  Rows 0 .. 9 share 60 ordinary edges; no other edge
points into a column below 10 or above 380."""
import ctypes
import os
import re
from collections import namedtuple

import pytest
import torch

from oracle import rspmm_oracle
from tests import test_edit_rows_shapes_cpu as shapes
from ultra_amd import _lib, rspmm
from ultra_amd.data import Data

TILE = _lib.HUB_TILE
N, R = 400, shapes.R
HUB, HUB_B = 390, 391
HUB_LEN, HUB_B_LEN = 3 * TILE + 5, 2 * TILE + 3
RUN = list(range(TILE - 2, TILE + 3))                         # the slots of the straddling column
RUN_TYPES = [0, 1, 2, 3, 1]
DUP = (40, 41)
CAPACITY = 1024


def _hub_row(row, length, seed):
    g = torch.Generator().manual_seed(seed)
    kinds = torch.randint(0, R, (length,), generator=g).tolist()
    cols, col = [], 10
    for slot in range(length):
        cols.append(col)
        if not (row == HUB and (slot in RUN[:-1] or slot == DUP[0])):
            col += 1
    if row == HUB:
        for slot, kind in zip(RUN, RUN_TYPES):
            kinds[slot] = kind
        kinds[DUP[1]] = kinds[DUP[0]]
    return [(row, c, k) for c, k in zip(cols, kinds)]


def _edges():
    g = torch.Generator().manual_seed(17)
    rows = torch.randint(0, 10, (60,), generator=g).tolist()
    cols = torch.randint(10, 380, (60,), generator=g).tolist()
    kinds = torch.randint(0, R, (60,), generator=g).tolist()
    return list(zip(rows, cols, kinds)) + _hub_row(HUB, HUB_LEN, 5) + _hub_row(HUB_B, HUB_B_LEN, 6)


EDGES = _edges()
BASE_SET = set(EDGES)
BASE_ROWS = {row: [(col, kind) for r, col, kind in sorted(EDGES, key=lambda e: e[1]) if r == row] for row in range(N)}
RUN_COL = BASE_ROWS[HUB][TILE][0]
LAST_COL = BASE_ROWS[HUB][-1][0]


def base_graph():
    row, col, kind = (torch.tensor(v) for v in zip(*EDGES))
    return Data(edge_index=torch.stack([row, col]), edge_type=kind, num_nodes=N, num_relations=R)


def slot(row, pos):
    return (row,) + BASE_ROWS[row][pos]


ADD_BELOW, ADD_EQUAL, ADD_ABOVE = (HUB, 1, 4), (HUB, RUN_COL, 5), (HUB, 399, 2)
ADDED = [ADD_BELOW, ADD_EQUAL, ADD_ABOVE]
Case = namedtuple("Case", "added dead survivors")     # dead: base slots of HUB; survivors: HUB's edges in materialize()
_EDGE_SLOTS = [0, TILE - 1, TILE, 2 * TILE - 1, HUB_LEN - 1]
CASES = {
    # slot TILE - 1 takes its duplicate at slot TILE + 2 along
    "slots_at_tile_edges": Case([], _EDGE_SLOTS, HUB_LEN - 6),
    # ... and slot TILE + 2 its duplicate at slot TILE - 1
    "a_whole_tile_dead": Case([], list(range(TILE, 2 * TILE)), HUB_LEN - TILE - 1),
    "all_dead_delta_left": Case(ADDED, list(range(HUB_LEN)), 3),
    "all_dead_none_left": Case([], list(range(HUB_LEN)), 0),
    "three_added": Case(ADDED, [], HUB_LEN + 3),
    "added_and_dead": Case(ADDED, _EDGE_SLOTS + [DUP[0]], HUB_LEN - 8 + 3),
}
_QUIET = (3, 381, 0)                                  # a key that names no edge of a touched row
# per-slice keys, five slices: a base edge AT a tile edge by its type; the same column by any type (the whole run and the added
# edge of that column go); a delta edge by its type and another by any type; the slot ahead of the second tile edge by any type;
# nothing
KEYS = [
    [slot(HUB, TILE), ADD_ABOVE],
    [(HUB, RUN_COL, -1), _QUIET],
    [ADD_EQUAL, ADD_BELOW[:2] + (-1,)],
    [slot(HUB, 2 * TILE - 1)[:2] + (-1,), slot(HUB, 2 * TILE)],
    [_QUIET, _QUIET],
]


def apply_case(data, case, row=HUB):
    delta = rspmm.GraphDelta(data, capacity=CAPACITY)
    if case.added:
        delta.add(*zip(*[shapes.fact(*edge) for edge in case.added]))
    gone = sorted({shapes.fact(*slot(row, pos)) for pos in case.dead})
    if gone:
        delta.remove(*zip(*gone))
    return delta


@pytest.fixture(scope="module")
def data():
    return base_graph()


# ---- the entry ----
def test_the_symbol_is_exported_and_declared():
    lib = _lib.lib
    assert hasattr(lib, "ultra_rspmm_edit_rows_split") and hasattr(lib, "ultra_rspmm_hub_tile")
    assert lib.ultra_abi_version() == 7
    assert TILE == lib.ultra_rspmm_hub_tile() and TILE >= 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ultra_rspmm.h")).read()
    found = re.search(r"int32_t ultra_rspmm_edit_rows_split\(([^;]*)\);", header)
    assert found, "the header declares the entry"
    args = [" ".join(a.split()) for a in found.group(1).split(",")]
    assert args == ["ultra_plan *plan", "int32_t sum", "int32_t mul", "int32_t dtype", "const ultra_mat *relation",
                    "const ultra_mat *input", "const ultra_mat *boundary", "const int64_t *point_rows_dev",
                    "const ultra_mat *output", "const ultra_delta *delta", "const ultra_tombstones *removed",
                    "const ultra_sample_keys *keys", "int64_t hub_len", "void *stream"]
    assert rspmm.EDIT_ROWS_HUB_SPLIT is True


def test_the_entry_validates_on_the_host(data):
    """The checks are those of the other edit-row entries, before anything is launched (host tensors here)."""
    lib = _lib.lib
    delta = apply_case(data, CASES["added_and_dead"])
    exact = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=True)
    loose = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=False)
    x, rel, out = torch.zeros(2, N, 64), torch.zeros(2, R, 64), torch.zeros(2, N, 64)
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, out)]
    operand, removed = ctypes.byref(delta.operand()), ctypes.byref(delta.removed_operand())
    key = torch.zeros(2, 2, dtype=torch.int32)
    good_keys = ctypes.byref(_lib.UltraSampleKeys(key.data_ptr(), key.data_ptr(), key.data_ptr(), 2))

    def call(plan=exact, sum=0, mul=0, dtype=_lib.F32, relation=mats[0], input=mats[1], boundary=None, rows=None, output=mats[2],
             operand=operand, removed=removed, keys=None, hub_len=-1):
        return lib.ultra_rspmm_edit_rows_split(plan._h if plan is not None else None, sum, mul, dtype, relation, input, boundary,
                                               rows, output, operand, removed, keys, hub_len, None)

    def invalid(**kw):
        return call(**kw) == _lib.ULTRA_ERR_INVALID and b"ultra_rspmm_edit_rows_split: " in lib.ultra_last_error()

    assert invalid(plan=None) and invalid(sum=3) and invalid(mul=5) and invalid(dtype=7)
    assert invalid(output=None) and invalid(operand=None) and invalid(relation=None) and invalid(input=None)
    assert invalid(rows=torch.zeros(2, dtype=torch.long).data_ptr())                              # point rows without values
    tombs, rows = delta.removed_operand(), delta.operand()
    for bad in (_lib.UltraTombstones(None, tombs.col_dev, tombs.type_dev, tombs.capacity_keys),
                _lib.UltraTombstones(tombs.ptr_dev, tombs.col_dev, tombs.type_dev, -1),
                _lib.UltraTombstones(tombs.ptr_dev, tombs.col_dev, tombs.type_dev, 1 << 30)):
        assert invalid(removed=ctypes.byref(bad)) and b"removed" in lib.ultra_last_error()
    for capacity in (-1, 1 << 30):
        bad = _lib.UltraDelta(rows.row_dev, rows.ptr_dev, rows.col_dev, rows.type_dev, rows.count_dev, capacity, rows.capacity_edges)
        assert invalid(operand=ctypes.byref(bad)) and b"capacities" in lib.ultra_last_error()
    for per_sample in (0, 9):
        bad = _lib.UltraSampleKeys(key.data_ptr(), key.data_ptr(), key.data_ptr(), per_sample)
        assert invalid(keys=ctypes.byref(bad), plan=None) and b"per_sample" in lib.ultra_last_error()
    assert invalid(keys=ctypes.byref(_lib.UltraSampleKeys(None, key.data_ptr(), key.data_ptr(), 2))) and b"keys" in lib.ultra_last_error()
    assert invalid(keys=good_keys, plan=None)
    for hub_len in (-1, 0, 16, 1 << 40):
        assert call(plan=loose, hub_len=hub_len) == _lib.ULTRA_ERR_UNSUPPORTED
        assert call(mul=_lib.MUL_CODES["rotate"], hub_len=hub_len) == _lib.ULTRA_ERR_UNSUPPORTED
    odd = [ctypes.byref(rspmm.as_mat(torch.zeros(2, n, 6))[1]) for n in (R, N, N)]
    assert call(relation=odd[0], input=odd[1], output=odd[2]) == _lib.ULTRA_ERR_UNSUPPORTED
    assert call(removed=None, keys=good_keys, plan=loose) == _lib.ULTRA_ERR_UNSUPPORTED
    empty = ctypes.byref(rspmm.UltraMat(out.data_ptr(), 0, 0, N, 64, 64))
    assert call(output=empty) == _lib.ULTRA_OK                                                    # n_outer == 0
    assert call(operand=ctypes.byref(_lib.UltraDelta(None, None, None, None, None, 0, 0))) == _lib.ULTRA_OK
    assert lib.ultra_abi_version() == 7


def test_the_plan_method_refuses_host_tensors_the_way_edit_rows_does(data):
    delta = apply_case(data, CASES["added_and_dead"])
    exact = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=True)
    loose = rspmm.Plan(data.edge_index, data.edge_type, N, R, exact_order=False)
    x, rel, out = torch.zeros(2, N, 64), torch.zeros(2, R, 64), torch.zeros(2, N, 64)
    assert loose.edit_rows(rel, x, out, delta) is None and loose.edit_rows_split(rel, x, out, delta) is None
    messages = []
    for method in (exact.edit_rows, exact.edit_rows_split):
        with pytest.raises(RuntimeError, match="expected a GPU") as caught:
            method(rel, x, out, delta)
        messages.append(str(caught.value))
    assert messages[0] == messages[1]
    assert exact.has_hub_rows and not loose.has_hub_rows           # the hubs exceed the default seg_len
    assert 16 < HUB_B_LEN <= exact.info()["seg_len"] < HUB_LEN      # HUB is a hub at the default hub_len, HUB_B below 16


# ---- the long-row graph ----
def test_the_long_row_graph_is_what_the_cases_rely_on(data):
    degree = torch.bincount(data.edge_index[0], minlength=N)
    assert int(degree[HUB]) == HUB_LEN == 3 * TILE + 5 and int(degree[HUB_B]) == HUB_B_LEN
    assert int(degree.sort().values[-3]) <= 16                    # every other row is short
    for row in (HUB, HUB_B):
        cols = [col for col, _ in BASE_ROWS[row]]
        assert cols == sorted(cols) and cols[0] == 10 and cols[-1] < 380
        # edge order is slot order: the plan's (row, col, edge id) order keeps the slots where they were written
        assert [e[1:] for e in EDGES if e[0] == row] == BASE_ROWS[row]
    hub = BASE_ROWS[HUB]
    assert [hub[s] for s in RUN] == [(RUN_COL, kind) for kind in RUN_TYPES]
    assert hub[RUN[0] - 1][0] < RUN_COL < hub[RUN[-1] + 1][0] and RUN[0] < TILE <= RUN[-1]      # the run straddles the tile edge
    assert hub[TILE - 1] == hub[TILE + 2] and hub[DUP[0]] == hub[DUP[1]]                        # duplicate (col, type) edges
    assert len(set(hub)) == HUB_LEN - 2
    assert ADD_BELOW[1] < hub[0][0] and ADD_EQUAL[1] == RUN_COL and ADD_ABOVE[1] > LAST_COL
    assert all(edge not in BASE_SET for edge in ADDED) and ADD_EQUAL[2] not in RUN_TYPES


@pytest.mark.parametrize("name", list(CASES))
def test_the_long_row_case_is_what_its_name_says(data, name):
    case = CASES[name]
    delta = apply_case(data, case)
    count = int(delta.count)
    touched = delta.rows[:count].tolist()
    assert HUB in touched and len(delta) == len(case.added)
    k = touched.index(HUB)
    ptr, dead_ptr = delta.ptr[:count + 1].tolist(), delta.dead_ptr[:count + 1].tolist()
    extra = list(zip(delta.col[ptr[k]:ptr[k + 1]].tolist(), delta.type[ptr[k]:ptr[k + 1]].tolist()))
    assert extra == sorted(edge[1:] for edge in case.added)
    held = set(zip(delta.dead_col[dead_ptr[k]:dead_ptr[k + 1]].tolist(), delta.dead_type[dead_ptr[k]:dead_ptr[k + 1]].tolist()))
    dead_slots = [p for p, pair in enumerate(BASE_ROWS[HUB]) if pair in held]
    assert set(case.dead) <= set(dead_slots) and held == {BASE_ROWS[HUB][p] for p in case.dead}
    mat = delta.materialize()
    assert int((mat.edge_index[0] == HUB).sum()) == case.survivors == HUB_LEN - len(dead_slots) + len(case.added)
    if name == "slots_at_tile_edges":
        assert dead_slots == sorted(case.dead + [TILE + 2])
    if name == "a_whole_tile_dead":
        assert dead_slots == list(range(TILE - 1, 2 * TILE))


def test_the_keys_name_what_they_say():
    assert len(KEYS) == 5 and all(len(keys) == 2 for keys in KEYS)
    assert KEYS[0][0] == slot(HUB, TILE) and KEYS[0][0] in BASE_SET and KEYS[0][1] in ADDED
    hub_edges = [(HUB,) + pair for pair in BASE_ROWS[HUB]] + ADDED
    assert sum(shapes.key_hits(edge, KEYS[1]) for edge in hub_edges) == len(RUN) + 1               # the run and the added edge
    assert [edge for edge in hub_edges if shapes.key_hits(edge, KEYS[2])] == [ADD_BELOW, ADD_EQUAL]
    assert [edge for edge in hub_edges if shapes.key_hits(edge, KEYS[3])] == [slot(HUB, 2 * TILE - 1), slot(HUB, 2 * TILE)]
    assert not any(shapes.key_hits(edge, KEYS[4]) for edge in hub_edges)


def merged_rows(delta, rel, x, bnd, sum, mul):
    """tests/test_edit_rows_shapes_cpu.merged_rows on THIS module's base rows: the documented stream of ultra_rspmm_edit_rows_split
    -- live base edges merged with the delta's edges by column, base first on ties, base edges of one column in plan order --
    reduced one after the other from the start value, the boundary last."""
    count = int(delta.count)
    rows, ptr, dead_ptr = delta.rows[:count].tolist(), delta.ptr[:count + 1].tolist(), delta.dead_ptr[:count + 1].tolist()
    col, kind, dead_col, dead_type = (t.tolist() for t in (delta.col, delta.type, delta.dead_col, delta.dead_type))
    out = {}
    for k, row in enumerate(rows):
        dead = set(zip(dead_col[dead_ptr[k]:dead_ptr[k + 1]], dead_type[dead_ptr[k]:dead_ptr[k + 1]]))
        base = [pair for pair in BASE_ROWS[row] if pair not in dead]
        extra = list(zip(col[ptr[k]:ptr[k + 1]], kind[ptr[k]:ptr[k + 1]]))
        merged = []
        while base or extra:
            merged.append(base.pop(0) if base and (not extra or base[0][0] <= extra[0][0]) else extra.pop(0))
        acc = torch.full((x.shape[1],), shapes.start_value(sum, x.dtype), dtype=x.dtype)
        for c, t in merged:
            acc = shapes.reduce_step(sum, acc, rel[t] * x[c] if mul == "mul" else rel[t] + x[c])
        out[row] = acc if bnd is None else shapes.reduce_step(sum, acc, bnd[row])
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("sum,mul", [("add", "mul"), ("max", "add"), ("min", "mul")])
def test_the_documented_order_equals_the_oracle_on_the_long_row(data, sum, mul, dtype):
    g = torch.Generator().manual_seed(11)
    x, rel, bnd = (torch.randn(n, 8, generator=g, dtype=dtype) for n in (N, R, N))
    for name, case in CASES.items():
        delta = apply_case(data, case)
        mat = delta.materialize()
        plain = rspmm_oracle.generalized_rspmm(mat.edge_index, mat.edge_type, torch.ones(mat.edge_index.shape[1], dtype=dtype),
                                               rel, x, sum=sum, mul=mul)
        for boundary in (None, bnd):
            want = plain if boundary is None else shapes.reduce_step(sum, plain, boundary)
            got = merged_rows(delta, rel, x, boundary, sum, mul)
            assert sorted(got) == delta.rows[:int(delta.count)].tolist(), name
            for row, value in got.items():
                assert torch.equal(value, want[row]), (name, row, boundary is not None)
