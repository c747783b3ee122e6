"""The shapes the edit-row kernels (csrc/delta_kernels.hip) must serve, the parts that need no GPU: a crafted base graph whose rows
put a dead edge at a chosen SORTED POSITION -- next to the 16-pair reload of the base cursor, next to the DELTA_BATCH = 8 boundary
of the gather -- a table of named edits on it, every property a name promises asserted on GraphDelta's arrays and on
materialize(), and the kernel's documented order (merge by column, base first on ties, tombstoned base edges left out, sequential
reduction from the start value, boundary last) restated in plain Python against the CPU oracle on the materialised list.
tests/test_edit_rows_shapes_gpu.py imports the graph, the cases and the key tables from here.

The graph: 128 nodes (a row of 100 DISTINCT columns needs more than 100), 6 relations (3 direct), 380 directed edges.  Rows
110 .. 120 are the special rows of base degree 0, 1, 7, 8, 9, 15, 16, 17, 18, 33 and 100: their columns are distinct, so "the
edge at sorted position p" is one edge, but for column 64 of the 18-row, which carries types 0, 1, 1 and 2.  Their columns lie in
8 .. 109: columns 0 and 1 sit below every special row, 121 .. 126 above, 127 is used by no base edge, and rows 2 .. 7 are ordinary
rows that no case touches.  Rows 0 .. 99 share the other edges, six of them stated twice."""
from collections import namedtuple

import pytest
import torch

from oracle import rspmm_oracle
from ultra_amd import rspmm
from ultra_amd.data import Data

N, R, R_DIRECT = 128, 6, 3
ROW_0, ROW_1, ROW_7, ROW_8, ROW_9, ROW_15, ROW_16, ROW_17, ROW_18, ROW_33, ROW_100 = range(110, 121)
DEGREES = {ROW_0: 0, ROW_1: 1, ROW_7: 7, ROW_8: 8, ROW_9: 9, ROW_15: 15, ROW_16: 16, ROW_17: 17, ROW_18: 18, ROW_33: 33,
           ROW_100: 100}
MULTI_ROW, MULTI_COL, MULTI_TYPES = ROW_18, 64, [0, 1, 1, 2]
UNUSED_COL = 127
QUIET_ROWS = range(2, 8)
CAPACITY = 64


def _edges():
    """(row, col, type) of the base graph, in edge order."""
    g = torch.Generator().manual_seed(41)
    pool = [c for c in range(8, 110) if c != MULTI_COL]
    edges = []
    for row, degree in DEGREES.items():
        distinct = degree - len(MULTI_TYPES) if row == MULTI_ROW else degree
        cols = sorted(pool[i] for i in torch.randperm(len(pool), generator=g)[:distinct].tolist())
        kinds = torch.randint(0, R, (distinct,), generator=g).tolist()
        edges += [(row, col, kind) for col, kind in zip(cols, kinds)]
        if row == MULTI_ROW:
            edges += [(row, MULTI_COL, kind) for kind in MULTI_TYPES]
    rows = torch.randint(0, 100, (150,), generator=g).tolist()
    cols = torch.randint(0, UNUSED_COL, (150,), generator=g).tolist()
    kinds = torch.randint(0, R, (150,), generator=g).tolist()
    edges += list(zip(rows, cols, kinds))
    edges += edges[-40:-34]                                   # six duplicates among the ordinary rows
    order = torch.randperm(len(edges), generator=g).tolist()
    return [edges[i] for i in order]


EDGES = _edges()
BASE_SET = set(EDGES)
# per row its (col, type) pairs in the plan's order: sorted by (col, edge id)
BASE_ROWS = {row: [(col, kind) for r, col, kind in sorted(EDGES, key=lambda e: e[1]) if r == row] for row in range(N)}


def base_graph():
    row, col, kind = (torch.tensor(v) for v in zip(*EDGES))
    return Data(edge_index=torch.stack([row, col]), edge_type=kind, num_nodes=N, num_relations=R)


def fact(row, col, kind):
    """The fact (h, r, t) that states the edge (row, col, kind) of the plan's direction (row = edge_index[0])."""
    return (row, kind, col) if kind < R_DIRECT else (col, kind - R_DIRECT, row)


def partner(row, col, kind):
    """The other edge of the same fact."""
    return (col, row, kind + R_DIRECT if kind < R_DIRECT else kind - R_DIRECT)


def edge_at(row, pos):
    return (row,) + BASE_ROWS[row][pos]


def other_type(row, pos):
    """An edge at the column of base position `pos` of `row`, of another type than the base edge there."""
    col, kind = BASE_ROWS[row][pos]
    return (row, col, (kind + 1) % R)


MULTI_DEAD = [p for p, (col, kind) in enumerate(BASE_ROWS[MULTI_ROW]) if col == MULTI_COL and kind == 1]
# one added edge per row of 7, 8 and 9 edges: below the first base column, AT a base column (the base edge goes first), above the last
ADD = {
    ROW_7: {"below": (ROW_7, 1, 4), "equal": other_type(ROW_7, 3), "above": (ROW_7, 121, 2)},
    ROW_8: {"below": (ROW_8, 0, 1), "equal": other_type(ROW_8, 7), "above": (ROW_8, 122, 5)},
    ROW_9: {"below": (ROW_9, 1, 0), "equal": other_type(ROW_9, 0), "above": (ROW_9, 123, 3)},
}
ADD_0 = [(ROW_0, 20, 1), (ROW_0, 11, 5), (ROW_0, 20, 3)]
ADD_1 = (ROW_1, 126, 0)
ADD_17 = other_type(ROW_17, 16)                               # a delta edge behind the 17-row's last base edge
ADD_100 = [(ROW_100, 0, 2), other_type(ROW_100, 80)]
ADD_16 = (ROW_16, 124, 1)                                     # above the 16-row's last column: the base cursor ends where a reload would begin
ADD_33 = [other_type(ROW_33, 15), other_type(ROW_33, 32)]     # equal columns on both sides of the second reload and at the last pair

# added: edges (row, col, type) in the plan's direction, each stated through its fact; dead: (row, sorted base positions);
# survivors: the number of edges the named rows keep in materialize()
Case = namedtuple("Case", "added dead survivors")
CASES = {
    "r17_dead_0": Case([], {ROW_17: [0]}, {ROW_17: 16}),
    "r17_dead_15": Case([], {ROW_17: [15]}, {ROW_17: 16}),
    "r17_dead_16_the_last": Case([], {ROW_17: [16]}, {ROW_17: 16}),
    "r17_dead_15_16": Case([], {ROW_17: [15, 16]}, {ROW_17: 15}),
    "r17_dead_14_15_16_over_the_reload": Case([], {ROW_17: [14, 15, 16]}, {ROW_17: 14}),
    "r17_all_dead": Case([], {ROW_17: list(range(17))}, {ROW_17: 0}),
    "r17_delta_behind_16": Case([ADD_17], {}, {ROW_17: 18}),
    "r16_dead_15_the_last": Case([], {ROW_16: [15]}, {ROW_16: 15}),
    "r16_add_above": Case([ADD_16], {}, {ROW_16: 17}),
    "r33_add_equal_15_32": Case(ADD_33, {}, {ROW_33: 35}),
    "r100_two_added": Case(ADD_100, {}, {ROW_100: 102}),
    "r33_dead_16": Case([], {ROW_33: [16]}, {ROW_33: 32}),
    "r33_dead_31_32": Case([], {ROW_33: [31, 32]}, {ROW_33: 31}),
    "r33_dead_15_to_32_over_a_chunk": Case([], {ROW_33: list(range(15, 33))}, {ROW_33: 15}),
    "multi_type_1": Case([], {MULTI_ROW: MULTI_DEAD}, {MULTI_ROW: 16}),
    "r0_delta_only": Case(ADD_0, {}, {ROW_0: 3}),
    "r1_emptied": Case([], {ROW_1: [0]}, {ROW_1: 0}),
    "r1_emptied_with_delta": Case([ADD_1], {ROW_1: [0]}, {ROW_1: 1}),
    "r100_one_dead_two_added": Case(ADD_100, {ROW_100: [57]}, {ROW_100: 101}),
    "everything": Case(
        [ADD[ROW_7]["below"], ADD[ROW_8]["equal"], ADD[ROW_9]["above"]] + ADD_0 + [ADD_1, ADD_17] + ADD_100,
        {ROW_17: [14, 15, 16], ROW_33: list(range(15, 33)), MULTI_ROW: MULTI_DEAD, ROW_1: [0], ROW_100: [57], ROW_16: [15],
         ROW_15: [0]},
        {ROW_0: 3, ROW_1: 1, ROW_7: 8, ROW_8: 9, ROW_9: 10, ROW_15: 14, ROW_16: 15, ROW_17: 15, ROW_18: 16, ROW_33: 15,
         ROW_100: 101}),
    "nothing": Case([], {}, {}),
}
for _row, _length in ((ROW_7, 8), (ROW_8, 9), (ROW_9, 10)):   # merged lengths 8, 9 and 10
    for _place in ("below", "equal", "above"):
        CASES["r%d_add_%s" % (_length - 1, _place)] = Case([ADD[_row][_place]], {}, {_row: _length})
ADD_ONLY = [name for name, case in CASES.items() if not case.dead]

# Per-slice dead (row, col, type) keys for ultra_rspmm_edit_rows_samples, five slices each (a test takes the first n_outer).
# slice 0: all eight name the 17-row -- its base edge at position 16 and the delta edge behind it among them;
# slice 1: the type = -1 key on the multi-type column, and the rows of 0 and 1 edges left without any edge wherever they are touched;
# slice 2: rows that no case touches;  slice 3: first / last positions, an edge that "everything" also tombstones, a delta edge;
# slice 4: delta edges of the small rows, a key of the wrong type.
_QUIET_EDGES = [e for e in EDGES if e[0] in QUIET_ROWS][:8]
KEYS_8 = [
    [edge_at(ROW_17, 16), ADD_17, edge_at(ROW_17, 0), edge_at(ROW_17, 15), edge_at(ROW_17, 3)[:2] + (-1,), (ROW_17, UNUSED_COL, 0),
     other_type(ROW_17, 5), edge_at(ROW_17, 8)],
    [(MULTI_ROW, MULTI_COL, -1), edge_at(ROW_1, 0), ADD_1, (ROW_0, 20, -1), (ROW_0, 11, 5), edge_at(ROW_100, 99),
     edge_at(ROW_33, 32), (ROW_7, 1, -1)],
    _QUIET_EDGES + [(3, UNUSED_COL, 0)] * (8 - len(_QUIET_EDGES)),
    [edge_at(ROW_9, 8), edge_at(ROW_8, 0), edge_at(ROW_16, 15), edge_at(ROW_15, 7), edge_at(ROW_33, 16), edge_at(ROW_33, 15),
     edge_at(ROW_100, 0), ADD_100[0]],
    [edge_at(ROW_17, 16), edge_at(ROW_33, 17)[:2] + (-1,), (MULTI_ROW, MULTI_COL, 1), partner(*ADD[ROW_7]["below"])[:2] + (-1,),
     ADD[ROW_8]["equal"][:2] + (-1,), ADD[ROW_9]["above"], ADD_0[1], (ROW_1, 126, 1)],
]
KEYS_1 = [[edge_at(ROW_17, 16)], [(MULTI_ROW, MULTI_COL, -1)], [_QUIET_EDGES[0]], [edge_at(ROW_1, 0)], [ADD_17]]
KEY_TABLES = {"keys_1": KEYS_1, "keys_8": KEYS_8}


def apply_case(data, case, capacity=CAPACITY):
    """A fresh GraphDelta on `data` with the case's facts added, then its facts retracted."""
    delta = rspmm.GraphDelta(data, capacity=capacity)
    if case.added:
        delta.add(*zip(*[fact(*edge) for edge in case.added]))
    gone = [fact(*edge_at(row, pos)) for row, positions in case.dead.items() for pos in positions]
    if gone:
        delta.remove(*zip(*gone))
    return delta


def key_hits(edge, keys):
    return any(edge[:2] == key[:2] and (key[2] < 0 or key[2] == edge[2]) for key in keys)


@pytest.fixture(scope="module")
def data():
    return base_graph()


@pytest.fixture(scope="module")
def deltas(data):
    return {name: apply_case(data, case) for name, case in CASES.items()}


def test_the_base_graph_is_what_the_cases_rely_on(data):
    assert data.edge_index.shape[1] == len(EDGES) == 380
    degree = torch.bincount(data.edge_index[0], minlength=N)
    assert {row: int(degree[row]) for row in DEGREES} == DEGREES
    assert len(BASE_SET) < len(EDGES)                                         # duplicates
    assert not bool((data.edge_index[1] == UNUSED_COL).any())
    for row in DEGREES:
        cols = [col for col, _ in BASE_ROWS[row]]
        assert cols == sorted(cols) and all(8 <= col < 110 for col in cols), row
        plain = [col for col in cols if not (row == MULTI_ROW and col == MULTI_COL)]
        assert len(set(plain)) == len(plain), row                             # "the edge at position p" is one edge
    assert sorted(kind for col, kind in BASE_ROWS[MULTI_ROW] if col == MULTI_COL) == MULTI_TYPES and len(MULTI_DEAD) == 2
    assert len(_QUIET_EDGES) >= 2                                             # the quiet rows hold edges for keys to name
    # the added edges sit where their names say
    for row, places in ADD.items():
        cols = [col for col, _ in BASE_ROWS[row]]
        assert places["below"][1] < cols[0] and places["above"][1] > cols[-1] and places["equal"][1] in cols, row
    assert ADD_17[1] == BASE_ROWS[ROW_17][16][0] and ADD_17 not in BASE_SET
    assert ADD_16[1] > BASE_ROWS[ROW_16][15][0] and [edge[1] for edge in ADD_33] == [BASE_ROWS[ROW_33][p][0] for p in (15, 32)]
    assert all(edge not in BASE_SET for case in CASES.values() for edge in case.added)


@pytest.mark.parametrize("name", list(CASES))
def test_the_case_is_what_its_name_says(data, deltas, name):
    case, delta = CASES[name], deltas[name]
    dead = [edge_at(row, pos) for row, positions in case.dead.items() for pos in positions]
    # no retraction took an added fact out; the keys are the dead edges and those of their partner edges that the base graph states
    assert len(delta) == len(case.added)
    keys = set(dead) | {partner(*edge) for edge in dead if partner(*edge) in BASE_SET}
    assert delta.num_removed == len(keys)
    added = list(case.added) + [partner(*edge) for edge in case.added]
    touched = sorted({edge[0] for edge in added} | {key[0] for key in keys})
    count = int(delta.count)
    assert delta.rows[:count].tolist() == touched and delta.edited == bool(touched)
    assert not set(touched) & set(QUIET_ROWS)
    # per touched row: the delta's edges ascend by column, the dead keys are distinct and ascend by (col, type), and in the special
    # rows they sit at the sorted positions the case names
    ptr, dead_ptr = delta.ptr[:count + 1].tolist(), delta.dead_ptr[:count + 1].tolist()
    assert ptr[0] == 0 and dead_ptr[0] == 0 and ptr[-1] == 2 * len(case.added) and dead_ptr[-1] == len(keys)
    for k, row in enumerate(touched):
        extra = list(zip(delta.col[ptr[k]:ptr[k + 1]].tolist(), delta.type[ptr[k]:ptr[k + 1]].tolist()))
        assert sorted(extra) == sorted(edge[1:] for edge in added if edge[0] == row), (name, row)
        assert [col for col, _ in extra] == sorted(col for col, _ in extra), (name, row)
        held = list(zip(delta.dead_col[dead_ptr[k]:dead_ptr[k + 1]].tolist(), delta.dead_type[dead_ptr[k]:dead_ptr[k + 1]].tolist()))
        assert held == sorted(set(held)) == sorted(key[1:] for key in keys if key[0] == row), (name, row)
        if row in DEGREES:
            assert [p for p, pair in enumerate(BASE_ROWS[row]) if pair in held] == case.dead.get(row, []), (name, row)
    # the materialised list: per row the base edges that no key names, then the added ones
    mat = delta.materialize()
    left = torch.bincount(mat.edge_index[0], minlength=N).tolist()
    for row in range(N):
        want = sum((row,) + pair not in keys for pair in BASE_ROWS[row]) + sum(edge[0] == row for edge in added)
        assert left[row] == want, (name, row)
    for row, want in case.survivors.items():
        assert left[row] == want, (name, row)
    assert set(case.survivors) == {row for row in touched if row in DEGREES}


def test_the_key_tables_are_what_they_say(deltas):
    mat = deltas["everything"].materialize()
    edges = list(zip(mat.edge_index[0].tolist(), mat.edge_index[1].tolist(), mat.edge_type.tolist()))
    everything = set(deltas["everything"].rows[:int(deltas["everything"].count)].tolist())
    ever_touched = set()
    for delta in deltas.values():
        ever_touched |= set(delta.rows[:int(delta.count)].tolist())
    for table in KEY_TABLES.values():
        assert len(table) == 5 and len({len(keys) for keys in table}) == 1
        assert not {key[0] for key in table[2]} & ever_touched                # a slice whose keys name no touched row
    assert {key[0] for key in KEYS_8[0]} == {ROW_17} and len(KEYS_8[0]) == 8   # all eight keys of one slice name one row
    # slice 0 kills the base edge at position 16 of the 17-row -- where "everything" has not taken it already -- and a delta edge
    assert edge_at(ROW_17, 16) in KEYS_8[0] and ADD_17 in KEYS_8[0] and ADD_17 in edges
    for table in KEY_TABLES.values():
        assert (MULTI_ROW, MULTI_COL, -1) in table[1]                         # the any-type key on the multi-type column
    assert sum(key_hits(edge, KEYS_8[1]) for edge in edges if edge[:2] == (MULTI_ROW, MULTI_COL)) == 2      # types 0 and 2 were left
    # slice 1 leaves the rows of 0 and 1 base edges without any edge, though "everything" gave both delta edges
    for row in (ROW_0, ROW_1):
        assert row in everything and any(edge[0] == row for edge in edges)
        assert all(key_hits(edge, KEYS_8[1]) for edge in edges if edge[0] == row)


# ---- the kernel's documented order, restated on the host ----
def start_value(sum, dtype):
    return 0.0 if sum == "add" else (torch.finfo(dtype).max if sum == "min" else -torch.finfo(dtype).max)


def reduce_step(sum, acc, term):
    return acc + term if sum == "add" else (torch.minimum(acc, term) if sum == "min" else torch.maximum(acc, term))


def merged_rows(delta, rel, x, bnd, sum, mul):
    """{touched row: its value}: per touched row the base edges that carry no tombstone merged with the delta's edges by column,
    base first on ties; reduced one after the other from the start value; the boundary last.  Read from the arrays the kernels
    read (GraphDelta._prepare) and from the base rows in the plan's order."""
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
        acc = torch.full((x.shape[1],), start_value(sum, x.dtype), dtype=x.dtype)
        for c, t in merged:
            acc = reduce_step(sum, acc, rel[t] * x[c] if mul == "mul" else rel[t] + x[c])
        out[row] = acc if bnd is None else reduce_step(sum, acc, bnd[row])
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("mul", ["mul", "add"])
@pytest.mark.parametrize("sum", ["add", "min", "max"])
def test_the_documented_order_equals_the_oracle_on_the_materialised_list(deltas, sum, mul, dtype):
    g = torch.Generator().manual_seed(7)
    x, rel, bnd = (torch.randn(n, 8, generator=g, dtype=dtype) for n in (N, R, N))
    moved = 0
    for name, delta in deltas.items():
        mat = delta.materialize()
        plain = rspmm_oracle.generalized_rspmm(mat.edge_index, mat.edge_type, torch.ones(mat.edge_index.shape[1], dtype=dtype),
                                               rel, x, sum=sum, mul=mul)
        for boundary in (None, bnd):
            want = plain if boundary is None else reduce_step(sum, plain, boundary)
            got = merged_rows(delta, rel, x, boundary, sum, mul)
            assert sorted(got) == delta.rows[:int(delta.count)].tolist(), name
            for row, value in got.items():
                assert torch.equal(value, want[row]), (name, row, boundary is not None)
        # the tie rule is observable: with the delta edge of an equal column taken FIRST, a sum of three or more terms rounds otherwise
        if sum == "add" and name.endswith("add_equal"):
            (row, col, kind), = CASES[name].added
            early = torch.zeros(8, dtype=dtype)
            for c, t in sorted(BASE_ROWS[row] + [(col, kind)], key=lambda pair: (pair[0], pair != (col, kind))):
                early = early + (rel[t] * x[c] if mul == "mul" else rel[t] + x[c])
            moved += int(not torch.equal(early, plain[row]))
    if sum == "add":
        assert moved >= 1
