"""The host compiler of logical queries (ultra_amd/query_exec.py) on the CPU: the schedule of the golden batch and of every
type alone, `run_reference` against `UltraQuery.forward` with recording stub projections (logits, final symbolic sets and every
projection call's inputs, bit for bit and in order), every compile-time error, and the two new entry points' bindings."""
import io
import lzma
import os
import random
import re
import types

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz")
LOGICS = ["product", "godel", "lukasiewicz"]
_GOLDEN = []


def load():
    if not _GOLDEN:
        with open(GOLDEN, "rb") as f:
            _GOLDEN.append(torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False))
    return _GOLDEN[0]


def plain(query):
    return torch.as_tensor(query).as_subclass(torch.Tensor)


def type_rows(g, name):
    """The golden queries of one type (two of each)."""
    t = g["id2type"].index(name)
    return plain(g["query"])[g["type"] == t]


def remap_entities(query, num_nodes):
    """The same queries over a graph of num_nodes nodes: entity ids modulo num_nodes, everything else untouched."""
    from ultra_amd.ultraquery import Query
    q = plain(query).clone()
    operand = (q & Query.operation) == 0
    q[operand] = q[operand] % num_nodes
    return q


def random_queries(batch, num_nodes, num_relations, seed, max_len=9):
    """Seeded random valid postfix rows: every prefix keeps the stack within [1, 2] values and the row ends with one."""
    from ultra_amd.ultraquery import Query
    rng = random.Random(seed)
    rows = []
    for _ in range(batch):
        row, depth = [rng.randrange(num_nodes)], 1
        want = rng.randint(1, max_len)
        while len(row) < want or depth != 1:
            choices = ["p", "n"] if len(row) < want else []
            if depth < 2 and len(row) < want:
                choices.append("e")
            if depth == 2:
                choices += ["i", "u"] * (1 if len(row) < want else 4)
            op = rng.choice(choices)
            if op == "e":
                row.append(rng.randrange(num_nodes))
                depth += 1
            elif op == "p":
                row.append(Query.projection | rng.randrange(num_relations))
            elif op == "n":
                row.append(Query.negation)
            else:
                row.append((Query.intersection if op == "i" else Query.union) | 2)
                depth -= 1
        rows.append(row + [Query.stop])
    width = max(len(r) for r in rows)
    return torch.tensor([r + [Query.stop] * (width - len(r)) for r in rows], dtype=torch.long)


class RecordingStub(nn.Module):
    """A projection stand-in: a deterministic torch function of (h, r) that records its calls."""

    def __init__(self, symbolic):
        super(RecordingStub, self).__init__()
        self.symbolic = symbolic
        self.calls = []

    def forward(self, graph, h_prob, r_index):
        self.calls.append((h_prob.clone(), r_index.as_subclass(torch.Tensor).clone()))
        return stub_projection(h_prob, r_index, self.symbolic)


def stub_projection(h, r, symbolic):
    r = r.as_subclass(torch.Tensor).float().unsqueeze(1)
    if symbolic:      # 0/1 sets stay 0/1 sets
        return torch.max(h.roll(1, -1), h.roll(-2, -1)) * ((r % 3) != 1).float() + h * ((r % 3) == 1).float()
    col = torch.arange(h.shape[1], dtype=torch.float32, device=h.device)
    return torch.sigmoid(h.roll(1, -1) * 3 - 1 + torch.sin(col * 0.37 + r))


def stub_model(logic):
    from ultra_amd.ultraquery import UltraQuery
    uq = UltraQuery(nn.Module(), logic=logic)
    uq.model = RecordingStub(False)
    uq.symbolic_model = RecordingStub(True)
    return uq.eval()


def check_against_interpreter(query, num_nodes, num_relations, logic, symbolic):
    from ultra_amd import query_exec
    graph = types.SimpleNamespace(num_nodes=num_nodes, num_relations=num_relations)
    eager, compiled = stub_model(logic), stub_model(logic)
    want = eager(graph, query, symbolic_traversal=symbolic)
    program = query_exec.compile(query, num_nodes, num_relations)
    prob, sym = query_exec.run_reference(
        program, logic, lambda h, r: compiled.model(graph, h, r),
        (lambda h, r: compiled.symbolic_model(graph, h, r)) if symbolic else None)
    assert torch.equal(query_exec.logit(prob), want)
    for a, b in ((eager.model, compiled.model), (eager.symbolic_model, compiled.symbolic_model)):
        assert len(a.calls) == len(b.calls) == (len(program.projections) if (symbolic or a is eager.model) else 0)
        for (h0, r0), (h1, r1) in zip(a.calls, b.calls):
            assert torch.equal(h0, h1) and torch.equal(r0, r1)
    if symbolic:
        st = eager.symbolic_stack
        assert torch.equal(st.SP, torch.ones_like(st.SP))
        assert torch.equal(sym, st.stack[torch.arange(len(query)), st.SP - 1])
    else:
        assert sym is None


def test_compile_golden_batch_schedule():
    from ultra_amd import query_exec
    g = load()
    program = query_exec.compile(g["query"], g["num_nodes"], g["num_relations"])
    assert program.batch == 28
    assert [len(p.samples) for p in program.projections] == [28, 26, 18]
    assert [program.num_micro_ops(s) for s in range(len(program.segments))] == [28, 16, 32, 14]
    assert program.max_depth() == 2
    for p in program.projections:
        assert p.samples == sorted(p.samples) and len(p.relations) == len(p.samples)
    last = program.segments[-1]
    assert last.pop_row == list(range(28))
    # every sample ends with exactly one value
    for b in range(28):
        d = last.entry_depth[b] + (1 if last.push_row[b] >= 0 else 0)
        d += sum(1 if k == query_exec.PUSH_ENTITY else (-1 if k in (query_exec.AND, query_exec.OR) else 0)
                 for k, _ in last.ops[b])
        assert d == 1
    # ids do not enter the signature, structure does
    other = remap_entities(g["query"], 17)
    assert query_exec.compile(other, 17, g["num_relations"]).signature() == program.signature()
    assert query_exec.compile(plain(g["query"])[:27], g["num_nodes"], g["num_relations"]).signature() != program.signature()
    hash(program.signature())


def test_compile_projection_calls_per_type():
    """Two queries of one type advance in lockstep: one projection call per relation of the structure (the two projections of
    a 2i belong to one sample, so they cannot share a call)."""
    from ultra_amd import query_data, query_exec
    g = load()

    def relations(struct):
        return sum(relations(s) for s in struct) if isinstance(struct, tuple) else int(struct == "r")
    want = {name: relations(struct) for struct, name in query_data.STRUCT2TYPE.items()}
    assert (want["1p"], want["2p"], want["3p"], want["2i"], want["3i"], want["ip"], want["up-DNF"]) == (1, 2, 3, 2, 3, 3, 3)
    for name in g["id2type"]:
        rows = type_rows(g, name)
        assert len(rows) == 2
        program = query_exec.compile(rows, g["num_nodes"], g["num_relations"])
        assert len(program.projections) == want[name], name
        assert all(p.samples == [0, 1] for p in program.projections)
        assert len(program.segments) == want[name] + 1


@pytest.mark.parametrize("logic", LOGICS)
@pytest.mark.parametrize("symbolic", [True, False])
def test_run_reference_equals_interpreter(logic, symbolic):
    g = load()
    check_against_interpreter(g["query"], g["num_nodes"], g["num_relations"], logic, symbolic)
    for name in g["id2type"]:
        check_against_interpreter(type_rows(g, name), g["num_nodes"], g["num_relations"], logic, symbolic)
    check_against_interpreter(random_queries(9, 23, 5, seed=4), 23, 5, logic, symbolic)


def test_compile_errors():
    from ultra_amd import query_exec
    from ultra_amd.ultraquery import Query
    P, I, U, N, S = Query.projection, Query.intersection | 2, Query.union | 2, Query.negation, Query.stop

    def refuse(row, match, num_nodes=10, num_relations=4):
        with pytest.raises(ValueError, match=match):
            query_exec.compile(torch.tensor([[0, P | 1, S] + [S] * (len(row) - 3), row]), num_nodes, num_relations)

    refuse([1, 2, 3, S], "Stack overflow: a selected sample already holds 2 values")
    refuse([I, S, S, S], "Stack underflow: a selected sample holds no value")
    refuse([1, U, S, S], "Stack underflow")
    refuse([N, S, S, S], "Stack underflow")
    refuse([P | 1, S, S, S], "Stack underflow")
    refuse([1, 2, S, S], "More operands than expected")
    refuse([S, S, S, S], "Stack underflow")                    # ends with an empty stack
    refuse([1, P | 1, N, N], "no stop")
    refuse([10, P | 1, S, S], r"entity id 10 outside \[0, 10\)")
    refuse([1, P | 4, S, S], r"relation id 4 outside \[0, 4\)")
    refuse([1, P | I, S, S], "Unknown operator")
    with pytest.raises(ValueError, match="int64"):
        query_exec.compile(torch.zeros(3, dtype=torch.long), 10, 4)
    # the arity field of an intersection is ignored, as in UltraQuery._binary
    program = query_exec.compile(torch.tensor([[1, 2, Query.intersection | 3, S]]), 10, 4)
    assert program.segments[0].ops[0][-1] == (query_exec.AND, 0)
    # the eager route refuses the same rows with the same texts
    from ultra_amd.ultraquery import UltraQuery
    uq = UltraQuery(nn.Module()).eval()
    graph = types.SimpleNamespace(num_nodes=10, num_relations=4)
    with pytest.raises(ValueError, match="Stack overflow: a selected sample already holds 2 values"):
        uq(graph, torch.tensor([[1, 2, 3, S]]))
    with pytest.raises(ValueError, match="More operands than expected"):
        uq(graph, torch.tensor([[1, 2, S, S]]))


def test_execute_refuses_training_and_runs_the_reference_on_cpu():
    from ultra_amd import query_exec
    g = load()
    graph = types.SimpleNamespace(num_nodes=g["num_nodes"], num_relations=g["num_relations"],
                                  edge_index=torch.zeros(2, 0, dtype=torch.long))
    uq = stub_model("godel")
    rows = type_rows(g, "pin")
    want = stub_model("godel")(graph, rows, symbolic_traversal=True)
    logits, sym = query_exec.execute(uq, graph, rows)
    assert torch.equal(logits, want) and sym.shape == want.shape
    assert torch.equal(query_exec.forward(uq, graph, query_exec.compile(rows, g["num_nodes"], g["num_relations"]), False), want)
    assert not hasattr(uq, "stack")                 # (the compiled route does not populate the interpreter's stacks)
    uq.train()
    with pytest.raises(ValueError, match="eval mode only"):
        query_exec.execute(uq, graph, rows)


def test_new_entry_points_bound_as_declared():
    """The argument counts of the bindings equal those of the header's declarations (the exports themselves are covered by
    tests/test_abi.py)."""
    from ultra_amd import _lib
    text = open(os.path.join(ROOT, "include", "ultra_nbfnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ultra_query_segment", "ultra_nonzero_lists"):
        params = re.search(r"int32_t %s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(getattr(_lib.lib, name).argtypes) == params.count(",") + 1, name
    lib = _lib.lib
    # decided before any pointer is looked at / nothing launched
    assert lib.ultra_query_segment(None, None, None, None, None, 1, 8, 3, 0, 0, None, None, 0, None, 0, None, None, None,
                                   None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_query_segment(None, None, None, None, None, 1, 8, 2, 1, 0, None, None, 0, None, 0, None, None, None,
                                   None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_query_segment(None, None, None, None, None, 1, 1 << 31, 2, 0, 0, None, None, 0, None, 0, None, None, None,
                                   None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_query_segment(None, None, None, None, None, 1, 8, 2, 0, 0, None, None, 0, None, 0, None, None, None,
                                   None) == _lib.ULTRA_ERR_INVALID
    assert lib.ultra_query_segment(None, None, None, None, None, 1, 8, 2, 0, 3, None, None, 0, None, 0, None, None, None,
                                   None) == _lib.ULTRA_ERR_INVALID
    assert lib.ultra_nonzero_lists(None, 2, 8, None, None, None, 16, None) == _lib.ULTRA_ERR_INVALID
