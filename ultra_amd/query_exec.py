"""Compiled execution of complex logical queries.

`UltraQuery.execute` interprets a batch of postfix queries on the device: every instruction is a handful of small torch
launches and about a dozen host synchronisations (mask reductions, boolean-mask indexing, the stack's overflow checks).  But
the queries are known on the host before anything runs, so the interpreter's whole schedule is too:

  compile          replays the interpreter's loop on the host (instruction pointer and stack depth per sample) and returns a
                   `Program`: segment, projection, segment, ..., segment.  A projection is ONE call for the samples that
                   wait at one (ascending sample order), placed where the interpreter places it: when no other operation is
                   pending anywhere in the batch.  A segment is, per sample, the micro-ops (PUSH_ENTITY, AND, OR, NOT) it
                   runs between two projections.  Every error the interpreter finds on the device is found here.
  run_reference    the program in plain torch on any device -- the definition the kernel is tested against
  execute/forward  the program on the GPU: one asynchronous upload of all program arrays per batch, one launch of
                   ultra_query_segment (csrc/query_exec_kernels.hip) per segment, the unchanged `model.model` /
                   `model.symbolic_model` per projection, and no call that waits for the device
  nonzero_lists    the non-zero ids of every row of a (batch, n) matrix as ragged ascending lists (ultra_nonzero_lists): the
                   layout ultra_filtered_topk takes for the entities to leave out; num_live: over the live ids of a graph
                   with reserved rows (ultra_nonzero_lists_live); retired: without the ids of a device
                   bitmap (ultra_nonzero_lists_alive)

The compiled route computes exactly what the interpreter computes: the same fuzzy-set arithmetic operation for operation,
the same projection calls with the same inputs in the same order.  It keeps what a caller of `forward` gets -- the logits
and the final symbolic sets.  It does NOT keep the interpreter's `var` / `symbolic_var` stacks (nothing in the package reads
them) and it does not populate `model.stack` / `model.symbolic_stack`.  Training stays with the interpreter: its traversal
dropout draws per projection.
"""
import inspect
from collections import namedtuple

import torch

from . import _lib, models, selection
from .ultraquery import Query, UltraQuery, _logic

PUSH_ENTITY, AND, OR, NOT = 0, 1, 2, 3
KIND_NAMES = ("e", "i", "u", "n")
# device encoding of a micro-op, one 32-bit word: an entity id (>= 0) pushes its one-hot set
OP_AND, OP_OR, OP_NOT = -1, -2, -3
LOGIC_CODES = {"product": 0, "godel": 1, "lukasiewicz": 2}
MAX_BATCH = 65535

Segment = namedtuple("Segment", "entry_depth push_row pop_row ops")
Projection = namedtuple("Projection", "samples relations")

_OVERFLOW = "Stack overflow: a selected sample already holds %d values"
_UNDERFLOW = "Stack underflow: a selected sample holds no value"


class Program(object):
    """The schedule of one batch: `segments` (len(projections) + 1 of them) and `projections`.

    Segment s, per sample b: entry_depth[b] values are on b's stack; if push_row[b] >= 0 row push_row[b] of projection
    s - 1's output is pushed; ops[b], a list of (kind, entity id or 0), run in order; if pop_row[b] >= 0 the top is popped into
    row pop_row[b] of projection s's input -- in the last segment pop_row[b] = b, the result."""

    def __init__(self, batch, num_nodes, num_relations, stack_size, segments, projections):
        self.batch, self.num_nodes, self.num_relations, self.stack_size = batch, num_nodes, num_relations, stack_size
        self.segments, self.projections = segments, projections
        self._packed = None

    def num_micro_ops(self, s):
        return sum(len(ops) for ops in self.segments[s].ops)

    def max_depth(self):
        """The deepest any sample's stack gets."""
        deepest = 0
        for seg in self.segments:
            for b in range(self.batch):
                d = seg.entry_depth[b] + (1 if seg.push_row[b] >= 0 else 0)
                deepest = max(deepest, d)
                for kind, _ in seg.ops[b]:
                    d += 1 if kind == PUSH_ENTITY else (-1 if kind in (AND, OR) else 0)
                    deepest = max(deepest, d)
        return deepest

    def signature(self):
        """A hashable summary of the structure without entity and relation ids: programs with equal signatures differ
        only in the ids of their operands."""
        segs = tuple(tuple("".join(KIND_NAMES[k] for k, _ in ops) for ops in seg.ops) for seg in self.segments)
        return (self.batch, self.stack_size, segs, tuple(tuple(p.samples) for p in self.projections))

    def packed(self):
        """(bytes, relation offsets, segment offsets): every array the device needs as one uint8 host tensor.  First the
        relation ids of all projections (int64), then per segment entry_depth, push_row, pop_row (batch each), op_ptr
        (batch + 1) and the micro-op words (int32).  Offsets count elements of their own type."""
        if self._packed is None:
            rel, rel_off = [], []
            for p in self.projections:
                rel_off.append(len(rel))
                rel += p.relations
            words, seg_off = [], []
            for seg in self.segments:
                ptr, ops = [0], []
                for sample in seg.ops:
                    ops += [e if kind == PUSH_ENTITY else (OP_AND, OP_OR, OP_NOT)[kind - 1] for kind, e in sample]
                    ptr.append(len(ops))
                seg_off.append(len(words))
                words += seg.entry_depth + seg.push_row + seg.pop_row + ptr + ops
            rel_t = torch.tensor(rel, dtype=torch.int64)
            word_t = torch.tensor(words, dtype=torch.int32)
            self._packed = (torch.cat([rel_t.view(torch.uint8), word_t.view(torch.uint8)]), rel_off, seg_off)
        return self._packed


def _kind(word, row):
    flags = word & Query.operation
    if word < 0 or flags & (flags - 1):
        raise ValueError("Unknown operator `%d` in query %d" % (word, row))
    return flags


def compile(query, num_nodes, num_relations, stack_size=UltraQuery.stack_size, num_live=None, retired=None):
    """The `Program` of a (batch, L) int64 batch of postfix queries (a `Query` or a tensor; a CUDA tensor is copied to the
    host once).  Raises ValueError for everything `UltraQuery.forward` would refuse, or fault on, while it runs: stack
    overflow and underflow, more than one value left, nothing left, a row without `stop`, an entity id outside
    [0, num_nodes), a relation id outside [0, num_relations).  num_live (a graph with reserved rows, DESIGN.md section 21:
    num_nodes counts slots): the anchors are the ids below it; None: below num_nodes.  retired (a collection of ids, DESIGN.md
    section 29: the entities a served graph retired): an anchor among them is a ValueError too."""
    q = torch.as_tensor(query)
    if q.dim() != 2 or q.dtype != torch.int64:
        raise ValueError("compile takes a (batch, L) int64 batch of postfix queries, got %s %s" % (tuple(q.shape), q.dtype))
    rows = q.detach().as_subclass(torch.Tensor).cpu().tolist()
    batch, length = len(rows), q.shape[1]
    num_nodes, num_relations, stack_size = int(num_nodes), int(num_relations), int(stack_size)
    num_live = num_nodes if num_live is None else int(num_live)
    if not 0 <= num_live <= num_nodes:
        raise ValueError("num_live must lie in [0, num_nodes = %d], got %d" % (num_nodes, num_live))
    if retired is None:
        retired = ()
    elif torch.is_tensor(retired):
        retired = retired.detach().as_subclass(torch.Tensor).flatten().cpu().tolist()
    retired = frozenset(int(v) for v in retired)
    payload = ~Query.operation
    ip, depth = [0] * batch, [0] * batch
    segments, projections = [], []
    entry, push_row, ops = [0] * batch, [-1] * batch, [[] for _ in range(batch)]
    while True:
        for b in range(batch):
            if ip[b] >= length:
                raise ValueError("query %d has no stop" % b)
        word = [rows[b][ip[b]] for b in range(batch)]
        kind = [_kind(word[b], b) for b in range(batch)]
        if all(k == Query.stop for k in kind):
            break
        elementwise = [b for b in range(batch) if kind[b] not in (Query.projection, Query.stop)]
        for b in elementwise:
            if kind[b] == 0:
                if depth[b] >= stack_size:
                    raise ValueError(_OVERFLOW % stack_size)
                if not 0 <= word[b] < num_live:
                    raise ValueError("query %d: entity id %d outside [0, %d)" % (b, word[b], num_live))
                if word[b] in retired:
                    raise ValueError("query %d: entity id %d was retired and is no anchor" % (b, word[b]))
                ops[b].append((PUSH_ENTITY, word[b]))
                depth[b] += 1
            elif kind[b] == Query.negation:
                if depth[b] < 1:
                    raise ValueError(_UNDERFLOW)
                ops[b].append((NOT, 0))
            else:       # two operands whatever the arity field says, as UltraQuery._binary
                if depth[b] < 2:
                    raise ValueError(_UNDERFLOW)
                ops[b].append((AND if kind[b] == Query.intersection else OR, 0))
                depth[b] -= 1
            ip[b] += 1
        if elementwise:
            continue
        # no other operation is pending anywhere: the samples at a projection form one call, in ascending order
        samples = [b for b in range(batch) if kind[b] == Query.projection]
        pop_row = [-1] * batch
        for i, b in enumerate(samples):
            if depth[b] < 1:
                raise ValueError(_UNDERFLOW)
            if not 0 <= word[b] & payload < num_relations:
                raise ValueError("query %d: relation id %d outside [0, %d)" % (b, word[b] & payload, num_relations))
            pop_row[b] = i
            depth[b] -= 1
        segments.append(Segment(entry, push_row, pop_row, ops))
        projections.append(Projection(samples, [word[b] & payload for b in samples]))
        entry, push_row, ops = list(depth), [-1] * batch, [[] for _ in range(batch)]
        for i, b in enumerate(samples):
            push_row[b] = i
            depth[b] += 1
            ip[b] += 1
    if any(d > 1 for d in depth):
        raise ValueError("More operands than expected")
    if any(d < 1 for d in depth):
        raise ValueError(_UNDERFLOW)
    segments.append(Segment(entry, push_row, list(range(batch)), ops))
    return Program(batch, num_nodes, num_relations, stack_size, segments, projections)


def logit(prob):
    """UltraQuery.forward's last line."""
    return ((prob + 1e-10) / (1 - prob + 1e-10)).log()


def _as_program(query_or_program, graph):
    if isinstance(query_or_program, Program):
        if query_or_program.num_nodes != int(graph.num_nodes):
            raise ValueError("the program was compiled for %d nodes, the graph has %d"
                             % (query_or_program.num_nodes, int(graph.num_nodes)))
        return query_or_program
    return compile(query_or_program, graph.num_nodes, graph.num_relations)


def run_reference(program, logic, projection, symbolic=None, device=None):
    """The program in plain torch: (prob (batch, num_nodes) fp32, final symbolic set or None).  `projection(h_prob,
    r_index)` and `symbolic(sym_h_prob, r_index)` are called once per projection of the program, in order, neural first;
    symbolic None: no symbolic stack."""
    conj, disj = _logic(logic)
    batch, n, depth_max = program.batch, program.num_nodes, program.stack_size
    stacks = [torch.zeros(batch, depth_max, n, device=device)]
    results = [torch.zeros(batch, n, device=device)]
    if symbolic is not None:
        stacks.append(torch.zeros(batch, depth_max, n, device=device))
        results.append(torch.zeros(batch, n, device=device))
    outs = [None] * len(stacks)
    last = len(program.segments) - 1
    for s, seg in enumerate(program.segments):
        rows = batch if s == last else len(program.projections[s].samples)
        targets = results if s == last else [torch.zeros(rows, n, device=device) for _ in stacks]
        for stack, out, target in zip(stacks, outs, targets):
            for b in range(batch):
                d = seg.entry_depth[b]
                if seg.push_row[b] >= 0:
                    stack[b, d] = out[seg.push_row[b]]
                    d += 1
                for kind, e in seg.ops[b]:
                    if kind == PUSH_ENTITY:
                        stack[b, d] = 0
                        stack[b, d, e] = 1
                        d += 1
                    elif kind == NOT:
                        stack[b, d - 1] = 1 - stack[b, d - 1]
                    else:
                        stack[b, d - 2] = (conj if kind == AND else disj)(stack[b, d - 2], stack[b, d - 1])
                        d -= 1
                if seg.pop_row[b] >= 0:
                    target[seg.pop_row[b]] = stack[b, d - 1]
        if s < last:
            r_index = torch.tensor(program.projections[s].relations, dtype=torch.int64, device=device)
            outs[0] = projection(targets[0], r_index)
            if symbolic is not None:
                outs[1] = symbolic(targets[1], r_index)
    return results[0], (results[1] if symbolic is not None else None)


def segment(words, offset, batch, num_nodes, logic, stack, push_src, pop_dst, sym_stack=None, sym_push_src=None,
            sym_pop_dst=None):
    """One launch of ultra_query_segment.  `words`: the int32 device tensor of Program.packed(), `offset` the segment's
    start in it; stack (batch, 2, N) fp32; push_src (rows, N) or None; pop_dst (rows, N) or None; the symbolic three alike."""
    def rows(t):
        return 0 if t is None else t.shape[0]
    for t in (stack, push_src, pop_dst, sym_stack, sym_push_src, sym_pop_dst):
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("ultra_amd.query_exec.segment: expected contiguous GPU tensors; there is no CPU path "
                               "(run_reference is the restatement)")
    dtype = _lib.F32 if stack.dtype == torch.float32 else (_lib.F64 if stack.dtype == torch.float64 else -1)
    base = words.data_ptr() + 4 * offset
    total_ops_at = base + 4 * (3 * batch)
    _lib.check(_lib.lib.ultra_query_segment(
        base, base + 4 * batch, base + 8 * batch, total_ops_at, total_ops_at + 4 * (batch + 1), batch, num_nodes,
        stack.shape[1] if stack.dim() == 3 else -1, dtype, LOGIC_CODES[logic], _lib.ptr(stack), _lib.ptr(push_src),
        rows(push_src), _lib.ptr(pop_dst), rows(pop_dst), _lib.ptr(sym_stack), _lib.ptr(sym_push_src), _lib.ptr(sym_pop_dst),
        _lib.stream_of(stack)))


def nonzero_lists(x, num_live=None, retired=None):
    """(ptr (batch + 1) int64, index int64): per row of x (batch, n) fp32 on the GPU the ids v with x[b, v] != 0, ascending
    (NaN counts, -0.0 does not).  `index` has room for batch * n ids; the first ptr[-1] are filled.  No host wait.
    num_live (rows of n SLOTS of which the first num_live are entities in use): ultra_nonzero_lists_live on the full rows -- no
    slice, no copy; a dead slot is never read.  One int64 on x's device is handed to the kernels as it is (they clamp it to
    [0, n]); an int is checked against [0, n] on the host and uploaded.  None: ultra_nonzero_lists.
    retired (the device bitmap of a graph that retired entities -- id v is bit v & 31 of word v >> 5, live.retired_words -- or
    the pair (bits, count) of LiveGraph.retired_operand): ultra_nonzero_lists_alive, the lists without those ids, with num_live
    or without it (every slot is below the bound).  The bitmap is read by the kernels, not on the host."""
    # (the operand's own rules first, against x as it is: they hold wherever x lives)
    retired = None if x.dim() != 2 else selection.retired_operand(retired, x.shape[1], x.device, bare=True)
    if not x.is_cuda:
        raise RuntimeError("ultra_amd.query_exec.nonzero_lists: expected a GPU tensor; the MI355X engine has no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError("nonzero_lists takes a (batch, n) fp32 matrix, got %s %s" % (tuple(x.shape), x.dtype))
    x = x.contiguous()
    batch, n = x.shape
    ptr = torch.empty(batch + 1, dtype=torch.int64, device=x.device)
    index = torch.empty(max(1, batch * n), dtype=torch.int64, device=x.device)
    counts = torch.empty(max(1, batch), dtype=torch.int64, device=x.device)
    # (an empty list is a list: the live count may be 0 here.  Referenced until the launch is enqueued)
    live = selection.live_operand(num_live, n, x.device, lowest=0, exact=True, whose="matrix's")
    selection.launch("ultra_nonzero_lists", (x.data_ptr(), batch, n, counts.data_ptr(), ptr.data_ptr(), index.data_ptr(), batch * n),
                     live, x.device, retired)
    return ptr, index


class Executor(object):
    """Runs programs on the GPU.  The stacks and projection input buffers are cached per (device, batch, num_nodes,
    symbolic); one call in flight per executor and stream."""

    def __init__(self):
        self._buffers = {}
        self._prog = {}

    def _get(self, dev, batch, n, symbolic):
        key = (str(dev), batch, n, symbolic)
        hit = self._buffers.get(key)
        if hit is None:
            count = 2 if symbolic else 1
            hit = ([torch.empty(batch, UltraQuery.stack_size, n, device=dev) for _ in range(count)],
                   [torch.empty(batch, n, device=dev) for _ in range(count)])
            self._buffers[key] = hit
        return hit

    def _upload(self, dev, program):
        host, rel_off, seg_off = program.packed()
        size = host.numel()
        buf = self._prog.get(str(dev))
        if buf is None or buf.numel() < size:
            buf = torch.empty(max(4096, 2 * size), dtype=torch.uint8, device=dev)
            self._prog[str(dev)] = buf
        # (a fresh pinned block per call: the host allocator hands it out again only after the copy below has run)
        stage = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        stage.copy_(host)
        buf[:size].copy_(stage, non_blocking=True)
        n_rel = sum(len(p.relations) for p in program.projections)
        return buf[:8 * n_rel].view(torch.int64), buf[8 * n_rel:size].view(torch.int32), rel_off, seg_off

    @torch.no_grad()
    def run(self, model, graph, program, symbolic_traversal=True, delta=None):
        """(prob, final symbolic set or None) of `program` through `model` (an UltraQuery in eval mode) on a CUDA graph.
        delta (rspmm.GraphDelta of `graph`): the same on delta.materialize(graph) -- see `projections`."""
        if model.training:
            raise ValueError("the compiled executor serves eval mode only: training keeps UltraQuery.execute, whose "
                             "traversal dropout draws per projection")
        if program.stack_size != UltraQuery.stack_size:
            raise ValueError("the device route takes stacks of depth %d" % UltraQuery.stack_size)
        if program.batch > MAX_BATCH:
            raise ValueError("the device route takes at most %d queries a batch" % MAX_BATCH)
        symbolic = bool(symbolic_traversal)
        dev = graph.edge_index.device
        batch, n, logic = program.batch, program.num_nodes, model.logic
        _logic(logic)
        count = 2 if symbolic else 1
        results = [torch.empty(batch, n, device=dev) for _ in range(count)]
        if batch == 0:
            return results[0], (results[1] if symbolic else None)
        stacks, inputs = self._get(dev, batch, n, symbolic)
        rel, words, rel_off, seg_off = self._upload(dev, program)
        project, project_symbolic = projections(model, graph, delta)
        outs = [None, None]
        last = len(program.segments) - 1
        for s in range(last + 1):
            targets = results if s == last else inputs
            segment(words, seg_off[s], batch, n, logic, stacks[0], outs[0], targets[0],
                    stacks[1] if symbolic else None, outs[1] if symbolic else None, targets[1] if symbolic else None)
            if s == last:
                break
            rows = len(program.projections[s].samples)
            r_index = rel[rel_off[s]:rel_off[s] + rows]
            outs[0] = self._output(project(inputs[0][:rows], r_index), inputs[0], rows, n)
            if symbolic:
                outs[1] = self._output(project_symbolic(inputs[1][:rows], r_index), inputs[1], rows, n)
        return results[0], (results[1] if symbolic else None)

    @staticmethod
    def _output(out, source, rows, n):
        if out.shape != (rows, n) or out.dtype != torch.float32:
            raise TypeError("a projection must return (%d, %d) fp32, got %s %s" % (rows, n, tuple(out.shape), out.dtype))
        out = out.contiguous()
        # (the next segment reads rows of `out` while it writes rows of `source`)
        if out.untyped_storage().data_ptr() == source.untyped_storage().data_ptr():
            out = out.clone()
        return out


_EXECUTOR = Executor()


def _on_gpu(model, graph):
    edge_index = getattr(graph, "edge_index", None)
    param = next(model.parameters(), None)
    return edge_index is not None and edge_index.is_cuda and (param is None or param.is_cuda)


def _takes_delta(module):
    try:
        return "delta" in inspect.signature(getattr(module, "forward", module)).parameters
    except (TypeError, ValueError):
        return False


def projections(model, graph, delta=None):
    """The two projection calls (h_prob, r_index) -> set of a run: model.model and model.symbolic_model on `graph`.  Without a
    delta, or with one that holds no edit, exactly `projection(graph, h_prob, r_index)`.  With an edited delta
    `projection(graph, h_prob, r_index, delta=delta)` -- the cached plan and CSR of `graph` with the touched rows fixed; a
    projection whose forward keeps the reference's three arguments offers `forward_delta(graph, h_prob, r_index, delta)`
    instead (RelationProjection) --, and `projection(delta.materialize(graph), h_prob, r_index)` on a CPU graph or where a
    projection offers neither."""
    def call(projection):
        if delta is None or not delta.edited:
            return lambda h, r: projection(graph, h, r)
        if graph.edge_index.is_cuda and _takes_delta(projection):
            return lambda h, r: projection(graph, h, r, delta=delta)
        if graph.edge_index.is_cuda and hasattr(projection, "forward_delta"):
            return lambda h, r: projection.forward_delta(graph, h, r, delta)
        return lambda h, r: projection(delta.materialize(graph), h, r)
    return call(model.model), call(model.symbolic_model)


def in_lockstep(program):
    """Does every projection of `program` cover all samples in ascending order -- row j of every projection is sample j?  True for
    a batch of queries of one structure (QueryPredictor._programs)."""
    every = list(range(program.batch))
    return all(list(p.samples) == every for p in program.projections)


def execute(model, graph, query_or_program, symbolic_traversal=True, executor=None, delta=None):
    """(logits (batch, num_nodes), final symbolic sets or None): `UltraQuery.forward` and the top of its symbolic stack,
    through the compiled program.  A CPU graph or model runs `run_reference` on the model's own projections.  delta
    (rspmm.GraphDelta of `graph`): the same on delta.materialize(graph) (`projections`).  delta an rspmm.AssumedFacts (DESIGN.md
    33): sample j on the materialised graph plus the facts it assumes -- the overlay names a sample by its row, so the program
    must be in lockstep (`in_lockstep`) and no larger than the overlay's batch_size, on the GPU; models.NotOnFusedPath otherwise
    (the caller runs query_predict.assume_reference's loop)."""
    program = _as_program(query_or_program, graph)
    if getattr(delta, "per_query_owned", False):
        if not _on_gpu(model, graph):
            raise models.NotOnFusedPath("an overlay of assumed facts is served on the GPU only")
        if not in_lockstep(program) or program.batch > delta.batch_size:
            raise models.NotOnFusedPath("an overlay of assumed facts names a sample by its row: every projection of the program "
                                        "must cover all %d samples in ascending order, at most %d of them"
                                        % (program.batch, delta.batch_size))
    if model.training:
        raise ValueError("the compiled executor serves eval mode only: training keeps UltraQuery.execute, whose traversal "
                         "dropout draws per projection")
    if _on_gpu(model, graph):
        prob, sym = (executor or _EXECUTOR).run(model, graph, program, symbolic_traversal, delta=delta)
    else:
        project, project_symbolic = projections(model, graph, delta)
        with torch.no_grad():
            prob, sym = run_reference(program, model.logic, project, project_symbolic if symbolic_traversal else None,
                                      device=graph.edge_index.device)
    return logit(prob), sym


def forward(model, graph, query_or_program, symbolic_traversal=True, delta=None):
    """`UltraQuery.forward(graph, query, symbolic_traversal)` through the compiled program: the same logits, bit for bit.
    delta: as in `execute`."""
    return execute(model, graph, query_or_program, symbolic_traversal, delta=delta)[0]
