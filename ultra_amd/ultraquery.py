"""UltraQuery -- complex logical query answering on the propagation engine (reference: ultra/ultraquery.py,
ultra/query_utils.py:13-236).

A query is a postfix program over entities and relations (`Query`, the reference's bit flags).  `UltraQuery.execute` runs
a batch of such programs with a batched stack of (batch, num_nodes) fuzzy sets: operands push one-hot sets, intersection,
union and negation combine them under a fuzzy logic, and every relation projection is one `RelationProjection` call, that
is one `Ultra(RelNBFNet, QueryNBFNet)` forward on the HIP engine.  The stack machine stays in torch, as in the reference:
it is control flow over whole fuzzy sets.  `SymbolicTraversal` (the exact, neural-free projection the reference runs next
to the neural one) is one call of ultra_symbolic_traversal (csrc/query_kernels.hip) over a CSR keyed by (tail, relation)
that is built once per graph and cached.  In train() mode every projection first drops edges (traversal dropout,
query_train.traversal_dropout: keep vectors over the static graphs, read through their cached plans).  DESIGN.md section 10.
"""
import copy
import ctypes
from collections import OrderedDict, namedtuple

import torch
from torch import nn

from ._lib import check, lib, stream_of


class Query(torch.Tensor):
    """Tensor storage of logical queries in postfix notation (query_utils.py:13-196): an operand is an entity or relation
    id, an operation carries one of the flag bits below in its high bits."""

    projection = 1 << 58
    intersection = 1 << 59
    union = 1 << 60
    negation = 1 << 61
    stop = 1 << 62
    operation = projection | intersection | union | negation | stop

    stack_size = 2

    def __new__(cls, data, device=None):
        query = torch.as_tensor(data, dtype=torch.long, device=device)
        return torch.Tensor._make_subclass(cls, query)

    @classmethod
    def from_nested(cls, nested, binary_op=True):
        """A query from BetaE nested tuples, e.g. ((e1, (r1,)), (e2, (r2,))) for 2i, terminated by `stop`."""
        if not binary_op:
            raise ValueError("Query.from_nested encodes binary intersections and unions only (binary_op=True)")
        return cls(cls.nested_to_postfix(nested) + [cls.stop])

    @classmethod
    def nested_to_postfix(cls, nested, binary_op=True):
        """BetaE nested tuples -> postfix list.  A pair (anchor, (op, ...)) whose op tuple holds ints is a chain applied to
        the anchor (an entity, or a nested query): -2 negates, any other op projects along that relation.  Any other tuple
        combines its branches pairwise, left to right: a union when it ends with the one-element marker (-1,), else an
        intersection.  Every intersection / union carries its arity 2 as operand."""
        if len(nested) == 2 and isinstance(nested[1][-1], int):
            anchor, chain = nested
            out = cls.nested_to_postfix(anchor) if isinstance(anchor, tuple) else [anchor]
            return out + [cls.negation if step == -2 else cls.projection | step for step in chain]
        is_union = len(nested[-1]) == 1
        branches = nested[:-1] if is_union else nested
        combine = (cls.union if is_union else cls.intersection) | 2
        out = cls.nested_to_postfix(branches[0])
        for branch in branches[1:]:
            out += cls.nested_to_postfix(branch) + [combine]
        return out

    def to_readable(self):
        """One query as lines `A <- projection_3(17)`, ..."""
        if self.ndim > 1:
            raise ValueError("readable() can only be called for a single query")
        num_variable = 0
        stack, lines = [], []
        for op in self.tolist():
            op = Query(op)
            if op.is_operand():
                stack.append(str(int(op.get_operand())))
                continue
            if op.is_stop():
                break
            var = chr(ord("A") + num_variable)
            if op.is_projection():
                line = "%s <- projection_%d(%s)" % (var, int(op.get_operand()), stack.pop())
            elif op.is_intersection() or op.is_union():
                num_args = int(op.get_operand())
                args, stack = stack[-num_args:], stack[:-num_args]
                line = "%s <- %s(%s)" % (var, "intersection" if op.is_intersection() else "union", ", ".join(args))
            elif op.is_negation():
                line = "%s <- negation(%s)" % (var, stack.pop())
            else:
                raise ValueError("Unknown operator `%d`" % int(op))
            lines.append(line)
            stack.append(var)
            num_variable += 1
        if len(stack) > 1:
            raise ValueError("Invalid query. More operands than expected")
        return "\n".join(lines)

    def _has(self, flags):
        return (self & flags) != 0

    def is_operation(self):
        return self._has(self.operation)

    def is_operand(self):
        return ~self._has(self.operation)

    def is_projection(self):
        return self._has(self.projection)

    def is_intersection(self):
        return self._has(self.intersection)

    def is_union(self):
        return self._has(self.union)

    def is_negation(self):
        return self._has(self.negation)

    def is_stop(self):
        return self._has(self.stop)

    def get_operation(self):
        """The flag bits of every entry (0 for operands)."""
        return self & self.operation

    def get_operand(self):
        """Every entry without its flag bits: entity id, relation id, or arity."""
        return self & ~self.operation

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


class Stack(object):
    """One fixed-depth stack per sample of a batch (query_utils.py:198-236): `stack` holds (batch, stack_size, *shape)
    values, `SP` the number of filled slots per sample.  push / pop act on the samples selected by a boolean mask."""

    def __init__(self, batch_size, stack_size, *shape, dtype=None, device=None):
        self.batch_size, self.stack_size = batch_size, stack_size
        self.stack = torch.zeros((batch_size, stack_size) + tuple(shape), dtype=dtype, device=device)
        self.SP = torch.zeros(batch_size, dtype=torch.long, device=device)

    def _select(self, mask):
        return torch.ones(self.batch_size, dtype=torch.bool, device=self.SP.device) if mask is None else mask

    def push(self, mask, value):
        depth = self.SP[mask]
        if bool((depth >= self.stack_size).any()):
            raise ValueError("Stack overflow: a selected sample already holds %d values" % self.stack_size)
        self.stack[mask, depth] = value
        self.SP[mask] = depth + 1

    def pop(self, mask=None):
        mask = self._select(mask)
        depth = self.SP[mask]
        if bool((depth <= 0).any()):
            raise ValueError("Stack underflow: a selected sample holds no value")
        self.SP[mask] = depth - 1
        return self.stack[mask, depth - 1]

    def top(self, mask=None):
        if bool((self.SP <= 0).any()):
            raise ValueError("Stack is empty")
        mask = self._select(mask)
        return self.stack[mask, self.SP[mask] - 1]


# fuzzy logics: (conjunction, disjunction) on fuzzy sets in [0, 1]; negation is 1 - x in all three
_LOGICS = {
    "product": (lambda x, y: x * y, lambda x, y: x + y - x * y),
    "godel": (torch.min, torch.max),
    "lukasiewicz": (lambda x, y: (x + y - 1).clamp(min=0), lambda x, y: (x + y).clamp(max=1)),
}


def _logic(name):
    if name not in _LOGICS:
        raise ValueError("Unknown fuzzy logic `%s`: one of %s" % (name, ", ".join(sorted(_LOGICS))))
    return _LOGICS[name]


class UltraQuery(nn.Module):
    """Query executor for multi-hop logical queries (ultraquery.py:12-243).

    model: an `Ultra` whose entity model is a `QueryNBFNet`; logic: ``product``, ``godel`` or ``lukasiewicz``;
    dropout_ratio / more_dropout: traversal dropout ratios of training (train() mode, on the GPU); threshold: the projection's score threshold.  The submodules are named as the reference's, so the
    state_dict of ultraquery.pth (`model.model.relation_model...`) loads with strict=True.
    """

    stack_size = 2

    def __init__(self, model, logic="product", dropout_ratio=0.25, threshold=0.0, more_dropout=0.0):
        super(UltraQuery, self).__init__()
        self.model = RelationProjection(model, threshold)
        self.symbolic_model = SymbolicTraversal()
        self.logic = logic
        self.dropout_ratio = dropout_ratio
        self.more_dropout = more_dropout

    def execute(self, graph, query, symbolic_traversal):
        if self.training:
            # the reference's training execution (ultraquery.py:96-98, 199-224): traversal dropout needs the symbolic sets,
            # and runs on the GPU only (query_train: keep vectors over the static graphs' cached plans)
            edge_index = getattr(graph, "edge_index", None)
            if edge_index is None or not edge_index.is_cuda:
                raise NotImplementedError(
                    "UltraQuery trains on the GPU only: traversal dropout (ultraquery.py:33-84) is a HIP kernel; pass the "
                    "graph on a CUDA device")
            if symbolic_traversal is not True:
                raise ValueError("symbolic_traversal is needed at train time for dropout")
        self.symbolic_traversal = symbolic_traversal
        query = query if isinstance(query, Query) else Query(query)
        batch_size = len(query)
        self.stack = Stack(batch_size, self.stack_size, graph.num_nodes, device=query.device)
        self.var = Stack(batch_size, query.shape[1], graph.num_nodes, device=query.device)
        if self.symbolic_traversal:
            self.symbolic_stack = Stack(batch_size, self.stack_size, graph.num_nodes, device=query.device)
            self.symbolic_var = Stack(batch_size, query.shape[1], graph.num_nodes, device=query.device)

        # instruction pointer
        self.IP = torch.zeros(batch_size, dtype=torch.long, device=query.device)
        all_sample = torch.ones(batch_size, dtype=torch.bool, device=query.device)
        op = query[all_sample, self.IP]

        while not op.is_stop().all():
            is_operand = op.is_operand()
            is_intersection = op.is_intersection()
            is_union = op.is_union()
            is_negation = op.is_negation()
            is_projection = op.is_projection()
            if is_operand.any():
                self.apply_operand(is_operand, op[is_operand].get_operand(), graph.num_nodes)
            if is_intersection.any():
                self.apply_intersection(is_intersection)
            if is_union.any():
                self.apply_union(is_union)
            if is_negation.any():
                self.apply_negation(is_negation)
            # projections only when no other operation is pending: they are the expensive step, and this batches as many
            # samples into one projection as possible
            if not (is_operand | is_negation | is_intersection | is_union).any() and is_projection.any():
                self.apply_projection(is_projection, graph, op[is_projection].get_operand())
            op = query[all_sample, self.IP]

        if (self.stack.SP > 1).any():
            raise ValueError("More operands than expected")

    def forward(self, graph, query, symbolic_traversal=True):
        """(batch, num_nodes) logits of the answer set of every query: log((p + 1e-10) / (1 - p + 1e-10))."""
        self.execute(graph, query, symbolic_traversal)
        t_prob = self.stack.pop()
        return ((t_prob + 1e-10) / (1 - t_prob + 1e-10)).log()

    def apply_operand(self, mask, h_index, num_node):
        h_prob = torch.nn.functional.one_hot(h_index.as_subclass(torch.Tensor), num_node).float()
        self._push(mask, h_prob, h_prob)
        self.IP[mask] += 1

    def apply_intersection(self, mask):
        self._binary(mask, self.conjunction)

    def apply_union(self, mask):
        self._binary(mask, self.disjunction)

    def apply_negation(self, mask):
        x_prob = self.stack.pop(mask)
        sym = self.negation(self.symbolic_stack.pop(mask)) if self.symbolic_traversal else None
        self._push(mask, self.negation(x_prob), sym)
        self.IP[mask] += 1

    def apply_projection(self, mask, graph, r_index):
        r_index = r_index.as_subclass(torch.Tensor)
        h_prob = self.stack.pop(mask).detach()
        sym_h_prob = self.symbolic_stack.pop(mask) if self.symbolic_traversal else None
        if self.training:
            # traversal dropout (ultraquery.py:34-83, 202-206) as keep vectors: over the entity graph's edges from the symbolic
            # sets, and over the relation graph's edges for the relation graph of the dropped graph
            from . import query_train, rspmm
            keep = query_train.traversal_dropout(graph.edge_index, graph.edge_type, graph.num_nodes, graph.num_relations,
                                                 sym_h_prob, r_index, self.dropout_ratio, self.more_dropout,
                                                 getattr(graph, "inverse_rel_plus_one", False))
            rel_keep = query_train.relation_graph_keep(graph, keep)
            # the dropped graph is the same graph object with its keep vectors attached (the reference's filtered copy,
            # ultraquery.py:79-83): every plan and CSR of the static graphs stays cached
            graph = copy.copy(graph)
            graph.traversal_keep = rspmm.tag_edge_weight(keep)
            graph.relation_keep = rspmm.tag_edge_weight(rel_keep)
        t_prob = self.model(graph, h_prob, r_index)
        sym = self.symbolic_model(graph, sym_h_prob, r_index) if self.symbolic_traversal else None
        self._push(mask, t_prob, sym)
        self.IP[mask] += 1

    def _binary(self, mask, fn):
        y_prob = self.stack.pop(mask)
        x_prob = self.stack.pop(mask)
        sym = None
        if self.symbolic_traversal:
            sym_y = self.symbolic_stack.pop(mask)
            sym_x = self.symbolic_stack.pop(mask)
            sym = fn(sym_x, sym_y)
        self._push(mask, fn(x_prob, y_prob), sym)
        self.IP[mask] += 1

    def _push(self, mask, value, symbolic_value):
        self.stack.push(mask, value)
        self.var.push(mask, value)
        if self.symbolic_traversal:
            self.symbolic_stack.push(mask, symbolic_value)
            self.symbolic_var.push(mask, symbolic_value)

    def conjunction(self, x, y):
        return _logic(self.logic)[0](x, y)

    def disjunction(self, x, y):
        return _logic(self.logic)[1](x, y)

    def negation(self, x):
        return 1 - x


class RelationProjection(nn.Module):
    """One projection step (ultraquery.py:245-277): a fuzzy set of head entities `h_prob` (batch, num_nodes) and one query
    relation per sample become a fuzzy set of tail entities.  `model` is an `Ultra` whose entity model is a `QueryNBFNet`."""

    def __init__(self, model, threshold=0.0):
        super(RelationProjection, self).__init__()
        self.model = model
        self.threshold = threshold

    def forward(self, graph, h_prob, r_index):
        # (the reference's interface, ultraquery.py:245-277, pinned by tests/test_models_cpu.py: a graph delta comes in through
        # forward_delta)
        return self._project(graph, h_prob, r_index, None)

    def forward_delta(self, graph, h_prob, r_index, delta=None):
        """forward on a CHANGING graph (serving): the projection on delta.materialize(graph) -- the relation model
        on the delta's relation graph (delta.live_view), the entity model on graph's cached plan with the touched rows fixed
        (QueryNBFNet.forward(delta=), which falls back to the materialised graph by itself).  delta None or without edits:
        forward.  ValueError in training mode or with traversal_keep / relation_keep on the graph."""
        return self._project(graph, h_prob, r_index, delta)

    def _project(self, graph, h_prob, r_index, delta):
        # (training) graph.traversal_keep / graph.relation_keep: 0/1 vectors over the edges of the entity graph and of its
        # relation graph -- the projection then runs on the graph without the zero edges (traversal dropout)
        edge_keep = getattr(graph, "traversal_keep", None)
        relation_keep = getattr(graph, "relation_keep", None)
        if delta is not None and not delta.edited:
            delta = None
        if delta is not None:
            if self.training or edge_keep is not None or relation_keep is not None:
                raise ValueError("a graph delta serves eval mode only, without traversal_keep / relation_keep on the graph")
            graph = delta.live_view(graph)
        bs = r_index.shape[0]
        # relation representations conditioned on the query relations, (bs, num_rel, dim)  (ultraquery.py:258)
        if relation_keep is not None:
            rel_reprs = self.model.relation_model(graph.relation_graph, query=r_index, edge_keep=relation_keep)
        else:
            rel_reprs = self.model.relation_model(graph.relation_graph, query=r_index)
        query = rel_reprs[torch.arange(bs, device=r_index.device), r_index]            # (bs, dim)
        # initial node features: the fuzzy set scaled query vector (ultraquery.py:262); scores at or below the threshold
        # are cut off first (ultraquery.py:266-270: alleviates multi-source propagation)
        prob = h_prob
        if self.threshold > 0.0:
            prob = torch.where(h_prob <= self.threshold, torch.zeros_like(h_prob), h_prob)
        input = prob.unsqueeze(-1) * query.unsqueeze(1)                                # einsum("bn, bd -> bnd")
        if delta is not None:
            output = self.model.entity_model(graph, input, rel_reprs, query, delta=delta)
        elif edge_keep is not None:
            output = self.model.entity_model(graph, input, rel_reprs, query, edge_keep=edge_keep)
        else:
            output = self.model.entity_model(graph, input, rel_reprs, query)           # (bs, num_nodes) scores
        return torch.sigmoid(output)


TraversalCSR = namedtuple("TraversalCSR", "row_ptr src type num_node num_edge")

_CSR_CACHE = OrderedDict()
_CSR_CACHE_SIZE = 8


def traversal_csr(edge_index, edge_type, num_node):
    """The CSR of a graph keyed by (tail, relation), cached like explain.beam_csr: row v holds the in-edges of v sorted by
    relation (a stable sort of the key tail * R + relation on the device)."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
           edge_type.data_ptr(), edge_type._version, str(edge_index.device), int(num_node))
    hit = _CSR_CACHE.get(key)
    if hit is not None:
        _CSR_CACHE.move_to_end(key)
        return hit[0]
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.shape != (edge_index.shape[1],):
        raise ValueError("Expected `edge_index` of shape (2, num_edge) and `edge_type` of shape (num_edge,)")
    if not edge_index.is_cuda:
        raise RuntimeError("the symbolic traversal runs on the GPU: pass the graph on a CUDA device")
    num_edge = edge_index.shape[1]
    if num_node <= 0 or num_node >= 2 ** 31 or num_edge >= 2 ** 31:
        raise ValueError("the symbolic traversal takes 0 < num_node < 2^31 and num_edge < 2^31")
    if num_edge and (int(edge_index.min()) < 0 or int(edge_index.max()) >= num_node or int(edge_type.min()) < 0
                     or int(edge_type.max()) >= 2 ** 31):
        raise ValueError("edge_index holds node ids outside [0, num_node) or edge_type negative relations")
    src, dst = edge_index[0], edge_index[1]
    num_rel = int(edge_type.max()) + 1 if num_edge else 1
    order = torch.sort(dst * num_rel + edge_type, stable=True).indices
    deg = torch.bincount(dst, minlength=num_node)
    row_ptr = torch.zeros(num_node + 1, dtype=torch.int64, device=dst.device)
    torch.cumsum(deg, 0, out=row_ptr[1:])
    csr = TraversalCSR(row_ptr, src[order].to(torch.int32).contiguous(), edge_type[order].to(torch.int32).contiguous(),
                       int(num_node), int(num_edge))
    _CSR_CACHE[key] = (csr, edge_index, edge_type)     # (the tensors stay alive with the entry: no recycled data_ptr aliases it)
    while len(_CSR_CACHE) > _CSR_CACHE_SIZE:
        _CSR_CACHE.popitem(last=False)
    return csr


def clear_csr_cache():
    _CSR_CACHE.clear()
    _ORDER_CACHE.clear()


_ORDER_CACHE = OrderedDict()


def traversal_order(edge_index, edge_type, num_node):
    """The edge id of every slot of traversal_csr (the same stable sort), cached alike: training maps its keep vectors
    into slot order with it."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
           edge_type.data_ptr(), edge_type._version, str(edge_index.device), int(num_node))
    hit = _ORDER_CACHE.get(key)
    if hit is not None:
        _ORDER_CACHE.move_to_end(key)
        return hit[0]
    num_rel = int(edge_type.max()) + 1 if edge_type.numel() else 1
    order = torch.sort(edge_index[1] * num_rel + edge_type, stable=True).indices
    _ORDER_CACHE[key] = (order, edge_index, edge_type)
    while len(_ORDER_CACHE) > _CSR_CACHE_SIZE:
        _ORDER_CACHE.popitem(last=False)
    return order


def symbolic_traversal(edge_index, edge_type, num_node, h_prob, r_index, edge_keep=None, delta=None):
    """t[b, v] = max(0, max{h[b, u] : edge u -> v of type r_index[b]}) on the GPU (ultra_symbolic_traversal); with
    edge_keep (num_edge, 0/1) over the edges whose keep is not 0 only (ultra_symbolic_traversal_keep).  delta (an edited
    rspmm.GraphDelta whose base graph the edge list is; not with edge_keep): the traversal of delta.materialize(...) -- the base
    launch on the cached CSR of the base graph, then one launch that recomputes the tails an added or a removed edge points
    into (ultra_symbolic_traversal_edit_rows).  The same bits: a max has no order.  delta an rspmm.AssumedFacts
    (`per_query_owned`): row b is the traversal of the materialised graph plus the facts sample b assumes
    (ultra_symbolic_traversal_edit_rows_owned) -- row b is sample b, at most the overlay's batch_size rows."""
    if delta is not None and not delta.edited:
        delta = None
    if delta is not None:
        if edge_keep is not None:
            raise ValueError("a graph delta is not combined with edge_keep")
        if delta.num_nodes != int(num_node) or delta.device != edge_index.device:
            raise ValueError("the delta was made for a graph of %d nodes on %s, the traversal runs over %d nodes on %s"
                             % (delta.num_nodes, delta.device, num_node, edge_index.device))
        if getattr(delta, "per_query_owned", False) and h_prob.shape[0] > delta.batch_size:
            raise ValueError("the overlay of assumed facts was laid out for %d samples, the traversal has %d rows"
                             % (delta.batch_size, h_prob.shape[0]))
    if h_prob.dtype not in (torch.float32, torch.float64):
        raise TypeError("the symbolic traversal takes fp32 or fp64 fuzzy sets, got %s" % h_prob.dtype)
    if h_prob.dim() != 2 or h_prob.shape[1] != num_node or r_index.shape != (h_prob.shape[0],):
        raise ValueError("Expected h_prob (batch, %d) and r_index (batch,), got %s and %s"
                         % (num_node, tuple(h_prob.shape), tuple(r_index.shape)))
    csr = traversal_csr(edge_index, edge_type, num_node)
    if not (h_prob.is_cuda and h_prob.device == csr.row_ptr.device == r_index.device):
        raise RuntimeError("fuzzy sets, relations and graph must be on one CUDA device")
    h = h_prob.contiguous()
    r = r_index.to(torch.int64).contiguous()
    t = torch.empty_like(h)
    stream = stream_of(h)
    if edge_keep is not None:
        # the keep vector in the CSR's slot order
        keep_slot = edge_keep.to(torch.float32)[traversal_order(edge_index, edge_type, num_node)].contiguous()
        check(lib.ultra_symbolic_traversal_keep(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(),
                                                keep_slot.data_ptr(), csr.num_node, r.data_ptr(), h.shape[0],
                                                0 if h.dtype == torch.float32 else 1, h.data_ptr(), t.data_ptr(), stream))
        return t
    check(lib.ultra_symbolic_traversal(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), csr.num_node,
                                       r.data_ptr(), h.shape[0], 0 if h.dtype == torch.float32 else 1, h.data_ptr(),
                                       t.data_ptr(), stream))
    if delta is not None and getattr(delta, "per_query_owned", False):
        # facts assumed per sample (rspmm.AssumedFacts): row b sees the delta's edges and sample b's own
        edits, owner = delta.traversal_operand(), delta.traversal_owner
        check(lib.ultra_symbolic_traversal_edit_rows_owned(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(),
                                                           csr.num_node, ctypes.byref(edits), owner.data_ptr(), r.data_ptr(),
                                                           h.shape[0], 0 if h.dtype == torch.float32 else 1, h.data_ptr(),
                                                           t.data_ptr(), stream))
    elif delta is not None:
        edits = delta.traversal_operand()
        check(lib.ultra_symbolic_traversal_edit_rows(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(),
                                                     csr.num_node, ctypes.byref(edits), r.data_ptr(), h.shape[0],
                                                     0 if h.dtype == torch.float32 else 1, h.data_ptr(), t.data_ptr(), stream))
    return t


def symbolic_traversal_reference(edge_index, edge_type, num_node, h_prob, r_index):
    """The torch restatement of the reference's SymbolicTraversal (ultraquery.py:280-298): the (batch, num_edge) relation
    mask, a max-scatter of h[b, src] into the edge tails with torch_scatter's zero for empty rows, clamp(min=0)."""
    bs = h_prob.shape[0]
    mask = edge_type.unsqueeze(0) == r_index.unsqueeze(1)                  # (bs, E)
    sample, edge = mask.nonzero().t()
    src, dst = edge_index[0, edge], edge_index[1, edge]
    value = h_prob[sample, src]
    out = torch.zeros(bs * num_node, dtype=h_prob.dtype, device=h_prob.device)
    out = out.scatter_reduce(0, sample * num_node + dst, value, reduce="amax", include_self=False)
    return out.view(bs, num_node).clamp(min=0)


class SymbolicTraversal(nn.Module):
    """Symbolic traversal (ultraquery.py:280-298): the exact projection of a fuzzy set along one relation per sample."""

    def forward(self, graph, h_prob, r_index, delta=None):
        """delta (rspmm.GraphDelta of `graph`, serving): the traversal of delta.materialize(graph) on graph's cached CSR."""
        return symbolic_traversal(graph.edge_index, graph.edge_type, graph.num_nodes, h_prob, r_index,
                                  edge_keep=getattr(graph, "traversal_keep", None), delta=delta)
