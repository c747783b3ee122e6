"""Drop-in operator boundary: generalized_rspmm and the RSPMM*Function classes.

Mirrors /root/reference/ultra/rspmm/rspmm.py (names, argument meaning, error behaviour):
  * generalized_rspmm(edge_index, edge_type, edge_weight, relation, input, sum="add", mul="mul")
    (rspmm.py:168-179) -- accepts unsorted edges, ValueError for unknown (sum, mul) pairs;
  * RSPMM{Add,Min,Max}{Mul,Add}Function (rspmm.py:12-165) -- require sorted `edge_index`
    (AssertionError "Expect sorted `edge_index`"), differentiable w.r.t. edge_weight, relation, input;
  * `rspmm` -- a namespace exporting the reference extension's function names
    rspmm_<sum>_<mul>_{forward,backward}_cuda (rspmm.cpp:270-282), bound to the stateless C entry points.

Beyond the reference: mul="rotate" (ULTRA_MUL_ROTATE, include/ultra_rspmm.h) -- the RotatE message of the reference LAYER
(layers.py:142-147) as an rspmm operator: a row is one complex vector, real half | imaginary half.  `Plan.forward` /
`Plan.backward` / `plan_rspmm` / `generalized_rspmm` take it and RSPMM{Add,Min,Max}RotateFunction exist; the `rspmm`
namespace of reference exports does not grow.  In the 2-D (N, D) layout the whole row is ONE complex vector: batched
callers pass batch-major (batch, N, d) operands.

What changes underneath: the per-call argsort / ind2ptr / host syncs of the reference are replaced by a
cached `Plan` (built once per graph) and the HIP kernels of libultra_amd.so.  CPU tensors raise: this
engine has no CPU path (the reference's `rspmm_*_cpu` names exist only to say so).
"""
import copy
import ctypes
import sys
from collections import OrderedDict, namedtuple

import torch
from torch import autograd

from . import _lib, tasks
from .data import Data
from ._lib import UltraMat, check, lib, ptr, stream_of

module = sys.modules[__name__]

_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}


_WEIGHT_EPOCH = [0]
# the relation gradient of dense-twin graphs on the matrix cores (A/B switch for tests: the relation-major edge walk is the other side)
DENSE_RELATION_GRAD = True
# the touched rows of a graph delta through ultra_rspmm_edit_rows_split: a row longer than the plan's seg_len is recomputed by a
# workgroup, not by one 16-lane chain (A/B switch for tests: delta_rows / edit_rows / edit_rows_samples are the other side)
EDIT_ROWS_HUB_SPLIT = True


def tag_edge_weight(edge_weight):
    """Marks a per-step edge-weight vector (a training step's 0/1 keep mask) as unchanged from here on: the plans then bring
    it into their edge order once per step instead of once per rspmm call (ultra_rspmm_weight_epoch).  An in-place write
    to the tensor voids the tag."""
    _WEIGHT_EPOCH[0] += 1
    edge_weight._ultra_epoch = (_WEIGHT_EPOCH[0], edge_weight._version)
    return edge_weight


def _weight_epoch(edge_weight):
    tag = getattr(edge_weight, "_ultra_epoch", None) if edge_weight is not None else None
    return tag[0] if tag is not None and tag[1] == edge_weight._version else 0


def _announce_weight(edge_weight, epoch=None):
    """Tells the library which tagged vector the next weighted call carries (0: untagged)."""
    if edge_weight is not None:
        lib.ultra_rspmm_weight_epoch(int(_weight_epoch(edge_weight) if epoch is None else epoch))


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("ultra_amd.rspmm: expected a GPU (ROCm `cuda`) tensor, got device `%s`; "
                               "the MI355X engine has no CPU path" % t.device)


def _dtype_code(*tensors):
    dt = tensors[0].dtype
    for t in tensors:
        if t.dtype != dt:
            raise RuntimeError("Expected tensors of the same floating type (edge_weight, relation, input), got %s and %s"
                               % (dt, t.dtype))  # checkAllSameType, rspmm.cpp:23
    if dt not in _DTYPES:
        raise RuntimeError("rspmm supports float32 / float64, got %s" % dt)  # AT_DISPATCH_FLOATING_TYPES
    return _DTYPES[dt]


def as_mat(t):
    """Describe a 2-D (rows, D) or batch-major 3-D (batch, rows, d) tensor to the C ABI without copying."""
    if t.dim() == 2:
        if t.stride(1) != 1 and t.shape[1] > 1:
            t = t.contiguous()
        return t, UltraMat(t.data_ptr(), 1, 0, t.shape[0], t.stride(0), t.shape[1])
    if t.dim() == 3:
        if t.stride(2) != 1 and t.shape[2] > 1:
            t = t.contiguous()
        return t, UltraMat(t.data_ptr(), t.shape[0], t.stride(0), t.shape[1], t.stride(1), t.shape[2])
    raise RuntimeError("Expected a 2-dimensional (or batch-major 3-dimensional) tensor, got %d dims" % t.dim())


def _opt_mat(t):
    """An optional matrix operand: (the tensor as_mat describes -- hold it until the launch is enqueued --, byref of its
    UltraMat), or (None, None)."""
    if t is None:
        return None, None
    t, m = as_mat(t)
    return t, ctypes.byref(m)


def _point_operand(point, input):
    """The point boundary (rows, values) of a 2-D or batch-major 3-D `input` as the entry points take it: (int64 rows, values
    as one row per outer slice, the rows' pointer, byref of the values' UltraMat).  The caller holds the two tensors (and
    checks their device)."""
    rows, vals = point
    n_outer = 1 if input.dim() == 2 else input.shape[0]
    rows = rows.to(torch.int64).contiguous()
    if rows.numel() != n_outer:
        raise RuntimeError("Expected one boundary row per outer slice (%d), got %d" % (n_outer, rows.numel()))
    vals, mv = as_mat(vals.reshape(n_outer, 1, vals.shape[-1]) if input.dim() == 3 else vals.reshape(1, vals.shape[-1]))
    return rows, vals, rows.data_ptr(), ctypes.byref(mv)


def _weight_operand(edge_weight, num_edge, weight_epoch=None):
    """The edge-weight operand: (the contiguous vector, its pointer, its epoch -- the caller's, else the tag of a vector
    that is passed on as it is, else 0), or (None, None, weight_epoch)."""
    if edge_weight is None:
        return None, None, weight_epoch
    if edge_weight.dim() != 1 or edge_weight.shape[0] != num_edge:
        raise RuntimeError("Expected `edge_weight` of shape (num_edge,)")
    if weight_epoch is None:
        weight_epoch = _weight_epoch(edge_weight) if edge_weight.is_contiguous() else 0
    edge_weight = edge_weight.contiguous()
    return edge_weight, edge_weight.data_ptr(), weight_epoch


def _out_like(input, num_node):
    """A fresh output of `num_node` rows, shaped like the input otherwise."""
    shape = list(input.shape)
    shape[-2] = num_node
    return torch.empty(shape, dtype=input.dtype, device=input.device)


# A forward launch's operands as the entry points take them: the dtype code, the edge-weight pointer (or None) and its epoch,
# byrefs of relation and input, the boundary's byref (the point's values where a point is given, else the dense boundary or
# None), the point's rows pointer (or None), the output and its byref, and `held`: the tensors behind the pointers, which
# live as long as this tuple -- keep it until the launch is enqueued.
_ForwardOperands = namedtuple("_ForwardOperands", "dtype weight epoch relation input boundary rows out out_ref held")


class Plan(object):
    """Aggregation plan of one graph (sorted CSR + balanced work list), resident in HBM."""

    TYPE_RUN_MIN_MEAN_LENGTH = 16   # build the type-run twin when (row, type) runs average at least this many edges
    DENSE_MIN_FILL = 0.25           # build the dense-format twin when this share of the (row, type, col) cells holds an edge

    def __init__(self, edge_index, edge_type, num_node, num_relation, seg_len=0, g_max=0, exact_order=False,
                 num_in=None, type_runs="auto", dense="auto"):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise RuntimeError("Expected `edge_index` of shape (2, num_edge)")          # checkDim/checkSize
        if edge_type.dim() != 1 or edge_type.shape[0] != edge_index.shape[1]:
            raise RuntimeError("Expected `edge_type` of shape (num_edge,)")
        if edge_index.dtype != edge_type.dtype:
            raise RuntimeError("Expected `edge_index` and `edge_type` of the same type")  # checkSameType, rspmm.cpp:22
        ei = edge_index.detach().to("cpu", torch.int64).contiguous()
        et = edge_type.detach().to("cpu", torch.int64).contiguous()
        flags = ((_lib.PLAN_EXACT_ORDER if exact_order else 0) | (_lib.PLAN_TYPE_RUNS if type_runs == "only" else 0)
                 | (_lib.PLAN_DENSE if dense == "only" else 0))
        opts = _lib.PlanOpts(int(seg_len), int(g_max), flags, 0)
        handle = ctypes.c_void_p()
        self.num_edge = ei.shape[1]
        self.num_node = int(num_node)
        self.num_in = int(num_node if num_in is None else num_in)
        self.num_relation = int(num_relation)
        check(lib.ultra_plan_create(ctypes.byref(handle), ei.data_ptr(), et.data_ptr(), self.num_edge, self.num_node,
                                    self.num_in, self.num_relation, ctypes.byref(opts)))
        self._h = handle
        self.exact = bool(exact_order)
        self._has_hub_rows = None
        # Dense graphs with few relation types (ULTRA's relation graph: 474 nodes, 4 types, ~470 edges per
        # (row, type) run) get a twin plan whose items hold one relation each; add_mul forwards use it.
        self.typed = None
        self.dense = None
        self._edges = None
        self._dense_t = None
        if dense == "only" or type_runs == "only":
            return
        # (Nearly) complete graphs -- again ULTRA's relation graph -- also get a dense-format twin: fp32 add_mul with unit
        # edge weights then runs on the matrix cores (csrc/rspmm_dense.hip).
        cells = self.num_node * self.num_in * max(self.num_relation, 1)
        if dense in ("auto", True) and self.num_edge > 0 and self.num_in <= _lib.DENSE_MAX_IN_ROW \
                and cells <= (1 << 26) and (dense is True or self.num_edge >= self.DENSE_MIN_FILL * cells):
            try:
                self.dense = Plan(ei, et, num_node, num_relation, num_in=num_in, type_runs=False, dense="only")
                self._edges = (ei, et)      # (a few hundred nodes: kept for the transposed twin of the backward)
            except _lib.UltraError:     # an edge repeated more than 255 times: the edge walk serves it
                if dense is True:
                    raise
            # a reference-order plan only keeps the twin for the reference-order layer kernel (fused_layer), and only
            # when the graph qualifies for it (parallel edges sorted by type, no repeats, at most 4 types)
            if exact_order and self.dense is not None and self.dense.info()["dense_order_bytes"] == 0:
                self.dense = None
        if type_runs in ("auto", True) and not exact_order and self.num_edge > 0:
            runs = max(1, self.info()["n_type_run"])
            if type_runs is True or self.num_edge / runs >= self.TYPE_RUN_MIN_MEAN_LENGTH:
                self.typed = Plan(ei, et, num_node, num_relation, seg_len=seg_len, g_max=g_max, num_in=num_in,
                                  type_runs="only", dense=False)

    def _twin_for(self, sum, mul, edge_weight, input, *others):
        """The specialised twin plan that serves this call, or None for the general (row, col) plan."""
        if sum != "add" or mul != "mul" or self.exact:     # (the twins' kernels re-associate the sum)
            return None
        if self.dense is not None and edge_weight is None and input.dtype == torch.float32 \
                and input.shape[-1] % 32 == 0 and input.dim() in (2, 3) \
                and all(t is None or (t.stride(-1) == 1 and t.data_ptr() % 16 == 0
                                      and all(st % 4 == 0 for st in t.stride()[:-1])) for t in (input,) + others):
            return self.dense
        return self.typed

    def dense_transposed(self):
        """The dense-format plan of the TRANSPOSED graph (built on first use): the input gradient of add_mul,
        input_grad[col] = sum_e rel[type] * output_grad[row] (rspmm.cpp:110-112), is an rspmm forward over it."""
        if self._dense_t is None and self.dense is not None and self._edges is not None:
            ei, et = self._edges
            self._dense_t = Plan(ei.flip(0).contiguous(), et, self.num_in, self.num_relation, num_in=self.num_node,
                                 type_runs=False, dense="only")
        return self._dense_t

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:   # (module globals are gone at interpreter shutdown)
            try:
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
                lib.ultra_plan_destroy(h)
            except Exception:
                pass
            self._h = None

    def pin(self, delta=1):
        """A captured hipGraph starts (+1) / stops (-1) referencing this plan's device arrays (twins included)."""
        for p in (self, self.typed, self.dense, self._dense_t):
            if p is not None and getattr(p, "_h", None):
                check(lib.ultra_plan_pin(p._h, int(delta)))

    def info(self):
        info = _lib.PlanInfo()
        check(lib.ultra_plan_get_info(self._h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in _lib.PlanInfo._fields_}

    @property
    def has_hub_rows(self):
        """Does a row of this reference-order plan hold more than seg_len edges (a chain row of the base walk: n_chain_row)?
        Only such a row is a hub to edit_rows_split at its default hub_len; a plan without one gains nothing from it."""
        if self._has_hub_rows is None:
            self._has_hub_rows = self.exact and self.info()["n_chain_row"] > 0
        return self._has_hub_rows

    def schedule_info(self, nparts):
        info = _lib.ScheduleInfo()
        check(lib.ultra_plan_schedule_info(self._h, int(nparts), ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in _lib.ScheduleInfo._fields_ if name != "reserved"}

    def _export(self, fn, *key):
        """One array of the plan as an int32 host tensor: ask `fn` for the count, allocate, call again."""
        n = ctypes.c_int64()
        check(fn(self._h, *key, None, 0, ctypes.byref(n)))
        out = torch.empty(n.value, dtype=torch.int32)
        check(fn(self._h, *key, out.data_ptr(), n.value, ctypes.byref(n)))
        return out

    def schedule(self, nparts):
        """(chunk_ptr, unit_ptr, units, chunks[n, 4]) of the static schedule for `nparts` workgroups per span."""
        out = [self._export(lib.ultra_plan_schedule_export, int(nparts), which) for which in range(4)]
        return tuple(out[:3]) + (out[3].view(-1, 4),)

    def streams(self, nparts, walkers=16):
        """(sdesc[nparts * 64, 2] = {first record, steps}, srec[n, 2] = (col, type) records, markers (row, num_relation)).
        walkers=12: the schedule of the launches whose last four waves apply the layer update beside the walk."""
        nparts = int(nparts) | ((1 << 24) if walkers == 12 else 0)
        return tuple(self._export(lib.ultra_plan_schedule_export, nparts, which).view(-1, 2) for which in (4, 5))

    def part_rows(self, nparts):
        """(prow, prow_ptr): the rows each workgroup aggregates -- ascending, -1 padded to whole 32-row tiles -- and their
        bounds per workgroup (schedule arrays 6 and 7: the work list of the update tail)."""
        return tuple(self._export(lib.ultra_plan_schedule_export, int(nparts), which) for which in (6, 7))

    def export(self, which):
        out = self._export(lib.ultra_plan_export, which)
        return out.view(torch.uint8) if which in (_lib.ARR_DENSE, _lib.ARR_DENSE_ORDER) else out

    # ---- kernels ----
    def forward(self, relation, input, edge_weight=None, boundary=None, sum="add", mul="mul", out=None, point=None,
                keep=False, weight_epoch=None):
        """point=(rows, values): a boundary that is zero except row rows[o] of outer slice o, where it is values[o]
        (the NBFNet boundary condition); excludes `boundary`.  sum="add": added to that row only.  sum="min" / "max":
        that row meets values[o], every other row meets 0 (max(update, boundary), layers.py:206-207) -- served by
        reference-order plans; returns None where it is not (the caller then passes the boundary as a tensor).
        keep=True: `edge_weight` is a 0/1 keep mask -- an edge with 0 is absent from the graph for this call
        (ultra_rspmm_forward_masked; differs from a zero weight under min / max only)."""
        if edge_weight is not None and edge_weight.dim() == 2:
            return self._forward_samples(relation, input, edge_weight, boundary, sum, mul, out, point, keep)
        if point is not None:
            if boundary is not None:
                raise RuntimeError("a point boundary excludes `boundary`")
            if sum != "add" and not self.exact:
                return None
            twin = self._twin_for(sum, mul, edge_weight, input, relation, point[1], out)
        else:
            twin = self._twin_for(sum, mul, edge_weight, input, relation, boundary, out)
        if twin is not None:
            return twin.forward(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum, mul=mul, out=out,
                                point=point, keep=keep, weight_epoch=weight_epoch)
        op = self._forward_operands(relation, input, edge_weight, boundary, out, point, weight_epoch)
        _announce_weight(edge_weight, op.epoch)
        if point is not None:
            rc = lib.ultra_rspmm_forward_point(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], op.dtype, op.weight, op.relation,
                                               op.input, op.rows, op.boundary, op.out_ref, stream_of(input))
            if rc == _lib.ULTRA_ERR_UNSUPPORTED and sum != "add":
                return None      # (min / max: the caller passes the boundary as a tensor)
            check(rc)
            return op.out
        entry = lib.ultra_rspmm_forward_masked if (keep and op.weight is not None and sum != "add") else lib.ultra_rspmm_forward
        check(entry(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], op.dtype, op.weight, op.relation, op.input, op.boundary,
                    op.out_ref, stream_of(input)))
        return op.out

    def _forward_operands(self, relation, input, edge_weight, boundary, out, point, weight_epoch=None):
        """The operands of a forward launch, checked and described to the C ABI (_ForwardOperands)."""
        _require_gpu(relation, input, edge_weight, boundary)
        dt = _dtype_code(*([relation, input] + ([edge_weight] if edge_weight is not None else [])
                           + ([boundary] if boundary is not None else [])))
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        if relation.dim() != input.dim():
            raise RuntimeError("relation and input must both be 2-D or both batch-major 3-D")
        if out is None:
            out = _out_like(input, self.num_node)
        out, mout = as_mat(out)
        if point is None:
            boundary, mb = _opt_mat(boundary)
        edge_weight, w, weight_epoch = _weight_operand(edge_weight, self.num_edge, weight_epoch)
        rows = rows_ptr = None
        if point is not None:
            rows, boundary, rows_ptr, mb = _point_operand(point, input)
            _require_gpu(rows, boundary)
        return _ForwardOperands(dt, w, weight_epoch, ctypes.byref(mrel), ctypes.byref(mx), mb, rows_ptr, out, ctypes.byref(mout),
                                (relation, input, edge_weight, boundary, rows))

    def masked_samples_entry(self, relation, input, edge_keep, boundary, sum, mul, out):
        """ultra_rspmm_forward_masked_samples on batch-major 3-D operands; returns the entry's status code (ULTRA_ERR_UNSUPPORTED:
        nothing was launched -- general-walk plans, rotate messages, rows the reference-order kernels do not take)."""
        _require_gpu(relation, input, edge_keep, boundary, out)
        dt = _dtype_code(*([relation, input, edge_keep] + ([boundary] if boundary is not None else [])))
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        out_c, mout = as_mat(out)
        if out_c is not out:
            raise RuntimeError("`out` must have unit stride along its last dimension")
        boundary, mb = _opt_mat(boundary)
        return lib.ultra_rspmm_forward_masked_samples(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], dt, edge_keep.data_ptr(),
                                                      edge_keep.stride(0), ctypes.byref(mrel), ctypes.byref(mx), mb,
                                                      ctypes.byref(mout), stream_of(input))

    def _forward_samples(self, relation, input, edge_keep, boundary, sum, mul, out, point, keep):
        """forward() with one keep mask per outer slice: `edge_keep` (n_outer, num_edge), 0/1, original edge order -- slice s
        runs on the graph without the edges whose keep[s] is 0 (ultra_rspmm_forward_masked_samples).  Where the entry answers
        ULTRA_ERR_UNSUPPORTED, one masked call per slice on views of the operands computes the same values."""
        if not keep:
            raise RuntimeError("a 2-D `edge_weight` is a per-sample keep mask: pass keep=True (per-sample weights are not served)")
        if point is not None:
            raise RuntimeError("per-sample keep masks take a dense boundary (or none), not a point boundary")
        if relation.dim() != 3 or input.dim() != 3:
            raise RuntimeError("per-sample keep masks need batch-major 3-D operands")
        n_outer = input.shape[0]
        if tuple(edge_keep.shape) != (n_outer, self.num_edge):
            raise RuntimeError("Expected a per-sample `edge_weight` of shape (n_outer, num_edge) = (%d, %d), got %s"
                               % (n_outer, self.num_edge, tuple(edge_keep.shape)))
        if (edge_keep.stride(1) != 1 and self.num_edge > 1) or edge_keep.stride(0) < self.num_edge:      # (expanded rows too)
            edge_keep = edge_keep.contiguous()
        if out is None:
            out = torch.empty((n_outer, self.num_node, input.shape[2]), dtype=input.dtype, device=input.device)
        if n_outer == 0:
            return out
        rc = self.masked_samples_entry(relation, input, edge_keep, boundary, sum, mul, out)
        if rc != _lib.ULTRA_ERR_UNSUPPORTED:
            check(rc)
            return out
        for s in range(n_outer):
            self.forward(relation[s:s + 1], input[s:s + 1], edge_weight=edge_keep[s],
                         boundary=None if boundary is None else boundary[s:s + 1], sum=sum, mul=mul, out=out[s:s + 1],
                         keep=True, weight_epoch=0)
        return out

    def delta_rows(self, relation, input, out, delta, boundary=None, sum="add", mul="mul", point=None):
        """`out` = forward(relation, input, boundary / point, sum, mul) on THIS plan; afterwards `out` is that forward on a fresh
        reference-order plan of the graph with `delta`'s added edges (GraphDelta), bit for bit: the rows an added edge points
        into are recomputed in place, nothing else is written (ultra_rspmm_delta_rows).  One launch sized by the delta's
        capacity, so a hipGraph that recorded it serves the delta's later contents.  Returns `out`, or None where the engine
        does not serve the call (general-walk and dense-format plans, rotate messages, misaligned rows) -- nothing was
        launched then."""
        return self._recompute_rows(lib.ultra_rspmm_delta_rows, relation, input, out, delta, boundary, sum, mul, point,
                                    lambda: (delta.operand(),))

    def _recompute_rows(self, entry, relation, input, out, delta, boundary, sum, mul, point, edits, on_gpu=(), tail=()):
        """The body of delta_rows, edit_rows, edit_rows_samples and edit_rows_split: the checks, the operands, one call of `entry`.
        `edits()` -- called once the checks have passed -- returns the entry's struct operands between `output` and `stream`, the
        delta's first (None: a NULL pointer; an int: a device address, passed as it is); `tail`: plain arguments that follow them;
        `on_gpu`: further tensors the entry reads."""
        if not self.exact:
            return None
        if (delta.num_nodes, delta.num_relations) != (self.num_node, self.num_relation) or self.num_in != self.num_node:
            raise RuntimeError("the delta was made for a graph of %d nodes and %d relations, the plan has %d and %d"
                               % (delta.num_nodes, delta.num_relations, self.num_node, self.num_relation))
        if point is not None and boundary is not None:
            raise RuntimeError("a point boundary excludes `boundary`")
        _require_gpu(out, delta.count, *on_gpu)
        op = self._forward_operands(relation, input, None, boundary, out, point)
        if op.out is not out:
            raise RuntimeError("`out` must have unit stride along its last dimension")
        operands = edits()
        rc = entry(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], op.dtype, op.relation, op.input, op.boundary, op.rows,
                   op.out_ref, *[operand if operand is None or isinstance(operand, int) else ctypes.byref(operand)
                                 for operand in operands], *tail, stream_of(input))
        if rc == _lib.ULTRA_ERR_UNSUPPORTED:
            return None
        check(rc)
        return out

    def edit_rows(self, relation, input, out, delta, boundary=None, sum="add", mul="mul", point=None):
        """delta_rows for a delta that also holds RETRACTED facts (GraphDelta.remove): afterwards `out` is the forward on a fresh
        reference-order plan of delta.materialize(...) -- the base edges without the tombstoned ones, then the added edges --
        bit for bit.  The rows an added or a removed edge points into are recomputed in place, dead base edges skipped
        (ultra_rspmm_edit_rows); nothing is read per edge of the graph, nothing else is written, and a captured launch follows
        the delta's buffers.  Returns `out`, or None exactly where delta_rows does."""
        return self._recompute_rows(lib.ultra_rspmm_edit_rows, relation, input, out, delta, boundary, sum, mul, point,
                                    lambda: (delta.operand(), delta.removed_operand()))

    def edit_rows_samples(self, relation, input, out, delta, keys, boundary=None, sum="add", mul="mul", point=None):
        """edit_rows with dead edges PER OUTER SLICE: `keys` = (row, col, type), int32 (n_outer, per_sample) each, per_sample in
        1 .. 8 (GraphDelta.sample_keys).  The rows an edit of `delta` points into are recomputed in place; in slice s an edge
        (row, col, type) -- of the base graph or of the delta -- takes no part if one of keys[.][s] names it (type < 0: every
        type).  Afterwards those rows of out[s] are the forward on a fresh reference-order plan of delta.materialize(...) without
        slice s's dead edges, bit for bit (ultra_rspmm_edit_rows_samples); the other rows are not written -- they are right
        where `out` came from forward(edge_weight=keep (n_outer, num_edge), keep=True) with keep rows that leave the same base
        edges out.  Returns `out`, or None exactly where edit_rows does."""
        def edits():
            return delta.operand(), delta.removed_operand(), self._sample_keys_operand(keys, out)

        return self._recompute_rows(lib.ultra_rspmm_edit_rows_samples, relation, input, out, delta, boundary, sum, mul, point,
                                    edits, on_gpu=keys)

    def edit_rows_split(self, relation, input, out, delta, keys=None, boundary=None, sum="add", mul="mul", point=None,
                        hub_len=None):
        """edit_rows -- with `keys` edit_rows_samples -- where a touched row of more than `hub_len` BASE edges is recomputed by a
        whole workgroup per outer slice, not by one 16-lane group (ultra_rspmm_edit_rows_split): the same rows
        written with the same bits, in one launch sized by the delta's capacity; which rows are hubs is read on the device, so a
        captured launch follows the delta's buffers.  hub_len None: the plan's seg_len; 0: every touched row with a base edge.
        A delta without tombstones passes none (delta_rows).  Returns `out`, or None exactly where edit_rows does."""
        def edits():
            sample_keys = None
            if keys is not None:
                sample_keys = self._sample_keys_operand(keys, out)
            removed = delta.removed_operand() if delta.num_removed or keys is not None else None
            return delta.operand(), removed, sample_keys

        return self._recompute_rows(lib.ultra_rspmm_edit_rows_split, relation, input, out, delta, boundary, sum, mul, point,
                                    edits, on_gpu=keys or (), tail=(ctypes.c_int64(-1 if hub_len is None else int(hub_len)),))

    def edit_rows_owned(self, relation, input, out, overlay, boundary=None, sum="add", mul="mul", point=None, hub_len=None):
        """edit_rows_split for an OVERLAY (AssumedFacts) whose delta edges have an owner each: -1 -- live in every
        outer slice, s -- live in slice s alone, anything else -- live nowhere (ultra_rspmm_edit_rows_owned).  Afterwards slice
        s of every touched row that holds a tombstone key or an edge live in s is the forward on a fresh reference-order plan of
        [surviving base edges ; shared edges ; slice s's edges], bit for bit; the other (row, slice) pairs are NOT written --
        `out` came from forward() on this plan, which is right there.  One launch, both roles, sized by the overlay's capacity.
        Returns `out`, or None exactly where edit_rows does."""
        def edits():
            return overlay.operand(), overlay.owner.data_ptr(), overlay.removed_operand()

        return self._recompute_rows(lib.ultra_rspmm_edit_rows_owned, relation, input, out, overlay, boundary, sum, mul, point,
                                    edits, on_gpu=(overlay.owner,), tail=(ctypes.c_int64(-1 if hub_len is None else int(hub_len)),))

    @staticmethod
    def _sample_keys_operand(keys, out):
        """The per-slice keys of edit_rows_samples / edit_rows_split as the entries take them, checked against `out`."""
        key_row, key_col, key_type = keys
        n_outer = out.shape[0] if out.dim() == 3 else 1
        for t in keys:
            if t.dtype != torch.int32 or t.dim() != 2 or t.shape != key_row.shape or not t.is_contiguous():
                raise RuntimeError("`keys` are three contiguous int32 tensors of one shape (n_outer, per_sample)")
        if key_row.shape[0] != n_outer or not 1 <= key_row.shape[1] <= 8:
            raise RuntimeError("Expected keys of shape (n_outer = %d, 1 .. 8), got %s" % (n_outer, tuple(key_row.shape)))
        return _lib.UltraSampleKeys(key_row.data_ptr(), key_col.data_ptr(), key_type.data_ptr(), key_row.shape[1])

    def forward_update(self, relation, input, weight, bias, ln_weight, ln_bias, eps, flags, mul="mul", point=None, timed=None,
                       sum="add"):
        """Aggregate (`sum`, `mul`, optional point boundary) AND the layer update
        `[input +] relu(layer_norm(linear(cat[input, aggregate])))` in one launch (ultra_rspmm_forward_update: the workgroup
        that aggregated a row also updates it).  Bit-equal with forward(point=...) followed by dense.conv_update.
        Returns the layer output, or None where the launch does not serve the call (the caller makes the two calls).
        timed=(warmup, iters): returns (ms per call, ms of the kernel alone) between HIP events instead
        (ultra_rspmm_forward_update_timed)."""
        if not self.exact or input.dtype != torch.float32 or input.dim() != 3 or input.shape[-1] != 64 or not input.is_cuda:
            return None
        _require_gpu(relation, input, weight)
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        agg = torch.empty((input.shape[0], self.num_node, 64), dtype=torch.float32, device=input.device)
        out = torch.empty_like(agg)
        agg, magg = as_mat(agg)
        out, mout = as_mat(out)
        rows_ptr, mv = None, None
        if point is not None:
            rows, vals, rows_ptr, mv = _point_operand(point, input)
            _require_gpu(rows, vals)
        weight = weight.contiguous()
        args = (self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], ctypes.byref(mrel), ctypes.byref(mx), rows_ptr, mv, ctypes.byref(magg),
                weight.data_ptr(), ptr(bias), ptr(ln_weight), ptr(ln_bias), float(eps), int(flags), ctypes.byref(mout),
                stream_of(input))
        if timed is not None:
            ms, ms_kernel = ctypes.c_float(), ctypes.c_float()
            rc = lib.ultra_rspmm_forward_update_timed(*(args + (int(timed[0]), int(timed[1]), ctypes.byref(ms), ctypes.byref(ms_kernel))))
            if rc == _lib.ULTRA_ERR_UNSUPPORTED:
                return None
            check(rc)
            return ms.value, ms_kernel.value
        rc = lib.ultra_rspmm_forward_update(*args)
        if rc == _lib.ULTRA_ERR_UNSUPPORTED:
            return None
        check(rc)
        return out

    def forward_onehot(self, relation, input, src_rows, edge_weight=None, boundary=None):
        """add_mul forward for an input that is zero outside row src_rows[o] of every outer slice (the NBFNet
        layer-0 boundary condition).  Same result as forward(sum="add", mul="mul"), visiting only the edges
        gathered from the source rows."""
        _require_gpu(relation, input, edge_weight, boundary, src_rows)
        dt = _dtype_code(*([relation, input] + ([edge_weight] if edge_weight is not None else [])
                           + ([boundary] if boundary is not None else [])))
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        out, mout = as_mat(_out_like(input, self.num_node))
        n_outer = 1 if input.dim() == 2 else input.shape[0]
        src_rows = src_rows.to(torch.int64).contiguous()
        if src_rows.numel() != n_outer:
            raise RuntimeError("Expected one source row per outer slice (%d), got %d" % (n_outer, src_rows.numel()))
        boundary, mb = _opt_mat(boundary)
        edge_weight, w, _ = _weight_operand(edge_weight, self.num_edge)
        check(lib.ultra_rspmm_forward_onehot(self._h, dt, w, ctypes.byref(mrel), ctypes.byref(mx), src_rows.data_ptr(), mb,
                                             ctypes.byref(mout), stream_of(input)))
        return out

    def fused_layer(self, relation, input, linear, layer_norm=None, relu=True, residual=False, boundary=None, point=None):
        """A whole layer -- add_mul aggregate (+ boundary), Linear(cat[input, agg]), LayerNorm, ReLU, residual -- in one
        launch on the dense-format twin (ultra_nbf_dense_layer).  Returns None when this plan / these operands are not
        served (the caller then runs forward() + the update kernel)."""
        d = self.dense
        if d is None or self.num_relation > 4 or self.num_node != self.num_in or input.dim() != 3 or input.shape[-1] != 64 \
                or input.dtype != torch.float32 or relation.dtype != torch.float32 or tuple(linear.weight.shape) != (64, 128):
            return None
        others = (relation, boundary, point[1] if point is not None else None)
        if not all(t is None or (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(st % 4 == 0 for st in t.stride()[:-1]))
                   for t in (input,) + others):
            return None
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        out = torch.empty_like(input)
        _, mout = as_mat(out)
        rows = vals = rows_ptr = None
        if point is not None:
            rows, vals, rows_ptr, mb = _point_operand(point, input)
        else:
            boundary, mb = _opt_mat(boundary)
        _require_gpu(relation, input, boundary, rows, vals)
        weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(
            linear, layer_norm, relu, residual, _lib.LAYER_REFERENCE_ORDER if self.exact else 0)
        check(lib.ultra_nbf_dense_layer(d._h, ctypes.byref(mrel), ctypes.byref(mx), mb, rows_ptr, weight.data_ptr(), ptr(bias),
                                        ptr(ln_weight), ptr(ln_bias), eps, flags, ctypes.byref(mout), stream_of(input)))
        return out

    def layer0_fill(self, batch_size, linear, layer_norm=None, relu=True, device=None):
        """The constant rows of layer0() -- relu(LayerNorm(bias)) everywhere -- into a fresh (batch, N, 64) tensor: they depend
        on the layer's parameters only, so a caller may launch this early (on a side stream, beside the relation model) and
        hand the tensor to layer0(out=...) for the special rows."""
        device = device if device is not None else linear.weight.device
        out = torch.empty(batch_size, self.num_node, 64, dtype=torch.float32, device=device)
        _, mout = as_mat(out)
        weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(linear, layer_norm, relu,
                                                                        extra_flags=_lib.LAYER0_ONLY_FILL)
        check(lib.ultra_nbf_layer0(self._h, None, None, None, None, weight.data_ptr(), ptr(bias), ptr(ln_weight), ptr(ln_bias),
                                   eps, flags, ctypes.byref(mout), stream_of(out)))
        return out

    def layer0(self, relation, src_rows, src_values, linear, layer_norm=None, relu=True, residual=False, edge_weight=None,
               aggregate="sum", out=None):
        """Layer 0 of an NBFNet on its one-hot boundary condition (ultra_nbf_layer0): returns the (batch, N, 64) hidden
        state of `relu(LayerNorm(linear(cat[x0, rspmm(x0) + x0]))) [+ x0]`, x0 = src_values[b] (ones if None) at row
        src_rows[b] and zero elsewhere, without materialising x0 or the aggregate."""
        _require_gpu(relation, src_rows, src_values, edge_weight)
        relation, mrel = as_mat(relation)
        bs = relation.shape[0]
        prefilled = out is not None       # (layer0_fill wrote the constant rows already)
        if out is None:
            out = torch.empty(bs, self.num_node, 64, dtype=torch.float32, device=relation.device)
        elif tuple(out.shape) != (bs, self.num_node, 64) or out.dtype != torch.float32 or not out.is_contiguous():
            raise RuntimeError("layer0(out=...): expected the (batch, num_node, 64) fp32 tensor of layer0_fill")
        _, mout = as_mat(out)
        src_rows = src_rows.to(torch.int64).contiguous()
        if src_values is not None:
            src_values = src_values.contiguous()
        if edge_weight is not None:
            edge_weight = edge_weight.to(torch.float32).contiguous()
        weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(
            linear, layer_norm, relu, residual,
            (_lib.LAYER0_MAX if aggregate == "max" else 0) | (_lib.LAYER0_SKIP_FILL if prefilled else 0))
        check(lib.ultra_nbf_layer0(self._h, ptr(edge_weight), ctypes.byref(mrel), src_rows.data_ptr(), ptr(src_values),
                                   weight.data_ptr(), ptr(bias), ptr(ln_weight), ptr(ln_bias), eps, flags, ctypes.byref(mout),
                                   stream_of(relation)))
        return out

    def backward(self, relation, input, output, output_grad, edge_weight=None, need_weight_grad=False, sum="add",
                 mul="mul", weight_epoch=None, input_grad_base=None, keep=False):
        """input_grad_base (sum == "add"): a tensor of the input's shape that the returned input gradient starts from (the
        input's gradient from another consumer); it is overwritten with the total and returned.
        keep=True: `edge_weight` was the forward's 0/1 keep mask -- a dropped edge is absent from the graph, so its weight
        gradient (asked for with need_weight_grad) is zero; relation / input gradients need no flag (ultra_rspmm_forward_masked)."""
        _require_gpu(relation, input, output, output_grad, edge_weight)
        dt = _dtype_code(relation, input, output, output_grad)
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        output, mo = as_mat(output)
        output_grad, mog = as_mat(output_grad)
        rgrad = torch.empty(relation.shape, dtype=relation.dtype, device=relation.device)
        _, mrg = as_mat(rgrad)
        # A graph with a dense-format twin (ULTRA's relation graph) takes its input gradient as that twin's forward over
        # the transposed graph -- the matrix-core kernel of the forward pass, 15 us where the edge walk over the
        # transposed plan takes 70 -- and asks ultra_rspmm_backward for the relation gradient alone.
        xgrad, mxg = None, None
        if self._twin_for(sum, mul, edge_weight, output_grad, relation) is self.dense and self.dense is not None \
                and input.dtype == torch.float32:
            twin = self.dense_transposed()
            if twin is not None:
                xgrad = twin.forward(relation, output_grad, boundary=input_grad_base)
            # ... and its relation gradient from the same format: the per-type products A_t . x of the forward kernel, weighed
            # with output_grad (ultra_rspmm_dense_relation_grad) -- 15 us where the walk over the relation-major plan took 71 + 12
            if xgrad is not None and not need_weight_grad and DENSE_RELATION_GRAD:
                rc = lib.ultra_rspmm_dense_relation_grad(self.dense._h, ctypes.byref(mx), ctypes.byref(mog), ctypes.byref(mrg),
                                                         stream_of(input))
                if rc == _lib.ULTRA_OK:
                    return None, rgrad, xgrad
                if rc != _lib.ULTRA_ERR_UNSUPPORTED:
                    check(rc)
        base = None
        if xgrad is None:
            if input_grad_base is not None:
                if sum != "add" or tuple(input_grad_base.shape) != tuple(input.shape) or input_grad_base.dtype != input.dtype:
                    raise RuntimeError("input_grad_base: the input's shape and dtype, sum == 'add'")
                xgrad = input_grad_base if input_grad_base.is_contiguous() else input_grad_base.contiguous()
                base = xgrad
            else:
                xgrad = torch.empty(input.shape, dtype=input.dtype, device=input.device)
            _, mxg = as_mat(xgrad)
        edge_weight, w, weight_epoch = _weight_operand(edge_weight, self.num_edge, weight_epoch)
        wgrad = None
        wg = None
        if need_weight_grad:
            wgrad = torch.zeros(self.num_edge, dtype=input.dtype, device=input.device)
            wg = wgrad.data_ptr()
        _announce_weight(edge_weight, weight_epoch)
        if base is not None:      # (in place: every row's base is read by the thread that writes its total)
            check(lib.ultra_rspmm_backward_add(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], dt, w, ctypes.byref(mrel),
                                               ctypes.byref(mx), ctypes.byref(mo), ctypes.byref(mog), wg, ctypes.byref(mrg),
                                               ctypes.byref(mxg), ctypes.byref(mxg), stream_of(input)))
        else:
            check(lib.ultra_rspmm_backward(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], dt, w, ctypes.byref(mrel),
                                           ctypes.byref(mx), ctypes.byref(mo), ctypes.byref(mog), wg, ctypes.byref(mrg),
                                           ctypes.byref(mxg) if mxg is not None else None, stream_of(input)))
        if keep and wgrad is not None and edge_weight is not None:
            wgrad = wgrad * (edge_weight != 0).to(wgrad.dtype)
        return wgrad, rgrad, xgrad

    def edge_grad_samples(self, relation, input, output_grad, sum="add", mul="mul"):
        """The edge-weight gradient of every outer slice on its own (ultra_rspmm_edge_grad_samples) -- backward() sums it over
        them: (n_outer, num_edge) fp32 in original edge order for (n_outer, rows, d) operands (2-D: one slice); relation may be
        2-D or an expanded view, one table for every slice.  Deterministic, and at one slice backward()'s weight gradient bit
        for bit.  None where the engine does not serve the call (min / max, rotate, other dtypes): the caller falls back."""
        _require_gpu(relation, input, output_grad)
        if (sum != "add" or mul not in ("mul", "add") or input.dtype != torch.float32 or relation.dtype != torch.float32
                or output_grad.dtype != torch.float32):
            return None
        if input.dim() not in (2, 3) or output_grad.dim() != input.dim():
            raise ValueError("Expected `input` and `output_grad` of the same 2 or 3 dimensions, got %d and %d"
                             % (input.dim(), output_grad.dim()))
        if input.dim() == 2:
            input, output_grad = input.unsqueeze(0), output_grad.unsqueeze(0)
        n_outer, d = input.shape[0], input.shape[2]
        if relation.dim() == 2:
            relation = relation.unsqueeze(0).expand(n_outer, -1, -1)
        if (relation.dim() != 3 or relation.shape[0] != n_outer or relation.shape[2] != d or relation.shape[1] < self.num_relation
                or input.shape[1] < self.num_in or tuple(output_grad.shape) != (n_outer, output_grad.shape[1], d)
                or output_grad.shape[1] < self.num_node):
            raise ValueError("edge_grad_samples: expected relation (n_outer, >= %d, d), input (n_outer, >= %d, d) and output_grad "
                             "(n_outer, >= %d, d), got %s, %s and %s" % (self.num_relation, self.num_in, self.num_node,
                                                                        tuple(relation.shape), tuple(input.shape),
                                                                        tuple(output_grad.shape)))
        wgrad = torch.empty((n_outer, self.num_edge), dtype=torch.float32, device=input.device)
        if n_outer == 0 or d == 0 or self.num_edge == 0:
            return wgrad.zero_()
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        output_grad, mog = as_mat(output_grad)
        rc = lib.ultra_rspmm_edge_grad_samples(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], _lib.F32, ctypes.byref(mrel),
                                               ctypes.byref(mx), ctypes.byref(mog), wgrad.data_ptr(), self.num_edge,
                                               stream_of(input))
        if rc == _lib.ULTRA_ERR_UNSUPPORTED:
            return None
        check(rc)
        return wgrad

    def forward_timed(self, relation, input, edge_weight=None, boundary=None, sum="add", mul="mul", warmup=3, iters=20,
                      point=None):
        """Mean HIP-event time (ms) of the forward launch sequence on the current stream; `point` as in forward()."""
        twin = self._twin_for(sum, mul, edge_weight, input, relation, boundary if point is None else point[1])
        if twin is not None:
            res = twin.forward_timed(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum,
                                     mul=mul, warmup=warmup, iters=iters, point=point)
            self.last_main_kernel_ms = twin.last_main_kernel_ms
            return res
        op = self._forward_operands(relation, input, edge_weight, boundary, None, point)
        ms, ms_kernel = ctypes.c_float(), ctypes.c_float()
        check(lib.ultra_rspmm_forward_timed(self._h, _lib.SUM_CODES[sum], _lib.MUL_CODES[mul], op.dtype, op.weight, op.relation,
                                            op.input, op.boundary, op.rows, op.out_ref, stream_of(input), warmup, iters,
                                            ctypes.byref(ms), ctypes.byref(ms_kernel)))
        self.last_main_kernel_ms = ms_kernel.value
        return ms.value, op.out


def _check_adjacency(adjacency, num_node):
    tiles = (int(num_node) + 15) // 16
    if adjacency.dtype != torch.uint8 or adjacency.dim() != 1 or adjacency.numel() != tiles * tiles * 1024 \
            or not adjacency.is_contiguous():
        raise RuntimeError("Expected the byte adjacency of %d nodes: a contiguous uint8 vector of ceil(n / 16)^2 * 1024 = %d "
                           "bytes, got %s %s" % (num_node, tiles * tiles * 1024, adjacency.dtype, tuple(adjacency.shape)))


def dense_layer_adjacency(adjacency, num_node, relation, input, linear, layer_norm=None, relu=True, residual=False,
                          boundary=None, point=None):
    """Plan.fused_layer in the reference's order on a byte adjacency that is an operand (ultra_nbf_dense_layer_adjacency):
    `adjacency` is tasks.relation_graph_dense_adjacency's vector over `num_node` nodes, read as it stands when the launch
    runs -- a live relation graph rewrites it in place.  No plan is involved.  An operand the engine does not
    serve is an error here, not a None: the caller decided on this route by the layer's kind."""
    _check_adjacency(adjacency, num_node)
    if input.dtype != torch.float32 or relation.dtype != torch.float32 or input.dim() != 3 or input.shape[-1] != 64 \
            or tuple(linear.weight.shape) != (64, 128):
        raise RuntimeError("dense_layer_adjacency serves fp32 at hidden dim 64 (input (batch, num_node, 64), weight (64, 128))")
    relation, mrel = as_mat(relation)
    input, mx = as_mat(input)
    out = torch.empty_like(input)
    _, mout = as_mat(out)
    rows = vals = rows_ptr = None
    if point is not None:
        rows, vals, rows_ptr, mb = _point_operand(point, input)
    else:
        boundary, mb = _opt_mat(boundary)
    _require_gpu(adjacency, relation, input, boundary, rows, vals)
    weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(linear, layer_norm, relu, residual, _lib.LAYER_REFERENCE_ORDER)
    check(lib.ultra_nbf_dense_layer_adjacency(adjacency.data_ptr(), int(num_node), ctypes.byref(mrel), ctypes.byref(mx), mb,
                                              rows_ptr, weight.data_ptr(), ptr(bias), ptr(ln_weight), ptr(ln_bias), eps, flags,
                                              ctypes.byref(mout), stream_of(input)))
    return out


def dense_layer0_adjacency(adjacency, num_node, relation, src_rows, src_values, linear, layer_norm=None, relu=True,
                           residual=False):
    """Plan.layer0 (sum aggregate, no edge weights) read off the byte adjacency (ultra_nbf_dense_layer0_adjacency): the
    (batch, num_node, 64) hidden state of layer 0 on its one-hot boundary condition, bit for bit what Plan.layer0 returns on
    a fresh reference-order plan of the edge list the bytes stand for."""
    _check_adjacency(adjacency, num_node)
    _require_gpu(adjacency, relation, src_rows, src_values)
    if relation.dtype != torch.float32 or relation.dim() != 3 or tuple(linear.weight.shape) != (64, 128) \
            or linear.weight.dtype != torch.float32 or (src_values is not None and src_values.dtype != torch.float32):
        raise RuntimeError("dense_layer0_adjacency serves fp32 at hidden dim 64 (relation (batch, >= 4, 64), weight (64, 128))")
    relation, mrel = as_mat(relation)
    out = torch.empty(relation.shape[0], int(num_node), 64, dtype=torch.float32, device=relation.device)
    _, mout = as_mat(out)
    src_rows = src_rows.to(torch.int64).contiguous()
    if src_values is not None:
        src_values = src_values.contiguous()
    weight, bias, ln_weight, ln_bias, eps, flags = _lib.update_args(linear, layer_norm, relu, residual)
    check(lib.ultra_nbf_dense_layer0_adjacency(adjacency.data_ptr(), int(num_node), ctypes.byref(mrel), src_rows.data_ptr(),
                                               ptr(src_values), weight.data_ptr(), ptr(bias), ptr(ln_weight), ptr(ln_bias), eps,
                                               flags, ctypes.byref(mout), stream_of(relation)))
    return out


TraversalLayout = namedtuple("TraversalLayout", "rows count add_ptr add_src add_type dead_ptr dead_src dead_type")
OwnedTraversalLayout = namedtuple("OwnedTraversalLayout", "rows count add_ptr add_src add_type owner dead_ptr")
ExplainLayout = namedtuple("ExplainLayout", "rows count add_ptr add_src add_dst add_type add_j dead_ptr dead_src dead_type "
                                            "src_rows src_count src_ptr src_dst src_type src_j")


class GraphDelta(object):
    """Facts added to and retracted from a served graph, held beside the cached plan of the base graph instead of rebuilding it
    (DESIGN.md 17, 18).

    A fact (h, r, t) -- r a direct relation, h and t existing entities -- contributes the two edges the loader would create,
    (h, t, r) and (t, h, r + num_relations / 2).  add() appends them; a repeated fact, or one the base graph already states, is
    one more parallel edge.  remove() takes EVERY edge equal to either of the two out of the graph: matching base edges become
    tombstones (one (row, col, type) key stands for all duplicates), matching added facts are deleted from `facts` (later facts
    move up).  Tombstones apply to base edges only, so a fact removed and then added again is one new edge at the end of the
    list.  The MATERIALISED graph is the edge list
    [base edges that carry no tombstone, in base order ; m direct edges in insertion order ; m inverse edges in insertion order]
    (`materialize`), and every result on (base graph, delta) is defined as the same call on the materialised graph.

    `capacity` counts edits: num_facts + num_removed / 2 <= capacity (a retracted fact holds up to two keys, an added one two
    edges).  Prepared at add() / remove() time with torch on the edge list's device, into buffers that keep their address (a
    captured launch reads whatever they hold at replay):
      col / type  int32 (2 capacity)      the delta's edges in the plan's direction (row = edge_index[0], col = edge_index[1]),
                                          sorted by (row, col, id) with id = the edge's position in the materialised list
      rows        int32 (2 capacity)      the distinct rows an added OR a removed edge points into, ascending
      ptr         int32 (2 capacity + 1)  the added edges' ranges per touched row (empty for a row touched by removals only)
      dead_ptr    int32 (2 capacity + 1)  the tombstone keys' ranges per touched row
      dead_col / dead_type  int32 (2 capacity)   the distinct dead (col, type) keys, sorted by (row, col, type)
      count       int32 (1)               the number of touched rows -- the SAME tensor object across add() / remove() calls
      degree      int64 (num_nodes)       SIGNED: added minus removed edges counted at edge_index[1] (what `mean` adds to the base
                                          bincount)
    relation_graph: tasks.build_relation_graph of the materialised list, rebuilt at add() / remove(); the previous object is kept
    when the new adjacency equals the old one (the common case), so its plan and the captures that pin it stay valid.
    `traversal`: a second layout of the same edits keyed by the tail, for the symbolic traversal -- None until
    traversal_operand() is first called (a Predictor never asks), then refreshed with the arrays above (_prepare_traversal).

    A GROWING graph: `data` may hold reserved rows -- num_nodes counts SLOTS, of which the ids below `num_live`
    are entities in use.  num_nodes stays what the plan check of Plan.delta_rows / edit_rows compares and what sizes `degree`
    and the key codes; `check` takes the live bound, which the owner raises as entities arrive (Predictor.add_entities), and
    materialize(num_nodes=num_live) is the graph a fresh predictor would be given.

    A growing VOCABULARY: `data` may be laid out over reserved relation slots -- num_relations // 2 counts the
    direct SLOTS (it stays the inverse offset of edges() and the served numbering), of which the ids below `num_live_relations`
    are relations in use: the bound `check` takes, raised by the owner as relations arrive (Predictor.add_relations).

    The relation graph kept current: on the GPU, add() does not rebuild the relation graph from all base edges.
    The entities' relation bit sets and the four adjacency bit matrices stay resident (`_resident`, seeded at the first add()
    by ultra_relation_graph_bits while the two (num_nodes, W) bit sets fit `relation_bits_budget` bytes), add() runs
    ultra_relation_graph_add_edges over the new facts' edges alone and reads its `changed` word: unchanged -- the relation-graph
    object is kept; changed -- a new one is emitted from a copy of the resident matrices.  remove() cannot clear bits: it
    rebuilds from the edge list as before and drops the resident state, which the next add() seeds again.  `_full_rebuild`
    (tools and tests only): True forces the rebuild from the edge list at every add().

    The relation graph kept current IN PLACE (`live_relation_graph=True`, default False = everything above):
    where the resident route applies and the relation graph has at most DENSE_MAX_IN_ROW nodes, the first add() installs ONE
    tasks.LiveRelationGraph over the resident matrices as `relation_graph`, and that object stays: a later add() that changes
    cells rewrites its byte adjacency in place and raises its version; remove() zeroes the resident sets and marks them again
    from the surviving + added edges into the same buffers (one pass on the device, no host plan).  materialize() hands out
    the object's snapshot(), which no later change writes to.  Where the route does not apply, add() / remove() take the
    route above and the object changes as it does there."""

    def __init__(self, data, capacity=1024, num_live=None, num_live_relations=None, relation_bits_budget=256 << 20,
                 live_relation_graph=False):
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError("capacity must be a positive int (facts), got %r" % (capacity,))
        if not isinstance(live_relation_graph, bool):
            raise ValueError("live_relation_graph must be True or False, got %r" % (live_relation_graph,))
        self.live_relation_graph = live_relation_graph
        self.base = data
        self.num_nodes, self.num_relations = int(data.num_nodes), int(data.num_relations)
        self.num_live = self.num_nodes if num_live is None else int(num_live)
        if not 0 <= self.num_live <= self.num_nodes:
            raise ValueError("num_live must lie in [0, num_nodes = %d], got %r" % (self.num_nodes, num_live))
        self.num_live_relations = self.num_relations // 2 if num_live_relations is None else int(num_live_relations)
        if not 0 <= self.num_live_relations <= self.num_relations // 2:
            raise ValueError("num_live_relations must lie in [0, num_relations // 2 = %d], got %r"
                             % (self.num_relations // 2, num_live_relations))
        self.relation_bits_budget = int(relation_bits_budget)
        self._resident = None           # (hbits, tbits, adj, row_counts, changed) of the materialised list, on the GPU
        self._full_rebuild = False
        self.capacity = capacity
        dev = data.edge_index.device
        self.device = dev
        self.facts = torch.zeros(capacity, 3, dtype=torch.long, device=dev)        # (h, r, t) in insertion order
        self.num_facts = 0
        self.version = 0
        self.col = torch.zeros(2 * capacity, dtype=torch.int32, device=dev)
        self.type = torch.zeros(2 * capacity, dtype=torch.int32, device=dev)
        self.rows = torch.zeros(2 * capacity, dtype=torch.int32, device=dev)
        self.ptr = torch.zeros(2 * capacity + 1, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.degree = torch.zeros(self.num_nodes, dtype=torch.long, device=dev)
        # tombstones: the keys as codes (row * num_nodes + col) * num_relations + type, ascending = sorted by (row, col, type)
        self.dead_keys = []
        self.dead_col = torch.zeros(2 * capacity, dtype=torch.int32, device=dev)
        self.dead_type = torch.zeros(2 * capacity, dtype=torch.int32, device=dev)
        self.dead_ptr = torch.zeros(2 * capacity + 1, dtype=torch.int32, device=dev)
        self._base_codes = None
        self.relation_graph = getattr(data, "relation_graph", None)
        self._materialized = None
        self.traversal = None       # the layout in the symbolic traversal's direction: laid out when first asked for
        self.explain = None         # the layout keyed by destination, for explanations: laid out when first asked for
        self._keep = None           # (version, keep vector)
        self.retired = None         # ids `check` refuses (a sorted int64 vector; set by the owner: LiveGraph.remove_entities)

    def __len__(self):
        return self.num_facts

    @property
    def num_removed(self):
        """The number of tombstone keys held (two per retracted fact the base graph states in both directions)."""
        return len(self.dead_keys)

    @property
    def edited(self):
        """Does the delta change the graph at all (added facts or tombstones)?"""
        return self.num_facts > 0 or len(self.dead_keys) > 0

    def edges(self):
        """(edge_index (2, 2 m), edge_type (2 m)): the appended edges in materialised order -- the m direct ones, then the m
        inverse ones."""
        h, r, t = self.facts[:self.num_facts].unbind(1)
        return torch.stack([torch.cat([h, t]), torch.cat([t, h])]), torch.cat([r, r + self.num_relations // 2])

    def check(self, h, r, t):
        """(h, r, t) as int64 vectors of one length on the delta's device; ValueError for ids outside the graph or a relation
        that is not direct (the entities are the ids below num_live -- num_nodes unless rows are reserved -- and the direct
        relations the ids below num_live_relations -- num_relations // 2 unless relation slots are reserved)."""
        h, r, t = (torch.as_tensor(v, dtype=torch.long, device=self.device).flatten() for v in (h, r, t))
        if not (h.shape == r.shape == t.shape):
            raise ValueError("one head, relation and tail per fact: got %d heads, %d relations and %d tails" % (len(h), len(r), len(t)))
        if len(h):
            if bool(((h < 0) | (h >= self.num_live) | (t < 0) | (t >= self.num_live)).any()):
                raise ValueError("a fact's head and tail must be existing entities (ids in [0, %d))" % self.num_live)
            if self.retired is not None and len(self.retired) and bool(torch.isin(torch.cat([h, t]), self.retired).any()):
                raise ValueError("a fact's head and tail must be existing entities: %d ids are retired (remove_entities) and "
                                 "an id is never handed out again" % len(self.retired))
            if bool(((r < 0) | (r >= self.num_live_relations)).any()):
                raise ValueError("a fact is stated through a direct relation (r < num_relations // 2 = %d); its inverse edge "
                                 "is added with it" % self.num_live_relations)
        return h, r, t

    def add(self, h, r, t):
        """Append the facts (h[i], r[i], t[i]) (ints or vectors); returns the number of facts held.  ValueError for ids out of
        range, inverse relations, or more edits than the capacity holds (the caller compacts first: Predictor.add_facts)."""
        h, r, t = self.check(h, r, t)
        n = len(h)
        if 2 * (self.num_facts + n) + len(self.dead_keys) > 2 * self.capacity:
            raise ValueError("the delta holds %d facts and %d tombstone keys of %d edits: %d more facts do not fit"
                             % (self.num_facts, len(self.dead_keys), self.capacity, n))
        if n == 0:
            return self.num_facts
        self.facts[self.num_facts:self.num_facts + n] = torch.stack([h, r, t], dim=1)
        self.num_facts += n
        self._changed(added=n)
        return self.num_facts

    def _edge_codes(self, row, col, edge_type):
        return (row * self.num_nodes + col) * self.num_relations + edge_type

    def remove(self, h, r, t):
        """Retract the facts (h[i], r[i], t[i]) (ints or vectors, the argument rules of add), one after the other: every base
        edge equal to (h, t, r) or to (t, h, r + num_relations / 2) becomes a tombstone, every added fact equal to (h, r, t) is
        deleted.  Returns an int64 vector: entry i is the number of DIRECT edges fact i took out (0 for a fact stated nowhere,
        which uses no capacity and changes no version).  ValueError where the tombstones would exceed the capacity -- nothing
        is changed then (the caller compacts first: Predictor.remove_facts)."""
        h, r, t = self.check(h, r, t)
        n = len(h)
        removed = [0] * n
        if n == 0:
            return torch.zeros(0, dtype=torch.long, device=self.device)
        if self._base_codes is None:      # the base edges' codes, sorted once: a retraction is two binary searches
            row, col = self.base.edge_index.to(self.device)
            self._base_codes = torch.sort(self._edge_codes(row, col, self.base.edge_type.to(self.device))).values
        queries = torch.stack([self._edge_codes(h, t, r), self._edge_codes(t, h, r + self.num_relations // 2)])
        stated = torch.searchsorted(self._base_codes, queries, right=True) - torch.searchsorted(self._base_codes, queries)
        (direct, inverse), (n_direct, n_inverse) = queries.tolist(), stated.tolist()
        wanted = torch.stack([h, r, t], dim=1).tolist()
        facts = self.facts[:self.num_facts].tolist()
        keys = set(self.dead_keys)
        for i in range(n):
            kept = [f for f in facts if f != wanted[i]]
            removed[i] = len(facts) - len(kept)
            facts = kept
            if n_direct[i] and direct[i] not in keys:
                keys.add(direct[i])
                removed[i] += n_direct[i]
            if n_inverse[i] and inverse[i] not in keys:
                keys.add(inverse[i])
        if len(facts) != self.num_facts or len(keys) != len(self.dead_keys):
            if 2 * len(facts) + len(keys) > 2 * self.capacity:
                raise ValueError("the delta holds %d facts and %d tombstone keys of %d edits: these retractions do not fit"
                                 % (self.num_facts, len(self.dead_keys), self.capacity))
            if len(facts) != self.num_facts:
                self.num_facts = len(facts)
                if facts:
                    self.facts[:len(facts)] = torch.tensor(facts, dtype=torch.long, device=self.device)
            self.dead_keys = sorted(keys)
            self._changed()
        return torch.tensor(removed, dtype=torch.long, device=self.device)

    def _changed(self, added=0):
        self.version += 1
        self._materialized = None
        self._prepare()
        if self.traversal is not None:
            self._prepare_traversal()
        if self.explain is not None:
            self._prepare_explain()
        if not (added and self._add_to_relation_graph(added)) and not (not added and self._remark_live_relation_graph()):
            self._rebuild_relation_graph()

    def _prepare_traversal(self):
        """The edits keyed by the TAIL they point into, into buffers allocated at the first call and refreshed in
        place by every later add() / remove().  The symbolic traversal writes t[b, v] for v = edge_index[1], the other end of
        the plan's row.  Laid out from the facts and the tombstone codes themselves, not from the plan-direction arrays with
        the relations mapped to their inverses: a base graph may state a fact in one direction only, and then the tombstones
        are not symmetric.
          rows       int32 (2 capacity)      the distinct tails an added or a removed edge points into, ascending
          count      int32 (1)               their number -- the SAME tensor object for the delta's life
          add_ptr    int32 (2 capacity + 1)  the added edges' ranges per touched tail
          add_src / add_type    int32 (2 capacity)   the added edges (source, relation), sorted by (tail, relation, source)
          dead_ptr   int32 (2 capacity + 1)  the dead keys' ranges per touched tail
          dead_src / dead_type  int32 (2 capacity)   the distinct dead keys (source, relation), sorted alike: every base edge
                                             source -> tail of that relation is absent; never an added edge"""
        dev, cap = self.device, 2 * self.capacity
        if self.traversal is None:
            buf = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
            self.traversal = TraversalLayout(rows=buf(cap), count=buf(1), add_ptr=buf(cap + 1), add_src=buf(cap),
                                             add_type=buf(cap), dead_ptr=buf(cap + 1), dead_src=buf(cap), dead_type=buf(cap))
        lay = self.traversal
        edge_index, edge_type = self.edges()
        src, dst = edge_index
        order = torch.argsort((dst * self.num_relations + edge_type) * self.num_nodes + src)
        src, dst, edge_type = src[order], dst[order], edge_type[order]
        keys = torch.tensor(self.dead_keys, dtype=torch.long, device=dev)
        key_type = keys % self.num_relations
        key_dst = (keys // self.num_relations) % self.num_nodes
        key_src = keys // (self.num_relations * self.num_nodes)
        order = torch.argsort((key_dst * self.num_relations + key_type) * self.num_nodes + key_src)
        key_src, key_dst, key_type = key_src[order], key_dst[order], key_type[order]
        touched = torch.unique(torch.cat([dst, key_dst]))      # (ascending)
        num_touched = len(touched)
        lay.add_src[:len(src)] = src.to(torch.int32)
        lay.add_type[:len(src)] = edge_type.to(torch.int32)
        lay.dead_src[:len(keys)] = key_src.to(torch.int32)
        lay.dead_type[:len(keys)] = key_type.to(torch.int32)
        lay.rows[:num_touched] = touched.to(torch.int32)
        for ptr, of in ((lay.add_ptr, dst), (lay.dead_ptr, key_dst)):
            counts = torch.bincount(torch.searchsorted(touched, of), minlength=num_touched)
            ptr[1:num_touched + 1] = counts.cumsum(0).to(torch.int32)
        lay.count.fill_(num_touched)

    def traversal_operand(self):
        """The edits in the traversal's direction as the engine takes them (ultra_traversal_edits); valid while this object
        lives.  The first call lays the buffers out; from then on add() / remove() keep them current.  The dead arrays are always
        handed over (empty ranges where no tombstone is held): a captured launch then serves tombstones that arrive later."""
        if self.traversal is None:
            self._prepare_traversal()
        lay = self.traversal
        return _lib.UltraTraversalEdits(lay.rows.data_ptr(), lay.count.data_ptr(), lay.add_ptr.data_ptr(),
                                        lay.add_src.data_ptr(), lay.add_type.data_ptr(), lay.dead_ptr.data_ptr(),
                                        lay.dead_src.data_ptr(), lay.dead_type.data_ptr(), lay.rows.numel(),
                                        lay.add_src.numel(), lay.dead_src.numel())

    def _prepare_explain(self):
        """The edits keyed by the DESTINATION they point into, for the explanation route, whose messages go from
        edge_index[0] into edge_index[1] -- the flipped plan, the opposite of col / type / rows / ptr.  Buffers allocated at the
        first call and refreshed in place by every later add() / remove(); j is an added edge's position in edges().
          rows       int32 (2 capacity)      the distinct destinations an added or a tombstoned edge points into, ascending
          count      int32 (1)               their number -- the SAME tensor object for the delta's life
          add_ptr    int32 (2 capacity + 1)  the added edges' ranges per touched row
          add_src / add_dst / add_type / add_j   int32 (2 capacity)   the added edges, sorted by (destination, j)
          dead_ptr   int32 (2 capacity + 1)  the dead keys' ranges per touched row
          dead_src / dead_type  int32 (2 capacity)   the distinct dead (source, type) keys, sorted by (destination, source, type)
          src_rows / src_count / src_ptr / src_dst / src_type / src_j   the transpose of the added edges: the distinct sources
                                             ascending, their number, and per source its edges (destination, type, j) by j"""
        dev, cap = self.device, 2 * self.capacity
        if self.explain is None:
            buf = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
            self.explain = ExplainLayout(rows=buf(cap), count=buf(1), add_ptr=buf(cap + 1), add_src=buf(cap), add_dst=buf(cap),
                                         add_type=buf(cap), add_j=buf(cap), dead_ptr=buf(cap + 1), dead_src=buf(cap),
                                         dead_type=buf(cap), src_rows=buf(cap), src_count=buf(1), src_ptr=buf(cap + 1),
                                         src_dst=buf(cap), src_type=buf(cap), src_j=buf(cap))
        lay = self.explain
        edge_index, edge_type = self.edges()
        src, dst = edge_index
        num_edge = len(src)
        ids = torch.arange(num_edge, device=dev)
        keys = torch.tensor(self.dead_keys, dtype=torch.long, device=dev)
        key_type = keys % self.num_relations
        key_dst = (keys // self.num_relations) % self.num_nodes
        key_src = keys // (self.num_relations * self.num_nodes)
        order = torch.argsort((key_dst * self.num_nodes + key_src) * self.num_relations + key_type)
        key_src, key_dst, key_type = key_src[order], key_dst[order], key_type[order]
        by_dst = torch.argsort(dst * max(num_edge, 1) + ids)
        by_src = torch.argsort(src * max(num_edge, 1) + ids)
        touched = torch.unique(torch.cat([dst, key_dst]))      # (ascending)
        sources = torch.unique(src)
        for buffer, values in ((lay.add_src, src[by_dst]), (lay.add_dst, dst[by_dst]), (lay.add_type, edge_type[by_dst]),
                               (lay.add_j, by_dst), (lay.src_dst, dst[by_src]), (lay.src_type, edge_type[by_src]),
                               (lay.src_j, by_src), (lay.dead_src, key_src), (lay.dead_type, key_type), (lay.rows, touched),
                               (lay.src_rows, sources)):
            buffer[:len(values)] = values.to(torch.int32)
        for ptr, rows, of in ((lay.add_ptr, touched, dst), (lay.dead_ptr, touched, key_dst), (lay.src_ptr, sources, src)):
            counts = torch.bincount(torch.searchsorted(rows, of), minlength=len(rows))
            ptr[1:len(rows) + 1] = counts.cumsum(0).to(torch.int32)
        lay.count.fill_(len(touched))
        lay.src_count.fill_(len(sources))

    def explain_operand(self):
        """The edits keyed by destination as the engine takes them (ultra_explain_edits); valid while this object lives.  The
        first call lays the buffers out; from then on add() / remove() keep them current."""
        if self.explain is None:
            self._prepare_explain()
        lay = self.explain
        return _lib.UltraExplainEdits(*([getattr(lay, name).data_ptr() for name in ExplainLayout._fields if name != "src_j"]
                                        + [lay.rows.numel(), lay.add_src.numel(), lay.dead_src.numel()]))

    def keep_vector(self):
        """(num_edge,) fp32 over the BASE edge list: 0 where a tombstone key matches the edge, 1 elsewhere -- the rule of
        surviving().  Built with torch on the delta's device, once per version."""
        hit = self._keep
        if hit is not None and hit[0] == self.version:
            return hit[1]
        edge_index, edge_type = self.base.edge_index.to(self.device), self.base.edge_type.to(self.device)
        if not self.dead_keys:
            keep = torch.ones(edge_index.shape[1], dtype=torch.float32, device=self.device)
        else:
            keys = torch.tensor(self.dead_keys, dtype=torch.long, device=self.device)
            codes = self._edge_codes(edge_index[0], edge_index[1], edge_type)
            at = torch.searchsorted(keys, codes).clamp_(max=len(keys) - 1)
            keep = (keys[at] != codes).to(torch.float32)
        self._keep = (self.version, keep)
        return keep

    def delta_edge_grad_samples(self, relation, input, output_grad):
        """The per-sample edge-weight gradients of the ADDED edges (ultra_rspmm_delta_edge_grad_samples): (S, 2 capacity) fp32,
        column j = sum_d output_grad[s, dst_j, d] * relation[s, type_j, d] * input[s, src_j, d] for the edge at position j of
        edges(), the columns from 2 num_facts on zero.  (S, N, d) fp32 operands on the GPU."""
        _require_gpu(relation, input, output_grad)
        if not (relation.dtype == input.dtype == output_grad.dtype == torch.float32) or input.dim() != 3:
            raise RuntimeError("delta_edge_grad_samples takes (S, N, d) fp32 operands")
        operand = self.explain_operand()
        relation, mrel = as_mat(relation)
        input, mx = as_mat(input)
        output_grad, mog = as_mat(output_grad)
        wgrad = torch.empty((input.shape[0], 2 * self.capacity), dtype=torch.float32, device=input.device)
        check(lib.ultra_rspmm_delta_edge_grad_samples(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mx),
                                                      ctypes.byref(mog), wgrad.data_ptr(), wgrad.stride(0), stream_of(input)))
        return wgrad

    def _prepare(self):
        """Sort the delta's edges, decode the tombstone keys, and lay out the union of their rows with both ptr arrays, into the
        fixed buffers."""
        edge_index, edge_type = self.edges()
        num_edge = edge_index.shape[1]
        row, col = edge_index
        ids = torch.arange(num_edge, device=self.device)
        order = torch.argsort((row * self.num_nodes + col) * max(num_edge, 1) + ids)
        row, col, edge_type = row[order], col[order], edge_type[order]
        keys = torch.tensor(self.dead_keys, dtype=torch.long, device=self.device)
        key_type = keys % self.num_relations
        key_col = (keys // self.num_relations) % self.num_nodes
        key_row = keys // (self.num_relations * self.num_nodes)
        touched = torch.unique(torch.cat([row, key_row]))      # (ascending)
        num_touched = len(touched)
        self.col[:num_edge] = col.to(torch.int32)
        self.type[:num_edge] = edge_type.to(torch.int32)
        self.dead_col[:len(keys)] = key_col.to(torch.int32)
        self.dead_type[:len(keys)] = key_type.to(torch.int32)
        self.rows[:num_touched] = touched.to(torch.int32)
        for ptr, of in ((self.ptr, row), (self.dead_ptr, key_row)):
            counts = torch.bincount(torch.searchsorted(touched, of), minlength=num_touched)
            ptr[1:num_touched + 1] = counts.cumsum(0).to(torch.int32)
        self.degree.copy_(torch.bincount(edge_index[1], minlength=self.num_nodes))
        if len(keys):
            lo, hi = torch.searchsorted(self._base_codes, keys), torch.searchsorted(self._base_codes, keys, right=True)
            self.degree -= torch.bincount(key_col, weights=(hi - lo).double(), minlength=self.num_nodes).long()
        self.count.fill_(num_touched)

    def surviving(self, edge_index, edge_type):
        """(edge_index, edge_type) without the edges a tombstone key matches, in their order (the arguments themselves where no
        key is held)."""
        if not self.dead_keys:
            return edge_index, edge_type
        dev = edge_index.device
        keys = torch.tensor(self.dead_keys, dtype=torch.long, device=dev)
        codes = self._edge_codes(edge_index[0], edge_index[1], edge_type.to(dev))
        at = torch.searchsorted(keys, codes).clamp_(max=len(keys) - 1)
        keep = keys[at] != codes
        return edge_index[:, keep], edge_type[keep]

    def _add_to_relation_graph(self, added):
        """The relation graph after the last `added` facts were appended, from their edges alone (the class docstring).  False
        where this route does not apply -- off the GPU, bit sets beyond the budget, no relation graph, the private switch --
        and the caller rebuilds from the edge list."""
        words = (self.num_relations + 31) // 32
        if (self.relation_graph is None or self._full_rebuild or self.device.type != "cuda"
                or 2 * self.num_nodes * words * 4 > self.relation_bits_budget):
            return False
        edge_index, edge_type = self.edges()
        m = self.num_facts
        new = torch.cat([torch.arange(m - added, m, device=self.device), torch.arange(2 * m - added, 2 * m, device=self.device)])
        live = self.live_relation_graph and self.num_relations <= _lib.DENSE_MAX_IN_ROW
        if self._resident is None:      # seeded from the list as it was before these facts
            old = torch.ones(2 * m, dtype=torch.bool, device=self.device)
            old[new] = False
            base_index, base_type = self.surviving(self.base.edge_index, self.base.edge_type)
            before = Data(edge_index=torch.cat([base_index, edge_index[:, old]], dim=1),
                          edge_type=torch.cat([base_type, edge_type[old]]), num_nodes=self.num_nodes,
                          num_relations=self.num_relations)
            adj, counts, hbits, tbits = tasks.relation_graph_bits(before, incidence=True)
            self._resident = (hbits, tbits, adj, counts, torch.zeros(1, dtype=torch.int32, device=self.device))
            if live:
                # the ONE object change of the live route: from here on the resident matrices are the relation graph
                self.relation_graph = tasks.LiveRelationGraph(adj, counts)
            else:
                # (a relation graph handed in that is not the edge list's own is replaced here, as the rebuild replaces it)
                seeded = tasks.relation_graph_from_bits(adj.clone(), counts)
                if not self._same_relation_graph(self.relation_graph, seeded):
                    self.relation_graph = seeded
        live = live and isinstance(self.relation_graph, tasks.LiveRelationGraph)
        hbits, tbits, adj, counts, changed = self._resident
        tasks.relation_graph_add_edges(edge_index[:, new], edge_type[new], self.num_nodes, hbits, tbits, adj, counts, changed)
        status = int(changed)       # (the one host read of the update)
        if status & _lib.RELGRAPH_OUT_OF_RANGE:     # (check() has seen every id: the state and the facts disagree)
            raise RuntimeError("GraphDelta: an added edge lies outside the graph the relation bit sets were laid out for")
        if status & _lib.RELGRAPH_CHANGED:
            if live:
                # in place: the byte adjacency a captured step reads keeps its address and holds the new cells at the next replay
                self.relation_graph.changed()
            else:
                # a copy: the object an older capture holds is not written to by later additions
                self.relation_graph = tasks.relation_graph_from_bits(adj.clone(), counts)
        return True

    def _remark_live_relation_graph(self):
        """The live relation graph after a retraction: bits cannot be cleared one by one, so the resident sets are zeroed and
        marked again from the surviving + added edges, into the SAME buffers -- one pass over the edge list on the device, the
        object and its byte adjacency's address kept.  False where no live relation graph is installed or the route is off."""
        if (not isinstance(self.relation_graph, tasks.LiveRelationGraph) or self._resident is None or self._full_rebuild
                or self.relation_graph.adjacency_bits is not self._resident[2]):
            return False
        hbits, tbits, adj, counts, _ = self._resident
        edge_index, edge_type = self.edges()
        base_index, base_type = self.surviving(self.base.edge_index, self.base.edge_type)
        full = Data(edge_index=torch.cat([base_index, edge_index], dim=1), edge_type=torch.cat([base_type, edge_type]),
                    num_nodes=self.num_nodes, num_relations=self.num_relations)
        tasks.relation_graph_bits(full, incidence=True, out=(adj, counts, hbits, tbits))
        self.relation_graph.changed()
        return True

    def _rebuild_relation_graph(self):
        if self.relation_graph is None:
            return
        self._resident = None       # (bits cannot be cleared: seeded again by the next add())
        edge_index, edge_type = self.edges()
        base_index, base_type = self.surviving(self.base.edge_index, self.base.edge_type)
        full = Data(edge_index=torch.cat([base_index, edge_index], dim=1),
                    edge_type=torch.cat([base_type, edge_type]), num_nodes=self.num_nodes,
                    num_relations=self.num_relations)
        new = tasks.build_relation_graph(full).relation_graph
        # (a live relation graph whose resident state was just dropped is never kept: nothing would keep it current)
        if isinstance(self.relation_graph, tasks.LiveRelationGraph) or not self._same_relation_graph(self.relation_graph, new):
            self.relation_graph = new

    @staticmethod
    def _same_relation_graph(old, new):
        old_bits, new_bits = getattr(old, "adjacency_bits", None), getattr(new, "adjacency_bits", None)
        if old_bits is not None and new_bits is not None and old_bits.device == new_bits.device:
            return old_bits.shape == new_bits.shape and torch.equal(old_bits, new_bits)
        return (old.edge_index.shape == new.edge_index.shape and torch.equal(old.edge_index, new.edge_index)
                and torch.equal(old.edge_type, new.edge_type))

    def materialize(self, data=None, num_nodes=None):
        """`data` (default: the base graph) without the edges a tombstone matches and with the delta's edges appended in
        materialised order, and the delta's relation graph: a copy that shares every other field.  Kept until the next add() /
        remove(), so the plan cache sees one graph.  num_nodes (a graph with reserved rows: the live count): the copy's
        num_nodes, every edge below it -- the same edge list without the reserved rows, a new copy at every call."""
        data = self.base if data is None else data
        if num_nodes is not None and int(num_nodes) != int(data.num_nodes):
            out = copy.copy(self.materialize(data))
            out.num_nodes = int(num_nodes)
            if out.edge_index.numel() and int(out.edge_index.max()) >= out.num_nodes:
                raise ValueError("an edge names id %d, outside num_nodes = %d" % (int(out.edge_index.max()), out.num_nodes))
            return out
        hit = self._materialized
        if hit is not None and hit[0] is data:
            return hit[1]
        edge_index, edge_type = self.edges()
        base_index, base_type = self.surviving(data.edge_index, data.edge_type)
        out = copy.copy(data)
        out.edge_index = torch.cat([base_index, edge_index.to(data.edge_index.device)], dim=1)
        out.edge_type = torch.cat([base_type, edge_type.to(data.edge_type.device)])
        if self.relation_graph is not None and data is self.base:
            # (a live relation graph is written in place: the caller gets the snapshot of this version, which never is)
            live = isinstance(self.relation_graph, tasks.LiveRelationGraph)
            out.relation_graph = self.relation_graph.snapshot() if live else self.relation_graph
        self._materialized = (data, out)
        return out

    def live_view(self, data):
        """`data` with the delta's relation graph in place of its own and nothing else changed (the edge list stays the base
        graph's, so the cached plan is found): what the models walk with this delta beside it.  One object per relation graph."""
        hit = getattr(self, "_live", None)
        if hit is None or hit[0] is not data or hit[1].relation_graph is not self.relation_graph:
            view = copy.copy(data)
            view.relation_graph = self.relation_graph
            hit = self._live = (data, view)
        return hit[1]

    def operand(self):
        """The delta as the engine takes it (ultra_delta); valid while this object lives."""
        return _lib.UltraDelta(self.rows.data_ptr(), self.ptr.data_ptr(), self.col.data_ptr(), self.type.data_ptr(),
                               self.count.data_ptr(), self.rows.numel(), self.col.numel())

    def sample_keys(self, triples, any_type=False, out=None):
        """The edges each stated fact triples[s] = (h, t, r) -- (n, 3) int64 on the delta's device, r direct -- must not see, as
        Plan.edit_rows_samples takes them: (row, col, type), int32 (n, 2) each, in the plan's direction (row = edge_index[0],
        col = edge_index[1], as `_prepare` lays the delta out).  Key 0 is the fact (h, t, r), key 1 its inverse
        (t, h, r + num_relations // 2); any_type=True (the model's `remove_one_hop`): both types are -1, every edge between
        the two nodes goes.  The same edges BaseNBFNet.easy_edge_mask of that single triple drops on materialize().  A few
        copies that a capture records; `out` = (row, col, type): written in place and returned."""
        if triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError("Expected triples of shape (n, 3) = (h, t, r), got %s" % (tuple(triples.shape),))
        n = triples.shape[0]
        if out is None:
            out = tuple(torch.empty(n, 2, dtype=torch.int32, device=triples.device) for _ in range(3))
        row, col, edge_type = out
        for t in out:
            if t.dtype != torch.int32 or tuple(t.shape) != (n, 2):
                raise ValueError("`out` is three int32 tensors of shape (n, 2) = (%d, 2)" % n)
        ends = triples[:, :2]
        row.copy_(ends)                      # (h, t)
        col[:, 0].copy_(ends[:, 1])          # (t, h)
        col[:, 1].copy_(ends[:, 0])
        if any_type:
            edge_type.fill_(-1)
        else:
            edge_type[:, 0].copy_(triples[:, 2])
            edge_type[:, 1].copy_(triples[:, 2] + self.num_relations // 2)
        return out

    def removed_operand(self):
        """The tombstones as the engine takes them (ultra_tombstones); valid while this object lives."""
        return _lib.UltraTombstones(self.dead_ptr.data_ptr(), self.dead_col.data_ptr(), self.dead_type.data_ptr(),
                                    self.dead_col.numel())


class AssumedFacts(object):
    """The OVERLAY of one batch of what-if queries: the persistent delta's edges, live in every sample, then the
    facts each query ASSUMES, live in that query's sample alone.  Nothing is stated: the delta, the graph and the filter graph
    are only read.

        overlay = AssumedFacts(data, delta, batch_size, per_query)      # delta: the served graph's GraphDelta, or None
        overlay.fill([facts_0, None, facts_2, ...])                     # one (m_i, 3) int64 (h, r, t) tensor / list or None each

    Sample i then runs on G_i = [delta.materialize(data) ; its assumed direct edges (h, t, r) in the given order ; their inverse
    edges (t, h, r + num_relations / 2)], duplicates kept as edges.  Laid out the way GraphDelta._prepare lays a delta out, into
    buffers that keep their address and have room for delta.capacity + batch_size * per_query facts -- fill() rewrites them, a
    captured launch reads whatever they hold at replay:
      col / type / owner  int32 (2 F)      the edges in the plan's direction, sorted by (row, col, insertion id); the delta's
                                           edges carry the lowest ids and owner -1, query i's edges (direct, then inverse) owner i
      rows        int32 (2 F)              the distinct rows an edge of the overlay or a tombstone key points into, ascending
      ptr         int32 (2 F + 1)          the edges' ranges per touched row
      dead_ptr    int32 (2 F + 1)          the delta's tombstone keys' ranges per touched row OF THIS LAYOUT; the keys themselves
                                           are the delta's own dead_col / dead_type arrays (the tombstone operand shares them)
      count       int32 (1)                the number of touched rows -- the same tensor for the overlay's life
    The live subsequence of sample s in a row is the sorted row of G_s (Plan.edit_rows_owned).  It offers what
    layers._propagate_delta and Ultra.forward(delta=) ask of a delta; it has no shared materialised edge list (`edges`,
    `surviving` and `materialize` raise): a route that needs one runs predict.assume_reference's loop instead."""
    per_query_owned = True

    def __init__(self, data, delta, batch_size, per_query):
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError("batch_size must be a positive int, got %r" % (batch_size,))
        if isinstance(per_query, bool) or not isinstance(per_query, int) or per_query < 1:
            raise ValueError("per_query must be a positive int (facts one query may assume), got %r" % (per_query,))
        self.base, self.delta, self.batch_size, self.per_query = data, delta, batch_size, per_query
        self.num_nodes, self.num_relations = int(data.num_nodes), int(data.num_relations)
        if delta is not None and (delta.num_nodes, delta.num_relations) != (self.num_nodes, self.num_relations):
            raise ValueError("the delta was made for a graph of %d nodes and %d relations, the overlay's has %d and %d"
                             % (delta.num_nodes, delta.num_relations, self.num_nodes, self.num_relations))
        dev = self.device = data.edge_index.device
        self.capacity = (0 if delta is None else delta.capacity) + batch_size * per_query
        cap = 2 * self.capacity
        self.col, self.type, self.owner, self.rows = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(4))
        self.ptr = torch.zeros(cap + 1, dtype=torch.int32, device=dev)
        self.dead_ptr = torch.zeros(cap + 1, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._no_keys = torch.zeros(1, dtype=torch.int32, device=dev)
        self.num_edges = 0
        self._shared_cache = None       # (delta.version, _shared()'s parts)
        self.traversal = None           # the layout in the symbolic traversal's direction: laid out when first asked for
        self._filled = None             # (src, dst, type, owner) of the last fill, in insertion order
        self.fill([None] * batch_size)

    edited = True       # (handed to a model it always takes the delta route: an empty overlay is a launch that ends at once)

    @property
    def num_removed(self):
        return 0 if self.delta is None else self.delta.num_removed

    @property
    def relation_graph(self):
        """The served relation graph: the delta's, kept as it is (the reference keeps it when a sample's edge set differs)."""
        return getattr(self.base, "relation_graph", None) if self.delta is None else self.delta.relation_graph

    def live_view(self, data):
        return data if self.delta is None else self.delta.live_view(data)

    def check(self, assumed):
        """`assumed` -- one entry per sample -- as a list of (m_i, 3) int64 (h, r, t) tensors on the overlay's device; ValueError
        for a wrong count, a wrong shape, or more than per_query facts in one entry.  (Ids are the caller's to check.)"""
        if len(assumed) != self.batch_size:
            raise ValueError("one entry of assumed facts per sample: got %d for %d samples" % (len(assumed), self.batch_size))
        out = []
        for facts in assumed:
            facts = torch.zeros(0, 3, dtype=torch.long) if facts is None else torch.as_tensor(facts, dtype=torch.long)
            facts = facts.to(self.device).reshape(-1, 3) if facts.numel() == 0 else facts.to(self.device)
            if facts.dim() != 2 or facts.shape[1] != 3:
                raise ValueError("assumed facts are (m, 3) rows (h, r, t), got %s" % (tuple(facts.shape),))
            if len(facts) > self.per_query:
                raise ValueError("a query assumes at most %d facts, got %d" % (self.per_query, len(facts)))
            out.append(facts)
        return out

    def _shared(self):
        """(edge_index, edge_type, key_row, key_tail) of the delta as it is now: its edges in materialised order and the rows
        (edge_index[0]) and the tails (edge_index[1]) of its tombstone keys, built once per delta.version -- a refill between two
        replays does not walk the host list of keys again."""
        version = None if self.delta is None else self.delta.version
        hit = self._shared_cache
        if hit is None or hit[0] != version:
            dev = self.device
            if self.delta is None:
                parts = (torch.zeros(2, 0, dtype=torch.long, device=dev),) + tuple(
                    torch.zeros(0, dtype=torch.long, device=dev) for _ in range(3))
            else:
                keys = torch.tensor(self.delta.dead_keys, dtype=torch.long, device=dev)
                parts = self.delta.edges() + (keys // (self.num_relations * self.num_nodes),
                                              (keys // self.num_relations) % self.num_nodes)
            hit = self._shared_cache = (version, parts)
        return hit[1]

    def fill(self, assumed):
        """Lay out the delta's edges as they are now and the facts `assumed` (check) into the fixed buffers.  Returns the number
        of edges held."""
        assumed = self.check(assumed)
        dev, n, half = self.device, self.num_nodes, self.num_relations // 2
        rows, cols, kinds, owners = [], [], [], []
        shared_index, shared_type, key_row, _ = self._shared()
        if len(shared_type):
            rows.append(shared_index[0]), cols.append(shared_index[1]), kinds.append(shared_type)
            owners.append(torch.full_like(shared_type, -1))
        for s, facts in enumerate(assumed):
            if len(facts):
                h, r, t = facts.unbind(1)
                rows.append(torch.cat([h, t])), cols.append(torch.cat([t, h])), kinds.append(torch.cat([r, r + half]))
                owners.append(torch.full((2 * len(facts),), s, dtype=torch.long, device=dev))
        empty = torch.zeros(0, dtype=torch.long, device=dev)
        row, col, kind, owner = (torch.cat(v) if v else empty for v in (rows, cols, kinds, owners))
        num_edge = len(row)
        self._filled = (row, col, kind, owner)
        order = torch.argsort((row * n + col) * max(num_edge, 1) + torch.arange(num_edge, device=dev))
        row, col, kind, owner = row[order], col[order], kind[order], owner[order]
        touched = torch.unique(torch.cat([row, key_row]))      # (ascending; its length is the refill's one host read)
        num_touched = len(touched)
        self.col[:num_edge] = col.to(torch.int32)
        self.type[:num_edge] = kind.to(torch.int32)
        self.owner[:num_edge] = owner.to(torch.int32)
        self.rows[:num_touched] = touched.to(torch.int32)
        for ptr, of in ((self.ptr, row), (self.dead_ptr, key_row)):
            counts = torch.bincount(torch.searchsorted(touched, of), minlength=num_touched)
            ptr[1:num_touched + 1] = counts.cumsum(0).to(torch.int32)
        self.count.fill_(num_touched)
        self.num_edges = num_edge
        if self.traversal is not None:
            self._prepare_traversal()
        return num_edge

    def _prepare_traversal(self):
        """The last fill keyed by the TAIL an edge points into, as GraphDelta._prepare_traversal lays a delta out,
        into buffers allocated at the first call and rewritten in place by every later fill():
          rows       int32 (2 F)       the distinct tails an edge of the overlay or a dead key of the delta points into, ascending
          count      int32 (1)         their number -- the same tensor for the overlay's life
          add_ptr    int32 (2 F + 1)   the edges' ranges per touched tail
          add_src / add_type / owner   int32 (2 F)   the edges (source, relation, owner: -1 the delta's, i query i's), sorted by
                                       (tail, relation, source) -- a stable sort: equal edges stay in insertion order
          dead_ptr   int32 (2 F + 1)   the delta's dead keys' ranges per touched tail OF THIS LAYOUT; the keys themselves are the
                                       delta's own traversal arrays (dead_src / dead_type, sorted by tail first)"""
        dev, cap = self.device, 2 * self.capacity
        if self.traversal is None:
            buf = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
            self.traversal = OwnedTraversalLayout(rows=buf(cap), count=buf(1), add_ptr=buf(cap + 1), add_src=buf(cap),
                                                  add_type=buf(cap), owner=buf(cap), dead_ptr=buf(cap + 1))
        lay = self.traversal
        if self.delta is not None and self.delta.traversal is None:
            self.delta._prepare_traversal()      # (its dead_src / dead_type: kept current by the delta from here on)
        src, dst, kind, owner = self._filled
        key_dst = self._shared()[3]
        order = torch.sort((dst * self.num_relations + kind) * self.num_nodes + src, stable=True).indices
        src, dst, kind, owner = src[order], dst[order], kind[order], owner[order]
        touched = torch.unique(torch.cat([dst, key_dst]))      # (ascending)
        num_touched, num_edge = len(touched), len(src)
        lay.add_src[:num_edge] = src.to(torch.int32)
        lay.add_type[:num_edge] = kind.to(torch.int32)
        lay.owner[:num_edge] = owner.to(torch.int32)
        lay.rows[:num_touched] = touched.to(torch.int32)
        for ptr, of in ((lay.add_ptr, dst), (lay.dead_ptr, key_dst)):
            counts = torch.bincount(torch.searchsorted(touched, of), minlength=num_touched)
            ptr[1:num_touched + 1] = counts.cumsum(0).to(torch.int32)
        lay.count.fill_(num_touched)

    def traversal_operand(self):
        """The overlay in the traversal's direction as the engine takes it (ultra_traversal_edits), beside `traversal_owner`;
        valid while this object lives.  The first call lays the buffers out; from then on fill() keeps them current.  Without a
        delta the dead arrays are NULL: no tombstones."""
        if self.traversal is None:
            self._prepare_traversal()
        lay = self.traversal
        if self.delta is None:
            dead = (None, None, None, 0)
        else:
            keys = self.delta.traversal
            dead = (lay.dead_ptr.data_ptr(), keys.dead_src.data_ptr(), keys.dead_type.data_ptr(), keys.dead_src.numel())
        return _lib.UltraTraversalEdits(lay.rows.data_ptr(), lay.count.data_ptr(), lay.add_ptr.data_ptr(), lay.add_src.data_ptr(),
                                        lay.add_type.data_ptr(), dead[0], dead[1], dead[2], lay.rows.numel(),
                                        lay.add_src.numel(), dead[3])

    @property
    def traversal_owner(self):
        """int32 (2 F): the owner of every edge of the traversal layout, parallel to its add_src (laid out when first asked for)."""
        if self.traversal is None:
            self._prepare_traversal()
        return self.traversal.owner

    def operand(self):
        """The overlay's rows and edges as the engine takes a delta (ultra_delta); valid while this object lives."""
        return _lib.UltraDelta(self.rows.data_ptr(), self.ptr.data_ptr(), self.col.data_ptr(), self.type.data_ptr(),
                               self.count.data_ptr(), self.rows.numel(), self.col.numel())

    def removed_operand(self):
        """The delta's tombstone keys under this layout's row ranges (ultra_tombstones): the key arrays are the delta's own."""
        if self.delta is None:
            return _lib.UltraTombstones(self.dead_ptr.data_ptr(), self._no_keys.data_ptr(), self._no_keys.data_ptr(), 0)
        return _lib.UltraTombstones(self.dead_ptr.data_ptr(), self.delta.dead_col.data_ptr(), self.delta.dead_type.data_ptr(),
                                    self.delta.dead_col.numel())

    def _no_shared_list(self, *args, **kwargs):
        raise RuntimeError("an overlay of assumed facts has one edge list per sample, no shared one: the per-query loop "
                           "(predict.assume_reference) serves what the engine route does not")

    edges = surviving = materialize = _no_shared_list


# ---- plan cache: the graph is static across the 12 rspmm calls of a forward and across batches ----
_PLAN_CACHE = OrderedDict()
_PLAN_CACHE_SIZE = 16
# Plans built for the operator / module API sum in the reference's order (rspmm.cpp:61-72) by default: scores and
# rankings then reproduce the reference's.  exact_order=False selects the re-associating plans (split hub rows,
# type-run / dense-format twins): same sums up to fp32 rounding, a different rounding pattern.
_plan_defaults = {"seg_len": 0, "g_max": 0, "exact_order": True, "type_runs": "auto", "dense": "auto"}


def set_plan_defaults(seg_len=0, g_max=0, exact_order=True, type_runs="auto", dense="auto"):
    """Tuning hook: defaults for newly built plans (clears the cache)."""
    _plan_defaults.update(seg_len=seg_len, g_max=g_max, exact_order=exact_order, type_runs=type_runs, dense=dense)
    _PLAN_CACHE.clear()


def get_plan(edge_index, edge_type, num_node, num_relation, exact_order=None):
    """The cached plan of a graph.  exact_order=None: the default kind (set_plan_defaults; reference summation order);
    False: the re-associating kind, whatever the default -- what the models' training step asks for (its forward feeds a
    scatter-add backward and a stochastic optimiser step: no summation order to reproduce there)."""
    defaults = _plan_defaults if exact_order is None else dict(_plan_defaults, exact_order=bool(exact_order))
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
           edge_type.data_ptr(), edge_type._version, tuple(edge_type.shape), str(edge_index.device),
           int(num_node), int(num_relation), defaults["exact_order"])
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        plan, ei_ref, et_ref = hit
        _PLAN_CACHE.move_to_end(key)
        if _PLAN_RECORDER is not None:
            _PLAN_RECORDER.append(plan)
        return plan
    plan = Plan(edge_index, edge_type, num_node, num_relation, **defaults)
    if _PLAN_RECORDER is not None:
        _PLAN_RECORDER.append(plan)
    # the tensors are kept alive with the plan so a recycled data_ptr can never alias a stale entry
    _PLAN_CACHE[key] = (plan, edge_index, edge_type)
    while len(_PLAN_CACHE) > _PLAN_CACHE_SIZE:
        _PLAN_CACHE.popitem(last=False)
    return plan


def clear_plan_cache():
    _PLAN_CACHE.clear()


def cached_plans():
    """The Plan objects currently held by the cache."""
    return [entry[0] for entry in _PLAN_CACHE.values()]


_PLAN_RECORDER = None


class record_plans(object):
    """with record_plans() as used: ...   -- `used` collects the plans get_plan() hands out inside the block (each once).
    A hipGraph capture pins exactly the plans its warm-up runs asked for (graph.py), not whatever else sits in the cache."""

    def __enter__(self):
        global _PLAN_RECORDER
        self._outer = _PLAN_RECORDER
        self._raw = []
        _PLAN_RECORDER = self._raw
        self.plans = []
        return self

    def __exit__(self, *exc):
        global _PLAN_RECORDER
        _PLAN_RECORDER = self._outer
        seen = set()
        for plan in self._raw:
            if id(plan) not in seen:
                seen.add(id(plan))
                self.plans.append(plan)
        if self._outer is not None:
            self._outer.extend(self.plans)
        return False


class _PlanRSPMM(autograd.Function):
    """autograd node shared by every (sum, mul) pair; the graph plan rides along as a non-tensor arg."""

    @staticmethod
    def forward(ctx, plan, sum, mul, edge_weight, relation, input, boundary=None, keep=False, point_rows=None,
                point_values=None):
        """boundary (sum == "add" only): added in the kernel's epilogue (layers.py:199-200), its gradient is the output
        gradient itself.  keep: `edge_weight` is a 0/1 keep mask (Plan.forward).  point_rows / point_values (sum == "add",
        excludes `boundary`): the boundary condition in closed form -- point_values[b] at row point_rows[b] of sample b,
        zero elsewhere; its gradient is those rows of the output gradient, so the (batch, N, d) gradient of a boundary
        TENSOR -- which six layers would each hand to autograd to be summed -- never exists."""
        if (boundary is not None or point_rows is not None) and sum != "add":
            raise RuntimeError("the fused boundary of the differentiable rspmm serves the sum aggregate only")
        point = (point_rows, point_values) if point_rows is not None else None
        output = plan.forward(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum, mul=mul, keep=keep,
                              point=point)
        ctx.plan, ctx.sum, ctx.mul = plan, sum, mul
        ctx.keep = bool(keep)
        ctx.point_rows = point_rows
        ctx.weight_epoch = _weight_epoch(edge_weight)       # (the tag rides on the Python object: read it while it is at hand)
        ctx.save_for_backward(edge_weight, relation, input, output)   # rspmm.py:25
        return output

    @staticmethod
    def backward(ctx, output_grad):
        edge_weight, relation, input, output = ctx.saved_tensors
        need_w = ctx.needs_input_grad[3]
        output_grad = output_grad.contiguous()
        weight_grad, relation_grad, input_grad = ctx.plan.backward(
            relation, input, output, output_grad, edge_weight=edge_weight, need_weight_grad=need_w,
            sum=ctx.sum, mul=ctx.mul, keep=ctx.keep,
            weight_epoch=ctx.weight_epoch if (edge_weight is not None and edge_weight.is_contiguous()) else 0)
        boundary_grad = output_grad if ctx.needs_input_grad[6] else None
        values_grad = None
        if ctx.point_rows is not None and ctx.needs_input_grad[9]:
            rows = ctx.point_rows
            values_grad = (output_grad.gather(1, rows.view(-1, 1, 1).expand(-1, 1, output_grad.shape[-1])).squeeze(1) if output_grad.dim() == 3
                           else output_grad[rows[0]].unsqueeze(0))
        return None, None, None, weight_grad, relation_grad, input_grad, boundary_grad, None, None, values_grad   # rspmm.py:35


class _PlanDeltaRSPMM(autograd.Function):
    """The sum / DistMult aggregate of the explanation direction on (base graph, delta): `plan` is the flipped
    re-associating plan of the BASE graph, `delta` a GraphDelta of it.  fp32, (S, N, d) operands; the relation is a constant.
    Both engine calls of each pass write in place."""

    @staticmethod
    def forward(ctx, plan, delta, relation, input, boundary=None):
        if relation.requires_grad:
            raise RuntimeError("the differentiable aggregate on a graph delta takes the relation as a constant: detach it")
        if input.dim() != 3 or relation.dim() != 3 or input.dtype != torch.float32 or relation.dtype != torch.float32:
            raise RuntimeError("the differentiable aggregate on a graph delta serves (S, N, d) fp32 operands")
        if (delta.num_nodes, delta.num_relations) != (plan.num_node, plan.num_relation) or plan.num_in != plan.num_node \
                or delta.base.edge_index.shape[1] != plan.num_edge:
            raise RuntimeError("the delta was made for a graph of %d nodes and %d relations, the plan has %d and %d"
                               % (delta.num_nodes, delta.num_relations, plan.num_node, plan.num_relation))
        # a tombstoned edge is absent, exactly: its message is multiplied by 0 (no tombstone held: unit weights, no vector)
        keep = delta.keep_vector() if delta.num_removed else None
        operand = delta.explain_operand()
        output = plan.forward(relation, input, edge_weight=keep, boundary=boundary, sum="add", mul="mul", keep=keep is not None)
        rel, mrel = as_mat(relation)
        x, mx = as_mat(input)
        out, mout = as_mat(output)
        check(lib.ultra_rspmm_delta_edges_forward(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mx), ctypes.byref(mout),
                                                  stream_of(input)))
        ctx.plan, ctx.delta, ctx.version = plan, delta, delta.version
        ctx.save_for_backward(keep, relation, input, output)
        return output

    @staticmethod
    def backward(ctx, output_grad):
        keep, relation, input, output = ctx.saved_tensors
        if ctx.delta.version != ctx.version:
            raise RuntimeError("the graph delta changed between the forward and the backward of an explanation")
        output_grad = output_grad.contiguous()
        _, _, input_grad = ctx.plan.backward(relation, input, output, output_grad, edge_weight=keep, sum="add", mul="mul",
                                             keep=keep is not None)
        operand = ctx.delta.explain_operand()
        rel, mrel = as_mat(relation)
        og, mog = as_mat(output_grad)
        xg, mxg = as_mat(input_grad)
        check(lib.ultra_rspmm_delta_edges_backward_input(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mog),
                                                         ctypes.byref(mxg), stream_of(input)))
        return None, None, None, input_grad, (output_grad if ctx.needs_input_grad[4] else None)


def plan_delta_rspmm(plan, delta, relation, input, boundary=None):
    """sum / DistMult aggregate on (the base graph of `plan`, `delta`), differentiable in `input` and `boundary`
    (_PlanDeltaRSPMM)."""
    return _PlanDeltaRSPMM.apply(plan, delta, relation, input, boundary)


_OUT_CSR_CACHE = OrderedDict()


def out_edge_csr(edge_index, edge_type, num_node):
    """Edges grouped by their SOURCE node (edge_index[1], the gathered side), every node's edges sorted by type:
    (ptr (num_node + 1), edge ids in (source, type) order, largest out-degree); built once per edge list and kept with it."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), edge_type.data_ptr(), edge_type._version,
           int(num_node))
    hit = _OUT_CSR_CACHE.get(key)
    if hit is None:
        src = edge_index[1]
        count = torch.bincount(src, minlength=int(num_node))
        ptr = torch.zeros(int(num_node) + 1, dtype=torch.int64, device=src.device)
        ptr[1:] = count.cumsum(0)
        num_type = int(edge_type.max()) + 1 if edge_type.numel() else 1
        order = torch.sort(src * num_type + edge_type, stable=True)[1].contiguous()
        hit = (ptr, order, int(count.max()) if count.numel() else 0, edge_index, edge_type)      # (the tensors stay with their entry)
        _OUT_CSR_CACHE[key] = hit
        while len(_OUT_CSR_CACHE) > _PLAN_CACHE_SIZE:
            _OUT_CSR_CACHE.popitem(last=False)
    return hit[:3]


class _OnehotRSPMM(autograd.Function):
    """Differentiable add_mul rspmm of an NBFNet's FIRST layer: the input is the boundary condition itself -- values[b]
    at row rows[b] of sample b, zero elsewhere (models.py:59-66, 135-141) -- and so is the boundary added to the sum
    (layers.py:199-200).  Only the edges leaving the source rows carry a message:

        out[b, row_e] += w_e rel[b, type_e] * values[b]        for e with col_e == rows[b];     out[b, rows[b]] += values[b]

    Forward: Plan.forward_onehot (those edges only).  Backward: the same few edges -- S[b, t] = sum of w_e
    output_grad[b, row_e] over the source's out-edges of type t gives relation_grad[b, t] = values[b] * S[b, t] and
    values_grad[b] = sum_t rel[b, t] * S[b, t] + output_grad[b, rows[b]] -- as a handful of small torch kernels over a
    (batch, largest out-degree) padded edge table, instead of two walks over every edge of the graph (at YAGO3-10's
    size 0.56 + 0.89 ms of a 21 ms step, plus 0.56 for the full forward walk).  `dense_input` is the boundary as a
    tensor, which the layer's update reads anyway; its gradient is returned through `values`."""

    @staticmethod
    def forward(ctx, plan, edge_index, edge_type, edge_weight, relation, rows, values, dense_input):
        out = plan.forward_onehot(relation, dense_input, rows, edge_weight=edge_weight, boundary=dense_input)
        ctx.plan, ctx.edge_index, ctx.edge_type = plan, edge_index, edge_type
        ctx.save_for_backward(edge_weight, relation, rows, values)
        return out

    @staticmethod
    def backward(ctx, output_grad):
        edge_weight, relation, rows, values = ctx.saved_tensors
        edge_index, edge_type = ctx.edge_index, ctx.edge_type
        og = output_grad.contiguous()
        need_rel, need_val = ctx.needs_input_grad[4], ctx.needs_input_grad[6]
        ptr, order, max_deg = out_edge_csr(edge_index, edge_type, ctx.plan.num_in)
        grads = _onehot_backward_kernel(ptr, order, edge_index, edge_type, edge_weight, relation, rows, values, og,
                                        need_rel, need_val)
        if grads is None:       # (shapes the kernel does not serve)
            grads = _onehot_backward_torch(ptr, order, max_deg, edge_index, edge_type, edge_weight, relation, rows, values, og,
                                           need_rel, need_val)
        return None, None, None, None, grads[0], None, grads[1], None


def _onehot_backward_kernel(ptr, order, edge_index, edge_type, edge_weight, relation, rows, values, og, need_rel, need_val):
    """(relation_grad, values_grad) of _OnehotRSPMM in one launch (csrc/onehot_bwd.hip); None where it does not apply."""
    if not (og.is_cuda and og.dtype == torch.float32 and relation.dtype == torch.float32 and values.dtype == torch.float32
            and og.dim() == 3 and edge_index.dtype == torch.int64 and edge_type.dtype == torch.int64
            and (edge_weight is None or edge_weight.dtype == torch.float32)):
        return None
    relation, mrel = as_mat(relation)
    og, mog = as_mat(og)
    values = values.contiguous()
    rows = rows.to(torch.int64).contiguous()
    target = edge_index[0].contiguous()
    weight = edge_weight.contiguous() if edge_weight is not None else None
    bs, dim = og.shape[0], og.shape[2]
    rel_grad = torch.empty(bs, relation.shape[1], dim, dtype=torch.float32, device=og.device) if need_rel else None
    val_grad = torch.empty(bs, dim, dtype=torch.float32, device=og.device) if need_val else None
    rc = lib.ultra_rspmm_onehot_backward(ptr.data_ptr(), order.data_ptr(), target.data_ptr(), edge_type.data_ptr(),
                                         _lib.ptr(weight), ctypes.byref(mrel), values.data_ptr(), rows.data_ptr(),
                                         ctypes.byref(mog), _lib.ptr(rel_grad), _lib.ptr(val_grad), stream_of(og))
    if rc == _lib.ULTRA_ERR_UNSUPPORTED:
        return None
    check(rc)
    return rel_grad, val_grad


def _onehot_backward_torch(ptr, order, max_deg, edge_index, edge_type, edge_weight, relation, rows, values, og, need_rel, need_val):
    """The same gradients as a handful of torch kernels over a (batch, largest out-degree) padded edge table: the
    restatement the kernel is tested against, and the route for shapes it does not serve."""
    bs, _, dim = og.shape
    num_rel = relation.shape[1]
    dev = og.device
    batch_ids = torch.arange(bs, device=dev)
    own = og[batch_ids, rows]                                            # (bs, dim): the boundary's share
    if max_deg == 0 or edge_index.shape[1] == 0:
        return (torch.zeros(bs, num_rel, dim, dtype=og.dtype, device=dev) if need_rel else None), (own if need_val else None)
    start = ptr[rows]
    deg = ptr[rows + 1] - start
    slot = torch.arange(max_deg, device=dev).unsqueeze(0)                # (1, max_deg)
    valid = slot < deg.unsqueeze(1)                                      # (bs, max_deg)
    edge = order[(start.unsqueeze(1) + slot).clamp_(max=edge_index.shape[1] - 1)]
    weight = valid.to(og.dtype)
    if edge_weight is not None:
        weight = weight * edge_weight[edge].to(og.dtype)
    picked = og.gather(1, edge_index[0][edge].unsqueeze(-1).expand(-1, -1, dim)) * weight.unsqueeze(-1)
    cell = (edge_type[edge] + num_rel * batch_ids.unsqueeze(1)).flatten()
    s = og.new_zeros(bs * num_rel, dim).index_add_(0, cell, picked.flatten(0, 1)).view(bs, num_rel, dim)
    return (values.unsqueeze(1) * s if need_rel else None), ((relation * s).sum(dim=1) + own if need_val else None)


def onehot_rspmm(plan, edge_index, edge_type, relation, rows, values, dense_input, edge_weight=None):
    """Differentiable first-layer rspmm on the boundary condition (rows, values); see _OnehotRSPMM."""
    return _OnehotRSPMM.apply(plan, edge_index, edge_type, edge_weight, relation, rows, values, dense_input)


def _check_args(edge_index, edge_type, edge_weight, relation, input):
    # rspmm_forward_check, rspmm.cpp:15-27
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise RuntimeError("Expected 2-dimensional `edge_index` of size (2, num_edge)")
    if edge_type.dim() != 1 or edge_weight.dim() != 1 or relation.dim() != 2 or input.dim() != 2:
        raise RuntimeError("Expected 1-dimensional edge_type / edge_weight and 2-dimensional relation / input")
    E = edge_index.shape[1]
    if edge_type.shape[0] != E or edge_weight.shape[0] != E:
        raise RuntimeError("Expected edge_type and edge_weight of size (%d,)" % E)
    if relation.shape[1] != input.shape[1]:
        raise RuntimeError("Expected relation.size(1) == input.size(1), got %d and %d"
                           % (relation.shape[1], input.shape[1]))
    _require_gpu(edge_index, edge_type, edge_weight, relation, input)
    _dtype_code(edge_weight, relation, input)


def _sorted_assert(edge_index):
    node_in, node_out = edge_index
    if node_in.numel():
        key = node_in * (node_out.max() + 1) + node_out
        assert (key.diff() >= 0).all(), "Expect sorted `edge_index`"   # rspmm.py:16-18


def _make_function(sum, mul):
    class _Function(autograd.Function):
        @staticmethod
        def forward(ctx, edge_index, edge_type, edge_weight, relation, input):
            _check_args(edge_index, edge_type, edge_weight, relation, input)
            _sorted_assert(edge_index)
            plan = get_plan(edge_index, edge_type, input.shape[0], relation.shape[0])
            output = plan.forward(relation, input, edge_weight=edge_weight, sum=sum, mul=mul)
            ctx.plan = plan
            ctx.save_for_backward(edge_index, edge_type, edge_weight, relation, input, output)
            return output

        @staticmethod
        def backward(ctx, output_grad):
            edge_index, edge_type, edge_weight, relation, input, output = ctx.saved_tensors
            weight_grad, relation_grad, input_grad = ctx.plan.backward(
                relation, input, output, output_grad.contiguous(), edge_weight=edge_weight,
                need_weight_grad=True, sum=sum, mul=mul)
            return None, None, weight_grad, relation_grad, input_grad

    _Function.__name__ = _Function.__qualname__ = "RSPMM%s%sFunction" % (sum.capitalize(), mul.capitalize())
    return _Function


RSPMMAddMulFunction = _make_function("add", "mul")   # rspmm.py:12
RSPMMMinMulFunction = _make_function("min", "mul")   # rspmm.py:38
RSPMMMaxMulFunction = _make_function("max", "mul")   # rspmm.py:64
RSPMMAddAddFunction = _make_function("add", "add")   # rspmm.py:90
RSPMMMinAddFunction = _make_function("min", "add")   # rspmm.py:116
RSPMMMaxAddFunction = _make_function("max", "add")   # rspmm.py:142
# RotatE messages (no reference twin): (N, D) operands, the whole row one complex vector -- real half | imaginary half
RSPMMAddRotateFunction = _make_function("add", "rotate")
RSPMMMinRotateFunction = _make_function("min", "rotate")
RSPMMMaxRotateFunction = _make_function("max", "rotate")


def generalized_rspmm(edge_index, edge_type, edge_weight, relation, input, sum="add", mul="mul"):
    """rspmm.py:168-179.  Unsorted edges are fine: the cached plan carries the sort."""
    name = "RSPMM%s%sFunction" % (sum.capitalize(), mul.capitalize())
    if not hasattr(module, name):
        raise ValueError("No generalized rspmm implementation found for summation `%s` and multiplication `%s`"
                         % (sum, mul))
    _check_args(edge_index, edge_type, edge_weight, relation, input)
    plan = get_plan(edge_index, edge_type, input.shape[0], relation.shape[0])
    return _PlanRSPMM.apply(plan, sum, mul, edge_weight, relation, input, None, False)


def plan_rspmm(plan, relation, input, edge_weight=None, sum="add", mul="mul", boundary=None, keep=False, point=None):
    """Differentiable rspmm on an explicit plan; accepts batch-major (batch, N, d) operands.  point=(rows, values): the
    boundary condition in closed form (sum == "add"; excludes `boundary`), differentiable in `values`."""
    if point is not None:
        if boundary is not None:
            raise RuntimeError("a point boundary excludes `boundary`")
        return _PlanRSPMM.apply(plan, sum, mul, edge_weight, relation, input, None, keep, point[0], point[1])
    return _PlanRSPMM.apply(plan, sum, mul, edge_weight, relation, input, boundary, keep)


class _ReferenceExports(object):
    """The reference extension's pybind surface (rspmm.cpp:256-283) over the stateless C entry points."""

    def __getattr__(self, name):
        parts = name.split("_")
        if len(parts) == 5 and parts[0] == "rspmm" and parts[1] in _lib.SUM_CODES and parts[2] in ("mul", "add") \
                and parts[3] in ("forward", "backward") and parts[4] in ("cuda", "cpu"):
            if parts[4] == "cpu":
                def no_cpu(*args, **kwargs):
                    raise RuntimeError("ultra_amd: `%s` -- this engine is MI355X-only and has no CPU path" % name)
                return no_cpu
            return self._forward(parts[1], parts[2]) if parts[3] == "forward" else self._backward(parts[1], parts[2])
        raise AttributeError(name)

    @staticmethod
    def _forward(sum, mul):
        fn = getattr(lib, "ultra_rspmm_%s_%s_forward_cuda" % (sum, mul))

        def forward(edge_index, edge_type, edge_weight, relation, input):
            _check_args(edge_index, edge_type, edge_weight, relation, input)
            dt = _dtype_code(edge_weight, relation, input)
            ei, et, ew = edge_index.contiguous(), edge_type.contiguous(), edge_weight.contiguous()
            rel, x = relation.contiguous(), input.contiguous()
            out = torch.empty_like(x)
            check(fn(ei.data_ptr(), et.data_ptr(), ew.data_ptr(), rel.data_ptr(), x.data_ptr(), out.data_ptr(),
                     ei.shape[1], x.shape[0], rel.shape[0], x.shape[1], dt, stream_of(input)))
            return out
        return forward

    @staticmethod
    def _backward(sum, mul):
        fn = getattr(lib, "ultra_rspmm_%s_%s_backward_cuda" % (sum, mul))

        def backward(edge_index, edge_type, edge_weight, relation, input, output, output_grad):
            _check_args(edge_index, edge_type, edge_weight, relation, input)
            dt = _dtype_code(edge_weight, relation, input, output, output_grad)
            ei, et, ew = edge_index.contiguous(), edge_type.contiguous(), edge_weight.contiguous()
            rel, x = relation.contiguous(), input.contiguous()
            o, og = output.contiguous(), output_grad.contiguous()
            wg, rg, xg = torch.zeros_like(ew), torch.zeros_like(rel), torch.zeros_like(x)
            check(fn(ei.data_ptr(), et.data_ptr(), ew.data_ptr(), rel.data_ptr(), x.data_ptr(), o.data_ptr(),
                     og.data_ptr(), wg.data_ptr(), rg.data_ptr(), xg.data_ptr(), ei.shape[1], x.shape[0],
                     rel.shape[0], x.shape[1], dt, stream_of(input)))
            return wg, rg, xg
        return backward


rspmm = _ReferenceExports()


def get_tuning():
    """The launch knobs in force (ultra_get_tuning) as a dict."""
    t = _lib.Tuning()
    check(lib.ultra_get_tuning(ctypes.byref(t)))
    return {"threads": t.threads, "grid": t.grid, "rel_lds": t.rel_lds, "x_lds": t.x_lds, "unroll": t.unroll,
            "general_walk": t.reserved[0], "unit_walk": t.reserved[1], "update_form": t.reserved[2]}


class tuning_scope(object):
    """with tuning_scope(grid=192): ... -- the launches inside run (and a capture inside records them) with the given knobs changed,
    every other knob as it was; the former tuning is back afterwards.  The knobs are process-wide (ultra_set_tuning): not for
    threads that launch at the same time with different ones."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        self.was = _lib.Tuning()
        check(lib.ultra_get_tuning(ctypes.byref(self.was)))
        t = _lib.Tuning()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(self.was), ctypes.sizeof(t))
        for k, v in self.knobs.items():
            if k in ("general_walk", "unit_walk", "update_form"):
                t.reserved[("general_walk", "unit_walk", "update_form").index(k)] = int(v)
            else:
                setattr(t, k, int(v))
        check(lib.ultra_set_tuning(ctypes.byref(t)))
        return self

    def __exit__(self, *exc):
        check(lib.ultra_set_tuning(ctypes.byref(self.was)))
        return False


def check_device_error():
    """Raise if a launch before this point ended on a bounded wait of the one-launch layer's hand-off (ultra_device_error,
    include/ultra_rspmm.h): call after synchronising.  The same word is looked at on entry of every rspmm forward."""
    check(lib.ultra_device_error())


def set_tuning(threads=0, grid=0, rel_lds=-1, x_lds=-1, unroll=0, general_walk=0, unit_walk=0, update_form=0):
    """Kernel-launch tuning knobs (measurement / tests).  set_tuning() restores the defaults.
    general_walk: reference-order plans on the general walk kernel; unit_walk: the reference-order kernels walk units of
    four rows (C++ loops) instead of group streams (assembly loops); update_form: where forward_update applies the layer
    update -- 0 the library's choice (3 where it fits and the graph has 10+ steps a row, else 1), 1 in the kernel's tail, 3 beside the
    walk with the rows passing through LDS (forward_update returns None where it does not fit; 2 -- rows by reference -- was removed
    in ABI 6 and always answers None)."""
    t = _lib.Tuning(int(threads), int(grid), int(rel_lds), int(x_lds), int(unroll),
                    (ctypes.c_int32 * 3)(int(general_walk), int(unit_walk), int(update_form)))
    check(lib.ultra_set_tuning(ctypes.byref(t)))
