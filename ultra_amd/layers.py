"""GeneralizedRelationalConv -- the relational message-passing layer (reference: ultra/layers.py).

Same constructor, forward signature, parameter names and numerics as the reference layer, without
PyG: the fused path (layers.py:183-231) calls the HIP rspmm engine directly on the module-level
batch-major layout (batch, N, dim), so the three `transpose(0, 1).flatten(1)` copies of the
reference (layers.py:190-192) and the per-call edge sort disappear, and under no_grad the boundary
epilogue (layers.py:199-207) is fused into the kernel.  `rotate` messages, which the reference runs unfused, go through the
same engine (mul="rotate") in the unfused path's direction for the sum / mean / max / min aggregates.  The unfused
message/aggregate path (layers.py:135-181; differentiable edge weights, `rotate` with pna or on the CPU) is kept as
plain torch index ops.
"""
import os

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, dense, rspmm


# Layer 0 of every NBFNet reads the boundary condition itself: zero everywhere except the head row of each sample.
# With sum aggregation and DistMult messages only that row's out-edges contribute (exactly), so the layer can ask
# the engine for the row-sparse forward instead of the dense one.  Module-level switch for A/B tests.
ONEHOT_FAST_PATH = True
# the boundary condition kept as (row, value) per sample instead of a (batch, N, d) tensor; layer 0 computed on its
# special rows only (A/B switch for tests)
POINT_BOUNDARY_FAST_PATH = True
# ... and under autograd (fine-tuning): the sum aggregate's differentiable rspmm reads the closed form too (A/B switch for tests)
POINT_BOUNDARY_TRAINING = True
# aggregate + update of a training step's layer as one autograd node (A/B switch for tests)
TRAINING_LAYER_NODE = True
# the last layer of a training step evaluated at the rows the readout reads.  Its backward is a pair of gathers in a fixed order
# (ultra_rspmm_rows_backward_gather; round 5 scattered with float atomics: dense.ROWS_BACKWARD_GATHER = False is that route);
# ULTRA_LAST_LAYER_ON_ROWS=0 (or the attribute) runs the whole layer's walk instead
LAST_LAYER_ON_ROWS = os.environ.get("ULTRA_LAST_LAYER_ON_ROWS", "1") != "0"
# aggregate + update of a layer in one launch on dense-format plans (A/B switch for tests)
FUSED_DENSE_LAYER = True
# aggregate + update of a layer in one launch on the reference-order plan of a sparse graph: the update runs in the tail of
# the rspmm kernel, on the rows each workgroup has just summed.  Same bits as the two launches, 1 - 2.7 % faster on the
# benchmark step.  ULTRA_FUSED_SPARSE_LAYER=0 (or the attribute, for A/B tests) selects the two launches.
FUSED_SPARSE_LAYER = os.environ.get("ULTRA_FUSED_SPARSE_LAYER", "1") != "0"
# `rotate` messages through the rspmm engine (mul="rotate") instead of index_select / cat / scatter over (batch, |E|, d)
# tensors: memory O(|V| d) instead of O(|E| d), a fixed summation order.  False = the unfused route (A/B switch for tests)
FUSED_ROTATE = True


class PointBoundary(object):
    """The NBFNet boundary condition (models.py:59-66, 135-141) in closed form: zero everywhere except row rows[b]
    of sample b, which holds values[b]."""

    def __init__(self, rows, values, num_node):
        # (made contiguous once here: every layer hands these pointers to a kernel)
        self.rows, self.values, self.num_node = rows.to(torch.int64).contiguous(), values.contiguous(), num_node
        self._dense = None

    @property
    def requires_grad(self):
        return self.values.requires_grad

    def dense(self):
        """The (batch, num_node, dim) tensor the reference builds with zeros + scatter_add_ (built once per boundary
        where no gradient flows through it)."""
        if self._dense is not None:
            return self._dense
        if dense.boundary_supported(self.rows, self.values):
            out = dense.onehot_boundary(self.rows, self.values, self.num_node, self.values.shape[-1])
        else:
            out = torch.zeros(len(self.rows), self.num_node, self.values.shape[-1], device=self.values.device,
                              dtype=self.values.dtype)
            index = self.rows.view(-1, 1, 1).expand(-1, 1, self.values.shape[-1])
            out = out.scatter_add_(1, index, self.values.unsqueeze(1))
        if not (torch.is_grad_enabled() and self.values.requires_grad):
            self._dense = out
        return out


def _scatter(src, index, dim_size, reduce):
    # src (batch, M, d) scattered along dim 1 (what torch_scatter.scatter does at layers.py:165-179)
    shape = (src.shape[0], dim_size, src.shape[2])
    idx = index.view(1, -1, 1).expand_as(src)
    if reduce in ("sum", "add"):
        return torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(1, idx, src)
    if reduce == "mean":
        total = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(1, idx, src)
        count = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(1, idx, torch.ones_like(src))
        return total / count.clamp(min=1)
    if reduce in ("max", "min"):
        out = torch.zeros(shape, dtype=src.dtype, device=src.device)
        return out.scatter_reduce(1, idx, src, reduce="amax" if reduce == "max" else "amin", include_self=False)
    raise ValueError("Unknown aggregation function `%s`" % reduce)


_FLIPPED = {}


def _flipped_edges(edge_index):
    """edge_index with its two rows swapped, one tensor per graph (so the plan cache, keyed on the tensor, hits)."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), str(edge_index.device))
    hit = _FLIPPED.pop(key, None)
    if hit is None:
        # (the eight graphs used last stay: a served base graph keeps its tensor -- and with it its cached plan -- while
        # explanations of other graphs come and go)
        while len(_FLIPPED) >= 8:
            del _FLIPPED[next(iter(_FLIPPED))]
        hit = (edge_index.flip(0).contiguous(), edge_index)
    _FLIPPED[key] = hit
    return hit[0]


_IN_DEGREE = {}


def _in_degree(edge_index, num_node):
    """bincount(edge_index[1]) as int64, one tensor per graph (bincount reads its size back: not for a captured step)."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), str(edge_index.device), int(num_node))
    hit = _IN_DEGREE.get(key)
    if hit is None:
        if len(_IN_DEGREE) >= 8:
            _IN_DEGREE.clear()
        hit = _IN_DEGREE[key] = (torch.bincount(edge_index[1], minlength=num_node), edge_index)
    return hit[0]


class GeneralizedRelationalConv(nn.Module):

    eps = 1e-6

    message2mul = {
        "transe": "add",
        "distmult": "mul",
    }

    def __init__(self, input_dim, output_dim, num_relation, query_input_dim, message_func="distmult",
                 aggregate_func="pna", layer_norm=False, activation="relu", dependent=False, project_relations=False):
        super(GeneralizedRelationalConv, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.num_relation = num_relation
        self.query_input_dim = query_input_dim
        self.message_func = message_func
        self.aggregate_func = aggregate_func
        self.dependent = dependent
        self.project_relations = project_relations
        self.node_dim = -2

        if layer_norm:
            self.layer_norm = nn.LayerNorm(output_dim)
        else:
            self.layer_norm = None
        if isinstance(activation, str):
            self.activation = getattr(F, activation)
        else:
            self.activation = activation

        if self.aggregate_func == "pna":
            self.linear = nn.Linear(input_dim * 13, output_dim)
        else:
            self.linear = nn.Linear(input_dim * 2, output_dim)

        if dependent:
            self.relation_linear = nn.Linear(query_input_dim, num_relation * input_dim)
        else:
            if not self.project_relations:
                self.relation = nn.Embedding(num_relation, input_dim)
            else:
                # set by EntityNBFNet.forward from the relation-graph pass (models.py:184-185)
                self.relation = None
                self.relation_projection = nn.Sequential(
                    nn.Linear(input_dim, input_dim),
                    nn.ReLU(),
                    nn.Linear(input_dim, input_dim)
                )

    def forward(self, input, query, boundary, edge_index, edge_type, size, edge_weight=None, delta=None):
        """delta (rspmm.GraphDelta, inference only): the layer on the graph with the delta's added and without its retracted
        facts, computed on the cached plan of (edge_index, edge_type) -- _propagate_delta; where the engine does not serve that,
        on the materialised edge list."""
        if delta is not None and delta.edited:
            out = self._forward_impl(input, query, boundary, edge_index, edge_type, size, edge_weight, residual=False, delta=delta)
            if out is not None:
                return out
            # (an overlay of per-sample facts, rspmm.AssumedFacts, has no shared edge list: its edges() raises)
            extra_index, extra_type = delta.edges()
            edge_index, edge_type = delta.surviving(edge_index, edge_type)
            edge_index, edge_type = torch.cat([edge_index, extra_index], dim=1), torch.cat([edge_type, extra_type])
        return self._forward_impl(input, query, boundary, edge_index, edge_type, size, edge_weight, residual=False)

    def _forward_impl(self, input, query, boundary, edge_index, edge_type, size, edge_weight=None, residual=False,
                      relation=None, onehot_rows=None, edge_keep=False, delta=None, sample_keys=None):
        """forward() plus the option to fuse the caller's residual `hidden + layer_input` (models.py:158-160),
        to take this layer's relation features precomputed by the caller, to be told that `input` is zero
        outside row onehot_rows[b] of every sample (the layer-0 boundary condition, models.py:139-141), that
        `edge_weight` is a 0/1 keep mask (edge_keep=True: edges with 0 are absent, base_nbfnet.py:54-77), and to run on
        the graph with the added facts of `delta` (rspmm.GraphDelta; _propagate_delta) -- with `sample_keys` and 2-D keep rows:
        without each sample's own dead edges (_propagate_delta_samples)."""
        batch_size = len(query)

        if relation is None:
            relation = self._relation_for(query, batch_size)
        # edge_weight=None means "all ones" (what every caller on the fused path passes, models.py:143):
        # the kernel then skips the weight stream instead of multiplying by 1.
        if delta is not None:
            if sample_keys is not None:
                # leave-one-out on a live graph: per-sample keep rows over the base edges AND the same edges as keys
                if edge_weight is None or edge_weight.dim() != 2 or not edge_keep:
                    raise RuntimeError("`sample_keys` go with the per-sample keep rows of the base edge list (edge_keep=True)")
                return self._propagate_delta_samples(edge_index, size, input, relation, boundary, edge_type, delta, edge_weight,
                                                     sample_keys, residual=residual)
            if edge_weight is not None or edge_keep:
                raise RuntimeError("a graph delta (added facts) is combined with per-sample keep rows only through `sample_keys` "
                                   "(leave-one-out verification), not with edge weights or other keep masks")
            return self._propagate_delta(edge_index, size, input, relation, boundary, edge_type, delta, residual=residual)
        return self.propagate(input=input, relation=relation, boundary=boundary, edge_index=edge_index,
                              edge_type=edge_type, size=size, edge_weight=edge_weight, residual=residual,
                              onehot_rows=onehot_rows, edge_keep=edge_keep)

    def update_args(self, residual=False):
        """This layer's update as the engine's entry points take it: (weight, bias, ln_weight, ln_bias, eps, flags)."""
        return _lib.update_args(self.linear, self.layer_norm, self.activation is not None, residual)

    def _relation_for(self, query, batch_size):
        if self.dependent:
            return self.relation_linear(query).view(batch_size, self.num_relation, self.input_dim)
        if not self.project_relations:
            return self.relation.weight.expand(batch_size, -1, -1)   # stride-0 view, never materialised
        return self.relation_projection(self.relation)

    def layer0_point_supported(self, point, relation, edge_weight):
        """Can ultra_nbf_layer0 run this layer on a one-hot input?  (sum / DistMult, 64-d, fp32, inference)"""
        return (POINT_BOUNDARY_FAST_PATH and point.values.is_cuda and point.values.dtype == torch.float32
                and not torch.is_grad_enabled() and self.aggregate_func in ("sum", "max") and self.message_func == "distmult"
                and self.input_dim == 64 and self.output_dim == 64 and self.linear.in_features == 128
                and (self.activation is None or self.activation is F.relu)
                and (relation is None or (relation.dtype == torch.float32 and relation.shape[-1] == 64))
                and (edge_weight is None or not edge_weight.requires_grad))

    def adjacency_supported(self):
        """Can this layer run on a relation graph's byte adjacency alone (ultra_nbf_dense_layer0_adjacency as layer
        0, ultra_nbf_dense_layer_adjacency as any other)?  sum / DistMult, 64-d, fp32, its own relation embedding of at least
        the graph's four types -- what the layer is, not what a call hands it."""
        return (self.aggregate_func == "sum" and self.message_func == "distmult" and self.input_dim == 64
                and self.output_dim == 64 and self.linear.in_features == 128 and self.linear.weight.dtype == torch.float32
                and (self.activation is None or self.activation is F.relu) and not self.dependent
                and not self.project_relations and self.relation.weight.shape[0] >= 4)

    def forward_adjacency(self, adjacency, num_node, point, input=None, residual=False):
        """This layer on the byte adjacency of a live relation graph, no plan involved.  `point`: the boundary condition (a
        PointBoundary).  input=None: the boundary condition is the input too -- layer 0, evaluated in closed form."""
        relation = self._relation_for(None, len(point.rows))
        if input is None:
            return rspmm.dense_layer0_adjacency(adjacency, num_node, relation, point.rows, point.values, self.linear,
                                                self.layer_norm, relu=self.activation is not None, residual=residual)
        return rspmm.dense_layer_adjacency(adjacency, num_node, relation, input, self.linear, self.layer_norm,
                                           relu=self.activation is not None, residual=residual,
                                           point=(point.rows, point.values))

    def layer0_fill(self, edge_index, edge_type, num_node, num_relation, batch_size):
        """The constant rows of forward_layer0_point (every row that layer 0 cannot reach: relu(LayerNorm(bias))) as a fresh
        (batch, N, 64) tensor on the CURRENT stream -- they depend on this layer's parameters only, so a model may launch
        them beside whatever produces the layer's other operands and pass the tensor as `out`."""
        plan = rspmm.get_plan(edge_index, edge_type, num_node, num_relation)
        return plan.layer0_fill(batch_size, self.linear, self.layer_norm, relu=self.activation is not None,
                                device=edge_index.device)

    def forward_layer0_point(self, point, query, edge_index, edge_type, num_node, edge_weight=None, residual=False,
                             relation=None, out=None):
        """This layer applied to the boundary condition itself (what layer 0 of every NBFNet does, models.py:72-80,
        150-163), evaluated only where the result differs from relu(LayerNorm(bias))."""
        batch_size = len(point.rows)
        if relation is None:
            relation = self._relation_for(query, batch_size)
        plan = rspmm.get_plan(edge_index, edge_type, num_node, relation.shape[1])
        return plan.layer0(relation, point.rows, point.values, self.linear, self.layer_norm,
                           relu=self.activation is not None, residual=residual, edge_weight=edge_weight,
                           aggregate=self.aggregate_func, out=out)

    def propagate(self, edge_index, size=None, residual=False, onehot_rows=None, edge_keep=False, **kwargs):
        edge_weight = kwargs["edge_weight"]
        if edge_weight is not None and edge_weight.dim() == 2:
            return self._propagate_samples(edge_index, size, residual=residual, edge_keep=edge_keep, **kwargs)
        rotate_fused = self.rotate_fused(kwargs["input"], kwargs["relation"], edge_weight)
        if edge_keep and self.message_func == "rotate" and not rotate_fused:
            # the unfused scatter path needs the edges really gone: the caller removes them
            raise RuntimeError("edge_keep masks serve the fused TransE / DistMult / RotatE paths")
        if isinstance(kwargs["boundary"], PointBoundary) and (
                (edge_weight is not None and edge_weight.requires_grad) or self.message_func == "rotate"
                or self.aggregate_func not in ("sum", "max") or not kwargs["input"].is_cuda
                or (self.aggregate_func == "max" and (torch.is_grad_enabled() or edge_keep))
                or (torch.is_grad_enabled() and not self.point_boundary_trains()
                    and (kwargs["input"].requires_grad or kwargs["relation"].requires_grad
                         or kwargs["boundary"].requires_grad))):
            kwargs["boundary"] = kwargs["boundary"].dense()     # paths that need the boundary as a tensor
        if rotate_fused:
            return self._propagate_rotate(edge_index, size, residual=residual, edge_keep=edge_keep, **kwargs)
        if (edge_weight is not None and edge_weight.requires_grad) or self.message_func == "rotate":
            # layers.py:91-94: the reference's fused kernel covers TransE / DistMult with constant edge weights only
            out = self._propagate_unfused(edge_index, size, **kwargs)
            return out + kwargs["input"] if residual else out
        num_node = size[0] if size is not None else kwargs["input"].shape[1]
        fused = self._fused_dense_layer(edge_index, kwargs, num_node, residual, onehot_rows)
        if fused is not None:
            return fused
        fused = self._fused_sparse_layer(edge_index, kwargs, num_node, residual, onehot_rows, edge_keep)
        if fused is not None:
            return fused
        fused = self._training_layer(edge_index, kwargs, num_node, residual, onehot_rows, edge_keep)
        if fused is not None:
            return fused
        out = self.message_and_aggregate(edge_index, kwargs["input"], kwargs["relation"], kwargs["boundary"],
                                         kwargs["edge_type"], edge_weight, edge_index[1], num_node,
                                         onehot_rows=onehot_rows, edge_keep=edge_keep)
        return self.update(out, kwargs["input"], residual=residual)

    def _propagate_samples(self, edge_index, size, input, relation, boundary, edge_type, edge_weight, residual=False,
                           edge_keep=False):
        """The layer with one 0/1 keep mask PER SAMPLE: `edge_weight` (batch, num_edge), sample s runs on the graph without the
        edges whose keep[s] is 0 (rspmm.Plan.forward with a 2-D mask).  Inference only: aggregate, then update -- two launches,
        as every weighted inference call; the boundary condition goes in as a tensor."""
        if not edge_keep:
            raise RuntimeError("a 2-D `edge_weight` is a per-sample keep mask (edge_keep=True); per-sample weights are not served")
        if torch.is_grad_enabled():
            raise RuntimeError("per-sample keep masks serve inference (torch.no_grad()) only")
        rotate = self.message_func == "rotate"
        if self.aggregate_func == "pna" or (rotate and not self.rotate_fused(input, relation)) \
                or (not rotate and self.aggregate_func not in ("sum", "mean", "max")):
            raise RuntimeError("per-sample keep masks serve the fused sum / mean / max (RotatE: also min) paths")
        if isinstance(boundary, PointBoundary):
            boundary = boundary.dense()
        edge_weight = edge_weight.to(input.dtype)
        boundary = boundary.to(input.dtype)
        if rotate:      # (the unfused path's direction on the flipped graph: _propagate_rotate)
            num_node = size[1] if size is not None else input.shape[1]
            edges, mul = _flipped_edges(edge_index), "rotate"
        else:
            num_node = size[0] if size is not None else input.shape[1]
            edges, mul = edge_index, self.message2mul[self.message_func]
        plan = rspmm.get_plan(edges, edge_type, num_node, relation.shape[1],
                              exact_order=False if self._order_free(edge_index, num_node) else None)
        sum = {"sum": "add", "mean": "add"}.get(self.aggregate_func, self.aggregate_func)
        update = plan.forward(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum, mul=mul, keep=True)
        if self.aggregate_func == "mean":
            # the degree of each sample's own graph (+ 1: the boundary's self loop), counted at edge_index[1] like the shared mask
            degree = torch.zeros(len(edge_weight), num_node, dtype=input.dtype, device=input.device).index_add_(
                1, edge_index[1], edge_weight)
            update = update / (degree + 1).unsqueeze(-1)
        return self.update(update, input, residual=residual)

    def delta_supported(self):
        """Does _propagate_delta serve this layer's configuration?  (sum / mean / max / min with TransE or DistMult)"""
        return self.aggregate_func in ("sum", "mean", "max", "min") and self.message_func in self.message2mul

    def _propagate_delta(self, edge_index, size, input, relation, boundary, edge_type, delta, residual=False):
        """The layer on the graph WITH the added and WITHOUT the retracted facts of `delta` (rspmm.GraphDelta), on the cached plan
        of the base graph: the aggregate by plan.forward (the two-launch form: the one-launch layer would update rows before they
        are fixed), then plan.delta_rows -- plan.edit_rows once the delta holds tombstones -- which recomputes the rows an added
        or a removed edge points into in the reference's order, then the update.  Equals
        the layer on delta.materialize(...) bit for bit.  Inference only; sum / mean / max / min, TransE / DistMult; a dense or a
        point boundary (layer 0 included: its closed form does not know the delta).  Returns None where the engine does not
        serve the call (a re-associating or dense-format plan, misaligned rows): the caller materialises."""
        if torch.is_grad_enabled():
            raise RuntimeError("a graph delta (added facts) serves inference (torch.no_grad()) only")
        if not self.delta_supported():
            raise RuntimeError("a graph delta (added facts) serves the sum / mean / max / min aggregates with TransE / DistMult "
                               "messages, not `%s` / `%s`" % (self.aggregate_func, self.message_func))
        num_node = size[0] if size is not None else input.shape[1]
        if not input.is_cuda or self._order_free(edge_index, num_node):
            return None
        plan = rspmm.get_plan(edge_index, edge_type, num_node, relation.shape[1])
        sum = {"sum": "add", "mean": "add"}.get(self.aggregate_func, self.aggregate_func)
        mul = self.message2mul[self.message_func]
        if getattr(delta, "per_query_owned", False):
            # an overlay of facts assumed per sample (rspmm.AssumedFacts): the owned entry, one launch with both
            # roles, tombstones or none.  `mean` would need a per-sample degree: not served
            if self.aggregate_func == "mean":
                return None
            fix_rows = plan.edit_rows_owned
        elif rspmm.EDIT_ROWS_HUB_SPLIT and plan.has_hub_rows:      # (the same rows, the same bits: hub rows by a workgroup each)
            fix_rows = plan.edit_rows_split
        else:
            fix_rows = plan.edit_rows if delta.num_removed else plan.delta_rows
        update = None
        if isinstance(boundary, PointBoundary):
            point = (boundary.rows, boundary.values)
            update = plan.forward(relation, input, sum=sum, mul=mul, point=point)
            if update is not None:
                update = fix_rows(relation, input, update, delta, sum=sum, mul=mul, point=point)
            else:       # (a plan that does not serve the point form under min / max: the boundary as a tensor)
                boundary = boundary.dense()
        if update is None:
            if isinstance(boundary, PointBoundary):
                return None
            boundary = boundary.to(input.dtype)
            update = plan.forward(relation, input, boundary=boundary, sum=sum, mul=mul)
            update = fix_rows(relation, input, update, delta, boundary=boundary, sum=sum, mul=mul)
            if update is None:
                return None
        if self.aggregate_func == "mean":
            # bincount(edge_index[1]) of the materialised list (+ 1: the boundary's self loop), as message_and_aggregate counts it
            # (delta.degree is signed: added minus retracted edges)
            degree = _in_degree(edge_index, num_node) + delta.degree
            update = update / (degree.to(input.dtype) + 1).view(1, -1, 1)
        return self.update(update, input, residual=residual)

    def delta_samples_supported(self):
        """Does _propagate_delta_samples serve this layer's configuration?  (sum / max with TransE or DistMult: what
        _propagate_samples and _propagate_delta both serve, minus `mean`, whose per-sample degree of the materialised list is
        not built)"""
        return self.aggregate_func in ("sum", "max") and self.message_func in self.message2mul

    def _propagate_delta_samples(self, edge_index, size, input, relation, boundary, edge_type, delta, edge_weight, sample_keys,
                                 residual=False):
        """The layer on the graph with `delta`'s edits where sample s does not see a few edges of its own (leave-one-out
        verification on a live graph): `edge_weight` (batch, num_edge) are the 0/1 keep rows over the BASE edge list
        (BaseNBFNet.leave_one_out_keep), `sample_keys` = (row, col, type) name the same edges for the rows an edit points into,
        base and delta edges alike (GraphDelta.sample_keys).  The aggregate by plan.forward with the keep rows -- right for
        every row no edit points into -- then plan.edit_rows_samples on the same buffer with the same dense boundary, which
        recomputes the touched rows of every sample without that sample's dead edges, then the update.  Equals the layer on
        delta.materialize(...) filtered per sample, bit for bit.  Inference only; sum / max, TransE / DistMult.  Returns None
        where the engine does not serve the call: the caller runs sample by sample on the materialised graph."""
        if torch.is_grad_enabled():
            raise RuntimeError("a graph delta with per-sample keep masks serves inference (torch.no_grad()) only")
        if not self.delta_samples_supported():
            raise RuntimeError("a graph delta with per-sample keep masks serves the sum / max aggregates with TransE / DistMult "
                               "messages, not `%s` / `%s`" % (self.aggregate_func, self.message_func))
        num_node = size[0] if size is not None else input.shape[1]
        if not input.is_cuda or self._order_free(edge_index, num_node):
            return None
        if isinstance(boundary, PointBoundary):
            boundary = boundary.dense()
        edge_weight = edge_weight.to(input.dtype)
        boundary = boundary.to(input.dtype)
        plan = rspmm.get_plan(edge_index, edge_type, num_node, relation.shape[1])
        if not plan.exact:
            return None
        sum = {"sum": "add"}.get(self.aggregate_func, self.aggregate_func)
        mul = self.message2mul[self.message_func]
        update = plan.forward(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum, mul=mul, keep=True)
        if rspmm.EDIT_ROWS_HUB_SPLIT and plan.has_hub_rows:
            update = plan.edit_rows_split(relation, input, update, delta, keys=sample_keys, boundary=boundary, sum=sum, mul=mul)
        else:
            update = plan.edit_rows_samples(relation, input, update, delta, sample_keys, boundary=boundary, sum=sum, mul=mul)
        if update is None:
            return None
        return self.update(update, input, residual=residual)

    def edge_grad_layer(self, input, query, boundary, edge_index, edge_type, num_node, edge_weight, residual=False,
                        relation=None):
        """The layer on the unfused path's direction (messages from edge_index[0] into edge_index[1], layers.py:135-181) with
        differentiable edge weights, through the plan-based rspmm over the flipped graph: d output / d edge_weight comes from
        ultra_rspmm_backward's weight gradient.  What BaseNBFNet.visualize asks for; sum / DistMult, fp32 on the GPU only
        (None otherwise: the caller keeps the unfused route)."""
        if not (self.aggregate_func == "sum" and self.message_func == "distmult" and input.is_cuda
                and input.dtype == torch.float32 and input.dim() == 3 and input.shape[0] == 1):
            return None
        if relation is None:
            relation = self._relation_for(query, len(query))
        if isinstance(boundary, PointBoundary):
            boundary = boundary.dense()
        plan = rspmm.get_plan(_flipped_edges(edge_index), edge_type, num_node, relation.shape[1], exact_order=False)
        # (one sample: the 2-D (N, d) operands of the reference kernel's layout)
        update = rspmm.plan_rspmm(plan, relation[0], input[0], edge_weight, sum="add", mul="mul", boundary=boundary[0])
        return self.update(update.unsqueeze(0), input, residual=residual)

    def edge_grad_layer_batch(self, input, query, boundary, edge_index, edge_type, num_node, residual=False, relation=None,
                              delta=None):
        """edge_grad_layer for S independent samples at once -- (S, N, d) operands, the same flipped-graph plan, CONSTANT unit
        edge weights: a batched backward would sum the weight gradient over the samples, which explains none of them.  The
        aggregate `update` is kept instead; with its gradient u the per-sample weight gradient of this layer is
        plan.edge_grad_samples(relation, input, u) (ultra_rspmm_edge_grad_samples).  Returns (hidden, (plan, relation, input,
        update)); None where edge_grad_layer would return None for a sample (the caller then explains triple by triple).
        `delta` (an edited rspmm.GraphDelta of this graph): the aggregate on (graph, delta) -- without the tombstoned edges,
        with the added ones -- on the same plan of the base graph (rspmm.plan_delta_rspmm); the relation is then a constant, and
        the added edges' gradients are delta.delta_edge_grad_samples(relation, input, u)."""
        if not (self.aggregate_func == "sum" and self.message_func == "distmult" and input.is_cuda
                and input.dtype == torch.float32 and input.dim() == 3):
            return None
        if relation is None:
            relation = self._relation_for(query, len(query))
        if relation.dtype != torch.float32 or relation.dim() != 3 or relation.shape[0] != input.shape[0]:
            return None
        if isinstance(boundary, PointBoundary):
            boundary = boundary.dense()
        plan = rspmm.get_plan(_flipped_edges(edge_index), edge_type, num_node, relation.shape[1], exact_order=False)
        if delta is not None and delta.edited:
            relation = relation.detach()
            update = rspmm.plan_delta_rspmm(plan, delta, relation, input, boundary)
        else:
            update = rspmm.plan_rspmm(plan, relation, input, None, sum="add", mul="mul", boundary=boundary)
        if not update.requires_grad:      # (frozen parameters: nothing upstream asks for a gradient, this tensor still does)
            update.requires_grad_()
        return self.update(update, input, residual=residual), (plan, relation, input, update)

    def explain_live_supported(self):
        """Does edge_grad_layer_batch(delta=) serve this layer's configuration?  (sum / DistMult: the batched explanation route)"""
        return self.aggregate_func == "sum" and self.message_func == "distmult"

    def point_boundary_trains(self):
        """The differentiable rspmm takes the boundary condition in closed form for the sum aggregate (rspmm._PlanRSPMM,
        rspmm._OnehotRSPMM): no (batch, N, d) boundary gradient is formed, layer 0 walks the sources' edges only."""
        return POINT_BOUNDARY_TRAINING and self.aggregate_func == "sum" and self.message_func in self.message2mul

    def _fused_dense_layer(self, edge_index, kwargs, num_node, residual, onehot_rows):
        """Aggregate + update in one launch where the graph has a dense-format plan (ULTRA's relation graph)."""
        input, relation, boundary = kwargs["input"], kwargs["relation"], kwargs["boundary"]
        if not (FUSED_DENSE_LAYER and kwargs["edge_weight"] is None and self.aggregate_func == "sum"
                and self.message_func == "distmult" and input.is_cuda and not torch.is_grad_enabled()
                and onehot_rows is None and dense.conv_update_supported(self, input, input)):
            return None
        plan = rspmm.get_plan(edge_index, kwargs["edge_type"], num_node, relation.shape[1])
        if plan.dense is None:
            return None
        point = (boundary.rows, boundary.values) if isinstance(boundary, PointBoundary) else None
        return plan.fused_layer(relation, input, self.linear, self.layer_norm, relu=self.activation is not None,
                                residual=residual, boundary=None if point is not None else boundary, point=point)

    def _order_free(self, edge_index, num_node):
        """max (and min) do not depend on the order of their operands (but for the sign of a zero), so a graph whose rows are
        mostly long -- ULTRA's relation graph: every row has hundreds of edges, each a serial chain on the reference-order
        kernels -- goes to the re-associating plan, which splits such rows over many lanes, and still returns the
        reference's values."""
        return self.aggregate_func == "max" and edge_index.shape[1] >= 128 * max(int(num_node), 1)

    def _fused_sparse_layer(self, edge_index, kwargs, num_node, residual, onehot_rows, edge_keep):
        """Aggregate + update in one launch on the reference-order plan of a sparse graph (the entity graph): the workgroup
        that sums a row also applies the layer update to it (ultra_rspmm_forward_update).  Same bits as the two launches."""
        input, relation, boundary = kwargs["input"], kwargs["relation"], kwargs["boundary"]
        if not (FUSED_SPARSE_LAYER and kwargs["edge_weight"] is None and self.aggregate_func in ("sum", "max")
                and self.message_func in self.message2mul and input.is_cuda and not torch.is_grad_enabled()
                and onehot_rows is None and not edge_keep and isinstance(boundary, PointBoundary)
                and input.dim() == 3 and relation.dtype == torch.float32 and dense.conv_update_supported(self, input, input)
                and not self._order_free(edge_index, num_node)):
            return None
        plan = rspmm.get_plan(edge_index, kwargs["edge_type"], num_node, relation.shape[1])
        return plan.forward_update(relation, input, *self.update_args(residual),
                                   mul=self.message2mul[self.message_func], point=(boundary.rows, boundary.values),
                                   sum="add" if self.aggregate_func == "sum" else "max")

    def _training_layer(self, edge_index, kwargs, num_node, residual, onehot_rows, edge_keep):
        """Aggregate + update of a training step's layer as one autograd node (dense.TrainLayerFunction): the layer input's two
        gradient shares -- through the rspmm and through the update -- leave the backward already summed.  Sum aggregate,
        TransE / DistMult, the ULTRA update shape; layer 0 (one-hot input) has its own route in message_and_aggregate."""
        input, relation, boundary, edge_weight = kwargs["input"], kwargs["relation"], kwargs["boundary"], kwargs["edge_weight"]
        point = boundary if isinstance(boundary, PointBoundary) else None
        if not (TRAINING_LAYER_NODE and torch.is_grad_enabled() and onehot_rows is None and self.aggregate_func == "sum"
                and self.message_func in self.message2mul and input.is_cuda and input.dim() == 3
                and input.dtype == torch.float32 and relation.dtype == torch.float32
                and (edge_weight is None or (not edge_weight.requires_grad and edge_weight.dtype == torch.float32))
                and (input.requires_grad or relation.requires_grad or boundary.requires_grad)
                and (point is not None or boundary.dtype == torch.float32)
                and dense.conv_update_supported(self, input, input)):
            return None
        plan = rspmm.get_plan(edge_index, kwargs["edge_type"], num_node, relation.shape[1], exact_order=False)
        weight, bias, ln_weight, ln_bias, eps, flags = self.update_args(residual)
        return dense.TrainLayerFunction.apply(
            plan, self.message2mul[self.message_func], bool(edge_keep), eps, flags,
            edge_weight, relation, input, None if point is not None else boundary,
            point.rows if point is not None else None, point.values if point is not None else None,
            weight, bias, ln_weight, ln_bias)

    def training_rows_layer(self, input, query, boundary, edge_index, edge_type, num_node, rows, edge_weight=None, residual=False,
                            relation=None):
        """This layer's output at the listed rows only -- (batch, n_list, 64) for rows (batch, n_list) -- as one autograd node
        (dense.TrainRowsLayerFunction): what the LAST layer of a training step needs, since the readout reads the candidates'
        rows alone (models.py:202-207).  None where the route does not apply (the caller then runs the whole layer)."""
        if relation is None:
            relation = self._relation_for(query, len(query))
        point = boundary if isinstance(boundary, PointBoundary) else None
        if not (LAST_LAYER_ON_ROWS and torch.is_grad_enabled() and self.aggregate_func == "sum"
                and self.message_func in self.message2mul and input.is_cuda and input.dim() == 3 and rows.dim() == 2
                and 4 * rows.shape[1] <= num_node         # (a list that covers most of the graph: the whole layer's walk is the better one)
                and input.dtype == torch.float32 and relation.dtype == torch.float32
                and (edge_weight is None or (not edge_weight.requires_grad and edge_weight.dtype == torch.float32))
                and (input.requires_grad or relation.requires_grad or boundary.requires_grad)
                and (point is not None or (boundary.dtype == torch.float32 and not boundary.requires_grad))
                and (point is None or point.values.dtype == torch.float32)
                and dense.conv_update_supported(self, input, input)):
            return None
        plan = rspmm.get_plan(edge_index, edge_type, num_node, relation.shape[1], exact_order=False)
        weight, bias, ln_weight, ln_bias, eps, flags = self.update_args(residual)
        return dense.TrainRowsLayerFunction.apply(
            plan, self.message2mul[self.message_func], eps, flags, edge_weight, relation, input,
            rows, None if point is not None else boundary, point.rows if point is not None else None,
            point.values if point is not None else None, weight, bias, ln_weight, ln_bias)

    # ---- RotatE through the engine, in the unfused path's direction ----
    def rotate_fused(self, input, relation, edge_weight=None):
        """Does this layer's `rotate` message run on the rspmm engine?  sum / mean / max / min, GPU tensors, constant edge
        weights, an even feature dim (pna needs the squared MESSAGE, and (r x)^2 = r^2 x^2 does not hold for a complex
        product: it stays unfused, like differentiable edge weights and CPU tensors)."""
        return (FUSED_ROTATE and self.message_func == "rotate" and self.aggregate_func in ("sum", "mean", "max", "min")
                and input.is_cuda and input.dim() == 3 and input.shape[-1] % 2 == 0
                and input.dtype in (torch.float32, torch.float64) and relation.dtype == input.dtype
                and (edge_weight is None or not edge_weight.requires_grad))

    def _propagate_rotate(self, edge_index, size, input, relation, boundary, edge_type, edge_weight, residual=False,
                          edge_keep=False):
        """The reference runs `rotate` unfused: messages gathered at edge_index[0], aggregated into edge_index[1] together with
        one boundary self-loop per node (layers.py:135-181).  The same on the engine: the plan of the FLIPPED edge list, the
        boundary fused as the walk's last operand -- on a reference-order plan the sum is the CPU scatter_add_'s on an edge list
        sorted by (target, source, id), bit for bit.  No (batch, |E|, d) tensor is formed."""
        num_target = size[1] if size is not None else input.shape[1]
        if edge_weight is not None and edge_weight.dtype != input.dtype:
            edge_weight = edge_weight.to(input.dtype)
        if boundary.dtype != input.dtype:
            boundary = boundary.to(input.dtype)
        needs_grad = torch.is_grad_enabled() and (input.requires_grad or relation.requires_grad or boundary.requires_grad)
        flipped = _flipped_edges(edge_index)
        # (as message_and_aggregate: reference order under no_grad, the re-associating plan for a training step)
        plan = rspmm.get_plan(flipped, edge_type, num_target, relation.shape[1],
                              exact_order=False if (needs_grad or self._order_free(edge_index, num_target)) else None)
        sum = {"sum": "add", "mean": "add"}.get(self.aggregate_func, self.aggregate_func)
        if not needs_grad:
            update = plan.forward(relation, input, edge_weight=edge_weight, boundary=boundary, sum=sum, mul="rotate", keep=edge_keep)
        elif sum == "add":
            update = rspmm.plan_rspmm(plan, relation, input, edge_weight, sum=sum, mul="rotate", boundary=boundary, keep=edge_keep)
        else:
            update = rspmm.plan_rspmm(plan, relation, input, edge_weight, sum=sum, mul="rotate", keep=edge_keep)
            update = torch.max(update, boundary) if sum == "max" else torch.min(update, boundary)
        if self.aggregate_func == "mean":
            # scatter(..., "mean") over the in-edges + the self loop; under a keep mask the kept edges only
            if edge_keep and edge_weight is not None:
                degree = torch.zeros(num_target, dtype=input.dtype, device=input.device).index_add_(
                    0, edge_index[1], edge_weight.detach())
            else:
                degree = torch.bincount(edge_index[1], minlength=num_target).to(input.dtype)
            update = update / (degree + 1).view(1, -1, 1)
        return self.update(update, input, residual=residual)

    # ---- unfused path: gather edge_index[0], scatter to edge_index[1] -- PyG's direction (layers.py:135-181) ----
    def _propagate_unfused(self, edge_index, size, input, relation, boundary, edge_type, edge_weight):
        num_target = size[1] if size is not None else input.shape[1]
        if edge_weight is None:
            edge_weight = torch.ones(edge_index.shape[1], device=input.device, dtype=input.dtype)
        message = self.message(input.index_select(self.node_dim, edge_index[0]), relation, boundary, edge_type)
        return self.update(self.aggregate(message, edge_weight, edge_index[1], num_target), input)

    @staticmethod
    def _combine(message_func, source, relation):
        """One message per edge from its source state and relation feature (layers.py:138-151)."""
        if message_func == "transe":
            return source + relation
        if message_func == "distmult":
            return source * relation
        if message_func == "rotate":         # complex product on (real | imaginary) halves
            s_re, s_im = source.chunk(2, dim=-1)
            r_re, r_im = relation.chunk(2, dim=-1)
            return torch.cat([s_re * r_re - s_im * r_im, s_re * r_im + s_im * r_re], dim=-1)
        raise ValueError("Unknown message function `%s`" % message_func)

    def message(self, input_j, relation, boundary, edge_type):
        edges = self._combine(self.message_func, input_j, relation.index_select(self.node_dim, edge_type))
        # the boundary condition rides along as one self-loop message per node (layers.py:153-155)
        return torch.cat([edges, boundary], dim=self.node_dim)

    def aggregate(self, input, edge_weight, index, dim_size):
        # the self-loop messages appended by message(): target = the node itself, weight 1
        loops = torch.arange(dim_size, device=input.device)
        index = torch.cat([index, loops])
        weight = torch.cat([edge_weight, torch.ones(dim_size, device=input.device, dtype=edge_weight.dtype)]).view(1, -1, 1)
        weighted = input * weight
        if self.aggregate_func != "pna":
            return _scatter(weighted, index, dim_size, self.aggregate_func)
        degree = torch.bincount(index, minlength=dim_size).to(input.dtype).view(1, -1, 1)
        return self._pna(_scatter(weighted, index, dim_size, "mean"), _scatter(input ** 2 * weight, index, dim_size, "mean"),
                         _scatter(weighted, index, dim_size, "max"), _scatter(weighted, index, dim_size, "min"), degree)

    def _pna(self, mean, sq_mean, maximum, minimum, degree):
        """Principal neighbourhood aggregation (layers.py:165-179, 208-226): [mean, max, min, std] x [1, s, 1 / s] with
        s = log(degree) / mean(log(degree)); (batch, node, 12 d) in the reference's feature order."""
        std = (sq_mean - mean ** 2).clamp(min=self.eps).sqrt()
        stats = torch.stack([mean, maximum, minimum, std], dim=-1).flatten(-2)      # (batch, node, 4 d), statistic fastest
        scale = degree.log()
        scale = scale / scale.mean()
        scalers = torch.cat([torch.ones_like(scale), scale, 1 / scale.clamp(min=1e-2)], dim=-1)      # (1, node, 3)
        return (stats.unsqueeze(-1) * scalers.unsqueeze(-2)).flatten(-2)

    # ---- fused path ----
    def message_and_aggregate(self, edge_index, input, relation, boundary, edge_type, edge_weight, index, dim_size,
                              onehot_rows=None, edge_keep=False):
        """(batch, N, d) in, (batch, N, d') out.  Aggregates into edge_index[0] from edge_index[1]
        (the fused kernel's direction, rspmm.cpp:143-145) -- not the unfused path's direction."""
        batch_size, num_node = input.shape[:2]
        if self.message_func in self.message2mul:
            mul = self.message2mul[self.message_func]
        else:
            raise ValueError("Unknown message function `%s`" % self.message_func)
        if edge_weight is not None and not torch.is_floating_point(edge_weight):
            edge_weight = edge_weight.to(input.dtype)
        needs_grad = torch.is_grad_enabled() and (input.requires_grad or relation.requires_grad or
                                                   boundary.requires_grad)
        # a differentiable call (training step) takes the re-associating plan: its backward is a scatter-add and its
        # result feeds a stochastic optimiser step -- there is no reference summation order to reproduce
        plan = rspmm.get_plan(edge_index, edge_type, num_node, relation.shape[1],
                              exact_order=False if (needs_grad or self._order_free(edge_index, num_node)) else None)

        point, point_boundary = None, None
        if isinstance(boundary, PointBoundary):     # (propagate() only lets it through for the fused sum / max paths)
            point, point_boundary, boundary = (boundary.rows, boundary.values), boundary, None

        def agg(sum, rel=relation, x=input, fuse_boundary=None):
            if point is not None and needs_grad:
                # (propagate() lets the closed form through under autograd for the sum aggregate only)
                return rspmm.plan_rspmm(plan, rel, x, edge_weight, sum=sum, mul=mul, keep=edge_keep, point=point)
            if point is not None:
                out = plan.forward(rel, x, edge_weight=edge_weight, sum=sum, mul=mul, point=point)
                if out is not None:
                    return out
                # (a plan that does not serve the point form under min / max: the boundary as a tensor)
                return plan.forward(rel, x, edge_weight=edge_weight, boundary=point_boundary.dense(), sum=sum, mul=mul)
            if needs_grad:
                if sum == "add":      # boundary added in the kernel's epilogue; its gradient is the output gradient
                    return rspmm.plan_rspmm(plan, rel, x, edge_weight, sum=sum, mul=mul, boundary=fuse_boundary,
                                            keep=edge_keep)
                out = rspmm.plan_rspmm(plan, rel, x, edge_weight, sum=sum, mul=mul, keep=edge_keep)
                if fuse_boundary is None:
                    return out
                return torch.max(out, fuse_boundary) if sum == "max" else torch.min(out, fuse_boundary)
            return plan.forward(rel, x, edge_weight=edge_weight, boundary=fuse_boundary, sum=sum, mul=mul, keep=edge_keep)

        if self.aggregate_func in ("mean", "pna"):
            # layers.py:193 -- PyG's `index` is edge_index[1]; under a keep mask the degree counts the kept edges only
            # (what bincount gives on the reference's filtered copy of the graph, base_nbfnet.py:54-77)
            if edge_keep and edge_weight is not None:
                degree_out = torch.zeros(dim_size, dtype=input.dtype, device=input.device).index_add_(
                    0, index, edge_weight.detach().to(input.dtype))
            else:
                degree_out = torch.bincount(index, minlength=dim_size).to(input.dtype)
            degree_out = (degree_out + 1).view(1, -1, 1)

        if (ONEHOT_FAST_PATH and onehot_rows is not None and needs_grad and point is not None and self.aggregate_func == "sum"
                and mul == "mul" and input.is_cuda and input.dtype == torch.float32 and dim_size == input.shape[1]
                and (edge_weight is None or not edge_weight.requires_grad)):
            # layer 0 of a training step: `input` IS the boundary condition as a tensor (the caller's contract for
            # onehot_rows beside a PointBoundary) -- forward and backward visit the sources' out-edges only
            update = rspmm.onehot_rspmm(plan, edge_index, edge_type, relation, point[0], point[1], input, edge_weight)
        elif (ONEHOT_FAST_PATH and onehot_rows is not None and not needs_grad and self.aggregate_func == "sum"
                and mul == "mul" and input.is_cuda and point is None):
            # row-sparse input (layer 0): only the edges leaving the source rows contribute to a sum of products
            update = plan.forward_onehot(relation, input, onehot_rows, edge_weight=edge_weight, boundary=boundary)
        elif self.aggregate_func == "sum":
            update = agg("add", fuse_boundary=boundary)
        elif self.aggregate_func == "mean":
            update = agg("add", fuse_boundary=boundary) / degree_out
        elif self.aggregate_func == "max":
            update = agg("max", fuse_boundary=boundary)
        elif self.aggregate_func == "pna":
            # four rspmm calls: sum and sum of squares (relation and input squared: (r x)^2 = r^2 x^2), max, min
            total = agg("add")
            sq_total = agg("add", rel=relation ** 2, x=input ** 2)
            update = self._pna((total + boundary) / degree_out, (sq_total + boundary ** 2) / degree_out,
                               agg("max", fuse_boundary=boundary), agg("min", fuse_boundary=boundary), degree_out)
        else:
            raise ValueError("Unknown aggregation function `%s`" % self.aggregate_func)
        return update

    def update(self, update, input, residual=False):
        if dense.conv_update_supported(self, input, update):
            # one MFMA kernel: Linear(cat[input, update]) -> LayerNorm -> ReLU (-> + input)
            return dense.conv_update(self, input, update, residual)
        output = self.linear(torch.cat([input, update], dim=-1))
        if self.layer_norm:
            output = self.layer_norm(output)
        if self.activation:
            output = self.activation(output)
        if residual:
            output = output + input
        return output
