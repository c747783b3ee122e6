"""Ultra / RelNBFNet / EntityNBFNet / QueryNBFNet on the MI355X engine.

Drop-in for the reference's ultra/models.py + ultra/base_nbfnet.py (hot-path part): same class
names, constructor arguments, forward signatures and state-dict keys, so
`model.load_state_dict(torch.load(ckpt)["model"])` works unchanged (script/run.py:257-258).
`data` is duck-typed: .edge_index, .edge_type, .num_nodes, .num_relations, .relation_graph.
EntityNBFNet.visualize / beam_search_distance / topk_average_length (base_nbfnet.py:156-263) explain one prediction with
its top paths: ultra_amd.explain (HIP beam search); Ultra.visualize is the same from the full model.
"""
import contextlib
import copy
import threading
from collections.abc import Sequence

import torch
from torch import autograd, nn

from . import dense, explain, layers, rspmm, tasks


# inference fast path of EntityNBFNet.forward: fused batch prologue + readout from the raw batch (A/B switch for tests)
PROLOGUE_FAST_PATH = True
# the constant rows of the entity model's layer 0 are written on a side stream beside the relation model (EntityNBFNet.prefill_layer0)
# (measured on MI355X, tools/step_probe.py: the fork / join of the side stream inside the captured graph costs more than the
# 11 us of fill it hides -- 0.717 vs 0.687 ms per step one batch at a time, 0.631 vs 0.621 two in flight -- so: off)
PREFILL_LAYER0 = False
_capture_flags = threading.local()


@contextlib.contextmanager
def capture_generic_path():
    """with capture_generic_path(): ... -- inside, a hipGraph capture made by THIS thread may record the generic (training) path of
    EntityNBFNet.forward (train.GraphedTrainStep around its capture); off again afterwards, whatever happens."""
    _capture_flags.generic = True
    try:
        yield
    finally:
        _capture_flags.generic = False


def generic_path_capturable():
    return getattr(_capture_flags, "generic", False)
# the six relation_projection MLPs of a training step as one autograd node (A/B switch for tests: two batched torch products are the other side)
RELATION_PROJECTION_NODE = True
# the training step's 0/1 edge vector straight from the batch's triples (dense.easy_edge_keep; A/B switch for tests: off = the
# list of easy edges, its sorted keys and dense.edge_keep_mask)
EASY_EDGE_KEEP_KERNEL = True
# ... and for the batches neither of the LDS routes takes (> 8,192 keys): dense.easy_edge_keep_table (A/B switch for tests: off =
# tasks.edge_match, a host synchronisation)
EASY_EDGE_TABLE_KERNEL = True


class NotOnFusedPath(RuntimeError):
    """Raised when a hipGraph capture reaches a forward that is outside the fused inference path (the only thing the
    evaluation loop falls back to eager launches for -- HIP errors, out-of-memory and engine errors propagate)."""


def index_to_mask(index, size):
    mask = torch.zeros(size, dtype=torch.bool, device=index.device)
    mask[index] = True
    return mask


class BaseNBFNet(nn.Module):
    """base_nbfnet.py:11-52 (constructor) and 54-86 (edge removal, head->tail conversion)."""

    def __init__(self, input_dim, hidden_dims, num_relation, message_func="distmult", aggregate_func="sum",
                 short_cut=False, layer_norm=False, activation="relu", concat_hidden=False, num_mlp_layer=2,
                 dependent=False, remove_one_hop=False, num_beam=10, path_topk=10, **kwargs):
        super(BaseNBFNet, self).__init__()

        if not isinstance(hidden_dims, Sequence):
            hidden_dims = [hidden_dims]

        self.dims = [input_dim] + list(hidden_dims)
        self.num_relation = num_relation
        self.short_cut = short_cut
        self.concat_hidden = concat_hidden
        self.remove_one_hop = remove_one_hop
        self.num_beam = num_beam
        self.path_topk = path_topk

        self.message_func = message_func
        self.aggregate_func = aggregate_func
        self.layer_norm = layer_norm
        self.activation = activation
        self.num_mlp_layers = num_mlp_layer

    # ---- dynamic edge dropout of the training step (base_nbfnet.py:54-77): the batch's own triples and their inverses ----
    def _easy_edges(self, data, h_index, t_index, r_index):
        """Rows [heads; tails(; types)] of the edges to drop: every (h, t, r) of the batch and its inverse (t, h, r + R/2);
        with `remove_one_hop` every edge between the two nodes whatever its type."""
        heads = torch.cat([h_index, t_index], dim=-1)
        tails = torch.cat([t_index, h_index], dim=-1)
        if self.remove_one_hop:
            return torch.stack([heads, tails]).flatten(1)
        types = torch.cat([r_index, r_index + data.num_relations // 2], dim=-1)
        return torch.stack([heads, tails, types]).flatten(1)

    def easy_edge_mask(self, data, h_index, t_index, r_index=None):
        """True for the edges base_nbfnet.py:54-77 keeps, False for the batch's own (h, t[, r]) edges and inverses."""
        graph = data.edge_index if self.remove_one_hop else torch.cat([data.edge_index, data.edge_type.unsqueeze(0)])
        dropped = tasks.edge_match(graph, self._easy_edges(data, h_index, t_index, r_index))[0]
        return ~index_to_mask(dropped, data.num_edges)

    def easy_edge_keep(self, data, h_index, t_index, r_index, dtype=torch.float32):
        """easy_edge_mask as the 0/1 float vector the rspmm kernels read (dense.easy_edge_keep: one kernel on the GPU, the
        batch's triples hashed in LDS; dense.edge_keep_mask -- a sorted list of keys -- for batches it does not take)."""
        if EASY_EDGE_KEEP_KERNEL and data.edge_index.is_cuda:
            keep = dense.easy_edge_keep(data.edge_index, None if self.remove_one_hop else data.edge_type, h_index, t_index,
                                        r_index, data.num_nodes, data.num_relations, dtype)
            if keep is not None:
                return rspmm.tag_edge_weight(keep)
        easy = self._easy_edges(data, h_index, t_index, r_index)
        if data.edge_index.is_cuda and data.edge_index.dtype == torch.int64 and easy.shape[1] <= dense.EDGE_KEEP_MAX_EASY:
            keep = dense.edge_keep_mask(data.edge_index, None if self.remove_one_hop else data.edge_type, easy,
                                        data.num_nodes, data.num_relations, dtype)
            # (one vector for every layer's forward and backward walks of this step: permuted into each plan's order once)
            return rspmm.tag_edge_weight(keep)
        if EASY_EDGE_TABLE_KERNEL and data.edge_index.is_cuda:
            # batches above both LDS routes' 8,192 keys (pre-training's 64 x 513): the keys in a global hash table, no host
            # synchronisation (edge_match reads its match count back, which no captured step can do)
            keep = dense.easy_edge_keep_table(data.edge_index, None if self.remove_one_hop else data.edge_type, h_index,
                                              t_index, r_index, data.num_nodes, data.num_relations, dtype)
            if keep is not None:
                return rspmm.tag_edge_weight(keep)
        return self.easy_edge_mask(data, h_index, t_index, r_index).to(dtype)

    # ---- leave-one-out verification: one keep row per stated fact ----
    def leave_one_out_mask(self, data, h_index, t_index, r_index):
        """The torch restatement of leave_one_out_keep (any device): row s is easy_edge_mask of the single triple s as 0/1 fp32."""
        rows = [self.easy_edge_mask(data, h_index[s:s + 1], t_index[s:s + 1], r_index[s:s + 1]) for s in range(len(h_index))]
        if not rows:
            return torch.ones(0, data.edge_index.shape[1], dtype=torch.float32, device=data.edge_index.device)
        return torch.stack(rows).to(torch.float32)

    def leave_one_out_keep(self, data, triples, out=None, validate=True):
        """(n, num_edge) fp32: row s is the 0/1 keep mask of `data`'s edge list WITHOUT the stated fact s = triples[s] = (h, t, r)
        and its inverse (t, h, r + num_relations // 2) -- _easy_edges of that single triple; with `remove_one_hop` without
        every edge between h and t.  All duplicates of an edge go; a triple that is not in the graph gives a row of ones.  r
        must be a direct relation (ValueError otherwise; validate=False skips that host read -- a captured step's caller has
        checked its ids already).  GPU: ultra_leave_one_out_keep, one launch into `out` if given; elsewhere the torch
        restatement via tasks.edge_match."""
        if triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError("Expected triples of shape (n, 3) = (h, t, r), got %s" % (tuple(triples.shape),))
        h_index, t_index, r_index = triples.unbind(-1)
        if validate and triples.numel() and bool(((r_index < 0) | (r_index >= data.num_relations // 2)).any()):
            raise ValueError("leave-one-out verification takes direct relations (r < num_relations // 2 = %d); a fact stated "
                             "through an inverse relation is its direct twin" % (data.num_relations // 2))
        if data.edge_index.is_cuda:
            keep = dense.leave_one_out_keep(data.edge_index, None if self.remove_one_hop else data.edge_type, h_index, t_index,
                                            r_index, data.num_nodes, data.num_relations, out=out)
            if keep is not None:
                return keep
        keep = self.leave_one_out_mask(data, h_index, t_index, r_index)
        if out is not None:
            out[:keep.shape[0], :keep.shape[1]].copy_(keep)
            return out[:keep.shape[0], :keep.shape[1]]
        return keep

    def remove_easy_edges(self, data, h_index, t_index, r_index=None):
        """The reference's route: a filtered copy of the graph (only `rotate` off the engine still needs it: layers.rotate_fused)."""
        keep = self.easy_edge_mask(data, h_index, t_index, r_index)
        data = copy.copy(data)
        data.edge_index = data.edge_index[:, keep]
        data.edge_type = data.edge_type[keep]
        return data

    def negative_sample_to_tail(self, h_index, t_index, r_index, num_direct_rel):
        # p(h | t, r) -> p(t' | h', r'): h' = t, r' = r^-1, t' = h (base_nbfnet.py:79-86)
        is_t_neg = (h_index == h_index[:, :1]).all(dim=-1, keepdim=True)
        new_h_index = torch.where(is_t_neg, h_index, t_index)
        new_t_index = torch.where(is_t_neg, t_index, h_index)
        new_r_index = torch.where(is_t_neg, r_index, r_index + num_direct_rel)
        return new_h_index, new_t_index, new_r_index

    # ---- explanations (base_nbfnet.py:173-263): the beam search over every layer's edge gradients, ultra_amd.explain ----
    @torch.no_grad()
    def beam_search_distance(self, data, edge_grads, h_index, t_index, num_beam=10):
        return explain.beam_search_distance(data, edge_grads, h_index, t_index, num_beam)

    def topk_average_length(self, distances, back_edges, t_index, k=10):
        return explain.topk_average_length(distances, back_edges, t_index, k)

    def _propagate_layers(self, data, layer_input, query, boundary, separate_grad=False, relations=None,
                          edge_weight=None, onehot_rows=None, edge_keep=False, prefilled=None, last_rows=None,
                          edge_grad_route=False, edge_grad_batch=None, delta=None, sample_keys=None):
        """The Bellman-Ford loop shared by every model (models.py:72-80, 150-163, 233-246).
        `delta` (rspmm.GraphDelta, inference only): every layer runs on the graph with the delta's added facts, on the cached
        plan of `data` (layers._propagate_delta); _DeltaRouteUnsupported where a layer or the engine does not serve that.
        `sample_keys` (with `delta` and a 2-D keep mask `edge_weight` over data's edge list): every sample also without its own
        dead edges, base or added (layers._propagate_delta_samples; GraphDelta.sample_keys).
        `relations`: optional per-layer relation features computed up front (EntityNBFNet batches the six
        relation_projection MLPs, which all read the same relation representations).
        `boundary` may be a layers.PointBoundary (then `layer_input` is ignored: layer 0 reads the boundary condition).
        `edge_grad_route` (with separate_grad; visualize only): the layers that can take their edge-weight gradient from the
        plan-based differentiable rspmm do (layers.edge_grad_layer), the others keep the unfused route.
        `edge_grad_batch` (with separate_grad; edge_grads_batch only): a list that receives every layer's (plan, relation, input,
        update) from layers.edge_grad_layer_batch -- constant weights, S samples; _BatchRouteUnsupported where a layer has no
        such route; with `delta` the aggregates run on (data, delta) (layers.edge_grad_layer_batch)."""
        size = (data.num_nodes, data.num_nodes)
        self._last_hidden_on_rows = False
        # edge_weight None = all ones (only materialised when its gradient is asked for); a 0/1 vector = edge dropout
        hiddens, edge_weights = [], []
        first = 0
        if isinstance(boundary, layers.PointBoundary):
            layer = self.layers[0]
            rel0 = None if relations is None else relations[0]
            # (a per-sample keep mask -- 2-D -- has no layer-0 kernel: the layer takes the boundary as a tensor)
            per_sample = edge_weight is not None and edge_weight.dim() == 2
            # (... nor does a graph delta: the closed form walks the base graph's out-edges only)
            if not separate_grad and not per_sample and delta is None and layer.layer0_point_supported(boundary, rel0, edge_weight):
                # layer 0 on its one-hot input: constant fill + the rows reached from the source (ultra_nbf_layer0);
                # the boundary condition never becomes a (batch, N, d) tensor on this path
                residual = self.short_cut and layer.output_dim == layer.input_dim
                # (prefilled: layer 0's constant rows, written ahead of time by EntityNBFNet.prefill_layer0)
                hidden = layer.forward_layer0_point(boundary, query, data.edge_index, data.edge_type, data.num_nodes,
                                                    edge_weight=edge_weight, residual=residual, relation=rel0, out=prefilled)
                hiddens.append(hidden)
                edge_weights.append(edge_weight)
                layer_input = hidden
                first = 1
            else:
                # (the layers still get the closed form: those that can use it -- the sum and max aggregates of the
                # inference path -- do, the others ask it for the tensor, which is built once)
                layer_input = boundary.dense()
                # (a training step of the sum aggregate keeps the closed form: its gradient is bs rows of each layer's
                # output gradient, not a (batch, N, d) tensor per layer for autograd to sum -- layers.point_boundary_trains)
                if separate_grad or (torch.is_grad_enabled() and not all(l.point_boundary_trains() for l in self.layers)):
                    boundary = layer_input
        for i, layer in enumerate(self.layers):
            if i < first:
                continue
            if edge_grad_batch is not None:
                residual = self.short_cut and layer.output_dim == layer_input.shape[-1]
                out = layer.edge_grad_layer_batch(layer_input, query, boundary, data.edge_index, data.edge_type, data.num_nodes,
                                                  residual=residual, relation=None if relations is None else relations[i],
                                                  delta=delta)
                if out is None:
                    raise _BatchRouteUnsupported()
                hiddens.append(out[0])
                edge_weights.append(None)
                edge_grad_batch.append(out[1])
                layer_input = out[0]
                continue
            if separate_grad and edge_grad_route:
                # models.py:150-152: every layer's weights are a clone of the previous layer's, so d score / d weight of layer
                # i sums the direct gradients of layers i .. L-1 -- the reference's edge gradients for visualize
                first_weight = edge_weights[-1] if edge_weights else torch.ones(data.num_edges, device=layer_input.device)
                edge_weight = first_weight.clone().requires_grad_()
            elif separate_grad:
                edge_weight = torch.ones(data.num_edges, device=layer_input.device).requires_grad_()
            # residual connection (models.py:158-160) is fused into the layer's update kernel
            residual = self.short_cut and layer.output_dim == layer_input.shape[-1]
            if separate_grad and edge_grad_route:
                hidden = layer.edge_grad_layer(layer_input, query, boundary, data.edge_index, data.edge_type, data.num_nodes,
                                               edge_weight, residual=residual,
                                               relation=None if relations is None else relations[i])
                if hidden is not None:
                    hiddens.append(hidden)
                    edge_weights.append(edge_weight)
                    layer_input = hidden
                    continue
            if last_rows is not None and i == len(self.layers) - 1 and i > 0 and not separate_grad:
                # the caller reads the last hidden state at `last_rows` only: that layer on those rows' in-edges alone.
                # hiddens[-1] is then (batch, n_list, d), flagged by self._last_hidden_on_rows
                rows_hidden = layer.training_rows_layer(layer_input, query, boundary, data.edge_index, data.edge_type,
                                                        data.num_nodes, last_rows, edge_weight=edge_weight, residual=residual,
                                                        relation=None if relations is None else relations[i])
                if rows_hidden is not None:
                    hiddens.append(rows_hidden)
                    edge_weights.append(edge_weight)
                    self._last_hidden_on_rows = True
                    break
            if delta is not None:
                served = layer.delta_supported() if sample_keys is None else layer.delta_samples_supported()
                if separate_grad or torch.is_grad_enabled() or not served:
                    raise _DeltaRouteUnsupported()
                masked = {} if sample_keys is None else {"edge_weight": edge_weight, "edge_keep": True, "sample_keys": sample_keys}
                hidden = layer._forward_impl(layer_input, query, boundary, data.edge_index, data.edge_type, size,
                                             residual=residual, relation=None if relations is None else relations[i],
                                             delta=delta, **masked)
                if hidden is None:
                    raise _DeltaRouteUnsupported()
                hiddens.append(hidden)
                edge_weights.append(None)
                layer_input = hidden
                continue
            hidden = layer._forward_impl(layer_input, query, boundary, data.edge_index, data.edge_type, size,
                                         edge_weight, residual=residual,
                                         relation=None if relations is None else relations[i],
                                         onehot_rows=onehot_rows if i == 0 else None,
                                         edge_keep=edge_keep and not separate_grad)
            hiddens.append(hidden)
            edge_weights.append(edge_weight)
            layer_input = hidden
        return hiddens, edge_weights


class _DeltaRouteUnsupported(Exception):
    """The engine route of a graph delta (added facts on the cached plan) does not apply -- CPU tensors, a model outside the 64-d
    fused inference path, a layer kind or a plan the delta kernel does not serve: the forward runs on the materialised graph."""


def _materialized_forward(run, data, delta, on_gpu):
    """`run(graph)` on delta.materialize(data) -- today's route: a host plan of the concatenated edge list (the plan cache keeps
    it until the next add).  Not under a hipGraph capture, like the generic path."""
    if on_gpu and torch.cuda.is_current_stream_capturing():
        raise NotOnFusedPath("a graph delta outside the engine route runs on the materialised graph (a host plan): not "
                             "capturable")
    return run(delta.materialize(data))


def _capturing(tensor):
    return tensor.is_cuda and torch.cuda.is_current_stream_capturing()


class _BatchRouteUnsupported(Exception):
    """A layer or the engine does not serve the batched explanation route: edge_grads_batch falls back to one triple a call."""


class RelNBFNet(BaseNBFNet):
    """NBFNet over the relation graph (4 interaction types); returns (batch, num_rel, hidden). models.py:32-102."""

    def __init__(self, input_dim, hidden_dims, num_relation=4, **kwargs):
        super().__init__(input_dim, hidden_dims, num_relation, **kwargs)

        self.layers = nn.ModuleList()
        for i in range(len(self.dims) - 1):
            self.layers.append(
                layers.GeneralizedRelationalConv(
                    self.dims[i], self.dims[i + 1], num_relation,
                    self.dims[0], self.message_func, self.aggregate_func, self.layer_norm,
                    self.activation, dependent=False)
            )

        if self.concat_hidden:
            feature_dim = sum(hidden_dims) + input_dim
            self.mlp = nn.Sequential(
                nn.Linear(feature_dim, feature_dim),
                nn.ReLU(),
                nn.Linear(feature_dim, input_dim)
            )

    def bellmanford(self, data, h_index, separate_grad=False, edge_keep=None):
        batch_size = len(h_index)
        # (one tensor per batch size and device, never dropped: a captured step points at the one its warm-up made, and a
        # forward of another batch size in between -- a ragged last batch run eagerly -- must not free it under the graph)
        cached = self.__dict__.setdefault("_ones_queries", {})
        ones = None if torch.is_grad_enabled() else cached.get((batch_size, h_index.device))
        if ones is None:
            ones = torch.ones(batch_size, self.dims[0], device=h_index.device, dtype=torch.float)
            if not torch.is_grad_enabled():
                cached[(batch_size, h_index.device)] = ones        # constant: not refilled on every forward
        query = ones
        index = h_index.unsqueeze(-1).expand_as(query)
        # boundary: ones at the query relation's node, zeros elsewhere (models.py:59-66) -- in closed form
        boundary = layers.PointBoundary(h_index, query, data.num_nodes)
        adjacency = getattr(data, "dense_adjacency", None)
        if (adjacency is not None and edge_keep is None and not separate_grad and not self.training
                and not torch.is_grad_enabled() and h_index.is_cuda and self.adjacency_blocker() is None):
            # a relation graph kept current in place (tasks.LiveRelationGraph): every layer reads its byte
            # adjacency -- layer 0 in closed form, the others as the reference-order dense layer -- and no plan is asked for, so
            # a captured step sees the cells of a later change at its next replay
            hiddens, hidden = [], None
            for layer in self.layers:
                hidden = layer.forward_adjacency(adjacency, data.num_nodes, boundary, input=hidden,
                                                 residual=self.short_cut and layer.output_dim == layer.input_dim)
                hiddens.append(hidden)
            return self._readout(hiddens, query, data.num_nodes, [None] * len(hiddens))
        if not (layers.POINT_BOUNDARY_FAST_PATH and h_index.is_cuda
                and (not torch.is_grad_enabled() or all(l.point_boundary_trains() for l in self.layers))):
            boundary = boundary.dense()
        # layer 0 reads the one-hot boundary itself: tell the layer which row of each sample is non-zero
        # edge_keep: a 0/1 vector over the relation graph's edges (UltraQuery's training: the relation graph of a dropped graph)
        hiddens, edge_weights = self._propagate_layers(data, boundary, query, boundary, separate_grad=False,
                                                       onehot_rows=h_index, edge_weight=edge_keep,
                                                       edge_keep=edge_keep is not None)
        return self._readout(hiddens, query, data.num_nodes, edge_weights)

    def adjacency_blocker(self):
        """None where every layer can run on a live relation graph's byte adjacency (layers.adjacency_supported); else the
        name of the first layer that cannot, with what it is."""
        for i, layer in enumerate(self.layers):
            if not layer.adjacency_supported():
                return "layers.%d (%s aggregate, %s message, %d -> %d)" % (i, layer.aggregate_func, layer.message_func,
                                                                           layer.input_dim, layer.output_dim)
        return None

    def _readout(self, hiddens, query, num_nodes, edge_weights):
        node_query = query.unsqueeze(1).expand(-1, num_nodes, -1)
        if self.concat_hidden:
            output = torch.cat(hiddens + [node_query], dim=-1)
            output = self.mlp(output)
        else:
            output = hiddens[-1]
        return {
            "node_feature": output,
            "edge_weights": edge_weights,
        }

    def forward(self, rel_graph, query, edge_keep=None):
        return self.bellmanford(rel_graph, h_index=query, edge_keep=edge_keep)["node_feature"]


class EntityNBFNet(BaseNBFNet):
    """NBFNet over the entity graph conditioned on relation representations. models.py:105-209."""

    def __init__(self, input_dim, hidden_dims, num_relation=1, **kwargs):
        # num_relation is a dummy: layers take their relation features from the relation model
        super().__init__(input_dim, hidden_dims, num_relation, **kwargs)

        self.layers = nn.ModuleList()
        for i in range(len(self.dims) - 1):
            self.layers.append(
                layers.GeneralizedRelationalConv(
                    self.dims[i], self.dims[i + 1], num_relation,
                    self.dims[0], self.message_func, self.aggregate_func, self.layer_norm,
                    self.activation, dependent=False, project_relations=True)
            )

        feature_dim = (sum(hidden_dims) if self.concat_hidden else hidden_dims[-1]) + input_dim
        mlp = []
        for i in range(self.num_mlp_layers - 1):
            mlp.append(nn.Linear(feature_dim, feature_dim))
            mlp.append(nn.ReLU())
        mlp.append(nn.Linear(feature_dim, 1))
        self.mlp = nn.Sequential(*mlp)

    _side_streams = {}

    def prefill_layer0(self, data, batch_size):
        """Layer 0 of the entity model leaves all but a few thousand rows at one constant value that depends on its parameters
        alone (layers.forward_layer0_point): the 30 MB fill is launched here, on a side stream, BEFORE the relation model
        runs -- whose launches are latency bound and leave the memory system idle -- instead of behind it.  Returns
        (tensor, stream) for forward(prefill=...), or None where layer 0 will not take that path."""
        layer = self.layers[0]
        dev = data.edge_index.device
        if not (layers.POINT_BOUNDARY_FAST_PATH and dev.type == "cuda" and not torch.is_grad_enabled() and not self.training
                and layer.aggregate_func in ("sum", "max") and layer.message_func == "distmult" and layer.input_dim == 64
                and layer.output_dim == 64 and layer.linear.in_features == 128
                and (layer.activation is None or layer.activation is torch.nn.functional.relu)
                and layer.linear.weight.dtype == torch.float32):
            return None
        key = str(dev)
        side = EntityNBFNet._side_streams.get(key)
        if side is None:
            with torch.cuda.device(dev):
                side = EntityNBFNet._side_streams[key] = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            out = layer.layer0_fill(data.edge_index, data.edge_type, data.num_nodes, int(data.num_relations), batch_size)
        return out, side

    def _bellmanford_hidden(self, data, h_index, r_index, separate_grad=False, edge_weight=None, edge_keep=False, prefilled=None,
                            last_rows=None, edge_grad_route=False, edge_grad_batch=None, delta=None, sample_keys=None):
        batch_size = len(r_index)
        # query = representation of each sample's query relation, scattered to its head node
        fused = (dense.boundary_supported(h_index, self.query) and self.query.dim() == 3
                 and self.query.shape[0] == batch_size and self.query.shape[-1] == self.dims[0])
        if fused and layers.POINT_BOUNDARY_FAST_PATH and not torch.is_grad_enabled():
            # gather the query rows; the boundary stays in closed form
            _, query, _ = dense.query_boundary(h_index, self.query, r_index, data.num_nodes, materialize=False)
            boundary = layers.PointBoundary(h_index, query, data.num_nodes)
        elif (layers.POINT_BOUNDARY_FAST_PATH and h_index.is_cuda and torch.is_grad_enabled() and self.query.dim() == 3
              and all(l.point_boundary_trains() for l in self.layers)):
            # training step: the query rows through autograd's gather, the boundary in closed form (its dense form, which
            # layer 0's update reads, is built from it once: PointBoundary.dense)
            # (gather, not advanced indexing: its backward is one scatter_add instead of index_put_'s sort + ~ 10 launches)
            query = dense.pick_rows(self.query, r_index)
            boundary = layers.PointBoundary(h_index, query, data.num_nodes)
        elif fused:
            # gather + scatter, one kernel
            boundary, query, _ = dense.query_boundary(h_index, self.query, r_index, data.num_nodes)
        else:
            query = self.query[torch.arange(batch_size, device=r_index.device), r_index]
            index = h_index.unsqueeze(-1).expand_as(query)
            boundary = torch.zeros(batch_size, data.num_nodes, self.dims[0], device=h_index.device, dtype=query.dtype)
            boundary.scatter_add_(1, index.unsqueeze(1), query.unsqueeze(1))
        hiddens, edge_weights = self._propagate_layers(data, boundary, query, boundary, separate_grad,
                                                       relations=self._project_relations_batched(),
                                                       edge_weight=edge_weight, onehot_rows=h_index, edge_keep=edge_keep,
                                                       prefilled=prefilled, last_rows=last_rows, edge_grad_route=edge_grad_route,
                                                       edge_grad_batch=edge_grad_batch, delta=delta, sample_keys=sample_keys)
        return hiddens, edge_weights, query

    def _project_relations_batched(self):
        """All layers' relation_projection MLPs (layers.py:80) read the same input: one MFMA kernel for the ULTRA
        shape (two batched GEMMs otherwise) instead of 12 small GEMMs.  Inference only; training keeps the per-layer
        modules."""
        rel = self.query
        if rel is None or not rel.is_cuda or not all(
                getattr(l, "project_relations", False) and not l.dependent for l in self.layers):
            return None
        if torch.is_grad_enabled():
            if (RELATION_PROJECTION_NODE and rel.dtype == torch.float32 and rel.shape[-1] == 64 and len(self.layers) <= 8 and all(
                    tuple(l.relation_projection[i].weight.shape) == (64, 64) and l.relation_projection[i].bias is not None
                    for l in self.layers for i in (0, 2))):
                # Training: every layer's MLP as ONE autograd node over the layers' own parameters -- one launch forward, three
                # backward (dense.RelationProjectionFunction)
                return dense.relation_projection_train(
                    rel, [(l.relation_projection[0].weight, l.relation_projection[0].bias, l.relation_projection[2].weight,
                           l.relation_projection[2].bias) for l in self.layers])
            # (other shapes) the same twelve products as two batched ones that autograd differentiates -- torch.stack hands every
            # layer's parameters their own gradient slice.  Per layer the step otherwise spends two 39-us GEMM launches forward
            # (3,792 x 64 x 64: launch-bound) and four backward.  Same formula as nn.Sequential(Linear, ReLU, Linear).
            n = len(self.layers)
            w0 = torch.stack([l.relation_projection[0].weight for l in self.layers]).transpose(1, 2)
            b0 = torch.stack([l.relation_projection[0].bias for l in self.layers]).unsqueeze(1)
            w2 = torch.stack([l.relation_projection[2].weight for l in self.layers]).transpose(1, 2)
            b2 = torch.stack([l.relation_projection[2].bias for l in self.layers]).unsqueeze(1)
            x = rel.reshape(1, -1, rel.shape[-1]).expand(n, -1, -1)
            h = torch.baddbmm(b0, x, w0).relu()
            out = torch.baddbmm(b2, h, w2)
            return list(out.view(n, *rel.shape[:-1], out.shape[-1]).unbind(0))
        params = [p for l in self.layers for p in l.relation_projection.parameters()]
        key = tuple((p.data_ptr(), p._version) for p in params)
        if getattr(self, "_proj_key", None) != key:
            self._proj_w0 = torch.stack([l.relation_projection[0].weight for l in self.layers]).transpose(1, 2).contiguous()
            self._proj_b0 = torch.stack([l.relation_projection[0].bias for l in self.layers]).unsqueeze(1)
            self._proj_w2 = torch.stack([l.relation_projection[2].weight for l in self.layers]).transpose(1, 2).contiguous()
            self._proj_b2 = torch.stack([l.relation_projection[2].bias for l in self.layers]).unsqueeze(1)
            # [out][in] stacks for the fused kernel
            self._proj_k = [torch.stack([l.relation_projection[i].weight for l in self.layers]).contiguous() for i in (0, 2)] \
                + [torch.stack([l.relation_projection[i].bias for l in self.layers]).contiguous() for i in (0, 2)]
            self._proj_key = key
        n = len(self.layers)
        if rel.dtype == torch.float32 and rel.shape[-1] == 64 and all(
                tuple(l.relation_projection[i].weight.shape) == (64, 64) for l in self.layers for i in (0, 2)):
            w0, w2, b0, b2 = self._proj_k
            return list(dense.relation_projection(rel, w0, b0, w2, b2).unbind(0))
        x = rel.reshape(1, -1, rel.shape[-1]).expand(n, -1, -1)
        h = torch.baddbmm(self._proj_b0, x, self._proj_w0).relu_()
        out = torch.baddbmm(self._proj_b2, h, self._proj_w2)
        return list(out.view(n, *rel.shape[:-1], out.shape[-1]).unbind(0))

    def bellmanford(self, data, h_index, r_index, separate_grad=False):
        hiddens, edge_weights, query = self._bellmanford_hidden(data, h_index, r_index, separate_grad)
        node_query = query.unsqueeze(1).expand(-1, data.num_nodes, -1)
        if self.concat_hidden:
            output = torch.cat(hiddens + [node_query], dim=-1)
        else:
            output = torch.cat([hiddens[-1], node_query], dim=-1)
        return {
            "node_feature": output,
            "edge_weights": edge_weights,
        }

    def edge_grads(self, data, batch):
        """d score(h, t, r) / d edge_weight for every layer (base_nbfnet.py:156-167): the relation representations must be
        installed (self.query, as forward() does).  sum / DistMult layers take their gradient from the plan-based rspmm,
        the others from the unfused route.  Returns (edge_grads, score)."""
        assert batch.shape == (1, 3)
        h_index, t_index, r_index = batch.unbind(-1)
        last_hidden_on_rows = getattr(self, "_last_hidden_on_rows", False)
        with torch.enable_grad():
            hiddens, edge_weights, query = self._bellmanford_hidden(data, h_index, r_index, separate_grad=True,
                                                                    edge_grad_route=True)
            picked = [h[:, t_index] for h in (hiddens if self.concat_hidden else hiddens[-1:])]     # (1, 1, d) each
            feature = torch.cat(picked + [query.unsqueeze(1)], dim=-1).squeeze(0)
            score = self.mlp(feature).squeeze(-1)
            edge_grads = autograd.grad(score, edge_weights)
        self._last_hidden_on_rows = last_hidden_on_rows
        return list(edge_grads), score.detach()

    def visualize(self, data, batch):
        """base_nbfnet.py:156-171: the top `path_topk` paths from h to t of one triple (1, 3) -- lists of (h, t, r) -- and
        their average edge weights, from a beam of `num_beam` over every layer's edge gradients."""
        assert batch.shape == (1, 3)
        h_index, t_index, r_index = batch.unbind(-1)
        edge_grads, _ = self.edge_grads(data, batch)
        distances, back_edges = self.beam_search_distance(data, edge_grads, h_index, t_index, self.num_beam)
        return self.topk_average_length(distances, back_edges, t_index, self.path_topk)

    # ---- explanations of S triples at once (they may differ in h, r and t) ----
    def _installed_slice(self, lo, hi):
        """Install rows lo:hi of the installed (S, R, d) relation representations as the model's (what a forward() on those
        triples alone would have installed); returns what to hand to _restore_installed."""
        saved = (getattr(self, "query", None), [getattr(l, "relation", None) for l in self.layers])
        full = saved[0]
        self.query = full[lo:hi]
        for layer, rel in zip(self.layers, saved[1]):
            if torch.is_tensor(rel) and rel.dim() == 3 and rel.shape[0] == full.shape[0]:
                layer.relation = rel[lo:hi]
        return saved

    def _restore_installed(self, saved):
        self.query = saved[0]
        for layer, rel in zip(self.layers, saved[1]):
            layer.relation = rel

    def _edge_grads_per_triple(self, data, batch):
        """edge_grads_batch through edge_grads, one triple at a time (the route of every layer kind)."""
        grads, scores = [], []
        for s in range(batch.shape[0]):
            saved = self._installed_slice(s, s + 1)
            try:
                g, score = self.edge_grads(data, batch[s:s + 1])
            finally:
                self._restore_installed(saved)
            grads.append(g)
            scores.append(score)
        return [torch.stack([g[i] for g in grads]) for i in range(len(self.layers))], torch.cat(scores)

    def edge_grads_batch(self, data, batch, delta=None):
        """edge_grads for S triples, batch (S, 3), with the (S, R, d) relation representations of their query relations
        installed (self.query, row s for triple s): ONE forward and one backward for all of them.  The samples are independent,
        so row s of the gradient of scores.sum() with respect to a layer's aggregate is triple s's; each layer's direct
        edge-weight gradient then comes per sample from ultra_rspmm_edge_grad_samples, and the reference's clone chain
        (models.py:150-152: layer i's weights are a clone of layer i - 1's) makes layer i's gradient the sum of the direct ones
        of layers i .. L-1.  Returns ([(S, num_edge)] * L, scores (S)).  Models whose layers are not sum / DistMult / fp32 on
        the GPU are explained triple by triple through edge_grads: the same values either way.
        `delta` (rspmm.GraphDelta of `data`): the gradients on (data, delta), defined as those of this call on
        delta.materialize(data) -- equal to them up to fp32 re-association, not bit for bit: the route was never order-pinned
        (the re-associating plan and autograd), and an edited row adds its new edges' total with one more add.  The plan and the
        edge list stay the base graph's.  Returns (base_grads [(S, num_edge)] * L over data's edge list -- the columns of
        tombstoned edges are not part of the result --, added_grads [(S, 2 capacity)] * L over delta.edges() with the columns
        from 2 num_facts on zero, scores (S)); the clone chain applies to both halves.  No per-triple fallback: RuntimeError
        where a layer or the engine does not serve the batched route (predict.explain_live_supported)."""
        if batch.dim() != 2 or batch.shape[1] != 3:
            raise ValueError("Expected a batch of triples of shape (S, 3), got %s" % (tuple(batch.shape),))
        if delta is not None:
            return self._edge_grads_batch_delta(data, batch, delta)
        query = getattr(self, "query", None)
        if not torch.is_tensor(query) or query.dim() != 3 or query.shape[0] != batch.shape[0]:
            raise ValueError("edge_grads_batch: install the (S, num_relation, d) relation representations of the batch's query "
                             "relations first (self.query), S = %d" % batch.shape[0])
        num_sample = batch.shape[0]
        dev = data.edge_index.device
        if num_sample == 0:
            return ([torch.zeros((0, data.num_edges), device=dev) for _ in self.layers], torch.zeros(0, device=dev))
        if not (batch.is_cuda and query.is_cuda and query.dtype == torch.float32):
            return self._edge_grads_per_triple(data, batch)
        h_index, t_index, r_index = batch.unbind(-1)
        last_hidden_on_rows = getattr(self, "_last_hidden_on_rows", False)
        try:
            with torch.enable_grad():
                records = []
                hiddens, _, query = self._bellmanford_hidden(data, h_index, r_index, separate_grad=True, edge_grad_batch=records)
                sample = torch.arange(num_sample, device=batch.device)
                picked = [h[sample, t_index] for h in (hiddens if self.concat_hidden else hiddens[-1:])]     # (S, d) each
                scores = self.mlp(torch.cat(picked + [query], dim=-1)).squeeze(-1)
                update_grads = autograd.grad(scores.sum(), [rec[3] for rec in records])
            edge_grads = [None] * len(records)
            with torch.no_grad():
                for i in range(len(records) - 1, -1, -1):
                    plan, relation, layer_input, _ = records[i]
                    direct = plan.edge_grad_samples(relation.detach(), layer_input.detach(), update_grads[i].contiguous())
                    if direct is None:
                        raise _BatchRouteUnsupported()
                    edge_grads[i] = direct if i == len(records) - 1 else direct + edge_grads[i + 1]
        except _BatchRouteUnsupported:
            return self._edge_grads_per_triple(data, batch)
        finally:
            self._last_hidden_on_rows = last_hidden_on_rows
        return edge_grads, scores.detach()

    def _edge_grads_batch_delta(self, data, batch, delta):
        """edge_grads_batch on (data, delta): the batched route alone."""
        query = getattr(self, "query", None)
        num_sample = batch.shape[0]
        if not torch.is_tensor(query) or query.dim() != 3 or query.shape[0] != num_sample:
            raise ValueError("edge_grads_batch: install the (S, num_relation, d) relation representations of the batch's query "
                             "relations first (self.query), S = %d" % num_sample)
        dev = data.edge_index.device
        if not (batch.is_cuda and query.is_cuda and query.dtype == torch.float32) or num_sample == 0:
            raise RuntimeError("edge_grads_batch(delta=) serves a non-empty batch of fp32 representations on the GPU")
        unserved = RuntimeError("edge_grads_batch(delta=): a layer or the engine does not serve the batched explanation route "
                                "on a graph delta (sum / DistMult, fp32)")
        h_index, t_index, r_index = batch.unbind(-1)
        last_hidden_on_rows = getattr(self, "_last_hidden_on_rows", False)
        try:
            with torch.enable_grad():
                records = []
                hiddens, _, query = self._bellmanford_hidden(data, h_index, r_index, separate_grad=True, edge_grad_batch=records,
                                                             delta=delta)
                sample = torch.arange(num_sample, device=batch.device)
                picked = [h[sample, t_index] for h in (hiddens if self.concat_hidden else hiddens[-1:])]     # (S, d) each
                scores = self.mlp(torch.cat(picked + [query], dim=-1)).squeeze(-1)
                update_grads = autograd.grad(scores.sum(), [rec[3] for rec in records])
            base_grads, added_grads = [None] * len(records), [None] * len(records)
            with torch.no_grad():
                for i in range(len(records) - 1, -1, -1):
                    plan, relation, layer_input, _ = records[i]
                    grad = update_grads[i].contiguous()
                    direct = plan.edge_grad_samples(relation.detach(), layer_input.detach(), grad)
                    if direct is None:
                        raise unserved
                    if delta.edited:
                        added = delta.delta_edge_grad_samples(relation.detach(), layer_input.detach(), grad)
                    else:
                        added = torch.zeros((num_sample, 2 * delta.capacity), device=dev)
                    last = i == len(records) - 1
                    base_grads[i] = direct if last else direct + base_grads[i + 1]
                    added_grads[i] = added if last else added + added_grads[i + 1]
        except _BatchRouteUnsupported:
            raise unserved
        finally:
            self._last_hidden_on_rows = last_hidden_on_rows
        return base_grads, added_grads, scores.detach()

    def visualize_batch(self, data, batch, chunk=16, delta=None):
        """visualize for S triples, batch (S, 3), with their (S, R, d) relation representations installed: a list of (paths,
        weights), entry s what visualize returns for triple s.  `chunk` triples share one forward, one backward and the
        launches of one beam search (explain.beam_search_distance_batch); it bounds the memory of the 2 L (chunk, ...) tables.
        `delta` (an edited rspmm.GraphDelta of `data`): the explanations on (data, delta), defined as those of this call on
        delta.materialize(data) (edge_grads_batch(delta=), beam_search_distance_batch(delta=)); an unedited or absent delta is
        the call without it."""
        if batch.dim() != 2 or batch.shape[1] != 3:
            raise ValueError("Expected a batch of triples of shape (S, 3), got %s" % (tuple(batch.shape),))
        if not isinstance(chunk, int) or chunk < 1:
            raise ValueError("chunk must be a positive int, got %r" % (chunk,))
        host = batch.cpu()      # (one read for the whole batch: the heads and tails are checked against the graph on the host)
        results = []
        live = delta is not None and delta.edited
        live_args = (lambda added: {"delta": delta, "added_grads": added}) if live else (lambda added: {})
        for lo in range(0, batch.shape[0], chunk):
            hi = min(lo + chunk, batch.shape[0])
            saved = self._installed_slice(lo, hi)
            added_grads = None
            try:
                if live:
                    edge_grads, added_grads, _ = self.edge_grads_batch(data, batch[lo:hi], delta=delta)
                else:
                    edge_grads, _ = self.edge_grads_batch(data, batch[lo:hi])
            finally:
                self._restore_installed(saved)
            distances, back_edges = explain.beam_search_distance_batch(data, edge_grads, host[lo:hi, 0], host[lo:hi, 1],
                                                                       self.num_beam, **live_args(added_grads))
            results.extend(explain.topk_average_length_batch(distances, back_edges, host[lo:hi, 1], self.path_topk))
        return results

    def prologue_supported(self, batch):
        """The inference fast path of forward(): one prologue kernel instead of the index arithmetic of models.py:190-197."""
        return (PROLOGUE_FAST_PATH and not self.training and not torch.is_grad_enabled() and batch.is_cuda
                and batch.dtype == torch.long and batch.dim() == 3 and not self.concat_hidden)

    def _check_edge_keep(self, data, batch, edge_keep):
        """edge_keep of forward(): one 0/1 keep row over data's edge list per sample; inference only."""
        if self.training or torch.is_grad_enabled():
            raise ValueError("edge_keep (per-sample keep masks) serves eval mode under torch.no_grad() only: a training step "
                             "builds its own batch-wide vector")
        if not torch.is_tensor(edge_keep) or edge_keep.dim() != 2 \
                or tuple(edge_keep.shape) != (batch.shape[0], data.edge_index.shape[1]):
            raise ValueError("edge_keep must be a (batch, num_edge) = (%d, %d) tensor" % (batch.shape[0], data.edge_index.shape[1]))

    def forward(self, data, relation_representations, batch, prefill=None, prologue=None, edge_keep=None, delta=None,
                leave_out=None, leave_out_buffers=None, leave_out_fallback=None):
        """edge_keep (batch, num_edge), 0/1, original edge order: sample s runs on the graph without the edges whose
        edge_keep[s] is 0 -- row s of the result is this forward on data filtered by edge_keep[s] with batch[s:s+1] (eval mode
        under no_grad only).  The relation graph is the caller's: not rebuilt.
        delta (rspmm.GraphDelta; eval mode under no_grad, not with edge_keep): the forward on the graph with the delta's added
        facts -- it equals this forward on delta.materialize(data).  On the fused inference path a branch shaped like the masked
        one runs on data's cached plans (prologue, delta layers, readout: every step an engine launch, so a capture records
        it); elsewhere the materialised graph is used (relation_representations are the caller's in both cases).
        leave_out (batch, 3) int64 = the stated facts (h, t, r), r direct (eval mode under no_grad, not with edge_keep): sample s
        is scored without fact s and its inverse -- with `remove_one_hop` without any edge between the two nodes.  Without a
        delta (or with an unedited one) that is edge_keep=leave_one_out_keep(data, leave_out).  With an edited delta sample s
        runs on delta.materialize(data) without those edges, whether they are base edges or the delta's own
        (_forward_leave_out); the delta is not folded into the graph.  leave_out_buffers = (keep (batch, num_edge) fp32,
        (row, col, type) int32 (batch, 2) each): a captured step's own buffers for the keep rows and the keys.
        leave_out_fallback: the caller's definition loop for the case the engine route does not apply (Ultra.forward's)."""
        if delta is not None and not delta.edited:
            delta = None
        if leave_out is not None:
            if edge_keep is not None:
                raise ValueError("leave_out builds its own keep rows: not together with edge_keep")
            if self.training or torch.is_grad_enabled():
                raise ValueError("leave_out (leave-one-out verification) serves eval mode under torch.no_grad() only")
            if not torch.is_tensor(leave_out) or leave_out.dim() != 2 or tuple(leave_out.shape) != (batch.shape[0], 3):
                raise ValueError("leave_out must be a (batch, 3) = (%d, 3) tensor of stated facts (h, t, r)" % batch.shape[0])
            keep_out, keys_out = leave_out_buffers if leave_out_buffers is not None else (None, None)
            if delta is None:       # (no edits: exactly the keep rows' route)
                edge_keep = self.leave_one_out_keep(data, leave_out, out=keep_out, validate=not _capturing(leave_out))
            else:
                return self._forward_leave_out(data, relation_representations, batch, prologue, delta, leave_out, keep_out,
                                               keys_out, leave_out_fallback)
        if delta is not None:
            if edge_keep is not None or self.training or torch.is_grad_enabled():
                raise ValueError("a graph delta (added facts) serves eval mode under torch.no_grad() only, without edge_keep")
            try:
                if not self.prologue_supported(batch):
                    raise _DeltaRouteUnsupported()
                return self._forward_delta(data, relation_representations, batch, prologue, delta)
            except _DeltaRouteUnsupported:
                if getattr(delta, "per_query_owned", False):
                    # (facts assumed per sample, rspmm.AssumedFacts: no shared materialised graph to fall back to)
                    raise NotOnFusedPath("an overlay of assumed facts outside the engine route runs query by query "
                                         "(predict.assume_reference's loop)")
                return _materialized_forward(lambda graph: self.forward(graph, relation_representations, batch), data, delta,
                                             batch.is_cuda)
        if edge_keep is not None:
            self._check_edge_keep(data, batch, edge_keep)
        h_index, t_index, r_index = batch.unbind(-1)
        prefilled = None
        if prefill is not None:       # (prefill_layer0: the side stream joins here, whatever path the forward takes)
            prefilled, side = prefill
            torch.cuda.current_stream(prefilled.device).wait_stream(side)
            if tuple(prefilled.shape) != (batch.shape[0], data.num_nodes, 64):
                prefilled = None

        self.query = relation_representations
        for layer in self.layers:
            layer.relation = relation_representations

        edge_weight = None
        if self.training:
            rotate_keep = (self.message_func == "rotate" and self.aggregate_func in ("sum", "min", "max", "mean")
                           and all(layer.rotate_fused(relation_representations, relation_representations) for layer in self.layers))
            if rotate_keep or (self.aggregate_func in ("sum", "min", "max", "mean", "pna")
                               and self.message_func in ("distmult", "transe")):
                # Edge dropout without touching the graph: a 0/1 keep vector over the static edge list (one kernel), read
                # by the rspmm kernels as "edge absent" -- so the cached plan of the static graph serves every batch
                # (the reference filters the edge list, base_nbfnet.py:54-77, and re-sorts it inside every rspmm call);
                # mean / pna take their degree from the same vector (layers.message_and_aggregate).
                edge_weight = self.easy_edge_keep(data, h_index, t_index, r_index, relation_representations.dtype)
            else:
                # rotate off the engine (pna, CPU tensors, layers.FUSED_ROTATE = False) runs the unfused scatter path: the
                # reference's filtered copy of the graph
                data = self.remove_easy_edges(data, h_index, t_index, r_index)
        elif edge_keep is not None:
            # per-sample masks: every layer walks the cached plan of the full graph with its sample's row (layers._propagate_samples)
            edge_weight = edge_keep if edge_keep.dtype == relation_representations.dtype \
                else edge_keep.to(relation_representations.dtype)
            prefilled = None

        shape = h_index.shape
        if (edge_weight is None or edge_keep is not None) and self.prologue_supported(batch):
            # inference fast path: one prologue kernel (row uniformity, head->tail conversion, validity flag) and
            # a readout that picks its candidate column straight from the raw batch
            batch_c, h0, r0, side, valid = prologue if prologue is not None else dense.batch_prologue(batch, data.num_relations // 2)
            # (with edge_keep: the masked branch -- prologue, masked layers, readout, every step an engine launch, so a capture
            # records it like the unmasked one)
            hiddens, _, query = self._bellmanford_hidden(data, h0, r0, prefilled=prefilled, edge_weight=edge_weight,
                                                         edge_keep=edge_weight is not None)
            if dense.readout_supported(self, hiddens[-1]):
                score = dense.readout_batch(self, hiddens[-1], query, batch_c, side).view(shape)
                self._check_valid(valid)
                return score
            # (shape not covered by the fused readout: fall through to the generic path below)
        if batch.is_cuda and torch.cuda.is_current_stream_capturing() and not generic_path_capturable():
            # the generic path goes through torch reductions / memsets whose captured nodes were seen to go stale
            # when replays interleave with eager work (ROCm 7.2); of the inference paths only the fused one is
            # graph-captured.  train.GraphedTrainStep captures the training step (this path, under autograd) inside
            # capture_generic_path().
            raise NotOnFusedPath("hipGraph capture is supported for the fused inference path only "
                                 "(64-d hidden, no concat_hidden, eval mode, no_grad)")
        # One reduction tells, per row, whether heads / tails / relations are constant along the candidates:
        # it drives the head->tail conversion (base_nbfnet.py:82) AND replaces the two asserts of models.py:196-197
        # (two host syncs in the middle of the forward there; here the flag is checked after the whole forward has
        # been enqueued): a converted row has a uniform head iff its heads or its tails were uniform.
        num_direct_rel = data.num_relations // 2
        if PROLOGUE_FAST_PATH and batch.is_cuda and batch.dtype == torch.long and batch.dim() == 3 and batch.shape[1] <= 65536:
            # the same in ONE launch (dense.batch_prologue: uniformity per row, conversion, the converted rows' candidates)
            pro = dense.batch_prologue(batch, num_direct_rel, candidates=True)
            h0, r0, valid, t_index = pro[1], pro[2], pro[4], pro.cand
        else:
            same = (batch == batch[:, :1]).all(dim=1)                      # (bs, 3): h, t, r uniform?
            is_t_neg = same[:, :1]
            h_index, t_index, r_index = (torch.where(is_t_neg, h_index, t_index), torch.where(is_t_neg, t_index, h_index),
                                         torch.where(is_t_neg, r_index, r_index + num_direct_rel))
            h0, r0 = h_index[:, 0], r_index[:, 0]
            valid = ((same[:, 0] | same[:, 1]) & same[:, 2]).all()

        # (under autograd only the candidates' rows of the last hidden state are read below: the last layer is evaluated on
        # those rows' in-edges alone where the layer supports it -- layers.training_rows_layer)
        rows_wanted = t_index if (torch.is_grad_enabled() and not self.concat_hidden and t_index.is_cuda) else None
        hiddens, _, query = self._bellmanford_hidden(data, h0, r0, edge_weight=edge_weight,
                                                     edge_keep=edge_weight is not None, last_rows=rows_wanted)
        if self._last_hidden_on_rows:
            if torch.is_grad_enabled() and dense.readout_train_supported(self, hiddens[-1], query):
                score = dense.readout_train(self, hiddens[-1], query)          # one autograd node: 1 + 2 launches
            else:
                feature = torch.cat([hiddens[-1], query.unsqueeze(1).expand(-1, t_index.shape[1], -1)], dim=-1)
                score = self.mlp(feature).squeeze(-1)
            self._check_valid(valid)
            return score.view(shape)
        if dense.readout_supported(self, hiddens[-1]):
            # gather + cat[hidden, query] + MLP in one MFMA kernel (nothing of size (bs, N, 128) is materialised)
            score = dense.readout(self, hiddens[-1], query, t_index).view(shape)
            self._check_valid(valid)
            return score
        # models.py:202-207 builds cat[hidden, query] for EVERY node and then gathers the candidates' rows; gathering first
        # gives the same (batch, 1 + num_negative, feature_dim) rows without the (batch, N, 128) tensor -- and, under
        # autograd, without its backward: a (batch, N, 128) scatter target and the reduction over N of the expanded query
        # (90 us of a 7 ms fine-tuning step at FB15k237's size, 0.9 ms of 23 at YAGO3-10's)
        picked = [h.gather(1, t_index.unsqueeze(-1).expand(-1, -1, h.shape[-1]))
                  for h in (hiddens if self.concat_hidden else hiddens[-1:])]
        feature = torch.cat(picked + [query.unsqueeze(1).expand(-1, t_index.shape[1], -1)], dim=-1)
        score = self.mlp(feature).squeeze(-1)
        self._check_valid(valid)
        return score.view(shape)

    def _forward_delta(self, data, relation_representations, batch, prologue, delta):
        """The delta branch of forward(): dense.batch_prologue, the layers with the delta's rows fixed after every aggregate,
        dense.readout_batch."""
        self.query = relation_representations
        for layer in self.layers:
            layer.relation = relation_representations
        batch_c, h0, r0, side, valid = prologue if prologue is not None else dense.batch_prologue(batch, data.num_relations // 2)
        hiddens, _, query = self._bellmanford_hidden(data, h0, r0, delta=delta)
        if not dense.readout_supported(self, hiddens[-1]):
            raise _DeltaRouteUnsupported()
        score = dense.readout_batch(self, hiddens[-1], query, batch_c, side).view(batch.shape[:-1])
        self._check_valid(valid)
        return score

    def _forward_leave_out(self, data, relation_representations, batch, prologue, delta, leave_out, keep_out, keys_out,
                           fallback):
        """leave_out= with an edited delta.  The engine route: dense.batch_prologue, the keep rows over data's (the base) edge
        list and the same edges as per-sample keys, every layer as layers._propagate_delta_samples, dense.readout_batch -- every
        step an engine launch or a small torch copy, so a capture records it.  Where that does not apply (CPU tensors, a model
        off the fused path, a layer kind or a plan the kernel does not serve) the DEFINITION runs: sample by sample this forward
        on remove_easy_edges(delta.materialize(data), fact s)."""
        try:
            if not self.prologue_supported(batch) or not all(l.delta_samples_supported() for l in self.layers):
                raise _DeltaRouteUnsupported()
            self.query = relation_representations
            for layer in self.layers:
                layer.relation = relation_representations
            keep = self.leave_one_out_keep(data, leave_out, out=keep_out, validate=not _capturing(leave_out))
            keys = delta.sample_keys(leave_out, any_type=self.remove_one_hop, out=keys_out)
            if keep.dtype != relation_representations.dtype:
                keep = keep.to(relation_representations.dtype)
            batch_c, h0, r0, side, valid = prologue if prologue is not None else dense.batch_prologue(batch, data.num_relations // 2)
            hiddens, _, query = self._bellmanford_hidden(data, h0, r0, delta=delta, edge_weight=keep, edge_keep=True,
                                                         sample_keys=keys)
            if not dense.readout_supported(self, hiddens[-1]):
                raise _DeltaRouteUnsupported()
            score = dense.readout_batch(self, hiddens[-1], query, batch_c, side).view(batch.shape[:-1])
            self._check_valid(valid)
            return score
        except _DeltaRouteUnsupported:
            pass
        if _capturing(batch):
            raise NotOnFusedPath("leave_out with a graph delta outside the engine route runs sample by sample on the materialised "
                                 "graph (host plans): not capturable")
        if fallback is not None:
            return fallback()
        full = delta.materialize(data)
        h_index, t_index, r_index = leave_out.unbind(-1)
        rows = []
        for s in range(batch.shape[0]):
            without = self.remove_easy_edges(full, h_index[s:s + 1], t_index[s:s + 1], r_index[s:s + 1])
            rows.append(self.forward(without, relation_representations[s:s + 1], batch[s:s + 1]))
        return torch.cat(rows)

    def _check_valid(self, valid):
        if valid.is_cuda and torch.cuda.is_current_stream_capturing():
            self._pending_valid = valid      # checked by the graph wrapper after replay (graph.py)
            return
        assert bool(valid.all()), "every row of `batch` must share its head (or tail) and its relation (models.py:196-197)"


class QueryNBFNet(EntityNBFNet):
    """Entity-level reasoner of UltraQuery: initial node features and queries come from outside,
    scores every node (models.py:212-275)."""

    def bellmanford(self, data, node_features, query, separate_grad=False):
        hiddens, edge_weights = self._propagate_layers(data, node_features, query, node_features, separate_grad)
        node_query = query.unsqueeze(1).expand(-1, data.num_nodes, -1)
        if self.concat_hidden:
            output = torch.cat(hiddens + [node_query], dim=-1)
        else:
            output = torch.cat([hiddens[-1], node_query], dim=-1)
        return {
            "node_feature": output,
            "edge_weights": edge_weights,
        }

    def forward(self, data, node_features, relation_representations, query, edge_keep=None, delta=None):
        """delta (rspmm.GraphDelta; under no_grad, not with edge_keep): the scores on the graph with the delta's added facts --
        the layers on data's cached plan where the engine serves them, else on delta.materialize(data)."""
        for layer in self.layers:
            layer.relation = relation_representations
        self.query = relation_representations      # input of the batched relation projections
        if delta is not None and delta.edited:
            if edge_keep is not None or torch.is_grad_enabled():
                raise ValueError("a graph delta (added facts) serves inference under torch.no_grad() only, without edge_keep")
            try:
                hiddens, _ = self._propagate_layers(data, node_features, query, node_features, delta=delta,
                                                    relations=self._project_relations_batched())
            except _DeltaRouteUnsupported:
                if getattr(delta, "per_query_owned", False):
                    # (facts assumed per sample, rspmm.AssumedFacts: no shared materialised graph to fall back to)
                    raise NotOnFusedPath("an overlay of assumed facts outside the engine route runs query by query "
                                         "(query_predict.assume_reference's loop)")
                return _materialized_forward(lambda graph: self.forward(graph, node_features, relation_representations, query),
                                             data, delta, query.is_cuda)
            if dense.readout_supported(self, hiddens[-1]):
                every = torch.arange(data.num_nodes, device=query.device).unsqueeze(0).expand(len(query), -1)
                return dense.readout(self, hiddens[-1], query, every)
            node_query = query.unsqueeze(1).expand(-1, data.num_nodes, -1)
            feature = torch.cat((hiddens if self.concat_hidden else hiddens[-1:]) + [node_query], dim=-1)
            return self.mlp(feature).squeeze(-1)
        if edge_keep is not None:
            # UltraQuery's training projection: traversal dropout as a 0/1 keep vector over the static edge list (read through
            # the full graph's cached plan), and the readout of every node as one autograd node where it applies
            hiddens, _ = self._propagate_layers(data, node_features, query, node_features, edge_weight=edge_keep,
                                                edge_keep=True, relations=self._project_relations_batched())
            if torch.is_grad_enabled() and dense.readout_train_supported(self, hiddens[-1], query):
                return dense.readout_train(self, hiddens[-1], query)
            node_query = query.unsqueeze(1).expand(-1, data.num_nodes, -1)
            feature = torch.cat((hiddens if self.concat_hidden else hiddens[-1:]) + [node_query], dim=-1)
            return self.mlp(feature).squeeze(-1)
        hiddens, _ = self._propagate_layers(data, node_features, query, node_features,
                                            relations=self._project_relations_batched())
        if dense.readout_supported(self, hiddens[-1]):
            every = torch.arange(data.num_nodes, device=query.device).unsqueeze(0).expand(len(query), -1)
            return dense.readout(self, hiddens[-1], query, every)
        node_query = query.unsqueeze(1).expand(-1, data.num_nodes, -1)
        feature = torch.cat((hiddens if self.concat_hidden else hiddens[-1:]) + [node_query], dim=-1)
        return self.mlp(feature).squeeze(-1)   # (batch, num_nodes)


class Ultra(nn.Module):
    """models.py:7-26: relation model over data.relation_graph, then the entity model."""

    def __init__(self, rel_model_cfg, entity_model_cfg):
        super(Ultra, self).__init__()
        rel_model_cfg, entity_model_cfg = dict(rel_model_cfg), dict(entity_model_cfg)
        self.relation_model = globals()[rel_model_cfg.pop('class')](**rel_model_cfg)
        self.entity_model = globals()[entity_model_cfg.pop('class')](**entity_model_cfg)

    # ---- relation representations of every query relation, computed once (opt-in) ----
    # The relation model sees the relation graph and the query RELATION only (models.py:20-21): its output for relation r
    # does not depend on the batch's heads, tails or candidates.  A job that scores many batches over one graph with fixed
    # weights -- the filtered-ranking protocol: thousands of test triples over a few hundred relations -- may compute the
    # (num_relations, num_relations, dim) table once and pick rows from it: the same kernels on the same inputs, hence the
    # same bits.  NOT used by the benchmark's timed step (every step there runs the relation model, like the reference).
    def cache_relation_representations(self, data, chunk=8):
        """Fill the table for `data.relation_graph` under the current parameters (inference only); forward() then gathers
        from it while the graph object and the parameters stay the same.  Returns the table."""
        rg = data.relation_graph
        # (a live relation graph emits its edge list on demand only: its bits name the device)
        dev = rg.adjacency_bits.device if getattr(rg, "dense_adjacency", None) is not None else rg.edge_index.device
        num_rel = int(rg.num_nodes)
        was_training = self.training
        self.eval()
        table = None      # (preallocated on the first chunk: a list of chunks + torch.cat would hold the table twice at its peak)
        with torch.no_grad():
            for lo in range(0, num_rel, chunk):
                ids = torch.arange(lo, min(lo + chunk, num_rel), device=dev)
                if ids.numel() < chunk:      # (one batch shape for every call: plans and kernels see what a forward shows them)
                    ids = torch.cat([ids, ids.new_zeros(chunk - ids.numel())])
                rep = self.relation_model(rg, query=ids)
                if table is None:
                    table = rep.new_empty((num_rel,) + tuple(rep.shape[1:]))
                table[lo:min(lo + chunk, num_rel)] = rep[: min(chunk, num_rel - lo)]
        self.train(was_training)
        self._rel_table = table
        self._rel_table_key = self._relation_table_key(rg)
        return self._rel_table

    def drop_relation_cache(self):
        self._rel_table = None
        self._rel_table_key = None

    def _relation_table_key(self, rg):
        # (the version: a live relation graph changes in place, under one id -- tasks.LiveRelationGraph)
        return (id(rg), getattr(rg, "version", None), self._relation_param_state())

    def _relation_param_state(self):
        return tuple((p.data_ptr(), p._version) for p in self.relation_model.parameters())

    def _cached_relations(self, data, query_rels):
        table = getattr(self, "_rel_table", None)
        if table is None or self.training or torch.is_grad_enabled():
            return None
        if self._rel_table_key != self._relation_table_key(data.relation_graph):
            self.drop_relation_cache()       # another graph, or the weights moved: the table is stale
            return None
        return table.index_select(0, query_rels)

    def visualize(self, data, batch):
        """EntityNBFNet.visualize of one triple (1, 3) from the full model: the query relation's representations from the
        relation model (models.py:20-21), installed in the entity model the way its forward() does, then its paths and
        weights.  The model is left as it was: parameters, training flag, the entity model's installed representations and
        the relation cache."""
        assert batch.shape == (1, 3)
        ent = self.entity_model
        saved = (getattr(ent, "query", None), [getattr(l, "relation", None) for l in ent.layers])
        try:
            with torch.no_grad():
                rel = self._cached_relations(data, batch[:, 2])
                if rel is None:
                    rel = self.relation_model(data.relation_graph, query=batch[:, 2])
            ent.query = rel
            for layer in ent.layers:
                layer.relation = rel
            return ent.visualize(data, batch)
        finally:
            ent.query = saved[0]
            for layer, r in zip(ent.layers, saved[1]):
                layer.relation = r

    def visualize_batch(self, data, batch, chunk=16, delta=None):
        """visualize for S triples at once, batch (S, 3) -- they may differ in h, r and t: a list of (paths, weights), entry s
        what visualize(data, batch[s:s + 1]) returns.  Every chunk of `chunk` triples takes its query relations'
        representations from the relation model (or the relation cache, as visualize does), one entity-model forward and
        backward and the launches of one beam search (EntityNBFNet.visualize_batch).  The model is left as it was, like
        visualize.
        `delta` (an edited rspmm.GraphDelta of `data`): the explanations on (data, delta), defined as those of this
        call on delta.materialize(data).  The relation representations come from delta.live_view(data).relation_graph, as
        forward(delta=) takes them; the entity model keeps data's plan and CSR.  Edge gradients equal the materialised route's
        up to fp32 re-association (EntityNBFNet.edge_grads_batch); given the gradients the beam search is exact.  An unedited
        or absent delta is exactly the call without it."""
        if batch.dim() != 2 or batch.shape[1] != 3:
            raise ValueError("Expected a batch of triples of shape (S, 3), got %s" % (tuple(batch.shape),))
        if not isinstance(chunk, int) or chunk < 1:
            raise ValueError("chunk must be a positive int, got %r" % (chunk,))
        ent = self.entity_model
        if not hasattr(ent, "visualize_batch"):
            raise TypeError("%s cannot explain a batch; EntityNBFNet can" % type(ent).__name__)
        saved = (getattr(ent, "query", None), [getattr(l, "relation", None) for l in ent.layers])
        results = []
        live = delta is not None and delta.edited
        view = delta.live_view(data) if live else data
        try:
            for lo in range(0, batch.shape[0], chunk):
                part = batch[lo:lo + chunk]
                with torch.no_grad():
                    rel = self._cached_relations(view, part[:, 2])
                    if rel is None:
                        rel = self.relation_model(view.relation_graph, query=part[:, 2])
                ent.query = rel
                for layer in ent.layers:
                    layer.relation = rel
                results.extend(ent.visualize_batch(data, part, chunk=chunk, **({"delta": delta} if live else {})))
        finally:
            ent.query = saved[0]
            for layer, r in zip(ent.layers, saved[1]):
                layer.relation = r
        return results

    def forward(self, data, batch, edge_keep=None, delta=None, leave_out=None, leave_out_buffers=None):
        # batch: (bs, 1 + num_negs, 3); the relation is shared by every triple of a row
        # edge_keep (bs, num_edge): per-sample 0/1 keep masks over data's edge list (EntityNBFNet.forward); the relation graph is
        # not rebuilt -- the reference's filtered copy keeps data.relation_graph too
        # delta (rspmm.GraphDelta, a non-empty one; eval mode under no_grad): the scores on the graph WITH the delta's added facts
        # -- this forward on delta.materialize(data), bit for bit on reference-order plans.  The relation model runs on
        # delta.relation_graph, the entity model on data's cached plan with the touched rows fixed after every aggregate; where
        # that route does not apply (EntityNBFNet.forward), on the materialised graph.  An empty delta (or None): nothing changes.
        # leave_out (bs, 3) = stated facts (h, t, r), r direct (eval mode under no_grad, not with edge_keep): sample s is scored
        # without fact s and its inverse (remove_one_hop: without any edge between the two nodes).  Without edits this is
        # edge_keep=leave_one_out_keep(data, leave_out); with an edited delta sample s runs on delta.materialize(data) without
        # those edges -- base edges or the delta's own -- on data's cached plan (EntityNBFNet._forward_leave_out), the relation
        # model on delta.relation_graph, unmasked.  The definition, and the route where the engine does not serve the call: per
        # sample this forward on remove_easy_edges(delta.materialize(data), fact s).
        entity_kwargs = {}
        if leave_out is not None:
            if edge_keep is not None:
                raise ValueError("leave_out builds its own keep rows: not together with edge_keep")
            if self.training or torch.is_grad_enabled():
                raise ValueError("leave_out (leave-one-out verification) serves eval mode under torch.no_grad() only")
            if not hasattr(self.entity_model, "_forward_leave_out"):
                raise TypeError("%s has no leave-one-out route; EntityNBFNet has" % type(self.entity_model).__name__)
            entity_kwargs["leave_out"] = leave_out
            if leave_out_buffers is not None:
                entity_kwargs["leave_out_buffers"] = leave_out_buffers
            if delta is not None and delta.edited:
                served = data

                def definition():
                    full = delta.materialize(served)
                    rows = []
                    for s in range(batch.shape[0]):
                        h_index, t_index, r_index = leave_out[s:s + 1].unbind(-1)
                        rows.append(self.forward(self.entity_model.remove_easy_edges(full, h_index, t_index, r_index),
                                                 batch[s:s + 1]))
                    return torch.cat(rows)

                entity_kwargs["leave_out_fallback"] = definition
        if delta is not None and delta.edited:
            if edge_keep is not None:
                raise ValueError("a graph delta (added facts) is not combined with edge_keep: a caller-made mask runs over an "
                                 "edge list of which the caller cannot see the delta's part (leave-one-out: leave_out=)")
            if delta.relation_graph is not None and delta.relation_graph is not data.relation_graph:
                data = delta.live_view(data)
            entity_kwargs["delta"] = delta
        if edge_keep is not None:
            if self.training or torch.is_grad_enabled():
                raise ValueError("edge_keep (per-sample keep masks) serves eval mode under torch.no_grad() only")
            entity_kwargs["edge_keep"] = edge_keep
        prologue = None
        if getattr(self.entity_model, "prologue_supported", lambda b: False)(batch):
            # the batch prologue first: it also hands out every row's relation as a contiguous vector -- the relation model's
            # query -- which otherwise costs a strided 8-element copy kernel (6 us in the captured forward)
            prologue = dense.batch_prologue(batch, data.num_relations // 2)
            query_rels = prologue.rel_first
        else:
            query_rels = batch[:, 0, 2]
        prefill = None
        if PREFILL_LAYER0 and batch.is_cuda and batch.dim() == 3 and hasattr(self.entity_model, "prefill_layer0") \
                and "delta" not in entity_kwargs:      # (the delta's layer 0 is a full layer: nothing to prefill)
            prefill = self.entity_model.prefill_layer0(data, batch.shape[0])
        relation_representations = self._cached_relations(data, query_rels)
        if relation_representations is None:
            relation_representations = self.relation_model(data.relation_graph, query=query_rels)
        if prefill is not None or prologue is not None:
            return self.entity_model(data, relation_representations, batch, prefill=prefill, prologue=prologue, **entity_kwargs)
        return self.entity_model(data, relation_representations, batch, **entity_kwargs)
