"""Training UltraQuery on complex queries (reference: ultra/ultraquery.py:34-83, script/run_query.py:53-156).

Traversal dropout is a 0/1 keep vector over the static edge list (ultra_traversal_dropout, csrc/query_train_kernels.hip): the
entity layers read it through the cached plan of the full graph, as the fine-tuning step reads its easy-edge vector, and the
relation graph of the dropped graph becomes a 0/1 vector over the static relation graph's edges
(ultra_relation_graph_bits_keep + ultra_relation_graph_edge_keep), so the relation model's plan is never rebuilt either.
The query loss and its gradient are one launch (ultra_query_loss).  The loop follows run_query.py at world size 1.
DESIGN.md section 10.4.
"""
import logging
import math
import os
from collections import OrderedDict
from itertools import islice

import torch

from ._lib import check, lib, ptr, stream_of
from .data import Data

logger = logging.getLogger(__name__)

_DEG_CACHE = OrderedDict()
_DEG_CACHE_SIZE = 8


def degrees(edge_index, num_node):
    """(deg_out, deg_in) int32 (num_node) of the full graph, cached per graph: the must-keep rule of ultraquery.py:66-69."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), str(edge_index.device), int(num_node))
    hit = _DEG_CACHE.get(key)
    if hit is not None:
        _DEG_CACHE.move_to_end(key)
        return hit[0]
    deg = (torch.bincount(edge_index[0], minlength=num_node).to(torch.int32),
           torch.bincount(edge_index[1], minlength=num_node).to(torch.int32))
    _DEG_CACHE[key] = (deg, edge_index)
    while len(_DEG_CACHE) > _DEG_CACHE_SIZE:
        _DEG_CACHE.popitem(last=False)
    return deg


def drop_table(ratio, batch, device):
    """q[k] = 1 - (1 - ratio)^k for k = 0 .. 2 batch: the probability that one of k independent draws lands at or below
    `ratio` (computed in fp64, rounded once to fp32)."""
    k = torch.arange(2 * batch + 1, dtype=torch.float64)
    return (1 - (1 - float(ratio)) ** k).to(torch.float32).to(device)


def traversal_dropout(edge_index, edge_type, num_node, num_relation, sym, r_index, ratio, more_dropout=0.0,
                      inverse_rel_plus_one=False, u1=None, u2=None, return_k=False):
    """The keep vector (num_edge) fp32 of UltraQuery.traversal_dropout for one projection (ultra_traversal_dropout).
    sym (batch, num_node) fp32 / fp64 symbolic sets, r_index (batch) relations.  u1 / u2: the uniforms (num_edge) fp32,
    drawn with torch.rand on the device when not given (u2 only where more_dropout > 0).  return_k: also k(e) int32."""
    if sym.dtype not in (torch.float32, torch.float64):
        raise TypeError("traversal dropout takes fp32 or fp64 symbolic sets, got %s" % sym.dtype)
    num_edge = edge_index.shape[1]
    batch = sym.shape[0]
    if sym.dim() != 2 or sym.shape[1] != num_node or r_index.shape != (batch,) or batch == 0:
        raise ValueError("Expected sym (batch, %d) and r_index (batch,), got %s and %s"
                         % (num_node, tuple(sym.shape), tuple(r_index.shape)))
    if not (edge_index.is_cuda and sym.is_cuda and r_index.is_cuda):
        raise RuntimeError("traversal dropout runs on the GPU: graph, sets and relations on one CUDA device")
    dev = edge_index.device
    deg_out, deg_in = degrees(edge_index, num_node)
    ei, et = edge_index.contiguous(), edge_type.contiguous()
    sym, r = sym.contiguous(), r_index.to(torch.int64).contiguous()
    if u1 is None:
        u1 = torch.rand(num_edge, device=dev)
    more = float(more_dropout)
    if more > 0 and u2 is None:
        u2 = torch.rand(num_edge, device=dev)
    u1 = u1.to(torch.float32).contiguous()
    u2 = u2.to(torch.float32).contiguous() if (more > 0 and u2 is not None) else None
    q = drop_table(ratio, batch, dev)
    words = lib.ultra_traversal_dropout_mask_words(batch)
    masks = torch.empty(2 * num_relation * words, dtype=torch.int32, device=dev)
    keep = torch.empty(num_edge, dtype=torch.float32, device=dev)
    k = torch.empty(num_edge, dtype=torch.int32, device=dev) if return_k else None
    check(lib.ultra_traversal_dropout(ei.data_ptr(), et.data_ptr(), num_edge, num_node, num_relation, int(bool(inverse_rel_plus_one)),
                                      deg_out.data_ptr(), deg_in.data_ptr(), r.data_ptr(), batch,
                                      0 if sym.dtype == torch.float32 else 1, sym.data_ptr(), q.data_ptr(), u1.data_ptr(),
                                      ptr(u2), more, masks.data_ptr(), keep.data_ptr(),
                                      ptr(k), stream_of(keep)))
    return (keep, k) if return_k else keep


def traversal_dropout_reference(edge_index, edge_type, num_node, num_relation, sym, r_index, ratio, more_dropout=0.0,
                                inverse_rel_plus_one=False, u1=None, u2=None):
    """The torch restatement of the dropout rule (any device): (keep (num_edge) fp32, k (num_edge) int32)."""
    src, dst = edge_index
    r = r_index.to(torch.int64)
    if inverse_rel_plus_one:
        inv = r ^ 1
    else:
        half = num_relation // 2
        inv = torch.where(r >= half, r - half, r + half)
    nz = sym != 0                                                                  # what nonzero() selects
    direct = (edge_type.unsqueeze(0) == r.unsqueeze(1)) & nz[:, src]               # (batch, E)
    inverse = (edge_type.unsqueeze(0) == inv.unsqueeze(1)) & nz[:, dst]
    k = (direct.sum(0) + inverse.sum(0)).to(torch.int32)
    deg_out = torch.bincount(src, minlength=num_node)
    deg_in = torch.bincount(dst, minlength=num_node)
    must_keep = (deg_out[src] <= 1) | (deg_in[dst] <= 1)
    q = drop_table(ratio, sym.shape[0], edge_index.device)
    drop = (k > 0) & (u1 <= q[k.long()])
    if more_dropout > 0:
        drop = drop | (u2 <= more_dropout)
    drop = drop & ~must_keep
    return (~drop).to(torch.float32), k


def relation_graph_bits_keep(graph, keep):
    """(adj, row_counts) of the relation graph of `graph` without the edges whose keep is 0 (ultra_relation_graph_bits_keep);
    the same layout as tasks.relation_graph_bits."""
    ei, et = graph.edge_index.to(torch.int64).contiguous(), graph.edge_type.to(torch.int64).contiguous()
    keep = keep.to(torch.float32).contiguous()
    n, r = int(graph.num_nodes), int(graph.num_relations)
    w = (r + 31) // 32
    dev = ei.device
    hbits = torch.zeros(n * w, dtype=torch.int32, device=dev)
    tbits = torch.zeros(n * w, dtype=torch.int32, device=dev)
    adj = torch.zeros(4, r, w, dtype=torch.int32, device=dev)
    counts = torch.empty(4 * r, dtype=torch.int64, device=dev)
    check(lib.ultra_relation_graph_bits_keep(ei.data_ptr(), et.data_ptr(), keep.data_ptr(), ei.shape[1], n, r, hbits.data_ptr(),
                                             tbits.data_ptr(), adj.data_ptr(), counts.data_ptr(), stream_of(ei)))
    return adj, counts


def relation_graph_keep(graph, keep):
    """The relation graph of the dropped graph as a 0/1 fp32 vector over the edges of graph.relation_graph (which it can only
    lose): what the relation model reads through the static relation graph's cached plan."""
    adj, _ = relation_graph_bits_keep(graph, keep)
    rg = graph.relation_graph
    rei, ret = rg.edge_index.to(torch.int64).contiguous(), rg.edge_type.to(torch.int64).contiguous()
    out = torch.empty(rei.shape[1], dtype=torch.float32, device=rei.device)
    check(lib.ultra_relation_graph_edge_keep(adj.data_ptr(), int(graph.num_relations), rei.data_ptr(), ret.data_ptr(), rei.shape[1],
                                             out.data_ptr(), stream_of(out)))
    return out


def build_dropped_relation_graph(graph, keep):
    """The relation graph of the dropped graph as its own edge list (ultra_relation_graph_emit over the keep-aware bits): the
    reference's build_relation_graph of the filtered copy, edge for edge."""
    adj, counts = relation_graph_bits_keep(graph, keep)
    r = int(graph.num_relations)
    offsets = torch.cumsum(counts, 0) - counts
    total = int(counts.sum())
    dev = adj.device
    edge_index = torch.empty(2, total, dtype=torch.int64, device=dev)
    edge_type = torch.empty(total, dtype=torch.int64, device=dev)
    check(lib.ultra_relation_graph_emit(adj.data_ptr(), offsets.data_ptr(), r, total, edge_index.data_ptr(), edge_type.data_ptr(),
                                        stream_of(adj)))
    return Data(edge_index=edge_index, edge_type=edge_type, num_nodes=r, num_relations=4)


# ---- the query loss (run_query.py:94-114) ----
class _QueryLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, temperature):
        p = pred.detach().float().contiguous()
        t = target.to(torch.uint8).contiguous()
        rows, n = p.shape
        work = torch.zeros(rows + 1, dtype=torch.float32, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        check(lib.ultra_query_loss(p.data_ptr(), t.data_ptr(), rows, n, float(temperature), work.data_ptr(), loss.data_ptr(),
                                   grad.data_ptr(), stream_of(p)))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return grad * grad_out, None, None


def query_loss(pred, target, adversarial_temperature=0.0):
    """run_query.py:94-114 on (rows, num_nodes) logits and 0/1 targets: BCE with logits, positives weighted 1 / num_pos,
    negatives by softmax(pred / T) (a constant) or uniformly (T = 0); one launch forward, the gradient comes with it."""
    if pred.dim() != 2 or target.shape != pred.shape:
        raise ValueError("query_loss takes pred and target of one shape (rows, num_nodes)")
    if not pred.is_cuda:
        raise RuntimeError("query_loss runs on the GPU (ultra_query_loss)")
    if pred.dtype != torch.float32:
        raise TypeError("query_loss takes fp32 logits, got %s" % pred.dtype)
    return _QueryLoss.apply(pred, target > 0.5 if target.is_floating_point() else target != 0, float(adversarial_temperature))


def query_loss_reference(pred, target, adversarial_temperature=0.0):
    """The torch restatement (run_query.py:96-114 in one formula per row; any device, any float dtype)."""
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, target.to(pred.dtype), reduction="none")
    is_pos = target > 0.5
    num_pos = is_pos.sum(-1, keepdim=True).to(pred.dtype)
    num_neg = (~is_pos).sum(-1, keepdim=True).to(pred.dtype)
    with torch.no_grad():
        if adversarial_temperature > 0:
            logit = (pred / adversarial_temperature).masked_fill(is_pos, float("-inf"))
            neg_w = torch.softmax(logit, dim=-1)
        else:
            neg_w = (~is_pos).to(pred.dtype) / num_neg
        weight = torch.where(is_pos, 1 / num_pos, neg_w)
    return ((loss * weight).sum(-1) / weight.sum(-1)).mean()


# ---- the loop (run_query.py:40-156) ----
def predict_and_target(model, graph, batch):
    """run_query.py:40-64 in training mode: the executor's logits with symbolic traversal on, and the easy answers as
    float targets."""
    pred = model(graph, batch["query"], symbolic_traversal=model.training)
    return pred, batch["easy_answer"].float()


def train_step(model, graph, batch, optimizer, adversarial_temperature=0.0):
    """One optimiser step on one batch (run_query.py:89-121); returns the loss as a Python float."""
    model.train()
    pred, target = predict_and_target(model, graph, batch)
    loss = query_loss(pred, target, adversarial_temperature)
    loss.backward()
    optimizer.step()
    optimizer.zero_grad()
    return loss.item()


def _cfg(cfg, *path, default=None):
    for key in path:
        cfg = cfg.get(key, None) if isinstance(cfg, dict) else getattr(cfg, key, None)
        if cfg is None:
            return default
    return cfg


def train_and_validate(cfg, model, train_graph, train_data, valid_graph, valid_data, query_id2type, device,
                       batch_per_epoch=None, working_dir="."):
    """run_query.py:53-156 at world size 1: the optimizer from cfg.optimizer (class name and its arguments), epochs in chunks
    of ceil(num_epoch / 10), a checkpoint model_epoch_<epoch>.pth per chunk, validation by query_eval.test_queries and, at
    the end, the weights of the chunk with the best MRR.  Returns the best validation metrics."""
    from torch.utils import data as torch_data
    from . import distributed as udist, query_eval

    num_epoch = int(_cfg(cfg, "train", "num_epoch", default=0))
    if num_epoch == 0:
        return None
    if udist.world_size() > 1:
        raise NotImplementedError("UltraQuery training runs at world size 1 only")
    batch_size = int(_cfg(cfg, "train", "batch_size"))
    log_interval = int(_cfg(cfg, "train", "log_interval", default=100))
    temperature = float(_cfg(cfg, "task", "adversarial_temperature", default=0.0))
    metrics = tuple(_cfg(cfg, "task", "metric", default=("mrr", "hits@1", "hits@3", "hits@10")))
    opt_cfg = dict(_cfg(cfg, "optimizer"))
    cls = opt_cfg.pop("class")
    optimizer = getattr(torch.optim, cls)(model.parameters(), **opt_cfg)
    logger.warning("Number of parameters: %d", sum(p.numel() for p in model.parameters()))

    sampler = torch_data.DistributedSampler(train_data, 1, 0)
    loader = torch_data.DataLoader(train_data, batch_size, sampler=sampler)
    batch_per_epoch = batch_per_epoch or len(loader)
    train_graph = train_graph.to(device)
    step = math.ceil(num_epoch / 10)
    best_result, best_epoch, best_metrics = float("-inf"), -1, None
    batch_id = 0
    for i in range(0, num_epoch, step):
        model.train()
        for epoch in range(i, min(num_epoch, i + step)):
            losses = []
            sampler.set_epoch(epoch)
            for batch in islice(loader, batch_per_epoch):
                batch = {k: v.to(device) for k, v in batch.items()}
                loss = train_step(model, train_graph, batch, optimizer, temperature)
                if batch_id % log_interval == 0:
                    logger.warning("binary cross entropy: %g", loss)
                losses.append(loss)
                batch_id += 1
            logger.warning("Epoch %d end: average binary cross entropy: %g", epoch, sum(losses) / max(len(losses), 1))
        epoch = min(num_epoch, i + step)
        path = os.path.join(working_dir, "model_epoch_%d.pth" % epoch)
        torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()}, path)
        result = query_eval.test_queries(model, valid_graph, valid_data, batch_size, query_id2type, metrics=metrics,
                                         device=device)
        if result["mrr"] > best_result:
            best_result, best_epoch, best_metrics = result["mrr"], epoch, result
    state = torch.load(os.path.join(working_dir, "model_epoch_%d.pth" % best_epoch), map_location=device)
    model.load_state_dict(state["model"])
    return best_metrics
