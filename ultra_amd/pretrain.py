"""Multi-graph pre-training on the HIP engine (the reference's script/pretrain.py: config/transductive/pretrain_3g.yaml and
pretrain_4g.yaml).

  multigraph_collator   pretrain.py:26-37    a graph by edge-count multinomial, then randperm(n_g)[:len(batch)] of its targets
  batch_loader          pretrain.py:51-55    the DataLoader over the concatenated target triples, DistributedSampler, collator
  PretrainTrainer                            one captured step (train.GraphedTrainStep) per training graph, sharing the model,
                                             the fused capturable AdamW and its device step counter; short batches run eagerly
  train_and_validate    pretrain.py:40-138   epochs in chunks of ceil(num_epoch / 10), a checkpoint per chunk, validation,
                                             the best chunk reloaded
  test                  pretrain.py:141-218  per-graph metrics (eval.evaluate against each graph's filter graph) + mean MRR
  run                   pretrain.py:221-289  the CPU generator consumed in the reference's order: seed, fast_test subsets, model
                                             init (or cfg.checkpoint), the loop -- a seeded run draws what the reference draws

Random streams.  The batch source draws from the global CPU generator (creating the loader's iterator takes one draw, every batch
a multinomial and a randperm), the negatives from the device generator (tasks.prefetch_negatives, one batch ahead on a side
stream, each batch against its own graph).  The two are independent, so drawing batch k + 1 on the host while the GPU replays
step k changes neither sequence.

World size > 1.  Ranks are seeded `seed + rank` (pretrain.py:230) and so start from different weights; DDP would broadcast rank
0's parameters when it wraps the model, and the trainer does the same before its first warm-up.  Each rank then replays its own
graph's forward and backward and all-reduces one flat gradient bucket per step -- the eager short batch as well.
"""
import copy
import logging
import math
import os
from functools import partial
from itertools import islice

import torch
from torch.utils import data as torch_data

from . import distributed as udist
from . import eval as ueval
from . import models, tasks, train
from .data import Data

logger = logging.getLogger(__name__)


def _cfg(cfg, *path, default=None):
    for key in path:
        cfg = cfg.get(key, None) if isinstance(cfg, dict) else getattr(cfg, key, None)
        if cfg is None:
            return default
    return cfg


def target_triples(graph):
    """(n, 3) rows (h, t, r) of the graph's targets, on the graph's device."""
    return torch.cat([graph.target_edge_index, graph.target_edge_type.unsqueeze(0)]).t()


def multigraph_collator(batch, train_graphs, host_targets=None):
    """pretrain.py:26-37: one graph per batch, drawn with probability proportional to its edge count, then len(batch) of its
    targets by randperm.  Returns (graph id, (len(batch), 3) triples on the CPU).  host_targets: each graph's target triples
    on the CPU (the batch is gathered on the host and copied to the device beside the step)."""
    probs = torch.tensor([graph.edge_index.shape[1] for graph in train_graphs]).float()
    probs /= probs.sum()
    graph_id = torch.multinomial(probs, 1, replacement=False).item()
    targets = host_targets[graph_id] if host_targets is not None else target_triples(train_graphs[graph_id]).cpu()
    edge_mask = torch.randperm(targets.shape[0])[:len(batch)]
    return graph_id, targets[edge_mask]


def batch_loader(train_graphs, batch_size, world_size=1, rank=0):
    """pretrain.py:51-55: a DataLoader over the concatenated target triples of every training graph with a DistributedSampler
    (the sampler only decides how many rows each batch has; the collator picks them).  Returns (loader, sampler)."""
    host = [target_triples(g).cpu() for g in train_graphs]
    train_triplets = torch.cat(host)
    sampler = torch_data.DistributedSampler(train_triplets, world_size, rank)
    loader = torch_data.DataLoader(train_triplets, batch_size, sampler=sampler,
                                   collate_fn=partial(multigraph_collator, train_graphs=train_graphs, host_targets=host))
    return loader, sampler


def fast_test_subsets(valid_graphs, num_edges):
    """pretrain.py:238-243: a copy of every validation graph with `num_edges` of its targets picked by randperm (global CPU
    generator, one draw per graph in order)."""
    out = []
    for graph in valid_graphs:
        graph = copy.copy(graph)
        mask = torch.randperm(graph.target_edge_index.shape[1])[:num_edges]
        graph.target_edge_index = graph.target_edge_index[:, mask.to(graph.target_edge_index.device)]
        graph.target_edge_type = graph.target_edge_type[mask.to(graph.target_edge_type.device)]
        if hasattr(graph, "target_triples"):
            graph.target_triples = target_triples(graph)
        out.append(graph)
    return out


def filter_graphs(train_data, valid_data, test_data):
    """pretrain.py:265-271: per graph, the targets of all three splits (no inverses) -- the transductive filtered ranking."""
    return [Data(edge_index=torch.cat([a.target_edge_index, b.target_edge_index, c.target_edge_index], dim=1),
                 edge_type=torch.cat([a.target_edge_type, b.target_edge_type, c.target_edge_type]),
                 num_nodes=a.num_nodes, num_relations=a.num_relations)
            for a, b, c in zip(train_data, valid_data, test_data)]


def example_batch(graph, batch_size, num_negative):
    """A (batch_size, 1 + num_negative, 3) batch of the step's layout, with no random draw: the graph's first targets, the
    first half with tail candidates, the second with head candidates (tasks.negative_sampling's layout).  What a capture's
    warm-up runs on; the warm-up leaves no trace on the parameters or the optimiser."""
    pos = target_triples(graph)
    pos = pos[torch.arange(batch_size, device=pos.device) % pos.shape[0]]
    cand = torch.arange(1, num_negative + 1, device=pos.device) % int(graph.num_nodes)
    h, t, r = (pos[:, i:i + 1].repeat(1, num_negative + 1) for i in range(3))
    half = batch_size // 2
    t[:half, 1:] = cand
    h[half:, 1:] = cand
    return torch.stack([h, t, r], dim=-1)


class PretrainTrainer(object):
    """trainer.step(graph_id, batch) -> loss (0-d device tensor, no host synchronisation).

    capture=True: a train.GraphedTrainStep per training graph for full batches of `batch_size` rows, all over the same model and
    optimizer (which must be capturable: train.make_adamw(model, capturable=True)).  Every capture starts with .grad unset (the
    step's own warm-up does that), and each step holds its own gradient tensors: the graphs write them, and no later capture
    may take their memory.  Each capture has a memory pool of its own.  Build the trainer before any eager training step on the
    model: such a step leaves the model holding its autograd graph (EntityNBFNet.query), whose gradient accumulators belong to
    the stream of that step, and a capture must not reach them.  Batches of another row count (the short last batch of an
    epoch) run eagerly -- with the same one all-reduce of one flat bucket at world size > 1."""

    def __init__(self, model, train_graphs, optimizer, batch_size, num_negative, adversarial_temperature=1.0, capture=True,
                 process_group=None, warmup=3):
        self.model, self.graphs, self.optimizer = model, list(train_graphs), optimizer
        self.batch_size, self.num_negative, self.temperature = int(batch_size), int(num_negative), adversarial_temperature
        self.group = process_group
        self.world = torch.distributed.get_world_size(process_group) if (
            torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
        if self.world > 1:
            self.broadcast_parameters()
        self.steps = [None] * len(self.graphs)
        self._replayed = set()
        if capture:
            for gid, graph in enumerate(self.graphs):
                example = example_batch(graph, self.batch_size, self.num_negative)
                self.steps[gid] = train.GraphedTrainStep(model, graph, optimizer, example, adversarial_temperature,
                                                         self.num_negative, warmup, process_group)
            optimizer.zero_grad(set_to_none=True)

    @torch.no_grad()
    def broadcast_parameters(self):
        """rank 0's parameters and buffers to every rank (what DistributedDataParallel does when it wraps the model)."""
        for t in list(self.model.parameters()) + list(self.model.buffers()):
            torch.distributed.broadcast(t.data, src=0, group=self.group)

    def step(self, graph_id, batch):
        captured = self.steps[graph_id]
        if captured is not None and batch.shape[0] == self.batch_size:
            self._replayed.add(graph_id)
            return captured(batch)
        return self.eager_step(self.graphs[graph_id], batch)

    def eager_step(self, graph, batch):
        """train.train_step with, at world size > 1, the captured steps' one all-reduce of one flat gradient bucket."""
        model, opt = self.model, self.optimizer
        model.train()
        opt.zero_grad(set_to_none=True)       # (the grads may be a captured step's tensors: never accumulate into them)
        pred = model(graph, batch)
        loss = train.ranking_loss(pred, self.temperature, self.num_negative)
        loss.backward()
        if self.world > 1:
            train.all_reduce_grads([p for group in opt.param_groups for p in group["params"]], self.world, self.group)
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss.detach()

    def parameters_updated(self):
        """A replay updates the parameters in place without bumping their version counters, and the inference paths cache what
        they derive from the parameters under those counters (the stacked relation projections, the relation table, captured
        forwards).  Call this before the model is used outside the training steps (validation, a checkpoint)."""
        for p in self.model.parameters():
            torch.autograd.graph.increment_version(p)

    def check(self):
        """The row-uniformity assertion of models.py:196-197 for the last batch of every graph replayed since the previous check
        (a host synchronisation).  A capture that has not been replayed holds no result yet: it is not read."""
        for graph_id in sorted(self._replayed):
            self.steps[graph_id].check()
        self._replayed.clear()


def _train_cfg(cfg):
    return dict(batch_size=int(_cfg(cfg, "train", "batch_size")), num_epoch=int(_cfg(cfg, "train", "num_epoch", default=0)),
                log_interval=int(_cfg(cfg, "train", "log_interval", default=100)),
                num_negative=int(_cfg(cfg, "task", "num_negative")),
                strict=bool(_cfg(cfg, "task", "strict_negative", default=True)),
                temperature=float(_cfg(cfg, "task", "adversarial_temperature", default=0.0)),
                metrics=tuple(_cfg(cfg, "task", "metric", default=("mr", "mrr", "hits@1", "hits@3", "hits@10"))))


def make_optimizer(cfg, model, capture=True):
    """cfg.optimizer (class name + arguments, pretrain.py:59-60).  AdamW is built fused and capturable (train.make_adamw), as the
    captured step needs it."""
    opt_cfg = dict(_cfg(cfg, "optimizer"))
    cls = opt_cfg.pop("class")
    if cls == "AdamW":
        return train.make_adamw(model, capturable=capture, **opt_cfg)
    if capture:
        raise ValueError("the captured pre-training step needs AdamW (fused, capturable); got %s" % cls)
    return getattr(torch.optim, cls)(model.parameters(), **opt_cfg)


def train_and_validate(cfg, model, train_data, valid_data, filtered_data=None, batch_per_epoch=None, working_dir=".",
                       capture=True, eval_batch_size=8, stats=None):
    """pretrain.py:40-138.  Returns the best validation result (mean MRR over the graphs), or None when num_epoch is 0.
    Losses stay on the device: they are read at `log_interval` and once per epoch.  stats: a dict that receives the per-epoch
    mean losses and the chunk results."""
    c = _train_cfg(cfg)
    if c["num_epoch"] == 0:
        return None
    world, rank = udist.world_size(), udist.rank()
    loader, sampler = batch_loader(train_data, c["batch_size"], world, rank)
    batch_per_epoch = batch_per_epoch or len(loader)
    optimizer = make_optimizer(cfg, model, capture)
    logger.warning("Number of parameters: %d", sum(p.numel() for p in model.parameters()))
    trainer = PretrainTrainer(model, train_data, optimizer, c["batch_size"], c["num_negative"], c["temperature"], capture=capture)

    step = math.ceil(c["num_epoch"] / 10)
    best_result, best_epoch = float("-inf"), -1
    batch_id = 0
    for i in range(0, c["num_epoch"], step):
        model.train()
        for epoch in range(i, min(c["num_epoch"], i + step)):
            losses = []
            sampler.set_epoch(epoch)
            batches = islice(loader, batch_per_epoch)
            for graph_id, batch in tasks.prefetch_negatives(batches, train_data, c["num_negative"], strict=c["strict"]):
                loss = trainer.step(graph_id, batch).clone()       # (a captured step's loss is overwritten by its next replay)
                if rank == 0 and batch_id % c["log_interval"] == 0:
                    logger.warning("binary cross entropy: %g", loss.item())
                losses.append(loss)
                batch_id += 1
            trainer.check()
            trainer.parameters_updated()
            avg = torch.stack(losses).mean().item() if losses else float("nan")
            if stats is not None:
                stats.setdefault("epoch_loss", []).append(avg)
            if rank == 0:
                logger.warning("Epoch %d end: average binary cross entropy: %g", epoch, avg)
        epoch = min(c["num_epoch"], i + step)
        path = os.path.join(working_dir, "model_epoch_%d.pth" % epoch)
        if rank == 0:
            torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()}, path)
        _barrier()
        _, result = test(cfg, model, valid_data, filtered_data=filtered_data, eval_batch_size=eval_batch_size)
        if stats is not None:
            stats.setdefault("valid", []).append((epoch, result))
        if result > best_result:
            best_result, best_epoch = result, epoch
    logger.warning("Load checkpoint from model_epoch_%d.pth", best_epoch)
    state = torch.load(os.path.join(working_dir, "model_epoch_%d.pth" % best_epoch), map_location=next(model.parameters()).device)
    model.load_state_dict(state["model"])
    _barrier()
    return best_result


def _barrier():
    if udist.world_size() > 1:
        torch.distributed.barrier()


def loader_draw(graph, batch_size, world_size=1, rank=0):
    """The one draw of the global CPU generator that the reference's test() takes per graph (pretrain.py:150-152: a DataLoader
    iterator is created, and creating one seeds its workers from the global generator)."""
    triples = target_triples(graph)
    iter(torch_data.DataLoader(triples, batch_size, sampler=torch_data.DistributedSampler(triples, world_size, rank)))


@torch.no_grad()
def test(cfg, model, test_data, filtered_data=None, eval_batch_size=8):
    """pretrain.py:141-218: every graph in turn through eval.evaluate (filtered ranking against filtered_data[i], or the graph
    itself).  Returns ([metrics of each graph], mean MRR over the graphs).  Per graph the reference builds a DataLoader iterator,
    which takes one draw of the global CPU generator: taken here too, so that a seeded run stays on the reference's stream."""
    world, rank = udist.world_size(), udist.rank()
    metrics = _train_cfg(cfg)["metrics"]
    per_graph = []
    for k, graph in enumerate(test_data):
        loader_draw(graph, int(_cfg(cfg, "train", "batch_size")), world, rank)
        filt = filtered_data[k] if filtered_data is not None else graph
        result = ueval.evaluate(model, graph, batch_size=eval_batch_size, filtered_data=filt,
                                metrics=tuple(m for m in metrics if m != "mrr") + ("mrr",))
        if rank == 0:
            for m in metrics:
                logger.warning("%s: %g", m, result[m])
        per_graph.append(result)
    return per_graph, sum(float(r["mrr"]) for r in per_graph) / len(per_graph)


def run(cfg, seed, train_data, valid_data, test_data, device, working_dir=".", capture=True, eval_batch_size=8):
    """pretrain.py:221-289 from already built datasets (lists of graphs on any device): the global CPU generator is consumed in
    the reference's order -- seed + rank, the fast_test subsets, the model's initialisation (or cfg.checkpoint) -- then the
    loop, then validation and test on the full splits.  Returns (model, valid per-graph metrics, test per-graph metrics)."""
    torch.manual_seed(seed + udist.rank())
    fast = _cfg(cfg, "train", "fast_test")
    short_valid = fast_test_subsets(valid_data, int(fast)) if fast is not None else None
    train_data = [g.to(device) for g in train_data]
    valid_data = [g.to(device) for g in valid_data]
    test_data = [g.to(device) for g in test_data]
    if short_valid is not None:
        short_valid = [g.to(device) for g in short_valid]
    model = models.Ultra(rel_model_cfg=dict(_cfg(cfg, "model", "relation_model")),
                         entity_model_cfg=dict(_cfg(cfg, "model", "entity_model")))
    checkpoint = _cfg(cfg, "checkpoint")
    if checkpoint is not None:
        model.load_state_dict(torch.load(checkpoint, map_location="cpu")["model"])
    model = model.to(device)
    filtered_data = filter_graphs(train_data, valid_data, test_data)
    train_and_validate(cfg, model, train_data, short_valid if short_valid is not None else valid_data, filtered_data,
                       batch_per_epoch=_cfg(cfg, "train", "batch_per_epoch"), working_dir=working_dir, capture=capture,
                       eval_batch_size=eval_batch_size)
    valid_metrics, _ = test(cfg, model, valid_data, filtered_data, eval_batch_size)
    test_metrics, _ = test(cfg, model, test_data, filtered_data, eval_batch_size)
    return model, valid_metrics, test_metrics
