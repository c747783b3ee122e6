"""Timing of UltraQuery training steps at FB15k237's shape (14,541 nodes, 544,230 edges, 474 relations) on one GPU.

    python tools/query_train_bench.py [--batch 8 32] [--steps 10]

Prints one JSON line.  Per batch size (queries of all 14 BetaE types, sampled by ultra_amd.query_data.sample_queries over
the synthetic graph): training steps/s of query_train.train_step (forward, loss, backward, Adam; host clock around a device
synchronise, after two warm-up steps), and its parts, each by device events over the same steps:
  dropout          ultra_traversal_dropout (+ its uniforms), per step summed over the projections
  relation_graph   the keep-aware relation graph and its keep vector over the static relation graph
  projection       RelationProjection forward calls; backward: the whole loss.backward() (nearly all of it the projections')
  loss             ultra_query_loss
  executor         the rest: the torch stack machine, fuzzy logic, symbolic traversal, optimizer
The weights are the reference's ultraquery.pth as recorded in tests/golden/ultraquery.pt.xz.
"""
import argparse
import io
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, query_data, query_train, synthetic, ultraquery  # noqa: E402


class Timer(object):
    """Device-event time of every call of a wrapped function, summed per step."""

    def __init__(self):
        self.ms = 0.0
        self.pending = []

    def wrap(self, fn):
        def inner(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            self.pending.append((s, e))
            return out
        return inner

    def collect(self):
        torch.cuda.synchronize()
        ms = sum(s.elapsed_time(e) for s, e in self.pending)
        self.pending = []
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz"), "rb") as f:
        weights = torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)["weights"]
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=False)
    train, ds = query_data.sample_queries(kg, max(args.batch) // 7 + 2, seed=1)
    graph = train.to(dev)
    from ultra_amd import tasks
    tasks.build_relation_graph(graph)
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = ultraquery.UltraQuery(models.Ultra(**cfg), logic="product", dropout_ratio=0.25)
    model.load_state_dict(weights, strict=True)
    model.to(dev).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=5e-4)

    timers = {k: Timer() for k in ("dropout", "relation_graph", "projection_forward", "projection_backward", "loss")}
    orig = (query_train.traversal_dropout, query_train.relation_graph_keep, query_train.query_loss)
    query_train.traversal_dropout = timers["dropout"].wrap(orig[0])
    query_train.relation_graph_keep = timers["relation_graph"].wrap(orig[1])
    query_train.query_loss = timers["loss"].wrap(orig[2])
    proj_forward = model.model.forward
    model.model.forward = timers["projection_forward"].wrap(proj_forward)

    # the backward as a whole, by events (but for the executor's elementwise fuzzy logic it is the projections')
    bwd = timers["projection_backward"]

    def step(batch):
        model.train()
        pred, target = query_train.predict_and_target(model, graph, batch)
        loss = query_train.query_loss(pred, target, 0.2)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss.backward()
        e.record()
        bwd.pending.append((s, e))
        optimizer.step()
        optimizer.zero_grad()
        return loss

    out = {"shape": {"num_node": graph.num_nodes, "num_edge": int(graph.edge_index.shape[1]),
                     "num_relation": int(graph.num_relations)}, "batches": {}}
    items = [ds[i] for i in range(len(ds))]
    for bs in args.batch:
        torch.manual_seed(0)
        chosen = [items[i] for i in torch.randperm(len(items))[:bs].tolist()]
        batch = {k: torch.stack([torch.as_tensor(it[k]) for it in chosen]).to(dev) for k in ("query", "easy_answer")}
        for _ in range(2):
            step(batch)
        for t in timers.values():
            t.collect()
        walls, parts = [], {k: [] for k in timers}
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(batch)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            for k, t in timers.items():
                parts[k].append(t.collect())
        wall = statistics.median(walls)
        med = {k: round(statistics.median(v), 3) for k, v in parts.items()}
        accounted = med["dropout"] + med["relation_graph"] + med["projection_forward"] + med["projection_backward"] + med["loss"]
        out["batches"][str(bs)] = dict(steps_per_s=round(1e3 / wall, 2), step_ms=round(wall, 3), dropout_ms=med["dropout"],
                                       relation_graph_ms=med["relation_graph"],
                                       projection_forward_ms=med["projection_forward"],
                                       backward_ms=med["projection_backward"], loss_ms=med["loss"],
                                       executor_ms=round(wall - accounted, 3))
    query_train.traversal_dropout, query_train.relation_graph_keep, query_train.query_loss = orig
    model.model.forward = proj_forward
    print(json.dumps(out))


if __name__ == "__main__":
    main()
