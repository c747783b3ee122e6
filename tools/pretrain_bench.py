"""Timing of the multi-graph pre-training step at the 3g shape (FB15k237, WN18RR, CoDEx-M: config/transductive/pretrain_3g.yaml)
on one GPU: batch 64, 512 strict negatives, temperature 1, AdamW.

    python tools/pretrain_bench.py [--graphs fb15k237 wn18rr codex_m] [--steps 10] [--warmup 3]

Prints one JSON line.  Synthetic graphs of the public shapes (ultra_amd.synthetic.make_split); random initial weights.  Per graph:
  eager_ms       train.train_step (the step launched op by op), device events around each step, warm-up excluded (median)
  captured_ms    the same step as one hipGraph replay (pretrain.PretrainTrainer), device events, warm-up excluded (median)
  filter_us      ultra_easy_edge_keep_table alone (clear + insert + probe) on that graph's batch, device events (median)
and overall: peak device memory with the first graph's capture alone (peak_gb_one) and with all of them (peak_gb_all), and the
host time per step of the batch source (DataLoader + multigraph_collator: a multinomial and randperm(n_g)) and of the strict
sampler's launches -- the host work that runs beside a replay.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import dense, models, pretrain, synthetic, tasks, train  # noqa: E402


def _log(msg):
    print("[pretrain_bench] %s" % msg, file=sys.stderr, flush=True)


def _median_ms(fn, n):
    pairs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="+", default=["fb15k237", "wn18rr", "codex_m"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--negative", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    graphs = []
    for name in args.graphs:
        s = synthetic.SHAPES[name]
        g = synthetic.make_split(s["num_node"], s["num_triple"], s["num_relation_base"], num_valid=64, num_test=64, seed=7,
                                 relation_graph=False)[0].to(dev)
        graphs.append(tasks.build_relation_graph(g))
        _log("graph %s ready" % name)
    torch.manual_seed(0)
    model = models.Ultra(**synthetic.default_model_cfg()).to(dev).train()
    bs, neg = args.batch, args.negative
    batches = []
    for g in graphs:
        pos = pretrain.target_triples(g)[torch.randperm(g.target_edge_index.shape[1], device=dev)[:bs]]
        batches.append(tasks.negative_sampling(g, pos, neg, strict=True))
    out = {"batch": bs, "num_negative": neg, "graphs": {}}

    opt = train.make_adamw(model, lr=5e-4)
    for name, g, b in zip(args.graphs, graphs, batches):
        for _ in range(args.warmup):
            train.train_step(model, g, b, opt, 1.0, neg)
        row = out["graphs"][name] = {"num_node": int(g.num_nodes), "num_edge": int(g.num_edges)}
        row["eager_ms"] = _median_ms(lambda: train.train_step(model, g, b, opt, 1.0, neg), args.steps)
        _log("%s eager %.2f ms" % (name, row["eager_ms"]))
        h, t, r = b.unbind(-1)
        row["filter_us"] = 1e3 * _median_ms(lambda: dense.easy_edge_keep_table(
            g.edge_index, g.edge_type, h, t, r, g.num_nodes, g.num_relations), max(args.steps, 20))
    # the captures get a model of their own with the same weights: an eager step leaves the model holding its autograd graph
    # (EntityNBFNet.query), whose gradient accumulators belong to the default stream, and a capture must not reach them
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    del opt, model
    model = models.Ultra(**synthetic.default_model_cfg()).to(dev).train()
    model.load_state_dict(state)

    opt = train.make_adamw(model, lr=5e-4, capturable=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    first = pretrain.PretrainTrainer(model, graphs[:1], opt, bs, neg, 1.0, warmup=args.warmup)
    torch.cuda.synchronize()
    out["peak_gb_one"] = torch.cuda.max_memory_allocated(dev) / 1e9
    del first
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    trainer = pretrain.PretrainTrainer(model, graphs, opt, bs, neg, 1.0, warmup=args.warmup)
    for gid, (name, b) in enumerate(zip(args.graphs, batches)):
        for _ in range(args.warmup):
            trainer.step(gid, b)
        out["graphs"][name]["captured_ms"] = _median_ms(lambda: trainer.step(gid, b), args.steps)
        _log("%s captured %.2f ms" % (name, out["graphs"][name]["captured_ms"]))
    torch.cuda.synchronize()
    out["peak_gb_all"] = torch.cuda.max_memory_allocated(dev) / 1e9

    loader, _ = pretrain.batch_loader(graphs, bs)
    it = iter(loader)
    t0 = time.perf_counter()
    for _ in range(50):
        gid, pos = next(it)
    out["host_batch_source_ms"] = (time.perf_counter() - t0) * 1e3 / 50
    pos = pos.to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        tasks.negative_sampling(graphs[gid], pos, neg, strict=True)
    out["host_sampler_ms"] = (time.perf_counter() - t0) * 1e3 / 20
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
