"""Timing and peak memory of RotatE message passing at FB15k237's shape on one GPU: the rspmm engine against the unfused route.

    python tools/rotate_bench.py [--batch 8] [--warmup 3] [--reps 20] [--timeout 300] [--only NAME]

Configurations (each in a child process of its own under its own time limit, so an out-of-memory unfused run ends that
child only; a child that ends on a signal or its time limit ends the whole run -- nothing more is started on the GPU):
  layer_rotate_fused      one GeneralizedRelationalConv(64, 64, "rotate", "sum"), layers.FUSED_ROTATE = True  (the engine)
  layer_rotate_unfused    the same layer, FUSED_ROTATE = False: index_select / cat / scatter_add_ over (batch, |E|, d) tensors
  layer_distmult_general  the same layer with DistMult messages on the SAME general-walk kernel (reference-order plan, boundary
                          as a tensor, rspmm.tuning_scope(general_walk=1)): it gathers the same bytes, so rotate / distmult is
                          the price of the complex product and the lane exchange
  net_rotate_fused / net_rotate_unfused    a six-layer EntityNBFNet (sum, 64-d) with rotate messages, batch of 1 + 32 candidates
each as `forward` (no_grad) and `forward_backward` (the sum of the output, back to parameters and inputs).
Per configuration, one JSON line: milliseconds by device events (median of --reps after --warmup) and
torch.cuda.max_memory_allocated above what was allocated before the timed runs (plans and operands excluded).
The last line gathers them and the ratios.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/rotate_bench.py
--only layer_rotate_fused` in a run of its own.  The graph is synthetic (ultra_amd.synthetic: FB15k237's node, edge and relation
counts), the weights are seeded random.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("layer_rotate_fused", "layer_rotate_unfused", "layer_distmult_general", "net_rotate_fused", "net_rotate_unfused")


def child(name, batch, warmup, reps):
    import contextlib

    import torch

    from ultra_amd import layers, models, rspmm, synthetic

    dev = torch.device("cuda:0")
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=False)
    data = synthetic.to_device(kg, dev)
    n, r = data.num_nodes, data.num_relations
    layers.FUSED_ROTATE = not name.endswith("_unfused")
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(6)
    scope = contextlib.nullcontext()
    if name.startswith("layer_"):
        message = "distmult" if "distmult" in name else "rotate"
        layer = layers.GeneralizedRelationalConv(64, 64, r, 64, message, "sum", True, "relu").to(dev)
        x, bnd = (torch.randn(batch, n, 64, generator=g).to(dev) for _ in range(2))
        query = torch.randn(batch, 64, generator=g).to(dev)
        if message == "distmult":
            layers.FUSED_SPARSE_LAYER = False
            scope = rspmm.tuning_scope(general_walk=1)

        def run(grad):
            xx = x.clone().requires_grad_() if grad else x
            out = layer(xx, query, bnd, data.edge_index, data.edge_type, (n, n))
            if grad:
                out.sum().backward()
        params = layer.parameters()
    else:
        net = models.EntityNBFNet(64, [64] * 6, 1, message_func="rotate", aggregate_func="sum", short_cut=True,
                                  layer_norm=True).to(dev).eval()
        rel = torch.randn(batch, r, 64, generator=g).to(dev)
        pos = kg.target_triples[:batch]
        tails = torch.randint(0, n, (batch, 33), generator=g)
        tails[:, 0] = pos[:, 1]
        cand = torch.stack([pos[:, :1].expand(-1, 33), tails, pos[:, 2:].expand(-1, 33)], dim=-1).to(dev)

        def run(grad):
            rr = rel.clone().requires_grad_() if grad else rel
            out = net(data, rr, cand)
            if grad:
                out.sum().backward()
        params = net.parameters()
    params = list(params)

    result = {"config": name, "batch": batch, "num_node": n, "num_edge": int(data.edge_index.shape[1]), "fused_rotate": layers.FUSED_ROTATE}
    with scope:
        for mode, grad in (("forward", False), ("forward_backward", True)):
            ctx = torch.enable_grad() if grad else torch.no_grad()
            with ctx:
                for _ in range(warmup):
                    run(grad)
                    for p in params:
                        p.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                times = []
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run(grad)
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b))
                    for p in params:
                        p.grad = None
                result[mode + "_ms"] = round(statistics.median(times), 4)
                result[mode + "_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per configuration")
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.batch, args.warmup, args.reps)
    results = {}
    for name in CONFIGS:
        if args.only and name != args.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--batch", str(args.batch), "--warmup", str(args.warmup),
               "--reps", str(args.reps)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"config": name, "error": "time limit of %g s" % args.timeout}), flush=True)
            print("a configuration hit its time limit: nothing more is started", file=sys.stderr)
            return 1
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
        if done.returncode == 0 and lines:
            results[name] = json.loads(lines[-1])
            print(lines[-1], flush=True)
            continue
        tail = (done.stderr or "").strip().splitlines()[-1:] or [""]
        print(json.dumps({"config": name, "error": "exit %d: %s" % (done.returncode, tail[0][:200])}), flush=True)
        if done.returncode < 0 or "out of memory" not in (done.stderr or "").lower():
            print("a configuration ended abnormally: nothing more is started", file=sys.stderr)
            return 1
    summary = {"summary": "rotate_bench", "batch": args.batch}

    def ratio(a, b, key):
        if a in results and b in results and results[a].get(key):
            summary["%s / %s %s" % (b, a, key)] = round(results[b][key] / results[a][key], 2)
    for key in ("forward_ms", "forward_backward_ms", "forward_peak_mb", "forward_backward_peak_mb"):
        ratio("layer_rotate_fused", "layer_rotate_unfused", key)
        ratio("net_rotate_fused", "net_rotate_unfused", key)
    for key in ("forward_ms", "forward_backward_ms"):
        ratio("layer_distmult_general", "layer_rotate_fused", key)
    print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
