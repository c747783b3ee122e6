"""Timing of the path explanations (Ultra.visualize) at FB15k237's shape on one GPU.

    python tools/explain_bench.py [--triples 20] [--warmup 3] [--reps 20] [--num-beam 10]
    python tools/explain_bench.py --batch 1,4,10,16 [--reps 20] [--num-beam 10]

Reports, as one JSON line:
  visualize_ms     per-triple Ultra.visualize wall time (host clock around a device synchronise, after warm-up): relation
                   model, six layers forward + edge-gradient backward, the six beam-search launches, the backtracking
  beam_hip_ms      the six beam-search launches of one triple (explain.beam_search_distance) by device events
  beam_torch_ms    the same semantics as plain torch on the GPU (the restatement of tests/test_explain_cpu.py), same inputs,
                   timed in the same process, alternating with the HIP runs
  beam_bytes       bytes a layer must move at least: CSR (row pointers, source / type / edge id per slot), the edge gradients,
                   the gathered beams (num_edge x K fp32) and the outputs (N x K x (4 + 32) bytes); beam_gbps = those bytes of
                   six layers over beam_hip_ms; roof = beam_gbps / 8 TB/s
--batch S[,S...]: one JSON line per S instead -- S triples explained by one Ultra.visualize_batch call against the loop of S
Ultra.visualize calls, in one process with the two routes alternating, by device events (recorded around the whole route,
host work and read-backs included), the median of --reps:
  batch_ms_per_triple / loop_ms_per_triple            the whole explanation, per triple
  beam_batch_ms_per_triple / beam_loop_ms_per_triple  the six beam-search layers alone (explain.beam_search_distance_batch against
                                                      S calls of explain.beam_search_distance on the same gradients)
  same_paths                                          the two routes returned the same paths and weights
Kernel times: run the same under `rocprofv3 --kernel-trace --stats -- python tools/explain_bench.py --triples 4` on its own.
The graph is synthetic (ultra_amd.synthetic: FB15k237's node, edge and relation counts), the weights are ultra_3g's.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.test_explain_cpu import restate_chain  # noqa: E402
from ultra_amd import explain, models, synthetic  # noqa: E402

HBM_BPS = 8e12


def _timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def batch_mode(model, data, kg, sizes, args):
    dev = data.edge_index.device
    k = args.num_beam
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for size in sizes:
        triples = kg.target_triples[:size].to(dev)
        host = triples.cpu()
        loop = lambda: [model.visualize(data, triples[i:i + 1]) for i in range(size)]       # noqa: E731
        batched = lambda: model.visualize_batch(data, triples, chunk=max(size, 1))           # noqa: E731
        with torch.no_grad():
            rel = model.relation_model(data.relation_graph, query=triples[:, 2])
        model.entity_model.query = rel
        grads, _ = model.entity_model.edge_grads_batch(data, triples)
        single_grads = [[g[i] for g in grads] for i in range(size)]
        beam_loop = lambda: [explain.beam_search_distance(data, single_grads[i], int(host[i, 0]), int(host[i, 1]), k)   # noqa: E731
                             for i in range(size)]
        beam_batched = lambda: explain.beam_search_distance_batch(data, grads, host[:, 0], host[:, 1], k)               # noqa: E731
        t = dict(loop=[], batch=[], beam_loop=[], beam_batch=[])
        for rep in range(args.reps + 2):
            for name, fn in (("loop", loop), ("batch", batched), ("beam_loop", beam_loop), ("beam_batch", beam_batched)):
                ms, out = _timed(fn, ev)
                if rep >= 2:
                    t[name].append(ms)
                if name == "loop":
                    want = out
                elif name == "batch":
                    same = [(list(p), list(w)) for p, w in out] == [(list(p), list(w)) for p, w in want]
        med = {name: statistics.median(v) for name, v in t.items()}
        print(json.dumps(dict(tool="explain_bench", mode="batch", batch=size, num_node=data.num_nodes, num_edge=data.num_edges,
                              num_beam=k, reps=args.reps,
                              batch_ms_per_triple=round(med["batch"] / size, 3), loop_ms_per_triple=round(med["loop"] / size, 3),
                              speedup=round(med["loop"] / med["batch"], 2),
                              beam_batch_ms_per_triple=round(med["beam_batch"] / size, 4),
                              beam_loop_ms_per_triple=round(med["beam_loop"] / size, 4),
                              beam_speedup=round(med["beam_loop"] / med["beam_batch"], 2), same_paths=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", help="comma-separated batch sizes: time visualize_batch against the per-triple loop")
    ap.add_argument("--triples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num-beam", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=True)
    data = synthetic.to_device(kg, dev)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    model.entity_model.num_beam = args.num_beam
    if args.batch:
        return batch_mode(model, data, kg, [int(x) for x in args.batch.split(",")], args)
    triples = kg.target_triples[: args.warmup + args.triples].to(dev)

    # per-triple visualize
    times, npaths = [], []
    for i in range(args.warmup + args.triples):
        batch = triples[i:i + 1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths, _ = model.visualize(data, batch)
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
            npaths.append(len(paths))

    # the six beam-search launches of one triple: HIP vs the torch restatement, alternating
    batch = triples[:1]
    h, t = int(batch[0, 0]), int(batch[0, 1])
    with torch.no_grad():
        rel = model.relation_model(data.relation_graph, query=batch[:, 2])
    model.entity_model.query = rel
    grads, _ = model.entity_model.edge_grads(data, batch)
    k = args.num_beam
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    hip, tor = [], []
    for rep in range(args.reps + 2):
        ev[0].record()
        explain.beam_search_distance(data, grads, batch[:, 0], batch[:, 1], k)
        ev[1].record()
        ev[2].record()
        restate_chain(data.edge_index, data.edge_type, data.num_nodes, grads, h, t, k)
        ev[3].record()
        torch.cuda.synchronize()
        if rep >= 2:
            hip.append(ev[0].elapsed_time(ev[1]))
            tor.append(ev[2].elapsed_time(ev[3]))
    hip_d, _ = explain.beam_search_distance(data, grads, batch[:, 0], batch[:, 1], k)
    ref_d, _ = restate_chain(data.edge_index, data.edge_type, data.num_nodes, grads, h, t, k)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(hip_d, ref_d))

    n, e = data.num_nodes, data.num_edges
    csr = explain.beam_csr(data.edge_index, data.edge_type, n)
    layer_bytes = 8 * (n + 1) + 12 * e + 4 * e + 4 * e * k + n * k * (4 + 32)
    hip_ms = statistics.median(hip)
    out = dict(tool="explain_bench", num_node=n, num_edge=e, num_beam=k, num_hub_rows=csr.num_hub,
               triples=args.triples, visualize_ms=round(statistics.median(times), 3),
               visualize_ms_min=round(min(times), 3), visualize_ms_max=round(max(times), 3),
               paths_per_triple=statistics.mean(npaths),
               beam_hip_ms=round(hip_ms, 4), beam_torch_ms=round(statistics.median(tor), 4),
               speedup_vs_torch=round(statistics.median(tor) / hip_ms, 2),
               beam_bytes_per_layer=layer_bytes, beam_gbps=round(6 * layer_bytes / (hip_ms * 1e-3) / 1e9, 1),
               roof=round(6 * layer_bytes / (hip_ms * 1e-3) / HBM_BPS, 4), hip_equals_torch=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
