"""Timing of serving a CHANGING graph (ultra_amd.predict.Predictor.add_facts) on one GPU:

    python tools/live_graph_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--out profiles/live_graph_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries.

  (a) fact_to_answer     wall-clock milliseconds from "16 new facts" to the answers of the next tails() call, host work included
                         (time.perf_counter around the calls, the device synchronised before and after; median of --fact-reps):
                           live_first_ms    add_facts on a predictor that held no facts: the step is captured again
                           live_next_ms     add_facts on a predictor that already holds facts: no capture, no plan
                           rebuild_ms       the route without a delta: a new Data of the concatenated edge list, its relation
                                            graph, a new Predictor, its first tails() (host plan, upload, capture)
  (b) step_ms            the captured predict step by device events, run alternately: static (no delta), with a delta of 16 and
                         of 1,024 facts
  (c) delta_rows         ultra_rspmm_delta_rows alone (a captured call) with those deltas: touched rows, edges walked, bytes
                         (per edge a source row, a relation row and 8 bytes of indices, per row one output row, times the
                         batch), their share of 8 TB/s
  (d) empty_delta        the step captured with an EMPTY delta against the static step: the kernels of one replay of each,
                         counted with torch.profiler and asserted equal, and the two times
One JSON line per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, predict, rspmm, synthetic, tasks  # noqa: E402
from ultra_amd.data import Data  # noqa: E402

HBM_BPS = 8e12


def timed(fns, reps, warmup):
    """Median and minimum device-event milliseconds of every callable, run alternately."""
    times = [[] for _ in fns]
    for rep in range(warmup + reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times], [min(t) for t in times]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        keep = fn()
    g.keep = keep
    return g.replay


def random_facts(data, count, seed, dev):
    g = torch.Generator().manual_seed(seed)
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    return (torch.randint(0, n, (count,), generator=g).to(dev), torch.randint(0, direct, (count,), generator=g).to(dev),
            torch.randint(0, n, (count,), generator=g).to(dev))


def replay_kernels(step, args):
    """Names of the kernels one replay of a captured step runs, in order of their names (torch.profiler); None where the profiler
    reports no device activity."""
    from torch.profiler import ProfilerActivity, profile
    step(*args)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(*args)
        torch.cuda.synchronize()
    names = sorted(e.name for e in prof.events() if getattr(e, "device_type", None) is not None
                   and "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return names or None


def delta_rows_case(data, delta, bs, reps, warmup, dev):
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs, data.num_nodes, 64, generator=g).to(dev)
    rel = torch.randn(bs, data.num_relations, 64, generator=g).to(dev)
    rows = torch.zeros(bs, dtype=torch.long, device=dev)
    vals = torch.randn(bs, 64, generator=g).to(dev)
    out = plan.forward(rel, x, point=(rows, vals))
    call = graphed(lambda: plan.delta_rows(rel, x, out, delta, point=(rows, vals)))
    (ms,), (ms_min,) = timed([call], reps, warmup)
    touched = delta.rows[:int(delta.count)].long()
    base_degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)[touched]
    edges = int(base_degree.sum()) + 2 * len(delta)
    nbytes = bs * (edges * (256 + 256) + len(touched) * 256) + edges * 8
    return dict(facts=len(delta), touched_rows=len(touched), edges_walked=edges, longest_row=int(base_degree.max()),
                ms=round(ms, 4), ms_min=round(ms_min, 4), bytes=nbytes, gbps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                roof=round(nbytes / (ms * 1e-3) / HBM_BPS, 4))


def shape_case(name, k, bs, reps, warmup, fact_reps, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    out = dict(tool="live_graph_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]), k=k)

    # (a) from new facts to their first answers
    live_first, live_next, rebuild = [], [], []
    for rep in range(fact_reps):
        facts = random_facts(data, 32, 100 + rep, dev)
        live = predict.Predictor(model, data, k=k, batch_size=bs)
        live.tails(h, r)                                           # serving: plan and capture exist
        live_first.append(wall_ms(lambda: (live.add_facts(*(f[:16] for f in facts)), live.tails(h, r))))
        live_next.append(wall_ms(lambda: (live.add_facts(*(f[16:] for f in facts)), live.tails(h, r))))
        live.close()

        def rebuilt():
            fh, fr, ft = (f[:16] for f in facts)
            fresh = Data(edge_index=torch.cat([data.edge_index, torch.stack([torch.cat([fh, ft]), torch.cat([ft, fh])])], dim=1),
                         edge_type=torch.cat([data.edge_type, fr, fr + data.num_relations // 2]), num_nodes=data.num_nodes,
                         num_relations=data.num_relations)
            tasks.build_relation_graph(fresh)
            served = predict.Predictor(model, fresh, k=k, batch_size=bs)
            served.tails(h, r)
            served.close()
        rebuild.append(wall_ms(rebuilt))
        rspmm.clear_plan_cache()
    out["fact_to_answer"] = dict(facts=16, reps=fact_reps, live_first_ms=round(statistics.median(live_first), 3),
                                 live_next_ms=round(statistics.median(live_next), 3),
                                 rebuild_ms=round(statistics.median(rebuild), 3),
                                 rebuild_over_live_next=round(statistics.median(rebuild) / statistics.median(live_next), 1),
                                 rebuild_over_live_first=round(statistics.median(rebuild) / statistics.median(live_first), 1))

    # (b) the steady-state step, (d) the empty delta
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    deltas = {}
    for count in (0, 16, 1024):
        deltas[count] = rspmm.GraphDelta(data, 1024)
        if count:
            deltas[count].add(*random_facts(data, count, 7, dev))
    steps = {"static": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16)}
    for count, delta in deltas.items():
        steps[count] = predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16, delta=delta)
    for step in steps.values():
        step.load_index(index)
    order = ["static", 0, 16, 1024]
    med, low = timed([lambda s=steps[key]: s(h, r, ptr) for key in order], reps, warmup)
    out["step_ms"] = {str(key): round(m, 4) for key, m in zip(order, med)}
    out["step_ms_min"] = {str(key): round(m, 4) for key, m in zip(order, low)}
    out["step_over_static"] = {str(key): round(m / med[0], 4) for key, m in zip(order, med)}
    out["relation_graph_kept"] = {str(c): bool(d.relation_graph is data.relation_graph) for c, d in deltas.items()}
    try:
        static_kernels, empty_kernels = replay_kernels(steps["static"], (h, r, ptr)), replay_kernels(steps[0], (h, r, ptr))
        live_kernels = replay_kernels(steps[16], (h, r, ptr))
    except Exception as exc:      # (no profiler on this build: the count is not taken, and the line says so)
        static_kernels = empty_kernels = live_kernels = None
        out["kernel_count_error"] = repr(exc)
    if static_kernels is not None and empty_kernels is not None:
        assert static_kernels == empty_kernels, "the step with an empty delta does not run the static step's kernels"
    out["empty_delta"] = dict(static_kernels=None if static_kernels is None else len(static_kernels),
                              empty_delta_kernels=None if empty_kernels is None else len(empty_kernels),
                              live16_kernels=None if live_kernels is None else len(live_kernels),
                              static_ms=round(med[0], 4), empty_delta_ms=round(med[1], 4))

    # (c) the delta kernel alone
    out["delta_rows"] = [delta_rows_case(data, deltas[count], bs, reps, warmup, dev) for count in (16, 1024)]
    for step in steps.values():
        step.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_graph_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/live_graph_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
