"""Timing of verifying stated facts on a CHANGING graph (Predictor.add_facts -> verify_tails) on one GPU:

    python tools/verify_live_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--only a,b,c]
                                      [--out profiles/verify_live_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8.

  (a) fact_to_verdict    wall-clock milliseconds from add_facts of ONE fact to the result of verify_tails of that fact, host work
                         included (time.perf_counter, the device synchronised before and after; median, min and max of --fact-reps):
                           first_ms     the first edit of a predictor that has verified before: the verify step is captured again
                           next_ms      on a predictor that already holds edits: no plan, no capture
                           compact_ms   add_facts, predictor.compact(), verify_tails: the route that folds the edits in first
                                        (a host plan of the materialised graph, its relation graph, a new capture)
                         Uses the public Predictor interface only, so `--only a` runs on an older checkout too: there next_ms is
                         that checkout's add_facts -> verify_tails, whatever route it takes.
  (b) step_ms            the captured verify step by device events, run alternately: static (no delta), with 16 facts held, with
                         16 retractions held
  (c) edit_rows_samples  ultra_rspmm_edit_rows_samples alone (a captured call) against ultra_rspmm_edit_rows on the same delta (16
                         facts and 16 retractions, a dense boundary): touched rows, edges walked, bytes (per edge a source row, a
                         relation row and 8 bytes of indices, per row a boundary row and an output row, times the batch; per
                         group its slice's keys), their share of 8 TB/s
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


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def fact_to_verdict(model, data, bs, fact_reps, dev):
    h, t, r = data.target_triples[:bs].unbind(-1)
    first, nxt, compact = [], [], []
    kept = None
    for rep in range(fact_reps):
        fh, fr, ft = random_facts(data, 3, 100 + rep, dev)
        live = predict.Predictor(model, data, batch_size=bs)
        live.verify_tails(h, r, t)                                 # serving: plan and capture exist

        def state_and_verify(i, fold=False):
            live.add_facts(fh[i:i + 1], fr[i:i + 1], ft[i:i + 1])
            if fold:
                live.compact()
            live.verify_tails(fh[i:i + 1], fr[i:i + 1], ft[i:i + 1])
        first.append(wall_ms(lambda: state_and_verify(0)))
        nxt.append(wall_ms(lambda: state_and_verify(1)))
        kept = bool(live.delta is not None and live.delta.edited)  # did the edits stay beside the plan?
        compact.append(wall_ms(lambda: state_and_verify(2, fold=True)))
        live.close()
        rspmm.clear_plan_cache()
    return dict(facts=1, reps=fact_reps, delta_kept=kept, first_ms=spread(first), next_ms=spread(nxt), compact_ms=spread(compact),
                compact_over_next=round(statistics.median(compact) / statistics.median(nxt), 1))


def edited_delta(data, facts, retractions, dev):
    delta = rspmm.GraphDelta(data, 1024)
    if facts:
        delta.add(*random_facts(data, facts, 7, dev))
    if retractions:
        direct = (data.edge_type < data.num_relations // 2).nonzero().flatten()
        pick = direct[torch.randperm(len(direct), generator=torch.Generator().manual_seed(9))[:retractions].to(dev)]
        delta.remove(data.edge_index[0, pick], data.edge_type[pick], data.edge_index[1, pick])
    return delta


def step_case(model, data, bs, reps, warmup, dev):
    triples = data.target_triples[:bs].contiguous()                # (h, t, r)
    ptr, index = tasks.known_answers(data, triples, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    deltas = {"static": None, "facts16": edited_delta(data, 16, 0, dev), "retractions16": edited_delta(data, 0, 16, dev)}
    steps = {key: predict._GraphedVerifyStep(model, data, bs, "tail", 1 << 16, delta=delta) for key, delta in deltas.items()}
    for step in steps.values():
        step.load_index(index)
    order = list(steps)
    med, low = timed([lambda s=steps[key]: s(triples, ptr) for key in order], reps, warmup)
    for step in steps.values():
        step.release()
    return dict(step_ms={key: round(m, 4) for key, m in zip(order, med)},
                step_ms_min={key: round(m, 4) for key, m in zip(order, low)},
                step_over_static={key: round(m / med[0], 4) for key, m in zip(order, med)})


def kernel_case(data, bs, reps, warmup, dev):
    delta = edited_delta(data, 16, 16, dev)
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs, data.num_nodes, 64, generator=g).to(dev)
    rel = torch.randn(bs, data.num_relations, 64, generator=g).to(dev)
    bnd = torch.randn(bs, data.num_nodes, 64, generator=g).to(dev)
    # every slice verifies one of the delta's own facts: its keys name a touched row
    triples = torch.stack([delta.facts[:bs, 0], delta.facts[:bs, 2], delta.facts[:bs, 1]], dim=-1).contiguous()
    keys = delta.sample_keys(triples)
    out = plan.forward(rel, x, boundary=bnd)
    calls = [graphed(lambda: plan.edit_rows(rel, x, out, delta, boundary=bnd)),
             graphed(lambda: plan.edit_rows_samples(rel, x, out, delta, keys, boundary=bnd))]
    med, low = timed(calls, reps, warmup)
    touched = delta.rows[:int(delta.count)].long()
    base_degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)[touched]
    edges = int(base_degree.sum()) + 2 * len(delta)
    nbytes = bs * (edges * (256 + 256) + len(touched) * (256 + 256)) + edges * 8
    key_bytes = bs * len(touched) * 2 * 12
    case = lambda ms, ms_min, extra: dict(ms=round(ms, 4), ms_min=round(ms_min, 4), bytes=nbytes + extra,
                                          gbps=round((nbytes + extra) / (ms * 1e-3) / 1e9, 1),
                                          roof=round((nbytes + extra) / (ms * 1e-3) / HBM_BPS, 4))
    return dict(facts=len(delta), tombstone_keys=delta.num_removed, touched_rows=len(touched), edges_walked=edges,
                longest_row=int(base_degree.max()), edit_rows=case(med[0], low[0], 0),
                edit_rows_samples=case(med[1], low[1], key_bytes), samples_over_edit_rows=round(med[1] / med[0], 4))


def shape_case(name, bs, reps, warmup, fact_reps, only, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    out = dict(tool="verify_live_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]))
    if "a" in only:
        out["fact_to_verdict"] = fact_to_verdict(model, data, bs, fact_reps, dev)
    if "b" in only:
        out.update(step_case(model, data, bs, reps, warmup, dev))
    if "c" in only:
        out["edit_rows_samples"] = kernel_case(data, bs, reps, warmup, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--tag", default=None, help="a label stored with every line (which checkout ran)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_live_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/verify_live_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        case = shape_case(name, args.batch, args.reps, args.warmup, args.fact_reps, set(args.only.split(",")), dev)
        if args.tag:
            case["tag"] = args.tag
        line = json.dumps(case)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
