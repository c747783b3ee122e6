"""Timing of RETIRING entities from a served graph (ultra_amd.predict.Predictor.remove_entities) on one GPU:

    python tools/retire_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--out profiles/retire_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries, everything
in one process.  The retired entities have the median degree of the graph and are no anchor of the queries.

  (a) retirement_to_answer  wall-clock milliseconds from "remove_entities of one entity" to the answers of the next tails() call,
                            host work included (time.perf_counter around the calls, the device synchronised before and after;
                            median of --fact-reps with min .. max):
                              live_first_ms   on a predictor whose first retirement this is: the step is captured again
                              live_next_ms    on a predictor that already holds a retirement: no capture, no plan
                              rebuild_ms      the rebuild route of tools/retract_bench.py: a new Data without the entity's edges,
                                              its relation graph, a new Predictor, its first tails() (host plan, upload, capture)
                            with the facts retracted, the rows the tombstones touch and the longest of them -- a neighbour that
                            is a hub pays DESIGN.md 18's chain over its whole row
  (b) step_ms               the captured predict step by device events, run alternately: static, static captured a second time
                            (the run-to-run spread), and with 1 and with 64 retired entities -- each twice: the step the
                            predictor runs (tombstones + the _alive selection) and the same delta under the _live-less selection
                            of DESIGN.md 18 (tombstones only, the retired ids still candidates).  The difference of the two is
                            what the mask costs; the rest is the price of the tombstones
  (c) selection_ms          each _alive entry alone against its _live twin on the same (8, N) scores and lists, captured calls:
                            with an all-zero bitmap and with 1 % of the ids retired; medians with min .. max
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

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks  # noqa: E402
from ultra_amd.data import Data  # noqa: E402
from ultra_amd.live import retired_words  # noqa: E402


def timed(fns, reps, warmup):
    """Per callable, run alternately: (median, minimum, maximum) of device-event milliseconds."""
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
    return [(statistics.median(t), min(t), max(t)) for t in times]


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


def spread(values, digits=3):
    return dict(ms=round(statistics.median(values), digits), ms_min=round(min(values), digits), ms_max=round(max(values), digits))


def median_entities(data, count, avoid):
    """`count` entities of the median degree of the graph (the ones next to the median in degree order) that are not in `avoid`."""
    deg = torch.bincount(data.edge_index.flatten(), minlength=int(data.num_nodes))
    order = torch.argsort(deg, stable=True)
    order = order[deg[order] > 0]
    order = order[~torch.isin(order, avoid)]
    mid = len(order) // 2
    lo = max(0, mid - count // 2)
    return order[lo:lo + count].contiguous(), deg


def selection_case(n, bs, k, reps, warmup, dev):
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(bs, n, generator=g).to(dev)
    n_live = torch.tensor([n], dtype=torch.long, device=dev)
    rows = [torch.unique(torch.randint(0, n, (64,), generator=g)) for _ in range(bs)]
    pos = torch.stack([row[0] for row in rows]).to(dev)
    ptr = torch.tensor([0] + [len(row) for row in rows]).cumsum(0).to(dev)
    index = torch.cat(rows)
    gone = torch.randperm(n, generator=g)[:max(1, n // 100)]
    gone = gone[~torch.isin(gone, index)]           # (the known ids and the positives are alive)
    index = index.to(dev)
    masks = {"zero": (torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.long, device=dev)),
             "percent": (retired_words(gone, n).to(dev), torch.tensor([len(gone)], dtype=torch.long, device=dev))}
    threshold = 1.5                              # (about 7 % of a standard normal row)
    lib = _lib.lib
    ids = torch.empty(bs, k, dtype=torch.long, device=dev)
    top = torch.empty(bs, k, dtype=torch.float32, device=dev)
    count = torch.empty(bs, dtype=torch.long, device=dev)
    ws = torch.empty(max(1, lib.ultra_filtered_topk_workspace(bs, n, k) // 8), dtype=torch.long, device=dev)
    a_ptr = torch.zeros(bs + 1, dtype=torch.long, device=dev)
    a_ids = torch.empty(bs * n, dtype=torch.long, device=dev)
    a_scores = torch.empty(bs * n, dtype=torch.float32, device=dev)
    a_size = torch.empty(bs, dtype=torch.long, device=dev)
    a_ws = torch.empty(lib.ultra_filtered_above_workspace(bs, n) // 8, dtype=torch.long, device=dev)
    rank, neg = torch.empty(bs, dtype=torch.long, device=dev), torch.empty(bs, dtype=torch.long, device=dev)
    args = {"topk": (pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, n, k, ids.data_ptr(), top.data_ptr(), count.data_ptr(),
                     ws.data_ptr(), ws.numel() * 8),
            "above": (pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, n, threshold, a_ptr.data_ptr(), a_ids.data_ptr(),
                      a_scores.data_ptr(), a_ids.numel(), a_size.data_ptr(), a_ws.data_ptr(), a_ws.numel() * 8),
            "rank": (pred.data_ptr(), pos.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, n, rank.data_ptr(), neg.data_ptr())}
    live = n_live.data_ptr()
    calls = {}
    for name, a in args.items():
        calls[name + "_live"] = lambda a=a, name=name: _lib.check(
            getattr(lib, "ultra_filtered_%s_live" % name)(*a, live, _lib.stream_of(dev)))
        for mask, (words, total) in masks.items():
            calls["%s_alive_%s" % (name, mask)] = lambda a=a, name=name, words=words, total=total: _lib.check(
                getattr(lib, "ultra_filtered_%s_alive" % name)(*a, live, words.data_ptr(), total.data_ptr(), _lib.stream_of(dev)))
    stats = timed([graphed(fn) for fn in calls.values()], reps, warmup)
    out = dict(N=n, k=k, threshold=threshold, retired_percent=len(gone))
    for name, (med, low, high) in zip(calls, stats):
        out[name] = dict(ms=round(med, 4), ms_min=round(low, 4), ms_max=round(high, 4))
    return out


def shape_case(name, k, bs, reps, warmup, fact_reps, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    n = int(data.num_nodes)
    out = dict(tool="retire_bench", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k)
    victims, deg = median_entities(data, 64 + 2 * fact_reps, h)
    in_degree = torch.bincount(data.edge_index[0], minlength=n)

    # (a) from a retirement to the first answers without the entity: the three routes, in turn, in every repetition
    live_first, live_next, rebuild, cases = [], [], [], []
    for rep in range(fact_reps):
        first, second = victims[64 + 2 * rep:64 + 2 * rep + 1], victims[64 + 2 * rep + 1:64 + 2 * rep + 2]
        live = predict.Predictor(model, data, k=k, batch_size=bs)
        live.tails(h, r)                                           # serving: plan and capture exist
        took = []
        live_first.append(wall_ms(lambda: (took.append(live.remove_entities(first)), live.tails(h, r))))
        touched = live.delta.rows[:int(live.delta.count)].long()
        cases.append(dict(entity=int(first), degree=int(deg[first]), facts=int(took[0]), touched_rows=len(touched),
                          longest_touched_row=int(in_degree[touched].max())))
        live_next.append(wall_ms(lambda: (live.remove_entities(second), live.tails(h, r))))
        got = live.tails(h, r)[0]
        assert live.num_retired == 2 and not bool(torch.isin(got, live.retired_entities).any())
        live.close()

        def rebuilt():
            keep = ~((data.edge_index == first).any(dim=0))
            fresh = Data(edge_index=data.edge_index[:, keep], edge_type=data.edge_type[keep], num_nodes=data.num_nodes,
                         num_relations=data.num_relations)
            tasks.build_relation_graph(fresh)
            served = predict.Predictor(model, fresh, k=k, batch_size=bs)
            served.tails(h, r)
            served.close()
        rebuild.append(wall_ms(rebuilt))
        rspmm.clear_plan_cache()
    med = statistics.median
    out["retirement_to_answer"] = dict(entities=1, reps=fact_reps, live_first=spread(live_first), live_next=spread(live_next),
                                       rebuild=spread(rebuild), rebuild_over_live_next=round(med(rebuild) / med(live_next), 1),
                                       rebuild_over_live_first=round(med(rebuild) / med(live_first), 1), cases=cases)

    # (b) the steady-state step: what the tombstones cost and what the mask costs on top
    holders, steps = [], {}
    steps["static"] = predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16)
    steps["static_again"] = predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16)
    lists = {"static": predict.known_answers(data, h, r, "tail")}
    lists["static_again"] = lists["static"]
    for count in (1, 64):
        live = predict.Predictor(model, data, k=k, batch_size=bs, delta_capacity=8192)
        facts = int(live.remove_entities(victims[:count]).sum())
        assert live.delta.num_removed > 0 and live.num_retired == count
        holders.append(live)
        known = predict.known_answers(live.filter_graph, h, r, "tail")
        for key, retired in (("retired_%d" % count, live._live.retired_operand), ("tombstones_%d" % count, None)):
            steps[key] = predict._GraphedPredictStep(model, live.data, bs, k, "tail", 1 << 16, delta=live.delta, retired=retired)
            lists[key] = known
        out["retired_%d" % count] = dict(facts=facts, tombstone_keys=live.delta.num_removed, touched_rows=int(live.delta.count),
                                         longest_touched_row=int(in_degree[live.delta.rows[:int(live.delta.count)].long()].max()))
    for key, step in steps.items():
        step.load_index(lists[key][1].contiguous())
    ptrs = {key: lists[key][0].contiguous() for key in steps}
    stats = timed([lambda s=step, p=ptrs[key]: s(h, r, p) for key, step in steps.items()], reps, warmup)
    out["step_ms"] = {key: dict(ms=round(s[0], 4), ms_min=round(s[1], 4), ms_max=round(s[2], 4)) for key, s in zip(steps, stats)}
    by = dict(zip(steps, stats))
    out["static_spread_ms"] = round(abs(by["static"][0] - by["static_again"][0]), 4)
    out["mask_ms"] = {str(c): round(by["retired_%d" % c][0] - by["tombstones_%d" % c][0], 4) for c in (1, 64)}
    out["tombstones_ms"] = {str(c): round(by["tombstones_%d" % c][0] - by["static"][0], 4) for c in (1, 64)}
    for count, live in zip((1, 64), holders):     # (the masked step returns no retired id; the unmasked one may)
        got = steps["retired_%d" % count](h, r, ptrs["retired_%d" % count])[0]
        torch.cuda.synchronize()
        assert not bool(torch.isin(got, live.retired_entities).any())
    for step in steps.values():
        step.release()
    for live in holders:
        live.close()

    # (c) the selection calls alone
    out["selection_ms"] = selection_case(n, bs, k, reps, warmup, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retire_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/retire_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
