"""Timing of WHAT-IF queries (ultra_amd.predict.Predictor.tails(assuming=)) on one GPU:

    python tools/assume_bench.py [--reps 30] [--warmup 5] [--fact-reps 5] [--shapes fb15k237,yago310] [--out profiles/assume_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries; every
query assumes ONE fact of its own.

  (a) hypothesis_to_answer  wall-clock milliseconds from "eight queries, one hypothesis each" to their answers, host work included
                            (time.perf_counter, the device synchronised before and after; median of --fact-reps), in the same run:
                              assume_ms       one tails(h, r, assuming=[...]) call: overlay refill, one replay
                              state_ms        the route without the argument, per query add_facts -> tails -> remove_facts on
                                              the same predictor (batch 8: a single query is padded), the eight in turn
                              state_bs1_ms    ... on a predictor of batch_size 1
  (b) step_ms               the captured steps by device events, run alternately: static (no delta), the add-only live step (a
                            delta of 8 stated facts), and the what-if step with its overlay filled for two cases -- hypotheses
                            between the rows of the fewest edges (`off_hubs`), and every query's hypothesis at the graph's
                            longest row (`longest_row`: the hub is live in all eight slices) -- plus one query alone at the
                            longest row (`longest_row_one`: one workgroup walks the hub)
  (c) refill_ms             AssumedFacts.fill on the host for those cases (wall clock, synchronised; median of --reps)
  (d) kernel_ms             ultra_rspmm_edit_rows_owned alone (a captured call) for `off_hubs` and `longest_row_one`, against the
                            same edges with every owner rewritten to -1 -- every (touched row, slice) is then walked and written,
                            what the launch would do without the early-out (a row's one delta edge more per walk)
One JSON line per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from live_graph_bench import graphed, timed, wall_ms  # noqa: E402
from ultra_amd import models, predict, rspmm, synthetic, tasks  # noqa: E402


def cases(data, bs, dev):
    """{name: one (1, 3) fact per query, or None} -- see the module docstring."""
    degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)
    short = degree.argsort()[:2 * bs].tolist()
    hub = int(degree.argmax())
    fact = lambda h, r, t: torch.tensor([[h, r, t]], device=dev)
    return {
        "off_hubs": [fact(short[i], 0, short[bs + i]) for i in range(bs)],
        "longest_row": [fact(hub, 1, short[i]) for i in range(bs)],
        "longest_row_one": [fact(hub, 1, short[0])] + [None] * (bs - 1),
    }, hub, int(degree[hub])


def kernel_case(data, overlay, bs, reps, warmup, dev):
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs, data.num_nodes, 64, generator=g).to(dev)
    rel = torch.randn(bs, data.num_relations, 64, generator=g).to(dev)
    rows = torch.zeros(bs, dtype=torch.long, device=dev)
    vals = torch.randn(bs, 64, generator=g).to(dev)
    out = plan.forward(rel, x, point=(rows, vals))
    call = graphed(lambda: plan.edit_rows_owned(rel, x, out, overlay, point=(rows, vals)))
    owners = overlay.owner.clone()
    (early,), (early_min,) = timed([call], reps, warmup)
    overlay.owner.fill_(-1)                      # every slice walks every touched row: the launch without the early-out
    (every,), (every_min,) = timed([call], reps, warmup)
    overlay.owner.copy_(owners)
    return dict(touched_rows=int(overlay.count), edges=overlay.num_edges, early_out_ms=round(early, 4),
                early_out_ms_min=round(early_min, 4), every_slice_ms=round(every, 4), every_slice_ms_min=round(every_min, 4))


def shape_case(name, k, bs, reps, warmup, fact_reps, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    fills, hub, hub_len = cases(data, bs, dev)
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    out = dict(tool="assume_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]), k=k,
               seg_len=plan.info()["seg_len"], longest_row=hub_len)
    med = statistics.median

    # (a) one hypothesis per query to its answers: the what-if call against stating and retracting
    live = predict.Predictor(model, data, k=k, batch_size=bs)
    one = predict.Predictor(model, data, k=k, batch_size=1)
    facts = fills["off_hubs"]
    live.tails(h, r), live.tails(h, r, assuming=facts), one.tails(h[:1], r[:1])       # serving: plans and captures exist

    def stated(served):
        for i in range(bs):
            f = facts[i][0]
            served.add_facts(f[0:1], f[1:2], f[2:3])
            served.tails(h[i:i + 1], r[i:i + 1])
            served.remove_facts(f[0:1], f[1:2], f[2:3])

    stated(live), stated(one)       # (the live step with a delta is captured once, outside the timing)
    assume, state, state_one = [], [], []
    for _ in range(fact_reps):
        assume.append(wall_ms(lambda: live.tails(h, r, assuming=facts)))
        state.append(wall_ms(lambda: stated(live)))
        state_one.append(wall_ms(lambda: stated(one)))
    out["hypothesis_to_answer"] = dict(queries=bs, reps=fact_reps, assume_ms=round(med(assume), 3), state_ms=round(med(state), 3),
                                       state_bs1_ms=round(med(state_one), 3), state_over_assume=round(med(state) / med(assume), 1),
                                       state_bs1_over_assume=round(med(state_one) / med(assume), 1))
    live.close(), one.close()

    # (b) the captured steps, alternately
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    added = rspmm.GraphDelta(data, 256)
    added.add(*(torch.cat([f[:, i] for f in fills["off_hubs"]]) for i in range(3)))
    empty = rspmm.GraphDelta(data, 256)
    steps = {"static": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16),
             "added8": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16, delta=added)}
    for key in fills:
        steps[key] = predict._GraphedAssumeStep(model, data, bs, k, "tail", 1 << 16, 8, delta=empty)
        steps[key].overlay.fill(fills[key])
    for step in steps.values():
        step.load_index(index)
    order = list(steps)
    med_ms, low = timed([lambda s=steps[key]: s(h, r, ptr) for key in order], reps, warmup)
    out["step_ms"] = {key: round(m, 4) for key, m in zip(order, med_ms)}
    out["step_ms_min"] = {key: round(m, 4) for key, m in zip(order, low)}
    out["step_over_static"] = {key: round(m / med_ms[0], 4) for key, m in zip(order, med_ms)}

    # (c) the refill on the host
    overlay = steps["off_hubs"].overlay
    refill = {}
    for key, fill in fills.items():
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            overlay.fill(fill)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        refill[key] = round(med(times), 4)
    out["refill_ms"] = refill

    # (d) the kernel alone, with and without the early-out
    out["kernel_ms"] = {}
    for key in ("off_hubs", "longest_row_one", "longest_row"):
        overlay.fill(fills[key])
        out["kernel_ms"][key] = kernel_case(data, overlay, bs, reps, warmup, dev)
    for step in steps.values():
        step.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assume_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/assume_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
