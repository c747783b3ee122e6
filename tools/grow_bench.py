"""Timing of serving a GROWING graph (ultra_amd.predict.Predictor.add_entities) on one GPU:

    python tools/grow_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--out profiles/grow_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries.  Every
route is measured in the same run.

  (a) entity_to_answer   wall-clock milliseconds from "one new entity and four facts about it" to the answers of the next
                         tails() call, host work included (time.perf_counter around the calls, the device synchronised before
                         and after; median of --fact-reps), on a Predictor(entity_capacity=256):
                           live_first_ms    the predictor held no facts: the step is captured again (the delta's route)
                           live_next_ms     the predictor already holds facts: no capture, no plan
                           rebuild_ms       the route without a reserve: a new Data of N + 1 nodes and the concatenated edge
                                            list, its relation graph, a new Predictor, its first tails() (plan, upload, capture)
  (b) step_ms            the captured predict step by device events, run alternately, no entity added: entity_capacity 0 (the
                         static step, captured TWICE -- the difference of the two and their quartiles are the run-to-run spread
                         the reserve's cost is read against), 256 and 4096
  (c) selection_ms       the three _live calls against their parents on the same (batch, N + 256) scores, each a captured call:
                         the parents over all slots, the twins with N live
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
from ultra_amd.live import with_slots  # noqa: E402
from ultra_amd.data import Data  # noqa: E402


def timed(fns, reps, warmup):
    """Per callable, run alternately: (median, minimum, lower quartile, upper quartile) of device-event milliseconds."""
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
    out = []
    for t in times:
        t = sorted(t)
        out.append((statistics.median(t), t[0], t[len(t) // 4], t[(3 * len(t)) // 4]))
    return out


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


def facts_about(new_id, data, seed, dev):
    """Four facts about the entity `new_id`: two with it as the head, two as the tail, the other ends drawn among the old ids."""
    g = torch.Generator().manual_seed(seed)
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    other = torch.randint(0, n, (4,), generator=g)
    me = torch.full((4,), new_id)
    h, t = torch.cat([me[:2], other[2:]]), torch.cat([other[:2], me[2:]])
    return h.to(dev), torch.randint(0, direct, (4,), generator=g).to(dev), t.to(dev)


def selection_case(n, reserve, bs, k, reps, warmup, dev):
    slots = n + reserve
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(bs, slots, generator=g).to(dev)
    n_live = torch.tensor([n], dtype=torch.long, device=dev)
    rows = [torch.unique(torch.randint(0, n, (64,), generator=g)) for _ in range(bs)]
    pos = torch.stack([row[0] for row in rows]).to(dev)
    ptr = torch.tensor([0] + [len(row) for row in rows]).cumsum(0).to(dev)
    index = torch.cat(rows).to(dev)
    threshold = 1.5                              # (about 7 % of a standard normal row)
    lib = _lib.lib
    ids = torch.empty(bs, k, dtype=torch.long, device=dev)
    top = torch.empty(bs, k, dtype=torch.float32, device=dev)
    count = torch.empty(bs, dtype=torch.long, device=dev)
    ws = torch.empty(max(1, lib.ultra_filtered_topk_workspace(bs, slots, k) // 8), dtype=torch.long, device=dev)
    a_ptr = torch.zeros(bs + 1, dtype=torch.long, device=dev)
    a_ids = torch.empty(bs * slots, dtype=torch.long, device=dev)
    a_scores = torch.empty(bs * slots, dtype=torch.float32, device=dev)
    a_size = torch.empty(bs, dtype=torch.long, device=dev)
    a_ws = torch.empty(lib.ultra_filtered_above_workspace(bs, slots) // 8, dtype=torch.long, device=dev)
    rank, neg = torch.empty(bs, dtype=torch.long, device=dev), torch.empty(bs, dtype=torch.long, device=dev)
    topk_args = (pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, slots, k, ids.data_ptr(), top.data_ptr(), count.data_ptr(),
                 ws.data_ptr(), ws.numel() * 8)
    above_args = (pred.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, slots, threshold, a_ptr.data_ptr(), a_ids.data_ptr(),
                  a_scores.data_ptr(), a_ids.numel(), a_size.data_ptr(), a_ws.data_ptr(), a_ws.numel() * 8)
    rank_args = (pred.data_ptr(), pos.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs, slots, rank.data_ptr(), neg.data_ptr())
    live = n_live.data_ptr()
    calls = {
        "topk": lambda: _lib.check(lib.ultra_filtered_topk(*topk_args, _lib.stream_of(dev))),
        "topk_live": lambda: _lib.check(lib.ultra_filtered_topk_live(*topk_args, live, _lib.stream_of(dev))),
        "above": lambda: _lib.check(lib.ultra_filtered_above(*above_args, _lib.stream_of(dev))),
        "above_live": lambda: _lib.check(lib.ultra_filtered_above_live(*above_args, live, _lib.stream_of(dev))),
        "rank": lambda: _lib.check(lib.ultra_filtered_rank(*rank_args, _lib.stream_of(dev))),
        "rank_live": lambda: _lib.check(lib.ultra_filtered_rank_live(*rank_args, live, _lib.stream_of(dev))),
    }
    replays = [graphed(fn) for fn in calls.values()]
    stats = timed(replays, reps, warmup)
    out = dict(slots=slots, live=n, k=k, threshold=threshold)
    for name, (med, low, q1, q3) in zip(calls, stats):
        out[name] = dict(ms=round(med, 4), ms_min=round(low, 4), q1=round(q1, 4), q3=round(q3, 4))
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
    out = dict(tool="grow_bench", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k)

    # (a) from a new entity and its facts to the first answers
    live_first, live_next, rebuild = [], [], []
    for rep in range(fact_reps):
        live = predict.Predictor(model, data, k=k, batch_size=bs, entity_capacity=256)
        live.tails(h, r)                                           # serving: plan and capture exist

        def arrive(seed):
            (new_id,) = live.add_entities(1).tolist()
            live.add_facts(*facts_about(new_id, data, seed, dev))
            live.tails(h, r)
        live_first.append(wall_ms(lambda: arrive(100 + rep)))
        live_next.append(wall_ms(lambda: arrive(200 + rep)))
        assert live.num_entities == n + 2 and len(live.delta) == 8 and live.num_slots == n + 256
        live.close()

        def rebuilt():
            fh, fr, ft = facts_about(n, data, 100 + rep, dev)
            fresh = Data(edge_index=torch.cat([data.edge_index, torch.stack([torch.cat([fh, ft]), torch.cat([ft, fh])])], dim=1),
                         edge_type=torch.cat([data.edge_type, fr, fr + data.num_relations // 2]), num_nodes=n + 1,
                         num_relations=data.num_relations)
            tasks.build_relation_graph(fresh)
            served = predict.Predictor(model, fresh, k=k, batch_size=bs)
            served.tails(h, r)
            served.close()
        rebuild.append(wall_ms(rebuilt))
        rspmm.clear_plan_cache()
    out["entity_to_answer"] = dict(entities=1, facts=4, reps=fact_reps, live_first_ms=round(statistics.median(live_first), 3),
                                   live_next_ms=round(statistics.median(live_next), 3),
                                   rebuild_ms=round(statistics.median(rebuild), 3),
                                   rebuild_over_live_next=round(statistics.median(rebuild) / statistics.median(live_next), 1),
                                   rebuild_over_live_first=round(statistics.median(rebuild) / statistics.median(live_first), 1))

    # (b) what the reserve costs a step that uses none of it
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    steps, keep = {}, []
    for key, reserve in (("0", 0), ("0_again", 0), ("256", 256), ("4096", 4096)):
        served, n_live = data, None
        if reserve:
            served = with_slots(data, n + reserve, relation_graph=True)
            n_live = torch.tensor([n], dtype=torch.long, device=dev)
        keep.append((served, n_live))
        steps[key] = predict._GraphedPredictStep(model, served, bs, k, "tail", 1 << 16, n_live=n_live)
        steps[key].load_index(index)
    stats = timed([lambda s=step: s(h, r, ptr) for step in steps.values()], reps, warmup)
    out["step_ms"] = {key: round(s[0], 4) for key, s in zip(steps, stats)}
    out["step_ms_min"] = {key: round(s[1], 4) for key, s in zip(steps, stats)}
    out["step_ms_quartiles"] = {key: [round(s[2], 4), round(s[3], 4)] for key, s in zip(steps, stats)}
    out["step_over_static"] = {key: round(s[0] / stats[0][0], 4) for key, s in zip(steps, stats)}
    out["static_spread_ms"] = round(abs(stats[0][0] - stats[1][0]), 4)
    want = steps["0"](h, r, ptr)
    want = [t.clone() for t in want]
    for key in ("256", "4096"):       # (the reserve changes no answer: the same ids, the same bits)
        got = steps[key](h, r, ptr)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), key
    for step in steps.values():
        step.release()

    # (c) the selection calls alone
    out["selection_ms"] = selection_case(n, 256, bs, k, reps, warmup, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/grow_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
