"""Timing of LINK DISCOVERY (predict.Predictor.propose_tails, ultra_topk_pairs_merge) on one GPU:

    python tools/propose_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--heads 2048]
                                  [--out profiles/propose_bench.jsonl]

  (a) merge_ms     ultra_topk_pairs_merge alone against the torch route a user had -- cat of the running list and the batch,
                   one stable descending sort, a slice, three gathers -- both as captured calls on the same operands (no pads,
                   no floor: the torch route does not tell them apart), batch 8 and 64, k = k_row 10 and 256, medians with
                   min .. max.  The two routes agree: asserted.
  (b) step_ms      per replay, by device events, run alternately: the captured best step (predict step + merge) against the
                   captured `tails` step of the same shape -- the parent's step, captured twice: its run-to-run spread.
      call_ms      propose_tails over `--heads` heads (0: every entity) against tails(heads, r) + torch.sort over the (n, k)
                   result, wall time of the whole call; and the bytes of result each route keeps on the device.
One JSON line per merge shape and per graph shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, predict, synthetic, tasks  # noqa: E402


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
    return [dict(ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4)) for t in times]


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return round(1e3 * (time.perf_counter() - t0), 3), out


def merge_case(batch, k, reps, warmup, dev):
    g = torch.Generator().manual_seed(7)
    scores = torch.sort(torch.randn(batch + 1, k, generator=g), dim=1, descending=True).values.to(dev)
    ids = torch.stack([torch.sort(torch.randperm(4 * k, generator=g)[:k]).values for _ in range(batch + 1)]).to(dev)
    # a full running list (query 0) and a batch of `batch` later queries
    start = predict.merge_pairs(tuple(t.to(dev) for t in predict.empty_pairs(k)), ids[:1].contiguous(), scores[:1].contiguous(), 0)
    b_ids, b_scores = ids[1:].contiguous(), scores[1:].contiguous()
    base = torch.ones(1, dtype=torch.long, device=dev)
    queries = (1 + torch.arange(batch, device=dev)).repeat_interleave(k)
    best = tuple(t.clone() for t in start)
    out = {}

    def kernel():
        for dst, src in zip(best, start):       # (both routes start from the same list every time: two small copies more for each)
            dst.copy_(src)
        predict.merge_pairs(best, b_ids, b_scores, base)

    def torch_route():
        for dst, src in zip(best, start):
            dst.copy_(src)
        score = torch.cat([best[2], b_scores.reshape(-1)])
        order = torch.sort(score, descending=True, stable=True).indices[:k]
        out["torch"] = (torch.cat([best[0], queries])[order], torch.cat([best[1], b_ids.reshape(-1)])[order], score[order])

    def copies_alone():
        for dst, src in zip(best, start):
            dst.copy_(src)

    kernel()
    got = tuple(t.clone() for t in best)
    torch_route()
    assert all(torch.equal(a, b) for a, b in zip(got[:3], out["torch"])), "the two routes disagree"
    stats = timed([graphed(kernel), graphed(torch_route), graphed(copies_alone)], reps, warmup)
    return dict(tool="propose_bench", part="merge", batch=batch, k=k, k_row=k, keys=k + batch * k, kernel=stats[0], torch=stats[1],
                reset_copies=stats[2], torch_over_kernel=round(stats[1]["ms"] / stats[0]["ms"], 2),
                kernel_minus_copies_ms=round(stats[0]["ms"] - stats[2]["ms"], 4),
                torch_minus_copies_ms=round(stats[1]["ms"] - stats[2]["ms"], 4))


def shape_case(name, k, bs, heads, reps, warmup, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    n = int(data.num_nodes)
    out = dict(tool="propose_bench", part="step", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k)

    # (b) per replay: the best step against the tails step, captured twice
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    ptr, index = predict.known_answers(data, h, r, "tail")
    steps = {"tails": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16),
             "tails_again": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16),
             "best": predict._GraphedBestStep(model, data, bs, k, k, "tail", 1 << 16, False),
             "best_floor": predict._GraphedBestStep(model, data, bs, k, k, "tail", 1 << 16, True)}
    for step in steps.values():
        step.load_index(index.contiguous())
    for key in ("best", "best_floor"):
        steps[key].where.copy_(torch.tensor([0, bs], device=dev))
    stats = timed([lambda s=step: s(h, r, ptr.contiguous()) for step in steps.values()], reps, warmup)
    out["step_ms"] = dict(zip(steps, stats))
    out["tails_spread_ms"] = round(abs(stats[0]["ms"] - stats[1]["ms"]), 4)
    out["best_minus_tails_ms"] = round(stats[2]["ms"] - min(stats[0]["ms"], stats[1]["ms"]), 4)
    out["best_floor_minus_tails_ms"] = round(stats[3]["ms"] - min(stats[0]["ms"], stats[1]["ms"]), 4)
    for step in steps.values():
        step.release()

    # the whole call: propose_tails against tails + torch.sort
    g = torch.Generator().manual_seed(3)
    chosen = torch.arange(n) if not heads or heads >= n else torch.sort(torch.randperm(n, generator=g)[:heads]).values
    chosen = chosen.to(dev)
    relation = int(r[0])
    served = predict.Predictor(model, data, k=k, batch_size=bs)
    rel = torch.full_like(chosen, relation)

    def torch_route():
        ids, scores, _ = served.tails(chosen, rel)
        present = (ids >= 0).reshape(-1)
        order = torch.sort(scores.reshape(-1)[present], descending=True, stable=True).indices[:k]
        query = torch.arange(len(chosen), device=dev).repeat_interleave(k)[present][order]
        return chosen[query], ids.reshape(-1)[present][order], scores.reshape(-1)[present][order]

    served.propose_tails(relation, heads=chosen[:bs])          # (both captures are made outside the timed calls)
    served.tails(chosen[:bs], rel[:bs])
    t_propose, got = wall_ms(lambda: served.propose_tails(relation, heads=chosen))
    t_torch, want = wall_ms(torch_route)
    t_propose2, _ = wall_ms(lambda: served.propose_tails(relation, heads=chosen))
    t_torch2, _ = wall_ms(torch_route)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want)), "propose_tails and tails + torch.sort disagree"
    served.close()
    out["call_ms"] = dict(heads=len(chosen), replays=-(-len(chosen) // bs), propose_tails=[t_propose, t_propose2],
                          tails_then_sort=[t_torch, t_torch2],
                          result_bytes_propose=k * 20 + 8, result_bytes_tails=len(chosen) * (k * 12 + 8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=2048, help="heads of the whole-call comparison (0: every entity)")
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propose_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/propose_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cases = [lambda b=b, k=k: merge_case(b, k, args.reps, args.warmup, dev) for b in (8, 64) for k in (10, 256)]
    cases += [lambda s=s: shape_case(s, args.k, args.batch, args.heads, args.reps, args.warmup, dev)
              for s in args.shapes.split(",") if s]
    for case in cases:
        line = json.dumps(case())
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
