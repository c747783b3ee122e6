"""Timing of the serving path (ultra_amd.predict) on one GPU, by device events after a warm-up, alternating in one process:

    python tools/predict_bench.py [--reps 30] [--warmup 5] [-k 10] [--shapes fb15k237,yago310,long] [--out profiles/predict_bench.jsonl]

  (a) predict_step_ms   the captured predict step (candidate construction, forward, ultra_filtered_topk: one hipGraph replay)
  (b) forward_ms        the captured bare forward, graph.GraphedForward, on a prebuilt (bs, N, 3) batch
  (c) topk_hip_ms       ultra_filtered_topk alone, on the scores of that forward and the known lists of the queries (a captured
                        call, like (d): neither carries the host's launch overhead)
  (d) topk_torch_ms     the torch route a user would write today on the same scores and lists: a strict-style (bs, N) boolean
                        mask, masked_fill(-inf), torch.topk (torch_topk_only_ms: the torch.topk call by itself)
Shapes: FB15k237 and YAGO3-10 (synthetic graphs of their node, edge and relation counts, ultra_3g weights, tail queries of the
test triples, batch 8), and one long row -- N = 2,000,000, batch 8, random scores, 2,000 known ids per row, (c) and (d) only.
For (c): topk_bytes = scores read once + known lists + outputs; topk_gbps = those bytes over topk_hip_ms; roof = topk_gbps over
8 TB/s; latency_bound = the bytes would take under 2 us at 8 TB/s (less than the floor of the call's two launches), so the
time is launch and dependency latency, not traffic.  One JSON line per shape, appended to --out.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py --reps 5` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import graph, models, predict, synthetic, tasks  # noqa: E402

HBM_BPS = 8e12


def timed(fns, reps, warmup):
    """Median device-event milliseconds of every callable, run alternately."""
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


def graphed(fn):
    """fn captured into a hipGraph after a warm-up: the replay -- both selection routes are timed this way, so neither carries
    the host's launch overhead."""
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


def torch_route(pred, flat, k):
    """flat = row * N + id of every known answer (precomputed: `mask[rows, ids] = False` does not record into a graph)."""
    mask = torch.ones(pred.shape, dtype=torch.bool, device=pred.device)
    mask.view(-1).index_fill_(0, flat, False)
    return pred.masked_fill(~mask, float("-inf")).topk(k)


def selection_case(name, pred, ptr, index, k, reps, warmup, extra=None):
    bs, n = pred.shape
    flat = torch.arange(bs, device=pred.device).repeat_interleave(ptr[1:] - ptr[:-1]) * n + index
    (hip_ms, torch_ms, only_ms), (hip_min, torch_min, _) = timed(
        [graphed(lambda: predict.filtered_topk(pred, k, ptr, index)), graphed(lambda: torch_route(pred, flat, k)),
         graphed(lambda: pred.topk(k))], reps, warmup)
    ids, _, count = predict.filtered_topk(pred, k, ptr, index)
    t_ids = torch_route(pred, flat, k).indices
    full = count == k
    nbytes = 4 * bs * n + 8 * (bs + 1) + 8 * index.numel() + bs * k * 12 + 8 * bs
    out = dict(tool="predict_bench", shape=name, batch=bs, N=n, k=k, known=int(index.numel()),
               topk_hip_ms=round(hip_ms, 4), topk_hip_ms_min=round(hip_min, 4), topk_torch_ms=round(torch_ms, 4),
               topk_torch_ms_min=round(torch_min, 4), torch_topk_only_ms=round(only_ms, 4),
               torch_over_hip=round(torch_ms / hip_ms, 2), topk_bytes=nbytes,
               topk_gbps=round(nbytes / (hip_ms * 1e-3) / 1e9, 1), roof=round(nbytes / (hip_ms * 1e-3) / HBM_BPS, 4),
               latency_bound=bool(nbytes / HBM_BPS < 2e-6),
               # (the torch route leaves ties to the backend: only the id SETS of full rows are compared)
               same_id_sets_as_torch=bool(torch.equal(ids[full].sort(dim=1).values, t_ids[full].sort(dim=1).values)))
    out.update(extra or {})
    return out


def model_case(name, k, bs, reps, warmup, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    t_batch, _ = tasks.all_negative(data, triples)
    t_batch = t_batch.contiguous()
    forward = graph.GraphedForward(model, data, t_batch)
    predictor = predict.Predictor(model, data, k=k, batch_size=bs)
    predictor.tails(h, r)                                  # (captures the step)
    step = predictor._steps["tail"]
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    step.load_index(index)
    (step_ms, fwd_ms), (step_min, fwd_min) = timed([lambda: step(h, r, ptr), lambda: forward(t_batch)], reps, warmup)
    pred = forward(t_batch).float().clone()
    got = [t.clone() for t in step(h, r, ptr)]
    want = predict.filtered_topk(pred, k, ptr, index)
    extra = dict(predict_step_ms=round(step_ms, 4), predict_step_ms_min=round(step_min, 4), forward_ms=round(fwd_ms, 4),
                 forward_ms_min=round(fwd_min, 4), step_over_forward=round(step_ms / fwd_ms, 4),
                 step_minus_forward_us=round(1e3 * (step_ms - fwd_ms), 2),
                 step_equals_kernel_on_forward_scores=bool(all(torch.equal(a, b) for a, b in zip(got, want))))
    out = selection_case(name, pred, ptr, index, k, reps, warmup, extra)
    predictor.close()
    return out


def long_case(k, reps, warmup, dev, n=2_000_000, bs=8, known_per_row=2000):
    gen = torch.Generator().manual_seed(7)
    pred = torch.randn(bs, n, generator=gen).to(dev)
    rows = [torch.randperm(n, generator=gen)[:known_per_row].sort().values for _ in range(bs)]
    ptr = torch.arange(bs + 1) * known_per_row
    return selection_case("long", pred, ptr.to(dev), torch.cat(rows).to(dev), k, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310,long")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        if name == "long":
            out = long_case(args.k, args.reps, args.warmup, dev)
        else:
            out = model_case(name, args.k, args.batch, args.reps, args.warmup, dev)
        line = json.dumps(out)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
