"""Timing of the answer-set selection (ultra_filtered_above) on one GPU, by device events after a warm-up, alternating in one
process with the torch route a user would write today:

    python tools/answer_set_bench.py [--reps 30] [--warmup 5] [--batch 8] [--sizes 14541,123182,2000000]
                                     [--shares 0.001,0.05,0.5] [--out profiles/answer_set_bench.jsonl]

  (a) above_hip_ms     predict.filtered_above: every candidate above the threshold that the row's known list does not name,
                       ranked, the lists back to back (count, scan, sort per chunk, merge levels: csrc/above_kernels.hip)
  (b) above_torch_ms   the torch route on the same scores and lists: a (batch, N) boolean mask from the lists,
                       masked_fill(-inf), a stable descending torch.sort of every row, a comparison with the threshold (which
                       marks where every row's list ends; cutting the rows apart would take a host read on top)
Both are captured calls (hipGraph replays): neither carries the host's launch overhead.  Scores: standard normal, so a threshold
at the normal quantile gives the wanted share of members; 2,000 known ids per row (a tenth of the row where it is shorter).
above_bytes = what (a) moves at least: the scores and the known lists read twice (count and fill), the keys written once and read
and written again by every merge level, the gathered scores and the outputs; above_gbps = those bytes over above_hip_ms; roof
= above_gbps over 8 TB/s.  One JSON line per (N, share), appended to --out.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import _lib, predict  # noqa: E402

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
    """fn captured into a hipGraph after a warm-up: the replay, and what the captured call returned."""
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
    return g.replay, keep


def torch_route(pred, flat, threshold):
    """flat = row * N + id of every known answer (precomputed: `mask[rows, ids] = False` does not record into a graph)."""
    mask = torch.ones(pred.shape, dtype=torch.bool, device=pred.device)
    mask.view(-1).index_fill_(0, flat, False)
    values, ids = torch.sort(pred.masked_fill(~mask, float("-inf")), dim=1, descending=True, stable=True)
    return values, ids, values > threshold


def case(n, share, bs, reps, warmup, dev):
    gen = torch.Generator().manual_seed(7)
    pred = torch.randn(bs, n, generator=gen).to(dev)
    threshold = math.sqrt(2.0) * float(torch.erfinv(torch.tensor(1.0 - 2.0 * share, dtype=torch.float64)))
    per_row = min(2000, n // 10)
    rows = [torch.randperm(n, generator=gen)[:per_row].sort().values for _ in range(bs)]
    ptr = (torch.arange(bs + 1) * per_row).to(dev)
    index = torch.cat(rows).to(dev)
    flat = torch.arange(bs, device=dev).repeat_interleave(ptr[1:] - ptr[:-1]) * n + index
    hip, got = graphed(lambda: predict.filtered_above(pred, threshold, ptr, index))
    plain, want = graphed(lambda: torch_route(pred, flat, threshold))
    (hip_ms, torch_ms), (hip_min, torch_min) = timed([hip, plain], reps, warmup)
    out_ptr, ids, _, size = got
    lengths = (out_ptr[1:] - out_ptr[:-1]).tolist()
    same = torch.equal(want[2].sum(dim=1), out_ptr[1:] - out_ptr[:-1]) and all(
        torch.equal(ids[int(out_ptr[b]):int(out_ptr[b + 1])], want[1][b, :lengths[b]]) for b in range(bs))
    total = int(out_ptr[-1])
    chunks = (n + _lib.TOPK_CHUNK - 1) // _lib.TOPK_CHUNK
    levels = max(0, math.ceil(math.log2(chunks)))
    key_bytes = 8 * total * 2 * levels      # written by the fill and read by the last level; both by every level between
    nbytes = 2 * (4 * bs * n + 8 * (bs + 1) + 8 * index.numel()) + key_bytes + total * (4 + 12) + 16 * bs * chunks + 16 * bs
    return dict(tool="answer_set_bench", batch=bs, N=n, share=share, threshold=round(threshold, 4), known=int(index.numel()),
                members=int(size.sum()), listed=total, merge_levels=levels, above_hip_ms=round(hip_ms, 4),
                above_hip_ms_min=round(hip_min, 4), above_torch_ms=round(torch_ms, 4), above_torch_ms_min=round(torch_min, 4),
                torch_over_hip=round(torch_ms / hip_ms, 2), above_bytes=nbytes,
                above_gbps=round(nbytes / (hip_ms * 1e-3) / 1e9, 1), roof=round(nbytes / (hip_ms * 1e-3) / HBM_BPS, 4),
                same_lists_as_torch=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sizes", default="14541,123182,2000000")
    ap.add_argument("--shares", default="0.001,0.05,0.5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "answer_set_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for n in (int(v) for v in args.sizes.split(",")):
        for share in (float(v) for v in args.shares.split(",")):
            line = json.dumps(case(n, share, args.batch, args.reps, args.warmup, dev))
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
