"""Timing of CANDIDATE SETS (predict.Predictor.tails(among=), the ultra_filtered_*_among entries) on one GPU:

    python tools/among_bench.py [--reps 30] [--warmup 5] [--sizes 14541,123182,2000000] [--shapes fb15k237,yago310]
                                [--out profiles/among_bench.jsonl]

  (a) selection_ms   the selection alone, as captured calls on the same (8, N) scores, k = 10, medians with min .. max: the list
                     route -- ultra_filtered_topk_among, and ultra_filtered_above_among at a threshold with about 5 % members --
                     against the route a user had before: the parent entry with known u complement(among) as its deny list.
                     Lists of 100, 4,096 and N / 4 ids, each once shared by the 8 rows and once one per row; 64 known ids a row.
                     index_bytes: the bytes of index buffer each route needs (the lists with their spans / offsets).
  (b) step_ms        the captured `tails` step with a shared 4,096-id set against the same step without one (captured twice: the
                     run-to-run spread), run alternately, by device events.
  (c) first_call_ms  Predictor.tails(among=S): the first call with a set (captures the step of its own key), and a later call
                     with a different set of the same size -- which must not capture: asserted from the capture count.
One JSON line per selection size and per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import _lib, models, predict, synthetic, tasks  # noqa: E402


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
    fn()
    torch.cuda.synchronize()
    return round(1e3 * (time.perf_counter() - t0), 3)


def selection_case(n, bs, k, reps, warmup, dev):
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(bs, n, generator=g).to(dev)
    known = torch.zeros(bs, n, dtype=torch.bool, device=dev)
    for b in range(bs):
        known[b, torch.randint(0, n, (64,), generator=g).to(dev)] = True
    rows, ids = known.nonzero().t()
    ptr = torch.searchsorted(rows.contiguous(), torch.arange(bs + 1, device=dev))
    index = ids.contiguous()
    threshold = 1.645                            # (about 5 % of a standard normal row, so of a random list of it)
    out = dict(tool="among_bench", part="selection", N=n, batch=bs, k=k, threshold=threshold, cases={})
    calls, notes = {}, {}
    for length in (100, 4096, n // 4):
        for shared in (True, False):
            lists = [torch.randperm(n, generator=g)[:length].sort().values for _ in range(1 if shared else bs)]
            span = torch.tensor([[0, length]] * bs if shared else [[b * length, (b + 1) * length] for b in range(bs)], device=dev)
            listed = torch.cat(lists).to(dev)
            deny = known.clone()                 # the route of before: known u complement(among), one list per row
            for b in range(bs):
                allowed = torch.zeros(n, dtype=torch.bool, device=dev)
                allowed[lists[0 if shared else b].to(dev)] = True
                deny[b] |= ~allowed
            d_rows, d_ids = deny.nonzero().t()
            d_ptr = torch.searchsorted(d_rows.contiguous(), torch.arange(bs + 1, device=dev))
            d_index = d_ids.contiguous()
            name = "%d_%s" % (length, "shared" if shared else "per_row")
            among = dict(among=(span, listed), among_capacity=length)
            calls[name + "/topk_among"] = lambda among=among: predict.filtered_topk(pred, k, ptr, index, **among)
            calls[name + "/topk_complement"] = lambda p=d_ptr, i=d_index: predict.filtered_topk(pred, k, p, i)
            calls[name + "/above_among"] = lambda among=among: predict.filtered_above(pred, threshold, ptr, index, **among)
            calls[name + "/above_complement"] = lambda p=d_ptr, i=d_index: predict.filtered_above(pred, threshold, p, i)
            notes[name] = dict(list_ids=length, index_bytes_among=8 * (listed.numel() + span.numel() + index.numel() + ptr.numel()),
                               index_bytes_complement=8 * (d_index.numel() + d_ptr.numel()))
            # the two routes agree
            a, c = calls[name + "/topk_among"](), calls[name + "/topk_complement"]()
            assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
            a, c = calls[name + "/above_among"](), calls[name + "/above_complement"]()
            total = int(c[0][-1])
            assert torch.equal(a[0], c[0]) and torch.equal(a[1][:total], c[1][:total])
    stats = dict(zip(calls, timed([graphed(fn) for fn in calls.values()], reps, warmup)))
    for name, note in notes.items():
        note.update({key.split("/")[1]: value for key, value in stats.items() if key.startswith(name + "/")})
        for kind in ("topk", "above"):
            note[kind + "_complement_over_among"] = round(note[kind + "_complement"]["ms"] / note[kind + "_among"]["ms"], 2)
        out["cases"][name] = note
    return out


def shape_case(name, k, bs, reps, warmup, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    n = int(data.num_nodes)
    g = torch.Generator().manual_seed(9)
    sets = [torch.randperm(n, generator=g)[:4096].sort().values.to(dev) for _ in range(2)]
    out = dict(tool="among_bench", part="step", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k, set_ids=4096)

    # (b) the captured step with a shared set against the step without one
    ptr, index = predict.known_answers(data, h, r, "tail")
    steps = {"static": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16),
             "static_again": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16),
             "among_4096": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16, among=(1 << 16, _lib.TOPK_CHUNK))}
    for step in steps.values():
        step.load_index(index.contiguous())
    steps["among_4096"].load_among(sets[0])
    steps["among_4096"].among_span.copy_(torch.tensor([[0, 4096]] * bs, device=dev))
    stats = timed([lambda s=step: s(h, r, ptr.contiguous()) for step in steps.values()], reps, warmup)
    out["step_ms"] = dict(zip(steps, stats))
    out["static_spread_ms"] = round(abs(stats[0]["ms"] - stats[1]["ms"]), 4)
    out["among_minus_static_ms"] = round(stats[2]["ms"] - stats[0]["ms"], 4)
    for step in steps.values():
        step.release()

    # (c) the first call with a set, and a later call with another set of the same size: no capture
    captures = [0]
    real = torch.cuda.CUDAGraph

    def counting(*args, **kwargs):
        captures[0] += 1
        return real(*args, **kwargs)

    torch.cuda.CUDAGraph = counting
    try:
        served = predict.Predictor(model, data, k=k, batch_size=bs)
        served.tails(h, r)
        without = captures[0]
        first = wall_ms(lambda: served.tails(h, r, among=sets[0]))
        after_first = captures[0]
        later = wall_ms(lambda: served.tails(h, r, among=sets[1]))
        plain = wall_ms(lambda: served.tails(h, r))
        assert after_first == without + 1 and captures[0] == after_first, "a later call with another set of the same size captured"
        served.close()
    finally:
        torch.cuda.CUDAGraph = real
    out["first_call_ms"] = dict(first_with_a_set=first, later_with_another_set=later, without_a_set=plain,
                                captures=dict(without=without, first_with_a_set=after_first - without, later=0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sizes", default="14541,123182,2000000")
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "among_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/among_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cases = [lambda n=int(n): selection_case(n, args.batch, args.k, args.reps, args.warmup, dev) for n in args.sizes.split(",") if n]
    cases += [lambda s=s: shape_case(s, args.k, args.batch, args.reps, args.warmup, dev) for s in args.shapes.split(",") if s]
    for case in cases:
        line = json.dumps(case())
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
