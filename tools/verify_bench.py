"""Timing of leave-one-out verification (Predictor.verify_tails) on one GPU, by device events after a warm-up, the routes
alternating in one process:

    python tools/verify_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--routes a,b,c,d,w] [--out profiles/verify_bench.jsonl]

  (a) verify_step_ms        the captured verify step: keep rows, candidates, masked forward, filtered rank, score gather -- one
                            hipGraph replay for 8 stated facts
  (b) predict_step_ms       the captured predict step on the same queries: the same forward WITHOUT masks (one-hot layer 0, fused
                            layers) plus the top-k selection -- the floor
  (c) verify_loop_step_ms   the verify step captured with every per-sample call forced through the per-slice loop (the tool
                            answers ULTRA_ERR_UNSUPPORTED in the entry's place while that step is built; the library has no switch)
  (d) per_triple_ms         what a user had to do before: per triple a remove_easy_edges copy of the graph and a forward on it,
                            plan construction included (predict.verify_reference), on the same 8 facts; median of --reps-d runs
  (w) the layer walk alone, (bs, N, 64) operands with a dense boundary on the reference-order plan, captured calls:
      walk_samples_ms (one keep row per sample), walk_shared_ms (one row for the batch), walk_plain_ms (no weights: the
      assembly walk).  mask_bytes = bs * E * 4 (read through perm); compulsory_bytes = input + boundary + output
      (3 * bs * N * 256) + records and perm once (12 * E); walk_samples_roof = (mask + compulsory bytes) / walk_samples_ms / 8 TB/s.
Shapes: FB15k237 and YAGO3-10 (synthetic graphs of their node, edge and relation counts, ultra_3g weights, the first 8
training facts, batch 8).  One JSON line per shape, appended to --out; a route left out is written as "not measured".
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/verify_bench.py --reps 5 --routes a,c,w --shapes fb15k237` in a
run of its own.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks  # noqa: E402

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


class loop_route(object):
    """Inside: Plan.masked_samples_entry answers ULTRA_ERR_UNSUPPORTED without launching, so Plan.forward runs its per-slice loop."""

    def __enter__(self):
        self.plain = rspmm.Plan.masked_samples_entry
        rspmm.Plan.masked_samples_entry = lambda *args, **kwargs: _lib.ULTRA_ERR_UNSUPPORTED

    def __exit__(self, *exc):
        rspmm.Plan.masked_samples_entry = self.plain


def case(name, bs, reps, warmup, reps_d, routes, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    num_edge, n = data.edge_index.shape[1], int(data.num_nodes)
    h, t, r = (c.contiguous() for c in (data.edge_index[0, :bs], data.edge_index[1, :bs], data.edge_type[:bs]))
    triples = torch.stack([h, t, r], dim=-1)
    out = dict(tool="verify_bench", shape=name, batch=bs, N=n, E=num_edge, reps=reps)
    fns, names, results = [], [], {}
    predictor = loop_predictor = None
    if "a" in routes or "b" in routes:
        predictor = predict.Predictor(model, data, k=10, batch_size=bs)
    if "a" in routes:
        results["captured"] = [v.clone() for v in predictor.verify_tails(h, r, t)]
        step = predictor._steps["verify_tail"]
        ptr, index = tasks.known_answers(data, triples, "tail")
        ptr = ptr.contiguous()
        step.load_index(index)
        fns.append(lambda: step(triples, ptr))
        names.append("verify_step_ms")
    if "b" in routes:
        predictor.tails(h, r)
        pstep = predictor._steps["tail"]
        pptr, pindex = predict.known_answers(data, h, r, "tail")
        pptr = pptr.contiguous()
        pstep.load_index(pindex)
        fns.append(lambda: pstep(h, r, pptr))
        names.append("predict_step_ms")
    if "c" in routes:
        loop_predictor = predict.Predictor(model, data, k=10, batch_size=bs)
        with loop_route():
            results["loop"] = [v.clone() for v in loop_predictor.verify_tails(h, r, t)]
        lstep = loop_predictor._steps["verify_tail"]
        lptr, lindex = tasks.known_answers(data, triples, "tail")
        lptr = lptr.contiguous()
        lstep.load_index(lindex)
        fns.append(lambda: lstep(triples, lptr))
        names.append("verify_loop_step_ms")
    if fns:
        med, low = timed(fns, reps, warmup)
        for k, m, lo in zip(names, med, low):
            out[k], out[k.replace("_ms", "_ms_min")] = round(m, 4), round(lo, 4)
    if "d" in routes:
        (med,), (low,) = timed([lambda: results.__setitem__("reference", predict.verify_reference(model, data, data, h, r, t, "tail"))],
                               reps_d, 1)
        out["per_triple_ms"], out["per_triple_ms_min"], out["per_triple_reps"] = round(med, 3), round(low, 3), reps_d
    if "captured" in results:
        for other in ("loop", "reference"):
            if other in results:
                out["captured_equals_" + other] = bool(all(torch.equal(a, b) for a, b in zip(results["captured"], results[other])))
    if "w" in routes:
        gen = torch.Generator().manual_seed(1)
        plan = rspmm.get_plan(data.edge_index, data.edge_type, n, int(data.num_relations))
        rel = torch.randn(bs, int(data.num_relations), 64, generator=gen).to(dev)
        x = torch.randn(bs, n, 64, generator=gen).to(dev)
        bnd = torch.randn(bs, n, 64, generator=gen).to(dev)
        keep = model.entity_model.leave_one_out_keep(data, triples)
        res = torch.empty_like(x)
        (ws, wl, wsh, wp), _ = timed([
            graphed(lambda: plan.forward(rel, x, edge_weight=keep, boundary=bnd, keep=True, out=res)),
            graphed(lambda: [plan.forward(rel[s:s + 1], x[s:s + 1], edge_weight=keep[s], boundary=bnd[s:s + 1], keep=True,
                                          out=res[s:s + 1], weight_epoch=0) for s in range(bs)]),
            graphed(lambda: plan.forward(rel, x, edge_weight=keep[0], boundary=bnd, keep=True, out=res)),
            graphed(lambda: plan.forward(rel, x, boundary=bnd, out=res))], reps, warmup)
        mask_bytes, compulsory = bs * num_edge * 4, 3 * bs * n * 256 + 12 * num_edge
        out.update(walk_samples_ms=round(ws, 4), walk_loop_ms=round(wl, 4), walk_shared_ms=round(wsh, 4), walk_plain_ms=round(wp, 4),
                   mask_bytes=mask_bytes, compulsory_bytes=compulsory, plan_exact=bool(plan.exact),
                   walk_samples_roof=round((mask_bytes + compulsory) / (ws * 1e-3) / HBM_BPS, 4))
    for k in ("verify_step_ms", "predict_step_ms", "verify_loop_step_ms", "per_triple_ms", "walk_samples_ms"):
        out.setdefault(k, "not measured")
    num = lambda k: isinstance(out[k], float)      # noqa: E731
    if num("verify_step_ms") and num("predict_step_ms"):
        out["leave_one_out_price_ms"] = round(out["verify_step_ms"] - out["predict_step_ms"], 4)
    if num("verify_step_ms") and num("per_triple_ms"):
        out["per_triple_over_verify_step"] = round(out["per_triple_ms"] / out["verify_step_ms"], 1)
    if num("verify_step_ms") and num("verify_loop_step_ms"):
        out["loop_over_kernel_route"] = round(out["verify_loop_step_ms"] / out["verify_step_ms"], 4)
    for p in (predictor, loop_predictor):
        if p is not None:
            p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--reps-d", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--routes", default="a,b,c,d,w")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        out = case(name, args.batch, args.reps, args.warmup, args.reps_d, set(args.routes.split(",")), dev)
        line = json.dumps(out)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rspmm.clear_plan_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
