"""Timing of complex logical query answering (UltraQuery) at FB15k237's shape on one GPU.

    python tools/query_bench.py [--per-type 16] [--reps 3] [--compiled]

Prints one JSON line:
  types            per BetaE type: queries/s of UltraQuery.forward + batch_evaluate on a batch of `per-type` queries of that
                   type (host clock around a device synchronise, after one warm-up batch), and that time split into
                   projections (RelationProjection calls, by device events), ranking (batch_evaluate) and executor (the
                   rest: the torch stack machine and fuzzy logic); with --compiled also compiled_ms,
                   compiled_projection_ms and compiled_executor_ms: the same batches through query_exec.forward (the host
                   compiler, one upload and one ultra_query_segment launch per segment in place of the stack machine)
  traversal        ultra_symbolic_traversal vs its torch restatement (the reference's form: (B, E) relation mask, gather,
                   max-scatter), 64 queries, fp32, by device events; bytes = CSR + one read of h per edge of the query's
                   relation + the output -- the kernel is a gather whose time should be judged against latency, not HBM bytes
  ranking          ultra_answer_ranking vs its torch restatement (stable argsort), 64 queries; bytes = one read of pred --
                   judged against the HBM roof only for large batches; at 64 workgroups it is latency bound
The graph and queries are synthetic (ultra_amd.synthetic, ultra_amd.query_data.sample_queries); the weights are those of the
reference's ultraquery.pth as recorded in tests/golden/ultraquery.pt.xz.
"""
import argparse
import io
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, query_data, query_eval, query_exec, synthetic, ultraquery  # noqa: E402

HBM_BPS = 8e12


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-type", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--compiled", action="store_true", help="also time the compiled executor (query_exec.forward)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz"), "rb") as f:
        weights = torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)["weights"]
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=False)
    train, ds = query_data.sample_queries(kg, args.per_type * 2, seed=1)
    graph = train.to(dev)
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = ultraquery.UltraQuery(models.Ultra(**cfg))
    model.load_state_dict(weights, strict=True)
    model = model.to(dev).eval()

    proj_ms = []
    orig_forward = model.model.forward

    def timed_projection(g, h, r):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = orig_forward(g, h, r)
        b.record()
        proj_ms.append((a, b))
        return out
    model.model.forward = timed_projection

    types = {}
    for t, name in enumerate(ds.id2type):
        idx = [i for i in range(len(ds)) if ds.types[i] == t]
        batches = []
        for k in range(2):
            items = [ds[i] for i in idx[k * args.per_type:(k + 1) * args.per_type]]
            batches.append({key: torch.stack([torch.as_tensor(it[key]) for it in items]).to(dev) for key in items[0]})

        def measure(forward):
            rows = []
            with torch.no_grad():
                for rep in range(1 + args.reps):
                    batch = batches[rep % 2]
                    proj_ms.clear()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pred = forward(batch["query"])
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    query_eval.batch_evaluate(pred, (batch["type"], batch["easy_answer"], batch["hard_answer"]))
                    r1.record()
                    torch.cuda.synchronize()
                    total = (time.perf_counter() - t0) * 1e3
                    if rep:
                        proj = sum(a.elapsed_time(b) for a, b in proj_ms)
                        rank = r0.elapsed_time(r1)
                        rows.append((total, proj, rank, len(proj_ms)))
            return tuple(statistics.median(r[i] for r in rows) for i in range(3)) + (rows[0][3],)

        total, proj, rank, calls = measure(lambda q: model(graph, q, symbolic_traversal=False))
        types[name] = dict(queries_per_s=round(args.per_type / total * 1e3, 1), ms=round(total, 2),
                           projection_ms=round(proj, 2), ranking_ms=round(rank, 3),
                           executor_ms=round(total - proj - rank, 2), projection_calls=calls)
        if args.compiled:
            total, proj, rank, calls = measure(lambda q: query_exec.forward(model, graph, q, symbolic_traversal=False))
            assert calls == types[name]["projection_calls"]
            types[name].update(compiled_ms=round(total, 2), compiled_projection_ms=round(proj, 2),
                               compiled_executor_ms=round(total - proj - rank, 2))

    # kernel 2a against the restatement
    n = graph.num_nodes
    gen = torch.Generator().manual_seed(3)
    h = (torch.rand(64, n, generator=gen) * (torch.rand(64, n, generator=gen) < 0.05)).to(dev)
    r = torch.randint(0, graph.num_relations, (64,), generator=gen).to(dev)
    ei, et = graph.edge_index, graph.edge_type
    ultraquery.symbolic_traversal(ei, et, n, h, r)
    hip = event_ms(lambda: ultraquery.symbolic_traversal(ei, et, n, h, r), 20)
    ref = event_ms(lambda: ultraquery.symbolic_traversal_reference(ei, et, n, h, r), 5)
    match = int(sum(int((et == int(x)).sum()) for x in r.tolist()))
    tb = 8 * (n + 1) + 8 * ei.shape[1] + 64 * 4 * n + match * 8 + 64 * 4 * n
    traversal = dict(hip_ms=round(hip, 4), torch_ms=round(ref, 3), speedup=round(ref / hip, 1), bytes=tb,
                     gbps=round(tb / hip / 1e6, 1), hbm_roof_fraction=round(tb / hip / 1e-3 / HBM_BPS, 4))

    # kernel 2b against the restatement
    pred = torch.randn(64, n, generator=gen).to(dev)
    easy = (torch.rand(64, n, generator=gen) < 0.003).to(dev)
    hard = ((torch.rand(64, n, generator=gen) < 0.001).to(dev)) & ~easy
    target = (None, easy, hard)
    query_eval.batch_evaluate(pred, target)
    hip = event_ms(lambda: query_eval.batch_evaluate(pred, target), 20)
    ref = event_ms(lambda: query_eval.batch_evaluate_reference(pred, target), 5)
    rb = 64 * n * 4
    ranking = dict(hip_ms=round(hip, 4), torch_ms=round(ref, 3), speedup=round(ref / hip, 1), bytes=rb,
                   gbps=round(rb / hip / 1e6, 1), hbm_roof_fraction=round(rb / hip / 1e-3 / HBM_BPS, 4),
                   note="host-side answer lists and output sizing are included in both")
    print(json.dumps(dict(shape="fb15k237", per_type=args.per_type, types=types, traversal=traversal, ranking=ranking)))


if __name__ == "__main__":
    main()
