"""Timing of serving complex logical queries (ultra_amd.query_predict) at FB15k237's shape on one GPU, by device events after a
warm-up.

    python tools/query_predict_bench.py [--per-type 16] [--reps 5] [-k 10] [--out FILE]

Prints one JSON line (appended to --out when given):
  answers          per BetaE type: QueryPredictor.answers on `per-type` queries of that type (one batch: host compiler, upload,
                   segments, projections with symbolic traversal, ultra_nonzero_lists, ultra_filtered_topk) -- median
                   milliseconds between device events around the call, and queries/s from them
  segment          ultra_query_segment alone: every segment of the program of a mixed batch (`per-type` queries, all types),
                   both stacks, product logic, launched back to back on buffers of the right shapes.  bytes = what the
                   contract reads and writes (live slots, pushed and popped rows, changed slots); roof = those bytes over
                   the time over 8 TB/s.  A segment moves a few MB at most: latency_bound says whether its bytes would take
                   under 2 us at 8 TB/s, in which case the time is launch latency, not traffic, and the roof share means
                   little
  nonzero          ultra_nonzero_lists against torch.nonzero plus the split into rows (a searchsorted on the row ids), on
                   (per-type, N) sets with 1 % non-zeros; the torch route waits for the device inside nonzero
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, query_data, query_exec, query_predict, synthetic, ultraquery  # noqa: E402

HBM_BPS = 8e12


def event_ms(fn, reps, warmup=1):
    out = []
    for rep in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def segment_bytes(seg, batch, n, stacks):
    """Bytes one launch moves under the contract of ultra_query_segment."""
    rows = 0
    for b in range(batch):
        d = seg.entry_depth[b]
        work = seg.push_row[b] >= 0 or seg.ops[b] or seg.pop_row[b] >= 0
        if not work:
            continue
        rows += d                                       # live slots loaded
        dirty = set()
        if seg.push_row[b] >= 0:
            rows += 1
            dirty.add(d)
            d += 1
        for kind, _ in seg.ops[b]:
            if kind == query_exec.PUSH_ENTITY:
                dirty.add(d)
                d += 1
            elif kind == query_exec.NOT:
                dirty.add(d - 1)
            else:
                dirty.add(0)
                d = 1
        if seg.pop_row[b] >= 0:
            rows += 1
            d -= 1
        rows += sum(1 for j in range(d) if j in dirty)
    return 4 * n * rows * stacks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-type", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz"), "rb") as f:
        weights = torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)["weights"]
    kg = synthetic.make_kg(**synthetic.SHAPES["fb15k237"], seed=11, relation_graph=False)
    train, ds = query_data.sample_queries(kg, args.per_type, seed=1)
    graph = train.to(dev)
    n = graph.num_nodes
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = ultraquery.UltraQuery(models.Ultra(**cfg))
    model.load_state_dict(weights, strict=True)
    model = model.to(dev).eval()

    qp = query_predict.QueryPredictor(model, graph, k=args.k, batch_size=args.per_type)
    answers = {}
    for t, name in enumerate(ds.id2type):
        queries = [ds.queries[i] for i in range(len(ds)) if ds.types[i] == t][:args.per_type]
        ms = event_ms(lambda: qp.answers(queries), args.reps)
        answers[name] = dict(ms=round(ms, 2), queries_per_s=round(len(queries) / ms * 1e3, 1), batches=len(qp.batches(queries)))

    # the segment kernel alone: a mixed batch, one query of every type in turn
    by_type = [[ds.queries[i] for i in range(len(ds)) if ds.types[i] == t] for t in range(len(ds.id2type))]
    mixed = [by_type[j % len(by_type)][j // len(by_type)] for j in range(args.per_type)]
    width = max(len(q) for q in mixed)
    rows = torch.tensor([q.tolist() + [ultraquery.Query.stop] * (width - len(q)) for q in mixed], dtype=torch.long)
    program = query_exec.compile(rows, n, graph.num_relations)
    batch = program.batch
    host, _, seg_off = program.packed()
    n_rel = sum(len(p.relations) for p in program.projections)
    words = host.to(dev)[8 * n_rel:].clone().view(torch.int32)
    stacks = [torch.rand(batch, 2, n, device=dev) for _ in range(2)]
    src = [torch.rand(batch, n, device=dev) for _ in range(2)]
    dst = [torch.empty(batch, n, device=dev) for _ in range(2)]
    segments = []
    for s, seg in enumerate(program.segments):
        first = s == 0

        def launch():
            query_exec.segment(words, seg_off[s], batch, n, "product", stacks[0], None if first else src[0], dst[0],
                               stacks[1], None if first else src[1], dst[1])
        ms = event_ms(launch, 20, warmup=3)
        nbytes = segment_bytes(seg, batch, n, 2)
        segments.append(dict(micro_ops=program.num_micro_ops(s), ms=round(ms, 4), bytes=nbytes,
                             gbps=round(nbytes / ms / 1e6, 1), roof=round(nbytes / (ms * 1e-3) / HBM_BPS, 4),
                             latency_bound=bool(nbytes / HBM_BPS < 2e-6)))
    segment = dict(batch=batch, N=n, projections=len(program.projections), segments=segments,
                   note="latency-bound at these sizes: one launch's bytes take microseconds at the HBM rate, the time is "
                        "launch and dependency latency" if all(x["latency_bound"] for x in segments) else
                        "see latency_bound per segment")

    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(args.per_type, n, generator=gen) * (torch.rand(args.per_type, n, generator=gen) < 0.01)).to(dev)
    edges = torch.arange(args.per_type + 1, device=dev)

    def torch_route():
        sample, col = (x != 0).nonzero().t()
        return torch.searchsorted(sample.contiguous(), edges), col
    hip = event_ms(lambda: query_exec.nonzero_lists(x), 20, warmup=3)
    ref = event_ms(torch_route, 20, warmup=3)
    ptr, index = query_exec.nonzero_lists(x)
    t_ptr, t_index = torch_route()
    nonzero = dict(batch=args.per_type, N=n, hip_ms=round(hip, 4), torch_ms=round(ref, 4), torch_over_hip=round(ref / hip, 2),
                   equal=bool(torch.equal(ptr, t_ptr) and torch.equal(index[:len(t_index)], t_index)))
    line = json.dumps(dict(tool="query_predict_bench", shape="fb15k237", per_type=args.per_type, k=args.k, answers=answers,
                           segment=segment, nonzero=nonzero))
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
