"""Timing of WHAT-IF logical queries (ultra_amd.query_predict.QueryPredictor.answers(assuming=)) on one GPU:

    python tools/query_assume_bench.py [--reps 20] [--warmup 3] [--fact-reps 5] [--shapes fb15k237,yago310]
                                       [--out profiles/query_assume_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, the ultraquery weights of
tests/golden/ultraquery.pt.xz, batch 16, 16 satisfiable 1p and 16 satisfiable 2p queries drawn from the edge list
(tools/query_live_bench.py's).  Hypotheses `off_hubs` run between the nodes of the fewest in-edges.  Every figure is a median with
its minimum and maximum, everything compared in the same run.

  (1) hypothesis_to_answer  wall-clock milliseconds from "the sixteen 2p queries, one hypothesis each" to their answers, host work
                            included (the device synchronised before and after; --fact-reps repetitions):
                              assume_ms   one answers(queries, assuming=[...]) call: one overlay refill, one batch
                              state_ms    the route without the argument: per query add_facts -> answers([query]) ->
                                          remove_facts on the same predictor, the sixteen in turn
  (2) answers_ms            answers() of the 32 queries (two batches) by device events, run alternately:
                              static          a predictor that holds no edit
                              stated16        the sixteen off-hub facts stated (add_facts), held in the delta
                              whatif_off_hubs the same sixteen facts as hypotheses, eight among the 1p and eight among the 2p
                                              queries: both batches run over the overlay
                              whatif_longest  ONE hypothesis whose edge points into the graph's longest (tail, relation) segment
  (3) traversal_ms          ultra_symbolic_traversal_edit_rows_owned alone (a captured call, 16 samples that all ask for the
                            relation of the edges) with its owners, and with every owner rewritten to -1 on the same layout --
                            every sample then scans every touched tail, what the launch would do without the early-out: for
                            `off_hubs` and for `longest_one`, one sample's hypothesis at the longest segment
  (4) fill_ms               AssumedFacts.fill of sixteen hypotheses with the traversal view kept current, wall clock with the
                            device synchronised, over an empty delta and over one that holds 256 facts
One JSON line per shape, appended to --out."""
import argparse
import ctypes
import io
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from live_graph_bench import graphed, random_facts, wall_ms  # noqa: E402
from query_live_bench import sample_queries  # noqa: E402
from ultra_amd import _lib, models, query_predict, rspmm, synthetic, tasks, ultraquery  # noqa: E402


def spread(times, digits=3):
    return dict(median=round(statistics.median(times), digits), min=round(min(times), digits), max=round(max(times), digits))


def timed_spread(fns, reps, warmup):
    """Per callable the device-event milliseconds of `reps` runs, the callables run alternately."""
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
    return times


def longest_segment(data):
    """(tail, relation, length) of the longest (tail, relation) segment of the traversal CSR."""
    rels = int(data.num_relations)
    size = torch.bincount(data.edge_index[1] * rels + data.edge_type, minlength=int(data.num_nodes) * rels)
    at = int(size.argmax())
    return at // rels, at % rels, int(size[at])


def fact_into(tail, relation, other, half):
    """The fact whose direct or inverse edge is other -> tail of type `relation`."""
    return (other, relation, tail) if relation < half else (tail, relation - half, other)


def traversal_case(data, overlay, relation, bs, reps, warmup, dev):
    n = int(data.num_nodes)
    gen = torch.Generator().manual_seed(2)
    h = (torch.rand(bs, n, generator=gen) * (torch.rand(bs, n, generator=gen) < 0.01)).to(dev)
    r = torch.full((bs,), relation, dtype=torch.long, device=dev)
    csr = ultraquery.traversal_csr(data.edge_index, data.edge_type, n)
    t = ultraquery.symbolic_traversal(data.edge_index, data.edge_type, n, h, r)
    operand, owner = overlay.traversal_operand(), overlay.traversal_owner

    def fix_up():
        _lib.check(_lib.lib.ultra_symbolic_traversal_edit_rows_owned(
            csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), n, ctypes.byref(operand), owner.data_ptr(),
            r.data_ptr(), bs, _lib.F32, h.data_ptr(), t.data_ptr(), _lib.stream_of(h)))
    call = graphed(fix_up)
    owners = owner.clone()
    (owned,) = timed_spread([call], reps, warmup)
    owner.fill_(-1)
    (shared,) = timed_spread([call], reps, warmup)
    owner.copy_(owners)
    return dict(touched_tails=int(overlay.traversal.count), edges=overlay.num_edges, owned_ms=spread(owned, 4),
                every_owner_shared_ms=spread(shared, 4))


def shape_case(name, k, bs, reps, warmup, fact_reps, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    with open(os.path.join(ROOT, "tests", "golden", "ultraquery.pt.xz"), "rb") as f:
        weights = torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)["weights"]
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = ultraquery.UltraQuery(models.Ultra(**cfg))
    model.load_state_dict(weights, strict=True)
    model = model.to(dev).eval()
    one, two = sample_queries(data, bs, 3)
    queries = one + two
    half = int(data.num_relations) // 2
    degree = torch.bincount(data.edge_index[1], minlength=data.num_nodes)
    short = degree.argsort()[:2 * bs].tolist()
    off_hubs = [(short[i], i % half, short[bs + i]) for i in range(bs)]
    tail, relation, length = longest_segment(data)
    at_hub = fact_into(tail, relation, short[0], half)
    out = dict(tool="query_assume_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]), k=k,
               longest_segment=length)

    # (1) sixteen hypotheses to their answers: the what-if call against stating and retracting
    live = query_predict.QueryPredictor(model, data, k=k, batch_size=bs)
    facts = [[f] for f in off_hubs]
    live.answers(two), live.answers(two, assuming=facts)        # serving: the plan, the CSR and the overlay exist
    assert not live._assume_loop_only, "the engine route serves the shape"

    def stated():
        for query, (h, r, t) in zip(two, off_hubs):
            live.add_facts(h, r, t)
            live.answers([query])
            live.remove_facts(h, r, t)

    stated()
    assume, state = [], []
    for _ in range(fact_reps):
        assume.append(wall_ms(lambda: live.answers(two, assuming=facts)))
        state.append(wall_ms(stated))
    out["hypothesis_to_answer"] = dict(queries=bs, reps=fact_reps, assume_ms=spread(assume), state_ms=spread(state),
                                       state_over_assume=round(statistics.median(state) / statistics.median(assume), 1))

    # (2) answers() in four states, alternately
    static = query_predict.QueryPredictor(model, data, k=k, batch_size=bs)
    held = query_predict.QueryPredictor(model, data, k=k, batch_size=bs)
    held.add_facts(*[list(column) for column in zip(*off_hubs)])
    part = bs // 2
    both = [[f] for f in off_hubs[:part]] + [None] * (bs - part) + [[f] for f in off_hubs[part:]] + [None] * part
    longest = [None] * bs + [[at_hub]] + [None] * (bs - 1)
    runs = {"static": lambda: static.answers(queries), "stated16": lambda: held.answers(queries),
            "whatif_off_hubs": lambda: static.answers(queries, assuming=both),
            "whatif_longest": lambda: static.answers(queries, assuming=longest)}
    order = list(runs)
    times = timed_spread([runs[key] for key in order], reps, warmup)
    assert not static._assume_loop_only
    out["answers_ms"] = {key: spread(t) for key, t in zip(order, times)}
    base = statistics.median(times[0])
    out["answers_over_static"] = {key: round(statistics.median(t) / base, 3) for key, t in zip(order, times)}
    out["whatif_off_hubs_over_stated16"] = round(statistics.median(times[2]) / statistics.median(times[1]), 3)

    # (3) the traversal entry alone, with its owners and with every owner shared
    overlay = rspmm.AssumedFacts(data, None, bs, 8)
    out["traversal_ms"] = {}
    same_relation = [(short[i], 0, short[bs + i]) for i in range(bs)]
    for key, fill, rel in (("off_hubs", [[f] for f in same_relation], 0), ("longest_one", [[at_hub]] + [None] * (bs - 1), relation)):
        overlay.fill(fill)
        out["traversal_ms"][key] = traversal_case(data, overlay, rel, bs, reps, warmup, dev)

    # (4) the refill with the traversal view
    out["fill_ms"] = {}
    full = rspmm.GraphDelta(data, 256)
    full.add(*random_facts(data, 256, 7, dev))
    for key, delta in (("empty_delta", rspmm.GraphDelta(data, 256)), ("delta_256_facts", full)):
        filled = rspmm.AssumedFacts(data, delta, bs, 8)
        filled.traversal_operand()
        fill = [torch.tensor([f], device=dev) for f in off_hubs]
        times = []
        for rep in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            filled.fill(fill)
            torch.cuda.synchronize()
            if rep >= warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        out["fill_ms"][key] = spread(times, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fact-reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_assume_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/query_assume_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
