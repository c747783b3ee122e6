"""Timing of RETIRING entities under logical queries (ultra_amd.query_predict.QueryPredictor.retire_entities) on
one GPU:

    python tools/query_retire_bench.py [--reps 20] [--warmup 3] [--fact-reps 3] [--shapes fb15k237,yago310]
                                       [--out profiles/query_retire_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, the ultraquery weights of
tests/golden/ultraquery.pt.xz, batch 16, 16 satisfiable 1p and 16 satisfiable 2p queries drawn from the edge list (those of
tools/query_live_bench.py), everything in one process.  The retired entities have the median degree of the graph and are no
anchor of the queries.

  (a) retirement_to_answers  wall-clock milliseconds from "retire_entities of one entity" to the answers of the next answers()
                             call (the 32 queries: two batches), host work included (time.perf_counter around the calls, the
                             device synchronised before and after; median of --fact-reps with min .. max):
                               live_first_ms  on a predictor whose first edit this is (the delta and its traversal layout are made)
                               live_next_ms   on a predictor that already holds a retirement
                               rebuild_ms     the rebuild: materialized() of a predictor that holds the first retirement, a fresh
                                              QueryPredictor on it and its first answers() (host plan, upload, traversal CSR)
                             with the facts retracted, the rows the tombstones touch and the longest of them -- a neighbour that
                             is a hub pays DESIGN.md 18's chain over its whole row
  (b) answers_ms             answers() of the 32 queries by device events, run alternately, median with min .. max: static, static
                             again (the run-to-run spread), with 1 and with 64 entities retired, and with the same tombstones put
                             there by remove_facts alone (the retired ids still candidates, the lists and the selection those of
                             before).  The difference of the two is what the mask costs; the rest is the price of the tombstones
  (c) lists_ms               the list call alone on (16, N) sets (1 % non-zeros, 1.0 in every retired slot: the final sets of
                             queries that end in a negation), captured calls, run alternately: ultra_nonzero_lists_live,
                             ultra_nonzero_lists_alive with an all-zero bitmap, and with 1 % of the ids retired
One JSON line per shape, appended to --out."""
import argparse
import io
import json
import lzma
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from query_live_bench import sample_queries  # noqa: E402
from retire_bench import graphed, median_entities, spread, timed, wall_ms  # noqa: E402
from ultra_amd import _lib, models, query_predict, rspmm, synthetic, tasks, ultraquery  # noqa: E402
from ultra_amd.live import retired_words  # noqa: E402


def facts_at(data, ids):
    """The distinct direct triples (h, r, t) of `data` that name one of `ids`: what retire_entities retracts."""
    (row, col), kind = data.edge_index, data.edge_type
    at = (torch.isin(row, ids) | torch.isin(col, ids)).nonzero().flatten()
    row, col, kind = row[at], col[at], kind[at]
    direct = int(data.num_relations) // 2
    inverse = kind >= direct
    triples = torch.stack([torch.where(inverse, col, row), torch.where(inverse, kind - direct, kind),
                           torch.where(inverse, row, col)], dim=1)
    return torch.unique(triples, dim=0).unbind(1)


def lists_case(n, bs, reps, warmup, dev):
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(bs, n, generator=gen) * (torch.rand(bs, n, generator=gen) < 0.01)
    gone = torch.randperm(n, generator=gen)[:max(1, n // 100)]
    x[:, gone] = 1.0
    xd = x.to(dev)
    live = torch.full((1,), n, dtype=torch.long, device=dev)
    counts = torch.empty(bs, dtype=torch.long, device=dev)
    masks = {"alive_zero": torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev), "alive_percent": retired_words(gone, n).to(dev)}
    lib, outputs, calls = _lib.lib, {}, {}
    for name in ("live", "alive_zero", "alive_percent"):
        ptr = torch.empty(bs + 1, dtype=torch.long, device=dev)
        index = torch.empty(bs * n, dtype=torch.long, device=dev)
        args = (xd.data_ptr(), bs, n, counts.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs * n, live.data_ptr())
        if name == "live":
            calls[name] = lambda args=args: _lib.check(lib.ultra_nonzero_lists_live(*(args + (_lib.stream_of(xd),))))
        else:
            calls[name] = lambda args=args, words=masks[name]: _lib.check(
                lib.ultra_nonzero_lists_alive(*(args + (words.data_ptr(), _lib.stream_of(xd)))))
        outputs[name] = (ptr, index)
    stats = timed([graphed(fn) for fn in calls.values()], reps, warmup)
    torch.cuda.synchronize()
    keep = torch.ones(n, dtype=torch.bool)
    keep[gone] = False
    cols = keep.nonzero().flatten()
    _, at = (x[:, cols] != 0).nonzero().t()
    total = int(outputs["alive_percent"][0][-1])
    assert total == len(at) and torch.equal(outputs["alive_percent"][1][:total].cpu(), cols[at]), "the lists differ from torch.nonzero"
    assert torch.equal(outputs["alive_zero"][0], outputs["live"][0]) and int(outputs["live"][0][-1]) == total + bs * len(gone)
    out = dict(batch=bs, N=n, retired_percent=len(gone), listed_live=total + bs * len(gone), listed_alive=total)
    for name, (med, low, high) in zip(calls, stats):
        out[name] = dict(ms=round(med, 4), ms_min=round(low, 4), ms_max=round(high, 4))
    return out


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
    anchors = torch.tensor([q[0] for q in queries], device=dev)
    n = int(data.num_nodes)
    out = dict(tool="query_retire_bench", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k)
    victims, deg = median_entities(data, 64 + 2 * fact_reps, anchors)
    in_degree = torch.bincount(data.edge_index[0], minlength=n)

    def caches_cleared():
        rspmm.clear_plan_cache()
        ultraquery.clear_csr_cache()

    # (a) from a retirement to the first answers without the entity: the three routes, in turn, in every repetition
    live_first, live_next, rebuild, cases = [], [], [], []
    for rep in range(fact_reps):
        first, second = victims[64 + 2 * rep:64 + 2 * rep + 1], victims[64 + 2 * rep + 1:64 + 2 * rep + 2]
        live = query_predict.QueryPredictor(model, data, k=k, batch_size=bs)
        live.answers(queries)                                      # serving: plan and CSR exist
        took = []
        live_first.append(wall_ms(lambda: (took.append(live.retire_entities(first)), live.answers(queries))))
        touched = live.delta.rows[:int(live.delta.count)].long()
        cases.append(dict(entity=int(first), degree=int(deg[first]), facts=int(took[0]), touched_rows=len(touched),
                          longest_touched_row=int(in_degree[touched].max())))
        holder = query_predict.QueryPredictor(model, data, k=k, batch_size=bs)      # (the state the rebuild starts from)
        holder.retire_entities(first)
        live_next.append(wall_ms(lambda: (live.retire_entities(second), live.answers(queries))))
        got = live.answers(queries)[0]
        assert live.num_retired == 2 and live.graph is data and not bool(torch.isin(got, live.retired_entities).any())
        del live
        caches_cleared()

        def rebuilt():
            query_predict.QueryPredictor(model, holder.materialized(), k=k, batch_size=bs).answers(queries)
        rebuild.append(wall_ms(rebuilt))
        del holder
        caches_cleared()
    med = statistics.median
    out["retirement_to_answers"] = dict(entities=1, reps=fact_reps, live_first=spread(live_first), live_next=spread(live_next),
                                        rebuild=spread(rebuild), rebuild_over_live_next=round(med(rebuild) / med(live_next), 2),
                                        rebuild_over_live_first=round(med(rebuild) / med(live_first), 2), cases=cases)

    # (b) the steady state: what the tombstones cost and what the mask costs on top
    served = {"static": query_predict.QueryPredictor(model, data, k=k, batch_size=bs),
              "static_again": query_predict.QueryPredictor(model, data, k=k, batch_size=bs)}
    for count in (1, 64):
        retired = query_predict.QueryPredictor(model, data, k=k, batch_size=bs, delta_capacity=8192)
        facts = int(retired.retire_entities(victims[:count]).sum())
        tombs = query_predict.QueryPredictor(model, data, k=k, batch_size=bs, delta_capacity=8192)
        tombs.remove_facts(*facts_at(data, victims[:count]))
        assert retired.graph is data and tombs.graph is data and retired.delta.num_removed == tombs.delta.num_removed > 0
        assert retired.num_retired == count and tombs.num_retired == 0
        served["retired_%d" % count], served["tombstones_%d" % count] = retired, tombs
        rows = retired.delta.rows[:int(retired.delta.count)].long()
        out["retired_%d" % count] = dict(facts=facts, tombstone_keys=retired.delta.num_removed, touched_rows=len(rows),
                                         longest_touched_row=int(in_degree[rows].max()))
    stats = timed([lambda qp=qp: qp.answers(queries) for qp in served.values()], reps, warmup)
    out["answers_ms"] = {key: dict(ms=round(s[0], 4), ms_min=round(s[1], 4), ms_max=round(s[2], 4)) for key, s in zip(served, stats)}
    by = dict(zip(served, stats))
    out["static_spread_ms"] = round(abs(by["static"][0] - by["static_again"][0]), 4)
    out["mask_ms"] = {str(c): round(by["retired_%d" % c][0] - by["tombstones_%d" % c][0], 4) for c in (1, 64)}
    out["tombstones_ms"] = {str(c): round(by["tombstones_%d" % c][0] - by["static"][0], 4) for c in (1, 64)}
    for count in (1, 64):
        qp = served["retired_%d" % count]
        assert not bool(torch.isin(qp.answers(queries)[0], qp.retired_entities).any())
    del served
    caches_cleared()

    # (c) the list call alone
    out["lists_ms"] = lists_case(n, bs, reps, warmup, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_retire_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/query_retire_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
