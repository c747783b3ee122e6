"""Timing of serving logical queries on a GROWING graph (ultra_amd.query_predict.QueryPredictor(entity_capacity=) /
add_entities) on one GPU:

    python tools/query_grow_bench.py [--reps 20] [--warmup 3] [--fact-reps 3] [--shapes fb15k237,yago310]
                                     [--out profiles/query_grow_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, the ultraquery weights of
tests/golden/ultraquery.pt.xz, batch 16, 16 satisfiable 1p and 16 satisfiable 2p queries drawn from the edge list (those of
tools/query_live_bench.py).  Everything is compared in the same run, alternately.

  (a) entity_to_answers  wall-clock milliseconds from one add_entities(1) plus four add_facts about the new entity (two with it as
                         the head, two as the tail, the other ends drawn uniformly) to the answers of the next answers() call
                         (the 32 queries: two batches), host work included, median of --fact-reps, entity_capacity=256:
                           live_first_ms  on a predictor that was never edited (the delta and its traversal layout are made)
                           live_next_ms   on a predictor that already holds edits: one more entity, four more facts
                           rebuild_ms     a new Data of N + 1 nodes with the eight edges appended, its relation graph, a new
                                          QueryPredictor and its first answers() (host plan, upload, traversal CSR)
  (b) reserve_ms         answers() of the 32 queries by device events, run alternately, median and quartiles, on predictors with
                         entity_capacity 0, 0 again (the run-to-run spread of the static case), 256 and 4,096 -- no entity added
  (c) lists              ultra_nonzero_lists over all N + 256 slots against ultra_nonzero_lists_live with N live, on the same
                         (16, N + 256) sets (1 % non-zeros among the live ids, 1.0 in every reserved slot: the final sets of
                         queries that end in a negation), both captured, device events, run alternately, median and quartiles;
                         bytes = 2 x 4 B per element read (count, fill) + 8 B per listed id + 8 B per row of counts read and
                         written + 8 B per ptr entry, and their share of 8 TB/s
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

from live_graph_bench import HBM_BPS, graphed, wall_ms  # noqa: E402
from query_live_bench import sample_queries  # noqa: E402
from ultra_amd import _lib, models, query_predict, rspmm, synthetic, tasks, ultraquery  # noqa: E402
from ultra_amd.data import Data  # noqa: E402


def timed_quartiles(fns, reps, warmup):
    """(median, first quartile, third quartile) of the device-event milliseconds of every callable, run alternately."""
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
        q1, med, q3 = statistics.quantiles(t, n=4) if len(t) > 1 else (t[0], t[0], t[0])
        out.append(dict(median=round(med, 4), q1=round(q1, 4), q3=round(q3, 4)))
    return out


def entity_facts(num_entities, new_id, num_direct, seed, dev):
    """Four facts about `new_id`: two with it as the head, two as the tail, the other ends uniform over the known entities."""
    gen = torch.Generator().manual_seed(seed)
    other = torch.randint(0, num_entities, (4,), generator=gen)
    r = torch.randint(0, num_direct, (4,), generator=gen)
    new = torch.full((2,), new_id)
    return torch.cat([new, other[2:]]).to(dev), r.to(dev), torch.cat([other[:2], new]).to(dev)


def rebuilt_graph(data, h, r, t):
    """A new Data of N + 1 nodes with the facts' edges appended and its relation graph: the route without a reserve."""
    index = torch.cat([data.edge_index, torch.stack([torch.cat([h, t]), torch.cat([t, h])])], dim=1)
    kind = torch.cat([data.edge_type, r, r + int(data.num_relations) // 2])
    fresh = Data(edge_index=index, edge_type=kind, num_nodes=int(data.num_nodes) + 1, num_relations=data.num_relations)
    return tasks.build_relation_graph(fresh)


def lists_case(n, reserve, bs, reps, warmup, dev):
    slots = n + reserve
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(bs, slots, generator=gen) * (torch.rand(bs, slots, generator=gen) < 0.01))
    x[:, n:] = 1.0
    x = x.to(dev)
    live = torch.full((1,), n, dtype=torch.long, device=dev)
    counts = torch.empty(bs, dtype=torch.long, device=dev)
    out = {}
    calls = []
    for name in ("parent", "twin"):
        ptr = torch.empty(bs + 1, dtype=torch.long, device=dev)
        index = torch.empty(bs * slots, dtype=torch.long, device=dev)
        args = (x.data_ptr(), bs, slots, counts.data_ptr(), ptr.data_ptr(), index.data_ptr(), bs * slots)
        if name == "parent":
            fn = lambda args=args: _lib.check(_lib.lib.ultra_nonzero_lists(*(args + (_lib.stream_of(x),))))
        else:
            fn = lambda args=args: _lib.check(_lib.lib.ultra_nonzero_lists_live(*(args + (live.data_ptr(), _lib.stream_of(x)))))
        calls.append(graphed(fn))
        out[name] = dict(ptr=ptr, index=index)
    stats = timed_quartiles(calls, reps, warmup)
    sample, col = (x[:, :n] != 0).nonzero().t()
    listed_live = int(out["twin"]["ptr"][-1])
    assert listed_live == len(col) and torch.equal(out["twin"]["index"][:listed_live], col), "the twin differs from torch.nonzero"
    assert int(out["parent"]["ptr"][-1]) == listed_live + bs * reserve
    result = dict(batch=bs, slots=slots, live=n)
    for name, stat, width, listed in (("parent", stats[0], slots, listed_live + bs * reserve), ("twin", stats[1], n, listed_live)):
        nbytes = 2 * 4 * bs * width + 8 * listed + 2 * 8 * bs + 8 * (bs + 1)
        result[name] = dict(ms=stat, listed=listed, bytes=nbytes, gbps=round(nbytes / (stat["median"] * 1e-3) / 1e9, 2),
                            roof=round(nbytes / (stat["median"] * 1e-3) / HBM_BPS, 6))
    return result


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
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    out = dict(tool="query_grow_bench", shape=name, batch=bs, N=n, E=int(data.edge_index.shape[1]), k=k)

    # (a) from a new entity and its facts to the first answers
    first, later, rebuild = [], [], []
    for rep in range(fact_reps):
        live = query_predict.QueryPredictor(model, data, k=k, batch_size=bs, entity_capacity=256)
        live.answers(queries)                                      # serving: plan and CSR exist

        def arrive(seed):
            (new_id,) = live.add_entities(1).tolist()
            live.add_facts(*entity_facts(n, new_id, direct, seed, dev))
            return live.answers(queries)
        first.append(wall_ms(lambda: arrive(100 + rep)))
        later.append(wall_ms(lambda: arrive(200 + rep)))
        assert live.graph.edge_index is data.edge_index and len(live.delta) == 8

        def rebuilt():
            fresh = rebuilt_graph(data, *entity_facts(n, n, direct, 100 + rep, dev))
            query_predict.QueryPredictor(model, fresh, k=k, batch_size=bs).answers(queries)
        rebuild.append(wall_ms(rebuilt))
        del live
        rspmm.clear_plan_cache()
        ultraquery.clear_csr_cache()
    med = statistics.median
    out["entity_to_answers"] = dict(entity_capacity=256, facts=4, reps=fact_reps, live_first_ms=round(med(first), 3),
                                    live_next_ms=round(med(later), 3), rebuild_ms=round(med(rebuild), 3),
                                    rebuild_over_live_first=round(med(rebuild) / med(first), 2),
                                    rebuild_over_live_next=round(med(rebuild) / med(later), 2))

    # (b) what an unused reserve costs
    order = [("0", 0), ("0_again", 0), ("256", 256), ("4096", 4096)]
    served = [query_predict.QueryPredictor(model, data, k=k, batch_size=bs, entity_capacity=m) for _, m in order]
    stats = timed_quartiles([lambda qp=qp: qp.answers(queries) for qp in served], reps, warmup)
    out["reserve_ms"] = {key: stat for (key, _), stat in zip(order, stats)}
    base = stats[0]["median"]
    out["reserve_spread_ms"] = round(abs(stats[1]["median"] - base), 4)
    out["reserve_over_static"] = {key: round(stat["median"] / base, 4) for (key, _), stat in zip(order, stats)}
    del served

    # (c) the lists alone
    out["lists"] = lists_case(n, 256, bs, reps, warmup, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_grow_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/query_grow_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
