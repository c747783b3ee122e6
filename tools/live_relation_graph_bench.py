"""Timing of a relation graph kept current IN PLACE (Predictor(live_relation_graph=True)) on one GPU:

    python tools/live_relation_graph_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310]
                                              [--out profiles/live_relation_graph_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries,
relation_capacity 16.  The flag-off and the flag-on route are measured in the same process, one after the other per repetition.

  relation_to_answer  tools/relation_grow_bench.py's case (a) -- wall-clock milliseconds from "one new relation and four facts
                      through it" to the answers of the next tails() call, host work included -- per route:
                        first_ms   they are the predictor's first edits (both routes record their step here)
                        next_ms    the predictor already holds edits: the flag-off route plans the new relation graph and records
                                   the step again, the flag-on route rewrites the byte adjacency and replays
  add_facts           its case (c): wall clock of add_facts of 16 facts that leave the relation graph unchanged, per route
  step                the captured predict step by device events with no edit pending beyond the one fact that installs the
                      delta's route, the two routes' steps replayed alternately: what reading the adjacency as an operand and
                      the new layer-0 launch cost or save per query
  layer0              ultra_nbf_dense_layer0_adjacency against ultra_nbf_layer0 on the relation graph of the shape (over its
                      2 (R + 16) slots), batch 8, each a captured call, by device events
One JSON line per shape and measurement, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from grow_bench import graphed, timed, wall_ms  # noqa: E402
from relation_grow_bench import facts_through, spread  # noqa: E402
from ultra_amd import models, predict, rspmm, synthetic, tasks  # noqa: E402
from ultra_amd.live import with_relation_slots  # noqa: E402

RESERVE = 16


def arrival_case(model, data, h, r, k, bs, fact_reps, dev):
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    times = {(flag, which): [] for flag in (False, True) for which in ("first", "next")}
    for rep in range(fact_reps):
        for flag in (False, True):
            live = predict.Predictor(model, data, k=k, batch_size=bs, relation_capacity=RESERVE, live_relation_graph=flag)
            live.tails(h, r)                                           # serving: plan and capture exist

            def arrive(seed):
                (new,) = live.add_relations(1).tolist()
                live.add_facts(*facts_through(new, n, seed, dev))
                live.tails(h, torch.cat([r[:-1], r.new_tensor([new])]))
            times[(flag, "first")].append(wall_ms(lambda: arrive(100 + rep)))
            graph, steps = live.delta.relation_graph, dict(live._steps)
            times[(flag, "next")].append(wall_ms(lambda: arrive(200 + rep)))
            assert live.num_direct_relations == direct + 2 and len(live.delta) == 8
            # (what the flag is about: the object and the captured step survive the second relation's cells)
            assert (live.delta.relation_graph is graph and live._steps["tail"] is steps["tail"]) == flag
            live.close()
            rspmm.clear_plan_cache()
    out = {"%s_%s_ms" % ("in_place" if flag else "flag_off", which): spread(v) for (flag, which), v in times.items()}
    for which in ("first", "next"):
        out["flag_off_over_in_place_" + which] = round(out["flag_off_%s_ms" % which]["median"]
                                                       / out["in_place_%s_ms" % which]["median"], 2)
    return dict(relations=1, facts=4, reps=fact_reps, reserve=RESERVE, **out)


def add_facts_case(model, data, k, bs, reps, dev):
    """16 copies of edges the graph holds per call: the relation graph cannot change."""
    e, direct = int(data.edge_index.shape[1]), int(data.num_relations) // 2
    out = {}
    for key, flag in (("flag_off_ms", False), ("in_place_ms", True)):
        live = predict.Predictor(model, data, k=k, batch_size=bs, delta_capacity=16 * (reps + 2), relation_capacity=RESERVE,
                                 live_relation_graph=flag)
        g = torch.Generator().manual_seed(11)
        times = []
        for rep in range(reps + 1):
            at = torch.randint(0, e, (64,), generator=g).to(dev)
            at = at[data.edge_type[at] < direct][:16]
            assert len(at) == 16
            fh, ft, fr = data.edge_index[0, at], data.edge_index[1, at], data.edge_type[at]
            graph = live.delta.relation_graph
            ms = wall_ms(lambda: live.add_facts(fh, fr, ft))
            assert rep == 0 or live.delta.relation_graph is graph
            if rep:        # (the first call seeds the resident state)
                times.append(ms)
        assert isinstance(live.delta.relation_graph, tasks.LiveRelationGraph) == flag
        out[key] = spread(times)
        live.close()
    return dict(facts=16, reps=reps, **out)


def step_case(model, data, h, r, k, bs, reps, warmup, dev):
    replays, keep, answers = {}, [], {}
    e0 = (int(data.edge_index[0, 0]), int(data.edge_type[0]), int(data.edge_index[1, 0]))       # (a fact the graph holds)
    assert e0[1] < int(data.num_relations) // 2
    for key, flag in (("flag_off", False), ("in_place", True), ("flag_off_again", False)):
        live = predict.Predictor(model, data, k=k, batch_size=bs, relation_capacity=RESERVE, live_relation_graph=flag)
        live.add_facts(*e0)
        answers[key] = [t.clone() for t in live.tails(h, r)]
        assert isinstance(live.delta.relation_graph, tasks.LiveRelationGraph) == flag
        keep.append(live)
        replays[key] = live._steps["tail"].graph.replay
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(answers["flag_off"], answers["in_place"]))
    stats = timed(list(replays.values()), reps, warmup)
    out = dict(step_ms={key: round(s[0], 4) for key, s in zip(replays, stats)},
               step_ms_min={key: round(s[1], 4) for key, s in zip(replays, stats)},
               step_ms_quartiles={key: [round(s[2], 4), round(s[3], 4)] for key, s in zip(replays, stats)},
               flag_off_spread_ms=round(abs(stats[0][0] - stats[2][0]), 4))
    for live in keep:
        live.close()
    return out


def layer0_case(model, data, bs, reps, warmup, dev):
    direct = int(data.num_relations) // 2
    rg = with_relation_slots(data, direct + RESERVE, direct).relation_graph
    n = int(rg.num_nodes)
    a_ex = tasks.relation_graph_dense_adjacency(rg.adjacency_bits)
    plan = rspmm.get_plan(rg.edge_index, rg.edge_type, n, 4)
    layer = model.relation_model.layers[0]
    relation = layer.relation.weight.detach().expand(bs, -1, -1)
    src = (torch.arange(bs, device=dev) * 37) % (2 * direct)
    ones = torch.ones(bs, 64, device=dev)
    args = dict(layer_norm=layer.layer_norm, relu=True, residual=True)
    fns = {"plan_layer0": lambda: plan.layer0(relation, src, ones, layer.linear, **args),
           "adjacency_layer0": lambda: rspmm.dense_layer0_adjacency(a_ex, n, relation, src, ones, layer.linear, **args)}
    with torch.no_grad():
        want, got = fns["plan_layer0"](), fns["adjacency_layer0"]()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        stats = timed([graphed(fn) for fn in fns.values()], reps, warmup)
    out = {name: dict(ms=round(s[0], 4), ms_min=round(s[1], 4), q1=round(s[2], 4), q3=round(s[3], 4)) for name, s in zip(fns, stats)}
    return dict(relation_graph_nodes=n, relation_graph_edges=int(rg.edge_index.shape[1]), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=5)
    ap.add_argument("--add-reps", type=int, default=10)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_relation_graph_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/live_relation_graph_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.shapes.split(","):
        data = synthetic.to_device(synthetic.make_kg(**synthetic.SHAPES[name], seed=1234), dev)
        tasks.build_relation_graph(data)
        triples = data.target_triples[:args.batch].contiguous()
        h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
        head = dict(tool="live_relation_graph_bench", shape=name, batch=args.batch, N=int(data.num_nodes),
                    E=int(data.edge_index.shape[1]), R=int(data.num_relations) // 2, k=args.k)
        cases = (("relation_to_answer", lambda: arrival_case(model, data, h, r, args.k, args.batch, args.fact_reps, dev)),
                 ("add_facts", lambda: add_facts_case(model, data, args.k, args.batch, args.add_reps, dev)),
                 ("step", lambda: step_case(model, data, h, r, args.k, args.batch, args.reps, args.warmup, dev)),
                 ("layer0", lambda: layer0_case(model, data, args.batch, args.reps, args.warmup, dev)))
        for measurement, run in cases:
            line = json.dumps(dict(head, measurement=measurement, **run()))
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
