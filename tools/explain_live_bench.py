"""Timing of explaining answers on a CHANGING graph (Predictor.add_facts -> explain_tails) on one GPU:

    python tools/explain_live_bench.py [--reps 5] [--shapes fb15k237,yago310] [-k 3] [--out profiles/explain_live_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, one query, its k answers
explained.  Wall-clock milliseconds (time.perf_counter, the device synchronised before and after), host work included, on a
predictor that has served and explained before (plans, CSR and captures of the base graph exist):

  fact_ms          add_facts of ONE fact, tails, then the first explanations of the k answers:
                     live      explain_tails(compact=False): the delta stays a delta
                     compact   explain_tails(compact=True): the edits are folded in first (a host plan of the materialised
                               graph, its relation graph, new captures) -- the route of a checkout without compact=False
  retract_ms       the same after 16 retractions on a predictor that already holds the fact
  explain_only_ms  the explanations alone, second call on the same state (live: the delta still held; compact: nothing left to fold)
Medians of --reps with min .. max.  One JSON line per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ultra_amd import models, predict, rspmm, synthetic, tasks  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def random_facts(data, count, seed, dev):
    g = torch.Generator().manual_seed(seed)
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    return (torch.randint(0, n, (count,), generator=g).to(dev), torch.randint(0, direct, (count,), generator=g).to(dev),
            torch.randint(0, n, (count,), generator=g).to(dev))


def stated_facts(data, count, seed, dev):
    direct = (data.edge_type < data.num_relations // 2).nonzero().flatten()
    pick = direct[torch.randperm(len(direct), generator=torch.Generator().manual_seed(seed))[:count].to(dev)]
    return data.edge_index[0, pick], data.edge_type[pick], data.edge_index[1, pick]


def shape_case(name, k, reps, dev):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    h, _, r = data.target_triples[:1].unbind(-1)
    times = {route: dict(fact=[], retract=[], explain_only=[]) for route in ("live", "compact")}
    kept = None
    for rep in range(reps):
        for route in ("live", "compact"):
            p = predict.Predictor(model, data, k=k, batch_size=1)
            p.explain_tails(h, r)                                  # serving: plans, CSR and captures of the base graph exist
            fh, fr, ft = random_facts(data, 1, 100 + rep, dev)
            fold = route == "compact"

            def state_and_explain(edit):
                edit()
                p.tails(h, r)
                p.explain_tails(h, r, compact=fold)
            times[route]["fact"].append(wall_ms(lambda: state_and_explain(lambda: p.add_facts(fh, fr, ft))))
            gone = stated_facts(p.data, 16, 200 + rep, dev)
            times[route]["retract"].append(wall_ms(lambda: state_and_explain(lambda: p.remove_facts(*gone))))
            times[route]["explain_only"].append(wall_ms(lambda: p.explain_tails(h, r, compact=fold)))
            if route == "live":
                kept = bool(p.delta is not None and p.delta.edited)
            p.close()
            rspmm.clear_plan_cache()
    out = dict(tool="explain_live_bench", shape=name, k=k, reps=reps, N=int(data.num_nodes), E=int(data.edge_index.shape[1]),
               delta_kept=kept)
    for key in ("fact", "retract", "explain_only"):
        out[key + "_ms"] = {route: spread(times[route][key]) for route in times}
        out[key + "_compact_over_live"] = round(statistics.median(times["compact"][key]) / statistics.median(times["live"][key]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--tag", default=None, help="a label stored with every line (which checkout ran)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_live_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/explain_live_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        case = shape_case(name, args.k, args.reps, dev)
        if args.tag:
            case["tag"] = args.tag
        line = json.dumps(case)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
