"""Timing of RETRACTING facts from a served graph (ultra_amd.predict.Predictor.remove_facts) on one GPU:

    python tools/retract_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--out profiles/retract_bench.jsonl]
                                  [--routes split,old] [--parts abcd]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries.  The
retracted facts are triples the graph states, drawn at random.

  (a) retraction_to_answer  wall-clock milliseconds from "16 retractions" to the answers of the next tails() call, host work
                            included (time.perf_counter around the calls, the device synchronised before and after; median of
                            --fact-reps), all three routes in the same run:
                              live_first_ms   remove_facts on a predictor that held no tombstone: the step is captured again
                              live_next_ms    remove_facts on a predictor that already holds tombstones: no capture, no plan
                              rebuild_ms      the route without a delta: a new Data of the remaining edge list, its relation
                                              graph, a new Predictor, its first tails() (host plan, upload, capture)
                              masked_ms       the route DESIGN.md 17 named: the shared keep vector of ultra_leave_one_out_keep's
                                              rule (every duplicate of the edge and its inverse set to 0) built with torch, then
                                              one eager forward whose twelve walks take it (ultra_rspmm_forward_masked), then
                                              the filtered top-k -- the base graph's relation graph and plan, no capture
  (b) step_ms               the captured predict step by device events, run alternately: static (no delta), with an add-only
                            delta of 16 facts, with 16 and with 1,024 retractions; and the kernels of one replay of each, counted
                            with torch.profiler: the add-only step must launch ultra_rspmm_delta_rows' kernel and never the
                            retraction kernel, and the step with retractions as many kernels as the add-only one (asserted)
  (c) edit_rows             ultra_rspmm_edit_rows alone (a captured call) with those deltas: touched rows, base edges walked,
                            longest row, bytes (per edge a source row, a relation row and 8 bytes of indices, per row one output
                            row, times the batch), their share of 8 TB/s
  (d) length_sweep          one retracted fact whose row has about 32 .. 8,192 base edges, and the graph's longest row: the
                            16-lane walk (ultra_rspmm_edit_rows) against the hub walker (ultra_rspmm_edit_rows_split with
                            hub_len = 0: every touched row by a workgroup), captured calls run alternately
--routes: (b) and (c) once per route -- `split`: rspmm.EDIT_ROWS_HUB_SPLIT on, a touched row longer than seg_len by a workgroup
(the kernels' names end in _split_kernel); `old`: the switch off, the kernels of DESIGN.md 17 / 18, whose names the
assertions of (b) check.  The keys of the `old` route carry no suffix, those of `split` end in `_split`.
One JSON line per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from live_graph_bench import HBM_BPS, graphed, random_facts, replay_kernels, timed, wall_ms  # noqa: E402
from ultra_amd import dense, models, predict, rspmm, synthetic, tasks  # noqa: E402
from ultra_amd.data import Data  # noqa: E402


def stated_facts(data, count, seed, dev):
    """`count` distinct triples the graph states, as (h, r, t) on `dev`."""
    direct = data.edge_index.shape[1] // 2
    pick = torch.randperm(direct, generator=torch.Generator().manual_seed(seed))[:count].to(dev)
    return data.edge_index[0, pick].contiguous(), data.edge_type[pick].contiguous(), data.edge_index[1, pick].contiguous()


def edge_codes(data, row, col, edge_type):
    return (row * int(data.num_nodes) + col) * int(data.num_relations) + edge_type


def shared_keep(data, h, r, t):
    """The keep vector (E) fp32 of the graph without the facts: 0 at every edge equal to (h, t, r) or (t, h, r + R / 2)."""
    gone = torch.cat([edge_codes(data, h, t, r), edge_codes(data, t, h, r + int(data.num_relations) // 2)]).unique()
    codes = edge_codes(data, data.edge_index[0], data.edge_index[1], data.edge_type)
    dead = gone[torch.searchsorted(gone, codes).clamp_(max=len(gone) - 1)] == codes
    return (~dead).float()


def masked_forward(model, data, batch, keep):
    """Ultra.forward on the fused inference path with ONE keep vector shared by the batch: every layer's walk reads it as "edge
    absent" (ultra_rspmm_forward_masked), the relation graph stays the base graph's."""
    ent = model.entity_model
    pro = dense.batch_prologue(batch, data.num_relations // 2)
    relations = model.relation_model(data.relation_graph, query=pro.rel_first)
    ent.query = relations
    for layer in ent.layers:
        layer.relation = relations
    hiddens, _, query = ent._bellmanford_hidden(data, pro[1], pro[2], edge_weight=keep, edge_keep=True)
    return dense.readout_batch(ent, hiddens[-1], query, pro[0], pro[3]).view(batch.shape[:2])


def edit_rows_case(data, delta, bs, reps, warmup, dev, routes=("old",), hub_len=None):
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(bs, data.num_nodes, 64, generator=g).to(dev)
    rel = torch.randn(bs, data.num_relations, 64, generator=g).to(dev)
    rows = torch.zeros(bs, dtype=torch.long, device=dev)
    vals = torch.randn(bs, 64, generator=g).to(dev)
    out = plan.forward(rel, x, point=(rows, vals))
    entries = {"old": lambda: plan.edit_rows(rel, x, out, delta, point=(rows, vals)),
               "split": lambda: plan.edit_rows_split(rel, x, out, delta, point=(rows, vals), hub_len=hub_len)}
    med, low = timed([graphed(entries[route]) for route in routes], reps, warmup)
    ms, ms_min = med[0], low[0]
    touched = delta.rows[:int(delta.count)].long()
    base_degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)[touched]
    edges = int(base_degree.sum()) + 2 * len(delta)        # (dead edges are walked too: their indices are read, their rows are not)
    nbytes = bs * (edges * (256 + 256) + len(touched) * 256) + edges * 8
    line = dict(retractions=delta.num_removed // 2, keys=delta.num_removed, touched_rows=len(touched), edges_walked=edges,
                longest_row=int(base_degree.max()), route=routes[0], ms=round(ms, 4), ms_min=round(ms_min, 4), bytes=nbytes,
                gbps=round(nbytes / (ms * 1e-3) / 1e9, 1), roof=round(nbytes / (ms * 1e-3) / HBM_BPS, 4))
    for route, m, lo in list(zip(routes, med, low))[1:]:
        line.update({route + "_ms": round(m, 4), route + "_ms_min": round(lo, 4), route + "_roof": round(nbytes / (m * 1e-3) / HBM_BPS, 4)})
    return line


def length_sweep(data, bs, reps, warmup, dev):
    """(d): per target length the row of the nearest base degree loses one stated fact -- the one whose other end is the
    shortest row, which is touched too."""
    degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)
    half = int(data.num_relations) // 2
    lines = []
    for target in [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, int(degree.max())]:
        row = int((degree - target).abs().argmin())
        at = (data.edge_index[0] == row).nonzero().flatten()
        e = int(at[degree[data.edge_index[1, at]].argmin()])
        col, kind = int(data.edge_index[1, e]), int(data.edge_type[e])
        fact = (row, kind, col) if kind < half else (col, kind - half, row)
        delta = rspmm.GraphDelta(data, 1024)
        delta.remove(*fact)
        line = edit_rows_case(data, delta, bs, reps, warmup, dev, routes=("old", "split"), hub_len=0)
        line.update(target=target, row_len=int(degree[row]), other_row_len=int(degree[col]))
        lines.append(line)
    return lines


def shape_case(name, k, bs, reps, warmup, fact_reps, dev, routes=("split", "old"), parts="abcd"):
    kg = synthetic.make_kg(**synthetic.SHAPES[name], seed=1234)
    data = synthetic.to_device(kg, dev)
    tasks.build_relation_graph(data)
    model = models.Ultra(**synthetic.default_model_cfg())
    model.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "ultra_3g_model.pt")))
    model = model.to(dev).eval()
    triples = data.target_triples[:bs].contiguous()
    h, r = triples[:, 0].contiguous(), triples[:, 2].contiguous()
    out = dict(tool="retract_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]), k=k)
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()

    # (a) from retractions to the first answers without them: the three routes, in turn, in every repetition
    live_first, live_next, rebuild, masked = [], [], [], []
    for rep in range(fact_reps if "a" in parts else 0):
        facts = stated_facts(data, 32, 100 + rep, dev)
        fh, fr, ft = (f[:16] for f in facts)
        live = predict.Predictor(model, data, k=k, batch_size=bs)
        live.tails(h, r)                                           # serving: plan and capture exist
        live_first.append(wall_ms(lambda: (live.remove_facts(fh, fr, ft), live.tails(h, r))))
        live_next.append(wall_ms(lambda: (live.remove_facts(*(f[16:] for f in facts)), live.tails(h, r))))
        live.close()

        def rebuilt():
            keep = shared_keep(data, fh, fr, ft).bool()
            fresh = Data(edge_index=data.edge_index[:, keep], edge_type=data.edge_type[keep], num_nodes=data.num_nodes,
                         num_relations=data.num_relations)
            tasks.build_relation_graph(fresh)
            served = predict.Predictor(model, fresh, k=k, batch_size=bs)
            served.tails(h, r)
            served.close()
        rebuild.append(wall_ms(rebuilt))

        def masked_route():
            keep = shared_keep(data, fh, fr, ft)
            with torch.no_grad():
                score = masked_forward(model, data, predict._candidates(data, h, r, "tail"), keep).float().contiguous()
            return predict.filtered_topk(score, k, ptr, index)
        try:
            masked_route()                                         # (the base plan and the eager path are warm, as a server's are)
            masked.append(wall_ms(masked_route))
        except Exception as exc:      # (the route is a yardstick, not the product: a failure is reported, the rest is measured)
            out["masked_route_error"] = repr(exc)
        rspmm.clear_plan_cache()
    med = statistics.median
    if "a" in parts:
        out["retraction_to_answer"] = dict(retractions=16, reps=fact_reps, live_first_ms=round(med(live_first), 3),
                                           live_next_ms=round(med(live_next), 3), rebuild_ms=round(med(rebuild), 3),
                                           masked_ms=round(med(masked), 3) if masked else None,
                                           rebuild_over_live_next=round(med(rebuild) / med(live_next), 1),
                                           masked_over_live_next=round(med(masked) / med(live_next), 2) if masked else None)

    # (b) the steady-state step, per route
    deltas = {}
    for count in (16, 1024):
        deltas[count] = rspmm.GraphDelta(data, 1024)
        deltas[count].remove(*stated_facts(data, count, 7, dev))
    added = rspmm.GraphDelta(data, 1024)
    added.add(*random_facts(data, 16, 7, dev))
    quiet = rspmm.GraphDelta(data, 1024)                # 16 added facts between the rows of the fewest edges: no hub touched
    degree = torch.bincount(data.edge_index[0], minlength=data.num_nodes)
    short = degree.argsort()[:32]
    quiet.add(short[:16].contiguous(), torch.zeros(16, dtype=torch.long, device=dev), short[16:].contiguous())
    plan = rspmm.get_plan(data.edge_index, data.edge_type, data.num_nodes, data.num_relations)
    out["seg_len"], out["has_hub_rows"] = plan.info()["seg_len"], bool(plan.has_hub_rows)
    steps = {"static": predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16)}
    order = ["static"]
    for route in (routes if "b" in parts else ()):
        rspmm.EDIT_ROWS_HUB_SPLIT = route == "split"
        suffix = "_split" if route == "split" else ""
        for key, delta in (("added16_no_hub", quiet), ("added16", added), ("16", deltas[16]), ("1024", deltas[1024])):
            steps[key + suffix] = predict._GraphedPredictStep(model, data, bs, k, "tail", 1 << 16, delta=delta)
            steps[key + suffix].load_index(index)
            steps[key + suffix](h, r, ptr)              # (captured under its route's switch)
            order.append(key + suffix)
    rspmm.EDIT_ROWS_HUB_SPLIT = True
    steps["static"].load_index(index)
    if "b" in parts:
        med_ms, low = timed([lambda s=steps[key]: s(h, r, ptr) for key in order], reps, warmup)
        out["step_ms"] = {key: round(m, 4) for key, m in zip(order, med_ms)}
        out["step_ms_min"] = {key: round(m, 4) for key, m in zip(order, low)}
        out["step_over_static"] = {key: round(m / med_ms[0], 4) for key, m in zip(order, med_ms)}
        out["relation_graph_kept"] = {str(c): bool(d.relation_graph is data.relation_graph) for c, d in deltas.items()}
        try:
            kernels = {key: replay_kernels(steps[key], (h, r, ptr)) for key in order}
        except Exception as exc:      # (no profiler on this build: the count is not taken, and the line says so)
            kernels = {key: None for key in order}
            out["kernel_count_error"] = repr(exc)
        if kernels.get("added16") is not None and kernels.get("16") is not None:
            # an add-only delta keeps its kernels: ultra_rspmm_delta_rows' launches and none of the retraction kernel's; the step
            # with tombstones runs the same NUMBER of kernels, the retraction kernel in the other's place
            assert not any("edit_rows" in name for name in kernels["added16"]), "an add-only delta launches the retraction kernel"
            assert any("delta_rows" in name for name in kernels["added16"])
            assert not any("split" in name for name in kernels["added16"] + kernels["16"]), "the switch is off: the old kernels"
            assert len(kernels["16"]) == len(kernels["added16"]), (len(kernels["16"]), len(kernels["added16"]))
            assert any("edit_rows" in name for name in kernels["16"]) and not any("delta_rows" in name for name in kernels["16"])
        if kernels.get("added16_split") is not None and kernels.get("16_split") is not None and plan.has_hub_rows:
            # the split route: one launch in the other's place, the roles inside it
            assert any("delta_rows_split" in name for name in kernels["added16_split"])
            assert any("edit_rows_split" in name for name in kernels["16_split"])
            assert len(kernels["16_split"]) == len(kernels["added16_split"])
        out["kernels"] = {key: None if names is None else len(names) for key, names in kernels.items()}

    # (c) the retraction kernel alone
    if "c" in parts:
        out["edit_rows"] = [edit_rows_case(data, deltas[count], bs, reps, warmup, dev, routes=tuple(reversed(routes)))
                            for count in (16, 1024)]
    if "d" in parts:
        out["length_sweep"] = length_sweep(data, bs, reps, warmup, dev)
    for step in steps.values():
        step.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--routes", default="split,old", help="comma list of split, old: the routes (b) and (c) measure")
    ap.add_argument("--parts", default="abcd", help="the parts to run, letters of abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retract_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/retract_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev,
                                     routes=tuple(args.routes.split(",")), parts=args.parts))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
