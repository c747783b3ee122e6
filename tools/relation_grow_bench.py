"""Timing of serving a growing VOCABULARY (ultra_amd.predict.Predictor.add_relations) on one GPU:

    python tools/relation_grow_bench.py [--reps 30] [--warmup 5] [--shapes fb15k237,yago310] [--out profiles/relation_grow_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, ultra_3g weights, batch 8, tail queries.  Every
route is measured in the same run.

  (a) relation_to_answer wall-clock milliseconds from "one new relation and four facts through it" to the answers of the next
                         tails() call (one of its queries asks the new relation), host work included (time.perf_counter around
                         the calls, the device synchronised before and after; median and min..max of --fact-reps), on a
                         Predictor(relation_capacity=16):
                           live_first_ms    they are the predictor's first edits
                           live_next_ms     the predictor already holds edits (the relation before this one and its facts)
                           rebuild_ms       the route without a reserve: a new Data of R + 1 relations with the inverse types
                                            renumbered and the concatenated edge list, its relation graph, a new Predictor, its
                                            first tails() (plan, upload, capture)
  (b) step_ms            the captured predict step by device events, run alternately, nothing added: relation_capacity 0 (the
                         static step, captured TWICE -- the difference of the two and their quartiles are the run-to-run spread
                         the reserve's cost is read against), 16 and 64
  (c) add_facts_ms       wall clock of add_facts of 16 facts between established entities and relations that leave the relation
                         graph unchanged (copies of edges the graph holds), to its return: the relation graph kept current from
                         the delta's edges against the delta forced to the rebuild from the whole edge list
  (d) kernel_ms          ultra_relation_graph_add_edges for 32 and 2,048 edges against ultra_relation_graph_bits over the full
                         list (its buffers zeroed in the same replay, as the rebuild must), each a captured call
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
from ultra_amd import _lib, models, predict, rspmm, synthetic, tasks  # noqa: E402
from ultra_amd.data import Data  # noqa: E402
from ultra_amd.live import with_relation_slots  # noqa: E402


def facts_through(relation, n, seed, dev):
    """Four facts through `relation` between entities drawn among the n ids."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, n, (4,), generator=g).to(dev), torch.full((4,), relation, device=dev),
            torch.randint(0, n, (4,), generator=g).to(dev))


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def arrival_case(model, data, h, r, k, bs, fact_reps, dev):
    n, direct = int(data.num_nodes), int(data.num_relations) // 2
    live_first, live_next, rebuild = [], [], []
    for rep in range(fact_reps):
        live = predict.Predictor(model, data, k=k, batch_size=bs, relation_capacity=16)
        live.tails(h, r)                                           # serving: plan and capture exist

        def arrive(seed):
            (new,) = live.add_relations(1).tolist()
            live.add_facts(*facts_through(new, n, seed, dev))
            live.tails(h, torch.cat([r[:-1], r.new_tensor([new])]))
        live_first.append(wall_ms(lambda: arrive(100 + rep)))
        live_next.append(wall_ms(lambda: arrive(200 + rep)))
        assert live.num_direct_relations == direct + 2 and len(live.delta) == 8 and live.num_relation_slots == direct + 16
        live.close()

        def rebuilt():
            fh, fr, ft = facts_through(direct, n, 100 + rep, dev)
            fresh = with_relation_slots(data, direct + 1, direct, relation_graph=False)
            fresh.edge_index = torch.cat([fresh.edge_index, torch.stack([torch.cat([fh, ft]), torch.cat([ft, fh])])], dim=1)
            fresh.edge_type = torch.cat([fresh.edge_type, fr, fr + direct + 1])
            tasks.build_relation_graph(fresh)
            served = predict.Predictor(model, fresh, k=k, batch_size=bs)
            served.tails(h, torch.cat([r[:-1], r.new_tensor([direct])]))
            served.close()
        rebuild.append(wall_ms(rebuilt))
        rspmm.clear_plan_cache()
    return dict(relations=1, facts=4, reps=fact_reps, reserve=16, live_first_ms=spread(live_first), live_next_ms=spread(live_next),
                rebuild_ms=spread(rebuild),
                rebuild_over_live_first=round(statistics.median(rebuild) / statistics.median(live_first), 1),
                rebuild_over_live_next=round(statistics.median(rebuild) / statistics.median(live_next), 1))


def step_case(model, data, h, r, k, bs, reps, warmup, dev):
    direct = int(data.num_relations) // 2
    ptr, index = predict.known_answers(data, h, r, "tail")
    ptr, index = ptr.contiguous(), index.contiguous()
    steps, keep = {}, []
    for key, reserve in (("0", 0), ("0_again", 0), ("16", 16), ("64", 64)):
        served = with_relation_slots(data, direct + reserve, direct) if reserve else data
        keep.append(served)
        steps[key] = predict._GraphedPredictStep(model, served, bs, k, "tail", 1 << 16)
        steps[key].load_index(index)
    stats = timed([lambda s=step: s(h, r, ptr) for step in steps.values()], reps, warmup)
    out = dict(step_ms={key: round(s[0], 4) for key, s in zip(steps, stats)},
               step_ms_min={key: round(s[1], 4) for key, s in zip(steps, stats)},
               step_ms_quartiles={key: [round(s[2], 4), round(s[3], 4)] for key, s in zip(steps, stats)},
               step_over_static={key: round(s[0] / stats[0][0], 4) for key, s in zip(steps, stats)},
               static_spread_ms=round(abs(stats[0][0] - stats[1][0]), 4))
    want = [t.clone() for t in steps["0"](h, r, ptr)]
    for key in ("16", "64"):       # (the reserve changes no answer: the same ids, the same bits)
        got = steps[key](h, r, ptr)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), key
    for step in steps.values():
        step.release()
    return out


def add_facts_case(model, data, k, bs, reps, dev):
    """16 copies of edges the graph holds per call: the relation graph cannot change."""
    e, direct = int(data.edge_index.shape[1]), int(data.num_relations) // 2
    out = {}
    for key, full in (("incremental_ms", False), ("full_rebuild_ms", True)):
        live = predict.Predictor(model, data, k=k, batch_size=bs, delta_capacity=16 * (reps + 2))
        live.delta._full_rebuild = full
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
        assert (live.delta._resident is None) == full
        out[key] = spread(times)
        live.close()
    out["full_over_incremental"] = round(out["full_rebuild_ms"]["median"] / out["incremental_ms"]["median"], 2)
    return dict(facts=16, reps=reps, **out)


def kernel_case(data, reps, warmup, dev):
    n, rels, e = int(data.num_nodes), int(data.num_relations), int(data.edge_index.shape[1])
    adj, counts, hbits, tbits = tasks.relation_graph_bits(data, incidence=True)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    ei, et = data.edge_index.contiguous(), data.edge_type.contiguous()
    lib, fns = _lib.lib, {}
    g = torch.Generator().manual_seed(3)
    keep = []
    for m in (32, 2048):        # (edges of the list itself: every OR is skipped, as for established relations)
        at = torch.randint(0, e, (m,), generator=g).to(dev)
        sub_i, sub_t = ei[:, at].contiguous(), et[at].contiguous()
        keep.append((sub_i, sub_t))
        fns["add_edges_%d" % m] = lambda sub_i=sub_i, sub_t=sub_t, m=m: _lib.check(lib.ultra_relation_graph_add_edges(
            sub_i.data_ptr(), sub_t.data_ptr(), m, n, rels, hbits.data_ptr(), tbits.data_ptr(), adj.data_ptr(), counts.data_ptr(),
            changed.data_ptr(), _lib.stream_of(dev)))
    f_adj, f_counts, f_h, f_t = torch.zeros_like(adj), torch.zeros_like(counts), torch.zeros_like(hbits), torch.zeros_like(tbits)

    def full():
        f_adj.mul_(0), f_h.mul_(0), f_t.mul_(0)      # (kernels, not memset nodes, in the captured call)
        _lib.check(lib.ultra_relation_graph_bits(ei.data_ptr(), et.data_ptr(), e, n, rels, f_h.data_ptr(), f_t.data_ptr(),
                                                 f_adj.data_ptr(), f_counts.data_ptr(), _lib.stream_of(dev)))
    fns["bits_full_list"] = full
    stats = timed([graphed(fn) for fn in fns.values()], reps, warmup)
    assert int(changed) == 0 and torch.equal(adj, f_adj)
    out = {name: dict(ms=round(s[0], 4), ms_min=round(s[1], 4), q1=round(s[2], 4), q3=round(s[3], 4)) for name, s in zip(fns, stats)}
    return dict(bit_set_bytes=2 * hbits.numel() * 4, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fact-reps", type=int, default=5)
    ap.add_argument("--add-reps", type=int, default=10)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation_grow_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/relation_grow_bench.py needs a GPU")
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
        head = dict(tool="relation_grow_bench", shape=name, batch=args.batch, N=int(data.num_nodes),
                    E=int(data.edge_index.shape[1]), R=int(data.num_relations) // 2, k=args.k)
        cases = (("relation_to_answer", lambda: arrival_case(model, data, h, r, args.k, args.batch, args.fact_reps, dev)),
                 ("step", lambda: step_case(model, data, h, r, args.k, args.batch, args.reps, args.warmup, dev)),
                 ("add_facts", lambda: add_facts_case(model, data, args.k, args.batch, args.add_reps, dev)),
                 ("kernel", lambda: kernel_case(data, args.reps, args.warmup, dev)))
        for measurement, run in cases:
            line = json.dumps(dict(head, measurement=measurement, **run()))
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
