"""Timing of serving logical queries on a CHANGING graph (ultra_amd.query_predict.QueryPredictor.add_facts / remove_facts,
DESIGN.md 20) on one GPU:

    python tools/query_live_bench.py [--reps 20] [--warmup 3] [--fact-reps 3] [--shapes fb15k237,yago310]
                                     [--out profiles/query_live_bench.jsonl]

Synthetic graphs of FB15k237's and YAGO3-10's node, edge and relation counts, the ultraquery weights of
tests/golden/ultraquery.pt.xz, batch 16, satisfiable 1p and 2p queries drawn from the edge list.  Added facts are drawn
uniformly over (entity, relation, entity); retracted facts are triples the graph states, drawn uniformly over the edges -- so
their endpoints are the graph's hubs.  Everything is compared in the same run.

  (a) traversal        one symbolic traversal (16 sets with 1 % non-zeros, random relations, the hub relation among them) with
                       16 and with 1,024 edits (half additions, half retractions), device events, run alternately: the base
                       launch alone, base launch + fix-up, and ultra_symbolic_traversal_edit_rows alone with the rows it
                       touches, the longest (tail, relation) segment among them, its bytes (per (touched tail, sample): 16 B of
                       row_ptr and 4 B written; 8 B per slot of the sample's relation scanned -- a source id and the gathered
                       value -- base and added alike) and their share of 8 TB/s.  rebuild_ms: the alternative it replaces --
                       ultraquery.symbolic_traversal on the materialised edge list with the CSR rebuilt (a sort over all E
                       edges), wall clock; the materialised list itself is given to it for free
  (b) edits_to_answers wall-clock milliseconds from 16 add_facts, and from 16 remove_facts, to the answers of the next
                       answers() call (16 1p and 16 2p queries: two batches), host work included, median of --fact-reps:
                         live_first_ms  on a predictor that was never edited (the delta and its traversal layout are made)
                         live_next_ms   on a predictor that already holds edits
                         rebuild_ms     a new Data of the edited edge list, its relation graph, a new QueryPredictor and its
                                        first answers() (host plan, upload, traversal CSR)
  (c) answers_ms       answers() of those 32 queries by device events, run alternately, on predictors that hold no delta, 16 and
                       1,024 added facts, and -- separately, because the rspmm fix-up walks a hub row as one chain
                       -- 16 and 1,024 retractions
One JSON line per shape, appended to --out.  That a predictor which was never edited costs what it cost before is measured with
tools/query_predict_bench.py on the parent commit and on this one, alternately in one session."""
import argparse
import ctypes
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

from live_graph_bench import HBM_BPS, graphed, random_facts, timed, wall_ms  # noqa: E402
from retract_bench import shared_keep, stated_facts  # noqa: E402
from ultra_amd import _lib, models, query_predict, rspmm, synthetic, tasks, ultraquery  # noqa: E402
from ultra_amd.data import Data  # noqa: E402


def sample_queries(data, count, seed):
    """`count` satisfiable 1p queries (h, (r,)) and `count` satisfiable 2p queries (h, (r1, r2)) read off the edge list."""
    gen = torch.Generator().manual_seed(seed)
    ei, et = data.edge_index.cpu(), data.edge_type.cpu()
    one, two = [], []
    for e in torch.randint(0, ei.shape[1], (count,), generator=gen).tolist():
        one.append((int(ei[0, e]), (int(et[e]),)))
    for e in torch.randint(0, ei.shape[1], (count,), generator=gen).tolist():
        into = (ei[1] == ei[0, e]).nonzero().flatten()          # an edge into the second hop's source
        if len(into) == 0:
            two.append((int(ei[0, e]), (int(et[e]), int(et[e]))))
            continue
        first = int(into[int(torch.randint(0, len(into), (1,), generator=gen))])
        two.append((int(ei[0, first]), (int(et[first]), int(et[e]))))
    return one, two


def edited_delta(data, adds, removes, seed, dev, capacity=1024):
    delta = rspmm.GraphDelta(data, capacity)
    if adds:
        delta.add(*random_facts(data, adds, seed, dev))
    if removes:
        delta.remove(*stated_facts(data, removes, seed, dev))
    return delta


def traversal_case(data, edits, bs, reps, warmup, dev):
    n, rels = int(data.num_nodes), int(data.num_relations)
    ei, et = data.edge_index, data.edge_type
    delta = edited_delta(data, edits // 2, edits // 2, 7, dev)
    gen = torch.Generator().manual_seed(2)
    h = (torch.rand(bs, n, generator=gen) * (torch.rand(bs, n, generator=gen) < 0.01)).to(dev)
    r = torch.randint(0, rels, (bs,), generator=gen)
    r[::4] = rels // 2                                              # the inverse of the most frequent relation: into the hubs
    r = r.to(dev)
    base = graphed(lambda: ultraquery.symbolic_traversal(ei, et, n, h, r))
    both = graphed(lambda: ultraquery.symbolic_traversal(ei, et, n, h, r, delta=delta))
    csr = ultraquery.traversal_csr(ei, et, n)
    t = ultraquery.symbolic_traversal(ei, et, n, h, r)
    operand = delta.traversal_operand()

    def fix_up():
        _lib.check(_lib.lib.ultra_symbolic_traversal_edit_rows(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), n,
                                                               ctypes.byref(operand), r.data_ptr(), bs, _lib.F32, h.data_ptr(),
                                                               t.data_ptr(), _lib.stream_of(h)))
    alone = graphed(fix_up)
    (base_ms, both_ms, alone_ms), (_, _, alone_min) = timed([base, both, alone], reps, warmup)
    mat = delta.materialize()
    want = ultraquery.symbolic_traversal(mat.edge_index, mat.edge_type, n, h, r)
    assert torch.equal(both.__self__.keep, want), "the fix-up differs from the traversal of the materialised graph"

    def rebuilt():
        ultraquery.clear_csr_cache()
        return ultraquery.symbolic_traversal(mat.edge_index, mat.edge_type, n, h, r)
    rebuild = statistics.median(wall_ms(rebuilt) for _ in range(3))
    ultraquery.clear_csr_cache()
    lay = delta.traversal
    touched = lay.rows[:int(lay.count)].long()
    segment = torch.bincount(ei[1] * rels + et, minlength=n * rels).view(n, rels)[touched]          # (touched, rels) base slots
    added = torch.zeros(n * rels, dtype=torch.long, device=dev)
    d_index, d_type = delta.edges()
    added.index_add_(0, d_index[1] * rels + d_type, torch.ones_like(d_type))
    slots = (segment + added.view(n, rels)[touched])[:, r].sum()
    nbytes = int(slots) * 8 + bs * len(touched) * 20
    return dict(edits=edits, added=len(delta), keys=delta.num_removed, touched_rows=len(touched),
                longest_segment=int(segment.max()), slots_scanned=int(slots), base_ms=round(base_ms, 4),
                base_plus_fix_up_ms=round(both_ms, 4), fix_up_ms=round(alone_ms, 4), fix_up_ms_min=round(alone_min, 4),
                bytes=nbytes, gbps=round(nbytes / (alone_ms * 1e-3) / 1e9, 2), roof=round(nbytes / (alone_ms * 1e-3) / HBM_BPS, 6),
                rebuild_ms=round(rebuild, 3), rebuild_over_live=round(rebuild / both_ms, 1))


def rebuilt_graph(data, added=None, removed=None):
    """A new Data of the edited edge list with its relation graph: the route without a delta."""
    index, kind = data.edge_index, data.edge_type
    if removed is not None:
        keep = shared_keep(data, *removed).bool()
        index, kind = index[:, keep], kind[keep]
    if added is not None:
        h, r, t = added
        index = torch.cat([index, torch.stack([torch.cat([h, t]), torch.cat([t, h])])], dim=1)
        kind = torch.cat([kind, r, r + int(data.num_relations) // 2])
    fresh = Data(edge_index=index, edge_type=kind, num_nodes=data.num_nodes, num_relations=data.num_relations)
    return tasks.build_relation_graph(fresh)


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
    out = dict(tool="query_live_bench", shape=name, batch=bs, N=int(data.num_nodes), E=int(data.edge_index.shape[1]), k=k)

    # (a) the traversal alone
    out["traversal"] = [traversal_case(data, edits, bs, reps, warmup, dev) for edits in (16, 1024)]

    # (b) from edits to the first answers
    result = {}
    for kind in ("add", "remove"):
        first, later, rebuild = [], [], []
        for rep in range(fact_reps):
            draw = random_facts if kind == "add" else stated_facts
            facts = draw(data, 32, 100 + rep, dev)
            head, tail = [f[:16].contiguous() for f in facts], [f[16:].contiguous() for f in facts]
            live = query_predict.QueryPredictor(model, data, k=k, batch_size=bs, delta_capacity=1024)
            live.answers(queries)                                      # serving: plan and CSR exist
            edit = live.add_facts if kind == "add" else live.remove_facts
            first.append(wall_ms(lambda: (edit(*head), live.answers(queries))))
            later.append(wall_ms(lambda: (edit(*tail), live.answers(queries))))

            def rebuilt():
                fresh = rebuilt_graph(data, **{"added" if kind == "add" else "removed": head})
                query_predict.QueryPredictor(model, fresh, k=k, batch_size=bs).answers(queries)
            rebuild.append(wall_ms(rebuilt))
            rspmm.clear_plan_cache()
            ultraquery.clear_csr_cache()
        med = statistics.median
        result[kind] = dict(edits=16, reps=fact_reps, live_first_ms=round(med(first), 3), live_next_ms=round(med(later), 3),
                            rebuild_ms=round(med(rebuild), 3), rebuild_over_live_next=round(med(rebuild) / med(later), 2))
    out["edits_to_answers"] = result

    # (c) the steady state
    states = {"static": (0, 0), "added16": (16, 0), "added1024": (1024, 0), "retracted16": (0, 16), "retracted1024": (0, 1024)}
    served = {}
    for key, (adds, removes) in states.items():
        qp = query_predict.QueryPredictor(model, data, k=k, batch_size=bs, delta_capacity=1024)
        if adds:
            qp.add_facts(*random_facts(data, adds, 7, dev))
        if removes:
            qp.remove_facts(*stated_facts(data, removes, 7, dev))
        assert qp.graph is data, "the edits fit the delta"
        served[key] = qp
    order = list(states)
    med_ms, low = timed([lambda qp=served[key]: qp.answers(queries) for key in order], reps, warmup)
    out["answers_ms"] = {key: round(m, 3) for key, m in zip(order, med_ms)}
    out["answers_ms_min"] = {key: round(m, 3) for key, m in zip(order, low)}
    out["answers_over_static"] = {key: round(m / med_ms[0], 3) for key, m in zip(order, med_ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fact-reps", type=int, default=3)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="fb15k237,yago310")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_live_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/query_live_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        line = json.dumps(shape_case(name, args.k, args.batch, args.reps, args.warmup, args.fact_reps, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
