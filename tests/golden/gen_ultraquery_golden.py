"""Generate the committed golden vectors of complex logical query answering by RUNNING THE REFERENCE in this container.

    python tests/golden/gen_ultraquery_golden.py

Like gen_golden.py and gen_explain_golden.py: needs /root/reference and runs the unchanged reference modules
(ultra.ultraquery, ultra.query_utils, ultra.models) on CPU under the test-only shim in tests/golden/pyg_shim/.  The query
modules import a few names the shim lacks; they are added here, in this process only (torch_scatter's scatter_max with its
zero for empty rows, scatter_mean, torch_scatter.composite, Batch.from_data_list, InMemoryDataset / download_url stubs).
Output: ultraquery.pt.xz (a torch.save'd dict, xz-compressed; committed), holding

  weights     ultraquery.pth["model"] (the reference checkpoint, fp32)
  graph       a 200-node KG with inverse relations (synthetic.make_kg) and its relation graph; the training graph of the
              queries (query_data.sample_queries: 90 % of the triples)
  batch       28 queries, two of each of the 14 BetaE types, postfix-encoded by the reference's Query.from_nested, with their
              types, easy and hard answer masks and the nested tuples
  executor    for each logic (product, godel, lukasiewicz) and symbolic_traversal on / off: UltraQuery's final probabilities
              and logits, and with traversal on the final symbolic stack and its stack pointers
  traversal   SymbolicTraversal on random sparse fuzzy sets (repeated relations, relations without edges)
  ranking     batch_evaluate on the model's logits, and on random tie-free logits with varied answer counts (zero easy
              answers, hundreds of answers) with and without restrict_nodes; `tied` marks hard answers whose score ties
              another node's (there the reference's ranks depend on its unstable argsort)
  metrics     evaluate() on the model logits' results after gather_results at world size 1 (which truncates num_pred to
              int64), as script/run_query.py:test() reports them: mrr, hits@1/3/10, mape, spearmanr, auroc
"""
import io
import lzma
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "pyg_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

METRICS = ["mrr", "hits@1", "hits@3", "hits@10", "mape", "spearmanr", "auroc"]


def _extend_shim():
    import torch_geometric
    import torch_geometric.data as pyg_data
    import torch_scatter

    def scatter_max(src, index, dim=-1, out=None, dim_size=None):
        dim = dim % src.dim()
        if index.dim() == 1 and src.dim() > 1:
            shape = [1] * src.dim()
            shape[dim] = -1
            index = index.view(shape).expand_as(src)
        if dim_size is None:
            dim_size = int(index.max()) + 1 if index.numel() else 0
        shape = list(src.shape)
        shape[dim] = dim_size
        res = torch.zeros(shape, dtype=src.dtype, device=src.device)
        res = res.scatter_reduce(dim, index, src, reduce="amax", include_self=False)     # empty rows stay 0
        return res, None

    def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
        return torch_scatter.scatter(src, index, dim=dim, dim_size=dim_size, reduce="mean")

    torch_scatter.scatter_max = scatter_max
    torch_scatter.scatter_mean = scatter_mean
    composite = types.ModuleType("torch_scatter.composite")
    composite.scatter_log_softmax = composite.scatter_softmax = None
    sys.modules["torch_scatter.composite"] = composite
    torch_scatter.composite = composite

    class Batch(pyg_data.Data):
        @classmethod
        def from_data_list(cls, data_list):
            offset, parts = 0, []
            for d in data_list:
                parts.append(d.edge_index + offset)
                offset += d.num_nodes
            return cls(edge_index=torch.cat(parts, dim=1), num_nodes=offset)

    pyg_data.Batch = Batch
    pyg_data.InMemoryDataset = object
    pyg_data.download_url = pyg_data.extract_zip = None
    torch_geometric.data = pyg_data


def main():
    _extend_shim()
    from torch_geometric.data import Data
    from ultra import datasets_query  # noqa: F401  (first, as script/run_query.py: query_utils and it import each other)
    from ultra import query_utils, tasks as ref_tasks
    from ultra.models import Ultra
    from ultra.ultraquery import SymbolicTraversal, UltraQuery
    from ultra_amd import query_data, synthetic

    torch.manual_seed(0)
    kg = synthetic.make_kg(num_node=200, num_triple=1600, num_relation_base=6, seed=17, relation_graph=False)
    train, ds = query_data.sample_queries(kg, 2, seed=5)
    graph = ref_tasks.build_relation_graph(Data(edge_index=train.edge_index, edge_type=train.edge_type,
                                                num_nodes=train.num_nodes, num_relations=train.num_relations))
    items = [ds[i] for i in range(len(ds))]
    query = query_utils.Query(torch.stack([it["query"] for it in items]))
    type_ = torch.tensor([it["type"] for it in items])
    easy = torch.stack([it["easy_answer"] for it in items])
    hard = torch.stack([it["hard_answer"] for it in items])

    cfg = synthetic.default_model_cfg()
    ent_cfg = dict(cfg["entity_model_cfg"])
    ent_cfg["class"] = "QueryNBFNet"
    weights = torch.load(os.path.join(REF, "ckpts", "ultraquery.pth"), map_location="cpu")["model"]
    out = dict(weights=weights, id2type=ds.id2type, num_nodes=graph.num_nodes, num_relations=graph.num_relations,
               edge_index=graph.edge_index, edge_type=graph.edge_type, rel_edge_index=graph.relation_graph.edge_index,
               rel_edge_type=graph.relation_graph.edge_type, query=query.as_subclass(torch.Tensor), type=type_,
               easy_answer=easy, hard_answer=hard, executor={}, nested=ds.nested,
               reference_postfix=[query_utils.Query.from_nested(q).tolist() for q in ds.nested])
    with torch.no_grad():
        for logic in ("product", "godel", "lukasiewicz"):
            model = UltraQuery(Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(ent_cfg)), logic=logic)
            model.load_state_dict(weights)
            model.eval()
            for sym in (True, False):
                logit = model(graph, query, symbolic_traversal=sym)
                rec = dict(prob=model.stack.stack[torch.arange(len(query)), model.stack.SP].clone(), logit=logit)
                if sym:
                    rec["symbolic_stack"] = model.symbolic_stack.stack.clone()
                    rec["symbolic_sp"] = model.symbolic_stack.SP.clone()
                out["executor"][(logic, sym)] = rec
                print(logic, sym, float(rec["prob"].min()), float(rec["prob"].max()))

        # SymbolicTraversal on random sparse fuzzy sets
        g = torch.Generator().manual_seed(3)
        n = graph.num_nodes
        h = torch.rand(10, n, generator=g) * (torch.rand(10, n, generator=g) < 0.2)
        r = torch.tensor([0, 3, 3, 7, 11, 1, 5, 5, 2, 9])
        out["traversal"] = dict(h=h, r_index=r, t=SymbolicTraversal()(graph, h, r),
                                t64=SymbolicTraversal()(graph, h.double(), r))

    # batch_evaluate / evaluate
    def ranking_case(pred, easy_, hard_, limit=None):
        ranking, answer_ranking = query_utils.batch_evaluate(pred.clone(), (None, easy_, hard_), limit)
        p = pred.clone()
        if limit is not None:
            keep = torch.zeros(p.shape[1], dtype=torch.bool)
            keep[limit] = True
            p[:, ~keep] = float("-inf")
        tied = []
        for b in range(p.shape[0]):
            for a in hard_[b].nonzero().flatten().tolist():
                tied.append(bool(((p[b] == p[b, a]).sum() > 1).item()))
        return dict(pred=pred, easy_answer=easy_, hard_answer=hard_, limit_nodes=limit, ranking=ranking,
                    answer_ranking=answer_ranking, tied=torch.tensor(tied, dtype=torch.bool))

    logit = out["executor"][("product", False)]["logit"]
    cases = {"model": ranking_case(logit, easy, hard)}
    g = torch.Generator().manual_seed(11)
    B, N = 12, 1000
    pred = torch.randperm(B * N, generator=g).float().view(B, N) / 7.0 - 500.0          # distinct values: no ties
    counts = [0, 1, 3, 17, 60, 250, 600, 5, 2, 40, 900, 12]
    e_r, h_r = torch.zeros(B, N, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)
    for b, c in enumerate(counts):
        ids = torch.randperm(N, generator=g)[: c + 1 + b % 4]
        h_r[b, ids[: 1 + b % 4]] = True
        e_r[b, ids[1 + b % 4:]] = True
    cases["random"] = ranking_case(pred, e_r, h_r)
    limit = torch.randperm(N, generator=g)[:700].sort().values
    cases["random_restricted"] = ranking_case(pred, e_r, h_r, limit)
    out["ranking"] = cases

    prob = torch.sigmoid(logit)
    num_pred = (prob * (prob > 0.5)).sum(dim=-1)
    c = cases["model"]
    # through gather_results at world size 1, as script/run_query.py:test() does: it returns num_pred as int64
    pred_t, target_t = query_utils.gather_results((c["ranking"], num_pred),
                                                  (type_, c["answer_ranking"], easy.sum(-1), hard.sum(-1)),
                                                  0, 1, torch.device("cpu"))
    out["metrics"] = query_utils.evaluate(pred_t, target_t, METRICS, ds.id2type)
    out["num_pred"] = num_pred                  # before the gather (float)
    out["gathered_num_pred"] = pred_t[1]        # after it (int64)
    print({k: round(v, 4) for k, v in out["metrics"].items() if "[" not in k})
    print("tied hard answers: model %d / %d, random %d, restricted %d" % (int(c["tied"].sum()), len(c["tied"]),
          int(cases["random"]["tied"].sum()), int(cases["random_restricted"]["tied"].sum())))

    buf = io.BytesIO()
    torch.save(out, buf)
    path = os.path.join(HERE, "ultraquery.pt.xz")
    with open(path, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
