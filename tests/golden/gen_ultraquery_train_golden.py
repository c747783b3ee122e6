"""Generate the committed golden vectors of UltraQuery TRAINING by running the reference in this container.

    python tests/golden/gen_ultraquery_train_golden.py

Like gen_ultraquery_golden.py (whose shim additions it reuses): needs /root/reference and runs the unchanged reference modules
(ultra.ultraquery, ultra.tasks, script/run_query.py) on CPU under tests/golden/pyg_shim.  A few more names are added in this
process only: torch_scatter.composite.scatter_softmax (exp(x - max) / sum per group), easydict / tqdm stubs where the packages
are missing, and recording wrappers around the reference's own edge_match, index_to_mask and predict_and_target.
Output: ultraquery_train.pt.xz (torch.save'd dict, xz-compressed; committed), holding

  graph       the training graph and relation graph of gen_ultraquery_golden.py (200 nodes, 6 + 6 relations)
  dropout     for several projections (random sparse symbolic sets, repeated relations) in both inverse conventions:
              sym, r_index, the reference's edge_match index lists (direct ++ inverse, duplicates included) and, per
              (ratio, more) in (1, 0), (0, 1), (1, 1), the kept-edge mask of UltraQuery.traversal_dropout and
              build_relation_graph of the dropped graph
  train       one batch of all 14 types (two each) through the reference's own train_and_validate (product logic,
              dropout ratio 1, adversarial temperature 0.2, SGD at lr 1 for one batch): the batch as the sampler ordered it,
              predict_and_target's logits, every parameter's gradient (= its change), and the logged loss
"""
import io
import logging
import lzma
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_ultraquery_golden as base  # noqa: E402  (sets up sys.path: shim, reference, repository)

import torch  # noqa: E402

REF = base.REF
RATIOS = ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0))


def _extend_shim():
    base._extend_shim()
    import torch_scatter

    def scatter_softmax(src, index, dim=-1):
        dim = dim % src.dim()
        size = int(index.max()) + 1 if index.numel() else 0
        mx = torch.full((size,), float("-inf"), dtype=src.dtype).scatter_reduce(0, index, src, reduce="amax", include_self=True)
        e = (src - mx[index]).exp()
        s = torch.zeros(size, dtype=src.dtype).index_add_(0, index, e)
        return e / s[index]

    torch_scatter.composite.scatter_softmax = scatter_softmax
    try:
        import easydict  # noqa: F401
    except ImportError:
        mod = types.ModuleType("easydict")

        class EasyDict(dict):
            __getattr__ = dict.__getitem__

        mod.EasyDict = EasyDict
        sys.modules["easydict"] = mod
    try:
        import tqdm  # noqa: F401
    except ImportError:
        mod = types.ModuleType("tqdm")

        class tqdm(object):
            def __init__(self, iterable=None, *args, **kwargs):
                self.iterable = iterable

            def __iter__(self):
                return iter(self.iterable)

            def update(self, *args):
                pass

        mod.tqdm = tqdm
        sys.modules["tqdm"] = mod
    import torch_geometric
    if "torch_geometric.datasets" not in sys.modules:
        ds = types.ModuleType("torch_geometric.datasets")
        ds.RelLinkPredDataset = ds.WordNet18RR = object
        sys.modules["torch_geometric.datasets"] = ds
        torch_geometric.datasets = ds


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _Log(logging.Logger):
    def __init__(self):
        super().__init__("golden")
        self.lines = []

    def warning(self, msg, *args, **kwargs):
        self.lines.append(msg % args if args else msg)


def main():
    _extend_shim()
    from torch_geometric.data import Data
    from ultra import datasets_query  # noqa: F401
    from ultra import query_utils, tasks as ref_tasks, ultraquery as ref_uq
    from ultra.models import Ultra
    sys.path.insert(0, os.path.join(REF, "script"))
    import run_query
    from ultra_amd import query_data, synthetic

    torch.manual_seed(0)
    kg = synthetic.make_kg(num_node=200, num_triple=1600, num_relation_base=6, seed=17, relation_graph=False)
    train, ds = query_data.sample_queries(kg, 2, seed=5)
    graph = ref_tasks.build_relation_graph(Data(edge_index=train.edge_index, edge_type=train.edge_type,
                                                num_nodes=train.num_nodes, num_relations=train.num_relations))
    cfg = synthetic.default_model_cfg()
    ent_cfg = dict(cfg["entity_model_cfg"])
    ent_cfg["class"] = "QueryNBFNet"
    weights = torch.load(os.path.join(REF, "ckpts", "ultraquery.pth"), map_location="cpu")["model"]

    def make_model():
        m = ref_uq.UltraQuery(Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(ent_cfg)), logic="product",
                              dropout_ratio=1.0)
        m.load_state_dict(weights)
        return m

    out = dict(num_nodes=graph.num_nodes, num_relations=graph.num_relations, edge_index=graph.edge_index,
               edge_type=graph.edge_type, rel_edge_index=graph.relation_graph.edge_index,
               rel_edge_type=graph.relation_graph.edge_type, dropout=[])

    # ---- traversal dropout: recording wrappers around the reference's own helpers ----
    rec = {}
    edge_match, index_to_mask = ref_uq.edge_match, ref_uq.index_to_mask

    def edge_match_rec(*a):
        res = edge_match(*a)
        rec.setdefault("match", []).append(res[0].clone())
        return res

    def index_to_mask_rec(index, size):
        m = index_to_mask(index, size)
        rec["dropped"] = m.clone()
        return m

    ref_uq.edge_match, ref_uq.index_to_mask = edge_match_rec, index_to_mask_rec
    model = make_model()
    g = torch.Generator().manual_seed(23)
    n = graph.num_nodes
    R = graph.num_relations
    cases = [(1, 0.5), (4, 0.1), (9, 0.05), (70, 0.03)]
    for plus_one in (False, True):
        for bs, density in cases:
            sym = torch.rand(bs, n, generator=g) * (torch.rand(bs, n, generator=g) < density)
            r = torch.randint(0, R, (bs,), generator=g)
            if bs > 2:
                r[1] = r[0]                       # repeated relations
            gr = Data(edge_index=graph.edge_index, edge_type=graph.edge_type, num_nodes=n, num_relations=R)
            if plus_one:
                gr.inverse_rel_plus_one = True
            entry = dict(sym=sym, r_index=r, inverse_rel_plus_one=plus_one, kept={}, rel_edge_index={}, rel_edge_type={})
            for ratio, more in RATIOS:
                model.dropout_ratio, model.more_dropout = ratio, more
                rec.clear()
                dropped = model.traversal_dropout(gr, sym, r)
                entry["match"] = torch.cat(rec["match"])
                entry["kept"][(ratio, more)] = ~rec["dropped"]
                rg = ref_tasks.build_relation_graph(dropped).relation_graph
                entry["rel_edge_index"][(ratio, more)] = rg.edge_index
                entry["rel_edge_type"][(ratio, more)] = rg.edge_type
            out["dropout"].append(entry)
            print("dropout", plus_one, bs, int(entry["match"].numel()),
                  {k: int((~v).sum()) for k, v in entry["kept"].items()})
    ref_uq.edge_match, ref_uq.index_to_mask = edge_match, index_to_mask

    # ---- one training batch through the reference's train_and_validate ----
    items = [ds[i] for i in range(len(ds))]
    data = [dict(query=query_utils.Query(it["query"]), type=it["type"], easy_answer=it["easy_answer"],
                 hard_answer=it["hard_answer"]) for it in items]
    model = make_model()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    seen = []
    predict_and_target = run_query.predict_and_target

    def pat_rec(m, gr, batch):
        pred, target = predict_and_target(m, gr, batch)
        if m.training:
            seen.append(dict(query=batch["query"].as_subclass(torch.Tensor).clone(), type=batch["type"].clone(),
                             easy_answer=batch["easy_answer"].clone(), hard_answer=batch["hard_answer"].clone(),
                             pred=pred.detach().clone(), target=target.clone()))
        return pred, target

    run_query.predict_and_target = pat_rec
    train_cfg = _Cfg(train=_Cfg(num_epoch=1, batch_size=len(data), log_interval=1),
                     optimizer=_Cfg({"class": "SGD", "lr": 1.0}),
                     task=_Cfg(adversarial_temperature=0.2, metric=["mrr"]))
    log = _Log()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            torch.manual_seed(1)
            run_query.train_and_validate(train_cfg, model, graph, data, graph, data, ds.id2type, torch.device("cpu"), log,
                                         batch_per_epoch=1)
        finally:
            os.chdir(cwd)
    run_query.predict_and_target = predict_and_target
    assert len(seen) == 1, len(seen)
    grads = {k: (before[k] - v.detach()) for k, v in model.named_parameters()}
    losses = [float(line.split(":")[1]) for line in log.lines if line.startswith("binary cross entropy:")]
    out["train"] = dict(seen[0], grads=grads, logged_loss=losses[0], temperature=0.2, dropout_ratio=1.0, logic="product",
                        id2type=ds.id2type)
    print("train: loss", losses[0], "pred", float(seen[0]["pred"].min()), float(seen[0]["pred"].max()))

    buf = io.BytesIO()
    torch.save(out, buf)
    path = os.path.join(HERE, "ultraquery_train.pt.xz")
    with open(path, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
