"""Generate the committed golden vectors of multi-graph PRE-TRAINING by running the reference in this container.

    python tests/golden/gen_pretrain_golden.py

Like gen_ultraquery_train_golden.py (whose shim additions it reuses): needs the reference checkout and runs its unchanged
script/pretrain.py functions (train_and_validate with its DataLoader, DistributedSampler and multigraph_collator; test) on CPU
under tests/golden/pyg_shim.  What is recorded is the global CPU generator's side of a seeded run, so the step itself is
replaced, in this process only: a recording wrapper around the reference's tasks.negative_sampling that notes (graph id,
positives) and returns them without drawing (on a GPU the negatives come from the device generator, not the CPU one), and a
one-parameter stand-in for the model (Ultra's forward draws nothing).  The order of pretrain.py:228-262 is kept: seed, the
fast_test subsets, the model's initialisation, the loop.
Output: pretrain.pt.xz (torch.save'd dict, xz-compressed; committed), holding

  graphs        three small train / valid / test splits (ultra_amd.synthetic.make_split): their target triples and edge lists
  seed, batch_size, num_epoch, fast_test_size
  fast_test     per graph, the (2, k) targets and the types of the fast_test subset
  init_digest   per state-dict key of the reference's Ultra right after its seeded initialisation: shape, fp64 sum, fp64 sum of
                squares and the first 8 values
  batches       the (graph id, (rows, 3) positives) sequence over two epochs, the short last batch of each included
"""
import io
import logging
import lzma
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_ultraquery_train_golden as uqt  # noqa: E402  (sets up sys.path: shim, reference, repository)

import torch  # noqa: E402

REF = uqt.REF
SEED = 1024
BATCH_SIZE = 16
NUM_EPOCH = 2
FAST_TEST = 12
SHAPES = ((90, 150, 4, 30, 20, 11), (60, 90, 3, 20, 14, 12), (120, 70, 5, 18, 16, 13))   # nodes, train, R/2, valid, test, seed


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    uqt._extend_shim()
    from torch_geometric.data import Data
    from ultra import tasks as ref_tasks
    from ultra.models import Ultra
    sys.path.insert(0, os.path.join(REF, "script"))
    import pretrain as ref_pretrain
    from ultra_amd import synthetic

    splits = [synthetic.make_split(n, m, r, num_valid=v, num_test=t, seed=s, relation_graph=False) for n, m, r, v, t, s in SHAPES]

    def pyg(g):
        return Data(edge_index=g.edge_index, edge_type=g.edge_type, num_nodes=g.num_nodes, num_relations=g.num_relations,
                    target_edge_index=g.target_edge_index, target_edge_type=g.target_edge_type)

    train_data = [pyg(s[0]) for s in splits]
    valid_data = [pyg(s[1]) for s in splits]
    test_data = [pyg(s[2]) for s in splits]
    out = dict(seed=SEED, batch_size=BATCH_SIZE, num_epoch=NUM_EPOCH, fast_test_size=FAST_TEST, shapes=SHAPES,
               graphs=[dict(edge_index=s[0].edge_index, edge_type=s[0].edge_type, num_nodes=s[0].num_nodes,
                            num_relations=s[0].num_relations, train=s[0].target_triples, valid=s[1].target_triples,
                            test=s[2].target_triples) for s in splits])

    # ---- pretrain.py:228-262, in its order ----
    torch.manual_seed(SEED)
    short_valid = []
    for graph in valid_data:
        mask = torch.randperm(graph.target_edge_index.shape[1])[:FAST_TEST]
        short_valid.append(Data(edge_index=graph.edge_index, edge_type=graph.edge_type, num_nodes=graph.num_nodes,
                                num_relations=graph.num_relations, target_edge_index=graph.target_edge_index[:, mask],
                                target_edge_type=graph.target_edge_type[mask]))
    out["fast_test"] = [dict(target_edge_index=g.target_edge_index, target_edge_type=g.target_edge_type) for g in short_valid]
    cfg = synthetic.default_model_cfg()
    model = Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(cfg["entity_model_cfg"]))
    out["init_digest"] = {k: dict(shape=tuple(v.shape), sum=float(v.double().sum()), sumsq=float((v.double() ** 2).sum()),
                                  head=v.flatten()[:8].clone()) for k, v in model.state_dict().items()}
    filtered_data = [Data(edge_index=torch.cat([a.target_edge_index, b.target_edge_index, c.target_edge_index], dim=1),
                          edge_type=torch.cat([a.target_edge_type, b.target_edge_type, c.target_edge_type]), num_nodes=a.num_nodes)
                     for a, b, c in zip(train_data, valid_data, test_data)]

    # ---- the loop: the reference's train_and_validate, the step replaced by a recorder ----
    seen = []
    negative_sampling = ref_tasks.negative_sampling

    def record(graph, batch, num_negative, strict=True):
        seen.append((next(i for i, g in enumerate(train_data) if g is graph), batch.clone()))
        return torch.stack([batch, batch], dim=1)

    class Stand(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(()))

        def forward(self, graph, batch):
            return batch[..., 0].to(torch.float32) * 0 + self.w

    ref_pretrain.tasks.negative_sampling = record
    ref_pretrain.logger = logging.getLogger("golden")
    ref_pretrain.device = torch.device("cpu")
    train_cfg = _Cfg(train=_Cfg(num_epoch=NUM_EPOCH, batch_size=BATCH_SIZE, log_interval=1000),
                     optimizer=_Cfg({"class": "SGD", "lr": 0.0}),
                     task=_Cfg(num_negative=1, strict_negative=True, adversarial_temperature=1, metric=["mrr"]))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            ref_pretrain.train_and_validate(train_cfg, Stand(), train_data, short_valid, filtered_data=filtered_data)
        finally:
            os.chdir(cwd)
            ref_pretrain.tasks.negative_sampling = negative_sampling
    out["batches"] = seen
    print("batches", len(seen), [len(b) for _, b in seen][-3:], "graphs", [g for g, _ in seen])

    buf = io.BytesIO()
    torch.save(out, buf)
    with lzma.open(os.path.join(HERE, "pretrain.pt.xz"), "wb", preset=9) as f:
        f.write(buf.getvalue())


if __name__ == "__main__":
    main()
