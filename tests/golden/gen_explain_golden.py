"""Generate the committed golden vectors of the path explanations by RUNNING THE REFERENCE in this container.

    python tests/golden/gen_explain_golden.py

Like gen_golden.py: needs /root/reference, runs the unchanged reference modules (ultra.base_nbfnet, ultra.models) under the
test-only shim in tests/golden/pyg_shim/ on CPU.  Output: explain.pt.xz (a torch.save'd dict, xz-compressed; committed), holding

  beam       BaseNBFNet.beam_search_distance (base_nbfnet.py:173-232) on small seeded graphs with synthetic edge gradients
             (multiples of 1/8, plus 2^-9 steps around 300 in the `close` case so beams fall within isclose's tolerance),
             for several num_beam, run twice: with torch's default sorts and with every sort / argsort made stable.
             Each case holds a hub row, isolated nodes, rows of in-degree < num_beam, self-loops, adjacent and non-adjacent
             parallel edges and a tail with out-edges; one case starts from a head without out-edges (all -inf layers).
             The generator asserts that the reference's offset keys (scatter_topk, base_nbfnet.py:308-312) kept every pair
             of distinct values of a row apart and in order, so the stable run is exact for these inputs.
  visualize  EntityNBFNet.visualize (base_nbfnet.py:156-171) on the 200-node KG of gen_golden.py with the ultra_3g weights,
             for 8 test triples: the relation model's output, per-layer edge gradients, the tail's row of every layer's
             distances and back edges, the paths and their weights.
"""
import io
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
os.environ.setdefault("TORCH_EXTENSIONS_DIR", "/tmp/torch_ext_ref")
sys.path.insert(0, os.path.join(HERE, "pyg_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class stable_sorts(object):
    """Every Tensor.sort / argsort and torch.sort / argsort inside the block is stable."""

    def __enter__(self):
        self.saved = (torch.Tensor.sort, torch.Tensor.argsort, torch.sort, torch.argsort)
        ts, ta, fs, fa = self.saved
        torch.Tensor.sort = lambda self_, *a, **k: ts(self_, *a, **dict(k, stable=True))
        torch.Tensor.argsort = lambda self_, *a, **k: ta(self_, *a, **dict(k, stable=True))
        torch.sort = lambda x, *a, **k: fs(x, *a, **dict(k, stable=True))
        torch.argsort = lambda x, *a, **k: fa(x, *a, **dict(k, stable=True))
        return self

    def __exit__(self, *exc):
        torch.Tensor.sort, torch.Tensor.argsort, torch.sort, torch.argsort = self.saved
        return False


def _check_offset_keys(input, size, k, largest=True):
    """The reference's scatter_topk sorts value + offset * group in fp32: assert that this kept every pair of distinct values
    of a group apart and in order and the groups apart (then the stable run is the exact top-k)."""
    group = torch.arange(len(size)).repeat_interleave(size)
    fin = ~torch.isinf(input)
    mx, mn = input[fin].max().item(), input[fin].min().item()
    assert mx > mn, "degenerate fixture: one finite value"
    safe = input.clamp(2 * mn - mx, 2 * mx - mn)
    ext = safe + (-(mx - mn) * 4) * group
    for gi in range(len(size)):
        sel = (group == gi).nonzero().flatten()
        v, e = input[sel].double(), ext[sel].double()
        order = torch.argsort(v, descending=True, stable=True)
        v, e = v[order], e[order]
        assert bool(((v[1:] < v[:-1]) <= (e[1:] < e[:-1])).all()), "offset keys merged distinct values"
        if gi + 1 < len(size):
            nxt = ext[group == gi + 1]
            assert e.min() > nxt.max(), "offset keys merged two rows"


def _graph(seed, num_node, num_edge, hub_in, tail):
    """A seeded multigraph: node 1 a hub of in-degree `hub_in`, the last two nodes isolated, self-loops, parallel edges adjacent
    and not adjacent in edge-id order, out-edges of `tail`."""
    g = torch.Generator().manual_seed(seed)
    live = num_node - 2
    src = torch.randint(0, live, (num_edge,), generator=g)
    dst = torch.randint(0, live, (num_edge,), generator=g)
    typ = torch.randint(0, 4, (num_edge,), generator=g)
    hub_src = torch.randint(0, live, (hub_in,), generator=g)
    src = torch.cat([src, hub_src, torch.tensor([5, 6, tail, tail])])
    dst = torch.cat([dst, torch.ones(hub_in, dtype=torch.long), torch.tensor([5, 6, 2, 3])])      # self-loops, tail out-edges
    typ = torch.cat([typ, torch.randint(0, 4, (hub_in,), generator=g), torch.tensor([0, 1, 2, 3])])
    perm = torch.randperm(src.numel(), generator=g)
    src, dst, typ = src[perm], dst[perm], typ[perm]
    # parallel edges: one copy right behind its original (adjacent ids), one far away
    adj = torch.randint(0, src.numel(), (4,), generator=g)
    far = torch.randint(0, src.numel(), (4,), generator=g)
    parts_s, parts_d, parts_t = [], [], []
    for i in range(src.numel()):
        parts_s.append(src[i:i + 1]), parts_d.append(dst[i:i + 1]), parts_t.append(typ[i:i + 1])
        if bool((adj == i).any()):
            parts_s.append(src[i:i + 1]), parts_d.append(dst[i:i + 1]), parts_t.append(typ[i:i + 1])
    src, dst, typ = torch.cat(parts_s + [src[far]]), torch.cat(parts_d + [dst[far]]), torch.cat(parts_t + [typ[far]])
    return torch.stack([src, dst]), typ


def _grads(seed, num_edge, num_layer, base=0.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(num_layer):
        span = 2 if base else 40      # (the close case: few distinct eighths, so paths meet within isclose's tolerance)
        eighths = torch.randint(-span, span + 1, (num_edge,), generator=g).double() / 8
        fine = torch.randint(0, 4, (num_edge,), generator=g).double() * 2.0 ** -9 if base else 0.0
        out.append((base + eighths + fine).float())
    return out


def gen_beam():
    from torch_geometric.data import Data
    from ultra import base_nbfnet
    from ultra.base_nbfnet import BaseNBFNet

    orig_topk = base_nbfnet.scatter_topk

    def checked_topk(input, size, k, largest=True):
        _check_offset_keys(input, size, k, largest)
        return orig_topk(input, size, k, largest)

    model = BaseNBFNet(64, [64], 4)
    cases = []
    specs = [  # (name, seed, num_node, num_edge, hub_in, h, t, num_beam, grad base, layers)
        ("small_k3", 1, 24, 60, 12, 0, 7, 3, 0.0, 4),
        ("hub_k10", 2, 40, 120, 40, 0, 9, 10, 0.0, 4),
        ("hub_k16", 3, 40, 160, 70, 4, 11, 16, 0.0, 3),
        ("close_k10", 4, 20, 60, 20, 0, 3, 10, 300.0, 3),
        ("k1", 5, 24, 60, 12, 0, 7, 1, 0.0, 4),
        ("no_out_edges", 6, 16, 40, 8, 15, 2, 4, 0.0, 2),     # head 15 is isolated: every layer is all -inf
    ]
    base_nbfnet.scatter_topk = checked_topk
    try:
        for name, seed, n, e, hub_in, h, t, k, base, num_layer in specs:
            ei, et = _graph(seed, n, e, hub_in, t)
            data = Data(edge_index=ei, edge_type=et, num_nodes=n)
            grads = _grads(seed + 100, ei.shape[1], num_layer, base)
            h_index, t_index = torch.tensor([h]), torch.tensor([t])
            d_def, b_def = model.beam_search_distance(data, grads, h_index, t_index, k)
            with stable_sorts():
                d_st, b_st = model.beam_search_distance(data, grads, h_index, t_index, k)
                paths, weights = model.topk_average_length(d_st, b_st, t_index, k)
            cases.append(dict(name=name, edge_index=ei, edge_type=et, num_nodes=n, h=h, t=t, num_beam=k, edge_grads=grads,
                              distances_default=d_def, back_edges_default=[b.to(torch.int32) for b in b_def], distances=d_st,
                              back_edges=[b.to(torch.int32) for b in b_st],
                              paths=[list(p) for p in paths], weights=list(weights)))
            differ = sum(int(not torch.equal(a, b)) for a, b in zip(d_def, d_st))
            print("beam", name, "edges", ei.shape[1], "layers whose default-sort distances differ:", differ)
    finally:
        base_nbfnet.scatter_topk = orig_topk
    return cases


def gen_visualize():
    from torch_geometric.data import Data
    from ultra import tasks as ref_tasks
    from ultra.models import Ultra
    from ultra_amd import synthetic

    state = torch.load(os.path.join(HERE, "ultra_3g_model.pt"))
    kg = synthetic.make_kg(num_node=200, num_triple=1500, num_relation_base=6, num_test=16, seed=7, relation_graph=False)
    data = Data(edge_index=kg.edge_index, edge_type=kg.edge_type, num_nodes=kg.num_nodes, num_relations=kg.num_relations)
    data = ref_tasks.build_relation_graph(data)
    cfg = synthetic.default_model_cfg()
    model = Ultra(rel_model_cfg=dict(cfg["rel_model_cfg"]), entity_model_cfg=dict(cfg["entity_model_cfg"]))
    model.load_state_dict(state)
    model.eval()
    ent = model.entity_model
    seen = {}
    beam = ent.beam_search_distance

    def rec_beam(data_, edge_grads, h_index, t_index, num_beam=10):
        seen["edge_grads"] = [g.detach().clone() for g in edge_grads]
        out = beam(data_, edge_grads, h_index, t_index, num_beam)
        seen["distances"], seen["back_edges"] = out
        return out

    ent.beam_search_distance = rec_beam
    triples = []
    with stable_sorts():
        for triple in kg.target_triples[:8]:
            batch = triple.view(1, 3)
            with torch.no_grad():
                rel = model.relation_model(data.relation_graph, query=batch[:, 2])
            ent.query = rel
            for layer in ent.layers:
                layer.relation = rel
            paths, weights = ent.visualize(data, batch)
            t = int(triple[1])
            triples.append(dict(batch=batch, relation_representations=rel, edge_grads=seen["edge_grads"],
                                tail_distances=torch.stack([d[t] for d in seen["distances"]]),        # (layers, num_beam)
                                tail_back_edges=torch.stack([b[t] for b in seen["back_edges"]]),      # (layers, num_beam, 4)
                                paths=[list(p) for p in paths], weights=list(weights)))
            print("visualize", batch.tolist(), "paths", len(paths), "best", weights[0] if weights else None)
    return dict(edge_index=data.edge_index, edge_type=data.edge_type, num_nodes=data.num_nodes,
                num_relations=data.num_relations, rel_edge_index=data.relation_graph.edge_index,
                rel_edge_type=data.relation_graph.edge_type, num_beam=ent.num_beam, path_topk=ent.path_topk, triples=triples)


if __name__ == "__main__":
    assert os.path.isdir(REF), "golden generation needs the reference checkout at /root/reference"
    torch.manual_seed(0)
    out = dict(beam=gen_beam(), visualize=gen_visualize())
    buf = io.BytesIO()
    torch.save(out, buf)
    path = os.path.join(HERE, "explain.pt.xz")
    with open(path, "wb") as f:
        f.write(lzma.compress(buf.getvalue()))
    print("wrote", path, os.path.getsize(path), "bytes")
