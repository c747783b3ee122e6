"""Generate the committed golden vectors of the RotatE layer by RUNNING THE REFERENCE in this container.

    python tests/golden/gen_rotate_golden.py

Needs the reference checkout; runs its UNCHANGED ultra.layers.GeneralizedRelationalConv(64, 64, R, 64, "rotate", aggr, True,
"relu") on the CPU under tests/golden/pyg_shim -- for rotate the reference takes its unfused route (message / aggregate /
update, layers.py:135-181), all torch ops.  Output: rotate.pt.xz (torch.save'd dict, xz-compressed; committed), holding

  graph      tests/helpers.random_graph (rows (target, source)) with duplicate edges, nodes without in-edges and one hub node
             with more in-edges than the default seg_len (256: a chain row of a reference-order plan); 6 relation types;
             num_node, num_relation, edge_type and two orders of the same edge list IN THE REFERENCE'S (source, target) LAYOUT:
             `sorted` (by target, source, edge id) and `shuffled`, each with its edge types
  x, boundary, query, og    the layer's inputs (batch 2, d = 64) and the output gradient of the backward runs
  state      the layer's state dict (one seeded initialisation serves the four aggregates: asserted)
  <aggr>     for sum, mean, max, min -- {order: {"aggregate", "out"} fp32, "aggregate64" / "out64" from the layer run in float64
             (sorted order; the other order differs from it by fp64 roundings only)}; max / min aggregates do not depend on the edge
             order: asserted, so `shuffled` holds the layer output alone
  grads      for sum and max (sorted order): d out.backward(og) / d x, boundary and every parameter
  sorted_scatter_is_sequential   the CPU scatter_add_ the reference's sum ends in equals, bit for bit, a loop that adds the k-th
             in-edge's message of every node in turn and the boundary last -- on the `sorted` list (asserted here): the engine's
             reference order (sequential per row in sorted order, then + boundary)
  shuffled_differs               whether the `shuffled` list's scatter_add_ (list order per target) differs from that loop in
             the sorted order (it does, in the last bits: recorded, not asserted)
"""
import io
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "pyg_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, R, D, BATCH = 32, 6, 64, 2
AGGRS = ("sum", "mean", "max", "min")


def sequential_sum(edge_index, messages, boundary):
    """Adds the k-th in-edge's message of every node in turn (k = 0, 1, ...: list order per target), the boundary last."""
    target = edge_index[1]
    order = torch.sort(target, stable=True)[1]
    count = torch.bincount(target, minlength=boundary.shape[1])
    start = count.cumsum(0) - count
    acc = torch.zeros_like(boundary)
    for k in range(int(count.max())):
        nodes = (count > k).nonzero().flatten()
        acc[:, nodes] = acc[:, nodes] + messages[:, order[start[nodes] + k]]
    return acc + boundary


def main():
    from tests.helpers import random_graph
    from ultra.layers import GeneralizedRelationalConv

    ei, et = random_graph(N, 330, R, seed=41, hub=(5, 280), empty_rows=3, duplicates=30)   # rows: (target, source)
    ei_ref = ei.flip(0).contiguous()                                                         # PyG: (source, target)
    E = ei.shape[1]
    key = (ei_ref[1] * N + ei_ref[0]) * E + torch.arange(E)
    perm = torch.sort(key)[1]
    orders = {"sorted": (ei_ref[:, perm].contiguous(), et[perm].contiguous()), "shuffled": (ei_ref, et)}
    assert torch.bincount(ei_ref[1], minlength=N).max() > 256 and (torch.bincount(ei_ref[1], minlength=N) == 0).any()

    g = torch.Generator().manual_seed(42)
    x = torch.randn(BATCH, N, D, generator=g)
    boundary = torch.randn(BATCH, N, D, generator=g)
    query = torch.randn(BATCH, D, generator=g)
    og = torch.randn(BATCH, N, D, generator=g)

    out = {"num_node": N, "num_relation": R, "x": x, "boundary": boundary, "query": query, "og": og, "grads": {},
           "graph": {name: {"edge_index": e, "edge_type": t} for name, (e, t) in orders.items()}}
    state = None
    for aggr in AGGRS:
        torch.manual_seed(43)
        layer = GeneralizedRelationalConv(D, D, R, D, "rotate", aggr, True, "relu")
        sd = {k: v.clone() for k, v in layer.state_dict().items()}
        if state is None:
            state = sd
        assert all(torch.equal(sd[k], state[k]) for k in state)
        captured = []
        inner = layer.aggregate

        def recording(input, edge_weight, index, dim_size, _inner=inner):     # (the shim reads this signature)
            captured.append(_inner(input, edge_weight, index, dim_size))
            return captured[-1]
        layer.aggregate = recording
        rec = {}
        for name, (e, t) in orders.items():
            with torch.no_grad():
                y = layer(x, query, boundary, e, t, (N, N))
            rec[name] = {"aggregate": captured.pop().clone(), "out": y.clone()}
        if aggr in ("max", "min"):
            assert torch.equal(rec["sorted"]["aggregate"], rec["shuffled"]["aggregate"])
            del rec["shuffled"]["aggregate"]
        e, t = orders["sorted"]
        layer.double()
        with torch.no_grad():
            y = layer(x.double(), query.double(), boundary.double(), e, t, (N, N))
        rec["aggregate64"], rec["out64"] = captured.pop().clone(), y.clone()
        layer.float()
        if aggr in ("sum", "max"):
            xg, bg = x.clone().requires_grad_(), boundary.clone().requires_grad_()
            layer.zero_grad()
            layer(xg, query, bg, e, t, (N, N)).backward(og)
            captured.clear()
            out["grads"][aggr] = {"x": xg.grad.clone(), "boundary": bg.grad.clone(),
                                  "params": {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}}
        out[aggr] = rec
    out["state"] = state

    # the finding the bit-exact pin rests on: on the sorted list the CPU scatter_add_ is the sequential loop
    rel = state["relation.weight"].expand(BATCH, -1, -1)
    e, t = orders["sorted"]
    x_j, r_j = x[:, e[0]], rel[:, t]
    x_re, x_im = x_j.chunk(2, dim=-1)
    r_re, r_im = r_j.chunk(2, dim=-1)
    msg = torch.cat([x_re * r_re - x_im * r_im, x_re * r_im + x_im * r_re], dim=-1)
    sequential = sequential_sum(e, msg, boundary)
    flags = {name: torch.equal(sequential, out["sum"][name]["aggregate"]) for name in orders}
    assert flags["sorted"], "sorted-list scatter_add_ != sequential loop"
    out["sorted_scatter_is_sequential"] = flags["sorted"]
    out["shuffled_differs"] = not flags["shuffled"]
    print("shuffled list against the sorted order: max abs difference %g"
          % (out["sum"]["shuffled"]["aggregate"] - sequential).abs().max().item())

    buf = io.BytesIO()
    torch.save(out, buf)
    path = os.path.join(HERE, "rotate.pt.xz")
    with lzma.open(path, "wb", preset=9) as f:
        f.write(buf.getvalue())
    print("wrote %s (%d bytes; sorted == sequential: %s, shuffled differs: %s)"
          % (path, os.path.getsize(path), flags["sorted"], out["shuffled_differs"]))


if __name__ == "__main__":
    main()
