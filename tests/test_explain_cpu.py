"""Path explanations on the CPU: a plain-torch restatement of the beam-search semantics against the
reference's recorded outputs (tests/golden/gen_explain_golden.py, explain.pt.xz), and ultra_amd.explain.topk_average_length against the
reference's paths and weights.

The restatement is the contract the HIP kernel is held to bit for bit (tests/test_explain_gpu.py).  Against the stable-sort
run of the reference it is bit-exact everywhere but one place: a destination without candidates is -inf / (0, 0, 0, 0) here
and 0 / (0, 0, 0, 0) in the reference (its scatter_add into zeros, base_nbfnet.py:216-217), which reads as "reached with
distance 0".  Each layer is therefore fed the reference's own input distances."""
import io
import lzma
import os

import pytest
import torch

from ultra_amd import explain

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain.pt.xz")
_GOLDEN = []


def load():
    if not _GOLDEN:
        with open(GOLDEN, "rb") as f:
            _GOLDEN.append(torch.load(io.BytesIO(lzma.decompress(f.read()))))
    return _GOLDEN[0]


def restate_layer(edge_index, edge_type, edge_grad, dist_in, tail, num_beam):
    """One layer of the beam search in plain torch (works on any device): returns (num_node, K) distances and (num_node, K, 4)
    back edges [src, dst, type, prev_rank]."""
    num_node, K = dist_in.shape
    dev = dist_in.device
    src, dst = edge_index[0], edge_index[1]
    live = (src != tail).nonzero().flatten()                       # ascending edge id
    s, d, r, g = src[live], dst[live], edge_type[live], edge_grad[live]
    dist = torch.full((num_node, K), float("-inf"), device=dev)
    back = torch.zeros(num_node, K, 4, dtype=torch.long, device=dev)
    if live.numel() == 0:
        return dist, back
    m = dist_in[s] + g.unsqueeze(-1)                               # (E', K): one fp32 add
    if not torch.isfinite(m).any():
        return dist, back                                          # every message -inf: the whole layer -inf and zeros
    close = torch.isclose(m.unsqueeze(-1), m.unsqueeze(-2))        # [e, b, j] = isclose(m_b, m_j)
    beams = torch.arange(K, device=dev)
    prev_rank = torch.where(close, beams, K).min(dim=-1).values
    prev_rank = torch.where(prev_rank == K, 0, prev_rank)
    # candidates of every destination: ascending edge id, then beam
    order = torch.sort(d, stable=True).indices
    s, d, r, m, prev_rank = s[order], d[order], r[order], m[order], prev_rank[order]
    key = torch.stack([s.unsqueeze(-1).expand(-1, K), d.unsqueeze(-1).expand(-1, K), r.unsqueeze(-1).expand(-1, K),
                       prev_rank], dim=-1).reshape(-1, 4)
    value = m.reshape(-1)
    dup = torch.cat([torch.zeros(1, dtype=torch.bool, device=dev), (key[1:] == key[:-1]).all(dim=-1)])
    key, value = key[~dup], value[~dup]
    # top K per destination: by value descending, ties to the earlier candidate
    by_value = torch.sort(value, descending=True, stable=True).indices
    by_dst = torch.sort(key[by_value, 1], stable=True).indices
    pick = by_value[by_dst]
    key, value = key[pick], value[pick]
    dest = key[:, 1]
    count = torch.bincount(dest, minlength=num_node)
    start = torch.cumsum(count, 0) - count
    rank = torch.arange(dest.numel(), device=dev) - start[dest]
    top = rank < K
    dist[dest[top], rank[top]] = value[top]
    back[dest[top], rank[top]] = key[top]
    # fewer than K survivors: pad with the last one kept
    short = (count > 0) & (count < K)
    rows = short.nonzero().flatten()
    if rows.numel():
        last = (count[rows] - 1)
        fill = beams.unsqueeze(0) >= count[rows].unsqueeze(1)               # (rows, K)
        dist[rows] = torch.where(fill, dist[rows, last].unsqueeze(1), dist[rows])
        back[rows] = torch.where(fill.unsqueeze(-1), back[rows, last].unsqueeze(1), back[rows])
    return dist, back


def restate_chain(edge_index, edge_type, num_node, edge_grads, h, t, num_beam):
    """beam_search_distance through the restated layers."""
    dist = torch.full((num_node, num_beam), float("-inf"), device=edge_index.device)
    dist[h, 0] = 0
    distances, back_edges = [], []
    for g in edge_grads:
        dist, back = restate_layer(edge_index, edge_type, g, dist, t, num_beam)
        distances.append(dist)
        back_edges.append(back)
    return distances, back_edges


def _layer_inputs(case, distances):
    init = torch.full((case["num_nodes"], case["num_beam"]), float("-inf"))
    init[case["h"], 0] = 0
    return [init] + list(distances[:-1])


def _has_candidates(case):
    ei = case["edge_index"]
    return torch.bincount(ei[1][ei[0] != case["t"]], minlength=case["num_nodes"]) > 0


CASES = [c["name"] for c in load()["beam"]]


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_stable_reference(name):
    case = next(c for c in load()["beam"] if c["name"] == name)
    has = _has_candidates(case)
    for i, (d_in, g) in enumerate(zip(_layer_inputs(case, case["distances"]), case["edge_grads"])):
        dist, back = restate_layer(case["edge_index"], case["edge_type"], g, d_in, case["t"], case["num_beam"])
        want_d, want_b = case["distances"][i], case["back_edges"][i].long()
        if torch.isinf(want_d).all() and not want_b.any():
            # an all -inf layer: every row -inf and zeros (base_nbfnet.py:220)
            assert torch.isinf(dist).all() and not back.any(), (name, i)
            continue
        assert torch.equal(dist[has], want_d[has]), (name, i)
        assert torch.equal(back[has], want_b[has]), (name, i)
        # destinations without candidates: -inf here, the reference's scatter_add zeros there; back edges zeros on both sides
        assert torch.isinf(dist[~has]).all() and (want_d[~has] == 0).all(), (name, i)
        assert not back[~has].any() and not want_b[~has].any(), (name, i)


def test_fixture_covers_the_edge_cases():
    cases = load()["beam"]
    names = {c["name"] for c in cases}
    assert {"close_k10", "no_out_edges", "k1"} <= names
    for c in cases:
        ei, t, k = c["edge_index"], c["t"], c["num_beam"]
        deg = torch.bincount(ei[1], minlength=c["num_nodes"])
        assert (deg == 0).any() and ((deg > 0) & (deg < k)).any() or k == 1, c["name"]      # isolated, in-degree < K
        assert (ei[0] == ei[1]).any(), c["name"]                                            # self-loops
        assert (ei[0] == t).any(), c["name"]                                                # t has out-edges
        trip = torch.stack([ei[0], ei[1], c["edge_type"]], dim=-1)
        assert (trip[1:] == trip[:-1]).all(-1).any(), c["name"]                             # adjacent parallel edges
    # the close case really has beams within isclose's tolerance that are not equal
    c = next(c for c in cases if c["name"] == "close_k10")
    d = torch.stack(c["distances"])
    fin = torch.isfinite(d[..., 1:]) & torch.isfinite(d[..., :-1])
    near = torch.isclose(d[..., 1:], d[..., :-1]) & (d[..., 1:] != d[..., :-1]) & fin
    assert near.any()
    # every layer of the head without out-edges is all -inf
    c = next(c for c in cases if c["name"] == "no_out_edges")
    assert all(torch.isinf(d).all() for d in c["distances"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_default_sort_reference_where_orders_agree(name):
    case = next(c for c in load()["beam"] if c["name"] == name)
    has = _has_candidates(case)
    for i, (d_in, g) in enumerate(zip(_layer_inputs(case, case["distances"]), case["edge_grads"])):
        dist, _ = restate_layer(case["edge_index"], case["edge_type"], g, d_in, case["t"], case["num_beam"])
        agree = (case["distances_default"][i] == case["distances"][i]) & has.unsqueeze(-1)
        assert torch.equal(dist[agree], case["distances_default"][i][agree]), (name, i)


@pytest.mark.parametrize("name", CASES)
def test_topk_average_length_matches_reference(name):
    case = next(c for c in load()["beam"] if c["name"] == name)
    backs = [b.long() for b in case["back_edges"]]
    paths, weights = explain.topk_average_length(case["distances"], backs, torch.tensor([case["t"]]), case["num_beam"])
    assert [list(p) for p in paths] == case["paths"]
    assert list(weights) == case["weights"]


def test_restatement_matches_reference_visualize_tail_rows():
    """The tail's row of every layer (what topk_average_length starts from) from the restated layers on the reference's own
    edge gradients: the reference's distances and back edges bit for bit."""
    vis = load()["visualize"]
    for tr in vis["triples"]:
        h, t, _ = tr["batch"][0].tolist()
        dists, backs = restate_chain(vis["edge_index"], vis["edge_type"], vis["num_nodes"], tr["edge_grads"], h, t,
                                     vis["num_beam"])
        assert torch.equal(torch.stack([d[t] for d in dists]), tr["tail_distances"])
        assert torch.equal(torch.stack([b[t] for b in backs]), tr["tail_back_edges"])


def test_restatement_reproduces_reference_visualize_paths():
    """The whole chain of restated layers from the head on the reference's own edge gradients: the same paths and weights
    (the 8 triples reach no destination without candidates that would make the two differ)."""
    vis = load()["visualize"]
    for tr in vis["triples"]:
        h, t, _ = tr["batch"][0].tolist()
        dists, backs = restate_chain(vis["edge_index"], vis["edge_type"], vis["num_nodes"], tr["edge_grads"], h, t,
                                     vis["num_beam"])
        paths, weights = explain.topk_average_length(dists, backs, torch.tensor([t]), vis["path_topk"])
        assert [list(p) for p in paths] == tr["paths"]
        assert list(weights) == tr["weights"]


def test_empty_and_all_inf_layers():
    ei = torch.tensor([[0, 1], [1, 2]])
    et = torch.tensor([0, 1])
    d_in = torch.full((3, 2), float("-inf"))
    dist, back = restate_layer(ei, et, torch.tensor([1.0, 2.0]), d_in, 2, 2)
    assert torch.isinf(dist).all() and not back.any()
    d_in[0, 0] = 0
    dist, back = restate_layer(ei, et, torch.tensor([1.0, 2.0]), d_in, 2, 2)
    assert dist[1].tolist() == [1.0, float("-inf")]
    # beam 1 of edge 0 is -inf: prev_rank 1, not a duplicate of beam 0 -- the row keeps both
    assert back[1].tolist() == [[0, 1, 0, 0], [0, 1, 0, 1]]
