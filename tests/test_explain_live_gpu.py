"""Explanations on a graph that holds edits, on the GPU: the three delta aggregate kernels against fp64
restatements on exactly representable inputs, the differentiable aggregate on (base, delta) against the plan of the
materialised graph, the beam fix-up launch against the plain-torch restatement of tests/test_explain_cpu.py on
materialize(), EntityNBFNet.edge_grads_batch(delta=) against the materialised route and against fp64 autograd, and
Predictor.explain_tails / explain_heads(compact=False) end to end."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_explain_batch_gpu import _compare_paths, _golden_data, _quarters, _ultra_3g
from tests.test_explain_cpu import load, restate_layer
from ultra_amd import _lib, explain, predict, rspmm
from ultra_amd.data import Data

pytestmark = pytest.mark.gpu
SAMPLES = (1, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- 1: the delta aggregate kernels ----
def _small_graph(dev, retract=True):
    """N = 37, R = 3 direct relations in loader form [direct ; inverse], with the edits the kernels can go wrong at: node 30
    gains 5 added in-edges, nodes 20 .. 24 one each, the fact (7, 1, 22) is stated twice (two added edges with the same
    (src, dst, type), twice), (3, 0, 3) is a self loop, and two base facts are retracted (rows touched by removals only)."""
    g = torch.Generator().manual_seed(4)
    h, t = torch.randint(0, 19, (2, 90), generator=g)       # (the base graph lives on nodes 0 .. 18)
    r = torch.randint(0, 3, (90,), generator=g)
    data = Data(edge_index=torch.stack([torch.cat([h, t]), torch.cat([t, h])]).to(dev), edge_type=torch.cat([r, r + 3]).to(dev),
                num_nodes=37, num_relations=6)
    delta = rspmm.GraphDelta(data, capacity=12)
    facts = [(20, 0, 30), (21, 1, 30), (22, 2, 30), (23, 0, 30), (24, 1, 30), (7, 1, 22), (7, 1, 22), (3, 0, 3)]
    delta.add(*zip(*facts))
    if retract:
        delta.remove([int(h[0]), int(h[5])], [int(r[0]), int(r[5])], [int(t[0]), int(t[5])])
    return data, delta


def _restate_delta(delta, rel, x, og):
    """fp64: the added edges' messages scattered into their destinations, the transpose, and the per-edge gradients."""
    (src, dst), ty = (v.cpu() for v in delta.edges()[0]), delta.edges()[1].cpu()
    rel, x, og = rel.double(), x.double(), og.double()
    fwd = torch.zeros_like(x).index_add_(1, dst, rel[:, ty] * x[:, src])
    bwd = torch.zeros_like(x).index_add_(1, src, rel[:, ty] * og[:, dst])
    wgrad = torch.zeros(x.shape[0], 2 * delta.capacity, dtype=torch.float64)
    wgrad[:, :len(src)] = (og[:, dst] * rel[:, ty] * x[:, src]).sum(-1)
    return fwd, bwd, wgrad


def _rows_entry(entry, delta, rel, x, out):
    operand = delta.explain_operand()
    (_, mrel), (_, mx), (_, mout) = rspmm.as_mat(rel), rspmm.as_mat(x), rspmm.as_mat(out)
    _lib.check(entry(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mx), ctypes.byref(mout), _lib.stream_of(x)))
    return out


@pytest.mark.parametrize("row_len", (64, 192, 132))
def test_delta_aggregate_kernels_are_exact_on_quarters(dev, row_len):
    """Operands in {-4 .. 4} / 4: every product is a multiple of 1/64 and every sum here far below 2^24 / 64, so forward, input
    gradient and edge gradients must equal the fp64 restatement exactly, in any order -- and twice with the same bits."""
    data, delta = _small_graph(dev)
    in_degree = torch.bincount(delta.edges()[0][1], minlength=37)
    assert int(in_degree[30]) == 5 and int(in_degree[20]) == 1 and int(in_degree[22]) == 3 and int(in_degree[3]) == 2
    assert delta.num_removed > 0
    empty = rspmm.GraphDelta(data, capacity=12)
    g = torch.Generator().manual_seed(row_len)
    for num_sample in SAMPLES:
        rel, x, og, start = (_quarters((num_sample, n, row_len), g) for n in (6, 37, 37, 37))
        fwd, bwd, wgrad = _restate_delta(delta, rel, x, og)
        rel_d, x_d, og_d = rel.to(dev), x.to(dev), og.to(dev)
        for _ in range(2):
            got = _rows_entry(_lib.lib.ultra_rspmm_delta_edges_forward, delta, rel_d, x_d, start.to(dev))
            assert torch.equal(got.cpu().double(), start.double() + fwd), (num_sample, row_len)
            got = _rows_entry(_lib.lib.ultra_rspmm_delta_edges_backward_input, delta, rel_d, og_d, start.to(dev))
            assert torch.equal(got.cpu().double(), start.double() + bwd), (num_sample, row_len)
            got = delta.delta_edge_grad_samples(rel_d, x_d, og_d)
            assert got.shape == (num_sample, 24) and torch.equal(got.cpu().double(), wgrad), (num_sample, row_len)
        # one relation table for every sample (outer stride 0)
        shared = rel_d[:1].expand(num_sample, -1, -1)
        fwd0, _, wgrad0 = _restate_delta(delta, rel[:1].expand(num_sample, -1, -1), x, og)
        got = _rows_entry(_lib.lib.ultra_rspmm_delta_edges_forward, delta, shared, x_d, start.to(dev))
        assert torch.equal(got.cpu().double(), start.double() + fwd0)
        assert torch.equal(delta.delta_edge_grad_samples(shared, x_d, og_d).cpu().double(), wgrad0)
        # an empty layout (count 0): the rows are untouched, every gradient column is zero
        for entry in (_lib.lib.ultra_rspmm_delta_edges_forward, _lib.lib.ultra_rspmm_delta_edges_backward_input):
            got = _rows_entry(entry, empty, rel_d, x_d, start.to(dev))
            assert torch.equal(got.cpu().view(torch.int32), start.view(torch.int32))
        assert not empty.delta_edge_grad_samples(rel_d, x_d, og_d).any()


def test_delta_aggregate_entries_refuse_what_they_do_not_serve(dev):
    data, delta = _small_graph(dev)
    rel, x = torch.zeros(2, 6, 64, device=dev), torch.zeros(2, 37, 64, device=dev)
    lib = _lib.lib
    (_, mrel), (_, mx) = rspmm.as_mat(rel), rspmm.as_mat(x)
    operand = delta.explain_operand()
    assert lib.ultra_rspmm_delta_edges_forward(None, ctypes.byref(mrel), ctypes.byref(mx), ctypes.byref(mx), None) == _lib.ULTRA_ERR_INVALID
    assert b"edits" in lib.ultra_last_error()
    assert lib.ultra_rspmm_delta_edges_forward(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mx), None, None) == _lib.ULTRA_ERR_INVALID
    _, odd = rspmm.as_mat(torch.zeros(2, 37, 66, device=dev)[:, :, 1:65])       # (rows off the 16-byte grid)
    assert lib.ultra_rspmm_delta_edges_forward(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(odd), ctypes.byref(odd),
                                               None) == _lib.ULTRA_ERR_UNSUPPORTED
    out = torch.zeros(2, 24, device=dev)
    assert lib.ultra_rspmm_delta_edge_grad_samples(ctypes.byref(operand), ctypes.byref(mrel), ctypes.byref(mx), ctypes.byref(mx),
                                                   out.data_ptr(), 23, None) == _lib.ULTRA_ERR_INVALID
    assert b"weight_grad_stride" in lib.ultra_last_error()
    plan = rspmm.get_plan(data.edge_index.flip(0).contiguous(), data.edge_type, 37, 6, exact_order=False)
    with pytest.raises(RuntimeError, match="constant"):
        rspmm.plan_delta_rspmm(plan, delta, rel.clone().requires_grad_(), x)


@pytest.mark.parametrize("retract", (True, False))
@pytest.mark.parametrize("row_len", (64, 128))
def test_differentiable_aggregate_equals_the_materialised_plan_on_quarters(dev, row_len, retract):
    """rspmm.plan_delta_rspmm on (base plan, delta) against rspmm.plan_rspmm on a plan of materialize(): output, input gradient
    and boundary gradient, exact on quarters whatever the association.  retract=False: a delta without tombstones, which runs
    the base plan with unit weights instead of the keep vector."""
    data, delta = _small_graph(dev, retract)
    assert bool(delta.num_removed) == retract
    mat = delta.materialize()
    base_plan = rspmm.get_plan(data.edge_index.flip(0).contiguous(), data.edge_type, 37, 6, exact_order=False)
    mat_plan = rspmm.get_plan(mat.edge_index.flip(0).contiguous(), mat.edge_type, 37, 6, exact_order=False)
    g = torch.Generator().manual_seed(10 + row_len)
    for num_sample in SAMPLES:
        rel, og = _quarters((num_sample, 6, row_len), g).to(dev), _quarters((num_sample, 37, row_len), g).to(dev)
        outs = []
        for live in (True, False):
            x = _quarters((num_sample, 37, row_len), torch.Generator().manual_seed(row_len)).to(dev).requires_grad_()
            bnd = _quarters((num_sample, 37, row_len), torch.Generator().manual_seed(1 + row_len)).to(dev).requires_grad_()
            out = (rspmm.plan_delta_rspmm(base_plan, delta, rel, x, bnd) if live
                   else rspmm.plan_rspmm(mat_plan, rel, x, None, sum="add", mul="mul", boundary=bnd))
            outs.append((out.detach(),) + torch.autograd.grad(out, (x, bnd), og))
        for got, want in zip(*outs):
            assert torch.equal(got, want), (num_sample, row_len)


# ---- 2: the beam fix-up ----
def _beam_graph(dev):
    """The golden `hub_k10` graph (40 nodes) plus seven rows made for the fix-up launch, and the edits laid on them:
      A     no base in-edge; gains added edges, one from sample 0's tail
      B     three base in-edges, all retracted: -inf and (0, 0, 0, 0)
      C     a dead key that stands for three duplicate slots in the middle of the row; an added edge equal to its last base edge
      D     a dead slot between two equal slots: without it the second is a duplicate of the first
      H     base degree 300 (a hub row), dead keys in its first and its last slice, an added edge
      G256 / G257   base degree exactly 256 and 257, one dead key and one added edge each."""
    case = next(c for c in load()["beam"] if c["name"] == "hub_k10")
    ei, et, n0 = case["edge_index"], case["edge_type"], case["num_nodes"]
    rd = int(et.max()) + 1
    assert n0 == 40 and rd >= 3
    A, B, C, D, H, G256, G257 = range(n0, n0 + 7)
    g = torch.Generator().manual_seed(7)
    extra = [(1, B, 0), (2, B, 1), (2, B, 1)]
    extra += [(3, C, 0), (4, C, 1), (5, C, 0), (5, C, 0), (5, C, 0), (6, C, 2), (4, C, 1)]
    extra += [(3, D, 0), (8, D, 1), (3, D, 0), (10, D, 0)]
    wide = {}
    for row, degree in ((H, 300), (G256, 256), (G257, 257)):
        wide[row] = list(zip(torch.randint(0, n0, (degree,), generator=g).tolist(), [row] * degree,
                             torch.randint(0, rd, (degree,), generator=g).tolist()))
        extra += wide[row]
    s, d, ty = (torch.tensor(v) for v in zip(*extra))
    data = Data(edge_index=torch.cat([ei, torch.stack([s, d])], dim=1).to(dev), edge_type=torch.cat([et, ty]).to(dev),
                num_nodes=n0 + 7, num_relations=2 * rd)
    tails = [case["t"], 3, 5]
    delta = rspmm.GraphDelta(data, capacity=16)
    adds = [(12, 0, A), (13, 1, A), (tails[0], 0, A), (4, 1, C), (14, 2, H), (15, 0, G256), (16, 1, G257)]
    delta.add(*zip(*adds))
    first, last = wide[H][0], wide[H][-1]
    removes = [(1, 0, B), (2, 1, B), (5, 0, C), (8, 1, D), (first[0], first[2], H), (last[0], last[2], H),
               (wide[G256][100][0], wide[G256][100][2], G256), (wide[G257][-1][0], wide[G257][-1][2], G257)]
    delta.remove(*[torch.tensor(v) for v in zip(*removes)])
    in_degree = torch.bincount(data.edge_index[1], minlength=n0 + 7)
    assert in_degree[[A, B, C, D, H, G256, G257]].tolist() == [0, 3, 7, 4, 300, 256, 257]
    assert _lib.BEAM_HUB_DEGREE == 256
    mat = delta.materialize()
    assert not (mat.edge_index[1] == B).any()                                      # every in-edge of B is dead
    g = torch.Generator().manual_seed(8)
    grads = [(torch.randint(-40, 41, (3, data.edge_index.shape[1]), generator=g).float() / 8).to(dev) for _ in range(3)]
    added = [(torch.randint(-40, 41, (3, 32), generator=g).float() / 8).to(dev) for _ in range(3)]
    keep = delta.keep_vector().bool()
    # the gradients in materialised order: the surviving base edges, then the 2 m added ones
    mat_grads = [torch.cat([x[:, keep], y[:, :2 * len(delta)]], dim=1) for x, y in zip(grads, added)]
    delta.explain_operand()
    touched = delta.explain.rows[:int(delta.explain.count)].long()
    return dict(data=data, delta=delta, mat=mat, grads=grads, added=added, mat_grads=mat_grads, heads=[case["h"], 12, 4],
                tails=tails, touched=touched, rows=dict(A=A, B=B, C=C, D=D, H=H))


_BEAM = {}


def _beam_case(dev, k):
    """The graph, and per beam width the restated chain on materialize(): per layer the (3, N, K) input and outputs."""
    if "graph" not in _BEAM:
        _BEAM["graph"] = _beam_graph(dev)
    graph = _BEAM["graph"]
    if k not in _BEAM:
        n, mat = graph["data"].num_nodes, graph["mat"]
        dist = torch.full((3, n, k), float("-inf"), device=dev)
        dist[torch.arange(3, device=dev), torch.tensor(graph["heads"], device=dev), 0] = 0
        layers = []
        for grad in graph["mat_grads"]:
            outs = [restate_layer(mat.edge_index, mat.edge_type, grad[s], dist[s], graph["tails"][s], k) for s in range(3)]
            want_d, want_b = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
            layers.append((dist, want_d, want_b))
            dist = want_d
        _BEAM[k] = layers
    return graph, _BEAM[k]


@pytest.mark.parametrize("k", (1, 10, 64))
def test_beam_fix_up_equals_the_restatement_on_the_materialised_graph(dev, k):
    graph, layers = _beam_case(dev, k)
    data, delta = graph["data"], graph["delta"]
    csr = explain.beam_csr(data.edge_index, data.edge_type, data.num_nodes)
    untouched = torch.ones(data.num_nodes, dtype=torch.bool, device=dev)
    untouched[graph["touched"]] = False
    assert int(untouched.sum()) > 0 and int((~untouched).sum()) >= 14
    reached = False
    for num_sample in SAMPLES:
        tails = torch.tensor(graph["tails"][:num_sample], device=dev)
        for i, (dist_in, want_d, want_b) in enumerate(layers):
            got_d, got_b = explain.beam_search_layer_batch(csr, graph["grads"][i][:num_sample], dist_in[:num_sample], tails, k,
                                                           delta=delta, added_grad=graph["added"][i][:num_sample])
            base_d, base_b = explain.beam_search_layer_batch(csr, graph["grads"][i][:num_sample], dist_in[:num_sample], tails, k)
            # rows no edit touches are the base launch's
            assert torch.equal(got_d[:, untouched].view(torch.int32), base_d[:, untouched].view(torch.int32))
            assert torch.equal(got_b[:, untouched], base_b[:, untouched])
            got_b = got_b * torch.isfinite(got_d).flatten(1).any(1).view(-1, 1, 1, 1)     # (the all -inf rule, per sample)
            where = (k, num_sample, i)
            assert torch.equal(got_d.view(torch.int32), want_d[:num_sample].view(torch.int32)), where
            assert torch.equal(got_b, want_b[:num_sample]), where
            # a row whose base edges are all dead
            assert torch.isinf(got_d[:, graph["rows"]["B"]]).all() and not got_b[:, graph["rows"]["B"]].any()
            reached = reached or bool(torch.isfinite(got_d[:, [graph["rows"][name] for name in "ACDH"]]).any())
    assert reached       # (the made rows take part in the search)
    # all -inf distances: every row -inf, and the rule zeroes the back edges
    dist_in = torch.full((3, data.num_nodes, k), float("-inf"), device=dev)
    got_d, got_b = explain.beam_search_layer_batch(csr, graph["grads"][0], dist_in, torch.tensor(graph["tails"], device=dev), k,
                                                   delta=delta, added_grad=graph["added"][0])
    assert torch.isinf(got_d).all() and (got_d < 0).all()
    # the whole chain through beam_search_distance_batch
    dists, backs = explain.beam_search_distance_batch(data, graph["grads"], graph["heads"], graph["tails"], k, delta=delta,
                                                      added_grads=graph["added"])
    for (_, want_d, want_b), got_d, got_b in zip(layers, dists, backs):
        assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)) and torch.equal(got_b, want_b)


def test_beam_fix_up_argument_rules(dev):
    graph, _ = _beam_case(dev, 1)
    data, delta = graph["data"], graph["delta"]
    csr = explain.beam_csr(data.edge_index, data.edge_type, data.num_nodes)
    dist_in = torch.full((3, data.num_nodes, 4), float("-inf"), device=dev)
    tails = torch.tensor(graph["tails"], device=dev)
    with pytest.raises(ValueError, match="go together"):
        explain.beam_search_layer_batch(csr, graph["grads"][0], dist_in, tails, 4, delta=delta)
    with pytest.raises(ValueError, match="added gradients"):
        explain.beam_search_layer_batch(csr, graph["grads"][0], dist_in, tails, 4, delta=delta, added_grad=graph["added"][0][:, :-1])
    with pytest.raises(ValueError):
        explain.beam_search_distance_batch(data, graph["grads"], graph["heads"], graph["tails"], 4, delta=delta,
                                           added_grads=graph["added"][:2])


# ---- 3: the model's edge gradients ----
def _fp64_edge_grads(state, edge_index, edge_type, num_node, reps, triple):
    """d score / d edge weight of every layer of the sum / DistMult entity model in fp64 on the CPU with plain torch autograd:
    messages from edge_index[0] into edge_index[1], the clone chain summed (layer i: the direct gradients of layers i .. L-1)."""
    sd = {k[len("entity_model."):]: v.double().cpu() for k, v in state.items() if k.startswith("entity_model.")}
    h, t, r = triple
    reps = reps.double()
    query = reps[r]
    boundary = torch.zeros(num_node, query.shape[0], dtype=torch.float64)
    boundary[h] = query
    x, weights, i = boundary, [], 0
    while "layers.%d.linear.weight" % i in sd:
        p = "layers.%d." % i
        rel = F.linear(F.relu(F.linear(reps, sd[p + "relation_projection.0.weight"], sd[p + "relation_projection.0.bias"])),
                       sd[p + "relation_projection.2.weight"], sd[p + "relation_projection.2.bias"])
        w = torch.ones(edge_index.shape[1], dtype=torch.float64, requires_grad=True)
        weights.append(w)
        update = torch.zeros_like(boundary).index_add(0, edge_index[1], rel[edge_type] * x[edge_index[0]] * w.unsqueeze(-1))
        out = F.linear(torch.cat([x, update + boundary], dim=-1), sd[p + "linear.weight"], sd[p + "linear.bias"])
        out = F.relu(F.layer_norm(out, (out.shape[-1],), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"]))
        x = out + x if out.shape == x.shape else out
        i += 1
    hidden = F.relu(F.linear(torch.cat([x[t], query]), sd["mlp.0.weight"], sd["mlp.0.bias"]))
    score = F.linear(hidden, sd["mlp.2.weight"], sd["mlp.2.bias"]).squeeze(-1)
    direct = torch.autograd.grad(score, weights)
    return torch.stack(direct).flip(0).cumsum(0).flip(0)


def _golden_facts(data):
    direct = (data.edge_type < data.num_relations // 2).cpu()
    ei, et = data.edge_index.cpu(), data.edge_type.cpu()
    return list(zip(ei[0][direct].tolist(), et[direct].tolist(), ei[1][direct].tolist()))


def _golden_edits(data, batch):
    """Four facts to state -- a direct edge from the first triple's head to its tail, one parallel to a base edge, two more at
    the heads of other triples -- and two stated facts to retract: base facts at the first two triples' heads."""
    base = _golden_facts(data)
    heads = batch[:, 0].tolist()
    at = lambda v: next(f for f in base if v in (f[0], f[2]) and f[0] != f[2])
    adds = [(heads[0], 0, int(batch[0, 1])), at(heads[2]), (heads[3], 2, 17), (33, 4, heads[4])]
    removes = [at(heads[0]), at(heads[1])]
    assert adds[1] in base and len(set(removes)) == 2 and not set(removes) & set(adds)
    return adds, removes


def test_edge_grads_on_the_delta_match_the_materialised_route(dev, monkeypatch):
    """The golden graph and the ultra_3g weights with four facts stated and two retracted: edge_grads_batch(data, batch, delta=)
    against edge_grads_batch(materialize(), batch) column by column, with the project's tolerance for this quantity
    (tests/test_explain_batch_gpu.py: rtol 1e-4, atol 1e-6 max |want|), and both against fp64 autograd on the CPU.  The live
    route sums the terms of the compacting route in another association plus one add per touched row, so its error against
    fp64 may be at most twice the other's."""
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    ent = model.entity_model
    batch = torch.cat([tr["batch"] for tr in vis["triples"]]).to(dev)
    reps = torch.cat([tr["relation_representations"] for tr in vis["triples"]]).to(dev)
    delta = rspmm.GraphDelta(data, capacity=8)
    adds, removes = _golden_edits(data, batch.cpu())
    delta.add(*zip(*adds))
    assert int(delta.remove(*zip(*removes)).sum()) >= 2 and len(delta) == 4 and delta.num_removed >= 4
    mat = delta.materialize()
    ent.query = reps
    want, want_scores = ent.edge_grads_batch(mat, batch)

    def refuse(name):
        def fail(*args, **kwargs):
            raise AssertionError("the live route called %s" % name)
        return fail

    known = set(id(p) for p in rspmm.cached_plans())
    with monkeypatch.context() as patch:
        patch.setattr(ent, "edge_grads", refuse("the per-triple fallback"))
        patch.setattr(rspmm.GraphDelta, "materialize", refuse("GraphDelta.materialize"))
        base_grads, added_grads, scores = ent.edge_grads_batch(data, batch, delta=delta)
        # (the one plan the live route may build is the flipped plan of the BASE edge list, once per base graph)
        new = [p for p in rspmm.cached_plans() if id(p) not in known]
        assert all(p.num_edge == data.num_edges for p in new) and len(new) <= 1
        again = ent.edge_grads_batch(data, batch, delta=delta)
        assert len([p for p in rspmm.cached_plans() if id(p) not in known]) == len(new)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base_grads + added_grads, again[0] + again[1]))
    keep = delta.keep_vector().bool()
    num_added = 2 * len(delta)
    assert len(base_grads) == len(added_grads) == 6 and added_grads[0].shape == (8, 16)
    assert all(not a[:, num_added:].any() for a in added_grads)
    got = [torch.cat([b[:, keep], a[:, :num_added]], dim=1) for b, a in zip(base_grads, added_grads)]
    assert got[0].shape == want[0].shape == (8, mat.num_edges)
    torch.testing.assert_close(scores, want_scores, rtol=1e-5, atol=1e-6)
    for i in range(6):
        for s in range(8):
            torch.testing.assert_close(got[i][s], want[i][s], rtol=1e-4, atol=1e-6 * float(want[i][s].abs().max()))
    assert any(bool(a[:, :num_added].abs().max() > 0) for a in added_grads)      # (the added edges carry gradient)
    # the measured errors of both routes against fp64 autograd
    state = model.state_dict()
    live_err = compact_err = scale = 0.0
    for s in range(8):
        exact = _fp64_edge_grads(state, mat.edge_index.cpu(), mat.edge_type.cpu(), mat.num_nodes, reps[s].cpu(), batch[s].tolist())
        live_err = max(live_err, float((torch.stack([x[s] for x in got]).cpu().double() - exact).abs().max()))
        compact_err = max(compact_err, float((torch.stack([x[s] for x in want]).cpu().double() - exact).abs().max()))
        scale = max(scale, float(exact.abs().max()))
    print("edge gradients against fp64 autograd: live route max |error| = %.3g, compacting route %.3g (max |gradient| %.3g)"
          % (live_err, compact_err, scale))
    assert live_err <= 2 * compact_err


# ---- 4: serving ----
def _edges_of(graph):
    return set(zip(graph.edge_index[0].tolist(), graph.edge_index[1].tolist(), graph.edge_type.tolist()))


def _check_against_fresh(model, p, anchor, relation, retracted, dev):
    """explain_tails / explain_heads(compact=False) of `p`, which holds edits: answers, the delta left alone, no plan and no
    capture, paths over the materialised graph, and the paths and weights of a fresh Predictor on p.materialized()."""
    mat = p.materialized()
    edges = _edges_of(mat)
    num_direct = p.num_direct_relations
    dead = {(h, t, r) for h, r, t in retracted} | {(t, h, r + num_direct) for h, r, t in retracted}
    fresh = predict.Predictor(model, mat, k=p.k, batch_size=p.batch_size)
    total = separated = 0
    for mode in ("tail", "head"):
        ids, scores, count = (x.clone() for x in (p.tails if mode == "tail" else p.heads)(anchor, relation))
        delta, data, version = p.delta, p.data, p.delta.version
        plans, steps = len(rspmm.cached_plans()), dict(p._steps)
        got = (p.explain_tails if mode == "tail" else p.explain_heads)(anchor, relation, compact=False)
        assert p.delta is delta and delta.edited and delta.version == version and p.data is data
        assert len(rspmm.cached_plans()) == plans
        assert p._steps.keys() == steps.keys() and all(p._steps[key] is steps[key] for key in steps)
        assert torch.equal(got[0], ids) and torch.equal(got[2], count)
        assert torch.equal(got[1].view(torch.int32), scores.view(torch.int32))
        want = (fresh.explain_tails if mode == "tail" else fresh.explain_heads)(anchor, relation)
        assert torch.equal(want[0], ids) and torch.equal(want[2], count)
        for i, (per_query, per_query_want) in enumerate(zip(got[3], want[3])):
            assert len(per_query) == len(per_query_want) == int(count[i])
            for j, ((paths, weights), (paths_want, weights_want)) in enumerate(zip(per_query, per_query_want)):
                for path in paths:
                    assert path[0][0] == int(anchor[i]) and path[-1][1] == int(ids[i, j])
                    assert all(a[1] == b[0] for a, b in zip(path, path[1:]))
                    assert all(edge in edges and edge not in dead for edge in path)
                    assert all(0 <= r < 2 * num_direct and max(h, t) < p.num_entities for h, t, r in path)
                separated += _compare_paths(paths, weights, paths_want, weights_want)
                total += len(paths_want)
    fresh.close()
    return total, separated


def _serving_case(dev, **kwargs):
    vis = load()["visualize"]
    data = _golden_data(vis, dev)
    model = _ultra_3g(dev)
    batch = torch.cat([tr["batch"] for tr in vis["triples"]])
    p = predict.Predictor(model, data, k=3, batch_size=2, delta_capacity=8, **kwargs)
    num_direct = data.num_relations // 2
    anchor = torch.tensor([int(batch[0, 0]), int(batch[1, 0])], device=dev)
    relation = torch.tensor([int(batch[0, 2]) % num_direct, int(batch[1, 2]) % num_direct], device=dev)
    # the explanation plan of the base graph is built by the first explanation on it, whatever the route: before the edits
    p.explain_tails(anchor, relation)
    return model, data, batch, p, anchor, relation


def test_predictor_explains_on_the_delta(dev):
    model, data, batch, p, anchor, relation = _serving_case(dev)
    adds, removes = _golden_edits(data, batch)
    assert p.add_facts(*zip(*adds)) == 4
    assert int(p.remove_facts(*zip(*removes)).sum()) >= 2
    total, separated = _check_against_fresh(model, p, anchor, relation, removes, dev)
    assert total > 0 and 4 * separated >= 3 * total, (separated, total)
    # a second add_facts: again no plan, no capture, the delta a delta
    assert p.add_facts([int(anchor[1])], [1], [int(batch[5, 0])]) == 5
    total, separated = _check_against_fresh(model, p, anchor, relation, removes, dev)
    assert total > 0 and 4 * separated >= 3 * total, (separated, total)
    # compact=True is the folding route still
    p.explain_tails(anchor, relation)
    assert not p.delta.edited
    p.close()


def test_predictor_explains_on_the_delta_with_reserves(dev):
    """Reserved entity rows and a reserved relation slot, a new entity and a new relation in use: the served slot-layout graph is
    the base, the paths name the compact numbering of materialized()."""
    model, data, batch, p, anchor, relation = _serving_case(dev, entity_capacity=2, relation_capacity=1)
    adds, removes = _golden_edits(data, batch)
    (entity,), (rel,) = p.add_entities(1).tolist(), p.add_relations(1).tolist()
    assert entity == data.num_nodes and rel == data.num_relations // 2
    adds = adds + [(int(anchor[0]), rel, entity), (entity, 1, int(batch[0, 1]))]
    assert p.add_facts(*zip(*adds)) == 6
    assert int(p.remove_facts(*zip(*removes)).sum()) >= 2
    assert p.num_relation_slots == p.num_direct_relations and p.num_slots == p.num_entities + 1
    total, separated = _check_against_fresh(model, p, anchor, relation, removes, dev)
    assert total > 0 and 4 * separated >= 3 * total, (separated, total)
    p.close()


def test_predictor_explains_on_the_delta_with_a_live_relation_graph(dev):
    model, data, batch, p, anchor, relation = _serving_case(dev, live_relation_graph=True)
    adds, removes = _golden_edits(data, batch)
    assert p.add_facts(*zip(*adds)) == 4
    assert int(p.remove_facts(*zip(*removes)).sum()) >= 2
    total, separated = _check_against_fresh(model, p, anchor, relation, removes, dev)
    assert total > 0 and 4 * separated >= 3 * total, (separated, total)
    p.close()
