"""Leave-one-out verification of stated facts, the parts that need no GPU: the torch restatement of the per-sample keep
mask (BaseNBFNet.leave_one_out_keep on CPU tensors) against a brute-force double loop, the two new C entry points' host-side
validation, and the argument checks of Predictor.verify_* and of the `edge_keep=` forward."""
import ctypes
import os
import re

import pytest
import torch

from ultra_amd import _lib, dense, models, predict, rspmm, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"ultra_rspmm_forward_masked_samples": "ultra_rspmm.h", "ultra_leave_one_out_keep": "ultra_nbfnet.h"}


@pytest.fixture(scope="module")
def kg():
    return synthetic.make_kg(num_node=60, num_triple=400, num_relation_base=3, seed=5)


def brute_force_keep(data, triples, remove_one_hop):
    """keep[s, e] = 0 iff edge e is (h_s, t_s, r_s) or (t_s, h_s, r_s + R / 2); with remove_one_hop iff it joins the two nodes."""
    heads, tails = data.edge_index.tolist()
    types = data.edge_type.tolist()
    half = data.num_relations // 2
    keep = torch.ones(len(triples), len(types))
    for s, (h, t, r) in enumerate(triples.tolist()):
        for e in range(len(types)):
            if remove_one_hop:
                gone = (heads[e], tails[e]) in ((h, t), (t, h))
            else:
                gone = (heads[e], tails[e], types[e]) in ((h, t, r), (t, h, r + half))
            if gone:
                keep[s, e] = 0.0
    return keep


def chosen_triples(data):
    """Six facts of the graph (one of them stated twice, one whose inverse (t, r, h) is also stated directly) and one triple
    the graph does not hold."""
    half = data.num_relations // 2
    n_direct = data.edge_index.shape[1] // 2
    facts = torch.stack([data.edge_index[0, :n_direct], data.edge_index[1, :n_direct], data.edge_type[:n_direct]], dim=-1)
    listed = [tuple(f) for f in facts.tolist()]
    stated = set(listed)
    repeated = next(f for f in listed if listed.count(f) > 1)
    mirrored = next(f for f in listed if (f[1], f[0], f[2]) in stated and f[0] != f[1])
    joined = {(f[0], f[1]) for f in listed} | {(f[1], f[0]) for f in listed}
    absent = next((h, t, 1) for h in range(data.num_nodes) for t in range(data.num_nodes) if (h, t) not in joined)
    picked = [listed[0], listed[7], repeated, mirrored, listed[123], absent]
    return torch.tensor(picked, dtype=torch.long), picked.index(repeated), picked.index(mirrored), picked.index(absent)


@pytest.mark.parametrize("remove_one_hop", [False, True])
def test_leave_one_out_mask_equals_the_double_loop(kg, remove_one_hop):
    triples, i_rep, i_mir, i_absent = chosen_triples(kg)
    net = models.EntityNBFNet(64, [64], remove_one_hop=remove_one_hop)
    got = net.leave_one_out_keep(kg, triples)
    want = brute_force_keep(kg, triples, remove_one_hop)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    dropped = (want == 0).sum(dim=1)
    assert dropped[i_rep] >= 4                        # a fact stated twice: both copies and both inverse edges go
    assert dropped[i_mir] >= 2
    assert torch.equal(got[i_absent], torch.ones(kg.edge_index.shape[1]))      # no edge joins the two nodes: a row of ones
    if not remove_one_hop:
        # the mirrored fact (h, r, t) keeps the DIRECT edge (t, r, h): only (h, t, r) and (t, h, r + R/2) go
        h, t, r = triples[i_mir].tolist()
        twin = ((kg.edge_index[0] == t) & (kg.edge_index[1] == h) & (kg.edge_type == r)).nonzero().flatten()
        assert len(twin) and bool((got[i_mir, twin] == 1).all())
    # every sample alone: row s is what the batch-wide mask of the single triple s is
    for s in range(len(triples)):
        alone = net.easy_edge_mask(kg, triples[s:s + 1, 0], triples[s:s + 1, 1], triples[s:s + 1, 2])
        assert torch.equal(got[s], alone.float())


def test_an_inverse_relation_is_refused(kg):
    net = models.EntityNBFNet(64, [64])
    bad = torch.tensor([[1, 2, kg.num_relations // 2]])
    with pytest.raises(ValueError, match="direct relations"):
        net.leave_one_out_keep(kg, bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        net.leave_one_out_keep(kg, bad[0])


def test_new_symbols_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, header in NEW_SYMBOLS.items():
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, text), "%s is not declared in %s" % (name, header)
        assert hasattr(lib, name), "%s is not exported" % name
    assert _lib.lib.ultra_abi_version() == 7


def test_leave_one_out_entry_validates_sizes_before_pointers():
    lib = _lib.lib
    # (no pointer is valid here: the answers come from the sizes alone)
    rc = lib.ultra_leave_one_out_keep(None, None, None, 100, None, None, None, 1025, 1, 10, 4, 2, None, 100, None)
    assert rc == _lib.ULTRA_ERR_UNSUPPORTED
    assert b"1024" in lib.ultra_last_error()
    rc = lib.ultra_leave_one_out_keep(None, None, None, 100, None, None, None, 4, 1, 10, 4, 2, None, 99, None)
    assert rc == _lib.ULTRA_ERR_INVALID
    assert b"keep_stride" in lib.ultra_last_error()
    rc = lib.ultra_leave_one_out_keep(None, None, None, 100, None, None, None, 4, 1, 10, 4, 2, None, 100, None)
    assert rc == _lib.ULTRA_ERR_INVALID                    # NULL operands
    assert dense.LEAVE_ONE_OUT_MAX_SAMPLES == 1024


def test_masked_samples_entry_validates_on_the_host(kg):
    lib = _lib.lib
    plan = rspmm.Plan(kg.edge_index, kg.edge_type, kg.num_nodes, kg.num_relations, exact_order=True)
    num_edge = kg.edge_index.shape[1]
    x = torch.zeros(2, kg.num_nodes, 64)
    rel = torch.zeros(2, kg.num_relations, 64)
    out = torch.zeros(2, kg.num_nodes, 64)
    keep = torch.ones(2, num_edge)
    mats = [ctypes.byref(rspmm.as_mat(t)[1]) for t in (rel, x, out)]
    # keep_stride < num_edge, a NULL mask, a NULL output: ULTRA_ERR_INVALID before anything is launched (host tensors here)
    rc = lib.ultra_rspmm_forward_masked_samples(plan._h, 0, 0, _lib.F32, keep.data_ptr(), num_edge - 1, mats[0], mats[1], None,
                                                mats[2], None)
    assert rc == _lib.ULTRA_ERR_INVALID and b"keep_stride" in lib.ultra_last_error()
    rc = lib.ultra_rspmm_forward_masked_samples(plan._h, 0, 0, _lib.F32, None, num_edge, mats[0], mats[1], None, mats[2], None)
    assert rc == _lib.ULTRA_ERR_INVALID
    rc = lib.ultra_rspmm_forward_masked_samples(plan._h, 0, 0, _lib.F32, keep.data_ptr(), num_edge, mats[0], mats[1], None, None,
                                                None)
    assert rc == _lib.ULTRA_ERR_INVALID
    rc = lib.ultra_rspmm_forward_masked_samples(None, 0, 0, _lib.F32, keep.data_ptr(), num_edge, mats[0], mats[1], None, mats[2],
                                                None)
    assert rc == _lib.ULTRA_ERR_INVALID
    # n_outer == 0: nothing to do
    empty = rspmm.UltraMat(out.data_ptr(), 0, 0, kg.num_nodes, 64, 64)
    rc = lib.ultra_rspmm_forward_masked_samples(plan._h, 0, 0, _lib.F32, keep.data_ptr(), num_edge, mats[0], mats[1], None,
                                                ctypes.byref(empty), None)
    assert rc == _lib.ULTRA_OK


def test_plan_forward_refuses_per_sample_weights_that_are_not_masks(kg):
    plan = rspmm.Plan(kg.edge_index, kg.edge_type, kg.num_nodes, kg.num_relations, exact_order=True)
    x = torch.zeros(2, kg.num_nodes, 64)
    rel = torch.zeros(2, kg.num_relations, 64)
    with pytest.raises(RuntimeError, match="keep=True"):
        plan.forward(rel, x, edge_weight=torch.ones(2, kg.edge_index.shape[1]))
    with pytest.raises(RuntimeError, match=r"\(n_outer, num_edge\)"):
        plan.forward(rel, x, edge_weight=torch.ones(3, kg.edge_index.shape[1]), keep=True)


def test_verify_argument_checks_need_no_device(kg):
    model = models.Ultra(**synthetic.default_model_cfg()).eval()
    predictor = predict.Predictor(model, kg, batch_size=4)
    h, t, r = kg.target_triples[:5].unbind(-1)
    with pytest.raises(ValueError, match="direct relations"):
        predictor.verify_tails(h, r + kg.num_relations // 2, t)
    with pytest.raises(ValueError, match="direct relations"):
        predictor.verify_heads(h, r + kg.num_relations // 2, t)
    with pytest.raises(ValueError, match="one head, relation and tail per fact"):
        predictor.verify_tails(h, r[:4], t)
    with pytest.raises(ValueError, match="one head, relation and tail per fact"):
        predict.verify_reference(model, kg, kg, h[:2], r, t)
    with pytest.raises(ValueError, match="mode"):
        predict.verify_reference(model, kg, kg, h, r, t, mode="both")


def test_edge_keep_is_refused_outside_inference(kg):
    model = models.Ultra(**synthetic.default_model_cfg())
    batch = kg.target_triples[:2].unsqueeze(1)
    keep = torch.ones(2, kg.edge_index.shape[1])
    model.train()
    with torch.no_grad(), pytest.raises(ValueError, match="eval mode"):
        model(kg, batch, edge_keep=keep)
    with torch.no_grad(), pytest.raises(ValueError, match="eval mode"):
        model.entity_model(kg, torch.zeros(2, kg.num_relations, 64), batch, edge_keep=keep)
    model.eval()
    with pytest.raises(ValueError, match="eval mode"):          # autograd on
        model(kg, batch, edge_keep=keep)
    with torch.no_grad(), pytest.raises(ValueError, match=r"\(batch, num_edge\)"):
        model.entity_model(kg, torch.zeros(2, kg.num_relations, 64), batch, edge_keep=keep[:1])
