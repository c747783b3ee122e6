"""A relation graph kept current in place, as far as it shows without a GPU: the flag's default and argument
checks, the CPU fall-back to the flag-off route, tasks.LiveRelationGraph's snapshot / lazy edge list on hand-made bits, and the
two new entry points' host-visible argument checks."""
import ctypes
import inspect

import pytest
import torch

from ultra_amd import _lib, live, models, predict, rspmm, synthetic, tasks


def make_graph(seed=5):
    return synthetic.make_kg(30, 80, 4, seed=seed)


def test_the_flag_defaults_to_false_everywhere():
    for fn in (rspmm.GraphDelta.__init__, live.LiveGraph.__init__, predict.Predictor.__init__):
        assert inspect.signature(fn).parameters["live_relation_graph"].default is False
    data = make_graph()
    assert rspmm.GraphDelta(data).live_relation_graph is False
    assert live.LiveGraph(data).live_relation_graph is False
    model = models.Ultra(**synthetic.default_model_cfg()).eval()
    assert predict.Predictor(model, data).live_relation_graph is False


@pytest.mark.parametrize("bad", [1, 0, None, "yes"])
def test_the_flag_is_a_bool(bad):
    data = make_graph()
    model = models.Ultra(**synthetic.default_model_cfg()).eval()
    for make in (lambda: rspmm.GraphDelta(data, live_relation_graph=bad), lambda: live.LiveGraph(data, live_relation_graph=bad),
                 lambda: predict.Predictor(model, data, live_relation_graph=bad)):
        with pytest.raises(ValueError, match="live_relation_graph"):
            make()


def test_a_model_that_does_not_qualify_is_named():
    data = make_graph()
    good = models.Ultra(**synthetic.default_model_cfg()).eval()
    assert predict.live_relation_graph_supported(good) and predict.live_relation_graph_blocker(good) is None
    bad = models.Ultra(**synthetic.default_model_cfg(aggregate_func="max")).eval()
    assert not predict.live_relation_graph_supported(bad)
    with pytest.raises(ValueError, match=r"relation_model\.layers\.0 \(max aggregate"):
        predict.Predictor(bad, data, live_relation_graph=True)
    predict.Predictor(bad, data)        # (flag off: served as before)
    assert not predict.live_relation_graph_supported(torch.nn.Linear(2, 2))


def test_on_the_cpu_the_flag_takes_the_route_of_before():
    data = make_graph()
    on, off = rspmm.GraphDelta(data, live_relation_graph=True), rspmm.GraphDelta(data)
    for delta in (on, off):
        delta.add([0, 3], [1, 2], [5, 7])
        delta.add(9, 0, 11)
        delta.remove(0, 1, 5)
    assert not isinstance(on.relation_graph, tasks.LiveRelationGraph) and on._resident is None
    assert torch.equal(on.relation_graph.edge_index, off.relation_graph.edge_index)
    assert torch.equal(on.relation_graph.edge_type, off.relation_graph.edge_type)
    a, b = on.materialize(), off.materialize()
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_type, b.edge_type)
    # ... and through the owner of the state (a qualifying model has no CPU path to answer with: the graphs are compared)
    got, want = live.LiveGraph(data, live_relation_graph=True, relation_capacity=2), live.LiveGraph(data, relation_capacity=2)
    for g in (got, want):
        (new,) = g.add_relations(1).tolist()
        g.add_facts([0, 3], [new, 2], [5, 7])
        g.remove_facts(3, 2, 7)
    a, b = got.materialized(), want.materialized()
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_type, b.edge_type)
    assert torch.equal(a.relation_graph.edge_index, b.relation_graph.edge_index)
    assert torch.equal(a.relation_graph.edge_type, b.relation_graph.edge_type)


def hand_made_bits():
    """5 nodes, one word: hh 1 -> {2, 4}, tt 0 -> {0}, th 4 -> {0, 3}."""
    adj = torch.zeros(4, 5, 1, dtype=torch.int32)
    adj[0, 1, 0] = 0b10100
    adj[1, 0, 0] = 0b00001
    adj[3, 4, 0] = 0b01001
    return adj


def test_live_relation_graph_emits_its_edges_lazily_and_per_version():
    adj = hand_made_bits()
    rg = tasks.LiveRelationGraph(adj, None)
    assert rg.adjacency_bits is adj and rg.num_nodes == 5 and rg.num_relations == 4 and rg.version == 0
    assert rg.dense_adjacency is None       # (bits on the CPU: no kernel reads it)
    assert rg._edges is None                # (nothing is emitted until someone asks)
    # the reference's order: the hh, tt, ht, th blocks, each sorted by (row, col)
    assert rg.edge_index.tolist() == [[1, 1, 0, 4, 4], [2, 4, 0, 0, 3]] and rg.edge_type.tolist() == [0, 0, 1, 3, 3]
    assert rg.num_edges == 5 and rg.edge_index is rg.edge_index       # (kept while the version stays)
    held_index, held_type = rg.edge_index, rg.edge_type
    adj[2, 3, 0] |= 0b00010         # the owner writes in place and says so
    rg.changed()
    assert rg.version == 1
    assert rg.edge_index.tolist() == [[1, 1, 0, 3, 4, 4], [2, 4, 0, 1, 0, 3]] and rg.edge_type.tolist() == [0, 0, 1, 2, 3, 3]
    assert held_index.tolist() == [[1, 1, 0, 4, 4], [2, 4, 0, 0, 3]] and held_type.tolist() == [0, 0, 1, 3, 3]


def test_a_snapshot_is_never_written_by_a_later_change():
    adj = hand_made_bits()
    rg = tasks.LiveRelationGraph(adj, None)
    snap = rg.snapshot()
    assert snap is rg.snapshot()        # (one per version)
    assert not isinstance(snap, tasks.LiveRelationGraph) and snap.num_nodes == 5 and snap.num_relations == 4
    assert snap.adjacency_bits is not adj and torch.equal(snap.adjacency_bits, adj)
    before = (snap.edge_index.clone(), snap.edge_type.clone(), snap.adjacency_bits.clone())
    adj[2, 3, 0] |= 0b00010
    rg.changed()
    later = rg.snapshot()
    assert later is not snap and later.edge_index.shape[1] == 6 and torch.equal(later.adjacency_bits, adj)
    assert torch.equal(snap.edge_index, before[0]) and torch.equal(snap.edge_type, before[1])
    assert torch.equal(snap.adjacency_bits, before[2])


def test_live_relation_graph_checks_its_bits():
    with pytest.raises(ValueError, match="bit matrices"):
        tasks.LiveRelationGraph(torch.zeros(4, 5, 2, dtype=torch.int32), None)
    with pytest.raises(ValueError, match="bit matrices"):
        tasks.LiveRelationGraph(torch.zeros(4, 5, 1, dtype=torch.int64), None)
    with pytest.raises(ValueError, match="edge counts"):
        tasks.LiveRelationGraph(hand_made_bits(), torch.zeros(7, dtype=torch.long))


def test_the_relation_table_key_carries_the_version():
    model = models.Ultra(**synthetic.default_model_cfg()).eval()
    rg = tasks.LiveRelationGraph(hand_made_bits(), None)
    key = model._relation_table_key(rg)
    rg.changed()
    assert model._relation_table_key(rg) != key and model._relation_table_key(rg)[0] == key[0]


def mat(n_outer, n_row, row_len, address=4096):
    """An ultra_mat over memory that is never read: the checks below answer before anything is launched."""
    return _lib.UltraMat(address, n_outer, n_row * row_len, n_row, row_len, row_len)


def test_the_library_exports_the_two_entry_points_and_they_check_what_the_host_sees():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ultra_nbf_dense_layer_adjacency") and hasattr(lib, "ultra_nbf_dense_layer0_adjacency")
    lib = _lib.lib
    assert lib.ultra_abi_version() == 7       # (symbols added, none changed)
    order = _lib.LAYER_REFERENCE_ORDER
    rel, x, out = mat(2, 4, 64), mat(2, 20, 64), mat(2, 20, 64, 8192)
    ref = ctypes.byref

    def layer(a_ex, n, flags, out=out):
        return lib.ultra_nbf_dense_layer_adjacency(a_ex, n, ref(rel), ref(x), None, None, 4096, None, None, None, 1e-5, flags,
                                                   ref(out), None)

    assert layer(None, 20, order) == _lib.ULTRA_ERR_INVALID and b"adjacency is NULL" in lib.ultra_last_error()
    assert layer(4096, 0, order) == _lib.ULTRA_ERR_INVALID
    assert layer(4096, -3, order) == _lib.ULTRA_ERR_INVALID
    assert layer(4096, _lib.DENSE_MAX_IN_ROW + 1, order) == _lib.ULTRA_ERR_INVALID and b"1024" in lib.ultra_last_error()
    assert layer(4096, 20, 0) == _lib.ULTRA_ERR_INVALID and b"REFERENCE_ORDER" in lib.ultra_last_error()
    # (the operand checks of ultra_nbf_dense_layer: 21 rows asked of matrices of 20; LayerNorm without its vectors)
    assert layer(4096, 21, order) == _lib.ULTRA_ERR_INVALID
    assert layer(4096, 20, order | 1) == _lib.ULTRA_ERR_INVALID and b"LayerNorm" in lib.ultra_last_error()

    def layer0(a_ex, n, flags, out=out, src=4096, weight=4096):
        return lib.ultra_nbf_dense_layer0_adjacency(a_ex, n, ref(rel), src, None, weight, None, None, None, 1e-5, flags, ref(out),
                                                    None)

    assert layer0(None, 20, 0) == _lib.ULTRA_ERR_INVALID and b"adjacency is NULL" in lib.ultra_last_error()
    assert layer0(4096, 0, 0) == _lib.ULTRA_ERR_INVALID
    assert layer0(4096, _lib.DENSE_MAX_IN_ROW + 1, 0) == _lib.ULTRA_ERR_INVALID
    assert layer0(4096, 20, 64) == _lib.ULTRA_ERR_INVALID and b"unknown flag" in lib.ultra_last_error()
    assert layer0(4096, 20, 0, src=None) == _lib.ULTRA_ERR_INVALID
    assert layer0(4096, 20, 0, weight=None) == _lib.ULTRA_ERR_INVALID
    assert layer0(4096, 20, 1) == _lib.ULTRA_ERR_INVALID and b"LayerNorm" in lib.ultra_last_error()
    assert layer0(4096, 20, _lib.LAYER0_MAX) == _lib.ULTRA_ERR_UNSUPPORTED      # (the sum aggregate only)
    assert layer0(4096, 20, 0, out=mat(2, 20, 32, 8192)) == _lib.ULTRA_ERR_UNSUPPORTED and b"64" in lib.ultra_last_error()
    assert layer0(4096, 21, 0) == _lib.ULTRA_ERR_INVALID      # (an output of 20 rows)
