"""Retiring entities from a served graph, the parts that need no GPU: LiveGraph.remove_entities -- the argument
checks, the facts it retracts, the retired state and what survives a compaction and a rebuild --, the `retired=` restatements
against a brute-force loop, Predictor on the CPU route against the definition (a fresh Predictor on materialized(), asked for
k + num_retired answers, the retired ids dropped), and the host side of the ultra_filtered_*_alive entries.

The model is the golden ultra_3g weights under `rotate` messages, the configuration that runs on CPU tensors (test_grow_cpu.py).
A predictor without a reserve and the fresh one it is compared with walk graphs of the SAME row count through the same host
route, so their scores are compared bit for bit here too; with a reserve the row counts differ and test_grow_cpu.py's SCORE_TOL
and its reasoning apply."""
import ctypes
import math
import os
import re

import pytest
import torch

from ultra_amd import _lib, models, predict, synthetic
from ultra_amd import data as udata
from ultra_amd.data import Data
from ultra_amd.live import LiveGraph, retired_words

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIVE_SYMBOLS = ("ultra_filtered_topk_alive", "ultra_filtered_above_alive", "ultra_filtered_rank_alive")
SCORE_TOL = 1e-5        # (test_grow_cpu.py: graphs of different row counts on the host BLAS)


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def served():
    model = models.Ultra(**synthetic.default_model_cfg(message_func="rotate"))
    model.load_state_dict(torch.load(os.path.join(GOLDEN, "ultra_3g_model.pt")))
    data = udata.load_triples_dir(os.path.join(GOLDEN, "kg_fixture"))
    assert data.num_nodes == 300 and data.num_relations == 14 and data.filtered_data is not None
    return model.eval(), data


def degrees(data):
    return torch.bincount(data.edge_index.flatten(), minlength=int(data.num_nodes))


def pick(data):
    """(a leaf, an entity of about the median degree, one more): three distinct ids of the fixture."""
    deg = degrees(data)
    order = torch.argsort(deg, stable=True)
    order = order[deg[order] > 0]
    return int(order[0]), int(order[len(order) // 2]), int(order[len(order) // 2 + 1])


def facts_at(data, ids):
    """The distinct direct triples (h, r, t) of `data` that name one of `ids`, from both columns of the edge list."""
    direct = int(data.num_relations) // 2
    out = set()
    for (row, col), typ in zip(data.edge_index.t().tolist(), data.edge_type.tolist()):
        if row in ids or col in ids:
            out.add((row, typ, col) if typ < direct else (col, typ - direct, row))
    return out


def names(graph, ids):
    return bool(torch.isin(graph.edge_index, torch.as_tensor(list(ids))).any())


# ---- LiveGraph ----
def small_graph():
    """6 nodes, 2 direct relations; closed under inverses but for (4 -> 5, r0), which has no inverse edge."""
    facts = [(0, 0, 1), (1, 1, 2), (2, 0, 3), (3, 1, 0), (1, 0, 4), (2, 1, 5)]
    h, r, t = (torch.tensor(v) for v in zip(*facts))
    edge_index = torch.stack([torch.cat([h, t, torch.tensor([4])]), torch.cat([t, h, torch.tensor([5])])])
    edge_type = torch.cat([r, r + 2, torch.tensor([0])])
    return Data(edge_index=edge_index, edge_type=edge_type, num_nodes=6, num_relations=4)


def test_the_argument_checks():
    live = LiveGraph(small_graph(), delta_capacity=8, entity_capacity=2, delta_policy="eager")
    for bad in (-1, 6, 7, 8, [1, 1], [0, 6]):       # negative, in the reserve, beyond the slots, repeated
        with pytest.raises(ValueError):
            live.remove_entities(bad)
    assert live.num_retired == 0 and live.retired_bits is None and live.retired_count is None
    assert live.remove_entities([]).tolist() == [] and live.num_retired == 0
    assert live.remove_entities(1).tolist() == [3]
    with pytest.raises(ValueError):
        live.remove_entities(1)                      # already retired
    with pytest.raises(ValueError):
        live.remove_entities([2, 1])
    assert live.retired_entities.tolist() == [1] and live.num_retired == 1


def test_a_graph_not_closed_under_inverses_loses_every_edge_at_the_entity():
    data = small_graph()
    for victim, count in ((5, 2), (4, 2)):
        live = LiveGraph(data, delta_capacity=8, delta_policy="eager")
        assert live.remove_entities(victim).tolist() == [count]
        mat = live.materialized()
        assert mat.num_nodes == 6 and not names(mat, [victim])
        # every other edge is still there, in its order
        keep = ~((data.edge_index == victim).any(dim=0))
        assert torch.equal(mat.edge_index, data.edge_index[:, keep]) and torch.equal(mat.edge_type, data.edge_type[keep])
        assert mat.retired_entities.tolist() == [victim]


def test_the_counts_and_the_retired_state():
    data = small_graph()
    live = LiveGraph(data, delta_capacity=16, entity_capacity=30, delta_policy="eager", keep_filter=True)
    assert live.add_facts([0, 2], [1, 1], [2, 2]) == 2           # (0, r1, 2) and the loop (2, r1, 2): held delta facts
    before = facts_at(live.materialized(), {2, 5})
    assert len(before) == 6
    got = live.remove_entities([5, 2])
    assert got.dtype == torch.long and got.tolist() == [2, 5]        # (2, r1, 5) names both ids: counted for each
    assert live.retired_entities.tolist() == [2, 5] and live.retired_entities.dtype == torch.long and live.num_retired == 2
    assert len(live.delta) == 0                                      # the delta facts that named 2 are gone
    mat = live.materialized()
    assert not names(mat, [2, 5]) and not names(live.filter_graph, [2, 5]) and mat.num_nodes == 6
    assert mat.retired_entities.tolist() == [2, 5]
    # the bitmap: uint32 words over the SLOTS, id v bit v & 31 of word v >> 5; one device int64
    bits, count = live.retired_bits, live.retired_count
    assert bits.dtype == torch.int32 and bits.numel() == math.ceil(36 / 32) == 2 and bits.tolist() == [(1 << 2) | (1 << 5), 0]
    assert count.dtype == torch.long and count.tolist() == [2]
    # a later retirement writes into the same tensors; compaction keeps them and the retired rows stay isolated slots
    assert live.remove_entities(0).tolist() == [2]
    assert live.retired_bits is bits and live.retired_count is count and bits.tolist() == [0b100101, 0] and int(count) == 3
    live.compact()
    assert not live.delta.edited and live.retired_bits is bits and live.retired_count is count and int(count) == 3
    assert live.num_entities == 6 and live.retired_entities.tolist() == [0, 2, 5] and not names(live.graph, [0, 2, 5])
    for call in (live.add_facts, live.remove_facts):
        for h, t in ((2, 1), (1, 2)):
            with pytest.raises(ValueError, match="retired"):
                call(h, 0, t)
    # a rebuild that changes the slot count lays a longer bitmap out, the bits copied
    new = live.add_entities(31)
    assert new.tolist() == list(range(6, 37)) and live.num_slots == 37 + 30
    assert live.retired_bits.numel() == 3 and live.retired_bits.tolist() == [0b100101, 0, 0] and int(live.retired_count) == 3
    live.remove_entities(36)
    assert live.retired_bits.tolist() == [0b100101, 1 << 4, 0] and live.retired_entities.tolist() == [0, 2, 5, 36]
    with pytest.raises(ValueError, match="retired"):
        live.add_facts(36, 0, 1)


def test_bit_31_of_a_word():
    words = retired_words(torch.tensor([31, 32, 95]), 96)
    assert words.dtype == torch.int32 and (words.long() & 0xffffffff).tolist() == [1 << 31, 1, 1 << 31]


def test_retiring_on_the_fixture_graph(served):
    _, data = served
    leaf, median, other = pick(data)
    live = LiveGraph(data, delta_capacity=256, filter_data=data.filtered_data, keep_filter=True, delta_policy="eager")
    stated = (leaf, 3, other)
    live.add_facts(*stated)
    want = facts_at(live.materialized(), {median, other})
    assert stated in want
    per_id = [len(facts_at(live.materialized(), {v})) for v in (median, other)]
    assert live.remove_entities([median, other]).tolist() == per_id
    assert len(live.delta) == 0                                          # the delta fact named `other`
    mat = live.materialized()
    assert mat.num_nodes == 300 and not names(mat, [median, other]) and not names(mat.filtered_data, [median, other])
    assert not names(live.filter_graph, [median, other])
    assert facts_at(data, set(range(300))) - want == facts_at(mat, set(range(300)))
    assert mat.retired_entities.tolist() == sorted([median, other])
    # larger than the capacity: folded, the same materialised graph
    tiny = LiveGraph(data, delta_capacity=2, filter_data=data.filtered_data, keep_filter=True, delta_policy="eager")
    tiny.add_facts(*stated)
    assert tiny.remove_entities([median, other]).tolist() == per_id
    assert not tiny.delta.edited and not names(tiny.graph, [median, other])
    folded = tiny.materialized()
    assert torch.equal(folded.edge_index, mat.edge_index) and torch.equal(folded.edge_type, mat.edge_type)
    assert torch.equal(folded.filtered_data.edge_index, mat.filtered_data.edge_index)
    assert folded.retired_entities.tolist() == mat.retired_entities.tolist()


# ---- the restatements ----
def brute(pred, ptr, index, retired, num_live):
    """Per row the candidate ids in answer order: not known, not retired, below num_live; stable descending, NaN on top."""
    n = pred.shape[1] if num_live is None else num_live
    rows = []
    for b in range(pred.shape[0]):
        known = set(index[int(ptr[b]):int(ptr[b + 1])].tolist())

        def key(v, b=b):
            x = float(pred[b, v])
            return (0, 0.0, v) if math.isnan(x) else (1, -x, v)
        rows.append(sorted((v for v in range(n) if v not in known and v not in retired), key=key))
    return rows


@pytest.fixture(scope="module")
def matrix():
    gen = torch.Generator().manual_seed(28)
    pred = torch.randint(-2, 3, (3, 70), generator=gen).float() / 2         # heavy ties
    pred[0, 9], pred[1, 33], pred[2, 64] = float("nan"), float("-inf"), float("nan")
    pred[1, 2] = float("-inf")
    rows = [torch.tensor([3, 17, 40]), torch.zeros(0, dtype=torch.long), torch.tensor([0, 1, 62])]
    ptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0)
    return pred, ptr, torch.cat(rows)


@pytest.mark.parametrize("num_live", [None, 63])
@pytest.mark.parametrize("retired", [[], [9], [2, 31, 32, 33], [4, 5, 61, 64, 69]])
def test_the_restatements_with_retired_against_a_brute_force_loop(matrix, retired, num_live):
    pred, ptr, index = matrix
    gone = torch.tensor(retired, dtype=torch.long)
    n = 70 if num_live is None else num_live
    below = [v for v in retired if v < n]
    poisoned = pred.clone()
    poisoned[:, gone] = float("nan")            # whatever a retired column holds reaches no output
    rows = brute(pred, ptr, index, set(retired), num_live)
    kwargs = {} if num_live is None else {"num_live": num_live}
    for k in (1, 10, 256):
        for scores in (pred, poisoned):
            ids, top, count = predict.filtered_topk_reference(scores, k, ptr, index, retired=gone, **kwargs)
            for b, row in enumerate(rows):
                m = min(k, len(row))
                assert int(count[b]) == m == min(k, n - len(below) - int(ptr[b + 1] - ptr[b]))
                assert ids[b, :m].tolist() == row[:m] and ids[b, m:].eq(-1).all() and top[b, m:].eq(float("-inf")).all()
                assert torch.equal(top[b, :m].view(torch.int32), pred[b, row[:m]].view(torch.int32))
    for thr in (0.0, float("-inf")):
        out_ptr, ids, top, size = predict.filtered_above_reference(poisoned, thr, ptr, index, retired=gone, **kwargs)
        for b, row in enumerate(rows):
            members = [v for v in row if float(pred[b, v]) > thr]
            assert ids[int(out_ptr[b]):int(out_ptr[b + 1])].tolist() == members
            assert torch.equal(top[int(out_ptr[b]):int(out_ptr[b + 1])].view(torch.int32), pred[b, members].view(torch.int32))
            everyone = [v for v in range(n) if v not in retired and float(pred[b, v]) > thr]
            assert int(size[b]) == len(everyone)                         # before the filter, without the retired
    pos = torch.tensor([17, 20, 62])
    r_rows = [torch.tensor([3, 17, 40]), torch.tensor([20]), torch.tensor([0, 1, 62])]
    r_ptr, r_index = torch.tensor([0] + [len(r) for r in r_rows]).cumsum(0), torch.cat(r_rows)
    rank, neg = predict.filtered_rank_reference(poisoned, pos, r_ptr, r_index, retired=gone, **kwargs)
    for b, row in enumerate(brute(pred, r_ptr, r_index, set(retired), num_live)):
        assert int(neg[b]) == len(row) == n - len(below) - int(r_ptr[b + 1] - r_ptr[b])
        assert int(rank[b]) == 1 + sum(1 for v in row if float(pred[b, v]) >= float(pred[b, pos[b]]))
    with pytest.raises(ValueError):             # a known id that is retired breaks the contract: refused, not miscounted
        predict.filtered_topk_reference(pred, 5, ptr, index, retired=torch.tensor([17]))


# ---- Predictor, the CPU route ----
def definition(fresh, live, call, anchor, relation):
    """Item 1 of the definition: the fresh predictor asked for k + num_retired answers, the retired ids dropped, the first k."""
    ids, scores, _ = getattr(fresh, call)(anchor, relation)
    k, retired = live.k, live.retired_entities
    out_ids = torch.full((len(anchor), k), -1, dtype=torch.long)
    out_scores = torch.full((len(anchor), k), float("-inf"))
    for b in range(len(anchor)):
        keep = (ids[b] >= 0) & ~torch.isin(ids[b], retired)
        m = min(k, int(keep.sum()))
        out_ids[b, :m], out_scores[b, :m] = ids[b][keep][:m], scores[b][keep][:m]
    return out_ids, out_scores


@pytest.mark.parametrize("reserve", [0, 8])
def test_predictor_equals_the_definition_on_the_cpu_route(served, reserve):
    model, data = served
    leaf, median, other = pick(data)
    live = predict.Predictor(model, data, k=10, batch_size=4, entity_capacity=reserve)
    assert live.num_retired == 0 and live.retired_entities.numel() == 0
    if reserve:
        (new,) = live.add_entities().tolist()
        live.add_facts([new, leaf], [1, 3], [median, other])
    else:
        live.add_facts(leaf, 3, other)
    counts = live.remove_entities([leaf, median, other])
    assert counts.dtype == torch.long and bool((counts > 0).all())
    assert live.num_retired == 3 and live.retired_entities.tolist() == sorted([leaf, median, other])
    n = 300 + (1 if reserve else 0)
    assert live.num_entities == n
    mat = live.materialized()
    assert mat.num_nodes == n and not names(mat, [leaf, median, other])
    fresh = predict.Predictor(model, mat, k=10 + 3, batch_size=4)
    h, t, r = data.target_triples[:12].unbind(-1)
    ok = ~(torch.isin(h, live.retired_entities) | torch.isin(t, live.retired_entities))
    h, t, r = h[ok][:6], t[ok][:6], r[ok][:6]
    assert len(h) == 6
    for call, anchor in (("tails", h), ("heads", t)):
        ids, scores, count = getattr(live, call)(anchor, r)
        want_ids, want_scores = definition(fresh, live, call, anchor, r)
        assert torch.equal(ids, want_ids), call
        if reserve:
            assert torch.allclose(scores, want_scores, rtol=0.0, atol=SCORE_TOL), call
        else:
            assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32)), call
        assert not bool(torch.isin(ids, live.retired_entities).any())
        ptr, _ = predict.known_answers(live.filter_graph, anchor, r, "tail" if call == "tails" else "head")
        assert count.tolist() == [min(10, n - 3 - int(ptr[b + 1] - ptr[b])) for b in range(6)]
    # the answer sets: the _reference twin on the fresh predictor's own scores
    with torch.no_grad():
        pred = model(mat, predict._candidates(mat, h, r, "tail")).float()
    ptr, index = predict.known_answers(live.filter_graph, h, r, "tail")
    want = predict.filtered_above_reference(pred, -1e30, ptr, index, retired=live.retired_entities)
    got = live.tails_above(h, r, -1e30)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    assert got[3].tolist() == [n - 3] * 6 and not bool(torch.isin(got[1], live.retired_entities).any())
    # (verify_*: per-sample keep masks have no host route under `rotate` messages -- its ranks are checked in test_retire_gpu.py)
    # a retired id is no entity any more
    for victim in (leaf, median, other):
        for call in (live.tails, live.heads):
            with pytest.raises(ValueError, match="retired"):
                call([victim], [0])
        with pytest.raises(ValueError, match="retired"):
            live.tails_above([victim], [0], 0.0)
        with pytest.raises(ValueError, match="retired"):
            live.verify_tails([victim], [0], [int(h[0])])
        with pytest.raises(ValueError, match="retired"):
            live.add_facts(victim, 0, int(h[0]))
        with pytest.raises(ValueError, match="retired"):
            live.add_facts(int(h[0]), 0, victim)
        with pytest.raises(ValueError, match="retired"):
            live.remove_facts(int(h[0]), 0, victim)
        with pytest.raises(ValueError):
            live.remove_entities(victim)
    # compaction keeps the retired set and the answers
    before = live.tails(h, r)
    live.compact()
    assert live.num_retired == 3 and live.num_entities == n
    after = live.tails(h, r)
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2])


def test_query_predictor_does_not_forward_remove_entities():
    from ultra_amd import query_predict
    assert not hasattr(query_predict.QueryPredictor, "remove_entities")


# ---- the ABI ----
def test_the_header_declares_the_alive_entries_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "ultra_nbfnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ALIVE_SYMBOLS:
        decl = re.search(r"int32_t %s\(([^;]*)\);" % name, text)
        assert decl, name
        assert "const uint32_t *retired_bits" in decl.group(1) and "const int64_t *n_retired" in decl.group(1)
        assert "const int64_t *n_live" in decl.group(1)
        assert hasattr(lib, name), name
    assert _lib.lib.ultra_abi_version() == 7


def test_the_alive_entries_refuse_null_operands_on_the_host():
    """NULL retired_bits or n_retired: ULTRA_ERR_INVALID before any GPU call (no device is touched here)."""
    lib = _lib.lib
    one = ctypes.c_void_p(8)        # (a non-NULL address that is never dereferenced: the check comes first)
    for bits, count in ((None, one), (one, None), (None, None)):
        rc = lib.ultra_filtered_topk_alive(one, None, None, 1, 70, 10, one, one, one, one, 1 << 20, None, bits, count, None)
        assert rc == _lib.ULTRA_ERR_INVALID and b"ultra_filtered_topk_alive" in lib.ultra_last_error()
        rc = lib.ultra_filtered_above_alive(one, None, None, 1, 70, 0.0, one, one, one, 70, one, one, 1 << 20, None, bits, count, None)
        assert rc == _lib.ULTRA_ERR_INVALID and b"ultra_filtered_above_alive" in lib.ultra_last_error()
        rc = lib.ultra_filtered_rank_alive(one, one, one, one, 1, 70, one, one, None, bits, count, None)
        assert rc == _lib.ULTRA_ERR_INVALID and b"ultra_filtered_rank_alive" in lib.ultra_last_error()
    # the parent's UNSUPPORTED cases come first, as for the _live twins
    assert lib.ultra_filtered_topk_alive(None, None, None, 1, 70, 0, None, None, None, None, 0, None, None, None, None) \
        == _lib.ULTRA_ERR_UNSUPPORTED
