"""Serving link-prediction queries, the parts that need no GPU: the plain-torch restatement of the filtered top-k against a
brute-force Python sort, the known-answer lists against a scan of the graph, the C entry point's argument checks, the
vocabulary reader."""
import ctypes
import math
import os

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "kg_fixture")
SPECIAL_ROW = [0., -0., float("nan"), float("inf"), 1., 1., float("-inf"), float("nan"), -1., 0.]
NEG_INF_BITS = torch.tensor(float("-inf")).view(torch.int32).item()


def brute_force_topk(row, k, known=()):
    """ids of the k best candidates of `row` (a list of Python floats) by an explicit sort key: NaN first, then the value
    descending (-0.0 == 0.0 as Python floats), then the id."""
    known = set(int(i) for i in known)
    cand = [i for i in range(len(row)) if i not in known]
    cand.sort(key=lambda i: (0, 0.0, i) if math.isnan(row[i]) else (1, -row[i], i))
    return cand[:k]


def special_mix(shape, gen):
    """Scores from {-1, -.5, 0, .5, 1} with 10 % NaN, 5 % -inf and 5 % -0.0: heavy ties and every special value."""
    pred = torch.randint(-2, 3, shape, generator=gen).float() / 2
    u = torch.rand(shape, generator=gen)
    pred[u < 0.10] = float("nan")
    pred[(u >= 0.10) & (u < 0.15)] = float("-inf")
    pred[(u >= 0.15) & (u < 0.20)] = -0.0
    return pred


def random_known(batch, n, share, gen):
    """(ptr, index): about `share` of the ids of every row, ascending."""
    rows = [torch.nonzero(torch.rand(n, generator=gen) < share).flatten() for _ in range(batch)]
    ptr = torch.zeros(batch + 1, dtype=torch.long)
    ptr[1:] = torch.tensor([len(r) for r in rows]).cumsum(0)
    return ptr, torch.cat(rows) if rows else torch.zeros(0, dtype=torch.long)


def check_against_brute_force(pred, k, ptr, index):
    from ultra_amd import predict
    ids, scores, count = predict.filtered_topk_reference(pred, k, ptr, index)
    assert ids.shape == scores.shape == (pred.shape[0], k) and count.shape == (pred.shape[0],)
    for b in range(pred.shape[0]):
        known = [] if ptr is None else index[int(ptr[b]):int(ptr[b + 1])].tolist()
        want = brute_force_topk(pred[b].tolist(), k, known)
        m = min(k, pred.shape[1] - len(known))
        assert int(count[b]) == m == len(want)
        assert ids[b, :m].tolist() == want
        assert torch.equal(scores[b, :m].view(torch.int32), pred[b, want].view(torch.int32))      # the stored bits
        assert ids[b, m:].tolist() == [-1] * (k - m)                                              # padding
        assert scores[b, m:].view(torch.int32).tolist() == [NEG_INF_BITS] * (k - m)


def test_restatement_on_the_special_value_row():
    from ultra_amd import predict
    pred = torch.tensor([SPECIAL_ROW])
    ids, scores, count = predict.filtered_topk_reference(pred, 10)
    assert ids[0].tolist() == [2, 7, 3, 4, 5, 0, 1, 9, 8, 6]
    assert int(count[0]) == 10
    assert math.copysign(1.0, float(scores[0, 6])) == -1.0      # id 1: -0.0 comes back as -0.0
    for k in (1, 3, 10, 12):
        check_against_brute_force(pred, k, None, None)
        check_against_brute_force(pred, k, torch.tensor([0, 3]), torch.tensor([2, 3, 6]))
    # a filtered candidate is removed; a genuine -inf stays a candidate, ranked last
    ids, scores, count = predict.filtered_topk_reference(pred, 10, torch.tensor([0, 2]), torch.tensor([2, 7]))
    assert ids[0].tolist() == [3, 4, 5, 0, 1, 9, 8, 6, -1, -1] and int(count[0]) == 8
    assert float(scores[0, 7]) == float("-inf") and int(ids[0, 7]) == 6


def test_restatement_on_random_rows_with_ties_and_special_values():
    gen = torch.Generator().manual_seed(20240607)
    rows = 0
    for case in range(50):
        n = int(torch.randint(1, 70, (1,), generator=gen))
        k = int(torch.randint(1, n + 6, (1,), generator=gen))
        pred = special_mix((4, n), gen)
        ptr, index = random_known(4, n, 0.3, gen)
        check_against_brute_force(pred, k, ptr, index)
        rows += 4
    assert rows == 200


def scan_known(data, anchor, relation, mode):
    h, t, r = data.edge_index[0].tolist(), data.edge_index[1].tolist(), data.edge_type.tolist()
    out = []
    for a, q in zip(anchor.tolist(), relation.tolist()):
        if mode == "tail":
            out.append(sorted(set(tt for hh, tt, rr in zip(h, t, r) if hh == a and rr == q)))
        else:
            out.append(sorted(set(hh for hh, tt, rr in zip(h, t, r) if tt == a and rr == q)))
    return out


def ragged(ptr, index):
    return [index[int(ptr[b]):int(ptr[b + 1])].tolist() for b in range(len(ptr) - 1)]


def filter_graphs():
    from ultra_amd import data as udata
    from ultra_amd import synthetic
    yield udata.load_triples_dir(FIXTURE, relation_graph=False).filtered_data
    yield synthetic.make_kg(num_node=50, num_triple=400, num_relation_base=3, num_test=8, seed=5, relation_graph=False)


@pytest.mark.parametrize("which", [0, 1])
def test_known_answers_equal_a_scan_of_the_graph(which):
    from ultra_amd import predict, tasks
    graph = list(filter_graphs())[which]
    gen = torch.Generator().manual_seed(3 + which)
    pick = torch.randperm(graph.edge_index.shape[1], generator=gen)[:24]
    true = torch.stack([graph.edge_index[0, pick], graph.edge_index[1, pick], graph.edge_type[pick]], dim=-1)
    for mode, col in (("tail", 0), ("head", 1)):
        # (anchor, relation) of true triples, then random pairs: some of them have no known answer
        anchor = torch.cat([true[:, col], torch.randint(0, graph.num_nodes, (40,), generator=gen)])
        relation = torch.cat([true[:, 2], torch.randint(0, int(graph.edge_type.max()) + 1, (40,), generator=gen)])
        ptr, index = predict.known_answers(graph, anchor, relation, mode)
        want = scan_known(graph, anchor, relation, mode)
        assert ptr.dtype == index.dtype == torch.long and ptr.shape == (len(anchor) + 1,)
        assert ragged(ptr, index) == want
        assert any(len(w) == 0 for w in want) and all(len(w) > 0 for w in want[:24])
        # a query without a known answer: an empty range
        for b, w in enumerate(want):
            assert int(ptr[b + 1] - ptr[b]) == len(w)
        # true triples of the filter graph: the positive is already listed, so tasks.known_answers says the same
        t_ptr, t_index = tasks.known_answers(graph, true, mode)
        ptr, index = predict.known_answers(graph, true[:, col], true[:, 2], mode)
        assert torch.equal(ptr, t_ptr) and torch.equal(index, t_index)


def test_known_answers_of_queries_outside_the_graph_are_empty():
    from ultra_amd import predict
    graph = list(filter_graphs())[1]
    used = set(zip(graph.edge_index[0].tolist(), graph.edge_type.tolist()))
    free = [(a, q) for a in range(graph.num_nodes) for q in range(3) if (a, q) not in used][:5]
    assert free
    anchor, relation = torch.tensor(free).t()
    ptr, index = predict.known_answers(graph, anchor, relation, "tail")
    assert ptr.tolist() == [0] * (len(free) + 1) and index.numel() == 0


def test_topk_entry_point_checks_its_arguments_without_a_gpu():
    from ultra_amd import _lib
    lib = _lib.lib
    assert lib.ultra_abi_version() == 7
    # k out of range, n_cand >= 2^31: decided before any pointer is looked at
    for k in (0, -1, _lib.TOPK_MAX + 1):
        assert lib.ultra_filtered_topk(None, None, None, 1, 100, k, None, None, None, None, 0, None) == _lib.ULTRA_ERR_UNSUPPORTED
    assert lib.ultra_filtered_topk(None, None, None, 1, 2 ** 31, 10, None, None, None, None, 0, None) == _lib.ULTRA_ERR_UNSUPPORTED
    # a valid k with NULL outputs
    for k in (1, 10, _lib.TOPK_MAX):
        assert lib.ultra_filtered_topk(None, None, None, 1, 100, k, None, None, None, None, 0, None) == _lib.ULTRA_ERR_INVALID
        assert b"ultra_filtered_topk" in lib.ultra_last_error()
    # an empty candidate set and a workspace that is too small (the pointers are not followed: nothing is launched)
    host = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(host)
    assert lib.ultra_filtered_topk(p, None, None, 1, 0, 10, p, p, p, p, 512, None) == _lib.ULTRA_ERR_INVALID
    need = lib.ultra_filtered_topk_workspace(1, 100, 10)
    assert need > 0
    assert lib.ultra_filtered_topk(p, None, None, 1, 100, 10, p, p, p, p, need - 1, None) == _lib.ULTRA_ERR_INVALID
    assert b"workspace" in lib.ultra_last_error()
    assert lib.ultra_filtered_topk(p, None, None, 0, 100, 10, p, p, p, p, 0, None) == _lib.ULTRA_OK      # batch 0


def test_topk_workspace_query():
    from ultra_amd import _lib
    lib = _lib.lib
    c = _lib.TOPK_CHUNK
    sizes = [lib.ultra_filtered_topk_workspace(8, n, 10) for n in (1, 2, c - 1, c, c + 1, 2 * c + 3, 40 * c + 5, 2 * 10 ** 6)]
    assert all(s >= 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # room for k survivors of every chunk of every row
    assert lib.ultra_filtered_topk_workspace(8, 40 * c + 5, 256) >= 8 * 41 * 256 * 8
    assert lib.ultra_filtered_topk_workspace(3, 100, 10) <= lib.ultra_filtered_topk_workspace(8, 100, 10)
    assert lib.ultra_filtered_topk_workspace(-1, 100, 10) < 0
    assert lib.ultra_filtered_topk_workspace(8, -1, 10) < 0
    assert lib.ultra_filtered_topk_workspace(8, 100, -1) < 0
    assert lib.ultra_filtered_topk_workspace(8, 100, 0) < 0
    assert lib.ultra_filtered_topk_workspace(8, 100, _lib.TOPK_MAX + 1) < 0


def test_header_constants_match_the_binding():
    from ultra_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "ultra_nbfnet.h")).read()
    import re
    assert int(re.search(r"#define ULTRA_TOPK_MAX\s+(\d+)", header).group(1)) == _lib.TOPK_MAX == 256
    assert int(re.search(r"#define ULTRA_TOPK_CHUNK\s+(\d+)", header).group(1)) == _lib.TOPK_CHUNK


def test_read_vocab_agrees_with_the_ids_of_load_triples_dir(tmp_path):
    from ultra_amd import data as udata
    ent, rel = udata.read_vocab(FIXTURE)
    data = udata.load_triples_dir(FIXTURE, relation_graph=False)
    assert len(ent) == data.num_nodes and 2 * len(rel) == data.num_relations
    with open(os.path.join(FIXTURE, "test.txt")) as f:
        lines = [line.split() for line in f if len(line.split()) == 3]
    assert len(lines) == len(data.target_triples)
    for (h, r, t), row in zip(lines, data.target_triples.tolist()):
        assert [ent[row[0]], ent[row[1]], rel[row[2]]] == [h, t, r]
    # without .dict files: first-seen order, the same in both readers
    for name in ("train.txt", "valid.txt", "test.txt"):
        with open(os.path.join(FIXTURE, name)) as f, open(tmp_path / name, "w") as g:
            g.write(f.read())
    ent2, rel2 = udata.read_vocab(str(tmp_path))
    data2 = udata.load_triples_dir(str(tmp_path), relation_graph=False)
    assert len(ent2) == data2.num_nodes and 2 * len(rel2) == data2.num_relations
    for (h, r, t), row in zip(lines, data2.target_triples.tolist()):
        assert [ent2[row[0]], ent2[row[1]], rel2[row[2]]] == [h, t, r]
    with open(os.path.join(FIXTURE, "train.txt")) as f:
        first = f.readline().split()
    assert ent2[0] == first[0] and ent2[1] == first[2] and rel2[0] == first[1]


def test_filtered_topk_has_no_cpu_path():
    from ultra_amd import predict
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict.filtered_topk(torch.zeros(2, 5), 3)
    with pytest.raises(ValueError):
        predict.filtered_topk(torch.zeros(2, 5), 0)
