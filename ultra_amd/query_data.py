"""Complex logical query data: a loader of BetaE-format directories and a seeded synthetic sampler (reference:
ultra/datasets_query.py).  Nothing is downloaded.

A BetaE directory holds train.txt (`h r t` id triples, inverse relations included), id2ent.pkl / id2rel.pkl (or stats.txt
with `numentity:` / `numrelations:`) and, per split, {split}-queries.pkl (query structure -> set of nested queries),
{split}-easy-answers.pkl and {split}-hard-answers.pkl (nested query -> set of entity ids).  The graph of every split is the
training graph, as in the reference.
"""
import os
import pickle
import random

import torch
from torch.nn import functional as F
from torch.utils import data as torch_data

from . import tasks
from .data import Data
from .ultraquery import Query

# query structures of BetaE ("e" entity, "r" relation projection, "n" negation, "u" union) and their type names
STRUCT2TYPE = {
    ("e", ("r",)): "1p",
    ("e", ("r", "r")): "2p",
    ("e", ("r", "r", "r")): "3p",
    (("e", ("r",)), ("e", ("r",))): "2i",
    (("e", ("r",)), ("e", ("r",)), ("e", ("r",))): "3i",
    ((("e", ("r",)), ("e", ("r",))), ("r",)): "ip",
    (("e", ("r", "r")), ("e", ("r",))): "pi",
    (("e", ("r",)), ("e", ("r", "n"))): "2in",
    (("e", ("r",)), ("e", ("r",)), ("e", ("r", "n"))): "3in",
    ((("e", ("r",)), ("e", ("r", "n"))), ("r",)): "inp",
    (("e", ("r", "r")), ("e", ("r", "n"))): "pin",
    (("e", ("r", "r", "n")), ("e", ("r",))): "pni",
    (("e", ("r",)), ("e", ("r",)), ("u",)): "2u-DNF",
    ((("e", ("r",)), ("e", ("r",)), ("u",)), ("r",)): "up-DNF",
}
TYPE2STRUCT = {v: k for k, v in STRUCT2TYPE.items()}
ID2TYPE = sorted(STRUCT2TYPE.values())


class QueryDataset(torch_data.Dataset):
    """Queries with their answers; an item is the reference's dict (datasets_query.py:166-175): `query` (postfix, padded
    with stop to the longest query), `type` (index into id2type), `easy_answer` / `hard_answer` (num_nodes,) masks."""

    def __init__(self, queries, types, easy_answers, hard_answers, num_nodes, id2type=ID2TYPE):
        self.nested = [None if isinstance(q, Query) else q for q in queries]      # the BetaE tuples, where given
        self.queries = [q if isinstance(q, Query) else Query.from_nested(q) for q in queries]
        self.types = list(types)
        self.easy_answers = [sorted(a) for a in easy_answers]
        self.hard_answers = [sorted(a) for a in hard_answers]
        self.num_nodes = int(num_nodes)
        self.id2type = list(id2type)
        self.max_query_length = max((len(q) for q in self.queries), default=1)

    def __len__(self):
        return len(self.queries)

    def __getitem__(self, index):
        query = self.queries[index].as_subclass(torch.Tensor)
        return {
            "query": F.pad(query, (0, self.max_query_length - len(query)), value=Query.stop),
            "type": self.types[index],
            "easy_answer": _mask(self.easy_answers[index], self.num_nodes),
            "hard_answer": _mask(self.hard_answers[index], self.num_nodes),
        }


def _mask(ids, n):
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.tensor(ids, dtype=torch.long)] = True
    return m


def load_betae(root, split="test", query_types=None):
    """(graph, QueryDataset) of one split of a local BetaE directory ("train", "valid" or "test"; the train split reads
    train-answers.pkl as easy answers and has no hard ones).  query_types: type names to keep (default: the 14 of ID2TYPE).  The graph carries its relation graph; id2type is sorted as in the reference."""
    num_node, num_rel = _read_sizes(root)
    h, r, t = [], [], []
    with open(os.path.join(root, "train.txt")) as fin:
        for line in fin:
            if line.strip():
                a, b, c = (int(x) for x in line.split())
                h.append(a), r.append(b), t.append(c)
    graph = Data(edge_index=torch.tensor([h, t], dtype=torch.long), edge_type=torch.tensor(r, dtype=torch.long),
                 num_nodes=num_node, num_relations=num_rel, inverse_rel_plus_one=True)
    tasks.build_relation_graph(graph)
    id2type = sorted(query_types) if query_types else ID2TYPE
    type2id = {name: i for i, name in enumerate(id2type)}
    with open(os.path.join(root, "%s-queries.pkl" % split), "rb") as fin:
        struct2queries = pickle.load(fin)
    if split == "train":
        # the training split has one answer file, its answers are all easy (datasets_query.py:133-135)
        with open(os.path.join(root, "train-answers.pkl"), "rb") as fin:
            easy = pickle.load(fin)
        hard = {}
    else:
        with open(os.path.join(root, "%s-easy-answers.pkl" % split), "rb") as fin:
            easy = pickle.load(fin)
        with open(os.path.join(root, "%s-hard-answers.pkl" % split), "rb") as fin:
            hard = pickle.load(fin)
    queries, types, easy_answers, hard_answers = [], [], [], []
    for struct, qs in struct2queries.items():
        name = STRUCT2TYPE.get(struct)
        if name not in type2id:
            continue
        for q in sorted(qs):
            queries.append(q)
            types.append(type2id[name])
            easy_answers.append(easy.get(q, set()))
            hard_answers.append(hard.get(q, set()))
    return graph, QueryDataset(queries, types, easy_answers, hard_answers, num_node, id2type)


def _read_sizes(root):
    ent, rel = os.path.join(root, "id2ent.pkl"), os.path.join(root, "id2rel.pkl")
    if os.path.exists(ent) and os.path.exists(rel):
        with open(ent, "rb") as f1, open(rel, "rb") as f2:
            return len(pickle.load(f1)), len(pickle.load(f2))
    stats = {}
    with open(os.path.join(root, "stats.txt")) as fin:
        for line in fin:
            if ":" in line:
                k, v = line.split(":", 1)
                stats[k.strip()] = int(v)
    return stats["numentity"], stats["numrelations"]


# ---- synthetic queries ----

class _Adjacency(object):
    def __init__(self, edge_index, edge_type, num_node):
        self.num_node = num_node
        self.out, self.inn = {}, {}
        for u, v, r in zip(edge_index[0].tolist(), edge_index[1].tolist(), edge_type.tolist()):
            self.out.setdefault((u, r), set()).add(v)
            self.inn.setdefault(v, []).append((u, r))

    def project(self, nodes, r):
        out = set()
        for u in nodes:
            out |= self.out.get((u, r), set())
        return out


def answer_set(nested, adj):
    """The exact answers of a nested query on a graph (the set semantics the fuzzy logic relaxes)."""
    if len(nested) == 2 and isinstance(nested[-1][-1], int):
        var, ops = nested
        cur = answer_set(var, adj) if isinstance(var, tuple) else {var}
        for op in ops:
            cur = set(range(adj.num_node)) - cur if op == -2 else adj.project(cur, op)
        return cur
    if len(nested[-1]) > 1:
        sets = [answer_set(b, adj) for b in nested]
        return set.intersection(*sets)
    return set.union(*[answer_set(b, adj) for b in nested[:-1]])


def _ground(struct, target, adj, rng):
    """Nested query of `struct` with ids, walking back from `target` so that target answers its positive part."""
    if len(struct) == 2 and isinstance(struct[-1][-1], str) and struct[-1][-1] in ("r", "n"):
        var, ops = struct
        ids = []
        for op in reversed(ops):
            if op == "n":
                target = rng.randrange(adj.num_node)      # the negated branch: an unrelated set
                ids.append(-2)
                continue
            edges = adj.inn.get(target)
            if not edges:
                target = rng.randrange(adj.num_node)
                edges = adj.inn.get(target) or [(target, 0)]
            u, r = edges[rng.randrange(len(edges))]
            ids.append(r)
            target = u
        ids = tuple(reversed(ids))
        return (target if var == "e" else _ground(var, target, adj, rng), ids)
    if struct[-1] == ("u",):
        branches = struct[:-1]
        return tuple(_ground(b, target if i == 0 else rng.randrange(adj.num_node), adj, rng)
                     for i, b in enumerate(branches)) + ((-1,),)
    return tuple(_ground(b, target, adj, rng) for b in struct)


def sample_queries(data, num_per_type, train_fraction=0.9, query_types=None, seed=0, max_tries=50):
    """Seeded queries of every BetaE type over a KG with inverse edges (ultra_amd.synthetic.make_kg).  A `train_fraction` of
    the base triples (with their inverses) forms the training graph; easy answers are the answers on it, hard answers are
    the full graph's answers minus the easy ones.  Returns (training graph with its relation graph, QueryDataset)."""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    num_edge = data.edge_index.shape[1]
    half = num_edge // 2
    keep = torch.rand(half, generator=g) < train_fraction
    keep = torch.cat([keep, keep])
    train = Data(edge_index=data.edge_index[:, keep], edge_type=data.edge_type[keep], num_nodes=data.num_nodes,
                 num_relations=data.num_relations)
    tasks.build_relation_graph(train)
    full_adj = _Adjacency(data.edge_index, data.edge_type, data.num_nodes)
    train_adj = _Adjacency(train.edge_index, train.edge_type, data.num_nodes)
    heldout = (~keep[:half]).nonzero().flatten().tolist()
    id2type = sorted(query_types) if query_types else ID2TYPE
    queries, types, easy_answers, hard_answers = [], [], [], []
    for type_id, name in enumerate(id2type):
        struct = TYPE2STRUCT[name]
        for _ in range(num_per_type):
            for attempt in range(max_tries):
                # aim at the tail of a held-out triple, so that hard answers exist
                e = heldout[rng.randrange(len(heldout))] if heldout else rng.randrange(half)
                target = int(data.edge_index[1, e])
                q = _ground(struct, target, full_adj, rng)
                full = answer_set(q, full_adj)
                easy = answer_set(q, train_adj)
                hard = full - easy
                if hard and easy <= full:
                    break
            queries.append(q)
            types.append(type_id)
            easy_answers.append(easy & full)
            hard_answers.append(hard)
    return train, QueryDataset(queries, types, easy_answers, hard_answers, data.num_nodes, id2type)
