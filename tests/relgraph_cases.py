"""The graphs and the reference of the relation-graph shape tests (test_relgraph_shapes_cpu.py, test_relgraph_shapes_gpu.py).

`reference` is written from the definition of the relation graph -- an edge r1 -> r2 of type hh / tt / ht / th exists iff some
entity is a head (h) or tail (t) of an r1 edge and of an r2 edge respectively -- as four fp32 matrix products over dense bool
incidence matrices on the CPU, and derives from them every format csrc/relgraph.hip produces.  It runs no ultra_amd code.

`wide_case` graphs have few entities and many relations: what counts is the number of 32-bit words of a relation bit set
(W = ceil(R / 32)), which the kernels walk 64 words per pass.  `many_case` has few relations and many edges and entities: what
counts is the second trip of the grid-stride loops."""
import functools

import numpy as np
import torch

WIDE_NODES = 300
BOUNDARY_RELATIONS = (0, 31, 32, 33, 2046, 2047, 2048, 2049, 2079, 2080, 4095, 4096)
# the relation counts of the GPU file: one word and its edges, one pass (2048 relations = 64 words) and its edges, a partial
# last word in a second pass (2050), a second pass of 37 words (3210), a third pass (4100)
WIDE_RELATIONS = (1, 31, 32, 33, 2047, 2048, 2049, 2050, 2080, 3210, 4100)
MANY_RELATIONS, MANY_NODES, MANY_EDGES = 40, 40000, 1200000
MANY_EDGE_STRIDE = 4096 * 256       # the threads of the widest launch of the per-edge kernels
MANY_NODE_STRIDE = 8192 * 4         # the waves of the widest launch of the per-entity kernels
MANY_LATE_NODES = 39000             # the entities from here on are touched by the edges from MANY_EDGE_STRIDE on only


class Case(object):
    def __init__(self, name, edge_index, edge_type, num_nodes, num_relations):
        self.name, self.edge_index, self.edge_type = name, edge_index, edge_type
        self.num_nodes, self.num_relations = num_nodes, num_relations


class Reference(object):
    """adj (4, R, W) int32, counts (4 R) int64, hbits / tbits (num_nodes W) int32, edge_index (2, n) / edge_type (n) int64."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def dense(self):
        return byte_adjacency(self.edge_index, self.edge_type, self.num_relations)


def pack_bits(matrix):
    """(..., R) bool -> (..., ceil(R / 32)) int32: bit r & 31 of word r >> 5; the padding bits of the last word are zero."""
    matrix = np.ascontiguousarray(matrix.numpy().astype(bool))
    r = matrix.shape[-1]
    w = (r + 31) // 32
    padded = np.zeros(matrix.shape[:-1] + (32 * w,), dtype=bool)
    padded[..., :r] = matrix
    octets = np.packbits(padded, axis=-1, bitorder="little")            # bit k of byte b = column 8 b + k
    return torch.from_numpy(np.ascontiguousarray(octets).view("<u4").astype(np.int32))


def unpack_bits(words, r):
    """The inverse of pack_bits: (..., W) int32 -> (..., r) bool."""
    octets = np.ascontiguousarray(words.numpy().astype("<i4")).view(np.uint8)
    return torch.from_numpy(np.unpackbits(octets, axis=-1, bitorder="little")[..., :r].astype(bool))


def byte_adjacency(rel_edge_index, rel_edge_type, r):
    """The byte adjacency of the reference-order layer kernel: ceil(r / 16)^2 * 1024 bytes, byte
    (((rt njc + jc) 64) + i + 16 type) 16 + q = 1 for the edge (row = 16 rt + i, col = 16 jc + q, type)."""
    njc = (r + 15) // 16
    out = torch.zeros(njc * njc * 1024, dtype=torch.uint8)
    row, col = rel_edge_index
    rt, i, jc, q = row // 16, row % 16, col // 16, col % 16
    out[(((rt * njc + jc) * 64) + i + 16 * rel_edge_type) * 16 + q] = 1
    return out


def reference(edge_index, edge_type, num_nodes, R, keep=None):
    edge_index, edge_type = edge_index.cpu().to(torch.int64), edge_type.cpu().to(torch.int64)
    if keep is not None:
        on = keep.cpu() != 0
        edge_index, edge_type = edge_index[:, on], edge_type[on]
    H = torch.zeros(num_nodes, R, dtype=torch.bool)
    T = torch.zeros(num_nodes, R, dtype=torch.bool)
    H[edge_index[0], edge_type] = True
    T[edge_index[1], edge_type] = True
    h, t = H.float(), T.float()
    A = torch.stack([h.t() @ h, t.t() @ t, h.t() @ t, t.t() @ h]) > 0        # counts <= num_nodes < 2^24: exact in fp32
    edges = A.nonzero()                                                         # sorted by (type, row, col)
    return Reference(num_nodes=num_nodes, num_relations=R, adj=pack_bits(A), counts=A.sum(2).flatten(),
                     hbits=pack_bits(H).flatten(), tbits=pack_bits(T).flatten(),
                     edge_index=edges[:, 1:].t().contiguous(), edge_type=edges[:, 0].contiguous())


def case_reference(case, keep=None):
    return reference(case.edge_index, case.edge_type, case.num_nodes, case.num_relations, keep)


@functools.lru_cache(maxsize=None)
def wide_case(R, seed=0):
    """300 entities.  10 .. 279: head of 1 - 6 edges each, random relation, random tail among themselves.  0: head, with tail
    1, of every boundary relation below R.  2: head, with tail 3, of the relations 3, 10, 17, ... (at most 600): rows whose
    columns lie in every word of every pass.  4: a self loop on relation R - 1.  280 .. 299: no edge.  The first 50 edges are
    repeated at the end."""
    g = torch.Generator().manual_seed(1000003 * seed + R)
    degree = torch.randint(1, 7, (270,), generator=g)
    head = torch.repeat_interleave(torch.arange(10, 280), degree)
    tail = torch.randint(10, 280, (len(head),), generator=g)
    rel = torch.randint(0, R, (len(head),), generator=g)
    boundary = torch.tensor(sorted({r for r in BOUNDARY_RELATIONS + (R - 1,) if r < R}))
    spread = torch.arange(3, max(R, 3), 7)[:600]
    head = torch.cat([head, torch.zeros_like(boundary), torch.full_like(spread, 2), torch.tensor([4])])
    tail = torch.cat([tail, torch.ones_like(boundary), torch.full_like(spread, 3), torch.tensor([4])])
    rel = torch.cat([rel, boundary, spread, torch.tensor([R - 1])])
    edge_index = torch.stack([head, tail])
    return Case("wide_%d_%d" % (R, seed), torch.cat([edge_index, edge_index[:, :50]], dim=1), torch.cat([rel, rel[:50]]),
                WIDE_NODES, R)


def wide_split(case):
    """The position from which on a wide case lists the edges of entities 0, 2 and 4 (and the repeated first 50)."""
    first = int((case.edge_index[0] < 10).nonzero()[0])
    assert bool((case.edge_index[0, :first] >= 10).all())
    return first


@functools.lru_cache(maxsize=None)
def many_case(seed=0):
    """40 relations, 40,000 entities, 1,200,000 edges.  The first 4096 * 256 edges run among the entities below 39,000 over
    the relations below 38; the rest all touch an entity from 39,000 on, and those among them that run between two such
    entities are the only ones of relations 38 and 39."""
    g = torch.Generator().manual_seed(77 + seed)
    early, late = MANY_EDGE_STRIDE, MANY_EDGES - MANY_EDGE_STRIDE
    half = late // 2
    rand = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g)
    head = torch.cat([rand(0, MANY_LATE_NODES, early), rand(MANY_LATE_NODES, MANY_NODES, late)])
    tail = torch.cat([rand(0, MANY_LATE_NODES, early), rand(0, MANY_NODES, half), rand(MANY_LATE_NODES, MANY_NODES, late - half)])
    rel = torch.cat([rand(0, MANY_RELATIONS - 2, early + half), rand(0, MANY_RELATIONS, late - half)])
    return Case("many_%d" % seed, torch.stack([head, tail]), rel, MANY_NODES, MANY_RELATIONS)


@functools.lru_cache(maxsize=None)
def cached_reference(kind, *args):
    """reference() of wide_case(*args) / many_case(*args), computed once per process.  Nobody writes to its tensors."""
    return case_reference({"wide": wide_case, "many": many_case}[kind](*args))


@functools.lru_cache(maxsize=None)
def checked(kind, *args):
    """(case, reference) of wide_case(*args) / many_case(*args), its conditions asserted."""
    case, ref = {"wide": wide_case, "many": many_case}[kind](*args), cached_reference(kind, *args)
    assert conditions(case, ref)
    return case, ref


def conditions(case, ref=None):
    """What a case must hold for the tests built on it to mean anything, from the reference alone.  Raises AssertionError."""
    ref = case_reference(case) if ref is None else ref
    R = case.num_relations
    assert ref.edge_index.shape[1] == int(ref.counts.sum()) <= 1500000
    rows = unpack_bits(ref.adj, R)                      # (4, R, R)
    if R >= 31:
        assert all(int((ref.edge_type == k).sum()) > 0 for k in range(4)), "a type without an edge"
    if R >= 2048:
        assert bool((ref.counts == 0).any()), "no empty row"
    if R > 2048:
        both = rows[:, :, :2048].any(2) & rows[:, :, 2048:].any(2)
        assert bool(both.any()), "no row with columns on both sides of 2048"
        if R > 4096:
            assert bool((both & rows[:, :, 4096:].any(2)).any()), "no row with columns in all three passes"
    if case.name.startswith("many"):
        touched = (case.edge_index >= MANY_LATE_NODES).any(0)
        assert not bool(touched[:MANY_EDGE_STRIDE].any()) and bool(touched[MANY_EDGE_STRIDE:].all())
        # a pair of relations that only the entities of the second trip carry
        low = (case.edge_index < MANY_NODE_STRIDE).any(0)
        assert not bool(((case.edge_type >= MANY_RELATIONS - 2) & low).any())
        assert int(ref.counts.view(4, R)[:, MANY_RELATIONS - 2:].min()) > 0
    return True
