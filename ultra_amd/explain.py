"""Path explanations of link predictions: BaseNBFNet.visualize's beam search (reference: ultra/base_nbfnet.py:156-263).

visualize takes the gradient of one triple's score with respect to every layer's edge weights, beam-searches the
highest-weight paths from head to tail through those gradients and returns the top paths with their average edge weight.
Here every layer of the beam search is one call of ultra_beam_search_layer (csrc/beam_search.hip) over a
destination-major CSR of the graph that is built once per graph and cached, and the backtracking of topk_average_length
runs as device gathers with one copy to the host at the end.  The *_batch functions do the same for S triples at once:
the sample is a grid dimension of the beam kernels (ultra_beam_search_layer_batch), so S searches cost the launches of one.

Semantics: the reference's with stable sorts and exact top-k keys.  The reference itself is
order-dependent -- its ties follow whatever its unstable sorts produce, and its scatter_topk merges values closer than
about 4 (max - min) N 2^-23 -- so it is not a bit-exact target.
"""
from collections import OrderedDict, namedtuple

import ctypes

import torch

from . import _lib
from ._lib import check, lib, stream_of

BeamCSR = namedtuple("BeamCSR", "row_ptr src type eid hub_rows num_hub num_node num_edge")

_CSR_CACHE = OrderedDict()
_CSR_CACHE_SIZE = 8


def beam_csr(edge_index, edge_type, num_node):
    """The destination-major CSR of a graph for the beam search (cached like rspmm.get_plan): a stable sort by destination
    on the device, so the slots of every row keep ascending edge id; rows above ULTRA_BEAM_HUB_DEGREE listed apart."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
           edge_type.data_ptr(), edge_type._version, str(edge_index.device), int(num_node))
    hit = _CSR_CACHE.get(key)
    if hit is not None:
        _CSR_CACHE.move_to_end(key)
        return hit[0]
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.shape != (edge_index.shape[1],):
        raise ValueError("Expected `edge_index` of shape (2, num_edge) and `edge_type` of shape (num_edge,)")
    if not edge_index.is_cuda:
        raise RuntimeError("the beam search runs on the GPU: pass the graph on a CUDA device")
    num_edge = edge_index.shape[1]
    if num_node <= 0 or num_node >= 2 ** 31 or num_edge >= 2 ** 31:
        raise ValueError("the beam search takes 0 < num_node < 2^31 and num_edge < 2^31")
    if num_edge and (int(edge_index.min()) < 0 or int(edge_index.max()) >= num_node):
        raise ValueError("edge_index holds node ids outside [0, num_node)")
    src, dst = edge_index[0], edge_index[1]
    order = torch.sort(dst, stable=True).indices
    deg = torch.bincount(dst, minlength=num_node)
    row_ptr = torch.zeros(num_node + 1, dtype=torch.int64, device=dst.device)
    torch.cumsum(deg, 0, out=row_ptr[1:])
    hub_rows = torch.nonzero(deg > _lib.BEAM_HUB_DEGREE).flatten().to(torch.int64).contiguous()
    csr = BeamCSR(row_ptr, src[order].to(torch.int32).contiguous(), edge_type[order].to(torch.int32).contiguous(),
                  order.to(torch.int32).contiguous(), hub_rows, int(hub_rows.numel()), int(num_node), int(num_edge))
    _CSR_CACHE[key] = (csr, edge_index, edge_type)     # (the tensors stay alive with the entry: no recycled data_ptr aliases it)
    while len(_CSR_CACHE) > _CSR_CACHE_SIZE:
        _CSR_CACHE.popitem(last=False)
    return csr


def clear_csr_cache():
    _CSR_CACHE.clear()


def beam_search_layer(csr, edge_grad, dist_in, tail, num_beam):
    """One layer (ultra_beam_search_layer): (num_node, num_beam) fp32 distances and (num_node, num_beam, 4) int64 back
    edges [src, dst, type, prev_rank], on the current stream of the operands' device."""
    if not isinstance(num_beam, int) or not 1 <= num_beam <= _lib.BEAM_MAX:
        raise ValueError("num_beam must be an int in [1, %d], got %r" % (_lib.BEAM_MAX, num_beam))
    if edge_grad.dtype != torch.float32 or dist_in.dtype != torch.float32:
        raise TypeError("the beam search takes fp32 edge gradients and distances, got %s / %s" % (edge_grad.dtype, dist_in.dtype))
    if tuple(edge_grad.shape) != (csr.num_edge,):
        raise ValueError("Expected edge gradients of shape (%d,), got %s" % (csr.num_edge, tuple(edge_grad.shape)))
    if tuple(dist_in.shape) != (csr.num_node, num_beam):
        raise ValueError("Expected distances of shape (%d, %d), got %s" % (csr.num_node, num_beam, tuple(dist_in.shape)))
    if not (edge_grad.is_cuda and dist_in.is_cuda and edge_grad.device == csr.row_ptr.device == dist_in.device):
        raise RuntimeError("edge gradients, distances and graph must be on one CUDA device")
    tail = int(tail)
    if not 0 <= tail < csr.num_node:
        raise ValueError("tail %d outside [0, %d)" % (tail, csr.num_node))
    edge_grad, dist_in = edge_grad.contiguous(), dist_in.contiguous()
    dist = torch.empty((csr.num_node, num_beam), dtype=torch.float32, device=dist_in.device)
    back = torch.empty((csr.num_node, num_beam, 4), dtype=torch.int64, device=dist_in.device)
    stream = stream_of(dist_in)
    check(lib.ultra_beam_search_layer(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), csr.eid.data_ptr(),
                                      csr.hub_rows.data_ptr() if csr.num_hub else None, csr.num_hub, csr.num_node,
                                      csr.num_edge, edge_grad.data_ptr(), dist_in.data_ptr(), tail, num_beam,
                                      dist.data_ptr(), back.data_ptr(), stream))
    return dist, back


def beam_search_distance(data, edge_grads, h_index, t_index, num_beam=10):
    """base_nbfnet.py:173-232: per layer, the top `num_beam` distances of every node from h and their back edges."""
    h, t = _scalar_index(h_index, "h_index"), _scalar_index(t_index, "t_index")
    csr = beam_csr(data.edge_index, data.edge_type, data.num_nodes)
    dev = data.edge_index.device
    dist = torch.full((data.num_nodes, num_beam), float("-inf"), device=dev)
    dist[h, 0] = 0
    distances, back_edges = [], []
    with torch.no_grad():
        for edge_grad in edge_grads:
            dist, back = beam_search_layer(csr, edge_grad, dist, t, num_beam)
            # every message of the layer -inf: the whole layer is -inf and zeros (base_nbfnet.py:220).  A finite message
            # always leaves a finite distance behind, so "no finite distance" is that condition.
            back.mul_(torch.isfinite(dist).any())
            distances.append(dist)
            back_edges.append(back)
    return distances, back_edges


def topk_average_length(distances, back_edges, t_index, k=10):
    """base_nbfnet.py:234-263: backtrack the best `k` entries of t's row of every layer into paths [(h, t, r), ...] and
    weigh each with distance / length; the best `k` paths overall.  The backtracking is a chain of device gathers, copied
    to the host once."""
    t = _scalar_index(t_index, "t_index")
    records = []
    for i in range(len(distances)):
        distance, order = distances[i][t].flatten().sort(descending=True, stable=True)
        distance, order = distance[:k], order[:k]
        steps = [back_edges[i][t].index_select(0, order)]                 # (n, 4) edges into t
        for j in range(i - 1, -1, -1):
            prev = steps[-1]
            steps.append(back_edges[j][prev[:, 0], prev[:, 3]])
        records.append((distance, torch.stack(steps)))                    # (i + 1, n, 4), last edge first
    host = [(d.cpu().tolist(), s.cpu()) for d, s in records]
    paths, average_lengths = [], []
    for i, (dist, steps) in enumerate(host):
        for n, d in enumerate(dist):
            if d == float("-inf"):
                break
            path = [tuple(int(x) for x in steps[j, n, :3]) for j in range(i, -1, -1)]
            paths.append(path)
            average_lengths.append(d / len(path))
    if paths:
        average_lengths, paths = zip(*sorted(zip(average_lengths, paths), reverse=True)[:k])
    return paths, average_lengths


# ---- a batch of S independent searches over one graph: the sample is a grid dimension of the same two kernels ----
def _index_vector(index, name, num_sample=None):
    """(S,) int64 of `index` (a tensor of S entries, a sequence or one int) plus its smallest and largest entry as Python
    ints: read from the host copy where there is one, else with one device read."""
    if not torch.is_tensor(index):
        index = torch.as_tensor(index, dtype=torch.int64)
    index = index.reshape(-1).to(torch.int64)
    if num_sample is not None and index.numel() != num_sample:
        raise ValueError("%s: expected %d entries, got %d" % (name, num_sample, index.numel()))
    if index.numel() == 0:
        return index, 0, -1
    lo, hi = torch.aminmax(index)
    return index, int(lo), int(hi)


def _check_index_range(index, name, num_node, num_sample=None):
    index, lo, hi = _index_vector(index, name, num_sample)
    if lo < 0 or hi >= num_node:
        raise ValueError("%s holds node ids outside [0, %d)" % (name, num_node))
    return index


def beam_search_layer_batch(csr, edge_grad, dist_in, tails, num_beam, tails_checked=False, delta=None, added_grad=None):
    """One layer of S searches (ultra_beam_search_layer_batch): edge_grad (S, num_edge), dist_in (S, num_node, num_beam),
    tails (S) -> (S, num_node, num_beam) fp32 distances and (S, num_node, num_beam, 4) int64 back edges; sample s is
    beam_search_layer on slice s with tails[s], bit for bit.  Two launches whatever S is; `tails` is used on the device.
    tails_checked: the caller has already checked the tails against [0, num_node) (beam_search_distance_batch does it once
    for all layers: on device tensors the check is a read-back).
    delta (rspmm.GraphDelta of the CSR's graph) with added_grad (S, 2 capacity) fp32, column j the gradient of the edge at
    position j of delta.edges(): the layer on delta.materialize(), bit for bit, from the base graph's CSR -- after the two
    launches ultra_beam_search_edit_rows_batch recomputes the rows an added or a tombstoned edge points into (the base slots
    minus the dead keys, then the added edges in ascending j); edge_grad stays over the BASE edge list, the columns of
    tombstoned edges are never read.  One launch more, sized by the delta's capacity: nothing is read on the host."""
    if not isinstance(num_beam, int) or not 1 <= num_beam <= _lib.BEAM_MAX:
        raise ValueError("num_beam must be an int in [1, %d], got %r" % (_lib.BEAM_MAX, num_beam))
    if edge_grad.dtype != torch.float32 or dist_in.dtype != torch.float32:
        raise TypeError("the beam search takes fp32 edge gradients and distances, got %s / %s" % (edge_grad.dtype, dist_in.dtype))
    if edge_grad.dim() != 2 or edge_grad.shape[1] != csr.num_edge:
        raise ValueError("Expected edge gradients of shape (S, %d), got %s" % (csr.num_edge, tuple(edge_grad.shape)))
    num_sample = edge_grad.shape[0]
    if tuple(dist_in.shape) != (num_sample, csr.num_node, num_beam):
        raise ValueError("Expected distances of shape (%d, %d, %d), got %s"
                         % (num_sample, csr.num_node, num_beam, tuple(dist_in.shape)))
    if num_sample > 65535:
        raise ValueError("at most 65535 samples a call, got %d" % num_sample)
    if not (edge_grad.is_cuda and dist_in.is_cuda and edge_grad.device == csr.row_ptr.device == dist_in.device):
        raise RuntimeError("edge gradients, distances and graph must be on one CUDA device")
    if not tails_checked:
        tails = _check_index_range(tails, "tails", csr.num_node, num_sample)
    elif tuple(tails.shape) != (num_sample,) or tails.dtype != torch.int64:
        raise ValueError("Expected `tails` of shape (%d,) int64, got %s %s" % (num_sample, tuple(tails.shape), tails.dtype))
    if (delta is None) != (added_grad is None):
        raise ValueError("`delta` and `added_grad` go together")
    if delta is not None:
        if delta.num_nodes != csr.num_node or delta.base.edge_index.shape[1] != csr.num_edge:
            raise ValueError("the delta was made for a graph of %d nodes, the CSR has %d" % (delta.num_nodes, csr.num_node))
        if added_grad.dtype != torch.float32 or tuple(added_grad.shape) != (num_sample, 2 * delta.capacity):
            raise ValueError("Expected added gradients of shape (%d, %d) fp32, got %s %s"
                             % (num_sample, 2 * delta.capacity, tuple(added_grad.shape), added_grad.dtype))
        if added_grad.device != dist_in.device or delta.device != dist_in.device:
            raise RuntimeError("added gradients, delta and distances must be on one CUDA device")
        added_grad = added_grad.contiguous()
    tails = tails.to(dist_in.device).contiguous()
    edge_grad, dist_in = edge_grad.contiguous(), dist_in.contiguous()
    dist = torch.empty((num_sample, csr.num_node, num_beam), dtype=torch.float32, device=dist_in.device)
    back = torch.empty((num_sample, csr.num_node, num_beam, 4), dtype=torch.int64, device=dist_in.device)
    if num_sample == 0:
        return dist, back
    stream = stream_of(dist_in)
    check(lib.ultra_beam_search_layer_batch(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(), csr.eid.data_ptr(),
                                            csr.hub_rows.data_ptr() if csr.num_hub else None, csr.num_hub, csr.num_node,
                                            csr.num_edge, num_sample, edge_grad.data_ptr(), dist_in.data_ptr(),
                                            tails.data_ptr(), num_beam, dist.data_ptr(), back.data_ptr(), stream))
    if delta is not None:
        edits = delta.explain_operand()
        check(lib.ultra_beam_search_edit_rows_batch(csr.row_ptr.data_ptr(), csr.src.data_ptr(), csr.type.data_ptr(),
                                                    csr.eid.data_ptr(), csr.num_node, csr.num_edge, num_sample,
                                                    edge_grad.data_ptr(), ctypes.byref(edits), added_grad.data_ptr(),
                                                    added_grad.stride(0), dist_in.data_ptr(), tails.data_ptr(), num_beam,
                                                    dist.data_ptr(), back.data_ptr(), stream))
    return dist, back


def beam_search_distance_batch(data, edge_grads, h_index, t_index, num_beam=10, delta=None, added_grads=None):
    """beam_search_distance for S triples at once: edge_grads is a list of (S, num_edge) tensors, one per layer, h_index and
    t_index hold S node ids.  Returns per layer (S, num_node, num_beam) distances and (S, num_node, num_beam, 4) back
    edges; slice s is beam_search_distance of triple s, the all -inf rule applied per sample on the device.
    delta / added_grads (one (S, 2 capacity) tensor per layer): the search on delta.materialize(data) from data's own cached
    CSR (beam_search_layer_batch) -- no sort when the delta changes."""
    csr = beam_csr(data.edge_index, data.edge_type, data.num_nodes)
    dev = data.edge_index.device
    num_sample = edge_grads[0].shape[0] if len(edge_grads) else _index_vector(h_index, "h_index")[0].numel()
    h = _check_index_range(h_index, "h_index", csr.num_node, num_sample).to(dev)
    t = _check_index_range(t_index, "t_index", csr.num_node, num_sample).to(dev)
    if not isinstance(num_beam, int) or not 1 <= num_beam <= _lib.BEAM_MAX:
        raise ValueError("num_beam must be an int in [1, %d], got %r" % (_lib.BEAM_MAX, num_beam))
    dist = torch.full((num_sample, csr.num_node, num_beam), float("-inf"), device=dev)
    dist[torch.arange(num_sample, device=dev), h, 0] = 0
    distances, back_edges = [], []
    with torch.no_grad():
        if (delta is None) != (added_grads is None) or (delta is not None and len(added_grads) != len(edge_grads)):
            raise ValueError("`delta` goes with one `added_grads` tensor per layer")
        for i, edge_grad in enumerate(edge_grads):
            dist, back = beam_search_layer_batch(csr, edge_grad, dist, t, num_beam, tails_checked=True, delta=delta,
                                                 added_grad=None if delta is None else added_grads[i])
            # (beam_search_distance's all -inf rule, per sample and without leaving the device)
            back.mul_(torch.isfinite(dist).flatten(1).any(dim=1).view(-1, 1, 1, 1))
            distances.append(dist)
            back_edges.append(back)
    return distances, back_edges


def topk_average_length_batch(distances, back_edges, t_index, k=10):
    """topk_average_length for S samples: distances[i] (S, num_node, K), back_edges[i] (S, num_node, K, 4), t_index S node
    ids.  The backtracking is device gathers over all samples at once and ONE copy to the host per call; returns a list of
    (paths, average_lengths), entry s equal to topk_average_length on sample s's slices."""
    if not distances:
        return [([], []) for _ in range(_index_vector(t_index, "t_index")[0].numel())]
    num_sample, num_node = distances[0].shape[0], distances[0].shape[1]
    dev = distances[0].device
    t = _check_index_range(t_index, "t_index", num_node, num_sample).to(dev)
    if num_sample == 0:
        return []
    sample = torch.arange(num_sample, device=dev)
    flat_d, flat_s, shapes = [], [], []
    for i in range(len(distances)):
        distance, order = distances[i][sample, t].sort(dim=1, descending=True, stable=True)       # (S, K)
        distance, order = distance[:, :k], order[:, :k]
        n = order.shape[1]
        rows = sample.unsqueeze(1).expand(-1, n)
        steps = [back_edges[i][rows, t.unsqueeze(1).expand(-1, n), order]]      # (S, n, 4) edges into t
        for j in range(i - 1, -1, -1):
            prev = steps[-1]
            steps.append(back_edges[j][rows, prev[..., 0], prev[..., 3]])
        steps = torch.stack(steps, dim=1)                                      # (S, i + 1, n, 4), last edge first
        shapes.append((i + 1, n))
        flat_d.append(distance.to(torch.float64).reshape(num_sample, -1))
        flat_s.append(steps.reshape(num_sample, -1))
    # one copy: the distances ride as fp64 bit patterns beside the int64 steps (fp32 -> fp64 is exact)
    host = torch.cat([torch.cat(flat_d, dim=1).view(torch.int64), torch.cat(flat_s, dim=1)], dim=1).cpu()
    n_dist = sum(n for _, n in shapes)
    host_d = host[:, :n_dist].contiguous().view(torch.float64)
    host_s = host[:, n_dist:]
    results = []
    for s in range(num_sample):
        paths, average_lengths = [], []
        d_off = s_off = 0
        for i, (depth, n) in enumerate(shapes):
            dist = host_d[s, d_off:d_off + n].tolist()
            steps = host_s[s, s_off:s_off + depth * n * 4].view(depth, n, 4)
            d_off += n
            s_off += depth * n * 4
            for m, d in enumerate(dist):
                if d == float("-inf"):
                    break
                path = [tuple(int(x) for x in steps[j, m, :3]) for j in range(i, -1, -1)]
                paths.append(path)
                average_lengths.append(d / len(path))
        if paths:
            average_lengths, paths = zip(*sorted(zip(average_lengths, paths), reverse=True)[:k])
        results.append((paths, average_lengths))
    return results


def _scalar_index(index, name):
    if torch.is_tensor(index):
        if index.numel() != 1:
            raise ValueError("%s: one triple at a time (base_nbfnet.py:156), got %d indices" % (name, index.numel()))
        return int(index.reshape(()))
    return int(index)
