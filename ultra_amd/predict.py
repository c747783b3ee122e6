"""Serving link-prediction queries: the filtered top-k answers of (h, r, ?) and (?, r, t).

The evaluation protocol (eval.evaluate, tasks.filtered_ranking) returns the rank of a positive the caller already knows;
this module answers the question a user of a pre-trained model asks: which entities does the model predict for this head
and relation, leaving out the ones the graph already states?

  filtered_topk_reference   the semantics in plain torch, on any device -- the definition the kernel is tested against
  filtered_topk             csrc/topk_kernels.hip (ultra_filtered_topk): no (batch, N) mask, no clone of the scores
  filtered_rank             csrc/rank_kernels.hip (ultra_filtered_rank): the rank of a positive among a row's candidates
  filtered_above_reference  the answer SET of a row -- every candidate above a threshold, ranked -- in plain torch
  filtered_above            csrc/above_kernels.hip (ultra_filtered_above): the length of the lists is decided on the device
  logit_threshold           the logit threshold of a probability
  known_answers             the ragged lists of ids to leave out, from the filter graph (no positive is added)
  Predictor                 .tails(h, r) / .heads(t, r): candidate construction, the forward and the selection as one
                            hipGraph replay per batch; .tails_above(h, r, min_score) / .heads_above(t, r, min_score): the sets
  merge_pairs_reference     the best k (query, id, score) records of a running list and one more batch, in plain torch
  merge_pairs               csrc/pairs_kernels.hip (ultra_topk_pairs_merge): the running list updated in place on the device
  best_reference            the best k (query, answer) pairs over all queries of a call: one forward per query, one stable sort
  Predictor.best_tails / best_heads / propose_tails / propose_heads    ... the same as captured steps: link discovery
  verify_reference          leave-one-out verification of stated facts in plain torch: per triple a filtered copy of the graph
  Predictor.verify_tails    ... the same for a batch of facts as one hipGraph replay: per-sample keep masks over the cached plan
    / .verify_heads         of the full graph

Order: score descending, equal scores by ascending id, every NaN above every number (NaNs tie), -0.0 == +0.0
-- the stable descending torch.sort.  A filtered candidate is removed, not rescored: a genuine -inf score is a candidate
like any other, ranked last.  Slots beyond count = min(k, N - |known|) hold id -1 and score -inf.

A GROWING graph and RETIRED entities: Predictor(entity_capacity=M) reserves rows for entities
that arrive later and Predictor.remove_entities(ids) takes ids out of the candidate set for good -- `num_live` and `retired` of
every function here.  What the two operands are and which entry takes them: ultra_amd/selection.py.
"""

import contextlib
import functools
import inspect
import math

import torch

from . import _lib, dense, models, rspmm, selection, tasks
from .candidates import CandidateSets, span_rows
from .graph import Capture, param_state
from .live import LiveGraph, check_live, check_live_relations, check_not_retired, forwarded, with_facts

_select = selection.launch      # (the dispatcher, under the name and with the arguments it is called by here)


def _alive_columns(pred, retired, num_live, index=None):
    """The _reference functions with `retired` (a sorted int64 id vector): (pred with the columns at or beyond num_live and the
    retired columns deleted, the ids of the columns kept, `index` -- ids that are alive -- as positions among them)."""
    n = pred.shape[1] if num_live is None else selection.live_int(num_live, pred.shape[1])
    keep = torch.ones(n, dtype=torch.bool, device=pred.device)
    retired = torch.as_tensor(retired, dtype=torch.long, device=pred.device).flatten()
    keep[retired[retired < n]] = False
    cols = keep.nonzero().flatten()
    if index is not None:
        at = torch.searchsorted(cols, index)
        if len(index) and (bool((at >= len(cols)).any()) or not torch.equal(cols[at.clamp(max=max(len(cols) - 1, 0))], index)):
            raise ValueError("a known id or a positive is retired or not live: they must be alive")
        index = at
    return pred[:, cols], cols, index


def _among_keep(among, b, n, num_live, retired, dev):
    """The _reference functions with `among` (per row a vector or list of ids): the (n) bool row of the ELIGIBLE ids of row b's
    set -- listed, in [0, num_live or n), not retired.  By sets: order and repeats in the list do not matter."""
    live = n if num_live is None else selection.live_int(num_live, n)
    ids = torch.as_tensor(among[b], dtype=torch.long, device=dev).flatten()
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[ids[(ids >= 0) & (ids < live)]] = True
    if retired is not None:
        gone = torch.as_tensor(retired, dtype=torch.long, device=dev).flatten()
        keep[gone[(gone >= 0) & (gone < n)]] = False
    return keep


def _among_rows(among, batch):
    if len(among) != batch:
        raise ValueError("`among` of a _reference function is one id vector per row: got %d for %d rows" % (len(among), batch))
    return among


def filtered_rank_reference(pred, pos, ptr, index, num_live=None, retired=None, among=None):
    """(rank (batch) int64, num_negative (batch) int64) of pred[b, pos[b]] among the candidates of row b -- the ids not in
    index[ptr[b] : ptr[b + 1]] (the known answers, the positive among them), ties counting against the positive: what
    ultra_filtered_rank computes, in plain torch on any device (tasks.compute_ranking over the mask the lists stand for).
    num_live: only the ids below it exist.  retired (a sorted int64 id vector): those ids do not exist either -- this function on
    pred with their columns deleted, the positives and the known ids (all alive) renumbered.  among (one id vector per row):
    the candidates of row b are the eligible ids of among[b] (listed, below num_live, not retired) that are not known --
    rank = 1 + those that score at least pred[b, pos[b]], num_negative = how many there are; pos[b] need not be listed."""
    if among is not None:
        batch, n = pred.shape
        rank = torch.empty(batch, dtype=torch.long, device=pred.device)
        num_negative = torch.empty(batch, dtype=torch.long, device=pred.device)
        for b in range(batch):
            keep = _among_keep(_among_rows(among, batch), b, n, num_live, retired, pred.device)
            keep[index[int(ptr[b]):int(ptr[b + 1])]] = False
            rank[b] = 1 + int((keep & (pred[b, pos[b]] <= pred[b])).sum())
            num_negative[b] = int(keep.sum())
        return rank, num_negative
    if retired is not None:
        alive, cols, index = _alive_columns(pred, retired, num_live, index)
        return filtered_rank_reference(alive, _alive_columns(pred, retired, num_live, pos)[2], ptr, index)
    if num_live is not None:
        pred = pred[:, :selection.live_int(num_live, pred.shape[1])]
    mask = torch.ones(pred.shape, dtype=torch.bool, device=pred.device)
    for b in range(pred.shape[0]):
        mask[b, index[int(ptr[b]):int(ptr[b + 1])]] = False
    return tasks.compute_ranking(pred, pos, mask), mask.sum(dim=-1)


def filtered_topk_reference(pred, k, ptr=None, index=None, num_live=None, retired=None, among=None):
    """(ids (batch, k) int64, scores (batch, k) pred's dtype, count (batch) int64) -- per row, the candidates are the ids not
    in index[ptr[b] : ptr[b + 1]], in the order of the stable descending sort of their scores.  num_live: only the ids below it
    exist -- this function on pred[:, :num_live].  retired (a sorted int64 id vector): those ids do not exist either -- this
    function on pred with their columns deleted (the known ids are alive), the ids mapped back.  among (one id vector per row):
    the candidates of row b are the eligible ids of among[b] (listed, below num_live, not retired) that are not known, and
    count[b] = min(k, how many there are)."""
    if among is None and retired is not None:
        alive, cols, index = _alive_columns(pred, retired, num_live, index)
        ids, scores, count = filtered_topk_reference(alive, k, ptr, index)
        return torch.where(ids >= 0, cols[ids.clamp(min=0)] if len(cols) else ids, ids), scores, count
    if among is None and num_live is not None:
        return filtered_topk_reference(pred[:, :selection.live_int(num_live, pred.shape[1])], k, ptr, index)
    k = int(k)
    batch, n = pred.shape
    ids = torch.full((batch, k), -1, dtype=torch.long, device=pred.device)
    scores = torch.full((batch, k), float("-inf"), dtype=pred.dtype, device=pred.device)
    count = torch.zeros(batch, dtype=torch.long, device=pred.device)
    for b in range(batch):
        if among is None:
            keep = torch.ones(n, dtype=torch.bool, device=pred.device)
        else:
            keep = _among_keep(_among_rows(among, batch), b, n, num_live, retired, pred.device)
        if ptr is not None:
            keep[index[int(ptr[b]):int(ptr[b + 1])]] = False
        cand = keep.nonzero().flatten()
        order = torch.sort(pred[b, cand], descending=True, stable=True).indices[:k]
        m = order.numel()
        ids[b, :m] = cand[order]
        scores[b, :m] = pred[b, cand[order]]
        count[b] = m
    return ids, scores, count


def check_k(k):
    if not isinstance(k, int) or not 1 <= k <= _lib.TOPK_MAX:
        raise ValueError("k must be an int in [1, %d], got %r" % (_lib.TOPK_MAX, k))


def _gpu_scores(name, pred):
    """`pred` of the wrapper `name` as contiguous (batch, N) fp32 scores on the GPU (RuntimeError off it, else TypeError)."""
    if not pred.is_cuda:
        raise RuntimeError("ultra_amd.predict.%s: expected a GPU tensor; the MI355X engine has no CPU path" % name)
    if pred.dim() != 2 or pred.dtype != torch.float32:
        raise TypeError("%s takes (batch, N) fp32 scores, got %s %s" % (name, tuple(pred.shape), pred.dtype))
    return pred.contiguous()


def _known_lists(name, ptr, index, batch, dev):
    """The lists (ptr, index) of the wrapper `name`, contiguous: the caller holds them until the launch is enqueued."""
    if ptr.shape != (batch + 1,) or ptr.dtype != torch.long or index.dtype != torch.long or ptr.device != dev or index.device != dev:
        raise ValueError("%s takes int64 `ptr` of shape (batch + 1,) and int64 `index` on the scores' device" % name)
    return ptr.contiguous(), index.contiguous()


def filtered_topk(pred, k, ptr=None, index=None, num_live=None, retired=None, among=None, among_capacity=None):
    """filtered_topk_reference through the HIP kernel: pred (batch, N) fp32 on the GPU; ptr (batch + 1) / index int64, ids
    ascending and distinct within a row; ptr None: no filter.  num_live (an int in [1, N], or one int64 on the device, read by
    the kernels): ultra_filtered_topk_live on the full rows -- no slice, no copy; None: ultra_filtered_topk.  retired (the device
    pair (bits, count): live.retired_words over at least N slots and one int64, both read by the kernels):
    ultra_filtered_topk_alive, with num_live or without.  among (the device pair (span (batch, 2), index): row b's candidates
    are index[span[b, 0] : span[b, 1]], ascending and distinct; selection.among_operand): ultra_filtered_topk_among, with
    num_live and retired or without -- work and workspace O(among_capacity), which defaults to the longest span (one host
    read; a captured caller passes it)."""
    check_k(k)
    pred = _gpu_scores("filtered_topk", pred)
    batch, n = pred.shape
    dev = pred.device
    ids = torch.empty(batch, k, dtype=torch.long, device=dev)
    scores = torch.empty(batch, k, dtype=torch.float32, device=dev)
    count = torch.empty(batch, dtype=torch.long, device=dev)
    if batch == 0:
        return ids, scores, count
    if ptr is not None:
        ptr, index = _known_lists("filtered_topk", ptr, index, batch, dev)
    among = selection.among_operand(among, batch, n, dev, among_capacity)
    if among is None:
        ws_bytes = _lib.lib.ultra_filtered_topk_workspace(batch, n, k)
    else:
        ws_bytes = _lib.lib.ultra_filtered_topk_among_workspace(batch, among[2], k)
    ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.long, device=dev)
    args = (pred.data_ptr(), None if ptr is None else ptr.data_ptr(), None if ptr is None else index.data_ptr(), batch, n, k,
            ids.data_ptr(), scores.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    live = selection.live_operand(num_live, n, dev)     # (referenced until the launch is enqueued)
    _select("ultra_filtered_topk", args, live, dev, selection.retired_operand(retired, n, dev), among=among)
    return ids, scores, count


def filtered_rank(pred, pos, ptr, index, num_live=None, retired=None, out=None, among=None, among_capacity=None):
    """filtered_rank_reference through the HIP kernel (csrc/rank_kernels.hip): pred (batch, N) fp32 on the GPU; pos (batch), ptr
    (batch + 1) and index int64 on its device, the ids of a row ascending and distinct, the positive among them.  num_live,
    retired: as in filtered_topk -- ultra_filtered_rank_live / ultra_filtered_rank_alive; neither: ultra_filtered_rank.
    out: the pair (rank, num_negative) of (batch) int64 tensors to write into -- a captured step's own buffers -- and to
    return; None: new ones.  among, among_capacity: as in filtered_topk -- ultra_filtered_rank_among, the rank of the positive
    among the eligible listed ids that are not known; pos[b] need not be listed."""
    pred = _gpu_scores("filtered_rank", pred)
    batch, n = pred.shape
    dev = pred.device
    ptr, index = _known_lists("filtered_rank", ptr, index, batch, dev)
    if pos.shape != (batch,) or pos.dtype != torch.long or pos.device != dev:
        raise ValueError("filtered_rank takes int64 `pos` of shape (batch,) on the scores' device")
    if out is None:
        out = torch.empty(batch, dtype=torch.long, device=dev), torch.empty(batch, dtype=torch.long, device=dev)
    rank, num_negative = out
    if any(t.shape != (batch,) or t.dtype != torch.long or t.device != dev or not t.is_contiguous() for t in out):
        raise ValueError("`out` is the pair (rank, num_negative): contiguous int64 tensors of shape (batch,) on the scores' device")
    if batch == 0:
        return rank, num_negative
    pos = pos.contiguous()      # (referenced until the launch is enqueued)
    args = (pred.data_ptr(), pos.data_ptr(), ptr.data_ptr(), index.data_ptr(), batch, n, rank.data_ptr(), num_negative.data_ptr())
    live = selection.live_operand(num_live, n, dev)     # (referenced until the launch is enqueued)
    _select("ultra_filtered_rank", args, live, dev, selection.retired_operand(retired, n, dev),
            among=selection.among_operand(among, batch, n, dev, among_capacity), among_at=4)
    return rank, num_negative


def _fp32_threshold(threshold):
    """`threshold` rounded to fp32 (a Python float); ValueError unless it is finite or -inf."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise TypeError("the threshold is a Python float, got %r" % (threshold,))
    value = float(torch.tensor(float(threshold), dtype=torch.float64).to(torch.float32))
    if math.isnan(value) or value == float("inf"):
        raise ValueError("the threshold must be finite or -inf (after rounding to fp32), got %r" % (threshold,))
    return value


def logit_threshold(probability):
    """The logit at which sigmoid crosses `probability`: log(p / (1 - p)) in fp64, rounded to fp32; 0 < p < 1 (ValueError
    otherwise); p = 0.5 gives exactly 0.0.  The threshold `filtered_above` takes for "predicted with probability above p"."""
    p = float(probability)
    if not 0.0 < p < 1.0:
        raise ValueError("probability must lie strictly between 0 and 1, got %r" % (probability,))
    return float(torch.tensor(math.log(p / (1.0 - p)), dtype=torch.float64).to(torch.float32))


def filtered_above_reference(pred, threshold, ptr=None, index=None, num_live=None, retired=None, among=None):
    """The answer SET of every row, ranked: (out_ptr (batch + 1) int64, ids (total) int64, scores (total) pred's dtype, size
    (batch) int64), on any device -- the definition ultra_filtered_above is tested against.

    v is a member of row b iff pred[b, v] > threshold as an fp32 comparison: strict, a NaN is never a member, +inf is a member
    of any threshold, and with threshold -inf everything but -inf and NaN is.  threshold: a Python float, rounded to fp32,
    finite or -inf (ValueError otherwise).  size[b] counts the members among all ids, BEFORE the filter: the integer predicted
    cardinality, comparable with num_easy + num_hard.  ids[out_ptr[b] : out_ptr[b + 1]]: the members not in
    index[ptr[b] : ptr[b + 1]] (the lists of filtered_topk; ptr None: no filter) in the stable descending order -- score
    descending, equal scores by ascending id, -0.0 == +0.0; scores: their stored bits (a filtered member is removed, never
    rescored).

    Two differences from the reference's rule (script/run_query.py:42-44, `prob > 0.5`).  The rule here is on the LOGIT, logit
    > logit_threshold(p): for p = 0.5 the reference's fp32 sigmoid(x) > 0.5 is false for positive logits so small that the
    sigmoid rounds to 0.5 (roughly below 1e-7); such logits are members here.  And `size` is an integer count, not the
    reference's soft num_pred; query_eval keeps the reference's metrics as they are.

    num_live: only the ids below it exist -- this function on pred[:, :num_live].  retired (a sorted int64 id vector): those ids
    do not exist either, in the lists and in `size` -- this function on pred with their columns deleted, the ids mapped back.
    among (one id vector per row): only the eligible ids of among[b] (listed, below num_live, not retired) can be members of
    row b, in the lists and in `size`."""
    if among is None and retired is not None:
        alive, cols, index = _alive_columns(pred, retired, num_live, index)
        out_ptr, ids, scores, size = filtered_above_reference(alive, threshold, ptr, index)
        return out_ptr, cols[ids], scores, size
    if among is None and num_live is not None:
        return filtered_above_reference(pred[:, :selection.live_int(num_live, pred.shape[1])], threshold, ptr, index)
    thr = _fp32_threshold(threshold)
    batch, n = pred.shape
    dev = pred.device
    member = pred.float() > torch.tensor(thr, dtype=torch.float32, device=dev)
    if among is not None:
        member &= torch.stack([_among_keep(_among_rows(among, batch), b, n, num_live, retired, dev) for b in range(batch)]) \
            if batch else member
    size = member.sum(dim=-1)
    out_ptr = torch.zeros(batch + 1, dtype=torch.long, device=dev)
    ids, scores = [], []
    for b in range(batch):
        keep = member[b].clone()
        if ptr is not None:
            keep[index[int(ptr[b]):int(ptr[b + 1])]] = False
        cand = keep.nonzero().flatten()
        order = torch.sort(pred[b, cand], descending=True, stable=True).indices
        ids.append(cand[order])
        scores.append(pred[b, cand[order]])
        out_ptr[b + 1] = out_ptr[b] + cand.numel()
    ids = torch.cat(ids) if ids else torch.zeros(0, dtype=torch.long, device=dev)
    scores = torch.cat(scores) if scores else torch.zeros(0, dtype=pred.dtype, device=dev)
    return out_ptr, ids, scores, size


def filtered_above(pred, threshold, ptr=None, index=None, num_live=None, retired=None, among=None, among_capacity=None):
    """filtered_above_reference through the HIP kernels (csrc/above_kernels.hip): pred (batch, N) fp32 on the GPU; ptr
    (batch + 1) / index int64, ids ascending and distinct within a row; ptr None: no filter.  `ids` and `scores` come back as
    the full-capacity (batch * N) buffers: entries at or beyond out_ptr[batch] are unspecified.  No host wait is made -- the
    caller reads out_ptr[-1] when it wants to slice.  num_live (an int in [1, N], or one int64 on the device, read by the
    kernels): ultra_filtered_above_live on the full rows; None: ultra_filtered_above.  retired (the device pair (bits, count) of
    filtered_topk): ultra_filtered_above_alive.  among, among_capacity: as in filtered_topk -- ultra_filtered_above_among; the
    buffers that come back then hold batch * among_capacity entries."""
    thr = _fp32_threshold(threshold)
    pred = _gpu_scores("filtered_above", pred)
    batch, n = pred.shape
    dev = pred.device
    among = selection.among_operand(among, batch, n, dev, among_capacity) if batch else None
    out_ptr = torch.zeros(batch + 1, dtype=torch.long, device=dev)
    ids = torch.empty(batch * (n if among is None else among[2]), dtype=torch.long, device=dev)
    scores = torch.empty(ids.numel(), dtype=torch.float32, device=dev)
    size = torch.empty(batch, dtype=torch.long, device=dev)
    if batch == 0:
        return out_ptr, ids, scores, size
    if n == 0 or batch > _lib.ABOVE_MAX_BATCH:
        raise ValueError("filtered_above takes 1 to %d rows of at least one candidate, got %s" % (_lib.ABOVE_MAX_BATCH, tuple(pred.shape)))
    if ptr is not None:
        ptr, index = _known_lists("filtered_above", ptr, index, batch, dev)
    if among is None:
        ws_bytes = _lib.lib.ultra_filtered_above_workspace(batch, n)
    else:
        ws_bytes = _lib.lib.ultra_filtered_above_among_workspace(batch, among[2])
    ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.long, device=dev)
    args = (pred.data_ptr(), None if ptr is None else ptr.data_ptr(), None if ptr is None else index.data_ptr(), batch, n, thr,
            out_ptr.data_ptr(), ids.data_ptr(), scores.data_ptr(), ids.numel(), size.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    live = selection.live_operand(num_live, n, dev)     # (referenced until the launch is enqueued)
    _select("ultra_filtered_above", args, live, dev, selection.retired_operand(retired, n, dev), among=among)
    return out_ptr, ids, scores, size


# ---- the best k (query, id) pairs over many queries ----
def empty_pairs(k, device=None):
    """An empty running list of k slots -- (query (k) int64, id (k) int64, score (k) fp32, count (1) int64), every slot
    -1 / -1 / -inf -- for merge_pairs_reference / merge_pairs to fold batches into."""
    check_k(k)
    return (torch.full((k,), -1, dtype=torch.long, device=device), torch.full((k,), -1, dtype=torch.long, device=device),
            torch.full((k,), float("-inf"), dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.long, device=device))


def _pairs_operands(name, best, ids, scores):
    """The running list and the batch of `name` (merge_pairs / merge_pairs_reference), checked: (k, batch, k_row)."""
    if len(best) != 4:
        raise ValueError("%s: the running list is (query (k), id (k), score (k), count (1))" % name)
    query, best_id, best_score, count = best
    k = int(query.numel())
    check_k(k)
    if (query.shape != (k,) or best_id.shape != (k,) or best_score.shape != (k,) or count.numel() != 1
            or query.dtype != torch.long or best_id.dtype != torch.long or count.dtype != torch.long):
        raise ValueError("%s: the running list is (query (k), id (k), score (k), count (1)), the scores apart int64" % name)
    if ids.dim() != 2 or ids.shape != scores.shape or ids.dtype != torch.long or scores.dtype != best_score.dtype:
        raise TypeError("%s takes (batch, k_row) int64 ids and scores of the running list's dtype, got %s %s and %s %s"
                        % (name, tuple(ids.shape), ids.dtype, tuple(scores.shape), scores.dtype))
    batch, k_row = ids.shape
    if not 1 <= k_row <= _lib.TOPK_MAX or batch > _lib.PAIRS_MAX_BATCH:
        raise ValueError("%s takes at most %d rows of 1 to %d slots, got %s" % (name, _lib.PAIRS_MAX_BATCH, _lib.TOPK_MAX,
                                                                               tuple(ids.shape)))
    return k, batch, k_row


def merge_pairs_reference(best, ids, scores, query_base, n_rows=None, min_score=None):
    """The best k (query, id, score) records of a running list and one more batch of row-wise answers, in plain torch on any
    device -- the DEFINITION ultra_topk_pairs_merge is tested against.

    best: the running list (query (k), id (k), score (k), count (1)) -- empty_pairs(k) at first --, its first `count` records
    present.  ids, scores (batch, k_row): what a filtered_topk* call returned; row b is query query_base + b of the call; a
    slot with id < 0 is absent, a slot with id >= 0 and score -inf is a genuine candidate.  n_rows (None: batch): only the
    rows below it (clamped to [0, batch]) exist -- whatever the others hold.  min_score (None, or a Python float, finite or
    -inf): a record is a MEMBER iff score > min_score in fp32 -- strict, a NaN never is (filtered_above_reference's rule);
    None: every present record is a member, NaNs included.  The rule covers the running list's records too.

    [running list ; row 0 ; row 1 ; ...] is concatenated, absent slots and non-members are dropped, and the first k of ONE
    stable descending sort by score stay: score descending, NaN on top, -0.0 == +0.0, equal scores in the order they were laid
    out -- which is (query, id) ascending where every query of the batch is larger than every query of the running list (the
    caller's contract).  Returns a NEW running list, the slots beyond its count -1 / -1 / -inf; query_base, n_rows: ints or
    one-element tensors."""
    k, batch, k_row = _pairs_operands("merge_pairs_reference", best, ids, scores)
    best_query, best_id, best_score, count = best
    dev = ids.device
    old = min(max(int(count), 0), k)
    rows = batch if n_rows is None else min(max(int(n_rows), 0), batch)
    query = torch.cat([best_query[:old], (int(query_base) + torch.arange(rows, device=dev)).repeat_interleave(k_row)])
    answer = torch.cat([best_id[:old], ids[:rows].reshape(-1)])
    score = torch.cat([best_score[:old], scores[:rows].reshape(-1)])
    member = torch.cat([torch.ones(old, dtype=torch.bool, device=dev), ids[:rows].reshape(-1) >= 0])
    if min_score is not None:
        member &= score.float() > torch.tensor(_fp32_threshold(min_score), dtype=torch.float32, device=dev)
    query, answer, score = query[member], answer[member], score[member]
    order = torch.sort(score, descending=True, stable=True).indices[:k]
    m = order.numel()
    out = empty_pairs(k, dev)
    out = (out[0], out[1], out[2].to(best_score.dtype), out[3])
    out[0][:m], out[1][:m], out[2][:m] = query[order], answer[order], score[order]
    out[3].fill_(m)
    return out


def _device_scalar(name, what, value, dtype, dev):
    """`value` of merge_pairs' operand `what` as one `dtype` element on `dev`: a tensor is taken as it is (the kernel reads it
    when it runs), a Python number is copied there."""
    if torch.is_tensor(value):
        if value.numel() != 1 or value.dtype != dtype or value.device != dev:
            raise ValueError("%s: `%s` is a Python number or one %s on the scores' device" % (name, what, dtype))
        return value
    return torch.tensor([value], dtype=dtype, device=dev)


def merge_pairs(best, ids, scores, query_base, n_rows=None, min_score=None):
    """merge_pairs_reference through the HIP kernel (csrc/pairs_kernels.hip, ultra_topk_pairs_merge): everything fp32 / int64
    and contiguous on one GPU.  The running list `best` is updated IN PLACE and returned.  query_base, n_rows (int64) and
    min_score (fp32) may be one-element device tensors, which the kernel reads when it runs -- a recorded call serves new
    values --, or Python numbers (min_score then finite or -inf)."""
    name = "merge_pairs"
    if not scores.is_cuda:
        raise RuntimeError("ultra_amd.predict.%s: expected a GPU tensor; the MI355X engine has no CPU path" % name)
    k, batch, k_row = _pairs_operands(name, best, ids, scores)
    dev = scores.device
    if scores.dtype != torch.float32 or any(t.device != dev or not t.is_contiguous() for t in tuple(best) + (ids, scores)):
        raise TypeError("%s takes fp32 scores, everything contiguous on the scores' device" % name)
    if batch == 0:
        return best
    base = _device_scalar(name, "query_base", query_base, torch.long, dev)       # (referenced until the launch is enqueued)
    rows = None if n_rows is None else _device_scalar(name, "n_rows", n_rows, torch.long, dev)
    if min_score is not None and not torch.is_tensor(min_score):
        min_score = _fp32_threshold(min_score)
    low = None if min_score is None else _device_scalar(name, "min_score", min_score, torch.float32, dev)
    _lib.check(_lib.lib.ultra_topk_pairs_merge(ids.data_ptr(), scores.data_ptr(), batch, k_row, base.data_ptr(), _lib.ptr(rows),
                                               _lib.ptr(low), best[0].data_ptr(), best[1].data_ptr(), best[2].data_ptr(),
                                               best[3].data_ptr(), k, _lib.stream_of(scores)))
    return best


def known_answers(data, anchor, relation, mode="tail", extra=None):
    """(ptr (n + 1), index): per query the distinct tails of (anchor, relation, .) in `data` (mode="tail") or the distinct
    heads of (., relation, anchor) (mode="head"), ascending.  tasks.known_answers without the positive: for a true triple of
    `data` the two agree.  extra (None, or (sample, ids) int64 vectors): ids[j] is one more known answer of query
    sample[j] alone -- the answers a query's own assumed facts state."""
    if mode not in ("tail", "head"):
        raise ValueError("mode must be 'tail' or 'head', got %r" % (mode,))
    keyed, answer_row = (0, 1) if mode == "tail" else (1, 0)
    idx = tasks._key_index(mode, (data.edge_index, data.edge_type),
                           lambda: tasks.EdgeKeyIndex(torch.stack([data.edge_index[keyed], data.edge_type])))
    edge_id, count = tasks.edge_match(None, torch.stack([anchor, relation]), index=idx)
    truth = data.edge_index[answer_row, edge_id]
    sample = torch.arange(len(count), device=anchor.device).repeat_interleave(count)
    n = data.num_nodes
    key = sample * n + truth
    if extra is not None:
        key = torch.cat([key, extra[0].to(key.device) * n + extra[1].to(key.device)])
    key = torch.unique(key)                                    # sorted: grouped by query, ids ascending
    ptr = torch.searchsorted(key, torch.arange(len(anchor) + 1, device=anchor.device) * n)
    return ptr, key % n


def _candidates(data, anchor, relation, mode):
    """The t_batch (mode="tail") or h_batch (mode="head") form of tasks.all_negative for queries without a positive: every
    entity as the tail of (anchor, relation) or as the head of (relation, anchor).  The model turns the head form into a
    tail query with the inverse relation, exactly as in evaluation.  On a graph with reserved rows (Predictor(entity_capacity))
    data.num_nodes counts slots: the batch runs over all of them, and the selection afterwards knows how many are live."""
    n = data.num_nodes
    every = torch.arange(n, device=anchor.device).unsqueeze(0).expand(len(anchor), -1)
    fixed = anchor.unsqueeze(-1).expand(-1, n)
    r = relation.unsqueeze(-1).expand(-1, n)
    return torch.stack([fixed, every, r] if mode == "tail" else [every, fixed, r], dim=-1)


class _IndexedStep(Capture):
    """A captured step that reads the known lists of a whole call from a buffer of its own, `index` (loaded once per call), and
    the offsets of a batch's lists from `ptr`.  It holds what the Predictor compares to know whether the capture still serves:
    `params`, `capacity` (of `index`; 0 for index_capacity None -- no filter, nothing to load), `delta` and its `route`, and
    `retired`; `n_live` is the device live count the selection reads at replay."""

    def __init__(self, model, data, batch_size, index_capacity, delta, n_live, retired, among=None):
        """among (None, or (index capacity, list capacity): a step that selects among candidate lists): two
        more buffers -- `among_span` (bs, 2), copied per batch like `ptr`, and `among_index`, loaded once per call like
        `index` -- and the fixed `among_capacity` its selection is recorded with; `among_operand` is the triple it passes."""
        dev = data.edge_index.device
        Capture.__init__(self, dev)
        self.among_operand = None
        if among is not None:
            self.among_capacity = max(1, int(among[1]))
            self.among_span = torch.zeros(batch_size, 2, dtype=torch.long, device=dev)
            self.among_index = torch.zeros(max(1, int(among[0])), dtype=torch.long, device=dev)
            self.among_operand = (self.among_span, self.among_index, self.among_capacity)
        self.model, self.bs = model, batch_size
        self.delta, self.route, self.n_live, self.retired = delta, _delta_route(delta), n_live, retired
        self.filtered = index_capacity is not None
        self.capacity = max(1, int(index_capacity)) if self.filtered else 0
        self.ptr = torch.zeros(batch_size + 1, dtype=torch.long, device=dev)
        self.index = torch.zeros(max(1, self.capacity), dtype=torch.long, device=dev)

    def record_step(self, step, warmup, inputs, outputs):
        """Warm up and capture `step`, which reads the buffers `inputs` (and `ptr`, `index`) and writes the buffers `outputs`."""
        self.inputs, self.outputs = inputs, outputs
        self.warm_up(step, warmup)
        self.capture(step)
        self.params = param_state(self.model)

    def __call__(self, *rows_and_ptr):
        """The `outputs` of this batch -- the step's own buffers: copy before the next call -- from one row tensor per input and
        the batch's (bs + 1) offsets into the known lists (None where nothing is filtered)."""
        for buffer, rows in zip(self.inputs, rows_and_ptr):
            buffer.copy_(rows, non_blocking=True)
        if self.filtered:
            self.ptr.copy_(rows_and_ptr[-1], non_blocking=True)
        self.graph.replay()
        return self.outputs

    def load_index(self, index):
        self.index[:index.numel()].copy_(index, non_blocking=True)

    def load_among(self, index):
        self.among_index[:index.numel()].copy_(index, non_blocking=True)

    def among_fits(self, total, longest):
        """Do a call's candidate lists -- `total` ids, the longest `longest` -- fit this step's buffer and capacity?"""
        return self.among_operand is not None and total <= self.among_index.numel() and longest <= self.among_capacity


class _GraphedPredictStep(_IndexedStep):
    """One batch of one direction as ONE hipGraph replay (a graph.Capture, like graph.GraphedEvalStep): candidate construction, the
    forward and ultra_filtered_topk.  Per batch the host copies the (bs) anchors and relations and the (bs + 1) offsets into
    the known lists of the whole call, which live in a buffer of the step (`load_index`, once per call)."""

    def __init__(self, model, data, batch_size, k, mode, index_capacity, warmup=2, delta=None, n_live=None, retired=None,
                 among=None):
        """among (None, or _IndexedStep's (index capacity, list capacity)): the selection is ultra_filtered_topk_among over the
        step's own span and list buffers, n_live and retired its nullable operands; None: exactly the step of before.
        n_live (one int64 on the device, or None): the live count of a graph with reserved rows -- the selection is then
        ultra_filtered_topk_live, which reads it at replay; None: ultra_filtered_topk, exactly as before.
        retired (the device pair (bitmap, count) of a graph that retired entities, or None): the selection is
        ultra_filtered_topk_alive, which reads both at replay -- `retired` is what the Predictor compares.
        delta (rspmm.GraphDelta or None): handed to the model from the first capture.  While it is empty the model takes its
        normal path; once it holds facts or tombstones the capture records the delta's launches, which read its device buffers
        at replay --
        `route` is what the Predictor compares to know whether this capture still serves the delta."""
        _IndexedStep.__init__(self, model, data, batch_size, index_capacity, delta, n_live, retired, among)
        dev = data.edge_index.device
        self.k, self.mode = k, mode
        handed = self._model_delta(data, delta, batch_size)
        model_kwargs = {} if handed is None else {"delta": handed}
        self.anchor = torch.zeros(batch_size, dtype=torch.long, device=dev)
        self.relation = torch.zeros(batch_size, dtype=torch.long, device=dev)
        self.ids = torch.empty(batch_size, k, dtype=torch.long, device=dev)
        self.scores = torch.empty(batch_size, k, dtype=torch.float32, device=dev)
        self.count = torch.empty(batch_size, dtype=torch.long, device=dev)
        n = int(data.num_nodes)
        if among is None:
            ws_bytes = _lib.lib.ultra_filtered_topk_workspace(batch_size, n, k)
        else:
            ws_bytes = _lib.lib.ultra_filtered_topk_among_workspace(batch_size, self.among_capacity, k)
        self.ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.long, device=dev)

        def step():
            pred = model(data, _candidates(data, self.anchor, self.relation, mode), **model_kwargs).float().contiguous()
            args = (pred.data_ptr(), self.ptr.data_ptr() if self.filtered else None,
                    self.index.data_ptr() if self.filtered else None, batch_size, n, k, self.ids.data_ptr(),
                    self.scores.data_ptr(), self.count.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 8)
            _select("ultra_filtered_topk", args, n_live, dev, retired, among=self.among_operand)
            self._after_selection()

        self.record_step(step, warmup, (self.anchor, self.relation), (self.ids, self.scores, self.count))


    def _model_delta(self, data, delta, batch_size):
        """What the model is handed as `delta=` (None: nothing): the delta itself; _GraphedAssumeStep hands an overlay over it."""
        return delta

    def _after_selection(self):
        """What the step records behind its selection: nothing; _GraphedBestStep folds the batch into its running list."""


def _release(steps):
    """Release every captured step of the dict `steps` and empty it."""
    for step in steps.values():
        step.release()
    steps.clear()


def _delta_route(delta):
    """What a captured step remembers of the delta it was recorded with: whether it held edits (the model's route), whether it
    held tombstones (the layers then launch ultra_rspmm_edit_rows, not _delta_rows) and which relation-graph object the relation
    model walked."""
    if delta is None:
        return None
    return (delta.edited, delta.num_removed > 0, id(delta.relation_graph))


def _entity_model(model):
    return getattr(model, "entity_model", model)


@contextlib.contextmanager
def eval_mode(model):
    """Inside the block `model` is in eval mode; on the way out it is in the mode it was in."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def delta_samples_supported(model):
    """Does `model` verify stated facts on a graph that holds edits WITHOUT folding them in first -- forward(leave_out=,
    delta=) with every entity layer on layers._propagate_delta_samples (sum / max, TransE / DistMult)?"""
    try:
        params = inspect.signature(getattr(model, "forward", model)).parameters
    except (TypeError, ValueError):
        return False
    ent = _entity_model(model)
    layers = getattr(ent, "layers", None)
    return ("leave_out" in params and "delta" in params and hasattr(ent, "_forward_leave_out") and layers is not None
            and all(getattr(layer, "delta_samples_supported", lambda: False)() for layer in layers))


def explain_live_blocker(model):
    """None where `model` explains its answers on a graph that holds edits WITHOUT folding them in first
    (visualize_batch(delta=): every entity layer on the batched explanation route, sum / DistMult, fp32); else
    the name of what cannot."""
    try:
        params = inspect.signature(getattr(model, "visualize_batch", None)).parameters
    except (TypeError, ValueError):
        return "%s (no visualize_batch)" % type(model).__name__
    if "delta" not in params:
        return "%s.visualize_batch (takes no delta)" % type(model).__name__
    ent = _entity_model(model)
    layers = getattr(ent, "layers", None)
    if layers is None or not hasattr(ent, "edge_grads_batch"):
        return "%s (no batched explanation route)" % type(ent).__name__
    for i, layer in enumerate(layers):
        if not getattr(layer, "explain_live_supported", lambda: False)():
            return "entity layer %d (%s aggregate, %s messages: the route serves sum / distmult)" % (
                i, getattr(layer, "aggregate_func", "?"), getattr(layer, "message_func", "?"))
        if any(p.dtype != torch.float32 for p in layer.parameters()):
            return "entity layer %d (%s parameters: the route serves fp32)" % (i, next(layer.parameters()).dtype)
    return None


def explain_live_supported(model):
    """Does `model` serve explain_tails / explain_heads(compact=False)?  (explain_live_blocker names what does not)"""
    return explain_live_blocker(model) is None


def live_relation_graph_blocker(model):
    """None where every layer of `model`'s relation model can run on a relation graph that is kept current in place (its
    byte adjacency alone, DESIGN.md 25: sum aggregate, DistMult messages, 64-d, fp32); else the name of what cannot."""
    rel = getattr(model, "relation_model", None)
    if rel is None or not hasattr(rel, "adjacency_blocker"):
        return "%s (no relation model with an adjacency route)" % type(model).__name__
    blocker = rel.adjacency_blocker()
    return None if blocker is None else "relation_model." + blocker


def live_relation_graph_supported(model):
    """Does every relation-model layer of `model` qualify for Predictor(live_relation_graph=True)?"""
    return live_relation_graph_blocker(model) is None


def _check_facts(data, h, r, t, num_live=None, num_direct=None, retired=None):
    """(h, r, t) of verify_*: int64 vectors of one length on the graph's device, r a direct relation (ValueError otherwise);
    num_live (a graph with reserved rows): h and t below it; num_direct (a graph with reserved relation slots): the direct
    relations in use, in place of num_relations // 2; retired (a sorted id vector): h and t are none of them."""
    dev = data.edge_index.device
    h, r, t = (torch.as_tensor(v, dtype=torch.long, device=dev).flatten() for v in (h, r, t))
    if not (h.shape == r.shape == t.shape):
        raise ValueError("one head, relation and tail per fact: got %d heads, %d relations and %d tails" % (len(h), len(r), len(t)))
    direct = int(data.num_relations) // 2 if num_direct is None else int(num_direct)
    if len(r) and bool(((r < 0) | (r >= direct)).any()):
        raise ValueError("verify takes direct relations (r < num_relations // 2 = %d): a fact stated through an inverse relation "
                         "is its direct twin" % direct)
    if num_live is not None:
        check_live(torch.cat([h, t]), num_live, "a fact's head and tail")
    check_not_retired(torch.cat([h, t]), retired, "a fact's head and tail")
    return h, r, t


@torch.no_grad()
def verify_reference(model, data, filter_graph, h, r, t, mode="tail"):
    """Leave-one-out verification in the reference's own terms, on any device: fact i = (h[i], r[i], t[i]) is scored on a
    filtered COPY of the graph without itself and its inverse (BaseNBFNet.remove_easy_edges of that single triple, relation
    graph kept) -- mode="tail": t[i] among all tails of (h[i], r[i], ?); mode="head": h[i] among all heads of (?, r[i], t[i]),
    scored through the inverse relation as in evaluation -- and ranked under the filtered protocol of tasks.py:94-141 against
    `filter_graph`'s known answers (the positive among them; ties count against it).  Returns (score (n) fp32, rank (n)
    int64, num_negative (n) int64).  One plan, one forward per triple: the definition Predictor.verify_* is tested against."""
    if mode not in ("tail", "head"):
        raise ValueError("mode must be 'tail' or 'head', got %r" % (mode,))
    h, r, t = _check_facts(data, h, r, t)
    dev = h.device
    score = torch.empty(len(h), dtype=torch.float32, device=dev)
    rank = torch.empty(len(h), dtype=torch.long, device=dev)
    num_negative = torch.empty(len(h), dtype=torch.long, device=dev)
    ent = _entity_model(model)
    with eval_mode(model):
        for i in range(len(h)):
            batch = torch.stack([h[i:i + 1], t[i:i + 1], r[i:i + 1]], dim=-1)
            without = ent.remove_easy_edges(data, h[i:i + 1], t[i:i + 1], r[i:i + 1])
            cand = tasks.all_negative(data, batch)[0 if mode == "tail" else 1]
            pred = model(without, cand).float()
            mask = tasks.strict_negative_mask(filter_graph, batch)[0 if mode == "tail" else 1]
            pos = batch[:, 1] if mode == "tail" else batch[:, 0]
            score[i] = pred[0, pos[0]]
            rank[i] = tasks.compute_ranking(pred, pos, mask)[0]
            num_negative[i] = mask.sum(dim=-1)[0]
    return score, rank, num_negative


# ---- what-if queries: facts assumed per query ----
def assume_supported(model):
    """Does `model` answer what-if queries (tails(h, r, assuming=) ...) on the cached plan -- forward(delta=) with every entity
    layer on ultra_rspmm_edit_rows_owned: sum / max / min aggregates with TransE / DistMult messages?  (`mean` would need a
    per-sample degree; pna and RotatE have no delta route.)  Another model runs the per-query loop of assume_reference."""
    try:
        params = inspect.signature(getattr(model, "forward", model)).parameters
    except (TypeError, ValueError):
        return False
    layers = getattr(_entity_model(model), "layers", None)
    return ("delta" in params and layers is not None and len(layers) > 0
            and all(getattr(layer, "aggregate_func", None) in ("sum", "max", "min")
                    and getattr(layer, "message_func", None) in ("transe", "distmult") for layer in layers))


def _assumed_lists(data, assuming, n, per_query=None, **live):
    """`assuming` of a call with n queries as a list of n (m_i, 3) int64 (h, r, t) tensors on the graph's device: one (m, 3)
    tensor is assumed by every query; a list or tuple holds one entry per query -- (m_i, 3) rows, or None / empty.  The facts
    follow _check_facts (`live`: its num_live / num_direct / retired; h and t are ALWAYS bounded -- by num_live, else by
    data.num_nodes -- so no id reaches a forward or another query's known-answer keys unchecked); ValueError for a wrong count,
    a wrong shape, or more than per_query facts in one entry."""
    dev = data.edge_index.device
    if live.get("num_live") is None:        # (always bounded: without a reserve every row of the graph is an entity)
        live = dict(live, num_live=int(data.num_nodes))
    if torch.is_tensor(assuming):
        entries = [assuming] * n
    elif isinstance(assuming, (list, tuple)):
        if len(assuming) != n:
            raise ValueError("`assuming` is one (m, 3) tensor for every query or a list with one entry per query: got %d "
                             "entries for %d queries" % (len(assuming), n))
        entries = list(assuming)
    else:
        raise ValueError("`assuming` is one (m, 3) tensor or a list with one entry per query, got %r" % type(assuming).__name__)
    out, checked = [], {}
    for entry in entries:
        if id(entry) not in checked:
            facts = torch.zeros(0, 3, dtype=torch.long) if entry is None else torch.as_tensor(entry, dtype=torch.long)
            if facts.numel() == 0:
                facts = facts.reshape(0, 3)
            if facts.dim() != 2 or facts.shape[1] != 3:
                raise ValueError("assumed facts are (m, 3) rows (h, r, t), got shape %s" % (tuple(facts.shape),))
            if per_query is not None and len(facts) > per_query:
                raise ValueError("a query assumes at most assume_capacity = %d facts, got %d" % (per_query, len(facts)))
            facts = facts.to(dev)
            _check_facts(data, facts[:, 0], facts[:, 1], facts[:, 2], **live)
            checked[id(entry)] = facts
        out.append(checked[id(entry)])
    return out


def _assumed_known(assumed, anchor, relation, mode):
    """The (sample, ids) `extra` of known_answers: the answers of query i that its own assumed facts state -- the tails t of its
    facts (anchor[i], relation[i], t) (mode="tail") or the heads h of its facts (h, relation[i], anchor[i]) (mode="head")."""
    keyed, answer = (0, 2) if mode == "tail" else (2, 0)
    sample, ids = [], []
    for i, facts in enumerate(assumed):
        if len(facts):
            hit = (facts[:, keyed] == anchor[i]) & (facts[:, 1] == relation[i])
            ids.append(facts[hit, answer])
            sample.append(torch.full_like(ids[-1], i))
    if not ids:
        empty = torch.zeros(0, dtype=torch.long, device=anchor.device)
        return empty, empty
    return torch.cat(sample), torch.cat(ids)


def _assumed_graph(graph, facts):
    """A copy of `graph` with the edges of `facts` (m, 3) = (h, r, t) appended -- direct, then inverse -- and everything else,
    the relation graph included, kept."""
    return with_facts(graph, facts[:, 0], facts[:, 1], facts[:, 2]) if len(facts) else graph


@torch.no_grad()
def assume_reference(model, data, filter_graph, anchor, relation, assuming, k=10, mode="tail", min_score=None, num_live=None,
                     retired=None, among=None):
    """What-if queries in plain terms, on any device -- the DEFINITION Predictor.tails / heads / tails_above / heads_above
    (assuming=) are tested against.  Query i = (anchor[i], relation[i]) is answered on a COPY of `data` with its assumed facts
    appended -- [data's edges ; its direct edges (h, t, r) in the given order ; their inverse edges], duplicates kept, the
    relation graph kept as it is (the reference keeps it when a sample's edge set differs: remove_easy_edges) -- by one forward,
    and filtered against `filter_graph` (None: no filter) plus its own assumed facts: filtered_topk_reference, or with
    min_score filtered_above_reference.  No other query sees the facts; nothing is stated.  assuming: one (m, 3) tensor of
    (h, r, t) rows for every query, or a list with one entry per query (rows, None or empty).  Returns (ids (n, k), scores
    (n, k), count (n)), or with min_score (ptr (n + 1), ids, scores, size (n)).  One plan and one forward per query.
    num_live, retired, among: those of the _reference selections -- among is one id vector for every query or a list of one
    per query (the candidate set of `Predictor.tails(among=)`)."""
    if mode not in ("tail", "head"):
        raise ValueError("mode must be 'tail' or 'head', got %r" % (mode,))
    dev = data.edge_index.device
    anchor = torch.as_tensor(anchor, dtype=torch.long, device=dev).flatten()
    relation = torch.as_tensor(relation, dtype=torch.long, device=dev).flatten()
    assumed = _assumed_lists(data, assuming, len(anchor))
    select = {} if num_live is None else {"num_live": num_live}
    if retired is not None:
        select["retired"] = retired
    rows = []
    with eval_mode(model):
        for i, facts in enumerate(assumed):
            a, r = anchor[i:i + 1], relation[i:i + 1]
            graph = _assumed_graph(data, facts)
            pred = model(graph, _candidates(graph, a, r, mode)).float()
            ptr = index = None
            if filter_graph is not None:
                ptr, index = known_answers(_assumed_graph(filter_graph, facts), a, r, mode)
            if among is not None:
                select["among"] = [among[i] if isinstance(among, (list, tuple)) else among]
            if min_score is None:
                rows.append(filtered_topk_reference(pred, k, ptr, index, **select))
            else:
                rows.append(filtered_above_reference(pred, min_score, ptr, index, **select))
    if min_score is None:
        if not rows:
            return (torch.zeros(0, k, dtype=torch.long, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev),
                    torch.zeros(0, dtype=torch.long, device=dev))
        return tuple(torch.cat([row[j] for row in rows]) for j in range(3))
    return _join_above(rows, dev)


def _check_per_query(per_query, k, name="per_query"):
    if per_query is not None and (isinstance(per_query, bool) or not isinstance(per_query, int) or not 1 <= per_query <= k):
        raise ValueError("%s must be None or an int in [1, k = %d], got %r" % (name, k, per_query))


@torch.no_grad()
def best_reference(model, data, filter_graph, anchor, relation, k, mode="tail", min_score=None, per_query=None, among=None,
                   num_live=None, retired=None):
    """The best k (query, answer) pairs over ALL the queries (anchor[i], relation[i]) in plain terms, on any device -- the
    DEFINITION Predictor.best_tails / best_heads / propose_tails / propose_heads are tested against.  Query i
    is answered by one forward on `data` and filtered against `filter_graph` (None: no filter): its list is the first
    `per_query or k` answers of filtered_topk_reference.  All lists are laid end to end in query order, the pads are dropped,
    with min_score every pair whose score is not > min_score in fp32 is dropped (a NaN is), and ONE stable descending sort
    ranks the rest: score descending, then query ascending, then id ascending, NaN on top, -0.0 == +0.0.  Returns (query (k)
    int64 -- positions in `anchor` --, ids (k) int64, scores (k) fp32, count (0-d int64)), -1 / -1 / -inf beyond count.
    num_live, retired, among: those of filtered_topk_reference -- among is one id vector for every query or a list of one per
    query.  Nothing here goes batch by batch or through merge_pairs_reference."""
    if mode not in ("tail", "head"):
        raise ValueError("mode must be 'tail' or 'head', got %r" % (mode,))
    check_k(k)
    _check_per_query(per_query, k)
    dev = data.edge_index.device
    anchor = torch.as_tensor(anchor, dtype=torch.long, device=dev).flatten()
    relation = torch.as_tensor(relation, dtype=torch.long, device=dev).flatten()
    select = {} if num_live is None else {"num_live": num_live}
    if retired is not None:
        select["retired"] = retired
    query, answer, score = [], [], []
    with eval_mode(model):
        for i in range(len(anchor)):
            a, r = anchor[i:i + 1], relation[i:i + 1]
            pred = model(data, _candidates(data, a, r, mode)).float()
            ptr = index = None
            if filter_graph is not None:
                ptr, index = known_answers(filter_graph, a, r, mode)
            if among is not None:
                select["among"] = [among[i] if isinstance(among, (list, tuple)) else among]
            ids, scores, count = filtered_topk_reference(pred, per_query or k, ptr, index, **select)
            m = int(count[0])
            query.append(torch.full((m,), i, dtype=torch.long, device=dev))
            answer.append(ids[0, :m])
            score.append(scores[0, :m])
    out = (torch.full((k,), -1, dtype=torch.long, device=dev), torch.full((k,), -1, dtype=torch.long, device=dev),
           torch.full((k,), float("-inf"), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.long, device=dev))
    if not query:
        return out
    query, answer, score = torch.cat(query), torch.cat(answer), torch.cat(score)
    if min_score is not None:
        member = score > torch.tensor(_fp32_threshold(min_score), dtype=torch.float32, device=dev)
        query, answer, score = query[member], answer[member], score[member]
    order = torch.sort(score, descending=True, stable=True).indices[:k]
    m = order.numel()
    out[0][:m], out[1][:m], out[2][:m] = query[order], answer[order], score[order]
    out[3].fill_(m)
    return out


def _join_above(parts, dev):
    """The (ptr, ids, scores, size) of a whole call from those of its consecutive parts."""
    out_ptr, at = [torch.zeros(1, dtype=torch.long, device=dev)], 0
    for ptr, ids, _, _ in parts:
        out_ptr.append(ptr[1:] + at)
        at += ids.numel()
    if not parts:
        return (out_ptr[0], torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.long, device=dev))
    return (torch.cat(out_ptr),) + tuple(torch.cat([part[j] for part in parts]) for j in (1, 2, 3))


def _assume_route(delta):
    """What a captured what-if step remembers of the delta under its overlay: the relation-graph object alone (the owned entry
    takes tombstones or none in the same launch, and an empty overlay is a launch that ends at once)."""
    return None if delta is None else id(delta.relation_graph)


class _GraphedAssumeStep(_GraphedPredictStep):
    """_GraphedPredictStep for what-if queries: the model is handed `overlay` -- an rspmm.AssumedFacts over the
    predictor's delta with room for `per_query` facts a query -- so every entity layer records ultra_rspmm_edit_rows_owned over
    the overlay's buffers.  Between replays the host refills the overlay (`overlay.fill`); nothing is recorded again."""

    def __init__(self, model, data, batch_size, k, mode, index_capacity, per_query, **kwargs):
        self.per_query = per_query
        _GraphedPredictStep.__init__(self, model, data, batch_size, k, mode, index_capacity, **kwargs)

    def _model_delta(self, data, delta, batch_size):
        self.route = _assume_route(delta)
        self.overlay = rspmm.AssumedFacts(data, delta, batch_size, self.per_query)
        return self.overlay


class _GraphedBestStep(_GraphedPredictStep):
    """_GraphedPredictStep for the best pairs over many queries: the predict step with k_row answers a query,
    followed in the same capture by ultra_topk_pairs_merge into the step's own running list of `k_best` slots (`best`).  The
    merge reads at replay `where` = (query_base, n_rows) -- the batch's first query and how many of its rows are no padding --
    and, for a step made `with_floor`, the one float `min_score`; the host rewrites them between replays and zeroes the count
    (best[3]) ahead of a call's first batch.  Nothing is recorded again for another call of the same shape."""

    def __init__(self, model, data, batch_size, k_best, k_row, mode, index_capacity, with_floor, **kwargs):
        dev = data.edge_index.device
        self.k_best, self.k_row, self.with_floor = k_best, k_row, with_floor
        self.best = empty_pairs(k_best, dev)
        self.where = torch.zeros(2, dtype=torch.long, device=dev)
        self.min_score = torch.full((1,), float("-inf"), dtype=torch.float32, device=dev)
        _GraphedPredictStep.__init__(self, model, data, batch_size, k_row, mode, index_capacity, **kwargs)

    def _after_selection(self):
        merge_pairs(self.best, self.ids, self.scores, self.where[0:1], self.where[1:2], self.min_score if self.with_floor else None)


class _GraphedVerifyStep(_IndexedStep):
    """One batch of stated facts of one direction as ONE hipGraph replay (a graph.Capture, like _GraphedPredictStep): the
    leave-one-out keep rows from the (bs, 3) triples (ultra_leave_one_out_keep into the step's (bs, num_edge) fp32 buffer), the
    candidates, the masked forward on the full graph's cached plans, ultra_filtered_rank and the gather of the positives' scores.
    Per batch the host copies the triples and the (bs + 1) offsets into the known lists of the whole call (`load_index`)."""

    def __init__(self, model, data, batch_size, mode, index_capacity, warmup=2, n_live=None, delta=None, retired=None,
                 among=None):
        """among: as in _GraphedPredictStep -- ultra_filtered_rank_among, which zeroes with a kernel.
        n_live: as in _GraphedPredictStep -- ultra_filtered_rank_live over the live ids, or (None) ultra_filtered_rank.
        retired: as in _GraphedPredictStep -- ultra_filtered_rank_alive, which takes a NULL live count and zeroes with a kernel.
        delta (rspmm.GraphDelta or None; a model with the leave_out route): while it holds no edit the step records the masked
        forward above; once it holds facts or tombstones it records model(..., leave_out=triples, delta=delta) -- the keep rows
        over the base edge list, the same edges as per-sample keys (GraphDelta.sample_keys into the step's own key buffers) and
        the delta's fix-up launches, which read its device buffers at replay.  `route` is what the Predictor compares."""
        _IndexedStep.__init__(self, model, data, batch_size, index_capacity, delta, n_live, retired, among)
        dev = data.edge_index.device
        self.mode = mode
        live = delta is not None and delta.edited
        # (row, col, type) of every sample's two dead edges: allocated once, at fixed addresses
        self.keys = tuple(torch.zeros(batch_size, 2, dtype=torch.int32, device=dev) for _ in range(3)) if live else None
        self.triples = torch.zeros(batch_size, 3, dtype=torch.long, device=dev)       # (h, t, r)
        self.keep = torch.empty(batch_size, data.edge_index.shape[1], dtype=torch.float32, device=dev)
        self.score = torch.empty(batch_size, dtype=torch.float32, device=dev)
        self.rank = torch.empty(batch_size, dtype=torch.long, device=dev)
        self.num_negative = torch.empty(batch_size, dtype=torch.long, device=dev)
        ent = _entity_model(model)
        # The live route is replayed between eager edits (add_facts / remove_facts run torch ops of their own), and a memset node
        # captured into a hipGraph replays wrongly once eager memsets interleave with the replays (csrc/rank_kernels.hip): its
        # rank goes through the live-count entry, which zeroes with a kernel -- over all n ids where no rows are reserved.
        self.n_all = (torch.full((1,), int(data.num_nodes), dtype=torch.long, device=dev)
                      if live and n_live is None and retired is None and among is None else None)
        rank_count = n_live if n_live is not None else self.n_all

        def step():
            h, t, r = self.triples.unbind(-1)
            anchor, pos = (h, t) if mode == "tail" else (t, h)
            if live:
                pred = model(data, _candidates(data, anchor, r, mode), leave_out=self.triples,
                             leave_out_buffers=(self.keep, self.keys), delta=delta).float().contiguous()
            else:
                keep = ent.leave_one_out_keep(data, self.triples, out=self.keep, validate=False)
                pred = model(data, _candidates(data, anchor, r, mode), edge_keep=keep).float().contiguous()
            pos = pos.contiguous()
            if among is None:
                filtered_rank(pred, pos, self.ptr, self.index, num_live=rank_count, retired=retired, out=(self.rank, self.num_negative))
            else:
                filtered_rank(pred, pos, self.ptr, self.index, num_live=n_live, retired=retired, out=(self.rank, self.num_negative),
                              among=(self.among_span, self.among_index), among_capacity=self.among_capacity)
            self.score.copy_(pred.gather(1, pos.unsqueeze(-1)).squeeze(-1))

        self.record_step(step, warmup, (self.triples,), (self.score, self.rank, self.num_negative))



class Predictor(object):
    """Top-k answers of link-prediction queries on one graph.

        predictor = Predictor(model, data, k=10)
        ids, scores, count = predictor.tails(h, r)       # (n, k), (n, k), (n): the best tails of every (h[i], r[i], ?)
        ids, scores, count = predictor.heads(t, r)       # ... the best heads of every (?, r[i], t[i])
        ids, scores, count, why = predictor.explain_tails(h, r)    # ... and the top paths behind every answer (explain_heads alike)
        score, rank, num_negative = predictor.verify_tails(h, r, t)     # each fact scored on the graph without itself

    Known answers are left out (filtered=True): the tails of (h, r, .) / heads of (., r, t) in the filter graph --
    `filtered_data`, else data.filtered_data when present, else `data` (the rule of eval.evaluate).  On the GPU with use_graph
    every batch of batch_size queries is one hipGraph replay; one capture per direction is made on first use and kept (and
    made again when the model's parameters change or a call's known lists outgrow the capture's buffer).  A last batch
    shorter than batch_size is padded with copies of its last query and the padded rows are dropped.  A model outside the
    fused inference path (models.NotOnFusedPath) runs batch by batch without a capture.  One step in flight, one stream.

    A LIVE graph: add_facts(h, r, t) states new facts between existing entities.  They are held in a delta of
    up to `delta_capacity` facts beside the cached plan of `data` (rspmm.GraphDelta) and join the filter graph, so a tail that
    was just stated is a known answer from then on; tails / heads / tails_above / heads_above answer on the graph with the
    facts, exactly as a fresh Predictor on the materialised graph (GraphDelta.materialize) would.  The captured step is made
    again when the first facts arrive and when the relation graph changes; otherwise a further add_facts costs no capture and
    no plan.  remove_facts(h, r, t) retracts facts: every edge equal to (h, t, r) or its inverse leaves the served
    graph -- base edges as tombstones beside the same cached plan, added facts out of the delta -- and the filter graph, so a
    retracted tail can be returned as an answer again.  The captured step is made again when the first tombstone arrives; from
    then on further remove_facts / add_facts cost no capture and no plan unless the relation graph changes.  compact() folds
    the delta, tombstones included, into `data` (a host plan, new captures); add_facts / remove_facts do so themselves when
    the capacity would be exceeded, and explain_* does so first when the delta holds edits.  verify_* does NOT:
    fact i is scored on the materialised graph without itself, whether its edges are base edges or were just stated, on the
    same cached plan -- per-sample keep rows over the base edge list plus the same edges as per-sample keys for the rows an
    edit points into (ultra_rspmm_edit_rows_samples).  Its captured step follows the rule of the answer steps: made again
    when the first edits and the first tombstone arrive and when the relation-graph object changes, otherwise add_facts ->
    verify_* costs no plan and no capture.  A model whose layers do not serve that route (mean / min / pna aggregates, RotatE
    messages: delta_samples_supported) is verified after a compaction, as before; so is every model on a predictor with a
    reserve (entity_capacity > 0), whose "compact first" rule of DESIGN.md 19 stays.

    A GROWING graph: entity_capacity=M > 0 reserves M rows for entities that arrive later.  The graph served is
    then a shallow copy of `data` with num_nodes = N + M SLOTS (the same edge list; its own relation graph, equal to the
    unpadded one), `num_entities` of them live; add_entities(count) hands out the next ids and does nothing else -- no plan, no
    capture: the live count also lives in one device int64 (`live_count`, the same tensor for the predictor's life) that the
    selection kernels read at replay.  The new ids are heads, tails and anchors like any other from then on; an id in
    [num_entities, slots) is a ValueError everywhere and never an answer.  Every result is that of a fresh
    Predictor(entity_capacity=0) on delta.materialize(data, num_nodes=num_entities).  A call that would exceed the reserve
    compacts and reserves M rows anew (one rebuild).  entity_capacity=0 (the default): `data` itself is served, by exactly the
    entry points of before, and add_entities raises.

    A growing VOCABULARY: relation_capacity=K > 0 reserves K direct relation slots for relation types that arrive
    later.  The graph served is then a shallow copy of `data` laid out over R + K direct slots (num_relations = 2 (R + K), every
    inverse type moved from r + R to r + R + K, its own relation graph in which the unused slots are isolated nodes),
    `num_direct_relations` of them in use; add_relations(count) hands out the next direct ids and does nothing else.  A relation
    argument is a direct relation below num_direct_relations everywhere (ValueError otherwise), and every relation id handed back
    -- materialized(), the paths of explain_* -- is in the compact numbering, inverse type r + num_direct_relations.  Every result
    is that of a fresh Predictor on materialized().  explain_* and verify_* compact first where the delta is edited (the slot
    counts stay).  Both reserves may be used together.  relation_bits_budget: rspmm.GraphDelta's.

    A relation graph kept current IN PLACE: live_relation_graph=True (default False: everything above).  From the
    first add_facts on, the delta's relation graph is ONE tasks.LiveRelationGraph whose cells are rewritten in place, and the
    relation model reads its byte adjacency without a plan -- so a fact that changes relation-graph cells (every first fact
    through a new relation does) costs no relation-graph plan and no new capture: the captured steps see the new cells at
    their next replay.  remove_facts keeps the object too.  Results are those of the flag-off route, bit for bit.  Needs a
    relation model of sum / DistMult 64-d layers (live_relation_graph_supported; ValueError otherwise) and applies on the GPU
    to relation graphs of at most 1024 nodes; elsewhere the flag-off route runs.  A replay still in flight while add_facts
    writes is the caller's to order, as for the delta's own buffers.

    RETIRED entities: remove_entities(ids) takes entities out of the served graph -- every fact that names one is
    retracted (remove_facts: tombstones, the delta, the filter graph) and the id is retired: never an answer, never counted in
    count / size / num_negative, a ValueError as an anchor and as h / t of add_facts / remove_facts / verify_*.  Ids are not
    renumbered and a retired slot is not handed out again; `num_retired` and `retired_entities` tell which.  The retired set
    lives in one device bitmap and one device int64 that the ultra_filtered_*_alive entries read at replay: the first
    retirement makes the captured steps again (as the first tombstone does), later ones cost no capture.  Every result is that
    of a fresh Predictor on materialized() -- which keeps the id space, the retired ids isolated nodes -- with the retired ids
    taken out of the candidate set.  A predictor that never retires calls exactly the entries it called before."""

    def __init__(self, model, data, k=10, batch_size=8, filtered_data=None, filtered=True, use_graph=True, delta_capacity=256,
                 entity_capacity=0, relation_capacity=0, relation_bits_budget=256 << 20, live_relation_graph=False,
                 assume_capacity=8):
        check_k(k)
        if isinstance(assume_capacity, bool) or not isinstance(assume_capacity, int) or assume_capacity < 1:
            raise ValueError("assume_capacity must be a positive int (facts one query may assume), got %r" % (assume_capacity,))
        self.assume_capacity = assume_capacity
        self._assume_eager_only = False
        self._assume_overlay = None         # (delta, overlay): the overlay of the eager what-if batches
        if not isinstance(live_relation_graph, bool):
            raise ValueError("live_relation_graph must be True or False, got %r" % (live_relation_graph,))
        if live_relation_graph:
            blocker = live_relation_graph_blocker(model)
            if blocker is not None:
                raise ValueError("live_relation_graph=True needs a relation model whose layers all run on the relation graph's "
                                 "byte adjacency (sum aggregate, DistMult messages, 64-d, fp32): %s does not" % blocker)
        if filtered_data is None:
            filtered_data = getattr(data, "filtered_data", None)
        # (a model whose forward takes no `delta` is served by compacting at every add_facts)
        try:
            takes_delta = "delta" in inspect.signature(getattr(model, "forward", model)).parameters
        except (TypeError, ValueError):
            takes_delta = False
        self._steps = {}
        self._eager_only = False
        # (a rebuild drops the captures.  The hook holds the dict, not the predictor: no cycle, so __del__ runs with the last reference)
        self._live = LiveGraph(data, delta_capacity, entity_capacity, filter_data=filtered_data, keep_filter=True,
                               delta_policy="eager" if takes_delta else "never", owner="Predictor",
                               on_rebuild=functools.partial(_release, self._steps), relation_capacity=relation_capacity,
                               relation_bits_budget=relation_bits_budget, live_relation_graph=live_relation_graph)
        self.model, self.k, self.batch_size = model, k, int(batch_size)
        self.filtered, self.use_graph = bool(filtered), bool(use_graph)
        # (ids are stable: the sets outlive compact() and a rebuild.  The registry reads the slot count off the LiveGraph, not
        # off the predictor: no cycle, so __del__ runs with the last reference)
        self._sets = CandidateSets(functools.partial(getattr, self._live, "num_slots"))

    # ---- the state of the served graph: held by the LiveGraph ("The live graph's state in one place") ----
    data = forwarded("graph")
    filter_graph = forwarded("filter_graph")
    delta = forwarded("delta")
    entity_capacity = forwarded("entity_capacity")
    delta_capacity = forwarded("delta_capacity")
    num_entities = forwarded("num_entities")
    num_slots = forwarded("num_slots")
    live_count = forwarded("live_count")
    relation_capacity = forwarded("relation_capacity")
    live_relation_graph = forwarded("live_relation_graph")
    num_direct_relations = forwarded("num_direct_relations")
    num_relation_slots = forwarded("num_relation_slots")
    num_retired = forwarded("num_retired")
    retired_entities = forwarded("retired_entities")

    # ---- candidate sets ----
    def define_set(self, name, ids):
        """Name a candidate set: `among=name` of tails / heads / ..._above / verify_* / explain_* then restricts a query's
        candidates to `ids` -- any slots of the graph, sorted and de-duplicated here (ValueError outside [0, num_slots)); an id
        in the reserve or a retired one is absent until it is live and alive.  Replaces a set of that name; returns its size."""
        return self._sets.define_set(name, ids)

    def drop_set(self, name):
        self._sets.drop_set(name)

    def sets(self):
        """{name: size} of the candidate sets defined now."""
        return self._sets.sets()

    # ---- the growing vocabulary ----
    def add_relations(self, count=1):
        """`count` new relation types: returns their direct ids [num_direct_relations, num_direct_relations + count) (int64, on
        the graph's device) and raises the live count.  Nothing else happens -- no plan, no relation graph, no capture: a slot
        without facts is an isolated node the relation graph already holds; add_facts / tails / heads / ... take the ids from
        now on, and the first facts through one cost what any fact that changes the relation graph costs.  Beyond the reserve
        the graph is compacted and num_direct_relations + count + relation_capacity slots are laid out: one rebuild.
        ValueError on a predictor without a reserve (relation_capacity=0)."""
        return self._live.add_relations(count, compact=self.compact)

    # ---- the growing graph ----
    def add_entities(self, count=1):
        """`count` new entities: returns their ids [num_entities, num_entities + count) (int64, on the graph's device) and raises
        the live count -- the host int and the device scalar the captured selection reads.  Nothing else happens: no plan, no
        capture, no relation graph (an entity without facts plays no role); it is a candidate of every query from now on, scored
        as an isolated node, and add_facts / remove_facts / tails / heads / ... take its id.  Beyond the reserve the graph is
        compacted and num_entities + count + entity_capacity slots are laid out: one rebuild.  ValueError on a predictor
        without a reserve (entity_capacity=0)."""
        return self._live.add_entities(count, compact=self.compact)

    def materialized(self):
        """The graph a fresh Predictor would be given for the same answers: the served edge list with the delta's edits
        (GraphDelta.materialize) and num_nodes = num_entities -- no reserved row -- with the filter graph held now as its
        `filtered_data` where that is a graph of its own.  A new copy at every call."""
        return self._live.materialized()

    # ---- the live graph ----
    def add_facts(self, h, r, t):
        """State the facts (h[i], r[i], t[i]) -- ints or vectors; r direct relations, h and t existing entities (ValueError
        otherwise: the sets of entities and relations are fixed).  Each adds the edges (h, t, r) and (t, h, r + num_relations / 2)
        to the served graph and to the filter graph; a repeated fact is one more parallel edge.  Returns the number of facts the
        delta holds afterwards (0 after a compaction: more facts than delta_capacity, or a model without a delta route)."""
        before = self._relation_graph_state()
        out = self._live.add_facts(h, r, t)
        self._relation_graph_edited(before)
        return out

    def remove_facts(self, h, r, t):
        """Retract the facts (h[i], r[i], t[i]) -- the argument rules of add_facts -- one after the other: every edge equal to
        (h, t, r) or (t, h, r + num_relations / 2) leaves the served graph and the filter graph (a fact stated nowhere is a
        no-op).  Returns an int64 vector: the number of direct edges each fact took out of the served graph
        (GraphDelta.remove).  Compacts first where the delta cannot hold the tombstones."""
        before = self._relation_graph_state()
        out = self._live.remove_facts(h, r, t)
        self._relation_graph_edited(before)
        return out

    def remove_entities(self, ids):
        """Retire the entities `ids` -- an int or a vector of distinct ids in use, none retired before (ValueError otherwise):
        every fact that names one as head or tail is retracted (remove_facts) and the ids are never an answer, a candidate that
        is counted, an anchor or an argument of an edit again (LiveGraph.remove_entities).  Returns an int64 vector: per id the
        number of distinct facts retracted."""
        before = self._relation_graph_state()
        out = self._live.remove_entities(ids)
        self._relation_graph_edited(before)
        return out

    retire_entities = remove_entities       # (the one spelling QueryPredictor has too: DESIGN.md §29, "The name")

    def _relation_graph_state(self):
        rg = None if self.delta is None else self.delta.relation_graph
        return (rg, getattr(rg, "version", None))

    def _relation_graph_edited(self, before):
        """A live relation graph that changed in place under a model that holds a relation table
        (Ultra.cache_relation_representations): a captured step gathers from the table it was recorded with, which is stale
        now -- the table is dropped and the steps are made again (they then run the relation model)."""
        rg, version = self._relation_graph_state()
        if rg is before[0] and version != before[1] and getattr(self.model, "_rel_table", None) is not None:
            self.model.drop_relation_cache()
            _release(self._steps)

    def compact(self, extra=None, delta=None, slots=None, relation_slots=None):
        """Fold the delta's edits (and `extra` = (h, r, t), checked by the caller) into `data`: the materialised graph -- without
        the tombstoned edges, with the added ones -- becomes the served graph -- its relation graph rebuilt, a host plan on the
        next query, new captures -- and the delta is emptied.  `delta`: fold that one instead of the Predictor's own.  The
        slot counts and the live counts of a graph with reserved rows or relation slots stay; `slots` (add_entities beyond the
        reserve): the new slot count, laid out in the same rebuild; `relation_slots` (add_relations beyond its reserve): the
        new count of direct relation slots."""
        self._live.compact(extra, delta, slots, relation_slots)

    def _model_kwargs(self):
        delta = self.delta      # (handed over whenever it exists, empty or not: the capture relies on it)
        return {} if delta is None else {"delta": delta}

    def tails(self, h, r, among=None, assuming=None):
        """assuming (None: nothing): facts ASSUMED for this call only -- "if (a, r', b) were true, what would the
        tails of (h, r, ?) be?".  One (m, 3) int64 tensor of (h, r, t) rows is assumed by every query; a list holds one entry
        per query ((m_i, 3) rows, None or empty).  Query i is answered on [materialised served graph ; its direct edges in the
        given order ; their inverse edges] with the served relation graph, and filtered against the filter graph plus its own
        assumed facts: an assumed tail of (h[i], r[i], ?) is a known answer of query i only.  Nothing is stated -- materialized(),
        the delta, the filter graph and the other routes' captures are untouched, and query j never sees query i's facts.  The
        facts follow add_facts' rules (ValueError); at most `assume_capacity` a query (ValueError).  On the GPU a batch is one
        replay of a captured step of its own (key (mode, "assume")) whose entity layers run ultra_rspmm_edit_rows_owned over
        an overlay (rspmm.AssumedFacts) that the host refills between replays; a model outside assume_supported, and every
        call off the GPU, runs assume_reference's loop.  A call whose assumptions are all empty is the call without them.
        among (None: every entity): the candidates of query i are the ids of a set -- a name (define_set), a 1-D
        id vector or list (one set for every query) or a sequence of one name or vector per query (ValueError for a wrong
        count, KeyError for an unknown name, ValueError for an id outside [0, num_slots)) -- that are live, alive and not
        known: count[i] = min(k, how many there are).  The selection gathers the listed scores (ultra_filtered_topk_among): the
        same order and bits as the full ranking restricted to the set.  Captured under a key of its own; a later call whose
        sets fit the step's buffers records nothing."""
        return self._run(*self._query(h, r), "tail", among, assuming)

    def heads(self, t, r, among=None, assuming=None):
        return self._run(*self._query(t, r), "head", among, assuming)

    def tails_above(self, h, r, min_score, among=None, assuming=None):
        """Every tail of (h[i], r[i], ?) whose logit exceeds `min_score` (a Python float: the threshold of
        filtered_above_reference), ranked: (ptr (n + 1) int64, ids, scores, size (n) int64) for the whole call, in query order
        -- the set of query i is ids[ptr[i] : ptr[i + 1]], best first; known answers are left out as in `tails`, while size[i]
        counts every entity above the threshold, known ones included.  The forward runs eagerly, batch by batch, and
        ultra_filtered_above selects on the device; the host reads one number per batch (the batch's total) to slice the
        batch's lists out of their full-capacity buffers.  Off the GPU the plain-torch restatement selects, as in `tails`."""
        return self._run_above(h, r, min_score, "tail", among, assuming)

    def heads_above(self, t, r, min_score, among=None, assuming=None):
        """tails_above for the heads of (?, r[i], t[i])."""
        return self._run_above(t, r, min_score, "head", among, assuming)

    # ---- the best pairs over many queries: link discovery ----
    def best_tails(self, h, r, k=None, among=None, min_score=None, per_query=None):
        """The best k (default: the predictor's k) (query, tail) pairs over ALL the queries (h[i], r[i], ?) of the call:
        (query (k) int64 -- positions in h --, ids (k) int64, scores (k) fp32, count (0-d int64)); slots beyond count hold
        -1 / -1 / -inf.  Order: score descending, then query ascending, then id ascending, NaN on top, -0.0 == +0.0 -- the
        stable descending sort of the queries' row-wise lists laid end to end (best_reference is the definition).  Known answers
        are left out and `among` restricts the candidates as in `tails`; min_score (a Python float, finite or -inf) keeps only
        pairs whose logit exceeds it, as in `tails_above`; per_query (an int in [1, k]) caps how many pairs one query may
        contribute.  On the GPU every batch is one replay of a captured step of its own (key (mode, "best", k, k_row) ...): the predict
        step with per_query or k answers a row, then ultra_topk_pairs_merge into a running list on the device, which is read
        once after the last replay -- no per-batch copy-out.  A second call with the same k / per_query records nothing, whatever
        the queries and min_score.  Off the GPU, without use_graph and for a model outside the fused path: filtered_topk and
        merge_pairs (or their _reference twins) batch by batch."""
        return self._run_best(*self._query(h, r), "tail", k, among, min_score, per_query)

    def best_heads(self, t, r, k=None, among=None, min_score=None, per_query=None):
        """best_tails for the heads of (?, r[i], t[i]): `ids` are heads, `query` positions in t."""
        return self._run_best(*self._query(t, r), "head", k, among, min_score, per_query)

    def propose_tails(self, r, heads=None, k=None, among=None, min_score=None, per_head=None):
        """Which facts of the direct relation `r` are most likely MISSING from the graph?  The best k triples (head, r, tail)
        over the heads `heads` -- None: every entity in use (below the live count, not retired); the name of a set
        (define_set: its ids that are in use); or an id vector (entities in use, ValueError otherwise) --, de-duplicated and
        ascending, that the filter graph does not state: (heads (k), tails (k), scores (k), count), -1 / -1 / -inf beyond count,
        ordered by (score descending, head ascending, tail ascending).  best_tails over those heads: k, among (the tails'
        candidate set), min_score as there; per_head caps the proposals of one head.  Added and retracted facts, new and
        retired entities and relations are served as `tails` serves them -- the step is the predict step."""
        heads, relation = self._proposers(r, heads, "heads")
        query, ids, scores, count = self._run_best(heads, relation, "tail", k, among, min_score, per_head, "per_head")
        return torch.where(query >= 0, heads[query.clamp(min=0)] if len(heads) else query, query), ids, scores, count

    def propose_heads(self, r, tails=None, k=None, among=None, min_score=None, per_tail=None):
        """propose_tails from the other side: the best k triples (head, r, tail) over the tails `tails`, the heads ranked by
        best_heads -- (heads (k), tails (k), scores (k), count), ordered by (score descending, tail ascending, head ascending)."""
        tails, relation = self._proposers(r, tails, "tails")
        query, ids, scores, count = self._run_best(tails, relation, "head", k, among, min_score, per_tail, "per_tail")
        return ids, torch.where(query >= 0, tails[query.clamp(min=0)] if len(tails) else query, query), scores, count

    def _proposers(self, r, which, what):
        """(anchors, relation) of propose_*: the entities `which` (None, a set's name or ids) ascending and distinct, and `r`
        -- one direct relation in use -- once for each."""
        dev = self.data.edge_index.device
        if isinstance(r, bool) or (torch.is_tensor(r) and r.numel() != 1) or not (torch.is_tensor(r) or isinstance(r, int)):
            raise ValueError("propose takes ONE direct relation (an int), got %r" % (r,))
        r = int(r)
        if not 0 <= r < self.num_direct_relations:
            raise ValueError("propose takes a direct relation in use (0 <= r < %d), got %d" % (self.num_direct_relations, r))
        if which is None or isinstance(which, str):
            ids = torch.arange(self.num_entities, device=dev) if which is None else self._sets.resolve(which, 1)[0][1].to(dev)
            keep = ids < self.num_entities
            keep[torch.isin(ids, self.retired_entities.to(dev))] = False
            ids = ids[keep]
        else:
            ids = torch.unique(torch.as_tensor(which, dtype=torch.long, device=dev).flatten())
            if len(ids) and (int(ids[0]) < 0 or int(ids[-1]) >= self.num_slots):
                raise ValueError("the %s of a proposal are entity ids in [0, %d)" % (what, self.num_slots))
        anchors, relation = self._query(ids, torch.full_like(ids, r))
        return anchors, relation

    @torch.no_grad()
    def _run_best(self, anchor, relation, mode, k, among, min_score, per_query, per_name="per_query"):
        """best_tails / best_heads of the queries (anchor, relation) as _query gives them."""
        k = self.k if k is None else k
        check_k(k)
        _check_per_query(per_query, k, per_name)
        k_row = per_query or k
        floor = None if min_score is None else _fp32_threshold(min_score)
        data, bs, live, model_kwargs = self.data, self.batch_size, self._live, self._model_kwargs()
        dev = data.edge_index.device
        n = len(anchor)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        state = {"best": empty_pairs(k, dev), "step": None}      # the eager route's list; the captured step that served the call
        if n:
            with eval_mode(self.model):
                ptr = index = None
                if self.filtered:       # the known lists of the whole call, once
                    ptr, index = known_answers(self.filter_graph, anchor, relation, mode)

                def eager(lo):
                    pred = self.model(data, _candidates(data, anchor[lo:lo + bs], relation[lo:lo + bs], mode), **model_kwargs).float()
                    on_gpu = pred.is_cuda
                    ids, scores, _ = (filtered_topk if on_gpu else filtered_topk_reference)(
                        pred, k_row, None if ptr is None else ptr[lo:lo + len(pred) + 1], index, **live.selection_for(on_gpu),
                        **self._among_for(among, lo, len(pred), on_gpu))
                    state["best"] = (merge_pairs if on_gpu else merge_pairs_reference)(state["best"], ids, scores, lo, None, floor)
                    state["step"] = None
                    return ()

                starts = torch.arange(0, n, bs, device=dev)
                where = torch.stack([starts, (n - starts).clamp(max=bs)], dim=1)      # (query_base, n_rows) of every batch

                def before(step, lo):
                    if lo == 0:     # a new call: the running list is empty, the floor is this call's
                        step.best[3].fill_(0)
                        if floor is not None:
                            step.min_score.fill_(floor)
                    step.where.copy_(where[lo // bs], non_blocking=True)
                    state["step"] = step

                # (k and k_row are part of the key: a caller who alternates two values keeps both captures)
                key = (mode, "best", k, k_row) + (() if floor is None else ("floor",)) + (() if among is None else ("among",))
                self._batched(key, lambda capacity, among_sizes=None: _GraphedBestStep(
                    self.model, data, bs, k, k_row, mode, capacity, floor is not None, delta=self.delta, n_live=self.live_count,
                    retired=self._live.retired_operand, **({} if among_sizes is None else {"among": among_sizes})),
                    (anchor, relation), ptr, index, state["best"][:1], eager, among=among, before=before, copy_out=False)
        query, ids, scores, count = (t.clone() for t in (state["best"] if state["step"] is None else state["step"].best))
        return query, ids, scores, count.reshape(())

    def explain_tails(self, h, r, chunk=16, compact=True, among=None):
        """tails(h, r) plus why: (ids, scores, count, explanations).  explanations[i][j], j < count[i], is the (paths, weights)
        of model.visualize_batch for the triple (h[i], ids[i, j], r[i]) -- answer j of query i -- so every path runs from
        h[i] to the answer.  The answers come from the same captured step as tails; the explanations run `chunk` triples a
        forward / backward / beam search.
        compact=True: a delta that holds edits is folded into the graph first (compact()), and the explanations walk the
        graph's own edge list.  compact=False: the delta stays a delta -- the answers come from the live step as
        tails' do, the explanations are computed on (base graph, delta) and are DEFINED as those of the same call on
        materialized(): no host plan, no relation-graph rebuild, no new capture.  The explanation path was never order-pinned
        (the re-associating plan and autograd), so the edge gradients of this route equal those of the
        materialised route up to fp32 re-association, not bit for bit; given the gradients the beam search is exact.  Paths
        whose weights differ by less than that may come in another order.  ValueError on a model the route does not serve
        (explain_live_supported: sum / DistMult / fp32 entity layers); an unedited delta is compact=True."""
        return self._explain(h, r, "tail", chunk, compact, among)

    def explain_heads(self, t, r, chunk=16, compact=True, among=None):
        """heads(t, r) plus why.  The model scores (?, r, t) as the TAIL query (t, r + num_direct_rel, ?) -- the inverse
        relation, as in evaluation -- so the triple explained for answer a is (t[i], a, r[i] + num_direct_rel), the one whose
        score was served: every path runs from t[i] to the answer over the graph's edges, inverse ones included.  `compact` as
        in explain_tails."""
        return self._explain(t, r, "head", chunk, compact, among)

    def _explain(self, anchor, relation, mode, chunk, compact=True, among=None):
        if not hasattr(self.model, "visualize_batch"):
            raise TypeError("%s cannot explain its answers: models.Ultra and models.EntityNBFNet (visualize_batch) can"
                            % type(self.model).__name__)
        if not isinstance(compact, bool):
            raise ValueError("compact must be True or False, got %r" % (compact,))
        if not compact:
            blocker = explain_live_blocker(self.model)
            if blocker is not None:
                raise ValueError("compact=False: explanations on a graph delta are not served by %s" % blocker)
        live = {}
        if self.delta is not None and self.delta.edited:
            if compact:
                self.compact()      # (explanations walk the graph's own edge list: the edits become part of it first)
            else:
                live = {"delta": self.delta}
        anchor, relation = self._query(anchor, relation)
        ids, scores, count = self._run(anchor, relation, mode) if among is None else self._run(anchor, relation, mode, among)
        dev = ids.device
        if mode == "head":
            relation = relation + self.data.num_relations // 2
        counts = count.tolist()
        rows = torch.tensor([i for i, c in enumerate(counts) for _ in range(c)], dtype=torch.long, device=dev)
        cols = torch.tensor([j for c in counts for j in range(c)], dtype=torch.long, device=dev)
        triples = torch.stack([anchor[rows], ids[rows, cols], relation[rows]], dim=-1)
        flat = self.model.visualize_batch(self.data, triples, chunk=chunk, **live) if len(rows) else []
        slots, live = self.num_relation_slots, self.num_direct_relations
        if slots != live:       # (the caller sees the compact numbering of materialized(): inverse type r + live)
            flat = [(type(paths)([(h, t, r - (slots - live) if r >= slots else r) for h, t, r in path] for path in paths), weights)
                    for paths, weights in flat]
        explanations, at = [], 0
        for c in counts:
            explanations.append(flat[at:at + c])
            at += c
        return ids, scores, count, explanations

    def verify_tails(self, h, r, t, among=None):
        """How plausible is each STATED fact (h[i], r[i], t[i]) given the rest of the graph?  Scoring a triple that is an edge of
        the graph says nothing -- its own edge is a one-hop path from h to t -- so fact i is scored on the graph WITHOUT itself
        and its inverse (with the model's `remove_one_hop`: without any edge between the two nodes), while it still sees every
        other fact of the batch: a leave-one-out view per sample, as per-sample keep masks over the cached plan of the full
        graph (the relation graph is not rebuilt, as in the reference's training-time removal).  On a live graph "the graph" is
        the materialised one -- added facts in, retracted ones out -- and the delta stays a delta.  Returns (score (n) fp32: the
        logit of t[i] as the tail of (h[i], r[i], ?); rank (n) int64: 1 + the candidates outside the filter graph's known tails
        of (h[i], r[i]) that score at least as high; num_negative (n) int64: how many such candidates there are).  r must be
        direct relations (ValueError).  On the GPU with use_graph each batch is one hipGraph replay; predict.verify_reference
        is the plain-torch restatement.  among (as in `tails`): the type-constrained filtered rank -- rank and num_negative
        count only the candidates of fact i's set (ultra_filtered_rank_among); t[i] itself need not be in it."""
        return self._verify(h, r, t, "tail", among)

    def verify_heads(self, h, r, t, among=None):
        """verify_tails for h[i] as the head of (?, r[i], t[i]): scored as the tail query (t[i], r[i] + num_direct_rel, ?), exactly
        as evaluation does; the removed edges are the same two."""
        return self._verify(h, r, t, "head", among)

    def close(self):
        """Drop the captured steps (their plans are unpinned)."""
        _release(self._steps)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _query(self, anchor, relation):
        """(anchor, relation) of a query as int64 vectors on the graph's device: one relation per anchor, the anchors entities in
        use -- not in the reserve, not retired --, the relations direct relations in use (ValueError otherwise)."""
        dev = self.data.edge_index.device
        anchor = torch.as_tensor(anchor, dtype=torch.long, device=dev).flatten()
        relation = torch.as_tensor(relation, dtype=torch.long, device=dev).flatten()
        if anchor.shape != relation.shape:
            raise ValueError("one relation per query: got %d entities and %d relations" % (len(anchor), len(relation)))
        self._live.check_entities(anchor, "the anchors of a query")
        if self.relation_capacity:
            check_live_relations(relation, self.num_direct_relations, "the relations of a query")
        return anchor, relation

    def _step(self, key, need, build, among_need=None, route=_delta_route):
        """The captured step `key` of `_steps`, (re)built -- build(capacity) -- when there is none, the weights changed, the known
        lists of the call (`need` ids; None: no filter) do not fit its buffer, the delta, its route or the retired pair changed.
        among_need ((ids in all, longest list) of a call with candidate sets; None: none): ... or the call's lists do not fit the
        step's buffer or its longest list its capacity -- build(capacity, (index capacity, list capacity)) then, both doubled."""
        step = self._steps.get(key)
        if step is not None and step.params == param_state(self.model) and (need is None or need <= step.capacity) \
                and step.delta is self.delta and step.route == route(self.delta) and step.retired is self._live.retired_operand \
                and (among_need is None or step.among_fits(*among_need)):
            return step
        if step is not None:
            step.release()
            del self._steps[key]
        capacity = None if need is None else max(2 * need, 1 << 16)
        if among_need is None:
            step = self._steps[key] = build(capacity)
        else:       # (a list capacity up to a chunk costs one chunk: no less is reserved)
            step = self._steps[key] = build(capacity, (max(2 * among_need[0], 1 << 16), max(2 * among_need[1], _lib.TOPK_CHUNK)))
        return step

    def _batched(self, key, build, rows, ptr, index, outs, eager, capturable=True, among=None, route=_delta_route, before=None,
                 eager_flag="_eager_only", copy_out=True):
        """The batch loop of tails / heads / verify_*, inside eval_mode: `rows` (the per-query tensors a step takes) in batches of
        batch_size into `outs`.  On the GPU with use_graph each batch is one replay of the captured step `key` (_step): a last
        batch that is short is padded with copies of its last row with no known list, `index` is loaded once, and the step's
        buffers are copied out, the padded rows dropped.  A model outside the fused inference path (models.NotOnFusedPath),
        and every other case: eager(lo) gives the outputs of the batch that starts at row lo.
        among (None, or the call's (span, index, longest) of CandidateSets.assemble): the step -- under a key of its own --
        takes the call's lists once (load_among) and a batch's spans per replay; a padded row gets an empty span.
        route: what the step remembers of the delta (_step); before(step, lo): called ahead of the replay of the batch at lo;
        eager_flag: the attribute that remembers "this route is not capturable here" -- every route owns its own.
        copy_out=False (the best pairs): a step that keeps its result itself -- nothing is copied out of its buffers
        per batch, `outs` only tells the device, and eager(lo) keeps its own result and returns ()."""
        n, bs = len(rows[0]), self.batch_size
        start = 0
        if capturable and self.use_graph and outs[0].is_cuda and not getattr(self, eager_flag):
            try:
                step = self._step(key, None if index is None else index.numel(), build,
                                  None if among is None else (among[1].numel(), among[2]), route=route)
                pad = (-n) % bs
                padded, ptr_p = rows, ptr
                if pad:
                    padded = [torch.cat([t, t[-1:].expand(pad, *t.shape[1:])]) for t in rows]
                    ptr_p = None if ptr is None else torch.cat([ptr, ptr[-1:].expand(pad)])
                if index is not None:
                    step.load_index(index)
                if among is not None:
                    step.load_among(among[1])
                    span_p = torch.cat([among[0], among[0].new_zeros(pad, 2)]) if pad else among[0]
                for lo in range(0, n, bs):
                    if among is not None:
                        step.among_span.copy_(span_p[lo:lo + bs], non_blocking=True)
                    if before is not None:
                        before(step, lo)
                    got = step(*(t[lo:lo + bs] for t in padded), None if ptr_p is None else ptr_p[lo:lo + bs + 1])
                    for out, b_out in zip(outs, got if copy_out else ()):
                        out[lo:lo + bs].copy_(b_out[:min(bs, n - lo)], non_blocking=True)
                start = n
            except models.NotOnFusedPath:       # model outside the fused inference path: everything runs eagerly below
                torch.cuda.synchronize()
                setattr(self, eager_flag, True)
        for lo in range(start, n, bs):
            for out, b_out in zip(outs, eager(lo)):
                out[lo:lo + len(b_out)] = b_out

    @torch.no_grad()
    def _verify(self, h, r, t, mode, among=None):
        h, r, t = _check_facts(self.data, h, r, t, num_live=self.num_entities if self.entity_capacity else None,
                               num_direct=self.num_direct_relations if self.relation_capacity else None,
                               retired=self.retired_entities)
        if self.delta is not None and self.delta.edited and (self.entity_capacity or self.relation_capacity
                                                             or not delta_samples_supported(self.model)):
            # a model without the combined route: the keep masks run over the graph's own edge list.  A graph with reserved rows
            # or relation slots keeps DESIGN.md 19's rule -- compact first, the slot counts and the live counts stay
            self.compact()
        data, bs, delta = self.data, self.batch_size, self.delta
        live = delta is not None and delta.edited      # (the edits stay beside the plan: leave_out= with the delta)
        dev = h.device
        n = len(h)
        outs = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.long, device=dev),
                torch.empty(n, dtype=torch.long, device=dev))       # (score, rank, num_negative)
        if n == 0:
            return outs
        ent = _entity_model(self.model)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        with eval_mode(self.model):
            triples = torch.stack([h, t, r], dim=-1)
            ptr, index = tasks.known_answers(self.filter_graph, triples, mode)      # the known lists of the whole call, once
            ptr, index = ptr.contiguous(), index.contiguous()

            def eager(lo):
                part = triples[lo:lo + bs].contiguous()
                anchor, pos = (part[:, 0], part[:, 1]) if mode == "tail" else (part[:, 1], part[:, 0])
                if live:
                    pred = self.model(data, _candidates(data, anchor, part[:, 2], mode), leave_out=part,
                                      delta=delta).float().contiguous()
                else:
                    keep = ent.leave_one_out_keep(data, part, validate=False)
                    pred = self.model(data, _candidates(data, anchor, part[:, 2], mode), edge_keep=keep).float().contiguous()
                pos = pos.contiguous()
                # the kernel on the GPU; the restatement with the same interface elsewhere, as in `tails`
                rank_of = filtered_rank if pred.is_cuda else filtered_rank_reference
                b_rank, b_neg = rank_of(pred, pos, ptr[lo:lo + len(part) + 1], index, **self._live.selection_for(pred.is_cuda),
                                        **self._among_for(among, lo, len(part), pred.is_cuda))
                return pred.gather(1, pos.unsqueeze(-1)).squeeze(-1), b_rank, b_neg

            self._batched("verify_" + mode if among is None else ("verify_" + mode, "among"),
                          lambda capacity, among_sizes=None: _GraphedVerifyStep(
                              self.model, data, bs, mode, capacity, n_live=self.live_count, delta=delta,
                              retired=self._live.retired_operand, **({} if among_sizes is None else {"among": among_sizes})),
                          (triples,), ptr, index, outs, eager, capturable=bs <= dense.LEAVE_ONE_OUT_MAX_SAMPLES, among=among)
        return outs

    @staticmethod
    def _among_for(among, lo, rows, on_gpu):
        """The among= arguments of one eager batch -- rows [lo, lo + rows) of the call's assembled (span, index, longest) -- for
        the kernels' wrappers (the device pair and the capacity) or for the _reference functions (a list of id vectors)."""
        if among is None:
            return {}
        span, index, longest = among
        part = span[lo:lo + rows].contiguous()
        if on_gpu:
            return {"among": (part, index), "among_capacity": max(1, longest)}
        return {"among": span_rows(part, index)}

    # ---- what-if queries ----
    def _assumed(self, assuming, n):
        """`assuming` of a call with n queries: None where nothing is assumed (the plain route), else _assumed_lists under the
        rules of add_facts and the capacity."""
        if assuming is None:
            return None
        assumed = _assumed_lists(self.data, assuming, n, per_query=self.assume_capacity,
                                 num_live=self.num_entities if self.entity_capacity else None,
                                 num_direct=self.num_direct_relations if self.relation_capacity else None,
                                 retired=self.retired_entities)
        return assumed if any(len(facts) for facts in assumed) else None

    def _assume_served(self):
        """Does the engine route answer what-if queries here: a model in assume_supported, a delta to lay the overlay over, the GPU?"""
        return (not self._assume_eager_only and self.delta is not None and self.data.edge_index.is_cuda
                and assume_supported(self.model))

    def _assume_scores(self, assumed, anchor, relation, mode, lo):
        """The (rows, N) fp32 scores of the what-if batch that starts at query lo, eagerly: one forward over the overlay where
        the engine serves it, else query by query on a copy of the materialised served graph with the query's facts appended
        (assume_reference's loop)."""
        data, bs = self.data, self.batch_size
        part = assumed[lo:lo + bs]
        if self._assume_served():
            if self._assume_overlay is None or self._assume_overlay[0] is not self.delta:
                self._assume_overlay = (self.delta, rspmm.AssumedFacts(data, self.delta, bs, self.assume_capacity))
            overlay = self._assume_overlay[1]
            overlay.fill(part + [None] * (bs - len(part)))
            try:
                return self.model(data, _candidates(data, anchor[lo:lo + bs], relation[lo:lo + bs], mode), delta=overlay).float()
            except models.NotOnFusedPath:       # (a plan or a shape the owned entry does not serve)
                self._assume_eager_only = True
        full = self._live._probe().materialize(data)
        rows = []
        for i, facts in enumerate(part):
            graph = _assumed_graph(full, facts)
            rows.append(self.model(graph, _candidates(graph, anchor[lo + i:lo + i + 1], relation[lo + i:lo + i + 1], mode)).float())
        return torch.cat(rows)

    @torch.no_grad()
    def _run_above(self, anchor, relation, min_score, mode, among=None, assuming=None):
        threshold = _fp32_threshold(min_score)
        data, bs, live, model_kwargs = self.data, self.batch_size, self._live, self._model_kwargs()
        dev = data.edge_index.device
        anchor, relation = self._query(anchor, relation)
        n = len(anchor)
        assumed = self._assumed(assuming, n)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        out_ptr, ids, scores, size = [torch.zeros(1, dtype=torch.long, device=dev)], [], [], []
        with eval_mode(self.model):
            ptr = index = None
            if self.filtered and n:     # the known lists of the whole call, once
                extra = None if assumed is None else _assumed_known(assumed, anchor, relation, mode)
                ptr, index = known_answers(self.filter_graph, anchor, relation, mode, extra=extra)
            at = 0
            for lo in range(0, n, bs):
                if assumed is not None:
                    pred = self._assume_scores(assumed, anchor, relation, mode, lo)
                else:
                    pred = self.model(data, _candidates(data, anchor[lo:lo + bs], relation[lo:lo + bs], mode),
                                      **model_kwargs).float()
                b_ptr = None if ptr is None else ptr[lo:lo + len(pred) + 1]
                if pred.is_cuda:
                    b_out, b_ids, b_scores, b_size = filtered_above(pred, threshold, b_ptr, index, **live.selection_for(pred.is_cuda),
                                                                    **self._among_for(among, lo, len(pred), True))
                    total = int(b_out[-1])      # (the one host read of the batch)
                    b_ids, b_scores = b_ids[:total].clone(), b_scores[:total].clone()
                else:
                    b_out, b_ids, b_scores, b_size = filtered_above_reference(pred, threshold, b_ptr, index,
                                                                              **live.selection_for(pred.is_cuda),
                                                                              **self._among_for(among, lo, len(pred), False))
                    total = b_ids.numel()
                out_ptr.append(b_out[1:] + at)
                ids.append(b_ids)
                scores.append(b_scores)
                size.append(b_size)
                at += total
        if not ids:
            return (out_ptr[0], torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                    torch.zeros(0, dtype=torch.long, device=dev))
        return torch.cat(out_ptr), torch.cat(ids), torch.cat(scores), torch.cat(size)

    @torch.no_grad()
    def _run_assume(self, anchor, relation, mode, among, assumed):
        """_run for a call in which some query assumes facts (`assumed`: _assumed's list): the captured step (mode, "assume") --
        its overlay refilled ahead of every replay -- or, where that does not apply, _assume_scores batch by batch."""
        data, bs, k, live = self.data, self.batch_size, self.k, self._live
        dev = data.edge_index.device
        n = len(anchor)
        outs = (torch.empty(n, k, dtype=torch.long, device=dev), torch.empty(n, k, dtype=torch.float32, device=dev),
                torch.empty(n, dtype=torch.long, device=dev))       # (ids, scores, count)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        with eval_mode(self.model):
            ptr = index = None
            if self.filtered:       # the known lists of the whole call, once: every query's own assumed answers among them
                ptr, index = known_answers(self.filter_graph, anchor, relation, mode,
                                           extra=_assumed_known(assumed, anchor, relation, mode))

            def eager(lo):
                pred = self._assume_scores(assumed, anchor, relation, mode, lo)
                select = filtered_topk if pred.is_cuda else filtered_topk_reference
                return select(pred, k, None if ptr is None else ptr[lo:lo + len(pred) + 1], index, **live.selection_for(pred.is_cuda),
                              **self._among_for(among, lo, len(pred), pred.is_cuda))

            def refill(step, lo):
                part = assumed[lo:lo + bs]
                step.overlay.fill(part + [None] * (bs - len(part)))

            self._batched((mode, "assume") if among is None else (mode, "assume", "among"),
                          lambda capacity, among_sizes=None: _GraphedAssumeStep(
                              self.model, data, bs, k, mode, capacity, self.assume_capacity, delta=self.delta,
                              n_live=self.live_count, retired=self._live.retired_operand,
                              **({} if among_sizes is None else {"among": among_sizes})),
                          (anchor, relation), ptr, index, outs, eager, capturable=self._assume_served(), among=among,
                          route=_assume_route, before=refill, eager_flag="_assume_eager_only")
        return outs

    @torch.no_grad()
    def _run(self, anchor, relation, mode, among=None, assuming=None):
        """tails / heads of the queries (anchor, relation) as _query gives them; among, assuming: as the caller gave them."""
        data, bs, k, live, model_kwargs = self.data, self.batch_size, self.k, self._live, self._model_kwargs()
        dev = data.edge_index.device
        n = len(anchor)
        assumed = self._assumed(assuming, n)
        if assumed is not None:
            return self._run_assume(anchor, relation, mode, among, assumed)
        outs = (torch.empty(n, k, dtype=torch.long, device=dev), torch.empty(n, k, dtype=torch.float32, device=dev),
                torch.empty(n, dtype=torch.long, device=dev))       # (ids, scores, count)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        if n == 0:
            return outs
        with eval_mode(self.model):
            ptr = index = None
            if self.filtered:       # the known lists of the whole call, once
                ptr, index = known_answers(self.filter_graph, anchor, relation, mode)

            def eager(lo):
                pred = self.model(data, _candidates(data, anchor[lo:lo + bs], relation[lo:lo + bs], mode), **model_kwargs).float()
                # the fused kernel on the GPU; the restatement with the same interface elsewhere (as eval._local_rows does)
                select = filtered_topk if pred.is_cuda else filtered_topk_reference
                return select(pred, k, None if ptr is None else ptr[lo:lo + len(pred) + 1], index, **live.selection_for(pred.is_cuda),
                              **self._among_for(among, lo, len(pred), pred.is_cuda))

            self._batched(mode if among is None else (mode, "among"), lambda capacity, among_sizes=None: _GraphedPredictStep(
                self.model, data, bs, k, mode, capacity, delta=self.delta, n_live=self.live_count, retired=self._live.retired_operand,
                **({} if among_sizes is None else {"among": among_sizes})),
                (anchor, relation), ptr, index, outs, eager, among=among)
        return outs
