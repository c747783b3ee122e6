"""Answer ranking and metrics of complex logical queries (reference: ultra/query_utils.py:238-426, script/run_query.py).

batch_evaluate ranks every answer of every query among all entities.  On the GPU that is one call of
ultra_answer_ranking (csrc/query_kernels.hip): one read of the predictions, integer counts, no full sort.  CPU tensors take
batch_evaluate_reference, the torch restatement.  The order is the stable descending one: u is ahead of v iff p_u > p_v,
or p_u == p_v and u < v.  The reference sorts with an unstable argsort, so on tied scores its ranks
follow whatever that sort returns.
"""

import torch

from . import _lib
from . import distributed as udist
from ._lib import check, lib, ptr, stream_of


def _answer_lists(easy_answer, hard_answer):
    """Per query its easy answers by ascending id, then its hard ones: (entity ids, query of each, sizes)."""
    if easy_answer.shape != hard_answer.shape or easy_answer.dim() != 2:
        raise ValueError("easy_answer and hard_answer must both be (batch, num_nodes) masks")
    easy_answer, hard_answer = easy_answer.bool(), hard_answer.bool()
    if bool((easy_answer & hard_answer).any()):
        raise ValueError("an entity is both an easy and a hard answer of one query: the answer sets must be disjoint")
    num_entity = easy_answer.shape[1]
    sample, col = torch.cat([easy_answer, hard_answer], dim=-1).nonzero().t()
    return col % num_entity, sample, easy_answer.sum(-1), hard_answer.sum(-1)


def _keep_mask(limit_nodes, num_entity, device):
    if limit_nodes is None:
        return None
    keep = torch.zeros(num_entity, dtype=torch.bool, device=device)
    keep[limit_nodes.to(device)] = True
    return keep


def batch_evaluate(pred, target, limit_nodes=None):
    """query_utils.py:284-325.  pred (batch, num_nodes) logits; target (type, easy_answer, hard_answer); limit_nodes: the
    only nodes that may rank (every other node scores -inf).  Returns (ranking, answer_ranking): the filtered 1-based rank
    of every hard answer, and the 0-based unfiltered position of every answer (per query its easy answers by ascending
    id, then its hard ones).  pred is not modified."""
    if not pred.is_cuda:
        return batch_evaluate_reference(pred, target, limit_nodes)
    _, easy_answer, hard_answer = target
    if pred.dtype != torch.float32 or pred.dim() != 2:
        raise TypeError("batch_evaluate takes (batch, num_nodes) fp32 logits, got %s %s" % (pred.dtype, tuple(pred.shape)))
    if easy_answer.shape != pred.shape:
        raise ValueError("answer masks %s do not match pred %s" % (tuple(easy_answer.shape), tuple(pred.shape)))
    batch, num_entity = pred.shape
    dev = pred.device
    ent, _, num_easy, num_hard = _answer_lists(easy_answer.to(dev), hard_answer.to(dev))
    num_answer = num_easy + num_hard
    ans_ptr = torch.zeros(batch + 1, dtype=torch.int64, device=dev)
    torch.cumsum(num_answer, 0, out=ans_ptr[1:])
    hard_ptr = torch.cumsum(num_hard, 0) - num_hard
    # queries whose answers, padded to a power of two P, do not fit in LDS work in a global workspace of 4 P words each
    counts = num_answer.tolist()
    padded = [1 << (a - 1).bit_length() if a > 0 else 0 for a in counts]
    words = [4 * p if p > _lib.RANKING_LDS_ANSWERS else 0 for p in padded]
    offsets = [0]
    for w in words[:-1]:
        offsets.append(offsets[-1] + w)
    ws_off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    ws_words, total_answer, total_hard = sum(words), sum(counts), int(num_hard.sum())
    ws = torch.empty(max(ws_words, 1), dtype=torch.int32, device=dev)
    keep = _keep_mask(limit_nodes, num_entity, dev)
    keep_u8 = keep.to(torch.uint8) if keep is not None else None
    answer_ranking = torch.empty(total_answer, dtype=torch.int64, device=dev)
    ranking = torch.empty(total_hard, dtype=torch.int64, device=dev)
    pred_c = pred.contiguous()
    ent = ent.contiguous()
    stream = stream_of(dev)
    check(lib.ultra_answer_ranking(pred_c.data_ptr(), ptr(keep_u8), ent.data_ptr(),
                                   ans_ptr.data_ptr(), hard_ptr.data_ptr(), num_easy.data_ptr(), ws_off.data_ptr(),
                                   ws.data_ptr(), batch, num_entity, answer_ranking.data_ptr(), ranking.data_ptr(), stream))
    return ranking, answer_ranking


def batch_evaluate_reference(pred, target, limit_nodes=None):
    """The torch restatement of batch_evaluate with a stable descending sort: positions from argsort, the answers ahead of
    an answer from a sort of the answers' positions."""
    _, easy_answer, hard_answer = target
    batch, num_entity = pred.shape
    ent, sample, num_easy, num_hard = _answer_lists(easy_answer, hard_answer)
    keep = _keep_mask(limit_nodes, num_entity, pred.device)
    if keep is not None:
        pred = pred.masked_fill(~keep, float("-inf"))
    order = pred.argsort(dim=-1, descending=True, stable=True)
    position = torch.empty_like(order)
    position.scatter_(-1, order, torch.arange(num_entity, device=pred.device).expand_as(order))
    answer_ranking = position[sample, ent]
    num_answer = num_easy + num_hard
    start = torch.cumsum(num_answer, 0) - num_answer
    # answers ahead of each answer: its index among the answers of its query sorted by position
    sorted_idx = torch.argsort(sample * num_entity + answer_ranking, stable=True)
    among = torch.empty_like(sorted_idx)
    among[sorted_idx] = torch.arange(len(sorted_idx), device=pred.device) - start[sample[sorted_idx]]
    filtered = answer_ranking - among + 1
    index_in_query = torch.arange(len(sample), device=pred.device) - start[sample]
    is_hard = index_in_query >= num_easy[sample]
    return filtered[is_hard], answer_ranking


def _scatter_mean(x, index, size):
    """torch_scatter.scatter_mean: the mean of every group, 0 for an empty one."""
    total = torch.zeros(size, dtype=x.dtype, device=x.device).index_add_(0, index, x)
    count = torch.zeros(size, dtype=x.dtype, device=x.device).index_add_(0, index, torch.ones_like(x))
    return total / count.clamp(min=1)


def _variadic_mean(x, size):
    return _scatter_mean(x, torch.repeat_interleave(size), len(size))


def _masked_mean(x, mask):
    return torch.where(mask, x, torch.zeros_like(x)).sum() / mask.sum().clamp(1)


def _tie_mean_ranking(x):
    """1-based ranks of x, tied values sharing the mean of their ranks."""
    values, inverse = x.unique(return_inverse=True)
    order = inverse.argsort(stable=True)
    ranking = torch.zeros(len(x), dtype=torch.float, device=x.device)
    ranking[order] = torch.arange(1, len(x) + 1, dtype=torch.float, device=x.device)
    return _scatter_mean(ranking, inverse, len(values))[inverse]


def spearmanr(pred, target):
    """query_utils.py:400-426."""
    pred, target = _tie_mean_ranking(pred), _tie_mean_ranking(target)
    covariance = (pred * target).mean() - pred.mean() * target.mean()
    return covariance / (pred.std(unbiased=False) * target.std(unbiased=False) + 1e-10)


def variadic_area_under_roc(answer_ranking, is_hard, size):
    """query_utils.py:376-397: per query, the fraction of (easy, hard) answer pairs whose hard answer is ranked behind the
    easy one."""
    query = torch.repeat_interleave(size)
    num_entity = int(answer_ranking.max()) + 1 if answer_ranking.numel() else 1
    order = torch.argsort(query * num_entity + (num_entity - 1 - answer_ranking), stable=True)  # worst answer first
    target = is_hard[order].float()
    hard_before = torch.cumsum(target, 0) - target
    offset = torch.zeros(len(size) + 1, dtype=target.dtype, device=target.device)
    offset[1:] = torch.cumsum(torch.zeros(len(size), dtype=target.dtype, device=target.device).index_add_(0, query, target), 0)
    hit = torch.where(target == 0, hard_before - offset[query], torch.zeros_like(target))
    num_hard = torch.zeros(len(size), device=target.device).index_add_(0, query, target)
    num_easy = size.float() - num_hard
    area = torch.zeros(len(size), device=target.device).index_add_(0, query, hit)
    return area / (num_easy * num_hard + 1e-10)


def evaluate(pred, target, metrics, id2type):
    """query_utils.py:327-374.  pred (ranking, num_pred), target (type, answer_ranking, num_easy, num_hard) as gathered;
    metrics among mrr, hits@k, mape, spearmanr, auroc.  Keys `[type] metric`, `[EPFO] metric`, `[negation] metric`,
    `metric` (the mean over types)."""
    ranking, num_pred = pred
    type, answer_ranking, num_easy, num_hard = target
    num_type = len(id2type)
    metric = {}
    for name in metrics:
        if name == "mrr":
            type_score = _scatter_mean(_variadic_mean(1 / ranking.float(), num_hard), type, num_type)
        elif name.startswith("hits@"):
            threshold = int(name[5:])
            type_score = _scatter_mean(_variadic_mean((ranking <= threshold).float(), num_hard), type, num_type)
        elif name == "mape":
            query_score = (num_pred - num_easy - num_hard).abs() / (num_easy + num_hard).float()
            type_score = _scatter_mean(query_score, type, num_type)
        elif name == "spearmanr":
            type_score = torch.stack([spearmanr(num_pred[type == i], (num_easy + num_hard)[type == i])
                                      for i in range(num_type)])
        elif name == "auroc":
            size = num_easy + num_hard
            index_in_query = torch.arange(len(answer_ranking)) - torch.repeat_interleave(torch.cumsum(size, 0) - size, size)
            is_hard = index_in_query >= torch.repeat_interleave(num_easy, size)
            answer_score = variadic_area_under_roc(answer_ranking, is_hard, size)
            mask = (num_easy > 0) & (num_hard > 0)
            type_score = _scatter_mean(answer_score[mask], type[mask], num_type)
        else:
            raise ValueError("Unknown metric `%s`" % name)
        is_neg = torch.tensor(["n" in t for t in id2type])
        for i, query_type in enumerate(id2type):
            metric["[%s] %s" % (query_type, name)] = type_score[i].item()
        if (~is_neg).any():
            metric["[EPFO] %s" % name] = _masked_mean(type_score, ~is_neg).item()
        if is_neg.any():
            metric["[negation] %s" % name] = _masked_mean(type_score, is_neg).item()
        metric[name] = type_score.mean().item()
    return metric


def predict_and_target(model, graph, batch, batch_evaluate_fn=batch_evaluate, compiled=False):
    """run_query.py:32-52 at inference: the logits of a batch, its ranks and the predicted answer-set sizes
    num_pred = sum(sigmoid(pred) * (sigmoid(pred) > 0.5)), over the restricted logits when the graph restricts nodes.
    compiled: the logits come from the compiled executor (query_exec.forward: the same bits, without the interpreter's host
    synchronisations) instead of model.forward."""
    query, type, easy_answer, hard_answer = batch["query"], batch["type"], batch["easy_answer"], batch["hard_answer"]
    if compiled:
        from . import query_exec
        pred = query_exec.forward(model, graph, query, symbolic_traversal=False)
    else:
        pred = model(graph, query, symbolic_traversal=False)
    restrict_nodes = getattr(graph, "restrict_nodes", None)
    ranking, answer_ranking = batch_evaluate_fn(pred, (type, easy_answer, hard_answer), restrict_nodes)
    keep = _keep_mask(restrict_nodes, pred.shape[-1], pred.device)
    if keep is not None:    # (the reference masks pred in place inside batch_evaluate before it takes num_pred)
        pred = pred.masked_fill(~keep, float("-inf"))
    prob = torch.sigmoid(pred)
    num_pred = (prob * (prob > 0.5)).sum(dim=-1)
    return (ranking, num_pred), (type, answer_ranking, easy_answer.sum(dim=-1), hard_answer.sum(dim=-1))


def gather_results(pred, target):
    """query_utils.py:238-282: every rank's per-query results concatenated in rank order, on the host.  One variable-length
    all-gather per quantity over the process group (ultra_amd.distributed).  As in the reference, which gathers into int64
    buffers at every world size, the predicted answer-set sizes num_pred come back truncated to integers: mape and
    spearmanr are taken on those."""
    (ranking, num_pred), (type, answer_ranking, num_easy, num_hard) = pred, target
    num_pred = num_pred.long()
    parts = [ranking, num_pred, type, answer_ranking, num_easy, num_hard]
    if udist.world_size() > 1:
        parts = [udist.all_gather_variable(p.contiguous()) for p in parts]
    ranking, num_pred, type, answer_ranking, num_easy, num_hard = (p.cpu() for p in parts)
    return (ranking, num_pred), (type, answer_ranking, num_easy, num_hard)


@torch.no_grad()
def test_queries(model, graph, queries, batch_size, id2type, metrics=("mrr", "hits@1", "hits@3", "hits@10", "mape",
                                                                      "spearmanr", "auroc"),
                 device=None, batch_evaluate_fn=batch_evaluate, compiled=False):
    """run_query.py:159-189: score `queries` (a dataset of dicts query / type / easy_answer / hard_answer, e.g.
    query_data.QueryDataset) in batches of `batch_size`, this rank's DistributedSampler shard (shuffled with its default
    seed, as the reference's; where the query count does not divide by the world size it pads with repeated queries, which
    then count twice); gather every rank's results and return the metrics on every rank.  compiled: see predict_and_target."""
    from torch.utils import data as torch_data
    world, rank = udist.world_size(), udist.rank()
    sampler = torch_data.DistributedSampler(queries, world, rank)
    loader = torch_data.DataLoader(queries, batch_size, sampler=sampler)
    if isinstance(model, torch.nn.Module):
        model.eval()
    if device is not None:
        graph = graph.to(device)
    preds, targets = [], []
    for batch in loader:
        if device is not None:
            batch = {k: v.to(device) for k, v in batch.items()}
        p, t = predict_and_target(model, graph, batch, batch_evaluate_fn, compiled=compiled)
        preds.append(p)
        targets.append(t)
    pred = tuple(torch.cat(x) for x in zip(*preds))
    target = tuple(torch.cat(x) for x in zip(*targets))
    pred, target = gather_results(pred, target)
    return evaluate(pred, target, metrics, id2type)
