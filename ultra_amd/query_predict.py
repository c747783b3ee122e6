"""Serving complex logical queries: the k best answers of every query, leaving out what the graph already entails.

    qp = QueryPredictor(model, graph, k=10, batch_size=16)
    ids, scores, count = qp.answers(queries)       # (n, k) int64, (n, k) fp32, (n) int64
    ptr, ids, scores, size = qp.answer_sets(queries, probability=0.5)      # every answer above the threshold

`queries`: BetaE nested tuples (`Query.from_nested`) or (n, L) postfix rows.  The queries are grouped by the structure of
their programs (`Program.signature()`), in input order within a group, and every group is cut into batches of at most
`batch_size`; nothing is padded.  Every batch runs through the compiled executor (query_exec.execute); the answers are
selected by ultra_filtered_topk on the logits.  With filtered=True the entities whose final symbolic set is non-zero -- the
answers the graph already entails, from the symbolic traversal of the same run -- are left out: ultra_nonzero_lists turns the
sets into the kernel's lists on the device.  Order, count and padding are those of predict.filtered_topk.
"""
import torch

from . import predict, query_exec
from .ultraquery import Query, _logic


class QueryPredictor(object):
    """model: an `UltraQuery`; graph: the graph to answer on; logic: overrides model.logic for the calls of this predictor."""

    def __init__(self, model, graph, k=10, batch_size=16, filtered=True, logic=None):
        predict._check_k(k)
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        if logic is not None:
            _logic(logic)
        self.model, self.graph, self.k, self.batch_size = model, graph, k, int(batch_size)
        self.filtered, self.logic = bool(filtered), logic
        self._executor = query_exec.Executor()

    def _rows(self, queries):
        """One postfix row (a list ending with stop) per query."""
        if isinstance(queries, torch.Tensor):
            if queries.dim() != 2:
                raise ValueError("postfix queries come as (n, L) rows, got %s" % (tuple(queries.shape),))
            return queries.as_subclass(torch.Tensor).cpu().tolist()
        return [Query.nested_to_postfix(q) + [Query.stop] if isinstance(q, tuple) else
                torch.as_tensor(q).as_subclass(torch.Tensor).flatten().tolist() for q in queries]

    def _programs(self, queries):
        """[(indices, Program)] of the batches of `answers`."""
        rows = self._rows(queries)
        n, r = self.graph.num_nodes, self.graph.num_relations
        groups = {}
        for i, row in enumerate(rows):
            single = query_exec.compile(torch.tensor([row], dtype=torch.long), n, r)
            groups.setdefault(single.signature(), []).append(i)
        out = []
        for members in groups.values():
            for lo in range(0, len(members), self.batch_size):
                index = members[lo:lo + self.batch_size]
                width = max(len(rows[i]) for i in index)
                batch = torch.tensor([rows[i] + [Query.stop] * (width - len(rows[i])) for i in index], dtype=torch.long)
                out.append((index, query_exec.compile(batch, n, r)))
        return out

    def batches(self, queries):
        """The index lists of the batches `answers` runs, in the order it runs them."""
        return [index for index, _ in self._programs(queries)]

    @torch.no_grad()
    def answers(self, queries):
        dev = self.graph.edge_index.device
        plan = self._programs(queries)
        n, k = sum(len(index) for index, _ in plan), self.k
        ids = torch.empty(n, k, dtype=torch.long, device=dev)
        scores = torch.empty(n, k, dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.long, device=dev)
        was_training, logic = self.model.training, self.model.logic
        self.model.eval()
        if self.logic is not None:
            self.model.logic = self.logic
        try:
            for index, program in plan:
                logits, sym = query_exec.execute(self.model, self.graph, program, symbolic_traversal=self.filtered,
                                                 executor=self._executor)
                ptr = known = None
                if logits.is_cuda:
                    if self.filtered:
                        ptr, known = query_exec.nonzero_lists(sym)
                    got = predict.filtered_topk(logits, k, ptr, known)
                else:
                    if self.filtered:
                        sample, known = (sym != 0).nonzero().t()
                        ptr = torch.searchsorted(sample.contiguous(), torch.arange(len(index) + 1))
                    got = predict.filtered_topk_reference(logits, k, ptr, known)
                where = torch.tensor(index, dtype=torch.long).to(dev, non_blocking=True)
                ids[where], scores[where], count[where] = got
        finally:
            self.model.train(was_training)
            self.model.logic = logic
        return ids, scores, count

    @torch.no_grad()
    def answer_sets(self, queries, probability=0.5):
        """The answer SET of every query, ranked: (ptr (n + 1) int64, ids, scores, size (n) int64) in INPUT order -- the set of
        query i is ids[ptr[i] : ptr[i + 1]], best first.  An entity belongs to the set iff its logit exceeds
        predict.logit_threshold(probability) (predict.filtered_above_reference: the rule is on the logit, so a positive logit
        too small for the reference's fp32 `sigmoid > 0.5` is a member here).  size[i] is the integer predicted cardinality:
        every entity above the threshold, entailed ones included -- not the reference's soft num_pred.  With filtered=True
        the entailed answers are left out of the lists exactly as in `answers`.  The batches are those of `answers`, through
        the same executor call; ultra_filtered_above selects on the device and the host reads one number per batch (the
        batch's total) to slice the batch's lists."""
        threshold = predict.logit_threshold(probability)
        dev = self.graph.edge_index.device
        plan = self._programs(queries)
        n = sum(len(index) for index, _ in plan)
        length = torch.zeros(n, dtype=torch.long, device=dev)
        size = torch.zeros(n, dtype=torch.long, device=dev)
        done = []
        was_training, logic = self.model.training, self.model.logic
        self.model.eval()
        if self.logic is not None:
            self.model.logic = self.logic
        try:
            for index, program in plan:
                logits, sym = query_exec.execute(self.model, self.graph, program, symbolic_traversal=self.filtered,
                                                 executor=self._executor)
                ptr = known = None
                if logits.is_cuda:
                    if self.filtered:
                        ptr, known = query_exec.nonzero_lists(sym)
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above(logits, threshold, ptr, known)
                    total = int(b_ptr[-1])      # (the one host read of the batch)
                    b_ids, b_scores = b_ids[:total].clone(), b_scores[:total].clone()
                else:
                    if self.filtered:
                        sample, known = (sym != 0).nonzero().t()
                        ptr = torch.searchsorted(sample.contiguous(), torch.arange(len(index) + 1))
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above_reference(logits, threshold, ptr, known)
                where = torch.tensor(index, dtype=torch.long).to(dev, non_blocking=True)
                length[where], size[where] = b_ptr[1:] - b_ptr[:-1], b_size
                done.append((where, b_ptr, b_ids, b_scores))
        finally:
            self.model.train(was_training)
            self.model.logic = logic
        # the lists of every batch, moved to where the input order puts them
        out_ptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
        out_ptr[1:] = length.cumsum(0)
        total = sum(b_ids.numel() for _, _, b_ids, _ in done)
        ids = torch.empty(total, dtype=torch.long, device=dev)
        scores = torch.empty(total, dtype=torch.float32, device=dev)
        for where, b_ptr, b_ids, b_scores in done:
            rows = torch.repeat_interleave(torch.arange(len(where), device=dev), b_ptr[1:] - b_ptr[:-1], output_size=b_ids.numel())
            to = out_ptr[where][rows] + (torch.arange(b_ids.numel(), device=dev) - b_ptr[rows])
            ids[to], scores[to] = b_ids, b_scores
        return out_ptr, ids, scores, size
