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

A CHANGING graph: `add_facts` / `remove_facts` hold the edits in an rspmm.GraphDelta beside the served graph --
no new relation-graph plan, host plan or traversal CSR -- and every answer equals a fresh QueryPredictor's on `materialized()`.

A GROWING graph: QueryPredictor(entity_capacity=M) reserves M rows for entities that arrive later
(`add_entities`), as predict.Predictor does (§19).  The final symbolic sets are then listed over the LIVE ids
(ultra_nonzero_lists_live: after a negation every reserved slot holds 1.0) and the selection runs over them
(ultra_filtered_topk_live / ultra_filtered_above_live).
"""
import copy

import torch

from . import predict, query_exec, rspmm, tasks
from .ultraquery import Query, _logic


class QueryPredictor(object):
    """model: an `UltraQuery`; graph: the graph to answer on; logic: overrides model.logic for the calls of this predictor;
    delta_capacity: the edits (added facts + retracted facts) held beside the served graph before they are folded into it.

    entity_capacity=M > 0 (the interface of predict.Predictor, §19): the graph served is a shallow copy of `graph`
    with num_nodes = N + M SLOTS (the same edge list; its own relation graph, equal to the unpadded one), `num_entities` of them
    live.  add_entities(count) hands out the next ids and does nothing else; the live count also lives in one device int64
    (`live_count`, the same tensor for the predictor's life) that the list and selection kernels read.  The new ids are heads,
    tails and anchors from then on; an id in [num_entities, slots) is a ValueError everywhere and never an answer.  Every result
    is that of a fresh QueryPredictor(entity_capacity=0) on `materialized()`.  entity_capacity=0 (the default): `graph` itself is
    served, by exactly the entry points of before, and add_entities raises."""

    def __init__(self, model, graph, k=10, batch_size=16, filtered=True, logic=None, delta_capacity=256, entity_capacity=0):
        predict._check_k(k)
        if isinstance(entity_capacity, bool) or not isinstance(entity_capacity, int) or entity_capacity < 0:
            raise ValueError("entity_capacity must be a non-negative int (reserved rows), got %r" % (entity_capacity,))
        if isinstance(delta_capacity, bool) or not isinstance(delta_capacity, int) or delta_capacity < 1:
            raise ValueError("delta_capacity must be a positive int (facts), got %r" % (delta_capacity,))
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        if logic is not None:
            _logic(logic)
        self.entity_capacity = entity_capacity
        self.num_entities = int(graph.num_nodes)
        self.live_count = None
        if entity_capacity:
            graph = predict._with_slots(graph, self.num_entities + entity_capacity, relation_graph=True)
            self.live_count = torch.full((1,), self.num_entities, dtype=torch.long, device=graph.edge_index.device)
        self.model, self.graph, self.k, self.batch_size = model, graph, k, int(batch_size)
        self.filtered, self.logic = bool(filtered), logic
        self._executor = query_exec.Executor()
        self.delta_capacity = delta_capacity
        self.delta = None       # made at the first edit: a predictor that was never edited runs exactly what it ran before

    # ---- the live graph (the rules of Predictor.add_facts / remove_facts; there is no separate filter graph: the entailed
    # answers come from the symbolic traversal of the same run) ----
    def _new_delta(self, capacity=None):
        capacity = self.delta_capacity if capacity is None else capacity
        if not self.entity_capacity:
            return rspmm.GraphDelta(self.graph, capacity)
        return rspmm.GraphDelta(self.graph, capacity, num_live=self.num_entities)

    # ---- the growing graph (the rules of Predictor.add_entities) ----
    @property
    def num_slots(self):
        """The rows of the served graph: num_entities live ones and the rest of the reserve."""
        return int(self.graph.num_nodes)

    def add_entities(self, count=1):
        """`count` new entities: returns their ids [num_entities, num_entities + count) (int64, on the graph's device) and raises
        the live count -- the host int, the device scalar the kernels read and the delta's bound.  Nothing else happens: no plan,
        no relation graph, no traversal CSR (an entity without facts plays no role); it is a candidate of every query from now
        on, scored as an isolated node, and add_facts / remove_facts / the anchors of a query take its id.  Beyond the reserve
        the graph is compacted and num_entities + count + entity_capacity slots are laid out: one rebuild.  ValueError on a
        predictor without a reserve (entity_capacity=0)."""
        if not self.entity_capacity:
            raise ValueError("this QueryPredictor reserves no rows: create it with entity_capacity > 0 to add entities")
        if isinstance(count, bool) or not isinstance(count, int) or count < 1:
            raise ValueError("count must be a positive int, got %r" % (count,))
        first = self.num_entities
        if first + count > self.num_slots:
            self.compact(slots=first + count + self.entity_capacity)
        self.num_entities = first + count
        self.live_count.fill_(self.num_entities)
        if self.delta is not None:
            self.delta.num_live = self.num_entities
        return torch.arange(first, first + count, dtype=torch.long, device=self.graph.edge_index.device)

    def _fits(self, n):
        held = 0 if self.delta is None else 2 * len(self.delta) + self.delta.num_removed
        return held + 2 * n <= 2 * self.delta_capacity

    def add_facts(self, h, r, t):
        """State the facts (h[i], r[i], t[i]) -- ints or vectors; r direct relations, h and t existing entities (ValueError
        otherwise).  Each adds the edges (h, t, r) and (t, h, r + num_relations / 2) to the served graph: the projections
        traverse them and the symbolic side entails through them from the next call on.  Returns the number of facts the
        delta holds afterwards (0 after a compaction: more edits than delta_capacity)."""
        probe = self.delta if self.delta is not None else self._new_delta(1)
        h, r, t = probe.check(h, r, t)
        if len(h) == 0:
            return 0 if self.delta is None else len(self.delta)
        if not self._fits(len(h)):
            self.compact(extra=(h, r, t))
            return 0
        if self.delta is None:
            self.delta = self._new_delta()
        self.delta.add(h, r, t)
        return len(self.delta)

    def remove_facts(self, h, r, t):
        """Retract the facts (h[i], r[i], t[i]) -- the argument rules of add_facts -- one after the other: every edge equal to
        (h, t, r) or (t, h, r + num_relations / 2) leaves the served graph (a fact stated nowhere is a no-op).  Returns an
        int64 vector: the number of direct edges each fact took out (GraphDelta.remove).  A call that may not fit compacts
        first; one larger than the whole capacity is applied to a delta of its own and folded at once."""
        probe = self.delta if self.delta is not None else self._new_delta(1)
        h, r, t = probe.check(h, r, t)
        if len(h) == 0:
            return torch.zeros(0, dtype=torch.long, device=h.device)
        if not self._fits(len(h)):
            self.compact()
        if self._fits(len(h)):
            if self.delta is None:
                self.delta = self._new_delta()
            return self.delta.remove(h, r, t)
        fold = self._new_delta(len(h))
        removed = fold.remove(h, r, t)
        self.compact(delta=fold)
        return removed

    def compact(self, extra=None, delta=None, slots=None):
        """Fold the delta's edits (and `extra` = (h, r, t), checked by the caller) into the served graph: the materialised graph
        -- its relation graph rebuilt; a host plan and a traversal CSR on the next query -- becomes `graph`, and the delta is
        emptied.  `delta`: fold that one instead of the predictor's own.  The slot count and the live count of a graph with
        reserved rows stay; `slots` (add_entities beyond the reserve): the new slot count, laid out in the same rebuild."""
        delta = self.delta if delta is None else delta
        facts = [] if delta is None else [delta.facts[:len(delta)]]
        if extra is not None:
            facts.append(torch.stack(list(extra), dim=1))
        facts = torch.cat(facts) if facts else torch.zeros(0, 3, dtype=torch.long)
        if slots is not None and int(slots) == self.num_slots:
            slots = None
        if len(facts) == 0 and not (delta is not None and delta.num_removed) and slots is None:
            return
        fh, fr, ft = facts.unbind(1)
        base = self.graph
        if delta is not None and delta.num_removed:
            base = copy.copy(self.graph)
            base.edge_index, base.edge_type = delta.surviving(self.graph.edge_index, self.graph.edge_type)
        graph = predict._with_facts(base, fh, fr, ft)
        if slots is not None:
            graph.num_nodes = int(slots)
        if getattr(self.graph, "relation_graph", None) is not None:
            tasks.build_relation_graph(graph)
        self.graph = graph
        self.delta = None

    def materialized(self):
        """The graph a fresh QueryPredictor would be given for the same answers: the served edge list with the delta's edits and
        the delta's relation graph (GraphDelta.materialize); the served graph itself where no edit is held.  With a reserve:
        num_nodes = num_entities -- no reserved row -- and a new copy at every call."""
        if self.entity_capacity:
            probe = self.delta if self.delta is not None else self._new_delta(1)
            return copy.copy(probe.materialize(self.graph, num_nodes=self.num_entities))
        if self.delta is None or not self.delta.edited:
            return self.graph
        return self.delta.materialize(self.graph)

    def _delta_kwargs(self):
        return {"delta": self.delta} if self.delta is not None and self.delta.edited else {}

    def _live_kwargs(self, on_gpu):
        """What the lists and the selection take beside today's arguments: nothing without a reserve; with one, the live count --
        the device scalar for the kernels, the host int for the plain-torch restatements."""
        if not self.entity_capacity:
            return {}
        return {"num_live": self.live_count if on_gpu else self.num_entities}

    def _known_reference(self, sym, rows):
        """(ptr, index) of the final symbolic sets in plain torch (the CPU route): the non-zero LIVE ids of every row."""
        if self.entity_capacity:
            sym = sym[:, :self.num_entities]
        sample, known = (sym != 0).nonzero().t()
        return torch.searchsorted(sample.contiguous(), torch.arange(rows + 1)), known

    def _rows(self, queries):
        """One postfix row (a list ending with stop) per query."""
        if isinstance(queries, torch.Tensor):
            if queries.dim() != 2:
                raise ValueError("postfix queries come as (n, L) rows, got %s" % (tuple(queries.shape),))
            return queries.as_subclass(torch.Tensor).cpu().tolist()
        return [Query.nested_to_postfix(q) + [Query.stop] if isinstance(q, tuple) else
                torch.as_tensor(q).as_subclass(torch.Tensor).flatten().tolist() for q in queries]

    def _programs(self, queries):
        """[(indices, Program)] of the batches of `answers`.  With a reserve the programs are compiled against the slot count
        (the served graph's num_nodes) and an anchor in [num_entities, slots) is a ValueError."""
        rows = self._rows(queries)
        n, r = self.graph.num_nodes, self.graph.num_relations
        compile = query_exec.compile
        if self.entity_capacity:
            compile = lambda q, n, r: query_exec.compile(q, n, r, num_live=self.num_entities)
        groups = {}
        for i, row in enumerate(rows):
            single = compile(torch.tensor([row], dtype=torch.long), n, r)
            groups.setdefault(single.signature(), []).append(i)
        out = []
        for members in groups.values():
            for lo in range(0, len(members), self.batch_size):
                index = members[lo:lo + self.batch_size]
                width = max(len(rows[i]) for i in index)
                batch = torch.tensor([rows[i] + [Query.stop] * (width - len(rows[i])) for i in index], dtype=torch.long)
                out.append((index, compile(batch, n, r)))
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
                                                 executor=self._executor, **self._delta_kwargs())
                ptr = known = None
                live = self._live_kwargs(logits.is_cuda)
                if logits.is_cuda:
                    if self.filtered:
                        ptr, known = query_exec.nonzero_lists(sym, **live)
                    got = predict.filtered_topk(logits, k, ptr, known, **live)
                else:
                    if self.filtered:
                        ptr, known = self._known_reference(sym, len(index))
                    got = predict.filtered_topk_reference(logits, k, ptr, known, **live)
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
                                                 executor=self._executor, **self._delta_kwargs())
                ptr = known = None
                live = self._live_kwargs(logits.is_cuda)
                if logits.is_cuda:
                    if self.filtered:
                        ptr, known = query_exec.nonzero_lists(sym, **live)
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above(logits, threshold, ptr, known, **live)
                    total = int(b_ptr[-1])      # (the one host read of the batch)
                    b_ids, b_scores = b_ids[:total].clone(), b_scores[:total].clone()
                else:
                    if self.filtered:
                        ptr, known = self._known_reference(sym, len(index))
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above_reference(logits, threshold, ptr, known, **live)
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
