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

RETIRED entities: `retire_entities` takes entities out of the served graph as predict.Predictor.remove_entities
does (§28) -- their facts retracted, their ids never a candidate, an entailed answer or an anchor again.  From the first
retirement on the lists leave the ids of the device bitmap out (ultra_nonzero_lists_alive: after a negation a retired slot holds
1.0 in the middle of the id range) and the selection runs over the alive ids (ultra_filtered_topk_alive /
ultra_filtered_above_alive).

CANDIDATE sets: `answers(queries, among=)` / `answer_sets(queries, probability, among=)` restrict a query's
candidates to a set -- a name (`define_set`), one id vector for every query, or one name or vector per query, which follows its
query through the grouping into batches.  The entailed lists stay the deny list; the selection gathers the listed logits
(ultra_filtered_topk_among / ultra_filtered_above_among) with the live count and the retired set as its optional operands.

WHAT-IF queries: `answers(queries, assuming=)` / `answer_sets(queries, probability, assuming=)` -- facts a query
ASSUMES for itself (the rules of predict.Predictor.tails(assuming=), §32): query i runs, neural and symbolic projection alike, on
materialized() plus its own direct and inverse edges, so what it entails through a hypothesis is left out for that query alone.
Nothing is stated.  `assume_reference` is the definition.
"""
import contextlib
import functools

import torch

from . import models, predict, query_exec, rspmm
from .candidates import CandidateSets, span_rows
from .live import LiveGraph, forwarded
from .ultraquery import Query, _logic


def _postfix_rows(queries):
    """One postfix row (a list ending with stop) per query."""
    if isinstance(queries, torch.Tensor):
        if queries.dim() != 2:
            raise ValueError("postfix queries come as (n, L) rows, got %s" % (tuple(queries.shape),))
        return queries.as_subclass(torch.Tensor).cpu().tolist()
    return [Query.nested_to_postfix(q) + [Query.stop] if isinstance(q, tuple) else
            torch.as_tensor(q).as_subclass(torch.Tensor).flatten().tolist() for q in queries]


def postfix_batch(queries):
    """`queries` (nested tuples, lists or rows) as one (n, L) int64 batch of postfix rows, padded with stop."""
    rows = _postfix_rows(queries)
    width = max(len(row) for row in rows)
    return torch.tensor([row + [Query.stop] * (width - len(row)) for row in rows], dtype=torch.long)


def _entailed(sym, num_live=None, retired=None):
    """(ptr (rows + 1), ids) of the final symbolic sets `sym` in plain torch: per row the non-zero ids below num_live that are not
    retired (after a negation a reserved or a retired slot holds 1.0)."""
    if num_live is not None:
        sym = sym[:, :int(num_live)]
    listed = sym != 0
    if retired is not None and len(retired):
        retired = torch.as_tensor(retired, dtype=torch.long, device=sym.device).flatten()
        listed[:, retired[retired < sym.shape[1]]] = False
    sample, known = listed.nonzero().t()
    return torch.searchsorted(sample.contiguous(), torch.arange(sym.shape[0] + 1, device=sym.device)), known


def assume_supported(model):
    """Does the engine route answer what-if logical queries for `model` (an UltraQuery): predict.assume_supported of the Ultra
    its projection holds -- sum / max / min with TransE / DistMult?"""
    return predict.assume_supported(getattr(getattr(model, "model", None), "model", None))


@torch.no_grad()
def assume_reference(model, graph, queries, assuming, k=10, filtered=True, logic=None, probability=None, num_live=None,
                     retired=None, among=None):
    """What-if logical queries in plain terms, on any device -- the DEFINITION QueryPredictor.answers / answer_sets (assuming=)
    are tested against.  Query i is answered on a COPY of `graph` with its assumed facts appended -- [graph's edges ; its direct
    edges (h, t, r) in the given order ; their inverse edges], duplicates kept, the relation graph kept as it is
    (predict._assumed_graph) -- by query_exec.execute on a batch of that one query: both projections, the neural and the
    symbolic one, run on the copy, so the entailed answers left out (filtered=True: the non-zero ids of the final symbolic set)
    are those the copy entails.  No other query sees the facts; nothing is stated.  The selection is
    predict.filtered_topk_reference, or with `probability` filtered_above_reference at logit_threshold(probability).
    assuming: one (m, 3) tensor of (h, r, t) rows for every query, or a list with one entry per query (rows, None or empty), under
    predict._assumed_lists' rules.  logic: overrides model.logic.  num_live, retired (a sorted id vector): the ids that exist --
    for the anchors, the facts, the entailed lists and the selection.  among: one id vector for every query or a list of one per
    query.  Returns (ids (n, k), scores (n, k), count (n)), or with probability (ptr (n + 1), ids, scores, size (n))."""
    rows = _postfix_rows(queries)
    dev = graph.edge_index.device
    live = {} if num_live is None else {"num_live": int(num_live)}
    if retired is not None:
        retired = torch.as_tensor(retired, dtype=torch.long).flatten()
    assumed = predict._assumed_lists(graph, assuming, len(rows), retired=retired, **live)
    select = dict(live)
    compile_kwargs = dict(live)
    if retired is not None and len(retired):
        select["retired"] = retired.to(dev)
        compile_kwargs["retired"] = frozenset(retired.tolist())
    threshold = None if probability is None else predict.logit_threshold(probability)
    n, r = int(graph.num_nodes), int(graph.num_relations)
    programs = [query_exec.compile(torch.tensor([row], dtype=torch.long), n, r, **compile_kwargs) for row in rows]
    out = []
    was = model.logic
    with predict.eval_mode(model):
        if logic is not None:
            _logic(logic)
            model.logic = logic
        try:
            for i, (program, facts) in enumerate(zip(programs, assumed)):
                logits, sym = query_exec.execute(model, predict._assumed_graph(graph, facts), program, symbolic_traversal=filtered)
                ptr = known = None
                if filtered:
                    ptr, known = _entailed(sym, num_live, select.get("retired"))
                if among is not None:
                    select["among"] = [among[i] if isinstance(among, (list, tuple)) else among]
                if threshold is None:
                    out.append(predict.filtered_topk_reference(logits, k, ptr, known, **select))
                else:
                    out.append(predict.filtered_above_reference(logits, threshold, ptr, known, **select))
        finally:
            model.logic = was
    if threshold is not None:
        return predict._join_above(out, dev)
    if not out:
        return (torch.zeros(0, k, dtype=torch.long, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.long, device=dev))
    return tuple(torch.cat([part[j] for part in out]) for j in range(3))


class QueryPredictor(object):
    """model: an `UltraQuery`; graph: the graph to answer on; logic: overrides model.logic for the calls of this predictor;
    delta_capacity: the edits (added facts + retracted facts) held beside the served graph before they are folded into it.

    entity_capacity=M > 0 (the interface of predict.Predictor, §19): the graph served is a shallow copy of `graph`
    with num_nodes = N + M SLOTS (the same edge list; its own relation graph, equal to the unpadded one), `num_entities` of them
    live.  add_entities(count) hands out the next ids and does nothing else; the live count also lives in one device int64
    (`live_count`, the same tensor for the predictor's life) that the list and selection kernels read.  The new ids are heads,
    tails and anchors from then on; an id in [num_entities, slots) is a ValueError everywhere and never an answer.  Every result
    is that of a fresh QueryPredictor(entity_capacity=0) on `materialized()`.  entity_capacity=0 (the default): `graph` itself is
    served, by exactly the entry points of before, and add_entities raises.

    retire_entities(ids) (LiveGraph.remove_entities, §28): with or without a reserve.  Every result is then that
    of a fresh QueryPredictor on `materialized()` -- which keeps the id space, the retired ids isolated nodes named by its
    `retired_entities` -- with the retired ids taken out of the candidates and of the entailed lists.  A retired slot of an
    intermediate fuzzy or symbolic set is left as the logic leaves it: nothing is zeroed on the way, so every score keeps the
    bits of the fresh predictor's.  Until the first retirement every call reaches exactly the entries it reached before.  (The
    method is not called remove_entities: see DESIGN.md §29, "The name".)

    assume_capacity: the facts one query may assume (`answers(assuming=)`)."""

    def __init__(self, model, graph, k=10, batch_size=16, filtered=True, logic=None, delta_capacity=256, entity_capacity=0,
                 assume_capacity=8):
        predict.check_k(k)
        if isinstance(assume_capacity, bool) or not isinstance(assume_capacity, int) or assume_capacity < 1:
            raise ValueError("assume_capacity must be a positive int (facts one query may assume), got %r" % (assume_capacity,))
        self.assume_capacity = assume_capacity
        self._assume_loop_only = False      # (an engine route that did not serve this predictor once is not tried again)
        self._assume_overlay = None         # (graph, delta, overlay): the overlay of the what-if batches
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        if logic is not None:
            _logic(logic)
        # (the delta is made at the first edit: a predictor that was never edited runs exactly what it ran before.  There is no
        # filter graph: the entailed answers come from the symbolic traversal of the same run)
        self._live = LiveGraph(graph, delta_capacity, entity_capacity, delta_policy="lazy", owner="QueryPredictor")
        self.model, self.k, self.batch_size = model, k, int(batch_size)
        self.filtered, self.logic = bool(filtered), logic
        self._executor = query_exec.Executor()
        # (ids are stable: the sets outlive compact() and a rebuild.  The registry reads the slot count off the LiveGraph, not
        # off the predictor: no cycle, so __del__ runs with the last reference)
        self._sets = CandidateSets(functools.partial(getattr, self._live, "num_slots"))

    # ---- the state of the served graph: held by the LiveGraph ("The live graph's state in one place") ----
    graph = forwarded("graph")
    delta = forwarded("delta")
    entity_capacity = forwarded("entity_capacity")
    delta_capacity = forwarded("delta_capacity")
    num_entities = forwarded("num_entities")
    num_slots = forwarded("num_slots")
    live_count = forwarded("live_count")
    num_retired = forwarded("num_retired")
    retired_entities = forwarded("retired_entities")

    # ---- candidate sets (the rules of Predictor.define_set) ----
    def define_set(self, name, ids):
        """Name a candidate set for `among=name`: any slots of the graph, sorted and de-duplicated (ValueError outside
        [0, num_slots)); an id in the reserve or a retired one is absent until it is live and alive.  Returns its size."""
        return self._sets.define_set(name, ids)

    def drop_set(self, name):
        self._sets.drop_set(name)

    def sets(self):
        """{name: size} of the candidate sets defined now."""
        return self._sets.sets()

    # ---- the growing graph (the rules of Predictor.add_entities) ----
    def add_entities(self, count=1):
        """`count` new entities: returns their ids [num_entities, num_entities + count) (int64, on the graph's device) and raises
        the live count -- the host int, the device scalar the kernels read and the delta's bound.  Nothing else happens: no plan,
        no relation graph, no traversal CSR (an entity without facts plays no role); it is a candidate of every query from now
        on, scored as an isolated node, and add_facts / remove_facts / the anchors of a query take its id.  Beyond the reserve
        the graph is compacted and num_entities + count + entity_capacity slots are laid out: one rebuild.  ValueError on a
        predictor without a reserve (entity_capacity=0)."""
        return self._live.add_entities(count, compact=self.compact)

    # ---- retiring entities (the rules of Predictor.remove_entities) ----
    def retire_entities(self, ids):
        """Retire the entities `ids` -- an int or a vector of distinct ids in use, none retired before (ValueError otherwise, and
        nothing is changed): every fact that names one as head or tail is retracted (remove_facts: tombstones, the delta) and
        the ids are never an answer, an entailed answer, a candidate that is counted, an anchor or an argument of an edit again
        (LiveGraph.remove_entities).  Ids are not renumbered and a slot is not handed out again; the set survives compact() and
        a rebuild beyond the reserve.  Returns an int64 vector: per id the number of distinct facts retracted."""
        return self._live.remove_entities(ids)

    # ---- the live graph (the rules of Predictor.add_facts / remove_facts) ----
    def add_facts(self, h, r, t):
        """State the facts (h[i], r[i], t[i]) -- ints or vectors; r direct relations, h and t existing entities (ValueError
        otherwise).  Each adds the edges (h, t, r) and (t, h, r + num_relations / 2) to the served graph: the projections
        traverse them and the symbolic side entails through them from the next call on.  Returns the number of facts the
        delta holds afterwards (0 after a compaction: more edits than delta_capacity)."""
        return self._live.add_facts(h, r, t)

    def remove_facts(self, h, r, t):
        """Retract the facts (h[i], r[i], t[i]) -- the argument rules of add_facts -- one after the other: every edge equal to
        (h, t, r) or (t, h, r + num_relations / 2) leaves the served graph (a fact stated nowhere is a no-op).  Returns an
        int64 vector: the number of direct edges each fact took out (GraphDelta.remove).  A call that may not fit compacts
        first; one larger than the whole capacity is applied to a delta of its own and folded at once."""
        return self._live.remove_facts(h, r, t)

    def compact(self, extra=None, delta=None, slots=None):
        """Fold the delta's edits (and `extra` = (h, r, t), checked by the caller) into the served graph: the materialised graph
        -- its relation graph rebuilt; a host plan and a traversal CSR on the next query -- becomes `graph`, and the delta is
        emptied.  `delta`: fold that one instead of the predictor's own.  The slot count and the live count of a graph with
        reserved rows stay; `slots` (add_entities beyond the reserve): the new slot count, laid out in the same rebuild."""
        self._live.compact(extra, delta, slots)

    def materialized(self):
        """The graph a fresh QueryPredictor would be given for the same answers: the served edge list with the delta's edits and
        the delta's relation graph (GraphDelta.materialize); the served graph itself where no edit is held.  With a reserve:
        num_nodes = num_entities -- no reserved row -- and a new copy at every call.  Once an entity was retired, with a reserve
        or without: LiveGraph.materialized() too -- the copy keeps the id space and names `retired_entities`."""
        if self.entity_capacity or self.num_retired:
            return self._live.materialized()
        delta = self.delta
        return self.graph if delta is None or not delta.edited else delta.materialize(self.graph)

    def _delta_kwargs(self):
        delta = self.delta      # (handed over only while it holds edits)
        return {"delta": delta} if delta is not None and delta.edited else {}

    def _known_reference(self, sym, rows):
        """(ptr, index) of the final symbolic sets in plain torch (the CPU route): the non-zero LIVE ids of every row that are
        not retired (after a negation a retired slot holds 1.0)."""
        if self.entity_capacity:
            sym = sym[:, :self.num_entities]
        listed = sym != 0
        if self.num_retired:
            retired = self.retired_entities.to(sym.device)
            listed[:, retired[retired < sym.shape[1]]] = False
        sample, known = listed.nonzero().t()
        return torch.searchsorted(sample.contiguous(), torch.arange(rows + 1)), known

    def _rows(self, queries):
        """One postfix row (a list ending with stop) per query."""
        return _postfix_rows(queries)

    def _programs(self, queries):
        """[(indices, Program)] of the batches of `answers`.  With a reserve the programs are compiled against the slot count
        (the served graph's num_nodes) and an anchor in [num_entities, slots) is a ValueError; a retired anchor is one too."""
        rows = self._rows(queries)
        n, r = self.graph.num_nodes, self.graph.num_relations
        compile = query_exec.compile
        if self.entity_capacity or self.num_retired:
            live = {"num_live": self.num_entities} if self.entity_capacity else {}
            if self.num_retired:
                live["retired"] = frozenset(self.retired_entities.tolist())
            compile = lambda q, n, r: query_exec.compile(q, n, r, **live)
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

    @contextlib.contextmanager
    def _batches(self, plan, among=None, assumed=None):
        """The batches of `plan` (_programs) as answers and answer_sets run them: inside the block the model is in eval mode
        under this predictor's logic (both restored on the way out), and the value is an iterator of (index, logits, ptr, known,
        live) -- the batch's query indices, its logits from the compiled executor, the lists of its entailed answers (None, None
        unless filtered) and the kwargs of the selection: the live count and, once an entity was retired, the retired set
        (LiveGraph.selection_for) -- the lists take the same two.  among (the call's assembled (span, index, longest), or None):
        the kwargs gain the batch's candidate lists -- the spans of its queries, through `index` -- in the form the selection
        of that device takes.  assumed (_assumed's list, or None; the engine route of what-if queries): a batch
        in which a query assumes facts runs with the overlay -- filled for that batch, a short one padded -- as its delta;
        models.NotOnFusedPath where the engine does not serve it."""
        graph, live_graph, delta_kwargs = self.graph, self._live, self._delta_kwargs()

        def run():
            for index, program in plan:
                kwargs = delta_kwargs
                if assumed is not None and any(len(assumed[i]) for i in index):
                    overlay = self._overlay()
                    overlay.fill([assumed[i] for i in index] + [None] * (self.batch_size - len(index)))
                    kwargs = {"delta": overlay}
                logits, sym = query_exec.execute(self.model, graph, program, symbolic_traversal=self.filtered,
                                                 executor=self._executor, **kwargs)
                live = live_graph.selection_for(logits.is_cuda)
                ptr = known = None
                if self.filtered:
                    ptr, known = query_exec.nonzero_lists(sym, **live) if logits.is_cuda else self._known_reference(sym, len(index))
                if among is not None:
                    span, listed, longest = among
                    part = span[torch.tensor(index, dtype=torch.long, device=span.device)].contiguous()
                    if logits.is_cuda:
                        live = dict(live, among=(part, listed), among_capacity=max(1, longest))
                    else:
                        live = dict(live, among=span_rows(part, listed))
                yield index, logits, ptr, known, live

        logic = self.model.logic
        with predict.eval_mode(self.model):
            if self.logic is not None:
                self.model.logic = self.logic
            try:
                yield run()
            finally:
                self.model.logic = logic

    # ---- what-if queries ----
    def _assumed(self, assuming, n):
        """`assuming` of a call with n queries: None where nothing is assumed (the plain route), else predict._assumed_lists under
        the rules of add_facts and the capacity."""
        if assuming is None:
            return None
        assumed = predict._assumed_lists(self.graph, assuming, n, per_query=self.assume_capacity,
                                         num_live=self.num_entities if self.entity_capacity else None,
                                         retired=self.retired_entities if self.num_retired else None)
        return assumed if any(len(facts) for facts in assumed) else None

    def _assume_served(self):
        """Does the engine route answer what-if queries here: a model in assume_supported, on the GPU, not refused before?"""
        return not self._assume_loop_only and query_exec._on_gpu(self.model, self.graph) and assume_supported(self.model)

    def _overlay(self):
        """The overlay of this predictor's what-if batches: one per (served graph, delta object) -- the delta is made at the first
        edit, so a never-edited predictor lays its overlay over no delta."""
        graph, delta = self.graph, self.delta
        hit = self._assume_overlay
        if hit is None or hit[0] is not graph or hit[1] is not delta:
            hit = self._assume_overlay = (graph, delta, rspmm.AssumedFacts(graph, delta, self.batch_size, self.assume_capacity))
        return hit[2]

    def _assume_loop(self, queries, assumed, among, probability=None):
        """The call query by query on copies of materialized() (assume_reference): exact and slow -- a model, a device or a
        program the engine route does not serve."""
        retired = self.retired_entities if self.num_retired else None
        if among is not None:
            among = span_rows(among[0], among[1])
        return assume_reference(self.model, self.materialized(), queries, assumed, k=self.k, filtered=self.filtered,
                                logic=self.logic, probability=probability, retired=retired, among=among)

    def _what_if(self, run, queries, assumed, among, probability=None):
        """`run(assumed)` -- the batches of the call, with the overlay where a query assumes facts -- where the engine serves the
        call, else (remembered per predictor) _assume_loop."""
        if assumed is None:
            return run(None)
        if self._assume_served():
            try:
                return run(assumed)
            except models.NotOnFusedPath:       # (a plan, a shape or a program the owned entries do not serve)
                self._assume_loop_only = True
        return self._assume_loop(queries, assumed, among, probability)

    @torch.no_grad()
    def answers(self, queries, among=None, assuming=None):
        """among (None: every entity): a candidate set per query -- a name, one id vector for all, or one name or vector per
        query, in input order (CandidateSets.resolve) -- count[i] = min(k, its ids that are live, alive and not entailed).
        assuming (None: nothing): facts the queries assume -- one (m, 3) int64 tensor of (h, r, t) rows for every
        query, or a list with one entry per query in input order (rows, None or empty), which follows its query through the
        grouping into batches; the rules of add_facts, at most assume_capacity a query (ValueError, before anything runs).
        Query i is answered on materialized() plus its own direct and inverse edges, the served relation graph kept: both
        projections see them, so an answer the hypothesis entails is left out (filtered=True) for that query alone.  Nothing is
        stated.  Every answer equals assume_reference's.  A call whose assumptions are all empty is the call without them."""
        dev = self.graph.edge_index.device
        plan = self._programs(queries)
        n, k = sum(len(index) for index, _ in plan), self.k
        assumed = self._assumed(assuming, n)
        if among is not None:
            among = self._sets.assemble(among, n, dev)

        def run(assumed):
            ids = torch.empty(n, k, dtype=torch.long, device=dev)
            scores = torch.empty(n, k, dtype=torch.float32, device=dev)
            count = torch.empty(n, dtype=torch.long, device=dev)
            with self._batches(plan, among, assumed) as batches:
                for index, logits, ptr, known, live in batches:
                    select = predict.filtered_topk if logits.is_cuda else predict.filtered_topk_reference
                    got = select(logits, k, ptr, known, **live)
                    where = torch.tensor(index, dtype=torch.long).to(dev, non_blocking=True)
                    ids[where], scores[where], count[where] = got
            return ids, scores, count

        return self._what_if(run, queries, assumed, among)

    @torch.no_grad()
    def answer_sets(self, queries, probability=0.5, among=None, assuming=None):
        """The answer SET of every query, ranked: (ptr (n + 1) int64, ids, scores, size (n) int64) in INPUT order -- the set of
        query i is ids[ptr[i] : ptr[i + 1]], best first.  An entity belongs to the set iff its logit exceeds
        predict.logit_threshold(probability) (predict.filtered_above_reference: the rule is on the logit, so a positive logit
        too small for the reference's fp32 `sigmoid > 0.5` is a member here).  size[i] is the integer predicted cardinality:
        every entity above the threshold, entailed ones included -- not the reference's soft num_pred.  With filtered=True
        the entailed answers are left out of the lists exactly as in `answers`.  The batches are those of `answers`, through
        the same executor call; ultra_filtered_above selects on the device and the host reads one number per batch (the
        batch's total) to slice the batch's lists.  among: as in `answers` -- only the set's ids can be members, in the lists
        and in size.  assuming: as in `answers` -- the sets of the what-if queries, assume_reference(probability=)'s."""
        threshold = predict.logit_threshold(probability)
        dev = self.graph.edge_index.device
        plan = self._programs(queries)
        n = sum(len(index) for index, _ in plan)
        assumed = self._assumed(assuming, n)
        if among is not None:
            among = self._sets.assemble(among, n, dev)
        return self._what_if(lambda assumed: self._answer_sets(plan, n, threshold, among, assumed), queries, assumed, among,
                             probability)

    def _answer_sets(self, plan, n, threshold, among, assumed):
        dev = self.graph.edge_index.device
        length = torch.zeros(n, dtype=torch.long, device=dev)
        size = torch.zeros(n, dtype=torch.long, device=dev)
        done = []
        with self._batches(plan, among, assumed) as batches:
            for index, logits, ptr, known, live in batches:
                if logits.is_cuda:
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above(logits, threshold, ptr, known, **live)
                    total = int(b_ptr[-1])      # (the one host read of the batch)
                    b_ids, b_scores = b_ids[:total].clone(), b_scores[:total].clone()
                else:
                    b_ptr, b_ids, b_scores, b_size = predict.filtered_above_reference(logits, threshold, ptr, known, **live)
                where = torch.tensor(index, dtype=torch.long).to(dev, non_blocking=True)
                length[where], size[where] = b_ptr[1:] - b_ptr[:-1], b_size
                done.append((where, b_ptr, b_ids, b_scores))
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
