"""The edit state of one served graph, in one place ("The live graph's state in one place").

predict.Predictor and query_predict.QueryPredictor each hold one LiveGraph and forward add_facts / remove_facts / add_entities /
compact / materialized to it.  The rules that define a served graph live here and nowhere else: what counts as an edit, when the
delta is folded into the graph, which ids are live, and what `materialized()` means.

  LiveGraph        the served graph (reserved rows included), its rspmm.GraphDelta, the live count and -- where the owner reads known
                   answers from a graph -- the filter graph
  with_facts       a copy of a graph with facts appended the way GraphDelta.materialize appends them
  without_facts    ... without every edge of the facts
  with_slots       ... with reserved rows
  with_relation_slots / compact_relations   ... laid out over reserved relation slots, and back in the compact numbering
  check_live       ValueError for an id in the reserve
  check_not_retired   ... for an id that was retired (LiveGraph.remove_entities)
  retired_words    the retired bitmap of a set of ids, as the ultra_filtered_*_alive entries read it
  check_live_relations   ... for a relation id that is no direct relation in use
  forwarded        a read-only property of an owner that reads a field of its LiveGraph
"""
import copy
import operator

import torch

from . import rspmm, tasks


def with_facts(graph, h, r, t):
    """A copy of `graph` with the edges of the facts appended the way GraphDelta.materialize appends them: the direct edges
    (h, t, r), then the inverse ones (t, h, r + num_relations / 2)."""
    out = copy.copy(graph)
    dev = graph.edge_index.device
    h, r, t = h.to(dev), r.to(dev), t.to(dev)
    out.edge_index = torch.cat([graph.edge_index, torch.stack([torch.cat([h, t]), torch.cat([t, h])])], dim=1)
    out.edge_type = torch.cat([graph.edge_type, torch.cat([r, r + int(graph.num_relations) // 2])])
    return out


def without_facts(graph, h, r, t):
    """A copy of `graph` without every edge equal to (h[i], t[i], r[i]) or to (t[i], h[i], r[i] + num_relations / 2)."""
    out = copy.copy(graph)
    dev = graph.edge_index.device
    h, r, t = h.to(dev), r.to(dev), t.to(dev)
    n, rels = int(graph.num_nodes), int(graph.num_relations)
    gone = torch.cat([(h * n + t) * rels + r, (t * n + h) * rels + r + rels // 2]).unique()
    codes = (graph.edge_index[0] * n + graph.edge_index[1]) * rels + graph.edge_type
    keep = gone[torch.searchsorted(gone, codes).clamp_(max=len(gone) - 1)] != codes
    out.edge_index, out.edge_type = graph.edge_index[:, keep], graph.edge_type[keep]
    return out


def with_slots(graph, slots, relation_graph=False):
    """A shallow copy of `graph` with num_nodes = slots >= graph.num_nodes: the same edge list, the rows beyond the old count
    reserved (no edge names them).  relation_graph: build the copy's own where `graph` carries one -- it equals graph's, a
    node without edges plays no role."""
    out = copy.copy(graph)
    out.num_nodes = int(slots)
    if relation_graph and getattr(graph, "relation_graph", None) is not None:
        tasks.build_relation_graph(out)
    return out


def _renumbered(graph, old_direct, new_direct, relation_graph):
    out = copy.copy(graph)
    out.num_relations = 2 * int(new_direct)
    if new_direct != old_direct:
        out.edge_type = torch.where(graph.edge_type >= old_direct, graph.edge_type + (new_direct - old_direct), graph.edge_type)
    if relation_graph and getattr(graph, "relation_graph", None) is not None:
        tasks.build_relation_graph(out)
    return out


def with_relation_slots(graph, direct_slots, direct_live, relation_graph=True):
    """A shallow copy of `graph` -- direct_live direct relations, inverse type r + direct_live -- laid out over direct_slots >=
    direct_live direct relation SLOTS: num_relations = 2 direct_slots, every inverse type moved to r + direct_slots, the edge
    order untouched.  relation_graph: build the copy's own where `graph` carries one -- over the 2 direct_slots
    nodes, the slots without a relation isolated."""
    if int(direct_slots) < int(direct_live):
        raise ValueError("%d direct relations do not fit %d slots" % (direct_live, direct_slots))
    return _renumbered(graph, int(direct_live), int(direct_slots), relation_graph)


def compact_relations(graph, direct_slots, direct_live, relation_graph=True):
    """The inverse of with_relation_slots: `graph`, laid out over direct_slots slots of which the ids below direct_live are in
    use, in the compact numbering -- num_relations = 2 direct_live, inverse type r + direct_live."""
    return _renumbered(graph, int(direct_slots), int(direct_live), relation_graph)


def check_live_relations(ids, num_live, what):
    """ValueError unless every id is a direct relation in use: ids in [0, num_live) (a graph with reserved relation slots; one
    host read)."""
    if len(ids) and bool(((ids < 0) | (ids >= num_live)).any()):
        raise ValueError("%s must be direct relations in use (ids in [0, %d)): a reserved slot is no relation until "
                         "add_relations hands it out" % (what, num_live))


def check_live(ids, num_live, what):
    """ValueError unless every id is an entity in use: ids in [0, num_live) (a graph with reserved rows; one host read)."""
    if len(ids) and bool(((ids < 0) | (ids >= num_live)).any()):
        raise ValueError("%s must be existing entities (ids in [0, %d)): a reserved row is no entity until add_entities hands "
                         "it out" % (what, num_live))


def check_not_retired(ids, retired, what):
    """ValueError where an id is one of `retired` (a sorted int64 vector, or None: nothing is retired; one host read)."""
    if retired is not None and len(retired) and len(ids) and bool(torch.isin(ids, retired.to(ids.device)).any()):
        raise ValueError("%s must be existing entities: %s retired (remove_entities) and an id is never handed out again"
                         % (what, "ids %s are" % retired.tolist() if len(retired) <= 8 else "%d ids are" % len(retired)))


def retired_words(ids, num_slots, device=None):
    """The bitmap of the distinct ids `ids` over num_slots slots: ceil(num_slots / 32) 32-bit words, id v bit v & 31 of word
    v >> 5 -- the uint32 words the ultra_filtered_*_alive entries read, held as int32 (torch has no arithmetic on uint32; bit
    31 is the sign bit, the bits are the same)."""
    ids = torch.as_tensor(ids, dtype=torch.long, device=device).flatten()
    words = torch.zeros((int(num_slots) + 31) // 32, dtype=torch.long, device=ids.device)
    words.index_add_(0, ids >> 5, torch.ones_like(ids) << (ids & 31))      # (distinct ids: a sum of distinct bits is their OR)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)


def forwarded(name):
    """For an owner that holds its LiveGraph as `_live`: a read-only property that reads `name` of it, so that the owner's
    attributes of before stay readable under their names."""
    return property(operator.attrgetter("_live." + name))


class LiveGraph(object):
    """data: the graph to serve; delta_capacity: the facts (added + retracted) held in an rspmm.GraphDelta beside it before they
    are folded into it; entity_capacity=M > 0: M rows reserved for entities that arrive later -- `graph` is then a shallow copy
    of `data` with num_nodes = N + M slots and its own relation graph, `num_entities` of them live, and `live_count` one device
    int64 that holds the same number for the owner's life (None without a reserve).  relation_capacity=K > 0: K
    direct relation slots reserved for relations that arrive later -- `graph` is then laid out over R + K direct slots
    (with_relation_slots; the filter graph alike), `num_direct_relations` of them in use.  relation_bits_budget: the delta's
    (rspmm.GraphDelta).  live_relation_graph: the delta's too -- True: its relation graph is one object that is
    kept current in place, so an edit that changes relation-graph cells costs no plan and no new capture.

    delta_policy: when the delta exists.  "eager": from construction, and a new empty one after every compaction (a captured
    step is handed the delta before the first edit).  "lazy": None until the first edit and None again after a compaction (an
    owner that was never edited runs exactly what it ran before).  "never": no delta -- every add_facts compacts, every
    remove_facts is folded at once (a model without a delta route).

    keep_filter: also hold the graph known answers are read from, `filter_graph` -- `filter_data` with the same edits, or (None)
    the served graph with them.  Without it `filter_graph` is None.

    owner: the class name in add_entities' error text.  on_rebuild(): called in every compaction that changes the served
    graph, before `graph` is replaced.

    RETIRED entities (remove_entities): `retired_entities` (a sorted int64 vector on the graph's device) are ids
    below num_entities whose facts are gone and that are never an answer, an anchor or an argument again; ids are not
    renumbered and a slot is not handed out again.  From the first retirement on `retired_bits` (retired_words over num_slots:
    one device bitmap, rewritten in place) and `retired_count` (one device int64) hold the same set for the selection kernels;
    both keep their addresses, survive compact(), and only a rebuild that changes the slot count lays a longer bitmap out (the
    captured steps are released there anyway).  `retired_operand`: the pair (retired_bits, retired_count), one object while the
    bitmap is -- what a captured step takes and remembers.  All three are None before the first retirement."""

    def __init__(self, data, delta_capacity=256, entity_capacity=0, filter_data=None, keep_filter=False, delta_policy="lazy",
                 owner="LiveGraph", on_rebuild=None, relation_capacity=0, relation_bits_budget=256 << 20,
                 live_relation_graph=False):
        if not isinstance(live_relation_graph, bool):
            raise ValueError("live_relation_graph must be True or False, got %r" % (live_relation_graph,))
        self.live_relation_graph = live_relation_graph
        if isinstance(entity_capacity, bool) or not isinstance(entity_capacity, int) or entity_capacity < 0:
            raise ValueError("entity_capacity must be a non-negative int (reserved rows), got %r" % (entity_capacity,))
        if isinstance(relation_capacity, bool) or not isinstance(relation_capacity, int) or relation_capacity < 0:
            raise ValueError("relation_capacity must be a non-negative int (reserved relation slots), got %r" % (relation_capacity,))
        if isinstance(delta_capacity, bool) or not isinstance(delta_capacity, int) or delta_capacity < 1:
            raise ValueError("delta_capacity must be a positive int (facts), got %r" % (delta_capacity,))
        if delta_policy not in ("eager", "lazy", "never"):
            raise ValueError("delta_policy must be 'eager', 'lazy' or 'never', got %r" % (delta_policy,))
        self.entity_capacity, self.delta_capacity = entity_capacity, delta_capacity
        self.relation_capacity, self.relation_bits_budget = relation_capacity, relation_bits_budget
        self.num_entities = int(data.num_nodes)
        self.num_direct_relations = int(data.num_relations) // 2
        self.live_count = None
        if entity_capacity:
            slots = self.num_entities + entity_capacity
            data = with_slots(data, slots, relation_graph=not relation_capacity)
            if filter_data is not None:
                filter_data = with_slots(filter_data, slots)
            self.live_count = torch.full((1,), self.num_entities, dtype=torch.long, device=data.edge_index.device)
        if relation_capacity:
            direct = self.num_direct_relations
            data = with_relation_slots(data, direct + relation_capacity, direct)
            if filter_data is not None:
                filter_data = with_relation_slots(filter_data, direct + relation_capacity, direct, relation_graph=False)
        self.graph = data
        self._policy, self._owner, self._on_rebuild = delta_policy, owner, on_rebuild
        self.filter_graph = self._filter_base = None
        self._filter_is_graph = False
        if keep_filter:
            self.filter_graph = self._filter_base = data if filter_data is None else filter_data
            self._filter_is_graph = self.filter_graph is data
        self.retired_entities = torch.zeros(0, dtype=torch.long, device=data.edge_index.device)
        self.retired_bits = self.retired_count = self.retired_operand = None
        self.delta = self._new_delta() if delta_policy == "eager" else None

    @property
    def num_retired(self):
        """How many entities were retired (remove_entities)."""
        return int(self.retired_entities.numel())

    @property
    def num_slots(self):
        """The rows of the served graph: num_entities live ones and the rest of the reserve."""
        return int(self.graph.num_nodes)

    @property
    def num_relation_slots(self):
        """The direct relation slots of the served graph: num_direct_relations in use and the rest of the reserve."""
        return int(self.graph.num_relations) // 2

    def _new_delta(self, capacity=None):
        delta = rspmm.GraphDelta(self.graph, self.delta_capacity if capacity is None else capacity, num_live=self.num_entities,
                                 num_live_relations=self.num_direct_relations, relation_bits_budget=self.relation_bits_budget,
                                 live_relation_graph=self.live_relation_graph)
        delta.retired = self.retired_entities if self.num_retired else None
        return delta

    def _probe(self):
        """A delta to check arguments with or to materialise through: the one held, or an empty one."""
        return self.delta if self.delta is not None else self._new_delta(1)

    def _own_delta(self):
        if self.delta is None:      # ("lazy": made at the first edit that fits)
            self.delta = self._new_delta()
        return self.delta

    def _fits(self, n):
        """Can the delta take n more facts or retractions?  A fact holds two edges, a retraction at most two tombstone keys."""
        if self._policy == "never":
            return False
        held = 0 if self.delta is None else 2 * len(self.delta) + self.delta.num_removed
        return held + 2 * n <= 2 * self.delta_capacity

    def num_live_for(self, on_gpu):
        """What the lists and the selection take beside their arguments: nothing without a reserve; with one, the live count --
        the device scalar for the kernels, the host int for the plain-torch restatements."""
        if not self.entity_capacity:
            return {}
        return {"num_live": self.live_count if on_gpu else self.num_entities}

    def selection_for(self, on_gpu):
        """num_live_for plus, once an entity was retired, `retired`: the device pair (retired_bits, retired_count) for the
        kernels, the sorted id vector for the plain-torch restatements.  Before the first retirement: num_live_for."""
        out = self.num_live_for(on_gpu)
        if self.num_retired:
            out["retired"] = self.retired_operand if on_gpu else self.retired_entities
        return out

    def check_entities(self, ids, what):
        """ValueError unless every id is an entity in use: not in the reserve (where rows are reserved) and not retired."""
        if self.entity_capacity:
            check_live(ids, self.num_entities, what)
        check_not_retired(ids, self.retired_entities, what)

    # ---- retiring entities ----
    def remove_entities(self, ids):
        """Retire the entities `ids` (an int or a vector of distinct live ids that are not retired yet; ValueError otherwise, and
        nothing is changed): every fact of the materialised graph that names one of them as head or tail is retracted through
        remove_facts -- base edges become tombstones, held delta facts leave the delta, the filter graph loses them in both
        directions (a filter graph of its own also loses every other edge at the ids: no retired id is a known answer), a call
        that does not fit compacts or folds as remove_facts does -- and the ids are retired: never an answer, never counted, a
        ValueError as an anchor or as h / t of add_facts / remove_facts.  Ids stay what they are; num_entities stays the prefix
        bound.  The incident facts are collected on the device, once per call, from BOTH columns of the edge list (a list that
        is not closed under inverses loses every edge at the ids) as distinct direct triples.  Returns an int64 vector: per id
        the number of distinct facts retracted that name it (a fact between two ids of the call counts for both)."""
        dev = self.graph.edge_index.device
        ids = torch.as_tensor(ids, dtype=torch.long, device=dev).flatten()
        if len(ids) == 0:
            return torch.zeros(0, dtype=torch.long, device=dev)
        if bool(((ids < 0) | (ids >= self.num_entities)).any()):
            raise ValueError("remove_entities takes existing entities (ids in [0, %d)): a negative id, an id beyond the slots or "
                             "a reserved row is none" % self.num_entities)
        if len(torch.unique(ids)) != len(ids):
            raise ValueError("remove_entities takes distinct ids: one is repeated")
        check_not_retired(ids, self.retired_entities, "the entities to retire")
        graph = self._probe().materialize(self.graph)
        (row, col), edge_type = graph.edge_index, graph.edge_type
        at = (torch.isin(row, ids) | torch.isin(col, ids)).nonzero().flatten()
        row, col, edge_type = row[at], col[at], edge_type[at]
        direct = self.num_relation_slots
        inverse = edge_type >= direct
        triples = torch.stack([torch.where(inverse, col, row), torch.where(inverse, edge_type - direct, edge_type),
                               torch.where(inverse, row, col)], dim=1)
        triples = torch.unique(triples, dim=0) if len(triples) else triples
        h, r, t = triples.unbind(1)
        counts = ((h.unsqueeze(0) == ids.unsqueeze(1)) | (t.unsqueeze(0) == ids.unsqueeze(1))).sum(dim=1)
        if len(h):
            self.remove_facts(h, r, t)
        if self.filter_graph is not None and not self._filter_is_graph:
            base = self._filter_base
            keep = ~(torch.isin(base.edge_index[0], ids.to(base.edge_index.device))
                     | torch.isin(base.edge_index[1], ids.to(base.edge_index.device)))
            if not bool(keep.all()):
                self._filter_base = copy.copy(base)
                self._filter_base.edge_index, self._filter_base.edge_type = base.edge_index[:, keep], base.edge_type[keep]
                self._refresh_filter_graph()
        self.retired_entities = torch.sort(torch.cat([self.retired_entities, ids])).values
        self._lay_out_retired()
        if self.delta is not None:
            self.delta.retired = self.retired_entities
        return counts

    def _lay_out_retired(self):
        """retired_bits / retired_count of retired_entities over the slots there are now: written into the tensors held, which
        are allocated at the first retirement and replaced only where the slot count changed."""
        if not self.num_retired:
            return
        words = retired_words(self.retired_entities, self.num_slots)
        if self.retired_bits is None or self.retired_bits.numel() != words.numel():
            self.retired_bits = words
        else:
            self.retired_bits.copy_(words)
        if self.retired_count is None:
            self.retired_count = torch.zeros(1, dtype=torch.long, device=words.device)
        self.retired_count.fill_(self.num_retired)
        if self.retired_operand is None or self.retired_operand[0] is not self.retired_bits:
            self.retired_operand = (self.retired_bits, self.retired_count)

    # ---- the growing graph ----
    def add_entities(self, count=1, compact=None):
        """`count` new entities: their ids [num_entities, num_entities + count), and the live count raised -- the host int, the
        device scalar and the delta's bound.  Beyond the reserve num_entities + count + entity_capacity slots are laid out by
        `compact(slots=...)`: this object's, or the owner's own `compact` where it hands that in (it forwards here)."""
        if not self.entity_capacity:
            raise ValueError("this %s reserves no rows: create it with entity_capacity > 0 to add entities" % self._owner)
        if isinstance(count, bool) or not isinstance(count, int) or count < 1:
            raise ValueError("count must be a positive int, got %r" % (count,))
        first = self.num_entities
        if first + count > self.num_slots:
            (compact or self.compact)(slots=first + count + self.entity_capacity)
        self.num_entities = first + count
        self.live_count.fill_(self.num_entities)
        if self.delta is not None:
            self.delta.num_live = self.num_entities
        return torch.arange(first, first + count, dtype=torch.long, device=self.graph.edge_index.device)

    def add_relations(self, count=1, compact=None):
        """`count` new direct relations: their ids [num_direct_relations, num_direct_relations + count), and the live count
        raised, here and in the delta.  No plan, no relation graph, no capture: a slot without facts is an isolated node the
        relation graph already holds.  Beyond the reserve num_direct_relations + count + relation_capacity slots are laid out
        by `compact(relation_slots=...)` -- this object's, or the owner's own where it hands that in."""
        if not self.relation_capacity:
            raise ValueError("this %s reserves no relation slots: create it with relation_capacity > 0 to add relations" % self._owner)
        if isinstance(count, bool) or not isinstance(count, int) or count < 1:
            raise ValueError("count must be a positive int, got %r" % (count,))
        first = self.num_direct_relations
        if first + count > self.num_relation_slots:
            (compact or self.compact)(relation_slots=first + count + self.relation_capacity)
        self.num_direct_relations = first + count
        if self.delta is not None:
            self.delta.num_live_relations = self.num_direct_relations
        return torch.arange(first, first + count, dtype=torch.long, device=self.graph.edge_index.device)

    def materialized(self):
        """The served edge list with the delta's edits (GraphDelta.materialize) and num_nodes = num_entities -- no reserved row --
        with the filter graph held now as its `filtered_data` where that is a graph of its own.  With reserved relation slots:
        in the compact numbering -- num_relations = 2 num_direct_relations, inverse type r + num_direct_relations, the relation
        graph built for it (the filter graph alike).  Retired ids keep their place: they are isolated nodes of the copy, named
        by its `retired_entities` (a sorted int64 vector).  A new copy at every call."""
        out = copy.copy(self._probe().materialize(self.graph, num_nodes=self.num_entities))
        out.retired_entities = self.retired_entities.clone()
        slots, live = self.num_relation_slots, self.num_direct_relations
        if self.relation_capacity:
            out = compact_relations(out, slots, live)
        if self.filter_graph is not None and not self._filter_is_graph:     # (the one held now, the stated facts included)
            out.filtered_data = copy.copy(self.filter_graph)
            out.filtered_data.num_nodes = self.num_entities
            if self.relation_capacity:
                out.filtered_data = compact_relations(out.filtered_data, slots, live, relation_graph=False)
        return out

    # ---- the changing graph ----
    def add_facts(self, h, r, t):
        h, r, t = self._probe().check(h, r, t)
        if len(h) == 0:
            return 0 if self.delta is None else len(self.delta)
        if not self._fits(len(h)):
            self.compact(extra=(h, r, t))
            return 0
        self._own_delta().add(h, r, t)
        self._refresh_filter_graph()
        return len(self.delta)

    def remove_facts(self, h, r, t):
        h, r, t = self._probe().check(h, r, t)
        if len(h) == 0:
            return torch.zeros(0, dtype=torch.long, device=h.device)
        # (a call that may not fit compacts first, and one larger than the whole capacity is applied to a delta of its own and
        # folded at once)
        if not self._fits(len(h)):
            self.compact()
        fold = None
        if self._fits(len(h)):
            removed = self._own_delta().remove(h, r, t)
        else:
            fold = self._new_delta(len(h))
            removed = fold.remove(h, r, t)
        if self.filter_graph is not None and not self._filter_is_graph:
            self._filter_base = without_facts(self._filter_base, h, r, t)
        if fold is not None:
            self.compact(delta=fold)
        self._refresh_filter_graph()
        return removed

    def _refresh_filter_graph(self):
        if self.filter_graph is None:
            return
        if self.delta is None:
            self.filter_graph = self._filter_base
        elif self._filter_is_graph:
            self.filter_graph = self.delta.materialize(self.graph)
        else:
            fh, fr, ft = self.delta.facts[:len(self.delta)].unbind(1)
            self.filter_graph = with_facts(self._filter_base, fh, fr, ft)

    def compact(self, extra=None, delta=None, slots=None, relation_slots=None):
        """Fold the delta's edits (and `extra` = (h, r, t), checked by the caller) into the served graph: the materialised graph
        -- without the tombstoned edges, with the added ones, its relation graph rebuilt -- becomes `graph`, and the delta is
        emptied.  `delta`: fold that one instead of the one held.  The slot count and the live count of a graph with reserved
        rows stay; `slots` (add_entities beyond the reserve): the new slot count, laid out in the same rebuild; `relation_slots`
        (add_relations beyond the reserve): the new count of direct relation slots, the inverse types renumbered in it."""
        delta = self.delta if delta is None else delta
        facts = [] if delta is None else [delta.facts[:len(delta)]]
        if extra is not None:
            facts.append(torch.stack(list(extra), dim=1))
        facts = torch.cat(facts) if facts else torch.zeros(0, 3, dtype=torch.long)
        if slots is not None and int(slots) == self.num_slots:
            slots = None
        old_rel = self.num_relation_slots
        if relation_slots is not None and int(relation_slots) == old_rel:
            relation_slots = None
        if len(facts) == 0 and not (delta is not None and delta.num_removed) and slots is None and relation_slots is None:
            return
        fh, fr, ft = facts.unbind(1)
        base = self.graph
        if delta is not None and delta.num_removed:
            base = copy.copy(self.graph)
            base.edge_index, base.edge_type = delta.surviving(self.graph.edge_index, self.graph.edge_type)
        graph = with_facts(base, fh, fr, ft)
        if slots is not None:
            graph.num_nodes = int(slots)
        if relation_slots is not None:      # (the in-use ids lie below both counts: only the inverse types move)
            graph = _renumbered(graph, old_rel, int(relation_slots), relation_graph=False)
        if getattr(self.graph, "relation_graph", None) is not None:
            tasks.build_relation_graph(graph)
        if self.filter_graph is not None:
            if self._filter_is_graph:
                self._filter_base = graph
            else:
                self._filter_base = with_facts(self._filter_base, fh, fr, ft)
                if slots is not None:
                    self._filter_base.num_nodes = int(slots)
                if relation_slots is not None:
                    self._filter_base = _renumbered(self._filter_base, old_rel, int(relation_slots), relation_graph=False)
            self.filter_graph = self._filter_base
        if self._on_rebuild is not None:
            self._on_rebuild()
        self.graph = graph
        self._lay_out_retired()     # (the retired rows stay, as isolated slots; a new slot count: a longer bitmap, the bits kept)
        self.delta = self._new_delta() if self._policy == "eager" else None
