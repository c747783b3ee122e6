"""Candidate sets: the allow lists of a served graph.

A query's candidates are, by default, every entity minus a deny list (the known or entailed answers, the reserve, the retired
ids).  `among=` of the predictors restricts them to a set instead -- "the tail must be a drug", "rank these 100 ids" -- and
this module owns what such an argument may be and how a call's sets reach the kernels:

    sets = CandidateSets(slots)                 # slots: the ids' range, an int or a callable that gives it now
    sets.define_set("drug", ids)                # sorted, de-duplicated, range-checked; replaces a set of that name
    span, index, longest = sets.assemble(among, n, device)

`among` is a name (one set for every query), a 1-D id vector or list of ids (likewise), or a sequence of n names or vectors (one
per query).  assemble stores every DISTINCT set of the call once in `index` and gives every query a (begin, end) span into it:
the operands of the ultra_filtered_*_among entries (selection.among_operand).  An id is any slot of the graph: one in the reserve
or a retired one is allowed in a set and simply absent until it is live and alive -- the kernels decide, at run time.  Ids are
stable (a compaction or a rebuild beyond the reserve renumbers nothing), so a set outlives both.
"""
import torch


class CandidateSets(object):
    def __init__(self, slots):
        self._slots = slots if callable(slots) else (lambda: slots)
        self._sets = {}

    @property
    def slots(self):
        return int(self._slots())

    def normalise(self, ids):
        """`ids` (a vector, a list, an int) as ascending distinct int64 ids on the host; ValueError for an id outside
        [0, slots) or something that is no vector of integers."""
        try:
            ids = torch.as_tensor(ids)
            if ids.numel() and (ids.dtype == torch.bool or ids.is_floating_point() or ids.is_complex()):     # ([] is a float tensor)
                raise TypeError
            ids = ids.to(device="cpu", dtype=torch.long).flatten()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("a candidate set is a vector of integer entity ids, got %r" % (type(ids).__name__,))
        slots = self.slots
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= slots):
            bad = ids[(ids < 0) | (ids >= slots)]
            raise ValueError("a candidate set holds entity ids in [0, %d) (the slots of the served graph), got %d"
                             % (slots, int(bad[0])))
        return torch.unique(ids)        # (sorted)

    def define_set(self, name, ids):
        """Name the set `ids` (normalise): `among=name` means it from now on.  A set of that name is replaced.  Returns its size."""
        if not isinstance(name, str) or not name:
            raise ValueError("a candidate set's name is a non-empty string, got %r" % (name,))
        ids = self.normalise(ids)
        self._sets[name] = ids
        return ids.numel()

    def drop_set(self, name):
        """Forget the set `name` (KeyError where there is none)."""
        if name not in self._sets:
            raise KeyError("no candidate set named %r (defined: %s)" % (name, ", ".join(sorted(self._sets)) or "none"))
        del self._sets[name]

    def sets(self):
        """{name: size} of the sets defined now."""
        return {name: ids.numel() for name, ids in sorted(self._sets.items())}

    def _named(self, name):
        if name not in self._sets:
            raise KeyError("no candidate set named %r (defined: %s)" % (name, ", ".join(sorted(self._sets)) or "none"))
        return self._sets[name]

    @staticmethod
    def _is_one_vector(among):
        """Is `among` ONE set of ids (a 1-D tensor, or a flat sequence of ints) rather than a sequence of sets?"""
        if torch.is_tensor(among):
            return among.dim() <= 1
        if hasattr(among, "dtype") and hasattr(among, "ndim"):      # (a numpy array)
            return among.ndim <= 1
        return all(isinstance(v, int) and not isinstance(v, bool) for v in among)

    def resolve(self, among, n):
        """`among` as a list of n (key, ids) pairs, one per query: ids normalised, key equal where two queries mean the same
        stored set (a name, or the very object given).  KeyError: an unknown name; ValueError: a wrong count, a bad id."""
        if isinstance(among, str):
            return [(("name", among), self._named(among))] * n
        if self._is_one_vector(among):
            return [(("all",), self.normalise(among))] * n
        among = list(among)
        if len(among) != n:
            raise ValueError("one candidate set per query: got %d sets for %d queries" % (len(among), n))
        seen, out = {}, []
        for one in among:
            key = ("name", one) if isinstance(one, str) else ("object", id(one))
            if key not in seen:
                seen[key] = self._named(one) if isinstance(one, str) else self.normalise(one)
            out.append((key, seen[key]))
        return out

    def assemble(self, among, n, device):
        """(span (n, 2) int64, index int64, longest): the call's sets, every distinct one stored once in `index`, query i's
        candidates index[span[i, 0] : span[i, 1]]; both on `device`; longest: the longest set's length (a host int)."""
        at, chunks, total, span, longest = {}, [], 0, [], 0
        for key, ids in self.resolve(among, n):
            if key not in at:
                at[key] = (total, total + ids.numel())
                chunks.append(ids)
                total += ids.numel()
                longest = max(longest, ids.numel())
            span.append(at[key])
        index = torch.cat(chunks) if chunks else torch.zeros(0, dtype=torch.long)
        span = torch.tensor(span, dtype=torch.long).reshape(n, 2)
        return span.to(device), index.to(device), longest


def span_rows(span, index):
    """The sets of (span, index) as a list of per-row id vectors: the form the _reference functions take."""
    return [index[int(b):int(e)] for b, e in span.tolist()]


def named_ids(vocab, names=None, path=None):
    """The command-line form of a candidate set (tools/predict.py, tools/query_predict.py: --among NAME ..., --among-file FILE
    with one entity name per line): the ids of the names in `vocab` (the entity names of data.read_vocab, in id order), or
    None where neither option was given.  ValueError for an unknown name, which the message names."""
    if names is None and path is None:
        return None
    wanted = list(names or [])
    if path is not None:
        with open(path) as f:
            wanted += [line.strip() for line in f if line.strip()]
    at = {name: i for i, name in enumerate(vocab)}
    unknown = [name for name in wanted if name not in at]
    if unknown:
        raise ValueError("unknown entity %r in the candidate set" % unknown[0])
    return [at[name] for name in wanted]
