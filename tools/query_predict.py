"""Answer one complex logical query on a dataset of triple files: the k entities the model predicts, with their scores.

    python tools/query_predict.py --data-root DIR [--ckpt FILE] --query "(('e1', ('r1',)), ('e2', ('r2', -2)))" [-k 10]
                                  [--logic product] [--unfiltered] [--above P] [--add-fact H R T]... [--remove-fact H R T]...
                                  [--entity-capacity M] [--add-entity NAME]... [--remove-entity NAME]...
                                  [--among NAME [NAME ...]] [--among-file FILE] [--assume H R T]...

DIR holds train.txt / valid.txt / test.txt (`head relation tail` per line) and optionally entities.dict / relations.dict
(ultra_amd.data.load_triples_dir).  The query is a BetaE nested tuple (ultra_amd.ultraquery.Query.from_nested): a pair
(anchor, (relation, ...)) projects the anchor -- an entity, or a nested query -- along the chain, where -2 negates; any other
tuple intersects its branches, or unites them when it ends with (-1,).  Entities and relations are names of the
vocabularies or integer ids.  Answers the graph already entails (the symbolic traversal of the query) are left out unless
--unfiltered.  --above P prints the answer SET instead of the k best: every entity the model predicts with probability above P
(0 < P < 1: a logit above log(P / (1 - P)), QueryPredictor.answer_sets), ranked, and the predicted size of the set, which
counts the entailed answers too.  --ckpt: an UltraQuery checkpoint (a state dict, or a dict with the state under "model"); without it the
weights are randomly initialised, and the tool says so.

--add-fact H R T (repeatable) states a fact between known entities before the query is answered (QueryPredictor.add_facts): the
query's projections traverse it and the answers it entails are left out.  --remove-fact H R T (repeatable) retracts one
(QueryPredictor.remove_facts): every edge that states it leaves the graph, so it is no longer traversed and its tail can be
predicted again.  Both kinds are applied in command-line order; H, R and T are names of the vocabularies or integer ids, R a
relation of the dataset (not an inverse).

--add-entity NAME (repeatable) introduces an entity the dataset does not know (QueryPredictor.add_entities): it takes one of the
rows reserved by --entity-capacity M (default: as many as there are --add-entity options), costs no plan, no relation graph and
no traversal index, and from then on NAME is an entity like any other -- in the --add-fact / --remove-fact options that FOLLOW it
on the command line, as an anchor of the query and in the printed answers.

--remove-entity NAME (repeatable) takes an entity out of the graph served before the query is answered
(QueryPredictor.retire_entities): every fact that names it is retracted and the entity is retired -- never an
answer, never an entailed answer, no anchor.  It is applied in command-line order with the other edit options; NAME (a name of
the vocabulary, one added earlier on the command line, or an integer id) no longer resolves in the options that follow it, nor
in the query.

--among NAME [NAME ...] and --among-file FILE (entity names, one per line; both may be given, the set is their union) restrict
the candidates to a set (QueryPredictor.answers(among=)): only these entities are ranked, or listed by --above.
An unknown name is an error that names it; a name introduced by --add-entity may be listed, a retired entity is simply absent.

--assume H R T (repeatable) answers the query as if the fact were true WITHOUT stating it (QueryPredictor.answers(assuming=),
DESIGN.md 33): the query's projections traverse it and the answers it entails are left out, while the graph served and its
edits stay what they were.  The names are those known after every edit option; R is a relation of the dataset (not an inverse).
"""
import argparse
import ast
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def resolve(nested, ent, rel, gone=()):
    """The nested tuple with every name replaced by its id (the shapes are those of Query.nested_to_postfix); `gone`: the names
    that were retired on the command line, which resolve no longer."""
    def lookup(name, vocab, what):
        if isinstance(name, int):
            return name
        if name not in vocab or (vocab is ent and name in gone):
            sys.exit("unknown %s %r" % (what, name))
        return vocab.index(name)
    if len(nested) == 2 and not isinstance(nested[1][-1], tuple):
        anchor, chain = nested
        anchor = resolve(anchor, ent, rel, gone) if isinstance(anchor, tuple) else lookup(anchor, ent, "entity")
        return (anchor, tuple(lookup(step, rel, "relation") for step in chain))
    return tuple(branch if branch == (-1,) else resolve(branch, ent, rel, gone) for branch in nested)


def lookup_fact(fact, ent, rel, gone=()):
    """(h, r, t) ids of an --add-fact / --remove-fact option: names of the vocabularies, or integer ids; `gone`: the entity
    names retired earlier on the command line, which resolve no longer."""
    out = []
    for name, vocab, what in zip(fact, (ent, rel, ent), ("entity", "relation", "entity")):
        if name in vocab and not (vocab is ent and name in gone):
            out.append(vocab.index(name))
        elif name.lstrip("-").isdigit():
            out.append(int(name))
        else:
            sys.exit("unknown %s %r" % (what, name))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-root", required=True)
    ap.add_argument("--ckpt")
    ap.add_argument("--query", required=True, help="a BetaE nested tuple of names or ids")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--logic", default="product", choices=["product", "godel", "lukasiewicz"])
    ap.add_argument("--unfiltered", action="store_true")
    ap.add_argument("--above", type=float, metavar="P", help="print the whole answer set: every entity with probability above P")
    class Edit(argparse.Action):       # (one list for all kinds: they are applied in command-line order)
        def __call__(self, parser, namespace, values, option_string=None):
            namespace.edits = getattr(namespace, "edits", None) or []
            if option_string == "--add-entity":
                namespace.edits.append((None, values))
            elif option_string == "--remove-entity":
                namespace.edits.append(("retire", values))
            else:
                namespace.edits.append((option_string == "--add-fact", tuple(values)))

    ap.add_argument("--add-fact", nargs=3, action=Edit, metavar=("H", "R", "T"),
                    help="state the fact (H, R, T) before the query; repeatable")
    ap.add_argument("--remove-fact", nargs=3, action=Edit, metavar=("H", "R", "T"),
                    help="retract the fact (H, R, T) before the query; repeatable, applied in order with --add-fact")
    ap.add_argument("--add-entity", action=Edit, metavar="NAME",
                    help="introduce a new entity before the query; repeatable, applied in order with the fact options")
    ap.add_argument("--remove-entity", action=Edit, metavar="NAME",
                    help="retire an entity and retract its facts before the query; repeatable, applied in order with the other edits")
    ap.add_argument("--entity-capacity", type=int, default=None, metavar="M",
                    help="rows reserved for new entities (default: the number of --add-entity options)")
    ap.add_argument("--assume", nargs=3, action="append", default=[], metavar=("H", "R", "T"),
                    help="answer as if the fact (H, R, T) were true, without stating it; repeatable")
    ap.add_argument("--among", nargs="+", metavar="NAME", help="rank only these entities (a shortlist, a type)")
    ap.add_argument("--among-file", metavar="FILE", help="... the entity names of FILE, one per line")
    ap.set_defaults(edits=[])
    args = ap.parse_args(argv)
    if args.entity_capacity is not None and args.entity_capacity < 0:
        sys.exit("--entity-capacity must not be negative")
    if args.above is not None and not 0.0 < args.above < 1.0:
        sys.exit("--above takes a probability strictly between 0 and 1, got %r" % args.above)
    if not torch.cuda.is_available():
        sys.exit("tools/query_predict.py needs a GPU: the engine has no CPU path")
    from ultra_amd import data as udata
    from ultra_amd import models, query_predict, synthetic, ultraquery
    ent, rel = udata.read_vocab(args.data_root)
    ent = list(ent)        # (grows along the command line: a name resolves in the options after its --add-entity; the ids are
    num_known = len(ent)   # handed out in that order)
    gone = set()           # (the names retired so far: they resolve no longer; their ids stay theirs)
    edits = []
    for kind, value in args.edits:
        if kind is None:
            if value in ent:
                sys.exit("--add-entity %r: the entity exists" % value)
            ent.append(value)
            edits.append((None, value))
        elif kind == "retire":
            if value in ent and value not in gone:
                retired_id = ent.index(value)
            elif value not in ent and value.isdigit() and int(value) < len(ent) and ent[int(value)] not in gone:
                retired_id = int(value)
            else:
                sys.exit("--remove-entity %r: unknown entity (or one retired earlier on the command line)" % value)
            gone.add(ent[retired_id])
            edits.append(("retire", retired_id))
        else:
            edits.append((kind, lookup_fact(value, ent, rel, gone)))
    reserve = len(ent) - num_known if args.entity_capacity is None else args.entity_capacity
    if len(ent) > num_known and not reserve:
        sys.exit("--add-entity needs --entity-capacity above 0")
    nested = resolve(ast.literal_eval(args.query), ent, rel, gone)
    assumed = [lookup_fact(fact, ent, rel, gone) for fact in args.assume]       # (the names known after every edit)
    among = {}
    if args.among or args.among_file:
        from ultra_amd.candidates import named_ids
        try:
            among = {"among": named_ids(ent, args.among, args.among_file)}
        except ValueError as exc:
            sys.exit("--among: %s" % exc)
    dev = torch.device("cuda:0")
    data = udata.load_triples_dir(args.data_root).to(dev)
    cfg = synthetic.default_model_cfg()
    cfg["entity_model_cfg"]["class"] = "QueryNBFNet"
    model = ultraquery.UltraQuery(models.Ultra(**cfg), logic=args.logic)
    if args.ckpt:
        state = torch.load(args.ckpt, map_location="cpu")
        model.load_state_dict(state["model"] if "model" in state else state)
    else:
        print("no --ckpt: randomly initialised weights, the answers mean nothing")
    model = model.to(dev).eval()
    qp = query_predict.QueryPredictor(model, data, k=args.k, batch_size=1, filtered=not args.unfiltered, entity_capacity=reserve,
                                      assume_capacity=max(8, len(assumed)))
    at = 0
    while at < len(edits):        # (runs of one kind go in one call)
        if edits[at][0] is None:
            (new_id,) = qp.add_entities(1).tolist()
            assert ent[new_id] == edits[at][1]
            print("entity %r added as id %d (%d of %d rows in use)" % (edits[at][1], new_id, qp.num_entities, qp.num_slots))
            at += 1
            continue
        if edits[at][0] == "retire":
            try:
                (took,) = qp.retire_entities(edits[at][1]).tolist()
            except ValueError as exc:
                sys.exit(str(exc))
            print("entity %r retired: %d fact(s) retracted (%d of %d entities retired)"
                  % (ent[edits[at][1]], took, qp.num_retired, qp.num_entities))
            at += 1
            continue
        end = at
        while end < len(edits) and edits[end][0] == edits[at][0]:
            end += 1
        ids = [list(column) for column in zip(*(fact for _, fact in edits[at:end]))]
        try:
            if edits[at][0]:
                held = qp.add_facts(*ids)
                print("%d fact(s) stated on top of the dataset%s" % (end - at, "" if held else " (folded into the graph)"))
            else:
                took = qp.remove_facts(*ids).tolist()
                print("%d fact(s) retracted from the dataset: %s edge(s) removed" % (end - at, " + ".join(str(n) for n in took)))
        except ValueError as exc:
            sys.exit(str(exc))
        at = end
    print(ultraquery.Query.from_nested(nested).to_readable())
    if among:
        print("candidates: the %d listed entities" % len(set(among["among"])))
    if assumed:
        among["assuming"] = torch.tensor(assumed, dtype=torch.long, device=dev)
        print("assuming %d fact(s) for this query only: nothing is stated" % len(assumed))
    try:
        return show(args, qp, nested, among, ent)
    except ValueError as exc:
        if not assumed:
            raise
        sys.exit(str(exc))      # (an assumed fact the predictor refuses: an inverse relation, a retired entity)


def show(args, qp, nested, among, ent):
    if args.above is not None:
        ptr, ids, scores, size = qp.answer_sets([nested], probability=args.above, **among)
        print("%d answers with probability above %g%s; predicted size of the set %d"
              % (int(ptr[1]), args.above, "" if args.unfiltered else ", entailed answers left out", int(size[0])))
        for i, (v, s) in enumerate(zip(ids.tolist(), scores.tolist())):
            print("%3d  %-40s %.6g" % (i + 1, ent[v], s))
        return
    ids, scores, count = qp.answers([nested], **among)
    print("top %d%s" % (int(count[0]), "" if args.unfiltered else ", entailed answers left out"))
    for i in range(int(count[0])):
        print("%3d  %-40s %.6g" % (i + 1, ent[int(ids[0, i])], float(scores[0, i])))


if __name__ == "__main__":
    main()
