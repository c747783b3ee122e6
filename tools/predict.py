"""Answer one link-prediction query on a dataset of triple files: the k entities the model predicts, with their scores.

    python tools/predict.py --data-root DIR [--ckpt FILE] --head NAME --relation NAME [--inverse] [-k 10] [--unfiltered] [--explain [--no-compact]]
                            [--add-fact H R T]... [--remove-fact H R T]... [--entity-capacity M] [--add-entity NAME]...
                            [--relation-capacity K] [--add-relation NAME]... [--live-relation-graph] [--remove-entity NAME]...
                            [--among NAME [NAME ...]] [--among-file FILE] [--assume H R T]...
    python tools/predict.py --data-root DIR [--ckpt FILE] --verify (--head NAME --relation NAME --tail NAME | --triples FILE) [--inverse]
    python tools/predict.py --data-root DIR [--ckpt FILE] --propose RELATION [--propose-k K] [--min-score X] [--among-file FILE] [--inverse]

DIR holds train.txt / valid.txt / test.txt (`head relation tail` per line) and optionally entities.dict / relations.dict
(ultra_amd.data.load_triples_dir).  The query is (NAME, relation, ?); with --inverse it is (?, relation, NAME) and heads are
predicted.  Answers the dataset already states (in any split) are left out unless --unfiltered.  --ckpt: an ULTRA
checkpoint (a state dict, or a dict with the state under "model"); without it the weights are randomly initialised, and the
tool says so.  --explain: under every answer, the paths the model's score rests on (Predictor.explain_tails /
explain_heads) with their weights; a relation walked against its direction is printed as NAME^-1.

--add-fact H R T (repeatable) states a fact between known entities before the query is answered (Predictor.add_facts): the
graph served is the dataset's plus these facts, and their tails and heads count as known answers.  --remove-fact H R T
(repeatable) retracts a fact before the query is answered (Predictor.remove_facts): every edge that states it leaves the graph
served and the known answers, so its tail can be predicted again.  Both kinds are applied in command-line order.

--add-entity NAME (repeatable) introduces an entity the dataset does not know (Predictor.add_entities): it takes one of the rows
reserved by --entity-capacity M (default: as many as there are --add-entity options), costs no plan and no capture, and from then
on NAME can be used by the --add-fact / --remove-fact options that FOLLOW it on the command line and by --head; answers print it
by its name.  It is applied in command-line order with the fact options.

--remove-entity NAME (repeatable) takes an entity out of the graph served before the query is answered
(Predictor.remove_entities): every fact that names it is retracted and the entity is retired -- never an answer,
never counted among the candidates.  It is applied in command-line order with the other edit options, and NAME no longer
resolves in the options that FOLLOW it on the command line, nor in --head / --tail / --triples.

--add-relation NAME (repeatable) introduces a relation type the dataset does not know (Predictor.add_relations): it takes one of
the slots reserved by --relation-capacity K (default: as many as there are --add-relation options) and costs no plan, no relation
graph and no capture.  The --add-relation options are applied in command-line order BEFORE every --add-fact / --remove-fact, so
NAME can be used by all of them and by --relation.

--live-relation-graph keeps the relation graph current in place (Predictor(live_relation_graph=True)): a fact that
changes relation-graph cells -- every first fact through an --add-relation -- then costs no relation-graph plan and no new
capture.  The answers are the same.  Needs a relation model of sum / DistMult layers (the default configuration's).

--among NAME [NAME ...] and --among-file FILE (entity names, one per line; both may be given, the set is their union) restrict
the candidates to a set (Predictor.tails(among=)): only these entities are ranked -- a shortlist, or the entities
of a type -- and with --verify the fact is ranked among them.  An unknown name is an error that names it; a name introduced by
--add-entity may be listed, and an entity retired by --remove-entity is simply absent.

--assume H R T (repeatable) answers the query as if the fact were true WITHOUT stating it (Predictor.tails(assuming=), DESIGN.md
32): the graph served, the delta and the known answers of later queries stay what they were; an assumed tail of the query's own
(head, relation) is left out of its answers.  The names are those known after every edit option.  Not with --verify / --explain.

--propose RELATION asks which facts of RELATION are most likely MISSING (Predictor.propose_tails): every entity in
use is a head, and the --propose-k (default 10) best triples (head, RELATION, tail) that the dataset does not state are printed
with their scores, best first; equal scores in the order of (head, tail) ids.  --min-score X keeps only triples whose logit
exceeds X; --among / --among-file restrict the TAILS to a set; the edit options apply first, as for a query.  With --inverse the
heads are ranked for every tail (Predictor.propose_heads).  Not with --verify / --explain / --assume, and --head / --relation /
--tail / --triples / -k are refused beside it.

--verify judges facts the dataset may already state: every (head, relation, tail) -- one from the command line, or the
`head relation tail` lines of FILE -- is scored on the graph WITHOUT itself and its inverse edge (Predictor.verify_tails; with
--inverse the head is the answer judged, Predictor.verify_heads) and printed with its score, its filtered rank and the number
of candidates it was ranked among.  With --add-fact / --remove-fact / --add-entity the facts are judged on the EDITED graph -- a
fact that was just stated is judged without itself -- and without --add-entity the edits stay a delta beside the cached plan
(with reserved rows they are folded into the graph first).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def format_path(path, ent, rel):
    """A path [(h, t, r), ...] with the names of read_vocab; r >= len(rel) is the inverse of relation r - len(rel)."""
    out = ent[path[0][0]]
    for _, t, r in path:
        out += " -[%s]-> %s" % (rel[r] if r < len(rel) else rel[r - len(rel)] + "^-1", ent[t])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-root", required=True)
    ap.add_argument("--ckpt")
    ap.add_argument("--head", help="the known entity of the query (the tail with --inverse)")
    ap.add_argument("--relation")
    ap.add_argument("--verify", action="store_true", help="judge stated facts on the graph without themselves")
    ap.add_argument("--tail", help="--verify: the tail of the fact")
    ap.add_argument("--triples", help="--verify: a file of `head relation tail` lines")
    ap.add_argument("--inverse", action="store_true", help="predict heads of (?, relation, NAME)")
    ap.add_argument("-k", type=int, default=None, help="answers of the query (default 10)")
    ap.add_argument("--unfiltered", action="store_true")
    ap.add_argument("--explain", action="store_true", help="print the top paths behind every answer")
    ap.add_argument("--no-compact", action="store_true",
                    help="--explain on a graph that holds edits: explain on the delta, do not fold it into the graph first")
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
    ap.add_argument("--add-relation", action="append", default=[], metavar="NAME",
                    help="introduce a new relation type before the facts and the query; repeatable")
    ap.add_argument("--relation-capacity", type=int, default=None, metavar="K",
                    help="slots reserved for new relation types (default: the number of --add-relation options)")
    ap.add_argument("--live-relation-graph", action="store_true",
                    help="keep the relation graph current in place: no relation-graph plan, no new capture for an edit")
    ap.add_argument("--assume", nargs=3, action="append", default=[], metavar=("H", "R", "T"),
                    help="answer as if the fact (H, R, T) were true, without stating it; repeatable")
    ap.add_argument("--propose", metavar="RELATION", help="the most likely missing facts of RELATION, over all heads")
    ap.add_argument("--propose-k", type=int, default=10, metavar="K", help="--propose: how many triples")
    ap.add_argument("--min-score", type=float, default=None, metavar="X", help="--propose: only triples whose logit exceeds X")
    ap.add_argument("--among", nargs="+", metavar="NAME", help="rank only these entities (a shortlist, a type)")
    ap.add_argument("--among-file", metavar="FILE", help="... the entity names of FILE, one per line")
    ap.set_defaults(edits=[])
    args = ap.parse_args(argv)
    if args.k is None and not args.propose:
        args.k = 10
    if args.propose:
        if args.verify or args.explain or args.assume:
            ap.error("--propose goes alone: not with --verify, --explain or --assume")
        given = [name for name, value in (("--head", args.head), ("--relation", args.relation), ("--tail", args.tail),
                                          ("--triples", args.triples), ("-k", args.k)) if value is not None]
        if given:
            ap.error("--propose takes no %s: every entity in use is a head, the relation is --propose's and the number of "
                     "triples is --propose-k" % " / ".join(given))
        if not 1 <= args.propose_k <= 256:
            ap.error("--propose-k must lie in [1, 256]")
    elif args.verify:
        if not (args.triples or (args.head and args.relation and args.tail)):
            ap.error("--verify takes --head, --relation and --tail, or --triples FILE")
    elif not (args.head and args.relation):
        ap.error("--head and --relation are required")
    if not torch.cuda.is_available():
        sys.exit("tools/predict.py needs a GPU: the engine has no CPU path")
    from ultra_amd import data as udata
    from ultra_amd import models, predict, synthetic
    ent, rel = udata.read_vocab(args.data_root)
    facts = None
    if args.verify:
        facts = [tuple(line.split()) for line in open(args.triples) if line.strip()] if args.triples \
            else [(args.head, args.relation, args.tail)]
        if any(len(f) != 3 for f in facts):
            sys.exit("--triples: every line is `head relation tail`")
    new_names = [name for kind, name in args.edits if kind is None]
    if args.entity_capacity is not None and args.entity_capacity < 0:
        sys.exit("--entity-capacity must not be negative")
    if args.relation_capacity is not None and args.relation_capacity < 0:
        sys.exit("--relation-capacity must not be negative")
    rel = list(rel)
    num_old_relations = len(rel)
    for name in args.add_relation:      # (applied before the facts: usable by every one of them and by --relation)
        if name in rel:
            sys.exit("--add-relation %r: the relation exists" % name)
        rel.append(name)
    known = set(ent)        # (grows along the command line: a name can be used after its --add-entity)
    checks = []
    for kind, value in args.edits:
        if kind is None:
            if value in known:
                sys.exit("--add-entity %r: the entity exists" % value)
            known.add(value)
        elif kind == "retire":
            if value not in known:
                sys.exit("--remove-entity %r: unknown entity (or one retired earlier on the command line)" % value)
            known.discard(value)
        else:
            checks.append((value, set(known)))
    if args.propose:
        if args.propose not in rel:
            sys.exit("unknown relation %r" % args.propose)
    else:
        for triple in (facts if facts is not None else [(args.head, args.relation, args.head)]):
            checks.append((triple, known))
    if args.assume and (args.verify or args.explain):
        sys.exit("--assume goes with the plain query: not with --verify or --explain")
    for triple in args.assume:          # (judged against the names known after every edit)
        checks.append((tuple(triple), known))
    for (h_name, r_name, t_name), names in checks:
        for name, vocab, what in ((h_name, names, "entity"), (r_name, rel, "relation"), (t_name, names, "entity")):
            if name not in vocab:
                sys.exit("unknown %s %r" % (what, name))
    dev = torch.device("cuda:0")
    data = udata.load_triples_dir(args.data_root).to(dev)
    model = models.Ultra(**synthetic.default_model_cfg())
    if args.ckpt:
        state = torch.load(args.ckpt, map_location="cpu")
        model.load_state_dict(state["model"] if "model" in state else state)
    else:
        print("no --ckpt: randomly initialised weights, the answers mean nothing")
    model = model.to(dev).eval()
    reserve = len(new_names) if args.entity_capacity is None else args.entity_capacity
    rel_reserve = len(args.add_relation) if args.relation_capacity is None else args.relation_capacity
    if facts is not None:
        predictor = predict.Predictor(model, data, batch_size=min(8, len(facts)), entity_capacity=reserve,
                                      relation_capacity=rel_reserve, live_relation_graph=args.live_relation_graph)
    elif args.propose:
        predictor = predict.Predictor(model, data, k=args.propose_k, batch_size=8, filtered=not args.unfiltered,
                                      entity_capacity=reserve, relation_capacity=rel_reserve,
                                      live_relation_graph=args.live_relation_graph)
    else:
        predictor = predict.Predictor(model, data, k=args.k, batch_size=1, filtered=not args.unfiltered, entity_capacity=reserve,
                                      relation_capacity=rel_reserve, live_relation_graph=args.live_relation_graph,
                                      assume_capacity=max(8, len(args.assume)))
    for name in args.add_relation:
        if not rel_reserve:
            sys.exit("--add-relation needs --relation-capacity above 0")
        (new_id,) = predictor.add_relations(1).tolist()
        assert rel[new_id] == name and new_id >= num_old_relations
        print("relation %r added as id %d (%d of %d slots in use)"
              % (name, new_id, predictor.num_direct_relations, predictor.num_relation_slots))
    ent = list(ent)
    at = 0
    while at < len(args.edits):        # (runs of one kind go in one call)
        if args.edits[at][0] is None:
            if not reserve:
                sys.exit("--add-entity needs --entity-capacity above 0")
            (new_id,) = predictor.add_entities(1).tolist()
            assert new_id == len(ent)
            ent.append(args.edits[at][1])
            print("entity %r added as id %d (%d of %d rows in use)" % (ent[-1], new_id, predictor.num_entities, predictor.num_slots))
            at += 1
            continue
        if args.edits[at][0] == "retire":
            name = args.edits[at][1]
            (took,) = predictor.remove_entities(ent.index(name)).tolist()
            print("entity %r retired: %d fact(s) retracted (%d of %d entities retired)"
                  % (name, took, predictor.num_retired, predictor.num_entities))
            at += 1
            continue
        end = at
        while end < len(args.edits) and args.edits[end][0] == args.edits[at][0]:
            end += 1
        run = [f for _, f in args.edits[at:end]]
        ids = [[vocab.index(f[i]) for f in run] for i, vocab in ((0, ent), (1, rel), (2, ent))]
        if args.edits[at][0]:
            held = predictor.add_facts(*ids)
            print("%d fact(s) stated on top of the dataset%s" % (len(run), "" if held else " (folded into the graph)"))
        else:
            took = predictor.remove_facts(*ids).tolist()
            print("%d fact(s) retracted from the dataset: %s edge(s) removed" % (len(run), " + ".join(str(n) for n in took)))
        at = end
    among = {}
    if args.among or args.among_file:
        from ultra_amd.candidates import named_ids
        try:
            among = {"among": named_ids(ent, args.among, args.among_file)}
        except ValueError as exc:
            sys.exit("--among: %s" % exc)
        print("candidates: the %d listed entities" % len(set(among["among"])))
    if facts is not None:
        # (the edits above stay a delta beside the cached plan: every fact is judged on the edited graph without itself)
        h, r, t = (torch.tensor([vocab.index(f[i]) for f in facts], device=dev) for i, vocab in ((0, ent), (1, rel), (2, ent)))
        score, rank, num_negative = (predictor.verify_heads if args.inverse else predictor.verify_tails)(h, r, t, **among)
        print("%s judged on the graph without the fact itself: score, filtered rank / candidates"
              % ("heads" if args.inverse else "tails"))
        for f, s, k, n in zip(facts, score.tolist(), rank.tolist(), num_negative.tolist()):
            print("%-28s %-24s %-28s %12.6g  %6d / %d" % (f[0], f[1], f[2], s, k, n + 1))
        return
    if args.propose:
        propose = predictor.propose_heads if args.inverse else predictor.propose_tails
        try:
            heads, tails, scores, count = propose(rel.index(args.propose), min_score=args.min_score, **among)
        except ValueError as exc:
            sys.exit("--propose: %s" % exc)
        print("(?, %s, ?): the %d most likely missing facts over all %s%s%s"
              % (args.propose, int(count), "tails" if args.inverse else "heads",
                 "" if args.unfiltered else ", stated facts left out",
                 "" if args.min_score is None else ", logit above %g" % args.min_score))
        for i in range(int(count)):
            print("%3d  %-28s %-24s %-28s %.6g" % (i + 1, ent[int(heads[i])], args.propose, ent[int(tails[i])], float(scores[i])))
        return
    anchor = torch.tensor([ent.index(args.head)], device=dev)
    relation = torch.tensor([rel.index(args.relation)], device=dev)
    why = None
    if args.explain:
        ids, scores, count, why = (predictor.explain_heads if args.inverse else predictor.explain_tails)(
            anchor, relation, compact=not args.no_compact, **among)
    else:
        if args.assume:
            among["assuming"] = torch.tensor([[vocab.index(f[i]) for i, vocab in ((0, ent), (1, rel), (2, ent))]
                                              for f in args.assume], device=dev)
            print("assuming %d fact(s) for this query only: nothing is stated" % len(args.assume))
        ids, scores, count = (predictor.heads if args.inverse else predictor.tails)(anchor, relation, **among)
    query = "(?, %s, %s)" % (args.relation, args.head) if args.inverse else "(%s, %s, ?)" % (args.head, args.relation)
    print("%s: top %d%s" % (query, int(count[0]), "" if args.unfiltered else ", known answers left out"))
    for i in range(int(count[0])):
        print("%3d  %-40s %.6g" % (i + 1, ent[int(ids[0, i])], float(scores[0, i])))
        if why is not None:
            for path, weight in zip(*why[0][i]):
                print("       %+.4g  %s" % (weight, format_path(path, ent, rel)))


if __name__ == "__main__":
    main()
