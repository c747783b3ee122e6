"""Answer one link-prediction query on a dataset of triple files: the k entities the model predicts, with their scores.

    python tools/predict.py --data-root DIR [--ckpt FILE] --head NAME --relation NAME [--inverse] [-k 10] [--unfiltered] [--explain]

DIR holds train.txt / valid.txt / test.txt (`head relation tail` per line) and optionally entities.dict / relations.dict
(ultra_amd.data.load_triples_dir).  The query is (NAME, relation, ?); with --inverse it is (?, relation, NAME) and heads are
predicted.  Answers the dataset already states (in any split) are left out unless --unfiltered.  --ckpt: an ULTRA
checkpoint (a state dict, or a dict with the state under "model"); without it the weights are randomly initialised, and the
tool says so.  --explain: under every answer, the paths the model's score rests on (Predictor.explain_tails /
explain_heads) with their weights; a relation walked against its direction is printed as NAME^-1.
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
    ap.add_argument("--head", required=True, help="the known entity of the query (the tail with --inverse)")
    ap.add_argument("--relation", required=True)
    ap.add_argument("--inverse", action="store_true", help="predict heads of (?, relation, NAME)")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--unfiltered", action="store_true")
    ap.add_argument("--explain", action="store_true", help="print the top paths behind every answer")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/predict.py needs a GPU: the engine has no CPU path")
    from ultra_amd import data as udata
    from ultra_amd import models, predict, synthetic
    ent, rel = udata.read_vocab(args.data_root)
    for name, vocab, what in ((args.head, ent, "entity"), (args.relation, rel, "relation")):
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
    predictor = predict.Predictor(model, data, k=args.k, batch_size=1, filtered=not args.unfiltered)
    anchor = torch.tensor([ent.index(args.head)], device=dev)
    relation = torch.tensor([rel.index(args.relation)], device=dev)
    why = None
    if args.explain:
        ids, scores, count, why = (predictor.explain_heads if args.inverse else predictor.explain_tails)(anchor, relation)
    else:
        ids, scores, count = (predictor.heads if args.inverse else predictor.tails)(anchor, relation)
    query = "(?, %s, %s)" % (args.relation, args.head) if args.inverse else "(%s, %s, ?)" % (args.head, args.relation)
    print("%s: top %d%s" % (query, int(count[0]), "" if args.unfiltered else ", known answers left out"))
    for i in range(int(count[0])):
        print("%3d  %-40s %.6g" % (i + 1, ent[int(ids[0, i])], float(scores[0, i])))
        if why is not None:
            for path, weight in zip(*why[0][i]):
                print("       %+.4g  %s" % (weight, format_path(path, ent, rel)))


if __name__ == "__main__":
    main()
