"""Answer one complex logical query on a dataset of triple files: the k entities the model predicts, with their scores.

    python tools/query_predict.py --data-root DIR [--ckpt FILE] --query "(('e1', ('r1',)), ('e2', ('r2', -2)))" [-k 10]
                                  [--logic product] [--unfiltered]

DIR holds train.txt / valid.txt / test.txt (`head relation tail` per line) and optionally entities.dict / relations.dict
(ultra_amd.data.load_triples_dir).  The query is a BetaE nested tuple (ultra_amd.ultraquery.Query.from_nested): a pair
(anchor, (relation, ...)) projects the anchor -- an entity, or a nested query -- along the chain, where -2 negates; any other
tuple intersects its branches, or unites them when it ends with (-1,).  Entities and relations are names of the
vocabularies or integer ids.  Answers the graph already entails (the symbolic traversal of the query) are left out unless
--unfiltered.  --ckpt: an UltraQuery checkpoint (a state dict, or a dict with the state under "model"); without it the
weights are randomly initialised, and the tool says so.
"""
import argparse
import ast
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def resolve(nested, ent, rel):
    """The nested tuple with every name replaced by its id (the shapes are those of Query.nested_to_postfix)."""
    def lookup(name, vocab, what):
        if isinstance(name, int):
            return name
        if name not in vocab:
            sys.exit("unknown %s %r" % (what, name))
        return vocab.index(name)
    if len(nested) == 2 and not isinstance(nested[1][-1], tuple):
        anchor, chain = nested
        anchor = resolve(anchor, ent, rel) if isinstance(anchor, tuple) else lookup(anchor, ent, "entity")
        return (anchor, tuple(lookup(step, rel, "relation") for step in chain))
    return tuple(branch if branch == (-1,) else resolve(branch, ent, rel) for branch in nested)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-root", required=True)
    ap.add_argument("--ckpt")
    ap.add_argument("--query", required=True, help="a BetaE nested tuple of names or ids")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--logic", default="product", choices=["product", "godel", "lukasiewicz"])
    ap.add_argument("--unfiltered", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/query_predict.py needs a GPU: the engine has no CPU path")
    from ultra_amd import data as udata
    from ultra_amd import models, query_predict, synthetic, ultraquery
    ent, rel = udata.read_vocab(args.data_root)
    nested = resolve(ast.literal_eval(args.query), ent, rel)
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
    qp = query_predict.QueryPredictor(model, data, k=args.k, batch_size=1, filtered=not args.unfiltered)
    ids, scores, count = qp.answers([nested])
    print(ultraquery.Query.from_nested(nested).to_readable())
    print("top %d%s" % (int(count[0]), "" if args.unfiltered else ", entailed answers left out"))
    for i in range(int(count[0])):
        print("%3d  %-40s %.6g" % (i + 1, ent[int(ids[0, i])], float(scores[0, i])))


if __name__ == "__main__":
    main()
