"""Child process of tests/test_gpu_tree_search_shapes.py: a trajectory tree search whose plan stays under 64 KiB and the table's largest
plan (a few bytes under MG_TREE_LDS_MAX) on ONE fresh context, in the order given on the command line.  The large-LDS opt-in of the
kernel is made at the first plan beyond 64 KiB, so each order needs a process that has launched neither.  Prints the records.
usage: python tree_search_optin_child.py feature|kd small-first|large-first"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import tree_search_cases as sc  # noqa: E402
from morphablegraphs_amd import _capi  # noqa: E402
from morphablegraphs_amd.cluster_tree import search_on_device  # noqa: E402
from test_gpu_tree_search_shapes import Search  # noqa: E402


def main(kind, order):
    ctx = _capi.Context(0)
    prim = _capi.Primitive(ctx, sc.model("tiny"))
    families = ("small", "last_under_limit") if order == "small-first" else ("last_under_limit", "small")
    for family in families:
        r = sc.BY_NAME["%s-%s-s0" % (family, kind)]
        _, kf, trajs, leaves = sc.row_inputs(r)
        s = Search(prim, kind, kf, trajs, leaves, r["align"])
        plan = s.plan(r["n_cand"])
        assert plan["lds_opt_in"] == (family == "last_under_limit") and not plan["refused"], plan
        rec = search_on_device([s.triple()], r["n_cand"])
        assert rec["flags"][0] == 0, rec
        print("record %s %s" % (family, rec.tobytes().hex()))
        s.close()
    prim.close()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
