"""Reads the reference's pickled cluster trees (`<primitive>_cluster_tree.pck` in a model zip, utilities/zip_io.py:204-213;
written by construction/cluster_tree_builder.py:235-262 with pickle.HIGHEST_PROTOCOL, or by Python 2) without running
anything the file names beyond an allow-list.

The Unpickler resolves only
  * the reference's space_partitioning classes ClusterTree, ClusterTreeNode, KDTreeWrapper, KDTree, Node and
    FeatureClusterTree, under any module path that ends in `space_partitioning.<their file>`; they become plain stand-ins
    that only hold the pickled attributes;
  * NumPy's array and scalar reconstructors (multiarray._reconstruct, multiarray.scalar, numeric._frombuffer under
    numpy.core or numpy._core; numpy.dtype, numpy.ndarray);
  * copyreg / copy_reg._reconstructor and builtins / __builtin__.object;
  * _codecs.encode (how Python 3 writes bytes -- an array's buffer -- in protocols 0 to 2);
and raises pickle.UnpicklingError for every other global before anything is called.  Python 2 pickles load with
encoding="latin1".  A ClusterTree becomes a kd_cluster_tree.HipClusterTree, a FeatureClusterTree a
cluster_tree.HipFeatureClusterTree (its _mean, _indices and _children as the JSON layout's mean, indices and children)."""
import codecs
import copyreg
import importlib
import io
import pickle

import numpy as np

from .cluster_tree import HipFeatureClusterTree
from .kd_cluster_tree import HipClusterTree


class _StandIn(object):
    """An object of one of the reference's classes: its pickled attributes and nothing else."""

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        if isinstance(state, tuple) and len(state) == 2:    # (dict, slots)
            state = dict(state[0] or {}, **(state[1] or {}))
        if not isinstance(state, dict):
            raise pickle.UnpicklingError("cluster tree pickle: a %s with state of type %s" % (type(self).__name__, type(state).__name__))
        self.__dict__.update(state)


def _stand_in(name):
    return type(name, (_StandIn,), {"__module__": __name__})


# file of space_partitioning -> {class name: stand-in}
_REFERENCE = {
    "cluster_tree": {"ClusterTree": _stand_in("ClusterTree")},
    "cluster_tree_node": {"ClusterTreeNode": _stand_in("ClusterTreeNode")},
    "kdtree_wrapper_node": {"KDTreeWrapper": _stand_in("KDTreeWrapper")},
    "kdtree": {"KDTree": _stand_in("KDTree"), "Node": _stand_in("Node")},
    "feature_cluster_tree": {"FeatureClusterTree": _stand_in("FeatureClusterTree")},
}
ClusterTree = _REFERENCE["cluster_tree"]["ClusterTree"]
FeatureClusterTree = _REFERENCE["feature_cluster_tree"]["FeatureClusterTree"]


def _numpy_module(suffix):
    for base in ("numpy._core", "numpy.core"):
        try:
            return importlib.import_module(base + "." + suffix)
        except ImportError:
            continue
    raise ImportError("numpy has no %s module" % suffix)


_NUMPY = {("multiarray", "_reconstruct"), ("multiarray", "scalar"), ("numeric", "_frombuffer")}


class SafeUnpickler(pickle.Unpickler):
    """pickle.Unpickler whose find_class resolves the allow-list alone."""

    def find_class(self, module, name):
        parts = module.split(".")
        if len(parts) >= 2 and parts[-2] == "space_partitioning" and name in _REFERENCE.get(parts[-1], {}):
            return _REFERENCE[parts[-1]][name]
        if parts[0] == "numpy":
            if module == "numpy" and name in ("dtype", "ndarray"):
                return getattr(np, name)
            if len(parts) == 3 and parts[1] in ("core", "_core") and (parts[2], name) in _NUMPY:
                return getattr(_numpy_module(parts[2]), name)
        if module in ("copyreg", "copy_reg") and name == "_reconstructor":
            return copyreg._reconstructor
        if module in ("builtins", "__builtin__") and name == "object":
            return object
        if module == "_codecs" and name == "encode":
            return codecs.encode
        raise pickle.UnpicklingError("cluster tree pickle: global %s.%s is not allowed" % (module, name))


def unpickle(path_or_bytes):
    """The pickled object with stand-ins for the reference's classes (UnpicklingError for anything outside the allow-list)."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        f = io.BytesIO(bytes(path_or_bytes))
    else:
        f = open(path_or_bytes, "rb")
    with f:
        return SafeUnpickler(f, encoding="latin1").load()


def _feature_tree_json(tree):
    """A FeatureClusterTree stand-in as the JSON layout HipFeatureClusterTree.from_json reads (iteratively)."""
    def node_dict(node):
        if not isinstance(node, FeatureClusterTree) or not hasattr(node, "_mean"):
            raise ValueError("cluster tree: a node that is not a FeatureClusterTree with a mean")
        idx = getattr(node, "_indices", None)
        return {"mean": np.asarray(node._mean, dtype=np.float64).tolist(), "indices": None if idx is None else [int(i) for i in idx],
                "children": []}
    root = node_dict(tree)
    stack, seen = [(tree, root)], {id(tree)}
    while stack:
        node, d = stack.pop()
        for c in getattr(node, "_children", None) or []:
            if id(c) in seen:
                raise ValueError("cluster tree: every node but the root needs exactly one parent")
            seen.add(id(c))
            cd = node_dict(c)
            d["children"].append(cd)
            stack.append((c, cd))
    return {"data": np.asarray(tree.data, dtype=np.float64), "features": getattr(tree, "_features", None),
            "options": getattr(tree, "_options", None), "root": root}


def tree_from_object(obj, n_spatial=None):
    """HipClusterTree or HipFeatureClusterTree of an unpickled tree."""
    if isinstance(obj, ClusterTree):
        return HipClusterTree.from_reference(obj, n_spatial)
    if isinstance(obj, FeatureClusterTree):
        return HipFeatureClusterTree.from_json(_feature_tree_json(obj), n_spatial)
    raise ValueError("cluster tree pickle: a %s, not a ClusterTree or FeatureClusterTree" % type(obj).__name__)


def load_cluster_tree_pickle(path_or_bytes, n_spatial=None):
    """A `_cluster_tree.pck` (a path or its bytes) as a HipClusterTree or HipFeatureClusterTree."""
    return tree_from_object(unpickle(path_or_bytes), n_spatial)
