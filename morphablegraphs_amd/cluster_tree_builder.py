"""Building the reference's two space partitionings on the device: the k-means / KD ClusterTree (space_partitioning/
cluster_tree.py:96-100, cluster_tree_node_builder.py:63-170, kdtree.py:39-73) and the FeatureClusterTree
(feature_cluster_tree.py:61-98, clustering.py:83-129), and ClusterTreeBuilder (construction/cluster_tree_builder.py:120-301)
around them.

The reference builds depth first and calls sklearn's KMeans once per node.  Here the construction is restated level by
level: every node of a level that the reference would cluster is a segment of one row permutation, and ONE call of
mg_kmeans_segments (sklearn's KMeans(algorithm="lloyd") semantics, _capi.kmeans_segments) clusters all of them; a stable
partition by (segment, label) -- rows keep their parent's order inside a cluster, the order in which the reference appends
`original_index` -- gives the next level.  Given the same k-means labels the tree is the reference's tree, node for node:
  * ClusterTree: a node of n rows is subdivided if n > n_subdivisions > 1; its non-empty clusters become cluster nodes while
    depth < max_level (or without KD trees), KD-tree wrappers after that; otherwise it is a leaf holding one KD tree of its
    rows, or (use_kd_tree False) a node with one single-row child per row, whose mean is that row.  k-means sees
    data[:, :dim], the KD trees hold full rows; the KD trees (axis depth % dim, stable sort, median len // 2) are built for
    all leaves at once, one np.lexsort per KD depth.  Departure: the reference hands its root indices None, so a root that
    is itself a leaf would wrap data[None] -- every row as ONE KD point; here the root holds its rows like any node.
  * FeatureClusterTree: clustering on `features`, means np.average of `data` (of features with use_feature_mean); the root's
    indices are None but it clusters every row; below MAX_SIMILARITY_CHECK = 10 members identical feature rows become
    singletons (all_equal); a node of more than n_subdivisions members is clustered, its empty clusters removed by the
    reference's remove-while-iterating loop (two adjacent empty clusters leave one behind), and a single cluster equal to
    the node's indices -- or a remaining cluster equal to them -- becomes one singleton child per member; a node of 2 ..
    n_subdivisions members gets one singleton child per member.
Node means are np.mean / np.average of the node's rows exactly as the reference computes them (bit for bit).

Random numbers: the device's k-means++ draws from Philox keyed by (seed, node id, run); a node's id is a hash of its path
(the parent's id and the child's position), so the tree does not depend on how nodes are batched.  Replaying the reference's
np.random stream is out of scope; parity with the reference is through given initial centres (`init`).

Writers: the reference's pickle of a ClusterTree (save_to_file_pickle: its module and class paths, the attributes the
loaders read) and the reference's JSON of a FeatureClusterTree (save_to_json_file) or its pickle.
"""
import json
import pickle
import sys
import types
import uuid

import numpy as np

from . import _capi
from .cluster_tree import HipFeatureClusterTree
from .kd_cluster_tree import HipClusterTree

MG_TREE_MAX_DEPTH, MG_KD_MAX_DEPTH = _capi.MG_TREE_MAX_DEPTH, _capi.MG_KD_MAX_DEPTH
MAX_SIMILARITY_CHECK = 10          # feature_cluster_tree.py:36
CLUSTERING_METHOD_KMEANS = 0       # clustering.py:32
_MASK = (1 << 64) - 1


def child_node_id(parent_id, position):
    """The id of a node's child at `position` (0-based) among its children: splitmix64 of the parent's id and the position.
    The root's id is 0."""
    z = (int(parent_id) * 0x9E3779B97F4A7C15 + int(position) + 1) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


class DeviceKMeans(object):
    """mg_kmeans_segments over one points table uploaded once: kmeans(seg_begin, rows, node_ids) -> a label per position of
    rows.  init: None (k-means++ on the device) or a callable members -> (k, dim) initial centres (then n_init is 1).  The
    per-segment centres, inertia and iteration counts of the last call are kept in .last."""

    def __init__(self, ctx, points, n_clusters, seed=0, n_init=1, max_iter=300, tol=1e-4, init=None):
        self.ctx = ctx
        pts = np.ascontiguousarray(points, dtype=np.float64)
        self.n_rows, self.dim = pts.shape
        self.k, self.seed, self.n_init, self.max_iter, self.tol, self.init = int(n_clusters), int(seed), int(n_init), int(max_iter), float(tol), init
        self.points_dev = ctx.upload(pts)
        self.calls, self.last = 0, None

    def __call__(self, seg_begin, rows, node_ids):
        seg_begin = np.asarray(seg_begin, dtype=np.int64)
        init = None
        if self.init is not None:
            init = np.stack([np.asarray(self.init(rows[seg_begin[s]:seg_begin[s + 1]]), dtype=np.float64).reshape(self.k, self.dim)
                             for s in range(len(seg_begin) - 1)])
        labels, centres, inertia, n_iter = _capi.kmeans_segments(self.ctx, self.points_dev, self.n_rows, self.dim, seg_begin, rows, self.k,
                                                                 1 if init is not None else self.n_init, init, node_ids, self.seed,
                                                                 self.max_iter, self.tol)
        self.calls += 1
        self.last = {"centres": centres, "inertia": inertia, "n_iter": n_iter}
        return labels

    def close(self):
        if self.points_dev is not None:
            self.points_dev.free()
        self.points_dev = None


def _cluster_level(kmeans, k, members, node_ids):
    """One batched k-means over the nodes `members` (arrays of rows): per node the k groups of its rows by label, each in
    the parent's order (a stable partition)."""
    if not members:
        return []
    sizes = np.array([len(m) for m in members], dtype=np.int64)
    seg_begin = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate(members).astype(np.int64)
    if k == 1:
        labels = np.zeros(len(rows), dtype=np.int64)
    else:
        labels = np.asarray(kmeans(seg_begin, rows, np.asarray(node_ids, dtype=np.uint64)), dtype=np.int64)
    key = np.repeat(np.arange(len(members), dtype=np.int64), sizes) * k + labels
    perm = np.argsort(key, kind="stable")
    ordered = rows[perm]
    counts = np.bincount(key, minlength=len(members) * k).reshape(len(members), k)
    bounds = np.concatenate([[0], np.cumsum(counts.ravel())])
    return [[ordered[bounds[s * k + j]:bounds[s * k + j + 1]] for j in range(k)] for s in range(len(members))]


def _kd_forest(data, trees, dim):
    """KD trees (kdtree.py:39-73) over the row lists `trees`, all at once, one stable lexsort per KD depth.  Returns the
    tables in the order HipClusterTree.from_reference flattens them (tree after tree, each breadth first): point rows,
    left, right, inner, and every tree's root index."""
    if not trees:
        e = np.zeros(0, dtype=np.int32)
        return np.zeros(0, dtype=np.int64), e, e, e, e
    sizes = np.array([len(t) for t in trees], dtype=np.int64)
    M = np.concatenate(trees).astype(np.int64)
    b = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    e = b + sizes
    tree = np.arange(len(trees), dtype=np.int64)
    parent = np.full(len(trees), -1, dtype=np.int64)
    side = np.zeros(len(trees), dtype=np.int64)
    rows, tree_of, depth_of, seq_of, inner, links = [], [], [], [], [], []
    n_tmp, depth = 0, 0
    while len(b):
        if depth > MG_KD_MAX_DEPTH:
            raise ValueError("cluster tree build: a KD tree deeper than %d levels (MG_KD_MAX_DEPTH)" % MG_KD_MAX_DEPTH)
        lengths = e - b
        total = int(lengths.sum())
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        idx = np.repeat(b - starts, lengths) + np.arange(total)
        seg = np.repeat(np.arange(len(b)), lengths)
        order = np.lexsort((data[M[idx], depth % dim], seg))       # list.sort(key=itemgetter(axis)) per node: stable
        M[idx] = M[idx][order]
        m = b + lengths // 2
        ids = n_tmp + np.arange(len(b))
        n_tmp += len(b)
        rows.append(M[m])
        tree_of.append(tree)
        depth_of.append(np.full(len(b), depth))
        seq_of.append(np.arange(len(b)))
        inner.append((lengths > 1).astype(np.int32))
        links.append((parent, side, ids))
        # children: left [b, m) then right [m + 1, e) of every node, in order
        nb = np.stack([b, m + 1], axis=1).ravel()
        ne = np.stack([m, e], axis=1).ravel()
        keep = ne > nb
        parent = np.repeat(ids, 2)[keep]
        side = np.tile([0, 1], len(b))[keep]
        tree = np.repeat(tree, 2)[keep]
        b, e = nb[keep], ne[keep]
        depth += 1
    rows, tree_of, depth_of, seq_of, inner = (np.concatenate(x) for x in (rows, tree_of, depth_of, seq_of, inner))
    left, right = np.full(n_tmp, -1, dtype=np.int64), np.full(n_tmp, -1, dtype=np.int64)
    for par, sd, ids in links[1:]:
        left[par[sd == 0]] = ids[sd == 0]
        right[par[sd == 1]] = ids[sd == 1]
    order = np.lexsort((seq_of, depth_of, tree_of))        # breadth first within each tree, the trees in order
    final = np.empty(n_tmp, dtype=np.int64)
    final[order] = np.arange(n_tmp)

    def link(a):
        out = np.where(a >= 0, final[np.maximum(a, 0)], -1)
        return out[order].astype(np.int32)
    roots = final[np.flatnonzero(depth_of == 0)]
    return rows[order], link(left), link(right), inner[order], roots.astype(np.int32)


def build_kd_cluster_tree(data, n_subdivisions=4, max_level=4, dim=None, use_kd_tree=True, kmeans=None, ctx=None, seed=0, n_init=1,
                          init=None, max_iter=300, tol=1e-4, n_spatial=None):
    """ClusterTree(n_subdivisions, max_level, dim, use_kd_tree=use_kd_tree).construct(data) as a kd_cluster_tree.HipClusterTree.
    dim None: every column.  kmeans: a callable (seg_begin, rows, node_ids) -> labels for every level's batch (default:
    DeviceKMeans on data[:, :dim] in ctx, default context 0, with seed / n_init / init / max_iter / tol)."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    if data.ndim != 2 or data.shape[0] < 1:
        raise ValueError("cluster tree build: data must be a non-empty (n, dim) array")
    n = data.shape[0]
    k, max_level = max(int(n_subdivisions), 1), max(int(max_level), 1)
    dim = min(data.shape[1], int(dim) if dim else data.shape[1])
    own = kmeans is None and k > 1 and n > k
    if own:
        kmeans = DeviceKMeans(_capi.default_context(ctx), data[:, :dim], k, seed, n_init, max_iter, tol, init)
    try:
        means, leaf, kids, wrappers = [], [], [], []
        level = [(np.arange(n, dtype=np.int64), 0, 0)]        # (rows, depth, node id), breadth first
        while level:
            nxt, sub, kinds = [], [], []
            for rows, depth, nid in level:
                m = len(rows)
                if not use_kd_tree and m == 1:
                    means.append(data[rows[0]].copy())
                    leaf.append(1)
                    kinds.append(0)
                elif m > k and k > 1:
                    means.append(np.mean(data if depth == 0 else data[rows], axis=0))
                    leaf.append(0)
                    kinds.append(1)
                    sub.append((rows, nid))
                else:
                    means.append(np.mean(data[rows], axis=0))
                    leaf.append(1 if use_kd_tree else 0)
                    kinds.append(2)
            groups = iter(_cluster_level(kmeans, k, [r for r, _ in sub], [i for _, i in sub]))
            for (rows, depth, nid), kind in zip(level, kinds):
                ch, wr = [], []
                if kind == 1:
                    parts = [g for g in next(groups) if len(g)]
                    if depth < max_level or not use_kd_tree:
                        ch = parts
                    else:
                        wr = parts
                elif kind == 2:
                    if use_kd_tree:
                        wr = [rows]
                    else:
                        ch = [rows[i:i + 1] for i in range(len(rows))]
                if ch and depth + 1 > MG_TREE_MAX_DEPTH:
                    raise ValueError("cluster tree build: deeper than %d levels (MG_TREE_MAX_DEPTH)" % MG_TREE_MAX_DEPTH)
                kids.append(len(ch))
                wrappers.append(wr)
                nxt.extend((g, depth + 1, child_node_id(nid, c)) for c, g in enumerate(ch))
            level = nxt
    finally:
        if own:
            kmeans.close()
    N = len(means)
    child_begin = np.concatenate([[0], np.cumsum(kids)]).astype(np.int32)
    kd_rows, kd_left, kd_right, kd_inner, kd_roots = _kd_forest(data, [w for ws in wrappers for w in ws], dim)
    kd_begin = np.concatenate([[0], np.cumsum([len(w) for w in wrappers])]).astype(np.int32)
    points = np.concatenate([data[kd_rows], np.asarray(means, dtype=np.float64).reshape(N, -1)], axis=0)
    options = {"n_subdivisions": k, "max_level": max_level, "dim": dim, "use_kd_tree": bool(use_kd_tree)}
    return HipClusterTree(data, points, len(kd_rows), child_begin, np.arange(1, N, dtype=np.int32), leaf, kd_begin, kd_roots,
                          kd_left, kd_right, kd_inner, n_spatial, options)


class _Cluster(object):
    """A cluster list of find_clusters as far as the reference's list operations see it: equal to another only if both
    are empty (or it is the same list) -- the members of two clusters are disjoint."""
    __slots__ = ("j", "n")

    def __init__(self, j, n):
        self.j, self.n = j, n

    def __eq__(self, other):
        return self is other or (self.n == 0 and other.n == 0)

    __hash__ = object.__hash__


def _find_clusters_groups(groups, n):
    """find_clusters (clustering.py:106-124) and FeatureClusterTree._construct's loop (feature_cluster_tree.py:86-96) on
    the label groups of a node of n members: the children's member arrays, None for 'one singleton per member'."""
    clusters = [_Cluster(j, len(g)) for j, g in enumerate(groups)]
    for c in clusters:          # the reference's remove-while-iterating
        if c.n == 0:
            clusters.remove(c)
    if len(clusters) == 1 and clusters[0].n == n:
        return None
    out = []
    for c in clusters:
        if c.n > 0:
            if c.n == n:        # np.alltrue(c == indices)
                out.extend(groups[c.j][i:i + 1] for i in range(n))
            else:
                out.append(groups[c.j])
    return out


def build_feature_cluster_tree(features, data=None, n_subdivisions=4, use_feature_mean=False, kmeans=None, ctx=None, seed=0, n_init=1,
                               init=None, max_iter=300, tol=1e-4, n_spatial=None):
    """FeatureClusterTree(features, data, None, {"n_subdivisions", "clustering_method": 0, "use_feature_mean"}, []) as a
    cluster_tree.HipFeatureClusterTree (data None: the features).  `.indices` holds every node's indices (None for the
    root), which the writers need.  kmeans: as for build_kd_cluster_tree (default: DeviceKMeans on the features)."""
    features = np.ascontiguousarray(features, dtype=np.float64)
    data = features if data is None else np.ascontiguousarray(data, dtype=np.float64)
    if features.ndim != 2 or features.shape[0] < 1 or data.shape[0] != features.shape[0]:
        raise ValueError("cluster tree build: features (n, f) and data (n, d) with n >= 1")
    n, k = features.shape[0], int(n_subdivisions)
    if k < 1:
        raise ValueError("cluster tree build: n_subdivisions = %d" % k)
    src = features if use_feature_mean else data
    own = kmeans is None and k > 1 and n > k
    if own:
        kmeans = DeviceKMeans(_capi.default_context(ctx), features, k, seed, n_init, max_iter, tol, init)
    try:
        indices, mean_of, kids = [], [], []
        level = [(None, np.arange(n, dtype=np.int64), 0, 0)]      # (indices or None, rows, depth, node id)
        while level:
            nxt, sub, plan = [], [], []
            for idx, rows, depth, nid in level:
                m = len(rows)
                indices.append(idx)
                mean_of.append(rows)
                if m <= 1:
                    plan.append(None)
                elif m < MAX_SIMILARITY_CHECK and np.all(features[rows] == features[rows[0]]):
                    plan.append("singletons")
                elif m > k:
                    plan.append("kmeans")
                    sub.append((rows, nid))
                else:
                    plan.append("singletons")
            groups = iter(_cluster_level(kmeans, k, [r for r, _ in sub], [i for _, i in sub]))
            for (idx, rows, depth, nid), what in zip(level, plan):
                ch = []
                if what == "kmeans":
                    ch = _find_clusters_groups(next(groups), len(rows))
                if what == "singletons" or ch is None:
                    ch = [rows[i:i + 1] for i in range(len(rows))]
                if ch and depth + 1 > MG_TREE_MAX_DEPTH:
                    raise ValueError("cluster tree build: deeper than %d levels (MG_TREE_MAX_DEPTH)" % MG_TREE_MAX_DEPTH)
                kids.append(len(ch))
                nxt.extend((g, g, depth + 1, child_node_id(nid, c)) for c, g in enumerate(ch))
            level = nxt
    finally:
        if own:
            kmeans.close()
    N = len(indices)
    means = np.empty((N, src.shape[1]), dtype=np.float64)
    single = np.array([len(r) == 1 for r in mean_of])
    if single.any():      # np.average of one row: 0 + row, divided by 1
        means[single] = src[np.array([r[0] for r, s in zip(mean_of, single) if s], dtype=np.int64)] + 0.0
    for i in np.flatnonzero(~single):
        means[i] = np.average(src[mean_of[i]], axis=0)
    first = np.array([-1 if idx is None else int(idx[0]) for idx in indices], dtype=np.int64)
    options = {"n_subdivisions": k, "clustering_method": CLUSTERING_METHOD_KMEANS, "use_feature_mean": bool(use_feature_mean)}
    tree = HipFeatureClusterTree(data, means, np.concatenate([[0], np.cumsum(kids)]), np.arange(1, N, dtype=np.int32), first, options,
                                 features, n_spatial)
    tree.indices = indices
    return tree


# ---- writers ---------------------------------------------------------------------------------------------------------
class _RefObject(object):
    """An object of one of the reference's space_partitioning classes, written under the reference's class path."""

    def __init__(self, **attrs):
        self.__dict__.update(attrs)


def _ref_class(module, name):
    return type(name, (_RefObject,), {"__module__": __name__, "_ref": ("morphablegraphs.space_partitioning." + module, name)})


_ClusterTree = _ref_class("cluster_tree", "ClusterTree")
_ClusterTreeNode = _ref_class("cluster_tree_node", "ClusterTreeNode")
_KDTreeWrapper = _ref_class("kdtree_wrapper_node", "KDTreeWrapper")
_KDTree = _ref_class("kdtree", "KDTree")
_KDNode = _ref_class("kdtree", "Node")
_FeatureClusterTree = _ref_class("feature_cluster_tree", "FeatureClusterTree")


class _ReferencePickler(pickle._Pickler):
    """The Python pickler with the stand-in classes written as the reference's globals (no import of the reference).  Its
    dispatch table is the pickle module's own (a library such as dill may have added entries to pickle._Pickler's)."""
    _P = pickle._Pickler
    dispatch = {type(None): _P.save_none, bool: _P.save_bool, int: _P.save_long, float: _P.save_float, bytes: _P.save_bytes,
                bytearray: _P.save_bytearray, pickle.PickleBuffer: _P.save_picklebuffer, str: _P.save_str, tuple: _P.save_tuple,
                list: _P.save_list, dict: _P.save_dict, set: _P.save_set, frozenset: _P.save_frozenset, types.FunctionType: _P.save_global,
                type: _P.save_type}

    def save(self, obj, save_persistent_id=True):
        if isinstance(obj, type) and issubclass(obj, _RefObject):
            x = self.memo.get(id(obj))
            if x is not None:
                self.write(self.get(x[0]))
                return
            return self.save_global(obj)
        return pickle._Pickler.save(self, obj, save_persistent_id)

    def save_global(self, obj, name=None):
        ref = getattr(obj, "_ref", None) if isinstance(obj, type) and issubclass(obj, _RefObject) else None
        if ref is None:
            return pickle._Pickler.save_global(self, obj, name)
        module, qualname = ref
        if self.proto >= 4:
            self.save(module)
            self.save(qualname)
            self.write(pickle.STACK_GLOBAL)
        else:
            self.write(pickle.GLOBAL + module.encode("ascii") + b"\n" + qualname.encode("ascii") + b"\n")
        self.memoize(obj)


def _dumps(obj, protocol):
    import io
    f = io.BytesIO()
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20000))
    try:
        _ReferencePickler(f, protocol).dump(obj)
    finally:
        sys.setrecursionlimit(limit)
    return f.getvalue()


def _node_depths(child_begin, children):
    depth = np.zeros(len(child_begin) - 1, dtype=np.int64)
    for v in range(len(depth)):        # breadth first: a parent precedes its children
        depth[children[child_begin[v]:child_begin[v + 1]]] = depth[v] + 1
    return depth


def kd_cluster_tree_object(tree):
    """The ClusterTree object graph of a HipClusterTree (what ClusterTree.save_to_file_pickle pickles)."""
    opts = tree.options
    max_level, dim = int(opts.get("max_level", 4)), int(opts.get("dim", tree.data.shape[1]))
    pts = tree.points
    kd_nodes = [_KDNode(index=0, type="inner" if tree.kd_inner[i] else "leaf", point=pts[i].tolist(), left=None, right=None)
                for i in range(tree.n_kd)]
    for i, node in enumerate(kd_nodes):       # breadth first: a node's depth is known before its children's
        for c, attr in ((tree.kd_left[i], "left"), (tree.kd_right[i], "right")):
            if c >= 0:
                setattr(node, attr, kd_nodes[c])
                kd_nodes[c].index = node.index + 1
    depth = _node_depths(tree.child_begin, tree.children)
    cb, kb = tree.child_begin, tree.kd_begin
    nodes = []
    for i in range(tree.n_nodes):
        d = int(depth[i])
        kind = ("root" if d == 0 else "inner") if d < max_level - 1 else "leaf"
        nodes.append(_ClusterTreeNode(id=str(uuid.UUID(int=i + 1)), clusters=[], mean=tree.means[i].copy(), leaf=bool(tree.leaf[i]),
                                      type=kind, depth=d, indices=None))
    for i, node in enumerate(nodes):
        node.clusters = [nodes[c] for c in tree.children[cb[i]:cb[i + 1]]]
        node.clusters += [_KDTreeWrapper(id=str(uuid.UUID(int=(1 << 64) + int(r))), kdtree=_KDTree(data=None, root=kd_nodes[r], global_bb=None),
                                         dim=dim, type="kdtree") for r in tree.kd_roots[kb[i]:kb[i + 1]]]
    return _ClusterTree(n_subdivisions=int(opts.get("n_subdivisions", 4)), max_level=max_level, dim=dim, root=nodes[0], data=tree.data,
                        store_indices=False, use_kd_tree=bool(opts.get("use_kd_tree", True)))


def kd_cluster_tree_pickle(tree, protocol=pickle.HIGHEST_PROTOCOL):
    """The bytes ClusterTree.save_to_file_pickle writes for this tree (cluster_tree_pickle.load_cluster_tree_pickle reads them)."""
    return _dumps(kd_cluster_tree_object(tree), protocol)


def feature_cluster_tree_json(tree):
    """FeatureClusterTree.save_to_json_file's dict (feature_cluster_tree.py:301-319): data, features, options, root."""
    cb, ch = tree.child_begin, tree.children
    nodes = [{"mean": tree.means[i].tolist(), "indices": None if tree.indices[i] is None else [int(v) for v in tree.indices[i]], "children": []}
             for i in range(tree.n_nodes)]
    for i, node in enumerate(nodes):
        node["children"] = [nodes[c] for c in ch[cb[i]:cb[i + 1]]]
    features = tree.features if tree.features is not None else tree.data
    return {"data": tree.data.tolist(), "features": np.asarray(features).tolist(), "options": dict(tree.options), "root": nodes[0]}


def feature_cluster_tree_object(tree):
    """The FeatureClusterTree object graph (what FeatureClusterTree.save_to_file_pickle pickles)."""
    features = np.asarray(tree.features if tree.features is not None else tree.data)
    opts = dict(tree.options)
    nodes = [_FeatureClusterTree(data=tree.data, _features=features, _indices=None if idx is None else [int(v) for v in idx], _children=[],
                                 _options=opts, _mean=tree.means[i].copy(), _n_subdivisions=int(opts.get("n_subdivisions", 4)), args=[])
             for i, idx in enumerate(tree.indices)]
    cb, ch = tree.child_begin, tree.children
    for i, node in enumerate(nodes):
        node._children = [nodes[c] for c in ch[cb[i]:cb[i + 1]]]
    return nodes[0]


def write_cluster_tree(tree, path, output_mode="pck"):
    """The file the reference writes: a ClusterTree always as its pickle; a FeatureClusterTree as JSON or (output_mode
    "pck") as its pickle."""
    if isinstance(tree, HipClusterTree):
        blob = kd_cluster_tree_pickle(tree)
    elif output_mode == "pck":
        blob = _dumps(feature_cluster_tree_object(tree), pickle.HIGHEST_PROTOCOL)
    else:
        with open(path, "wt") as f:
            json.dump(feature_cluster_tree_json(tree), f)
        return path
    with open(path, "wb") as f:
        f.write(blob)
    return path


# ---- ClusterTreeBuilder ----------------------------------------------------------------------------------------------
TREE_TYPE_CLUSTER_TREE, TREE_TYPE_FEATURE_CLUSTER_TREE = 0, 1          # construction/cluster_tree_builder.py:58-59
FEATURE_TYPE_S_VECTOR, FEATURE_TYPE_EUCLIDEAN_PCA = 0, 1
CLUSTER_TREE_FILE_ENDING = "_cluster_tree"


class HipClusterTreeBuilder(object):
    """ClusterTreeBuilder (construction/cluster_tree_builder.py:120-301) with the samples drawn and the trees built on the
    device.  settings: tree_type, feature_type, output_mode; set_config takes the reference's keys.  random_seed seeds the
    device k-means (the reference leaves sklearn's global RNG unseeded); None = 0."""

    def __init__(self, settings, ctx=None):
        from .cluster_tree_sampling import HipClusterTreeSampler
        self.morphable_model_directory = None
        self.n_samples = 10000
        self.n_subdivisions_per_level = 4
        self.n_levels = 4
        self.random_seed = None
        self.only_spatial_parameters = True
        self.store_indices = False
        self.use_kd_tree = True
        self.tree_type = settings["tree_type"]
        self.feature_type = settings["feature_type"]
        self.output_mode = settings["output_mode"]
        self.skeleton = None
        self.joint_names = None
        self.device_features = False       # "euclidean_pca" features on the device (mg_point_cloud_features, mg_pca_fit_leading); opt-in
        self.ctx = ctx
        self.sampler = HipClusterTreeSampler(self.n_samples)

    def set_config(self, config):
        self.morphable_model_directory = config["model_data_dir"]
        self.n_samples = config["n_random_samples"]
        self.n_subdivisions_per_level = config["n_subdivisions_per_level"]
        self.n_levels = config["n_levels"]
        self.random_seed = config["random_seed"]
        self.only_spatial_parameters = config["only_spatial_parameters"]
        self.store_indices = config["store_data_indices_in_nodes"]
        self.use_kd_tree = config["use_kd_tree"]
        self.device_features = bool(config.get("device_features", self.device_features))
        self.sampler.n_samples = int(self.n_samples)

    def _seed(self):
        return 0 if self.random_seed is None else int(self.random_seed)

    def _ctx(self, motion_primitive):
        if self.ctx is not None:
            return self.ctx
        prim = motion_primitive.motion_primitive if hasattr(motion_primitive, "motion_primitive") else motion_primitive
        p = getattr(prim, "_prim", None)
        return p.ctx if p is not None else _capi.default_context(None)

    # cluster_tree_builder.py:237-247
    def _build_tree(self, elementary_action_dir, cluster_file_name, data, motion_primitive):
        data = np.asarray(data, dtype=np.float64)
        n_dims = motion_primitive.get_n_spatial_components() if self.only_spatial_parameters else data.shape[1]
        tree = build_kd_cluster_tree(data, self.n_subdivisions_per_level, self.n_levels, n_dims, self.use_kd_tree, ctx=self._ctx(motion_primitive),
                                     seed=self._seed())
        if elementary_action_dir is not None:
            import os
            write_cluster_tree(tree, os.path.join(elementary_action_dir, cluster_file_name + CLUSTER_TREE_FILE_ENDING + ".pck"))
        return tree

    # cluster_tree_builder.py:249-264
    def _build_feature_tree(self, action_name, model_name, data, motion_primitive):
        data = np.asarray(data, dtype=np.float64)
        features = self._extract_features(motion_primitive, data)
        tree = build_feature_cluster_tree(features, data, self.n_subdivisions_per_level, False, ctx=self._ctx(motion_primitive), seed=self._seed())
        if self.morphable_model_directory is not None and action_name is not None:
            import os
            stem = os.path.join(self.morphable_model_directory, action_name, model_name + CLUSTER_TREE_FILE_ENDING)
            write_cluster_tree(tree, stem + (".pck" if self.output_mode == "pck" else ".json"), self.output_mode)
        return tree

    def _extract_features(self, motion_primitive, data):
        if self.feature_type == FEATURE_TYPE_EUCLIDEAN_PCA:
            if self.device_features:
                return self.sampler._extract_features(motion_primitive, data, "euclidean_pca", self.skeleton, self.joint_names, step=1, device_features=True)
            return self.sampler._extract_features(motion_primitive, data, "euclidean_pca", self.skeleton, self.joint_names, step=1)
        return self.sampler._extract_features(motion_primitive, data, "latent")

    def build_for_node(self, node, data=None):
        """The tree of self.tree_type for a HipMotionStateGraphNode from `data` (default: n_random_samples device samples of
        the node, sample_data) attached as node.cluster_tree, which search_best_sample and evaluate_options(use_cluster_trees=
        True) then search.  Nothing is written.  Returns the tree."""
        if data is None:
            data = self.sampler.sample_data(node)
        if self.tree_type == TREE_TYPE_FEATURE_CLUSTER_TREE:
            tree = self._build_feature_tree(None, None, data, node)
        else:
            tree = self._build_tree(None, None, data, node)
        tree.validate(node.get_n_spatial_components())
        old = getattr(node, "cluster_tree", None)
        if old is not None and hasattr(old, "close"):
            old.close()
        node.cluster_tree = tree
        return tree
