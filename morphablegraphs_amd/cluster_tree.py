"""The FeatureClusterTree of a graph node (reference morphablegraphs/space_partitioning/feature_cluster_tree.py) as the
reference loads it from a model zip (`space_partition_json`, motion_state_graph_node.py:99-104, utilities/zip_io.py:196-213)
and the search it runs over it, find_best_example_excluding_search_candidates (feature_cluster_tree.py:129-187).

The nested JSON tree is flattened once, iteratively and breadth first in the JSON's child order: node 0 is the root,
means (n_nodes, dim) float64, the children in CSR form (child_begin, children), indices[0] per node (-1 for a node without
indices) and the depth of every node.  The descent itself runs

  * on the host with any Python objective (`find_best_example_excluding_search_candidates(obj, args, n)`), the
    reference's loop call for call, or with one batched scoring call per level (`descend`); or
  * on the device, every search of a call in ONE launch (mg_cluster_tree_search; `search_on_device`).

The reference's quirks are kept, on every path:
  * the candidates kept per node and per level are the first n entries of the heap's LIST (`result_queue[:n]`,
    `new_candidates[:n]`), not the n smallest values;
  * a leaf's value is the objective of its mean, computed when it was pushed as a child (never recomputed);
  * the returned row is `data[leaf.indices[0]]`;
  * a root that is itself a leaf returns `(inf, data[root.indices[0]])` -- a TypeError where the root has no indices,
    which is what a tree built by the reference's constructor writes for its root;
  * two equal values meeting in a heap comparison make the tuples compare their tree nodes, which raises TypeError.
"""
import heapq

import numpy as np

from . import _capi

MG_TREE_MAX_DEPTH, MG_TREE_MAX_CHILDREN, MG_TREE_MAX_CANDIDATES = _capi.MG_TREE_MAX_DEPTH, _capi.MG_TREE_MAX_CHILDREN, _capi.MG_TREE_MAX_CANDIDATES


class _TreeNode(object):
    """A node in the heaps: like the reference's FeatureClusterTree and ClusterTreeNode it defines no ordering, so tuples
    that reach it raise TypeError when heapq compares them."""
    __slots__ = ("index",)

    def __init__(self, index):
        self.index = index


def _forest(n, roots, kids, max_depth, what, depth_of=None):
    """Depth of the forest below `roots` (kids(v): v's children); ValueError unless every node has one parent and is reached.
    depth_of: an array that receives every node's depth."""
    seen = np.zeros(n, dtype=bool)
    level = [int(r) for r in roots]
    for r in level:
        if r < 0 or r >= n or seen[r]:
            raise ValueError("cluster tree: every %s node needs exactly one parent" % what)
        seen[r] = True
    depth = 0
    while level:
        nxt = [int(c) for v in level for c in kids(v)]
        if not nxt:
            break
        depth += 1
        if depth > max_depth:
            raise ValueError("cluster tree: %s levels deeper than %d, or a cycle" % (what, max_depth))
        for c in nxt:
            if c < 0 or c >= n or seen[c]:
                raise ValueError("cluster tree: every %s node needs exactly one parent" % what)
            seen[c] = True
        if depth_of is not None:
            depth_of[nxt] = depth
        level = nxt
    if not seen.all():
        raise ValueError("cluster tree: %s nodes not reachable from the root (a cycle)" % what)
    return depth


class _SearchTree(object):
    """What the two kinds of tree share beside their tables: the device copy per context and the flags of a search record
    that mean the same for both."""
    _TIE = None     # the reference's TypeError text

    def _upload(self, prim):
        raise NotImplementedError

    def device_tree(self, prim):
        """The tree on the device of prim's context (a _capi.ClusterTree), uploaded once per context."""
        key = id(prim.ctx)
        t = self._device.get(key)
        if t is not None and t[0] is prim.ctx and t[1].handle and prim.ctx.handle:
            return t[1]
        tree = self._upload(prim)
        self._device[key] = (prim.ctx, tree)
        return tree

    def close(self):
        for _, tree in self._device.values():
            tree.close()
        self._device = {}

    def _flags_of_record(self, rec):
        """A record's flags, or the exception for a search that overflowed or met a tie."""
        flags = int(rec["flags"])
        if flags & _capi.MG_TREE_OVERFLOW:
            raise RuntimeError("cluster-tree search: a heap outgrew its bound")
        if flags & _capi.MG_TREE_TIE:
            raise TypeError(self._TIE)
        return flags


class HipFeatureClusterTree(_SearchTree):
    """A FeatureClusterTree loaded from the reference's JSON layout: {"data", "features", "options", "root": {"mean",
    "indices", "children"}} (feature_cluster_tree.py:293-333).  `.data` is the float64 array of the stored samples
    (what the exhaustive search scores)."""
    _TIE = "'<' not supported between instances of 'FeatureClusterTree' and 'FeatureClusterTree' (two candidates of equal value)"

    def __init__(self, data, means, child_begin, children, first_index, options=None, features=None, n_spatial=None):
        self.data = np.asarray(data, dtype=np.float64)
        self.means = np.ascontiguousarray(means, dtype=np.float64)
        self.child_begin = np.asarray(child_begin, dtype=np.int32)
        self.children = np.asarray(children, dtype=np.int32)
        self.first_index = np.asarray(first_index, dtype=np.int64)
        self.options = dict(options or {})
        self.features = features
        self._device = {}
        self.validate(n_spatial)
        self._nodes = [_TreeNode(i) for i in range(self.n_nodes)]

    @property
    def n_nodes(self):
        return self.means.shape[0]

    @classmethod
    def from_json(cls, tree_data, n_spatial=None):
        """Flatten tree_data["root"] iteratively (breadth first, children in JSON order) and validate it.  n_spatial: the
        primitive's spatial latent count, which the means must cover."""
        data = np.asarray(tree_data["data"], dtype=np.float64)
        if data.ndim != 2 or data.shape[0] == 0:
            raise ValueError("cluster tree: data must be a non-empty (n, dim) array")
        root = tree_data["root"]
        if not isinstance(root, dict) or "mean" not in root:
            raise ValueError("cluster tree: no root node")
        order, indices = [root], []
        child_begin, children, depth = [0], [], [0]
        head = 0
        while head < len(order):
            node = order[head]
            if not isinstance(node, dict) or "mean" not in node:
                raise ValueError("cluster tree: node %d has no mean" % head)
            idx = node.get("indices")
            indices.append(None if idx is None else list(idx))
            for c in node.get("children") or []:
                children.append(len(order))
                order.append(c)
                depth.append(depth[head] + 1)
                if depth[-1] > MG_TREE_MAX_DEPTH:
                    raise ValueError("cluster tree: deeper than %d levels" % MG_TREE_MAX_DEPTH)
            child_begin.append(len(children))
            head += 1
        widths = set(len(n["mean"]) for n in order)
        if len(widths) != 1:
            raise ValueError("cluster tree: node means of different widths %s" % sorted(widths))
        means = np.asarray([n["mean"] for n in order], dtype=np.float64).reshape(len(order), -1)
        for i, idx in enumerate(indices):
            if idx is not None and any((not isinstance(v, (int, np.integer))) or v < 0 or v >= data.shape[0] for v in idx):
                raise ValueError("cluster tree: node %d has an index outside [0, %d)" % (i, data.shape[0]))
        first = np.asarray([-1 if not idx else int(idx[0]) for idx in indices], dtype=np.int64)
        return cls(data, means, child_begin, children, first, tree_data.get("options"), tree_data.get("features"), n_spatial)

    def validate(self, n_spatial=None):
        """The checks mg_cluster_tree_create makes as well: ValueError for a tree the search must not walk."""
        n = self.n_nodes
        cb, ch = self.child_begin, self.children
        if self.means.ndim != 2 or n < 1:
            raise ValueError("cluster tree: no nodes")
        if self.means.shape[1] != self.data.shape[1]:
            raise ValueError("cluster tree: means of width %d, data of width %d" % (self.means.shape[1], self.data.shape[1]))
        if n_spatial is not None and self.means.shape[1] < int(n_spatial):
            raise ValueError("cluster tree: width %d < %d spatial components" % (self.means.shape[1], n_spatial))
        if cb.shape != (n + 1,) or cb[0] != 0 or cb[-1] != n - 1 or len(ch) != n - 1 or np.any(np.diff(cb) < 0):
            raise ValueError("cluster tree: every node but the root needs exactly one parent")
        counts = np.diff(cb)
        if counts.max(initial=0) > MG_TREE_MAX_CHILDREN:
            raise ValueError("cluster tree: a node with more than %d children" % MG_TREE_MAX_CHILDREN)
        if len(ch) and (ch.min() < 1 or ch.max() >= n or len(np.unique(ch)) != len(ch)):
            raise ValueError("cluster tree: every node but the root needs exactly one parent")
        self.depth = np.zeros(n, dtype=np.int32)     # every node's level below the root
        _forest(n, [0], lambda v: ch[cb[v]:cb[v + 1]], MG_TREE_MAX_DEPTH, "cluster", self.depth)
        fi = self.first_index
        if np.any(fi < -1) or np.any(fi >= self.data.shape[0]):
            raise ValueError("cluster tree: an index outside [0, %d)" % self.data.shape[0])
        leaves = np.nonzero(counts == 0)[0]
        if np.any(fi[leaves[leaves != 0]] < 0):
            raise ValueError("cluster tree: a leaf without indices")

    # ---- the descent ------------------------------------------------------------------------------------------
    def descend(self, score, n_candidates=1):
        """find_best_example_excluding_search_candidates with the children of each level scored by ONE call:
        score(node ids) -> their values, in order (the frontier's nodes in list order, each node's children in order --
        the order in which the reference calls its objective).  Returns (value, row, leaf, evaluations)."""
        n = int(n_candidates)
        cb, ch, nodes = self.child_begin, self.children, self._nodes
        results = []
        candidates = [(np.inf, nodes[0])]
        evaluations = 0
        while len(candidates) > 0:
            new_candidates = []
            ids = [int(c) for _, ref in candidates for c in ch[cb[ref.index]:cb[ref.index + 1]]]
            values = score(ids) if ids else ()
            evaluations += len(ids)
            pos = 0
            for value, ref in candidates:
                b, e = cb[ref.index], cb[ref.index + 1]
                if e > b:       # _find_best_cluster_candidates: every child pushed, the heap list's first n kept
                    result_queue = []
                    for k in range(b, e):
                        heapq.heappush(result_queue, (values[pos], nodes[ch[k]]))
                        pos += 1
                    for c in result_queue[:n]:
                        heapq.heappush(new_candidates, c)
                else:
                    heapq.heappush(results, (value, ref))
            candidates = new_candidates[:n]
        if len(results) > 0:
            value, ref = heapq.heappop(results)
            row = int(self.first_index[ref.index])
            if row < 0:
                raise TypeError("'NoneType' object is not subscriptable")     # the reference's node._indices[0] on None
            return value, self.data[row], ref.index, evaluations
        return np.inf, self._root_row(), 0, evaluations

    def _root_row(self):
        if self.first_index[0] < 0:
            raise TypeError("'NoneType' object is not subscriptable")
        return self.data[int(self.first_index[0])]

    def find_best_example_excluding_search_candidates(self, obj, args, n_candidates=1):
        """The reference's method: obj(mean, args) once per child of every frontier node.  Returns (value, row)."""
        means = self.means
        value, row, _, _ = self.descend(lambda ids: [obj(means[i], args) for i in ids], n_candidates)
        return value, row

    # ---- the device copy --------------------------------------------------------------------------------------
    def _upload(self, prim):
        return _capi.ClusterTree(prim, self.means, self.child_begin, self.children, self.first_index, self.data.shape[0])

    def result_of_record(self, rec):
        """(value, row) of a search record, or the reference's exception."""
        flags = self._flags_of_record(rec)
        if flags & _capi.MG_TREE_NO_RESULT:
            return np.inf, self._root_row()
        row = int(rec["row"])
        if row < 0:
            raise TypeError("'NoneType' object is not subscriptable")
        return float(rec["value"]), self.data[row]


class TreeSearchSet(object):
    """What a one-launch search scores a row against: the device keyframe set, then the root trajectory constraints
    [(_capi.Trajectory, min_u, weight)] in list order, both under `alignment` (None: local coordinates).  The trajectories
    are the cache's (candidate_scoring.cached_trajectory(..., pin=True)): release() hands them back, once.
    frame_constraints: None, or the per-frame constraint list scored behind them (frame_constraints.TreeFrameList: the track plan,
    the descriptors in list order, their pinned trajectories and grids), released with the set."""

    def __init__(self, cset, trajectories=(), alignment=None, frame_constraints=None):
        self.cset, self.trajectories, self.alignment = cset, list(trajectories), alignment
        self.frame_constraints = frame_constraints

    def release(self):
        from .candidate_scoring import release_trajectory
        held, self.trajectories = self.trajectories, []
        frames, self.frame_constraints = self.frame_constraints, None
        try:
            if frames is not None:
                frames.release()
        finally:
            for t, _, _ in held:
                release_trajectory(t)


def _frames_arguments(searches):
    prims = [p for _, p, _ in searches]
    trees = [t.device_tree(p) for t, p, _ in searches]
    sets = [c if isinstance(c, TreeSearchSet) else TreeSearchSet(c) for _, _, c in searches]
    return (prims, trees, [c.cset for c in sets]), ([c.trajectories for c in sets],
                                                    [c.alignment if (c.trajectories or c.frame_constraints is not None) else None for c in sets],
                                                    [c.frame_constraints for c in sets])


def frames_search_plan(searches, n_candidates):
    """What search_on_device would stage for searches that carry per-frame lists (_capi.cluster_tree_frames_plan); launches nothing."""
    head, tail = _frames_arguments(searches)
    return _capi.cluster_tree_frames_plan(*head, n_candidates, *tail)


def search_on_device(searches, n_candidates):
    """searches: [(HipFeatureClusterTree | HipClusterTree, _capi.Primitive, _capi.ConstraintSet | TreeSearchSet)], all in one
    context and of one tree kind.  ONE launch, one read-back, with or without trajectories and per-frame lists
    (mg_cluster_tree_search[_trajectories | _frames]).  Returns the records (the caller interprets them with tree.result_of_record)."""
    if not searches:
        return np.zeros(0, dtype=_capi.TREE_SEARCH_RECORD)
    prims = [p for _, p, _ in searches]
    trees = [t.device_tree(p) for t, p, _ in searches]
    sets = [c if isinstance(c, TreeSearchSet) else TreeSearchSet(c) for _, _, c in searches]
    csets = [c.cset for c in sets]
    if any(c.frame_constraints is not None for c in sets):
        head, tail = _frames_arguments(searches)
        return _capi.search_cluster_trees_frames(*head, n_candidates, *tail)
    if not any(c.trajectories for c in sets):
        return _capi.search_cluster_trees(prims, trees, csets, n_candidates)
    return _capi.search_cluster_trees(prims, trees, csets, n_candidates, trajectories=[c.trajectories for c in sets],
                                      alignments=[c.alignment if c.trajectories else None for c in sets])


def has_search_tree(node):
    return isinstance(getattr(node, "cluster_tree", None), HipFeatureClusterTree)
