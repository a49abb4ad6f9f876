"""The reference's other cluster tree: space_partitioning.ClusterTree, k-means clusters down to KD-tree leaves, as a pickled
model carries it (`<primitive>_cluster_tree.pck`, construction/cluster_tree_builder.py:235-247, read by
utilities/zip_io.py:204-213 into `space_partition_pickle`), and its search
find_best_example_excluding_search_candidates (cluster_tree.py:117-149; cluster_tree_node.py:63-79,113-138;
kdtree.py:132-164,233-250).

The tree is flattened once, breadth first in the reference's child order:
  * cluster nodes: node 0 is the root; CSR children (child_begin, children); `leaf` (the node's flag); the roots of its
    KDTreeWrapper children in CSR form (kd_begin, kd_roots);
  * KD nodes: KD node k's point is row k of `points`; kd_left / kd_right (-1: none); kd_inner (type == "inner");
  * points (n_kd + n_nodes, dim) float64: the KD points, then every cluster node's mean (`means` is that tail);
  * `.data`, the tree's samples, for the exhaustive search.

The descent runs on the host with any Python objective, call for call (`find_best_example_excluding_search_candidates`),
with one batched scoring call per level or KD step (`descend`), or on the device in one launch
(mg_cluster_tree_search; cluster_tree.search_on_device).  The reference's behaviour is kept on every path:
  * the heap LIST's first n entries are kept per node and per level; new_candidates holds (value, idx, node) with idx the
    position in a node's prefix, so equal values with equal idx compare tree nodes: TypeError;
  * a leaf's answer is the best of its KD descents ((value, point list), lists compared on equal values) or, without KD
    trees, (obj(mean), mean.tolist()); results holds (value, c_idx, point list);
  * a KD descent scores its root's point, then at every inner node the right child and then the left, going left only if
    strictly better, and returns the first of its (cost, depth) heap;
  * a non-leaf node whose children are KD trees raises AttributeError when the search expands it;
  * no result: (inf, root.mean).
"""
import heapq

import numpy as np

from . import _capi
from .cluster_tree import _forest, _SearchTree, _TreeNode

MG_TREE_MAX_DEPTH, MG_TREE_MAX_CHILDREN, MG_KD_MAX_DEPTH = _capi.MG_TREE_MAX_DEPTH, _capi.MG_TREE_MAX_CHILDREN, _capi.MG_KD_MAX_DEPTH

_NO_MEAN = "'KDTreeWrapper' object has no attribute 'mean'"


class _Point(list):
    """A point list (compares as a list) that remembers its row of the points table and its cluster node."""

    def __init__(self, values, row, leaf):
        list.__init__(self, values)
        self.row, self.leaf = row, leaf


class HipClusterTree(_SearchTree):
    """A k-means / KD ClusterTree flattened and validated (see the module's docstring for the tables)."""
    _TIE = "'<' not supported between instances of 'ClusterTreeNode' and 'ClusterTreeNode' (two candidates of equal value and index)"

    def __init__(self, data, points, n_kd, child_begin, children, leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner, n_spatial=None,
                 options=None):
        self.data = np.asarray(data, dtype=np.float64)
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.n_kd = int(n_kd)
        self.child_begin = np.asarray(child_begin, dtype=np.int32)
        self.children = np.asarray(children, dtype=np.int32)
        self.leaf = np.asarray(leaf, dtype=np.int32)
        self.kd_begin = np.asarray(kd_begin, dtype=np.int32)
        self.kd_roots = np.asarray(kd_roots, dtype=np.int32)
        self.kd_left = np.asarray(kd_left, dtype=np.int32)
        self.kd_right = np.asarray(kd_right, dtype=np.int32)
        self.kd_inner = np.asarray(kd_inner, dtype=np.int32)
        self.options = dict(options or {})
        self._device = {}
        self.validate(n_spatial)
        self._nodes = [_TreeNode(i) for i in range(self.n_nodes)]

    @property
    def n_nodes(self):
        return self.points.shape[0] - self.n_kd

    @property
    def means(self):
        return self.points[self.n_kd:]

    @classmethod
    def from_reference(cls, tree, n_spatial=None):
        """Flatten a ClusterTree object (the reference's own, or what cluster_tree_pickle reads): tree.root, tree.data; a
        ClusterTreeNode has .mean, .leaf, .clusters; a KDTreeWrapper .kdtree.root; a KD Node .point, .left, .right, .type."""
        root = getattr(tree, "root", None)
        if root is None or not hasattr(root, "mean"):
            raise ValueError("cluster tree: no root node")
        order, seen = [root], {id(root)}
        child_begin, children, leaf, kd_begin, kd_roots = [0], [], [], [0], []
        kd_points, kd_left, kd_right, kd_inner, depth = [], [], [], [], [0]
        head = 0
        while head < len(order):
            node = order[head]
            kids = list(getattr(node, "clusters", None) or [])
            is_kd = [hasattr(c, "kdtree") for c in kids]
            if any(is_kd) and not all(is_kd):
                raise ValueError("cluster tree: node %d mixes cluster-node and KD-tree children" % head)
            if len(kids) > MG_TREE_MAX_CHILDREN:
                raise ValueError("cluster tree: a node with more than %d children" % MG_TREE_MAX_CHILDREN)
            leaf.append(1 if getattr(node, "leaf", False) else 0)
            for c in kids:
                if id(c) in seen:
                    raise ValueError("cluster tree: every node but the root needs exactly one parent")
                seen.add(id(c))
                if is_kd[0]:
                    r = getattr(c.kdtree, "root", None)
                    if r is None:
                        raise ValueError("cluster tree: node %d has a KD tree without a root" % head)
                    kd_roots.append(cls._flatten_kd(r, kd_points, kd_left, kd_right, kd_inner, seen))
                else:
                    if not hasattr(c, "mean"):
                        raise ValueError("cluster tree: node %d has a child that is neither a cluster node nor a KD tree" % head)
                    children.append(len(order))
                    order.append(c)
                    depth.append(depth[head] + 1)
                    if depth[-1] > MG_TREE_MAX_DEPTH:
                        raise ValueError("cluster tree: deeper than %d levels" % MG_TREE_MAX_DEPTH)
            child_begin.append(len(children))
            kd_begin.append(len(kd_roots))
            head += 1
        try:
            rows = [np.asarray(p, dtype=np.float64) for p in kd_points] + [np.asarray(nd.mean, dtype=np.float64) for nd in order]
        except (TypeError, ValueError):
            raise ValueError("cluster tree: a point or mean that is not a vector of numbers")
        shapes = set(r.shape for r in rows)
        if len(shapes) != 1 or len(next(iter(shapes))) != 1:
            raise ValueError("cluster tree: points and means of different shapes %s" % sorted(shapes))
        data = getattr(tree, "data", None)
        data = np.asarray(rows[len(kd_points):] if data is None else data, dtype=np.float64)
        options = {k: getattr(tree, k) for k in ("n_subdivisions", "max_level", "dim", "use_kd_tree") if hasattr(tree, k)}
        return cls(data, np.stack(rows), len(kd_points), child_begin, children, leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner,
                   n_spatial, options)

    @staticmethod
    def _flatten_kd(root, points, left, right, inner, seen):
        """A KD tree's nodes appended breadth first; returns its root's index."""
        base = len(points)
        order = [root]
        head = 0
        while head < len(order):
            node = order[head]
            if not hasattr(node, "point"):
                raise ValueError("cluster tree: a KD node without a point")
            points.append(node.point)
            inner.append(1 if getattr(node, "type", None) == "inner" else 0)
            links = []
            for c in (getattr(node, "left", None), getattr(node, "right", None)):
                if c is None:
                    links.append(-1)
                    continue
                if id(c) in seen:
                    raise ValueError("cluster tree: every KD node needs exactly one parent")
                seen.add(id(c))
                links.append(base + len(order))
                order.append(c)
                if len(order) - base > (1 << 24):
                    raise ValueError("cluster tree: a KD tree of more than 2^24 nodes")
            left.append(links[0])
            right.append(links[1])
            head += 1
        return base

    def validate(self, n_spatial=None):
        """The checks mg_cluster_tree_create_kd makes as well: ValueError for a tree the search must not walk."""
        n, nk = self.n_nodes, self.n_kd
        cb, ch, kb, kr = self.child_begin, self.children, self.kd_begin, self.kd_roots
        if self.points.ndim != 2 or n < 1 or nk < 0:
            raise ValueError("cluster tree: no nodes")
        if n_spatial is not None and self.points.shape[1] < int(n_spatial):
            raise ValueError("cluster tree: width %d < %d spatial components" % (self.points.shape[1], n_spatial))
        if self.data.ndim != 2 or self.data.shape[1] != self.points.shape[1]:
            raise ValueError("cluster tree: points of width %d, data of shape %s" % (self.points.shape[1], self.data.shape))
        if cb.shape != (n + 1,) or cb[0] != 0 or cb[-1] != n - 1 or len(ch) != n - 1 or np.any(np.diff(cb) < 0):
            raise ValueError("cluster tree: every node but the root needs exactly one parent")
        if kb.shape != (n + 1,) or kb[0] != 0 or kb[-1] != len(kr) or np.any(np.diff(kb) < 0):
            raise ValueError("cluster tree: kd_begin must run from 0 to the number of KD roots")
        if self.leaf.shape != (n,) or any(a.shape != (nk,) for a in (self.kd_left, self.kd_right, self.kd_inner)):
            raise ValueError("cluster tree: leaf (n_nodes), kd_left / kd_right / kd_inner (n_kd)")
        counts, kcounts = np.diff(cb), np.diff(kb)
        if max(counts.max(initial=0), kcounts.max(initial=0)) > MG_TREE_MAX_CHILDREN:
            raise ValueError("cluster tree: a node with more than %d children" % MG_TREE_MAX_CHILDREN)
        if np.any((counts > 0) & (kcounts > 0)):
            raise ValueError("cluster tree: a node mixes cluster-node and KD-tree children")
        if np.any((self.leaf != 0) & (counts > 0)):
            raise ValueError("cluster tree: a leaf with cluster-node children")
        if len(ch) and ch.min() < 1:
            raise ValueError("cluster tree: every node but the root needs exactly one parent")
        self.depth = _forest(n, [0], lambda v: ch[cb[v]:cb[v + 1]], MG_TREE_MAX_DEPTH, "cluster")
        kl, krt = self.kd_left, self.kd_right
        self.kd_depth = _forest(nk, kr, lambda v: [c for c in (kl[v], krt[v]) if c >= 0], MG_KD_MAX_DEPTH, "KD")

    # ---- the reference's search, call for call --------------------------------------------------------------
    def find_best_example_excluding_search_candidates(self, obj, data, n_candidates=1):
        """obj(x, data) in the reference's order: a child's mean (ndarray), a KD point (list), a childless leaf's mean
        (ndarray).  Returns (value, sample list), or (inf, root mean) when no leaf is reached."""
        n = n_candidates
        cb, ch, kb, nodes, means = self.child_begin, self.children, self.kd_begin, self._nodes, self.means
        results = []
        candidates = [(np.inf, 0, nodes[0])]
        while len(candidates) > 0:
            new_candidates = []
            for c_idx, (value, _, node) in enumerate(candidates):
                i = node.index
                if not self.leaf[i]:
                    if kb[i + 1] > kb[i]:
                        raise AttributeError(_NO_MEAN)
                    result_queue = []
                    for cluster_index, k in enumerate(ch[cb[i]:cb[i + 1]]):
                        heapq.heappush(result_queue, (obj(means[k], data), cluster_index, nodes[k]))
                    for idx, c in enumerate(result_queue[:n]):
                        heapq.heappush(new_candidates, (c[0], idx, c[2]))
                else:
                    v, sample = self._leaf_best(i, obj, data)
                    heapq.heappush(results, (v, c_idx, sample))
            candidates = new_candidates[:n]
        if len(results) > 0:
            r = heapq.heappop(results)
            return r[0], r[2]
        return np.inf, means[0].copy()

    def _leaf_best(self, i, obj, data):
        result_queue = []
        roots = self.kd_roots[self.kd_begin[i]:self.kd_begin[i + 1]]
        if len(roots) > 0:
            for r in roots:
                heapq.heappush(result_queue, self._kd_best(int(r), obj, data))
        else:
            mean = self.means[i]
            heapq.heappush(result_queue, (obj(mean, data), mean.tolist()))
        return heapq.heappop(result_queue)

    def _kd_best(self, node, obj, data):
        """KDTree.find_best_example(obj, data, 1)[0]."""
        pts, left, right, inner = self.points, self.kd_left, self.kd_right, self.kd_inner
        eval_points, result_queue, depth = [node], [], 0
        heapq.heappush(result_queue, (obj(pts[node].tolist(), data), depth))
        while node >= 0 and inner[node]:
            depth += 1
            lc, rc = int(left[node]), int(right[node])
            if lc >= 0 and rc >= 0:
                r_d = obj(pts[rc].tolist(), data)
                l_d = obj(pts[lc].tolist(), data)
                node, cost = (lc, l_d) if l_d < r_d else (rc, r_d)
            elif rc >= 0:
                node, cost = rc, obj(pts[rc].tolist(), data)
            elif lc >= 0:
                node, cost = lc, obj(pts[lc].tolist(), data)
            else:
                node = -1
            if node >= 0:
                heapq.heappush(result_queue, (cost, depth))
                eval_points.append(node)
        value, index = result_queue[0]
        return value, pts[eval_points[index]].tolist()

    # ---- the same search, batched as the device runs it ------------------------------------------------------
    def descend_rows(self, score, n_candidates=1):
        """The search with score(rows of `points`) -> their values, called once per level for the inner nodes' children,
        the leaves' KD roots and childless leaves' means, then once per KD step for every running descent's children
        (right before left): the order of mg_kd_tree_search_kernel.  Returns (value, row, leaf, evaluations); row = -1
        when no leaf is reached (value inf).  Raises TypeError / AttributeError where the reference does."""
        n = int(n_candidates)
        cb, ch, kb, kr, nodes, nk, P = self.child_begin, self.children, self.kd_begin, self.kd_roots, self._nodes, self.n_kd, self.points
        kl, krt, kin = self.kd_left, self.kd_right, self.kd_inner
        results, candidates, evaluations = [], [nodes[0]], 0

        def scored(rows):
            return list(score(rows)) if rows else []
        while candidates:
            stop = next((f for f, nd in enumerate(candidates) if not self.leaf[nd.index] and kb[nd.index + 1] > kb[nd.index]), None)
            front = candidates if stop is None else candidates[:stop]
            inner = [nd.index for nd in front if not self.leaf[nd.index]]
            kids = [int(k) for i in inner for k in ch[cb[i]:cb[i + 1]]]
            starts, owners = [], []   # the leaves' descents: a KD root, or the leaf's mean row
            if stop is None:
                for c_idx, nd in enumerate(front):
                    i = nd.index
                    if self.leaf[i]:
                        roots = kr[kb[i]:kb[i + 1]]
                        for r in (roots if len(roots) else [nk + i]):
                            starts.append(int(r))
                            owners.append(c_idx)
            values = scored([nk + k for k in kids] + starts)
            evaluations += len(kids) + len(starts)
            new_candidates, pos = [], 0
            for i in inner:
                result_queue = []
                for cluster_index in range(cb[i + 1] - cb[i]):
                    heapq.heappush(result_queue, (values[pos], cluster_index, nodes[kids[pos]]))
                    pos += 1
                for idx, c in enumerate(result_queue[:n]):
                    heapq.heappush(new_candidates, (c[0], idx, c[2]))
            if stop is not None:
                raise AttributeError(_NO_MEAN)
            # the descents side by side: a (cost, depth) heap and the point row per depth for each
            heaps = [[(values[pos + j], 0)] for j in range(len(starts))]
            visited = [[s] for s in starts]
            cur = [s if s < nk else -1 for s in starts]
            while True:
                active = [j for j in range(len(starts)) if cur[j] >= 0 and kin[cur[j]]]
                if not active:
                    break
                slots = [int(c) for j in active for c in (krt[cur[j]], kl[cur[j]]) if c >= 0]
                step = scored(slots)
                evaluations += len(slots)
                q = 0
                for j in active:
                    rc, lc = int(krt[cur[j]]), int(kl[cur[j]])
                    if rc >= 0 and lc >= 0:
                        r_d, l_d = step[q], step[q + 1]
                        q += 2
                        cur[j], cost = (lc, l_d) if l_d < r_d else (rc, r_d)
                    elif rc >= 0 or lc >= 0:
                        cur[j], cost = max(rc, lc), step[q]
                        q += 1
                    else:
                        cur[j] = -1
                    if cur[j] >= 0:
                        heapq.heappush(heaps[j], (cost, len(visited[j])))
                        visited[j].append(cur[j])
            leaf_queue = []
            for j in range(len(starts)):
                v, d = heaps[j][0]
                row = visited[j][d]
                heapq.heappush(leaf_queue, (v, _Point(P[row].tolist(), row, front[owners[j]].index)))
                if j + 1 == len(starts) or owners[j + 1] != owners[j]:
                    v, sample = heapq.heappop(leaf_queue)
                    heapq.heappush(results, (v, owners[j], sample))
                    leaf_queue = []
            candidates = [c[2] for c in new_candidates[:n]]
        if results:
            v, _, sample = results[0]
            return v, sample.row, sample.leaf, evaluations
        return np.inf, -1, 0, evaluations

    def descend(self, score, n_candidates=1):
        """descend_rows as (value, sample, leaf, evaluations): the sample a list, the root's mean when no leaf is reached."""
        value, row, leaf, evaluations = self.descend_rows(score, n_candidates)
        return value, (self.means[0].copy() if row < 0 else self.points[row].tolist()), leaf, evaluations

    # ---- the device copy --------------------------------------------------------------------------------------
    def _upload(self, prim):
        return _capi.KdClusterTree(prim, self.points, self.n_kd, self.child_begin, self.children, self.leaf, self.kd_begin, self.kd_roots,
                                   self.kd_left, self.kd_right, self.kd_inner)

    def result_of_record(self, rec):
        """(value, sample list) of a search record, or the reference's exception."""
        flags = self._flags_of_record(rec)
        if flags & _capi.MG_TREE_NO_MEAN:
            raise AttributeError(_NO_MEAN)
        if flags & _capi.MG_TREE_NO_RESULT:
            return np.inf, self.means[0].copy()
        return float(rec["value"]), self.points[int(rec["row"])].tolist()
