"""Plain restatement of the contact clusters (rt_contact_clusters) over a prepared scene's L (oracle_lib.OracleScene(...).arrays() or
Prepared.bvh_arrays()): the connected components of the graph whose vertices are the spheres L[0 .. n) and whose edges are exactly
within_ref.contact_pairs(L, margin)'s rows -- the one-sided float32 predicate, evaluated from the lower index.

The answer is (root [n] int32, cluster [n] int32, size [n] int32, num int): root[i] the smallest index in i's component, cluster[i] the rank
of root[i] among the roots (a dense id in [0, num), ascending with the root), size[i] the component's vertex count, num the number of
components.  Two independent routes: clusters() is a sequential union-find over the pair rows, clusters_by_labels() propagates the smallest
label along the edges in numpy until nothing changes.  The CPU suite holds the two equal.
"""
import numpy as np

import within_ref as W


def pairs(L, margin, near=False):
    """the edges: within_ref.contact_pairs's rows, [total, 2] int32"""
    return W.contact_pairs(L, margin, near=near)[0]


def from_roots(root):
    """(root, cluster, size, num) from the [n] roots (each the smallest index of its component)"""
    root = np.asarray(root, np.int32)
    n = root.shape[0]
    is_root = root == np.arange(n, dtype=np.int32)
    rank = np.cumsum(is_root) - is_root            # the number of roots below each index
    cluster = rank[root].astype(np.int32)
    size = np.bincount(root, minlength=n)[root].astype(np.int32)
    return root, cluster, size, int(is_root.sum())


def roots_union_find(n, edges):
    """sequential union-find over the [m, 2] edges, in order: [n] int32, the smallest index of every component"""
    parent = list(range(n))
    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.empty(n, np.int32)
    for i in range(n):                             # (parent[i] < i for every non-root, so parent[i]'s entry is already final)
        root[i] = i if parent[i] == i else root[parent[i]]
    return root


def roots_by_labels(n, edges):
    """min-label propagation: every vertex takes the smallest label among itself and its neighbours, with pointer jumping, until a sweep
    changes nothing"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, e[:, 0], label[e[:, 1]])
        np.minimum.at(new, e[:, 1], label[e[:, 0]])
        new = new[new]                             # a label is a vertex of the same component: its label is one too
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def clusters(L, margin, near=False):
    """(root, cluster, size, num): the sequential union-find over within_ref.contact_pairs(L, margin)"""
    return from_roots(roots_union_find(np.asarray(L).shape[0], pairs(L, margin, near)))


def clusters_by_labels(L, margin, near=False):
    """(root, cluster, size, num): min-label propagation over the same edges"""
    return from_roots(roots_by_labels(np.asarray(L).shape[0], pairs(L, margin, near)))


def is_coarsening(fine_root, coarse_root):
    """every component of the fine partition lies inside one component of the coarse partition"""
    fine_root, coarse_root = np.asarray(fine_root), np.asarray(coarse_root)
    return bool(np.array_equal(coarse_root, coarse_root[fine_root]))
