"""Matrices for the fused pass two's tests (tests/test_fused_pass_two_cpu.py,
tests/test_gpu_fused_pass_two.py): KKT-shaped blocks [[D, E^T], [E, 0]] — arc rows first, node
rows after — whose open-row sets have the shapes the row classes distinguish.
"""
import numpy as np
import scipy.sparse as sp


def kkt_from_arcs(n_nodes, tails, heads, d=None):
    """[[D, E^T], [E, 0]] for the arcs tails[i] -> heads[i] (E: +1 at the tail, -1 at the
    head; D = diag(d) or empty)."""
    m = len(tails)
    ar = np.arange(m)
    e = sp.coo_matrix((np.concatenate([np.ones(m), -np.ones(m)]),
                       (np.concatenate([tails, heads]), np.concatenate([ar, ar]))),
                      shape=(n_nodes, m)).tocsr()
    dd = sp.diags(np.asarray(d, dtype=np.float64)) if d is not None else sp.csr_matrix((m, m))
    a = sp.bmat([[dd, e.T], [e, None]], format="csr")
    a.sort_indices()
    return a


def hub_arcs(hubs, span=8):
    """Arcs among `hubs` hub nodes: hub i -> hub (i + s) % hubs, s = 1 .. span (each hub gets
    2 span arcs: a long row)."""
    t = np.repeat(np.arange(hubs), span)
    h = (t + np.tile(np.arange(1, span + 1), hubs)) % hubs
    return t, h


def kkt_hubs(hubs=30, leaves=0, d=False, span=8):
    """`hubs` hub nodes and `leaves` nodes of degree 1, each hanging on a hub by one arc."""
    t, h = hub_arcs(hubs, span)
    t = np.concatenate([t, hubs + np.arange(leaves)])
    h = np.concatenate([h, np.arange(leaves) % hubs])
    return kkt_from_arcs(hubs + leaves, t, h, 2.0 + np.arange(len(t)) % 3 if d else None)


def split_kkt(a, num_arcs):
    """(tails, heads, n_nodes) of a D = 0 KKT matrix with num_arcs arc rows."""
    e = a[num_arcs:, :num_arcs].tocsc()
    e.sort_indices()
    tails = np.empty(num_arcs, dtype=np.int64)
    heads = np.empty(num_arcs, dtype=np.int64)
    for j in range(num_arcs):
        rows = e.indices[e.indptr[j]:e.indptr[j + 1]]
        vals = e.data[e.indptr[j]:e.indptr[j + 1]]
        tails[j], heads[j] = rows[vals > 0][0], rows[vals < 0][0]
    return tails, heads, a.shape[0] - num_arcs


def without_leaf(kkt):
    """The KKT block without its degree-1 node and that node's arc: no open row."""
    t, h, nn = split_kkt(kkt.a, kkt.num_arcs)
    deg = np.bincount(np.concatenate([t, h]), minlength=nn)
    leaf = int(np.flatnonzero(deg == 1)[0])
    keep = (t != leaf) & (h != leaf)
    t, h = t[keep], h[keep]
    t, h = t - (t > leaf), h - (h > leaf)
    return kkt_from_arcs(nn - 1, t, h)


def with_low_degree_nodes(kkt):
    """The KKT block plus two nodes of degree 2 joined by an arc (open rows that reference
    open rows), and nodes of degree 2, 3 and 4 hanging on hubs: short node rows beside the
    width-2 arc rows."""
    t, h, nn = split_kkt(kkt.a, kkt.num_arcs)
    deg = np.bincount(np.concatenate([t, h]), minlength=nn)
    hubs = np.flatnonzero(deg > 8)[:16]
    p, q = nn, nn + 1
    extra = [(p, q), (p, hubs[0]), (hubs[1], q)]
    node = nn + 2
    for d in (2, 3, 4):
        extra += [(node, hubs[2 + i]) for i in range(d)]
        node += 1
    et, eh = np.array(extra).T
    return kkt_from_arcs(node, np.concatenate([t, et]), np.concatenate([h, eh]))


def with_d(kkt):
    """The KKT block with D = diag(2, 3, 4, 2, ...) on the arc rows: width-3 arc rows whose
    self column is closed."""
    m = kkt.num_arcs
    d = sp.diags(np.concatenate([2.0 + np.arange(m) % 3, np.zeros(kkt.a.shape[0] - m)]))
    a = (kkt.a + d).tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a
