"""Trees for the pulled-leaf tests: one-column leaves with CHOSEN rows under a parent of a chosen shape.

tests/front_shapes.py places a child's rows on the first positions of its parent's front; a leaf that straddles the
panel / update boundary or a 64-row tile boundary of its parent needs rows anywhere in that front, so the pattern is built
here, with front_shapes' value rule (strict diagonal dominance, known x_true, exact b, a-priori condition bound) and its
Case record, error measures and bounds.

A tree is, in elimination order (ORDER_NATURAL):
    leaves      one column each, rows = chosen positions of P's front (P's columns, then P's rows), the first in a column
    others      regular children of P: (nc, positions), dense columns
    S           (k, 1): a poison sibling, its row P's first column
    P           (rp, sp): the parent, its rows the first sp columns of G
    G           (ng, 0): the root
Relaxed amalgamation (csrc/symbolic.cpp, step 5) tries P's widest child first with twice the allowance: S merges and
leaves P' = (rp + k, sp) with k (rp + sp - 1) explicit zeros, after which every leaf (and P' into G) would push the zero
fraction over the allowance and stays out -- `tree` checks that arithmetic and the host test checks the outcome.  In P''s
front the positions move up by k."""
import numpy as np
import scipy.sparse as sp

from tests import front_shapes as fs


def _trap(nc, nb):
    return nc * (nc + 1) / 2 + nc * nb


def _allow(width, first):
    for c, z in zip((8, 32, 128), (1.0, 0.5, 0.15)):
        if width <= c:
            return z * (2.0 if first else 1.0)
    return 0.05 * (2.0 if first else 1.0)


def tree(rp, sp_, ng, k, leaves, others=()):
    """-> (cols, rows) per front, leaves first; raises where the amalgamation arithmetic would merge a designed front."""
    assert ng >= sp_ and all(p[0] < rp and list(p) == sorted(set(p)) and p[-1] < rp + sp_ for p in leaves)
    # S into P (the first, widest child)
    z = k * (rp + sp_ - 1)
    assert z / _trap(rp + k, sp_) <= _allow(rp + k, True), "the poison sibling would stay out"
    true_p = _trap(rp + k, sp_) - z
    for nc, pos in [(1, p) for p in leaves] + list(others):
        tot = _trap(rp + k + nc, sp_)
        frac = (tot - true_p - _trap(nc, len(pos))) / tot
        assert frac > _allow(rp + k + nc, False), ("a child would merge into its parent", nc, len(pos), frac)
    tot = _trap(rp + k + ng, 0)
    assert (tot - true_p - _trap(ng, 0)) / tot > _allow(rp + k + ng, True), "the parent would merge into the root"
    cols, rows, c = [], [], 0
    sizes = [1] * len(leaves) + [nc for nc, _ in others] + [k, rp, ng]
    for n in sizes:
        cols.append(list(range(c, c + n)))
        c += n
    pc, gc = cols[-2], cols[-1]
    front = pc + gc[:sp_]
    for pos in list(leaves) + [p for _, p in others]:
        rows.append([front[i] for i in pos])
    rows += [[pc[0]], gc[:sp_], []]
    return cols, rows


def make_case(cols, rows, seed):
    """front_shapes.make_case for explicit (cols, rows) lists."""
    from cuclarabel_amd import _lib
    rng = np.random.default_rng(seed)
    I, J = [], []
    for cs, rs in zip(cols, rows):
        cs = np.asarray(cs, dtype=np.int64)
        ii, jj = np.triu_indices(len(cs))
        I.append(cs[ii]); J.append(cs[jj])
        if rs:
            a, r = np.meshgrid(cs, np.asarray(rs, dtype=np.int64), indexing="ij")
            I.append(a.ravel()); J.append(r.ravel())
    I, J = np.concatenate(I), np.concatenate(J)
    N = cols[-1][-1] + 1
    cnt = np.zeros(N)
    np.add.at(cnt, I, 1)
    np.add.at(cnt, J, 1)
    off = I != J
    scale = 1.0 / np.sqrt(np.maximum(cnt, 1))
    v = rng.uniform(-1.0, 1.0, I.size) * np.minimum(scale[I], scale[J])
    rowsum = np.zeros(N)
    np.add.at(rowsum, I[off], np.abs(v[off]))
    np.add.at(rowsum, J[off], np.abs(v[off]))
    dsigns = np.where(rng.random(N) < 0.5, -1, 1).astype(np.int64)
    d = ~off
    v[d] = dsigns[I[d]] * (1.0 + rowsum[I[d]] + rng.uniform(0.0, 0.5, d.sum()))
    K = sp.csc_matrix((v, (I, J)), shape=(N, N))
    K.sort_indices()
    margin = (np.abs(K.diagonal()) - rowsum).min()
    x_true = rng.standard_normal(N)
    b = fs.symmetric_matvec_ld(K, x_true).astype(np.float64)
    return fs.Case(K=K, dsigns=dsigns, ordering=_lib.ORDER_NATURAL, x_true=x_true, b=b,
                   cond_bound=fs.norm_inf_sym(K) / margin, cols=cols, rows=rows, Kt=K)


def _spread(nb, rp, f):
    """nb positions of a front of f rows: the first in the panel, the others spread over panel and update rows."""
    pos = sorted({int(round(x)) for x in np.linspace(1, f - 2, nb)})
    pos[0] = min(pos[0], rp - 1)
    assert len(pos) == nb
    return pos


P48 = dict(rp=40, sp_=60, ng=100, k=8)           # P' = (48, 60): f = 108, one tile row


def cases():
    """name -> (cols, rows, leaves, terms, parent is block-class): the leaves and the terms a handle must report pulled
    (0 where the parent is a one-wave front)."""
    T = {}

    def add(name, shape, leaves, others=(), block=True):
        cols, rows = tree(leaves=leaves, others=others, **shape)
        n = len(leaves) if block else 0
        T[name] = (cols, rows, n, sum(len(p) * (len(p) + 1) // 2 for p in leaves) if block else 0, block)

    f = 100
    # leaf heights: the tiny class and its edge (f = 8: nb = 7), the first k_front_wave leaf (nb = 8), the tallest level-0
    # single column of cfg2 (nb = 35); rows in the panel and in the update block (a leaf straddles that boundary)
    add("heights", P48, [[0], [39], _spread(7, 40, f), _spread(7, 40, f), _spread(8, 40, f), [3] + list(range(38, 45)),
                         _spread(35, 40, f), [39] + list(range(40, 74))])
    # the one-wave / block-class boundary of the PARENT: f * nc + nb^2 <= 1536 holds for (16, 28), not for (16, 29); and a
    # front of f = 64 is block-class like one of 65 (no (nc, nb) with f = 64 meets the one-wave rule)
    few = [[0, 1, 2], [2, 7, 10], [5, 6, 20], [7, 9, 11]]
    add("parent_16_28", dict(rp=8, sp_=28, ng=120, k=8), few, block=False)
    add("parent_16_29", dict(rp=8, sp_=29, ng=120, k=8), few)
    add("parent_f64", dict(rp=12, sp_=40, ng=120, k=12), few)
    add("parent_f65", dict(rp=12, sp_=41, ng=120, k=12), few)
    # a parent with two tile rows (nb = 120): leaves on rows 63 and 64 of U -- entries in the diagonal tiles (0, 0) and
    # (1, 1) and in the off-diagonal tile (1, 0) -- and on the panel / update boundary
    P120 = dict(rp=40, sp_=120, ng=160, k=8)
    add("tile_edge", P120, [[5, 40 + 63, 40 + 64], [39, 40, 40 + 63, 40 + 64, 40 + 119], [0, 40 + 64], [39, 40]])
    # stacks: 70 and 130 leaves on the same parent entries (more than a wave, more than sixteen in flight, fewer than a
    # sibling bundle takes: HIPKKT_BUNDLE_KIDS_PANEL 400) -- a wave with more than 64 terms, other waves and tiles with none
    add("stack_70", P48, [[0, 1]] * 70)
    add("stack_130", P48, [[3, 45]] * 130)
    # pulled leaves beside regular children (two columns; one column with children of its own is not built here: a
    # one-column front with a child merges) and a dense child (P' = 120 columns is cut into two panels: the lower
    # one's update block is the upper one's whole front); the leaves hang under both panels
    wide = dict(rp=100, sp_=60, ng=100, k=20)
    add("mixed", wide, [[0, 1, 2], [10, 70, 120], [60, 61, 159], [99, 100], [70, 101, 158], [50, 51]],
        others=[(2, [4, 6, 80, 130]), (3, [65, 66, 140])])
    return T


def case(name, seed=1):
    cols, rows, *_ = cases()[name]
    return make_case(cols, rows, seed)


def write_pattern(K, path):
    K = sp.csc_matrix(K)
    with open(path, "wb") as f:
        np.array([K.shape[0], K.nnz], dtype=np.int64).tofile(f)
        K.indptr.astype(np.int64).tofile(f)
        K.indices.astype(np.int64).tofile(f)
