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
    """-> (cols, rows) per front, leaves first; raises where the amalgamation arithmetic would merge a designed front.
    sp_ = 0 (and ng = 0): P is a root itself, there is no G."""
    assert ng >= sp_ and all(p[0] < rp and list(p) == sorted(set(p)) and p[-1] < rp + sp_ for p in leaves)
    assert all(nc < k and p[0] < rp and list(p) == sorted(set(p)) and p[-1] < rp + sp_ for nc, p in others), \
        "the poison sibling is the widest child; a child's first row is a column of P"
    # S into P (the first, widest child)
    z = k * (rp + sp_ - 1)
    assert z / _trap(rp + k, sp_) <= _allow(rp + k, True), "the poison sibling would stay out"
    true_p = _trap(rp + k, sp_) - z
    for nc, pos in [(1, p) for p in leaves] + list(others):
        tot = _trap(rp + k + nc, sp_)
        frac = (tot - true_p - _trap(nc, len(pos))) / tot
        assert frac > _allow(rp + k + nc, False), ("a child would merge into its parent", nc, len(pos), frac)
    if sp_:
        tot = _trap(rp + k + ng, 0)
        assert (tot - true_p - _trap(ng, 0)) / tot > _allow(rp + k + ng, True), "the parent would merge into the root"
    else:
        assert ng == 0
    # sibling bundles (symbolic.cpp, step 5) would put the children into supernodes of their own: by their number (more than
    # HIPKKT_BUNDLE_KIDS 200 under a front of <= 64 rows, HIPKKT_BUNDLE_KIDS_PANEL 400 per 96-column panel under a taller
    # one) or by their update blocks, together more than 16 times the parent's front (HIPKKT_BUNDLE_COST)
    kids, f = len(leaves) + len(others), rp + k + sp_
    assert kids <= 200 if f <= 64 else kids * min(1.0, 96 / (rp + k)) <= 400, "the children would be bundled by their number"
    assert sum(len(p) ** 2 for p in leaves) + sum(len(p) ** 2 for _, p in others) <= 16 * f * f, \
        "the children would be bundled by the size of their update blocks"
    cols, rows, c = [], [], 0
    sizes = [1] * len(leaves) + [nc for nc, _ in others] + [k, rp] + ([ng] if sp_ else [])
    for n in sizes:
        cols.append(list(range(c, c + n)))
        c += n
    pc, gc = (cols[-2], cols[-1]) if sp_ else (cols[-1], [])
    front = pc + gc[:sp_]
    for pos in list(leaves) + [p for _, p in others]:
        rows.append([front[i] for i in pos])
    rows += [[pc[0]], gc[:sp_]] + ([[]] if sp_ else [])
    return cols, rows


def make_case(cols, rows, seed, signs=None):
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
    if signs is not None:
        dsigns = np.asarray(signs, np.int64)          # (after the draw, as in front_shapes: the other values do not move)
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


# --------------------------------------------------------------------------- the many-column sweeps' pulled leaves
# (csrc/engine_tables.cpp, mark_solve_pulled: a leaf is pulled by the SOLVES when it has no children, one column, a parent, 1 <= nb <= 47
# rows and sits in a one-wave launch -- whatever its parent's class.)  Two things follow from the schedule and shape the
# cases:
#   * a one-column front of nb rows is one-wave only up to nb = 38 (f + nb^2 <= 1536), so nb = 39 .. 47 is a block-class
#     front, never in a one-wave launch and never pulled: the rule's bound of 47 cannot bind;
#   * a level with a block-class front keeps up to 128 one-wave fronts in that front's launch (merge_small): one such front
#     in level 0 and NO leaf of the tree is pulled.
W16_28 = dict(rp=4, sp_=28, ng=120, k=12)        # P' = (16, 28): one-wave; twelve poison columns so that tall leaves stay out
B16_29 = dict(rp=4, sp_=29, ng=120, k=12)        # P' = (16, 29): block-class
B40_65 = dict(rp=32, sp_=65, ng=120, k=8)        # P' = (40, 65): block-class, f = 105


def _rows_of(nb, shape, first=0):
    """nb positions of the parent's front: `first` (a column of P), the others spread over its columns and update rows."""
    f = shape["rp"] + shape["sp_"]
    if nb == 1:
        return [first]
    cand = list(range(first + 1, f))
    pos = [first] + [cand[int(i)] for i in np.round(np.linspace(0, len(cand) - 1, nb - 1))]
    assert len(set(pos)) == nb and pos == sorted(pos)
    return pos


def solve_cases():
    """name -> (cols, rows, expect): expect = (a, b, c) of the engine's "<a> of <b> contribution rows pulled from one-column
    leaves into <c> sums" line, from the construction: a = the pulled leaves' rows, b = the rows below every front that has
    a parent, c = the distinct parent rows the pulled leaves reach; plus `pulled`, the first columns of the pulled leaves."""
    T = {}

    def add(name, shape, leaves, others=(), pulled=None):
        cols, rows = tree(leaves=leaves, others=others, **shape)
        pulled = list(range(len(leaves))) if pulled is None else pulled
        a = sum(len(leaves[i]) for i in pulled)
        # (the root of ng > 96 columns is cut into a chain of equal panels, symbolic.cpp 7b: each link's rows are the
        #  columns of the links above it)
        parts = -(-shape["ng"] // 96)
        w = -(-shape["ng"] // parts)
        chain = sum(max(shape["ng"] - w * (i + 1), 0) for i in range(parts))
        b = sum(len(p) for p in leaves) + sum(len(p) for _, p in others) + shape["sp_"] + chain
        c = len({q for i in pulled for q in leaves[i]})
        T[name] = (cols, rows, dict(a=a, b=b, c=c, pulled=[cols[i][0] for i in pulled], shape=shape))

    # leaf heights around the chunks of eight of k_bwd_leaf_m (1, 8, 9) and the tallest one-wave single column (38; 31 under
    # the 32-row front of (16, 28)), rows in the parent's columns AND its update rows (i >= nc), under a one-wave parent
    # and two block-class ones
    for name, shape, tall in (("heights_16_28", W16_28, 31), ("heights_16_29", B16_29, 32), ("heights_40_65", B40_65, 38)):
        add(name, shape, [_rows_of(nb, shape, first=i % shape["rp"]) for i, nb in enumerate((tall, 1, 8, 9))])
    # 1, 3, 4, 5 and 9 leaves on one parent row (pr_ptr is walked in chunks of four), each count on a column row p and on
    # an update row 40 + p of P' = (40, 65)
    many = []
    for p, n in enumerate((1, 3, 4, 5, 9)):
        many += [[p, 40 + p]] * n
    add("counts_40_65", B40_65, many)
    add("counts_16_28", W16_28, [[p, 20 + p] for p, n in enumerate((1, 3, 4)) for _ in range(n)] + [[3]] * 5)
    # one parent row with pulled terms only (0, 2), one with pulled terms and a stored contribution of a regular child (1:
    # the sum takes the first slot of the row's run), rows with stored contributions only (3, 50 / 25)
    add("slots_40_65", B40_65, [[0, 1], [1, 2]], others=[(2, [1, 3, 50])])
    add("slots_16_28", W16_28, [[0, 1], [1, 2]], others=[(2, [1, 3, 25])])
    # nb = 39, 47 and 48: block-class leaves, and with them in level 0 the short leaves ride in their launch -- nothing pulled
    add("ride_40_65", B40_65, [_rows_of(nb, B40_65) for nb in (1, 8, 39, 47, 48)], pulled=[])
    # no leaf at all: gather lists of 5, 4, 3, 1 and 0 STORED contributions (k_fwd_wave_m sums them four at a time) on rows
    # of a one-wave parent of 17 columns -- a row among its first 16 own unknowns (8), its 17th (16: past kWC) and update rows
    add("gather_17_24", dict(rp=9, sp_=24, ng=40, k=8), [],
        others=[(2, [0, 8, 20, 30]), (2, [0, 8, 20]), (2, [0, 8, 20]), (2, [0, 8]), (2, [0])])
    return T


def solve_case(name, seed=1):
    cols, rows, _ = solve_cases()[name]
    return make_case(cols, rows, seed)


def write_pattern(K, path):
    K = sp.csc_matrix(K)
    with open(path, "wb") as f:
        np.array([K.shape[0], K.nnz], dtype=np.int64).tofile(f)
        K.indptr.astype(np.int64).tofile(f)
        K.indices.astype(np.int64).tofile(f)
