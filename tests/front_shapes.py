"""Matrices whose supernodal fronts have CHOSEN shapes, for the level-A (hipkkt_ldl_*) boundary tests.

A case is a forest of supernodes listed children first: ``(nc, nb, parent)`` is a front of ``nc`` dense columns whose
``nb`` rows below are the first ``nb`` positions of its parent's front (the parent's columns, then the parent's own
rows).  The columns are numbered in that order, so ORDER_NATURAL's elimination order is the listed one.

Two parts of the symbolic phase (csrc/symbolic.cpp) change shapes on their own:

* Relaxed amalgamation merges a child into its parent when the merged front has few explicit zeros: any merged front
  of <= 32 columns always, wider ones when the zero fraction stays under 0.3 (<= 128 columns) or 0.1 (the allowances of
  the tallest child, which is tried first; the others get half of them).  Two constructions keep a designed front
  T = (nc, nb) apart:
  - ``designed``: T hangs below a narrow, tall STICK P = (rp, sp) that T's rows fill only in part; P itself is
    absorbed by the root G = (sp + 1, 0) above it afterwards, but a child's decision is never revisited, so T stays.
    ``stick`` finds the smallest such P.  This needs nc >= ~10 (T's zero fraction is at most ~nc / (nc + rp)).
  - ``beside_sibling``, for narrow fronts: P = (1, R) first absorbs a wider sibling S = (20, 1) (the widest child is
    tried first, with the larger allowance).  P then carries S's explicit zeros, and the merge test counts them: T,
    tried second with the plain allowance, would make P's front mostly zeros and stays out -- (1, 38), (2, 6) ...
* Sibling bundles act on more than 200 one-wave children of one parent: the many-front cases are forests of roots.

Values: off-diagonal entries are uniform in (-s, s) with s = 1 / sqrt(rows), the diagonal is sign * (1 + |row|_1)
with a random sign per column.  K is then strictly diagonally dominant, hence quasi-definite in every order (no pivot
changes sign), and no eigenvalue lies in (-m, m) for the smallest dominance margin m (K - mu I stays dominant), which
gives cond_2(K) <= |K|_inf / m a priori.
"""
import dataclasses

import numpy as np
import scipy.sparse as sp

U = np.finfo(np.float64).eps / 2          # unit round-off

# csrc/symbolic.hpp SymbolicOptions: relax_cols {8, 32, 128}, relax_zeros {1.0, 0.5, 0.15, 0.05}, relax_tall 2.0
_RELAX_COLS = (8, 32, 128)
_RELAX_ZEROS = (1.0, 0.5, 0.15, 0.05)
_RELAX_TALL = 2.0

# shapes of the issue's table that no matrix produces, with the reason
UNREACHABLE = {
    "nb = 0 at a non-root":
        "a supernode's parent is the one that holds its first row below (elimination tree): with no rows below it is a "
        "root.  The cases place (nc, 0) roots in a level beside non-roots instead",
}


def _trap(nc, nb):
    return nc * (nc + 1) / 2 + nc * nb


def _allowance(width, tall=True):
    z = _RELAX_ZEROS[3]
    for c, zz in zip(_RELAX_COLS, _RELAX_ZEROS):
        if width <= c:
            z = zz
            break
    return z * (_RELAX_TALL if tall else 1.0)


def stays_separate(nc, nb, rp, sp):
    """Would a dense (nc, nb) child stay out of its only parent (rp, sp)?  (symbolic.cpp step 5)"""
    if nb >= rp + sp:
        return False                      # fundamental supernode with its parent
    frac = nc * (rp + sp - nb) / _trap(nc + rp, sp)
    return frac > _allowance(nc + rp)


def stick(nc, nb):
    """Smallest stick (rp, sp) above which a designed (nc, nb) front survives amalgamation, or None (a narrow front:
    use beside_sibling)."""
    best = None
    for rp in range(1, 130):
        for sp in range(max(nb - rp + 1, 1), 1200):
            if stays_separate(nc, nb, rp, sp):
                if best is None or rp + sp < sum(best):
                    best = (rp, sp)
                break
    return best


def designed(nc, nb, copies=1, st=None):
    """Spec of `copies` independent trees, each: the (nc, nb) front, a stick P = st (default: stick(nc, nb)) above it
    and the root G above P.  nb = 0: `copies` independent (nc, 0) roots."""
    spec = []
    for _ in range(copies):
        if nb == 0:
            spec.append((nc, 0, -1))
            continue
        st = st or stick(nc, nb)
        if st is None or not stays_separate(nc, nb, *st):
            raise ValueError(f"({nc}, {nb}) cannot be placed (see UNREACHABLE)")
        rp, sp = st
        b = len(spec)
        spec += [(nc, nb, b + 1), (rp, sp, b + 2), (sp + 1, 0, -1)]
    return spec


def beside_sibling(nc, nb, R=40):
    """Spec of one tree for a narrow (nc, nb) front: T and a wider sibling S = (20, 1) below P = (1, R), below the root
    G = (R + 1, 0).  S merges into P first; T stays out (see the module docstring).  nb <= R."""
    if not 0 < nb <= R:
        raise ValueError("0 < nb <= R")
    return [(nc, nb, 2), (20, 1, 2), (1, R, 3), (R + 1, 0, -1)]


@dataclasses.dataclass
class Case:
    K: sp.csc_matrix                 # upper triangle, CSC, explicit zeros kept
    dsigns: np.ndarray
    ordering: int
    x_true: np.ndarray
    b: np.ndarray                    # K~ x_true accumulated in long double, rounded once
    cond_bound: float
    cols: list                       # per spec entry: its column indices
    rows: list                       # per spec entry: its row indices below (absolute)
    Kt: sp.csc_matrix = None         # K~: K with the regularised pivots replaced (== K when there are none)


def layout(spec):
    """Column and row index lists of every spec entry."""
    cols, rows, c = [], [None] * len(spec), 0
    for nc, _, _ in spec:
        cols.append(list(range(c, c + nc)))
        c += nc
    # parents come after their children: fill rows top-down
    for s in range(len(spec) - 1, -1, -1):
        nc, nb, p = spec[s]
        if p < 0:
            if nb:
                raise ValueError("a root has no rows below it")
            rows[s] = []
            continue
        if p <= s:
            raise ValueError("children must be listed before their parents")
        front = cols[p] + rows[p]
        if nb > len(front) - 1:
            raise ValueError(f"entry {s}: nb {nb} exceeds its parent's front less one")
        rows[s] = front[:nb]
    return cols, rows, c


def pattern(spec):
    """(rows, cols) of the upper triangle (row <= col)."""
    cols, rows, N = layout(spec)
    I, J = [], []
    for cs, rs in zip(cols, rows):
        cs = np.asarray(cs, dtype=np.int64)
        ii, jj = np.triu_indices(len(cs))
        I.append(cs[ii]); J.append(cs[jj])
        if rs:
            a, r = np.meshgrid(cs, np.asarray(rs, dtype=np.int64), indexing="ij")
            I.append(a.ravel()); J.append(r.ravel())
    return np.concatenate(I), np.concatenate(J), N, cols, rows


def symmetric_matvec_ld(K, x):
    """K_full @ x in long double from the upper triangle K (CSC)."""
    K = sp.coo_matrix(K)
    xl = np.asarray(x, dtype=np.longdouble)
    v = K.data.astype(np.longdouble)
    y = np.zeros(K.shape[0], dtype=np.longdouble)
    np.add.at(y, K.row, v * xl[K.col])
    off = K.row != K.col
    np.add.at(y, K.col[off], v[off] * xl[K.row[off]])
    return y


_LD_CSR = {}


def symmetric_matmat_ld(K, X):
    """K_full @ X in long double from the upper triangle K, for a block of columns: every product and sum in long double,
    as symmetric_matvec_ld does column by column (scipy's CSR product in extended precision; the order of a row's sums
    differs from symmetric_matvec_ld's, both are exact to ~1e-19 relative).  The extended copy of K is kept per matrix."""
    key = id(K)
    if key not in _LD_CSR or _LD_CSR[key][0] is not K:
        _LD_CSR[key] = (K, full(K).tocsr().astype(np.longdouble))
    Y = _LD_CSR[key][1] @ np.asarray(X, dtype=np.longdouble)
    assert Y.dtype == np.longdouble
    return Y


def errors_columns(case, X, Xt, B):
    """errors() for the columns of X against known Xt and right-hand sides B: (forward errors, backward errors)."""
    xt = np.abs(Xt).max(axis=0)
    fwd = np.abs(X - Xt).max(axis=0) / np.where(xt > 0, xt, 1.0)
    Bl = np.asarray(B, np.longdouble)
    R = np.abs(Bl - symmetric_matmat_ld(case.Kt, X)).max(axis=0)
    den = np.longdouble(norm_inf_sym(case.Kt)) * np.abs(X).max(axis=0).astype(np.longdouble) + np.abs(Bl).max(axis=0)
    return fwd, (R / np.where(den > 0, den, 1)).astype(np.float64)


def norm_inf_sym(K):
    K = sp.coo_matrix(K)
    a = np.abs(K.data)
    r = np.zeros(K.shape[0])
    np.add.at(r, K.row, a)
    off = K.row != K.col
    np.add.at(r, K.col[off], a[off])
    return r.max()


def full(K):
    """The symmetric matrix of the upper triangle K, as CSC (explicit zeros kept)."""
    K = sp.csc_matrix(K)
    return (K + sp.triu(K, 1, format="csc").T).tocsc()


def make_case(spec, seed, ordering=None, signs=None):
    """Matrix, signs, ordering, x_true, b and a condition bound for a spec (see the module docstring)."""
    from cuclarabel_amd import _lib
    rng = np.random.default_rng(seed)
    I, J, N, cols, rows = pattern(spec)
    cnt = np.zeros(N)
    np.add.at(cnt, I, 1)
    np.add.at(cnt, J, 1)
    off = I != J
    scale = 1.0 / np.sqrt(np.maximum(cnt, 1))
    v = rng.uniform(-1.0, 1.0, I.size) * np.minimum(scale[I], scale[J])
    rowsum = np.zeros(N)
    np.add.at(rowsum, I[off], np.abs(v[off]))
    np.add.at(rowsum, J[off], np.abs(v[off]))
    dsigns = np.where(rng.random(N) < 0.5, -1, 1).astype(np.int64) if signs is None else np.asarray(signs, np.int64)
    d = ~off
    v[d] = dsigns[I[d]] * (1.0 + rowsum[I[d]] + rng.uniform(0.0, 0.5, d.sum()))
    K = sp.csc_matrix((v, (I, J)), shape=(N, N))
    K.sort_indices()
    margin = (np.abs(K.diagonal()) - rowsum).min()
    x_true = rng.standard_normal(N)
    b = symmetric_matvec_ld(K, x_true).astype(np.float64)
    return Case(K=K, dsigns=dsigns, ordering=_lib.ORDER_NATURAL if ordering is None else ordering, x_true=x_true, b=b,
                cond_bound=norm_inf_sym(K) / margin, cols=cols, rows=rows, Kt=K)


def set_pivots(case, pivots, eps, delta):
    """Pivot-rule cases.  For each (column k, value, sign): row k becomes an explicit zero in every column eliminated
    before k (ORDER_NATURAL on these matrices eliminates in index order), so that the pivot met at k is exactly the
    value put on the diagonal; the sign goes into dsigns.  K~ is K with sign * delta on the diagonal where
    value * sign < eps (the rule is a strict <).  b, K~ and the condition number (measured) are rebuilt."""
    K = sp.coo_matrix(case.K)
    I, J, v = K.row.astype(np.int64), K.col.astype(np.int64), K.data.copy()
    vt = None
    for k, val, sg in pivots:
        v[(J == k) & (I < k)] = 0.0
        v[(I == k) & (J == k)] = val
        case.dsigns[k] = sg
    vt = v.copy()
    for k, val, sg in pivots:
        if val * sg < eps:
            vt[(I == k) & (J == k)] = sg * delta
    N = case.K.shape[0]
    case.K = sp.csc_matrix((v, (I, J)), shape=(N, N))
    case.Kt = sp.csc_matrix((vt, (I, J)), shape=(N, N))
    case.K.sort_indices()
    case.Kt.sort_indices()
    case.b = symmetric_matvec_ld(case.Kt, case.x_true).astype(np.float64)
    case.cond_bound = float(np.linalg.cond(full(case.Kt).toarray()))
    return case


def errors(case, x):
    """(forward error |x - x_true|_inf / |x_true|_inf, long-double backward error |b - K~ x| / (|K~||x| + |b|))."""
    fwd = np.abs(x - case.x_true).max() / np.abs(case.x_true).max()
    r = np.asarray(case.b, dtype=np.longdouble) - symmetric_matvec_ld(case.Kt, x)
    bwd = float(np.abs(r).max() / (np.longdouble(norm_inf_sym(case.Kt)) * np.abs(np.asarray(x, np.longdouble)).max()
                                   + np.abs(np.asarray(case.b, np.longdouble)).max()))
    return float(fwd), bwd


def reference_solve(case, K=None):
    """scipy's sparse LU solve of K~ (or K) x = b in fp64."""
    import scipy.sparse.linalg as spla
    A = full(case.Kt if K is None else K)
    return spla.splu(A.tocsc(), permc_spec="COLAMD").solve(case.b)


def forward_bound(case, scipy_fwd):
    return max(100.0 * case.cond_bound * U, 10.0 * scipy_fwd)


BWD_BOUND = 64 * U


# --------------------------------------------------------------------------- the shape table
# name -> (spec, expected level 0 (count, fmax, ncmax, n_f<=8, n_f<=64), intended class of the designed front)
# class: "tiny" (f <= 8), "wave" (one-wave: f <= 64 and f*nc + nb^2 <= 1536), "block" (panel kernel), "chain" (a
# supernode wider than a panel, cut into links), "sliced" (row slices)
def _one_wave(nc, nb):
    f = nc + nb
    return f <= 64 and f * nc + nb * nb <= 1536


def _roots(nc, copies):
    f = nc
    return designed(nc, 0, copies), (copies, f, nc, copies * (f <= 8), copies * (f <= 64))


def _child(nc, nb, copies=1):
    f = nc + nb
    return designed(nc, nb, copies), (copies, f, nc, copies * (f <= 8), copies * (f <= 64))


def _narrow(nc, nb):
    f = nc + nb
    return beside_sibling(nc, nb), (1, f, nc, int(f <= 8), int(f <= 64))


def _mixed(n_small, small=(39, 0), big=(96, 0)):
    spec = [small + (-1,)] * n_small + [big + (-1,)]
    return spec, (n_small + 1, big[0], big[0], 0, n_small)


def shape_table():
    T = {}
    for nc in (1, 2, 8, 9):
        T[f"f{nc}_root"] = _roots(nc, 3) + ("tiny" if nc <= 8 else "wave",)
    # tiny and one-wave fronts WITH update rows (extend-add into a parent): f = 2, 8, 9, and the binding clause of the
    # one-wave rule at one column, f * nc + nb^2 = 39 + 1444 <= 1536 < 40 + 1521
    T["tiny_1_1"] = _narrow(1, 1) + ("tiny",)
    T["tiny_2_6"] = _narrow(2, 6) + ("tiny",)
    T["wave_1_8"] = _narrow(1, 8) + ("wave",)
    T["wave_1_38"] = _narrow(1, 38) + ("wave",)
    T["block_1_39"] = _narrow(1, 39) + ("block",)
    T["wave_39_0"] = _roots(39, 2) + ("wave",)
    T["block_40_0"] = _roots(40, 2) + ("block",)
    T["wave_16_28"] = _child(16, 28) + ("wave",)
    T["block_16_29"] = _child(16, 29) + ("block",)
    T["merge_128"] = _mixed(128) + ("wave+block",)
    T["merge_129"] = _mixed(129) + ("wave+block",)
    for nc in (15, 16, 17, 31, 32, 33, 95, 96):
        T[f"panel_nc{nc}"] = _child(nc, 40) + ("block",)
    for nb in (1, 63, 64, 65, 127, 128, 129, 192, 193):
        T[f"schur_nb{nb}"] = _child(40, nb) + ("block",)
    for f in (128, 129, 192, 193):
        T[f"bs_f{f}"] = _child(64, f - 64) + ("block",)
    T["trap_96_151"] = _child(96, 151) + ("block",)
    return T


# fronts whose designed supernode is cut by the symbolic split (7b): name -> (spec, level-0 tuple, class)
def chain_table():
    T = {}
    # 97 columns: two links, (49, 48 + 40) and (48, 40)
    T["chain_nc97"] = (designed(97, 40), (1, 137, 49, 0, 0), "chain")
    # one past the trapezoid cap (96 * 97 / 2 + 96 * 152 > 19 200): two links of 48 columns
    T["trap_96_152"] = (designed(96, 152), (1, 248, 48, 0, 0), "chain")
    return T


def solve_bs_table():
    # (the schedule summary does not report the sweep's workgroup size: these two cases show that both sides of the
    #  solve_bs switch -- 1023 fronts on 256-thread, 1024 on 128-thread workgroups -- solve correctly, not which one
    #  each took)
    return {f"solve_bs_{n}": (designed(40, 0, n), (n, 40, 40, 0, n), "block") for n in (1023, 1024)}


# --------------------------------------------------------------------------- forests for the sweep-path tests
# (tests/test_gpu_sweep_paths.py): the constructors above side by side, so that a LEVEL holds a chosen number of fronts
# of chosen classes, and towers tall enough for a chained range below a persistent set.
def forest(*parts):
    """Independent trees side by side: the specs concatenated, parent indices shifted."""
    spec = []
    for part in parts:
        b = len(spec)
        spec += [(nc, nb, p if p < 0 else p + b) for nc, nb, p in part]
    return spec


def tower(links):
    """One tree that is a chain of fronts, lowest first: links = [(nc, nb), ..., (nc, 0)].  A link's nb rows are the
    first nb columns of the link above it; every link must stay out of the one above (stays_separate)."""
    for (nc, nb), (rp, sp) in zip(links, links[1:]):
        if nb > rp or not stays_separate(nc, nb, rp, sp):
            raise ValueError(f"link ({nc}, {nb}) would merge into ({rp}, {sp})")
    if links[-1][1] != 0:
        raise ValueError("the last link is the root")
    return [(nc, nb, i + 1 if i + 1 < len(links) else -1) for i, (nc, nb) in enumerate(links)]


# A tree with the fronts that SURVIVE amalgamation, per level (leaves = level 0), as (f, nc) pairs -- from the
# constructions' own reasoning, not from the symbolic phase: test_front_shapes_host compares.
def _t_root(nc):
    return [(nc, 0, -1)], [[(nc, nc)]]


def _t_designed(nc, nb):
    st = stick(nc, nb)
    return designed(nc, nb, st=st), [[(nc + nb, nc)], [(sum(st) + 1, sum(st) + 1)]]        # T; the stick merged into its root


def _t_sibling(nc, nb, R=40):
    return beside_sibling(nc, nb, R), [[(nc + nb, nc)], [(21 + R, 21)], [(R + 1, R + 1)]]    # T; P with S absorbed; G


def _t_tower(links):
    return tower(links), [[(nc + nb, nc)] for nc, nb in links]


def _grow(klass_, *trees):
    """(spec, per level (count, fmax, ncmax, n_f<=8, n_f<=64), class) of the trees side by side."""
    depth = max(len(t[1]) for t in trees)
    lev = [[fr for t in trees if l < len(t[1]) for fr in t[1][l]] for l in range(depth)]
    tup = tuple((len(v), max(f for f, _ in v), max(nc for _, nc in v), sum(f <= 8 for f, _ in v), sum(f <= 64 for f, _ in v))
                for v in lev)
    return forest(*[t[0] for t in trees]), tup, klass_


def _tiny_group(n):
    """n tiny fronts in level 0, f in {1, 2, 8} mixed: the first two with update rows (f = 8: (2, 6), f = 2: (1, 1)),
    the others roots of 1, 2 and 8 columns in turn."""
    with_rows = [_t_sibling(2, 6), _t_sibling(1, 1)][:min(n, 2)]
    return with_rows + [_t_root((1, 2, 8)[i % 3]) for i in range(n - len(with_rows))]


# the two lowest levels hold one-wave fronts only (launches of their own), the three above block-class fronts (the
# persistent set): five launches, the chained range [0, 2) below the set
_TOWER = [(20, 4), (20, 4), (40, 4), (40, 4), (40, 0)]


def sweep_table():
    """name -> (spec, level tuples of EVERY level, classes in level 0)."""
    T = {}
    # tiny fronts: eight to a wave, so counts around 8 and 32 (a 256-thread workgroup's worth)
    for n in (1, 7, 8, 9, 31, 32, 33):
        T[f"tiny_n{n}"] = _grow("tiny", *_tiny_group(n))
    # one-wave fronts: four to a 256-thread workgroup
    for n in (3, 4, 5):
        T[f"wave9_n{n}"] = _grow("wave", *[_t_root(9)] * n)
        T[f"wave39_n{n}"] = _grow("wave", *[_t_root(39)] * n)
        T[f"wave_16_28_n{n}"] = _grow("wave", *[_t_designed(16, 28)] * n)
        T[f"wave_1_38_n{n}"] = _grow("wave", *[_t_sibling(1, 38)] * n)
    # all three classes in one level: few enough one-wave fronts to ride in the block-class launch (merge_small), and
    # one more than that (129 = 96 one-wave + 33 tiny: a launch of their own beside the block-class one)
    T["mixed_few"] = _grow("tiny+wave+block", *_tiny_group(9), *[_t_root(39)] * 5, _t_root(96))
    T["mixed_129"] = _grow("tiny+wave+block", *_tiny_group(33), *[_t_root(9)] * 96, _t_root(40), _t_root(40))
    # taller trees
    T["tall_wave"] = _grow("wave", _t_tower(_TOWER), _t_tower(_TOWER))
    # ... with a level 0 of all three classes (one block-class launch: the small ones ride along), one-wave fronts alone
    # in level 1: the chained range holds a block-class launch
    T["tall_mixed"] = _grow("tiny+wave+block", _t_tower(_TOWER), _t_tower(_TOWER), _t_root(40), _t_root(40),
                            _t_root(1), _t_root(2), _t_root(8))
    return T


# cases of the shape table that ride along in the sweep-path tests: the merge_small threshold, a workgroup-size edge,
# a chain of panels and the widest trapezoid
SWEEP_EXTRA = ("merge_128", "merge_129", "bs_f129", "chain_nc97", "trap_96_151")


def sweep_cases():
    T = {n: c for n, c in sweep_table().items()}
    A = all_cases()
    T.update({n: A[n] for n in SWEEP_EXTRA})
    return T


# --------------------------------------------------------------------------- cases for the many-column sweeps
# (tests/test_gpu_multi_sweeps.py; csrc/solve_kernels.hip, "several right-hand sides")
MULTI_FROM_SWEEP = ("tiny_n9", "tiny_n33", "wave9_n5", "wave39_n5", "wave_16_28_n5", "wave_1_38_n5", "mixed_few", "mixed_129",
                    "tall_mixed")
MULTI_FROM_SHAPES = ("panel_nc15", "panel_nc17", "panel_nc33", "panel_nc95", "panel_nc96", "schur_nb1", "schur_nb65", "bs_f129",
                     "trap_96_151", "chain_nc97")

# one-wave fronts around kWC = 16 (k_fwd_wave_m / k_bwd_wave_m keep a front's first 16 own unknowns in registers and re-read
# the others from the work vector): 15, 16, 17 and 33 columns, as roots and with rows below (f <= 64, f nc + nb^2 <= 1536)
WC_FRONTS = ((15, 29), (16, 28), (17, 24), (33, 10))


def bwd_multi_slices(nc, f, nwaves):
    """(nt, ns) of k_bwd_block_m for a front: nt = ceil(nc / 16) column tiles, ns = min(nwaves / nt, ceil(f / 32)) row
    slices, at least one (csrc/solve_kernels.hip: bwd_multi_slices); nwaves = 8 below 128 columns, 4 from there on."""
    nt = (nc + 15) // 16
    return nt, max(1, min(nwaves // nt, (f + 31) // 32))


# block-class fronts for that rule, f on both sides of 32 ns: name -> [(nc, nb), ...], one designed tree each, side by side
# (nt = 1 with all eight slices needs f > 224 and a stick of 600 rows above it: left out, ns = NW / nt binds at nt = 2)
SLICE_FRONTS = {
    "slice_nt1": [(16, 48), (16, 49), (16, 112), (16, 113)],       # ns = 2 | 3 and 4 | 5 by f (8 waves), 2 | 3 and 4 | 4 (4 waves)
    "slice_nt2": [(32, 32), (32, 33), (32, 96), (32, 97)],         # ns = 2 | 3 by f, 4 | 4 (8 waves); 2 | 2 (4 waves)
    "slice_nt3": [(48, 16), (48, 17)],                             # ns = 2 | 2 of 8 waves (two idle); 1 of 4 (one idle)
    "slice_nt5": [(80, 16), (80, 17)],                             # ns = 1: five tiles on 8 waves (three idle), on 4 in two rounds
    "slice_nt6": [(96, 32), (96, 33)],                             # ns = 1: six tiles
}


def multi_forests():
    """name -> (spec, level-0 fronts as sorted (nc, nb) pairs, classes): the new forests of the many-column tests."""
    T = {}
    T["wc_roots"] = (forest(*[designed(nc, 0) for nc, _ in WC_FRONTS]), sorted((nc, 0) for nc, _ in WC_FRONTS), "wave")
    T["wc_designed"] = (forest(*[designed(nc, nb) for nc, nb in WC_FRONTS]), sorted(WC_FRONTS), "wave")
    for name, fronts in SLICE_FRONTS.items():
        T[name] = (forest(*[designed(nc, nb) for nc, nb in fronts]), sorted(fronts), "block")
    return T


def multi_specs():
    """name -> spec of every front_shapes case of the many-column tests."""
    S, A = sweep_table(), all_cases()
    T = {n: S[n][0] for n in MULTI_FROM_SWEEP}
    T.update({n: A[n][0] for n in MULTI_FROM_SHAPES})
    T.update({n: v[0] for n, v in multi_forests().items()})
    return T


# --------------------------------------------------------------------------- cases for the builds of k_panel and k_schur
# (tests/test_gpu_factor_builds.py).  k_schur works on 64 x 64 tiles, one 32 x 32 quadrant per wave, in chunks of KC = 16
# columns and MFMA steps of 4; which BUILD of it (and of k_panel) a front meets is the schedule's decision:
#   plain      k_panel<BS, false, false>, k_schur<false, false>   outside the overlap mode
#   pipelined  k_schur<false, true>                               ... in launches of many deep tiles (HIPKKT_SCHUR_PIPE_*)
#   overlap    k_panel<BS, false, true>, k_schur<true, true>      the schedule's tail of >= 3 block-class launches
QUADRANT_NB = (31, 32, 33, 95, 96, 97)           # at nc = 40: a quadrant of the (last) tile row empty, full, one row over
CHUNK_NC = (15, 16, 17, 33, 48, 49)              # chunk edges ...
CHUNK_NB = (65, 129)                             # ... with off-diagonal tiles whose last tile row has ONE row (nr = 1, nq = 64)
SHALLOW_NC = (3, 4, 5)                           # a partial MFMA step, one step, one step and a partial one
# the shape-table cases that get a tall variant as well
BUILD_FROM_SHAPES = tuple(f"panel_nc{nc}" for nc in (15, 16, 17, 31, 32, 33, 95, 96)) + \
    tuple(f"schur_nb{nb}" for nb in (1, 63, 64, 65, 127, 128, 129, 192, 193)) + \
    tuple(f"bs_f{f}" for f in (128, 129, 192, 193)) + ("trap_96_151", "block_1_39", "block_16_29")


def build_table():
    """name -> (spec, level-0 tuple, class) of the new shapes, in the form of shape_table()."""
    T = {}
    for nb in QUADRANT_NB:
        T[f"quad_nb{nb}"] = _child(40, nb) + ("block",)
    for nc, nb in [(nc, nb) for nc in CHUNK_NC for nb in CHUNK_NB] + [(96, 129)]:
        T[f"chunk_{nc}_{nb}"] = _child(nc, nb) + ("block",)
    # f * nc + nb^2 = 42 * 3 + 1521 > 1536: block-class fronts of 3, 4 and 5 columns
    for nc in SHALLOW_NC:
        T[f"shallow_{nc}_39"] = _narrow(nc, 39) + ("block",)
    return T


# csrc/symbolic.hpp: panel_cap, panel_max_cols, panel_slice_below, panel_max_slices
_TRAP_CAP, _PANEL_COLS, _SLICE_BELOW, _PANEL_SLICES = 19200, 96, 64, 128


def chain_links(W, nb=0):
    """Widths of the links symbolic.cpp 7b cuts a supernode of W columns and nb rows into: the widest panel (<= 96 columns)
    whose trapezoid fits the cap -- or, where that one is narrower than 64 columns and a ROW-SLICED panel (its rows in up to
    128 slices) saves a link, the widest sliced one --, the remaining columns balanced over the remaining links.  (Fronts
    of a few hundred rows: the sweep kernels' own cap does not bind.)"""
    out = []
    while W > 0:
        f = W + nb
        wd = w1 = min(W, _PANEL_COLS)
        while wd > 1 and wd * (wd + 1) // 2 + -(-(f - wd) // _PANEL_SLICES) * wd > _TRAP_CAP:
            wd -= 1
        while w1 > 1 and _trap(w1, f - w1) > _TRAP_CAP:
            w1 -= 1
        if w1 >= _SLICE_BELOW or -(-W // w1) <= -(-W // wd):
            wd = w1
        if wd < W:
            parts = -(-W // wd)
            wd = -(-W // parts)
        out.append(wd)
        W -= wd
    return out


def _link_fronts(W, nb=0):
    out = []
    for w in chain_links(W, nb):
        out.append((W + nb, w))
        W -= w
    return out


TALL_NG = 200                                    # columns of a tall variant's root: three links of its own (67, 67, 66)


def tall(spec):
    """The tall variant of a designed() / beside_sibling() tree: the same fronts under a root G = (ng, 0) of at least
    TALL_NG columns, which 7b cuts into a chain of three links or more (as the roots of tests/extend_add_shapes.py:
    ng, _g_links) -- at least three block-class launches follow the designed front's own, the condition of the overlap
    mode (csrc/schedule.cpp: admit_overlap)."""
    *below, (g, nb, p) = spec
    assert nb == 0 and p == -1 and len(below) >= 2, "one tree with a stick"
    return below + [(max(g, TALL_NG), 0, -1)]


def tall_fronts(spec):
    """(f, nc) of every front ABOVE level 0 of tall(spec), lowest first, from the amalgamation arithmetic: the stick P --
    with the sibling S = (20, 1) absorbed, in a beside_sibling tree -- merges into the wide root or stays out of it, and
    what is wider than a panel is cut into links."""
    (rp, sp, _), (g, _, _) = spec[-2], tall(spec)[-1]
    sibling = spec[1][:2] == (20, 1)
    true_p = _trap(20, 1) + _trap(1, sp) if sibling else _trap(rp, sp)
    rp += 20 if sibling else 0
    tot = _trap(rp + g, 0)
    if (tot - true_p - _trap(g, 0)) / tot > _allowance(rp + g):
        return _link_fronts(rp, sp) + _link_fronts(g)
    return _link_fronts(rp + g)


def build_cases():
    """name -> (spec, tall spec, group) of every case of the factor-build tests: the new shapes and the shape-table
    cases of BUILD_FROM_SHAPES."""
    T, old = {}, shape_table()
    for n, v in build_table().items():
        T[n] = (v[0], tall(v[0]), "edges")
    for n in BUILD_FROM_SHAPES:
        T[n] = (old[n][0], tall(old[n][0]), "schur" if n.startswith("schur") else "panel")
    return T


# XCD tile order (csrc/engine_tables.cpp: HIPKKT_TILE_XCD deals the tiles of a launch's fronts, eight fronts at a time, to the
# residue classes of the workgroup index): ONE level with eleven fronts of 1, 1, 3, 3, 6 and 10 tiles -- a group of eight
# with unequal tile counts and a last group of three -- and two block-class roots without tiles between them
XCD_NB = (1, 193, 64, 129, 65, 128, 193, 1, 129, 65, 64)


def xcd_forest(tall_=False):
    trees = [designed(40, nb) for nb in XCD_NB]
    if tall_:
        trees = [tall(t) for t in trees]
    trees.insert(8, [(40, 0, -1)])
    trees.insert(3, [(40, 0, -1)])
    return forest(*trees)


def build_specs():
    """name -> spec of everything the factor-build tests run that is built from specs: every case of build_cases() as it
    is and as "<name>+tall", and the XCD forest both ways.  (The second XCD forest, parents with stored children, is
    tests/extend_add_shapes.py's: xcd_parents.)"""
    T = {}
    for n, (spec, tall_spec, _) in build_cases().items():
        T[n], T[n + "+tall"] = spec, tall_spec
    T["xcd_forest"], T["xcd_forest+tall"] = xcd_forest(), xcd_forest(True)
    return T


def product_fault(case):
    """K~ + E of a fault in the PRODUCT of the designed front (the first spec entry, a leaf of the tree): the term
    l_ik d_k l_jk of the front's last column k is left out of ONE entry of its update block, the last row and column.  From
    an exact LDL^T of the front (a leaf's factor depends on its own columns alone): a factorisation without that term is
    the exact one of K~ with the term added to entry (i, i)."""
    cols, rows = np.asarray(case.cols[0]), np.asarray(case.rows[0])
    A = full(case.Kt).tocsr()[np.concatenate([cols, rows])][:, cols].toarray()
    n = len(cols)
    L, d = A.copy(), np.zeros(n)
    for k in range(n):
        d[k] = L[k, k]
        L[k:, k] /= d[k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:n, k]) * d[k]
    term = L[-1, n - 1] * d[n - 1] * L[-1, n - 1]
    assert term != 0.0
    K = sp.lil_matrix(case.Kt)
    K[rows[-1], rows[-1]] = K[rows[-1], rows[-1]] + term
    return sp.csc_matrix(K)


def klass(f, nc):
    """Kernel class of a front of f rows and nc columns, as the schedule decides it (kernels.hpp: one-wave when
    f <= 64 and f * nc + nb^2 <= 1536; tiny fronts are one-wave fronts with a solve kernel of their own)."""
    nb = f - nc
    return "tiny" if f <= 8 else "wave" if _one_wave(nc, nb) else "block"


def all_cases():
    T = {}
    T.update(shape_table())
    T.update(chain_table())
    T.update(solve_bs_table())
    return T


def designed_front(case):
    """Columns and rows of the designed front: the first spec entry."""
    return case.cols[0], case.rows[0]


def perturbed(case, rel=1e-7):
    """K~ + E: one diagonal entry in the designed front's update region (its first row below; the front's last
    column for a root) changed by `rel` relative -- a stand-in for a dropped or misplaced extend-add term."""
    cols, rows = designed_front(case)
    k = rows[0] if rows else cols[-1]
    K = sp.csc_matrix(case.Kt, copy=True)
    K[k, k] = K[k, k] * (1.0 + rel)
    return K
