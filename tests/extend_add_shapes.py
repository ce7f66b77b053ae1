"""Trees whose STORED children sit on chosen rows of their parent's front, for the extend-add tests (tests/test_gpu_extend_add.py,
tests/test_extend_add_shapes_host.py).

The extend-add is how k_front_wave, k_panel and k_schur (csrc/factor_kernels.hip) bring the children's update blocks into a
parent front, through the work lists of csrc/schedule.cpp (build_factor_lists): panel items of at most 64 rows, 64 descriptors
per round, 16 in flight, cut into 16 wave slices (wcut); tile sub-items per (tile, tile column), 64 per round, 16 in flight,
four waves per tile (tcut); the dense child of a chain link; the row-slice mapping of a sliced panel; the two update buffers a
chain of panels shares (csrc/symbolic.cpp, step 10).  tests/front_shapes.py puts a child on the first rows of its parent's front
(rel = 0 .. nb - 1) and tests/pulled_leaf_shapes.py chooses rows for one-column leaves; the trees here are built with
pulled_leaf_shapes.tree (children of >= 2 columns on chosen positions, a poison sibling that keeps them apart from their
parent), with front_shapes' value rule, Case record, error measures and bounds.

A case carries what the CONSTRUCTION predicts, from the chosen positions alone (tests compare with the symbolic phase's dump):
    level1      the "[pieces]" figures of the parents' tree level with every child listed (HIPKKT_PULL_FACTOR_LEAVES=0):
                (panel pieces, panel entries, tile pieces, tile entries, (pieces of <= 4, 5 .. 16, 17 .. 64 entries))
    links       for chains: the widths of the links the designed supernode is cut into (read once from the host dump and
                written down here: symbolic.cpp 7b balances the columns over the panels the trapezoid cap allows)
    dense       dense children of the whole tree (one per chain link but the first; the root G above, where it is cut, too)
    shared      chains of three or more links (they share two update buffers)
    pulled      (leaves, terms) a handle pulls with HIPKKT_PULL_FACTOR_LEAVES=1
Positions are those of P's own front (its rp columns, then its sp rows); in the front of P' = P + poison sibling they move up by
the k poison columns.

What cannot exist (UNREACHABLE) and the one tiny parent that keeps children (REACHABLE_AFTER_ALL) are recorded below with the
arithmetic."""
import numpy as np
import scipy.sparse as sp

from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls

UNREACHABLE = {
    "a stored child under the second or the last link of a chain":
        "symbolic.cpp 7b hangs EVERY child of a supernode it cuts under the first link (nparent = first_new[parent]): the first "
        "link's front holds all later columns as rows, so the child's rows are all there.  The chain cases put children whose "
        "first row is a column of the second and of the last link; they are children of the first link, their pieces land in "
        "its update block alone (tile pieces only) and reach their columns through the dense children of the links above",
    "a parent with a dense child and listed items or pulled terms":
        "a child is dense when its rows are its parent's whole front.  Amalgamation always merges such a pair (no explicit "
        "zeros), so dense children come from the cut of 7b only, and a link above the first has the link below as its ONLY "
        "child (see the entry above).  The chain cases have the listed items, the pulled terms and the dense children in one "
        "chain, on neighbouring links",
    "a tiny parent (f <= 8) whose merged front has at most 32 columns":
        "relaxed amalgamation accepts any zero fraction up to 1.0 for a merged front of <= 8 columns, and 0.5 x 2 for the "
        "first-tried child up to 32 columns: the pair always merges.  See REACHABLE_AFTER_ALL for the one that stays",
}

REACHABLE_AFTER_ALL = {
    "a tiny parent with a child":
        "a tiny parent absorbs most children (UNREACHABLE); the exception: a root (8, 0) and a dense child (n, 1) merge into "
        "n + 8 columns with 7 n explicit zeros of (n + 8)(n + 9) / 2 entries.  From 33 columns on the first-tried child's allowance is 0.15 x 2 = 0.3, and n = 25 gives "
        "175 / 561 = 0.312, n = 26 gives 182 / 595 = 0.306 (n = 27: 189 / 630 = 0.300, merges; n <= 24: at most 32 columns, "
        "merges).  A second child is tried with 0.15 and stays out as well.  Case tiny_parent: k_front_tiny with three children",
}


# --------------------------------------------------------------------------- predictions from positions
def pieces(pnc, rel):
    """The pieces of ONE listed child whose rows are positions `rel` (ascending) of a parent front with pnc columns:
    (panel pieces, panel entries, tile pieces, tile entries, [pieces of <= 4, 5 .. 16, 17 .. 64 entries]).  A child column b
    whose row rel[b] is a panel column brings its entries a >= b in pieces of at most 64; one whose row is an update row brings
    them cut at the parent's 64-row tile boundaries."""
    n = len(rel)
    pp = pe = tp = te = 0
    cls = [0, 0, 0]
    for b in range(n):
        if rel[b] < pnc:
            pp += -(-(n - b) // 64)
            pe += n - b
        else:
            rows = [(r - pnc) >> 6 for r in rel[b:]]
            for ti in sorted(set(rows)):
                m = rows.count(ti)
                tp += 1
                te += m
                cls[0 if m <= 4 else 1 if m <= 16 else 2] += 1
    return pp, pe, tp, te, cls


def level_pieces(pnc, rels):
    tot = [0, 0, 0, 0, [0, 0, 0]]
    for rel in rels:
        p = pieces(pnc, rel)
        for i in range(4):
            tot[i] += p[i]
        tot[4] = [x + y for x, y in zip(tot[4], p[4])]
    return tot[0], tot[1], tot[2], tot[3], tuple(tot[4])


def scatter(n, first, f, must=(), avoid=()):
    """n positions of a front of f rows: `first`, every position of `must`, none of `avoid`, the others spread over (first, f)
    with gaps."""
    cand = [i for i in range(first + 1, f) if i not in avoid]
    must = sorted(set(must))
    assert all(first < m < f for m in must) and len(must) <= n - 1 <= len(cand)
    free = [i for i in cand if i not in must]
    ndrop = len(cand) - (n - 1)
    drop = {free[int(i)] for i in np.round(np.linspace(0, len(free) - 1, ndrop))} if ndrop else set()
    assert len(drop) == ndrop, "gaps collide: choose another size"
    pos = [first] + [i for i in cand if i not in drop]
    assert len(pos) == n and pos == sorted(set(pos))
    return pos


# --------------------------------------------------------------------------- the cases
P40_120 = dict(rp=32, sp_=120, ng=160, k=8)      # P' = (40, 120): block-class, two tile rows (tiles (0,0), (1,0), (1,1))
P40_60 = dict(rp=32, sp_=60, ng=100, k=8)        # P' = (40, 60): block-class, one tile (the root G = (100, 0) is two panels: overlap
                                                 # mode needs three block-class launches at the top of the tree)
P76_128 = dict(rp=64, sp_=128, ng=160, k=12)     # P' = (76, 128): f = 204, two full tile rows
P40_128 = dict(rp=32, sp_=128, ng=160, k=8)      # P' = (40, 128): cut into row slices under HIPKKT_PANEL_CAP=3000
W16_28 = dict(rp=8, sp_=28, ng=120, k=8)         # P' = (16, 28): a one-wave front (f nc + nb^2 = 704 + 784 <= 1536)

COUNTS = (15, 16, 17, 63, 64, 65, 129)           # 16 in flight; 64 descriptors per round (the first round comes from the
                                                 # caller); a third round

# links of the chain cases, as symbolic.cpp 7b cuts P' (and then the root G): read from the host dump, asserted by the host test
CHAINS = {
    #                shape                                   links of P'            links of G   first link(s) row-sliced
    "chain3_root": (dict(rp=192, sp_=0, ng=0, k=8), (67, 67, 66), (), 0),
    "chain3_stick": (dict(rp=192, sp_=40, ng=100, k=8), (67, 67, 66), (50, 50), 0),
    # 400 columns: a 96-column panel of 400 rows is over the trapezoid cap; unsliced panels would be 51 columns wide (eight
    # links), so 7b keeps wider ROW-SLICED first links -- the longest chains are five links, the first one or two sliced
    "chain5_root": (dict(rp=388, sp_=0, ng=0, k=12), (80, 64, 86, 85, 85), (), 1),
    "chain5_stick": (dict(rp=388, sp_=40, ng=160, k=12), (80, 80, 60, 90, 90), (80, 80), 2),
}


def _g_links(ng):
    """Links of a root G = (ng, 0) of the non-chain cases: one panel up to 96 columns, two equal ones up to 192."""
    return 0 if ng == 0 else -(-ng // 96)


def cases():
    """name -> dict(group, shape, cols, rows, children, leaves, level1, dense, links, shared, pulled, env, klass, fault)."""
    T = {}

    def add(name, group, shape, children=(), leaves=(), links=None, glinks=None, env=None, block=True, pulled=None, fault=None,
            sliced=0):
        cols, rows = pls.tree(leaves=list(leaves), others=list(children), **shape)
        k, pnc = shape["k"], (links[0] if links else shape["rp"] + shape["k"])
        rels = [[p + k for p in pos] for pos in leaves] + [[p + k for p in pos] for _, pos in children]
        nlinks = len(links) if links else 1
        gl = _g_links(shape["ng"]) if glinks is None else len(glinks)
        if pulled is None:
            # (a leaf is pulled under an unsliced block-class parent when its level's launch is a one-wave launch: every front
            #  of level 0 -- the children and the poison sibling -- must be one-wave)
            small0 = all(fs.klass(nc + len(pos), nc) != "block" for nc, pos in children)
            pl = list(leaves) if block and not sliced and not env and small0 else []
            pulled = (len(pl), sum(len(p) * (len(p) + 1) // 2 for p in pl))
        T[name] = dict(group=group, shape=shape, cols=cols, rows=rows, children=list(children), leaves=list(leaves),
                       level1=level_pieces(pnc, rels) if block else (0, 0, 0, 0, (0, 0, 0)), pnc=pnc,
                       dense=(nlinks - 1) + max(gl - 1, 0), links=links, glinks=glinks, shared=int(nlinks >= 3) + int(gl >= 3),
                       pulled=pulled, env=env or {}, block=block, fault=fault, sliced=sliced)

    # ---- piece lengths and starts: one two-column child of nbc rows under P' = (40, 120).  Its first row is panel column 5 of
    # P (13 of P'), its rows have gaps, straddle the panel / update boundary (30 .. 33 of P: the update rows start at 32) and U
    # rows 63 / 64 (U rows 62, 63 | 66: rows 64 and 65 are left out, so a column's rows in tile row 1 start at position 2 of
    # the tile, not at its first row).
    f = P40_120["rp"] + P40_120["sp_"]
    must = (30, 31, 32, 33, 32 + 62, 32 + 63, 32 + 66)
    for nbc in (63, 64, 65, 128, 129):
        pos = scatter(nbc, 5, f, must, avoid=(32 + 64, 32 + 65))
        # fault: the entry of the child's LAST row in its first column (row 65 of a 65-row child: the second piece's only entry)
        add(f"len_{nbc}", "lengths", P40_120, [(2, pos)], fault=("entry", pos[-1], pos[0]))
    # update rows in tile row 1 only: no sub-item in tiles (0, 0) and (1, 0), the diagonal tile (1, 1) hit at a non-zero row
    tail = [7] + scatter(29, 32 + 66, f, (32 + 119,))
    add("len_tail", "lengths", P40_120, [(2, tail)], fault=("entry", tail[-1], tail[1]))

    # ---- rounds and pieces in flight, panel: n two-column children of two rows on the same two panel columns (3 and 9 of P).
    # Column 3 and column 9 then hold n one-piece items each, and the 16 wave slices are cut between whole columns: two slices
    # of n items, the others empty
    for n in COUNTS:
        add(f"panel_n{n}", "panel_rounds", P40_60, [(2, [3, 9])] * n, fault=("drop", n - 1, 1, 0))

    # ---- rounds and pieces in flight, tiles: n two-column children on panel column 5, U rows 0 and 63 and all of tile row 1
    # (U rows 64 .. 127).  Per child: tile (0, 0) gets a piece of cnt 2 in qcol 0 and one of cnt 1 in qcol 63; the off-diagonal
    # tile (1, 0) a piece of cnt 64 in qcol 0 and in qcol 63; the diagonal tile (1, 1) pieces of cnt 64 - q in every qcol q.
    # Tiles (0, 0) and (1, 0) hold n sub-items in each of two columns: two of the four wave shares hold n, two none.
    # ("_b": without U row 63 -- cnt 1 in qcol 0.)
    rp = P76_128["rp"]
    rows_a = [5, rp + 0, rp + 63] + list(range(rp + 64, rp + 128))
    rows_b = [5, rp + 0] + list(range(rp + 64, rp + 128))
    for n in COUNTS:
        add(f"tile_n{n}", "tile_rounds", P76_128, [(2, rows_a)] * n, fault=("drop", n - 1, 3, 2))      # (U row 64, U row 63): tile (1, 0), qcol 63
    for n in (17, 65):
        add(f"tile_n{n}_b", "tile_rounds", P76_128, [(2, rows_b)] * n, fault=("drop", n - 1, 1, 1))    # (U row 0, U row 0): tile (0, 0), qcol 0, cnt 1

    # ---- many children, one entry: 33 children of 2, 3 and 5 columns on the same four rows -- two panel columns, U rows 1 and
    # 70 -- ten parent entries, in the panel and in tiles (0, 0), (1, 0) and (1, 1); the order of the additions is the lists'
    many = [((2, 3, 5)[i % 3], [2, 6, 32 + 1, 32 + 70]) for i in range(33)]
    add("many_33", "many", P40_120, many, fault=("drop", 32, 3, 2))

    # ---- chains of three and of five links, as a root (nb = 0) and under a stick (nb > 0).  A regular scattered child and a
    # one-column leaf whose first rows are columns of the SECOND link, and the same of the LAST link (UNREACHABLE: they are
    # children of the first link; every piece is a tile piece of its update block).  "_bare": no child at all.
    for name, (shape, links, glinks, sliced) in CHAINS.items():
        k, rpc, f = shape["k"], shape["rp"], shape["rp"] + shape["sp_"]
        s2, sl = links[0] - k, sum(links[:-1]) - k               # first columns of the second / last link, as positions of P
        A = (2, scatter(20, s2 + 7, f, (sl + 2, f - 1)))
        B = (2, scatter(12, sl + 5, f, (f - 1,)))
        leaves = [[s2 + 2, s2 + 31, sl + 3], [sl + 1, rpc - 1]]
        # fault: a term of the child under the last link is dropped (B's entry (row 2, row 1): in the last link's columns)
        add(name, "chains", shape, [A, B], leaves, links=links, glinks=glinks, sliced=sliced, fault=("drop", 3, 2, 1))
    shape, links, glinks, sliced = CHAINS["chain3_root"]
    add("chain3_bare", "chains", shape, links=links, glinks=glinks, fault=("stale",))
    shape, links, glinks, sliced = CHAINS["chain5_stick"]
    add("chain5_bare", "chains", shape, links=links, glinks=glinks, sliced=sliced, fault=("stale",))

    # ---- a row-sliced parent: HIPKKT_PANEL_CAP=3000 cuts P' = (40, 128) into three slices of 43, 43 and 42 update rows (820 +
    # 40 rows <= 3000: at most 54 rows a slice).  A piece of a panel column starts at that column's own row, so a FIRST piece
    # always starts in the top block; a piece below it needs a child of more than 64 rows.  Two-column children with a piece
    #   wholly in the top block (rows 3, 9, 20 of P);
    #   wholly inside slice 2 and outside slices 0 and 1 (the second piece of an 84-row child: U rows 90 .. 109);
    #   across the slice boundary 85 | 86 (the second piece of a 79-row child: U rows 80 .. 94), outside slice 0;
    #   across the top-block boundary (rows 28 .. 36 of P: the panel ends at 31; and the long children's first pieces, which
    #   run from the top block through slices 0 and 1).
    # The same cap cuts the root G = (160, 0) into three row-sliced links (54, 53, 53): a shared chain above P'.
    r = P40_128["rp"]
    sl_kids = [(2, [3, 9, 20]), (2, scatter(64, 4, r + 86) + list(range(r + 90, r + 110))),
               (2, scatter(64, 6, r + 80) + list(range(r + 80, r + 95))), (2, [7] + list(range(28, 37)))]
    add("sliced_kinds", "sliced", P40_128, sl_kids, env={"HIPKKT_PANEL_CAP": "3000"}, fault=("entry", r + 86, 6), glinks=(54, 53, 53),
        sliced=1)

    # ---- a one-wave parent (k_front_wave): children of 10 rows (one load round: 55 entries) and of 11 (the column loop) on
    # scattered rows, and 64 / 65 one-column children (the headers are read 64 children at a time)
    fw = W16_28["rp"] + W16_28["sp_"]
    for nbc in (10, 11):
        add(f"wave_nbc{nbc}", "wave", W16_28, [(2, scatter(nbc, 2, fw, (7, 8, fw - 1)))], block=False, fault=("drop", 0, nbc - 1, 0))
    for n in (64, 65):
        kids = [[i % 8, 8 + (5 * i) % 28] for i in range(n - 1)] + [[3, 8 + 27]]
        add(f"wave_kids{n}", "wave", W16_28, leaves=kids, block=False, fault=("drop", n - 1, 1, 1))
    return T


def tiny_parent():
    """(cols, rows) of REACHABLE_AFTER_ALL's tree: a root (8, 0) with the children (25, 1) on its column 0, (26, 1) on column 0
    and (25, 1) on column 5 -- k_front_tiny adds three update blocks, two of them into one entry."""
    cols, c = [], 0
    for n in (25, 26, 25, 8):
        cols.append(list(range(c, c + n)))
        c += n
    root = cols[-1]
    return cols, [[root[0]], [root[0]], [root[5]], []]


def names(group=None):
    T = cases()
    return [n for n, d in T.items() if group is None or d["group"] == group] + (["tiny_parent"] if group in (None, "wave") else [])


GROUPS = ("lengths", "panel_rounds", "tile_rounds", "many", "chains", "sliced", "wave")

_CASES = {}


def case(name, seed=1):
    """The fs.Case of a name (cached per (name, seed): a reference is computed once and left unchanged)."""
    if (name, seed) not in _CASES:
        if name == "tiny_parent":
            cols, rows = tiny_parent()
        elif name == "xcd_parents":
            cols, rows = xcd_parents()
        else:
            d = cases()[name]
            cols, rows = d["cols"], d["rows"]
        _CASES[(name, seed)] = pls.make_case(cols, rows, seed)
    return _CASES[(name, seed)]


# --------------------------------------------------------------------------- parents side by side (tests/test_gpu_factor_builds.py)
# Ten designed parents in ONE launch for the XCD tile order (csrc/engine_tables.cpp: HIPKKT_TILE_XCD permutes a launch's tiles together
# with their pass-through ranges, tile_cut and ptile_cut): nine whose stored children bring tile pieces -- update blocks of 120
# and of 128 rows, three tiles each, with very different lists -- and one of 60 rows, one tile, without any.  A group of eight
# fronts and a last group of two; the roots above are two links each, so the forest is tall enough for the overlap mode.
XCD_PARENTS = ("len_63", "len_64", "len_65", "len_128", "len_129", "len_tail", "tile_n15", "tile_n17_b", "many_33", "panel_n15")


def xcd_parents():
    """(cols, rows) of the trees of XCD_PARENTS side by side in one matrix, each tree's indices behind the one before."""
    T = cases()
    cols, rows, base = [], [], 0
    for n in XCD_PARENTS:
        cols += [[i + base for i in c] for c in T[n]["cols"]]
        rows += [[i + base for i in r] for r in T[n]["rows"]]
        base = cols[-1][-1] + 1
    return cols, rows


def second(name):
    """New values on the same pattern with the same pivot signs (seed 2): what hipkkt_ldl_update_values + refactor get."""
    if (name, "second") not in _CASES:
        c = case(name)
        _CASES[(name, "second")] = pls.make_case(c.cols, c.rows, 2, signs=c.dsigns)
    return _CASES[(name, "second")]


# --------------------------------------------------------------------------- fault stand-ins
def ldl(c):
    """Dense LDL^T of K~ without pivoting in fp64 (the matrices are strictly diagonally dominant): (L, d)."""
    A = fs.full(c.Kt).toarray()
    n = A.shape[0]
    L, d = np.eye(n), np.zeros(n)
    for k in range(n):
        d[k] = A[k, k]
        L[k + 1:, k] = A[k + 1:, k] / d[k]
        nz = np.nonzero(L[k + 1:, k])[0] + k + 1
        if nz.size:
            A[np.ix_(nz, nz)] -= np.outer(L[nz, k], L[nz, k]) * d[k]
    return L, d


def _with_entry(c, i, j, value=None, factor=None):
    K = sp.lil_matrix(c.Kt)
    i, j = min(i, j), max(i, j)
    K[i, j] = K[i, j] * factor if factor is not None else K[i, j] + value
    return sp.csc_matrix(K)


def faulted(name, c=None, rel=1e-7):
    """K~ + E of an extend-add fault at an entry that only the case's edge reaches (the case's `fault`), as
    front_shapes.perturbed does for a diagonal entry:
      ("entry", a, b)        the parent entry at P's positions (a, b) is wrong by `rel` relative;
      ("drop", child, a, b)  the term (a, b) of child number `child` (leaves first, then the regular children) is NOT added: a
                             factorisation that loses the term U_c(a, b) = -sum_k L(ra, k) d_k L(rb, k) (k: the child's columns)
                             is the exact one of K~ with U_c(a, b) taken off entry (ra, rb);
      ("stale",)             the third link of the chain reads the FIRST link's update block instead of the second's: the second
                             link's own update L_2 D_2 L_2^T is missing from the third link's front."""
    c = c or case(name)
    if name == "tiny_parent":
        kind = ("drop", 1, 0, 0)
        d = dict(cols=c.cols, rows=c.rows, shape=None)
    else:
        d = cases()[name]
        kind = d["fault"]
    if kind[0] == "entry":
        sh = d["shape"]
        pc, gc = d["cols"][-2], d["cols"][-1]
        front = pc + gc[:sh["sp_"]]
        return _with_entry(c, front[kind[1]], front[kind[2]], factor=1.0 + rel)
    L, dd = ldl(c)
    if kind[0] == "drop":
        _, ch, a, b = kind
        cs, rs = d["cols"][ch], d["rows"][ch]
        ra, rb = rs[a], rs[b]
        u = -float(np.sum(L[ra, cs] * dd[cs] * L[rb, cs]))
        assert u != 0.0
        return _with_entry(c, ra, rb, value=-u)
    # stale: columns of the second link, rows of the third link's front (its columns and everything behind them)
    links, k = d["links"], d["shape"]["k"]
    c0 = d["cols"][-2][0] - k if d["shape"]["sp_"] else d["cols"][-1][0] - k          # first column of P' (the poison columns)
    c2 = np.arange(c0 + links[0], c0 + links[0] + links[1])
    below = np.arange(c0 + links[0] + links[1], c.K.shape[0])
    E = (L[np.ix_(below, c2)] * dd[c2]) @ L[np.ix_(below, c2)].T
    E[np.abs(E) < 1e-300] = 0.0
    K = sp.lil_matrix(fs.full(c.Kt))
    K[np.ix_(below, below)] = K[np.ix_(below, below)].toarray() + E
    return sp.triu(sp.csc_matrix(K), format="csc")


# --------------------------------------------------------------------------- the "[pieces]" lines (HIPKKT_DUMP_LEVELS; a handle under HIPKKT_VERBOSE=2)
import re

_PIECES = re.compile(r"\[pieces\] parent level\s+(\d+): tile pieces (\d+) \((\d+) entries; <=4: (\d+), 5-16: (\d+), 17-64: (\d+)\), panel pieces (\d+) "
                     r"\((\d+) entries\) \| pulled leaves took out (\d+) tile and (\d+) panel pieces: (\d+) terms")
_PULLED = re.compile(r"\[pieces\] pulled leaves (\d+), terms (\d+) in")


def parse_pieces(err):
    """-> ({level: dict(listed=(panel pieces, panel entries, tile pieces, tile entries, (<=4, 5-16, 17-64)), out=(tile pieces,
    panel pieces, terms) of the pulled leaves)}, (pulled leaves, terms)) of the LAST block of [pieces] lines in `err`."""
    blocks, cur = [], {}
    for line in err.splitlines():
        m = _PIECES.search(line)
        if m:
            v = list(map(int, m.groups()))
            cur[v[0]] = dict(listed=(v[6], v[7], v[1], v[2], (v[3], v[4], v[5])), out=(v[8], v[9], v[10]))
        m = _PULLED.search(line)
        if m:
            blocks.append((cur, (int(m[1]), int(m[2]))))
            cur = {}
    assert blocks, err[-2000:]
    return blocks[-1]
