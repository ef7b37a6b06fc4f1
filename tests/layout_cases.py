"""Deterministic matrices that pin which instance of the SpMV-shaped kernels runs, and the
edges of the layout they read (tests/test_layout_cases.py on the CPU, tests/
test_gpu_variants.py on the GPU). Plain numpy / scipy: no GPU, no files, fixed seeds.

The kernels k_spmv<F>, k_p1_spmv<F> (and _wide / _gp) and k_p2_spmv<F> are compiled once per
variant flag F (two-pass-lanczos_amd/csrc/tpl_device.h kVar*):

    F = uniform chunk width 1..4 (0: generic) | 8 int8 values | 16 uint16 chunk columns
        | 32 uint16 bin columns | 64 chunk column window in LDS

and tpl_layout.cpp build_layout decides every bit from the matrix and the schedule setters.
A case is (name, matrix, setters, expected F); `case(name)` builds it. Three tables:

  VARIANTS  one case per compiled instance (56), named "F%03d"
  EDGES     layout edges (chunk widths, empty rows, piece lengths, bin counts), each in an
            int8 / uint16 format ("...-i8") and an fp64 / int32 one ("...-f64")
  WIDE      more than 256 norm partials (k_p1_spmv_wide), named "wide-F%03d"

How the building blocks steer build_layout (all of it restated by `plan`, which the CPU test
checks against the runtime's own host plan wherever no setter is involved):
  * short rows are a banded block on their own index space, W entries per interior row, so
    every chunk has width W; the band's first and last row are narrower, which leaves room
    for one LINK entry between them without widening a chunk. The link sets the column
    span of two chunks: 2,637 (wider than the LDS window, uint16 still fits) or 65,999
    (uint16 no longer fits).
  * long rows are two fully connected cliques of hub rows (48 rows: pieces of at most
    kBigPiece entries; 72 rows: longer ones) that reference no short row. Clustered hubs
    keep the bins' spans small; hubs at both ends of >= 65,536 columns, in the caller's
    order and one slice, do not.
  * the locality order (default) moves the hubs behind the short rows; a layout held in a
    permuted order never gets the window. Hubs that already are the last rows leave the
    order the identity.
"""
import functools

import numpy as np
import scipy.sparse as sp

CHUNK = 512          # kChunkRows
TPB = 256            # kTPB
BIG_PIECE = 64       # kBigPiece
BIN_MIN = 2048       # kBinMin
BIN_MAX = 7936       # kBinMax
BIN_SEGS = 255       # kBinSegs
WIN_MAX = 2048       # kWinMax
V8, SC16, BC16, WIN = 8, 16, 32, 64

NS_SMALL = 1324      # short rows: 3 chunks, the last one 300 rows
NS_MID = 2638        # 6 chunks, the last one 78 rows; a linked block of this size spans 2,637
NS_FAR = 69934       # 137 chunks, the last one 302 rows
LINK_MID = 2638      # rows of the linked block (span 2,637 > kWinMax)
LINK_FAR = 66000     # span 65,999 >= 65,535
HUBS_A, HUBS_B = 48, 72


class Case:
    def __init__(self, name, a, setters, F):
        self.name, self.a, self.setters, self.F = name, a, list(setters), F

    def apply_setters(self, op):
        for method, kwargs in self.setters:
            getattr(op, method)(**kwargs)


# ------------------------------------------------------------------ building blocks
def _values(rng, count, ints):
    if ints:
        return (rng.integers(1, 4, count) * rng.choice([-1, 1], count)).astype(np.float64)
    return rng.standard_normal(count)


def band_upper(lo, hi, W, link=False, split=None, gap=False):
    """Upper triangle (diagonal included) of a band on the short positions [lo, hi) with W
    entries per interior row: W odd = the diagonal and (W - 1) / 2 neighbours to either side,
    W even = W / 2 neighbours to either side and no diagonal, W = 1 = disjoint pairs
    (p, p + 1), with gap the last pair but one left out (two empty rows: the only padding a
    chunk of width 1 can hold). split: rows from this position on carry one more neighbour pair (W + 2).
    link: one more entry between the first and the last row (W = 1: the first and the last
    pair are re-paired across the block)."""
    m = hi - lo
    p = np.arange(lo, hi)
    if W == 1:
        assert m % 2 == 0 and m >= 8
        r, c = p[0::2].copy(), p[1::2].copy()
        if gap:
            r, c = np.delete(r, -2), np.delete(c, -2)
        if link:
            r = np.concatenate([[lo, lo + 1], r[1:-1]])
            c = np.concatenate([[hi - 2, hi - 1], c[1:-1]])
        return r, c
    rows, cols = [], []
    if W % 2:
        rows.append(p)
        cols.append(p)
    for d in range(1, W // 2 + 1):
        rows.append(p[:-d])
        cols.append(p[d:])
    if split is not None:
        d = W // 2 + 1
        q = p[:-d]
        q = q[q >= split]
        rows.append(q)
        cols.append(q + d)
    if link:
        rows.append(np.array([lo]))
        cols.append(np.array([hi - 1]))
    return np.concatenate(rows), np.concatenate(cols)


def symmetric(n, r, c, v):
    """CSR of the symmetric matrix with the upper entries (r, c, v), r <= c, stored zeros
    kept."""
    off = r != c
    rr = np.concatenate([r, c[off]])
    cc = np.concatenate([c, r[off]])
    vv = np.concatenate([v, v[off]])
    order = np.lexsort((cc, rr))
    rr, cc, vv = rr[order], cc[order], vv[order]
    assert not np.any((rr[1:] == rr[:-1]) & (cc[1:] == cc[:-1])), "duplicate entry"
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rr + 1, 1)
    return sp.csr_matrix((vv, cc.astype(np.int32), np.cumsum(indptr)), shape=(n, n))


def clique_upper(rows):
    rows = np.asarray(rows)
    i, j = np.triu_indices(len(rows))
    return rows[i], rows[j]


def hub_positions(ns, place):
    """Global rows of the two hub cliques among n = ns + 120 rows."""
    H = HUBS_A + HUBS_B
    n = ns + H
    if place == "end":
        h = np.arange(ns, n)
    elif place == "mid":   # the small clique straddles n / 2, a bound of 2 and of 4 column
        lo = n // 2 - HUBS_A // 2   # slices: its rows are cut in two, the others stay whole
        h = np.arange(lo, lo + H)
    elif place == "ends":
        first, last = np.arange(H // 2), np.arange(n - H // 2, n)
        a = np.concatenate([first[:HUBS_A // 2], last[:HUBS_A // 2]])
        b = np.concatenate([first[HUBS_A // 2:], last[HUBS_A // 2:]])
        return n, a, b
    else:
        raise ValueError(place)
    return n, h[:HUBS_A], h[HUBS_A:]


def variant_matrix(seed, ns, W, ints, place=None, link_rows=0):
    """ns short rows (band width W, or W = "mixed": 3 entries per row in the first half, 5 in
    the second) plus, with `place`, the 120 hub rows. link_rows > 0: the first link_rows short
    rows are a band block of their own whose first and last row are linked."""
    rng = np.random.default_rng(seed)
    # empty rows sort first in the locality order: only where the caller's order is kept
    gap = place == "ends"
    if W == "mixed":
        r, c = band_upper(0, ns, 3, split=ns // 2)
    elif link_rows == ns:
        r, c = band_upper(0, ns, W, link=True)
    elif link_rows:
        r0, c0 = band_upper(0, link_rows, W, link=True)
        r1, c1 = band_upper(link_rows, ns, W, gap=gap)
        r, c = np.concatenate([r0, r1]), np.concatenate([c0, c1])
    else:
        r, c = band_upper(0, ns, W, gap=gap)
    n = ns
    if place:
        n, ha, hb = hub_positions(ns, place)
        short = np.setdiff1d(np.arange(n), np.concatenate([ha, hb]))
        r, c = short[r], short[c]
        for h in (ha, hb):
            hr, hc = clique_upper(np.sort(h))
            r, c = np.concatenate([r, hr]), np.concatenate([c, hc])
    return symmetric(n, r, c, _values(rng, len(r), ints))


# ------------------------------------------------------------------ the variant table
# every format of every width, and the window where a uniform width 1..4 has uint16 chunk
# columns (tests/test_layout_cases.py holds the kernels' predicate and compares)
ALL_VARIANTS = sorted(
    [w | v | s | b for w in range(5) for v in (0, V8) for s in (0, SC16) for b in (0, BC16)] +
    [w | v | SC16 | b | WIN for w in range(1, 5) for v in (0, V8) for b in (0, BC16)])
# instance -> the build_layout rule that forbids it (none: all 56 are reachable)
UNREACHABLE = {}

REORDER_OFF = ("set_reorder", {"mode": 0})


def _slices(s):
    return ("set_slices", {"slices": s})


def variant_spec(F):
    """(variant_matrix arguments, setters) that make build_layout choose F."""
    w, v8, sc, bc, win = F & 7, bool(F & V8), bool(F & SC16), bool(F & BC16), bool(F & WIN)
    W = w if w else (5 if sc else "mixed")
    uniform = W != "mixed"
    kw = dict(seed=1000 + F, ns=NS_SMALL, W=W, ints=v8, place=None, link_rows=0)
    setters = []
    if bc:                       # clustered hubs: every bin spans fewer than 65,535 columns
        if win:                  # hubs last: the locality order is the identity
            kw.update(place="end")
        elif sc and w:           # hubs in the middle: the order moves them, no window
            kw.update(place="mid")
        elif sc:                 # width 0 has no window: caller's order, rows cut in 4 slices
            kw.update(place="mid")
            setters = [REORDER_OFF, _slices(4)]
        elif uniform:            # a chunk spanning 65,999 columns; rows cut in 2 slices (auto)
            kw.update(place="mid", ns=NS_FAR, link_rows=LINK_FAR)
            setters = [REORDER_OFF]
        else:                    # mixed widths never get uint16 chunk columns
            kw.update(place="mid")
    elif not v8 and sc and not win:   # no long rows at all: no bins, no uint16 bin columns
        if w:
            kw.update(ns=NS_MID, link_rows=LINK_MID)
    else:                        # hubs at both ends of > 65,535 columns, one slice, as given
        kw.update(place="ends", ns=NS_FAR)
        setters = [REORDER_OFF, _slices(1)]
        if uniform and not sc:
            kw.update(link_rows=LINK_FAR)
        elif uniform and w and not win:
            kw.update(link_rows=LINK_MID)
    return kw, setters


VARIANTS = {"F%03d" % F: F for F in ALL_VARIANTS if F not in UNREACHABLE}


# ------------------------------------------------------------------ k_p1_spmv_wide
NS_WIDE = 131500     # + 120 hubs: 258 row blocks of 512 (> 256 norm partials)
WIDE = {"wide-F%03d" % F: F
        for F in [w | V8 | SC16 | BC16 | win for w in (1, 2, 4) for win in (0, WIN)] +
                 [0 | SC16 | BC16] + [w | SC16 | BC16 | win for w in (1, 3) for win in (0, WIN)]}


def wide_spec(F):
    w, win = F & 7, bool(F & WIN)
    return dict(seed=2000 + F, ns=NS_WIDE, W=w if w else 5, ints=bool(F & V8), place="end",
                link_rows=0 if (win or not w) else LINK_MID), []


# ------------------------------------------------------------------ the edge table
def star_matrix(seed, lengths, ints, n=None, columns=None, order="long-first"):
    """One long row per entry of `lengths`, each referencing that many pool rows of its own;
    a pool row holds its diagonal and the one link (2 entries). Long rows come first
    (rows 0 .. len(lengths) - 1) or last. columns: per long row, the explicit pool rows it
    references (global indices) instead of the next free ones."""
    rng = np.random.default_rng(seed)
    nl = len(lengths)
    total = int(np.sum(lengths))
    if columns is None:
        n = n or nl + total
        base = nl if order == "long-first" else 0
        ends = np.cumsum(lengths)
        columns = [np.arange(base + e - l, base + e) for l, e in zip(lengths, ends)]
    lrows = np.arange(nl) if order == "long-first" else np.arange(n - nl, n)
    r = np.concatenate([np.full(len(c), lr) for lr, c in zip(lrows, columns)])
    c = np.concatenate(columns)
    assert len(np.unique(c)) == len(c) and not np.intersect1d(c, lrows).size
    pool = np.setdiff1d(np.arange(n), lrows)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    v = _values(rng, len(r), ints)
    d = (rng.integers(1, 100, len(pool)).astype(np.float64) if ints
         else rng.uniform(1.0, 2.0, len(pool)))
    return symmetric(n, np.concatenate([lo, pool]), np.concatenate([hi, pool]),
                     np.concatenate([v, d]))


def chunk_blocks_matrix(seed, widths, last_rows, ints, empty_every=0):
    """Short rows only: chunk c is a band block of its own with widths[c] entries per row
    (0: an all-empty chunk); the last chunk holds last_rows rows. empty_every > 0: every
    such row (and its column) is removed from the band, which leaves it empty."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    n = CHUNK * (len(widths) - 1) + last_rows
    for ci, W in enumerate(widths):
        lo, hi = CHUNK * ci, min(n, CHUNK * (ci + 1))
        if W == 0:
            continue
        r, c = band_upper(lo, hi - (hi - lo) % 2 if W == 1 else hi, W)
        rows.append(r)
        cols.append(c)
    r, c = np.concatenate(rows), np.concatenate(cols)
    if empty_every:
        keep = (r % empty_every != 3) & (c % empty_every != 3)
        r, c = r[keep], c[keep]
    return symmetric(n, r, c, _values(rng, len(r), ints))


def hubs_and_short(seed, n_short, ints):
    """n_short tridiagonal short rows followed by one clique of 48 hub rows."""
    rng = np.random.default_rng(seed)
    r, c = band_upper(0, n_short, 3) if n_short > 1 else (np.array([0]), np.array([0]))
    hr, hc = clique_upper(np.arange(n_short, n_short + HUBS_A))
    r, c = np.concatenate([r, hr]), np.concatenate([c, hc])
    return symmetric(n_short + HUBS_A, r, c, _values(rng, len(r), ints))


PIECE_LENGTHS = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 143]
_MAIN = [6, 7, 8, 9, 62, 63, 64, 65, 126, 127, 128, 129, 142, 143]


def piece_matrix(seed, ints):
    """Long row i (rows 0..13) holds _MAIN[i] entries in column slice 1 + (i % 3) of four and
    one entry in slice 0: whole rows (S = 1) of _MAIN[i] + 1 entries, and under S = 4 pieces
    of 1 and of _MAIN[i] entries. A piece of one entry needs S > 1: a row of one entry is
    never long (the threshold is at least 1)."""
    n = 4096
    nxt = {s: n * s // 4 + (len(_MAIN) if s == 0 else 0) for s in range(4)}
    cols = []
    for i, m in enumerate(_MAIN):
        s = 1 + i % 3
        cols.append(np.concatenate([[nxt[0]], np.arange(nxt[s], nxt[s] + m)]))
        nxt[0] += 1
        nxt[s] += m
    return star_matrix(seed, [m + 1 for m in _MAIN], ints, n=n, columns=cols)


# bins by first fit under bin_cap 2,048: 3, 4 and 5 big pieces; 2 big + 7, 8 and 9 small
BIN_COUNT_LENGTHS = ([600] * 3 + [500] * 4 + [400] * 5 + [800, 800] + [60] * 7 + [800, 800] +
                     [50] * 8 + [800, 800] + [40] * 9 + [800])
BIN_COUNT_EXPECT = [(3, 3), (4, 4), (5, 5), (9, 2), (10, 2), (11, 2), (1, 1)]  # (pieces, big)


def slice_rows_matrix(seed, ints):
    """n = 4096 under S = 8 (512 columns per slice): long rows 0..3 of 40 entries lying in
    slice 3 only, in slices 2 and 5, in all eight, and in slices 1..7 (slice 0 empty)."""
    n = 4096
    at = {s: 512 * s + (8 if s == 0 else 0) for s in range(8)}

    def take(s, m):
        c = np.arange(at[s], at[s] + m)
        at[s] += m
        return c
    cols = [take(3, 40), np.concatenate([take(2, 20), take(5, 20)]),
            np.concatenate([take(s, 5) for s in range(8)]),
            np.concatenate([take(s, 6 if s < 6 else 5) for s in range(1, 8)])]
    return star_matrix(seed, [40, 40, 40, 40], ints, n=n, columns=cols)


def _edge_builders():
    T = ("set_schedule", {"short_row_max": 2})
    e = {}
    for W in (5, 8, 9, 16, 17, 32):
        e["width%d" % W] = (lambda ints, W=W: variant_matrix(300 + W, NS_SMALL, W, ints), [])
    e["widths-1-2-3-4-7"] = (
        lambda ints: chunk_blocks_matrix(311, [7, 1, 7, 2, 7, 3, 7, 4, 7], 300, ints), [])
    e["empty-chunk"] = (lambda ints: chunk_blocks_matrix(312, [3, 0, 3], 300, ints), [])
    e["empty-rows"] = (
        lambda ints: chunk_blocks_matrix(313, [3, 3, 3], 300, ints, empty_every=7), [])
    for ns in (1, 511, 512, 513):
        e["nshort%d" % ns] = (lambda ints, ns=ns: hubs_and_short(320 + ns, ns, ints), [])
    e["pieces-S1"] = (lambda ints: piece_matrix(330, ints), [REORDER_OFF, T, _slices(1)])
    e["pieces-S4"] = (lambda ints: piece_matrix(330, ints), [REORDER_OFF, T, _slices(4)])
    e["bin-counts"] = (lambda ints: star_matrix(331, BIN_COUNT_LENGTHS, ints),
                       [REORDER_OFF, T, _slices(1)])
    e["bins-by-count"] = (
        lambda ints: star_matrix(332, [3 + i % 3 for i in range(764)], ints),
        [REORDER_OFF, T, _slices(1)])
    e["wide-bins"] = (lambda ints: star_matrix(333, [2049, 6000], ints),
                      [REORDER_OFF, T, _slices(1)])
    e["forced-slices"] = (lambda ints: star_matrix(334, [7937], ints, order="long-last"), [])
    e["slices-1-2-8"] = (lambda ints: slice_rows_matrix(335, ints),
                         [REORDER_OFF, T, _slices(8)])
    return e


_EDGE = _edge_builders()
FP64_INT32 = ("set_value_format", {"compress": False})
# Expected F of every edge in its two formats. "-i8": small-integer values and whatever
# uint16 formats and window the spans allow; "-f64": normal-distributed values and
# set_value_format(False), which leaves the width bits alone. A uniform width above 4 and
# per-chunk widths both run the generic instance (width bits 0), the former with uint16
# chunk columns. tests/test_layout_cases.py checks the column against `plan`.
_EDGE_F = {
    "width5": (24, 0), "width8": (24, 0), "width9": (24, 0), "width16": (24, 0),
    "width17": (24, 0), "width32": (24, 0), "widths-1-2-3-4-7": (8, 0), "empty-chunk": (8, 0),
    "empty-rows": (91, 3), "nshort1": (121, 1), "nshort511": (123, 3), "nshort512": (123, 3),
    "nshort513": (40, 0), "pieces-S1": (40, 0), "pieces-S4": (40, 0), "bin-counts": (58, 2),
    "bins-by-count": (58, 2), "wide-bins": (58, 2), "forced-slices": (58, 2),
    "slices-1-2-8": (58, 2),
}
EDGES = {"%s-%s" % (b, f): _EDGE_F[b][i] for b in _EDGE for i, f in enumerate(("i8", "f64"))}
# n = 600, nnz = 0: two all-empty chunks on the generic instance; with nothing stored every
# value (the padding's 0.0) is a small integer, so the int8 format is chosen
EMPTY_MATRIX = "all-empty"
EMPTY_MATRIX_F = 8


@functools.lru_cache(maxsize=4)
def case(name):
    """The case of that name from VARIANTS, WIDE, EDGES or EMPTY_MATRIX."""
    if name in VARIANTS or name in WIDE:
        F = VARIANTS[name] if name in VARIANTS else WIDE[name]
        kw, setters = variant_spec(F) if name in VARIANTS else wide_spec(F)
        return Case(name, variant_matrix(**kw), setters, F)
    if name == EMPTY_MATRIX:
        return Case(name, sp.csr_matrix((600, 600), dtype=np.float64), [], EMPTY_MATRIX_F)
    base, fmt = name.rsplit("-", 1)
    build, setters = _EDGE[base]
    a = build(fmt == "i8")
    return Case(name, a, setters + ([FP64_INT32] if fmt == "f64" else []), EDGES[name])


# six variant cases through k_spmv with special values in x: widths 0, 1, 3 and 4, the
# window (81, 124), int8 (56, 124, 11, 9), bins under S = 4 (56)
SPECIAL = ["F056", "F081", "F051", "F124", "F011", "F009"]
STORED_ZERO = "F051"   # its copy with an explicitly stored 0.0 at (0, 1) and (1, 0)


def with_stored_zero(a):
    a = a.copy()
    for i, j in ((0, 1), (1, 0)):
        q = a.indptr[i] + int(np.searchsorted(a.indices[a.indptr[i]:a.indptr[i + 1]], j))
        assert a.indices[q] == j
        a.data[q] = 0.0
    return a


def padded_rows_off_column(p, col):
    """Internal short rows of plan p that are narrower than their chunk, whose padding
    entries gather internal column `col`, and that hold no stored entry in that column.
    Off the window path every chunk's padding gathers internal column 0 (xsrc[0]); in a
    window instance it reads the window's first element, i.e. the chunk's column base
    (tpl_kcommon.h short_chunk_w: lds[0] = xsrc[s_cbase[chunk]]), so only the chunks whose
    base is `col` count."""
    a = p["a"]
    lens = np.diff(a.indptr)
    out = []
    for c, w in enumerate(p["widths"]):
        if p["window"] and p["chunk_base"][c] != col:
            continue
        rows = p["short"][c * CHUNK:(c + 1) * CHUNK]
        for r in rows[lens[rows] < w]:
            if col not in a.indices[a.indptr[r]:a.indptr[r + 1]]:
                out.append(r)
    return np.array(out, dtype=np.int64)


def poisoned_column(p, perm=None):
    """The caller's column whose value the padding of some live row gathers without that
    row referencing it: internal column 0, or — window instances — the base of the first
    chunk that holds such a padded row (F124: chunk 0, base 0, row 0 has no diagonal; F081:
    the last chunk, whose two empty rows are the only padding a width of 1 allows)."""
    cols = sorted(set(p["chunk_base"])) if p["window"] else [0]
    for col in cols:
        if padded_rows_off_column(p, col).size:
            return int(col) if perm is None else int(perm[col])
    raise ValueError("no padded row that does not reference the column its padding gathers")


def special_columns(a, p, perm=None):
    """(p0, three columns): p0 = poisoned_column; the three others, each referenced by some
    row, take -0.0 and the subnormals."""
    p0 = poisoned_column(p, perm)
    cols = [int(j) for j in np.unique(a.indices) if j != p0][1:7:2]
    return p0, cols


SPECIAL_X0 = [np.nan, np.inf, -np.inf]
SPECIAL_SMALL = [-0.0, 5e-324, 1e-310]


def special_x(a, p, perm, x0, seed=77):
    """A random x with x0 at the poisoned column and SPECIAL_SMALL at special_columns."""
    x = np.random.default_rng(seed).standard_normal(a.shape[0])
    p0, cols = special_columns(a, p, perm)
    x[cols] = SPECIAL_SMALL
    x[p0] = x0
    return x, p0


# ------------------------------------------------------------------ build_layout restated
def short_row_threshold(lens, requested=-1):
    if requested > 0:
        return requested
    if lens.size == 0:
        return 32
    m = int(np.sort(np.minimum(lens, 33))[(lens.size + 1) // 2 - 1])
    return max(4, min(32, 2 * m))


def setter_values(setters):
    s = {"reorder": 2, "short_row_max": -1, "slices": 0, "compress": True, "max_g2": 1024}
    for method, kw in setters:
        if method == "set_reorder":
            s["reorder"] = kw["mode"]
        elif method == "set_schedule":
            if kw.get("short_row_max", 0):
                s["short_row_max"] = kw["short_row_max"]
            if kw.get("max_g2", 0) > 0:
                s["max_g2"] = kw["max_g2"]
        elif method == "set_slices":
            s["slices"] = kw["slices"]
        elif method == "set_value_format":
            s["compress"] = bool(kw["compress"])
        else:
            raise ValueError(method)
    return s


def small_int(v):
    return bool(np.all((v >= -128) & (v <= 127) & (v == np.trunc(v)) &
                       ~((v == 0) & np.signbit(v))))


def plan(a, setters=(), perm=None):
    """tpl_layout.cpp build_layout restated for a single-GPU operator: the short / long split,
    chunk widths, slices, (row, slice) pieces, first-fit bins, and the format bits, hence F.
    perm: the locality order the operator holds (None: the caller's order).

    What ties this restatement to the runtime: F for every case (the host plan where a case
    has no setter, the live operator's kernel_variant() in tests/test_gpu_variants.py for
    all of them), and for the cases without setters the short rows, the order and the slice
    count against the host plan. The bins (pieces per bin, big and small counts, bin_cap)
    are NOT reported by any introspection call: those claims rest on this restatement of
    the first fit alone. Bin membership never enters a sum (a piece's sum depends on its
    entries and its length only), so the piece LENGTHS the edge table claims follow from
    the matrix, the threshold and the slice count; the per-bin COUNTS (3/4/5 big, 7/8/9
    small, 255/255/254) would have to be re-derived if the packing rule (bin_cap, kBinSegs,
    the default bin_balance, which only moves whole bins) changed."""
    sv = setter_values(setters)
    a = sp.csr_matrix(a)
    if perm is not None:
        a = a[perm][:, perm].tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    lens = np.diff(rp)
    T = short_row_threshold(lens, sv["short_row_max"])
    short = np.nonzero(lens <= T)[0]
    long_ = np.nonzero(lens > T)[0]
    ns = short.size
    nchunks = -(-ns // CHUNK)
    widths = [int(lens[short[c * CHUNK:(c + 1) * CHUNK]].max()) for c in range(nchunks)]
    uniform = nchunks > 0 and len(set(widths)) == 1 and widths[0] > 0
    s_width = widths[0] if uniform else 0
    # column span of every chunk
    spans, chunk_base = [], []
    for c in range(nchunks):
        rows = short[c * CHUNK:(c + 1) * CHUNK]
        cols = np.concatenate([ci[rp[r]:rp[r + 1]] for r in rows]) if lens[rows].sum() else None
        spans.append(0 if cols is None else int(cols.max() - cols.min()))
        chunk_base.append(0 if cols is None else int(cols.min()))
    # slices and pieces
    S = sv["slices"]
    if S <= 0:
        S = 1
        while S < 8 and n * 8.0 / S > 0.5 * 1024 * 1024:
            S *= 2

    def cut(S):
        bounds = np.array([n * s // S for s in range(1, S)], dtype=np.int64)
        return [np.bincount(np.searchsorted(bounds, ci[rp[r]:rp[r + 1]], side="right"),
                            minlength=S) for r in long_]
    pieces = cut(S)
    while sv["slices"] <= 0 and S < 8 and max((int(p.max()) for p in pieces), default=0) > BIN_MAX:
        S *= 2
        pieces = cut(S)
    widest = max((int(p.max()) for p in pieces), default=0)
    assert widest <= BIN_MAX
    bin_cap = max(BIN_MIN, -(-widest // TPB) * TPB)
    bin_cap = -(-bin_cap // BIN_MIN) * BIN_MIN
    bins = []        # per slice: list of bins, each a list of (long-row rank, piece length)
    for s in range(S):
        out = []
        fill = 0
        for k, p in enumerate(pieces):
            cnt = int(p[s])
            if cnt == 0 and not (s == 0 and p.sum() == 0):
                continue
            if not out or fill + cnt > bin_cap or len(out[-1]) == BIN_SEGS:
                out.append([])
                fill = 0
            out[-1].append((k, cnt))
            fill += cnt
        bins.append(out)
    M = max((len(b) for b in bins), default=0) if long_.size else 0
    bin_spans = []
    for s in range(S):
        lo_b, hi_b = n * s // S, n * (s + 1) // S
        for b in bins[s]:
            cols = []
            for k, cnt in b:
                r = long_[k]
                cc = ci[rp[r]:rp[r + 1]]
                cols.append(cc[(cc >= lo_b) & (cc < hi_b)])
            cols = np.concatenate(cols)
            bin_spans.append(int(cols.max() - cols.min()) if cols.size else 0)
    val_i8 = sv["compress"] and small_int(a.data)
    s_col16 = sv["compress"] and uniform and max(spans) < 0xFFFF
    b_col16 = sv["compress"] and S * M > 0 and max(bin_spans, default=0) < 0xFFFF
    window = (perm is None and s_col16 and 1 <= s_width <= 4 and
              0 < max(spans) + 1 <= WIN_MAX)
    cw = s_width if 1 <= s_width <= 4 else 0
    F = cw | (V8 if val_i8 else 0) | (SC16 if s_col16 else 0) | (BC16 if b_col16 else 0) | \
        (WIN if window else 0)
    return {"F": F, "T": T, "short": short, "long": long_, "n_short": ns, "chunks": nchunks,
            "widths": widths, "slices": S, "pieces": pieces, "bins": bins, "M": M,
            "bin_cap": bin_cap, "a": a, "window": bool(window), "chunk_base": chunk_base}
