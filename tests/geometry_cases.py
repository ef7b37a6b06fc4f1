"""The table of the geometry tests (tests/test_geometry_cases.py, tests/test_gpu_geometry.py):
operators of a few thousand rows whose element grid is wider than 512 rows per block.

elem_geometry (two-pass-lanczos_amd/csrc/tpl_layout.cpp) gives every operator of up to 195,584
rows E = 512 rows per row block: chunk_of_block (tpl_kcommon.h) then has one chunk per block, the
canonical pair order "thread t owns the pairs i0 = b E + 2 t + 512 q" never reaches q = 1, and no
row block is empty. The headline sizes run at E = 2048 and E = 5120, the latter with row blocks
that start past n. tpl_op_set_schedule(op, 0, max_g2) caps the number of row blocks, so a
3,000-row operator runs at E = 1024, 1536, 2560 or 3072 — with more chunks than fit the blocks
evenly, and with empty trailing blocks. The oracle takes G2 and E from the schedule, and its bits
depend on them (tests/test_geometry_cases.py checks that), so a bitwise comparison at these
geometries sees a chunk skipped or done twice, a partial summed in another q order, and a kernel
that mishandles a block whose first row lies past n.

Nothing here touches a GPU. The matrices are kept out of state_cases.MATRICES on purpose: the
call-order tests multiply over that tuple.

The KKT block. The issue of this table named kkt_hubs(30, leaves=1366, d=True) (n = 3002) and
asked for it to run fused at default settings, adjusting `leaves` if it does not. It does not,
and no number of leaves helps: a leaf's arc row and node row reference each other, so both are
open, and the fused pass two takes at most 256 rows in its hub set — 2 leaves + the hubs they
hang on <= 256, which with 30 hubs ends at leaves = 113 and n = 496, one row block. The rows
that cost nothing are the hub-to-hub arcs (closed: their columns are the row itself and two long
rows). Their number is bounded too: the default long-row cache holds 2 n / n_long steps and a
solve runs fused only when it holds all of them, so K_BIG = 24 steps need n_long <= 250 hubs.
kkt_hubs(224, leaves=45, d=True, span=12) has the same 3002 rows and therefore the same
geometries: 224 long rows (26 cached steps), 90 open rows, |H| = 135.
"""
import numpy as np

import state_cases as sc

KNOBS = dict(w=3, hub_every=97, hub_half=60, hub_step=7, seed=5)
KKT_HUBS, KKT_LEAVES, KKT_SPAN = 224, 45, 12

MATRICES = ("band3001", "band2301", "kkt3002", "band9473")


def matrix(name):
    if name == "kkt3002":
        from fused_cases import kkt_hubs
        a = kkt_hubs(KKT_HUBS, leaves=KKT_LEAVES, d=True, span=KKT_SPAN)
        assert a.shape == (3002, 3002)
        return a
    from conftest import banded_hub
    return banded_hub(n={"band3001": 3001, "band2301": 2301, "band9473": 9473}[name], **KNOBS)


class Case:
    """One geometry: the matrix, the cap handed to set_schedule (None: no setter, the default
    geometry), and what elem_geometry must make of it: G2 row blocks of E rows, `empty` of them
    starting at or past n. n_short and n_long pin the row split the chunk count follows from."""

    def __init__(self, mat, max_g2, G2, E, empty, n_short, n_long):
        self.mat, self.max_g2, self.G2, self.E, self.empty = mat, max_g2, G2, E, empty
        self.n_short, self.n_long = n_short, n_long
        self.id = "%s-%s" % (mat, "default" if max_g2 is None else "g%d" % max_g2)

    @property
    def cpe(self):
        """Chunks per row block (chunk_of_block)."""
        return self.E // 512

    @property
    def n_chunks(self):
        return -(-self.n_short // 512)


_ROWS = {"band3001": (2970, 31), "band2301": (2277, 24), "kkt3002": (2778, 224),
         "band9473": (9375, 98)}
_TABLE = (
    #  matrix    max_g2  G2    E  empty
    ("band3001", None,    6,  512, 0),
    ("band3001", 5,       5, 1024, 2),   # blocks 3 and 4 start at rows 3072 and 4096
    ("band3001", 3,       3, 1024, 0),
    ("band3001", 2,       2, 1536, 0),
    ("band3001", 1,       1, 3072, 0),
    ("band2301", None,    5,  512, 0),
    ("band2301", 3,       3, 1024, 0),   # 5 chunks in blocks of 2: the last block holds one
    ("band2301", 2,       2, 1536, 0),
    ("band2301", 1,       1, 2560, 0),
    ("kkt3002",  None,    6,  512, 0),
    ("kkt3002",  5,       5, 1024, 2),
    ("kkt3002",  3,       3, 1024, 0),
    ("kkt3002",  2,       2, 1536, 0),
    ("kkt3002",  1,       1, 3072, 0),
    ("band9473", 10,     10, 1024, 0),   # rb_first: two row blocks on XCDs 1 and 5
    ("band9473", 9,       9, 1536, 2),   # blocks 7 and 8 start at rows 10752 and 12288
)
CASES = tuple(Case(*row, *_ROWS[row[0]]) for row in _TABLE)
CASE_IDS = tuple(c.id for c in CASES)


_MATRIX, _RHS, _INPUTS = {}, {}, {}


def cached_matrix(name):
    if name not in _MATRIX:
        _MATRIX[name] = matrix(name)
    return _MATRIX[name]


def host_schedule(case):
    """The case's schedule from the layout rule restated in conftest.py (no GPU)."""
    from conftest import canon_schedule
    return canon_schedule(cached_matrix(case.mat), max_g2=case.max_g2 or 1024, reorder=True)


def empty_blocks(schedule, n):
    return sum(1 for b in range(int(schedule["G2"])) if b * int(schedule["E"]) >= n)


def inputs(case, schedule=None):
    """state_cases.Inputs of the case's matrix — the seven right-hand sides of the call-order
    tests, made once per matrix — with the host decompositions in `schedule`'s reduction order
    (a live operator's, or by default the restated rule's). Memoised per case: the GPU tests
    assert the live schedule equals the restated one before they rely on it."""
    if case.id not in _INPUTS:
        a = cached_matrix(case.mat)
        if case.mat not in _RHS:
            _RHS[case.mat] = sc.Inputs.right_hand_sides(a)
        _INPUTS[case.id] = sc.Inputs(case.id, a=a, schedule=schedule or host_schedule(case),
                                     B=_RHS[case.mat])
    return _INPUTS[case.id]


same_schedule = sc.same_schedule
