"""speck_multiply_masked_* (speck_amd/csrc/masked.hip) with inputs placed on every positional switch of its kernels: the
four group widths and their two product walks, the batches of A in the workgroup classes, the LDS table at its sizes and
with adversarial clusters, the span cut, the second trip of every class kernel over its list, FULL_PATTERN at size, the
forks over the four stream groups, the column checks by position.

The call cannot report which kernel served a row (info.rows_class sums the four widths and the two LDS launches).  What
makes these tests meaningful is tests/test_masked_edges_host.py: it builds the same inputs with the generators of this
file and proves, without a GPU and against the real rules (masked_rules.hpp, compiled for the host), that every planned
row lands in the cell it is meant for.

Reference: every value of A and B is a nonzero integer in [-8, 8], so every product and every partial sum is exact in
double in any order, for both value types.  The expectation is the oracle's exact product filtered by the mask (Expect of
test_gpu_masked.py, over order-preserving compacted column ids: the oracle and scipy work on arrays of cols(B) words);
offsets, column ids AND values are compared byte for byte -- there is no tolerance.  A lost or doubled product changes an
integer sum by at least 1 (no product is zero); a product added to the wrong entry changes two of them.

Not covered: the branch of the classifying pass for a tile with 2^32 products or more (unreachable in seconds)."""
import functools

import numpy as np
import pytest

import speck_amd as sa
from oracle import pyoracle as po
import test_gpu_add as t_add
import test_gpu_hostile_tiles as t_tiles
from test_gpu_masked import Expect, as_dtype, to_dev, scan_case, _update

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
MODES = [False, True]
ERR_INVALID, ERR_UNSORTED = 1, 8
LISTS = ["g8", "g16", "g32", "g64", "lds_s", "lds_l", "global"]
IDLE = -1
# rows one trip of a list's grid serves: the grid caps of masked_run times the rows of a workgroup
GRID_ROWS = {"g8": 2048 * 32, "g16": 2048 * 16, "g32": 2048 * 8, "g64": 2048 * 4, "lds_s": 2048, "lds_l": 512, "global": 512}
THREADS = {"lds_s": 256, "lds_l": 1024, "global": 1024}     # = entries of A per batch
# the option settings a case runs under
RUNS = {"default": (sa.MASK_GROUP_MAX, sa.MASK_LDS_MAX), "g0": (0, sa.MASK_LDS_MAX), "g0l0": (0, 0)}
VALUES = np.array([v for v in range(-8, 9) if v], dtype=np.float64)


@pytest.fixture
def cfg():
    c = sa.spECKConfig.initialize(0)
    yield c
    c.cleanup()


# ---------------------------------------------------------------------------------------------------- building blocks
def csr_of(rows_cols, cols, rng):
    """the rows given as ascending arrays of columns; values: nonzero integers in [-8, 8]"""
    ro = np.zeros(len(rows_cols) + 1, dtype=np.uint32)
    ro[1:] = np.cumsum([len(c) for c in rows_cols])
    ci = np.concatenate(list(rows_cols) + [np.zeros(0, np.int64)]).astype(np.uint32)
    return po.HostCSR(len(rows_cols), cols, ro, ci, rng.choice(VALUES, size=len(ci)))


def csr_of_lens(lens, first, step, cols, rng):
    """row r: lens[r] columns first[r], first[r] + step[r], ...; no Python loop over the rows"""
    lens = np.asarray(lens, dtype=np.int64)
    ro = np.zeros(len(lens) + 1, dtype=np.int64)
    ro[1:] = np.cumsum(lens)
    row = np.repeat(np.arange(len(lens)), lens)
    ci = np.asarray(first)[row] + (np.arange(int(ro[-1])) - ro[row]) * np.asarray(step)[row]
    assert ci.max(initial=0) < cols
    return po.HostCSR(len(lens), cols, ro.astype(np.uint32), ci.astype(np.uint32), rng.choice(VALUES, size=len(ci)))


def intended_lists(n, width):
    """the list a row with work of n mask entries is meant for under each option setting (width: its group width)"""
    by_n = "lds_s" if n <= 1024 else "lds_l" if n <= 4096 else "global"
    return {"default": f"g{width}" if n <= 256 else by_n, "g0": by_n, "g0l0": "global"}


class Case:
    """one input: A, B, M, the option settings it runs under, the list every row is meant for under each (an index into
    LISTS, IDLE for a row without work), and per planned row what else the host test has to prove"""

    def __init__(self, name, A, B, M, runs, lists, plans=()):
        self.name, self.A, self.B, self.M, self.runs, self.lists, self.plans = name, A, B, M, tuple(runs), lists, list(plans)
        self._expect = None

    def expect(self):
        if self._expect is None:
            self._expect = exact_expect(self.A, self.B, self.M)
        return self._expect


def exact_expect(A, B, M):
    """Expect (test_gpu_masked.py) of the inputs with the columns in use renumbered in order: the same structure, the
    same sums, without arrays of cols(B) words (2^27 columns in the span cases)"""
    used = np.unique(np.concatenate([B.col_ids[:B.nnz], M.col_ids[:M.nnz]]))
    cols = max(len(used), 1)
    Bc = po.HostCSR(B.rows, cols, B.row_offsets, np.searchsorted(used, B.col_ids[:B.nnz]), B.data)
    Mc = po.HostCSR(M.rows, cols, M.row_offsets, np.searchsorted(used, M.col_ids[:M.nnz]), M.data)
    X = Expect(A, Bc, Mc)
    X.cols = B.cols
    X.ci, X.full_ci = used[X.ci].astype(np.uint32), used[X.full_ci].astype(np.uint32)
    return X


def draw(rng, u, lens):
    """sel[i, j]: row i holds column j of a universe of u columns -- lens[i] of them, at random"""
    lens = np.asarray(lens, dtype=np.int64)
    order = rng.random((len(lens), u)).argsort(axis=1)
    sel = np.zeros((len(lens), u), dtype=bool)
    sel[np.arange(len(lens))[:, None], order] = np.arange(u)[None, :] < lens[:, None]
    return sel


def force(sel, i, j, present, keep=()):
    """row i holds (does not hold) column j afterwards; its length and what it holds of `keep` stay"""
    if sel[i, j] == present:
        return
    swap = [x for x in np.flatnonzero(sel[i] == present) if x != j and x not in keep]
    sel[i, swap[len(swap) // 2]] = not present
    sel[i, j] = present


class Builder:
    """a case whose rows of A have rows of B of their own: the k-th entry of a row of A points at a row of B of exactly
    the length the plan gives it"""

    def __init__(self, name, cols, seed):
        self.name, self.cols, self.rng = name, cols, np.random.default_rng(seed)
        self.m, self.a, self.b, self.plans, self.lists = [], [], [], [], {run: [] for run in RUNS}

    def row(self, mask, b_rows, width=8, **plan):
        """a row with work: its mask row, and one private row of B per entry of A"""
        k0 = len(self.b)
        self.b.extend(b_rows)
        self.m.append(np.asarray(mask))
        self.a.append(np.arange(k0, k0 + len(b_rows)))
        for run, name in intended_lists(len(mask), width).items():
            self.lists[run].append(LISTS.index(name))
        plan.update(row=len(self.m) - 1, width=width)
        self.plans.append(plan)

    def idle_row(self, mask=()):
        self.m.append(np.asarray(mask, dtype=np.int64))
        self.a.append(np.zeros(0, np.int64))
        for run in RUNS:
            self.lists[run].append(IDLE)

    def planned(self, n, lens, batch, width=8, universe=None, mpos=None, span=False, **plan):
        """a row of n mask entries whose entries of A meet rows of B of the lengths `lens`, drawn from a universe of
        columns of which the mask row is a part (in its middle: products fall on either side of the span too).
        batch: entries of A per batch in the kernel the row is meant for.  Forced where the lengths allow it:
          * a hit and a miss in the row;
          * with three mask entries and two batches or more (late=True in the plan): the first mask column is hit in the
            last batch only, the last mask column in the first batch and in the last one;
          * span: products on cmin - 1 / cmin (first entry of A) and on cmax / cmax + 1 (last one)."""
        rng, lens = self.rng, np.asarray(lens, dtype=np.int64)
        if universe is None:
            u = int(max(2 * n + 40, lens.max(initial=0) + 8))
            universe = np.sort(rng.choice(self.cols, size=u, replace=False))
            mpos = np.sort(rng.choice(np.arange(u // 5, u - u // 5), size=n, replace=False))
        u = len(universe)
        sel = draw(rng, u, lens)
        in_mask = np.zeros(u, dtype=bool)
        in_mask[mpos] = True
        inside = np.flatnonzero(~in_mask & (np.arange(u) > mpos[0]) & (np.arange(u) < mpos[-1]))
        miss = int(inside[len(inside) // 2]) if len(inside) else int(np.flatnonzero(~in_mask)[0])
        j_late, j_multi = int(mpos[0]), int(mpos[-1])
        some = np.flatnonzero(lens > 0)
        nbatch = (len(lens) + batch - 1) // batch
        last = np.arange((nbatch - 1) * batch, len(lens))
        last_some = last[lens[last] > 0]
        late = False
        if nbatch >= 2 and n >= 3 and len(some) and some[0] < batch and not span:
            big = int(last[np.argmax(lens[last])])
            spots = [big] * 3 if lens[big] >= 3 else [int(x) for x in last_some[:3]]
            if len(spots) == 3:
                late = True
                specials = (j_late, j_multi, miss)
                for i in range((nbatch - 1) * batch):
                    force(sel, i, j_late, False, keep=specials)
                for i, j in zip(spots, specials):
                    force(sel, i, j, True, keep=specials)
                for i in last:
                    if i not in spots:
                        force(sel, int(i), j_late, False, keep=specials)
                force(sel, int(some[0]), j_multi, True, keep=specials)
        if span:
            assert lens[0] >= 2 and lens[-1] >= 2 and len(lens) >= 2 and j_late > 0 and j_multi < u - 1
            for i, js in ((0, (j_late - 1, j_late)), (len(lens) - 1, (j_multi, j_multi + 1))):
                for j in js:
                    force(sel, i, j, True, keep=(j_late - 1, j_late, j_multi, j_multi + 1))
        elif not late and len(some):
            force(sel, int(some[0]), j_multi, True)
            if some[-1] != some[0] or lens[some[0]] >= 2:
                force(sel, int(some[-1]), miss, True, keep=(j_multi,))
        assert (sel.sum(axis=1) == lens).all()
        self.row(universe[mpos], [universe[s] for s in sel], width=width, late=late, span=span, batch=batch, **plan)

    def case(self, runs):
        rng = self.rng
        M, A, B = csr_of(self.m, self.cols, rng), csr_of(self.a, max(len(self.b), 1), rng), csr_of(self.b, self.cols, rng)
        lists = {run: np.array(self.lists[run], dtype=np.int64) for run in runs}
        return Case(self.name, A, B, M, runs, lists, self.plans)


def batch_lens(nb, total, pattern, zeros, start):
    """nb lengths summing to `total`: the pattern from `start` on, `zeros` empty, what is missing on one entry"""
    lens = np.array([pattern[(start + i) % len(pattern)] for i in range(nb)], dtype=np.int64)
    free = [i for i in range(nb) if i not in zeros] or [nb // 2]
    lens[[z for z in zeros if z < nb and z not in free]] = 0
    s = 0
    for i in range(nb):
        if s + lens[i] > total:
            lens[i] = 0
        s += lens[i]
    lens[free[len(free) // 2]] += total - s
    return lens


# ---------------------------------------------------------------------------------------------------- a: widths and walks
WIDTHS = (8, 16, 32, 64)
OPS_RANGE = {8: (0, 287), 16: (288, 543), 32: (544, 1055), 64: (1056, None)}     # products that ask for the width
LEN_TOP = {8: 32, 16: 64, 32: 128, 64: 256}                                       # mask entries the width holds
MASK_LENS = {8: (1, 2, 31, 32), 16: (1, 2, 33, 63, 64), 32: (1, 2, 65, 127, 128), 64: (1, 2, 129, 255, 256)}
VARIANTS = ("team", "team_more", "flat", "flat_tails", "team_flat", "flat_team")
TEAM_LENS = (0, 1, 7, 8, 9, 31, 32, 33)      # the eight-lane step and the four-fold unroll of the team walk
FLAT_LENS = (0, 1, 2, 3, 5, 0, 4, 1)


def a_lens(L):
    return (1, L - 1, L, L + 1, 2 * L, 2 * L + 1) + ((4 * L + 3,) if L == 64 else ())


def batch_plan(L, len_a, variant, k):
    """[(entries, team walk?, products)] per batch; None where the variant needs a second batch and there is none"""
    nbs = [L] * (len_a // L) + ([len_a % L] if len_a % L else [])
    if variant in ("team_flat", "flat_team") and len(nbs) < 2:
        return None
    out = []
    for b, nb in enumerate(nbs):
        team = {"team": True, "team_more": True, "flat": False, "flat_tails": False, "team_flat": b % 2 == 0,
                "flat_team": b % 2 == 1}[variant]
        if team:
            total = 16 * nb + ((1, 17, 5)[(b + k) % 3] if variant == "team_more" else 0)      # "team": 16 nb exactly
        elif variant == "flat_tails":                                                       # the unroll of walk_products<L>
            tails = [t for t in (1, 4 * L - 1, 4 * L, 4 * L + 1) if t <= 16 * nb - 1]
            total = tails[(b + k) % len(tails)]
        else:
            total = 16 * nb - 1
        out.append([nb, team, total])
    return out


def fit_products(L, n, plan):
    """the batch totals moved into the products the width rule leaves the row: None where it leaves none"""
    lo, hi = (0 if n > LEN_TOP[L] // 2 else OPS_RANGE[L][0]), OPS_RANGE[L][1]     # (by length alone: any number up to hi)
    ops = sum(t for _, _, t in plan)
    if hi is not None and ops > hi:                   # give back what "team_more" added
        for p in plan:
            if p[1] and ops > hi:
                back = min(p[2] - 16 * p[0], ops - hi)
                p[2] -= back
                ops -= back
    if ops < lo:                                      # a team batch may hold any number of products
        team = [p for p in plan if p[1]]
        if team:
            team[0][2] += lo - ops
            ops = lo
    return plan if ops >= lo and (hi is None or ops <= hi) else None


@functools.lru_cache(maxsize=None)
def case_widths():
    """-> (Case, [(L, n, len_a, variant)] the cells the width rule makes unreachable)"""
    bld, unreachable, k = Builder("widths", 1 << 16, 101), [], 0
    for L in WIDTHS:
        for n in MASK_LENS[L]:
            for len_a in a_lens(L):
                for variant in VARIANTS:
                    plan = batch_plan(L, len_a, variant, k)
                    if plan is None:
                        continue
                    plan = fit_products(L, n, plan)
                    if plan is None:
                        unreachable.append((L, n, len_a, variant))
                        continue
                    k += 1
                    lens = []
                    for b, (nb, team, total) in enumerate(plan):
                        if team:
                            lens.append(batch_lens(nb, total, TEAM_LENS, (), k + b))
                        else:       # first, last and several middle entries of A on empty rows of B
                            lens.append(batch_lens(nb, total, FLAT_LENS, (0, nb - 1, nb // 2, nb // 3, nb // 2 + 1), k + b))
                    bld.planned(n, np.concatenate(lens), L, width=L, variant=variant,
                                walks=tuple(team for _, team, _ in plan), totals=tuple(t for _, _, t in plan))
                    if k % 9 == 0:
                        bld.idle_row(mask=[3, 9])
    return bld.case(("default",)), unreachable


# ---------------------------------------------------------------------------------------------------- b: width by products
SATURATING = (300, 4096)      # entries of A, entries of each row of B they meet: 1.2 M products a row


@functools.lru_cache(maxsize=None)
def case_products():
    bld = Builder("products", 1 << 16, 202)
    for n in (1, 4):
        for ops in (287, 288, 543, 544, 1055, 1056):
            lens = np.full(12, ops // 12)
            lens[-1] += ops - lens.sum()
            width = next(L for L in WIDTHS if OPS_RANGE[L][1] is None or ops <= OPS_RANGE[L][1])
            bld.planned(n, lens, width, width=width, ops=ops)
    case = bld.case(("default", "g0"))
    # two rows beyond the saturation of the per-row count: 300 / 301 entries of A on shared rows of B of 4096 entries
    rng = bld.rng
    na, nb = SATURATING
    big_b = [(k % 16) + 16 * np.arange(nb) for k in range(na + 1)]
    B2 = csr_of(big_b, 1 << 16, rng)
    masks = [np.array([5]), np.array([5, 1000, 1001, 40000])]
    k0 = case.B.rows
    A, B, M = case.A, case.B, case.M
    a_rows = [np.arange(k0, k0 + na), np.arange(k0 + 1, k0 + na + 1)]
    A2 = csr_of(a_rows, k0 + na + 1, rng)
    A = po.HostCSR(A.rows + 2, k0 + na + 1, np.concatenate([A.row_offsets, A.row_offsets[-1] + A2.row_offsets[1:]]),
                   np.concatenate([A.col_ids, A2.col_ids]), np.concatenate([A.data, A2.data]))
    B = po.HostCSR(k0 + na + 1, B.cols, np.concatenate([B.row_offsets, B.row_offsets[-1] + B2.row_offsets[1:]]),
                   np.concatenate([B.col_ids, B2.col_ids]), np.concatenate([B.data, B2.data]))
    M2 = csr_of(masks, 1 << 16, rng)
    M = po.HostCSR(M.rows + 2, M.cols, np.concatenate([M.row_offsets, M.row_offsets[-1] + M2.row_offsets[1:]]),
                   np.concatenate([M.col_ids, M2.col_ids]), np.concatenate([M.data, M2.data]))
    lists = {run: np.concatenate([case.lists[run], [LISTS.index(intended_lists(len(m), 64)[run]) for m in masks]])
             for run in case.runs}
    plans = case.plans + [dict(row=M.rows - 2 + i, width=64, saturated=True) for i in range(2)]
    return Case("products", A, B, M, case.runs, lists, plans)


# ---------------------------------------------------------------------------------------------------- c: batches of A
def wg_lens(rng, len_a, T):
    """rows of B of 0 - 3 entries, empty at both ends of every batch of T; a last batch of one entry gets three"""
    lens = rng.integers(0, 4, size=len_a)
    edges = [p for b in range(0, len_a, T) for p in (b, min(b + T, len_a) - 1)]
    lens[edges] = 0
    if len_a % T == 1:
        lens[-1] = 3
    return lens


@functools.lru_cache(maxsize=None)
def case_batches():
    """small-LDS rows (mask rows of 300) around batches of 256, large-LDS rows (1030) around batches of 1024 -- the global
    class runs the same rows with both limits 0.  The batches with 4 T - 1 and 4 T products hold rows of B of 4 entries:
    T rows of at most 3 cannot reach them."""
    bld = Builder("batches", 1 << 14, 303)
    rng = bld.rng
    for T, n in ((256, 300), (1024, 1030)):
        for len_a in (T - 1, T, T + 1, 2 * T + 1):
            bld.planned(n, wg_lens(rng, len_a, T), T, kind="edge")
        first = wg_lens(rng, T, T)
        one = np.zeros(T, dtype=np.int64)
        one[T // 2] = 1
        almost = np.full(T, 4)
        almost[T // 3] = 3
        bld.planned(n, np.concatenate([first, np.full(T, 4), one]), T, kind="remainders")           # .., 4 T, 1
        bld.planned(n, np.concatenate([first, almost, np.zeros(T, dtype=np.int64)]), T, kind="remainders")   # .., 4 T - 1, 0
    return bld.case(("default", "g0l0"))


# ---------------------------------------------------------------------------------------------------- d: the table
def py_slot(c, bits):
    """table_slot in Python integers"""
    return ((int(c) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)


def slots_of(cols, bits):
    """... for every column id below cols, in 64-bit integers"""
    return ((np.arange(cols, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def homed(home, lo, hi, count, rng):
    """`count` columns whose home slot lies in [lo, hi]"""
    found = np.flatnonzero((home >= lo) & (home <= hi))
    assert len(found) >= count, (lo, hi, len(found), count)     # (more columns: use 2^21)
    return rng.choice(found, size=count, replace=False)


def adversarial(bld, home, bits, n_tail, n_head, n_absent, kind, tail_slots=8, one_home=None, entries=24, width=8):
    """a mask row of n_tail columns homed in the last `tail_slots` slots (or all in `one_home`) and n_head homed in slots
    0 - 3; rows of B over these and over n_absent columns with the same homes that the mask row does not hold, all of them
    inside its span (the span cut would drop them otherwise)"""
    rng, slots = bld.rng, 1 << bits
    lo, hi = (one_home, one_home) if one_home is not None else (slots - tail_slots, slots - 1)
    half = n_absent // 2 if n_head else n_absent
    tail = homed(home, lo, hi, n_tail + half, rng)
    head = homed(home, 0, 3, n_head + n_absent - half, rng) if n_head else np.zeros(0, np.int64)
    universe = np.sort(np.concatenate([tail, head]))
    u = len(universe)
    is_tail = np.isin(universe, tail)
    inner = np.arange(1, u - 1)          # (the smallest and the largest column stay in the mask row)
    absent = rng.choice(inner[is_tail[1:-1]], size=half, replace=False)
    if n_head:
        absent = np.concatenate([absent, rng.choice(inner[~is_tail[1:-1]], size=n_absent - half, replace=False)])
    mpos = np.setdiff1d(np.arange(u), absent)
    n = len(mpos)
    lens = rng.integers(min(24, u // 2), min(40, u) + 1, size=entries)
    bld.planned(n, lens, 256 if n <= 1024 else 1024, width=width, universe=universe, mpos=mpos, kind=kind, bits=bits,
                absent=universe[absent])


@functools.lru_cache(maxsize=None)
def case_table(cols=1 << 20):
    bld = Builder("table", cols, 404)
    rng = bld.rng
    for n in (1, 2, 7, 8, 9, 257, 512, 513, 1024, 1025, 2048, 2049, 4096):
        T = 256 if n <= 1024 else 1024
        lens = rng.integers(2, 12, size=20) if n <= 32 else rng.integers(8, 40, size=20)     # (n <= 32: few products, G8)
        bld.planned(n, lens, T, kind="size", width=8)
    h4, h10, h11, h12 = (slots_of(cols, b) for b in (4, 10, 11, 12))
    adversarial(bld, h11, 11, 600, 20, 200, "wrap")             # 2048 slots, small launch
    adversarial(bld, h10, 10, 300, 0, 100, "one_home", one_home=517)
    adversarial(bld, h12, 12, 1080, 20, 200, "wrap")            # 4096 slots, large launch
    adversarial(bld, h4, 4, 6, 2, 8, "wrap", tail_slots=4, entries=10)   # 16 slots: the LDS class with mask_group_max = 0
    return bld.case(("default", "g0"))


# ---------------------------------------------------------------------------------------------------- e: the span cut
def distinct(rng, lo, hi, count):
    """`count` distinct integers of [lo, hi), without an array of hi words"""
    found = np.unique(rng.integers(lo, hi, size=2 * count + 16))
    assert len(found) >= count
    return rng.permutation(found)[:count]


@functools.lru_cache(maxsize=None)
def case_span(cols=1 << 27):
    """every row: products on cmin - 1, cmin, cmax and cmax + 1 (where there is such a column); mask rows of one entry hit
    and missed by one on either side; mask rows from column 0 to column cols - 1"""
    bld = Builder("span", cols, 505)
    rng = bld.rng
    for n in (2, 5, 40, 300, 1100):
        T = {2: 8, 5: 8, 40: 16}.get(n, 256 if n <= 1024 else 1024)
        w = 16 if n == 40 else 8
        # n + 12 columns: two outside the span on either side (the inner ones at cmin - 1 and cmax + 1), eight misses inside
        universe = np.sort(distinct(rng, 1000, cols - 1000, n + 12))
        universe[1], universe[-2] = universe[2] - 1, universe[-3] + 1
        assert (np.diff(universe) > 0).all()
        mpos = np.setdiff1d(np.arange(2, n + 10), rng.choice(np.arange(3, n + 9), size=8, replace=False))
        assert len(mpos) == n and mpos[0] == 2 and mpos[-1] == n + 9
        bld.planned(n, rng.integers(2, 8, size=6), T, width=w, universe=universe, mpos=mpos, span=True)
        # ... and from column 0 to column cols - 1: nothing lies outside, 1 and cols - 2 are misses inside
        universe = np.sort(np.concatenate([[0, 1, cols - 2, cols - 1],
                                           distinct(rng, 1000, cols - 1000, n + 4)]))
        mpos = np.concatenate([[0], np.sort(rng.choice(np.arange(2, n + 6), size=n - 2, replace=False)), [n + 7]])
        bld.planned(n, rng.integers(2, 8, size=6), T, width=w, universe=universe, mpos=mpos, ends=True)
        bld.b[-6] = np.unique(np.concatenate([bld.b[-6], [0, 1]]))
        bld.b[-1] = np.unique(np.concatenate([bld.b[-1], [cols - 2, cols - 1]]))
    c = int(rng.integers(1000, cols - 1000))
    others = np.array([c - 1000, c - 1, c + 1, c + 1000])
    bld.row([c], [np.array([c - 1, c, c + 1]), np.array([c - 1000, c]), np.array([c, c + 1000])], width=8, one="hit", batch=8)
    bld.row([c], [others, others[:2], others[2:], others[1:3]], width=8, one="missed", batch=8)
    return bld.case(("default", "g0", "g0l0"))


# ---------------------------------------------------------------------------------------------------- f: second trips
def strided_case(name, seed, groups, cols, inner, runs):
    """groups: [(rows, shortest mask row, longest mask row)], interleaved at random; a mask row is first, first + step, ..;
    A: two entries per row; B: rows of at most 8 entries.  Built with array operations only."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(lo, hi + 1, size=rows) for rows, lo, hi in groups])
    lens = lens[rng.permutation(len(lens))]
    rows = len(lens)
    step = rng.integers(1, 4, size=rows)
    first = rng.integers(0, cols - (lens - 1) * step)
    M = csr_of_lens(lens, first, step, cols, rng)
    k = np.sort(rng.integers(0, inner - 1, size=(rows, 2)), axis=1)
    k[:, 1] += 1                                                         # two distinct ascending rows of B
    A = po.HostCSR(rows, inner, 2 * np.arange(rows + 1), k.ravel(), rng.choice(VALUES, size=2 * rows))
    b_lens = rng.integers(0, 9, size=inner)
    b_step = rng.integers(1, cols // 8, size=inner)
    B = csr_of_lens(b_lens, rng.integers(0, cols - 7 * b_step), b_step, cols, rng)
    return A, B, M, lens


@functools.lru_cache(maxsize=None)
def case_trips_groups():
    groups = [(GRID_ROWS["g8"] + 70, 1, 32), (GRID_ROWS["g16"] + 70, 33, 64), (GRID_ROWS["g32"] + 70, 65, 128),
              (GRID_ROWS["g64"] + 70, 129, 256)]
    A, B, M, lens = strided_case("trips_groups", 606, groups, 1024, 4096, ("default",))
    lists = {"default": np.searchsorted([32, 64, 128], lens)}           # at most 16 products a row: the length decides
    return Case("trips_groups", A, B, M, ("default",), lists)


@functools.lru_cache(maxsize=None)
def case_trips_workgroups():
    groups = [(GRID_ROWS["lds_s"] + 70, 1, 1024), (GRID_ROWS["lds_l"] + 20, 1025, 1400)]
    A, B, M, lens = strided_case("trips_workgroups", 707, groups, 8192, 2048, ("g0", "g0l0"))
    lists = {"g0": np.where(lens <= 1024, LISTS.index("lds_s"), LISTS.index("lds_l")),
             "g0l0": np.full(len(lens), LISTS.index("global"))}
    return Case("trips_workgroups", A, B, M, ("g0", "g0l0"), lists)


# ---------------------------------------------------------------------------------------------------- h: stream forks
STREAM_GROUPS = (("g8",), ("g16", "g32"), ("g64",), ("lds_s", "lds_l", "global"))


@functools.lru_cache(maxsize=None)
def fork_cases():
    """[(subset of the four stream groups, Case)]: one M and one B; A holds the rows of the subset's groups only"""
    bld = Builder("forks", 1 << 14, 808)
    rng = bld.rng
    group_of = []
    for g, (n, width) in enumerate(((5, 8), (50, 16), (100, 32), (200, 64), (300, 8), (1100, 8))):
        for _ in range(6):
            bld.planned(n, rng.integers(1, 9, size=int(rng.integers(2, 14))), width if n <= 256 else 256, width=width)
            group_of.append(min(g, 1) if g < 2 else 1 if g == 2 else 2 if g == 3 else 3)
    full = bld.case(("default",))
    group_of = np.array(group_of)
    len_a = np.diff(full.A.row_offsets.astype(np.int64))
    out = []
    for bits in range(1, 16):
        subset = tuple(g for g in range(4) if bits >> g & 1)
        keep = np.isin(group_of, subset)
        entry_kept = np.repeat(keep, len_a)
        ro = np.zeros(full.A.rows + 1, dtype=np.uint32)
        ro[1:] = np.cumsum(np.where(keep, len_a, 0))
        A = po.HostCSR(full.A.rows, full.A.cols, ro, full.A.col_ids[entry_kept], full.A.data[entry_kept])
        lists = {"default": np.where(keep, full.lists["default"], IDLE)}
        out.append((subset, Case(f"forks{bits}", A, full.B, full.M, ("default",), lists)))
    return out


# ---------------------------------------------------------------------------------------------------- i: column checks
def tile_case(shape, seed=909):
    """rows = 2 tiles + 3 at either tile size of the classifying pass; one empty row of M and of A in the second tile"""
    tile, per_row, cols = t_tiles.SHAPES[shape]
    rng = np.random.default_rng(seed + tile)
    rows = 2 * tile + 3
    after_empty = tile + 6
    lens_m, lens_a = (rng.integers(per_row - 2, per_row + 3, size=rows) for _ in range(2))
    lens_m[after_empty - 1] = lens_a[after_empty - 1] = 0
    M = t_add.from_lengths(lens_m, cols, seed + 1)
    A = t_add.from_lengths(lens_a, cols, seed + 2)
    B = t_add.from_lengths(rng.integers(1, 8, size=cols), cols, seed + 3)
    as_po = lambda H: po.HostCSR(H.rows, H.cols, H.row_offsets, H.col_ids, rng.choice(VALUES, size=H.nnz))
    return as_po(A), as_po(B), as_po(M), (tile, tile - 1, rows - 1, after_empty)


def hostile_columns(A, B, M, rows_at):
    """[(operand, its column ids with one fault, status)]"""
    cases = []
    for r in rows_at:
        m0, m1 = int(M.row_offsets[r]), int(M.row_offsets[r + 1])
        a0, a1 = int(A.row_offsets[r]), int(A.row_offsets[r + 1])
        assert m1 - m0 >= 2 and a1 - a0 >= 2
        for i in (m0, m1 - 2):                                       # the first two entries, the last two
            equal, desc = M.col_ids.copy(), M.col_ids.copy()
            equal[i + 1] = equal[i]
            desc[i], desc[i + 1] = M.col_ids[i + 1], M.col_ids[i]
            cases += [("M", equal, ERR_UNSORTED), ("M", desc, ERR_UNSORTED)]
        beyond = M.col_ids.copy()
        beyond[m1 - 1] = B.cols                                      # (still ascending: only the range is wrong)
        cases.append(("M", beyond, ERR_UNSORTED))
        for i in (a0, a0 + 1, a1 - 2, a1 - 1):
            bad = A.col_ids.copy()
            bad[i] = B.rows
            cases.append(("A", bad, ERR_INVALID))
    return cases


def overlapping_mask(M, cols, rng):
    """the rows of M shifted so that every row starts below the last column of the row before it: a valid mask"""
    lens = np.diff(M.row_offsets.astype(np.int64))
    first = np.where(np.arange(M.rows) % 2 == 0, 1, 0)
    return csr_of_lens(lens, first, np.full(M.rows, 2), cols, rng)


# ==================================================================================================== the GPU side
def run_exact(cfg, case, dtype, full, views=None):
    """one call per option setting of the case: offsets, column ids and VALUES byte for byte, the statistics from the
    patterns"""
    X = case.expect()
    views = views or (to_dev(as_dtype(case.A, dtype)), to_dev(as_dtype(case.B, dtype)), to_dev(case.M))
    for run in case.runs:
        group_max, lds_max = RUNS[run]
        cfg.set_option("mask_group_max", group_max)
        cfg.set_option("mask_lds_max", lds_max)
        dC, info = sa.multiply_masked(*views, cfg, full_pattern=full)
        got = dC.to_host()
        ro, ci, data = (X.full_ro, X.full_ci, X.full_data) if full else (X.ro, X.ci, X.data)
        assert dC.dtype == np.dtype(dtype) and (got.rows, got.cols) == (X.rows, X.cols), (case.name, run)
        assert got.nnz == len(ci) == info.nnz_out, (case.name, run)
        assert got.row_offsets.tobytes() == ro.tobytes(), (case.name, run, "row_offsets differ")
        assert got.col_ids.tobytes() == ci.tobytes(), (case.name, run, "col_ids differ")
        wrong = np.flatnonzero(got.data != data.astype(dtype))
        assert got.data.tobytes() == data.astype(dtype).tobytes(), (case.name, run, "values differ", len(wrong), wrong[:5])
        assert (info.rows_idle, info.products, info.hits) == (X.rows_idle, X.products, X.hits), (case.name, run)
        assert info.rows_class == X.classes(group_max, lds_max), (case.name, run)
    cfg.set_option("mask_group_max", sa.MASK_GROUP_MAX)
    cfg.set_option("mask_lds_max", sa.MASK_LDS_MAX)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_every_group_width_at_its_mask_lengths_with_both_walks(cfg, dtype, full):
    """a. For L = 8, 16, 32, 64: mask rows of 1, 2, 4 L - 1, 4 L entries and the shortest the width takes by length alone;
    rows of A of 1, L - 1, L, L + 1, 2 L, 2 L + 1 (L = 64: also 4 L + 3) entries; per batch shape a row whose batches all
    take the team walk (with exactly 16 nb products, and with a few more), one whose batches all take the flattened walk
    (16 nb - 1 products; 1, 4 L - 1, 4 L, 4 L + 1), and rows that alternate.  Team batches meet rows of B of 0, 1, 7, 8, 9,
    31, 32, 33 entries; flat ones have empty rows of B first, last and in the middle.

    Unreachable by the width rule, and therefore absent (test_masked_edges_host.py proves each from the literal rule):
      * a mask row of at most 2 L entries reaches a width L > 8 only with 288 / 544 / 1056 products or more -- so no row of
        it whose batches all take the flattened walk unless 16 len_a - batches reaches that number (L = 64: only 2 L
        entries of A and more), and no single flat batch;
      * L < 64 holds at most 287 / 543 / 1055 products: a third full team-walk batch (48 L products) does not exist, nor
        does the team walk of 2 L + 1 entries with more than the minimum in every batch (the surplus is cut to what fits)."""
    case, _ = case_widths()
    run_exact(cfg, case, dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_group_width_chosen_by_the_products(cfg, dtype, full):
    """b. Mask rows of 1 and 4 entries with 287 / 288, 543 / 544, 1055 / 1056 products, and two rows of 1.2 M products
    (beyond the saturation of the classifying pass' per-row count); again in the LDS class (mask_group_max = 0)"""
    run_exact(cfg, case_products(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_second_and_third_batches_of_a_in_the_workgroup_classes(cfg, dtype, full):
    """c. Rows of A of T - 1, T, T + 1, 2 T + 1 entries for T = 256 (small LDS launch) and 1024 (large one; global class with
    both limits 0); batch totals of 0, 1, 4 T - 1 and 4 T; a mask entry hit in the last batch only"""
    run_exact(cfg, case_batches(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_lds_table_at_its_sizes_and_with_wrapping_clusters(cfg, dtype, full):
    """d. Mask rows on both sides of every table size; a cluster that starts in the last 8 slots and wraps, with columns
    homed in slots 0 - 3 displaced by it; 300 columns with one home slot; absent columns homed inside the clusters"""
    run_exact(cfg, case_table(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_span_cut_at_both_ends_in_every_class(cfg, dtype, full):
    """e. Products on cmin - 1, cmin, cmax, cmax + 1; one-entry mask rows hit and missed by one; columns 0 and 2^27 - 1"""
    run_exact(cfg, case_span(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_group_kernels_take_a_second_trip_over_their_lists(cfg, dtype, full):
    """f. More rows of every width than its grid of 2048 workgroups serves in one trip"""
    run_exact(cfg, case_trips_groups(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_workgroup_kernels_take_a_second_trip_over_their_lists(cfg, dtype, full):
    """f. More than 2048 rows for the small LDS launch, more than 512 for the large one (mask_group_max = 0) and for the
    global class (both limits 0): the LDS slice and the table are reused for the next row"""
    run_exact(cfg, case_trips_workgroups(), dtype, full)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [4096 * 256, 1024 * 1024 + 1])
def test_full_pattern_at_size(cfg, dtype, rows):
    """g. FULL_PATTERN beyond one trip of the rebase (4096 x 256 rows: rows + 1 offsets, so 4096 * 256 rows leave the last
    trip a single one) and, fp32, of the rounding pass (8192 x 256 mask entries): M's pattern, +0.0 where nothing falls"""
    A, B, M, (e_ro, e_ci, e_va) = scan_case(rows)
    m_ro = M.row_offsets.astype(np.int64)
    key_m = np.repeat(np.arange(rows, dtype=np.int64), np.diff(m_ro)) * 8 + M.col_ids
    key_e = np.repeat(np.arange(rows, dtype=np.int64), np.diff(e_ro.astype(np.int64))) * 8 + e_ci
    values = np.zeros(M.nnz)
    values[np.searchsorted(key_m, key_e)] = e_va
    dC, info = sa.multiply_masked(to_dev(as_dtype(A, dtype)), to_dev(as_dtype(B, dtype)), to_dev(M), cfg, full_pattern=True)
    got = dC.to_host()
    assert (got.rows, got.cols, got.nnz) == (rows, 8, M.nnz) and info.nnz_out == M.nnz
    assert info.hits == len(e_ci) and info.products == 2 * rows
    assert got.row_offsets.tobytes() == M.row_offsets.tobytes(), "row_offsets differ"
    assert got.col_ids.tobytes() == M.col_ids.tobytes(), "col_ids differ"
    assert got.data.dtype == np.dtype(dtype) and got.data.tobytes() == values.astype(dtype).tobytes(), "values differ"


@pytest.mark.parametrize("guard", [0, 4096])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", MODES)
def test_every_combination_of_stream_groups_on_one_config(guard, dtype, full):
    """h. One call per non-empty subset of the four stream groups (G8, G16 | G32, G64, LDS | global) in shuffled order on one
    config, then all four after one: which groups have work decides whether the call forks and which events it waits for"""
    cfg = sa.spECKConfig.initialize(0)
    try:
        if guard:
            cfg.set_option("guard_bytes", guard)
        cases = fork_cases()
        dB, dM = to_dev(as_dtype(cases[0][1].B, dtype)), to_dev(cases[0][1].M)
        order = [int(i) for i in np.random.default_rng(11).permutation(len(cases))]
        single = next(i for i, (subset, _) in enumerate(cases) if subset == (2,))
        for i in order + [single, len(cases) - 1]:
            subset, case = cases[i]
            run_exact(cfg, case, dtype, full, views=(to_dev(as_dtype(case.A, dtype)), dB, dM))
    finally:
        if guard:
            cfg.set_option("guard_bytes", 0)
        cfg.cleanup()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(t_tiles.SHAPES))
def test_column_checks_by_position(cfg, shape, dtype):
    """i. An equal pair, a descending pair, an id = cols(B) as the last entry of a mask row, an id of A = rows(B) -- on the
    first two and the last two entries of the first row of a tile, of the last row of a tile, of the last row of the
    matrix and of the row behind an empty row, at both tile sizes.  Each is refused with its status, C and its struct
    stay as they were byte for byte, a valid call succeeds afterwards."""
    A, B, M, rows_at = tile_case(shape)
    A, B = as_dtype(A, dtype), as_dtype(B, dtype)
    t_tiles.picks_long_tile(shape, A, M)
    d = {"A": to_dev(A), "B": to_dev(B), "M": to_dev(M)}
    good = {"A": A.col_ids, "M": M.col_ids}
    out = t_tiles.Sentinels(dtype, A.rows, B.cols)
    for which, bad, status in hostile_columns(A, B, M, rows_at):
        _update(d[which], ci=bad)
        for full in MODES:
            with pytest.raises(sa.SpeckError) as e:
                sa.multiply_masked(d["A"], d["B"], d["M"], cfg, matOut=out.dC, full_pattern=full)
            assert e.value.status == status, (which, status)
            out.untouched()
        _update(d[which], ci=good[which])
    case = Case("tiles", A, B, M, ("default",), None)
    for full in MODES:
        run_exact(cfg, case, dtype, full, views=(d["A"], d["B"], d["M"]))


@pytest.mark.parametrize("shape", sorted(t_tiles.SHAPES))
def test_rows_that_start_below_the_end_of_the_row_before_are_valid(cfg, shape):
    """i, the control: a mask whose every row's first column is below the last column of the row before it (the first
    entry of a tile and of a row is exempt from the ascent check) is not refused"""
    A, B, M, _ = tile_case(shape)
    M = overlapping_mask(M, B.cols, np.random.default_rng(5))
    ro = M.row_offsets.astype(np.int64)
    nonempty = np.flatnonzero(np.diff(ro) > 0)
    firsts, lasts = M.col_ids[ro[nonempty]], M.col_ids[ro[nonempty + 1] - 1]
    assert (firsts[1:] < lasts[:-1]).all()
    t_tiles.picks_long_tile(shape, A, M)
    for full in MODES:
        run_exact(cfg, Case("overlap", A, B, M, ("default",), None), np.float64, full)
