"""The decision rules of the masked product (speck_amd/csrc/masked_rules.hpp) and the inputs of tests/test_gpu_masked_edges.py,
without a GPU.

The call cannot report which kernel served a row, so the GPU tests rest on two facts proven here:
  * the real header, compiled for the host (tests/cpp/masked_probe.cpp), answers as the rules written down below as
    literal thresholds -- at every threshold and one beside it;
  * every input of the GPU file, built by the same generators, puts each planned row into the cell it is meant for by
    those literal rules AND by the real header: its list and group width, the walk of each of its batches, the number of
    batches, the table's size, the clusters in the table, and lists longer than one trip of their grid.
"""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_masked_edges as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rules, as tables of thresholds -----------------------------------------------------------------------------
GROUP_MAX, LDS_SMALL, LDS_MAX = 256, 1024, 4096
LEN_LANES = ((32, 8), (64, 16), (128, 32), (256, 64))      # a mask row of up to .. entries needs .. lanes
OPS_LANES = ((287, 8), (543, 16), (1055, 32))              # up to .. products ask for .. lanes; more: 64
TABLE_BITS = ((8, 4), (16, 5), (32, 6), (64, 7), (128, 8), (256, 9), (512, 10), (1024, 11), (2048, 12), (4096, 13))
OPS_CEILING = OPS_ADD_CAP = 1 << 20                        # the per-row count stops growing there; one add brings that at most
G8, G16, G32, G64, LDS_S, LDS_L, GLOBAL = range(7)
LIST_OF_LANES = {8: G8, 16: G16, 32: G32, 64: G64}


def literal_list(n, ops, group_max=GROUP_MAX, lds_max=LDS_MAX):
    if n <= min(group_max, GROUP_MAX):
        by_len = next(lanes for top, lanes in LEN_LANES if n <= top)
        by_ops = next((lanes for top, lanes in OPS_LANES if ops <= top), 64)
        return LIST_OF_LANES[max(by_len, by_ops)]
    if n <= min(lds_max, LDS_MAX):
        return LDS_S if n <= LDS_SMALL else LDS_L
    return GLOBAL


def literal_bits(n):
    return next(bits for top, bits in TABLE_BITS if n <= top)


def literal_team(total, nb):
    return total > 16 * nb - 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("masked") / "masked_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           "-I", os.path.join(ROOT, "speck_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "masked_probe.cpp"), "-o", exe])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines) and not any(o.startswith("error") for o in out), out[:3]
        return [[int(x) for x in o.split()] for o in out]
    return ask


# ---------------------------------------------------------------------------------------------------- the header
def test_constants(probe):
    assert probe(["K"]) == [[OPS_CEILING, OPS_ADD_CAP, GROUP_MAX, LDS_MAX, LDS_SMALL, 7]]
    assert (g.sa.MASK_GROUP_MAX, g.sa.MASK_LDS_MAX) == (GROUP_MAX, LDS_MAX)


def test_list_of_a_row_at_every_threshold(probe):
    lens = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 100_000]
    ops = [0, 1, 286, 287, 288, 289, 542, 543, 544, 545, 1054, 1055, 1056, 1057, OPS_CEILING - 1, OPS_CEILING,
           OPS_CEILING + OPS_ADD_CAP - 1, 2 * OPS_CEILING]
    limits = [(256, 4096), (0, 4096), (0, 0), (64, 4096), (63, 4096), (256, 1000), (256, 1024), (256, 1025), (300, 5000),
              (33, 40), (0, 2)]
    queries = [(n, o, gm, lm) for gm, lm in limits for n in lens for o in ops]
    got = probe([f"L {n} {o} {gm} {lm}" for n, o, gm, lm in queries])
    for q, (answer,) in zip(queries, got):
        assert answer == literal_list(*q), q
    # the cells by name, so that a slip in literal_list itself does not go unnoticed
    named = {(1, 0): G8, (32, 287): G8, (33, 0): G16, (1, 288): G16, (64, 543): G16, (65, 0): G32, (1, 544): G32,
             (128, 1055): G32, (129, 0): G64, (1, 1056): G64, (4, OPS_CEILING): G64, (256, 0): G64, (257, 0): LDS_S,
             (1024, 0): LDS_S, (1025, 0): LDS_L, (4096, 0): LDS_L, (4097, 0): GLOBAL}
    for (n, o), want in named.items():
        assert literal_list(n, o) == want and probe([f"L {n} {o} 256 4096"]) == [[want]], (n, o)
    # lowered limits: rows beyond mask_group_max leave the group class, rows beyond mask_lds_max the LDS class
    assert [literal_list(n, 0, 64, 4096) for n in (64, 65)] == [G16, LDS_S]
    assert [literal_list(n, 0, 256, 1024) for n in (1024, 1025)] == [LDS_S, GLOBAL]
    assert [literal_list(n, 0, 0, 0) for n in (1, 5000)] == [GLOBAL, GLOBAL]
    assert [literal_list(n, 0, 10_000, 10_000) for n in (256, 257, 4096, 4097)] == [G64, LDS_S, LDS_L, GLOBAL]


def test_table_bits_and_slots(probe):
    ns = [1, 2, 7, 8, 9, 16, 17, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096]
    got = probe([f"B {n}" for n in ns])
    for n, (bits,) in zip(ns, got):
        assert bits == literal_bits(n), n
        assert (1 << bits) >= max(2 * n, 16) and ((1 << bits) == 16 or (1 << (bits - 1)) < 2 * n)   # the smallest such power of two
    assert [literal_bits(n) for n in (1, 8, 9, 512, 513, 1024, 1025, 2048, 2049, 4096)] == [4, 4, 5, 10, 11, 11, 12, 12, 13, 13]
    rng = np.random.default_rng(1)
    cols = [0, 1, 2, (1 << 27) - 1, (1 << 27) - 2, 0x7FFFFFFF] + [int(c) for c in rng.integers(0, 1 << 27, size=300)]
    queries = [(c, bits) for c in cols for bits in (4, 5, 10, 11, 12, 13)]
    got = probe([f"S {c} {bits}" for c, bits in queries])
    for (c, bits), (slot,) in zip(queries, got):
        assert slot == g.py_slot(c, bits) == ((c * 0x9E3779B1) % (1 << 32)) // (1 << (32 - bits)) < (1 << bits), (c, bits)
    for bits in (4, 11):
        some = np.arange(5000, dtype=np.int64)
        assert g.slots_of(5000, bits).tolist() == [g.py_slot(c, bits) for c in some]


def test_walk_choice(probe):
    queries = [(t, nb) for nb in (1, 2, 7, 8, 15, 16, 31, 32, 63, 64) for t in (0, 1, 16 * nb - 1, 16 * nb, 16 * nb + 1, 1 << 20)]
    got = probe([f"W {t} {nb}" for t, nb in queries])
    for (t, nb), (team,) in zip(queries, got):
        assert team == int(literal_team(t, nb)), (t, nb)
    assert [literal_team(*q) for q in ((15, 1), (16, 1), (1023, 64), (1024, 64))] == [False, True, False, True]


# ---------------------------------------------------------------------------------------------------- the inputs
def b_rows_of(case, row):
    """the rows of B (arrays of columns) the entries of A's row meet, in order"""
    A, B = case.A, case.B
    ks = A.col_ids[int(A.row_offsets[row]):int(A.row_offsets[row + 1])]
    return [B.col_ids[int(B.row_offsets[k]):int(B.row_offsets[k + 1])] for k in ks]


def mask_row(case, row):
    return case.M.col_ids[int(case.M.row_offsets[row]):int(case.M.row_offsets[row + 1])]


def shapes(case):
    """per row: mask entries, entries of A, products"""
    A, B, M = case.A, case.B, case.M
    len_m, len_a = np.diff(M.row_offsets.astype(np.int64)), np.diff(A.row_offsets.astype(np.int64))
    b_len = np.diff(B.row_offsets.astype(np.int64))
    ops = np.bincount(np.repeat(np.arange(A.rows), len_a), weights=b_len[A.col_ids[:A.nnz]], minlength=A.rows).astype(np.int64)
    return len_m, len_a, ops


def lists_hold(case, probe):
    """every row of the case sits in the list it is meant for, under every option setting it runs with: by the literal
    rule and by the real header.  -> {run: rows per list}"""
    len_m, len_a, ops = shapes(case)
    held = np.minimum(ops, OPS_CEILING)               # what the classifying pass holds (beyond the ceiling: some value >= it)
    work = (len_m > 0) & (len_a > 0)
    counts = {}
    for run in case.runs:
        gm, lm = g.RUNS[run]
        want = np.array([literal_list(int(n), int(o), gm, lm) if w else g.IDLE for n, o, w in zip(len_m, held, work)])
        assert (want == case.lists[run]).all(), (case.name, run, np.flatnonzero(want != case.lists[run])[:5])
        cells = sorted({(int(n), int(o)) for n, o in zip(len_m[work], held[work])})
        cells += [(n, o + OPS_ADD_CAP - 1) for n, o in cells if o == OPS_CEILING]      # the largest value it can hold
        got = probe([f"L {n} {o} {gm} {lm}" for n, o in cells])
        for (n, o), (answer,) in zip(cells, got):
            assert answer == literal_list(n, o, gm, lm), (case.name, run, n, o)
        counts[run] = np.bincount(want[work], minlength=7)
    return counts


def batches_of(lens, batch):
    return [lens[i:i + batch] for i in range(0, len(lens), batch)]


def hit_batches(b_rows, batch, column):
    """the batches in which a product falls on `column`"""
    return sorted({i // batch for i, cols in enumerate(b_rows) if column in cols})


def late_holds(case, plan):
    rows, m = b_rows_of(case, plan["row"]), mask_row(case, plan["row"])
    last = (len(rows) - 1) // plan["batch"]
    assert last >= 1
    assert hit_batches(rows, plan["batch"], m[0]) == [last], plan               # hit in the last batch only
    multi = hit_batches(rows, plan["batch"], m[-1])
    assert len(multi) >= 2 and multi[0] == 0 and multi[-1] == last, plan        # hit in several batches


def hits_and_misses(case, plan):
    rows, m = b_rows_of(case, plan["row"]), mask_row(case, plan["row"])
    products = np.concatenate(rows + [np.zeros(0, np.uint32)])
    hits = int(np.isin(products, m).sum())
    return hits, len(products) - hits


def test_widths_and_walks_plan(probe):
    case, unreachable = g.case_widths()
    counts = lists_hold(case, probe)["default"]
    assert all(counts[k] >= 60 for k in (G8, G16, G32, G64)) and counts[4:].sum() == 0
    seen = {L: dict(cells=set(), team_lens=set(), flat_totals=set(), edge=set(), late=0, multi=0, alternating=0, full_team=0) for L in g.WIDTHS}
    walk_queries = []
    for plan in case.plans:
        L, row = plan["width"], plan["row"]
        assert LIST_OF_LANES[L] == case.lists["default"][row]
        n = len(mask_row(case, row))
        rows = b_rows_of(case, row)
        lens = np.array([len(r) for r in rows])
        batches = batches_of(lens, L)
        assert len(batches) == len(plan["walks"]) == (len(lens) + L - 1) // L
        s = seen[L]
        for b, (walk, total) in zip(batches, zip(plan["walks"], plan["totals"])):
            nb = len(b)
            assert int(b.sum()) == total and literal_team(total, nb) == walk, plan
            walk_queries.append((total, nb, walk))
            s["edge"].add((nb, total - 16 * nb))
            if walk:
                s["team_lens"] |= set(int(x) for x in b)
            else:
                s["flat_totals"].add(total)
                if nb >= 5:      # first, last and middle entries of A on empty rows of B
                    assert b[0] == 0 and b[-1] == 0 and b[nb // 2] == 0 and b[nb // 3] == 0, plan
        s["cells"].add((n, len(lens), plan["variant"]))
        s["full_team"] = max(s["full_team"], sum(1 for b, walk in zip(batches, plan["walks"]) if walk and len(b) == L))
        s["alternating"] += len(set(plan["walks"])) == 2
        hits, misses = hits_and_misses(case, plan)
        if hits + misses >= 2:
            assert hits > 0 and misses > 0, plan
        # wherever the lengths allow it, a mask entry is hit in the last batch only and another one in several batches
        can_late = len(batches) >= 2 and n >= 3 and batches[0].sum() > 0 and (batches[-1].max() >= 3 or (batches[-1] > 0).sum() >= 3)
        assert plan["late"] == can_late, plan
        if plan["late"]:
            late_holds(case, plan)
            s["late"] += 1
        s["multi"] += len(batches) >= 2 and n >= 3
    got = probe([f"W {t} {nb}" for t, nb, _ in walk_queries])
    assert [x for (x,) in got] == [int(w) for _, _, w in walk_queries]
    for L, s in seen.items():
        # the totals on either side of the walk choice: a full batch, a partial one, a single entry
        for nb in (L, L - 1, 1):
            assert {(nb, -1), (nb, 0)} <= s["edge"], (L, nb)
        assert set(g.TEAM_LENS) <= s["team_lens"], L
        assert {1, 4 * L - 1, 4 * L, 4 * L + 1, 16 * L - 1} <= s["flat_totals"], L
        assert s["alternating"] >= 4 and s["late"] >= 0.8 * s["multi"] and s["late"] >= 25, (L, s["late"], s["multi"])
        # every cell is either planned or provably out of reach of the width rule
        for n in g.MASK_LENS[L]:
            for len_a in g.a_lens(L):
                nbs = [L] * (len_a // L) + ([len_a % L] if len_a % L else [])
                for variant in g.VARIANTS:
                    if variant in ("team_flat", "flat_team") and len(nbs) < 2:
                        continue
                    if (n, len_a, variant) in s["cells"]:
                        assert (L, n, len_a, variant) not in unreachable
                        continue
                    assert (L, n, len_a, variant) in unreachable
                    team = [{"team": True, "team_more": True, "flat": False, "flat_tails": False, "team_flat": b % 2 == 0,
                             "flat_team": b % 2 == 1}[variant] for b in range(len(nbs))]
                    fewest = sum(16 * nb for nb, t in zip(nbs, team) if t)
                    most = None if any(team) else sum(16 * nb - 1 for nb in nbs)
                    if variant == "flat_tails":      # its batch totals are the four around the unroll, where they are flat
                        most = sum(max(t for t in (1, 4 * L - 1, 4 * L, 4 * L + 1) if t <= 16 * nb - 1) for nb in nbs)
                    reachable = [o for o in (fewest, most, 287, 288, 543, 544, 1055, 1056, 5000)
                                 if o is not None and o >= fewest and (most is None or o <= most)
                                 and literal_list(n, o) == LIST_OF_LANES[L]]
                    assert not reachable, (L, n, len_a, variant, reachable)
    # a third full team-walk batch exists for L = 64 only
    assert {L: s["full_team"] for L, s in seen.items()} == {8: 2, 16: 2, 32: 2, 64: 4}


def test_products_plan(probe):
    case = g.case_products()
    counts = lists_hold(case, probe)
    assert (counts["default"][:4] > 0).all() and counts["g0"][LDS_S] == case.A.rows
    _, len_a, ops = shapes(case)
    for plan in case.plans:
        row = plan["row"]
        if plan.get("saturated"):
            assert ops[row] == g.SATURATING[0] * g.SATURATING[1] > OPS_CEILING and len_a[row] > 256     # two batches in the LDS class
            assert case.lists["default"][row] == G64
        else:
            assert ops[row] == plan["ops"] and LIST_OF_LANES[plan["width"]] == case.lists["default"][row]
            hits, misses = hits_and_misses(case, plan)
            assert hits > 0 and misses > 0
    by_ops = {(len(mask_row(case, p["row"])), p["ops"]): case.lists["default"][p["row"]] for p in case.plans if "ops" in p}
    assert by_ops == {(n, o): k for n in (1, 4) for o, k in ((287, G8), (288, G16), (543, G16), (544, G32), (1055, G32), (1056, G64))}
    X = case.expect()
    assert X.row_hits[-2:].min() > 0                  # the saturating rows produce something


def test_batches_plan(probe):
    case = g.case_batches()
    counts = lists_hold(case, probe)
    assert counts["default"][LDS_S] == counts["default"][LDS_L] == 6 and counts["g0l0"][GLOBAL] == 12
    for T, name in ((256, "lds_s"), (1024, "lds_l")):
        plans = [p for p in case.plans if case.lists["default"][p["row"]] == g.LISTS.index(name)]
        assert all(p["batch"] == T == g.THREADS[name] for p in plans)
        lens_a, remainders, late = set(), set(), 0
        for plan in plans:
            lens = np.array([len(r) for r in b_rows_of(case, plan["row"])])
            lens_a.add(len(lens))
            assert lens.max() <= (4 if plan["kind"] == "remainders" else 3)
            for b in batches_of(lens, T):
                remainders.add((int(b.sum()) % (4 * T), int(b.sum()) > 0))
                if len(b) >= 3 and b.max() <= 3:
                    assert b[0] == 0 and b[-1] == 0, plan          # empty rows of B first and last in the batch
            if plan["late"]:
                late_holds(case, plan)
                late += 1
            hits, misses = hits_and_misses(case, plan)
            assert hits > 0 and misses > 0
        assert {T - 1, T, T + 1, 2 * T + 1, 3 * T} <= lens_a
        assert {(0, True), (0, False), (1, True), (4 * T - 1, True)} <= remainders
        assert late >= 2            # (the rows of T + 1 and 2 T + 1 entries: the others end in a batch without three products)
    # the global class (both limits 0) batches the rows of the large launch in the same way: 1024 threads
    assert g.THREADS["global"] == g.THREADS["lds_l"]


def occupied_slots(columns, bits):
    """the slots a linear-probing table holds after the columns were inserted: the set does not depend on the order"""
    slots, used = 1 << bits, set()
    for c in columns:
        s = g.py_slot(c, bits)
        while s in used:
            s = (s + 1) % slots
        used.add(s)
    return used


def probe_path(column, used, bits):
    """the slots a look-up of an absent column reads: up to and including the first empty one"""
    slots, s, path = 1 << bits, g.py_slot(column, bits), []
    while s in used:
        path.append(s)
        s = (s + 1) % slots
    return path + [s]


def test_table_plan(probe):
    case = g.case_table()
    counts = lists_hold(case, probe)
    assert counts["default"][LDS_S] >= 6 and counts["default"][LDS_L] >= 5 and counts["g0"][:4].sum() == 0
    sizes, kinds = set(), set()
    for plan in case.plans:
        m = mask_row(case, plan["row"])
        n, bits = len(m), literal_bits(len(m))
        assert probe([f"B {n}"]) == [[bits]]
        if plan["kind"] == "size":
            sizes.add(n)
            continue
        assert bits == plan["bits"]
        slots = 1 << bits
        used = occupied_slots(m, bits)
        rows = b_rows_of(case, plan["row"])
        products = np.unique(np.concatenate(rows))
        absent = np.setdiff1d(products, m)
        assert len(absent) >= 0.4 * len(plan["absent"]) and np.isin(absent, plan["absent"]).all()
        assert (absent > m[0]).all() and (absent < m[-1]).all()            # inside the span: the span cut keeps them
        assert np.isin(m, products).sum() >= 0.3 * n                       # ... and rows of B with the present columns
        homes = np.array([g.py_slot(c, bits) for c in m])
        if plan["kind"] == "one_home":
            assert len(set(homes)) == 1 and n >= 300                       # every insertion contends for the same words
            home = int(homes[0])
            assert used == {(home + i) % slots for i in range(n)}
            assert all(len(probe_path(c, used, bits)) == n + 1 for c in absent)      # an absent column walks the whole cluster
        else:
            tail = 4 if bits == 4 else 8
            in_tail = homes >= slots - tail
            assert in_tail.sum() > tail and (homes[~in_tail] <= 3).all() and (~in_tail).sum() >= 2
            # the cluster that starts in the last slots runs through the table's end into its first slots ...
            wrapped = in_tail.sum() - tail
            assert {slots - 1, 0} <= used and set(range(wrapped)) <= used
            # ... so the columns homed in slots 0 - 3 are displaced behind it, and absent columns walk through the wrap
            through = [c for c in absent if g.py_slot(c, bits) >= slots - tail and probe_path(c, used, bits)[-1] < slots - tail]
            assert len(through) >= min(4, len(absent) // 2), plan
            assert any(g.py_slot(c, bits) <= 3 for c in absent)
        kinds.add((plan["kind"], bits))
    assert sizes == {1, 2, 7, 8, 9, 257, 512, 513, 1024, 1025, 2048, 2049, 4096}
    assert kinds == {("wrap", 4), ("wrap", 11), ("wrap", 12), ("one_home", 10)}
    # with mask_group_max = 0 the rows of 1 .. 9 entries are in the LDS class: 16 and 32 slots
    small = [p["row"] for p in case.plans if len(mask_row(case, p["row"])) <= 9]
    assert (case.lists["g0"][small] == LDS_S).all() and (case.lists["default"][small] == G8).all()


def test_span_plan(probe):
    case = g.case_span()
    counts = lists_hold(case, probe)
    assert counts["default"][G8] and counts["default"][G16] and counts["default"][LDS_S] and counts["default"][LDS_L]
    assert counts["g0"][LDS_S] and counts["g0"][LDS_L] and counts["g0l0"][GLOBAL] == case.A.rows
    cols = case.B.cols
    assert cols == 1 << 27
    spans = ends = 0
    for plan in case.plans:
        m = mask_row(case, plan["row"])
        products = np.unique(np.concatenate(b_rows_of(case, plan["row"])))
        if plan.get("span"):
            assert np.isin([m[0] - 1, m[0], m[-1], m[-1] + 1], products).all(), plan
            spans += 1
        if plan.get("ends"):
            assert m[0] == 0 and m[-1] == cols - 1 and np.isin([0, 1, cols - 2, cols - 1], products).all()
            assert 1 not in m and cols - 2 not in m
            ends += 1
        if plan.get("one") == "hit":
            assert len(m) == 1 and np.isin([m[0] - 1, m[0], m[0] + 1], products).all()
        if plan.get("one") == "missed":
            assert len(m) == 1 and m[0] not in products and np.isin([m[0] - 1, m[0] + 1], products).all()
    assert spans == ends == 5 and {p.get("one") for p in case.plans} >= {"hit", "missed"}


def test_second_trips_plan(probe):
    case = g.case_trips_groups()
    counts = lists_hold(case, probe)["default"]
    for k, name in enumerate(g.LISTS[:4]):
        assert g.GRID_ROWS[name] < counts[k] <= g.GRID_ROWS[name] + 100, name
    assert g.GRID_ROWS == {"g8": 65536, "g16": 32768, "g32": 16384, "g64": 8192, "lds_s": 2048, "lds_l": 512, "global": 512}
    case = g.case_trips_workgroups()
    counts = lists_hold(case, probe)
    assert counts["g0"][LDS_S] > g.GRID_ROWS["lds_s"] and counts["g0"][LDS_L] > g.GRID_ROWS["lds_l"]
    assert counts["g0l0"][GLOBAL] > g.GRID_ROWS["global"]
    for c in (g.case_trips_groups(), case):
        X = c.expect()
        assert 0 < X.hits < X.products and 0 < X.found.sum() < c.M.nnz


def test_fork_plan(probe):
    cases = g.fork_cases()
    assert sorted(subset for subset, _ in cases) == sorted(
        tuple(k for k in range(4) if bits >> k & 1) for bits in range(1, 16))
    for subset, case in cases:
        counts = lists_hold(case, probe)["default"]
        with_work = tuple(k for k, names in enumerate(g.STREAM_GROUPS) if sum(counts[g.LISTS.index(x)] for x in names))
        assert with_work == subset
    assert cases[-1][0] == (0, 1, 2, 3)
    counts = lists_hold(cases[-1][1], probe)["default"]
    assert all(counts[k] for k in (G8, G16, G32, G64, LDS_S, LDS_L))


def test_column_check_plan():
    for shape in sorted(g.t_tiles.SHAPES):
        tile = g.t_tiles.SHAPES[shape][0]
        A, B, M, rows_at = g.tile_case(shape)
        assert A.rows == 2 * tile + 3 and rows_at == (tile, tile - 1, A.rows - 1, tile + 6)
        assert M.row_offsets[tile + 6] == M.row_offsets[tile + 5] and A.row_offsets[tile + 6] == A.row_offsets[tile + 5]
        g.t_tiles.picks_long_tile(shape, A, M)
        cases = g.hostile_columns(A, B, M, rows_at)
        assert len(cases) == 4 * 9
        places = set()
        for which, bad, status in cases:
            H = {"A": A, "M": M}[which]
            at = np.flatnonzero(bad != H.col_ids)
            row = int(np.searchsorted(H.row_offsets, at[0], side="right")) - 1
            assert row in rows_at and status == (g.ERR_INVALID if which == "A" else g.ERR_UNSORTED)
            r0, r1 = int(H.row_offsets[row]), int(H.row_offsets[row + 1])
            assert set(at) <= {r0, r0 + 1, r1 - 2, r1 - 1}
            places.add((which, row, int(at[-1]) - r0 < 2, int(r1 - at[0]) <= 2))
        assert len({(which, row) for which, row, _, _ in places}) == 8          # both operands, the four rows
        assert all({(w, r, True, False), (w, r, False, True)} <= places or (w, r, True, True) in places for w, r, _, _ in places)
        O = g.overlapping_mask(M, B.cols, np.random.default_rng(5))
        assert (np.diff(O.row_offsets.astype(np.int64)) == np.diff(M.row_offsets.astype(np.int64))).all()
