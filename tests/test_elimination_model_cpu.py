"""tests/_elimination_model.py — the Python restatement of window_lm_kernel's structure analysis — against graph theory written
independently of it, against the layout table recorded in tests/golden/kernel_layouts_table.npz, and the BRANCH every window of
tests/test_gpu_window_structures.py is there for.  A window that does not take its branch is resized here, on the CPU, until it does."""
import os
import sys

import numpy as np
import pytest

import _elimination_model as M
import _graph_families as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG_GRAPHS = [(n, [tuple(int(x) for x in p) for p in np.random.default_rng(100 + n).integers(0, n, (2 * n, 2)) if p[0] != p[1]]) for n in (3, 9, 17, 40, 64)]
GRAPHS = RNG_GRAPHS + [(20, F.ring(20)), (36, F.grid(6, 6)), (64, F.grid(8, 8)), (30, F.chain_with_clique(30, 8)), (24, F.components(24)), (12, F.clique(12)),
                       (1, []), (5, []), (77, F.arrowhead_with_pendant(70, 6)), (130, F.components(130)), (128, F.grid(8, 16))]


def dense_fill(nv, pairs, perm):
    """the factor's structure by boolean elimination of the dense adjacency matrix in the order perm (pose -> position)"""
    A = np.eye(nv, dtype=bool)
    for u, v in pairs:
        A[perm[u], perm[v]] = A[perm[v], perm[u]] = True
    for k in range(nv):
        below = np.flatnonzero(A[k + 1:, k]) + k + 1
        A[np.ix_(below, below)] = True
    return np.tril(A)


def summary(m):
    return [f"{mode}{len(cols)}" for mode, cols in zip(m.modes, m.levels)]


@pytest.mark.parametrize("natural", [False, True])
@pytest.mark.parametrize("order", ["small", "wide"])
def test_model_is_an_elimination(order, natural):
    for nv, pairs in GRAPHS:
        if order == "small" and nv > 64:
            continue
        m = M.order_small(nv, pairs, natural) if order == "small" else M.order_wide(nv, pairs, natural)
        assert sorted(m.perm) == list(range(nv))
        assert not natural or m.perm == list(range(nv))
        L = dense_fill(nv, pairs, m.perm)
        for J in range(nv):
            assert m.col[J] == (np.flatnonzero(L[:, J])[1:]).tolist(), (order, nv, J)
        assert m.nb == L.sum()
        # elimination-tree levels; a round of compute_sparse_mw is a level of independent columns that lies ABOVE every column of its rows
        want = [0] * nv
        for i in range(nv):
            want[i] = max((want[K] + 1 for K in np.flatnonzero(L[i, :i])), default=0)
        if order == "small":
            assert m.level == want
        else:
            assert all(m.level[i] >= want[i] for i in range(nv)) and all(m.level[K] < m.level[i] for i in range(nv) for K in np.flatnonzero(L[i, :i]))
            assert [J for cols in m.levels for J in cols] == list(range(nv))
        assert sorted(J for cols in m.levels for J in cols) == list(range(nv))
        for mode, cols in zip(m.modes, m.levels):
            assert (mode == "C") == all(len(m.col[J]) <= 1 and (order == "small" or len(m.row[J]) < M.DENSE_K) for J in cols)
        assert all(len(m.col[J]) == 1 and m.modes[m.level[J]] != "R" for J in m.pushed)


def test_closed_forms():
    rng = np.random.default_rng(5)
    for n in (2, 7, 40, 64):
        assert M.order_small(n, F.random_tree(rng, n)).nb == 2 * n - 1
        assert set(M.order_small(n, F.random_tree(rng, n)).modes) == {"C"}
    forest = F.random_tree(rng, 20) + [(20 + u, 20 + v) for u, v in F.random_tree(rng, 9)] + [(29 + u, 29 + v) for u, v in F.chain(6)]
    assert M.order_small(35, forest).nb == 2 * 35 - 3 and M.order_small(38, forest).nb == 2 * 38 - 6      # (38: with three isolated poses)
    for n in (3, 12, 20, 64):
        assert M.order_small(n, F.ring(n)).nb == 3 * n - 3
        assert M.order_small(min(n, 16), F.clique(min(n, 16))).nb == min(n, 16) * (min(n, 16) + 1) // 2
    m = M.order_small(10, F.chain(10))
    assert (m.nb, len(m.levels)) == (19, 6) and summary(m) == ["C2", "C2", "C2", "C2", "C1", "C1"]


def test_config5_keyframe_tree(built):
    sys.path.insert(0, os.path.join(ROOT, "tests", "perf"))
    import bench_window as bw
    from _general_cov_inputs import window_pairs
    wb = bw.build_pose64(1, np.random.default_rng(6))[0]
    m = M.order_small(64, window_pairs(wb, 0))
    assert (m.nb, len(m.levels)) == (127, 6) and set(m.modes) == {"C"}
    assert M.result7(m) == 6 * 65536 + 127


def test_the_table_of_structures():
    """what the suite's structures look like to the kernel: C column mode, R row mode, W wide-level column mode, the number = columns"""
    table = {
        "ring20": (20, F.ring(20), 57, ["R1"] * 18 + ["C1", "C1"]),
        "grid6x6": (36, F.grid(6, 6), 167, ["R11", "R4", "R4", "R3", "R2", "R2", "R2"] + ["R1"] * 6 + ["C1", "C1"]),
        "grid8x8": (64, F.grid(8, 8), 359, ["W23", "R5", "R4", "R4", "R4", "R3", "R2", "R2", "R2", "R2"] + ["R1"] * 11 + ["C1", "C1"]),
        "chain30clique8": (30, F.chain_with_clique(30, 8), 80, ["C1"] * 22 + ["R1"] * 6 + ["C1", "C1"]),
        "components24": (24, F.components(24), 56, ["R3"] * 5 + ["R2", "R2", "R1", "R1", "R1", "C1", "C1"]),
        "clique12": (12, F.clique(12), 78, ["R1"] * 10 + ["C1", "C1"]),
    }
    for name, (nv, pairs, nb, levels) in table.items():
        m = M.order_small(nv, pairs)
        assert (m.nb, summary(m)) == (nb, levels), (name, m.nb, summary(m))
    m = M.order_small(40, F._TREE40)
    assert (m.nb, len(m.levels)) == (79, 7) and set(m.modes) == {"C"}


def test_layout_predicates_against_the_recorded_table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "kernel_layouts_table.npz"))
    col = {str(n): k for k, n in enumerate(z["columns"])}
    seen = set()
    for row, want in zip(z["rows"], z["table"]):
        caps = (int(row[0]), int(row[2]), int(row[3]), int(row[4]), int(row[1]))
        if caps[0] > 512:
            continue
        assert M.nnz_capacity_blocks(caps) * 36 == want[col["nnz_capacity"]] and M.mask_words(caps) == want[col["mask_words"]]
        assert 8 * M.index_doubles(caps) == want[col["window.ws.i.bytes"]] and M.table_bytes(caps) == want[col["window.ws.t.bytes"]], caps
        assert M.index_in_lds(caps) == want[col["index_in_lds"]] and M.root_lds_doubles(caps) == want[col["root_lds_doubles"]], caps
        if caps[0] <= 64:
            assert M.lds_mode_bytes(caps) == want[col["window.lds.lds_bytes"]] and M.recA_capacity(caps) == want[col["window.lds.recA_cap"]], caps
            assert M.arrays_in_lds(caps) == want[col["window_arrays_in_lds"]], caps
        seen.add((caps[0] <= 64, bool(M.arrays_in_lds(caps)), bool(M.root_lds_doubles(caps))))
    assert seen == {(True, True, False), (True, False, False), (False, False, True), (False, False, False)}


# ---- the branch every GPU case is there for ------------------------------------------------------------------------------------------------
def models(name, natural=False):
    caps = F.batch_caps(name)
    return caps, {w[0]: M.model_for(*F.window_spec(name, i), caps, natural) for i, w in enumerate(F.BATCHES[name][3])}


def test_branches_small_lds(built):
    for name in ("lds6", "lds3"):
        caps, ms = models(name)
        assert caps[0] <= 16 and M.arrays_in_lds(caps)
        assert all(not m.pushed and not m.natural for m in ms.values())                       # (in LDS nothing is pushed)
        assert "R" in ms["ring12"].modes and "R" in ms["components14"].modes and len({m.nb for m in ms.values()}) == len(ms)
    caps, ms = models("lds3")
    assert ms["clique12"].recA_cap == ms["clique10"].recA_cap == M.recA_capacity(caps) == 224
    assert (ms["clique12"].recA, ms["clique12"].tables) == (365, False)                      # the records overflow: factor_and_solve_sparse in LDS
    assert (ms["clique10"].recA, ms["clique10"].tables) == (221, True)                       # three records from the capacity
    assert all(m.tables for m in models("lds6")[1].values()) and ms["ring12"].tables and ms["components14"].tables
    assert set(models("lds6")[1]["clique6"].modes[:-2]) == {"R"} and set(models("lds6")[1]["pad5"].modes) == {"C"}


def test_branches_small_workspace(built):
    for name in ("ws6", "ws3"):
        caps, ms = models(name)
        assert caps[0] == 64 and not M.arrays_in_lds(caps) and all(not m.natural for m in ms.values())
        assert ms["grid8x8"].modes[0] == "W" and len(ms["grid8x8"].levels[0]) >= M.WIDE_LEVEL     # the wide level: column mode whatever the columns look like
        assert max(len(ms["grid8x8"].col[J]) for J in ms["grid8x8"].levels[0]) > 1
        assert set(ms["ring20"].modes[:-2]) == {"R"} and ms["ring20"].nb == 57                 # fill created by a cycle, row mode
        assert {"C", "R"} <= set(ms["chain30clique8"].modes) and len(ms["chain30clique8"].pushed) == 23   # pushed updates feeding row-mode levels
        assert len(ms["components24"].levels[0]) == 3                                          # both components in the first level
    caps, ms = models("ws6")
    assert set(ms["tree40"].modes) == {"C"} and len(ms["tree40"].pushed) == 39 and set(ms["pad5"].modes) == {"C"}
    assert "R" in ms["grid6x6"].modes and "W" not in ms["grid6x6"].modes and len(ms["grid6x6"].levels[0]) == 11   # one column short of a wide level
    for name in ("ws6", "ws3"):   # the caller's order: more fill, a level per pose on the grids
        nat = models(name, True)[1]
        assert nat["grid8x8"].nb == 519 and len(nat["grid8x8"].levels) == 64 and all(m.natural and m.nb <= M.nnz_capacity_blocks(caps) for m in nat.values())


def test_branches_wide(built):
    for name in ("wide6", "wide3"):
        caps, ms = models(name)
        assert 64 < caps[0] <= 512 and M.root_lds_doubles(caps) and all(m.dense_ok and not m.natural for m in ms.values())
        assert (ms["ring200"].root, len(ms["ring200"].levels)) == (2, 9)                       # nested dissection: log2 levels
        assert ms["grid10x30"].dense > 0 and (ms["grid10x30"].root, ms["grid10x30"].root_run) == (M.ROOT_MAX, 18)
        assert ms["grid8x16"].root == M.ROOT_MAX and ms["ladder60"].root == 4
        assert (ms["pendant"].root, ms["pendant"].root_refused, ms["pendant"].root_run) == (0, "pushed child", 9)
        assert (ms["components130"].root, ms["components130"].root_refused) == (0, "no clique")   # two components: no trailing clique
        assert all("W" not in m.modes for m in ms.values())                                    # (eight waves: a wide level stays in row mode)
        nat = models(name, True)[1]
        assert not nat["grid10x30"].dense_ok and nat["grid10x30"].root_refused == "dense list overflowed"   # 2 139 entries for 600 places
        assert all(len(m.levels) == len(m.perm) for m in nat.values()) and nat["pendant"].root == 7
    caps, ms = models("wide6")
    assert (ms["arrowhead70+6"].root, ms["arrowhead70+6"].root_run) == (9, 9)                  # the border and the chain's last poses
    assert (ms["arrowhead64+12"].root, ms["arrowhead64+12"].root_run) == (M.ROOT_MAX, 14)      # stops at ROOT_MAX
    caps, ms = models("selfcal6")
    assert M.root_lds_doubles(caps) and (ms["arrow70+6"].root, ms["arrow64+12"].root, ms["arrow64+12"].root_run) == (9, M.ROOT_MAX, 14)
    assert ms["arrow64+12"].dense >= 2 * 12


def test_branches_dense_list(built):
    for name in ("dense6", "dense3"):
        caps, ms = models(name)
        assert caps[0] == 66 and M.root_lds_doubles(caps)
        a, b = ms["chain66clique48"], ms["chain60clique30"]
        assert (a.dense, a.dense_cap, a.dense_ok, a.root_refused) == (324, 132, False, "dense list overflowed")
        assert (b.dense, b.dense_ok) == (27, True) and b.root_run == 30


def test_skyline_and_fallback(built):
    caps = F.batch_caps("sky6")
    assert caps[0] == 520 and caps[4] == 40 and M.model_for(*F.window_spec("sky6", 0), caps) is None
    found = F.fallback_graph()
    assert found is not None, "no fallback graph in 10 000 draws"
    draw, nv, band, pairs = found
    caps, ms = models("fallback6")
    print(f"fallback search: draw {draw}: {nv} poses, band {band}: minimum-degree fill {M.order_small(nv, pairs).nb} blocks, capacity {M.nnz_capacity_blocks(caps)}")
    assert caps[0] == nv and caps[4] == band and nv <= 64
    assert M.order_small(nv, pairs).nb > M.nnz_capacity_blocks(caps) >= ms["banded"].nb and ms["banded"].natural
    assert not ms["chain30"].natural and not ms["ladder10"].natural and "R" in ms["ladder10"].modes
