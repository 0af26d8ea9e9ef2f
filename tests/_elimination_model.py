"""Test helper: what window_lm_kernel's structure analysis (localization_amd/csrc/window_kernel.hip: compute_sparse, compute_sparse_mw,
build_small_tables) decides from a window's graph alone, restated in plain Python from the kernel's text — and the few layout predicates of
window_layouts.h those decisions depend on.  Its only job is to tell the tests which branch a window takes and what result[7] must be: short
and obvious, not fast.  Poses are numbers 0 .. nv - 1, `pairs` the pose-to-pose edges in any order and orientation."""
from types import SimpleNamespace

WIDE_LEVEL = 12      # window_kernel.hip
DENSE_K = 24
ROOT_MAX = 10        # window_layouts.h
WINDOW_MAX_LDS = 160 * 1024 - 512
WINDOW_WIDE_MAX_LDS = 160 * 1024 - 4096


# ---- window_layouts.h, for caps = (nv_max, nr_max, np_max, ns_max, bw_max) ------------------------------------------------------------
def nnz_capacity_blocks(caps):
    """window_nnz_capacity / 36: the envelope of the band (windows of 65 .. 512 poses: of a band of at least 3)"""
    nv, bw = caps[0], caps[4]
    if 64 < nv <= 512 and bw < 3:
        bw = 3 if nv > 3 else nv - 1
    return sum(min(v, bw) + 1 for v in range(nv))


def mask_words(caps):
    return 1 if caps[0] <= 64 else 8


def table_bytes(caps):
    """window_tables(c).bytes on the SPARSE path"""
    nv, W = caps[0], mask_words(caps)
    words = 3 * nv * W + (W if W > 1 else 0)
    ints = nv + 4 * (nv + 1) + nv        # perm; boff, ioff, lvl_col, lvl_blk; colorder
    if W > 1:
        ints += nv * W + (nv + 1) + (nv + 2) + 2 * nv + 1      # rowpre, lvl_mode, dense_off, dense, one reserved
    else:
        ints += nnz_capacity_blocks(caps)                        # otask
    return 8 * words + 4 * ints


def index_doubles(caps):
    _, nr, npr, ns, _ = caps
    return sum((n + 1) // 2 for n in (2 * nr + npr + 2 * ns, nr + ns + 1, 2 * nr, npr, 4 * ns))


def recA_capacity(caps):
    return caps[0] + 2 * nnz_capacity_blocks(caps)


def lds_mode_bytes(caps):
    """window_layout(c, false).lds_bytes of a window of at most 64 poses: everything in LDS"""
    nv, nr, npr, ns, _ = caps
    nb = nnz_capacity_blocks(caps)
    p = 2 * 36 * nb + 4 * 6 * nv + 2 * 12 * nv + 16 * nr + 28 * npr + 90 * ns + index_doubles(caps)
    p += (table_bytes(caps) + 7) // 8 + 5 * nr + 18 * npr + 48 * ns
    pad = p & 1
    p += pad + 2 * recA_capacity(caps) + nb + 1 + (1 - pad)
    return 8 * p


def arrays_in_lds(caps):
    return caps[0] <= 64 and lds_mode_bytes(caps) <= WINDOW_MAX_LDS


def index_in_lds(caps):
    b = 8 * index_doubles(caps)
    if caps[0] <= 64:
        return b <= 16 * 1024
    return b <= 72 * 1024 and b + table_bytes(caps) + 1024 <= WINDOW_MAX_LDS


def root_lds_doubles(caps):
    """room for the root supernode's dense system (eight-word windows), or 0"""
    if not 64 < caps[0] <= 512:
        return 0
    need = (6 * ROOT_MAX + 1) * 6 * ROOT_MAX
    used = (table_bytes(caps) + 7) // 8 * 8 + (8 * index_doubles(caps) if index_in_lds(caps) else 0)
    return need if used + 8 * need <= WINDOW_WIDE_MAX_LDS else 0


# ---- the elimination ------------------------------------------------------------------------------------------------------------------
def _eliminate(nv, pairs, pick):
    """Rounds of independent poses: pick(remaining, adjacency) names a round's poses in index order; their remaining neighbours become
    cliques.  Returns (perm: pose -> position, col: per position the sorted positions below it in the factor, rounds as position lists)."""
    adj = [set() for _ in range(nv)]
    for u, v in pairs:
        adj[u].add(v); adj[v].add(u)
    for v in range(nv):
        adj[v].discard(v)
    rem, perm, struct, rounds = set(range(nv)), [None] * nv, {}, []
    while rem:
        S = pick(rem, adj)
        rounds.append(list(range(nv - len(rem), nv - len(rem) + len(S))))
        for r, v in enumerate(S):
            perm[v] = nv - len(rem) + r
            struct[v] = adj[v] & rem
        for u in rem - set(S):
            for v in adj[u] & set(S):
                adj[u] |= struct[v]
            adj[u].discard(u)
        rem -= set(S)
    col = [None] * nv
    for v in range(nv):
        col[perm[v]] = sorted(perm[u] for u in struct[v])
    return perm, col, rounds


def _pick_natural(rem, adj):
    return [min(rem)]


def _pick_small(rem, adj):
    """every pose of minimum degree that has no lower-numbered minimum-degree neighbour"""
    deg = {v: len(adj[v] & rem) for v in rem}
    cand = {v for v in rem if deg[v] == min(deg.values())}
    return sorted(v for v in cand if not any(u < v for u in adj[v] & cand))


def _pick_wide(rem, adj):
    """candidates: degree within 1 of the minimum; among adjacent candidates the one whose rank among the candidates (index order) has the
    fewer trailing zero bits goes first, then the lower rank"""
    deg = {v: len(adj[v] & rem) for v in rem}
    cand = sorted(v for v in rem if deg[v] <= min(deg.values()) + 1)
    prio = {v: ((((r & -r).bit_length() - 1) if r else 31), r) for r, v in enumerate(cand)}
    return [v for v in cand if not any(prio[u] < prio[v] for u in adj[v] & set(cand))]


def _rows(nv, col):
    row = [set() for _ in range(nv)]     # row[i]: the earlier columns K < i with a block (i, K)
    for K in range(nv):
        for i in col[K]:
            row[i].add(K)
    return row


def _common(row, i, J):
    """the earlier columns K < J that rows i and J share: the length of block (i, J)'s product sum"""
    return len({K for K in row[i] & row[J] if K < J}) if i != J else len(row[J])


def order_small(nv, pairs, natural=False, workspace=True, caps=None):
    """compute_sparse: windows of at most 64 poses.  workspace: the arrays live in the HBM workspace (columns are pushed); else in LDS, and
    with caps the stage-A records build_small_tables needs are counted against small_recA_capacity."""
    perm, col, _ = _eliminate(nv, pairs, _pick_natural if natural else _pick_small)
    row = _rows(nv, col)
    level = [0] * nv
    for i in range(nv):
        level[i] = max((level[K] + 1 for K in row[i]), default=0)
    levels = [[J for J in range(nv) if level[J] == l] for l in range(max(level, default=-1) + 1)]
    m = SimpleNamespace(perm=perm, col=col, row=row, nb=nv + sum(len(c) for c in col), level=level, levels=levels, modes=[], pushed=set())
    for cols in levels:
        multi = any(len(col[J]) > 1 for J in cols)
        m.modes.append("C" if not multi else ("W" if len(cols) >= WIDE_LEVEL else "R"))
        if m.modes[-1] != "R" and workspace:
            m.pushed |= {J for J in cols if len(col[J]) == 1}
    if not workspace:
        # two first records per column, one per off-diagonal block; a continuation record (two for a column: block and right-hand side) per
        # further earlier column of a product sum
        m.recA = nv + m.nb + sum(2 * max(0, len(row[J]) - 1) + sum(max(0, _common(row, i, J) - 1) for i in col[J]) for J in range(nv))
        m.recA_cap = None if caps is None else recA_capacity(caps)
        m.tables = None if caps is None else m.recA <= m.recA_cap
    return m


def order_wide(nv, pairs, natural=False, caps=None, solo=True):
    """compute_sparse_mw: windows of 65 .. 512 poses (capacity nv_max).  A round is a level.  solo: the launch runs eight waves per window
    (the set-up on one of them), where a wide level stays in row mode."""
    perm, col, rounds = _eliminate(nv, pairs, _pick_natural if natural else _pick_wide)
    row = _rows(nv, col)
    level = [None] * nv
    for l, cols in enumerate(rounds):
        for J in cols:
            level[J] = l
    m = SimpleNamespace(perm=perm, col=col, row=row, nb=nv + sum(len(c) for c in col), level=level, levels=rounds, modes=[], pushed=set())
    for cols in rounds:
        multi = any(len(col[J]) > 1 or len(row[J]) >= DENSE_K for J in cols)
        m.modes.append("C" if not multi else ("W" if not solo and len(cols) >= WIDE_LEVEL else "R"))
        if m.modes[-1] != "R":
            m.pushed |= {J for J in cols if len(col[J]) == 1}
    # the dense list: per column with at least DENSE_K earlier columns its diagonal block and its right-hand side, and every off-diagonal
    # block whose product sum is that long
    m.dense = sum(2 * (len(row[J]) >= DENSE_K) + sum(_common(row, i, J) >= DENSE_K for i in col[J]) for J in range(nv))
    m.dense_cap = None if caps is None else 2 * caps[0]
    m.dense_ok = None if caps is None else m.dense <= m.dense_cap
    # the root supernode: the trailing run of single-column levels whose column holds all later poses, at most ROOT_MAX of them, none with a
    # pushed child among the earlier columns
    nlev = len(rounds)
    run = 0                               # the run's length with no limit on it
    while run < nlev and len(rounds[nlev - 1 - run]) == 1 and len(col[rounds[nlev - 1 - run][0]]) == nv - 1 - rounds[nlev - 1 - run][0]:
        run += 1
    m.root_run = run
    m.root, m.root_level, m.root_refused = 0, nlev, None
    if caps is not None and (not root_lds_doubles(caps) or not m.dense_ok):
        m.root_refused = "no room" if m.dense_ok else "dense list overflowed"
    else:
        take = min(run, ROOT_MAX)
        jr = nv - take
        if take < 2:
            m.root_refused = "no clique"
        elif any(K < jr and K in m.pushed for a in range(jr, nv) for K in row[a]):
            m.root_refused = "pushed child"
        else:
            m.root, m.root_level = take, nlev - take
    return m


def result7(m):
    """result[7] of a window on the SPARSE path: levels * 65536 + blocks (+ poses in the root supernode / 16)"""
    return len(m.levels) * 65536 + m.nb + getattr(m, "root", 0) / 16.0


def model_for(nv, pairs, caps, natural=False):
    """the model of a window of nv poses in a handle of capacities caps, on the path the handle takes (None: the skyline path).  The
    natural order is also what the kernel falls back to when the minimum-degree fill exceeds the capacity."""
    if caps[0] > 512:
        return None
    nb_max = nnz_capacity_blocks(caps)
    for nat in ((True,) if natural else (False, True)):
        m = order_small(nv, pairs, nat, not arrays_in_lds(caps), caps) if caps[0] <= 64 else order_wide(nv, pairs, nat, caps)
        m.natural = nat
        if m.nb <= nb_max:
            break
    return m
