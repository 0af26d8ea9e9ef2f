"""Test helper: a batch of windows as plain numpy tables, and an independent restatement of what localization_amd/csrc/window_structure.cpp
promises about it, written from the comments of window_structure.h / .cpp and window_kernel.h (the table layouts, "Layout of one
instance", ArrowAux, TreeSched).  Verdict models return values; the two table builders are CHECKED (the tables are read back the way the
kernels read them and compared with the input graph), since more than one correct schedule exists."""
import numpy as np

I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
TABLES = ("poses", "counts", "r_val", "p_val", "s_val", "r_idx", "p_idx", "s_idx")   # window_tables.h: WindowTable order
ARROW_MAX_ANCHORS = 256          # window_kernel.h: kArrowMaxAnchors
ARROW_LDS_LIMIT = 160 * 1024 - 512


class Batch:
    """n instances in the C ABI's layout.  Every slot starts POISONED (INT32_MIN / INT32_MAX / NaN): what the add_* calls do not
    fill is an unused slot, and a pass that reads one changes its verdict or trips a sanitizer."""

    def __init__(self, n, nv_max, nr_max, np_max, ns_max, bw_max, n_anchors=0, has_off1=False):
        self.n, self.caps, self.n_anchors, self.has_off1 = n, (nv_max, nr_max, np_max, ns_max, bw_max), n_anchors, has_off1
        self.poses = np.full((n, nv_max, 12), np.nan)
        self.counts = np.zeros((n, 4), np.int32)
        self.r_val = np.full((n, nr_max, 5), np.nan)
        self.p_val = np.full((n, np_max, 18), np.nan)
        self.s_val = np.full((n, ns_max, 48), np.nan)
        self.r_idx = np.full((n, nr_max, 2), I32_MIN, np.int32)
        self.p_idx = np.full((n, np_max), I32_MAX, np.int32)
        self.s_idx = np.full((n, ns_max, 4), I32_MIN, np.int32)
        self.s_idx[:, :, 1::2] = I32_MAX

    def copy(self, *deep):
        """A batch that shares every table with this one except the named ones."""
        out = Batch.__new__(Batch)
        out.__dict__.update(self.__dict__)
        for name in deep:
            setattr(out, name, getattr(self, name).copy())
        return out

    def with_caps(self, **kw):
        out = self.copy()
        names = ("nv_max", "nr_max", "np_max", "ns_max", "bw_max")
        out.caps = tuple(kw.get(k, v) for k, v in zip(names, self.caps))
        return out

    def add_pose(self, i, t=(0.0, 0.0, 0.0), R=None):
        k = self.counts[i, 0]
        self.poses[i, k, :9] = np.eye(3).reshape(9) if R is None else np.asarray(R).reshape(9)
        self.poses[i, k, 9:] = t
        self.counts[i, 0] = k + 1
        return int(k)

    def add_range(self, i, v0, v1, meas=1.0, info=1.0, lever=(0.0, 0.0, 0.0)):
        e = self.counts[i, 1]
        self.r_idx[i, e] = (v0, v1)
        self.r_val[i, e] = (meas, info) + tuple(lever)
        self.counts[i, 1] = e + 1
        return int(e)

    def add_prior(self, i, v, t=(0.0, 0.0, 0.0), info=(1.0, 1.0, 1.0, 0.0, 0.0, 0.0), R=None):
        e = self.counts[i, 2]
        self.p_idx[i, e] = v
        self.p_val[i, e, :9] = np.eye(3).reshape(9) if R is None else np.asarray(R).reshape(9)
        self.p_val[i, e, 9:12] = t
        self.p_val[i, e, 12:] = info
        self.counts[i, 2] = e + 1
        return int(e)

    def add_se3(self, i, vi, vj, robust=0):
        e = self.counts[i, 3]
        self.s_idx[i, e] = (vi, vj, robust, 0)
        self.s_val[i, e] = 0.0
        self.s_val[i, e, 0:9:4] = 1.0
        self.s_val[i, e, 12::7] = 1.0
        self.counts[i, 3] = e + 1
        return int(e)

    def write(self, f):
        np.array(self.caps + (self.n_anchors, int(self.has_off1), 0), np.int32).tofile(f)
        np.array([self.n], np.int64).tofile(f)
        nv, nr, npr, ns, _ = self.caps
        shapes = {"poses": (nv, 12), "counts": (4,), "r_val": (nr, 5), "p_val": (npr, 18), "s_val": (ns, 48), "r_idx": (nr, 2), "p_idx": (npr,), "s_idx": (ns, 4)}
        for name in TABLES:
            a = getattr(self, name)
            assert a.shape == (self.n,) + shapes[name], (name, a.shape)     # (with_caps changes what the passes are TOLD, never the tables)
            np.ascontiguousarray(a).tofile(f)


def read_sections(path):
    """The driver's output: one dict of arrays per batch."""
    types = {0: np.int32, 1: np.float64, 2: np.int64}
    out = []
    with open(path, "rb") as f:
        raw = f.read()
    at = 0
    while at < len(raw):
        name = raw[at:at + 16].split(b"\0")[0].decode()
        typ = int(np.frombuffer(raw, np.int32, 1, at + 16)[0])
        cnt = int(np.frombuffer(raw, np.int64, 1, at + 20)[0])
        data = np.frombuffer(raw, types[typ], cnt, at + 28)
        at += 28 + data.nbytes
        if name == "batch":
            out.append({})
        out[-1][name] = data
    return out


def thread_ranges(n, hw):
    """The instance ranges of the threaded passes: one range below 4 096 instances, else min(8, hardware threads) equal ranges."""
    nt = min(8, max(hw, 1)) if n >= 4096 else 1
    per = -(-n // nt)
    return [(min(n, t * per), min(n, (t + 1) * per)) for t in range(nt)]


# ---- verdicts -------------------------------------------------------------------------------------------------------------------

def first_failed_check(b, i):
    """check_instances' code for instance i alone: counts, then every range edge in turn (index, then distance), priors, SE3 edges."""
    nv_max, nr_max, np_max, ns_max, bw = b.caps
    nv, nr, npr, ns = (int(x) for x in b.counts[i])
    if not (0 <= nv <= nv_max and 0 <= nr <= nr_max and 0 <= npr <= np_max and 0 <= ns <= ns_max):
        return 1
    for v0, v1 in b.r_idx[i, :nr].tolist():
        if not 0 <= v0 < nv or not -b.n_anchors <= v1 < nv or v0 == v1:
            return 2
        if v1 >= 0 and abs(v0 - v1) > bw:
            return 3
    for v in b.p_idx[i, :npr].tolist():
        if not 0 <= v < nv:
            return 4
    for vi, vj, _, _ in b.s_idx[i, :ns].tolist():
        if not 0 <= vi < nv or not 0 <= vj < nv or vi == vj:
            return 5
        if abs(vi - vj) > bw:
            return 6
    return 0


def translation_only(b):
    if b.n_anchors > 500000:
        return False
    eye = np.eye(3).reshape(9)
    for i in range(b.n):
        nv, nr, npr, ns = (int(x) for x in b.counts[i])
        if ns or nv > 1048575:
            return False
        if np.any(b.r_val[i, :nr, 2:5] != 0.0) or np.any(b.poses[i, :nv, :9] != eye):
            return False
        if np.any(b.p_val[i, :npr, :9] != eye) or np.any(b.p_val[i, :npr, 15:18] != 0.0):
            return False
    return True


def chain_scan(b, ordered):
    """(chain, single_pairs, se3_pairs); the pair verdicts are defined for chain batches in edge order only."""
    chain, dup_r, dup_s, any_s = True, False, False, False
    for i in range(b.n):
        nv, nr, npr, ns = (int(x) for x in b.counts[i])
        rr = b.r_idx[i, :nr].tolist()
        ss = [x[:2] for x in b.s_idx[i, :ns].tolist()]
        any_s = any_s or ns > 0
        pose_pairs_r = [(min(p), max(p)) for p in rr if p[1] >= 0]
        pose_pairs_s = [(min(p), max(p)) for p in ss]
        if any(hi - lo != 1 for lo, hi in pose_pairs_r + pose_pairs_s):
            chain = False
        if ordered:
            keys_r = [max(p) for p in rr]                    # (a range to an anchor sorts by its pose)
            keys_s = [max(p) for p in ss]
            pri = b.p_idx[i, :npr].tolist()
            if keys_r != sorted(keys_r) or keys_s != sorted(keys_s) or pri != sorted(pri):
                chain = False
        dup_r = dup_r or len(set(pose_pairs_r)) != len(pose_pairs_r)
        dup_s = dup_s or len(set(pose_pairs_s)) != len(pose_pairs_s)
    return chain, (not any_s and not dup_r), (any_s and not dup_r and not dup_s)


def envelope_blocks_max(b):
    nv_max, nr_max, _, ns_max, _ = b.caps
    most = 0
    for i in range(b.n):
        nv, nr, _, ns = (int(x) for x in b.counts[i])
        if not (0 <= nv <= nv_max and 0 <= nr <= nr_max and 0 <= ns <= ns_max):
            return -1
        first = list(range(nv))
        for v0, v1 in b.r_idx[i, :nr].tolist() + [x[:2] for x in b.s_idx[i, :ns].tolist()]:
            if not 0 <= v0 < nv or v1 >= nv:
                return -1
            if v1 >= 0:
                first[max(v0, v1)] = min(first[max(v0, v1)], v0, v1)
        for _, v1 in [x[:2] for x in b.s_idx[i, :ns].tolist()]:
            if v1 < 0:
                return -1
        most = max(most, sum(v - first[v] + 1 for v in range(nv)))
    return most


# ---- arrowhead windows ----------------------------------------------------------------------------------------------------------

def arrow3_lds_bytes(nv_max, nb_max):
    """window_layouts.h: arrow3_lds_layout (four waves, an anchor table of 256 entries), in bytes."""
    D = 3 * nb_max
    D16 = 16 * ((D + 15) // 16)
    return 8 * (nv_max * 28 + D * (D + 1) // 2 + (D + 1) * (D + 2) // 2 + 3 * D + 4 * D + 4 * 4 * D16 * 3 + 6 * nb_max + 16 + 3 * ARROW_MAX_ANCHORS)


def arrow_border(b, i):
    """nb0: the smallest number of last slots that holds an endpoint of every pose-to-pose edge between non-consecutive slots."""
    nv, nr = int(b.counts[i, 0]), int(b.counts[i, 1])
    return max([nv - max(v0, v1) for v0, v1 in b.r_idx[i, :nr].tolist() if v1 >= 0 and abs(v0 - v1) != 1], default=0)


def arrow_nseg(n0):
    return min(max(n0 // 24, 1), 4)


def check_arrow_tables(b, out):
    """Reads hdr / rslot / rec / prec of an accepted batch as arrow3_lm_kernel does and compares them with the batch; returns the
    maxima (nb_max, jmax, jpmax, jch[16], jpch[16], list_cap) the batch implies."""
    nv_max = b.caps[0]
    nchunk = (nv_max + 63) // 64
    sizes = out["arrow"]
    assert sizes[0] == 1
    jmax, jpmax = int(sizes[3]), int(sizes[4])
    hdr = out["ahdr"].reshape(b.n, 8)
    rslot = out["arslot"].reshape(b.n, nv_max)
    rec = out["arec"].reshape(b.n, nchunk, jmax, 64, 3)
    prec = out["aprec"].reshape(b.n, nchunk, jpmax, 64, 7)
    m_nb, m_j, m_jp, m_list = 0, 1, 1, 1
    m_jch, m_jpch = [1] * 16, [1] * 16
    for i in range(b.n):
        nv, nr, npr, _ = (int(x) for x in b.counts[i])
        nb0 = arrow_border(b, i)
        n0 = nv - nb0
        nseg = arrow_nseg(n0)
        nb, nc = nb0 + nseg - 1, n0 - (nseg - 1)
        assert hdr[i, :3].tolist() == [nb, nseg, nc], (i, hdr[i], nb, nseg, nc)
        seg = hdr[i, 3:8].tolist()
        assert seg[0] == 0 and all(seg[s] <= seg[s + 1] for s in range(4)) and all(x == nc for x in seg[nseg:]), (i, seg)
        assert all(seg[s] < seg[s + 1] for s in range(nseg)), (i, seg)                   # no empty segment among the nseg
        # one wave sweeps each segment, so the cut is an even one: separator k at k / nseg of the chain.  The lengths then differ by the
        # rounding (1) and by the separator the first segment does not have in front of it (1)
        lens = [seg[s + 1] - seg[s] for s in range(nseg)]
        assert max(lens) - min(lens) <= 2, (i, lens)
        rows = rslot[i, :nc + nb].tolist()
        assert sorted(rows) == list(range(nv)), (i, rows)
        seps, border = rows[nc:nc + nseg - 1], rows[nc + nseg - 1:]
        assert border == list(range(n0, nv)), (i, border)
        assert seps == sorted(seps) and all(0 < s < n0 - 1 for s in seps), (i, seps)
        assert rows[:nc] == [v for v in range(n0) if v not in seps], (i, "chain rows in slot order")
        for s in range(1, nseg):                                                          # segment s starts right after separator s - 1
            assert rows[seg[s]] == seps[s - 1] + 1 and rows[seg[s] - 1] == seps[s - 1] - 1, (i, s, seg, seps)
        row_of = {v: r for r, v in enumerate(rows)}
        want = [[] for _ in rows]
        pair_seen = set()
        for (v0, v1), (meas, info) in zip(b.r_idx[i, :nr].tolist(), b.r_val[i, :nr, :2].tolist()):
            if v1 < 0:
                row, kind, idx, own0 = row_of[v0], 0, -1 - v1, 1
            else:
                r0, r1 = row_of[v0], row_of[v1]
                if r0 < nc and r1 < nc:                     # chain to chain: the previous chain row, which must be the previous SLOT too
                    assert abs(v0 - v1) == 1 and abs(r0 - r1) == 1 and (min(v0, v1), max(v0, v1)) not in pair_seen, (i, v0, v1)
                    pair_seen.add((min(v0, v1), max(v0, v1)))
                    row, kind, idx, own0 = max(r0, r1), 1, 0, int(r0 > r1)
                elif r0 < nc or r1 < nc:                    # chain to border: the chain row owns it
                    row, kind, idx, own0 = min(r0, r1), 2, max(r0, r1) - nc, int(r0 < r1)
                else:                                       # border to border: the higher border row owns it
                    row, kind, idx, own0 = max(r0, r1), 2, min(r0, r1) - nc, int(r0 > r1)
            want[row].append(((idx << 3) | (kind << 1) | own0, meas, info))
        code_want = np.full((nchunk, jmax, 64), -1.0)
        for r, lst in enumerate(want):
            for j, (code, meas, info) in enumerate(lst):
                assert j < jmax, (i, r, len(lst), jmax)
                code_want[r // 64, j, r % 64] = code
                assert rec[i, r // 64, j, r % 64].tolist() == [code, meas, info], (i, r, j, rec[i, r // 64, j, r % 64], code, meas, info)
        assert np.array_equal(rec[i, :, :, :, 0], code_want), (i, "a record nobody owns, or a used slot without its code")
        pwant = [[] for _ in rows]
        for v, val in zip(b.p_idx[i, :npr].tolist(), b.p_val[i, :npr].tolist()):
            pwant[row_of[v]].append(val[9:15])
        flag_want = np.zeros((nchunk, jpmax, 64))
        for r, lst in enumerate(pwant):
            for j, six in enumerate(lst):
                assert j < jpmax, (i, r, len(lst), jpmax)
                flag_want[r // 64, j, r % 64] = 1.0
                assert prec[i, r // 64, j, r % 64, 1:].tolist() == six, (i, r, j)
        assert np.array_equal(prec[i, :, :, :, 0] > 0, flag_want > 0), (i, "prior flags")
        deg = [0] * nv
        for v0, v1 in b.r_idx[i, :nr].tolist():
            deg[v0] += 1
            if v1 >= 0:
                deg[v1] += 1
        for v in b.p_idx[i, :npr].tolist():
            deg[v] += 1
        m_list = max([m_list] + deg[:n0])
        m_nb = max(m_nb, nb)
        for r in range(len(rows)):
            m_j, m_jp = max(m_j, len(want[r])), max(m_jp, len(pwant[r]))
            if r // 64 < 16:
                m_jch[r // 64] = max(m_jch[r // 64], len(want[r]))
                m_jpch[r // 64] = max(m_jpch[r // 64], len(pwant[r]))
    return m_nb, m_j, m_jp, m_jch, m_jpch, m_list


# ---- forest windows of one topology ---------------------------------------------------------------------------------------------

def _components_and_diameters(nv, pairs):
    adj = [set() for _ in range(nv)]
    for u, v in pairs:
        adj[u].add(v); adj[v].add(u)

    def bfs(s):
        dist = {s: 0}
        q = [s]
        for v in q:
            for x in adj[v]:
                if x not in dist:
                    dist[x] = dist[v] + 1
                    q.append(x)
        return dist
    comp, diam = {}, {}
    for v in range(nv):
        if v in comp:
            continue
        d = bfs(v)
        far = max(d, key=d.get)
        d2 = bfs(far)
        for x in d:
            comp[x] = v
        diam[v] = max(d2.values())
    return comp, diam


def is_forest(nv, pairs):
    uf = list(range(nv))

    def find(v):
        while uf[v] != v:
            v = uf[v]
        return v
    for u, v in set((min(p), max(p)) for p in pairs):
        a, c = find(u), find(v)
        if a == c:
            return False
        uf[a] = c
    return True


def check_tree_sched(b, out):
    """Walks h_tsched section by section, checks that bind_tree_sched (window_structure.cpp) puts TreeSched's pointers at those sections
    and that the last one ends where the table ends, and checks every list against instance 0's graph."""
    sizes = [int(x) for x in out["tree_sizes"]]
    nv, nr, npr, ns, depth, nroots, nlev, max_s, nu, max_r = sizes
    assert [nv, nr, npr, ns] == b.counts[0].tolist()
    t = out["tsched"].tolist()
    at = [0]

    starts = []

    def take(k):
        assert at[0] + k <= len(t), "the schedule is shorter than its pointer walk"
        starts.append(at[0])
        at[0] += k
        return t[at[0] - k:at[0]]
    node, par = take(nv), take(nv)
    r_off, r_list = take(nv + 1), take(nr)
    p_off, p_list = take(nv + 1), take(npr)
    s_off, s_list = take(nv + 1), take(ns)
    r_idx, s_idx = take(2 * nr), take(4 * ns)
    w_par, w_height = take(nv), take(nv)
    w_koff, w_klist = take(nv + 1), take(nv - nroots)
    w_roff, w_rlist = take(nv + 1), take(nr)
    w_poff, w_plist = take(nv + 1), take(npr)
    w_soff, w_slist = take(nv + 1), take(ns)
    w_kleaf, w_ulist, w_kpos = take(nv), take(nu), take(nv)
    assert at[0] == len(t), (at[0], len(t))
    bind = [int(x) for x in out["tsched_bind"]]
    assert len(starts) == 23 and bind[:-1] == starts, (bind, starts)      # TreeSched's pointers in its declaration order = the sections' order
    assert bind[-1] == len(t) == starts[-1] + nv                          # the last section, w_kpos, ends at the end of the table
    redges = b.r_idx[0, :nr].tolist()
    sedges = [x[:2] for x in b.s_idx[0, :ns].tolist()]
    prior = b.p_idx[0, :npr].tolist()
    assert r_idx == [x for e in redges for x in e] and s_idx == b.s_idx[0, :ns].reshape(-1).tolist()
    pairs = [tuple(e) for e in redges if e[1] >= 0] + [tuple(e) for e in sedges]
    pairset = set((min(p), max(p)) for p in pairs)
    # the order
    assert sorted(node) == list(range(nv))
    assert all(p == -1 or k < p < nv for k, p in enumerate(par)), par
    pos = {v: k for k, v in enumerate(node)}
    parent = {node[k]: (-1 if par[k] < 0 else node[par[k]]) for k in range(nv)}
    for v, p in parent.items():                           # a parent is a neighbour; with nv - nroots such pairs, all distinct, every pair is used
        assert p == -1 or (min(v, p), max(v, p)) in pairset, (v, p)
    comp, diam = _components_and_diameters(nv, pairs)
    roots = [v for v in range(nv) if parent[v] == -1]
    assert len(roots) == nroots == len(diam) and len(set(comp[v] for v in roots)) == nroots
    assert len(pairset) == nv - nroots

    def lists(off, lst, count):
        assert off[0] == 0 and off[-1] == count and all(off[k] <= off[k + 1] for k in range(nv)), off
        assert sorted(lst) == list(range(count)), lst     # every edge exactly once
        return [lst[off[k]:off[k + 1]] for k in range(nv)]

    def child_end(v0, v1):                                # the endpoint that is the child of the pair
        assert parent[v0] == v1 or parent[v1] == v0, (v0, v1)
        return v0 if parent[v0] == v1 else v1
    r_by, p_by, s_by = lists(r_off, r_list, nr), lists(p_off, p_list, npr), lists(s_off, s_list, ns)
    for k in range(nv):
        for e in r_by[k]:
            v0, v1 = redges[e]
            assert node[k] == (v0 if v1 < 0 else child_end(v0, v1)), (k, e)
        for e in p_by[k]:
            assert node[k] == prior[e], (k, e)
        for e in s_by[k]:
            assert node[k] == child_end(*sedges[e]), (k, e)
    assert max_r == max(len(x) for x in r_by) and max_s == max(len(x) for x in s_by)
    # the same by pose slot
    assert w_par == [parent[v] for v in range(nv)]
    assert w_koff[0] == 0 and w_koff[-1] == nv - nroots and all(w_koff[v] <= w_koff[v + 1] for v in range(nv)), w_koff
    kids = [w_klist[w_koff[v]:w_koff[v + 1]] for v in range(nv)]
    height = {}
    for k in range(nv):                                   # children come before their parent in `node`
        v = node[k]
        assert sorted(kids[v]) == sorted(c for c in range(nv) if parent[c] == v), (v, kids[v])
        height[v] = 1 + max(height[c] for c in kids[v]) if kids[v] else 0
    assert w_height == [height[v] for v in range(nv)]
    for v in range(nv):
        nleaf = sum(1 for c in kids[v] if height[c] == 0)
        assert w_kleaf[v] == nleaf and all(height[c] == 0 for c in kids[v][:nleaf]) and all(height[c] > 0 for c in kids[v][nleaf:]), (v, kids[v])
    for off, lst, by, count in ((w_roff, w_rlist, r_by, nr), (w_poff, w_plist, p_by, npr), (w_soff, w_slist, s_by, ns)):
        w_by = lists(off, lst, count)
        assert all(sorted(w_by[v]) == sorted(by[pos[v]]) for v in range(nv))
    assert sorted(w_ulist) == sorted(v for v in range(nv) if height[v] >= 1) and nu == len(w_ulist)
    assert all(height[w_ulist[k]] >= height[w_ulist[k + 1]] for k in range(nu - 1)), [height[v] for v in w_ulist]
    assert all(w_kpos[c] == j for j, c in enumerate(w_klist)), (w_kpos, w_klist)
    assert sorted(w_kpos[v] for v in roots) == list(range(nv - nroots, nv))
    assert nlev == max(height.values()) + 1
    dep = {}
    for k in reversed(range(nv)):
        dep[node[k]] = 0 if parent[node[k]] < 0 else dep[parent[node[k]]] + 1
    assert depth == max(dep.values()) + 1
    for v in roots:
        assert height[v] == (diam[comp[v]] + 1) // 2, (v, height[v], diam[comp[v]])
