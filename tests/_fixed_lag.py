"""Test helper: translation-only chains for the marginal-prior tests (tests/test_marginal_prior_cpu.py on the oracle and numpy alone,
tests/test_gpu_marginal_prior.py on the GPU) and the fixed-lag smoother built from them: next_window builds the window after a slide from the
previous one and the prior row loc_window_marginal_prior_host (or tests/_dense_prior_ref.marginal_ref) returned for its oldest pose.

A chain: a random walk whose poses range 3 .. 5 of six surveyed anchors each (sigma 0.03 m) and are joined by zero-range smoothness edges
(sigma 0.3 m), as the node's windows are — with three or more anchors per pose, so that a pose's own factors determine it.

The one-drop and fixed-lag PROPERTIES (a window solved again after the drop stays where it was) hold at a converged solve: those tests run
PROPERTY_ITERATIONS LM iterations (g2o's damping policy needs far more than the node's ten on some of these windows: at 10 iterations the
kept poses of one window still move 3e-3 m by themselves, at 50 at most 3e-5 m)."""
import numpy as np

ANCH = np.array([[3, -3, 0.58], [3, 3, 1.97], [-3, 3, 0.54], [-3, -3, 1.76], [0.2, -3.5, 2.6], [-0.3, 3.5, 0.2]], dtype=float)
RANGE_INFO = 1.0 / 0.03 ** 2
SMOOTH_INFO = 1.0 / 0.3 ** 2
NA_MAX = 5
PROPERTY_ITERATIONS = 100


class Chain:
    """N poses of one trajectory: truth, initial estimates, the anchors every pose ranges and the measured ranges"""

    def __init__(self, seed, N, n_anch):
        rng = np.random.default_rng(seed)
        self.N = N
        self.truth = np.cumsum(rng.normal(0, 0.12, (N, 3)), axis=0) + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.1])
        self.est = self.truth + rng.normal(0, 0.05, (N, 3))
        self.which = []
        for _ in range(N):   # two or three neighbouring corner anchors and the high / the low one: never three along one wall
            c = int(rng.integers(4))
            w = [c, (c + 1) % 4, 4 + int(rng.integers(2))] if n_anch == 3 else [c, (c + 1) % 4, (c + 2) % 4, 4, 5][:n_anch]
            self.which.append(sorted(w))
        self.meas = [[float(np.float32(np.linalg.norm(self.truth[k] - ANCH[a]) + rng.normal(0, 0.03))) for a in self.which[k]] for k in range(N)]


def window_caps(W):
    """(nv_max, nr_max, np_max, ns_max) of a window of W poses: NA_MAX anchors per pose, two smoothness edges per pair, two priors per window"""
    return W, W * NA_MAX + 2 * (W - 1), 2, 0


def add_chain_poses(wb, i, ch, start, T, est=None, doubled=(), missing=(), keep_ranges=None):
    """poses start .. start + T - 1 of chain ch into window i: estimates (est [T][3], default ch.est), anchor ranges, smoothness edges
    (k - 1, k) — stored (k, k - 1) for odd k; doubled: pairs k that get a second one the other way round; missing: pairs k that get none;
    keep_ranges: {slot: n} keeps only the first n anchor ranges of that slot"""
    for s in range(T):
        wb.add_pose(i, ch.est[start + s] if est is None else est[s])
    for s in range(T):
        k = start + s
        n = len(ch.which[k]) if keep_ranges is None or s not in keep_ranges else keep_ranges[s]
        for a, d in list(zip(ch.which[k], ch.meas[k]))[:n]:
            wb.add_range(i, s, a, d, RANGE_INFO, anchor=True)
        if s and s not in missing:
            if s % 2: wb.add_range(i, s, s - 1, 0.0, SMOOTH_INFO)
            else: wb.add_range(i, s - 1, s, 0.0, SMOOTH_INFO)
            if s in doubled:
                if s % 2: wb.add_range(i, s - 1, s, 0.0, 0.5 * SMOOTH_INFO)
                else: wb.add_range(i, s, s - 1, 0.0, 0.5 * SMOOTH_INFO)


def add_prior_row(wb, i, slot, row):
    """a prior row of the marginal pass ([48]: Z^-1 as R(9), t(3), the 6 x 6 information) on pose `slot` of window i"""
    Ri = row[:9].reshape(3, 3)
    wb.add_prior(i, slot, -Ri.T @ row[9:12], Ri.T, info=row[12:].reshape(6, 6))


def first_window(la, chains, W):
    wb = la.WindowBatch(len(chains), *window_caps(W))
    for i, ch in enumerate(chains):
        add_chain_poses(wb, i, ch, 0, W)
    return wb


def next_window(la, prev, chains, start, W, slots=None, rows=None):
    """The windows of poses start .. start + W - 1 after the slide that dropped pose start - 1 (slot 0 of prev, the solved previous
    batch): the kept poses start from prev's estimates, the new pose from the chain's; rows [B][48] with slots [B]: the marginal prior
    of the dropped pose, on the pose it names (the new slot 0); None: the plain drop, everything the dropped pose's factors knew is gone."""
    wb = la.WindowBatch(len(chains), *window_caps(W))
    for i, ch in enumerate(chains):
        nv = int(prev.counts[i, 0])
        est = np.vstack([prev.poses[i, 1:nv, 9:12], ch.est[start + W - 1][None]])
        add_chain_poses(wb, i, ch, start, W, est=est)
        if rows is not None and slots[i] >= 0:
            assert slots[i] == 1   # the dropped pose's one neighbour: the next pose
            add_prior_row(wb, i, 0, rows[i])
    if rows is not None and wb.p_info is None:   # (no window carried a prior: the table still exists, as on every later slide)
        wb.p_info = np.zeros((wb.B, max(wb.caps[2], 1), 36))
    return wb


# ---- the inputs of the marginal-prior parity tests: name -> eight window specifications --------------------------------------------------------
def _spec(T=10, na=4, drop=0, **kw):
    return dict(T=T, na=na, drop=drop, **kw)


CASES = {
    "chain1": [_spec(T=1, na=3 + i % 3) for i in range(8)],
    "chain2": [_spec(T=2, na=3 + i % 3, drop=i % 2) for i in range(8)],
    "chain3": [_spec(T=3, na=3 + i % 3, drop=(0, 2)[i % 2]) for i in range(8)],
    "chain10": [_spec(na=3 + i % 3) for i in range(8)],
    "doubled": [_spec(na=3 + i % 3, doubled=(1,)) for i in range(8)],
    "missing": [_spec(na=3 + i % 3, missing=(1,) if i % 2 == 0 else ()) for i in range(8)],
    "zprior": [_spec(na=3 + i % 3, zprior=True) for i in range(8)],
    "fullprior": [_spec(na=3 + i % 3, fullprior=1 + i % 3, zprior=i % 2 == 1) for i in range(8)],
    "last": [_spec(na=3 + i % 3, drop=9, doubled=(9,) if i % 4 == 3 else ()) for i in range(8)],
    "ragged": [_spec(T=(10, 4, 7, 2, 9, 1, 6, 3)[i], na=3 + i % 3, drop=(0, 3, 0, 1, 8, 0, 0, 2)[i]) for i in range(8)],
    "one_range": [_spec(na=3 + i % 3, one_range=i in (2, 5)) for i in range(8)],
}
SEED = {name: 7100 + 10 * k for k, name in enumerate(CASES)}


def case_batch(la, name):
    """(batch, drop [8]) of a parity case.  zprior: a lidar-style z prior on the dropped pose; fullprior = r: a full-information prior of
    rank r on it (what an earlier slide leaves); one_range: the dropped pose keeps one anchor range and its smoothness edge — its own
    factors do not determine it."""
    specs = CASES[name]
    W = max(s["T"] for s in specs)
    wb = la.WindowBatch(len(specs), *window_caps(W))
    rng = np.random.default_rng(SEED[name] + 5)
    for i, s in enumerate(specs):
        ch = Chain(SEED[name] + i, s["T"], s["na"])
        d = s["drop"]
        add_chain_poses(wb, i, ch, 0, s["T"], doubled=s.get("doubled", ()), missing=s.get("missing", ()),
                        keep_ranges={d: 1} if s.get("one_range") else None)
        if s.get("zprior"):
            wb.add_prior(i, d, np.array([ch.est[d, 0], ch.est[d, 1], ch.truth[d, 2] + rng.normal(0, 0.02)]), np.eye(3), np.array([0, 0, 1 / 0.05, 0, 0, 0.0]))
        if s.get("fullprior"):
            A = rng.normal(size=(3, s["fullprior"]))
            info = np.zeros((6, 6)); info[:3, :3] = 40.0 * (A @ A.T)
            wb.add_prior(i, d, ch.truth[d] + rng.normal(0, 0.05, 3), np.eye(3), info=info)
    return wb, np.array([s["drop"] for s in specs], dtype=np.int32)
