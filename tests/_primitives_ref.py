"""References for the device primitives of the 6-DoF kernels (tools/primitives_probe.hip, tests/test_gpu_device_primitives.py), written
from the definitions and not from the device code:

  Eigen::Quaternion(Matrix3) (the index form i / j / k of Eigen's quat_product / quaternionbase_assign_impl), Eigen's toRotationMatrix,
  g2o's internal::normalize, toVectorMQT / fromVectorMQT, e = toVectorMQT(Z^-1 Xi^-1 Xj) (EdgeSE3), e = toVectorMQT(Z^-1 X)
  (EdgeSE3Prior), the Cauchy kernel rho = log(1 + chi), rho' = 1 / (1 + chi).

Every definition is stated ONCE, over a number type: evaluated with mpmath at 50 digits it is the reference; evaluated with Python
floats (IEEE float64, one rounding per operation, no FMA) it is the plain float64 evaluation whose own distance from the reference
sets the tolerance the device is held to.  The Jacobians of the reference are 50-digit central differences of the error over the MQT
increment (X <- X * fromVectorMQT(v), step 1e-20); the float64 evaluation has to take the analytic derivative (J_ANALYTIC), which
tests/test_primitives_ref_cpu.py also holds to the central differences at 50 digits."""
import math

import mpmath
import numpy as np

DPS = 50
STEP = mpmath.mpf(10) ** -20


class F64:
    """IEEE float64, one rounding per operation"""
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    log = staticmethod(math.log)


class MP:
    """mpmath at the working precision (callers hold mpmath.workdps(DPS))"""
    num = staticmethod(mpmath.mpf)
    sqrt = staticmethod(mpmath.sqrt)
    log = staticmethod(mpmath.log)


def _mat(C, R):
    return [[C.num(R[3 * i + j]) for j in range(3)] for i in range(3)]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def branch_of(R):
    """which branch Eigen::Quaternion(Matrix3) takes for the row-major 3x3 R: 0 = trace > 0, 1 + i = the largest diagonal entry i"""
    R = [float(x) for x in R]
    if R[0] + R[4] + R[8] > 0:
        return 0
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    return 1 + i


def mat_to_quat(C, R):
    """Eigen::Quaternion(Matrix3): (w, x, y, z) of the 3x3 list-of-lists R"""
    t = R[0][0] + R[1][1] + R[2][2]
    q = [None] * 4
    if t > 0:
        t = C.sqrt(t + 1)
        q[0] = t / 2
        t = C.num(0.5) / t
        q[1] = (R[2][1] - R[1][2]) * t
        q[2] = (R[0][2] - R[2][0]) * t
        q[3] = (R[1][0] - R[0][1]) * t
        return q
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = C.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    q[1 + i] = t / 2
    t = C.num(0.5) / t
    q[0] = (R[k][j] - R[j][k]) * t
    q[1 + j] = (R[j][i] + R[i][j]) * t
    q[1 + k] = (R[k][i] + R[i][k]) * t
    return q


def quat_normalize_sign(C, q):
    """g2o internal::normalize: w < 0 flips the sign, then unit norm; returns (q, the sign applied)"""
    n = C.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    sg = -1 if q[0] < 0 else 1
    return [sg * x / n for x in q], sg


def quat_mul(C, a, b):
    """the Hamilton product, (w, x, y, z)"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def quat_to_mat(C, q):
    """Eigen toRotationMatrix (no normalisation)"""
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def quat_right_jac(C, q, sgn):
    """d vec(q (x) (sqrt(1 - |v|^2), v)) / dv at v = 0, for sgn * q: w I + [q_xyz]x"""
    w, x, y, z = [sgn * c for c in q]
    return [[w, -z, y], [z, w, -x], [-y, x, w]]


def to_vector_mqt(C, R, t):
    q, _ = quat_normalize_sign(C, mat_to_quat(C, R))
    return [t[0], t[1], t[2], q[1], q[2], q[3]]


def from_vector_mqt(C, v):
    w = 1 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5])
    R = quat_to_mat(C, [C.sqrt(w), v[3], v[4], v[5]]) if w >= 0 else [[C.num(i == j) for j in range(3)] for i in range(3)]
    return R, [v[0], v[1], v[2]]


def _oplus(C, R, t, v):
    Rv, tv = from_vector_mqt(C, v)
    p = _mv(R, tv)
    return _mm(R, Rv), [t[0] + p[0], t[1] + p[1], t[2] + p[2]]


def se3_error(C, Ri, ti, Rj, tj, Rz, tz):
    """e = toVectorMQT(Zinv * Xi^-1 * Xj) with Zinv = (Rz, tz) the INVERSE measurement (what the device's record holds) and
    X^-1 = (R^T, -R^T t)"""
    RiT = _tr(Ri)
    RB = _mm(RiT, Rj)
    tB = _mv(RiT, [tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]])
    RE = _mm(Rz, RB)
    p = _mv(Rz, tB)
    return to_vector_mqt(C, RE, [p[0] + tz[0], p[1] + tz[1], p[2] + tz[2]])


def prior_error(C, R, t, Rz, tz):
    """e = toVectorMQT(Zinv * X)"""
    p = _mv(Rz, t)
    return to_vector_mqt(C, _mm(Rz, R), [p[0] + tz[0], p[1] + tz[1], p[2] + tz[2]])


def _central(err_at):
    """6x6 Jacobian (rows: error, columns: increment) by 50-digit central differences with step 1e-20"""
    cols = []
    for d in range(6):
        vp = [mpmath.mpf(0)] * 6
        vm = [mpmath.mpf(0)] * 6
        vp[d] = STEP
        vm[d] = -STEP
        ep, em = err_at(vp), err_at(vm)
        cols.append([(a - b) / (2 * STEP) for a, b in zip(ep, em)])
    return [[cols[c][r] for c in range(6)] for r in range(6)]


def se3_jacobians_central(Ri, ti, Rj, tj, Rz, tz):
    C = MP

    def at_i(v):
        R, t = _oplus(C, Ri, ti, v)
        return se3_error(C, R, t, Rj, tj, Rz, tz)

    def at_j(v):
        R, t = _oplus(C, Rj, tj, v)
        return se3_error(C, Ri, ti, R, t, Rz, tz)
    return _central(at_i), _central(at_j)


def prior_jacobian_central(R, t, Rz, tz):
    def at(v):
        R2, t2 = _oplus(MP, R, t, v)
        return prior_error(MP, R2, t2, Rz, tz)
    return _central(at)


def _zeros6(C):
    return [[C.num(0)] * 6 for _ in range(6)]


def se3_jacobians_analytic(C, Ri, ti, Rj, tj, Rz, tz):
    """The derivative of e over the increments, taken by hand from the definitions (exact for orthonormal inputs):
      translation rows: tE = Rz Ri^T (tj - ti) + tz; Xi's increment (a, v) moves ti by Ri a and Ri by (I + 2 [v]x): d tE = -Rz a +
        2 Rz [tB]x v; Xj's moves tj by Rj a: d tE = RE a.
      rotation rows: the error quaternion is qZ (x) conj(qv) (x) qB for Xi's increment (qv = (sqrt(1 - |v|^2), v)): d / dv_k =
        -(qZ (x) e_k (x) qB), in the sign that makes w >= 0 and over the product's norm; qE (x) qv for Xj's: w I + [qE_xyz]x."""
    RiT = _tr(Ri)
    RB = _mm(RiT, Rj)
    tB = _mv(RiT, [tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]])
    RE = _mm(Rz, RB)
    qE, _ = quat_normalize_sign(C, mat_to_quat(C, RE))
    J0, J1 = _zeros6(C), _zeros6(C)
    S = [[0, -tB[2], tB[1]], [tB[2], 0, -tB[0]], [-tB[1], tB[0], 0]]
    RS = _mm(Rz, S)
    Q = quat_right_jac(C, qE, 1)
    qA, qB = mat_to_quat(C, Rz), mat_to_quat(C, RB)
    qAB = quat_mul(C, qA, qB)
    n = C.sqrt(sum(x * x for x in qAB))
    sg = -1 if qAB[0] < 0 else 1
    for i in range(3):
        for j in range(3):
            J0[i][j] = -Rz[i][j]
            J0[i][3 + j] = 2 * RS[i][j]
            J1[i][j] = RE[i][j]
            J1[3 + i][3 + j] = Q[i][j]
    for k in range(3):
        ek = [C.num(0)] * 4
        ek[1 + k] = C.num(1)
        r = quat_mul(C, quat_mul(C, qA, ek), qB)
        for i in range(3):
            J0[3 + i][3 + k] = -sg * r[1 + i] / n
    return J0, J1


def prior_jacobian_analytic(C, R, t, Rz, tz):
    RE = _mm(Rz, R)
    q, _ = quat_normalize_sign(C, mat_to_quat(C, RE))
    Q = quat_right_jac(C, q, 1)
    J = _zeros6(C)
    for i in range(3):
        for j in range(3):
            J[i][j] = RE[i][j]
            J[3 + i][3 + j] = Q[i][j]
    return J


def _jtwj(A, W, B):
    """A^T W B, 6x6"""
    WB = [[sum(W[i][k] * B[k][c] for k in range(6)) for c in range(6)] for i in range(6)]
    return [[sum(A[i][r] * WB[i][c] for i in range(6)) for c in range(6)] for r in range(6)]


def _lower(H, n=6):
    return [H[r][c] for r in range(n) for c in range(r + 1)]


def se3_terms(C, e, J0, J1, W, robust, j_is_later):
    """what chain_se3_terms hands out, from the error and Jacobians: chi, rterm, Hii (21), Hjj (21), Hoff (36: the block with the rows
    of the LATER pose, column-major), bi (6), bj (6)"""
    We = [sum(W[i][j] * e[j] for j in range(6)) for i in range(6)]
    chi = sum(e[i] * We[i] for i in range(6))
    rterm = C.log(1 + chi) if robust else chi
    w = 1 / (1 + chi) if robust else C.num(1)
    Hii = [w * x for x in _lower(_jtwj(J0, W, J0))]
    Hjj = [w * x for x in _lower(_jtwj(J1, W, J1))]
    Ho = _jtwj(J1, W, J0) if j_is_later else _jtwj(J0, W, J1)
    Hoff = [w * Ho[r][c] for c in range(6) for r in range(6)]
    bi = [-w * sum(J0[i][r] * We[i] for i in range(6)) for r in range(6)]
    bj = [-w * sum(J1[i][r] * We[i] for i in range(6)) for r in range(6)]
    return [chi, rterm] + Hii + Hjj + Hoff + bi + bj


SE3_SLICES = {"chi": slice(0, 1), "rterm": slice(1, 2), "Hii": slice(2, 23), "Hjj": slice(23, 44), "Hoff": slice(44, 80),
              "bi": slice(80, 86), "bj": slice(86, 92)}


def _pose(C, X):
    return _mat(C, X[:9]), [C.num(x) for x in X[9:12]]


def se3_row_linearization(row):
    """the 50-digit error and central-difference Jacobians of one probe row (Xi 12, Xj 12, Zinv 12, ...): flag-independent, so
    computed once per base row"""
    with mpmath.workdps(DPS):
        (Ri, ti), (Rj, tj), (Rz, tz) = _pose(MP, row[0:12]), _pose(MP, row[12:24]), _pose(MP, row[24:36])
        e = se3_error(MP, Ri, ti, Rj, tj, Rz, tz)
        J0, J1 = se3_jacobians_central(Ri, ti, Rj, tj, Rz, tz)
        return e, J0, J1


def se3_row_reference(row, lin=None):
    """all 92 outputs of a probe row at 50 digits, as mpf"""
    with mpmath.workdps(DPS):
        e, J0, J1 = lin if lin is not None else se3_row_linearization(row)
        W = [[mpmath.mpf(row[36 + 6 * i + j]) for j in range(6)] for i in range(6)]
        return se3_terms(MP, e, J0, J1, W, row[72] != 0, row[73] != 0)


def se3_row_float64(row):
    """the same outputs from the plain float64 evaluation of the definitions (analytic Jacobians)"""
    C = F64
    (Ri, ti), (Rj, tj), (Rz, tz) = _pose(C, row[0:12]), _pose(C, row[12:24]), _pose(C, row[24:36])
    e = se3_error(C, Ri, ti, Rj, tj, Rz, tz)
    J0, J1 = se3_jacobians_analytic(C, Ri, ti, Rj, tj, Rz, tz)
    W = [[float(row[36 + 6 * i + j]) for j in range(6)] for i in range(6)]
    return se3_terms(C, e, J0, J1, W, row[72] != 0, row[73] != 0)


def _prior_hessian(C, J, W):
    return _lower(_jtwj(J, W, J))


def prior_block_reference(val18, X):
    """cov_prior_block: J^T diag(W) J of the EdgeSE3Prior (Zinv = val[0:12], W = val[12:18]) at X, lower triangle; 50 digits"""
    with mpmath.workdps(DPS):
        (R, t), (Rz, tz) = _pose(MP, X), _pose(MP, val18[:12])
        W = [[mpmath.mpf(val18[12 + i]) if i == j else mpmath.mpf(0) for j in range(6)] for i in range(6)]
        return _prior_hessian(MP, prior_jacobian_central(R, t, Rz, tz), W)


def prior_block_float64(val18, X):
    (R, t), (Rz, tz) = _pose(F64, X), _pose(F64, val18[:12])
    W = [[float(val18[12 + i]) if i == j else 0.0 for j in range(6)] for i in range(6)]
    return _prior_hessian(F64, prior_jacobian_analytic(F64, R, t, Rz, tz), W)


def prior_block_full_reference(val12, W36, X):
    with mpmath.workdps(DPS):
        (R, t), (Rz, tz) = _pose(MP, X), _pose(MP, val12)
        W = [[mpmath.mpf(W36[6 * i + j]) for j in range(6)] for i in range(6)]
        return _prior_hessian(MP, prior_jacobian_central(R, t, Rz, tz), W)


def prior_block_full_float64(val12, W36, X):
    (R, t), (Rz, tz) = _pose(F64, X), _pose(F64, val12)
    W = [[float(W36[6 * i + j]) for j in range(6)] for i in range(6)]
    return _prior_hessian(F64, prior_jacobian_analytic(F64, R, t, Rz, tz), W)


def prior_block3(C, val12, W36, X):
    """cov_prior_block3: R_E^T W R_E, W the symmetric 3x3 whose LOWER triangle is the top-left block of the table row; lower triangle"""
    RE = _mm(_mat(C, val12[:9]), _mat(C, X[:9]))
    W = [[C.num(W36[6 * max(i, j) + min(i, j)]) for j in range(3)] for i in range(3)]
    H = _mm(_tr(RE), _mm(W, RE))
    return _lower(H, 3)


def prior_full_hessian(C, J36, W36):
    J = [[C.num(J36[6 * i + j]) for j in range(6)] for i in range(6)]
    W = [[C.num(W36[6 * i + j]) for j in range(6)] for i in range(6)]
    return _prior_hessian(C, J, W)


def prior3_mul_add(C, w6, e, acc):
    W = [[C.num(w6[max(i, j) * (max(i, j) + 1) // 2 + min(i, j)]) for j in range(3)] for i in range(3)]
    return [C.num(acc[i]) + sum(W[i][j] * C.num(e[j]) for j in range(3)) for i in range(3)]


def with_mp(f, *args):
    """f(MP, ...) at 50 digits"""
    with mpmath.workdps(DPS):
        return f(MP, *args)


def to_f64_err(got, ref):
    """|got - ref| per entry as float64, the difference taken at 50 digits (got: floats, ref: mpf)"""
    with mpmath.workdps(DPS):
        return np.array([float(abs(mpmath.mpf(float(g)) - r)) for g, r in zip(got, ref)])


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def rotvec(v):
    """Rodrigues, float64, row-major 3x3 as a (3, 3) array"""
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


AXES = {"x": np.array([1.0, 0, 0]), "y": np.array([0, 1.0, 0]), "z": np.array([0, 0, 1.0]), "d": np.ones(3) / math.sqrt(3.0)}


def half_turn(n):
    """the exact half turn 2 n n^T - I about the unit vector n"""
    n = np.asarray(n, dtype=np.float64)
    return 2.0 * np.outer(n, n) - np.eye(3)


def near_axis(rng, k, spread=0.3):
    """a random unit axis whose largest component is k (so that a rotation beyond 120 degrees about it takes branch 1 + k)"""
    a = rng.normal(0, spread, 3)
    a[k] = 1.0
    return a / np.linalg.norm(a)


# relative rotation Xi^T Xj / error rotation Zinv Xi^T Xj in degrees: the pairs at which the oracle's linearisation was checked, and the
# small angles every other 6-DoF test draws
SE3_ANGLE_PAIRS = ((30, 150), (150, 5), (150, 150), (170, 130), (125, 125), (2, 1))


def spd6(rng):
    """a full SPD information matrix, as test_gpu_covariance._twist_batch builds it"""
    A = rng.normal(size=(6, 6))
    W = A @ A.T + 6 * np.eye(6)
    return W * (1e3 / np.trace(W))


def se3_base_rows(seed=11):
    """[N, 72] rows (Xi 12, Xj 12, Zinv 12, W 36) and per row the branches (of Zinv, of Xi^T Xj, of the error rotation).
    Relative and error rotations: every angle pair about axes led by x, y and z and about the diagonal; then inverse measurements
    beyond 120 degrees about each axis, so that the Jacobian's conversion of Zinv takes every branch as well."""
    rng = np.random.default_rng(seed)
    rows, branches = [], []

    def add(RB, Rz):
        Ri = rotvec(rng.normal(0, 1.0, 3))
        ti = rng.normal(0, 2.0, 3)
        Rj = Ri @ RB
        tj = ti + rng.normal(0, 1.0, 3)
        tB = Ri.T @ (tj - ti)
        tz = -(Rz @ tB) + rng.normal(0, 0.02, 3)
        row = np.concatenate([Ri.ravel(), ti, Rj.ravel(), tj, Rz.ravel(), tz, spd6(rng).ravel()])
        rows.append(row)
        branches.append((branch_of(Rz.ravel()), branch_of((Ri.T @ Rj).ravel()), branch_of((Rz @ (Ri.T @ Rj)).ravel())))

    def axis(k):
        return AXES["d"] if k == 3 else near_axis(rng, k)

    for rel, err in SE3_ANGLE_PAIRS:
        for kb in range(4):
            for ke in range(4):
                ab, ae = axis(kb), axis(ke)
                RB = rotvec(ab / np.linalg.norm(ab) * math.radians(rel))
                RE = rotvec(ae / np.linalg.norm(ae) * math.radians(err))
                add(RB, RE @ RB.T)
    for ang in (125, 150, 170):
        for kz in range(4):
            for kb in range(4):
                az, ab = axis(kz), axis(kb)
                add(rotvec(ab / np.linalg.norm(ab) * math.radians(150 if kb % 2 else 20)), rotvec(az / np.linalg.norm(az) * math.radians(ang)))
    return np.array(rows), np.array(branches)


def prior_base_rows(seed=12):
    """[N, 24] rows (Zinv 12, X 12) and the branch of the error rotation Zinv X: 121, 150 and 175 degrees about axes led by x, y, z and
    about the diagonal, and the small errors of the other tests"""
    rng = np.random.default_rng(seed)
    rows, branches = [], []
    for ang in (1.0, 121.0, 150.0, 175.0):
        for k in range(4):
            for _ in range(3):
                a = AXES["d"] if k == 3 else near_axis(rng, k)
                RE = rotvec(a * math.radians(ang))
                Rz = rotvec(rng.normal(0, 1.0, 3))
                R = Rz.T @ RE
                t = rng.normal(0, 2.0, 3)
                tz = -(Rz @ t) + rng.normal(0, 0.05, 3)
                rows.append(np.concatenate([Rz.ravel(), tz, R.ravel(), t]))
                branches.append(branch_of((Rz @ R).ravel()))
    return np.array(rows), np.array(branches)


# ---- the 6x6 block steps of the general window kernel (window_block_device.h) ---------------------------------------------------------------
# Matrices are 6x6 lists of lists over the number type.
def mat6(C, rows36):
    """a 6x6 list of lists from 36 row-major numbers"""
    return [[C.num(rows36[6 * i + j]) for j in range(6)] for i in range(6)]


def chol6(C, A):
    """The Cholesky factor of the symmetric 6x6 A (its lower triangle is read): G lower with G G^T = A, column by column, and the inverse
    pivots ig_j = 1 / G_jj"""
    G = [[C.num(0)] * 6 for _ in range(6)]
    ig = [None] * 6
    for j in range(6):
        d = A[j][j] - sum(G[j][k] * G[j][k] for k in range(j))
        G[j][j] = C.sqrt(d)
        ig[j] = 1 / G[j][j]
        for i in range(j + 1, 6):
            G[i][j] = (A[i][j] - sum(G[i][k] * G[j][k] for k in range(j))) / G[j][j]
    return G, ig


def chol6_pivots(A36):
    """the exact (50-digit) pivots d_j = A_jj - sum_k G_jk^2 of the float64 matrix A36 (36 row-major), up to and including the first one
    that is not positive and finite"""
    with mpmath.workdps(DPS):
        A = [[mpmath.mpf(float(A36[6 * i + j])) for j in range(6)] for i in range(6)]
        G = [[mpmath.mpf(0)] * 6 for _ in range(6)]
        out = []
        for j in range(6):
            d = A[j][j] - sum(G[j][k] * G[j][k] for k in range(j))
            out.append(d)
            if not (d > 0 and mpmath.isfinite(d)):
                break
            G[j][j] = mpmath.sqrt(d)
            for i in range(j + 1, 6):
                G[i][j] = (A[i][j] - sum(G[i][k] * G[j][k] for k in range(j))) / G[j][j]
        return out


def forward_row(C, G, ig, s):
    """x G^T = s with the factor's inverse pivots given: x_c = (s_c - sum_{k<c} x_k G_ck) ig_c"""
    x = []
    for c in range(6):
        x.append((s[c] - sum(x[k] * G[c][k] for k in range(c))) * ig[c])
    return x


def back_solve(C, G, ig, t):
    """G^T x = t: x_r = (t_r - sum_{s>r} G_sr x_s) ig_r"""
    x = [None] * 6
    for r in range(5, -1, -1):
        x[r] = (t[r] - sum(G[s][r] * x[s] for s in range(r + 1, 6))) * ig[r]
    return x


def dot_sub(C, a, b, out):
    return out - sum(x * y for x, y in zip(a, b))


def chol_spd_cases(seed=21):
    """[(class, A 36 row-major)]: J^T J + lambda I with the singular values of J from 1 down to 1e-8, so that the condition number is about
    1 / lambda (classes 'cond 1e0' .. 'cond 1e12'; lambda I alone: 'cond 1'), and diagonal matrices spanning 1e-12 .. 1e12"""
    rng = np.random.default_rng(seed)
    out = []
    for e in (0, 2, 4, 6, 8, 10, 12):
        for _ in range(5):
            U, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            V, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            J = U @ np.diag(10.0 ** np.linspace(0, -8, 6)) @ V.T
            A = J.T @ J + 10.0 ** -e * np.eye(6)
            out.append((f"cond 1e{e}", ((A + A.T) / 2).ravel()))
    for lam in (1.0, 1e-3, 7.0):
        out.append(("cond 1", (lam * np.eye(6)).ravel()))
    span = 10.0 ** np.array([-12.0, -7, -2, 3, 8, 12])
    for _ in range(4):
        out.append(("diagonal", np.diag(rng.permutation(span)).ravel()))
    return out


CHOL_FAIL_KINDS = ("negative", "zero", "inf", "nan")


def chol_failing_cases(seed=22):
    """[(A 36 row-major, position, kind, the same with the pivot put right)]: A = L D L^T with L unit lower triangular with small integer
    entries and D powers of four, so that A is exact in float64 and its exact pivots ARE the entries of D; the pivot at `position` (0, 3,
    5) is -4 (negative), 0 (zero), or the diagonal entry itself is +inf / NaN (then so is the pivot).  Every other pivot is at least 1/4."""
    rng = np.random.default_rng(seed)
    out = []
    for p in (0, 3, 5):
        for kind in CHOL_FAIL_KINDS:
            for _ in range(2):
                Lm = np.tril(rng.integers(-2, 3, (6, 6)).astype(np.float64), -1) + np.eye(6)
                D = 4.0 ** rng.integers(-1, 3, 6)
                good = Lm @ np.diag(D) @ Lm.T
                D[p] = {"negative": -4.0, "zero": 0.0}.get(kind, D[p])
                A = Lm @ np.diag(D) @ Lm.T
                if kind in ("inf", "nan"):
                    A[p, p] = np.inf if kind == "inf" else np.nan
                out.append((A.ravel(), p, kind, good.ravel()))
    return out


def solve_operands(seed=23, n=48):
    """(random, integer) operand sets for the row solves: G (36 row-major, strict lower triangle used), ig (6), s (6).  The integer set —
    integer G and s, inverse pivots powers of two — solves exactly in float64"""
    rng = np.random.default_rng(seed)
    rnd = np.concatenate([np.tril(rng.normal(size=(n, 6, 6)), -1).reshape(n, 36), rng.uniform(0.5, 2.0, (n, 6)), rng.normal(size=(n, 6)) * 3], axis=1)
    ints = np.concatenate([np.tril(rng.integers(-3, 4, (n, 6, 6)), -1).reshape(n, 36), 2.0 ** rng.integers(-2, 2, (n, 6)), rng.integers(-8, 9, (n, 6))],
                          axis=1).astype(np.float64)
    return rnd, ints
