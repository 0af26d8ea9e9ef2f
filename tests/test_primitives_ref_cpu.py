"""tests/_primitives_ref.py is what tests/test_gpu_device_primitives.py holds the device to; here it is checked without a GPU: its
conversion against exact quaternions in every branch, its hand-taken derivatives against its own 50-digit central differences, its
float64 evaluation against its 50-digit one, and the branch coverage of the inputs it generates.  (tests/test_oracle_kats.py holds
the oracle's linearisation to it on the same inputs.)"""
import math

import mpmath
import numpy as np

import _primitives_ref as P


def _max_abs(A, B):
    return max(float(abs(a - b)) for ra, rb in zip(A, B) for a, b in zip(ra, rb))


def test_conversion_inverts_the_rotation_matrix_of_a_quaternion_in_every_branch():
    rng = np.random.default_rng(0)
    seen = set()
    with mpmath.workdps(P.DPS):
        cases = [rng.normal(size=4) for _ in range(400)]
        cases += [np.array(q, dtype=float) for q in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 1, 1), (1, 0, 0, 0), (0.01, 1, 1, 0))]
        for c in cases:
            q = [mpmath.mpf(float(x)) for x in c]
            n = mpmath.sqrt(sum(x * x for x in q))
            q = [x / n for x in q]
            R = P.quat_to_mat(P.MP, q)             # orthonormal to 50 digits
            seen.add(P.branch_of([float(x) for row in R for x in row]))
            back = P.mat_to_quat(P.MP, R)
            d = min(max(abs(a - b) for a, b in zip(back, q)), max(abs(a + b) for a, b in zip(back, q)))
            assert d < mpmath.mpf(10) ** -45, (c, d)
            unit, sg = P.quat_normalize_sign(P.MP, [3 * x for x in back])
            assert unit[0] >= 0 and sg == (-1 if back[0] < 0 else 1)
            assert max(abs(sg * a - b) for a, b in zip(back, unit)) < mpmath.mpf(10) ** -45
    assert seen == {0, 1, 2, 3}


def test_generated_rows_cover_every_branch_of_every_conversion():
    base, branches = P.se3_base_rows()
    assert base.shape[1] == 72
    for conv in range(3):   # the inverse measurement, the relative rotation, the error rotation
        assert set(branches[:, conv]) == {0, 1, 2, 3}
    # every ordered pair (branch of Xi^T Xj, branch of the error rotation) occurs: the qA / qB product sees them combined
    assert len({(b, e) for _, b, e in branches}) == 16
    _, pb = P.prior_base_rows()
    assert set(pb) == {0, 1, 2, 3} and np.bincount(pb).min() >= 9


def test_hand_taken_derivatives_match_central_differences_at_50_digits():
    # (the rows are float64 matrices, orthonormal to a few 2^-53 only: the hand-taken derivative assumes orthonormality, so the two differ
    #  by that times the Jacobian's magnitude, <= 20 here)
    base, _ = P.se3_base_rows()
    with mpmath.workdps(P.DPS):
        for row in base[::3]:
            (Ri, ti), (Rj, tj), (Rz, tz) = P._pose(P.MP, row[0:12]), P._pose(P.MP, row[12:24]), P._pose(P.MP, row[24:36])
            J0, J1 = P.se3_jacobians_central(Ri, ti, Rj, tj, Rz, tz)
            A0, A1 = P.se3_jacobians_analytic(P.MP, Ri, ti, Rj, tj, Rz, tz)
            assert _max_abs(J0, A0) < 1e-14 and _max_abs(J1, A1) < 1e-14
        for row in P.prior_base_rows()[0]:
            (Rz, tz), (R, t) = P._pose(P.MP, row[:12]), P._pose(P.MP, row[12:])
            assert _max_abs(P.prior_jacobian_central(R, t, Rz, tz), P.prior_jacobian_analytic(P.MP, R, t, Rz, tz)) < 1e-14


def test_float64_evaluation_is_the_reference_up_to_rounding():
    base, _ = P.se3_base_rows()
    for row in base[::5]:
        r = np.concatenate([row, [1.0, 1.0]])
        ref, f64 = P.se3_row_reference(r), P.se3_row_float64(r)
        for name, sl in P.SE3_SLICES.items():
            err = P.to_f64_err(f64[sl], ref[sl])
            scale = max(abs(float(x)) for x in ref[sl])
            assert err.max() <= 1e-12 * scale, (name, err.max(), scale)   # (chi cancels metres of translation down to centimetres)


def test_rodrigues_helper_and_exact_half_turns():
    for a in P.AXES.values():
        R = P.rotvec(a * math.radians(150))
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.trace(R) - (1 + 2 * math.cos(math.radians(150)))) < 1e-15
        H = P.half_turn(a)
        assert np.allclose(H @ H, np.eye(3), atol=1e-15) and np.allclose(H @ a, a, atol=1e-15)


def test_cholesky_cases_fail_where_they_say_and_by_a_margin_no_rounding_can_close():
    """the matrices behind the exact comparison of the block Cholesky's ok flag (tests/test_gpu_device_primitives.py): at 50 digits every
    pivot before the named position is at least 1/4, the named pivot is -4 (at most -1e-3 of the diagonal entry), exactly 0, +inf or NaN, and
    the repaired matrix has every pivot at least 1/4"""
    seen = set()
    for A, p, kind, good in P.chol_failing_cases():
        seen.add((p, kind))
        d = P.chol6_pivots(A)
        assert len(d) == p + 1 and all(x >= 0.25 for x in d[:p]), (p, kind, d)
        if kind == "negative":
            assert d[p] == -4 and d[p] <= -1e-3 * abs(A[7 * p]), (p, d[p], A[7 * p])
        elif kind == "zero":
            assert d[p] == 0
        else:
            assert (d[p] == mpmath.inf) if kind == "inf" else mpmath.isnan(d[p])
        dg = P.chol6_pivots(good)
        assert len(dg) == 6 and all(x >= 0.25 for x in dg), (p, kind, dg)
    assert seen == {(p, k) for p in (0, 3, 5) for k in P.CHOL_FAIL_KINDS}


def test_positive_definite_cases_span_the_condition_numbers_and_keep_their_pivots_clear_of_rounding():
    conds = {}
    for cls, A in P.chol_spd_cases():
        d = P.chol6_pivots(A)
        assert len(d) == 6 and all(x > 1e-13 * abs(A[7 * j]) for j, x in enumerate(d)), (cls, d)   # (rounding moves a pivot by ~1e-15 of it)
        conds.setdefault(cls, []).append(np.linalg.cond(A.reshape(6, 6)))
    assert max(conds["cond 1"]) == 1.0 and min(conds["cond 1e12"]) > 1e11 and max(conds["cond 1e0"]) < 3
    assert all(c == 1e24 or abs(c / 1e24 - 1) < 1e-9 for c in conds["diagonal"])


def test_block_step_references_agree_between_float64_and_50_digits():
    rnd, ints = P.solve_operands()
    for row in list(rnd[:8]) + list(ints[:8]):
        G, ig, s = row[:36], [float(x) for x in row[36:42]], [float(x) for x in row[42:]]
        for f in (P.forward_row, P.back_solve):
            a = f(P.F64, P.mat6(P.F64, G), ig, s)
            with mpmath.workdps(P.DPS):
                b = f(P.MP, P.mat6(P.MP, [float(x) for x in G]), [mpmath.mpf(x) for x in ig], [mpmath.mpf(x) for x in s])
            assert P.to_f64_err(a, b).max() <= 1e-12 * max(abs(float(x)) for x in b)
    for cls, A in P.chol_spd_cases()[::6]:
        G, ig = P.chol6(P.F64, P.mat6(P.F64, A))
        recon = np.array(G) @ np.array(G).T
        assert np.abs(np.tril(recon - A.reshape(6, 6))).max() <= 1e-14 * np.abs(A).max(), cls
        assert np.allclose(np.array(ig) * np.diag(np.array(G)), 1.0, rtol=1e-15)
