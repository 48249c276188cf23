"""CPU checks of the blocked stepper's twisted interior solve (crb_blocked.h: blk_twist_interior_solve, restated on the host by
crb_blocked_twist_solve_host): a lane's nodes 0 and 2 are eliminated into its centre node, which needs the mirror structure
of a mass matrix of equal elements -- every interior diagonal block B diagonal, C = J A J with J = diag(1, -1) on (w, phi).
On the five plans of test_blocked_solve_cpu.py: the plan's own node blocks have that structure bitwise, the twisted solve
reproduces a dense solve at that file's 1e-13, its difference from the block-Thomas restatement is recorded (printed, and
bounded by the two solves' own bound against the dense one), and node blocks without the structure are refused."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import nitinol_columns
from tests.test_blocked_solve_cpu import blocked_solve, node_blocks, plan_mass

_dp = C.POINTER(C.c_double)
TOL = 1e-13   # (test_blocked_solve_cpu.py's)

PLANS = [("nonlinear", dict()), ("linear", dict()), ("nonlinear", dict(length=0.05)),
         ("nonlinear", dict(length=1.0, density=1000.0)), ("linear", dict(radius=0.02))]


def plan_columns(kind, scale):
    cols = nitinol_columns(256, kind)
    if "length" in scale:
        cols["length"] = np.full(256, scale["length"])
    if "density" in scale:
        cols["density"] = np.full(256, scale["density"])
    if "radius" in scale:
        rr = scale["radius"]
        cols["moment_inertia"] = np.full(256, np.pi * rr**4 / 4)
        cols["cross_area"] = np.full(256, np.pi * rr**2)
    return cols


@pytest.fixture(scope="module", params=range(len(PLANS)), ids=[f"{k}-{'-'.join(s) or 'nitinol'}" for k, s in PLANS])
def plan(request):
    kind, scale = PLANS[request.param]
    cols = plan_columns(kind, scale)
    M = plan_mass(cols)
    assert M.shape == (768, 768)
    return M, node_blocks(M), float(cols["length"][0])


def twist_solve_blocks(blk, L, r):
    """x, levels, norms of crb_blocked_twist_solve_host on node blocks [256][15]"""
    from continuum_robot import _native as nat

    lib = nat.load()
    blk = np.ascontiguousarray(blk)
    x = np.zeros_like(r)
    lv = C.c_int32(0)
    norms = np.zeros(6)
    nat.check(lib.crb_blocked_twist_solve_host(blk.ctypes.data_as(_dp), L, np.ascontiguousarray(r).ctypes.data_as(_dp),
                                               x.ctypes.data_as(_dp), C.byref(lv), norms.ctypes.data_as(_dp)))
    return x, lv.value, norms


def test_node_blocks_have_the_mirror_structure_bitwise(plan):
    """Columns of a node block: [a_ax, b_ax, c_ax, A[4], B[4], C[4]].  Every node but the tip (no right neighbour); the node at
    the fixed root has no left coupling, so C = J A J is asked of the others."""
    _, blk, _ = plan
    B, A, Cr = blk[:, 7:11], blk[:, 3:7], blk[:, 11:15]
    assert np.all(B[:255, 1] == 0.0) and np.all(B[:255, 2] == 0.0)
    J = np.array([1.0, -1.0, -1.0, 1.0])
    assert np.array_equal(Cr[1:255], A[1:255] * J)
    assert np.array_equal(blk[1:255, 2], blk[1:255, 0])
    # what the twisted form takes as one block: the diagonal blocks and both couplings are the same at every interior node
    assert np.all(blk[1:255, 1] == blk[0, 1]) and np.all(B[1:255] == B[0])
    assert np.all(A[2:255] == A[1]) and np.all(Cr[1:255] == Cr[0])
    # ... and with them the centre pivot Dc = B1 - A1 B0^-1 C0 - C1 B2^-1 A2 has no off-diagonal, exactly
    a, c, bi = A[1].reshape(2, 2), Cr[1].reshape(2, 2), np.diag(1.0 / np.diag(B[0].reshape(2, 2)))
    p1, p2 = (a @ bi) @ c, (c @ bi) @ a
    assert p1[0, 1] == -p2[0, 1] and p1[1, 0] == -p2[1, 0] and p1[0, 1] != 0.0


def test_twisted_solve_matches_a_dense_solve(plan):
    M, blk, L = plan
    rng = np.random.default_rng(7)
    for trial in range(3):
        r = rng.normal(size=768) * (10.0 ** rng.uniform(-3, 3, 768))
        want = np.linalg.solve(M, r)
        got, lv, norms = twist_solve_blocks(blk, L, r)
        thomas, lv_t, norms_t = blocked_solve(M, L, r)
        # the separator system is the same one: same levels, same multipliers
        assert lv == lv_t and np.array_equal(norms, norms_t)
        for c in range(3):
            scale = np.max(np.abs(want[c::3]))
            err = np.max(np.abs(got[c::3] - want[c::3])) / scale
            diff = np.max(np.abs(got[c::3] - thomas[c::3])) / scale
            print(f"trial {trial} dof {c}: twisted vs dense {err:.2e}, twisted vs block Thomas {diff:.2e}")
            assert err <= TOL, (trial, c, err)
            # (each is within TOL of the dense solve, so they are within 2 TOL of each other; not bit for bit, or the
            #  twisted form did not run)
            assert 0.0 < diff <= 2 * TOL, (trial, c, diff)
        res = np.max(np.abs(M @ got - r)) / np.max(np.abs(r))
        print(f"trial {trial}: residual {res:.2e}")
        assert res <= TOL, res


def every_lane(blk, node, col, change):
    """`blk` with entry `col` of interior node `node` of EVERY lane changed: the lanes stay bitwise uniform"""
    out = blk.copy()
    for lane in range(64):
        out[4 * lane + node, col] = change(out[4 * lane + node, col])
    return out


@pytest.mark.parametrize("node,col,change", [
    (1, 8, lambda v: 1e-9),             # B[0][1] of the centre node: an off-diagonal of B
    (0, 9, lambda v: -1e-12),           # B[1][0] of node 0
    (2, 8, lambda v: 1e-300),           # B[0][1] of node 2, as small as it gets
    (1, 12, lambda v: -v),              # C[0][1] of the centre node: the sign that J flips
    (1, 11, lambda v: v * (1 + 2e-16)),  # C[0][0] of the centre node, by one rounding
    (0, 2, lambda v: v * 1.5),          # the axial right coupling of node 0
], ids=["B1_wp", "B0_pw", "B2_wp_tiny", "C1_wp_sign", "C1_ww_ulp", "C0_axial"])
def test_blocks_without_the_mirror_structure_are_refused(plan, node, col, change):
    """Uniform over the lanes, so that the block-Thomas restatement still takes them, but not mirrored."""
    from continuum_robot import _native as nat

    M, blk, L = plan
    bad = every_lane(blk, node, col, change)
    assert not np.array_equal(bad, blk)
    r = np.ones(768)
    with pytest.raises(nat.NativeError, match="mirror structure"):
        twist_solve_blocks(bad, L, r)
    # the unperturbed blocks pass, and the existing entry point does not ask for the structure
    twist_solve_blocks(blk, L, r)
    lib = nat.load()
    x = np.zeros(768)
    nat.check(lib.crb_blocked_solve_host(np.ascontiguousarray(bad).ctypes.data_as(_dp), L, r.ctypes.data_as(_dp),
                                         x.ctypes.data_as(_dp), None, None))
    assert np.isfinite(x).all()


def test_a_host_plan_holds_no_blocked_tables():
    """crb_plan_get_blocked_form is declared, exported and bound; the blocked tables are built for device plans only."""
    import os

    from continuum_robot import _native as nat

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crbeam.h")).read()
    assert "int crb_plan_get_blocked_form(const crb_plan* plan, int32_t* form, int32_t* levels);" in hdr
    assert "int crb_blocked_twist_solve_host(" in hdr
    assert nat.Plan(nitinol_columns(256, "nonlinear"), n_beams=1, device=-1).blocked_form() == (0, 0)


def test_one_lane_off_is_refused_as_non_uniform(plan):
    from continuum_robot import _native as nat

    _, blk, L = plan
    bad = blk.copy()
    bad[4 * 20 + 1, 12] *= 1.01   # one entry of C in one lane
    with pytest.raises(nat.NativeError, match="not uniform|mirror structure"):
        twist_solve_blocks(bad, L, np.ones(768))
