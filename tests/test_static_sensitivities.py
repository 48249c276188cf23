"""Sensitivities of the static equilibrium on the GPU (BeamEnsemble.static_jvp / static_vjp / equilibrium; crb_static.h:
crb_static_sens_kernel, crb_paramgrad.h: crb_static_param_kernel).

1. The whole chain (solve_static -> static_vjp -> parameter dict) against central differences of equilibria of the C
   oracle, on short rods, by the rule of test_adjoint.py / test_param_gradients.py.
2. Every thread mapping against LAPACK on the dense J = -M A21 (linearize, plan.mass()), at seeded smooth shapes, under the
   conditioning rule of tests/test_static_sensitivities_cpu.py (``conditioning_bound``).
3. Duality of static_jvp and static_vjp, and that J^-T is not J^-1.
4. The parameter records against the oracle's k(q) and dg/d(g_x, g_y), to rounding.
5. Bitwise properties: directions per call, heterogeneous ensembles, a beam seeded NaN.
6. ``equilibrium``: backward is static_vjp, a beam that did not converge gets a zero row, nothing resident is touched.
7. 4096 x 256 once.

An interior FIXED / PINNED node shifts the reference's reduced gravity indexing just as a PINNED root does, so under gravity
such a plan is refused by the rule the plan builder records (a rotation source more than one slot from a node its segment
loads); the interior-pin case therefore runs without gravity and asserts the refusal with it."""
import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams
from tests.helpers import nitinol_columns, oracle_beam
from tests.test_static_sensitivities_cpu import block_errors, block_max, conditioning_bound

pytestmark = pytest.mark.gpu
G_Y = -9.81
NR = 4   # crb_static_launch.h: STATIC_SENS_NR


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def force_params(grav):
    return ForceParams(enable_gravity_effects=bool(grav))


# =========================================================================== 1. the chain against the oracle's differences
def xi_of(n):
    """seeded element weights of the column directions: E_e (1 + eps xi_e)"""
    return np.random.default_rng(77).uniform(0.5, 1.5, n)


# Step sizes: those at which the oracle's own two differences agree, measured on the CPU over a ladder 1e-2 ... 3e-5 with
# this file's loss (|FD(h) - FD(h/4)| / |FD(h/4)|, the beams checked): force 1e-3 N <= 3.2e-8, elastic_modulus and
# moment_inertia 1e-4 <= 1.1e-8 except moment_inertia of nonlinear_8's second beam (3.6e-7: that derivative nearly cancels,
# 2.4e-4 against 6.3e-3 for the first beam), g_y 1e-4 <= 4.6e-9, g_x 1e-3 <= 7.8e-8 (at 1e-4 it is already 1.9e-6 on
# nonlinear_8: the loss is far less sensitive to g_x, 5e-5, and the equilibrium's residual floor shows).  The corrected axial
# term raises the oracle's residual floor to 6e-11 of |k| (large cancelling terms), so its differences are noisier and its
# steps larger: the table below gives <= 3.9e-8 there.
FD_STEP = {"force": 1e-3, "elastic_modulus": 1e-4, "moment_inertia": 1e-4, "g_y": 1e-4, "g_x": 1e-3}
FD_STEP_OF_CASE = {"corrected_8": {"force": 1e-3, "elastic_modulus": 3e-4, "moment_inertia": 1e-3, "g_y": 3e-4, "g_x": 1e-2}}
CHAIN_CASES = {
    # name: (elements, kind, corrected_axial, beams)
    "nonlinear_8": (8, "nonlinear", False, 2),
    "linear_8": (8, "linear", False, 2),
    "nonlinear_6_packed": (6, "nonlinear", False, 12),
    "corrected_8": (8, "nonlinear", True, 1),
}


def chain_oracle(cols, corrected, direction=None, eps=0.0):
    c = {k: np.array(v, copy=True) for k, v in cols.items()}
    grav = (0.0, G_Y, 0.0)
    if direction in ("elastic_modulus", "moment_inertia"):
        c[direction] = c[direction] * (1.0 + eps * xi_of(len(c[direction])))
    elif direction == "g_y":
        grav = (0.0, G_Y * (1.0 + eps), 0.0)
    elif direction == "g_x":
        grav = (eps * 9.81, G_Y, 0.0)
    return oracle_beam(c, enable_gravity=True, gravity=grav, corrected_axial=corrected)


def host_newton(ob, u, q, max_iter=12):
    """numpy_newton's pattern (tests/test_static_equilibrium.py), warm-started at ``q``: Newton on the ORACLE's residual with
    a central-difference tangent, a step halved while it does not lower the residual, until no step lowers it any more"""
    n = u.size
    zero = np.zeros(n)
    res = lambda v: ob.internal_force(v) - ob.gravity(np.concatenate([v, zero])) - u   # noqa: E731
    best = np.max(np.abs(res(q)))
    for _ in range(max_iter):
        J = np.empty((n, n))
        for j in range(n):
            h = 1e-6 * max(1e-2, abs(q[j]))   # (fd_tangent's step: the corrected axial term is too noisy for 1e-7 |q|)
            e = np.zeros(n)
            e[j] = h
            J[:, j] = (res(q + e) - res(q - e)) / (2 * h)
        dq = np.linalg.solve(J, res(q))
        for t in (1.0, 0.5, 0.25, 0.125):
            qn = q - t * dq
            hn = np.max(np.abs(res(qn)))
            if hn < best:
                break
        if hn >= best:
            break
        q, best = qn, hn
    return q


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chain_matches_the_oracles_central_differences(name):
    """Loss = seeded random weighting of q.  Rule: |g - FD(h/4)| <= min(max(1e-7, 4 |FD(h) - FD(h/4)|), 1e-6) |FD(h/4)|, every
    direction, h = FD_STEP.  Measured on one MI355X, error (the oracle's own |FD(h) - FD(h/4)|), both relative to FD(h/4),
    worst beam: nonlinear_8 force 2.4e-9 (1.9e-8), elastic_modulus 9.8e-10 (1.2e-8), moment_inertia 5.6e-7 (6.1e-7, the
    derivative that nearly cancels) and 2.9e-9 (4.1e-9) on the first beam, g_y 8.9e-9 (1.1e-8), g_x 1.5e-7 (1.7e-7);
    linear_8 <= 2.3e-9 (3.2e-8) in every direction; nonlinear_6_packed <= 5.1e-9 (3.2e-8) except g_x 1.2e-7 (1.1e-7);
    corrected_8 force 1.2e-7 (9.8e-8), elastic_modulus 6.5e-9 (7.1e-8), moment_inertia 1.0e-8 (5.4e-9), g_y 7.2e-8
    (9.2e-8), g_x 1.5e-8 (2.8e-8).  Wherever the error exceeds 1e-8 it is the size of the oracle's own disagreement."""
    n_el, kind, corrected, B = CHAIN_CASES[name]
    cols = nitinol_columns(n_el, kind)
    ens = BeamEnsemble(cols, B, force_params=force_params(True), corrected_axial=corrected)
    n = ens.n
    rng = np.random.default_rng(2024)
    U = np.zeros((B, n))
    U[:, -3:] = np.array([0.02, 0.05, 0.002])[None, :] * (1.0 + 0.1 * np.arange(B))[:, None]
    sol = ens.solve_static(held_force=U, rtol=1e-11)
    assert bool(sol.converged.all())
    Q = np_(sol.q)
    W = rng.normal(0.0, 1.0, (B, n))
    du = rng.normal(0.0, 1.0, n)
    du /= np.max(np.abs(du))
    fbar, grads = ens.static_vjp(W, Q, params=True)
    assert int(ens.static_status.abs().sum()) == 0
    fbar, grads = np_(fbar), {k: np_(v) for k, v in grads.items()}
    for b in sorted({0, B - 1}):
        q0 = host_newton(chain_oracle(cols, corrected), U[b], Q[b].copy())
        assert np.max(np.abs(q0 - Q[b])) <= 1e-9 * np.max(np.abs(Q[b]))

        def loss(direction, e):
            ob = chain_oracle(cols, corrected, direction, e)
            u = U[b] + (e * du if direction == "force" else 0.0)
            return float(W[b] @ host_newton(ob, u, q0.copy()))

        for direction, h in FD_STEP_OF_CASE.get(name, FD_STEP).items():
            fd1 = (loss(direction, h) - loss(direction, -h)) / (2 * h)
            fd4 = (loss(direction, h / 4) - loss(direction, -h / 4)) / (h / 2)
            if direction == "force":
                g = float(fbar[b] @ du)
            elif direction in ("elastic_modulus", "moment_inertia"):
                g = float(np.sum(xi_of(n_el) * cols[direction] * grads[direction][b, :n_el]))
            elif direction == "g_y":
                g = G_Y * float(grads["gravity"][b, 1])
            else:
                g = 9.81 * float(grads["gravity"][b, 0])
            own = abs(fd1 - fd4) / abs(fd4)
            allowed = min(max(1e-7, 4 * own), 1e-6)
            err = abs(g - fd4) / abs(fd4)
            print(f"[static-chain] {name} beam {b} {direction}: g {g:.12e} FD(h/4) {fd4:.12e} err {err:.2e} allowed {allowed:.2e} "
                  f"|FD(h)-FD(h/4)| {own:.2e}")
            assert err <= allowed, (name, b, direction, g, fd4, err, allowed)


# =========================================================================== 2. every mapping against LAPACK
def pin_at(n, nodes, root="FIXED"):
    bcs = [root] + ["NONE"] * (n - 1)
    for i in nodes:
        bcs[i] = "PINNED"
    return bcs


MAPPING_CASES = {
    # name: (column kwargs, gravity, beams, slots)
    "s1": (dict(n=1, kind="nonlinear"), True, 3, 1),
    "s6_packed": (dict(n=6, kind="nonlinear"), True, 12, 6),
    "s8": (dict(n=8, kind="nonlinear"), True, 3, 8),
    "s33_mixed": (dict(n=33, kind=["linear", "nonlinear", "nonlinear"] * 11), True, 2, 33),
    "s33_interior_pin": (dict(n=33, kind="nonlinear", bcs=pin_at(33, [16])), False, 2, 33),
    "s33_pinned_root": (dict(n=32, kind="nonlinear", bcs=pin_at(32, [20], root="PINNED")), False, 2, 33),
    "s64": (dict(n=64, kind="nonlinear"), True, 2, 64),
    "s65": (dict(n=65, kind="nonlinear"), True, 2, 65),
    "s129": (dict(n=129, kind="nonlinear"), True, 2, 129),
    "s256": (dict(n=256, kind="nonlinear"), True, 2, 256),
}
_CACHE = {}


def smooth_shape(cols, free_index, scale=1.0, seed=0):
    """A reduced q: the parabola w = d (x / L)^2 with tip deflection d = 2 % of the rod's length (times ``scale``), its slope as
    phi and the second-order shortening u = -int w'^2 / 2, plus 1e-5 seeded noise"""
    x = np.concatenate([[0.0], np.cumsum(cols["length"])])
    Lt = x[-1]
    d = 0.02 * Lt * scale
    full = np.stack([-2.0 * d * d * x ** 3 / (3.0 * Lt ** 4), d * (x / Lt) ** 2, 2.0 * d * x / Lt ** 2], axis=1).ravel()
    q = full[free_index]
    return q + np.random.default_rng(seed).normal(0.0, 1e-5, q.size)


def dense_tangent(ens, Q):
    """J = -M A21 per beam from linearize and plan.mass(), with the entries that J cannot have set to zero: J couples a node
    only to itself and its two neighbours (the sensitivities refuse every other plan), so whatever -M A21 holds elsewhere is
    the rounding of M (M^-1 J), eps cond(M) |J| per entry, spread over all n^2 entries -- against a bound built on a 4-ulp
    perturbation, noise that belongs to this reference and not to the code under test"""
    n = ens.n
    A, _ = ens.linearize(np.concatenate([Q, np.zeros_like(Q)], axis=1))
    J = -np.einsum("ij,bjk->bik", np.asarray(ens.plan.mass()), np_(A)[:, n:, :n])
    node = np.asarray(ens.free_index) // 3
    J[:, np.abs(node[:, None] - node[None, :]) > 1] = 0.0
    return J


def mapping_case(name):
    """the ensemble of a mapping case, its shapes Q, dense J per beam and the static_vjp / static_jvp results -- once"""
    if name not in _CACHE:
        kw, grav, B, slots = MAPPING_CASES[name]
        kw = dict(kw)
        cols = nitinol_columns(kw.pop("n"), **kw)
        ens = BeamEnsemble(cols, B, force_params=force_params(grav))
        assert ens.plan.layout.n_slots == slots
        n = ens.n
        fi = np.asarray(ens.free_index)
        Q = np.stack([smooth_shape(cols, fi, 1.0 - 0.3 * b / max(B - 1, 1), seed=b) for b in range(B)])
        J = dense_tangent(ens, Q)
        rng = np.random.default_rng(len(name) + slots)
        D = NR + 1
        qbar, du = rng.normal(0.0, 1.0, (D, B, n)), rng.normal(0.0, 1.0, (D, B, n))
        mu, grads = ens.static_vjp(qbar, Q, params=True)
        st_v = np_(ens.static_status).copy()
        dq = ens.static_jvp(du, Q)
        st_j = np_(ens.static_status).copy()
        _CACHE[name] = dict(cols=cols, grav=grav, ens=ens, Q=Q, J=J, qbar=qbar, du=du, mu=np_(mu), dq=np_(dq),
                            grads={k: np_(v) for k, v in grads.items()}, dof=fi % 3, status=(st_v, st_j))
    return _CACHE[name]


def lapack_check(c, beams, what):
    """static_vjp against solve(J^T, qbar) and static_jvp against solve(J, du), per direction and DOF block; returns the worst
    error and the worst error / allowed"""
    worst = worst_ratio = 0.0
    for b in beams:
        for got, M, rhs, tag in ((c["mu"][:, b], c["J"][b].T, c["qbar"][:, b], "vjp"), (c["dq"][:, b], c["J"][b], c["du"][:, b], "jvp")):
            ref, allowed = conditioning_bound(M, rhs, c["dof"])
            err = block_errors(got, ref, c["dof"])
            print(f"[static-lapack] {what} beam {b} {tag}: cond {np.linalg.cond(M):.1e} worst block error {err.max():.2e} "
                  f"allowed there {allowed.ravel()[err.argmax()]:.2e} worst error/allowed {np.max(err / allowed):.2e}")
            worst, worst_ratio = max(worst, err.max()), max(worst_ratio, np.max(err / allowed))
            assert np.all(err <= allowed), (what, b, tag, err, allowed)
    return worst, worst_ratio


@pytest.mark.parametrize("name", list(MAPPING_CASES))
def test_every_mapping_matches_lapack(name):
    """D = NR + 1 directions in one call (a full chunk and a tail) and D = 1 (the NR = 1 kernel), every beam.  Bound:
    conditioning_bound.  Measured on one MI355X: worst block error 1.8e-9 (256 slots, condition 8e9); worst error / allowed
    0.79 (64 slots, second beam, vjp: 5e-11 against 6e-11), 0.31 at 256 slots, <= 0.1 at 1 .. 33 slots; 2e10 is the largest
    condition number (129 slots, second beam: error 8e-10, allowed 1.9e-7).  With the out-of-band entries of -M A21 left in
    (dense_tangent) the same solutions were 1.4 x (64 slots), 1.6 x (256) and 4.2 x (full size) the bound, before and after
    the kernel gained its refinement step: that noise was the reference's."""
    c = mapping_case(name)
    assert not c["status"][0].any() and not c["status"][1].any()
    lapack_check(c, range(c["ens"].n_beams), name)
    ens, b = c["ens"], c["ens"].n_beams - 1
    one_v, one_j = np_(ens.static_vjp(c["qbar"][NR], c["Q"])), np_(ens.static_jvp(c["du"][NR], c["Q"]))
    single = dict(c, mu=one_v[None], dq=one_j[None], qbar=c["qbar"][NR:], du=c["du"][NR:])
    lapack_check(single, [b], name + " D=1")
    if name == "s33_interior_pin":   # ... and under gravity the plan is refused, not approximated
        kw = dict(MAPPING_CASES[name][0])
        heavy = BeamEnsemble(nitinol_columns(kw.pop("n"), **kw), 2, force_params=force_params(True))
        for f in (heavy.static_jvp, heavy.static_vjp):
            with pytest.raises(nat.NativeError, match="more than one slot away"):
                f(c["du"][0], c["Q"])


# =========================================================================== 3. duality
@pytest.mark.parametrize("name", ["s8", "s65"])
def test_duality_and_the_transposition(name):
    c = mapping_case(name)
    for b in range(c["ens"].n_beams):
        for d in range(NR + 1):
            qbar, du, mu, dq = c["qbar"][d, b], c["du"][d, b], c["mu"][d, b], c["dq"][d, b]
            _, al_v = conditioning_bound(c["J"][b].T, qbar, c["dof"])
            _, al_j = conditioning_bound(c["J"][b], du, c["dof"])
            lhs, rhs = float(qbar @ dq), float(mu @ du)
            # an entry of block k of dq (mu) may be off by al_j[k] (al_v[k]) times the block's maximum
            l1 = lambda v: np.array([np.sum(np.abs(v[c["dof"] == k])) for k in range(3)])   # noqa: E731
            allowed = float(np.sum(al_j[0] * block_max(dq, c["dof"]) * l1(qbar)) + np.sum(al_v[0] * block_max(mu, c["dof"]) * l1(du)))
            print(f"[static-duality] {name} beam {b} dir {d}: <qbar, dq> {lhs:.12e} <mu, du> {rhs:.12e} diff {abs(lhs - rhs):.2e} "
                  f"allowed {allowed:.2e}")
            assert abs(lhs - rhs) <= allowed
    ens = c["ens"]
    wrong = np_(ens.static_jvp(c["qbar"][0], c["Q"]))
    assert np.min(np.max(block_errors(wrong, c["mu"][0], c["dof"]), axis=-1)) > 1e-3


# =========================================================================== 4. parameter records
@pytest.mark.parametrize("name", list(MAPPING_CASES))
def test_parameter_records_are_mu_dotted_with_the_oracles_forces(name):
    """k is linear in E and g in the gravity vector, so with mu from test 2's call the sums hold to rounding: 1e-12 relative
    to sum |mu_i k_i| (sum |mu_i dg_i|).  Measured worst on one MI355X: <= 8.6e-15 up to 64 slots with a FIXED root, 6.6e-14
    with pins, 1.0e-13 at 65 slots, 3.7e-13 at 129, 8.8e-13 at 256."""
    c = mapping_case(name)
    cols, g, ens = c["cols"], c["grads"], c["ens"]
    ob = oracle_beam(cols, enable_gravity=False)
    obx = oracle_beam(cols, enable_gravity=True, gravity=(1.0, 0.0, 0.0))
    oby = oracle_beam(cols, enable_gravity=True, gravity=(0.0, 1.0, 0.0))
    worst = 0.0
    for b in range(ens.n_beams):
        q = c["Q"][b]
        k = ob.internal_force(q)
        x = np.concatenate([q, np.zeros_like(q)])
        for d in range(NR + 1):
            mu = c["mu"][d, b]
            got = float(np.sum(g["EA_scale"][d, b] + g["EI_scale"][d, b]))
            scale = float(np.sum(np.abs(mu * k)))
            worst = max(worst, abs(got + float(mu @ k)) / scale)
            assert abs(got + float(mu @ k)) <= 1e-12 * scale, (name, b, d, got, -float(mu @ k))
            if c["grav"]:
                for i, o in enumerate((obx, oby)):
                    dg = o.gravity(x)
                    scale = float(np.sum(np.abs(mu * dg)))
                    worst = max(worst, abs(g["gravity"][d, b, i] - float(mu @ dg)) / scale)
                    assert abs(g["gravity"][d, b, i] - float(mu @ dg)) <= 1e-12 * scale, (name, b, d, i)
    print(f"[static-records] {name}: worst {worst:.2e}")
    for key in ("drag_scale", "fluid_density", "drag_coef"):
        assert not g[key].any()
    if not c["grav"]:
        assert not g["gravity"].any()


def test_records_past_a_beams_own_elements_are_zero():
    sets = [nitinol_columns(6, "nonlinear"), nitinol_columns(4, "nonlinear"), nitinol_columns(6, "linear")]
    ens = BeamEnsemble.from_dataframes(sets, force_params=[force_params(True)] * 3)
    rng = np.random.default_rng(8)
    Q = rng.normal(0.0, 1e-3, (3, ens.n))
    Q[1, 12:] = 0.0
    qbar = rng.normal(0.0, 1.0, (2, 3, ens.n))
    mu, grads = ens.static_vjp(qbar, Q, params=True)
    mu = np_(mu)
    assert not mu[:, 1, 12:].any() and mu[:, 1, :12].all()
    for key in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia"):
        v = np_(grads[key])
        assert not v[:, 1, 4:].any() and v[:, 1, :4].all() and v[:, 0].all()
    dq = np_(ens.static_jvp(qbar, Q))
    assert not dq[:, 1, 12:].any() and dq[:, 1, :12].all()


# =========================================================================== 5. bitwise properties
def bits(a):
    return np.ascontiguousarray(np_(a)).view(np.uint64)


@pytest.mark.parametrize("name", ["s6_packed", "s65", "s256"])
def test_directions_in_one_call_equal_one_call_each(name):
    c = mapping_case(name)
    ens = c["ens"]
    _, records, _, _ = ens._static_sens(c["qbar"], c["Q"], True, True, "test")   # the kernel's own records [D, B, n_node, 8]
    for d in (0, NR - 1, NR):
        mu1, rec1, _, _ = ens._static_sens(c["qbar"][d], c["Q"], True, True, "test")
        assert np.array_equal(bits(mu1[0]), bits(c["mu"][d]))
        assert np.array_equal(bits(rec1[0]), bits(records[d]))
        g1 = ens.static_vjp(c["qbar"][d], c["Q"], params=True)[1]
        for k in ("EA_scale", "EI_scale", "elastic_modulus", "moment_inertia", "drag_scale"):
            assert np.array_equal(bits(g1[k]), bits(c["grads"][k][d])), k
        # (gravity is a torch sum of the records over the nodes, whose order of additions follows the tensor's shape)
        assert np.allclose(np_(g1["gravity"]), c["grads"]["gravity"][d], rtol=1e-14, atol=0.0)
        assert np.array_equal(bits(ens.static_jvp(c["du"][d], c["Q"])), bits(c["dq"][d]))


def test_a_beam_of_a_heterogeneous_ensemble_equals_the_beam_alone():
    from tests.helpers import graded_columns

    sets = [nitinol_columns(6, "nonlinear"), graded_columns(6, "nonlinear", "taper3"), nitinol_columns(6, "linear")]
    ens = BeamEnsemble.from_dataframes(sets, force_params=[force_params(True)] * 3)
    rng = np.random.default_rng(12)
    Q = rng.normal(0.0, 1e-3, (3, ens.n))
    v = rng.normal(0.0, 1.0, (NR + 1, 3, ens.n))
    mu, grads = ens.static_vjp(v, Q, params=True)
    dq = ens.static_jvp(v, Q)
    for b, s in enumerate(sets):
        alone = BeamEnsemble(s, 1, force_params=force_params(True))
        mu1, g1 = alone.static_vjp(v[:, b:b + 1], Q[b:b + 1], params=True)
        assert np.array_equal(bits(mu1[:, 0]), bits(mu[:, b]))
        assert np.array_equal(bits(alone.static_jvp(v[:, b:b + 1], Q[b:b + 1])[:, 0]), bits(dq[:, b]))
        for k in ("EA_scale", "EI_scale", "gravity"):
            assert np.array_equal(bits(g1[k][:, 0]), bits(grads[k][:, b])), k


def test_a_beam_seeded_nan_leaves_its_wave_mates_alone():
    c = mapping_case("s6_packed")
    ens = c["ens"]
    Q = c["Q"].copy()
    Q[3, 7] = np.nan
    for f, ref, v in ((ens.static_vjp, c["mu"], c["qbar"]), (ens.static_jvp, c["dq"], c["du"])):
        got = np_(f(v, Q))
        status = np_(ens.static_status)
        assert status[3] == -2 and not np.delete(status, 3).any()
        assert np.array_equal(bits(np.delete(got, 3, axis=1)), bits(np.delete(ref, 3, axis=1)))
        assert not np.isfinite(got[:, 3]).all()


# =========================================================================== 6. equilibrium
def test_equilibrium_backward_is_static_vjp_and_touches_nothing_resident():
    cols = nitinol_columns(8, "nonlinear")
    B = 3
    ens = BeamEnsemble(cols, B, force_params=force_params(True))
    rng = np.random.default_rng(4)
    ens.set_state(rng.normal(0.0, 1e-3, (B, 2 * ens.n)), time=0.75)
    state0, time0, status0 = ens.state.clone(), ens.time, ens.status.clone()
    U = torch.zeros((B, ens.n), dtype=torch.float64, device=ens.device)
    U[:, -2] = torch.tensor([0.05, 0.5, 5.0], dtype=torch.float64, device=ens.device)
    U.requires_grad_(True)
    W = torch.as_tensor(rng.normal(0.0, 1.0, (B, ens.n)), device=ens.device)
    q, conv = ens.equilibrium(U, rtol=1e-10)
    assert bool(conv.all()) and not conv.requires_grad
    (W * q).sum().backward()
    ref = ens.static_vjp(W, q.detach())
    assert np.array_equal(bits(U.grad), bits(ref))
    sol = ens.solve_static(held_force=U.detach(), rtol=1e-10)
    assert np.array_equal(bits(sol.q), bits(q))
    ens.static_jvp(W, q.detach())
    assert torch.equal(ens.state, state0) and ens.time == time0 and torch.equal(ens.status, status0)


def test_equilibrium_gives_a_beam_that_did_not_converge_a_zero_gradient():
    cols = nitinol_columns(8, "nonlinear")
    B = 3
    ens = BeamEnsemble(cols, B, force_params=force_params(True))
    U = torch.zeros((B, ens.n), dtype=torch.float64, device=ens.device)
    U[:, -2] = torch.tensor([0.0, 50.0, 0.0], dtype=torch.float64, device=ens.device)   # beam 1: beyond one Newton step
    U.requires_grad_(True)
    q, conv = ens.equilibrium(U, load_steps=1, max_iter=1, rtol=1e-12)
    conv = np_(conv)
    assert not conv[1]
    q.sum().backward()
    g = np_(U.grad)
    assert not g[~conv].any()
    ok = ens.equilibrium(U.detach().clone().requires_grad_(True), rtol=1e-10)
    assert bool(ok[1].all())


# =========================================================================== 7. full size once
def test_full_size_ensemble():
    """4096 x 256 nonlinear rods under gravity on test 2's shape scaled per beam, D = 4: every status 0; beams 0, 2047, 4095
    against LAPACK under test 2's rule (their J from a three-beam ensemble of the same rod at the same shapes).  Measured on
    one MI355X: worst block error 6.3e-10, worst error / allowed 0.87 (beam 4095, vjp: 1.6e-10 against 6.3e-10 ... 2.4e-9)."""
    B, n_el, picks = 4096, 256, (0, 2047, 4095)
    cols = nitinol_columns(n_el, "nonlinear")
    ens = BeamEnsemble(cols, B, force_params=force_params(True))
    fi = np.asarray(ens.free_index)
    noise = np.random.default_rng(1).normal(0.0, 1e-5, fi.size)
    clean = smooth_shape(cols, fi, 1.0, seed=1) - noise
    scale = np.linspace(1.0, 0.5, B)
    dof = fi % 3
    # the parabola scales with the deflection (u with its square), the noise stays
    Q = clean[None, :] * np.where(dof == 0, scale[:, None] ** 2, scale[:, None]) + noise[None, :]
    rng = np.random.default_rng(7)
    D = NR
    qbar = torch.as_tensor(rng.normal(0.0, 1.0, (D, 1, ens.n)), device=ens.device).expand(D, B, ens.n)
    Qd = torch.as_tensor(Q, device=ens.device)
    mu = ens.static_vjp(qbar, Qd)
    assert not bool(ens.static_status.any())
    dq = ens.static_jvp(qbar, Qd)
    assert not bool(ens.static_status.any())
    small = BeamEnsemble(cols, len(picks), force_params=force_params(True))
    Qs = Q[list(picks)]
    J = dense_tangent(small, Qs)
    rhs = np_(qbar[:, :1]).repeat(len(picks), axis=1)
    c = dict(J=J, dof=dof, qbar=rhs, du=rhs, mu=np_(mu[:, list(picks)]), dq=np_(dq[:, list(picks)]))
    lapack_check(c, range(len(picks)), "full size")
