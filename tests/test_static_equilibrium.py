"""Static equilibrium and tangent stiffness on the GPU (BeamEnsemble.solve_static / tangent_stiffness, crb_static.h),
checked against the C oracle, the reference-pinned equilibria of tests/golden/g10_static.npz and numpy."""
import numpy as np
import pytest
import torch

from continuum_robot import _native as nat
from continuum_robot.batched import BeamEnsemble
from continuum_robot.models.force_params import ForceParams
from tests.helpers import Golden, assert_blocks, beam_columns, nitinol_columns, oracle_beam

pytestmark = pytest.mark.gpu
G = Golden()
GRAV = ForceParams(enable_gravity_effects=True)


def fd_tangent(ob, q, rel=1e-6):
    n = q.size
    J = np.empty((n, n))
    for j in range(n):
        h = rel * max(1e-2, abs(q[j]))
        e = np.zeros(n)
        e[j] = h
        J[:, j] = (ob.internal_force(q + e) - ob.internal_force(q - e)) / (2 * h)
    return J


def numpy_newton(ob, u, load_steps=8, max_iter=30):
    """Independent host solve: Newton from q = 0 on the ORACLE's residual with a central-difference tangent, along the same
    load path in equal increments, each increment iterated to the residual's fp64 floor (until a step no longer lowers
    it).  Returns the q of the smallest final residual."""
    n = u.size
    zero = np.zeros(n)
    res = lambda q: ob.internal_force(q) - ob.gravity(np.concatenate([q, zero])) - u   # noqa: E731
    q = np.zeros(n)
    r0 = res(q)
    for s in range(1, load_steps + 1):
        lt = s / load_steps
        best = np.inf
        for _ in range(max_iter):
            H = res(q) - (1 - lt) * r0
            J = np.empty((n, n))
            for j in range(n):
                h = 1e-7 * max(1e-3, abs(q[j]))
                e = np.zeros(n)
                e[j] = h
                J[:, j] = (ob.internal_force(q + e) - ob.internal_force(q - e)) / (2 * h)
            qn = q - np.linalg.solve(J, H)
            hn = np.max(np.abs(res(qn) - (1 - lt) * r0))
            if hn >= best:
                break
            q, best = qn, hn
    return q


def oracle_rel_residual(ob, q, u):
    k = ob.internal_force(q)
    gu = ob.gravity(np.concatenate([q, np.zeros_like(q)])) + u
    return np.max(np.abs(k - gu)) / max(np.max(np.abs(k)), np.max(np.abs(gu)))


TANGENT_BEAMS = {
    "linear": (dict(kind="linear"), False),
    "nonlinear": (dict(kind="nonlinear"), False),
    "corrected": (dict(kind="nonlinear"), True),
    "mixed": (dict(kind=["linear", "nonlinear"] * 4), False),
    "pinned_root": (dict(kind="nonlinear", bcs=["PINNED"] + ["NONE"] * 7), False),
    "interior": (dict(kind="nonlinear", bcs=["FIXED", "NONE", "NONE", "PINNED", "NONE", "FIXED", "NONE", "NONE"]), False),
    "two_waves": (dict(kind="nonlinear", n=100), False),
    "four_waves": (dict(kind=["linear", "nonlinear"] * 100, n=200), False),
}


@pytest.mark.parametrize("name", list(TANGENT_BEAMS))
def test_tangent_matches_finite_differences_of_the_oracle(name):
    kw, corrected = TANGENT_BEAMS[name]
    kw = dict(kw)
    cols = nitinol_columns(kw.pop("n", 8), **kw)
    B = 3
    ens = BeamEnsemble(cols, B, corrected_axial=corrected)
    ob = oracle_beam(cols, corrected_axial=corrected)
    rng = np.random.default_rng(11)
    Q = rng.normal(0.0, 2e-2, (B, ens.n))
    K = ens.tangent_stiffness(Q).cpu().numpy()
    for b in range(B):
        ref = fd_tangent(ob, Q[b])
        # per DOF block of rows and columns, relative to the block's largest entry
        dof = ens.free_index % 3
        for r in range(3):
            for c in range(3):
                sub, subr = K[b][np.ix_(dof == r, dof == c)], ref[np.ix_(dof == r, dof == c)]
                if subr.size == 0:
                    continue
                scale = max(np.max(np.abs(subr)), 1e-9 * np.max(np.abs(ref)))
                assert np.max(np.abs(sub - subr)) / scale <= 1e-6, (name, b, r, c)
    if corrected:
        assert np.max(np.abs(K - K.transpose(0, 2, 1))) <= 1e-12 * np.max(np.abs(K))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_tangent_of_linear_beams_at_zero_is_the_stiffness_matrix(dtype):
    cols = nitinol_columns(12, "linear", bcs=["FIXED", "NONE", "NONE", "PINNED"] + ["NONE"] * 8)
    ens = BeamEnsemble(cols, 4, dtype=dtype)
    K = ens.tangent_stiffness().double().cpu().numpy()
    ref = ens.plan.stiffness()
    tol = 1e-15 if dtype == torch.float64 else 1e-6
    assert np.max(np.abs(K - ref[None])) <= tol * np.max(np.abs(ref))


@pytest.mark.parametrize("name", [str(c) for c in G["g10_static"]["cases"]])
def test_solve_static_matches_the_reference_equilibria(name):
    z = G["g10_static"]
    cols = beam_columns(z, name)
    fp = ForceParams(enable_gravity_effects=True, gravity_vector=list(z[f"{name}/gravity"]))
    ens = BeamEnsemble(cols, 2, force_params=fp)
    u = np.tile(z[f"{name}/u"], (2, 1))
    # (rtol 1e-9: these rods of <= 40 elements reach it; the default is set by 256-element rods)
    sol = ens.solve_static(held_force=u, load_steps=int(z[f"{name}/load_steps"]), rtol=1e-9)
    assert bool(sol.converged.all()), (sol.iterations, sol.residual)
    got = sol.q.cpu().numpy()
    # measured: worst block 3.4e-8 (lin10_tip50, u: |phi| ~ 1.5 there), every nonlinear case <= 1.1e-11
    errs = assert_blocks(got, np.tile(z[f"{name}/q"], (2, 1)), ens.free_index, 1e-7, what=name)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()}, sol.iterations.tolist(), sol.residual.tolist())
    assert torch.equal(ens.state, torch.zeros_like(ens.state)) and ens.time == 0.0   # state untouched


def test_linear_rods_without_gravity_solve_in_one_step():
    cols = nitinol_columns(10, "linear")
    B = 5
    ens = BeamEnsemble(cols, B)
    rng = np.random.default_rng(3)
    U = rng.normal(0.0, 1.0, (B, ens.n))
    sol = ens.solve_static(held_force=U)
    K = ens.plan.stiffness()
    ref = np.linalg.solve(K, U.T).T
    assert int(sol.iterations.max()) <= 2 and bool(sol.converged.all())
    assert np.max(np.abs(sol.q.cpu().numpy() - ref)) <= 1e-10 * np.max(np.abs(ref))


def test_solution_has_zero_acceleration_and_warm_start_takes_no_iteration():
    cols = nitinol_columns(24, "nonlinear")
    B = 8
    ens = BeamEnsemble(cols, B, force_params=GRAV)
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.linspace(0.0, 20.0, B)
    sol = ens.solve_static(held_force=U, rtol=1e-10)
    assert bool(sol.converged.all())
    x = ens.pack_state(torch.cat([sol.q, torch.zeros_like(sol.q)], dim=1))
    acc = ens.unpack_state(ens.rhs_device(x, ens.pack_vec(U)))[:, ens.n:]
    # the load's own acceleration scale: Minv (g + u) at q = 0
    acc0 = ens.unpack_state(ens.rhs_device(torch.zeros_like(x), ens.pack_vec(U)))[:, ens.n:]
    assert float(acc.abs().max()) <= 1e-9 * float(acc0.abs().max())
    again = ens.solve_static(held_force=U, q0=sol.q, rtol=1e-10)
    assert int(again.iterations.max()) <= 1 and bool(again.converged.all())


@pytest.mark.parametrize("n_el", [100, 180])
def test_several_wave_beams_match_an_independent_numpy_newton(n_el):
    # 100 elements: two waves per beam; 180: four
    cols = nitinol_columns(n_el, "nonlinear")
    cols["length"] = np.full(n_el, 1.5 / n_el)
    B = 3
    ens = BeamEnsemble(cols, B, force_params=GRAV)
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.array([1.0, 3.0, 5.0])
    sol = ens.solve_static(held_force=U, rtol=1e-7)
    assert bool(sol.converged.all()), (sol.iterations, sol.residual)
    ob = oracle_beam(cols, enable_gravity=True)
    got = sol.q.cpu().numpy()
    ref = np.array([numpy_newton(ob, U[b]) for b in range(B)])
    errs = assert_blocks(got, ref, ens.free_index, 1e-6, what=f"{n_el} elements")
    print(n_el, {k: f"{v:.1e}" for k, v in errs.items()}, sol.iterations.tolist(), flush=True)


def test_large_ensemble_residual_no_worse_than_numpy_newton():
    n_el, B = 255, 4096   # 256 nodes, 255 carried by threads: one beam per workgroup of four waves
    cols = nitinol_columns(n_el, "nonlinear")
    cols["length"] = np.full(n_el, 1.5 / n_el)
    ens = BeamEnsemble(cols, B, force_params=GRAV)
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.linspace(0.0, 5.0, B)
    sol = ens.solve_static(held_force=U)   # default rtol (1e-6: what every one of these beams reaches)
    assert bool(sol.converged.all()), (int((~sol.converged).sum()), sol.iterations.min())
    ob = oracle_beam(cols, enable_gravity=True)
    Q = sol.q.cpu().numpy()
    pick = [B // 2, B - 1]
    # the sampled loads again to rtol 1e-8 (these tip loads reach it), then against the host's own floor
    tight = BeamEnsemble(cols, len(pick), force_params=GRAV).solve_static(held_force=U[pick], rtol=1e-8)
    assert bool(tight.converged.all()), tight.residual
    for k, b in enumerate(pick):
        q_np = numpy_newton(ob, U[b])   # from q = 0, finite-difference tangent: independent of the GPU
        host = oracle_rel_residual(ob, q_np, U[b])
        gpu_default = oracle_rel_residual(ob, Q[b], U[b])
        gpu = oracle_rel_residual(ob, tight.q[k].cpu().numpy(), U[b])
        print(b, f"gpu(default rtol) {gpu_default:.2e} gpu(1e-8) {gpu:.2e} numpy {host:.2e}", flush=True)
        assert gpu_default <= 1e-6
        assert gpu <= max(host, 1e-8)


def test_residual_floor_above_rtol_terminates_with_minus_one():
    # 255-element rods under gravity cannot reach rtol 1e-9 (their fp64 residual floor is 1e-8 .. 1e-7 at these loads):
    # the increment floor ends every beam with -1 instead of creeping towards that point for ever
    import time

    n_el, B = 255, 4096
    cols = nitinol_columns(n_el, "nonlinear")
    cols["length"] = np.full(n_el, 1.5 / n_el)
    ens = BeamEnsemble(cols, B, force_params=GRAV)
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.linspace(0.0, 5.0, B)
    for rtol in (1e-9, 1e-10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = ens.solve_static(held_force=U, rtol=rtol)
        it = sol.iterations.cpu()
        dt = time.perf_counter() - t0
        assert bool((it == -1).all()), (rtol, it.unique())
        assert dt < 5.0, dt


def test_heterogeneous_ensemble_matches_beams_solved_alone():
    beams = [nitinol_columns(6, "nonlinear"), nitinol_columns(9, "linear"),
             nitinol_columns(7, ["linear", "nonlinear"] * 3 + ["linear"]),
             nitinol_columns(8, "nonlinear", bcs=["FIXED", "NONE", "PINNED"] + ["NONE"] * 5)]
    fps = [GRAV, ForceParams(), GRAV, GRAV]
    ens = BeamEnsemble(beams, len(beams), force_params=fps)
    U = np.zeros((len(beams), ens.n))
    for b in range(len(beams)):
        U[b, int(ens.n_per_beam[b]) - 2] = -3.0
    sol = ens.solve_static(held_force=U)
    assert bool(sol.converged.all())
    for b, cols in enumerate(beams):
        one = BeamEnsemble(cols, 1, force_params=fps[b])
        nb = int(ens.n_per_beam[b])
        s1 = one.solve_static(held_force=U[b:b + 1, :nb])
        ref = s1.q.cpu().numpy()[0]
        got = sol.q.cpu().numpy()[b, :nb]
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref)), b


def test_non_finite_beam_is_isolated():
    cols = nitinol_columns(10, "nonlinear")
    B = 12   # 6 beams of 10 slots per wave: the bad beam shares its wave
    ens = BeamEnsemble(cols, B, force_params=GRAV)
    U = np.zeros((B, ens.n))
    U[:, -2] = -np.linspace(1.0, 10.0, B)
    clean = ens.solve_static(held_force=U)
    U[4, 7] = np.nan
    bad = ens.solve_static(held_force=U)
    assert int(bad.iterations[4]) == -2
    keep = [b for b in range(B) if b != 4]
    assert torch.equal(bad.q[keep], clean.q[keep])
    assert torch.equal(bad.iterations[keep], clean.iterations[keep])


def test_refusals():
    cols = nitinol_columns(6, "nonlinear")
    with pytest.raises(nat.NativeError, match="fp64"):
        BeamEnsemble(cols, 2, dtype=torch.float32).solve_static()
    ens = BeamEnsemble(cols, 2)
    with pytest.raises(nat.NativeError, match="impulse"):
        import ctypes as C

        desc, keep = ens._input_desc(impulse_amp=np.ones(2))
        iters = torch.empty(2, dtype=torch.int32, device=ens.device)
        nat.check(ens._lib.crb_solve_static(ens.plan.h, ens._ptr(ens.state.clone()), C.byref(desc), 8, 20, 1e-9, 0.0,
                                            ens._ptr(iters), None, ens._stream()))
    with pytest.raises(nat.NativeError, match="FIXED or PINNED"):
        BeamEnsemble(nitinol_columns(6, "nonlinear", bcs=["NONE"] * 6), 2).solve_static()
    with pytest.raises(nat.NativeError, match="load_steps"):
        ens.solve_static(load_steps=0)
    with pytest.raises(nat.NativeError, match="max_iter"):
        ens.solve_static(max_iter=1001)
    long_ = BeamEnsemble(nitinol_columns(300, "linear"), 1)
    with pytest.raises(nat.NativeError, match="256 thread-carried"):
        long_.solve_static()
    with pytest.raises(nat.NativeError, match="256 thread-carried"):
        long_.tangent_stiffness()
