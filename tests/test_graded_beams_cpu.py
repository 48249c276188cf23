"""CPU side of the graded-beam tests (tests/test_graded_beams.py holds the GPU side and imports the case table from here).

Every other beam of more than 7 elements in this suite has equal elements, so a per-slot table read one slot off, or a
reduction level never reached, stays invisible.  Here:
  1. the layout of host plans (Plan(..., device=-1), no GPU) of beams that vary along the span: slots, beams per wave, threads
     and the reduction levels that pick_levels keeps, fp64 and fp32 -- tapered rods land one level above every uniform rod;
  2. the C oracle against the REFERENCE on such beams (tests/golden/g11_graded.npz, make_golden_graded.py), at the bounds
     test_oracle_golden.py holds for the goldens of equal elements: k(q) 1e-12 (g2), RHS 1e-10 per block (g34), the RK4
     rollout 1e-11 per block (g5);
  3. the inputs of the GPU cases on the oracle: every rollout finite, and the oracle's own response to a 4-ulp change of the
     impulse (helpers.rollout_conditioning) below 1e-13 in every block, so the fixed bounds of the GPU file are owed to
     nobody's conditioning."""
import numpy as np
import pytest

from tests.helpers import (GRADED_FAMILIES, assert_blocks, beam_columns, force_kwargs, graded_columns, nitinol_columns,
                           oracle_beam, rel_err, rollout_conditioning)

DT = 2e-5
DT_MESH = 5e-6      # mesh4's shortest element is half the uniform rod's: at 2e-5 its rate grows to 94 within 40 steps
STEPS = 40
FP32_STEPS = 200    # the horizon of FP32_TOL (test_gpu_parity.py: test_fp32_plan_tracks_fp64_within_measured_drift)
FP32_CASES = ["packed20_taper3", "wave64_taper3", "wave64_step", "waves2_100_taper3", "waves2_128_taper10", "waves4_200_taper10",
              "waves4_200_taper30", "waves4_256_taper30"]
AMPS = 0.05 * (1.0 + np.arange(8))
DRAG = dict(fluid_density=1000.0, enable_fluid=True)
GRAV = dict(enable_gravity=True)
BOTH = dict(DRAG, **GRAV)


def pinned_root(n):
    return ["PINNED"] + ["NONE"] * (n - 1)


def mixed(n):
    return (["linear", "nonlinear"] * n)[:n]


# One table for both files.  layout = (n_slots, beams_per_group, threads, pcr_levels, pcr_levels_full) of the fp64 plan,
# lv32 = pcr_levels of the fp32 plan (same slots and threads).  mid = the node of the mid-span impulse: next to a wave seam
# (slots 63 / 64, 127 / 128, 191 / 192) where the beam has one, next to the beam seam of a packed wave otherwise.  The level
# count picks the kernel instance: lean_step_built / lean_stage_built / lean_rk45_built (levels, log2 waves).
CASES = {
    # packed: 3 beams per wave, B = 5 leaves the last group partly filled; 5 levels
    "packed20_taper3": dict(n=20, family="taper3", kind="nonlinear", B=5, mid=10, layout=(20, 3, 64, 5, 5), lv32=5),
    "packed31_taper3": dict(n=31, family="taper3", kind=mixed(31), B=5, mid=30, layout=(31, 2, 64, 5, 5), lv32=5),
    # one wave: 6 levels (5 in fp32) on the tapers, 5 (4 in fp32) on the material step
    "wave40_taper3": dict(n=40, family="taper3", kind="nonlinear", B=3, mid=20, layout=(40, 1, 64, 6, 6), lv32=5),
    "wave64_taper3": dict(n=64, family="taper3", kind="nonlinear", B=3, mid=32, layout=(64, 1, 64, 6, 6), lv32=5),
    "wave64_step": dict(n=64, family="step", kind=mixed(64), B=3, mid=32, layout=(64, 1, 64, 5, 6), lv32=4),
    "wave64_pinned_taper10": dict(n=63, family="taper10", kind="nonlinear", bcs=pinned_root(63), B=3, mid=31,
                                  layout=(64, 1, 64, 6, 6), lv32=5),          # PINNED root, 64 slots: off = 0
    # two waves: seam at slots 63 / 64
    "waves2_100_taper3": dict(n=100, family="taper3", kind="nonlinear", B=3, mid=64, layout=(100, 1, 128, 6, 7), lv32=4),
    "waves2_100_taper10": dict(n=100, family="taper10", kind=mixed(100), B=3, mid=65, layout=(100, 1, 128, 6, 7), lv32=5),
    "waves2_100_allcols": dict(n=100, family="allcols", kind="nonlinear", B=3, mid=64, layout=(100, 1, 128, 5, 7), lv32=4),
    "waves2_128_taper10": dict(n=128, family="taper10", kind="nonlinear", B=3, mid=64, layout=(128, 1, 128, 6, 7), lv32=5),
    "waves2_128_step": dict(n=128, family="step", kind="nonlinear", B=3, mid=64, layout=(128, 1, 128, 5, 7), lv32=4),
    # four waves: seams at 63 / 64, 127 / 128, 191 / 192
    "waves4_200_taper10": dict(n=200, family="taper10", kind="nonlinear", B=2, mid=128, layout=(200, 1, 256, 6, 8), lv32=4),
    "waves4_200_taper30": dict(n=200, family="taper30", kind=mixed(200), B=2, mid=192, layout=(200, 1, 256, 6, 8), lv32=5),
    "waves4_200_mesh4": dict(n=200, family="mesh4", kind="nonlinear", B=2, mid=128, dt=DT_MESH, layout=(200, 1, 256, 5, 8),
                             lv32=4),
    "waves4_256_taper30": dict(n=256, family="taper30", kind="nonlinear", B=2, mid=192, layout=(256, 1, 256, 6, 8), lv32=4),
    "waves4_256_taper10": dict(n=256, family="taper10", kind="nonlinear", B=2, mid=128, layout=(256, 1, 256, 5, 8), lv32=4),
    "waves4_256_pinned_taper30": dict(n=255, family="taper30", kind="nonlinear", bcs=pinned_root(255), B=2, mid=127,
                                      layout=(256, 1, 256, 6, 8), lv32=4),    # PINNED root, 256 slots
}


def case_columns(name):
    c = CASES[name]
    return graded_columns(c["n"], c["kind"], c["family"], bcs=c.get("bcs"))


def case_dt(name):
    return CASES[name].get("dt", DT)


def reduced_index(ob, node, dof):
    """the reduced index of (node, dof: 0 u / 1 w / 2 phi) of an oracle beam"""
    hit = np.nonzero(ob.red2full() == 3 * node + dof)[0]
    assert hit.size == 1, (node, dof)
    return int(hit[0])


def seeded_gain(ob, rng):
    """a dense gain of the uniform-rod tests' size (N(0, 2e-2)), row i scaled by M_ii / max M_ii: the thin end of a tapered
    rod carries 1 / 900 of the root's inertia, and an unscaled row would drive it at a rate RK4 does not integrate"""
    m = np.diag(ob.mass())
    return rng.normal(0.0, 2e-2, (ob.n, 2 * ob.n)) * (m / m.max())[:, None]


def closed_loop_gain(ob, rng, kp=200.0, kd=2.0):
    """u = -kp q - kd v (test_controlled_closed_loop_large.py:pd_gain, stabilising), every row scaled by its share of the
    inertia as in seeded_gain, plus that dense seeded gain: every entry is read, the diagonal keeps the loop stable"""
    m = np.diag(ob.mass())
    return np.hstack([kp * np.eye(ob.n), kd * np.eye(ob.n)]) * (m / m.max())[:, None] + seeded_gain(ob, rng)


def host_plan(cols, dtype, **kw):
    from continuum_robot import _native as nat

    return nat.Plan(cols, n_beams=5, device=-1, dtype=dtype, **kw)


def layout_of(p):
    return (p.n_slots, p.beams_per_group, p.threads, p.pcr_levels, p.pcr_levels_full)


# ---- 1. the layout table
@pytest.mark.parametrize("name", list(CASES))
def test_case_layouts_on_host_plans(name):
    c = CASES[name]
    cols = case_columns(name)
    for kw in (dict(), BOTH):     # (the forces do not move the layout)
        p64, p32 = host_plan(cols, "f64", **kw), host_plan(cols, "f32", **kw)
        assert layout_of(p64) == c["layout"], (name, layout_of(p64))
        assert layout_of(p32)[:3] == c["layout"][:3] and p32.pcr_levels == c["lv32"], (name, layout_of(p32))
        assert p32.pcr_levels_full == c["layout"][4]
    assert 0 < c["mid"] < c["n"]


# radius taper r0 -> r0 / ratio, L = 0.25: (elements) -> (fp64 levels used, full, fp32 used).  Uniform Nitinol rods of 40 to 256
# elements keep 5 levels in fp64 and 4 in fp32.
TAPER_LEVELS = {
    ("taper3", 20): (5, 5, 5), ("taper3", 31): (5, 5, 5), ("taper3", 40): (6, 6, 5), ("taper3", 64): (6, 6, 5),
    ("taper3", 100): (6, 7, 4), ("taper10", 100): (6, 7, 5), ("taper10", 128): (6, 7, 5), ("taper10", 200): (6, 8, 4),
    ("taper30", 200): (6, 8, 5), ("taper30", 256): (6, 8, 4), ("taper10", 256): (5, 8, 4),
}


@pytest.mark.parametrize("family,n", list(TAPER_LEVELS))
def test_tapered_rods_keep_one_level_more_than_uniform_rods(family, n):
    want = TAPER_LEVELS[(family, n)]
    cols = graded_columns(n, "nonlinear", family)
    p64, p32 = host_plan(cols, "f64"), host_plan(cols, "f32")
    assert (p64.pcr_levels, p64.pcr_levels_full, p32.pcr_levels) == want
    packed = {20: 3, 31: 2}.get(n, 1)
    assert p64.beams_per_group == packed and p64.n_slots == n and p64.threads == (64 if n <= 64 else 128 if n <= 128 else 256)
    if n >= 40:
        u64, u32 = host_plan(nitinol_columns(n, "nonlinear"), "f64"), host_plan(nitinol_columns(n, "nonlinear"), "f32")
        assert (u64.pcr_levels, u32.pcr_levels) == (5, 4)


def test_no_graded_family_reaches_seven_levels():
    """the instances of 7 levels and more are not built: no family of graded_columns asks for one"""
    for family in GRADED_FAMILIES:
        for n in (40, 64, 100, 128, 200, 256):
            if family == "nearly_uniform" and n <= 100:      # (it lengthens element 100)
                with pytest.raises(AssertionError, match="more than 100 elements"):
                    graded_columns(n, "nonlinear", family)
                continue
            assert host_plan(graded_columns(n, "nonlinear", family), "f64").pcr_levels <= 6, (family, n)


def test_graded_columns_families():
    for n in (20, 100, 256):
        t = graded_columns(n, "linear", "taper10")
        assert np.isclose(t["cross_area"][0] / t["cross_area"][-1], 100.0) and np.all(np.diff(t["moment_inertia"]) < 0)
        assert np.allclose(t["wetted_area"], 2 * np.pi * np.sqrt(t["cross_area"] / np.pi) * 0.25)
        m = graded_columns(n, "linear", "mesh4")
        assert np.isclose(m["length"][-1] / m["length"][0], 4.0) and np.isclose(m["length"][0], 0.125)
        a = graded_columns(n, mixed(n), "allcols")
        for c in ("length", "cross_area", "moment_inertia", "wetted_area", "drag_coef"):
            assert np.all(np.diff(a[c]) != 0.0), c
        # (cos(2 pi j / 5) repeats between j = 2 and 3 of every five: the density differs from one neighbour at least)
        d = np.diff(a["density"]) != 0.0
        assert np.all(d[:-1] | d[1:]) and np.ptp(a["density"]) > 0.3 * 6450.0
        assert list(a["type"][:2]) == ["linear", "nonlinear"]
    s = graded_columns(128, "nonlinear", "step")
    assert s["density"][63] == 6450.0 and s["density"][64] == 645.0 and s["elastic_modulus"][64] == 7.5e9
    u, nu = nitinol_columns(256, "nonlinear"), graded_columns(256, "nonlinear", "nearly_uniform")
    diff = [c for c in u if not np.array_equal(u[c], nu[c])]
    assert diff == ["length"] and np.flatnonzero(u["length"] != nu["length"]).tolist() == [100]


# ---- 2. the oracle against the reference on graded beams
def _g11(golden):
    return golden["g11_graded"]


@pytest.mark.parametrize("name", ["taper10_40_nl_drag", "taper10_100_mixed_grav", "taper10_256_nl_drag", "allcols_40_mixed_both",
                                  "allcols_100_nl_drag", "allcols_256_lin_grav"])
def test_g11_oracle_matches_the_reference_on_graded_beams(golden, name):
    z = _g11(golden)
    assert name in [str(c) for c in z["cases"]]
    cols = beam_columns(z, name)
    ob = oracle_beam(cols, **force_kwargs(z, name))
    n = ob.n
    family, n_e = name.split("_")[0], int(name.split("_")[1])
    X, u = z[f"{name}/x"], z[f"{name}/u"]
    assert X.shape == (1 if n_e == 256 else 2, 2 * n)
    # the stored columns are graded_columns' own (as the reference's CSV parser read them: within a few ulp)
    mine = graded_columns(n_e, list(cols["type"]), family)
    for c in ("length", "elastic_modulus", "moment_inertia", "density", "cross_area", "wetted_area", "drag_coef"):
        assert np.allclose(cols[c], mine[c], rtol=1e-12, atol=0), c
    for i, x in enumerate(X):
        assert rel_err(ob.internal_force(x[:n]), z[f"{name}/k_q"][i]) < 1e-12, i                 # g2's bound for k(q)
        assert_blocks(ob.rhs(x, u), z[f"{name}/xdot"][i], ob.red2full(), 1e-10, what=(name, i))   # g34's for the RHS
    steps, dt = int(z["steps"]), float(z["dt"])
    xT = ob.rk4_impulse(X[-1], dt, steps, float(z["amp"]), float(z["duration"]), -2)
    assert_blocks(xT, z[f"{name}/x_end"], ob.red2full(), 1e-11, what=name)                       # g5's for the rollout
    assert abs(xT[n - 2] - z[f"{name}/x_end"][n - 2]) <= 1e-12 * abs(z[f"{name}/x_end"][n - 2])


# ---- 3. the GPU cases' inputs on the oracle: finite, and conditioned far below the bounds
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_case_inputs_are_finite_and_well_conditioned(name):
    c = CASES[name]
    cols, dt = case_columns(name), case_dt(name)
    worst = 0.0
    for kw in (DRAG, GRAV, BOTH):
        ob = oracle_beam(cols, **kw)
        for idx in (-2, reduced_index(ob, c["mid"], 1)):
            x = ob.rk4_impulse(np.zeros(2 * ob.n), dt, STEPS, AMPS[c["B"] - 1], idx=idx)
            assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0.0, (name, kw, idx)
            cond = rollout_conditioning(ob, np.zeros(2 * ob.n), dt, STEPS, AMPS[c["B"] - 1], idx=idx)
            worst = max(worst, max(cond.values()))
            assert max(cond.values()) < 1e-13, (name, kw, idx, cond)
    print(name, f"worst block conditioning {worst:.1e}")


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_case_inputs_are_finite_and_well_conditioned(name):
    """the 200-step rollouts of the fp32 cases (nonlinear elements, drag, tip impulse) on the oracle"""
    c = CASES[name]
    ob = oracle_beam(graded_columns(c["n"], "nonlinear", c["family"]), **DRAG)
    for amp in (0.1, 0.2):
        x = ob.rk4_impulse(np.zeros(2 * ob.n), DT, FP32_STEPS, amp)
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0.0
        cond = rollout_conditioning(ob, np.zeros(2 * ob.n), DT, FP32_STEPS, amp)
        print(name, f"worst block conditioning over {FP32_STEPS} steps {max(cond.values()):.1e}")
        assert max(cond.values()) < 1e-13, (name, amp, cond)


@pytest.mark.parametrize("name", ["wave40_taper3", "wave64_taper3"])
def test_closed_loop_gain_is_integrable_at_the_controllers_rungs(name):
    """the controlled closed loop of the GPU file on the oracle: finite over the 3 ms at 64, 128 and 256 steps per ms"""
    c = CASES[name]
    ob = oracle_beam(case_columns(name), **DRAG)
    K = closed_loop_gain(ob, np.random.default_rng(850 + c["n"]))
    for m in (64, 128, 256):
        x = ob.rk4_feedback(np.zeros(2 * ob.n), 1e-3 / m, 3 * m, K, amp=AMPS[c["B"] - 1], duration=1.5e-3)
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0.0, (name, m)
