"""BeamEnsemble -- B independent beams of one topology stepped on an MI355X.

This is the batched entry point of the drop-in: it owns the state tensor
``[B, 2, n_node, 4]`` on the GPU (PyTorch-ROCm memory) and calls the HIP kernels of libcrbeam.so
through the C ABI (include/crbeam.h).  The planning / control layers hold one ensemble per robot
model and roll it out; nothing here runs on the CPU -- without the extension or a GPU every
operation raises.

Reference interfaces mirrored (file:line under /root/reference/src/continuum_robot/models/):
  constructor arguments   dynamic_beam_model.py:25-29 (CSV schema :78-90, ForceParams)
  rhs()                   get_dynamic_system()(t, x, u), dynamic_beam_model.py:343-362
  internal_force()        get_stiffness_function(), euler_bernoulli_beam.py:364-368
  step()                  the scipy.solve_ivp call sites (examples/example_utilities.py:153-159)
"""
import ctypes as C
import pathlib
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .models.force_params import ForceParams

_CSV_REQUIRED = ["length", "elastic_modulus", "moment_inertia", "density", "cross_area", "type", "boundary_condition"]
_PARAM = {"u": 0, "w": 1, "phi": 2}

# Default relative tolerance of solve_static (profiles/exp_static.py), measured on 4096 255-element nonlinear
# rods under gravity and tip loads of 0 .. 5 N: at 1e-7, 20 of them (the lightest loads) stay above their fp64 residual
# floor; at 1e-6 every beam converges.  Shorter rods reach far less: ~1e-9 at 64 elements, ~1e-12 at 10.
STATIC_RTOL = 1e-6


class ControlSchedule(NamedTuple):
    """A piecewise-constant control sequence for the RK4 rollout family (crb_input_schedule): ``control`` reduced [K, B, n],
    vector k held for RK4 steps k * hold .. (k + 1) * hold - 1 of the call.  ``step``, ``step_adjoint_params`` and ``rollout``
    take it as ``control=`` / ``control_hold=``; every method of the family -- ``step_tangent`` and ``step_adjoint`` this way
    only -- takes it in place of a held force, ``held_force=ControlSchedule(U, hold)``.  The implicit family takes it too
    (``step_implicit`` and ``rollout_implicit`` both ways, ``step_implicit_adjoint`` in place of a held force); ``hold`` then
    counts implicit steps."""
    control: object
    hold: int


class StaticSolution(NamedTuple):
    """Result of BeamEnsemble.solve_static: reduced positions [B, n], and per beam whether it converged, the Newton
    iterations it used (-1 not converged, -2 non-finite) and its final scaled residual."""
    q: torch.Tensor
    converged: torch.Tensor
    iterations: torch.Tensor
    residual: torch.Tensor


def _columns(parameters, need_fluid):
    if isinstance(parameters, (str, pathlib.Path)):
        parameters = pd.read_csv(parameters)  # FileNotFoundError propagates, as in the reference (:46)
    if isinstance(parameters, pd.DataFrame):
        cols = {c: parameters[c].to_numpy() for c in parameters.columns}
    elif isinstance(parameters, dict):
        cols = dict(parameters)
    else:
        raise TypeError("Parameters must be filepath, pandas DataFrame or a dict of columns")
    required = _CSV_REQUIRED + (["wetted_area", "drag_coef"] if need_fluid else [])
    if not all(c in cols for c in required):
        raise ValueError(f"CSV must contain columns: {', '.join(required)}")
    bad = set(str(b) for b in cols["boundary_condition"]) - {"FIXED", "PINNED", "NONE"}
    if bad:
        raise ValueError(f"Invalid boundary conditions: {bad}")
    return cols


class _NoContext:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_CONTEXT = _NoContext()


class _FusedForce:
    """Marker for a built-in force that the RHS kernel evaluates itself (drag: fluid_forces.py:103-142, gravity:
    gravity_forces.py:66-148).  It sits in the ensemble's registry like the reference's auto-registered force
    objects (dynamic_beam_model.py:220-241); switching ``enabled`` off takes effect at the next call, because the
    registry is re-read on every call (force_registry.py:66-67)."""

    def __init__(self, kind: str):
        self.kind = kind
        self.enabled = True

    def is_enabled(self) -> bool:
        return self.enabled

    def compute_forces(self, x, t):
        raise RuntimeError(f"the built-in {self.kind} force is evaluated inside the RHS kernel, not on the host")


class BatchedForceRegistry:
    """ForceRegistry of an ensemble (reference: models/force_registry.py:6-88, same methods and semantics): force
    components whose ``compute_forces(x, t)`` maps the reduced states ``x[B, 2n]`` (a torch tensor on the ensemble's
    device) to generalised forces ``[B, n]``.  ``register`` ignores a component that is disabled at that moment
    (:20-21); the aggregate re-checks ``is_enabled()`` on every call (:66-67); ``get_registered_forces`` returns a copy."""

    def __init__(self):
        self._forces = []

    def register(self, force_instance) -> None:
        if force_instance.is_enabled():
            self._forces.append(force_instance)

    def unregister(self, force_instance) -> bool:
        if force_instance in self._forces:
            self._forces.remove(force_instance)
            return True
        return False

    def clear(self) -> None:
        self._forces.clear()

    def get_registered_forces(self):
        return self._forces.copy()

    def __len__(self) -> int:
        return len(self._forces)

    def __contains__(self, force_instance) -> bool:
        return force_instance in self._forces


class BeamEnsemble:
    """B independent beams stepped together on one GPU.

    ``parameters``: one parameter set (CSV path / DataFrame / dict of columns) shared by all ``n_beams`` beams, or a
    list of ``n_beams`` of them -- a heterogeneous ensemble (SURVEY f-3): every beam has its own element columns and
    types and may have its own element COUNT and boundary-condition column.  ``force_params`` is then one
    ``ForceParams`` for all beams or a list of ``n_beams`` (what examples/beam_comparison_fluid.py:49-83 runs as six
    processes -- three beams without, three with fluid -- is ONE ensemble here).

    Reduced vectors ([q_red ; v_red], the reference's state ordering) are ``[B, 2 n]``.  When the beams' free-DOF
    sets differ (``mixed_topology``), ``n`` is the largest beam's and beam b uses the first ``n_per_beam[b]`` entries
    of each half (the rest is ignored on input and zero on output); ``beam_state(b)`` / ``pad_states`` convert."""

    def __init__(self, parameters, n_beams: int, force_params=None, dtype=torch.float64,
                 device: Union[str, torch.device, int] = "cuda", corrected_axial: bool = False, node_bc=None):
        per_beam_fp = isinstance(force_params, (list, tuple))
        if per_beam_fp:
            if not isinstance(parameters, (list, tuple)):
                parameters = [parameters] * n_beams      # one beam description, per-beam ForceParams
            if len(force_params) != n_beams:
                raise ValueError("a list of ForceParams must have n_beams entries")
            self.force_params = [fp or ForceParams() for fp in force_params]
        else:
            self.force_params = force_params or ForceParams()
        fp_of = (lambda b: self.force_params[b]) if per_beam_fp else (lambda b: self.force_params)
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype must be torch.float64 or torch.float32")
        nat.load()  # raises if the extension was not built
        if not torch.cuda.is_available():
            raise RuntimeError("BeamEnsemble needs a HIP device: the beam stepper has no CPU path")
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type != "cuda":
            raise RuntimeError("BeamEnsemble needs a HIP device: the beam stepper has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._device_index = int(self.device.index)
        self.dtype = dtype
        if isinstance(parameters, (list, tuple)):
            # heterogeneous ensemble: one parameter set per beam
            if len(parameters) != n_beams:
                raise ValueError("a list of parameter sets must have n_beams entries")
            self.columns = [_columns(p, fp_of(b).enable_fluid_effects) for b, p in enumerate(parameters)]
        else:
            self.columns = _columns(parameters, fp_of(0).enable_fluid_effects)
        fps = [fp_of(b) for b in range(n_beams)] if per_beam_fp else None
        with torch.cuda.device(self.device):    # (plan creation selects the plan's device: keep the caller's current one)
            self.plan = nat.Plan(
                self.columns, n_beams=n_beams, node_bc=node_bc,
                fluid_density=[f.fluid_density for f in fps] if fps else fp_of(0).fluid_density,
                enable_fluid=[f.enable_fluid_effects for f in fps] if fps else fp_of(0).enable_fluid_effects,
                gravity=[f.get_gravity_vector() for f in fps] if fps else fp_of(0).get_gravity_vector(),
                enable_gravity=[f.enable_gravity_effects for f in fps] if fps else fp_of(0).enable_gravity_effects,
                corrected_axial=corrected_axial, dtype="f64" if dtype == torch.float64 else "f32", device=self.device.index)
        p = self.plan
        self.n_beams, self.n_elem, self.n_node, self.n = n_beams, p.n_elem, p.n_node, p.n_free
        self.mixed_topology = p.mixed_topology
        self.free_index = p.free_index.copy()                 # beam 0's (every beam's unless mixed_topology)
        if self.mixed_topology:
            self.free_index_per_beam = [p.beam_free_index(b) for b in range(n_beams)]
            self.n_per_beam = np.array([fi.size for fi in self.free_index_per_beam])
        else:
            self.free_index_per_beam = [self.free_index] * n_beams
            self.n_per_beam = np.full(n_beams, self.n)
        # (element counts can differ with ONE free-DOF set: a longer beam whose extra nodes are all FIXED)
        self.n_elem_per_beam = (np.array([p.beam_info(b)[0] for b in range(n_beams)]) if p.per_beam
                                else np.full(n_beams, self.n_elem))
        self.state = torch.zeros((n_beams, 2, self.n_node, 4), dtype=dtype, device=self.device)
        self.time = 0.0
        self.static_status = None   # int32 [B] of the last static_jvp / static_vjp: 0, or -2 (non-finite sensitivity)
        self._lib = nat.load()
        # functional composition (step_composed): the built-in forces appear in the registry as markers, user forces
        # are torch callables; plans with a built-in force switched off are created on demand
        self._plan_args = dict(n_beams=n_beams, node_bc=node_bc, corrected_axial=corrected_axial,
                               dtype="f64" if dtype == torch.float64 else "f32", device=self.device.index)
        self._fps = fps if fps else [fp_of(0)]
        self._plans = {}
        self.force_registry = BatchedForceRegistry()
        self._auto_drag = self._auto_gravity = None
        if any(f.enable_fluid_effects for f in self._fps):
            self._auto_drag = _FusedForce("drag")
            self.force_registry.register(self._auto_drag)
        if any(f.enable_gravity_effects for f in self._fps):
            self._auto_gravity = _FusedForce("gravity")
            self.force_registry.register(self._auto_gravity)
        self._plans[(self._auto_drag is not None, self._auto_gravity is not None)] = self.plan

    @classmethod
    def from_dataframes(cls, frames: Sequence, force_params=None, **kwargs):
        """One beam per entry of ``frames`` (DataFrames, CSV paths or column dicts -- the reference's beam files,
        euler_bernoulli_beam.py:26-109; boundary conditions from each file's own column,
        dynamic_beam_model.py:205-218), ``force_params`` one ForceParams or one per beam."""
        frames = list(frames)
        return cls(frames, len(frames), force_params=force_params, **kwargs)

    # ------------------------------------------------------------------ ragged reduced vectors (mixed_topology)
    def pad_states(self, states: Sequence) -> np.ndarray:
        """per-beam reference state vectors [2 n_b] -> the ensemble's [B, 2 n] layout ([q_b, 0.. ; v_b, 0..])"""
        if len(states) != self.n_beams:
            raise ValueError("expected one state vector per beam")
        out = np.zeros((self.n_beams, 2 * self.n))
        for b, x in enumerate(states):
            nb = int(self.n_per_beam[b])
            x = np.asarray(x, dtype=np.float64)
            if x.shape != (2 * nb,):
                raise ValueError(f"beam {b}: expected a state of {2 * nb} entries, got {x.shape}")
            out[b, :nb] = x[:nb]
            out[b, self.n:self.n + nb] = x[nb:]
        return out

    def beam_state(self, b: int, x_red=None) -> np.ndarray:
        """the reference's state vector [q_red ; v_red] of beam ``b`` (host array of 2 n_b entries)"""
        x = self.unpack_state() if x_red is None else x_red
        row = x[b].detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x[b])
        nb = int(self.n_per_beam[b])
        return np.concatenate([row[:nb], row[self.n:self.n + nb]])

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self):
        """Context in which the library calls run: the plan's device current.  The library selects it itself
        (hipSetDevice); when it already is the current one there is nothing to restore afterwards, and the call path of
        a short launch saves the context manager's two device switches."""
        if torch.cuda.current_device() == self._device_index:
            return _NO_CONTEXT
        return torch.cuda.device(self.device)

    def _dev(self, a, shape=None):
        t = torch.as_tensor(a, dtype=self.dtype, device=self.device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    @staticmethod
    def _ref(struct):
        """an optional descriptor struct of a library call by reference (None = NULL)"""
        return C.byref(struct) if struct is not None else None

    def reduced_index(self, node: int, param: str, beam: int = 0) -> int:
        """Reduced position index of (node, 'u'|'w'|'phi') in beam ``beam``; KeyError when constrained or absent
        (reference: EulerBernoulliBeam.get_dof_index, euler_bernoulli_beam.py:404-420)."""
        full = 3 * node + _PARAM[param]
        hit = np.nonzero(self.free_index_per_beam[beam] == full)[0]
        if node < 0 or node >= self.n_node or hit.size == 0:
            raise KeyError(f"Invalid node/parameter combination: ({node}, {param})")
        return int(hit[0])

    # ------------------------------------------------------------------ layout conversion
    def pack_state(self, x_red) -> torch.Tensor:
        """reduced [B, 2n] (reference ordering [q_red ; v_red]) -> device layout [B, 2, n_node, 4]"""
        x_red = self._dev(x_red, (self.n_beams, 2 * self.n))
        out = torch.empty_like(self.state)
        with self._on_device():
            nat.check(self._lib.crb_pack_state(self.plan.h, self._ptr(x_red), self._ptr(out), self._stream()))
        return out

    def unpack_state(self, x=None, out=None) -> torch.Tensor:
        """Device layout -> the reference's reduced ordering [B, 2n]; ``out``: a contiguous [B, 2n] tensor to write into (e.g.
        this rank's slot of an all-gather's result)."""
        x = self.state if x is None else x
        if out is None:
            out = torch.empty((self.n_beams, 2 * self.n), dtype=self.dtype, device=self.device)
        elif tuple(out.shape) != (self.n_beams, 2 * self.n) or out.dtype != self.dtype or not out.is_contiguous():
            raise ValueError("unpack_state: out must be a contiguous [n_beams, 2n] tensor of the ensemble's dtype")
        with self._on_device():
            nat.check(self._lib.crb_unpack_state(self.plan.h, self._ptr(x), self._ptr(out), self._stream()))
        return out

    def pack_vec(self, v_red) -> torch.Tensor:
        v_red = self._dev(v_red, (self.n_beams, self.n))
        out = torch.empty((self.n_beams, self.n_node, 4), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_pack_vec(self.plan.h, self._ptr(v_red), self._ptr(out), self._stream()))
        return out

    def unpack_vec(self, v) -> torch.Tensor:
        out = torch.empty((self.n_beams, self.n), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_unpack_vec(self.plan.h, self._ptr(v), self._ptr(out), self._stream()))
        return out

    def unpack_snapshots(self, snaps: torch.Tensor) -> torch.Tensor:
        """[n_rec, B, 2, n_node, 4] snapshots of step(..., record="all") -> reduced [n_rec, B, 2n] (sol.y ordering)."""
        return torch.stack([self.unpack_state(snaps[k]) for k in range(snaps.shape[0])])

    def beam_shapes(self, snaps: torch.Tensor, dx: float, as_reference: bool = True):
        """Beam x, y coordinates over time from whole-state snapshots (``step(..., record="all")`` /
        ``solve_rk45(record="all")`` / ``step_implicit(record="all")``), the reference's
        ``extract_beam_shapes(sol, n_segments, dx)`` (examples/example_utilities.py:173-205) for every beam:
        x[t, b, j] = j * dx, y[t, b, 0] = 0 (fixed base), y[t, b, j + 1] = pos[j].

        ``as_reference=True`` reproduces the reference's indexing ``pos = sol.y[n_pos + 1::3]`` -- entries of the
        VELOCITY half of the state (the transverse RATES dw/dt of the free nodes, not the
        displacements); ``False`` reads the transverse displacements ``sol.y[1:n_pos:3]`` the docstring there means.
        Returns numpy arrays of shape [n_t, B, n_elem + 1]."""
        red = self.unpack_snapshots(snaps).detach().cpu().numpy()        # [n_t, B, 2n]: sol.y per beam, transposed
        n_t, n_pts = red.shape[0], self.n_elem + 1
        x = np.broadcast_to(np.arange(n_pts) * float(dx), (n_t, self.n_beams, n_pts)).copy()
        y = np.zeros((n_t, self.n_beams, n_pts))
        pos = red[:, :, self.n + 1::3] if as_reference else red[:, :, 1:self.n:3]
        m = min(pos.shape[2], self.n_elem)
        y[:, :, 1:1 + m] = pos[:, :, :m]
        return x, y

    def set_state(self, x_red, time: float = 0.0) -> None:
        self.state = self.pack_state(x_red)
        self.time = float(time)
        self.reset_status()

    def zero_state(self) -> None:
        self.state.zero_()
        self.time = 0.0
        self.reset_status()

    # ------------------------------------------------------------------ per-beam status
    @property
    def status(self) -> torch.Tensor:
        """int32 [B]: 0 while a beam's state is finite, else the number of steps the ensemble had taken at the END of the launch
        in which the beam went non-finite (fixed-step steppers: step, step_implicit, step_feedback, step_composed's stages).
        The first access switches the reporting on; `set_state` / `zero_state` / `reset_status` start it afresh.  The
        reference's solve_ivp just returns NaN rows when its shipped nonlinear element (segments.py:178-208) diverges."""
        if getattr(self, "_status", None) is None:
            self._status = torch.zeros((self.n_beams,), dtype=torch.int32, device=self.device)
            with self._on_device():
                nat.check(self._lib.crb_plan_set_status(self.plan.h, self._ptr(self._status), 0))
        return self._status

    def reset_status(self) -> None:
        if getattr(self, "_status", None) is not None:
            self._status.zero_()
            with self._on_device():
                nat.check(self._lib.crb_plan_set_status(self.plan.h, self._ptr(self._status), 0))

    def _input_desc(self, impulse_amp=None, impulse_duration=0.01, impulse_index=-2, held_force=None):
        """The crb_input_desc of a call and the device buffers it points to (they must outlive the asynchronous launch):
        amplitudes [B] on reduced position index ``impulse_index`` of EVERY beam (-2 = each beam's own tip w,
        example_utilities.py:147) while t < impulse_duration, and the reduced [B, n] ``held_force``."""
        desc, keep = nat.InputDesc(), []
        desc.kind = nat.CRB_INPUT_NONE
        if impulse_amp is not None:
            amp = self._dev(impulse_amp, (self.n_beams,))
            nodes, dofs = [], []
            for b in (range(self.n_beams) if self.mixed_topology else (0,)):
                fi = self.free_index_per_beam[b]
                idx = impulse_index if impulse_index >= 0 else fi.size + impulse_index
                if not 0 <= idx < fi.size:
                    raise IndexError("impulse_index out of range")
                nodes.append(int(fi[idx]) // 3)
                dofs.append(int(fi[idx]) % 3)
            if len(set(dofs)) != 1:
                raise ValueError("impulse_index addresses different DOF kinds (u / w / phi) in different beams")
            desc.kind, desc.node, desc.dof = nat.CRB_INPUT_IMPULSE, nodes[0], dofs[0]
            desc.duration = float(impulse_duration)
            desc.amp = amp.data_ptr()
            keep.append(amp)
            if len(set(nodes)) > 1:       # beams of different length / boundary conditions: each forced at its own node
                node_b = torch.as_tensor(nodes, dtype=torch.int32, device=self.device)
                desc.node_b = node_b.data_ptr()
                keep.append(node_b)
        if held_force is not None:
            held = self.pack_vec(held_force)
            desc.f_held = held.data_ptr()
            keep.append(held)
        return desc, keep

    def _sample_address(self, samples):
        """The address of a record buffer for a crb_record_desc.  A call that takes no sample (record_every > n_steps) has an
        empty buffer, which has no address, and the library refuses a NULL ``out`` before it counts the samples: such a
        call gets the address of a one-element placeholder, which nothing reads or writes."""
        if samples.numel() > 0:
            return samples.data_ptr()
        if getattr(self, "_no_samples", None) is None:
            self._no_samples = torch.zeros(1, dtype=self.dtype, device=self.device)
        return self._no_samples.data_ptr()

    def _record_desc(self, record, n: int, every: int = 1):
        """The crb_record_desc of a call and its zeroed buffer of n_samples = n // every samples (n steps, a sample every
        ``every``-th; or the n points of a t_eval grid): record="all" = whole-state snapshots (every DOF of the reference's
        sol.y) [n_samples, B, 2, n_node, 4] in device layout (unpack_snapshots() gives the reduced ordering),
        (node, 'u'|'w'|'phi'|'du_dt'|'dw_dt'|'dphi_dt') = that DOF's series [B, n_samples]; (None, None) for record=None."""
        if record is None:
            return None, None
        n_samples = int(n) // int(every)
        if isinstance(record, str) and record == "all":
            samples = torch.zeros((n_samples,) + tuple(self.state.shape), dtype=self.dtype, device=self.device)
            return nat.RecordDesc(0, -1, 0, int(every), self._sample_address(samples)), samples
        node, param = record
        vel = param.startswith("d") and param.endswith("_dt")
        samples = torch.zeros((self.n_beams, n_samples), dtype=self.dtype, device=self.device)
        return nat.RecordDesc(int(vel), int(node), _PARAM[param[1:-3] if vel else param], int(every),
                              self._sample_address(samples)), samples

    def _control(self, held_force, control, control_hold, n_steps, who, unit="RK4 steps"):
        """The held force or the control schedule of a call of a rollout family: (held_force, None) or
        (None, (control [K, B, n] on the device, hold)).  A schedule comes as ``control`` / ``control_hold`` or as
        ``held_force=ControlSchedule(control, hold)``.  ``unit``: what ``hold`` counts, for the error text."""
        if isinstance(held_force, ControlSchedule):
            if control is not None or control_hold is not None:
                raise ValueError(f"{who}: a ControlSchedule as held_force and control= are given together")
            held_force, control, control_hold = None, held_force.control, held_force.hold
        if control is None:
            if control_hold is not None:
                raise ValueError(f"{who}: control_hold needs control")
            return held_force, None
        if held_force is not None:
            raise ValueError(f"{who}: control and held_force are given together (a schedule takes the held force's place)")
        if control_hold is None or int(control_hold) != control_hold or int(control_hold) < 1:
            raise ValueError(f"{who}: control_hold must be an integer >= 1 ({unit} per interval)")
        U = torch.as_tensor(control, dtype=self.dtype, device=self.device)
        if U.dim() != 3 or tuple(U.shape[1:]) != (self.n_beams, self.n) or U.shape[0] < 1:
            raise ValueError(f"{who}: control must be [K >= 1, {self.n_beams}, {self.n}], got {tuple(U.shape)}")
        if int(n_steps) > U.shape[0] * int(control_hold):
            raise ValueError(f"{who}: n_steps = {int(n_steps)} exceeds K * control_hold = {U.shape[0]} * {int(control_hold)}")
        return None, (U, int(control_hold))

    def _sched_desc(self, sch):
        """The crb_input_schedule of (control [K, B, n], hold) and its packed device buffer [K, B, n_node, 4] (one scatter for
        the whole sequence; it must outlive the asynchronous launch); (None, None) for None"""
        if sch is None:
            return None, None
        U, hold = sch
        packed = self._pack_dirs(U.detach().contiguous(), False)
        return nat.InputSchedule(packed.data_ptr(), int(U.shape[0]), int(hold)), packed

    # ------------------------------------------------------------------ the hot path
    def internal_force(self, q_red) -> torch.Tensor:
        """k(q) for every beam, reduced [B, n]."""
        q = self._dev(q_red, (self.n_beams, self.n))
        x = self.pack_state(torch.cat([q, torch.zeros_like(q)], dim=1))
        k = torch.empty((self.n_beams, self.n_node, 4), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_internal_force(self.plan.h, self._ptr(x), self._ptr(k), self._stream()))
        return self.unpack_vec(k)

    def _positions(self, q_red) -> torch.Tensor:
        """a fresh device-layout state with positions ``q_red`` [B, n] (zeros: None) and zero velocities"""
        if q_red is None:
            return torch.zeros_like(self.state)
        q = self._dev(q_red, (self.n_beams, self.n))
        return self.pack_state(torch.cat([q, torch.zeros_like(q)], dim=1))

    def _tangent_index(self):
        """(source entries of the [B, n_node, 3, 3, 3] block tensor, their rows / columns in the full DOF ordering, the
        reduced -> full index [B, n] with padding entries pointing at a zero row, the padding mask) -- built once"""
        if getattr(self, "_tangent_idx", None) is None:
            nn = self.n_node
            node, blk, r, c = np.meshgrid(np.arange(nn), np.arange(3), np.arange(3), np.arange(3), indexing="ij")
            other = node + blk - 1
            ok = (other >= 0) & (other < nn)
            src = np.nonzero(ok.ravel())[0]
            rows = (3 * node + r).ravel()[src]
            cols = (3 * other + c).ravel()[src]
            red = np.full((self.n_beams, self.n), 3 * nn, dtype=np.int64)   # (3 nn: the zero row / column appended below)
            for b in range(self.n_beams):
                fi = self.free_index_per_beam[b]
                red[b, :fi.size] = fi
            dev = lambda a: torch.as_tensor(a, dtype=torch.long, device=self.device)   # noqa: E731
            self._tangent_idx = (dev(src), dev(rows), dev(cols), dev(red))
        return self._tangent_idx

    def tangent_stiffness(self, q_red=None) -> torch.Tensor:
        """dk/dq of every beam, dense and reduced [B, n, n] (crb_tangent_stiffness): the Jacobian of the reference's
        stiffness function (EulerBernoulliBeam.create_stiffness_function, euler_bernoulli_beam.py:163-219) at the reduced
        positions ``q_red`` [B, n] (None: the resident state's).  For all-linear beams it is get_stiffness_matrix()
        (``plan.stiffness()``) at any q; for nonlinear ones it is what that function refuses to give.  Padding rows and
        columns of ``mixed_topology`` ensembles are zero."""
        x = self.state if q_red is None else self._positions(q_red)
        blocks = torch.empty((self.n_beams, self.n_node, 3, 3, 3), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_tangent_stiffness(self.plan.h, self._ptr(x), self._ptr(blocks), self._stream()))
        src, rows, cols, red = self._tangent_index()
        nf = 3 * self.n_node
        dense = torch.zeros((self.n_beams, nf + 1, nf + 1), dtype=self.dtype, device=self.device)
        dense[:, rows, cols] = blocks.reshape(self.n_beams, -1)[:, src]
        bidx = torch.arange(self.n_beams, device=self.device)[:, None, None]
        return dense[bidx, red[:, :, None], red[:, None, :]]

    def solve_static(self, held_force=None, q0=None, load_steps: int = 8, max_iter: int = 20, rtol: float = STATIC_RTOL,
                     atol: float = 0.0) -> StaticSolution:
        """Static equilibrium k(q) = g(q) + u of every beam (crb_solve_static): the rest shape under the held generalised
        force ``held_force`` (reduced [B, n], None = 0) and the plan's gravity -- where the reference's dynamic system
        (dynamic_beam_model.py:294-328) has zero acceleration at zero velocity.  Newton from ``q0`` (reduced [B, n], None =
        0) along the load path H(q, lam) = r(q) - (1 - lam) r(q0), lam = 0 -> 1 in ``load_steps`` increments (halved when
        one does not converge within ``max_iter`` iterations): the equilibrium returned is the one that path reaches.  A
        beam has converged when |r|inf <= rtol max(|k|inf, |g + u|inf) + atol.  One launch; fp64 ensembles only.
        ``state`` and ``time`` are left alone: ``set_state`` starts dynamics from the result."""
        x = self._positions(q0)
        desc, keep = self._input_desc(held_force=held_force)
        iters = torch.empty((self.n_beams,), dtype=torch.int32, device=self.device)
        resid = torch.empty((self.n_beams,), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_solve_static(self.plan.h, self._ptr(x), C.byref(desc), int(load_steps), int(max_iter),
                                                 float(rtol), float(atol), self._ptr(iters), self._ptr(resid), self._stream()))
        self._keep = keep
        q = self.unpack_state(x)[:, :self.n]
        return StaticSolution(q, iters >= 0, iters, resid)

    # ------------------------------------------------------------------ sensitivities of the equilibrium (crb_static.h)
    def _static_sens(self, v_red, q_red, transpose: bool, params: bool, who: str):
        """one crb_static_jvp / crb_static_vjp launch: (solution [D, B, n], param_bar or None, status [B], single)"""
        v, single = self._dirs(v_red, self.n, f"{who}: {'qbar_red' if transpose else 'du_red'}")
        D = v.shape[0]
        x = self.state if q_red is None else self._positions(q_red)
        vd = self._pack_dirs(v, False)
        out = torch.empty_like(vd)
        status = torch.empty((self.n_beams,), dtype=torch.int32, device=self.device)
        param_bar = None
        with self._on_device():
            if transpose:
                if params:
                    param_bar = torch.zeros((D, self.n_beams, self.n_node, 8), dtype=self.dtype, device=self.device)
                nat.check(self._lib.crb_static_vjp(self.plan.h, self._ptr(x), self._ptr(vd), int(D), self._ptr(out),
                                                   self._ptr(param_bar), self._ptr(status), self._stream()))
            else:
                nat.check(self._lib.crb_static_jvp(self.plan.h, self._ptr(x), self._ptr(vd), int(D), self._ptr(out),
                                                   self._ptr(status), self._stream()))
        self._keep = [x, vd]
        self.static_status = status
        return self._unpack_force_dirs(out), param_bar, status, single

    def static_jvp(self, du_red, q_red=None):
        """Forward sensitivity of the static equilibrium (crb_static_jvp): dq = J^-1 du, the change of the rest shape of
        ``solve_static`` with the held force -- its compliance -- with J = dk/dq - dg/dq the exact tangent at the reduced
        positions ``q_red`` [B, n] (None: the resident state's positions, as in ``tangent_stiffness``).  ``du_red`` [B, n] or
        D directions [D, B, n] in one launch; returns the same shape.  ``static_status`` [B] holds 0, or -2 for a beam
        whose result is not finite (a singular tangent: the equilibrium is a limit point).  Entries past a beam's own DOFs
        (mixed-topology ensembles) are zero.  fp64 ensembles only; refused for a PINNED root under gravity, whose tangent
        is not block tridiagonal."""
        out, _, _, single = self._static_sens(du_red, q_red, False, False, "static_jvp")
        return out[0] if single else out

    def static_vjp(self, qbar_red, q_red=None, params: bool = False):
        """Reverse sensitivity of the static equilibrium (crb_static_vjp): for a cotangent ``qbar_red`` = dL/dq of the rest
        shape ([B, n], or D cotangents [D, B, n] in one launch) returns f_bar = dL/d held_force = J^-T qbar in the same
        shape, J as in ``static_jvp`` -- unsymmetric for nonlinear elements, so this is a solve of its own.  ``q_red``
        [B, n]: the equilibrium (None: the resident state's positions).  With ``params=True`` also the dict of
        ``step_adjoint_params`` (EA_scale, EI_scale, elastic_modulus, moment_inertia, gravity, ...: dL/d of the rod's own
        parameters, mu . d(u - k + g)/d theta with mu = f_bar), its drag entries zero: nothing moves at rest.
        ``static_status`` as in ``static_jvp``."""
        out, param_bar, _, single = self._static_sens(qbar_red, q_red, True, params, "static_vjp")
        fb = out[0] if single else out
        if not params:
            return fb
        pd = self._param_dict(param_bar)
        return fb, ({k: v[0] for k, v in pd.items()} if single else pd)

    def equilibrium(self, held_force=None, q0=None, load_steps: int = 8, max_iter: int = 20, rtol: float = STATIC_RTOL,
                    atol: float = 0.0):
        """A differentiable ``solve_static``: (q [B, n], converged [B]) as a torch.autograd.Function whose backward is one
        ``static_vjp`` launch at q -- ``loss.backward()`` reaches ``held_force`` [B, n] when it requires grad.  Rows of
        beams that did not converge, or whose sensitivity status is -2 (singular tangent), get a ZERO gradient: their q
        is not an equilibrium, so there is nothing the implicit function theorem could differentiate.  The rod's
        parameters are not autograd inputs (the forward would need parameter overrides, as for ``rollout``); use
        ``static_vjp(..., params=True)``.  Leaves ``state``, ``time`` and ``status`` alone.  fp64 ensembles only; once
        differentiable."""
        held = None if held_force is None else torch.as_tensor(held_force, dtype=self.dtype, device=self.device)
        opts = dict(q0=q0, load_steps=int(load_steps), max_iter=int(max_iter), rtol=float(rtol), atol=float(atol))
        return _Equilibrium.apply(self, opts, held)

    def rhs_device(self, x: torch.Tensor, u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """xdot in device layout for a state (and optional force) in device layout."""
        out = torch.empty_like(x)
        with self._on_device():
            nat.check(self._lib.crb_rhs(self.plan.h, self._ptr(x), self._ptr(u), self._ptr(out), self._stream()))
        return out

    def rhs(self, x_red=None, u_red=None) -> torch.Tensor:
        """dynamic_system(t, x, u) for every beam: reduced [B, 2n] in, reduced [B, 2n] out."""
        x = self.state if x_red is None else self.pack_state(x_red)
        u = None if u_red is None else self.pack_vec(u_red)
        return self.unpack_state(self.rhs_device(x, u))

    def step(self, n_steps: int, dt: float, impulse_amp=None, impulse_duration: float = 0.01,
             impulse_index: int = -2, held_force=None, t0: Optional[float] = None, record=None, record_every: int = 1,
             control=None, control_hold: Optional[int] = None):
        """Advance the resident state by ``n_steps`` RK4 steps in one kernel launch.

        impulse_amp    per-beam amplitudes [B] of the examples' forcing: that value on reduced
                       position index ``impulse_index`` (-2 = tip w, example_utilities.py:147)
                       while t < impulse_duration
        held_force     reduced [B, n] generalised force held constant over the call
        control        reduced [K, B, n] control sequence, vector k held for ``control_hold`` steps (step i of the call applies
                       control[i // control_hold]; n_steps <= K * control_hold); switched inside the kernel, still one
                       launch, bitwise the chain of one call per interval with ``held_force=control[k]``.  Not together with
                       ``held_force``.
        record         (node, 'u'|'w'|'phi'|'du_dt'|'dw_dt'|'dphi_dt'): sample that DOF on the device after
                       every ``record_every``-th step (the t_eval output of the reference's solve_ivp
                       calls); the call then returns (clock, samples[B, n_steps // record_every]).
                       "all": whole-state snapshots instead, (clock, snaps[n_rec, B, 2, n_node, 4])
        Returns the clock after the call (accumulated by addition, as the oracle does).
        """
        held_force, sch = self._control(held_force, control, control_hold, n_steps, "step")
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        rec, samples = self._record_desc(record, n_steps, record_every)
        keep.append(samples)
        t_end = C.c_double(0.0)
        sd, packed = self._sched_desc(sch)
        keep.append(packed)
        with self._on_device():   # (without a schedule, sd None, this is crb_step_rk4_rec)
            nat.check(self._lib.crb_step_rk4_sched(self.plan.h, self._ptr(self.state), self.time, float(dt), int(n_steps),
                                                   C.byref(desc), self._ref(sd), self._ref(rec), C.byref(t_end), self._stream()))
        self._keep = keep  # device buffers must outlive the asynchronous launch
        self.time = t_end.value
        return (self.time, samples) if record is not None else self.time

    # ------------------------------------------------------------------ tangent-linear model (crb_tangent.h)
    def _dir_index(self):
        """(state, force) gather indices of reduced [B, 2n] / [B, n] entries into the flattened device layouts [B, 2, n_node,
        4] / [B, n_node, 4] with one extra zero entry at the end, to which padding entries of mixed_topology point -- built
        once"""
        if getattr(self, "_dir_idx", None) is None:
            nn, n, B = self.n_node, self.n, self.n_beams
            sidx = np.full((B, 2 * n), B * 2 * nn * 4, dtype=np.int64)
            fidx = np.full((B, n), B * nn * 4, dtype=np.int64)
            for b in range(B):
                fi = self.free_index_per_beam[b].astype(np.int64)
                rec = (fi // 3) * 4 + fi % 3
                sidx[b, :fi.size] = b * 2 * nn * 4 + rec
                sidx[b, n:n + fi.size] = b * 2 * nn * 4 + nn * 4 + rec
                fidx[b, :fi.size] = b * nn * 4 + rec
            dev = lambda a: torch.as_tensor(a.ravel(), dtype=torch.long, device=self.device)   # noqa: E731
            self._dir_idx = (dev(sidx), dev(fidx))
        return self._dir_idx

    def _dirs(self, v, width, what):
        """reduced [B, width] or [D, B, width] -> ([D, B, width] on the device, whether the input had no direction axis)"""
        t = torch.as_tensor(v, dtype=self.dtype, device=self.device)
        single = t.dim() == 2
        if single:
            t = t.unsqueeze(0)
        if t.dim() != 3 or tuple(t.shape[1:]) != (self.n_beams, width) or t.shape[0] < 1:
            raise ValueError(f"{what}: expected shape [{self.n_beams}, {width}] or [D >= 1, {self.n_beams}, {width}], "
                             f"got {tuple(t.shape)}")
        return t.contiguous(), single

    def _pack_dirs(self, v, state: bool) -> torch.Tensor:
        """[D, B, 2n] (state) / [D, B, n] (force) reduced -> device layout [D, B, 2, n_node, 4] / [D, B, n_node, 4], on the
        device in one scatter"""
        sidx, fidx = self._dir_index()
        idx = sidx if state else fidx
        D = v.shape[0]
        rec = (2 if state else 1) * self.n_node * 4
        flat = torch.zeros((D, self.n_beams * rec + 1), dtype=self.dtype, device=self.device)
        flat[:, idx] = v.reshape(D, -1)        # (padding entries all land on the last, discarded column)
        return flat[:, :-1].reshape((D, self.n_beams) + ((2,) if state else ()) + (self.n_node, 4)).contiguous()

    def _unpack_dirs(self, x: torch.Tensor) -> torch.Tensor:
        """device layout [D, B, 2, n_node, 4] -> reduced [D, B, 2n] (padding entries 0)"""
        sidx, _ = self._dir_index()
        D = x.shape[0]
        flat = torch.cat([x.reshape(D, -1), torch.zeros((D, 1), dtype=self.dtype, device=self.device)], dim=1)
        return flat[:, sidx].reshape(D, self.n_beams, 2 * self.n)

    def rhs_jvp(self, dx_red, x_red=None, u_red=None, du_red=None):
        """Forward-mode derivative of the RHS (crb_rhs_jvp): returns (xdot, dxdot) with xdot = f(x, u) reduced [B, 2n] -- the
        reference's dynamic_system(t, x, u), dynamic_beam_model.py:294-362 -- and dxdot = df/dx dx + df/du du, exact (dual
        numbers, no finite differences), in the shape of ``dx_red``: [B, 2n] or D directions [D, B, 2n] in one launch.
        ``x_red`` reduced [B, 2n] (None: the resident state), ``u_red`` [B, n] held force (None = 0), ``du_red`` its tangent
        [B, n] / [D, B, n] (None = 0).  fp64 ensembles only."""
        dx, single = self._dirs(dx_red, 2 * self.n, "rhs_jvp: dx_red")
        D = dx.shape[0]
        du = None
        if du_red is not None:
            du, _ = self._dirs(du_red, self.n, "rhs_jvp: du_red")
            if du.shape[0] != D:
                du = du.expand(D, -1, -1) if du.shape[0] == 1 else None
            if du is None:
                raise ValueError("rhs_jvp: du_red must have the directions of dx_red")
        x = self.state if x_red is None else self.pack_state(x_red)
        u = None if u_red is None else self.pack_vec(u_red)
        dxd = self._pack_dirs(dx, True)
        dud = None if du is None else self._pack_dirs(du, False)
        xdot = torch.empty_like(x)
        dxdot = torch.empty_like(dxd)
        with self._on_device():
            nat.check(self._lib.crb_rhs_jvp(self.plan.h, self._ptr(x), self._ptr(u), self._ptr(dxd), self._ptr(dud), int(D),
                                            self._ptr(xdot), self._ptr(dxdot), self._stream()))
        out = self._unpack_dirs(dxdot)
        return self.unpack_state(xdot), (out[0] if single else out)

    def linearize(self, x_red=None, u_red=None):
        """The linearised dynamics at (x, u): (A [B, 2n, 2n], Bu [B, 2n, n]), the dense Jacobians d f / d x and d f / d u of
        the reference's dynamic_system (dynamic_beam_model.py:294-362) -- for a linear beam at rest without drag or gravity,
        LinearQuadraticRegulator's A = [[0, I], [-M^-1 K, 0]] and B = [0; M^-1] (linear_quadratic_regulator.py:84-147); for a
        nonlinear, dragged, gravity-loaded rod the exact Jacobian about any operating point, e.g. its equilibrium from
        solve_static.  Two launches of crb_rhs_jvp with identity seeds (2n state, n input directions).  ``x_red`` reduced
        [B, 2n] (None: the resident state), ``u_red`` [B, n] (None = 0).  Padding rows and columns of ``mixed_topology``
        ensembles are zero."""
        B, n = self.n_beams, self.n
        eye2 = torch.eye(2 * n, dtype=self.dtype, device=self.device)
        _, dA = self.rhs_jvp(eye2[:, None, :].expand(2 * n, B, 2 * n), x_red, u_red)
        eye1 = torch.eye(n, dtype=self.dtype, device=self.device)
        _, dB = self.rhs_jvp(torch.zeros((n, B, 2 * n), dtype=self.dtype, device=self.device), x_red, u_red,
                             eye1[:, None, :].expand(n, B, n))
        return dA.permute(1, 2, 0).contiguous(), dB.permute(1, 2, 0).contiguous()

    def step_tangent(self, n_steps: int, dt: float, dx0_red, impulse_amp=None, impulse_duration: float = 0.01,
                     impulse_index: int = -2, held_force=None, d_impulse_amp=None, d_held_force=None,
                     t0: Optional[float] = None):
        """``step()`` with the tangent of the rollout alongside (crb_step_rk4_tangent): advances ``state`` and ``time`` exactly as
        step() does, and returns dx(T) = dx(T)/dx(0) dx0 + dx(T)/d amp d_impulse_amp + dx(T)/d f_held d_held_force in the shape
        of ``dx0_red`` ([B, 2n] or D directions [D, B, 2n], one launch).  An identity batch of seeds (D = 2n) gives the
        state-transition matrix.  ``d_impulse_amp`` [B] / [D, B] and ``d_held_force`` [B, n] / [D, B, n] are the tangents of
        ``impulse_amp`` and ``held_force`` (None = 0; a [B] / [B, n] tangent is used for every direction).  The derivative is
        that of the discrete RK4 map itself, exact.  fp64 ensembles only.
        ``held_force=ControlSchedule(U, hold)`` runs a control sequence U [K, B, n] as step(control=U, control_hold=hold)
        does; ``d_held_force`` is then its tangent, [K, B, n] or [D, K, B, n]."""
        def launch(dxd, D, t_start, desc, tan, sd, dsd, t_end):   # (without a schedule, sd and dsd None: crb_step_rk4_tangent)
            return self._lib.crb_step_rk4_tangent_sched(self.plan.h, self._ptr(self.state), self._ptr(dxd), int(D), t_start,
                                                        float(dt), int(n_steps), C.byref(desc), C.byref(tan), self._ref(sd),
                                                        self._ptr(dsd), C.byref(t_end), self._stream())
        return self._rollout_tangent("step_tangent", "RK4 steps", launch, n_steps, dx0_red, impulse_amp, impulse_duration,
                                     impulse_index, held_force, d_impulse_amp, d_held_force, t0)

    def _rollout_tangent(self, who, unit, launch, n_steps, dx0_red, impulse_amp, impulse_duration, impulse_index, held_force,
                         d_impulse_amp, d_held_force, t0):
        """The body step_tangent and step_implicit_tangent share: _tangent_inputs, then _tangent_launch of
        ``launch(dxd, D, t_start, desc, tan, sd, dsd, t_end)`` (the library call on the resident state).  ``who`` / ``unit``:
        the caller's name and what a schedule's hold counts."""
        held_force, sch = self._control(held_force, None, None, n_steps, who, unit)
        dx, single, D, desc, tan, keep, sd, dsd = self._tangent_inputs(who, dx0_red, impulse_amp, impulse_duration, impulse_index,
                                                                       held_force, sch, d_impulse_amp, d_held_force)
        return self._tangent_launch(lambda dxd, t_start, t_end: launch(dxd, D, t_start, desc, tan, sd, dsd, t_end), dx, single, t0,
                                    keep)

    def _tangent_inputs(self, who, dx0_red, impulse_amp, impulse_duration, impulse_index, held_force, sch, d_impulse_amp,
                        d_held_force):
        """What every tangent rollout decodes alike: the seeds dx [D, B, 2n] (and whether ``dx0_red`` had no direction axis), the
        input's descriptor, the crb_input_tangent of ``d_impulse_amp`` and ``d_held_force`` and, with a schedule ``sch`` (of
        _control), its descriptor and its packed tangent -- (dx, single, D, desc, tan, keep, sd, dsd), ``keep`` the device
        buffers these point to."""
        dx, single = self._dirs(dx0_red, 2 * self.n, f"{who}: dx0_red")
        D = dx.shape[0]
        if d_impulse_amp is not None and impulse_amp is None:
            impulse_amp = torch.zeros((self.n_beams,), dtype=self.dtype, device=self.device)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        tan = nat.InputTangent()
        if d_impulse_amp is not None:
            da = torch.as_tensor(d_impulse_amp, dtype=self.dtype, device=self.device)
            if tuple(da.shape) not in ((self.n_beams,), (D, self.n_beams)):
                raise ValueError(f"{who}: d_impulse_amp must be [{self.n_beams}] or [{D}, {self.n_beams}]")
            da = da.expand(D, self.n_beams).contiguous()
            tan.d_amp = da.data_ptr()
            keep.append(da)
        dsd = None
        if d_held_force is not None and sch is not None:   # the tangent of the schedule, [D, K, B, n_node, 4] in one scatter
            K = sch[0].shape[0]
            dU = torch.as_tensor(d_held_force, dtype=self.dtype, device=self.device)
            if dU.dim() == 3:
                dU = dU.unsqueeze(0)
            if dU.dim() != 4 or tuple(dU.shape[1:]) != (K, self.n_beams, self.n) or dU.shape[0] not in (1, D):
                raise ValueError(f"{who}: the tangent of a control schedule must be [{K}, {self.n_beams}, {self.n}] or "
                                 f"[{D}, {K}, {self.n_beams}, {self.n}], got {tuple(dU.shape)}")
            dsd = self._pack_dirs(dU.expand(D, -1, -1, -1).reshape(D * K, self.n_beams, self.n), False)
            keep.append(dsd)
        elif d_held_force is not None:
            dh, _ = self._dirs(d_held_force, self.n, f"{who}: d_held_force")
            if dh.shape[0] not in (1, D):
                raise ValueError(f"{who}: d_held_force must have the directions of dx0_red")
            dhd = self._pack_dirs(dh.expand(D, -1, -1), False)
            tan.df_held = dhd.data_ptr()
            keep.append(dhd)
        sd, packed = self._sched_desc(sch)
        keep.append(packed)
        return dx, single, D, desc, tan, keep, sd, dsd

    def _tangent_launch(self, call, dx, single, t0, keep):
        """``call(dxd, t_start, t_end)``, the library call of a tangent rollout on the resident state with the seeds packed, from
        the clock ``t0`` (None: ``time``, which moves only when the launch is accepted); the tangent in the seeds' shape"""
        dxd = self._pack_dirs(dx, True)
        t_end = C.c_double(0.0)
        with self._on_device():
            nat.check(call(dxd, self.time if t0 is None else float(t0), t_end))
        self._keep = keep + [dxd]
        self.time = float(t_end.value)
        out = self._unpack_dirs(dxd)
        return out[0] if single else out

    def step_implicit_tangent(self, n_steps: int, h: float, dx0_red, n_iter: int = 2, impulse_amp=None,
                              impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None, d_impulse_amp=None,
                              d_held_force=None, t0: Optional[float] = None):
        """``step_implicit()`` with the tangent of the rollout alongside (crb_step_implicit_tangent) -- forward mode through
        the stepper that takes h = 1e-4 ... 1e-3 s: advances ``state`` and ``time`` as step_implicit() does (``time`` moves
        only when the launch is accepted) and returns dx(T) = dx(T)/dx(0) dx0 + dx(T)/d amp d_impulse_amp + dx(T)/d f_held
        d_held_force.  Shapes, [B, .] / [D, B, .] broadcasting and ``held_force=ControlSchedule(U, hold)`` with
        ``d_held_force`` [K, B, n] / [D, K, B, n] (``hold`` counting implicit steps) are step_tangent's.  The derivative is
        that of the discrete map step_implicit computes -- ``n_iter`` (1 ... 16) modified-Newton iterations per step, each
        step's iteration and its tangent starting from the previous step's iterate, from 0 at the first step of a call and of
        every schedule interval -- the map whose transpose step_implicit_adjoint applies; not of the converged midpoint rule.
        The base state agrees with step_implicit to rounding, not bitwise.  fp64 ensembles only.
        Not available: the damped variant (``rho_inf`` < 1), tangents of recorded samples, parameter tangents.  The closed
        loop has its own call, step_implicit_feedback_tangent."""
        def launch(dxd, D, t_start, desc, tan, sd, dsd, t_end):   # (without a schedule: crb_step_implicit_tangent)
            return self._lib.crb_step_implicit_tangent_sched(self.plan.h, self._ptr(self.state), self._ptr(dxd), int(D), t_start,
                                                             float(h), int(n_steps), int(n_iter), C.byref(desc), C.byref(tan),
                                                             self._ref(sd), self._ptr(dsd), C.byref(t_end), self._stream())
        return self._rollout_tangent("step_implicit_tangent", "implicit steps", launch, n_steps, dx0_red, impulse_amp,
                                     impulse_duration, impulse_index, held_force, d_impulse_amp, d_held_force, t0)

    def linearize_implicit(self, h: float, n_steps: int = 1, n_iter: int = 2, x_red=None, held_force=None):
        """The discrete-time linearisation of the implicit stepper: (A_d [B, 2n, 2n], B_d [B, 2n, n]), the Jacobians of
        x(t + n_steps h) with respect to x(t) and to a force held over those steps, of the sampled plant
        x_{k+1} = Phi_h(x_k, u_k) that ``step_implicit(n_steps, h, n_iter, held_force=u_k)`` applies -- what a digital LQR
        (the sampled form of LinearQuadraticRegulator, linear_quadratic_regulator.py:84-147) or a linear MPC designs on
        (examples/digital_lqr.py).  Taken at (``x_red`` [B, 2n], ``held_force`` [B, n]); None = the resident state and 0.
        Two launches of crb_step_implicit_tangent with identity seeds (2n state, n input directions) on a copy: ``state``,
        ``time`` and ``status`` are untouched.  Padding rows and columns of ``mixed_topology`` ensembles are zero."""
        B, n = self.n_beams, self.n
        x0 = self.state.clone() if x_red is None else self.pack_state(x_red)
        held = None if held_force is None else self._dev(held_force, (B, n))
        eye2 = torch.eye(2 * n, dtype=self.dtype, device=self.device)
        eye1 = torch.eye(n, dtype=self.dtype, device=self.device)
        return self._jacobians_on_a_copy(
            x0,
            lambda: self.step_implicit_tangent(n_steps, h, eye2[:, None, :].expand(2 * n, B, 2 * n), n_iter=n_iter,
                                               held_force=held, t0=0.0),
            lambda: self.step_implicit_tangent(n_steps, h, torch.zeros((n, B, 2 * n), dtype=self.dtype, device=self.device),
                                               n_iter=n_iter, held_force=held, d_held_force=eye1[:, None, :].expand(n, B, n),
                                               t0=0.0))

    def _jacobians_on_a_copy(self, x0, first, second):
        """The Jacobians [B, 2n, D] of two tangent calls with identity seeds (each returns [D, B, 2n]), ``first`` on a copy of
        the device-layout state ``x0`` and ``second`` on ``x0`` itself: ``state``, ``time`` and the status -- the plan's
        pointer and step count -- are put back, whatever the calls raise."""
        saved = (self.state, self.time, getattr(self, "_status", None))
        had_status = saved[2] is not None
        try:
            if had_status:   # (the launches below must not report into the ensemble's status, nor count as its steps)
                with self._on_device():
                    steps_done = int(self._lib.crb_plan_status_steps(self.plan.h))
                    nat.check(self._lib.crb_plan_set_status(self.plan.h, None, 0))
            self.state = x0.clone()
            d1 = first()
            self.state = x0
            d2 = second()
        finally:
            self.state, self.time = saved[0], saved[1]
            if had_status:
                with self._on_device():
                    nat.check(self._lib.crb_plan_set_status(self.plan.h, self._ptr(saved[2]), steps_done))
        return d1.permute(1, 2, 0).contiguous(), d2.permute(1, 2, 0).contiguous()

    # ------------------------------------------------------------------ adjoint (reverse mode, crb_adjoint.h)
    ADJOINT_WORK_BUDGET = 1 << 30   # bytes the default checkpoint interval keeps crb_step_rk4_adjoint's work buffer under

    def _unpack_force_dirs(self, v: torch.Tensor) -> torch.Tensor:
        """device layout [D, B, n_node, 4] -> reduced [D, B, n] (padding entries 0): the transposed gather of force-shaped
        outputs"""
        _, fidx = self._dir_index()
        D = v.shape[0]
        flat = torch.cat([v.reshape(D, -1), torch.zeros((D, 1), dtype=self.dtype, device=self.device)], dim=1)
        return flat[:, fidx].reshape(D, self.n_beams, self.n)

    def _unpack_sched_dirs(self, v: torch.Tensor) -> torch.Tensor:
        """device layout [D, K, B, n_node, 4] -> reduced [D, K, B, n] (padding entries 0), one gather for all intervals"""
        D, K = v.shape[0], v.shape[1]
        return self._unpack_force_dirs(v.reshape((D * K,) + tuple(v.shape[2:]))).reshape(D, K, self.n_beams, self.n)

    def rhs_vjp(self, lam_red, x_red=None, u_red=None):
        """Reverse-mode derivative of the RHS (crb_rhs_vjp): returns (xbar, ubar) = ((df/dx)^T lam, (df/du)^T lam) for the
        reference's dynamic_system(t, x, u) (dynamic_beam_model.py:294-362), exact, in the shape of ``lam_red``: [B, 2n] ->
        ([B, 2n], [B, n]), or D cotangents [D, B, 2n] -> ([D, B, 2n], [D, B, n]) in one launch.  ``x_red`` reduced [B, 2n]
        (None: the resident state), ``u_red`` [B, n] held force (None = 0).  fp64 ensembles only."""
        lam, single = self._dirs(lam_red, 2 * self.n, "rhs_vjp: lam_red")
        D = lam.shape[0]
        x = self.state if x_red is None else self.pack_state(x_red)
        u = None if u_red is None else self.pack_vec(u_red)
        lamd = self._pack_dirs(lam, True)
        xbar = torch.empty_like(lamd)
        ubar = torch.empty((D, self.n_beams, self.n_node, 4), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_rhs_vjp(self.plan.h, self._ptr(x), self._ptr(u), self._ptr(lamd), int(D), None,
                                            self._ptr(xbar), self._ptr(ubar), self._stream()))
        xb, ub = self._unpack_dirs(xbar), self._unpack_force_dirs(ubar)
        return (xb[0], ub[0]) if single else (xb, ub)

    def checkpoint_interval(self, n_steps: int, checkpoint_every: Optional[int] = None,
                            param_cotangents: Optional[int] = None, feedback_cotangents: Optional[int] = None,
                            implicit: Optional[Tuple[int, int]] = None,
                            implicit_feedback: Optional[Tuple[int, int, int]] = None,
                            implicit_params: Optional[Tuple[int, int]] = None) -> int:
        """Steps per checkpoint segment of an adjoint rollout: ``checkpoint_every``, or ceil(sqrt(n_steps)) lowered until the
        work buffer of crb_step_rk4_adjoint (crb_rk4_adjoint_work_bytes) fits ADJOINT_WORK_BUDGET.  ``param_cotangents``: the
        number of cotangents of a ``step_adjoint_params`` call, whose work buffer
        (crb_rk4_adjoint_params_work_bytes) is sized instead; ``feedback_cotangents``: that of a ``step_feedback_adjoint`` call
        (crb_rk4_feedback_adjoint_work_bytes); ``implicit`` = (n_iter, n_cot): that of a ``step_implicit_adjoint`` call
        (crb_implicit_adjoint_work_bytes); ``implicit_feedback`` = (n_iter, hold, n_cot): that of a
        ``step_implicit_feedback_adjoint`` call (crb_implicit_feedback_adjoint_work_bytes), whose segments are whole samples:
        ceil(sqrt(n_steps)) rounded up to a multiple of ``hold`` and lowered by ``hold`` while the buffer exceeds the budget
        (ValueError if one sample per segment does not fit); a given ``checkpoint_every`` must be a multiple of ``hold``;
        ``implicit_params`` = (n_iter, n_cot): that of a ``step_implicit_adjoint_params`` call
        (crb_implicit_adjoint_params_work_bytes)."""
        if implicit_params is not None:
            if any(a is not None for a in (implicit, implicit_feedback, param_cotangents, feedback_cotangents)):
                raise ValueError("checkpoint_interval: implicit_params and another family's argument are given together")
            return self._interval(_IMPLICIT_PARAMS, n_steps, checkpoint_every, (None, implicit_params[0]), implicit_params[1])
        if implicit_feedback is not None:
            if implicit is not None or param_cotangents is not None or feedback_cotangents is not None:
                raise ValueError("checkpoint_interval: implicit_feedback and another family's argument are given together")
            return self._implicit_feedback_interval(n_steps, checkpoint_every, *implicit_feedback)
        if checkpoint_every is not None:   # (given: no family's work buffer is sized)
            return self._interval(None, n_steps, checkpoint_every, (), 1)
        if implicit is not None:
            if param_cotangents is not None or feedback_cotangents is not None:
                raise ValueError("checkpoint_interval: implicit and param_cotangents / feedback_cotangents are given together")
            return self._interval(_IMPLICIT, n_steps, None, (None, implicit[0]), implicit[1])
        if feedback_cotangents is not None:
            if param_cotangents is not None:
                raise ValueError("checkpoint_interval: param_cotangents and feedback_cotangents are given together")
            return self._interval(_FEEDBACK, n_steps, None, (), feedback_cotangents)
        if param_cotangents is not None:
            return self._interval(_RK4_PARAMS, n_steps, None, (), param_cotangents)
        return self._interval(_RK4, n_steps, None, (), 1)

    def _interval(self, fam, n_steps, checkpoint_every, step, n_cot):
        """checkpoint_interval for the adjoint family ``fam`` (_AdjointFamily) with its step arguments and ``n_cot`` cotangents"""
        if checkpoint_every is not None:
            if int(checkpoint_every) < 1:
                raise ValueError("checkpoint_every must be >= 1")
            return int(checkpoint_every)
        every = max(1, int(np.ceil(np.sqrt(max(int(n_steps), 1)))))
        while every > 1 and fam.work_bytes(self, every, step, int(n_cot)) > self.ADJOINT_WORK_BUDGET:
            every -= 1
        return every

    def _work_buffer(self, fam, every, step, n_cot):
        """the device work buffer of ``fam``'s checkpoint pass or sweep: its work-bytes call in whole doubles, never empty"""
        nbytes = int(fam.work_bytes(self, int(every), step, int(n_cot)))
        return torch.empty((max(1, nbytes) + 7) // 8, dtype=torch.float64, device=self.device)

    def _checkpoint_pass(self, fam, x, n_steps, t0, step, desc, every, rec, sd=None):
        """``fam``'s checkpoint call (with the crb_input_schedule ``sd``: its *_sched form) on the device state ``x``
        (advanced in place): returns the checkpoint buffer, [n_seg] of ``fam.ckpt_shape``"""
        nseg = max(1, -(-int(n_steps) // every))
        ckpt = torch.empty((nseg,) + fam.ckpt_shape(self), dtype=self.dtype, device=self.device)
        t_end = C.c_double(0.0)
        with self._on_device():
            rc, held = fam.checkpoint(self, x, ckpt, int(n_steps), int(every), float(t0), step, desc, sd, rec, t_end)
            nat.check(rc)
        # The lifetime rule of the adjoint calls: a device buffer that an enqueued launch reads or writes stays referenced
        # from _keep until a later call replaces the list.  The pass and the sweep each start a new list with what they
        # allocated or were handed (``held``: the pass's own work buffer; ``step`` holds the closed loop's gain and
        # reference); their callers append the rest -- input descriptions, packed schedules, record buffers -- right after.
        # Replacing the list releases the previous call's buffers while its launches may still be queued: that relies on every
        # call running on torch's current stream, on which the caching allocator hands freed memory out in stream order.
        self._keep = [held, step, x]
        return ckpt

    def _sweep(self, fam, ckpt, lamd, n_steps, t0, step, desc, every, rec_bar, want, sd=None):
        """``fam``'s backward sweep over the checkpoints, lamd [D, B, 2, n_node, 4] in place: returns the cotangent buffers
        ``fam.outputs`` allocated (``want``: whether the optional first one is asked for).  ``sd``: the crb_input_schedule of
        the forward pass -- the *_sched call, and the force cotangent is the schedule's, [D, K, B, n_node, 4]."""
        D = lamd.shape[0]
        outs = fam.outputs(self, D, want, sd)
        work = self._work_buffer(fam, every, step, D)
        with self._on_device():
            nat.check(fam.sweep(self, ckpt, lamd, int(n_steps), int(every), float(t0), step, desc, sd, rec_bar, outs, work))
        self._keep = [work, ckpt, lamd, step, outs]   # (the lifetime rule: _checkpoint_pass)
        return outs

    def _param_columns(self):
        """Per-beam parameter columns padded to [B, n_elem] (1 past a beam's own elements, so that divisions stay finite
        where the gradients are zero anyway), the fluid densities [B] and the fluid switches [B], on the device"""
        if getattr(self, "_param_cols", None) is None:
            B, ne = self.n_beams, self.n_elem
            cols = self.columns if isinstance(self.columns, list) else [self.columns] * B
            fps = self._fps if len(self._fps) == B else [self._fps[0]] * B
            out = {k: np.ones((B, ne)) for k in ("elastic_modulus", "moment_inertia", "drag_coef")}
            for b, c in enumerate(cols):
                nb = int(self.n_elem_per_beam[b])
                out["elastic_modulus"][b, :nb] = np.asarray(c["elastic_modulus"], dtype=np.float64)[:nb]
                out["moment_inertia"][b, :nb] = np.asarray(c["moment_inertia"], dtype=np.float64)[:nb]
                if fps[b].enable_fluid_effects:
                    out["drag_coef"][b, :nb] = np.asarray(c["drag_coef"], dtype=np.float64)[:nb]
            out["fluid_density"] = np.array([f.fluid_density if f.enable_fluid_effects else 0.0 for f in fps])
            self._param_cols = {k: torch.as_tensor(v, dtype=self.dtype, device=self.device) for k, v in out.items()}
        return self._param_cols

    def _param_dict(self, param_bar: torch.Tensor):
        """crb_param_cotangent records [D, B, n_node, 8] -> step_adjoint_params' dict of parameter gradients, each [D, ...]"""
        pc = self._param_columns()
        D, B, ne = param_bar.shape[0], self.n_beams, self.n_elem
        sA, sI = param_bar[:, :, 1:, 0].contiguous(), param_bar[:, :, 1:, 1].contiguous()   # element e lies left of node e + 1
        sD = param_bar[:, :, :, 2].contiguous()
        # the plan builder's node factor 0.5 rho_f Cd[row] A_wet[row], row = the node's own element row, the last row again
        # for the tip (crbeam.hip; fluid_forces.py:59-61, 87-90): element e collects node e, the last one the tip too
        last = torch.as_tensor(self.n_elem_per_beam - 1, dtype=torch.int64, device=self.device).view(1, B, 1).expand(D, B, 1)
        tip = sD.gather(2, last + 1)
        row_sum = sD.scatter(2, last + 1, 0.0)[:, :, :ne].contiguous()
        row_sum.scatter_add_(2, last, tip)
        cd, rho = pc["drag_coef"], pc["fluid_density"]
        zero = torch.zeros((), dtype=self.dtype, device=self.device)
        return {
            "EA_scale": sA, "EI_scale": sI,
            "elastic_modulus": (sA + sI) / pc["elastic_modulus"],
            "moment_inertia": sI / pc["moment_inertia"],
            "drag_scale": sD,
            "fluid_density": torch.where(rho != 0, sD.sum(dim=2) / torch.where(rho != 0, rho, 1.0), zero),
            "drag_coef": torch.where(cd != 0, row_sum / torch.where(cd != 0, cd, 1.0), zero),
            "gravity": torch.stack([param_bar[:, :, :, 3].sum(dim=2), param_bar[:, :, :, 4].sum(dim=2)], dim=2),
        }

    def _record_cotangent(self, record, n_steps, every, lam_record, D):
        """crb_record_desc pointing at the cotangent of step()'s record samples, [D, ...] on the device (zeros if None)"""
        rec, samples = self._record_desc(record, n_steps, every)
        if rec is None:
            return None, None
        shape = (D,) + tuple(samples.shape)
        if lam_record is None:
            cot = torch.zeros(shape, dtype=self.dtype, device=self.device)
        else:
            cot = torch.as_tensor(lam_record, dtype=self.dtype, device=self.device)
            if tuple(cot.shape) == tuple(samples.shape):
                cot = cot.unsqueeze(0)
            if tuple(cot.shape[1:]) != tuple(samples.shape) or cot.shape[0] not in (1, D):
                raise ValueError(f"lam_record: expected shape {tuple(samples.shape)} or [D, ...] of it, got {tuple(cot.shape)}")
            cot = cot.expand(shape).contiguous()
        rec.out = self._sample_address(cot)
        return rec, cot

    def step_adjoint(self, n_steps: int, dt: float, lam_red, x0_red=None, impulse_amp=None, impulse_duration: float = 0.01,
                     impulse_index: int = -2, held_force=None, t0: Optional[float] = None, record=None,
                     record_every: int = 1, lam_record=None, checkpoint_every: Optional[int] = None):
        """Gradient of a scalar loss through an RK4 rollout of ``step()`` (crb_step_rk4_checkpoint + crb_step_rk4_adjoint), in
        ONE backward sweep: for the cotangent ``lam_red`` = dL/dx(T) (reduced [B, 2n], or D cotangents [D, B, 2n]) and,
        with ``record`` as in step(), ``lam_record`` = dL/d samples (the samples' shape, or [D, ...] of it), returns
        (xbar0, amp_bar, f_held_bar) = (dL/dx(0) [B, 2n], dL/d impulse_amp [B] or None without an impulse,
        dL/d held_force [B, n]), with a leading D axis when ``lam_red`` has one.  The rollout starts at ``x0_red`` (None: the
        resident state) and clock ``t0`` (None: ``time``); ``state``, ``time`` and ``status`` are left alone.
        ``checkpoint_every``: steps per checkpoint segment (checkpoint_interval); the result does not depend on it, bitwise.
        The derivative is the exact transpose of the discrete RK4 map.  fp64 ensembles only.
        ``held_force=ControlSchedule(U, hold)`` differentiates the rollout of step(control=U, control_hold=hold): the third
        return is then dL/d control, [K, B, n] ([D, K, B, n]); intervals the rollout does not reach, and entries past a beam's
        own DOF count in mixed-topology ensembles, are zero.
        ``step_adjoint_params`` also gives the gradient with respect to the rod's own parameters."""
        return self._rollout_adjoint(_RK4, n_steps, (dt, None, None), lam_red, x0_red, impulse_amp, impulse_duration,
                                     impulse_index, held_force, t0, record, record_every, lam_record, checkpoint_every)

    def step_adjoint_params(self, n_steps: int, dt: float, lam_red, x0_red=None, impulse_amp=None,
                            impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                            t0: Optional[float] = None, record=None, record_every: int = 1, lam_record=None,
                            checkpoint_every: Optional[int] = None, control=None, control_hold: Optional[int] = None):
        """``step_adjoint`` (the same arguments, ``control`` [K, B, n] / ``control_hold`` for
        ``held_force=ControlSchedule(control, control_hold)``; the first three returns are bitwise its returns) with a fourth return: the
        gradient of the loss with respect to the rod itself -- stiffness per element, drag, gravity -- as fitting a rod to a
        recorded trajectory needs it (crb_step_rk4_adjoint_params: the same sweep, storing its per-stage M^-T lambda_v, and one
        reduction launch per segment).  A dict of tensors, each with a leading D axis when ``lam_red`` has one:
          EA_scale, EI_scale [B, n_elem]  dL/d of relative scales of each element's EA and EI, at scale 1
          elastic_modulus [B, n_elem]     (EA_scale + EI_scale) / E   (complete: E enters only the stiffness)
          moment_inertia  [B, n_elem]     EI_scale / I                (complete)
          drag_scale      [B, n_node]     dL/d of a relative scale of each node's drag factor 0.5 rho_f Cd A_wet
          fluid_density   [B]             sum of drag_scale / rho_f; zeros when the fluid is off
          drag_coef       [B, n_elem]     drag_scale through the node factor's map from the drag_coef column (a node reads its
                                          own element row, the tip the last row again); zero where drag_coef is 0
          gravity         [B, 2]          dL/d (g_x, g_y), summed over the segments
        Entries past a beam's own element / node count (mixed-topology ensembles) are zero.  Not available: gradients with
        respect to length, cross_area and density (they enter the mass matrix and its reduction tables), parameters as
        autograd inputs of ``rollout`` (its forward would need parameter overrides)."""
        return self._rollout_adjoint(_RK4_PARAMS, n_steps, (dt, control, control_hold), lam_red, x0_red, impulse_amp,
                                     impulse_duration, impulse_index, held_force, t0, record, record_every, lam_record,
                                     checkpoint_every)

    def _rollout_adjoint(self, fam, n_steps, args, lam_red, x0_red, impulse_amp, impulse_duration, impulse_index, held_force, t0,
                         record, record_every, lam_record, checkpoint_every):
        """The body step_adjoint, step_adjoint_params, step_implicit_adjoint and step_feedback_adjoint share: the checkpoint
        pass and the backward sweep of the adjoint family ``fam`` (_AdjointFamily), whose ``prepare`` turns the caller's own
        arguments ``args`` into the step arguments, and the cotangents in the shape of ``lam_red``."""
        lam, single = self._dirs(lam_red, 2 * self.n, f"{fam.who}: lam_red")
        D = lam.shape[0]
        step, held_force, sch, want = fam.prepare(self, n_steps, args, held_force, impulse_amp, record)
        t0 = self.time if t0 is None else float(t0)
        every = self._interval(fam, n_steps, checkpoint_every, step, D)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        sd, packed = self._sched_desc(sch)
        x = self.state.clone() if x0_red is None else self.pack_state(x0_red)
        ckpt = self._checkpoint_pass(fam, x, n_steps, t0, step, desc, every, None, sd)
        rec_bar, cot = self._record_cotangent(record, n_steps, record_every, lam_record, D)
        lamd = self._pack_dirs(lam, True)
        outs = self._sweep(fam, ckpt, lamd, n_steps, t0, step, desc, every, rec_bar, want, sd)
        self._keep += keep + [x, cot, packed]
        res = (self._unpack_dirs(lamd),) + fam.unpack(self, outs, sd)
        return tuple(_first(v) for v in res) if single else res

    def rollout(self, x0_red, n_steps: int, dt: float, impulse_amp=None, held_force=None, impulse_duration: float = 0.01,
                impulse_index: int = -2, t0: float = 0.0, record=None, record_every: int = 1,
                checkpoint_every: Optional[int] = None, control=None, control_hold: Optional[int] = None):
        """A differentiable RK4 rollout: x(T) reduced [B, 2n] from ``x0_red`` after ``n_steps`` steps of ``step()``'s map
        (and the ``record`` samples as step() returns them), as a torch.autograd.Function whose backward is the adjoint
        (crb_step_rk4_adjoint) -- ``loss.backward()`` reaches whichever of ``x0_red``, ``impulse_amp`` [B],
        ``held_force`` [B, n] and ``control`` [K, B, n] (held ``control_hold`` steps each, as in step()) require grad: the
        whole control sequence in one backward sweep.  The forward is the checkpoint pass, whose checkpoints backward reuses.
        Leaves ``state`` and ``time`` alone.  fp64 ensembles only; once differentiable."""
        x0 = torch.as_tensor(x0_red, dtype=self.dtype, device=self.device)
        amp = None if impulse_amp is None else torch.as_tensor(impulse_amp, dtype=self.dtype, device=self.device)
        held_force, sch = self._control(held_force, control, control_hold, n_steps, "rollout")
        held = None if held_force is None else torch.as_tensor(held_force, dtype=self.dtype, device=self.device)
        ctrl, hold = (None, None) if sch is None else sch
        opts = dict(n_steps=int(n_steps), step=(float(dt),), t0=float(t0), duration=float(impulse_duration),
                    index=int(impulse_index), record=record, record_every=int(record_every),
                    every=self.checkpoint_interval(n_steps, checkpoint_every), hold=hold)
        xT, samples = _Rollout.apply(self, _RK4, opts, x0, amp, held, ctrl)
        return (xT, samples) if record is not None else xT

    # ------------------------------------------------------------------ adjoint of the implicit stepper (crb_implicit_adjoint.h)
    def step_implicit_adjoint(self, n_steps: int, h: float, lam_red, n_iter: int = 2, x0_red=None, impulse_amp=None,
                              impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                              t0: Optional[float] = None, record=None, record_every: int = 1, lam_record=None,
                              checkpoint_every: Optional[int] = None):
        """Gradient of a scalar loss through a rollout of ``step_implicit()`` (crb_step_implicit_checkpoint +
        crb_step_implicit_adjoint) -- the stepper that takes h = 1e-4 ... 1e-3 s -- in ONE backward sweep: the arguments and
        returns of ``step_adjoint``, (xbar0, amp_bar, f_held_bar) = (dL/dx(0) [B, 2n], dL/d impulse_amp [B] or None without
        an impulse, dL/d held_force [B, n]), with a leading D axis when ``lam_red`` has one.  The derivative is the exact
        transpose of the discrete map step_implicit computes -- ``n_iter`` (1 ... 16) modified-Newton iterations per step,
        each step's iteration starting from the previous step's iterate -- not of the converged midpoint rule.  ``state``,
        ``time`` and ``status`` are left alone; the result does not depend on ``checkpoint_every``, bitwise.  fp64 ensembles
        only.
        ``held_force=ControlSchedule(U, hold)`` differentiates the rollout of step_implicit(control=U, control_hold=hold)
        (crb_step_implicit_checkpoint_sched + crb_step_implicit_adjoint_sched): the third return is then dL/d control, [K, B, n]
        ([D, K, B, n]); intervals the rollout does not reach, and entries past a beam's own DOF count in mixed-topology
        ensembles, are exact zeros.  The scheduled rollout is the chain of one call per interval, so every interval's first step
        starts its iteration from 0 and the cotangent carried through the starting iterate is dropped there.
        Not available: the damped variant (``rho_inf`` < 1) and the closed loop.  ``step_implicit_adjoint_params`` also gives
        the gradient with respect to the rod's own parameters."""
        return self._rollout_adjoint(_IMPLICIT, n_steps, (h, n_iter, None, None), lam_red, x0_red, impulse_amp, impulse_duration,
                                     impulse_index, held_force, t0, record, record_every, lam_record, checkpoint_every)

    def step_implicit_adjoint_params(self, n_steps: int, h: float, lam_red, n_iter: int = 2, x0_red=None, impulse_amp=None,
                                     impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                                     t0: Optional[float] = None, record=None, record_every: int = 1, lam_record=None,
                                     checkpoint_every: Optional[int] = None, control=None, control_hold: Optional[int] = None):
        """``step_implicit_adjoint`` (the same arguments, ``control`` [K, B, n] / ``control_hold`` for
        ``held_force=ControlSchedule(control, control_hold)``; the first three returns are bitwise its returns) with a fourth
        return: ``step_adjoint_params``' dict of gradients with respect to the rod itself -- EA_scale, EI_scale,
        elastic_modulus, moment_inertia, drag_scale, drag_coef, fluid_density, gravity, with the shapes and meanings given
        there -- through the stepper that takes h = 1e-4 ... 1e-3 s (crb_step_implicit_adjoint_params: the same sweep, storing
        gbar = A^-T abar of every iteration, and one reduction launch per segment).  E and I enter the iteration matrix
        A = M + h^2/4 K0 as well as the force, so every iteration adds gbar^T dF/dtheta at its (q_m, v_m) AND
        h^2/4 gbar^T (dK0/dtheta) (a^i - a^{i+1}), the part a fixed iteration count leaves; the gradient is that of the map
        step_implicit computes with ``n_iter`` iterations, and does not depend on ``checkpoint_every``, bitwise.
        Not available: gradients with respect to length, cross_area and density (they enter the mass matrix), the damped
        variant, the sampled-data loop, parameters as autograd inputs of ``rollout_implicit``."""
        return self._rollout_adjoint(_IMPLICIT_PARAMS, n_steps, (h, n_iter, control, control_hold), lam_red, x0_red, impulse_amp,
                                     impulse_duration, impulse_index, held_force, t0, record, record_every, lam_record,
                                     checkpoint_every)

    def rollout_implicit(self, x0_red, n_steps: int, h: float, n_iter: int = 2, impulse_amp=None, held_force=None,
                         impulse_duration: float = 0.01, impulse_index: int = -2, t0: float = 0.0, record=None,
                         record_every: int = 1, checkpoint_every: Optional[int] = None, control=None,
                         control_hold: Optional[int] = None):
        """A differentiable rollout of the implicit stepper: x(T) reduced [B, 2n] from ``x0_red`` after ``n_steps`` steps of
        ``step_implicit()``'s map (and the ``record`` samples as step_implicit() returns them), as a torch.autograd.Function
        whose backward is crb_step_implicit_adjoint -- ``loss.backward()`` reaches whichever of ``x0_red``, ``impulse_amp``
        [B], ``held_force`` [B, n] and ``control`` [K, B, n] (held ``control_hold`` implicit steps each, as in
        step_implicit()) require grad, over the 0.1 ... 1 s horizons the examples simulate
        (examples/reach_tip_implicit.py, examples/steer_tip_implicit.py): the whole control sequence in one backward sweep.
        The forward is the checkpoint pass (it agrees with step_implicit to rounding), whose checkpoints backward reuses.
        Leaves ``state``, ``time`` and ``status`` alone.  fp64 ensembles only; once differentiable; no damped variant."""
        x0 = torch.as_tensor(x0_red, dtype=self.dtype, device=self.device)
        amp = None if impulse_amp is None else torch.as_tensor(impulse_amp, dtype=self.dtype, device=self.device)
        held_force, sch = self._control(held_force, control, control_hold, n_steps, "rollout_implicit", "implicit steps")
        held = None if held_force is None else torch.as_tensor(held_force, dtype=self.dtype, device=self.device)
        ctrl, hold = (None, None) if sch is None else sch
        opts = dict(n_steps=int(n_steps), step=(float(h), int(n_iter)), t0=float(t0), duration=float(impulse_duration),
                    index=int(impulse_index), record=record, record_every=int(record_every),
                    every=self.checkpoint_interval(n_steps, checkpoint_every, implicit=(n_iter, 1)), hold=hold)
        xT, samples = _Rollout.apply(self, _IMPLICIT, opts, x0, amp, held, ctrl)
        return (xT, samples) if record is not None else xT

    # ------------------------------------------------------------------ adjoint of the closed loop (crb_feedback_adjoint.h)
    def _feedback_gain(self, gain, who):
        """the one [n, 2n] gain of a differentiable closed loop on the device"""
        if isinstance(gain, (list, tuple)):
            raise NotImplementedError(f"{who}: a list of gains (per-beam or grouped gains) is not differentiable; pass one "
                                      f"[{self.n}, {2 * self.n}] gain for the whole ensemble")
        return self._dev(gain.detach() if isinstance(gain, torch.Tensor) else gain, (self.n, 2 * self.n))

    def step_feedback_adjoint(self, n_steps: int, dt: float, lam_red, gain, reference=None, x0_red=None, impulse_amp=None,
                              impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                              t0: Optional[float] = None, record=None, record_every: int = 1, lam_record=None,
                              checkpoint_every: Optional[int] = None, want_gain: bool = True):
        """Gradient of a scalar loss through the closed-loop rollout of ``step_feedback`` -- u = K (r - x) in every RK4 stage,
        examples/lqr_control.py:95-125 -- with respect to the start state, the gain and the reference, in ONE backward sweep
        (crb_step_rk4_feedback_checkpoint + crb_step_rk4_feedback_adjoint): for the cotangent ``lam_red`` = dL/dx(T) (reduced
        [B, 2n], or D cotangents [D, B, 2n]) and, with ``record`` = (node, name) as in step(), ``lam_record`` = dL/d samples,
        returns (xbar0 [B, 2n], gain_bar [n, 2n], ref_bar [B, 2n]), with a leading D axis when ``lam_red`` has one.
        ``gain`` [n, 2n] is one gain for the whole ensemble (a list of gains raises NotImplementedError); ``reference``
        [B, 2n] or None (= 0; ref_bar is returned all the same).  ``impulse_amp`` and ``held_force`` [B, n] are disturbances
        added to u; they are not differentiated.  The rollout starts at ``x0_red`` (None: the resident state) and clock
        ``t0`` (None: ``time``) and always runs the stage-split launches; ``state``, ``time`` and ``status`` are left alone.
        ``checkpoint_every``: steps per checkpoint segment; the result does not depend on it, bitwise.  ``want_gain=False``
        skips the gain-gradient product (gain_bar is None; the other returns are bitwise the same).  A non-finite cotangent
        of one beam stays in that beam's rows of xbar0 and ref_bar but reaches gain_bar, a sum over the beams.  fp64
        ensembles with one free-DOF set only."""
        return self._rollout_adjoint(_FEEDBACK, n_steps, (dt, gain, reference, want_gain), lam_red, x0_red, impulse_amp,
                                     impulse_duration, impulse_index, held_force, t0, record, record_every, lam_record,
                                     checkpoint_every)

    def rollout_feedback(self, x0_red, n_steps: int, dt: float, gain, reference=None, impulse_amp=None,
                         impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None, t0: float = 0.0,
                         record=None, record_every: int = 1, checkpoint_every: Optional[int] = None):
        """A differentiable closed-loop rollout: x(T) reduced [B, 2n] from ``x0_red`` after ``n_steps`` RK4 steps with
        u = K (r - x) in every stage (``step_feedback``'s map in its stage-split form; and the ``record`` = (node, name)
        samples [B, n_steps // record_every]), as a torch.autograd.Function whose backward is crb_step_rk4_feedback_adjoint:
        ``loss.backward()`` reaches whichever of ``x0_red``, ``gain`` [n, 2n] and ``reference`` [B, 2n] require grad -- tuning
        an LQR gain on the nonlinear rod (examples/tune_gain.py).  ``impulse_amp`` and ``held_force`` are disturbances, not
        differentiated.  Leaves ``state``, ``time`` and ``status`` alone.  fp64 ensembles only; once differentiable."""
        if isinstance(gain, (list, tuple)):
            self._feedback_gain(gain, "rollout_feedback")
        if record is not None and isinstance(record, str):
            raise NotImplementedError("rollout_feedback: whole-state snapshots (record='all') are not available in the closed loop")
        x0 = torch.as_tensor(x0_red, dtype=self.dtype, device=self.device)
        K = torch.as_tensor(gain, dtype=self.dtype, device=self.device)
        ref = None if reference is None else torch.as_tensor(reference, dtype=self.dtype, device=self.device)
        opts = dict(n_steps=int(n_steps), dt=float(dt), t0=float(t0), amp=impulse_amp, duration=float(impulse_duration),
                    index=int(impulse_index), held=held_force, record=record, record_every=int(record_every),
                    every=self.checkpoint_interval(n_steps, checkpoint_every, feedback_cotangents=1))
        xT, samples = _FeedbackRollout.apply(self, opts, x0, K, ref)
        return (xT, samples) if record is not None else xT

    # ------------------------------------------------- adjoint of the sampled-data implicit loop (crb_implicit_feedback_adjoint.h)
    def _implicit_feedback_interval(self, n_steps, checkpoint_every, n_iter, hold, n_cot):
        """checkpoint_interval(implicit_feedback=(n_iter, hold, n_cot)): segments of whole samples"""
        hold = int(hold)
        if checkpoint_every is not None:
            every = int(checkpoint_every)
            if every < 1 or every % hold != 0:
                raise ValueError(f"checkpoint_every = {checkpoint_every} must be a positive multiple of hold = {hold} "
                                 f"(a checkpoint sits on a sample start)")
            return every

        def nbytes(every):
            return int(self._lib.crb_implicit_feedback_adjoint_work_bytes(self.plan.h, every, int(n_iter), hold, int(n_cot)))

        every = -(-max(1, int(np.ceil(np.sqrt(max(int(n_steps), 1))))) // hold) * hold
        while every > hold and nbytes(every) > self.ADJOINT_WORK_BUDGET:
            every -= hold
        if nbytes(every) > self.ADJOINT_WORK_BUDGET:
            raise ValueError(f"step_implicit_feedback_adjoint: the work buffer of one sample per checkpoint segment "
                             f"({nbytes(every)} bytes at hold = {hold}) exceeds ADJOINT_WORK_BUDGET = {self.ADJOINT_WORK_BUDGET}")
        return every

    @staticmethod
    def _hold(hold, who) -> int:
        """``hold`` of a sampled-data loop, as an int"""
        if int(hold) != hold or int(hold) < 1:
            raise ValueError(f"{who}: hold must be an integer >= 1 (implicit steps per sample)")
        return int(hold)

    def _control_records(self, n_steps, hold, D=None) -> torch.Tensor:
        """zeroed device records for the held input of every sample, [K, B, n_node, 4] (with ``D`` directions [D, K, ...]),
        K = ceil(n_steps / hold) but at least one (the library is given an address)"""
        K = max(-(-int(n_steps) // int(hold)), 1)
        return torch.zeros(((K,) if D is None else (D, K)) + (self.n_beams, self.n_node, 4), dtype=self.dtype, device=self.device)

    def _unpack_controls(self, u: torch.Tensor, n_steps, hold) -> torch.Tensor:
        """_control_records -> reduced [K, B, n] / [D, K, B, n], K = ceil(n_steps / hold), none included"""
        K = -(-int(n_steps) // int(hold))
        if K == 0:
            return torch.zeros(tuple(u.shape[:-4]) + (0, self.n_beams, self.n), dtype=self.dtype, device=self.device)
        return self._unpack_force_dirs(u[:K]) if u.dim() == 4 else self._unpack_sched_dirs(u[:, :K])

    def _implicit_feedback_args(self, gain, hold, record, who):
        """the argument errors step_implicit_feedback_adjoint and rollout_implicit_feedback share; returns hold as an int"""
        if isinstance(gain, (list, tuple)):
            self._feedback_gain(gain, who)
        hold = self._hold(hold, who)
        if record is not None and isinstance(record, str):
            raise NotImplementedError(f"{who}: whole-state snapshots (record='all') are not available in the differentiable loop")
        return hold

    def step_implicit_feedback_adjoint(self, n_steps: int, h: float, lam_red, gain, reference=None, hold: int = 1,
                                       n_iter: int = 2, x0_red=None, impulse_amp=None, impulse_duration: float = 0.01,
                                       impulse_index: int = -2, held_force=None, t0: Optional[float] = None, record=None,
                                       record_every: int = 1, lam_record=None, checkpoint_every: Optional[int] = None,
                                       want_gain: bool = True):
        """Gradient of a scalar loss through the digital loop of ``step_implicit_feedback`` -- u_k = held_force + K (r - x_k),
        sampled every ``hold`` implicit steps of size ``h`` and held -- in ONE backward sweep
        (crb_step_implicit_feedback_checkpoint + crb_step_implicit_feedback_adjoint): for the cotangent ``lam_red`` = dL/dx(T)
        (reduced [B, 2n], or D cotangents [D, B, 2n]) and, with ``record`` = (node, name) as in step_implicit_feedback,
        ``lam_record`` = dL/d samples, returns (xbar0 [B, 2n], gain_bar [n, 2n], ref_bar [B, 2n], amp_bar [B] or None without
        an impulse, f_held_bar [B, n]), each with a leading D axis when ``lam_red`` has one.  ``gain`` [n, 2n] is one gain for
        the ensemble (a list raises NotImplementedError); ``reference`` [B, 2n] or None (= 0; ref_bar is returned all the
        same).  The derivative is the exact transpose of the discrete map: ``n_iter`` modified-Newton iterations per step,
        every sample's first step started from the zero iterate.  The rollout starts at ``x0_red`` (None: the resident
        state) and clock ``t0`` (None: ``time``) and always runs as the chain (one product and one launch per sample);
        ``state``, ``time`` and ``status`` are left alone.  ``checkpoint_every``: steps per checkpoint segment, a multiple of
        ``hold`` (ValueError otherwise; checkpoint_interval(implicit_feedback=...)); no result depends on it, bitwise.
        ``want_gain=False`` skips the gain gradient (gain_bar is None; the other returns are bitwise the same).  A non-finite
        cotangent of one beam stays in that beam's rows of xbar0, ref_bar and f_held_bar; it reaches gain_bar, a sum over the
        beams.  fp64 ensembles with one free-DOF set.  Not available: the damped variant, per-beam gain groups, gradients
        with respect to the rod's own parameters."""
        who = "step_implicit_feedback_adjoint"
        hold = self._implicit_feedback_args(gain, hold, record, who)
        lam = torch.as_tensor(lam_red)
        every = self._implicit_feedback_interval(n_steps, checkpoint_every, n_iter, hold, lam.shape[0] if lam.dim() == 3 else 1)
        return self._rollout_adjoint(_IMPLICIT_FEEDBACK, n_steps, (h, n_iter, hold, gain, reference, want_gain), lam_red,
                                     x0_red, impulse_amp, impulse_duration, impulse_index, held_force, t0, record,
                                     record_every, lam_record, every)

    def rollout_implicit_feedback(self, x0_red, n_steps: int, h: float, gain, reference=None, hold: int = 1, n_iter: int = 2,
                                  impulse_amp=None, held_force=None, impulse_duration: float = 0.01, impulse_index: int = -2,
                                  t0: float = 0.0, record=None, record_every: int = 1,
                                  checkpoint_every: Optional[int] = None, return_control: bool = False):
        """A differentiable digital loop: x(T) reduced [B, 2n] from ``x0_red`` after ``n_steps`` implicit steps of
        ``step_implicit_feedback``'s map (then the ``record`` = (node, name) samples [B, n_steps // record_every] when
        ``record`` is given, then with ``return_control`` the held input of every sample, ``control`` [K, B, n],
        non-differentiable), as a torch.autograd.Function whose backward is crb_step_implicit_feedback_adjoint:
        ``loss.backward()`` reaches whichever of ``x0_red``, ``gain`` [n, 2n], ``reference`` [B, 2n], ``impulse_amp`` [B] and
        ``held_force`` [B, n] require grad -- tuning the gain of a 1 kHz regulator on the nonlinear rod at h = 1e-3 s
        (examples/tune_digital_gain.py).  The forward is the checkpoint pass (the chain; it agrees with
        step_implicit_feedback to rounding), whose checkpoints and controls backward reuses.  Leaves ``state``, ``time`` and
        ``status`` alone.  fp64 ensembles with one free-DOF set; once differentiable."""
        who = "rollout_implicit_feedback"
        hold = self._implicit_feedback_args(gain, hold, record, who)
        every = self._implicit_feedback_interval(n_steps, checkpoint_every, n_iter, hold, 1)
        x0 = torch.as_tensor(x0_red, dtype=self.dtype, device=self.device)
        K = torch.as_tensor(gain, dtype=self.dtype, device=self.device)
        ref = None if reference is None else torch.as_tensor(reference, dtype=self.dtype, device=self.device)
        amp = None if impulse_amp is None else torch.as_tensor(impulse_amp, dtype=self.dtype, device=self.device)
        held = None if held_force is None else torch.as_tensor(held_force, dtype=self.dtype, device=self.device)
        opts = dict(n_steps=int(n_steps), h=float(h), n_iter=int(n_iter), hold=hold, t0=float(t0),
                    duration=float(impulse_duration), index=int(impulse_index), record=record,
                    record_every=int(record_every), every=every)
        xT, samples, control = _ImplicitFeedbackRollout.apply(self, opts, x0, K, ref, amp, held)
        out = (xT,) + ((samples,) if record is not None else ()) + ((control,) if return_control else ())
        return out if len(out) > 1 else xT

    # ------------------------------------------------- tangent of the sampled-data implicit loop (crb_implicit_feedback_tangent.h)
    def step_implicit_feedback_tangent(self, n_steps: int, h: float, dx0_red, gain, reference=None, hold: int = 1,
                                       n_iter: int = 2, d_gain=None, d_reference=None, impulse_amp=None,
                                       impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                                       d_impulse_amp=None, d_held_force=None, t0: Optional[float] = None,
                                       return_control: bool = False):
        """``step_implicit_feedback()`` with the tangent of the digital loop alongside (crb_step_implicit_feedback_tangent):
        advances ``state`` and ``time`` as step_implicit_feedback does (``time`` moves only when the launch is accepted) and
        returns dx(T) along ``dx0_red`` ([B, 2n], or D directions [D, B, 2n] in one call), ``d_gain`` ([n, 2n] / [D, n, 2n]),
        ``d_reference`` ([B, 2n] / [D, B, 2n]), ``d_held_force`` ([B, n] / [D, B, n]) and ``d_impulse_amp`` ([B] / [D, B]);
        None = 0, and a tangent without a direction axis is used for every direction, as in step_implicit_tangent.  At the
        top of every sample du_k = d_held_force + K (d_reference - dx_k) + d_gain (r - x_k); the sample's steps are one
        interval of step_implicit_tangent's scheduled form.  The derivative is the exact forward mode of the map whose
        transpose step_implicit_feedback_adjoint applies.  With ``return_control`` also returns (control [K, B, n], d_control
        [D, K, B, n]), K = ceil(n_steps / hold): ``step_implicit_tangent(held_force=ControlSchedule(control, hold),
        d_held_force=d_control)`` replays ``state`` and dx(T) bitwise.  Always the chain form: ``state`` agrees with
        step_implicit_feedback to rounding, not bitwise.  ``gain`` is one [n, 2n] gain for the ensemble (a list raises
        NotImplementedError).  fp64 ensembles with one free-DOF set.  Not available: an in-kernel form, tangents of recorded
        samples, gain groups, the damped variant, parameter tangents, the RK4 closed loop's tangent."""
        who = "step_implicit_feedback_tangent"
        K = self._feedback_gain(gain, who)
        hold = self._hold(hold, who)
        B, n = self.n_beams, self.n
        dx, single, D, desc, tan, keep, _, _ = self._tangent_inputs(who, dx0_red, impulse_amp, impulse_duration, impulse_index,
                                                                    held_force, None, d_impulse_amp, d_held_force)
        ref = None if reference is None else self._dev(reference, (B, 2 * n))
        fbt = nat.FeedbackTangent()
        dK = dr = None
        if d_gain is not None:
            dK = torch.as_tensor(d_gain, dtype=self.dtype, device=self.device)
            if tuple(dK.shape) not in ((n, 2 * n), (D, n, 2 * n)):
                raise ValueError(f"{who}: d_gain must be [{n}, {2 * n}] or [{D}, {n}, {2 * n}], got {tuple(dK.shape)}")
            dK = dK.expand(D, n, 2 * n).contiguous()
            fbt.d_gain = dK.data_ptr()
        if d_reference is not None:
            dr, _ = self._dirs(d_reference, 2 * n, f"{who}: d_reference")
            if dr.shape[0] not in (1, D):
                raise ValueError(f"{who}: d_reference must have the directions of dx0_red")
            dr = dr.expand(D, B, 2 * n).contiguous()
            fbt.d_ref = dr.data_ptr()
        u_out = self._control_records(n_steps, hold) if return_control else None
        du_out = self._control_records(n_steps, hold, D) if return_control else None
        nbytes = int(self._lib.crb_implicit_feedback_tangent_work_bytes(self.plan.h, int(D)))
        work = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=self.device)

        def call(dxd, t_start, t_end):
            return self._lib.crb_step_implicit_feedback_tangent(
                self.plan.h, self._ptr(self.state), self._ptr(dxd), int(D), t_start, float(h), int(n_steps), int(n_iter), hold,
                self._ptr(K), self._ptr(ref), C.byref(fbt), C.byref(desc), C.byref(tan), self._ptr(u_out), self._ptr(du_out),
                self._ptr(work), C.byref(t_end), self._stream())
        out = self._tangent_launch(call, dx, single, t0, keep + [K, ref, dK, dr])
        self._keep += [u_out, du_out, work]
        if not return_control:
            return out
        return out, (self._unpack_controls(u_out, n_steps, hold), self._unpack_controls(du_out, n_steps, hold))

    def linearize_implicit_feedback(self, h: float, gain, reference=None, hold: int = 1, n_samples: int = 1, n_iter: int = 2,
                                    x_red=None, held_force=None):
        """The sampled linearisation of the digital loop: (Phi_cl [B, 2n, 2n], G_ref [B, 2n, 2n]), the Jacobians of the state
        after ``n_samples`` samples of ``step_implicit_feedback(n_samples * hold, h, gain, reference, hold, n_iter,
        held_force=held_force)`` with respect to the state it starts from and to the reference -- on a linear rod
        A_d - B_d K and B_d K of ``linearize_implicit(h, hold, n_iter)``; on the nonlinear rod, in water and under gravity,
        the closed loop's state-transition matrix about any operating point, whose spectral radius says whether the
        regulator designed on (A_d, B_d) is stable on the plant the stepper applies (examples/closed_loop_margin.py).  Taken
        at (``x_red`` [B, 2n], ``held_force`` [B, n]); None = the resident state and 0.  Two calls of
        crb_step_implicit_feedback_tangent with identity seeds (2n state, 2n reference directions) on a copy: ``state``,
        ``time`` and ``status`` are untouched."""
        who = "linearize_implicit_feedback"
        if int(n_samples) != n_samples or int(n_samples) < 1:
            raise ValueError(f"{who}: n_samples must be an integer >= 1")
        hold = self._hold(hold, who)
        B, n = self.n_beams, self.n
        n_steps = int(n_samples) * hold
        x0 = self.state.clone() if x_red is None else self.pack_state(x_red)
        held = None if held_force is None else self._dev(held_force, (B, n))
        eye2 = torch.eye(2 * n, dtype=self.dtype, device=self.device)[:, None, :].expand(2 * n, B, 2 * n)
        zero = torch.zeros((2 * n, B, 2 * n), dtype=self.dtype, device=self.device)
        return self._jacobians_on_a_copy(
            x0,
            lambda: self.step_implicit_feedback_tangent(n_steps, h, eye2, gain, reference, hold, n_iter, held_force=held, t0=0.0),
            lambda: self.step_implicit_feedback_tangent(n_steps, h, zero, gain, reference, hold, n_iter, d_reference=eye2,
                                                        held_force=held, t0=0.0))

    def step_implicit(self, n_steps: int, h: float, n_iter: int = 2, impulse_amp=None, impulse_duration: float = 0.01,
                      impulse_index: int = -2, held_force=None, t0: Optional[float] = None, record=None,
                      record_every: int = 1, rho_inf: float = 1.0, control=None, control_hold: Optional[int] = None):
        """Advance the resident state by ``n_steps`` steps of size ``h`` of the implicit midpoint rule in one launch
        (crb_step_implicit): the stiff end of the reference's call sites -- the examples integrate 1 s with
        ``solve_ivp(method="LSODA")`` (example_utilities.py:153-159) because explicit steppers are limited to
        dt <= ~7e-5 s; here h = 1e-3 ... 1e-4 s is stable.  ``n_iter`` modified-Newton iterations per step (2
        reproduces the converged step); inputs are sampled at the step midpoint.  ``record`` as in ``step``.
        Displacements converge at second order in h; velocity components of modes with |lambda| h >> 1 are not
        resolved (amplitude kept, phase not).  ``rho_inf`` < 1: the numerically damped member of the family
        (generalised-alpha, crb_step_implicit_damped) -- those modes lose the factor ``rho_inf`` per step instead, as
        they do under LSODA's BDF formulas; 0 removes them within a step or two, 1 is the midpoint rule.
        ``control`` [K, B, n] / ``control_hold`` (or ``held_force=ControlSchedule(control, hold)``): a piecewise-constant control
        sequence as in ``step``, vector k held for ``control_hold`` implicit steps, switched inside the kernel
        (crb_step_implicit_sched) -- bitwise the chain of one call per interval with ``held_force=control[k]``.  Every call
        starts its first step's iteration from 0, so every interval's first step does: a sequence of K equal vectors is the
        chain of K calls, not bitwise the one held-force call (they differ by the iteration's convergence error).  Not
        together with ``held_force`` [B, n]; not with ``rho_inf`` < 1 (NotImplementedError)."""
        held_force, sch = self._control(held_force, control, control_hold, n_steps, "step_implicit", "implicit steps")
        if sch is not None and float(rho_inf) < 1.0:
            raise NotImplementedError("step_implicit: the damped variant (rho_inf < 1) has no scheduled form")
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        rec, samples = self._record_desc(record, n_steps, record_every)
        keep.append(samples)
        t_end = C.c_double(0.0)
        if sch is not None:
            sd, packed = self._sched_desc(sch)
            keep.append(packed)
            with self._on_device():
                nat.check(self._lib.crb_step_implicit_sched(self.plan.h, self._ptr(self.state), self.time, float(h), int(n_steps),
                                                            int(n_iter), C.byref(desc), C.byref(sd), self._ref(rec),
                                                            C.byref(t_end), self._stream()))
            self._keep = keep
            self.time = t_end.value
            return (self.time, samples) if record is not None else self.time
        with self._on_device():
            nat.check(self._lib.crb_step_implicit_damped(self.plan.h, self._ptr(self.state), self.time, float(h), int(n_steps),
                                                         int(n_iter), float(rho_inf), C.byref(desc),
                                                         C.byref(rec) if rec is not None else None, C.byref(t_end), self._stream()))
        self._keep = keep
        self.time = t_end.value
        return (self.time, samples) if record is not None else self.time

    def step_implicit_feedback(self, n_steps: int, h: float, gain, reference=None, hold: int = 1, n_iter: int = 2,
                               impulse_amp=None, impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                               t0: Optional[float] = None, record=None, record_every: int = 1, return_control: bool = False):
        """A digital (sampled-data) state-feedback loop in ONE native call (crb_step_implicit_feedback): ``n_steps`` implicit
        midpoint steps of size ``h``; every ``hold`` steps the controller samples the state as it stands and holds
        u_k = held_force + K (r - x_k) until the next sample (zero-order hold), the tip impulse on top -- the loop that
        examples/digital_lqr.py closes from Python with unpack_state(), a matmul and step_implicit(hold, h, held_force=u) per
        sample, and exactly the chain of those calls.  The held input is constant over a step, so the iteration matrix is the
        open loop's and the loop is as stable at h = 1e-4 ... 1e-3 s as the open loop is (``step_feedback`` evaluates
        u = K (r - x) inside the RK4 stages and needs dt <= ~8e-6 s).

        gain       [n, 2n], reduced ordering (e.g. from ``linearize_implicit`` and a discrete Riccati solve), one gain for the
                   whole ensemble (a list of gains raises NotImplementedError)
        reference  [B, 2n] or None (= regulation to 0)
        hold       implicit steps per controller sample (>= 1); the last sample may be cut short by ``n_steps``
        record     as in ``step_implicit``; ``record_every`` must divide ``hold`` or be a multiple of it
        Returns ``time``, then ``samples`` when ``record`` is given, then ``control`` [K, B, n] (K = ceil(n_steps / hold),
        reduced ordering: the held input of every sample) when ``return_control`` is set -- ``ControlSchedule(control, hold)``
        replays the call through ``step_implicit``.  ``implicit_feedback_path()`` says which form runs.  fp64 ensembles with
        one free-DOF set."""
        who = "step_implicit_feedback"
        if isinstance(gain, (list, tuple)):
            raise NotImplementedError(f"{who}: a list of gains (per-beam or grouped gains) is not available in the implicit closed "
                                      f"loop; pass one [{self.n}, {2 * self.n}] gain for the whole ensemble")
        hold = self._hold(hold, who)
        K = torch.as_tensor(gain, dtype=self.dtype, device=self.device).contiguous()
        if tuple(K.shape) != (self.n, 2 * self.n):
            raise ValueError(f"{who}: gain must be [{self.n}, {2 * self.n}], got {tuple(K.shape)}")
        ref = None
        if reference is not None:
            ref = torch.as_tensor(reference, dtype=self.dtype, device=self.device).contiguous()
            if tuple(ref.shape) != (self.n_beams, 2 * self.n):
                raise ValueError(f"{who}: reference must be [{self.n_beams}, {2 * self.n}], got {tuple(ref.shape)}")
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        rec, samples = self._record_desc(record, n_steps, record_every)
        u_out = self._control_records(n_steps, hold) if return_control else None
        nbytes = int(self._lib.crb_implicit_feedback_work_bytes(self.plan.h))
        work = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=self.device)
        t_end = C.c_double(0.0)
        with self._on_device():
            nat.check(self._lib.crb_step_implicit_feedback(self.plan.h, self._ptr(self.state), self.time, float(h), int(n_steps),
                                                           int(n_iter), hold, self._ptr(K), self._ptr(ref), C.byref(desc),
                                                           self._ref(rec), self._ptr(u_out), self._ptr(work), C.byref(t_end),
                                                           self._stream()))
        self._keep = keep + [samples, K, ref, u_out, work]
        self.time = float(t_end.value)
        out = (self.time,)
        if record is not None:
            out += (samples,)
        if return_control:
            out += (self._unpack_controls(u_out, n_steps, hold),)
        return out if len(out) > 1 else self.time

    def implicit_feedback_path(self) -> str:
        """Which form ``step_implicit_feedback`` takes for this ensemble: "in-kernel" (beams of one wave whose gain fits LDS: the
        whole call is one launch) or "chain" (per sample one ensemble GEMM and one launch of the implicit stepper)."""
        return {0: "chain", 1: "in-kernel"}[int(self._lib.crb_implicit_feedback_path(self.plan.h))]

    def solve_ivp(self, t_span, t_eval, method: str = "LSODA", impulse_amp=None, impulse_duration: float = 0.01,
                  impulse_index: int = -2, held_force=None, substeps: Union[int, str, None] = None,
                  rtol: float = 1e-3, atol: float = 1e-6, control: str = "all", gain=None, reference=None,
                  controller: str = "auto", rho_inf: float = 1.0):
        """The examples' integration call for the whole ensemble (examples/example_utilities.py:153-159:
        ``solve_ivp(f, t_span, x0, method="LSODA", t_eval=np.arange(t0, t1, DT))``) from the RESIDENT state, with the
        examples' forcing.  ``t_eval`` must be a uniform grid starting at ``t_span[0]`` (what ``np.arange`` gives).

        method   "LSODA" / "BDF" / "Radau" (the stiff solvers the examples use): the A-stable implicit stepper
                 (``step_implicit``).  ``substeps="auto"`` (the default, as the reference's call means it): the step size
                 is CONTROLLED by ``rtol`` / ``atol`` (``_solve_implicit_controlled``: every interval is integrated with
                 h and with h / 2, the difference is the error estimate, all beams take the step the worst one needs;
                 at the examples' default tolerances the whole state, velocities included, lands as close to a
                 tight-tolerance LSODA run as LSODA itself does at these tolerances -- h = 3 ... 6 us for the 10-element
                 example).  An integer: that many steps per ``t_eval`` interval, no control, one launch for the whole
                 span -- DT = 1e-3 with 10 substeps is h = 1e-4 s (displacements within the examples' tolerance band,
                 velocity content of the unresolved modes not);
                 "RK45": ``solve_rk45`` (scipy's algorithm, per-beam step control, rtol / atol) with
                 its dense output on the grid;   "RK4": the fused explicit stepper with ``substeps`` steps per interval
                 (default 10; stable for dt <= ~7e-5 s).
        gain     [n, 2n]: the CLOSED loop of examples/lqr_control.py:94-125 (``u = K (reference - x)`` inside the RHS, default
                 reference 0, plus the impulse) -- RK4 with the feedback evaluated in every stage (``step_feedback``) for
                 every method except "RK45"; the stiff methods choose its step by ``rtol`` / ``atol`` with the same
                 controller ((fine - coarse) / 15 for the fourth-order scheme; a step beyond RK4's stability limit shows
                 as a failed estimate and is halved), "RK4" takes ``substeps`` as given.
        rho_inf  (integer ``substeps`` of the stiff methods) < 1: the damped implicit scheme, see ``step_implicit``.
        controller  where the step-size control of ``substeps="auto"`` runs.  "device": inside the kernel, every beam with its
                 own step sequence, the whole span in ONE launch (``solve_controlled`` / crb_solve_controlled; the closed loop
                 with one gain for a uniform topology: held in LDS up to ~30 elements, streamed from global memory beyond);
                 "host": the same controller as a host loop
                 over fixed-step launches, the worst beam deciding for the ensemble (``_solve_controlled``; any gain, through
                 ``step_feedback``);  "device-packed" (implicit scheme, beams of 2 .. 32 thread-carried nodes): G = 64 / slots
                 beams share a wave and ONE step sequence, the worst of them deciding -- thousands of short beams fill the
                 chip with a fifth of the waves;  "auto": the device whenever it can -- for the closed loop only while the
                 gain fits the LDS, the host loop beyond --, packed once one workgroup per beam would need more than two rounds
                 of resident waves (2048).
        Returns an object with ``t`` [n_t] and ``y`` [B, 2n, n_t] (``y[b]`` is the reference's ``sol.y`` of beam b,
        first column = the state at ``t_span[0]``), ``success``, ``method``; the resident state ends at the last
        ``t_eval`` point reached by whole intervals (RK45: at ``t_span[1]``)."""
        t_eval = np.asarray(t_eval, dtype=np.float64)
        if t_eval.ndim != 1 or t_eval.size < 1 or abs(t_eval[0] - t_span[0]) > 1e-12 * max(1.0, abs(t_span[0])):
            raise ValueError("t_eval must be a 1-D grid starting at t_span[0]")
        n_t = t_eval.size
        dt_eval = float(t_eval[1] - t_eval[0]) if n_t > 1 else float(t_span[1] - t_span[0])
        if n_t > 2 and np.max(np.abs(np.diff(t_eval) - dt_eval)) > 1e-9 * dt_eval:
            raise ValueError("t_eval must be uniform (np.arange / np.linspace)")
        self.time = float(t_span[0])
        first = self.unpack_state().unsqueeze(0)                       # the state at t_span[0]
        kind = method.upper()
        if substeps is None:
            substeps = "auto" if kind in ("LSODA", "BDF", "RADAU", "IMPLICIT") else 10
        elif not isinstance(substeps, str) and int(substeps) < 1:
            raise ValueError('substeps must be a positive integer or "auto"')
        kw = dict(impulse_amp=impulse_amp, impulse_duration=impulse_duration, impulse_index=impulse_index,
                  held_force=held_force)
        stiff = kind in ("LSODA", "BDF", "RADAU", "IMPLICIT")
        if isinstance(substeps, str) and substeps != "auto":
            raise ValueError('substeps must be a positive integer or "auto"')
        if gain is not None:
            if held_force is not None or kind == "RK45" or not (stiff or kind == "RK4"):
                raise ValueError("the closed loop (gain=...) runs with the stiff methods or RK4, without a held force")
            fkw = dict(reference=reference, impulse_amp=impulse_amp, impulse_duration=impulse_duration, impulse_index=impulse_index)

            def advance(m, h, t_start, forced=None):
                self.step_feedback(m, h, gain, t0=t_start, **(fkw if forced is None else forced_input(fkw, forced)))
        else:
            def advance(m, h, t_start, forced=None):
                self.step_implicit(m, h, t0=t_start, **(kw if forced is None else forced_input(kw, forced)))

        def forced_input(args, on):
            # the controller integrates between breakpoints of the input: inside a piece the impulse is simply on or off
            # (a stage time that lands ON the switch would otherwise put a first-order error into a fourth-order step)
            args = dict(args)
            if on:
                args["impulse_duration"] = float("inf")
            else:
                args["impulse_amp"] = None
            return args

        t_switch = None if impulse_amp is None else float(impulse_duration)
        ctrl_stats = None
        if controller not in ("auto", "device", "device-packed", "host"):
            raise ValueError('controller must be "auto", "device", "device-packed" or "host"')
        if n_t == 1:
            ys = first
        elif gain is not None and not isinstance(substeps, str):
            out = [first]
            for k in range(n_t - 1):
                advance(int(substeps), dt_eval / int(substeps), float(t_span[0]) + k * dt_eval)
                out.append(self.unpack_state().unsqueeze(0))
            self.time = float(t_span[0]) + (n_t - 1) * dt_eval
            ys = torch.cat(out, dim=0)
        elif (stiff or gain is not None) and isinstance(substeps, str) and self._device_controller(controller, gain):
            snaps, stats, per_beam = self.solve_controlled(n_t - 1, dt_eval, rtol=rtol, atol=atol, control=control, gain=gain,
                                                           reference=reference, t0=float(t_span[0]),
                                                           per_wave=self._packs_per_wave(controller, gain), **kw)
            ys = torch.cat([first, self.unpack_snapshots(snaps)], dim=0)
            used = [int(v) for v in per_beam.max(axis=0)]
            ctrl_stats = (stats, per_beam)
        elif gain is not None:
            # (RK4 is only conditionally stable: start near the closed loop's limit for the Nitinol examples, 8.6e-6 s)
            ys, used = self._solve_controlled(advance, 4, max(1, int(np.ceil(dt_eval / 5e-6))), float(t_span[0]), dt_eval, n_t,
                                              first, rtol, atol, control, t_switch)
        elif stiff and isinstance(substeps, str):
            ys, used = self._solve_controlled(advance, 2, max(1, int(np.ceil(dt_eval / 1e-4))), float(t_span[0]), dt_eval, n_t,
                                              first, rtol, atol, control, t_switch)
        elif kind in ("LSODA", "BDF", "RADAU", "IMPLICIT"):
            _, snaps = self.step_implicit((n_t - 1) * int(substeps), dt_eval / int(substeps), record="all",
                                          record_every=int(substeps), rho_inf=rho_inf, **kw)
            ys = torch.cat([first, self.unpack_snapshots(snaps)], dim=0)
        elif kind == "RK4":
            if isinstance(substeps, str):
                raise ValueError("RK4 takes an integer number of substeps")
            _, snaps = self.step((n_t - 1) * int(substeps), dt_eval / int(substeps), record="all",
                                 record_every=int(substeps), **kw)
            ys = torch.cat([first, self.unpack_snapshots(snaps)], dim=0)
        elif kind == "RK45":
            st = self.solve_rk45(float(t_span[1]), rtol=rtol, atol=atol, record="all",
                                 t_eval=(float(t_eval[0]), dt_eval, n_t), **kw)
            if np.any(st["status"] != 0):
                raise RuntimeError("solve_ivp(RK45): a beam stopped before t_span[1]")
            ys = self.unpack_snapshots(st["y"])
        else:
            raise ValueError(f"unknown method {method!r}: LSODA / BDF / Radau (implicit), RK45, RK4")

        class OdeResult:   # the fields of scipy's OdeResult that the examples read
            pass

        sol = OdeResult()
        sol.t, sol.y, sol.success, sol.method = t_eval.copy(), ys.permute(1, 2, 0).contiguous(), True, kind
        if isinstance(substeps, str) and stiff and n_t > 1:
            sol.substeps = used      # steps per t_eval interval that the controller accepted (device: the most any beam took)
            if ctrl_stats is not None:
                sol.controller = "device-packed" if self._packs_per_wave(controller, gain) else "device"
                sol.substeps_per_beam = ctrl_stats[1]        # [B, n_t - 1]
                sol.doublings = ctrl_stats[0][:, 1].copy()   # repeated pieces per beam
            else:
                sol.controller = "host"
        return sol

    def _device_controller(self, controller, gain) -> bool:
        """Whether ``solve_ivp(substeps="auto")`` runs its controller inside the kernel (crb_solve_controlled's conditions)."""
        if controller == "host":
            return False
        if controller == "device-packed":
            controller = "device"
        ok = self.dtype == torch.float64 and int(self.plan.layout.threads) <= 256
        if ok and gain is not None:
            ok = not isinstance(gain, (list, tuple)) and not self.mixed_topology
            if controller == "auto":
                # (the kernel streams a gain that does not fit the LDS; "auto" keeps the host loop for those until the two are
                #  compared across ensemble sizes -- profiles/exp_ctrl_large_gain.py)
                n2p = (2 * self.n + 7) // 8 * 8
                lds = 14 * int(self.plan.layout.threads) * 8 + (n2p + n2p * self.n + 32) * 8 + 512
                ok = ok and lds <= 160 * 1024
        if controller == "device" and not ok:
            raise ValueError("controller=\"device\": fp64 plans with beams of up to 256 thread-carried nodes; the closed loop "
                             "needs one gain for a uniform topology")
        return ok

    def _packs_per_wave(self, controller, gain) -> bool:
        """Whether the device controller packs short beams G to a wave (``per_wave``): asked for, or -- "auto" -- when one
        workgroup per beam would need more than two rounds of resident waves (one wave per SIMD: 1024 waves are resident;
        4096 x 10 elements for 1 s: 0.75 s with one beam per wave, the host loop 0.28 s)."""
        lay = self.plan.layout
        can = gain is None and int(lay.beams_per_group) > 1 and int(lay.pcr_levels_full) <= 5 and int(lay.pcr_levels_full) >= 1
        if controller == "device-packed":
            if not can:
                raise ValueError("controller=\"device-packed\": implicit scheme, beams of 2 .. 32 thread-carried nodes")
            return True
        return controller == "auto" and can and self.n_beams * (int(lay.threads) // 64) > 2048

    def solve_controlled(self, n_intervals: int, dt_eval: float, rtol: float = 1e-3, atol: float = 1e-6, control: str = "all",
                         gain=None, reference=None, impulse_amp=None, impulse_duration: float = 0.01, impulse_index: int = -2,
                         held_force=None, t0: Optional[float] = None, n_iter: int = 1, first_rate: float = 0.0,
                         max_rungs: int = 0, record=True, per_wave: bool = False):
        """``n_intervals`` intervals of length ``dt_eval`` from the resident state with the step size chosen per beam by
        ``rtol`` / ``atol`` INSIDE the kernel, one launch (crb_solve_controlled, csrc/crb_ctrl.h): the implicit midpoint rule,
        or -- with ``gain`` -- RK4 with the feedback in every stage.  ``n_iter``: modified-Newton iterations per implicit step (1: at
        the controller's step sizes the previous step's iterate is converged after one, profiles/exp_niter.py).  Returns (snapshots [n_intervals, B, 2, n_node, 4] or
        None -- or, with ``record=(node, param)``, that DOF's series [B, n_intervals] --, stats [B, 4] (fine steps accepted,
        doublings, status, last rung), steps per beam and interval [B, n_intervals]); raises when a beam could not meet the
        tolerances."""
        if control not in ("all", "positions"):
            raise ValueError('control must be "all" or "positions"')
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        K = None if gain is None else self._dev(gain, (self.n, 2 * self.n))
        ref = None if reference is None else self._dev(reference, (self.n_beams, 2 * self.n))
        n_intervals = int(n_intervals)
        # record: True = whole-state snapshots, False = none, (node, param) = that DOF's series [B, n_intervals] instead (what the
        # examples read; param "w" / "dw_dt" ...): the first return value is then the series
        series, sp, sn, sd = None, 0, 0, 0
        if isinstance(record, tuple):
            node, param = record
            vel = param.startswith("d") and param.endswith("_dt")
            sp, sn, sd = int(vel), int(node), _PARAM[param[1:-3] if vel else param]
            series = torch.zeros((self.n_beams, max(n_intervals, 1)), dtype=self.dtype, device=self.device)
        ctl = nat.ControlDesc(float(rtol), float(atol), float(first_rate), int(control == "positions"), int(n_iter), int(max_rungs),
                              int(bool(per_wave)), sp, sn, sd, 0, series.data_ptr() if series is not None else None)
        snaps = torch.zeros((n_intervals,) + tuple(self.state.shape), dtype=self.dtype, device=self.device) if record is True else None
        stats = torch.zeros((self.n_beams, 4), dtype=torch.int32, device=self.device)
        used = torch.zeros((self.n_beams, max(n_intervals, 1)), dtype=torch.int32, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_solve_controlled(self.plan.h, self._ptr(self.state), self.time, float(dt_eval), n_intervals,
                                                     C.byref(ctl), C.byref(desc), self._ptr(K), self._ptr(ref), self._ptr(snaps),
                                                     self._ptr(stats), self._ptr(used), self._stream()))
        self._keep = keep + [K, ref, snaps, stats, used, series]
        st = stats.cpu().numpy()
        if np.any(st[:, 2] != 0):
            bad = int(np.flatnonzero(st[:, 2] != 0)[0])
            raise RuntimeError(f"solve_controlled: the tolerances ask for more steps per interval than the ladder holds "
                               f"(beam {bad}; {int(np.count_nonzero(st[:, 2]))} beams in all)")
        self.time = self.time + n_intervals * float(dt_eval)
        return (series[:, :n_intervals] if series is not None else snaps), st, used.cpu().numpy()[:, :n_intervals]

    def _solve_controlled(self, advance, order, m_first, t0, dt_eval, n_t, first, rtol, atol, control, t_switch=None,
                          max_substeps=1 << 14):
        """Step-size control by step doubling for a fixed-step scheme of the given order (``advance(m, h, t, on)`` takes m
        steps of size h from the resident state at time t with the impulse on or off: the implicit midpoint rule, order
        2, or the closed-loop RK4, order 4): every ``t_eval`` interval -- cut in two at ``t_switch``, the end of the
        impulse, when that falls inside it -- is integrated from the same state with m steps and with 2m steps;
        (fine - coarse) / (2^order - 1)
        estimates the error of the fine solution, which is measured like scipy measures its own (RMS over a beam's state
        of err / (atol + rtol |y|), tolerances of the reference's call, example_utilities.py:153-159 /
        lqr_control.py:117-125) -- the worst beam decides for the ensemble.  Above 1 the interval is repeated with
        twice the steps (the fine solution becomes the coarse one; so is an estimate that is not finite -- an explicit
        scheme beyond its stability limit), the accepted solution is the fine one; an estimate far below 1 halves m for
        the next interval.  ``control="positions"`` measures the position half of the state
        only (velocity components of modes far above 1 / h keep their amplitude but not their phase, which the full
        norm answers with the small steps LSODA itself takes).  Returns (states [n_t, B, 2n], accepted m per interval)."""
        if control not in ("all", "positions"):
            raise ValueError('control must be "all" or "positions"')
        n_dof = torch.as_tensor(np.asarray(self.n_per_beam, dtype=np.float64) * (2.0 if control == "all" else 1.0),
                                dtype=torch.float64, device=self.device)
        rows = slice(None) if control == "all" else slice(0, 1)

        def estimate(fine, coarse, start):
            scale = atol + rtol * torch.maximum(fine[:, rows].abs(), start[:, rows].abs())
            e = ((fine[:, rows] - coarse[:, rows]) / (float(2 ** order - 1) * scale)).double()
            return float(torch.sqrt((e * e).sum(dim=(1, 2, 3)) / n_dof).max().item())

        def run(start, t_a, length, on, m):
            self.state = start.clone()
            advance(m, length / m, t_a, on)
            return self.state

        rate = float(m_first) / dt_eval       # steps per second of the coarse solution; doubled / halved by the controller
        shrink = 0.8 / float(2 ** order)      # half the steps multiply the estimate by 2^order: still below 1 with margin
        out, used = [first], []
        for k in range(n_t - 1):
            t_k, t_n = t0 + k * dt_eval, t0 + (k + 1) * dt_eval
            pieces = [(t_k, t_n)]
            if t_switch is not None and t_k + 1e-9 * dt_eval < t_switch < t_n - 1e-9 * dt_eval:
                pieces = [(t_k, t_switch), (t_switch, t_n)]
            taken = 0
            for t_a, t_b in pieces:
                on = None if t_switch is None else (0.5 * (t_a + t_b) < t_switch)
                m = max(1, int(np.ceil(rate * (t_b - t_a) - 1e-9)))
                start = self.state
                coarse = run(start, t_a, t_b - t_a, on, m)
                while True:
                    fine = run(start, t_a, t_b - t_a, on, 2 * m)
                    err = estimate(fine, coarse, start)
                    if err <= 1.0:
                        break
                    m, coarse, rate = 2 * m, fine, 2.0 * rate
                    if 2 * m > max_substeps:
                        raise RuntimeError(f"solve_ivp: the tolerances ask for more than {max_substeps} steps per t_eval "
                                           f"interval at t = {t_a:.6g} s (error estimate {err:.3g})")
                taken += 2 * m
                self.state = fine
                if err < shrink * 0.25 and m > 1:
                    rate *= 0.5
            used.append(taken)
            self.time = t_n
            out.append(self.unpack_state().unsqueeze(0))
        return torch.cat(out, dim=0), used

    def solve_rk45(self, t_end: float, rtol: float = 1e-3, atol: float = 1e-6, impulse_amp=None,
                   impulse_duration: float = 0.01, impulse_index: int = -2, held_force=None,
                   first_step=None, t0: Optional[float] = None, max_steps: int = 0, record=None, t_eval=None):
        """Integrate every beam from the current clock to ``t_end`` with adaptive Dormand-Prince 5(4),
        per-beam step control, in ONE kernel launch -- the algorithm (and defaults) of
        ``scipy.integrate.solve_ivp(method="RK45")`` that the reference's tests call
        (tests/test_dynamic_beam.py:218-220).  Returns a dict of per-beam statistics:
        accepted / rejected steps, nfev, status (0 = reached t_end), next_step.

        record=(node, param) with t_eval=(start, step, count): also returns "y" [B, count], that DOF on the
        uniform grid start + k*step by scipy's dense output; record="all": "y" is the whole state on the grid,
        [count, B, 2, n_node, 4] (unpack_snapshots() gives the reduced ordering) (what ``sol.y[i]`` holds when solve_ivp is
        given ``t_eval=np.arange(...)``, example_utilities.py:158)."""
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index, held_force)
        h = torch.zeros((self.n_beams,), dtype=torch.float64, device=self.device)
        if first_step is not None:
            h += torch.as_tensor(first_step, dtype=torch.float64, device=self.device)
        stats = torch.zeros((self.n_beams, 4), dtype=torch.int32, device=self.device)
        grid = (0.0, 0.0, 0) if record is None else (float(t_eval[0]), float(t_eval[1]), int(t_eval[2]))
        rec, ys = self._record_desc(record, grid[2])
        with self._on_device():
            nat.check(self._lib.crb_solve_rk45_eval(self.plan.h, self._ptr(self.state), self.time, float(t_end), float(rtol),
                                                    float(atol), C.byref(desc), self._ptr(h), self._ptr(stats),
                                                    int(max_steps), C.byref(rec) if rec is not None else None, grid[0],
                                                    grid[1], grid[2], self._stream()))
        self._keep = keep + [h, stats, ys]
        st = stats.cpu().numpy()
        out = {"accepted": st[:, 0], "rejected": st[:, 1], "nfev": st[:, 2], "status": st[:, 3],
               "next_step": h.cpu().numpy()}
        if np.any(st[:, 3] != 0):
            # a beam that gave up (step too small / max_steps) stopped BEFORE t_end: the ensemble no longer has one
            # clock, so the clock is not advanced and the caller is told (scipy reports status -1 the same way)
            import warnings

            bad = np.nonzero(st[:, 3] != 0)[0]
            warnings.warn(f"solve_rk45: {bad.size} of {self.n_beams} beams stopped before t_end (first: beam {int(bad[0])}); "
                          "ensemble clock left unchanged", RuntimeWarning, stacklevel=2)
        else:
            self.time = float(t_end)
        if ys is not None:
            out["y"] = ys
        return out

    def step_feedback(self, n_steps: int, dt: float, gain, reference=None, impulse_amp=None,
                      impulse_duration: float = 0.01, impulse_index: int = -2, t0: Optional[float] = None) -> float:
        """Closed-loop rollout: RK4 with the state feedback u = K (r - x) evaluated inside the RHS at
        EVERY stage, as examples/lqr_control.py:95-111 does through FullStateLinear.compute_input
        (control/full_state_linear.py:81), plus the optional tip impulse.

        gain       [n, 2n] LQR gain (reduced ordering, e.g. LinearQuadraticRegulator.compute_gain_matrix()) for the whole
                   ensemble, or a list of B matrices (None = no feedback for that beam): one gain per beam of a heterogeneous
                   ensemble, each in its own beam's reduced ordering; equal gains on like beams run as one group
        reference  [B, 2n] or None (= regulation to 0)
        Stage-split path: per stage one GEMM over the whole ensemble, [B, 2n] x [2n, n] -- the fused
        MFMA kernel crb_feedback_force (gather + GEMM + scatter, in the plan's dtype) -- then one launch
        of the stage kernel (crb_rk4_stage); the loop itself is crb_step_rk4_feedback.
        Note: the LQR loop is stiff (|lambda|max ~ 3e5 1/s for the Nitinol example): RK4 needs
        dt <= ~8e-6 s, not the 2e-5 s of the open-loop configs.
        """
        if t0 is not None:
            self.time = float(t0)
        if isinstance(gain, (list, tuple)):
            return self._step_feedback_grouped(n_steps, dt, gain, reference, impulse_amp, impulse_duration, impulse_index)
        K = self._dev(gain, (self.n, 2 * self.n))
        ref = None if reference is None else self._dev(reference, (self.n_beams, 2 * self.n))
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index)
        # the whole loop is one native call (crb_step_rk4_feedback issues every launch)
        work = torch.empty((int(self._lib.crb_feedback_work_bytes(self.plan.h)),), dtype=torch.uint8, device=self.device)
        t_end = C.c_double(0.0)
        with self._on_device():
            nat.check(self._lib.crb_step_rk4_feedback(self.plan.h, self._ptr(self.state), self.time, float(dt), int(n_steps),
                                                      self._ptr(K), self._ptr(ref), C.byref(desc), self._ptr(work),
                                                      C.byref(t_end), self._stream()))
        self._keep = keep + [K, ref, work]
        self._feedback_work = work
        self.time = float(t_end.value)
        return self.time

    def _gain_groups(self, gains):
        """Per-beam gains -> (group of every beam, one device gain per group): beams with the same free-DOF set and an equal gain
        matrix form a group (the reference designs one gain per model, lqr_control.py:46-84); None = no feedback for that beam."""
        if len(gains) != self.n_beams:
            raise ValueError(f"per-beam gains: expected {self.n_beams} matrices, got {len(gains)}")
        index, group_of, mats = {}, np.full(self.n_beams, -1, dtype=np.int32), []
        for b, K in enumerate(gains):
            if K is None:
                continue
            K = np.ascontiguousarray(K, dtype=np.float64)
            nb = int(self.n_per_beam[b])
            if K.shape != (nb, 2 * nb):
                raise ValueError(f"gain of beam {b}: expected shape {(nb, 2 * nb)} (its own reduced state), got {K.shape}")
            key = (self.free_index_per_beam[b].tobytes(), K.tobytes())
            if key not in index:
                index[key] = len(mats)
                mats.append(torch.as_tensor(K, dtype=self.dtype, device=self.device).contiguous())
            group_of[b] = index[key]
        if not mats:
            raise ValueError("per-beam gains: every entry is None")
        return group_of, mats

    def _step_feedback_grouped(self, n_steps, dt, gains, reference, impulse_amp, impulse_duration, impulse_index):
        """step_feedback with one gain per beam (heterogeneous ensembles, `from_dataframes`): grouped by free-DOF set and gain,
        one MFMA launch per group and stage (crb_step_rk4_feedback_grouped).  `reference`: [B, 2 n_max] padded reduced states."""
        group_of, mats = self._gain_groups(gains)
        ref = None if reference is None else self._dev(reference, (self.n_beams, 2 * self.n))
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index)
        ptrs = (C.c_void_p * len(mats))(*[m.data_ptr() for m in mats])
        work = torch.empty((int(self._lib.crb_feedback_work_bytes(self.plan.h)),), dtype=torch.uint8, device=self.device)
        t_end = C.c_double(0.0)
        with self._on_device():
            nat.check(self._lib.crb_step_rk4_feedback_grouped(
                self.plan.h, self._ptr(self.state), self.time, float(dt), int(n_steps), len(mats),
                group_of.ctypes.data_as(C.POINTER(C.c_int32)), ptrs, self._ptr(ref), C.byref(desc), self._ptr(work), C.byref(t_end),
                self._stream()))
        self._keep = keep + mats + [ref, work]
        self._feedback_work = work
        self.time = float(t_end.value)
        return self.time

    def feedback_path(self) -> str:
        """Which form `step_feedback` takes for this ensemble: "persistent" (one launch per rollout, csrc/crb_loop.h), "fused"
        (small beams, gain in LDS) or "stage-split" (one GEMM + one stage launch per RK4 stage)."""
        return {0: "stage-split", 1: "fused", 2: "persistent"}[int(self._lib.crb_feedback_path(self.plan.h))]

    def feedback_status(self) -> int:
        """0, or which hand-off of the last `step_feedback` gave up (the persistent stepper's workgroups wait for each
        other with a time limit instead of hanging the device; the state is unusable then).  Synchronises the stream."""
        work = getattr(self, "_feedback_work", None)
        if work is None:
            return 0
        status = C.c_int32(0)
        with self._on_device():
            nat.check(self._lib.crb_feedback_status(self.plan.h, self._ptr(work), C.byref(status), self._stream()))
        return int(status.value)

    # ------------------------------------------------------------------ functional composition
    def _plan_with(self, drag_on: bool, gravity_on: bool):
        """The ensemble's plan with the built-in drag / gravity terms of the RHS kernel switched on or off."""
        key = (bool(drag_on), bool(gravity_on))
        if key not in self._plans:
            fps, per = self._fps, len(self._fps) > 1
            pick = (lambda f: [f(p) for p in fps]) if per else (lambda f: f(fps[0]))
            with self._on_device():
                self._plans[key] = nat.Plan(
                    self.columns, fluid_density=pick(lambda p: p.fluid_density),
                    enable_fluid=pick(lambda p: bool(p.enable_fluid_effects and drag_on)),
                    gravity=pick(lambda p: p.get_gravity_vector()),
                    enable_gravity=pick(lambda p: bool(p.enable_gravity_effects and gravity_on)), **self._plan_args)
        return self._plans[key]

    def step_composed(self, n_steps: int, dt: float, forces_func=None, u=None, impulse_amp=None,
                      impulse_duration: float = 0.01, impulse_index: int = -2, t0: Optional[float] = None) -> float:
        """RK4 with the reference's functional force composition, batched (dynamic_beam_model.py:243-274, 343-362):
        xdot = [v ; Minv(-k(q) + forces(x, 0.0) + u(t))] with

        forces_func  ``callable(x[B, 2n], t) -> [B, n]`` (torch, on the ensemble's device) used INSTEAD of the registry,
                     as ``create_system_func(forces_func)`` does (:253-254), called with t = 0.0 (:265, quirk B-3);
                     None: the aggregate of ``self.force_registry`` -- the enabled built-in drag / gravity markers run
                     fused inside the RHS kernel, every other enabled component (``compute_forces(x, t)``, e.g. the
                     reference's StateAwareForce, tests/test_advanced_composition.py:36-65) is summed on the device;
                     ``enabled`` is re-read at EVERY evaluation (force_registry.py:66-67)
        u            ``[B, n]`` held input, or ``callable(t) -> [B, n]`` evaluated at every stage time (:357-360)
        impulse_*    the examples' tip impulse on top (as in ``step``).

        Stage-split path: per stage the state is unpacked to the reduced ordering, the callables run as torch ops,
        and one crb_rk4_stage launch takes their sum as its input force.  Returns the clock (accumulated by addition).
        """
        if t0 is not None:
            self.time = float(t0)
        desc, keep = self._input_desc(impulse_amp, impulse_duration, impulse_index)
        acc, bufs = torch.empty_like(self.state), (torch.empty_like(self.state), torch.empty_like(self.state))
        zeros = torch.zeros((self.n_beams, self.n_node, 4), dtype=self.dtype, device=self.device)
        u_held = None if (u is None or callable(u)) else self._dev(u, (self.n_beams, self.n))
        t = self.time
        dt = float(dt)
        with self._on_device():
            for _ in range(int(n_steps)):
                cur = self.state
                for s, ts in enumerate((t, t + 0.5 * dt, t + 0.5 * dt, t + dt)):   # crb_step_rk4's clock convention
                    total = None
                    if forces_func is not None:
                        plan = self._plan_with(False, False)
                        total = self._force_tensor(forces_func(self.unpack_state(cur), 0.0))
                    else:
                        drag_on = grav_on = False
                        x_red = None
                        for force in self.force_registry.get_registered_forces():
                            if not force.is_enabled():
                                continue
                            if force is self._auto_drag:
                                drag_on = True
                            elif force is self._auto_gravity:
                                grav_on = True
                            else:
                                if x_red is None:
                                    x_red = self.unpack_state(cur)
                                part = self._force_tensor(force.compute_forces(x_red, 0.0))
                                total = part.clone() if total is None else total + part
                        plan = self._plan_with(drag_on, grav_on)
                    if u is not None:
                        ut = self._force_tensor(u(ts)) if callable(u) else u_held
                        total = ut if total is None else total + ut
                    u_stage = zeros if total is None else self.pack_vec(total)
                    nxt = bufs[s & 1]
                    nat.check(self._lib.crb_rk4_stage(plan.h, self._ptr(self.state), self._ptr(cur), self._ptr(acc),
                                                      self._ptr(nxt), self._ptr(u_stage), s, float(ts), dt, C.byref(desc),
                                                      self._stream()))
                    cur = nxt
                t = t + dt
        self._keep = keep + [acc, bufs, zeros]
        self.time = t
        return self.time

    def _force_tensor(self, f) -> torch.Tensor:
        """A user callable's result as a [B, n] tensor of the ensemble's dtype and device; the wrong shape is a
        ValueError (the reference's M_inv.dot raises a dimension mismatch, dynamic_beam_model.py:270)."""
        f = torch.as_tensor(f, dtype=self.dtype, device=self.device)
        if tuple(f.shape) != (self.n_beams, self.n):
            raise ValueError(f"dimension mismatch: force of shape {tuple(f.shape)} for {(self.n_beams, self.n)} position DOFs")
        return f.contiguous()

    def gather(self, node: int, param: str, velocity: bool = False) -> torch.Tensor:
        out = torch.empty((self.n_beams,), dtype=self.dtype, device=self.device)
        with self._on_device():
            nat.check(self._lib.crb_gather_dof(self.plan.h, self._ptr(self.state), int(velocity), int(node),
                                               _PARAM[param], self._ptr(out), self._stream()))
        return out

    def tip_displacement(self) -> torch.Tensor:
        """w of the last node of every beam (the examples' 'tip displacement', lqr_control.py:168)."""
        if len(set(self.n_elem_per_beam.tolist())) == 1:
            return self.gather(self.n_elem, "w")
        rows = torch.arange(self.n_beams, device=self.device)      # beams of different length: each beam's own last node
        nodes = torch.as_tensor(self.n_elem_per_beam, device=self.device)
        return self.state[rows, 0, nodes, 1].clone()


class _AdjointFamily(NamedTuple):
    """What differs between the checkpointed adjoints that BeamEnsemble._rollout_adjoint, _checkpoint_pass, _sweep and the
    rollout Functions serve.  ``step`` is the family's own tuple of step arguments, opaque to the shared code; the callables
    take the ensemble first."""
    who: str              # the public method's name in error texts
    prepare: object       # (ens, n_steps, args, held_force, impulse_amp, record) -> (step, held_force, schedule, want)
    ckpt_shape: object    # (ens) -> the shape of one segment's checkpoint
    work_bytes: object    # (ens, every, step, n_cot) -> the library's work-bytes call
    checkpoint: object    # (ens, x, ckpt, n_steps, every, t0, step, desc, sd, rec, t_end) -> (return code, what it allocated)
    outputs: object       # (ens, D, want, sd) -> the cotangent buffers of the sweep, the optional one (``want``) first
    sweep: object         # (ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work) -> return code
    unpack: object        # (ens, outs, sd) -> the returns after xbar0, each with its leading D axis


def _first(v):
    """one return of _rollout_adjoint without its leading D axis (a dict of them entry by entry)"""
    if isinstance(v, dict):
        return {k: t[0] for k, t in v.items()}
    return None if v is None else v[0]


def _input_outputs(ens, D, want_amp, sd):
    """[amp_bar [D, B] or None, f_bar [D, B, n_node, 4] -- with a schedule its cotangent, [D, K, B, n_node, 4]]"""
    amp_bar = torch.zeros((D, ens.n_beams), dtype=ens.dtype, device=ens.device) if want_amp else None
    f_bar = torch.zeros((D,) + (() if sd is None else (int(sd.n_intervals),)) + (ens.n_beams, ens.n_node, 4),
                        dtype=ens.dtype, device=ens.device)
    return [amp_bar, f_bar]


def _input_cotangent(ens, outs, sd):
    """(crb_input_cotangent, sched_bar) of _input_outputs: f_bar is grad.f_held_bar without a schedule, sched_bar with one"""
    grad = nat.InputCotangent()
    grad.amp_bar = outs[0].data_ptr() if outs[0] is not None else None
    grad.f_held_bar = outs[1].data_ptr() if sd is None else None
    return grad, ens._ptr(outs[1] if sd is not None else None)


def _input_unpack(ens, outs, sd):
    return outs[0], (ens._unpack_force_dirs(outs[1]) if sd is None else ens._unpack_sched_dirs(outs[1]))


def _rk4_prepare(ens, n_steps, args, held_force, impulse_amp, record):
    dt, control, control_hold = args
    held_force, sch = ens._control(held_force, control, control_hold, n_steps, "step_adjoint")
    return (dt,), held_force, sch, impulse_amp is not None


def _rk4_checkpoint(ens, x, ckpt, n_steps, every, t0, step, desc, sd, rec, t_end):
    return ens._lib.crb_step_rk4_checkpoint_sched(ens.plan.h, ens._ptr(x), t0, float(step[0]), n_steps, every, C.byref(desc),
                                                  ens._ref(sd), ens._ref(rec), ens._ptr(ckpt), C.byref(t_end),
                                                  ens._stream()), None


def _rk4_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    grad, sched_bar = _input_cotangent(ens, outs, sd)
    return ens._lib.crb_step_rk4_adjoint_sched(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), int(lamd.shape[0]), t0,
                                               float(step[0]), n_steps, every, C.byref(desc), ens._ref(rec_bar), C.byref(grad),
                                               ens._ref(sd), sched_bar, ens._ptr(work), ens._stream())


def _rk4_params_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    grad, sched_bar = _input_cotangent(ens, outs, sd)
    pgrad = nat.ParamCotangent()
    pgrad.param_bar = outs[2].data_ptr()
    return ens._lib.crb_step_rk4_adjoint_params_sched(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), int(lamd.shape[0]), t0,
                                                      float(step[0]), n_steps, every, C.byref(desc), ens._ref(rec_bar),
                                                      C.byref(grad), C.byref(pgrad), ens._ref(sd), sched_bar, ens._ptr(work),
                                                      ens._stream())


_RK4 = _AdjointFamily(
    who="step_adjoint", prepare=_rk4_prepare, ckpt_shape=lambda ens: tuple(ens.state.shape),
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_rk4_adjoint_work_bytes(ens.plan.h, every),
    checkpoint=_rk4_checkpoint, outputs=_input_outputs, sweep=_rk4_sweep, unpack=_input_unpack)

# step_adjoint_params: the same pass, the storing sweep, and a third buffer param_bar [D, B, n_node, 8] returned as a dict
_RK4_PARAMS = _RK4._replace(
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_rk4_adjoint_params_work_bytes(ens.plan.h, every, n_cot),
    outputs=lambda ens, D, want_amp, sd: _input_outputs(ens, D, want_amp, sd) + [
        torch.zeros((D, ens.n_beams, ens.n_node, 8), dtype=ens.dtype, device=ens.device)],
    sweep=_rk4_params_sweep,
    unpack=lambda ens, outs, sd: _input_unpack(ens, outs, sd) + (ens._param_dict(outs[2]),))


def _implicit_prepare(ens, n_steps, args, held_force, impulse_amp, record):
    h, n_iter, control, control_hold = args
    held_force, sch = ens._control(held_force, control, control_hold, n_steps, "step_implicit_adjoint", "implicit steps")
    return (h, n_iter), held_force, sch, impulse_amp is not None


def _implicit_checkpoint(ens, x, ckpt, n_steps, every, t0, step, desc, sd, rec, t_end):
    return ens._lib.crb_step_implicit_checkpoint_sched(ens.plan.h, ens._ptr(x), t0, float(step[0]), n_steps, int(step[1]), every,
                                                       C.byref(desc), ens._ref(sd), ens._ref(rec), ens._ptr(ckpt),
                                                       C.byref(t_end), ens._stream()), None


def _implicit_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    grad, sched_bar = _input_cotangent(ens, outs, sd)
    return ens._lib.crb_step_implicit_adjoint_sched(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), int(lamd.shape[0]), t0,
                                                    float(step[0]), n_steps, int(step[1]), every, C.byref(desc),
                                                    ens._ref(rec_bar), C.byref(grad), ens._ref(sd), sched_bar, ens._ptr(work),
                                                    ens._stream())


# step = (h, n_iter); a segment's checkpoint holds q, v and the starting iterate of its first step
_IMPLICIT = _AdjointFamily(
    who="step_implicit_adjoint", prepare=_implicit_prepare, ckpt_shape=lambda ens: (ens.n_beams, 3, ens.n_node, 4),
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_implicit_adjoint_work_bytes(ens.plan.h, every, int(step[1]), n_cot),
    checkpoint=_implicit_checkpoint, outputs=_input_outputs, sweep=_implicit_sweep, unpack=_input_unpack)


def _implicit_params_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    grad, sched_bar = _input_cotangent(ens, outs, sd)
    pgrad = nat.ParamCotangent()
    pgrad.param_bar = outs[2].data_ptr()
    return ens._lib.crb_step_implicit_adjoint_params_sched(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), int(lamd.shape[0]), t0,
                                                           float(step[0]), n_steps, int(step[1]), every, C.byref(desc),
                                                           ens._ref(rec_bar), C.byref(grad), C.byref(pgrad), ens._ref(sd),
                                                           sched_bar, ens._ptr(work), ens._stream())


# step_implicit_adjoint_params: the same pass, the storing sweep, and _RK4_PARAMS' third buffer and dict
_IMPLICIT_PARAMS = _IMPLICIT._replace(
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_implicit_adjoint_params_work_bytes(ens.plan.h, every, int(step[1]),
                                                                                               n_cot),
    outputs=_RK4_PARAMS.outputs, sweep=_implicit_params_sweep, unpack=_RK4_PARAMS.unpack)


def _feedback_prepare(ens, n_steps, args, held_force, impulse_amp, record):
    dt, gain, reference, want_gain = args
    K = ens._feedback_gain(gain, "step_feedback_adjoint")
    ref = None if reference is None else ens._dev(reference, (ens.n_beams, 2 * ens.n))
    if record is not None and isinstance(record, str):
        raise NotImplementedError("step_feedback_adjoint: whole-state snapshots (record='all') are not available in the closed loop")
    return (dt, K, ref), held_force, None, want_gain


def _feedback_checkpoint(ens, x, ckpt, n_steps, every, t0, step, desc, sd, rec, t_end):
    dt, K, ref = step
    work = ens._work_buffer(_FEEDBACK, every, step, 1)
    return ens._lib.crb_step_rk4_feedback_checkpoint(ens.plan.h, ens._ptr(x), t0, float(dt), n_steps, every, ens._ptr(K),
                                                     ens._ptr(ref), C.byref(desc), ens._ref(rec), ens._ptr(ckpt), ens._ptr(work),
                                                     C.byref(t_end), ens._stream()), work


def _feedback_outputs(ens, D, want_gain, sd):
    """[gain_bar [D, n, 2n] or None, ref_bar [D, B, 2n]]"""
    gain_bar = torch.zeros((D, ens.n, 2 * ens.n), dtype=ens.dtype, device=ens.device) if want_gain else None
    return [gain_bar, torch.zeros((D, ens.n_beams, 2 * ens.n), dtype=ens.dtype, device=ens.device)]


def _feedback_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    dt, K, ref = step
    grad = nat.FeedbackCotangent()
    grad.gain_bar = outs[0].data_ptr() if outs[0] is not None else None
    grad.ref_bar = outs[1].data_ptr()
    return ens._lib.crb_step_rk4_feedback_adjoint(ens.plan.h, ens._ptr(ckpt), ens._ptr(lamd), int(lamd.shape[0]), t0, float(dt),
                                                  n_steps, every, ens._ptr(K), ens._ptr(ref), C.byref(desc), ens._ref(rec_bar),
                                                  C.byref(grad), ens._ptr(work), ens._stream())


# step = (dt, gain [n, 2n], reference [B, 2n] or None) on the device; the pass needs the work buffer of one cotangent
_FEEDBACK = _AdjointFamily(
    who="step_feedback_adjoint", prepare=_feedback_prepare, ckpt_shape=lambda ens: tuple(ens.state.shape),
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_rk4_feedback_adjoint_work_bytes(ens.plan.h, every, n_cot),
    checkpoint=_feedback_checkpoint, outputs=_feedback_outputs, sweep=_feedback_sweep,
    unpack=lambda ens, outs, sd: tuple(outs))


def _implicit_feedback_prepare(ens, n_steps, args, held_force, impulse_amp, record):
    h, n_iter, hold, gain, reference, want_gain = args
    K = ens._feedback_gain(gain, "step_implicit_feedback_adjoint")
    ref = None if reference is None else ens._dev(reference, (ens.n_beams, 2 * ens.n))
    return (h, n_iter, hold, K, ref, ens._control_records(n_steps, hold)), held_force, None, (want_gain, impulse_amp is not None)


def _implicit_feedback_checkpoint(ens, x, ckpt, n_steps, every, t0, step, desc, sd, rec, t_end):
    h, n_iter, hold, K, ref, u_ckpt = step
    work = ens._work_buffer(_IMPLICIT_FEEDBACK, every, step, 1)
    return ens._lib.crb_step_implicit_feedback_checkpoint(ens.plan.h, ens._ptr(x), t0, float(h), n_steps, int(n_iter), int(hold),
                                                          every, ens._ptr(K), ens._ptr(ref), C.byref(desc), ens._ref(rec),
                                                          ens._ptr(ckpt), ens._ptr(u_ckpt), ens._ptr(work), C.byref(t_end),
                                                          ens._stream()), work


def _implicit_feedback_outputs(ens, D, want, sd):
    """[gain_bar [D, n, 2n] or None, ref_bar [D, B, 2n], amp_bar [D, B] or None, f_held_bar [D, B, n_node, 4]];
    ``want`` = (the gain gradient, the amplitude's)"""
    return _feedback_outputs(ens, D, want[0], sd) + _input_outputs(ens, D, want[1], sd)


def _implicit_feedback_sweep(ens, ckpt, lamd, n_steps, every, t0, step, desc, sd, rec_bar, outs, work):
    h, n_iter, hold, K, ref, u_ckpt = step
    grad = nat.FeedbackCotangent()
    grad.gain_bar = outs[0].data_ptr() if outs[0] is not None else None
    grad.ref_bar = outs[1].data_ptr()
    igrad, _ = _input_cotangent(ens, outs[2:], None)
    return ens._lib.crb_step_implicit_feedback_adjoint(ens.plan.h, ens._ptr(ckpt), ens._ptr(u_ckpt), ens._ptr(lamd),
                                                       int(lamd.shape[0]), t0, float(h), n_steps, int(n_iter), int(hold), every,
                                                       ens._ptr(K), ens._ptr(ref), C.byref(desc), ens._ref(rec_bar),
                                                       C.byref(grad), C.byref(igrad), ens._ptr(work), ens._stream())


# step = (h, n_iter, hold, gain [n, 2n], reference [B, 2n] or None, u_ckpt [K, B, n_node, 4]) on the device: the pass fills
# u_ckpt, the sweep's recompute reads it as its schedule; a segment's checkpoint is the implicit adjoint's
_IMPLICIT_FEEDBACK = _AdjointFamily(
    who="step_implicit_feedback_adjoint", prepare=_implicit_feedback_prepare, ckpt_shape=_IMPLICIT.ckpt_shape,
    work_bytes=lambda ens, every, step, n_cot: ens._lib.crb_implicit_feedback_adjoint_work_bytes(
        ens.plan.h, every, int(step[1]), int(step[2]), n_cot),
    checkpoint=_implicit_feedback_checkpoint, outputs=_implicit_feedback_outputs, sweep=_implicit_feedback_sweep,
    unpack=lambda ens, outs, sd: (outs[0], outs[1], outs[2], ens._unpack_force_dirs(outs[3])))


def _rollout_result(ctx, ens, opts, x, samples):
    """what a rollout's forward returns: x(T) reduced and the samples (without a record an empty placeholder that takes no
    gradient)"""
    if samples is None:
        samples = torch.zeros(0, dtype=ens.dtype, device=ens.device)
    if opts["record"] is None:
        ctx.mark_non_differentiable(samples)
    return ens.unpack_state(x), samples


def _rollout_seed(ens, o, g_x, g_samples):
    """the seeds of a rollout's backward from the output gradients (a missing g_x is zero): (lamd, rec_bar, cot)"""
    g_x = torch.zeros((ens.n_beams, 2 * ens.n), dtype=ens.dtype, device=ens.device) if g_x is None else g_x
    lamd = ens._pack_dirs(g_x.to(ens.dtype).reshape(1, ens.n_beams, 2 * ens.n).contiguous(), True)
    rec_bar, cot = ens._record_cotangent(o["record"], o["n_steps"], o["record_every"],
                                         g_samples if o["record"] is not None else None, 1)
    return lamd, rec_bar, cot


class _Rollout(torch.autograd.Function):
    """BeamEnsemble.rollout (``fam`` = _RK4) and rollout_implicit (_IMPLICIT): forward = the family's checkpoint pass,
    backward = its sweep on the saved checkpoints"""

    @staticmethod
    def forward(ctx, ens, fam, opts, x0, amp, held, ctrl):
        desc, keep = ens._input_desc(None if amp is None else amp.detach(), opts["duration"], opts["index"],
                                     None if held is None else held.detach())
        sd, packed = ens._sched_desc(None if ctrl is None else (ctrl.detach(), opts["hold"]))
        x = ens.pack_state(x0.detach())
        rec, samples = ens._record_desc(opts["record"], opts["n_steps"], opts["record_every"])
        ckpt = ens._checkpoint_pass(fam, x, opts["n_steps"], opts["t0"], opts["step"], desc, opts["every"], rec, sd)
        ens._keep += keep + [samples, packed]
        ctx.ens, ctx.fam, ctx.opts = ens, fam, opts
        ctx.has_amp, ctx.has_held, ctx.has_ctrl = amp is not None, held is not None, ctrl is not None
        ctx.save_for_backward(ckpt, None if amp is None else amp.detach(), None if held is None else held.detach(), packed)
        return _rollout_result(ctx, ens, opts, x, samples)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_samples):
        ens, o = ctx.ens, ctx.opts
        ckpt, amp, held, packed = ctx.saved_tensors
        desc, keep = ens._input_desc(amp, o["duration"], o["index"], held)
        sd = nat.InputSchedule(packed.data_ptr(), int(packed.shape[0]), int(o["hold"])) if ctx.has_ctrl else None
        lamd, rec_bar, cot = _rollout_seed(ens, o, g_x, g_samples)
        amp_bar, f_bar = ens._sweep(ctx.fam, ckpt, lamd, o["n_steps"], o["t0"], o["step"], desc, o["every"], rec_bar,
                                    ctx.has_amp, sd)
        ens._keep += keep + [cot, packed]
        gx0 = ens._unpack_dirs(lamd)[0] if ctx.needs_input_grad[3] else None
        gamp = amp_bar[0] if (ctx.has_amp and ctx.needs_input_grad[4]) else None
        gheld = ens._unpack_force_dirs(f_bar)[0] if (ctx.has_held and ctx.needs_input_grad[5]) else None
        gctrl = ens._unpack_sched_dirs(f_bar)[0] if (ctx.has_ctrl and ctx.needs_input_grad[6]) else None
        return None, None, None, gx0, gamp, gheld, gctrl


class _FeedbackRollout(torch.autograd.Function):
    """BeamEnsemble.rollout_feedback: forward = crb_step_rk4_feedback_checkpoint, backward = crb_step_rk4_feedback_adjoint on
    the saved checkpoints"""

    @staticmethod
    def forward(ctx, ens, opts, x0, gain, ref):
        K = ens._feedback_gain(gain, "rollout_feedback")
        r = None if ref is None else ens._dev(ref.detach(), (ens.n_beams, 2 * ens.n))
        desc, keep = ens._input_desc(opts["amp"], opts["duration"], opts["index"], opts["held"])
        x = ens.pack_state(x0.detach())
        rec, samples = ens._record_desc(opts["record"], opts["n_steps"], opts["record_every"])
        ckpt = ens._checkpoint_pass(_FEEDBACK, x, opts["n_steps"], opts["t0"], (opts["dt"], K, r), desc, opts["every"], rec)
        ens._keep += keep + [samples]
        ctx.ens, ctx.opts, ctx.has_ref = ens, opts, ref is not None
        ctx.save_for_backward(ckpt, K, r)
        return _rollout_result(ctx, ens, opts, x, samples)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_samples):
        ens, o = ctx.ens, ctx.opts
        ckpt, K, r = ctx.saved_tensors
        desc, keep = ens._input_desc(o["amp"], o["duration"], o["index"], o["held"])
        lamd, rec_bar, cot = _rollout_seed(ens, o, g_x, g_samples)
        gain_bar, ref_bar = ens._sweep(_FEEDBACK, ckpt, lamd, o["n_steps"], o["t0"], (o["dt"], K, r), desc, o["every"], rec_bar,
                                       ctx.needs_input_grad[3])
        ens._keep += keep + [cot]
        gx0 = ens._unpack_dirs(lamd)[0] if ctx.needs_input_grad[2] else None
        ggain = gain_bar[0] if ctx.needs_input_grad[3] else None
        gref = ref_bar[0] if (ctx.has_ref and ctx.needs_input_grad[4]) else None
        return None, None, gx0, ggain, gref


class _ImplicitFeedbackRollout(torch.autograd.Function):
    """BeamEnsemble.rollout_implicit_feedback: forward = crb_step_implicit_feedback_checkpoint, backward =
    crb_step_implicit_feedback_adjoint on the saved checkpoints and controls"""

    @staticmethod
    def forward(ctx, ens, opts, x0, gain, ref, amp, held):
        amp_d, held_d = (None if v is None else v.detach() for v in (amp, held))
        step, _, _, _ = _implicit_feedback_prepare(ens, opts["n_steps"], (opts["h"], opts["n_iter"], opts["hold"], gain,
                                                                          None if ref is None else ref.detach(), True),
                                                   held_d, amp_d, opts["record"])
        desc, keep = ens._input_desc(amp_d, opts["duration"], opts["index"], held_d)
        x = ens.pack_state(x0.detach())
        rec, samples = ens._record_desc(opts["record"], opts["n_steps"], opts["record_every"])
        ckpt = ens._checkpoint_pass(_IMPLICIT_FEEDBACK, x, opts["n_steps"], opts["t0"], step, desc, opts["every"], rec)
        ens._keep += keep + [samples]
        ctx.ens, ctx.opts = ens, opts
        ctx.has = tuple(v is not None for v in (ref, amp, held))
        ctx.save_for_backward(ckpt, step[3], step[4], step[5], amp_d, held_d)
        control = ens._unpack_controls(step[5], opts["n_steps"], opts["hold"])
        ctx.mark_non_differentiable(control)
        return _rollout_result(ctx, ens, opts, x, samples) + (control,)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_samples, g_control):
        ens, o = ctx.ens, ctx.opts
        ckpt, K, r, u_ckpt, amp, held = ctx.saved_tensors
        has_ref, has_amp, has_held = ctx.has
        desc, keep = ens._input_desc(amp, o["duration"], o["index"], held)
        lamd, rec_bar, cot = _rollout_seed(ens, o, g_x, g_samples)
        need = ctx.needs_input_grad
        gain_bar, ref_bar, amp_bar, f_bar = ens._sweep(_IMPLICIT_FEEDBACK, ckpt, lamd, o["n_steps"], o["t0"],
                                                       (o["h"], o["n_iter"], o["hold"], K, r, u_ckpt), desc, o["every"],
                                                       rec_bar, (need[3], has_amp))
        ens._keep += keep + [cot]
        gx0 = ens._unpack_dirs(lamd)[0] if need[2] else None
        ggain = gain_bar[0] if need[3] else None
        gref = ref_bar[0] if (has_ref and need[4]) else None
        gamp = amp_bar[0] if (has_amp and need[5]) else None
        gheld = ens._unpack_force_dirs(f_bar)[0] if (has_held and need[6]) else None
        return None, None, gx0, ggain, gref, gamp, gheld


class _Equilibrium(torch.autograd.Function):
    """BeamEnsemble.equilibrium: forward = crb_solve_static, backward = one crb_static_vjp at the solution"""

    @staticmethod
    def forward(ctx, ens, opts, held):
        sol = ens.solve_static(None if held is None else held.detach(), opts["q0"], opts["load_steps"], opts["max_iter"],
                               opts["rtol"], opts["atol"])
        ctx.ens, ctx.has_held = ens, held is not None
        ctx.save_for_backward(sol.q, sol.converged)
        ctx.mark_non_differentiable(sol.converged)
        return sol.q, sol.converged

    @staticmethod
    @once_differentiable
    def backward(ctx, g_q, g_conv):
        ens = ctx.ens
        q, converged = ctx.saved_tensors
        if not (ctx.has_held and ctx.needs_input_grad[2]):
            return None, None, None
        g_q = torch.zeros_like(q) if g_q is None else g_q
        fb, _, status, _ = ens._static_sens(g_q.to(ens.dtype).contiguous(), q, True, False, "equilibrium")
        ok = (converged & (status == 0)).view(-1, 1)
        return None, None, torch.where(ok, fb[0], torch.zeros_like(fb[0]))
