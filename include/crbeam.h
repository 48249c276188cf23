/*
 * crbeam.h -- C ABI of libcrbeam.so, the MI355X (gfx950) beam-dynamics stepper.
 *
 * The reference (cram9030/continuum-robot, pure Python) has no FFI/plugin interface: its
 * boundary for this path is the Python class API of
 * src/continuum_robot/models/dynamic_beam_model.py (DynamicEulerBernoulliBeam) and the
 * scipy.solve_ivp call sites that step its RHS.  This header is the native boundary a
 * maintainer binds with ctypes; every entry point names the reference
 * interface it stands in for.  Plain pointers and sizes only; no torch / C++ types.
 *
 * Conventions
 *   - every function returns 0 (CRB_OK) or a negative CRB_E* code; crb_last_error() returns
 *     a thread-local message for the last failure on the calling thread.
 *   - "device pointer" = HIP device memory of the plan's device and dtype; the caller owns
 *     all state/force tensors, the library owns only what hangs off the opaque plan.
 *   - launches are asynchronous on the passed stream (a hipStream_t passed as void*; NULL =
 *     the default stream).  A plan is not thread-safe; distinct plans are independent.
 *   - device state layout  x[B][2][n_node][4] : plane 0 = positions, plane 1 = velocities,
 *     record = {u, w, phi, 0}.  This is the reference's interleaved full DOF order
 *     (euler_bernoulli_beam.py:111-133) padded to 32-byte (fp64) / 16-byte (fp32) records;
 *     constrained DOFs keep their slot and hold 0.  Generalised-force tensors use
 *     f[B][n_node][4] the same way.  crb_pack_* / crb_unpack_* convert to and from the
 *     reference's REDUCED ordering (euler_bernoulli_beam.py:258-259, state = [q_red ; v_red],
 *     dynamic_beam_model.py:135-145).
 */
#ifndef CRBEAM_H
#define CRBEAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRB_VERSION 106

enum { CRB_OK = 0, CRB_EINVAL = -1, CRB_EHIP = -2, CRB_ENODEV = -3, CRB_EUNSUPPORTED = -4 };
enum { CRB_F64 = 0, CRB_F32 = 1 };
enum { CRB_BC_NONE = 0, CRB_BC_FIXED = 1, CRB_BC_PINNED = 2 }; /* abstractions.py:16-20 */
enum {
    CRB_FORCE_DRAG = 1u,      /* FluidDragForce auto-registration, dynamic_beam_model.py:223-231 */
    CRB_FORCE_GRAVITY = 2u,   /* GravityForce auto-registration,   dynamic_beam_model.py:234-241 */
    CRB_CORRECTED_AXIAL = 4u  /* opt-in f1 = -f2 instead of the shipped f1 (segments.py:178-208) */
};
enum { CRB_INPUT_NONE = 0, CRB_INPUT_IMPULSE = 1 };

typedef struct crb_plan crb_plan;

/* One beam topology shared by all beams of the ensemble: the CSV schema of
 * dynamic_beam_model.py:78-90 plus ForceParams (force_params.py:16-22).  Host pointers. */
typedef struct crb_beam_desc {
    int32_t n_elem;
    const double* length;          /* [n_elem] */
    const double* elastic_modulus; /* [n_elem] */
    const double* moment_inertia;  /* [n_elem] */
    const double* density;         /* [n_elem] */
    const double* cross_area;      /* [n_elem] */
    const uint8_t* nonlinear;      /* [n_elem] CSV 'type': 0 linear, 1 nonlinear */
    const uint8_t* node_bc;        /* [n_elem+1] CRB_BC_* per NODE (CSV row i -> node i, last node free) */
    const double* wetted_area;     /* [n_elem] or NULL when CRB_FORCE_DRAG is off */
    const double* drag_coef;       /* [n_elem] or NULL */
    double fluid_density;          /* ForceParams.fluid_density */
    double gravity[3];             /* ForceParams.gravity_vector (gz unused, gravity_forces.py:18) */
    uint32_t flags;                /* CRB_FORCE_* | CRB_CORRECTED_AXIAL */
} crb_beam_desc;

typedef struct crb_layout {
    int32_t dtype;        /* CRB_F64 / CRB_F32 */
    int32_t n_beams;
    int32_t n_elem;
    int32_t n_node;       /* n_elem + 1 */
    int32_t n_free;       /* size n of the reference's reduced position vector */
    int32_t node_offset;  /* 1 when node 0 is FIXED and therefore has no thread slot, else 0 */
    int32_t n_slots;      /* nodes carried by threads = n_node - node_offset */
    int32_t beams_per_group; /* beams handled by one workgroup */
    int32_t threads;      /* workgroup size */
    int32_t pcr_levels;   /* cyclic-reduction levels the mass solve applies */
    int32_t pcr_levels_full; /* ceil(log2(n_slots)): levels of the untruncated reduction */
    int32_t mixed_topology; /* 1: the beams' free-DOF sets differ (per-beam n_elem / boundary conditions): n_elem and
                             * n_free are the ensemble's maxima, reduced vectors are padded to n_free per beam
                             * (crb_plan_get_beam_info / crb_plan_get_beam_free_index give each beam's own) */
} crb_layout;

/* External generalised force u(t) added to the right-hand side, the `u` of
 * get_dynamic_system()(t, x, u) (dynamic_beam_model.py:343-362).
 *   held    : f_held[B][n_node][4] (device, may be NULL) is constant over the call.
 *   impulse : the examples' forcing (example_utilities.py:144-148, lqr_control.py:33-41):
 *             amp[b] on DOF (node, dof) while t < duration, else 0; evaluated at every RK4
 *             stage time. */
typedef struct crb_input_desc {
    int32_t kind;        /* CRB_INPUT_NONE / CRB_INPUT_IMPULSE */
    int32_t node;        /* impulse: node index (0..n_elem) */
    int32_t dof;         /* impulse: 0 = u, 1 = w, 2 = phi */
    int32_t reserved;
    double duration;     /* impulse: seconds */
    const void* amp;     /* impulse: device [B], plan dtype */
    const void* f_held;  /* device [B][n_node][4] or NULL */
    const int32_t* node_b; /* impulse: device [B] per-beam node (overrides `node`), or NULL -- beams of different length
                            * each forced at their own tip (`u[-2]` of example_utilities.py:147 per beam) */
} crb_input_desc;

/* Strided on-device recording of one DOF during crb_step_rk4_rec: the `t_eval` output of the
 * reference's solve_ivp calls (example_utilities.py:153-159) reduced to what the examples read
 * (tip displacement, lqr_control.py:168; example_utilities.py:173-205).  After every `every`-th step
 * out[b][k] = x[b][plane][node][dof], k = (step+1)/every - 1; out holds floor(n_steps/every)
 * values per beam (device, plan dtype). */
#define CRB_RECORD_ALL (-1) /* node = CRB_RECORD_ALL: whole-state snapshots (every DOF of sol.y on the t_eval grid,
                             * what examples/example_utilities.py:173-205 reads beam shapes from): out is device
                             * [floor(n_steps/every)][B][2][n_node][4], zero-initialised by the caller */
typedef struct crb_record_desc {
    int32_t plane;   /* 0 position, 1 velocity */
    int32_t node;
    int32_t dof;
    int32_t every;   /* >= 1 */
    void* out;       /* device [B][floor(n_steps/every)] */
} crb_record_desc;

int crb_version(void);
const char* crb_last_error(void);

/* Builds everything DynamicEulerBernoulliBeam.__init__ precomputes (dynamic_beam_model.py:25-74):
 * element coefficient packs (segments.py:32-78), the boundary-condition masks
 * (euler_bernoulli_beam.py:221-298), the mass matrix in node-block form and its cyclic-reduction
 * factorisation (replaces M_inv = inv(M), dynamic_beam_model.py:60), drag factors
 * (fluid_forces.py:50-101) and the gravity index table (gravity_forces.py:97-146).
 * device >= 0: HIP device ordinal, tables are uploaded.  device == -1: host-only plan for
 * inspection (crb_plan_get_* work, every launch returns CRB_ENODEV). */
int crb_plan_create(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* desc);
/* Heterogeneous ensembles (SURVEY f-3): descs[n_beams], one CSV-schema record + ForceParams per beam -- what the
 * reference's parallel examples run as independent simulations (examples/beam_comparison_fluid.py:49-83: six beams,
 * three without and three with fluid; beam_comparison_gravity.py:53-66).  Per beam: every element column and the
 * linear/nonlinear type; n_elem (the plan is laid out for the longest beam, a shorter one ends in padding nodes that
 * are fully constrained and carry no element); node_bc (dynamic_beam_model.py:205-218, euler_bernoulli_beam.py:221-298);
 * fluid_density, the gravity vector and the DRAG / GRAVITY flags (dynamic_beam_model.py:220-241).  Only
 * CRB_CORRECTED_AXIAL must be common.  Assembly and factorisation run batched on the device (one workgroup per beam).
 * When the beams' free-DOF sets differ (crb_layout.mixed_topology) the reduced vectors of crb_pack_* / crb_unpack_*
 * are [B][rows][n_free] with n_free the ensemble's maximum: beam b uses the first n_free_b entries of each row, the
 * rest is ignored on pack and zero on unpack; crb_feedback_force (one gain for the whole ensemble) is not available --
 * crb_feedback_force_grouped takes one gain per group of like beams.
 * The host inspectors (crb_plan_get_free_index/_mass/_stiffness/_pcr_tables/_slot_tables) describe beam 0. */
int crb_plan_create_ensemble(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* descs);
/* n_elem and n_free (size of the reference's reduced position vector) of one beam of the plan; either may be NULL */
int crb_plan_get_beam_info(const crb_plan* plan, int beam, int32_t* n_elem, int32_t* n_free);
/* reduced index -> full index 3*node+dof of one beam, [n_free of that beam] host */
int crb_plan_get_beam_free_index(const crb_plan* plan, int beam, int32_t* full_index);
void crb_plan_destroy(crb_plan* plan);
int crb_plan_get_layout(const crb_plan* plan, crb_layout* out);
/* reduced index -> full index 3*node+dof, ascending (euler_bernoulli_beam.py:258-259); [n_free] host */
int crb_plan_get_free_index(const crb_plan* plan, int32_t* full_index);
/* Host copies of the solve tables in fp64, for inspection/tests:
 *   levels [pcr_levels_full][n_slots][10], final_ [n_slots][6] (computed after `pcr_levels`
 *   levels), norms [pcr_levels_full].  Any pointer may be NULL. */
int crb_plan_get_pcr_tables(const crb_plan* plan, double* levels, double* final_, double* norms);
/* Host copies of the per-slot constants the kernels keep in registers, for inspection/tests:
 *   drag [n_slots], half_mass [n_slots], mask [n_slots][3],
 *   grav [n_slots][12] = {phiA, phiB, segA[3], segB[3], comp[3], 0} (see crb_generic.h GravTab),
 *   elem_kind [n_slots] (0 none, 1 linear, 2 nonlinear; the element LEFT of the slot's node).
 * Any pointer may be NULL. */
int crb_plan_get_slot_tables(const crb_plan* plan, double* drag, double* half_mass, double* mask, int16_t* grav,
                             int32_t* elem_kind);
/* Host restatement of the register-blocked stepper's mass solve, for tests: blocks = the 256 node rows of a mass matrix as
 * [a_ax, b_ax, c_ax, A[4], B[4], C[4]] (axial left / diagonal / right, then the (w, phi) 2x2 blocks row-major), Lc the
 * length that scales rotations in the level norms.  x = M^-1 r for r, x of [256][3]; *levels = the separator cyclic-reduction
 * levels kept, norms[6] = each separator level's largest multiplier (either may be NULL).  CRB_EUNSUPPORTED when the lane
 * interiors (4 nodes per lane) are not bitwise uniform. */
int crb_blocked_solve_host(const double* blocks, double Lc, const double* r, double* x, int32_t* levels, double* norms);
/* The same with every lane's interior solved about its centre node, the form the blocked stepper runs (crb_blocked.h:
 * blk_twist_interior_solve).  CRB_EUNSUPPORTED also when the lanes are uniform but an interior lacks the mirror structure of
 * equal elements (diagonal B, C = J A J with J = diag(1, -1) on (w, phi)); the message then names the mirror structure. */
int crb_blocked_twist_solve_host(const double* blocks, double Lc, const double* r, double* x, int32_t* levels, double* norms);
/* Which tables of the register-blocked stepper the plan holds: *form = 0 none (the plan never runs it), 1 the block-Thomas
 * interior solve, 2 the interior solve twisted about each lane's centre node (nonlinear plans whose node blocks have the mirror
 * structure of equal elements bitwise); *levels = its separator levels (0 for form 0).  Either may be NULL.  The plan's
 * fixed-step RK4 calls without gravity and held input run that form unless CRB_DISABLE_BLOCKED is set. */
int crb_plan_get_blocked_form(const crb_plan* plan, int32_t* form, int32_t* levels);
/* Dense reduced mass matrix as assembled by the plan, [n_free][n_free] host fp64
 * (EulerBernoulliBeam.get_mass_matrix, euler_bernoulli_beam.py:358-362). */
int crb_plan_get_mass(const crb_plan* plan, double* M);
/* Dense reduced stiffness matrix of an all-linear beam, [n_free][n_free] host fp64
 * (EulerBernoulliBeam.get_stiffness_matrix, euler_bernoulli_beam.py:422-511); CRB_EINVAL with the
 * reference's message when a segment is nonlinear. */
int crb_plan_get_stiffness(const crb_plan* plan, double* K);

/* reduced [B][2n] <-> device layout [B][2][n_node][4]  (stiffness_with_boundary's
 * scatter/gather, euler_bernoulli_beam.py:280-289, done once at the API edge) */
int crb_pack_state(const crb_plan* plan, const void* x_red, void* x, void* stream);
int crb_unpack_state(const crb_plan* plan, const void* x, void* x_red, void* stream);
/* reduced [B][n] <-> device layout [B][n_node][4] for force / position-like vectors */
int crb_pack_vec(const crb_plan* plan, const void* v_red, void* v, void* stream);
int crb_unpack_vec(const crb_plan* plan, const void* v, void* v_red, void* stream);

/* k(q): EulerBernoulliBeam.get_stiffness_function() (euler_bernoulli_beam.py:163-219, 270-289).
 * x: device state (only the position plane is read); k: device [B][n_node][4]. */
int crb_internal_force(const crb_plan* plan, const void* x, void* k, void* stream);

/* xdot = [v ; Minv(-k(q) + f_drag + f_gravity + u)]: get_dynamic_system()(t, x, u)
 * (dynamic_beam_model.py:256-272, 294-328, 343-362).  u: device [B][n_node][4] or NULL. */
int crb_rhs(const crb_plan* plan, const void* x, const void* u, void* xdot, void* stream);

/* The same two functions for HOST vectors in the reference's reduced ordering, synchronously: what the single-beam
 * closures handed to scipy.solve_ivp call (get_dynamic_system()(t, x, u), dynamic_beam_model.py:343-362;
 * get_stiffness_function(), euler_bernoulli_beam.py:364-368) -- 6e5 calls per simulated second under LSODA.  The
 * (un)packing is fused into the kernel's own loads and stores, the vectors travel through pinned, device-mapped
 * staging of the plan: ONE launch + one stream synchronisation per call (the device-pointer forms above need
 * pack + kernel + unpack + copies).  x_red / xdot_red: [n_beams][2 n_free], u_red: [n_beams][n_free] or NULL,
 * q_red / k_red: [n_beams][n_free].  fp64 plans with one free-DOF set; not thread-safe per plan. */
int crb_rhs_host(const crb_plan* plan, const double* x_red, const double* u_red, double* xdot_red);
int crb_internal_force_host(const crb_plan* plan, const double* q_red, double* k_red);

/* Tangent stiffness dk/dq of every beam at its positions: the derivative of
 * EulerBernoulliBeam.create_stiffness_function() (euler_bernoulli_beam.py:163-219) -- what get_stiffness_matrix()
 * (euler_bernoulli_beam.py:422-511) returns for all-linear beams, for nonlinear beams at any q.
 * dk/dq at positions x (plane 0 of x[B][2][n_node][4]); out: device [B][n_node][3][3][3] plan dtype,
 * block 0/1/2 = coupling to the left node / own / right node, rows and cols [u, w, phi].  Constrained DOFs have
 * identity rows and zero columns.  Beams of up to 256 thread-carried nodes, fp64 and fp32 plans. */
int crb_tangent_stiffness(const crb_plan* plan, const void* x, void* out, void* stream);
/* Static equilibrium: the q at which DynamicEulerBernoulliBeam.get_dynamic_system() (dynamic_beam_model.py:294-328)
 * returns zero acceleration at v = 0, i.e. k(q) = g(q) + u (drag vanishes at rest).  Newton on the block-tridiagonal
 * tangent with load continuation from the initial guess (load_steps <= 4096 increments, each halved up to 6 times when it
 * does not converge within max_iter <= 1000 steps, never below 1/64 of its nominal size), converged when |k - g - u|inf <= rtol max(|k|inf, |g + u|inf) + atol per beam.
 * Equilibrium k(q) = g(q) + u of every beam; x: in = initial guess (plane 0), out = solution, plane 1 zeroed.
 * input: kind CRB_INPUT_NONE, f_held = u or NULL.  iters: device int32 [B], >= 0 Newton iterations used,
 * -1 not converged, -2 non-finite.  residual: device [B] plan dtype, final scaled residual (may be NULL).
 * fp64 plans only (CRB_EUNSUPPORTED otherwise); every beam needs a FIXED or PINNED node; up to 256 thread-carried nodes. */
int crb_solve_static(const crb_plan* plan, void* x, const crb_input_desc* input, int load_steps, int max_iter,
                     double rtol, double atol, int32_t* iters, void* residual, void* stream);

/* Tangents of the inputs of crb_step_rk4_tangent, per direction (device, fp64; layouts of crb_input_desc with a leading
 * direction index). */
typedef struct crb_input_tangent {
    const void* d_amp;    /* device [n_dir][B]: derivative of the impulse amplitude per direction, or NULL (= 0) */
    const void* df_held;  /* device [n_dir][B][n_node][4]: derivative of the held force, or NULL (= 0) */
} crb_input_tangent;

/* Forward-mode derivative (Jacobian-vector products) of the RHS: the derivative of get_dynamic_system()(t, x, u)
 * (dynamic_beam_model.py:294-362) along n_dir directions per beam, exact (dual numbers through the element forces, drag
 * and gravity, the same cyclic-reduction mass solve as crb_rhs; no finite differences).
 * xdot = f(x, u) and dxdot[d] = df/dx·dx[d] + df/du·du[d], for d < n_dir.
 * x: [B][2][n_node][4]; u: [B][n_node][4] or NULL; dx, dxdot: [n_dir][B][2][n_node][4];
 * du: [n_dir][B][n_node][4] or NULL; xdot: may be NULL.  Outputs must not alias inputs.
 * fp64 plans only (CRB_EUNSUPPORTED), beams of up to 256 thread-carried nodes, 1 <= n_dir <= 65535. */
int crb_rhs_jvp(const crb_plan* plan, const void* x, const void* u, const void* dx, const void* du, int n_dir,
                void* xdot, void* dxdot, void* stream);

/* crb_step_rk4 (same clock, same input), with the tangent dx [n_dir][B][2][n_node][4] of the rollout propagated
 * in place: dx(T) = ∂x(T)/∂x(0)·dx(0) + ∂x(T)/∂amp·d_amp + ∂x(T)/∂f_held·df_held.
 * The derivative of the discrete RK4 map crb_step_rk4 applies (the scipy.solve_ivp call sites it replaces,
 * example_utilities.py:153-159, lqr_control.py:117-125), in ONE launch: an identity batch of seeds (n_dir = 2 n_free)
 * gives the state-transition matrix.  x advances exactly as under crb_step_rk4; *t_end as there.  dinput may be NULL;
 * d_amp needs an impulse input.  fp64 plans only, beams of up to 256 thread-carried nodes, 1 <= n_dir <= 65535. */
int crb_step_rk4_tangent(const crb_plan* plan, void* x, void* dx, int n_dir, double t0, double dt, int n_steps,
                         const crb_input_desc* input, const crb_input_tangent* dinput, double* t_end, void* stream);

/* Reverse-mode derivative (vector-Jacobian products) of the RHS: the transpose of crb_rhs_jvp's derivative of
 * get_dynamic_system()(t, x, u) (dynamic_beam_model.py:294-362), exact (the element Jacobian on dual numbers, drag, gravity
 * through inverse lists of the plan's index table, and the exact transpose of the plan's truncated cyclic-reduction solve).
 * For n_cot cotangents lam[c] of xdot:  xbar[c] = (df/dx)^T lam[c],  ubar[c] = (df/du)^T lam[c];  xdot = f(x, u) when not NULL.
 * x: [B][2][n_node][4]; u: [B][n_node][4] or NULL; lam, xbar: [n_cot][B][2][n_node][4]; ubar: [n_cot][B][n_node][4] or NULL.
 * Constrained DOFs (and node 0 of plans without its slot) are zero in xbar and ubar.  Outputs must not alias inputs or each
 * other.  fp64 plans only (CRB_EUNSUPPORTED), beams of up to 256 thread-carried nodes, 1 <= n_cot <= 65535. */
int crb_rhs_vjp(const crb_plan* plan, const void* x, const void* u, const void* lam, int n_cot, void* xdot, void* xbar,
                void* ubar, void* stream);

/* Cotangents of the inputs of a rollout, ACCUMULATED by crb_step_rk4_adjoint (device, fp64; NULL = not wanted). */
typedef struct crb_input_cotangent {
    void* amp_bar;     /* device [n_cot][B]: dL/d amp of the impulse (needs an impulse input) */
    void* f_held_bar;  /* device [n_cot][B][n_node][4]: dL/d f_held */
} crb_input_cotangent;

/* Device bytes of the work buffer of crb_step_rk4_adjoint for checkpoints every `every` steps:
 * every * (4 * B * 2 * n_node * 4 + 1) * sizeof(double) -- the four RK4 stage points of each step of one segment, then the
 * steps' clocks.  0 for every < 1. */
size_t crb_rk4_adjoint_work_bytes(const crb_plan* plan, int every);

/* The forward pass of a differentiable rollout: crb_step_rk4 (same clock, same input; x advances in place, *t_end as there) in
 * the adjoint's own arithmetic, writing the state at the start of steps 0, every, 2 every, ... to
 * ckpt [ceil(n_steps / every)][B][2][n_node][4] (device).  rec: as crb_step_rk4_rec (may be NULL), so that a loss over the
 * recorded trajectory (the t_eval samples of example_utilities.py:153-159, 173-205) can be differentiated.  x agrees with
 * crb_step_rk4 to rounding, not bitwise.  fp64 plans only, beams of up to 256 thread-carried nodes. */
int crb_step_rk4_checkpoint(const crb_plan* plan, void* x, double t0, double dt, int n_steps, int every,
                            const crb_input_desc* input, const crb_record_desc* rec, void* ckpt, double* t_end, void* stream);

/* Adjoint (reverse-mode) of the RK4 rollout crb_step_rk4_checkpoint ran from t0 (the same dt, n_steps, every and input):
 * the gradient of a scalar loss L(x(T), samples) with respect to x(0) and the inputs in ONE backward sweep, for n_cot
 * cotangents per beam -- what central differences of the scipy.solve_ivp call sites (example_utilities.py:153-159,
 * lqr_control.py:117-125) or one crb_step_rk4_tangent direction per input would otherwise give.
 *   lam      device [n_cot][B][2][n_node][4], in place: dL/dx(T) on entry, dL/dx(0) on exit
 *   rec_bar  the record of the forward pass with out = its cotangent dL/d samples: [n_cot][B][n_rec] for one DOF,
 *            [n_cot][n_rec][B][2][n_node][4] for CRB_RECORD_ALL; NULL when the loss reads no samples
 *   grad     amp_bar / f_held_bar += dL/d amp, dL/d f_held (may be NULL)
 *   work     crb_rk4_adjoint_work_bytes(plan, every) device bytes
 * Per segment of `every` steps, last to first: one launch recomputes its RK4 stage points from the checkpoint, one sweeps it
 * back for all cotangents.  The result is the exact transpose of the discrete map (the derivative crb_step_rk4_tangent
 * propagates forward), bitwise independent of `every`, and D cotangents in one call are bitwise D calls of one.  lam must
 * not alias any other buffer; the outputs and work must not alias each other or ckpt.  fp64 plans only
 * (CRB_EUNSUPPORTED), beams of up to 256 thread-carried nodes, 1 <= n_cot <= 65535; host-only plans CRB_ENODEV. */
int crb_step_rk4_adjoint(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double dt, int n_steps,
                         int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                         const crb_input_cotangent* grad, void* work, void* stream);

/* Cotangents of the rod's own parameters, ACCUMULATED by crb_step_rk4_adjoint_params (device, fp64). */
typedef struct crb_param_cotangent {
    void* param_bar;   /* device [n_cot][B][n_node][8]; the record of node i: sA, sI of the element left of node i, sD of
                          node i, gx, gy of the segment of that node's slot, 0, 0, 0 (see crb_step_rk4_adjoint_params) */
} crb_param_cotangent;

/* Device bytes of the work buffer of crb_step_rk4_adjoint_params: crb_rk4_adjoint_work_bytes(plan, every) +
 * every * 4 * n_cot * B * n_node * 4 * sizeof(double) -- after the stage points and the clocks, the rbar = M^-T lambda_v of
 * every stage of one segment, per cotangent.  0 for every < 1 or n_cot < 1. */
size_t crb_rk4_adjoint_params_work_bytes(const crb_plan* plan, int every, int n_cot);

/* crb_step_rk4_adjoint (the same arguments, the same segments; lam, amp_bar and f_held_bar come out bitwise as there) that
 * also gives the gradient of the loss with respect to the rod -- what fitting a rod to a recorded trajectory needs, and what
 * central differences of the scipy.solve_ivp call sites (example_utilities.py:153-159) over rebuilt models
 * (euler_bernoulli_beam.py:26-109, fluid_forces.py:59-90, gravity_forces.py:104-146) would otherwise give, two rollouts per
 * parameter.  The right-hand side is linear in every parameter that stays out of the mass matrix, so per stage, with
 * rbar = M^-T lambda_v:
 *   sA, sI   -<(rbar_{i-1}, rbar_i), element force with only its EA / only its EI part>: dL/d of RELATIVE scales of EA and EI
 *            of the element left of node i, at scale 1 (dL/dE = (sA + sI) / E, dL/dI = sI / I)
 *   sD       rbar_w times the node's drag force: dL/d of a relative scale of the node's factor 0.5 rho_f Cd A_wet
 *   gx, gy   dL/d of the gravity vector through the segment of the node's slot; the caller sums them over the nodes of a beam
 * pgrad->param_bar is ACCUMULATED; constrained DOFs contribute nothing; padding nodes, and node 0 of plans without its slot,
 * hold zeros.  Per segment: the sweep that also stores rbar, then one reduction launch; every sum has a fixed order (no
 * atomics), so the result is bitwise independent of `every`, and D cotangents in one call are bitwise D calls of one.
 *   work     crb_rk4_adjoint_params_work_bytes(plan, every, n_cot) device bytes
 * Not differentiated: length, cross-section area and density (they enter the mass matrix).  CRB_EINVAL for a NULL pgrad,
 * param_bar or work, or a bad n_cot or every; otherwise the checks, limits and codes of crb_step_rk4_adjoint. */
int crb_step_rk4_adjoint_params(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double dt, int n_steps,
                                int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                                const crb_input_cotangent* grad, const crb_param_cotangent* pgrad, void* work, void* stream);

/* Sensitivities of the static equilibrium of crb_solve_static.  With R(q; u, theta) = k(q) - g(q) - u = 0 and the exact
 * tangent J = dk/dq - dg/dq at the positions of plane 0 of x [B][2][n_node][4], the implicit function theorem gives both
 * directions -- what central differences over crb_solve_static would otherwise give, one Newton solve per parameter and no
 * better than the equilibrium's residual floor.  J does not depend on the held force, so neither call takes an input.
 *   du, dq, q_bar, f_held_bar   device [n][B][n_node][4], fp64; component 3, constrained DOFs, padding nodes and node 0 of
 *                               plans without its slot come out zero
 *   status                      device int32 [B] or NULL: 0, or -2 where a component of a direction is not finite (a singular
 *                               tangent: the equilibrium is a limit point; or a non-finite q).  Other beams are unaffected.
 * One launch solves 4 right-hand sides per workgroup (1 for n < 4) by the block cyclic reduction of crb_solve_static;
 * n directions in one call are bitwise n calls of one.  Outputs must not alias inputs or each other.
 * CRB_EINVAL: NULL plan or pointers, n outside 1 .. 65535, aliasing.  CRB_EUNSUPPORTED: fp32 plans; more than 256
 * thread-carried nodes; plans with gravity whose index table couples a node to a rotation more than one slot away (a PINNED
 * root under gravity: such terms lie outside the block-tridiagonal tangent -- crb_solve_static only iterates with it, a
 * sensitivity would be wrong).  Then host-only plans: CRB_ENODEV. */
/* dq = J^-1 du at the positions of plane 0 of x: the sensitivity of the static equilibrium to the held force. */
int crb_static_jvp(const crb_plan* plan, const void* x, const void* du, int n_dir, void* dq, int32_t* status, void* stream);
/* mu = J^-T q_bar (= dL/d held force) into f_held_bar; param_bar: NULL, or device [n_cot][B][n_node][8] crb_param_cotangent
 * records (sA, sI, 0, gx, gy, 0, 0, 0) WRITTEN (not accumulated) from mu and q by the formulas of crb_step_rk4_adjoint_params
 * with rbar := mu at the one point q and no drag (v = 0). */
int crb_static_vjp(const crb_plan* plan, const void* x, const void* q_bar, int n_cot, void* f_held_bar, void* param_bar,
                   int32_t* status, void* stream);

/* Inverse lists of the gravity index table of beam `beam` (crb_plan_get_slot_tables' grav, reversed), host-only plans too:
 *   seg [n_slots][2][2]: per segment and force component (0 axial / 1 transverse), slot*4+dof of the node DOFs it adds to
 *   phi [n_slots][3][2]: per DOF of a slot, (segment << 1) | half of the segments whose rotation reads it (half: the segment
 *                        averages two rotations, weight 0.5)
 *   -1 = no entry; fanin[2] = the largest fan-in of each list kind.  Any pointer may be NULL.  CRB_EUNSUPPORTED when a
 *   fan-in exceeds the lists (the adjoint kernels refuse such plans). */
int crb_plan_get_grav_transpose(const crb_plan* plan, int beam, int32_t* seg, int32_t* phi, int32_t* fanin);

/* n_steps classical RK4 steps of size dt, in place, in ONE launch (replaces the
 * scipy.solve_ivp call sites example_utilities.py:153-159, lqr_control.py:117-125).  The clock
 * starts at t0 and accumulates by addition (t <- t + dt); stage times t, t+dt/2, t+dt.
 * *t_end (host, may be NULL) receives the final clock value, to be passed as the next t0. */
int crb_step_rk4(const crb_plan* plan, void* x, double t0, double dt, int n_steps, const crb_input_desc* input,
                 double* t_end, void* stream);

/* Adaptive integration t0 -> t_end of every beam with embedded Dormand-Prince 5(4) and per-beam step-size
 * control, one launch: the algorithm of scipy.integrate.solve_ivp(method="RK45"), which the reference's
 * tests hand their RHS to (tests/test_dynamic_beam.py:218-220, test_functional_composition.py:539-546).
 *   h    device [B] fp64: in  first step per beam (<= 0: scipy's select_initial_step), out next step
 *   stats device [B][4] int32: accepted steps, rejected steps, RHS evaluations, status (0 ok / 1 step
 *        too small or max_steps exceeded).  h and stats may be NULL.  One beam per workgroup (small beams are
 *        not packed here: every beam has its own step sequence); beams of up to 256 slots (LDS-resident stages). */
int crb_solve_rk45(const crb_plan* plan, void* x, double t0, double t_end, double rtol, double atol,
                   const crb_input_desc* input, void* h, void* stats, int max_steps, void* stream);

/* crb_solve_rk45 plus solve_ivp's `t_eval` for one DOF: values on the uniform grid
 * t_eval[k] = eval_t0 + k*eval_dt (k < n_eval, eval_t0 >= t0) by scipy's dense output (RkDenseOutput, the
 * 4th-order interpolant of RK45) -- what the examples read from `sol.y` (example_utilities.py:153-159,
 * 173-205).  rec->every is unused here; rec->out is device [B][n_eval], plan dtype; with rec->node =
 * CRB_RECORD_ALL it is [n_eval][B][2][n_node][4] (zero-initialised by the caller): every DOF of sol.y. */
int crb_solve_rk45_eval(const crb_plan* plan, void* x, double t0, double t_end, double rtol, double atol,
                        const crb_input_desc* input, void* h, void* stats, int max_steps,
                        const crb_record_desc* rec, double eval_t0, double eval_dt, int n_eval, void* stream);

/* Implicit fixed-step integration for the stiff end of the reference's call sites: the examples hand the beam RHS to
 * solve_ivp(method="LSODA") for 1 s (examples/example_utilities.py:153-159, examples/lqr_control.py:117-125) because
 * explicit steppers are stability-limited to dt <= ~7e-5 s.  n_steps steps of size h of the implicit midpoint rule
 * (for linear systems the trapezoidal rule / Newmark average acceleration: A-stable, second order, no numerical
 * damping) on M a = -k(q) + f_drag(v) + f_gravity(q) + u(t), each step solved by n_iter modified-Newton iterations
 * with the constant matrix A = M + (h^2/4) K0 (K0 = element tangent stiffness at q = 0; cyclic reduction with
 * multipliers factorised on the device whenever h changes); one launch, in place.
 *   n_iter 1 is exact for linear elements without drag / gravity; 2 reproduces the converged step otherwise (the
 *          state dependence of drag, gravity and the geometric stiffness is not stiff); every step starts from the
 *          previous step's iterate, the first step of a call from 0.
 *   input  sampled at the step MIDPOINT (impulse: on while t + h/2 < duration), held force as in crb_step_rk4.
 *   rec    as crb_step_rk4_rec (may be NULL).  Beams of up to 256 thread-carried nodes; fp64 plans only
 *          (cond(A) = 1e6 ... 1e9 at these step sizes).
 * Modes with |lambda| h >> 1 are not resolved (their amplitude is kept, their phase is not): displacements converge
 * at second order in h from h ~ 1e-3 s down, velocities only once h resolves the modes they contain. */
int crb_step_implicit(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter,
                      const crb_input_desc* input, const crb_record_desc* rec, double* t_end, void* stream);
/* The numerically DAMPED member of the same family: generalised-alpha (Chung & Hulbert) with spectral radius rho_inf in
 * [0, 1] at infinite frequency -- second order, unconditionally stable, modes with |lambda| h >> 1 lose the factor rho_inf
 * per step instead of ringing on with the wrong phase (rho_inf = 1: crb_step_implicit exactly; 0: they are gone after one
 * step).  What LSODA's BDF formulas do to the unresolved modes of the examples' runs (example_utilities.py:153-159) and the
 * midpoint rule does not.  Same iteration (matrix M + kappa K0, kappa = (1 - alpha_f) beta h^2 / (1 - alpha_m)); the
 * acceleration history starts from the RHS at t0 (one extra launch per call), the input is sampled at
 * t + (1 - alpha_f) h.  Runs the general kernel (one wave per SIMD) for every beam shape. */
int crb_step_implicit_damped(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter, double rho_inf,
                             const crb_input_desc* input, const crb_record_desc* rec, double* t_end, void* stream);

/* The examples' integration call with its TOLERANCES, one launch for the whole span and the whole ensemble:
 * solve_ivp(f, t_span, x0, method="LSODA", t_eval=np.arange(t0, t1, DT)) at scipy's default rtol 1e-3 / atol 1e-6
 * (examples/example_utilities.py:153-159) and the closed loop of examples/lqr_control.py:117-125 at rtol 1e-8 / atol 1e-10.
 * The step size is controlled INSIDE the kernel, per beam (one workgroup per beam; csrc/crb_ctrl.h):
 *   gain == NULL  the implicit midpoint rule of crb_step_implicit (order 2);
 *   gain != NULL  RK4 with u = K (ref - x) in every stage (order 4; device [n][2n] / [B][2n] like crb_step_rk4_feedback;
 *                 one free-DOF set, no held force).  The gain is held in LDS while it fits there (beams of up to ~30
 *                 elements); larger gains are streamed: every call first writes a transposed copy [2n][n] that the plan owns
 *                 (never cached: callers overwrite gains in place), and the node threads read their rows of it from global
 *                 memory in every stage, with the multiply-adds in the LDS form's order.  Environment CRB_CTRL_STREAM_GAIN=1 forces the
 *                 streamed form for every gain (tests).
 * by step doubling per piece -- a t_eval interval [t0 + k dt_eval, t0 + (k+1) dt_eval], cut at input->duration when the
 * impulse ends inside it (the impulse is then simply on or off within a piece): m = 2^r and 2m steps from the same state,
 * (fine - coarse) / (2^order - 1) measured in scipy's norm (RMS over the beam's reduced state -- its position half with
 * positions_only -- of err / (atol + rtol max(|fine|, |start|))); above 1 or not finite: twice the steps; the fine
 * solution is the accepted one; far below 1: half the rate for the next piece.  The cyclic-reduction tables of
 * A = M + (h^2/4) K0 for the whole ladder h = len / 2^r, r < max_rungs, are factorised on the device before the launch (and
 * kept with the plan).
 *   y_out  device [n_intervals][B][2][n_node][4] (the state at t0 + (k+1) dt_eval in slot k) or NULL
 *   stats  device int32 [B][4]: fine steps accepted, doublings, status (0 = reached the end, 2 = a piece asked for more than
 *          2^(max_rungs-1) steps: the beam stops at the start of that piece), rung of the last piece
 *   used   device int32 [B][n_intervals] fine steps accepted per interval, or NULL
 * x ends at t0 + n_intervals dt_eval.  fp64 plans, beams of up to 256 thread-carried nodes. */
typedef struct crb_control_desc {
    double rtol, atol;
    double first_rate;       /* steps per second of the first coarse solution; <= 0: 1e4 (implicit) / 2e5 (closed-loop RK4) */
    int32_t positions_only;  /* measure the position half of the state only */
    int32_t n_iter;          /* implicit scheme: modified-Newton iterations per step; <= 0: 1 (enough at the controller's step sizes) */
    int32_t max_rungs;       /* <= 0: 15 */
    int32_t per_wave;        /* 0: every beam its own step sequence (one workgroup per beam).  1 (implicit scheme, beams of 2 .. 32
                              * thread-carried nodes): G = 64 / n_slots beams share a wave AND its step sequence -- the worst of them
                              * decides -- so thousands of short beams fill the chip with a fifth of the waves */
    /* one DOF on the t_eval grid instead of (or next to) whole-state snapshots -- what the examples read (tip displacement,
     * lqr_control.py:168): series_out != NULL: device [B][n_intervals], plan dtype, series_out[b][k] = x[b][plane][node][dof] at
     * t0 + (k + 1) dt_eval (4096 beams x 1000 outputs: 33 MB instead of the 2.9 GB of y_out) */
    int32_t series_plane, series_node, series_dof, series_pad;
    void* series_out;
} crb_control_desc;
int crb_solve_controlled(const crb_plan* plan, void* x, double t0, double dt_eval, int n_intervals,
                         const crb_control_desc* control, const crb_input_desc* input, const void* gain, const void* ref,
                         void* y_out, void* stats, void* used, void* stream);

/* Per-beam status of the fixed-step steppers (crb_step_rk4[_rec], crb_step_implicit, crb_step_rk4_feedback, crb_rk4_stage at
 * stage 3).  status: device int32 [B], zeroed by the caller, or NULL to switch the reporting off; steps_done: the number of
 * steps the ensemble has taken so far.  A launch that leaves a non-finite value in beam b's state writes status[b] = the
 * ensemble's step count at the END of that launch (once: later launches leave a marked beam alone), so 0 = finite and k > 0 =
 * "went non-finite within the launch that ended at step k".  The reference has no such report: the shipped nonlinear element
 * (segments.py:178-208) is linearly unstable for long chains and solve_ivp simply returns NaN rows; this turns that into a
 * condition the planning layer can read per rollout.  The beams are independent: a diverged beam never affects another. */
int crb_plan_set_status(const crb_plan* plan, void* status, long long steps_done);
/* The step count the status reporting stands at (steps_done of crb_plan_set_status plus the steps of every launch since), so
 * that a caller can switch the reporting off around launches on a copy of the state and restore it exactly
 * (BeamEnsemble.linearize_implicit); -1 for a NULL plan. */
long long crb_plan_status_steps(const crb_plan* plan);

/* Feedback force of a whole ensemble, u = K (r - x) (FullStateLinear.compute_input,
 * control/full_state_linear.py:81; loop of examples/lqr_control.py:95-111), as one MFMA GEMM in the plan's dtype
 * (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32) with the gather from the state layout and the scatter into
 * the force layout fused in.
 *   xs   device [B][2][n_node][4]           gain  device [n][2n] row-major, reduced ordering
 *   ref  device [B][2n] reduced or NULL=0   u     device [B][n_node][4]: free-DOF entries are
 *                                                  overwritten, the rest must already be zero */
int crb_feedback_force(const crb_plan* plan, const void* xs, const void* gain, const void* ref, void* u, void* stream);

/* The same for heterogeneous ensembles (crb_plan_create_ensemble; SURVEY f-3): one gain per GROUP of beams, as the reference
 * designs one gain per model (examples/lqr_control.py:46-84, control/linear_quadratic_regulator.py:84-191).
 *   beam_group  host int32 [B]: the group of every beam, or -1 (no feedback: its u stays 0)
 *   gains       host array of n_groups device pointers, gains[g] = [n_g][2 n_g] row-major in the reduced ordering of group g's
 *               beams, which must share one free-DOF set (n_g = their n_free)
 *   ref         device [B][2 n_free] padded reduced states as crb_pack_state takes them, or NULL
 * One MFMA launch per group (rows gathered through the group's beam list); u must be zero where no group writes. */
int crb_feedback_force_grouped(const crb_plan* plan, const void* xs, int n_groups, const int32_t* beam_group,
                               const void* const* gains, const void* ref, void* u, void* stream);
/* crb_step_rk4_feedback with per-group gains: the stage-split loop (grouped force, then crb_rk4_stage, per stage). */
int crb_step_rk4_feedback_grouped(const crb_plan* plan, void* x, double t0, double dt, int n_steps, int n_groups,
                                  const int32_t* beam_group, const void* const* gains, const void* ref,
                                  const crb_input_desc* input, void* work, double* t_end, void* stream);

/* ONE stage of the stage-split RK4 stepper, for inputs that change from stage to stage -- state
 * feedback u = K(r - x) evaluated inside the RHS as examples/lqr_control.py:95-111 does
 * (FullStateLinear.compute_input, control/full_state_linear.py:81).  The caller computes this
 * stage's generalised force u_stage[B][n_node][4] from xs (e.g. one GEMM over the whole ensemble) and
 * calls:   k = f(t_stage, xs, u_stage + impulse);  acc = (stage ? acc : 0) + w_stage * k;
 *          stage < 3: xs_next = x + c_stage * k;      stage == 3: x += dt/6 * acc.
 * Stage 0 passes xs == x.  x, xs, acc, xs_next: device [B][2][n_node][4]; xs_next may not alias xs.
 * All state / force buffers of this header must be aligned to 32 bytes (a node record is read as one
 * vector); hipMalloc and torch allocations are. */
int crb_rk4_stage(const crb_plan* plan, void* x, const void* xs, void* acc, void* xs_next, const void* u_stage,
                  int stage, double t_stage, double dt, const crb_input_desc* input, void* stream);

/* The closed loop of examples/lqr_control.py:95-125 as ONE call: n_steps RK4 steps with u = K (r - x)
 * re-evaluated at every stage (crb_feedback_force, then crb_rk4_stage), all launches issued from here
 * (either dtype).  work: device scratch of crb_feedback_work_bytes(plan) bytes (three state-sized buffers and
 * one force-sized buffer; contents need not be initialised).  Returns the accumulated clock in *t_end.
 * Beams that live in one wave (fewer than 64 thread-carried nodes: the reference's own LQR example has 6 elements)
 * and whose gain fits LDS take ONE launch for the whole rollout instead: the packed lean stepper (several beams per wave,
 * 3 .. 5 reduction levels, gravity absent or of the plain cantilever's form; the general stepper otherwise) with the gain
 * resident in LDS and K (r - x) formed per stage -- on the matrix cores for gains of 21 .. 32 rows, by the node threads
 * otherwise (10 instead of 36 us per step at 6 and at 10 elements, 21 instead of 40 - 48 at 16 .. 20).
 * CRB_FUSED_FEEDBACK=0 / 1 in the environment forces the stage-split / the fused form.
 * Large ensembles of beams with 33 .. 128 thread-carried nodes (fp64, one table set) take ONE persistent launch for the
 * whole rollout (csrc/crb_loop.h): groups of workgroups own 64 beams each, keep their slice of the gain in registers,
 * and alternate between the fp64-MFMA product and the stage arithmetic, handing tiles to each other through L2.
 * CRB_LOOP=0 / 1 forces the stage-split / the persistent form.  A hand-off that does not complete within
 * CRB_LOOP_TIMEOUT_MS (default 2000) makes every workgroup leave; crb_feedback_status reports it. */
size_t crb_feedback_work_bytes(const crb_plan* plan);
/* Which form crb_step_rk4_feedback takes for this plan (without a held input): 0 stage-split, 1 fused (gain in LDS), 2 persistent. */
int crb_feedback_path(const crb_plan* plan);
/* *status = 0, or (group + 1) of the first hand-off of the last crb_step_rk4_feedback call on `work` that timed out (the
 * state is then unusable).  Synchronises `stream`. */
int crb_feedback_status(const crb_plan* plan, const void* work, int32_t* status, void* stream);
int crb_step_rk4_feedback(const crb_plan* plan, void* x, double t0, double dt, int n_steps, const void* gain,
                          const void* ref, const crb_input_desc* input, void* work, double* t_end, void* stream);

/* ---- Adjoint of the closed loop: gradients of a rollout of crb_step_rk4_feedback with respect to the gain and the reference.
 * The controller of examples/lqr_control.py:95-125 (u = K (r - x) in every RK4 stage, FullStateLinear.compute_input,
 * control/full_state_linear.py:81) designs K on the linear model and runs it on the nonlinear rod; these entry points give
 * dL/dK and dL/dr of a loss over that run in one backward sweep instead of two closed-loop rollouts per gain entry. */

/* Cotangents of the controller, ACCUMULATED by crb_step_rk4_feedback_adjoint (device, fp64; NULL = not wanted)
 * (lqr_control.py:95-125, full_state_linear.py:81: the K and the reference of compute_input). */
typedef struct crb_feedback_cotangent {
    void* gain_bar;  /* device [n_cot][n][2n], ACCUMULATED, or NULL */
    void* ref_bar;   /* device [n_cot][B][2n] reduced, ACCUMULATED, or NULL */
} crb_feedback_cotangent;

/* Device bytes of the work buffer of crb_step_rk4_feedback_checkpoint / _adjoint (lqr_control.py:95-125,
 * full_state_linear.py:81).  With S = B * 2 * n_node * 4 doubles (a state) and F = S / 2 (a force), in this order:
 *   every * 4 * S   the four RK4 stage states of every step of one segment (stage 0 = the step's start state)
 *   S, S, F         the RK4 accumulator, the running state of the recompute, the stage's feedback force
 *   n_cot * S  x 3  the stage's seed cotangent, its (df/dx)^T, the running sum of the step's stage cotangents
 *   n_cot * F       the stage's (df/du)^T
 *   n_cot * Z * n * 2n   the gain gradient's partial tiles, only when its beam reduction runs in Z > 1 slices:
 *                   Z = min(ceil(B / 32), ceil(1536 / (ceil(n / 32) * ceil(2n / 32)))), n = n_free
 * = ((4 every + 2 + 3 n_cot) S + (1 + n_cot) F + [Z > 1] n_cot Z n 2n) * sizeof(double).  0 for every < 1 or n_cot < 1. */
size_t crb_rk4_feedback_adjoint_work_bytes(const crb_plan* plan, int every, int n_cot);

/* The forward pass of a differentiable closed-loop rollout (lqr_control.py:95-125, full_state_linear.py:81): n_steps RK4 steps
 * with u = K (ref - x) in every stage, ALWAYS in the stage-split form (crb_feedback_force + crb_rk4_stage per stage, whatever
 * crb_feedback_path says), so x(T) is bitwise crb_step_rk4_feedback with CRB_FUSED_FEEDBACK=0 CRB_LOOP=0.  Writes the state at
 * the start of steps 0, every, 2 every, ... to ckpt [ceil(n_steps / every)][B][2][n_node][4].  rec: one DOF every rec->every
 * steps into out[B][floor(n_steps / every)] as crb_step_rk4_rec takes it (may be NULL); CRB_RECORD_ALL: CRB_EUNSUPPORTED.
 * input: the impulse and / or a held force, both disturbances d(t) added to u and not differentiated (without a held force the
 * launches are exactly those of the stage-split crb_step_rk4_feedback).  work: crb_rk4_feedback_adjoint_work_bytes(plan, every, 1) device bytes are enough.  Does not report to
 * crb_plan_set_status.  Limits and codes as crb_step_rk4_feedback_adjoint. */
int crb_step_rk4_feedback_checkpoint(const crb_plan* plan, void* x, double t0, double dt, int n_steps, int every,
                                     const void* gain, const void* ref, const crb_input_desc* input, const crb_record_desc* rec,
                                     void* ckpt, void* work, double* t_end, void* stream);

/* Adjoint of the rollout crb_step_rk4_feedback_checkpoint ran from t0 (the same dt, n_steps, every, gain, ref and input;
 * lqr_control.py:95-125, full_state_linear.py:81): for n_cot cotangents,
 *   lam      device [n_cot][B][2][n_node][4], in place: dL/dx(T) on entry, dL/dx(0) on exit (only free-DOF entries change)
 *   rec_bar  the record of the forward pass with out = its cotangent [n_cot][B][n_rec], or NULL
 *   grad     gain_bar += dL/dK, ref_bar += dL/d ref; gain_bar == NULL skips its product
 * Segments last to first: each is recomputed from its checkpoint (the stage states go straight into work), then swept back
 * per stage: crb_rhs_vjp at the stage state, P = ubar . K with s = xbar - P, ref_bar += P and the next stage's seed in its
 * epilogue, gain_bar += sum_b ubar_b (x) (ref_b - X_b) -- both products on v_mfma_f64_16x16x4_f64, about 12 launches per step (the
 * beam reduction of large ensembles runs in slices whose partial tiles a second launch sums in a fixed order).
 * The RHS is affine in u, so only the stage STATES are needed, not the stage forces.  Every sum has a fixed order (no atomics)
 * and every stage accumulates in place in sweep order: lam, gain_bar and ref_bar are bitwise independent of `every`, D
 * cotangents in one call are bitwise D calls of one, and two identical calls agree bitwise.  A non-finite cotangent of one beam
 * stays in that beam's rows of lam and ref_bar; it reaches gain_bar (a sum over beams).
 * Checked before the device is touched (host-only plans show them; valid calls there: CRB_ENODEV): CRB_EUNSUPPORTED for fp32
 * plans, plans with more than one free-DOF set (mixed topology), beams of more than 256 thread-carried nodes, a gravity table
 * crb_rhs_vjp refuses and CRB_RECORD_ALL; CRB_EINVAL for n_cot outside 1 .. 65535, a NULL gain, lam, ckpt, work or
 * grad, bad n_steps / every / dt, and lam, gain_bar or ref_bar aliasing ckpt, work, gain, ref or each other.  crb_last_error()
 * names the argument. */
int crb_step_rk4_feedback_adjoint(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                  int n_steps, int every, const void* gain, const void* ref, const crb_input_desc* input,
                                  const crb_record_desc* rec_bar, const crb_feedback_cotangent* grad, void* work, void* stream);

/* crb_step_rk4 plus strided recording of one DOF (rec may be NULL). */
int crb_step_rk4_rec(const crb_plan* plan, void* x, double t0, double dt, int n_steps, const crb_input_desc* input,
                     const crb_record_desc* rec, double* t_end, void* stream);

/* A piecewise-constant control sequence for the RK4 rollout family: the `u` of get_dynamic_system()(t, x, u)
 * (dynamic_beam_model.py:343-362) as a zero-order hold, what the u(t) closures of lqr_control.py:33-41 hand the integrator --
 * here a whole shooting / MPC horizon in one call.  Step i of the call (counted from the call's first step) applies vector
 * i / hold in all four RK4 stages, on top of the impulse if there is one; n_steps <= n_intervals * hold, the last interval may
 * be cut short.  n_intervals = 1, hold >= n_steps is crb_input_desc.f_held.  A schedule and input->f_held together are refused. */
typedef struct crb_input_schedule {
    const void* f_sched;   /* device [n_intervals][B][n_node][4], plan dtype */
    int32_t n_intervals;   /* K >= 1 */
    int32_t hold;          /* steps per interval, >= 1 (RK4 steps; implicit steps in the crb_step_implicit*_sched calls) */
} crb_input_schedule;

/* The RK4 rollout family with a control schedule: each call is its counterpart above (the same arguments, clock, impulse
 * window, recording and status; bitwise the chain of one call per interval with f_held = that interval's vector) and, with
 * sched == NULL, exactly that call.  The schedule is switched inside the kernels: one launch (one launch pair per checkpoint
 * segment for the adjoint), whatever n_intervals.  Checked before the device is touched, so that host-only plans show them
 * (valid calls on those: CRB_ENODEV): CRB_EINVAL for a NULL f_sched, n_intervals < 1, hold < 1, n_steps > n_intervals * hold,
 * a schedule together with input->f_held (or with its tangent df_held / cotangent f_held_bar), d_sched / sched_bar without a
 * schedule, sched_bar aliasing lam, work, ckpt or f_sched; CRB_EUNSUPPORTED for fp32 plans in the tangent and adjoint calls.
 * crb_last_error() names the offending argument.
 *   crb_step_rk4_sched            crb_step_rk4_rec; fp64 and fp32 plans
 *   crb_step_rk4_tangent_sched    crb_step_rk4_tangent; d_sched: device [n_dir][n_intervals][B][n_node][4], the tangent of the
 *                                 schedule per direction, or NULL (= 0)
 *   crb_step_rk4_checkpoint_sched crb_step_rk4_checkpoint
 *   crb_step_rk4_adjoint_sched    crb_step_rk4_adjoint run after crb_step_rk4_checkpoint_sched with the same schedule;
 *                                 sched_bar: device [n_cot][n_intervals][B][n_node][4], dL/d f_sched, ACCUMULATED as
 *                                 f_held_bar is (intervals the rollout does not reach are left as they are), or NULL
 *   crb_step_rk4_adjoint_params_sched  crb_step_rk4_adjoint_params likewise */
int crb_step_rk4_sched(const crb_plan* plan, void* x, double t0, double dt, int n_steps, const crb_input_desc* input,
                       const crb_input_schedule* sched, const crb_record_desc* rec, double* t_end, void* stream);
int crb_step_rk4_tangent_sched(const crb_plan* plan, void* x, void* dx, int n_dir, double t0, double dt, int n_steps,
                               const crb_input_desc* input, const crb_input_tangent* dinput, const crb_input_schedule* sched,
                               const void* d_sched, double* t_end, void* stream);
int crb_step_rk4_checkpoint_sched(const crb_plan* plan, void* x, double t0, double dt, int n_steps, int every,
                                  const crb_input_desc* input, const crb_input_schedule* sched, const crb_record_desc* rec,
                                  void* ckpt, double* t_end, void* stream);
int crb_step_rk4_adjoint_sched(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double dt, int n_steps,
                               int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                               const crb_input_cotangent* grad, const crb_input_schedule* sched, void* sched_bar, void* work,
                               void* stream);
int crb_step_rk4_adjoint_params_sched(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                      int n_steps, int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                                      const crb_input_cotangent* grad, const crb_param_cotangent* pgrad,
                                      const crb_input_schedule* sched, void* sched_bar, void* work, void* stream);

/* ---- Adjoint of the implicit stepper: gradients through stiff rollouts (csrc/crb_implicit_adjoint.h).
 * The exact discrete adjoint of the map crb_step_implicit computes (the implicit midpoint rule with n_iter modified-Newton
 * iterations on A = M + h^2/4 K0, each step's iteration starting from the previous step's final iterate, 0 at the first step
 * of a call) -- not of the converged rule.  The three calls below follow crb_rk4_adjoint_work_bytes,
 * crb_step_rk4_checkpoint and crb_step_rk4_adjoint; lam, rec_bar and grad keep their layouts and accumulate semantics.
 *
 * crb_implicit_adjoint_work_bytes: device bytes of the work buffer of crb_step_implicit_adjoint,
 *     (every * ((2 + n_iter) * B * n_node * 4 + 1) + n_cot * B * n_node * 4) * sizeof(double)
 * -- per step of one segment its start state (q0, v0) [B][2][n_node][4], then the iterates a^0 .. a^{n_iter-1}
 * [n_iter][B][n_node][4] of every step, then the steps' clocks, then per cotangent the carry [n_cot][B][n_node][4] (the
 * cotangent of a segment's starting iterate, handed to the segment before it).  0 for a NULL plan, every < 1, n_iter outside
 * 1 ... 16 or n_cot outside 1 ... 65535.
 *
 * crb_step_implicit_checkpoint: crb_step_implicit (same clock, same input, midpoint sampling; x advances in place, *t_end as
 * there) in the adjoint's own arithmetic, writing the state and the starting iterate of steps 0, every, 2 every, ... to
 * ckpt [ceil(n_steps / every)][B][3][n_node][4] (device; planes q, v, a).  rec: as crb_step_rk4_rec (may be NULL).  x agrees
 * with crb_step_implicit to rounding, not bitwise.  Per-beam status is not written.
 *
 * crb_step_implicit_adjoint: the gradient of a scalar loss L(x(T), samples) of the rollout crb_step_implicit_checkpoint ran
 * from t0 (the same h, n_steps, n_iter, every and input) with respect to x(0), amp and f_held, for n_cot cotangents:
 *   lam      device [n_cot][B][2][n_node][4], in place: dL/dx(T) on entry, dL/dx(0) on exit
 *   rec_bar  the record of the forward pass with out = the cotangent of its samples (as crb_step_rk4_adjoint), or NULL
 *   grad     amp_bar / f_held_bar += dL/d amp, dL/d f_held (may be NULL)
 *   work     crb_implicit_adjoint_work_bytes(plan, every, n_iter, n_cot) device bytes
 * Per segment, last to first: one launch recomputes the segment's step data from its checkpoint, one sweeps it back for all
 * cotangents.  The result is bitwise independent of `every`, and D cotangents in one call are bitwise D calls of one.
 *
 * Refusals, all before the device is touched, crb_last_error() naming the entry point, in this order: CRB_EINVAL for a NULL
 * plan or buffer, aliasing buffers, n_cot outside 1 ... 65535, n_steps < 0, every < 1, n_iter outside 1 ... 16, h <= 0, a bad
 * input or record description, amp_bar without an impulse input; CRB_EUNSUPPORTED for fp32 plans and beams of more than 256
 * thread-carried nodes; CRB_ENODEV for host-only plans.  *t_end is written only by a call that is not refused.
 * Not covered: the damped variant (rho_inf < 1) and the closed loop.  Parameter gradients: crb_step_implicit_adjoint_params
 * below.  Control schedules: the *_sched calls below. */
size_t crb_implicit_adjoint_work_bytes(const crb_plan* plan, int every, int n_iter, int n_cot);
int crb_step_implicit_checkpoint(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter, int every,
                                 const crb_input_desc* input, const crb_record_desc* rec, void* ckpt, double* t_end, void* stream);
int crb_step_implicit_adjoint(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double h, int n_steps,
                              int n_iter, int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                              const crb_input_cotangent* grad, void* work, void* stream);

/* ---- The implicit family with a control schedule (crb_input_schedule; `hold` counts implicit steps: step i of the call
 * applies vector i / hold at its midpoint, on top of the impulse; n_steps <= n_intervals * hold, the last interval may be cut
 * short).  Each call is its counterpart above -- the same arguments, clock, impulse window, recording and status -- and, with
 * sched == NULL (and sched_bar == NULL), exactly that call.  The schedule is switched inside the kernels: one launch (one
 * launch pair per checkpoint segment for the adjoint), whatever n_intervals.
 * A scheduled call IS the chain of one call per interval with f_held = that interval's vector, bitwise.  crb_step_implicit
 * starts the first step of a call from the iterate a^0 = 0, so the first step of EVERY interval starts its modified-Newton
 * iteration from a^0 = 0, and the adjoint drops the carried cotangent of the starting iterate there, as it does at step 0 of a
 * call.  Consequence: a schedule of K equal vectors is the chain of K calls, not bitwise the one call with that f_held; the
 * two differ by the size of the iteration's convergence error (n_iter = 2: DESIGN.md section 10 has the measured figure).
 *   crb_step_implicit_sched             crb_step_implicit (the damped variant has no scheduled form)
 *   crb_step_implicit_checkpoint_sched  crb_step_implicit_checkpoint; the checkpoint layout is unchanged, and the `a` plane of
 *                                       a checkpoint taken at an interval's first step holds zeros
 *   crb_step_implicit_adjoint_sched     crb_step_implicit_adjoint run after crb_step_implicit_checkpoint_sched with the same
 *                                       schedule; sched_bar: device [n_cot][n_intervals][B][n_node][4], dL/d f_sched,
 *                                       ACCUMULATED as f_held_bar is (intervals the rollout does not reach are left as they
 *                                       are; padding and constrained entries as in f_held_bar), or NULL.  The work buffer is
 *                                       that of crb_implicit_adjoint_work_bytes.
 * Refusals with a schedule, all before the device is touched, crb_last_error() naming the entry point and the argument, in this
 * order: the counterpart's own CRB_EINVAL cases in their order; then CRB_EINVAL for a NULL f_sched, n_intervals < 1, hold < 1,
 * n_steps > n_intervals * hold, a schedule together with input->f_held or with grad->f_held_bar, sched_bar without a schedule,
 * sched_bar aliasing lam, work, ckpt, f_sched or amp_bar; then CRB_EUNSUPPORTED for fp32 plans and beams of more than 256
 * thread-carried nodes; then CRB_ENODEV for host-only plans. */
int crb_step_implicit_sched(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter,
                            const crb_input_desc* input, const crb_input_schedule* sched, const crb_record_desc* rec,
                            double* t_end, void* stream);
int crb_step_implicit_checkpoint_sched(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter, int every,
                                       const crb_input_desc* input, const crb_input_schedule* sched, const crb_record_desc* rec,
                                       void* ckpt, double* t_end, void* stream);
int crb_step_implicit_adjoint_sched(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double h,
                                    int n_steps, int n_iter, int every, const crb_input_desc* input,
                                    const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                    const crb_input_schedule* sched, void* sched_bar, void* work, void* stream);

/* ---- Parameter gradients of the implicit adjoint: stiffness, drag and gravity, the iteration matrix included
 * (csrc/crb_implicit_paramgrad.h).  crb_step_implicit_adjoint(_sched) with one more output, the crb_param_cotangent of
 * crb_step_rk4_adjoint_params: the same struct, the same record [n_cot][B][n_node][8] = (sA, sI, sD, gx, gy, 0, 0, 0) per node
 * (sA, sI of node j: the element left of it), param_bar ACCUMULATED.  lam, grad and sched_bar come out bitwise as from the
 * plain call.
 * E and I enter the iteration matrix A = M + alpha K0(theta), alpha = h^2 / 4, as well as the force.  With iteration i of a step
 *     q_m = qp + alpha a^i,  v_m = v0 + h/2 a^i,  a^{i+1} = A^-1 (F(q_m, v_m; theta) + u + alpha K0(theta) a^i)
 * and gbar = A^-T abar of that iteration (what the sweep forms), dA^-1 = -A^-1 (alpha dK0) A^-1 gives its contribution
 *     theta_bar += gbar^T dF/dtheta (q_m, v_m)  +  alpha gbar^T (dK0/dtheta) (a^i - a^{i+1})
 * The first term is crb_step_rk4_adjoint_params' sum with gbar in the place of rbar; the second exists for sA and sI only (drag
 * and gravity are not in K0): dK0/dsA is the element's linear stiffness with the EI entries zeroed, dK0/dsI with the EA entries
 * zeroed, the axial block [[c0, -s c0], [-c0, c0]] with s = 0 for the shipped nonlinear element.  It vanishes as the iteration
 * converges and is what a fixed iteration count leaves; a^0 = 0 at the first step of a call and of every schedule interval.
 * Per segment, last to first: the recompute (which also keeps the final iterate of the segment's last step), the storing sweep
 * (gbar of every iteration to the work buffer) and one reduction launch; fixed summation order, no atomics: param_bar is
 * bitwise independent of `every`, and D cotangents in one call are bitwise D calls of one.
 *
 * crb_implicit_adjoint_params_work_bytes:
 *     crb_implicit_adjoint_work_bytes(plan, every, n_iter, n_cot) + (every * n_iter * n_cot + 1) * B * n_node * 4 * sizeof(double)
 * -- after the plain buffer gbar [every][n_iter][n_cot][B][n_node][4], then the final iterate [B][n_node][4].  0 where the
 * plain call returns 0.
 *
 * Refusals, all before the device is touched, in this order: CRB_EINVAL for a NULL plan, ckpt or lam, a NULL pgrad or
 * pgrad->param_bar, a NULL work buffer (each named in crb_last_error()), lam aliasing another buffer, param_bar aliasing lam,
 * work or ckpt, other aliasing buffers, n_cot, n_steps, every, n_iter or h out of range; then every further check of
 * crb_step_implicit_adjoint(_sched) in its order, param_bar aliasing the schedule or sched_bar with the schedule's cases;
 * CRB_EUNSUPPORTED for fp32 plans and beams of more than 256 thread-carried nodes; CRB_ENODEV for host-only plans.
 * Not covered: length, cross-section area and density (they enter M), the damped variant, the sampled-data loop. */
size_t crb_implicit_adjoint_params_work_bytes(const crb_plan* plan, int every, int n_iter, int n_cot);
int crb_step_implicit_adjoint_params(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double h, int n_steps,
                                     int n_iter, int every, const crb_input_desc* input, const crb_record_desc* rec_bar,
                                     const crb_input_cotangent* grad, const crb_param_cotangent* pgrad, void* work, void* stream);
int crb_step_implicit_adjoint_params_sched(const crb_plan* plan, const void* ckpt, void* lam, int n_cot, double t0, double h,
                                           int n_steps, int n_iter, int every, const crb_input_desc* input,
                                           const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                           const crb_param_cotangent* pgrad, const crb_input_schedule* sched, void* sched_bar,
                                           void* work, void* stream);

/* ---- Tangent of the implicit stepper: forward-mode derivatives of stiff rollouts (csrc/crb_implicit_tangent.h).
 * crb_step_implicit with the tangent of its discrete map alongside: the exact derivative of what crb_step_implicit computes
 * (n_iter modified-Newton iterations per step on A = M + h^2/4 K0, each step's iteration and its tangent starting from the
 * previous step's final iterate, both 0 at the first step of a call) -- the statement the implicit adjoint transposes -- at the
 * steps h = 1e-4 ... 1e-3 s that take the horizons the examples integrate with solve_ivp(method="LSODA")
 * (examples/example_utilities.py:153-159).  With identity seeds it gives the discrete-time pair (A_d, B_d) of the sampled
 * plant x_{k+1} = Phi_h(x_k, u_k) that a sampled design of control/linear_quadratic_regulator.py's controller needs.
 *   x, dx, n_dir, input, dinput   as crb_step_rk4_tangent (x advances in place, dx [n_dir][B][2][n_node][4] in place, per-beam
 *                                 status written); the clock and the midpoint sampling of the impulse are crb_step_implicit's
 *   sched, d_sched                as crb_step_rk4_tangent_sched, `hold` counting implicit steps.  A scheduled call is the chain
 *                                 of one call per interval with dx carried: the first step of every interval starts from
 *                                 a^0 = 0 and da^0 = 0
 * Refusals, all before the device is touched, crb_last_error() naming the entry point, in this order: CRB_EINVAL for a NULL
 * plan, state or tangent, n_dir outside 1 ... 65535, n_steps < 0, n_iter outside 1 ... 16, h <= 0, a bad input description,
 * d_amp without an impulse input, then the schedule's cases (a NULL f_sched, n_intervals < 1, hold < 1,
 * n_steps > n_intervals * hold, a schedule together with input->f_held or dinput->df_held, d_sched without a schedule); then
 * CRB_EUNSUPPORTED for fp32 plans and beams of more than 256 thread-carried nodes; then CRB_ENODEV for host-only plans.
 * *t_end is written only by a call that is not refused; n_steps == 0 returns CRB_OK and touches nothing else.
 * Not covered: the damped variant (rho_inf < 1), tangents of recorded samples, parameter tangents.  The closed loop
 * u_k = f_held + K (r - x_k) has its own entry point, crb_step_implicit_feedback_tangent below. */
int crb_step_implicit_tangent(const crb_plan* plan, void* x, void* dx, int n_dir, double t0, double h, int n_steps, int n_iter,
                              const crb_input_desc* input, const crb_input_tangent* dinput, double* t_end, void* stream);
int crb_step_implicit_tangent_sched(const crb_plan* plan, void* x, void* dx, int n_dir, double t0, double h, int n_steps,
                                    int n_iter, const crb_input_desc* input, const crb_input_tangent* dinput,
                                    const crb_input_schedule* sched, const void* d_sched, double* t_end, void* stream);

/* ---- Sampled-data state feedback inside the implicit stepper: a digital (zero-order-hold) controller on the stiff loop.
 * n_steps implicit-midpoint steps of size h; sample k covers steps k * hold ... (k + 1) * hold - 1 (the last sample may be cut
 * short by n_steps).  At the top of a sample's first step e = r - x is formed from the state as it stands (reduced ordering),
 * u_k = f_held + K e becomes the held input of the sample and the starting iterate is reset to 0; the impulse is added on top
 * as in every implicit call.  The call IS the chain of one crb_step_implicit call per sample with f_held = u_k.  u_k is
 * constant over a step, so the iteration matrix A = M + h^2/4 K0 is the open loop's: the feedback adds no stiffness (inside
 * the RK4 stages, crb_step_rk4_feedback, the LQR loop needs dt <= 8.6e-6 s).
 *   gain    device [n][2n] row-major, reduced ordering (as crb_step_rk4_feedback); one gain for the ensemble
 *   ref     device [B][2n] reduced ordering, or NULL (= 0)
 *   input   impulse and f_held [B][n_node][4] as in crb_step_implicit; rec as there, its stride `every` a divisor or a
 *           multiple of hold
 *   u_out   device [ceil(n_steps / hold)][B][n_node][4] or NULL: the total held input u_k of every sample in the layout of a
 *           crb_input_schedule's records (zeros at constrained DOFs) -- crb_step_implicit_sched with f_sched = u_out and this
 *           hold replays the call bitwise wherever it runs the general implicit kernel
 *   work    device, crb_implicit_feedback_work_bytes(plan) bytes (never NULL)
 * Two forms, the same map (they differ by the rounding of K e, whose summation order differs):
 *   in-kernel (crb_implicit_feedback_path = 1): beams that live in one wave and whose gain fits LDS (up to ~30 elements) -- the
 *           whole call is ONE launch, the product in LDS or on the matrix cores (gains of 21 ... 32 rows)
 *   chain (0): everything else -- per sample one ensemble GEMM (crb_feedback_force) and one crb_step_implicit launch, issued
 *           inside this call.  CRB_IMPLICIT_FEEDBACK=0 forces this form, =1 the in-kernel form wherever the gain fits.
 * A beam that goes non-finite is marked (crb_plan_set_status) with the ensemble's step count at the end of the call.
 * Refusals, all before the device is touched, crb_last_error() naming the entry point, in this order: CRB_EINVAL for a NULL
 * plan, x, gain or work, n_steps < 0, h <= 0, n_iter < 1, hold < 1, a bad record or a record stride that neither divides hold
 * nor is a multiple of it, a bad input description; then CRB_EUNSUPPORTED for fp32 plans, beams of more than 256 thread-carried
 * nodes, ensembles of mixed topology or per-beam free-DOF sets; then CRB_ENODEV for host-only plans.  n_steps == 0 sets *t_end
 * and returns CRB_OK.  Not covered: per-beam gain groups, the damped variant.  The adjoint of this map:
 * crb_step_implicit_feedback_adjoint below. */
int crb_step_implicit_feedback(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter, int hold,
                               const void* gain, const void* ref, const crb_input_desc* input, const crb_record_desc* rec,
                               void* u_out, void* work, double* t_end, void* stream);
size_t crb_implicit_feedback_work_bytes(const crb_plan* plan);
int crb_implicit_feedback_path(const crb_plan* plan);   /* 0 chain, 1 in-kernel */

/* ---- Adjoint of the sampled-data implicit loop: gradients of a rollout of crb_step_implicit_feedback with respect to the start
 * state, the gain, the reference, the impulse amplitude and the held force, in one backward sweep -- tuning the digital gain
 * that runs at h = 1e-3 s on the nonlinear rod (examples/tune_digital_gain.py).
 *
 * The map, sample k over steps k * hold ... (k + 1) * hold - 1:  u_k = f_held + K (r - x_k) in reduced ordering,
 * x_{k+1} = Phi(x_k, u_k) = the sample's implicit-midpoint steps with f_held = u_k, the first step's iteration started from
 * a^0 = 0 (one crb_step_implicit call per sample; one interval of a crb_input_schedule).
 * Its transpose, last sample first, with lambda = dL/dx_{k+1} plus the cotangents of the samples recorded inside the interval:
 *   the implicit sweep over the sample's steps (crb_step_implicit_adjoint's kernel) gives lambda' = (dPhi/dx)^T lambda,
 *   ubar_k = (dPhi/du)^T lambda and the amp_bar contributions; a^0 = 0 is a constant, so the cotangent carried through the
 *   starting iterate is dropped at the sample's first step (the launch that ends a sample starts with carry_in = 0);
 *   P = ubar_k,red . K            [rows x n] . [n x 2n], rows = n_cot * B
 *   dL/dx_k = lambda' - P,   ref_bar += P,   f_held_bar += ubar_k,   gain_bar += sum_b ubar_k,b (x) (r_b - x_k,b).
 *
 * crb_implicit_feedback_adjoint_work_bytes: device bytes of the work buffer of the two calls.  With F = B * n_node * 4 doubles
 * (a force record), in this order:
 *   every * 2F, every * n_iter * F, every   a segment's step start states, iterates and clocks (crb_implicit_adjoint_work_bytes)
 *   n_cot * F                               the cotangent of the starting iterate the sweep's launches write
 *   n_cot * (every / hold) * F              ubar_k of every sample of a segment, [n_cot][every / hold][B][n_node][4]
 *   n_cot * Z * n * 2n                      the gain gradient's running partial tiles, only when its beam reduction runs in Z > 1
 *                                           slices (Z as in crb_rk4_feedback_adjoint_work_bytes)
 * = (every ((2 + n_iter) F + 1) + n_cot (1 + every / hold) F + [Z > 1] n_cot Z n 2n) * sizeof(double).  0 for a NULL plan,
 * every < 1, hold < 1, every not a multiple of hold, n_iter outside 1 .. 16 or n_cot outside 1 .. 65535.
 *
 * crb_step_implicit_feedback_checkpoint: the forward pass in the adjoint's own arithmetic, ALWAYS as the chain (whatever
 * crb_implicit_feedback_path says): per sample crb_feedback_force plus the held force into record k of u_ckpt, then one
 * checkpoint launch of the implicit adjoint's kernel over the sample's steps.  x agrees with crb_step_implicit_feedback to
 * rounding, not bitwise.
 *   every    steps per checkpoint segment, a multiple of hold: a checkpoint always sits on a sample start
 *   ckpt     device [ceil(n_steps / every)][B][3][n_node][4]: (q, v, starting iterate) at steps 0, every, ...; the third plane
 *            holds zeros (a sample starts from a^0 = 0)
 *   u_ckpt   device [ceil(n_steps / hold)][B][n_node][4], required: u_k of every sample, laid out as u_out of
 *            crb_step_implicit_feedback (zeros at constrained DOFs and padding) -- the schedule the adjoint's recompute reads
 *   rec      one DOF, its stride a divisor or a multiple of hold (may be NULL); CRB_RECORD_ALL: CRB_EUNSUPPORTED
 *   work     crb_implicit_feedback_adjoint_work_bytes(plan, every, n_iter, hold, 1) bytes are enough
 * Does not write per-beam status (crb_plan_set_status).
 *
 * crb_step_implicit_feedback_adjoint: the adjoint of the rollout the pass ran from t0 (the same h, n_steps, n_iter, hold, every,
 * gain, ref and input), for n_cot cotangents:
 *   lam      device [n_cot][B][2][n_node][4], in place: dL/dx(T) on entry, dL/dx(0) on exit
 *   rec_bar  the record of the pass with out = its cotangent [n_cot][B][n_rec], or NULL
 *   grad     gain_bar += dL/dK (NULL skips its product; the other results are bitwise unchanged), ref_bar += dL/d ref
 *   igrad    amp_bar += dL/d amp (needs an impulse), f_held_bar += dL/d f_held [n_cot][B][n_node][4]; either or igrad may be NULL
 * Per segment, last to first: one scheduled recompute launch from the checkpoint (f_sched = u_ckpt, this hold); per sample,
 * last first, one sweep launch over its steps that writes ubar_k into the sample's slot of work, and one boundary launch
 * (P on v_mfma_f64_16x16x4_f64, lam -= P, ref_bar += P, f_held_bar += ubar_k); then ONE gain-gradient launch for all samples of the
 * segment, each workgroup adding every sample's beam reduction to a running tile in sweep order.  The beam reduction of large
 * ensembles runs in slices whose tiles persist in work across the segments and are summed in ascending order at the end of
 * the call.  No floating-point atomics; every sum has a fixed order: lam and every cotangent are bitwise independent of
 * `every`, D cotangents in one call are bitwise D calls of one, and two identical calls agree bitwise.  A non-finite cotangent
 * of one beam stays in that beam's rows of lam, ref_bar and f_held_bar; it reaches gain_bar (a sum over beams).
 *
 * Refusals, all before the device is touched, crb_last_error() naming the entry point and the argument, in this order:
 * CRB_EINVAL for a NULL plan or buffer (the pass: x, gain, ckpt, u_ckpt, work; the adjoint: ckpt, u_ckpt, lam, gain, work, grad);
 * aliasing (the pass: x, ckpt, u_ckpt, work against each other, gain, ref, rec->out, input->f_held; the adjoint: lam, gain_bar,
 * ref_bar, amp_bar, f_held_bar against ckpt, u_ckpt, work, gain, ref or each other); n_cot outside 1 .. 65535; n_steps < 0;
 * every < 1; hold < 1; every % hold != 0; n_iter outside 1 .. 16; h <= 0; a bad record, or a record stride that neither divides
 * hold nor is a multiple of it; a bad input; amp_bar without an impulse.  Then CRB_EUNSUPPORTED for fp32 plans, beams of more
 * than 256 thread-carried nodes, ensembles of mixed topology, CRB_RECORD_ALL.  Then CRB_ENODEV for host-only plans.
 * n_steps == 0 returns CRB_OK and, in the pass, sets *t_end.
 * Not covered: an in-kernel sweep for gains that fit LDS (the adjoint is always the chain), per-beam gain groups, the damped
 * variant, parameter gradients, checkpoint segments shorter than a sample. */
size_t crb_implicit_feedback_adjoint_work_bytes(const crb_plan* plan, int every, int n_iter, int hold, int n_cot);
int crb_step_implicit_feedback_checkpoint(const crb_plan* plan, void* x, double t0, double h, int n_steps, int n_iter, int hold,
                                          int every, const void* gain, const void* ref, const crb_input_desc* input,
                                          const crb_record_desc* rec, void* ckpt, void* u_ckpt, void* work, double* t_end,
                                          void* stream);
int crb_step_implicit_feedback_adjoint(const crb_plan* plan, const void* ckpt, const void* u_ckpt, void* lam, int n_cot,
                                       double t0, double h, int n_steps, int n_iter, int hold, int every, const void* gain,
                                       const void* ref, const crb_input_desc* input, const crb_record_desc* rec_bar,
                                       const crb_feedback_cotangent* grad, const crb_input_cotangent* igrad, void* work,
                                       void* stream);

/* ---- Tangent of the sampled-data implicit loop: forward-mode derivatives of a rollout of crb_step_implicit_feedback with
 * respect to the start state, the gain, the reference, the held force and the impulse amplitude, n_dir directions in one call
 * (csrc/crb_implicit_feedback_tangent.h).  With identity seeds it gives the closed loop's sampled state-transition matrix
 * d x_{k+N} / d x_k on the nonlinear rod -- whether the regulator of control/linear_quadratic_regulator.py:84-191, designed on
 * crb_step_implicit_tangent's (A_d, B_d) and applied as control/full_state_linear.py:81 applies it, is stable on the plant the
 * stepper runs -- and the Gauss-Newton columns of gain tuning and reference shaping.
 *
 * The map is crb_step_implicit_feedback_adjoint's.  Sample k covers steps k * hold ... (k + 1) * hold - 1 (the last sample may
 * be cut short by n_steps); at its top, in reduced ordering,
 *     u_k  = f_held  + K (r - x_k)
 *     du_k = df_held + K (dr - dx_k) + dK (r - x_k)          per direction
 * and the sample's steps are one interval of crb_step_implicit_tangent_sched with the held input u_k and its tangent du_k:
 * a^0 = 0 and da^0 = 0 at the sample's first step, the impulse and d_amp added on the impulse DOF while the midpoint clock
 * __dadd_rn(tc, 0.5 h) < duration, the clock advanced by __dadd_rn.
 *   x        device [B][2][n_node][4], advances in place; per-beam status (crb_plan_set_status) is written by direction 0 with
 *            the ensemble's step count at the end of the call
 *   dx       device [n_dir][B][2][n_node][4], in place: the seeds on entry, dx(T) on exit
 *   gain     device [n][2n] row-major; ref device [B][2n] or NULL (= 0)
 *   dfb      d_gain [n_dir][n][2n] row-major, d_ref [n_dir][B][2n]; either or dfb may be NULL (= 0).  With d_gain NULL the
 *            product dK (r - x_k) is skipped entirely (no loads, no MFMAs) and every other result is bitwise unchanged
 *   input    impulse and f_held as crb_step_implicit_feedback; dinput: d_amp [n_dir][B] (needs an impulse) and df_held
 *            [n_dir][B][n_node][4] as crb_step_implicit_tangent; either or dinput may be NULL (= 0)
 *   u_out    device [K][B][n_node][4], du_out device [n_dir][K][B][n_node][4], K = ceil(n_steps / hold), either may be NULL: the
 *            held input of every sample and its tangent, zeros at constrained DOFs and padding; du_out in the layout
 *            crb_step_implicit_tangent_sched takes as d_sched (with f_sched = u_out and this hold it replays x and dx bitwise)
 *   work     device, crb_implicit_feedback_tangent_work_bytes(plan, n_dir) = (1 + n_dir) * B * n_node * 4 * sizeof(double) bytes:
 *            one force record for u_k and one per direction for du_k, used where u_out / du_out is NULL (never NULL itself).
 *            0 for a NULL plan or n_dir outside 1 .. 65535
 * The call always runs the chain form, as the adjoint does: per sample one boundary launch (both products on
 * v_mfma_f64_16x16x4_f64, straight from the state layout and to the force layout) and one launch of the implicit tangent's
 * scheduled kernel over the sample's steps.  A workgroup of the boundary kernel owns 32 beams x 32 force DOFs of ONE direction
 * (or of u) and sums K (dr - dx) and then dK (r - x) over 2n in ascending order: no floating-point atomics, every output
 * element has one owner; D directions in one call are bitwise D calls of one, two identical calls agree bitwise, and u does
 * not depend on n_dir.  A non-finite seed stays in its beam and direction.  x agrees with crb_step_implicit_feedback to
 * rounding, not bitwise (the products sum in another order).
 *
 * Refusals, all before the device is touched, crb_last_error() naming the entry point and the argument, in this order:
 * CRB_EINVAL for a NULL plan, x, dx, gain or work; dx, u_out, du_out or work aliasing each other, x, gain, ref, d_gain, d_ref,
 * f_held, amp, df_held or d_amp; n_dir outside 1 .. 65535; n_steps < 0; n_iter outside 1 .. 16; h <= 0; hold < 1; a bad input
 * description; d_amp without an impulse.  Then CRB_EUNSUPPORTED for fp32 plans, beams of more than 256 thread-carried nodes,
 * ensembles of mixed topology or per-beam free-DOF sets.  Then CRB_ENODEV for host-only plans.  n_steps == 0 sets *t_end,
 * returns CRB_OK and touches nothing else.
 * Not covered: an in-kernel (one-launch) form, tangents of recorded samples, per-beam gain groups, the damped variant, fp32,
 * parameter tangents, the tangent of the RK4 closed loop (crb_step_rk4_feedback). */
typedef struct crb_feedback_tangent {
    const void* d_gain;   /* [n_dir][n][2n] row-major, or NULL */
    const void* d_ref;    /* [n_dir][B][2n] reduced, or NULL */
} crb_feedback_tangent;
size_t crb_implicit_feedback_tangent_work_bytes(const crb_plan* plan, int n_dir);
int crb_step_implicit_feedback_tangent(const crb_plan* plan, void* x, void* dx, int n_dir, double t0, double h, int n_steps,
                                       int n_iter, int hold, const void* gain, const void* ref, const crb_feedback_tangent* dfb,
                                       const crb_input_desc* input, const crb_input_tangent* dinput, void* u_out, void* du_out,
                                       void* work, double* t_end, void* stream);

/* out[b] = x[b][plane][node][dof]  (e.g. tip displacement = plane 0, node n_elem, dof 1;
 * lqr_control.py:168) */
int crb_gather_dof(const crb_plan* plan, const void* x, int plane, int node, int dof, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CRBEAM_H */
