// crbeam.hip -- C ABI of libcrbeam.so (include/crbeam.h): plan construction on the host,
// kernel launches on gfx950.  Build: hipcc -O3 --offload-arch=gfx950 -shared -fPIC.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/crbeam.h"
#include "crb_kernels.h"
#include "crb_lean_launch.h"
#include "crb_loop_launch.h"
#include "crb_ctrl_launch.h"
#include "crb_static_launch.h"
#include "crb_tangent_launch.h"
#include "crb_adjoint_launch.h"
#include "crb_implicit_adjoint_launch.h"
#include "crb_implicit_tangent_launch.h"
#include "crb_implicit_feedback_launch.h"
#include "crb_feedback_adjoint_launch.h"
#include "crb_implicit_feedback_adjoint_launch.h"
#include "crb_implicit_feedback_tangent_launch.h"
#include "crb_host.h"
#include "crb_blocked.h"

using namespace crb;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) return fail(CRB_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// ---- device-side assembly (crb_assemble_kernel) -------------------------------------------------
template <typename X>
struct DevBuf {
    X* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(X)) == hipSuccess ? 0 : -1; }
    int upload(const X* h, size_t n) {
        if (alloc(n)) return -1;
        return (!n || hipMemcpy(p, h, n * sizeof(X), hipMemcpyHostToDevice) == hipSuccess) ? 0 : -1;
    }
};
// The assembly kernel's inputs stay on the device for the life of the plan: the implicit stepper factorises
// A = M + alpha K0 from them for every new step size (crb_step_implicit).
struct AsmInputs {
    DevBuf<double> dL, dE, dI, dRho, dA, dWet, dCd, dFd, dNormScratch;
    DevBuf<uint8_t> dNl, dFree;
    DevBuf<crb::GravTab> dGrav;
    DevBuf<int32_t> dNe;
    DevBuf<uint32_t> dFl;
    crb::AsmParams a;   // the launch parameters of the plan's own assembly (pointers into the buffers above)
    int nd = 1, threads = 64;
    size_t smem = 0;
};

struct crb_plan {
    int device = -1, dtype = CRB_F64, B = 0;
    int n_elem = 0, n_node = 0, n_free = 0, off = 0, S = 0, G = 1, NT = 64;
    int levels = 0, levels_full = 0, lognw = 0;
    size_t slot_stride = 0, lv_stride = 0, fin_stride = 0;  // per-beam coefficient tables (0 = shared)
    bool canonical_gravity = false;  // gravity index table is the nearest-neighbour pattern of the plain cantilever
    bool gravity_out_of_band = false;  // a gravity rotation source lies more than one slot from a node its segment loads
                                       // (a PINNED root): dg/dq leaves the block-tridiagonal tangent (crb_static.h)
    uint32_t flags = 0;
    int elem_mode = 0;           // EM_* (crb_generic.h)
    double gx = 0, gy = 0;
    std::vector<int32_t> free_index;  // reduced -> full   (beam 0; every beam of a uniform-topology plan)
    std::vector<int32_t> full2red;    // full -> reduced or -1
    // mixed ensembles (SURVEY f-3): beams that differ in n_elem / boundary conditions / force parameters
    bool mixed_topology = false;      // the beams' free-DOF sets differ: reduced vectors are padded to n_free (the maximum)
    std::vector<int32_t> beam_n_elem, beam_n_free;        // [B] (empty for uniform plans)
    std::vector<std::vector<int32_t>> beam_free_index;    // [B][n_free_b] (empty for uniform plans)
    std::vector<uint8_t> any_free;    // [3 n_node]: DOF free in at least one beam
    size_t free_index_stride = 0;     // d_free_index is [B][n_free] (padded with -1) when != 0
    void* d_gvec = nullptr;           // [B][2] per-beam gravity vector in the plan dtype, or null (shared gx, gy)
    // implicit stepper: cyclic-reduction tables of A = M + alpha K0 for the step size last used (all levels: A is not
    // as diagonally dominant as M, nothing is truncated)
    AsmInputs* asm_in = nullptr;
    mutable void* d_alevels = nullptr;   // [nd][levels_full][S][10]   (the set in use: one of `stiff_sets`)
    mutable void* d_afinal = nullptr;    // [nd][S][6]
    mutable double stiff_alpha = 0.0;    // alpha the tables above were built for (0 = none yet)
    mutable int stiff_levels = 0;        // reduction levels of A that the implicit kernels run (the rest are below roundoff)
    // the table sets of the step sizes used last (a step-size controller alternates between h and h / 2: without this
    // every change would factorise again and synchronise the stream); the oldest set is overwritten
    struct StiffSet { void* lev = nullptr; void* fin = nullptr; double alpha = 0.0; int levels = 0; unsigned long long used = 0; };
    static constexpr int N_STIFF_SETS = 4;
    mutable StiffSet stiff_sets[N_STIFF_SETS];
    mutable unsigned long long stiff_clock = 0;
    // crb_solve_controlled: the table LADDERS of the implicit scheme (A = M + h^2/4 K0 for h = len / 2^r, r < rungs),
    // one per distinct piece length, the most recently used kept; the piece list of the last call
    struct Ladder { double len = 0.0; int rungs = 0; void* lev = nullptr; void* fin = nullptr; unsigned long long used = 0; };
    static constexpr int N_LADDERS = 6;
    mutable Ladder ladders[N_LADDERS];
    mutable void* d_pieces = nullptr;
    mutable size_t pieces_cap = 0;
    // ... and its closed loop with a gain too large for the LDS: the gain transposed, rebuilt by every call (callers overwrite
    // gains in place, so nothing is cached by pointer)
    mutable void* d_gain_t = nullptr;
    mutable size_t gain_t_cap = 0;
    mutable void* d_rhs0 = nullptr;      // [B][2][n_node][4]: the RHS at the start of a crb_step_implicit_damped call (its a_0)
    mutable void* d_tan_x0 = nullptr;    // [B][2][n_node][4]: the base state at the start of a crb_step_rk4_tangent call (n_dir > 1)
    // the adjoint kernels (crb_adjoint.h): the gravity index table of every distinct beam topology and which one each beam
    // uses (empty: one table, topology 0), and their inverse lists on the device, built on first use
    std::vector<std::vector<crb::GravTab>> h_grav_topo;
    std::vector<int32_t> grav_topo_of;
    mutable crb::GravAdj* d_gadj = nullptr;
    mutable int32_t* d_gadj_beam = nullptr;
    // host-vector entry points (crb_rhs_host): full -> reduced map on the device, pinned staging, a stream of the plan's own
    mutable int32_t* d_red_map = nullptr;
    mutable double* h_stage = nullptr;   // pinned + mapped: [2n | n | 2n] doubles (x, u, out)
    mutable double* d_stage = nullptr;   // the device's view of h_stage
    mutable unsigned long long host_seq = 0;   // sequence number of the last flagged host-path launch
    mutable hipStream_t host_stream = nullptr;
    double host_spin_ms = 200.0;      // CRB_HOST_SPIN_MS at plan creation: how long a host-path call spins on the completion flag
    int32_t* d_n_state = nullptr;     // [B] 2 * n_free_b, or null
    std::vector<double> h_levels, h_final, h_norms, h_mass, h_stiff;
    int first_nonlinear = -1;
    std::vector<crb::SlotConst<double>> h_slots;
    std::vector<int> h_kinds;
    // device
    void* d_slot = nullptr;
    void* d_levels = nullptr;
    void* d_final = nullptr;
    // the register-blocked stepper's tables (crb_blocked.h; fp64 uniform 256-slot beams with one table set, else nullptr)
    double* d_blocked = nullptr;
    int blocked_levels = 0;
    bool blocked_twist = false;   // the blocked tables hold the twisted interior's table: the plan runs that instance
    int32_t* d_free_index = nullptr;
    int32_t* d_col_off = nullptr;  // [2n] reduced state index -> offset in a beam's state record
    int32_t* d_row_off = nullptr;  // [n]  reduced position index -> offset in a beam's force record
    // crb_feedback_force_grouped: device tables of the last beam -> group assignment (beam lists, reduced -> layout offsets)
    struct GainGroup { int32_t* beam_idx = nullptr; int32_t* col = nullptr; int32_t* row = nullptr; int n = 0, count = 0; };
    mutable std::vector<GainGroup> gain_groups;
    mutable std::vector<int32_t> gain_group_key;
    mutable int32_t* d_status = nullptr;      // caller's per-beam status words (crb_plan_set_status), or null
    mutable long long status_steps = 0;       // steps the ensemble has taken since the status buffer was set
    mutable bool loop_used = false;   // the last crb_step_rk4_feedback ran the persistent stepper (its work buffer holds a status word)
};

extern "C" int crb_version(void) { return CRB_VERSION; }
extern "C" const char* crb_last_error(void) { return g_err.c_str(); }

namespace {

// a parameter block with every byte zero (padding too)
template <typename P>
P zeroed() { P q; std::memset(&q, 0, sizeof(q)); return q; }
// thread blocks of a launch over the ensemble: G beams each
int beam_groups(const crb_plan* p) { return (p->B + p->G - 1) / p->G; }
// doubles (elements) of the device state [B][2][n_node][4] and of a force-shaped buffer [B][n_node][4]
size_t state_doubles(const crb_plan* p) { return size_t(p->B) * 2 * size_t(p->n_node) * 4; }
size_t force_doubles(const crb_plan* p) { return size_t(p->B) * size_t(p->n_node) * 4; }

void mass_from_blocks(crb_plan* p, const std::vector<NodeBlocks>& blk) {
    const int n = int(p->free_index.size()), S = p->S;   // (beam 0's reduced size; n_free is the ensemble's maximum)
    p->h_mass.assign(size_t(n) * n, 0.0);
    auto put = [&](int fr, int fc, double v) {
        const int r = p->full2red[fr], c = p->full2red[fc];
        if (r >= 0 && c >= 0) p->h_mass[size_t(r) * n + c] += v;
    };
    for (int j = 0; j < S; ++j) {
        const int f0 = 3 * (j + p->off);
        const NodeBlocks& b = blk[j];
        put(f0, f0, b.b_ax);
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 2; ++c) put(f0 + 1 + r, f0 + 1 + c, b.B[2 * r + c]);
        if (j + 1 < S) {
            put(f0, f0 + 3, b.c_ax);
            put(f0 + 3, f0, b.c_ax);
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 2; ++c) {
                    put(f0 + 1 + r, f0 + 4 + c, b.C[2 * r + c]);
                    put(f0 + 4 + c, f0 + 1 + r, b.C[2 * r + c]);
                }
        }
    }
}

int pick_levels(crb_plan* p) {
    // a level whose multipliers are below the unit roundoff of the plan dtype cannot change a
    // result by more than half an ulp: the reduction stops there (exact to rounding)
    const double tol = (p->dtype == CRB_F64) ? std::ldexp(1.0, -53) : std::ldexp(1.0, -24);
    int used = p->levels_full;
    while (used > 0 && p->h_norms[used - 1] < tol) --used;
    p->levels = used;
    return used;
}

// Runs crb_assemble_kernel on the plan's device (one workgroup per described beam) and fills both
// the device tables the steppers load and, for beam 0, the host copies the crb_plan_get_* inspectors
// return.  nd == 1: coefficients shared by all beams of the plan; nd == n_beams: per-beam coefficients.
// Integer topology of one beam inside a plan of n_node nodes (built on the host): free-DOF flags (padding nodes
// beyond the beam's own last node are fully constrained), the reduced <-> full maps and the gravity index table.
struct BeamTopo {
    int n_elem = 0, n_free = 0;
    bool canonical_gravity = false;
    std::vector<uint8_t> free_dof;      // [3 n_node]
    std::vector<int32_t> full2red, free_index;
    std::vector<GravTab> grav;          // [S]
};

template <typename T>
int device_assemble(crb_plan* p, const crb_beam_desc* descs, int nd, const std::vector<SlotConst<double>>& slots,
                    const std::vector<const BeamTopo*>& topo /* [nd] */, bool per_beam_topo) {
    const int S = p->S, ne = p->n_elem, lf = p->levels_full, nn = p->n_node;
    const crb_beam_desc* d = descs;
    p->asm_in = new AsmInputs();
    AsmInputs& in = *p->asm_in;
    DevBuf<double>&dL = in.dL, &dE = in.dE, &dI = in.dI, &dRho = in.dRho, &dA = in.dA, &dWet = in.dWet, &dCd = in.dCd, &dFd = in.dFd;
    DevBuf<uint8_t>&dNl = in.dNl, &dFree = in.dFree;
    DevBuf<GravTab>& dGrav = in.dGrav;
    DevBuf<int32_t>& dNe = in.dNe;
    DevBuf<uint32_t>& dFl = in.dFl;
    DevBuf<double> dFinAll, dNorms, dBlocks, dLv64;
    const int nt = per_beam_topo ? nd : 1;   // beams whose integer topology is uploaded
    std::vector<GravTab> grav(size_t(nt) * S);
    std::vector<uint8_t> free_dof(size_t(nt) * nn * 3);
    for (int b = 0; b < nt; ++b) {
        std::memcpy(&grav[size_t(b) * S], topo[b]->grav.data(), size_t(S) * sizeof(GravTab));
        std::memcpy(&free_dof[size_t(b) * nn * 3], topo[b]->free_dof.data(), size_t(nn) * 3);
    }
    (void)slots;
    bool drag = false;
    for (int b = 0; b < nd; ++b) drag = drag || (descs[b].flags & CRB_FORCE_DRAG);
    // element columns, [nd][n_elem]; a beam shorter than the plan is padded (1.0: never read by an element)
    auto gather = [&](const double* crb_beam_desc::*col) {
        std::vector<double> v(size_t(nd) * ne, 1.0);
        for (int b = 0; b < nd; ++b)
            if (descs[b].*col) std::memcpy(&v[size_t(b) * ne], descs[b].*col, size_t(descs[b].n_elem) * sizeof(double));
        return v;
    };
    std::vector<uint8_t> nl(size_t(nd) * ne, 0);
    for (int b = 0; b < nd; ++b) std::memcpy(&nl[size_t(b) * ne], descs[b].nonlinear, size_t(descs[b].n_elem));
    std::vector<int32_t> ne_b(nd);
    std::vector<uint32_t> fl_b(nd);
    std::vector<double> fd_b(nd);
    for (int b = 0; b < nd; ++b) { ne_b[b] = descs[b].n_elem; fl_b[b] = descs[b].flags; fd_b[b] = descs[b].fluid_density; }
    const auto vL = gather(&crb_beam_desc::length), vE = gather(&crb_beam_desc::elastic_modulus),
               vI = gather(&crb_beam_desc::moment_inertia), vR = gather(&crb_beam_desc::density),
               vA = gather(&crb_beam_desc::cross_area);
    std::vector<double> vW, vC;
    if (drag) { vW = gather(&crb_beam_desc::wetted_area); vC = gather(&crb_beam_desc::drag_coef); }
    if (dL.upload(vL.data(), vL.size()) || dE.upload(vE.data(), vE.size()) || dI.upload(vI.data(), vI.size()) ||
        dRho.upload(vR.data(), vR.size()) || dA.upload(vA.data(), vA.size()) || dNl.upload(nl.data(), nl.size()) ||
        dFree.upload(free_dof.data(), free_dof.size()) || dGrav.upload(grav.data(), grav.size()) ||
        dNe.upload(ne_b.data(), nd) || dFl.upload(fl_b.data(), nd) || dFd.upload(fd_b.data(), nd) ||
        (drag && (dWet.upload(vW.data(), vW.size()) || dCd.upload(vC.data(), vC.size()))) ||
        dFinAll.alloc(size_t(lf + 1) * S * PCR_FINAL_VALS) || dNorms.alloc(lf) || dBlocks.alloc(size_t(S) * 15) ||
        dLv64.alloc(size_t(lf) * S * PCR_LEVEL_VALS))
        return fail(CRB_EHIP, "crb_plan_create: device allocation/upload failed");
    HIP_TRY(hipMalloc(&p->d_slot, size_t(nd) * S * sizeof(SlotConst<T>)));
    HIP_TRY(hipMalloc(&p->d_levels, size_t(nd) * size_t(lf > 0 ? lf : 1) * S * PCR_LEVEL_VALS * sizeof(T)));
    HIP_TRY(hipMalloc(&p->d_final, size_t(nd) * S * PCR_FINAL_VALS * sizeof(T)));
    if (p->mixed_topology) {   // per-beam reduced -> full maps, padded with -1 to the largest beam
        std::vector<int32_t> fi(size_t(nd) * p->n_free, -1), nst(nd);
        for (int b = 0; b < nd; ++b) {
            std::memcpy(&fi[size_t(b) * p->n_free], topo[b]->free_index.data(), topo[b]->free_index.size() * sizeof(int32_t));
            nst[b] = 2 * topo[b]->n_free;
        }
        p->free_index_stride = size_t(p->n_free);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_free_index), fi.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(p->d_free_index, fi.data(), fi.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_n_state), nst.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(p->d_n_state, nst.data(), nst.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    } else {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_free_index), p->free_index.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(p->d_free_index, p->free_index.data(), p->free_index.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    {   // per-beam gravity vectors (only when they differ)
        bool differ = false;
        for (int b = 1; b < nd; ++b) differ = differ || descs[b].gravity[0] != d->gravity[0] || descs[b].gravity[1] != d->gravity[1];
        if (differ) {
            std::vector<T> gv(size_t(nd) * 2);
            for (int b = 0; b < nd; ++b) { gv[2 * b] = T(descs[b].gravity[0]); gv[2 * b + 1] = T(descs[b].gravity[1]); }
            HIP_TRY(hipMalloc(&p->d_gvec, gv.size() * sizeof(T)));
            HIP_TRY(hipMemcpy(p->d_gvec, gv.data(), gv.size() * sizeof(T), hipMemcpyHostToDevice));
        }
    }
    {   // offsets of the reduced ordering inside the device layouts (crb_feedback_force)
        const int n = p->n_free;
        std::vector<int32_t> col(size_t(2) * n), row(n);
        for (int r = 0; r < n; ++r) {
            const int f = r < int(p->free_index.size()) ? p->free_index[r] : 0;   // (mixed plans: beam 0 may be shorter)
            row[r] = (f / 3) * 4 + (f % 3);
            col[r] = row[r];
            col[n + r] = p->n_node * 4 + row[r];
        }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_col_off), col.size() * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_row_off), row.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(p->d_col_off, col.data(), col.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p->d_row_off, row.data(), row.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (nd > 1) {
        p->slot_stride = size_t(S);
        p->lv_stride = size_t(lf) * S * PCR_LEVEL_VALS;
        p->fin_stride = size_t(S) * PCR_FINAL_VALS;
    }

    AsmParams a = zeroed<AsmParams>();
    a.L = dL.p; a.E = dE.p; a.I = dI.p; a.rho = dRho.p; a.A = dA.p;
    a.nonlinear = dNl.p; a.free_dof = dFree.p; a.wet = dWet.p; a.cd = dCd.p; a.grav = dGrav.p;
    a.fluid_density = d->fluid_density; a.flags = d->flags;
    a.n_elem = ne; a.n_node = p->n_node; a.off = p->off; a.S = S; a.levels_full = lf;
    if (nd > 1) { a.n_elem_b = dNe.p; a.fluid_density_b = dFd.p; a.flags_b = dFl.p; }
    a.free_stride = per_beam_topo ? size_t(nn) * 3 : 0;
    a.grav_stride = per_beam_topo ? size_t(S) : 0;
    a.slot_out = p->d_slot; a.lv64 = dLv64.p; a.lvT = p->d_levels; a.fin64_all = dFinAll.p; a.norms = dNorms.p;
    a.blocks0 = dBlocks.p; a.finT = nullptr; a.fin_level = -1;
    a.elem_stride = nd > 1 ? size_t(ne) : 0;
    const int nta = (S + 63) / 64 * 64;
    const size_t smem = size_t(S) * sizeof(NodeBlocks);
    HIP_TRY(lds_opt_in(crb_assemble_kernel<T>, smem));
    // pass 1: constants, multipliers of every level, their norms (max over beams)
    HIP_TRY(hipMemset(dNorms.p, 0, size_t(lf ? lf : 1) * sizeof(double)));
    hipLaunchKernelGGL((crb_assemble_kernel<T>), dim3(nd), dim3(nta), smem, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    p->h_levels.assign(size_t(lf > 0 ? lf : 1) * S * PCR_LEVEL_VALS, 0.0);
    p->h_norms.assign(size_t(lf > 0 ? lf : 1), 0.0);
    if (lf > 0) {
        HIP_TRY(hipMemcpy(p->h_levels.data(), dLv64.p, size_t(lf) * S * PCR_LEVEL_VALS * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(p->h_norms.data(), dNorms.p, size_t(lf) * sizeof(double), hipMemcpyDeviceToHost));
    }
    const int used = pick_levels(p);
    if (used > MAX_LV)
        return fail(CRB_EUNSUPPORTED, "mass matrix needs more cyclic-reduction levels than the kernels carry in registers");
    in.a = a; in.nd = nd; in.threads = nta; in.smem = smem;   // (kept for the implicit stepper's factorisations)
    // pass 2: the final inverses after `used` levels, straight into the steppers' table
    a.finT = p->d_final; a.fin_level = used; a.lv64 = nullptr; a.blocks0 = nullptr; a.fin64_all = nullptr;
    hipLaunchKernelGGL((crb_assemble_kernel<T>), dim3(nd), dim3(nta), smem, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());

    // ---- inspection copies (beam 0)
    p->h_final.assign(size_t(S) * PCR_FINAL_VALS, 0.0);
    HIP_TRY(hipMemcpy(p->h_final.data(), dFinAll.p + size_t(used) * S * PCR_FINAL_VALS,
                      size_t(S) * PCR_FINAL_VALS * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> b0(size_t(S) * 15);
    HIP_TRY(hipMemcpy(b0.data(), dBlocks.p, b0.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<NodeBlocks> blk(S);
    for (int j = 0; j < S; ++j) {
        const double* b = &b0[size_t(j) * 15];
        blk[j].a_ax = b[0]; blk[j].b_ax = b[1]; blk[j].c_ax = b[2];
        for (int k = 0; k < 4; ++k) { blk[j].A[k] = b[3 + k]; blk[j].B[k] = b[7 + k]; blk[j].C[k] = b[11 + k]; }
    }
    mass_from_blocks(p, blk);
    std::vector<SlotConst<T>> hs(S);
    HIP_TRY(hipMemcpy(hs.data(), p->d_slot, size_t(S) * sizeof(SlotConst<T>), hipMemcpyDeviceToHost));
    p->h_slots.assign(S, SlotConst<double>());
    p->h_kinds.assign(S, KIND_NONE);
    for (int j = 0; j < S; ++j) {
        SlotConst<double>& o = p->h_slots[j];
        std::memset(&o, 0, sizeof(o));
        o.drag = double(hs[j].drag);
        o.half_mass = double(hs[j].half_mass);
        for (int c = 0; c < 3; ++c) o.mask[c] = double(hs[j].mask[c]);
        o.grav = hs[j].grav;
        p->h_kinds[j] = hs[j].elem.kind;
    }
    if constexpr (sizeof(T) == 8) {
        // the register-blocked stepper (crb_lean.h, NPL = 4): one table set, 256 slots of equal constants, every DOF free, and
        // a mass matrix whose lane interiors are bitwise equal (crb_blocked.h: blocked_factor)
        bool uniform = nd == 1 && S == BLK_S && p->G == 1;
        for (int j = 0; uniform && j < S; ++j)
            uniform = std::memcmp(&hs[j].elem, &hs[0].elem, sizeof(hs[0].elem)) == 0 &&
                      std::memcmp(&hs[j].drag, &hs[0].drag, sizeof(T)) == 0 && hs[j].mask[0] == T(1) && hs[j].mask[1] == T(1) &&
                      hs[j].mask[2] == T(1);
        if (uniform) {
            // (CRB_BLK_TWIST: the twisted interior's table behind them, for node blocks that have the mirror structure it needs
            //  bitwise; the others -- the device assembly contracts B's off-diagonal differences into fused multiply-adds, which
            //  leave a rounding residue at some element lengths -- run the block-Thomas instance)
            std::vector<double> tab(size_t(blk_twist_offset(BLK_MAX_LV)) + BT_TAB);
            double norms[BLK_MAX_LV], tw[BT_TAB];
            //  (nonlinear elements: the linear instance is not built in that form)
            const bool twist_ok = CRB_BLK_TWIST && hs[0].elem.kind == KIND_NONLINEAR && blocked_mirrored(blk.data());
            bool twist = twist_ok;
            int lv = blocked_factor(blk.data(), d->length[0], tab.data(), tab.data() + BU_N, norms, twist ? tw : nullptr);
            if (lv < 0 && twist) {   // (the twisted constants differ between lanes: the block-Thomas instance, if its own do not)
                twist = false;
                lv = blocked_factor(blk.data(), d->length[0], tab.data(), tab.data() + BU_N, norms);
            }
            if (lv >= 1) {
                // nonlinear elements: the force polynomials' folded constants behind the tables (crb_math.h: elem_fold_build),
                // and behind those the constants of the form that shares the membrane combinations (elem_share_build)
                const bool fold = hs[0].elem.kind == KIND_NONLINEAR;
                size_t n = fold ? size_t(blk_share_offset(lv)) + SK_N : size_t(blk_fold_offset(lv));
                if (twist) {
                    n = size_t(blk_twist_offset(lv)) + BT_TAB;
                    std::memcpy(tab.data() + blk_twist_offset(lv), tw, sizeof(tw));
                }
                if (fold) {
                    ElemCoef<double> ecd;
                    for (int i = 0; i < 6; ++i) ecd.c[i] = double(hs[0].elem.c[i]);
                    elem_fold_build(ecd, tab.data() + blk_fold_offset(lv));
                    elem_share_build(ecd, tab.data() + blk_share_offset(lv));
                }
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_blocked), n * sizeof(double)));
                HIP_TRY(hipMemcpy(p->d_blocked, tab.data(), n * sizeof(double), hipMemcpyHostToDevice));
                p->blocked_levels = lv;
                p->blocked_twist = twist;
            }
        }
    }
    return CRB_OK;
}

}  // namespace

static int plan_create_impl(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* d, int nd);

extern "C" int crb_plan_create(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* d) {
    return plan_create_impl(out, device, dtype, n_beams, d, 1);
}

extern "C" int crb_plan_create_ensemble(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* descs) {
    if (!out || !descs) return fail(CRB_EINVAL, "crb_plan_create_ensemble: null argument");
    if (n_beams < 1) return fail(CRB_EINVAL, "n_beams must be >= 1");
    if (device < 0) return fail(CRB_EUNSUPPORTED, "per-beam coefficient plans are built on the device (no host-only form)");
    const crb_beam_desc& a = descs[0];
    for (int b = 1; b < n_beams; ++b)   // the one thing an ensemble must share: the element variant compiled into the kernels
        if ((descs[b].flags & CRB_CORRECTED_AXIAL) != (a.flags & CRB_CORRECTED_AXIAL))
            return fail(CRB_EINVAL, "ensemble beams must share the CRB_CORRECTED_AXIAL option");
    return plan_create_impl(out, device, dtype, n_beams, descs, n_beams);
}

namespace {
// CSV-row validation of one beam: Properties.__post_init__ / EulerBernoulliBeam._validate_parameters
// (abstractions.py:39-53, euler_bernoulli_beam.py:100-103), ForceParams / FluidDragForce (force_params.py:41-43,
// fluid_forces.py:59-72).  Returns nullptr or the reference's message.
const char* validate_desc(const crb_beam_desc& o) {
    if (o.n_elem < 1) return "n_elem must be >= 1";
    if (!o.length || !o.elastic_modulus || !o.moment_inertia || !o.density || !o.cross_area || !o.nonlinear || !o.node_bc)
        return "beam description has null columns";
    for (int e = 0; e < o.n_elem; ++e) {
        if (!(o.length[e] > 0) || !(o.elastic_modulus[e] > 0) || !(o.moment_inertia[e] > 0) || !(o.density[e] > 0) ||
            !(o.cross_area[e] > 0))
            return "All numeric parameters must be positive";
        if (o.nonlinear[e] > 1) return "Invalid element type";
    }
    for (int i = 0; i <= o.n_elem; ++i)
        if (o.node_bc[i] != CRB_BC_NONE && o.node_bc[i] != CRB_BC_FIXED && o.node_bc[i] != CRB_BC_PINNED)
            return "Unsupported boundary condition type";
    if (o.flags & CRB_FORCE_DRAG) {
        if (!o.wetted_area || !o.drag_coef) return "drag enabled but wetted_area/drag_coef missing";
        if (!(o.fluid_density > 0)) return "fluid_density must be positive when fluid effects are enabled";
        for (int e = 0; e < o.n_elem; ++e) {
            if (o.drag_coef[e] < 0) return "Drag coefficients cannot be negative";
            if (o.wetted_area[e] < 0) return "Wetted areas cannot be negative";
        }
    }
    return nullptr;
}

// Integer topology of a beam of d.n_elem elements inside a plan of nn nodes whose first `off` nodes carry no slot:
// boundary conditions -> free masks and the reduced ordering (euler_bernoulli_beam.py:240-259); the gravity index
// table with the reference's reduced-index addressing (gravity_forces.py:97-146).
BeamTopo build_topology(const crb_beam_desc& d, int nn, int off) {
    BeamTopo t;
    const int ne = d.n_elem, S = nn - off;
    t.n_elem = ne;
    t.free_dof.assign(size_t(nn) * 3, 0);    // nodes past the beam's own last node (index ne) stay fully constrained
    for (int i = 0; i <= ne; ++i) {
        const int bc = d.node_bc[i];
        const bool fx = bc == CRB_BC_FIXED, pin = bc == CRB_BC_PINNED;
        t.free_dof[3 * i] = t.free_dof[3 * i + 1] = (fx || pin) ? 0 : 1;
        t.free_dof[3 * i + 2] = fx ? 0 : 1;
    }
    t.full2red.assign(size_t(nn) * 3, -1);
    for (int f = 0; f < 3 * nn; ++f)
        if (t.free_dof[f]) { t.full2red[f] = int32_t(t.free_index.size()); t.free_index.push_back(f); }
    t.n_free = int(t.free_index.size());
    const int n = t.n_free;
    t.grav.resize(S);
    const bool grav = d.flags & CRB_FORCE_GRAVITY;
    for (int j = 0; j < S; ++j) {
        GravTab& gt = t.grav[j];
        gt.phiA = gt.phiB = -1;
        for (int c = 0; c < 3; ++c) { gt.segA[c] = gt.segB[c] = -1; gt.comp[c] = 0; }
        gt.pad = 0;
        if (!grav) continue;
        const int node = j + off;
        auto enc = [&](int red) -> int16_t {
            const int f = t.free_index[red];
            return int16_t(((f / 3) - off) * 4 + (f % 3));
        };
        if (j < ne) {  // this thread evaluates segment j (gravity_forces.py:97-128)
            const int sp = 3 * j + 2, ep = 3 * (j + 1) + 2;  // indices into the REDUCED vector
            if (sp < n) gt.phiA = enc(sp);
            if (ep < n) gt.phiB = enc(ep);
        }
        for (int c = 0; c < 3; ++c) {  // which segments add to this DOF (gravity_forces.py:130-146)
            const int r = t.full2red[3 * node + c];
            if (r < 0 || r % 3 == 2) continue;
            gt.comp[c] = int8_t(r % 3);
            if (r / 3 < ne) gt.segA[c] = int16_t(r / 3);
            if (r / 3 - 1 >= 0) gt.segB[c] = int16_t(r / 3 - 1);
        }
    }
    // does the gravity table reduce to "segment j <-> slots j, j+1" (the plain cantilever filling the whole plan)?
    t.canonical_gravity = false;
    if (grav && off == 1 && ne == S) {
        bool canon = true;
        for (int j = 0; j < S && canon; ++j) {
            const GravTab& gt = t.grav[j];
            canon = gt.phiA == int16_t(j * 4 + 2) && gt.phiB == (j + 1 < S ? int16_t((j + 1) * 4 + 2) : int16_t(-1)) &&
                    gt.segA[2] < 0 && gt.segB[2] < 0;
            for (int c = 0; c < 2 && canon; ++c)
                canon = gt.comp[c] == c && gt.segA[c] == int16_t(j) && gt.segB[c] == int16_t(j - 1 >= 0 ? j - 1 : -1);
        }
        t.canonical_gravity = canon;
    }
    return t;
}
}  // namespace

static int plan_create_impl(crb_plan** out, int device, int dtype, int n_beams, const crb_beam_desc* d, int nd) {
    if (!out || !d) return fail(CRB_EINVAL, "crb_plan_create: null argument");
    *out = nullptr;
    if (dtype != CRB_F64 && dtype != CRB_F32) return fail(CRB_EINVAL, "dtype must be CRB_F64 or CRB_F32");
    if (n_beams < 1) return fail(CRB_EINVAL, "n_beams must be >= 1");
    for (int b = 0; b < nd; ++b)
        if (const char* msg = validate_desc(d[b])) return fail(CRB_EINVAL, msg);
    // the plan's node count is the longest beam's; shorter beams end in padding nodes (fully constrained, no element)
    int ne = 0;
    bool all_fixed_root = true, any_drag = false, any_grav = false;
    for (int b = 0; b < nd; ++b) {
        ne = d[b].n_elem > ne ? d[b].n_elem : ne;
        all_fixed_root = all_fixed_root && d[b].node_bc[0] == CRB_BC_FIXED;
        any_drag = any_drag || (d[b].flags & CRB_FORCE_DRAG);
        any_grav = any_grav || (d[b].flags & CRB_FORCE_GRAVITY);
    }
    const bool grav = any_grav;

    crb_plan* p = new crb_plan();
    p->device = device;
    if (const char* v = env("CRB_HOST_SPIN_MS")) p->host_spin_ms = std::atof(v);
    p->dtype = dtype;
    p->B = n_beams;
    p->n_elem = ne;
    p->n_node = ne + 1;
    // force terms compiled into a launch = the union over the beams; a beam without drag / gravity has zero drag
    // factors / zero segment masses in its slot table
    p->flags = (d->flags & CRB_CORRECTED_AXIAL) | (any_drag ? CRB_FORCE_DRAG : 0u) | (any_grav ? CRB_FORCE_GRAVITY : 0u);
    p->gx = d->gravity[0];
    p->gy = d->gravity[1];
    const int nn = p->n_node;
    // node 0 carries no thread slot when it is FIXED in every beam (the cantilever of the examples)
    p->off = all_fixed_root ? 1 : 0;
    p->S = nn - p->off;
    const int S = p->S;
    if (S > 1024) { delete p; return fail(CRB_EUNSUPPORTED, "more than 1024 thread-carried nodes per beam"); }

    // ---- integer topology per DISTINCT (n_elem, boundary conditions, gravity on/off) among the beams
    std::vector<BeamTopo> topos;
    std::vector<int> topo_of(nd, 0);
    for (int b = 0; b < nd; ++b) {
        int hit = -1;
        for (int c = 0; c < b && hit < 0; ++c)
            if (d[c].n_elem == d[b].n_elem && std::memcmp(d[c].node_bc, d[b].node_bc, size_t(d[b].n_elem) + 1) == 0 &&
                ((d[c].flags ^ d[b].flags) & CRB_FORCE_GRAVITY) == 0)
                hit = topo_of[c];
        if (hit < 0) { topos.push_back(build_topology(d[b], nn, p->off)); hit = int(topos.size()) - 1; }
        topo_of[b] = hit;
    }
    std::vector<const BeamTopo*> topo(nd);
    for (int b = 0; b < nd; ++b) topo[b] = &topos[topo_of[b]];
    const BeamTopo& t0 = *topo[0];
    for (const BeamTopo& t : topos) p->h_grav_topo.push_back(t.grav);
    for (const BeamTopo& t : topos)   // (tables of gravity-free topologies are empty of entries)
        for (int j = 0; j < S; ++j)
            for (int c = 0; c < 3; ++c)
                for (const int sg : {int(t.grav[j].segA[c]), int(t.grav[j].segB[c])}) {
                    if (sg < 0 || sg >= S) continue;
                    for (const int src : {int(t.grav[sg].phiA), int(t.grav[sg].phiB)})
                        if (src >= 0 && std::abs((src >> 2) - j) > 1) p->gravity_out_of_band = true;
                }
    if (topos.size() > 1) p->grav_topo_of = topo_of;
    p->free_index = t0.free_index;
    p->full2red = t0.full2red;
    p->n_free = t0.n_free;
    p->any_free = t0.free_dof;
    bool per_beam_topo = topos.size() > 1;
    for (int b = 1; b < nd; ++b) {
        if (topo[b]->free_dof != t0.free_dof) p->mixed_topology = true;
        if (topo[b]->n_free > p->n_free) p->n_free = topo[b]->n_free;
        for (size_t f = 0; f < p->any_free.size(); ++f) p->any_free[f] = p->any_free[f] | topo[b]->free_dof[f];
    }
    // per-beam sizes whenever they differ -- also when the free-DOF sets agree (a longer beam whose extra nodes are all FIXED
    // has the shorter beam's masks: its element count, and with it the tip node, is still its own)
    bool sizes_differ = p->mixed_topology;
    for (int b = 1; b < nd; ++b) sizes_differ = sizes_differ || topo[b]->n_elem != t0.n_elem;
    if (sizes_differ) {
        p->beam_n_elem.resize(nd); p->beam_n_free.resize(nd); p->beam_free_index.resize(nd);
        for (int b = 0; b < nd; ++b) {
            p->beam_n_elem[b] = topo[b]->n_elem; p->beam_n_free[b] = topo[b]->n_free; p->beam_free_index[b] = topo[b]->free_index;
        }
    }
    for (int b = 0; b < nd; ++b)
        if (topo[b]->n_free == 0) { delete p; return fail(CRB_EINVAL, "Cannot constrain all degrees of freedom"); }

    // S >= 64: one beam per workgroup of NW = 2^lognw wavefronts (slots interleaved over the waves);
    // S < 64: G = 64/S whole beams per single-wave workgroup
    p->lognw = 0;
    if (S >= 64) {
        p->G = 1;
        while ((64 << p->lognw) < S) ++p->lognw;
        p->NT = 64 << p->lognw;
    } else {
        p->G = 64 / S;
        p->NT = 64;
    }
    int lf = 0;
    while ((1 << lf) < S) ++lf;
    p->levels_full = lf;

    // ---- per-slot constants of beam 0 (host copies for the inspectors; the device tables come from crb_assemble_kernel)
    std::vector<SlotConst<double>> slots(S);
    std::vector<int> kinds(S, KIND_NONE);
    const bool drag = d->flags & CRB_FORCE_DRAG;
    for (int j = 0; j < S; ++j) {
        SlotConst<double>& s = slots[j];
        std::memset(&s, 0, sizeof(s));
        const int node = j + p->off;
        const int e = node - 1;
        if (e >= 0 && e < d->n_elem) kinds[j] = d->nonlinear[e] ? KIND_NONLINEAR : KIND_LINEAR;
        for (int c = 0; c < 3; ++c) s.mask[c] = t0.free_dof[3 * node + c] ? 1.0 : 0.0;
        if (drag && t0.free_dof[3 * node + 1]) {
            // fluid_forces.py:59-61, 87-90: the node's own segment row, last row repeated for the tip
            const int row = node < d->n_elem ? node : d->n_elem - 1;
            s.drag = 0.5 * d->fluid_density * d->drag_coef[row] * d->wetted_area[row];
        }
        s.grav = t0.grav[j];
        if ((d->flags & CRB_FORCE_GRAVITY) && j < d->n_elem) s.half_mass = 0.5 * (d->density[j] * d->cross_area[j] * d->length[j]);
    }
    p->h_slots = slots;
    p->h_kinds = kinds;
    {   // one element kind over the whole ensemble?
        bool all_nl = true, all_lin = true;
        for (int b = 0; b < nd; ++b)
            for (int e = 0; e < d[b].n_elem; ++e) { all_nl = all_nl && d[b].nonlinear[e]; all_lin = all_lin && !d[b].nonlinear[e]; }
        p->elem_mode = all_lin ? EM_LINEAR : (all_nl && !(d->flags & CRB_CORRECTED_AXIAL)) ? EM_NONLINEAR : EM_MIXED;
    }
    if (grav) {   // nearest-neighbour gravity (lean kernels) only if EVERY beam that has gravity is the canonical cantilever
        bool canon = true;
        for (int b = 0; b < nd; ++b)
            if (d[b].flags & CRB_FORCE_GRAVITY) canon = canon && topo[b]->canonical_gravity;
            else canon = canon && d[b].n_elem == S && p->off == 1;   // (a gravity-free beam only needs the same slot layout)
        p->canonical_gravity = canon;
    }

    const int n = t0.n_free;
    {   // dense reduced stiffness of beam 0's linear elements (get_stiffness_matrix); columns = K_e * unit vectors
        p->h_stiff.assign(size_t(n) * n, 0.0);
        for (int e = 0; e < d->n_elem; ++e) {
            if (d->nonlinear[e]) { if (p->first_nonlinear < 0) p->first_nonlinear = e; continue; }
            ElemCoef<double> ec;
            elem_coef_build<double>(ec, KIND_LINEAR, d->length[e], d->elastic_modulus[e], d->moment_inertia[e],
                                    d->cross_area[e]);
            for (int col = 0; col < 6; ++col) {
                double xe[6] = {0, 0, 0, 0, 0, 0}, fl[3], fr[3];
                xe[col] = 1.0;
                elem_force_linear<double>(ec.c, xe, xe + 3, fl, fr);
                const int rc = p->full2red[3 * e + col];
                if (rc < 0) continue;
                for (int row = 0; row < 6; ++row) {
                    const int rr = p->full2red[3 * e + row];
                    if (rr >= 0) p->h_stiff[size_t(rr) * n + rc] += row < 3 ? fl[row] : fr[row - 3];
                }
            }
        }
    }
    if (device < 0) {
    // ======== host-only plan (inspection, one shared beam): same arithmetic (crb_math.h) in plain C++ ========
    const std::vector<uint8_t>& free_dof = t0.free_dof;
    // ---- mass matrix in node-block form + cyclic-reduction factorisation (all fp64)
    std::vector<NodeBlocks> cur(S), nxt(S);
    auto fm = [&](int node, int c) { return node >= 0 && node < nn && free_dof[3 * node + c] != 0; };
    for (int j = 0; j < S; ++j) {
        NodeBlocks nb = zeroed<NodeBlocks>();
        const int node = j + p->off;
        const int el = node - 1, er = node;
        if (el >= 0) mass_add_as_left_elem(nb, d->length[el], d->density[el] * d->cross_area[el], j >= 1);
        if (er < ne) mass_add_as_right_elem(nb, d->length[er], d->density[er] * d->cross_area[er]);
        const bool hl = j >= 1, hr = j + 1 < S;
        mass_apply_masks(nb, fm(node, 0), fm(node, 1), fm(node, 2), hl && fm(node - 1, 0), hl && fm(node - 1, 1),
                         hl && fm(node - 1, 2), hr && fm(node + 1, 0), hr && fm(node + 1, 1), hr && fm(node + 1, 2));
        cur[j] = nb;
    }
    mass_from_blocks(p, cur);
    std::vector<std::vector<NodeBlocks>> states;
    states.push_back(cur);
    p->h_levels.assign(size_t(lf > 0 ? lf : 1) * S * PCR_LEVEL_VALS, 0.0);
    p->h_norms.assign(size_t(lf > 0 ? lf : 1), 0.0);
    for (int l = 0; l < lf; ++l) {
        const int s = 1 << l;
        double nm = 0.0;
        for (int j = 0; j < S; ++j) {
            PcrLevel lv;
            const bool hl = j - s >= 0, hh = j + s < S;
            pcr_factor_level(cur[j], cur[hl ? j - s : j], hl, cur[hh ? j + s : j], hh, lv, nxt[j]);
            double* o = &p->h_levels[(size_t(l) * S + j) * PCR_LEVEL_VALS];
            o[0] = lv.al_ax;
            o[1] = lv.ga_ax;
            for (int k = 0; k < 4; ++k) { o[2 + k] = lv.al[k]; o[6 + k] = lv.ga[k]; }
            const int node = j + p->off;
            const int el = node - 1 >= 0 ? node - 1 : 0;
            const double nj = pcr_level_norm(lv, d->length[el < ne ? el : ne - 1]);
            nm = nj > nm ? nj : nm;
        }
        p->h_norms[l] = nm;
        cur.swap(nxt);
        states.push_back(cur);
    }
    const int used = pick_levels(p);
    if (used > MAX_LV) {
        delete p;
        return fail(CRB_EUNSUPPORTED, "mass matrix needs more cyclic-reduction levels than the kernels carry in registers");
    }
    p->h_final.assign(size_t(S) * PCR_FINAL_VALS, 0.0);
    for (int j = 0; j < S; ++j) {
        const NodeBlocks& b = states[used][j];
        double Bi[4];
        inv2(b.B, Bi);
        double* o = &p->h_final[size_t(j) * PCR_FINAL_VALS];
        // constrained DOFs: zero row/column in the final inverse, so the kernels need no mask multiply
        const double mu = slots[j].mask[0], mw = slots[j].mask[1], mp = slots[j].mask[2];
        o[0] = mu / b.b_ax;
        o[1] = mw * mw * Bi[0];
        o[2] = mw * mp * Bi[1];
        o[3] = mp * mw * Bi[2];
        o[4] = mp * mp * Bi[3];
        o[5] = 0.0;
    }

    }
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
            delete p;
            return fail(CRB_ENODEV, "crb_plan_create: HIP device not available (no fallback path exists)");
        }
        // plan creation works on the plan's device and hands the caller's current device back (launch entry points
        // select the plan's device and leave it selected, as a HIP stream of that device must be current anyway)
        int prev = -1;
        (void)hipGetDevice(&prev);
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { delete p; return fail(CRB_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); }
        // ======== device plan: crb_assemble_kernel builds every floating-point table ========
        const int rc = (dtype == CRB_F64) ? device_assemble<double>(p, d, nd, slots, topo, per_beam_topo)
                                          : device_assemble<float>(p, d, nd, slots, topo, per_beam_topo);
        if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
        if (rc != CRB_OK) { crb_plan_destroy(p); return rc; }
    }
    *out = p;
    return CRB_OK;
}

namespace {
void free_gain_groups(const crb_plan* p);
}
extern "C" void crb_plan_destroy(crb_plan* p) {
    if (!p) return;
    if (p->device >= 0) {
        (void)hipFree(p->d_slot);
        (void)hipFree(p->d_levels);
        (void)hipFree(p->d_final);
        (void)hipFree(p->d_blocked);
        (void)hipFree(p->d_free_index);
        free_gain_groups(p);
        (void)hipFree(p->d_col_off);
        (void)hipFree(p->d_row_off);
        (void)hipFree(p->d_gvec);
        (void)hipFree(p->d_n_state);
        for (auto& set : p->stiff_sets) { (void)hipFree(set.lev); (void)hipFree(set.fin); }
        for (auto& lad : p->ladders) { (void)hipFree(lad.lev); (void)hipFree(lad.fin); }
        (void)hipFree(p->d_pieces);
        (void)hipFree(p->d_gain_t);
        (void)hipFree(p->d_rhs0);
        (void)hipFree(p->d_tan_x0);
        (void)hipFree(p->d_gadj);
        (void)hipFree(p->d_gadj_beam);
        (void)hipFree(p->d_red_map);
        if (p->h_stage) (void)hipHostFree(p->h_stage);
        if (p->host_stream) (void)hipStreamDestroy(p->host_stream);
        delete p->asm_in;
    }
    delete p;
}

extern "C" int crb_plan_set_status(const crb_plan* p, void* status, long long steps_done) {
    if (!p) return fail(CRB_EINVAL, "crb_plan_set_status: null plan");
    if (steps_done < 0) return fail(CRB_EINVAL, "crb_plan_set_status: steps_done must be >= 0");
    p->d_status = static_cast<int32_t*>(status);
    p->status_steps = steps_done;
    return CRB_OK;
}

extern "C" long long crb_plan_status_steps(const crb_plan* p) { return p ? p->status_steps : -1; }

extern "C" int crb_plan_get_layout(const crb_plan* p, crb_layout* o) {
    if (!p || !o) return fail(CRB_EINVAL, "null argument");
    o->dtype = p->dtype;
    o->n_beams = p->B;
    o->n_elem = p->n_elem;
    o->n_node = p->n_node;
    o->n_free = p->n_free;
    o->node_offset = p->off;
    o->n_slots = p->S;
    o->beams_per_group = p->G;
    o->threads = p->NT;
    o->pcr_levels = p->levels;
    o->pcr_levels_full = p->levels_full;
    o->mixed_topology = p->mixed_topology ? 1 : 0;
    return CRB_OK;
}

extern "C" int crb_plan_get_free_index(const crb_plan* p, int32_t* out) {
    if (!p || !out) return fail(CRB_EINVAL, "null argument");
    std::memcpy(out, p->free_index.data(), p->free_index.size() * sizeof(int32_t));
    return CRB_OK;
}

extern "C" int crb_plan_get_beam_info(const crb_plan* p, int beam, int32_t* n_elem, int32_t* n_free) {
    if (!p) return fail(CRB_EINVAL, "null argument");
    if (beam < 0 || beam >= p->B) return fail(CRB_EINVAL, "crb_plan_get_beam_info: beam out of range");
    const bool per_beam = !p->beam_n_elem.empty();
    if (n_elem) *n_elem = per_beam ? p->beam_n_elem[beam] : p->n_elem;
    if (n_free) *n_free = per_beam ? p->beam_n_free[beam] : int32_t(p->free_index.size());
    return CRB_OK;
}

extern "C" int crb_plan_get_beam_free_index(const crb_plan* p, int beam, int32_t* out) {
    if (!p || !out) return fail(CRB_EINVAL, "null argument");
    if (beam < 0 || beam >= p->B) return fail(CRB_EINVAL, "crb_plan_get_beam_free_index: beam out of range");
    const std::vector<int32_t>& fi = !p->beam_free_index.empty() ? p->beam_free_index[beam] : p->free_index;
    std::memcpy(out, fi.data(), fi.size() * sizeof(int32_t));
    return CRB_OK;
}

// Host restatement of the register-blocked stepper's mass solve (crb_blocked.h), for the test suite: blocks = the 256 node rows
// of M as [a_ax, b_ax, c_ax, A[4], B[4], C[4]], Lc the length that scales rotations in the level norms.  x = M^-1 r ([256][3]),
// *levels the separator levels the solve keeps, norms[6] every separator level's largest multiplier.
namespace {
int blocked_solve_host_impl(const char* who, bool twist, const double* blocks, double Lc, const double* r, double* x, int32_t* levels,
                            double* norms) {
    if (!blocks || !r || !x) return fail(CRB_EINVAL, std::string(who) + ": null argument");
    std::vector<NodeBlocks> blk(BLK_S);
    for (int j = 0; j < BLK_S; ++j) {
        const double* b = blocks + size_t(j) * 15;
        blk[j].a_ax = b[0]; blk[j].b_ax = b[1]; blk[j].c_ax = b[2];
        for (int k = 0; k < 4; ++k) { blk[j].A[k] = b[3 + k]; blk[j].B[k] = b[7 + k]; blk[j].C[k] = b[11 + k]; }
    }
    std::vector<double> tab(BU_N + size_t(blk_sep_vals(BLK_MAX_LV)) * BLK_LANES);
    double nrm[BLK_MAX_LV], tw[BT_TAB];
    const bool mirrored = !twist || blocked_mirrored(blk.data());
    const int lv = blocked_factor(blk.data(), Lc, tab.data(), tab.data() + BU_N, nrm, twist && mirrored ? tw : nullptr);
    if (lv >= 0 && !mirrored)
        return fail(CRB_EUNSUPPORTED, std::string(who) + ": the lane interiors of this mass matrix lack the mirror structure of equal elements");
    if (lv < 0) return fail(CRB_EUNSUPPORTED, std::string(who) + ": the lane interiors of this mass matrix are not uniform");
    blocked_solve_host(tab.data(), tab.data() + BU_N, lv, r, x, twist ? tw : nullptr);
    if (levels) *levels = lv;
    if (norms) std::memcpy(norms, nrm, sizeof(nrm));
    return CRB_OK;
}
}  // namespace
extern "C" int crb_blocked_solve_host(const double* blocks, double Lc, const double* r, double* x, int32_t* levels, double* norms) {
    return blocked_solve_host_impl("crb_blocked_solve_host", false, blocks, Lc, r, x, levels, norms);
}
// ... with the interiors solved about their centre nodes, as the blocked stepper does (CRB_BLK_TWIST)
extern "C" int crb_blocked_twist_solve_host(const double* blocks, double Lc, const double* r, double* x, int32_t* levels, double* norms) {
    return blocked_solve_host_impl("crb_blocked_twist_solve_host", true, blocks, Lc, r, x, levels, norms);
}

extern "C" int crb_plan_get_blocked_form(const crb_plan* p, int32_t* form, int32_t* levels) {
    if (!p) return fail(CRB_EINVAL, "null argument");
    if (form) *form = !p->d_blocked ? 0 : (p->blocked_twist ? 2 : 1);
    if (levels) *levels = p->d_blocked ? p->blocked_levels : 0;
    return CRB_OK;
}

extern "C" int crb_plan_get_pcr_tables(const crb_plan* p, double* levels, double* final_, double* norms) {
    if (!p) return fail(CRB_EINVAL, "null argument");
    const size_t S = size_t(p->S);
    if (levels) std::memcpy(levels, p->h_levels.data(), size_t(p->levels_full) * S * PCR_LEVEL_VALS * sizeof(double));
    if (final_) std::memcpy(final_, p->h_final.data(), S * PCR_FINAL_VALS * sizeof(double));
    if (norms) std::memcpy(norms, p->h_norms.data(), size_t(p->levels_full) * sizeof(double));
    return CRB_OK;
}

extern "C" int crb_plan_get_slot_tables(const crb_plan* p, double* drag, double* half_mass, double* mask, int16_t* grav,
                                        int32_t* elem_kind) {
    if (!p) return fail(CRB_EINVAL, "null argument");
    for (int j = 0; j < p->S; ++j) {
        const SlotConst<double>& s = p->h_slots[j];
        if (drag) drag[j] = s.drag;
        if (half_mass) half_mass[j] = s.half_mass;
        if (mask) for (int c = 0; c < 3; ++c) mask[3 * j + c] = s.mask[c];
        if (grav) {
            int16_t* g = grav + 12 * j;
            g[0] = s.grav.phiA;
            g[1] = s.grav.phiB;
            for (int c = 0; c < 3; ++c) { g[2 + c] = s.grav.segA[c]; g[5 + c] = s.grav.segB[c]; g[8 + c] = s.grav.comp[c]; }
            g[11] = 0;
        }
        if (elem_kind) elem_kind[j] = p->h_kinds[j];
    }
    return CRB_OK;
}

extern "C" int crb_plan_get_mass(const crb_plan* p, double* M) {
    if (!p || !M) return fail(CRB_EINVAL, "null argument");
    std::memcpy(M, p->h_mass.data(), p->h_mass.size() * sizeof(double));
    return CRB_OK;
}

extern "C" int crb_plan_get_stiffness(const crb_plan* p, double* K) {
    if (!p || !K) return fail(CRB_EINVAL, "null argument");
    if (p->first_nonlinear >= 0)
        return fail(CRB_EINVAL, "Cannot extract stiffness matrix from beam with nonlinear segments. Segment " +
                                    std::to_string(p->first_nonlinear) +
                                    " is nonlinear. Stiffness matrix is only valid for purely linear beams.");
    std::memcpy(K, p->h_stiff.data(), p->h_stiff.size() * sizeof(double));
    return CRB_OK;
}

// ------------------------------------------------------------------ launches
namespace {

int need_device(const crb_plan* p, const char* who) {
    if (!p) return fail(CRB_EINVAL, std::string(who) + ": null plan");
    if (p->device < 0)
        return fail(CRB_ENODEV, std::string(who) + ": host-only plan; the stepper has no CPU path, a HIP device is required");
    hipError_t e = hipSetDevice(p->device);
    if (e != hipSuccess) return fail(CRB_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return CRB_OK;
}

template <typename T>
KParams<T> base_params(const crb_plan* p) {
    KParams<T> k = zeroed<KParams<T>>();
    k.slot = static_cast<const SlotConst<T>*>(p->d_slot);
    k.pcr_levels = static_cast<const T*>(p->d_levels);
    k.pcr_final = static_cast<const T*>(p->d_final);
    k.B = p->B;
    k.S = p->S;
    k.G = p->G;
    k.n_node = p->n_node;
    k.off = p->off;
    k.levels = p->levels;
    k.lognw = p->lognw;
    k.slot_stride = p->slot_stride; k.lv_stride = p->lv_stride; k.fin_stride = p->fin_stride;
    k.flags = p->flags;
    k.imp_slot = -1;
    k.imp_dof = 0;
    k.imp_node_b = nullptr;
    k.duration = 0.0;
    k.gx = T(p->gx);
    k.gy = T(p->gy);
    k.gvec = static_cast<const T*>(p->d_gvec);
    return k;
}

// per-beam status of a stepper launch of `n_steps` steps (crb_plan_set_status): what a beam found non-finite at the end of
// this launch is marked with -- the ensemble's step count by then
template <typename T>
void arm_status(const crb_plan* p, KParams<T>& k, int n_steps) {
    k.status = p->d_status;
    if (!p->d_status) return;
    p->status_steps += n_steps;
    k.status_value = int32_t(p->status_steps < 2147483647LL ? p->status_steps : 2147483647LL);
}

// calls f(T()) with T the plan's dtype (one instantiation of f's body per dtype)
template <typename F>
int with_dtype(const crb_plan* p, F&& f) { return p->dtype == CRB_F64 ? f(double()) : f(float()); }
// what with_int (crb_host.h) returns for a level count no instance covers
auto unsupported(const char* msg) {
    return [msg] { return fail(CRB_EUNSUPPORTED, msg); };
}

// ---- decoded inputs and records: the one check of a crb_input_desc / crb_record_desc against the plan
// The forcing of a launch: amp[b] on DOF `dof` of thread slot `slot` (of node node_b[b] - off per beam when node_b is given)
// while t < duration; the held force [B][n_node][4] or null.
struct Forcing {
    bool impulse = false;
    int slot = -1, dof = 0;
    double duration = 0.0;
    const void* amp = nullptr;
    const int32_t* node_b = nullptr;
    const void* held = nullptr;
};
int decode_input(const crb_plan* p, const crb_input_desc* in, const char* who, Forcing* f) {
    *f = Forcing();
    if (!in) return CRB_OK;
    f->held = in->f_held;
    if (in->kind == CRB_INPUT_NONE) return CRB_OK;
    if (in->kind != CRB_INPUT_IMPULSE) return fail(CRB_EINVAL, std::string(who) + ": unknown input kind");
    if (in->node < 0 || in->node >= p->n_node || in->dof < 0 || in->dof > 2)
        return fail(CRB_EINVAL, std::string(who) + ": impulse node/dof out of range");
    if (!in->amp) return fail(CRB_EINVAL, std::string(who) + ": impulse amplitude array is null");
    if (!p->any_free[3 * in->node + in->dof])   // (mixed ensembles: a beam in which the DOF is constrained ignores it)
        return fail(CRB_EINVAL, std::string(who) + ": impulse targets a constrained DOF");
    f->impulse = true;
    f->slot = in->node - p->off;
    f->dof = in->dof;
    f->duration = in->duration;
    f->amp = in->amp;
    f->node_b = in->node_b;
    return CRB_OK;
}
// The recording of a launch: `count` samples of component `comp` (0 .. 5 of {q, v}) of thread slot `slot`, one every `every`
// steps, into `out`; slot REC_ALL_SLOTS: whole-state snapshots; slot -1: nothing is recorded.
struct Recording {
    int slot = -1, comp = 0, every = 1, count = 0;
    void* out = nullptr;
};
// n: the steps of the launch (a sample after every rec->every-th), or with stepped == false the samples of a t_eval grid
// (crb_solve_rk45_eval: rec->every is unused)
int decode_record(const crb_plan* p, const crb_record_desc* rec, int n, bool stepped, const char* who, Recording* r) {
    *r = Recording();
    if (!rec) return CRB_OK;
    const bool all = rec->node == CRB_RECORD_ALL;
    if ((!all && (rec->plane < 0 || rec->plane > 1 || rec->node < 0 || rec->node >= p->n_node || rec->dof < 0 || rec->dof > 2)) ||
        (stepped && rec->every < 1) || !rec->out)
        return fail(CRB_EINVAL, std::string(who) + ": bad record description");
    const int every = stepped ? rec->every : 1;
    r->count = n / every;
    if (r->count > 0 && (all || rec->node - p->off >= 0)) {   // (the dropped FIXED node 0 records nothing: it is 0 forever)
        r->slot = all ? REC_ALL_SLOTS : rec->node - p->off;
        r->comp = all ? 0 : rec->plane * 3 + rec->dof;
        r->every = every;
        r->out = rec->out;
    }
    return CRB_OK;
}
// the clock a stepper holds after n_steps steps: the same fp64 additions as the kernels and the oracle make
double clock_after(double t0, double dt, int n_steps) {
    double t = t0;
    for (int i = 0; i < n_steps; ++i) t = t + dt;
    return t;
}
// body(g, k0, n, t) for checkpoint segment g of an adjoint rollout -- steps k0 .. k0 + n - 1 of the call, from the clock t the
// checkpoint pass held at step k0 (the same additions) -- from the last segment down, until one returns non-zero
template <typename F>
int for_segments_reversed(int n_steps, int every, double t0, double dt, F&& body) {
    for (int g = (n_steps + every - 1) / every - 1; g >= 0; --g) {
        const int k0 = g * every, n = (n_steps - k0) < every ? (n_steps - k0) : every;
        if (int rc = body(g, k0, n, clock_after(t0, dt, k0))) return rc;
    }
    return CRB_OK;
}
// body(ks, s, hs, t) for sample ks of a sampled-data rollout -- steps s .. s + hs - 1 of the call (hs < hold where the call
// ends inside the sample), from the clock t that the samples before it leave -- in order, until one returns non-zero
template <typename F>
int for_samples(int n_steps, int hold, double t0, double h, F&& body) {
    double t = t0;
    for (int s = 0, ks = 0; s < n_steps; s += hold, ++ks) {
        const int hs = n_steps - s < hold ? n_steps - s : hold;
        if (int rc = body(ks, s, hs, t)) return rc;
        t = clock_after(t, h, hs);
    }
    return CRB_OK;
}
// the decoded recording, and the decoded forcing (and recording), in a launch's parameter block
template <typename T>
void set_record(KParams<T>& k, const Recording& r) {
    k.rec_out = static_cast<T*>(r.out); k.rec_slot = r.slot; k.rec_comp = r.comp; k.rec_every = r.every; k.rec_n = r.count;
}
template <typename T>
void set_io(KParams<T>& k, const Forcing& f, const Recording* r = nullptr) {
    k.u_held = static_cast<const T*>(f.held);
    k.amp = static_cast<const T*>(f.amp);
    k.imp_slot = f.slot; k.imp_dof = f.dof; k.duration = f.duration; k.imp_node_b = f.node_b;
    if (r) set_record(k, *r);
}

// the direction / cotangent count of a derivative call (`name`), refused where each entry point's own documented order has it
int check_count(const std::string& who, const char* name, int n) {
    return n < 1 || n > 65535 ? fail(CRB_EINVAL, who + ": " + name + " must be in [1, 65535]") : CRB_OK;
}

// The control schedule of a call (crb_input_schedule), checked against the call's steps and input; f == nullptr: none.
struct Schedule {
    const void* f = nullptr;
    int K = 0, hold = 0;
};
int decode_schedule(const crb_input_schedule* s, const crb_input_desc* in, int n_steps, const char* who_c, Schedule* out) {
    *out = Schedule();
    if (!s) return CRB_OK;
    const std::string who(who_c);
    if (!s->f_sched) return fail(CRB_EINVAL, who + ": f_sched of the schedule is null");
    if (s->n_intervals < 1) return fail(CRB_EINVAL, who + ": n_intervals of the schedule must be >= 1");
    if (s->hold < 1) return fail(CRB_EINVAL, who + ": hold of the schedule must be >= 1");
    if ((long long)n_steps > (long long)s->n_intervals * (long long)s->hold)
        return fail(CRB_EINVAL, who + ": n_steps exceeds the schedule's n_intervals * hold");
    if (in && in->f_held) return fail(CRB_EINVAL, who + ": a schedule and input->f_held are given together");
    out->f = s->f_sched;
    out->K = s->n_intervals;
    out->hold = s->hold;
    return CRB_OK;
}
// the schedule in the parameter block of a launch whose first step is step `first_step` of the call
template <typename T>
void set_sched(const crb_plan* p, KParams<T>& k, const Schedule& s, int first_step) {
    if (!s.f) return;
    k.sched_stride = force_doubles(p);   // (elements from one interval of a schedule-shaped tensor [K][B][n_node][4] to the next)
    k.sched_hold = s.hold;
    k.sched_first = s.hold - first_step % s.hold;
    k.u_held = static_cast<const T*>(s.f) + size_t(first_step / s.hold) * k.sched_stride;
}

// ---- which kernel a call runs: the condition of every path, side by side.  The shapes the lean kernels are built for are
// stated once per family next to its launcher (lean_*_built, controlled_built, loop_built in crb_*_launch.h: the launchers
// instantiate exactly those); a predicate here asks that function and adds what only a plan knows -- beams per wave,
// threads, the form of gravity, the runtime switches, LDS.  Every other plan runs the general kernels.
bool grav_on(const crb_plan* p) { return (p->flags & CRB_FORCE_GRAVITY) != 0; }
bool f64(const crb_plan* p) { return p->dtype == CRB_F64; }
// the lean kernels carry gravity only in the plain cantilever's nearest-neighbour form
bool lean_grav_ok(const crb_plan* p) { return !grav_on(p) || p->canonical_gravity; }
// crb_step_rk4: one beam per workgroup, or beams of fewer than 64 slots packed G > 1 to a wave (the PACK instantiation); a
// held input has its own instantiation
bool lean_step_ok(const crb_plan* p) {
    const bool packed = p->G > 1 && p->lognw == 0 && p->NT == 64;
    return lean_grav_ok(p) && (p->G == 1 || packed) && p->NT == (64 << p->lognw) && lean_step_built(f64(p), p->levels, p->lognw) &&
           !env_set("CRB_DISABLE_LEAN");
}
// ... and its register-blocked form (crb_lean.h, NPL = 4: one wave per 256-slot beam): fp64 plans with the blocked tables
// (built at plan time for one table set, 256 slots of equal constants, every DOF free, bitwise-uniform lane interiors:
// crb_blocked.h), no gravity, no held input.  CRB_DISABLE_BLOCKED=1: the one-node-per-lane stepper.
bool blocked_step_ok(const crb_plan* p, const void* held) {
    return p->d_blocked && lean_step_ok(p) && !grav_on(p) && !held && p->G == 1 &&
           lean_blocked_built(f64(p), p->blocked_levels, p->elem_mode) && !env_set("CRB_DISABLE_BLOCKED");
}
// crb_rk4_stage: the lean stepper's plans less the packed ones (the stage kernel walks over whole beams)
bool lean_stage_ok(const crb_plan* p) {
    return lean_step_ok(p) && lean_stage_built(f64(p), p->levels, p->lognw) && p->G == 1 && !env_set("CRB_DISABLE_LEAN_STAGE");
}
// crb_solve_rk45: the lean RHS has no gravity form at all; one beam per workgroup
bool lean_rk45_ok(const crb_plan* p) {
    return !grav_on(p) && p->NT == (64 << p->lognw) && lean_rk45_built(f64(p), p->levels, p->lognw) && !env_set("CRB_DISABLE_LEAN");
}
// crb_step_implicit, one beam per workgroup: beams that take more than half of the workgroup's lanes (the full level count
// of that width) ...
bool implicit_group_shape(const crb_plan* p) {
    return p->G == 1 && p->NT == (64 << p->lognw) && p->levels_full == 6 + p->lognw && lean_implicit_built(f64(p), p->levels_full, p->lognw);
}
// ... or several beams per wave
bool implicit_pack_shape(const crb_plan* p) {
    return p->G > 1 && p->lognw == 0 && p->NT == 64 && lean_implicit_pack_built(f64(p), p->levels_full);
}
bool lean_implicit_enabled() { return !env_set("CRB_DISABLE_LEAN") && !env_set("CRB_DISABLE_LEAN_IMPLICIT"); }
// (stiff_levels: where the reduction of A stops for the step size at hand, stiff_tables)
bool lean_implicit_ok(const crb_plan* p) {
    const bool built = implicit_group_shape(p) ? lean_implicit_built(f64(p), p->stiff_levels, p->lognw)
                                               : implicit_pack_shape(p) && lean_implicit_pack_built(f64(p), p->stiff_levels);
    return built && lean_grav_ok(p) && lean_implicit_enabled();
}
// ... with a control schedule: the SCHED instances (lean_implicit_sched_built / lean_implicit_pack_sched_built: the same
// shapes, so that a scheduled call runs the kernel family of the chain of held-force calls it stands for)
bool lean_implicit_sched_ok(const crb_plan* p) {
    if (!lean_implicit_ok(p)) return false;
    return implicit_group_shape(p) ? lean_implicit_sched_built(f64(p), p->stiff_levels, p->lognw)
                                   : lean_implicit_pack_sched_built(f64(p), p->stiff_levels);
}
// crb_solve_controlled: one beam per workgroup; the closed loop (fb) at the levels of M, the implicit scheme at all levels of A
bool lean_controlled_ok(const crb_plan* p, bool fb) {
    const bool shape = p->NT == (64 << p->lognw) && lean_grav_ok(p) && !env_set("CRB_DISABLE_LEAN") &&
                       controlled_built(fb ? p->levels : p->levels_full, fb, p->lognw, grav_on(p), false, false);
    return shape && !env_set(fb ? "CRB_DISABLE_LEAN_FEEDBACK" : "CRB_DISABLE_LEAN_IMPLICIT");
}
// crb_solve_controlled, closed loop: the gain in LDS while it fits there (beams of up to ~30 elements), else streamed from a
// transposed copy in global memory (crb_ctrl.h, SG).  CRB_CTRL_STREAM_GAIN=1: streamed whatever the size.
bool ctrl_stream_gain(const crb_plan* p) {
    if (const char* v = env("CRB_CTRL_STREAM_GAIN"))
        if (std::atoi(v) != 0) return true;
    return ctrl_lds_bytes<double>(p->NT, true, p->n_free) > size_t(160) * 1024;
}
// crb_solve_controlled per_wave: beams of 2 .. 32 slots packed G to a wave, implicit scheme through the lean kernel only
bool controlled_pack_ok(const crb_plan* p, bool fb, bool lean) {
    return !fb && lean && p->G > 1 && controlled_built(p->levels_full, false, p->lognw, grav_on(p), true, false);
}
// crb_step_rk4_feedback, fused: beams that live in one wave and whose gain fits LDS -- the whole rollout as ONE launch of the
// general stepper's feedback instantiation (crb_generic.h, FB) instead of eight launches per step
bool fused_feedback_ok(const crb_plan* p, const void* held) {
    if (p->lognw != 0 || p->NT != 64 || p->mixed_topology || held) return false;
    const char* v = env("CRB_FUSED_FEEDBACK");     // 0 = never, 1 = whenever the gain fits LDS, unset = choose
    if (v && std::atoi(v) == 0) return false;
    const size_t need = p->dtype == CRB_F64 ? fb_lds_bytes<double>(p->NT, p->G, p->n_free) : fb_lds_bytes<float>(p->NT, p->G, p->n_free);
    if (need > size_t(144) * 1024) return false;
    if (v) return true;
    // a workgroup is ONE wave here: with a gain of more than ~50 KB few of them share a CU, and an ensemble that needs
    // several rounds of workgroups is faster through the stage-split path (2048 x 27 elements: 125 against 67 us/step;
    // 64 x 27: 31 against 48; up to 16 elements the fused form wins at every size: 21 against 40 - 48 us/step)
    const size_t per_cu = (size_t(160) * 1024) / need;
    return need <= size_t(52) * 1024 || size_t(beam_groups(p)) <= per_cu * 256;
}
// ... and its packed lean form: several beams per wave (its right-hand side costs half of the general kernel's)
template <typename T>
bool lean_fused_feedback_ok(const crb_plan* p) {
    return p->G > 1 && lean_step_ok(p) && lean_feedback_built(p->levels) && fb_lean_lds_bytes<T>(p->G, p->n_free) <= size_t(144) * 1024 &&
           !env_set("CRB_DISABLE_LEAN_FEEDBACK");
}
// crb_step_rk4_feedback, persistent (crb_loop.h): fp64 plans with one table set and one free-DOF set, beams of 33 .. 128
// thread-carried nodes, gravity absent or canonical, no held input.  CRB_LOOP=0 / 1: never / whenever eligible; unset:
// ensembles of at least LOOP_MIN_BEAMS beams (a group of workgroups owns 64 beams: small ensembles leave most of the chip
// idle and are faster through the stage-split launches).
constexpr int LOOP_MIN_BEAMS = 512;
bool loop_shape_ok(const crb_plan* p) {
    return f64(p) && !p->mixed_topology && shared_tables(*p) && p->G == 1 && p->NT == (64 << p->lognw) && p->S > 32 &&
           loop_built(p->levels, p->lognw) && lean_grav_ok(p);
}
bool loop_ok(const crb_plan* p, const void* held) {
    if (!loop_shape_ok(p) || held) return false;
    if (const char* v = env("CRB_LOOP")) return std::atoi(v) != 0;
    return p->B >= LOOP_MIN_BEAMS;
}

template <typename T, int MODE, int LV, bool LEAN>
int launch_beam_lean(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
    const dim3 grid(beam_groups(p)), block(p->NT);
    const size_t smem = lds_bytes<T>(p->NT);
    // register budget: <=256-thread groups run 2 groups per CU (2 waves/SIMD, 256 VGPRs) so that the
    // solve multipliers stay in registers; 1024-thread groups get what their size allows
    if (p->NT <= 256) {
        hipLaunchKernelGGL((crb_beam_kernel<T, MODE, LV, 256, 2, LEAN>), grid, block, smem, st, k);
    } else if constexpr (LV >= 4) {
        // (beams of more than 256 slots always run a truncated reduction -- their full one has 9 or 10 levels -- and the
        //  truncation never lands below 4 levels: the multipliers of level 3 are ~1e-3; fewer levels are not built)
        if (p->NT <= 512) {
            HIP_TRY(lds_opt_in(crb_beam_kernel<T, MODE, LV, 512, 2, LEAN>, smem));
            hipLaunchKernelGGL((crb_beam_kernel<T, MODE, LV, 512, 2, LEAN>), grid, block, smem, st, k);
        } else {
            HIP_TRY(lds_opt_in(crb_beam_kernel<T, MODE, LV, 1024, 4, LEAN>, smem));
            hipLaunchKernelGGL((crb_beam_kernel<T, MODE, LV, 1024, 4, LEAN>), grid, block, smem, st, k);
        }
    } else {
        return fail(CRB_EUNSUPPORTED, "a beam of more than 256 thread-carried nodes with fewer than 4 cyclic-reduction levels");
    }
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}

template <typename T, int MODE, int LV>
int launch_beam_lv(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
    // LEAN: the stepper without gravity tables and without a held input (BASELINE config 3/4)
    if (MODE == MODE_STEP && !(p->flags & CRB_FORCE_GRAVITY) && !k.u_held)
        return launch_beam_lean<T, MODE, LV, MODE == MODE_STEP>(p, k, st);
    return launch_beam_lean<T, MODE, LV, false>(p, k, st);
}

template <typename T, int MODE>
int launch_beam(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
#ifdef CRB_FAST_BUILD  // kernel-tuning build (make fast): only the config-3 lean stepper is instantiated
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: generic kernels not built");
#else
    return with_int<0, 8>(p->levels, [&](auto lv) { return launch_beam_lv<T, MODE, lv>(p, k, st); },
                          unsupported("unsupported number of cyclic-reduction levels"));
#endif
}

// the lean stepper (crb_lean.hip, one translation unit per dtype)
template <typename T>
int launch_lean(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
#ifdef CRB_FAST_BUILD   // (make fast: the fp64 config-3 instance only; make fast32: the fp32 config-4 one)
#ifdef CRB_FAST_F32
    if constexpr (sizeof(T) == 8) return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD (fp32): fp64 lean stepper not built");
#else
    if constexpr (sizeof(T) == 4) return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: fp32 lean stepper not built");
#endif
    else
#endif
    HIP_TRY(crb::launch_lean(k, p->B, p->levels, p->lognw, grav_on(p), p->elem_mode, st));
    return CRB_OK;
}

// One RK4 stage through the lean machinery (crb_stage_lean_kernel).  Shared-table plans run a bounded number of
// workgroups, each walking over several beams with the solve tables in registers.
template <typename T>
int launch_stage_lean(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
    int groups = p->B;
    if (shared_tables(*p)) {
        // one wave per SIMD (256 CUs x 4) / waves per group: measured best at 2048 x 128 (208 us per step
        // against 220 with two waves per SIMD and 236 with one group per beam) -- the table reload per
        // group costs more than the extra latency hiding gains
        const int cap = int(env_int("CRB_STAGE_GROUPS", 256 * 4 / (1 << p->lognw)));
        if (cap > 0 && groups > cap) groups = cap;
    }
#ifdef CRB_FAST_BUILD
#ifdef CRB_FAST_F32
    if constexpr (sizeof(T) == 8) return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD (fp32): fp64 lean stage kernel not built");
#else
    if constexpr (sizeof(T) == 4) return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: fp32 lean stage kernel not built");
#endif
    else
#endif
    HIP_TRY(crb::launch_stage_lean(k, groups, p->levels, p->lognw, grav_on(p), p->elem_mode, st));
    return CRB_OK;
}

template <typename T>
int pack_impl(const crb_plan* p, bool pack, int rows, const void* red_in, void* dev, void* red_out, hipStream_t st) {
    const size_t total = size_t(p->B) * rows * p->n_free;
    const int bs = 256;
    const unsigned grid = unsigned((total + bs - 1) / bs);
    if (pack) {
        HIP_TRY(hipMemsetAsync(dev, 0, size_t(p->B) * rows * p->n_node * 4 * sizeof(T), st));
        hipLaunchKernelGGL((crb_pack_kernel<T, true>), dim3(grid), dim3(bs), 0, st, p->d_free_index, p->free_index_stride, p->n_free, p->n_node,
                           rows, p->B, static_cast<const T*>(red_in), static_cast<T*>(dev), static_cast<T*>(nullptr));
    } else {
        hipLaunchKernelGGL((crb_pack_kernel<T, false>), dim3(grid), dim3(bs), 0, st, p->d_free_index, p->free_index_stride, p->n_free, p->n_node,
                           rows, p->B, static_cast<const T*>(nullptr), static_cast<T*>(dev), static_cast<T*>(red_out));
    }
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}

int pack_dispatch(const crb_plan* p, bool pack, int rows, const void* red_in, void* dev, void* red_out, void* stream,
                  const char* who) {
    if (int rc = need_device(p, who)) return rc;
    if (!dev || (pack && !red_in) || (!pack && !red_out)) return fail(CRB_EINVAL, std::string(who) + ": null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return p->dtype == CRB_F64 ? pack_impl<double>(p, pack, rows, red_in, dev, red_out, st)
                               : pack_impl<float>(p, pack, rows, red_in, dev, red_out, st);
}

}  // namespace

extern "C" int crb_pack_state(const crb_plan* p, const void* x_red, void* x, void* stream) {
    return pack_dispatch(p, true, 2, x_red, x, nullptr, stream, "crb_pack_state");
}
extern "C" int crb_unpack_state(const crb_plan* p, const void* x, void* x_red, void* stream) {
    return pack_dispatch(p, false, 2, nullptr, const_cast<void*>(x), x_red, stream, "crb_unpack_state");
}
extern "C" int crb_pack_vec(const crb_plan* p, const void* v_red, void* v, void* stream) {
    return pack_dispatch(p, true, 1, v_red, v, nullptr, stream, "crb_pack_vec");
}
extern "C" int crb_unpack_vec(const crb_plan* p, const void* v, void* v_red, void* stream) {
    return pack_dispatch(p, false, 1, nullptr, const_cast<void*>(v), v_red, stream, "crb_unpack_vec");
}

extern "C" int crb_internal_force(const crb_plan* p, const void* x, void* kout, void* stream) {
    if (int rc = need_device(p, "crb_internal_force")) return rc;
    if (!x || !kout) return fail(CRB_EINVAL, "crb_internal_force: null pointer");
    return with_dtype(p, [&](auto t) {
        using T = decltype(t);
        KParams<T> k = base_params<T>(p);
        k.x = static_cast<T*>(const_cast<void*>(x));
        k.out = static_cast<T*>(kout);
        return launch_beam<T, MODE_KQ>(p, k, static_cast<hipStream_t>(stream));
    });
}

extern "C" int crb_rhs(const crb_plan* p, const void* x, const void* u, void* xdot, void* stream) {
    if (int rc = need_device(p, "crb_rhs")) return rc;
    if (!x || !xdot) return fail(CRB_EINVAL, "crb_rhs: null pointer");
    if (x == xdot) return fail(CRB_EINVAL, "crb_rhs: xdot must not alias x");
    return with_dtype(p, [&](auto t) {
        using T = decltype(t);
        KParams<T> k = base_params<T>(p);
        k.x = static_cast<T*>(const_cast<void*>(x));
        k.u_held = static_cast<const T*>(u);
        k.out = static_cast<T*>(xdot);
        return launch_beam<T, MODE_RHS>(p, k, static_cast<hipStream_t>(stream));
    });
}

extern "C" int crb_step_rk4(const crb_plan* p, void* x, double t0, double dt, int n_steps, const crb_input_desc* in,
                            double* t_end, void* stream) {
    return crb_step_rk4_rec(p, x, t0, dt, n_steps, in, nullptr, t_end, stream);
}

namespace {
template <typename T>
int step_rk4_impl(const crb_plan* p, void* x, double t0, double dt, int n_steps, const Forcing& f, const Schedule& sc,
                  const Recording& r, hipStream_t st) {
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(x);
    set_io(k, f, &r);
    set_sched(p, k, sc, 0);   // (a held input of its own: never the lean forms without one, nor the register-blocked stepper)
    k.t0 = t0; k.dt = dt; k.n_steps = n_steps;
    arm_status(p, k, n_steps);
    if constexpr (sizeof(T) == 8) {
        if (blocked_step_ok(p, k.u_held)) {
            k.blocked = p->d_blocked;
            HIP_TRY(crb::launch_lean_blocked(k, p->B, p->blocked_levels, p->elem_mode, p->blocked_twist, st));
            return CRB_OK;
        }
    }
    if (lean_step_ok(p)) return launch_lean<T>(p, k, st);
    return launch_beam<T, MODE_STEP>(p, k, st);
}
}  // namespace

extern "C" int crb_step_rk4_rec(const crb_plan* p, void* x, double t0, double dt, int n_steps, const crb_input_desc* in,
                                const crb_record_desc* rec, double* t_end, void* stream) {
    return crb_step_rk4_sched(p, x, t0, dt, n_steps, in, nullptr, rec, t_end, stream);
}

extern "C" int crb_step_rk4_sched(const crb_plan* p, void* x, double t0, double dt, int n_steps, const crb_input_desc* in,
                                  const crb_input_schedule* sched, const crb_record_desc* rec, double* t_end, void* stream) {
    Schedule sc;
    if (sched) {   // (refused before the device is touched)
        if (!p) return fail(CRB_EINVAL, "crb_step_rk4_sched: null plan");
        if (int rc = decode_schedule(sched, in, n_steps, "crb_step_rk4_sched", &sc)) return rc;
    }
    if (int rc = need_device(p, "crb_step_rk4")) return rc;
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, "crb_step_rk4", &r)) return rc;
    if (!x) return fail(CRB_EINVAL, "crb_step_rk4: null state");
    if (n_steps < 0) return fail(CRB_EINVAL, "crb_step_rk4: n_steps must be >= 0");
    if (!(dt > 0)) return fail(CRB_EINVAL, "crb_step_rk4: dt must be positive");
    Forcing f;
    if (int rc = decode_input(p, in, "crb_step_rk4", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return p->dtype == CRB_F64 ? step_rk4_impl<double>(p, x, t0, dt, n_steps, f, sc, r, st)
                               : step_rk4_impl<float>(p, x, t0, dt, n_steps, f, sc, r, st);
}

// ------------------------------------------------------------------ host-vector entry points (single-beam closures)
namespace {
// device copy of the full -> reduced index map (plans with one free-DOF set)
int ensure_red_map(const crb_plan* p) {
    if (p->d_red_map) return CRB_OK;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_red_map), p->full2red.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(p->d_red_map, p->full2red.data(), p->full2red.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return CRB_OK;
}
int host_path_setup(const crb_plan* p, const char* who) {
    if (int rc = need_device(p, who)) return rc;
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, std::string(who) + ": host-vector calls need an fp64 plan");
    if (p->mixed_topology) return fail(CRB_EUNSUPPORTED, std::string(who) + ": host-vector calls need one free-DOF set for the plan");
    if (p->h_stage) return CRB_OK;
    if (int rc = ensure_red_map(p)) return rc;
    const size_t n = p->free_index.size();
    // (+ 64 bytes: the completion flag of one-workgroup launches)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p->h_stage), size_t(p->B) * 5 * n * sizeof(double) + 64, hipHostMallocMapped));
    std::memset(p->h_stage + size_t(p->B) * 5 * n, 0, 64);
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_stage), p->h_stage, 0));
    HIP_TRY(hipStreamCreateWithFlags(&p->host_stream, hipStreamNonBlocking));
    return CRB_OK;
}
}  // namespace

namespace {
// Waits for a host-path launch.  One workgroup: the kernel raises a flag in host-mapped memory after its output stores
// and the host spins on it (a stream synchronise costs ~8 us of wake-up latency on top of a 5 us kernel).  The spin is
// bounded by the wall clock (CRB_HOST_SPIN_MS, default 200 ms) and looks at the stream every 4096 polls: a launch that failed
// ends the wait with its error at once, a flag that never comes falls back to synchronising the stream.
int host_path_wait(const crb_plan* p, bool flagged, unsigned long long seq) {
    if (flagged) {
        const size_t n = p->free_index.size();
        volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(p->h_stage + size_t(p->B) * 5 * n);
        timespec t0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (unsigned long spin = 1;; ++spin) {
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return CRB_OK;
            __builtin_ia32_pause();
            if ((spin & 4095ul) == 0) {
                const hipError_t q = hipStreamQuery(p->host_stream);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(CRB_EHIP, std::string("host-path launch: ") + hipGetErrorString(q));
                if (q == hipSuccess) break;   // the stream is idle: the kernel has run (its flag store is visible after the synchronise below)
                timespec t1;
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000.0 + (t1.tv_nsec - t0.tv_nsec) * 1e-6 > p->host_spin_ms) break;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(p->host_stream));
    return CRB_OK;
}
}  // namespace

extern "C" int crb_rhs_host(const crb_plan* p, const double* x_red, const double* u_red, double* xdot_red) {
    if (int rc = host_path_setup(p, "crb_rhs_host")) return rc;
    if (!x_red || !xdot_red) return fail(CRB_EINVAL, "crb_rhs_host: null pointer");
    const size_t n = p->free_index.size(), B = size_t(p->B);
    double *hx = p->h_stage, *hu = hx + B * 2 * n, *ho = hu + B * n;
    std::memcpy(hx, x_red, B * 2 * n * sizeof(double));
    if (u_red) std::memcpy(hu, u_red, B * n * sizeof(double));
    KParams<double> k = base_params<double>(p);
    k.x = p->d_stage;
    k.u_held = u_red ? p->d_stage + B * 2 * n : nullptr;
    k.out = p->d_stage + B * 3 * n;
    k.red_map = p->d_red_map;
    k.n_red = int(n);
    const bool flagged = beam_groups(p) == 1;
    if (flagged) {
        k.done_flag = reinterpret_cast<unsigned long long*>(p->d_stage + B * 5 * n);
        k.done_seq = ++p->host_seq;
    }
    if (int rc = launch_beam<double, MODE_RHS>(p, k, p->host_stream)) return rc;
    if (int rc = host_path_wait(p, flagged, k.done_seq)) return rc;
    std::memcpy(xdot_red, ho, B * 2 * n * sizeof(double));
    return CRB_OK;
}

extern "C" int crb_internal_force_host(const crb_plan* p, const double* q_red, double* k_red) {
    if (int rc = host_path_setup(p, "crb_internal_force_host")) return rc;
    if (!q_red || !k_red) return fail(CRB_EINVAL, "crb_internal_force_host: null pointer");
    const size_t n = p->free_index.size(), B = size_t(p->B);
    double *hx = p->h_stage, *ho = hx + B * 3 * n;
    for (size_t b = 0; b < B; ++b) std::memcpy(hx + b * 2 * n, q_red + b * n, n * sizeof(double));   // (state rows of 2n: q | unused)
    KParams<double> k = base_params<double>(p);
    k.x = p->d_stage;
    k.out = p->d_stage + B * 3 * n;
    k.red_map = p->d_red_map;
    k.n_red = int(n);
    const bool flagged = beam_groups(p) == 1;
    if (flagged) {
        k.done_flag = reinterpret_cast<unsigned long long*>(p->d_stage + B * 5 * n);
        k.done_seq = ++p->host_seq;
    }
    if (int rc = launch_beam<double, MODE_KQ>(p, k, p->host_stream)) return rc;
    if (int rc = host_path_wait(p, flagged, k.done_seq)) return rc;
    std::memcpy(k_red, ho, B * n * sizeof(double));
    return CRB_OK;
}

// ------------------------------------------------------------------ implicit stepper (crb_stiff.h)
namespace {
// (re)builds the cyclic-reduction tables of A = M + alpha K0 on `st` when the step size changed
template <typename T>
int stiff_tables(const crb_plan* p, double alpha, hipStream_t st) {
    if (p->stiff_alpha == alpha && p->d_alevels) return CRB_OK;
    AsmInputs& in = *p->asm_in;
    const int S = p->S, lf = p->levels_full, nd = in.nd;
    // a set built earlier for this step size, else the least recently used one (work queued on `st` that still reads
    // the overwritten set is ordered before the assembly launched below on the same stream)
    crb_plan::StiffSet* set = nullptr;
    for (auto& c : p->stiff_sets)
        if (c.lev && c.alpha == alpha) set = &c;
    const bool hit = set != nullptr;
    if (!set) {
        set = &p->stiff_sets[0];
        for (auto& c : p->stiff_sets)
            if (c.used < set->used) set = &c;
    }
    if (!set->lev || !set->fin) {
        // both tables or neither: a set with one of them would pass for built at the next call
        void *lev = nullptr, *fin = nullptr;
        const bool ok = hipMalloc(&lev, size_t(nd) * size_t(lf > 0 ? lf : 1) * S * PCR_LEVEL_VALS * sizeof(T)) == hipSuccess &&
                        hipMalloc(&fin, size_t(nd) * S * PCR_FINAL_VALS * sizeof(T)) == hipSuccess &&
                        (in.dNormScratch.p || in.dNormScratch.alloc(size_t(lf > 0 ? lf : 1)) == 0);
        if (!ok) {
            if (lev) (void)hipFree(lev);
            if (fin) (void)hipFree(fin);
            (void)hipGetLastError();
            return fail(CRB_EHIP, "crb_step_implicit: device allocation failed");
        }
        set->lev = lev;
        set->fin = fin;
    }
    set->used = ++p->stiff_clock;
    p->d_alevels = set->lev;
    p->d_afinal = set->fin;
    if (hit) {
        p->stiff_levels = set->levels;
        p->stiff_alpha = alpha;
        return CRB_OK;
    }
    set->alpha = 0.0;   // (not valid until the build below has been queued; neither is "the set in use" if a launch below fails)
    p->stiff_alpha = 0.0;
    AsmParams a = in.a;
    a.alpha = alpha;
    a.slot_out = nullptr; a.lv64 = nullptr; a.fin64_all = nullptr; a.blocks0 = nullptr;
    a.lvT = p->d_alevels; a.finT = p->d_afinal; a.fin_level = lf; a.norms = in.dNormScratch.p;
    HIP_TRY(hipMemsetAsync(in.dNormScratch.p, 0, size_t(lf > 0 ? lf : 1) * sizeof(double), st));
    hipLaunchKernelGGL((crb_assemble_kernel<T>), dim3(nd), dim3(in.threads), in.smem, st, a);
    HIP_TRY(hipGetLastError());
    // The reduction of A stops where its multipliers fall below the unit roundoff, like the mass matrix's (pick_levels):
    // for the step sizes the examples use (h = 1e-4: the stride-32 multipliers of a 256-node Nitinol rod are ~1e-19) that is
    // 5 levels instead of 8; large steps (h = 1e-3) keep them all.  One stream synchronisation per new step size.
    int used = lf;
    if (lf > 0 && !env_set("CRB_STIFF_ALL_LEVELS")) {
        std::vector<double> norms(static_cast<size_t>(lf));
        HIP_TRY(hipMemcpyAsync(norms.data(), in.dNormScratch.p, size_t(lf) * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        while (used > 0 && norms[size_t(used) - 1] < std::ldexp(1.0, -53)) --used;
        // (the lean kernels are built from some level count on: no fewer than that, lean_implicit_built / lean_implicit_pack_built)
        if (implicit_group_shape(p) && lean_implicit_enabled())
            while (used < lf && !lean_implicit_built(f64(p), used, p->lognw)) ++used;
        if (implicit_pack_shape(p))
            while (used < lf && !lean_implicit_pack_built(f64(p), used)) ++used;
        if (used < lf) {   // the final block inverses after `used` levels
            a.fin_level = used;
            hipLaunchKernelGGL((crb_assemble_kernel<T>), dim3(nd), dim3(in.threads), in.smem, st, a);
            HIP_TRY(hipGetLastError());
        }
    }
    p->stiff_levels = used;
    p->stiff_alpha = alpha;
    set->levels = used;
    set->alpha = alpha;
    return CRB_OK;
}

template <typename T, int LV>
int launch_implicit_lv(const crb_plan* p, const KParams<T>& k, const StiffParams<T>& q, hipStream_t st) {
    const dim3 grid(beam_groups(p)), block(p->NT);
    const size_t smem = lds_bytes<T>(p->NT);
    // one wave per SIMD: the thread's rows of A's tables (10 per level, up to 8 levels) stay in registers
    if (p->NT > 256) return fail(CRB_EUNSUPPORTED, "crb_step_implicit: beams of more than 256 thread-carried nodes are not supported");
    // Up to 5 levels two waves per SIMD fit the register file (65536 x 10: 32 instead of 42 us per step); a launch that
    // does not fill the GPU at one wave per SIMD keeps the whole file per wave (ONE 10-element beam: 3.6 instead of 4.3 us
    // per step).  The full tables of long beams take the file whole.
    const long waves = long(grid.x) * ((p->NT + 63) / 64);
    if (k.sched_stride) {   // a control schedule: the SCHED instances; the two-wave form up to 2 levels (beyond, it would spill)
        if (LV <= 2 && waves > 1024)
            hipLaunchKernelGGL((crb_implicit_kernel<T, LV, 256, (LV <= 2 ? 2 : 1), false, true>), grid, block, smem, st, k, q);
        else hipLaunchKernelGGL((crb_implicit_kernel<T, LV, 256, 1, false, true>), grid, block, smem, st, k, q);
    } else if (LV <= 5 && waves > 1024) hipLaunchKernelGGL((crb_implicit_kernel<T, LV, 256, (LV <= 5 ? 2 : 1)>), grid, block, smem, st, k, q);
    else hipLaunchKernelGGL((crb_implicit_kernel<T, LV, 256, 1>), grid, block, smem, st, k, q);
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}
template <typename T>
int launch_implicit(const crb_plan* p, const KParams<T>& k, const StiffParams<T>& q, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: implicit stepper not built");
#else
    if (k.sched_stride ? lean_implicit_sched_ok(p) : lean_implicit_ok(p)) {
        // one wave per SIMD (the tables of A fill the register file): 256 CUs x 4 / waves per beam workgroups are resident
        const bool grav = grav_on(p);
        const bool shared = shared_tables(*p);   // (the tables of A are per beam exactly where the plan's own are)
        const int minw = k.sched_stride ? implicit_lean_sched_minw(p->stiff_levels, grav, p->lognw, p->G > 1)
                                        : implicit_lean_minw(p->stiff_levels, grav, p->lognw);   // (waves per SIMD: crb_stiff.h)
        int resident = 256 * 4 / (1 << p->lognw) * minw;
        if (const int cap = int(env_int("CRB_LEAN_MAX_GROUPS", 0)); cap > 0) resident = cap;   // (tests)
        const int groups = beam_groups(p);
        HIP_TRY(crb::launch_implicit_lean(k, q, shared ? walk_grid(groups, resident) : groups, p->stiff_levels, p->lognw, grav,
                                          p->elem_mode, st));
        return CRB_OK;
    }
    // (the levels of A whose multipliers matter, stiff_tables)
    return with_int<0, 8>(p->stiff_levels, [&](auto lv) { return launch_implicit_lv<T, lv>(p, k, q, st); },
                          unsupported("crb_step_implicit: beams of more than 256 thread-carried nodes are not supported"));
#endif
}

// the general implicit kernel in its damped form (generalised-alpha): any level count, one wave per SIMD
template <typename T, int LV>
int launch_implicit_damped_lv(const crb_plan* p, const KParams<T>& k, const StiffParams<T>& q, hipStream_t st) {
    const dim3 grid(beam_groups(p)), block(p->NT);
    hipLaunchKernelGGL((crb_implicit_kernel<T, LV, 256, 1, true>), grid, block, lds_bytes<T>(p->NT), st, k, q);
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}
template <typename T>
int launch_implicit_damped(const crb_plan* p, const KParams<T>& k, const StiffParams<T>& q, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: implicit stepper not built");
#else
    if (p->NT > 256) return fail(CRB_EUNSUPPORTED, "crb_step_implicit: beams of more than 256 thread-carried nodes are not supported");
    return with_int<0, 8>(p->stiff_levels, [&](auto lv) { return launch_implicit_damped_lv<T, lv>(p, k, q, st); },
                          unsupported("crb_step_implicit: beams of more than 256 thread-carried nodes are not supported"));
#endif
}

template <typename T>
int step_implicit_impl(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, double rho, const Forcing& f,
                       const Schedule& sc, const Recording& rec, hipStream_t st) {
    const bool damped = rho < 1.0;
    // generalised-alpha coefficients (crb_stiff.h: StiffParams); rho = 1 is the midpoint rule with kappa = h^2 / 4
    const double am_ = (2.0 * rho - 1.0) / (rho + 1.0), af_ = rho / (rho + 1.0);
    const double gam = 0.5 - am_ + af_, bet = 0.25 * (1.0 - am_ + af_) * (1.0 - am_ + af_);
    const double kappa = damped ? (1.0 - af_) * bet * h * h / (1.0 - am_) : 0.25 * h * h;
    if (int rc = stiff_tables<T>(p, kappa, st)) return rc;
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(x);
    set_io(k, f, &rec);
    set_sched(p, k, sc, 0);   // (never with the damped variant)
    k.t0 = t0; k.dt = h; k.n_steps = n_steps;
    arm_status(p, k, n_steps);
    StiffParams<T> q;
    q.a_levels = static_cast<const T*>(p->d_alevels);
    q.a_final = static_cast<const T*>(p->d_afinal);
    q.alv_stride = p->asm_in->nd > 1 ? size_t(p->levels_full) * p->S * PCR_LEVEL_VALS : 0;
    q.afin_stride = p->asm_in->nd > 1 ? size_t(p->S) * PCR_FINAL_VALS : 0;
    q.h = h;
    q.n_iter = n_iter;
    q.a0 = nullptr;
    if (!damped) return launch_implicit<T>(p, k, q, st);
    // a_0: the RHS of the state at t0 with the input of t0 (one launch of the RHS kernel into the plan's scratch)
    if (!p->d_rhs0) HIP_TRY(hipMalloc(&p->d_rhs0, state_doubles(p) * sizeof(T)));
    {
        KParams<T> r = base_params<T>(p);
        r.x = static_cast<T*>(x);
        r.out = static_cast<T*>(p->d_rhs0);
        set_io(r, f);
        r.t0 = t0;
        if (int rc = launch_beam<T, MODE_RHS>(p, r, st)) return rc;
    }
    q.a0 = static_cast<const T*>(p->d_rhs0);
    const double cv = (1.0 - af_) * gam * h / (1.0 - am_);
    q.kappa = kappa; q.cv = cv;
    q.c_qv = (1.0 - af_) * h; q.c_qa = (1.0 - af_) * h * h * (0.5 - bet) - kappa * am_;
    q.c_va = (1.0 - af_) * h * (1.0 - gam) - cv * am_;
    q.tf_frac = 1.0 - af_; q.alpha_m = am_; q.inv1m = 1.0 / (1.0 - am_);
    q.c_q0 = h * h * (0.5 - bet); q.c_q1 = h * h * bet; q.c_v0 = h * (1.0 - gam); q.c_v1 = h * gam;
    return launch_implicit_damped<T>(p, k, q, st);
}
}  // namespace

extern "C" int crb_step_implicit(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter,
                                 const crb_input_desc* in, const crb_record_desc* rec, double* t_end, void* stream) {
    return crb_step_implicit_sched(p, x, t0, h, n_steps, n_iter, in, nullptr, rec, t_end, stream);
}

extern "C" int crb_step_implicit_sched(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter,
                                       const crb_input_desc* in, const crb_input_schedule* sched, const crb_record_desc* rec,
                                       double* t_end, void* stream) {
    if (!sched) return crb_step_implicit_damped(p, x, t0, h, n_steps, n_iter, 1.0, in, rec, t_end, stream);
    // with a schedule every refusal comes before the device is touched: CRB_EINVAL (the stepper's own cases, then the
    // schedule's), CRB_EUNSUPPORTED, CRB_ENODEV
    const char* who = "crb_step_implicit_sched";
    if (!p) return fail(CRB_EINVAL, std::string(who) + ": null plan");
    if (!x) return fail(CRB_EINVAL, std::string(who) + ": null pointer");
    if (n_steps < 0) return fail(CRB_EINVAL, std::string(who) + ": n_steps must be >= 0");
    if (!(h > 0)) return fail(CRB_EINVAL, std::string(who) + ": h must be positive");
    if (n_iter < 1) return fail(CRB_EINVAL, std::string(who) + ": n_iter must be >= 1");
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, who, &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who, &f)) return rc;
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, who, &sc)) return rc;
    if (p->dtype != CRB_F64)
        return fail(CRB_EUNSUPPORTED, std::string(who) + ": the implicit stepper needs an fp64 plan (the iteration matrix is too ill-conditioned for fp32)");
    if (p->NT > 256) return fail(CRB_EUNSUPPORTED, std::string(who) + ": beams of more than 256 thread-carried nodes are not supported");
    if (int rc = need_device(p, who)) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    return step_implicit_impl<double>(p, x, t0, h, n_steps, n_iter, 1.0, f, sc, r, static_cast<hipStream_t>(stream));
}

extern "C" int crb_step_implicit_damped(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, double rho_inf,
                                        const crb_input_desc* in, const crb_record_desc* rec, double* t_end, void* stream) {
    if (int rc = need_device(p, "crb_step_implicit")) return rc;
    if (!(rho_inf >= 0.0 && rho_inf <= 1.0)) return fail(CRB_EINVAL, "crb_step_implicit_damped: rho_inf must be in [0, 1]");
    if (!x) return fail(CRB_EINVAL, "crb_step_implicit: null pointer");
    if (n_steps < 0) return fail(CRB_EINVAL, "crb_step_implicit: n_steps must be >= 0");
    if (!(h > 0)) return fail(CRB_EINVAL, "crb_step_implicit: h must be positive");
    if (n_iter < 1) return fail(CRB_EINVAL, "crb_step_implicit: n_iter must be >= 1");
    if (p->dtype != CRB_F64)   // cond(M + h^2/4 K0) is 1e6 ... 1e9 at the step sizes this stepper is for
        return fail(CRB_EUNSUPPORTED, "crb_step_implicit: the implicit stepper needs an fp64 plan (the iteration matrix is too ill-conditioned for fp32)");
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, "crb_step_implicit", &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, "crb_step_implicit", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    return step_implicit_impl<double>(p, x, t0, h, n_steps, n_iter, rho_inf, f, Schedule(), r, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------ step-size control in the kernel (crb_ctrl.h)
namespace {
// the ladder of A's tables for pieces of length `len`: rung r holds the factorisation for h = len / 2^r (all levels)
int ctrl_ladder(const crb_plan* p, double len, int rungs, hipStream_t st, const crb_plan::Ladder** out) {
    AsmInputs& in = *p->asm_in;
    const int S = p->S, lf = p->levels_full, nd = in.nd;
    const size_t lv_rung = size_t(nd) * size_t(lf > 0 ? lf : 1) * S * PCR_LEVEL_VALS, fin_rung = size_t(nd) * S * PCR_FINAL_VALS;
    crb_plan::Ladder* lad = nullptr;
    for (auto& c : p->ladders)
        if (c.lev && c.len == len && c.rungs >= rungs) lad = &c;
    if (lad) {
        lad->used = ++p->stiff_clock;
        *out = lad;
        return CRB_OK;
    }
    lad = &p->ladders[0];
    for (auto& c : p->ladders)
        if (c.used < lad->used) lad = &c;
    if (lv_rung * size_t(rungs) * sizeof(double) > (size_t(8) << 30))
        return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: the table ladder of this ensemble (per-beam tables) exceeds 8 GiB; give the step count instead");
    // (work queued on `st` that still reads a replaced ladder is ordered before the frees below: hipFree waits for the device)
    if (lad->lev) (void)hipFree(lad->lev);
    if (lad->fin) (void)hipFree(lad->fin);
    lad->lev = lad->fin = nullptr;
    lad->len = 0.0; lad->rungs = 0;
    void *lev = nullptr, *fin = nullptr;
    const bool ok = hipMalloc(&lev, lv_rung * size_t(rungs) * sizeof(double)) == hipSuccess &&
                    hipMalloc(&fin, fin_rung * size_t(rungs) * sizeof(double)) == hipSuccess &&
                    (in.dNormScratch.p || in.dNormScratch.alloc(size_t(lf > 0 ? lf : 1)) == 0);
    if (!ok) {
        if (lev) (void)hipFree(lev);
        if (fin) (void)hipFree(fin);
        (void)hipGetLastError();
        return fail(CRB_EHIP, "crb_solve_controlled: device allocation failed");
    }
    lad->lev = lev;
    lad->fin = fin;
    HIP_TRY(hipMemsetAsync(in.dNormScratch.p, 0, size_t(lf > 0 ? lf : 1) * sizeof(double), st));
    for (int r = 0; r < rungs; ++r) {
        const double h = len / double(1 << r);
        AsmParams a = in.a;
        a.alpha = 0.25 * h * h;
        a.slot_out = nullptr; a.lv64 = nullptr; a.fin64_all = nullptr; a.blocks0 = nullptr;
        a.lvT = static_cast<double*>(lev) + size_t(r) * lv_rung;
        a.finT = static_cast<double*>(fin) + size_t(r) * fin_rung;
        a.fin_level = lf;
        a.norms = in.dNormScratch.p;
        hipLaunchKernelGGL((crb_assemble_kernel<double>), dim3(nd), dim3(in.threads), in.smem, st, a);
        HIP_TRY(hipGetLastError());
    }
    lad->len = len;
    lad->rungs = rungs;
    lad->used = ++p->stiff_clock;
    *out = lad;
    return CRB_OK;
}
}  // namespace

extern "C" int crb_solve_controlled(const crb_plan* p, void* x, double t0, double dt_eval, int n_intervals,
                                    const crb_control_desc* ctl, const crb_input_desc* in, const void* gain, const void* ref,
                                    void* y_out, void* stats, void* used, void* stream) {
    if (int rc = need_device(p, "crb_solve_controlled")) return rc;
    if (!x || !ctl || !stats) return fail(CRB_EINVAL, "crb_solve_controlled: null pointer");
    if (n_intervals < 0 || !(dt_eval > 0)) return fail(CRB_EINVAL, "crb_solve_controlled: n_intervals >= 0 and dt_eval > 0 required");
    if (!(ctl->rtol > 0) || !(ctl->atol >= 0)) return fail(CRB_EINVAL, "crb_solve_controlled: tolerances must be positive");
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: the controlled steppers need an fp64 plan");
    if (p->NT > 256) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: beams of more than 256 thread-carried nodes are not supported");
    const bool fb = gain != nullptr;
    // (one modified-Newton iteration per step: at the step sizes the controller takes the previous step's iterate is converged
    //  after one -- same errors and step counts +-15 % as with two on linear, nonlinear and mixed rods at rtol 1e-1 .. 1e-3,
    //  half the time: profiles/exp_niter.py; what is left of the iteration error scales with h and is part of the estimate)
    const int n_iter = ctl->n_iter > 0 ? ctl->n_iter : 1;
    const int rungs = ctl->max_rungs > 0 ? ctl->max_rungs : 15;   // up to 2^14 fine steps per piece
    if (rungs < 2 || rungs > 24) return fail(CRB_EINVAL, "crb_solve_controlled: max_rungs must be in 2 .. 24");
    Forcing f;
    if (int rc = decode_input(p, in, "crb_solve_controlled", &f)) return rc;
    if (fb) {
        if (p->mixed_topology) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: one gain matrix for the ensemble needs one free-DOF set");
        if (f.held) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: the closed loop runs without a held force");
        // (the closed loop's instances cover 0 .. 6 levels of M: uniform Nitinol rods of up to 255 elements keep 5, crb_ctrl_launch.h)
        if (p->levels > 6) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: unsupported number of cyclic-reduction levels");
    } else if (ref) {
        return fail(CRB_EINVAL, "crb_solve_controlled: a reference without a gain");
    }
    if (n_intervals == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);

    // the pieces: whole t_eval intervals, the one the impulse ends in cut at that instant (inside a piece the input is constant)
    const bool impulse = f.impulse;
    const double t_switch = f.duration;
    std::vector<crb::CtrlPiece> pieces;
    pieces.reserve(size_t(n_intervals) + 1);
    double lens[crb::CTRL_MAX_LADDERS] = {dt_eval, 0.0, 0.0};
    int n_ladders = 1;
    for (int k = 0; k < n_intervals; ++k) {
        const double t_k = t0 + k * dt_eval, t_n = t0 + (k + 1) * dt_eval;
        const bool cut = impulse && t_k + 1e-9 * dt_eval < t_switch && t_switch < t_n - 1e-9 * dt_eval;
        const int parts = cut ? 2 : 1;
        for (int part = 0; part < parts; ++part) {
            crb::CtrlPiece c;
            c.t_a = part == 0 ? t_k : t_switch;
            const double t_b = (cut && part == 0) ? t_switch : t_n;
            c.len = cut ? t_b - c.t_a : dt_eval;
            c.ladder = 0;
            if (cut) { c.ladder = n_ladders; lens[n_ladders++] = c.len; }
            c.on = (impulse && 0.5 * (c.t_a + t_b) < t_switch) ? 1 : 0;
            c.rec = (part == parts - 1 && y_out) ? k : -1;
            c.interval = k;
            pieces.push_back(c);
        }
    }
    crb::CtrlParams<double> q = zeroed<crb::CtrlParams<double>>();
    if (!fb) {
        if (p->levels_full > 8) return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: beams of more than 256 thread-carried nodes are not supported");
        const int lf = p->levels_full, nd = p->asm_in->nd;
        for (int l = 0; l < n_ladders; ++l) {
            const crb_plan::Ladder* lad = nullptr;
            if (int rc = ctrl_ladder(p, lens[l], rungs, st, &lad)) return rc;
            q.a_levels[l] = static_cast<const double*>(lad->lev);
            q.a_final[l] = static_cast<const double*>(lad->fin);
        }
        for (int l = n_ladders; l < crb::CTRL_MAX_LADDERS; ++l) { q.a_levels[l] = q.a_levels[0]; q.a_final[l] = q.a_final[0]; }
        q.lv_rung = size_t(nd) * size_t(lf > 0 ? lf : 1) * p->S * PCR_LEVEL_VALS;
        q.fin_rung = size_t(nd) * p->S * PCR_FINAL_VALS;
        q.alv_stride = nd > 1 ? size_t(lf > 0 ? lf : 1) * p->S * PCR_LEVEL_VALS : 0;
        q.afin_stride = nd > 1 ? size_t(p->S) * PCR_FINAL_VALS : 0;
    }
    // (the piece list of an earlier call may still be read by its launch: wait for the stream before replacing it)
    const size_t piece_bytes = pieces.size() * sizeof(crb::CtrlPiece);
    HIP_TRY(hipStreamSynchronize(st));
    if (p->pieces_cap < piece_bytes) {
        if (p->d_pieces) (void)hipFree(p->d_pieces);
        p->d_pieces = nullptr; p->pieces_cap = 0;
        HIP_TRY(hipMalloc(&p->d_pieces, piece_bytes));
        p->pieces_cap = piece_bytes;
    }
    HIP_TRY(hipMemcpy(p->d_pieces, pieces.data(), piece_bytes, hipMemcpyHostToDevice));
    q.pieces = static_cast<const crb::CtrlPiece*>(p->d_pieces);
    // the streamed gain: its transposed copy, rebuilt from `gain` on every call (after the wait above: no launch reads the old one)
    const bool stream_gain = fb && ctrl_stream_gain(p);
    q.gain_t = nullptr;
    if (stream_gain) {
        const int n = p->n_free, rows = crb::ctrl_sg_rows(2 * n);
        const size_t bytes = size_t(rows) * size_t(n) * sizeof(double);
        if (p->gain_t_cap < bytes) {
            if (p->d_gain_t) (void)hipFree(p->d_gain_t);
            p->d_gain_t = nullptr; p->gain_t_cap = 0;
            HIP_TRY(hipMalloc(&p->d_gain_t, bytes));
            p->gain_t_cap = bytes;
        }
        HIP_TRY(crb::launch_gain_transpose(static_cast<const double*>(gain), static_cast<double*>(p->d_gain_t), n, rows, st));
        q.gain_t = static_cast<const double*>(p->d_gain_t);
    }
    q.n_pieces = int(pieces.size());
    q.n_rungs = rungs; q.n_iter = n_iter; q.n_intervals = n_intervals;
    q.rtol = ctl->rtol; q.atol = ctl->atol;
    // the first coarse solution: h ~ 1e-4 s for the implicit scheme, 5e-6 s for RK4 (near the closed loop's stability limit
    // for the Nitinol examples, 8.6e-6 s)
    q.rate0 = ctl->first_rate > 0 ? ctl->first_rate : (fb ? 2e5 : 1e4);
    q.n_state = 2 * p->n_free; q.n_state_b = p->d_n_state; q.positions_only = ctl->positions_only ? 1 : 0;
    q.stats = static_cast<int32_t*>(stats);
    q.used = static_cast<int32_t*>(used);
    q.y_out = static_cast<double*>(y_out);
    q.series_out = nullptr; q.series_slot = -1; q.series_comp = 0;
    if (ctl->series_out) {
        if (ctl->series_plane < 0 || ctl->series_plane > 1 || ctl->series_node < 0 || ctl->series_node >= p->n_node || ctl->series_dof < 0 ||
            ctl->series_dof > 2)
            return fail(CRB_EINVAL, "crb_solve_controlled: bad series description");
        if (ctl->series_node - p->off >= 0) {   // (a node without a thread slot -- the fixed root -- stays at the caller's zeros)
            q.series_out = static_cast<double*>(ctl->series_out);
            q.series_slot = ctl->series_node - p->off;
            q.series_comp = 3 * ctl->series_plane + ctl->series_dof;
        }
    }

    KParams<double> k = base_params<double>(p);
    k.G = 1;
    k.x = static_cast<double*>(x);
    set_io(k, f);
    k.t0 = t0;
    arm_status(p, k, 1);   // (per-beam status, crb_plan_set_status: a controlled launch counts as one step of the ensemble)
    if (fb) {
        if (int rc = ensure_red_map(p)) return rc;
        k.red_map = p->d_red_map;
        k.n_red = p->n_free;
        k.fb_gain = static_cast<const double*>(gain);
        k.fb_ref = static_cast<const double*>(ref);
    }
    const int threads = p->NT;
    // the lean iteration (crb_stiff.h) where the plan allows it
    const bool lean = lean_controlled_ok(p, fb);
    const int lean_lognw = lean ? p->lognw : -1;
    // per_wave: short beams packed G to a wave, one step sequence per wave (the worst of its beams decides)
    const bool pack = ctl->per_wave != 0 && controlled_pack_ok(p, fb, lean);
    if (ctl->per_wave != 0 && !pack)
        return fail(CRB_EUNSUPPORTED, "crb_solve_controlled: per_wave packs beams of 2 .. 32 thread-carried nodes of the implicit scheme (gravity absent or canonical)");
    if (pack) k.G = p->G;
    HIP_TRY(crb::launch_controlled(k, q, fb ? p->levels : p->levels_full, fb, stream_gain, lean_lognw, grav_on(p), pack, threads,
                                   ctrl_lds_bytes<double>(threads, fb, p->n_free, fb ? -1 : lean_lognw, stream_gain), st));
    return CRB_OK;
}

namespace {
// One RK4 stage of the stage-split stepper (crb_rk4_stage) with its input force u_stage, which takes the place of the held
// force: the forcing's f_held is not read here
template <typename T>
int rk4_stage_impl(const crb_plan* p, void* x, const void* xs, void* acc, void* xs_next, const void* u_stage, int stage,
                   double t_stage, double dt, const Forcing& f, hipStream_t st, bool report) {
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(x); k.xs = static_cast<const T*>(xs); k.acc = static_cast<T*>(acc);
    k.out = static_cast<T*>(xs_next);
    set_io(k, f);
    k.u_held = static_cast<const T*>(u_stage);
    k.stage = stage; k.t0 = t_stage; k.dt = dt;
    if (stage == 3 && report) arm_status(p, k, 1);
    if (lean_stage_ok(p)) return launch_stage_lean<T>(p, k, st);
    return launch_beam<T, MODE_STAGE>(p, k, st);
}
// report: stage 3 marks non-finite beams in the plan's status words (the differentiable rollouts leave the status alone)
int rk4_stage(const crb_plan* p, void* x, const void* xs, void* acc, void* xs_next, const void* u_stage, int stage, double t_stage,
              double dt, const Forcing& f, void* stream, bool report = true) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return p->dtype == CRB_F64 ? rk4_stage_impl<double>(p, x, xs, acc, xs_next, u_stage, stage, t_stage, dt, f, st, report)
                               : rk4_stage_impl<float>(p, x, xs, acc, xs_next, u_stage, stage, t_stage, dt, f, st, report);
}

// The stage-split closed loop: per RK4 stage the feedback force of the stage state (force(xs, u): one GEMM over the ensemble,
// or one per gain group) and one stage launch.  work: the accumulator, two stage states and the force.
template <typename Force>
int feedback_rollout(const crb_plan* p, void* x, double t0, double dt, int n_steps, const Forcing& f, void* work, Force force,
                     void* stream) {
    const size_t state = state_doubles(p) * (p->dtype == CRB_F64 ? sizeof(double) : sizeof(float));
    char* w = static_cast<char*>(work);
    void* acc = w;
    void* bufs[2] = {w + state, w + 2 * state};
    void* u = w + 3 * state;
    // entries of u that no GEMM writes (constrained DOFs, beams without a gain) must read as zero
    HIP_TRY(hipMemsetAsync(u, 0, state / 2, static_cast<hipStream_t>(stream)));
    double t = t0;
    for (int s = 0; s < n_steps; ++s) {
        const double th = t + 0.5 * dt, t1 = t + dt;   // same clock convention as crb_step_rk4
        const double ts[4] = {t, th, th, t1};
        const void* cur = x;
        for (int stage = 0; stage < 4; ++stage) {
            if (int rc = force(cur, u)) return rc;
            void* nxt = bufs[stage & 1];
            if (int rc = rk4_stage(p, x, cur, acc, nxt, u, stage, ts[stage], dt, f, stream)) return rc;
            cur = nxt;
        }
        t = t + dt;
    }
    return CRB_OK;
}

template <typename T, int LV>
int launch_fused_feedback_lv(const crb_plan* p, const KParams<T>& k, hipStream_t st) {
    const dim3 grid(beam_groups(p)), block(p->NT);
    const size_t smem = fb_lds_bytes<T>(p->NT, p->G, p->n_free);
    HIP_TRY(lds_opt_in(crb_beam_kernel<T, MODE_STEP, LV, 64, 1, false, true>, smem));
    hipLaunchKernelGGL((crb_beam_kernel<T, MODE_STEP, LV, 64, 1, false, true>), grid, block, smem, st, k);
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}
template <typename T>
int fused_feedback_impl(const crb_plan* p, void* x, double t0, double dt, int n_steps, const void* gain, const void* ref,
                        const Forcing& f, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: generic kernels not built");
#else
    if (int rc = ensure_red_map(p)) return rc;
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(x);
    k.t0 = t0; k.dt = dt; k.n_steps = n_steps;
    arm_status(p, k, n_steps);
    const Recording none;
    set_io(k, f, &none);
    k.red_map = p->d_red_map;
    k.n_red = p->n_free;
    k.fb_gain = static_cast<const T*>(gain);
    k.fb_ref = static_cast<const T*>(ref);
    if (lean_fused_feedback_ok<T>(p)) {
        HIP_TRY(crb::launch_lean_feedback(k, p->B, p->levels, grav_on(p), st));
        return CRB_OK;
    }
    // (a beam inside one wave: at most 6 levels)
    return with_int<0, 6>(p->levels, [&](auto lv) { return launch_fused_feedback_lv<T, lv>(p, k, st); },
                          unsupported("crb_step_rk4_feedback: unsupported number of cyclic-reduction levels"));
#endif
}

int loop_feedback(const crb_plan* p, void* x, double t0, double dt, int n_steps, const void* gain, const void* ref, const Forcing& f,
                  void* work, hipStream_t st) {
    if (int rc = ensure_red_map(p)) return rc;
    const int nb = loop_nb(p->lognw), n_rb = (p->B + 63) / 64;
    const crb::LoopWork lay = crb::loop_work_layout(nb, n_rb < crb::LOOP_MAX_GROUPS ? n_rb : crb::LOOP_MAX_GROUPS);
    char* w = static_cast<char*>(work);
    crb::LoopParams<double> P = zeroed<crb::LoopParams<double>>();
    P.k = base_params<double>(p);
    P.k.x = static_cast<double*>(x);
    P.k.t0 = t0; P.k.dt = dt; P.k.n_steps = n_steps;
    arm_status(p, P.k, n_steps);
    set_io(P.k, f);
    P.ref = static_cast<const double*>(ref);
    P.red_map = p->d_red_map;
    P.n_red = p->n_free;
    P.sync = reinterpret_cast<unsigned*>(w);
    P.kfrag = reinterpret_cast<const double*>(w + lay.kfrag);
    P.ebuf = reinterpret_cast<double*>(w + lay.ebuf);
    P.ubuf = reinterpret_cast<double*>(w + lay.ubuf);
    P.ownbuf = reinterpret_cast<double*>(w + lay.ownbuf);
    P.n_rb = n_rb;
    P.fences = int(env_int("CRB_LOOP_FENCES", 0));
    P.timeout = (unsigned long long)env_int("CRB_LOOP_TIMEOUT_MS", 2000) * 100000ull;   // 100 MHz ticks
    // every polled word starts at zero, in every call
    HIP_TRY(hipMemsetAsync(w, 0, size_t(crb::LOOP_SYNC_WORDS) * sizeof(unsigned), st));
    const hipError_t e = p->lognw == 1 ? crb::launch_loop_long(P, static_cast<const double*>(gain), p->levels, grav_on(p), p->elem_mode, st)
                                       : crb::launch_loop_short(P, static_cast<const double*>(gain), p->levels, grav_on(p), p->elem_mode, st);
    if (e != hipSuccess) return fail(CRB_EHIP, std::string("crb_step_rk4_feedback (persistent stepper): ") + hipGetErrorString(e));
    p->loop_used = true;
    return CRB_OK;
}
}  // namespace

extern "C" size_t crb_feedback_work_bytes(const crb_plan* p) {
    if (!p) return 0;
    const size_t state = state_doubles(p) * (p->dtype == CRB_F64 ? sizeof(double) : sizeof(float)), force = state / 2;
    size_t need = 3 * state + force;
    if (loop_shape_ok(p)) {
        const int n_rb = (p->B + 63) / 64;
        const size_t loop = crb::loop_work_layout(loop_nb(p->lognw), n_rb < crb::LOOP_MAX_GROUPS ? n_rb : crb::LOOP_MAX_GROUPS).total;
        if (loop > need) need = loop;
    }
    return need;
}

extern "C" int crb_feedback_path(const crb_plan* p) {
    if (!p || p->device < 0) return 0;
    if (loop_ok(p, nullptr)) return 2;
    return fused_feedback_ok(p, nullptr) ? 1 : 0;
}

extern "C" int crb_feedback_status(const crb_plan* p, const void* work, int32_t* status, void* stream) {
    if (int rc = need_device(p, "crb_feedback_status")) return rc;
    if (!work || !status) return fail(CRB_EINVAL, "crb_feedback_status: null pointer");
    *status = 0;
    if (!p->loop_used) return CRB_OK;   // (only the persistent stepper keeps a status word)
    unsigned words[2] = {0, 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(words, work, sizeof(words), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *status = int32_t(words[1]);
    return CRB_OK;
}

extern "C" int crb_step_rk4_feedback(const crb_plan* p, void* x, double t0, double dt, int n_steps, const void* gain,
                                     const void* ref, const crb_input_desc* in, void* work, double* t_end, void* stream) {
    if (int rc = need_device(p, "crb_step_rk4_feedback")) return rc;
    if (!x || !gain || !work) return fail(CRB_EINVAL, "crb_step_rk4_feedback: null pointer");
    if (n_steps < 0 || !(dt > 0)) return fail(CRB_EINVAL, "crb_step_rk4_feedback: n_steps >= 0 and dt > 0 required");
    p->loop_used = false;
    Forcing f;
    if (int rc = decode_input(p, in, "crb_step_rk4_feedback", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (loop_ok(p, f.held)) {
        if (n_steps == 0) return CRB_OK;
        return loop_feedback(p, x, t0, dt, n_steps, gain, ref, f, work, st);
    }
    if (fused_feedback_ok(p, f.held)) {
        if (n_steps == 0) return CRB_OK;
        return p->dtype == CRB_F64 ? fused_feedback_impl<double>(p, x, t0, dt, n_steps, gain, ref, f, st)
                                   : fused_feedback_impl<float>(p, x, t0, dt, n_steps, gain, ref, f, st);
    }
    return feedback_rollout(p, x, t0, dt, n_steps, f, work,
                            [&](const void* xs, void* u) { return crb_feedback_force(p, xs, gain, ref, u, stream); }, stream);
}

namespace {
template <typename T, int LV>
int launch_rk45_lv(const crb_plan* p, const KParams<T>& k, const Rk45Params& q, hipStream_t st) {
    const dim3 grid(p->B), block(p->NT);
    const size_t smem = rk45_lds_bytes<T>(p->NT);
    if (p->NT <= 256) {
        HIP_TRY(lds_opt_in(crb_rk45_kernel<T, LV, 256, 1>, smem));
        hipLaunchKernelGGL((crb_rk45_kernel<T, LV, 256, 1>), grid, block, smem, st, k, q);
    } else if constexpr (LV >= 4) {
        HIP_TRY(lds_opt_in(crb_rk45_kernel<T, LV, 1024, 1>, smem));
        hipLaunchKernelGGL((crb_rk45_kernel<T, LV, 1024, 1>), grid, block, smem, st, k, q);
    } else {
        return fail(CRB_EUNSUPPORTED, "a beam of more than 256 thread-carried nodes with fewer than 4 cyclic-reduction levels");
    }
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}
template <typename T>
int launch_rk45(const crb_plan* p, const KParams<T>& k, const Rk45Params& q, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: rk45 not built");
#else
    if (lean_rk45_ok(p)) {   // the lean RHS (crb_lean.hip)
        HIP_TRY(crb::launch_rk45_lean(k, q, p->B, p->levels, p->lognw, p->elem_mode, st));
        return CRB_OK;
    }
    return with_int<0, 6>(p->levels, [&](auto lv) { return launch_rk45_lv<T, lv>(p, k, q, st); },
                          unsupported("crb_solve_rk45: unsupported number of cyclic-reduction levels"));
#endif
}
template <typename T>
int rk45_impl(const crb_plan* p, void* x, const Forcing& f, const Rk45Params& q, hipStream_t st) {
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(x);
    set_io(k, f);
    return launch_rk45<T>(p, k, q, st);
}
}  // namespace

extern "C" int crb_solve_rk45(const crb_plan* p, void* x, double t0, double t_end, double rtol, double atol,
                              const crb_input_desc* in, void* h, void* stats, int max_steps, void* stream) {
    return crb_solve_rk45_eval(p, x, t0, t_end, rtol, atol, in, h, stats, max_steps, nullptr, 0.0, 0.0, 0, stream);
}

extern "C" int crb_solve_rk45_eval(const crb_plan* p, void* x, double t0, double t_end, double rtol, double atol,
                                   const crb_input_desc* in, void* h, void* stats, int max_steps,
                                   const crb_record_desc* rec, double eval_t0, double eval_dt, int n_eval, void* stream) {
    if (int rc = need_device(p, "crb_solve_rk45")) return rc;
    Recording r;   // (a record with no grid points records nothing and is not checked)
    if (int rc = decode_record(p, n_eval > 0 ? rec : nullptr, n_eval, false, "crb_solve_rk45", &r)) return rc;
    if (rec && n_eval > 0 && (!(eval_dt > 0) || eval_t0 < t0)) return fail(CRB_EINVAL, "crb_solve_rk45: bad t_eval description");
    if (!x) return fail(CRB_EINVAL, "crb_solve_rk45: null state");
    if (!(t_end > t0)) return fail(CRB_EINVAL, "crb_solve_rk45: t_end must be greater than t0");
    if (!(rtol > 0) || !(atol >= 0)) return fail(CRB_EINVAL, "crb_solve_rk45: tolerances must be positive");
    // (beams of fewer than 64 slots run one per wave here, not packed: every beam has its own step sequence)
    if (rk45_lds_bytes<double>(p->NT) > 160 * 1024)
        return fail(CRB_EUNSUPPORTED, "crb_solve_rk45: beam too long for the LDS-resident stage storage");
    Forcing f;
    if (int rc = decode_input(p, in, "crb_solve_rk45", &f)) return rc;
    Rk45Params q;
    q.t0 = t0; q.t_end = t_end; q.rtol = rtol; q.atol = atol;
    q.h_io = static_cast<double*>(h); q.stats = static_cast<int32_t*>(stats);
    q.n_state = 2 * p->n_free; q.n_state_b = p->d_n_state; q.max_steps = max_steps > 0 ? max_steps : 100000000;
    q.eval_t0 = eval_t0; q.eval_dt = eval_dt;
    q.eval_out = r.out; q.n_eval = r.out ? r.count : 0; q.eval_slot = r.slot; q.eval_comp = r.comp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return p->dtype == CRB_F64 ? rk45_impl<double>(p, x, f, q, st) : rk45_impl<float>(p, x, f, q, st);
}

namespace {
template <typename T, int BM, int BN, int BK, int WR>
int launch_feedback_tile(const FeedbackParams<T>& f, int ksplit, hipStream_t st) {
    const dim3 grid((f.B + BM - 1) / BM, (f.n + BN - 1) / BN, ksplit);
    const size_t smem = feedback_lds_bytes<T, BM, BN, BK>(f.n2);
    if (ksplit > 1) HIP_TRY(hipMemsetAsync(f.u, 0, size_t(f.B) * f.u_stride * sizeof(T), st));
    if (f.ref) {
        HIP_TRY(lds_opt_in(crb_feedback_kernel<T, BM, BN, BK, WR, true>, smem));
        hipLaunchKernelGGL((crb_feedback_kernel<T, BM, BN, BK, WR, true>), grid, dim3(256), smem, st, f);
    } else {
        HIP_TRY(lds_opt_in(crb_feedback_kernel<T, BM, BN, BK, WR, false>, smem));
        hipLaunchKernelGGL((crb_feedback_kernel<T, BM, BN, BK, WR, false>), grid, dim3(256), smem, st, f);
    }
    return CRB_OK;
}
template <typename T, int BN, int BK>
int launch_feedback_ws(const FeedbackParams<T>& f, hipStream_t st) {
    const dim3 grid((f.B + 63) / 64, (f.n + BN - 1) / BN);
    const size_t smem = feedback_lds_bytes<T, 64, BN, BK>(f.n2);
    if (f.ref) {
        HIP_TRY(lds_opt_in(crb_feedback_ws_kernel<T, BN, BK, true>, smem));
        hipLaunchKernelGGL((crb_feedback_ws_kernel<T, BN, BK, true>), grid, dim3(256 + WS_NL), smem, st, f);
    } else {
        HIP_TRY(lds_opt_in(crb_feedback_ws_kernel<T, BN, BK, false>, smem));
        hipLaunchKernelGGL((crb_feedback_ws_kernel<T, BN, BK, false>), grid, dim3(256 + WS_NL), smem, st, f);
    }
    return CRB_OK;
}
// tile: 0 = choose.  Large ensembles: 64 x 48 outputs per workgroup, wave-specialised (one workgroup per CU
// and the fewest L2 reads at the config-5 shape: 32.7 us at 2048 x 768 x 384 against 37 us for 32 x 32);
// small ensembles: 32 x 32 for the larger grid.  CRB_FEEDBACK_TILE=48|32 forces one (tests cover both).
template <typename T>
int launch_feedback(int tile, const FeedbackParams<T>& f, hipStream_t st) {
    const long wide_groups = long((f.B + 63) / 64) * ((f.n + 47) / 48);
    const bool wide_fits = feedback_lds_bytes<T, 64, 48, 64>(f.n2) <= size_t(160) * 1024;
    if (tile == 0) tile = (wide_groups >= 192 && wide_fits) ? 48 : 32;
    if (tile == 48 && wide_fits) return launch_feedback_ws<T, 48, 64>(f, st);
    return launch_feedback_tile<T, 32, 32, 32, 2>(f, 1, st);
}
template <typename T>
int feedback_force_impl(const crb_plan* p, const void* xs, const void* gain, const void* ref, void* u, void* stream) {
    FeedbackParams<T> f;
    f.xs = static_cast<const T*>(xs);
    f.ref = static_cast<const T*>(ref);
    f.gain = static_cast<const T*>(gain);
    f.u = static_cast<T*>(u);
    f.col_off = p->d_col_off;
    f.row_off = p->d_row_off;
    f.B = p->B; f.n = p->n_free; f.n2 = 2 * p->n_free;
    f.x_stride = size_t(2) * p->n_node * 4;
    f.u_stride = size_t(p->n_node) * 4;
    f.beam_idx = nullptr; f.ref_ld = 2 * p->n_free; f.ref_half = p->n_free;
    if (int rc = launch_feedback<T>(int(env_int("CRB_FEEDBACK_TILE", 0)), f, static_cast<hipStream_t>(stream))) return rc;
    HIP_TRY(hipGetLastError());
    return CRB_OK;
}
}  // namespace

extern "C" int crb_feedback_force(const crb_plan* p, const void* xs, const void* gain, const void* ref, void* u, void* stream) {
    if (int rc = need_device(p, "crb_feedback_force")) return rc;
    if (!xs || !gain || !u) return fail(CRB_EINVAL, "crb_feedback_force: null pointer");
    if (p->mixed_topology)
        return fail(CRB_EUNSUPPORTED, "crb_feedback_force: one gain matrix for the ensemble needs one free-DOF set (uniform boundary conditions / lengths)");
    return p->dtype == CRB_F64 ? feedback_force_impl<double>(p, xs, gain, ref, u, stream)
                               : feedback_force_impl<float>(p, xs, gain, ref, u, stream);
}

// ------------------------------------------------------------------ sampled-data state feedback in the implicit stepper
// crb_step_implicit_feedback: u_k = f_held + K (r - x) sampled every `hold` steps and held (zero-order hold), the chain of one
// crb_step_implicit call per sample.  In-kernel form (crb_stiff.h, FB): beams of one wave whose gain fits LDS, the whole call
// one launch.  Chain form: per sample one GEMM over the ensemble (crb_feedback_force) and one launch of the implicit stepper.
namespace {
// the gain fits LDS next to the exchange columns (the limit of fused_feedback_ok) and a beam lives in one wave
bool implicit_feedback_fits(const crb_plan* p) {
    return f64(p) && !p->mixed_topology && p->lognw == 0 && p->NT == 64 && crb::implicit_feedback_built(p->levels_full) &&
           crb::implicit_feedback_lds_bytes(p->NT, p->G, p->n_free) <= size_t(144) * 1024;
}
// CRB_IMPLICIT_FEEDBACK=0: the chain form; =1: the in-kernel form wherever the gain fits; unset: wherever it fits AND every
// workgroup of the launch is resident at once.  A workgroup is ONE wave at one wave per SIMD with its own copy of the gain: a
// CU holds min(4, 160 KB / LDS bytes) of them, and an ensemble that needs several rounds of workgroups is faster as a chain,
// whose steps run at the lean kernels' occupancy (hold = 1: 4096 x 30 elements, one workgroup per CU, 8 rounds, 78 against
// 23 us per sample; 512 x 30, resident, 10.2 against 14.1; 4096 x 10, 683 workgroups in one round, 4.9 against 11.2 --
// DESIGN.md section 10, which also names the case this rule loses: 16384 x 10 at hold <= 2)
bool implicit_feedback_in_kernel(const crb_plan* p) {
    if (!implicit_feedback_fits(p)) return false;
    if (const char* v = env("CRB_IMPLICIT_FEEDBACK")) return std::atoi(v) != 0;
    const size_t per_cu = (size_t(160) * 1024) / crb::implicit_feedback_lds_bytes(p->NT, p->G, p->n_free);
    return size_t(beam_groups(p)) <= 256 * (per_cu < 4 ? per_cu : 4);
}
StiffParams<double> stiff_params(const crb_plan* p, double h, int n_iter) {
    StiffParams<double> q{};
    q.a_levels = static_cast<const double*>(p->d_alevels);
    q.a_final = static_cast<const double*>(p->d_afinal);
    q.alv_stride = p->asm_in->nd > 1 ? size_t(p->levels_full) * p->S * PCR_LEVEL_VALS : 0;
    q.afin_stride = p->asm_in->nd > 1 ? size_t(p->S) * PCR_FINAL_VALS : 0;
    q.h = h;
    q.n_iter = n_iter;
    return q;
}
int implicit_feedback_fused(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, int hold, const void* gain,
                            const void* ref, const Forcing& f, const Recording& rec, void* u_out, hipStream_t st) {
#ifdef CRB_FAST_BUILD
    return fail(CRB_EUNSUPPORTED, "CRB_FAST_BUILD: implicit stepper not built");
#else
    if (int rc = ensure_red_map(p)) return rc;
    if (int rc = stiff_tables<double>(p, 0.25 * h * h, st)) return rc;
    KParams<double> k = base_params<double>(p);
    k.x = static_cast<double*>(x);
    set_io(k, f, &rec);
    k.t0 = t0; k.dt = h; k.n_steps = n_steps;
    arm_status(p, k, n_steps);
    k.red_map = p->d_red_map;
    k.n_red = p->n_free;
    k.fb_gain = static_cast<const double*>(gain);
    k.fb_ref = static_cast<const double*>(ref);
    // (the kernel writes the records of the thread-carried nodes: a dropped fixed node's entries read as zero)
    if (u_out)
        HIP_TRY(hipMemsetAsync(u_out, 0, size_t((n_steps + hold - 1) / hold) * force_doubles(p) * sizeof(double), st));
    StiffFbParams<double> q{};
    static_cast<StiffParams<double>&>(q) = stiff_params(p, h, n_iter);
    q.u_out = static_cast<double*>(u_out);
    q.hold = hold;
    const hipError_t e = crb::launch_implicit_feedback(k, q, p->stiff_levels, beam_groups(p),
                                                       crb::implicit_feedback_lds_bytes(p->NT, p->G, p->n_free), st);
    if (e != hipSuccess) return fail(CRB_EHIP, std::string("crb_step_implicit_feedback: ") + hipGetErrorString(e));
    return CRB_OK;
#endif
}
// The slice of a call's recording that the launch of one sample takes (steps s .. s + hs - 1 of the call): `every` divides hold
// (hs / every samples) or is a multiple of it (one sample at the end of every (every / hold)-th whole sample).  plane2: doubles
// of one whole-state snapshot.
Recording sample_recording(const Recording& rec, int s, int hs, int hold, size_t plane2) {
    Recording rs;
    if (!rec.out) return rs;
    long first = -1;
    if (hold % rec.every == 0) {
        if (hs / rec.every > 0) { rs = rec; first = s / rec.every; }
    } else if (hs == hold && (s + hold) % rec.every == 0) {
        rs = rec; rs.every = hold; first = (s + hold) / rec.every - 1;
    }
    if (first >= 0) rs.out = static_cast<double*>(rec.out) + size_t(first) * (rec.slot == REC_ALL_SLOTS ? plane2 : size_t(1));
    return rs;
}
// The controls of a sampled-data loop: record ks of the caller's u_out (one per sample), else the one record of the work buffer.
// Zeroed first: entries of a force record that the product does not write (constrained DOFs, the padding component) read as zero
double* control_record(const crb_plan* p, void* u_out, void* work, int ks) {
    return u_out ? static_cast<double*>(u_out) + size_t(ks) * force_doubles(p) : static_cast<double*>(work);
}
hipError_t zero_controls(const crb_plan* p, void* u_out, void* work, int n_steps, int hold, hipStream_t st) {
    const size_t records = u_out ? size_t((n_steps + hold - 1) / hold) : 1;
    return hipMemsetAsync(u_out ? u_out : work, 0, records * force_doubles(p) * sizeof(double), st);
}
// u_k = f_held + K (r - x) into the force record u (the product, then the held force), and in k the sample's launch: the call's
// forcing with u as its held input, the sample's slice of the recording
int sample_control(const crb_plan* p, KParams<double>& k, const void* x, const void* gain, const void* ref, const Forcing& f,
                   const Recording& rec, double* u, int s, int hs, int hold, hipStream_t st) {
    if (int rc = feedback_force_impl<double>(p, x, gain, ref, u, st)) return rc;
    if (f.held)
        HIP_TRY(crb::launch_feedback_held(u, static_cast<const double*>(f.held), p->d_row_off, p->n_free, p->B, size_t(p->n_node) * 4, st));
    const Recording rs = sample_recording(rec, s, hs, hold, state_doubles(p));
    set_io(k, f, &rs);
    k.u_held = u;
    return CRB_OK;
}
int implicit_feedback_chain(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, int hold, const void* gain,
                            const void* ref, const Forcing& f, const Recording& rec, void* u_out, void* work, hipStream_t st) {
    if (int rc = stiff_tables<double>(p, 0.25 * h * h, st)) return rc;
    const StiffParams<double> q = stiff_params(p, h, n_iter);
    HIP_TRY(zero_controls(p, u_out, work, n_steps, hold, st));
    // a beam that goes non-finite is marked with the step count at the end of the CALL, as the one launch of the other form does
    KParams<double> base = base_params<double>(p);
    arm_status(p, base, n_steps);
    base.x = static_cast<double*>(x); base.dt = h;
    return for_samples(n_steps, hold, t0, h, [&](int ks, int s, int hs, double t) -> int {
        KParams<double> k = base;
        if (int rc = sample_control(p, k, x, gain, ref, f, rec, control_record(p, u_out, work, ks), s, hs, hold, st)) return rc;
        k.t0 = t; k.n_steps = hs;
        return launch_implicit<double>(p, k, q, st);
    });
}
}  // namespace

extern "C" size_t crb_implicit_feedback_work_bytes(const crb_plan* p) {
    if (!p) return 0;
    return force_doubles(p) * sizeof(double);   // one force record (the chain form's held input)
}

extern "C" int crb_implicit_feedback_path(const crb_plan* p) {
    if (!p) return 0;
    return implicit_feedback_in_kernel(p) ? 1 : 0;
}

extern "C" int crb_step_implicit_feedback(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, int hold,
                                          const void* gain, const void* ref, const crb_input_desc* in, const crb_record_desc* rec,
                                          void* u_out, void* work, double* t_end, void* stream) {
    // every refusal before the device is touched, in the order of crb_step_implicit_sched: CRB_EINVAL, CRB_EUNSUPPORTED, CRB_ENODEV
    const std::string who("crb_step_implicit_feedback");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !gain || !work) return fail(CRB_EINVAL, who + ": null pointer");
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (!(h > 0)) return fail(CRB_EINVAL, who + ": h must be positive");
    if (n_iter < 1) return fail(CRB_EINVAL, who + ": n_iter must be >= 1");
    if (hold < 1) return fail(CRB_EINVAL, who + ": hold must be >= 1");
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, who.c_str(), &r)) return rc;
    if (rec && hold % rec->every != 0 && rec->every % hold != 0)
        return fail(CRB_EINVAL, who + ": the record stride must divide hold or be a multiple of it");
    Forcing f;
    if (int rc = decode_input(p, in, who.c_str(), &f)) return rc;
    if (p->dtype != CRB_F64)
        return fail(CRB_EUNSUPPORTED, who + ": the implicit stepper needs an fp64 plan (the iteration matrix is too ill-conditioned for fp32)");
    if (p->NT > 256) return fail(CRB_EUNSUPPORTED, who + ": beams of more than 256 thread-carried nodes are not supported");
    if (p->mixed_topology)
        return fail(CRB_EUNSUPPORTED, who + ": one gain matrix for the ensemble needs one free-DOF set (uniform boundary conditions / lengths)");
    if (int rc = need_device(p, who.c_str())) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (implicit_feedback_in_kernel(p)) return implicit_feedback_fused(p, x, t0, h, n_steps, n_iter, hold, gain, ref, f, r, u_out, st);
    return implicit_feedback_chain(p, x, t0, h, n_steps, n_iter, hold, gain, ref, f, r, u_out, work, st);
}

namespace {
void free_gain_groups(const crb_plan* p) {
    for (auto& g : p->gain_groups) {
        if (g.beam_idx) (void)hipFree(g.beam_idx);
        if (g.col) (void)hipFree(g.col);
        if (g.row) (void)hipFree(g.row);
    }
    p->gain_groups.clear();
    p->gain_group_key.clear();
}
// device tables for a beam -> group assignment: per group the list of its beams and the offsets of ITS reduced ordering
// inside the device layouts (the beams of a group must share the free-DOF set); cached for the assignment last used
int ensure_gain_groups(const crb_plan* p, int n_groups, const int32_t* beam_group) {
    std::vector<int32_t> key(beam_group, beam_group + p->B);
    key.push_back(n_groups);
    if (key == p->gain_group_key) return CRB_OK;
    free_gain_groups(p);
    std::vector<std::vector<int32_t>> members(static_cast<size_t>(n_groups));
    for (int b = 0; b < p->B; ++b) {
        const int g = beam_group[b];
        if (g >= n_groups) return fail(CRB_EINVAL, "crb_feedback_force_grouped: group index out of range");
        if (g >= 0) members[size_t(g)].push_back(b);
    }
    auto free_index_of = [&](int b) -> const std::vector<int32_t>& { return p->beam_free_index.empty() ? p->free_index : p->beam_free_index[size_t(b)]; };
    p->gain_groups.resize(static_cast<size_t>(n_groups));
    for (int g = 0; g < n_groups; ++g) {
        const auto& m = members[size_t(g)];
        crb_plan::GainGroup& G = p->gain_groups[size_t(g)];
        G.count = int(m.size());
        if (m.empty()) continue;
        const std::vector<int32_t>& fi = free_index_of(m[0]);
        for (int b : m)
            if (free_index_of(b) != fi) {
                free_gain_groups(p);
                return fail(CRB_EINVAL, "crb_feedback_force_grouped: the beams of a gain group must share one free-DOF set (boundary conditions and length)");
            }
        G.n = int(fi.size());
        std::vector<int32_t> col(size_t(2) * G.n), row(size_t(G.n));
        for (int r = 0; r < G.n; ++r) {
            row[r] = (fi[r] / 3) * 4 + (fi[r] % 3);
            col[r] = row[r];
            col[G.n + r] = p->n_node * 4 + row[r];
        }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&G.beam_idx), m.size() * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&G.col), col.size() * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&G.row), row.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(G.beam_idx, m.data(), m.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(G.col, col.data(), col.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(G.row, row.data(), row.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    p->gain_group_key = key;
    return CRB_OK;
}
template <typename T>
int feedback_force_grouped_impl(const crb_plan* p, const void* xs, int n_groups, const void* const* gains, const void* ref, void* u,
                                void* stream) {
    for (int g = 0; g < n_groups; ++g) {
        const crb_plan::GainGroup& G = p->gain_groups[size_t(g)];
        if (G.count == 0) continue;
        if (!gains[g]) return fail(CRB_EINVAL, "crb_feedback_force_grouped: null gain for a group that has beams");
        FeedbackParams<T> f;
        f.xs = static_cast<const T*>(xs);
        f.ref = static_cast<const T*>(ref);
        f.gain = static_cast<const T*>(gains[g]);
        f.u = static_cast<T*>(u);
        f.col_off = G.col;
        f.row_off = G.row;
        f.B = G.count; f.n = G.n; f.n2 = 2 * G.n;
        f.x_stride = size_t(2) * p->n_node * 4;
        f.u_stride = size_t(p->n_node) * 4;
        f.beam_idx = G.beam_idx; f.ref_ld = 2 * p->n_free; f.ref_half = p->n_free;
        if (int rc = launch_feedback<T>(int(env_int("CRB_FEEDBACK_TILE", 0)), f, static_cast<hipStream_t>(stream))) return rc;
        HIP_TRY(hipGetLastError());
    }
    return CRB_OK;
}
}  // namespace

extern "C" int crb_feedback_force_grouped(const crb_plan* p, const void* xs, int n_groups, const int32_t* beam_group,
                                          const void* const* gains, const void* ref, void* u, void* stream) {
    if (int rc = need_device(p, "crb_feedback_force_grouped")) return rc;
    if (!xs || !u || !beam_group || !gains || n_groups < 1) return fail(CRB_EINVAL, "crb_feedback_force_grouped: null pointer or no group");
    if (int rc = ensure_gain_groups(p, n_groups, beam_group)) return rc;
    return p->dtype == CRB_F64 ? feedback_force_grouped_impl<double>(p, xs, n_groups, gains, ref, u, stream)
                               : feedback_force_grouped_impl<float>(p, xs, n_groups, gains, ref, u, stream);
}

extern "C" int crb_step_rk4_feedback_grouped(const crb_plan* p, void* x, double t0, double dt, int n_steps, int n_groups,
                                             const int32_t* beam_group, const void* const* gains, const void* ref,
                                             const crb_input_desc* in, void* work, double* t_end, void* stream) {
    if (int rc = need_device(p, "crb_step_rk4_feedback_grouped")) return rc;
    if (!x || !work || !beam_group || !gains || n_groups < 1) return fail(CRB_EINVAL, "crb_step_rk4_feedback_grouped: null pointer or no group");
    if (n_steps < 0 || !(dt > 0)) return fail(CRB_EINVAL, "crb_step_rk4_feedback_grouped: n_steps >= 0 and dt > 0 required");
    if (int rc = ensure_gain_groups(p, n_groups, beam_group)) return rc;
    p->loop_used = false;
    Forcing f;
    if (int rc = decode_input(p, in, "crb_step_rk4_feedback_grouped", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    return feedback_rollout(p, x, t0, dt, n_steps, f, work, [&](const void* xs, void* u) {
        return crb_feedback_force_grouped(p, xs, n_groups, beam_group, gains, ref, u, stream);
    }, stream);
}

extern "C" int crb_rk4_stage(const crb_plan* p, void* x, const void* xs, void* acc, void* xs_next, const void* u_stage,
                             int stage, double t_stage, double dt, const crb_input_desc* in, void* stream) {
    if (int rc = need_device(p, "crb_rk4_stage")) return rc;
    if (!x || !xs || !acc) return fail(CRB_EINVAL, "crb_rk4_stage: null pointer");
    if (stage < 0 || stage > 3) return fail(CRB_EINVAL, "crb_rk4_stage: stage must be 0..3");
    if (stage < 3 && (!xs_next || xs_next == xs)) return fail(CRB_EINVAL, "crb_rk4_stage: xs_next must be a distinct buffer");
    if (!(dt > 0)) return fail(CRB_EINVAL, "crb_rk4_stage: dt must be positive");
    Forcing f;
    if (int rc = decode_input(p, in, "crb_rk4_stage", &f)) return rc;
    return rk4_stage(p, x, xs, acc, xs_next, u_stage, stage, t_stage, dt, f, stream);
}

extern "C" int crb_gather_dof(const crb_plan* p, const void* x, int plane, int node, int dof, void* out, void* stream) {
    if (int rc = need_device(p, "crb_gather_dof")) return rc;
    if (!x || !out) return fail(CRB_EINVAL, "crb_gather_dof: null pointer");
    if (plane < 0 || plane > 1 || node < 0 || node >= p->n_node || dof < 0 || dof > 2)
        return fail(CRB_EINVAL, "crb_gather_dof: index out of range");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t stride = size_t(2) * p->n_node * 4, off = (size_t(plane) * p->n_node + node) * 4 + dof;
    const int bs = 256, grid = (p->B + bs - 1) / bs;
    return with_dtype(p, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((crb_gather_kernel<T>), dim3(grid), dim3(bs), 0, st, static_cast<const T*>(x), stride, off, p->B, static_cast<T*>(out));
        HIP_TRY(hipGetLastError());
        return CRB_OK;
    });
}

// ------------------------------------------------------------------ static equilibrium, tangent stiffness (crb_static.h)
namespace {
// the tangent of a beam without a FIXED or PINNED node is singular (rigid translation): every node's u is free
bool beam_supported(const std::vector<int32_t>& free_index, int n_elem) {
    std::vector<uint8_t> u_free(size_t(n_elem) + 1, 0);
    for (const int32_t f : free_index)
        if (f % 3 == 0 && f / 3 <= n_elem) u_free[size_t(f / 3)] = 1;
    for (const uint8_t u : u_free)
        if (!u) return true;
    return false;
}
int static_checks(const crb_plan* p, const char* who) {
    if (int rc = need_device(p, who)) return rc;
    if (p->NT > STATIC_MAX_NT)
        return fail(CRB_EUNSUPPORTED, std::string(who) + ": beams of more than 256 thread-carried nodes are not supported");
    return CRB_OK;
}
template <typename T>
KParams<T> static_params(const crb_plan* p, const void* x) {
    KParams<T> k = base_params<T>(p);
    k.x = static_cast<T*>(const_cast<void*>(x));
    k.levels = p->levels_full;   // (the static solve runs every level of the reduction: J is not diagonally dominant)
    return k;
}
}  // namespace

extern "C" int crb_tangent_stiffness(const crb_plan* p, const void* x, void* out, void* stream) {
    if (int rc = static_checks(p, "crb_tangent_stiffness")) return rc;
    if (!x || !out) return fail(CRB_EINVAL, "crb_tangent_stiffness: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(p, [&](auto t) -> int {
        using T = decltype(t);
        StaticParams<T> q{};
        q.blocks = static_cast<T*>(out);
        HIP_TRY(crb::launch_tangent(static_params<T>(p, x), q, beam_groups(p), p->NT, st));
        return CRB_OK;
    });
}

extern "C" int crb_solve_static(const crb_plan* p, void* x, const crb_input_desc* in, int load_steps, int max_iter, double rtol,
                                double atol, int32_t* iters, void* residual, void* stream) {
    if (int rc = static_checks(p, "crb_solve_static")) return rc;
    if (p->dtype != CRB_F64)   // (the tangent's condition number reaches 1e7 at 10 elements and grows with the element count)
        return fail(CRB_EUNSUPPORTED, "crb_solve_static: the static solve needs an fp64 plan");
    if (!x || !iters) return fail(CRB_EINVAL, "crb_solve_static: null pointer");
    // (bounds of the per-beam work: at most 2^6 load_steps + 1 accepted increments, 7 attempts of max_iter + 1 evaluations
    //  between two of them -- crb_static.h)
    if (load_steps < 1 || load_steps > 4096) return fail(CRB_EINVAL, "crb_solve_static: load_steps must be in [1, 4096]");
    if (max_iter < 1 || max_iter > 1000) return fail(CRB_EINVAL, "crb_solve_static: max_iter must be in [1, 1000]");
    if (!(rtol >= 0.0) || !(atol >= 0.0)) return fail(CRB_EINVAL, "crb_solve_static: rtol and atol must be >= 0");
    Forcing f;
    if (int rc = decode_input(p, in, "crb_solve_static", &f)) return rc;
    if (f.impulse) return fail(CRB_EINVAL, "crb_solve_static: an impulse input has no static equilibrium (held forces only)");
    if (p->beam_free_index.empty()) {
        if (!beam_supported(p->free_index, p->n_elem))
            return fail(CRB_EINVAL, "crb_solve_static: the beams have no FIXED or PINNED node (singular tangent stiffness)");
    } else {
        for (size_t b = 0; b < p->beam_free_index.size(); ++b)
            if (!beam_supported(p->beam_free_index[b], p->beam_n_elem[b]))
                return fail(CRB_EINVAL, "crb_solve_static: beam " + std::to_string(b) +
                                            " has no FIXED or PINNED node (singular tangent stiffness)");
    }
    KParams<double> k = static_params<double>(p, x);
    set_io(k, f);
    StaticParams<double> q{};
    q.load_steps = load_steps;
    q.max_iter = max_iter;
    q.rtol = rtol;
    q.atol = atol;
    q.iters = iters;
    q.residual = static_cast<double*>(residual);
    HIP_TRY(crb::launch_static(k, q, beam_groups(p), p->NT, static_cast<hipStream_t>(stream)));
    return CRB_OK;
}

// ------------------------------------------------------------------ tangent-linear RHS and rollout (crb_tangent.h)
namespace {
int tangent_checks(const crb_plan* p, int n_dir, const char* who) {
    if (int rc = need_device(p, who)) return rc;
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, std::string(who) + ": the tangent kernels need an fp64 plan");
    if (p->NT > TANGENT_MAX_NT)
        return fail(CRB_EUNSUPPORTED, std::string(who) + ": beams of more than 256 thread-carried nodes are not supported");
    return check_count(who, "n_dir", n_dir);
}
// the input of a tangent rollout (CRB_EINVAL): the forcing, and the rule of its amplitude tangent
int tangent_input(const crb_plan* p, const crb_input_desc* in, const crb_input_tangent* din, const std::string& who, Forcing* f) {
    if (int rc = decode_input(p, in, who.c_str(), f)) return rc;
    if (din && din->d_amp && !f->impulse)
        return fail(CRB_EINVAL, who + ": d_amp needs an impulse input (its amplitude is what it differentiates)");
    return CRB_OK;
}
// The base of a tangent launch from the state x as it stands on the stream: the seeds dx, the amplitude tangents and x -- for
// more than one direction a copy of x, made here (instance d = 0 writes the base back while the others may still be loading it)
int tangent_base(const crb_plan* p, const void* x, void* dx, int n_dir, const crb_input_tangent* din, hipStream_t st,
                 TangentParams<double>* q) {
    *q = TangentParams<double>{};
    q->x0 = static_cast<const double*>(x);
    if (n_dir > 1) {
        const size_t bytes = state_doubles(p) * sizeof(double);
        if (!p->d_tan_x0) HIP_TRY(hipMalloc(&p->d_tan_x0, bytes));
        HIP_TRY(hipMemcpyAsync(p->d_tan_x0, x, bytes, hipMemcpyDeviceToDevice, st));
        q->x0 = static_cast<const double*>(p->d_tan_x0);
    }
    q->dx = static_cast<double*>(dx);
    if (din) q->d_amp = static_cast<const double*>(din->d_amp);
    return CRB_OK;
}
// What the two tangent rollouts share once the caller has put its family's tables and step size into k: the state, forcing,
// clock and status in k, the TangentParams -- tangent_base and the held force's tangents (with a schedule its tangent d_sched
// in df_held's place) -- and the family's launch(k, q).
template <typename L>
int tangent_rollout(const crb_plan* p, KParams<double> k, void* x, void* dx, int n_dir, double t0, int n_steps, const Forcing& f,
                    const crb_input_tangent* din, const Schedule& sc, const void* d_sched, hipStream_t st, L&& launch) {
    k.x = static_cast<double*>(x);
    set_io(k, f);
    k.t0 = t0; k.n_steps = n_steps;
    arm_status(p, k, n_steps);
    TangentParams<double> q;
    if (int rc = tangent_base(p, x, dx, n_dir, din, st, &q)) return rc;
    if (din) q.du_held = static_cast<const double*>(din->df_held);
    if (sc.f) {
        set_sched(p, k, sc, 0);
        q.du_held = static_cast<const double*>(d_sched);
        q.du_dir_stride = size_t(sc.K) * force_doubles(p);
    }
    HIP_TRY(launch(k, q));
    return CRB_OK;
}
}  // namespace

extern "C" int crb_rhs_jvp(const crb_plan* p, const void* x, const void* u, const void* dx, const void* du, int n_dir, void* xdot,
                           void* dxdot, void* stream) {
    if (int rc = tangent_checks(p, n_dir, "crb_rhs_jvp")) return rc;
    if (!x || !dx || !dxdot) return fail(CRB_EINVAL, "crb_rhs_jvp: null pointer");
    if (x == xdot || dx == dxdot) return fail(CRB_EINVAL, "crb_rhs_jvp: outputs must not alias inputs");
    KParams<double> k = base_params<double>(p);
    k.x = static_cast<double*>(const_cast<void*>(x));
    k.u_held = static_cast<const double*>(u);
    k.out = static_cast<double*>(xdot);
    TangentParams<double> q{};
    q.dx = static_cast<double*>(const_cast<void*>(dx));
    q.dxdot = static_cast<double*>(dxdot);
    q.du_held = static_cast<const double*>(du);
    HIP_TRY(crb::launch_jvp_rhs(k, q, beam_groups(p), n_dir, p->NT, static_cast<hipStream_t>(stream)));
    return CRB_OK;
}

extern "C" int crb_step_rk4_tangent(const crb_plan* p, void* x, void* dx, int n_dir, double t0, double dt, int n_steps,
                                    const crb_input_desc* in, const crb_input_tangent* din, double* t_end, void* stream) {
    return crb_step_rk4_tangent_sched(p, x, dx, n_dir, t0, dt, n_steps, in, din, nullptr, nullptr, t_end, stream);
}

extern "C" int crb_step_rk4_tangent_sched(const crb_plan* p, void* x, void* dx, int n_dir, double t0, double dt, int n_steps,
                                          const crb_input_desc* in, const crb_input_tangent* din, const crb_input_schedule* sched,
                                          const void* d_sched, double* t_end, void* stream) {
    Schedule sc;
    if (sched || d_sched) {   // (refused before the device is touched)
        const char* who = "crb_step_rk4_tangent_sched";
        if (!p) return fail(CRB_EINVAL, std::string(who) + ": null plan");
        if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, std::string(who) + ": the tangent kernels need an fp64 plan");
        if (!sched) return fail(CRB_EINVAL, std::string(who) + ": d_sched needs a schedule (sched is null)");
        if (int rc = decode_schedule(sched, in, n_steps, who, &sc)) return rc;
        if (din && din->df_held) return fail(CRB_EINVAL, std::string(who) + ": a schedule and dinput->df_held are given together");
    }
    if (int rc = tangent_checks(p, n_dir, "crb_step_rk4_tangent")) return rc;
    if (!x || !dx) return fail(CRB_EINVAL, "crb_step_rk4_tangent: null state or tangent");
    if (n_steps < 0) return fail(CRB_EINVAL, "crb_step_rk4_tangent: n_steps must be >= 0");
    if (!(dt > 0)) return fail(CRB_EINVAL, "crb_step_rk4_tangent: dt must be positive");
    Forcing f;
    if (int rc = tangent_input(p, in, din, "crb_step_rk4_tangent", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> k = base_params<double>(p);
    k.dt = dt;
    return tangent_rollout(p, k, x, dx, n_dir, t0, n_steps, f, din, sc, d_sched, st, [&](auto& kk, auto& q) {
        return crb::launch_jvp_step(kk, q, beam_groups(p), n_dir, p->NT, st);
    });
}

// ------------------------------------------------------------------ adjoint RHS and rollout (crb_adjoint.h)
namespace {
// The inverse lists of one gravity index table (crb_adjoint.h GravAdj): every forward edge once, in ascending order of the
// slot that reads it.  *seg_fanin / *phi_fanin: the largest fan-in found; false when one exceeds the kernels' lists.
bool grav_transpose(const std::vector<GravTab>& g, std::vector<GravAdj>& out, int* seg_fanin, int* phi_fanin) {
    const int S = int(g.size());
    GravAdj none;
    for (int m = 0; m < 2; ++m)
        for (int i = 0; i < GRAV_SEG_FANIN; ++i) none.seg[m][i] = -1;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < GRAV_PHI_FANIN; ++i) none.phi[c][i] = -1;
    out.assign(size_t(S), none);
    std::vector<int> ns(size_t(S) * 2, 0), np(size_t(S) * 3, 0);
    int ms = 0, mp = 0;
    for (int j = 0; j < S; ++j)   // node DOF (j, c) sums component comp[c] of segments segA[c], segB[c]
        for (int c = 0; c < 3; ++c) {
            const int segs[2] = {g[j].segA[c], g[j].segB[c]};
            for (int e = 0; e < 2; ++e) {
                const int sg = segs[e];
                if (sg < 0 || sg >= S) continue;
                const int m = g[j].comp[c] & 1;
                const int k = ns[size_t(sg) * 2 + m]++;
                ms = k + 1 > ms ? k + 1 : ms;
                if (k < GRAV_SEG_FANIN) out[sg].seg[m][k] = j * 4 + c;
            }
        }
    for (int sg = 0; sg < S; ++sg) {   // segment sg reads rotation phiA (weight 1, or 0.5 next to phiB) and phiB (0.5)
        const int ia = g[sg].phiA, ib = g[sg].phiB;
        const int idx[2] = {ia, ib};
        for (int e = 0; e < 2; ++e) {
            const int f = idx[e];
            if (f < 0 || (f >> 2) >= S || (f & 3) > 2) continue;
            const int j = f >> 2, c = f & 3;
            const int k = np[size_t(j) * 3 + c]++;
            mp = k + 1 > mp ? k + 1 : mp;
            if (k < GRAV_PHI_FANIN) out[j].phi[c][k] = (sg << 1) | (ib >= 0 ? 1 : 0);
        }
    }
    // (ascending order of the reading slot per list: the segment loop above visits segments in order)
    if (seg_fanin) *seg_fanin = ms;
    if (phi_fanin) *phi_fanin = mp;
    return ms <= GRAV_SEG_FANIN && mp <= GRAV_PHI_FANIN;
}

// the plan and size checks of every adjoint entry point, before the device is touched (so that they hold for host-only plans
// too; a valid call on a host-only plan then fails with CRB_ENODEV)
int adjoint_checks(const crb_plan* p, int n_cot, const char* who) {
    if (!p) return fail(CRB_EINVAL, std::string(who) + ": null plan");
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, std::string(who) + ": the adjoint kernels need an fp64 plan");
    if (p->NT > ADJ_MAX_NT)
        return fail(CRB_EUNSUPPORTED, std::string(who) + ": beams of more than 256 thread-carried nodes are not supported");
    return check_count(who, "n_cot", n_cot);
}

// the inverse gravity lists on the device (built and uploaded on first use; gravity-free plans need none)
int ensure_gadj(const crb_plan* p, const char* who) {
    if (!(p->flags & CRB_FORCE_GRAVITY) || p->d_gadj) return CRB_OK;
    const size_t S = size_t(p->S), nt = p->h_grav_topo.size();
    std::vector<GravAdj> all(nt * S), one;
    for (size_t t = 0; t < nt; ++t) {
        int ms = 0, mp = 0;
        if (!grav_transpose(p->h_grav_topo[t], one, &ms, &mp))
            return fail(CRB_EUNSUPPORTED, std::string(who) + ": the gravity index table has a fan-in of " + std::to_string(ms) +
                                              " / " + std::to_string(mp) + ", beyond the adjoint's lists");
        std::memcpy(&all[t * S], one.data(), S * sizeof(GravAdj));
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_gadj), all.size() * sizeof(GravAdj)));
    HIP_TRY(hipMemcpy(p->d_gadj, all.data(), all.size() * sizeof(GravAdj), hipMemcpyHostToDevice));
    if (!p->grav_topo_of.empty()) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_gadj_beam), p->grav_topo_of.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(p->d_gadj_beam, p->grav_topo_of.data(), p->grav_topo_of.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return CRB_OK;
}

AdjParams<double> adj_params(const crb_plan* p) {
    AdjParams<double> q = zeroed<AdjParams<double>>();
    q.gadj = p->d_gadj;
    q.gadj_beam = p->d_gadj_beam;
    q.store_every = 1;
    return q;
}
// the checkpoint pass: the state at the start of every segment of `every` steps into ckpt, the final state back into x
AdjParams<double> checkpoint_params(const crb_plan* p, void* ckpt, int every) {
    AdjParams<double> q = adj_params(p);
    q.states = static_cast<double*>(ckpt);
    q.store_every = every;
    q.write_back = 1;
    return q;
}
// the backward sweep over the segment of steps k0 .. k0 + n - 1: its recomputed data and clocks, lam in place, the input
// cotangents.  With a schedule f_bar is its cotangent [n_cot][K][B][n_node][4]: the sweep starts in the interval of the
// segment's last step and walks down (one accumulator: the interval's record).  The cotangent stride is set for every schedule,
// as the implicit sweep always did; the RK4 sweep left it 0 without an f_bar, where no kernel reads it (crb_adjoint.h fboff).
AdjParams<double> sweep_params(const crb_plan* p, const double* wstates, const double* wclock, void* lam, void* amp_bar, void* f_bar,
                               const Schedule& sc, int k0, int n) {
    AdjParams<double> b = adj_params(p);
    b.work = wstates;
    b.work_clock = wclock;
    b.lam = static_cast<double*>(lam);
    b.amp_bar = static_cast<double*>(amp_bar);
    b.f_bar = static_cast<double*>(f_bar);
    if (sc.f) {
        if (f_bar) b.f_bar += size_t((k0 + n - 1) / sc.hold) * force_doubles(p);
        b.fbar_cot_stride = size_t(sc.K) * force_doubles(p);
    }
    b.step0 = k0;
    return b;
}
}  // namespace

extern "C" int crb_plan_get_grav_transpose(const crb_plan* p, int beam, int32_t* seg, int32_t* phi, int32_t* fanin) {
    if (!p) return fail(CRB_EINVAL, "crb_plan_get_grav_transpose: null plan");
    if (beam < 0 || beam >= p->B) return fail(CRB_EINVAL, "crb_plan_get_grav_transpose: beam out of range");
    const size_t t = p->grav_topo_of.empty() ? 0 : size_t(p->grav_topo_of[size_t(beam)]);
    std::vector<GravAdj> lists;
    int ms = 0, mp = 0;
    const bool ok = grav_transpose(p->h_grav_topo[t], lists, &ms, &mp);
    if (fanin) { fanin[0] = ms; fanin[1] = mp; }
    for (int j = 0; j < p->S; ++j) {
        if (seg)
            for (int m = 0; m < 2; ++m)
                for (int i = 0; i < GRAV_SEG_FANIN; ++i) seg[(size_t(j) * 2 + m) * GRAV_SEG_FANIN + i] = lists[j].seg[m][i];
        if (phi)
            for (int c = 0; c < 3; ++c)
                for (int i = 0; i < GRAV_PHI_FANIN; ++i) phi[(size_t(j) * 3 + c) * GRAV_PHI_FANIN + i] = lists[j].phi[c][i];
    }
    return ok ? CRB_OK : fail(CRB_EUNSUPPORTED, "crb_plan_get_grav_transpose: fan-in beyond the adjoint's lists");
}

extern "C" int crb_rhs_vjp(const crb_plan* p, const void* x, const void* u, const void* lam, int n_cot, void* xdot, void* xbar,
                           void* ubar, void* stream) {
    if (int rc = adjoint_checks(p, n_cot, "crb_rhs_vjp")) return rc;
    if (!x || !lam || !xbar) return fail(CRB_EINVAL, "crb_rhs_vjp: null pointer");
    if (xbar == x || xbar == lam || xbar == u || (xdot && (xdot == x || xdot == lam || xdot == xbar)) ||
        (ubar && (ubar == x || ubar == lam || ubar == u || ubar == xbar)))
        return fail(CRB_EINVAL, "crb_rhs_vjp: outputs must not alias inputs or each other");
    if (int rc = need_device(p, "crb_rhs_vjp")) return rc;
    if (int rc = ensure_gadj(p, "crb_rhs_vjp")) return rc;
    KParams<double> k = base_params<double>(p);
    k.x = static_cast<double*>(const_cast<void*>(x));
    k.u_held = static_cast<const double*>(u);
    k.out = static_cast<double*>(xdot);
    AdjParams<double> q = adj_params(p);
    q.lam_in = static_cast<const double*>(lam);
    q.xbar = static_cast<double*>(xbar);
    q.ubar = static_cast<double*>(ubar);
    HIP_TRY(crb::launch_adj_rhs(k, q, beam_groups(p), n_cot, p->NT, static_cast<hipStream_t>(stream)));
    return CRB_OK;
}

namespace {
// The work buffer of the RK4 adjoint, in doubles: a segment's stage points [every][4] states, its clocks [every], and with
// parameter gradients (crb_rk4_adjoint_params_work_bytes) the sweep's per-stage rbar, [every][4][n_cot] force records.
struct AdjWork { double *states, *clock, *rbar; };
AdjWork adj_work(const crb_plan* p, void* work, int every) {
    double* const states = static_cast<double*>(work), * const clock = states + size_t(every) * 4 * state_doubles(p);
    return {states, clock, clock + size_t(every)};
}
}  // namespace

extern "C" size_t crb_rk4_adjoint_work_bytes(const crb_plan* p, int every) {
    if (!p || every < 1) return 0;
    return size_t(every) * (4 * state_doubles(p) + 1) * sizeof(double);
}

extern "C" int crb_step_rk4_checkpoint(const crb_plan* p, void* x, double t0, double dt, int n_steps, int every,
                                       const crb_input_desc* in, const crb_record_desc* rec, void* ckpt, double* t_end,
                                       void* stream) {
    return crb_step_rk4_checkpoint_sched(p, x, t0, dt, n_steps, every, in, nullptr, rec, ckpt, t_end, stream);
}

extern "C" int crb_step_rk4_checkpoint_sched(const crb_plan* p, void* x, double t0, double dt, int n_steps, int every,
                                             const crb_input_desc* in, const crb_input_schedule* sched,
                                             const crb_record_desc* rec, void* ckpt, double* t_end, void* stream) {
    if (int rc = adjoint_checks(p, 1, "crb_step_rk4_checkpoint")) return rc;
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, "crb_step_rk4_checkpoint_sched", &sc)) return rc;
    if (!x || !ckpt) return fail(CRB_EINVAL, "crb_step_rk4_checkpoint: null state or checkpoint buffer");
    if (x == ckpt) return fail(CRB_EINVAL, "crb_step_rk4_checkpoint: the checkpoint buffer must not alias the state");
    if (n_steps < 0) return fail(CRB_EINVAL, "crb_step_rk4_checkpoint: n_steps must be >= 0");
    if (every < 1) return fail(CRB_EINVAL, "crb_step_rk4_checkpoint: every must be >= 1");
    if (!(dt > 0)) return fail(CRB_EINVAL, "crb_step_rk4_checkpoint: dt must be positive");
    if (int rc = need_device(p, "crb_step_rk4_checkpoint")) return rc;
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, "crb_step_rk4_checkpoint", &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, "crb_step_rk4_checkpoint", &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, "crb_step_rk4_checkpoint")) return rc;
    KParams<double> k = base_params<double>(p);
    k.x = static_cast<double*>(x);
    set_io(k, f, &r);
    set_sched(p, k, sc, 0);
    k.t0 = t0; k.dt = dt; k.n_steps = n_steps;
    HIP_TRY(crb::launch_adj_forward(k, checkpoint_params(p, ckpt, every), beam_groups(p), p->NT, static_cast<hipStream_t>(stream)));
    return CRB_OK;
}

namespace {
// crb_step_rk4_adjoint and crb_step_rk4_adjoint_params (want_params): the same segments and launches, the
// latter with the storing sweep and crb_param_grad_kernel after each
int adjoint_rollout(const char* who_c, const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt, int n_steps,
                    int every, const crb_input_desc* in, const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                    bool want_params, const crb_param_cotangent* pgrad, const crb_input_schedule* sched, void* sched_bar,
                    void* work, void* stream) {
    const std::string who(who_c);
    if (int rc = adjoint_checks(p, n_cot, who_c)) return rc;
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, who_c, &sc)) return rc;
    if (sched_bar && !sc.f) return fail(CRB_EINVAL, who + ": sched_bar needs a schedule (sched is null)");
    if (sc.f && grad && grad->f_held_bar)
        return fail(CRB_EINVAL, who + ": a schedule and grad->f_held_bar are given together (sched_bar takes its place)");
    if (sched_bar && (sched_bar == lam || sched_bar == work || sched_bar == ckpt || sched_bar == sc.f))
        return fail(CRB_EINVAL, who + ": sched_bar must not alias lam, the work buffer, the checkpoints or f_sched");
    if (!ckpt || !lam) return fail(CRB_EINVAL, who + ": null checkpoint buffer or cotangent");
    if (want_params && (!pgrad || !pgrad->param_bar))
        return fail(CRB_EINVAL, who + ": null parameter cotangent (crb_param_cotangent.param_bar)");
    if (!work) return fail(CRB_EINVAL, who + (want_params ? ": null work buffer (crb_rk4_adjoint_params_work_bytes)"
                                                             : ": null work buffer (crb_rk4_adjoint_work_bytes)"));
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (every < 1) return fail(CRB_EINVAL, who + ": every must be >= 1");
    if (!(dt > 0)) return fail(CRB_EINVAL, who + ": dt must be positive");
    if (lam == ckpt || lam == work) return fail(CRB_EINVAL, who + ": lam must not alias another buffer of the call");
    void* const param_bar = want_params ? pgrad->param_bar : nullptr;
    if (param_bar && (param_bar == lam || param_bar == work || param_bar == ckpt))
        return fail(CRB_EINVAL, who + ": param_bar must not alias lam, the work buffer or the checkpoints");
    if (int rc = need_device(p, who_c)) return rc;
    Recording r;
    if (int rc = decode_record(p, rec_bar, n_steps, true, who_c, &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who_c, &f)) return rc;
    void* amp_bar = grad ? grad->amp_bar : nullptr;
    void* f_bar = sc.f ? sched_bar : (grad ? grad->f_held_bar : nullptr);   // (one accumulator in the sweep: the interval's record)
    if (amp_bar && !f.impulse)
        return fail(CRB_EINVAL, who + ": amp_bar needs an impulse input (its amplitude is what it differentiates)");
    const void* bufs[7] = {ckpt, work, amp_bar, f_bar, r.out, f.held, sc.f};
    for (const void* b : bufs)
        if (b && b == lam) return fail(CRB_EINVAL, who + ": lam must not alias another buffer of the call");
    if ((amp_bar && (amp_bar == work || amp_bar == ckpt || amp_bar == f_bar)) || (f_bar && (f_bar == work || f_bar == ckpt)) ||
        work == ckpt || (sc.f && (sc.f == work || sc.f == amp_bar || sc.f == param_bar)) ||
        (param_bar && (param_bar == amp_bar || param_bar == f_bar || param_bar == r.out || param_bar == f.held)))
        return fail(CRB_EINVAL, who + ": the output and work buffers must not alias each other or the checkpoints");
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who_c)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int groups = beam_groups(p);
    const AdjWork w = adj_work(p, work, every);
    return for_segments_reversed(n_steps, every, t0, dt, [&](int g, int k0, int n, double tg) -> int {
        KParams<double> k = base_params<double>(p);
        set_io(k, f);
        set_sched(p, k, sc, k0);   // (the recompute starts mid-rollout: its interval and phase)
        k.dt = dt; k.t0 = tg; k.n_steps = n;
        // 1. the segment's stage points from its checkpoint
        k.x = const_cast<double*>(static_cast<const double*>(ckpt)) + size_t(g) * state_doubles(p);
        AdjParams<double> q = adj_params(p);
        q.states = w.states;
        q.clocks = w.clock;
        q.stage_pts = 1;
        HIP_TRY(crb::launch_adj_forward(k, q, groups, p->NT, st));
        // 2. the sweep back over it, every cotangent
        k.x = nullptr;
        set_record(k, r);
        AdjParams<double> b = sweep_params(p, w.states, w.clock, lam, amp_bar, f_bar, sc, k0, n);
        if (!want_params) {
            HIP_TRY(crb::launch_adj_backward(k, b, groups, n_cot, p->NT, st));
            return CRB_OK;
        }
        b.rbar = w.rbar;
        b.param_bar = static_cast<double*>(param_bar);
        HIP_TRY(crb::launch_adj_backward_store(k, b, groups, n_cot, p->NT, st));
        // 3. the parameter sums of the segment, from its stage points and the sweep's rbar
        HIP_TRY(crb::launch_param_grad(k, b, groups, n_cot, p->NT, st));
        return CRB_OK;
    });
}
}  // namespace

extern "C" int crb_step_rk4_adjoint(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt, int n_steps,
                                    int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                                    const crb_input_cotangent* grad, void* work, void* stream) {
    return adjoint_rollout("crb_step_rk4_adjoint", p, ckpt, lam, n_cot, t0, dt, n_steps, every, in, rec_bar, grad, false, nullptr,
                           nullptr, nullptr, work, stream);
}

extern "C" int crb_step_rk4_adjoint_sched(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                          int n_steps, int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                                          const crb_input_cotangent* grad, const crb_input_schedule* sched, void* sched_bar,
                                          void* work, void* stream) {
    return adjoint_rollout(sched ? "crb_step_rk4_adjoint_sched" : "crb_step_rk4_adjoint", p, ckpt, lam, n_cot, t0, dt, n_steps,
                           every, in, rec_bar, grad, false, nullptr, sched, sched_bar, work, stream);
}

extern "C" size_t crb_rk4_adjoint_params_work_bytes(const crb_plan* p, int every, int n_cot) {
    if (!p || every < 1 || n_cot < 1) return 0;
    return crb_rk4_adjoint_work_bytes(p, every) + size_t(every) * 4 * size_t(n_cot) * force_doubles(p) * sizeof(double);
}

extern "C" int crb_step_rk4_adjoint_params(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                           int n_steps, int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                                           const crb_input_cotangent* grad, const crb_param_cotangent* pgrad, void* work,
                                           void* stream) {
    return adjoint_rollout("crb_step_rk4_adjoint_params", p, ckpt, lam, n_cot, t0, dt, n_steps, every, in, rec_bar, grad, true,
                           pgrad, nullptr, nullptr, work, stream);
}

extern "C" int crb_step_rk4_adjoint_params_sched(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                                 int n_steps, int every, const crb_input_desc* in,
                                                 const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                                 const crb_param_cotangent* pgrad, const crb_input_schedule* sched,
                                                 void* sched_bar, void* work, void* stream) {
    return adjoint_rollout(sched ? "crb_step_rk4_adjoint_params_sched" : "crb_step_rk4_adjoint_params", p, ckpt, lam, n_cot, t0,
                           dt, n_steps, every, in, rec_bar, grad, true, pgrad, sched, sched_bar, work, stream);
}

// ---- adjoint of the implicit stepper (crb_implicit_adjoint.h)
namespace {
constexpr int IMP_ADJ_MAX_ITER = 16;
// the argument checks the two implicit-adjoint entry points share, in the documented order: CRB_EINVAL first (the caller adds
// its own pointer and aliasing checks before this), then imp_adjoint_plan_checks
int imp_adjoint_arg_checks(const std::string& who, int n_cot, int n_steps, int every, int n_iter, double h) {
    if (int rc = check_count(who, "n_cot", n_cot)) return rc;
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (every < 1) return fail(CRB_EINVAL, who + ": every must be >= 1");
    if (n_iter < 1 || n_iter > IMP_ADJ_MAX_ITER) return fail(CRB_EINVAL, who + ": n_iter must be in [1, 16]");
    if (!(h > 0)) return fail(CRB_EINVAL, who + ": h must be positive");
    return CRB_OK;
}
int imp_adjoint_plan_checks(const crb_plan* p, const std::string& who) {
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, who + ": the adjoint of the implicit stepper needs an fp64 plan");
    if (p->NT > ADJ_MAX_NT) return fail(CRB_EUNSUPPORTED, who + ": beams of more than 256 thread-carried nodes are not supported");
    return CRB_OK;
}
// their siblings of the two implicit-tangent entry points: the caller's own CRB_EINVAL cases and tangent_input lie between them
int imp_tangent_arg_checks(const std::string& who, int n_dir, int n_steps, int n_iter, double h) {
    if (int rc = check_count(who, "n_dir", n_dir)) return rc;
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (n_iter < 1 || n_iter > IMP_ADJ_MAX_ITER) return fail(CRB_EINVAL, who + ": n_iter must be in [1, 16]");
    if (!(h > 0)) return fail(CRB_EINVAL, who + ": h must be positive");
    return CRB_OK;
}
int imp_tangent_plan_checks(const crb_plan* p, const std::string& who) {
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, who + ": the tangent of the implicit stepper needs an fp64 plan");
    if (p->NT > TANGENT_MAX_NT) return fail(CRB_EUNSUPPORTED, who + ": beams of more than 256 thread-carried nodes are not supported");
    return CRB_OK;
}
// the launch parameters of the implicit adjoint kernels: A's tables (stiff_tables, for alpha = h^2 / 4) where M's are
int imp_adjoint_params(const crb_plan* p, double h, hipStream_t st, KParams<double>* k) {
    if (int rc = stiff_tables<double>(p, 0.25 * h * h, st)) return rc;
    *k = base_params<double>(p);
    const bool per_beam = p->asm_in->nd > 1;
    k->pcr_levels = static_cast<const double*>(p->d_alevels);
    k->pcr_final = static_cast<const double*>(p->d_afinal);
    k->lv_stride = per_beam ? size_t(p->levels_full) * p->S * PCR_LEVEL_VALS : 0;
    k->fin_stride = per_beam ? size_t(p->S) * PCR_FINAL_VALS : 0;
    k->levels = p->stiff_levels;
    k->dt = h;
    return CRB_OK;
}
// The work buffer of the implicit adjoint, in doubles: a segment's step start states [every], iterates [every][n_iter] force
// records and clocks [every], and the cotangent carried through the starting iterate from one segment to the one before it,
// [n_cot] force records.  With parameter gradients (crb_implicit_adjoint_params_work_bytes) the sweep's per-iteration gbar,
// [every][n_iter][n_cot] force records, and the final iterate of the segment's last step, one force record.
struct ImpAdjWork { double *states, *iters, *clock, *carry, *gbar, *fin; };
ImpAdjWork imp_adj_work(const crb_plan* p, void* work, int every, int n_iter, int n_cot) {
    double* const states = static_cast<double*>(work), * const iters = states + size_t(every) * state_doubles(p);
    double* const clock = iters + size_t(every) * size_t(n_iter) * force_doubles(p);
    double* const carry = clock + size_t(every), * const gbar = carry + size_t(n_cot) * force_doubles(p);
    return {states, iters, clock, carry, gbar, gbar + size_t(every) * size_t(n_iter) * size_t(n_cot) * force_doubles(p)};
}
int imp_adjoint_rollout(const std::string& who, const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h,
                        int n_steps, int n_iter, int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                        const crb_input_cotangent* grad, bool want_params, const crb_param_cotangent* pgrad,
                        const crb_input_schedule* sched, void* sched_bar, void* work, void* stream);
}  // namespace

extern "C" size_t crb_implicit_adjoint_work_bytes(const crb_plan* p, int every, int n_iter, int n_cot) {
    if (!p || every < 1 || n_iter < 1 || n_iter > IMP_ADJ_MAX_ITER || n_cot < 1 || n_cot > 65535) return 0;
    return (size_t(every) * ((2 + size_t(n_iter)) * force_doubles(p) + 1) + size_t(n_cot) * force_doubles(p)) * sizeof(double);
}

extern "C" int crb_step_implicit_checkpoint(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter, int every,
                                            const crb_input_desc* in, const crb_record_desc* rec, void* ckpt, double* t_end,
                                            void* stream) {
    return crb_step_implicit_checkpoint_sched(p, x, t0, h, n_steps, n_iter, every, in, nullptr, rec, ckpt, t_end, stream);
}

extern "C" int crb_step_implicit_checkpoint_sched(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter,
                                                  int every, const crb_input_desc* in, const crb_input_schedule* sched,
                                                  const crb_record_desc* rec, void* ckpt, double* t_end, void* stream) {
    const std::string who(sched ? "crb_step_implicit_checkpoint_sched" : "crb_step_implicit_checkpoint");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !ckpt) return fail(CRB_EINVAL, who + ": null state or checkpoint buffer");
    if (x == ckpt) return fail(CRB_EINVAL, who + ": the checkpoint buffer must not alias the state");
    if (int rc = imp_adjoint_arg_checks(who, 1, n_steps, every, n_iter, h)) return rc;
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, who.c_str(), &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who.c_str(), &f)) return rc;
    if (r.out && (r.out == x || r.out == ckpt)) return fail(CRB_EINVAL, who + ": the record must not alias the state or the checkpoints");
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, who.c_str(), &sc)) return rc;
    if (int rc = imp_adjoint_plan_checks(p, who)) return rc;
    if (int rc = need_device(p, who.c_str())) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> k;
    if (int rc = imp_adjoint_params(p, h, st, &k)) return rc;
    k.x = static_cast<double*>(x);
    set_io(k, f, &r);
    set_sched(p, k, sc, 0);
    k.t0 = t0; k.n_steps = n_steps;
    ImpAdjParams<double> iq = zeroed<ImpAdjParams<double>>();
    iq.n_iter = n_iter;
    HIP_TRY(crb::launch_imp_adj_checkpoint(k, checkpoint_params(p, ckpt, every), iq, beam_groups(p), p->NT, st));
    return CRB_OK;
}

extern "C" int crb_step_implicit_adjoint(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h, int n_steps,
                                         int n_iter, int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                                         const crb_input_cotangent* grad, void* work, void* stream) {
    return crb_step_implicit_adjoint_sched(p, ckpt, lam, n_cot, t0, h, n_steps, n_iter, every, in, rec_bar, grad, nullptr, nullptr,
                                           work, stream);
}

extern "C" int crb_step_implicit_adjoint_sched(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h,
                                               int n_steps, int n_iter, int every, const crb_input_desc* in,
                                               const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                               const crb_input_schedule* sched, void* sched_bar, void* work, void* stream) {
    return imp_adjoint_rollout(sched ? "crb_step_implicit_adjoint_sched" : "crb_step_implicit_adjoint", p, ckpt, lam, n_cot, t0, h,
                               n_steps, n_iter, every, in, rec_bar, grad, false, nullptr, sched, sched_bar, work, stream);
}

extern "C" size_t crb_implicit_adjoint_params_work_bytes(const crb_plan* p, int every, int n_iter, int n_cot) {
    const size_t plain = crb_implicit_adjoint_work_bytes(p, every, n_iter, n_cot);
    if (!plain) return 0;
    return plain + (size_t(every) * size_t(n_iter) * size_t(n_cot) + 1) * force_doubles(p) * sizeof(double);
}

extern "C" int crb_step_implicit_adjoint_params(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h,
                                                int n_steps, int n_iter, int every, const crb_input_desc* in,
                                                const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                                const crb_param_cotangent* pgrad, void* work, void* stream) {
    return imp_adjoint_rollout("crb_step_implicit_adjoint_params", p, ckpt, lam, n_cot, t0, h, n_steps, n_iter, every, in, rec_bar,
                               grad, true, pgrad, nullptr, nullptr, work, stream);
}

extern "C" int crb_step_implicit_adjoint_params_sched(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h,
                                                      int n_steps, int n_iter, int every, const crb_input_desc* in,
                                                      const crb_record_desc* rec_bar, const crb_input_cotangent* grad,
                                                      const crb_param_cotangent* pgrad, const crb_input_schedule* sched,
                                                      void* sched_bar, void* work, void* stream) {
    return imp_adjoint_rollout(sched ? "crb_step_implicit_adjoint_params_sched" : "crb_step_implicit_adjoint_params", p, ckpt, lam,
                               n_cot, t0, h, n_steps, n_iter, every, in, rec_bar, grad, true, pgrad, sched, sched_bar, work, stream);
}

namespace {
// crb_step_implicit_adjoint(_sched) and crb_step_implicit_adjoint_params(_sched) (want_params): the same segments and launches,
// the latter with the recompute that keeps the last final iterate, the storing sweep and crb_imp_param_grad_kernel after each
int imp_adjoint_rollout(const std::string& who, const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double h,
                        int n_steps, int n_iter, int every, const crb_input_desc* in, const crb_record_desc* rec_bar,
                        const crb_input_cotangent* grad, bool want_params, const crb_param_cotangent* pgrad,
                        const crb_input_schedule* sched, void* sched_bar, void* work, void* stream) {
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!ckpt || !lam) return fail(CRB_EINVAL, who + ": null checkpoint buffer or cotangent");
    if (want_params && (!pgrad || !pgrad->param_bar))
        return fail(CRB_EINVAL, who + ": null parameter cotangent (crb_param_cotangent.param_bar)");
    if (!work) return fail(CRB_EINVAL, who + (want_params ? ": null work buffer (crb_implicit_adjoint_params_work_bytes)"
                                                             : ": null work buffer (crb_implicit_adjoint_work_bytes)"));
    void* const param_bar = want_params ? pgrad->param_bar : nullptr;
    void* const amp_bar = grad ? grad->amp_bar : nullptr;
    void* f_bar = grad ? grad->f_held_bar : nullptr;
    const void* const rec_out = rec_bar ? rec_bar->out : nullptr;
    const void* const held = in ? in->f_held : nullptr;
    const void* bufs[6] = {ckpt, work, amp_bar, f_bar, rec_out, held};
    for (const void* b : bufs)
        if (b && b == lam) return fail(CRB_EINVAL, who + ": lam must not alias another buffer of the call");
    if (param_bar && (param_bar == lam || param_bar == work || param_bar == ckpt))
        return fail(CRB_EINVAL, who + ": param_bar must not alias lam, the work buffer or the checkpoints");
    if (work == ckpt || (amp_bar && (amp_bar == work || amp_bar == ckpt || amp_bar == f_bar)) ||
        (f_bar && (f_bar == work || f_bar == ckpt)) ||
        (param_bar && (param_bar == amp_bar || param_bar == f_bar || param_bar == rec_out || param_bar == held)))
        return fail(CRB_EINVAL, who + ": the output and work buffers must not alias each other or the checkpoints");
    if (int rc = imp_adjoint_arg_checks(who, n_cot, n_steps, every, n_iter, h)) return rc;
    Recording r;
    if (int rc = decode_record(p, rec_bar, n_steps, true, who.c_str(), &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who.c_str(), &f)) return rc;
    if (amp_bar && !f.impulse)
        return fail(CRB_EINVAL, who + ": amp_bar needs an impulse input (its amplitude is what it differentiates)");
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, who.c_str(), &sc)) return rc;
    if (sc.f && f_bar)
        return fail(CRB_EINVAL, who + ": a schedule and grad->f_held_bar are given together (sched_bar takes its place)");
    if (sched_bar && !sc.f) return fail(CRB_EINVAL, who + ": sched_bar needs a schedule (sched is null)");
    if (sched_bar && (sched_bar == lam || sched_bar == work || sched_bar == ckpt || sched_bar == sc.f || sched_bar == amp_bar))
        return fail(CRB_EINVAL, who + ": sched_bar must not alias lam, the work buffer, the checkpoints, f_sched or amp_bar");
    if (param_bar && (param_bar == sched_bar || param_bar == sc.f))
        return fail(CRB_EINVAL, who + ": param_bar must not alias the schedule or its cotangent");
    if (sc.f) f_bar = sched_bar;   // (one accumulator in the sweep: the interval's record)
    if (int rc = imp_adjoint_plan_checks(p, who)) return rc;
    if (int rc = need_device(p, who.c_str())) return rc;
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> base;
    if (int rc = imp_adjoint_params(p, h, st, &base)) return rc;
    set_io(base, f);
    const ImpAdjWork w = imp_adj_work(p, work, every, n_iter, n_cot);
    ImpAdjParams<double> iter = zeroed<ImpAdjParams<double>>();
    iter.n_iter = n_iter;
    const int groups = beam_groups(p);
    return for_segments_reversed(n_steps, every, t0, h, [&](int g, int k0, int n, double tg) -> int {
        KParams<double> k = base;
        k.t0 = tg;
        k.n_steps = n;
        set_sched(p, k, sc, k0);   // (the recompute starts mid-rollout: its interval and phase)
        // 1. the segment's step data from its checkpoint
        AdjParams<double> q = adj_params(p);
        q.states = w.states;
        q.clocks = w.clock;
        ImpAdjParams<double> iq = iter;
        iq.start = static_cast<const double*>(ckpt) + size_t(g) * 3 * force_doubles(p);
        iq.iters_out = w.iters;
        if (want_params) {
            iq.fin_out = w.fin;
            HIP_TRY(crb::launch_imp_adj_segment_final(k, q, iq, groups, p->NT, st));
        } else {
            HIP_TRY(crb::launch_imp_adj_segment(k, q, iq, groups, p->NT, st));
        }
        // 2. the sweep back over it, every cotangent
        set_record(k, r);
        ImpAdjParams<double> ib = iter;
        ib.iters = w.iters;
        ib.carry = w.carry;
        ib.carry_in = k0 + n < n_steps ? 1 : 0;   // (every segment but the one that ends the rollout)
        AdjParams<double> b = sweep_params(p, w.states, w.clock, lam, amp_bar, f_bar, sc, k0, n);
        if (!want_params) {
            HIP_TRY(crb::launch_imp_adj_backward(k, b, ib, groups, n_cot, p->NT, st));
            return CRB_OK;
        }
        ib.gbar = w.gbar;
        ib.fin_out = w.fin;
        b.param_bar = static_cast<double*>(param_bar);
        HIP_TRY(crb::launch_imp_adj_backward_store(k, b, ib, groups, n_cot, p->NT, st));
        // 3. the parameter sums of the segment, from its step data and the sweep's gbar
        HIP_TRY(crb::launch_imp_param_grad(k, b, ib, groups, n_cot, p->NT, st));
        return CRB_OK;
    });
}
}  // namespace

// ---- tangent of the implicit stepper (crb_implicit_tangent.h)
extern "C" int crb_step_implicit_tangent(const crb_plan* p, void* x, void* dx, int n_dir, double t0, double h, int n_steps, int n_iter,
                                         const crb_input_desc* in, const crb_input_tangent* din, double* t_end, void* stream) {
    return crb_step_implicit_tangent_sched(p, x, dx, n_dir, t0, h, n_steps, n_iter, in, din, nullptr, nullptr, t_end, stream);
}

extern "C" int crb_step_implicit_tangent_sched(const crb_plan* p, void* x, void* dx, int n_dir, double t0, double h, int n_steps,
                                               int n_iter, const crb_input_desc* in, const crb_input_tangent* din,
                                               const crb_input_schedule* sched, const void* d_sched, double* t_end, void* stream) {
    // every refusal before the device is touched, in the order the implicit adjoint documents: CRB_EINVAL (the call's own cases,
    // then the schedule's), CRB_EUNSUPPORTED, CRB_ENODEV
    const std::string who(sched || d_sched ? "crb_step_implicit_tangent_sched" : "crb_step_implicit_tangent");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !dx) return fail(CRB_EINVAL, who + ": null state or tangent");
    if (int rc = imp_tangent_arg_checks(who, n_dir, n_steps, n_iter, h)) return rc;
    Forcing f;
    if (int rc = tangent_input(p, in, din, who, &f)) return rc;
    if (d_sched && !sched) return fail(CRB_EINVAL, who + ": d_sched needs a schedule (sched is null)");
    Schedule sc;
    if (int rc = decode_schedule(sched, in, n_steps, who.c_str(), &sc)) return rc;
    if (sc.f && din && din->df_held) return fail(CRB_EINVAL, who + ": a schedule and dinput->df_held are given together");
    if (int rc = imp_tangent_plan_checks(p, who)) return rc;
    if (int rc = need_device(p, who.c_str())) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> k;
    if (int rc = imp_adjoint_params(p, h, st, &k)) return rc;   // (A's tables where M's are, k.dt = h)
    return tangent_rollout(p, k, x, dx, n_dir, t0, n_steps, f, din, sc, d_sched, st, [&](auto& kk, auto& q) {
        return crb::launch_imp_jvp_step(kk, q, n_iter, sc.f != nullptr, beam_groups(p), n_dir, p->NT, st);
    });
}

// ---- sensitivities of the equilibrium (crb_static.h: crb_static_sens_kernel; crb_paramgrad.h: crb_static_param_kernel)
namespace {
// every refusal before the device is touched, so that they hold for host-only plans too
int static_sens_plan_checks(const crb_plan* p, const std::string& who) {
    if (p->dtype != CRB_F64) return fail(CRB_EUNSUPPORTED, who + ": the static sensitivities need an fp64 plan");
    if (p->NT > STATIC_MAX_NT)
        return fail(CRB_EUNSUPPORTED, who + ": beams of more than 256 thread-carried nodes are not supported");
    if ((p->flags & CRB_FORCE_GRAVITY) && p->gravity_out_of_band)
        return fail(CRB_EUNSUPPORTED, who + ": the gravity index table couples a node to a rotation more than one slot away (a "
                                            "PINNED root under gravity); such terms lie outside the block-tridiagonal tangent, "
                                            "and a sensitivity without them would be wrong");
    return need_device(p, who.c_str());
}
}  // namespace

extern "C" int crb_static_jvp(const crb_plan* p, const void* x, const void* du, int n_dir, void* dq, int32_t* status, void* stream) {
    const std::string who = "crb_static_jvp";
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !du || !dq) return fail(CRB_EINVAL, who + ": null pointer");
    if (int rc = check_count(who, "n_dir", n_dir)) return rc;
    if (dq == x || dq == du || (status && (static_cast<const void*>(status) == x || static_cast<const void*>(status) == du ||
                                           static_cast<const void*>(status) == dq)))
        return fail(CRB_EINVAL, who + ": outputs must not alias inputs or each other");
    if (int rc = static_sens_plan_checks(p, who)) return rc;
    StaticSensParams<double> q{};
    q.rhs = static_cast<const double*>(du);
    q.sol = static_cast<double*>(dq);
    q.n_dir = n_dir;
    q.status = status;
    HIP_TRY(crb::launch_static_sens(static_params<double>(p, x), q, false, beam_groups(p), p->NT,
                                    static_cast<hipStream_t>(stream)));
    return CRB_OK;
}

extern "C" int crb_static_vjp(const crb_plan* p, const void* x, const void* q_bar, int n_cot, void* f_held_bar, void* param_bar,
                              int32_t* status, void* stream) {
    const std::string who = "crb_static_vjp";
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !q_bar || !f_held_bar) return fail(CRB_EINVAL, who + ": null pointer");
    if (int rc = check_count(who, "n_cot", n_cot)) return rc;
    const void* const st_v = status;
    if (f_held_bar == x || f_held_bar == q_bar || (param_bar && (param_bar == x || param_bar == q_bar || param_bar == f_held_bar)) ||
        (status && (st_v == x || st_v == q_bar || st_v == f_held_bar || st_v == param_bar)))
        return fail(CRB_EINVAL, who + ": outputs must not alias inputs or each other");
    if (int rc = static_sens_plan_checks(p, who)) return rc;
    if (param_bar)
        if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const KParams<double> k = static_params<double>(p, x);
    StaticSensParams<double> q{};
    q.rhs = static_cast<const double*>(q_bar);
    q.sol = static_cast<double*>(f_held_bar);
    q.n_dir = n_cot;
    q.status = status;
    HIP_TRY(crb::launch_static_sens(k, q, true, beam_groups(p), p->NT, st));
    if (param_bar) {
        AdjParams<double> a = adj_params(p);
        a.work = static_cast<const double*>(x);
        a.rbar = static_cast<double*>(f_held_bar);
        a.param_bar = static_cast<double*>(param_bar);
        HIP_TRY(crb::launch_static_param(k, a, beam_groups(p), n_cot, p->NT, st));
    }
    return CRB_OK;
}

// ------------------------------------------------------------------ adjoint of the closed loop (crb_feedback_adjoint.h)
namespace {
// The work buffer of the closed-loop checkpoint pass and adjoint (crb_rk4_feedback_adjoint_work_bytes), in doubles.
struct FbAdjWork {
    double *stages, *acc, *xcur, *u, *seed, *xbar, *sum, *ubar, *partial;
};
// doubles of the gain gradient's partial tiles (0 while one slice covers the beam reduction)
size_t fb_adj_partial_doubles(const crb_plan* p, int n_cot) {
    const int slices = crb::feedback_gain_grad_slices(p->B, p->n_free);
    return slices > 1 ? size_t(n_cot) * size_t(slices) * size_t(p->n_free) * size_t(2 * p->n_free) : 0;
}
FbAdjWork fb_adj_work(const crb_plan* p, void* work, int every, int n_cot) {
    const size_t S = state_doubles(p), F = S / 2;
    FbAdjWork w;
    w.stages = static_cast<double*>(work);
    w.acc = w.stages + size_t(every) * 4 * S;
    w.xcur = w.acc + S;
    w.u = w.xcur + S;
    w.seed = w.u + F;
    w.xbar = w.seed + size_t(n_cot) * S;
    w.sum = w.xbar + size_t(n_cot) * S;
    w.ubar = w.sum + size_t(n_cot) * S;
    w.partial = w.ubar + size_t(n_cot) * F;
    return w;
}

// the plan, size and input checks both calls share, before the device is touched
int fb_adj_checks(const crb_plan* p, int n_cot, const void* gain, const crb_input_desc* in, const crb_record_desc* rec, int n_steps,
                  int every, double dt, const std::string& who) {
    if (int rc = adjoint_checks(p, n_cot, who.c_str())) return rc;
    if (p->mixed_topology)
        return fail(CRB_EUNSUPPORTED, who + ": one gain for the ensemble needs one free-DOF set (the plan has mixed topology)");
    if (p->flags & CRB_FORCE_GRAVITY) {
        std::vector<GravAdj> lists;
        for (const auto& tab : p->h_grav_topo) {
            int ms = 0, mp = 0;
            if (!grav_transpose(tab, lists, &ms, &mp))
                return fail(CRB_EUNSUPPORTED, who + ": the gravity index table has a fan-in of " + std::to_string(ms) + " / " +
                                                  std::to_string(mp) + ", beyond the adjoint's lists (crb_rhs_vjp refuses the plan)");
        }
    }
    if (rec && rec->node == CRB_RECORD_ALL)
        return fail(CRB_EUNSUPPORTED, who + ": rec with CRB_RECORD_ALL (whole-state snapshots) is not supported in the closed loop");
    if (!gain) return fail(CRB_EINVAL, who + ": gain is null");
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (every < 1) return fail(CRB_EINVAL, who + ": every must be >= 1");
    if (!(dt > 0)) return fail(CRB_EINVAL, who + ": dt must be positive");
    return CRB_OK;
}

// no output of a differentiable closed-loop call may be one of its inputs (`ins_text` names them) or another output
template <size_t NO, size_t NI>
int fb_adj_alias_checks(const std::string& who, const void* const (&outs)[NO], const char* const (&out_names)[NO],
                        const void* const (&ins)[NI], const char* ins_text) {
    for (size_t i = 0; i < NO; ++i) {
        if (!outs[i]) continue;
        for (const void* b : ins)
            if (b && b == outs[i]) return fail(CRB_EINVAL, who + ": " + out_names[i] + " must not alias " + ins_text);
        for (size_t j = i + 1; j < NO; ++j)
            if (outs[j] == outs[i]) return fail(CRB_EINVAL, who + ": " + out_names[i] + " must not alias " + out_names[j]);
    }
    return CRB_OK;
}

// what the matrix kernels of both closed-loop adjoints read of the plan and the call (ubar, xs and partial are the loop's own)
void fba_params(FbaParams& q, const crb_plan* p, int n_cot, const void* gain, const void* ref, void* lam,
                const crb_feedback_cotangent* grad) {
    q.col_off = p->d_col_off;
    q.row_off = p->d_row_off;
    q.rows = n_cot * p->B; q.B = p->B; q.n = p->n_free; q.n2 = 2 * p->n_free;
    q.x_stride = size_t(2) * p->n_node * 4;
    q.u_stride = size_t(p->n_node) * 4;
    q.gain = static_cast<const double*>(gain);
    q.lam = static_cast<double*>(lam);
    q.ref_bar = static_cast<double*>(grad->ref_bar);
    q.ref = static_cast<const double*>(ref);
    q.gain_bar = static_cast<double*>(grad->gain_bar);
}

// one RK4 step of the stage-split closed loop from xcur (advanced in place): feedback_rollout's launches (plus the held
// disturbance, if any, added to each stage's force), the stage states
// X_2 .. X_4 written to s1 .. s3 (stage 3's unused xs_next goes to `spare`)
int fb_adj_step(const crb_plan* p, void* xcur, double* s1, double* s2, double* s3, double* spare, const FbAdjWork& w, double t,
                double dt, const void* gain, const void* ref, const Forcing& f, void* stream) {
    const double th = t + 0.5 * dt, t1 = t + dt;   // same clock convention as crb_step_rk4
    const double ts[4] = {t, th, th, t1};
    void* const nxt[4] = {s1, s2, s3, spare};
    const void* cur = xcur;
    for (int stage = 0; stage < 4; ++stage) {
        if (int rc = crb_feedback_force(p, cur, gain, ref, w.u, stream)) return rc;
        if (f.held)   // (a held disturbance: crb_rk4_stage reads the stage force in the held force's place)
            HIP_TRY(crb::launch_feedback_held(w.u, static_cast<const double*>(f.held), p->d_row_off, p->n_free, p->B,
                                              size_t(p->n_node) * 4, static_cast<hipStream_t>(stream)));
        if (int rc = rk4_stage(p, xcur, cur, w.acc, nxt[stage], w.u, stage, ts[stage], dt, f, stream, false)) return rc;
        cur = nxt[stage];
    }
    return CRB_OK;
}
}  // namespace

extern "C" size_t crb_rk4_feedback_adjoint_work_bytes(const crb_plan* p, int every, int n_cot) {
    if (!p || every < 1 || n_cot < 1) return 0;
    const size_t S = state_doubles(p), F = S / 2;
    return ((size_t(4) * size_t(every) + 2 + 3 * size_t(n_cot)) * S + (1 + size_t(n_cot)) * F + fb_adj_partial_doubles(p, n_cot)) *
           sizeof(double);
}

extern "C" int crb_step_rk4_feedback_checkpoint(const crb_plan* p, void* x, double t0, double dt, int n_steps, int every,
                                                const void* gain, const void* ref, const crb_input_desc* in,
                                                const crb_record_desc* rec, void* ckpt, void* work, double* t_end, void* stream) {
    const std::string who("crb_step_rk4_feedback_checkpoint");
    if (int rc = fb_adj_checks(p, 1, gain, in, rec, n_steps, every, dt, who)) return rc;
    if (!x) return fail(CRB_EINVAL, who + ": x is null");
    if (!ckpt) return fail(CRB_EINVAL, who + ": ckpt is null");
    if (!work) return fail(CRB_EINVAL, who + ": work is null (crb_rk4_feedback_adjoint_work_bytes)");
    const void* ins[4] = {gain, ref, rec ? rec->out : nullptr, in ? in->f_held : nullptr};
    for (const void* b : ins)
        if (b && (b == x || b == ckpt || b == work)) return fail(CRB_EINVAL, who + ": x, ckpt and work must not alias gain, ref, rec->out or input->f_held");
    if (x == ckpt || x == work || ckpt == work) return fail(CRB_EINVAL, who + ": x, ckpt and work must not alias each other");
    if (int rc = need_device(p, who.c_str())) return rc;
    Recording r;
    if (int rc = decode_record(p, rec, n_steps, true, who.c_str(), &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who.c_str(), &f)) return rc;
    if (t_end) *t_end = clock_after(t0, dt, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t S = state_doubles(p), x_stride = size_t(2) * p->n_node * 4;
    const FbAdjWork w = fb_adj_work(p, work, 1, 1);
    HIP_TRY(hipMemsetAsync(w.u, 0, S / 2 * sizeof(double), st));   // (entries of u no product writes must read as zero)
    const size_t rec_off = r.slot >= 0 ? (size_t(r.comp / 3) * p->n_node + size_t(r.slot + p->off)) * 4 + size_t(r.comp % 3) : 0;
    double t = t0;
    for (int s = 0; s < n_steps; ++s) {
        if (s % every == 0)
            HIP_TRY(hipMemcpyAsync(static_cast<double*>(ckpt) + size_t(s / every) * S, x, S * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (int rc = fb_adj_step(p, x, w.stages, w.stages + S, w.stages + 2 * S, w.stages + 3 * S, w, t, dt, gain, ref, f, stream)) return rc;
        t = t + dt;
        if (r.slot >= 0 && (s + 1) % r.every == 0 && (s + 1) / r.every <= r.count)
            HIP_TRY(crb::launch_feedback_record(static_cast<const double*>(x), x_stride, rec_off, p->B, static_cast<double*>(r.out),
                                                r.count, (s + 1) / r.every - 1, st));
    }
    return CRB_OK;
}

extern "C" int crb_step_rk4_feedback_adjoint(const crb_plan* p, const void* ckpt, void* lam, int n_cot, double t0, double dt,
                                             int n_steps, int every, const void* gain, const void* ref, const crb_input_desc* in,
                                             const crb_record_desc* rec_bar, const crb_feedback_cotangent* grad, void* work,
                                             void* stream) {
    const std::string who("crb_step_rk4_feedback_adjoint");
    if (int rc = fb_adj_checks(p, n_cot, gain, in, rec_bar, n_steps, every, dt, who)) return rc;
    if (!lam) return fail(CRB_EINVAL, who + ": lam is null");
    if (!ckpt) return fail(CRB_EINVAL, who + ": ckpt is null");
    if (!work) return fail(CRB_EINVAL, who + ": work is null (crb_rk4_feedback_adjoint_work_bytes)");
    if (!grad) return fail(CRB_EINVAL, who + ": grad is null (crb_feedback_cotangent; its members may be null)");
    const void* const outs[3] = {lam, grad->gain_bar, grad->ref_bar};
    const char* const out_names[3] = {"lam", "grad->gain_bar", "grad->ref_bar"};
    const void* const ins[6] = {ckpt, work, gain, ref, rec_bar ? rec_bar->out : nullptr, in ? in->f_held : nullptr};
    if (int rc = fb_adj_alias_checks(who, outs, out_names, ins, "ckpt, work, gain, ref, rec_bar->out or input->f_held")) return rc;
    if (work == ckpt || work == gain || work == ref) return fail(CRB_EINVAL, who + ": work must not alias ckpt, gain or ref");
    if (int rc = need_device(p, who.c_str())) return rc;
    Recording r;
    if (int rc = decode_record(p, rec_bar, n_steps, true, who.c_str(), &r)) return rc;
    Forcing f;
    if (int rc = decode_input(p, in, who.c_str(), &f)) return rc;
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t S = state_doubles(p), x_stride = size_t(2) * p->n_node * 4;
    const FbAdjWork w = fb_adj_work(p, work, every, n_cot);
    // a sample of a constrained DOF has no cotangent to hand on (the state holds 0 there)
    const bool rec_on = r.slot >= 0 && p->any_free[size_t(3) * size_t(r.slot + p->off) + size_t(r.comp % 3)];
    const size_t rec_off = rec_on ? (size_t(r.comp / 3) * p->n_node + size_t(r.slot + p->off)) * 4 + size_t(r.comp % 3) : 0;

    FeedbackAdjParams q = zeroed<FeedbackAdjParams>();
    fba_params(q, p, n_cot, gain, ref, lam, grad);
    q.ubar = w.ubar;
    q.xbar = w.xbar;
    q.sum = w.sum;
    q.seed = w.seed;
    q.partial = w.partial;
    // the seeds of DESIGN 10: kbar4 = dt/6 l+, kbar3 = dt/3 l+ + dt s4, kbar2 = dt/3 l+ + dt/2 s3, kbar1 = dt/6 l+ + dt/2 s2;
    // the launch after stage s forms the seed of stage s - 1
    const double ca_next[4] = {0.0, dt / 6.0, dt / 3.0, dt / 3.0}, cb_next[4] = {0.0, 0.5 * dt, 0.5 * dt, dt};

    return for_segments_reversed(n_steps, every, t0, dt, [&](int g, int k0, int n, double t) -> int {
        // 1. the segment's stage states from its checkpoint, straight into the work buffer
        HIP_TRY(hipMemcpyAsync(w.xcur, static_cast<const double*>(ckpt) + size_t(g) * S, S * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(w.u, 0, S / 2 * sizeof(double), st));
        for (int i = 0; i < n; ++i) {
            double* const X = w.stages + size_t(i) * 4 * S;
            HIP_TRY(hipMemcpyAsync(X, w.xcur, S * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (int rc = fb_adj_step(p, w.xcur, X + S, X + 2 * S, X + 3 * S, w.xbar, w, t, dt, gain, ref, f, stream)) return rc;
            t = t + dt;
        }
        // 2. the sweep back over it, every cotangent: per stage crb_rhs_vjp, the transposed product, the gain gradient
        for (int i = n - 1; i >= 0; --i) {
            const int kstep = k0 + i;
            const bool sample = rec_on && (kstep + 1) % r.every == 0 && (kstep + 1) / r.every <= r.count;
            HIP_TRY(crb::launch_feedback_seed(q.lam, w.seed, size_t(q.rows) * x_stride, x_stride, dt / 6.0,
                                              sample ? static_cast<const double*>(r.out) : nullptr, rec_off, r.count,
                                              sample ? (kstep + 1) / r.every - 1 : 0, st));
            for (int s = 3; s >= 0; --s) {
                double* const X = w.stages + (size_t(i) * 4 + size_t(s)) * S;
                KParams<double> k = base_params<double>(p);
                k.x = X;
                AdjParams<double> a = adj_params(p);
                a.lam_in = w.seed;
                a.xbar = w.xbar;
                a.ubar = w.ubar;
                HIP_TRY(crb::launch_adj_rhs(k, a, beam_groups(p), n_cot, p->NT, st));
                q.first = s == 3; q.last = s == 0;
                q.ca = ca_next[s]; q.cb = cb_next[s];
                HIP_TRY(crb::launch_feedback_transpose(q, st));
                if (q.gain_bar) {
                    q.xs = X;
                    HIP_TRY(crb::launch_feedback_gain_grad(q, st));
                }
            }
        }
        return CRB_OK;
    });
}

// ------------------------------------------------------------------ adjoint of the sampled-data implicit loop
// (crb_implicit_feedback_adjoint.h): the implicit adjoint's launches per sample, the boundary products between them
namespace {
// CRB_EINVAL checks of the sizes both calls share, in the documented order
int imp_fb_adjoint_arg_checks(const std::string& who, int n_cot, int n_steps, int every, int hold, int n_iter, double h) {
    if (int rc = check_count(who, "n_cot", n_cot)) return rc;
    if (n_steps < 0) return fail(CRB_EINVAL, who + ": n_steps must be >= 0");
    if (every < 1) return fail(CRB_EINVAL, who + ": every must be >= 1");
    if (hold < 1) return fail(CRB_EINVAL, who + ": hold must be >= 1");
    if (every % hold != 0) return fail(CRB_EINVAL, who + ": every must be a multiple of hold (a checkpoint sits on a sample start)");
    if (n_iter < 1 || n_iter > IMP_ADJ_MAX_ITER) return fail(CRB_EINVAL, who + ": n_iter must be in [1, 16]");
    if (!(h > 0)) return fail(CRB_EINVAL, who + ": h must be positive");
    return CRB_OK;
}
// the record and the input of both calls (CRB_EINVAL), then what the plan cannot do (CRB_EUNSUPPORTED), then the device
int imp_fb_adjoint_io_checks(const crb_plan* p, const std::string& who, const crb_record_desc* rec, const crb_input_desc* in,
                             int n_steps, int hold, bool amp_bar, Recording* r, Forcing* f) {
    if (int rc = decode_record(p, rec, n_steps, true, who.c_str(), r)) return rc;
    if (rec && hold % rec->every != 0 && rec->every % hold != 0)
        return fail(CRB_EINVAL, who + ": the record stride must divide hold or be a multiple of it");
    if (int rc = decode_input(p, in, who.c_str(), f)) return rc;
    if (amp_bar && !f->impulse)
        return fail(CRB_EINVAL, who + ": amp_bar needs an impulse input (its amplitude is what it differentiates)");
    if (int rc = imp_adjoint_plan_checks(p, who)) return rc;
    if (p->mixed_topology)
        return fail(CRB_EUNSUPPORTED, who + ": one gain matrix for the ensemble needs one free-DOF set (the plan has mixed topology)");
    if (rec && rec->node == CRB_RECORD_ALL)
        return fail(CRB_EUNSUPPORTED, who + ": rec with CRB_RECORD_ALL (whole-state snapshots) is not supported in the differentiable loop");
    return need_device(p, who.c_str());
}
// The work buffer (crb_implicit_feedback_adjoint_work_bytes), in doubles: the implicit adjoint's (imp_adj_work), then ubar of
// every sample of a segment [n_cot][every / hold] force records, then the gain gradient's running partial tiles.
struct ImpFbAdjWork {
    ImpAdjWork imp;
    double *ubar, *partial;
};
ImpFbAdjWork imp_fb_adj_work(const crb_plan* p, void* work, int every, int n_iter, int hold, int n_cot) {
    ImpFbAdjWork w;
    w.imp = imp_adj_work(p, work, every, n_iter, n_cot);
    w.ubar = w.imp.carry + size_t(n_cot) * force_doubles(p);
    w.partial = w.ubar + size_t(n_cot) * size_t(every / hold) * force_doubles(p);
    return w;
}
}  // namespace

extern "C" size_t crb_implicit_feedback_adjoint_work_bytes(const crb_plan* p, int every, int n_iter, int hold, int n_cot) {
    if (!p || every < 1 || hold < 1 || every % hold != 0 || n_iter < 1 || n_iter > IMP_ADJ_MAX_ITER || n_cot < 1 || n_cot > 65535)
        return 0;
    const size_t F = force_doubles(p);
    return (size_t(every) * ((2 + size_t(n_iter)) * F + 1) + size_t(n_cot) * (1 + size_t(every / hold)) * F +
            fb_adj_partial_doubles(p, n_cot)) * sizeof(double);
}

extern "C" int crb_step_implicit_feedback_checkpoint(const crb_plan* p, void* x, double t0, double h, int n_steps, int n_iter,
                                                     int hold, int every, const void* gain, const void* ref,
                                                     const crb_input_desc* in, const crb_record_desc* rec, void* ckpt,
                                                     void* u_ckpt, void* work, double* t_end, void* stream) {
    const std::string who("crb_step_implicit_feedback_checkpoint");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !gain || !ckpt || !u_ckpt || !work) return fail(CRB_EINVAL, who + ": null x, gain, ckpt, u_ckpt or work");
    const void* const outs[4] = {x, ckpt, u_ckpt, work};
    const void* const ins[4] = {gain, ref, rec ? rec->out : nullptr, in ? in->f_held : nullptr};
    for (int i = 0; i < 4; ++i) {
        for (const void* b : ins)
            if (b && b == outs[i]) return fail(CRB_EINVAL, who + ": x, ckpt, u_ckpt and work must not alias gain, ref, rec->out or input->f_held");
        for (int j = i + 1; j < 4; ++j)
            if (outs[j] == outs[i]) return fail(CRB_EINVAL, who + ": x, ckpt, u_ckpt and work must not alias each other");
    }
    if (int rc = imp_fb_adjoint_arg_checks(who, 1, n_steps, every, hold, n_iter, h)) return rc;
    Recording r;
    Forcing f;
    if (int rc = imp_fb_adjoint_io_checks(p, who, rec, in, n_steps, hold, false, &r, &f)) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> base;
    if (int rc = imp_adjoint_params(p, h, st, &base)) return rc;
    base.x = static_cast<double*>(x);
    HIP_TRY(zero_controls(p, u_ckpt, nullptr, n_steps, hold, st));
    ImpAdjParams<double> iq = zeroed<ImpAdjParams<double>>();
    iq.n_iter = n_iter;
    return for_samples(n_steps, hold, t0, h, [&](int ks, int s, int hs, double t) -> int {
        KParams<double> k = base;
        if (int rc = sample_control(p, k, x, gain, ref, f, r, control_record(p, u_ckpt, nullptr, ks), s, hs, hold, st)) return rc;
        k.t0 = t; k.n_steps = hs;
        // one launch per sample: it starts from a^0 = 0 and stores the state it starts from -- into the checkpoint where the
        // sample opens a segment (every is a multiple of hold), else into the head of the work buffer, where nothing reads it
        void* const start = s % every == 0 ? static_cast<double*>(ckpt) + size_t(s / every) * 3 * force_doubles(p) : static_cast<double*>(work);
        HIP_TRY(crb::launch_imp_adj_checkpoint(k, checkpoint_params(p, start, hold), iq, beam_groups(p), p->NT, st));
        return CRB_OK;
    });
}

extern "C" int crb_step_implicit_feedback_adjoint(const crb_plan* p, const void* ckpt, const void* u_ckpt, void* lam, int n_cot,
                                                  double t0, double h, int n_steps, int n_iter, int hold, int every,
                                                  const void* gain, const void* ref, const crb_input_desc* in,
                                                  const crb_record_desc* rec_bar, const crb_feedback_cotangent* grad,
                                                  const crb_input_cotangent* igrad, void* work, void* stream) {
    const std::string who("crb_step_implicit_feedback_adjoint");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!ckpt || !u_ckpt || !lam || !gain || !work) return fail(CRB_EINVAL, who + ": null ckpt, u_ckpt, lam, gain or work");
    if (!grad) return fail(CRB_EINVAL, who + ": grad is null (crb_feedback_cotangent; its members may be null)");
    void* const amp_bar = igrad ? igrad->amp_bar : nullptr;
    void* const f_bar = igrad ? igrad->f_held_bar : nullptr;
    const void* const outs[5] = {lam, grad->gain_bar, grad->ref_bar, amp_bar, f_bar};
    const char* const out_names[5] = {"lam", "grad->gain_bar", "grad->ref_bar", "igrad->amp_bar", "igrad->f_held_bar"};
    const void* const ins[7] = {ckpt, u_ckpt, work, gain, ref, rec_bar ? rec_bar->out : nullptr, in ? in->f_held : nullptr};
    if (int rc = fb_adj_alias_checks(who, outs, out_names, ins, "ckpt, u_ckpt, work, gain, ref, rec_bar->out or input->f_held"))
        return rc;
    if (work == ckpt || work == u_ckpt || work == gain || work == ref || ckpt == u_ckpt)
        return fail(CRB_EINVAL, who + ": work, ckpt and u_ckpt must not alias each other, gain or ref");
    if (int rc = imp_fb_adjoint_arg_checks(who, n_cot, n_steps, every, hold, n_iter, h)) return rc;
    Recording r;
    Forcing f;
    if (int rc = imp_fb_adjoint_io_checks(p, who, rec_bar, in, n_steps, hold, amp_bar != nullptr, &r, &f)) return rc;
    if (n_steps == 0) return CRB_OK;
    if (int rc = ensure_gadj(p, who.c_str())) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> base;
    if (int rc = imp_adjoint_params(p, h, st, &base)) return rc;
    set_io(base, f);
    base.u_held = nullptr;   // (the held force is inside every u_k: the recompute reads u_ckpt as its schedule)
    const size_t F = force_doubles(p), S = state_doubles(p);
    const int per_seg = every / hold, slices = crb::feedback_gain_grad_slices(p->B, p->n_free);
    const ImpFbAdjWork w = imp_fb_adj_work(p, work, every, n_iter, hold, n_cot);
    const Schedule sc{u_ckpt, (n_steps + hold - 1) / hold, hold};
    ImpAdjParams<double> iter = zeroed<ImpAdjParams<double>>();
    iter.n_iter = n_iter;

    ImpFbAdjParams q = zeroed<ImpFbAdjParams>();
    fba_params(q, p, n_cot, gain, ref, lam, grad);
    q.cot_stride = size_t(per_seg) * F;
    q.sample_stride = F;
    q.f_held_bar = static_cast<double*>(f_bar);
    q.xs = w.imp.states;
    q.xs_stride = size_t(hold) * S;
    q.partial = w.partial;
    if (q.gain_bar && slices > 1)   // the slices' running tiles persist across the segments of the call
        HIP_TRY(hipMemsetAsync(w.partial, 0, fb_adj_partial_doubles(p, n_cot) * sizeof(double), st));

    const int rc = for_segments_reversed(n_steps, every, t0, h, [&](int g, int k0, int n, double tg) -> int {
        // 1. the segment's step data from its checkpoint: the scheduled recompute with f_sched = u_ckpt (every sample's first
        //    step starts from a^0 = 0, as the pass's launch per sample did)
        KParams<double> k = base;
        k.t0 = tg;
        k.n_steps = n;
        set_sched(p, k, sc, k0);
        AdjParams<double> qs = adj_params(p);
        qs.states = w.imp.states;
        qs.clocks = w.imp.clock;
        ImpAdjParams<double> iq = iter;
        iq.start = static_cast<const double*>(ckpt) + size_t(g) * 3 * F;
        iq.iters_out = w.imp.iters;
        HIP_TRY(crb::launch_imp_adj_segment(k, qs, iq, beam_groups(p), p->NT, st));
        // 2. per sample, last first: the sweep over its steps (ubar_k into the sample's slot, which it accumulates into),
        //    then the boundary
        const int ns = (n + hold - 1) / hold;
        HIP_TRY(hipMemsetAsync(w.ubar, 0, size_t(n_cot) * size_t(per_seg) * F * sizeof(double), st));
        for (int j = ns - 1; j >= 0; --j) {
            const int i0 = j * hold, hs = n - i0 < hold ? n - i0 : hold;
            KParams<double> kb = base;
            kb.n_steps = hs;
            set_sched(p, kb, sc, k0 + i0);
            set_record(kb, r);
            AdjParams<double> b = adj_params(p);
            b.work = w.imp.states + size_t(i0) * S;
            b.work_clock = w.imp.clock + i0;
            b.lam = static_cast<double*>(lam);
            b.amp_bar = static_cast<double*>(amp_bar);
            b.f_bar = w.ubar + size_t(j) * F;
            b.fbar_cot_stride = q.cot_stride;
            b.step0 = k0 + i0;
            ImpAdjParams<double> ib = iter;
            ib.iters = w.imp.iters + size_t(i0) * size_t(n_iter) * F;
            ib.carry = w.imp.carry;
            ib.carry_in = 0;   // (the launch ends a sample: the next sample's a^0 = 0 is a constant)
            HIP_TRY(crb::launch_imp_adj_backward(kb, b, ib, beam_groups(p), n_cot, p->NT, st));
            ImpFbAdjParams qb = q;
            qb.ubar = w.ubar + size_t(j) * F;
            HIP_TRY(crb::launch_imp_fb_boundary(qb, st));
        }
        // 3. the gain gradient of the segment's samples in one launch
        if (q.gain_bar) {
            ImpFbAdjParams qg = q;
            qg.ubar = w.ubar;
            qg.n_samples = ns;
            HIP_TRY(crb::launch_imp_fb_gain_grad(qg, st));
        }
        return CRB_OK;
    });
    if (rc) return rc;
    if (q.gain_bar && slices > 1) HIP_TRY(crb::launch_feedback_gain_reduce(q.gain_bar, w.partial, p->n_free, n_cot, slices, st));
    return CRB_OK;
}

// ------------------------------------------------------------------ tangent of the sampled-data implicit loop
// (crb_implicit_feedback_tangent.h): per sample the boundary products, then the implicit tangent's scheduled kernel over the
// sample's steps as ONE interval of a schedule (u_k, du_k) -- a^0 = 0 and da^0 = 0 at its first step
extern "C" size_t crb_implicit_feedback_tangent_work_bytes(const crb_plan* p, int n_dir) {
    if (!p || n_dir < 1 || n_dir > 65535) return 0;
    return (size_t(1) + size_t(n_dir)) * force_doubles(p) * sizeof(double);
}

extern "C" int crb_step_implicit_feedback_tangent(const crb_plan* p, void* x, void* dx, int n_dir, double t0, double h, int n_steps,
                                                  int n_iter, int hold, const void* gain, const void* ref,
                                                  const crb_feedback_tangent* dfb, const crb_input_desc* in,
                                                  const crb_input_tangent* din, void* u_out, void* du_out, void* work,
                                                  double* t_end, void* stream) {
    const std::string who("crb_step_implicit_feedback_tangent");
    if (!p) return fail(CRB_EINVAL, who + ": null plan");
    if (!x || !dx || !gain || !work) return fail(CRB_EINVAL, who + ": null x, dx, gain or work");
    const void* const d_gain = dfb ? dfb->d_gain : nullptr;
    const void* const d_ref = dfb ? dfb->d_ref : nullptr;
    const void* const d_amp = din ? din->d_amp : nullptr;
    const void* const df_held = din ? din->df_held : nullptr;
    const void* const outs[4] = {dx, u_out, du_out, work};
    const char* const out_names[4] = {"dx", "u_out", "du_out", "work"};
    const void* const ins[9] = {x, gain, ref, d_gain, d_ref, in ? in->f_held : nullptr, in ? in->amp : nullptr, df_held, d_amp};
    if (int rc = fb_adj_alias_checks(who, outs, out_names, ins,
                                     "x, gain, ref, dfb->d_gain, dfb->d_ref, input->f_held, input->amp, dinput->df_held or dinput->d_amp"))
        return rc;
    if (int rc = imp_tangent_arg_checks(who, n_dir, n_steps, n_iter, h)) return rc;
    if (hold < 1) return fail(CRB_EINVAL, who + ": hold must be >= 1");
    Forcing f;
    if (int rc = tangent_input(p, in, din, who, &f)) return rc;
    if (int rc = imp_tangent_plan_checks(p, who)) return rc;
    if (p->mixed_topology)
        return fail(CRB_EUNSUPPORTED, who + ": one gain matrix for the ensemble needs one free-DOF set (the plan has mixed topology)");
    if (int rc = need_device(p, who.c_str())) return rc;
    if (t_end) *t_end = clock_after(t0, h, n_steps);
    if (n_steps == 0) return CRB_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KParams<double> base;
    if (int rc = imp_adjoint_params(p, h, st, &base)) return rc;   // (A's tables where M's are, base.dt = h)
    base.x = static_cast<double*>(x);
    set_io(base, f);
    base.u_held = nullptr;   // (the held force is inside every u_k)
    // a beam that goes non-finite is marked with the step count at the end of the CALL, as crb_step_implicit_feedback does
    arm_status(p, base, n_steps);
    const size_t F = force_doubles(p);
    // a sample's du_k beside its u_k: record k of du_out, else one record per direction behind work's; zeroed as the controls are
    double* const du0 = du_out ? static_cast<double*>(du_out) : static_cast<double*>(work) + F;
    const size_t du_step = du_out ? F : 0, du_dir = du_out ? size_t((n_steps + hold - 1) / hold) * F : F;
    HIP_TRY(zero_controls(p, u_out, work, n_steps, hold, st));
    HIP_TRY(hipMemsetAsync(du0, 0, size_t(n_dir) * du_dir * sizeof(double), st));

    crb::ImpFbTanParams b = zeroed<crb::ImpFbTanParams>();
    b.col_off = p->d_col_off;
    b.row_off = p->d_row_off;
    b.B = p->B; b.n = p->n_free; b.n2 = 2 * p->n_free; b.n_dir = n_dir;
    b.x_stride = size_t(2) * p->n_node * 4;
    b.u_stride = size_t(p->n_node) * 4;
    b.gain = static_cast<const double*>(gain);
    b.d_gain = static_cast<const double*>(d_gain);
    b.ref = static_cast<const double*>(ref);
    b.d_ref = static_cast<const double*>(d_ref);
    b.x = static_cast<const double*>(x);
    b.dx = static_cast<const double*>(dx);
    b.f_held = static_cast<const double*>(f.held);
    b.df_held = static_cast<const double*>(df_held);
    b.du_dir_stride = du_dir;

    return for_samples(n_steps, hold, t0, h, [&](int ks, int, int hs, double t) -> int {
        b.u = control_record(p, u_out, work, ks);
        b.du = du0 + size_t(ks) * du_step;
        HIP_TRY(crb::launch_imp_fb_tangent_boundary(b, st));
        TangentParams<double> q;   // (the base as the boundary kernel read it: the sample's steps advance x)
        if (int rc = tangent_base(p, x, dx, n_dir, din, st, &q)) return rc;
        q.du_held = b.du; q.du_dir_stride = du_dir;
        KParams<double> k = base;
        k.t0 = t; k.n_steps = hs;
        // the sample as the one interval of a schedule: the kernel never switches (hs <= hold)
        set_sched(p, k, Schedule{b.u, 1, hold}, 0);
        HIP_TRY(crb::launch_imp_jvp_step(k, q, n_iter, true, beam_groups(p), n_dir, p->NT, st));
        return CRB_OK;
    });
}
