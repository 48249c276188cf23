// crb_static_rows.cpp -- TEST HARNESS ONLY: the block cyclic reduction of the static sensitivities (crb_static.h:
// static_solve_multi) on the host, one "thread" per node row in a loop, built from the same CRB_HD row functions the
// kernel calls (crb_math.h: row3_normalise_matrix / _rhs, row3_level_matrix / _rhs): transposition of the rows, symmetric
// Jacobi scaling, all ceil(log2 S) levels, NR right-hand sides per pass with a tail (tests/test_static_sensitivities_cpu.py).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../continuum-robot_amd/csrc/crb_math.h"

using namespace crb;

namespace {
constexpr int NR = 4;
struct Row {
    double A[9], B[9], C[9];
    double r[NR][3];
};

// row3_normalise and row3_level as they were before they were split (one function each, matrix and right-hand side together)
void unsplit_normalise(Row3& w) {
    double Bi[9], t[9], v[3];
    inv3<double>(w.B, Bi);
    mul3<double>(Bi, w.A, t);
    for (int k = 0; k < 9; ++k) w.A[k] = t[k];
    mul3<double>(Bi, w.C, t);
    for (int k = 0; k < 9; ++k) w.C[k] = t[k];
    mulv3<double>(Bi, w.r, v);
    for (int k = 0; k < 3; ++k) { w.r[k] = v[k]; w.B[k * 3 + 0] = k == 0; w.B[k * 3 + 1] = k == 1; w.B[k * 3 + 2] = k == 2; }
}
void unsplit_level(const Row3& me, const double loA[9], const double loC[9], const double lor[3], const double hiA[9],
                   const double hiC[9], const double hir[3], Row3& out) {
    double t[9], u[9], v[3], w[3];
    mul3<double>(me.A, loC, t);
    mul3<double>(me.C, hiA, u);
    for (int k = 0; k < 9; ++k) out.B[k] = ((k % 4) == 0 ? 1.0 : 0.0) - t[k] - u[k];
    mul3<double>(me.A, loA, t);
    mul3<double>(me.C, hiC, u);
    for (int k = 0; k < 9; ++k) { out.A[k] = -t[k]; out.C[k] = -u[k]; }
    mulv3<double>(me.A, lor, v);
    mulv3<double>(me.C, hir, w);
    for (int k = 0; k < 3; ++k) out.r[k] = me.r[k] - v[k] - w[k];
}

// the node rows of J^T from those of J: lower = (C_{j-1})^T, own = B_j^T, upper = (A_{j+1})^T; zero blocks outside
void transpose_rows(std::vector<Row>& w) {
    const int S = int(w.size());
    std::vector<Row> o(w);
    for (int j = 0; j < S; ++j)
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) {
                o[j].A[3 * i + c] = j >= 1 ? w[j - 1].C[3 * c + i] : 0.0;
                o[j].C[3 * i + c] = j + 1 < S ? w[j + 1].A[3 * c + i] : 0.0;
                o[j].B[3 * i + c] = w[j].B[3 * c + i];
            }
    w = o;
}

// one pass: NR right-hand sides (already in w[j].r), solution into x [S][NR][3]
void solve_pass(std::vector<Row> w, double* x) {
    const int S = int(w.size());
    int levels = 0;
    while ((1 << levels) < S) ++levels;
    std::vector<double> d(size_t(S) * 3);
    for (int j = 0; j < S; ++j)
        for (int c = 0; c < 3; ++c) {
            const double a = std::fabs(w[j].B[4 * c]);
            d[3 * j + c] = (a > 0.0 && a < INFINITY) ? 1.0 / std::sqrt(a) : 1.0;
        }
    for (int j = 0; j < S; ++j)
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < NR; ++k) w[j].r[k][i] *= d[3 * j + i];
            for (int c = 0; c < 3; ++c) {
                w[j].A[3 * i + c] *= d[3 * j + i] * (j >= 1 ? d[3 * (j - 1) + c] : 1.0);
                w[j].B[3 * i + c] *= d[3 * j + i] * d[3 * j + c];
                w[j].C[3 * i + c] *= d[3 * j + i] * (j + 1 < S ? d[3 * (j + 1) + c] : 1.0);
            }
        }
    const double zero9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, zero3[3] = {0, 0, 0};
    for (int l = 0; l < levels; ++l) {
        const int s = 1 << l;
        for (int j = 0; j < S; ++j) {
            double Bi[9];
            row3_normalise_matrix(w[j].A, w[j].B, w[j].C, Bi);
            for (int k = 0; k < NR; ++k) row3_normalise_rhs(Bi, w[j].r[k]);
        }
        std::vector<Row> o(w);
        for (int j = 0; j < S; ++j) {
            const bool lo = j - s >= 0, hi = j + s < S;
            const Row* L = lo ? &w[j - s] : nullptr;
            const Row* H = hi ? &w[j + s] : nullptr;
            for (int k = 0; k < NR; ++k)
                row3_level_rhs(w[j].A, w[j].C, w[j].r[k], lo ? L->r[k] : zero3, hi ? H->r[k] : zero3, o[j].r[k]);
            row3_level_matrix(w[j].A, w[j].C, lo ? L->A : zero9, lo ? L->C : zero9, hi ? H->A : zero9, hi ? H->C : zero9, o[j].A,
                              o[j].B, o[j].C);
        }
        w = o;
    }
    for (int j = 0; j < S; ++j) {
        double Bi[9];
        inv3<double>(w[j].B, Bi);
        for (int k = 0; k < NR; ++k) {
            double v[3];
            mulv3<double>(Bi, w[j].r[k], v);
            for (int c = 0; c < 3; ++c) x[(size_t(j) * NR + k) * 3 + c] = v[c] * d[3 * j + c];
        }
    }
}
}  // namespace

extern "C" {
int rows_nr() { return NR; }

// blocks [S][3][9] (A, B, C of every node row of J), rhs / out [n_rhs][S][3]; transpose != 0 solves with J^T; refine != 0
// adds the kernel's refinement step.  The
// right-hand sides go through in chunks of NR; the tail chunk's missing ones are zero and store nothing.
void rows_solve(int S, const double* blocks, int transpose, int refine, int n_rhs, const double* rhs, double* out) {
    std::vector<Row> w;
    w.resize(size_t(S));
    for (int j = 0; j < S; ++j) {
        std::memcpy(w[j].A, blocks + size_t(j) * 27, 9 * sizeof(double));
        std::memcpy(w[j].B, blocks + size_t(j) * 27 + 9, 9 * sizeof(double));
        std::memcpy(w[j].C, blocks + size_t(j) * 27 + 18, 9 * sizeof(double));
    }
    if (transpose) transpose_rows(w);
    std::vector<double> x(size_t(S) * NR * 3);
    for (int d0 = 0; d0 < n_rhs; d0 += NR) {
        for (int j = 0; j < S; ++j)
            for (int k = 0; k < NR; ++k)
                for (int c = 0; c < 3; ++c) w[j].r[k][c] = d0 + k < n_rhs ? rhs[(size_t(d0 + k) * S + j) * 3 + c] : 0.0;
        solve_pass(w, x.data());
        if (refine) {   // one step of iterative refinement on b - J x with the unscaled rows, as the kernel takes it
            std::vector<Row> v(w);
            for (int j = 0; j < S; ++j)
                for (int k = 0; k < NR; ++k) {
                    const double zero[3] = {0, 0, 0};
                    double a[3], b[3], c3[3];
                    mulv3<double>(w[j].A, j >= 1 ? &x[(size_t(j - 1) * NR + k) * 3] : zero, a);
                    mulv3<double>(w[j].B, &x[(size_t(j) * NR + k) * 3], b);
                    mulv3<double>(w[j].C, j + 1 < S ? &x[(size_t(j + 1) * NR + k) * 3] : zero, c3);
                    for (int c = 0; c < 3; ++c) v[j].r[k][c] = w[j].r[k][c] - a[c] - b[c] - c3[c];
                }
            std::vector<double> dx(x.size());
            solve_pass(v, dx.data());
            for (size_t i = 0; i < x.size(); ++i) x[i] += dx[i];
        }
        for (int k = 0; k < NR && d0 + k < n_rhs; ++k)
            for (int j = 0; j < S; ++j)
                for (int c = 0; c < 3; ++c) out[(size_t(d0 + k) * S + j) * 3 + c] = x[(size_t(j) * NR + k) * 3 + c];
    }
}

// One normalisation + level of a row three ways: the unsplit functions above (out_old), the split ones (out_new), and today's
// row3_normalise / row3_level, which must equal the unsplit ones too (return value: 1 if they do, bit for bit).  Outputs [30] =
// A, B, C, r after the level.  me [30] = A, B, C, r; lo, hi [21] = A, C, r of the (already normalised) neighbours.
int rows_old_and_split(const double* me, const double* lo, const double* hi, double* out_old, double* out_new) {
    Row3 w, o;
    std::memcpy(w.A, me, 9 * sizeof(double));
    std::memcpy(w.B, me + 9, 9 * sizeof(double));
    std::memcpy(w.C, me + 18, 9 * sizeof(double));
    std::memcpy(w.r, me + 27, 3 * sizeof(double));
    Row3 v = w, w2 = w, o2;
    unsplit_normalise(w);
    unsplit_level(w, lo, lo + 9, lo + 18, hi, hi + 9, hi + 18, o);
    row3_normalise(w2);
    row3_level(w2, lo, lo + 9, lo + 18, hi, hi + 9, hi + 18, o2);
    const int same = std::memcmp(&o, &o2, sizeof(Row3)) == 0 && std::memcmp(&w, &w2, sizeof(Row3)) == 0;
    std::memcpy(out_old, o.A, 9 * sizeof(double));
    std::memcpy(out_old + 9, o.B, 9 * sizeof(double));
    std::memcpy(out_old + 18, o.C, 9 * sizeof(double));
    std::memcpy(out_old + 27, o.r, 3 * sizeof(double));
    double Bi[9], nA[9], nB[9], nC[9], nr[3];
    row3_normalise_matrix(v.A, v.B, v.C, Bi);
    row3_normalise_rhs(Bi, v.r);
    row3_level_rhs(v.A, v.C, v.r, lo + 18, hi + 18, nr);
    row3_level_matrix(v.A, v.C, lo, lo + 9, hi, hi + 9, nA, nB, nC);
    std::memcpy(out_new, nA, 9 * sizeof(double));
    std::memcpy(out_new + 9, nB, 9 * sizeof(double));
    std::memcpy(out_new + 18, nC, 9 * sizeof(double));
    std::memcpy(out_new + 27, nr, 3 * sizeof(double));
    return same;
}
}
