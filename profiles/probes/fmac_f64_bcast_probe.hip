// probe: issue cost and latency of v_fmac_f64 with a DPP row_newbcast source against the plain VOP2 form on gfx950.
// Per wave, s_memtime around ITERS x UNROLL instructions: NACC independent accumulators (issue rate) or one (dependent chain,
// latency), plain / broadcast / 1:1 mix, at one and at two waves per SIMD (workgroups of 4 / 8 waves, one workgroup per CU).
// The s_memtime tick is calibrated against HIP events of the same launch (ticks per ns are printed with every line).
// Build: hipcc --offload-arch=gfx950 -O3 -o fmac_f64_bcast_probe fmac_f64_bcast_probe.hip     Run once, under a time limit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(call) do { if ((call) != hipSuccess) { printf("HIP error at line %d\n", __LINE__); exit(1); } } while (0)

enum { PLAIN = 0, BCAST = 1, MIX = 2 };
constexpr int UNROLL = 96, ITERS = 2000;

#define FMAC_PLAIN(acc, tab, x) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(acc) : "v"(tab), "v"(x))
#define FMAC_BCAST(acc, tab, x, n) \
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #n " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(tab), "v"(x))

template <int MODE, int NACC>
__global__ void __launch_bounds__(512) probe(unsigned long long* ticks, double* sink, double x0, double t0) {
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = double(i);
    const double x = x0 + 1e-3 * threadIdx.x;
    double tab = t0 * double((threadIdx.x & 15) + 1);   // constant k in lane k of every 16-lane row
    asm volatile("" : "+v"(tab));                        // (written here, well ahead of the first DPP read)
    __builtin_amdgcn_s_barrier();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            double& a = acc[u % NACC];
            const bool b = MODE == BCAST || (MODE == MIX && (u & 1));
            if (!b) FMAC_PLAIN(a, tab, x);
            else if (u % 3 == 0) FMAC_BCAST(a, tab, x, 3);
            else if (u % 3 == 1) FMAC_BCAST(a, tab, x, 9);
            else FMAC_BCAST(a, tab, x, 14);
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double s = 0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i];
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    sink[gt] = s;
    if ((threadIdx.x & 63) == 0) ticks[gt >> 6] = c1 - c0;
}

// one lane's check of what the broadcast form computes: acc + tab[lane n of the row] * x
__global__ void check(double* out) {
    double acc = 1.0, x = 2.0 + threadIdx.x;
    double tab = 100.0 * double(threadIdx.x);
    asm volatile("" : "+v"(tab));
    __builtin_amdgcn_s_barrier();
    double neg = acc;
    FMAC_BCAST(acc, tab, x, 5);
    asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(neg) : "v"(tab), "v"(x));
    out[threadIdx.x] = acc;
    out[64 + threadIdx.x] = neg;
}

template <int MODE, int NACC>
void run(const char* name, int waves_per_simd, unsigned long long* d_ticks, double* d_sink) {
    const int cus = 256, threads = 256 * waves_per_simd, nwaves = cus * threads / 64;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    probe<MODE, NACC><<<cus, threads>>>(d_ticks, d_sink, 1.0, 1e-9);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    probe<MODE, NACC><<<cus, threads>>>(d_ticks, d_sink, 1.0, 1e-9);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> t(nwaves);
    CK(hipMemcpy(t.data(), d_ticks, sizeof(unsigned long long) * nwaves, hipMemcpyDeviceToHost));
    std::sort(t.begin(), t.end());
    const double n = double(ITERS) * UNROLL, med = double(t[nwaves / 2]);
    printf("%-22s NACC=%2d waves/SIMD=%d: %8.3f ticks per instruction per wave (min %.3f max %.3f), launch %.3f ms = %.3f ns per "
           "instruction per wave, %.4f ticks per ns\n", name, NACC, waves_per_simd, med / n, double(t.front()) / n, double(t.back()) / n,
           ms, ms * 1e6 / n, med / (ms * 1e6));
}

int main() {
    unsigned long long* d_ticks;
    double* d_sink;
    CK(hipMalloc(&d_ticks, sizeof(unsigned long long) * 256 * 8));
    CK(hipMalloc(&d_sink, sizeof(double) * 256 * 512));
    {
        double h[128];
        check<<<1, 64>>>(d_sink);
        CK(hipMemcpy(h, d_sink, sizeof(h), hipMemcpyDeviceToHost));
        int bad = 0;
        for (int l = 0; l < 64; ++l) {
            const double c = 100.0 * double((l & ~15) + 5), x = 2.0 + l;
            if (h[l] != 1.0 + c * x || h[64 + l] != 1.0 - c * x) ++bad;
        }
        printf("row_newbcast:5 semantics (lane l reads lane 16*(l/16)+5, neg modifier): %s\n", bad ? "WRONG" : "ok");
        if (bad) return 2;
    }
    for (int w = 1; w <= 2; ++w) {
        run<PLAIN, 16>("independent plain", w, d_ticks, d_sink);
        run<BCAST, 16>("independent broadcast", w, d_ticks, d_sink);
        run<MIX, 16>("independent 1:1 mix", w, d_ticks, d_sink);
        run<PLAIN, 1>("dependent plain", w, d_ticks, d_sink);
        run<BCAST, 1>("dependent broadcast", w, d_ticks, d_sink);
        run<MIX, 1>("dependent 1:1 mix", w, d_ticks, d_sink);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
}
