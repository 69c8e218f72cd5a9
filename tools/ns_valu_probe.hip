// One Newton-Schulz step of k_pf2_algebra_ns at rank <= 16 (P = Z Y, T = a I - b P, Y <- Y T, Z <- T Z), two ways:
//   mfma : the shipped form - 12 v_mfma_f64_16x16x4_f64 + three transposes through LDS (one wave issues such an MFMA every
//          143 cycles on gfx950, tools/mfma64_rate.hip)
//   valu : 192 v_fmac_f64 with the A operand broadcast inside its 16-lane row by DPP (row_newbcast:k - the D layout of the
//          MFMA IS the layout in which row q + 4 v of a matrix sits in DPP row q) and the B operand as a full column per lane,
//          gathered across the four DPP rows through a padded LDS image (4 ds_write_b64 + 8 ds_read_b128 per matrix)
// One wave per workgroup, 1024 workgroups (config 4: one slab per SIMD); prints cycles per step and the difference of the results.
// build: hipcc --offload-arch=gfx950 -O3 tools/ns_valu_probe.hip -o /tmp/ns_valu_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- MFMA form (pf2polar.hip: mm_t / tr_lds at NB = 1)
static __device__ __forceinline__ f64x4 mm_t(const f64x4 &A, const f64x4 &B) {  // A^T B, operands and result in D layout
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[st], B[st], acc, 0, 0, 0);
    return acc;
}
static __device__ __forceinline__ f64x4 tr_lds(const f64x4 &A, double *W, int q, int c16) {
    constexpr int LD = 17;
    f64x4 At;
#pragma unroll
    for (int v = 0; v < 4; ++v) W[(q + 4 * v) * LD + c16] = A[v];
#pragma unroll
    for (int v = 0; v < 4; ++v) At[v] = W[c16 * LD + q + 4 * v];
    return At;
}

// ---- VALU form
#define FM(v, k) "v_fmac_f64_dpp %[c" #v "], %[a" #v "], %[b" #k "] row_newbcast:" #k " row_mask:0xf bank_mask:0xf\n"
#define FMK(k) FM(0, k) FM(1, k) FM(2, k) FM(3, k)
// C = A B: A in D layout (lane (q, p), register v: A[q + 4 v][p]), B as full columns (lane (q, p): B[0..16)[p]); C in D layout
static __device__ __forceinline__ f64x4 mm_dpp(const f64x4 &A, const double (&B)[16]) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    // (s_nop 1: a VGPR written by a VALU instruction must not be read through DPP in the next two slots - the compiler does not
    // see the DPP reads inside this block)
    asm("s_nop 1\n" FMK(0) FMK(1) FMK(2) FMK(3) FMK(4) FMK(5) FMK(6) FMK(7) FMK(8) FMK(9) FMK(10) FMK(11) FMK(12) FMK(13) FMK(14) FMK(15)
        : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3)
        : [a0] "v"(A[0]), [a1] "v"(A[1]), [a2] "v"(A[2]), [a3] "v"(A[3]), [b0] "v"(B[0]), [b1] "v"(B[1]), [b2] "v"(B[2]), [b3] "v"(B[3]),
          [b4] "v"(B[4]), [b5] "v"(B[5]), [b6] "v"(B[6]), [b7] "v"(B[7]), [b8] "v"(B[8]), [b9] "v"(B[9]), [b10] "v"(B[10]),
          [b11] "v"(B[11]), [b12] "v"(B[12]), [b13] "v"(B[13]), [b14] "v"(B[14]), [b15] "v"(B[15]));
    return f64x4{c0, c1, c2, c3};
}
constexpr int GLD = 18;  // doubles per column of the gather image: 144 B - sixteen columns start in sixteen different 16-byte bank groups
static __device__ __forceinline__ void gather_put(const f64x4 &M, double *W, int q, int p) {
#pragma unroll
    for (int v = 0; v < 4; ++v) W[p * GLD + q + 4 * v] = M[v];
}
static __device__ __forceinline__ void gather_get(double (&col)[16], const double *W, int p) {
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        const f64x2 t = *reinterpret_cast<const f64x2 *>(W + p * GLD + k);
        col[k] = t[0], col[k + 1] = t[1];
    }
}

static __device__ __forceinline__ double lcg(unsigned &s) {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) * (1.0 / 16777216.0);
}

// G = M M^T / tr + shift: a well-conditioned SPD start, the same in both kernels (D layout: lane (q, p), register v = G[q + 4 v][p])
static __device__ void make_start(f64x4 &Y, double *W, int q, int p, int slab) {
    unsigned s = 12345u + 977u * slab;
    for (int e = threadIdx.x; e < 256; e += 64) {
        unsigned t = s + 7919u * e;
        W[e] = lcg(t) - 0.5;
    }
    __builtin_amdgcn_s_waitcnt(0);  // (one wave: LDS operations complete in order - no workgroup barrier, the second wave has left)
    double tr = 0.0;
    f64x4 g;
    for (int v = 0; v < 4; ++v) {
        const int i = q + 4 * v;
        double acc = 0.0;
        for (int k = 0; k < 16; ++k) acc += W[i * 16 + k] * W[p * 16 + k];
        g[v] = acc;
    }
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 16; ++k) tr += W[i * 16 + k] * W[i * 16 + k];
    for (int v = 0; v < 4; ++v) Y[v] = g[v] / tr + ((q + 4 * v == p) ? 0.02 : 0.0);
}

// BIG: the register and LDS footprint of the shipped kernel (196 VGPRs, 11.5 KB): does the dispatcher still put one wave on every SIMD?
template <int WAVES, bool BIG = false>
__global__ __launch_bounds__(64 * WAVES) void k_mfma(double *out, long long *ticks, int steps) {
    __shared__ double W[BIG ? 1472 : 16 * 18 * 2];
    if (BIG) {
        asm volatile("v_mov_b32 v195, 0" ::: "v195");
        if (steps < 0) W[1400 + threadIdx.x] = 1.0;
    }
    if (threadIdx.x >= 64) {  // the shipped kernel's second wave (column sums of the L2 ball): a few loads, then done
        if (out[threadIdx.x] == 123.0) ticks[0] = 0;
        return;
    }
    const int lane = threadIdx.x, q = lane >> 4, p = lane & 15;
    f64x4 Y, Yt, Z, Zt;
    make_start(Y, W, q, p, blockIdx.x);
    Yt = tr_lds(Y, W, q, p);
    for (int v = 0; v < 4; ++v) Z[v] = (q + 4 * v == p) ? 1.0 : 0.0;
    Zt = Z;
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < steps; ++it) {
        const f64x4 P = mm_t(Zt, Y);
        const f64x4 Pt = tr_lds(P, W, q, p);
        f64x4 Tm, Tmt;
        for (int v = 0; v < 4; ++v) {
            const double id = (q + 4 * v == p) ? 1.0 : 0.0;
            Tm[v] = 1.5 * id - 0.5 * P[v];
            Tmt[v] = 1.5 * id - 0.5 * Pt[v];
        }
        const f64x4 N1 = mm_t(Yt, Tm);
        const f64x4 N3 = mm_t(Tmt, Z);
        Yt = tr_lds(N1, W, q, p);
        Zt = tr_lds(N3, W, q, p);
        Y = N1, Z = N3;
    }
    const long long t1 = __builtin_readcyclecounter();
    for (int v = 0; v < 4; ++v) out[(long)blockIdx.x * 256 + (q + 4 * v) * 16 + p] = Z[v];
    if (lane == 0) ticks[blockIdx.x] = t1 - t0;
}

__global__ __launch_bounds__(64) void k_valu(double *out, long long *ticks, int steps) {
    __shared__ double W[16 * 18 * 2];
    double *W2 = W + 16 * GLD;
    const int lane = threadIdx.x, q = lane >> 4, p = lane & 15;
    f64x4 Y, Z;
    make_start(Y, W, q, p, blockIdx.x);
    for (int v = 0; v < 4; ++v) Z[v] = (q + 4 * v == p) ? 1.0 : 0.0;
    double Yc[16], Zc[16], Tc[16];
    gather_put(Y, W, q, p);
    gather_put(Z, W2, q, p);
    gather_get(Yc, W, p);
    gather_get(Zc, W2, p);
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < steps; ++it) {
        const f64x4 P = mm_dpp(Z, Yc);
        f64x4 Tm;
        for (int v = 0; v < 4; ++v) Tm[v] = 1.5 * ((q + 4 * v == p) ? 1.0 : 0.0) - 0.5 * P[v];
        gather_put(Tm, W, q, p);
        gather_get(Tc, W, p);
        const f64x4 N3 = mm_dpp(Tm, Zc);  // Z <- T Z first: it does not wait for the gather of T
        gather_put(N3, W2, q, p);
        const f64x4 N1 = mm_dpp(Y, Tc);  // Y <- Y T
        gather_put(N1, W, q, p);
        gather_get(Zc, W2, p);
        gather_get(Yc, W, p);
        Y = N1, Z = N3;
    }
    const long long t1 = __builtin_readcyclecounter();
    for (int v = 0; v < 4; ++v) out[(long)blockIdx.x * 256 + (q + 4 * v) * 16 + p] = Z[v];
    if (lane == 0) ticks[blockIdx.x] = t1 - t0;
}

int main(int argc, char **argv) {
    const int steps = argc > 1 ? atoi(argv[1]) : 12;
    const int blocks = argc > 2 ? atoi(argv[2]) : 1024;  // 2048: two Newton-Schulz waves per SIMD
    double *o1, *o2;
    long long *tk;
    hipMalloc(&o1, (size_t)blocks * 256 * 8);
    hipMalloc(&o2, (size_t)blocks * 256 * 8);
    hipMalloc(&tk, blocks * 8);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {
        for (int which = 0; which < 2; ++which) {
            hipEventRecord(e0);
            for (int i = 0; i < 20; ++i) {
                if (which == 0 && rep == 0) hipLaunchKernelGGL(k_mfma<1>, dim3(blocks), dim3(64), 0, 0, o1, tk, steps);
                else if (which == 0 && rep == 1) hipLaunchKernelGGL((k_mfma<1, true>), dim3(blocks), dim3(64), 0, 0, o1, tk, steps);
                else if (which == 0) hipLaunchKernelGGL(k_mfma<2>, dim3(blocks), dim3(128), 0, 0, o1, tk, steps);
                else hipLaunchKernelGGL(k_valu, dim3(blocks), dim3(64), 0, 0, o2, tk, steps);
            }
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            std::vector<long long> h(blocks);
            hipMemcpy(h.data(), tk, blocks * 8, hipMemcpyDeviceToHost);
            double mn = 1e30, mx = 0, sum = 0;
            int slow = 0;
            for (int b = 0; b < blocks; ++b) mn = fmin(mn, (double)h[b]), mx = fmax(mx, (double)h[b]), sum += (double)h[b];
            for (int b = 0; b < blocks; ++b) slow += (double)h[b] > 1.25 * mn;
            printf("%s%s: %d steps, %.2f us per launch (%d slabs), ticks per step: min %.0f mean %.0f max %.0f; %d of %d slabs more than 25 %% above the fastest\n",
                   which ? "valu" : "mfma", (which == 0 && rep == 2) ? " + a second wave per workgroup" : ((which == 0 && rep == 1) ? " with 196 VGPRs and 11.5 KB of LDS" : ""), steps, ms * 1e3 / 20, blocks, mn / steps,
                   sum / blocks / steps, mx / steps, slow, blocks);
        }
    }
    std::vector<double> a((size_t)blocks * 256), b((size_t)blocks * 256);
    hipMemcpy(a.data(), o1, a.size() * 8, hipMemcpyDeviceToHost);
    hipMemcpy(b.data(), o2, b.size() * 8, hipMemcpyDeviceToHost);
    double num = 0, den = 0, amax = 0;
    for (size_t i = 0; i < a.size(); ++i) num += (a[i] - b[i]) * (a[i] - b[i]), den += a[i] * a[i], amax = fmax(amax, fabs(a[i]));
    printf("Z after %d steps: |mfma - valu| / |mfma| = %.3e (max |Z| %.3e)\n", steps, sqrt(num / den), amax);
    return 0;
}
