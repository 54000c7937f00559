// cone_eval2 (csrc/solve_g.h) after its outputs stopped being merged across early returns, against a frozen copy of the early-return form:
// all 28 output fields of every row, as 32-bit words.  One point per lane, 64 rows = one wave per block, so the order of the rows decides
// which lanes share a wave (the wave-uniform skip of the middle zone runs both ways); a row that is switched off sits out behind a
// divergent branch, as the lanes without a contact do in eval_at, and keeps its sentinel in both outputs.
//   hipcc <CODEGEN_FLAGS of hsr_env_amd/build.py> -o cone_merge cone_merge.hip && ./cone_merge IN OUT
// IN: n rows of 20 words {float mu, fri[5], D[6], x[6]; int on; int pad}, n a multiple of 64.  OUT: n rows of the product's function, then n rows
// of the frozen one, 28 words each: cost, Dm, k3, zone, g[6], dw[6], gn[6], u[6].  Nothing is compared here: tests/test_gpu_cone_merge.py does.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../hsr_env_amd/csrc/solve_mf.h"

enum { IN_W = 20, OUT_W = 28 };

// ---- frozen: cone_eval2 as it was (zero-initialised outputs, one early return per zone).  Do not edit.
__device__ __forceinline__ void cone_eval2_frozen(int /*dim*/, float mu, const float *fri, const float *D, const float *x, ConeOut &o) {
    float U[6], T2 = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) { o.g[j] = 0; o.dw[j] = 0; o.gn[j] = 0; o.u[j] = 0; }
    o.cost = 0; o.Dm = 0; o.k3 = 0; o.zone = 0;
    U[0] = x[0] * mu;
    const float Nn = U[0];
#pragma unroll
    for (int j = 1; j < 6; j++) { U[j] = x[j] * fri[j - 1]; T2 += U[j] * U[j]; }
    const float T = fsqrt(T2);
    if (Nn >= mu * T || (T <= 0 && Nn >= 0)) return;
    if (mu * Nn + T <= 0 || (T <= 0 && Nn < 0)) {
        o.zone = 1;
#pragma unroll
        for (int j = 0; j < 6; j++) { o.cost += 0.5f * D[j] * x[j] * x[j]; o.g[j] = D[j] * x[j]; o.dw[j] = D[j]; }
        return;
    }
    o.zone = 2;
    const float Dm = D[0] * frcp(mu * mu * (1 + mu * mu)), NT = Nn - mu * T, invT = frcp(T);
    const float kappa = -Dm * NT * mu;
    const bool tiny = T2 < 0x1p-64f;
    const float us = tiny ? 0x1p40f : 1.f, ts = tiny ? 0x1p80f : 1.f;
    o.Dm = Dm; o.k3 = kappa * invT * frcp(T2 * ts);
    o.gn[0] = mu;
#pragma unroll
    for (int j = 1; j < 6; j++) {
        o.gn[j] = -mu * U[j] * fri[j - 1] * invT;
        o.u[j] = fri[j - 1] * U[j] * us;
        o.dw[j] = kappa * fri[j - 1] * fri[j - 1] * invT;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) o.g[j] = Dm * NT * o.gn[j];
    o.cost = 0.5f * Dm * NT * NT;
}

template <bool FROZEN> __global__ void k_cone(const float *in, unsigned *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const float *p = in + IN_W * i;
    unsigned *w = out + OUT_W * i;
#pragma unroll
    for (int k = 0; k < OUT_W; k++) w[k] = 0xdeadbeefu;
    float fri[5], D[6], x[6];
    const float mu = p[0];
#pragma unroll
    for (int j = 0; j < 5; j++) fri[j] = p[1 + j];
#pragma unroll
    for (int j = 0; j < 6; j++) { D[j] = p[6 + j]; x[j] = p[12 + j]; }
    if (__float_as_int(p[18]) != 0) {
        ConeOut o;
        if constexpr (FROZEN) cone_eval2_frozen(0, mu, fri, D, x, o);
        else cone_eval2(0, mu, fri, D, x, o);
        w[0] = __float_as_uint(o.cost); w[1] = __float_as_uint(o.Dm); w[2] = __float_as_uint(o.k3); w[3] = (unsigned)o.zone;
#pragma unroll
        for (int j = 0; j < 6; j++) { w[4 + j] = __float_as_uint(o.g[j]); w[10 + j] = __float_as_uint(o.dw[j]); w[16 + j] = __float_as_uint(o.gn[j]); w[22 + j] = __float_as_uint(o.u[j]); }
    }
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 1; }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 1; }
    fseek(fi, 0, SEEK_END);
    const long size = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    if (size <= 0 || size % (64 * IN_W * 4) != 0) { fprintf(stderr, "%s: not a whole number of 64-row blocks\n", argv[1]); return 1; }
    std::vector<uint32_t> in(size / 4);
    if (fread(in.data(), 1, size, fi) != (size_t)size) { fprintf(stderr, "%s: short read\n", argv[1]); return 1; }
    fclose(fi);
    const size_t n = in.size() / IN_W;
    void *din, *dout;
    CK(hipMalloc(&din, in.size() * 4));
    CK(hipMalloc(&dout, 2 * n * OUT_W * 4));
    CK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0, 2 * n * OUT_W * 4));
    k_cone<false><<<n / 64, 64>>>((const float *)din, (unsigned *)dout);
    CK(hipGetLastError());
    k_cone<true><<<n / 64, 64>>>((const float *)din, (unsigned *)dout + n * OUT_W);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(2 * n * OUT_W);
    CK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(din));
    CK(hipFree(dout));
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 1; }
    fwrite(out.data(), 4, out.size(), fo);
    if (fclose(fo) != 0) { perror(argv[2]); return 1; }
    printf("cone_merge: %zu rows\n", n);
    return 0;
}
