// The solver's dependent DPP chains, new against old, bit for bit: the factorisations and triangular solves of csrc/solve_g.h / solve_mf.h
// (16-lane pivot steps as single asm statements, paired group sums in the back substitutions) against frozen copies of the routines as they
// were before the issue slots were filled (ref_*, verbatim), and gsum2 / gsum3 against gsum.  Same arithmetic in another issue order: every
// word must be equal, also the NaN pattern of a matrix whose pivot fails.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -o dpp_chains dpp_chains.hip && ./dpp_chains
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../hsr_env_amd/csrc/solve_mf.h"

// ---- the routines as they were (frozen) ----
template <int G, int NK = G> __device__ __forceinline__ bool ref_chol_g(float (&row)[G], float &invd, int nv, int ndense, int c) {
    asm volatile("" : "+v"(c));          // lane masks formed where they are used, not hoisted out of the caller's loops as spilled SGPR pairs (chol_g_fwd)
    invd = 1.f;
    static_for<0, NK>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < nv) {
            const float ajj = gbcast_after_asm<G, j>(row[j]);
            const float inv = __builtin_amdgcn_rsqf(ajj);            // 1 ulp; the factor only shapes a Newton / Euler solve
            const float lcj = row[j] * inv;                          // lane j: ajj * rsq(ajj) = sqrt(ajj)
            if (c == j) invd = inv;
            row[j] = lcj;
            if (j < ndense) {
                const float nl = -lcj;
                const BcSrc<G> bl = bc_prepare<G>(lcj);
                static_for<j + 1, NK>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    fmac_bcast<G, i, bc_first<G, i, j + 1>()>(row[i], nl, bl);   // row[i] -= lcj * L[i][j]; unconditional: entries i > c are never read
                });
            }
        }
    });
    return chol_pivots_ok<G>(invd);
}
template <int G, int NK = G> __device__ __forceinline__ bool ref_chol_g_fwd(float (&row)[G], float &invd, int nv, int c, float b, float &y) {
    invd = 1.f;
    float sacc = b;
    y = 0.f;
    // the lane id is laundered per call: the thirteen `c == j` masks are then formed where they are used (one v_cmp each) instead of being hoisted out of
    // the Newton loop as SGPR pairs, spilled into VGPR lanes and read back with two v_readlane per step
    asm volatile("" : "+v"(c));
    static_for<0, NK>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < nv) {
            const float ajj = gbcast_after_asm<G, j>(row[j]);
            const float inv = __builtin_amdgcn_rsqf(ajj);
            const float lcj = row[j] * inv;
            const float t = sacc * inv;                               // lane j: y_j
            if (c == j) { invd = inv; y = t; }
            row[j] = lcj;
            const float nl = -lcj;
            const BcSrc<G> bl = bc_prepare<G>(lcj);
            static_for<j + 1, NK>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                fmac_bcast<G, i, bc_first<G, i, j + 1>()>(row[i], nl, bl);
            });
            fmac_bcast<G, j, true>(sacc, nl, bc_prepare<G>(t));      // sacc -= L[c][j] y_j (a lane c <= j has taken its y already: what lands in its sacc is never read)
        }
    });
    return chol_pivots_ok<G>(invd);
}
template <int G, int NK, int ND> __device__ __forceinline__ bool ref_chol_g_tail(float (&row)[G], float &invd, float diag, int c) {
    asm volatile("" : "+v"(c));          // lane masks formed where they are used, not hoisted out of the caller's loops as spilled SGPR pairs (chol_g_fwd)
    invd = 1.f;
    static_for<0, ND>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const float ajj = gbcast_after_asm<G, j>(row[j]);
        const float inv = __builtin_amdgcn_rsqf(ajj);
        const float lcj = row[j] * inv;
        if (c == j) invd = inv;
        row[j] = lcj;
        const float nl = -lcj;
        const BcSrc<G> bl = bc_prepare<G>(lcj);
        static_for<j + 1, ND>([&](auto ic) { constexpr int i = decltype(ic)::value; fmac_bcast<G, i, bc_first<G, i, j + 1>()>(row[i], nl, bl); });
    });
    if (c >= ND) invd = __builtin_amdgcn_rsqf(diag);
    return chol_pivots_ok<G>(invd);
}
template <int G, int NK = G> __device__ __forceinline__ float ref_chol_solve_mf(const float (&row)[G], float invd, float b, int nv, int c) {
    asm volatile("" : "+v"(c));          // lane masks formed where they are used, not hoisted out of the caller's loops as spilled SGPR pairs (chol_g_fwd)
    float nlo[G];                                                // minus the strictly lower part of row c of L, 0 elsewhere
#pragma unroll
    for (int k = 0; k < NK; k++) nlo[k] = (k < c) ? -row[k] : 0.f;
    float sacc = b, y = 0.f;
    static_for<0, NK>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < nv) {
            const float t = sacc * invd;                         // lane j: y_j
            if (c == j) y = t;
            fmac_bcast<G, j, true>(sacc, nlo[j], bc_prepare<G>(t));   // sacc -= L[c][j] y_j
        }
    });
    // L^T x = y: x_j = (y_j - sum_{i > j} L[i][j] x_i) / L[j][j]; the sum runs over lanes (nlo[j] is 0 for lanes i <= j).  Two columns
    // per step: the two group sums over the lanes solved so far run side by side, x_j follows, and column j - 1 only lacks the term of
    // lane j itself, which lane j forms and broadcasts - one reduction latency per two columns of the dependent chain
    float x = 0.f;
    static_for<0, NK / 2>([&](auto jc) {
        constexpr int j = NK - 1 - 2 * decltype(jc)::value;           // columns j and j - 1
        if (j - 1 < nv) {
            const float A = gsum<G>(nlo[j] * x), B = gsum<G>(nlo[j - 1] * x);
            const float xj = (j < nv) ? (y + A) * invd : 0.f;
            if (c == j) x = xj;
            const float t = gbcast<G, j>(nlo[j - 1] * xj);
            if (c == j - 1) x = (y + B + t) * invd;
        }
    });
    if constexpr (NK % 2 == 1) {
        if (0 < nv) { const float tot = gsum<G>(nlo[0] * x); if (c == 0) x = (y + tot) * invd; }
    }
    return x;
}
template <int G, int NK = G> __device__ __forceinline__ float ref_chol_back_mf(const float (&row)[G], float invd, float y, int nv, int c) {
    asm volatile("" : "+v"(c));          // lane masks formed where they are used, not hoisted out of the caller's loops as spilled SGPR pairs (chol_g_fwd)
    float nlo[G];
#pragma unroll
    for (int k = 0; k < NK; k++) nlo[k] = (k < c) ? -row[k] : 0.f;
    float x = 0.f;
    static_for<0, NK / 2>([&](auto jc) {
        constexpr int j = NK - 1 - 2 * decltype(jc)::value;
        if (j - 1 < nv) {
            const float A = gsum<G>(nlo[j] * x), B = gsum<G>(nlo[j - 1] * x);
            const float xj = (j < nv) ? (y + A) * invd : 0.f;
            if (c == j) x = xj;
            const float t = gbcast<G, j>(nlo[j - 1] * xj);
            if (c == j - 1) x = (y + B + t) * invd;
        }
    });
    if constexpr (NK % 2 == 1) {
        if (0 < nv) { const float tot = gsum<G>(nlo[0] * x); if (c == 0) x = (y + tot) * invd; }
    }
    return x;
}
template <int G, int NK, int ND> __device__ __forceinline__ float ref_chol_solve_tail(const float (&row)[G], float invd, float b, int c) {
    asm volatile("" : "+v"(c));          // lane masks formed where they are used, not hoisted out of the caller's loops as spilled SGPR pairs (chol_g_fwd)
    float nlo[ND > 0 ? ND : 1];
#pragma unroll
    for (int k = 0; k < ND; k++) nlo[k] = (k < c && c < ND) ? -row[k] : 0.f;
    float sacc = b, y = 0.f;
    static_for<0, ND>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const float t = sacc * invd;
        if (c == j) y = t;
        fmac_bcast<G, j, true>(sacc, nlo[j], bc_prepare<G>(t));
    });
    float x = 0.f;
    if (c >= ND) x = b * invd * invd;
    static_for<0, ND>([&](auto jc) {
        constexpr int j = ND - 1 - decltype(jc)::value;
        const float tot = (ND <= 16) ? gsum<16>(nlo[j] * x) : gsum<G>(nlo[j] * x);      // the coupled dofs sit in the first DPP row
        if (c == j) x = (y + tot) * invd;
    });
    return x;
}

// ---- the test ----
enum { NMAT = 256, LD = 32 };          // matrices of up to 32 x 32, row-major with leading dimension LD
// MODE 0: chol_g_fwd + chol_back_mf; 1: chol_g_tail + chol_solve_tail; 2: chol_g + chol_solve_mf.  One group of G lanes per matrix, 64 / G
// different matrices per wave.  Record per lane: row[0 .. NK - 1], invd, y, x, pivot check.
template <int G, int NK, int ND, int MODE, bool REF> __global__ void k_chain(const float *A, const float *rhs, unsigned *out) {
    const int g = threadIdx.x / G, c = threadIdx.x % G, mat = blockIdx.x * (64 / G) + g;
    const float *M = A + (size_t)mat * LD * LD;
    float row[G];
#pragma unroll
    for (int k = 0; k < G; k++) row[k] = (c < NK && k < NK) ? M[c * LD + k] : (k == c ? 1.f : 0.f);
    const float b = c < NK ? rhs[mat * LD + c] : 0.f, diag = c < NK ? M[c * LD + c] : 1.f;
    float invd = 0, y = 0, x = 0;
    bool ok;
    if constexpr (MODE == 0) {
        if constexpr (REF) { ok = ref_chol_g_fwd<G, NK>(row, invd, NK, c, b, y); x = ref_chol_back_mf<G, NK>(row, invd, y, NK, c); }
        else { ok = chol_g_fwd<G, NK>(row, invd, NK, c, b, y); x = chol_back_mf<G, NK>(row, invd, y, NK, c); }
    } else if constexpr (MODE == 1) {
        if constexpr (REF) { ok = ref_chol_g_tail<G, NK, ND>(row, invd, diag, c); x = ref_chol_solve_tail<G, NK, ND>(row, invd, b, c); }
        else { ok = chol_g_tail<G, NK, ND>(row, invd, diag, c); x = chol_solve_tail<G, NK, ND>(row, invd, b, c); }
    } else {
        if constexpr (REF) { ok = ref_chol_g<G, NK>(row, invd, NK, NK, c); x = ref_chol_solve_mf<G, NK>(row, invd, b, NK, c); }
        else { ok = chol_g<G, NK>(row, invd, NK, NK, c); x = chol_solve_mf<G, NK>(row, invd, b, NK, c); }
    }
    unsigned *o = out + ((size_t)mat * G + c) * (LD + 4);
#pragma unroll
    for (int k = 0; k < NK; k++) o[k] = __float_as_uint(row[k]);
    o[LD] = __float_as_uint(invd); o[LD + 1] = __float_as_uint(y); o[LD + 2] = __float_as_uint(x); o[LD + 3] = ok ? 1u : 0u;
}
// gsum2 / gsum3 against gsum, in every lane; HALF: every second lane group sits out behind a group-uniform branch
template <int G, bool HALF> __global__ void k_sums(const float *v, unsigned *out) {
    const int l = threadIdx.x, i = blockIdx.x * 64 + l;
    const float a = v[3 * i], b = v[3 * i + 1], c = v[3 * i + 2];
    unsigned *o = out + 8 * (size_t)i;
    for (int k = 0; k < 8; k++) o[k] = 0xdeadbeefu;
    if (HALF && ((l / G) & 1)) return;
    float s2a, s2b, s3a, s3b, s3c;
    gsum2<G>(a, b, s2a, s2b);
    gsum3<G>(a, b, c, s3a, s3b, s3c);
    o[0] = __float_as_uint(gsum<G>(a)); o[1] = __float_as_uint(gsum<G>(b)); o[2] = __float_as_uint(gsum<G>(c));
    o[3] = __float_as_uint(s2a); o[4] = __float_as_uint(s2b); o[5] = __float_as_uint(s3a); o[6] = __float_as_uint(s3b); o[7] = __float_as_uint(s3c);
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)
static unsigned long long rng_ = 0x9E3779B97F4A7C15ull;
static double urand() { rng_ ^= rng_ << 13; rng_ ^= rng_ >> 7; rng_ ^= rng_ << 17; return (double)(rng_ >> 11) / 9007199254740992.0; }

// 256 seeded SPD matrices D (B B^T + I) D, D = column scales over 1e-3 .. 1e3; TAILFROM < n: no off-diagonal entries from that column on.
// Matrix 100 gets a non-positive pivot in the middle.
static void make(std::vector<float> &A, std::vector<float> &rhs, int n, int tailfrom) {
    A.assign((size_t)NMAT * LD * LD, 0.f); rhs.assign((size_t)NMAT * LD, 0.f);
    std::vector<double> B(n * n), d(n);
    for (int m = 0; m < NMAT; m++) {
        for (auto &x : B) x = 2 * urand() - 1;
        for (auto &x : d) x = pow(10.0, 6 * urand() - 3);
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < n; k++) s += B[i * n + k] * B[j * n + k];
            if (i != j && (i >= tailfrom || j >= tailfrom)) s = 0;
            A[((size_t)m * LD + i) * LD + j] = (float)(s * d[i] * d[j]);
        }
        if (m == 100) { const int q = tailfrom < n ? tailfrom / 2 : n / 2; A[((size_t)m * LD + q) * LD + q] *= -1.f; }
        for (int i = 0; i < n; i++) rhs[m * LD + i] = (float)((2 * urand() - 1) * d[i]);
    }
}

template <int G, int NK, int ND, int MODE> static int run(const char *what, int &total) {
    std::vector<float> A, rhs;
    make(A, rhs, NK, MODE == 1 ? ND : NK);
    const size_t nout = (size_t)NMAT * G * (LD + 4);
    float *dA, *dr; unsigned *dn, *df;
    CK(hipMalloc(&dA, A.size() * 4)); CK(hipMalloc(&dr, rhs.size() * 4)); CK(hipMalloc(&dn, nout * 4)); CK(hipMalloc(&df, nout * 4));
    CK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dr, rhs.data(), rhs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dn, 0, nout * 4)); CK(hipMemset(df, 0, nout * 4));
    k_chain<G, NK, ND, MODE, false><<<NMAT / (64 / G), 64>>>(dA, dr, dn);
    k_chain<G, NK, ND, MODE, true><<<NMAT / (64 / G), 64>>>(dA, dr, df);
    CK(hipDeviceSynchronize());
    std::vector<unsigned> hn(nout), hf(nout);
    CK(hipMemcpy(hn.data(), dn, nout * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hf.data(), df, nout * 4, hipMemcpyDeviceToHost));
    int bad = 0, okc = 0, nanx = 0;
    for (int m = 0; m < NMAT; m++) for (int c = 0; c < G; c++) {
        const unsigned *a = &hn[((size_t)m * G + c) * (LD + 4)], *b = &hf[((size_t)m * G + c) * (LD + 4)];
        for (int k = 0; k < LD + 4; k++) {
            if (k < LD && (k >= NK || k > c)) continue;          // entries above the diagonal are scratch
            if (a[k] != b[k]) { if (bad < 8) printf("%s: matrix %d lane %d word %d: %08x, was %08x\n", what, m, c, k, a[k], b[k]); bad++; }
        }
        if (c == 0) okc += a[LD + 3];
        float x; memcpy(&x, &a[LD + 2], 4); if (c < NK && x != x) nanx++;
        // the failed pivot must be seen by both, the sound matrices must pass in both
        if ((a[LD + 3] != 0) != (m != 100) || (b[LD + 3] != 0) != (m != 100)) { if (bad < 8) printf("%s: matrix %d lane %d pivot check %u / %u\n", what, m, c, a[LD + 3], b[LD + 3]); bad++; }
    }
    printf("%-44s %d of %d factorisations pass their pivot check, %d NaN in x, %d words differ\n", what, okc, NMAT, nanx, bad);
    total += bad;
    hipFree(dA); hipFree(dr); hipFree(dn); hipFree(df);
    return 0;
}

template <int G, bool HALF> static int run_sums(const char *what, int &total) {
    const int n = 64 * 16;
    std::vector<float> v(3 * n);
    for (auto &x : v) x = (float)((2 * urand() - 1) * pow(10.0, 6 * urand() - 3));
    float *dv; unsigned *d;
    CK(hipMalloc(&dv, v.size() * 4)); CK(hipMalloc(&d, 8 * n * 4));
    CK(hipMemcpy(dv, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    k_sums<G, HALF><<<n / 64, 64>>>(dv, d);
    CK(hipDeviceSynchronize());
    std::vector<unsigned> h(8 * n);
    CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost));
    int bad = 0, live = 0;
    for (int i = 0; i < n; i++) {
        const unsigned *o = &h[8 * i];
        const bool off = HALF && (((i % 64) / G) & 1);
        if (off) { for (int k = 0; k < 8; k++) bad += o[k] != 0xdeadbeefu; continue; }
        live++;
        bad += (o[3] != o[0]) + (o[4] != o[1]) + (o[5] != o[0]) + (o[6] != o[1]) + (o[7] != o[2]);
        if (i % G) bad += (o[0] != o[-8]) + (o[1] != o[-7]) + (o[2] != o[-6]);          // gsum itself: the same in every lane of the group
    }
    printf("%-44s %d lanes, %d words differ\n", what, live, bad);
    total += bad;
    hipFree(dv); hipFree(d);
    return 0;
}

int main() {
    int total = 0, r = 0;
    r |= run<16, 13, 13, 0>("G16 NK13: chol_g_fwd + chol_back_mf", total);
    r |= run<16, 13, 13, 2>("G16 NK13: chol_g + chol_solve_mf", total);
    r |= run<16, 13, 7, 1>("G16 NK13 ND7: chol_g_tail + chol_solve_tail", total);
    r |= run<32, 25, 25, 0>("G32 NK25: chol_g_fwd + chol_back_mf", total);
    r |= run<32, 25, 25, 2>("G32 NK25: chol_g + chol_solve_mf", total);
    r |= run<32, 25, 7, 1>("G32 NK25 ND7: chol_g_tail + chol_solve_tail", total);
    r |= run_sums<16, false>("G16: gsum2 / gsum3 against gsum", total);
    r |= run_sums<16, true>("G16: ... two of four groups switched off", total);
    r |= run_sums<32, false>("G32: gsum2 / gsum3 against gsum", total);
    r |= run_sums<32, true>("G32: ... one of two groups switched off", total);
    if (r) return r;
    printf("mismatches: %d\n", total);
    return total != 0;
}
