// support<8> / mpr_penetration<8> (csrc/collide.h) against a frozen copy of the form they had before the geom type masks, the bound_ctrl DPP
// moves and the scan whose slots past the end of a hull count as vertex 0: one convex pair per 8-lane sub-group, eight different pairs per wave, and every output as 32-bit words.  A pair that is switched off sits
// out behind a divergent branch, as the sub-groups without an item do in the persistent kernel, and keeps its sentinel in every output.
//   hipcc <CODEGEN_FLAGS of hsr_env_amd/build.py> -o mpr_frozen mpr_frozen.hip && ./mpr_frozen PAIRS VERTS OUT
// PAIRS: n rows of 48 words, n a multiple of 8:
//   int   type1 nvert1 voff1 type2 nvert2 voff2 warm[3] on            (voff: first float4 of the hull in VERTS; warm: Sup::id + 1 of a portal, 0 = none)
//   float pos1[3] mat1[9] size1[3] pos2[3] mat2[9] size2[3] d[3]      (d: the direction of the two plain support calls, as the margin rescan makes them)
//   5 words of padding
// VERTS: float4 hull vertices.  OUT: three blocks of n rows of 24 words - the product's functions with the masks of a model whose first geoms are boxes,
// cylinders and meshes and whose second geoms are boxes and meshes (every committed configuration), the product's functions with any type allowed
// (the generic instances), the frozen functions:
//   hit depth dir[3] pos[3] sep[3] nsup warm[3] | support(G1, d)[3] support(G2, -d)[3] | 3 words of padding
// (depth, dir, pos are written only on a hit, as their caller reads them.)  Nothing is compared here: tests/test_gpu_mpr_frozen.py does.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../hsr_env_amd/csrc/collide.h"

enum { IN_W = 48, OUT_W = 24 };

// ---- frozen: the support function and the portal refinement as they were (four type arms at every call site, DPP moves without bound_ctrl, a bound test in the scan's compare).  Do not edit.
template <int W> __device__ __forceinline__ void sup_merge_frozen(float &b, int &idx, float pb, int pi) {
    // bitwise, not short-circuit: `a || (b && c)` came back from the compiler as two nested exec-mask branches per merge step
    const bool take = (pb > b) | ((pb == b) & (pi < idx));
    b = take ? pb : b; idx = take ? pi : idx;
}
__device__ __forceinline__ v3 support_vertex_frozen(const Geom &G, int vid) {
    v3 loc;
    if (G.type == GEOM_BOX) loc = mk3((vid & 1) ? G.size.x : -G.size.x, (vid & 2) ? G.size.y : -G.size.y, (vid & 4) ? G.size.z : -G.size.z);
    else { const float4 w = G.verts[vid]; loc = mk3(w.x, w.y, w.z); }
    return mulmv(G.mat, loc) + G.pos;
}
template <int W = 1> __device__ __forceinline__ v3 support_frozen(const Geom &G, v3 dir, int *vid = nullptr) {
    const v3 dl = mulmtv(G.mat, dir);
    v3 loc;
    if (vid) *vid = VID_NONE;
    if (G.type == GEOM_BOX) {
        loc = mk3(dl.x > 0 ? G.size.x : -G.size.x, dl.y > 0 ? G.size.y : -G.size.y, dl.z > 0 ? G.size.z : -G.size.z);
        if (vid) *vid = (dl.x > 0 ? 1 : 0) | (dl.y > 0 ? 2 : 0) | (dl.z > 0 ? 4 : 0);
    } else if (G.type == GEOM_CYLINDER) {
        const float r2 = dl.x * dl.x + dl.y * dl.y, ir = frsq(r2);
        if (r2 > HSR_MINVAL * HSR_MINVAL) { loc.x = dl.x * ir * G.size.x; loc.y = dl.y * ir * G.size.x; } else { loc.x = 0; loc.y = 0; }
        loc.z = dl.z > 0 ? G.size.y : -G.size.y;
    } else if (G.type == GEOM_SPHERE) {
        loc = normalized(dl) * G.size.x;
    } else {
        // mesh hull: exhaustive search, first maximum wins (same tie-break as a sequential scan).  Two independent
        // (value, index) chains over even/odd vertices give the VALU two dependency chains; the winning vertex is
        // fetched once at the end.  Vertices are LDS broadcast reads.
      if constexpr (W > 1) {
        const int sub = threadIdx.x & (W - 1);
        float b = -3.0e38f;
        int idx = 0x7fffffff;
        // the sub-group scans are only used by the persistent kernel: the hulls of the deepest links (the fingers) are staged in LDS, the others stay in
        // global memory (kin2.h: geom_cached3), so these are generic (flat) loads - a global_load here measured no faster (round 4)
        const float *gverts = (const float *)G.verts;
        auto gvert = [&](int i) { return make_float4(gverts[4 * i], gverts[4 * i + 1], gverts[4 * i + 2], 0.f); };
        for (int i0 = 0; i0 < G.nvert; i0 += 4 * W) {
            float4 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = i0 + u * W + sub; q[u] = gvert(i < G.nvert ? i : 0); }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * W + sub;
                const float t = q[u].x * dl.x + q[u].y * dl.y + q[u].z * dl.z;
                if (i < G.nvert && t > b) { b = t; idx = i; }
            }
        }
        sup_merge_frozen<W>(b, idx, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), 0xB1, 0xf, 0xf, false)), __builtin_amdgcn_update_dpp(0, idx, 0xB1, 0xf, 0xf, false));
        if constexpr (W >= 4) sup_merge_frozen<W>(b, idx, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), 0x4E, 0xf, 0xf, false)), __builtin_amdgcn_update_dpp(0, idx, 0x4E, 0xf, 0xf, false));
        if constexpr (W >= 8) sup_merge_frozen<W>(b, idx, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), 0x141, 0xf, 0xf, false)), __builtin_amdgcn_update_dpp(0, idx, 0x141, 0xf, 0xf, false));
        if constexpr (W >= 16) sup_merge_frozen<W>(b, idx, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), 0x140, 0xf, 0xf, false)), __builtin_amdgcn_update_dpp(0, idx, 0x140, 0xf, 0xf, false));
        const float4 w = gvert(G.nvert > 0 ? idx : 0);
        loc = mk3(w.x, w.y, w.z);
        if (vid) *vid = G.nvert > 0 ? idx : 0;
      } else {
        float bA = -3.0e38f, bB = -3.0e38f;
        int iA = 0, iB = 1;
        int i = 0;
        for (; i + 8 <= G.nvert; i += 8) {
            // 8 vertex loads in flight before the first use (the table may live in global memory / L1)
            float4 q[8];
#pragma unroll
            for (int u = 0; u < 8; u++) q[u] = G.verts[i + u];
#pragma unroll
            for (int u = 0; u < 8; u += 2) {
                const float ta = q[u].x * dl.x + q[u].y * dl.y + q[u].z * dl.z, tb = q[u + 1].x * dl.x + q[u + 1].y * dl.y + q[u + 1].z * dl.z;
                iA = ta > bA ? i + u : iA; bA = fmaxf(bA, ta);
                iB = tb > bB ? i + u + 1 : iB; bB = fmaxf(bB, tb);
            }
        }
        for (; i < G.nvert; i++) {
            const float4 a = G.verts[i];
            const float t = a.x * dl.x + a.y * dl.y + a.z * dl.z;
            if (i & 1) { iB = t > bB ? i : iB; bB = fmaxf(bB, t); } else { iA = t > bA ? i : iA; bA = fmaxf(bA, t); }
        }
        const int best = (bB > bA || (bB == bA && iB < iA)) ? iB : iA;
        const float4 w = G.verts[G.nvert > 0 ? best : 0];
        loc = mk3(w.x, w.y, w.z);
        if (vid) *vid = G.nvert > 0 ? best : 0;
      }
    }
    return mulmv(G.mat, loc) + G.pos;
}
template <int W = 1> __device__ __forceinline__ Sup mpr_support_frozen(const Geom &G1, const Geom &G2, v3 dir) {
    Sup s;
    int i1, i2;
    s.v1 = support_frozen<W>(G1, dir, &i1);
    s.v2 = support_frozen<W>(G2, -dir, &i2);
    s.id = i1 | (i2 << VID_BITS);
    s.v = s.v1 - s.v2;
    return s;
}
__device__ __forceinline__ float point_seg_dist2_frozen(v3 x0, v3 b, v3 &wit) {   // P = origin
    const v3 d = b - x0;
    const float t = -dot(x0, d) / dot(d, d);
    if (t < 0 || fabsf(t) < 1e-30f) wit = x0;
    else if (t >= 1) wit = b;
    else wit = x0 + d * t;
    return dot(wit, wit);
}
// libccd's ccdVec3PointTriDist2 for P = origin.  fp32 note: libccd's expanded quadratic form
// s^2 v + t^2 w + 2 s t r + 2 s p + 2 t q + u cancels catastrophically in fp32 (u ~ 0.1, result ~ 1e-8),
// so the interior case only reports `interior` and the caller measures the depth along the portal normal.
__device__ __forceinline__ float point_tri_dist2_frozen(v3 x0, v3 B, v3 Cc, v3 &wit, bool &interior) {
    const v3 d1 = B - x0, d2 = Cc - x0, a = x0;
    const float v = dot(d1, d1), w = dot(d2, d2), p = dot(a, d1), q = dot(a, d2), r = dot(d1, d2);
    const float den = w * v - r * r;
    float sx = -1, t = -1;
    interior = false;
    if (fabsf(den) > 0) { sx = (q * r - w * p) / den; t = (-sx * r - q) / w; }
    if (sx >= 0 && sx <= 1 && t >= 0 && t <= 1 && t + sx <= 1) {
        wit = x0 + d1 * sx + d2 * t;
        interior = true;
        return dot(wit, wit);
    }
    v3 w2;
    float best = point_seg_dist2_frozen(x0, B, wit);
    float dist = point_seg_dist2_frozen(x0, Cc, w2);
    if (dist < best) { best = dist; wit = w2; }
    dist = point_seg_dist2_frozen(B, Cc, w2);
    if (dist < best) { best = dist; wit = w2; }
    return best;
}
__device__ __forceinline__ v3 portal_dir_frozen(const Sup &p1, const Sup &p2, const Sup &p3) {
    return normalized(cross(p2.v - p1.v, p3.v - p1.v));
}
// branch-free selects keep the portal in registers (struct assignment under divergent ifs made the compiler
// place the three portal points in a scratch array with dynamic indexing: every MPR step went through memory)
__device__ __forceinline__ Sup selS_frozen(bool c, const Sup &a, const Sup &b) {
    Sup r;
    r.v = sel3(c, a.v, b.v); r.v1 = sel3(c, a.v1, b.v1); r.v2 = sel3(c, a.v2, b.v2); r.id = c ? a.id : b.id;
    return r;
}
__device__ __forceinline__ void expand_portal_frozen(const Sup &p0, Sup &p1, Sup &p2, Sup &p3, const Sup &v4) {
    const v3 v4v0 = cross(v4.v, p0.v);
    const bool d1 = dot(p1.v, v4v0) > 0, d2 = dot(p2.v, v4v0) > 0, d3 = dot(p3.v, v4v0) > 0;
    // d1: (d2 ? p1 : p3) <- v4 ; !d1: (d3 ? p2 : p1) <- v4
    const bool w1 = (d1 && d2) || (!d1 && !d3), w2 = !d1 && d3, w3 = d1 && !d2;
    p1 = selS_frozen(w1, v4, p1); p2 = selS_frozen(w2, v4, p2); p3 = selS_frozen(w3, v4, p3);
}
__device__ __forceinline__ bool reach_tol_frozen(const Sup &p1, const Sup &p2, const Sup &p3, const Sup &v4, v3 dir, float tol) {
    const float dv4 = dot(v4.v, dir);
    const float mn = fminf(fminf(dv4 - dot(p1.v, dir), dv4 - dot(p2.v, dir)), dv4 - dot(p3.v, dir));
    return mn < tol;
}

// returns true on penetration; otherwise `sep` is a proven separating direction of the Minkowski difference
// (support_frozen(A-B, sep) . sep < 0) or zero when MPR gave up without one
// warm: in: the vertex ids of last substep's final portal of this pair (three Sup::id, 0 = none); out: this run's.
// The same six material points, placed with the present poses, are a portal again whenever the origin ray still passes through their
// triangle (checked; else the search starts from scratch): the refinement then confirms the face it ended on last time with one or
// two support calls instead of rediscovering it with eight.
template <int W = 1> __device__ __forceinline__ bool mpr_penetration_frozen(const Geom &G1, const Geom &G2, float tol, int maxit, float &depth, v3 &dirout, v3 &pos, v3 &sep, int &nsup, int *warm = nullptr) {
    const float eps = HSR_EPS;
    Sup p0, p1, p2, p3, v4;
    p0.v1 = G1.pos; p0.v2 = G2.pos; p0.v = p0.v1 - p0.v2; p0.id = 0;
    if (fabsf(p0.v.x) < eps && fabsf(p0.v.y) < eps && fabsf(p0.v.z) < eps) p0.v.x += 1e-5f;
    v3 dir = normalized(-p0.v);
    sep = mk3(0, 0, 0);
    nsup = 0;
    bool warm_ok = false;
    if (warm && warm[0] > 0) {
        auto rebuild = [&](int id, Sup &p) { p.id = id; p.v1 = support_vertex_frozen(G1, id & VID_NONE); p.v2 = support_vertex_frozen(G2, (id >> VID_BITS) & VID_NONE); p.v = p.v1 - p.v2; };
        rebuild(warm[0] - 1, p1); rebuild(warm[1] - 1, p2); rebuild(warm[2] - 1, p3);
        // the ray from p0 through the origin crosses the triangle, with the winding the refinement expects (the three tests of the
        // portal discovery below), by a clear margin
        const float m1 = 1e-4f * norm(p0.v);
        const float s13 = dot(cross(p1.v, p3.v), p0.v), s32 = dot(cross(p3.v, p2.v), p0.v), s21 = dot(cross(p2.v, p1.v), p0.v);
        const float sc = fmaxf(fmaxf(dot(p1.v, p1.v), dot(p2.v, p2.v)), dot(p3.v, p3.v)) * m1;
        warm_ok = s13 > sc && s32 > sc && s21 > sc;
    }
    if (warm) { warm[0] = warm[1] = warm[2] = 0; }
  cold_start:
  if (!warm_ok) {
    p1 = mpr_support_frozen<W>(G1, G2, dir); nsup++;
    if (dot(p1.v, dir) < eps) { sep = dir; return false; }
    dir = cross(p0.v, p1.v);
    if (dot(dir, dir) < eps * eps) {
        const float l1 = norm(p1.v);
        if (l1 < eps) return false;
        depth = l1; dirout = normalized(p1.v); pos = (p1.v1 + p1.v2) * 0.5f;
        return true;
    }
    dir = normalized(dir);
    p2 = mpr_support_frozen<W>(G1, G2, dir); nsup++;
    if (dot(p2.v, dir) < eps) { sep = dir; return false; }
    dir = normalized(cross(p1.v - p0.v, p2.v - p0.v));
    {
        const bool sw = dot(dir, p0.v) > 0;
        const Sup t1 = selS_frozen(sw, p2, p1), t2 = selS_frozen(sw, p1, p2);
        p1 = t1; p2 = t2; dir = sel3(sw, -dir, dir);
    }
    for (int it = 0;; it++) {
        if (it > 100) return false;
        p3 = mpr_support_frozen<W>(G1, G2, dir); nsup++;
        if (dot(p3.v, dir) < eps) { sep = dir; return false; }
        const bool c1 = dot(cross(p1.v, p3.v), p0.v) < -eps;
        const bool c2 = !c1 && dot(cross(p3.v, p2.v), p0.v) < -eps;
        p2 = selS_frozen(c1, p3, p2);
        p1 = selS_frozen(c2, p3, p1);
        if (!(c1 || c2)) break;
        dir = normalized(cross(p1.v - p0.v, p2.v - p0.v));
    }
  }
    for (int it = 0;; it++) {
        dir = portal_dir_frozen(p1, p2, p3);
        if (dot(dir, p1.v) >= -eps) break;
        v4 = mpr_support_frozen<W>(G1, G2, dir); nsup++;
        if (dot(v4.v, dir) < -eps) { sep = dir; return false; }
        if (reach_tol_frozen(p1, p2, p3, v4, dir, tol) || it > maxit) return false;
        expand_portal_frozen(p0, p1, p2, p3, v4);
    }
    for (int it = 0;; it++) {
        dir = portal_dir_frozen(p1, p2, p3);
        v4 = mpr_support_frozen<W>(G1, G2, dir); nsup++;
        if (reach_tol_frozen(p1, p2, p3, v4, dir, tol) || it > maxit) {
            v3 pdir;
            bool interior;
            depth = fsqrt(point_tri_dist2_frozen(p1.v, p2.v, p3.v, pdir, interior));
            // Where the origin projects into the final triangle, depth and direction are those of the face's plane - the same for every
            // triangle of that face, however the run got there.  Where it does not, libccd measures to the triangle's edge and the answer
            // depends on the triangle: a warm-started run then starts over from scratch, so that it ends where libccd's own search does
            // (as far as single precision follows it).
            if (!interior && warm_ok) { warm_ok = false; dir = normalized(-p0.v); goto cold_start; }
            if (interior) {
                // the witness is the foot of the perpendicular: depth = |n . v1|, direction = +-n
                const float dn = dot(dir, p1.v);
                depth = fabsf(dn);
                dirout = dn >= 0 ? dir : -dir;
            } else {
                if (fabsf(pdir.x) < eps && fabsf(pdir.y) < eps && fabsf(pdir.z) < eps) pdir = dir;
                dirout = normalized(pdir);
            }
            // mpr_find_pos
            float b0 = dot(cross(p1.v, p2.v), p3.v), b1 = dot(cross(p3.v, p2.v), p0.v);
            float b2 = dot(cross(p0.v, p1.v), p3.v), b3 = dot(cross(p2.v, p1.v), p0.v);
            float sum = b0 + b1 + b2 + b3;
            if (sum <= 0) {
                b0 = 0; b1 = dot(cross(p2.v, p3.v), dir); b2 = dot(cross(p3.v, p1.v), dir); b3 = dot(cross(p1.v, p2.v), dir);
                sum = b1 + b2 + b3;
            }
            const float inv = 0.5f * frcp(sum);
            pos = (p0.v1 * b0 + p1.v1 * b1 + p2.v1 * b2 + p3.v1 * b3 + p0.v2 * b0 + p1.v2 * b1 + p2.v2 * b2 + p3.v2 * b3) * inv;
            // the portal this run ended on, for the next substep - only vertices carry over (mesh, box)
            auto vertex_ids = [](int id) { return (id & VID_NONE) != VID_NONE && ((id >> VID_BITS) & VID_NONE) != VID_NONE; };
            // (only from a run whose witness was interior: one that ended on a triangle edge would be started over next time anyway)
            if (warm && interior && vertex_ids(p1.id) && vertex_ids(p2.id) && vertex_ids(p3.id)) { warm[0] = p1.id + 1; warm[1] = p2.id + 1; warm[2] = p3.id + 1; }
            return true;
        }
        expand_portal_frozen(p0, p1, p2, p3, v4);
    }
}
// ---- end of the frozen copy

enum { MODE_MASKED = 0, MODE_ANY = 1, MODE_FROZEN = 2 };
constexpr int TM_FIRST = (1 << GEOM_BOX) | (1 << GEOM_CYLINDER) | (1 << GEOM_MESH), TM_SECOND = (1 << GEOM_BOX) | (1 << GEOM_MESH);

__device__ __forceinline__ Geom read_geom(const unsigned *pi, const float *pf, const float4 *verts) {
    Geom G;
    G.type = (int)pi[0]; G.nvert = (int)pi[1];
    G.verts = G.type == GEOM_MESH ? verts + pi[2] : nullptr;
    G.pos = mk3(pf[0], pf[1], pf[2]);
#pragma unroll
    for (int k = 0; k < 9; k++) G.mat.a[k] = pf[3 + k];
    G.size = mk3(pf[12], pf[13], pf[14]);
    G.bc = G.pos; G.bh = G.size;
    return G;
}

template <int MODE> __global__ void k_mpr(const unsigned *in, const float4 *verts, unsigned *out) {
    const size_t pair = (size_t)blockIdx.x * 8 + threadIdx.x / 8;
    const unsigned *p = in + IN_W * pair;
    const float *pf = reinterpret_cast<const float *>(p) + 10;
    unsigned *w = out + OUT_W * pair;
    if ((threadIdx.x & 7) == 0) {
#pragma unroll
        for (int k = 0; k < OUT_W; k++) w[k] = 0xdeadbeefu;
    }
    const Geom A = read_geom(p, pf, verts), B = read_geom(p + 3, pf + 15, verts);
    const v3 d = mk3(pf[30], pf[31], pf[32]);
    int wid[3] = {(int)p[6], (int)p[7], (int)p[8]};
    if (p[9] != 0) {
        float depth = 0; v3 dir = mk3(0, 0, 0), pos = mk3(0, 0, 0), sep;
        int nsup = 0;
        bool hit;
        v3 s1, s2;
        if constexpr (MODE == MODE_FROZEN) {
            hit = mpr_penetration_frozen<8>(A, B, 1e-6f, 50, depth, dir, pos, sep, nsup, wid);
            s1 = support_frozen<8>(A, d); s2 = support_frozen<8>(B, -d);
        } else if constexpr (MODE == MODE_ANY) {
            hit = mpr_penetration<8>(A, B, 1e-6f, 50, depth, dir, pos, sep, nsup, wid);
            s1 = support<8>(A, d); s2 = support<8>(B, -d);
        } else {
            hit = mpr_penetration<8, TM_FIRST, TM_SECOND>(A, B, 1e-6f, 50, depth, dir, pos, sep, nsup, wid);
            s1 = support<8, TM_FIRST>(A, d); s2 = support<8, TM_SECOND>(B, -d);
        }
        if ((threadIdx.x & 7) == 0) {
            w[0] = hit ? 1u : 0u;
            if (hit) { w[1] = __float_as_uint(depth); w[2] = __float_as_uint(dir.x); w[3] = __float_as_uint(dir.y); w[4] = __float_as_uint(dir.z);
                       w[5] = __float_as_uint(pos.x); w[6] = __float_as_uint(pos.y); w[7] = __float_as_uint(pos.z); }
            else { for (int k = 1; k < 8; k++) w[k] = 0; }
            w[8] = __float_as_uint(sep.x); w[9] = __float_as_uint(sep.y); w[10] = __float_as_uint(sep.z);
            w[11] = (unsigned)nsup; w[12] = (unsigned)wid[0]; w[13] = (unsigned)wid[1]; w[14] = (unsigned)wid[2];
            w[15] = __float_as_uint(s1.x); w[16] = __float_as_uint(s1.y); w[17] = __float_as_uint(s1.z);
            w[18] = __float_as_uint(s2.x); w[19] = __float_as_uint(s2.y); w[20] = __float_as_uint(s2.z);
            w[21] = w[22] = w[23] = 0;
        }
    }
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

static bool read_words(const char *path, std::vector<uint32_t> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (size <= 0 || size % 4 != 0) { fprintf(stderr, "%s: empty or not whole words\n", path); fclose(f); return false; }
    v.resize(size / 4);
    const bool ok = fread(v.data(), 1, size, f) == (size_t)size;
    fclose(f);
    if (!ok) fprintf(stderr, "%s: short read\n", path);
    return ok;
}

// every index the kernels will form stays inside VERTS: hull ranges, and the vertex ids of a warm portal (which only pairs of boxes and meshes carry)
static bool rows_in_bounds(const std::vector<uint32_t> &in, size_t n, size_t nverts) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t *p = in.data() + IN_W * i;
        bool vertex_shapes = true;
        for (int side = 0; side < 2; side++) {
            const uint32_t type = p[3 * side], nv = p[3 * side + 1], off = p[3 * side + 2];
            if (type != GEOM_BOX && type != GEOM_CYLINDER && type != GEOM_MESH) { fprintf(stderr, "row %zu: geom type %u\n", i, type); return false; }
            if (type == GEOM_MESH ? (nv < 1 || nv > 256 || (size_t)off + nv > nverts) : nv != 0) { fprintf(stderr, "row %zu: hull range\n", i); return false; }
            if (type == GEOM_CYLINDER) vertex_shapes = false;
        }
        for (int k = 0; k < 3; k++) {
            const uint32_t wv = p[6 + k];
            if (wv == 0) continue;
            if (!vertex_shapes || wv > (1u << (2 * VID_BITS))) { fprintf(stderr, "row %zu: warm id on a pair without vertices\n", i); return false; }
            const uint32_t id = wv - 1, i1 = id & VID_NONE, i2 = (id >> VID_BITS) & VID_NONE;
            if (i1 >= (p[0] == GEOM_BOX ? 8u : p[1]) || i2 >= (p[3] == GEOM_BOX ? 8u : p[4])) { fprintf(stderr, "row %zu: warm vertex id out of range\n", i); return false; }
        }
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s PAIRS VERTS OUT\n", argv[0]); return 1; }
    std::vector<uint32_t> in, vt;
    if (!read_words(argv[1], in) || !read_words(argv[2], vt)) return 1;
    if (in.size() % (8 * IN_W) != 0 || vt.size() % 4 != 0) { fprintf(stderr, "not a whole number of 8-pair waves / float4 vertices\n"); return 1; }
    const size_t n = in.size() / IN_W, nverts = vt.size() / 4;
    if (!rows_in_bounds(in, n, nverts)) return 1;
    void *din, *dvt, *dout;
    CK(hipMalloc(&din, in.size() * 4));
    CK(hipMalloc(&dvt, vt.size() * 4));
    CK(hipMalloc(&dout, 3 * n * OUT_W * 4));
    CK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dvt, vt.data(), vt.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0, 3 * n * OUT_W * 4));
    k_mpr<MODE_MASKED><<<n / 8, 64>>>((const unsigned *)din, (const float4 *)dvt, (unsigned *)dout);
    CK(hipGetLastError());
    k_mpr<MODE_ANY><<<n / 8, 64>>>((const unsigned *)din, (const float4 *)dvt, (unsigned *)dout + n * OUT_W);
    CK(hipGetLastError());
    k_mpr<MODE_FROZEN><<<n / 8, 64>>>((const unsigned *)din, (const float4 *)dvt, (unsigned *)dout + 2 * n * OUT_W);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(3 * n * OUT_W);
    CK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(din));
    CK(hipFree(dvt));
    CK(hipFree(dout));
    FILE *fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 1; }
    fwrite(out.data(), 4, out.size(), fo);
    if (fclose(fo) != 0) { perror(argv[3]); return 1; }
    printf("mpr_frozen: %zu pairs\n", n);
    return 0;
}
