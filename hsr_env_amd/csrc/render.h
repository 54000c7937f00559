// k_render: batched ray caster over the collision geoms (include/hsrsim.h: hsr_batch_render).  Read-only on the simulation state:
// it reads the link poses of the last reset / forward / step (DevState::xpos / xmat) - or, k_render<true>, captured frames of the last
// step (hsr_batch_render_frames) - and writes nothing but its three images.
//
// Layout: one 256-thread workgroup (4 waves) renders one 16 x 16 pixel tile of one env, one lane per pixel; grid = envs x tiles.
// Prologue (wave 0): every geom's world placement from its link pose, culled by its bounding sphere (geom_rbound around the geom
// origin; planes always pass) against the tile's frustum, survivors compacted into an LDS list with a wave ballot, each as a
// 32-float record that already holds the camera origin in the geom frame.  Per pixel: the candidates in order (wave-uniform loop
// index and type), a slab test of the padded geom_aabb first - a geom that no lane of the wave can hit in front of its current
// nearest hit is skipped by the whole wave - then the exact test of the type.  Nearest hit with znear <= depth <= zfar wins; ties
// keep the lower geom id.  A result depends on the env's own poses only.
//
// Ray parametrisation: dir = fwd + u right + v up has a unit component along the camera axis, so the ray parameter t of a hit IS
// its depth along that axis (MuJoCo's depth buffer, linearised).  Shading (fixed; DESIGN.md section f):
//   rgb = clamp(rgba.rgb * (0.1 + 0.4 max(0, n.v) + 0.5 max(0, n.z)), 0, 1), rounded to 0..255
// with n the world normal of the entering surface and v the unit direction back to the camera; background black, depth zfar, id -1.
#pragma once
#include <float.h>
#include "devmath.h"
#include "model.h"

struct RenderCam {
    float fwd[3], right[3], up[3];    // unit camera axes (MuJoCo free camera: azimuth / elevation)
    float lookat[3], dist;            // camera origin = lookat (+ tracked body origin) - dist * fwd
    float tanx, tany, znear, zfar;    // half extents of the image at depth 1
    int track_link;                   // -1: fixed lookat; else lookat += xpos(link) + xmat(link) track_off (the tracked body's origin)
    float track_off[3];
    int W, H, tiles_x, ntiles, env0;  // image size, 16 x 16 tiles per row / per image, first env of the launch
};

enum { RREC = 32 };                   // floats per candidate record in LDS
// record: R[0..8] (geom -> world, row-major) | camera origin in the geom frame [9..11] | size [12..14] | type [15] |
//         padded aabb centre [16..18] | half [19..21] | rgb [22..24] | plane offset [25] | plane count [26] | geom id [27]

__device__ __forceinline__ int rd_int(const float *p) { return __builtin_amdgcn_readfirstlane(__float_as_int(*p)); }

// slab test against an axis-aligned box (centre c, half extents h) in the geom frame: entering / leaving t and the entering axis
__device__ __forceinline__ void slab(v3 o, v3 inv, const float *c, const float *h, float &t0, float &t1, int &ax) {
    t0 = -FLT_MAX; t1 = FLT_MAX; ax = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float ok = comp(o, k), ik = comp(inv, k);
        const float a = (c[k] - h[k] - ok) * ik, b = (c[k] + h[k] - ok) * ik;
        const float lo = fminf(a, b), hi = fmaxf(a, b);     // fminf / fmaxf drop the NaN of 0 * inf (ray in a slab's boundary plane)
        if (lo > t0) { t0 = lo; ax = k; }
        t1 = fminf(t1, hi);
    }
}

// FR (hsr_batch_render_frames): the poses come from the captured frames instead of the state - image i = slot i / rows, frame i % rows
// of the capture buffer (model.h: StepIO::cap); a frame at or past its slot's count, other than the last (final) one, is not rendered
struct FrameSrc { const float *cap; const int *cnt; int R, rows; };

template <bool FR>
__global__ void __launch_bounds__(256) k_render(DevModel m, DevState s, RenderCam c, const float4 *__restrict__ planes,
                                                const int2 *__restrict__ prange, const float4 *__restrict__ rgba, uint8_t *rgb, float *depth, int32_t *segid,
                                                FrameSrc fs) {
    extern __shared__ float rrec[];                       // [ngeom][RREC] candidates, then the candidate count
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.x % c.ntiles, e = c.env0 + blockIdx.x / c.ntiles, N = s.N;      // e: the image (FR: slot x frame)
    const int x0 = (tile % c.tiles_x) * 16, y0 = (tile / c.tiles_x) * 16;
    const v3 fwd = mk3(c.fwd[0], c.fwd[1], c.fwd[2]), rt = mk3(c.right[0], c.right[1], c.right[2]), up = mk3(c.up[0], c.up[1], c.up[2]);
    View xpos{s.xpos + e, N}, xmat{s.xmat + e, N};
    if constexpr (FR) {
        const int slot = e / fs.rows, k = e % fs.rows;
        if (k < fs.rows - 1 && k >= fs.cnt[slot]) return;              // (whole workgroup)
        float *p = const_cast<float *>(fs.cap) + (size_t)k * 12 * m.nlink * fs.R + slot;
        xpos = View{p, fs.R}; xmat = View{p + (size_t)3 * m.nlink * fs.R, fs.R};
    }
    // camera origin of this env
    v3 look = mk3(c.lookat[0], c.lookat[1], c.lookat[2]);
    if (c.track_link >= 0)
        look = look + xpos.get3(c.track_link) + mulmv(xmat.getm(c.track_link), mk3(c.track_off[0], c.track_off[1], c.track_off[2]));
    const v3 cam = look - fwd * c.dist;
    int *ncand = reinterpret_cast<int *>(rrec + RREC * m.ngeom);
    if (tid < 64) {
        // the tile's frustum: side planes through the camera origin, inward normals in camera coordinates (u, v, 1)
        const float uL = (2.f * x0 / c.W - 1.f) * c.tanx, uR = (2.f * min(x0 + 16, c.W) / c.W - 1.f) * c.tanx;
        const float vT = (1.f - 2.f * y0 / c.H) * c.tany, vB = (1.f - 2.f * min(y0 + 16, c.H) / c.H) * c.tany;
        const v3 nL = (rt - fwd * uL) * frsq(1.f + uL * uL), nR = (fwd * uR - rt) * frsq(1.f + uR * uR);
        const v3 nB = (up - fwd * vB) * frsq(1.f + vB * vB), nT = (fwd * vT - up) * frsq(1.f + vT * vT);
        int count = 0;
        for (int base = 0; base < m.ngeom; base += 64) {
            const int g = base + lane;
            bool pass = false;
            m3 R; v3 p;
            if (g < m.ngeom) {
                const int l = m.geom_link[g];
                const m3 Rg = ldm(m.geom_mat, g);
                const v3 pg = ld3(m.geom_pos, g);
                if (l == 0) { R = Rg; p = pg; }          // world link: identity pose
                else {
                    const m3 Rl = xmat.getm(l);
                    R = mulmm(Rl, Rg); p = xpos.get3(l) + mulmv(Rl, pg);
                }
                const float r = m.geom_rbound[g];
                const v3 q = p - cam;
                const float z = dot(q, fwd);
                pass = m.geom_type[g] == GEOM_PLANE ||
                       (dot(q, nL) >= -r && dot(q, nR) >= -r && dot(q, nB) >= -r && dot(q, nT) >= -r && z >= c.znear - r && z <= c.zfar + r);
            }
            const unsigned long long bal = __ballot(pass);
            if (pass) {
                float *o = rrec + RREC * (count + __popcll(bal & ((1ull << lane) - 1ull)));
#pragma unroll
                for (int k = 0; k < 9; k++) o[k] = R.a[k];
                const v3 og = mulmtv(R, cam - p);
                o[9] = og.x; o[10] = og.y; o[11] = og.z;
                const v3 sz = ld3(m.geom_size, g);
                o[12] = sz.x; o[13] = sz.y; o[14] = sz.z;
                o[15] = __int_as_float(m.geom_type[g]);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float h = m.geom_aabb[6 * g + 3 + k];
                    o[16 + k] = m.geom_aabb[6 * g + k];
                    o[19 + k] = h * 1.0001f + 1e-6f;      // padded: the exact tests below never hit outside it
                }
                const float4 col = rgba[g];
                o[22] = col.x; o[23] = col.y; o[24] = col.z;
                const int2 pr = prange[g];                  // hull face planes of a mesh (offset, count); 0, 0 otherwise
                o[25] = __int_as_float(pr.x); o[26] = __int_as_float(pr.y);
                o[27] = __int_as_float(g);
            }
            count += __popcll(bal);
        }
        if (lane == 0) *ncand = count;
    }
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(*ncand);

    const int px = x0 + (tid & 15), py = y0 + (tid >> 4);
    const float u = ((px + 0.5f) * (2.f / c.W) - 1.f) * c.tanx, v = (1.f - (py + 0.5f) * (2.f / c.H)) * c.tany;
    const v3 dir = fwd + rt * u + up * v;
    float best = FLT_MAX;
    int bk = -1;
    v3 bn = mk3(0.f, 0.f, 1.f);
    for (int k = 0; k < n; k++) {
        const float *r = rrec + RREC * k;
        const int type = rd_int(r + 15);
        m3 R;
#pragma unroll
        for (int i = 0; i < 9; i++) R.a[i] = r[i];
        const v3 o = mk3(r[9], r[10], r[11]);
        const v3 d = mulmtv(R, dir);
        const float lim = fminf(best, c.zfar);
        float t0, t1;
        v3 ng;                                             // entering normal in the geom frame
        bool hit;
        if (type == GEOM_PLANE) {                          // MuJoCo's plane: z = 0, front side only, finite where size[0..1] > 0
            t0 = -o.z * frcp(d.z);
            const float hx = o.x + t0 * d.x, hy = o.y + t0 * d.y;
            hit = o.z > 0.f && d.z < 0.f && (r[12] <= 0.f || fabsf(hx) <= r[12]) && (r[13] <= 0.f || fabsf(hy) <= r[13]);
            ng = mk3(0.f, 0.f, 1.f);
        } else {
            const v3 inv = mk3(frcp(d.x), frcp(d.y), frcp(d.z));
            int ax;
            slab(o, inv, r + 16, r + 19, t0, t1, ax);
            const bool inbox = t0 <= t1 && t1 >= c.znear && t0 <= lim;
            if (!wave_any(inbox)) continue;
            if (type == GEOM_BOX) {
                slab(o, inv, r + 16, r + 12, t0, t1, ax);      // aabb centre of a box is its origin; half extents = size
                hit = t0 <= t1;
                ng = mk3(0.f, 0.f, 0.f);
                const float sg = comp(d, ax) > 0.f ? -1.f : 1.f;
                ng.x = ax == 0 ? sg : 0.f; ng.y = ax == 1 ? sg : 0.f; ng.z = ax == 2 ? sg : 0.f;
            } else if (type == GEOM_SPHERE) {
                // roots about the closest approach (no cancellation between |o|^2 and r^2 at camera distance)
                const float a = dot(d, d), tc = -dot(o, d) / a;
                const v3 q = o + d * tc;
                const float h2 = (r[12] * r[12] - dot(q, q)) / a;
                hit = h2 >= 0.f;
                t0 = tc - fsqrt(fmaxf(h2, 0.f));
                ng = normalized(o + d * t0);
            } else if (type == GEOM_CYLINDER) {
                const float rad = r[12], hl = r[13];
                const float a = d.x * d.x + d.y * d.y;
                float s0 = -FLT_MAX, s1 = FLT_MAX;
                bool side_ok;
                if (a > 1e-20f) {
                    const float tc = -(o.x * d.x + o.y * d.y) / a, qx = o.x + tc * d.x, qy = o.y + tc * d.y;
                    const float h2 = (rad * rad - qx * qx - qy * qy) / a, sq = fsqrt(fmaxf(h2, 0.f));
                    side_ok = h2 >= 0.f; s0 = tc - sq; s1 = tc + sq;
                } else side_ok = o.x * o.x + o.y * o.y <= rad * rad;
                const float za = (-hl - o.z) / d.z, zb = (hl - o.z) / d.z;
                const float c0 = fminf(za, zb), c1 = fmaxf(za, zb);
                t0 = fmaxf(s0, c0); t1 = fminf(s1, c1);
                hit = side_ok && t0 <= t1;
                if (s0 >= c0) { const v3 hp = o + d * t0; ng = normalized(mk3(hp.x, hp.y, 0.f)); }
                else ng = mk3(0.f, 0.f, d.z > 0.f ? -1.f : 1.f);
            } else {                                       // mesh: clip the ray against the hull's face planes n.x <= w
                const int off = rd_int(r + 25), np = rd_int(r + 26);
                t0 = -FLT_MAX; t1 = FLT_MAX;
                ng = mk3(0.f, 0.f, 1.f);
                for (int j = 0; j < np; j++) {
                    const float4 P = planes[off + j];
                    const float den = P.x * d.x + P.y * d.y + P.z * d.z, num = P.w - (P.x * o.x + P.y * o.y + P.z * o.z);
                    const float t = num / den;
                    if (den < 0.f) { if (t > t0) { t0 = t; ng = mk3(P.x, P.y, P.z); } }
                    else if (den > 0.f) t1 = fminf(t1, t);
                    else if (num < 0.f) t1 = -FLT_MAX;
                }
                hit = t0 <= t1 && t0 > -FLT_MAX;
            }
        }
        if (hit && t0 >= c.znear && t0 <= c.zfar && t0 < best) { best = t0; bk = k; bn = mulmv(R, ng); }
    }
    if (px >= c.W || py >= c.H) return;
    const size_t pix = ((size_t)e * c.H + py) * c.W + px;
    if (depth) depth[pix] = bk >= 0 ? best : c.zfar;
    if (segid) segid[pix] = bk >= 0 ? __float_as_int(rrec[RREC * bk + 27]) : -1;
    if (rgb) {
        uint8_t o3[3] = {0, 0, 0};
        if (bk >= 0) {
            const float sh = 0.1f + 0.4f * fmaxf(0.f, -dot(bn, dir) * frsq(dot(dir, dir))) + 0.5f * fmaxf(0.f, bn.z);
#pragma unroll
            for (int k = 0; k < 3; k++) o3[k] = (uint8_t)(fminf(fmaxf(rrec[RREC * bk + 22 + k] * sh, 0.f), 1.f) * 255.f + 0.5f);
        }
        uint8_t *q = rgb + 3 * pix;
        q[0] = o3[0]; q[1] = o3[1]; q[2] = o3[2];
    }
}
