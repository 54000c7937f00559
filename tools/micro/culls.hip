// The conservative collision culls as the kernels call them, one pair per lane: sphere_hits_obb, obb_overlap, pair_cull (csrc/collide.h), pair_cull_box_nb and
// pair_pack (csrc/kin2.h) with the radius that level 1 of the persistent kernel reads back from the packed record (csrc/persist.h).  Nothing is re-typed: the
// product headers are included and their functions called.  Every second wave runs with a quarter of its lanes (lane % 4 == 3) switched off behind a divergent
// branch; those lanes keep the sentinel in every output word.
//   hipcc <CODEGEN_FLAGS of hsr_env_amd/build.py> -o culls culls.hip && ./culls ROWS OUT
// ROWS: n rows of 64 words, n a multiple of 64:
//   int   type1 nvert1 voff1 type2 nvert2 voff2 g1 g2 fn -                                  (g1, g2 < 64 and fn < 4: the fields of pair_pack)
//   float pos1[3] mat1[9] size1[3] bc1[3] bh1[3] | the same of geom 2 | rb1 rb2 skin rad     (words 10 .. 55; rad: the radius bound handed to pair_pack)
//   8 words of padding
// OUT: n rows of 16 words:
//   sphere_hits_obb(pos2, rb2, G1)  sphere_hits_obb(pos1, rb1, G2)  obb_overlap(G1, G2)  pair_cull(m, G1, G2, 0, 1) with m.geom_rbound = {rb1, rb2}
//   pair_cull_box_nb(G1, G2, rb1, rb2, 0)  pair_cull_box_nb(G1, G2, rb1, rb2, HSR_SKIN)  pair_pack(g1, g2, fn, rad)  the radius unpacked from it (float bits)
//   that radius + skin (float bits)  pk_g1  pk_g2  pk_fn  HSR_SKIN (float bits)  3 words of padding
// Nothing is judged here: tests/test_gpu_culls.py does, against the exact geometry of tests/cull_ref.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../hsr_env_amd/csrc/kin2.h"
#include "../../hsr_env_amd/csrc/solve_g.h"

enum { IN_W = 64, OUT_W = 16 };
constexpr unsigned SENTINEL = 0xdeadbeefu;

__device__ __forceinline__ Geom read_geom(const unsigned *pi, const float *pf) {
    Geom G;
    G.type = (int)pi[0]; G.nvert = (int)pi[1];
    G.verts = nullptr;                                   // no cull reads a hull
    G.pos = mk3(pf[0], pf[1], pf[2]);
#pragma unroll
    for (int k = 0; k < 9; k++) G.mat.a[k] = pf[3 + k];
    G.size = mk3(pf[12], pf[13], pf[14]);
    G.bc = mk3(pf[15], pf[16], pf[17]);
    G.bh = mk3(pf[18], pf[19], pf[20]);
    return G;
}

__global__ void __launch_bounds__(64) k_culls(const unsigned *in, float *rbtab, unsigned *out) {
    const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
    const unsigned *p = in + IN_W * row;
    const float *pf = reinterpret_cast<const float *>(p) + 10;
    unsigned *w = out + OUT_W * row;
#pragma unroll
    for (int k = 0; k < OUT_W; k++) w[k] = SENTINEL;
    const bool off = (blockIdx.x & 1) && (threadIdx.x & 3) == 3;
    if (!off) {
        const Geom A = read_geom(p, pf), B = read_geom(p + 3, pf + 21);
        const float rb1 = pf[42], rb2 = pf[43], skin = pf[44], rad = pf[45];
        rbtab[2 * row] = rb1; rbtab[2 * row + 1] = rb2;
        DevModel m = {};
        m.geom_rbound = rbtab + 2 * row;                  // the only table pair_cull reads
        w[0] = sphere_hits_obb(B.pos, rb2, A) ? 1u : 0u;
        w[1] = sphere_hits_obb(A.pos, rb1, B) ? 1u : 0u;
        w[2] = obb_overlap(A, B) ? 1u : 0u;
        w[3] = pair_cull(m, A, B, 0, 1) ? 1u : 0u;
        w[4] = pair_cull_box_nb(A, B, rb1, rb2, 0.f) ? 1u : 0u;
        w[5] = pair_cull_box_nb(A, B, rb1, rb2, HSR_SKIN) ? 1u : 0u;
        const unsigned pk = pair_pack((int)p[6], (int)p[7], (int)p[8], rad);
        const float back = __uint_as_float(pk & 0xffff0000u);      // persist.h, level 1
        w[6] = pk; w[7] = __float_as_uint(back); w[8] = __float_as_uint(back + skin);
        w[9] = (unsigned)pk_g1(pk); w[10] = (unsigned)pk_g2(pk); w[11] = (unsigned)pk_fn(pk);
        w[12] = __float_as_uint(HSR_SKIN);
        w[13] = w[14] = w[15] = 0;
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

// the kernel forms no index from a row's contents but the fields of pair_pack, which it only packs: types and those fields are checked all the same
static bool rows_ok(const std::vector<uint32_t> &in, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t *p = in.data() + IN_W * i;
        for (int side = 0; side < 2; side++) {
            const uint32_t type = p[3 * side];
            if (type != GEOM_PLANE && type != GEOM_BOX && type != GEOM_CYLINDER && type != GEOM_MESH) { fprintf(stderr, "row %zu: geom type %u\n", i, type); return false; }
        }
        if (p[6] >= 64 || p[7] >= 64 || p[8] >= 4) { fprintf(stderr, "row %zu: pair_pack fields out of range\n", i); return false; }
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s ROWS OUT\n", argv[0]); return 1; }
    std::vector<uint32_t> in;
    if (!read_words(argv[1], in)) return 1;
    if (in.size() % (64 * IN_W) != 0) { fprintf(stderr, "not a whole number of 64-row waves\n"); return 1; }
    const size_t n = in.size() / IN_W;
    if (!rows_ok(in, n)) return 1;
    void *din, *drb, *dout;
    CK(hipMalloc(&din, in.size() * 4));
    CK(hipMalloc(&drb, 2 * n * 4));
    CK(hipMalloc(&dout, n * OUT_W * 4));
    CK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(drb, 0, 2 * n * 4));
    CK(hipMemset(dout, 0, n * OUT_W * 4));
    k_culls<<<n / 64, 64>>>((const unsigned *)din, (float *)drb, (unsigned *)dout);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(n * OUT_W);
    CK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(din));
    CK(hipFree(drb));
    CK(hipFree(dout));
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 1; }
    fwrite(out.data(), 4, out.size(), fo);
    if (fclose(fo) != 0) { perror(argv[2]); return 1; }
    printf("culls: %zu rows\n", n);
    return 0;
}
