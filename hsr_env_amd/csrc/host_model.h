// The library's error message, the model-blob loader with its JSON reader, the hsr_model_* entry points and the hull-plane builder.
// Plain C++17: nothing here needs a HIP header (it compiles with a host compiler on its own).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/hsrsim.h"

enum { HSR_GEOM_MESH = 7 };        // model.h: GEOM_MESH (host_batch.h asserts that they agree)

static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, const char *detail = "") {
    snprintf(g_err, sizeof g_err, fmt, detail);
    return code;
}
extern "C" const char *hsr_last_error(void) { return g_err; }

// ------------------------------------------------------------------ blob parsing
struct BlobEntry { char name[32]; uint32_t dtype, ndim, shape[4]; uint64_t off, nbytes; };

struct hsr_model {
    std::vector<uint8_t> raw;
    std::map<std::string, const BlobEntry *> entries;
    const uint8_t *data = nullptr;
    std::string json;
    uint64_t fingerprint = 0;      // 64-bit FNV-1a of the blob's bytes: what a snapshot is bound to (host_snapshot.h)
    int sizes[16];
    double opt[16];
    std::vector<std::string> body_names, joint_names;
    std::vector<std::pair<int, int>> joint_qposadr;
    // host copies used to build device tables for each batch's device
    std::vector<float> ctrlrange, qpos0;
    std::vector<std::string> geom_names;
    // face planes of the mesh hulls (hull_planes_build, on first use): float4 (n, w) with n.x <= w inside, per geom offset / count
    mutable std::vector<float> hull_planes;
    mutable std::vector<int> hull_off, hull_cnt;
    mutable bool hull_done = false;

    const double *f64(const char *n, size_t *count = nullptr) const {
        auto it = entries.find(n);
        if (it == entries.end()) return nullptr;
        if (count) *count = it->second->nbytes / 8;
        return (const double *)(data + it->second->off);
    }
    const int *i32(const char *n, size_t *count = nullptr) const {
        auto it = entries.find(n);
        if (it == entries.end()) return nullptr;
        if (count) *count = it->second->nbytes / 4;
        return (const int *)(data + it->second->off);
    }
};

// minimal JSON helpers for the "names"/"meta" sidecar (flat lists of strings / int pairs)
static size_t json_find_key(const std::string &js, const char *key, size_t from = 0) {
    std::string k = std::string("\"") + key + "\":";
    return js.find(k, from);
}
static std::vector<std::string> json_string_list(const std::string &js, size_t pos) {
    std::vector<std::string> out;
    size_t lb = js.find('[', pos);
    if (lb == std::string::npos) return out;
    size_t i = lb + 1;
    while (i < js.size() && js[i] != ']') {
        if (js[i] == '"') {
            size_t j = js.find('"', i + 1);
            out.push_back(js.substr(i + 1, j - i - 1));
            i = j + 1;
        } else if (js.compare(i, 4, "null") == 0) { out.push_back(""); i += 4; }
        else i++;
    }
    return out;
}
static std::vector<std::pair<int, int>> json_pair_list(const std::string &js, size_t pos) {
    std::vector<std::pair<int, int>> out;
    size_t lb = js.find('[', pos);
    if (lb == std::string::npos) return out;
    size_t i = lb + 1;
    int depth = 1;
    std::vector<int> cur;
    while (i < js.size() && depth > 0) {
        char ch = js[i];
        if (ch == '[') { depth++; cur.clear(); i++; }
        else if (ch == ']') { depth--; if (depth == 1 && cur.size() == 2) out.push_back({cur[0], cur[1]}); i++; }
        else if ((ch >= '0' && ch <= '9') || ch == '-') { char *endp; long v = strtol(js.c_str() + i, &endp, 10); cur.push_back((int)v); i = endp - js.c_str(); }
        else i++;
    }
    return out;
}

extern "C" int hsr_model_load(const void *blob, size_t len, hsr_model **out) {
    if (!blob || !out) return fail(HSR_EINVAL, "null argument");
    if (len < 16 || memcmp(blob, "HSRM0001", 8) != 0) return fail(HSR_EBLOB, "not an HSRM0001 model blob");
    // the blob is untrusted input (hsr/mujoco_env.py:30-31: a bad model file is an IOError, never a crash): every length and offset
    // is checked against `len` before it is used
    const uint8_t *in = (const uint8_t *)blob;
    uint32_t n;
    memcpy(&n, in + 8, 4);
    if (n > 4096 || 16 + (uint64_t)n * sizeof(BlobEntry) + 8 > len) return fail(HSR_EBLOB, "truncated model blob (entry table)");
    uint64_t jl;
    memcpy(&jl, in + 16 + (size_t)n * sizeof(BlobEntry), 8);
    const uint64_t data_off = 16 + (uint64_t)n * sizeof(BlobEntry) + 8;
    if (jl > len - data_off || (jl & 7) != 0) return fail(HSR_EBLOB, "truncated model blob (names / meta)");
    const uint64_t data_len = len - data_off - jl;
    {
        const BlobEntry *ent0 = (const BlobEntry *)(in + 16);
        for (uint32_t i = 0; i < n; i++) {
            BlobEntry e;
            memcpy(&e, ent0 + i, sizeof e);
            if (e.off > data_len || e.nbytes > data_len - e.off) return fail(HSR_EBLOB, "model blob entry out of bounds");
            if ((e.off & 7) != 0) return fail(HSR_EBLOB, "model blob entry misaligned");
        }
    }
    hsr_model *m = new hsr_model();
    m->raw.assign(in, in + len);
    const uint8_t *raw = m->raw.data();
    m->fingerprint = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; i++) m->fingerprint = (m->fingerprint ^ raw[i]) * 0x100000001b3ull;
    const BlobEntry *ent = (const BlobEntry *)(raw + 16);
    const uint8_t *p = raw + 16 + (size_t)n * sizeof(BlobEntry);
    m->json.assign((const char *)p + 8, (size_t)jl);
    m->data = p + 8 + jl;
    for (uint32_t i = 0; i < n; i++) m->entries[std::string(ent[i].name, strnlen(ent[i].name, 32))] = &ent[i];
    size_t nsz = 0, nop = 0;
    const int *sz = m->i32("sizes", &nsz);
    const double *op = m->f64("opt", &nop);
    if (!sz || !op || nsz < 16 || nop < 16) { delete m; return fail(HSR_EBLOB, "blob lacks sizes/opt"); }
    memcpy(m->sizes, sz, sizeof m->sizes);
    memcpy(m->opt, op, sizeof m->opt);
    for (int i = 0; i < 16; i++) if (m->sizes[i] < 0 || m->sizes[i] > (1 << 20)) { delete m; return fail(HSR_EBLOB, "blob sizes out of range"); }
    {   // every table the host code and the kernels index by a model size must be at least that long, and every index table
        // must point inside the table it indexes: a corrupted file is refused here, not found by a kernel
        const int nq = m->sizes[HSR_NQ], nv = m->sizes[HSR_NV], nu = m->sizes[HSR_NU], nl = m->sizes[HSR_NLINK], nb = m->sizes[HSR_NBODY],
                  ng = m->sizes[HSR_NGEOM], np_ = m->sizes[HSR_NPAIR], nmv = m->sizes[HSR_NMESHVERT], nslot = m->sizes[HSR_NSLOT];
        struct Need { const char *name; int dtype; long long count; };
        const Need need[] = {
            {"qpos0", 0, nq}, {"link_parent", 1, nl}, {"link_pos", 0, 3LL * nl}, {"link_quat", 0, 4LL * nl}, {"link_dofadr", 1, nl}, {"link_dofnum", 1, nl},
            {"link_qposadr", 1, nl}, {"link_free", 1, nl}, {"link_mass", 0, nl}, {"link_com", 0, 3LL * nl}, {"link_inertia", 0, 6LL * nl}, {"link_dofmask", 1, nl},
            {"dof_link", 1, nv}, {"dof_type", 1, nv}, {"dof_axis", 0, 3LL * nv}, {"dof_pos", 0, 3LL * nv}, {"dof_parent", 1, nv}, {"dof_damping", 0, nv},
            {"dof_qposadr", 1, nv}, {"dof_invweight0", 0, nv}, {"dof_limited", 1, nv}, {"dof_range", 0, 2LL * nv}, {"dof_solref", 0, 2LL * nv}, {"dof_solimp", 0, 5LL * nv},
            {"body_link", 1, nb}, {"body_pos", 0, 3LL * nb}, {"body_quat", 0, 4LL * nb}, {"body_mocap", 1, nb},
            {"geom_type", 1, ng}, {"geom_link", 1, ng}, {"geom_pos", 0, 3LL * ng}, {"geom_quat", 0, 4LL * ng}, {"geom_size", 0, 3LL * ng}, {"geom_rbound", 0, ng},
            {"geom_meshadr", 1, ng}, {"geom_meshnum", 1, ng}, {"geom_invweight", 0, 2LL * ng}, {"geom_aabb", 0, 6LL * ng}, {"mesh_vert", 0, 3LL * nmv},
            {"pair_geom1", 1, np_}, {"pair_geom2", 1, np_}, {"pair_fn", 1, np_}, {"pair_condim", 1, np_}, {"pair_slot", 1, np_ + 1LL}, {"pair_friction", 0, 5LL * np_},
            {"pair_solref", 0, 2LL * np_}, {"pair_solimp", 0, 5LL * np_},
            {"act_dof", 1, nu}, {"act_gear", 0, nu}, {"act_kp", 0, nu}, {"act_ctrlrange", 0, 2LL * nu}, {"act_forcerange", 0, 2LL * nu}};
        for (const Need &nd : need) {
            auto it = m->entries.find(nd.name);
            if (it == m->entries.end()) { delete m; return fail(HSR_EBLOB, "blob entry '%s' missing", nd.name); }
            if ((int)it->second->dtype != nd.dtype || (long long)(it->second->nbytes / (nd.dtype == 0 ? 8 : 4)) < nd.count) { delete m; return fail(HSR_EBLOB, "blob entry '%s' shorter than the model sizes say", nd.name); }
        }
        auto in_range = [&](const char *name, int cnt, int lo, int hi) {       // all of the first cnt values in [lo, hi)
            const int *v = m->i32(name);
            for (int i = 0; i < cnt; i++) if (v[i] < lo || v[i] >= hi) return false;
            return true;
        };
        bool ok = nl >= 1 && in_range("link_parent", nl, 0, nl) && in_range("dof_link", nv, 0, nl) && in_range("dof_parent", nv, -1, nv) && in_range("dof_qposadr", nv, 0, nq > 0 ? nq : 1)
                  && in_range("body_link", nb, 0, nl) && in_range("geom_link", ng, 0, nl) && in_range("pair_geom1", np_, 0, ng) && in_range("pair_geom2", np_, 0, ng)
                  && in_range("pair_fn", np_, 0, 4) && in_range("pair_slot", np_ + 1, 0, nslot + 1) && in_range("act_dof", nu, 0, nv > 0 ? nv : 1)
                  && in_range("link_dofadr", nl, -1, nv + 1) && in_range("link_dofnum", nl, 0, nv + 1) && in_range("link_qposadr", nl, -1, nq + 1);
        if (ok) {
            const int *ma = m->i32("geom_meshadr"), *mn = m->i32("geom_meshnum"), *gt = m->i32("geom_type");
            for (int g = 0; g < ng; g++)
                if (gt[g] == HSR_GEOM_MESH && (ma[g] < 0 || mn[g] < 0 || (long long)ma[g] + mn[g] > nmv)) ok = false;
        }
        if (!ok) { delete m; return fail(HSR_EBLOB, "blob index table out of range"); }
    }
    size_t np = json_find_key(m->json, "names");
    if (np != std::string::npos) {
        size_t bp = json_find_key(m->json, "body", np), jp = json_find_key(m->json, "joint", np);
        if (bp != std::string::npos) m->body_names = json_string_list(m->json, bp);
        if (jp != std::string::npos) m->joint_names = json_string_list(m->json, jp);
        size_t gp = json_find_key(m->json, "geom", np);
        if (gp != std::string::npos) m->geom_names = json_string_list(m->json, gp);
    }
    size_t qp = json_find_key(m->json, "joint_qposadr");
    if (qp != std::string::npos) m->joint_qposadr = json_pair_list(m->json, qp);
    const int nu = m->sizes[HSR_NU], nq = m->sizes[HSR_NQ];
    size_t ncr = 0, nq0 = 0;
    const double *cr = m->f64("act_ctrlrange", &ncr), *q0 = m->f64("qpos0", &nq0);
    if ((nu > 0 && (!cr || ncr < (size_t)nu * 2)) || (nq > 0 && (!q0 || nq0 < (size_t)nq))) { delete m; return fail(HSR_EBLOB, "blob lacks act_ctrlrange / qpos0"); }
    m->ctrlrange.resize((size_t)nu * 2);
    for (int i = 0; i < nu * 2; i++) m->ctrlrange[i] = (float)cr[i];
    m->qpos0.resize(nq);
    for (int i = 0; i < nq; i++) m->qpos0[i] = (float)q0[i];
    *out = m;
    return HSR_OK;
}
extern "C" void hsr_model_destroy(hsr_model *m) { delete m; }
extern "C" int hsr_model_size(const hsr_model *m, int which) { return (m && which >= 0 && which < 16) ? m->sizes[which] : HSR_EINVAL; }
extern "C" double hsr_model_timestep(const hsr_model *m) { return m ? m->opt[0] : 0.0; }
extern "C" int hsr_model_ctrlrange(const hsr_model *m, float *out) {
    if (!m || !out) return fail(HSR_EINVAL, "null argument");
    memcpy(out, m->ctrlrange.data(), m->ctrlrange.size() * sizeof(float)); return HSR_OK;
}
extern "C" int hsr_model_qpos0(const hsr_model *m, float *out) {
    if (!m || !out) return fail(HSR_EINVAL, "null argument");
    memcpy(out, m->qpos0.data(), m->qpos0.size() * sizeof(float)); return HSR_OK;
}
extern "C" int hsr_model_body_id(const hsr_model *m, const char *name) {
    if (!m || !name) return fail(HSR_EINVAL, "null argument");
    for (size_t i = 0; i < m->body_names.size(); i++) if (m->body_names[i] == name) return (int)i;
    return fail(HSR_ENAME, "unknown body '%s'", name);
}
extern "C" int hsr_model_joint_qpos_addr(const hsr_model *m, const char *name, int *start, int *end) {
    if (!m || !name || !start || !end) return fail(HSR_EINVAL, "null argument");
    for (size_t i = 0; i < m->joint_names.size() && i < m->joint_qposadr.size(); i++)
        if (m->joint_names[i] == name) { *start = m->joint_qposadr[i].first; *end = m->joint_qposadr[i].first + m->joint_qposadr[i].second; return HSR_OK; }
    return fail(HSR_ENAME, "unknown joint '%s'", name);
}

// Face planes of the mesh hulls (the blob stores the hull vertices only; the ray caster clips rays against the faces).  Brute force
// in double over vertex triples: the plane through three vertices is a face when no vertex lies outside it by more than 1e-9 of
// the hull's size (the scan stops at the first vertex on either side that disagrees); coplanar triples of one facet give the same
// plane and are merged.  At most 256 vertices per hull: ~2.7 M triples, most rejected after a few vertices.
static void hull_planes_build(const hsr_model *m) {
    if (m->hull_done) return;
    const int ng = m->sizes[HSR_NGEOM];
    const int *gt = m->i32("geom_type"), *ma = m->i32("geom_meshadr"), *mn = m->i32("geom_meshnum");
    const double *mv = m->f64("mesh_vert");
    m->hull_off.assign(ng, 0); m->hull_cnt.assign(ng, 0); m->hull_planes.clear();
    for (int g = 0; g < ng; g++) {
        m->hull_off[g] = (int)(m->hull_planes.size() / 4);
        if (gt[g] != HSR_GEOM_MESH) continue;
        const int nv = mn[g];
        const double *V = mv + 3 * (size_t)ma[g];
        double size = 0;
        for (int i = 0; i < 3 * nv; i++) size = std::max(size, fabs(V[i]));
        const double tol = 1e-9 * size;
        std::vector<double> pl;                            // accepted planes: nx ny nz w
        for (int i = 0; i < nv; i++) for (int j = i + 1; j < nv; j++) for (int k = j + 1; k < nv; k++) {
            const double *a = V + 3 * i, *b = V + 3 * j, *c = V + 3 * k;
            const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (len <= 1e-12 * size * size) continue;      // (nearly) collinear
            for (double &x : n) x /= len;
            const double d = n[0] * a[0] + n[1] * a[1] + n[2] * a[2];
            bool above = false, below = false;
            for (int q = 0; q < nv && !(above && below); q++) {
                const double sd = n[0] * V[3 * q] + n[1] * V[3 * q + 1] + n[2] * V[3 * q + 2] - d;
                above |= sd > tol; below |= sd < -tol;
            }
            if (above && below) continue;
            const double sg = above ? -1.0 : 1.0;          // orient outward: every vertex at n.x <= w
            const double cand[4] = {sg * n[0], sg * n[1], sg * n[2], sg * d};
            bool dup = false;
            for (size_t p = 0; p < pl.size() && !dup; p += 4)
                dup = fabs(pl[p] - cand[0]) + fabs(pl[p + 1] - cand[1]) + fabs(pl[p + 2] - cand[2]) < 1e-7 && fabs(pl[p + 3] - cand[3]) <= 100 * tol;
            if (!dup) pl.insert(pl.end(), cand, cand + 4);
        }
        for (double x : pl) m->hull_planes.push_back((float)x);
        m->hull_cnt[g] = (int)(pl.size() / 4);
    }
    m->hull_done = true;
}
extern "C" int hsr_model_hull_planes(const hsr_model *m, int geom, float *out, int cap) {
    if (!m || geom < 0 || geom >= m->sizes[HSR_NGEOM]) return fail(HSR_EINVAL, "hull_planes: bad geom");
    if (m->i32("geom_type")[geom] != HSR_GEOM_MESH) return fail(HSR_EINVAL, "hull_planes: geom is not a mesh");
    hull_planes_build(m);
    const int n = m->hull_cnt[geom];
    if (out) for (int i = 0; i < std::min(n, cap); i++) for (int k = 0; k < 4; k++) out[4 * i + k] = m->hull_planes[4 * (size_t)(m->hull_off[geom] + i) + k];
    return n;
}
