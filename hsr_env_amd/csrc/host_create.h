// Creation of a batch: the environment switches, the table of persistent-kernel instances and the choice among them (plan_persist), the
// model's tables on the device, the state arrays, the LDS sizes of the chain's kernels, the initial reset; and hsr_batch_destroy.

// Every environment switch of the library, read once, by hsr_batch_create before anything uses a value.  Diagnostics and experiments:
// the product runs with none of them set.
static void read_switches(hsr_batch *b) {
    auto env = [](const char *name) { const char *v = getenv(name); return v ? v : ""; };
    auto is0 = [&](const char *name) { return strcmp(env(name), "0") == 0; };
    auto set = [&](const char *name) { return getenv(name) != nullptr; };
    b->sw.no_const = set("HSR_NO_CONST") && !is0("HSR_NO_CONST");                 // any value but 0: generic kernel instances only
    if (set("HSR_NFB")) b->sw.nfb_max = std::max(atoi(env("HSR_NFB")), 0);        // only ever lowers nfb; 0 keeps the per-contact assembly
    b->sw.tables_lds = is0("HSR_TABLES_GLOBAL");                                  // 0 keeps the persistent kernel's tables in LDS
    b->sw.debug = set("HSR_DEBUG");                                               // set: print the chosen instance's resources
    if (set("HSR_SOLO")) b->solo_servers = atoi(env("HSR_SOLO"));                 // solo servers of a queued launch (hsr_batch_set_solo)
    if (atof(env("HSR_SOLO_TRIPS")) > 0) b->solo_trips = (float)atof(env("HSR_SOLO_TRIPS"));     // their hand-over threshold
    if (set("HSR_SPLIT")) b->split = atoi(env("HSR_SPLIT")) != 0;                 // hard envs handed over inside a launch (hsr_batch_set_split)
    if (atoi(env("HSR_SPLIT_PERIOD")) > 0) b->split_period = atoi(env("HSR_SPLIT_PERIOD"));      // substeps between its check points ...
    if (set("HSR_SPLIT_TRIPS") && atof(env("HSR_SPLIT_TRIPS")) >= 0) b->split_trips = (float)atof(env("HSR_SPLIT_TRIPS"));      // ... its threshold (0: every live env counts as hard) ...
    if (atoi(env("HSR_SPLIT_MIN_LEFT")) > 0) b->split_min_left = atoi(env("HSR_SPLIT_MIN_LEFT"));      // ... and the substeps that must remain
    if (set("HSR_SPLIT_LONE")) b->split_lone = atoi(env("HSR_SPLIT_LONE")) != 0;  // the lone rule: a lone hard env leaves its easier neighbours (hsr_batch_set_split_lone)
    if (atof(env("HSR_SPLIT_LONE_TRIPS")) > 0) b->split_lone_trips = (float)atof(env("HSR_SPLIT_LONE_TRIPS"));      // ... and its threshold
    if (set("HSR_QUEUE")) b->queue = atoi(env("HSR_QUEUE")) != 0;                 // work queue forced on / off (hsr_batch_set_queue)
    if (atoi(env("HSR_QUEUE_CHUNK")) > 0) b->queue_chunk = atoi(env("HSR_QUEUE_CHUNK"));         // substeps per round of the work queue ...
    b->queue_chunk_set = atoi(env("HSR_QUEUE_CHUNK")) > 0;                        // ... and no automatic choice then
    if (set("HSR_MPR_WARM")) b->mpr_warm = atoi(env("HSR_MPR_WARM")) != 0;        // 0: MPR starts every substep from scratch
    b->schedule = !is0("HSR_SCHEDULE");                                           // on unless exactly 0: wave packing (k_schedule)
    if (atoi(env("HSR_NARROW_BLOCKS")) > 0) b->narrow_blocks = atoi(env("HSR_NARROW_BLOCKS"));   // grid of k_narrow (the chain)
    if (atoi(env("HSR_PPW")) > 0) b->pairs_per_wave = atoi(env("HSR_PPW"));       // pairs walked by one wave of k_cull (the chain)
}

// The persistent kernel instances.  Every reference configuration has an instance with ALL scalar model fields at compile time
// (cfg_consts.h, generated from the committed blobs; chosen only when the loaded model matches the generated row value for value -
// HSR_NO_CONST=1 never chooses them); any other model runs a generic instance (lanes per env, bound on nv).  A new constant
// configuration adds its entries here.
struct PersistInstance {
    int row;                       // row of kCfgConsts, or -1: a generic instance for ...
    int group, nv;                 // ... this many lanes per env and (nv >= 0) exactly this many dofs
    bool tg;                       // pair / geom tables in global memory (LDS budget: 8 workgroups per CU)
    persist_fn fn, sv;             // the instance and its twin with the solo-server path (persist.h SV), or NULL
    bool split = false;            // its launches may hand hard envs over inside the launch (persist.h): the arm models, whose envs differ in hardness
};
// (persist.h SplitOf: the instances that carry the hand-over code - the rows with `split` below)
template <> struct SplitOf<DevModel_cfg3> : std::true_type {};
template <> struct SplitOf<DevModel_cupboard> : std::true_type {};
static const PersistInstance kPersistInstances[] = {
#ifdef HSR_DEV_CFG3
    // development builds (tools/build_variants.py): only the cfg3 instance is compiled - a sixth of the build time
    {2, 16, -1, false, k_env_step_mf<16, 13, true, 7, false, DevModel_cfg3>, k_env_step_mf<16, 13, true, 7, false, DevModel_cfg3, true>, true},
#else
    {0, 16, -1, false, k_env_step_mf<16, 2, true, 0, false, DevModel_cfg1>, nullptr},                  // two orthogonal slides
    {1, 16, -1, false, k_env_step_mf<16, 8, true, 0, false, DevModel_cfg2>, k_env_step_mf<16, 8, true, 0, false, DevModel_cfg2, true>},      // the slides + one block
    {2, 16, -1, false, k_env_step_mf<16, 13, true, 7, false, DevModel_cfg3>, k_env_step_mf<16, 13, true, 7, false, DevModel_cfg3, true>, true},    // arm + block
    {3, 32, -1, false, k_env_step_mf<32, 25, true, 7, false, DevModel_cfg4>, nullptr},                 // arm + three blocks
    {3, 32, -1, true, k_env_step_mf<32, 25, true, 7, true, DevModel_cfg4>, nullptr},                   // 124 constraint rows per env (compiler.py: eff_njmax)
    {4, 16, -1, false, k_env_step_mf<16, 13, true, -1, false, DevModel_cupboard>, k_env_step_mf<16, 13, true, -1, false, DevModel_cupboard, true>, true},   // cupboard with its tables in LDS (HSR_TABLES_GLOBAL=0: 7 workgroups per CU)
    {4, 16, -1, true, k_env_step_mf<16, 13, true, -1, true, DevModel_cupboard>, k_env_step_mf<16, 13, true, -1, true, DevModel_cupboard, true>, true},      // 274 candidate pairs
    {-1, 16, 13, false, k_env_step_mf<16, 13, true>, nullptr},                                          // ndense at run time
    {-1, 16, -1, false, k_env_step_mf<16, 16, false>, nullptr},
    {-1, 32, -1, false, k_env_step_mf<32, 32, false>, nullptr},
#endif
};
static const PersistInstance *find_instance(int row, int group, int nv, bool tg) {
    for (const PersistInstance &p : kPersistInstances)
        if (p.row == row && p.group == group && (p.nv < 0 || p.nv == nv) && p.tg == tg) return &p;
    return nullptr;
}
static void quat2mat_h(const double *q, float *mt) {
    double n = sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
    double w = q[0]/n, x = q[1]/n, y = q[2]/n, z = q[3]/n;
    mt[0] = (float)(1 - 2*(y*y + z*z)); mt[1] = (float)(2*(x*y - w*z)); mt[2] = (float)(2*(x*z + w*y));
    mt[3] = (float)(2*(x*y + w*z)); mt[4] = (float)(1 - 2*(x*x + z*z)); mt[5] = (float)(2*(y*z - w*x));
    mt[6] = (float)(2*(x*z - w*y)); mt[7] = (float)(2*(y*z + w*x)); mt[8] = (float)(1 - 2*(x*x + y*y));
}
// the row of kCfgConsts whose constant instance may serve the model, -1 if none (or HSR_NO_CONST=1): every scalar field equal, and for a
// row compiled with its kinematic tree (kin3.h) the tree tables too, value for value (kKin3Checks, in the order tools/gen_cfg_consts.py writes them)
static int cfg_const_row(const hsr_batch *b, const hsr_model *m, const DevModel &d) {
    if (b->sw.no_const) return -1;
    int iv[sizeof kCfgConsts[0].i / sizeof(int)]; float fv[sizeof kCfgConsts[0].f / sizeof(float)];
    cfg_const_values(d, iv, fv);
    int r = 0;
    const int nrows = (int)(sizeof kCfgConsts / sizeof kCfgConsts[0]);
    while (r < nrows && !(memcmp(iv, kCfgConsts[r].i, sizeof iv) == 0 && memcmp(fv, kCfgConsts[r].f, sizeof fv) == 0)) r++;
    if (r == nrows) return -1;
    const Kin3Check &k = kKin3Checks[r];
    if (!k.i) return r;
    std::vector<int> ti = {d.nlink, d.nv};
    for (const char *n : {"link_parent", "link_free", "link_dofadr", "link_dofnum", "link_qposadr", "dof_type", "dof_qposadr", "dof_link"}) {
        size_t cnt = 0; const int *p = m->i32(n, &cnt);
        ti.insert(ti.end(), p, p + cnt);
    }
    std::vector<float> tf;
    auto addf = [&](const char *n) { size_t cnt = 0; const double *p = m->f64(n, &cnt); for (size_t i = 0; i < cnt; i++) tf.push_back((float)p[i]); };
    addf("link_pos");
    { size_t cnt = 0; const double *q = m->f64("link_quat", &cnt); for (size_t i = 0; i < cnt / 4; i++) { float mt[9]; quat2mat_h(q + 4 * i, mt); tf.insert(tf.end(), mt, mt + 9); } }
    for (const char *n : {"link_com", "link_inertia", "link_mass", "dof_axis", "dof_pos"}) addf(n);
    return k.ni == (int)ti.size() && k.nf == (int)tf.size() && memcmp(k.i, ti.data(), ti.size() * sizeof(int)) == 0
           && memcmp(k.f, tf.data(), tf.size() * sizeof(float)) == 0 ? r : -1;
}
static int upload_f(hsr_batch *b, const float **dst, const hsr_model *m, const char *name) {
    size_t cnt = 0;
    const double *src = m->f64(name, &cnt);
    if (!src) return fail(HSR_EBLOB, "blob entry '%s' missing", name);
    std::vector<float> tmp(cnt ? cnt : 1, 0.f);
    for (size_t i = 0; i < cnt; i++) tmp[i] = (float)src[i];
    return upload(b, dst, tmp);
}
static int upload_i(hsr_batch *b, const int **dst, const hsr_model *m, const char *name) {
    size_t cnt = 0;
    const int *src = m->i32(name, &cnt);
    if (!src) return fail(HSR_EBLOB, "blob entry '%s' missing", name);
    return upload(b, dst, src, cnt, 16);       // zero padding: the solver reads pair_slot in rows of eight (solve_body.inc, E2)
}
static int upload_mats(hsr_batch *b, const float **dst, const hsr_model *m, const char *quat_name) {
    size_t cnt = 0;
    const double *q = m->f64(quat_name, &cnt);
    if (!q) return fail(HSR_EBLOB, "blob entry '%s' missing", quat_name);
    size_t n = cnt / 4;
    std::vector<float> tmp(n * 9 + 1);
    for (size_t i = 0; i < n; i++) quat2mat_h(q + 4 * i, tmp.data() + 9 * i);
    return upload(b, dst, tmp);
}

// trailing free bodies: link l owns exactly the dofs [nv - 6 (k + 1), nv - 6 k), lin then ang (the constant instances are matched on nfb too)
static int trailing_free_bodies(const hsr_batch *b, const hsr_model *m) {
    const DevModel &d = b->dm;
    const int *dn = m->i32("link_dofnum"), *lf = m->i32("link_free"), *da = m->i32("link_dofadr"), *dt = m->i32("dof_type"), *dl = m->i32("dof_link");
    int nfb = 0;
    for (int k = 0; 6 * (k + 1) <= d.nv; k++) {
        const int a0 = d.nv - 6 * (k + 1), l = dl[a0];
        bool fb = l > 0 && lf[l] && da[l] == a0 && dn[l] == 6;
        for (int j = 0; fb && j < 6; j++) fb = dl[a0 + j] == l && dt[a0 + j] == (j < 3 ? DOF_FREE_LIN : DOF_FREE_ANG);
        if (!fb) break;
        nfb++;
    }
    if (nfb * 28 * (64 / b->group) > 4 * 48) nfb = 0;            // the per-body accumulators live in the box-box polygon scratch
    return std::min(nfb, b->sw.nfb_max);                         // diagnostic: HSR_NFB=0 keeps the per-contact assembly
}
// hulls staged in LDS by the instances that know their tree at compile time (their kin2 table area is free: persist.h): the hulls of the
// deepest links first (the fingers: what the hard envs run MPR on), smaller ones first within a link depth, while they fit
static int stage_hulls(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    const int *gl = m->i32("geom_link"), *gt = m->i32("geom_type"), *ma = m->i32("geom_meshadr"), *mn = m->i32("geom_meshnum"), *lp = m->i32("link_parent");
    std::vector<int> ldsv(std::max(d.ngeom, 1), -1), src;
    if (b->kin3) {
        const int budget = KIN2_FLOATS * d.nlink / 4;
        auto depth = [&](int l) { int k = 0; while (l > 0) { l = lp[l]; k++; } return k; };
        std::vector<int> order;
        for (int g = 0; g < d.ngeom; g++) if (gt[g] == GEOM_MESH && gl[g] > 0 && mn[g] > 0) order.push_back(g);
        std::stable_sort(order.begin(), order.end(), [&](int a, int bb) { const int da = depth(gl[a]), db = depth(gl[bb]); return da != db ? da > db : mn[a] < mn[bb]; });
        for (int g : order) if ((int)src.size() + mn[g] <= budget) { ldsv[g] = (int)src.size(); for (int k = 0; k < mn[g]; k++) src.push_back(ma[g] + k); }
    }
    d.nldsv = (int)src.size();
    const int rc = upload(b, &d.geom_ldsv, ldsv);
    return rc ? rc : upload(b, &d.ldsv_src, src, 1);
}
// what the persistent kernel's lane maps and kinematics assume (kin2.h, persist.h); a model outside it runs the per-substep chain
static bool fits_persist(const hsr_batch *b, const hsr_model *m) {
    const DevModel &d = b->dm;
    const int G = b->group;
    bool ok = d.nq <= G && d.nv <= G && d.nlink <= G && d.nlink <= NLMAX && d.ngeom <= 64 && d.npair < (1 << 14) && d.maxdepth <= 9;
    {   // the persistent kernel keeps every dof's chain to the root in one 64-bit register, 6 bits per dof (persist.h: anc_c)
        const int *dp = m->i32("dof_parent");
        for (int c = 0; ok && c < d.nv; c++) { int depth = 0; for (int k = c; k >= 0 && depth <= 10; k = dp[k]) depth++; if (depth > 10) ok = false; }
    }
    {
        const int *dn = m->i32("link_dofnum"), *lf = m->i32("link_free"), *lp = m->i32("link_parent"), *gl = m->i32("geom_link");
        for (int l = 1; l < d.nlink; l++) {
            if (!lf[l] && dn[l] > 3) ok = false;                          // at most three scalar joints per link record
            if (lf[l] && lp[l] != 0) ok = false;                          // free bodies hang off the world ...
            if (lf[lp[l]]) ok = false;                                    // ... and carry no children
        }
        for (int gi = d.nstatic_geom; gi < d.ngeom; gi++) if (gl[gi] == 0) ok = false;   // static geoms form a prefix of the geom list
    }
    return ok && b->persist_lds_bytes <= 160 * 1024;
}
// The persistent kernel: the instance that serves the model (kPersistInstances) and what it needs from the host - the free bodies at the
// tail of the dof vector, the hulls it stages in LDS, its tables in LDS or in global memory, its dynamic LDS, the workgroups the GPU
// holds at once.  Decided once, here; every later use reads the record.  A model outside the kernel's lane maps keeps b->kernel == NULL
// and runs the per-substep chain.
static int plan_persist(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    const int G = b->group;
    auto layout = [&](auto g, bool tg) {
        return PersistLayout<decltype(g)::value>(d.njmax, b->ds.kstride, d.npair_pad, d.nlink, d.ngeom, d.nstatic_geom, tg);
    };
    d.nfb = trailing_free_bodies(b, m);
    int row = cfg_const_row(b, m, d);
    if (row >= 0 && kKin3Checks[row].i) {      // kin3.h stages 12 floats per dof and the robot's block of M in the row-scalar region of an env (Kin3Stage): it has to fit
        const int *lf = m->i32("link_free"), *dl = m->i32("dof_link");
        int nrd = 0;
        for (int k = 0; k < d.nv; k++) nrd += lf[dl[k]] ? 0 : 1;
        const int stage = 12 * d.nv + ((nrd + 3) & ~3) * nrd;
        const int region = by_group(G, [&](auto g) { return layout(g, false).oCnt; });
        if (stage > region) row = -1;
    }
    b->const_row = row;
    b->kin3 = row >= 0 && kKin3Checks[row].i;
    const int rc = stage_hulls(b, m);
    if (rc) return rc;
    auto lds_total = [&](bool tg) { return (size_t)sizeof(float) * by_group(G, [&](auto g) { return layout(g, tg).total; }); };
    // a model whose tables cost the eighth workgroup per CU (160 KB / 8 = 20480 B each, static LDS included) reads them from global memory
    const PersistInstance *in_lds = find_instance(row, G, d.nv, false), *in_global = find_instance(row, G, d.nv, true);
    hipFuncAttributes fa;
    b->persist_tg = in_lds && in_global && !b->sw.tables_lds         // diagnostic: HSR_TABLES_GLOBAL=0 keeps the tables in LDS
                    && hipFuncGetAttributes(&fa, (const void *)in_lds->fn) == hipSuccess && lds_total(false) + fa.sharedSizeBytes > 20480
                    && hipFuncGetAttributes(&fa, (const void *)in_global->fn) == hipSuccess && lds_total(true) + fa.sharedSizeBytes <= 20480;
    b->persist_lds_bytes = lds_total(b->persist_tg);
    const PersistInstance *inst = b->persist_tg ? in_global : in_lds;
    if (!fits_persist(b, m) || !inst) { d.nfb = 0; return HSR_OK; }   // no instance: development builds carry one only
    b->kernel = inst->fn;
    b->kernel_sv = inst->sv;
    b->split_inst = inst->split;
    b->persist = true;
    for (persist_fn f : {b->kernel, b->kernel_sv})
        if (f && b->persist_lds_bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->persist_lds_bytes));
    int pb = -1;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pb, b->kernel, 64, b->persist_lds_bytes) == hipSuccess && pb > 0
        && hipGetDeviceProperties(&prop, b->device) == hipSuccess) b->slots = pb * prop.multiProcessorCount;
    if (b->sw.debug && hipFuncGetAttributes(&fa, (const void *)b->kernel) == hipSuccess)
        fprintf(stderr, "[hsrsim] k_env_step_mf<%d>: regs %d, static LDS %zu, dyn LDS %zu, scratch %zu -> %d workgroups per CU\n", G, fa.numRegs, fa.sharedSizeBytes, b->persist_lds_bytes, fa.localSizeBytes, pb);
    return HSR_OK;
}

// the model's sizes and options, and its blob tables as they are (fp64 -> fp32)
static int upload_model(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    const int *sz = m->sizes;
    d.nq = sz[HSR_NQ]; d.nv = sz[HSR_NV]; d.nu = sz[HSR_NU]; d.nlink = sz[HSR_NLINK]; d.nbody = sz[HSR_NBODY];
    d.ngeom = sz[HSR_NGEOM]; d.npair = sz[HSR_NPAIR]; d.nslot = sz[HSR_NSLOT]; d.nconmax = sz[HSR_NCONMAX]; d.njmax = sz[HSR_NJMAX];
    if (d.npair > 384) return fail(HSR_EINVAL, "more than 384 candidate geom pairs");
    if (d.ngeom > 255) return fail(HSR_EINVAL, "more than 255 geoms");
    d.nM = d.nv * (d.nv + 1) / 2;
    d.ndense = sz[13];
    d.timestep = (float)m->opt[0]; d.impratio = (float)m->opt[1]; d.gravz = (float)m->opt[2]; d.tolerance = (float)m->opt[3];
    d.iterations = (int)m->opt[4]; d.ls_iterations = (int)m->opt[5]; d.ls_tolerance = (float)m->opt[6];
    d.mpr_tolerance = (float)m->opt[7]; d.mpr_iterations = (int)m->opt[8]; d.meaninertia = (float)m->opt[9];
    int rc = 0;
#define UI(f) if ((rc = upload_i(b, &d.f, m, #f))) { return rc; }
#define UF(f) if ((rc = upload_f(b, &d.f, m, #f))) { return rc; }
    UI(link_parent) UI(link_dofadr) UI(link_dofnum) UI(link_qposadr) UI(link_free)
    UF(link_pos) UF(link_mass) UF(link_com) UF(link_inertia) UI(link_dofmask)
    UI(dof_link) UI(dof_type) UI(dof_parent) UI(dof_qposadr) UI(dof_limited)
    UF(dof_axis) UF(dof_pos) UF(dof_damping) UF(dof_invweight0) UF(dof_range) UF(dof_solref) UF(dof_solimp)
    UI(body_link) UI(body_mocap) UF(body_pos)
    UI(geom_type) UI(geom_link) UI(geom_meshadr) UI(geom_meshnum)
    UF(geom_pos) UF(geom_size) UF(geom_rbound) UF(geom_invweight) UF(mesh_vert) UF(geom_aabb)
    UI(pair_geom1) UI(pair_geom2) UI(pair_fn) UI(pair_condim) UI(pair_slot)
    UF(pair_friction) UF(pair_solref) UF(pair_solimp)
    UI(act_dof) UF(act_gear) UF(act_kp) UF(act_ctrlrange) UF(act_forcerange)
#undef UI
#undef UF
    return HSR_OK;
}
// per-pair record and dof -> actuator map
static int derive_pair_rec(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    const int *g1 = m->i32("pair_geom1"), *g2 = m->i32("pair_geom2"), *cd = m->i32("pair_condim"), *gl = m->i32("geom_link"), *ad = m->i32("act_dof");
    const double *fr = m->f64("pair_friction"), *sr = m->f64("pair_solref"), *si = m->f64("pair_solimp"), *iw = m->f64("geom_invweight");
    std::vector<float> rec((size_t)std::max(d.npair, 1) * 16, 0.f);
    for (int p = 0; p < d.npair; p++) {
        float *r = rec.data() + 16 * p;
        r[0] = (float)cd[p]; r[1] = (float)gl[g1[p]]; r[2] = (float)gl[g2[p]]; r[3] = (float)(iw[2 * g1[p]] + iw[2 * g2[p]]);
        for (int j = 0; j < 5; j++) r[4 + j] = (float)fr[5 * p + j];
        // [9], [10]: what the contact rows need of solref and solimp's dmax, formed here in double: B = 2 / (dmax timeconst), K = 1 / (dmax^2 timeconst^2 dampratio^2)
        const double dmax = std::min(std::max(si[5 * p + 1], (double)HSR_MINIMP), (double)HSR_MAXIMP), tc = sr[2 * p], dr = sr[2 * p + 1];
        r[9] = (float)(2.0 / (dmax * tc)); r[10] = (float)(1.0 / (dmax * dmax * tc * tc * dr * dr));
        for (int j = 0; j < 5; j++) r[11 + j] = (float)si[5 * p + j];
    }
    std::vector<int> da(std::max(d.nv, 1), -1);
    for (int a = 0; a < d.nu; a++) da[ad[a]] = a;
    const int rc = upload(b, &d.pair_rec, rec);
    return rc ? rc : upload(b, &d.dof_act, da);
}
// packed collision constants: one 32-float record per geom, one 8-float record per candidate pair
static int derive_collision_recs(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    const int *g1 = m->i32("pair_geom1"), *g2 = m->i32("pair_geom2"), *fn = m->i32("pair_fn"), *sl = m->i32("pair_slot");
    const int *gl = m->i32("geom_link"), *gt = m->i32("geom_type"), *ma = m->i32("geom_meshadr"), *mn = m->i32("geom_meshnum");
    const double *gp = m->f64("geom_pos"), *gq = m->f64("geom_quat"), *gs = m->f64("geom_size"), *gb = m->f64("geom_aabb"), *gr = m->f64("geom_rbound");
    std::vector<float> rec((size_t)std::max(d.npair, 1) * 8, 0.f), grec((size_t)std::max(d.ngeom, 1) * 32, 0.f);
    for (int p = 0; p < d.npair; p++) {
        float *r = rec.data() + 8 * p;
        r[0] = (float)(g1[p] + 256 * (gt[g1[p]] == GEOM_PLANE ? 1 : 0)); r[1] = (float)g2[p]; r[2] = (float)gr[g1[p]]; r[3] = (float)gr[g2[p]];   // [0]: geom1 | plane flag << 8
        r[4] = (float)fn[p]; r[5] = (float)sl[p]; r[6] = (float)(sl[p + 1] - sl[p]); r[7] = (float)gt[g1[p]];
    }
    for (int gg = 0; gg < d.ngeom; gg++) {
        // seven float4: link type nvert meshadr | lpos rbound | lmat[0..3] | lmat[4..7] | lmat[8] size | aabb centre - | aabb half -
        float *o = grec.data() + 32 * gg, lm[9];
        quat2mat_h(gq + 4 * gg, lm);
        o[0] = (float)gl[gg]; o[1] = (float)gt[gg]; o[2] = (float)mn[gg]; o[3] = (float)ma[gg];
        for (int k = 0; k < 3; k++) o[4 + k] = (float)gp[3 * gg + k];
        o[7] = (float)gr[gg];
        for (int k = 0; k < 9; k++) o[8 + k] = lm[k];
        for (int k = 0; k < 3; k++) o[17 + k] = (float)gs[3 * gg + k];
        for (int k = 0; k < 3; k++) { o[20 + k] = (float)gb[6 * gg + k]; o[24 + k] = (float)gb[6 * gg + 3 + k]; }
    }
    const int rc = upload(b, &d.pair_geo, rec);
    return rc ? rc : upload(b, &d.geom_rec, grec);
}
// what the kernels read that the blob does not hold as such: tree depths, padded hull vertices, packed records, rotation matrices, flags
static int derive_tables(hsr_batch *b, const hsr_model *m) {
    DevModel &d = b->dm;
    int rc = 0;
    {   // tree depth of every link: the persistent kernel walks the tree level by level with lane = link
        const int *lp = m->i32("link_parent");
        std::vector<int> dep(std::max(d.nlink, 1), 0);
        d.maxdepth = 0;
        for (int l = 1; l < d.nlink; l++) { dep[l] = dep[lp[l]] + 1; d.maxdepth = std::max(d.maxdepth, dep[l]); }
        if ((rc = upload(b, &d.link_depth, dep))) return rc;
    }
    {   // hull vertices as float4
        size_t cnt = 0;
        const double *mv = m->f64("mesh_vert", &cnt);
        const size_t nvt = cnt / 3;
        std::vector<float> v4((nvt + 1) * 4, 0.f);
        for (size_t i = 0; i < nvt; i++) for (int k = 0; k < 3; k++) v4[4 * i + k] = (float)mv[3 * i + k];
        if ((rc = upload(b, &d.mesh_vert4, v4))) return rc;
        const int *mn = m->i32("geom_meshnum");
        for (int g = 0; g < d.ngeom; g++) if (mn[g] > 256) return fail(HSR_EINVAL, "mesh hull with more than 256 vertices");
    }
    {   // static geoms (world link) form a prefix of the geom list in every compiled model; anything else counts as moving
        const int *gl = m->i32("geom_link");
        d.nstatic_geom = 0;
        while (d.nstatic_geom < d.ngeom && gl[d.nstatic_geom] == 0) d.nstatic_geom++;
    }
    d.npair_pad = (d.npair + 7) & ~7;
    if (d.npair_pad == 0) d.npair_pad = 8;
    if ((rc = derive_pair_rec(b, m)) || (rc = derive_collision_recs(b, m))) return rc;
    if ((rc = upload_mats(b, &d.link_mat, m, "link_quat"))) return rc;
    if ((rc = upload_mats(b, &d.geom_mat, m, "geom_quat"))) return rc;
    if ((rc = upload_mats(b, &d.body_mat, m, "body_quat"))) return rc;
    d.any_damping = 0;
    { size_t cnt; const double *dmp = m->f64("dof_damping", &cnt); for (size_t i = 0; i < cnt; i++) if (dmp[i] > 0) d.any_damping = 1; }
    d.solimp_general = 0;
    for (const char *nm : {"dof_solimp", "pair_solimp"}) {
        size_t cnt; const double *si = m->f64(nm, &cnt);
        for (size_t i = 4; si && i < cnt; i += 5) { const double pw = si[i] < 1 ? 1 : si[i]; if (pw != 1 && pw != 2) d.solimp_general = 1; }
    }
    d.cv_types = 0;
    {
        const int *g1 = m->i32("pair_geom1"), *g2 = m->i32("pair_geom2"), *fn = m->i32("pair_fn"), *gt = m->i32("geom_type");
        for (int p = 0; p < d.npair; p++) if (fn[p] == FN_CONVEX) d.cv_types |= (1 << (gt[g1[p]] & 7)) | (256 << (gt[g2[p]] & 7));
    }
    return HSR_OK;
}
// the state arrays, [rows][N], zeroed; the counters and the work queue of the persistent kernel
static int alloc_state(hsr_batch *b) {
    const DevModel &d = b->dm;
    DevState &s = b->ds;
    const size_t N = (size_t)b->N;
    int rc = 0;
    s.N = b->N;
    s.npair_sep = std::max(d.npair, 1);
#define DA(field, rows) if ((rc = dalloc(b, &s.field, (size_t)(rows) * N))) return rc;
    DA(qpos, d.nq) DA(qvel, d.nv) DA(ctrl, d.nu) DA(mocap, 3) DA(warm, d.nv) DA(time, 1)
    DA(done, 1) DA(bad, 1) DA(nsteps, 1)
    DA(xpos, 3 * d.nlink) DA(xmat, 9 * d.nlink) DA(lvel, 6 * d.nlink)
    s.kstride = (9 * d.nv + 15 * d.nlink + 15) & ~15;
    DA(kin_aos, s.kstride)
    DA(con, 8 * d.nslot) DA(ncon_pair, d.npair_pad) DA(sepax, 4 * std::max(d.npair, 1)) DA(septick, std::max(d.npair, 1)) DA(tick, 1) DA(pair_list, std::max(d.npair, 1))
    if ((rc = dalloc(b, &s.pair_count, (size_t)d.npair_pad))) return rc;
    if ((rc = dalloc(b, &s.pair_pack, (size_t)((d.npair_pad + 7) & ~7)))) return rc;
    if ((rc = dalloc(b, &s.geom_c, (size_t)8 * std::max(d.ngeom, 1)))) return rc;
    DA(M, d.nM) DA(qacc, d.nv) DA(qacc_smooth, d.nv) DA(qfrc_smooth, d.nv) DA(qfrc_constraint, d.nv)
    DA(ncon, 1) DA(nefc, 1) DA(niter, 1)
#undef DA
    if ((rc = dalloc(b, &s.phase_cyc, 32 + 40 * 8192))) return rc;
    if ((rc = dalloc(b, &s.capstat, 12))) return rc;
    if ((rc = dalloc(b, &s.trips, N))) return rc;
    // (a splitting launch gives every workgroup a task row of its own behind the tasks' rows: persist.h)
    if ((rc = dalloc(b, &b->d_slot_env, 2 * (N + 64) + 4 * (size_t)SPLIT_MAX_EXTRA))) return rc;
    // work queue of the persistent kernel: up to QUEUE_ROUNDS rounds of one ticket per task (a task = the envs of one workgroup)
    const size_t tasks = (N + 1) / 2;
    if ((rc = dalloc(b, &s.q_head, QUEUE_ROUNDS))) return rc;
    if ((rc = dalloc(b, &s.q_wpos, QUEUE_ROUNDS))) return rc;
    if ((rc = dalloc(b, &s.q_items, (size_t)QUEUE_ROUNDS * tasks))) return rc;
    if ((rc = dalloc(b, &s.q_err, 1))) return rc;
    s.sq_cap = (int)N + 4096;
    if ((rc = dalloc(b, &s.sq_items, (size_t)s.sq_cap))) return rc;
    if ((rc = dalloc(b, &s.sq_ctl, SPLIT_CTL_WORDS))) return rc;
    s.solo_servers = 0; s.solo_trips_x4 = 14; s.solo_min_left = 40;
    s.split_period = 0; s.split_trips_x4 = 14; s.split_min_left = 40; s.split_lone_x4 = 0;
    s.q_chunk = 0;
    s.slot_env = nullptr;
    return HSR_OK;
}
// cooperative solver geometry (16 lanes per env when nv <= 16, else 32), what it bounds, and the dynamic LDS of k_solve_mf
static int size_solver(hsr_batch *b) {
    const DevModel &d = b->dm;
    b->group = d.nv <= 16 ? 16 : 32;
    if (d.nv > 32 || d.nq > 64 || d.nlink > NLMAX || d.nconmax > b->group || b->ds.kstride > 8 * 4 * b->group)
        return fail(HSR_EINVAL, "model exceeds the lane-group solver (nv <= 32, nlink <= 16, nconmax <= lanes per env)");
    const int total = by_group(b->group, [&](auto g) { return MfLayout<decltype(g)::value>(d.njmax, b->ds.kstride).total; });
    b->mf_lds_bytes = (size_t)total * (64 / b->group) * sizeof(float);
    if (b->mf_lds_bytes > 160 * 1024) return fail(HSR_EINVAL, "model exceeds the LDS budget of the solver");
    if (b->mf_lds_bytes <= 48 * 1024) return HSR_OK;
    const void *fn = by_group(b->group, [](auto g) { return (const void *)k_solve_mf<decltype(g)::value>; });
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->mf_lds_bytes));
    return HSR_OK;
}
static int size_kinematics(hsr_batch *b) {
    const size_t kb = (size_t)64 * (b->ds.kstride + 24 * b->dm.nlink + 1) * sizeof(float);
    if (kb > 160 * 1024) return fail(HSR_EINVAL, "kinematics tile exceeds LDS");
    if (kb > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)k_kinematics, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kb));
    return HSR_OK;
}
// staging of the host-pointer API, the profiling events, and the initial state = mj_resetData
static int alloc_staging_and_reset(hsr_batch *b, const hsr_model *m) {
    const DevModel &d = b->dm;
    const size_t N = (size_t)b->N;
    int rc = 0;
    b->stage_floats = N * (size_t)(std::max(std::max(std::max(d.nq + d.nv, 25), 7 * d.nslot), std::max(d.nv * d.nv, 9 * d.nlink)) + d.nu + d.nq + d.nv + 4) + 16;
    if ((rc = dalloc(b, &b->d_stage, b->stage_floats))) return rc;
    if ((rc = dalloc(b, &b->d_stage_u8, N))) return rc;
    if ((rc = dalloc(b, &b->d_stage_i32, N))) return rc;
    HIPCHK(hipEventCreate(&b->ev0));
    HIPCHK(hipEventCreate(&b->ev1));
    if ((rc = upload(b, &b->d_qpos0, m->qpos0.data(), (size_t)d.nq))) return rc;
    hipLaunchKernelGGL(k_build_tables, grid1((size_t)std::max(d.ngeom, (d.npair_pad + 7) & ~7)), dim3(256), 0, b->stream, b->dm, b->ds);
    hipLaunchKernelGGL(k_reset, grid1(N), dim3(256), 0, b->stream, b->dm, b->ds, (const uint8_t *)nullptr, (const float *)nullptr,
                       (const float *)b->d_qpos0, (const float *)nullptr, 0);
    HIPCHK(hipStreamSynchronize(b->stream));
    return HSR_OK;
}

static int batch_init(hsr_batch *b, const hsr_model *m) {
    int rc;
    HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    if ((rc = upload_model(b, m)) || (rc = derive_tables(b, m)) || (rc = alloc_state(b)) || (rc = size_solver(b))) return rc;
    if ((rc = plan_persist(b, m)) || (rc = size_kinematics(b))) return rc;
    return alloc_staging_and_reset(b, m);
}
extern "C" int hsr_batch_create(const hsr_model *m, int n_envs, int device_id, hsr_batch **out) {
    if (!m || !out || n_envs <= 0) return fail(HSR_EINVAL, "bad arguments to hsr_batch_create");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(HSR_EDEVICE, "no HIP device available%s");
    if (device_id < 0 || device_id >= ndev) return fail(HSR_EINVAL, "device id out of range");
    HIPCHK(hipSetDevice(device_id));
    hsr_batch *b = new hsr_batch();
    b->model = m; b->N = n_envs; b->device = device_id;
    read_switches(b);
    const int rc = batch_init(b, m);
    if (rc) { hsr_batch_destroy(b); return rc; }       // frees the stream, the events and every allocation made so far
    *out = b;
    return HSR_OK;
}

extern "C" void hsr_batch_destroy(hsr_batch *b) {
    if (!b) return;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    for (auto &kv : b->graphs) hipGraphExecDestroy(kv.second);
    snap_release_all(b);
    replay_release_all(b);
    rollout_release_all(b);
    norm_release_all(b);
    plan_release_all(b);
    for (void *p : b->allocs) hipFree(p);
    if (b->d_rimg) hipFree(b->d_rimg);
    if (b->d_cap) hipFree(b->d_cap);
    for (hipEvent_t ev : b->kev) hipEventDestroy(ev);
    for (auto &pr : b->klog) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    if (b->ev0) hipEventDestroy(b->ev0);
    if (b->ev1) hipEventDestroy(b->ev1);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
}
