// Shared body of the matrix-free solver (phases B..G up to the new velocity), textually included by
// k_solve_mf (one substep per launch) and k_env_step_mf (persistent substep loop) so that both run identical code.
// Expects in scope: NK (compile-time bound on nv: matrix loops run k < NK <= G), lvbuf / lvcap (LDS scratch for the per-link
// velocity fields of jmul: 6 lvcap floats per env), m, s, N, nv, R, MS, e, c, g, tid, valid, isdof, bad, mode, debug, the LDS pointers (rD.., kAng.., M, con,
// sParent, sMask, sMass), the per-lane inputs (qvel_c, warm_c, my_q, my_ctrl, damp_c, my_limited, my_act, lim_*, act_p,
// the macro PAIR_CNT8(p) = the contact counts of the candidate pairs p .. p + 7 of this env, one byte each, p a multiple of 8 below npair), fbK / nfb (LDS accumulators of the per-body Hessian assembly: 28 floats per
// trailing free body of this env; nfb = 0 turns it off) and the kin record already in LDS.  Leaves: qacc_c, qfc_c, acc_c, vnew, ncon, nefc, iter.
    v3 a_c = mk3(0, 0, 0), l_c = mk3(0, 0, 0), n_c = mk3(0, 0, 0);
#ifdef SOLVE_LANE_TABLES
#define LINK_MOVES_WITH_DOF(l) ((sub_c >> (l)) & 1u)          // from the lane's register (persist.h)
#else
#define LINK_MOVES_WITH_DOF(l) ((sMask[l] >> c) & 1)
#endif
    float bias_c = 0;
    float Mrow[G];
    float Mdiag_c;          // NDK >= 0 (compile-time ndense): the tail lanes factor / solve with their own diagonal entry
    if constexpr (KIN3) {
        // the kinematics pass (kin3.h) has left this lane's dof record, its row of M and its bias force in the staging area
        Kin3Lane<G> k3l;
        kin3_fetch<typename Kin3Of<MT>::type, G, NK>(c, kAng, k3l);
        a_c = k3l.a; l_c = k3l.l; n_c = k3l.n; bias_c = k3l.bias; Mdiag_c = k3l.Mdiag;
#pragma unroll
        for (int k = 0; k < NK; k++) Mrow[k] = k3l.Mrow[k];
        PHASE(0);
    } else {
#pragma unroll
    for (int k = 0; k < G + 1; k++) M[c * MS + k] = 0.f;
    wave_sync();
    if (isdof) {
        a_c = mk3(kAng[3 * c], kAng[3 * c + 1], kAng[3 * c + 2]);
        l_c = mk3(kLin[3 * c], kLin[3 * c + 1], kLin[3 * c + 2]);
        n_c = mk3(kAnc[3 * c], kAnc[3 * c + 1], kAnc[3 * c + 2]);
    }
    PHASE(0);
    // ---------------- phase B/C: inertia rows (a-2.2), bias force (a-2.5), lane = dof
    if (isdof) {
        // M[c][k] for k = c and its ancestor dofs: sum over the links l below dof c of jp_k(l) . (m_l jp_c(l)) + a_k . (I_l a_c).
        // With jp_k(l) = lin_k + a_k x (com_l - anc_k) the sum over l separates from k:
        //   M[c][k] = lin_k . V + a_k . (T + (n_c - anc_k) x V + U),   V = sum m_l jp_c(l), U = sum I_l a_c,
        //   T = sum (com_l - n_c) x (m_l jp_c(l))        (moments taken about dof c's own anchor: no large lever arms)
        // one pass over the links, then one dot-product pair per ancestor
        v3 V = mk3(0, 0, 0), U = mk3(0, 0, 0), T = mk3(0, 0, 0);
        for (int l = 1; l < m.nlink; l++) {
            if (!LINK_MOVES_WITH_DOF(l)) continue;
            const float *q = lk + 15 * l;
            const v3 com = mk3(q[0], q[1], q[2]), F = mk3(q[9], q[10], q[11]), Nt = mk3(q[12], q[13], q[14]);
            const v3 r = com - n_c;
            const v3 jpc = l_c + cross(a_c, r);
            const v3 v = jpc * sMass[l];
            const v3 u = mk3(q[3] * a_c.x + q[6] * a_c.y + q[7] * a_c.z, q[6] * a_c.x + q[4] * a_c.y + q[8] * a_c.z, q[7] * a_c.x + q[8] * a_c.y + q[5] * a_c.z);
            bias_c += dot(jpc, F) + dot(a_c, Nt);
            V = V + v; U = U + u; T = T + cross(r, v);
        }
        const v3 TU = T + U;
        PHASE_S(4, 26);
#ifdef SOLVE_LANE_TABLES
        for (unsigned long long al_ = anc_c; al_ != 0; al_ >>= 6) {
            const int k = (int)(al_ & 63u) - 1;
#else
        for (int k = c; k >= 0; k = sParent[k]) {
#endif
            const v3 ak = mk3(kAng[3 * k], kAng[3 * k + 1], kAng[3 * k + 2]), lk_ = mk3(kLin[3 * k], kLin[3 * k + 1], kLin[3 * k + 2]);
            const v3 dk = n_c - mk3(kAnc[3 * k], kAnc[3 * k + 1], kAnc[3 * k + 2]);
            M[c * MS + k] = dot(lk_, V) + dot(ak, TU + cross(dk, V));
        }
    }
    PHASE_S(4, 27);
    wave_sync();
    PHASE_S(4, 28);
#ifdef SOLVE_LANE_TABLES
    if (isdof) for (unsigned long long al_ = anc_c >> 6; al_ != 0; al_ >>= 6) { const int k = (int)(al_ & 63u) - 1; M[k * MS + c] = M[c * MS + k]; }   // mirror
#else
    if (isdof) for (int k = sParent[c]; k >= 0; k = sParent[k]) M[k * MS + c] = M[c * MS + k];   // mirror
#endif
    if (!isdof) M[c * MS + c] = 1.f;
    wave_sync();
    if (debug && valid && isdof) for (int k = 0; k <= c; k++) s.M[(size_t)(c * (c + 1) / 2 + k) * N + e] = M[c * MS + k];
#pragma unroll
    for (int k = 0; k < NK; k++) Mrow[k] = M[c * MS + k];
    PHASE_S(4, 29);
    Mdiag_c = M[c * MS + c];
    }
    float qfs_c = 0;
    if (isdof) {
        qfs_c = -damp_c * qvel_c - bias_c;
        if (my_act >= 0) {
            const float ct = fminf(fmaxf(my_ctrl, act_p[2]), act_p[3]);
            float f = act_p[0] * ct - act_p[0] * act_p[1] * my_q;
            f = fminf(fmaxf(f, act_p[4]), act_p[5]);
            qfs_c += act_p[1] * f;
        }
    }

    PHASE(1);
#ifdef SOLVE_LIMITS_FROM_MODEL
    // the constants of this lane's joint limit are read here, ahead of the factorisation of M (pure register arithmetic for a while), and used right
    // after it (E1): as launch-long registers they were parked in scratch memory and reloaded at their first use, a round trip in plain sight
    float lim_lo = 0, lim_hi = 0, lim_iw = 0, lim_sr0 = 1, lim_sr1 = 1, lim_si[5] = {0, 0, 0, 0, 0};
    if (isdof && my_limited) {
        typedef const __attribute__((address_space(1))) float *gcf_;
        const gcf_ rg_ = (gcf_)m.dof_range, sr_ = (gcf_)m.dof_solref, si_ = (gcf_)m.dof_solimp, iw_ = (gcf_)m.dof_invweight0;
        lim_lo = rg_[2 * c]; lim_hi = rg_[2 * c + 1]; lim_sr0 = sr_[2 * c]; lim_sr1 = sr_[2 * c + 1]; lim_iw = iw_[c];
#pragma unroll
        for (int j = 0; j < 5; j++) lim_si[j] = si_[5 * c + j];
    }
#endif
    // the first contact slots of this lane's eight candidate pairs of the compaction's first round (E2): fetched here, used after the factorisation -
    // in E2 itself the load was a global round trip in the dependent chain of every substep
    int4 pslot_a = make_int4(0, 0, 0, 0), pslot_b = pslot_a;
    if (8 * c < m.npair_pad) {
        typedef int v4i_ __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) v4i_ *gci4_;
        const gci4_ ps_ = (gci4_)(m.pair_slot + 8 * c);
        const v4i_ pa_ = ps_[0], pb_ = ps_[1];
        pslot_a = make_int4(pa_.x, pa_.y, pa_.z, pa_.w); pslot_b = make_int4(pb_.x, pb_.y, pb_.z, pb_.w);
    }
    // ---------------- qacc_smooth = M^-1 qfrc_smooth
    float qas_c;
    {
        float Lr[G];
#pragma unroll
        for (int k = 0; k < NK; k++) Lr[k] = Mrow[k];
        float invd;
        if constexpr (NDK >= 0) {
            if (!chol_g_tail<G, NK, NDK>(Lr, invd, Mdiag_c, c)) bad = 1;
            qas_c = chol_solve_tail<G, NK, NDK>(Lr, invd, qfs_c, c);
        } else {
            if (!chol_g<G, NK>(Lr, invd, nv, m.ndense, c)) bad = 1;
            qas_c = chol_solve_mf<G, NK>(Lr, invd, qfs_c, nv, c);
        }
        if (!isdof) qas_c = 0;
    }
    wave_sync();          // M (LDS) is dead from here: its region becomes the contact records

    PHASE(2);
    // ---------------- phase E: constraint assembly (a-2.4)
    // E2 contact compaction in (pair, index) order: lane c owns the eight CONSECUTIVE candidate pairs 8 c .. 8 c + 7 of a round (their
    // counts are one 64-bit read), so that lane order is pair order and one scan per round of 8 G pairs places every contact
    // (a round without any contact is skipped wave-uniformly); only the lanes that own contacts walk their bytes
    int ncon = 0;
    {
        int base = 0;
        for (int p0 = 0; p0 < m.npair; p0 += 8 * G) {
            const int pb = p0 + 8 * c;
            unsigned long long c8 = (valid && pb < m.npair) ? PAIR_CNT8(pb) : 0ull;
            const int mine = (int)((c8 * 0x0101010101010101ull) >> 56);      // sum of the eight counts (each <= 8)
            if (__ballot(mine > 0) == 0ull) continue;
            const int incl = gscan_incl<G>(mine, c);
            const int tot = glast<G>(incl);
            int ci = base + incl - mine;
            while (c8) {
                const int k = (__ffsll((long long)c8) - 1) >> 3;
                const int cnt = (int)((c8 >> (8 * k)) & 0xffull);
                c8 &= ~(0xffull << (8 * k));
                const int sl8[8] = {pslot_a.x, pslot_a.y, pslot_a.z, pslot_a.w, pslot_b.x, pslot_b.y, pslot_b.z, pslot_b.w};
                int slot0 = sl8[0];
#pragma unroll
                for (int q = 1; q < 8; q++) slot0 = k == q ? sl8[q] : slot0;
                if (p0 > 0) slot0 = m.pair_slot[pb + k];          // later rounds (models with more than 8 G candidate pairs)
                for (int i = 0; i < cnt; i++, ci++)
                    if (ci < G) { float *cr = con + C2_SIZE * ci; cr[C2_PAIR] = (float)(pb + k); cr[C2_SLOT] = (float)(slot0 + i); }
            }
            base += tot;
        }
        ncon = base < G ? base : G;
        if (ncon > m.nconmax) ncon = m.nconmax;
#ifdef SOLVE_COUNT_CAPS
        if (valid && c == 0 && base > ncon) cap_con++;
#endif
    }
    wave_sync();
    PHASE(3);
    // E3 lane = contact: frame, impedance, regulariser, row addresses.  Its global reads (the pair's constants, the contact the narrowphase wrote) are
    // issued first and the limit rows (E1: registers only) are formed while they are under way
    float4 e3_pr[4] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)}, e3_cd0 = make_float4(0, 0, 0, 0), e3_cd1 = e3_cd0;
    if (c < ncon) {
        const float *cr = con + C2_SIZE * c;
        const int p = (int)cr[C2_PAIR], slot = (int)cr[C2_SLOT];
        typedef float v4f_ __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) v4f_ *gcf4_;
        const gcf4_ prp = (gcf4_)(m.pair_rec + 16 * p);
        const gcf4_ cdp = (gcf4_)(s.con + ((size_t)e * m.nslot + slot) * 8);
        const v4f_ r0_ = prp[0], r1_ = prp[1], r2_ = prp[2], r3_ = prp[3], c0_ = cdp[0], c1_ = cdp[1];
        e3_pr[0] = make_float4(r0_.x, r0_.y, r0_.z, r0_.w); e3_pr[1] = make_float4(r1_.x, r1_.y, r1_.z, r1_.w); e3_pr[2] = make_float4(r2_.x, r2_.y, r2_.z, r2_.w);
        e3_pr[3] = make_float4(r3_.x, r3_.y, r3_.z, r3_.w); e3_cd0 = make_float4(c0_.x, c0_.y, c0_.z, c0_.w); e3_cd1 = make_float4(c1_.x, c1_.y, c1_.z, c1_.w);
    }
    // E1 joint limits: rows in dof order (lower side then upper side); everything about a limit row stays in the
    // registers of its dof lane (index 0 = lower, 1 = upper)
    int nlim;
    bool lim_on[2] = {false, false};
    float lim_D[2] = {0, 0}, lim_aref[2] = {0, 0}, lim_gr[2] = {0, 0}, lim_dw[2] = {0, 0};
    {
        float dlo = 0, dhi = 0;
        if (valid && my_limited) { dlo = my_q - lim_lo; dhi = lim_hi - my_q; lim_on[0] = dlo < 0; lim_on[1] = dhi < 0; }
        const int cnt = (int)lim_on[0] + (int)lim_on[1];
        const int incl = gscan_incl<G>(cnt, c);
        nlim = glast<G>(incl);
        int r = incl - cnt;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            if (lim_on[side]) {
                if (r < R) {
                    const float dist = side == 0 ? dlo : dhi, sg = side == 0 ? 1.f : -1.f;
                    // lim_B = 2 / (dmax timeconst), lim_K = 1 / (dmax^2 timeconst^2 dampratio^2): constants of the joint, formed once per launch
#ifdef SOLVE_LIMITS_FROM_MODEL
                    const float dmax_ = fminf(fmaxf(lim_si[1], HSR_MINIMP), HSR_MAXIMP);          // the expressions of the launch prologue (solve_mf.h), bit for bit
                    const float lim_B = 2.0f / (dmax_ * lim_sr0), lim_K = 1.0f / (dmax_ * dmax_ * lim_sr0 * lim_sr0 * lim_sr1 * lim_sr1);
#endif
                    const float imp = impedance<SolimpGeneral<MT>::value>(lim_si, dist);
                    lim_aref[side] = -lim_B * sg * qvel_c - imp * lim_K * dist;
                    lim_D[side] = frcp(fmaxf((1 - imp) * frcp(imp) * lim_iw, HSR_MINVAL));
                } else lim_on[side] = false;
                r++;
            }
        }
        if (nlim > R) nlim = R;
    }
    PHASE_S(5, 26);
    int nefc = nlim, lmask = 0;
    // SPARSE_CHOL: 32-lane instances whose dofs are a robot's dense block followed by several free bodies: chol_sparse_fwd / chol_sparse_back factor the Newton Hessian; in the substeps in
    // which every env of the wave couples at most one body to the robot and none to another (sparse_ok: wave-uniform, per substep) the bodies' pivot steps are merged
    constexpr bool SPARSE_CHOL = G == 32 && EXACT_CT && NDK > 0 && (NK - NDK) % 6 == 0 && (NK - NDK) / 6 >= 2;
    bool sparse_ok = false;
    (void)sparse_ok;
    int kslots = 0;          // contact lane: the scratch slots of its two links (s1 + 32 s2): J v reads the link fields without first reading its record for them
    // trailing free bodies: lane c of body my_fb is its dof my_kk; contacts of such a body with the world (bits of fbmask; the
    // others in dmask) enter the Newton Hessian through one 6 x 6 matrix per body instead of one rank-1 update per row
    const int fb_base = nv - 6 * nfb;
    const int my_fb = (isdof && c >= fb_base) ? (c - fb_base) / 6 : -1, my_kk = c - fb_base - 6 * my_fb;
    unsigned fbmask = 0, dmask = 0, relmask = 0;
    // contact dims as two bit masks per env (dim = 1 + 2 lo + 3 hi: 1, 3, 4, 6), so that the row address of contact ci is
    // nlim + ci + 2 popc(lo below ci) + 3 popc(hi below ci) - register arithmetic instead of a dependent LDS read of its record
    unsigned dim_lo = 0, dim_hi = 0;
    if (my_fb >= 0 && my_kk == 3) { float *K = fbK + 28 * my_fb; K[24] = n_c.x; K[25] = n_c.y; K[26] = n_c.z; }     // reference point of the body's 6 x 6 matrix: its origin
    {
        int dim = 0, fbi = -1;
        float *cr = con + C2_SIZE * c;
        const float4 (&pr)[4] = e3_pr; const float4 cd0 = e3_cd0, cd1 = e3_cd1;
        if (c < ncon) dim = (int)pr[0].x;
        PHASE_S(5, 27);
        const int incl = gscan_incl<G>(dim, c);
        const int adr = nlim + incl - dim;
        const bool ovf = c < ncon && adr + dim > R;
        unsigned long long bal = __ballot(ovf);
        const unsigned int gm = (unsigned int)((bal >> (g * G)) & ((G == 32) ? 0xffffffffull : 0xffffull));
        if (gm) ncon = __ffs(gm) - 1;
#ifdef SOLVE_COUNT_CAPS
        {   // rows beyond njmax are dropped: count the event, and how far beyond the cap the env wanted to go (capstat[4 ..]: 8 rows per bin)
            const int want = nlim + glast<G>(incl);
            if (valid && c == 0 && (gm || nlim >= R)) { cap_row++; const int bin = (want - R - 1) >> 3; atomicAdd(&s.capstat[4 + (bin < 0 ? 0 : (bin > 7 ? 7 : bin))], 1ull); }
        }
#endif
        if (c < ncon) {
            const v3 pos = mk3(cd0.x, cd0.y, cd0.z), nrm = mk3(cd0.w, cd1.x, cd1.y);
            const float dist = cd1.z;
            v3 t1 = (nrm.y > -0.5f && nrm.y < 0.5f) ? mk3(0, 1, 0) : mk3(0, 0, 1);
            t1 = normalized(t1 - nrm * dot(nrm, t1));
            const v3 t2 = cross(nrm, t1);
            const float fri[5] = {pr[1].x, pr[1].y, pr[1].z, pr[1].w, pr[2].x};
            const float solimp[5] = {pr[2].w, pr[3].x, pr[3].y, pr[3].z, pr[3].w};
            // pair constants formed on the host (host_create.h: derive_pair_rec): B = 2 / (dmax timeconst), K = 1 / (dmax^2 timeconst^2 dampratio^2)
            const float tran = pr[0].w;
            const float imp = impedance<SolimpGeneral<MT>::value>(solimp, dist);
            const float B = pr[2].y, Kimp = imp * pr[2].z;
            // regularisers: R0 = (1 - imp) / imp * diagApprox, friction rows R1 = R0 / impratio, R_j = R1 mu0^2 / mu_j^2 - only their reciprocals are used
            const float ir = fmaxf(m.impratio, HSR_MINVAL);
            const float iR0 = frcp(fmaxf((1 - imp) * frcp(imp) * tran, HSR_MINVAL)), iR1 = iR0 * ir, if0 = frcp(fri[0] * fri[0]);
            cr[C2_POS] = pos.x; cr[C2_POS + 1] = pos.y; cr[C2_POS + 2] = pos.z;
            cr[C2_N] = nrm.x; cr[C2_N + 1] = nrm.y; cr[C2_N + 2] = nrm.z;
            cr[C2_T1] = t1.x; cr[C2_T1 + 1] = t1.y; cr[C2_T1 + 2] = t1.z;
            cr[C2_T2] = t2.x; cr[C2_T2 + 1] = t2.y; cr[C2_T2 + 2] = t2.z;
            // the dof masks of the two links' chains (bit patterns, never used as numbers): what every consumer wants from the link ids
            cr[C2_L1] = __int_as_float(sMask[(int)pr[0].y]); cr[C2_L2] = __int_as_float(sMask[(int)pr[0].z]);
            cr[C2_ADR] = (float)adr; cr[C2_DIM] = (float)dim;
            cr[C2_MU] = dim > 1 ? fri[0] * frsq(ir) : fri[0];           // mu = fri sqrt(R1 / R0)
            cr[C2_F0] = fri[0]; cr[C2_F2] = fri[2]; cr[C2_F3] = fri[3];
            cr[C2_ZONE] = -1.f;
            cr[C2_B] = B; cr[C2_KD] = Kimp * dist;
            for (int j = 0; j < dim; j++) rD[adr + j] = j == 0 ? iR0 : (j == 1 ? iR1 : iR1 * (fri[j - 1] * fri[j - 1]) * if0);
        }
        PHASE_S(5, 28);
        // distinct moving links among the kept contacts: bit l of lmask; a contact stores the slots (rank of the bit) of its
        // two links, 0 = world, in its record
        {
            const int l1 = (int)pr[0].y, l2 = (int)pr[0].z;
            lmask = gor<G>((c < ncon) ? (((l1 ? 1 << l1 : 0) | (l2 ? 1 << l2 : 0))) : 0);
            if constexpr (SPARSE_CHOL) {
                // which bodies does this env's contact list couple?  At most one body to the robot and no body to another: the sparse factorisation (solve_g.h) applies.
                // Per env (group-uniform), never a property of the wave: a result must not depend on the env's neighbours.
                const unsigned rb_ = (1u << (NDK > 0 ? NDK : 0)) - 1u;
                const unsigned m1_ = (c < ncon && l1) ? (unsigned)sMask[l1] : 0u, m2_ = (c < ncon && l2) ? (unsigned)sMask[l2] : 0u;
                const bool r1_ = (m1_ & rb_) != 0u, r2_ = (m2_ & rb_) != 0u;
                const bool two_ = c < ncon && l1 != 0 && l2 != 0;
                const int bodies_ = gor<G>((two_ && r1_ != r2_) ? (int)((r1_ ? m2_ : m1_) >> (NDK > 0 ? NDK : 0)) : 0);
                const int bb_ = gor<G>((two_ && !r1_ && !r2_) ? 1 : 0);
                // Wave-uniform: the sparse factorisation performs the dense one's arithmetic on the entries that are not structurally zero, in the same order, and skips
                // updates by exact zeros - its results are BIT-IDENTICAL (test_sparse_factorisation_equals_the_dense_one asserts it), so that which of the two a wave runs
                // never shows in an env's result.  (A per-env choice under exec masks ran both paths in practice: 12 % slower than the dense one alone.)
                sparse_ok = !wave_any(!(bb_ == 0 && __popc((unsigned)bodies_ & 0x41041041u) <= 1)) && !hook_dense_chol;          // (bit 0 of every six-dof tile)
            }
#ifdef HSR_CPLSTAT
            {   // diagnostic (timing build, tools/block_times.py with HSR_CPLSTAT=1): which bodies does the env's contact list couple?  Counter 3 of lane 0's env:
                // substeps with no robot <-> body contact | exactly one body coupled to the robot and no body <-> body contact << 21 | anything else << 42
                const unsigned rb_ = (NDK > 0) ? ((1u << NDK) - 1u) : 0u;
                const unsigned m1_ = (c < ncon && l1) ? (unsigned)sMask[l1] : 0u, m2_ = (c < ncon && l2) ? (unsigned)sMask[l2] : 0u;
                const bool r1_ = (m1_ & rb_) != 0u, r2_ = (m2_ & rb_) != 0u;
                const bool rbody_ = c < ncon && l1 && l2 && (r1_ != r2_);
                const bool bbody_ = c < ncon && l1 && l2 && !r1_ && !r2_;
                const int bodies_ = gor<G>(rbody_ ? (int)((r1_ ? m2_ : m1_) >> NDK) : 0);
                const int bb_ = gor<G>(bbody_ ? 1 : 0);
                const int nb_ = __popc(bodies_ & 0x41041);          // bit 0 of every six-dof tile
                if (valid && nefc >= 0) dc_[3] += (nb_ == 0 && !bb_) ? 1ull : ((nb_ == 1 && !bb_) ? (1ull << 21) : (1ull << 42));
            }
#endif
            if (c < ncon) {
                const int s1 = l1 ? 1 + __popc(lmask & ((1 << l1) - 1)) : 0, s2 = l2 ? 1 + __popc(lmask & ((1 << l2) - 1)) : 0;
                // world <-> trailing free body (one chain mask empty, the other exactly the six dofs of body fbi): assembled per body
                if (nfb > 0 && (l1 == 0) != (l2 == 0)) {
                    const unsigned mm = (unsigned)sMask[l1 | l2];
                    const int lb = __ffs(mm) - 1 - fb_base;
                    if (lb >= 0 && lb % 6 == 0 && mm == (0x3fu << (lb + fb_base))) fbi = lb / 6;
                }
                cr[C2_PAIR] = (float)(s1 + 32 * s2 + 1024 * (fbi + 1));
                kslots = s1 + 32 * s2;
            }
        }
        {
            const unsigned long long bf = __ballot(c < ncon && fbi >= 0), bd = __ballot(c < ncon && fbi < 0);
            constexpr unsigned long long GM = (G == 32) ? 0xffffffffull : 0xffffull;
            fbmask = (unsigned)((bf >> (g * G)) & GM); dmask = (unsigned)((bd >> (g * G)) & GM);
            const unsigned long long bl = __ballot(c < ncon && (dim == 3 || dim == 6)), bh = __ballot(c < ncon && (dim == 4 || dim == 6));
            dim_lo = (unsigned)((bl >> (g * G)) & GM); dim_hi = (unsigned)((bh >> (g * G)) & GM);
            // the contacts whose Jacobian has an entry in lane c's dof at all: the body-coupling ones, and for a dof of a trailing free body
            // the world contacts of that body - J^T f (every Newton iteration) walks these instead of all contacts
            relmask = dmask;
            for (int b = 0; b < nfb; b++) { const unsigned long long bb = __ballot(c < ncon && fbi == b); if (my_fb == b) relmask |= (unsigned)((bb >> (g * G)) & GM); }
        }
        // total row count = address past the last kept contact
        const int endrow = (c < ncon) ? adr + dim : nlim;
        nefc = gmax<G>(endrow);
    }
    wave_sync();
    PHASE(4);

    // (J v) for every contact row into out[] (no aref); lane c contributes v_c.
    // J v at a contact = ax . (V_l2(pos) - V_l1(pos)) with V_l(p) = A_l + W_l x p the velocity field of link l under v:
    //   W_l = sum_{c in chain(l)} v_c a_c,  A_l = sum_c v_c (l_c - a_c x n_c)        (six width-G reductions per DISTINCT link,
    // not per contact: the four corner contacts of a resting block share one link), then lane = contact forms its rows.
    const v3 b_c = l_c - cross(a_c, n_c);
    // J v: the six rows of lane c's contact (zero beyond its dim) land in that lane's registers jv[] - nobody else ever reads them, so
    // neither they nor the residual and the reference acceleration built from them pass through LDS
    auto jmul_links = [&](float vc, float (&jv)[6]) {
        // slot 0 of the scratch is the world (a zero field): a contact then subtracts the fields of its two links without asking which is
        // which; slot k >= 1 belongs to the k-th distinct moving link
        if (c < 6) lvbuf[c] = 0.f;
        int slot = 1;
        for (int mm = lmask; mm; mm &= mm - 1, slot++) {
            const int l = __ffs(mm) - 1;
            const float w = LINK_MOVES_WITH_DOF(l) ? vc : 0.f;
            const float p[6] = {b_c.x * w, b_c.y * w, b_c.z * w, a_c.x * w, a_c.y * w, a_c.z * w};
            const float r = gsum6_packed<G>(p, c);
            const int q = gsum6_index(c);
            if (c < 16 && (c & 1) == 0 && q < 6) lvbuf[6 * slot + q] = r;
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < 6; j++) jv[j] = 0.f;
        if (c < ncon) {
            const float *cr = con + C2_SIZE * c;
            const float4 q0 = lds4(cr), q1 = lds4(cr + 4), q2 = lds4(cr + 8), q3 = lds4(cr + 12);
            const int s1 = kslots & 31, s2 = (kslots >> 5) & 31;
            const float *p2 = lvbuf + 6 * s2, *p1 = lvbuf + 6 * s1;
            const v3 A = mk3(p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]), W = mk3(p2[3] - p1[3], p2[4] - p1[4], p2[5] - p1[5]);
            const v3 V = A + cross(W, mk3(q0.x, q0.y, q0.z));
            const int dim = (int)q3.w;
            const v3 nn = mk3(q1.x, q1.y, q1.z), t1 = mk3(q2.x, q2.y, q2.z), t2 = mk3(q3.x, q3.y, q3.z);
            jv[0] = dot(nn, V);
            jv[1] = dim > 1 ? dot(t1, V) : 0.f; jv[2] = dim > 1 ? dot(t2, V) : 0.f;
            jv[3] = dim > 3 ? dot(nn, W) : 0.f;
            jv[4] = dim > 4 ? dot(t1, W) : 0.f; jv[5] = dim > 4 ? dot(t2, W) : 0.f;
        }
    };
    auto jmul_contacts = [&](float vc, float *out) {
        // the next contact's record is fetched while the six reductions of the current one run
        float4 q0 = lds4(con), q1 = lds4(con + 4), q2 = lds4(con + 8), q3 = lds4(con + 12);
        for (int ci = 0; ci < ncon; ci++) {
            const float *nx = con + C2_SIZE * (ci + 1 < ncon ? ci + 1 : ci);
            const float4 n0 = lds4(nx), n1 = lds4(nx + 4), n2 = lds4(nx + 8), n3 = lds4(nx + 12);
            const int m1 = __float_as_int(q0.w), m2 = __float_as_int(q1.w);
            const float sg = (float)(((m2 >> c) & 1) - ((m1 >> c) & 1)) * vc;
            const v3 pos = mk3(q0.x, q0.y, q0.z);
            const v3 P = (l_c + cross(a_c, pos - n_c)) * sg, Q = a_c * sg;
            const float Vx = gsum<G>(P.x), Vy = gsum<G>(P.y), Vz = gsum<G>(P.z);
            const float Wx = gsum<G>(Q.x), Wy = gsum<G>(Q.y), Wz = gsum<G>(Q.z);
            const int adr = (int)q2.w, dim = (int)q3.w;
            if (c < dim) {
                const int jj = c % 3;
                const v3 ax = jj == 0 ? mk3(q1.x, q1.y, q1.z) : (jj == 1 ? mk3(q2.x, q2.y, q2.z) : mk3(q3.x, q3.y, q3.z));
                out[adr + c] = c < 3 ? (ax.x * Vx + ax.y * Vy + ax.z * Vz) : (ax.x * Wx + ax.y * Wy + ax.z * Wz);
            }
            q0 = n0; q1 = n1; q2 = n2; q3 = n3;
        }
    };
    const bool by_links = !hook_jv_per_contact && __popc(lmask) < lvcap;          // one slot is the world's          // per env (never a property of its wave neighbours: results must not depend on them)
    auto jmul = [&](float vc, float (&jv)[6]) {
        if (by_links) jmul_links(vc, jv);
        else {          // rare (more distinct links than the scratch holds): per contact through the J v rows in LDS, read back by the contact lane
            jmul_contacts(vc, rJv);
            wave_sync();
#pragma unroll
            for (int j = 0; j < 6; j++) jv[j] = 0.f;
            if (c < ncon) {
                const float *cr = con + C2_SIZE * c;
                const int adr = (int)cr[C2_ADR], dim = (int)cr[C2_DIM];
#pragma unroll
                for (int j = 0; j < 6; j++) { const float t = rJv[adr + j]; jv[j] = j < dim ? t : 0.f; }
            }
            wave_sync();
        }
    };
    // The three products the setup needs - J qvel (reference acceleration), J qacc_smooth and J qacc_warmstart (warm-start choice) - in ONE
    // pass over the distinct links: three packed reduction trees per link side by side (independent chains), one barrier, one round of
    // reads per contact lane, instead of three passes.  Scratch: the rows of the reference acceleration / residual arrays, which live in
    // the contact lanes' registers since round 3 (3 x 6 lvcap <= 2 R floats).
    auto jmul3 = [&](float v0, float v1, float v2, float (&j0)[6], float (&j1)[6], float (&j2)[6]) {
        const int lvcap3 = (2 * R) / 18;          // link slots per vector when three share the scratch
        if (!by_links || __popc(lmask) >= lvcap3) { jmul(v0, j0); jmul(v1, j1); jmul(v2, j2); return; }
        float *lv3 = rAref;
        const int vs = 6 * lvcap3;
        if (c < 6) { lv3[c] = 0.f; lv3[vs + c] = 0.f; lv3[2 * vs + c] = 0.f; }
        int slot = 1;
        for (int mm = lmask; mm; mm &= mm - 1, slot++) {
            const int l = __ffs(mm) - 1;
            const bool on = LINK_MOVES_WITH_DOF(l);
            const float w0 = on ? v0 : 0.f, w1 = on ? v1 : 0.f, w2 = on ? v2 : 0.f;
            const float p0[6] = {b_c.x * w0, b_c.y * w0, b_c.z * w0, a_c.x * w0, a_c.y * w0, a_c.z * w0};
            const float p1[6] = {b_c.x * w1, b_c.y * w1, b_c.z * w1, a_c.x * w1, a_c.y * w1, a_c.z * w1};
            const float p2[6] = {b_c.x * w2, b_c.y * w2, b_c.z * w2, a_c.x * w2, a_c.y * w2, a_c.z * w2};
            const float r0 = gsum6_packed<G>(p0, c), r1 = gsum6_packed<G>(p1, c), r2 = gsum6_packed<G>(p2, c);
            const int q = gsum6_index(c);
            if (c < 16 && (c & 1) == 0 && q < 6) { lv3[6 * slot + q] = r0; lv3[vs + 6 * slot + q] = r1; lv3[2 * vs + 6 * slot + q] = r2; }
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < 6; j++) { j0[j] = 0.f; j1[j] = 0.f; j2[j] = 0.f; }
        if (c < ncon) {
            const float *cr = con + C2_SIZE * c;
            const float4 q0 = lds4(cr), q1 = lds4(cr + 4), q2 = lds4(cr + 8), q3 = lds4(cr + 12);
            const int s1 = kslots & 31, s2 = (kslots >> 5) & 31;
            const int dim = (int)q3.w;
            const v3 pos = mk3(q0.x, q0.y, q0.z), nn = mk3(q1.x, q1.y, q1.z), t1 = mk3(q2.x, q2.y, q2.z), t2 = mk3(q3.x, q3.y, q3.z);
            auto rows = [&](const float *lv, float (&jv)[6]) {
                const float *p2_ = lv + 6 * s2, *p1_ = lv + 6 * s1;
                const v3 A = mk3(p2_[0] - p1_[0], p2_[1] - p1_[1], p2_[2] - p1_[2]), W = mk3(p2_[3] - p1_[3], p2_[4] - p1_[4], p2_[5] - p1_[5]);
                const v3 V = A + cross(W, pos);
                jv[0] = dot(nn, V);
                jv[1] = dim > 1 ? dot(t1, V) : 0.f; jv[2] = dim > 1 ? dot(t2, V) : 0.f;
                jv[3] = dim > 3 ? dot(nn, W) : 0.f;
                jv[4] = dim > 4 ? dot(t1, W) : 0.f; jv[5] = dim > 4 ? dot(t2, W) : 0.f;
            };
            rows(lv3, j0); rows(lv3 + vs, j1); rows(lv3 + 2 * vs, j2);
        }
        wave_sync();          // the scratch rows are free again
    };
    // lane c's entry of J^T (world wrench stored per contact in C2_FW / C2_TW) + its own limit rows
    auto jt_contact = [&](const float *cr) -> float {
        const float4 q0 = lds4(cr), fw = lds4(cr + C2_FW), tw = lds4(cr + C2_TW);
        const int m1 = __float_as_int(q0.w), m2 = __float_as_int(cr[C2_L2]);
        const float sg = (float)(((m2 >> c) & 1) - ((m1 >> c) & 1));
        const v3 pos = mk3(q0.x, q0.y, q0.z);
        const v3 P = l_c + cross(a_c, pos - n_c);
        return sg * (P.x * fw.x + P.y * fw.y + P.z * fw.z + a_c.x * tw.x + a_c.y * tw.y + a_c.z * tw.z);
    };
    // The Jacobian entries of lane c's dof in the rows of the env's first KJ contacts: a contact's geometry is fixed for the substep, so the
    // entries are formed once (below, after the contact frames) and the Newton iterations - gradient and Hessian, five or six times
    // over in the envs that set the launch time - read them from registers instead of rebuilding them from the contact records
    // (lever arm, cross product, six dot products per contact and iteration).  16-lane groups only (G = 32 assembles per body).
    constexpr int KJ = (G == 16) ? 4 : 0;      // round 3: 3: 367k, 4: 381k, 6: 366k, 8: 355k env-steps/s on cfg3 (registers); round 6 (12 B of scratch): 4: 482k, 5: 484k, 6: 476k over 40 env-steps
    float Jc[KJ > 0 ? KJ : 1][6];
    // The row-space gradient g of contact lane c at the last evaluation stays in that lane's REGISTERS: the dof lanes fetch it for the first KJ
    // contacts with DPP broadcasts folded into the FMAs of J^T g (row_newbcast: lane ci of the env's row) - no LDS round trip (+3.3 %).
    // The same for the cone's Hessian terms was slower than reading them from LDS (a chain of 32 hand-written DPP-FMAs per contact that the
    // scheduler cannot interleave, and a matrix-core operand must not come straight out of inline asm: measured -3 %, removed).
    constexpr bool CZG = KJ > 0;
    float cz_g[6] = {0, 0, 0, 0, 0, 0};
    // REP (replicas of one env in the lane groups of a solo server): sum of a per-group partial result over the groups, identical in all
    auto xgroup_sum = [&](float v) -> float {
        if constexpr (G == 16) {
            const unsigned u = __builtin_bit_cast(unsigned, v);
            const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
            const float s1 = __builtin_bit_cast(float, (unsigned)a[0]) + __builtin_bit_cast(float, (unsigned)a[1]);
            const unsigned u2 = __builtin_bit_cast(unsigned, s1);
            const auto b2 = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
            return __builtin_bit_cast(float, (unsigned)b2[0]) + __builtin_bit_cast(float, (unsigned)b2[1]);
        } else {
            const unsigned u = __builtin_bit_cast(unsigned, v);
            const auto b2 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            return __builtin_bit_cast(float, (unsigned)b2[0]) + __builtin_bit_cast(float, (unsigned)b2[1]);
        }
    };
    auto jt_force = [&]() -> float {
        float acc = 0.f;
        if (lim_on[0]) acc += lim_gr[0];
        if (lim_on[1]) acc -= lim_gr[1];
        if constexpr (REP) {          // the contacts go round the replicas (every contact lane has left its world wrench), the parts are added up
            float part = 0.f;
            for (int ci = g; ci < ncon; ci += 64 / G) part += jt_contact(con + C2_SIZE * ci);
            acc += xgroup_sum(part);
            return isdof ? acc : 0.f;
        }
        // one accumulator per cached contact (four independent chains of six DPP-FMAs instead of one chain of twenty-four); cz_g was written by the
        // evaluation, far upstream; the first read of each cz_g[j] still carries the wait states of the VALU-write -> DPP-read hazard, like every run of fmac_bcast
        float accj[KJ > 0 ? KJ : 1];
        static_for<0, KJ>([&](auto cc) { accj[decltype(cc)::value] = 0.f; });
        if constexpr (CZG) {
            static_for<0, 6>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                static_for<0, KJ>([&](auto cc) { constexpr int ci = decltype(cc)::value; fmac_bcast<G, ci, ci == 0>(accj[ci], Jc[ci][j], bc_prepare<G>(cz_g[j])); });
            });
            if constexpr (KJ == 4) acc += (accj[0] + accj[1]) + (accj[2] + accj[3]);
            else static_for<0, KJ>([&](auto cc) { acc += accj[decltype(cc)::value]; });
        }
        static_for<0, KJ>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            if constexpr (CZG) {
            } else if (ci < ncon) {
                // the first KJ contact lanes leave their row-space gradient g[6] where the others leave their world wrench
                const float *cr = con + C2_SIZE * ci;
                const float4 ga = lds4(cr + C2_FW), gb = lds4(cr + C2_TW);
                acc += Jc[ci][0] * ga.x + Jc[ci][1] * ga.y + Jc[ci][2] * ga.z + Jc[ci][3] * gb.x + Jc[ci][4] * gb.y + Jc[ci][5] * gb.z;
            }
        });
        if constexpr (G == 32) { for (unsigned mk = relmask; mk; mk &= mk - 1) acc += jt_contact(con + C2_SIZE * (__ffs(mk) - 1)); }      // KJ = 0 there
        else { for (int ci = KJ; ci < ncon; ci++) acc += jt_contact(con + C2_SIZE * ci); }
        return isdof ? acc : 0.f;
    };

    // E5 reference acceleration of contact rows: aref = -B (J qvel) - K imp dist (row 0 only)
    float kAref[6] = {0, 0, 0, 0, 0, 0}, kx[6] = {0, 0, 0, 0, 0, 0};          // contact lane c: reference acceleration and residual J a - aref of its rows
    float jv_smooth[6], jv_warm[6];          // J qacc_smooth, J qacc_warmstart of contact lane c: consumed by the warm-start choice
    {
        float jv[6];
        jmul3(qvel_c, qas_c, warm_c, jv, jv_smooth, jv_warm);
        if (c < ncon) {
            const float *cr = con + C2_SIZE * c;
            const int dim = (int)cr[C2_DIM];
            const float Bc = cr[C2_B], kd = cr[C2_KD];
#pragma unroll
            for (int j = 0; j < 6; j++) kAref[j] = j < dim ? -Bc * jv[j] - (j == 0 ? kd : 0.f) : 0.f;
        }
    }
    wave_sync();
    PHASE_S(5, 29);

    if constexpr (!REP)
    static_for<0, KJ>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        const float *cr = con + C2_SIZE * ci;
        const float4 q0 = lds4(cr), q1 = lds4(cr + 4), q2 = lds4(cr + 8), q3 = lds4(cr + 12);
        const bool have = ci < ncon && isdof;
        const int m1 = __float_as_int(q0.w), m2 = __float_as_int(q1.w), dim = (int)q3.w;
        const float sg = (float)(((m2 >> c) & 1) - ((m1 >> c) & 1));
        const v3 P = (l_c + cross(a_c, mk3(q0.x, q0.y, q0.z) - n_c)) * sg, Q = a_c * sg;
        const v3 axs[3] = {mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z), mk3(q3.x, q3.y, q3.z)};
#pragma unroll
        for (int j = 0; j < 6; j++) { const float jc = j < 3 ? dot(axs[j % 3], P) : dot(axs[j % 3], Q); Jc[ci][j] = (have && j < dim) ? jc : 0.f; }
    });
    if constexpr (!REP && KJ > 0) {
        // records ncon .. KJ - 1 (contacts this env does not have, but a neighbour in the wave may): zero weights and cone vectors, so that the
        // select-free Hessian terms of hess_cached vanish (what lies there is left over from the kinematics: finite or not, nobody knows)
        if (c >= ncon && c < KJ) {
            float *cr = con + C2_SIZE * c;
            const float4 z4 = make_float4(0, 0, 0, 0);
            *reinterpret_cast<float4 *>(cr + C2_ZONE) = z4; *reinterpret_cast<float4 *>(cr + C2_FW) = z4; *reinterpret_cast<float4 *>(cr + C2_TW) = z4;
            *reinterpret_cast<float4 *>(cr + C2_GN) = z4; *reinterpret_cast<float4 *>(cr + C2_GN + 4) = z4; *reinterpret_cast<float4 *>(cr + C2_GN + 8) = z4;
        }
    }
    // contact lane c's own constants for the substep (row weights D, friction per row, cone mu, first row and dim): what the cost
    // evaluation and the line search of every iteration would otherwise fetch from LDS again
    PHASE_S(5, 30);
    float kD[6] = {0, 0, 0, 0, 0, 0}, kfri[5] = {0, 0, 0, 0, 0}, kmu = 0;
    int kadr = 0, kdim = 0;
    if (c < ncon) {
        const float *cr = con + C2_SIZE * c;
        kadr = (int)cr[C2_ADR]; kdim = (int)cr[C2_DIM]; kmu = cr[C2_MU];
        const float f0 = cr[C2_F0], f2 = cr[C2_F2], f3 = cr[C2_F3];
        kfri[0] = kdim > 1 ? f0 : 0.f; kfri[1] = kdim > 2 ? f0 : 0.f; kfri[2] = kdim > 3 ? f2 : 0.f; kfri[3] = kdim > 4 ? f3 : 0.f; kfri[4] = kdim > 5 ? f3 : 0.f;
#pragma unroll
        for (int j = 0; j < 6; j++) { const float t = rD[kadr + j]; kD[j] = j < kdim ? t : 0.f; }
    }
    PHASE(5);
    // ---------------- phase F: Newton solver (a-2.6)
    const float tol = m.tolerance, scale = 1.0f / (m.meaninertia * (nv > 1 ? nv : 1));
    float cost = 0, Ma_c = 0;
    bool zones_changed = true, zones_flipped = true;      // since the last evaluation: not purely quadratic / an active set changed
    // cost at acceleration a (one register per lane); leaves Ma_c, jar, gr, dw, zones and contact wrenches behind
    // inc (workgroup-uniform): ac is the previous point plus ls_alpha * search, so M a and the row residuals are advanced
    // with the products M search (ls_mv) and J search (rJv) that the line search already formed, as mj_solNewton does
    float ls_mv = 0, ls_alpha = 0, ls_jv[6] = {0, 0, 0, 0, 0, 0};          // ls_jv: J search of lane c's contact, from the line search to the evaluation after it
    // the six rows of contact lane c out of a row array, zero beyond its dim: unconditional reads (what lies behind a short contact's rows
    // is the next contact's or the padding - read, not used) and selects instead of six branches; likewise its friction coefficients
    auto cone_rows = [&](const float *arr, int adr, int dim, float (&o)[6]) {
#pragma unroll
        for (int j = 0; j < 6; j++) { const float t = arr[adr + j]; o[j] = j < dim ? t : 0.f; }
    };
    auto cone_fri = [&](const float *cr, int dim, float (&f)[5]) {
        const float f0 = cr[C2_F0], f2 = cr[C2_F2], f3 = cr[C2_F3];
        f[0] = dim > 1 ? f0 : 0.f; f[1] = dim > 2 ? f0 : 0.f; f[2] = dim > 3 ? f2 : 0.f; f[3] = dim > 4 ? f3 : 0.f; f[4] = dim > 5 ? f3 : 0.f;
    };
    // rows j < dim of contact lane c into a row array: dim is 1, 3, 4 or 6 - three tests, not six
    auto store_rows = [&](float *arr, int adr, int dim, const float (&v)[6]) {
        arr[adr] = v[0];
        if (dim > 1) { arr[adr + 1] = v[1]; arr[adr + 2] = v[2]; }
        if (dim > 3) arr[adr + 3] = v[3];
        if (dim > 4) { arr[adr + 4] = v[4]; arr[adr + 5] = v[5]; }
    };
    bool kx_ready = false;          // the row residuals of contact lane c at the point to be evaluated are already in kx (warm-start choice below)
    auto eval_at = [&](float ac, bool inc) -> float {
        float unstable = 0.f;
        if (!inc) {
            float ma = 0;
            const BcSrc<G> bac = bc_prepare<G>(ac);
            static_for<0, NK>([&](auto kc) { constexpr int k = decltype(kc)::value; fmac_bcast<G, k, bc_first<G, k, 0>()>(ma, Mrow[k], bac); });
            Ma_c = isdof ? ma : 0.f;
        } else if (isdof) Ma_c += ls_alpha * ls_mv;
        float part = isdof ? 0.5f * (ac - qas_c) * (Ma_c - qfs_c) : 0.f;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            if (lim_on[side]) {
                const float x = (side == 0 ? ac : -ac) - lim_aref[side];
                const bool was = lim_dw[side] != 0.f;
                if (x < 0) { part += 0.5f * lim_D[side] * x * x; lim_gr[side] = lim_D[side] * x; lim_dw[side] = lim_D[side]; unstable += was ? 0.f : 1024.f; }
                else { lim_gr[side] = 0; lim_dw[side] = 0; unstable += was ? 1024.f : 0.f; }
            }
        }
        if (!inc) {
            if (!kx_ready) {          // workgroup-uniform
                float jv[6];
                jmul(ac, jv);
#pragma unroll
                for (int j = 0; j < 6; j++) kx[j] = jv[j] - kAref[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 6; j++) kx[j] += ls_alpha * ls_jv[j];
        }
        if (c < ncon) {
            float *cr = con + C2_SIZE * c;
            const int adr = kadr, dim = kdim;
            const float (&D)[6] = kD; const float (&fri)[5] = kfri; const float (&x)[6] = kx;
            ConeOut o;
            cone_eval2(dim, kmu, fri, D, x, o);
            part += o.cost;
            if ((int)cr[C2_ZONE] != o.zone) unstable += 1024.f;          // a flip counts 1024, a contact in the (non-quadratic) middle zone 1
            else if (o.zone == 2) unstable += 1.f;
            cr[C2_ZONE] = (float)o.zone;
            cr[C2_DM] = o.Dm; cr[C2_K3] = o.k3;
            if constexpr (CZG) {
#pragma unroll
                for (int j = 0; j < 6; j++) cz_g[j] = o.g[j];
            }
            auto world_wrench = [&]() {
                const v3 nn = mk3(cr[C2_N], cr[C2_N + 1], cr[C2_N + 2]), t1 = mk3(cr[C2_T1], cr[C2_T1 + 1], cr[C2_T1 + 2]), t2 = mk3(cr[C2_T2], cr[C2_T2 + 1], cr[C2_T2 + 2]);
                const v3 fw = nn * o.g[0] + t1 * o.g[1] + t2 * o.g[2], tw = nn * o.g[3] + t1 * o.g[4] + t2 * o.g[5];
                cr[C2_FW] = fw.x; cr[C2_FW + 1] = fw.y; cr[C2_FW + 2] = fw.z; cr[C2_TW] = tw.x; cr[C2_TW + 1] = tw.y; cr[C2_TW + 2] = tw.z;
            };
            if constexpr (!REP && CZG) {          // jt_force reads g out of this lane's registers; the wrench slots carry the row weights for hess_cached
                // stored by EVERY contact lane, out of the registers the selects left them in, and overwritten by the lanes c >= KJ: one store for both kinds of
                // lane behind the branch had the weights and the wrench merged into a third set of registers first (six copies per evaluation)
                cr[C2_FW] = o.dw[0]; cr[C2_FW + 1] = o.dw[1]; cr[C2_FW + 2] = o.dw[2]; cr[C2_TW] = o.dw[3]; cr[C2_TW + 1] = o.dw[4]; cr[C2_TW + 2] = o.dw[5];
                if (c >= KJ) world_wrench();
            } else if (!REP && c < KJ) {          // read back through the cached Jacobian entries (jt_force)
                cr[C2_FW] = o.g[0]; cr[C2_FW + 1] = o.g[1]; cr[C2_FW + 2] = o.g[2]; cr[C2_TW] = o.g[3]; cr[C2_TW + 1] = o.g[4]; cr[C2_TW + 2] = o.g[5];
            } else world_wrench();
#pragma unroll
            for (int j = 0; j < 6; j++) { cr[C2_GN + j] = o.gn[j]; cr[C2_U + j] = o.u[j]; }
            if (REP || !(CZG && c < KJ)) store_rows(rDw, adr, dim, o.dw);
        }
        float tot, unst;
        gsum2<G>(part, unstable, tot, unst);
        zones_changed = unst > 0.f; zones_flipped = unst >= 1024.f;
        wave_sync();
        return tot;
    };

    // constraint cost at qacc_smooth (its Gauss term is zero) for the warm-start choice: no solver state is touched,
    // J qacc_smooth goes to the J v rows, which are free between the reference acceleration and the first line search
    float xs_smooth[6] = {0, 0, 0, 0, 0, 0};       // J qacc_smooth - aref of contact lane c: reused if the env starts from qacc_smooth
    auto cost_smooth = [&]() -> float {
        float part = 0.f;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            if (lim_on[side]) {
                const float x = (side == 0 ? qas_c : -qas_c) - lim_aref[side];
                if (x < 0) part += 0.5f * lim_D[side] * x * x;
            }
        }
        float x[6];
#pragma unroll
        for (int j = 0; j < 6; j++) { x[j] = jv_smooth[j] - kAref[j]; xs_smooth[j] = x[j]; }
        if (c < ncon) part += cone_cost(kdim, kmu, kfri, kD, x);
        const float tot = gsum<G>(part);
        wave_sync();
        return tot;
    };

#if !defined(HSR_ZSTAT) && !defined(HSR_LSCOUNT) && !defined(HSR_F0COUNT) && !defined(HSR_CPLSTAT) && !defined(HSR_NOSTEPCOUNT) && !defined(HSR_ACTSTAT)
    DBGCNT(3, nefc);
#endif
    bool active = valid && nefc > 0;
    int iter = 0;
    float qacc_c;
    {
        const float cost_s = cost_smooth();
        PHASE_S(6, 26);
#pragma unroll
        for (int j = 0; j < 6; j++) kx[j] = jv_warm[j] - kAref[j];
        kx_ready = true;
        const float cost_w = eval_at(warm_c, false);
        kx_ready = false;
        PHASE_S(6, 27);
        const bool use_warm = cost_w < cost_s;
        qacc_c = use_warm ? warm_c : qas_c;
        cost = use_warm ? cost_w : cost_s;
        if (wave_any(active && !use_warm)) {          // (an env that will not iterate - finished, or without constraints - takes qacc_smooth below whatever is rebuilt here)
#ifdef HSR_F0COUNT
            DBGCNT(3, 1ull);
#endif
            // some env of the wave starts from qacc_smooth: the state (zones, forces, M a) is rebuilt at the chosen point - its row residuals
            // exist already (from the evaluation at the warm start, or from cost_smooth), the J v pass is not repeated
#pragma unroll
            for (int j = 0; j < 6; j++) kx[j] = use_warm ? kx[j] : xs_smooth[j];
            kx_ready = true;
            cost = eval_at(qacc_c, false);
            kx_ready = false;
        }
    }
    PHASE(6);
    int newton_trips = 0;          // workgroup-uniform
    for (int it = 0; it < m.iterations; it++) {
        if (!wave_any(active)) break;
        newton_trips++;
        DBGCNT(0, 1);
#ifdef HSR_ACTSTAT
        // diagnostic (timing build; tools/block_times.py with HSR_ACTSTAT=1): counter 3 = Newton trips of the wave by the number of its envs that are still iterating: 1 | 2 << 21 | 3-4 << 42
        { const int na_ = __popcll(__ballot(active && c == 0)); DBGCNT(3, na_ <= 1 ? 1ull : (na_ == 2 ? (1ull << 21) : (1ull << 42))); }
#endif
        const float jtf = jt_force();
        const float grad_c = isdof ? Ma_c - qfs_c + jtf : 0.f;
        const float gnorm = fsqrt(gsum<G>(grad_c * grad_c));
        if (scale * gnorm < tol) active = false;
        PHASE(7);
        // Hessian rows H = M + J^T (d2s) J, lane = row c of H
        float Hrow[G];
        constexpr bool HESS_MFMA = G == 16;
        // G = 16: the rank-1 terms w z z^T of the four envs of the wave are ONE v_mfma_f32_16x16x1 (4 blocks of 16x16, K = 1: block = lane
        // group = env, A = z and B = w z straight from the lanes that hold them - no broadcasts), accumulated in 16 registers in the
        // matrix core's layout and brought into the row layout once per Hessian (build_H); 13 DPP-FMAs per term before
        HessAcc hacc;
        constexpr bool HESS_MFMA32 = G == 32;
        HessAcc32 hacc32;       // G = 32: the same with v_mfma_f32_32x32x1 (2 blocks = the two envs of the wave), for the contacts that couple bodies
        auto emit8 = [&](float (&acc)[G], const float (&z)[8], const float (&w)[8], const float (&gn)[6], const float (&uu)[6]) {
            if constexpr (HESS_MFMA32) {
                const float s6 = w[6] * z[6], s7 = w[7] * z[7];
#pragma unroll
                for (int r = 0; r < 6; r++) hacc32.v = __builtin_amdgcn_mfma_f32_32x32x1f32(z[r], w[r] * z[r] + s6 * gn[r] + s7 * uu[r], hacc32.v, 0, 0, 0);
            } else if constexpr (HESS_MFMA) {
                // J^T C J with C = diag(w) + w6 gn gn^T + w7 u u^T as six products z_r (C z)_r^T: the two cone terms ride in the B operand
                const float s6 = w[6] * z[6], s7 = w[7] * z[7];
#pragma unroll
                for (int r = 0; r < 6; r++) hacc.v = __builtin_amdgcn_mfma_f32_16x16x1f32(z[r], w[r] * z[r] + s6 * gn[r] + s7 * uu[r], hacc.v, 0, 0, 0);
            } else {
                static_for<0, 8>([&](auto rc) {
                    constexpr int r = decltype(rc)::value;
                    const float t = w[r] * z[r];
                    const BcSrc<G> bz = bc_prepare<G>(z[r]);
                    static_for<0, NK>([&](auto kc) { constexpr int k = decltype(kc)::value; fmac_bcast<G, k, bc_first<G, k, 0>()>(acc[k], t, bz); });
                });
            }
        };
        // contribution of one contact (record cr, row weights in dwp) to row c of the Hessian
        // contact CI < KJ: the same eight terms from the cached Jacobian entries (what is left to read: zone, cone vectors, row weights)
        auto hess_cached = [&](float (&acc)[G], auto cc, bool with_neg) {
            constexpr int CI = decltype(cc)::value;
            static_assert(CZG, "the select-free terms below read the row weights out of the record (C2_FW / C2_TW), where only the CZG evaluation leaves them");
            const float *cr = con + C2_SIZE * CI;
            const float4 q5 = lds4(cr + C2_ZONE);
            const float4 ga = lds4(cr + 32), gb = lds4(cr + 36), gc = lds4(cr + 40);
            const float4 wa = lds4(cr + C2_FW), wb = lds4(cr + C2_TW);          // the row weights sit in the record itself (two wide reads, no row address to form)
            const float wj[6] = {wa.x, wa.y, wa.z, wb.x, wb.y, wb.z};
            const float gn[6] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y}, uu[6] = {gb.z, gb.w, gc.x, gc.y, gc.z, gc.w};
            float z[8], w[8];
            float pc = 0.f, wc = 0.f;
            // No selects: every term that does not exist carries a zero weight by construction - the evaluation leaves dw = Dm = k3 = 0 in the top zone and
            // Dm = k3 = 0 in the bottom zone, rows beyond a contact's dim have zero weights and zero Jacobian entries, the cached Jacobian of a contact the
            // env does not have is zero and its record's weights are cleared once per substep (below, after the cache is filled); an env that has left the
            // Newton loop assembles a Hessian nobody reads.  Same arithmetic for every term that exists: results are bit-identical.
#pragma unroll
            for (int j = 0; j < 6; j++) { z[j] = Jc[CI > KJ - 1 ? 0 : CI][j]; pc += z[j] * gn[j]; wc += z[j] * uu[j]; w[j] = wj[j]; }
            z[6] = pc; w[6] = q5.y;
            z[7] = wc; w[7] = with_neg ? -q5.z : 0.f;
            emit8(acc, z, w, gn, uu);
        };
        // Branch-free: the eight rank-1 terms of a contact (its <= 6 rows, then the two cone terms of the middle zone) are ALWAYS
        // issued, with weight 0 where a term does not exist (row beyond dim, zero row weight, zone 0 / 1, lane group that has no
        // contact ci) - eight straight runs of NK v_fmac_f32_dpp instead of seventeen exec-mask branches around them (the branches
        // cost more than the FMAs they skipped: 2.1 k cycles per contact of which the 104 FMAs were a third).  `live` = this lane's
        // env has a contact ci; a dead lane reads record 0 of its env (finite values, weights forced to 0).
        auto hess_contact = [&](float (&acc)[G], int ci, const float *dwp, bool with_neg, bool env_on) {
            const bool live = env_on && ci < ncon;
            const int cj = live ? ci : 0;
            const float *cr = con + C2_SIZE * cj;
            const unsigned below = (1u << cj) - 1u;
            const int adr = nlim + cj + 2 * __popc(dim_lo & below) + 3 * __popc(dim_hi & below);
            const int dim = 1 + 2 * (int)((dim_lo >> cj) & 1u) + 3 * (int)((dim_hi >> cj) & 1u);
            const float4 q5 = lds4(cr + C2_ZONE);
            const float4 q0 = lds4(cr), q1 = lds4(cr + 4), q2 = lds4(cr + 8), q3 = lds4(cr + 12);
            const float4 ga = lds4(cr + 32), gb = lds4(cr + 36), gc = lds4(cr + 40);
            float wj[6];
#pragma unroll
            for (int j = 0; j < 6; j++) wj[j] = dwp[adr + j];
            const int zone = (int)q5.x;
            const bool on = live && zone != 0 && isdof;
            const int m1 = __float_as_int(q0.w), m2 = __float_as_int(q1.w);
            const float gn[6] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y}, uu[6] = {gb.z, gb.w, gc.x, gc.y, gc.z, gc.w};
            const float sg = (float)(((m2 >> c) & 1) - ((m1 >> c) & 1));
            const v3 pos = mk3(q0.x, q0.y, q0.z);
            const v3 P = (l_c + cross(a_c, pos - n_c)) * sg, Q = a_c * sg;
            const v3 axs[3] = {mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z), mk3(q3.x, q3.y, q3.z)};
            float z[8], w[8];
            float pc = 0.f, wc = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const float jc = j < 3 ? dot(axs[j % 3], P) : dot(axs[j % 3], Q);
                const bool rowon = on && j < dim;
                z[j] = rowon ? jc : 0.f;
                pc += z[j] * gn[j]; wc += z[j] * uu[j];
                w[j] = rowon ? wj[j] : 0.f;
            }
            const bool mid = on && zone == 2;
            z[6] = mid ? pc : 0.f; w[6] = mid ? q5.y : 0.f;
            z[7] = mid ? wc : 0.f; w[7] = (mid && with_neg) ? -q5.z : 0.f;
            emit8(acc, z, w, gn, uu);
        };
        // World <-> free-body contacts, per body: with x_j = (ax_j, r x ax_j) (rows 0-2) or (0, ax_j) (rows 3-5), r from the body's
        // reference point o, row j of the contact Jacobian is x_j . s_k for the body's dof k with the spatial velocity s_k = (v_k(o), w_k),
        // so the body's diagonal block of J^T W J is S^T K S with K = sum over its contacts of X W X^T (6 x 6, symmetric):
        // lane = contact builds its K and adds the 21 entries into the body's LDS accumulator, lane = dof forms K s and the six
        // lanes of the body exchange those vectors.  Cost per iteration: one pass, whatever the number of such contacts.
        auto body_hess = [&](float (&acc)[G], bool with_neg) {
            if (my_fb >= 0) *reinterpret_cast<float4 *>(fbK + 28 * my_fb + 4 * my_kk) = make_float4(0, 0, 0, 0);
            wave_sync();
            if ((fbmask >> c) & 1) {
                const float *cr = con + C2_SIZE * c;
                const float4 q5 = lds4(cr + C2_ZONE);
                const int zone = (int)q5.x;
                if (zone != 0) {
                    const float4 q0 = lds4(cr), q1 = lds4(cr + 4), q2 = lds4(cr + 8), q3 = lds4(cr + 12);
                    const float4 ga = lds4(cr + 32), gb = lds4(cr + 36), gc = lds4(cr + 40);
                    const int adr = (int)q2.w, dim = (int)q3.w;
                    float *K = fbK + 28 * (((int)cr[C2_PAIR] >> 10) - 1);
                    const v3 r = mk3(q0.x - K[24], q0.y - K[25], q0.z - K[26]);
                    const v3 axs[3] = {mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z), mk3(q3.x, q3.y, q3.z)};
                    const float gn[6] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y}, uu[6] = {gb.z, gb.w, gc.x, gc.y, gc.z, gc.w};
                    float kk[21], pv[6] = {0, 0, 0, 0, 0, 0}, qv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < 21; i++) kk[i] = 0.f;
                    // kk += w x x^T, upper triangle row by row: (0,0) (0,1) .. (0,5) (1,1) ..
                    auto rank1 = [&](float w, const float (&x)[6]) {
                        int idx = 0;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            const float t = w * x[a];
#pragma unroll
                            for (int b = a; b < 6; b++) kk[idx++] += t * x[b];
                        }
                    };
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        if (j < dim) {
                            const v3 mo = cross(r, axs[j]);
                            const float x[6] = {axs[j].x, axs[j].y, axs[j].z, mo.x, mo.y, mo.z};
                            const float w = rDw[adr + j];
                            if (w != 0.f) rank1(w, x);
#pragma unroll
                            for (int a = 0; a < 6; a++) { pv[a] += gn[j] * x[a]; qv[a] += uu[j] * x[a]; }
                        }
                    }
                    if (dim > 3) {
#pragma unroll
                        for (int j = 3; j < 6; j++) {
                            if (j < dim) {
                                const float x[6] = {0.f, 0.f, 0.f, axs[j - 3].x, axs[j - 3].y, axs[j - 3].z};
                                const float w = rDw[adr + j];
                                if (w != 0.f) rank1(w, x);
#pragma unroll
                                for (int a = 3; a < 6; a++) { pv[a] += gn[j] * x[a]; qv[a] += uu[j] * x[a]; }
                            }
                        }
                    }
                    if (zone == 2) {
                        rank1(q5.y, pv);
                        if (with_neg) rank1(-q5.z, qv);
                    }
#pragma unroll
                    for (int i = 0; i < 21; i++) __hip_atomic_fetch_add(K + i, kk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                }
            }
            wave_sync();
            float sv[6] = {0, 0, 0, 0, 0, 0}, y[6] = {0, 0, 0, 0, 0, 0};
            if (my_fb >= 0) {
                const float *K = fbK + 28 * my_fb;
                const float4 k0 = lds4(K), k1 = lds4(K + 4), k2 = lds4(K + 8), k3 = lds4(K + 12), k4 = lds4(K + 16), k5 = lds4(K + 20), k6 = lds4(K + 24);
                const float kf[21] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y, k2.z, k2.w, k3.x, k3.y, k3.z, k3.w, k4.x, k4.y, k4.z, k4.w, k5.x};
                const v3 vo = l_c + cross(a_c, mk3(k6.x, k6.y, k6.z) - n_c);
                sv[0] = vo.x; sv[1] = vo.y; sv[2] = vo.z; sv[3] = a_c.x; sv[4] = a_c.y; sv[5] = a_c.z;
                int idx = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int b = a; b < 6; b++) { y[a] += kf[idx] * sv[b]; if (b != a) y[b] += kf[idx] * sv[a]; idx++; }
                }
            }
            BcSrc<G> by[6];
#pragma unroll
            for (int i = 0; i < 6; i++) by[i] = bc_prepare<G>(y[i]);
            // H[c][k] += s_c . (K s_k) for the dofs k of lane c's own body: body b's columns are the static tile NK - 6 (nfb - b) ...
            static_for<0, NK / 6>([&](auto tc) {
                constexpr int T = decltype(tc)::value, LO = NK - 6 * (T + 1);
                if (T < nfb) {                                                                       // workgroup-uniform
                    const bool mine = my_fb == nfb - 1 - T;
                    float ts[6];
#pragma unroll
                    for (int i = 0; i < 6; i++) ts[i] = mine ? sv[i] : 0.f;
                    static_for<LO, LO + 6>([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        static_for<0, 6>([&](auto ic) { constexpr int i = decltype(ic)::value; fmac_bcast<G, k, k == LO>(acc[k], ts[i], by[i]); });
                    });
                }
            });
        };
        auto build_H = [&](bool with_neg) {
#pragma unroll
            for (int k = 0; k < NK; k++) Hrow[k] = Mrow[k];
            if constexpr (G == 16) {
                // G = 16 has no per-body assembly: every contact takes the per-contact path.  Wave-uniform trip count (the largest
                // contact count among the envs of the wave that are still iterating): a scalar loop, no exec masks; a lane group with
                // fewer contacts, or one that has left the Newton loop, adds zeros
                const float dl = active ? (lim_on[0] ? lim_dw[0] : 0.f) + (lim_on[1] ? lim_dw[1] : 0.f) : 0.f;
#pragma unroll
                for (int k = 0; k < NK; k++) Hrow[k] += (k == c) ? dl : 0.f;
                if constexpr (REP) {
                    // replicas: contact base + g in lane group g - one pass of the matrix core per EPB contacts; then the blocks are added
                    if (active && ncon > 0) {          // wave-uniform: every group holds the same env
                        hacc.clear();
                        float part[G];
#pragma unroll
                        for (int k = 0; k < NK; k++) part[k] = 0.f;
                        for (int base = 0; base < ncon; base += 64 / G) hess_contact(part, base + g, rDw, with_neg, true);
                        if constexpr (HESS_MFMA) hacc.template add_rows<NK>(part);
#pragma unroll
                        for (int k = 0; k < NK; k++) Hrow[k] += xgroup_sum(part[k]);
                    }
                } else {
                const int ncw = wave_max_groups<G>(active ? ncon : 0);
                hacc.clear();
                PHASE_S(7, 26);
#ifdef HSR_ZSTAT
                { const int zc = (c < ncon) ? (int)con[C2_SIZE * c + C2_ZONE] : -1;
                  dc_[3] += (unsigned long long)ncw | ((unsigned long long)__popcll(__ballot(active && zc == 1)) << 20) | ((unsigned long long)__popcll(__ballot(active && zc == 2)) << 40); }
#endif
                // contact 0 is not behind `0 < ncw`: the chain's first matrix-core product then takes the cleared accumulator as a literal zero, where sixteen
                // zeroed registers were merged with the chain's result across that test (16 copies per Hessian).  A wave without contacts (ncw = 0) adds
                // record 0 with zero weights - or whatever it holds - into an accumulator that nothing reads: add_rows below keeps its test
                if constexpr (KJ > 0) hess_cached(Hrow, std::integral_constant<int, 0>{}, with_neg);
                static_for<(KJ > 0 ? 1 : 0), KJ>([&](auto cc) { if (decltype(cc)::value < ncw) hess_cached(Hrow, cc, with_neg); });
                PHASE_S(7, 27);
                for (int ci = KJ; ci < ncw; ci++) hess_contact(Hrow, ci, rDw, with_neg, active);
                PHASE_S(7, 28);
                if constexpr (HESS_MFMA) { if (ncw > 0) hacc.template add_rows<NK>(Hrow); }
                PHASE_S(7, 29);
                }
            } else
            if constexpr (HESS_MFMA32) {
                // the contacts that couple bodies (robot <-> block, block <-> block), over the union of the two envs' sets: wave-uniform
                // loop, a lane group without the contact (or out of the Newton loop) adds zeros; the matrix core ignores no lane
                const unsigned wm = (unsigned)wave_or_groups<G>(active ? (int)dmask : 0);
                if (wm) {
                    hacc32.clear();
                    for (unsigned mk = wm; mk; mk &= mk - 1) { const int ci = __ffs(mk) - 1; hess_contact(Hrow, ci, rDw, with_neg, active && ((dmask >> ci) & 1u)); }
                    hacc32.template add_rows<NK>(Hrow);
                }
                if (active) {
                    const float dl = (lim_on[0] ? lim_dw[0] : 0.f) + (lim_on[1] ? lim_dw[1] : 0.f);
#pragma unroll
                    for (int k = 0; k < NK; k++) Hrow[k] += (k == c) ? dl : 0.f;
                    if (fbmask) body_hess(Hrow, with_neg);
                }
            } else
            if (active) {
                const float dl = (lim_on[0] ? lim_dw[0] : 0.f) + (lim_on[1] ? lim_dw[1] : 0.f);
#pragma unroll
                for (int k = 0; k < NK; k++) Hrow[k] += (k == c) ? dl : 0.f;
                { for (unsigned mk = dmask; mk; mk &= mk - 1) hess_contact(Hrow, __ffs(mk) - 1, rDw, with_neg, true); }
                if (fbmask) body_hess(Hrow, with_neg);
            }
            if (!isdof) {
#pragma unroll
                for (int k = 0; k < NK; k++) Hrow[k] = (k == c) ? 1.f : 0.f;
            }
        };
        build_H(true);
        PHASE(8);
        float hinvd, hy;
        auto factor = [&]() -> bool {
            if constexpr (SPARSE_CHOL) return chol_sparse_fwd<G, NK, (NDK > 0 ? NDK : 1)>(Hrow, hinvd, c, -grad_c, hy, my_fb, my_kk, sparse_ok);
            else return chol_g_fwd<G, NK>(Hrow, hinvd, nv, c, -grad_c, hy);
        };
        bool hfail = (!factor() || hook_majorant) && active;
        const bool majorant = hfail;          // this env's Hessian is replaced by its PSD majorant below
        if (wave_any(hfail)) {
            build_H(!hfail);
            hfail = !factor() && active;
            if (hfail) active = false;
        }
        auto back = [&]() -> float {
            if constexpr (SPARSE_CHOL) return chol_sparse_back<G, NK, (NDK > 0 ? NDK : 1)>(Hrow, hinvd, hy, c, sparse_ok);
            else return chol_back_mf<G, NK>(Hrow, hinvd, hy, nv, c);
        };
        float search_c = back();
        if (!isdof || !active) search_c = 0;       // an env that just dropped out (no usable factor) must not feed NaN into the shared products below
        // The decrement test, as soon as the direction exists (round 6): phi'(0) = grad . search, and with the exact Hessian phi''(0) = -phi'(0).  An env whose
        // scaled decrement is below the tolerance is finished BEFORE M search, J search and the evaluation are formed for it - and when that ends the last env of
        // the wave, the iteration ends here (the verification pass of a hard env paid 3 k cycles for products nobody used).  Same test, same operands as below.
        const float dp_exact = gsum<G>(grad_c * search_c);
        if (active && !majorant && (dp_exact >= 0 || scale * 0.5f * (-dp_exact) < tol)) active = false;
        if (!wave_any(active)) break;
        PHASE(9);
        // exact line search (safeguarded 1-D Newton on phi')
        float mv = 0;
        const BcSrc<G> bs_ = bc_prepare<G>(search_c);
        static_for<0, NK>([&](auto kc) { constexpr int k = decltype(kc)::value; fmac_bcast<G, k, bc_first<G, k, 0>()>(mv, Mrow[k], bs_); });
        float g1, g2, snorm2;
        gsum3<G>(search_c * (Ma_c - qfs_c), isdof ? search_c * mv : 0.f, search_c * search_c, g1, g2, snorm2);
        const float snorm = fsqrt(snorm2);
        PHASE(13);
        jmul(search_c, ls_jv);
        PHASE(25);
        float alpha = 0;
        bool last_step = false;         // the predicted decrease of this step is so small that the step after it cannot matter
        if (active) {
            // what the cone of contact lane c needs along the search line x(al) = x + al v, reduced once per iteration to the parts that
            // are linear or constant in al (cone_dd's formulas, regrouped): U_j(al) = f_j x_j + al f_j v_j for the friction rows,
            // N(al) = mu (x_0 + al v_0), S2 = sum (f_j v_j)^2, and the bottom zone's quadratic d1 = Q1 + al Q2, d2 = Q2
            float Ux[5] = {0, 0, 0, 0, 0}, Uv[5] = {0, 0, 0, 0, 0}, N0 = 0, Nv = 0, S2 = 0, Q1 = 0, Q2 = 0, cDm = 0, cmu = 0;
            if (c < ncon) {
                const float (&cD)[6] = kD; const float (&cfri)[5] = kfri; const float (&cx)[6] = kx; const float (&cv)[6] = ls_jv;
                cmu = kmu;
                N0 = cx[0] * cmu; Nv = cv[0] * cmu;
                cDm = cD[0] * frcp(cmu * cmu * (1 + cmu * cmu));
#pragma unroll
                for (int j = 0; j < 5; j++) { Ux[j] = cx[j + 1] * cfri[j]; Uv[j] = cv[j + 1] * cfri[j]; S2 += Uv[j] * Uv[j]; }
#pragma unroll
                for (int j = 0; j < 6; j++) { const float dv = cD[j] * cv[j]; Q1 += dv * cx[j]; Q2 += dv * cv[j]; }
            }
            // limit rows of this dof lane: residual at alpha = 0 and slope
            float lx[2], lv[2];
#pragma unroll
            for (int side = 0; side < 2; side++) { lx[side] = (side == 0 ? qacc_c : -qacc_c) - lim_aref[side]; lv[side] = side == 0 ? search_c : -search_c; }
            auto ls_eval = [&](float al, float &dphi, float &ddphi) {
                // Branch-free: every arm is a handful of instructions, and an exec-mask branch around a handful of instructions costs more than they do
                // (round-3 rule) - twelve of them per evaluation before.  A lane without a limit row / contact carries zeros (lim_D, the cone's
                // precomputed terms), which put it into the top zone: no contribution.
                float dp = 0, hp = 0;
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const float x = lx[side] + al * lv[side];
                    const bool on = lim_on[side] & (x < 0);
                    dp += on ? lim_D[side] * x * lv[side] : 0.f; hp += on ? lim_D[side] * lv[side] * lv[side] : 0.f;
                }
                {
                    const float Nn = N0 + al * Nv;
                    float T2 = 0, S1 = 0;
#pragma unroll
                    for (int j = 0; j < 5; j++) { const float Uj = Ux[j] + al * Uv[j]; T2 += Uj * Uj; S1 += Uj * Uv[j]; }
                    const float T = fsqrt(T2);
                    const bool tz = T <= 0;
                    const bool top = (Nn >= cmu * T) | (tz & (Nn >= 0));
                    const bool bot = (cmu * Nn + T <= 0) | (tz & (Nn < 0));
                    const float NT = Nn - cmu * T, invT = frcp(T);          // (T = 0 is top or bottom: the infinities below are never selected)
                    const float kappa = -cDm * NT * cmu, gnv = Nv - cmu * invT * S1;
                    const float d1m = cDm * NT * gnv;
                    const float d2m = kappa * invT * S2 + cDm * gnv * gnv - (kappa * invT * frcp(T2)) * S1 * S1;
                    const float d1 = top ? 0.f : (bot ? Q1 + al * Q2 : d1m), d2 = top ? 0.f : (bot ? Q2 : d2m);
                    dp += d1; hp += d2;
                }
                float sdp, shp;
                gsum2<G>(dp, hp, sdp, shp);
                dphi = g1 + al * g2 + sdp;
                ddphi = g2 + shp;
            };
            const float gtol = tol * m.ls_tolerance * snorm / scale;
            float dp, hp, lo = 0, hi = -1;
            // phi'(0) = grad . search and, with the exact Hessian, phi''(0) = search^T H search = -phi'(0): the first
            // 1-D Newton step is alpha = 1 without evaluating the cones at alpha = 0
            if (majorant) ls_eval(0.f, dp, hp);
            else { dp = dp_exact; hp = -dp; }
            const float dp0abs = fabsf(dp);
            // far from the solution (large predicted decrease) the step length need not be exact: the next iteration corrects it
            const float ls_rel = scale * 0.5f * dp0abs > HSR_LS_FAR ? HSR_LS_REL_FAR : HSR_LS_REL;
            if (dp >= 0 || hp <= 0 || scale * 0.5f * (-dp) < tol) active = false;
            else {
                alpha = -dp * frcp(hp);
                // phi' has kinks where a cone changes its zone, and the 1-D Newton iteration can hop between the two ends of its bracket for
                // ever (the fp64 oracle did, round 4: 0.2575 <-> 0.4224 for all 50 iterations): from the sixth evaluation on every second
                // step bisects the bracket (a search that converges - nearly all do within four evaluations - never gets there)
                for (int k = 0; k < m.ls_iterations; k++) {
                    ls_eval(alpha, dp, hp);
#ifdef HSR_LSCOUNT
                    DBGCNT(3, 1ull);            // tools/block_times.py: line-search evaluations of lane 0's env (low word), its Newton iterations (<< 32)
#endif
                    if (fabsf(dp) < fmaxf(gtol, ls_rel * dp0abs)) break;
                    if (dp < 0) lo = alpha; else hi = alpha;
                    float nxt = alpha - dp * frcp(hp);
                    if (!(nxt > lo) || (hi > 0 && !(nxt < hi))) nxt = hi > 0 ? 0.5f * (lo + hi) : 2 * alpha;
                    else if (k >= 5 && (k & 1) && hi > 0) nxt = 0.5f * (lo + hi);
                    if (nxt == alpha) break;
                    alpha = nxt;
                }
                if (!(alpha > 0)) { active = false; alpha = 0; }
                // Newton converges quadratically here: a step predicted to gain less than HSR_LAST_DEC (scaled) and accepted at
                // nearly full length leaves a decrement of the order of its square, far below the tolerance - the next
                // iteration would assemble and factor the Hessian only to find that out (provided no contact or limit changes
                // its zone during the step: checked after the evaluation at the new point)
                last_step = scale * 0.5f * dp0abs < HSR_LAST_DEC && fabsf(alpha - 1.f) < 0.2f;
            }
        }
        PHASE(10);
#ifdef HSR_LSCOUNT
        if (active) DBGCNT(3, 1ull << 32);
#endif
        if (active) qacc_c += alpha * search_c;
#ifdef HSR_NOSTEPCOUNT
        // diagnostic (timing build; tools/block_times.py with HSR_NOSTEPCOUNT=1): counter 3 = substeps whose FIRST Newton iteration took no step in any env of the wave (the
        // iteration only confirmed convergence) | substeps with at least one iteration << 32
        if (it == 0) DBGCNT(3, (1ull << 32) | (wave_any(active && alpha > 0.f) ? 0ull : 1ull));
#endif
        ls_mv = mv; ls_alpha = active ? alpha : 0.f;
        const float newcost = eval_at(qacc_c, true);
        if (active) { iter++; cost = newcost; if (!zones_changed || (last_step && !zones_flipped)) active = false; }
        PHASE(11);
    }
    float qfc_c = 0;
    if (nefc == 0) qacc_c = qas_c;
    else if (SOLVE_STORE_DIAG && debug) qfc_c = -jt_force();          // only the introspection fields need the constraint force itself
    PHASE(14);
    if (SOLVE_STORE_DIAG) {
        if (valid && isdof) {
            s.qacc[(size_t)c * N + e] = qacc_c;
            if (debug) { s.qacc_smooth[(size_t)c * N + e] = qas_c; s.qfrc_smooth[(size_t)c * N + e] = qfs_c; s.qfrc_constraint[(size_t)c * N + e] = qfc_c; }
        }
        if (valid && c == 0) { s.ncon[e] = ncon; s.nefc[e] = nefc; s.niter[e] = iter; }
    }
    if (mode == 0) {
        PHASE_FLUSH();
        const float bsum = gsum<G>((float)bad);
        if (valid && c == 0 && bsum > 0) s.bad[e] = 1;
        return;
    }

    PHASE(12);
    // ---------------- phase G: mj_Euler (a-2.7): implicit joint damping, semi-implicit update
    const float h = m.timestep;
    float acc_c = qacc_c;
    if (m.any_damping) {
        float Ar[G];
#pragma unroll
        for (int k = 0; k < NK; k++) Ar[k] = Mrow[k] + ((k == c) ? h * damp_c : 0.f);
        float ainvd;
        if constexpr (NDK >= 0) { if (!chol_g_tail<G, NK, NDK>(Ar, ainvd, Mdiag_c + (isdof ? h * damp_c : 0.f), c)) bad = 1; }
        else if (!chol_g<G, NK>(Ar, ainvd, nv, m.ndense, c)) bad = 1;
        PHASE(15);
        // right-hand side M qacc: equal to qfrc_smooth + qfrc_constraint at the solver's fixed point (its gradient), but immune to what
        // the solver leaves unconverged - a residual force along a stiff contact direction (H >> M there) that is negligible in the
        // solver's own metric would otherwise be integrated as if it were real
        if constexpr (NDK >= 0) acc_c = chol_solve_tail<G, NK, NDK>(Ar, ainvd, nefc == 0 ? qfs_c : Ma_c, c);
        else acc_c = chol_solve_mf<G, NK>(Ar, ainvd, nefc == 0 ? qfs_c : Ma_c, nv, c);
    }
    PHASE(12);
    const float vnew = isdof ? qvel_c + h * acc_c : 0.f;
    if (!(fabsf(vnew) <= 1e10f)) bad = 1;
#undef LINK_MOVES_WITH_DOF
