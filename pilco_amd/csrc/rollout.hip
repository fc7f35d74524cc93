// Rollouts (PILCO.predict / propagate, pilco/models/pilco.py:118-153): plan, launch sequence, hipGraph capture
// and replay, and the policy / reward evaluation entry points.
#include "ctx.h"
#include "reward_factor.h"

namespace {

constexpr size_t GLUE_LDS_LIMIT = 160 * 1024;   // bytes of LDS a workgroup can have on gfx950

// marshal reward terms into a host staging vector; pointers are patched relative to dev_base
int stage_rewards(pilco_ctx* ctx, const pilco_reward_term* rw, int n_rw, int E, std::vector<double>& hp, size_t& off,
                  const double* dev_base, RewardDev* out) {
    for (int i = 0; i < n_rw; ++i) {
        out[i].kind = rw[i].kind;
        out[i].coef = rw[i].coef;
        out[i].F = nullptr;
        out[i].rank = -1;
        if (!rw[i].W) return fail(ctx, PILCO_E_SHAPE, "reward: W is required");
        if (rw[i].kind == PILCO_REWARD_EXPONENTIAL) {
            hp.resize(std::max(hp.size(), off + (size_t)2 * E * E + E));
            memcpy(&hp[off], rw[i].W, sizeof(double) * E * E);
            out[i].W = dev_base + off; off += (size_t)E * E;
            if (rw[i].t) memcpy(&hp[off], rw[i].t, sizeof(double) * E);
            else std::fill(hp.begin() + off, hp.begin() + off + E, 0.0);
            out[i].t = dev_base + off; off += E;
            std::vector<double> F;
            const int r = pilco::psd_factor(rw[i].W, E, F);   // (reward_factor.h)
            out[i].rank = r;
            if (r > 0) {
                memcpy(&hp[off], F.data(), sizeof(double) * E * r);
                out[i].F = dev_base + off;
            } else if (r == 0) {
                out[i].F = dev_base + off;
            }
            off += (size_t)E * E;
        } else if (rw[i].kind == PILCO_REWARD_LINEAR) {
            hp.resize(std::max(hp.size(), off + (size_t)E));
            memcpy(&hp[off], rw[i].W, sizeof(double) * E);
            out[i].W = dev_base + off; off += E;
            out[i].t = out[i].W;
        } else {
            return fail(ctx, PILCO_E_SHAPE, "reward: unknown kind");
        }
    }
    return PILCO_OK;
}

}  // namespace

int setup_rollout(pilco_ctx* ctx, const pilco_policy* pol, const pilco_reward_term* rw, int n_rw, int H, bool want_traj,
                  RolloutPlan& plan) {
    Slot& s = ctx->slot[0];
    if (!s.factor_valid) return fail(ctx, PILCO_E_STATE, "rollout: dynamics model has no current factorisation");
    if (!s.beta_complete) return fail(ctx, PILCO_E_STATE, "rollout: beta of the other ranks is missing (attach a communicator before factorising, or pilco_group_sync_model)");
    if (s.shW != ctx->nranks || s.shRank != ctx->rank) return fail(ctx, PILCO_E_STATE, "rollout: the model was factorised under a different rank layout; factorise again");
    if (!pol) return fail(ctx, PILCO_E_SHAPE, "rollout: null policy");
    const int E = s.E, D = s.D, U = D - E;
    if (pol->state_dim != E || pol->control_dim != U || U < 0)
        return fail(ctx, PILCO_E_SHAPE, "rollout: policy dims do not match the model (state_dim must be E, control_dim D-E)");
    if (pol->kind == PILCO_POLICY_NONE && U != 0) return fail(ctx, PILCO_E_SHAPE, "rollout: policy NONE needs D == E");
    if (pol->kind == PILCO_POLICY_LINEAR && (U == 0 || !pol->W || !pol->b)) return fail(ctx, PILCO_E_SHAPE, "rollout: linear policy needs W, b and control_dim > 0");
    if (pol->kind == PILCO_POLICY_RBF) {
        Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
        if (!ps.factor_valid) return fail(ctx, PILCO_E_STATE, "rollout: RBF policy slot has no current factorisation");
        if (ps.D != E || ps.E != U || U == 0) return fail(ctx, PILCO_E_SHAPE, "rollout: RBF policy GP must map state_dim -> control_dim");
        if (ctx->nranks != 1 && !(ctx->inline_policy && rbf_inline_lds_doubles(E, U, ps.n) > 0))
            return fail(ctx, PILCO_E_STATE, "rollout: with several ranks an RbfController must be small enough for the inline evaluation (pilco_set_inline_policy)");
        if (int r = build_work(ctx, ps)) return r;
    }
    if (pol->kind < 0 || pol->kind > 2) return fail(ctx, PILCO_E_SHAPE, "rollout: unknown policy kind");
    if (n_rw < 0 || n_rw > MAX_REWARD_TERMS || (n_rw > 0 && !rw)) return fail(ctx, PILCO_E_SHAPE, "rollout: 0..4 reward terms supported");
    if (int r = build_work(ctx, s)) return r;
    ctx->route.fill(0);
    ctx->route[ROUTE_ENTRY] = 1;
    // state: 2 x (m_x[E] s_x[E*E]) | s1[E*D] | reward[1]
    const size_t n_state = 2 * ((size_t)E + E * E) + 2 * (size_t)E * D + 1 + 8;
    ENSURE(ctx->state, n_state);
    // params: W[U*E] b[U] maxact[U] then per reward W[E*E] t[E] F[E*E]
    const size_t n_par = (size_t)U * E + 2 * U + (size_t)MAX_REWARD_TERMS * (2 * E * E + E) + 8;
    ENSURE(ctx->params, n_par);
    if (want_traj) ENSURE(ctx->traj, (size_t)(H + 1) * (E + E * E));
    std::vector<double> hp(n_par, 0.0);
    size_t off = 0;
    GlueArgs& g = plan.g;
    g = GlueArgs{};
    g.E = E; g.D = D; g.U = U;
    g.wk = s.wk;
    g.var = s.var.p;
    plan.st[0] = ctx->state.p;
    plan.st[1] = ctx->state.p + (E + E * E);
    g.s1 = ctx->state.p + 2 * (E + E * E);
    plan.s1b[0] = g.s1;
    plan.s1b[1] = g.s1 + (size_t)E * D;
    g.reward = g.s1 + 2 * (size_t)E * D;
    g.traj = want_traj ? ctx->traj.p : nullptr;
    g.pol_kind = pol->kind;
    g.squash = pol->squash;
    if (pol->kind == PILCO_POLICY_RBF) {
        g.pwk = ctx->slot[PILCO_SLOT_POLICY].wk;
        g.pvar = ctx->slot[PILCO_SLOT_POLICY].var.p;
        g.pmd = model_of(ctx->slot[PILCO_SLOT_POLICY]);
        g.pol_lds = rbf_inline_lds_doubles(E, U, ctx->slot[PILCO_SLOT_POLICY].n);   // (g.pol_inline: plan_route)
        for (int u = 0; u < U; ++u) hp[off + u] = pol->max_action ? pol->max_action[u] : 1.0;
        g.maxact = ctx->params.p + off; off += U;
    }
    if (pol->kind == PILCO_POLICY_LINEAR) {
        memcpy(&hp[off], pol->W, sizeof(double) * U * E);
        g.W = ctx->params.p + off; off += (size_t)U * E;
        memcpy(&hp[off], pol->b, sizeof(double) * U);
        g.b = ctx->params.p + off; off += U;
        for (int u = 0; u < U; ++u) hp[off + u] = pol->max_action ? pol->max_action[u] : 1.0;
        g.maxact = ctx->params.p + off; off += U;
    }
    g.n_rewards = n_rw;
    g.rew_out = nullptr;
    if (int r = stage_rewards(ctx, rw, n_rw, E, hp, off, ctx->params.p, g.rw)) return r;
    if (hp.size() > n_par) return fail(ctx, PILCO_E_ALLOC, "rollout: parameter staging overflow");
    // the policy / reward parameters of consecutive rollouts are usually the same bytes (bench loop, restarts,
    // compute_reward after an optimiser step): upload only when they changed
    if (ctx->params_dev != ctx->params.p || ctx->params_host.size() != n_par ||
        memcmp(ctx->params_host.data(), hp.data(), sizeof(double) * n_par) != 0) {
        HIPCHK(hipMemcpyAsync(ctx->params.p, hp.data(), sizeof(double) * n_par, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));  // hp is a local vector
        ctx->params_host = hp;
        ctx->params_dev = ctx->params.p;
    }
    plan.E = E; plan.D = D; plan.U = U;
    return PILCO_OK;
}

// Host side of a rollout's exchanges: the epoch base goes up before the rollout's launches (outside any graph: the
// value changes per replay), `n` exchanges are accounted for afterwards.
static int xq_begin(pilco_ctx* ctx) {
    PeerXch& x = ctx->xq;
    unsigned long long* slot = x.pin + (x.ring++ & 127u);   // a ring: rollouts may be queued without a host sync in between
    *slot = x.epoch;
    HIPCHK(hipMemcpyAsync(x.local, slot, sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->st));
    return PILCO_OK;
}

// Column splits of the one-launch small step (MMWork::NCS): with 64-row workgroups whose operands stay in LDS, a pair's
// columns are dealt over up to four workgroups as long as the whole launch stays ONE round of the chip (one workgroup per
// CU) -- a small model with few outputs would otherwise leave most CUs idle while 40 of them work through the pair sums.
static int small_col_splits(pilco_ctx* ctx, const Slot& s, bool rew) {
    if (s.npad / s.wk.NCH != 64 || s.wk.KP > 16) return 1;
    static const int forced = getenv("PILCO_SMALL_NCS") ? atoi(getenv("PILCO_SMALL_NCS")) : 0;   // (tools: A/B)
    const int cus = device_cus_of(ctx->device), spare = s.wk.EL * s.wk.NCHM + (rew ? 1 : 0);
    int ncs = 1;
    while (ncs * 2 <= s.wk.NCH && ncs * 2 <= 4 && s.wk.PL * s.wk.NCH * ncs * 2 + spare <= cus) ncs *= 2;
    if (forced > 0 && forced <= s.wk.NCH && (forced & (forced - 1)) == 0 && forced <= 4) ncs = forced;
    return ncs;
}

// Decide the route of a rollout of H steps before anything is enqueued (`timed`: event pairs will bracket its O(N^2)
// launches).  Sets plan.route, the policy evaluation it implies (plan.g.pol_inline) and the route record
// (pilco_debug_last_route): the eager launches, the graph key and a replay all follow this one decision.
static int plan_route(pilco_ctx* ctx, RolloutPlan& plan, int H, bool timed) {
    const Slot& s = ctx->slot[0];
    const GlueArgs& g = plan.g;
    const bool rbf = g.pol_kind == PILCO_POLICY_RBF, jac = plan.jrec != nullptr;
    const bool one = ctx->nranks == 1 && !ctx->comm, steps = s.wk.PL > 0 && H > 0;
    // The fused heads need the serial link's and the operand kernel's LDS side by side in one workgroup: wide models
    // (D > 24 with many outputs) exceed the CU's 160 KB and run the three-kernel step instead (same results).
    // The answer must be the SAME ON EVERY RANK (it selects between the peer exchange and the collective path, and ranks
    // that disagree wait for each other forever): it is computed from the model dimensions and the rank COUNT only -- the
    // geometry of rank 0, which holds the largest share of pairs and outputs under the round-robin dealing.
    auto fits = [&](bool inline_pol) {
        GlueArgs gl = g;
        gl.pol_inline = inline_pol ? 1 : 0;
        if (ctx->nranks > 1) {
            const int W = ctx->nranks, P = s.E * (s.E + 1) / 2;
            gl.wk.PL = (P + W - 1) / W;
            gl.wk.EL = (s.E + W - 1) / W;
            mm_prep_chunks(s.npad, std::max(gl.wk.PL, 1), gl.wk.EL, &gl.wk.NCH, &gl.wk.NCHM);
        } else if (s.wk.PL <= 0) {
            return true;
        }
        const bool rbf_k = rbf && !inline_pol;   // the policy GP as launches of its own (an inline policy is part of the link)
        gl.flags = GF_TRAJ | GF_POLICY | GF_PACK | GF_ASSEMBLE | GF_PROPAGATE | (rbf_k ? (GF_RBF_PRE | GF_RBF_POST) : 0);
        const int rew_E = g.n_rewards > 0 ? plan.E : 0;
        return mm_fused_head_fits(model_of(s), rew_E, gl) &&
               (!rbf_k || mm_fused_head_fits(model_of(ctx->slot[PILCO_SLOT_POLICY]), rew_E, gl));
    };
    // An RbfController small enough (GlueArgs::pol_lds) is evaluated inside the link: on one rank when the fused head runs
    // the step (which makes it the LinearController's: two launches); on several ranks always -- the policy GP is never
    // sharded (every rank holds all of it) and its own launches would deal its pairs over the ranks -- by the fused head
    // over the peer exchange, or (value-and-gradient rollouts: the three-kernel step with the all-gather) by the link kernel.
    const bool eligible = rbf && ctx->inline_policy && g.pol_lds > 0;
    if (rbf && !one && !eligible)
        return fail(ctx, PILCO_E_STATE, "rollout: several ranks run an RbfController only with the inline policy (at most 256 basis functions, see pilco_set_inline_policy)");
    const bool inl = eligible && (!one || (ctx->fused && steps && fits(true)));
    const bool fit = fits(inl);
    StepRoute r;
    int step = STEP_THREE;
    if (one && ctx->fused && fit && steps && (!rbf || inl)) {
        step = STEP_FUSED;
        // Small models: the pair sums ride in the head launch (prep_device.h) -- one launch per step.  The head instantiated for
        // this input dimension carries the pair arithmetic of ONE contraction depth (that of D = DT); the workgroup's rows must
        // be whole 32-row groups and one thread per point must cover the columns.  Value-and-gradient rollouts (the Jacobian
        // tape, D <= 14) take the same road when the workgroup's operands stay in LDS (64-row chunks, KP <= 16): the pair
        // workgroups run the reverse sweep of their block (small_sweep).
        const int dt = mm_prep_dt(s.D);
        const bool small = ctx->fuse_small && !timed && !MM_ABL(s.wk, 255) && s.npad <= 256 && s.wk.KP == mm_kp(dt) &&
                           (s.wk.vsep != 0) == mm_vsep(dt) &&
                           (jac ? s.npad / s.wk.NCH == 64 && s.wk.KP <= 16 : (s.npad / s.wk.NCH) % 32 == 0 && ctx->variant == 0);
        if (small) {
            step = STEP_SMALL;
            r.ncs = small_col_splits(ctx, s, g.n_rewards > 0 && !MM_ABL(s.wk, 8));
        }
    } else if (ctx->xq.ready && ctx->nranks > 1 && ctx->xq.W == ctx->nranks && H > 0 && (!rbf || inl) && s.wk.SEG <= ctx->xq.cap &&
               !g.tape && !jac && fit) {
        step = STEP_PEER;   // the peer exchange is attached and the segments fit its slots; otherwise the RCCL / group path runs
    } else if (one && ctx->fused && fit && rbf && steps && ctx->slot[PILCO_SLOT_POLICY].wk.PL > 0) {
        step = STEP_FUSED_RBF;
    }
    r.step = H > 0 ? step : STEP_NONE;
    r.policy = rbf ? (inl ? 1 : 2) : 0;
    r.pair = !steps ? -1 : step == STEP_SMALL ? (jac ? 5 : 3) : jac ? 4 : ctx->variant;
    r.timed = timed;
    plan.route = r;
    plan.g.pol_inline = inl ? 1 : 0;
    auto& w = ctx->route;
    w[ROUTE_STEP] = r.step;
    w[ROUTE_POLICY] = r.policy;
    w[ROUTE_DT] = mm_prep_dt(s.D);
    w[ROUTE_KP] = s.wk.KP;
    w[ROUTE_VSEP] = s.wk.vsep ? 1 : 0;
    w[ROUTE_PAIR] = r.pair;
    w[ROUTE_TAPE] = jac ? 2 : (g.tape ? 1 : 0);
    w[ROUTE_H] = H;
    w[ROUTE_NPAD] = s.npad;
    return PILCO_OK;
}

// single-rank fused heads (STEP_FUSED / STEP_SMALL): the closing launch hands the results to the host where the caller gave it a
// pinned block (plan.host_out: pilco_rollout and the lanes of pilco_rollout_batch)
static bool results_to_host(const RolloutPlan& plan, int H) {
    return H > 0 && plan.host_out && (plan.route.step == STEP_FUSED || plan.route.step == STEP_SMALL);
}

// The reward of a state (pilco.py:133) rides in a spare workgroup of a head or prep launch: of the state the link holds in
// LDS, or (m_x given: the three-kernel step) of the state at m_x
static PrepReward reward_arg(const RolloutPlan& plan, const double* m_x = nullptr) {
    PrepReward pr{};
    pr.n = plan.g.n_rewards;
    pr.E = plan.E;
    for (int i = 0; i < plan.g.n_rewards; ++i) pr.rw[i] = plan.g.rw[i];
    if (m_x) {
        pr.m_x = m_x;
        pr.s_x = m_x + plan.E;
    }
    pr.reward = plan.g.reward;
    return pr;
}
// Head of step h: its link turns state h - 1 into state h (h > 0) and hands state h on.  The state and s1 the link reads
// (written by the launch before) and those it writes alternate between two buffers, because the workgroups of one launch
// are not ordered.
static GlueArgs head_args(const RolloutPlan& plan, const GlueArgs& g, int h, int flags) {
    GlueArgs gh = g;
    gh.step = h;
    gh.flags = flags;
    gh.m_x = plan.st[h > 0 ? (h - 1) & 1 : 0];
    gh.s_x = gh.m_x + plan.E;
    gh.m_out = h > 0 ? plan.st[h & 1] : nullptr;
    gh.s_out = h > 0 ? plan.st[h & 1] + plan.E : nullptr;
    gh.s1 = plan.s1b[(h + 1) & 1];
    gh.s1_out = plan.s1b[h & 1];
    return gh;
}
// The closing glue launch: state H from state H - 1
static GlueArgs closing_args(const RolloutPlan& plan, const GlueArgs& g, int H, int flags) {
    GlueArgs gf = g;
    gf.step = H;
    gf.flags = flags;
    gf.m_x = plan.st[(H - 1) & 1];
    gf.s_x = gf.m_x + plan.E;
    gf.m_out = plan.st[H & 1];
    gf.s_out = gf.m_out + plan.E;
    gf.s1 = plan.s1b[(H - 1) & 1];
    gf.s1_out = nullptr;
    return gf;
}
// The dynamics step's O(N^2) launch of step t -- the pair kernel, or with the Jacobian tape the reverse sweep, which writes
// the step's records -- bracketed by an event pair in a timed rollout
static int dyn_pairs(pilco_ctx* ctx, const RolloutPlan& plan, const MMModel& md, const MMWork& w, int t) {
    const Slot& s = ctx->slot[0];
    if (plan.route.timed) HIPCHK(hipEventRecord(ctx->pair_events[2 * t], ctx->st));
    if (plan.jrec)
        launch_mm_sweep(ctx->st, md, w, s.jac_rowmom.p + (size_t)t * mm_jac_rowmom_size(s.npad, s.wk.PL),
                        s.jac_cpart.p + (size_t)t * mm_jac_cpart_size(s.npad, s.wk.PL, s.wk.EL),
                        s.jac_head.p + (size_t)t * mm_jac_head_size(s.D, s.E, s.wk.PL), s.jac_np.p);
    else
        launch_mm_pair(ctx->st, md, w, ctx->variant);
    if (plan.route.timed) HIPCHK(hipEventRecord(ctx->pair_events[2 * t + 1], ctx->st));
    return PILCO_OK;
}

// STEP_FUSED / STEP_SMALL: launch h = 0..H-1 is [serial link producing state h and its joint Gaussian | operands of step h],
// followed by the pair kernel of step h; one plain glue launch closes the rollout.  What the link reads (previous step's
// pair_isdet / mean_part / s1 / state) and what the same launch writes alternate between two buffer sets.  The one-launch
// small step runs the pair sums (or the reverse sweep) of step h inside head h.
static int enqueue_fused(pilco_ctx* ctx, const RolloutPlan& plan, const GlueArgs& g, int H) {
    Slot& s = ctx->slot[0];
    const MMModel md = model_of(s);
    const bool small = plan.route.step == STEP_SMALL, jac = plan.jrec != nullptr, rew = g.n_rewards > 0 && !MM_ABL(s.wk, 8);
    MMWork wkb[2] = {g.wk, g.wk};
    wkb[1].pair_isdet = s.alt_isdet;
    wkb[1].mean_part = s.alt_mean;
    if (small)
        for (int k = 0; k < 2; ++k) {
            wkb[k].fuse_pair = jac ? 2 : 1;
            wkb[k].sk_waves = 0;           // the link packs tile partials: one per (pair, row chunk)
            wkb[k].NCS = plan.route.ncs;
            wkb[k].share_cu = ctx->share_cu;
            wkb[k].NT = g.wk.NCH * plan.route.ncs;
            wkb[k].pair_part = s.w_fpart.p + (size_t)k * std::max(g.wk.PL, 1) * g.wk.NCH * 4 * 2;
        }
    const PrepReward pr = reward_arg(plan);   // reward of state h, from the link's LDS copy of the state
    for (int h = 0; h < H; ++h) {
        GlueArgs gh = head_args(plan, g, h, GF_TRAJ | GF_POLICY | (h > 0 ? (GF_PACK | GF_ASSEMBLE | GF_PROPAGATE) : 0));
        gh.dbg_off = h > 0 ? 48 : 0;              // fused heads stamp slots 56..61 (the closing k_glue keeps 8..13)
        gh.wk = wkb[(h + 1) & 1];                 // read side: written by launch h - 1
        MMWork wh = wkb[h & 1];
        if (small && jac) wh.sw_gpart = s.jac_rowmom.p + (size_t)h * mm_jac_rowmom_size(s.npad, s.wk.PL);
        launch_mm_prep(ctx->st, md, wh, rew ? &pr : nullptr, &gh);
        if (!small)
            if (int r = dyn_pairs(ctx, plan, md, wkb[h & 1], h)) return r;
    }
    GlueArgs gf = closing_args(plan, g, H, GF_PACK | GF_ASSEMBLE | GF_PROPAGATE | GF_TRAJ);
    gf.wk = wkb[(H - 1) & 1];
    launch_glue(ctx->st, gf, false, results_to_host(plan, H) ? plan.host_out : nullptr);
    return PILCO_OK;
}

// STEP_PEER: sharded rollout with the peer exchange (GlueArgs::xq): per step
//   head  [wait for the W flags of exchange h - 1, segments from the own area -> assemble / propagate / controller
//          / joint, redundantly in every workgroup | operands of step h]        (ranks without pairs: a plain k_glue)
//   pairs of this rank
//   push  [pack this rank's segment, store it into every rank's area, raise the flag there]   (one workgroup)
// No host involvement and no collective launch per step; the state and s1 alternate between two buffers as in the
// single-rank fused path.  The reward of state h is taken by head h (k_glue launches: by the launch that propagates
// state h, from its pre-propagation copy), i.e. in the same order on every rank.
static int enqueue_peer(pilco_ctx* ctx, const RolloutPlan& plan, const GlueArgs& g, int H) {
    Slot& s = ctx->slot[0];
    const MMModel md = model_of(s);
    const bool rew = g.n_rewards > 0 && !MM_ABL(s.wk, 8);
    PeerXch& x = ctx->xq;
    {   // executed now (not being captured into a graph): this rollout's epoch base goes up ahead of its launches
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCHK(hipStreamIsCapturing(ctx->st, &cs));
        if (cs == hipStreamCaptureStatusNone) {
            if (int r = xq_begin(ctx)) return r;
            x.epoch += (unsigned long long)H;
        }
    }
    const int spin = 2000000;   // ~2 s of polling before a wait gives up
    // Contexts of ONE process sharing a GPU (pilco_rollout_group after pilco_group_peer_attach): their streams may share
    // hardware queues, which start their packets in order, so a rank's flag wait could sit in a queue ahead of the push
    // it waits for.  The ranks' host threads therefore enqueue in lockstep -- every rank's push of step h is in the
    // queues before any rank's wait for it -- and run_rollout does not capture these rollouts into a graph.
    PeerGroup* lockstep = (x.wait_kernel && ctx->group) ? ctx->group.get() : nullptr;
    auto with_xq = [&](GlueArgs& ga, int k) {
        ga.xq = x.local;
        ga.xq_k = k;
        ga.xq_W = x.W;
        ga.xq_cap = x.cap;
        ga.xq_spin = x.wait_kernel ? 1000 : spin;   // behind a wait launch the flags are already up
    };
    const PrepReward pr = reward_arg(plan);
    for (int h = 0; h < H; ++h) {
        GlueArgs gh = head_args(plan, g, h, GF_TRAJ | GF_POLICY | (h > 0 ? (GF_ASSEMBLE | GF_PROPAGATE) : 0));
        gh.wk = s.wk;
        if (h > 0) {
            with_xq(gh, h - 1);
            if (x.wait_kernel) launch_peer_wait(ctx->st, x.local, h - 1, x.W, spin);
        }
        if (s.wk.PL > 0) {
            launch_mm_prep(ctx->st, md, s.wk, rew ? &pr : nullptr, &gh);
            if (int r = dyn_pairs(ctx, plan, md, s.wk, h)) return r;
        } else {
            launch_glue(ctx->st, gh, rew && h > 0);   // its reward workgroup takes the pre-propagation state h - 1
        }
        GlueArgs gp = g;
        gp.step = h + 1;
        gp.wk = s.wk;
        gp.flags = GF_PACK;
        with_xq(gp, h);
        gp.xq_peers = x.d_peers;
        launch_glue(ctx->st, gp);
        if (lockstep && !lockstep->arrive_and_wait()) return fail(ctx, PILCO_E_STATE, "rollout: another rank of the group failed");
    }
    GlueArgs gf = closing_args(plan, g, H, GF_ASSEMBLE | GF_PROPAGATE | GF_TRAJ);
    gf.wk = s.wk;
    with_xq(gf, H - 1);
    if (x.wait_kernel) launch_peer_wait(ctx->st, x.local, H - 1, x.W, spin);
    launch_glue(ctx->st, gf, rew && s.wk.PL == 0);
    return PILCO_OK;
}

// STEP_FUSED_RBF: fused heads with an RbfController (controllers.py:108-121): the policy is a moment-matching GP of its own,
// so a step is two head + pair rounds and the serial link splits in two:
//   policy head   [pack / assemble / propagate of step h - 1 -> state h | operands of the POLICY GP at state h]
//   policy pairs
//   dynamics head [reduce the policy GP, S -= diag(var - 1e-6), squash, joint Gaussian | operands of step h]
//   dynamics pairs
// four launches per step instead of six (two of them single-workgroup glue launches).  What a head's link reads was
// written by EARLIER launches and what its prep part writes belongs to the other GP: no double buffering beyond the
// state's (one s1).
static int enqueue_fused_rbf(pilco_ctx* ctx, const RolloutPlan& plan, const GlueArgs& g, int H) {
    Slot& s = ctx->slot[0];
    Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
    const MMModel md = model_of(s), pmd = model_of(ps);
    const bool rew = g.n_rewards > 0 && !MM_ABL(s.wk, 8);
    const PrepReward pr = reward_arg(plan);   // reward of state h, from the link's LDS copy of the state
    for (int h = 0; h < H; ++h) {
        GlueArgs ga = head_args(plan, g, h, GF_TRAJ | GF_RBF_PRE | (h > 0 ? (GF_PACK | GF_ASSEMBLE | GF_PROPAGATE) : 0));
        ga.dbg_off = h > 0 ? 48 : 0;
        ga.s1 = g.s1;
        ga.s1_out = g.s1_out;
        launch_mm_prep(ctx->st, pmd, ps.wk, rew ? &pr : nullptr, &ga);
        launch_mm_pair(ctx->st, pmd, ps.wk, ctx->variant);
        GlueArgs gc = g;
        gc.step = h;
        gc.flags = GF_RBF_POST | GF_POLICY;
        gc.m_x = plan.st[h & 1];
        gc.s_x = gc.m_x + plan.E;
        gc.m_out = nullptr;
        gc.s_out = nullptr;
        launch_mm_prep(ctx->st, md, s.wk, nullptr, &gc);
        if (int r = dyn_pairs(ctx, plan, md, s.wk, h)) return r;
    }
    GlueArgs gf = closing_args(plan, g, H, GF_PACK | GF_ASSEMBLE | GF_PROPAGATE | GF_TRAJ);
    gf.s1 = g.s1;
    launch_glue(ctx->st, gf);
    return PILCO_OK;
}

// STEP_THREE: per step a prep launch, the pair launch and a glue launch (pack / assemble / propagate / policy; several
// ranks: a pack launch and the all-gather of the segments in between).  An RbfController with launches of its own
// (controllers.py:108-121): the glue that produced the state hands it to the policy GP (GF_RBF_PRE), the policy's moment
// matching runs as its own prep/pair, a second glue squashes and builds the joint Gaussian (GF_RBF_POST | GF_POLICY).
static int enqueue_three_kernel(pilco_ctx* ctx, const RolloutPlan& plan, GlueArgs g, int H) {
    Slot& s = ctx->slot[0];
    Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
    const bool rbf = g.pol_kind == PILCO_POLICY_RBF, rew = g.n_rewards > 0 && !MM_ABL(s.wk, 8);
    const MMModel md = model_of(s), pmd = rbf ? model_of(ps) : MMModel{};
    auto policy_stage = [&](GlueArgs& ga) {
        launch_mm_prep(ctx->st, pmd, ps.wk);
        launch_mm_pair(ctx->st, pmd, ps.wk, ctx->variant);
        const int keep = ga.flags;
        ga.flags = GF_RBF_POST | GF_POLICY;
        launch_glue(ctx->st, ga);
        ga.flags = keep;
    };
    const bool rbf_l = rbf && !g.pol_inline;   // the policy GP as launches of its own (an inline policy is part of the link kernel)
    g.flags = GF_TRAJ | (H > 0 ? (rbf_l ? GF_RBF_PRE : GF_POLICY) : 0);
    launch_glue(ctx->st, g);
    if (rbf_l && H > 0) policy_stage(g);
    for (int t = 0; t < H; ++t) {
        if (s.wk.PL > 0) {
            const PrepReward pr = reward_arg(plan, plan.st[t & 1]);   // reward of state t
            launch_mm_prep(ctx->st, md, s.wk, rew ? &pr : nullptr);
            if (ctx->dbg && MM_ABL(s.wk, 64)) launch_stamp(ctx->st, ctx->dbg, 30);
            if (int r = dyn_pairs(ctx, plan, md, s.wk, t)) return r;
        }
        g.step = t + 1;
        g.m_x = plan.st[t & 1];
        g.s_x = plan.st[t & 1] + plan.E;
        g.m_out = plan.st[(t + 1) & 1];
        g.s_out = plan.st[(t + 1) & 1] + plan.E;
        const bool more = t + 1 < H;
        const int tail = GF_ASSEMBLE | GF_PROPAGATE | GF_TRAJ | (more ? (rbf_l ? GF_RBF_PRE : GF_POLICY) : 0);
        if (ctx->nranks == 1 && !ctx->comm) {
            g.flags = GF_PACK | tail;
        } else {
            g.flags = GF_PACK;
            launch_glue(ctx->st, g);
            if (int r = all_gather_segments(ctx, s)) return r;
            g.flags = tail;
        }
        launch_glue(ctx->st, g, rew && s.wk.PL == 0);   // (a rank without pairs keeps the reward in the glue launch)
        if (rbf_l && more) {  // the policy stage reads the NEW state
            g.m_x = g.m_out;
            g.s_x = g.s_out;
            policy_stage(g);
        }
    }
    return PILCO_OK;
}

// Enqueue one full rollout of H steps along plan.route (initial state already in plan.st[0]); the final state ends up in
// plan.st[H & 1].
static int enqueue_rollout_steps(pilco_ctx* ctx, const RolloutPlan& plan, int H) {
    Slot& s = ctx->slot[0];
    while (plan.route.timed && ctx->pair_events.size() < (size_t)2 * std::max(H, 1)) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        ctx->pair_events.push_back(e);
    }
    HIPCHK(hipMemsetAsync(plan.g.reward, 0, sizeof(double), ctx->st));
    GlueArgs g = plan.g;
    g.step = 0;
    g.m_x = plan.st[0];
    g.s_x = plan.st[0] + plan.E;
    g.m_out = nullptr;
    g.s_out = nullptr;
    if (plan.jrec) {   // Jacobian tape (bwd.hip): the serial link packs N_ab from the per-workgroup partials the reverse sweep
        g.wk.sk_waves = 0;   // leaves in the tile-partial layout
        g.wk.NT = mm_jac_nt(s.npad, s.wk.P, s.wk.KP);
        g.wk.pair_part = s.jac_np.p;
    }
    switch (plan.route.step) {
        case STEP_FUSED:
        case STEP_SMALL: return enqueue_fused(ctx, plan, g, H);
        case STEP_PEER: return enqueue_peer(ctx, plan, g, H);
        case STEP_FUSED_RBF: return enqueue_fused_rbf(ctx, plan, g, H);
        default: return enqueue_three_kernel(ctx, plan, g, H);
    }
}

// Run one rollout to completion: replay the cached hipGraph when the launch sequence is unchanged (same route, buffers,
// sizes, horizon, policy / reward structure), otherwise (re)capture it first.  `upload` enqueues the initial state into
// plan.st[0]; a capture's eager warm-up overwrites it, so it is enqueued again in front of the replay.
template <class Upload>
static int run_rollout(pilco_ctx* ctx, RolloutPlan& plan, int H, Upload&& upload) {
    Slot& s = ctx->slot[0];
    if (int r = plan_route(ctx, plan, H, ctx->time_pairs)) return r;
    const StepRoute& rt = plan.route;
    const bool peer = rt.step == STEP_PEER;   // no collective nodes: captured like a single-rank rollout
    // With a communicator the captured graph contains the ncclAllGather nodes (RCCL supports stream capture); if capture or
    // instantiation fails the rollout falls back to eager launches for good.
    const bool sharded = (ctx->nranks != 1 || ctx->comm) && !peer;
    auto eager = [&] {
        if (int r = upload()) return r;
        return enqueue_rollout_steps(ctx, plan, H);
    };
    if (ctx->time_pairs) {   // measurement mode (pilco_set_pair_timing): eager, an event pair around every O(N^2) launch
        ctx->timed_pairs = 0;
        if (int r = eager()) return r;
        ctx->timed_pairs = (s.wk.PL > 0) ? H : 0;
        return PILCO_OK;
    }
    const bool lockstep = peer && ctx->group && ctx->xq.wait_kernel;   // enqueued step by step with the group (enqueue_peer)
    if (!ctx->use_graph || lockstep || (sharded && (!ctx->comm || ctx->graph_rccl_failed)) || (ctx->dbg && !getenv("PILCO_DBG_GRAPH")))
        return eager();
    const GlueArgs& g = plan.g;
    std::vector<unsigned long long> key = {
        (unsigned long long)H, (unsigned long long)g.pol_kind, (unsigned long long)g.n_rewards, (unsigned long long)g.squash,
        (unsigned long long)ctx->variant, (unsigned long long)rt.step, (unsigned long long)rt.policy, (unsigned long long)(long long)rt.pair,
        (unsigned long long)rt.ncs, (unsigned long long)(ctx->share_cu != 0), (unsigned long long)(uintptr_t)plan.st[0], (unsigned long long)(uintptr_t)g.s1,
        (unsigned long long)(uintptr_t)g.traj, (unsigned long long)(uintptr_t)g.tape, (unsigned long long)(uintptr_t)g.W, (unsigned long long)(uintptr_t)g.maxact,
        (unsigned long long)(uintptr_t)s.w_part.p, (unsigned long long)(uintptr_t)s.w_At.p, (unsigned long long)(uintptr_t)s.w_Wt.p,
        (unsigned long long)(uintptr_t)s.w_small.p, (unsigned long long)(uintptr_t)s.w_gath.p, (unsigned long long)(uintptr_t)s.w_out.p,
        (unsigned long long)(uintptr_t)s.w_in.p, (unsigned long long)(uintptr_t)s.beta.p,
        (unsigned long long)(uintptr_t)s.iK.p, (unsigned long long)s.iK_null, (unsigned long long)(uintptr_t)s.Xt.p,
        (unsigned long long)(uintptr_t)s.Zt.p, (unsigned long long)(uintptr_t)s.ls.p, (unsigned long long)s.n,
        (unsigned long long)s.wk.sk_waves, (unsigned long long)s.wk.NT, (unsigned long long)s.wk.NCH, (unsigned long long)s.wk.NCHM, (unsigned long long)s.wk.KP, (unsigned long long)s.wk.abl,
        (unsigned long long)(uintptr_t)ctx->slot[1].w_part.p, (unsigned long long)(uintptr_t)ctx->slot[1].w_At.p,
        (unsigned long long)(uintptr_t)ctx->slot[1].beta.p, (unsigned long long)(uintptr_t)ctx->slot[1].Xt.p,
        (unsigned long long)ctx->slot[1].n,
        (unsigned long long)ctx->slot[1].wk.sk_waves, (unsigned long long)(uintptr_t)ctx->slot[1].w_small.p,
        (unsigned long long)(uintptr_t)ctx->slot[1].w_in.p, (unsigned long long)(uintptr_t)ctx->slot[1].ls.p,
        (unsigned long long)(uintptr_t)ctx->xq.local, (unsigned long long)ctx->nranks, (unsigned long long)ctx->rank,
        (unsigned long long)(uintptr_t)ctx->slot[1].var.p,
        (unsigned long long)(uintptr_t)plan.jrec, (unsigned long long)plan.jstride, (unsigned long long)(uintptr_t)s.jac_rowmom.p,
        (unsigned long long)(uintptr_t)s.jac_cpart.p, (unsigned long long)(uintptr_t)s.jac_part.p, (unsigned long long)(uintptr_t)s.jac_head.p,
        (unsigned long long)(uintptr_t)s.jac_np.p, (unsigned long long)(uintptr_t)plan.host_out};
    // the shapes themselves: buffers only grow (DevBuf::ensure), so a smaller or differently laid-out model keeps every address
    // above -- an exact model after a sparse one with M = N keeps n and npad too, and would replay the graph that reads Zt
    const Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
    for (long v : {(long)s.N, (long)s.M, (long)s.n, (long)s.npad, (long)s.Npad, (long)s.D, (long)s.E, (long)plan.U, (long)s.wk.PL,
                   (long)s.wk.EL, (long)s.wk.P, (long)s.wk.sk_total, (long)s.wk.sk_nd, (long)s.ignore_iK, (long)ps.n, (long)ps.npad,
                   (long)ps.D, (long)ps.E, (long)ps.M})
        key.push_back((unsigned long long)v);
    for (int i = 0; i < g.n_rewards; ++i) {
        key.push_back((unsigned long long)g.rw[i].kind);
        key.push_back((unsigned long long)(long long)g.rw[i].rank);
        key.push_back((unsigned long long)(uintptr_t)g.rw[i].W);
        unsigned long long cbits;
        memcpy(&cbits, &g.rw[i].coef, sizeof(cbits));
        key.push_back(cbits);
    }
    // a few instantiated graphs are kept (value rollouts and tape rollouts of an optimiser alternate): find this key
    size_t i = 0;
    while (i < ctx->graph_cache.size() && ctx->graph_cache[i].first != key) ++i;
    if (i == ctx->graph_cache.size()) {
        ctx->graph = nullptr;
        if (ctx->graph_cache.size() >= 4) {   // evict the least recently used
            (void)hipGraphExecDestroy(ctx->graph_cache.back().second);
            ctx->graph_cache.pop_back();
        }
        // warm the per-kernel one-time host configuration outside the capture (a one-step rollout: with the peer
        // exchange attached every rank runs it, so it is a complete exchange of its own epoch)
        if (int r = upload()) return r;
        if (int r = enqueue_rollout_steps(ctx, plan, H > 0 ? 1 : 0)) return r;
        HIPCHK(hipStreamSynchronize(ctx->st));
        hipGraph_t graph = nullptr;
        HIPCHK(hipStreamBeginCapture(ctx->st, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_rollout_steps(ctx, plan, H);
        hipError_t e = hipStreamEndCapture(ctx->st, &graph);
        auto eager_for_good = [&] {   // a sharded capture that fails is not fatal: this and all later sharded rollouts run eagerly
            ctx->graph_rccl_failed = true;
            (void)hipGetLastError();
            return eager();
        };
        if (rc != PILCO_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return sharded ? eager_for_good() : rc;
        }
        if (e != hipSuccess)
            return sharded ? eager_for_good() : fail(ctx, PILCO_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        e = hipGraphInstantiate(&ctx->graph, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) {
            ctx->graph = nullptr;
            return sharded ? eager_for_good() : fail(ctx, PILCO_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        }
        ctx->graph_cache.insert(ctx->graph_cache.begin(), std::make_pair(key, ctx->graph));
    } else if (i != 0) {
        std::swap(ctx->graph_cache[i], ctx->graph_cache[0]);   // most recently used first
    }
    ctx->graph = ctx->graph_cache[0].second;
    ctx->graph_key = key;
    if (int r = upload()) return r;
    if (peer) {
        if (int r = xq_begin(ctx)) return r;
        ctx->xq.epoch += (unsigned long long)H;
    }
    HIPCHK(hipGraphLaunch(ctx->graph, ctx->st));
    return PILCO_OK;
}

int rollout_run(pilco_ctx* ctx, RolloutPlan& plan, int H, const double* m0, const double* S0) {
    auto upload = [&]() -> int {
        HIPCHK(hipMemcpyAsync(plan.st[0], m0, sizeof(double) * plan.E, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipMemcpyAsync(plan.st[0] + plan.E, S0, sizeof(double) * plan.E * plan.E, hipMemcpyHostToDevice, ctx->st));
        return PILCO_OK;
    };
    return run_rollout(ctx, plan, H, upload);
}

// pilco_rollout in two halves, so that several rollouts (the lanes of pilco_rollout_batch) can be in flight at once:
// rollout_begin enqueues everything -- upload of (m0, S0), the rollout, the downloads into pinned memory -- and returns;
// rollout_end waits for the stream and hands the results out.
struct RolloutCall {
    RolloutPlan plan;
    size_t nst = 0;
    double* pin_out = nullptr;
    bool peer = false;
};
static int rollout_begin(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* m0,
                         const double* S0, int H, double* traj, RolloutCall& rc) {
    HIPCHK(hipSetDevice(ctx->device));
    RolloutPlan& plan = rc.plan;
    if (int r = setup_rollout(ctx, policy, rewards, n_rewards, H, traj != nullptr, plan)) return r;
    const int E = plan.E;
    // one pinned staging area: [m0 | S0] up in ONE asynchronous copy; [m_H | S_H | reward] come down without a copy where the
    // rollout closes with the fused heads' k_glue (it stores them here: results_to_host), else in two; one host
    // synchronisation at the end (pageable buffers would cost a blocking staging copy per call)
    const size_t nst = (size_t)E + (size_t)E * E;
    if (ctx->pin_io_cap < 2 * nst + 8) {
        if (ctx->pin_io) (void)hipHostFree(ctx->pin_io);
        ctx->pin_io = nullptr;
        ctx->pin_io_cap = 0;
        HIPCHK(hipHostMalloc((void**)&ctx->pin_io, sizeof(double) * (2 * nst + 8), hipHostMallocDefault));
        ctx->pin_io_cap = 2 * nst + 8;
    }
    double* pin_in = ctx->pin_io;
    double* pin_out = ctx->pin_io + nst;
    memcpy(pin_in, m0, sizeof(double) * E);
    memcpy(pin_in + E, S0, sizeof(double) * E * E);
    auto upload = [&]() -> int {
        HIPCHK(hipMemcpyAsync(plan.st[0], pin_in, sizeof(double) * nst, hipMemcpyHostToDevice, ctx->st));
        return PILCO_OK;
    };
    plan.host_out = pin_out;   // (part of the graph key: a block that moved re-captures)
    if (int r = run_rollout(ctx, plan, H, upload)) return r;
    if (!results_to_host(plan, H)) {
        HIPCHK(hipMemcpyAsync(pin_out, plan.st[H & 1], sizeof(double) * nst, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipMemcpyAsync(pin_out + nst, plan.g.reward, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    }
    if (traj)
        HIPCHK(hipMemcpyAsync(traj, ctx->traj.p, sizeof(double) * (size_t)(H + 1) * (E + E * E), hipMemcpyDeviceToHost, ctx->st));
    rc.peer = plan.route.step == STEP_PEER;
    if (rc.peer) HIPCHK(hipMemcpyAsync(ctx->xq.pin + 128, ctx->xq.local + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->st));
    rc.nst = nst;
    rc.pin_out = pin_out;
    return PILCO_OK;
}
static int rollout_end(pilco_ctx* ctx, RolloutCall& rc, double* mH, double* SH, double* reward) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    if (rc.peer && ctx->xq.pin[128] != 0ULL) {   // a flag wait gave up: some rank never delivered that exchange
        const unsigned long long ep = ctx->xq.pin[128];
        (void)hipMemsetAsync(ctx->xq.local + 1, 0, sizeof(unsigned long long), ctx->st);
        return fail(ctx, PILCO_E_STATE, "rollout: peer exchange " + std::to_string(ep) + " timed out on rank " + std::to_string(ctx->rank) +
                                            " (the ranks must make the same sequence of rollout calls)");
    }
    const int E = rc.plan.E;
    memcpy(mH, rc.pin_out, sizeof(double) * E);
    memcpy(SH, rc.pin_out + E, sizeof(double) * E * E);
    *reward = rc.pin_out[rc.nst];
    return PILCO_OK;
}

// A lane of pilco_rollout_batch: a context of its own whose dynamics slot borrows the parent's model.  (Re)pointed at the
// parent's current buffers before every batch; a changed geometry drops the lane's workspace and graphs.
static int lane_sync_model(pilco_ctx* parent, pilco_ctx* lane) {
    const Slot& p = parent->slot[0];
    Slot& l = lane->slot[0];
    const bool same = l.N == p.N && l.D == p.D && l.E == p.E && l.M == p.M && l.Npad == p.Npad && l.n == p.n && l.npad == p.npad &&
                      l.iK_null == p.iK_null && l.Xt.p == p.Xt.p && l.Zt.p == p.Zt.p && l.beta.p == p.beta.p && l.iK.p == p.iK.p &&
                      l.ls.p == p.ls.p && l.var.p == p.var.p;
    l.N = p.N; l.D = p.D; l.E = p.E; l.M = p.M; l.Npad = p.Npad; l.n = p.n; l.npad = p.npad;
    l.has_data = p.has_data; l.has_hyp = p.has_hyp; l.factor_valid = p.factor_valid; l.user_factors = p.user_factors;
    l.iK_null = p.iK_null; l.ignore_iK = p.ignore_iK;
    l.shW = p.shW; l.shEL = p.shEL; l.shOwn = p.shOwn; l.shRank = p.shRank; l.beta_complete = p.beta_complete;
    l.Xt.borrow(p.Xt); l.Yt.borrow(p.Yt); l.Zt.borrow(p.Zt); l.ls.borrow(p.ls); l.var.borrow(p.var); l.noise.borrow(p.noise);
    l.beta.borrow(p.beta); l.iK.borrow(p.iK);
    lane->variant = parent->variant;
    lane->fused = parent->fused;
    lane->use_graph = parent->use_graph;
    lane->fuse_small = parent->fuse_small;
    lane->inline_policy = parent->inline_policy;
    lane->grad_mode = parent->grad_mode;
    lane->dev_chain = parent->dev_chain;
    if (!same) {
        l.wk_valid = false;
        for (auto& ge : lane->graph_cache) (void)hipGraphExecDestroy(ge.second);
        lane->graph_cache.clear();
        lane->graph = nullptr;
    }
    return PILCO_OK;
}

// The B lanes of a batch call: lane 0 is the context itself, lanes 1.. are created on first use and pointed at its model.
int rollout_lanes(pilco_ctx* ctx, int B, std::vector<pilco_ctx*>& lane, const char* who) {
    while ((int)ctx->lanes.size() < B - 1) {
        pilco_ctx* l = nullptr;
        if (int r = pilco_ctx_create(ctx->device, &l)) return fail(ctx, r, std::string(who) + ": could not create a lane context");
        l->is_lane = true;
        ctx->lanes.push_back(l);
    }
    lane.resize((size_t)B);
    for (int i = 0; i < B; ++i) {
        lane[i] = i == 0 ? ctx : ctx->lanes[i - 1];
        lane[i]->share_cu = B > 1 ? 1 : 0;   // (the caller resets lane 0's when the batch is over: rollout_lanes_done)
        if (i > 0) {
            HIPCHK(hipStreamSynchronize(lane[i]->st));
            if (int r = lane_sync_model(ctx, lane[i])) return r;
        }
    }
    // the parent's model must be complete in memory before another stream reads it
    HIPCHK(hipStreamSynchronize(ctx->st));
    return PILCO_OK;
}

void rollout_lanes_done(pilco_ctx* ctx) { ctx->share_cu = 0; }

extern "C" {

int pilco_rollout(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                  const double* m0, const double* S0, int H, double* mH, double* SH, double* reward, double* traj) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!m0 || !S0 || !mH || !SH || !reward || H < 0) return fail(ctx, PILCO_E_SHAPE, "rollout: bad arguments");
    RolloutCall rc;
    if (int r = rollout_begin(ctx, policy, rewards, n_rewards, m0, S0, H, traj, rc)) return r;
    return rollout_end(ctx, rc, mH, SH, reward);
}

// B independent rollouts of ONE model in flight together (multi-start policy search, several initial states; the restart
// loop of pilco.py:96-110 evaluates its candidates one after the other).  Lane 0 is this context; lanes 1..B-1 are
// contexts of their own -- stream, per-step workspace, state, policy parameters, cached graph -- that borrow this context's
// model (X, hyper-parameters, beta, iK are not copied).  All B graph replays are enqueued before the first wait, so the
// serial head of one lane's step (a chain of latencies that leaves the chip idle) runs under the pair kernels of the
// others.  Every lane runs exactly the launch sequence of pilco_rollout: its result is bit-identical to its solo run.
int pilco_rollout_batch(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                        const double* m0, const double* S0, int H, double* mH, double* SH, double* reward) {
    if (!ctx) return PILCO_E_SHAPE;
    if (B <= 0 || B > 64 || !policies || !m0 || !S0 || !mH || !SH || !reward || H < 0) return fail(ctx, PILCO_E_SHAPE, "rollout_batch: bad arguments");
    if (ctx->nranks != 1 || ctx->comm) return fail(ctx, PILCO_E_STATE, "rollout_batch: single rank only (shard OR batch)");
    for (int i = 0; i < B; ++i)
        if (policies[i].kind == PILCO_POLICY_RBF) return fail(ctx, PILCO_E_SHAPE, "rollout_batch: RbfController lanes are not supported (one policy GP slot per context)");
    HIPCHK(hipSetDevice(ctx->device));
    const Slot& s = ctx->slot[0];
    if (!s.factor_valid) return fail(ctx, PILCO_E_STATE, "rollout_batch: dynamics model has no current factorisation");
    const int E = s.E;
    std::vector<RolloutCall> rc((size_t)B);
    std::vector<pilco_ctx*> lane;
    LanesGuard lanes_guard{ctx};
    if (int r = rollout_lanes(ctx, B, lane, "rollout_batch")) return r;
    return run_lanes(
        ctx, lane, false,
        [&](int i) { return rollout_begin(lane[i], &policies[i], rewards, n_rewards, m0 + (size_t)i * E, S0 + (size_t)i * E * E, H, nullptr, rc[i]); },
        [&](int i) { return rollout_end(lane[i], rc[i], mH + (size_t)i * E, SH + (size_t)i * E * E, reward + i); });
}

int pilco_propagate(pilco_ctx* ctx, const pilco_policy* policy, const double* m_x, const double* s_x, double* M_x, double* S_x) {
    double r = 0.0;
    return pilco_rollout(ctx, policy, nullptr, 0, m_x, s_x, 1, M_x, S_x, &r, nullptr);
}

// Shapes: state_dim and control_dim are bounded SEPARATELY (each <= 32), so D = E + U may reach 64 here, twice what a rollout
// takes.  The link's code is sound for that (every misc[] slot is indexed by E or by U alone, the square buffers are carved
// with nm = D, squash_inplace keeps U^2 <= 1024 elements in 4 registers per thread), so 32 < D <= 64 IS supported -- as far as
// k_glue's buffers fit the 160 KB of LDS a workgroup can have (7 D^2 + 3 D + 256 doubles and the reward scratch: (20, 20)
// and (32, 8) fit, (32, 32) would need 275 KB).  A shape that does not fit is refused with PILCO_E_SHAPE before anything
// is copied or launched (tests/test_gpu_link_edges.py holds both answers).
int pilco_policy_action(pilco_ctx* ctx, const pilco_policy* policy, const double* m, const double* s_in, double* M, double* S, double* V) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!policy || !m || !s_in || !M || !S || !V) return fail(ctx, PILCO_E_SHAPE, "policy_action: null pointer");
    if (policy->kind != PILCO_POLICY_LINEAR && policy->kind != PILCO_POLICY_RBF) return fail(ctx, PILCO_E_SHAPE, "policy_action: policy kind must be LINEAR or RBF");
    HIPCHK(hipSetDevice(ctx->device));
    const int E = policy->state_dim, U = policy->control_dim;
    if (E <= 0 || U <= 0 || E > MAX_D || U > MAX_D) return fail(ctx, PILCO_E_SHAPE, "policy_action: bad dims");
    if (policy->kind == PILCO_POLICY_RBF) {
        Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
        if (!ps.factor_valid) return fail(ctx, PILCO_E_STATE, "policy_action: RBF policy slot has no current factorisation");
        if (ps.D != E || ps.E != U) return fail(ctx, PILCO_E_SHAPE, "policy_action: RBF policy GP must map state_dim -> control_dim");
        if (int r = build_work(ctx, ps)) return r;
        const size_t n_st = (size_t)E + E * E + U + (U + U * U + (size_t)E * U);
        ENSURE(ctx->state, n_st + 8);
        std::vector<double> h(n_st, 0.0);
        memcpy(&h[0], m, sizeof(double) * E);
        memcpy(&h[E], s_in, sizeof(double) * E * E);
        size_t off = (size_t)E + E * E;
        GlueArgs g{};
        g.E = E; g.D = E + U; g.U = U;
        g.m_x = ctx->state.p;
        g.s_x = ctx->state.p + E;
        for (int u = 0; u < U; ++u) h[off + u] = policy->max_action ? policy->max_action[u] : 1.0;
        g.maxact = ctx->state.p + off; off += U;
        g.act_out = ctx->state.p + off;
        g.pol_kind = PILCO_POLICY_RBF;
        g.squash = policy->squash;
        g.pwk = ps.wk;
        g.pvar = ps.var.p;
        g.flags = GF_RBF_POST | GF_POLICY;
        if (sizeof(double) * glue_lds_doubles_for(g) > GLUE_LDS_LIMIT) return fail(ctx, PILCO_E_SHAPE, "policy_action: state_dim + control_dim too large for the link's LDS");
        HIPCHK(hipMemcpyAsync(ctx->state.p, h.data(), sizeof(double) * n_st, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipMemcpyAsync(ps.wk.in_m, m, sizeof(double) * E, hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipMemcpyAsync(ps.wk.in_s, s_in, sizeof(double) * E * E, hipMemcpyHostToDevice, ctx->st));
        const MMModel pmd = model_of(ps);
        launch_mm_prep(ctx->st, pmd, ps.wk);
        launch_mm_pair(ctx->st, pmd, ps.wk, ctx->variant);
        launch_glue(ctx->st, g);
        std::vector<double> o((size_t)U + U * U + (size_t)E * U);
        HIPCHK(hipMemcpyAsync(o.data(), g.act_out, sizeof(double) * o.size(), hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        HIPCHK(hipGetLastError());
        memcpy(M, &o[0], sizeof(double) * U);
        memcpy(S, &o[U], sizeof(double) * U * U);
        memcpy(V, &o[(size_t)U + U * U], sizeof(double) * E * U);
        return PILCO_OK;
    }
    if (!policy->W || !policy->b) return fail(ctx, PILCO_E_SHAPE, "policy_action: linear policy needs W and b");
    if (glue_lds_bytes(E, E + U) > GLUE_LDS_LIMIT) return fail(ctx, PILCO_E_SHAPE, "policy_action: state_dim + control_dim too large for the link's LDS");
    const size_t n_state = (size_t)E + E * E + (size_t)U * E + 2 * U + (U + U * U + (size_t)E * U);
    ENSURE(ctx->state, n_state + 8);
    std::vector<double> h(n_state, 0.0);
    memcpy(&h[0], m, sizeof(double) * E);
    memcpy(&h[E], s_in, sizeof(double) * E * E);
    size_t off = (size_t)E + E * E;
    GlueArgs g{};
    g.E = E; g.D = E + U; g.U = U;
    g.m_x = ctx->state.p;
    g.s_x = g.m_x + E;
    memcpy(&h[off], policy->W, sizeof(double) * U * E);
    g.W = ctx->state.p + off; off += (size_t)U * E;
    memcpy(&h[off], policy->b, sizeof(double) * U);
    g.b = ctx->state.p + off; off += U;
    for (int u = 0; u < U; ++u) h[off + u] = policy->max_action ? policy->max_action[u] : 1.0;
    g.maxact = ctx->state.p + off; off += U;
    g.act_out = ctx->state.p + off;
    g.pol_kind = PILCO_POLICY_LINEAR;
    g.squash = policy->squash;
    g.flags = GF_POLICY;
    HIPCHK(hipMemcpyAsync(ctx->state.p, h.data(), sizeof(double) * n_state, hipMemcpyHostToDevice, ctx->st));
    launch_glue(ctx->st, g);
    std::vector<double> o((size_t)U + U * U + (size_t)E * U);
    HIPCHK(hipMemcpyAsync(o.data(), g.act_out, sizeof(double) * o.size(), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    memcpy(M, &o[0], sizeof(double) * U);
    memcpy(S, &o[U], sizeof(double) * U * U);
    memcpy(V, &o[(size_t)U + U * U], sizeof(double) * E * U);
    return PILCO_OK;
}

int pilco_reward_eval(pilco_ctx* ctx, const pilco_reward_term* rewards, int n_rewards, int state_dim, const double* m,
                      const double* s_in, double* muR, double* sR) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!rewards || n_rewards <= 0 || n_rewards > MAX_REWARD_TERMS || !m || !s_in || !muR || !sR || state_dim <= 0 || state_dim > MAX_D)
        return fail(ctx, PILCO_E_SHAPE, "reward_eval: bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    const int E = state_dim;
    const size_t n = (size_t)E + E * E + (size_t)n_rewards * (2 * E * E + E) + 2;
    ENSURE(ctx->state, n + 8);
    std::vector<double> h(n, 0.0);
    memcpy(&h[0], m, sizeof(double) * E);
    memcpy(&h[E], s_in, sizeof(double) * E * E);
    size_t off = (size_t)E + E * E;
    GlueArgs g{};
    g.E = E; g.D = E; g.U = 0;
    g.m_x = ctx->state.p;
    g.s_x = ctx->state.p + E;
    g.n_rewards = n_rewards;
    if (int r = stage_rewards(ctx, rewards, n_rewards, E, h, off, ctx->state.p, g.rw)) return r;
    if (h.size() < off + 2) h.resize(off + 2, 0.0);
    if (h.size() + 8 > ctx->state.cap) return fail(ctx, PILCO_E_ALLOC, "reward_eval: staging overflow");
    g.rew_out = ctx->state.p + off;
    g.flags = 0;  // workgroup 0 idles; workgroup 1 evaluates mean and variance
    HIPCHK(hipMemcpyAsync(ctx->state.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->st));
    launch_glue(ctx->st, g, true);
    double o[2];
    HIPCHK(hipMemcpyAsync(o, g.rew_out, sizeof(double) * 2, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    *muR = o[0];
    *sR = o[1];
    return PILCO_OK;
}

int pilco_rollout_timed(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                        const double* m0, const double* S0, int H, int reps, double* mH, double* SH, double* reward,
                        float* ms_total, float* ms_pair, int* n_pair_launches) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!m0 || !S0 || !mH || !SH || !reward || H < 0 || reps <= 0 || !ms_total) return fail(ctx, PILCO_E_SHAPE, "rollout_timed: bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    RolloutPlan plan;
    if (int r = setup_rollout(ctx, policy, rewards, n_rewards, H, false, plan)) return r;
    const int E = plan.E;
    ENSURE(ctx->selftest, (size_t)E + E * E + 256);
    double* init = ctx->selftest.p + 256;  // device copy of (m0, S0) so that the timed region has no host traffic
    HIPCHK(hipMemcpyAsync(init, m0, sizeof(double) * E, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(init + E, S0, sizeof(double) * E * E, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    auto upload = [&]() -> int {
        HIPCHK(hipMemcpyAsync(plan.st[0], init, sizeof(double) * (E + E * E), hipMemcpyDeviceToDevice, ctx->st));
        return PILCO_OK;
    };
    if (int r = run_rollout(ctx, plan, H, upload)) return r;   // the graph exists before the timed region
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipEventRecord(ctx->ev0, ctx->st));
    for (int rep = 0; rep < reps; ++rep)
        if (int r = run_rollout(ctx, plan, H, upload)) return r;
    HIPCHK(hipEventRecord(ctx->ev1, ctx->st));
    HIPCHK(hipEventSynchronize(ctx->ev1));
    HIPCHK(hipEventElapsedTime(ms_total, ctx->ev0, ctx->ev1));
    if (ms_pair) {
        // second pass with an event pair around every pair-kernel launch (perturbs the total, so timed separately)
        if (int r = upload()) return r;
        if (int r = plan_route(ctx, plan, H, true)) return r;
        if (int r = enqueue_rollout_steps(ctx, plan, H)) return r;
        HIPCHK(hipStreamSynchronize(ctx->st));
        float tot = 0.f;
        int cnt = 0;
        if (ctx->slot[0].wk.PL > 0)
            for (int t = 0; t < H; ++t) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, ctx->pair_events[2 * t], ctx->pair_events[2 * t + 1]));
                tot += ms;
                ++cnt;
            }
        *ms_pair = tot;
        if (n_pair_launches) *n_pair_launches = cnt;
    }
    HIPCHK(hipMemcpyAsync(mH, plan.st[H & 1], sizeof(double) * E, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(SH, plan.st[H & 1] + E, sizeof(double) * E * E, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(reward, plan.g.reward, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

// pilco_rollout that also records, for every step t < H, the joint Gaussian (m, s, s1) handed to
// the dynamics GP and its outputs (M, S, V): tape [H][tape_rec(D, E).size] (grad_layout.h).  The reverse
// sweep of the policy gradient replays these records (pilco_amd/adjoint.py).
int pilco_rollout_tape(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                       const double* m0, const double* S0, int H, double* mH, double* SH, double* reward, double* traj,
                       double* tape) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!m0 || !S0 || !mH || !SH || !reward || !tape || H < 0) return fail(ctx, PILCO_E_SHAPE, "rollout_tape: bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    RolloutPlan plan;
    if (int r = setup_rollout(ctx, policy, rewards, n_rewards, H, traj != nullptr, plan)) return r;
    const int E = plan.E;
    const size_t TS = tape_rec(plan.D, E).size;
    ENSURE(ctx->tape, std::max<size_t>(1, (size_t)H * TS));
    plan.g.tape = ctx->tape.p;
    if (int r = rollout_run(ctx, plan, H, m0, S0)) return r;   // replayed as a hipGraph like pilco_rollout (the tape pointer is part of the graph key)
    HIPCHK(hipMemcpyAsync(mH, plan.st[H & 1], sizeof(double) * E, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(SH, plan.st[H & 1] + E, sizeof(double) * E * E, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(reward, plan.g.reward, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    if (traj) HIPCHK(hipMemcpyAsync(traj, ctx->traj.p, sizeof(double) * (size_t)(H + 1) * (E + E * E), hipMemcpyDeviceToHost, ctx->st));
    if (H > 0) HIPCHK(hipMemcpyAsync(tape, ctx->tape.p, sizeof(double) * (size_t)H * TS, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

}  // extern "C"

// test aid (pilco_debug_geometry): the step geometry of the dynamics slot's current workspace
int pilco_debug_geometry(pilco_ctx* ctx, int* out, int n) {
    if (!ctx || !out || n <= 0) return PILCO_E_SHAPE;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    if (!s.wk_valid) return fail(ctx, PILCO_E_STATE, "debug_geometry: the dynamics slot has no step workspace (run a rollout first)");
    const MMWork& wk = s.wk;
    const int sk_cap = (ctx->variant == 0 && wk.PL > 0) ? mm_pair_sk_capacity(wk.KP, wk.vsep != 0, false) : 0;
    const int v[PILCO_GEOMETRY_WORDS] = {s.npad, wk.PL, wk.EL, wk.NCH, wk.NCHM, wk.NT, wk.sk_waves, wk.sk_total, wk.sk_nd, wk.sk_maxw,
                                         sk_cap, device_cus_of(ctx->device), small_col_splits(ctx, s, true), small_col_splits(ctx, s, false)};
    for (int i = 0; i < std::min(n, (int)PILCO_GEOMETRY_WORDS); ++i) out[i] = v[i];
    return PILCO_OK;
}

// test aid (pilco_debug_sk_cut_probe): the dynamics slot's stream-K cut as the device functions of the pair kernel give it
int pilco_debug_sk_cut_probe(pilco_ctx* ctx, int* out, int n) {
    if (!ctx || !out || n < PILCO_SK_PROBE_HEAD) return PILCO_E_SHAPE;
    HIPCHK(hipSetDevice(ctx->device));
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    if (!s.wk_valid || s.wk.sk_waves <= 0) return fail(ctx, PILCO_E_STATE, "debug_sk_cut_probe: the dynamics slot has no stream-K cut (run a rollout with the stream-K pair kernel first)");
    const MMWork& wk = s.wk;
    const size_t words = (size_t)wk.sk_waves * PILCO_SK_PROBE_WORDS;
    if ((size_t)n < PILCO_SK_PROBE_HEAD + words) return fail(ctx, PILCO_E_SHAPE, "debug_sk_cut_probe: the buffer is too small");
    const int head[PILCO_SK_PROBE_HEAD] = {wk.sk_waves, wk.sk_nd, wk.sk_tdiag, wk.sk_toff, wk.sk_total, wk.sk_ud, wk.sk_uo, wk.PL, (int)wk.skm.fast, s.npad};
    for (int i = 0; i < PILCO_SK_PROBE_HEAD; ++i) out[i] = head[i];
    int* dev = nullptr;
    HIPCHK(hipMalloc((void**)&dev, sizeof(int) * words));
    launch_sk_cut_probe(ctx->st, model_of(s), wk, dev);
    hipError_t e = hipMemcpyAsync(out + PILCO_SK_PROBE_HEAD, dev, sizeof(int) * words, hipMemcpyDeviceToHost, ctx->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    (void)hipFree(dev);
    HIPCHK(e);
    return PILCO_OK;
}
