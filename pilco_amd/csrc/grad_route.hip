// The route of a value-and-gradient rollout (pilco_rollout_grad*; DESIGN.md section 9, docs/gradient_routes.md): the plan
// (plan_grad), the forward half along each route (grad_forward), the exchange of the ranks' Jacobian records and the device
// chain's finish.  Host code only: the steps themselves are the rollout's (rollout.hip, with RolloutPlan::jrec set), the
// records' kernels are bwd.hip's, the chain's rev.hip's; the host chains are grad.hip's.
#include "ctx.h"
#include "lds_layout.h"

namespace {

// What every step of the Jacobian tape keeps in buffers of its own until the batched finish (nothing on the chain waits
// for a buffer), in doubles: at C2u 29 MB per step -- HBM is 288 GB
struct JacBufs {
    size_t rowmom, cpart, head, part;
};
JacBufs jac_bufs(const Slot& s) {
    const int P = s.wk.PL;   // (EL: owned outputs = diagonal pairs held here, E on one rank)
    return {mm_jac_rowmom_size(s.npad, P), mm_jac_cpart_size(s.npad, P, s.wk.EL), mm_jac_head_size(s.D, s.E, P), mm_jac_part_size(s.D, s.E, P, s.npad)};
}

// The sums, moments and records of steps [t0, t1) in two launches behind the forward chain
void jac_finish_range(pilco_ctx* ctx, const RolloutPlan& plan, int t0, int t1, const RevLocalArgs* rl = nullptr) {
    Slot& s = ctx->slot[0];
    const JacBufs jb = jac_bufs(s);
    const size_t TS = tape_rec(plan.D, plan.E).size, o = (size_t)t0;
    launch_mm_jac_finish(ctx->st, model_of(s), s.wk, t1 - t0, s.jac_rowmom.p + o * jb.rowmom, s.jac_cpart.p + o * jb.cpart, s.jac_head.p + o * jb.head,
                         s.jac_part.p + o * jb.part, plan.g.tape + o * TS, TS, plan.jrec + o * plan.jstride,
                         s.wk.NCH * plan.route.ncs, rl);   // (the small step's chunks per pair, or 0)
}

// The forward half common to the routes with Jacobian records: pilco_rollout_tape with every dynamics step run as the
// reverse sweep (launch_mm_sweep), so that the step's value and what its records are made from come out of ONE O(N^2) pass.
// The pinned area (pin_doubles) starts with the trajectory, the tape and the records' place; direct: k_mm_jac_fin writes
// the records straight into it (device-visible) -- on one rank their 4.3 MB cross PCIe while the kernel runs instead of as
// four copies that hold the stream between the chunks of the finish.
int jtape_run(pilco_ctx* ctx, GradCall& gc, const double* m0, const double* S0, size_t pin_doubles, bool direct) {
    Slot& s = ctx->slot[0];
    RolloutPlan& plan = gc.plan;
    const int H = gc.H, E = plan.E, D = plan.D, P = s.wk.PL;
    const size_t Hn = (size_t)std::max(H, 1), TS = tape_rec(D, E).size, JS = mm_jac_rec_size(D, E, P);
    const JacBufs jb = jac_bufs(s);
    ENSURE(s.jac_rowmom, Hn * jb.rowmom);
    ENSURE(s.jac_cpart, Hn * jb.cpart);
    ENSURE(s.jac_head, Hn * jb.head);
    ENSURE(s.jac_part, Hn * jb.part);
    ENSURE(s.jac_np, (size_t)2 * std::max(P, 1) * mm_jac_nt(s.npad, s.wk.P, s.wk.KP));
    ENSURE(ctx->tape, std::max<size_t>(1, (size_t)H * TS));
    ENSURE(ctx->jrec, std::max<size_t>(1, (size_t)H * JS));
    if (ctx->jpin_cap < pin_doubles) {
        if (ctx->jpin) (void)hipHostFree(ctx->jpin);
        ctx->jpin = nullptr;
        ctx->jpin_cap = 0;
        HIPCHK(hipHostMalloc((void**)&ctx->jpin, sizeof(double) * pin_doubles, hipHostMallocDefault));
        ctx->jpin_cap = pin_doubles;
    }
    plan.g.tape = ctx->tape.p;
    plan.jrec = direct ? ctx->jpin + (size_t)(H + 1) * (E + (size_t)E * E) + (size_t)H * TS : ctx->jrec.p;
    plan.jstride = JS;
    return rollout_run(ctx, plan, H, m0, S0);   // (plan.route: the steps' layout the finish reads)
}

// Several ranks: every rank sweeps ITS pairs (k_mm_bwd_pair is per-pair independent; the mean-part records of all E outputs
// are cheap and computed on every rank with pairs), the per-step exchange of the forward chain is the sharded rollout's own,
// and after the batched finish the records are all-gathered ONCE -- records, not sums: the chains add them in the
// single-rank order.  This rank's records of every step are compacted into its block (JacGather) and the W blocks land
//   host_all == nullptr: in ctx->jgath [W][gblk] on the device (the device chain reads them there),
//   host_all != nullptr: in host_all [W][gblk], and the call returns when they are there.
// xch = GRAD_XCH_COMM: ncclAllGather (and one download); GRAD_XCH_GROUP (contexts of one process, pilco_rollout_grad_group):
// every rank takes the peers' blocks itself between two host barriers.
int exchange_records(pilco_ctx* ctx, GradExchange xch, const RolloutPlan& plan, const JacGather& gg, int H, double* host_all) {
    const int W = gg.W, P = ctx->slot[0].wk.PL;
    const RevDims d = rev_dims(plan.E, plan.U, plan.D);
    const size_t gblk = gg.gblk, JS = plan.jstride;
    ENSURE(ctx->jgath, (size_t)(W + 1) * gblk);
    double* own = ctx->jgath.p + (size_t)W * gblk;
    HIPCHK(hipMemsetAsync(own, 0, sizeof(double) * gblk, ctx->st));
    if (P > 0) {   // [H][PLcap pair records | E output records]; a rank without pairs ran no sweep at all
        HIPCHK(hipMemcpy2DAsync(own, sizeof(double) * gg.gstep, ctx->jrec.p, sizeof(double) * JS, sizeof(double) * P * d.recp, (size_t)H,
                                hipMemcpyDeviceToDevice, ctx->st));
        HIPCHK(hipMemcpy2DAsync(own + gg.out_off, sizeof(double) * gg.gstep, ctx->jrec.p + (size_t)P * d.recp, sizeof(double) * JS,
                                sizeof(double) * plan.E * d.reco, (size_t)H, hipMemcpyDeviceToDevice, ctx->st));
    }
    if (xch == GRAD_XCH_COMM) {
        ncclResult_t r = ncclAllGather(own, ctx->jgath.p, gblk, ncclDouble, ctx->comm, ctx->st);
        if (r != ncclSuccess) return fail(ctx, PILCO_E_RCCL, std::string("ncclAllGather(jacobian records): ") + ncclGetErrorString(r));
        if (host_all) {
            HIPCHK(hipMemcpyAsync(host_all, ctx->jgath.p, sizeof(double) * (size_t)W * gblk, hipMemcpyDeviceToHost, ctx->st));
            HIPCHK(hipStreamSynchronize(ctx->st));
        }
        return PILCO_OK;
    }
    HIPCHK(hipStreamSynchronize(ctx->st));
    std::shared_ptr<PeerGroup> grp = ctx->group;
    if (!grp->arrive_and_wait()) return fail(ctx, PILCO_E_STATE, "rollout_grad: another rank of the group failed");
    // The peers may reuse their blocks after the second barrier, so every copy must have FINISHED in front of it.  To the host a
    // blocking hipMemcpy does that.  Device to device it does not: such a hipMemcpy is ordered on the null stream only and
    // need not have finished when it returns -- the chain, on a non-blocking stream, read blocks that were still being copied
    // once in ten runs.  Those copies therefore go on THIS context's stream and are waited for before the barrier.
    for (int j = 0; j < W; ++j) {
        const double* theirs = grp->ctxs[j]->jgath.p + (size_t)W * gblk;
        if (host_all) HIPCHK(hipMemcpy(host_all + (size_t)j * gblk, theirs, sizeof(double) * gblk, hipMemcpyDeviceToHost));
        else HIPCHK(hipMemcpyAsync(ctx->jgath.p + (size_t)j * gblk, theirs, sizeof(double) * gblk, hipMemcpyDeviceToDevice, ctx->st));
    }
    if (!host_all) HIPCHK(hipStreamSynchronize(ctx->st));
    if (!grp->arrive_and_wait()) return fail(ctx, PILCO_E_STATE, "rollout_grad: another rank of the group failed");
    return PILCO_OK;
}

// GRAD_CHAIN_DEVICE: the records stay on the device and the reverse chain runs there (rev.hip); nothing but the reward, the
// gradient -- and, for a caller with cotangent seeds, the trajectory -- crosses to the host.  Enqueues the forward half, the
// records' finish, the exchange and -- without seeds -- the chain itself, and returns without waiting (grad_device_finish).
// Pinned area: trajectory | 8 | seeds | the chain's output vector.
int forward_device(pilco_ctx* ctx, GradCall& gc, const double* m0, const double* S0) {
    RolloutPlan& plan = gc.plan;
    const int H = gc.H, E = plan.E, U = plan.U, D = plan.D, W = ctx->nranks;
    const size_t NTJ = (size_t)(H + 1) * (E + (size_t)E * E);
    const RevOut ro = rev_out(E, U);
    gc.n_seeds = NTJ;
    if (int r = jtape_run(ctx, gc, m0, S0, NTJ + 8 + gc.n_seeds + ro.size + 8, false)) return r;
    gc.traj = ctx->jpin;   // (seeds only; valid once jwait_ev[0] has passed)
    gc.h_seeds = gc.traj + NTJ + 8;
    if (!ctx->jwait_ev[0]) HIPCHK(hipEventCreateWithFlags(&ctx->jwait_ev[0], hipEventDisableTiming));
    if (gc.route.seeds) {
        HIPCHK(hipMemcpyAsync(gc.traj, ctx->traj.p, sizeof(double) * NTJ, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipEventRecord(ctx->jwait_ev[0], ctx->st));   // the host turns the trajectory into seeds while the finish runs
    }
    const RevDims d = rev_dims(E, U, D);
    RevArgs& ra = gc.ra;
    ra = RevArgs{};
    ra.E = E; ra.U = U; ra.D = D; ra.H = H; ra.P = d.P;
    ra.W = 1; ra.gblk = 0; ra.gstep = (long)plan.jstride; ra.out_off = (long)ctx->slot[0].wk.PL * d.recp;
    ra.jrec = ctx->jrec.p;
    ENSURE(ctx->revloc, std::max<size_t>(1, (size_t)H * rev_loc_doubles(E, U)));
    const RevLocalArgs rl = rev_local_args(plan.g.n_rewards, plan.g.rw, E, U, ctx->traj.p, plan.g.W, plan.g.b, plan.g.maxact, ctx->revloc.p);
    if (H > 0) jac_finish_range(ctx, plan, 0, H, &rl);   // (the trajectory-only quantities of the chain ride in its last launch)
    if (gc.route.exchange != GRAD_XCH_NONE) {   // the chain reads every rank's records where the all-gather leaves them
        const JacGather gg = jac_gather(D, E, W, H);
        if (int r = exchange_records(ctx, gc.route.exchange, plan, gg, H, nullptr)) return r;
        ra.jrec = ctx->jgath.p;
        ra.W = W; ra.gblk = (long)gg.gblk; ra.gstep = (long)gg.gstep; ra.out_off = (long)gg.out_off;
    }
    ra.traj = ctx->traj.p;
    ra.tape = ctx->tape.p;
    ra.TS = (long)tape_rec(D, E).size;
    ra.loc = ctx->revloc.p;
    ENSURE(ctx->revmat, std::max<size_t>(1, (size_t)H * rev_mat_doubles(E, U, D)));
    ra.amat = ctx->revmat.p;
    ra.reward_dev = plan.g.reward;
    ra.Wp = plan.g.W;
    ra.out = gc.h_seeds + gc.n_seeds;
    gc.h_out = ra.out;
    gc.reward = ra.out + ro.reward;   // (valid with h_out)
    if (!gc.route.seeds) launch_rev_chain(ctx->st, ra);
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

// The host chain over the records, both exchanges: the forward half, where its results land in the pinned area --
// trajectory | tape | records [H][JS] | reward (8) | `extra` doubles -- and the downloads of the reward and the trajectory.
int host_forward(pilco_ctx* ctx, GradCall& gc, const double* m0, const double* S0, size_t JS, size_t extra, bool direct) {
    const int H = gc.H, E = gc.plan.E;
    const size_t NTJ = (size_t)(H + 1) * (E + (size_t)E * E), TS = tape_rec(gc.plan.D, E).size;
    if (int r = jtape_run(ctx, gc, m0, S0, NTJ + (size_t)H * TS + (size_t)H * JS + 8 + extra, direct)) return r;
    gc.traj = ctx->jpin;
    gc.tape = gc.traj + NTJ;
    gc.jrec = gc.tape + (size_t)H * TS;   // (direct: = plan.jrec, written by the finish itself)
    gc.reward = gc.jrec + (size_t)H * JS;
    gc.JS = JS;
    HIPCHK(hipMemcpyAsync(gc.reward, gc.plan.g.reward, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipMemcpyAsync(gc.traj, ctx->traj.p, sizeof(double) * NTJ, hipMemcpyDeviceToHost, ctx->st));
    return PILCO_OK;
}

// GRAD_CHAIN_RECORDS on one rank (and any rollout without steps): enqueues everything and returns without waiting.  The
// records come down in chunks, LAST steps first, an event behind each: the host's reverse sweep starts on the last steps
// while the earlier ones are still on their way (grad_wait).
int forward_one_rank(pilco_ctx* ctx, GradCall& gc, const double* m0, const double* S0) {
    const int H = gc.H;
    if (int r = host_forward(ctx, gc, m0, S0, mm_jac_rec_size(gc.plan.D, gc.plan.E, ctx->slot[0].wk.PL), 0, true)) return r;
    gc.wait_from = H;
    if (H <= 0) return PILCO_OK;
    HIPCHK(hipMemcpyAsync(gc.tape, ctx->tape.p, sizeof(double) * (size_t)H * tape_rec(gc.plan.D, gc.plan.E).size, hipMemcpyDeviceToHost, ctx->st));
    // chunks in the order the reverse sweep consumes them, SHRINKING towards step 0.  Measured at C2u: the device finishes
    // a step's records in ~11 us, the host sweeps one in ~9 us, and every chunk costs both sides a fixed ~40-60 us (two
    // launches, an event wait) -- four chunks of 16/12/8/4 fortieths: 6.03 -> 5.97 ms; six chunks (8,8,8,8,4,4): 6.14 ms;
    // finishing the early chunks on a second stream WHILE the chain runs: 6.09 ms with one fork, 7.4 ms with three (the
    // chain's kernels lose what the finish gains)
    static const int parts[4] = {16, 12, 8, 4};   // fortieths of H
    const int nch = std::min(H, 4);
    int t1 = H, used = 0;
    for (int k = 0; k < nch; ++k) {
        used += parts[k];
        const int t0 = (k == nch - 1) ? 0 : std::min(t1 - 1, std::max(0, H - (int)((long)used * H / 40)));   // steps [t0, t1), never empty
        jac_finish_range(ctx, gc.plan, t0, t1);
        if (!ctx->jwait_ev[k]) HIPCHK(hipEventCreateWithFlags(&ctx->jwait_ev[k], hipEventDisableTiming));
        HIPCHK(hipEventRecord(ctx->jwait_ev[k], ctx->st));
        gc.wait_t0[k] = t0;
        t1 = t0;
    }
    gc.wait_n = nch;
    return PILCO_OK;
}

// GRAD_CHAIN_RECORDS on several ranks: the finish of all steps, the exchange of the records into host memory (behind the
// reward: every rank's block), and the assembly of the GLOBAL records [P pair records | E output records] per step that
// the host chain reads.  Returns with everything on the host.
int forward_sharded(pilco_ctx* ctx, GradCall& gc, const double* m0, const double* S0, double* reward) {
    const int H = gc.H, E = gc.plan.E, D = gc.plan.D, W = ctx->nranks;
    const RevDims d = rev_dims(E, gc.plan.U, D);
    const JacGather gg = jac_gather(D, E, W, H);
    if (int r = host_forward(ctx, gc, m0, S0, gg.JSg, (size_t)W * gg.gblk, false)) return r;
    const double* h_all = gc.reward + 8;
    jac_finish_range(ctx, gc.plan, 0, H);
    HIPCHK(hipMemcpyAsync(gc.tape, ctx->tape.p, sizeof(double) * (size_t)H * tape_rec(D, E).size, hipMemcpyDeviceToHost, ctx->st));
    if (int r = exchange_records(ctx, gc.route.exchange, gc.plan, gg, H, gc.reward + 8)) return r;
    HIPCHK(hipGetLastError());
    for (int t = 0; t < H; ++t) {
        double* dst = gc.jrec + (size_t)t * gg.JSg;
        for (int kk = 0; kk < gg.P; ++kk)
            memcpy(dst + (size_t)kk * d.recp, h_all + (size_t)(kk % W) * gg.gblk + (size_t)t * gg.gstep + (size_t)(kk / W) * d.recp, sizeof(double) * d.recp);
        memcpy(dst + (size_t)gg.P * d.recp, h_all + (size_t)t * gg.gstep + gg.out_off, sizeof(double) * E * d.reco);   // rank 0's
    }
    *reward = *gc.reward;
    gc.arrived = true;
    gc.tm1 = std::chrono::steady_clock::now();
    return PILCO_OK;
}

// GRAD_CHAIN_ADJOINT: the plain tape rollout, run to completion (nothing of it overlaps with other lanes); the O(N^2)
// adjoint of every step runs on the device during the host chain (pilco_gp_predict_vjp, the forward path's D <= 32).
int forward_plain_tape(pilco_ctx* ctx, GradCall& gc, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* m0,
                       const double* S0, double* reward) {
    const int H = gc.H, E = policy->state_dim, D = E + policy->control_dim;
    std::vector<double> mH(E), SH((size_t)E * E);
    gc.traj_v.resize((size_t)(H + 1) * (E + E * E));
    gc.tape_v.resize(std::max<size_t>(1, (size_t)H * tape_rec(D, E).size));
    if (int r = pilco_rollout_tape(ctx, policy, rewards, n_rewards, m0, S0, H, mH.data(), SH.data(), reward, gc.traj_v.data(), gc.tape_v.data()))
        return r;
    gc.traj = gc.traj_v.data();
    gc.tape = gc.tape_v.data();
    gc.arrived = true;
    gc.tm1 = std::chrono::steady_clock::now();
    return PILCO_OK;
}

}  // namespace

// Decide the route of a value-and-gradient rollout of H steps before anything of it is enqueued, and set the rollout up
// on this context (gc.plan; not for the plain tape, which goes through pilco_rollout_tape).  linear: a LinearController,
// whose reverse chain can run on the device.  decided: the context is a further lane of a batch call -- same model, same
// horizon, same kind of policy -- and takes lane 0's route; only the rollout is set up on it.
int plan_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, int H, bool linear, bool seeds,
              const GradRoute* decided, GradCall& gc) {
    gc.tm0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    gc.H = H;
    GradRoute& gr = gc.route;
    if (decided) {
        gr = *decided;
        return gr.chain == GRAD_CHAIN_ADJOINT ? PILCO_OK : setup_rollout(ctx, policy, rewards, n_rewards, H, true, gc.plan);
    }
    gr = GradRoute{};
    gr.seeds = seeds;
    // PILCO_GRAD_MODE=0 / pilco_set_grad_mode(ctx, 0): plain tape, and the O(N^2) adjoint of every step on the device again --
    // the two agree to rounding
    gr.chain = GRAD_CHAIN_ADJOINT;
    const bool sharded = ctx->nranks != 1 || ctx->comm;
    // the plain tape's per-step adjoint (pilco_gp_predict_vjp) is single rank only: a sharded call that would take it is refused
    // here, on every rank alike and before its collective forward tape is enqueued
    auto adjoint = [&](const char* why) {
        return sharded ? fail(ctx, PILCO_E_STATE, std::string("rollout_grad: ") + why + " takes the plain tape, which is single rank only") : PILCO_OK;
    };
    if (sharded && !ctx->comm && !ctx->group)
        return fail(ctx, PILCO_E_STATE, "rollout_grad: a sharded context needs a communicator (pilco_comm_init) or pilco_rollout_grad_group");
    if (ctx->grad_mode == 0) return adjoint("grad_mode 0");
    if (int r = setup_rollout(ctx, policy, rewards, n_rewards, H, true, gc.plan)) return r;
    const int E = gc.plan.E, U = gc.plan.U, D = gc.plan.D;
    if (D > 14) return adjoint("an input width D > 14");   // third-moment records and their LDS working set are sized for D <= 14
    // a rollout whose per-step buffers would need more than PILCO_JAC_GB (default 32) takes the plain tape too
    const JacBufs jb = jac_bufs(ctx->slot[0]);
    double cap_gb = 32.0;
    if (const char* ev = getenv("PILCO_JAC_GB")) cap_gb = atof(ev);
    if ((double)(jb.rowmom + jb.cpart + jb.head + jb.part) * 8.0 * (double)std::max(H, 1) > cap_gb * 1e9) return adjoint("a rollout over PILCO_JAC_GB");
    gr.chain = GRAD_CHAIN_RECORDS;
    if (sharded && H > 0) gr.exchange = ctx->comm ? GRAD_XCH_COMM : GRAD_XCH_GROUP;   // (no steps: no records to exchange)
    if (linear && ctx->dev_chain && rev_chain_supported(E, U, D)) {
        gr.chain = GRAD_CHAIN_DEVICE;
        gr.rev_lds = (int)rev_step_lds_bytes(E, U, D);
    }
    return PILCO_OK;
}

// The forward half along gc.route.  The device chain and -- with defer, one rank -- the host chain over the records return
// without waiting for anything (the lanes of a batch call are all enqueued before the first wait); otherwise the forward
// half's results are on the host and *reward is set.
int grad_forward(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* m0, const double* S0,
                 double* reward, bool defer, GradCall& gc) {
    switch (gc.route.chain) {
        case GRAD_CHAIN_DEVICE: return forward_device(ctx, gc, m0, S0);
        case GRAD_CHAIN_ADJOINT: return forward_plain_tape(ctx, gc, policy, rewards, n_rewards, m0, S0, reward);
        case GRAD_CHAIN_RECORDS: break;
    }
    if (gc.route.exchange != GRAD_XCH_NONE) return forward_sharded(ctx, gc, m0, S0, reward);
    if (int r = forward_one_rank(ctx, gc, m0, S0)) return r;
    if (defer && gc.H > 0) return PILCO_OK;   // a lane of a batch: the caller waits when it gets to this lane (grad_arrive)
    if (int r = grad_arrive(ctx, gc, reward)) return r;
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

int grad_arrive(pilco_ctx* ctx, GradCall& gc, double* reward) {
    if (gc.arrived) return PILCO_OK;
    if (gc.H > 0) {   // the reward, the trajectory, the tape and the last chunk of records
        if (int r = grad_wait(ctx, gc, gc.H - 1)) return r;
    } else {
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    *reward = *gc.reward;
    gc.arrived = true;
    gc.tm1 = std::chrono::steady_clock::now();
    return PILCO_OK;
}

// Block until the records of step t (and everything enqueued before them) are on the host.
int grad_wait(pilco_ctx* ctx, GradCall& gc, int t) {
    while (t < gc.wait_from && gc.wait_next < gc.wait_n) {
        const int k = gc.wait_next++;
        static const bool timing = getenv("PILCO_GRAD_TIMING") != nullptr;   // developer aid: how long the host waited for chunk k
        const auto w0 = std::chrono::steady_clock::now();
        HIPCHK(hipEventSynchronize(ctx->jwait_ev[k]));
        if (timing)
            fprintf(stderr, "[pilco grad] chunk %d (steps >= %d): waited %.3f ms (asked for step %d)\n", k, gc.wait_t0[k],
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count(), t);
        gc.wait_from = gc.wait_t0[k];
    }
    return PILCO_OK;
}

// Device chain, second half: with seeds, wait for the trajectory, let the caller turn it into cotangent seeds, upload them
// and launch the chain; then wait for the chain's output vector and hand the reward and the gradient out.
int grad_device_finish(pilco_ctx* ctx, GradCall& gc, pilco_seed_fn seed_fn, void* seed_user, double* reward, double* dW, double* db) {
    grad_route_record(ctx, gc.route);
    HIPCHK(hipSetDevice(ctx->device));
    const int E = gc.ra.E, U = gc.ra.U;
    if (gc.route.seeds) {
        HIPCHK(hipEventSynchronize(ctx->jwait_ev[0]));
        std::fill(gc.h_seeds, gc.h_seeds + gc.n_seeds, 0.0);
        seed_fn(seed_user, gc.H, E, gc.traj, gc.h_seeds);
        for (size_t q = 0; q < gc.n_seeds; ++q)
            if (!std::isfinite(gc.h_seeds[q])) {
                (void)hipStreamSynchronize(ctx->st);
                return fail(ctx, PILCO_E_SHAPE, "rollout_grad: the seed callback returned a non-finite cotangent");
            }
        ENSURE(ctx->revseeds, gc.n_seeds);
        HIPCHK(hipMemcpyAsync(ctx->revseeds.p, gc.h_seeds, sizeof(double) * gc.n_seeds, hipMemcpyHostToDevice, ctx->st));
        gc.ra.seeds = ctx->revseeds.p;
        launch_rev_chain(ctx->st, gc.ra);
    }
    HIPCHK(hipStreamSynchronize(ctx->st));
    HIPCHK(hipGetLastError());
    const RevOut ro = rev_out(E, U);
    if (gc.h_out[ro.status] != 0.0) return fail(ctx, PILCO_E_NOT_PD, "rollout_grad: singular s + Lambda^2 or I + Lambda s");
    *reward = *gc.reward;
    memcpy(dW, gc.h_out + ro.dW, sizeof(double) * (size_t)U * E);
    memcpy(db, gc.h_out + ro.db, sizeof(double) * (size_t)U);
    return PILCO_OK;
}

// The gradient words of the route record (pilco_debug_last_route), written when the chain's finish begins; the step's words
// and ROUTE_TAPE are the forward rollout's (plan_route).
void grad_route_record(pilco_ctx* ctx, const GradRoute& route) {
    ctx->route[ROUTE_ENTRY] = 2;
    ctx->route[ROUTE_CHAIN] = route.chain == GRAD_CHAIN_DEVICE ? 1 : 2;
    ctx->route[ROUTE_REV_LDS] = route.rev_lds;
    ctx->route[ROUTE_EXCHANGE] = route.exchange == GRAD_XCH_COMM ? 1 : route.exchange == GRAD_XCH_GROUP ? 2 : 0;
}
