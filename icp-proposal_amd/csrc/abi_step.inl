// abi_step.inl — part of icp_abi.hip (one translation unit; included there, in order).
// the merged step (five launches): what its entry points share (the poll of a pinned flag, the argument checks, launch 5's arguments over
// a result block), fronts and speculative decompositions, icp_chain_step_prelaunch / _prelaunch2, and icp_chain_step as a sequence of
// phases over one ChainStep
namespace {

// (the wide step: abi_wide.inl)
bool wide_chain_covered(icp_evaluator* e, int n_props, icp_proposal* const* props, int generator, const double* theta_cur,
                        const double* theta_prop_in);

// posteriors the regression launch being prepared will carry over all its chains (set by the batched issuers around their per-chain
// preparation; 1 for a lone chain): decides regression_fold
thread_local int tl_regression_posteriors = 1;

// Results and their completion flag are written into pinned memory by the kernels: the host polls the flag (≈ 4 µs less than a stream
// synchronisation), looking at the clock once in 65,536 spins.  -> false: the flag has not shown `seq` within `limit` — the caller
// synchronises its streams and lets them report what went wrong.
bool await_host_flag(volatile int* flag, int seq, std::chrono::seconds limit) {
  const auto t_start = std::chrono::steady_clock::now();
  long spins = 0;
  while (*flag != seq) {
    if ((++spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t_start > limit) return *flag == seq;
  }
  return true;
}

// The argument checks of a step, shared by icp_chain_step, the pre-launch (either key) and every chain of icp_chain_step_batched_issue.
// key: z (generator >= 0) or the proposed state.  The order decides which status a list with several faults gets; the null checks and
// the bound on n_props are the entry points' own, ahead of this.
void check_step_args(const icp_ctx& c, int n_props, icp_proposal* const* props, int generator, const double* theta_cur, const double* key) {
  require(generator < n_props, "generator index out of range");
  require(generator < 0 || key, "z is null");
  for (int i = 0; i < n_props; ++i) require(props[i] && props[i]->ctx == &c, "proposal belongs to another context");
  check_theta_finite(&c, theta_cur);
  if (generator < 0) check_theta_finite(&c, key);
  else
    for (int j = 0; j < c.r; ++j)
      if (!std::isfinite(key[j])) fail(ICP_ERR_NOT_FINITE, "z contains a non-finite value");
}

// 5: factorisations + tails of front `F` over the result block `res` and the status block `st` (kResTails / kStatTails / kStatFactor: the
// context's pinned areas, lane 1's, a loop chain's device memory).  The caller adds what is its own: done_counter, host_flag,
// ready_flag, seq.
StepFinishArgs step_finish_args(const icp_ctx& c, int n_props, icp_proposal* const* props, const StepFront& F, double* res, int* st) {
  StepFinishArgs a{};
  a.n = n_props; a.r = c.r; a.Ginv = c.Ginv.p; a.sigma2 = kSigma2;
  for (int i = 0; i < n_props; ++i) {
    icp_proposal* p = props[i];
    PosteriorEntry* lc = F.ec[i];
    PosteriorEntry* lp = F.ep[i];
    a.Mpart[i] = F.mpart[i]; a.splits[i] = F.splits[i];
    a.M[i] = lp->M.p; a.alpha[i] = lp->alpha.p;
    a.status[i] = p->status.p + lp->status_off;
    a.host_status[i] = st + kStatFactor + i;
    a.fwd[i] = TransitionTailIO{lc->alpha.p, lc->M.p, lc->coeffs.p, lp->coeffs.p, p->prm.step_length, res + kResTails + 2 * i,
                                st + kStatTails + 2 * i};
    a.bwd[i] = TransitionTailIO{lp->alpha.p, lp->M.p, lp->coeffs.p, lc->coeffs.p, p->prm.step_length, res + kResTails + 2 * i + 1,
                                st + kStatTails + 2 * i + 1};
  }
  return a;
}

// give back what a front holds without recording anything (its launches, if any, are harmless: they wrote to a state
// slot and memo entries that nobody refers to, to the search scratch and to the hints, which may be stale by design)
void release_front(StepFront& F) {
  if (F.mate) { StepFront* m = F.mate; F.mate = nullptr; if (m->valid || m->s) release_front(*m); }
  if (F.s) F.s->reserved = false;
  for (int i = 0; i < F.n_props; ++i)
    if (F.ep[i]) F.ep[i]->reserved = false;
  if (F.valid && F.eigen_first_use && F.generator >= 0 && F.ec[F.generator]) F.ec[F.generator]->eig_checked = false;
  F = StepFront{};
}
// A half step launched ahead for an outcome that did not happen.  Its launches may still be running — they write the search
// scratch, the hints, a state slot and memo entries that the replacement is about to be given — so the step that replaces it
// must be ordered behind it: it takes the dropped front's own stream (enqueue_front toggles the parity back), where stream
// order does that, instead of the other one, where nothing would.
void drop_front(icp_evaluator* e) {
  if (!e->front.valid) return;
  const int parity = e->front.parity;
  if (e->front.mate) ++e->ctx->twin_stats[2];  // (lane 1 goes with it)
  release_front(e->front);
  e->front_parity = parity ^ 1;
}
// Lane 1 of the twin pass whose lane 0 has been consumed, when the caller's next step is not the one it was made for (lane 0 was
// accepted).  Its part of the finish launch may still be running — it writes the entries' M and alpha, reads their coefficients —
// so the host sees its flag first (it trails lane 0's by a few µs at most); then the slots go back.  Its decomposition, if it was
// started with lane 0's, is cancelled before anything else (the eigen stream is held until it has seen the word), and its place in
// the proposal's count goes back.
void drop_twin(icp_evaluator* e, bool lane0_accepted = false) {
  if (!e->twin.valid) return;
  icp_ctx& c = *e->ctx;
  if (e->twin.eigen_early) {
    bool any = false;
    for (int i = 0; i < e->twin.F.n_props; ++i) {
      icp_proposal* p = e->twin.F.props[i];
      if (p->spec[1].e == e->twin.F.ep[i]) any = p->cancel_lane1_speculation() || any;
    }
    if (any && lane0_accepted) ++c.twin_eigen_stats[2];
  }
  if (!await_host_flag(c.h_flag + 1, e->twin.seq, std::chrono::seconds(2))) (void)hipStreamSynchronize(e->twin.F.stream);
  release_front(e->twin.F);
  e->twin = TwinPending{};
  ++c.twin_stats[2];
}
// everything an evaluator holds of steps launched ahead
void release_fronts(icp_evaluator* e) {
  drop_twin(e);
  if (e->front.valid) release_front(e->front);
}
bool fronts_use(const icp_evaluator* e, const icp_proposal* p) {
  return (e->front.valid && (e->front.props[0] == p || e->front.props[1] == p)) ||
         (e->twin.valid && (e->twin.F.props[0] == p || e->twin.F.props[1] == p));
}

// KL bases of a state's posteriors `ec` that are not on record yet: all of them are started now, in ONE launch on the eigen
// stream (they run side by side); a step waits for the one it draws from only (through its completion word) — the other
// is ready when a later step draws from it.  m_in_flight: `stream` may still be writing what they read.
struct EigenCollect {  // the decompositions of a batch of chains, launched together (icp_chain_step_batched)
  hipStream_t stream;                  // the eigen stream of the batch's first context
  std::vector<EigenRequest> rq;
  std::vector<PosteriorEntry*> all;    // every entry with a request: ONE event, recorded behind the launch, stands for them all
};

// Events for the decompositions of whole batches: one ring PER DEVICE (an event belongs to the device that was current when it
// was created) that lives as long as the process — the entries of many chains, many proposals, many contexts, destroyed in any
// order, point at its slots.  A slot is handed out again after 64 batches; the entries of the earlier batch notice by the slot's
// generation counter (PosteriorEntry::eigen_event_stale) and wait on the host instead of on an event that now stands for other work.
// One record per batch instead of one per chain that moved: ≈ 2.3 µs of host time each.
struct BatchEventSlot { hipEvent_t ev = nullptr; uint64_t gen = 0; };
BatchEventSlot& next_batch_event(int device) {
  constexpr int kMaxDevices = 64, kRing = 64;
  static std::mutex mu;
  static BatchEventSlot ring[kMaxDevices][kRing];
  static unsigned turn[kMaxDevices] = {};
  require(device >= 0 && device < kMaxDevices, "device ordinal out of range");
  std::lock_guard<std::mutex> lk(mu);
  BatchEventSlot& e = ring[device][turn[device]++ % kRing];
  if (!e.ev) HIP_OK(hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));  // (the caller has bound `device`)
  ++e.gen;
  return e;
}
// A launch that waits ON THE DEVICE for a word another stream's launch raises is safe as long as the waiting workgroups cannot keep
// the launch they wait for from becoming resident.  One chain's step cannot (its first launch is 14 workgroups, a decomposition
// six), two chains' neither; the batched step orders its chip-wide first launch behind the residency of its decompositions
// explicitly (StepBatchGate).  MANY contexts stepped one by one from many threads could, together, fill the chip with spinning first
// launches (round 2 saw the batched form of this: a 50 ms time-out): from three live contexts on, the single-chain
// step therefore takes its cross-stream order from events and stream order — no device-side wait at all.
bool device_side_waits_allowed() { return g_live_contexts.load(std::memory_order_relaxed) <= 2; }

void start_decompositions(icp_ctx& c, int n_props, icp_proposal* const* props, PosteriorEntry* const* ec, bool m_in_flight,
                          EigenCollect* collect = nullptr) {
  const int r = c.r;
  EigenRequest rqs[2];
  PosteriorEntry* need[2];
  int nn = 0;
  for (int i = 0; i < n_props; ++i)
    if (!ec[i]->eig_valid) { props[i]->prepare_eigen(*ec[i], &rqs[nn]); need[nn++] = ec[i]; }
  if (nn == 0) return;
  need[0]->eig_done_shared = nullptr;
  for (int i = 1; i < nn; ++i) need[i]->eig_done_shared = need[0]->eig_done;
  for (int i = 0; i < nn; ++i) need[i]->eig_shared_gen = nullptr;
  if (collect) {
    if (m_in_flight) HIP_OK(hipStreamSynchronize(c.stream));
    for (int i = 0; i < nn; ++i) need[i]->eig_event_valid = true;  // (recorded by the caller behind the batch's launch)
    (void)eigen_stream_for(c, collect->stream);
    for (int i = 0; i < nn; ++i) collect->rq.push_back(rqs[i]);
    for (int i = 0; i < nn; ++i) collect->all.push_back(need[i]);
    return;
  }
  const hipStream_t es = eigen_stream_for(c, c.eig_stream.get());
  // M of these entries is complete when they were recorded by a finished chain step (the host has seen its results);
  // only work another entry point has put on `stream` may still be writing them
  if (m_in_flight) {
    HIP_OK(hipEventRecord(c.ev_ready, c.stream));
    HIP_OK(hipStreamWaitEvent(es, c.ev_ready, 0));
  }
  if (launch_posterior_eigen_pair(es, r, c.sqrt_lambda.p, nn, rqs)) {
    if (!device_side_waits_allowed()) {
      // many contexts in the process: an event instead of the completion word (see device_side_waits_allowed)
      HIP_OK(hipEventRecord(need[0]->eig_done, es));
      for (int i = 0; i < nn; ++i) { need[i]->eig_event_valid = true; need[i]->done_value = 0; }
      return;
    }
    // completion words: the step's first launch waits for the one it draws from on the device; no event (host time on the
    // accepted path) — whoever else needs the basis waits for the eigen stream on the host (await_eigen)
    for (int i = 0; i < nn; ++i) need[i]->eig_event_valid = false;
    return;
  }
  for (int i = 0; i < nn; ++i) {  // (ranks > 64: one after the other)
    need[i]->done_value = 0;
    launch_posterior_eigen(es, r, rqs[i].M, c.sqrt_lambda.p, rqs[i].Vwarm, rqs[i].V, rqs[i].Vt, rqs[i].S, rqs[i].work, rqs[i].status,
                           nullptr, rqs[i].host_status);
  }
  HIP_OK(hipEventRecord(need[0]->eig_done, es));  // (one event for two launches in a row)
  for (int i = 0; i < nn; ++i) need[i]->eig_event_valid = true;
}

// launches 1-4 of a merged step with every choice made: F.ec / F.ep (the posterior entries of the current and of the proposed state),
// F.s (the proposed state's slot, its pose set), F.parity, F.stream.  enqueue_front above makes those choices from the memo; the
// on-device chain loop (icp_chains_run_on_device) fixes them once per chain and captures the arguments.
void front_launches(icp_evaluator* e, int n_props, icp_proposal* const* props, int generator, const double* key, StepFront& F, bool batched,
                    bool two_streams) {
  icp_ctx& c = *e->ctx;
  const int r = c.r;
  PosteriorEntry** ec = F.ec;
  PosteriorEntry** ep = F.ep;
  StateSlot& s = *F.s;
  const icp_evaluator_params& evp = e->prm;
  icp_proposal* pm = nullptr;  // ModelSampling proposal
  icp_proposal* pt = nullptr;  // TargetSampling proposal
  int im = -1, it = -1;
  for (int i = 0; i < n_props; ++i) {
    if (props[i]->prm.direction == ICP_MODEL_SAMPLING) { pm = props[i]; im = i; }
    else { pt = props[i]; it = i; }
  }
  const bool ev_m2t = evp.mode != ICP_TARGET_TO_MODEL, ev_t2m = evp.mode != ICP_MODEL_TO_TARGET;
  const int Ksurf = std::max(ev_m2t ? evp.n_model_ids : 0, pm ? pm->K : 0);
  F.Ksurf = Ksurf;
  require(Ksurf <= c.N, "model id count exceeds the number of model points");
  if (!F.h_coeffs) {  // (a front made by the on-device loop: lane 0's areas)
    F.h_coeffs = c.h_res + 16 + F.parity * kCoeffArea;
    F.h_reduce = c.h_res + kReduceArea + F.parity * 8;
  }
  // lane 1 of a twin pass: scratch sets and result buffers of its own; the hints are read and left as they are
  const int lane = F.lane, sw = lane ? 7 : 0;
  QueryBuffers qs = c.query_scratch(Ksurf, c.target.T, sw);
  QueryBuffers qv{};
  if (pt) qv = c.query_scratch(pt->K, c.N, sw + 1);

  SurfaceTask st_surf = make_surface_task(c.target.T, c.target.verts.p, c.target.tris.p, c.target.spheres.p, Ksurf, s.x.p,
                                          c.hint_surf.p, qs, s.surf_cp.p, s.surf_d2.p, s.surf_tri.p);
  VertexTask st_vert{};
  if (pt) st_vert = make_vertex_task(c.N, s.x.p, pt->K, pt->target_pts.p, pt->hint_nn.p, qv, nullptr, lane ? pt->nn_id2.p : pt->nn_id.p);
  st_surf.keep_hint = st_vert.keep_hint = lane;
  st_vert.thr2 = nullptr;  // bounds are computed by the filter launch itself (see vertex_filter)
  // the evaluator's reverse direction (IndependentPointDistanceEvaluator.scala:49-54, Collective…Evaluator.scala:55-64): its
  // decimated-target points against the surface of the NEW instance — spheres and bounds are taken by the filter launch itself
  SurfaceTask st_t2m{};
  if (ev_t2m) {
    QueryBuffers qt = c.query_scratch(e->Kt, c.T, sw + 2);
    st_t2m = make_surface_task(c.T, s.x.p, c.tris.p, nullptr, e->Kt, e->d_tpts, e->hint_tri.p, qt, lane ? e->t2m_cp2.p : e->t2m_cp.p,
                               lane ? e->t2m_d2_2.p : e->t2m_d2.p, lane ? e->t2m_tri2.p : e->t2m_tri.p);
    st_t2m.keep_hint = lane;
    st_t2m.order = c.tri_order.p;
    st_t2m.thrA = nullptr;
  }

  // 1: coefficients -> instance -> bounds
  StepBeginArgs b{};
  b.N = c.N; b.r = r; b.inst_blocks = (c.N + 255) / 256;
  b.Qp = c.Qp.p; b.ref = c.ref.p; b.mean = c.mean.p; b.pose = s.pose;
  b.propose = generator >= 0 ? 1 : 0;
  const double* src = generator >= 0 ? key : key + 10;
  // (the merged launches cover ranks whose factor fits LDS — step_finish_supported, about 116 — so the r host-drawn numbers
  // always travel inside the kernel arguments)
  require(r <= kStepInlineZ, "internal: merged step at a rank above the inline-argument limit");
  std::memcpy(b.zin, src, sizeof(double) * r);
  if (generator >= 0) {
    PosteriorEntry& g = *ec[generator];
    b.prop = ProposeIn{g.alpha.p, g.V.p, g.S.p, c.inv_sqrt_lambda.p, c.P.p, g.coeffs.p, nullptr, kSigma2,
                       props[generator]->prm.step_length, props[generator]->sampler == ICP_SAMPLER_CHOLESKY_ROOT};
    b.tpr_log2 = matvec_tpr_log2(r, 256);  // (as k_propose's)
  }
  b.n_out = 0;
  b.out[b.n_out++] = s.coeffs.p;
  for (int i = 0; i < n_props; ++i) b.out[b.n_out++] = ep[i]->coeffs.p;
  b.out[b.n_out++] = const_cast<double*>(F.h_coeffs);
  b.x = s.x.p;
  b.has_surf = 1; b.surf = st_surf;
  b.has_vert = pt ? 1 : 0; b.vert = st_vert;
  b.zero2 = ev_t2m ? st_t2m.cnt : nullptr; b.n_zero2 = ev_t2m ? st_t2m.Kpad : 0;
  // (nothing to wait for before the first finish launch, nor when every step is on one stream)
  b.wait_flag = (c.last_back_seq > 0 && two_streams) ? c.d_done.p + 2 : nullptr;
  // test hook: the first launch waits for a word that never comes, times out, and the step is repeated unpipelined
  static const int starve_pipeline = dev_env("ICP_TEST_STARVE_PIPELINE") ? (1 << 24) : 0;
  b.wait_seq = c.last_back_seq + starve_pipeline;
  b.wait_error = c.h_wait_error;
  b.wait_ticks = c.profiling ? c.d_wait_ticks.p : nullptr;
  if (generator >= 0 && ec[generator]->done_value != 0) {
    b.wait2_flag = props[generator]->eig_words.p + ec[generator]->status_off / 3;
    b.wait2_seq = ec[generator]->done_value;
    // still in flight (the register-holding variant of launch 1 multiplies with the KL basis: not for the Cholesky-root sampler)
    b.hold_regs = *(volatile int*)(props[generator]->h_eig + ec[generator]->status_off / 3) == -1 && !b.prop.root;
  }
  launch_step_begin(F.stream, b);

  // 2 + 3: searches and correspondences
  StepSearchArgs q{};
  q.n_surf = ev_t2m ? 2 : 1; q.n_vert = pt ? 1 : 0;
  q.s[0] = st_surf;
  q.fstart[0] = 0; q.fstart[1] = filter_grid_blocks(st_surf.tblocks, st_surf.ksplit);
  q.rstart[0] = 0; q.rstart[1] = Ksurf;
  int nt = 1;  // tasks so far (surface tasks first)
  if (ev_t2m) {
    q.s[1] = st_t2m;
    q.fstart[2] = q.fstart[1] + filter_grid_blocks(st_t2m.tblocks, st_t2m.ksplit);
    q.rstart[2] = q.rstart[1] + e->Kt;
    nt = 2;
  }
  q.s_corr[0] = q.s_corr[1] = q.v_corr[0] = q.v_corr[1] = -1;
  int n_corr = 0;
  if (pm) {
    q.corr[n_corr] = CorrTask{pm->K, ep[im]->corr(), s.x.p, nullptr, c.target.boundary.p, nullptr, pm->prm.boundary_aware,
                              s.pose, c.ref.p, c.mean.p, c.tris.p, c.adj_off.p, c.adj.p};
    q.s_corr[0] = n_corr++;
  }
  if (pt) {
    q.v[0] = st_vert;
    q.fstart[nt + 1] = q.fstart[nt] + filter_grid_blocks(st_vert.vblocks, st_vert.ksplit);
    q.rstart[nt + 1] = q.rstart[nt] + pt->K;
    q.corr[n_corr] = CorrTask{pt->K, ep[it]->corr(), s.x.p, pt->target_pts.p, c.boundary.p, nullptr, pt->prm.boundary_aware,
                              s.pose, c.ref.p, c.mean.p, c.tris.p, c.adj_off.p, c.adj.p};
    q.v_corr[0] = n_corr++;
  }
  // one surface task (the static target) and at most one vertex task of a lone chain: a wave per query, one launch (k_step_search)
  // (its kernel takes the surface task's posterior, if any, as corr[0]: q.s_corr[0] <= 0 by the order above)
  const bool one_search = !batched && !ev_t2m && !c.step_search_split && c.target.T > 0 && c.target.balls.p != nullptr &&
                          (!pt || c.N <= kStepSearchMaxV);
  if (one_search) {
    launch_step_search(F.stream, q, c.target.tables());
  } else {
    launch_step_filter(F.stream, q);
    launch_step_resolve(F.stream, q);
  }

  // 4: regressions + likelihood reduction
  StepRegressionArgs g{};
  g.n = n_props; g.r = r;
  g.ntiles = regression_tiles(r);
  g.Q = c.Q.p;
  g.ustart[0] = 0;
  int* splits = F.splits;
  for (int i = 0; i < n_props; ++i) {
    icp_proposal* p = props[i];
    const int leaves = regression_splits(p->K);
    g.K[i] = p->K;
    g.kchunk[i] = std::max(1, (p->K + leaves - 1) / leaves);
    // (chains stepped side by side fold a posterior's leaves into one partial: tl_regression_posteriors = posteriors in the launch)
    g.fold[i] = regression_fold(p->K, r, tl_regression_posteriors);
    g.macro[i] = regression_macro(r, g.fold[i]);
    splits[i] = leaves / g.fold[i];  // (fold is 1 or `leaves`)
    g.cb[i] = ep[i]->corr();
    g.wt[i] = 1.0 / (p->prm.tangential_noise * p->prm.tangential_noise);
    g.kappa[i] = 1.0 / (p->prm.noise_along_normal * p->prm.noise_along_normal) - g.wt[i];
    p->mpart_half = (p->mpart_half + 1) % icp_proposal::kMpartRing;
    g.Mpart[i] = p->mpart_for_write(p->mpart_half, F.stream);
    g.status[i] = p->status.p + ep[i]->status_off;
    g.ustart[i + 1] = g.ustart[i] + regression_units(r, leaves, g.fold[i], g.macro[i]);
  }
  if (n_props == 1) g.ustart[2] = g.ustart[1];
  g.reduce_kind = evp.kind == ICP_EVAL_INDEPENDENT_POINT_DISTANCE ? 1 : 2;
  g.Kred = ev_m2t ? evp.n_model_ids : 0; g.d2 = s.surf_d2.p; g.mean = evp.gauss_mean; g.sigma = evp.gauss_sigma;
  g.Kred2 = ev_t2m ? e->Kt : 0; g.d2b = lane ? e->t2m_d2_2.p : e->t2m_d2.p;
  g.red_out = F.h_reduce;
  for (int i = 0; i < n_props; ++i) { F.mpart[i] = g.Mpart[i]; F.mpart_half[i] = props[i]->mpart_half; }
  launch_step_regression(F.stream, g);
  if (!batched && !F.mate && !lane) {  // (a twin pass is not issued where 4b would be needed: twin_splits_ok) 4b: many partials are summed by many CUs before the one-workgroup factorisation (see launch_step_reduce)
    bool many = false;
    for (int i = 0; i < n_props; ++i) many = many || splits[i] >= kStepReduceSplits;
    if (many) {
      StepReduceArgs ra{};
      ra.n = n_props; ra.nn = (r + 1) * (r + 1);
      for (int i = 0; i < n_props; ++i) { ra.Mpart[i] = g.Mpart[i]; ra.splits[i] = splits[i]; splits[i] = 1; }
      launch_step_reduce(F.stream, ra);
    }
  }
}

// launches 1-3 of the step (theta_cur --generator/key--> proposal); `key` = z or the proposed state (see StepFront)
// (batched: the launches are being captured for icp_chain_step_batched — one stream, nothing to wait for on the device
// but the decomposition)
// F2 (with generator2 / key2): the step after it as well, from the same theta_cur, as lane 1 of a twin pass — ONE set of launches
void enqueue_front(icp_evaluator* e, int n_props, icp_proposal* const* props, int generator, const double* theta_cur,
                   const double* key, StepFront& F, bool batched = false, StepFront* F2 = nullptr, int generator2 = -1,
                   const double* key2 = nullptr) {
  icp_ctx& c = *e->ctx;
  const int r = c.r;
  F = StepFront{};
  F.n_props = n_props; F.generator = generator;
  for (int i = 0; i < n_props; ++i) F.props[i] = props[i];
  F.theta_cur.assign(theta_cur, theta_cur + 10 + r);
  F.key.assign(key, key + (generator >= 0 ? r : 10 + r));
  F.parity = (e->front_parity ^= 1);
  F.h_coeffs = c.h_res + 16 + F.parity * kCoeffArea;
  F.h_reduce = c.h_res + kReduceArea + F.parity * 8;  // (its own half: the host may still be reading the previous step's)
  if (F2) {
    *F2 = F;
    F2->lane = 1; F2->generator = generator2;
    F2->key.assign(key2, key2 + (generator2 >= 0 ? r : 10 + r));
    F2->h_coeffs = c.h_twin + 16 + F.parity * kCoeffArea;
    F2->h_reduce = c.h_twin + kReduceArea + F.parity * 8;
    F.mate = F2;  // (from here on lane 1 is released with lane 0)
  }
  // ---- cached side: posterior of the current state for every proposal (+ its KL basis for the generating one)
  PosteriorEntry** ec = F.ec;
  bool missing = false;
  for (int i = 0; i < n_props; ++i) missing = missing || !props[i]->find_entry(theta_cur);
  if (missing && c.front_stream_used) {  // the posteriors are computed on `stream` with the scratch a step in flight may still use
    c.front_stream.sync();
    c.front_stream_used = false;
  }
  for (int i = 0; i < n_props; ++i) ec[i] = &props[i]->posterior(theta_cur, false);  // NonRigidIcpProposal.scala:54,76
  if (missing) c.stream_used_elsewhere = true;  // … and this step reads them
  const bool m_in_flight = c.stream_used_elsewhere;  // `stream` may still be writing what the decompositions below read
  const bool two_streams = !c.pipeline_off && !batched && device_side_waits_allowed();
  F.stream = (F.parity && two_streams) ? c.front_stream.get() : c.stream;
  if (F.stream == c.front_stream.peek()) {
    if (c.stream_used_elsewhere) {  // another entry point has work on `stream` that this step may depend on: join once
      HIP_OK(hipEventRecord(c.ev_join, c.stream));
      HIP_OK(hipStreamWaitEvent(c.front_stream.get(), c.ev_join, 0));
    }
    c.front_stream_used = true;
  }
  c.stream_used_elsewhere = false;
  start_decompositions(c, n_props, props, ec, m_in_flight);
  if (F2) { F2->stream = F.stream; for (int i = 0; i < n_props; ++i) F2->ec[i] = ec[i]; }
  // (per lane; two lanes that draw from the same basis: the first one fetches its status)
  for (StepFront* L : {&F, F2}) {
    if (!L || L->generator < 0) continue;
    PosteriorEntry* g = ec[L->generator];
    // (await_eigen on the front's stream: through the decomposition's own completion word when it has one — see launch 1)
    if (g->done_value == 0 && g->eigen_event()) HIP_OK(hipStreamWaitEvent(F.stream, g->eigen_event(), 0));
    L->eigen_first_use = !g->eig_checked;  // (possibly of an earlier prefetch or speculation): fetch its status
    g->eig_checked = true;
  }

  // ---- new side: one state slot, one memo entry per proposal (and lane)
  for (StepFront* L : {&F, F2}) {
    if (!L) continue;
    StateSlot& s = c.fresh_state();
    s.reserved = true;
    L->s = &s;
    s.pose = c.pose_of(L->generator >= 0 ? theta_cur : L->key.data());
    for (int i = 0; i < n_props; ++i) { L->ep[i] = &props[i]->fresh_entry(); L->ep[i]->reserved = true; }
  }
  if (!F2) {
    front_launches(e, n_props, props, generator, key, F, batched, two_streams);
  } else {
    // both lanes' launches are captured (arguments finalised, grids known) and issued as one set
    StepCapture caps[2];
    struct CaptureGuard { ~CaptureGuard() { step_capture(nullptr); } } capture_guard;
    step_capture(&caps[0]);
    front_launches(e, n_props, props, generator, key, F, batched, two_streams);
    step_capture(&caps[1]);
    front_launches(e, n_props, props, generator2, key2, *F2, batched, two_streams);
    step_capture(nullptr);
    launch_step_twin_front(F.stream, caps[0], caps[1]);
    F2->valid = true;
    ++c.twin_stats[0];
  }
  F.valid = true;
}

// Host side of a merged step whose results have arrived in the context's pinned memory: status of the decomposition it
// drew from, the proposed state, the memo entries, the rare direct transition tail, likelihood and densities.
// -> false: the step has to be done again (nothing of it has been recorded)
bool chain_step_record(icp_evaluator* e, int n_props, icp_proposal* const* props, int generator, const double* theta_cur, StepFront& F,
                       const StepFinishArgs& f, double* theta_prop, double* log_value_prop, double* fwd, double* bwd, int* status) {
  icp_ctx& c = *e->ctx;
  const int r = c.r;
  PosteriorEntry** ec = F.ec;
  PosteriorEntry** ep = F.ep;
  StateSlot& s = *F.s;
  const int Ksurf = F.Ksurf;
  const bool eigen_first_use = F.eigen_first_use;
  const bool eigen_status_pinned = eigen_speculation_supported(r);
  const double* h_coeffs = F.h_coeffs;
  if (eigen_first_use && eigen_status_pinned) {  // this step's first launch waited for that decomposition: its status is in
    icp_proposal* p = props[generator];
    const int st = p->h_eig[ec[generator]->status_off / 3];
    if (st == kEigenGaveUp) {  // a speculative decomposition that never saw its input (see k_posterior_eigen_rr): the
      // step just computed drew from a stale basis — drop it (nothing of it has been recorded) and do it again
      ++c.stats.speculation_giveups; ++g_runtime_stats.speculation_giveups;
      ec[generator]->eig_valid = false;
      ec[generator]->eig_checked = false;
      p->warm_valid = false;  // (it pointed at the basis that was never written)
      return false;
    }
    p->h_status[ec[generator]->status_off + 2] = st;
  }
  const size_t P = 10 + (size_t)r;
  if (generator >= 0) {
    std::memcpy(theta_prop, theta_cur, sizeof(double) * 10);  // :64-66 only the shape changes
    for (int j = 0; j < r; ++j) {
      if (!std::isfinite(h_coeffs[j])) fail(ICP_ERR_NOT_FINITE, "proposed coefficients are not finite");
      theta_prop[10 + j] = h_coeffs[j];
    }
  }
  s.theta.assign(theta_prop, theta_prop + P);
  s.valid = true;
  s.stamp = ++c.clock;
  s.n_surf = Ksurf;
  for (int i = 0; i < n_props; ++i) {
    icp_proposal* p = props[i];
    ep[i]->theta.assign(theta_prop, theta_prop + P);
    ep[i]->valid = true;
    ep[i]->stamp = ++p->clock;
    p->h_status[ep[i]->status_off] = c.h_status[kStatFactor + i];
    p->h_status[ep[i]->status_off + 1] = 0;
    p->h_status[ep[i]->status_off + 2] = 0;
    p->check_status(*ec[i]);
    p->check_status(*ep[i]);
  }
  for (int t = 0; t < 2 * n_props; ++t)
    if (c.h_status[kStatTails + t] != 0) {  // rare: the fixed-point tail did not contract -> direct kernel
      std::vector<double> saved(c.h_res, c.h_res + 16);
      icp_proposal* p = props[t / 2];
      TransitionTailIO io = (t % 2 == 0) ? f.fwd[t / 2] : f.bwd[t / 2];
      io.out = c.d_res.p;
      io.status = c.d_status.p + 32;
      sync_eigen(c);  // (the direct form borrows the eigen work buffer)
      launch_transition_tail_direct(c.stream, r, io, c.G.p, kSigma2, p->work.p);
      c.finish(1, 64);
      if (c.h_status[32] != 0) fail(ICP_ERR_NOT_SPD, "G + sigma^2 M is not positive definite");
      saved[kResTails + t] = c.h_res[0];
      std::memcpy(c.h_res, saved.data(), sizeof(double) * saved.size());
    }
  for (int i = 0; i < 8; ++i) c.h_res[i] = F.h_reduce[i];  // launch 4's reductions, where finish_eval looks
  icp_evaluator::Memo* m = eval_store(e, theta_prop);
  m->status = finish_eval(e, c.h_res, &m->value, m->aux);
  *log_value_prop = m->value;
  *status = m->status;
  for (int i = 0; i < n_props; ++i) {
    fwd[i] = c.h_res[kResTails + 2 * i];
    bwd[i] = c.h_res[kResTails + 2 * i + 1];
    if (std::isnan(fwd[i]) || std::isnan(bwd[i])) fail(ICP_ERR_NOT_FINITE, "NaN transition probability");
  }
  return true;
}
bool front_matches(const StepFront& F, int n_props, icp_proposal* const* props, int generator, const double* theta_cur,
                   const double* key, int r) {
  if (!F.valid || F.n_props != n_props || F.generator != generator) return false;
  for (int i = 0; i < n_props; ++i)
    if (F.props[i] != props[i]) return false;
  return std::memcmp(F.theta_cur.data(), theta_cur, sizeof(double) * (10 + r)) == 0 &&
         std::memcmp(F.key.data(), key, sizeof(double) * F.key.size()) == 0;
}

// -> the merged launches cover this call (icp_chain_step, icp_chain_step_prelaunch and the batch ask before they issue anything)
bool chain_step_covered(icp_evaluator* e, int n_props, icp_proposal* const* props, int generator, const double* theta_cur,
                        const double* theta_prop_in) {
  icp_ctx& c = *e->ctx;
  bool per_stage = !step_pipeline_covers(e, n_props, props);
  if (!per_stage && generator < 0) {
    // a state the caches already know (or a pose move, whose ICP transition densities are -inf) has nothing to merge
    per_stage = !pose_equal(theta_cur, theta_prop_in) || c.find_state(theta_prop_in) || eval_lookup(e, theta_prop_in);
    for (int i = 0; i < n_props && !per_stage; ++i) per_stage = props[i]->find_entry(theta_prop_in) != nullptr;
  }
  return !per_stage;
}

// a twin pass has no launch 4b (launch_step_reduce): only where no posterior of the step has that many split-K partials
bool twin_splits_ok(const icp_ctx& c, int n_props, icp_proposal* const* props) {
  for (int i = 0; i < n_props; ++i) {
    const int leaves = regression_splits(props[i]->K);
    if (leaves / regression_fold(props[i]->K, c.r, 1) >= kStepReduceSplits) return false;
  }
  return true;
}

// icp_chain_step_prelaunch and icp_chain_step_prelaunch2 (generator2 / key2: the step after the next, or key2 == nullptr); -> lanes issued
int chain_step_prelaunch(icp_evaluator* e, int32_t n_props, icp_proposal* const* props, int32_t generator, const double* theta_cur,
                         const double* key, int32_t generator2, const double* key2) {
  require(e != nullptr, "null argument");
  if (n_props == 0) {  // "nothing further": drop a pending half step (and lane 1 of a twin pass being finished)
    std::lock_guard<std::recursive_mutex> lk0(e->ctx->mu);
    drop_front(e);
    drop_twin(e);
    return 0;
  }
  require(theta_cur && key, "null argument");
  require(n_props >= 1 && n_props <= 2 && props, "bad proposal list");
  require(generator2 < n_props, "generator index out of range");  // (both generators ahead of everything else)
  icp_ctx& c = *e->ctx;
  check_step_args(c, n_props, props, generator, theta_cur, key);
  if (key2) check_step_args(c, n_props, props, generator2, theta_cur, key2);
  std::lock_guard<std::recursive_mutex> lk(c.mu);
  drop_front(e);
  if (c.pipeline_off) return 0;
  // with several chains in the process the device is not idle during one chain's turn-around, and the launches of a
  // dropped half step cost the others host time (tools/multichain.py)
  if (g_live_contexts.load(std::memory_order_relaxed) > 1) return 0;
  if (!chain_step_covered(e, n_props, props, generator, theta_cur, key)) return 0;  // nothing to pre-launch
  // every posterior of the assumed current state must be on record already (the step in flight computed them)
  for (int i = 0; i < n_props; ++i)
    if (!props[i]->find_entry(theta_cur)) return 0;
  // the step after it beside it, as lane 1 of a twin pass: where the merged launches cover that one, too
  // (ranks <= 64: the decomposition's status reaches the host by itself, no copy on the step's stream)
  // Lane 1 is used only if lane 0's proposal is rejected: while the chain accepts more than every second step (acc_ema, as the
  // speculative decompositions use it — the first steps of a chain from the mean: 17 of 20) it would be dropped more often than
  // used, and its launches cost the accepted path about 1 % (the 20-step window of tools/ab_config1.py): one lane there.
  const bool twin = key2 && !c.twin_off && e->acc_ema <= 0.5 && eigen_speculation_supported(c.r) && chain_step_covered(e, n_props, props, generator2, theta_cur, key2) &&
                    twin_splits_ok(c, n_props, props) &&
                    !(generator < 0 && generator2 < 0 && std::memcmp(key, key2, sizeof(double) * (10 + (size_t)c.r)) == 0);
  Bound _b(&c, true);
  try {
    if (twin) enqueue_front(e, n_props, props, generator, theta_cur, key, e->front, false, &e->front2, generator2, key2);
    else enqueue_front(e, n_props, props, generator, theta_cur, key, e->front);
  } catch (...) {
    release_front(e->front);
    throw;
  }
  return twin ? 2 : 1;
}

// ---- icp_chain_step on the merged launches: phases over one ChainStep, called in order by the entry point below.  A step that is
// lane 1 of the twin pass the previous call finished skips the finish launch and the speculation: both went out with lane 0's.
struct ChainStep {
  icp_evaluator* e; int n_props; icp_proposal* const* props; int generator; const double* theta_cur; const double* key;
  double* theta_prop; double* log_value_prop; double* fwd; double* bwd;
  icp_ctx& c;
  const int r;
  ChainStep(icp_evaluator* e_, int n_props_, icp_proposal* const* props_, int generator_, const double* theta_cur_, const double* key_,
            double* theta_prop_, double* log_value_prop_, double* fwd_, double* bwd_)
      : e(e_), n_props(n_props_), props(props_), generator(generator_), theta_cur(theta_cur_), key(key_), theta_prop(theta_prop_),
        log_value_prop(log_value_prop_), fwd(fwd_), bwd(bwd_), c(*e_->ctx), r(c.r) {}
  bool lane1 = false;  // the step is lane 1 of the pending twin pass: launches 1-5 are out (or done), the previous call issued them
  bool reuse = false;  // the pre-launched front is this step's (asked by step_take_front only)
  struct FrontGuard {  // whatever happens, the slots of this step are not left reserved
    StepFront* f;
    ~FrontGuard() { if (f) release_front(*f); }
  };
  StepFront F;
  FrontGuard front_guard{&F};
  StepFront F1;  // lane 1 of a twin front, until its finish launch is out
  FrontGuard front1_guard{&F1};
  StepFinishArgs f{};
  int step_seq = 0;
  bool lane1_eigen_out = false;  // lane 1's decomposition went out with lane 0's: nothing to start for it
};

// 1: where the step's front comes from.  Lane 1 of the twin pass whose lane 0 the previous call consumed: this is the step it was made
// for (lane 0 was rejected), or it is dropped — and with it the front launched behind it, for a state the chain has left.
// -> false: the merged launches do not cover the call (nothing launched ahead matches it either)
bool step_classify(ChainStep& s) {
  icp_evaluator* e = s.e;
  s.lane1 = s.n_props <= 2 && front_matches(e->twin.F, s.n_props, s.props, s.generator, s.theta_cur, s.key, s.r);
  if (e->twin.valid && !s.lane1)  // (lane 0 accepted: the caller's current state is what the previous step proposed)
    drop_twin(e, kept_last_proposal(e, s.theta_cur, s.r));
  s.reuse = !s.lane1 && s.n_props <= 2 && front_matches(e->front, s.n_props, s.props, s.generator, s.theta_cur, s.key, s.r);
  if (e->front.valid && !s.reuse && !s.lane1) drop_front(e);  // pre-launched for another outcome: dropped
  return s.reuse || s.lane1 || chain_step_covered(e, s.n_props, s.props, s.generator, s.theta_cur, s.theta_prop);
}

// 2: what the previous step left open — its speculative decompositions are kept or cancelled, its outcome enters the acceptance
// estimate — and the front: lane 1's with its finish arguments, the pre-launched one (a twin front's lane 1 goes to F1), or issued now
void step_take_front(ChainStep& s) {
  icp_evaluator* e = s.e;
  bool kept_lane1 = false;
  for (int i = 0; i < s.n_props; ++i) kept_lane1 = s.props[i]->resolve_speculation(s.theta_cur, s.lane1) || kept_lane1;
  if (kept_lane1) ++s.c.twin_eigen_stats[1];
  if (!e->acc_counted) note_outcome(e, s.theta_cur, s.r);
  if (s.lane1) {
    s.F = std::move(e->twin.F); s.f = e->twin.f; s.step_seq = e->twin.seq; s.lane1_eigen_out = e->twin.eigen_early;
    e->twin = TwinPending{};
  } else if (s.reuse) {
    s.F = std::move(e->front); e->front = StepFront{};
    if (s.F.mate) { s.F1 = std::move(*s.F.mate); *s.F.mate = StepFront{}; s.F.mate = nullptr; }
  } else {
    enqueue_front(e, s.n_props, s.props, s.generator, s.theta_cur, s.key, s.F);
  }
}

// 3 (not for a lane-1 step): the finish launch, results straight to pinned host memory.  A twin front: one launch for both lanes; lane 1
// has result areas, a completion counter and a host flag of its own, so that this step's results are not held back by it, and stays
// with the evaluator: the next call takes it, or drops it.
void step_finish_launch(ChainStep& s) {
  icp_ctx& c = s.c;
  for (int i = 0; i < 16; ++i) c.h_res[i] = 0.0;
  for (int i = 0; i < 16; ++i) c.h_status[i] = 0;
  s.step_seq = ++c.step_seq;
  s.f = step_finish_args(c, s.n_props, s.props, s.F, c.h_res, c.h_status);
  s.f.seq = s.step_seq; s.f.done_counter = c.d_done.p; s.f.host_flag = c.h_flag;
  s.f.ready_flag = c.d_done.p + 2;  // (speculative decompositions and the next step's first launches wait for it)
  c.last_back_seq = s.step_seq;
  if (!s.F1.valid) {
    launch_step_finish(s.F.stream, s.f);
    return;
  }
  for (int i = 0; i < 16; ++i) c.h_twin[i] = 0.0;
  for (int i = 0; i < 16; ++i) c.h_twin_status[i] = 0;
  StepFinishArgs f1 = step_finish_args(c, s.n_props, s.props, s.F1, c.h_twin, c.h_twin_status);
  f1.seq = s.step_seq; f1.done_counter = c.d_done.p + 3; f1.host_flag = c.h_flag + 1;
  launch_step_twin_finish(s.F.stream, s.f, f1);
  TwinPending& tw = s.e->twin;
  tw.F = std::move(s.F1); tw.f = f1; tw.seq = s.step_seq; tw.valid = true;
  s.F1 = StepFront{};  // (its slots belong to the evaluator now)
}

// 4 (not where lane 1's decompositions went out with lane 0's: they are pending — icp_proposal::spec[0] now —, the call after this one
// keeps or cancels them): KL bases of the proposed state's posteriors, in case it is accepted.  They run on the eigen stream beside the
// factorisations and the host's round trip; the next call keeps or cancels them (resolve_speculation).  One launch (both directions
// side by side), issued BEFORE the caller's hook: the accepted path waits for nothing else.
// Adaptive (speculation_mode): an accepted step finds its basis ≈ 50 µs earlier; a rejected one has paid one launch for
// nothing: ≈ 3 µs of host time, a few CUs — and the eigen stream, which the next decomposition shares, until the launch has
// seen its cancel word.  The kernel looks at the word before it starts and every eight rounds (≈ 3 µs) of the iteration:
// the launch behind a rejected step then starts 0-8 µs after its input (median; 13-25 µs when the word was looked at once
// per sweep: profiles/spec_cancel_lag.md).  Worth it unless next to nothing is accepted (measured then: 8.3k against 7.4k
// it/s over a chain's first 20 steps).
// (A lane-1 step whose decomposition did not go out early — ICP_TWIN_LATE_EIGEN, or that call did not start it — starts it here: lane 0
// was rejected, its own has just been cancelled, and lane 1's input is complete.)
void step_speculate(ChainStep& s) {
  icp_ctx& c = s.c;
  icp_evaluator* e = s.e;
  const int n_props = s.n_props, r = s.r;
  // test hook: the speculative decompositions wait for a word that never comes, time out and are repeated
  static const int starve = dev_env("ICP_TEST_STARVE_SPECULATION") ? (1 << 24) : 0;
  if (c.speculation_off || g_live_contexts.load(std::memory_order_relaxed) > 2 || n_props <= 0 || !eigen_speculation_supported(r)) return;
  if (!speculation_wanted(e->acc_ema)) {
    // switched off where the default would speculate: the decompositions keep their places in the count (plan_eigen)
    if (speculation_mode() == 0 && e->acc_ema >= 0.1)
      for (int i = 0; i < n_props; ++i) s.props[i]->plan_eigen(*s.F.ep[i]);
    return;
  }
  EigenSpec specs[kEigenPairMax];
  EigenRequest rqs[kEigenPairMax];
  int nq = 0;
  for (int i = 0; i < n_props; ++i, ++nq)
    s.props[i]->speculate_eigen(*s.F.ep[i], *s.F.ec[i], s.F.splits[i], s.F.mpart_half[i], c.d_done.p + 2, s.step_seq + starve, &specs[nq], &rqs[nq]);
  // A twin pass just finished (lane 1 is with the evaluator): lane 1's as well, in the same launch — its normal matrix is as complete as
  // lane 0's (the finish launch raises the one `ready` word behind both lanes' regressions), and a pass that ends "lane 0 rejected,
  // lane 1 accepted" finds the basis a finish launch and a host turn-around earlier.  Lane 1 is used only behind a rejected lane 0:
  // started here exactly where its own call would have started it (the acceptance estimate after that rejection), so that the places
  // in the proposals' counts fall as they do one call at a time.  The Cholesky-root sampler keeps the late order.
  bool early = e->twin.valid && !c.twin_late_eigen && speculation_wanted(0.9 * e->acc_ema + 0.0);
  for (int i = 0; i < n_props; ++i) early = early && s.props[i]->sampler != ICP_SAMPLER_CHOLESKY_ROOT;
  if (early) {
    const StepFront& L1 = e->twin.F;
    bool cold = false;
    for (int i = 0; i < n_props; ++i, ++nq) {
      const bool cold_place = s.props[i]->eig.ahead_cold();
      s.props[i]->speculate_eigen(*L1.ep[i], *L1.ec[i], L1.splits[i], L1.mpart_half[i], c.d_done.p + 2, s.step_seq + starve, &specs[nq], &rqs[nq], 1);
      cold = cold || cold_place;
    }
    e->twin.eigen_early = true;
    ++c.twin_eigen_stats[0];
    if (cold) ++c.twin_eigen_stats[3];
  }
  const hipStream_t es = eigen_stream_for(c, c.eig_stream.get());
  // (no event: completion words, see start_decompositions)
  if (!launch_posterior_eigen_pair(es, r, c.sqrt_lambda.p, nq, rqs)) fail(ICP_ERR_DEVICE, "internal: no decomposition kernel for a speculative launch");
}

// 5: the results.  The finish launch's flag in pinned memory (give up after 2 s and let the synchronisation report what went wrong), or,
// where the decomposition the step drew from leaves its status in device memory only (ranks > 64), a synchronisation and a copy.  A
// lane-1 step's results then go where lane 0's are looked for.
void step_wait(ChainStep& s) {
  icp_ctx& c = s.c;
  const StepFront& F = s.F;
  if (F.eigen_first_use && !eigen_speculation_supported(s.r)) {
    if (F.stream != c.stream) HIP_OK(hipStreamSynchronize(F.stream));
    sync_proposal_status_if(s.props[s.generator], true);
    c.finish(0, 0);
  } else {
    if (!await_host_flag(s.f.host_flag, s.f.seq, std::chrono::seconds(2))) {
      if (F.stream != c.stream) HIP_OK(hipStreamSynchronize(F.stream));
      c.finish(0, 0);
    }
    c.stage_used = 0;
  }
  if (s.lane1) {
    for (int i = 0; i < 16; ++i) c.h_res[i] = c.h_twin[i];
    for (int i = 0; i < 16; ++i) c.h_status[i] = c.h_twin_status[i];
  }
}

// 6 (c.h_wait_error: this path's only reader): a first launch did not see the word it waits for within 50 ms and went ahead unordered.
// That is what a tool does that lets one kernel run at a time in an order of its own (rocprofv3 --pmc): drain everything, switch the
// pipelining off for this context, and have the step done again — nothing of it has been recorded.  (The decomposition started or
// planned for its proposed state is withdrawn first: the repeated step starts it again, in the same place of the count.)
void step_first_launch_timed_out(ChainStep& s) {
  icp_ctx& c = s.c;
  for (int i = 0; i < s.n_props; ++i) s.props[i]->withdraw_speculation();
  s.e->acc_counted = true;
  HIP_OK(hipStreamSynchronize(c.stream));
  c.front_stream.sync();  // (a half step launched ahead may time out here, too)
  sync_eigen(c);
  c.h_wait_error[0] = 0;
  ++c.stats.wait_timeouts; ++g_runtime_stats.wait_timeouts;
  if (c.pipeline_off) fail(ICP_ERR_DEVICE, "internal: a step's first launch timed out on its word");
  c.pipeline_off = true;
  ++c.stats.pipeline_fallbacks; ++g_runtime_stats.pipeline_fallbacks;
  ++c.stats.step_redos; ++g_runtime_stats.step_redos;
  release_fronts(s.e);  // (lane 1 of a twin pass included: nothing of either lane has been recorded)
}

// 7: bookkeeping with the results in hand (chain_step_record), the step's slots given back, counters.  -> false: the step has to be
// done again
bool step_record(ChainStep& s, int* status) {
  icp_ctx& c = s.c;
  icp_evaluator* e = s.e;
  if (!chain_step_record(e, s.n_props, s.props, s.generator, s.theta_cur, s.F, s.f, s.theta_prop, s.log_value_prop, s.fwd, s.bwd, status)) {
    ++c.stats.step_redos; ++g_runtime_stats.step_redos;
    drop_twin(e);  // (lane 1 may have drawn from the same basis)
    return false;
  }
  if (s.lane1) ++c.twin_stats[1];
  s.F.s->reserved = false;
  for (int i = 0; i < s.n_props; ++i) s.F.ep[i]->reserved = false;
  s.front_guard.f = nullptr;
  ++c.paths.n[0]; ++g_step_paths.n[0];
  e->last_prop.assign(s.theta_prop, s.theta_prop + 10 + s.r);
  e->acc_counted = false;
  return true;
}

}  // namespace

extern "C" {

int icp_chain_step_prelaunch(icp_evaluator* e, int32_t n_props, icp_proposal* const* props, int32_t generator, const double* theta_cur,
                             const double* z_or_theta_prop) {
  return guard([&] { (void)chain_step_prelaunch(e, n_props, props, generator, theta_cur, z_or_theta_prop, -1, nullptr); });
}

int icp_chain_step_prelaunch2(icp_evaluator* e, int32_t n_props, icp_proposal* const* props, int32_t generator, const double* theta_cur,
                              const double* z_or_theta_prop, int32_t generator2, const double* z_or_theta_prop2, int32_t* lanes_issued) {
  if (lanes_issued) *lanes_issued = 0;
  return guard([&] {
    const int lanes = chain_step_prelaunch(e, n_props, props, generator, theta_cur, z_or_theta_prop, generator2, z_or_theta_prop2);
    if (lanes_issued) *lanes_issued = lanes;
  });
}

int icp_ctx_twin_stats(icp_ctx* ctx, int64_t out[3]) {
  return guard([&] {
    require(ctx && out, "null argument");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    for (int i = 0; i < 3; ++i) out[i] = ctx->twin_stats[i];
  });
}

int icp_ctx_search_hints(icp_ctx* ctx, icp_proposal* prop, int32_t n_surface, int32_t* surface_out, int32_t n_vertex, int32_t* vertex_out) {
  return guard([&] {
    require(ctx && n_surface >= 0 && n_vertex >= 0 && (n_surface == 0 || surface_out) && (n_vertex == 0 || vertex_out), "bad argument");
    require(n_surface <= ctx->N, "more surface hints asked for than the model has points");
    require(n_vertex == 0 || (prop && prop->ctx == ctx && n_vertex <= prop->K && prop->hint_nn.p), "vertex hints need a TargetSampling proposal of this context");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->bind();
    HIP_OK(hipDeviceSynchronize());  // (diagnostic: whatever was launched ahead has written its hints)
    if (n_surface) HIP_OK(hipMemcpy(surface_out, ctx->hint_surf.p, sizeof(int32_t) * n_surface, hipMemcpyDeviceToHost));
    if (n_vertex) HIP_OK(hipMemcpy(vertex_out, prop->hint_nn.p, sizeof(int32_t) * n_vertex, hipMemcpyDeviceToHost));
  });
}

int icp_ctx_twin_eigen_stats(icp_ctx* ctx, int64_t out[4]) {
  return guard([&] {
    require(ctx && out, "null argument");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    for (int i = 0; i < 4; ++i) out[i] = ctx->twin_eigen_stats[i];
  });
}

int icp_chain_step(icp_evaluator* e, int32_t n_props, icp_proposal* const* props, int32_t generator, const double* theta_cur,
                   const double* z, double* theta_prop, double* log_value_prop, double* fwd, double* bwd) {
  int status = ICP_OK;
  bool per_stage = false, redo = false, wide = false;
  static thread_local int wide_depth = 0;  // (a wide step that has to be repeated comes back through this entry point: bounded)
  int rc = guard([&] {
    require(e && theta_cur && theta_prop && log_value_prop, "null argument");
    require(n_props >= 0 && n_props <= 8 && (n_props == 0 || (props && fwd && bwd)), "bad proposal list");
    icp_ctx& c = *e->ctx;
    const double* key = generator >= 0 ? z : theta_prop;
    check_step_args(c, n_props, props, generator, theta_cur, key);
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    ChainStep s{e, n_props, props, generator, theta_cur, key, theta_prop, log_value_prop, fwd, bwd};
    if (!step_classify(s)) {
      // what the five merged launches do not cover as a configuration takes the wide step (a batch of one chain)
      per_stage = true;
      wide = wide_depth < 2 && n_props >= 1 && n_props <= 2 && !step_pipeline_covers(e, n_props, props) &&
             wide_chain_covered(e, n_props, props, generator, theta_cur, theta_prop);
      return;
    }
    Bound _b(&c, true);
    g_host_timing.start();
    step_take_front(s);
    g_host_timing.mark(0);
    if (!s.lane1) step_finish_launch(s);
    g_host_timing.mark(1);
    if (!s.lane1_eigen_out) step_speculate(s);
    // the caller's outcome-independent host work runs beside the device — first of all the pre-launch of the next step's
    // first half (under the rejection assumption), which the device can start as soon as the finish launch above has
    if (c.idle_fn) c.idle_fn(c.idle_arg);
    g_host_timing.mark(2);
    step_wait(s);
    g_host_timing.mark_wait(s.F.eigen_first_use);
    if (c.h_wait_error[0]) {
      step_first_launch_timed_out(s);
      redo = true;
      return;
    }
    redo = !step_record(s, &status);
    if (redo) return;
    g_host_timing.mark(4);
    g_host_timing.end();
  });
  if (rc != ICP_OK) return rc;
  if (redo) return icp_chain_step(e, n_props, props, generator, theta_cur, z, theta_prop, log_value_prop, fwd, bwd);
  if (per_stage && wide) {
    int32_t gen = generator, st = ICP_OK;
    const double* tc = theta_cur;
    const double* zz = z;
    double* tp = theta_prop;
    ++wide_depth;
    rc = icp_chain_step_batched(1, &e, n_props, props, &gen, &tc, generator >= 0 ? &zz : nullptr, &tp, log_value_prop, fwd, bwd, &st);
    --wide_depth;
    return rc != ICP_OK ? rc : st;
  }
  if (per_stage) {  // same results through the per-stage kernels
    ++e->ctx->paths.n[2]; ++g_step_paths.n[2];
    if (generator >= 0) {
      rc = icp_proposal_propose(props[generator], theta_cur, z, theta_prop, nullptr);
      if (rc != ICP_OK) return rc;
    }
    return icp_chain_eval_step(e, n_props, props, theta_cur, theta_prop, log_value_prop, fwd, bwd);
  }
  return status;
}

}  // extern "C"
