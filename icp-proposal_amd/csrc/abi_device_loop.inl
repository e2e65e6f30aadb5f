// abi_device_loop.inl — part of icp_abi.hip (one translation unit; included there, in order).
// C ABI: icp_chains_run_on_device — the whole MH loop on the device (MhChain, kernels_step.hip).  Here: the loop of chains whose step
// is the MERGED one (five launches, ranks <= 64 on closed targets) and the entry point with its dispatch to the wide step's loop
// (abi_wide_loop.inl).  The driver (at the end) reads: check → claim → per group the captured records → per block of steps the normals
// and per step the enqueue with the token → drain → book results; the scaffold is abi_loop_common.inl's.
namespace {

struct MergedLoopChain {
  icp_evaluator* e = nullptr;
  icp_proposal* props[2] = {nullptr, nullptr};
  PosteriorEntry* set[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [sel][proposal]
  StateSlot* slot = nullptr;
  std::unique_lock<std::recursive_mutex> lk;
  bool busy = false;
};

struct MergedLoopGroup : LoopGroup {
  int grid[5] = {0, 0, 0, 0, 0};
  DBuf<StepBeginArgs> begin_alt, begin_live;
  DBuf<StepSearchArgs> search_alt, search_live;
  bool filter_prepared = true;  // (step_filter_prepared of every captured step)
  bool reg_folded = false;      // (the captured regressions fold their leaves: regression_fold)
  DBuf<StepRegressionArgs> regression_alt, regression_live;
  DBuf<StepFinishArgs> finish_alt, finish_live;
  DBuf<EigenProblem> eig_live;
  hipEvent_t ev_big = nullptr;  // recorded behind the token's launch: the next group's chip-wide launches may start
  ~MergedLoopGroup() { if (ev_big) (void)hipEventDestroy(ev_big); }
};

// ---- claim the chains' contexts, fix their posterior entries and state slot
void merged_loop_claim(const LoopRun& a, std::vector<MergedLoopChain>& chains) {
  const int n_props = a.n_props, r = a.r;
  const icp_ctx& lead = *a.lead;
  for (int b = 0; b < a.n_chains; ++b) {
    MergedLoopChain& ch = chains[b];
    require(a.evaluators[b] && a.theta[b], "null argument");
    icp_ctx& c = *a.evaluators[b]->ctx;
    require(c.device == lead.device && c.r == r, "chains of one run share a device and a rank");
    for (int o = 0; o < b; ++o) require(chains[o].e->ctx != &c, "every chain needs a context of its own");
    ch.e = a.evaluators[b];
    for (int i = 0; i < n_props; ++i) {
      ch.props[i] = a.props_in[(size_t)b * n_props + i];
      require(ch.props[i] && ch.props[i]->ctx == &c, "proposal belongs to another context");
      require(ch.props[i]->sampler == ch.props[0]->sampler && ch.props[i]->sampler == chains[0].props[0]->sampler, "one sampler per run");
    }
    check_theta_finite(&c, a.theta[b]);
    ch.lk = std::unique_lock<std::recursive_mutex>(c.mu);
    if (c.batch_busy) fail(ICP_ERR_BUSY, "a chain's context already belongs to a batch in flight");
    require(step_pipeline_covers(ch.e, n_props, ch.props), "configuration not covered by the merged launches");
    // (the device makes the proposed pose's matrix with the library's own convention: open to a host whose supplied matrices have
    // all agreed with it — icp_ctx_set_rotation's check —, closed to one whose convention is another)
    if (a.mix->w_pose > 0.0)
      require(c.rotations_mismatched == 0, "pose walks on the device: a caller-supplied rotation matrix disagreed with the library's Rz·Ry·Rx (icp_ctx_rotation_convention)");
    Bound _b(&c);
    release_fronts(ch.e);
    for (int i = 0; i < n_props; ++i) {
      icp_proposal* p = ch.props[i];
      p->resolve_speculation(a.theta[b]);
      PosteriorEntry& cur = p->posterior(a.theta[b], false);  // the current state's posterior and its basis, the ordinary way
      p->ensure_eigen(cur);
      cur.reserved = true;
      ch.set[0][i] = &cur;
      PosteriorEntry& other = p->fresh_entry();
      other.reserved = true;
      ch.set[1][i] = &other;
    }
    HIP_OK(hipStreamSynchronize(c.stream));
    c.front_stream.sync();
    sync_eigen(c);
    for (int i = 0; i < n_props; ++i) sync_proposal_status(ch.props[i]);
    HIP_OK(hipStreamSynchronize(c.stream));
    for (int i = 0; i < n_props; ++i) {
      ch.props[i]->check_status(*ch.set[0][i]);
      if (ch.props[i]->h_eig[ch.set[0][i]->status_off / 3] != 0) fail(ICP_ERR_NOT_FINITE, "posterior eigen-decomposition did not converge");
    }
    StateSlot& s = c.fresh_state();
    s.reserved = true;
    s.pose = c.pose_of(a.theta[b]);
    ch.slot = &s;
    // (the chain's lock is held over the whole claim: the mark goes up at its end.  The wide loop, whose claim lets go of the lock in
    // between, sets it at the start.)
    c.batch_busy = true;
    ch.busy = true;
    ch.lk.unlock();
  }
}

// what the contexts were claimed with goes back (after the guard, whatever its outcome)
void merged_loop_release(std::vector<MergedLoopChain>& chains) {
  for (auto& ch : chains) {
    if (!ch.e) continue;
    icp_ctx& c = *ch.e->ctx;
    if (!ch.lk.owns_lock()) ch.lk = std::unique_lock<std::recursive_mutex>(c.mu);
    for (int sel = 0; sel < 2; ++sel)
      for (int i = 0; i < 2; ++i)
        if (ch.set[sel][i]) ch.set[sel][i]->reserved = false;
    if (ch.slot) ch.slot->reserved = false;
    if (ch.busy) c.batch_busy = false;
    ch.lk.unlock();
  }
}

// the records of chain `k` of the group: the step's five launches captured twice — with the current state in set `sel` and the proposed
// one in the other (rows sel·B + k of hb / hs / hr / hf) —, the proposals' inputs and decompositions of either set, its MhChain
void merged_loop_chain_records(const LoopRun& a, MergedLoopChain& ch, MergedLoopGroup& gr, int k, const std::vector<double>& zero_key,
                               StepBeginArgs* hb, StepSearchArgs* hs, StepRegressionArgs* hr, StepFinishArgs* hf, MhChain& m) {
  const int B = gr.B, n_props = a.n_props, r = a.r, root = a.root;
  icp_ctx& c = *ch.e->ctx;
  std::lock_guard<std::recursive_mutex> lk(c.mu);
  Bound _b(&c, true, true);
  std::memset(&m, 0, sizeof(m));
  for (int sel = 0; sel < 2; ++sel) {
    StepCapture cap;
    std::memset(cap.grid, 0, sizeof(cap.grid));
    StepFront F;
    F.n_props = n_props; F.generator = -1; F.parity = 0; F.stream = c.stream; F.s = ch.slot;
    for (int i = 0; i < n_props; ++i) { F.props[i] = ch.props[i]; F.ec[i] = ch.set[sel][i]; F.ep[i] = ch.set[1 - sel][i]; }
    {
      struct CaptureScope { CaptureScope(StepCapture* cp) { step_capture(cp); } ~CaptureScope() { step_capture(nullptr); } } scope(&cap);
      front_launches(ch.e, n_props, ch.props, -1, zero_key.data(), F, true, false);
      StepFinishArgs f = step_finish_args(c, n_props, ch.props, F, gr.res.p + (size_t)k * 32, gr.stat.p + (size_t)k * 16);
      f.done_counter = c.d_done.p; f.host_flag = c.h_flag;  // (seq 0, no ready word: nobody waits for a step of the loop)
      launch_step_finish(c.stream, f);  // (captured; finalised by the launcher)
    }
    cap.begin.wait_flag = nullptr; cap.begin.wait2_flag = nullptr; cap.begin.wait_ticks = nullptr; cap.begin.hold_regs = 0;
    cap.regression.red_out = gr.res.p + (size_t)k * 32;  // (device memory instead of the context's pinned area)
    cap.begin.tpr_log2 = matvec_tpr_log2(r, 256);  // (launch 1's matvec layout: front_launches sets it only when it knows the generator)
    const size_t row = (size_t)sel * B + k;
    hb[row] = cap.begin; hs[row] = cap.search; hr[row] = cap.regression; hf[row] = cap.finish;
    for (int q = 0; q < 5; ++q) gr.grid[q] = std::max(gr.grid[q], cap.grid[q]);
    gr.filter_prepared = gr.filter_prepared && step_filter_prepared(cap.search);
    for (int i = 0; i < cap.regression.n && i < 2; ++i)  // (any folded record of any chain: the folded kernel takes both kinds)
      gr.reg_folded = gr.reg_folded || cap.regression.fold[i] > 1;
    m.begin_alt[sel] = gr.begin_alt.p + row;
    m.search_alt[sel] = gr.search_alt.p + row;
    m.regression_alt[sel] = gr.regression_alt.p + row;
    m.finish_alt[sel] = gr.finish_alt.p + row;
    for (int i = 0; i < n_props; ++i) {
      icp_proposal* p = ch.props[i];
      PosteriorEntry& cur = *ch.set[sel][i];
      m.prop_alt[sel][i] = ProposeIn{cur.alpha.p, cur.V.p, cur.S.p, c.inv_sqrt_lambda.p, c.P.p, cur.coeffs.p, nullptr, kSigma2,
                                     p->prm.step_length, root};
      // the decomposition of set `sel`'s posterior (an accepted state arrives there), warm-started from the other set's basis
      PosteriorEntry& other = *ch.set[1 - sel][i];
      EigenRequest rq{cur.M.p, root ? nullptr : other.V.p, cur.V.p, cur.Vt.p, cur.S.p, p->work.p, p->status.p + cur.status_off + 2, nullptr,
                      p->h_eig + cur.status_off / 3, p->eig_words.p + cur.status_off / 3, 0, c.sqrt_lambda.p};
      rq.root = root != 0;
      m.eig_alt[sel][i] = eigen_problem_of(r, rq);
    }
  }
  m.begin_live = gr.begin_live.p + k; m.search_live = gr.search_live.p + k;
  m.regression_live = gr.regression_live.p + k; m.finish_live = gr.finish_live.p + k;
  m.eig_live = gr.eig_live.p + (size_t)k * n_props;
  loop_fill_chain(m, a, gr, k, ch.e->prm);
  // (later steps of a block are prepared by the decide kernel of the step before — except with pose walks, whose proposed pose is made by
  // the front kernel; the wide loop's head is the front kernel's every step)
  if (a.mix->w_pose > 0.0) m.front_every_step = 1;
  // (the merged launches cover the independent and the collective evaluator — step_pipeline_covers —: k_mh_decide tells 0 from the
  // rest; the wide loop passes the kind on as it is)
  m.eval_kind = ch.e->prm.kind == ICP_EVAL_INDEPENDENT_POINT_DISTANCE ? 0 : 2;
  m.coeff_prop = ch.slot->coeffs.p;
  m.red = gr.res.p + (size_t)k * 32;
  m.chol_status = gr.stat.p + (size_t)k * 16 + kStatFactor;
  // (the loop counts on from the place and raises the completion words of the set's entries to the places it takes, at most one per
  // step: the host's numbers stay above them whatever becomes of the loop — booked, forgotten or failed)
  for (int i = 0; i < n_props; ++i) {
    m.eig_seq[i] = ch.props[i]->eig.place;
    ch.props[i]->eig.foreign_words_up_to(ch.props[i]->eig.place + a.n_steps);
  }
  for (int i = 0; i < 16; ++i) { c.h_res[i] = 0.0; c.h_status[i] = 0; }
}

// ---- the group's device data: buffers, both alternatives of every chain's launches, the chains' records
void merged_loop_records(const LoopRun& a, std::vector<MergedLoopChain>& chains, MergedLoopGroup& gr, const std::vector<double>& zero_key) {
  const int B = gr.B, n_props = a.n_props;
  struct FoldScope { FoldScope(int n) { tl_regression_posteriors = n; } ~FoldScope() { tl_regression_posteriors = 1; } } fold_scope(std::max(1, B * n_props));
  struct SearchHintScope2 { SearchHintScope2(int n) { search_chains_hint(n); } ~SearchHintScope2() { search_chains_hint(1); } } search_hint_scope2(B);
  gr.begin_alt.alloc(2 * B); gr.begin_live.alloc(B);
  gr.search_alt.alloc(2 * B); gr.search_live.alloc(B);
  gr.regression_alt.alloc(2 * B); gr.regression_live.alloc(B);
  gr.finish_alt.alloc(2 * B); gr.finish_live.alloc(B);
  gr.eig_live.alloc((size_t)B * n_props);
  HIP_OK(hipEventCreateWithFlags(&gr.ev_big, hipEventDisableTiming));
  gr.alloc(a);
  std::vector<StepBeginArgs> hb(2 * B);
  std::vector<StepSearchArgs> hs(2 * B);
  std::vector<StepRegressionArgs> hr(2 * B);
  std::vector<StepFinishArgs> hf(2 * B);
  std::vector<MhChain> hm(B);
  for (int k = 0; k < B; ++k) merged_loop_chain_records(a, chains[gr.b0 + k], gr, k, zero_key, hb.data(), hs.data(), hr.data(), hf.data(), hm[k]);
  HIP_OK(hipMemcpy(gr.begin_alt.p, hb.data(), sizeof(StepBeginArgs) * hb.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.search_alt.p, hs.data(), sizeof(StepSearchArgs) * hs.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.regression_alt.p, hr.data(), sizeof(StepRegressionArgs) * hr.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.finish_alt.p, hf.data(), sizeof(StepFinishArgs) * hf.size(), hipMemcpyHostToDevice));
  gr.upload_start(a);
  HIP_OK(hipMemcpy(gr.mh.p, hm.data(), sizeof(MhChain) * hm.size(), hipMemcpyHostToDevice));
  HIP_OK(hipStreamSynchronize(nullptr));  // (as DBuf::upload: the copies have reached the device before a non-blocking stream's launch reads them)
}

// One step of group `g`: eight launches on its stream, nothing waited for (`first`: the run's first step of its first group; `front`:
// the step's head is the front kernel's — a block's first step, and every step with pose walks).
// The chip-wide launches of two groups side by side slow each other down more than the overlap gains; what
// should run beside a group's chip-wide launches is the OTHER group's small ones (launch 5 on four CUs per chain, the
// decide kernel, the decompositions on three CUs each).  So the launches pass a token from group to group: a group's first
// launch waits for an event of the previous group's.  Which one: behind launch 4 while the filter launch held five workgroups per
// CU; with eight (§5.1c) behind launch 2 — the other group's begin and filter beside this group's resolve and regression, two
// chains of latencies that leave the CUs room — measures best (two groups of 32 chains: 202.0k it/s against 197.3k behind launch
// 4, 199.0k without a token; four groups of 16, on a build with a fourth stream: 216.2k against 215.0k behind launch 1, 206.3k
// without, 199.6k behind launch 3, 167.9k behind launch 4); behind launch 1 with 64 per group (two groups of 64: 249.5k against 244.7k / 241.5k).
void merged_loop_step(const LoopRun& a, std::vector<MergedLoopGroup>& groups, int g, bool first, bool front) {
  const int n_groups = (int)groups.size(), r = a.r;
  MergedLoopGroup& gr = groups[g];
  if (n_groups > 1) {
    MergedLoopGroup& prev = groups[(g + n_groups - 1) % n_groups];
    if (!first) HIP_OK(hipStreamWaitEvent(gr.st, prev.ev_big, 0));
  }
  if (front) launch_mh_front(gr.st, gr.B, gr.mh.p);
  const int token_at = gr.B >= 64 ? 1 : 2;
  {
    int ga[5] = {0, 0, 0, 0, 0}, gb[5] = {0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) (q < token_at ? ga : gb)[q] = gr.grid[q];
    if (token_at > 0)
      launch_step_batch_resident(gr.st, gr.B, ga, r, gr.begin_live.p, gr.search_live.p, gr.regression_live.p, gr.finish_live.p, gr.filter_prepared, gr.reg_folded);
    if (n_groups > 1) HIP_OK(hipEventRecord(gr.ev_big, gr.st));
    if (token_at < 4)
      launch_step_batch_resident(gr.st, gr.B, gb, r, gr.begin_live.p, gr.search_live.p, gr.regression_live.p, gr.finish_live.p, gr.filter_prepared, gr.reg_folded);
  }
  int g5[5] = {0, 0, 0, 0, gr.grid[4]};
  launch_step_batch_resident(gr.st, gr.B, g5, r, gr.begin_live.p, gr.search_live.p, gr.regression_live.p, gr.finish_live.p);
  launch_mh_decide(gr.st, gr.B, gr.mh.p);
  launch_posterior_eigen_resident(gr.st, r, gr.B * a.n_props, gr.eig_live.p, gr.eig_skip.p, a.root);
}

// ---- results
// whatever the sets of proposal `i` hold now belongs to no state on record
void merged_loop_forget(MergedLoopChain& ch, int i) {
  // (the entries' events and completion words — the claim's own decomposition may have left them — stay as they are)
  for (int sel = 0; sel < 2; ++sel) ch.set[sel][i]->off_record(false);
  ch.props[i]->warm_valid = false;
  ch.props[i]->forget_speculation();
}

// nothing is handed out unless every chain came through: the chains' errors, then the decompositions behind the LAST step's decisions —
// they have no decide kernel behind them: their status (pinned, written by the decomposition itself) is looked at here, before the
// sets are booked as decomposed and checked
void merged_loop_check(const LoopRun& a, std::vector<MergedLoopChain>& chains, const std::vector<MergedLoopGroup>& groups,
                       const std::vector<std::vector<MhChain>>& hms, int first_error) {
  if (first_error != 0) {
    for (auto& ch : chains) {
      std::lock_guard<std::recursive_mutex> lk(ch.e->ctx->mu);
      for (int i = 0; i < a.n_props; ++i) merged_loop_forget(ch, i);
      ch.slot->valid = false;
    }
    loop_fail(first_error);
  }
  for (size_t g = 0; g < groups.size(); ++g)
    for (int k = 0; k < groups[g].B; ++k) {
      MergedLoopChain& ch = chains[groups[g].b0 + k];
      for (int i = 0; i < a.n_props; ++i)
        if (ch.props[i]->h_eig[ch.set[hms[g][k].cur_sel][i]->status_off / 3] != 0) {
          std::lock_guard<std::recursive_mutex> lk(ch.e->ctx->mu);
          merged_loop_forget(ch, i);
          fail(ICP_ERR_NOT_FINITE, "on-device loop: posterior eigen-decomposition did not converge");
        }
    }
}

// the contexts' own bookkeeping: the set that holds the current state is on record again, decomposed
void merged_loop_book(const LoopRun& a, std::vector<MergedLoopChain>& chains, const MergedLoopGroup& gr, const std::vector<MhChain>& hm) {
  for (int k = 0; k < gr.B; ++k) {
    const int b = gr.b0 + k;
    MergedLoopChain& ch = chains[b];
    const MhChain& m = hm[k];
    std::lock_guard<std::recursive_mutex> lk(ch.e->ctx->mu);
    for (int i = 0; i < a.n_props; ++i) {
      icp_proposal* p = ch.props[i];
      for (int sel = 0; sel < 2; ++sel) {
        if (sel == m.cur_sel) p->on_record(*ch.set[sel][i], a.theta[b], a.P);
        else ch.set[sel][i]->off_record();
      }
      p->forget_speculation();
      p->eig.place = m.eig_seq[i];
    }
    ch.slot->valid = false;
    loop_count_steps(ch.e, a.n_steps);
  }
}

int merged_chains_run_on_device(LoopRun& a) {
  std::vector<MergedLoopChain> chains;
  int rc = guard([&] {
    loop_check_args(a);
    chains.resize(a.n_chains);
    require(a.jacobi, "the on-device loop covers ranks 3..64");
    merged_loop_claim(a, chains);
    // ---- groups: each its own stream, everything of a group in order on it; the groups overlap each other's launches
    // (three since the token moved forward, §5.1c: 64 chains 202k it/s in two groups, 211k in three; 128 chains 251k / 257k; 32 chains 130k /
    // 135k; 24 chains 104k / 108k.  Four — a fourth stream made with every context — measured 218k / 266k / 137k / 109k, but the extra
    // stream shifts every context's streams over the runtime's hardware queues, and the host-stepped lockstep path's decompositions, which
    // wait on the device for launches of other streams, then ran into their time-outs: 15 of them in a 50-chain test.  Not adopted.)
    const int n_groups = a.n_chains >= 16 ? 3 : 1;
    std::vector<MergedLoopGroup> groups(n_groups);  // (inside the guard: their buffers go before release)
    icp_ctx& lead = *a.lead;
    lead.bind();
    const std::vector<double> zero_key(a.P, 0.0);
    for (int g = 0; g < n_groups; ++g) {
      MergedLoopGroup& gr = groups[g];
      gr.set_range(g, n_groups, a.n_chains);
      // the first chain's three streams: created one after the other with the context, they sit on different hardware queues and run
      // beside each other (streams of DIFFERENT contexts, or streams made later, may share a queue: the runtime multiplexes streams
      // onto a handful of them, and two groups on one queue alternate in ~55 µs slices — every kernel of the step then "takes" a
      // multiple of that: eight streams made for the purpose on first use ran two groups at 116k it/s instead of 202k)
      gr.st = g == 0 ? lead.stream : g == 1 ? lead.front_stream.get() : lead.eig_stream.get();
      merged_loop_records(a, chains, gr, zero_key);
    }
    // ---- the loop: per block of kLoopChunk steps the chains' standard normals, then per step and group eight launches
    const int n_blocks = (a.n_steps + kLoopChunk - 1) / kLoopChunk;
    LoopProfBind prof_bind(lead);
    for (int blk = 0; blk < n_blocks; ++blk) {
      const int ns = std::min(kLoopChunk, a.n_steps - blk * kLoopChunk);
      for (auto& gr : groups) loop_feed_normals(gr, a, blk);
      for (int s_ = 0; s_ < ns; ++s_)
        for (int g = 0; g < n_groups; ++g) merged_loop_step(a, groups, g, blk == 0 && s_ == 0 && g == 0, s_ == 0 || a.mix->w_pose > 0.0);
    }
    // ---- results
    std::vector<std::vector<MhChain>> hms(n_groups);
    int first_error = 0;
    for (int g = 0; g < n_groups; ++g) first_error = loop_drain(groups[g], hms[g], first_error, [] {});
    merged_loop_check(a, chains, groups, hms, first_error);
    for (int g = 0; g < n_groups; ++g) {
      loop_hand_out(groups[g], a, hms[g]);
      merged_loop_book(a, chains, groups[g], hms[g]);
    }
  });
  merged_loop_release(chains);
  return rc;
}

}  // namespace

extern "C" {

int icp_chains_run_on_device(int32_t n_chains, icp_evaluator* const* evaluators, int32_t n_props, icp_proposal* const* props_in,
                             const icp_mh_mixture* mix, const uint64_t* seeds, const int64_t* first_step, double* const* theta,
                             double* log_value, int32_t n_steps, double* const* records, int64_t* accepted) {
  LoopRun a{n_chains, evaluators, n_props, props_in, mix, seeds, first_step, theta, log_value, n_steps, records, accepted};
  // chains whose step is the wide one (an open target, the Hausdorff evaluator, a rank above 64): the loop of their own
  if (n_chains >= 1 && evaluators && evaluators[0] && props_in && props_in[0] && n_props >= 1 && n_props <= 2) {
    bool wide = false, ok = true;
    for (int i = 0; i < n_props; ++i) ok = ok && props_in[i] && props_in[i]->ctx == evaluators[0]->ctx;
    if (ok) {
      std::lock_guard<std::recursive_mutex> lk(evaluators[0]->ctx->mu);
      // (… or the five merged launches at a rank whose decomposition is not the one-workgroup Jacobi iteration — ranks 65..116,
      // apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala at rank 101: the wide step's kernels compute the same step)
      wide = (!step_pipeline_covers(evaluators[0], n_props, props_in) || !eigen_speculation_supported(evaluators[0]->ctx->r)) &&
             wide_pipeline_covers(evaluators[0], n_props, props_in);
    }
    if (wide) return wide_chains_run_on_device(a);
  }
  return merged_chains_run_on_device(a);
}

}  // extern "C"
