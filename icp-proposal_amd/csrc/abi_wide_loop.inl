// abi_wide_loop.inl — part of icp_abi.hip (one translation unit; included there, in order).
// --------------------------------------------------------------------- the whole MH loop on the device, WIDE step (MhWide)
// Chains whose step is the wide one (open targets, the Hausdorff evaluator, ranks 65..256: apps/bfm/BfmFittingPartial.scala:62-96,
// apps/femur/StdIcpVsChainICPrandomInitComparisonAll.scala at rank 101).  Per step the wide step's own launches, from records that live
// in device memory and are the same every step: the current state's posteriors stay in the entries they are in — an accepted state's
// M, alpha, coefficients and correspondence records are copied there (k_mhw_adopt) —, the proposed state always has the same slot and
// entries.  What changes per step (the proposal's inputs, the proposed state's pose) is set by k_mhw_front; k_mhw_decide is
// MetropolisHastings.next.  The records are wide_issue's own, captured (WideCapture).
//   ranks <= 64: groups of chains, each in order on one stream; the warm-started Jacobi iteration in place behind the decision;
//   ranks above: ONE group; behind the summed partials the step forks — factorisations + tails | the PROPOSED states' decompositions
//   (tridiagonal route, started ahead of the decision; an accepted state's basis is copied with its posterior) | the evaluator's
//   searches — and joins at the decision (tails) and at the hand-over (decompositions).  DESIGN.md §5.3b.
// The driver (wide_chains_run_on_device, at the end) reads: check → claim → per group capture, records, restate → per block of steps
// the normals and per step the head and one of two layouts → drain → book results; the scaffold is abi_loop_common.inl's.
namespace {

struct WideLoopChain {
  icp_evaluator* e = nullptr;
  icp_proposal* props[2] = {nullptr, nullptr};
  PosteriorEntry* cur[2] = {nullptr, nullptr};
  bool busy = false;
  bool unfilled = false;  // the current state's posteriors are not on record: filled by the run's first pass
};

struct WideLoopGroup : LoopGroup {
  icp_step_ticket ticket;   // (holds the captured step's reservations: state slot, the proposed state's entries)
  WideCapture cap;
  DBuf<char> wide_dev;
  DBuf<WideProposeItem> items;
  DBuf<MhWide> wide;
  DBuf<MhAdopt> adopt;
  DBuf<EigenProblem> eig_rec;
  std::vector<EigenRequest> rqs;   // (ranks above 64: the tridiagonal route's by-value requests …
  std::vector<const double*> spec_parts;  // … and the summed partials their matrices are assembled from)
  DBuf<double> given;
  std::vector<std::vector<double>> theta_prop_scratch;
  // (ranks above 64) the streams of the step's independent branches — the group's first chain's own — and the events between them
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_sum = nullptr, ev_tails = nullptr, ev_decide = nullptr, ev_prop = nullptr, ev_inst = nullptr, ev_eig[2] = {nullptr, nullptr};
  int n_eig_streams = 0;
  bool eig_split = false;
  ~WideLoopGroup() {
    for (hipEvent_t e : {ev_eig[0], ev_eig[1], ev_sum, ev_tails, ev_decide, ev_prop, ev_inst})
      if (e) (void)hipEventDestroy(e);
  }
};

// the developer / A-B switches of the loop (test-hooks and developer builds: dev_env), read once
struct WideLoopSwitches {
  int forced_groups;  // ICP_WIDE_LOOP_GROUPS (developer sweep)
  bool no_head;       // ICP_WIDE_LOOP_HEAD_SPLIT=0: the instance launch in one piece
  bool no_split;      // ICP_WIDE_LOOP_EIG_SPLIT=0: the decompositions in one piece, ahead of the decision
  bool chain_main;    // unless ICP_WIDE_LOOP_CHAIN_MAIN=0 (or no_split): the step's critical chain on one queue; else the forked layout
  bool timing;        // ICP_WIDE_LOOP_TIMING: the phases' host times on stderr
};
const WideLoopSwitches& wide_loop_switches() {
  static const auto is_zero = [](const char* name) { return dev_env(name) && std::atoi(dev_env(name)) == 0; };
  static const WideLoopSwitches sw{dev_env("ICP_WIDE_LOOP_GROUPS") ? std::atoi(dev_env("ICP_WIDE_LOOP_GROUPS")) : 0, is_zero("ICP_WIDE_LOOP_HEAD_SPLIT"),
                                   is_zero("ICP_WIDE_LOOP_EIG_SPLIT"), !is_zero("ICP_WIDE_LOOP_CHAIN_MAIN") && !is_zero("ICP_WIDE_LOOP_EIG_SPLIT"),
                                   dev_env("ICP_WIDE_LOOP_TIMING") != nullptr};
  return sw;
}

struct WideLoopPhases {  // (ICP_WIDE_LOOP_TIMING) host time since the phase before
  bool on;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[icp wide loop] %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// ---- claim the chains' contexts; the current state's posteriors and their bases, the ordinary way
void wide_loop_claim(const LoopRun& a, std::vector<WideLoopChain>& chains) {
  const int n_props = a.n_props, r = a.r;
  const icp_ctx& lead = *a.lead;
  for (int b = 0; b < a.n_chains; ++b) {
    WideLoopChain& ch = chains[b];
    require(a.evaluators[b] && a.theta[b], "null argument");
    icp_ctx& c = *a.evaluators[b]->ctx;
    require(c.device == lead.device && c.r == r && c.Qp.p == lead.Qp.p, "chains of one run share a device, a rank and (wide step) a model");
    for (int o = 0; o < b; ++o) require(chains[o].e->ctx != &c, "every chain needs a context of its own");
    ch.e = a.evaluators[b];
    for (int i = 0; i < n_props; ++i) {
      ch.props[i] = a.props_in[(size_t)b * n_props + i];
      require(ch.props[i] && ch.props[i]->ctx == &c, "proposal belongs to another context");
      require(ch.props[i]->sampler == a.props_in[0]->sampler, "one sampler per run");
    }
    check_theta_finite(&c, a.theta[b]);
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    if (c.batch_busy) fail(ICP_ERR_BUSY, "a chain's context already belongs to a batch in flight");
    require((!step_pipeline_covers(ch.e, n_props, ch.props) || !a.jacobi) && wide_pipeline_covers(ch.e, n_props, ch.props),
            "chains of one run take the same kind of step (this run: the wide one)");
    if (a.mix->w_pose > 0.0)
      require(c.rotations_mismatched == 0, "pose walks on the device: a caller-supplied rotation matrix disagreed with the library's Rz·Ry·Rx (icp_ctx_rotation_convention)");
    Bound _b(&c);
    // the context is this run's from here on: between this point and the captured step the locks are released and taken again, and
    // another thread's call on the context must be refused, not let in (release clears the mark).  (The merged loop, which keeps the
    // chain's lock over its whole claim, sets the mark at the claim's end.)
    c.batch_busy = true;
    ch.busy = true;
    release_fronts(ch.e);
    for (int i = 0; i < n_props; ++i) {
      icp_proposal* p = ch.props[i];
      p->resolve_speculation(a.theta[b]);
      // Above rank 64 a state whose posterior is not on record is NOT computed here, chain after chain the per-stage way (2.5 ms each
      // at rank 200): the captured step gets an empty entry for it, and one pass of the run's own launches fills the entries of all
      // chains at once (wide_loop_restate)
      if (!a.jacobi && !p->find_entry(a.theta[b])) { ch.unfilled = true; continue; }
      PosteriorEntry& cur = p->posterior(a.theta[b], false);
      p->ensure_eigen(cur);
      cur.reserved = true;
      ch.cur[i] = &cur;
    }
    if (ch.unfilled)
      for (int i = 0; i < n_props; ++i)
        if (ch.cur[i]) { ch.cur[i]->reserved = false; ch.cur[i] = nullptr; }  // (all of the chain's entries the same way)
  }
  // (… every chain's work is on its own streams by now, side by side: waited for and looked at chain by chain)
  for (int b = 0; b < a.n_chains; ++b) {
    WideLoopChain& ch = chains[b];
    icp_ctx& c = *ch.e->ctx;
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    Bound _b(&c, false, true);
    HIP_OK(hipStreamSynchronize(c.stream));
    c.front_stream.sync();
    sync_eigen(c);
    if (ch.unfilled) continue;
    for (int i = 0; i < n_props; ++i) sync_proposal_status(ch.props[i]);
    HIP_OK(hipStreamSynchronize(c.stream));
    for (int i = 0; i < n_props; ++i) {
      ch.props[i]->check_status(*ch.cur[i]);
      if (ch.props[i]->h_eig[ch.cur[i]->status_off / 3] != 0) fail(ICP_ERR_NOT_FINITE, "posterior eigen-decomposition did not converge");
      ch.cur[i]->eig_checked = true;
    }
  }
}

// what the contexts were claimed with goes back (after the guard, whatever its outcome)
void wide_loop_release(std::vector<WideLoopChain>& chains, std::vector<std::unique_ptr<WideLoopGroup>>& groups) {
  for (auto& gp : groups)
    if (gp)
      for (auto& it : gp->ticket.items) {
        if (!it.e) continue;
        std::lock_guard<std::recursive_mutex> lk(it.e->ctx->mu);
        wide_release(it);
      }
  for (auto& ch : chains) {
    if (!ch.e) continue;
    icp_ctx& c = *ch.e->ctx;
    std::lock_guard<std::recursive_mutex> lk(c.mu);
    for (int i = 0; i < 2; ++i)
      if (ch.cur[i]) ch.cur[i]->reserved = false;
    if (ch.busy) c.batch_busy = false;
  }
}

// ---- a group's stream(s): the first chain's three streams (see the merged loop's driver), above rank 64 the group's first chain's own
void wide_loop_streams(const LoopRun& a, std::vector<WideLoopChain>& chains, WideLoopGroup& gr, int g) {
  icp_ctx& lead = *a.lead;
  if (a.jacobi) gr.st = g == 0 ? lead.stream : g == 1 ? lead.front_stream.get() : lead.eig_stream.get();
  else {
    icp_ctx& gc = *chains[gr.b0].e->ctx;
    std::lock_guard<std::recursive_mutex> glk(gc.mu);  // (LazyStream::get makes the stream on first use: not without the context's lock)
    gr.st = gc.stream;
    gr.side[0] = gc.front_stream.get(); gr.side[1] = gc.eig_stream.get(); gr.side[2] = gc.eig_stream2.get();
    for (hipEvent_t* e : {&gr.ev_sum, &gr.ev_tails, &gr.ev_decide, &gr.ev_prop, &gr.ev_inst, &gr.ev_eig[0], &gr.ev_eig[1]})
      HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
}

// ---- the step of every chain of the group, captured: an ICP move from the current state
void wide_loop_capture(const LoopRun& a, std::vector<WideLoopChain>& chains, WideLoopGroup& gr, const std::vector<double>& zero_z) {
  const int B = gr.B, n_props = a.n_props;
  icp_step_ticket& t = gr.ticket;
  t.n_chains = B; t.n_props = n_props;
  t.items.resize(B);
  t.theta_cur.resize(B); t.theta_prop.resize(B); t.z.assign(B, zero_z.data());
  gr.theta_prop_scratch.assign(B, std::vector<double>(a.P, 0.0));
  std::vector<std::unique_lock<std::recursive_mutex>> locks;
  for (int k = 0; k < B; ++k) {
    WideLoopChain& ch = chains[gr.b0 + k];
    BatchItem& it = t.items[k];
    it.e = ch.e;
    it.props = a.props_in + (size_t)(gr.b0 + k) * n_props;
    it.generator = 0;
    it.key = zero_z.data();
    it.wide = true;
    t.theta_cur[k] = a.theta[gr.b0 + k];
    t.theta_prop[k] = gr.theta_prop_scratch[k].data();
    locks.emplace_back(ch.e->ctx->mu);
  }
  icp_ctx& glead = *chains[gr.b0].e->ctx;
  for (int k = 0; k < B; ++k)  // (entries of a chain that is filled below: not to be handed out as another's proposed-state entry)
    if (chains[gr.b0 + k].unfilled)
      for (int i = 0; i < n_props; ++i)
        if (PosteriorEntry* en = chains[gr.b0 + k].props[i]->find_entry(a.theta[gr.b0 + k])) en->off_record();
  gr.cap.allow_unfilled = !a.jacobi;
  wide_issue(t, glead, glead, &gr.cap);
  const WideCapture& cap = gr.cap;
  require((int)cap.chain_args.size() == B && (int)cap.prop_items.size() == B && (int)cap.factors.size() == B * n_props &&
          (int)cap.tails.size() == 2 * B * n_props, "internal: captured wide step is incomplete");
  for (int k = 0; k < B; ++k) {
    WideLoopChain& ch = chains[gr.b0 + k];
    WideItem& w = t.items[k].W;
    for (int i = 0; i < n_props; ++i) {
      if (ch.unfilled) ch.cur[i] = w.ec[i];
      require(w.ec[i] && w.ec[i] == ch.cur[i] && w.ep[i] && w.ep[i] != w.ec[i], "internal: captured wide step lost the current state's posterior");
      ch.cur[i]->reserved = true;
    }
  }
}

// the records of chain `k` of the group: its proposal item, MhWide, per proposal the hand-over and decomposition records, its MhChain
void wide_loop_chain_records(const LoopRun& a, WideLoopChain& ch, WideLoopGroup& gr, int k, WideProposeItem& item, MhWide& mw, MhChain& m,
                             MhAdopt* had, EigenProblem* hrec) {
  const int B = gr.B, n_props = a.n_props, r = a.r, root = a.root;
  const bool jacobi = a.jacobi;
  WideCapture& cap = gr.cap;
  icp_ctx& c = *ch.e->ctx;
  WideItem& w = gr.ticket.items[k].W;
  std::memset(&m, 0, sizeof(m));
  // W1: the copy of the proposed coefficients for the host (the record's last output, pinned memory) is not made
  item = cap.prop_items[k];
  item.n_out -= 1;
  item.kind = 0; item.src = gr.given.p + (size_t)k * r;
  std::memset(&mw, 0, sizeof(mw));
  mw.item = gr.items.p + k;
  mw.given = gr.given.p + (size_t)k * r;
  mw.inst = wide_inst_record(gr.wide_dev.p, B, k);
  mw.search[0] = wide_search_record(gr.wide_dev.p, B, 0, k);
  mw.search[1] = wide_search_record(gr.wide_dev.p, B, 1, k);
  for (int i = 0; i < n_props; ++i) {
    icp_proposal* p = ch.props[i];
    PosteriorEntry& cur = *w.ec[i];
    PosteriorEntry& prop = *w.ep[i];
    mw.prop_in[i] = ProposeIn{cur.alpha.p, cur.V.p, cur.S.p, c.inv_sqrt_lambda.p, c.P.p, cur.coeffs.p, nullptr, kSigma2, p->prm.step_length, root};
    MhAdopt ad{};
    ad.M_from = prop.M.p; ad.M_to = cur.M.p; ad.alpha_from = prop.alpha.p; ad.alpha_to = cur.alpha.p; ad.c_from = prop.coeffs.p; ad.c_to = cur.coeffs.p;
    // Ranks up to 64: the decomposition of the current state's posterior IN PLACE, behind the decision (an accepted state has just
    // arrived there; warm start: the basis that is there).  Above: the tridiagonal route — 0.7 ms at rank 200 — on the PROPOSED
    // state's entry, started as soon as the summed partials exist, beside the factorisation, the tails and the evaluator's
    // searches (as the host-stepped wide step decomposes ahead); an accepted state's basis moves with its posterior.
    PosteriorEntry& de = jacobi ? cur : prop;
    // (ranks above 64: no host status, no completion word — the loop looks at the status words on the device, in stream order)
    EigenRequest rq{de.M.p, (root || !jacobi) ? nullptr : cur.V.p, de.V.p, de.Vt.p, de.S.p, p->work.p, p->status.p + de.status_off + 2, nullptr,
                    jacobi ? p->h_eig + de.status_off / 3 : nullptr, jacobi ? p->eig_words.p + de.status_off / 3 : nullptr, 0, c.sqrt_lambda.p};
    rq.root = root != 0;
    gr.rqs[(size_t)k * n_props + i] = rq;
    EigenProblem ep{};
    if (jacobi) ep = eigen_problem_of(r, rq);
    else {
      ep.status = p->status.p + cur.status_off + 2;  // (k_mhw_decide looks at the CURRENT state's status word only)
      ad.V_from = prop.V.p; ad.V_to = cur.V.p; ad.Vt_from = prop.Vt.p; ad.Vt_to = cur.Vt.p; ad.S_from = prop.S.p; ad.S_to = cur.S.p;
      ad.st_from = p->status.p + prop.status_off + 2; ad.st_to = p->status.p + cur.status_off + 2;
    }
    {
      const CorrBuffers cf = prop.corr(), ct = cur.corr();
      const size_t K = (size_t)std::max(p->K, 0);
      const void* from[6] = {cf.id, cf.aux, cf.pt, cf.keep, cf.nhat, cf.e};
      void* to[6] = {ct.id, ct.aux, ct.pt, ct.keep, ct.nhat, ct.e};
      const size_t bytes[6] = {sizeof(int) * K, sizeof(int) * K, sizeof(double) * 3 * K, K, sizeof(double) * 3 * K, sizeof(double) * 3 * K};
      for (int u = 0; u < 6; ++u) {
        ad.corr_from[u] = (const unsigned char*)from[u]; ad.corr_to[u] = (unsigned char*)to[u];
        ad.corr_bytes[u] = (from[u] && to[u]) ? (int)bytes[u] : 0;
      }
    }
    had[i] = ad;
    hrec[i] = ep;
    m.eig_alt[0][i] = ep; m.eig_alt[1][i] = ep;
    // the tails' results and status words in DEVICE memory (the decide kernel reads them)
    TransitionTailIO& fw = cap.tails[2 * ((size_t)k * n_props + i)];
    TransitionTailIO& bw = cap.tails[2 * ((size_t)k * n_props + i) + 1];
    fw.out = gr.res.p + (size_t)k * 32 + 8 + 2 * i; fw.status = gr.stat.p + (size_t)k * 16 + 2 * i;
    bw.out = gr.res.p + (size_t)k * 32 + 9 + 2 * i; bw.status = gr.stat.p + (size_t)k * 16 + 2 * i + 1;
    mw.chol[i] = cap.factors[(size_t)k * n_props + i].status;
    m.eig_seq[i] = p->eig.place;
    p->eig.foreign_words_up_to(p->eig.place + a.n_steps);  // (as the merged loop: the words it may raise stay below the host's numbers)
  }
  m.wide = gr.wide.p + k;
  m.eig_live = gr.eig_rec.p + (size_t)k * n_props;
  loop_fill_chain(m, a, gr, k, ch.e->prm);
  m.front_every_step = 1;  // (every wide step's head is k_mhw_front's, pose walks or not; the merged loop sets it with pose walks only)
  m.eval_kind = ch.e->prm.kind;  // (the wide decide kernel knows all three evaluators; the merged one tells the independent one from the rest)
  m.coeff_prop = w.s->coeffs.p;
  m.red = c.d_res.p;  // (W8's reductions: device memory already)
  m.chol_status = nullptr;  // (MhWide::chol: the factorisations report into their proposals' own status buffers)
}

// ---- the group's device data: buffers, the captured records packed, the chains' records
void wide_loop_records(const LoopRun& a, std::vector<WideLoopChain>& chains, WideLoopGroup& gr) {
  const int B = gr.B, n_props = a.n_props;
  const size_t nq = (size_t)B * n_props;
  WideCapture& cap = gr.cap;
  gr.items.alloc(B); gr.wide.alloc(B);
  gr.adopt.alloc(nq); gr.eig_rec.alloc(nq);
  gr.given.alloc((size_t)B * a.r);
  gr.alloc(a);
  const size_t wbytes = wide_batch_bytes(B);
  gr.wide_dev.alloc(wbytes);
  std::vector<char> hw(wbytes, 0);
  wide_pack_args(B, cap.chain_args.data(), hw.data());
  std::vector<WideProposeItem> hitems(B);
  std::vector<MhWide> hwide(B);
  std::vector<MhChain> hm(B);
  std::vector<MhAdopt> had(nq);
  std::vector<EigenProblem> hrec(nq);
  gr.rqs.resize(nq);
  gr.spec_parts.resize(nq);
  for (size_t q = 0; q < nq; ++q) gr.spec_parts[q] = cap.factors[q].Mpart;
  for (int k = 0; k < B; ++k)
    wide_loop_chain_records(a, chains[gr.b0 + k], gr, k, hitems[k], hwide[k], hm[k], had.data() + (size_t)k * n_props, hrec.data() + (size_t)k * n_props);
  HIP_OK(hipMemcpy(gr.wide_dev.p, hw.data(), wbytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.items.p, hitems.data(), sizeof(WideProposeItem) * hitems.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.wide.p, hwide.data(), sizeof(MhWide) * hwide.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.adopt.p, had.data(), sizeof(MhAdopt) * had.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(gr.eig_rec.p, hrec.data(), sizeof(EigenProblem) * hrec.size(), hipMemcpyHostToDevice));
  gr.upload_start(a);
  HIP_OK(hipMemcpy(gr.mh.p, hm.data(), sizeof(MhChain) * hm.size(), hipMemcpyHostToDevice));
  HIP_OK(hipStreamSynchronize(nullptr));
}

// ---- the launches of a step, shared by the layouts below
void wide_factors(hipStream_t st, const LoopRun& a, const WideCapture& cap) {
  const size_t fmax = (size_t)posterior_factor_max();
  for (size_t p0 = 0; p0 < cap.factors.size(); p0 += fmax)
    launch_posterior_factor(st, a.r, (int)std::min(fmax, cap.factors.size() - p0), cap.factors.data() + p0);
}
void wide_tails(hipStream_t st, const LoopRun& a, const WideCapture& cap) {
  for (size_t t0 = 0; t0 < cap.tails.size(); t0 += 2 * kWideMaxChains)
    launch_transition_tails(st, a.r, (int)std::min<size_t>(2 * kWideMaxChains, cap.tails.size() - t0), cap.tails.data() + t0, a.lead->Ginv.p, kSigma2);
}
// the group's decompositions by the tridiagonal route, kTriManyMax requests per launch; launch `u` goes to stream_of(u) (which makes that
// stream wait for whatever its first launch needs); returns the number of launches
template <class StreamOf>
int wide_tridiag_launches(const LoopRun& a, const WideLoopGroup& gr, StreamOf stream_of, int part, const int* skip) {
  const int nq = gr.B * a.n_props;
  int used = 0;
  for (int q0 = 0; q0 < nq; q0 += kTriManyMax, ++used)
    launch_posterior_eigen_tridiag_many(stream_of(used), a.r, std::min(kTriManyMax, nq - q0), gr.rqs.data() + q0, gr.spec_parts.data() + q0,
                                        skip ? skip + q0 : nullptr, part);
  return used;
}
// the two decomposition streams of the forked layout, used in turn; each waits for `ev` before its first launch
auto wide_side_streams(const WideLoopGroup& gr, hipEvent_t ev) {
  return [&gr, ev](int used) {
    const hipStream_t E = gr.side[1 + (used & 1)];
    if (used < 2) HIP_OK(hipStreamWaitEvent(E, ev, 0));
    return E;
  };
}

// The step's head on the group's stream: front, proposals, the proposed states' instances, main sequence, summed partials; returns
// whether the instance launch went out in two parts (then ev_inst stands for its rest, on the second stream).
// The main sequence (the proposals' K model ids against the target, their regression) reads the first blocks of model points only —
// the ids and the corners of their triangles (plan.inst_head_blocks: wide_issue) — and goes ahead after those; the rest of the 28,561
// points and the spheres over them (0.1 ms for 25 chains, what the evaluator's searches read) are beside it on the second stream
// (round 6).  `restate`: the "proposal" is the current state itself, the instance launch in one piece.
bool wide_step_head(const LoopRun& a, WideLoopGroup& gr, bool restate) {
  const hipStream_t S = gr.st;
  const WideCapture& cap = gr.cap;
  launch_mhw_front(S, gr.B, gr.mh.p, restate ? 1 : 0);
  launch_wide_propose_resident(S, a.r, gr.B, gr.items.p);
  const bool head_split = !restate && gr.side[0] && cap.any_split && cap.plan.inst_head_blocks > 0 && !wide_loop_switches().no_head;
  if (head_split) {
    // (the rest BEHIND the head, not beside it: every wave of this launch walks the same 13 batches of basis rows, and with 1,788
    // of them resident the head's 36 finish when all do — 97 µs; alone they take a fraction of that)
    launch_wide_head_resident(S, cap.plan, gr.wide_dev.p, 1);
    HIP_OK(hipEventRecord(gr.ev_prop, S));
    HIP_OK(hipStreamWaitEvent(gr.side[0], gr.ev_prop, 0));
    launch_wide_head_resident(gr.side[0], cap.plan, gr.wide_dev.p, 2);
    HIP_OK(hipEventRecord(gr.ev_inst, gr.side[0]));
  } else launch_wide_head_resident(S, cap.plan, gr.wide_dev.p);
  launch_wide_main(S, cap.plan, gr.wide_dev.p);
  for (size_t p0 = 0; p0 < cap.sum_parts.size(); p0 += kWideMaxChains)
    launch_sum_partials_many(S, a.r, (int)std::min<size_t>(kWideMaxChains, cap.sum_parts.size() - p0), cap.sum_parts.data() + p0, cap.sum_splits.data() + p0);
  return head_split;
}

// What the summed partials feed does not depend on each other: the factorisations and tails (one-workgroup kernels), above rank 64
// the proposed states' decompositions, the evaluator's searches and reductions; the decision waits for the tails, the hand-over of
// an accepted state for the decompositions.
// Round 6 (ranks above 64): the step's critical chain — main sequence, reduction to tridiagonal form, eigenpairs, back-transformation,
// hand-over — stays on ONE queue: a dependency that crosses queues costs 20-30 µs between the end of one kernel and the start of the
// next (profiles/r06_wide_loop25_step_timeline.txt before: 30 µs at the fork, 20 at the join).  The first launch of decompositions
// goes on `S` itself, and what has slack — the evaluator's searches and the decision, 0.1 ms ahead of the reduction's end —
// crosses instead: on the first decomposition stream of the older layout (wide_step_forked: ICP_WIDE_LOOP_CHAIN_MAIN=0, the A/B switch).
void wide_step_chain_main(const LoopRun& a, WideLoopGroup& gr, bool head_split) {
  const hipStream_t S = gr.st, F = gr.side[0], V = gr.side[1], E1 = gr.side[2];
  const WideCapture& cap = gr.cap;
  HIP_OK(hipEventRecord(gr.ev_sum, S));
  HIP_OK(hipStreamWaitEvent(F, gr.ev_sum, 0));
  HIP_OK(hipStreamWaitEvent(V, gr.ev_sum, 0));
  const int used = wide_tridiag_launches(a, gr, [&](int u) {  // part 1: the reductions (see wide_step_forked)
    if (u == 1) HIP_OK(hipStreamWaitEvent(E1, gr.ev_sum, 0));
    return (u & 1) ? E1 : S;
  }, 1, nullptr);
  const bool side_eig = used > 1;
  gr.n_eig_streams = 0; gr.eig_split = true;
  wide_factors(F, a, cap);
  wide_tails(F, a, cap);
  HIP_OK(hipEventRecord(gr.ev_tails, F));
  if (head_split) HIP_OK(hipStreamWaitEvent(V, gr.ev_inst, 0));
  if (cap.any_split) launch_wide_eval(V, cap.plan, gr.wide_dev.p);
  HIP_OK(hipStreamWaitEvent(V, gr.ev_tails, 0));
  launch_mhw_decide(V, gr.B, a.r, gr.mh.p);
  HIP_OK(hipEventRecord(gr.ev_decide, V));
  HIP_OK(hipStreamWaitEvent(S, gr.ev_decide, 0));  // (long satisfied when the reduction ends)
  if (side_eig) HIP_OK(hipStreamWaitEvent(E1, gr.ev_decide, 0));
  wide_tridiag_launches(a, gr, [&](int u) { return (u & 1) ? E1 : S; }, 2, gr.eig_skip.p);  // part 2, for the chains that moved
  if (side_eig) {
    HIP_OK(hipEventRecord(gr.ev_eig[0], E1));
    HIP_OK(hipStreamWaitEvent(S, gr.ev_eig[0], 0));
  }
  launch_mhw_adopt(S, a.r, gr.B * a.n_props, gr.adopt.p, gr.eig_skip.p);
}

// The older layout, and ranks <= 64 (everything on `S`, the warm-started Jacobi iteration in place behind the hand-over): factorisations
// and tails on a second stream, the decompositions on two more — kTriManyMax per launch, the launches side by side —, the evaluator's
// sequence on `S`.
void wide_step_forked(const LoopRun& a, WideLoopGroup& gr, bool head_split) {
  const hipStream_t S = gr.st;
  const WideCapture& cap = gr.cap;
  const int nq = gr.B * a.n_props;
  hipStream_t S2 = S;
  if (gr.side[0]) {
    S2 = gr.side[0];
    HIP_OK(hipEventRecord(gr.ev_sum, S));
    HIP_OK(hipStreamWaitEvent(S2, gr.ev_sum, 0));
    // the proposed states' decompositions in two parts (round 6): the reduction to tridiagonal form — one workgroup per posterior,
    // 0.4 ms at rank 200 — starts here for every chain; the eigenpairs, back-transformation and refinement behind it are issued
    // BEHIND the decision (which falls while the reduction runs: tails and the evaluator's searches take 0.3 ms) and skip the
    // chains that did not move — half of them and more: the solve launch is the chip's throughput kernel (6,000 eigenpair waves
    // for 25 chains), and an accepted state's basis is all anybody will read
    const bool no_split = wide_loop_switches().no_split;
    const int used = wide_tridiag_launches(a, gr, wide_side_streams(gr, gr.ev_sum), no_split ? 0 : 1, nullptr);
    gr.n_eig_streams = std::min(used, 2);
    gr.eig_split = !no_split;
    if (no_split) for (int u = 0; u < gr.n_eig_streams; ++u) HIP_OK(hipEventRecord(gr.ev_eig[u], gr.side[1 + u]));
  }
  wide_factors(S2, a, cap);
  wide_tails(S2, a, cap);
  if (S2 != S) HIP_OK(hipEventRecord(gr.ev_tails, S2));
  if (head_split) HIP_OK(hipStreamWaitEvent(S, gr.ev_inst, 0));
  if (cap.any_split) launch_wide_eval(S, cap.plan, gr.wide_dev.p);
  if (S2 != S) HIP_OK(hipStreamWaitEvent(S, gr.ev_tails, 0));
  launch_mhw_decide(S, gr.B, a.r, gr.mh.p);
  if (gr.n_eig_streams > 0 && gr.eig_split) {  // (ranks above 64) part 2 of the decompositions, for the chains that moved
    HIP_OK(hipEventRecord(gr.ev_decide, S));
    wide_tridiag_launches(a, gr, wide_side_streams(gr, gr.ev_decide), 2, gr.eig_skip.p);
    for (int u = 0; u < gr.n_eig_streams; ++u) HIP_OK(hipEventRecord(gr.ev_eig[u], gr.side[1 + u]));
  }
  for (int u = 0; u < gr.n_eig_streams; ++u) HIP_OK(hipStreamWaitEvent(S, gr.ev_eig[u], 0));
  launch_mhw_adopt(S, a.r, nq, gr.adopt.p, gr.eig_skip.p);
  if (a.jacobi) launch_posterior_eigen_resident(S, a.r, nq, gr.eig_rec.p, gr.eig_skip.p, a.root);
}

// "restate": the current states' posteriors and bases of a group with unfilled entries, by the step's own launches — the proposal is
// the current state itself, its posterior lands in the proposed state's entries, is decomposed there and handed over like an accepted
// state's (every chain of the group: the values of an entry that was on record are computed again, the same)
void wide_loop_restate(const LoopRun& a, WideLoopGroup& gr) {
  const hipStream_t S = gr.st;
  const WideCapture& cap = gr.cap;
  wide_step_head(a, gr, true);
  HIP_OK(hipEventRecord(gr.ev_sum, S));
  const int used = wide_tridiag_launches(a, gr, wide_side_streams(gr, gr.ev_sum), 0, nullptr);
  for (int u = 0; u < std::min(used, 2); ++u) HIP_OK(hipEventRecord(gr.ev_eig[u], gr.side[1 + u]));
  wide_factors(S, a, cap);
  for (int u = 0; u < std::min(used, 2); ++u) HIP_OK(hipStreamWaitEvent(S, gr.ev_eig[u], 0));
  launch_mhw_adopt(S, a.r, gr.B * a.n_props, gr.adopt.p, nullptr);
  HIP_OK(hipStreamSynchronize(S));
  // the factorisations' and decompositions' status words, as the per-stage path would have looked at them
  for (size_t q = 0; q < cap.factors.size(); ++q) {
    int st[3] = {0, 0, 0};
    HIP_OK(hipMemcpy(st, cap.factors[q].status, sizeof(int) * 3, hipMemcpyDeviceToHost));
    if (st[0] != 0) fail(ICP_ERR_NOT_SPD, "posterior matrix is not positive definite");
    if (st[2] != 0) fail(ICP_ERR_NOT_FINITE, "posterior eigen-decomposition did not converge");
  }
}

// ---- results
// whatever the chain's entries hold now belongs to no state on record
void wide_loop_forget(const LoopRun& a, WideLoopChain& ch, WideItem& w) {
  std::lock_guard<std::recursive_mutex> lk(ch.e->ctx->mu);
  for (int i = 0; i < a.n_props; ++i) {
    for (PosteriorEntry* en : {w.ec[i], w.ep[i]})
      if (en) en->off_record();
    ch.props[i]->warm_valid = false;
    ch.props[i]->forget_speculation();
  }
  if (w.s) w.s->valid = false;
}

// nothing is handed out unless every chain came through: the chains' errors, then the decompositions behind the LAST step's decisions —
// they have no decide kernel behind them: their status (pinned, written by the decomposition itself) is looked at here
void wide_loop_check(const LoopRun& a, std::vector<WideLoopChain>& chains, std::vector<std::unique_ptr<WideLoopGroup>>& groups, int first_error) {
  if (first_error != 0) {
    for (auto& gp : groups)
      for (int k = 0; k < gp->B; ++k) wide_loop_forget(a, chains[gp->b0 + k], gp->ticket.items[k].W);
    loop_fail(first_error);
  }
  for (auto& gp : groups)
    for (int k = 0; k < gp->B; ++k) {
      WideLoopChain& ch = chains[gp->b0 + k];
      for (int i = 0; i < a.n_props; ++i) {
        int st = ch.props[i]->h_eig[ch.cur[i]->status_off / 3];
        if (!a.jacobi)  // (decomposed in the proposed state's entry: the status word came over with the basis, in device memory)
          HIP_OK(hipMemcpy(&st, ch.props[i]->status.p + ch.cur[i]->status_off + 2, sizeof(int), hipMemcpyDeviceToHost));
        if (st != 0) {
          wide_loop_forget(a, ch, gp->ticket.items[k].W);
          fail(ICP_ERR_NOT_FINITE, "on-device loop: posterior eigen-decomposition did not converge");
        }
      }
    }
}

// the contexts' own bookkeeping: the current state's entries are on record again, decomposed; nothing else of the run is
void wide_loop_book(const LoopRun& a, std::vector<WideLoopChain>& chains, WideLoopGroup& gr, const std::vector<MhChain>& hm) {
  for (int k = 0; k < gr.B; ++k) {
    const int b = gr.b0 + k;
    WideLoopChain& ch = chains[b];
    WideItem& w = gr.ticket.items[k].W;
    std::lock_guard<std::recursive_mutex> lk(ch.e->ctx->mu);
    for (int i = 0; i < a.n_props; ++i) {
      icp_proposal* p = ch.props[i];
      p->on_record(*w.ec[i], a.theta[b], a.P);
      w.ep[i]->off_record();
      p->forget_speculation();
      if (a.jacobi) p->eig.place = hm[k].eig_seq[i];
    }
    w.s->valid = false;
    loop_count_steps(ch.e, a.n_steps);
  }
}

int wide_chains_run_on_device(LoopRun& a) {
  std::vector<WideLoopChain> chains;
  std::vector<std::unique_ptr<WideLoopGroup>> groups;  // (outlive the guard: release reads their tickets; their buffers go after it)
  int rc = guard([&] {
    loop_check_args(a);
    const WideLoopSwitches& sw = wide_loop_switches();
    a.timing = sw.timing;
    WideLoopPhases phase{a.timing};
    chains.resize(a.n_chains);
    require(a.jacobi || (eigen_tridiag_many_supported(a.r) && !a.root),
            "the on-device loop of the wide step covers ranks 3..256 (the Cholesky-root sampler up to rank 64)");
    wide_loop_claim(a, chains);
    phase("claim (current states' posteriors and bases)");
    // ---- groups: each its own stream, everything of a group in order on it
    // (every launch of a wide step costs about the same whatever it carries — one-workgroup factorisations and reductions, searches
    // bound by their longest candidate list —: three groups of 10 face chains measured 7.8k it/s, one group of 30 7.2k with everything in
    // stream order, tools/r5_wide_loop_rate.sh.  Ranks above 64 therefore run as ONE group whose independent branches take streams of
    // their own — see the layouts —; the warm-started iteration of ranks <= 64 keeps the groups of the merged loop.)
    // (Two such groups a phase apart — one group's decompositions beside the other's searches — measured 2.4 ms per step of 30 face chains
    // against 1.7 with one: the chip-wide launches of one group hold up the other's one-workgroup kernels.)
    const int n_groups = sw.forced_groups > 0 ? std::min(std::min(sw.forced_groups, a.jacobi ? 3 : 2), a.n_chains)
                                              : (!a.jacobi ? 1 : a.n_chains >= 12 ? 3 : 1);
    groups.resize(n_groups);
    const std::vector<double> zero_z(a.r, 0.0);
    a.lead->bind();
    for (int g = 0; g < n_groups; ++g) {
      groups[g].reset(new WideLoopGroup());
      WideLoopGroup& gr = *groups[g];
      gr.set_range(g, n_groups, a.n_chains);
      wide_loop_streams(a, chains, gr, g);
      wide_loop_capture(a, chains, gr, zero_z);
      phase("capture");
      if (a.timing) std::fprintf(stderr, "[icp wide loop] instance head %d of %d blocks (any_split %d)\n", gr.cap.plan.inst_head_blocks, (gr.cap.plan.N + 63) / 64, (int)gr.cap.any_split);
      a.lead->bind();
      wide_loop_records(a, chains, gr);
      phase("records");
      if (gr.cap.any_unfilled) {
        wide_loop_restate(a, gr);
        phase("restate (current states' posteriors, all chains at once)");
      }
    }
    const int n_blocks = (a.n_steps + kLoopChunk - 1) / kLoopChunk;
    LoopProfBind prof_bind(*a.lead);
    const auto t_loop0 = std::chrono::steady_clock::now();
    for (int blk = 0; blk < n_blocks; ++blk) {
      const int ns = std::min(kLoopChunk, a.n_steps - blk * kLoopChunk);
      for (auto& gp : groups) loop_feed_normals(*gp, a, blk);
      for (int s_ = 0; s_ < ns; ++s_)
        for (auto& gp : groups) {
          const bool head_split = wide_step_head(a, *gp, false);
          if (gp->side[0] && sw.chain_main) wide_step_chain_main(a, *gp, head_split);
          else wide_step_forked(a, *gp, head_split);
        }
    }
    // ---- results
    std::vector<std::vector<MhChain>> hms(n_groups);
    int first_error = 0;
    const auto t_enq = std::chrono::steady_clock::now();
    for (int g = 0; g < n_groups; ++g)
      first_error = loop_drain(*groups[g], hms[g], first_error, [&] {
        if (g == n_groups - 1 && a.timing)
          std::fprintf(stderr, "[icp wide loop] %d chains x %d steps: enqueue %.1f ms, drain %.1f ms\n", a.n_chains, a.n_steps,
                       std::chrono::duration<double, std::milli>(t_enq - t_loop0).count(),
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq).count());
      });
    wide_loop_check(a, chains, groups, first_error);
    for (int g = 0; g < n_groups; ++g) {
      loop_hand_out(*groups[g], a, hms[g]);
      wide_loop_book(a, chains, *groups[g], hms[g]);
    }
  });
  wide_loop_release(chains, groups);
  return rc;
}

}  // namespace
