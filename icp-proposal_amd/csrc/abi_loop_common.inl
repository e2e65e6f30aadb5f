// abi_loop_common.inl — part of icp_abi.hip (one translation unit; included there, in order).
// What the two on-device MH loops (abi_wide_loop.inl: the wide step's; abi_device_loop.inl: the merged step's) share: a run's arguments
// and their checks, the loop-independent part of an MhChain, a group's buffers, the harness' standard normals and their feed, the drain with
// its error mapping and the hand-out of results.  Plain functions and small structs; what the loops do differently on purpose stays at
// their call sites.  (A posterior entry that leaves or re-enters the record: PosteriorEntry::off_record, icp_proposal::on_record.)
namespace {

constexpr int kLoopChunk = 64;  // steps per block of standard normals

// StepRandom::normal of the C++ harness (host/icp_host.hpp; = orc_rng_normal of the oracle): Box–Muller over the counter-based uniforms
inline uint64_t harness_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
inline double harness_uniform(uint64_t seed, uint64_t step, uint64_t lane) {
  const uint64_t h = harness_splitmix64(harness_splitmix64(harness_splitmix64(seed) ^ (step * 0xD1342543DE82EF95ull)) ^ (lane * 0x2545F4914F6CDD1Dull));
  return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
inline double harness_normal(uint64_t seed, uint64_t step, uint64_t lane) {
  const double u1 = harness_uniform(seed, step, 2 * lane + 1000), u2 = harness_uniform(seed, step, 2 * lane + 1001);
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
}

// the arguments of icp_chains_run_on_device and the constants both loops derive from them (loop_check_args)
struct LoopRun {
  int32_t n_chains; icp_evaluator* const* evaluators; int32_t n_props; icp_proposal* const* props_in; const icp_mh_mixture* mix;
  const uint64_t* seeds; const int64_t* first_step; double* const* theta; double* log_value; int32_t n_steps; double* const* records;
  int64_t* accepted;
  icp_ctx* lead = nullptr;  // the first chain's context
  int r = 0, P = 0, root = 0;
  bool jacobi = false;  // the rank's decomposition is the warm-started one-workgroup Jacobi iteration (ranks <= 64)
  bool timing = false;  // (wide loop, ICP_WIDE_LOOP_TIMING)
};

void loop_check_args(LoopRun& a) {
  require(a.n_chains >= 1 && a.evaluators && a.props_in && a.mix && a.seeds && a.first_step && a.theta && a.log_value && a.n_steps >= 0, "null argument");
  require(a.n_props >= 1 && a.n_props <= 2, "the on-device loop takes one or two ICP proposals per chain");
  require(a.mix->struct_size == sizeof(icp_mh_mixture), "icp_mh_mixture::struct_size does not match this library's header");
  require(a.mix->w_icp > 0.0 && a.mix->w_rw >= 0.0 && a.mix->rw_sigma > 0.0 && a.mix->w_pose >= 0.0, "bad mixture");
  if (a.mix->w_pose > 0.0)
    for (int i = 0; i < 3; ++i) require(a.mix->pose_rot_sigma[i] > 0.0 && a.mix->pose_trans_sigma[i] > 0.0, "pose walk sigmas must be positive");
  a.lead = a.evaluators[0]->ctx;
  a.r = a.lead->r; a.P = 10 + a.r;
  a.root = a.props_in[0] && a.props_in[0]->sampler == ICP_SAMPLER_CHOLESKY_ROOT;  // (one sampler per run: the claims check it)
  a.jacobi = eigen_speculation_supported(a.r);
}

// ---- a group of chains: everything of a group in order on one stream.  Each loop's group derives from this and adds its own records
struct LoopGroup {
  int b0 = 0, B = 0;
  hipStream_t st = nullptr;
  DBuf<MhChain> mh;
  DBuf<int> eig_skip;
  DBuf<double> normals[2], theta, rec;
  DBuf<double> res;   // per chain 32 doubles: [0..7] the evaluator's reductions (merged loop), [8..11] the tails fwd_i / bwd_i — in DEVICE memory
  DBuf<int> stat;     // per chain 16 ints: [0..3] the tails' status, [8..9] the factorisations' (merged loop) (the decide kernel reads
                      // them: pinned host memory, where the host-stepped paths want them, would cost it a bus round trip per number)
  double* h_normals[2] = {nullptr, nullptr};
  hipEvent_t ev_copy[2] = {nullptr, nullptr};
  ~LoopGroup() {
    for (int k = 0; k < 2; ++k) {
      if (h_normals[k]) pinned_free(h_normals[k]);
      if (ev_copy[k]) (void)hipEventDestroy(ev_copy[k]);
    }
  }
  void set_range(int g, int n_groups, int n_chains) {
    b0 = (int)((long long)g * n_chains / n_groups);
    B = (int)((long long)(g + 1) * n_chains / n_groups) - b0;
  }
  void alloc(const LoopRun& a) {
    const size_t nb = (size_t)B;
    mh.alloc(nb);
    eig_skip.alloc(nb * a.n_props);
    theta.alloc(nb * a.P);
    res.alloc(nb * 32); res.fill_bytes(0);
    stat.alloc(nb * 16); stat.fill_bytes(0);
    rec.alloc(a.records ? nb * std::max(a.n_steps, 1) * (4 + a.P) : 1);
    for (int k = 0; k < 2; ++k) {
      normals[k].alloc(nb * kLoopChunk * a.r);
      pinned_alloc((void**)&h_normals[k], sizeof(double) * nb * kLoopChunk * a.r);
      HIP_OK(hipEventCreateWithFlags(&ev_copy[k], hipEventDisableTiming));
    }
  }
  // the records that every chain of the group starts with: nothing of a decomposition is skipped yet, the chains' states
  void upload_start(const LoopRun& a) {
    std::vector<int> hskip((size_t)B * a.n_props, 1);
    std::vector<double> hth((size_t)B * a.P);
    for (int k = 0; k < B; ++k) std::memcpy(hth.data() + (size_t)k * a.P, a.theta[b0 + k], sizeof(double) * a.P);
    HIP_OK(hipMemcpy(eig_skip.p, hskip.data(), sizeof(int) * hskip.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(theta.p, hth.data(), sizeof(double) * hth.size(), hipMemcpyHostToDevice));
  }
};

// the loop-independent part of chain `k` of the group: seed, mixture, pose walks, shape walk, evaluator constants, where its tails,
// records and state live.  The doubles enter the decide kernel: the expressions and their order are the host harness' own.
// (MhChain::front_every_step and ::eval_kind are the loops' own: set at the call sites)
void loop_fill_chain(MhChain& m, const LoopRun& a, const LoopGroup& gr, int k, const icp_evaluator_params& ep) {
  const icp_mh_mixture* mix = a.mix;
  const int r = a.r, b = gr.b0 + k;
  m.eig_skip = gr.eig_skip.p + (size_t)k * a.n_props;
  m.pw_id_mask = 2046;
  m.seed = a.seeds[b];
  m.r = r; m.n_icp = a.n_props;
  {  // MixtureProposal weights, normalised as the harness normalises them (host/icp_host.hpp: pick_component)
    double ws = 0.0;
    for (int i = 0; i < a.n_props; ++i) ws += mix->icp_weight[i];
    for (int i = 0; i < a.n_props; ++i) m.icp_w[i] = mix->icp_weight[i] / ws;
    double raw[3];
    int no = 0;
    if (mix->w_pose > 0.0) { m.outer_kind[no] = 0; raw[no++] = mix->w_pose; }  // (BfmFittingPartial.scala:70: pose, ICP, shape walk)
    m.outer_kind[no] = 1; raw[no++] = mix->w_icp;
    if (mix->w_rw > 0.0) { m.outer_kind[no] = 2; raw[no++] = mix->w_rw; }
    double wsum = 0.0;
    for (int o = 0; o < no; ++o) wsum += raw[o];
    for (int o = 0; o < no; ++o) m.outer_w[o] = raw[o] / wsum;
    m.n_outer = no;
  }
  if (mix->w_pose > 0.0) {  // MixedProposalDistributions.scala:29-39 / host/icp_host.cpp: mixed_random_pose_proposal
    static const int param_index[6] = {6, 5, 4, 1, 2, 3};  // yaw = rotation._3, pitch = _2, roll = _1 (PoseProposals.scala:39-41); x, y, z
    m.n_pose = 6;
    double wsum = 0.0;
    for (int i = 0; i < 6; ++i) wsum += 0.5;  // (the harness' own expression)
    for (int i = 0; i < 6; ++i) {
      const double sd = i < 3 ? mix->pose_rot_sigma[i] : mix->pose_trans_sigma[i - 3];
      m.pose_index[i] = param_index[i];
      m.pose_w[i] = 0.5 / wsum;
      m.pose_sigma[i] = sd;
      m.pose_logc[i] = std::log(std::sqrt(2.0 * M_PI)) + std::log(sd);  // breeze Gaussian(0, σ).logPdf's normaliser
    }
  }
  m.rw_sigma = mix->rw_sigma;
  m.rw_logc = 0.5 * (r * std::log(2.0 * M_PI) + r * std::log(mix->rw_sigma * mix->rw_sigma));
  m.prior_c = 0.5 * r * std::log(2.0 * M_PI);
  m.eval_mode = ep.mode;
  m.gauss_mean = ep.gauss_mean; m.gauss_sigma = ep.gauss_sigma;
  m.gauss_logn = std::log(std::sqrt(2.0 * M_PI)) + std::log(ep.gauss_sigma);
  m.exp_rate = ep.exp_rate; m.exp_lograte = std::log(ep.exp_rate);
  m.tails = gr.res.p + (size_t)k * 32 + kResTails;
  m.tail_status = gr.stat.p + (size_t)k * 16 + kStatTails;
  // (normals: the two buffers are addressed through MhChain::normals / normals_first, re-pointed per block of steps: loop_feed_normals)
  m.normals = nullptr; m.normals_first = 0; m.normals_rows = 0;
  m.records = a.records && a.records[b] ? gr.rec.p + (size_t)k * a.n_steps * (4 + a.P) : nullptr;
  m.rec_first = a.first_step[b];
  m.theta = gr.theta.p + (size_t)k * a.P;
  m.cur_p = a.log_value[b];
  m.step = a.first_step[b];
  m.accepted = 0; m.cur_sel = 0; m.gen = -1; m.leaf = -1; m.error = 0;
}

// ---- per block of kLoopChunk steps the chains' standard normals: the harness' own expression, drawn here on the host while the
// device works on the block before, uploaded behind the group's launches and handed to its chains
void loop_feed_normals(LoopGroup& gr, const LoopRun& a, int blk) {
  const int buf = blk & 1, s0 = blk * kLoopChunk, ns = std::min(kLoopChunk, a.n_steps - s0), r = a.r;
  HIP_OK(hipEventSynchronize(gr.ev_copy[buf]));  // (the staging buffer's previous upload has left it)
  double* out = gr.h_normals[buf];
  for (int k = 0; k < gr.B; ++k) {
    const uint64_t seed = a.seeds[gr.b0 + k];
    const uint64_t f0 = (uint64_t)a.first_step[gr.b0 + k] + (uint64_t)s0;
    for (int s_ = 0; s_ < ns; ++s_)
      for (int j = 0; j < r; ++j) out[((size_t)k * kLoopChunk + s_) * r + j] = harness_normal(seed, f0 + (uint64_t)s_, (uint64_t)j);
  }
  HIP_OK(hipMemcpyAsync(gr.normals[buf].p, gr.h_normals[buf], sizeof(double) * (size_t)gr.B * kLoopChunk * r, hipMemcpyHostToDevice, gr.st));
  HIP_OK(hipEventRecord(gr.ev_copy[buf], gr.st));
  launch_mh_set_normals(gr.st, gr.B, gr.mh.p, gr.normals[buf].p, kLoopChunk * r, s0, ns);
}

// (per-kernel event timing, if the first chain's context is being profiled: icp_ctx_profile_start — its event pool)
struct LoopProfBind { explicit LoopProfBind(icp_ctx& c) { g_prof = c.profiling ? &c.prof : nullptr; } ~LoopProfBind() { g_prof = nullptr; } };

// ---- results
// waits for the group's stream and fetches its chains; returns the first chain error seen so far (`drained`: called once the stream is idle)
template <class Drained>
int loop_drain(LoopGroup& gr, std::vector<MhChain>& hm, int first_error, Drained drained) {
  HIP_OK(hipStreamSynchronize(gr.st));
  drained();
  hm.resize(gr.B);
  HIP_OK(hipMemcpy(hm.data(), gr.mh.p, sizeof(MhChain) * hm.size(), hipMemcpyDeviceToHost));
  for (const MhChain& m : hm)
    if (m.error != 0 && first_error == 0) first_error = m.error;
  return first_error;
}

// MhChain::error (k_mh_decide / k_mhw_decide) as the call's error
[[noreturn]] void loop_fail(int first_error) {
  fail(first_error == 3 ? ICP_ERR_NOT_SPD : first_error == 5 ? ICP_ERR_EMPTY : ICP_ERR_NOT_FINITE,
       first_error == 2 ? "on-device loop: a transition tail did not contract (step these chains through icp_chain_step_batched)"
       : first_error == 6 ? "on-device loop: posterior eigen-decomposition did not converge"
                          : "on-device loop: a chain stopped on a non-finite, empty or non-positive-definite result");
}

// the group's states, log values, acceptance counts and records to the caller
void loop_hand_out(const LoopGroup& gr, const LoopRun& a, const std::vector<MhChain>& hm) {
  std::vector<double> hth((size_t)gr.B * a.P);
  HIP_OK(hipMemcpy(hth.data(), gr.theta.p, sizeof(double) * hth.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < gr.B; ++k) {
    const int b = gr.b0 + k;
    std::memcpy(a.theta[b], hth.data() + (size_t)k * a.P, sizeof(double) * a.P);
    a.log_value[b] = hm[k].cur_p;
    if (a.accepted) a.accepted[b] = hm[k].accepted;
    if (a.records && a.records[b] && a.n_steps > 0)
      HIP_OK(hipMemcpy(a.records[b], gr.rec.p + (size_t)k * a.n_steps * (4 + a.P), sizeof(double) * (size_t)a.n_steps * (4 + a.P), hipMemcpyDeviceToHost));
  }
}

// a chain's steps on the context's and the library's counters (under the context's lock)
void loop_count_steps(icp_evaluator* e, int n_steps) {
  e->last_prop.clear();
  e->ctx->paths.n[3] += n_steps; g_step_paths.n[3] += n_steps;
}

}  // namespace
