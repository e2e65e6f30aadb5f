// abi_variability_many.inl — C ABI: icp_posterior_variability_many, the posterior variability maps of many chains' samples
// (kernels_variability.hip, launch_instance_many; apps/util/PosteriorVariability.scala:30-73).
//
// Map m's out is, bit for bit, what icp_posterior_variability(ctxs[m], n_samples[m], thetas[m], modes[m], theta_refs[m], ·) gives.
// The sample meshes pass through ONE chunk buffer of kVarChunkDoubles doubles, round by round: a round holds the samples of as many
// whole maps as fit, or one segment of a map that is larger than the buffer.  Such a map runs its segments twice — once for the sums
// (mean, mode-2 normal), once for the centred moments, its meshes instanced again — because the mean needs every sample before the
// first centred term; a map within one round is instanced once and both sweeps read the parked meshes.  What a map carries from
// segment to segment (Σ x, Σ n, the moments: 10 N doubles) lives in its own buffers.  Device memory: the chunk buffer, 10 N doubles
// per map and the samples' coefficients and poses — no sample mesh outlives its round.  Everything is enqueued on the first context's
// stream: four launches per round at most, however many maps and models the round holds, and ONE synchronisation per call.

namespace {
constexpr size_t kVarChunkDoubles = (size_t)8 << 20;  // the chunk buffer: 64 MiB of sample meshes (and mode-2 sample normals)
constexpr int kVarMaxRoundSamples = 32768;            // meshes per round (every launch's grid.y stays below 65,536)
}  // namespace

extern "C" {

int icp_posterior_variability_many(int32_t n_maps, icp_ctx* const* ctxs, const int32_t* n_samples, const double* const* thetas,
                                   const int32_t* modes, const double* const* theta_refs, double* const* out, double* const* mean_out) {
  return guard([&] {
    require(n_maps >= 0, "n_maps is negative");
    if (n_maps == 0) return;
    require(n_maps <= 65535, "at most 65,535 maps a call");
    require(ctxs && n_samples && thetas && modes && out, "null argument");
    const int B = n_maps;
    for (int m = 0; m < B; ++m) {
      require(ctxs[m] && thetas[m] && out[m], "null argument");
      require(n_samples[m] >= 2, "at least two samples are needed");
      require(modes[m] >= 0 && modes[m] <= 2, "unknown mode");
      require(modes[m] != 1 || (theta_refs && theta_refs[m]), "theta_ref is null");
    }
    require_one_device(B, ctxs, "maps of one call share a device");
    size_t n_inst = 0, n_coeffs = 0;  // meshes to instance (samples and mode-1 references) and their coefficients
    for (int m = 0; m < B; ++m) {
      const size_t P = 10 + (size_t)ctxs[m]->r;
      require_finite(thetas[m], (size_t)n_samples[m] * P, "theta contains a non-finite value");
      if (modes[m] == 1) require_finite(theta_refs[m], P, "theta contains a non-finite value");
      const size_t k = (size_t)n_samples[m] + (modes[m] == 1 ? 1 : 0);
      n_inst += k;
      n_coeffs += k * (size_t)ctxs[m]->r;
    }
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    icp_ctx& lead = *ctxs[0];
    Bound _b(&lead);
    hipStream_t st = lead.stream;

    // ---- the maps' own buffers: [res of every map | mean of every map | nrm, acc per map]
    struct MapBuf { size_t res, mean, nrm, acc; };
    std::vector<MapBuf> mb(B);
    size_t sumN = 0, cap = test_chunk_doubles("ICP_TEST_VARIABILITY_CHUNK_DOUBLES", kVarChunkDoubles);
    int Nmax = 1;
    for (int m = 0; m < B; ++m) sumN += (size_t)ctxs[m]->N;
    {
      size_t o_res = 0, o_mean = sumN, o_rest = 4 * sumN;
      for (int m = 0; m < B; ++m) {
        const size_t N = (size_t)ctxs[m]->N;
        mb[m] = MapBuf{o_res, o_mean, o_rest, o_rest + 3 * N};
        o_res += N; o_mean += 3 * N; o_rest += 6 * N;
        Nmax = std::max(Nmax, ctxs[m]->N);
        cap = std::max(cap, 6 * N);  // (a mesh and its normals always fit)
      }
    }
    DBuf<double> state, chunk, coeffs;
    state.alloc(10 * sumN);
    chunk.alloc(cap);
    {
      PackedCoeffs hc(n_coeffs);  // per map: its mode-1 reference, then its samples
      for (int m = 0; m < B; ++m) {
        const int r = ctxs[m]->r;
        if (modes[m] == 1) hc.add(theta_refs[m], r);
        for (int s = 0; s < n_samples[m]; ++s) hc.add(thetas[m] + (size_t)s * (10 + (size_t)r), r);
      }
      hc.upload(coeffs);
    }

    // ---- the plan: records of every mesh, group, normal job and segment; rounds = ranges of them
    struct Round { size_t g0, g1, j0, j1, s0, s1, c0, c1; };  // groups, normal jobs, sum segments, centred segments
    InstancePlan inst;
    const std::vector<InstanceGroup>& h_grp = inst.groups;
    std::vector<VarNormalJob> h_job;
    std::vector<VarSeg> h_sum, h_cen;
    std::vector<Round> rounds;
    inst.items.reserve(n_inst);
    size_t used = 0, co = 0;  // the open round: doubles of the chunk buffer taken, coefficient cursor
    int held = 0;             // … and meshes
    auto open_round = [&] { rounds.push_back(Round{h_grp.size(), h_grp.size(), h_job.size(), h_job.size(), h_sum.size(), h_sum.size(), h_cen.size(), h_cen.size()}); used = 0; held = 0; };
    auto close_round = [&] { Round& rd = rounds.back(); rd.g1 = h_grp.size(); rd.j1 = h_job.size(); rd.s1 = h_sum.size(); rd.c1 = h_cen.size(); };
    auto add_meshes = [&](icp_ctx& c, const double* th, const double* cf, int n, double* x) {  // n consecutive thetas -> x[n][3N], in groups of their own
      const size_t P = 10 + (size_t)c.r, n3 = 3 * (size_t)c.N;
      inst.boundary();
      for (int s = 0; s < n; ++s) inst.add(c, cf + (size_t)s * c.r, c.pose_of(th + (size_t)s * P), x + (size_t)s * n3);
    };
    open_round();
    for (int m = 0; m < B; ++m) {
      icp_ctx& c = *ctxs[m];
      const int S = n_samples[m], mode = modes[m];
      const size_t n3 = 3 * (size_t)c.N, P = 10 + (size_t)c.r, per = mode == 2 ? 2 * n3 : n3, extra = mode == 1 ? n3 : 0;
      double* sb = state.p;
      VarSeg seg{};
      seg.N = c.N; seg.S = S; seg.mode = mode;
      seg.mean = sb + mb[m].mean; seg.nrm = mode != 0 ? sb + mb[m].nrm : nullptr; seg.acc = sb + mb[m].acc; seg.out = sb + mb[m].res;
      seg.nscale = 1.0 / S;
      const double* cf = coeffs.p + co;
      co += ((size_t)S + (mode == 1 ? 1 : 0)) * c.r;
      const bool whole = extra + (size_t)S * per <= cap && S + 1 <= kVarMaxRoundSamples;
      if (whole && (used + extra + (size_t)S * per > cap || held + S + 1 > kVarMaxRoundSamples)) { close_round(); open_round(); }
      if (!whole && held > 0) { close_round(); open_round(); }
      if (mode == 1) {  // the reference's mesh, into the open round; its normals are the map's
        add_meshes(c, theta_refs[m], cf, 1, chunk.p + used);
        h_job.push_back(VarNormalJob{chunk.p + used, c.tris.p, c.adj_off.p, c.adj.p, c.N, seg.nrm});
        cf += c.r; used += n3; ++held;
      }
      auto add_segment = [&](int s0, int n, bool sums, bool centred) {
        double* x = chunk.p + used;
        double* ns = x + (size_t)n * n3;
        add_meshes(c, thetas[m] + (size_t)s0 * P, cf + (size_t)s0 * c.r, n, x);
        seg.n = n; seg.x = x; seg.nsm = mode == 2 ? ns : nullptr;
        seg.first = s0 == 0; seg.last = s0 + n == S;
        if (sums) {
          if (mode == 2)
            for (int s = 0; s < n; ++s) h_job.push_back(VarNormalJob{x + (size_t)s * n3, c.tris.p, c.adj_off.p, c.adj.p, c.N, ns + (size_t)s * n3});
          h_sum.push_back(seg);
        }
        if (centred) h_cen.push_back(seg);
        used += (size_t)n * per; held += n;
      };
      if (whole) { add_segment(0, S, true, true); continue; }
      // a map larger than the buffer: a round per segment, first all sums, then all centred moments
      for (int sweep = 0; sweep < 2; ++sweep)
        for (int s0 = 0; s0 < S;) {
          const int n = (int)std::min<size_t>({(size_t)(S - s0), (cap - used) / per, (size_t)(kVarMaxRoundSamples - held)});
          if (n == 0) { close_round(); open_round(); continue; }  // (only behind the reference's mesh: a fresh round holds a sample)
          add_segment(s0, n, sweep == 0, sweep == 1);
          s0 += n;
          close_round(); open_round();
        }
    }
    close_round();

    DBuf<InstanceItem> d_smp;
    DBuf<InstanceGroup> d_grp;
    DBuf<VarNormalJob> d_job;
    DBuf<VarSeg> d_sum, d_cen;
    {
      NullStreamBatch _nb;
      inst.upload(d_smp, d_grp);
      if (!h_job.empty()) d_job.upload(h_job.data(), h_job.size());
      d_sum.upload(h_sum.data(), h_sum.size());
      d_cen.upload(h_cen.data(), h_cen.size());
    }
    // ---- launches
    for (const Round& rd : rounds) {
      launch_instance_many(st, (int)(rd.g1 - rd.g0), Nmax, d_grp.p + rd.g0, d_smp.p);
      launch_var_normals(st, (int)(rd.j1 - rd.j0), Nmax, d_job.p + rd.j0);
      launch_var_sum(st, (int)(rd.s1 - rd.s0), Nmax, d_sum.p + rd.s0);
      launch_var_centred(st, (int)(rd.c1 - rd.c0), Nmax, d_cen.p + rd.c0);
    }
    bool want_mean = false;
    if (mean_out)
      for (int m = 0; m < B; ++m) want_mean = want_mean || mean_out[m] != nullptr;
    std::vector<double> hr((want_mean ? 4 : 1) * sumN);
    HIP_OK(hipMemcpyAsync(hr.data(), state.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, st));
    lead.finish(0, 0);
    for (int m = 0; m < B; ++m) {
      const size_t N = (size_t)ctxs[m]->N;
      std::memcpy(out[m], &hr[mb[m].res], sizeof(double) * N);
      if (want_mean && mean_out[m]) std::memcpy(mean_out[m], &hr[mb[m].mean], sizeof(double) * 3 * N);
    }
  });
}

}  // extern "C"
