// abi_fit_many.inl — C ABI: icp_fit_deterministic_many, many deterministic ICP fits in lockstep (kernels_fit.hip).
//
// Fit b is what icp_fit_deterministic gives when it is called once per recursion (n_iterations = 0, one sigma2, that recursion's
// direction), each theta_out chained into the next theta_init — with every recursion of every fit enqueued up front on the first
// context's stream and ONE synchronisation at the end.  Per recursion: instances (launch_instance_many: one pass over the basis per
// kInstGroup fits),
// search initialisation, filter, resolve + correspondence rows, regression partial sums, factorisations (launch_posterior_factor, up
// to posterior_factor_max() a launch), mean steps.  Every fit's work is split as the one-fit path splits it (search tasks made by the
// same makers, regression_splits of the fit's own K), so a fit's bits do not depend on the other fits of the call or their order.

extern "C" {

int icp_fit_deterministic_many(int32_t n_fits, icp_ctx* const* ctxs, const icp_fit_params* const* params, const double* const* theta_init,
                               const uint8_t* directions, int32_t n_iterations, int32_t n_sigma, const double* sigma2_seq,
                               double* const* theta_out, int32_t* status) {
  std::vector<int> fit_status;
  int rc = guard([&] {
    require(n_fits > 0 && ctxs && params && theta_init && theta_out && status && sigma2_seq, "null argument");
    require(n_fits <= 65535, "at most 65,535 fits a call");
    require(n_iterations >= 0 && n_sigma >= 0, "negative iteration count");
    for (int i = 0; i < n_sigma; ++i) require(sigma2_seq[i] > 0.0 && std::isfinite(sigma2_seq[i]), "sigma2 must be positive");
    const int B = n_fits;
    const size_t R = (size_t)n_sigma * ((size_t)n_iterations + 1);  // recursions per fit
    for (int b = 0; b < B; ++b) require(ctxs[b] && params[b] && theta_init[b] && theta_out[b], "null argument");
    icp_ctx& lead = *ctxs[0];
    require_one_model(B, ctxs, "fits of one call share a device and a model");
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    const int r = lead.r, N = lead.N;
    require(r <= 512, "ranks up to 512 (the mean step keeps alpha in LDS)");
    const size_t P = 10 + (size_t)r;
    // ---- validation: nothing runs and no theta_out is written unless every fit's arguments are good
    std::vector<uint8_t> dirs((size_t)B * R);
    std::vector<char> uses_m(B, 0), uses_t(B, 0);
    for (int b = 0; b < B; ++b) {
      const icp_fit_params& p = *params[b];
      const icp_ctx& c = *ctxs[b];
      require_finite(theta_init[b], P, "theta_init contains a non-finite value");
      require(std::isfinite(p.step_length), "step_length must be finite");
      for (size_t s = 0; s < R; ++s) {
        const int d = directions ? directions[(size_t)b * R + s] : p.direction;
        require(d == ICP_MODEL_SAMPLING || d == ICP_TARGET_SAMPLING, "unknown direction");
        dirs[(size_t)b * R + s] = (uint8_t)d;
        (d == ICP_MODEL_SAMPLING ? uses_m : uses_t)[b] = 1;
      }
      if (uses_m[b]) {
        require(p.n_model_ids > 0 && p.model_ids, "a fit that samples the model needs model ids");
        require(c.target.T > 0 && c.target.spheres.p, "the target has no triangles");
        for (int k = 0; k < p.n_model_ids; ++k) require(p.model_ids[k] >= 0 && p.model_ids[k] < N, "model id out of range");
      }
      if (uses_t[b]) require(p.n_target_points > 0 && p.target_points, "a fit that samples the target needs target points");
    }
    fit_status.assign(B, ICP_OK);
    if (R == 0) {  // no recursion: theta_out = theta_init
      for (int b = 0; b < B; ++b) std::memmove(theta_out[b], theta_init[b], sizeof(double) * P);
      return;
    }
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    // ---- per-fit scratch, one block per kind with the largest fit's stride (sized per call)
    int km = 1, kt = 1, kmax = 1, Smax = 1;
    size_t cand = 1;
    for (int b = 0; b < B; ++b) {
      const int m = uses_m[b] ? params[b]->n_model_ids : 0, t = uses_t[b] ? params[b]->n_target_points : 0;
      km = std::max(km, m); kt = std::max(kt, t); kmax = std::max(kmax, std::max(m, t));
      if (m) Smax = std::max(Smax, regression_splits(m));
      if (t) Smax = std::max(Smax, regression_splits(t));
      if (m) cand = std::max(cand, (size_t)(query_kpad(m) + 4) * cand_stride(ctxs[b]->target.T));
      if (t) cand = std::max(cand, (size_t)(query_kpad(t) + 4) * cand_stride(N));
    }
    const int kmpad = query_kpad(km), ktpad = query_kpad(kt), kpad = std::max(kmpad, ktpad);
    const size_t nn = (size_t)(r + 1) * (r + 1), fsz = (size_t)(r + 1) * r + 8;
    DBuf<double> coeffs, x, Pm, tpts, thr2, pt, nhat, e, Mpart, M, alpha, fscratch;
    DBuf<float4> qrec;
    DBuf<float> thrA;
    DBuf<int> ids, hint_m, hint_t, cnt, cands, cid, caux, fstatus, sticky;
    DBuf<uint8_t> keep, ddirs;
    DBuf<FitItem> items;
    DBuf<InstanceItem> inst_items;
    DBuf<InstanceGroup> inst_groups;
    {
      PackedCoeffs hc((size_t)B * r);
      std::vector<int> hi((size_t)B * km, 0);
      std::vector<double> ht((size_t)B * 3 * kt, 0.0);
      for (int b = 0; b < B; ++b) {
        hc.add(theta_init[b], r);
        if (uses_m[b]) std::memcpy(&hi[(size_t)b * km], params[b]->model_ids, sizeof(int) * params[b]->n_model_ids);
        if (uses_t[b]) std::memcpy(&ht[(size_t)b * 3 * kt], params[b]->target_points, sizeof(double) * 3 * params[b]->n_target_points);
      }
      NullStreamBatch _nb;
      hc.upload(coeffs);
      ids.upload(hi.data(), hi.size());
      tpts.upload(ht.data(), ht.size());
      ddirs.upload(dirs.data(), dirs.size());
      hint_m.alloc((size_t)B * km); hint_m.fill_bytes(0xFF);
      hint_t.alloc((size_t)B * kt); hint_t.fill_bytes(0xFF);
      sticky.alloc(B); sticky.fill_bytes(0);
      fstatus.alloc((size_t)B * 4); fstatus.fill_bytes(0);
    }
    x.alloc((size_t)B * 3 * N);
    Pm.alloc((size_t)B * 3 * km);
    qrec.alloc((size_t)B * kmpad); thrA.alloc((size_t)B * kmpad);
    thr2.alloc((size_t)B * ktpad);
    cnt.alloc((size_t)B * kpad);
    cands.alloc((size_t)B * cand);
    cid.alloc((size_t)B * kmax); caux.alloc((size_t)B * kmax); keep.alloc((size_t)B * kmax);
    pt.alloc((size_t)B * 3 * kmax); nhat.alloc((size_t)B * 3 * kmax); e.alloc((size_t)B * 3 * kmax);
    Mpart.alloc((size_t)B * Smax * nn);
    M.alloc((size_t)B * r * r); alpha.alloc((size_t)B * r);
    fscratch.alloc((size_t)B * fsz);
    // ---- the fits' records, and their instance records (the same for every recursion: the coefficient vector is the fit's in / out one)
    std::vector<FitItem> h_items(B);
    InstancePlan inst;
    FitGrid g{kpad, kmax, 1, 1};
    search_chains_hint(B);
    for (int b = 0; b < B; ++b) {
      icp_ctx& c = *ctxs[b];
      FitItem& f = h_items[b];
      f = FitItem{};
      f.dirs = ddirs.p + (size_t)b * R;
      f.coeffs = coeffs.p + (size_t)b * r;
      f.x = x.p + (size_t)b * 3 * N;
      inst.add(lead, f.coeffs, c.pose_of(theta_init[b]), f.x);
      f.ids = ids.p + (size_t)b * km;
      f.P = Pm.p + (size_t)b * 3 * km;
      f.tpts = tpts.p + (size_t)b * 3 * kt;
      if (uses_m[b]) {
        const int K = params[b]->n_model_ids;
        QueryBuffers qb{nullptr, qrec.p + (size_t)b * kmpad, thrA.p + (size_t)b * kmpad, cnt.p + (size_t)b * kpad, cands.p + (size_t)b * cand, cand};
        f.surf = make_surface_task(c.target.T, c.target.verts.p, c.target.tris.p, c.target.spheres.p, K, f.P, hint_m.p + (size_t)b * km, qb,
                                   nullptr, nullptr, nullptr);
        f.fblocks_m = filter_grid_blocks(f.surf.tblocks, f.surf.ksplit);
        f.splits_m = regression_splits(K);
        g.filter = std::max(g.filter, f.fblocks_m);
        g.splits = std::max(g.splits, f.splits_m);
      }
      if (uses_t[b]) {
        const int K = params[b]->n_target_points;
        QueryBuffers qb{thr2.p + (size_t)b * ktpad, nullptr, nullptr, cnt.p + (size_t)b * kpad, cands.p + (size_t)b * cand, cand};
        f.vert = make_vertex_task(N, f.x, K, f.tpts, hint_t.p + (size_t)b * kt, qb, nullptr, nullptr);
        f.fblocks_t = filter_grid_blocks(f.vert.vblocks, f.vert.ksplit);
        f.splits_t = regression_splits(K);
        g.filter = std::max(g.filter, f.fblocks_t);
        g.splits = std::max(g.splits, f.splits_t);
      }
      f.cb = CorrBuffers{cid.p + (size_t)b * kmax, caux.p + (size_t)b * kmax, pt.p + (size_t)b * 3 * kmax, keep.p + (size_t)b * kmax,
                         nhat.p + (size_t)b * 3 * kmax, e.p + (size_t)b * 3 * kmax};
      f.Mpart = Mpart.p + (size_t)b * Smax * nn;
      f.alpha = alpha.p + (size_t)b * r;
      f.factor_status = fstatus.p + (size_t)b * 4;
      f.status = sticky.p + b;
      f.step = params[b]->step_length;
    }
    search_chains_hint(1);
    {
      NullStreamBatch _nb;
      items.upload(h_items.data(), h_items.size());
      inst.upload(inst_items, inst_groups);
    }
    // ---- every recursion of every fit, enqueued up front
    const int fmax = posterior_factor_max();
    std::vector<PosteriorFactorIO> io(B);
    for (int si = 0; si < n_sigma; ++si) {
      const double wt = 1.0 / sigma2_seq[si];  // isotropic noise N(0, sigma2·I) (IcpBasedSurfaceFitting.scala:81)
      for (int it = 0; it <= n_iterations; ++it) {
        const int rec = si * (n_iterations + 1) + it;
        launch_instance_many(st, (int)inst.groups.size(), N, inst_groups.p, inst_items.p);
        launch_fit_searches(st, B, rec, g, N, lead.ref.p, lead.mean.p, items.p);
        launch_fit_regression(st, B, rec, g, r, lead.Q.p, wt, items.p);
        for (int b = 0; b < B; ++b) {
          const FitItem& f = h_items[b];
          io[b] = PosteriorFactorIO{f.Mpart, dirs[(size_t)b * R + rec] == ICP_MODEL_SAMPLING ? f.splits_m : f.splits_t, M.p + (size_t)b * r * r,
                                    f.alpha, f.factor_status, fscratch.p + (size_t)b * fsz};
        }
        for (int b0 = 0; b0 < B; b0 += fmax) launch_posterior_factor(st, r, std::min(fmax, B - b0), io.data() + b0);
        launch_fit_mean_step(st, B, r, lead.P.p, kSigma2, items.p);
      }
    }
    std::vector<double> hc((size_t)B * r);
    std::vector<int> hs(B);
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpy(hc.data(), coeffs.p, sizeof(double) * hc.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hs.data(), sticky.p, sizeof(int) * B, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
      const double* cb = &hc[(size_t)b * r];
      if (hs[b] != 0) { fit_status[b] = ICP_ERR_NOT_SPD; continue; }
      bool finite = true;
      for (int j = 0; j < r; ++j) finite = finite && std::isfinite(cb[j]);
      if (!finite) { fit_status[b] = ICP_ERR_NOT_FINITE; continue; }
      std::memmove(theta_out[b], theta_init[b], sizeof(double) * 10);
      std::memcpy(theta_out[b] + 10, cb, sizeof(double) * r);
    }
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_fits, fit_status, status, [](int code) {
    return code == ICP_ERR_NOT_SPD ? "regression normal equations are not positive definite" : "fitted coefficients are not finite";
  });
}

}  // extern "C"
