// abi_posterior_models.inl — C ABI: icp_posterior_models_many, the posterior shape models of many sets of given correspondences
// (kernels_posterior_model.hip; the resident factorisations and decompositions of kernels_factor.hip and kernels_eigen.hip).
//
// Item b: M = I + Σ Q_iᵀ Σ_i⁻¹ Q_i and b = Σ Q_iᵀ Σ_i⁻¹ (y_i − x̄_i − μ_i) over its observations, α = M⁻¹ b, D M⁻¹ D = V S Vᵀ, and from
// those the model (μ + Q·α, Φ·V, S).  The items go through kPmGroup slots of r-space scratch, a group at a time: one regression launch for
// the group, its factorisations (launch_posterior_factor) and decompositions (launch_posterior_eigen_many up to rank 64,
// launch_posterior_eigen_tridiag_many up to 256) rank by rank, every launch carrying all items of its rank; then the group's rows of
// Q·[D⁻¹V | α] pass through ONE chunk buffer of kPmChunkDoubles doubles, round by round, and go back to the caller from there.  No
// item's basis outlives its round.  Everything is enqueued on the first context's stream, host copies included, with ONE
// synchronisation per call (a second one only for an item whose spectrum the side-by-side decomposition could not separate: it is
// decomposed again on its own, as the chain does).  An item's bits depend neither on the other items, nor on their order, nor on
// how its rows fall into rounds.

namespace {
constexpr size_t kPmChunkDoubles = (size_t)ICP_POSTERIOR_MODELS_CHUNK_BYTES / sizeof(double);
constexpr int kPmGroup = ICP_POSTERIOR_MODELS_GROUP;  // items whose r-space work is in flight together
constexpr int kPmMaxRank = 256;                       // what the resident decompositions serve side by side
constexpr int kPmRowQuantum = 48;                     // rows of a piece: whole 16-row tiles and whole vertices
constexpr int kPmMaxPieces = 32768;                   // pieces per round (k_pm_gemm's grid.z stays below 65,536)

// Σ⁻¹ of a symmetric 3 × 3 covariance (its symmetric part) in closed form; false: not positive definite
bool pm_precision(const double* c, double* w) {
  const double a = c[0], b = 0.5 * (c[1] + c[3]), d = 0.5 * (c[2] + c[6]), e = c[4], f = 0.5 * (c[5] + c[7]), g = c[8];
  const double c00 = e * g - f * f, c01 = d * f - b * g, c02 = b * f - d * e;
  const double det = (a * c00 + b * c01) + d * c02;
  if (!(a > 0.0) || !(a * e - b * b > 0.0) || !(det > 0.0) || !std::isfinite(det)) return false;
  w[0] = c00 / det; w[1] = c01 / det; w[2] = c02 / det;
  w[3] = (a * g - d * d) / det; w[4] = (b * d - a * f) / det; w[5] = (a * e - b * b) / det;
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(w[i])) return false;
  return true;
}
}  // namespace

extern "C" {

int icp_posterior_models_many(int32_t n_items, icp_ctx* const* ctxs, const int32_t* n_obs, const int32_t* const* vertex_ids,
                              const double* const* points, const double* const* sigma2, const double* const* covariances,
                              double* const* alpha_out, double* const* mean_out, double* const* basis_out, double* const* variance_out,
                              double* const* point_variance_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(ctxs && n_obs && vertex_ids && points && status, "null argument");
    const int B = n_items;
    for (int b = 0; b < B; ++b) require(ctxs[b] && vertex_ids[b] && points[b], "null argument");
    require_one_device(B, ctxs, "items of one call share a device");
    // ---- validation: nothing runs and nothing is written unless every item's arguments are good.  The precisions are made here.
    std::vector<size_t> off(B + 1, 0);
    for (int b = 0; b < B; ++b) {
      require(n_obs[b] >= 1, "an item needs at least one observation");
      off[b + 1] = off[b] + (size_t)n_obs[b];
    }
    std::vector<double> h_w(6 * off[B]);
    std::vector<char> bad(B, 0);  // 1: the rank is not served; 2: a covariance is not positive definite
    for (int b = 0; b < B; ++b) {
      const icp_ctx& c = *ctxs[b];
      const int K = n_obs[b];
      const bool iso = sigma2 && sigma2[b], full = covariances && covariances[b];
      require(iso != full, "an item's noise is given as sigma2 or as covariances, one of the two");
      for (int k = 0; k < K; ++k) require(vertex_ids[b][k] >= 0 && vertex_ids[b][k] < c.N, "vertex id out of range");
      require_finite(points[b], 3 * (size_t)K, "points contain a non-finite value");
      double* w = &h_w[6 * off[b]];
      if (iso) {
        const double s2 = sigma2[b][0];
        require(std::isfinite(s2) && s2 > 0.0, "sigma2 must be finite and positive");
        const double wi = 1.0 / s2;
        for (int k = 0; k < K; ++k) { double* wk = w + 6 * (size_t)k; wk[0] = wk[3] = wk[5] = wi; wk[1] = wk[2] = wk[4] = 0.0; }
      } else {
        require_finite(covariances[b], 9 * (size_t)K, "covariances contain a non-finite value");
        for (int k = 0; k < K; ++k)
          if (!pm_precision(covariances[b] + 9 * (size_t)k, w + 6 * (size_t)k)) { bad[b] = 2; break; }
      }
      if (c.r > kPmMaxRank) bad[b] = 1;
    }
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    icp_ctx& lead = *ctxs[0];
    Bound _b(&lead);
    hipStream_t st = lead.stream;
    item_status.assign(B, ICP_OK);

    std::vector<int> live;
    int rmax = 1, smax = 1;
    for (int b = 0; b < B; ++b) {
      if (bad[b]) { item_status[b] = bad[b] == 1 ? ICP_ERR_INVALID_ARG : ICP_ERR_NOT_FINITE; continue; }
      live.push_back(b);
      rmax = std::max(rmax, ctxs[b]->r);
      smax = std::max(smax, regression_splits(n_obs[b]));
    }
    const int n_live = (int)live.size();
    auto fill_nan = [&](int b) {
      const icp_ctx& c = *ctxs[b];
      const size_t r = (size_t)c.r, N = (size_t)c.N;
      if (alpha_out && alpha_out[b]) std::fill(alpha_out[b], alpha_out[b] + r, (double)NAN);
      if (mean_out && mean_out[b]) std::fill(mean_out[b], mean_out[b] + 3 * N, (double)NAN);
      if (basis_out && basis_out[b]) std::fill(basis_out[b], basis_out[b] + 3 * N * r, (double)NAN);
      if (variance_out && variance_out[b]) std::fill(variance_out[b], variance_out[b] + r, (double)NAN);
      if (point_variance_out && point_variance_out[b]) std::fill(point_variance_out[b], point_variance_out[b] + N, (double)NAN);
    };
    if (n_live == 0) {
      for (int b = 0; b < B; ++b)
        if (bad[b] == 2) fill_nan(b);
      return;
    }
    // ---- the call's buffers: the observations; alpha, S and the status words of every live item; kPmGroup slots of r-space scratch; the chunk
    const size_t rr = (size_t)rmax * rmax, nn = (size_t)(rmax + 1) * (rmax + 1);
    const int ldb_max = (rmax + 1 + 15) / 16 * 16, rp_max = (rmax + 15) / 16 * 16;
    const int slots = std::min(kPmGroup, n_live);
    size_t work_max = 1;
    for (int b : live) work_max = std::max(work_max, eigen_work_doubles(ctxs[b]->r));
    const size_t fsz = (size_t)(rmax + 1) * rmax + 8;
    size_t cap = test_chunk_doubles("ICP_TEST_POSTERIOR_MODELS_CHUNK_DOUBLES", kPmChunkDoubles);
    for (int b : live) cap = std::max(cap, (size_t)kPmRowQuantum * ((size_t)ctxs[b]->r + 2));  // (a piece always fits)
    DBuf<int> d_ids, d_status;
    DBuf<double> d_pts, d_w, d_alpha, d_S, Mpart, M, V, Vt, Bm, fscratch, work, chunk;
    DBuf<PmItem> d_items;
    DBuf<PmPiece> d_pieces;
    {
      std::vector<int> h_ids(off[B]);
      std::vector<double> h_pts(3 * off[B]);
      for (int b = 0; b < B; ++b) {
        std::memcpy(&h_ids[off[b]], vertex_ids[b], sizeof(int) * (size_t)n_obs[b]);
        std::memcpy(&h_pts[3 * off[b]], points[b], sizeof(double) * 3 * (size_t)n_obs[b]);
      }
      NullStreamBatch _nb;
      d_ids.upload(h_ids.data(), h_ids.size());
      d_pts.upload(h_pts.data(), h_pts.size());
      d_w.upload(h_w.data(), h_w.size());
      d_status.alloc(4 * (size_t)n_live);  // per live item {factorisation, sweeps, decomposition, -}
      d_status.fill_bytes(0);
    }
    d_alpha.alloc((size_t)n_live * rmax);
    d_S.alloc((size_t)n_live * rmax);
    Mpart.alloc((size_t)slots * smax * nn);
    M.alloc(slots * rr); V.alloc(slots * rr); Vt.alloc(slots * rr);
    Bm.alloc((size_t)slots * rp_max * ldb_max);
    fscratch.alloc(slots * fsz);
    work.alloc(slots * work_max);
    chunk.alloc(cap);
    d_items.alloc(n_live);
    void* pinned_rec = nullptr;
    pinned_alloc(&pinned_rec, eigen_many_record_bytes(n_live));
    struct PinnedGuard { void* p; ~PinnedGuard() { pinned_free(p); } } _pg{pinned_rec};

    // ---- the items' records (slot = position in the group)
    std::vector<PmItem> h_items(n_live);
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q], s = q % slots;
      const icp_ctx& c = *ctxs[b];
      PmItem& it = h_items[q];
      it.K = n_obs[b]; it.splits = regression_splits(n_obs[b]); it.r = c.r; it.ldb = (c.r + 1 + 15) / 16 * 16;
      it.id = d_ids.p + off[b]; it.pt = d_pts.p + 3 * off[b]; it.W = d_w.p + 6 * off[b];
      it.Q = c.Q.p; it.ref = c.ref.p; it.mean = c.mean.p; it.inv_sqrt_lambda = c.inv_sqrt_lambda.p;
      it.Mpart = Mpart.p + (size_t)s * smax * nn;
      it.V = V.p + s * rr;
      it.alpha = d_alpha.p + (size_t)q * rmax;
      it.Bm = Bm.p + (size_t)s * rp_max * ldb_max;
    }
    {
      NullStreamBatch _nb;
      d_items.upload(h_items.data(), h_items.size());
    }
    auto wants_cols = [&](int b) { return (basis_out && basis_out[b]) || (point_variance_out && point_variance_out[b]); };
    auto wants_mean = [&](int b) { return mean_out && mean_out[b] != nullptr; };

    // ---- the plan of the rows: an item's rows are cut into pieces that fill the chunk buffer; a full buffer — or the end of a group, whose
    // slots the next group takes over — is a round (product, point variances, copies back).  Made before anything is launched: the
    // piece table is uploaded once.
    struct Back { double* dev; double* host; size_t n; };
    struct Round { size_t p0, p1; int rows_max, tiles_max; bool any_pv; std::vector<Back> back; };
    auto plan_group = [&](int q0, int q1, std::vector<PmPiece>& pcs, std::vector<Round>& rounds) {
      size_t used = 0;
      Round cur{pcs.size(), pcs.size(), 0, 0, false, {}};
      auto flush = [&] {
        cur.p1 = pcs.size();
        if (cur.p1 > cur.p0) rounds.push_back(std::move(cur));
        cur = Round{pcs.size(), pcs.size(), 0, 0, false, {}};
        used = 0;
      };
      for (int q = q0; q < q1; ++q) {
        const int b = live[q];
        const icp_ctx& c = *ctxs[b];
        const PmItem& it = h_items[q];
        const bool cols = wants_cols(b), mean = wants_mean(b), pv = point_variance_out && point_variance_out[b];
        if (!cols && !mean) continue;
        const int R = 3 * c.N, r = c.r;
        const size_t per_q = (size_t)kPmRowQuantum * ((cols ? r : 0) + (mean ? 1 : 0)) + (pv ? kPmRowQuantum / 3 : 0);
        for (int row0 = 0; row0 < R;) {
          if (cap - used < per_q || cur.p0 + kPmMaxPieces == pcs.size()) flush();
          const size_t fit = (cap - used) / per_q * kPmRowQuantum;
          const int rows = (int)std::min<size_t>(fit, (size_t)(R - row0));
          PmPiece pc{};
          pc.Q = c.Q.p; pc.Bm = it.Bm; pc.mu = c.mean.p; pc.S = d_S.p + (size_t)q * rmax;
          pc.r = r; pc.ldb = it.ldb; pc.row0 = row0; pc.rows = rows;
          pc.t0 = cols ? 0 : r / 16;
          double* p = chunk.p + used;
          if (cols) { pc.basis = p; p += (size_t)rows * r; }
          if (mean) { pc.mean = p; p += rows; }
          if (pv) { pc.pvar = p; p += rows / 3; }
          used = (size_t)(p - chunk.p);
          if (basis_out && basis_out[b]) cur.back.push_back(Back{pc.basis, basis_out[b] + (size_t)row0 * r, (size_t)rows * r});
          if (mean) cur.back.push_back(Back{pc.mean, mean_out[b] + row0, (size_t)rows});
          if (pv) cur.back.push_back(Back{pc.pvar, point_variance_out[b] + row0 / 3, (size_t)rows / 3});
          cur.rows_max = std::max(cur.rows_max, rows);
          cur.tiles_max = std::max(cur.tiles_max, it.ldb / 16 - pc.t0);
          cur.any_pv = cur.any_pv || pv;
          pcs.push_back(pc);
          row0 += rows;
        }
      }
      flush();
    };
    auto issue_rounds = [&](const std::vector<Round>& rounds, size_t r0, size_t r1, const PmPiece* table) {
      HostCopies cp;
      for (size_t i = r0; i < r1; ++i) {
        const Round& rd = rounds[i];
        launch_pm_gemm(st, (int)(rd.p1 - rd.p0), rd.rows_max, rd.tiles_max, table + rd.p0);
        if (rd.any_pv) launch_pm_point_variance(st, (int)(rd.p1 - rd.p0), rd.rows_max, table + rd.p0);
        for (const Back& k : rd.back) cp.add(k.dev, k.host, k.n);
        cp.issue(st, false);
      }
    };
    // the r-space work of items q0 .. q1-1 (one group).  alone: every decomposition by launch_posterior_eigen, which falls back to the
    // Jacobi iteration on the device where the multisection gives up.
    size_t rec_used = 0;
    EigenProblem* rec_base = (EigenProblem*)pinned_rec;
    auto run_rspace = [&](int q0, int q1, bool alone) {
      const int n = q1 - q0;
      int gr = 1, gs = 1;
      for (int q = q0; q < q1; ++q) { gr = std::max(gr, h_items[q].r); gs = std::max(gs, h_items[q].splits); }
      HIP_OK(hipMemsetAsync(work.p, 0, sizeof(double) * work_max * (size_t)std::min(n, slots), st));  // (the decompositions' progress words)
      launch_pm_regression(st, n, gs, gr, d_items.p + q0);
      std::vector<int> order(n);  // factorisations and decompositions, rank by rank
      for (int i = 0; i < n; ++i) order[i] = q0 + i;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return h_items[x].r < h_items[y].r; });
      const int fmax = posterior_factor_max();
      for (int i0 = 0; i0 < n;) {
        int i1 = i0;
        const int r = h_items[order[i0]].r;
        while (i1 < n && h_items[order[i1]].r == r) ++i1;
        std::vector<PosteriorFactorIO> io;
        std::vector<EigenRequest> rq;
        for (int i = i0; i < i1; ++i) {
          const int q = order[i], s = q % slots;
          const PmItem& it = h_items[q];
          int* stw = d_status.p + 4 * (size_t)q;
          io.push_back(PosteriorFactorIO{it.Mpart, it.splits, M.p + s * rr, d_alpha.p + (size_t)q * rmax, stw, fscratch.p + s * fsz});
          rq.push_back(EigenRequest{M.p + s * rr, nullptr, V.p + s * rr, Vt.p + s * rr, d_S.p + (size_t)q * rmax, work.p + s * work_max, stw + 2,
                                    nullptr, nullptr, nullptr, 0, ctxs[live[q]]->sqrt_lambda.p});
        }
        const int m = i1 - i0;
        for (int p0 = 0; p0 < m; p0 += fmax) launch_posterior_factor(st, r, std::min(fmax, m - p0), io.data() + p0);
        bool done = false;
        if (!alone) {
          if (eigen_tridiag_many_supported(r)) {
            launch_posterior_eigen_tridiag_many(st, r, m, rq.data(), nullptr);
            done = true;
          } else if (launch_posterior_eigen_many(st, r, m, rq.data(), rec_base + rec_used, nullptr) >= 0) {
            rec_used += (size_t)m;
            done = true;
          }
        }
        if (!done)
          for (const EigenRequest& e : rq) launch_posterior_eigen(st, r, e.M, e.sqrt_lambda, nullptr, e.V, e.Vt, e.S, e.work, e.status);
        i0 = i1;
      }
      launch_pm_operand(st, n, gr, d_items.p + q0);
    };

    // ---- every group, enqueued up front
    std::vector<PmPiece> h_pc;
    std::vector<Round> rounds;
    std::vector<size_t> group_rounds(1, 0);
    for (int q0 = 0; q0 < n_live; q0 += slots) {
      plan_group(q0, std::min(n_live, q0 + slots), h_pc, rounds);
      group_rounds.push_back(rounds.size());
    }
    {
      NullStreamBatch _nb;
      d_pieces.upload(h_pc.data(), h_pc.size());
    }
    for (int q0 = 0, g = 0; q0 < n_live; q0 += slots, ++g) {
      run_rspace(q0, std::min(n_live, q0 + slots), false);
      issue_rounds(rounds, group_rounds[g], group_rounds[g + 1], d_pieces.p);
    }
    std::vector<double> h_alpha((size_t)n_live * rmax), h_S((size_t)n_live * rmax);
    std::vector<int> h_st(4 * (size_t)n_live);
    auto fetch_small = [&] {
      HIP_OK(hipMemcpyAsync(h_alpha.data(), d_alpha.p, sizeof(double) * h_alpha.size(), hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_S.data(), d_S.p, sizeof(double) * h_S.size(), hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_st.data(), d_status.p, sizeof(int) * h_st.size(), hipMemcpyDeviceToHost, st));
      lead.finish(0, 0);
    };
    fetch_small();
    // (rare) a spectrum the side-by-side decomposition could not separate: that item again, on its own
    bool again = false;
    for (int q = 0; q < n_live; ++q) {
      if (h_st[4 * q] != 0 || h_st[4 * q + 2] == 0) continue;
      std::vector<PmPiece> pc1;
      std::vector<Round> rd1;
      plan_group(q, q + 1, pc1, rd1);
      DBuf<PmPiece> d_pc1;
      {
        NullStreamBatch _nb;
        d_pc1.upload(pc1.data(), pc1.size());
        HIP_OK(hipMemset(d_status.p + 4 * (size_t)q, 0, sizeof(int) * 4));
      }
      run_rspace(q, q + 1, true);
      issue_rounds(rd1, 0, rd1.size(), d_pc1.p);
      HIP_OK(hipStreamSynchronize(st));
      again = true;
    }
    if (again) fetch_small();
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q], r = ctxs[b]->r;
      if (h_st[4 * q] != 0 || h_st[4 * q + 2] != 0) { item_status[b] = ICP_ERR_NOT_FINITE; continue; }
      if (alpha_out && alpha_out[b]) std::memcpy(alpha_out[b], &h_alpha[(size_t)q * rmax], sizeof(double) * r);
      if (variance_out && variance_out[b]) std::memcpy(variance_out[b], &h_S[(size_t)q * rmax], sizeof(double) * r);
    }
    for (int b = 0; b < B; ++b)
      if (item_status[b] == ICP_ERR_NOT_FINITE) fill_nan(b);
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG ? "an item's rank is above 256: no resident decomposition serves it"
                                       : "an item's covariance is not positive definite, or its M did not factor";
  });
}

}  // extern "C"
