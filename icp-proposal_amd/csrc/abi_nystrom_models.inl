// abi_nystrom_models.inl — C ABI: icp_nystrom_models_many, Gaussian-process shape models by the Nyström approximation on sample points,
// many in one call (kernels_nystrom_model.hip).  Item b: K = k(S, S) on its n sample points, K = U·Λ·Uᵀ by a two-sided
// block Jacobi iteration on the device, and the model (λ/n, k(X, S)·u·√n/λ) on its mesh points.
//
// Every argument of every item is checked before the device is touched (live_items, then PoolCall's device and stream:
// abi_pool_many.inl).  The live items then go through the device kNysGroup at a
// time: ONE upload (points, samples, weights), the kernel matrices in one launch, and the iteration — three launches per round of the
// tournament, each carrying every item of the group, an item that has converged returning at once — with one synchronisation per sweep,
// in which the host reads ONE word: how many items still iterate.  Behind it the eigenvalues' order, the operands, and the rows of the
// bases through ONE chunk buffer, round by round (the pieces are RowPieces' of icp_round_plan.hpp).  An item's bits depend neither on the other items,
// nor on their order, nor on how its rows fall into rounds.

namespace {
constexpr int kNysGroup = 16;       // items whose matrices are resident together
constexpr int kNysRowQuantum = 48;  // rows of a piece: whole 16-row tiles and whole vertices
constexpr int kNysMaxPieces = 32768;

void nys_models_run(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_samples,
                    const double* const* samples, const int32_t* n_terms, const icp_kernel_term_general* const* terms,
                    const double* const* const* sample_weights, const int32_t* rank, const double* min_variance, double* const* variance_out,
                    double* const* basis_out, double* const* eigenvalues_out, double* const* eigenvectors_out, double* const* info_out,
                    std::vector<int>& item_status) {
  const int B = n_items;
  // ---- validation, item by item, before the device is touched
  const std::vector<int> live = live_items(B, item_status, [&](int b) {
    if (!points[b] || !samples[b] || !terms[b]) return false;
    const long long N = n_points[b], n = n_samples[b];
    if (N < 1 || 3 * N > (long long)INT32_MAX) return false;
    if (n < 1 || 3 * n > (long long)kNysMaxRows) return false;
    if (n_terms[b] < 1 || n_terms[b] > kGpmMaxTerms) return false;
    if (!(rank[b] >= 1 && rank[b] <= kNysMaxRank && (long long)rank[b] <= 3 * n)) return false;
    if (min_variance && !(min_variance[b] >= 0.0 && std::isfinite(min_variance[b]))) return false;
    double lattice = 0.0;
    for (long long i = 0; i < 3 * N; ++i) {
      if (!std::isfinite(points[b][i])) return false;
      lattice = std::max(lattice, std::fabs(points[b][i]));
    }
    for (long long i = 0; i < 3 * n; ++i) {
      if (!std::isfinite(samples[b][i])) return false;
      lattice = std::max(lattice, std::fabs(samples[b][i]));
    }
    for (int t = 0; t < n_terms[b]; ++t) {
      if (!gpm_term_good(terms[b][t], N, lattice)) return false;
      if (!terms[b][t].weights) continue;
      // a weighted term needs its region weights at the sample points as well
      const double* w = sample_weights && sample_weights[b] ? sample_weights[b][t] : nullptr;
      if (!w) return false;
      bool positive = false;
      for (long long i = 0; i < n; ++i) {
        if (!(std::isfinite(w[i]) && w[i] >= 0.0)) return false;
        positive = positive || w[i] > 0.0;
      }
      if (!positive) return false;
    }
    return true;
  });
  const int n_live = (int)live.size();
  if (n_live == 0) return;

  PoolCall call(device);
  hipStream_t st = call.st;

  int rank_max = 1;
  for (int b : live) rank_max = std::max(rank_max, (int)rank[b]);
  size_t cap = test_chunk_doubles("ICP_TEST_NYSTROM_MODELS_CHUNK_DOUBLES", kGpmChunkDoubles);
  cap = std::max(cap, (size_t)kNysRowQuantum * rank_max);  // (a piece always fits)
  DBuf<double> chunk;
  {
    NullStreamBatch _nb;
    chunk.alloc(cap);
  }

  for (int g0 = 0; g0 < n_live; g0 += kNysGroup) {
    const int G = std::min(kNysGroup, n_live - g0);
    // ---- the group's records and buffers
    std::vector<NysItem> h_items(G);
    std::vector<size_t> o_pts(G + 1, 0), o_smp(G + 1, 0), o_A(G + 1, 0), o_U(G + 1, 0), o_pairs(G + 1, 0), o_mass(G + 1, 0), o_lam(G + 1, 0),
        o_W(G + 1, 0), o_var(G + 1, 0), o_Uk(G + 1, 0);
    std::vector<size_t> o_w((size_t)G * kGpmMaxTerms, 0), o_sw((size_t)G * kGpmMaxTerms, 0);
    size_t n_w = 0;
    int n_max = 1, rp_max = 2 * kNysBlock, kp_max = 16;
    for (int q = 0; q < G; ++q) {
      const int b = live[g0 + q];
      NysItem& it = h_items[q];
      it = NysItem{};
      it.n = n_samples[b]; it.R = 3 * it.n;
      it.nb = cdiv(it.R, kNysBlock);
      it.nb += it.nb & 1;
      it.Rp = it.nb * kNysBlock;
      it.N = n_points[b]; it.rank = rank[b]; it.kp = (it.rank + 15) / 16 * 16;
      it.n_terms = n_terms[b];
      it.min_variance = min_variance ? min_variance[b] : 1e-8;
      for (int t = 0; t < it.n_terms; ++t) {
        if (!terms[b][t].weights) continue;
        o_w[(size_t)q * kGpmMaxTerms + t] = n_w;
        n_w += (size_t)it.N;
        o_sw[(size_t)q * kGpmMaxTerms + t] = n_w;
        n_w += (size_t)it.n;
      }
      const size_t np = (size_t)it.nb / 2;
      o_pts[q + 1] = o_pts[q] + 3 * (size_t)it.N;
      o_smp[q + 1] = o_smp[q] + (size_t)it.R;
      o_A[q + 1] = o_A[q] + (size_t)it.Rp * it.Rp;
      o_U[q + 1] = o_U[q] + np * 4 * kNysBlock * kNysBlock;
      o_pairs[q + 1] = o_pairs[q] + np;
      o_mass[q + 1] = o_mass[q] + (size_t)(it.nb - 1) * np;
      o_lam[q + 1] = o_lam[q] + (size_t)it.R;
      o_W[q + 1] = o_W[q] + (size_t)it.Rp * it.kp;
      o_var[q + 1] = o_var[q] + (size_t)it.rank;
      o_Uk[q + 1] = o_Uk[q] + (size_t)it.R * it.rank;
      n_max = std::max(n_max, it.n); rp_max = std::max(rp_max, it.Rp); kp_max = std::max(kp_max, it.kp);
    }
    DBuf<double> d_in, d_A, d_V, d_U, d_mass, d_norm, d_off, d_lam, d_W, d_var, d_Uk;
    DBuf<int> d_rot, d_state, d_order, d_active;
    DBuf<NysItem> d_items;
    {
      const size_t w0 = o_pts[G] + o_smp[G];
      std::vector<double> h_in(w0 + n_w);
      for (int q = 0; q < G; ++q) {
        const int b = live[g0 + q];
        std::memcpy(&h_in[o_pts[q]], points[b], sizeof(double) * (o_pts[q + 1] - o_pts[q]));
        std::memcpy(&h_in[o_pts[G] + o_smp[q]], samples[b], sizeof(double) * (o_smp[q + 1] - o_smp[q]));
        for (int t = 0; t < n_terms[b]; ++t) {
          if (!terms[b][t].weights) continue;
          std::memcpy(&h_in[w0 + o_w[(size_t)q * kGpmMaxTerms + t]], terms[b][t].weights, sizeof(double) * (size_t)n_points[b]);
          std::memcpy(&h_in[w0 + o_sw[(size_t)q * kGpmMaxTerms + t]], sample_weights[b][t], sizeof(double) * (size_t)n_samples[b]);
        }
      }
      NullStreamBatch _nb;
      d_in.upload(h_in.data(), h_in.size());
      d_A.alloc(o_A[G]); d_V.alloc(o_A[G]); d_U.alloc(o_U[G]);
      d_rot.alloc(o_pairs[G]); d_mass.alloc(o_mass[G]);
      d_norm.alloc(4 * (size_t)G); d_state.alloc(4 * (size_t)G); d_off.alloc(G);
      d_lam.alloc(o_lam[G]); d_order.alloc(o_lam[G]);
      d_W.alloc(o_W[G]); d_var.alloc(o_var[G]); d_Uk.alloc(o_Uk[G]);
      d_active.alloc(kNysMaxSweeps);
      d_active.fill_bytes(0);
      d_A.fill_bytes(0);  // (the padding of K, and V in front of its diagonal: a pooled buffer holds anything)
      d_V.fill_bytes(0);
      for (int q = 0; q < G; ++q) {
        const int b = live[g0 + q];
        NysItem& it = h_items[q];
        for (int t = 0; t < it.n_terms; ++t) {
          const icp_kernel_term_general& k = terms[b][t];
          it.terms[t] = gpm_term_record(k, k.weights ? d_in.p + w0 + o_w[(size_t)q * kGpmMaxTerms + t] : nullptr);
          if (k.weights) it.sw[t] = d_in.p + w0 + o_sw[(size_t)q * kGpmMaxTerms + t];
          it.general = it.general || !gpm_term_plain(k);
        }
        it.pts = d_in.p + o_pts[q]; it.smp = d_in.p + o_pts[G] + o_smp[q];
        it.A = d_A.p + o_A[q]; it.V = d_V.p + o_A[q]; it.U = d_U.p + o_U[q];
        it.rotated = d_rot.p + o_pairs[q]; it.mass = d_mass.p + o_mass[q];
        it.norm = d_norm.p + 4 * (size_t)q; it.state = d_state.p + 4 * (size_t)q; it.offmass = d_off.p + q;
        it.lam = d_lam.p + o_lam[q]; it.order = d_order.p + o_lam[q];
        it.W = d_W.p + o_W[q]; it.variance = d_var.p + o_var[q]; it.Uk = d_Uk.p + o_Uk[q];
      }
      d_items.upload(h_items.data(), h_items.size());
    }
    // ---- the kernel matrices and the iteration: one word read per sweep
    launch_nys_kernel_matrix(st, G, n_max, d_items.p);
    const int rounds = rp_max / kNysBlock - 1;
    for (int sweep = 0; sweep < kNysMaxSweeps; ++sweep) {
      for (int round = 0; round < rounds; ++round) launch_nys_round(st, G, rp_max, round, d_items.p);
      launch_nys_sweep_end(st, G, d_items.p, d_active.p + sweep);
      int active = 0;
      HIP_OK(hipMemcpyAsync(&active, d_active.p + sweep, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if (active == 0) break;
    }
    launch_nys_finish(st, G, rp_max, kp_max, d_items.p);
    std::vector<int> h_state(4 * (size_t)G);
    std::vector<double> h_norm(4 * (size_t)G), h_off(G);
    HIP_OK(hipMemcpyAsync(h_state.data(), d_state.p, sizeof(int) * h_state.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_norm.data(), d_norm.p, sizeof(double) * h_norm.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_off.data(), d_off.p, sizeof(double) * h_off.size(), hipMemcpyDeviceToHost, st));
    for (int q = 0; q < G; ++q) {
      const int b = live[g0 + q];
      const NysItem& it = h_items[q];
      if (variance_out && variance_out[b])
        HIP_OK(hipMemcpyAsync(variance_out[b], it.variance, sizeof(double) * (size_t)it.rank, hipMemcpyDeviceToHost, st));
      if (eigenvalues_out && eigenvalues_out[b])
        HIP_OK(hipMemcpyAsync(eigenvalues_out[b], it.lam, sizeof(double) * (size_t)it.R, hipMemcpyDeviceToHost, st));
      if (eigenvectors_out && eigenvectors_out[b])
        HIP_OK(hipMemcpyAsync(eigenvectors_out[b], it.Uk, sizeof(double) * (size_t)it.R * it.rank, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    for (int q = 0; q < G; ++q) {
      const int b = live[g0 + q];
      // past the cap the outputs are still written, from the iteration as it stands
      if (h_state[4 * q] == 0) item_status[b] = ICP_ERR_NOT_CONVERGED;
      if (!std::isfinite(h_off[q]) || !std::isfinite(h_norm[4 * q])) item_status[b] = ICP_ERR_NOT_FINITE;
      if (info_out && info_out[b]) {
        info_out[b][0] = (double)h_state[4 * q + 2]; info_out[b][1] = (double)h_state[4 * q + 1];
        info_out[b][2] = h_norm[4 * q + 1]; info_out[b][3] = h_off[q];
      }
    }
    // ---- the rows of the group's bases through the chunk buffer: pieces that fill it are a round (product, copies back, synchronisation)
    std::vector<NysPiece> pcs;
    DBuf<NysPiece> d_pcs;
    HostCopies back;
    int rows_max = 0, tiles_max = 0;
    RowPieces{cap, kNysRowQuantum, kNysMaxPieces}.cut(
        0, G,
        [&](int q) {
          const int b = live[g0 + q];
          return RowPieces::Item{3 * h_items[q].N, (size_t)h_items[q].rank, basis_out && basis_out[b]};
        },
        [&](int q, int row0, int rows, size_t at) {
          const NysItem& it = h_items[q];
          NysPiece pc{};
          pc.item = d_items.p + q; pc.row0 = row0; pc.rows = rows; pc.out = chunk.p + at;
          back.add(pc.out, basis_out[live[g0 + q]] + (size_t)row0 * it.rank, (size_t)rows * it.rank);
          rows_max = std::max(rows_max, rows);
          tiles_max = std::max(tiles_max, it.kp / 16);
          pcs.push_back(pc);
        },
        [&] {
          {
            NullStreamBatch _nb;
            d_pcs.upload(pcs.data(), pcs.size());
          }
          launch_nys_basis(st, (int)pcs.size(), rows_max, tiles_max, d_pcs.p);
          back.issue(st, false);
          HIP_OK(hipStreamSynchronize(st));
          pcs.clear();
          rows_max = 0; tiles_max = 0;
        });
  }
}
}  // namespace

extern "C" {

int icp_nystrom_models_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_samples,
                            const double* const* samples, const int32_t* n_terms, const icp_kernel_term_general* const* terms,
                            const double* const* const* sample_weights, const int32_t* rank, const double* min_variance,
                            double* const* variance_out, double* const* basis_out, double* const* sample_eigenvalues_out,
                            double* const* sample_eigenvectors_out, double* const* info_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_samples && samples && n_terms && terms && rank && status, "null argument");
    nys_models_run(n_items, device, n_points, points, n_samples, samples, n_terms, terms, sample_weights, rank, min_variance, variance_out,
                   basis_out, sample_eigenvalues_out, sample_eigenvectors_out, info_out, item_status);
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG
               ? "an item is outside the limits: 1 <= rank <= min(256, 3n), 3n <= 2400, min_variance >= 0, finite points and samples, the "
                 "terms' checks of icp_gp_models_general_many, and for every weighted term its weights at the sample points"
               : code == ICP_ERR_NOT_CONVERGED ? "the block Jacobi iteration of an item did not reach its stop level within the cap on sweeps"
                                               : "an item's kernel matrix is not finite";
  });
}

}  // extern "C"
