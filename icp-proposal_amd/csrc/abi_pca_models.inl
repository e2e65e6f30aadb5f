// abi_pca_models.inl — C ABI: icp_pca_models_many, PCA shape models of meshes in correspondence with generalised Procrustes alignment
// (kernels_pca_model.hip), many in one call.  Item b: working copies of its meshes out of a pool that is uploaded once; up to
// gpa_iterations rounds of alignment to the mean shape, four launches a round for every item of the call and no synchronisation
// between them (an item that has stopped returns from every later launch); the centring launch; ONE synchronisation (rounds run, the
// last RMS, the transforms, the mean shapes, the partials of trace G); then the m-space half of the GP models (gpm_mspace_run of
// abi_gp_models.inl) on the centred columns, with the rank decided on the device.  It takes no context: the live items, the device and
// the stream are abi_pool_many.inl's.  An item's bits depend neither on the other items, nor on their order, nor on how its rows fall
// into the chunk buffer.

namespace {
constexpr double kPcaDataFloor = 0x1p-80;  // (2⁻⁴⁰)²: see icp_proposal.h, "τ₀"
}

extern "C" {

int icp_pca_models_many(int32_t n_items, int device, int32_t n_pool, const int32_t* pool_points, const double* const* pool,
                        const int32_t* n_meshes, const int32_t* const* mesh_ids, const double* const* reference, const int32_t* rank,
                        const int32_t* gpa_iterations, const double* halt_distance, double* const* variance_out, double* const* basis_out,
                        double* const* mean_out, double* const* transforms_out, double* const* info_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_pool >= 1 && pool_points && pool && n_meshes && mesh_ids && rank && gpa_iterations && halt_distance && status, "null argument");
    const int B = n_items;
    // ---- validation, item by item, before the device is touched; a pool mesh is looked at once, when the first item names it
    std::vector<signed char> pool_good(n_pool, -1);  // -1: not looked at yet
    auto mesh_good = [&](int k) {
      if (pool_good[k] >= 0) return pool_good[k] == 1;
      bool ok = pool[k] && pool_points[k] >= 1 && 3 * (long long)pool_points[k] <= (long long)INT32_MAX;
      for (long long i = 0; ok && i < 3 * (long long)pool_points[k]; ++i) ok = std::isfinite(pool[k][i]);
      pool_good[k] = ok ? 1 : 0;
      return ok;
    };
    const std::vector<int> live = live_items(B, item_status, [&](int b) {
      const int n = n_meshes[b];
      if (n < 2 || n > kGpmMaxPivots || !mesh_ids[b]) return false;
      if (!(rank[b] >= 1 && rank[b] <= n - 1)) return false;
      if (gpa_iterations[b] < 0 || gpa_iterations[b] > kPcaMaxRounds) return false;
      if (!(std::isfinite(halt_distance[b]) && halt_distance[b] >= 0.0)) return false;
      for (int j = 0; j < n; ++j) {
        const int k = mesh_ids[b][j];
        if (k < 0 || k >= n_pool || !mesh_good(k)) return false;
        if (pool_points[k] != pool_points[mesh_ids[b][0]]) return false;
      }
      if (reference && reference[b])
        for (long long i = 0; i < 3 * (long long)pool_points[mesh_ids[b][0]]; ++i)
          if (!std::isfinite(reference[b][i])) return false;
      return true;
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // ---- the pool meshes a live item names, in ONE upload; every item's records
    std::vector<size_t> pool_off(n_pool, (size_t)-1);
    size_t pool_doubles = 0;
    std::vector<size_t> off_X(n_live + 1, 0), off_R(n_live + 1, 0), off_c(n_live + 1, 0), off_h(n_live + 1, 0), off_d(n_live + 1, 0),
        off_n(n_live + 1, 0);
    int n_max = 2, nblk_max = 1, nblkR_max = 1, rounds_max = 0;
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q], n = n_meshes[b], N = pool_points[mesh_ids[b][0]], R = 3 * N;
      for (int j = 0; j < n; ++j) {
        const int k = mesh_ids[b][j];
        if (pool_off[k] != (size_t)-1) continue;
        pool_off[k] = pool_doubles;
        pool_doubles += (size_t)R;
      }
      const int nblk = cdiv(N, kPcaBlock), nblkR = cdiv(R, kPcaBlock);
      off_X[q + 1] = off_X[q] + (size_t)n * R;
      off_R[q + 1] = off_R[q] + (size_t)R;
      off_c[q + 1] = off_c[q] + 3 * (size_t)(n + 1) * nblk;
      off_h[q + 1] = off_h[q] + 9 * (size_t)n * nblk;
      off_d[q + 1] = off_d[q] + (size_t)nblkR;
      off_n[q + 1] = off_n[q] + (size_t)n;
      n_max = std::max(n_max, n); nblk_max = std::max(nblk_max, nblk); nblkR_max = std::max(nblkR_max, nblkR);
      rounds_max = std::max(rounds_max, (int)gpa_iterations[b]);
    }
    DBuf<double> d_pool, d_X, d_mean, d_cpart, d_hpart, d_dpart, d_tpart, d_tf, d_state;
    DBuf<int> d_stop;
    DBuf<const double*> d_src;
    DBuf<PcaItem> d_items;
    std::vector<PcaItem> h_items(n_live);
    {
      std::vector<double> h_pool(pool_doubles);
      for (int k = 0; k < n_pool; ++k)
        if (pool_off[k] != (size_t)-1) std::memcpy(&h_pool[pool_off[k]], pool[k], sizeof(double) * 3 * (size_t)pool_points[k]);
      NullStreamBatch _nb;
      d_pool.upload(h_pool.data(), h_pool.size());
      d_X.alloc(off_X[n_live]); d_mean.alloc(off_R[n_live]);
      d_cpart.alloc(off_c[n_live]); d_hpart.alloc(off_h[n_live]);
      d_dpart.alloc(off_d[n_live]); d_tpart.alloc(2 * off_d[n_live]);
      d_tf.alloc(12 * off_n[n_live]);
      d_state.alloc(2 * (size_t)n_live); d_stop.alloc(n_live);
      d_dpart.fill_bytes(0); d_state.fill_bytes(0); d_stop.fill_bytes(0);
      std::vector<const double*> h_src(off_n[n_live]);
      d_src.alloc(h_src.size());
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        PcaItem& it = h_items[q];
        it.n = n_meshes[b]; it.N = pool_points[mesh_ids[b][0]]; it.R = 3 * it.N;
        it.nblk = cdiv(it.N, kPcaBlock); it.nblkR = cdiv(it.R, kPcaBlock);
        it.max_rounds = gpa_iterations[b]; it.halt = halt_distance[b];
        for (int j = 0; j < it.n; ++j) h_src[off_n[q] + j] = d_pool.p + pool_off[mesh_ids[b][j]];
        it.src = d_src.p + off_n[q];
        it.X = d_X.p + off_X[q]; it.mean = d_mean.p + off_R[q];
        it.cpart = d_cpart.p + off_c[q]; it.hpart = d_hpart.p + off_h[q];
        it.dpart = d_dpart.p + off_d[q]; it.tpart = d_tpart.p + 2 * off_d[q];
        it.tf = d_tf.p + 12 * off_n[q];
        it.state = d_state.p + 2 * (size_t)q; it.stop = d_stop.p + q;
      }
      HIP_OK(hipMemcpy(d_src.p, h_src.data(), sizeof(const double*) * h_src.size(), hipMemcpyHostToDevice));
      d_items.upload(h_items.data(), h_items.size());
    }

    // ---- alignment and centring: 1 + 4·(the call's largest gpa_iterations) + 1 launches, no synchronisation between them
    launch_pca_init(st, n_live, nblkR_max, d_items.p);
    for (int k = 0; k < rounds_max; ++k) launch_pca_round(st, n_live, n_max, nblk_max, nblkR_max, k, d_items.p);
    launch_pca_centre(st, n_live, nblkR_max, d_items.p);
    std::vector<double> h_state(2 * (size_t)n_live), h_tpart(2 * off_d[n_live]), h_tf(12 * off_n[n_live]);
    HIP_OK(hipMemcpyAsync(h_state.data(), d_state.p, sizeof(double) * h_state.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_tpart.data(), d_tpart.p, sizeof(double) * h_tpart.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_tf.data(), d_tf.p, sizeof(double) * h_tf.size(), hipMemcpyDeviceToHost, st));
    for (int q = 0; q < n_live; ++q)
      if (mean_out && mean_out[live[q]])
        HIP_OK(hipMemcpyAsync(mean_out[live[q]], d_mean.p + off_R[q], sizeof(double) * (size_t)h_items[q].R, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));  // the call's one synchronisation in front of the m-space half

    // ---- trace G (the partials in order), the thresholds, and the items whose meshes are all equal
    auto fail_item = [&](int q) {
      const int b = live[q];
      const PcaItem& it = h_items[q];
      item_status[b] = ICP_ERR_NOT_FINITE;
      if (variance_out && variance_out[b]) std::fill(variance_out[b], variance_out[b] + rank[b], (double)NAN);
      if (basis_out && basis_out[b]) std::fill(basis_out[b], basis_out[b] + (size_t)it.R * rank[b], (double)NAN);
      if (mean_out && mean_out[b]) std::fill(mean_out[b], mean_out[b] + it.R, (double)NAN);
      if (transforms_out && transforms_out[b]) std::fill(transforms_out[b], transforms_out[b] + 12 * (size_t)it.n, (double)NAN);
      if (info_out && info_out[b]) std::fill(info_out[b], info_out[b] + 8, (double)NAN);
    };
    std::vector<GpmFactor> factors;
    std::vector<int> factor_q;
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q];
      const PcaItem& it = h_items[q];
      double trace = 0.0, raw = 0.0;
      for (int k = 0; k < it.nblkR; ++k) {
        trace += h_tpart[2 * off_d[q] + k];
        raw += h_tpart[2 * off_d[q] + it.nblkR + k];
      }
      const double tau0 = kPcaDataFloor * raw / (double)(it.n - 1);
      if (!(std::isfinite(trace) && std::isfinite(raw) && trace > tau0)) {  // every eigenvalue is <= trace: no component is left
        fail_item(q);
        continue;
      }
      const double tau = std::max(tau0, ((double)it.R * (double)it.n * 0x1p-52) * trace);
      factors.push_back(GpmFactor{b, it.X, it.R, it.n, rank[b], trace, (double)it.N, tau});
      factor_q.push_back(q);
    }
    gpm_mspace_run(st, factors, true, variance_out, basis_out, info_out, item_status);
    for (size_t i = 0; i < factors.size(); ++i) {
      const int q = factor_q[i], b = live[q];
      if (item_status[b] != ICP_OK) {  // (gpm_mspace_run has filled variance, basis and info[0..3])
        fail_item(q);
        continue;
      }
      if (transforms_out && transforms_out[b]) std::memcpy(transforms_out[b], &h_tf[12 * off_n[q]], sizeof(double) * 12 * (size_t)h_items[q].n);
      if (info_out && info_out[b]) {
        info_out[b][4] = h_state[2 * (size_t)q]; info_out[b][5] = h_state[2 * (size_t)q + 1];
        info_out[b][6] = 0.0; info_out[b][7] = 0.0;
      }
    }
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG
               ? "an item is outside the limits: 2 <= n_meshes <= 256, mesh ids in the pool, one N >= 1 per item with 3N <= INT32_MAX, "
                 "1 <= rank <= n_meshes - 1, 0 <= gpa_iterations <= 32, halt_distance >= 0 and finite, finite points"
               : "an item's meshes are all equal (no component is left), or the decomposition of its Gram matrix did not converge";
  });
}

}  // extern "C"
