// abi_gp_models.inl — C ABI: icp_gp_models_many and icp_gp_models_general_many, Gaussian-process shape models of analytic kernels on
// many reference meshes (kernels_gp_model.hip; the resident decompositions of kernels_eigen.hip), and icp_region_weights_many, the
// smoothed region weights of the face kernel's terms.  Both model entry points reach gpm_models_run: icp_gp_models_many restates its
// terms as plain general ones (Gaussian, no weights, no mirror), and an item of plain terms runs the plain expressions.
//
// Item b: the pivoted Cholesky factor L of its kernel matrix, up to n_pivots columns (one launch per pivot step carries every item
// of the call), then LᵀL = W·Θ·Wᵀ and the model (Θ/N, √N·L·W·Θ^-1/2).  The host synchronises ONCE behind the pivot loop, to read how
// many columns every item made: that is the rank of its decomposition.  The m-space work (gpm_mspace_run, which icp_pca_models_many
// calls with its centred data matrices as the factors) then goes through kGpmGroup slots of scratch,
// a group at a time: the Gram matrices in one launch, the decompositions rank by rank (launch_posterior_eigen_many up to rank 64,
// launch_posterior_eigen_tridiag_many up to 256, launch_posterior_eigen for ranks 1 and 2 and for a spectrum the side-by-side route
// could not separate), one refinement step of the eigenvectors and the operands in a launch each, and the group's rows of L·Op through ONE chunk buffer, round by round, one
// synchronisation per round.  The decompositions see sqrt_lambda ≡ 1 and a Gram matrix scaled by an exact power of two (trace(K) brought
// into [1, 2)): magnitudes like a posterior's, and θ comes back exactly.  An item's bits depend neither on the other items, nor on
// their order, nor on how its rows fall into rounds.  The entry points take no context: the live items, the device and the stream are
// abi_pool_many.inl's, a term's device record is gpm_term_record's, and the rows are cut into pieces by RowPieces (icp_round_plan.hpp).

namespace {
constexpr size_t kGpmChunkDoubles = (size_t)ICP_GP_MODELS_CHUNK_BYTES / sizeof(double);
constexpr int kGpmGroup = 16;       // items whose m-space work is in flight together
constexpr int kGpmRowQuantum = 48;  // rows of a piece: whole 16-row tiles and whole vertices
constexpr int kGpmMaxPieces = 32768;

// exactly symmetric and positive semi-definite, by the principal minors of a 3 × 3 in closed form (a rounding's worth of slack:
// a rank-one A = v·vᵀ has minors that are zero up to rounding); not zero
bool gpm_psd(const double* A) {
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(A[i])) return false;
  if (A[1] != A[3] || A[2] != A[6] || A[5] != A[7]) return false;
  const double a = A[0], b = A[1], d = A[2], e = A[4], f = A[5], g = A[8];
  const double eps = 0x1p-48;
  if (a < 0.0 || e < 0.0 || g < 0.0 || !(a + e + g > 0.0)) return false;
  if (a * e - b * b < -eps * (a * e + b * b) || a * g - d * d < -eps * (a * g + d * d) || e * g - f * f < -eps * (e * g + f * f)) return false;
  const double det = (a * (e * g - f * f) - b * (b * g - d * f)) + d * (b * f - d * e);
  const double mag = (a * (e * g + f * f) + std::fabs(b) * (std::fabs(b) * g + std::fabs(d * f))) + std::fabs(d) * (std::fabs(b * f) + std::fabs(d) * e);
  return det >= -eps * mag;
}

// a term with icp_gp_models_many's meaning: Gaussian, no weights, no mirror
bool gpm_term_plain(const icp_kernel_term_general& k) { return k.kind == ICP_KERNEL_GAUSSIAN && !k.weights && k.mirror_gain == 0.0; }

// one term of item b on N points; `lattice` = the largest |coordinate| of the item
bool gpm_term_good(const icp_kernel_term_general& k, long long N, double lattice) {
  if (k.struct_size != (int32_t)sizeof(icp_kernel_term_general)) return false;
  if (!(std::isfinite(k.scale) && k.scale > 0.0) || !gpm_psd(k.A)) return false;
  if (k.kind == ICP_KERNEL_GAUSSIAN) {
    if (!(std::isfinite(k.sigma) && k.sigma > 0.0 && std::isfinite(k.sigma * k.sigma) && k.sigma * k.sigma > 0.0)) return false;
  } else if (k.kind == ICP_KERNEL_BSPLINE3) {
    if (k.level < -32 || k.level > 32) return false;
    if (!(std::ldexp(lattice, k.level) < 0x1p31)) return false;  // lattice indices are exact doubles
  } else {
    return false;
  }
  if (k.mirror_axis < 0 || k.mirror_axis > 2 || !(k.mirror_gain >= 0.0 && k.mirror_gain <= 1.0)) return false;
  if (k.mirror_gain > 0.0)
    for (int c = 0; c < 3; ++c)
      if (c != k.mirror_axis && (k.A[3 * k.mirror_axis + c] != 0.0 || k.A[3 * c + k.mirror_axis] != 0.0)) return false;
  if (k.weights) {
    bool positive = false;
    for (long long i = 0; i < N; ++i) {
      if (!(std::isfinite(k.weights[i]) && k.weights[i] >= 0.0)) return false;
      positive = positive || k.weights[i] > 0.0;
    }
    if (!positive) return false;
  }
  return true;
}

// one item of the m-space half: a column-major factor L ([me][R]) whose L·Lᵀ is the item's covariance
struct GpmFactor {
  int b;             // the caller's item: the index into the output arrays and item_status
  const double* L;   // device
  int R, me, rank;   // rows 3N; columns; eigenpairs asked for
  double trace;      // trace(LᵀL) > 0: the Gram matrix is multiplied by the power of two that brings it into [1, 2)
  double n_points;   // N
  double tau;        // rank_rule: eigenvalues θ <= tau do not count (k_pca_rank); unused otherwise
};

// the m-space half of icp_gp_models_many, icp_gp_models_general_many and icp_pca_models_many: LᵀL = W·Θ·Wᵀ and the model (Θ/N,
// √N·L·W·Θ^-1/2) of every factor, a group of kGpmGroup at a time; variance_out / basis_out / info_out[..][0..3] and the statuses of
// the items that fail.  rank_rule: the effective rank is decided on the device between the refinement and the operand
// (launch_pca_rank), and an item that keeps no component fails.
void gpm_mspace_run(hipStream_t st, const std::vector<GpmFactor>& f, bool rank_rule, double* const* variance_out, double* const* basis_out,
                    double* const* info_out, std::vector<int>& item_status);

// the body of both entry points, inside their guard.  general_entry: an item whose pivot loop leaves no column is that item's failure
// (icp_gp_models_general_many) instead of the call's.
void gpm_models_run(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_terms,
                    const icp_kernel_term_general* const* terms, const int32_t* n_pivots, const int32_t* rank, const double* rel_tolerance,
                    double* const* variance_out, double* const* basis_out, int32_t* const* pivots_out, double* const* residual_out,
                    double* const* info_out, std::vector<int>& item_status, bool general_entry) {
  {
    const int B = n_items;
    // ---- validation, item by item, before the device is touched
    std::vector<int> live = live_items(B, item_status, [&](int b) {
      if (!points[b] || !terms[b]) return false;
      const long long N = n_points[b];
      if (N < 1 || 3 * N > (long long)INT32_MAX) return false;
      if (n_terms[b] < 1 || n_terms[b] > kGpmMaxTerms) return false;
      if (!(rank[b] >= 1 && rank[b] <= n_pivots[b] && n_pivots[b] <= kGpmMaxPivots && (long long)n_pivots[b] <= 3 * N)) return false;
      if (rel_tolerance && !(rel_tolerance[b] >= 0.0 && rel_tolerance[b] < 1.0)) return false;
      double lattice = 0.0;
      for (long long i = 0; i < 3 * N; ++i) {
        if (!std::isfinite(points[b][i])) return false;
        lattice = std::max(lattice, std::fabs(points[b][i]));
      }
      for (int t = 0; t < n_terms[b]; ++t)
        if (!gpm_term_good(terms[b][t], N, lattice)) return false;
      return true;
    });
    int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // ---- the pivot loop: every item's points, d, L and partials; one record per item
    std::vector<GpmItem> h_items(n_live);
    std::vector<size_t> off_pts(n_live + 1, 0), off_L(n_live + 1, 0), off_part(n_live + 1, 0), off_piv(n_live + 1, 0);
    int nblk_max = 1, m_max = 1;
    // a weighted term's weights travel behind the points, in the same upload: term t of item q at off_w[q * kGpmMaxTerms + t]
    std::vector<size_t> off_w((size_t)n_live * kGpmMaxTerms, 0);
    size_t n_weights = 0;
    bool any_general = false;
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q], R = 3 * n_points[b], nblk = cdiv(R, kGpmBlockRows);
      for (int t = 0; t < n_terms[b]; ++t) {
        any_general = any_general || !gpm_term_plain(terms[b][t]);
        if (!terms[b][t].weights) continue;
        off_w[(size_t)q * kGpmMaxTerms + t] = n_weights;
        n_weights += (size_t)n_points[b];
      }
      off_pts[q + 1] = off_pts[q] + (size_t)R;
      off_L[q + 1] = off_L[q] + (size_t)R * n_pivots[b];
      off_part[q + 1] = off_part[q] + 2 * (size_t)nblk;
      off_piv[q + 1] = off_piv[q] + (size_t)n_pivots[b];
      nblk_max = std::max(nblk_max, nblk);
      m_max = std::max(m_max, (int)n_pivots[b]);
    }
    DBuf<double> d_pts, d_d, d_L, d_pmax, d_psum, d_start;
    DBuf<int> d_pidx, d_meff, d_piv;
    DBuf<GpmItem> d_items;
    {
      const size_t w0 = off_pts[n_live];
      std::vector<double> h_pts(w0 + n_weights);
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        std::memcpy(&h_pts[off_pts[q]], points[b], sizeof(double) * (off_pts[q + 1] - off_pts[q]));
        for (int t = 0; t < n_terms[b]; ++t)
          if (terms[b][t].weights)
            std::memcpy(&h_pts[w0 + off_w[(size_t)q * kGpmMaxTerms + t]], terms[b][t].weights, sizeof(double) * (size_t)n_points[b]);
      }
      NullStreamBatch _nb;
      d_pts.upload(h_pts.data(), h_pts.size());
      d_d.alloc(off_pts[n_live]);
      d_L.alloc(off_L[n_live]);
      d_pmax.alloc(off_part[n_live]); d_psum.alloc(off_part[n_live]); d_pidx.alloc(off_part[n_live]);
      d_start.alloc(2 * (size_t)n_live);
      d_meff.alloc(n_live);
      d_piv.alloc(off_piv[n_live]);
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        GpmItem& it = h_items[q];
        it.R = 3 * n_points[b]; it.m = n_pivots[b]; it.n_terms = n_terms[b]; it.nblk = cdiv(it.R, kGpmBlockRows);
        it.rel_tol = rel_tolerance ? rel_tolerance[b] : 0.0;
        for (int t = 0; t < kGpmMaxTerms; ++t) {
          it.terms[t] = GpmTerm{};
          if (t >= it.n_terms) continue;
          const icp_kernel_term_general& k = terms[b][t];
          it.terms[t] = gpm_term_record(k, k.weights ? d_pts.p + w0 + off_w[(size_t)q * kGpmMaxTerms + t] : nullptr);
          it.general = it.general || !gpm_term_plain(k);
        }
        it.pts = d_pts.p + off_pts[q]; it.d = d_d.p + off_pts[q]; it.L = d_L.p + off_L[q];
        it.pmax = d_pmax.p + off_part[q]; it.psum = d_psum.p + off_part[q]; it.pidx = d_pidx.p + off_part[q];
        it.start = d_start.p + 2 * (size_t)q; it.m_eff = d_meff.p + q; it.pivots = d_piv.p + off_piv[q];
      }
      d_items.upload(h_items.data(), h_items.size());
    }
    launch_gpm_init(st, n_live, nblk_max, d_items.p, any_general);
    for (int j = 0; j < m_max; ++j) launch_gpm_pivot_step(st, n_live, nblk_max, j, d_items.p, any_general);
    std::vector<int> h_meff(n_live), h_piv(off_piv[n_live]);
    std::vector<double> h_start(2 * (size_t)n_live);
    HIP_OK(hipMemcpyAsync(h_meff.data(), d_meff.p, sizeof(int) * h_meff.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_start.data(), d_start.p, sizeof(double) * h_start.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_piv.data(), d_piv.p, sizeof(int) * h_piv.size(), hipMemcpyDeviceToHost, st));
    for (int q = 0; q < n_live; ++q)
      if (residual_out && residual_out[live[q]])
        HIP_OK(hipMemcpyAsync(residual_out[live[q]], d_d.p + off_pts[q], sizeof(double) * (off_pts[q + 1] - off_pts[q]), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));  // the one synchronisation behind the loop: the effective pivot counts
    // plain terms: A ≠ 0 and a tolerance < 1 leave a column.  General terms can make trace(K) = 0 (a mirror gain of 1, weights that
    // vanish where A does not): such an item fails alone — NaN outputs, info zero — and takes no part in the m-space work
    std::vector<int> with_column;
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q];
      if (h_meff[q] > n_pivots[b] || (h_meff[q] < 1 && !general_entry)) fail(ICP_ERR_DEVICE, "the pivot loop left no column");
      if (pivots_out && pivots_out[b]) std::memcpy(pivots_out[b], &h_piv[off_piv[q]], sizeof(int) * (size_t)n_pivots[b]);
      if (h_meff[q] >= 1) {
        with_column.push_back(q);
        continue;
      }
      item_status[b] = ICP_ERR_NOT_FINITE;
      const size_t R = 3 * (size_t)n_points[b];
      if (variance_out && variance_out[b]) std::fill(variance_out[b], variance_out[b] + rank[b], (double)NAN);
      if (basis_out && basis_out[b]) std::fill(basis_out[b], basis_out[b] + R * rank[b], (double)NAN);
      if (residual_out && residual_out[b]) std::fill(residual_out[b], residual_out[b] + R, (double)NAN);
      if (info_out && info_out[b]) std::fill(info_out[b], info_out[b] + 4, 0.0);
    }
    if ((int)with_column.size() != n_live) {  // (the records behind the loop: start of L, columns made, trace)
      for (size_t i = 0; i < with_column.size(); ++i) {
        const int q = with_column[i];
        live[i] = live[q]; off_L[i] = off_L[q]; h_meff[i] = h_meff[q];
        h_start[2 * i] = h_start[2 * (size_t)q]; h_start[2 * i + 1] = h_start[2 * (size_t)q + 1];
      }
      n_live = (int)with_column.size();
      if (n_live == 0) return;
    }

    // ---- m-space (gpm_mspace_run, shared with icp_pca_models_many)
    std::vector<GpmFactor> factors(n_live);
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q];
      factors[q] = GpmFactor{b, d_L.p + off_L[q], 3 * n_points[b], h_meff[q], rank[b], h_start[2 * (size_t)q + 1], (double)n_points[b], 0.0};
    }
    gpm_mspace_run(st, factors, false, variance_out, basis_out, info_out, item_status);
  }
}

void gpm_mspace_run(hipStream_t st, const std::vector<GpmFactor>& f, bool rank_rule, double* const* variance_out, double* const* basis_out,
                    double* const* info_out, std::vector<int>& item_status) {
  const int n_live = (int)f.size();
  if (n_live == 0) return;
  // ---- m-space: kGpmGroup slots of scratch sized for the call's largest decomposition; the chunk
  int me_max = 1, rank_max = 1, slabs_max = 1;
  std::vector<GpmSpace> h_sp(n_live);
  for (int q = 0; q < n_live; ++q) {
    GpmSpace& s = h_sp[q];
    s.R = f[q].R; s.me = f[q].me; s.mp = (s.me + 15) / 16 * 16;
    s.slab_rows = gpm_slab_rows(s.R); s.slabs = cdiv(s.R, s.slab_rows);
    s.rank = f[q].rank; s.re = std::min(s.rank, s.me); s.ldb = (s.rank + 15) / 16 * 16;
    s.scale = std::ldexp(1.0, -std::ilogb(f[q].trace));
    s.n_points = f[q].n_points; s.tau = f[q].tau;
    s.L = f[q].L;
    me_max = std::max(me_max, s.me); rank_max = std::max(rank_max, s.rank); slabs_max = std::max(slabs_max, s.slabs);
  }
  const int slots = std::min(kGpmGroup, n_live);
  const int mp_max = (me_max + 15) / 16 * 16, ldb_max = (rank_max + 15) / 16 * 16;
  const size_t mm = (size_t)me_max * me_max;
  size_t work_max = 1;
  for (int q = 0; q < n_live; ++q) work_max = std::max(work_max, eigen_work_doubles(h_sp[q].me));
  size_t cap = test_chunk_doubles("ICP_TEST_GP_MODELS_CHUNK_DOUBLES", kGpmChunkDoubles);
  cap = std::max(cap, (size_t)kGpmRowQuantum * rank_max);  // (a piece always fits)
  DBuf<double> Gpart, G, V, Vt, S, T, Sm, Rm, E, lam, Op, work, ones, d_var, chunk;
  DBuf<int> d_status, d_order;
  DBuf<GpmSpace> d_sp;
  {
    NullStreamBatch _nb;
    Gpart.alloc((size_t)slots * slabs_max * mp_max * mp_max);
    G.alloc(slots * mm); V.alloc(slots * mm); Vt.alloc(slots * mm);
    S.alloc((size_t)slots * me_max); lam.alloc((size_t)slots * me_max); d_order.alloc((size_t)slots * me_max);
    T.alloc(slots * mm); Sm.alloc(slots * mm); Rm.alloc(slots * mm); E.alloc(slots * mm);
    Op.alloc((size_t)slots * mp_max * ldb_max);
    work.alloc(slots * work_max);
    d_var.alloc((size_t)n_live * rank_max);
    chunk.alloc(cap);
    std::vector<double> h_ones(kGpmMaxPivots, 1.0);
    ones.upload(h_ones.data(), h_ones.size());
    d_status.alloc(4 * (size_t)n_live);  // per item {-, sweeps, decomposition, -}
    d_status.fill_bytes(0);
    for (int q = 0; q < n_live; ++q) {
      const int s = q % slots;
      GpmSpace& sp = h_sp[q];
      sp.Gpart = Gpart.p + (size_t)s * slabs_max * mp_max * mp_max;
      sp.G = G.p + s * mm; sp.V = V.p + s * mm;
      sp.T = T.p + s * mm; sp.Sm = Sm.p + s * mm; sp.Rm = Rm.p + s * mm; sp.E = E.p + s * mm;
      sp.lam = lam.p + (size_t)s * me_max; sp.order = d_order.p + (size_t)s * me_max;
      sp.Op = Op.p + (size_t)s * mp_max * ldb_max;
      sp.variance = d_var.p + (size_t)q * rank_max;
    }
    d_sp.upload(h_sp.data(), h_sp.size());
  }
  void* pinned_rec = nullptr;
  pinned_alloc(&pinned_rec, eigen_many_record_bytes(n_live));
  struct PinnedGuard { void* p; ~PinnedGuard() { pinned_free(p); } } _pg{pinned_rec};
  size_t rec_used = 0;
  EigenProblem* rec_base = (EigenProblem*)pinned_rec;

  // the m-space work of items q0 .. q1-1 (one group).  alone: every decomposition by launch_posterior_eigen, which falls back to the
  // Jacobi iteration on the device where the multisection gives up.
  auto run_mspace = [&](int q0, int q1, bool alone) {
    const int n = q1 - q0;
    int gmp = 16, gldb = 16, gslabs = 1;
    for (int q = q0; q < q1; ++q) {
      gmp = std::max(gmp, h_sp[q].mp); gldb = std::max(gldb, h_sp[q].ldb); gslabs = std::max(gslabs, h_sp[q].slabs);
    }
    HIP_OK(hipMemsetAsync(work.p, 0, sizeof(double) * work_max * (size_t)std::min(n, slots), st));  // (the decompositions' progress words)
    launch_gpm_gram(st, n, gmp, gslabs, d_sp.p + q0);
    std::vector<int> order(n);  // decompositions, rank by rank
    for (int i = 0; i < n; ++i) order[i] = q0 + i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return h_sp[x].me < h_sp[y].me; });
    for (int i0 = 0; i0 < n;) {
      int i1 = i0;
      const int r = h_sp[order[i0]].me;
      while (i1 < n && h_sp[order[i1]].me == r) ++i1;
      std::vector<EigenRequest> rq;
      for (int i = i0; i < i1; ++i) {
        const int q = order[i], s = q % slots;
        rq.push_back(EigenRequest{G.p + s * mm, nullptr, V.p + s * mm, Vt.p + s * mm, S.p + (size_t)s * me_max, work.p + s * work_max,
                                  d_status.p + 4 * (size_t)q + 2, nullptr, nullptr, nullptr, 0, ones.p});
      }
      const int m = i1 - i0;
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
    launch_gpm_refine(st, n, gmp, d_sp.p + q0);
    if (rank_rule) launch_pca_rank(st, n, d_sp.p + q0);  // the effective rank, decided on the device: k_gpm_operand reads it
    launch_gpm_operand(st, n, gmp, gldb, d_sp.p + q0);
  };
  // the rows of the group's bases through the chunk buffer: pieces that fill it are a round (product, copies back, synchronisation)
  auto run_rounds = [&](int q0, int q1) {
    std::vector<GpmPiece> pcs;
    DBuf<GpmPiece> d_pcs;
    HostCopies back;
    int rows_max = 0, tiles_max = 0;
    RowPieces{cap, kGpmRowQuantum, kGpmMaxPieces}.cut(
        q0, q1,
        [&](int q) {
          const int b = f[q].b;
          return RowPieces::Item{h_sp[q].R, (size_t)h_sp[q].rank, basis_out && basis_out[b]};
        },
        [&](int q, int row0, int rows, size_t at) {
          const GpmSpace& sp = h_sp[q];
          GpmPiece pc{};
          pc.L = sp.L; pc.Op = sp.Op; pc.R = sp.R; pc.me = sp.me; pc.rank = sp.rank; pc.ldb = sp.ldb; pc.row0 = row0; pc.rows = rows;
          pc.out = chunk.p + at;
          back.add(pc.out, basis_out[f[q].b] + (size_t)row0 * sp.rank, (size_t)rows * sp.rank);
          rows_max = std::max(rows_max, rows);
          tiles_max = std::max(tiles_max, sp.ldb / 16);
          pcs.push_back(pc);
        },
        [&] {
          {
            NullStreamBatch _nb;
            d_pcs.upload(pcs.data(), pcs.size());
          }
          launch_gpm_gemm(st, (int)pcs.size(), rows_max, tiles_max, d_pcs.p);
          back.issue(st, false);
          HIP_OK(hipStreamSynchronize(st));
          pcs.clear();
          rows_max = 0; tiles_max = 0;
        });
  };

  std::vector<double> h_var((size_t)n_live * rank_max);
  std::vector<int> h_st(4 * (size_t)n_live);
  auto fetch_small = [&] {
    HIP_OK(hipMemcpyAsync(h_var.data(), d_var.p, sizeof(double) * h_var.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_st.data(), d_status.p, sizeof(int) * h_st.size(), hipMemcpyDeviceToHost, st));
    if (rank_rule) HIP_OK(hipMemcpyAsync(h_sp.data(), d_sp.p, sizeof(GpmSpace) * h_sp.size(), hipMemcpyDeviceToHost, st));  // (the records' re)
    HIP_OK(hipStreamSynchronize(st));
  };
  for (int q0 = 0; q0 < n_live; q0 += slots) {
    const int q1 = std::min(n_live, q0 + slots);
    run_mspace(q0, q1, false);
    run_rounds(q0, q1);
  }
  fetch_small();
  // a spectrum the side-by-side decomposition could not separate (equal eigenvalues: an isotropic kernel has them in threes): that
  // item again, on its own
  bool again = false;
  for (int q = 0; q < n_live; ++q) {
    if (h_st[4 * q + 2] == 0) continue;
    {
      NullStreamBatch _nb;
      HIP_OK(hipMemset(d_status.p + 4 * (size_t)q, 0, sizeof(int) * 4));
    }
    run_mspace(q, q + 1, true);
    run_rounds(q, q + 1);
    again = true;
  }
  if (again) fetch_small();
  for (int q = 0; q < n_live; ++q) {
    const int b = f[q].b;
    const GpmSpace& sp = h_sp[q];
    const double* var = &h_var[(size_t)q * rank_max];
    bool ok = h_st[4 * q + 2] == 0 && sp.re >= (rank_rule ? 1 : 0) && sp.re <= std::min(sp.rank, sp.me);
    for (int j = 0; ok && j < sp.re; ++j) ok = std::isfinite(var[j]) && var[j] > 0.0;
    if (!ok) {
      item_status[b] = ICP_ERR_NOT_FINITE;
      const size_t R = (size_t)sp.R;
      if (variance_out && variance_out[b]) std::fill(variance_out[b], variance_out[b] + sp.rank, (double)NAN);
      if (basis_out && basis_out[b]) std::fill(basis_out[b], basis_out[b] + R * sp.rank, (double)NAN);
      if (info_out && info_out[b]) std::fill(info_out[b], info_out[b] + 4, (double)NAN);
      continue;
    }
    if (variance_out && variance_out[b]) std::memcpy(variance_out[b], var, sizeof(double) * (size_t)sp.rank);
    if (info_out && info_out[b]) {
      double sum = 0.0;
      for (int j = 0; j < sp.re; ++j) sum += var[j];
      info_out[b][0] = (double)sp.me; info_out[b][1] = (double)sp.re;
      info_out[b][2] = f[q].trace / sp.n_points; info_out[b][3] = sum;
    }
  }
}
}  // namespace

extern "C" {

int icp_gp_models_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_terms,
                       const icp_kernel_term* const* terms, const int32_t* n_pivots, const int32_t* rank, const double* rel_tolerance,
                       double* const* variance_out, double* const* basis_out, int32_t* const* pivots_out, double* const* residual_out,
                       double* const* info_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_terms && terms && n_pivots && rank && status, "null argument");
    // the terms restated as plain general ones (an item without terms, or with a count outside the limits, keeps a null list: refused)
    std::vector<std::vector<icp_kernel_term_general>> restated(n_items);
    std::vector<const icp_kernel_term_general*> lists(n_items, nullptr);
    for (int b = 0; b < n_items; ++b) {
      if (!terms[b] || n_terms[b] < 1 || n_terms[b] > kGpmMaxTerms) continue;
      restated[b].resize(n_terms[b]);
      for (int t = 0; t < n_terms[b]; ++t) {
        icp_kernel_term_general& g = restated[b][t];
        g = icp_kernel_term_general{};
        g.struct_size = (int32_t)sizeof(icp_kernel_term_general);
        g.kind = ICP_KERNEL_GAUSSIAN;
        g.scale = terms[b][t].scale; g.sigma = terms[b][t].sigma;
        std::memcpy(g.A, terms[b][t].A, sizeof(g.A));
      }
      lists[b] = restated[b].data();
    }
    gpm_models_run(n_items, device, n_points, points, n_terms, lists.data(), n_pivots, rank, rel_tolerance, variance_out, basis_out, pivots_out,
                   residual_out, info_out, item_status, false);
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG ? "an item is outside the limits: 1 <= rank <= n_pivots <= min(256, 3N), 1..8 terms with scale > 0, sigma > 0 "
                                         "and a symmetric positive semi-definite A, finite points, 0 <= rel_tolerance < 1"
                                       : "the decomposition of an item's Gram matrix did not converge";
  });
}

int icp_gp_models_general_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_terms,
                               const icp_kernel_term_general* const* terms, const int32_t* n_pivots, const int32_t* rank,
                               const double* rel_tolerance, double* const* variance_out, double* const* basis_out, int32_t* const* pivots_out,
                               double* const* residual_out, double* const* info_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_terms && terms && n_pivots && rank && status, "null argument");
    gpm_models_run(n_items, device, n_points, points, n_terms, terms, n_pivots, rank, rel_tolerance, variance_out, basis_out, pivots_out,
                   residual_out, info_out, item_status, true);
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG
               ? "an item is outside the limits: those of icp_gp_models_many; struct_size; a kind of 0 or 1; a B-spline level in [-32, 32] with "
                 "|coordinate| * 2^level < 2^31; 0 <= mirror_gain <= 1, mirror_axis 0..2, an A that does not couple the mirror axis when the "
                 "gain is positive; weights finite, >= 0 and not all zero"
               : "an item's pivot loop left no column (trace K = 0), or the decomposition of its Gram matrix did not converge";
  });
}

int icp_region_weights_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_region,
                            const double* const* region_points, const double* stddev, double* const* weights_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_region && region_points && stddev && weights_out && status, "null argument");
    const std::vector<int> live = live_items(n_items, item_status, [&](int b) {
      if (!points[b] || !region_points[b] || !weights_out[b]) return false;
      const long long N = n_points[b], M = n_region[b];
      if (N < 1 || 3 * N > (long long)INT32_MAX || M < 1 || 3 * M > (long long)INT32_MAX) return false;
      if (!(std::isfinite(stddev[b]) && stddev[b] > 0.0 && std::isfinite(stddev[b] * stddev[b]) && stddev[b] * stddev[b] > 0.0)) return false;
      for (long long i = 0; i < 3 * N; ++i)
        if (!std::isfinite(points[b][i])) return false;
      for (long long i = 0; i < 3 * M; ++i)
        if (!std::isfinite(region_points[b][i])) return false;
      return true;
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;
    PoolCall call(device);
    hipStream_t st = call.st;
    // every item's points, then every item's region, in ONE upload; the weights come back as one copy per item
    std::vector<size_t> off_p(n_live + 1, 0), off_r(n_live + 1, 0), off_o(n_live + 1, 0);
    int n_max = 1;
    for (int q = 0; q < n_live; ++q) {
      off_p[q + 1] = off_p[q] + 3 * (size_t)n_points[live[q]];
      off_r[q + 1] = off_r[q] + 3 * (size_t)n_region[live[q]];
      off_o[q + 1] = off_o[q] + (size_t)n_points[live[q]];
      n_max = std::max(n_max, (int)n_points[live[q]]);
    }
    std::vector<double> h_in(off_p[n_live] + off_r[n_live]);
    std::vector<GpmRegion> h_items(n_live);
    DBuf<double> d_in, d_w;
    DBuf<GpmRegion> d_items;
    {
      for (int q = 0; q < n_live; ++q) {
        std::memcpy(&h_in[off_p[q]], points[live[q]], sizeof(double) * (off_p[q + 1] - off_p[q]));
        std::memcpy(&h_in[off_p[n_live] + off_r[q]], region_points[live[q]], sizeof(double) * (off_r[q + 1] - off_r[q]));
      }
      NullStreamBatch _nb;
      d_in.upload(h_in.data(), h_in.size());
      d_w.alloc(off_o[n_live]);
      for (int q = 0; q < n_live; ++q) {
        GpmRegion& it = h_items[q];
        it.pts = d_in.p + off_p[q]; it.reg = d_in.p + off_p[n_live] + off_r[q]; it.w = d_w.p + off_o[q];
        it.n = n_points[live[q]]; it.n_reg = n_region[live[q]];
        it.s2 = stddev[live[q]] * stddev[live[q]];
      }
      d_items.upload(h_items.data(), h_items.size());
    }
    launch_gpm_region_weights(st, n_live, n_max, d_items.p);
    for (int q = 0; q < n_live; ++q)
      HIP_OK(hipMemcpyAsync(weights_out[live[q]], d_w.p + off_o[q], sizeof(double) * (off_o[q + 1] - off_o[q]), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) {
    return "an item is outside the limits: n_points >= 1, n_region >= 1, stddev > 0, finite points";
  });
}

}  // extern "C"
