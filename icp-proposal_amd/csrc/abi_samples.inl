// abi_samples.inl — C ABI: icp_surface_samples_many, uniform surface samples of many meshes with the nearest vertex of every sample
// (Scalismo's UniformMeshSampler3D as IcpBasedSurfaceFitting.scala:51-53 and both CreateGPModel.scala draw from it), and
// icp_kernel_total_variance_many, the mean trace of a kernel at given points (apps/femur/CreateGPModel.scala:38-46).
// kernels_samples.hip; DESIGN.md §5.19.
//
// Every limit is checked for every item before the device is touched.  The items of icp_surface_samples_many go through ONE buffer in
// rounds of at most kSmpRoundWords 8-byte words (an item above that has a round of its own), in three regions: the inputs (ONE upload),
// the work arrays, the outputs (ONE copy back).  Per round: three launches for the integer weights and their prefix, one for the picks,
// and — only if an item of the round asks for vertex ids — one for the nearest vertices; no synchronisation between them.  Neither
// entry point takes a context: the live items, the device and the stream are abi_pool_many.inl's, the rounds and every item's place in
// their regions RegionRounds' (icp_round_plan.hpp), a term's device record gpm_term_record's.  An item's bits depend neither on the
// other items, nor on their order, nor on the rounds, nor on which outputs are asked for.

namespace {
constexpr size_t kSmpRoundWords = (size_t)ICP_SURFACE_SAMPLES_ROUND_BYTES / sizeof(double);
constexpr int kSmpMaxVertices = 1 << 24;
constexpr int kSmpMaxTriangles = 1 << 26;
constexpr int kSmpMaxSamples = 1 << 24;
constexpr double kSmpMaxMagnitude = 0x1p60;
constexpr int kTvMaxPoints = 1 << 24;

// where an item's arrays lie, in 8-byte words from the start of its part of the round's region: inputs, work arrays, outputs
struct SmpLayout {
  size_t words[3];                      // the regions' lengths: kPoolIn, kPoolWork, kPoolOut
  size_t pts, tris;                     // inputs
  size_t a2, tmax, C, tblk, tcnt, Q;    // work arrays
  size_t info, opts, ocells, obary, oids;  // outputs
  SmpLayout(size_t M, size_t T, size_t n) {
    const size_t tiles = (T + kScanTile - 1) / kScanTile;
    RegionCursor c;
    pts = c.take(24 * M); tris = c.take(12 * T);
    words[kPoolIn] = c.close();
    a2 = c.take(8 * T); tmax = c.take(8 * tiles); C = c.take(8 * T); tblk = c.take(8 * tiles); tcnt = c.take(4 * tiles); Q = c.take(8);
    words[kPoolWork] = c.close();
    info = c.take(32); opts = c.take(24 * n); ocells = c.take(4 * n); obary = c.take(24 * n); oids = c.take(4 * n);
    words[kPoolOut] = c.close();
  }
};
}  // namespace

extern "C" {

int icp_surface_samples_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_triangles,
                             const int32_t* const* cells, const int32_t* n_samples, const uint64_t* seeds, double* const* points_out,
                             int32_t* const* cells_out, double* const* bary_out, int32_t* const* vertex_ids_out, double* const* info_out,
                             int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_triangles && cells && n_samples && seeds && status, "null argument");
    require(points_out || cells_out || bary_out || vertex_ids_out || info_out, "null argument: at least one output");
    const int B = n_items;
    // ---- validation, item by item, before the device is touched
    const std::vector<int> live = live_items(B, item_status, [&](int b) {
      const long long M = n_points[b], T = n_triangles[b], n = n_samples[b];
      if (M < 1 || M > kSmpMaxVertices || T < 1 || T > kSmpMaxTriangles || n < 1 || n > kSmpMaxSamples) return false;
      if (!points[b] || !cells[b]) return false;
      return all_within(points[b], 3 * (size_t)M, kSmpMaxMagnitude) && ids_in_range(cells[b], 3 * (size_t)T, M);
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // ---- the plan: every item's layout; rounds = ranges of consecutive live items whose footprints fit the budget
    std::vector<SmpLayout> lay;
    lay.reserve(n_live);
    RegionRounds<3> plan(test_chunk_doubles("ICP_TEST_SAMPLES_CHUNK_DOUBLES", kSmpRoundWords), n_live);
    using Round = RegionRounds<3>::Round;
    for (int b : live) {
      lay.emplace_back((size_t)n_points[b], (size_t)n_triangles[b], (size_t)n_samples[b]);
      plan.add(lay.back().words);
    }
    DBuf<double> chunk;
    DBuf<SmpItem> d_items;
    std::vector<SmpItem> h_items(n_live);
    chunk.alloc(plan.buffer_words);
    for (const Round& rd : plan.rounds) {
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const SmpLayout& l = lay[q];
        SmpItem& it = h_items[q];
        it = SmpItem{};
        it.M = n_points[b]; it.T = n_triangles[b]; it.n = n_samples[b];
        it.tiles = (it.T + kScanTile - 1) / kScanTile;
        it.want_ids = vertex_ids_out && vertex_ids_out[b] ? 1 : 0;
        it.seed = seeds[b];
        const auto& at = plan.at[q];  // the item's parts, from the start of its round's regions
        double* ib = chunk.p + rd.base(kPoolIn) + at[kPoolIn];
        double* wb = chunk.p + rd.base(kPoolWork) + at[kPoolWork];
        double* ob = chunk.p + rd.base(kPoolOut) + at[kPoolOut];
        it.pts = ib + l.pts; it.tris = (const int*)(ib + l.tris);
        it.a2 = wb + l.a2; it.tmax = wb + l.tmax; it.C = (unsigned long long*)(wb + l.C); it.tblk = (unsigned long long*)(wb + l.tblk);
        it.tcnt = (int*)(wb + l.tcnt); it.Q = (unsigned long long*)(wb + l.Q);
        it.info = ob + l.info; it.opts = ob + l.opts; it.ocells = (int*)(ob + l.ocells); it.obary = ob + l.obary;
        it.oids = (int*)(ob + l.oids);
      }
    }
    {
      NullStreamBatch _nb;
      d_items.upload(h_items.data(), h_items.size());
    }
    std::vector<double> stage_in(plan.stage_words[kPoolIn]), stage_out(plan.stage_words[kPoolOut]);

    // ---- the rounds
    for (const Round& rd : plan.rounds) {
      const int n = rd.q1 - rd.q0;
      const SmpItem* items = d_items.p + rd.q0;
      int t_max = 0, n_max = 0, n_ids_max = 0;
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const SmpItem& it = h_items[q];
        const SmpLayout& l = lay[q];
        t_max = std::max(t_max, it.T); n_max = std::max(n_max, it.n);
        if (it.want_ids) n_ids_max = std::max(n_ids_max, it.n);
        double* blk = stage_in.data() + plan.at[q][kPoolIn];
        std::memcpy(blk + l.pts, points[b], sizeof(double) * 3 * (size_t)it.M);
        std::memcpy(blk + l.tris, cells[b], sizeof(int) * 3 * (size_t)it.T);
      }
      HIP_OK(hipMemcpyAsync(chunk.p, stage_in.data(), sizeof(double) * rd.words[kPoolIn], hipMemcpyHostToDevice, st));
      launch_smp_weights(st, n, t_max, items);
      launch_smp_pick(st, n, n_max, items);
      if (n_ids_max > 0) launch_smp_nearest(st, n, n_ids_max, items);
      HIP_OK(hipMemcpyAsync(stage_out.data(), chunk.p + rd.base(kPoolOut), sizeof(double) * rd.words[kPoolOut], hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      for (int q = rd.q0; q < rd.q1; ++q) {
        const int b = live[q];
        const SmpLayout& l = lay[q];
        const size_t ns = (size_t)h_items[q].n;
        const double* blk = stage_out.data() + plan.at[q][kPoolOut];
        double info[4];
        std::memcpy(info, blk + l.info, sizeof(info));
        if (!(info[0] >= 1.0)) item_status[b] = ICP_ERR_NOT_FINITE;  // no triangle has a weight: NaN and -1 are what the device wrote
        if (info_out && info_out[b]) std::memcpy(info_out[b], info, sizeof(info));
        if (points_out && points_out[b]) std::memcpy(points_out[b], blk + l.opts, sizeof(double) * 3 * ns);
        if (cells_out && cells_out[b]) std::memcpy(cells_out[b], blk + l.ocells, sizeof(int) * ns);
        if (bary_out && bary_out[b]) std::memcpy(bary_out[b], blk + l.obary, sizeof(double) * 3 * ns);
        if (vertex_ids_out && vertex_ids_out[b]) std::memcpy(vertex_ids_out[b], blk + l.oids, sizeof(int) * ns);
      }
    }
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int code) {
    return code == ICP_ERR_INVALID_ARG
               ? "an item is outside the limits: 1 <= n_points <= 2^24, 1 <= n_triangles <= 2^26 with ids in [0, n_points), "
                 "1 <= n_samples <= 2^24, finite coordinates with |x| <= 2^60"
               : "an item has no area: every triangle's weight is zero";
  });
}

int icp_kernel_total_variance_many(int32_t n_items, int device, const int32_t* n_points, const double* const* points, const int32_t* n_terms,
                                   const icp_kernel_term_general* const* terms, const double* const* const* point_weights,
                                   double* total_variance_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(n_points && points && n_terms && terms && total_variance_out && status, "null argument");
    const int B = n_items;
    // ---- validation, item by item, before the device is touched (a term's `weights` field is not read: the weights at these points
    // are point_weights[b][t])
    auto weights_of = [&](int b, int t) -> const double* { return point_weights && point_weights[b] ? point_weights[b][t] : nullptr; };
    const std::vector<int> live = live_items(B, item_status, [&](int b) {
      if (!points[b] || !terms[b]) return false;
      const long long n = n_points[b];
      if (n < 1 || n > kTvMaxPoints) return false;
      if (n_terms[b] < 1 || n_terms[b] > kGpmMaxTerms) return false;
      double lattice = 0.0;
      for (long long i = 0; i < 3 * n; ++i) {
        if (!std::isfinite(points[b][i])) return false;
        lattice = std::max(lattice, std::fabs(points[b][i]));
      }
      for (int t = 0; t < n_terms[b]; ++t) {
        icp_kernel_term_general k = terms[b][t];
        k.weights = weights_of(b, t);
        if (!gpm_term_good(k, n, lattice)) return false;
      }
      return true;
    });
    const int n_live = (int)live.size();
    if (n_live == 0) return;

    PoolCall call(device);
    hipStream_t st = call.st;

    // every item's points, then every term's weights, in ONE upload; the block sums and the results behind them in one buffer
    std::vector<size_t> off_p(n_live + 1, 0), off_s(n_live + 1, 0);
    std::vector<size_t> off_w((size_t)n_live * kGpmMaxTerms, 0);
    size_t n_w = 0;
    int n_max = 1;
    for (int q = 0; q < n_live; ++q) {
      const int b = live[q];
      off_p[q + 1] = off_p[q] + 3 * (size_t)n_points[b];
      off_s[q + 1] = off_s[q] + (size_t)cdiv(n_points[b], kTvBlock);
      n_max = std::max(n_max, (int)n_points[b]);
      for (int t = 0; t < n_terms[b]; ++t) {
        if (!weights_of(b, t)) continue;
        off_w[(size_t)q * kGpmMaxTerms + t] = n_w;
        n_w += (size_t)n_points[b];
      }
    }
    const size_t w0 = off_p[n_live];
    std::vector<double> h_in(w0 + n_w), h_out(n_live);
    std::vector<TvItem> h_items(n_live);
    DBuf<double> d_in, d_sum;
    DBuf<TvItem> d_items;
    {
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        std::memcpy(&h_in[off_p[q]], points[b], sizeof(double) * 3 * (size_t)n_points[b]);
        for (int t = 0; t < n_terms[b]; ++t)
          if (const double* w = weights_of(b, t)) std::memcpy(&h_in[w0 + off_w[(size_t)q * kGpmMaxTerms + t]], w, sizeof(double) * (size_t)n_points[b]);
      }
      NullStreamBatch _nb;
      d_in.upload(h_in.data(), h_in.size());
      d_sum.alloc(off_s[n_live] + (size_t)n_live);
      for (int q = 0; q < n_live; ++q) {
        const int b = live[q];
        TvItem& it = h_items[q];
        it = TvItem{};
        it.n = n_points[b]; it.n_terms = n_terms[b]; it.nblk = cdiv(it.n, kTvBlock);
        for (int t = 0; t < it.n_terms; ++t)
          it.terms[t] = gpm_term_record(terms[b][t], weights_of(b, t) ? d_in.p + w0 + off_w[(size_t)q * kGpmMaxTerms + t] : nullptr);
        it.pts = d_in.p + off_p[q];
        it.bsum = d_sum.p + off_s[q];
        it.out = d_sum.p + off_s[n_live] + q;
      }
      d_items.upload(h_items.data(), h_items.size());
    }
    launch_tv(st, n_live, n_max, d_items.p);
    HIP_OK(hipMemcpyAsync(h_out.data(), d_sum.p + off_s[n_live], sizeof(double) * (size_t)n_live, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int q = 0; q < n_live; ++q) total_variance_out[live[q]] = h_out[q];
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) {
    return "an item is outside the limits: 1 <= n_points <= 2^24, finite points, the terms' checks of icp_gp_models_general_many with "
           "the lattice range over these points, and weights (point_weights) that are finite, >= 0 and not all zero";
  });
}

}  // extern "C"
