// abi_projection_many.inl — C ABI: icp_model_instances_many and icp_model_coefficients_many, the model's instances, coefficients
// and projections of many meshes (kernels_projection.hip, launch_instance_many).
//
// Instances: points_out[b] is, bit for bit, icp_transformed_mesh(ctxs[b], thetas[b], ·).  Coefficients: item b's mesh — its uploaded
// vertices, or the instance of its state — has the given pose taken off, and c = P·Qᵀ(x − x̄ − μ) with the model's resident
// P = (QᵀQ + σ²I)⁻¹ (kSigma2); project_out[b] is the instance of c under that pose.  The meshes pass through ONE chunk buffer of
// kProjChunkDoubles doubles, chunk by chunk (coefficients: as many doubles again, rounded up to whole groups of 16 items, for the
// residuals in the matrix instruction's layout, and the slabs' partial sums, which take less than that); no mesh outlives its chunk.
// Everything is enqueued on the first context's stream, host copies included, with ONE synchronisation per call.  An item's bits
// depend neither on the other items, nor on their order, nor on the chunks.

namespace {
constexpr size_t kProjChunkDoubles = (size_t)4 << 20;  // the chunk buffer: 32 MiB of meshes
constexpr int kProjMaxChunkItems = 32752;              // meshes per chunk (a multiple of 16; k_proj_residual's grid.y = items stays below 65,536)

const double kProjIdentityPose[10] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
}  // namespace

extern "C" {

int icp_model_instances_many(int32_t n_items, icp_ctx* const* ctxs, const double* const* thetas, double* const* points_out) {
  return guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(ctxs && thetas && points_out, "null argument");
    const int B = n_items;
    for (int b = 0; b < B; ++b) require(ctxs[b] && thetas[b] && points_out[b], "null argument");
    require_one_device(B, ctxs, "items of one call share a device");
    size_t n_coeffs = 0;
    for (int b = 0; b < B; ++b) {
      require_finite(thetas[b], 10 + (size_t)ctxs[b]->r, "theta contains a non-finite value");
      n_coeffs += (size_t)ctxs[b]->r;
    }
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    icp_ctx& lead = *ctxs[0];
    Bound _b(&lead);
    hipStream_t st = lead.stream;

    size_t cap = test_chunk_doubles("ICP_TEST_PROJECTION_CHUNK_DOUBLES", kProjChunkDoubles);
    int Nmax = 1;
    for (int b = 0; b < B; ++b) {
      Nmax = std::max(Nmax, ctxs[b]->N);
      cap = std::max(cap, 3 * (size_t)ctxs[b]->N);  // (a mesh always fits)
    }
    size_t total = 0;
    for (int b = 0; b < B; ++b) total += 3 * (size_t)ctxs[b]->N;
    DBuf<double> chunk, coeffs;
    chunk.alloc(std::min(cap, total));
    {
      PackedCoeffs hc(n_coeffs);
      for (int b = 0; b < B; ++b) hc.add(thetas[b], ctxs[b]->r);
      hc.upload(coeffs);
    }
    // ---- the plan: a record per mesh, groups of up to kInstGroup consecutive meshes of one model, rounds = ranges of groups
    struct Round { size_t g0, g1; int b0, b1; };
    InstancePlan inst;
    const std::vector<InstanceItem>& h_smp = inst.items;
    const std::vector<InstanceGroup>& h_grp = inst.groups;
    std::vector<Round> rounds;
    {
      size_t used = 0, co = 0;
      int held = 0;
      rounds.push_back(Round{0, 0, 0, 0});
      for (int b = 0; b < B; ++b) {
        icp_ctx& c = *ctxs[b];
        const size_t n3 = 3 * (size_t)c.N;
        if (used + n3 > cap || held == kProjMaxChunkItems) {
          rounds.back().g1 = h_grp.size(); rounds.back().b1 = b;
          rounds.push_back(Round{h_grp.size(), 0, b, 0});
          used = 0; held = 0;
          inst.boundary();
        }
        inst.add(c, coeffs.p + co, c.pose_of(thetas[b]), chunk.p + used);
        co += (size_t)c.r; used += n3; ++held;
      }
      rounds.back().g1 = h_grp.size(); rounds.back().b1 = B;
    }
    DBuf<InstanceItem> d_smp;
    DBuf<InstanceGroup> d_grp;
    inst.upload(d_smp, d_grp);
    // ---- launches: one per round, and the round's meshes back to the caller
    HostCopies back;
    for (const Round& rd : rounds) {
      launch_instance_many(st, (int)(rd.g1 - rd.g0), Nmax, d_grp.p + rd.g0, d_smp.p);  // ModelFittingParameters.scala:108-110
      for (int b = rd.b0; b < rd.b1; ++b) back.add(h_smp[b].x, points_out[b], 3 * (size_t)ctxs[b]->N);
      back.issue(st, false);
    }
    lead.finish(0, 0);
  });
}

int icp_model_coefficients_many(int32_t n_items, icp_ctx* const* ctxs, const double* const* points, const double* const* thetas,
                                const double* const* poses, double* coeffs_out, double* const* project_out, int32_t* status) {
  std::vector<int> item_status;
  int rc = guard([&] {
    require(n_items >= 1 && n_items <= 65535, "n_items must lie in [1, 65535]");
    require(ctxs && coeffs_out && status, "null argument");
    const int B = n_items;
    for (int b = 0; b < B; ++b) require(ctxs[b] != nullptr, "null argument");
    icp_ctx& lead = *ctxs[0];
    require_one_model(B, ctxs, "items of one call share a device and a model");
    const int r = lead.r, N = lead.N;
    const size_t n3 = 3 * (size_t)N, P = 10 + (size_t)r;
    int n_theta = 0;
    for (int b = 0; b < B; ++b) {
      const bool has_pts = points && points[b], has_th = thetas && thetas[b];
      require(has_pts != has_th, "an item is given as points or as a theta, one of the two");
      if (has_th) {
        require_finite(thetas[b], P, "theta contains a non-finite value");
        ++n_theta;
      }
      if (poses && poses[b]) {
        require_finite(poses[b], 10, "pose contains a non-finite value");
        require(poses[b][0] == 1.0, "the scale of a pose to take off must be exactly 1");
      }
    }
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    lock_contexts(B, ctxs, locks);
    Bound _b(&lead);
    hipStream_t st = lead.stream;

    // ---- buffers: [meshes of a chunk | their residuals, 16 items side by side], the slabs' partial sums, the call's coefficient rows
    const size_t cap = test_chunk_doubles("ICP_TEST_PROJECTION_CHUNK_DOUBLES", kProjChunkDoubles);
    const int per_chunk = (int)std::min<size_t>({(size_t)B, std::max<size_t>(1, cap / n3), (size_t)kProjMaxChunkItems});
    const int groups = (per_chunk + kProjGroup - 1) / kProjGroup, rpad = (r + 15) / 16 * 16;
    DBuf<double> xbuf, dbuf, part, coeffs, tcoeffs;
    DBuf<int> nonfinite;
    xbuf.alloc((size_t)per_chunk * n3);
    dbuf.alloc((size_t)groups * kProjGroup * n3);
    part.alloc((size_t)groups * proj_slabs(N) * rpad * kProjGroup);
    coeffs.alloc((size_t)B * r);
    nonfinite.alloc(B);
    if (n_theta > 0) {
      PackedCoeffs hc((size_t)n_theta * r);
      for (int b = 0; b < B; ++b)
        if (thetas && thetas[b]) hc.add(thetas[b], r);
      hc.upload(tcoeffs);
    }
    // ---- records: a ProjItem per mesh; instance records of the states' meshes (first) and of the projections (second), in groups
    std::vector<ProjItem> h_item(B);
    InstancePlan inst;
    const std::vector<InstanceGroup>& h_grp = inst.groups;
    struct Chunk { int b0, b1; size_t tg0, tg1, pg0, pg1; };  // items; groups of the states' instances / of the projections
    std::vector<Chunk> chunks;
    {
      size_t to = 0;
      for (int b0 = 0; b0 < B; b0 += per_chunk) {
        Chunk ch{b0, std::min(B, b0 + per_chunk), h_grp.size(), 0, 0, 0};
        inst.boundary();
        for (int b = ch.b0; b < ch.b1; ++b) {
          double* x = xbuf.p + (size_t)(b - b0) * n3;
          ProjItem& it = h_item[b];
          it.x = x;
          it.has_pose = poses && poses[b] ? 1 : 0;
          it.pose = ctxs[b]->pose_of(it.has_pose ? poses[b] : kProjIdentityPose);
          if (thetas && thetas[b]) { inst.add(*ctxs[b], tcoeffs.p + to, ctxs[b]->pose_of(thetas[b]), x); to += r; }
        }
        ch.tg1 = ch.pg0 = h_grp.size();
        inst.boundary();
        for (int b = ch.b0; b < ch.b1; ++b)
          if (project_out && project_out[b]) inst.add(*ctxs[b], coeffs.p + (size_t)b * r, h_item[b].pose, const_cast<double*>(h_item[b].x));
        ch.pg1 = h_grp.size();
        chunks.push_back(ch);
      }
    }
    DBuf<ProjItem> d_item;
    DBuf<InstanceItem> d_smp;
    DBuf<InstanceGroup> d_grp;
    {
      NullStreamBatch _nb;
      d_item.upload(h_item.data(), h_item.size());
      if (!inst.items.empty()) inst.upload(d_smp, d_grp);
    }
    // ---- launches
    HIP_OK(hipMemsetAsync(nonfinite.p, 0, sizeof(int) * (size_t)B, st));
    HostCopies up, back;
    for (const Chunk& ch : chunks) {
      const int n = ch.b1 - ch.b0;
      for (int b = ch.b0; b < ch.b1; ++b)
        if (points && points[b]) up.add(const_cast<double*>(h_item[b].x), points[b], n3);
      up.issue(st, true);
      launch_instance_many(st, (int)(ch.tg1 - ch.tg0), N, d_grp.p + ch.tg0, d_smp.p);
      launch_proj_residual(st, n, N, lead.ref.p, lead.mean.p, d_item.p + ch.b0, dbuf.p, nonfinite.p + ch.b0);
      launch_proj_gemm(st, n, N, r, lead.Q.p, dbuf.p, part.p);
      launch_proj_solve(st, n, N, r, part.p, lead.P.p, coeffs.p + (size_t)ch.b0 * r);
      if (ch.pg1 > ch.pg0) {
        launch_instance_many(st, (int)(ch.pg1 - ch.pg0), N, d_grp.p + ch.pg0, d_smp.p);
        for (int b = ch.b0; b < ch.b1; ++b)
          if (project_out && project_out[b]) back.add(const_cast<double*>(h_item[b].x), project_out[b], n3);
        back.issue(st, false);
      }
    }
    std::vector<double> hc((size_t)B * r);
    std::vector<int> hn(B);
    HIP_OK(hipMemcpyAsync(hc.data(), coeffs.p, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hn.data(), nonfinite.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    lead.finish(0, 0);
    item_status.assign(B, ICP_OK);
    for (int b = 0; b < B; ++b) {
      if (hn[b] == 0) continue;
      item_status[b] = ICP_ERR_NOT_FINITE;
      std::fill(hc.begin() + (size_t)b * r, hc.begin() + (size_t)(b + 1) * r, (double)NAN);
      if (project_out && project_out[b]) std::fill(project_out[b], project_out[b] + n3, (double)NAN);
    }
    std::memcpy(coeffs_out, hc.data(), sizeof(double) * hc.size());
  });
  if (rc != ICP_OK) return rc;
  return report_item_status(n_items, item_status, status, [](int) { return "an item's mesh is not finite"; });
}

}  // extern "C"
